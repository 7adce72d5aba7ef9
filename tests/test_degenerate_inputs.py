"""The degenerate genomes of degenerate_inputs.py on the CPU: the reference
that test_gpu_degenerate.py compares the device with is pinned here, and the
cases are shown not to be empty work, from the oracle alone.

  * the oracle's SA, ISA, LCP and map.bin of every genome, of `sigma2` and of
    the whole size sweep equal a naive suffix sort restated here (sorted
    suffixes as byte strings, the common prefix of neighbours byte by byte,
    longSA::show's rules in numpy);
  * they equal the reference's own files (tests/golden/degen_*_index.sha256,
    tools/make_golden_degenerate.sh), the oracle's MAM / MUM / MEM triples of
    the junction reads equal the reference's, and its resolve + tag of the
    mosaic's pipeline pairs equals the reference's mapout lines after
    mappability_tag, which throws on every pair left out of them;
  * the host emulation of k_mam_sm (tools/sm_emu) equals the oracle on the
    mosaic junction reads at 40, 100 and 150 bases, as rows and as records,
    plain and packed words, without an out-of-range probe;
  * non-vacuity (measured values, all from the oracle):

      genome      N  longest LCP  overflow ranks
      unary     6002      2999       91.5 %
      period2   8002      3998       93.6 %
      selfrc    6002      3000       91.5 %
      period3x2 12004     2999       91.5 %
      twins     16004     8001       48.4 %
      rctwins   16004     4002       46.8 %
      nruns     7326       662       21.9 %
      tailrun   6004       299        1.5 %
      specks    23200       15        0
      mosaic    58454     1501       11.5 %   (260 text sequences, K = 7)

    mosaic: 23 directory cells of 256 positions hold two or more contig
    starts, one holds 44; three binned chromosomes have no unique 36-mer
    start; the junction reads (468 per length) with / without a MAM match:
    340 / 128 at 40 bases, 418 / 50 at 100, 426 / 42 at 150; MEM gives up to
    762 / 1 600 / 1 700 matches for one read; over the three lengths 564
    forward and 998 reverse-strand matches have their left map byte outside
    their contig, and 1 609 alignments start before or end past their contig;
    map.bin holds 4 968 zero bytes, 45 005 of 1..254 and 8 221 of 255; the
    pipeline's pairs at 40 / 100 bases: 512 / 507 the tagger takes (413 / 409
    with a key, 26 / 9 duplicates, 110 / 99 with a match on a speck or within
    a read of a contig end) and 38 / 43 it throws on.  The pure repeats: no
    MAM match for a read inside one, up to 3 000 (40 bases) and 6 000 (100)
    MEM matches for a read with one foreign base.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

import degenerate_inputs as D
import oracle as O
from conftest import gold, read_gz_lines

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools", "sm_emu"))


def _sha(b):
    return hashlib.sha256(b).hexdigest()


_ix = {}


def index_of(name):
    if name not in _ix:
        _ix[name] = O.Index(*O.text_from_contigs(D.genome(name)))
    return _ix[name]


# ---------------------------------------------------------------------------
# the naive index
# ---------------------------------------------------------------------------
def naive_index(T):
    """(SA, ISA, LCP) of the byte string T by sorting its suffixes: two
    suffixes compared as byte strings, 64 bytes and then twice as many at a
    time (no suffix is copied whole; '$' is unique, so two differ)"""
    import functools
    N = len(T)

    def cmp(a, b):
        h, step = 0, 64
        while True:
            x, y = T[a + h:a + h + step], T[b + h:b + h + step]
            if x != y:
                return -1 if x < y else 1
            h += step
            step *= 2
    sa = sorted(range(N), key=functools.cmp_to_key(cmp))
    isa = [0] * N
    for r, x in enumerate(sa):
        isa[x] = r
    lcp = [0] * N
    for r in range(1, N):
        x, y = sa[r - 1], sa[r]
        h, step = 0, 16
        while T[x + h:x + h + step] == T[y + h:y + h + step]:    # (ends: '$' is unique)
            h += step
            step *= 2
        while T[x + h] == T[y + h]:
            h += 1
        lcp[r] = h
    return np.array(sa, np.int64), np.array(isa, np.int64), np.array(lcp, np.int64)


def naive_map(isa, lcp, startpos, sizes):
    """map.bin past its header (longSA.cpp:628-688): per forward base i of a
    contig of S bases at sp, m = max(LCP[r], LCP[r + 1]) + 1 at the rank of
    sp + i (right) and of its mirror sp + 2 S - i (left); right = 0 when
    right + i >= S, left = 0 when left >= i; capped at 255"""
    m = np.maximum(lcp, np.append(lcp[1:], 0)) + 1
    out = []
    for c in range(0, len(startpos), 2):
        sp, S = int(startpos[c]), int(sizes[c])
        i = np.arange(S, dtype=np.int64)
        right, left = m[isa[sp + i]], m[isa[sp + 2 * S - i]]
        right = np.where(right + i >= S, 0, right)
        left = np.where(left >= i, 0, left)
        out.append(np.stack([np.minimum(left, 255), np.minimum(right, 255)], 1).reshape(-1))
    return np.concatenate(out).astype(np.uint8) if out else np.zeros(0, np.uint8)


def check_naive(oix, rcref=True):
    sa, isa, lcp = naive_index(oix.T[:oix.N].tobytes())
    assert np.array_equal(oix.SA.astype(np.int64), sa)
    assert np.array_equal(oix.ISA.astype(np.int64), isa)
    assert np.array_equal(oix.LCP.astype(np.int64), lcp)
    if rcref:
        assert np.array_equal(oix.mappability()[2:], naive_map(isa, lcp, oix.startpos, oix.sizes))


@pytest.mark.parametrize("name", D.NAMES)
def test_oracle_equals_naive_sort(name):
    check_naive(index_of(name))


def test_oracle_equals_naive_sort_forward_only():
    T, sp, sz, names = D.sigma2()
    assert sorted(set(T.tobytes())) == sorted(b"$a")
    check_naive(O.Index(T, sp, sz, names), rcref=False)


def test_oracle_equals_naive_sort_size_sweep():
    assert {n % 16 for n in D.SWEEP_N if n <= 80} == set(range(16))
    for N in D.SWEEP_N:
        T, sp, sz, names, rcref = D.sweep_text(N)
        assert len(T) == N and T[-1] == ord("$")
        check_naive(O.Index(T, sp, sz, names), rcref)


# ---------------------------------------------------------------------------
# the reference's own files and triples
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.NAMES)
def test_oracle_equals_reference_index(name):
    oix = index_of(name)
    sums = {l.split()[0]: (l.split()[1], int(l.split()[2]))
            for l in open(gold("degen_%s_index.sha256" % name))}
    N = oix.N
    assert (_sha(oix.T[:N].tobytes()), N) == sums["rc1.ref.seq.bin"]
    assert (_sha(oix.SA.astype(np.uint32).tobytes()), 4 * N) == sums["rc1.i4.index.sa.bin"]
    assert (_sha(oix.ISA.astype(np.uint32).tobytes()), 4 * N) == sums["rc1.i4.index.isa.bin"]
    assert (_sha(oix.L8.tobytes()), N) == sums["rc1.i4.index.lcp.vec.bin"]
    assert (_sha(oix.ovf.tobytes()), 16 * len(oix.ovf)) == sums["rc1.i4.index.lcp.m.bin:masked"]
    mp = oix.mappability()
    assert (_sha(mp[2:].tobytes()), len(mp)) == sums["map.bin[2:]"]


def golden_triples(name, L, mode):
    """{read index: [(ref, q, len)]} of one of the reference's files"""
    out = {}
    for l in read_gz_lines("degen_%s_%d_%s.txt.gz" % (name, L, mode)):
        f = l.split()
        assert int(f[1]) == len(f) - 2
        out[int(f[0])] = [tuple(map(int, x.split(","))) for x in f[2:]]
    return out


@pytest.mark.parametrize("mode", ["MAM", "MUM", "MEM"])
@pytest.mark.parametrize("name,L", D.GOLDEN_READS)
def test_oracle_equals_reference_triples(name, L, mode):
    oix = index_of(name)
    reads = D.junction_reads(oix, L)
    exp = golden_triples(name, L, mode)
    assert len(exp) == len(reads) if mode != "MEM" else 0 < len(exp) <= len(reads)
    for r, e in exp.items():
        assert oix.search(reads[r].tobytes(), mode) == e, (r, bytes(reads[r]))


def _pairs(L):
    oix = index_of("mosaic")
    mapbin = oix.mappability()
    return (oix, mapbin) + D.pipeline_reads(D.genome("mosaic"), oix, mapbin, L)


@pytest.mark.parametrize("L", D.PIPE_LENGTHS)
def test_oracle_tagging_equals_reference_mapout(L):
    """resolve + tag of the mosaic's pipeline pairs against the lines of the
    reference's mummer -samout and mappability_tag: contigs shorter than a
    read, than min_len and than K + 2, major-named specks, map bytes read from
    a neighbouring contig or past the map"""
    from test_oracle_golden import _expected_lines
    oix, mapbin, reads, _ = _pairs(L)
    want = sorted("\t".join(x for x in l.split("\t") if not x.startswith("XO:Z:"))
                  for l in read_gz_lines("degen_mosaic_pairs_%d_mapout_tagged.txt.gz" % L))
    offsets = np.cumsum([0] + [int(x) for x in oix.sizes[0::2]][:-1]).astype(np.uint32)
    small = [1 if ("_gl000" in n or "chrM" in n) else 0 for n in oix.contigs]
    got = []
    for q in range(reads.shape[0] // 2):
        got += _expected_lines(oix, "r%09d" % q, (reads[2 * q].tobytes(), reads[2 * q + 1].tobytes()),
                               mapbin, offsets, small)
    got.sort()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b
    short = {n for n, s in zip(oix.contigs, oix.sizes[0::2]) if int(s) <= 60}
    assert sum(1 for l in want if l.split("\t")[2] in short and "\tL0:i:" in l) >= 50


@pytest.mark.parametrize("L", D.PIPE_LENGTHS)
def test_oracle_tag_errors_equal_reference(L):
    """every pair left out of the pipeline's reads makes the reference's
    mappability_tag throw, and the oracle's pipeline returns that error"""
    oix, mapbin, _, bad = _pairs(L)
    g = D.genome("mosaic")
    rows = [l.split() for l in open(gold("degen_mosaic_pairs_%d_tag_errors.txt" % L))]
    assert len(rows) == bad.shape[0] // 2 > 0
    for q, row in enumerate(rows):
        assert int(row[0]) == q and int(row[1]) != 0 and row[3:6] == ["mappability", "too", "big"], row
        op = O.Pipeline(oix, mapbin, D.chrom_sizes(g), D.bin_starts(g))
        assert op.run(np.ascontiguousarray(bad[2 * q:2 * q + 2])) == {"left": 1, "right": 2}[row[2]], row


# ---------------------------------------------------------------------------
# non-vacuity
# ---------------------------------------------------------------------------
def test_repeat_families_overflow_the_lcp_bytes():
    for name in D.REPEAT_FAMILIES + ("mosaic",):
        oix = index_of(name)
        print("%-10s N %6d longest LCP %5d overflow ranks %5.1f %%"
              % (name, oix.N, int(oix.LCP.max()), 100.0 * len(oix.ovf) / oix.N))
        assert int(oix.LCP.max()) >= 255 and len(oix.ovf) > 0, name
    for name in ("unary", "period2", "selfrc", "period3x2"):
        assert len(index_of(name).ovf) > 0.9 * index_of(name).N      # n_a stays near N
    assert len(index_of("specks").ovf) == 0 and int(index_of("specks").LCP.max()) < 255
    T = index_of("tailrun").T
    N = index_of("tailrun").N
    assert T[N - 301:N].tobytes() == b"a" * 300 + b"$"
    assert index_of("one").N == 4 and index_of("two").N == 10


@pytest.fixture(scope="module")
def mosaic():
    oix = index_of("mosaic")
    oix.accel()
    return oix


def test_mosaic_text(mosaic):
    oix = mosaic
    assert oix.N <= 60000 and len(oix.startpos) >= 250 and oix.acc.K >= 5
    cells = np.bincount(np.asarray(oix.startpos, np.int64) >> 8)   # pipeline.hip sp_cell
    print("cells with >= 2 starts:", int((cells >= 2).sum()), "most:", int(cells.max()))
    assert (cells >= 2).sum() > 10 and cells.max() >= 8
    sizes = [int(s) for s in oix.sizes[0::2]]
    B = oix.acc.B
    small = [n for n, s in zip(oix.contigs, sizes) if "_gl000" in n]
    assert len(small) >= 100 and max(s for n, s in zip(oix.contigs, sizes) if "_gl000" in n) <= 60
    major = [s for n, s in zip(oix.contigs, sizes) if "_" not in n and s <= 60]
    assert any(s < B for s in major) and any(B <= s < 20 for s in major) and any(s >= 20 for s in major)
    mp = oix.mappability()[2:]
    n0, n255 = int((mp == 0).sum()), int((mp == 255).sum())
    print("map bytes: 0:", n0, "1..254:", len(mp) - n0 - n255, "255:", n255)
    assert n0 > 0 and n255 > 0 and len(mp) - n0 - n255 > 0
    # a chromosome without one unique start: every right byte 0 or 255
    right = mp[1::2]
    uniq, g = [], 0
    for s in sizes:
        uniq.append(int(((right[g:g + s] >= 1) & (right[g:g + s] <= 36)).sum()))
        g += s
    assert sum(1 for n, u in zip(oix.contigs, uniq) if "_" not in n and u == 0) >= 2


def test_mosaic_junction_reads(mosaic):
    oix = mosaic
    fwd = rev = over = 0
    for L in (40, 100, 150):
        reads = D.junction_reads(oix, L)
        assert reads.shape[0] <= 500
        ms = [oix.search(r.tobytes()) for r in reads]
        hit = sum(1 for m in ms if m)
        mem = max(len(oix.search(r.tobytes(), "MEM")) for r in reads)
        print("L %d: %d reads, %d with a MAM match, %d without; most MEM matches %d"
              % (L, len(reads), hit, len(reads) - hit, mem))
        assert hit >= 0.5 * len(reads) and len(reads) - hit >= 30
        assert mem > 500
        for r, m in zip(reads, ms):
            for rc, left_out, hang in D.alignments(oix, r, m):
                fwd += left_out and not rc
                rev += left_out and rc
                over += hang
    print("left byte outside the contig: %d forward, %d reverse; overhanging alignments %d"
          % (fwd, rev, over))
    assert fwd >= 20 and rev >= 20 and over >= 20


def test_pure_repeats_have_no_mam_match():
    """a read inside a pure repeat has no almost-unique match: these genomes
    test the builder and MEM's counts, not the MAM search"""
    for name in D.PURE_REPEATS:
        oix = index_of(name)
        for L in (40, 100):
            reads = D.junction_reads(oix, L)
            mid = [r for r in reads if b"`" not in r.tobytes() and b"$" not in r.tobytes()]
            assert len(mid) >= 2
            assert all(oix.search(r.tobytes()) == [] for r in mid), name
            # (MEM wants a differing base on the left: a read that is all run
            # has one match per length; one with a foreign base has thousands)
            assert max(len(oix.search(r.tobytes(), "MEM")) for r in reads) > 1000, name


def test_mosaic_pipeline_pairs(mosaic):
    import geometry_inputs as G
    oix = mosaic
    g = D.genome("mosaic")
    mapbin = oix.mappability()
    for L in D.PIPE_LENGTHS:
        reads, bad = D.pipeline_reads(g, oix, mapbin, L)
        ch = G.Chain(oix, reads, mapbin=mapbin)
        keys = sum(k is not None for k in ch.keys)
        dups = sum(1 for k, kp in zip(ch.keys, ch.keep) if k is not None and not kp)
        # mates that overlap a speck contig or a contig end
        sp = np.asarray(oix.startpos, np.int64)
        edge = 0
        for q in range(len(ch.keys)):
            near = False
            for m in ch.matches[2 * q] + ch.matches[2 * q + 1]:
                si = int(np.searchsorted(sp, m[0], side="right")) - 1
                o, S = m[0] - int(sp[si]), int(oix.sizes[si])
                near = near or S <= 60 or o < L or o + m[2] > S - L
            edge += near
        print("L %d: %d error-free pairs (%d with a key, %d duplicates, %d at a speck or a "
              "contig end), %d pairs with tag errors" % (L, len(ch.keys), keys, dups, edge,
                                                         bad.shape[0] // 2))
        assert ch.tag_errors == 0 and keys >= 300 and dups >= 5 and edge >= 50
        assert bad.shape[0] >= 2


# ---------------------------------------------------------------------------
# the emulator of the search kernel, before anything goes to a device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("direct", ["1", "0"])
@pytest.mark.parametrize("L", [40, 100, 150])
def test_emulator_on_mosaic_junction_reads(mosaic, L, direct, monkeypatch):
    import sm_emu
    monkeypatch.setenv("SMASH_SM_DIRECT", direct)
    oix = mosaic
    reads = D.junction_reads(oix, L)
    B = oix.acc.B
    for emu in (sm_emu.Emu(oix), sm_emu.Emu(oix, packed=True)):
        for ml, lin in ((20, 8), (20, 1), (B + 2, 8), (B, 2)):
            got, _ = emu.map(reads, min_len=ml, lin_blocks=lin)      # (asserts every probe in range)
            for i in range(len(reads)):
                assert got[i] == oix.search(reads[i].tobytes(), min_len=ml), (emu.packed, ml, lin, i)


@pytest.mark.parametrize("name", ("specks", "nruns", "tailrun") + D.PURE_REPEATS)
def test_emulator_on_the_other_genomes(name):
    """the genomes test_gpu_degenerate.py searches besides the mosaic"""
    import sm_emu
    oix = index_of(name)
    oix.accel()
    for L in (40, 100, 150):
        reads = D.junction_reads(oix, L)
        for emu in (sm_emu.Emu(oix), sm_emu.Emu(oix, packed=True)):
            for ml, lin in ((20, 8), (oix.acc.B + 2, 1)):
                got, _ = emu.map(reads, min_len=ml, lin_blocks=lin)
                for i in range(len(reads)):
                    assert got[i] == oix.search(reads[i].tobytes(), min_len=ml), (emu.packed, ml, lin, i)
