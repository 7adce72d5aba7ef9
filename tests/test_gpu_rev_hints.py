"""The reverse-strand map hint on the device: k_mam_sm stores each match when
its (B) chain scan ends and writes the chain hint into bits 33..39 of the
match word; mate_fast takes a reverse-strand alignment's right map.bin byte
from it (csrc/mam_sm.hpp A_CHAIN_DONE, csrc/pipeline.hip).

On the tiny, the mid and a two-contig edge genome (8-byte packed words: the
generic packed kernel; fixed 150 / 100 bases as native rows and dense, and
mates of mixed lengths) with the inputs of test_sm_emu_hints.py:
  * counts, stats and every pair's hit list are the same with SMASH_MAP_HINT=1
    and 0, the counts and totals are the oracle pipeline's, and the hit lists
    the oracle's search -> resolve -> tag -> smash_pair;
  * the match words of the device run equal the emulator's, hints included.
On the hg19-shaped index (the GEO 150 and GEO 100 kernels: packed words, native
rows, hints on): the same comparison between hints on and off, and every hint
of the device's words against the device's own map.bin (which
test_gpu_configs.py pins to the reference's).
"""
import gc
import os
import sys

import numpy as np
import pytest

from conftest import gold, interleaved_reads, load_bins, load_chrom_sizes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402
import oracle as O  # noqa: E402
import synth  # noqa: E402
import rev_hint_inputs as R  # noqa: E402
import varlen_util as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "sm_emu"))
import sm_emu  # noqa: E402


def _idx8(T, sp, sz, names):
    old = os.environ.get("SMASH_IDX_BYTES")
    os.environ["SMASH_IDX_BYTES"] = "8"
    try:
        dix = S.Index.create(T, sp, sz, names)
    finally:
        if old is None:
            del os.environ["SMASH_IDX_BYTES"]
        else:
            os.environ["SMASH_IDX_BYTES"] = old
    assert dix.info.idx_bytes == 8 and dix.info.pos_bits == R.POS_BITS
    return dix


class Subject:
    """an oracle index with its emulator and map.bin, the device's packed
    index of the same text, and the chromosome offsets and bins of a run"""

    def __init__(self, oix, cs, starts):
        oix.accel()
        self.oix, self.cs, self.starts = oix, cs, np.ascontiguousarray(starts, np.int64)
        self.dix = _idx8(oix.T[:oix.N], oix.startpos, oix.sizes, oix.names)
        self.emu = sm_emu.Emu(oix, packed=True)
        self.chk = R.HintCheck(oix)
        self.mapbin = oix.mappability()
        fwd = [int(x) for x in oix.sizes[0::2]]
        self.offs = np.cumsum([0] + fwd[:-1]).astype(np.uint32)
        self.small = [1 if ("_gl000" in c or "chrM" in c) else 0 for c in oix.contigs]

    def oracle_keys(self, mates):
        """per pair: the kept hits [(tid, pos)] or None; its tag errors"""
        keys, errs = [], []
        for q in range(len(mates) // 2):
            hs, err = [], 0
            for P in mates[2 * q:2 * q + 2]:
                h, _ = self.oix.resolve(P, self.oix.search(P, min_len=R.MIN_LEN))
                for x in h:
                    err += 1 if O.tag(x, self.offs, self.mapbin, self.small[x.tid]) else 0
                hs.append(h)
            keys.append(O.smash_pair(hs[0], hs[1]))
            errs.append(err)
        return keys, errs

    def device(self, rows, L, n, hints, monkeypatch, native, var_len=False):
        monkeypatch.setenv("SMASH_MAP_HINT", "1" if hints else "0")
        pipe = S.Pipeline(self.dix, self.cs, self.starts, L, n, dedup_capacity=n,
                          read_stride=S.read_stride(L) if native else 0, var_len=var_len)
        assert pipe.map_hints == hints
        return _count(pipe, rows, n, len(self.starts))


def _count(pipe, rows, n, nbins):
    counts = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    pipe.reset()
    d = rows if hasattr(rows, "data_ptr") else torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    pipe.count_batch(d, n, counts)
    st = pipe.stats()
    assert st.error == 0
    words, nw = pipe.peek_matches(n)
    return counts.cpu().numpy().astype(np.uint64), st.as_dict(), pipe.peek(n), (words, nw)


def _same_run(a, b):
    """counts, stats, every pair's hit list"""
    (c1, s1, (nk1, keep1, h1), _), (c2, s2, (nk2, keep2, h2), _) = a, b
    assert np.array_equal(c1, c2) and s1 == s2
    assert np.array_equal(nk1, nk2) and np.array_equal(keep1, keep2)
    for q in np.nonzero(nk1 > 0)[0]:
        assert np.array_equal(h1[q, :nk1[q]], h2[q, :nk1[q]]), q


@pytest.fixture(scope="module")
def tiny(tiny_ix):
    return Subject(tiny_ix, load_chrom_sizes(gold("tiny_chrom_sizes.txt")),
                   load_bins(gold("tiny_bins.txt"))[1])


def _synthetic_subject(g, tmp):
    bins_path = str(tmp / "bins.txt")
    synth.make_bins(g, 4, bins_path)
    synth.write_index_side_files(str(tmp), g)
    cs = {l.split("\t")[0]: int(l.split("\t")[2]) for l in open(tmp / "chrom_sizes.txt")}
    starts = np.array([int(l.split("\t")[2]) for l in open(bins_path)], np.int64)
    return Subject(O.Index(*O.text_from_contigs(g)), cs, starts)


@pytest.fixture(scope="module")
def mid(tmp_path_factory):
    g = synth.make_genome("mid")
    s = _synthetic_subject(g, tmp_path_factory.mktemp("mid"))
    s.g = g
    return s


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    return _synthetic_subject(R.edge_genome(), tmp_path_factory.mktemp("edge"))


def _inputs(name, s, L):
    if name == "tiny":
        parts = [interleaved_reads("s%d" % L)[:600], R.hand_reads(s.oix, L)]
    elif name == "mid":
        parts = [R.synth_reads(s.g, 250, L, seed=91 + L), R.hand_reads(s.oix, L)]
    else:
        parts = [R.edge_genome_reads(s.oix, L)]
    if L == 150 and name != "edge":
        parts.append(R.edge_reads_150(s.oix))
    reads = np.concatenate(parts)
    if reads.shape[0] & 1:
        reads = np.concatenate([reads, reads[-1:]])
    # a short match between foreign bytes can be shorter than its map bytes:
    # mappability_tag throws on it (mappability_tag.cpp:104-110) and the whole
    # run is an error, in the reference, the oracle and the pipeline alike.
    # The pairs the oracle tags without an error go through the pipeline
    # (the edge genome's hand-placed reads lie on contigs it exempts)
    keys, errs = s.oracle_keys([reads[r].tobytes() for r in range(reads.shape[0])])
    ok = [q for q, e in enumerate(errs) if e == 0]
    assert len(ok) >= 0.5 * len(errs)
    rows = np.array([2 * q + m for q in ok for m in (0, 1)])
    return np.ascontiguousarray(reads[rows], np.uint8), [keys[q] for q in ok]


def _check_fixed(s, inputs, L, native, monkeypatch):
    reads, keys = inputs
    n = reads.shape[0] // 2
    rows = np.zeros((2 * n, S.read_stride(L) if native else L), np.uint8)
    rows[:, :L] = reads
    on = s.device(rows, L, n, True, monkeypatch, native)
    off = s.device(rows, L, n, False, monkeypatch, native)
    _same_run(on, off)
    # the oracle pipeline: counts and totals; the per-pair hit lists
    op = O.Pipeline(s.oix, s.mapbin, s.cs, s.starts)
    assert op.run(reads, threads=4) == 0
    counts, st, (nk, keep, hits), (words, nw) = on
    assert np.array_equal(counts, op.counts)
    assert (st["positions"], st["dups"], st["kept"]) == (op.state.total, op.state.dups,
                                                         op.state.kept)
    assert st["dupe_pairs"] == op.n_dupe.value
    _check_keys(keys, nk, hits)
    _check_words(s, reads, None, L, on[3], off[3])


def _check_keys(keys, nk, hits):
    for q, exp in enumerate(keys):
        if exp is None:
            assert nk[q] == -1, q
            continue
        got = [(int(w >> 48), int(w & 0xFFFFFFFFFFFF)) for w in hits[q, :max(nk[q], 0)]]
        assert got == exp, (q, got, exp)


def _check_words(s, reads, lens, L, on, off):
    """the device's match words == the emulator's, with hints and without;
    and the hints' own check (HintCheck) on the device's words"""
    slots = L - R.MIN_LEN + 1
    for hints, (words, nw) in ((True, on), (False, off)):
        s.emu.map(reads, min_len=R.MIN_LEN, cap=slots, lens=lens, hints=hints)
        for r in range(reads.shape[0]):
            k = min(int(nw[r]), slots)
            assert k == len(s.emu.words[r]), (hints, r)
            assert np.array_equal(words[r, :k], s.emu.words[r]), (hints, r)
            if hints:
                for w in words[r, :k]:
                    s.chk.word(w)
    assert s.chk.n_rev > 0 and s.chk.n_rev - s.chk.n_rev_hint <= 0.10 * s.chk.n_rev


@pytest.mark.parametrize("L", [150, 100])
@pytest.mark.parametrize("name,native", [("tiny", True), ("tiny", False), ("mid", True),
                                         ("edge", True), ("edge", False)])
def test_fixed_length(request, name, native, L, monkeypatch):
    s = request.getfixturevalue(name)
    _check_fixed(s, _inputs(name, s, L), L, native, monkeypatch)
    if name == "edge":
        assert s.chk.n_rev_zeroed > 0       # the zeroing rule decided


@pytest.mark.parametrize("native", [True, False])
def test_mixed_lengths(tiny, native, monkeypatch):
    """the variable-length pipeline (records with per-read lengths, the generic
    kernel): mates of 15..150 bases"""
    s, L = tiny, 150
    full = interleaved_reads("s150")[:600]
    rng = np.random.default_rng(7)
    lens = rng.integers(15, L + 1, size=full.shape[0]).astype(np.uint16)
    lens[:4] = (150, 20, 19, 128)
    mates = [full[r, :lens[r]].tobytes() for r in range(full.shape[0])]
    n = len(mates) // 2
    stride = S.read_stride(L) if native else L
    rows = V.rows_of(mates, L, stride)
    on = s.device(rows, L, n, True, monkeypatch, native, var_len=True)
    off = s.device(rows, L, n, False, monkeypatch, native, var_len=True)
    _same_run(on, off)
    keys, errs = s.oracle_keys(mates)
    assert sum(errs) == 0
    _check_keys(keys, on[2][0], on[2][2])
    _check_words(s, np.ascontiguousarray(rows[:, :L]), lens, L, on[3], off[3])


# ---------------------------------------------------------------------------
# the GEO kernels: the hg19-shaped index, native rows, hints on
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hg19():
    import genome_cache
    gc.collect()
    contigs, (T, sp, sz, names) = genome_cache.genome_text("hg19")
    dix = S.Index.create(T, sp, sz, names)
    assert dix.info.idx_bytes == 8 and dix.info.pos_bits == R.POS_BITS and dix.info.logN == 33
    cs, n = {}, 0
    for name, s in contigs:
        if "_" in name:
            continue
        cs[name] = n
        n += len(s)
    src = os.path.join(ROOT, "data", "bins", "50000", "bins.txt")
    starts = np.array([int(l.split("\t")[2]) for l in open(src)], np.int64)
    return contigs, dix, cs, starts, np.asarray(sp, np.int64), np.asarray(sz, np.int64)


@pytest.mark.parametrize("L", [150, 100])
def test_geo_kernels_on_hg19(hg19, L, monkeypatch):
    import readgen
    contigs, dix, cs, starts, sp, sz = hg19
    P = 20_000
    d = S.to_rows(readgen.Generator(dix, contigs, L, seed=1100 + L).generate(P), L)
    runs = []
    for hints in (True, False):
        monkeypatch.setenv("SMASH_MAP_HINT", "1" if hints else "0")
        pipe = S.Pipeline(dix, cs, starts, L, P, dedup_capacity=P, read_stride=d.shape[1])
        assert pipe.map_hints == hints
        runs.append(_count(pipe, d, P, len(starts)))
        pipe.close()
    _same_run(runs[0], runs[1])
    (w_on, n_on), (w_off, n_off) = runs[0][3], runs[1][3]
    slots = L - R.MIN_LEN + 1
    assert np.array_equal(n_on, n_off)
    live = np.arange(slots)[None, :] < np.minimum(n_on, slots)[:, None]
    w = w_on[live]
    assert np.array_equal(w & np.uint64(~(0x7FFF << R.POS_BITS) & (2 ** 64 - 1)), w_off[live])
    # every hint against the device's map.bin
    ref = (w & np.uint64(R.POS_MASK)).astype(np.int64)
    ln = (w >> np.uint64(56)).astype(np.int64)
    si = np.searchsorted(sp, ref, side="right") - 1
    assert si.min() >= 0
    o = ref - sp[si]
    size = sz[si & ~1]
    base = np.concatenate([[0], np.cumsum(sz[0::2])])[si >> 1]
    rc = (si & 1) == 1
    h_rc = ((w >> np.uint64(R.POS_BITS)) & np.uint64(0x7F)).astype(np.int64)
    h_fw = ((w >> np.uint64(40)) & np.uint64(0xFF)).astype(np.int64)
    inside = o + ln <= size
    rev = rc & inside
    assert rev.sum() > 1000 and (rev & (h_rc == 0)).sum() <= 0.10 * rev.sum()
    i = dix.info
    dmap = S.device_view(i.d_map, i.map_bytes, torch.uint8)

    def right_bytes(g):
        at = torch.from_numpy(2 + 2 * g + 1).cuda()
        return dmap[at].cpu().numpy().astype(np.int64)
    sel = rev & (h_rc > 0)
    want = right_bytes((base + size - o - ln)[sel])
    assert np.array_equal(np.where(h_rc >= o + ln, 0, h_rc)[sel], want)
    sel = ~rc & (h_fw > 0) & (o < size)
    assert sel.sum() > 1000
    want = right_bytes((base + o)[sel])
    assert np.array_equal(np.where(o + h_fw >= size, 0, h_fw)[sel], want)
