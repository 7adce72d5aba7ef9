"""The device index build, accelerators, search and pipeline on the degenerate
genomes of degenerate_inputs.py: unary, periodic, self-reverse-complement and
twin contigs (every suffix tied for thousands of bases: the prefix doubling of
csrc/sa_build.hip with n_a near N in every round), a repeat that runs into the
text's end, a two-symbol forward-only text, texts of every length from 4 to 80
and on either side of the bucket pass's blocks, hundreds of contigs shorter
than a read / min_len / K + 2 (the bisection branch of k_post_fast's contig
directory, the edge rules of map.bin and of the match hints), and the mosaic
of all of them between unique flanks.

Every comparison is exact, against the oracle, which test_degenerate_inputs.py
pins on the same inputs to a naive suffix sort and to the reference's own
files, and which shows there that no case is empty work.  Marked `gpu`
(MI355X)."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402
import oracle as O  # noqa: E402
import synth  # noqa: E402
import bins_spec  # noqa: E402
import degenerate_inputs as D  # noqa: E402
import geometry_inputs as G  # noqa: E402
import verify_spec as V  # noqa: E402
from test_gpu_bins import check_table  # noqa: E402
from test_gpu_geometry import Side, check_twice, search  # noqa: E402
from test_gpu_mappability import expected_counts, host_uniq, scan  # noqa: E402
from test_gpu_modes import run_match  # noqa: E402
from test_gpu_parity import run_pipeline  # noqa: E402
from test_gpu_rev_hints import _check_keys  # noqa: E402
from test_gpu_verify import assert_clean  # noqa: E402
from test_samout import py_records  # noqa: E402

PROOF = S.VERIFY_LAYOUT | S.VERIFY_SA | S.VERIFY_LCP


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def oracle_accel(oix):
    """oix.accel() with the B-mer bitmap at the device's B = K + 2: the
    oracle's own choice (orc_accel_b) has a floor of 8, which is K + 2 only
    from N = 4 096 on"""
    import ctypes as C
    U, KT, K = oix.accel()
    if oix.acc.B != K + 2:
        B = K + 2
        BM = np.zeros((1 << (2 * B)) // 64 + 1, np.uint64)
        in_text = np.zeros(256, np.uint8)
        O.lib().orc_build_bitmap(C.byref(oix.c), B, BM.ctypes.data_as(O.u64p),
                                 in_text.ctypes.data_as(O.u8p))
        oix.accel(U, KT, K, BM, B, in_text, oix._KTF)
    assert oix.acc.B == oix.acc.K + 2
    return oix


_oix, _dix = {}, {}


def oracle_index(name):
    if name not in _oix:
        _oix[name] = oracle_accel(O.Index(*O.text_from_contigs(D.genome(name))))
    return _oix[name]


def device_index(name, width=4):
    """the device's index of a genome, built once per module; 8: packed words"""
    if (name, width) not in _dix:
        assert torch.cuda.is_available()
        o = oracle_index(name)
        with env(SMASH_IDX_BYTES=width):
            _dix[name, width] = S.Index.create(o.T[:o.N], o.startpos, o.sizes, o.names)
        assert _dix[name, width].info.idx_bytes == width
    return _dix[name, width]


def arrays(dix):
    """_arrays with an empty overflow table and an index without a map"""
    i = dix.info
    SA, ISA = dix.download_sa_isa(plain=True)
    ovf = (S.download(i.d_lcp_ovf, 16 * i.n_lcp_overflow, np.uint64) if i.n_lcp_overflow
           else np.zeros(0, np.uint64)).reshape(-1, 2)
    mp = S.download(i.d_map, i.map_bytes) if dix.rcref else None
    return S.download(i.d_text, i.N), SA, ISA, S.download(i.d_lcp8, i.N), ovf, mp


def check_index(dix, oix, rcref=True):
    """text, SA, ISA, the LCP bytes, the overflow table and map.bin past its
    header equal the oracle's; verify() is clean and its report the spec's"""
    T, SA, ISA, L8, ovf, mp = arrays(dix)
    N = oix.N
    assert dix.info.N == N and dix.info.logN == O.lib().orc_logN(N)
    assert np.array_equal(T, oix.T[:N])
    bad = np.nonzero(SA.astype(np.uint64) != oix.SA.astype(np.uint64))[0]
    assert not len(bad), ("first differing rank", int(bad[0]), int(SA[bad[0]]), int(oix.SA[bad[0]]))
    assert np.array_equal(ISA.astype(np.uint64), oix.ISA.astype(np.uint64))
    bad = np.nonzero(L8 != oix.L8)[0]
    assert not len(bad), ("first differing LCP byte", int(bad[0]), int(L8[bad[0]]), int(oix.L8[bad[0]]))
    assert dix.info.n_lcp_overflow == len(oix.ovf) and np.array_equal(ovf, oix.ovf)
    omap = oix.mappability() if rcref else None
    if rcref:
        assert dix.info.map_bytes == len(omap) and np.array_equal(mp[2:], omap[2:])
    rep = dix.verify().as_dict()
    assert rep["ok"] == 1, (N, {k: v for k, v in rep.items() if v not in (0, V.NONE)})
    assert_clean(dix.verify(), S.VERIFY_ALL if rcref else PROOF)
    want = V.verify_spec(T, SA, ISA, L8, ovf, oix.startpos, oix.sizes, rcref=rcref, mapbin=mp,
                         true_map=omap, true_sa=oix.SA, true_lcp=oix.LCP)
    for k in V.FIELDS:
        assert rep[k] == want[k], (k, rep[k], want[k])


def check_accel(dix, oix):
    """test_gpu_parity.test_device_accelerators_equal_oracle on any index"""
    i = dix.info
    U2, KT2, K2 = oix._U, oix._KT, oix.acc.K
    assert i.kmer_k == K2 and i.bitmap_b == oix.acc.B == K2 + 2 and not i.d_bitmap
    assert np.array_equal(S.download(i.d_uniq, i.N + 64)[:i.N], U2[:i.N])
    KT = S.download(i.d_kmer, 16 << (2 * i.kmer_k), np.uint64)
    bad = np.nonzero(KT != oix._KTF)[0]
    assert not len(bad), ("first differing table word", int(bad[0]), hex(int(KT[bad[0]])),
                          hex(int(oix._KTF[bad[0]])))
    assert np.array_equal(KT & np.uint64((1 << 40) - 1), KT2)
    B = i.bitmap_b
    codes = np.arange(1 << (2 * B), dtype=np.uint64)
    bm = (oix._BM[codes >> np.uint64(6)] >> (codes & np.uint64(63))) & np.uint64(1)
    w0 = KT.reshape(-1, 2)[:, 0]
    bits = (w0[codes >> np.uint64(4)] >> (np.uint64(40) + (codes & np.uint64(15)))) & np.uint64(1)
    assert np.array_equal(bm, bits)
    assert [(i.in_text[c >> 6] >> (c & 63)) & 1 for c in range(256)] == list(oix.acc.in_text)
    return K2


# ---------------------------------------------------------------------------
# a. + b. the index build and the accelerators
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.NAMES)
def test_index_build(name):
    oix = oracle_index(name)
    dix = device_index(name)
    check_index(dix, oix)
    assert check_accel(dix, oix) == kmer_k(oix.N)


@pytest.mark.parametrize("name", ["mosaic", "selfrc", "twins"])
def test_index_build_wide_words(name):
    oix = oracle_index(name)
    dix = device_index(name, 8)
    assert dix.info.pos_bits == 33
    check_index(dix, oix)
    check_accel(dix, oix)


@pytest.mark.parametrize("name", ["unary", "tailrun", "nruns"])
def test_index_build_kasai_form(name):
    oix = oracle_index(name)
    with env(SMASH_LCP_KASAI=1):
        dix = S.Index.create(oix.T[:oix.N], oix.startpos, oix.sizes, oix.names)
    check_index(dix, oix)


def test_index_build_two_symbols_forward_only():
    T, sp, sz, names = D.sigma2()
    oix = O.Index(T, sp, sz, names)
    for kasai in (0, 1):
        with env(SMASH_LCP_KASAI=kasai):
            dix = S.Index.create(T, sp, sz, names, rcref=False)
        check_index(dix, oix, rcref=False)
    assert check_accel(dix, oracle_accel(oix)) == kmer_k(oix.N) == 5     # the first K >= 5


def kmer_k(N):
    """build_aux's K = max(4, floor(log4 N))"""
    K = 4
    while 4 ** (K + 1) <= N:
        K += 1
    return K


def _sweep(sizes, **kw):
    ks = set()
    for N in sizes:
        T, sp, sz, names, rcref = D.sweep_text(N)
        oix = oracle_accel(O.Index(T, sp, sz, names))
        with env(**kw):
            dix = S.Index.create(T, sp, sz, names, rcref=rcref)
        assert dix.info.idx_bytes == int(kw.get("SMASH_IDX_BYTES", 4))
        check_index(dix, oix, rcref)
        ks.add(check_accel(dix, oix))
    return ks


@pytest.mark.parametrize("lo", [4, 23, 42, 61])
@pytest.mark.parametrize("kasai", [0, 1])
def test_size_sweep_small(lo, kasai):
    """every text length from 4 to 80: every residue of N mod 16 (k_plcp's
    partial block), K = 4, k_kcode / k_kfilter's words past the text's end"""
    assert _sweep([n for n in D.SWEEP_N if lo <= n < lo + 19 and n <= 80],
                  SMASH_LCP_KASAI=kasai) == {4}


@pytest.mark.parametrize("N", [n for n in D.SWEEP_N if n > 80])
def test_size_sweep_bucket_blocks(N):
    """N on either side of one and of two blocks of 256 x 64 positions
    (k_bucket_count / k_bucket_scatter); the first K >= 5"""
    assert kmer_k(N) == (6 if N < 16384 else 7)
    assert _sweep([N]) == {kmer_k(N)}
    assert _sweep([N], SMASH_LCP_KASAI=1) == {kmer_k(N)}


@pytest.mark.parametrize("n", range(1, 10))
def test_scan_of_a_first_contig_of_a_few_bases(n):
    """the scan's 16-byte block of U at a reverse-complement position ends
    within the text's first 15 bytes when the first contig has fewer than 8
    bases: the block was taken as saturated instead of loaded, the scan wrote
    the contig's left bytes as 0, and verify(), which compares the scan with
    the index's map.bin, rejected the index the build itself had made"""
    T, sp, sz, names, _ = D.sweep_text(2 * n + 2)
    oix = O.Index(T, sp, sz, names)
    dix = S.Index.create(T, sp, sz, names)
    omap = oix.mappability()[2:]
    for k in (20, 36):
        mp, cc, _ = scan(dix, 0, n, k)
        assert np.array_equal(mp, omap), (n, mp.tolist(), omap.tolist())
        assert cc.tolist() == [int(((omap[1::2] >= 1) & (omap[1::2] <= k)).sum())]
    assert n < 3 or omap[0::2].any()             # (a left byte that is not zero)


def test_size_sweep_wide_words():
    _sweep([5, 48, 16385], SMASH_IDX_BYTES=8)


def check_save_and_load(dix, oix, contigs, fa):
    """save; Index.load(verify=VERIFY_ALL) gives the same arrays and
    accelerators behind a clean report; without map.bin the loader recomputes
    it on the device; every loaded index equals the oracle and verifies"""
    synth.write_fasta(fa, contigs)
    dix.save(fa)
    a = arrays(dix)
    got = S.Index.load(fa, verify=S.VERIFY_ALL)
    assert_clean(got.verify_report)
    for x, y in zip(a, arrays(got)):
        assert np.array_equal(x, y)
    check_accel(got, oix)
    os.remove(fa + ".bin/map.bin")
    again = S.Index.load(fa)
    check_index(again, oix)
    check_accel(again, oix)


@pytest.mark.parametrize("name", D.NAMES)
def test_save_and_load(name, tmp_path):
    check_save_and_load(device_index(name), oracle_index(name), D.genome(name),
                        str(tmp_path / (name + ".fa")))


@pytest.mark.parametrize("sizes", [[n for n in D.SWEEP_N if n % 2 == 0 and n <= 40],
                                   [n for n in D.SWEEP_N if n % 2 == 0 and 40 < n <= 80],
                                   [n for n in D.SWEEP_N if n % 2 == 0 and n > 80]])
def test_save_and_load_size_sweep(sizes, tmp_path):
    """the even sizes (a contig and its reverse complement: the layout with a
    map.bin), among them every first contig of 1..7 bases"""
    for N in sizes:
        T, sp, sz, names, rcref = D.sweep_text(N)
        assert rcref
        oix = oracle_accel(O.Index(T, sp, sz, names))
        dix = S.Index.create(T, sp, sz, names)
        check_save_and_load(dix, oix, [("chr1", T[:int(sz[0])])], str(tmp_path / ("n%d.fa" % N)))


def _bin_tables(name):
    """(chrom offsets per contig, bin starts) of a genome, every contig without
    '_' binned"""
    g = D.genome(name)
    cs = D.chrom_sizes(g)
    off = np.array([cs.get(n, -1) for n, _ in g], np.int64)
    return off, D.bin_starts(g)


@pytest.mark.parametrize("name", ["mosaic", "nruns", "unary"])
def test_mappability_scan_and_prepare(name, monkeypatch):
    """test_gpu_mappability's checks on genomes whose map.bin is mostly 0 and
    255 and whose chromosomes may hold no unique start: the scan at k 20 and
    36 over 1, 3 and 8 partitions, and U rebuilt from SA + L8 in every form"""
    oix, dix = oracle_index(name), device_index(name)
    off, starts = _bin_tables(name)
    total = sum(dix.contig_sizes)
    omap = oix.mappability()[2:]
    for k in (20, 36):
        ecc, ebc = expected_counts(omap, dix.contig_sizes, k, off, starts)
        for parts in (1, 3, 8):
            rng = np.random.default_rng(parts)
            cuts = [0] + sorted(int(x) for x in rng.integers(1, total, parts - 1)) + [total]
            maps, cc, bc = [], 0, 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                m, c1, b1 = scan(dix, a, b, k, off, starts)
                maps.append(m)
                cc, bc = cc + c1, bc + b1
            assert np.array_equal(np.concatenate(maps), omap), (k, parts)
            assert cc.tolist() == ecc.tolist() and bc.tolist() == ebc.tolist(), (k, parts)
    N = dix.info.N
    U = S.device_view(dix.info.d_uniq, N + 64, torch.uint8)
    want = host_uniq(oix)
    try:
        for form in ({}, {"SMASH_UNIQ_GATHER": "1"}, {"SMASH_UPART_E2MB": "1"},
                     {"SMASH_UPART_NT": "512", "SMASH_UPART_NT2": "512"}):
            for k, v in form.items():
                monkeypatch.setenv(k, v)
            U[:N].fill_(0x55)
            S.mappability_prepare(dix, 0, total)
            torch.cuda.synchronize()
            assert np.array_equal(U[:N].cpu().numpy(), want), form
            assert np.array_equal(scan(dix, 0, total, 36, off, starts)[0], omap), form
            for k in form:
                monkeypatch.delenv(k)
    finally:
        S.mappability_release(dix)


# ---------------------------------------------------------------------------
# c. the refusal
# ---------------------------------------------------------------------------
def test_alphabet_of_eight_symbols_is_refused(tiny_fa, tiny_ix):
    """an IUPAC code and its complement make eight symbols with the separator
    and the terminator: more than the two-character buckets hold.  The build
    refuses the text, and the next build in the process is correct."""
    g = [("chr1", np.frombuffer(b"ACGTTGCAGGR" + b"ACGGTCA" * 40, np.uint8))]
    T = O.text_from_contigs(g)[0]
    assert len(set(T.tobytes())) == 8
    with pytest.raises(S.SmashError) as e:
        S.Index.from_contigs(g)
    assert "alphabet too large for 2-char buckets" in str(e.value)
    check_index(S.Index.from_fasta(tiny_fa), tiny_ix)


# ---------------------------------------------------------------------------
# d. the search
# ---------------------------------------------------------------------------
_reads = {}


def junction_reads(name, L):
    if (name, L) not in _reads:
        _reads[name, L] = D.junction_reads(oracle_index(name), L)
    return _reads[name, L]


def side(name, width=4):
    o = oracle_index(name)
    return Side(o, device_index(name, width), o.acc.B)


@pytest.mark.parametrize("layout", ["rows", "dense"])
@pytest.mark.parametrize("L", [40, 100, 150])
@pytest.mark.parametrize("name,width", [("mosaic", 4), ("mosaic", 8), ("specks", 4), ("nruns", 4)])
def test_search_junction_reads(name, width, L, layout):
    s = side(name, width)
    reads = junction_reads(name, L)
    for ml in (20, s.oix.acc.B + 2):
        check_twice(s, reads, L, ml, layout)


@pytest.mark.parametrize("L", [40, 100, 150])
def test_search_unpacked_wide_words(L):
    s = side("mosaic", 8)
    reads = junction_reads("mosaic", L)
    s.dix.pack(False)
    try:
        assert s.dix.info.pos_bits == 0
        for layout in ("rows", "dense"):
            check_twice(s, reads, L, 20, layout)
    finally:
        s.dix.pack(True)


@pytest.mark.parametrize("L", [40, 100, 150])
@pytest.mark.parametrize("name,width", [("mosaic", 4), ("mosaic", 8), ("specks", 4), ("nruns", 4)])
def test_plain_mum_mem_junction_reads(name, width, L, monkeypatch):
    s = side(name, width)
    reads = junction_reads(name, L)
    cap = 4096
    s.want_all(reads, (20,), "MEM")
    sm, k_sm = search(s, reads, L, 20, "dense")
    plain, k_plain = search(s, reads, L, 20, "dense", mode=S.SMASH_MODE_MAM_PLAIN)
    assert np.array_equal(k_sm, k_plain) and plain == sm
    for mode, defer in (("MUM", None), ("MEM", None), ("MEM", "0"), ("MEM", "2")):
        if defer:
            monkeypatch.setenv("SMASH_MEM_DEFER", defer)
        got, n = run_match(s.dix, reads, mode, cap=cap, min_len=20)
        monkeypatch.delenv("SMASH_MEM_DEFER", raising=False)
        for r in range(reads.shape[0]):
            exp = s.want(reads[r], 20, mode)
            assert n[r] == len(exp), (mode, defer, r)
            assert got[r] == exp[:cap], (mode, defer, r, bytes(reads[r]))


@pytest.mark.parametrize("name", D.PURE_REPEATS)
def test_pure_repeats(name, monkeypatch):
    """no MAM match for any read inside the repeat; MEM with thousands of
    matches per read, past the cap (the count goes on, the list is cut)"""
    s = side(name)
    cap, most = 4096, 0
    for L in (40, 100):
        reads = junction_reads(name, L)
        inside = [r for r in range(reads.shape[0])
                  if b"`" not in reads[r].tobytes() and b"$" not in reads[r].tobytes()]
        for layout in ("rows", "dense"):
            got, k = search(s, reads, L, 20, layout)
            assert all(k[r] == 0 for r in inside)
            for r in range(reads.shape[0]):
                assert got[r] == s.want(reads[r], 20), (L, layout, r)
        s.want_all(reads, (20,), "MEM")
        for defer in ("0", "2"):
            monkeypatch.setenv("SMASH_MEM_DEFER", defer)
            got, n = run_match(s.dix, reads, "MEM", cap=cap, min_len=20)
            for r in range(reads.shape[0]):
                exp = s.want(reads[r], 20, "MEM")
                assert n[r] == len(exp) and got[r] == exp[:cap], (L, defer, r)
                most = max(most, len(exp))
    assert most > (cap if name in ("unary", "selfrc") else 1000)


# ---------------------------------------------------------------------------
# e. the pipeline on the mosaic
# ---------------------------------------------------------------------------
class Mosaic:
    def __init__(self):
        self.g = D.genome("mosaic")
        self.oix = oracle_index("mosaic")
        self.mapbin = self.oix.mappability()
        self.cs = D.chrom_sizes(self.g)
        self.starts = D.bin_starts(self.g)
        self.want = {}

    def case(self, L, ml):
        """(error-free reads, their chain, the oracle's pipeline per bin
        table, the pairs the tagger throws on)"""
        if (L, ml) not in self.want:
            reads, bad = D.pipeline_reads(self.g, self.oix, self.mapbin, L, ml)
            chain = G.Chain(self.oix, reads, min_len=ml, mapbin=self.mapbin)
            assert chain.tag_errors == 0
            self.want[L, ml] = reads, chain, {}, bad
        return self.want[L, ml]

    def oracle_pipeline(self, L, ml, starts):
        reads, _, ops, _ = self.case(L, ml)
        k = tuple(starts.tolist())
        if k not in ops:
            ops[k] = O.Pipeline(self.oix, self.mapbin, self.cs, starts, min_len=ml)
            assert ops[k].run(reads, threads=4) == 0
        return ops[k]


@pytest.fixture(scope="module")
def mosaic():
    return Mosaic()


def run_mosaic(m, dix, L, ml, starts, native, min_excess=4, batch=None):
    reads = m.case(L, ml)[0]
    n = reads.shape[0] // 2
    pipe = S.Pipeline(dix, m.cs, starts, read_len=L, max_pairs=n, min_len=ml, min_excess=min_excess,
                      read_stride=S.read_stride(L) if native else 0)
    rows = reads if not native else S.to_rows(torch.from_numpy(reads).cuda(), L).cpu().numpy()
    counts, st = run_pipeline(pipe, rows, len(starts), batch=batch)
    assert st.error == 0
    out = (counts, st.as_dict()) + ((pipe.peek(n), pipe.peek_matches(n)) if batch is None
                                    else (None, None))
    pipe.close()
    return out


def check_mosaic(m, run, L, ml, starts, min_excess=4):
    reads, chain, _, _ = m.case(L, ml)
    counts, st, pk, pm = run
    if pk is not None:
        (nk, keep, hits), (words, nw) = pk, pm
        assert nw.tolist() == [len(x) for x in chain.matches]
        # every mate's match words: position (the element bits; the map hints
        # sit above them), query offset and length, in the search's order
        for r, exp in enumerate(chain.matches):
            got = [(int(w) & ((1 << 33) - 1), (int(w) >> 48) & 0xFF, int(w) >> 56)
                   for w in words[r, :len(exp)]]
            assert got == exp, (r, got, exp)
        keys = chain.keys if min_excess == 4 else [
            O.smash_pair(*[_tagged(m, reads[2 * q + k], ml) for k in (0, 1)], min_excess=min_excess)
            for q in range(len(chain.keys))]
        for q, exp in enumerate(keys):
            assert nk[q] == (-1 if exp is None else len(exp)), q
        _check_keys(keys, nk, hits)
        if min_excess == 4:
            for q, exp in enumerate(keys):
                if exp is not None:
                    assert bool(keep[q]) == chain.keep[q], q
    if min_excess == 4:
        op = m.oracle_pipeline(L, ml, starts)
        assert np.array_equal(counts, op.counts)
        assert (st["positions"], st["dups"], st["kept"]) == (op.state.total, op.state.dups,
                                                             op.state.kept)
        assert st["dupe_pairs"] == op.n_dupe.value
        assert st["key_pairs"] == sum(k is not None for k in chain.keys)


def _tagged(m, read, ml):
    offs = np.cumsum([0] + [int(x) for x in m.oix.sizes[0::2]][:-1]).astype(np.uint32)
    P = read.tobytes()
    h, _ = m.oix.resolve(P, m.oix.search(P, min_len=ml))
    for x in h:
        assert O.tag(x, offs, m.mapbin, 1 if "_gl000" in m.oix.contigs[x.tid] else 0) == 0
    return h


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("L", D.PIPE_LENGTHS)
def test_pipeline(mosaic, L, width, native, monkeypatch):
    """min_len 20 and B + 2; min_excess 4 and -3; every mate through
    k_post_fast<8>, through the hand-offs (SMASH_POST_CAP=3), with the map
    hints and without; in one batch and in batches of 97"""
    m, dix = mosaic, device_index("mosaic", width)
    B = m.oix.acc.B
    for ml in (20, B + 2):
        one = run_mosaic(m, dix, L, ml, m.starts, native)
        check_mosaic(m, one, L, ml, m.starts)
        for e in ({"SMASH_POST_CAP": "3"}, {"SMASH_MAP_HINT": "0"}):
            for k, v in e.items():
                monkeypatch.setenv(k, v)
            other = run_mosaic(m, dix, L, ml, m.starts, native)
            for k in e:
                monkeypatch.delenv(k)
            check_mosaic(m, other, L, ml, m.starts)
            assert np.array_equal(other[0], one[0]) and other[1] == one[1]
        small = run_mosaic(m, dix, L, ml, m.starts, native, batch=97)
        assert np.array_equal(small[0], one[0]) and small[1] == one[1]
    check_mosaic(m, run_mosaic(m, dix, L, 20, m.starts, native, min_excess=-3), L, 20, m.starts, -3)


def test_designed_bins(mosaic):
    """Index.design_bins on a genome with chromosomes that hold no unique
    start, against the rule; and the pipeline over the designed table"""
    m, dix = mosaic, device_index("mosaic")
    off = S.contig_tables(dix.contigs, dix.contig_sizes, m.cs)[2]
    rows, M = bins_spec.design(m.mapbin[2:], dix.contig_sizes, off, 36, 200, m.oix.T,
                               m.oix.startpos[0::2])
    rec, gotM = dix.design_bins(m.cs, k=36, nbins=200, unique=True)
    check_table(rec, rows)
    assert gotM.tolist() == M and sum(1 for c, x in enumerate(M) if off[c] >= 0 and x == 0) >= 2
    starts = np.ascontiguousarray(rec["abspos"], np.int64)
    check_mosaic(m, run_mosaic(m, dix, 100, 20, starts, True), 100, 20, starts)


def test_tag_error_is_reported(mosaic):
    """a pair the tagger throws on (a block on a major-named speck, shorter
    than its neighbour's map byte): the device reports the data error the
    oracle's pipeline returns, not counts"""
    m, dix = mosaic, device_index("mosaic")
    L = 40
    bad = m.case(L, 20)[3]
    # (the pairs with one failing hit: the first error is that hit's, in
    # whatever order a pair's hits are tagged)
    one = [q for q, e in enumerate(D.pair_errors(m.oix, bad, m.mapbin)) if e == 1]
    assert one
    seen = set()
    for q in one:
        pair = np.ascontiguousarray(bad[2 * q:2 * q + 2])
        op = O.Pipeline(m.oix, m.mapbin, m.cs, m.starts)
        want = op.run(pair)
        assert want in (1, 2)
        if want in seen:
            continue
        seen.add(want)
        pipe = S.Pipeline(dix, m.cs, m.starts, read_len=L, max_pairs=1)
        counts = torch.zeros(len(m.starts), dtype=torch.int64, device="cuda")
        pipe.count_batch(torch.from_numpy(pair).cuda(), 1, counts)
        assert pipe.stats(raise_on_error=False).error == want
        with pytest.raises(S.SmashError):
            pipe.stats()
        pipe.close()


@pytest.mark.parametrize("L", [40, 100])
def test_sam_records(mosaic, L):
    """the memsam path's records (k_sam_recs) of the junction reads: reads
    longer than their contig, negative positions, map bytes past the map"""
    m, dix = mosaic, device_index("mosaic")
    reads = junction_reads("mosaic", L)
    offsets = np.cumsum([0] + [int(x) for x in m.oix.sizes[0::2]][:-1]).astype(np.uint32)
    cap = L - 20 + 1
    triples = [m.oix.search(r.tobytes()) for r in reads]
    exp, ecnt = py_records(m.oix, m.mapbin, offsets, reads, triples, cap)
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    got, cnt = S.sam_records(dix, d, reads.shape[0], L, cap, tag_offsets=offsets)
    assert cnt.tolist() == ecnt.tolist()
    o = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    assert len(got) == o[-1] and (exp["pos"] < 0).any()
    for r in range(reads.shape[0]):
        a, b = got[o[r]:o[r + 1]], exp[r * cap:r * cap + cnt[r]]
        assert a.tobytes() == b.tobytes(), (r, a, b)
