"""The device search and pipeline off the benchmark's read geometry (100 /
150 bases, min_len 20): every read length on either side of a step of the
LDS row, of the bad mask's words and of its second record chunk, up to the
ABI's 255, and min_len on every branch of the (F) window filter relative to
the index's B (tests/geometry_inputs.py; the emulator's sweep of the same
grid on one CPU lane: test_sm_emu.py).  What only the device has is under
test here: the row DMA into LDS and the per-lane row stride, 64 lanes
diverging, k_prep's launch geometry on unaligned dense reads, the LDS rows
launch_plain and launch_mem size from L, and the post stage with rows of 1 to
243 slots -- k_post_fast<8> / <16> / k_post hand-offs, keys longer than the
head row, hints at their caps, per-read lengths under other row widths.

Every comparison is exact, against the oracle (test_geometry_inputs.py shows
from the oracle alone that no case is empty work).  Marked `gpu` (MI355X)."""
import numpy as np
import pytest

from conftest import gold, load_bins, load_chrom_sizes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402
import oracle as O  # noqa: E402
import synth  # noqa: E402
import geometry_inputs as G  # noqa: E402
import varlen_util as V  # noqa: E402
from test_gpu_modes import _edge_reads as low_complexity_reads, run_match  # noqa: E402
from test_gpu_parity import run_pipeline  # noqa: E402
from test_gpu_rev_hints import Subject as PackedSubject, _check_keys, _same_run  # noqa: E402
from test_gpu_sm_merges import GARBAGE  # noqa: E402
from test_gpu_varlen import make_pipe as make_var_pipe, run as run_var  # noqa: E402

CS = load_chrom_sizes(gold("tiny_chrom_sizes.txt"))
STARTS = load_bins(gold("tiny_bins.txt"))[1]
MODE_LENGTHS = (20, 33, 41, 76, 129, 153, 255)


_want = {}      # oracle index -> {(read, min_len, mode): matches}, computed once


class Side:
    """one oracle index and a device index of the same text, with the
    oracle's matches of every (read, mode, min_len) asked for (shared by the
    device indexes of one text)"""

    def __init__(self, oix, dix, B):
        oix.accel()
        self.oix, self.dix = oix, dix
        # the min_len grid is relative to B: the device's and the oracle's agree
        assert dix.info.bitmap_b == oix.acc.B == B
        self._want = _want.setdefault(id(oix), {})

    def want(self, read, ml, mode="MAM"):
        k = (read.tobytes(), ml, mode)
        if k not in self._want:
            self._want[k] = self.oix.search(k[0], mode, min_len=ml)
        return self._want[k]

    def want_all(self, reads, mls, mode):
        """the same on 8 host threads: the oracle's MEM list of a read inside
        a long run (n * L in the text's N runs: 10^5 records) takes seconds"""
        from concurrent.futures import ThreadPoolExecutor
        todo = {(reads[r].tobytes(), ml, mode) for r in range(reads.shape[0]) for ml in mls}
        todo = sorted(todo - set(self._want))
        with ThreadPoolExecutor(8) as ex:
            for k, m in zip(todo, ex.map(lambda k: self.oix.search(k[0], k[2], min_len=k[1]), todo)):
                self._want[k] = m


@pytest.fixture(scope="module")
def tiny(tiny_fa, tiny_ix):
    assert torch.cuda.is_available()
    dix = S.Index.from_fasta(tiny_fa, device=0)
    assert dix.info.idx_bytes == 4
    return Side(tiny_ix, dix, 11)


@pytest.fixture(scope="module")
def mid_genome():
    g = synth.make_genome("mid")
    return g, O.Index(*O.text_from_contigs(g))


@pytest.fixture(scope="module")
def mid_packed(mid_genome, tmp_path_factory):
    """the mid genome as 8-byte packed words (SMASH_IDX_BYTES=8), with the
    chromosome offsets and bins of a pipeline run"""
    g, oix = mid_genome
    tmp = tmp_path_factory.mktemp("mid")
    rows = synth.make_bins(g, 4, str(tmp / "bins.txt"))
    synth.write_index_side_files(str(tmp), g)
    s = PackedSubject(oix, load_chrom_sizes(str(tmp / "chrom_sizes.txt")), [r[2] for r in rows])
    s.g = g
    s.side = Side(oix, s.dix, 13)
    return s


@pytest.fixture(scope="module")
def mid4(mid_genome):
    """4-byte elements, for the MEM / MUM test only"""
    _, oix = mid_genome
    dix = S.Index.create(oix.T[:oix.N], oix.startpos, oix.sizes, oix.names)
    assert dix.info.idx_bytes == 4
    return Side(oix, dix, 13)


def _side(request, name):
    if name == "tiny":
        return request.getfixturevalue("tiny")
    if name == "mid-4":
        return request.getfixturevalue("mid4")
    return request.getfixturevalue("mid_packed").side


_edge = {}


def edge_reads(side, L):
    k = (id(side.oix), L)
    if k not in _edge:
        _edge[k] = G.edge_reads(side.oix, L, 130, seed=L)
    return _edge[k]


def search(side, reads, L, ml, layout, fill=(0, -1), mode=S.SMASH_MODE_MAM):
    """smash_map_batch, synchronous (it fails when a probe left the index:
    mam.hip probe_check), cap = the slots of (L, min_len), the outputs
    pre-filled with `fill`; per read its matches and its count"""
    n = reads.shape[0]
    cap = L - ml + 1
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    stride = L                              # dense: odd L gives unaligned reads
    if layout == "rows":
        d = S.to_rows(d, L)
        stride = S.read_stride(L)
    o = torch.full((n * cap,), fill[0], dtype=torch.int64, device="cuda")
    nn = torch.full((n,), fill[1], dtype=torch.int32, device="cuda")
    S.check(S.lib().smash_map_batch(side.dix.h, mode, ml, S._ptr(d), stride, None, L, n,
                                    S._ptr(o), cap, S._ptr(nn),
                                    S.vp(torch.cuda.current_stream().cuda_stream)),
            "smash_map_batch")
    torch.cuda.synchronize()
    w = o.cpu().numpy().view(np.uint64).reshape(n, cap)
    k = nn.cpu().numpy()
    assert k.min() >= 0 and k.max() <= cap, (L, ml, layout, k.min(), k.max())
    return [S.unpack_matches(w[r], k[r]) for r in range(n)], k


def check_twice(side, reads, L, ml, layout):
    want = [side.want(reads[r], ml) for r in range(reads.shape[0])]
    for run, fill in enumerate(GARBAGE):
        got, k = search(side, reads, L, ml, layout, fill)
        for r in range(reads.shape[0]):
            assert k[r] == len(want[r]), (L, ml, layout, run, r, bytes(reads[r]))
            assert got[r] == want[r], (L, ml, layout, run, r, bytes(reads[r]))


# ---------------------------------------------------------------------------
# a. the search at every length and min_len
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("index", ["tiny", "mid-packed"])
@pytest.mark.parametrize("layout", ["rows", "dense"])
@pytest.mark.parametrize("L", G.LENGTHS)
def test_search_lengths_and_min_lens(request, L, layout, index):
    side = _side(request, index)
    if layout == "rows":
        # the C ABI's stride is the geometry's row (mam_sm.hpp make_geom)
        assert S.read_stride(L) == 4 * G.w_row(L)
    reads = edge_reads(side, L)
    assert reads.shape[0] % 64
    for ml in G.min_lens(side.oix.acc.B, L):
        check_twice(side, reads, L, ml, layout)


# ---------------------------------------------------------------------------
# b. one lane per wave, and 64 lanes in lock step plus one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", G.LENGTHS)
def test_one_lane_per_wave_at_each_length(tiny, L):
    """test_gpu_sm_loads' dummy-load and lock-step shapes at the other row
    widths: a wave whose other 63 lanes only ever issue the dummy loads, and
    65 copies of one read (a full wave in lock step, a second with one lane)"""
    reads = edge_reads(tiny, L)
    for ml in (tiny.oix.acc.B + 2, 20):
        check_twice(tiny, reads[-1:], L, ml, "rows")
        for r in (0, reads.shape[0] - 2):
            check_twice(tiny, np.repeat(reads[r][None, :], 65, axis=0), L, ml, "rows")


# ---------------------------------------------------------------------------
# c. k_mam (MAM_PLAIN), k_mum and k_mem size their LDS rows from L
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("index", ["tiny", "mid-4", "mid-8"])
@pytest.mark.parametrize("L", MODE_LENGTHS)
def test_plain_mum_mem_lengths(request, L, index, monkeypatch):
    side = _side(request, index)
    oix = side.oix
    reads = np.concatenate([edge_reads(side, L),
                            low_complexity_reads(oix.T[:oix.N - 1], L, 45, np.random.default_rng(L))])
    cap = 4096
    mls = G.pipe_min_lens(oix.acc.B, L)[:2]             # B + 2 and 20, those <= L
    side.want_all(reads, mls, "MEM")
    for ml in mls:
        sm, k_sm = search(side, reads, L, ml, "dense")
        plain, k_plain = search(side, reads, L, ml, "dense", mode=S.SMASH_MODE_MAM_PLAIN)
        assert np.array_equal(k_sm, k_plain), (L, ml)
        assert plain == sm, (L, ml)
        for mode, defer in (("MUM", None), ("MEM", None), ("MEM", "2")):
            if defer:
                monkeypatch.setenv("SMASH_MEM_DEFER", defer)
            got, n = run_match(side.dix, reads, mode, cap=cap, min_len=ml)
            monkeypatch.delenv("SMASH_MEM_DEFER", raising=False)
            for r in range(reads.shape[0]):
                exp = side.want(reads[r], ml, mode)
                assert n[r] == len(exp), (L, ml, mode, defer, r)
                assert got[r] == exp[:cap], (L, ml, mode, defer, r, bytes(reads[r]))


# ---------------------------------------------------------------------------
# d. the pipeline at other lengths and min_len
# ---------------------------------------------------------------------------
_pipe_want = {}


def pipe_want(oix, genome, L, ml, n_pairs=1500, seed=None, **kw):
    """(reads, the oracle's per-pair chain, its pipeline) of one case"""
    k = (L, ml, n_pairs, seed, tuple(sorted(kw.items())))
    if k not in _pipe_want:
        reads = G.smash_reads(genome, n_pairs, L, seed=L if seed is None else seed, **kw)
        mapbin = oix.mappability()
        op = O.Pipeline(oix, mapbin, CS, STARTS, min_len=ml)
        assert op.run(reads, threads=4) == 0
        _pipe_want[k] = reads, G.Chain(oix, reads, min_len=ml, mapbin=mapbin), op
    return _pipe_want[k]


def device_rows(reads, L, native):
    if not native:
        return reads
    return S.to_rows(torch.from_numpy(reads).cuda(), L).cpu().numpy()


def run_and_peek(dix, reads, L, ml, native, batch, peek=True):
    n = reads.shape[0] // 2
    assert S.pipeline_max_batch(L, ml) >= n
    pipe = S.Pipeline(dix, CS, STARTS, read_len=L, max_pairs=n, min_len=ml,
                      read_stride=S.read_stride(L) if native else 0)
    counts, st = run_pipeline(pipe, device_rows(reads, L, native), len(STARTS), batch=batch)
    assert st.error == 0
    out = counts, st.as_dict(), (pipe.peek(n) if peek else None)
    pipe.close()
    return out


def check_against_oracle(run, chain, op):
    counts, st, pk = run
    assert np.array_equal(counts, op.counts)
    assert (st["positions"], st["dups"], st["kept"]) == (op.state.total, op.state.dups,
                                                         op.state.kept)
    assert st["dupe_pairs"] == op.n_dupe.value
    assert st["key_pairs"] == sum(k is not None for k in chain.keys)
    if pk is not None:
        nk, keep, hits = pk
        for q, exp in enumerate(chain.keys):
            assert nk[q] == (-1 if exp is None else len(exp)), q
        _check_keys(chain.keys, nk, hits)
        for q, exp in enumerate(chain.keys):
            if exp is not None:
                assert bool(keep[q]) == chain.keep[q], q      # the host's first-wins set


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("L", G.PIPE_LENGTHS)
def test_pipeline_lengths(tiny, L, native):
    """L 20 at min_len 20 is the one-slot pipeline; 24 has 5 slots, below
    k_post_fast<8>'s capacity (post_cap = min(16, slots))"""
    genome = synth.make_genome("tiny")
    for ml in G.pipe_min_lens(tiny.oix.acc.B, L):
        reads, chain, op = pipe_want(tiny.oix, genome, L, ml)
        one = run_and_peek(tiny.dix, reads, L, ml, native, 1500)
        check_against_oracle(one, chain, op)
        small = run_and_peek(tiny.dix, reads, L, ml, native, 97, peek=False)
        assert np.array_equal(small[0], one[0]) and small[1] == one[1]


# ---------------------------------------------------------------------------
# e. many matches per mate: k_post_fast<8> -> <16> -> k_post, long keys
# ---------------------------------------------------------------------------
def test_pipeline_many_matches_per_mate(tiny, monkeypatch):
    c = G.LONG_CASE
    L, ml, n = c["L"], c["min_len"], c["n_pairs"]
    kw = {k: v for k, v in c.items() if k not in ("L", "n_pairs", "seed", "min_len")}
    reads, chain, op = pipe_want(tiny.oix, synth.make_genome("tiny"), L, ml, n, c["seed"], **kw)
    assert max(len(m) for m in chain.matches) > 16        # (test_geometry_inputs.py)
    runs = []
    for env in ({}, {"SMASH_KEY_HASH_BITS": "2"}, {"SMASH_POST_CAP": "3"}):
        for native in (True, False):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            runs.append(run_and_peek(tiny.dix, reads, L, ml, native, n))
            runs.append(run_and_peek(tiny.dix, reads, L, ml, native, 97, peek=False))
            for k in env:
                monkeypatch.delenv(k)
    for r in runs:
        check_against_oracle(r, chain, op)
        assert np.array_equal(r[0], runs[0][0]) and r[1] == runs[0][1]
    for r in runs[2::2]:
        (nk, keep, hits), (nk0, keep0, hits0) = r[2], runs[0][2]
        assert np.array_equal(nk, nk0) and np.array_equal(keep, keep0)
        for q in np.nonzero(nk0 > 0)[0]:
            assert np.array_equal(hits[q, :nk0[q]], hits0[q, :nk0[q]]), q


# ---------------------------------------------------------------------------
# f. the match hints at their caps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("native", [True, False])
def test_hints_at_their_caps(mid_packed, native, monkeypatch):
    s, c = mid_packed, G.HINT_CASE
    L, n = c["L"], c["n_pairs"]
    if "hint" not in _pipe_want:
        reads = G.case_reads(s.g, c)
        _pipe_want["hint"] = reads, G.Chain(s.oix, reads, mapbin=s.mapbin)
    reads, chain = _pipe_want["hint"]
    assert chain.tag_errors == 0
    rows = device_rows(reads, L, native)
    on = s.device(rows, L, n, True, monkeypatch, native)       # (asserts pipe.map_hints)
    off = s.device(rows, L, n, False, monkeypatch, native)     # SMASH_MAP_HINT=0
    _same_run(on, off)
    counts, st, (nk, keep, hits), (words, nw) = on
    _check_keys(chain.keys, nk, hits)
    for q, exp in enumerate(chain.keys):
        assert nk[q] == (-1 if exp is None else len(exp)), q
        if exp is not None:
            assert bool(keep[q]) == chain.keep[q], q
    # the run did hold matches longer than a hint can say
    slots = L - 20 + 1
    live = np.arange(slots)[None, :] < np.minimum(nw, slots)[:, None]
    assert nw.tolist() == [len(m) for m in chain.matches]
    n_long = sum(1 for m in chain.matches for _ref, _q, ln in m if ln > 127)
    assert n_long > 0 and int(((words[live] >> np.uint64(56)) > 127).sum()) == n_long


# ---------------------------------------------------------------------------
# g. per-read lengths under other row widths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", G.VAR_WIDTHS)
def test_var_len_row_widths(tiny, width):
    """geom_len other than 150 with per-read lengths (launch_sm's
    ws->geom_len branch): zero-padded rows of `width` bytes, dense and native"""
    mates = G.var_len_mates(width)
    n = len(mates) // 2
    exp = V.Chain(tiny.oix, mates)
    assert exp.tag_errors == 0 and exp.key_pairs > 0
    for native in (False, True):
        pipe = make_var_pipe(tiny.dix, width, n, native)
        counts, st, lines, lens = run_var(pipe, V.rows_of(mates, width, pipe.stride), n)
        assert lens.tolist() == [len(m) for m in mates]
        assert counts == exp.counts.tolist()
        assert (st.positions, st.dups, st.kept) == exp.totals
        assert "%d dupes\t%d non-dupes" % (st.dupe_pairs, st.key_pairs - st.dupe_pairs) == exp.summary
        assert lines == exp.lines
        nk, keep, hits = pipe.peek(n)
        _check_keys(exp.keys, nk, hits)
        for q, key in enumerate(exp.keys):
            if key is not None:
                assert bool(keep[q]) == exp.keep[q], q
        pipe.close()
