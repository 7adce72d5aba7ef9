"""The left map.bin byte's bound on the device: mate_fast leaves an
alignment's left byte unloaded when a hint of its match word bounds it and
the bound decides both uses of the byte (csrc/pipeline.hip, DESIGN.md section 3
"The left byte's bound"; the rule and its proof on the CPU: left_bound_inputs.py,
test_left_bound.py).

On the fixtures of test_gpu_rev_hints.py -- the tiny and the mid genome as
8-byte packed indexes, native rows and dense input, 150 / 100 bases and mates
of mixed lengths -- and on left_bound_inputs' bound genome, with that test's
reads plus the hand-made reads for the rule's conditions, at min_excess 4 and
at -3 (the rule compares it in signed arithmetic; a caller may pass any value):
  * counts, stats and every pair's hit list are the same with SMASH_MAP_HINT=1
    (the bound in use) and 0 (every byte loaded);
  * every pair's hit list is the oracle's search -> resolve -> tag ->
    smash_pair at that min_excess, and at min_excess 4, the value the oracle
    pipeline is built with, the counts and totals are the oracle pipeline's.
On the hg19-shaped index (the GEO 150 and GEO 100 kernels): hints on against
off in the same way, and the rule restated on the host over the device's
match words (smash_pipeline_peek_matches): every alignment it skips has its
left byte in the device's own map.bin within [1, b + 1].  The share of
alignments the rule decides there is printed (a measurement, not asserted
beyond being present on both strands)."""
import numpy as np
import pytest

from conftest import interleaved_reads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402
import oracle as O  # noqa: E402
import left_bound_inputs as B  # noqa: E402
import rev_hint_inputs as R  # noqa: E402
import varlen_util as V  # noqa: E402
from test_gpu_rev_hints import (_check_keys, _count, _same_run, _synthetic_subject,  # noqa: E402,F401
                                hg19, mid, tiny)

MIN_EXCESS = (4, -3)


@pytest.fixture(scope="module")
def bound(tmp_path_factory):
    return _synthetic_subject(B.bound_genome(), tmp_path_factory.mktemp("bound"))


_prepared = {}


def _inputs(name, s, L):
    """(reads, per pair its two mates' oracle hit lists); computed once per
    subject and length"""
    if (name, L) in _prepared:
        return _prepared[name, L]
    if name == "tiny":
        parts = [interleaved_reads("s%d" % L)[:400], R.hand_reads(s.oix, L), B.hand_reads(s.oix, L)]
    elif name == "mid":
        parts = [R.synth_reads(s.g, 200, L, seed=131 + L), R.hand_reads(s.oix, L),
                 B.hand_reads(s.oix, L)]
    else:
        parts = [B.bound_genome_reads(s.oix, L)]
    if L == 150 and name != "bound":
        parts.append(R.edge_reads_150(s.oix))
    reads = np.concatenate(parts)
    # a short match between foreign bytes can be shorter than its map bytes,
    # and a zeroed byte reads as 255: mappability_tag throws on both and the
    # whole run is an error (test_gpu_rev_hints._inputs).  The mates the
    # oracle tags without an error go through the pipeline, paired in order
    hits, errs = _oracle_hits(s, [reads[r].tobytes() for r in range(reads.shape[0])])
    ok = [r for r, e in enumerate(errs) if e == 0]
    ok = ok[:len(ok) & ~1]
    assert len(ok) >= 0.5 * len(errs)
    _prepared[name, L] = (np.ascontiguousarray(reads[ok], np.uint8),
                          [(hits[ok[i]], hits[ok[i + 1]]) for i in range(0, len(ok), 2)])
    return _prepared[name, L]


def _oracle_hits(s, mates):
    """per mate its tagged hits and the number of its tag errors"""
    hits, errs = [], []
    for P in mates:
        h, _ = s.oix.resolve(P, s.oix.search(P, min_len=R.MIN_LEN))
        errs.append(sum(1 if O.tag(x, s.offs, s.mapbin, s.small[x.tid]) else 0 for x in h))
        hits.append(h)
    return hits, errs


def _device(s, rows, L, n, hints, me, monkeypatch, native, var_len=False):
    monkeypatch.setenv("SMASH_MAP_HINT", "1" if hints else "0")
    pipe = S.Pipeline(s.dix, s.cs, s.starts, L, n, min_excess=me, dedup_capacity=n,
                      read_stride=S.read_stride(L) if native else 0, var_len=var_len)
    assert pipe.map_hints == hints
    out = _count(pipe, rows, n, len(s.starts))
    pipe.close()
    return out


def _skips(s, words, nw, lens, L, me):
    """alignments of the device's words that the rule skips, per strand (each
    checked against the oracle's map.bin by LeftBound.word)"""
    lb = B.LeftBound(s.oix, s.mapbin)
    slots = L - R.MIN_LEN + 1
    for r in range(words.shape[0]):
        for w in words[r, :min(int(nw[r]), slots)]:
            lb.word(w, int(lens[r]) if lens is not None else L, me)
    return lb.skipped


@pytest.mark.parametrize("me", MIN_EXCESS)
@pytest.mark.parametrize("L", [150, 100])
@pytest.mark.parametrize("name,native", [("tiny", True), ("tiny", False), ("mid", True),
                                         ("bound", True), ("bound", False)])
def test_fixed_length(request, name, native, L, me, monkeypatch):
    s = request.getfixturevalue(name)
    reads, hits = _inputs(name, s, L)
    n = reads.shape[0] // 2
    rows = np.zeros((2 * n, S.read_stride(L) if native else L), np.uint8)
    rows[:, :L] = reads
    on = _device(s, rows, L, n, True, me, monkeypatch, native)
    off = _device(s, rows, L, n, False, me, monkeypatch, native)
    _same_run(on, off)
    counts, st, (nk, keep, dhits), (words, nw) = on
    _check_keys([O.smash_pair(h[0], h[1], min_excess=me) for h in hits], nk, dhits)
    if me == 4:
        op = O.Pipeline(s.oix, s.mapbin, s.cs, s.starts)
        assert op.run(reads, threads=4) == 0
        assert np.array_equal(counts, op.counts)
        assert (st["positions"], st["dups"], st["kept"]) == (op.state.total, op.state.dups,
                                                             op.state.kept)
        assert st["dupe_pairs"] == op.n_dupe.value
    f, r = _skips(s, words, nw, None, L, me)
    print("%s %d min_excess %d: the rule skips %d forward, %d reverse" % (name, L, me, f, r))
    assert f > 0 and r > 0          # the runs above did use the bound


@pytest.mark.parametrize("me", MIN_EXCESS)
@pytest.mark.parametrize("native", [True, False])
def test_mixed_lengths(tiny, native, me, monkeypatch):
    """the variable-length pipeline: mates of 15..150 bases"""
    s, L = tiny, 150
    if ("mixed", L) not in _prepared:
        full = interleaved_reads("s150")[:400]
        rng = np.random.default_rng(7)
        lens = rng.integers(15, L + 1, size=full.shape[0]).astype(np.uint16)
        lens[:4] = (150, 20, 19, 128)
        mates = [full[r, :lens[r]].tobytes() for r in range(full.shape[0])]
        hits, errs = _oracle_hits(s, mates)
        assert sum(errs) == 0
        _prepared["mixed", L] = mates, lens, [(hits[i], hits[i + 1]) for i in range(0, len(hits), 2)]
    mates, lens, hits = _prepared["mixed", L]
    n = len(mates) // 2
    rows = V.rows_of(mates, L, S.read_stride(L) if native else L)
    on = _device(s, rows, L, n, True, me, monkeypatch, native, var_len=True)
    off = _device(s, rows, L, n, False, me, monkeypatch, native, var_len=True)
    _same_run(on, off)
    _check_keys([O.smash_pair(h[0], h[1], min_excess=me) for h in hits], on[2][0], on[2][2])
    f, r = _skips(s, on[3][0], on[3][1], lens, L, me)
    assert f > 0 and r > 0


@pytest.mark.parametrize("L", [150, 100])
def test_geo_kernels_on_hg19(hg19, L, monkeypatch):
    import readgen
    contigs, dix, cs, starts, sp, sz = hg19
    P = 20_000
    d = S.to_rows(readgen.Generator(dix, contigs, L, seed=1300 + L).generate(P), L)
    runs = []
    for hints in (True, False):
        monkeypatch.setenv("SMASH_MAP_HINT", "1" if hints else "0")
        pipe = S.Pipeline(dix, cs, starts, L, P, dedup_capacity=P, read_stride=d.shape[1])
        assert pipe.map_hints == hints
        runs.append(_count(pipe, d, P, len(starts)))
        pipe.close()
    _same_run(runs[0], runs[1])
    words, nw = runs[0][3]
    slots = L - R.MIN_LEN + 1
    w = words[np.arange(slots)[None, :] < np.minimum(nw, slots)[:, None]]
    c = B.decide_words(w, sp, sz, L, min_excess=4)
    i = dix.info
    dmap = S.device_view(i.d_map, i.map_bytes, torch.uint8)

    def entries(at):
        return dmap[torch.from_numpy(np.ascontiguousarray(at)).cuda()].cpu().numpy().astype(np.int64)
    loads = c["kept"] & (2 + 2 * c["g"] < i.map_bytes)       # the parent loads these bytes
    skip = c["skip"]
    assert not (skip & ~loads).any()
    byte = entries(2 + 2 * c["g"][skip])
    assert np.all((byte >= 1) & (byte <= c["b"][skip] + 1))
    assert (skip & c["rc"]).sum() > 1000 and (skip & ~c["rc"]).sum() > 1000
    # the decided share and the rest by cause (printed)
    wide = c["wide"] & loads
    right = entries(2 + 2 * (c["g"][wide] - c["ln"][wide]) + 1)
    right = np.where(right == 0, 255, right)
    passes = c["ln"][wide] - right >= 4
    n, rest = int(loads.sum()), int((loads & ~skip).sum())
    print("hg19-shaped genome, %d pairs of %d bases: %d alignments, %d skip the load (%.1f %%); "
          "of the other %d: no hint %d, contig edge %d, b > len - min_excess with the right "
          "byte passing %d, failing %d"
          % (P, L, n, int(skip.sum()), 100.0 * skip.sum() / n, rest,
             int((c["no_hint"] & loads).sum()), int((c["edge"] & loads).sum()),
             int(passes.sum()), int((~passes).sum())))
