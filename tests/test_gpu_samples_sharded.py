"""Many samples across ranks (smash_pipeline_samples_sharded): the sample table
is over the global pair indexes of a multi-GPU run, and every sample must come
out -- its count row and its six counters, summed over the ranks -- exactly as
a run of its own pairs alone.  The yardstick is the plain single pipeline (no
table) over each sample's pairs, which tests/test_gpu_samples.py pins to the
oracle, and for the touching inputs the oracle chain itself
(samples_inputs.oracle_run).  All integers, no tolerance.

The ranks are emulated on one device (tests/phase_emu_samples.py): W
pipelines, the collectives by tensor slicing, dist.ShardedCounter._prev for the
carried line.  The inputs are tests/samples_inputs.py's, unchanged; the
geometries (W, pairs per rank) put the sample boundary where the export, the
owner and the tail logic can go wrong (see GEOMETRIES)."""
import numpy as np
import pytest

import key_rows_inputs as K
import samples_inputs as SI
from conftest import interleaved_reads

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402
from phase_emu import run_emulated  # noqa: E402
from phase_emu_samples import make_pipes, run_sharded, six  # noqa: E402


@pytest.fixture(scope="module")
def gix(tiny_fa):
    return S.Index.from_fasta(tiny_fa)


@pytest.fixture(scope="module")
def setup():
    return SI.tiny_setup()


def own_run(pipe, reads):
    """one plain single-pipeline run over reads in batches of K.BATCH: (counts,
    the six counters)"""
    n = reads.shape[0] // 2
    pipe.reset()
    c = torch.zeros(len(pipe.bins), dtype=torch.int64, device="cuda")
    if n:
        d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    for b0 in range(0, n, K.BATCH):
        b = min(n, b0 + K.BATCH) - b0
        pipe.count_batch(d[2 * b0:2 * (b0 + b)], b, c)
    return c.cpu().numpy().tolist(), six(pipe.stats())


def own_runs(gix, setup, reads, first, var_len=False):
    cs, starts = setup
    pipe = S.Pipeline(gix, cs, starts, reads.shape[1], K.BATCH,
                      dedup_capacity=max(reads.shape[0] // 2, 1), var_len=var_len)
    refs = [own_run(pipe, part) for part in SI.split(reads, first)]
    assert sum(r[1][5] > 0 for r in refs) >= 2   # real work in two samples at least
    return refs


_REFS = {}


@pytest.fixture(scope="module")
def case(gix, setup):
    """name -> (reads, first, the samples' own plain runs): computed once and
    left unchanged"""
    def get(name):
        if name not in _REFS:
            reads, first = SI.INPUTS[name]()
            _REFS[name] = (reads, first, own_runs(gix, setup, reads, first))
        return _REFS[name]
    yield get
    _REFS.clear()


def check(got, refs):
    rows, ss, run = got
    assert len(rows) == len(ss) == len(refs)
    for s, ref in enumerate(refs):
        assert rows[s] == ref[0], "sample %d counts" % s
        assert ss[s] == ref[1], "sample %d statistics" % s
    assert run == tuple(sum(r[1][k] for r in refs) for k in range(6))


def sharded(gix, setup, reads, first, W, B, **kw):
    cs, starts = setup
    return run_sharded(gix, reads, first, W, B, starts, cs, **kw)


# (input, W, pairs per rank): where the boundary falls.  touching_mid and
# touching_gap: A = 10 pairs, B = 6 (gap: B opens on two pairs that emit
# nothing); touching_edge*: A = 14 pairs
GEOMETRIES = [
    ("touching_mid", 2, 5),        # at a step start: the carried line must not cross into B
    ("touching_mid", 3, 5),        # at rank 2's share; the last step short, ranks 1 and 2 empty
    ("touching_mid", 2, 4),        # inside a rank's batch
    ("touching_mid", 4, 1),        # shares of one pair
    ("touching_gap", 3, 5),        # a rank opens on pairs that emit nothing: the previous
    ("touching_gap", 4, 1),        # rank's tail is A's and must be ignored; one-pair shares
    ("touching_edge", 2, 7),       # the true adjacent duplicate of pairs 6 and 7 straddles a
    ("touching_edge_gap", 2, 7),   # rank boundary inside A; the A/B boundary at a step start
]


@pytest.mark.parametrize("name,W,B", GEOMETRIES)
def test_boundary_geometries(gix, setup, tiny_ix, case, name, W, B):
    reads, first, refs = case(name)
    got = sharded(gix, setup, reads, first, W, B)
    check(got, refs)
    rows, ss, _ = got
    for s, part in enumerate(SI.split(reads, first)):   # and the oracle chain per sample
        counts, totals, _ = SI.oracle_run(tiny_ix, part)
        assert rows[s] == counts and ss[s][3:6] == totals
    assert (ss[0][4], ss[1][4]) == SI.TOUCHING_DUPS


@pytest.mark.parametrize("W,B", [(1, 7), (2, 50), (3, 7)])
@pytest.mark.parametrize("name", ["replicas", "ragged", "long"])
def test_samples_equal_their_own_runs(gix, setup, case, name, W, B):
    reads, first, refs = case(name)
    check(sharded(gix, setup, reads, first, W, B), refs)


@pytest.mark.parametrize("W,B", [(2, 7), (3, 50)])
@pytest.mark.parametrize("name", ["replicas", "ragged", "long"])
def test_two_hash_bits(gix, setup, case, name, W, B, monkeypatch):
    """SMASH_KEY_HASH_BITS=2: the salted hash has two values, so an owner's
    every probe walk meets the other samples' keys of the same words and must
    tell them apart by sample and words; long: arena records of 24 words in
    two samples"""
    monkeypatch.setenv("SMASH_KEY_HASH_BITS", "2")
    reads, first, refs = case(name)
    check(sharded(gix, setup, reads, first, W, B), refs)


def test_plain_sharded_run_is_not_the_samples(gix, setup, case):
    """what the table is for: the replicas through the plain sharded run lose
    samples 2 and 3 whole (every key is a duplicate of sample 1's), with the
    table every replica counts like the first"""
    reads, first, refs = case("replicas")
    plain_rows, _, plain_run = sharded(gix, setup, reads, None, 2, 7)
    assert plain_rows[0] == refs[0][0]          # only sample 1 is counted
    assert plain_run[5] == refs[0][1][5]
    rows, ss, run = sharded(gix, setup, reads, first, 2, 7)
    assert rows[0] == rows[1] == rows[2] == refs[0][0]
    assert run[5] == 3 * plain_run[5] and plain_run[2] > run[2]


@pytest.mark.parametrize("ahead2", [False, True], ids=["ahead", "ahead2"])
def test_look_ahead_searches(gix, setup, case, ahead2):
    """the next batch's search issued with this one's (smash_phase_map_ahead),
    and the one after it right after the export (smash_phase_search_ahead)"""
    reads, first, refs = case("ragged")
    check(sharded(gix, setup, reads, first, 2, 7, ahead=True, ahead2=ahead2), refs)


def test_variable_length_mode(gix, setup):
    """ragged over trimmed copies of its reads (the v150 trim rule), variable-
    length mode on, two ranks"""
    from varlen_reads import vlen
    from varlen_util import rows_of
    reads, first = SI.ragged()
    mates = []
    for r in reads:
        s = r.tobytes()
        mates.append(s[:vlen(s.upper().replace(b"Z", b"N"))])
    assert len({len(m) for m in mates}) > 20
    rows = rows_of(mates, reads.shape[1])
    refs = own_runs(gix, setup, rows, first, var_len=True)
    assert sum(r[1][5] > 0 for r in refs) >= 3
    check(sharded(gix, setup, rows, first, 2, 7, var_len=True), refs)


def test_full_owner_set_fails_loudly(gix, setup, case):
    """each rank's key set sized for one batch of 7 pairs (16 slots), ragged's
    keys over two owners: SMASH_ERR_NOMEM is recorded and no counts come back"""
    reads, first, _ = case("ragged")
    with pytest.raises(S.SmashError, match="key set full"):
        sharded(gix, setup, reads, first, 2, 7, capacity=7)


def test_errors(gix, setup, case):
    reads, first, refs = case("ragged")
    cs, starts = setup
    n = reads.shape[0] // 2
    pipe = S.Pipeline(gix, cs, starts, reads.shape[1], K.BATCH, dedup_capacity=n)
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    c = torch.zeros((len(first) - 1, len(starts)), dtype=torch.int64, device="cuda")

    def code(fn):
        with pytest.raises(S.SmashError) as e:
            fn()
        return e.value.code

    pipe.reset()
    assert pipe.hdr_words == 1 and S.lib().smash_phase_hdr_words(pipe.h) == 1
    assert code(lambda: pipe.set_samples_sharded([0, 5, 3, n])) == S.SMASH_ERR_ARG   # descending
    assert code(lambda: pipe.set_samples_sharded([1, 5, n])) == S.SMASH_ERR_ARG      # first[0] != 0
    assert code(lambda: pipe.set_samples_sharded(list(range(65537)))) == S.SMASH_ERR_ARG
    pipe.set_samples_sharded(first)
    assert pipe.hdr_words == 2 and pipe.tail_words == 3
    # the single-GPU batch calls know no global index
    assert code(lambda: pipe.count_batch(d[:2 * K.BATCH], K.BATCH, c)) == S.SMASH_ERR_UNSUPPORTED
    assert code(lambda: pipe.count_batches(d, n, K.BATCH, c)) == S.SMASH_ERR_UNSUPPORTED
    # mid-run: once a phase call has taken pairs
    pipe.phase_map(d[:2 * K.BATCH], K.BATCH)
    assert code(lambda: pipe.set_samples_sharded(first)) == S.SMASH_ERR_ARG
    assert code(lambda: pipe.set_samples_sharded(None)) == S.SMASH_ERR_ARG
    assert code(lambda: pipe.set_samples(first)) == S.SMASH_ERR_ARG
    # an export past first[S]
    pipe.reset()
    pipe.set_samples_sharded([0, 3, 5])
    pipe.phase_map(d[:2 * K.BATCH], K.BATCH)
    assert code(lambda: pipe.phase_export(1, 0)) == S.SMASH_ERR_ARG
    assert code(lambda: pipe.phase_export(2, 5)) == S.SMASH_ERR_ARG
    # one kind of table at a time: smash_pipeline_samples' replaces the sharded one
    pipe.reset()
    pipe.set_samples(first)
    assert pipe.hdr_words == 1
    assert code(lambda: pipe.phase_map(d[:2 * K.BATCH], K.BATCH)) == S.SMASH_ERR_UNSUPPORTED
    pipe.set_samples(None)


def test_table_off_again(gix, setup, case):
    """pipelines that ran with a sharded table, the table cleared: their plain
    sharded run is phase_emu.run_emulated's over fresh pipelines"""
    reads, first, refs = case("ragged")
    cs, starts = setup
    s100 = interleaved_reads("s100")[:2 * 200]
    pipes = make_pipes(gix, cs, starts, reads.shape[1], 2, 50, 200)
    check(run_sharded(gix, reads, first, 2, 50, starts, cs, pipes=pipes), refs)
    pipes = make_pipes(gix, cs, starts, s100.shape[1], 2, 50, 200)
    run_sharded(gix, s100, [0, 120, 200], 2, 50, starts, cs, pipes=pipes)
    rows, ss, run = run_sharded(gix, s100, None, 2, 50, starts, cs, pipes=pipes)
    total, st = run_emulated(gix, s100, 2, 50, 2, starts, cs)
    assert ss == [] and [p.sample_stats() for p in pipes] == [[], []]
    assert rows[0] == total.tolist()
    assert (run[3], run[4], run[5], run[2]) == st
