"""The key set's row records (csrc/keyset.hpp): a pair key of at most 16 hit
words stays in its pair's head row for the whole run and its slot names the
pair; only longer keys are copied into the arena.  Every case runs on the
tiny index; counts, statistics and every pair's keep flag must equal a
one-batch run's, the keep flags the first-wins rule over the oracle's keys,
and the counts the oracle chain's (tests/key_rows_inputs.py builds the
inputs, tests/test_key_rows_inputs.py checks them on the CPU)."""
import numpy as np
import pytest

import key_rows_inputs as K
from conftest import gold, load_bins, load_chrom_sizes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import oracle as O  # noqa: E402
import smashgpu as S  # noqa: E402


@pytest.fixture(scope="module")
def gix(tiny_fa):
    return S.Index.from_fasta(tiny_fa)


@pytest.fixture(scope="module")
def setup():
    _, starts = load_bins(gold("tiny_bins.txt"))
    return load_chrom_sizes(gold("tiny_chrom_sizes.txt")), starts


def stat_tuple(st):
    return (st.pairs, st.key_pairs, st.dupe_pairs, st.positions, st.dups, st.kept, st.matches)


def run(gix, setup, reads, batch, how="batch", capacity=None, pipe=None, d=None):
    """reads through a pipeline in batches of `batch` pairs ->
    (counts, statistics, keep flags of the keyed pairs, nk).  how: "batch"
    (smash_count_batch per batch), "phases" (the phase calls, an owner of a
    world of one) or "batches" (smash_count_batches; no per-pair flags)."""
    cs, starts = setup
    n = reads.shape[0] // 2
    if d is None:
        d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    if pipe is None:
        pipe = S.Pipeline(gix, cs, starts, reads.shape[1], batch, dedup_capacity=capacity or n)
    pipe.reset()
    c = torch.zeros(len(starts), dtype=torch.int64, device="cuda")
    keep, nks = [], []
    if how == "batches":
        pipe.count_batches(d, n, batch, c)
    else:
        tail = torch.empty(2, dtype=torch.int64, device="cuda")
        for b0 in range(0, n, batch):
            b = min(n, b0 + batch) - b0
            if how == "phases":
                pipe.phase_map(d[2 * b0:2 * (b0 + b)], b)
                hdr, words, cnt, wcnt = pipe.phase_export(1, b0)
                flags = torch.empty(max(int(cnt.sum()), 1), dtype=torch.uint8, device="cuda")
                pipe.dedup_owner(hdr.clone(), int(cnt.sum()), words.clone(), cnt, wcnt, flags)
                pipe.phase_import(flags)
                pipe.phase_positions(tail)
                pipe.phase_bin(None, c)
            else:
                pipe.count_batch(d[2 * b0:2 * (b0 + b)], b, c)
            nk, kp, _ = pipe.peek(b)
            nks += nk.tolist()
            # (an unkeyed pair's flag is not compared: the owner path never writes it)
            keep += [bool(k) and m >= 0 for k, m in zip(kp.tolist(), nk.tolist())]
    st = pipe.stats()
    return c.cpu().numpy().tolist(), stat_tuple(st), keep, nks


def oracle_chain(tiny_ix, setup, reads):
    cs, starts = setup
    op = O.Pipeline(tiny_ix, tiny_ix.mappability(), cs, starts)
    assert op.run(reads, threads=4) == 0
    return op.counts.tolist(), (op.state.total, op.state.dups, op.state.kept)


@pytest.fixture(scope="module")
def dup_case(gix, setup, tiny_ix):
    """the duplicates input, its one-batch run, the first-wins flags over the
    oracle's keys and the oracle chain's counts: computed once, read only"""
    reads = K.dup_reads()
    n = reads.shape[0] // 2
    one = run(gix, setup, reads, n)
    keep = K.first_wins(K.host_keys(tiny_ix, reads))
    chain = oracle_chain(tiny_ix, setup, reads)
    assert one[2] == keep
    assert (one[0], one[1][3:6]) == chain
    return reads, one


@pytest.fixture(scope="module")
def long_case(gix, setup, tiny_ix):
    reads = K.long_reads()
    n = reads.shape[0] // 2
    one = run(gix, setup, reads, n)
    keep = K.first_wins(K.host_keys(tiny_ix, reads))
    chain = oracle_chain(tiny_ix, setup, reads)
    assert one[2] == keep
    assert (one[0], one[1][3:6]) == chain
    assert [m for w, m in zip(K.LONG_ORDER, one[3]) if w in ("A", "B")] == [24] * 7
    return reads, one


@pytest.mark.parametrize("bits", [0, 2, 1])
def test_ragged_batches(gix, setup, dup_case, bits, monkeypatch):
    """Batches of 7 pairs and a ragged last one; duplicates inside a batch
    (claims lowered by atomicMin) and of pairs of earlier batches (rows below
    row_base).  bits > 0: the key hash cut to `bits` bits (SMASH_KEY_HASH_BITS),
    so that every probe walk meets other keys' rows and must compare words."""
    if bits:
        monkeypatch.setenv("SMASH_KEY_HASH_BITS", str(bits))
    reads, one = dup_case
    assert (reads.shape[0] // 2) % K.BATCH
    assert run(gix, setup, reads, K.BATCH) == one


@pytest.mark.parametrize("bits", [0, 2])
@pytest.mark.parametrize("how", ["batch", "phases"])
def test_long_keys(gix, setup, long_case, how, bits, monkeypatch):
    """Pairs of 24 hit words (arena records) among row keys: first met, met
    again in the same and in later batches, two long keys that share their
    first 12 words; with 2 hash bits they share slots' hashes with row keys.
    how = phases: the same input through an owner's arena."""
    if bits:
        monkeypatch.setenv("SMASH_KEY_HASH_BITS", str(bits))
    reads, one = long_case
    assert run(gix, setup, reads, K.BATCH, how) == one


@pytest.mark.parametrize("bits", [0, 2])
def test_rows_grow_mid_run(gix, setup, dup_case, bits, monkeypatch):
    """A capacity of one batch: the rows, their word counts and the table
    grow several times mid-run with keys in place (smash_count_batch grows
    the set before it queues a batch the rows could not hold); and an explicit
    smash_pipeline_reserve_keys between two batches.  bits = 2: the words are
    compared against moved rows of other keys too."""
    if bits:
        monkeypatch.setenv("SMASH_KEY_HASH_BITS", str(bits))
    cs, starts = setup
    reads, one = dup_case
    n = reads.shape[0] // 2
    pipe = S.Pipeline(gix, cs, starts, reads.shape[1], K.BATCH, dedup_capacity=1)
    cap0 = pipe.key_capacity
    assert cap0 < n
    assert run(gix, setup, reads, K.BATCH, pipe=pipe) == one
    assert pipe.key_capacity >= n
    # grown by hand half way, the second half's duplicates are of moved rows
    pipe = S.Pipeline(gix, cs, starts, reads.shape[1], K.BATCH, dedup_capacity=n)
    pipe.reset()
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    c = torch.zeros(len(starts), dtype=torch.int64, device="cuda")
    keep = []
    for b0 in range(0, n, K.BATCH):
        b = min(n, b0 + K.BATCH) - b0
        if b0 == 9 * K.BATCH:
            pipe.reserve_keys(8 * n)
            assert pipe.key_capacity >= 8 * n
        pipe.count_batch(d[2 * b0:2 * (b0 + b)], b, c)
        nk, kp, _ = pipe.peek(b)
        keep += [bool(k) and m >= 0 for k, m in zip(kp.tolist(), nk.tolist())]
    assert (c.cpu().numpy().tolist(), stat_tuple(pipe.stats()), keep) == one[:3]


@pytest.mark.parametrize("bits", [0, 2])
def test_reset_between_runs(gix, setup, dup_case, bits, monkeypatch):
    """Two runs queued back to back over resident reads with a reset between
    them: the second run's rows land where the first's were; then a run over
    the pairs in another order on the same pipeline: its result is a fresh
    pipeline's, so no key came from the rows of the runs before."""
    if bits:
        monkeypatch.setenv("SMASH_KEY_HASH_BITS", str(bits))
    cs, starts = setup
    reads, one = dup_case
    n = reads.shape[0] // 2
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    torch.cuda.synchronize()
    pipe = S.Pipeline(gix, cs, starts, reads.shape[1], K.BATCH, dedup_capacity=n)
    cs_ = [torch.zeros(len(starts), dtype=torch.int64, device="cuda") for _ in range(2)]
    for c in cs_:
        pipe.reset()
        pipe.count_batches(d, n, K.BATCH, c, resident=True)
    st = stat_tuple(pipe.stats())
    for c in cs_:
        assert c.cpu().numpy().tolist() == one[0]
    assert st == one[1]
    # the pairs rotated by 10: other pairs are first now
    rot = np.ascontiguousarray(np.roll(reads, -20, axis=0))
    assert run(gix, setup, rot, K.BATCH, pipe=pipe) == run(gix, setup, rot, n)


def test_phase_calls_equal_count_batches(gix, setup, dup_case):
    reads, one = dup_case
    assert run(gix, setup, reads, K.BATCH, "phases") == one
    got = run(gix, setup, reads, K.BATCH, "batches")
    assert got[:2] == one[:2]


def test_long_keys_out_of_arena(gix, setup, long_case, monkeypatch):
    """An arena of 30 words holds the first long key's record (26 words) and
    not the second's: the run records SMASH_ERR_NOMEM (every store is checked
    against the arena's end first) and reading its statistics raises."""
    monkeypatch.setenv("SMASH_KEY_ARENA_WORDS", "30")
    cs, starts = setup
    reads, _ = long_case
    n = reads.shape[0] // 2
    pipe = S.Pipeline(gix, cs, starts, reads.shape[1], K.BATCH, dedup_capacity=n)
    pipe.reset()
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    c = torch.zeros(len(starts), dtype=torch.int64, device="cuda")
    pipe.count_batches(d, n, K.BATCH, c)
    assert pipe.stats(raise_on_error=False).error == S.SMASH_ERR_NOMEM
    with pytest.raises(S.SmashError, match="key set full"):
        pipe.stats()
