"""The host side of many samples across ranks, without a GPU
(smash-paper_amd/dist.py): the carried {pos0, sample} line, the packing of a
rank's share from the samples it overlaps, and ShardedCounter(samples=...) with
count_fastq_many over torch.distributed/gloo, two ranks, against a sample-aware
oracle-backed stand-in for the pipeline (tests/mock_samples.py).  The expected
values are each sample's own oracle run.

(smash_cli.py count-many under a multi-rank launch opens an RCCL process group
and a device pipeline: it cannot run on gloo without a GPU, so the CLI's
multi-rank form has no test here.)"""
import os
import queue as _queue

import numpy as np
import pytest

import key_rows_inputs as K
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, gold, interleaved_reads, load_bins, load_chrom_sizes
from dist import ShardedCounter, count_fastq_many, sample_first, sample_spans


def _port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def t(rows):
    return torch.tensor(rows, dtype=torch.int64)


def test_prev_carries_position_and_sample():
    prev = ShardedCounter._prev
    carried = t([77, 4])
    tails = t([[3, 100, 1], [0, -1, -1], [2, 250, 2], [0, -1, -1]])
    assert prev(tails, carried).tolist() == [250, 2]          # the latest non-empty shard
    assert prev(tails[:2], carried).tolist() == [100, 1]      # an empty shard is passed over
    assert prev(tails[:1], carried).tolist() == [100, 1]
    assert prev(tails[1:2], carried).tolist() == [77, 4]      # all shards empty: the carried pair
    assert prev(tails[:0], carried).tolist() == [77, 4]       # rank 0: no shard before it
    assert prev(t([[0, -1, -1]] * 3), t([-1, -1])).tolist() == [-1, -1]
    # two-word tails keep their meaning
    assert prev(t([[1, 5], [0, -1]]), t([9])).tolist() == [5]
    assert prev(t([[0, -1], [0, -1]]), t([9])).tolist() == [9]


def test_sample_spans_by_hand():
    first = [0, 4, 4, 9, 10, 30]          # samples of 4, 0, 5, 1 and 20 pairs
    assert sample_spans(first, 0, 4) == [(0, 0, 4, 0)]
    assert sample_spans(first, 2, 7) == [(0, 2, 4, 0), (2, 0, 3, 2)]         # over the empty one
    assert sample_spans(first, 3, 12) == [(0, 3, 4, 0), (2, 0, 5, 1), (3, 0, 1, 6), (4, 0, 2, 7)]
    assert sample_spans(first, 8, 11) == [(2, 4, 5, 0), (3, 0, 1, 1), (4, 0, 1, 2)]  # three samples
    assert sample_spans(first, 12, 20) == [(4, 2, 10, 0)]
    assert sample_spans(first, 30, 30) == []
    assert sample_spans([0, 0, 3], 0, 3) == [(1, 0, 3, 0)]                   # a leading empty sample


class ArrayIndex:
    """smashgpu.FastqIndex's plan over an array of pairs"""

    def __init__(self, reads):
        self.reads = reads
        self.n, self.L = reads.shape[0] // 2, reads.shape[1]

    def pack(self, k0, k1, out):
        assert 0 <= k0 <= k1 <= self.n
        out[:2 * (k1 - k0)] = torch.from_numpy(self.reads[2 * k0:2 * k1].copy())


class Recorder:
    """a ShardedCounter's face towards count_fastq_many: keeps every step's reads"""

    def __init__(self, rank, world, first):
        self.rank, self.world, self.samples = rank, world, first
        self.device = torch.device("cpu")
        self.steps = []

    def step(self, d_reads, n_pairs, step_base, d_counts, next_reads=None, next_pairs=0,
             stride=None, **kw):
        assert d_reads.shape[0] == 2 * n_pairs
        self.steps.append((step_base + self.rank * stride, d_reads.clone().numpy()))

    def finish(self):
        pass


@pytest.mark.parametrize("look_ahead", [True, False])
def test_count_fastq_many_packs_the_global_plan(look_ahead):
    """five samples (one empty) over three ranks with batches of 4: shares
    straddle up to three samples, the last step is short, and the ranks'
    shares put back in (step, rank) order are the samples one after the other"""
    rng = np.random.default_rng(5)
    sizes = [4, 0, 5, 1, 20]
    parts = [rng.integers(97, 123, (2 * z, 11), dtype=np.uint8) for z in sizes]
    ixs = [ArrayIndex(p) for p in parts]
    first = sample_first(ixs)
    assert first == [0, 4, 4, 9, 10, 30]
    plan = np.concatenate(parts)
    W, B = 3, 4
    recs = [Recorder(r, W, first) for r in range(W)]
    done = [count_fastq_many(rc, ixs, B, None, look_ahead=look_ahead) for rc in recs]
    assert sum(done) == 30
    assert len({len(rc.steps) for rc in recs}) == 1 and len(recs[0].steps) == 3
    got = sorted((x for rc in recs for x in rc.steps if len(x[1])), key=lambda x: x[0])
    at = 0
    for base, rows in got:
        assert base == at
        assert (rows == plan[2 * at:2 * at + len(rows)]).all()
        at += len(rows) // 2
    assert at == 30
    assert [len(x[1]) // 2 for x in recs[1].steps] == [4, 4, 2]   # a short share
    assert [len(x[1]) // 2 for x in recs[2].steps] == [4, 4, 0]   # and an empty one
    with pytest.raises(ValueError):
        count_fastq_many(Recorder(0, W, [0, 30]), ixs, B, None)


# ---- two ranks over gloo -------------------------------------------------------
SIZES = (130, 0, 127, 143)   # pairs per sample; sample 3 repeats sample 0's pairs
BATCH = 97                   # 400 pairs over 2 ranks: 3 steps, the last 12 + 0 pairs


def lane():
    s100 = interleaved_reads("s100")
    parts = [s100[:2 * 130], s100[:0], s100[2 * 130:2 * 257], s100[:2 * 143]]
    assert tuple(p.shape[0] // 2 for p in parts) == SIZES
    return parts


def _worker(rank, world, port, out_q):
    import sys
    for p in ("oracle", "tools", "tests", "smash-paper_amd"):
        sys.path.insert(0, os.path.join(ROOT, p))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import gzip, tempfile
    import oracle as O
    from mock_samples import SampleOraclePipeline
    d = tempfile.mkdtemp()
    fa = os.path.join(d, "tiny.fa")
    with gzip.open(gold("tiny.fa.gz"), "rb") as f, open(fa, "wb") as g:
        g.write(f.read())
    oix = O.Index.from_fasta(fa)
    _, starts = load_bins(gold("tiny_bins.txt"))
    cs = load_chrom_sizes(gold("tiny_chrom_sizes.txt"))
    ixs = [ArrayIndex(p) for p in lane()]
    first = sample_first(ixs)
    pipe = SampleOraclePipeline(oix, oix.mappability(), cs, starts, BATCH)
    sc = ShardedCounter(pipe, rank, world, torch.device("cpu"), samples=first)
    out = []
    for look_ahead in (True, False):   # two runs over one counter: the table stays set
        sc.reset()
        counts = torch.zeros((len(ixs), len(starts)), dtype=torch.int64)
        count_fastq_many(sc, ixs, BATCH, counts, look_ahead=look_ahead)
        dist.all_reduce(counts)
        out.append((counts.numpy().tolist(), sc.sample_stats()))
    if rank == 0:
        out_q.put(out)
    dist.destroy_process_group()


def test_two_ranks_equal_the_samples_own_runs(tiny_ix):
    import oracle as O
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    # the expected values meanwhile: every sample's own oracle run
    _, starts = load_bins(gold("tiny_bins.txt"))
    cs = load_chrom_sizes(gold("tiny_chrom_sizes.txt"))
    want, keyed = [], []
    for part in lane():
        op = O.Pipeline(tiny_ix, tiny_ix.mappability(), cs, starts)
        if part.shape[0]:
            assert op.run(part, threads=4) == 0
        keyed.append(sum(k is not None for k in K.host_keys(tiny_ix, part)))
        want.append((op.counts.tolist(), part.shape[0] // 2, int(op.n_dupe.value),
                     [op.state.total, op.state.dups, op.state.kept]))
    res = None
    for _ in range(600):
        try:
            res = q.get(timeout=1)
            break
        except _queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        if res is None:
            p.terminate()
    assert res is not None, [p.exitcode for p in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert want[3][3][2] > 0 and want[0][3][2] > 0   # the repeated pairs count in both samples
    for rows, stats in res:
        for s, (counts, pairs, dupes, totals) in enumerate(want):
            keyed_s = keyed[s]
            assert rows[s] == counts, "sample %d counts" % s
            assert stats[s][0] == pairs and stats[s][2] == dupes and stats[s][3:6] == totals
            assert stats[s][1] == keyed_s, "sample %d key_pairs" % s
