"""Inputs of tests/test_gpu_samples.py (many samples in one run,
smash_pipeline_samples): runs of pairs with a sample table first[0..S].  TEST
INFRASTRUCTURE; everything here comes from the golden reads, tiny.fa and the
oracle, and tests/test_samples_inputs.py checks on the CPU that the inputs
are what the GPU tests take them for.

Each input is (reads [2 * n, L], first): sample s is pairs
[first[s], first[s + 1])."""
import numpy as np

import key_rows_inputs as K
from conftest import gold, load_bins, load_chrom_sizes

RAGGED_SIZES = (1, 0, 2, 3, 40)   # then the rest of K.dup_reads()


def split(reads, first):
    """the samples' own reads"""
    return [reads[2 * a:2 * b] for a, b in zip(first[:-1], first[1:])]


def replicas():
    """K.dup_reads() three times as three samples: every key of sample 1
    comes again in samples 2 and 3, which one plain run drops whole"""
    one = K.dup_reads()
    n = one.shape[0] // 2
    return np.concatenate([one, one, one]), [0, n, 2 * n, 3 * n]


def ragged():
    """K.dup_reads() cut into samples of 1, 0, 2, 3 and 40 pairs and the rest:
    several boundaries in the first batch, an empty sample, samples that span
    many batches"""
    reads = K.dup_reads()
    first = [0]
    for z in RAGGED_SIZES:
        first.append(first[-1] + z)
    first.append(reads.shape[0] // 2)
    return reads, first


def long_twice():
    """K.long_reads() as sample 1 and again as sample 2: the 24-word keys A
    and B (arena records) occur, and are duplicated, in both"""
    one = K.long_reads()
    n = one.shape[0] // 2
    return np.concatenate([one, one]), [0, n, 2 * n]


# ---- touching: the adjacent chain at a sample boundary ----------------------
# One 20-base segment per mate, on two contigs per pair (K.long_mate rows): a
# pair's key is its two hits and it emits r1's position, then r2's.
_C1 = K.LONG_A[0]                          # 12 places on chr1
_C2 = K.LONG_A[1][:8] + K.LONG_B[1][:8]    # 16 on chr2
_CX = K.LONG_A[1][8:] + K.LONG_B[1][8:]    # 8 on chrX
T_A_LAST = (_C1[0], _C2[0])    # sample A's last pair: its last position is _C2[0]
T_B_FIRST = (_C2[0], _C1[1])   # sample B's first emitting pair: its first position is _C2[0]
T_DUP_1 = (_C1[3], _CX[0])     # inside A, pairs 6 and 7 (two batches): _CX[0] twice in a
T_DUP_2 = (_CX[0], _C1[5])     # row with different keys, a true adjacent duplicate
EMPTY = None                   # a pair of two all-N mates: no key, emits nothing

# variant -> (pairs of A, whether B opens on two pairs that emit nothing)
TOUCHING = {"mid": (10, False),       # the boundary inside the second batch
            "edge": (14, False),      # exactly at a batch boundary: the carried line
            "gap": (10, True),        # lps[q - 1] would reach back into A
            "edge_gap": (14, True)}   # the carried line must not outlive the gap either
TOUCHING_DUPS = (1, 0)                # DupsRemoved of A alone and of B alone


def _filler(k):
    """distinct (chr1, chr2) pairs, none of them T_A_LAST"""
    k += 1
    return (_C1[k % 12], _C2[(k + k // 12) % 16])


def touching_pairs(variant):
    """the pairs of both samples as place tuples (None: EMPTY), and first"""
    na, gap = TOUCHING[variant]
    k = 0
    a = []
    for i in range(na - 1):
        if i == K.BATCH - 1:
            a.append(T_DUP_1)
        elif i == K.BATCH:
            a.append(T_DUP_2)
        else:
            a.append(_filler(k))
            k += 1
    a.append(T_A_LAST)
    b = ([EMPTY, EMPTY] if gap else []) + [T_B_FIRST]
    while len(b) < 6:
        b.append(_filler(k))
        k += 1
    return a + b, [0, na, na + len(b)]


def touching(variant):
    pairs, first = touching_pairs(variant)
    seqs = K.tiny_contigs()
    out = np.full((2 * len(pairs), K.LONG_LEN), ord("z"), np.uint8)
    for q, pr in enumerate(pairs):
        if pr is not None:
            out[2 * q] = K.long_mate(seqs, [pr[0]])
            out[2 * q + 1] = K.long_mate(seqs, [pr[1]])
    return out, first


INPUTS = {"replicas": replicas, "ragged": ragged, "long": long_twice}
INPUTS.update({"touching_" + v: (lambda v=v: touching(v)) for v in TOUCHING})


def tiny_setup():
    """(chrom sizes, bin starts) of the tiny genome"""
    return load_chrom_sizes(gold("tiny_chrom_sizes.txt")), load_bins(gold("tiny_bins.txt"))[1]


def oracle_run(tiny_ix, reads):
    """the oracle chain over reads as one run: (counts, (TotalReads,
    DupsRemoved, ReadsKept), pair duplicates)"""
    import oracle as O
    cs, starts = tiny_setup()
    op = O.Pipeline(tiny_ix, tiny_ix.mappability(), cs, starts)
    if reads.shape[0]:
        assert op.run(reads, threads=4) == 0
    return (op.counts.tolist(), (op.state.total, op.state.dups, op.state.kept),
            int(op.n_dupe.value))
