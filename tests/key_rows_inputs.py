"""Inputs of tests/test_gpu_key_rows.py (the key set's row records): pair
lists with duplicates of earlier pairs, inside one batch and in later ones,
and pairs whose key has more than 16 hit words.  TEST INFRASTRUCTURE; the
CPU side (tests/test_key_rows_inputs.py) checks with the oracle that the
inputs are what the GPU tests take them for."""
import gzip

import numpy as np

from conftest import gold, interleaved_reads

BATCH = 7          # pairs per batch of the ragged runs
LONG_LEN = 255     # mate length of the long-key input

# 20-base segments of tiny.fa, (contig, 0-based start): each alone is a unique
# match that passes the excess-mappability filter, no two of one pair's r1 and
# r2 share a contig (the hit window drops nothing), so a pair of two mates of
# twelve segments keeps 24 hits
LONG_A = ([("chr1", p) for p in (2000, 11500, 32000, 47000, 54500, 59000, 69000, 74500, 81000,
                                 102000, 108000, 113000)],
          [("chr2", p) for p in (1000, 10000, 19000, 26500, 35000, 55000, 65000, 73500)] +
          [("chrX", p) for p in (1000, 13500, 30000, 46500)])
# a second long key: the same r1, another r2 (its first 12 words equal A's)
LONG_B = (LONG_A[0],
          [("chr2", p) for p in (2000, 11000, 20000, 27500, 36000, 57000, 66000, 74500)] +
          [("chrX", p) for p in (3000, 14500, 32000, 48000)])


def dup_order(n_base=90):
    """indices into the first n_base pairs of s150: every pair once, in order,
    some repeated at once (the same batch of BATCH, or across its end), some
    repeated 20 pairs on (a later batch), and the first 15 again at the end"""
    order = []
    for i in range(n_base):
        order.append(i)
        if i % 9 == 4:
            order.append(i)
        if i % 11 == 7 and i >= 20:
            order.append(i - 20)
    order += list(range(15))
    return order


def dup_reads():
    """[2 * n, 150] mates of dup_order(), n no multiple of BATCH"""
    base = interleaved_reads("s150")
    order = dup_order()
    assert len(order) % BATCH
    out = np.empty((2 * len(order), base.shape[1]), np.uint8)
    for k, i in enumerate(order):
        out[2 * k] = base[2 * i]
        out[2 * k + 1] = base[2 * i + 1]
    return out


def tiny_contigs():
    seqs, name = {}, None
    with gzip.open(gold("tiny.fa.gz"), "rt") as f:
        for l in f:
            l = l.strip()
            if l.startswith(">"):
                name = l[1:].split()[0]
                seqs[name] = []
            else:
                seqs[name].append(l)
    return {k: "".join(v).upper() for k, v in seqs.items()}


def long_mate(seqs, places):
    """the segments joined by one N each, N up to LONG_LEN (N -> z: no match
    runs across a joint)"""
    s = "N".join(seqs[c][p:p + 20] for c, p in places)
    assert len(s) <= LONG_LEN
    return np.frombuffer((s + "N" * (LONG_LEN - len(s))).replace("N", "Z").lower().encode(),
                         np.uint8)


# the long-key input's pairs: ("s", i) = pair i of s150, its mates padded with
# N to LONG_LEN (short keys); "A" / "B" = the long pairs.  Batches of BATCH:
# A first in batch 0 among short keys, B in batch 1, A again in batch 1 (a
# duplicate of an arena record), B again in batch 2 and twice in batch 3
LONG_ORDER = ([("s", 0), ("s", 1), "A", ("s", 2), ("s", 3), ("s", 1), ("s", 4)] +
              [("s", 5), "B", ("s", 6), "A", ("s", 0), ("s", 7), ("s", 8)] +
              [("s", 9), ("s", 10), "B", ("s", 11), ("s", 5), ("s", 12), ("s", 13)] +
              ["B", ("s", 14), "B", "A", ("s", 15)])


def long_reads():
    """[2 * n, LONG_LEN] mates of LONG_ORDER"""
    base = interleaved_reads("s150")
    seqs = tiny_contigs()
    longs = {k: (long_mate(seqs, v[0]), long_mate(seqs, v[1]))
             for k, v in (("A", LONG_A), ("B", LONG_B))}
    out = np.full((2 * len(LONG_ORDER), LONG_LEN), ord("z"), np.uint8)
    for k, what in enumerate(LONG_ORDER):
        if what in longs:
            out[2 * k], out[2 * k + 1] = longs[what]
        else:
            i = what[1]
            out[2 * k, :base.shape[1]] = base[2 * i]
            out[2 * k + 1, :base.shape[1]] = base[2 * i + 1]
    return out


def host_keys(oix, reads):
    """per pair its key (a tuple of (tid, pos0)) or None, by the oracle's
    search -> resolve -> tag -> smashMEM pair filter"""
    import oracle as O
    mapbin = oix.mappability()
    sizes = [int(x) for x in oix.sizes[0::2]]
    offs = np.cumsum([0] + sizes[:-1]).astype(np.uint32)
    small = [1 if ("_gl000" in c or "chrM" in c) else 0 for c in oix.contigs]
    out = []
    for q in range(reads.shape[0] // 2):
        hs = []
        for m in (0, 1):
            P = reads[2 * q + m].tobytes()
            h, _ = oix.resolve(P, oix.search(P))
            for x in h:
                O.tag(x, offs, mapbin, small[x.tid])
            hs.append(h)
        k = O.smash_pair(hs[0], hs[1])
        out.append(None if k is None else tuple(k))
    return out


def first_wins(keys):
    """keep flags of smashMEM.py:217-228 over the keys in order"""
    seen, keep = set(), []
    for k in keys:
        keep.append(k is not None and k not in seen)
        if k is not None:
            seen.add(k)
    return keep
