"""The inputs of tests/test_gpu_samples.py are what those tests take them for
(checked with the CPU oracle alone): where the sample boundaries fall, that
every sample does real work, that the samples share keys, and that the
touching samples' adjacent duplicates are the ones stated."""
import pytest

import key_rows_inputs as K
import samples_inputs as SI


def keys_of(tiny_ix, reads):
    return K.host_keys(tiny_ix, reads)


def test_replicas_boundaries_fall_inside_batches(tiny_ix):
    reads, first = SI.replicas()
    assert len(first) == 4 and first[-1] == reads.shape[0] // 2
    assert first[1] % K.BATCH and first[2] % K.BATCH
    one = SI.split(reads, first)[0]
    keep = K.first_wins(keys_of(tiny_ix, one))
    assert sum(keep) > 50 and sum(keep) < len(keep)
    # one plain run keeps nothing of samples 2 and 3
    all_keep = K.first_wins(keys_of(tiny_ix, reads))
    assert all_keep[:first[1]] == keep and not any(all_keep[first[1]:])
    counts, (total, dups, kept), _ = SI.oracle_run(tiny_ix, one)
    assert kept > 0 and sum(counts) == kept


def test_ragged_samples(tiny_ix):
    reads, first = SI.ragged()
    sizes = [b - a for a, b in zip(first[:-1], first[1:])]
    assert tuple(sizes[:5]) == SI.RAGGED_SIZES and sizes[5] > 5 * K.BATCH
    # several boundaries in the first batch, an empty sample, samples over many batches
    assert sum(1 for f in first[1:-1] if f < K.BATCH) >= 4
    assert 0 in sizes and sizes[4] > 2 * K.BATCH
    for part in SI.split(reads, first):
        n = part.shape[0] // 2
        keys = keys_of(tiny_ix, part)
        if n:
            assert any(k is not None for k in keys)        # no sample is empty work
        if n > 10:
            keep = K.first_wins(keys)
            assert sum(k is not None for k in keys) > sum(keep)   # a pair duplicate inside


def test_long_samples_share_their_long_keys(tiny_ix):
    reads, first = SI.long_twice()
    a, b = SI.split(reads, first)
    assert (a == b).all() and first[1] % K.BATCH
    keys = keys_of(tiny_ix, a)
    longs = [k for k in keys if k is not None and len(k) > 16]
    assert len(set(longs)) == 2 and len(longs) == 7       # A and B, each met again


@pytest.mark.parametrize("variant", sorted(SI.TOUCHING))
def test_touching_samples(tiny_ix, variant):
    reads, first = SI.touching(variant)
    pairs, _ = SI.touching_pairs(variant)
    na, gap = SI.TOUCHING[variant]
    assert first[1] == na and (na % K.BATCH == 0) == variant.startswith("edge")
    # the true duplicate inside A straddles the first batch boundary
    assert pairs[K.BATCH - 1] == SI.T_DUP_1 and pairs[K.BATCH] == SI.T_DUP_2
    keys = keys_of(tiny_ix, reads)
    names = tiny_ix.contigs
    for pr, k in zip(pairs, keys):
        if pr is None:
            assert k is None
        else:   # a pair's key is its two segments' hits, r1's first
            assert [(names[t], p) for t, p in k] == [pr[0], pr[1]]
    keyed = [k for k in keys if k is not None]
    assert len(set(keyed)) == len(keyed)                  # no pair duplicates at all
    b0 = na + (2 if gap else 0)
    assert keys[na - 1][-1] == keys[b0][0] and keys[na - 1] != keys[b0]
    assert all(k is None for k in keys[na:b0])
    a, b = SI.split(reads, first)
    ra, rb, whole = (SI.oracle_run(tiny_ix, x) for x in (a, b, reads))
    assert (ra[1][1], rb[1][1]) == SI.TOUCHING_DUPS
    assert whole[1][1] == sum(SI.TOUCHING_DUPS) + 1        # one run: the boundary is a duplicate
    assert ra[1][2] > 0 and rb[1][2] > 0
