"""The inputs of tests/test_gpu_key_rows.py are what those tests take them
for (checked with the CPU oracle): duplicates inside a batch and across
batches, a ragged last batch, and long pairs of 24 hit words each."""
import key_rows_inputs as K


def batches_of(flags):
    return [flags[i:i + K.BATCH] for i in range(0, len(flags), K.BATCH)]


def test_dup_input_has_both_kinds_of_duplicates(tiny_ix):
    reads = K.dup_reads()
    keys = K.host_keys(tiny_ix, reads)
    n = len(keys)
    assert n % K.BATCH and n > 10 * K.BATCH
    keep = K.first_wins(keys)
    first = {}
    in_batch = later = 0
    for q, k in enumerate(keys):
        if k is None:
            continue
        if k in first:
            if first[k] // K.BATCH == q // K.BATCH:
                in_batch += 1
            else:
                later += 1
        else:
            first[k] = q
    assert in_batch >= 5 and later >= 20
    assert all(len(k) <= 16 for k in first)     # row keys only
    assert sum(keep) == len(first)


def test_long_pairs_have_long_keys(tiny_ix):
    reads = K.long_reads()
    keys = K.host_keys(tiny_ix, reads)
    by = {}
    for what, k in zip(K.LONG_ORDER, keys):
        by.setdefault(what, set()).add(k)
    assert all(len(v) == 1 for v in by.values())
    a, b = next(iter(by["A"])), next(iter(by["B"]))
    assert len(a) == 24 and len(b) == 24 and a != b and a[:12] == b[:12]
    short = [k for what, k in zip(K.LONG_ORDER, keys) if what not in ("A", "B")]
    assert all(k is None or len(k) <= 16 for k in short)
    assert sum(k is not None for k in short) >= 15
    # every batch that holds a long pair holds short keys too
    for ws, ks in zip(batches_of(K.LONG_ORDER), batches_of(keys)):
        if "A" in ws or "B" in ws:
            assert any(w not in ("A", "B") and k is not None for w, k in zip(ws, ks))
