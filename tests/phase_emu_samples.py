"""tests/phase_emu.py's in-process emulation for a run with a sharded sample
table (smash_pipeline_samples_sharded; TEST INFRASTRUCTURE): W pipelines on
one device share one index, the collectives of smash-paper_amd/dist.py become
tensor slicing.  It carries what the table adds -- the same table on every
rank, headers of the queried width, three-word tails -- and, unlike
phase_emu.run_emulated, deals a run of any length as dist.count_fastq does:
rank r's share of step s is the global pairs [min(n, s W B + r B), + B) cut at
n, so a short last step leaves ranks with part of a batch or none.  The
carried line is dist.ShardedCounter._prev's, not restated here."""
import numpy as np
import torch

import smashgpu as S
from dist import ShardedCounter
from phase_emu import _rows

FIELDS = ("pairs", "key_pairs", "dupe_pairs", "positions", "dups", "kept")


def six(st):
    return tuple(int(getattr(st, f)) for f in FIELDS)


def make_pipes(ix, cs, starts, L, W, per_rank, capacity, var_len=False):
    return [S.Pipeline(ix, cs, starts, L, per_rank, dedup_capacity=capacity, var_len=var_len)
            for _ in range(W)]


def run_sharded(ix, reads, first, W, per_rank, starts, cs, ahead=False, ahead2=False,
                capacity=None, var_len=False, pipes=None):
    """reads: [2n, L] mates in global order; first: the sample table over the
    global pair indexes, or None for the plain sharded run (one count row).
    capacity: each rank's key-set capacity (default n: an owner may hold every
    key).  pipes: pipelines to reuse (made otherwise).  Returns (count rows
    summed over the ranks, the six counters per sample summed over the ranks,
    the run's six counters summed over the ranks)."""
    dev = torch.device("cuda")
    n = reads.shape[0] // 2
    B = per_rank
    steps = (n + W * B - 1) // (W * B)
    if pipes is None:
        pipes = make_pipes(ix, cs, starts, reads.shape[1], W, B, capacity or max(n, 1), var_len)
    for p in pipes:
        p.reset()
        p.set_samples_sharded(first)
    H, T = pipes[0].hdr_words, pipes[0].tail_words
    assert (H, T) == ((2, 3) if first is not None else (1, 2))
    S_rows = len(first) - 1 if first is not None else 1
    counts = [torch.zeros((S_rows, len(starts)), dtype=torch.int64, device=dev)
              for _ in range(W)]
    carried = torch.full((T - 1,), -1, dtype=torch.int64, device=dev)
    batches = {}   # (rank, step) -> (its reads on the device, pairs), kept alive for the run

    def batch(r, s):
        if (r, s) not in batches:
            lo = min(n, s * W * B + r * B)
            hi = min(n, lo + B)
            batches[(r, s)] = (_rows(reads, 2 * lo, 2 * hi, dev) if hi > lo else None, hi - lo)
        return batches[(r, s)]

    for s in range(steps):
        base = s * W * B
        sends = []
        for r in range(W):
            cur, m = batch(r, s)
            nxt, mn = batch(r, s + 1) if ahead and s + 1 < steps else (None, 0)
            if mn:
                pipes[r].phase_map_ahead(cur, m, nxt, mn)
            else:
                pipes[r].phase_map(cur, m)
            hdr, words, cnt, wcnt = pipes[r].phase_export(W, base + r * B)
            assert hdr.shape[1] == H
            if mn and ahead2 and s + 2 < steps and batch(r, s + 2)[1]:
                pipes[r].phase_search_ahead(*batch(r, s + 2))
            sends.append((hdr.clone(), words.clone(), [int(c) for c in cnt],
                          [int(c) for c in wcnt]))
        flags_back = [[None] * W for _ in range(W)]
        for o in range(W):   # all_to_all: owner o receives segment o of every rank, rank order
            hparts, wparts, rc, rw = [], [], [], []
            for r in range(W):
                hdr, words, cnt, wcnt = sends[r]
                h0, w0 = sum(cnt[:o]), sum(wcnt[:o])
                hparts.append(hdr[h0:h0 + cnt[o]])
                wparts.append(words[w0:w0 + wcnt[o]])
                rc.append(cnt[o])
                rw.append(wcnt[o])
            k = sum(rc)
            recv = torch.cat(hparts) if k else torch.zeros((1, H), dtype=torch.int64, device=dev)
            rwords = torch.cat(wparts) if sum(rw) else torch.zeros(1, dtype=torch.int64,
                                                                  device=dev)
            flags = torch.empty(max(k, 1), dtype=torch.uint8, device=dev)
            pipes[o].dedup_owner(recv.contiguous(), k, rwords, rc, rw, flags)
            at = 0
            for r in range(W):
                flags_back[r][o] = flags[at:at + rc[r]]
                at += rc[r]
        tails = []
        for r in range(W):
            back = torch.cat(flags_back[r]) if sum(sends[r][2]) else \
                torch.zeros(1, dtype=torch.uint8, device=dev)
            pipes[r].phase_import(back)
            tail = torch.empty(T, dtype=torch.int64, device=dev)
            pipes[r].phase_positions(tail)
            tails.append(tail)
        Ts = torch.stack(tails)
        for r in range(W):
            pipes[r].phase_bin(ShardedCounter._prev(Ts[:r], carried), counts[r])
        carried = ShardedCounter._prev(Ts, carried)
    st = [six(p.stats()) for p in pipes]   # (raises on a data error: a full key set)
    rows = sum(c.cpu().numpy().astype(np.int64) for c in counts).tolist()
    ss = []
    if first is not None:
        per = [[six(x) for x in p.sample_stats()] for p in pipes]
        ss = [tuple(sum(per[r][k][f] for r in range(W)) for f in range(6))
              for k in range(S_rows)]
    return rows, ss, tuple(sum(x[f] for x in st) for f in range(6))
