"""tests/mock_pipeline.py's oracle-backed stand-in with a sharded sample table
(smashgpu.Pipeline.set_samples_sharded), on CPU tensors.  TEST
INFRASTRUCTURE: lets tests/test_samples_sharded_cpu.py drive
dist.ShardedCounter(samples=...) and dist.count_fastq_many over
torch.distributed/gloo.  It follows smash_gpu.h's contract of the sample forms:
two-word headers {nk << 40 | word offset, sample}, first-wins over (sample,
key), three-word tails, {pos0, sample} carried into the bin phase, one count
row and one row of counters per sample."""
import bisect
from types import SimpleNamespace

import numpy as np
import torch

import oracle as O
from mock_pipeline import OraclePhasePipeline, key_hash, to_i64, to_u64

FIELDS = ("pairs", "key_pairs", "dupe_pairs", "positions", "dups", "kept")


class SampleOraclePipeline(OraclePhasePipeline):
    hdr_words = 2
    tail_words = 3

    def set_samples_sharded(self, first):
        self.first = [int(x) for x in first]
        self.reset()

    def reset(self, keep_search=False):
        super().reset(keep_search)
        S = len(getattr(self, "first", [0])) - 1
        self.sstats = np.zeros((S, 6), np.int64)

    def sample_of(self, g):
        return bisect.bisect_right(self.first, g, 0, len(self.first) - 1) - 1

    def sample_stats(self):
        return [SimpleNamespace(**dict(zip(FIELDS, (int(v) for v in row))))
                for row in self.sstats]

    def phase_export(self, world, gbase):
        assert self.n == 0 or gbase + self.n <= self.first[-1]
        self.smp = [self.sample_of(gbase + q) for q in range(self.n)]
        firstq = {}
        for q, k in enumerate(self.kept_hits):
            self.sstats[self.smp[q], 0] += 1
            if k is not None and (self.smp[q], tuple(k)) not in firstq:
                firstq[(self.smp[q], tuple(k))] = q
        groups = [[] for _ in range(world)]
        for (s, k), q in firstq.items():
            groups[(key_hash((s,) + k)[0] >> 1) % world].append((s, k, q))   # the salted owner
        self.order = []
        rows, words, counts, wcounts = [], [], [], []
        for w in range(world):
            seg = []
            for s, k, q in sorted(groups[w], key=lambda t: t[2]):
                rows.append(((len(k) << 40) | len(seg), s))
                seg += [to_i64((tid << 48) | pos) for tid, pos in k]
                self.order.append(q)
            words += seg
            counts.append(len(groups[w]))
            wcounts.append(len(seg))
        hdr = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)
        return (hdr, torch.tensor(words, dtype=torch.int64), np.array(counts, np.int64),
                np.array(wcounts, np.int64))

    def dedup_owner(self, d_recv, n_recv, d_recv_words, recv_counts, recv_words, d_flags):
        rows = d_recv[:n_recv].tolist()
        words = d_recv_words.tolist()
        hb = np.cumsum([0] + list(recv_counts))
        wb = np.cumsum([0] + list(recv_words))
        best = {}
        for j, (nw, s) in enumerate(rows):
            nk, off = nw >> 40, nw & ((1 << 40) - 1)
            src = int(np.searchsorted(hb, j, side="right")) - 1
            a = int(wb[src]) + off
            k = (s,) + tuple((to_u64(w) >> 48, to_u64(w) & 0xFFFFFFFFFFFF)
                             for w in words[a:a + nk])
            if k not in best:   # the first in receive order = global pair order
                best[k] = j
        flags = np.zeros(n_recv, np.uint8)
        for k, j in best.items():
            if k not in self.seen:
                flags[j] = 1
        self.seen.update(best.keys())
        if len(self.seen) > self.key_capacity:
            self.error = -4
        if n_recv:
            d_flags[:n_recv] = torch.from_numpy(flags)

    def phase_import(self, d_back):
        super().phase_import(d_back)
        for q, k in enumerate(self.kept_hits):
            if k is not None:
                self.sstats[self.smp[q], 1] += 1
                self.sstats[self.smp[q], 2] += 0 if self.keep[q] else 1

    def phase_positions(self, d_tail):
        self.pos = []   # (pos0, abspos, sample)
        for q in range(self.n):
            if self.keep[q]:
                for tid, p in self.kept_hits[q]:
                    if self.major[tid]:
                        self.pos.append((p, p + self.coff[tid], self.smp[q]))
        d_tail[0] = len(self.pos)
        d_tail[1] = self.pos[-1][0] if self.pos else -1
        d_tail[2] = self.pos[-1][2] if self.pos else -1

    def phase_bin(self, d_prev, d_counts):
        prev0, prev_s = (int(x) for x in d_prev.reshape(-1)[:2].tolist())
        i = 0
        while i < len(self.pos):
            s = self.pos[i][2]
            j = i
            while j < len(self.pos) and self.pos[j][2] == s:
                j += 1
            # the carried line opens only its own sample's chain
            st = O.OrcVarbinState(0, 0, 0, prev0 if i == 0 and prev_s == s else -1)
            c, st = O.varbin([p for p, _, _ in self.pos[i:j]], [a for _, a, _ in self.pos[i:j]],
                             self.bins, state=st)
            d_counts[s] += torch.from_numpy(c.astype(np.int64))
            self.sstats[s, 3:6] += (st.total, st.dups, st.kept)
            self.total += st.total
            self.dups += st.dups
            self.kept += st.kept
            i = j
