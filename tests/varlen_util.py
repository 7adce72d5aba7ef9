"""Helpers of the mixed-read-length tests (test_varlen_cpu.py,
test_gpu_varlen.py): the v150 fixture (tools/make_golden_varlen.sh: the s150
pairs trimmed by tools/varlen_reads.py, run through the reference chain) and
the oracle's per-read primitives chained per pair."""
import functools

import numpy as np

from conftest import fastq_reads, gold, load_bins, load_chrom_sizes, read_gz_lines

import oracle as O
from varlen_reads import vlen


def mixed_mates(prefix, cap=None, n_pairs=None, trim=False):
    """The mates of a golden FASTQ pair, interleaved r1, r2, r1, ..., as
    lowercased byte strings (N -> z); trim: cut by the trim rule first."""
    r1 = fastq_reads(prefix + "_r1.fq.gz")[:n_pairs]
    r2 = fastq_reads(prefix + "_r2.fq.gz")[:n_pairs]
    out = []
    for a, b in zip(r1, r2):
        for s in (a, b):
            out.append(O.lower_read(s[:vlen(s, cap)] if trim else s))
    return out


def rows_of(mates, width, stride=None):
    """[len(mates), stride] uint8 rows, each mate at its row's start, zero padded."""
    rows = np.zeros((len(mates), stride or width), np.uint8)
    for i, m in enumerate(mates):
        assert len(m) <= width
        rows[i, :len(m)] = np.frombuffer(m, np.uint8)
    return rows


def trim_rule_lengths(prefix, cap=None, n_pairs=None):
    r1 = fastq_reads(prefix + "_r1.fq.gz")[:n_pairs]
    r2 = fastq_reads(prefix + "_r2.fq.gz")[:n_pairs]
    return [vlen(s, cap) for ab in zip(r1, r2) for s in ab]


class Chain:
    """search -> resolve -> tag -> smash_pair per pair, a dict as smashMEM's
    first-wins set, the major chromosomes' positions, O.varbin."""

    def __init__(self, ix, mates, min_len=20):
        self.starts = load_bins(gold("tiny_bins.txt"))[1]
        cs = load_chrom_sizes(gold("tiny_chrom_sizes.txt"))
        mapbin = ix.mappability()
        offs = np.cumsum([0] + [int(x) for x in ix.sizes[0::2]][:-1]).astype(np.uint32)
        small = [1 if ("_gl000" in c or "chrM" in c) else 0 for c in ix.contigs]
        major = O.major_flags(ix.contigs, cs)
        self.keys, self.keep, self.lines = [], [], []
        self.tag_errors = 0
        seen = {}
        pos0, absp = [], []
        for q in range(len(mates) // 2):
            hs = []
            for m in (0, 1):
                P = mates[2 * q + m]
                h, _ = ix.resolve(P, ix.search(P, min_len=min_len))
                for x in h:
                    self.tag_errors += 1 if O.tag(x, offs, mapbin, small[x.tid]) else 0
                hs.append(h)
            key = O.smash_pair(hs[0], hs[1])
            self.keys.append(key)
            first = key is not None and tuple(key) not in seen
            self.keep.append(first)
            if key is None:
                continue
            if not first:
                continue
            seen[tuple(key)] = q
            for tid, pos in key:
                if major[tid]:
                    name = ix.contigs[tid]
                    self.lines.append("%s %d" % (name, pos))
                    pos0.append(pos)
                    absp.append(pos + cs[name])
        self.key_pairs = sum(k is not None for k in self.keys)
        self.dupe_pairs = self.key_pairs - len(seen)
        self.kept_hits = sum(len(k) for k, f in zip(self.keys, self.keep) if f)
        self.counts, self.state = O.varbin(pos0, absp, self.starts)

    @property
    def summary(self):
        return "%d dupes\t%d non-dupes" % (self.dupe_pairs, self.key_pairs - self.dupe_pairs)

    @property
    def totals(self):
        return (self.state.total, self.state.dups, self.state.kept)


@functools.lru_cache(maxsize=None)
def _golden(prefix):
    counts = [int(l.split("\t")[3]) for l in open(gold(prefix + "_varbin.txt"))]
    g = open(gold(prefix + "_varbin_stats_partial.txt")).read().split("\n")[1].split("\t")
    return {"counts": counts, "totals": (int(g[0]), int(g[1]), int(g[2])),
            "summary": read_gz_lines(prefix + "_smashmem.txt.gz")[-1],
            "positions": open(gold(prefix + "_positions.txt")).read().splitlines()}


def golden(prefix):
    """counts, (TotalReads, DupsRemoved, ReadsKept), the smashMEM summary line
    and the positions lines of the reference chain on `prefix`."""
    return _golden(prefix)
