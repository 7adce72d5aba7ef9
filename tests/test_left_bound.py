"""The left map.bin byte's bound (csrc/pipeline.hip mate_fast), proven on the
CPU: the rule of left_bound_inputs.py over the match words of the single-lane
emulation (tools/sm_emu, hints=True), on the genomes and reads of
rev_hint_inputs.py -- golden, edge, synthetic and hand-made reads at 150 and
100 bases -- and on left_bound_inputs' hand_reads and bound_genome, made for
the conditions those inputs do not reach.

Strict: for every alignment the rule skips, the oracle's map.bin left byte at
e, the forward base after the block's end, is in [1, b + 1], b the hint the
rule reads (LeftBound.word asserts it).  Against a vacuous test: every input
set has the rule skip at least one alignment, both strands are skipped, and
every branch of the rule's conditions is reached."""
import os
import sys

import numpy as np
import pytest

from conftest import interleaved_reads

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools", "sm_emu"))
import sm_emu  # noqa: E402
import left_bound_inputs as B  # noqa: E402
import rev_hint_inputs as R  # noqa: E402
import oracle as O  # noqa: E402

MIN_EXCESS = 4   # smash_mapping.sh:25


class Subject:
    def __init__(self, ix):
        ix.accel()
        self.ix, self.emu, self.lb = ix, sm_emu.Emu(ix, packed=True), B.LeftBound(ix)

    def run(self, reads, name, min_excess=MIN_EXCESS):
        """every match word of the reads through the rule; the skips"""
        before = list(self.lb.skipped)
        self.emu.map(reads, min_len=R.MIN_LEN, hints=True)
        n = 0
        for r in range(reads.shape[0]):
            for w in self.emu.words[r]:
                n += self.lb.word(w, reads.shape[1], min_excess) is not None
        skipped = [a - b for a, b in zip(self.lb.skipped, before)]
        print("%s: %d alignments, the rule skips %d forward and %d reverse"
              % (name, n, skipped[0], skipped[1]))
        assert sum(skipped) > 0, name
        return skipped


@pytest.fixture(scope="module")
def tiny(tiny_ix):
    return Subject(tiny_ix)


@pytest.fixture(scope="module")
def mid():
    g, (T, sp, sz, names) = R.mid_index()
    s = Subject(O.Index(T, sp, sz, names))
    s.g = g
    return s


@pytest.fixture(scope="module")
def edge():
    return Subject(O.Index(*O.text_from_contigs(R.edge_genome())))


@pytest.fixture(scope="module")
def bound():
    return Subject(O.Index(*O.text_from_contigs(B.bound_genome())))


@pytest.mark.parametrize("s", ["s150", "s100"])
def test_golden_reads_tiny(tiny, s):
    f, r = tiny.run(interleaved_reads(s), s)
    assert f > 0 and r > 0


def test_edge_and_hand_made_reads_tiny(tiny):
    # (the edge reads are homopolymers and bad bytes: their few matches are
    # one set with the hand-made reads of their length)
    for L in (150, 100):
        reads = R.hand_reads(tiny.ix, L)
        if L == 150:
            reads = np.concatenate([R.edge_reads_150(tiny.ix), reads])
        tiny.run(reads, "tiny edge + hand-made %d" % L)
        tiny.run(B.hand_reads(tiny.ix, L), "tiny bound reads %d" % L)


def test_synthetic_pairs_mid(mid):
    for n, L, seed in ((300, 150, 91), (200, 100, 92)):
        f, r = mid.run(R.synth_reads(mid.g, n, L, seed=seed), "mid %d" % L)
        assert f > 0 and r > 0


def test_edge_and_hand_made_reads_mid(mid):
    for L in (150, 100):
        reads = R.hand_reads(mid.ix, L)
        if L == 150:
            reads = np.concatenate([R.edge_reads_150(mid.ix), reads])
        mid.run(reads, "mid edge + hand-made %d" % L)
        mid.run(B.hand_reads(mid.ix, L), "mid bound reads %d" % L)


def test_edge_genome(edge):
    for L in (150, 100):
        edge.run(np.concatenate([R.edge_genome_reads(edge.ix, L), B.hand_reads(edge.ix, L)]),
                 "edge genome %d" % L)


def test_bound_genome(bound):
    """a match whose hint is as long as the match at its contig's first
    bases (b + 1 >= ie), and matches of 150 bases without a hint"""
    for L in (150, 100):
        bound.run(B.bound_genome_reads(bound.ix, L), "bound genome %d" % L)
    for strand in ("forward", "reverse"):                   # one kept read per length
        assert bound.lb.branch.get("b + 1 >= ie, " + strand, 0) >= 2
    assert bound.lb.branch.get("no hint", 0) >= 2


def test_signed_min_excess(tiny):
    """min_excess <= 0: b <= len alone limits the rule, and the bound holds"""
    s = Subject(tiny.ix)
    s.run(B.hand_reads(tiny.ix, 100, min_excess=-3), "min_excess -3", min_excess=-3)
    assert s.lb.cause[B.SKIP] > 0 and s.lb.branch.get("len - min_excess < b <= len", 0) == 0


def test_every_branch_reached(tiny, mid, edge, bound):
    """over the inputs above and the hand-made reads for the bound (run here
    too, so that the test stands alone)"""
    for s in (tiny, mid, edge):
        for L in (150, 100):
            s.run(B.hand_reads(s.ix, L), "bound reads %d" % L)
    bound.run(B.bound_genome_reads(bound.ix, 150), "bound genome 150")
    tiny.run(interleaved_reads("s100")[:400], "s100")      # (repeats: matches without a hint)
    hit = {}
    for s in (tiny, mid, edge, bound):
        for k, v in s.lb.branch.items():
            hit[k] = hit.get(k, 0) + v
    print(hit)
    for name in ("no hint", "forward ends on the last base", "reverse o = 0",
                 "b + 1 >= ie, forward", "b + 1 >= ie, reverse",
                 "len - min_excess < b <= len", "skip forward", "skip reverse"):
        assert hit.get(name, 0) > 0, (name, hit)
    cause = {c: sum(s.lb.cause[c] for s in (tiny, mid, edge, bound)) for c in B.CAUSES}
    assert cause[B.SKIP] > 0 and cause[B.NO_HINT] > 0 and cause[B.EDGE] > 0
    assert cause[B.WIDE_PASS] + cause[B.WIDE_FAIL] > 0
