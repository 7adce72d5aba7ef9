"""The map hints of k_mam_sm's match words, proven on the CPU through the
single-lane emulation (tools/sm_emu, hints=True): bits 40..47, a forward
match's right map.bin byte from its packed SA word, and bits 33..39, the chain
hint m = dch - j + 1 that A_CHAIN_DONE takes from the (B) chain scan -- the
length of the shortest unique string ending at the match's last base, which is
the right map.bin byte of a reverse-strand alignment (its first forward base
mirrors the match's last base, and the doubled text is closed under reverse
complement).

Strict: every non-zero chain hint of a match in a reverse-complement contig,
after the post stage's zeroing rule (m + i >= the contig size, i.e. m >= the
match's offset in its contig + its length), equals the map.bin byte it
replaces (the oracle's mappability_range); every forward hint equals its own
byte in the same way; the matches are the oracle's and the emulator's without
hints.  A condition, not a measurement: at most 10 % of the reverse matches
lack a chain hint (a hint is 7 bits: none past 127).  These inputs stay within
it at every length used, 150 included (the fractions are printed)."""
import os
import sys

import numpy as np
import pytest

from conftest import interleaved_reads

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools", "sm_emu"))
import sm_emu  # noqa: E402
import rev_hint_inputs as R  # noqa: E402
import oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def tiny(tiny_ix):
    tiny_ix.accel()
    return tiny_ix, sm_emu.Emu(tiny_ix, packed=True), R.HintCheck(tiny_ix)


@pytest.fixture(scope="module")
def mid():
    g, (T, sp, sz, names) = R.mid_index()
    ix = O.Index(T, sp, sz, names)
    ix.accel()
    return g, ix, sm_emu.Emu(ix, packed=True), R.HintCheck(ix)


def run(ix, emu, chk, reads, lens=None, max_lack=0.10, name=""):
    """searches with hints on and off; checks every word; returns the words"""
    before = (chk.n_rev, chk.n_rev_hint, chk.n_rev_zeroed, chk.n_fwd, chk.n_fwd_hint)
    got, _ = emu.map(reads, min_len=R.MIN_LEN, lens=lens, hints=True)
    words = emu.words
    off, _ = emu.map(reads, min_len=R.MIN_LEN, lens=lens)
    assert got == off
    assert [len(w) for w in words] == [len(m) for m in got]
    for r in range(reads.shape[0]):
        read = reads[r, :lens[r]] if lens is not None else reads[r]
        assert got[r] == ix.search(read.tobytes(), min_len=R.MIN_LEN), (name, r)
        assert [chk.word(w) for w in words[r]] == got[r], (name, r)
    n_rev, n_hint, n_zero, n_fwd, n_fh = (a - b for a, b in zip(
        (chk.n_rev, chk.n_rev_hint, chk.n_rev_zeroed, chk.n_fwd, chk.n_fwd_hint), before))
    print("%s: %d reverse matches, %d with a chain hint (%d zeroed by the edge rule); "
          "%d forward, %d hinted" % (name, n_rev, n_hint, n_zero, n_fwd, n_fh))
    if max_lack is not None:
        assert n_rev > 0 and n_rev - n_hint <= max_lack * n_rev, (name, n_rev, n_hint)
    return words


@pytest.mark.parametrize("s", ["s150", "s100"])
def test_golden_reads_tiny(tiny, s):
    ix, emu, chk = tiny
    run(ix, emu, chk, interleaved_reads(s), name=s)


def test_edge_and_hand_made_reads_tiny(tiny):
    """array ends, bytes outside acgt, homopolymers; matches touching a
    reverse-complement contig's first and last base; reads with an N"""
    ix, emu, chk = tiny
    # (edge reads: homopolymers and bad bytes, few matches: no fraction asked)
    run(ix, emu, chk, R.edge_reads_150(ix), max_lack=None, name="tiny edge")
    for L in (150, 100):
        run(ix, emu, chk, R.hand_reads(ix, L), name="tiny hand-made %d" % L)


def test_synthetic_pairs_mid(mid):
    g, ix, emu, chk = mid
    run(ix, emu, chk, R.synth_reads(g, 300, 150, seed=91), name="mid 150")
    run(ix, emu, chk, R.synth_reads(g, 200, 100, seed=92), name="mid 100")


def test_edge_and_hand_made_reads_mid(mid):
    g, ix, emu, chk = mid
    run(ix, emu, chk, R.edge_reads_150(ix), max_lack=None, name="mid edge")
    for L in (150, 100):
        run(ix, emu, chk, R.hand_reads(ix, L), name="mid hand-made %d" % L)


def test_zeroing_rule_decides_on_edge_genome():
    """a reverse-strand match at its contig's first base whose hint is as long
    as the match: the only case in which the rule m >= offset + length bites"""
    ix = O.Index(*O.text_from_contigs(R.edge_genome()))
    ix.accel()
    emu, chk = sm_emu.Emu(ix, packed=True), R.HintCheck(ix)
    for L in (150, 100):
        run(ix, emu, chk, R.edge_genome_reads(ix, L), name="edge genome %d" % L)
    assert chk.n_rev_zeroed >= 6          # the three hand-placed reads of each length


def test_mixed_lengths_through_records(tiny):
    """the generic kernel's path of the variable-length pipeline: per-read
    lengths, records in the geometry of the longest read"""
    ix, emu, chk = tiny
    reads = interleaved_reads("s150")[:400].copy()
    rng = np.random.default_rng(7)
    lens = rng.integers(15, 151, size=reads.shape[0]).astype(np.uint16)
    lens[:4] = (150, 20, 19, 128)
    for r in range(reads.shape[0]):
        reads[r, lens[r]:] = 0
    run(ix, emu, chk, reads, lens=lens, name="mixed lengths")


def test_hints_off_words_are_plain(tiny):
    ix, emu, _ = tiny
    reads = interleaved_reads("s100")[:200]
    emu.map(reads, min_len=R.MIN_LEN)
    for w in emu.words:
        assert not np.any((w >> np.uint64(R.POS_BITS)) & np.uint64(0x7FFF))
