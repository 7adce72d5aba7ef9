"""geometry_inputs' cases are not vacuous: what test_gpu_geometry.py relies
on to have given the device real work, asserted here from the oracle alone
(CPU).  The measured figures stand next to each threshold."""
import numpy as np
import pytest

from conftest import gold, load_bins, load_chrom_sizes

import oracle as O
import synth
import geometry_inputs as G


@pytest.fixture(scope="module")
def tiny(tiny_ix):
    tiny_ix.accel()
    return tiny_ix


@pytest.fixture(scope="module")
def mid():
    oix = O.Index(*O.text_from_contigs(synth.make_genome("mid")))
    oix.accel()
    return oix


def test_b_of_the_two_indexes(tiny, mid):
    """the min_len grid is relative to these"""
    assert tiny.acc.B == 11 and mid.acc.B == 13
    assert G.min_lens(11, 36) == [2, 10, 11, 13, 20, 21, 22, 24, 25]
    assert G.min_lens(11, 20) == [10, 11, 13, 20]
    assert G.min_lens(13, 255) == [12, 13, 15, 20, 23, 24, 26, 27]
    assert G.pipe_min_lens(11, 20) == [13, 20] and G.pipe_min_lens(11, 24) == [13, 20]
    assert G.pipe_min_lens(11, 36) == [13, 20, 25]
    assert set(G.PIPE_LENGTHS) <= set(G.LENGTHS)


@pytest.mark.parametrize("L", G.LENGTHS)
def test_edge_reads_match_and_do_not(tiny, L):
    """every (L, min_len) of the search grid: reads with matches, reads with
    none, reads with a byte the text lacks.  Measured over the grid's 164
    (L, min_len): 20..113 of the 130 reads match (the fewest: L 24 at min_len
    24), 17..110 do not, and 28..44 hold a byte absent from the text."""
    reads = G.edge_reads(tiny, L, 130, seed=L)
    assert reads.shape == (130, L) and 130 % 64
    in_text = np.zeros(256, bool)
    in_text[np.unique(tiny.T[:tiny.N])] = True
    foreign = int((~in_text[reads]).any(axis=1).sum())
    assert foreign >= 1
    for ml in G.min_lens(tiny.acc.B, L):
        n = [len(tiny.search(reads[r].tobytes(), min_len=ml)) for r in range(130)]
        hit = sum(1 for x in n if x)
        print("L %d min_len %d: %d reads match, %d do not, %d foreign" % (L, ml, hit, 130 - hit, foreign))
        assert hit >= 1 and hit < 130, (L, ml)
        assert max(n) <= L - ml + 1      # the cap the device runs with


@pytest.mark.parametrize("L", G.PIPE_LENGTHS)
def test_pipeline_cases_count_something(tiny, L):
    """1 500 pairs seeded by L at min_len B + 2, 20 and B + 14: no tag error,
    positions kept, duplicate pairs and at least 20 bins counted.  Measured
    over L 20..255 and the three min_len: 1 270..11 470 positions, all kept,
    6..18 duplicate pairs, 21 or 22 of the 24 bins nonzero."""
    starts = load_bins(gold("tiny_bins.txt"))[1]
    cs = load_chrom_sizes(gold("tiny_chrom_sizes.txt"))
    reads = G.smash_reads(synth.make_genome("tiny"), 1500, L, seed=L)
    mapbin = tiny.mappability()
    for ml in G.pipe_min_lens(tiny.acc.B, L):
        op = O.Pipeline(tiny, mapbin, cs, starts, min_len=ml)
        assert op.run(reads, threads=4) == 0
        print("L %d min_len %d: positions %d kept %d dupe pairs %d bins %d"
              % (L, ml, op.state.total, op.state.kept, op.n_dupe.value, int((op.counts > 0).sum())))
        assert op.state.kept > 0 and op.n_dupe.value > 0
        assert int((op.counts > 0).sum()) >= 20


def test_long_case_passes_the_post_capacities(tiny):
    """LONG_CASE: mates with more than 8 matches (k_post_fast<8> hands them to
    <16>), more than 16 (k_post), and keys of more than 16 words.  Measured:
    764 mates above 8, 38 above 16, 6 keys above 16 words (the longest 18)."""
    c = G.LONG_CASE
    reads = G.case_reads(synth.make_genome("tiny"), c)
    assert reads.shape == (2 * c["n_pairs"], c["L"])
    ch = G.Chain(tiny, reads, min_len=c["min_len"])
    assert ch.tag_errors == 0
    n = np.array([len(m) for m in ch.matches])
    nk = np.array([len(k) if k is not None else -1 for k in ch.keys])
    print("LONG_CASE: mates > 8: %d, > 16: %d; keys > 16 words: %d, max %d"
          % ((n > 8).sum(), (n > 16).sum(), (nk > 16).sum(), nk.max()))
    assert ((n > 8).sum(), (n > 16).sum(), (nk > 16).sum(), nk.max()) == (764, 38, 6, 18)


def test_hint_case_reaches_the_caps(mid):
    """HINT_CASE: matches longer than 127 bases on both strands (a chain hint
    holds m - 1 < 127, a map hint at most 127).  Measured: 482 such matches on
    the forward strand, 491 on the reverse."""
    c = G.HINT_CASE
    reads = G.case_reads(synth.make_genome("mid"), c)
    sp = np.asarray(mid.startpos, np.int64)
    long_ = [0, 0]
    for r in range(reads.shape[0]):
        for ref, _q, ln in mid.search(reads[r].tobytes()):
            if ln > 127:
                long_[(int(np.searchsorted(sp, ref, side="right")) - 1) & 1] += 1
    print("HINT_CASE: matches longer than 127: %d forward, %d reverse" % tuple(long_))
    assert long_[0] > 0 and long_[1] > 0
    # the pipeline run on it is no data error, and has keys and duplicates
    # (measured: every one of the 1 500 pairs has a key, 12 repeat an earlier one)
    ch = G.Chain(mid, reads)
    assert ch.tag_errors == 0
    keys = sum(k is not None for k in ch.keys)
    assert keys == 1500 and keys - sum(ch.keep) == 12


@pytest.mark.parametrize("width,pairs,key_pairs,dupes", [(40, 42, 23, 1), (76, 154, 117, 2),
                                                         (255, 650, 609, 6)])
def test_var_len_widths_hold_pairs(tiny, width, pairs, key_pairs, dupes):
    """the mates of every row width: pairs, pairs with a key and duplicate
    pairs as measured (at 255: the 600 v150 pairs plus 50 pairs of 255
    bases), mates shorter than min_len and mates as long as the width among
    them, and no tag error"""
    import varlen_util as V
    mates = G.var_len_mates(width)
    assert len(mates) == 2 * pairs
    lens = [len(m) for m in mates]
    assert min(lens) < 20 and max(lens) == width
    ch = V.Chain(tiny, mates)
    print("width %d: %d pairs, %d with a key, %d duplicates" % (width, pairs, ch.key_pairs, ch.dupe_pairs))
    assert ch.tag_errors == 0
    assert (ch.key_pairs, ch.dupe_pairs) == (key_pairs, dupes)
