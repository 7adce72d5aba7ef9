"""The bin design's host side (no device): smash_bins_apportion against the
rule in numpy (tests/bins_spec.py), and the bins.txt / gc.txt writers of
`smash_cli.py bins` from a hand-made table."""
import numpy as np
import pytest

import bins_spec
import smash_cli
import smashgpu as S


def lib_apportion(M, off, nbins):
    try:
        return [int(x) for x in S.bins_apportion(M, off, nbins)]
    except S.SmashError as e:
        assert e.code == -1, e          # SMASH_ERR_ARG
        return "ERR_ARG"


def spec_apportion(M, off, nbins):
    try:
        return bins_spec.apportion(M, [o >= 0 for o in off], nbins)
    except ValueError:
        return "ERR_ARG"


def offsets(binned):
    return [100 * c if b else -1 for c, b in enumerate(binned)]


@pytest.mark.parametrize("M,binned,nbins,want", [
    # remainder ties: the earlier contig wins
    ([5, 5, 5], [1, 1, 1], 4, [2, 1, 1]),
    ([5, 5, 5], [1, 1, 1], 5, [2, 2, 1]),
    ([1, 1, 1, 1], [1, 1, 1, 1], 6, [2, 2, 1, 1]),
    ([3, 1, 3, 1], [1, 1, 1, 1], 6, [2, 1, 2, 1]),
    # a binned contig without a unique base gets exactly its one bin
    ([0, 10, 7], [1, 1, 1], 10, None),
    ([0, 0, 9], [1, 1, 1], 40, [1, 1, 38]),
    # unbinned contigs get none, whatever they hold
    ([8, 1000, 8, 1000], [1, 0, 1, 0], 10, [5, 0, 5, 0]),
    ([8, 1000, 3, 7], [0, 0, 1, 1], 12, None),
    # as many bins as binned contigs; one less is an error
    ([4, 0, 9, 2], [1, 1, 0, 1], 3, [1, 1, 0, 1]),
    ([4, 0, 9, 2], [1, 1, 0, 1], 2, "ERR_ARG"),
    ([4, 0, 9, 2], [1, 1, 0, 1], 0, "ERR_ARG"),
    # bins left to share and nothing to share them by
    ([0, 0], [1, 1], 3, "ERR_ARG"),
    ([0, 0], [1, 1], 2, [1, 1]),
    # products past 32 bits
    ([2**32 - 1, 2**32 - 5, 2**31 + 7, 3 * 2**30], [1, 1, 1, 1], 500000, None),
    ([2**32 + 11, 2**32 - 1, 1, 2**33 - 9, 2**32 - 1], [1, 1, 1, 1, 1], 500000, None),
])
def test_apportion_equals_the_rule(M, binned, nbins, want):
    off = offsets(binned)
    spec = spec_apportion(M, off, nbins)
    if want is not None:
        assert spec == want             # the case is the one its comment names
    got = lib_apportion(M, off, nbins)
    assert got == spec
    if got != "ERR_ARG":
        assert sum(got) == nbins


def test_apportion_random_cases_equal_the_rule():
    rng = np.random.default_rng(11)
    for _ in range(300):
        n = int(rng.integers(1, 9))
        M = [int(x) for x in rng.integers(0, int(rng.choice([3, 50, 10**6, 2**33])), n)]
        binned = [int(x) for x in rng.integers(0, 2, n)]
        nbins = int(rng.integers(0, int(rng.choice([12, 500, 10**6]))))
        off = offsets(binned)
        assert lib_apportion(M, off, nbins) == spec_apportion(M, off, nbins), (M, binned, nbins)


CONTIGS = ["chr1", "chr2", "chrM", "chrX"]
SIZES = {"chr1": 1000, "chr2": 70, "chrX": 300}


def table():
    rows = np.zeros(6, S.BIN)
    #          contig start stop abspos n_unique n_gc n_acgt
    data = [(0, 0, 400, 0, 100, 150, 380),
            (0, 400, 401, 400, 100, 1, 1),
            (0, 401, 1000, 401, 101, 0, 0),         # no a, c, g or t at all
            (1, 0, 70, 1000, 7, 23, 69),
            (3, 0, 123, 1070, 50, 41, 123),
            (3, 123, 300, 1193, 50, 59, 176)]
    for r, d in zip(rows, data):
        (r["contig"], r["start"], r["stop"], r["abspos"], r["n_unique"], r["n_gc"],
         r["n_acgt"]) = d
    return rows


def test_bins_txt_parses_back_and_tiles_each_contig(tmp_path):
    rows = table()
    p = str(tmp_path / "bins.txt")
    smash_cli.write_bins_txt(rows, CONTIGS, p)
    parsed, starts = S.read_bins(p)
    assert starts.tolist() == rows["abspos"].tolist()
    assert all(len(r) == 6 for r in parsed)
    assert [r[0] for r in parsed] == ["chr1", "chr1", "chr1", "chr2", "chrX", "chrX"]
    for r, want in zip(parsed, rows):
        assert [int(x) for x in r[1:]] == [want["start"], want["abspos"], want["stop"],
                                           want["stop"] - want["start"], want["n_unique"]]
    for a, b in zip(parsed[:-1], parsed[1:]):
        if a[0] == b[0]:
            assert int(a[3]) == int(b[1])           # a bin stops where the next starts
        else:
            assert int(a[3]) == SIZES[a[0]] and int(b[1]) == 0
    assert int(parsed[-1][3]) == SIZES[parsed[-1][0]]


def test_gc_txt_has_the_reference_header_and_ten_columns(tmp_path):
    rows = table()
    p = str(tmp_path / "gc.txt")
    smash_cli.write_gc_txt(rows, CONTIGS, p)
    lines = open(p).read().split("\n")
    assert lines[-1] == "" and len(lines) == len(rows) + 2
    assert lines[0].split("\t") == ["bin.chrom", "bin.start", "bin.end", "bin.length",
                                    "gene.count", "cgi.count", "dist.telomere", "gc.content",
                                    "cviki_count", "nlaiii_count"]
    body = [l.split("\t") for l in lines[1:-1]]
    assert all(len(c) == 10 for c in body)
    assert body[0] == ["chr1", "0", "399", "400", "0", "0", "0", "0.394737", "0", "0"]
    assert body[1] == ["chr1", "400", "400", "1", "0", "0", "0", "1.000000", "0", "0"]
    assert body[2][7] == "0.000000"                 # n_acgt = 0
    assert body[3][:4] == ["chr2", "0", "69", "70"] and body[3][7] == "%.6f" % (23 / 69)
    assert body[5][:4] == ["chrX", "123", "299", "177"]
