"""Mixed read lengths on the host (no GPU): the three FASTQ readers under
SMASH_LEN_VAR, the v150 fixture (tests/golden/v150_*: the reference chain on
the s150 pairs trimmed by tools/varlen_reads.py) pinned to the oracle's
per-read primitives, the emulated device search with per-read lengths,
prepare_reads with mixed lengths and the CLI's error text."""
import gzip
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, gold, interleaved_reads, read_gz_lines

sys.path.insert(0, os.path.join(ROOT, "tools", "sm_emu"))
import sm_emu  # noqa: E402

import oracle as O
import smashgpu as S
import smash_cli
import varlen_util as V
from varlen_reads import SPECIAL

VAR = S.SMASH_LEN_VAR


@pytest.fixture(scope="module")
def v150_files(tmp_path_factory):
    """(gzip pair, plain pair) of the v150 FASTQ files"""
    d = tmp_path_factory.mktemp("v150")
    plain = []
    for m in ("r1", "r2"):
        p = d / ("v150_%s.fq" % m)
        p.write_bytes(gzip.open(gold("v150_%s.fq.gz" % m)).read())
        plain.append([str(p)])
    return ([gold("v150_r1.fq.gz")], [gold("v150_r2.fq.gz")]), tuple(plain)


@pytest.fixture(scope="module")
def v150_rows():
    mates = V.mixed_mates("v150")
    return mates, V.rows_of(mates, 150)


def test_fixture_lengths_follow_the_trim_rule(v150_rows):
    """v150 is s150 cut by the rule; every SPECIAL length, every length from
    1 to 150, mates under the minimum match length and whole mates occur"""
    mates, _ = v150_rows
    assert mates == V.mixed_mates("s150", trim=True)
    lens = [len(m) for m in mates]
    assert lens == V.trim_rule_lengths("s150")
    assert set(SPECIAL) <= set(lens) and set(lens) == set(range(1, 151))
    assert sum(l < 20 for l in lens) == 132 and sum(l == 150 for l in lens) == 28


@pytest.mark.parametrize("form", ["gzip", "plain"])
def test_three_readers_give_the_same_zero_padded_rows(v150_files, v150_rows, form):
    r1, r2 = v150_files[0 if form == "gzip" else 1]
    _, rows = v150_rows
    names, a = S.read_fastq_pairs(r1, r2, batch_pairs=250, read_len=VAR | 150)
    assert a.shape == (1200, 150) and np.array_equal(a, rows)       # *len returned the width
    assert names[0] == b"r000000000" and len(names) == 600
    n2, b = S.read_fastq_pairs_parallel(r1, r2, threads=3, read_len=VAR | 150)
    assert np.array_equal(b, rows) and n2.tolist() == names.tolist()
    fi = S.FastqIndex(r1, r2, threads=2, read_len=VAR | 150)
    assert (fi.n, fi.L) == (600, 150)
    out = np.full((2 * 593, 150), 7, np.uint8)                       # (a dirty buffer: pads are written)
    fi.pack(7, 600, out)
    assert np.array_equal(out, rows[14:])
    # a wider row: the same mates, more zeros
    _, w = S.read_fastq_pairs(r1, r2, read_len=VAR | 255)
    assert w.shape == (1200, 255) and np.array_equal(w[:, :150], rows) and not w[:, 150:].any()


def test_width_zero_is_the_longest_mate(v150_files, v150_rows):
    (r1, r2), _ = v150_files
    _, rows = v150_rows
    _, b = S.read_fastq_pairs_parallel(r1, r2, read_len=VAR)
    assert b.shape == (1200, 150) and np.array_equal(b, rows)
    fi = S.FastqIndex(r1, r2, read_len=VAR, sort_names=True)
    assert (fi.n, fi.L) == (600, 150)
    with pytest.raises(S.SmashError, match="maximum read length"):
        S.read_fastq_pairs(r1, r2, read_len=VAR)                     # a stream cannot know it


def test_longer_mate_and_old_errors(v150_files):
    (r1, r2), _ = v150_files
    for f in (S.read_fastq_pairs, S.read_fastq_pairs_parallel):
        with pytest.raises(S.SmashError, match=r"\(-1\).*longer than the maximum read length, 100 "
                                               r"\(r000000003\)"):
            f(r1, r2, read_len=VAR | 100)
        with pytest.raises(S.SmashError, match="same length"):       # without the flag: as before
            f(r1, r2)
    with pytest.raises(S.SmashError, match="longer than the maximum read length"):
        S.FastqIndex(r1, r2, read_len=VAR | 149)
    with pytest.raises(S.SmashError, match="same length"):
        S.FastqIndex(r1, r2)
    with pytest.raises(S.SmashError, match="read length, 150"):
        S.FastqIndex(r1, r2, read_len=150)


def test_empty_mate_rules_stay(tmp_path):
    a, b = tmp_path / "a.fq", tmp_path / "b.fq"
    a.write_bytes(b"@p0\nAC\n+\nII\n@p1\n\n+\n\n@p2\nACGTN\n+\nIIIII\n")
    b.write_bytes(b"@p0\nTTT\n+\nIII\n@p1\n\n+\n\n@p2\nC\n+\nJ\n")
    for f in (S.read_fastq_pairs, S.read_fastq_pairs_parallel):
        names, rows = f([str(a)], [str(b)], read_len=VAR | 6)
        assert names.tolist() == [b"p0", b"p2"]                      # both mates empty: dropped
        assert rows.tobytes() == b"ac\0\0\0\0" + b"ttt\0\0\0" + b"acgtz\0" + b"c\0\0\0\0\0"
    b.write_bytes(b"@p0\nTTT\n+\nIII\n@p1\nG\n+\nI\n@p2\nC\n+\nJ\n")
    for f in (S.read_fastq_pairs, S.read_fastq_pairs_parallel):
        with pytest.raises(S.SmashError, match="one mate of a pair has no bases"):
            f([str(a)], [str(b)], read_len=VAR | 6)


def test_oracle_chain_reproduces_the_reference(tiny_ix, v150_rows):
    """search -> resolve -> tag -> smash_pair per pair, a dict as the
    first-wins set, O.varbin == the reference's positions, bin counts,
    varbin totals and smashMEM summary: the fixture is pinned to the oracle."""
    mates, _ = v150_rows
    c = V.Chain(tiny_ix, mates)
    g = V.golden("v150")
    assert c.tag_errors == 0
    assert c.lines == g["positions"]
    assert c.counts.tolist() == g["counts"]
    assert c.totals == g["totals"]
    assert c.summary == g["summary"] == "5 dupes\t554 non-dupes"
    assert (c.key_pairs, c.dupe_pairs, c.kept_hits) == (559, 5, 1407)
    # the reference's own kept-hit lines: strands both well represented
    body = [l.split("\t") for l in read_gz_lines("v150_smashmem.txt.gz")[1:-1]]
    assert len(body) == 1407
    assert sum(f[5] == "1" for f in body) >= 100 and sum(f[5] == "0" for f in body) >= 100
    # fed as fixed-length rows the trimmed reads would not give this: the
    # reverse-strand position depends on the mate's own length
    assert g["positions"] != V.golden("s150")["positions"]


@pytest.mark.parametrize("packed", [False, True])
def test_emulated_search_with_lengths_equals_oracle(tiny_ix, packed):
    """the device search kernel (tools/sm_emu: k_prep / k_prep_direct records,
    k_mam_sm with per-read lengths) in the geometry of the longest read, as
    the variable-length pipeline launches it: every mate's match list == the
    oracle's longSA::MAM restatement (mates under min_len: none)"""
    tiny_ix.accel()
    e = sm_emu.Emu(tiny_ix, packed=packed)
    for prefix, cap, width in (("s150", None, 150), ("s150", None, 255), ("s100", 100, 100)):
        mates = V.mixed_mates(prefix, cap=cap, n_pairs=150, trim=True)
        lens = np.array([len(m) for m in mates], np.uint16)
        got, _ = e.map(V.rows_of(mates, width), lens=lens, cap=width - 19)
        for i, m in enumerate(mates):
            assert got[i] == tiny_ix.search(m), (prefix, width, i)
            assert len(m) >= 20 or got[i] == []


def test_prepare_reads_mixed_lengths():
    rows = S.prepare_reads([b"ACGTN", b"", b"acgtacgT"], max_len=8)
    assert rows.dtype == np.uint8 and rows.shape == (3, 8)
    assert rows.tobytes() == b"acgtz\0\0\0" + b"\0" * 8 + b"acgtacgt"
    with pytest.raises(S.SmashError, match="read 1 has 9 bases"):
        S.prepare_reads([b"A", b"ACGTACGTA"], max_len=8)
    with pytest.raises(S.SmashError, match="zero byte"):
        S.prepare_reads([b"A\0C"], max_len=8)
    # the fixed-length form is what it was
    raw = np.frombuffer(b"ACGN" + b"nNaC", np.uint8).reshape(2, 4)
    assert S.prepare_reads(raw).tobytes() == b"acgz" + b"nzac"
    assert np.array_equal(S.prepare_reads(interleaved_reads("s150")), interleaved_reads("s150"))


def test_cli_error_text_names_the_option(v150_files, tmp_path):
    (r1, r2), _ = v150_files
    pairs = smash_cli.fastq_pairs(r1, r2)
    with pytest.raises(SystemExit, match="same length.*--max-read-len"):
        smash_cli.reads_matrix(pairs)
    with pytest.raises(S.SmashError, match="same length.*--max-read-len"):
        smash_cli._read_pairs(r1, r2, 0)
    with pytest.raises(SystemExit, match="longer than --max-read-len 100"):
        smash_cli.reads_matrix(pairs, 100)
    rows = smash_cli.reads_matrix(pairs, 150)
    assert np.array_equal(rows, V.rows_of(V.mixed_mates("v150"), 150))
    names, rows2 = smash_cli._read_pairs(r1, r2, 150)
    assert np.array_equal(rows2, rows)
    ap_err = pytest.raises(SystemExit, match="--max-read-len must be 1..255")
    with ap_err:
        smash_cli._max_read_len(type("A", (), {"max_read_len": 300})())
    assert smash_cli._max_read_len(type("A", (), {"max_read_len": 0})()) == 0
    assert smash_cli._max_read_len(type("A", (), {"max_read_len": 150})()) == 150


def test_shard_reader_refuses_the_flag(v150_files):
    """smash_fastq_shard_open answers SMASH_ERR_UNSUPPORTED to SMASH_LEN_VAR;
    dist.open_fastq goes to the whole-input index for mixed lengths"""
    import ctypes as C
    from dist import open_fastq
    _, (r1, r2) = v150_files
    gather = lambda b: [b]                                           # noqa: E731 (world 1)
    with pytest.raises(S.SmashError) as e:
        S.FastqShards(r1, r2, 0, 1, gather, read_len=VAR | 150)
    assert e.value.code == S.SMASH_ERR_UNSUPPORTED
    sc = type("SC", (), {"rank": 0, "world": 1,
                         "comm": type("Cm", (), {"all_gather_bytes": staticmethod(gather)})()})()
    fq = open_fastq(sc, r1, r2, read_len=VAR | 150)
    assert isinstance(fq, S.FastqIndex) and (fq.n, fq.L) == (600, 150)
    assert C.c_uint32(VAR | 150).value == 0x80000096
