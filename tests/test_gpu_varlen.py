"""Pairs of mixed read lengths through the whole count chain on the device
(Pipeline(var_len=True): a mate's length is the offset of the first zero
byte of its row) against the reference's goldens of the trimmed s150 pairs
(tests/golden/v150_*, tools/make_golden_varlen.sh) and the oracle's per-read
primitives.  Every comparison is exact.

Marked `gpu` (MI355X).  The tiny genome is indexed once per element width:
the default (4-byte SA / ISA) and SMASH_IDX_BYTES=8 (packed words, map
hints).
"""
import gzip
import os

import numpy as np
import pytest

from conftest import gold, interleaved_reads, load_bins, load_chrom_sizes, read_gz_lines

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402
import varlen_util as V  # noqa: E402


@pytest.fixture(scope="module", params=[4, 8])
def gix(request, tiny_fa):
    assert torch.cuda.is_available()
    old = os.environ.get("SMASH_IDX_BYTES")
    if request.param == 8:
        os.environ["SMASH_IDX_BYTES"] = "8"
    try:
        ix = S.Index.from_fasta(tiny_fa)
    finally:
        if old is None:
            os.environ.pop("SMASH_IDX_BYTES", None)
        else:
            os.environ["SMASH_IDX_BYTES"] = old
    assert ix.info.idx_bytes == request.param
    return ix


@pytest.fixture(scope="module")
def v150():
    """the trimmed mates, the trim rule's lengths and the reference's results"""
    mates = V.mixed_mates("v150")
    lens = V.trim_rule_lengths("s150")
    assert [len(m) for m in mates] == lens
    return mates, np.array(lens, np.uint16), V.golden("v150")


@pytest.fixture(scope="module")
def v150_chain(tiny_ix, v150):
    return V.Chain(tiny_ix, v150[0])


CS = load_chrom_sizes(gold("tiny_chrom_sizes.txt"))
NAME_AT = {v: k for k, v in CS.items()}
STARTS = load_bins(gold("tiny_bins.txt"))[1]


def make_pipe(ix, L, max_pairs, native=False, var_len=True):
    # (the key set holds a whole run's pairs, whatever the batch size)
    return S.Pipeline(ix, CS, STARTS, L, max_pairs, read_stride=S.read_stride(L) if native else 0,
                      dedup_capacity=2000, var_len=var_len)


def run(pipe, rows, batch=None, batches=False):
    """rows: [2n, pipe.stride] host rows.  Returns counts, stats, positions
    lines, and the per-batch lengths the device took."""
    n = rows.shape[0] // 2
    batch = batch or n
    counts = torch.zeros(len(STARTS), dtype=torch.int64, device="cuda")
    pipe.reset()
    lines, lens = [], []
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    if batches:
        pipe.count_batches(d, n, batch, counts)
    else:
        for b0 in range(0, n, batch):
            b1 = min(n, b0 + batch)
            pipe.count_batch(d[2 * b0:2 * b1], b1 - b0, counts)
            pos0, absp = pipe.positions()
            lines += ["%s %d" % (NAME_AT[a - p], p) for p, a in zip(pos0.tolist(), absp.tolist())]
            lens.append(pipe.peek_lens(b1 - b0))
    st = pipe.stats()
    assert st.error == 0
    return counts.cpu().numpy().astype(np.uint64).tolist(), st, lines, \
        (np.concatenate(lens) if lens else None)


def check_golden(g, counts, st, lines=None):
    assert counts == g["counts"]
    assert (st.positions, st.dups, st.kept) == g["totals"]
    assert "%d dupes\t%d non-dupes" % (st.dupe_pairs, st.key_pairs - st.dupe_pairs) == g["summary"]
    if lines is not None:
        assert lines == g["positions"]


@pytest.mark.parametrize("batch", [600, 7])
@pytest.mark.parametrize("native", [False, True])
def test_v150_equals_reference(gix, v150, native, batch):
    """counts, (positions, dups, kept), the positions list, the smashMEM
    summary line; dense and native rows; one batch and batches of 7 (both
    search sets, the carried de-dup and adjacent-dup state); the lengths the
    device read == the trim rule."""
    mates, lens, g = v150
    pipe = make_pipe(gix, 150, 600, native)
    counts, st, lines, got_lens = run(pipe, V.rows_of(mates, 150, pipe.stride), batch)
    assert np.array_equal(got_lens, lens)
    assert st.pairs == 600
    check_golden(g, counts, st, lines)


@pytest.mark.parametrize("native", [False, True])
def test_v150_count_batches(gix, v150, native):
    """smash_count_batches: the searches of consecutive batches overlap on the
    two search streams, each set with its own lengths."""
    mates, _, g = v150
    pipe = make_pipe(gix, 150, 64, native)
    counts, st, _, _ = run(pipe, V.rows_of(mates, 150, pipe.stride), 64, batches=True)
    check_golden(g, counts, st)


def test_v150_per_pair_equals_oracle(gix, v150, v150_chain):
    """Per-pair kept hit lists (smashMEM output before de-dup) and first-wins
    keep flags == the oracle's search -> resolve -> tag -> smash_pair."""
    mates, _, _ = v150
    pipe = make_pipe(gix, 150, 600)
    run(pipe, V.rows_of(mates, 150))
    nk, keep, hits = pipe.peek(600)
    for q, exp in enumerate(v150_chain.keys):
        if exp is None:
            assert nk[q] == -1, q
            continue
        got = [(int(w >> 48), int(w & 0xFFFFFFFFFFFF)) for w in hits[q, :max(nk[q], 0)]]
        assert got == exp, (q, got, exp)
        assert bool(keep[q]) == v150_chain.keep[q], q


def test_one_bad_mask_chunk_geometry(gix, tiny_ix):
    """read_len <= 128 (one bad-mask chunk per record): the first 500 s100
    pairs trimmed by the same rule capped at 100, against the oracle chain."""
    mates = V.mixed_mates("s100", cap=100, n_pairs=500, trim=True)
    assert len(mates) == 1000 and max(len(m) for m in mates) == 100
    assert min(len(m) for m in mates) < 20
    exp = V.Chain(tiny_ix, mates)
    for native in (False, True):
        pipe = make_pipe(gix, 100, 500, native)
        counts, st, lines, lens = run(pipe, V.rows_of(mates, 100, pipe.stride), 500)
        assert lens.tolist() == [len(m) for m in mates]
        assert counts == exp.counts.tolist()
        assert (st.positions, st.dups, st.kept) == exp.totals
        assert (st.key_pairs, st.dupe_pairs) == (exp.key_pairs, exp.dupe_pairs)
        assert lines == exp.lines


@pytest.mark.parametrize("native", [False, True])
def test_full_length_rows_equal_s150(gix, native):
    """every row full (no zero byte among its read_len bytes): the
    fixed-length result, the reference's s150 goldens"""
    reads = interleaved_reads("s150")
    pipe = make_pipe(gix, 150, 600, native)
    rows = np.zeros((1200, pipe.stride), np.uint8)
    rows[:, :150] = reads
    counts, st, lines, lens = run(pipe, rows)
    assert (lens == 150).all()
    check_golden(V.golden("s150"), counts, st, lines)


def test_row_width_does_not_matter(gix, v150):
    """a read_len 255 pipeline fed v150 gives the v150 result"""
    mates, lens, g = v150
    for native in (False, True):
        pipe = make_pipe(gix, 255, 600, native)
        counts, st, lines, got_lens = run(pipe, V.rows_of(mates, 255, pipe.stride), 200)
        assert np.array_equal(got_lens, lens)
        check_golden(g, counts, st, lines)


def test_var_len_off_again(gix, v150):
    """the mode switched between runs on one pipeline: s150 (fixed), v150
    (variable), s150 again -- each the reference's result"""
    mates, _, g = v150
    reads = interleaved_reads("s150")
    pipe = make_pipe(gix, 150, 300, var_len=False)
    for var in (False, True, False):
        pipe.set_var_len(var)
        rows = V.rows_of(mates, 150) if var else reads
        counts, st, lines, lens = run(pipe, rows, 300)
        check_golden(g if var else V.golden("s150"), counts, st, lines)
        if not var:
            assert (lens == 150).all()


def test_var_len_refused_while_a_search_is_pending(gix, v150):
    mates, _, _ = v150
    pipe = make_pipe(gix, 150, 100, var_len=False)
    d = torch.from_numpy(V.rows_of(mates[:400], 150)).cuda()
    pipe.reset()
    pipe.phase_map_ahead(d[:200], 100, d[200:], 100)
    with pytest.raises(S.SmashError):
        pipe.set_var_len(True)
    pipe.reset()
    pipe.set_var_len(True)
    torch.cuda.synchronize()


def test_two_thread_ranks_equal_single(gix, v150, monkeypatch):
    """W = 2 ranks of the real sharded step (dist.ShardedCounter over
    tests/thread_ranks.py, look-ahead searches on) over v150 == the single-GPU
    counts and the reference's."""
    import thread_ranks
    mates, _, g = v150

    def var_pipes(ix, world, cs, starts, L, batch, capacity):
        pipes = [S.Pipeline(ix, cs, starts, L, batch, dedup_capacity=capacity, var_len=True)
                 for _ in range(world)]
        counts = [torch.zeros(len(starts), dtype=torch.int64, device="cuda") for _ in range(world)]
        return pipes, counts
    monkeypatch.setattr(thread_ranks, "make_pipes", var_pipes)
    d = torch.from_numpy(V.rows_of(mates, 150)).cuda()
    total, (pos, dups, kept, dupe_pairs) = thread_ranks.run_resident(gix, d, 2, 60, STARTS, CS)
    pipe = make_pipe(gix, 150, 600)
    counts, st, _, _ = run(pipe, V.rows_of(mates, 150))
    assert total.tolist() == counts == g["counts"]
    assert (pos, dups, kept) == g["totals"]
    assert dupe_pairs == st.dupe_pairs


def _gunzip(name, dst):
    with gzip.open(gold(name), "rb") as f, open(dst, "wb") as o:
        o.write(f.read())
    return str(dst)


@pytest.mark.parametrize("plain", [False, True])
def test_v150_count_fastq(gix, v150, tmp_path, plain):
    """the file feed (smash_count_fastq) on a variable-length pipeline reads
    with SMASH_LEN_VAR | read_len: gzip files through the streaming reader,
    plain ones through the parallel reader"""
    _, _, g = v150
    r1, r2 = gold("v150_r1.fq.gz"), gold("v150_r2.fq.gz")
    if plain:
        r1, r2 = _gunzip("v150_r1.fq.gz", tmp_path / "r1.fq"), _gunzip("v150_r2.fq.gz", tmp_path / "r2.fq")
    for native in (False, True):
        pipe = make_pipe(gix, 150, 250, native)
        counts = torch.zeros(len(STARTS), dtype=torch.int64, device="cuda")
        pipe.reset()
        fs = pipe.count_fastq([r1], [r2], counts)
        assert fs["pairs"] == 600
        st = pipe.stats()
        check_golden(g, counts.cpu().numpy().astype(np.uint64).tolist(), st)


def test_memsam_mixed_lengths(tmp_path, tiny_fa):
    """`smash_cli memsam -nomap --tag` on the trimmed pairs' unmapped SAM
    (fastqs_to_sam's lines, fastqs_to_sam.cpp:80-96) == the reference's tagged
    mapout, as a sorted line set (mixed lengths need no option, as with
    mummer); batches of 97 pairs: mixed and, by chance, none uniform"""
    import re
    import smash_cli
    sam = tmp_path / "v150.sam"
    with open(sam, "w") as o:
        for a, b in zip(_fq("v150_r1.fq.gz"), _fq("v150_r2.fq.gz")):
            for flag, (name, opt, seq, qual) in ((77, a), (141, b)):
                o.write("%s\t%d\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tXO:Z:%s\n"
                        % (name, flag, seq.replace("N", "Z"), qual, opt))
    out = tmp_path / "mapout.txt"
    smash_cli.main(["--ref", tiny_fa, "memsam", "-nomap", "--tag", "--out", str(out),
                    "--batch", "97", str(sam)])
    munge = re.compile(r"^(\S+?)/\S+/\d+")   # smash_mapping.sh:23's perl, before mappability_tag
    got = sorted(munge.sub(r"\1", l) for l in open(out).read().splitlines()
                 if not l.startswith("@"))
    assert got == sorted(read_gz_lines("v150_mapout_tagged_full.txt.gz"))


def _fq(name):
    lines = read_gz_lines(name)
    return [tuple(lines[i][1:].split()[:2]) + (lines[i + 1], lines[i + 3])
            for i in range(0, len(lines) - 3, 4)]


def test_cli_count_and_map_with_max_read_len(tmp_path, tiny_fa, monkeypatch):
    """`smash_cli count ... --max-read-len 150` on the v150 FASTQ pair writes
    the reference's varbin.txt (file-fed path, and the --sam path); `map`
    writes its positions and summary; without the option the error names it."""
    import shutil
    import smash_cli
    fa = str(tmp_path / "tiny.fa")
    shutil.copy(tiny_fa, fa)
    monkeypatch.chdir(tmp_path)
    os.makedirs(fa + ".bin")
    shutil.copy(gold("tiny_chrom_sizes.txt"), fa + ".bin/chrom_sizes.txt")
    bindir = tmp_path / "bins"
    bindir.mkdir()
    shutil.copy(gold("tiny_bins.txt"), bindir / "bins.txt")
    r1, r2 = gold("v150_r1.fq.gz"), gold("v150_r2.fq.gz")
    exp_rows = open(gold("v150_varbin.txt")).read()
    part = open(gold("v150_varbin_stats_partial.txt")).read()
    smash_cli.main(["--ref", fa, "count", "v", r1, r2, str(bindir), "--out", "c.txt",
                    "--max-read-len", "150", "--batch", "250"])
    assert open("c.txt").read() == exp_rows
    assert open("v.stats.txt").read().startswith(part)
    smash_cli.main(["--ref", fa, "map", "v", r1, r2, "--batch", "97", "--max-read-len", "200"])
    assert open("v.positions.txt").read() == open(gold("v150_positions.txt")).read()
    assert open("v.smash.summary.txt").read() == "5 dupes\t554 non-dupes\n"
    sam = tmp_path / "v150.sam"
    with open(sam, "w") as o:
        for a, b in zip(_fq("v150_r1.fq.gz"), _fq("v150_r2.fq.gz")):
            for flag, (name, opt, seq, qual) in ((77, a), (141, b)):
                o.write("%s\t%d\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tXO:Z:%s\n"
                        % (name, flag, seq.replace("N", "Z"), qual, opt))
    smash_cli.main(["--ref", fa, "count", "v", "--sam", str(sam), str(bindir), "--out", "c2.txt",
                    "--max-read-len", "150"])
    assert open("c2.txt").read() == exp_rows
    with pytest.raises(S.SmashError, match="--max-read-len"):
        smash_cli.main(["--ref", fa, "map", "v", r1, r2])
    with pytest.raises(S.SmashError, match="pipeline's read length.*--max-read-len"):
        smash_cli.main(["--ref", fa, "count", "v", r1, r2, str(bindir)])
    with pytest.raises(S.SmashError, match="longer than the (pipeline's )?maximum read length, 100"):
        smash_cli.main(["--ref", fa, "count", "v", r1, r2, str(bindir), "--max-read-len", "100"])
