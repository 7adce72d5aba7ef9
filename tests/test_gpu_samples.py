"""Many samples in one run (smash_pipeline_samples): a run's pairs are cut into
contiguous samples by a table first[0..S], and every sample must come out
exactly as a run of its own pairs alone does -- its count row, its six
counters and every pair's keep flag.  The yardstick is the plain pipeline
(no table): reset, then the sample's pairs alone; for the replicas and the
touching inputs also the oracle chain per sample.  All integers, no tolerance.
tests/samples_inputs.py builds the inputs, tests/test_samples_inputs.py checks
them on the CPU.

The emit kernel's counter paths: with the default short-run threshold (1024
pairs) every run of a sample inside a 7-pair batch is short, so the default
cases take the direct global atomics.  SMASH_BIN_SHORT=4 puts runs of 4 to 7
pairs on the LDS side: of ragged, the samples of 1, 2 and 3 pairs stay direct
and the runs of the 40-pair sample and of the rest go through the LDS sum and
the flush at the boundary; with SMASH_BIN_FLUSH=2 the overflow flush too."""
import gzip

import numpy as np
import pytest

import key_rows_inputs as K
import samples_inputs as SI
from conftest import gold

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import smashgpu as S  # noqa: E402

FIELDS = ("pairs", "key_pairs", "dupe_pairs", "positions", "dups", "kept")


@pytest.fixture(scope="module")
def gix(tiny_fa):
    return S.Index.from_fasta(tiny_fa)


@pytest.fixture(scope="module")
def setup():
    return SI.tiny_setup()


def six(st):
    return tuple(int(getattr(st, f)) for f in FIELDS)


def make_pipe(gix, setup, L, capacity, starts=None, var_len=False):
    cs, st = setup
    return S.Pipeline(gix, cs, st if starts is None else starts, L, K.BATCH,
                      dedup_capacity=capacity, var_len=var_len)


def single(pipe, reads):
    """one plain run over reads in batches of K.BATCH: (counts, the six
    counters, keep flags of the keyed pairs)"""
    n = reads.shape[0] // 2
    pipe.reset()
    pipe.set_samples(None)
    c = torch.zeros(len(pipe.bins), dtype=torch.int64, device="cuda")
    keep = []
    if n:
        d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    for b0 in range(0, n, K.BATCH):
        b = min(n, b0 + K.BATCH) - b0
        pipe.count_batch(d[2 * b0:2 * (b0 + b)], b, c)
        nk, kp, _ = pipe.peek(b)
        keep += [bool(k) and m >= 0 for k, m in zip(kp.tolist(), nk.tolist())]
    return c.cpu().numpy().tolist(), six(pipe.stats()), keep


def multi(pipe, reads, first, how="batch", before_batch=None):
    """the run with the table set: (count rows, the six counters per sample,
    keep flags or None, the run's six counters)"""
    n = reads.shape[0] // 2
    pipe.reset()
    pipe.set_samples(first)
    c = torch.zeros((len(first) - 1, len(pipe.bins)), dtype=torch.int64, device="cuda")
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    keep = None
    if how == "batches":
        pipe.count_batches(d, n, K.BATCH, c)
    else:
        keep = []
        for b0 in range(0, n, K.BATCH):
            b = min(n, b0 + K.BATCH) - b0
            if before_batch:
                before_batch(pipe, b0)
            pipe.count_batch(d[2 * b0:2 * (b0 + b)], b, c)
            nk, kp, _ = pipe.peek(b)
            keep += [bool(k) and m >= 0 for k, m in zip(kp.tolist(), nk.tolist())]
    ss = [six(x) for x in pipe.sample_stats()]
    return c.cpu().numpy().tolist(), ss, keep, six(pipe.stats())


def check(got, refs, first):
    """got (multi) against the samples' own runs (single)"""
    rows, ss, keep, run = got
    assert len(rows) == len(refs) == len(ss)
    for s, ref in enumerate(refs):
        assert rows[s] == ref[0], "sample %d counts" % s
        assert ss[s] == ref[1], "sample %d statistics" % s
        if keep is not None:
            assert keep[first[s]:first[s + 1]] == ref[2], "sample %d keep flags" % s
    assert run == tuple(sum(r[1][k] for r in refs) for k in range(6))


_REFS = {}


@pytest.fixture(scope="module")
def case(gix, setup):
    """name -> (reads, first, the samples' own single runs): each computed
    once with the plain pipeline and left unchanged"""
    def get(name):
        if name not in _REFS:
            reads, first = SI.INPUTS[name]()
            pipe = make_pipe(gix, setup, reads.shape[1], reads.shape[0] // 2)
            refs = [single(pipe, part) for part in SI.split(reads, first)]
            assert sum(r[1][5] > 0 for r in refs) >= 2   # real work in two samples at least
            _REFS[name] = (reads, first, refs)
        return _REFS[name]
    yield get
    _REFS.clear()


ALL = sorted(SI.INPUTS)


@pytest.mark.parametrize("how", ["batch", "batches"])
@pytest.mark.parametrize("name", ALL)
def test_samples_equal_their_own_runs(gix, setup, case, name, how):
    """(default threshold: every run is short, the direct global atomics)"""
    reads, first, refs = case(name)
    pipe = make_pipe(gix, setup, reads.shape[1], reads.shape[0] // 2)
    check(multi(pipe, reads, first, how), refs, first)


@pytest.mark.parametrize("name", ["replicas"] + ["touching_" + v for v in sorted(SI.TOUCHING)])
def test_samples_equal_the_oracle_chain(gix, setup, tiny_ix, case, name):
    reads, first, _ = case(name)
    pipe = make_pipe(gix, setup, reads.shape[1], reads.shape[0] // 2)
    rows, ss, _, _ = multi(pipe, reads, first, "batches")
    seen = {}
    for s, part in enumerate(SI.split(reads, first)):
        key = part.tobytes()
        if key not in seen:
            seen[key] = SI.oracle_run(tiny_ix, part)
        counts, totals, _ = seen[key]
        assert rows[s] == counts and ss[s][3:6] == totals
    if name.startswith("touching"):
        assert (ss[0][4], ss[1][4]) == SI.TOUCHING_DUPS


def test_one_plain_run_is_not_the_samples(gix, setup, case):
    """The case the code without sample tables cannot pass: the replicas as
    one plain run lose samples 2 and 3 whole (every key is a duplicate of
    sample 1's), with a table each replica counts like the first."""
    assert hasattr(S.lib(), "smash_pipeline_samples")
    assert hasattr(S.lib(), "smash_pipeline_sample_stats")
    reads, first, refs = case("replicas")
    pipe = make_pipe(gix, setup, reads.shape[1], reads.shape[0] // 2)
    plain = single(pipe, reads)
    rows, ss, keep, run = multi(pipe, reads, first)
    assert rows[0] == rows[1] == rows[2] == refs[0][0]
    assert plain[0] == rows[0]                       # one run: only sample 1 is counted
    assert not any(plain[2][first[1]:]) and any(keep[first[1]:first[2]]) and any(keep[first[2]:])
    assert plain[1][5] == ss[0][5] and run[5] == 3 * plain[1][5]
    assert plain[1][2] > run[2]


@pytest.mark.parametrize("name", ["replicas", "long"])
def test_two_hash_bits(gix, setup, case, name, monkeypatch):
    """SMASH_KEY_HASH_BITS=2: every probe walk meets the other samples' keys
    of the same words, in rows and (long) in arena records, and must tell
    them apart by sample"""
    monkeypatch.setenv("SMASH_KEY_HASH_BITS", "2")
    reads, first, refs = case(name)
    pipe = make_pipe(gix, setup, reads.shape[1], reads.shape[0] // 2)
    check(multi(pipe, reads, first), refs, first)
    check(multi(pipe, reads, first, "batches"), refs, first)


def test_set_grows_mid_run(gix, setup, case):
    """ragged with a capacity of one batch (the set grows as the batches come,
    the table set), and an explicit reserve_keys between two batches"""
    reads, first, refs = case("ragged")
    n = reads.shape[0] // 2
    pipe = make_pipe(gix, setup, reads.shape[1], 1)
    assert pipe.key_capacity < n
    check(multi(pipe, reads, first), refs, first)
    assert pipe.key_capacity >= n
    pipe = make_pipe(gix, setup, reads.shape[1], n)

    def grow(p, b0):
        if b0 == 9 * K.BATCH:
            p.reserve_keys(8 * n)
            assert p.key_capacity >= 8 * n
    check(multi(pipe, reads, first, before_batch=grow), refs, first)


@pytest.mark.parametrize("env", [{"SMASH_BIN_LDS": "0"},
                                 {"SMASH_BIN_SHORT": "4"},
                                 {"SMASH_BIN_SHORT": "4", "SMASH_BIN_FLUSH": "2"},
                                 {"SMASH_BIN_SHORT": "0", "SMASH_BIN_FLUSH": "2"}],
                         ids=["global_only", "lds_runs", "lds_flush2", "all_lds_flush2"])
@pytest.mark.parametrize("name", ["ragged", "replicas", "touching_gap"])
def test_counter_paths(gix, setup, case, name, env, monkeypatch):
    """global atomics only; runs of >= 4 pairs summed in LDS and flushed at the
    boundary, shorter ones direct (see the module docstring); a flush
    threshold of 2, so halves overflow into the sample's row mid-run; and every
    run on the LDS side"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads, first, refs = case(name)
    pipe = make_pipe(gix, setup, reads.shape[1], reads.shape[0] // 2)
    check(multi(pipe, reads, first), refs, first)
    check(multi(pipe, reads, first, "batches"), refs, first)


def test_more_bins_than_the_lds_parts_hold(gix, setup):
    """a synthetic table of 4 * 77 824 + 7 bins (above kBinPartsMax *
    kBinPart): the sample form with global atomics only"""
    cs, _ = setup
    starts = np.arange(4 * 77824 + 7, dtype=np.int64)
    reads, first = SI.ragged()
    n = reads.shape[0] // 2
    pipe = make_pipe(gix, setup, reads.shape[1], n, starts=starts)
    refs = [single(pipe, part) for part in SI.split(reads, first)]
    assert sum(max(r[0]) > 0 for r in refs) >= 3
    check(multi(pipe, reads, first), refs, first)


def test_variable_length_mode(gix, setup):
    """ragged over trimmed copies of its reads (the v150 trim rule), variable-
    length mode on"""
    from varlen_reads import vlen
    from varlen_util import rows_of
    reads, first = SI.ragged()
    mates = []
    for r in reads:
        s = r.tobytes()
        mates.append(s[:vlen(s.upper().replace(b"Z", b"N"))])
    assert len({len(m) for m in mates}) > 20
    rows = rows_of(mates, reads.shape[1])
    n = rows.shape[0] // 2
    pipe = make_pipe(gix, setup, rows.shape[1], n, var_len=True)
    refs = [single(pipe, part) for part in SI.split(rows, first)]
    assert sum(r[1][5] > 0 for r in refs) >= 3
    check(multi(pipe, rows, first), refs, first)
    check(multi(pipe, rows, first, "batches"), refs, first)


def test_table_off_again(gix, setup, case):
    """a table, a run, then no table: the plain run on the same pipeline is a
    fresh pipeline's"""
    reads, first, refs = case("replicas")
    n = reads.shape[0] // 2
    pipe = make_pipe(gix, setup, reads.shape[1], n)
    check(multi(pipe, reads, first, "batches"), refs, first)
    assert single(pipe, reads) == single(make_pipe(gix, setup, reads.shape[1], n), reads)
    assert pipe.sample_stats() == []


def test_errors(gix, setup, case, tmp_path):
    reads, first, refs = case("ragged")
    n = reads.shape[0] // 2
    pipe = make_pipe(gix, setup, reads.shape[1], n)
    d = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
    c = torch.zeros((len(first) - 1, len(pipe.bins)), dtype=torch.int64, device="cuda")

    def code(fn):
        with pytest.raises(S.SmashError) as e:
            fn()
        return e.value.code

    pipe.reset()
    assert code(lambda: pipe.set_samples([0, 5, 3, n])) == S.SMASH_ERR_ARG     # descending
    assert code(lambda: pipe.set_samples([1, 5, n])) == S.SMASH_ERR_ARG        # first[0] != 0
    assert code(lambda: pipe.set_samples(list(range(65537)))) == S.SMASH_ERR_ARG
    pipe.set_samples(first)
    pipe.count_batch(d[:2 * K.BATCH], K.BATCH, c)
    assert code(lambda: pipe.set_samples(first)) == S.SMASH_ERR_ARG            # mid-run
    assert code(lambda: pipe.set_samples(None)) == S.SMASH_ERR_ARG
    # a batch past first[S]: refused when queued, nothing of it counted
    pipe.reset()
    pipe.set_samples([0, 3, 10])
    pipe.count_batch(d[:2 * K.BATCH], K.BATCH, c)
    assert code(lambda: pipe.count_batch(d[:2 * K.BATCH], K.BATCH, c)) == S.SMASH_ERR_ARG
    assert code(lambda: pipe.count_batches(d, n, K.BATCH, c)) == S.SMASH_ERR_ARG
    assert sum(x[0] for x in map(six, pipe.sample_stats())) == K.BATCH
    # the phase calls and the file feed
    tail = torch.empty(2, dtype=torch.int64, device="cuda")
    assert code(lambda: pipe.phase_map(d[:2 * K.BATCH], K.BATCH)) == S.SMASH_ERR_UNSUPPORTED
    assert code(lambda: pipe.phase_export(1, 0)) == S.SMASH_ERR_UNSUPPORTED
    assert code(lambda: pipe.phase_positions(tail)) == S.SMASH_ERR_UNSUPPORTED
    assert code(lambda: pipe.phase_bin(None, c)) == S.SMASH_ERR_UNSUPPORTED
    fq = []
    for k in (1, 2):
        p = tmp_path / ("r%d.fq" % k)
        p.write_bytes(gzip.open(gold("s150_r%d.fq.gz" % k)).read())
        fq.append(str(p))
    assert code(lambda: pipe.count_fastq([fq[0]], [fq[1]], c)) == S.SMASH_ERR_UNSUPPORTED
    # a counts tensor of one row is refused before anything runs
    pipe.reset()
    with pytest.raises(S.SmashError, match="counts tensor"):
        pipe.count_batch(d[:2 * K.BATCH], K.BATCH, c[0])
    # the pipeline is usable afterwards
    check(multi(pipe, reads, first), refs, first)


def test_cli_count_many(tmp_path, tiny_fa, monkeypatch):
    """count-many over s150, v150 and s150 again under another ID writes, per
    ID, the files of `count ID ...`: equal keys in two samples go through the
    files too"""
    import shutil

    import smash_cli
    fa = tmp_path / "tiny.fa"
    shutil.copy(tiny_fa, fa)
    monkeypatch.chdir(tmp_path)
    smash_cli.main(["--ref", str(fa), "index"])
    bindir = tmp_path / "bins"
    bindir.mkdir()
    (bindir / "bins.txt").write_text(open(gold("tiny_bins.txt")).read())
    fq = {s: [gold("%s_r%d.fq.gz" % (s, k)) for k in (1, 2)] for s in ("s150", "v150")}
    ids = [("one", "s150"), ("trimmed", "v150"), ("again", "s150")]
    with open("lane.tsv", "w") as f:
        f.write("\n".join("%s\t%s\t%s\n" % ((i,) + tuple(fq[s])) for i, s in ids))
    smash_cli.main(["--ref", str(fa), "count-many", "lane.tsv", str(bindir),
                    "--max-read-len", "150", "--batch", "97"])
    for s in ("s150", "v150"):
        smash_cli.main(["--ref", str(fa), "count", "ref_" + s, fq[s][0], fq[s][1], str(bindir),
                        "--max-read-len", "150", "--batch", "97"])
    for i, s in ids:
        for ext in (".varbin.txt", ".stats.txt"):
            assert open(i + ext, "rb").read() == open("ref_" + s + ext, "rb").read()
    assert open("one.varbin.txt").read() == open(gold("s150_varbin.txt")).read()
