"""The bin design on the device (csrc/bins.hip): smash_bins_design and
smash_bins_design_raw against the rule in numpy (tests/bins_spec.py) over the
CPU oracle's map.bin, which is pinned to the reference; crafted maps that put
unique bases on tile edges; a map whose byte offsets pass 2^32; the
mappability scan as a second opinion on n_unique; `smash_cli.py bins` feeding
`count`.  Marked `gpu`."""
import os

import numpy as np
import pytest

from conftest import gold

import bins_spec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import oracle as O  # noqa: E402
import smash_cli  # noqa: E402
import smashgpu as S  # noqa: E402

ERR_ARG = -1


def expect(map2, sizes, off, k, nbins, text=None, text_start=None):
    try:
        return bins_spec.design(map2, sizes, off, k, nbins, text, text_start)
    except ValueError:
        return "ERR_ARG", None


def check_table(rec, rows):
    got = bins_spec.rows_of(rec)
    assert len(got) == len(rows)
    if got != rows:
        bad = [i for i, (a, b) in enumerate(zip(got, rows)) if a != b]
        raise AssertionError("%d rows differ, first %d: got %r, want %r"
                             % (len(bad), bad[0], got[bad[0]], rows[bad[0]]))
    assert np.all(np.diff(rec["abspos"]) > 0)
    assert not rec["reserved"].any()


# ---------------------------------------------------------------------------
# tiny genome: the index's own map and text
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tiny_fa, tiny_ix):
    dix = S.Index.from_fasta(tiny_fa)
    cs = S.read_chrom_sizes(gold("tiny_chrom_sizes.txt"))
    off = S.contig_tables(dix.contigs, dix.contig_sizes, cs)[2]
    return dix, cs, off, tiny_ix.mappability()[2:], tiny_ix


def test_tiny_fixture_has_the_cases_the_design_must_pass(tiny):
    """chr2 starts on a unique base and holds two tiles without one (its N
    run): a prefix value repeated over tiles the bisection must pass over"""
    dix, _, off, omap, _ = tiny
    T = S.bins_tile()
    assert off.tolist() == [0, 120000, 210000, -1, -1]
    right = omap[1::2][120000:210000]
    u = (right >= 1) & (right <= 36)
    assert u[0]
    assert sum(1 for a in range(0, len(u), T) if not u[a:a + T].any()) >= 2


@pytest.mark.parametrize("k,nbins,per_contig", [
    (36, 3, [1, 1, 1]), (36, 24, [9, 9, 6]), (20, 97, [37, 38, 22]),
    (36, 1000, [402, 372, 226]), (36, 60000, [24114, 22327, 13559])])
def test_tiny_design_equals_the_rule(tiny, k, nbins, per_contig):
    dix, cs, off, omap, oix = tiny
    rows, M = bins_spec.design(omap, dix.contig_sizes, off, k, nbins, oix.T, oix.startpos[0::2])
    rec, gotM = dix.design_bins(cs, k=k, nbins=nbins, unique=True)
    check_table(rec, rows)
    assert gotM.tolist() == M
    assert np.bincount(rec["contig"], minlength=3).tolist() == per_contig
    if nbins == 60000:
        assert set(rec["n_unique"].tolist()) == {3, 4}
    # an offset table in place of the chrom_sizes dict is the same call
    assert np.array_equal(dix.design_bins(off, k=k, nbins=nbins), rec)


def test_design_refuses_bad_arguments(tiny, tiny_fa):
    dix, cs, off, _, _ = tiny
    for kw in (dict(k=0, nbins=24), dict(k=255, nbins=24), dict(k=36, nbins=2)):
        with pytest.raises(S.SmashError) as e:
            dix.design_bins(cs, **kw)
        assert e.value.code == ERR_ARG
    fwd = S.Index.from_fasta(tiny_fa, rcref=False)          # no -rcref: no map.bin
    with pytest.raises(S.SmashError) as e:
        fwd.design_bins(off, k=36, nbins=24)
    assert e.value.code == ERR_ARG


# ---------------------------------------------------------------------------
# mid genome: 4- and 8-byte index, the scan as a second opinion
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    import synth
    g = synth.make_genome("mid")
    T, sp, sz, names = O.text_from_contigs(g)
    oix = O.Index(T, sp, sz, names)
    dix = {}
    old = os.environ.get("SMASH_IDX_BYTES")
    try:
        for w in (4, 8):
            os.environ["SMASH_IDX_BYTES"] = str(w)
            dix[w] = S.Index.create(T, sp, sz, names)
    finally:
        if old is None:
            os.environ.pop("SMASH_IDX_BYTES")
        else:
            os.environ["SMASH_IDX_BYTES"] = old
    assert (dix[4].info.idx_bytes, dix[8].info.idx_bytes) == (4, 8)
    cs, n = {}, 0
    for name, s in g:                      # chrom_sizes.txt (index_setup.sh:28)
        if "_" not in name:
            cs[name] = n
            n += len(s)
    off = S.contig_tables(dix[4].contigs, dix[4].contig_sizes, cs)[2]
    assert int((off >= 0).sum()) == 4
    return oix, dix, off, oix.mappability()[2:]


@pytest.mark.parametrize("k,nbins", [(36, 1000), (24, 50000)])
def test_mid_design_equals_the_rule_on_both_index_widths(mid, k, nbins):
    oix, dix, off, omap = mid
    rows, M = bins_spec.design(omap, dix[4].contig_sizes, off, k, nbins, oix.T,
                               oix.startpos[0::2])
    rec4, M4 = dix[4].design_bins(off, k=k, nbins=nbins, unique=True)
    check_table(rec4, rows)
    assert M4.tolist() == M
    assert np.array_equal(dix[8].design_bins(off, k=k, nbins=nbins), rec4)


def test_mid_fewer_bins_than_binned_contigs_is_an_argument_error(mid):
    _, dix, off, _ = mid
    with pytest.raises(S.SmashError) as e:
        dix[4].design_bins(off, k=36, nbins=3)
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("k,nbins", [(36, 1000), (24, 50000)])
def test_mid_scan_counts_the_designed_bins_to_n_unique(mid, k, nbins):
    """the two kernels agree: smash_mappability_scan over the whole genome,
    binning by the designed starts, counts n_unique into every bin"""
    _, dix, off, _ = mid
    ix = dix[4]
    rec = ix.design_bins(off, k=k, nbins=nbins)
    starts = torch.from_numpy(np.ascontiguousarray(rec["abspos"], np.int64)).cuda()
    counts = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    S.mappability_scan(ix, 0, sum(ix.contig_sizes), k, None, off, starts, nbins, counts, None)
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == rec["n_unique"].tolist()


# ---------------------------------------------------------------------------
# crafted maps through smash_bins_design_raw (no index)
# ---------------------------------------------------------------------------
K = 30


def crafted_sizes():
    T = S.bins_tile()
    return [1, T - 1, T, T + 1, 3 * T + 5]


def crafted_map(right_of):
    """[left, right] pairs of the five contigs; right_of(c, S) -> uint8[S].
    The left bytes all look unique: a kernel that read them would miscount."""
    sizes = crafted_sizes()
    rng = np.random.default_rng(3)
    parts = []
    for c, S_ in enumerate(sizes):
        m = np.empty((S_, 2), np.uint8)
        m[:, 0] = rng.integers(1, K + 1, S_)
        m[:, 1] = right_of(c, S_)
        parts.append(m.reshape(-1))
    return sizes, np.concatenate(parts)


def crafted_text(sizes):
    """the contigs' text with a gap of other bytes before each, N runs and a
    few bytes that are no base at all"""
    rng = np.random.default_rng(4)
    parts, starts, p = [], [], 0
    for S_ in sizes:
        gap = np.frombuffer(b"`tgca$", np.uint8)[:int(rng.integers(1, 7))]
        t = np.frombuffer(b"acgtn", np.uint8)[rng.integers(0, 5, S_)].copy()
        t[rng.integers(0, S_, S_ // 50)] = ord("r")
        if S_ > 200:
            t[100:180] = ord("n")
        parts += [gap, t]
        starts.append(p + len(gap))
        p += len(gap) + S_
    return np.concatenate(parts), np.array(starts, np.uint64)


def run_raw(sizes, map2, off, k, nbins, with_text=True):
    text, ts = crafted_text(sizes)
    d_map = torch.from_numpy(map2).cuda()
    d_text = torch.from_numpy(text).cuda() if with_text else None
    want = expect(map2, sizes, off, k, nbins, text if with_text else None, ts)
    try:
        rec, M = S.bins_design_raw(d_map, d_text, sizes, ts if with_text else None, off, k,
                                   nbins, unique=True)
    except S.SmashError as e:
        assert e.code == ERR_ARG, e
        assert want[0] == "ERR_ARG", "the device refused what the rule accepts: %s" % e
        return None
    assert want[0] != "ERR_ARG", "the device accepted what the rule refuses"
    check_table(rec, want[0])
    assert M.tolist() == want[1]
    return rec


def all_binned(sizes):
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)


def edge_positions(S_):
    T = S.bins_tile()
    return sorted({p for p in (0, T - 1, T, S_ - 1) if 0 <= p < S_})


def test_crafted_every_base_unique():
    rng = np.random.default_rng(5)
    sizes, m = crafted_map(lambda c, S_: rng.integers(1, K + 1, S_))
    off = all_binned(sizes)
    for nbins in (5, 42, 3000):
        assert run_raw(sizes, m, off, K, nbins) is not None
    assert run_raw(sizes, m, off, K, 42, with_text=False) is not None
    total = sum(sizes)
    run_raw(sizes, m, off, K, total)           # as the rule has it (bins of one base)


def test_crafted_no_base_unique():
    rng = np.random.default_rng(6)
    sizes, m = crafted_map(lambda c, S_: np.where(rng.integers(0, 2, S_) == 1, 0,
                                                  rng.integers(K + 1, 256, S_)))
    off = all_binned(sizes)
    rec = run_raw(sizes, m, off, K, 5)          # one bin each
    assert rec is not None and not rec["n_unique"].any()
    assert run_raw(sizes, m, off, K, 6) is None   # a bin to share, nothing to share it by


def test_crafted_unique_bases_on_tile_edges_only():
    def right(c, S_):
        r = np.zeros(S_, np.uint8)
        r[edge_positions(S_)] = K
        return r
    sizes, m = crafted_map(right)
    off = all_binned(sizes)
    outcomes = [run_raw(sizes, m, off, K, nbins) is not None for nbins in range(5, 14)]
    assert outcomes[0] and outcomes[3]          # 5 and 8 bins: tables (see bins_spec)
    assert not all(outcomes)                    # and some count asks a contig for too many
    # the two larger contigs alone: every edge base starts a bin
    off2 = np.array([-1, -1, -1, 0, sizes[3]], np.int64)
    rec = run_raw(sizes, m, off2, K, 7)
    T = S.bins_tile()
    assert rec["start"].tolist() == [0, T - 1, T, 0, T - 1, T, 3 * T + 4]


def test_crafted_right_of_k_plus_one_is_not_unique():
    def right(c, S_):
        r = np.full(S_, K + 1, np.uint8)
        if c == 4:
            r[2 * S.bins_tile() + 17] = K
        return r
    sizes, m = crafted_map(right)
    rec = run_raw(sizes, m, all_binned(sizes), K, 5)
    assert rec["n_unique"].tolist() == [0, 0, 0, 0, 1]
    # and where right alternates between k and k + 1 the bins cut at the k's
    sizes, m = crafted_map(lambda c, S_: K + (np.arange(S_) + c) % 2)
    assert run_raw(sizes, m, all_binned(sizes), K, 5 + 40) is not None


def test_crafted_right_zero_against_one():
    rng = np.random.default_rng(8)
    sizes, m = crafted_map(lambda c, S_: rng.integers(0, 2, S_))
    off = all_binned(sizes)
    for k in (1, K):
        assert run_raw(sizes, m, off, k, 5 + 64) is not None


def test_crafted_as_many_bins_as_unique_bases_and_one_more():
    rng = np.random.default_rng(9)

    def right(c, S_):
        r = np.zeros(S_, np.uint8)
        if c >= 3:
            r[rng.choice(S_, 50, replace=False)] = 1
        else:
            r[:] = 1                             # unbinned: never read
        return r
    sizes, m = crafted_map(right)
    off = np.array([-1, -1, -1, 0, sizes[3]], np.int64)
    rec = run_raw(sizes, m, off, K, 100)         # B = M = 50 for both
    assert rec is not None and set(rec["n_unique"].tolist()) == {1}
    assert np.bincount(rec["contig"]).tolist() == [0, 0, 0, 50, 50]
    assert run_raw(sizes, m, off, K, 101) is None   # B = M + 1


# ---------------------------------------------------------------------------
# byte offsets past 2^32
# ---------------------------------------------------------------------------
def test_offsets_past_32_bits():
    """one contig of 2^31 + 8192 bases: the right byte of its last bases lies
    past byte 2^32 of the map.  64 unique bases, 8 bins; the map never leaves
    the device."""
    T = S.bins_tile()
    S_ = (1 << 31) + 8192
    rng = np.random.default_rng(10)
    pos = np.concatenate([np.sort(rng.choice(T, 32, replace=False)),
                          S_ - 4096 + np.sort(rng.choice(4095, 31, replace=False)),
                          [S_ - 1]]).astype(np.int64)
    assert len(pos) == 64 and np.all(np.diff(pos) > 0)
    d_map = torch.zeros(2 * S_, dtype=torch.uint8, device="cuda")
    d_map[torch.from_numpy(2 * pos + 1).cuda()] = 1
    rows, M = bins_spec.design_positions([pos], [S_], [7], 8)
    rec, gotM = S.bins_design_raw(d_map, None, [S_], None, [7], 36, 8, unique=True)
    del d_map
    check_table(rec, rows)
    assert gotM.tolist() == [64] and rec["n_unique"].tolist() == [8] * 8
    assert int(rec["start"][4]) > 1 << 31 and int(rec["stop"][-1]) == S_


# ---------------------------------------------------------------------------
# end to end: the designed table feeds `count`
# ---------------------------------------------------------------------------
def test_cli_bins_then_count(tmp_path, tiny_fa, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cs = gold("tiny_chrom_sizes.txt")
    smash_cli.main(["--ref", tiny_fa, "bins", "24", "d24", "--chrom-sizes", cs])
    rows, starts = S.read_bins("d24/bins.txt")
    assert len(rows) == 24 and all(len(r) == 6 for r in rows)
    assert [r[0] for r in rows] == ["chr1"] * 9 + ["chr2"] * 9 + ["chrX"] * 6
    assert np.all(np.diff(starts) > 0)
    gc = open("d24/gc.txt").read().split("\n")
    assert gc[0].startswith("bin.chrom\tbin.start\tbin.end\t") and len(gc) == 26
    assert all(len(l.split("\t")) == 10 and 0.3 < float(l.split("\t")[7]) < 0.7 for l in gc[1:-1])
    assert not os.path.exists("d24/bad.txt")
    smash_cli.main(["--ref", tiny_fa, "count", "s", gold("s100_r1.fq.gz"), gold("s100_r2.fq.gz"),
                    "d24", "--chrom-sizes", cs])
    out = [l.split("\t") for l in open("s.varbin.txt").read().splitlines()]
    assert [r[:3] for r in out] == [r[:3] for r in rows]
    stats = open("s.stats.txt").read().splitlines()
    kept = int(stats[1].split("\t")[2])
    assert kept > 0 and sum(int(r[3]) for r in out) == kept
