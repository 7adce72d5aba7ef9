"""smash_index_verify / smash_index_load_verified on the device (csrc/verify.hip)
against tests/verify_spec.py, field for field.

A damaged cache is only ever opened through Index.load(verify=...): never
through the plain load, never searched.  Every corruption keeps every element
in range (< N).  Caches are written with Index.save and edited with numpy.

Marked `gpu` (MI355X).
"""
import os
import shutil

import numpy as np
import pytest
import torch

import oracle as O
import smashgpu as S
import verify_spec as V

pytestmark = pytest.mark.gpu

PROOF = S.VERIFY_LAYOUT | S.VERIFY_SA | S.VERIFY_LCP


@pytest.fixture(scope="module")
def vlib():
    """the entry point first: without it nothing below touches the device"""
    L = S.lib()
    L.smash_index_verify
    L.smash_index_load_verified
    assert torch.cuda.is_available()
    return L


def assert_clean(rep, checked=S.VERIFY_ALL):
    d = rep.as_dict()
    assert d["ok"] == 1 and d["checked"] == checked, d
    for k, v in d.items():
        if k.endswith("_bad"):
            assert v == 0, d
        if k.endswith("_first"):
            assert v == V.NONE, d
    return d


class Cache:
    """the files of <fasta>.bin/ as numpy arrays (rc1 layout), and back"""

    def __init__(self, fasta):
        self.dir = fasta + ".bin/"
        b = open(self.dir + "rc1.ref.bin", "rb").read()
        self.N, n = int.from_bytes(b[8:16], "little"), int.from_bytes(b[16:24], "little")
        self.startpos, self.sizes, off = [], [], 24
        for _ in range(n):
            self.startpos.append(int.from_bytes(b[off:off + 8], "little"))
            self.sizes.append(int.from_bytes(b[off + 8:off + 16], "little"))
            off += 24 + int.from_bytes(b[off + 16:off + 24], "little")
        self.W = 4 if os.path.exists(self.dir + "rc1.i4.index.bin") else 8
        self.base = self.dir + "rc1.i%d.index" % self.W
        dt = np.uint32 if self.W == 4 else np.uint64
        self.T = np.fromfile(self.dir + "rc1.ref.seq.bin", np.uint8)
        self.sa = np.fromfile(self.base + ".sa.bin", dt)
        self.isa = np.fromfile(self.base + ".isa.bin", dt)
        self.L8 = np.fromfile(self.base + ".lcp.vec.bin", np.uint8)
        self.ovf = np.fromfile(self.base + ".lcp.m.bin", np.uint64).reshape(-1, 2)
        if self.W == 4:
            self.ovf[:, 1] &= 0xFFFFFFFF
        self.map = (np.fromfile(self.dir + "map.bin", np.uint8)
                    if os.path.exists(self.dir + "map.bin") else None)

    def write(self):
        self.T.tofile(self.dir + "rc1.ref.seq.bin")
        self.sa.tofile(self.base + ".sa.bin")
        self.isa.tofile(self.base + ".isa.bin")
        self.L8.tofile(self.base + ".lcp.vec.bin")
        np.ascontiguousarray(self.ovf, np.uint64).tofile(self.base + ".lcp.m.bin")
        hdr = np.fromfile(self.base + ".bin", np.uint64)
        hdr[5] = len(self.ovf)
        hdr.tofile(self.base + ".bin")
        if self.map is not None:
            self.map.tofile(self.dir + "map.bin")

    def spec(self, truth, flags=S.VERIFY_ALL):
        return V.verify_spec(self.T, self.sa, self.isa, self.L8, self.ovf, self.startpos,
                             self.sizes, flags=flags, mapbin=self.map,
                             true_map=truth.get("map"), true_sa=truth["sa"],
                             true_lcp=truth["lcp"], true_T=truth["T"])


def rejected(cache, truth, flags=S.VERIFY_ALL):
    """write the edited cache, open it through the verified load (which must
    refuse it with SMASH_ERR_IO) and compare the report with the spec"""
    cache.write()
    want = cache.spec(truth, flags)
    assert want["ok"] == 0
    with pytest.raises(S.SmashError) as e:
        S.Index.load(cache.dir[:-5], verify=flags)
    assert e.value.code == -3 and e.value.report is not None, str(e.value)
    got = e.value.report.as_dict()
    for k in V.FIELDS:
        assert got[k] == want[k], (k, got, {f: want[f] for f in V.FIELDS})
    assert "rejected" in str(e.value)
    return got, want


# ---------------------------------------------------------------------------
# the tiny genome
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(vlib, tiny_fa):
    return S.Index.from_fasta(tiny_fa)


@pytest.fixture(scope="module")
def tiny_cache(tiny, tiny_fa, tmp_path_factory):
    d = tmp_path_factory.mktemp("vtiny")
    fa = str(d / "tiny.fa")
    shutil.copy(tiny_fa, fa)
    tiny.save(fa)
    return fa


def copy_cache(fa, tmp_path):
    dst = str(tmp_path / os.path.basename(fa))
    shutil.copy(fa, dst)
    shutil.copytree(fa + ".bin", dst + ".bin")
    return dst


def test_created_index_is_clean(tiny):
    d = assert_clean(tiny.verify())
    assert d["n_lcp255"] == tiny.info.n_lcp_overflow and d["lcp_irreducible"] > 0
    assert d["lcp_bytes_compared"] <= 2 * tiny.N * np.log2(tiny.N)   # 
    assert_clean(tiny.verify(S.VERIFY_SA), S.VERIFY_SA)
    # the map alone runs only behind the proof: skipped, not an error
    r = tiny.verify(S.VERIFY_MAP)
    assert r.checked == 0 and r.ok == 1


def test_created_index_equals_spec(tiny, tiny_ix):
    SA, ISA = tiny.download_sa_isa()
    i = tiny.info
    L8 = S.download(i.d_lcp8, i.N)
    ovf = S.download(i.d_lcp_ovf, 16 * i.n_lcp_overflow, np.uint64).reshape(-1, 2)
    T = S.download(i.d_text, i.N)
    m = S.download(i.d_map, i.map_bytes)
    want = V.verify_spec(T, SA, ISA, L8, ovf, tiny_ix.startpos, tiny_ix.sizes, mapbin=m,
                         true_map=tiny_ix.mappability(), true_sa=tiny_ix.SA,
                         true_lcp=tiny_ix.LCP)
    got = tiny.verify().as_dict()
    for k in V.FIELDS:
        assert got[k] == want[k], (k, got[k], want[k])


def test_wide_and_packed_words(vlib, tiny_fa, monkeypatch, tmp_path):
    monkeypatch.setenv("SMASH_IDX_BYTES", "8")
    ix = S.Index.from_fasta(tiny_fa)
    assert ix.info.idx_bytes == 8 and ix.info.pos_bits == 33      # packed words
    packed = assert_clean(ix.verify())
    ix.pack(False)
    assert ix.info.pos_bits == 0
    plain = assert_clean(ix.verify())
    for k in ("lcp_irreducible", "lcp_bytes_compared", "lcp_longest", "n_lcp255"):
        assert packed[k] == plain[k]
    # rc1.i8 files, loaded as 8-byte elements through the gate
    fa = str(tmp_path / "wide.fa")
    shutil.copy(tiny_fa, fa)
    ix.save(fa, fasta_size=1 << 32)
    assert os.path.exists(fa + ".bin/rc1.i8.index.sa.bin")
    got = S.Index.load(fa, verify=S.VERIFY_ALL)
    assert got.info.idx_bytes == 8
    assert_clean(got.verify_report)


def test_loaded_cache_is_clean(tiny_cache, tiny):
    ix = S.Index.load(tiny_cache, verify=S.VERIFY_ALL)
    d = assert_clean(ix.verify_report)           # (map.bin came from the file: rechecked)
    assert d["lcp_bytes_compared"] == tiny.verify().lcp_bytes_compared
    assert_clean(ix.verify())                    # and the live index, derived arrays built
    with pytest.raises(S.SmashError) as e:       # the proof is mandatory in the gate
        S.Index.load(tiny_cache, verify=S.VERIFY_MAP)
    assert e.value.code == -1


def test_forward_only_layout(vlib, tiny_fa):
    ix = S.Index.from_fasta(tiny_fa, rcref=False)
    assert_clean(ix.verify(), PROOF)             # MAP skipped: such an index has no map


def test_smallest_text(vlib):
    ix = S.Index.from_contigs([("c", np.frombuffer(b"a", np.uint8))])
    assert ix.N == 4 and ix.info.n_lcp_overflow == 0
    d = assert_clean(ix.verify())
    assert d["n_lcp255"] == 0


def test_map_byte(tiny_cache, tiny_ix, tmp_path):
    fa = copy_cache(tiny_cache, tmp_path)
    c = Cache(fa)
    truth = dict(T=tiny_ix.T, sa=tiny_ix.SA, lcp=tiny_ix.LCP, map=tiny_ix.mappability())
    c.map[1001] ^= 1
    got, _ = rejected(c, truth)
    assert got["map_bad"] == 1 and got["map_first"] == 1001 and got["checked"] == S.VERIFY_ALL
    ix = S.Index.load(fa, verify=PROOF)          # without the recheck the map is taken
    assert_clean(ix.verify_report, PROOF)


def test_cli_verify(tiny_cache, tiny_ix, tmp_path, capsys):
    import json

    import smash_cli
    smash_cli.main(["--ref", tiny_cache, "verify"])
    out = capsys.readouterr().out
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["ok"] == 1 and rep["checked"] == S.VERIFY_ALL
    fa = copy_cache(tiny_cache, tmp_path)
    c = Cache(fa)
    i = int(np.nonzero(tiny_ix.LCP >= 255)[0][0])
    swap_ranks(c, i, True)
    c.write()
    with pytest.raises(SystemExit) as e:
        smash_cli.main(["--ref", fa, "verify", "--no-map"])
    assert e.value.code == 1
    cap = capsys.readouterr()
    assert json.loads(cap.out.strip().splitlines()[-1])["order_bad"] >= 1
    assert "order" in cap.err and "rank %d" % i in cap.err


# ---------------------------------------------------------------------------
# the crafted contigs: long irreducible LCP at unequal alignments, a chain of
# step 2, an N-run
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(vlib, tmp_path_factory):
    contigs = V.crafted_contigs()
    oix = O.Index(*O.text_from_contigs(contigs))
    ix = S.Index.from_contigs(contigs)
    d = tmp_path_factory.mktemp("vcraft")
    fa = str(d / "crafted.fa")
    with open(fa, "w") as f:
        for name, s in contigs:
            f.write(">%s\n%s\n" % (name, s.tobytes().decode()))
    ix.save(fa)
    truth = dict(T=oix.T, sa=oix.SA.astype(np.int64), isa=oix.ISA.astype(np.int64),
                 lcp=oix.LCP.astype(np.int64), map=oix.mappability())
    return ix, fa, truth


def test_crafted_is_clean(crafted):
    ix, fa, truth = crafted
    d = assert_clean(ix.verify())
    assert d["lcp_longest"] >= 5000 and d["lcp_irreducible"] > 0
    c = Cache(fa)
    want = c.spec(truth)
    for k in V.FIELDS:
        assert d[k] == want[k], (k, d[k], want[k])
    assert_clean(S.Index.load(fa, verify=S.VERIFY_ALL).verify_report)


def swap_ranks(c, i, fix_isa):
    c.sa[[i - 1, i]] = c.sa[[i, i - 1]]
    if fix_isa:
        c.isa[c.sa[i - 1]] = i - 1
        c.isa[c.sa[i]] = i


def test_swapped_ranks_in_a_long_repeat(crafted, tmp_path):
    """SA and ISA agree, the LCP array is untouched: only the suffix order,
    checked without the LCP, can see it"""
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    i = int(np.nonzero(truth["lcp"] >= 255)[0][0])
    swap_ranks(c, i, True)
    got, _ = rejected(c, truth)
    assert got["perm_bad"] == 0 and got["order_bad"] >= 1 and got["order_first"] == i


def test_swapped_ranks_without_isa(crafted, tmp_path):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    swap_ranks(c, int(np.nonzero(truth["lcp"] >= 255)[0][0]), False)
    got, _ = rejected(c, truth)
    assert got["perm_bad"] == 2


@pytest.mark.parametrize("d", [1, -1])
def test_lcp_byte_off_by_one(crafted, tmp_path, d):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    i = int(np.nonzero((truth["lcp"] >= 1) & (truth["lcp"] <= 100))[0][5])
    c.L8[i] = int(c.L8[i]) + d
    got, want = rejected(c, truth)
    assert got["lcp_bad"] >= 1 and i in want["_lcp_bad_ranks"]
    assert got["perm_bad"] == got["order_bad"] == 0


def test_overflow_value_off_by_one(crafted, tmp_path):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    c.ovf[3, 1] += 1
    got, want = rejected(c, truth)
    assert got["lcp_bad"] >= 1 and int(c.ovf[3, 0]) in want["_lcp_bad_ranks"]
    assert got["ovf_bad"] == 0


def test_shifted_chain_is_flagged_at_its_head(crafted, tmp_path):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    T, sa, lcp = c.T, truth["sa"], truth["lcp"]
    n = ord("n")
    head = next(int(i) for i in np.nonzero(lcp >= 600)[0]
                if T[sa[i]] == n and T[sa[i - 1]] == n
                and (sa[i] == 0 or sa[i - 1] == 0 or T[sa[i] - 1] != T[sa[i - 1] - 1]))
    chain = V.reducible_chain(T, sa, truth["isa"], head)
    assert len(chain) >= 600
    shifted = lcp.copy()
    shifted[chain] += 1
    c.L8, c.ovf = V.split_lcp(shifted)
    got, want = rejected(c, truth)
    assert head in want["_lcp_bad_ranks"] and got["lcp_bad"] >= 1
    assert got["ovf_bad"] == 0 and got["n_lcp255"] == len(c.ovf)


def test_overflow_entry_removed(crafted, tmp_path):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    gone = int(c.ovf[2, 0])
    c.ovf = np.delete(c.ovf, 2, axis=0)          # (write() puts the count into the header)
    got, want = rejected(c, truth)
    assert got["n_lcp255"] == len(c.ovf) + 1 and gone in want["_lcp_bad_ranks"]


def test_overflow_entries_exchanged(crafted, tmp_path):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    c.ovf[[4, 5]] = c.ovf[[5, 4]]
    got, _ = rejected(c, truth)
    assert got["ovf_bad"] >= 1


def test_base_changed_in_an_rc_half(crafted, tmp_path):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    p = c.startpos[1] + 17
    c.T[p] = ord("a") if c.T[p] != ord("a") else ord("c")
    got, _ = rejected(c, truth)
    assert got["layout_bad"] >= 1 and got["layout_first"] == p


def test_separator_overwritten(crafted, tmp_path):
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    sep = c.startpos[2] - 1
    assert c.T[sep] == ord("`")
    c.T[sep] = ord("a")
    got, _ = rejected(c, truth)
    assert got["layout_bad"] >= 1 and got["layout_first"] == sep


@pytest.mark.parametrize("k", range(20))
def test_single_element_corruptions(crafted, tmp_path, k):
    """one in-range element of SA, ISA or L8 replaced (seeded)"""
    _, fa, truth = crafted
    c = Cache(copy_cache(fa, tmp_path))
    rng = np.random.default_rng(1000 + k)
    arr, top = [(c.sa, c.N), (c.isa, c.N), (c.L8, 256)][k % 3]
    at = int(rng.integers(0, c.N))
    new = int(rng.integers(0, top - 1))
    arr[at] = new if new < int(arr[at]) else new + 1     # (never the old value)
    got, _ = rejected(c, truth)
    assert got["ok"] == 0
