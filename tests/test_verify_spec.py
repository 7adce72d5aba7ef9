"""verify_spec.py (the numpy statement of smash_index_verify's predicates)
against the C oracle's index: all-zero on a true index, and the stated field
non-zero for each kind of damage the device tests write into a cache."""
import numpy as np
import pytest

import oracle as O
import verify_spec as V


def arrays(ix):
    N = ix.N
    return dict(T=ix.T[:N].copy(), sa=ix.SA.astype(np.int64), isa=ix.ISA.astype(np.int64),
                L8=ix.L8.copy(), ovf=ix.ovf.copy(), startpos=ix.startpos.copy(),
                sizes=ix.sizes.copy())


def spec(a, truth, **kw):
    return V.verify_spec(a["T"], a["sa"], a["isa"], a["L8"], a["ovf"], a["startpos"], a["sizes"],
                         true_sa=truth["sa"], true_lcp=truth["lcp"], **kw)


def assert_clean(r, checked):
    assert r["ok"] == 1 and r["checked"] == checked
    for k in V.FIELDS:
        if k.endswith("_bad"):
            assert r[k] == 0, k
        if k.endswith("_first"):
            assert r[k] == V.NONE, k


@pytest.fixture(scope="module")
def crafted():
    ix = O.Index(*O.text_from_contigs(V.crafted_contigs()))
    a = arrays(ix)
    return a, dict(sa=a["sa"].copy(), lcp=ix.LCP.astype(np.int64))


def test_tiny_index_is_clean(tiny_ix):
    a = arrays(tiny_ix)
    truth = dict(sa=a["sa"], lcp=tiny_ix.LCP.astype(np.int64))
    m = tiny_ix.mappability()
    r = spec(a, truth, mapbin=m, true_map=m)
    assert_clean(r, V.ALL)
    assert r["n_lcp255"] == len(tiny_ix.ovf) > 0
    assert r["lcp_irreducible"] > 0
    # Kaerkkaeinen-Manzini-Puglisi: the irreducible LCP values sum to <= 2 N log2 N
    assert r["lcp_bytes_compared"] <= 2 * tiny_ix.N * np.log2(tiny_ix.N)
    # without the true index every irreducible rank is compared as bytes: same figures
    few = dict(a, sa=a["sa"], isa=a["isa"])
    r2 = V.verify_spec(few["T"], few["sa"], few["isa"], few["L8"], few["ovf"], few["startpos"],
                       few["sizes"], flags=V.LCP)
    for k in ("lcp_bad", "lcp_irreducible", "lcp_bytes_compared", "lcp_longest"):
        assert r2[k] == r[k], k


def test_crafted_index_is_clean(crafted):
    a, truth = crafted
    r = spec(a, truth)
    assert_clean(r, V.LAYOUT | V.SA | V.LCP)      # (no map given: MAP skipped)
    assert r["lcp_longest"] >= 5000 and r["lcp_irreducible"] > 0
    r = spec(a, truth, flags=V.SA)
    assert_clean(r, V.SA)


def big_rank(truth):
    return int(np.nonzero(truth["lcp"] >= 255)[0][0])


def test_swapped_ranks_with_isa(crafted):
    a, truth = crafted
    a = {k: v.copy() for k, v in a.items()}
    i = big_rank(truth)
    a["sa"][[i - 1, i]] = a["sa"][[i, i - 1]]
    a["isa"][a["sa"][i - 1]] = i - 1
    a["isa"][a["sa"][i]] = i
    r = spec(a, truth)
    assert r["perm_bad"] == 0 and r["order_bad"] >= 1 and r["order_first"] == i and r["ok"] == 0


def test_swapped_ranks_without_isa(crafted):
    a, truth = crafted
    a = {k: v.copy() for k, v in a.items()}
    i = big_rank(truth)
    a["sa"][[i - 1, i]] = a["sa"][[i, i - 1]]
    r = spec(a, truth)
    assert r["perm_bad"] == 2 and r["perm_first"] == i - 1 and r["ok"] == 0


@pytest.mark.parametrize("d", [1, -1])
def test_lcp_byte_off_by_one(crafted, d):
    a, truth = crafted
    a = {k: v.copy() for k, v in a.items()}
    i = int(np.nonzero((truth["lcp"] >= 1) & (truth["lcp"] <= 100))[0][5])
    a["L8"][i] = int(a["L8"][i]) + d
    r = spec(a, truth)
    assert r["lcp_bad"] >= 1 and i in r["_lcp_bad_ranks"] and r["perm_bad"] == r["order_bad"] == 0


def test_overflow_value_off_by_one(crafted):
    a, truth = crafted
    a = {k: v.copy() for k, v in a.items()}
    a["ovf"][3, 1] += 1
    r = spec(a, truth)
    assert r["lcp_bad"] >= 1 and int(a["ovf"][3, 0]) in r["_lcp_bad_ranks"] and r["ovf_bad"] == 0


def test_shifted_chain_is_flagged_at_its_head(crafted):
    a, truth = crafted
    a = {k: v.copy() for k, v in a.items()}
    T, sa, lcp = a["T"], truth["sa"], truth["lcp"]
    n = ord("n")
    heads = [i for i in np.nonzero(lcp >= 600)[0]
             if T[sa[i]] == n and T[sa[i - 1]] == n
             and (sa[i] == 0 or sa[i - 1] == 0 or T[sa[i] - 1] != T[sa[i - 1] - 1])]
    head = int(heads[0])
    chain = V.reducible_chain(T, sa, a["isa"], head)
    assert len(chain) >= 600
    shifted = lcp.copy()
    shifted[chain] += 1
    a["L8"], a["ovf"] = V.split_lcp(shifted)
    r = spec(a, truth)
    # every link of the chain still holds (both ends moved); the head, compared
    # in full, does not.  (Other members may fail T[x+l] != T[y+l] as well.)
    assert head in r["_lcp_bad_ranks"] and set(r["_lcp_bad_ranks"]) <= set(chain)
    assert r["ovf_bad"] == 0 and r["n_lcp255"] == len(a["ovf"])


def test_overflow_entry_removed(crafted):
    a, truth = crafted
    a = {k: v.copy() for k, v in a.items()}
    gone = int(a["ovf"][2, 0])
    a["ovf"] = np.delete(a["ovf"], 2, axis=0)
    r = spec(a, truth)
    assert r["n_lcp255"] == len(a["ovf"]) + 1 and gone in r["_lcp_bad_ranks"] and r["ok"] == 0


def test_overflow_entries_exchanged(crafted):
    a, truth = crafted
    a = {k: v.copy() for k, v in a.items()}
    a["ovf"][[4, 5]] = a["ovf"][[5, 4]]
    r = spec(a, truth)
    assert r["ovf_bad"] >= 1 and r["ovf_first"] == 5 and r["ok"] == 0


def test_rc_half_and_separator(crafted):
    a, truth = crafted
    b = {k: v.copy() for k, v in a.items()}
    p = int(b["startpos"][1]) + 17
    b["T"][p] = ord("a") if b["T"][p] != ord("a") else ord("c")
    r = spec(b, truth, flags=V.LAYOUT)
    assert r["layout_bad"] == 1 and r["layout_first"] == p
    b = {k: v.copy() for k, v in a.items()}
    sep = int(b["startpos"][2]) - 1
    assert b["T"][sep] == ord("`")
    b["T"][sep] = ord("a")
    r = spec(b, truth, flags=V.LAYOUT)
    assert r["layout_bad"] == 2 and r["layout_first"] == sep   # the entry and the count


def test_map_byte(tiny_ix):
    a = arrays(tiny_ix)
    truth = dict(sa=a["sa"], lcp=tiny_ix.LCP.astype(np.int64))
    m = tiny_ix.mappability()
    bad = m.copy()
    bad[1001] ^= 1
    r = spec(a, truth, mapbin=bad, true_map=m)
    assert r["map_bad"] == 1 and r["map_first"] == 1001 and r["ok"] == 0
    r = spec(a, truth, mapbin=bad, true_map=m, flags=V.LAYOUT | V.SA | V.LCP)
    assert r["ok"] == 1 and r["map_bad"] == 0
