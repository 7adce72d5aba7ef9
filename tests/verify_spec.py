"""The predicates of smash_index_verify (include/smash_gpu.h, DESIGN.md
section 1) stated in numpy, for the tests: the same fields as
smash_verify_report, computed from host arrays.

    perm   rank i bad iff sa(i) >= N or isa(sa(i)) != i
    order  rank 0 bad iff sa(0) != N-1 or T[N-1] != '$'; rank i >= 1 with
           x = sa(i-1), y = sa(i) good iff both < N and (T[x] < T[y] or
           (T[x] == T[y] and x+1 < N and y+1 < N and isa(x+1) < isa(y+1)))
    lcp    l(i) = L8[i], or for 255 the overflow table's value for rank i
           (lower bound by bisection; absent = bad).  Rank 0 good iff l == 0.
           Rank i >= 1 needs x, y < N, l < N-x, l < N-y, T[x+l] != T[y+l];
           reducible (x, y > 0 and T[x-1] == T[y-1]): good iff j = isa(y-1)
           has 1 <= j < N, sa(j-1) == x-1 and l(j) == l+1; irreducible: good
           iff T[x..x+l) == T[y..y+l)
    ovf    entry e bad iff idx >= N or L8[idx] != 255 or val < 255 or
           (e > 0 and idx[e-1] >= idx[e])
    layout bad contig-table entries + rc-half mismatches +
           |count('`') - (n_seq-1)| + |count('$') - 1|
    map    differing bytes past the 2-byte header

An irreducible rank is "compared in full": with T[x+l] != T[y+l] already
required, that equals l == lcp(x, y), so where (x, y) is the true index's
adjacent pair the true LCP decides and no bytes are compared; other pairs
(a corrupted SA) are compared as numpy slices.  The bytes a comparison
reads: l when equal, else up to and including the first difference.

*_first: smallest bad rank (perm, order, lcp), table entry (ovf), map.bin
byte offset (map), text position (layout: a bad table entry counts at its
end position startpos + size when that is inside the text, else N-1; an rc
mismatch at its position in the rc half; a separator count alone at N-1).
Values are taken as < 2^63 (int64 arithmetic).
"""
import numpy as np

LAYOUT, SA, LCP, MAP, ALL = 1, 2, 4, 8, 15
NONE = 2 ** 64 - 1
FIELDS = ("layout_bad", "layout_first", "perm_bad", "perm_first", "order_bad", "order_first",
          "lcp_bad", "lcp_first", "ovf_bad", "ovf_first", "map_bad", "map_first", "n_lcp255",
          "lcp_irreducible", "lcp_bytes_compared", "lcp_longest", "checked", "ok")

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"acgtrymkbdhvACGTRYMKBDHV", b"tgcayrkmvhdbTGCAYRKMVHDB"):
    _COMP[_a] = _b


def _first(mask, values=None):
    idx = np.nonzero(mask)[0]
    if not len(idx):
        return NONE
    return int(idx[0]) if values is None else int(np.min(values[idx]))


def _lower_bound(keys, table):
    """per key the bisection of the verifier (first entry not < key), which
    is defined on an unsorted table too"""
    lo = np.zeros(len(keys), np.int64)
    hi = np.full(len(keys), len(table), np.int64)
    while True:
        m = lo < hi
        if not m.any():
            return lo
        mid = lo + ((hi - lo) >> 1)
        less = table[np.where(m, mid, 0)] < keys
        lo = np.where(m & less, mid + 1, lo)
        hi = np.where(m & ~less, mid, hi)


def _claim(L8, oidx, oval, ranks):
    """(present, l) of the claimed exact LCP at ranks (all < N)"""
    l8 = L8[ranks].astype(np.int64)
    have = l8 < 255
    l = l8.copy()
    big = np.nonzero(~have)[0]
    if len(big) and len(oidx):
        lo = _lower_bound(ranks[big], oidx)
        inr = lo < len(oidx)
        loc = np.where(inr, lo, 0)
        hit = inr & (oidx[loc] == ranks[big])
        have[big] = hit
        l[big] = np.where(hit, oval[loc], 0)
    return have, l


def crafted_contigs(seed=7):
    """[(name, uint8 bases)] for text_from_contigs: a 5 000-base segment in
    two contigs behind prefixes of 3 and 10 bases (one long irreducible LCP,
    unequal alignments), "ac" x 400 (a chain of step 2) and a 1 000-base
    N-run (one long reducible chain)."""
    rng = np.random.default_rng(seed)

    def rnd(n):
        return np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, n)]
    seg = rnd(5000)
    return [("chr1", np.concatenate([rnd(3), seg, rnd(200)])),
            ("chr2", np.concatenate([rnd(10), seg, rnd(211)])),
            ("chr3", np.frombuffer(b"ac" * 400, np.uint8)),
            ("chr4", np.concatenate([rnd(300), np.full(1000, ord("n"), np.uint8), rnd(333)]))]


def split_lcp(lcp):
    """(L8, ovf[n, 2]) of an exact LCP array (vec_uchar, longSA.h:18-61)"""
    lcp = np.asarray(lcp).astype(np.int64)
    big = np.nonzero(lcp >= 255)[0]
    return (np.minimum(lcp, 255).astype(np.uint8),
            np.stack([big, lcp[big]], 1).astype(np.uint64).reshape(-1, 2))


def reducible_chain(T, sa, isa, head):
    """the ranks whose LCP value hangs on rank `head`'s through reducible
    links: head's pair (x, y), then the rank of (x + 1, y + 1) while that pair
    is adjacent and T[x] == T[y], and so on"""
    N = len(sa)
    out, i = [int(head)], int(head)
    while True:
        x, y = int(sa[i - 1]), int(sa[i])
        if x + 1 >= N or y + 1 >= N or T[x] != T[y]:
            return out
        i2 = int(isa[y + 1])
        if i2 < 1 or int(sa[i2 - 1]) != x + 1:
            return out
        out.append(i2)
        i = i2


def verify_spec(T, sa, isa, L8, ovf, startpos, sizes, rcref=True, flags=ALL, mapbin=None,
                true_map=None, true_sa=None, true_lcp=None, true_T=None):
    """T: text (N bytes, or longer: N = len(sa)); sa / isa: the elements
    (masked); ovf: [n, 2] {idx, val}; mapbin / true_map: map.bin images
    (header included) or None (an index without a map); true_sa / true_lcp:
    the true index of true_T (default: of T; they decide the irreducible ranks
    only while T is that text).  Returns the report's fields, plus
    "_lcp_bad_ranks"."""
    N = len(sa)
    T = np.asarray(T, np.uint8)[:N]
    if true_T is not None and not np.array_equal(T, np.asarray(true_T, np.uint8)[:N]):
        true_sa = true_lcp = None
    sa = np.asarray(sa).astype(np.int64)
    isa = np.asarray(isa).astype(np.int64)
    L8 = np.asarray(L8, np.uint8)
    ovf = np.asarray(ovf).reshape(-1, 2).astype(np.int64)
    oidx, oval = ovf[:, 0], ovf[:, 1]
    r = {k: 0 for k in FIELDS}
    for k in FIELDS:
        if k.endswith("_first"):
            r[k] = NONE
    r["_lcp_bad_ranks"] = np.zeros(0, np.int64)
    ranks = np.arange(N, dtype=np.int64)
    y = sa
    yok = (y >= 0) & (y < N)
    yc = np.where(yok, y, 0)
    x = np.concatenate([[N], sa[:-1]])          # rank 0 has no x
    xok = (x >= 0) & (x < N)
    xok[0] = False
    xc = np.where(xok, x, 0)
    both = xok & yok

    if flags & SA:
        perm = ~yok | (isa[yc] != ranks)
        r["perm_bad"], r["perm_first"] = int(perm.sum()), _first(perm)
        nxt = both & (xc + 1 < N) & (yc + 1 < N)
        ix1 = isa[np.where(nxt, xc + 1, 0)]
        iy1 = isa[np.where(nxt, yc + 1, 0)]
        tx, ty = T[xc], T[yc]
        good = both & ((tx < ty) | ((tx == ty) & nxt & (ix1 < iy1)))
        good[0] = sa[0] == N - 1 and T[N - 1] == ord("$")
        r["order_bad"], r["order_first"] = int((~good).sum()), _first(~good)
        r["checked"] |= SA

    if flags & LCP:
        r["n_lcp255"] = int((L8 == 255).sum())
        have, l = _claim(L8, oidx, oval, ranks)
        pre = both & have & (l >= 0) & (l < N - xc) & (l < N - yc)
        lc = np.where(pre, l, 0)
        pre &= T[np.where(pre, xc + lc, 0)] != T[np.where(pre, yc + lc, 0)]
        left = pre & (xc > 0) & (yc > 0)
        red = left & (T[np.where(left, xc - 1, 0)] == T[np.where(left, yc - 1, 0)])
        j = isa[np.where(red, yc - 1, 0)]
        jok = red & (j >= 1) & (j < N)
        jc = np.where(jok, j, 1)
        hj, lj = _claim(L8, oidx, oval, jc)
        good = jok & (sa[jc - 1] == xc - 1) & hj & (lj == lc + 1)
        irr = pre & ~red
        nbytes = np.zeros(N, np.int64)
        for i in np.nonzero(irr)[0]:
            li, xi, yi = int(l[i]), int(x[i]), int(y[i])
            if (true_sa is not None and true_lcp is not None and int(true_sa[i - 1]) == xi
                    and int(true_sa[i]) == yi):
                tl = int(true_lcp[i])
                eq, n = li <= tl, (li if li <= tl else tl + 1)
            else:
                d = np.nonzero(T[xi:xi + li] != T[yi:yi + li])[0]
                eq, n = len(d) == 0, (li if len(d) == 0 else int(d[0]) + 1)
            good[i] = eq
            nbytes[i] = n
        good[0] = bool(have[0]) and int(l[0]) == 0
        bad = ~good
        r["lcp_bad"], r["lcp_first"] = int(bad.sum()), _first(bad)
        r["_lcp_bad_ranks"] = np.nonzero(bad)[0]
        r["lcp_irreducible"] = int(irr.sum())
        r["lcp_bytes_compared"] = int(nbytes.sum())
        r["lcp_longest"] = int(nbytes.max()) if N else 0
        e = np.arange(len(oidx), dtype=np.int64)
        inr = (oidx >= 0) & (oidx < N)
        ob = ~inr | (L8[np.where(inr, oidx, 0)] != 255) | (oval < 255)
        if len(oidx) > 1:
            ob[1:] |= oidx[:-1] >= oidx[1:]
        r["ovf_bad"], r["ovf_first"] = int(ob.sum()), _first(ob, e)
        r["checked"] |= LCP

    if flags & LAYOUT:
        sp = np.asarray(startpos).astype(np.int64)
        sz = np.asarray(sizes).astype(np.int64)
        n_seq = len(sp)
        inr = (sp >= 0) & (sz >= 0) & (sp <= N - 1) & (sz <= N - 1 - sp)
        end = np.where(inr, sp + sz, N - 1)
        tb = ~inr
        for c in range(n_seq):
            if inr[c]:
                if c == n_seq - 1:
                    tb[c] = end[c] != N - 1 or T[end[c]] != ord("$")
                else:
                    tb[c] = T[end[c]] != ord("`") or sp[c + 1] != end[c] + 1
            if rcref and sz[c ^ 1] != sz[c]:
                tb[c] = True
        n_bad = int(tb.sum())
        first = _first(tb, end)
        if rcref:
            for k in range(0, n_seq - 1, 2):
                if not (inr[k] and sp[k + 1] <= N - 1 and sz[k] <= N - 1 - sp[k + 1]
                        and sz[k] == sz[k + 1]):
                    continue
                fwd = T[sp[k]:sp[k] + sz[k]]
                rc = T[sp[k + 1]:sp[k + 1] + sz[k]]
                d = np.nonzero(rc != _COMP[fwd[::-1]])[0]
                n_bad += len(d)
                if len(d):
                    first = min(first, int(sp[k + 1] + d[0]))
        extra = abs(int((T == ord("`")).sum()) - (n_seq - 1)) + abs(int((T == ord("$")).sum()) - 1)
        if extra and first == NONE:
            first = N - 1
        r["layout_bad"], r["layout_first"] = n_bad + extra, first
        r["checked"] |= LAYOUT

    clean = not (r["layout_bad"] or r["perm_bad"] or r["order_bad"] or r["lcp_bad"]
                 or r["ovf_bad"]) and (not r["checked"] & LCP or r["n_lcp255"] == len(oidx))
    proof = LAYOUT | SA | LCP
    if flags & MAP and mapbin is not None and rcref and r["checked"] & proof == proof and clean:
        a, b = np.asarray(mapbin, np.uint8), np.asarray(true_map, np.uint8)
        if len(a) != len(b):
            r["map_bad"], r["map_first"] = 1, 0
        else:
            d = np.nonzero(a[2:] != b[2:])[0]
            r["map_bad"] = len(d)
            r["map_first"] = 2 + int(d[0]) if len(d) else NONE
        r["checked"] |= MAP
        clean = clean and not r["map_bad"]
    r["ok"] = 1 if clean else 0
    return r
