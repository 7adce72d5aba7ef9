"""The left map.bin byte's bound from the match hints (csrc/pipeline.hip
mate_fast, DESIGN.md section 3 "The left byte's bound"), restated on the host
next to rev_hint_inputs' reading of the hints, for test_left_bound.py (CPU),
test_gpu_left_bound.py (MI355X) and tools/left_bound_share.py (the share of
alignments the rule decides).

m(x): the length of the shortest string starting at text position x that
occurs once in the doubled text.  A string that contains a unique string is
unique, so m(x - 1) <= m(x) + 1.  The left byte of an alignment sits at e, the
forward base after the block's end, and is m of e's mirror in the
reverse-complement contig, zeroed when m >= e's offset ie in its contig.  The
mirror's right neighbour is the mirror of the block's last base (forward
match: the chain hint, bits 33..39, is its m) or the match's first base
(reverse-strand match: the SA-row hint, bits 40..47, is its m).  With that
hint b, the byte is in [1, b + 1] when e lies in the contig and b + 1 < ie;
the post stage uses b for left = byte - 1 when also b <= len and
b <= len - min_excess."""
import bisect

import numpy as np

import rev_hint_inputs as R

# what the rule does with one alignment
SKIP = "skip"                # decided: the byte is not loaded
NO_HINT = "no hint"
EDGE = "contig edge"         # e outside the contig, or b + 1 >= ie
WIDE_PASS = "b > len - min_excess, right byte passes"
WIDE_FAIL = "b > len - min_excess, right byte fails"
CAUSES = (SKIP, NO_HINT, EDGE, WIDE_PASS, WIDE_FAIL)


def hand_reads(oix, L, min_excess=4):
    """Reads for the conditions the shared inputs may not reach: k text bases
    between bytes that occur nowhere ('z').  On every contig: a forward match
    ending on the last base (e outside), a reverse-strand match at o = 0 (the
    contig's reverse complement from its first base), forward matches ending
    a few bases after the contig's start and reverse ones starting a few
    bases before its end (small ie: b + 1 >= ie), and short matches in the
    middle (b within min_excess of len)."""
    T = oix.T[:oix.N]
    out = []

    def put(cut, k):
        if k <= L and cut >= 0:
            r = np.full(L, ord("z"), np.uint8)
            r[(L - k) // 2:(L - k) // 2 + k] = T[cut:cut + k]
            out.append(r)
    for si in range(0, len(oix.startpos), 2):
        s0, s1, sz = int(oix.startpos[si]), int(oix.startpos[si + 1]), int(oix.sizes[si])
        for k in (R.MIN_LEN, 24, 40):
            if k + 8 > sz:
                continue
            put(s0 + sz - k, k)            # forward, ends on the last base: e = S
            put(s1, k)                     # reverse, o = 0: e = S
            put(s0, k)                     # forward from the first base: ie = k
            put(s1 + sz - k, k)            # reverse, ends on the last base: ie = k
            for d in (1, 2, 3):
                put(s0 + d, k)             # ie = k + d
                put(s1 + sz - k - d, k)
                put(s1 + d, k)             # reverse, o = d
        for k in range(R.MIN_LEN, R.MIN_LEN + max(min_excess, 0) + 3):
            if sz > 4 * k:
                put(s0 + sz // 2, k)
                put(s1 + sz // 3, k)
    return np.ascontiguousarray(np.stack(out), np.uint8)


BOUND_K = 25      # 'A' + W below
BOUND_V = 140     # a repeat longer than a hint can say (7 bits; L8 bytes cap at 127)


def bound_genome():
    """Contigs for the two conditions no random text reaches.  b + 1 >= ie
    with e inside the contig: the first contig starts with 'A' + W (W: 24
    random bases) and the third holds 'C' + W, so the match 'A' + W at offset
    0 is unique only as a whole -- its chain hint is its length, 25 = ie; its
    reverse complement matches the end of the reverse-complement contig with
    the SA-row hint 25 = ie.  No hint: a block V of 140 bases stands in the
    first and the third contig; a forward match that ends on V's last base
    and a reverse-strand match that starts on V's mirror are unique through
    their other end only, m = 141.  (Named like edge_genome's contigs: the two
    with hand-placed reads are exempt from mappability_tag's length check.)"""
    rng = np.random.default_rng(31337)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def rnd(n):
        return acgt[rng.integers(0, 4, size=n)]
    W, V = rnd(BOUND_K - 1), rnd(BOUND_V)
    a = np.concatenate([[ord("A")], W, rnd(975), V, rnd(2000)]).astype(np.uint8)   # V at 1000
    b = np.concatenate([rnd(1500), [ord("C")], W, rnd(500), V, rnd(1000)]).astype(np.uint8)
    return [("chrM", a), ("chr1", rnd(4000).astype(np.uint8)), ("chrUn_gl000998", b)]


def bound_genome_reads(oix, L):
    """'A' + W and its reverse complement (the post stage keeps the forward
    one at the read's start and the reverse one at its end: elsewhere the read
    hangs over the contig's edge, pos < 0); at 150 bases the two matches of 150
    bases around V without a hint; and hand_reads on this genome"""
    T = oix.T[:oix.N]
    s0, s1, sz = int(oix.startpos[0]), int(oix.startpos[1]), int(oix.sizes[0])
    out = []
    for cut in (s0, s1 + sz - BOUND_K):
        for lead in (0, (L - BOUND_K) // 2, L - BOUND_K):
            r = np.full(L, ord("z"), np.uint8)
            r[lead:lead + BOUND_K] = T[cut:cut + BOUND_K]
            out.append(r)
    if L > BOUND_V:
        v1 = 1000 + BOUND_V                                # V stands at 1000
        out.append(T[s0 + v1 - L:s0 + v1].copy())          # forward, ends on V's last base
        m = s1 + sz - v1                                   # V's mirror starts here
        out.append(T[m:m + L].copy())                      # reverse strand, starts on it
    return np.concatenate([np.stack(out), hand_reads(oix, L)])


class LeftBound:
    """the rule on the raw match words of one oracle index, with the
    oracle's map.bin to check it against"""

    def __init__(self, oix, mapbin=None):
        self.sp = [int(x) for x in oix.startpos]
        self.sz = [int(x) for x in oix.sizes]
        fwd = [int(x) for x in oix.sizes[0::2]]
        self.base = np.concatenate([[0], np.cumsum(fwd)]).astype(np.int64)
        self.map = oix.mappability() if mapbin is None else mapbin
        self.cause = dict.fromkeys(CAUSES, 0)
        self.branch = {}
        self.skipped = [0, 0]            # per strand

    def _hit(self, name):
        self.branch[name] = self.branch.get(name, 0) + 1

    def _byte(self, at):
        return int(self.map[at]) if at < len(self.map) else 0

    def word(self, w, L, min_excess=4):
        """One raw match word of a mate of L bases: None if the post stage
        erases the alignment (pos < 0), else (cause, b, left byte); checks
        the bound of a skipped alignment against the map."""
        w = int(w)
        ref, q, ln = w & R.POS_MASK, (w >> 48) & 0xFF, w >> 56
        si = bisect.bisect_right(self.sp, ref) - 1
        assert si >= 0
        o, S, rc = ref - self.sp[si], self.sz[si & ~1], si & 1
        pos = S - (o - q) - L if rc else o - q
        if pos < 0:
            self._hit("erased")
            return None
        b = (w >> 40) & 0xFF if rc else (w >> R.POS_BITS) & 0x7F
        ie = S - o if rc else o + ln
        inside = (o >= 1 and o + ln <= S) if rc else o + ln < S
        g = int(self.base[si >> 1]) + ie                 # e among all forward bases
        byte = self._byte(2 + 2 * g)
        if 2 + 2 * g >= len(self.map):
            self._hit("past the map")                    # reads 0, nothing to load
            return None
        if b == 0:
            cause = NO_HINT
            self._hit("no hint")
        elif not inside:
            cause = EDGE
            self._hit("reverse o = 0" if rc and o == 0 else
                      "reverse past the end" if rc else "forward ends on the last base")
        elif b + 1 >= ie:
            cause = EDGE
            self._hit("b + 1 >= ie, reverse" if rc else "b + 1 >= ie, forward")
        elif b > ln or b > ln - min_excess:
            self._hit("b > len" if b > ln else "len - min_excess < b <= len")
            right = self._byte(2 + 2 * (g - ln) + 1)
            right = right if right else 255
            cause = WIDE_PASS if ln - right >= min_excess else WIDE_FAIL
        else:
            cause = SKIP
            self._hit("skip reverse" if rc else "skip forward")
            self.skipped[rc] += 1
            assert 1 <= byte <= b + 1, ("reverse" if rc else "forward", hex(w), si, o, ln, b, byte)
        self.cause[cause] += 1
        return cause, b, byte

    def table(self):
        n = sum(self.cause.values())
        rest = n - self.cause[SKIP]
        rows = ["alignments whose left byte the parent loads: %d" % n,
                "  skip the load: %d (%.1f %%)" % (self.cause[SKIP], 100.0 * self.cause[SKIP] / max(n, 1)),
                "  still load:    %d (%.1f %%), by cause (share of these):" % (rest, 100.0 * rest / max(n, 1))]
        for c in CAUSES[1:]:
            rows.append("    %-44s %7d  %5.1f %%" % (c, self.cause[c], 100.0 * self.cause[c] / max(rest, 1)))
        return "\n".join(rows)


def decide_words(w, sp, sz, L, min_excess=4):
    """the rule over an array of raw match words of mates of L bases (numpy,
    the hg19-sized check).  Returns a dict of arrays over the words: kept (the
    post stage keeps the alignment, pos >= 0), rc, ln, b, g (e's index among
    all forward bases: its left byte is map entry 2 + 2 g, the block's right
    byte entry 2 + 2 (g - ln) + 1), and the rule's classes of the kept words:
    skip, no_hint, edge, wide (b > len - min_excess)."""
    sp, sz = np.asarray(sp, np.int64), np.asarray(sz, np.int64)
    ref = (w & np.uint64(R.POS_MASK)).astype(np.int64)
    q = ((w >> np.uint64(48)) & np.uint64(0xFF)).astype(np.int64)
    ln = (w >> np.uint64(56)).astype(np.int64)
    si = np.searchsorted(sp, ref, side="right") - 1
    assert si.min() >= 0
    o, S, rc = ref - sp[si], sz[si & ~1], (si & 1) == 1
    pos = np.where(rc, S - (o - q) - L, o - q)
    kept = pos >= 0
    b = np.where(rc, (w >> np.uint64(40)) & np.uint64(0xFF),
                 (w >> np.uint64(R.POS_BITS)) & np.uint64(0x7F)).astype(np.int64)
    ie = np.where(rc, S - o, o + ln)
    inside = np.where(rc, (o >= 1) & (o + ln <= S), o + ln < S)
    base = np.concatenate([[0], np.cumsum(sz[0::2])])[si >> 1]
    no_hint = kept & (b == 0)
    edge = kept & ~no_hint & (~inside | (b + 1 >= ie))
    wide = kept & ~no_hint & ~edge & ((b > ln) | (b > ln - min_excess))
    skip = kept & ~no_hint & ~edge & ~wide
    return dict(kept=kept, rc=rc, ln=ln, b=b, g=base + ie, skip=skip, no_hint=no_hint,
                edge=edge, wide=wide)
