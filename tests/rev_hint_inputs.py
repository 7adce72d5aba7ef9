"""Inputs and host-side checks shared by test_sm_emu_hints.py (CPU) and
test_gpu_rev_hints.py (MI355X): the reads both run, and the reading of a match
word's map hints (csrc/mam_sm.hpp pk_map_hint / pk_chain_hint, csrc/pipeline.hip
mate_fast)."""
import bisect

import numpy as np

import oracle as O
import synth

MIN_LEN = 20
POS_BITS = 33
POS_MASK = (1 << POS_BITS) - 1
LOWER = np.arange(256, dtype=np.uint8)
LOWER[65:91] += 32


def lower(reads):
    """N -> z, lowercase: what the search is given (oracle.lower_read)"""
    reads = np.where(reads == ord("N"), ord("Z"), reads).astype(np.uint8)
    return np.ascontiguousarray(LOWER[reads])


def mid_index():
    g = synth.make_genome("mid")
    T, sp, sz, names = O.text_from_contigs(g)
    return g, (T, sp, sz, names)


EDGE_K = 25


def edge_genome():
    """Contigs built so that the post stage's zeroing rule decides a
    reverse-strand hint: the first ends in W + 'a' (W: 24 random bases) and
    the second holds W followed by 'c'.  The reverse-complement contig of the
    first then starts with the 25 bases 't' + rc(W): unique, while its suffix
    rc(W) is not -- a match there has the chain hint m = 25 = its length at
    offset 0, and the map.bin right byte of its first forward base (m + i =
    the contig size) is zeroed.  A zeroed byte reads as 255, longer than any
    match, which mappability_tag accepts only on the contigs it exempts
    (chrM, *_gl000*): the two are named so, and a third gives the run a
    chromosome with bins."""
    rng = np.random.default_rng(2718)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    W = acgt[rng.integers(0, 4, size=EDGE_K - 1)]
    a = np.concatenate([acgt[rng.integers(0, 4, size=3000)], W, [ord("A")]]).astype(np.uint8)
    b = np.concatenate([acgt[rng.integers(0, 4, size=1500)], W, [ord("C")],
                        acgt[rng.integers(0, 4, size=1500)]]).astype(np.uint8)
    c = acgt[rng.integers(0, 4, size=4000)].astype(np.uint8)
    return [("chrM", a), ("chr1", c), ("chrUn_gl000999", b)]


def edge_genome_reads(oix, L):
    """the first EDGE_K bases of the first contig's reverse complement between
    'z's (the zeroed hint), and hand_reads on this genome"""
    T = oix.T[:oix.N]
    s0 = int(oix.startpos[1])
    out = []
    for lead in (0, 40, L - EDGE_K):
        r = np.full(L, ord("z"), np.uint8)
        r[lead:lead + EDGE_K] = T[s0:s0 + EDGE_K]
        out.append(r)
    return np.concatenate([np.stack(out), hand_reads(oix, L)])


def synth_reads(g, n_pairs, L, seed):
    r1, r2 = synth.make_reads(g, n_pairs, L, seed=seed)
    reads = np.empty((2 * n_pairs, L), np.uint8)
    reads[0::2], reads[1::2] = r1, r2
    return lower(reads)


def hand_reads(oix, L):
    """Reads whose reverse-strand matches touch their contig's first base and
    its last base: k text bases from the start / up to the end of every
    reverse-complement contig (the forward contig's last / first k bases,
    mirrored) between bytes that occur nowhere ('z'), for short and long k --
    a short match is where the hint can be as long as the match, the only
    case in which the post stage's zeroing rule decides.  And reads with an
    N (z after lowering) inside a reverse-strand match."""
    T = oix.T[:oix.N]
    out = []
    for si in range(1, len(oix.startpos), 2):
        s0, sz = int(oix.startpos[si]), int(oix.sizes[si])
        for k in (MIN_LEN, MIN_LEN + 1, 24, 31, 47, L - 30, L):
            if k > sz or k > L:
                continue
            for cut in (s0, s0 + sz - k):
                for lead in sorted({0, (L - k) // 2, L - k}):
                    r = np.full(L, ord("z"), np.uint8)
                    r[lead:lead + k] = T[cut:cut + k]
                    out.append(r)
        if sz >= L:
            for cut in (s0, s0 + sz - L, s0 + (sz - L) // 2):
                for at in (0, 33, L // 2, L - 1):
                    r = T[cut:cut + L].copy()
                    r[at] = ord("z")           # a read's N
                    out.append(r)
    return np.ascontiguousarray(np.stack(out), np.uint8)


def edge_reads_150(oix):
    """test_gpu_sm_loads.py's edge reads (150 bases)"""
    from test_gpu_sm_loads import _edge_reads
    return _edge_reads(oix)


class HintCheck:
    """the map.bin right bytes of an oracle index (mappability_range over all
    forward bases) and the post stage's reading of a match word's hints"""

    def __init__(self, oix):
        self.sp = [int(x) for x in oix.startpos]
        self.sz = [int(x) for x in oix.sizes]
        fwd = [int(x) for x in oix.sizes[0::2]]
        self.base = np.concatenate([[0], np.cumsum(fwd)]).astype(np.int64)   # contig -> first base
        total = int(self.base[-1])
        m, _ = oix.mappability_range(0, total)
        self.right = m[1::2]
        self.n_rev = self.n_rev_hint = self.n_rev_zeroed = self.n_fwd_hint = self.n_fwd = 0

    def word(self, w):
        """checks one raw match word; returns its (ref, q, len)"""
        w = int(w)
        ref, q, ln = w & POS_MASK, (w >> 48) & 0xFF, w >> 56
        si = bisect.bisect_right(self.sp, ref) - 1
        assert si >= 0
        o = ref - self.sp[si]
        S = self.sz[si & ~1]
        if si & 1:
            if o + ln > S:                       # runs past its contig: never hinted
                return ref, q, ln
            self.n_rev += 1
            h = (w >> POS_BITS) & 0x7F
            if h:
                self.n_rev_hint += 1
                i = S - o - ln                   # the block's first forward base
                zero = h >= o + ln               # m + i >= S
                self.n_rev_zeroed += zero
                want = int(self.right[self.base[si >> 1] + i])
                assert (0 if zero else h) == want, ("reverse", hex(w), si, o, ln, h, want)
        else:
            self.n_fwd += 1
            h = (w >> 40) & 0xFF
            if h and o < S:
                self.n_fwd_hint += 1
                want = int(self.right[self.base[si >> 1] + o])
                assert (0 if o + h >= S else h) == want, ("forward", hex(w), si, o, ln, h, want)
        return ref, q, ln
