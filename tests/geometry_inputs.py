"""Read lengths and min_len values off the benchmark's geometry (100 / 150
bases, min_len 20), one definition for test_geometry_inputs.py (CPU: the
cases are not vacuous, from the oracle alone) and test_gpu_geometry.py
(MI355X: the device search and pipeline at every one of them).

What moves with the two numbers (csrc/mam_sm.hpp make_geom and the (F) window
filter, csrc/mam.hip launch_plain, csrc/mem.hip launch_mem, csrc/pipeline.hip):
the LDS row w_row = max(8, ((L + 11) / 4 rounded up to 4 words)) steps every
16 bases; the bad mask gains a word per 32 bases and a second record chunk
above 128; the filter branches on D = min_len - B (B = K + 2, the index's
B-mer width); slots = L - min_len + 1 sizes every row of the pipeline and
caps k_post_fast's lists; the 7-bit chain hint and the 127-capped map hint
saturate on matches longer than 127."""
import numpy as np

import rev_hint_inputs as R
import synth

LENGTHS = (
    20,         # w_row at its floor of 8 words; one slot at min_len 20
    24,         # the last length of the floor (w_row 8 | 12 at 24 | 25); 5 slots at min_len 20
    32, 33,     # the bad mask's first | second 32-base word
    36,         # w_row 12, two mask words; min_len 2 runs here
    40, 41,     # w_row 12 | 16
    50,         # w_row 16, a length no step falls on
    64, 65,     # the bad mask's second | third word
    76,         # w_row 24 (73..88), a common trimmed length
    125,        # w_row 36 (121..136): the first chunk's last mask word, partly used
    128, 129,   # c_bad 1 | 2: the second record chunk of the bad mask
    136, 137,   # w_row 36 | 40
    152, 153,   # w_row 40 | 44, just past the benchmark's 150
    200,        # w_row 52, 7 mask words
    250,        # w_row 68 (249..255), matches longer than the hints' 127
    255,        # the ABI's longest: 8 mask words, query offsets up to 254
)
PIPE_LENGTHS = (20, 24, 36, 76, 129, 250, 255)

# many matches per mate (k_post_fast<8> -> <16> -> k_post) and keys of more
# than 16 words, on the tiny genome
LONG_CASE = dict(L=255, n_pairs=400, seed=255, err=0.0, seg=(14, 17), min_len=13)
# matches far longer than 127 (the caps of pk_chain_hint / pk_map_hint), on
# the mid genome
HINT_CASE = dict(L=250, n_pairs=1500, seed=250, seg=(20, 250))

BAD = b"acgtnz`$"


def w_row(L):
    """make_geom's LDS row words, restated (csrc/mam_sm.hpp:166)"""
    return max(8, ((L + 11) // 4 + 3) // 4 * 4)


def min_lens(B, L):
    """min_len values around the filter's branches for an index of B-mer
    width B: D = -1 (no filter, min_len < B), 0, 2 (production's), 10 | 11
    (the second entry per probe fits | does not), 13 | 14 (D + 3 = 16 | 17:
    the filter's last | none); the benchmark's 20; and at 36 bases the
    smallest the ABI takes."""
    out = {B + d for d in (-1, 0, 2, 10, 11, 13, 14)} | {20}
    if L == 36:
        out.add(2)
    return sorted(m for m in out if 2 <= m <= L)


def pipe_min_lens(B, L):
    return [m for m in (B + 2, 20, B + 14) if m <= L]


def _clean_window(T, c, L):
    acgt = np.frombuffer(b"acgt", np.uint8)
    while not np.isin(T[c:c + L], acgt).all():
        c += L
    return T[c:c + L].copy()


def edge_reads(oix, L, n, seed):
    """n reads of L bases (the recipe of test_gpu_sm_loads._edge_reads and
    test_sm_emu._edge_reads at any L; oix.accel() done): text windows with
    0..4 substituted bytes, then the hand-made ones -- the ends of the text,
    of the first forward contig and of its reverse complement, a separator
    inside, homopolymers and (ac)*, one bad byte at the read's end, its start
    and on either side of the first mask word's end, and per min_len of
    min_lens a window whose last min_len bases are its only clean ones."""
    T = oix.T[:oix.N]
    N = int(oix.N)
    sp = [int(x) for x in oix.startpos]
    sz = [int(x) for x in oix.sizes]
    rng = np.random.default_rng(seed)
    hand = [T[c:c + L].copy() for c in (
        0,                       # the first L bases of the text
        sp[0] + sz[0] - L,       # the last L of the first forward contig
        sp[1],                   # the first L of its reverse complement
        sp[1] + sz[1] - L,       # the last L of that
        sp[1] - 1 - L // 2,      # across the separator between the two
        N - L,                   # the text's end with its terminator
        N - 1 - L)]              # the last L bases of the text
    for ch in b"azn":
        hand.append(np.full(L, ch, np.uint8))
    hand.append(np.frombuffer((b"ac" * L)[:L], np.uint8).copy())
    mid = _clean_window(T, sp[0] + sz[0] // 2, L)
    for at in (L - 1, 0, min(31, L - 1), min(32, L - 1)):
        r = mid.copy()
        r[at] = ord("z")
        hand.append(r)
    for k, ml in enumerate(min_lens(oix.acc.B, L)):
        r = _clean_window(T, sp[0] + sz[0] // 3 + 997 * k, L)
        r[:L - ml] = ord("z")
        hand.append(r)
    assert len(hand) < n
    out = np.empty((n, L), np.uint8)
    bad = np.frombuffer(BAD, np.uint8)
    for i in range(n - len(hand)):
        p = int(rng.integers(0, N - L - 1))
        out[i] = T[p:p + L]
        for _k in range(int(rng.integers(0, 5))):
            out[i, int(rng.integers(0, L))] = bad[int(rng.integers(0, len(bad)))]
    out[n - len(hand):] = np.stack(hand)
    return out


def smash_reads(genome, n_pairs, L, seed, **kw):
    """[2 * n_pairs, L]: synth.make_reads' SMASH pairs, mates interleaved,
    N -> z and lowercased (what the search is given)"""
    r1, r2 = synth.make_reads(genome, n_pairs, L, seed=seed, **kw)
    reads = np.empty((2 * n_pairs, L), np.uint8)
    reads[0::2], reads[1::2] = r1, r2
    return R.lower(reads)


def case_reads(genome, case):
    kw = {k: v for k, v in case.items() if k not in ("L", "n_pairs", "seed", "min_len")}
    return smash_reads(genome, case["n_pairs"], case["L"], case["seed"], **kw)


VAR_WIDTHS = (40, 76, 255)


def var_len_mates(width):
    """mates of mixed lengths for a variable-length pipeline of read_len =
    width: the pairs of the v150 fixture (the trimmed s150 pairs) whose two
    mates have at most width bases, and at 255 also 50 pairs of 255 bases on
    the tiny genome -- byte strings, interleaved"""
    import varlen_util as V
    mates = V.mixed_mates("v150")
    out = []
    for q in range(len(mates) // 2):
        if max(len(mates[2 * q]), len(mates[2 * q + 1])) <= width:
            out += mates[2 * q:2 * q + 2]
    if width == 255:
        out += [r.tobytes() for r in smash_reads(synth.make_genome("tiny"), 50, 255, seed=255)]
    return out


class Chain:
    """search -> resolve -> tag -> smash_pair per pair of one oracle index at
    one min_len / min_excess: every mate's matches, every pair's key (or None)
    and the host's first-wins keep flags"""

    def __init__(self, oix, reads, min_len=20, min_excess=4, mapbin=None):
        import oracle as O
        mapbin = oix.mappability() if mapbin is None else mapbin
        offs = np.cumsum([0] + [int(x) for x in oix.sizes[0::2]][:-1]).astype(np.uint32)
        small = [1 if ("_gl000" in c or "chrM" in c) else 0 for c in oix.contigs]
        self.matches, self.keys, self.keep = [], [], []
        self.tag_errors = 0
        seen = set()
        for q in range(reads.shape[0] // 2):
            hs = []
            for m in (0, 1):
                P = reads[2 * q + m].tobytes()
                mt = oix.search(P, min_len=min_len)
                self.matches.append(mt)
                h, _ = oix.resolve(P, mt)
                for x in h:
                    self.tag_errors += 1 if O.tag(x, offs, mapbin, small[x.tid]) else 0
                hs.append(h)
            key = O.smash_pair(hs[0], hs[1], min_excess=min_excess)
            self.keys.append(key)
            self.keep.append(key is not None and tuple(key) not in seen)
            if key is not None:
                seen.add(tuple(key))
