"""Degenerate genomes: the texts on which the device index builder
(csrc/sa_build.hip: two-character buckets, packed-character keys, prefix
doubling over the tied suffixes only), the accelerators (aux_build.hip), the
post stage's contig directory (pipeline.hip sp_cell) and the mappability scan
take branches that random ACGT with a handful of long contigs never reaches.
One definition for test_degenerate_inputs.py (CPU: the oracle against a naive
suffix sort and the reference's goldens, and the cases are not vacuous) and
test_gpu_degenerate.py (MI355X).  Everything is made from code and seeded.

Every genome is [(name, uint8 bases)] for text_from_contigs, except the
forward-only layouts (`sigma2`, the odd sizes of the sweep), which are texts.
"""
import numpy as np

import rev_hint_inputs as R

ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"acgtACGT", b"tgcaTGCA"):
    _COMP[_a] = _b


def rc(s):
    return _COMP[np.asarray(s, np.uint8)[::-1]]


def _b(s):
    return np.frombuffer(s, np.uint8).copy()


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)]


# the pure-repeat families: every suffix tied with another for hundreds of
# bases, so n_a (the tied suffixes of a doubling round) stays near N
REPEAT_FAMILIES = ("unary", "period2", "selfrc", "period3x2", "twins", "rctwins", "nruns",
                   "tailrun")
# no read can have a maximal *almost-unique* match inside them
PURE_REPEATS = ("unary", "period2", "selfrc", "period3x2")
NAMES = REPEAT_FAMILIES + ("specks", "one", "two", "mosaic")


def speck_name(k):
    return "chrUn_gl000%03d" % k


def _mosaic(rng):
    """unique flanks around an a-run of 300 (> a 256-position directory cell),
    (ac)^200, an N-run, a duplicated and a reverse-duplicated 1 500-base
    segment, a self-rc contig, runs at both ends of a contig, and 126 speck
    contigs of 1..60 bases: 120 with small_chr names, 6 with major names"""
    seg = _rnd(rng, 1500)
    x = _rnd(rng, 600)
    out = [("chr1", np.concatenate([
        _rnd(rng, 2500), np.full(300, ord("A"), np.uint8), _rnd(rng, 2500), _b(b"AC" * 200),
        _rnd(rng, 2500), np.full(400, ord("N"), np.uint8), _rnd(rng, 2000), seg,
        _rnd(rng, 1500)]))]
    flank = out[0][1]
    # speck lengths: a cluster of very short ones (many contig starts in one
    # 256-position cell), then 1..60
    lens = [int(v) for v in rng.integers(1, 9, 40)] + [int(v) for v in rng.integers(1, 61, 80)]
    specks = []
    for k, n in enumerate(lens):
        if k % 10 == 9 and n >= 20:       # a copy of a flank window: not unique
            p = int(rng.integers(0, 2400))
            specks.append((speck_name(k), flank[p:p + n].copy()))
        else:
            specks.append((speck_name(k), _rnd(rng, n)))
    out += specks[:50]
    out.append(("chr2", np.concatenate([
        np.full(280, ord("T"), np.uint8), _rnd(rng, 3000), seg, _rnd(rng, 2000), rc(seg),
        _rnd(rng, 1500), np.full(270, ord("G"), np.uint8)])))
    # major-named specks: shorter than K + 2, than min_len, than a read
    for name, n in (("chr4", 5), ("chr5", 19), ("chr6", 45)):
        out.append((name, _rnd(rng, n)))
    out += specks[50:90]
    out.append(("chr3", np.concatenate([x, rc(x)])))          # equal to its reverse complement
    for name, n in (("chr7", 1), ("chr8", 30), ("chr9", 60)):
        out.append((name, _rnd(rng, n)))
    out += specks[90:]
    out.append(("chrX", _rnd(rng, 1800)))
    return out


def genome(name):
    rng = np.random.default_rng(sum(name.encode()) + 20260)
    if name == "unary":
        return [("chr1", np.full(3000, ord("A"), np.uint8))]
    if name == "period2":
        return [("chr1", _b(b"AC" * 2000))]
    if name == "selfrc":
        return [("chr1", _b(b"AT" * 1500))]
    if name == "period3x2":
        return [("chr1", _b(b"ACG" * 1000)), ("chr2", _b(b"CGA" * 1000))]
    if name == "twins":
        s = _rnd(rng, 4000)
        return [("chr1", s), ("chr2", s.copy())]
    if name == "rctwins":
        s = _rnd(rng, 4000)
        return [("chr1", s), ("chr2", rc(s))]
    if name == "nruns":
        n = ord("N")
        return [("chr1", np.concatenate([_rnd(rng, 700), np.full(600, n, np.uint8), _rnd(rng, 500),
                                         np.full(300, n, np.uint8)])),
                ("chr2", np.full(400, n, np.uint8)),
                ("chr3", np.concatenate([np.full(260, n, np.uint8), _rnd(rng, 900)]))]
    if name == "specks":
        out = [(speck_name(k), _rnd(rng, int(rng.integers(1, 41)))) for k in range(300)]
        return out[:150] + [("chr1", _rnd(rng, 5000))] + out[150:]
    if name == "one":
        return [("c", _b(b"A"))]
    if name == "two":
        return [("c1", _b(b"AC")), ("c2", _b(b"G"))]
    if name == "tailrun":
        # the last contig begins with 300 t: its rc half ends the text, ...aaa$
        return [("chr1", _rnd(rng, 2000)),
                ("chr2", np.concatenate([np.full(300, ord("T"), np.uint8), _rnd(rng, 700)]))]
    if name == "mosaic":
        return _mosaic(rng)
    raise KeyError(name)


def forward_text(contigs):
    """(T, startpos, sizes, names) of the forward-only layout (rcref=False):
    contigs lowercased, '`' between them, '$' last"""
    lower = np.arange(256, dtype=np.uint8)
    lower[ord("A"):ord("Z") + 1] += 32
    parts, sp, sz, names, pos = [], [], [], [], 0
    for k, (name, s) in enumerate(contigs):
        sp.append(pos), sz.append(len(s)), names.append(name)
        parts += [lower[s], _b(b"`" if k + 1 < len(contigs) else b"$")]
        pos += len(s) + 1
    return np.concatenate(parts), np.array(sp, np.uint64), np.array(sz, np.uint64), names


def sigma2():
    """forward-only, one contig of only a: two symbols with '$', the 2-bit
    32-characters-per-key form of the bucket sort"""
    return forward_text([("chr1", np.full(2500, ord("A"), np.uint8))])


# the text lengths of the sweep: every N from 4 to 80 (every residue mod 16,
# the partial 16-position block of k_plcp; K = 4 up to N = 1023), and N on
# either side of one and two blocks of 256 x 64 positions of the bucket pass
SWEEP_N = tuple(range(4, 81)) + (16383, 16384, 16385, 32768, 32769)


def sweep_text(N):
    """(T, startpos, sizes, names, rcref) of one random contig whose text has
    exactly N bytes: with its reverse complement N = 2 n + 2 is even, so an
    odd N is a forward-only text of N - 1 bases"""
    rng = np.random.default_rng(N)
    if N % 2 == 0:
        import oracle as O
        return O.text_from_contigs([("chr1", _rnd(rng, (N - 2) // 2))]) + (True,)
    return forward_text([("chr1", _rnd(rng, N - 1))]) + (False,)


def chrom_sizes(contigs):
    """the chrom_sizes dict of a genome (name -> offset, the contigs without
    '_' in order: synth.write_index_side_files)"""
    out, n = {}, 0
    for name, s in contigs:
        if "_" not in name:
            out[name] = n
            n += len(s)
    return out


def bin_starts(contigs, seed=99):
    """absolute bin starts in the manner of synth.make_bins: every binned
    contig of 8 bases or more cut at up to 7 random places, shorter ones one
    bin each"""
    rng = np.random.default_rng(seed)
    starts, off = [], 0
    for name, s in contigs:
        if "_" in name:
            continue
        n = len(s)
        cuts = np.sort(rng.choice(np.arange(1, n), size=min(7, n - 1), replace=False)) if n > 1 else []
        starts += [off] + [off + int(c) for c in cuts]
        off += n
    return np.array(starts, np.int64)


# ---------------------------------------------------------------------------
# reads
# ---------------------------------------------------------------------------
def text_rc(r):
    """reverse complement of a text window (bytes other than acgt as they are)"""
    return _COMP[r[::-1]]


def junction_centres(oix):
    """{kind: [text positions]}: the separator before every fourth
    reverse-complement half (contig|separator|its own reverse complement) and
    before every second contig after the first (the reverse complement of one
    contig|separator|the next contig: speck|separator|speck, the junction of
    two chromosomes), both ends of every run of 200 or more equal bytes
    (unique|run, unique|N), the middle of each (a window with no unique string
    in it) and the two ends of the text"""
    T = oix.T[:oix.N]
    N = int(oix.N)
    sp = [int(p) for p in oix.startpos]
    out = {"separator": [p - 1 for p in sp[1::4] + sp[2::4]]}
    edge = np.nonzero(T[1:] != T[:-1])[0] + 1
    b = np.concatenate([[0], edge, [N]])
    runs = [(int(a), int(z)) for a, z in zip(b[:-1], b[1:]) if z - a >= 200]
    out["run"] = [p for a, z in runs if T[a] != ord("n") for p in (a, z)]
    out["n"] = [p for a, z in runs if T[a] == ord("n") for p in (a, z)]
    out["run_middle"] = [(a + z) // 2 for a, z in runs]
    out["text_end"] = [0, N]
    return out


def junction_reads(oix, L, seed=1):
    """[n, L]: a text window centred on every junction_centres position
    (clipped to the text; the last one ends with '$'), the reverse complement
    of each, and each with 1..3 substituted bases"""
    T = oix.T[:oix.N]
    N = int(oix.N)
    rng = np.random.default_rng(seed * 1000 + L)
    cs = sorted({min(max(p - L // 2, 0), N - L) for v in junction_centres(oix).values() for p in v})
    plain = np.stack([T[c:c + L] for c in cs])
    mut = plain.copy()
    low = np.frombuffer(b"acgt", np.uint8)
    for r in mut:
        for _k in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, L))
            r[at] = low[(int(np.searchsorted(low, r[at])) + int(rng.integers(1, 4))) % 4]
    return np.concatenate([plain, np.stack([text_rc(r) for r in plain]), mut])


def speck_pairs(contigs, n_pairs, L, seed, max_speck=60):
    """[2 * n_pairs, L] SMASH pairs (mates interleaved, lowercased) whose
    mates are made of segments that overlap a speck contig or a contig end: a
    whole speck of 20 bases or more, or the first / last 20..L/2 bases of a
    longer contig, on either strand, joined and filled up with random bases;
    the second mate shares a source with the first.  Every tenth pair repeats
    an earlier one."""
    rng = np.random.default_rng(seed)
    small = [s for _, s in contigs if 20 <= len(s) <= max_speck]
    big = [s for _, s in contigs if len(s) > max_speck]
    assert small and big

    def piece(src):
        kind, k = src
        if kind == 0:
            s = small[k]
        else:
            n = int(rng.integers(20, max(21, L // 2)))
            s = big[k][:n] if rng.random() < 0.5 else big[k][-n:]
        return rc(s) if rng.random() < 0.5 else s

    def source():
        return (0, int(rng.integers(0, len(small)))) if rng.random() < 0.6 else \
            (1, int(rng.integers(0, len(big))))

    def mate(srcs):
        parts = [piece(s) for s in srcs]
        r = np.concatenate(parts + [_rnd(rng, L)])[:L]
        return r

    out = np.empty((2 * n_pairs, L), np.uint8)
    for q in range(n_pairs):
        a, b = source(), source()
        out[2 * q] = mate([a, b])
        out[2 * q + 1] = mate([b, source()] if rng.random() < 0.5 else [source(), a])
        if q % 10 == 9:
            src = int(rng.integers(0, q))
            out[2 * q:2 * q + 2] = out[2 * src:2 * src + 2]
    return R.lower(out)


def alignments(oix, read, matches):
    """per match (ref, q, len) of a read: (rc, left_out, overhang) -- on the
    reverse strand; the alignment's left map.bin byte (the forward base after
    the block's end, mappability_tag.cpp:98) lies in another contig or past
    the map; the read placed by the match starts before its contig (a negative
    position) or ends past it"""
    sp = np.asarray(oix.startpos, np.int64)
    out = []
    for ref, q, ln in matches:
        si = int(np.searchsorted(sp, ref, side="right")) - 1
        o, S, L = ref - int(sp[si]), int(oix.sizes[si]), len(read)
        if si & 1:
            pos = S - (o - q) - L
            left_out = o == 0 or o + ln > S
        else:
            pos = o - q
            left_out = o + ln >= S
        out.append((bool(si & 1), left_out, pos < 0 or pos + L > S))
    return out


def pair_errors(oix, reads, mapbin, min_len=20):
    """per pair the number of hits mappability_tag throws on (a block shorter
    than one of its map bytes on a contig that is not small_chr): such a pair
    makes the whole run an error, in the reference, the oracle and the device
    alike"""
    import oracle as O
    offs = np.cumsum([0] + [int(x) for x in oix.sizes[0::2]][:-1]).astype(np.uint32)
    small = [1 if ("_gl000" in c or "chrM" in c) else 0 for c in oix.contigs]
    errs = []
    for q in range(reads.shape[0] // 2):
        e = 0
        for m in (0, 1):
            P = reads[2 * q + m].tobytes()
            h, _ = oix.resolve(P, oix.search(P, min_len=min_len))
            e += sum(1 for x in h if O.tag(x, offs, mapbin, small[x.tid]))
        errs.append(e)
    return errs


PIPE_LENGTHS = (40, 100)


def pipeline_reads(contigs, oix, mapbin, L, min_len=20):
    """(reads the oracle tags without an error, the pairs left out): 400
    SMASH pairs of geometry_inputs.smash_reads and 150 speck_pairs, of L bases"""
    import geometry_inputs as G
    reads = np.concatenate([G.smash_reads(contigs, 400, L, seed=L),
                            speck_pairs(contigs, 150, L, seed=L)])
    errs = pair_errors(oix, reads, mapbin, min_len)
    ok = [q for q, e in enumerate(errs) if e == 0]
    rows = np.array([2 * q + m for q in ok for m in (0, 1)])
    bad = np.array([2 * q + m for q, e in enumerate(errs) if e for m in (0, 1)])
    return np.ascontiguousarray(reads[rows]), np.ascontiguousarray(reads[bad])


# the read sets whose MAM / MUM / MEM triples the reference itself wrote into
# tests/golden/degen_* (tools/make_golden_degenerate.sh): junction_reads of
# (genome, read length)
GOLDEN_READS = (("mosaic", 40), ("mosaic", 100), ("specks", 40), ("nruns", 100), ("twins", 100),
                ("rctwins", 100), ("tailrun", 100))
