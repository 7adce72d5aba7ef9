"""The bin design's rule in numpy (include/smash_gpu.h, "Bin design"): the
specification smash_bins_apportion / smash_bins_design are tested against.

w(g) = 1 iff 1 <= right(g) <= k.  The binned contigs share nbins by largest
remainder over their unique bases M, one bin each first; a contig with B bins
cuts at the unique bases of rank r[j] = j * M // B."""
import numpy as np


def apportion(M, binned, nbins):
    """bins per contig; ValueError where the library answers SMASH_ERR_ARG"""
    M = [int(x) for x in M]
    idx = [c for c in range(len(M)) if binned[c]]
    if nbins < len(idx):
        raise ValueError("fewer bins than binned contigs")
    B = [0] * len(M)
    for c in idx:
        B[c] = 1                                   # every binned contig gets one bin
    extra, tot = nbins - len(idx), sum(M[c] for c in idx)
    if extra and tot == 0:
        raise ValueError("bins to share and no unique base")
    if extra:                                      # largest remainder, ties by contig order
        q = {c: extra * M[c] // tot for c in idx}
        r = {c: extra * M[c] % tot for c in idx}
        for c in idx:
            B[c] += q[c]
        for c in sorted(idx, key=lambda c: (-r[c], c))[:extra - sum(q.values())]:
            B[c] += 1
    return B


def design_positions(pos_per_contig, sizes, off, nbins, gc=None):
    """The table from each contig's ascending unique positions (None / any for
    an unbinned contig).  gc: None or per contig (is_gc, is_acgt) bool arrays
    over its bases.  Returns (rows, M): rows of (contig, start, stop, abspos,
    n_unique, n_gc, n_acgt)."""
    n = len(sizes)
    binned = [off[c] >= 0 for c in range(n)]
    M = [len(pos_per_contig[c]) if binned[c] else 0 for c in range(n)]
    B = apportion(M, binned, nbins)
    rows = []
    for c in range(n):
        if not binned[c]:
            continue
        S, pos = int(sizes[c]), pos_per_contig[c]
        if B[c] > 1 and B[c] > M[c]:
            raise ValueError("more bins than unique positions")
        r = [j * M[c] // B[c] for j in range(B[c] + 1)]
        start = [0] + [int(pos[r[j]]) for j in range(1, B[c])]
        stop = start[1:] + [S]
        if gc is not None:
            cg = np.concatenate([[0], np.cumsum(gc[c][0], dtype=np.int64)])
            ac = np.concatenate([[0], np.cumsum(gc[c][1], dtype=np.int64)])
        for j in range(B[c]):
            a, b = start[j], stop[j]
            rows.append((c, a, b, int(off[c]) + a, r[j + 1] - r[j],
                         int(cg[b] - cg[a]) if gc is not None else 0,
                         int(ac[b] - ac[a]) if gc is not None else 0))
    return rows, M


def design(map2, sizes, off, k, nbins, text=None, text_start=None):
    """The table from the [left, right] byte pairs of the concatenated forward
    contigs (map.bin without its two header bytes) and, optionally, the text."""
    right = np.asarray(map2, np.uint8)[1::2]
    uniq = (right >= 1) & (right <= k)
    pos, gc, g = [], [], 0
    for c, S in enumerate(int(x) for x in sizes):
        pos.append(np.nonzero(uniq[g:g + S])[0])
        if text is not None:
            t = np.asarray(text, np.uint8)[int(text_start[c]):int(text_start[c]) + S]
            is_gc = (t == ord("c")) | (t == ord("g"))
            gc.append((is_gc, is_gc | (t == ord("a")) | (t == ord("t"))))
        g += S
    return design_positions(pos, sizes, off, nbins, gc if text is not None else None)


def rows_of(rec):
    """a smashgpu.BIN record array as the rows design() returns"""
    return [(int(r["contig"]), int(r["start"]), int(r["stop"]), int(r["abspos"]),
             int(r["n_unique"]), int(r["n_gc"]), int(r["n_acgt"])) for r in rec]
