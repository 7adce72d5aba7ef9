#!/usr/bin/env python3
"""tools/varlen_reads.py -- trim a FASTQ pair to mixed read lengths.

    varlen_reads.py in_r1.fq[.gz] in_r2.fq[.gz] out_r1.fq out_r2.fq [cap]

Each mate keeps its first vlen(seq) bases and qualities.  The length depends
only on the mate's bases, so exact duplicate pairs stay duplicates:

    h = zlib.crc32(seq), c = h % 10
    c == 0:    SPECIAL[(h >> 8) % 16]      (edges of the kernels' chunking)
    c == 1:    1 + (h >> 8) % 19           (shorter than min_len: no hits)
    otherwise: 20 + (h >> 8) % 131

`cap` (default: none) bounds the length from above (reads shorter than 150).
tests/golden/v150_* is this rule over s150 (tools/make_golden_varlen.sh).
"""
import gzip
import sys
import zlib

SPECIAL = [150, 150, 1, 19, 20, 21, 31, 32, 33, 63, 64, 65, 127, 128, 129, 149]


def vlen(seq, cap=None):
    """seq: the mate's bases as in the FASTQ file (bytes)."""
    h = zlib.crc32(seq)
    c = h % 10
    if c == 0:
        n = SPECIAL[(h >> 8) % 16]
    elif c == 1:
        n = 1 + (h >> 8) % 19
    else:
        n = 20 + (h >> 8) % 131
    n = min(n, len(seq))
    return min(n, cap) if cap else n


def _open(path):
    return gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")


def trim_file(src, dst, cap=None):
    lens = []
    with _open(src) as f, open(dst, "wb") as g:
        lines = f.read().split(b"\n")
        for i in range(0, len(lines) - 3, 4):
            name, seq, plus, qual = lines[i:i + 4]
            n = vlen(seq, cap)
            lens.append(n)
            g.write(b"\n".join((name, seq[:n], plus, qual[:n])) + b"\n")
    return lens


def main(argv):
    if len(argv) not in (5, 6):
        sys.exit(__doc__)
    cap = int(argv[5]) if len(argv) == 6 else None
    a = trim_file(argv[1], argv[3], cap)
    b = trim_file(argv[2], argv[4], cap)
    sys.stderr.write("varlen_reads: %d + %d mates, lengths %d..%d\n"
                     % (len(a), len(b), min(a + b), max(a + b)))


if __name__ == "__main__":
    main(sys.argv)
