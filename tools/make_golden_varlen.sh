#!/bin/bash
# tools/make_golden_varlen.sh -- mixed-read-length fixtures from the UPSTREAM
# reference (dev container only: needs /root/reference and oracle/_ref built
# by `make -C oracle ref`).  Everything written to tests/golden/ is DATA.
#
# The committed s150 pairs are trimmed by tools/varlen_reads.py (each mate
# keeps a prefix whose length is a function of its bases), then the unmodified
# reference chain runs as smash_mapping.sh:19-29 writes it (samtools is
# absent: name order is restated as in tools/make_golden_smashmem.sh, pysam
# is tools/pysam_shim):
#   1. fastqs_to_sam r1 r2 1
#   2. mummer -rcref -qthreads 2 -nomap -samin -samout
#   3. mappability_tag
#   4. name order (read 1 before read 2, stable otherwise)
#   5. smashMEM.py 0 0 10000 4
#   6. awk/perl extraction of the major chromosomes' positions
#   7. varbin.py (crashes at its median line under python3, varbin.py:113,
#      after writing every bin row; its exit code is ignored)
# Outputs: v150_r{1,2}.fq.gz, v150_mapout_tagged_full.txt.gz,
# v150_smashmem.txt.gz, v150_positions.txt, v150_varbin.txt,
# v150_varbin_stats_partial.txt.
# The script fails unless the reference's own output shows at least one dupe
# pair, at least 100 reverse-strand hits and mates at every SPECIAL length,
# and mappability_tag ran through without a throw.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REF=${REF:-/root/reference}
R=$ROOT/oracle/_ref
OUT=$ROOT/tests/golden
W=$(mktemp -d /tmp/goldenv.XXXXXX)
trap 'rm -rf "$W"' EXIT
make -s -C "$ROOT/oracle" ref
cd "$W"
gzip -dc "$OUT/tiny.fa.gz" > tiny.fa
"$R/mummer" -rcref tiny.fa dummy > /dev/null 2>&1 || true
"$R/mummer" -rcref -mappability tiny.fa tiny.fa.bin/map.bin > /dev/null 2>&1
cp "$OUT/tiny_sam_header.txt" tiny.fa.bin/sam_header.txt     # index_setup.sh:31
cp "$OUT/tiny_chrom_sizes.txt" tiny.fa.bin/chrom_sizes.txt   # index_setup.sh:28

python3 "$ROOT/tools/varlen_reads.py" "$OUT/s150_r1.fq.gz" "$OUT/s150_r2.fq.gz" v150_r1.fq v150_r2.fq
python3 - v150_r1.fq v150_r2.fq <<PY
import sys
sys.path.insert(0, "$ROOT/tools")
from varlen_reads import SPECIAL
have = set()
for p in sys.argv[1:]:
    lines = open(p).read().split("\n")
    have |= {len(lines[i]) for i in range(1, len(lines) - 1, 4)}
miss = sorted(set(SPECIAL) - have)
if miss:
    sys.exit("no mate of length %s" % miss)
PY

"$R/fastqs_to_sam" v150_r1.fq v150_r2.fq 1 > v150.sam
rm -rf mapout
"$R/mummer" -rcref -qthreads 2 -nomap -samin -samout tiny.fa v150.sam 2> /dev/null
cat mapout/*.txt | grep '^@' | LC_ALL=C sort -u > hdr.txt
cat mapout/*.txt | grep -v '^@' | perl -pe 's/^(\S+?)\/\S+\/\d+/\1/' > body.sam
# (a throw ends mappability_tag with a non-zero status: set -e stops here)
"$R/mappability_tag" tiny.fa <(cat hdr.txt body.sam) > tagged.sam 2> tag.err
if grep -qi 'terminate\|what()\|error' tag.err; then cat tag.err >&2; exit 1; fi
grep -v '^@' tagged.sam | LC_ALL=C sort > v150_mapout_tagged_full.txt

python3 - hdr.txt v150_mapout_tagged_full.txt > v150_namesort.sam <<'PY'
import sys
head = [l for l in open(sys.argv[1]) if l.startswith("@")]
body = open(sys.argv[2]).read().splitlines()
# samtools sort -n: name (fixed-width r%09d: plain order), read 1 first
body.sort(key=lambda l: (l.split("\t", 1)[0], 0 if int(l.split("\t")[1]) & 64 else 1))
sys.stdout.write("".join(head) + "\n".join(body) + "\n")
PY
PYTHONPATH=$ROOT/tools/pysam_shim python3 "$REF/smashMEM.py" v150_namesort.sam 0 0 10000 4 > v150_smashmem.txt
cat v150_smashmem.txt | awk '{print $4, $5}' | perl -ne 'print if /^chr(\d+|[XY]) \d+$/' > v150_positions.txt
python3 "$REF/varbin.py" v150_positions.txt "$OUT/tiny_bins.txt" v150_varbin.txt \
    v150_stats.txt tiny.fa.bin/chrom_sizes.txt > /dev/null 2>&1 || true

dupes=$(tail -n 1 v150_smashmem.txt | awk '{print $1}')
rev=$(awk -F'\t' 'NR > 1 && NF > 6 && $6 == 1' v150_smashmem.txt | wc -l)
fwd=$(awk -F'\t' 'NR > 1 && NF > 6 && $6 == 0' v150_smashmem.txt | wc -l)
echo "reference: $(tail -n 1 v150_smashmem.txt); $rev reverse-strand hits, $fwd forward;" \
     "$(wc -l < v150_positions.txt) positions"
[ "$dupes" -ge 1 ] || { echo "no dupe pair in the smashMEM summary" >&2; exit 1; }
[ "$rev" -ge 100 ] || { echo "fewer than 100 reverse-strand hits" >&2; exit 1; }
[ -s v150_varbin.txt ] || { echo "varbin.py wrote no bin rows" >&2; exit 1; }

gzip -9 -n -c v150_r1.fq > "$OUT/v150_r1.fq.gz"
gzip -9 -n -c v150_r2.fq > "$OUT/v150_r2.fq.gz"
gzip -9 -n -c v150_mapout_tagged_full.txt > "$OUT/v150_mapout_tagged_full.txt.gz"
gzip -9 -n -c v150_smashmem.txt > "$OUT/v150_smashmem.txt.gz"
cp v150_positions.txt "$OUT/v150_positions.txt"
cp v150_varbin.txt "$OUT/v150_varbin.txt"
cp v150_stats.txt "$OUT/v150_varbin_stats_partial.txt"
echo "mixed-length golden written to $OUT"
