#!/bin/bash
# tools/make_golden_degenerate.sh -- the degenerate genomes of
# tests/degenerate_inputs.py through the UPSTREAM reference (needs the
# reference's binaries under oracle/_ref, built by `make -C oracle ref`).
# Everything written to tests/golden/ is DATA: hashes, match triples and
# tagged SAM fields.  The genomes and reads are regenerated from code by the
# tests; none is stored.
#
# Per genome (every name of degenerate_inputs.NAMES):
#   mummer -rcref ref dummy; mummer -rcref -mappability   (index_setup.sh:19,22)
#   -> degen_<name>_index.sha256: the rc1.* files and map.bin[2:], in the
#      format of tiny_index.sha256
# Per read set (degenerate_inputs.GOLDEN_READS: genome, read length):
#   oracle/_ref/mam_harness MAM | MUM | MEM on degenerate_inputs.junction_reads
#   -> degen_<name>_<L>_{MAM,MUM,MEM}.txt.gz; the MEM file holds only the reads
#      with at most MEM_MAX matches (each line carries its read's index)
# The mosaic's pipeline pairs (degenerate_inputs.pipeline_reads at 40 and 100
# bases) through the chain of smash_mapping.sh:19-23 as tools/make_golden.sh
# runs it: fastqs_to_sam r1 r2 1; mummer -rcref -nomap -samin -samout;
# mappability_tag (with the whole header: the mosaic has 130 contigs)
#   -> degen_mosaic_pairs_<L>_mapout_tagged.txt.gz: fields 1-9 and the tags of
#      the pairs the tagger takes (it must run through without a throw)
#   -> degen_mosaic_pairs_<L>_tag_errors.txt: per pair it throws on, one run
#      of the chain on that pair alone: pair index, exit status, what it threw
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
R=$ROOT/oracle/_ref
OUT=$ROOT/tests/golden
MEM_MAX=300
W=$(mktemp -d /tmp/goldend.XXXXXX)
trap 'rm -rf "$W"' EXIT
make -s -C "$ROOT/oracle" ref oracle
cd "$W"

python3 - <<EOF
import sys
for p in ("tools", "tests", "oracle"):
    sys.path.insert(0, "$ROOT/" + p)
import numpy as np
import oracle as O
import synth
import degenerate_inputs as D
with open("names.txt", "w") as f:
    f.write("\n".join(D.NAMES) + "\n")
for name in D.NAMES:
    synth.write_fasta(name + ".fa", D.genome(name))
with open("readsets.txt", "w") as f:
    for name, L in D.GOLDEN_READS:
        oix = O.Index(*O.text_from_contigs(D.genome(name)))
        reads = D.junction_reads(oix, L)
        with open("%s_%d_reads.txt" % (name, L), "wb") as g:
            for r in reads:
                g.write(r.tobytes() + b"\n")
        f.write("%s %d\n" % (name, L))
g = D.genome("mosaic")
synth.write_index_side_files("mosaic.fa.bin", g)
oix = O.Index(*O.text_from_contigs(g))
mapbin = oix.mappability()
up = np.arange(256, dtype=np.uint8)
up[ord("a"):ord("z") + 1] -= 32
up[ord("z")] = ord("N")                      # (fastqs_to_sam's replaceN makes it Z again)
for L in D.PIPE_LENGTHS:
    ok, bad = D.pipeline_reads(g, oix, mapbin, L)
    synth.write_fastq("pairs_%d_r1.fq" % L, up[ok[0::2]], 1)
    synth.write_fastq("pairs_%d_r2.fq" % L, up[ok[1::2]], 2)
    for q in range(bad.shape[0] // 2):
        synth.write_fastq("bad_%d_%d_r1.fq" % (L, q), up[bad[2 * q:2 * q + 1]], 1)
        synth.write_fastq("bad_%d_%d_r2.fq" % (L, q), up[bad[2 * q + 1:2 * q + 2]], 2)
    open("bad_%d.n" % L, "w").write("%d\n" % (bad.shape[0] // 2))
EOF

while read -r g; do
  "$R/mummer" -rcref $g.fa dummy >/dev/null 2>&1 || true
  "$R/mummer" -rcref -mappability $g.fa $g.fa.bin/map.bin >/dev/null 2>&1
  {
    for f in rc1.ref.seq.bin rc1.ref.bin rc1.i4.index.bin rc1.i4.index.sa.bin \
             rc1.i4.index.isa.bin rc1.i4.index.lcp.vec.bin; do
      echo "$f $(sha256sum $g.fa.bin/$f | cut -d' ' -f1) $(stat -c %s $g.fa.bin/$f)"
    done
    # item_t{size_t idx; uint32 val} has 4 uninitialised padding bytes
    # (longSA.h:19-28): the (idx, val) content with the padding masked
    python3 -c "
import hashlib, numpy as np
m = np.fromfile('$g.fa.bin/rc1.i4.index.lcp.m.bin', np.uint64).reshape(-1, 2).copy()
m[:, 1] &= 0xFFFFFFFF
print('rc1.i4.index.lcp.m.bin:masked', hashlib.sha256(m.tobytes()).hexdigest(), m.size * 8)"
    echo "map.bin[2:] $(tail -c +3 $g.fa.bin/map.bin | sha256sum | cut -d' ' -f1) $(stat -c %s $g.fa.bin/map.bin)"
  } > "$OUT/degen_${g}_index.sha256"
done < names.txt

while read -r g L; do
  for mode in MAM MUM MEM; do
    "$R/mam_harness" $g.fa ${g}_${L}_reads.txt $mode > ${g}_${L}_${mode}.txt
  done
  awk -v m=$MEM_MAX '$2 <= m' ${g}_${L}_MEM.txt > mem_few.txt
  [ -s mem_few.txt ] || { echo "$g $L: no read with at most $MEM_MAX MEM matches" >&2; exit 1; }
  mv mem_few.txt ${g}_${L}_MEM.txt
  for mode in MAM MUM MEM; do
    gzip -9 -n -c ${g}_${L}_${mode}.txt > "$OUT/degen_${g}_${L}_${mode}.txt.gz"
  done
done < readsets.txt

chain() {   # $1, $2 = the mates' FASTQ files -> tagged.sam, tag.err; mappability_tag's status
  "$R/fastqs_to_sam" $1 $2 1 > q.sam
  rm -rf mapout
  "$R/mummer" -rcref -qthreads 2 -nomap -samin -samout mosaic.fa q.sam 2>/dev/null
  cat mapout/*.txt | grep '^@' | LC_ALL=C sort -u > hdr.txt
  cat mapout/*.txt | grep -v '^@' > body.sam
  "$R/mappability_tag" mosaic.fa <(cat hdr.txt body.sam) > tagged.sam 2> tag.err
}
for L in 40 100; do
  chain pairs_${L}_r1.fq pairs_${L}_r2.fq || { cat tag.err >&2; exit 1; }
  if grep -qi 'too big\|terminate\|what()' tag.err; then cat tag.err >&2; exit 1; fi
  grep -v '^@' tagged.sam \
    | awk -F'\t' 'BEGIN{OFS="\t"} {t=""; for(i=12;i<=NF;i++){ if($i ~ /^(XM|XU|XE|XS|NH|HI|L0|R0|cc|cp|xo|xc|CC|CP|XO|XC):/) t=t"\t"$i } print $1,$2,$3,$4,$5,$6,$7,$8,$9 t}' \
    | LC_ALL=C sort | gzip -9 -n -c > "$OUT/degen_mosaic_pairs_${L}_mapout_tagged.txt.gz"
  : > errors.txt
  for q in $(seq 0 $(( $(cat bad_$L.n) - 1 ))); do
    st=0
    chain bad_${L}_${q}_r1.fq bad_${L}_${q}_r2.fq || st=$?
    echo "$q $st $(grep -o '\(left\|right\) mappability too big [0-9]*' tag.err | tail -n 1)" >> errors.txt
  done
  cp errors.txt "$OUT/degen_mosaic_pairs_${L}_tag_errors.txt"
done
echo "degenerate golden written to $OUT"
