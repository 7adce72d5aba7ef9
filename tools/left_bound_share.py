#!/usr/bin/env python3
"""tools/left_bound_share.py [PAIRS] -- how often the left map.bin byte's bound
decides (csrc/pipeline.hip mate_fast), measured on the
CPU: the rule of tests/left_bound_inputs.py over the match words of the
single-lane emulation (tools/sm_emu, hints=True), checked against the oracle's
map.bin, on the inputs of tests/rev_hint_inputs.py and on the benchmark's own
read model (tools/synth.py make_reads, which tools/readgen.hip follows) over
the mid genome, PAIRS pairs (default 3000) of 150 bases.  Prints, per input,
the share of alignments that skip the load and the rest by cause."""
import gzip
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tools", "tests", os.path.join("tools", "sm_emu"), "smash-paper_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import oracle as O  # noqa: E402
import sm_emu  # noqa: E402
import left_bound_inputs as B  # noqa: E402
import rev_hint_inputs as R  # noqa: E402
from conftest import gold, interleaved_reads  # noqa: E402


def share(ix, sets, min_excess=4):
    ix.accel()
    emu, lb = sm_emu.Emu(ix, packed=True), B.LeftBound(ix)
    for reads in sets:
        emu.map(reads, min_len=R.MIN_LEN, hints=True)
        for r in range(reads.shape[0]):
            for w in emu.words[r]:
                lb.word(w, reads.shape[1], min_excess)
    return lb.table()


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "tiny.fa")
        with gzip.open(gold("tiny.fa.gz"), "rb") as f, open(fa, "wb") as g:
            g.write(f.read())
        tiny = O.Index.from_fasta(fa)
    print("tiny genome, golden reads s150 + s100")
    print(share(tiny, [interleaved_reads("s150"), interleaved_reads("s100")]))
    print("tiny genome, edge and hand-made reads (150, 100)")
    print(share(tiny, [R.edge_reads_150(tiny), R.hand_reads(tiny, 150), R.hand_reads(tiny, 100)]))
    edge = O.Index(*O.text_from_contigs(R.edge_genome()))
    print("edge genome, its reads (150, 100)")
    print(share(edge, [R.edge_genome_reads(edge, 150), R.edge_genome_reads(edge, 100)]))
    g, (T, sp, sz, names) = R.mid_index()
    mid = O.Index(T, sp, sz, names)
    print("mid genome, edge and hand-made reads (150, 100)")
    print(share(mid, [R.edge_reads_150(mid), R.hand_reads(mid, 150), R.hand_reads(mid, 100)]))
    print("mid genome, the benchmark's read model: %d pairs of 150 bases, min_excess 4" % pairs)
    print(share(mid, [R.synth_reads(g, pairs, 150, seed=1300)]))
    print("the same, 100 bases")
    print(share(mid, [R.synth_reads(g, pairs, 100, seed=1301)]))


if __name__ == "__main__":
    main()
