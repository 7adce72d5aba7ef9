#!/usr/bin/env python3
"""tools/varlen_probe.py -- what the variable-length mode costs (MI355X).

On bench.py's C2 inputs (the hg19-shaped index, 1 M x 100 bp SMASH reads in
native rows, sample_bins/100000; bench.py's own builders, imported) it times
reads/s, read -> bin counts, of
  (a) the fixed-length pipeline                       (direct rows, GEO 100),
  (b) the variable-length pipeline on the same rows   (every row full),
  (c) the variable-length pipeline on the rows trimmed by
      tools/varlen_reads.py's rule (lengths 1..100),
checks that (b) counts what (a) counts, and prints one JSON line.  With
SMASH_SM_OCC=1 (set here) the search launches report their residency, the
waves per SIMD, on stderr.

    python3 tools/varlen_probe.py [--steps 20] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SMASH_SM_OCC", "1")

import numpy as np  # noqa: E402

import bench  # noqa: E402  (puts smash-paper_amd, tools, oracle on sys.path)
from varlen_reads import SPECIAL  # noqa: E402


def rule_lengths(rows, L):
    """the trim rule over the prepared rows' first L bytes (the probe's reads
    are generated on the device: there is no FASTQ text to hash), capped at L"""
    out = np.empty(rows.shape[0], np.int64)
    for i in range(rows.shape[0]):
        h = zlib.crc32(rows[i, :L].tobytes())
        c = h % 10
        n = SPECIAL[(h >> 8) % 16] if c == 0 else 1 + (h >> 8) % 19 if c == 1 else 20 + (h >> 8) % 131
        out[i] = min(n, L)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import smashgpu as S
    import readgen
    cfg = bench.CONFIGS["c2"]
    fut = bench.genome_start(cfg["genome"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    contigs, (T, sp, sz, names) = fut.result()
    dix = S.Index.create(T, sp, sz, names, device=0)
    bench.log("device index: %.1f s" % dix.info.build_seconds)
    starts = bench.bin_starts_for(cfg, contigs, tempfile.mkdtemp())
    cs = bench.chrom_sizes_for(cfg, contigs)
    P, L = cfg["pairs"], cfg["read_len"]
    d_full = S.to_rows(readgen.Generator(dix, contigs, L, seed=cfg["seed"] * 1000).generate(P), L)
    h = d_full.cpu().numpy()
    lens = rule_lengths(h, L)
    h_trim = h.copy()
    h_trim[np.arange(h.shape[1])[None, :] >= lens[:, None]] = 0
    d_trim = torch.from_numpy(h_trim).to(dev)

    def measure(var_len, d_reads):
        pipe = S.Pipeline(dix, cs, starts, L, P, dedup_capacity=P + P // 8 + (1 << 20),
                          read_stride=d_reads.shape[1], var_len=var_len)
        counts = torch.zeros(len(starts), dtype=torch.int64, device=dev)

        def step():
            counts.zero_()
            pipe.reset()
            pipe.count_batches(d_reads, P, P, counts, resident=True)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        st = pipe.stats()
        out = counts.cpu().numpy().copy()
        pipe.close()
        return 2 * P * args.steps / el, out, st.as_dict()

    a, ca, sa = measure(False, d_full)
    b, cb, sb = measure(True, d_full)
    c, cc, sc = measure(True, d_trim)
    res = {"workload": cfg["workload"], "pairs": P, "read_len": L, "steps": args.steps,
           "warmup": args.warmup,
           "fixed_reads_per_s": a, "var_full_reads_per_s": b, "var_trimmed_reads_per_s": c,
           "var_full_counts_equal_fixed": bool(np.array_equal(ca, cb)) and sa == sb,
           "trimmed_mean_len": float(lens.mean()), "trimmed_under_min_len": int((lens < 20).sum()),
           "stats_fixed": sa, "stats_var_trimmed": sc}
    bench.log("fixed %.3e, variable on full rows %.3e (%.1f%%), variable on trimmed rows %.3e reads/s"
              % (a, b, 100.0 * b / a, c))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["var_full_counts_equal_fixed"] else 1


if __name__ == "__main__":
    sys.exit(main())
