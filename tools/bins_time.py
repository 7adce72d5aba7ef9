"""tools/bins_time.py [K [NBINS]] -- the bin design (smash_bins_design) timed at
the benchmark's hg19-shaped genome, next to smash_mappability_scan over the
whole genome in the same process: the scan is the yardstick (both stream the
genome once; the design reads 2 B of map.bin + 1 B of text per base, the scan
reads 2 B of U and writes 2 B of map.bin per base).  The design's per-step
times (count / prefix sums / place, HIP events) come on stderr
(SMASH_BINS_TIMES); its wall time includes the allocations, the host's
apportionment and the copies.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("smash-paper_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    import numpy as np
    import torch

    import genome_cache
    import smashgpu as S
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 36
    nbins = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
    reps = 5
    contigs, (T, sp, sz, names) = genome_cache.genome_text("hg19")
    dix = S.Index.create(T, sp, sz, names, device=0)
    print("[bins_time] index: %.1f s, N = %d" % (dix.info.build_seconds, dix.N), flush=True)
    cs, n = {}, 0
    for name, s in contigs:                 # chrom_sizes.txt (index_setup.sh:28)
        if "_" not in name:
            cs[name] = n
            n += len(s)
    off = S.contig_tables(dix.contigs, dix.contig_sizes, cs)[2]
    total = int(sum(dix.contig_sizes))
    binned = int(sum(s for s, o in zip(dix.contig_sizes, off) if o >= 0))

    os.environ["SMASH_BINS_TIMES"] = "1"
    rec, M = dix.design_bins(off, k=k, nbins=nbins, unique=True)       # warm-up
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        again = dix.design_bins(off, k=k, nbins=nbins)
        wall.append(1e3 * (time.perf_counter() - t))
        assert np.array_equal(again, rec)
    os.environ.pop("SMASH_BINS_TIMES")

    # the scan over the same genome, binning by the designed starts: its counts
    # are the table's n_unique column
    d_bins = torch.from_numpy(np.ascontiguousarray(rec["abspos"], np.int64)).cuda()
    bc = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    cc = torch.zeros(len(dix.contigs), dtype=torch.int64, device="cuda")
    out = torch.empty(2 * total, dtype=torch.uint8, device="cuda")
    scan = []
    for i in range(reps + 1):
        bc.zero_()
        cc.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        S.mappability_scan(dix, 0, total, k, out, off, d_bins, nbins, bc, cc)
        e1.record()
        torch.cuda.synchronize()
        if i:
            scan.append(e0.elapsed_time(e1))
    same = bc.cpu().numpy().tolist() == rec["n_unique"].tolist()
    design_bytes, scan_bytes = 3 * binned, 4 * total
    w, s = min(wall), min(scan)
    print(json.dumps({
        "genome": "hg19", "k": k, "nbins": nbins, "bases": total, "binned_bases": binned,
        "unique": int(M.sum()), "design_wall_ms": [round(x, 3) for x in wall],
        "scan_ms": [round(x, 3) for x in scan], "design_bytes": design_bytes,
        "scan_bytes": scan_bytes, "design_GBps_wall": round(design_bytes / w / 1e6, 1),
        "scan_GBps": round(scan_bytes / s / 1e6, 1),
        "scan_counts_equal_n_unique": same}))


if __name__ == "__main__":
    main()
