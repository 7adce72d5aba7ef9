"""tools/samples_time.py -- many samples in one run (smash_pipeline_samples)
against one run per sample, on the GPU.

    samples_time.py [--samples S] [--pairs N] [--runs R] [--sharded] [--out FILE.json]
    samples_time.py --ab [--ab-pairs P] [--ab-runs 64,256,...] [--out FILE.json]
    samples_time.py --parse TRACE.csv FILE.json

S samples of N synthetic pairs each (tools/synth.py's hg19-shaped genome,
reads generated on the device, C2's geometry: 100 bases, sample_bins/100000),
resident in HBM, at the batch size bench.fit_batch picks for S * N pairs.

  baseline  per sample: reset, count_batches over its pairs, stats() (the
            counters are the run's, so they are read before the next reset)
  samples   reset, one table, one count_batches over all pairs, sample_stats()

--sharded adds the multi-GPU step at world 1 (dist.ShardedCounter, its
collectives over a one-rank process group, the next two batches searched
ahead, as bench.py's SMASH_BENCH_SHARDED=1 step):

  sharded_samples  the table over the global pair indexes
                   (smash_pipeline_samples_sharded), every batch through the
                   phase calls, sample_stats(): rows and counters as baseline's
  sharded_plain    the same pairs through the phase calls without a table

R alternating runs of each after one untimed run of each; per run the wall
time, the union of the search launches (profile_active) and their difference,
the time no search covers.  The count rows and the counters of the two paths
must be equal.  The result goes to stdout as one line and, with --out, to
FILE.json.

--ab: the emit kernel's short-run threshold.  One batch of P pairs cut into
samples of r pairs each, for every r, counted with every run on the LDS side
(SMASH_BIN_SHORT=0) and with every run direct (SMASH_BIN_SHORT=4294967295);
the kernel's time comes from a kernel trace of this process (rocprofv3
--kernel-trace), which --parse reads: FILE.json holds the order of the
labelled launches.  --parse also sums the emit kernels of a traced timing run."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("smash-paper_amd", "tools", ""):
    sys.path.insert(0, os.path.join(ROOT, _p))

import numpy as np  # noqa: E402

EMIT = ("k_emit_bin_smp", "k_emit_bin_lds", "k_bin_reduce", "k_emit_bin")


def parse(trace, order_path):
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    order = json.load(open(order_path))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6  # noqa: E731
    tot = {}
    for r in rows:
        for k in EMIT:
            if k + "(" in r["Kernel_Name"] or k + "<" in r["Kernel_Name"] or \
                    r["Kernel_Name"].rstrip().endswith(k):
                t = tot.setdefault(k, [0, 0.0])
                t[0] += 1
                t[1] += ms(r)
                break
    for k, (c, t) in sorted(tot.items()):
        print("%-16s %6d launches %10.3f ms in all %9.4f ms each" % (k, c, t, t / c))
    smp = [ms(r) for r in rows if "k_emit_bin_smp" in r["Kernel_Name"]]
    i = 0
    for label, n in order.get("emit_launches", []):
        d = sorted(smp[i:i + n])
        i += n
        if d:
            print("%-28s %3d launches  min %.4f  median %.4f  max %.4f ms"
                  % (label, len(d), d[0], d[len(d) // 2], d[-1]))
    if i != len(smp):
        print("(%d k_emit_bin_smp launches in the trace, %d labelled)" % (len(smp), i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=48)
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--sharded", action="store_true")
    ap.add_argument("--ab-pairs", type=int, default=1_000_000)
    ap.add_argument("--ab-runs", default="64,256,1024,4096,16384")
    ap.add_argument("--out", default=None, help="also write the result to this file "
                    "(--ab needs it: --parse reads the launches' order from it)")
    ap.add_argument("--parse", nargs=2, metavar=("TRACE.csv", "FILE.json"))
    args = ap.parse_args()
    if args.parse:
        return parse(*args.parse)
    if args.ab and not args.out:
        ap.error("--ab needs --out FILE.json")

    import tempfile

    import torch

    import bench
    import genome_cache
    import readgen
    import smashgpu as S
    cfg = dict(bench.CONFIGS["c2"])
    L = cfg["read_len"]
    dev = torch.device("cuda", 0)
    contigs, (T, sp, sz, names) = genome_cache.genome_text(cfg["genome"])
    dix = S.Index.create(T, sp, sz, names, device=0)
    starts = bench.bin_starts_for(cfg, contigs, tempfile.mkdtemp())
    cs = bench.chrom_sizes_for(cfg, contigs)
    nS, n = args.samples, args.pairs
    P = args.ab_pairs if args.ab else nS * n
    d_reads = S.to_rows(readgen.Generator(dix, contigs, L, seed=cfg["seed"] * 1000).generate(P), L)
    torch.cuda.synchronize()
    res = {"read_len": L, "bins": len(starts), "pairs": P}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    if args.ab:
        res["emit_launches"] = []
        for r in [int(x) for x in args.ab_runs.split(",")]:
            first = list(range(0, P, r)) + [P]
            for label, short in (("lds", "0"), ("direct", "4294967295")):
                os.environ["SMASH_BIN_SHORT"] = short
                pipe = S.Pipeline(dix, cs, starts, L, P, dedup_capacity=P,
                                  read_stride=d_reads.shape[1])
                c = torch.zeros((len(first) - 1, len(starts)), dtype=torch.int64, device=dev)
                rows = None
                for _ in range(4):
                    c.zero_()
                    pipe.reset()
                    pipe.set_samples(first)
                    pipe.count_batches(d_reads, P, P, c, resident=True)
                    torch.cuda.synchronize()
                    k = c.sum(dim=1).cpu().numpy()
                    assert rows is None or np.array_equal(rows, k)
                    rows = k
                res.setdefault("kept_%d" % r, int(rows.sum()))
                assert res["kept_%d" % r] == int(rows.sum())   # both sides count the same
                # (one launch per batch: the bin parts are its grid's y)
                res["emit_launches"].append(["run %6d %s" % (r, label), 4])
                pipe.close()
                del c
        os.environ.pop("SMASH_BIN_SHORT", None)
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res))
        return

    free = torch.cuda.mem_get_info(dev)[0]
    B = bench.fit_batch(12_500_000, P, L, free, headroom=6 << 30, nbins=len(starts),
                        max_batch=S.pipeline_max_batch(L))
    pipe = S.Pipeline(dix, cs, starts, L, B, dedup_capacity=P + P // 8 + (1 << 20),
                      read_stride=d_reads.shape[1])
    first = [s * n for s in range(nS + 1)]
    fields = ("pairs", "key_pairs", "dupe_pairs", "positions", "dups", "kept")
    six = lambda st: tuple(int(getattr(st, f)) for f in fields)  # noqa: E731
    c_base = torch.zeros((nS, len(starts)), dtype=torch.int64, device=dev)
    c_new = torch.zeros((nS, len(starts)), dtype=torch.int64, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        pipe.profile(True)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        active = pipe.profile_active()
        launches = pipe.profile_read()[1]
        pipe.profile(False)
        return out, {"wall_ms": wall, "search_union_ms": active, "uncovered_ms": wall - active,
                     "search_launches": int(launches)}

    def baseline():
        c_base.zero_()
        out = []
        for s in range(nS):
            pipe.reset()
            if pipe.n_samples:
                pipe.set_samples(None)
            pipe.count_batches(d_reads[2 * first[s]:2 * first[s + 1]], n, B, c_base[s],
                               resident=True)
            out.append(six(pipe.stats()))
        return out

    def samples():
        c_new.zero_()
        pipe.reset()
        pipe.set_samples(first)
        pipe.count_batches(d_reads, P, B, c_new, resident=True)
        return [six(x) for x in pipe.sample_stats()]

    forms = [("baseline", baseline), ("samples", samples)]
    if args.sharded:
        import socket

        import torch.distributed as tdist
        from dist import ShardedCounter
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(sock.getsockname()[1]))
        sock.close()
        tdist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        cpu = tdist.new_group(backend="gloo")
        pipe.reset()
        sc_smp = ShardedCounter(pipe, 0, 1, dev, count_group=cpu, plan_pairs=P, samples=first)
        sc_plain = ShardedCounter(pipe, 0, 1, dev, count_group=cpu, plan_pairs=P)
        c_plain = torch.zeros(len(starts), dtype=torch.int64, device=dev)
        nb = (P + B - 1) // B

        def sharded(sc, counts):
            counts.zero_()
            sc.reset()
            for b in range(nb):
                b0, b1 = b * B, min(P, (b + 1) * B)
                n1 = min(P, b1 + B)
                m1 = min(P, n1 + B)
                sc.step(d_reads[2 * b0:2 * b1], b1 - b0, b0, counts,
                        d_reads[2 * b1:2 * n1] if n1 > b1 else None, n1 - b1,
                        next2_reads=d_reads[2 * n1:2 * m1] if m1 > n1 else None,
                        next2_pairs=m1 - n1)
            sc.finish()

        def sharded_samples():
            sharded(sc_smp, c_new)
            return [tuple(r) for r in sc_smp.sample_stats()]

        def sharded_plain():
            sharded(sc_plain, c_plain)
            return int(pipe.stats().kept)

        forms += [("sharded_samples", sharded_samples), ("sharded_plain", sharded_plain)]

    def prepare(name):
        """the form's table, set outside the timed region: setting one waits
        for the device and allocates (baseline clears it, samples sets its own)"""
        if name.startswith("sharded"):
            pipe.reset()
            pipe.set_samples_sharded(first if name == "sharded_samples" else None)
            pipe.reads_resident(True)
        else:
            pipe.reads_resident(False)

    runs = {name: [] for name, _ in forms}
    for i in range(args.runs + 1):   # (the first of each is the warm-up)
        for name, fn in forms:
            prepare(name)
            st, t = timed(fn)
            if i:
                runs[name].append(t)
            if name in ("samples", "sharded_samples"):
                assert st == base_st, "the samples' counters differ from their own runs'"
                assert torch.equal(c_new, c_base), "the samples' count rows differ"
            elif name == "baseline":
                base_st = st
    res.update(samples=nS, pairs_per_sample=n, batch=B, runs=runs)
    for name, rs in runs.items():
        for k in ("wall_ms", "search_union_ms", "uncovered_ms"):
            v = sorted(r[k] for r in rs)
            res["%s_%s" % (name, k)] = {"median": round(v[len(v) // 2], 3),
                                        "min": round(v[0], 3), "max": round(v[-1], 3)}
    res["rows_and_counters_equal"] = True
    res["emit_launches"] = []
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if args.sharded:
        tdist.destroy_process_group()


if __name__ == "__main__":
    main()
