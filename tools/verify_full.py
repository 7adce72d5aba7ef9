"""Full-size run of the index verifier (smash_index_verify): build the index
of a synthetic genome on the device (default: bench.py's "hg19", through
tools/genome_cache.py), verify everything, and write the report as JSON.

    python tools/verify_full.py [--genome hg19] [--out profiles/verify1/report.json]

Next to the report of SMASH_VERIFY_ALL the file holds the wall seconds of
the checks run alone (layout / SA / LCP / SA | LCP: the fused pass with the
work list and the overflow table), the index sizes, and the fused pass as a
fraction of the random-load ceiling it is measured against (DESIGN.md section
1).  SMASH_VERIFY_TIMES=1 prints the stages of every call on stderr.
"""
import argparse
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "smash-paper_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# random 16-byte loads per second the device sustains (profiles/r01/
# randbench_random16B_ceiling.log) and the random lines the fused pass touches
# per rank: T[y-1..y], ISA[y-1..y+1], T[x+l], T[y+l], and L8[j], SA[j-1] for
# the reducible ranks (counted as a whole pair here: an upper bound)
CEILING_LOADS_PER_S = 48e9
LINES_PER_RANK = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", default="hg19")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "verify1", "report.json"))
    a = ap.parse_args()
    import torch

    import genome_cache
    import smashgpu as S
    assert torch.cuda.is_available(), "verify_full.py needs cuda:0"
    torch.cuda.init()   # (before the library's first HIP call, as bench.py does)
    _, (T, sp, sz, names) = genome_cache.genome_text(a.genome)
    ix = S.Index.create(T, sp, sz, names)
    N = int(ix.N)
    rep = ix.verify(S.VERIFY_ALL).as_dict()
    alone = {}
    for name, f in (("layout", S.VERIFY_LAYOUT), ("sa", S.VERIFY_SA), ("lcp", S.VERIFY_LCP),
                    ("sa_lcp", S.VERIFY_SA | S.VERIFY_LCP)):
        r = ix.verify(f)
        assert r.ok == 1, (name, r.as_dict())
        alone[name] = r.seconds
    floor = N * LINES_PER_RANK / CEILING_LOADS_PER_S
    out = {"genome": a.genome, "N": N, "idx_bytes": int(ix.info.idx_bytes),
           "pos_bits": int(ix.info.pos_bits), "n_lcp_overflow": int(ix.info.n_lcp_overflow),
           "build_seconds": ix.info.build_seconds, "report": rep, "seconds_alone": alone,
           "bound_2NlogN": 2 * N * math.log2(N),
           "bytes_compared_over_bound": rep["lcp_bytes_compared"] / (2 * N * math.log2(N)),
           "fused_floor_seconds": floor, "fused_over_floor": alone["sa_lcp"] / floor}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if rep["ok"] == 1 else 1


if __name__ == "__main__":
    sys.exit(main())
