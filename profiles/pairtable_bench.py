"""The pair-table distance types (9 TN93, 10 LogDet, 11 paralinear) beside the costliest older bodies (3 Tajima-Nei, 4 K2P), same
run, same alignment:
    python3 profiles/pairtable_bench.py [--tips 30000] [--sites 1000] [--queries 5120] [--backbone 50000] [--block-sites 10000]
                                        [--rounds 3] [--reps 3] [--skip-block]
1. the whole matrix of --tips x --sites through dpr_dist_matrix, timed by the library's events (dpr_get_timing), the types
   alternating over --rounds rounds after one warm-up round;
2. one --queries x --backbone block of --block-sites sites through dpr_msa_dist_block(reps) (transposed, as placement calls it).
One JSON line per (workload, type): every round's milliseconds, their median, pairs/s and the ratio to type 3 of the same run.
Committed output: profiles/pairtable/."""
import argparse, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--tips", type=int, default=30000)
ap.add_argument("--sites", type=int, default=1000)
ap.add_argument("--queries", type=int, default=5120)
ap.add_argument("--backbone", type=int, default=50000)
ap.add_argument("--block-sites", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--skip-block", action="store_true")
args = ap.parse_args()
import numpy as np
import dipper_amd
from dipper_amd import capi

TYPES = (3, 4, 9, 10, 11)


def alignment(n, L):
    tmp = tempfile.mkdtemp(prefix="ptb_")
    p4 = os.path.join(tmp, "a.p4")
    subprocess.run([os.path.join(ROOT, "tools", "bin", "gen_synth"), "--tips", str(n), "--sites", str(L), "--seed", "4", "--mean-bl", "2e-4",
                    "--lo", "2e-5", "--hi", "2e-3", "--model", "gtr+g+i", "--indel-gaps", "--packed4", p4], check=True)
    packed = np.fromfile(p4, dtype=np.uint64).reshape(n, (L + 15) // 16)
    os.unlink(p4); os.rmdir(tmp)
    return packed


def report(workload, pairs, ms):
    base = statistics.median(ms[3])
    for dt in TYPES:
        med = statistics.median(ms[dt])
        print(json.dumps({"workload": workload, "dist_type": dt, "ms": [round(v, 3) for v in ms[dt]], "ms_median": round(med, 3),
                          "pairs_per_s": pairs / (med * 1e-3), "ratio_to_type_3": round(med / base, 3)}), flush=True)


d = dipper_amd.Dipper(0)
print(json.dumps({"device": d.device_name()}), flush=True)
n, L = args.tips, args.sites
d.set_msa(alignment(n, L), L)
ms = {dt: [] for dt in TYPES}
for rnd in range(args.rounds + 1):
    for dt in TYPES:
        d.dist_matrix(capi.SRC_MSA, dt)
        if rnd:
            ms[dt].append(d.timing()[0])
report(f"matrix {n} x {L}", n * (n - 1) // 2, ms)
if not args.skip_block:
    q, b, L = args.queries, args.backbone, args.block_sites
    d.set_msa(alignment(q + b, L), L)
    ms = {dt: [] for dt in TYPES}
    for rnd in range(args.rounds):
        for dt in TYPES:
            _, t = d.msa_dist_block(b, q, b, dist_type=dt, transposed=True, fetch=False, reps=args.reps)      # (one warm launch inside)
            ms[dt].append(t)
    report(f"block {q} x {b} x {L}", q * b, ms)
d.close()
