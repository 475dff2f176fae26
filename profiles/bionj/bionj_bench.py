"""BIONJ beside the streaming NJ loop on one GPU: run times (dpr_get_timing, medians of three runs after one warm-up) and, with
--accuracy, the normalised RF distance of both trees to the generating tree.  One JSON line per call on stdout.

    python profiles/bionj/bionj_bench.py --tips 20000 --sites 1000
    python profiles/bionj/bionj_bench.py --accuracy --tips 2000 --sites 500 --mean-bl 0.05

Inputs come from tools/bin/gen_synth (--model gtr+g+i), seeded; nothing is read from outside the repository."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402
from tests import _util  # noqa: E402


def build(d, packed4, sites, variant, dist_type):
    d.set_nj_mode(0)                 # NJ: the streaming loop (what DPR_NJ_MODE=stream selects); BIONJ runs it whatever the mode
    d.set_nj_variant(variant)
    d.dist_matrix(capi.SRC_MSA, dist_type)
    res = d.nj_run()
    return res, d.timing()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tips", type=int, default=20000)
    ap.add_argument("--sites", type=int, default=1000)
    ap.add_argument("--mean-bl", type=float, default=2e-4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dist", type=int, default=capi.DIST_JC)
    ap.add_argument("--accuracy", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        inp = _util.gen_synth(tmp, "in", a.tips, a.sites, a.seed, a.mean_bl, a.mean_bl / 10, a.mean_bl * 10, extra=("--model", "gtr+g+i"))
        d = dipper_amd.Dipper(0)
        try:
            d.set_msa(inp["packed4"], a.sites)
            rec = {"tips": a.tips, "sites": a.sites, "mean_bl": a.mean_bl, "dist_type": a.dist, "device": d.device_name()}
            if a.accuracy:
                for name, variant in (("nj", 0), ("bionj", 1)):
                    res, _ = build(d, inp["packed4"], a.sites, variant, a.dist)
                    nwk = _util.newick_from_merges(inp["names"], res["merge_x"], res["merge_y"], res["bl_x"], res["bl_y"], res["last_d"], fmt=repr)
                    rec["nrf_" + name] = _util.nrf(inp["tree"], nwk, tmp, name)
            else:
                for name, variant in (("nj_stream", 0), ("bionj", 1)):
                    build(d, inp["packed4"], a.sites, variant, a.dist)            # warm-up
                    ms = [build(d, inp["packed4"], a.sites, variant, a.dist)[1] for _ in range(a.runs)]
                    rec[name + "_ms"] = ms
                    rec[name + "_median_ms"] = statistics.median(ms)
                rec["ratio"] = rec["bionj_median_ms"] / rec["nj_stream_median_ms"]
                rec["extra_us_per_iteration"] = 1e3 * (rec["bionj_median_ms"] - rec["nj_stream_median_ms"]) / (a.tips - 2)
        finally:
            d.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
