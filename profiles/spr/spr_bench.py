"""Balanced minimum evolution SPR search (dpr_bme_spr) on one GPU.  One JSON line per call on stdout.

    python profiles/spr/spr_bench.py --tips 20000 --sites 1000            # the search from the NJ tree: table and scan ms, GB/s
    python profiles/spr/spr_bench.py --tips 5000 --sites 1000 --command   # + the whole `dipper --spr` command against `--nni`
    python profiles/spr/spr_bench.py --tips 5000 --caterpillar            # one evaluation of a caterpillar (paths of n - 3 edges)
    python profiles/spr/spr_bench.py --accuracy --tips 2000 --sites 500 --mean-bl 0.05

Inputs come from tools/bin/gen_synth (--model gtr+g+i), seeded; nothing is read from outside the repository."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402
from tests import _bme_ref, _util  # noqa: E402

BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


def full(v):
    return repr(float(v))


def search(d, dist_type, mx, my, rounds, spr=True):
    d.dist_matrix(capi.SRC_MSA, dist_type)
    t0 = time.perf_counter()
    res = d.bme_spr(mx, my, rounds) if spr else d.bme_nni(mx, my, rounds)
    wall = 1e3 * (time.perf_counter() - t0)
    table_ms, select_ms = d.bme_timing()
    ev = d.bme_stats()["evaluations"]
    out = dict(rounds=res["rounds"], moves=res["moves"], fallbacks=res["fallbacks"], candidates0=res["candidates0"], L0=res["L_rounds"][0],
               L1=res["L_rounds"][-1], evaluations=ev, table_ms_per_evaluation=table_ms / ev, select_ms_per_evaluation=select_ms / ev, call_wall_ms=wall)
    if spr:
        n = len(mx) + 2
        # every (pruned subtree, target edge): an edge with t tips on one side gives 2 (n - t - 2) targets to that side, whatever
        # the tree: 4 (n - 3)(n - 2) in all, counted at 6 reads of 8 bytes each
        pairs = 4 * (n - 3) * (n - 2)
        scan_ms = d.bme_spr_timing()
        out.update(long_moves=res["long_moves"], max_k=res["max_k"], scan_ms_per_evaluation=scan_ms / ev, pairs_per_evaluation=pairs,
                   scan_gbs=48.0 * pairs * ev / scan_ms / 1e6, host_ms_per_evaluation=(wall - table_ms - select_ms - scan_ms) / ev,
                   spr_stats=d.bme_spr_stats())
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tips", type=int, default=20000)
    ap.add_argument("--sites", type=int, default=1000)
    ap.add_argument("--mean-bl", type=float, default=2e-4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--dist", type=int, default=capi.DIST_JC)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget-s", type=float, default=0.0, help="cap the rounds so that one SPR search stays below this (from the warm-up's time per evaluation); the cap is recorded")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--command", action="store_true")
    ap.add_argument("--caterpillar", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        inp = _util.gen_synth(tmp, "in", a.tips, a.sites, a.seed, a.mean_bl, a.mean_bl / 10, a.mean_bl * 10, fasta=a.command, extra=("--model", "gtr+g+i"))
        d = dipper_amd.Dipper(0)
        try:
            d.set_msa(inp["packed4"], a.sites)
            rec = {"tips": a.tips, "sites": a.sites, "mean_bl": a.mean_bl, "dist_type": a.dist, "device": d.device_name()}
            if a.accuracy:
                for name, variant in (("nj", 0), ("bionj", 1)):
                    d.set_nj_variant(variant)
                    d.dist_matrix(capi.SRC_MSA, a.dist)
                    res = d.nj_run()
                    nwk = _util.newick_from_merges(inp["names"], res["merge_x"], res["merge_y"], res["bl_x"], res["bl_y"], res["last_d"], fmt=full)
                    rec["nrf_" + name] = _util.nrf(inp["tree"], nwk, tmp, name)
                    for how, spr in (("nni", False), ("spr", True)):
                        out, stats = search(d, a.dist, res["merge_x"], res["merge_y"], a.rounds, spr)
                        text = _bme_ref.newick(inp["names"], out["kids"], out["top"], out["len"], fmt=full)
                        rec["nrf_" + name + "_" + how] = _util.nrf(inp["tree"], text, tmp, name)
                        rec[name + "_" + how] = {k: stats[k] for k in ("rounds", "moves", "fallbacks", "L0", "L1", "long_moves", "max_k") if k in stats}
            elif a.caterpillar:
                mx, my = _bme_ref.caterpillar_log(a.tips)
                search(d, a.dist, mx, my, 0)
                rec["caterpillar"] = search(d, a.dist, mx, my, 0)[1]
            else:
                d.dist_matrix(capi.SRC_MSA, a.dist)
                res = d.nj_run()
                rec["nj_ms"] = d.timing()[1]
                warm = search(d, a.dist, res["merge_x"], res["merge_y"], 1)[1]      # warm-up: allocation, first launches
                warm = search(d, a.dist, res["merge_x"], res["merge_y"], 1)[1]
                if a.budget_s > 0:
                    a.rounds = max(1, min(a.rounds, int(a.budget_s * 1e3 / (warm["call_wall_ms"] / warm["evaluations"]))))
                rec["rounds_asked"] = a.rounds
                rec["spr"] = search(d, a.dist, res["merge_x"], res["merge_y"], a.rounds)[1]
                rec["nni"] = search(d, a.dist, res["merge_x"], res["merge_y"], a.rounds, False)[1]
                ms = C.c_float()
                nbytes = 8 * a.tips * a.tips
                assert d.L.dpr_bw_probe(d.h, nbytes, 0, 2048, 10, C.byref(ms)) == 0
                rec["bw_probe_gbs"] = nbytes / ms.value / 1e6
        finally:
            d.close()
        if a.command:
            for name, line in (("nni", "BME NNI:"), ("spr", "BME SPR:")):
                walls = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    r = subprocess.run([BIN, "-i", "m", "-I", inp["fasta"], "-O", os.path.join(tmp, "o.nwk"), "-m", "2", "-d", str(a.dist), "--" + name,
                                        str(a.rounds)], capture_output=True, text=True, timeout=900)
                    assert r.returncode == 0, r.stderr[-2000:]
                    walls.append(time.perf_counter() - t0)
                rec["command_" + name + "_s"] = walls
                rec["command_" + name + "_line"] = [ln for ln in r.stderr.split("\n") if ln.startswith(line)][0]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
