"""Balanced minimum evolution NNI refinement (dpr_bme_nni) on one GPU.  One JSON line per call on stdout.

    python profiles/nni/nni_bench.py --tips 20000 --sites 1000            # the search from the NJ tree: ms, launches, rounds, GB/s
    python profiles/nni/nni_bench.py --tips 5000 --sites 1000 --command   # + the whole `dipper --nni` command against the plain one
    python profiles/nni/nni_bench.py --tips 5000 --caterpillar            # one evaluation of a caterpillar (one launch per row)
    python profiles/nni/nni_bench.py --accuracy --tips 2000 --sites 500 --mean-bl 0.05

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

import numpy as np  # noqa: E402

import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402
from tests import _bme_ref, _util  # noqa: E402

BIN = os.path.join(ROOT, "dipper_amd", "bin", "dipper")


def full(v):
    return repr(float(v))


def search(d, dist_type, mx, my, rounds):
    d.dist_matrix(capi.SRC_MSA, dist_type)
    t0 = time.perf_counter()
    res = d.bme_nni(mx, my, rounds)
    wall = 1e3 * (time.perf_counter() - t0)
    table_ms, select_ms = d.bme_timing()
    st = d.bme_stats()
    n = len(mx) + 2
    M = 2 * n - 2
    # every average of a pair with an internal node: two 8-byte reads, two 8-byte writes (ancestor pairs counted too: an upper figure)
    alg_bytes = 32.0 * (M * (M - 1) / 2 - n * (n - 1) / 2)
    ev = st["evaluations"]
    return res, dict(rounds=res["rounds"], moves=res["moves"], fallbacks=res["fallbacks"], candidates0=res["candidates0"], L0=res["L_rounds"][0],
                     L1=res["L_rounds"][-1], evaluations=ev, launches=st["launches"], launches_per_evaluation=st["launches"] / ev,
                     table_ms=table_ms, select_ms=select_ms, call_wall_ms=wall, table_ms_per_evaluation=table_ms / ev,
                     select_ms_per_evaluation=select_ms / ev, table_bytes=st["table_bytes"], alg_bytes_per_evaluation=alg_bytes,
                     table_gbs=alg_bytes * ev / table_ms / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tips", type=int, default=20000)
    ap.add_argument("--sites", type=int, default=1000)
    ap.add_argument("--mean-bl", type=float, default=2e-4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--dist", type=int, default=capi.DIST_JC)
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
                    out, stats = search(d, a.dist, res["merge_x"], res["merge_y"], a.rounds)
                    rec["nrf_" + name + "_nni"] = _util.nrf(inp["tree"], _bme_ref.newick(inp["names"], out["kids"], out["top"], out["len"], fmt=full), tmp, name)
                    rec[name + "_nni"] = {k: stats[k] for k in ("rounds", "moves", "fallbacks", "L0", "L1")}
            elif a.caterpillar:
                mx, my = _bme_ref.caterpillar_log(a.tips)
                search(d, a.dist, mx, my, 0)
                rec["caterpillar"] = search(d, a.dist, mx, my, 0)[1]
            else:
                d.dist_matrix(capi.SRC_MSA, a.dist)
                res = d.nj_run()
                rec["nj_ms"] = d.timing()[1]
                search(d, a.dist, res["merge_x"], res["merge_y"], 1)                # warm-up: allocation, first launches
                rec["nni"] = search(d, a.dist, res["merge_x"], res["merge_y"], a.rounds)[1]
                ms = C.c_float()
                nbytes = 8 * a.tips * a.tips
                assert d.L.dpr_bw_probe(d.h, nbytes, 0, 2048, 10, C.byref(ms)) == 0
                rec["bw_probe_gbs"] = nbytes / ms.value / 1e6
        finally:
            d.close()
        if a.command:
            for name, extra in (("plain", ()), ("nni", ("--nni", str(a.rounds)))):
                walls = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    r = subprocess.run([BIN, "-i", "m", "-I", inp["fasta"], "-O", os.path.join(tmp, "o.nwk"), "-m", "2", "-d", str(a.dist), *extra],
                                       capture_output=True, text=True, timeout=600)
                    assert r.returncode == 0, r.stderr[-2000:]
                    walls.append(time.perf_counter() - t0)
                rec["command_" + name + "_s"] = walls
                if extra:
                    rec["command_line"] = [ln for ln in r.stderr.split("\n") if ln.startswith("BME NNI:")][0]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
