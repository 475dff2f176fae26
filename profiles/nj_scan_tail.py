"""Where the blocks of njp_scan_kernel end (DPR_NJ_PHASES stamps), for several iterations of ONE process, and the pass-2
counters of the whole run (DPR_NJ_PHASES=-2):

  python3 profiles/nj_scan_tail.py [--tips 30000] [--sites 10000] [--its 3000,12000,24000] [--halves 1|2] [--json out.json]

Per stamped iteration: median / p90 / slowest block end of the unit blocks and of the new-row blocks (ns after the kernel's
first stamp; "end" = the drained stamp 4 behind the record store), which role the slowest block has and how many tied rows
(pass-2 row hits, all four waves) it resolved.  --halves: unit blocks per list entry of the build under test (the new-row
blocks are the first ceil(P / 512) of the grid; P follows the epoch schedule of njp_epoch_due)."""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--tips", type=int, default=30000)
ap.add_argument("--sites", type=int, default=10000)
ap.add_argument("--its", default="3000,12000,24000")
ap.add_argument("--halves", type=int, default=1)
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch  # noqa: F401,E402  (the HIP runtime bench.py runs on)
import numpy as np  # noqa: E402
import dipper_amd  # noqa: E402
from dipper_amd import capi  # noqa: E402


def alignment(n, L, seed=1):
    tmp = tempfile.mkdtemp(prefix="njt_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    p4 = os.path.join(tmp, "a.p4")
    k = 10000.0 / L
    subprocess.run([os.path.join(ROOT, "tools", "bin", "gen_synth"), "--tips", str(n), "--sites", str(L), "--seed", str(seed),
                    "--mean-bl", repr(2e-5 * k), "--lo", repr(2e-6 * k), "--hi", repr(2e-4 * k), "--packed4", p4], check=True)
    packed = np.fromfile(p4, dtype=np.uint64).reshape(n, (L + 15) // 16)
    os.unlink(p4); os.rmdir(tmp)
    return packed


def positions_at(N, it, epoch_min=2048):
    P = N
    for i in range(it + 1):
        n = N - i
        if P >= epoch_min and n <= P * 80 // 100 and n >= 3:
            P = n
    return P


packed = alignment(args.tips, args.sites)
L_ = capi.load_library()
L_.dpr_get_nj_phase_stamps.argtypes = [C.c_void_p]
out = []
for it in [int(x) for x in args.its.split(",")] + [-2]:
    os.environ["DPR_NJ_PHASES"] = str(it)
    d = dipper_amd.Dipper(0)
    d.set_msa(packed, args.sites)
    d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    d.nj_run()
    nj_ms = d.timing()[1]
    units = d.prune_stats()[0]
    buf = np.zeros(4 * 2048 * 8, np.uint64)
    assert L_.dpr_get_nj_phase_stamps(buf.ctypes.data) == 0
    d.close()
    if it == -2:
        rec = {"iteration": -2, "nj_ms": nj_ms, "units_listed": int(units), "pass2_row_hits": int(buf[5]), "pass2_wave_unit_entries": int(buf[6]),
               "hits_per_iteration": float(buf[5]) / (args.tips - 2), "entries_per_iteration": float(buf[6]) / (args.tips - 2)}
        out.append(rec); print(json.dumps(rec), flush=True)
        continue
    b = buf[:2048 * 8].reshape(2048, 8).astype(np.int64)
    used = b[:, 0] > 0
    t0 = b[used][:, 0].min()
    P = positions_at(args.tips, it)
    nrb = (P + 511) // 512
    idx = np.arange(2048)
    done = used & (b[:, 4] > 0)
    rec = {"iteration": it, "nj_ms": nj_ms, "positions": P, "new_row_blocks": nrb, "blocks_stamped": int(used.sum()), "blocks_with_work": int(done.sum())}
    end = 10 * (b[:, 4] - t0)
    for name, m in (("unit", done & (idx >= nrb)), ("new_row", done & (idx < nrb))):
        if not m.any():
            continue
        e = end[m]
        rec[name] = {"blocks": int(m.sum()), "median_end_ns": int(np.median(e)), "p90_end_ns": int(np.percentile(e, 90)), "slowest_end_ns": int(e.max()),
                     "median_start_ns": int(np.median(10 * (b[m][:, 0] - t0))), "tied_rows_median": float(np.median(b[m][:, 5])), "tied_rows_max": int(b[m][:, 5].max())}
    s = int(np.argmax(np.where(done, end, -1)))
    rec["slowest_block"] = {"index": s, "role": "unit" if s >= nrb else "new_row", "end_ns": int(end[s]), "start_ns": int(10 * (b[s, 0] - t0)),
                            "tied_rows": int(b[s, 5]) if s >= nrb else 0, "list_entry": (s - nrb) // args.halves if s >= nrb else -1}
    # the eight slowest unit blocks: end, start, tied rows
    order = [int(i) for i in np.argsort(np.where(done & (idx >= nrb), end, -1))[-8:][::-1]]
    rec["slowest_unit_blocks"] = [{"end_ns": int(end[i]), "start_ns": int(10 * (b[i, 0] - t0)), "tied_rows": int(b[i, 5])} for i in order]
    out.append(rec); print(json.dumps(rec), flush=True)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
