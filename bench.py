#!/usr/bin/env python3
"""bench.py -- headline benchmark (BASELINE.json): tips/sec FASTA -> Newick at N = 30k on MI355X; with --full also
the Q-argmin HBM roofline, the hot path's own kernel record, a self-check of the timed result, CPU NJ baselines
timed on the host cores, the other sizes and the multi-rank legs.

One "step" = one pass of the whole path over one batch of synthetic input: the `dipper` command line (FASTA
parse, pack, H2D, all-pairs JC69 distances, all N-2 NJ iterations, Newick write) on this rank's GPU.  `value`
is BASELINE.json's metric measured over exactly K such steps.  A plain run does nothing else: input, W warm-up
steps, K timed steps, the outputs of the last step (--dump-outputs DIR) and the JSON line.  With --full the hot
path alone (packed tips resident in HBM -> distances -> NJ merge log, in process through the C ABI) is timed over
the same K/W next to it (`hot_path`), followed by everything listed above.
Run as `python bench.py --gpus N --steps K --warmup W [--full]`; for N > 1 the driver launches it under
torch.distributed.run (one rank per GPU, RCCL).  At 30 000 tips the default NJ (exact pruned scan) is ~16 us of
dependent latency per iteration, which no exchange can shorten, so the headline steps are replicas (`scaling: weak`);
north_star's own partitioning -- the matrix row-sharded over the ranks, one full Q scan per iteration -- is measured
next to it for every exchange plan of the library (`nj_scaling`), and the other sizes in `sharded_100k`.

Made for a first contact with several GPUs that cannot be rehearsed: every synthetic input is generated ONCE (rank 0,
native generator tools/bin/gen_synth, all host threads) into a shared directory and mapped by the ranks; every
child process and CPU leg gets host_cores() // ranks threads; optional legs are dropped against one global deadline
(`{"skipped": "budget"}`, exit code still 0); a hung collective is ended by one watchdog that prints the record and
exits non-zero; every multi-rank leg reports the rank count RCCL itself reports.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading
import time

T_START = time.monotonic()

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
UNIT_BYTES = 16 * 512 * 8      # one unit of the pruned scan: 16 rows x 512 columns of fp64
EXE = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
GEN = os.path.join(ROOT, "tools", "bin", "gen_synth")
NRF = os.path.join(ROOT, "tools", "bin", "nrf")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def elapsed():
    return time.monotonic() - T_START


def host_cores():
    """Threads this process may use: the smallest of os.cpu_count(), the affinity mask and the cgroup CPU
    quota (a GPU box exposes 256 logical CPUs but grants 16; oversubscribed OpenMP teams run many times slower)."""
    c = os.cpu_count() or 1
    try:
        c = min(c, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            c = min(c, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, c)


class Budget:
    """One global deadline (seconds since process start).  Optional legs ask before they start."""

    def __init__(self, deadline_s):
        self.deadline = float(deadline_s)

    def left(self):
        return self.deadline - elapsed()

    def allows(self, need_s):
        return self.left() > need_s

    agree = None        # several ranks: callable(bool) -> bool, true only when true on every rank (set once the ranks are joined)

    def allows_all(self, need_s):
        """the same answer on every rank (the clocks of the ranks start a little apart: a leg full of collectives must not
        be entered by some ranks and skipped by others)"""
        ok = self.allows(need_s)
        return self.agree(ok) if self.agree is not None else ok

    def skip(self, need_s):
        return {"skipped": "budget", "needed_s": need_s, "left_s": round(self.left(), 1)}


def stats_ms(xs):
    xs = [float(x) for x in xs]
    if not xs:
        return None
    return {"min": min(xs), "median": float(np.median(xs)), "max": max(xs), "mean": float(np.mean(xs))}


def pmc_traffic(n, world):
    """HBM bytes per scan launch from the committed rocprofv3 --pmc passes of
    `bench.py --probe-only` (profiles/pmc_scan.json; FETCH_SIZE doubled per the gfx950 correction of
    MI355X_MICROARCH.md, WRITE_SIZE as is).  None when no matching measurement is committed."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_scan.json")) as f:
            rec = json.load(f)
        if rec.get("n_active") == n and rec.get("n_gpus") == world:
            return rec["hbm_bytes_per_launch"]
    except Exception:
        pass
    return None


def merge_digest(res):
    h = hashlib.sha256()
    k = int(res.get("iters", len(res["merge_x"])))
    for key in ("merge_x", "merge_y", "bl_x", "bl_y"):
        h.update(np.ascontiguousarray(res[key][:k]).tobytes())
    return h.hexdigest()[:16]


def same_log(a, b):
    return bool(all(np.array_equal(a[k], b[k]) for k in ("merge_x", "merge_y", "bl_x", "bl_y")) and a["last_d"] == b["last_d"])


def nrf_of(true_tree, newick_text_or_path, tmp, tag):
    """normalised RF against the generating tree (the reference authors' accuracy measure, scripts/nrf.sh:26,36-60)"""
    path = newick_text_or_path
    if not os.path.exists(str(path)):
        path = os.path.join(tmp, "nrf_%s.nwk" % tag)
        with open(path, "w") as f:
            f.write(newick_text_or_path)
    r = subprocess.run([NRF, true_tree, path], capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": r.stderr[-200:]}
    d = json.loads(r.stdout)
    return {"nrf": d["nrf"], "rf": d["rf"], "splits_true": d["splits_a"], "splits_inferred": d["splits_b"]}


# ---------------------------------------------------------------------------------------------------------
# --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy (float64)
# ---------------------------------------------------------------------------------------------------------
DUMP_PAIRS = 1 << 19        # tip pairs whose path length is written: a fixed, seeded sample
DUMP_SEED = 20240611


def newick_arrays(text):
    """(parent, length, {leaf name: node}) of a Newick text.  Nodes are numbered in the order they open, so a parent comes
    before its children; the root's parent is -1, a missing length is 0.  Internal labels are ignored."""
    parent, length, leaf = [], [], {}
    stack, closed = [], None
    for tok in re.split(r"([(),;])", text):
        if tok == "(":
            parent.append(stack[-1] if stack else -1)
            length.append(0.0)
            stack.append(len(parent) - 1)
            closed = None
        elif tok == ")":
            closed = stack.pop()
        elif tok in (",", ";"):
            closed = None
        elif tok.strip():
            name, _, bl = tok.strip().partition(":")
            if closed is None:          # a leaf
                parent.append(stack[-1] if stack else -1)
                length.append(0.0)
                closed = len(parent) - 1
                leaf[name] = closed
            if bl:
                length[closed] = float(bl)
    return np.array(parent, dtype=np.int64), np.array(length, dtype=np.float64), leaf


def tree_outputs(text, pairs=DUMP_PAIRS, seed=DUMP_SEED):
    """The tree of a Newick text as arrays that do not depend on the order in which it lists children.  Tips are taken in
    the order of their names by (length, text): T1, T2, ..., T10, ...  tip_branch_length / tip_root_distance: per tip;
    tip_pair_index: a seeded sample of pairs of distinct tips; tip_pair_distance: the path length between them."""
    parent, length, leaf = newick_arrays(text)
    depth = np.zeros(len(parent))
    level = np.zeros(len(parent), dtype=np.int64)
    for v in range(1, len(parent)):
        depth[v] = depth[parent[v]] + length[v]
        level[v] = level[parent[v]] + 1
    tips = np.array([leaf[k] for k in sorted(leaf, key=lambda s: (len(s), s))], dtype=np.int64)
    n = len(tips)
    p = min(pairs, n * (n - 1) // 2)
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, p)
    b = rng.integers(0, max(n - 1, 1), p)
    b += b >= a
    # lowest common ancestors by binary lifting (ups[k] = the 2^k-th ancestor; the root is its own parent)
    ups = [np.where(parent < 0, 0, parent)]
    for _ in range(int(level.max(initial=0)).bit_length()):
        ups.append(ups[-1][ups[-1]])
    x, y = tips[a], tips[b]
    swap = level[x] < level[y]
    x, y = np.where(swap, y, x), np.where(swap, x, y)
    diff = level[x] - level[y]
    for k, up in enumerate(ups):
        sel = ((diff >> k) & 1).astype(bool)
        x[sel] = up[x[sel]]
    for up in reversed(ups):
        ux, uy = up[x], up[y]
        ne = ux != uy
        x, y = np.where(ne, ux, x), np.where(ne, uy, y)
    lca = np.where(x == y, x, ups[0][x])
    return {"tip_branch_length": length[tips], "tip_root_distance": depth[tips],
            "tip_pair_index": np.stack([a, b], axis=1).astype(np.float64),
            "tip_pair_distance": depth[tips[a]] + depth[tips[b]] - 2.0 * depth[lca]}


def dump_outputs(path, arrays):
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    log(f"[bench] outputs of the last timed step: {', '.join(sorted(arrays))} in {path}")


# ---------------------------------------------------------------------------------------------------------
# inputs: generated once per job by rank 0 into a shared directory, mapped by every rank
# ---------------------------------------------------------------------------------------------------------
class Stage:
    def __init__(self, rank, world, dist):
        self.rank, self.world, self.dist = rank, world, dist
        path = [None]
        if rank == 0:
            base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > (4 << 30) else tempfile.gettempdir()
            path[0] = tempfile.mkdtemp(prefix="dipper_bench_", dir=base)
        if dist is not None:
            dist.broadcast_object_list(path, src=0)
        self.dir = path[0]
        self.times = {}

    def sync(self):
        if self.dist is not None:
            self.dist.barrier()

    model = "gtr+g+i"      # substitution model of the aligned inputs (--model)

    def gen(self, tag, tips, sites, seed, mean, lo, hi, fasta=False, reads=False, shuffle=None, gap=None, model=None):
        """returns the paths of input `tag`; rank 0 runs the generator (all host threads: the other ranks wait)"""
        base = os.path.join(self.dir, tag)
        p = {"tips": tips, "sites": sites, "tree": base + ".nwk", "fasta": base + ".fa" if fasta else None,
             "packed4": None if reads else base + ".p4", "packed2": base if reads else None, "order": base + ".ord" if shuffle is not None else None}
        if self.rank == 0 and not os.path.exists(p["tree"]):
            t0 = time.perf_counter()
            cmd = [GEN, "--tips", str(tips), "--sites", str(sites), "--seed", str(seed), "--mean-bl", repr(mean), "--lo", repr(lo), "--hi", repr(hi),
                   "--tree", p["tree"], "--threads", str(host_cores())]
            if fasta:
                cmd += ["--fasta", p["fasta"]]
            if reads:
                cmd += ["--indel", "0.03,0.09", "--packed2", p["packed2"]]
            else:
                cmd += ["--packed4", p["packed4"]]
                if (model or self.model) != "jc69":
                    cmd += ["--model", model or self.model]
                if gap is not None and gap >= 0:      # (gap < 0 / None: gap-free; 0: inherited deletions only; > 0: + per-tip runs)
                    cmd += ["--indel-gaps"]
                    if gap > 0:
                        cmd += ["--gap-frac", repr(float(gap))]
            if shuffle is not None:
                cmd += ["--shuffle", str(shuffle), "--order", p["order"]]
            subprocess.run(cmd, check=True)
            self.times[tag] = time.perf_counter() - t0
            log(f"[bench] input {tag}: {tips} x {sites} generated in {self.times[tag]:.1f} s")
        self.sync()
        return p

    @staticmethod
    def packed4(p):
        return np.memmap(p["packed4"], dtype=np.uint64, mode="r", shape=(p["tips"], (p["sites"] + 15) // 16))

    @staticmethod
    def reads(p):
        return (np.fromfile(p["packed2"] + ".flat", dtype=np.uint64), np.fromfile(p["packed2"] + ".off", dtype=np.uint64),
                np.fromfile(p["packed2"] + ".len", dtype=np.uint64))

    def drop(self, p):
        """remove the files of one input (the protocol-length ones are gigabytes of /dev/shm, which is host memory)"""
        if self.rank != 0:
            return
        for f in (p.get("fasta"), p.get("packed4"), p.get("order")):
            if f and os.path.exists(f):
                os.unlink(f)
        if p.get("packed2"):
            for ext in (".flat", ".off", ".len"):
                if os.path.exists(p["packed2"] + ext):
                    os.unlink(p["packed2"] + ext)

    def room_for(self, nbytes):
        try:
            return shutil.disk_usage(self.dir).free > nbytes
        except OSError:
            return False

    def cleanup(self):
        if self.rank == 0 and self.dir:
            shutil.rmtree(self.dir, ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------
# CPU baselines (rank 0, N = 1 only; bounded samples)
# ---------------------------------------------------------------------------------------------------------
def gpu_matrix_block(dip, m):
    D = np.zeros((m, m), dtype=np.float64)
    for i in range(m):
        D[i, :] = dip.matrix_row(i)[:m]
    return D


def cpu_baseline(dip, n, cores, budget_s=15.0):
    """CPU NJ (the oracle's restatement of the reference's arithmetic, OpenMP over row bands) on a
    bounded sample: init + the first k iterations at full size on the GPU's own matrix, scaled to the
    whole run by the sum of n^2 (every iteration is one full scan).  Distances are NOT included."""
    import ctypes as C
    import psutil
    from tests import _orc
    from tests._orc import _p, c_f64p, c_i32p
    orc = _orc.load()
    log(f"[cpu_baseline] oracle NJ on {cores} host thread(s) ...")
    need = n * n * 8 * 1.15
    avail = psutil.virtual_memory().available
    ns = n
    if need > 0.5 * avail:
        ns = int((0.5 * avail / 9.2) ** 0.5)
        log(f"[cpu_baseline] host memory {avail/2**30:.0f} GiB: sampling the leading {ns} tips")
    D = np.tril(gpu_matrix_block(dip, ns), -1)
    k_max = 512
    mx = np.zeros(k_max, np.int32); my = np.zeros(k_max, np.int32)
    bx = np.zeros(k_max); by = np.zeros(k_max)
    last = C.c_double()

    def run(k):
        Dc = D.copy()
        t0 = time.perf_counter()
        orc.lib.orc_nj_run(_p(Dc, c_f64p), ns, ns, cores, k, _p(mx, c_i32p), _p(my, c_i32p),
                           _p(bx, c_f64p), _p(by, c_f64p), C.byref(last), None)
        return time.perf_counter() - t0

    t0 = run(0)            # mirror + row sums only
    t2 = run(2)
    per_it = max((t2 - t0) / 2, 1e-6)
    k = int(max(2, min(k_max, (budget_s - t2) / per_it)))
    tk = run(k) if k > 2 else t2
    per_it = (tk - t0) / k
    s_sample = sum(float(ns - i) ** 2 for i in range(k))
    s_full = sum(float(m) ** 2 for m in range(3, n + 1))
    t_full = t0 * (n / ns) ** 2 + per_it * k * s_full / s_sample
    return {
        "value": n / t_full, "unit": "tips/s", "cores": cores, "kind": "port",
        "sample": f"oracle NJ (reference arithmetic, OpenMP {cores} thread(s)) on the GPU's matrix "
                  f"(leading {ns} tips): init + first {k} of {n-2} iterations timed ({tk:.1f} s), scaled to the "
                  f"whole run by sum(n^2) (every iteration is one full O(n^2) scan); distance stage excluded",
    }


def cpu_baseline_rapidnj(dip, n, cores, budget_s=20.0):
    """Stronger CPU baseline: a from-scratch RapidNJ-style exact NJ (sorted rows + q_min pruning, OpenMP;
    oracle/rapidnj_baseline.c -- north_star names RapidNJ, which is not installed and cannot be fetched).
    Whole NJ run on the leading m tips of the GPU's matrix, m sized to the time budget; scaled to N with the
    exponent validated once against the full run.  Distances excluded."""
    import psutil
    from tests import _orc
    orc = _orc.load()
    log(f"[cpu_baseline_rapidnj] RapidNJ-style NJ on {cores} host threads ...")

    def run(D):
        t0 = time.perf_counter()
        r = orc.rapidnj_run(D, threads=cores)
        dt = time.perf_counter() - t0
        assert r["joins"] == D.shape[0] - 2
        log(f"[cpu_baseline_rapidnj] {D.shape[0]} tips: {dt:.2f} s")
        return dt

    # Round 4: ONE block as large as the budget allows, scaled with the exponent VALIDATED against the full run: 30 000 tips take
    # 161 s on 16 threads (186 tips/s), 15 295 tips 38.2 s -> exponent 2.14 (profiles/r4/cpu_baseline_validation.jsonl).  Until round 3
    # the exponent was measured in every run between two small blocks (3 000 / 6 000, then 4 000 / 8 000 tips): it came out anywhere
    # from 2.2 to 3.0 on the shared host, a 4 x spread of the extrapolated figure (48 .. 182 tips/s).
    expo = 2.14
    # (sizing: a pilot at 4 000 tips, and a deliberately steep exponent -- 2.6 -- for choosing the block, so that a slow or busy
    #  host cannot turn the 20 s budget into 100 s: the first version sized the block from a 2 000-tip pilot with 2.14 and once
    #  spent 102 s on 16 213 tips)
    m0 = min(n, 4000)
    t0 = run(gpu_matrix_block(dip, m0))
    avail = psutil.virtual_memory().available
    m = min(n, int(m0 * (budget_s / max(t0, 1e-3)) ** (1.0 / 2.6)), 12000)
    m = min(m, int((0.4 * avail / 14.0) ** 0.5))       # matrix copy + working copy + sorted rows
    m = max(m0, min(m, n))
    tm = run(gpu_matrix_block(dip, m)) if m > m0 else t0
    t_full = tm * (n / m) ** expo
    # The exponent's provenance travels with the figure (advisor, round 4): it was measured ONCE -- 15 295 vs 30 000 tips of the
    # JC69 gap-free input on one 16-thread host -- and is applied to whatever --tips / --model this run uses; the figure is an
    # EXTRAPOLATION by a factor (N/m)^2.14 >= 7 whenever N > m.  The same validation file holds the one full run there is:
    # 30 000 tips in 161 s = 186 tips/s; the driver's round-4 line extrapolated 114.8 tips/s from 10 265 tips on its host
    # (the sorted-row search prunes better as N grows: the effective exponent between 10 000 and 30 000 tips is below 2.14).
    same_as_validation = (n == 30000)
    return {"value": n / t_full, "unit": "tips/s", "cores": cores, "kind": "rapidnj-style reimplementation (not the oracle)",
            "status": "whole run timed" if m == n else ("extrapolated (exponent validated at this size on another host and input)" if same_as_validation
                                                         else "extrapolated, unvalidated at this size"),
            "exponent": None if m == n else expo,
            "exponent_provenance": {"fitted_between_tips": [15295, 30000], "input": "jc69, no gaps", "host_threads": 16,
                                    "record": "profiles/r4/cpu_baseline_validation.jsonl"},
            "validated_full_run": {"tips": 30000, "seconds": 161.0, "tips_per_s": 186.0, "host_threads": 16, "same_host": False,
                                   "record": "profiles/r4/cpu_baseline_validation.jsonl"},
            "sample": f"exact NJ with RapidNJ's sorted-row search on the GPU's matrix, leading {m} of {n} tips in {tm:.1f} s "
                      + ("(whole run)" if m == n else f"scaled by (N/m)^{expo:.2f}: an extrapolation by {(n / m) ** expo:.1f} x, not a measurement; the one full 30 000-tip run "
                         "on record took 161 s = 186 tips/s on 16 threads of another host")
                      + "; distance stage excluded"}


def rapidnj_probe(dip, n, cores, tmp, budget_s=30.0):
    """The reference authors' own baseline command (scripts/experiment.sh:123: `rapidnj <phylip> -i pd -c $(nproc)`),
    if a `rapidnj` binary is on PATH of this box; otherwise say so."""
    exe = shutil.which("rapidnj")
    if not exe:
        return {"found": False, "note": "no `rapidnj` on PATH (not installable here: no network); "
                                        "see cpu_baseline_rapidnj for the from-scratch stand-in"}
    from tests import _util
    m = min(n, 4000)
    D = gpu_matrix_block(dip, m)
    path = os.path.join(tmp, "rapidnj_in.phy")
    _util.write_phylip_lower(path, ["T%d" % (i + 1) for i in range(m)], D)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([exe, path, "-i", "pd", "-c", str(cores)], capture_output=True, text=True, timeout=budget_s * 4)
    except Exception as e:
        return {"found": True, "path": exe, "error": repr(e)}
    dt = time.perf_counter() - t0
    return {"found": True, "path": exe, "rc": r.returncode, "tips": m, "wall_s": dt, "tips_per_s": m / dt,
            "command": f"rapidnj in.phy -i pd -c {cores}", "note": "PHYLIP parse included; leading block of the GPU's matrix"}


# ---------------------------------------------------------------------------------------------------------
CLI_PHASE_TAGS = (("input_ms", "Input in:"), ("device_ready_ms", "Device ready in:"), ("parsed_ms", "Parsed in:"), ("tree_ms", "Tree Created in:"), ("sketch_ms", "Sketch Created in:"),
                  ("distance_ms", "Distance Operation Time"), ("tree_op_ms", "Tree Operation Time"))


def cli_phases(stderr_text):
    """milliseconds of the `dipper` command's own progress lines (the reference prints the same ones: src/tree_generation.cu:369-536,
    src/placement_close_k.cu:852-853,985-986); lines look like `Input in: 132 ms` or `Distance Operation Time 3640 ms`"""
    ph = {}
    for line in stderr_text.splitlines():
        for key, tag in CLI_PHASE_TAGS:
            if line.startswith(tag):
                try:
                    ph[key] = float(line[len(tag):].replace(":", " ").split()[0])
                except Exception:
                    pass
    return ph


def cli_step(fa, out, device, threads, idle_s=0.0):
    env = dict(os.environ, DPR_HOST_THREADS=str(threads))
    if idle_s > 0:
        time.sleep(idle_s)        # (isolated steps: the previous process's teardown in the kernel driver is over)
    t0 = time.perf_counter()
    r = subprocess.run([EXE, "-i", "m", "-I", fa, "-O", out, "-m", "2", "-d", "2", "--device", str(device)],
                       capture_output=True, text=True, env=env)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("dipper failed: " + r.stderr[-400:])
    ph = cli_phases(r.stderr)
    return dt, {k: ph[v] for k, v in (("input", "input_ms"), ("tree", "tree_ms"), ("device_ready", "device_ready_ms"), ("parsed", "parsed_ms")) if v in ph}


def join_comm(dip, rank, world, dist):
    """the library's own RCCL communicator on `dip`; returns the rank count RCCL reports.  DPR_BENCH_ONE_GPU=1 (every rank on
    GPU 0, which RCCL refuses): the ranks join through a shared region instead and exchange through device windows over hipIpc
    (dpr_comm_init_shared, transport ipc); the count is then the number of ranks the region has seen."""
    from dipper_amd import capi
    if ONE_GPU:
        name = [("dpr_bench_%d_%d" % (os.getpid(), int(time.time() * 1e3) % 1000000)) if rank == 0 else None]
        if rank == 0:
            capi.SharedRegion(name[0], create=True)
        dist.broadcast_object_list(name, src=0)
        region = capi.SharedRegion(name[0])
        dip.comm_init_shared(rank, world, region, capi.TRANSPORT_IPC)
        dist.barrier()
        if rank == 0:
            region.unlink()
        return dip.comm_info()[1]
    uid = [dip.comm_unique_id() if rank == 0 else None]
    dist.broadcast_object_list(uid, src=0)
    dip.comm_init(rank, world, uid[0])
    return dip.comm_info()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tips", type=int, default=30000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gap-frac", type=float, default=0.0,
                    help="STRESS input: expected fraction of '-' cells per tip in the aligned inputs, independent from tip to tip "
                         "(gen_synth --gap-frac).  Not the authors' protocol; at 0.03 the pruned NJ lists 80 x the units (5.7 s at 30 000 tips)")
    ap.add_argument("--model", default="gtr+g+i", choices=["jc69", "gtr+g+i"],
                    help="substitution model of the generated ALIGNED inputs (gen_synth --model): gtr+g+i = the authors' protocol "
                         "(scripts/alisim.sh:14), jc69 = the inputs of rounds 1-3.  The distance type of the runs stays -d 2 (JC69) either way")
    ap.add_argument("--no-indel-gaps", action="store_true",
                    help="aligned inputs without the inherited deletion gaps of the authors' indel model (gen_synth --indel-gaps, "
                         "scripts/alisim.sh:14): the gap-free inputs of rounds 1-3")
    ap.add_argument("--probe-reps", type=int, default=20)
    ap.add_argument("--deadline-s", type=float, default=float(os.environ.get("DPR_BENCH_DEADLINE_S", "500")),
                    help="optional legs are skipped when they would not finish this many seconds after process start "
                         "(the driver allows 600 s); a watchdog ends the run 60 s later, non-zero")
    ap.add_argument("--add-backbone", type=int, default=500000)
    ap.add_argument("--add-queries", type=int, default=50000)
    ap.add_argument("--no-add-leg", action="store_true", help="skip other_configs' configs[4] legs (--add of 50 000 queries onto 500 000 tips, aligned and Mash)")
    ap.add_argument("--no-protocol-length", action="store_true",
                    help="skip other_configs' legs at the authors' sequence length (10 000 sites / bases; scripts/experiment.sh:14) for configs[2]-[4]")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-cli", action="store_true",
                    help="skip the command-line steps: `value` is then the in-process hot path (used when profiling the kernels)")
    ap.add_argument("--no-parity", action="store_true", help="skip the untimed self-check of the timed result")
    ap.add_argument("--no-sharded", action="store_true", help="several GPUs: skip the 100 000-tip sub-record")
    ap.add_argument("--no-stream-leg", action="store_true", help="skip the row-sharded streaming-NJ sub-record (nj_scaling)")
    ap.add_argument("--no-virtual-pruned", action="store_true", help="skip the row-sharded pruned NJ with 8 virtual ranks on one GPU (nj_scaling.row_sharded_pruned_virtual)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="one GPU: skip the single runs of the other BASELINE sizes (NJ at 100 000 tips, placement of 100 000 unaligned tips, "
                         "divide-and-conquer of 1 000 000 tips)")
    ap.add_argument("--stream-iters", type=int, default=256)
    ap.add_argument("--exchanges", default=os.environ.get("DPR_BENCH_EXCHANGES", "legacy,peer,mailbox"),
                    help="exchange plans of the row-sharded NJ loop to time on several GPUs, in this order")
    ap.add_argument("--dc-tips", type=int, default=1000000, help="size of the divide-and-conquer sub-record")
    ap.add_argument("--sharded-tips", type=int, default=100000)
    ap.add_argument("--sharded-sites", type=int, default=10000)
    ap.add_argument("--probe-only", action="store_true",
                    help="with --full: skip the timed steps; only build the matrix and run the roofline probe "
                         "(used for the rocprofv3 --pmc passes)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline steps: the hot path in process with its kernel record, the self-check of the timed "
                         "result, the Q-argmin roofline, the CPU baselines, the other sizes and the multi-rank legs (the --no-* "
                         "options choose among them).  Without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step to DIR/<name>.npy (float64): for the `dipper` "
                         "command the tree it wrote (per-tip branch lengths and root distances, path lengths of a seeded sample of "
                         "tip pairs), for the in-process hot path the merge log")
    args = ap.parse_args()
    if args.probe_only and not args.full:
        ap.error("--probe-only is part of --full")

    # stdout carries exactly ONE line, the JSON record: everything else that writes to file descriptor 1 (RCCL prints
    # a version banner there when a communicator is created) is sent to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if world != args.gpus:
        log(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}: using WORLD_SIZE")
    threads = max(1, host_cores() // max(1, local_world))      # host threads of THIS rank (CLI readers, CPU legs)
    os.environ["DPR_HOST_THREADS"] = str(threads)
    budget = Budget(args.deadline_s)

    import torch
    import dipper_amd
    from dipper_amd import capi
    from tests import _util

    dist = None
    # DPR_BENCH_CHECK=1 under `torch.distributed.run --nproc-per-node 1` rehearses the multi-GPU legs on one GPU
    force_check = os.environ.get("DPR_BENCH_CHECK") == "1" and "RANK" in os.environ
    if world > 1 or force_check:
        import torch.distributed as dist
        if ONE_GPU:
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if dist is not None and world > 1:
        def agree(flag):
            t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=TDEV)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(int(t.item()))
        budget.agree = agree

    out = {}
    # the native input generator and the nRF tool are built by __graft_entry__.build(); a tree that was copied without its
    # binaries builds them here (`make -C tools` builds gen_synth and nrf with g++ only; the hipcc profiling aid lat_probe is a separate target), once, before any rank needs them
    if rank == 0 and not (os.path.exists(GEN) and os.path.exists(NRF)):
        log("[bench] building tools/ (gen_synth, nrf)")
        subprocess.run(["make", "-C", os.path.join(ROOT, "tools")], check=True, capture_output=True)
    stage = Stage(rank, world, dist)
    stage.model = args.model

    # ONE watchdog for the whole run: a hung collective (or anything else) must not outlive the driver's limit -- the
    # record so far is printed and the process ends NON-ZERO, which makes the launcher tear the job down
    def give_up():
        out["watchdog"] = "no result %d s after start: record printed by the watchdog, exit code 3" % int(elapsed())
        if rank == 0:
            os.write(json_fd, (json.dumps(out, default=str) + "\n").encode())
        stage.cleanup()
        os._exit(3)

    dog = threading.Timer(max(30.0, args.deadline_s + 60.0 - elapsed()), give_up)
    dog.daemon = True
    dog.start()
    # ... and shortly before that, where every thread of this rank is (stderr): a hang is then a line number, not a guess
    import faulthandler
    faulthandler.dump_traceback_later(max(20.0, args.deadline_s + 45.0 - elapsed()), exit=False)

    n, L = args.tips, args.sites
    want_cli = not args.no_cli and not args.probe_only and os.path.exists(EXE)
    inp = stage.gen("main", n, L, args.seed, 2e-5, 2e-6, 2e-4, fasta=want_cli, gap=None if args.no_indel_gaps else args.gap_frac)
    packed = Stage.packed4(inp)
    names = ["T%d" % (i + 1) for i in range(n)]
    tmp = tempfile.mkdtemp(prefix="dipper_bench_r%d_" % rank)
    fa, nwk = inp["fasta"], os.path.join(tmp, "out.nwk")
    if args.probe_only:
        args.steps = args.warmup = 0
    # the device the steps run on, opened through the library the `dipper` command links (set-up, before any timing): a
    # device or a build of the library that cannot run the steps ends the run here, and the line names the device measured
    ctx = dipper_amd.Dipper(local_rank)
    try:
        device = ctx.device_name()
    finally:
        ctx.close()
    if rank == 0:
        log(f"[bench] device {local_rank}: {device}")

    try:
        # =====================================================================================================
        # A. BASELINE.json's metric: FASTA -> Newick, the whole `dipper` command, K timed steps after W warm-ups
        # =====================================================================================================
        cli = None
        if want_cli:
            for _ in range(args.warmup):
                cli_step(fa, nwk, local_rank, threads)
            barrier()
            t0 = time.perf_counter()
            walls, inputs, trees, readies, parses = [], [], [], [], []
            for _ in range(args.steps):
                dt, ph = cli_step(fa, nwk, local_rank, threads)
                walls.append(dt * 1e3)
                inputs.append(ph.get("input", float("nan")))
                trees.append(ph.get("tree", float("nan")))
                readies.append(ph.get("device_ready", float("nan")))
                parses.append(ph.get("parsed", float("nan")))
            barrier()
            dt_cli = time.perf_counter() - t0
            if dist is not None:
                t = torch.tensor([dt_cli], dtype=torch.float64, device=TDEV)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt_cli = float(t.item())
            if args.dump_outputs and rank == 0 and args.steps > 0:
                with open(nwk) as f:
                    dump_outputs(args.dump_outputs, tree_outputs(f.read()))
            others = [w - i - t for w, i, t in zip(walls, inputs, trees)]
            cli = {"metric": "tips/sec FASTA -> Newick, whole CLI run (process start, FASTA parse, pack, H2D, JC69 distances, NJ, Newick write)",
                   "command": "dipper -i m -I in.fa -O out.nwk -m 2 -d 2 --device <local rank>",
                   "steps": args.steps, "warmup": args.warmup, "host_threads_per_rank": threads,
                   "wall_ms": stats_ms(walls), "input_ms": stats_ms(inputs), "tree_ms": stats_ms(trees),
                   "other_ms": stats_ms(others), "hip_startup_ms": stats_ms(readies), "parse_ms": stats_ms(parses),
                   "input_bound_by": {"device_ready": int(sum(1 for r_, p_ in zip(readies, parses) if r_ >= p_)),
                                      "parse": int(sum(1 for r_, p_ in zip(readies, parses) if r_ < p_))},
                   "note": "wall = input + tree + other; input ends when BOTH the parsed FASTA (parse_ms: file read + packed, host side) and "
                           "the device context (hip_startup_ms: dpr_create on the helper thread = runtime start-up + code object load; "
                           "waits for the PREVIOUS process's teardown in the kernel driver when steps run back to back) are there -- "
                           "input_bound_by counts which side ended it per step; other = process start + Newick write + exit "
                           "(mostly the driver taking this process's GPU context apart)",
                   "tips_per_s_median": n / (float(np.median(walls)) * 1e-3) if walls else None,
                   "fasta_bytes": os.path.getsize(fa), "newick_bytes": os.path.getsize(nwk) if os.path.exists(nwk) else None}
            log(f"[bench r{rank}] CLI steps: {cli['wall_ms']}")
            # the same command with the GPU left alone for 0.4 s before every step: hip_startup_ms is then the process's OWN runtime
            # start-up (~105 ms), not the wait for its predecessor's teardown -- separates the command's cost from the artefact of
            # running steps back to back (round 5's verdict, item 8).  Untimed as far as `value` goes.
            if args.full and rank == 0 and args.steps > 0 and budget.allows(12):
                try:
                    iw, ii, it_, ir, ipar = [], [], [], [], []
                    for _ in range(min(args.steps, 5)):
                        dt, ph = cli_step(fa, nwk, local_rank, threads, idle_s=0.4)
                        iw.append(dt * 1e3); ii.append(ph.get("input", float("nan"))); it_.append(ph.get("tree", float("nan")))
                        ir.append(ph.get("device_ready", float("nan"))); ipar.append(ph.get("parsed", float("nan")))
                    cli["isolated"] = {"idle_before_each_step_ms": 400, "steps": len(iw), "wall_ms": stats_ms(iw), "input_ms": stats_ms(ii), "tree_ms": stats_ms(it_),
                                       "other_ms": stats_ms([w - i - t for w, i, t in zip(iw, ii, it_)]), "hip_startup_ms": stats_ms(ir), "parse_ms": stats_ms(ipar),
                                       "tips_per_s_median": n / (float(np.median(iw)) * 1e-3),
                                       "note": "not part of `value`: the timed steps above run back to back, as the contract asks"}
                except Exception as e:
                    cli["isolated"] = {"error": repr(e)}

        # =====================================================================================================
        # B. the hot path alone, in process through the C ABI: inputs resident in HBM -> distances -> NJ merge log
        #    (--full; in a plain run only when it is the headline, i.e. without the command)
        # =====================================================================================================
        dip, hot, last_res, prune, nj_ms = None, None, None, None, []
        if args.full or cli is None:
            dip = dipper_amd.Dipper(local_rank)
            dip.set_nj_multi_plan(2)        # timed steps: every rank builds its own tree (no collective at 30k tips)
            dip.set_msa(packed, L)          # H2D + bit-plane conversion: inputs now resident in HBM
            if rank == 0:
                log(f"[bench] device: {dip.device_name()}")

            def step():
                dip.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                res = dip.nj_run()
                assert res["iters"] == n - 2
                return res

            phase, walls_hp = [], []
            prune = None
            last_res = None
            for _ in range(args.warmup):
                step()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ts = time.perf_counter()
                last_res = step()
                walls_hp.append((time.perf_counter() - ts) * 1e3)
                phase.append(dip.timing())
                try:
                    sc, full = dip.prune_stats()
                    prune = {"units_scanned": sc, "units_per_full_scan": full, "iterations": n - 2,
                             "scanned_fraction_of_full_scans": sc / (full * (n - 2.0))}
                except Exception:
                    prune = None
            barrier()
            dt_hp = time.perf_counter() - t0
            if dist is not None:
                t = torch.tensor([dt_hp], dtype=torch.float64, device=TDEV)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt_hp = float(t.item())
            ms_hp = dt_hp / max(args.steps, 1) * 1e3 if args.steps else float("nan")
            nj_ms = [p[1] for p in phase]
            hot = {"metric": "tips/sec packed aligned tips resident in HBM -> JC69 distances -> NJ merge log (C ABI, in process)",
                   "value": world * n / (ms_hp * 1e-3) if args.steps else None, "unit": "tips/s", "ms_per_step": ms_hp,
                   "steps": args.steps, "warmup": args.warmup,
                   "step_ms": stats_ms(walls_hp),
                   "phase_ms": {"dist": stats_ms([p[0] for p in phase]), "nj": stats_ms(nj_ms)},
                   "nj_us_per_iteration": (float(np.median(nj_ms)) * 1e3 / (n - 2)) if nj_ms else None,
                   "nj_iterations_per_s": (world * (n - 2) / (float(np.median(nj_ms)) * 1e-3)) if nj_ms else None,
                   "nj_algorithm": "exact pruned scan (njp.hip)" if prune else "full streaming scan (nj.hip)",
                   "prune": prune}
            log(f"[bench r{rank}] hot path steps: {hot['step_ms']} phases {hot['phase_ms']}")
            if args.dump_outputs and rank == 0 and cli is None and last_res is not None:
                dump_outputs(args.dump_outputs, {k: last_res[k] for k in ("merge_x", "merge_y", "bl_x", "bl_y", "last_d")})
            if args.full and (args.model != "jc69" or not args.no_indel_gaps) and args.steps > 0 and not args.probe_only and n <= 50000:
                # the same hot path on the input of rounds 1-3 (JC69 substitutions, no gaps), for comparison across rounds:
                # one warm-up + two timed steps on a context of its own
                try:
                    inp3 = stage.gen("main_r3", n, L, args.seed, 2e-5, 2e-6, 2e-4, gap=None, model="jc69")
                    d3 = dipper_amd.Dipper(local_rank)
                    try:
                        d3.set_nj_multi_plan(2)
                        d3.set_msa(Stage.packed4(inp3), L)
                        ph3 = []
                        for k in range(3):
                            d3.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                            r3 = d3.nj_run()
                            if k:
                                ph3.append(d3.timing())
                        hot["rounds_1_to_3_input"] = {"input": "jc69, no gaps", "dist_ms": float(np.mean([p[0] for p in ph3])),
                                                      "nj_ms": float(np.mean([p[1] for p in ph3])), "units_scanned": d3.prune_stats()[0],
                                                      "merge_log_digest": merge_digest(r3)}
                    finally:
                        d3.close()
                except Exception as e:
                    hot["rounds_1_to_3_input"] = {"error": repr(e)}

            # ---- the timed kernels' own record: what the pruned scan read, and how fast ---------------------------
            if args.full and prune and nj_ms and not args.probe_only:
                try:
                    # one more NJ run, eager, HIP events on the library's stream around every 16th iteration's launches
                    dip.set_nj_kernel_timing(16)
                    dip.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                    dip.nj_run()
                    kt = dip.nj_kernel_timing()
                except Exception as e:
                    kt = {"error": repr(e)}
                finally:
                    dip.set_nj_kernel_timing(0)
                bytes_scanned = prune["units_scanned"] * float(UNIT_BYTES)
                rec = {"kernels_per_iteration": kt.get("kernels_per_iteration"),
                       "units_scanned_per_iteration": prune["units_scanned"] / (n - 2.0),
                       "bytes_scanned_per_run_upper": bytes_scanned,
                       "note": "bytes = listed units x 64 KiB (an upper bound: a listed unit's sub-units whose own bound rules "
                               "them out are not loaded); kernel times: HIP events on the library's stream around every "
                               "16th iteration's launches in one extra eager (not graph-replayed) run"}
                rec.update({k: v for k, v in kt.items() if k != "kernels_per_iteration"})
                if kt.get("scan_us_avg"):
                    # an event pair with nothing in between costs ~5 us on this stream: subtract it (the rocprofv3 averages of
                    # the same kernels, profiles/, are the reference these net figures have to agree with)
                    ev = kt.get("kernel_us_avg", {}).get("(empty event pair)", 0.0)
                    net = {k: max(v - ev, 0.0) for k, v in kt.get("kernel_us_avg", {}).items() if not k.startswith("(")}
                    rec["kernel_us_net_of_event_overhead"] = net
                    scan_net = max(kt["scan_us_avg"] - ev, 1e-3)
                    t_scan = scan_net * 1e-6 * (n - 2)
                    ach = bytes_scanned / t_scan / 1e9
                    rec["roofline_timed"] = {"bound": "latency (about 110 units = 7 MB per launch; HBM-bound only from ~100 000 tips on)",
                                             "kernel": kt.get("scan_kernel"),
                                             "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                                             "bytes_per_launch": bytes_scanned / (n - 2.0), "us_per_launch": scan_net}
                hot["timed_kernels"] = rec

        # =====================================================================================================
        # C. self-check of the timed result (untimed)
        # =====================================================================================================
        parity = None
        if args.full and last_res is not None and not args.no_parity and rank == 0:
            parity = {"merge_log_digest": merge_digest(last_res)}
            try:
                # (1) the streaming algorithm (the reference's: one full Q scan per iteration) on the bench's own input
                chk = dipper_amd.Dipper(local_rank)
                chk.set_nj_mode(0)
                chk.set_msa(packed, L)
                ts = time.perf_counter()
                chk.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                ref = chk.nj_run()
                parity["stream_equals_pruned"] = same_log(ref, last_res)
                parity["stream_run_s"] = time.perf_counter() - ts
                chk.close()
                del ref
            except Exception as e:
                parity["stream_equals_pruned"] = None
                parity["stream_error"] = repr(e)
            try:
                # (2) the CPU oracle on the leading tips of the same alignment: GPU distances -> oracle NJ vs GPU NJ
                from tests import _orc
                orc = _orc.load()
                m = min(n, 1500)
                chk = dipper_amd.Dipper(local_rank)
                chk.set_msa(np.ascontiguousarray(packed[:m]), L)
                chk.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                Dm = chk.matrix()
                got = chk.nj_run()
                want = orc.nj_run(np.tril(Dm, -1), threads=threads)
                parity["oracle_prefix_equal"] = same_log(want, got)
                parity["oracle_prefix_tips"] = m
                Dref = orc.msa_dist_lower(np.ascontiguousarray(packed[:m]), L, 2)
                lo = np.tril_indices(m, -1)
                parity["oracle_prefix_dist_max_rel"] = float(np.max(np.abs(Dm[lo] - Dref[lo]) / np.maximum(np.abs(Dref[lo]), 1e-300))) if m > 1 else 0.0
                chk.close()
            except Exception as e:
                parity["oracle_prefix_equal"] = None
                parity["oracle_error"] = repr(e)
            if cli is not None:
                try:
                    # (3) the Newick text the CLI writes for the unshuffled input (--seed -1; the timed runs shuffle the input
                    # order like the reference) == the Newick assembled from the in-process merge log
                    r = subprocess.run([EXE, "-i", "m", "-I", fa, "-O", nwk, "-m", "2", "-d", "2", "--device", str(local_rank),
                                        "--seed", "-1"], capture_output=True, text=True, env=dict(os.environ, DPR_HOST_THREADS=str(threads)))
                    txt = open(nwk).read()
                    mine = _util.newick_from_merges(names, last_res["merge_x"], last_res["merge_y"], last_res["bl_x"],
                                                    last_res["bl_y"], last_res["last_d"])
                    parity["cli_newick_equals_merge_log"] = bool(r.returncode == 0 and txt.strip() == mine.strip())
                    # (4) the reference authors' accuracy measure: normalised RF of the tree the CLI wrote against the tree the
                    # input was generated from (near-clonal data: most true branches carry no substitution at all)
                    parity["nrf_vs_generating_tree"] = nrf_of(inp["tree"], nwk, tmp, "main")
                except Exception as e:
                    parity["cli_newick_equals_merge_log"] = None
                    parity["cli_error"] = repr(e)
            log(f"[bench] parity_check: {parity}")

        # ---- several ranks: same merge log everywhere (every rank built the same tree from the same input) ----
        mgpu_check = None
        if args.full:
            log(f"[bench r{rank}] +{elapsed():.0f}s: multi-rank digest check / roofline probe")
        if args.full and dist is not None and last_res is not None:
            digest = int(merge_digest(last_res)[:14], 16)
            mine = torch.tensor([digest], dtype=torch.int64, device=TDEV)
            allh = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allh, mine)
            mgpu_check = {"ranks_agree": bool(all(int(t.item()) == digest for t in allh))}

        # =====================================================================================================
        # D. roofline of the Q-argmin (BASELINE metric 2): full streaming scan at n = N on a fresh matrix
        # =====================================================================================================
        roofline = None
        if args.full:
            dip.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
            _, _, _, scan_ms = dip.argmin_once(reps=args.probe_reps)
            alg_bytes = 4.0 * n * n + 4.0 * n       # strict lower triangle + U once (this rank holds the whole matrix)
            achieved = alg_bytes / (scan_ms * 1e-3) / 1e9
            roofline = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": achieved / HBM_PEAK_GBS, "traffic": pmc_traffic(n, 1),
                        "kernel": "nj_scan_kernel<PROBE=true,...>: the full Q-argmin scan (SURVEY 8d's unit of work; the streaming NJ "
                                  "path runs it every iteration, the default pruned path does not -- see hot_path.timed_kernels)",
                        "n_active": n, "algorithmic_bytes": alg_bytes, "ms": scan_ms}

        primary = cli is not None
        ms_per_step = (dt_cli / max(args.steps, 1) * 1e3) if primary else ms_hp
        out.update({
            "metric": "tips/sec FASTA->Newick at N=%d" % n if primary else hot["metric"],
            "value": world * n / (ms_per_step * 1e-3) if args.steps else None,
            "unit": "tips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (seeded Yule-Harding tree, %s, L=%d, %s; own native generator tools/gen_synth.cpp: no alisim in the image)"
                    % ("GTR+G4+I substitutions with the parameters of scripts/alisim.sh:21" if args.model == "gtr+g+i" else "JC69 substitutions", L, "no gaps" if args.no_indel_gaps else ("deletions of the authors' indel model as inherited gap runs (gen_synth --indel-gaps)"
                                                                 + ("; stress: + %.3g of every tip's cells as its own '-' runs" % args.gap_frac if args.gap_frac > 0 else ""))),
            "config": {"workload": "configs[1]: %d aligned tips, -d 2 (JC69), conventional NJ (-m 2)" % n,
                       "tips": n, "sites": L, "device": device,
                       "step": "one whole `dipper` command per rank (FASTA -> Newick)" if primary else "in-process hot path (HBM-resident input -> merge log)",
                       "parallelism": "1 GPU" if world == 1 else
                                      ("replicas%d: every rank builds its own %d-tip tree on its own GPU, no collective "
                                       "(an iteration of the default pruned NJ at this size is dependent latency, not bandwidth); value = %d x tips / step time. "
                                       "The row-sharded NJ loop is measured in nj_scaling, the 100 000-tip plans in sharded_100k" % (world, n, world))},
            "step_ms": cli["wall_ms"] if primary else hot["step_ms"],
            "e2e_cli": cli,
            "hot_path": hot,
            "phase_ms": {"dist": hot["phase_ms"]["dist"]["mean"] if hot["phase_ms"]["dist"] else None,
                         "nj": hot["phase_ms"]["nj"]["mean"] if hot["phase_ms"]["nj"] else None} if hot is not None else None,
            "roofline": roofline,
            "parity_check": parity,
            "input_staging": {"generated_once_by": "rank 0 (tools/bin/gen_synth, %d host threads)" % host_cores(), "seconds": dict(stage.times),
                              "directory": os.path.dirname(stage.dir), "host_threads_per_rank": threads},
        })
        if not args.full:           # what a plain run did not measure is left out of its line
            for k in ("hot_path", "phase_ms", "roofline", "parity_check"):
                if out[k] is None:
                    del out[k]
        if mgpu_check is not None:
            out["multi_gpu_check"] = mgpu_check

        # =====================================================================================================
        # E. CPU baselines (rank 0, one GPU): bounded samples on the GPU's own matrix
        # =====================================================================================================
        if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.probe_only:
            cores = threads
            for key, fn, kw, need in (("cpu_baseline", cpu_baseline, {"cores": cores}, 35),
                                      ("cpu_baseline_1core", cpu_baseline, {"cores": 1, "budget_s": 10.0}, 25),
                                      ("cpu_baseline_rapidnj", cpu_baseline_rapidnj, {"cores": cores}, 45)):
                if not budget.allows(need):
                    out[key] = dict(budget.skip(need), value=None, unit="tips/s", cores=kw.get("cores"), kind="port", sample="skipped")
                    continue
                try:
                    out[key] = fn(dip, n, **kw)
                except Exception as e:  # a baseline must never take the bench line down
                    out[key] = {"value": None, "unit": "tips/s", "cores": kw.get("cores"), "kind": "port", "sample": f"failed: {e!r}"}
            try:
                out["rapidnj_path_probe"] = rapidnj_probe(dip, n, cores, tmp)
            except Exception as e:
                out["rapidnj_path_probe"] = {"found": None, "error": repr(e)}
        if dip is not None:
            dip.close()
            dip = None

        # =====================================================================================================
        # E2. north_star's partitioning on this run's GPUs: matrix row-sharded over the ranks, one full Q scan per
        #     iteration (streaming NJ) -- NJ iterations/s per exchange plan, next to one GPU alone and to the default plan
        # =====================================================================================================
        if args.full:
            log(f"[bench r{rank}] +{elapsed():.0f}s: nj_scaling")
        if args.full and not args.probe_only and not args.no_stream_leg:
            need = 25 + (0 if args.no_virtual_pruned else 45) + (12 * len(args.exchanges.split(",")) + 40 if world > 1 else 0)
            if budget.allows_all(need):
                try:
                    out["nj_scaling"] = nj_scaling(args, rank, world, local_rank, dist, torch, barrier, packed, n, L, args.stream_iters,
                                                   hot.get("nj_iterations_per_s"), budget, merge_digest(last_res) if last_res is not None else None)
                except Exception as e:
                    out["nj_scaling"] = {"error": repr(e)}
            else:
                out["nj_scaling"] = budget.skip(need)

        # =====================================================================================================
        # E3. north_star's other sizes, one run each on this GPU (rank 0 of a single-GPU run; no warm-up: first-touch of
        #     the buffers is inside the figures): NJ at 100 000 tips, k-closest placement of 100 000 unaligned tips (Mash),
        #     divide-and-conquer of 1 000 000 aligned tips
        # =====================================================================================================
        if args.full and world == 1 and rank == 0 and not args.no_other_configs and not args.probe_only:
            try:
                out["other_configs"] = other_configs(args, local_rank, stage, budget, tmp)
            except Exception as e:
                out["other_configs"] = {"error": repr(e)}

        # =====================================================================================================
        # F. several GPUs: 100 000 tips (80 GB matrix): unit-sharded pruned plan, row-sharded streaming plans, DC of 1 M tips
        # =====================================================================================================
        if args.full:
            log(f"[bench r{rank}] +{elapsed():.0f}s: other sizes")
        run_sharded = world > 1 or force_check
        if args.full and run_sharded and not args.no_sharded and not args.probe_only:
            try:
                out["sharded_100k"] = sharded_leg(args, rank, world, local_rank, dist, torch, barrier, stage, budget)
            except Exception as e:
                out["sharded_100k"] = {"error": repr(e)}
        # F2. the product's own multi-GPU boundary: the `dipper` command with one rank per GPU (configs[1]-[4]) next to one GPU
        if args.full and run_sharded and not args.probe_only and not args.no_cli and os.path.exists(EXE):
            try:
                out["cli_ranks"] = cli_ranks_leg(args, rank, world, local_rank, dist if world > 1 else None, stage, budget, tmp, fa if want_cli else None)
            except Exception as e:
                out["cli_ranks"] = {"error": repr(e)}
        out["bench_wall_s"] = round(elapsed(), 1)
        try:
            out = with_scaling_summary(out, world)
        except Exception as e:
            out["nj_iteration_scaling"] = {"error": repr(e)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        try:
            stage.sync()          # (still under the watchdog: a rank that died leaves the others here)
        except Exception:
            pass
        dog.cancel()
        faulthandler.cancel_dump_traceback_later()
        stage.cleanup()
    if rank == 0:
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if dist is not None:
        dist.destroy_process_group()


def other_configs(args, local_rank, stage, budget, tmp):
    """BASELINE.json configs[2] / configs[3] and north_star's N = 100 000 NJ, one run each (synthetic inputs as everywhere:
    seeded Yule tree, JC69; unaligned reads with seeded indels).  Every record: tips, seconds of the timed part, tips/s, and
    the normalised RF of the result against the generating tree."""
    import dipper_amd
    from dipper_amd import capi
    from tests import _util
    rec = {}

    def leg(name, fn, need):
        if not budget.allows(need):
            rec[name] = budget.skip(need)
            return
        t0 = time.perf_counter()
        try:
            rec[name] = fn()
        except Exception as e:       # one failing leg must not take the others (or the line) down
            rec[name] = {"error": repr(e)}
        rec[name]["leg_wall_s"] = time.perf_counter() - t0
        log(f"[bench] other_configs.{name}: {rec[name]}")

    def nj_100k():
        n, L = 100000, 10000
        inp = stage.gen("nj100k", n, L, args.seed + 7, 2e-5, 2e-6, 2e-4, gap=None if args.no_indel_gaps else args.gap_frac)
        packed = Stage.packed4(inp)
        d = dipper_amd.Dipper(local_rank)
        try:
            d.reserve_nj(n)          # the two 80 GB buffers (the CLI allocates them on its device thread while it parses the input)
            d.set_msa(packed, L)
            t0 = time.perf_counter()
            d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
            res = d.nj_run()
            wall = time.perf_counter() - t0
            dist_ms, nj_ms = d.timing()
            sc, _ = d.prune_stats()
            out = {"workload": "conventional NJ, %d aligned tips x %d sites, JC69 (80 GB matrix on one GPU), packed tips in HBM -> merge log" % (n, L),
                   "tips": n, "seconds": wall, "tips_per_s": n / wall, "dist_ms": dist_ms, "nj_ms": nj_ms,
                   "nj_iterations_per_s": res["iters"] / (nj_ms * 1e-3), "units_scanned": sc, "merge_log_digest": merge_digest(res)}
            out["input"] = "%s, %s" % (args.model, "no gaps" if args.no_indel_gaps else "inherited deletion gaps")
            if budget.allows(25):
                # the driver-run record carries a CHECK at this size, not only a digest: the first 256 iterations of the streaming loop
                # (the reference's algorithm: one full Q scan per iteration, src/neighborJoining.cu:117-148) on the same matrix
                # against the pruned run's log (whose first epoch runs the large launch shape, njp_post2_kernel<4>)
                k = 256
                d.set_nj_mode(0)
                try:
                    d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                    rs = d.nj_run(max_iters=k)
                    out["stream_prefix_equal"] = bool(rs["iters"] == k and all(np.array_equal(rs[key][:k], res[key][:k]) for key in ("merge_x", "merge_y", "bl_x", "bl_y")))
                    out["stream_prefix"] = {"iterations": int(rs["iters"]), "stream_ms": d.timing()[1]}
                finally:
                    d.set_nj_mode(1)
            if (args.model != "jc69" or not args.no_indel_gaps) and budget.allows(40):
                # the same size on the input of rounds 1-3 (JC69, gap-free), for comparison across rounds
                inp3 = stage.gen("nj100k_r3", n, L, args.seed + 7, 2e-5, 2e-6, 2e-4, gap=None, model="jc69")
                d.set_msa(Stage.packed4(inp3), L)
                d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
                res3 = d.nj_run()
                out["rounds_1_to_3_input"] = {"input": "jc69, no gaps", "dist_ms": d.timing()[0], "nj_ms": d.timing()[1], "units_scanned": d.prune_stats()[0],
                                              "merge_log_digest": merge_digest(res3)}
        finally:
            d.close()
        if budget.allows(20):
            names = ["T%d" % (i + 1) for i in range(n)]
            out["nrf_vs_generating_tree"] = nrf_of(inp["tree"], _util.newick_from_merges(names, res["merge_x"], res["merge_y"], res["bl_x"],
                                                                                       res["bl_y"], res["last_d"], fmt=repr), tmp, "nj100k")
        return out

    def place_100k_unaligned(L=3000):
        n = 100000
        inp = stage.gen("reads100k_%d" % L, n, L, args.seed + 8, 2e-5, 2e-6, 2e-4, reads=True)
        flat, off, lens = Stage.reads(inp)
        d = dipper_amd.Dipper(local_rank)
        try:
            d.set_reads_packed(flat, off, lens)
            t0 = time.perf_counter()
            d.sketch(15, 1000, fetch=False)
            t1 = time.perf_counter()
            st = d.place_run(capi.SRC_MASH, n, k=15)
            wall = time.perf_counter() - t0
            dist_ms, tree_ms = d.place_timing()
            overlapped, busy_ms = d.place_overlap()
            out = {"workload": "configs[2]: %d unaligned tips x ~%d bases, Mash sketches (k 15, 1000 values) + k-closest placement, reads in HBM -> tree arrays" % (n, L),
                   "tips": n, "bases": L, "protocol_length": L >= 10000, "seconds": wall, "tips_per_s": n / wall, "sketch_s": t1 - t0,
                   "distance_wait_ms": dist_ms, "tree_part_ms": tree_ms, "distance_batches_overlapped": overlapped, "distance_busy_ms": busy_ms,
                   "trace_digest": hashlib.sha256(np.ascontiguousarray(st["trace"]).tobytes()).hexdigest()[:16]}
        finally:
            d.close()
        if budget.allows(20):
            names = ["T%d" % (i + 1) for i in range(n)]
            out["nrf_vs_generating_tree"] = nrf_of(inp["tree"], _util.newick_from_placement(names, st["head"], st["e"], st["nxt"], st["len"], n, fmt=repr), tmp, "place100k")
        stage.drop(inp)
        return out

    def dc_1m(L=400):
        n = args.dc_tips
        # (400 sites: the branch lengths of rounds 2-5 -- 25 x the protocol's -- so that 400 sites carry the signal 10 000 do at the
        #  protocol's; 10 000 sites: the protocol's own lengths x 10, the divergence of a 1 M-tip tree the authors' own runs have)
        inp = stage.gen("dc1m" if L == 400 else "dc1m_%d" % L, n, L, args.seed + 9, 2e-3 if L == 400 else 2e-4, 2e-4 if L == 400 else 2e-5, 2e-2 if L == 400 else 2e-3,
                        shuffle=7, gap=None if args.no_indel_gaps else args.gap_frac)   # the CLI shuffles its input (src/tree_generation.cu:341-344)
        packed = Stage.packed4(inp)
        d = dipper_amd.Dipper(local_rank)
        try:
            d.set_msa(packed, L)
            t0 = time.perf_counter()
            st = d.dc_run(capi.SRC_MSA, n, n // 20, dist_type=capi.DIST_JC)
            wall = time.perf_counter() - t0
            out = {"workload": "configs[3] on one GPU: divide-and-conquer, %d aligned tips x %d sites, backbone %d, packed tips in HBM -> tree arrays" % (n, L, n // 20),
                   "tips": n, "sites": L, "protocol_length": L >= 10000, "seconds": wall, "tips_per_s": n / wall,
                   "device_s": (st["stats"]["backbone_ms"] + st["stats"]["assign_ms"] + st["stats"]["cluster_ms"]) * 1e-3,
                   "note": "seconds includes copying the tree arrays and closest lists (0.5 GB) back to the host",
                   "stats": {k: (float(v) if isinstance(v, float) else int(v)) for k, v in st["stats"].items()}}
        finally:
            d.close()
        if budget.allows(60):
            order = np.fromfile(inp["order"], dtype=np.int32)
            names = ["T%d" % (k + 1) for k in order]
            out["nrf_vs_generating_tree"] = nrf_of(inp["tree"], _util.newick_from_placement(names, st["head"], st["e"], st["nxt"], st["len"], n, fmt=repr), tmp, "dc1m")
        del packed
        if L != 400:
            stage.drop(inp)          # (5 GB of packed tips; the 400-site input is kept for the multi-rank leg)
        return out

    def add_onto_backbone(kind, L=None, m=None, nq=None):
        """BASELINE configs[4]: 50 000 queries added to a 500 000-tip backbone (src/placement_close_k.cu:858-990 addQuery,
        :126-264 initializeDeviceArrays) through the `dipper` command itself -- the backbone tree is the command's own
        divide-and-conquer tree of the first 500 000 records (untimed set-up), the timed step is
        `dipper -a -t backbone.nwk -I all.fa`.  kind "m": aligned input (-i m -d 2), "r": unaligned reads through Mash (-i r)."""
        m, nq = m or args.add_backbone, nq or args.add_queries
        n = m + nq
        L = L or (1000 if kind == "m" else 3000)
        scale = 1000.0 / L if kind == "m" else 1.0      # (aligned: the same expected substitutions per branch at every length)
        inp = stage.gen("add_%s_%d_%d" % (kind, L, n), n, L, args.seed + (10 if kind == "m" else 11), 1e-3 * scale, 1e-4 * scale, 1e-2 * scale, fasta=True, reads=(kind == "r"), shuffle=7,
                        gap=(None if args.no_indel_gaps else args.gap_frac) if kind == "m" else None)
        fa_all = inp["fasta"]
        # the first m records as their own file (the backbone's tips)
        buf = np.memmap(fa_all, dtype=np.uint8, mode="r")
        starts = np.flatnonzero(buf == ord(">"))
        cut = int(starts[m])
        fa_bb = os.path.join(tmp, "bb_%s.fa" % kind)
        with open(fa_bb, "wb") as f:
            f.write(buf[:cut].tobytes())
        del buf, starts
        bb_nwk, out_nwk = os.path.join(tmp, "bb_%s.nwk" % kind), os.path.join(tmp, "add_%s.nwk" % kind)
        env = dict(os.environ, DPR_HOST_THREADS=str(host_cores()))
        fmt = ["-i", kind] + (["-d", "2"] if kind == "m" else [])
        t0 = time.perf_counter()
        r = subprocess.run([EXE] + fmt + ["-m", "3", "-I", fa_bb, "-O", bb_nwk, "--device", str(local_rank)], capture_output=True, text=True, env=env)
        t_bb = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("dipper (backbone) failed: " + r.stderr[-300:])
        t0 = time.perf_counter()
        r = subprocess.run([EXE] + fmt + ["-a", "-t", bb_nwk, "-I", fa_all, "-O", out_nwk, "--device", str(local_rank)], capture_output=True, text=True, env=env)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("dipper --add failed: " + r.stderr[-300:])
        ph = cli_phases(r.stderr)
        out = {"workload": "configs[4] on one GPU: %d queries added to a %d-tip backbone, %s; the whole `dipper -a -t backbone.nwk` command "
                           "(FASTA of all %d records in, Newick out)" % (nq, m, "aligned x %d sites, -d 2" % L if kind == "m" else "unaligned reads x ~%d bases through Mash" % L, n),
               "backbone": m, "queries": nq, ("sites" if kind == "m" else "bases"): L, "protocol_length": L >= 10000, "seconds": wall, "queries_per_s": nq / wall, "phases_ms": ph,
               "addquery_s": (ph["distance_ms"] + ph["tree_op_ms"]) * 1e-3 if ("distance_ms" in ph and "tree_op_ms" in ph) else None,
               "note": "seconds = the whole command (FASTA parse of all records, packing, sketches, backbone import, addQuery, Newick write); addquery_s = the "
                       "command's own `Distance Operation Time` + `Tree Operation Time` lines (src/placement_close_k.cu:985-986)",
               "setup_untimed": {"backbone_tree_by_dc_s": t_bb, "fasta_bytes": os.path.getsize(fa_all)}}
        for f in (fa_bb,):
            try:
                os.unlink(f)
            except OSError:
                pass
        if budget.allows(40):
            out["nrf_vs_generating_tree"] = nrf_of(inp["tree"], out_nwk, tmp, "add_%s" % kind)
        for f in (bb_nwk, out_nwk):
            try:
                os.unlink(f)
            except OSError:
                pass
        stage.drop(inp)
        return out

    def exact_30k():
        # the exact placement mode (src/placement.cu:508-789), every tip against every edge of the growing tree
        n, L = 30000, 2000
        inp = stage.gen("exact30k", n, L, args.seed + 11, 1e-3, 1e-4, 1e-2, shuffle=7)
        d = dipper_amd.Dipper(local_rank)
        try:
            d.set_msa(Stage.packed4(inp), L)
            t0 = time.perf_counter()
            st = d.place_exact_run(capi.SRC_MSA, n, dist_type=capi.DIST_JC)
            wall = time.perf_counter() - t0
            out = {"workload": "exact placement, %d aligned tips x %d sites in random order, -d 2, packed tips in HBM -> tree arrays" % (n, L),
                   "tips": n, "sites": L, "seconds": wall, "tips_per_s": n / wall, "us_per_tip": wall / n * 1e6,
                   "max_depth": int(st["dep"][:2 * n - 1].max()),
                   "trace_digest": hashlib.sha256(np.ascontiguousarray(st["trace"]).tobytes()).hexdigest()[:16]}
        finally:
            d.close()
        stage.drop(inp)
        return out

    # keys carry the sequence length: the authors' protocol is 10 000 sites for every size (scripts/experiment.sh:14,
    # scripts/alisim.sh:14); the short inputs of rounds 2-5 stay beside the protocol-length ones
    leg("nj_100k_10000_sites", nj_100k, 30)
    leg("place_100k_unaligned_3000_bases", place_100k_unaligned, 25)
    leg("dc_1m_400_sites", dc_1m, 30)
    leg("place_exact_30k_2000_sites", exact_30k, 10)
    if not args.no_add_leg:
        leg("add_50k_onto_500k_aligned_1000_sites", lambda: add_onto_backbone("m"), 45)
        leg("add_50k_onto_500k_mash_3000_bases", lambda: add_onto_backbone("r"), 75)
    if not args.no_protocol_length:
        leg("place_100k_unaligned_10000_bases", lambda: place_100k_unaligned(10000), 40)
        if stage.room_for(12 << 30):
            leg("dc_1m_10000_sites", lambda: dc_1m(10000), 90)
        else:
            rec["dc_1m_10000_sites"] = {"skipped": "less than 12 GB of staging space for the 5 GB of packed tips"}
        if not args.no_add_leg:
            if stage.room_for(16 << 30) and budget.allows(150):
                leg("add_50k_onto_500k_aligned_10000_sites", lambda: add_onto_backbone("m", L=10000), 150)
            else:
                # (the 5.5 GB FASTA + 2.8 GB of packed tips, or the time, are not there: a size that fits, said so in the key)
                leg("add_20k_onto_200k_aligned_10000_sites", lambda: add_onto_backbone("m", L=10000, m=200000, nq=20000), 70)
    return rec


PLAN_ID = {"legacy": 0, "peer": 1, "mailbox": 2}
PRUNED_PLAN_ID = {"collective": 1, "mailbox": 2}      # exchange plans of the row-sharded pruned NJ (njr.hip)

# DPR_BENCH_ONE_GPU=1: rehearsal of the N > 1 control flow with N PROCESSES ON ONE GPU (a single-GPU box is all the builder
# has): torch.distributed over gloo, every rank on device 0, the library's ranks joined WITHOUT RCCL (dpr_comm_init_local +
# hipIpc windows; RCCL refuses two ranks on one device) -- so only the mailbox plan of the row-sharded loop runs and the
# legs that need RCCL collectives (unit-sharded pruned NJ, multi-rank divide-and-conquer) say so instead.
ONE_GPU = os.environ.get("DPR_BENCH_ONE_GPU") == "1"
TDEV = "cpu" if ONE_GPU else "cuda"


def streaming_run(d, torch, dist, barrier, packed, n, L, iters, timed_world):
    """`iters` iterations of the streaming NJ on an already configured context; returns (result, record)"""
    from dipper_amd import capi
    d.set_nj_mode(0)
    d.set_msa(packed, L)
    d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    log(f"[bench] +{elapsed():.0f}s: streaming run: matrix built, plan {d.nj_exchange_info()['plan'] if timed_world > 1 else 'single rank'}")
    d.nj_run(max_iters=8)           # warm-up: first launches / communicator channels
    d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
    if timed_world > 1:
        barrier()
    else:
        torch.cuda.synchronize()
    ts = time.perf_counter()
    res = d.nj_run(max_iters=iters)
    if timed_world > 1:
        barrier()
    wall = time.perf_counter() - ts
    _, loop_ms = d.timing()
    if timed_world > 1:
        t = torch.tensor([wall, loop_ms], dtype=torch.float64, device=TDEV)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall, loop_ms = float(t[0].item()), float(t[1].item())
    info = d.nj_exchange_info() if timed_world > 1 else {"launches": 2 * int(res["iters"]), "collectives": 0, "plan": "single rank", "note": ""}
    return res, stream_record(n, int(res["iters"]), loop_ms, wall, info, timed_world, merge_digest(res))


def with_scaling_summary(out, world):
    """north_star's scaling metric in ONE small object placed right behind `roofline` (so a truncated record still carries
    it): NJ iterations per second of the streaming loop on one GPU, of the default plan on one GPU, and of the row-sharded loop
    per exchange plan on this run's ranks, with what joined the ranks.  The top-level `scaling` key stays the contract's string."""
    njs = out.get("nj_scaling")
    if not isinstance(njs, dict) or "tips" not in njs:
        return out
    comp = {"tips": njs.get("tips"), "iterations_timed": njs.get("iterations_timed"), "n_gpus": world,
            "streaming_one_gpu_its_per_s": (njs.get("streaming_one_gpu") or {}).get("nj_iterations_per_s"),
            "default_plan_one_gpu_its_per_s": (njs.get("default_plan_one_gpu") or {}).get("nj_iterations_per_s"),
            "row_sharded": {}}
    for plan, r in (njs.get("row_sharded") or {}).items():
        if not isinstance(r, dict):
            continue
        if "nj_iterations_per_s" in r:
            comp["row_sharded"][plan] = {"its_per_s": r.get("nj_iterations_per_s"), "speedup_vs_streaming_one_gpu": r.get("iteration_speedup_vs_one_gpu"),
                                         "ranks": r.get("ranks"), "rccl": r.get("rccl"), "matches_single_gpu": r.get("matches_single_gpu"),
                                         "launches_per_iteration": r.get("launches_per_iteration"), "collectives_per_iteration": r.get("collectives_per_iteration")}
        else:
            comp["row_sharded"][plan] = {k: r[k] for k in ("skipped", "error") if k in r}
    comp["row_sharded_pruned"] = {}
    for plan, r in (njs.get("row_sharded_pruned") or {}).items():
        if isinstance(r, dict):
            comp["row_sharded_pruned"][plan] = ({"its_per_s": r.get("nj_iterations_per_s"), "ranks": r.get("ranks"), "rccl": r.get("rccl"),
                                                 "matches_single_gpu": r.get("matches_single_gpu"), "speedup_vs_streaming_one_gpu": r.get("iteration_speedup_vs_streaming_one_gpu"),
                                                 "speedup_vs_default_plan_one_gpu": r.get("iteration_speedup_vs_default_plan_one_gpu"),
                                                 "launches_per_iteration": r.get("launches_per_iteration"), "collectives_per_iteration": r.get("collectives_per_iteration")}
                                                if "nj_iterations_per_s" in r else {k: r[k] for k in ("skipped", "error") if k in r})
    v = njs.get("row_sharded_pruned_virtual")
    if isinstance(v, dict):
        comp["row_sharded_pruned_8_virtual_ranks_one_gpu"] = {plan: ({"per_rank_iteration_us": r.get("per_rank_iteration_us"), "per_rank_kernel_us": r.get("per_rank_kernel_us"),
                                                                      "matches_single_gpu": r.get("matches_single_gpu")} if isinstance(r, dict) and "per_rank_iteration_us" in r else r)
                                                              for plan, r in v.items() if plan in ("mailbox", "collective")}
    new = {}
    for k, v in out.items():
        new[k] = v
        if k == "roofline":
            new["nj_iteration_scaling"] = comp
    if "nj_iteration_scaling" not in new:
        new["nj_iteration_scaling"] = comp
    return new


def stream_record(n, iters, loop_ms, wall, info, timed_world, digest):
    k = max(int(iters), 1)
    # algorithmic bytes of iteration k: strict lower triangle of the n-k active rows, 8 bytes per element, read
    # once, + the row sums -- what the single-GPU roofline record counts (4 n^2 + 4 n)
    by = sum(4.0 * (n - j) * (n - j) + 4.0 * (n - j) for j in range(k))
    rec = {"iterations": int(iters), "wall_s": wall, "loop_ms_hip_events": loop_ms,
           "us_per_iteration": loop_ms * 1e3 / k, "nj_iterations_per_s": k / (loop_ms * 1e-3),
           "aggregate_GBps": by / (loop_ms * 1e-3) / 1e9, "peak_GBps": HBM_PEAK_GBS * timed_world,
           "frac_of_aggregate_peak": by / (loop_ms * 1e-3) / 1e9 / (HBM_PEAK_GBS * timed_world),
           "launches_per_iteration": info["launches"] / k, "collectives_per_iteration": info["collectives"] / k,
           "merge_log_digest": digest}
    if timed_world > 1:
        rec["exchange_plan_active"] = info["plan"]
        if info.get("note"):
            rec["exchange_note"] = info["note"]
    return rec


# ---------------------------------------------------------------------------------------------------------
# the row-sharded legs run in one CHILD PROCESS per rank that never imports torch
# ---------------------------------------------------------------------------------------------------------
# Why: a process that imports torch runs this library on the HIP runtime bundled with the wheel (7.0.51831 here), and that
# runtime does not return from hipIpcOpenMemHandle for allocations of 2^31 .. 2^32 bytes (profiles/r3/ipc_runtime_probe.txt) --
# a rank's rows of a 100 000-tip matrix are 10 - 40 GB.  The library refuses such mappings on that runtime (legacy loop), so
# the one-exchange plans would never be measured from inside this process.  The product (the `dipper` command, any C++ host)
# links the system runtime (7.2), where they map; a child without torch is that configuration.  It also keeps a hang of
# the one path that has never met a second GPU away from the benchmark's own process: the parent waits with a timeout
# and kills the child.  Parent and child talk in JSON lines over the child's stdin / stdout; the parents carry the RCCL id
# (or, ranks on one GPU: the 192-byte peer descriptions) between the children with torch.distributed.
def njs_worker():
    cfg = json.loads(sys.argv[2])
    out_fd = os.dup(1)
    os.dup2(2, 1)           # (RCCL prints its banner on fd 1)

    def say(obj):
        os.write(out_fd, (json.dumps(obj) + "\n").encode())

    def hear():
        line = sys.stdin.readline()
        if not line:
            os._exit(4)     # parent gone
        return json.loads(line)

    try:
        import ctypes
        import dipper_amd
        from dipper_amd import capi
        rank, world, n, L, iters = cfg["rank"], cfg["world"], cfg["tips"], cfg["sites"], cfg["iters"]
        packed = np.memmap(cfg["p4"], dtype=np.uint64, mode="r", shape=(n, (L + 15) // 16))
        d = dipper_amd.Dipper(cfg["device"])
        pruned_rows = cfg.get("algo") == "pruned_rows"      # the row-sharded exact PRUNED NJ (njr.hip) instead of the streaming loop
        try:
            if pruned_rows:
                d.set_nj_mode(1)
                d.set_nj_multi_plan(3)
            else:
                d.set_nj_mode(0)
            if cfg["local"]:
                d.comm_init_local(rank, world)
                say({"blob": d.peer_export(n).hex()})
                d.peer_attach([bytes.fromhex(b) for b in hear()["blobs"]])
                ranks = world
            else:
                if rank == 0:
                    say({"uid": bytes(d.comm_unique_id()).hex()})
                d.comm_init(rank, world, bytes.fromhex(hear()["uid"]))
                ranks = d.comm_info()[1]
            d.set_nj_exchange(PRUNED_PLAN_ID[cfg["plan"]] if pruned_rows else PLAN_ID[cfg["plan"]])
            d.set_msa(packed, L)
            d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
            d.nj_run(max_iters=8)           # warm-up: first launches / communicator channels
            d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
            ver = ctypes.c_int(0)
            for line in open("/proc/self/maps"):
                if "libamdhip64" in line:
                    ctypes.CDLL(line.split()[-1]).hipRuntimeGetVersion(ctypes.byref(ver))
                    break
            say({"ready": 1, "plan": d.nj_exchange_info()["plan"], "hip_runtime": ver.value, "torch_loaded": "torch" in sys.modules})
            hear()                          # go
            ts = time.perf_counter()
            res = d.nj_run(max_iters=iters)
            wall = time.perf_counter() - ts
            _, loop_ms = d.timing()
            info = d.nj_exchange_info()
            say({"result": {"iters": int(res["iters"]), "wall_s": wall, "loop_ms": loop_ms, "launches": info["launches"], "collectives": info["collectives"],
                            "plan": info["plan"], "note": info["note"], "digest": merge_digest(res), "ranks": ranks,
                            "rccl": not cfg["local"]}})
        finally:
            d.close()
    except BaseException as e:      # every failure is a line the parent can read (DPR_ERR_COMM when a mailbox poll ran out, ...)
        say({"error": repr(e)[:400]})
        os._exit(1)
    os._exit(0)


class Child:
    def __init__(self, cfg):
        import queue
        self.q = queue.Queue()
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--njs-worker", json.dumps(cfg)], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, cwd=ROOT)
        t = threading.Thread(target=self._pump, daemon=True)
        t.start()

    def _pump(self):
        for line in self.p.stdout:
            try:
                self.q.put(json.loads(line))
            except Exception:
                pass
        self.q.put(None)            # end of file

    def get(self, timeout_s):
        """next message of the child; {"error": ...} when it said nothing in time or ended"""
        import queue
        try:
            m = self.q.get(timeout=max(1.0, timeout_s))
        except queue.Empty:
            return {"error": "child said nothing for %d s (killed)" % int(timeout_s)}
        return m if m is not None else {"error": "child ended (exit code %s)" % self.p.poll()}

    def put(self, obj):
        try:
            self.p.stdin.write(json.dumps(obj) + "\n")
            self.p.stdin.flush()
        except Exception:
            pass

    def close(self):
        if self.p.poll() is None:
            try:
                self.p.wait(timeout=5)
            except Exception:
                self.p.kill()       # this exact process
                self.p.wait()


def njs_child_leg(plan, rank, world, local_rank, dist, torch, p4, n, L, iters, setup_s, run_s, algo="stream"):
    """one exchange plan of the row-sharded loop in a child per rank; every rank returns the same verdict, rank 0 the record"""
    def everyone(flag):
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=TDEV)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(int(t.item()))

    ch = Child({"rank": rank, "world": world, "device": local_rank, "tips": n, "sites": L, "iters": iters, "p4": p4, "plan": plan, "local": ONE_GPU, "algo": algo})
    try:
        if ONE_GPU:
            m = ch.get(setup_s)
            blobs = [None] * world
            dist.all_gather_object(blobs, m.get("blob"))
            if any(b is None for b in blobs):
                return {"error": "peer description missing: " + str(m.get("error"))}
            ch.put({"blobs": blobs})
        else:
            uid = [None]
            if rank == 0:
                uid[0] = ch.get(setup_s).get("uid")
            dist.broadcast_object_list(uid, src=0)
            if uid[0] is None:
                return {"error": "rank 0's child made no communicator id"}
            ch.put({"uid": uid[0]})
        m = ch.get(setup_s)
        if not everyone("ready" in m):
            return {"error": m.get("error", "another rank did not get ready")}
        ready = m
        ch.put({"go": 1})
        m = ch.get(run_s)
        if not everyone("result" in m):
            return {"error": m.get("error", "another rank failed")}
        mine = m["result"]
        allr = [None] * world
        dist.all_gather_object(allr, mine)
        loop_ms = max(r["loop_ms"] for r in allr)
        wall = max(r["wall_s"] for r in allr)
        if algo == "pruned_rows":
            k = max(int(mine["iters"]), 1)
            rec = {"iterations": int(mine["iters"]), "wall_s": wall, "loop_ms_hip_events": loop_ms, "us_per_iteration": loop_ms * 1e3 / k,
                   "nj_iterations_per_s": k / (loop_ms * 1e-3), "launches_per_iteration": mine["launches"] / k,
                   "collectives_per_iteration": mine["collectives"] / k, "merge_log_digest": mine["digest"], "exchange_plan": plan}
        else:
            rec = stream_record(n, mine["iters"], loop_ms, wall, mine, world, mine["digest"])
        # `ranks` = processes that took part; `rccl` says whether an RCCL communicator joined them (process ranks on ONE GPU are
        # joined through hipIpc windows only) -- a run without RCCL is never reported as rccl_ranks
        rec["ranks"] = mine["ranks"]
        rec["rccl"] = bool(mine.get("rccl"))
        if rec["rccl"]:
            rec["rccl_ranks"] = mine["ranks"]
        rec["ranks_agree"] = len({r["digest"] for r in allr}) == 1 and len({r["iters"] for r in allr}) == 1
        rec["child_process"] = {"hip_runtime": ready.get("hip_runtime"), "torch_loaded": ready.get("torch_loaded")}
        return rec
    finally:
        ch.close()


def row_sharded_pruned_virtual(local_rank, packed, n, L, vworld, solo_digest, budget):
    """The row-sharded exact pruned NJ (njr.hip) with `vworld` VIRTUAL ranks on this one GPU: every rank holds only its chunks of
    the position-space rows, its own vectors, lists and window; the whole NJ runs, its merge log is checked against the
    single-GPU run, and the launches of ONE rank are bracketed by HIP events every 16th iteration -- the per-rank iteration time a
    real rank would see without its exchange (the other ranks' launches serialise behind it on the one stream here)."""
    import dipper_amd
    from dipper_amd import capi
    out = {"virtual_ranks": vworld, "tips": n, "sites": L,
           "what": "whole NJ run, rows of the position-space matrix dealt to the ranks in chunks of 1 024; per-rank kernel times = HIP events around rank 0's "
                   "three launches of every 16th iteration (eager launches; all ranks share this GPU, so wall time is NOT a multi-GPU figure)"}
    for plan in ("mailbox", "collective"):
        if budget is not None and not budget.allows(25):
            out[plan] = budget.skip(25)
            continue
        d = dipper_amd.Dipper(local_rank, virtual_world=vworld)
        try:
            d.set_nj_mode(1)
            d.set_nj_multi_plan(3)
            d.set_nj_exchange(PRUNED_PLAN_ID[plan])
            d.set_nj_kernel_timing(16)
            d.set_msa(packed, L)
            t0 = time.perf_counter()
            d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
            t1 = time.perf_counter()
            res = d.nj_run()
            wall = time.perf_counter() - t1
            kt = d.nj_kernel_timing()
            info = d.nj_exchange_info()
            per_rank = {k: v for k, v in kt["kernel_us_avg"].items() if not k.startswith("(")}
            out[plan] = {"iterations": int(res["iters"]), "matches_single_gpu": (merge_digest(res) == solo_digest) if solo_digest else None,
                         "merge_log_digest": merge_digest(res), "per_rank_kernel_us": per_rank, "per_rank_iteration_us": sum(per_rank.values()),
                         "sampled_iterations": kt["sampled_iterations"], "launches_per_iteration_per_rank": 3,
                         "collectives_per_iteration": info["collectives"] / max(int(res["iters"]), 1),
                         "build_s_all_ranks_on_one_gpu": t1 - t0, "nj_wall_s_all_ranks_on_one_gpu": wall}
        except Exception as e:
            out[plan] = {"error": repr(e)}
        finally:
            d.close()
    return out


def nj_scaling(args, rank, world, local_rank, dist, torch, barrier, packed, n, L, iters, solo_pruned_its, budget=None, solo_pruned_digest=None):
    """NJ-iteration throughput side by side (north_star's scaling metric): the default plan on one GPU (exact pruned scan),
    the streaming loop (the reference's algorithm, src/neighborJoining.cu:211-243: one full Q scan per iteration) on one GPU
    alone, and row-sharded over this run's GPUs with every exchange plan of the library.  Every multi-rank record carries the
    rank count RCCL reports, launches and collectives per iteration as counted by the library, and digests checked against
    rank 0's single-GPU loop."""
    import dipper_amd
    iters = max(1, min(iters, n - 2))
    rec = {"tips": n, "sites": L, "iterations_timed": iters, "world": world,
           "layout": "rows block-cyclic over the ranks (dpr_shard_owner), one full Q scan of the own rows per iteration; "
                     "timed part: the first iterations of the run (dpr_nj_run with max_iters), HIP events on the library's stream",
           "default_plan_one_gpu": {"algorithm": "exact pruned scan (njp.hip)", "nj_iterations_per_s": (solo_pruned_its / world) if solo_pruned_its else None,
                                    "note": "whole-run average of hot_path (the early iterations timed below are the largest ones)"}}
    # one GPU alone (rank 0; the denominator of every speed-up below)
    solo = None
    log(f"[bench r{rank}] +{elapsed():.0f}s: nj_scaling at {n} tips: streaming loop on one GPU alone (rank 0)")
    if rank == 0:
        s1 = dipper_amd.Dipper(local_rank)
        try:
            solo, r1 = streaming_run(s1, torch, dist, barrier, packed, n, L, iters, 1)
        finally:
            s1.close()
        rec["streaming_one_gpu"] = r1
    # the row-sharded PRUNED plan with 8 virtual ranks on rank 0's GPU: merge log checked, per-rank kernel times
    if rank == 0 and not args.no_virtual_pruned and (budget is None or budget.allows(45)):
        log(f"[bench] +{elapsed():.0f}s: nj_scaling at {n} tips: row-sharded pruned NJ, 8 virtual ranks on one GPU")
        try:
            rec["row_sharded_pruned_virtual"] = row_sharded_pruned_virtual(local_rank, packed, n, L, 8, solo_pruned_digest, budget)
        except Exception as e:
            rec["row_sharded_pruned_virtual"] = {"error": repr(e)}
        log(f"[bench] nj_scaling.row_sharded_pruned_virtual: {rec['row_sharded_pruned_virtual']}")
    if dist is not None:
        dist.barrier()
    if world == 1 and not (dist is not None and os.environ.get("DPR_BENCH_CHECK") == "1"):
        return rec          # (DPR_BENCH_CHECK: one rank walks through the child legs too -- RCCL id relay, pipes, time limits)
    rec["row_sharded"] = {}
    rec["row_sharded_runs_in"] = "one child process per rank without torch (system HIP runtime; see njs_worker)"
    p4 = getattr(packed, "filename", None)
    solo_digest = merge_digest(solo) if solo is not None else None
    for plan in [p.strip() for p in args.exchanges.split(",") if p.strip() in PLAN_ID]:
        if ONE_GPU and plan != "mailbox":
            rec["row_sharded"][plan] = {"skipped": "needs RCCL (rehearsal with process ranks on one GPU)"}
            continue
        # a plan that hangs costs its time limits (90 + 30 s): the ranks agree on whether the deadline still allows that
        if budget is not None and not budget.allows_all(130):
            rec["row_sharded"][plan] = budget.skip(130)
            continue
        log(f"[bench r{rank}] +{elapsed():.0f}s: nj_scaling at {n} tips: row-sharded over {world} ranks, exchange plan {plan}")
        try:
            r = njs_child_leg(plan, rank, world, local_rank, dist, torch, str(p4), n, L, iters, setup_s=90.0, run_s=30.0)      # (set-up: child start, RCCL communicator of the children, matrix build, peer mappings, warm-up)
        except Exception as e:
            r = {"error": repr(e)}
        if rank == 0 and "error" not in r and solo_digest is not None:
            r["matches_single_gpu"] = bool(r["merge_log_digest"] == solo_digest and r["iterations"] == int(solo["iters"]))
            r["iteration_speedup_vs_one_gpu"] = rec["streaming_one_gpu"]["us_per_iteration"] / r["us_per_iteration"]
        rec["row_sharded"][plan] = r
        if rank == 0:
            log(f"[bench] nj_scaling.row_sharded.{plan}: {r}")
    # the row-sharded exact PRUNED NJ on this run's ranks (njr.hip): the WHOLE run (it is short), per exchange plan
    rec["row_sharded_pruned"] = {}
    for plan in ("collective", "mailbox"):
        if ONE_GPU and plan != "mailbox":
            rec["row_sharded_pruned"][plan] = {"skipped": "needs RCCL (rehearsal with process ranks on one GPU)"}
            continue
        if budget is not None and not budget.allows_all(150):
            rec["row_sharded_pruned"][plan] = budget.skip(150)
            continue
        log(f"[bench r{rank}] +{elapsed():.0f}s: nj_scaling at {n} tips: row-sharded PRUNED over {world} ranks, exchange plan {plan}")
        try:
            r = njs_child_leg(plan, rank, world, local_rank, dist, torch, str(p4), n, L, -1, setup_s=90.0, run_s=60.0, algo="pruned_rows")
        except Exception as e:
            r = {"error": repr(e)}
        if rank == 0 and "error" not in r:
            if solo_pruned_digest is not None:
                r["matches_single_gpu"] = bool(r["merge_log_digest"] == solo_pruned_digest and r["iterations"] == n - 2)
            if solo_pruned_its:
                r["iteration_speedup_vs_default_plan_one_gpu"] = r["nj_iterations_per_s"] / solo_pruned_its
            if "streaming_one_gpu" in rec:
                r["iteration_speedup_vs_streaming_one_gpu"] = r["nj_iterations_per_s"] / rec["streaming_one_gpu"]["nj_iterations_per_s"]
        rec["row_sharded_pruned"][plan] = r
        if rank == 0:
            log(f"[bench] nj_scaling.row_sharded_pruned.{plan}: {r}")
    return rec


def sharded_leg(args, rank, world, local_rank, dist, torch, barrier, stage, budget):
    """100 000 tips x 10 000 sites (80 GB matrix): the unit-sharded pruned plan over the library's RCCL communicator (matrix
    replicated, unit tests and scans owned by rank, one all-gather of block records per iteration) next to the single-GPU
    plan on rank 0's GPU alone; the row-sharded streaming loop per exchange plan; divide-and-conquer of 1 000 000 tips."""
    import dipper_amd
    from dipper_amd import capi
    ns, Ls = args.sharded_tips, args.sharded_sites
    rec = {"tips": ns, "sites": Ls, "world": world}
    if not budget.allows_all(60):
        return dict(rec, **budget.skip(60))
    inp = stage.gen("nj100k", ns, Ls, args.seed + 7, 2e-5 * 10000 / Ls, 2e-6 * 10000 / Ls, 2e-4 * 10000 / Ls, gap=None if args.no_indel_gaps else args.gap_frac)
    packed = Stage.packed4(inp)
    if ONE_GPU and world > 1:
        rec["unit_sharded_plan"] = {"skipped": "rehearsal with process ranks on ONE GPU: two 80 GB matrices per rank do not fit beside each other"}
        try:
            rec["nj_scaling"] = nj_scaling(args, rank, world, local_rank, dist, torch, barrier, packed, ns, Ls, max(8, args.stream_iters // 4), None, budget)
        except Exception as e:
            rec["nj_scaling"] = {"error": repr(e)}
        del packed
        # (the divide-and-conquer leg runs here too since round 6: the ranks' all-reduces go through the device windows of dpr_comm_init_shared)
        try:
            rec["dc_1m"] = dc_leg(args, rank, world, local_rank, dist, torch, barrier, stage)
        except Exception as e:
            rec["dc_1m"] = {"error": repr(e)}
        return rec
    d = dipper_amd.Dipper(local_rank)
    try:
        ranks = join_comm(d, rank, world, dist) if world > 1 else 1
        d.set_nj_multi_plan(1)
        d.set_msa(packed, Ls)
        barrier()
        ts = time.perf_counter()
        d.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
        res = d.nj_run()
        barrier()
        wall = time.perf_counter() - ts
        dist_ms, nj_ms = d.timing()
        rec["unit_sharded_plan"] = {"is_unit_sharded": d.nj_is_unit_sharded(), "rccl_ranks": ranks, "wall_s": wall, "dist_ms": dist_ms, "nj_ms": nj_ms,
                                    "nj_iterations_per_s": (ns - 2) / (nj_ms * 1e-3), "merge_log_digest": merge_digest(res)}
        try:
            sc, full = d.prune_stats()
            rec["unit_sharded_plan"]["units_scanned_this_rank"] = sc
        except Exception:
            pass
    finally:
        d.close()
    digest = int(merge_digest(res)[:14], 16)
    if dist is not None:
        mine = torch.tensor([digest], dtype=torch.int64, device=TDEV)
        allh = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allh, mine)
        rec["ranks_agree"] = bool(all(int(t.item()) == digest for t in allh))
    if rank == 0:       # the single-GPU plan on one GPU, for the 1-GPU denominator (the other ranks wait)
        s = dipper_amd.Dipper(local_rank)
        try:
            s.set_nj_multi_plan(2)
            s.set_msa(packed, Ls)
            ts = time.perf_counter()
            s.dist_matrix(capi.SRC_MSA, capi.DIST_JC)
            ref = s.nj_run()
            wall1 = time.perf_counter() - ts
            d1, n1 = s.timing()
            rec["single_gpu_plan"] = {"wall_s": wall1, "dist_ms": d1, "nj_ms": n1, "nj_iterations_per_s": (ns - 2) / (n1 * 1e-3)}
            rec["matches_single_gpu"] = same_log(ref, res)
            rec["nj_speedup_vs_single_gpu"] = n1 / nj_ms
        finally:
            s.close()
    if dist is not None:
        dist.barrier()
    # the row-sharded streaming loop at this size too (a scan is 40 GB per iteration: the exchange is small beside it)
    need = 30 + 15 * len(args.exchanges.split(","))
    if budget.allows_all(need):
        try:
            rec["nj_scaling"] = nj_scaling(args, rank, world, local_rank, dist if world > 1 else None, torch, barrier, packed, ns, Ls,
                                           max(8, args.stream_iters // 4), rec.get("single_gpu_plan", {}).get("nj_iterations_per_s"), budget, merge_digest(res))
        except Exception as e:
            rec["nj_scaling"] = {"error": repr(e)}
    else:
        rec["nj_scaling"] = budget.skip(need)
    del packed
    # configs[3]: divide-and-conquer of 1 000 000 tips over the ranks (query shares of the assignment and the clusters dealt
    # to the ranks, backbone distance rows sharded; dpr_dc_run after dpr_comm_init), with rank 0's single-GPU run beside it
    if budget.allows_all(45):
        try:
            rec["dc_1m"] = dc_leg(args, rank, world, local_rank, dist if world > 1 else None, torch, barrier, stage)
        except Exception as e:
            rec["dc_1m"] = {"error": repr(e)}
    else:
        rec["dc_1m"] = budget.skip(45)
    return rec


def cli_ranks_leg(args, rank, world, local_rank, dist, stage, budget, tmp, main_fasta):
    """The `dipper` COMMAND over this run's GPUs -- `dipper ... --devices 0,1,..,G-1`: the command forks one rank per GPU once its
    input is read, the ranks join through a shared region (RCCL over xGMI with one rank per GPU; device windows over hipIpc when
    DPR_BENCH_ONE_GPU=1 puts every rank on GPU 0) -- next to the same command on one GPU, for configs[1]-[4].  Rank 0 runs the
    commands (the bench's other ranks wait); `newick_identical` = the two output files are the same bytes; `ranks` / `transport`
    / `device_collectives` are the command's own closing line (ranks = ncclCommCount with RCCL)."""
    rec = {"devices": "0" if world == 1 else ",".join(str(0 if ONE_GPU else r) for r in range(world))}
    G = max(world, 2) if (ONE_GPU or world == 1) else world
    if world == 1:
        rec["devices"] = ",".join("0" for _ in range(G))      # (DPR_BENCH_CHECK on one GPU: two ranks share it)
    devices = rec["devices"]

    def one(name, fmt, make_input, need):
        if not budget.allows_all(need):
            rec[name] = budget.skip(need)
            return
        out = {}
        t0 = time.perf_counter()
        try:
            fa, prep, note = make_input()        # (collective: rank 0 generates, every rank waits inside stage.gen)
        except Exception as e:
            fa, prep, note = None, None, "input failed: %r" % (e,)
        if rank == 0:
            try:
                if fa is None:
                    raise RuntimeError(note)
                extra = prep() if prep else []
                out["workload"] = note
                out["setup_s"] = time.perf_counter() - t0
                env = dict(os.environ, DPR_HOST_THREADS=str(host_cores()))
                res = {}
                for tag, dev in (("one_gpu", ["--device", "0"]), ("ranks", ["--devices", devices])):
                    o = os.path.join(tmp, "%s_%s.nwk" % (name, tag))
                    ts = time.perf_counter()
                    r = subprocess.run([EXE] + fmt + extra + ["-I", fa, "-O", o] + dev, capture_output=True, text=True, env=env, timeout=240)
                    wall = time.perf_counter() - ts
                    if r.returncode != 0:
                        raise RuntimeError("dipper %s (%s) failed: %s" % (name, tag, r.stderr[-400:]))
                    res[tag] = (wall, o, r.stderr)
                    out[tag + "_s"] = wall
                    out[tag + "_phases_ms"] = cli_phases(r.stderr)
                same = open(res["one_gpu"][1], "rb").read() == open(res["ranks"][1], "rb").read()
                out["newick_identical"] = bool(same)
                out["speedup"] = res["one_gpu"][0] / res["ranks"][0]
                for line in res["ranks"][2].splitlines():
                    if line.startswith("Ranks: "):
                        out["ranks"] = int(line.split()[1])
                        out["transport"] = line.split("transport ")[1].split(",")[0]
                        out["device_collectives"] = int(line.split(", ")[1].split()[0])
                    if line.startswith("NJ over "):
                        out["nj_plan"] = line.split(": ", 1)[1]
                for tag in res:
                    os.unlink(res[tag][1])
            except Exception as e:
                out["error"] = repr(e)
            log(f"[bench] cli_ranks.{name}: {out}")
        if dist is not None:
            dist.barrier()
        rec[name] = out

    def nj_input():
        return main_fasta, None, "configs[1]: %d aligned tips x %d sites, -m 2 -d 2 (below 65 536 tips every rank runs the single-GPU plan: replicas)" % (args.tips, args.sites)

    def place_input():
        inp = stage.gen("cli_reads100k", 100000, 3000, args.seed + 8, 2e-5, 2e-6, 2e-4, fasta=True, reads=True)
        return inp["fasta"], None, "configs[2]: 100 000 unaligned tips x ~3 000 bases, -i r -m 1 (distance rows of a batch sharded + one all-gather per batch)"

    def dc_input():
        n = args.dc_tips
        inp = stage.gen("cli_dc1m", n, 400, args.seed + 9, 2e-3, 2e-4, 2e-2, fasta=True, gap=None if args.no_indel_gaps else args.gap_frac)
        return inp["fasta"], None, "configs[3]: divide-and-conquer, %d aligned tips x 400 sites, -m 3 -d 2 (query shares + clusters dealt to the ranks, all-reduces)" % n

    def add_input():
        m, nq = args.add_backbone, args.add_queries
        inp = stage.gen("cli_add", m + nq, 1000, args.seed + 10, 1e-3, 1e-4, 1e-2, fasta=True, shuffle=7, gap=None if args.no_indel_gaps else args.gap_frac)

        def prep():          # rank 0: the backbone tree = the command's own divide-and-conquer tree of the first m records (untimed)
            buf = np.memmap(inp["fasta"], dtype=np.uint8, mode="r")
            starts = np.flatnonzero(buf == ord(">"))
            fa_bb = os.path.join(tmp, "cli_bb.fa")
            with open(fa_bb, "wb") as f:
                f.write(buf[:int(starts[m])].tobytes())
            del buf, starts
            bb = os.path.join(tmp, "cli_bb.nwk")
            r = subprocess.run([EXE, "-i", "m", "-d", "2", "-m", "3", "-I", fa_bb, "-O", bb, "--device", "0"], capture_output=True, text=True)
            os.unlink(fa_bb)
            if r.returncode != 0:
                raise RuntimeError("dipper (backbone) failed: " + r.stderr[-300:])
            return ["-a", "-t", bb]
        return inp["fasta"], prep, "configs[4]: %d queries added to a %d-tip backbone, aligned x 1 000 sites, -a -t backbone.nwk (distance rows sharded + all-gathers)" % (nq, m)

    if main_fasta:
        one("nj_30k", ["-i", "m", "-m", "2", "-d", "2"], nj_input, 15)
    one("place_100k_unaligned", ["-i", "r", "-m", "1"], place_input, 40)
    one("dc_1m", ["-i", "m", "-m", "3", "-d", "2"], dc_input, 60)
    one("add_50k_onto_500k_aligned", ["-i", "m", "-d", "2"], add_input, 70)
    return rec


def dc_leg(args, rank, world, local_rank, dist, torch, barrier, stage):
    import dipper_amd
    from dipper_amd import capi
    n, L = args.dc_tips, 400
    inp = stage.gen("dc1m", n, L, args.seed + 9, 2e-3, 2e-4, 2e-2, shuffle=7, gap=None if args.no_indel_gaps else args.gap_frac)      # the CLI shuffles its input (src/tree_generation.cu:341-344)
    packed = Stage.packed4(inp)
    rec = {"tips": n, "sites": L, "backbone": n // 20, "world": world}

    def run(d, multi):
        d.set_msa(packed, L)
        if multi:
            barrier()
        t0 = time.perf_counter()
        st = d.dc_run(capi.SRC_MSA, n, n // 20, dist_type=capi.DIST_JC)
        wall = time.perf_counter() - t0
        h = hashlib.sha256()
        for key in ("head", "e", "nxt", "belong", "len"):
            h.update(np.ascontiguousarray(st[key]).tobytes())
        return wall, st["stats"], h.hexdigest()[:16]

    d = dipper_amd.Dipper(local_rank)
    try:
        if world > 1:
            nr = join_comm(d, rank, world, dist)
            rec["transport"] = d.comm_stats()[0]
            rec["rccl_ranks" if rec["transport"] == "rccl" else "ranks_joined"] = nr      # (never a window run reported as RCCL ranks)
        wall, stats, digest = run(d, world > 1)
        if world > 1:
            rec["device_collectives"] = d.comm_stats()[1]
    finally:
        d.close()
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64, device=TDEV)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
        mine = torch.tensor([int(digest[:14], 16)], dtype=torch.int64, device=TDEV)
        allh = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allh, mine)
        rec["ranks_agree"] = bool(all(int(x.item()) == int(digest[:14], 16) for x in allh))
    rec.update({"seconds": wall, "tips_per_s": n / wall, "tree_digest": digest,
                "stats_rank0": {k: (float(v) if isinstance(v, float) else int(v)) for k, v in stats.items()}})
    if world > 1:
        if rank == 0:
            solo = dipper_amd.Dipper(local_rank)
            try:
                w1, st1, dg1 = run(solo, False)
            finally:
                solo.close()
            rec["single_gpu"] = {"seconds": w1, "tips_per_s": n / w1}
            rec["matches_single_gpu"] = dg1 == digest
            rec["speedup_vs_single_gpu"] = w1 / wall
        dist.barrier()
    return rec


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "--njs-worker":
    njs_worker()

if __name__ == "__main__":
    main()
