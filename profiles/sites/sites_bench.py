"""Cost of the site filter (dpr_msa_filter_sites) beside the upload it follows, in one process.

    DPR_LOG=cli python profiles/sites/sites_bench.py --n 30000 --sites 10000 [--protein] [--permille 1000,900] [--reps 3]

The alignment is near-clonal with indel runs at shared hot spots (the shape of gen_synth --indel-gaps: most columns complete, the
rest gappy in many sequences).  Per repetition and threshold: a fresh upload, then the filter; host clocks around the two calls
(both end in a device synchronise) go to stdout as JSON lines.  With DPR_LOG=cli the library prints its own laps to stderr: the
segments of msa_upload (nucleotides; "H2D copy" + "planes kernel" is the yardstick) and of msa_filter_sites (coverage kernel;
flags, scan; sources and gather kernels; tables rebuilt), each ended by a synchronise of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def gap_mask(rng, n, L, hot=None, per_seq=20):
    """bool [n][L]: every sequence has per_seq runs of 5..40 sites, each starting at one of `hot` shared positions"""
    hot = hot or max(1, L // 100)
    starts = np.sort(rng.choice(L, size=hot, replace=False))
    rows = np.repeat(np.arange(n), per_seq)
    s = starts[rng.integers(0, hot, size=n * per_seq)]
    e = np.minimum(s + rng.integers(5, 41, size=n * per_seq), L)
    diff = np.zeros((n, L + 1), dtype=np.int16)
    np.add.at(diff, (rows, s), 1)
    np.add.at(diff, (rows, e), -1)
    return np.cumsum(diff, axis=1, dtype=np.int16)[:, :L] > 0


def codes(rng, n, L, states):
    """uint8 [n][L]: one root, 0.1 % of the cells redrawn (near-clonal)"""
    a = np.broadcast_to(rng.integers(0, states, size=L, dtype=np.uint8), (n, L)).copy()
    k = n * L // 1000
    a[rng.integers(0, n, size=k), rng.integers(0, L, size=k)] = rng.integers(0, states, size=k, dtype=np.uint8)
    return a


def pack4(a):
    """4-bit codes [n][L] -> uint64 [n][ceil(L/16)], 16 per word, low nibble first (dpr_pack4's layout); code 4 = not a base"""
    n, L = a.shape
    W = (L + 15) // 16
    p = np.full((n, W * 16), 4, dtype=np.uint8)
    p[:, :L] = a
    by = p[:, 0::2] | (p[:, 1::2] << 4)      # two codes a byte, eight bytes a little-endian word
    return np.ascontiguousarray(by).view("<u8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--protein", action="store_true")
    ap.add_argument("--permille", default="1000,900")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    o = ap.parse_args()
    import dipper_amd
    rng = np.random.default_rng(o.seed)
    n, L = o.n, o.sites
    a = codes(rng, n, L, 20 if o.protein else 4)
    a[gap_mask(rng, n, L)] = 255 if o.protein else 4
    data = a if o.protein else pack4(a)
    del a
    d = dipper_amd.Dipper(0)

    def upload():
        if o.protein:
            d.set_msa_aa(data)
        else:
            d.set_msa(data, L)

    upload()                  # warm-up: code objects, first launches
    d.msa_filter_sites(500)
    for pm in [int(v) for v in o.permille.split(",")]:
        for rep in range(o.reps):
            sys.stderr.write(f"--- permille {pm} rep {rep}\n")
            sys.stderr.flush()
            t0 = time.perf_counter()
            upload()
            t1 = time.perf_counter()
            kept = d.msa_filter_sites(pm)
            t2 = time.perf_counter()
            print(json.dumps({"n": n, "sites": L, "alphabet": "protein" if o.protein else "nucleotide", "permille": pm, "rep": rep,
                              "kept": kept, "upload_call_ms": round((t1 - t0) * 1e3, 3), "filter_call_ms": round((t2 - t1) * 1e3, 3)}), flush=True)
    d.close()


if __name__ == "__main__":
    main()
