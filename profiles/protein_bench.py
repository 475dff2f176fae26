"""Protein distances beside the nucleotide type-2 kernel at the same n x L, and the whole `dipper --protein -m 2` command:
    python3 profiles/protein_bench.py [--tips 30000] [--sites 1000] [--gap-rate 0.03] [--runs 3] [--out FILE]
Inputs are generated here with NumPy: residues (and, for the nucleotide alignment, bases) evolved down one Yule tree, the same
not-a-residue / not-a-base positions in both.  dist_matrix is timed for protein types 1 and 8 and nucleotide type 2, alternated
in one session, `--runs` times each (HIP events of dpr_dist_matrix with the plain matrix layout: the pair kernel plus the row
sums, a 2 ms pass at 30 000 tips).  The commands are timed wall-clock, FASTA in /dev/shm to Newick.  One JSON line on stdout."""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--tips", type=int, default=30000)
ap.add_argument("--sites", type=int, default=1000)
ap.add_argument("--gap-rate", type=float, default=0.03)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--no-cli", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
import numpy as np
import dipper_amd
from dipper_amd import capi

n, L = args.tips, args.sites
rng = np.random.default_rng(1)


def evolve(states, mean_bl, lo, hi):
    """n x L codes down a Yule tree: every substitution a uniform draw among the other states"""
    seqs = [rng.integers(0, states, size=L, dtype=np.uint8)]
    leaves = [0]
    while len(leaves) < n:
        k = int(rng.integers(len(leaves)))
        for _ in range(2):
            t = seqs[leaves[k]].copy()
            m = rng.poisson(L * float(np.clip(rng.exponential(mean_bl), lo, hi)))
            if m:
                pos = rng.integers(0, L, size=m)
                t[pos] = (t[pos] + rng.integers(1, states, size=m, dtype=np.uint8)) % states
            seqs.append(t)
        leaves.append(len(seqs) - 1)
        leaves[k] = len(seqs) - 2
    return np.stack([seqs[i] for i in leaves])


t0 = time.time()
aa = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)[evolve(20, 0.02, 0.002, 0.1)]
nt = np.frombuffer(b"ACGT", dtype=np.uint8)[evolve(4, 0.01, 0.001, 0.05)]
gaps = rng.random((n, L)) < args.gap_rate
aa[gaps] = ord("-")
nt[gaps] = ord("-")
aa_seqs = [r.tobytes() for r in aa]
nt_seqs = [r.tobytes() for r in nt]
gen_s = time.time() - t0

capi.set_nj_mode(0)      # plain matrix layout: dist_matrix is the pair kernel and the row sums
dp, dn = dipper_amd.Dipper(0), dipper_amd.Dipper(0)
dp.set_msa_aa(capi.pack_aa_many(aa_seqs))
dn.set_msa(capi.pack4_many(nt_seqs), L)
legs = [("protein_p", dp, capi.DIST_UNCORRECTED), ("protein_kimura", dp, capi.DIST_KIMURA), ("nucleotide_jc", dn, capi.DIST_JC)]
for _, d, dt in legs:      # warm-up: code objects, first-touch of the matrix
    d.dist_matrix(capi.SRC_MSA, dt)
ms = {k: [] for k, _, _ in legs}
for _ in range(args.runs):
    for k, d, dt in legs:
        d.dist_matrix(capi.SRC_MSA, dt)
        ms[k].append(d.timing()[0])
dp.close(); dn.close()
capi.set_nj_mode(1)

rec = {"tips": n, "sites": L, "gap_rate": args.gap_rate, "generated_s": round(gen_s, 2), "dist_matrix_ms": ms,
       "median_ms": {k: float(np.median(v)) for k, v in ms.items()}}
base = rec["median_ms"]["nucleotide_jc"]
rec["ratio_to_nucleotide_jc"] = {k: rec["median_ms"][k] / base for k in ("protein_p", "protein_kimura")}
pairs = n * (n + 63) / 2      # tiles on and below the diagonal, roughly
rec["protein_word_pairs_per_s"] = pairs * ((L + 31) // 32) / (rec["median_ms"]["protein_p"] * 1e-3)

if not args.no_cli:
    exe = os.path.join(ROOT, "dipper_amd", "bin", "dipper")
    tmp = tempfile.mkdtemp(prefix="protb_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    cli = {}
    for tag, seqs, extra in (("protein_kimura", aa_seqs, ["--protein", "-d", "8"]), ("nucleotide_jc", nt_seqs, ["-d", "2"])):
        fa = os.path.join(tmp, tag + ".fa")
        with open(fa, "wb") as f:
            for i, s in enumerate(seqs):
                f.write(b">T%d\n" % i + s + b"\n")
        walls = []
        for _ in range(args.runs + 1):      # the first run is a warm-up
            t0 = time.time()
            r = subprocess.run([exe, "-i", "m", "-I", fa, "-O", os.path.join(tmp, tag + ".nwk"), "-m", "2", *extra], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"dipper failed ({tag}): {r.stderr[-2000:]}")
            walls.append(time.time() - t0)
        cli[tag] = {"wall_s": [round(w, 3) for w in walls[1:]], "stderr_tail": r.stderr.splitlines()[-6:]}
        os.unlink(fa); os.unlink(os.path.join(tmp, tag + ".nwk"))
    os.rmdir(tmp)
    rec["command_m2"] = cli
line = json.dumps(rec)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
