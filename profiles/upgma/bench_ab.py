"""The flagship check of DESIGN.md section 17: `bench.py --gpus 1 --steps 5 --warmup 2` on a built checkout of the parent commit
and on this tree, alternating in one session (parent, this, parent, this).  One JSON document on stdout.

    python profiles/upgma/bench_ab.py PARENT_DIR > profiles/upgma/bench_parent_vs_this.json

PARENT_DIR: the parent commit checked out and built (`git worktree add DIR HEAD~1`, then `python __graft_entry__.py` in it)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = ["--gpus", "1", "--steps", "5", "--warmup", "2"]


def bench(where):
    r = subprocess.run([sys.executable, "bench.py", *ARGS], cwd=where, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().split("\n")[-1])
    return {k: d[k] for k in ("ms_per_step", "value", "unit", "steps", "warmup")}


def main():
    parent = os.path.abspath(sys.argv[1])
    order = ["parent_1", "this_1", "parent_2", "this_2"]
    runs = {name: bench(parent if name.startswith("parent") else ROOT) for name in order}
    print(json.dumps({"command": "python bench.py " + " ".join(ARGS), "order": order, "runs": runs}, indent=1))


if __name__ == "__main__":
    main()
