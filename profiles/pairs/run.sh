#!/bin/sh
# The measurements of DESIGN.md section 22 (tools/pairs_bench.py: every GPU step under a time limit of its own); results under $1
# (default profiles/pairs).
set -e
cd "$(dirname "$0")/../.."
out=${1:-profiles/pairs}
mkdir -p "$out"
timeout -k 10 1100 python tools/pairs_bench.py --matrix-command --out "$out/pairs_bench.jsonl"
