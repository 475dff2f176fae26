#!/bin/sh
# The measurements of DESIGN.md section 16, one time limit per GPU step; results under $1 (default profiles/spr).
set -e
cd "$(dirname "$0")/../.."
out=${1:-profiles/spr}
mkdir -p "$out"
timeout -k 10 240 python profiles/spr/spr_bench.py --tips 5000 --sites 1000 --command > "$out/time_5000x1000.json"
timeout -k 10 240 python profiles/spr/spr_bench.py --accuracy --tips 2000 --sites 500 --mean-bl 0.05 > "$out/nrf_2000x500_bl0.05.json"
timeout -k 10 240 python profiles/spr/spr_bench.py --accuracy --tips 2000 --sites 500 --mean-bl 0.15 > "$out/nrf_2000x500_bl0.15.json"
timeout -k 10 600 python profiles/spr/spr_bench.py --tips 20000 --sites 1000 --command --repeats 1 --budget-s 100 > "$out/time_20000x1000.json"
