# Round-4 profile sets (rocprofv3 with the program itself after --; counters in their own passes), one GPU job:
#   bash tools/profile_r4.sh        -> $DODT_PROFILE_DIR (default profile_out)/{r4,r4bf16,r4_dense}_{stats,pmc_mfma,pmc_fetch,pmc_write}, *_bench.json
# then, on any machine with the tree:  python3 tools/summarize_r4.py r4;  python3 tools/summarize_r4.py r4bf16 --dtype bf16
#   --conv-dtype bf16 --head-dtype bf16;  python3 tools/summarize_r4.py r4_dense --dense --points 300000 --proposals 4096 --tau 3 --boxes 40
set -o pipefail
out=${DODT_PROFILE_DIR:-profile_out}; mkdir -p "$out"
python3 bench.py --full --steps 40 --warmup 10 > $out/r4_bench.json 2> $out/r4_bench.err &&
bash tools/profile_r3.sh r4 &&
python3 bench.py --full --no-cpu-baseline --no-alt --steps 100 --warmup 10 --conv-dtype bf16 --head-dtype bf16 > $out/r4bf16_bench.json 2> $out/r4bf16_bench.err &&
bash tools/profile_r3.sh r4bf16 --conv-dtype bf16 --head-dtype bf16 &&
python3 bench.py --full --no-cpu-baseline --no-alt --steps 60 --warmup 10 --points 300000 --proposals 4096 --tau 3 --boxes 40 > $out/r4_dense_bench.json 2> $out/r4_dense_bench.err &&
bash tools/profile_r3.sh r4_dense --points 300000 --proposals 4096 --tau 3 --boxes 40
echo "profile_r4 rc $?"
