# Round-3 evidence set: plain bench runs + rocprofv3 passes of the same commands (tools/profile_r3.sh)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${DODT_PROFILE_DIR:-profile_out}; mkdir -p "$out"
timeout -k 10 600 python bench.py --full > $out/r3_bench.json 2> $out/r3_bench.err &&
bash tools/profile_r3.sh r3 &&
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-alt --conv-dtype bf16 --head-dtype bf16 > $out/r3bf16_bench.json 2>/dev/null &&
bash tools/profile_r3.sh r3bf16 --conv-dtype bf16 --head-dtype bf16 &&
DODT_CONV_WINO=4 timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-alt > $out/r3w4_bench.json 2>/dev/null
tail -c 300 $out/r3_bench.json
