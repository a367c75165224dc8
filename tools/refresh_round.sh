cd "$(dirname "$0")/.."
OUT=${1:-bench_out}
mkdir -p $OUT
bash tools/collect_round.sh r06 $OUT > $OUT/r06_collect.txt 2>&1
bash tools/profile_passes.sh r06_final > $OUT/r06_pp_final.log 2>&1
bash tools/profile_passes.sh r06_adm --scene adm > $OUT/r06_pp_adm.log 2>&1
bash tools/profile_passes.sh r06_moving --scene moving > $OUT/r06_pp_moving.log 2>&1
bash tools/profile_passes.sh r06_bursty_moving --scene bursty-moving > $OUT/r06_pp_bursty_moving.log 2>&1
bash tools/traffic_passes.sh r06_C2 --config C2 > $OUT/r06_tp_C2.log 2>&1
bash tools/traffic_passes.sh r06_C3 --config C3 > $OUT/r06_tp_C3.log 2>&1
bash tools/traffic_passes.sh r06_C5 --config C5 > $OUT/r06_tp_C5.log 2>&1
( time timeout 600 python bench.py --full ) 2> $OUT/r06_bench_default.err | tail -1 > $OUT/r06_bench_default.json
