# call B of the final artifacts (after the PMC summaries of call A were copied into profiles/): bench lines + rocprofv3
# kernel stats of the headline and the side configurations, the rehearsals.  tools/final_bench.sh <tag>
set -o pipefail
R=$GRAFT_REPO_ROOT
TAG=${1:-r03}
cd $R
# the JSON lines of bench.py --full go to BENCH_OUT (the other steps keep their own paths); tools/copy_final.sh reads
# them from the same BENCH_OUT: set it to a folder that comes back from the GPU machine
OUT=${BENCH_OUT:-$R/bench_out}
mkdir -p $OUT
timeout -k 10 600 python bench.py --full --steps 10 --warmup 3 > $OUT/bench_256_$TAG.json 2> $OUT/bench_256_$TAG.err || { tail $OUT/bench_256_$TAG.err; exit 1; }
cut -c1-300 $OUT/bench_256_$TAG.json
for S in basic ecsimcorr; do
  DT=1.0; [ $S = basic ] && DT=0.1
  timeout -k 10 300 python bench.py --full --scheme $S --grid 128 --ppc 32 --dt $DT --steps 5 --warmup 2 > $OUT/bench_${S}_$TAG.json 2> $OUT/bench_${S}_$TAG.err || { tail $OUT/bench_${S}_$TAG.err; exit 1; }
  cut -c1-300 $OUT/bench_${S}_$TAG.json
done
A4="--scheme ecsimcorr --grid-xyz 512 512 64 --ppc 32 --steps 5 --warmup 2 --full"
timeout -k 10 600 python bench.py $A4 > $OUT/bench_cfg4_$TAG.json 2> $OUT/bench_cfg4_$TAG.err || { tail $OUT/bench_cfg4_$TAG.err; exit 1; }
cut -c1-300 $OUT/bench_cfg4_$TAG.json
cd /tmp && export TMPDIR=/tmp
rm -rf $R/gpurun_out/prof_$TAG $R/gpurun_out/prof_basic_$TAG $R/gpurun_out/prof_ecsimcorr_$TAG $R/gpurun_out/prof_cfg4_$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_$TAG -- python3 $R/bench.py --no-cpu-baseline > $R/gpurun_out/prof_$TAG.log 2>&1 || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_basic_$TAG -- python3 $R/bench.py --scheme basic --grid 128 --ppc 32 --dt 0.1 --steps 5 --warmup 2 --no-cpu-baseline > $R/gpurun_out/prof_basic_$TAG.log 2>&1 || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_ecsimcorr_$TAG -- python3 $R/bench.py --scheme ecsimcorr --grid 128 --ppc 32 --steps 5 --warmup 2 --no-cpu-baseline > $R/gpurun_out/prof_ecsimcorr_$TAG.log 2>&1 || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/prof_cfg4_$TAG -- python3 $R/bench.py $A4 --no-cpu-baseline > $R/gpurun_out/prof_cfg4_$TAG.log 2>&1 || exit 1
cd $R
bash tools/official_run.sh $TAG rehearsal
