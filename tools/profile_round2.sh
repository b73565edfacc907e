#!/bin/bash
# The rocprofv3 evidence of round 2, each pass under its own timeout, one sub-directory per workload:
#   tools/profile_round2.sh <outdir under gpurun_out> [workloads...]     (default: headline + every per_config entry)
# <w>/trace      rocprofv3 --kernel-trace --stats      (per-kernel time)
# <w>/pmc_fetch  rocprofv3 --pmc FETCH_SIZE            (HBM bytes read; own pass, --kernel-trace only)
# <w>/pmc_write  rocprofv3 --pmc WRITE_SIZE            (HBM bytes written; own pass)
# then, in the build container:  python profiles/summarize_r2.py gpurun_out/<outdir> profiles/r2
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
ROOT=$PWD
export TMPDIR=/tmp
OUT=$ROOT/gpurun_out/$1; shift
WL=${@:-headline cfg1 cfg3_1k cfg3_10k cfg4_10000 cfg4_80000 cfg4_800000 cfg5}
mkdir -p $OUT
for w in $WL; do
  if [ $w = headline ]; then ARGS="--full --configs none --no-extras --no-cpu-baseline --steps 20 --warmup 3"; PARGS="--full --configs none --no-extras --no-cpu-baseline --steps 3 --warmup 1 --ramp-ms 0"
  else ARGS="--full --only $w --no-cpu-baseline --config-reps 20"; PARGS="--full --only $w --no-cpu-baseline --config-reps 3"; fi
  mkdir -p $OUT/$w
  (cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/$w/trace -o r -- python $ROOT/bench.py $ARGS > $OUT/$w/bench_under_trace.json 2> $OUT/$w/trace.err)
  (cd /tmp && timeout 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/$w/pmc_fetch -o r -- python $ROOT/bench.py $PARGS > /dev/null 2> $OUT/$w/pmc_fetch.err)
  (cd /tmp && timeout 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/$w/pmc_write -o r -- python $ROOT/bench.py $PARGS > /dev/null 2> $OUT/$w/pmc_write.err)
  echo "$w done $(date +%T)"
done
# the databases are tens of MB each: summarise here, carry only the text back (gpurun merges <= 64 MiB)
mkdir -p $OUT/summary
python profiles/summarize_r2.py $OUT $OUT/summary/r2 --build "${BUILD_ID:-unlabelled}" --traffic-json $OUT/summary/hbm_traffic.json > $OUT/summary/summarize.log 2>&1
for w in $WL; do cp $OUT/$w/bench_under_trace.json $OUT/summary/${w}_bench_under_trace.json 2>/dev/null; rm -rf $OUT/$w; done
ls $OUT/summary | head -40
