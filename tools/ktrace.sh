#!/bin/bash
# per-kernel times of one bench configuration: tools/ktrace.sh <outdir-name> <cfg> [lib.so]
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
ROOT=$PWD
export TMPDIR=/tmp
OUT=$PWD/gpurun_out/$1; CFG=$2; LIB=$3
mkdir -p $OUT
[ -n "$LIB" ] && export SPRINTZ_MI355X_LIB=$PWD/$LIB
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/trace_$CFG -o r -- python $ROOT/bench.py --full --only $CFG --no-cpu-baseline --config-reps 10 > $OUT/$CFG.json 2> $OUT/$CFG.err)
python - <<PY
import sqlite3,glob
db=sqlite3.connect(glob.glob("$OUT/trace_$CFG/*.db")[0])
for r in db.execute("select name,total_calls,average,percentage from top_kernels"):
    if any(k in r[0] for k in ("sprintz","huf","compact","scan_")):
        print(f"{r[0][:100]:100s} calls {r[1]:5d} avg {r[2]/1000:10.3f} ms")
PY
