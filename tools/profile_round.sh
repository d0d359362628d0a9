#!/bin/bash
# Round profile on the GPU box: kernel trace + stats of the bench, and the two
# PMC traffic passes.  usage: tools/profile_round.sh <round>   (e.g. r01)
set -o pipefail
R=${1:?round}
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
OUT=${OKM_OUT:-bench_out}/prof_$R  # OKM_OUT: where the traces and logs go
mkdir -p $OUT profiles
# --streams 1: every launch single-stream, so the kernel averages are the ones
# bench.py's roofline pass measures (the default timed region overlaps 2 streams)
B="python bench.py --steps 1 --warmup 1 --cpu-sample-reads 0 --no-timing --streams 1 --c3-steps 0"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/trace -o p -f csv -- \
    python bench.py --full --steps 10 --warmup 2 --cpu-sample-reads 0 --streams 1 --c3-steps 0 > $OUT/bench_trace.json 2> $OUT/trace.log &&
timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE -d $OUT/fetch -o p -f csv -- $B > $OUT/fetch.log 2>&1 &&
timeout -k 10 240 rocprofv3 --pmc WRITE_SIZE -d $OUT/write -o p -f csv -- $B > $OUT/write.log 2>&1 &&
python tools/pmc_traffic.py $R $OUT/fetch/p_counter_collection.csv \
    $OUT/write/p_counter_collection.csv "$B" > $OUT/traffic.txt &&
python tools/rocprof_summary.py $OUT/trace/p_kernel_stats.csv > profiles/${R}_kernel_stats.txt &&
cp $OUT/bench_trace.json profiles/${R}_bench_under_rocprof.json &&
cp profiles/${R}_pmc_traffic.json $OUT/ &&
cp profiles/${R}_kernel_stats.txt $OUT/
