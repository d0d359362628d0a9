#!/bin/bash
# A/B timing of alternative library builds: tools/ab_bench.sh name1 name2 ...
# (each orion-kmer_amd/build_<name>/liborion_kmer.so; "main" = orion-kmer_amd/build);
# parity via debug_count rand, then the C2 bench; one summary line per build.
cd "$GRAFT_REPO_ROOT"
OUT=${OKM_OUT:-bench_out}/ab  # OKM_OUT: where the runs' lines and logs go
mkdir -p $OUT
for n in "$@"; do
  if [ "$n" = main ]; then lib=orion-kmer_amd/build/liborion_kmer.so; else lib=orion-kmer_amd/build_$n/liborion_kmer.so; fi
  OKM_LIB=$lib timeout -k 5 90 python tools/debug_count.py rand > $OUT/$n.dbg 2>&1 || exit 1
  OKM_LIB=$lib timeout -k 10 200 python bench.py --full --c3-steps 0 --steps 10 --warmup 2 --cpu-sample-reads 0 > $OUT/$n.json 2> $OUT/$n.err || exit 1
  python3 -c "import json; d=json.load(open('$OUT/$n.json')); print('$n', d['ms_per_step'], {k: v['avg_ms'] for k, v in d['kernels'].items() if v['avg_ms'] > 0.03})"
done
