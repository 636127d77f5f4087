#!/bin/bash
# round 3, session 2, final: whole GPU suite (incl. the config-5 fixture), default bench line, rocprof kernel stats of the bench command,
# throughput table 19-26 qubits
set -o pipefail
out=gpurun_out/r3_final; mkdir -p $out
R=$GRAFT_REPO_ROOT
python -m pytest tests -m gpu -q > $out/tests_all.log 2>&1; echo "pytest rc $?"; tail -3 $out/tests_all.log
timeout -k 10 900 python bench.py --full > $out/bench_default.json 2> $out/bench_default.err; echo "bench rc $?"; cut -c1-300 $out/bench_default.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$out/prof_c3 -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-c4-reference --no-c5-leg --no-live-traffic > $R/$out/bench_profiled.json 2> $R/$out/bench_profiled.err
echo "rocprofv3 rc $?"
cd $R
f=$(find $out/prof_c3 -name "*kernel_stats.csv" | head -n 1); cp "$f" $out/c3_kernel_stats.csv; head -n 5 $out/c3_kernel_stats.csv | cut -c1-200
rm -rf $out/prof_c3
timeout -k 10 600 python tools/throughput_vs_n.py 19 26 > $out/throughput_19_26.txt 2>&1; cat $out/throughput_19_26.txt | grep -v amdgpu
