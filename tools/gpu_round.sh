# Round check on the GPU box: parity tests, the default bench line, a
# kernel-trace profile of the same bench command, HBM traffic PMC passes and
# the compressor's instruction-issue counts.  Everything under gpurun_out/round/.
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=gpurun_out/round
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/tests.log 2>&1 && \
timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 > $O/bench.json 2> $O/bench.err && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o run -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $O/prof_bench.json 2> $O/prof.log && \
python3 tools/prof_summary.py $O/prof > $O/kernels.md && \
bash tools/traffic.sh > $O/traffic.log 2>&1 && cp gpurun_out/traffic/traffic.json $O/traffic.json && \
bash tools/issue.sh > $O/issue.log 2>&1 && cp gpurun_out/issue/issue.json $O/issue.json && \
bash tools/clock_pmc.sh > $O/clock.json 2> $O/clock.log
rc=$?
tail -2 $O/tests.log; grep -E "^\[bench\]" $O/bench.err | tail -12; cat $O/kernels.md
exit $rc
