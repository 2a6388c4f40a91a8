# Wave-slot counters of lz4_tiles on the 1 GiB corpus, in a run of their own
# (counters only, no tracing): how many waves, how long they live, and how
# long they wait for an instruction to issue.
# usage: [OUT=dir] bash tools/lz4_wave_pmc.sh <name> [lib.so]  -> $OUT/<name>.txt
# (OUT defaults to rocprof_out/wavepmc, which git ignores)
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
NAME=${1:?name}
LIB=${2:-$PWD/lz4-jpeg_amd/lz4jpeg/liblz4jpeg.so}
D=${OUT:-rocprof_out/wavepmc}
mkdir -p $D
rm -rf $D/$NAME
LZ4JPEG_LIB=$LIB timeout -s KILL 150 rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY \
  -d $D/$NAME -o run -- python3 tools/lz4_one.py 1073741824 2 1 > $D/$NAME.log 2>&1 ||
  { echo "pmc pass failed"; tail -5 $D/$NAME.log; exit 1; }
python3 tools/pmc_summary.py $D/$NAME/run_results.db lz4_tiles > $D/$NAME.txt
cat $D/$NAME.txt
