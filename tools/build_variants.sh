# Build the compressor's tools builds into tools/ab/ (not shipped): the
# product objects (make lib first) with lz4r.o recompiled under one macro each,
# with the Makefile's own flags for that object.
#   liblz4_prof.so        -DLZ4R_PROF        per-phase cycles (tools/lz4_prof.py)
#   liblz4_mark.so        -DLZ4R_MARK        ;PHASE_END markers in the assembly
#   liblz4_stale_head.so  -DLZ4R_STALE_HEAD  tools/poison_check.sh
#   liblz4_run<N>.so      -DLZ4R_RUN=<N>     N = 1 2 4 8 16 blocks per lz4_tiles
#                                            workgroup (tools/ab_inproc.py; 1 =
#                                            a wave per block, no prefetch)
#   liblz4_prof_run1.so   -DLZ4R_PROF -DLZ4R_RUN=1   the phases of a wave per block
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/ab
HIPCC=$(make -s print-HIPCC)
FLAGS="$(make -s print-HIPFLAGS) $(make -s print-LZ4R_HIPFLAGS)"
build() {   # name, macros
  v=$1
  shift
  $HIPCC $FLAGS "$@" -c lz4-jpeg_amd/csrc/lz4r.hip -o tools/ab/lz4r_$v.o
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o tools/ab/liblz4_$v.so \
    tools/ab/lz4r_$v.o $(ls lz4-jpeg_amd/build/*.o | grep -v -e "/lz4r.o" -e _seq.o -e _par.o -e png_io.o -e jpeg_dec.o)
  echo built tools/ab/liblz4_$v.so
}
pids=""
for v in prof mark stale_head; do
  build $v -DLZ4R_$(echo $v | tr a-z A-Z) &
  pids="$pids $!"
done
for r in 1 2 4 8 16; do
  build run$r -DLZ4R_RUN=$r &
  pids="$pids $!"
done
build prof_run1 -DLZ4R_PROF -DLZ4R_RUN=1 &
pids="$pids $!"
for p in $pids; do wait $p; done   # (set -e: a failed build fails the script)
