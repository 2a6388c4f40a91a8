# Build the compressor's tools builds into tools/ab/ (not shipped): the
# product objects (make lib first) with lz4r.o recompiled under one macro each,
# with the Makefile's own flags for that object.
#   liblz4_prof.so        -DLZ4R_PROF        per-phase cycles (tools/lz4_prof.py)
#   liblz4_mark.so        -DLZ4R_MARK        ;PHASE_END markers in the assembly
#   liblz4_stale_head.so  -DLZ4R_STALE_HEAD  tools/poison_check.sh
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/ab
HIPCC=$(make -s print-HIPCC)
FLAGS="$(make -s print-HIPFLAGS) $(make -s print-LZ4R_HIPFLAGS)"
for v in prof mark stale_head; do
  $HIPCC $FLAGS -DLZ4R_$(echo $v | tr a-z A-Z) -c lz4-jpeg_amd/csrc/lz4r.hip -o tools/ab/lz4r_$v.o
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o tools/ab/liblz4_$v.so \
    tools/ab/lz4r_$v.o $(ls lz4-jpeg_amd/build/*.o | grep -v -e "/lz4r.o" -e _seq.o -e _par.o -e png_io.o)
  echo built tools/ab/liblz4_$v.so
done
