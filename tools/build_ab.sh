# Build an A/B variant library from a modified copy of one product source, a
# .hip or a header one includes (the copy keeps the product file's name):
#   tools/build_ab.sh path/to/lz4r_emit.h name          (headers: obj lz4r)
#   tools/build_ab.sh path/to/lz4r_dec_bare.h name lz4r_gpudec   (a decoder header)
#   tools/build_ab.sh path/to/jpegr.hip name            (obj: the .hip's name)
#   tools/build_ab.sh path/to/jpeg_tables.h name jpegr  (a header of another obj)
#     -> tools/ab/lib<obj>_<name>.so  (the product objects, make lib first, with
#        build/<obj>.o replaced by the variant; lib prefix liblz4_ for lz4r and
#        libjpeg_ for jpegr), its device assembly tools/ab/<obj>_<name>.s
# The variant compiles in a directory of its own, tools/ab/<obj>_<name>/: the
# product's csrc sources with the one file replaced, so every quoted include
# finds the variant's files first.
set -e
cd "$(dirname "$0")/.."
f=$(basename "$1")
case $f in *.hip) obj=${3:-${f%.hip}} ;; *) obj=${3:-lz4r} ;; esac
[ -f lz4-jpeg_amd/csrc/$f ] || { echo "$f: not a file of lz4-jpeg_amd/csrc"; exit 1; }
case $obj in lz4r) lib=liblz4_$2.so ;; jpegr) lib=libjpeg_$2.so ;; *) lib=lib${obj}_$2.so ;; esac
D=tools/ab/${obj}_$2
rm -rf $D
mkdir -p $D
cp lz4-jpeg_amd/csrc/*.h lz4-jpeg_amd/csrc/$obj.hip $D/
cp "$1" $D/$f
HIPCC=$(make -s print-HIPCC)
FLAGS="$(make -s print-HIPFLAGS) $EXTRA"
# the object's own flags: the Makefile variable of its stem (LZ4R_HIPFLAGS,
# LZ4R_GPUDEC_HIPFLAGS; empty for the others); NO_LZ4R_FLAGS=1 leaves them out
[ -z "$NO_LZ4R_FLAGS" ] && FLAGS="$FLAGS $(make -s print-$(echo $obj | tr a-z A-Z)_HIPFLAGS)"
$HIPCC $FLAGS -I lz4-jpeg_amd/csrc -c $D/$obj.hip -o $D/$obj.o
$HIPCC $FLAGS -I lz4-jpeg_amd/csrc --cuda-device-only -S $D/$obj.hip -o - | grep -v __hip_cuid_ > tools/ab/${obj}_$2.s
$HIPCC --offload-arch=gfx950 -shared -fPIC -o tools/ab/$lib \
  $D/$obj.o $(ls lz4-jpeg_amd/build/*.o | grep -v -e "/$obj.o" -e _seq.o -e _par.o -e _dec.o -e png_io.o)
echo built tools/ab/$lib
