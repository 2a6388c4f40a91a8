# Device-assembly identity of one translation unit (csrc/<unit>.hip and the
# headers it includes; default lz4r, the compressor) against a commit: both
# texts compiled with the Makefile's own flags for that unit (HIPFLAGS + the
# variable of the unit's stem, LZ4R_HIPFLAGS / LZ4R_GPUDEC_HIPFLAGS) and
# --cuda-device-only -S, the __hip_cuid_<hash> lines (a hash of the file's
# path) dropped, then compared.
#   tools/isa_gate.sh <commit> [name] [unit]   DEFS="-D.." for the working tree,
#                                              OLD_DEFS="-D.." for the commit (default: DEFS)
#   tools/isa_gate.sh <commit> gpudec lz4r_gpudec      the decoder
#   -> build/isa_gate/<name>_{old,new}.s; prints line counts, sha256 and the
#      kernels' register counts; exit 1 when the two differ
set -e -o pipefail
cd "$(dirname "$0")/.."
rev=$1
name=${2:-product}
unit=${3:-lz4r}
: "${OLD_DEFS=$DEFS}"
O=build/isa_gate
src=lz4-jpeg_amd/csrc/$unit.hip
rm -rf $O/old_tree
mkdir -p $O/old_tree
git archive "$rev" include lz4-jpeg_amd/csrc | tar -x -C $O/old_tree
uvar=$(echo "$unit" | tr a-z A-Z)_HIPFLAGS
FLAGS="$(make -s print-HIPFLAGS) $(make -s print-$uvar) --cuda-device-only -S"
HIPCC=$(make -s print-HIPCC)
echo "old: $HIPCC $FLAGS $OLD_DEFS <$rev>/$src"
$HIPCC $FLAGS $OLD_DEFS $O/old_tree/$src -o - | grep -v __hip_cuid_ > $O/${name}_old.s
echo "new: $HIPCC $FLAGS $DEFS $src"
$HIPCC $FLAGS $DEFS $src -o - | grep -v __hip_cuid_ > $O/${name}_new.s
for s in old new; do
  echo "$s: $(wc -l < $O/${name}_$s.s) lines, sha256 $(sha256sum < $O/${name}_$s.s | cut -c1-64)"
done
awk '/^ +\.name: /{k=$2} /\.sgpr_count:/{s=$2} /\.vgpr_count:/{print "  " k ": vgpr " $2 ", sgpr " s}' $O/${name}_new.s | c++filt | sed 's/(anonymous namespace):://; s/(.*):/:/'
cmp -s $O/${name}_old.s $O/${name}_new.s && echo "$name: identical" ||
  { echo "$name: DIFFERENT ($(diff $O/${name}_old.s $O/${name}_new.s | grep -c '^[<>]') lines)"; exit 1; }
