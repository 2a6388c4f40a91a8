// lz4r_prof.h -- measurement hooks of the compressor's tools builds
// (tools/build_variants.sh).  The product build defines none
// of the macros below: its PROF_MARK(k) call sites expand to nothing.
//   LZ4R_PROF  per-phase s_memtime ticks of every wave summed into
//              lz4r_prof_acc[], read by lz4r_prof_read (tools/lz4_prof.py).
//              The clock starts at the kernel's first instruction
//              (PROF_START) and travels into encode_block, so bucket 7 --
//              closed where the code first uses a block's key dwords
//              (keys_arrived, lz4r_tiles.h) -- is the wave-start wait of a
//              run's first block and, for the others, what the prefetch
//              left to wait for
//   LZ4R_MARK  static ;PHASE_END markers in the assembly (per-phase
//              instruction counts, read off tools/isa_gate.sh's output)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lz4r.h"

#ifdef LZ4R_PROF
// A wave sums its phases in scalar registers and adds them to the device
// totals once, as its last act (PROF_FLUSH), into one of kProfSlots copies
// (a 128-B line each) chosen by its workgroup index: an atomic per mark on
// one shared line made the build ~100 times slower than the product, and its
// shares those of the atomics.
constexpr int kProfSlots = 256;
__device__ unsigned long long lz4r_prof_acc[kProfSlots * 16];
struct ProfClock {
  uint64_t t;
  uint64_t acc[8];
};
#define PROF_START() \
  ProfClock { __builtin_amdgcn_s_memtime(), {} }
#define PROF_MARK(k)                                      \
  do {                                                    \
    const uint64_t prof_n = __builtin_amdgcn_s_memtime(); \
    prof.acc[k] += prof_n - prof.t;                       \
    prof.t = prof_n;                                      \
  } while (0)
#define PROF_FLUSH()                                                                       \
  do {                                                                                     \
    if (threadIdx.x == 0)                                                                  \
      for (int prof_k = 0; prof_k < 8; ++prof_k)                                           \
        atomicAdd(&lz4r_prof_acc[(blockIdx.x & (kProfSlots - 1)) * 16 + prof_k],           \
                  prof.acc[prof_k]);                                                       \
  } while (0)

extern "C" int lz4r_prof_read(unsigned long long *host16, int reset) {
  static unsigned long long all[kProfSlots * 16];
  if (hipMemcpyFromSymbol(all, HIP_SYMBOL(lz4r_prof_acc), sizeof(all)) != hipSuccess)
    return LZ4R_ERR_HIP;
  for (int k = 0; k < 16; ++k) {
    host16[k] = 0;
    for (int i = 0; i < kProfSlots; ++i) host16[k] += all[i * 16 + k];
  }
  if (reset) {
    static const unsigned long long zero[kProfSlots * 16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(lz4r_prof_acc), zero, sizeof(zero)) != hipSuccess)
      return LZ4R_ERR_HIP;
  }
  return LZ4R_OK;
}
#else
struct ProfClock {};
#define PROF_START() \
  ProfClock {}
#define PROF_FLUSH() \
  do {               \
  } while (0)
#ifdef LZ4R_MARK
#define PROF_MARK(k) asm volatile(";PHASE_END " #k ::: "memory")
#else
#define PROF_MARK(k) \
  do {               \
  } while (0)
#endif
#endif
