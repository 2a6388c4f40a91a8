// lz4r_prof.h -- measurement hooks of the compressor's tools builds
// (tools/build_variants.sh).  The product build defines none
// of the macros below: its PROF_MARK(k) call sites expand to nothing.
//   LZ4R_PROF  per-phase s_memtime cycles of every wave summed into
//              lz4r_prof_acc[], read by lz4r_prof_read (tools/lz4_prof.py)
//   LZ4R_MARK  static ;PHASE_END markers in the assembly (per-phase
//              instruction counts, read off tools/isa_gate.sh's output)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lz4r.h"

#ifdef LZ4R_PROF
__device__ unsigned long long lz4r_prof_acc[16];
#define PROF_DECL uint64_t prof_t = __builtin_amdgcn_s_memtime()
#define PROF_MARK(k)                                                     \
  do {                                                                   \
    const uint64_t prof_n = __builtin_amdgcn_s_memtime();                \
    if (threadIdx.x == 0) atomicAdd(&lz4r_prof_acc[k], prof_n - prof_t); \
    prof_t = prof_n;                                                     \
  } while (0)

extern "C" int lz4r_prof_read(unsigned long long *host16, int reset) {
  if (hipMemcpyFromSymbol(host16, HIP_SYMBOL(lz4r_prof_acc), 16 * sizeof(unsigned long long)) !=
      hipSuccess)
    return LZ4R_ERR_HIP;
  if (reset) {
    static const unsigned long long zero[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(lz4r_prof_acc), zero, sizeof(zero)) != hipSuccess)
      return LZ4R_ERR_HIP;
  }
  return LZ4R_OK;
}
#elif defined(LZ4R_MARK)
#define PROF_DECL
#define PROF_MARK(k) asm volatile(";PHASE_END " #k ::: "memory")
#else
#define PROF_DECL
#define PROF_MARK(k) \
  do {               \
  } while (0)
#endif
