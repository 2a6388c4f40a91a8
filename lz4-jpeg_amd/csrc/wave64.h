// wave64.h -- wave-level helpers of the compressor's gfx950 kernels: DPP scans,
// lane masks straight from SGPR pairs, EXEC-masked stores.  No LZ4 in here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// DPP helpers (gfx9 row_shr / row_bcast; identity 0 for lanes without a source)
template <int CTRL, int ROW, int BANK>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW, BANK, false);
}

__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
  v += dpp<0x111, 0xf, 0xf>(v);
  v += dpp<0x112, 0xf, 0xf>(v);
  v += dpp<0x114, 0xf, 0xf>(v);
  v += dpp<0x118, 0xf, 0xf>(v);
  v += dpp<0x142, 0xa, 0xf>(v);
  v += dpp<0x143, 0xc, 0xf>(v);
  return v;
}

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
  v = max(v, dpp<0x111, 0xf, 0xf>(v));
  v = max(v, dpp<0x112, 0xf, 0xf>(v));
  v = max(v, dpp<0x114, 0xf, 0xf>(v));
  v = max(v, dpp<0x118, 0xf, 0xf>(v));
  v = max(v, dpp<0x142, 0xa, 0xf>(v));
  v = max(v, dpp<0x143, 0xc, 0xf>(v));
  return v;
}

__device__ __forceinline__ uint32_t lane63(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// v with the wave-uniform s in lane kLane (v_writelane_b32, constant lane select)
template <int kLane>
__device__ __forceinline__ uint32_t write_lane(uint32_t v, uint32_t s) {
  asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "i"(kLane));
  return v;
}

// the wave's sum of each lane's 0 .. 3 (the JPEG decoders' rejected streams)
__device__ __forceinline__ uint32_t wave_rejected(uint32_t fails) {
  return (uint32_t)__popcll(__ballot(fails & 1)) + 2u * (uint32_t)__popcll(__ballot(fails & 2));
}

__device__ __forceinline__ int ctz64(uint64_t m) { return __builtin_ctzll(m); }

// lane mask of a predicate, straight from the compare (hip's __ballot goes
// through a 0/1 VGPR and a second compare)
__device__ __forceinline__ uint64_t ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }

// set bits of m in the lanes below this one (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ int rank_below(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                        __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// acc + the set bits of m in the lanes below this one (the adds fold into
// v_mbcnt's accumulator)
__device__ __forceinline__ uint32_t rank_below_plus(uint64_t m, uint32_t acc) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                   __builtin_amdgcn_mbcnt_lo((uint32_t)m, acc));
}

// per lane: t where the lane's bit of m is set, else f (v_cndmask with the
// mask straight from an SGPR pair)
__device__ __forceinline__ uint32_t sel_mask(uint64_t m, uint32_t t, uint32_t f) {
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m));
  return r;
}

// base[1 + off / 4] = v in the lanes of m: EXEC = EXEC & m around one
// global_store_dword, straight from the SGPR pair (a condition built from the
// mask costs a 0/1 select and a compare per store).  The untracked store only
// makes the compiler's later vmcnt waits conservative.
__device__ __forceinline__ void store_lanes1(uint64_t m, uint32_t *base, uint32_t off, uint32_t v) {
  uint64_t save;
  asm volatile(
      "s_and_saveexec_b64 %0, %1\n\t"
      "global_store_dword %2, %3, %4 offset:4\n\t"
      "s_or_b64 exec, exec, %0"
      : "=&s"(save)
      : "s"(m), "v"(off), "v"(v), "s"(base)
      : "memory", "scc");
}

// LDS dword at byte kOff + addr = v in the lanes of m, the same way: no
// select of a dummy address for the other lanes (the wave's LDS operations
// are served in order, so later reads see the store).  The address is
// absolute: the caller's array sits at LDS address 0 (lz4_tiles' TileLds)
template <int kOff>
__device__ __forceinline__ void lds_store_lanes(uint64_t m, uint32_t addr, uint32_t v) {
  uint64_t save;
  asm volatile(
      "s_and_saveexec_b64 %0, %1\n\t"
      "ds_write_b32 %2, %3 offset:%c4\n\t"
      "s_or_b64 exec, exec, %0"
      : "=&s"(save)
      : "s"(m), "v"(addr), "v"(v), "i"(kOff)
      : "memory", "scc");
}

// For a workgroup of one wave (lz4_tiles), or a wave's private LDS: a wave's
// LDS operations are served in order, so its phase boundaries need neither s_barrier nor the
// s_waitcnt vmcnt(0) lgkmcnt(0) that __syncthreads() implies: a compiler
// barrier that keeps the LDS accesses of both phases in program order is
// enough, and loads still in flight (LDS or global) stay in flight.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ uint32_t ffbl(uint32_t x) {   // v_ffbl_b32: -1 when x == 0
  uint32_t r;
  asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// 16 bytes as a native vector type (what the nontemporal builtins take)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

}  // namespace
