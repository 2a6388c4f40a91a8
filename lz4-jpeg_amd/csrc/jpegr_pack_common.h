// jpegr_pack_common.h -- what every reader and writer of the JPR stream
// (include/jpegr.h) shares: the record bounds, the tile count of a header, the
// scratch layout of jpegr_pack_scratch_bytes, the index scan (lz4r_scan.h as
// it is) and a workgroup's finish of that scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lz4r_scan.h"

namespace {

constexpr int kRecMax = 1036;               // 516 + 260 + 260
constexpr int kHdr = 16;

// slot bounds of channel c (0 Y, 1 Cr, 2 Cb): table entries = RLE ints, bits
__device__ __forceinline__ uint32_t slot_codes(int c) { return c ? 64u : 128u; }
__device__ __forceinline__ uint32_t slot_bits(int c) { return c ? 512u : 1024u; }

// Wave 0: the stream offsets of scan group g's 64 tiles into toff[0..64]
// (lz4_emit's finish of the scan: partial + earlier group sums + a wave scan).
__device__ __forceinline__ void group_offsets(const int tid, const size_t g, const size_t ntiles,
                                              const uint32_t *__restrict__ tsz,
                                              const uint32_t *__restrict__ gsum,
                                              const uint64_t *__restrict__ part, uint64_t *toff) {
  if (tid >= 64) return;
  const size_t g0 = g * kGT;
  const int nt = (int)min((size_t)kGT, ntiles - g0);
  const size_t p = g0 / kPart, gfirst = p * 64;
  const uint32_t gs = (gfirst + tid < g) ? gsum[gfirst + tid] : 0u;
  const uint64_t pt = part[p];
  const uint32_t tv = tid < nt ? tsz[g0 + tid] : 0u;
  // < 2^32: at most 4,096 tiles of at most 65,535 B before g in its partial
  const uint64_t base = pt + lane63(wave_incl_add(gs));
  const uint32_t inc = wave_incl_add(tv);
  toff[tid] = base + inc - tv;
  if (tid == 63) toff[kGT] = base + inc;
}

// tiles of nimg w x h images, 0 when a dimension is not positive or the
// count passes 2^32
inline size_t tiles_of(int w, int h, int nimg) {
  if (w <= 0 || h <= 0 || nimg <= 0) return 0;
  const uint64_t per = (uint64_t)(((int64_t)w + 7) / 8) * (uint64_t)(((int64_t)h + 7) / 8);
  if (per > (1ull << 32) || per * (uint64_t)nimg > (1ull << 32)) return 0;
  return (size_t)(per * (uint64_t)nimg);
}

// scratch: [partials u64][tile sizes u32, padded to 4][group sums u32]
struct Scratch {
  uint64_t *part;
  uint32_t *tsz, *gsum;
  size_t nparts, bytes;
};

inline Scratch scratch_of(void *base, size_t ntiles) {
  Scratch s;
  s.nparts = (ntiles + kPart - 1) / kPart;
  const size_t ngroups = (ntiles + kGT - 1) / kGT;
  const size_t part_b = (s.nparts * 8 + 15) & ~(size_t)15;
  const size_t tsz_b = ((ntiles + 3) & ~(size_t)3) * 4;
  auto *p = static_cast<uint8_t *>(base);
  s.part = reinterpret_cast<uint64_t *>(p);
  s.tsz = reinterpret_cast<uint32_t *>(p + part_b);
  s.gsum = reinterpret_cast<uint32_t *>(p + part_b + tsz_b);
  s.bytes = part_b + tsz_b + ngroups * 4;
  return s;
}

// HIP's grid limit is 2^32 work-items: launches of at most 2^22 workgroups
constexpr size_t kMaxWg = (size_t)1 << 22;

inline void scan(const Scratch &s, size_t ntiles, uint64_t *len, hipStream_t st) {
  hipLaunchKernelGGL(lz4_scan_reduce, dim3((unsigned)s.nparts), dim3(256), 0, st, s.tsz, ntiles,
                     (size_t)0, s.gsum, s.part);
  hipLaunchKernelGGL(lz4_scan_partials, dim3(1), dim3(1024), 0, st, s.part, s.nparts,
                     (uint64_t)kHdr + 2 * (uint64_t)ntiles, 1, 0, (uint32_t *)nullptr, len,
                     (uint64_t *)nullptr);
}

}  // namespace
