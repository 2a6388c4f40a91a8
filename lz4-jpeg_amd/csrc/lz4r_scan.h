// lz4r_scan.h -- the exclusive scan of per-tile byte counts that places every
// tile in a stream ("tiles": the compressor's 300-B blocks, lz4_tiles' bsizes;
// the JPEG stream writers' records).  The consumer finishes it per group:
// partial + earlier group sums + a wave scan.
//   lz4_scan_reduce16, lz4_scan_partials_frame   the compressor's: u16 counts,
//                                                the frame byte
//   lz4_scan_reduce, lz4_scan_partials           the JPEG stream sources': u32
#pragma once
#include "lz4r_layout.h"
#include "wave64.h"

namespace {

// (a source that includes this header launches one pair of these, not both)
#define LZ4R_SCAN_ENTRY __attribute__((unused))

// the four waves' totals -> the workgroup's partial (256 threads; all call)
__device__ __forceinline__ uint64_t scan_wg_total(uint32_t tot, uint32_t *ws) {
  const int tid = threadIdx.x;
  tot = wave_incl_add(tot);                  // < 2^32: 4096 tiles of <= 548 B
  if ((tid & 63) == 63) ws[tid >> 6] = tot;
  __syncthreads();
  return (uint64_t)ws[0] + ws[1] + ws[2] + ws[3];
}

// per group of 64 tiles: gsum; per 64 groups: part.  Coalesced: load k of
// the workgroup reads tiles [1024 k, 1024 k + 1024) of the partial as uint4,
// 16 lanes (one DPP row) per group of 64 tiles.
__global__ __launch_bounds__(256) LZ4R_SCAN_ENTRY void lz4_scan_reduce(
    const uint32_t *__restrict__ tsz, size_t ntiles, size_t p_first, uint32_t *__restrict__ gsum,
    uint64_t *__restrict__ part) {
  __shared__ uint32_t ws[4];
  const int tid = threadIdx.x;
  const size_t pi = p_first + blockIdx.x;                            // partial index
  const size_t q0 = pi * (kPart / 4);                                // its first uint4
  uint32_t v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t q = q0 + (size_t)(256 * k + tid);                   // tiles 4q .. 4q + 3
    if (4 * q + 4 <= ntiles) {
      const uint4 x = reinterpret_cast<const uint4 *>(tsz)[q];
      v[k] = x.x + x.y + x.z + x.w;
    } else {
      v[k] = 0;
      for (int j = 0; j < 4; ++j)
        if (4 * q + j < ntiles) v[k] += tsz[4 * q + j];
    }
  }
  uint32_t tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t x = v[k];                       // row prefix: lane 15 of the row holds the group
    x += dpp<0x111, 0xf, 0xf>(x);
    x += dpp<0x112, 0xf, 0xf>(x);
    x += dpp<0x114, 0xf, 0xf>(x);
    x += dpp<0x118, 0xf, 0xf>(x);
    const size_t g = pi * 64 + (size_t)(16 * k + (tid >> 4));
    if ((tid & 15) == 15) {
      if (g * kGT < ntiles) gsum[g] = x;
      tot += x;
    }
  }
  const uint64_t p = scan_wg_total(tot, ws);
  if (tid == 0) part[pi] = p;
}

// One workgroup of 1024: exclusive scan of the partials in place, as absolute
// stream offsets.  The scan starts at `hdr` (first != 0) or at *len (a
// continuation) and leaves its end in *len.  The call's last scan (last != 0)
// also folds the corrupt-index status word into bit 63 of *len (kLenCorrupt)
// and clears the word: every async caller gets the verdict in the length it
// reads anyway, and the next call starts clean.  The same verdict goes to
// *verdict, a word the context owns (lz4r_check reads it: the caller's
// length buffer may be gone by then).
__device__ __forceinline__ void scan_partials(uint64_t *__restrict__ part, size_t nparts,
                                              uint64_t hdr, int first, int last,
                                              uint32_t *__restrict__ status,
                                              uint64_t *__restrict__ len,
                                              uint64_t *__restrict__ verdict) {
  __shared__ uint64_t ws[16];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = first ? hdr : *len;
  __syncthreads();
  for (size_t c0 = 0; c0 < nparts; c0 += 1024) {
    const size_t i = c0 + threadIdx.x;
    const uint64_t v = i < nparts ? part[i] : 0;
    uint64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t o = __shfl_up(x, d, 64);
      if ((threadIdx.x & 63) >= d) x += o;
    }
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = x;
    __syncthreads();
    uint64_t pre = carry;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += ws[w];
    if (i < nparts) part[i] = pre + x - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = pre + x;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint64_t v = carry;
    if (last) {
      const bool bad = atomicExch(status, 0u) != 0u;
      if (bad) v |= kLenCorrupt;
      *verdict = bad ? 1u : 0u;
    }
    *len = v;
  }
}

__global__ __launch_bounds__(1024) LZ4R_SCAN_ENTRY void lz4_scan_partials(
    uint64_t *__restrict__ part, size_t nparts, uint64_t hdr, int first, int last,
    uint32_t *__restrict__ status, uint64_t *__restrict__ len, uint64_t *__restrict__ verdict) {
  scan_partials(part, nparts, hdr, first, last, status, len, verdict);
}

// The compressor's: the same scan, and the stream's frame byte (frame >= 0: a
// framed call's first chunk) -- one store here, not a test in every lz4_emit
// workgroup.
__global__ __launch_bounds__(1024) LZ4R_SCAN_ENTRY void lz4_scan_partials_frame(
    uint64_t *__restrict__ part, size_t nparts, uint64_t hdr, int first, int last,
    uint32_t *__restrict__ status, uint64_t *__restrict__ len, uint64_t *__restrict__ verdict,
    uint8_t *__restrict__ out, int frame) {
  scan_partials(part, nparts, hdr, first, last, status, len, verdict);
  if (threadIdx.x == 0 && frame >= 0) out[0] = (uint8_t)frame;
}

// The compressor's reduce, over the u16 counts lz4_tiles left (bsizes, gsum and
// part are the launch chunk's: tile 0 is its first block, so indices are
// 32-bit).  A uint4 holds 8 counts: load k of the workgroup reads tiles
// [2048 k, 2048 k + 2048) of the partial, and a group of 64 tiles is 8 lanes,
// half a DPP row.
__global__ __launch_bounds__(256) LZ4R_SCAN_ENTRY void lz4_scan_reduce16(
    const uint16_t *__restrict__ bsizes, uint32_t ntiles, uint32_t *__restrict__ gsum,
    uint64_t *__restrict__ part) {
  __shared__ uint32_t ws[4];
  const uint32_t tid = threadIdx.x, pi = blockIdx.x;
  const uint32_t q0 = pi * (uint32_t)(kPart / 8);                    // its first uint4
  uint32_t v[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t q = q0 + 256u * k + tid;                          // tiles 8q .. 8q + 7
    if (8 * q + 8 <= ntiles) {
      const uint4 x = reinterpret_cast<const uint4 *>(bsizes)[q];
      const uint32_t a = x.x + x.y + x.z + x.w;    // two sums of four counts <= 548: no carry
      v[k] = (a & 0xFFFFu) + (a >> 16);
    } else {
      v[k] = 0;
      for (uint32_t j = 0; j < 8; ++j)
        if (8 * q + j < ntiles) v[k] += bsizes[8 * q + j];
    }
  }
  uint32_t tot = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint32_t x = v[k];                       // row prefix: lanes 7 and 15 of the row hold a group
    x += dpp<0x111, 0xf, 0xf>(x);
    x += dpp<0x112, 0xf, 0xf>(x);
    const uint32_t y = x + dpp<0x114, 0xf, 0xf>(x);   // lanes i - 7 .. i of the row
    const uint32_t g = pi * 64u + 32u * k + (tid >> 3);
    if ((tid & 7u) == 7u) {
      if (g * (uint32_t)kGT < ntiles) gsum[g] = y;
      tot += y;
    }
  }
  const uint64_t p = scan_wg_total(tot, ws);
  if (tid == 0) part[pi] = p;
}

#undef LZ4R_SCAN_ENTRY

}  // namespace
