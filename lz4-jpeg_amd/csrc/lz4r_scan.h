// lz4r_scan.h -- the exclusive scan of the blocks' byte counts ("tiles" below:
// one per 300-B block, lz4_tiles' usz) that places every block in the stream.
// lz4_emit finishes it per group: partial + earlier group sums + a wave scan.
#pragma once
#include "lz4r_layout.h"
#include "wave64.h"

namespace {

// per group of 64 tiles: gsum; per 64 groups: part.  Coalesced: load k of
// the workgroup reads tiles [1024 k, 1024 k + 1024) of the partial as uint4,
// 16 lanes (one DPP row) per group of 64 tiles.
__global__ __launch_bounds__(256) void lz4_scan_reduce(const uint32_t *__restrict__ tsz,
                                                       size_t ntiles, size_t p_first,
                                                       uint32_t *__restrict__ gsum,
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
  tot = wave_incl_add(tot);                  // < 2^32: 4096 tiles of <= 548 B
  if ((tid & 63) == 63) ws[tid >> 6] = tot;
  __syncthreads();
  if (tid == 0) part[pi] = (uint64_t)ws[0] + ws[1] + ws[2] + ws[3];
}

// one workgroup: exclusive scan of the partials in place, as absolute stream
// offsets.  The scan starts at `hdr` (first != 0) or at *len (a continuation)
// and leaves its end in *len.  The call's last scan (last != 0) also folds
// lz4_tiles' corrupt-index status word into bit 63 of *len (kLenCorrupt) and
// clears the word: every async caller gets the verdict in the length it
// reads anyway, and the next call starts clean.  The same verdict goes to
// *verdict, a word the context owns (lz4r_check reads it: the caller's
// length buffer may be gone by then).
__global__ __launch_bounds__(1024) void lz4_scan_partials(uint64_t *__restrict__ part,
                                                          size_t nparts, uint64_t hdr,
                                                          int first, int last,
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

}  // namespace
