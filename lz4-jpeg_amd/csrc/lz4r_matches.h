// lz4r_matches.h -- the batch match finders behind lz4r_block_matches_device
// and lz4r_window_matches_device (find_longest_match at every position; the
// compressor itself launches neither).
#pragma once
#include "lz4r_tiles.h"

namespace {

// Per-position longest matches of every block (the batch form of
// find_longest_match): the same staging and match finder as lz4_tiles.
__global__ __launch_bounds__(64) void lz4_matches(const uint8_t *__restrict__ in, uint32_t nb,
                                                   uint32_t last_n, uint32_t *__restrict__ mout) {
  __shared__ TileLds S;
  const int lane = threadIdx.x;
  const uint32_t t = blockIdx.x;
  if (t >= nb) return;
  const int n = t == nb - 1 ? (int)last_n : kBlk;
  const uint8_t *src = in + (size_t)t * kBlk;
  for (int i = lane; i < n; i += 64) S.buf[kInOff + i] = src[i];
  if (lane < 16) S.buf[kInOff + n + lane] = 0;
  wave_sync();
  TileKeys K;                            // (unused: the block is staged)
  RecBatch B;                            // (unused: no records)
  ProfClock prof = PROF_START();
  encode_block<true, false>(S, n, nullptr, K, nullptr, mout + (size_t)t * kBlk, nullptr, nullptr,
                            nullptr, lane, prof, B, true, nullptr, 0u);
}

// find_longest_match over a block of any length n (block_encode with a
// block_length other than 300): the reference's whole window, LZ4.c:295-312
// -- sources i in [max(0, p - WINDOW_SIZE), p), match length capped at
// MAX_MATCH_LENGTH (1024) and, canonically, at the block end n - p; the
// longest wins, ties to the smallest i (strict '>', LZ4.c:307).  One wave
// per position, its lanes striding over the window, a max-reduction of
// len << 17 | dist (the larger dist is the smaller source).  A compatibility
// path, O(n * window): the 300-byte blocks of the compressor use lz4_tiles.
constexpr int kWindow = 65535;          // WINDOW_SIZE, LZ4.c:22
constexpr int kMaxMatch = 1024;         // MAX_MATCH_LENGTH, LZ4.c:20

__global__ __launch_bounds__(256) void lz4_window_matches(const uint8_t *__restrict__ in,
                                                          uint32_t n, uint32_t p_first,
                                                          uint32_t *__restrict__ mout) {
  const int lane = threadIdx.x & 63;
  const uint32_t p = p_first + blockIdx.x * 4u + (threadIdx.x >> 6);
  if (p >= n) return;
  const uint32_t cap = min((uint32_t)kMaxMatch, n - p);
  const uint32_t i0 = p >= (uint32_t)kWindow ? p - (uint32_t)kWindow : 0u;
  const uint8_t c0 = in[p];
  uint32_t best = 0;
  for (uint32_t i = i0 + (uint32_t)lane; i < p; i += 64) {
    if (in[i] != c0) continue;
    uint32_t l = 1;
    while (l < cap && in[i + l] == in[p + l]) ++l;
    best = max(best, (l << 17) | (p - i));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, d, 64));
  if (lane == 0) {
    const uint32_t len = best >> 17;
    mout[p] = len >= 4 ? len | ((best & 0x1FFFFu) << 16) : 0u;   // MIN_MATCH_LENGTH, LZ4.c:314
  }
}

}  // namespace
