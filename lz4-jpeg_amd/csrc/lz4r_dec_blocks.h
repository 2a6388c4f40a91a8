// lz4r_dec_blocks.h -- lz4_decode_blocks: a wave of 64 lanes decodes kBPW
// blocks, a lane each, into LDS slots and stores their contiguous output.
//   - LDS stays small for occupancy (10.1 KB per wave: 32 output slots of
//     300 B + 16 B of slack; 15 waves/CU);
//   - each lane touches its block's next four 128-B lines up front so that
//     the serial walk does not wait on HBM once per line;
//   - the wave's 32 x 300 = 9600 contiguous output bytes leave as 16-B
//     stores gathered across the slot ends (one v_perm per dword).
// (The mappings that lost to this one: profiles/design_history.md §4.4.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave64.h"
#include "lz4r_dec_layout.h"
#include "lz4r_dec_parse.h"

namespace {

constexpr int kPfN = 4;                    // L2 lines touched ahead of the walk
constexpr int kPfS = 128;                  // (2 / 4 / 8 lines, 64 or 128 B apart: same time)

struct DecLds {
  alignas(16) uint8_t out[kBPW * kSlotS + 48];  // lane l's block at out[kSlotS l] (+ slack)
  uint4 sel[17];                                 // sel[k]: v_perm selectors, bytes < k from A
  uint32_t qlen[kLanes];                         // decoded bytes per block (0 = failed)
};

// nb_dev (bare streams): the block count is read on the device, the grid is
// sized for an upper bound, and nothing is decoded unless *gate is kGateGo
__global__ __launch_bounds__(kLanes) void lz4_decode_blocks(
    const uint8_t *__restrict__ in, size_t in_len, const uint64_t *__restrict__ boff,
    size_t nb, uint8_t *__restrict__ out, size_t out_cap,
    unsigned long long *__restrict__ result, const unsigned long long *__restrict__ nb_dev,
    const unsigned long long *__restrict__ gate) {
  __shared__ DecLds S;
  const int lane = threadIdx.x;
  const size_t b0 = (size_t)blockIdx.x * kBPW;
  if (nb_dev) {
    if (*gate != kGateGo) return;
    nb = (size_t)*nb_dev;
  }
  if (b0 >= nb) return;
  const int nl = (int)(nb - b0 < (size_t)kBPW ? nb - b0 : kBPW);       // blocks here
  const size_t b = b0 + lane;

  int q = 0;                                         // decoded bytes (0 = failed / absent)
  uint32_t pfv[kPfN] = {};
  // the wave's base: its first block's first byte (a uniform load)
  const size_t wbeg = 1 + boff[b0];
  const uint8_t *const wbase = in + wbeg;
  if (lane < nl) {
    const bool last = b == nb - 1;
    const size_t beg = 1 + boff[b];
    const size_t end = last ? in_len : 1 + boff[b + 1];
    if (end >= beg + 3 && end <= in_len && end - beg <= (size_t)kInMax) {
      const Slot o{S.out + lane * kSlotS};
      // touch the block's next four 128-B lines now: the walk's header loads
      // then hit L2 instead of waiting on HBM one line at a time (the values
      // are folded into pfx after the walk; 1.82 -> 1.66 ms per GiB)
      {
        const uint8_t *q0 = in + ((beg + kPfS) & ~(size_t)(kPfS - 1));
        const uint8_t *qe = in + end;
#pragma unroll
        for (int t = 0; t < kPfN; ++t) {
          const uint8_t *q = q0 + kPfS * t;
          pfv[t] = *(q < qe ? q : q0 - kPfS);          // one byte: never past the stream
        }
      }
      // a lane's reads reach at most 32 bytes past its block (<= kInMax bytes):
      // unchecked loads only when that stays inside the stream, decided per
      // lane from its own offsets (caller-supplied offsets need not be
      // monotone; only the stream's last few blocks take the checked path)
      // (compressor offsets are monotone: the wave's blocks lie within
      // 32 x kInMax bytes of its base; other offsets take the checked path)
      if (beg + (size_t)kInMax + 64 <= in_len && beg >= wbeg && beg - wbeg < (1u << 30)) {
        const BytesW bw{wbase, (uint32_t)(beg - wbeg)};
        q = decode_block_plain(bw, (int)(end - beg), last, SlotW{S.out + lane * kSlotS});
        if (q < 0) q = decode_block(bw, (int)(end - beg), last, o);
      } else {
        q = decode_block(Bytes<true>{in + beg, in_len - beg}, (int)(end - beg), last, o);
      }
    }
    if (q == 0) atomicMin(&result[kResFail], (unsigned long long)b + 1);
    else if (last) result[kResLen] = (unsigned long long)(b * kBlk + q);
  }
  // keeps the prefetch loads alive; never true for a decoded block (q <= 300)
  uint32_t pfx = 0;
#pragma unroll
  for (int t = 0; t < kPfN; ++t) pfx ^= pfv[t];
  if (pfx == 0x5A5A5A5Au && q == 1000) q = 0;
  S.qlen[lane] = (uint32_t)q;
  if (lane < 17) {                                   // sel[k]: dword j, byte m from A iff 4 j + m < k
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t x = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) x |= (uint32_t)(4 * j + m < lane ? m : 4 + m) << (8 * m);
      w[j] = x;
    }
    S.sel[lane] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  __syncthreads();

  // ---- store the wave's contiguous output -----------------------------------
  // every block but the last decodes to exactly 300 bytes, so the valid range
  // is [300 b0, 300 b0 + sum q); a failed block leaves garbage (error raised).
  // Output byte x is slot l = x / 300, byte x - 300 l; a 16-B chunk that
  // crosses a slot end takes its first k bytes from slot l (A) and the rest
  // from slot l + 1, 16 B further on (B): one v_perm per dword.
  size_t total = 0;
  for (int l = 0; l < nl; ++l) total += l + 1 < nl ? kBlk : S.qlen[l];
  const size_t o0 = b0 * (size_t)kBlk;
  if (o0 >= out_cap) return;
  if (o0 + total > out_cap) total = out_cap - o0;
  auto src_of = [](uint32_t x) {                     // LDS offset of output byte x (< 2^15)
    const uint32_t l = (x * 27963u) >> 23;           // x / 300
    return x + 16u * l;
  };
  if (((reinterpret_cast<uintptr_t>(out) + o0) & 15) == 0) {
    const int nv = (int)(total >> 4);
    uint4 *dst = reinterpret_cast<uint4 *>(out + o0);
    for (int v = lane; v < nv; v += kLanes) {
      const uint32_t x = 16u * (uint32_t)v;
      const uint32_t l = (x * 27963u) >> 23;
      const uint32_t off = x - 300u * l;
      const uint32_t k = min(300u - off, 16u);
      const uint8_t *a = S.out + x + 16u * l;
      const uint4 A = *reinterpret_cast<const uint4 *>(a);
      const uint4 B = *reinterpret_cast<const uint4 *>(a + 16);
      const uint4 sl = S.sel[k];
      const u32x4 m = {__builtin_amdgcn_perm(B.x, A.x, sl.x), __builtin_amdgcn_perm(B.y, A.y, sl.y),
                       __builtin_amdgcn_perm(B.z, A.z, sl.z), __builtin_amdgcn_perm(B.w, A.w, sl.w)};
      // written once: non-temporal 16-B stores (-1.3 %, tools/ab_dec_inproc.py)
      __builtin_nontemporal_store(m, reinterpret_cast<u32x4 *>(dst) + v);
    }
    for (size_t i = (size_t)nv * 16 + lane; i < total; i += kLanes)
      out[o0 + i] = S.out[src_of((uint32_t)i)];
  } else {
    for (size_t i = lane; i < total; i += kLanes) out[o0 + i] = S.out[src_of((uint32_t)i)];
  }
}

}  // namespace
