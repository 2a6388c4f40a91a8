// lz4r_dec_read.h -- lz4_read_items: many byte ranges of the decoded stream in
// one launch, each decoded from the blocks it covers and from nothing else.
//   - the unit is an ITEM, one block covered by one read: a read of L bytes
//     covers at most K(L) = (L + 298) / 300 + 1 blocks, every read of a call
//     owns K(max_len) items, item i is read i / K's (i % K)-th block, and the
//     items past a read's last block idle (no scan, no search: uniform record
//     fetches fill the lanes, a skewed batch is correct and wastes them);
//   - as in lz4_decode_blocks a wave takes kBPW consecutive items, a lane
//     each, and decodes them into LDS slots kSlotS apart through the same
//     parsers (decode_block_plain, then decode_block where it declines);
//   - a wave's blocks can lie anywhere in the stream: the unchecked BytesW
//     loads only on a lane whose block starts less than 2^30 bytes above the
//     wave's lowest block start and kInMax + 64 bytes before the stream end,
//     the checked Bytes<true> everywhere else;
//   - all 64 lanes then store one item's slice per step: the bytes up to the
//     destination's next 16-B boundary and those after its last one as byte
//     stores (lanes 0-15 and 48-63), the 16-B pieces between as aligned dwordx4
//     stores (lanes 16-47; a slice has at most 18), each read from LDS as two
//     unaligned 8-B loads.
// The verdict: result[kRdBad] takes 1 + the first bad read (atomicMin).
// result[kRdSum] is the summed len of the delivered reads: a read's first item
// adds len once the read's own fields hold, and the read's FIRST failing item
// takes it back.  An item that fails finds out whether it is the first by
// parsing the read's earlier blocks itself (decode_block over a NullSlot:
// the parse does not depend on the decoded bytes); only a bad read pays that.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4r_dec_layout.h"
#include "lz4r_dec_parse.h"

namespace {

constexpr int kRdSum = 0, kRdBad = 1;      // the result pair of a read call

struct ReadReq {                           // lz4r_read
  uint64_t src, len, dst;
};

struct ReadLds {
  alignas(16) uint8_t out[kBPW * kSlotS + 48];   // lane l's block at out[kSlotS l] (+ slack)
  unsigned long long dst[kBPW];                  // the item's slice: its place in d_out,
  uint32_t lo[kBPW], n[kBPW];                    // its first byte in the slot, its length (0: none)
};

// block b's bytes [beg, end) of the stream, from offsets that may say
// anything: false unless they lie inside the stream and can hold a block
__device__ __forceinline__ bool read_block_span(size_t in_len, const uint64_t *__restrict__ boff,
                                                size_t nb, size_t b, size_t &beg, size_t &end,
                                                bool &last) {
  last = b == nb - 1;
  beg = 1 + boff[b];
  end = last ? in_len : 1 + boff[b + 1];
  return beg < end && end <= in_len && end - beg >= 3 && end - beg <= (size_t)kInMax;
}

// is block b well-formed?  (the parse alone, with checked loads)
__device__ bool read_block_ok(const uint8_t *__restrict__ in, size_t in_len,
                              const uint64_t *__restrict__ boff, size_t nb, size_t b) {
  size_t beg, end;
  bool last;
  if (!read_block_span(in_len, boff, nb, b, beg, end, last)) return false;
  return decode_block(Bytes<true>{in + beg, in_len - beg}, (int)(end - beg), last, NullSlot{}) != 0;
}

__global__ void lz4_read_init(unsigned long long *result) {
  result[kRdSum] = 0ull;
  result[kRdBad] = ~0ull;
}

__global__ __launch_bounds__(kLanes) void lz4_read_items(
    const uint8_t *__restrict__ in, size_t in_len, const uint64_t *__restrict__ boff, size_t nb,
    const ReadReq *__restrict__ reads, size_t nreads, size_t max_len, size_t K,
    uint8_t *__restrict__ out, size_t out_cap, unsigned long long *__restrict__ result) {
  __shared__ ReadLds S;
  const int lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kBPW + lane;

  ReadReq rd = {0, 0, 0};
  size_t r = 0, j = 0, b = 0, b_first = 0, beg = 0, end = 0;
  bool last = false;
  bool act = false;                        // the item has a block to decode
  bool fail = false;                       // the item makes its read a bad one
  bool counted = false;                    // ... after the read's len was added
  unsigned long long add = 0;              // len of the reads whose first item this is
  if (lane < kBPW) {
    r = i / K;
    j = i - r * K;
    if (r < nreads) rd = reads[r];
    if (rd.len != 0) {                     // (len 0: a good read with nothing to do)
      // the read's own fields, judged alike by each of its items: a read that
      // fails here has no item that decodes or stores anything
      const bool fields = rd.len <= max_len && rd.src + rd.len >= rd.src &&
                          rd.dst + rd.len >= rd.dst && rd.dst + rd.len <= out_cap;
      b_first = rd.src / kBlk;
      const size_t b_last = fields ? (rd.src + rd.len - 1) / kBlk : 0;
      if (!fields || b_last >= nb) {
        fail = j == 0;
      } else {
        if (j == 0) add = rd.len;
        b = b_first + j;                   // (j < K <= 2^62: no overflow)
        if (b <= b_last) {
          act = read_block_span(in_len, boff, nb, b, beg, end, last);
          fail = counted = !act;
        }
      }
    }
  }

  // the wave's base for BytesW: the lowest block start of its active lanes
  unsigned long long wmin = act ? (unsigned long long)beg : ~0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(wmin, d, 64);
    wmin = o < wmin ? o : wmin;
  }
  if (wmin == ~0ull) wmin = 0;             // (no active lane: nothing is loaded)

  uint32_t lo = 0, n = 0;
  unsigned long long dst = 0;
  if (act) {
    const int len = (int)(end - beg);
    const Slot o{S.out + lane * kSlotS};
    int q;
    if (beg + (size_t)kInMax + 64 <= in_len && beg - wmin < (1u << 30)) {
      const BytesW bw{in + wmin, (uint32_t)(beg - wmin)};
      q = decode_block_plain(bw, len, last, SlotW{S.out + lane * kSlotS});
      if (q < 0) q = decode_block(bw, len, last, o);
    } else {
      q = decode_block(Bytes<true>{in + beg, in_len - beg}, len, last, o);
    }
    // the read's bytes of this block: [lo, hi) of the slot; only the last
    // block can be short of them (the lane that learns the decoded length)
    const size_t s0 = b * (size_t)kBlk;
    const size_t e = rd.src + rd.len - s0;
    const uint32_t hi = e < (size_t)kBlk ? (uint32_t)e : (uint32_t)kBlk;
    lo = rd.src > s0 ? (uint32_t)(rd.src - s0) : 0u;
    if (q == 0 || hi > (uint32_t)q) {
      fail = counted = true;
    } else {
      n = hi - lo;
      dst = rd.dst + (s0 + lo - rd.src);
    }
  }
  if (lane < kBPW) {
    S.lo[lane] = lo;
    S.n[lane] = n;
    S.dst[lane] = dst;
  }

  // ---- the verdict ------------------------------------------------------------
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) add += __shfl_xor(add, d, 64);
  if (lane == 0 && add) atomicAdd(&result[kRdSum], add);
  if (fail) {
    atomicMin(&result[kRdBad], (unsigned long long)r + 1);
    if (counted) {
      // the read's first failing item takes the read's len back
      bool first = true;
      for (size_t t = j; t-- > 0 && first;) first = read_block_ok(in, in_len, boff, nb, b_first + t);
      if (first) atomicAdd(&result[kRdSum], 0ull - rd.len);
    }
  }
  __syncthreads();

  // ---- store the items' slices, one per step -----------------------------------
  uint64_t m = __builtin_amdgcn_ballot_w64(n != 0);
  while (m) {
    const int l = __builtin_ctzll(m);
    m &= m - 1;
    const uint32_t sn = __builtin_amdgcn_readfirstlane(S.n[l]);
    const uint32_t sl = __builtin_amdgcn_readfirstlane(S.lo[l]);
    const unsigned long long sd = S.dst[l];
    uint8_t *const g = out + (((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(sd >> 32)) << 32) |
                              __builtin_amdgcn_readfirstlane((uint32_t)sd));
    const uint8_t *const s = S.out + l * kSlotS + sl;
    const uint32_t to16 = (uint32_t)(0u - (uint32_t)reinterpret_cast<uintptr_t>(g)) & 15u;
    const uint32_t head = sn < to16 ? sn : to16;
    const uint32_t nv = (sn - head) >> 4;            // <= 18
    const uint32_t body = head + 16u * nv, tail = sn - body;
    if (lane >= 16 && lane < 48) {
      const uint32_t v = (uint32_t)lane - 16u;
      if (v < nv) {
        const u64u *p = reinterpret_cast<const u64u *>(s + head + 16u * v);
        const uint64_t a = p[0], c = p[1];
        *reinterpret_cast<uint4 *>(g + head + 16u * v) =
            make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)c, (uint32_t)(c >> 32));
      }
    } else {
      const bool hd = lane < 16;
      const uint32_t t = hd ? (uint32_t)lane : (uint32_t)lane - 48u;
      const uint32_t at = hd ? t : body + t;
      if (t < (hd ? head : tail)) g[at] = s[at];
    }
  }
}

}  // namespace
