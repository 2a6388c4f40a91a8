// lz4r_dec_bare.h -- bare streams: block boundaries found on the device.
// LZ4_decode (LZ4.c:1038) takes only the file.  The stream is cut into
// chunks of kChunkB bytes; in each chunk the first position that parses as
// a block header is a candidate start (lz4_bare_cand), a lane per chunk
// walks the blocks from its candidate to the next chunk (lz4_bare_walk),
// and one wave checks that every chunk's walk ends on the next chunk's
// candidate, re-walking a chunk from its predecessor's exit where it does
// not (lz4_bare_fix).  By induction from position 1 the candidates are then
// on the stream's own block chain.  A block's length is its u16 size field
// (fast mode) unless it holds truncated matches (M = 1..3, LZ4.c:317), whose
// size fields count a byte that is never written (LZ4.c:569-575): the exact
// mode parses every block (decode_block<kFindLen>).  The host tries the
// fast mode first; the decoder checks every block against its boundaries,
// so a wrong fast-mode boundary is an error, never wrong bytes.
// The scratch regions and control words the kernels share with the host:
// lz4r_dec_layout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4r_dec_layout.h"
#include "lz4r_dec_parse.h"

namespace {

constexpr int kWin = 2 * kInMax + 32;                // candidate window (LDS)

__device__ __forceinline__ int rd_u16(const uint8_t *w, int a) {
  return (int)w[a] | ((int)w[a + 1] << 8);
}

// Candidate start of every chunk: a wave per chunk, its window
// [s, s + kWin) of the stream in LDS.  x passes when its header is
// plausible (1 <= nseq, 3 + 5 nseq <= size <= kInMax, inside the stream) and
// the nseq sequence size fields, hopped as written, end exactly at x + size
// (a true block without truncated matches always does), and the next header
// is plausible too (or x + size is the stream end).
__global__ __launch_bounds__(256) void lz4_bare_cand(const uint8_t *__restrict__ in,
                                                      size_t in_len, size_t nchunks,
                                                      uint64_t *__restrict__ cand) {
  constexpr int kWin16 = (kWin + 16 + 15) / 16;       // 16-B pieces of the window
  __shared__ alignas(16) uint8_t win[4][kWin16 * 16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t c = (size_t)blockIdx.x * 4 + wv;
  if (c >= nchunks) return;
  if (c == 0) {                                      // the first block starts after the frame byte
    if (lane == 0) cand[0] = 1;
    return;
  }
  const size_t s = 1 + c * (size_t)kChunkB;
  // the window [s, s + kWin) as aligned 16-B loads from s & ~15 (pieces
  // past the stream end bytewise, zero-filled)
  const size_t a0 = s & ~(size_t)15;
  uint8_t *const w = win[wv] + (s - a0);            // w[i] = in[s + i]
  for (int k = lane; k < kWin16; k += 64) {
    const size_t at = a0 + 16 * (size_t)k;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at + 16 <= in_len) {
      v = *reinterpret_cast<const uint4 *>(in + at);
    } else {
      uint32_t t[4] = {0, 0, 0, 0};
      for (int b = 0; b < 16; ++b)
        if (at + b < in_len) t[b >> 2] |= (uint32_t)in[at + b] << (8 * (b & 3));
      v = make_uint4(t[0], t[1], t[2], t[3]);
    }
    reinterpret_cast<uint4 *>(win[wv])[k] = v;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const int avail = (int)min((size_t)kWin, in_len - s);   // window bytes inside the stream
  uint64_t found = kNone;
  for (int x0 = 0; x0 < kInMax && x0 < avail; x0 += 64) {
    const int x = x0 + lane;
    bool ok = x + 3 <= avail;
    int nseq = 0, size = 0;
    if (ok) {
      nseq = w[x];
      size = rd_u16(w, x + 1);
      ok = nseq >= 1 && size >= 3 + 5 * nseq && size <= kInMax && x + size <= avail;
    }
    if (ok) {
      int y = x + 3;
      for (int k = 0; k < nseq && ok; ++k) {
        const int S = y + 3 <= x + size ? rd_u16(w, y + 1) : 0;
        ok = S >= 5;
        y += S;
        ok = ok && y <= x + size;
      }
      ok = ok && y == x + size;
      if (ok && s + (size_t)(x + size) < in_len) {   // the next header
        const int z = x + size;
        ok = z + 3 <= avail && w[z] >= 1 && rd_u16(w, z + 1) >= 8 && rd_u16(w, z + 1) <= kInMax;
      }
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(ok);
    if (m) {
      found = s + (size_t)(x0 + __builtin_ctzll(m));
      break;
    }
  }
  if (lane == 0) cand[c] = found;
}

// the byte length of the block at x (0: no block can start there)
template <bool kExact>
__device__ __forceinline__ int bare_block_len(const uint8_t *in, size_t in_len, size_t x) {
  if (x + 3 > in_len) return 0;
  if (!kExact) {
    // the header as one unaligned dword load (three byte loads were three
    // scattered wave loads for the vector memory address unit)
    const uint32_t h = x + 4 <= in_len ? *reinterpret_cast<const u32u *>(in + x)
                                       : (uint32_t)in[x] | (uint32_t)in[x + 1] << 8 | (uint32_t)in[x + 2] << 16;
    const int size = (int)((h >> 8) & 0xFFFF);
    return (h & 255) >= 1 && size >= 8 && size <= kInMax && x + size <= in_len ? size : 0;
  }
  const size_t rem = in_len - x;
  const int len = rem < (size_t)kInMax ? (int)rem : kInMax;
  return decode_block<Bytes<true>, NullSlot, true>(Bytes<true>{in + x, rem}, len,
                                                   rem <= (size_t)kInMax, NullSlot{});
}

// the blocks of chunk c from x: count and exit (the first position at or
// past the next chunk), or kBad; kWrite: their offsets to boff[base ...]
// lst (walk only): the first kList block starts, relative to the chunk start
template <bool kExact, bool kWrite>
__device__ __forceinline__ uint64_t bare_walk_chunk(const uint8_t *in, size_t in_len, size_t c,
                                                    uint64_t x, uint32_t &cnt,
                                                    uint64_t *boff, uint64_t base,
                                                    uint64_t boff_cap = 0,
                                                    uint16_t *lst = nullptr) {
  cnt = 0;
  if (x == kNone || x == kBad) return kBad;
  const uint64_t c0 = 1 + c * (uint64_t)kChunkB;
  const uint64_t lim = c0 + kChunkB;
  while (x < lim && x < in_len) {
    const int L = bare_block_len<kExact>(in, in_len, x);
    if (L == 0) return kBad;
    if (kWrite && base + cnt < boff_cap) boff[base + cnt] = x - 1;
    if (!kWrite && lst && cnt < (uint32_t)kList) lst[cnt] = (uint16_t)(x - c0);
    ++cnt;
    x += (uint64_t)L;
  }
  return x;
}

// a lane per chunk: count and exit from the candidate, and per wave of 64
// chunks the block count (gsum)
template <bool kExact>
__global__ __launch_bounds__(64) void lz4_bare_walk(const uint8_t *__restrict__ in, size_t in_len,
                                                    size_t nchunks,
                                                    const uint64_t *__restrict__ cand,
                                                    uint32_t *__restrict__ cnt,
                                                    uint64_t *__restrict__ exitp,
                                                    unsigned long long *__restrict__ gsum,
                                                    uint16_t *__restrict__ lists,
                                                    uint32_t *__restrict__ lok) {
  // the lanes' lists are staged in LDS (a global store per block would make
  // every next header load wait for it: in-order vmcnt) and leave as one
  // coalesced 4 KB copy per wave
  __shared__ alignas(16) uint16_t ls[64 * kList];
  const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
  uint32_t n = 0;
  if (c < nchunks) {
    exitp[c] = bare_walk_chunk<kExact, false>(in, in_len, c, cand[c], n, nullptr, 0, 0,
                                              ls + threadIdx.x * kList);
    cnt[c] = n;
    lok[c] = n <= (uint32_t)kList ? 1u : 0u;   // the list holds every block start
  }
  __syncthreads();
  {
    const size_t c0 = (size_t)blockIdx.x * 64;
    const int nl = (int)min((size_t)64, nchunks - c0);
    uint4 *dst = reinterpret_cast<uint4 *>(lists + c0 * kList);
    const uint4 *src = reinterpret_cast<const uint4 *>(ls);
    for (int i = threadIdx.x; i < nl * kList / 8; i += 64) dst[i] = src[i];
  }
  unsigned long long t = n;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
  if (threadIdx.x == 0) gsum[blockIdx.x] = t;
}

// A lane per chunk: chunk c is consistent when its exit is the next chunk's
// candidate (the last chunk's: the stream end).  The inconsistent ones go to
// an unordered list (count in *nmis; the list holds at most kMisCap).
__global__ __launch_bounds__(256) void lz4_bare_check(size_t in_len, size_t nchunks,
                                                      const uint64_t *__restrict__ cand,
                                                      const uint64_t *__restrict__ exitp,
                                                      unsigned int *__restrict__ nmis,
                                                      unsigned int *__restrict__ mis) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nchunks) return;
  const uint64_t e = exitp[c];
  const bool bad = e == kBad || (c + 1 < nchunks ? e != cand[c + 1] : e != (uint64_t)in_len);
  if (bad) {
    const unsigned int k = atomicAdd(nmis, 1u);
    if (k < (unsigned)kMisCap) mis[k] = (unsigned int)c;
  }
}

// One wave, in stream order over the listed chunks: a chunk whose exit is
// not the next chunk's candidate has the next chunk re-walked from that exit
// (the stream's own chain, by induction from position 1), which is then
// checked in turn; the others keep what lz4_bare_walk found.  More than
// kMisCap inconsistent chunks: every chunk is checked in order.
// status[0] = 0 when the chain is consistent, else 1 + the chunk where it broke.
template <bool kExact>
__global__ __launch_bounds__(64) void lz4_bare_fix(const uint8_t *__restrict__ in, size_t in_len,
                                                   size_t nchunks, uint64_t *__restrict__ cand,
                                                   uint32_t *__restrict__ cnt,
                                                   uint64_t *__restrict__ exitp,
                                                   unsigned long long *__restrict__ gsum,
                                                   const unsigned int *__restrict__ nmis_p,
                                                   const unsigned int *__restrict__ mis,
                                                   unsigned long long *__restrict__ status,
                                                   uint32_t *__restrict__ lok) {
  __shared__ unsigned int list[kMisCap];
  const int lane = threadIdx.x;
  const unsigned int nmis = *nmis_p;
  const bool all = nmis > (unsigned)kMisCap;         // too many: check every chunk
  const int nl = all ? 0 : (int)nmis;
  for (int i = lane; i < nl; i += 64) list[i] = mis[i];
  __syncthreads();
  size_t ov_c = ~(size_t)0;                          // chunk re-walked last, and its exit
  uint64_t ov_exit = 0;                              // (a later load may not see the store)
  size_t pos = 0;                                    // chunks below pos are consistent
  size_t force = ~(size_t)0;                         // a re-walked chunk, checked next
  unsigned long long st = 0;
  for (;;) {
    size_t f;
    if (force != ~(size_t)0) {
      f = force;
    } else if (all) {
      f = pos;                                       // (slow path: every chunk in order)
    } else {
      size_t m = ~(size_t)0;                         // smallest listed chunk >= pos
      for (int i = lane; i < nl; i += 64)
        if (list[i] >= pos && list[i] < m) m = list[i];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const size_t o = __shfl_xor(m, d, 64);
        m = o < m ? o : m;
      }
      f = m;
    }
    if (f >= nchunks) break;
    force = ~(size_t)0;
    const uint64_t e = f == ov_c ? ov_exit : exitp[f];
    const bool bad =
        e == kBad || (f + 1 < nchunks ? e != cand[f + 1] : e != (uint64_t)in_len);
    if (!bad) {
      pos = f + 1;
      continue;
    }
    if (f + 1 >= nchunks || e == kBad) {             // no way on: a corrupt stream
      st = 1 + f;
      break;
    }
    // chunk f + 1 starts where chunk f's walk left off
    uint32_t n = 0;
    uint64_t ex = 0;
    if (lane == 0) ex = bare_walk_chunk<kExact, false>(in, in_len, f + 1, e, n, nullptr, 0);
    ex = __shfl(ex, 0, 64);
    n = (uint32_t)__shfl((int)n, 0, 64);
    if (lane == 0) {
      const uint32_t old = cnt[f + 1];
      cand[f + 1] = e;
      cnt[f + 1] = n;
      exitp[f + 1] = ex;
      lok[f + 1] = 0u;                               // its list is stale: re-walked for offsets
      atomicAdd(&gsum[(f + 1) / 64], (unsigned long long)n - (unsigned long long)old);
    }
    ov_c = f + 1;
    ov_exit = ex;
    pos = f + 1;
    force = f + 1;
  }
  if (lane == 0) status[0] = st;
}

// exclusive scan of the per-wave block counts (one workgroup) -> gbase; the
// total block count -> *nb
__global__ __launch_bounds__(1024) void lz4_bare_scan(const unsigned long long *__restrict__ gsum,
                                                      size_t ng,
                                                      unsigned long long *__restrict__ gbase,
                                                      unsigned long long *__restrict__ nb) {
  __shared__ unsigned long long ws[16];
  __shared__ unsigned long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (size_t c0 = 0; c0 < ng; c0 += 1024) {
    const size_t i = c0 + threadIdx.x;
    const unsigned long long v = i < ng ? gsum[i] : 0;
    unsigned long long x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(x, d, 64);
      if ((threadIdx.x & 63) >= d) x += o;
    }
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = x;
    __syncthreads();
    unsigned long long pre = carry;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pre += ws[w];
    if (i < ng) gbase[i] = pre + x - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = pre + x;
    __syncthreads();
  }
  if (threadIdx.x == 0) *nb = carry;
}

// a lane per chunk: its blocks' offsets (relative to the first block byte)
template <bool kExact>
__global__ __launch_bounds__(64) void lz4_bare_offsets(const uint8_t *__restrict__ in,
                                                       size_t in_len, size_t nchunks,
                                                       const uint64_t *__restrict__ cand,
                                                       const uint32_t *__restrict__ cnt,
                                                       const unsigned long long *__restrict__ gbase,
                                                       uint64_t *__restrict__ boff,
                                                       uint64_t boff_cap,
                                                       const uint16_t *__restrict__ lists,
                                                       const uint32_t *__restrict__ lok) {
  const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
  const uint32_t v = c < nchunks ? cnt[c] : 0u;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)x, d, 64);
    if ((int)threadIdx.x >= d) x += o;
  }
  // the wave's offsets are one contiguous range [wbase, wbase + total):
  // staged in LDS and stored coalesced when they fit, else stored per lane
  constexpr int kStageN = 1024;
  __shared__ uint64_t st[kStageN];
  const uint32_t total = (uint32_t)__shfl((int)x, 63, 64);
  const uint64_t wbase = gbase[blockIdx.x];
  const bool staged = total <= (uint32_t)kStageN;
  if (c < nchunks) {
    const uint32_t rel = x - v;
    if (lok[c]) {
      // the walk's list: no second walk of the chain (its loads wait on
      // memory once per block)
      const uint64_t c0 = 1 + c * (uint64_t)kChunkB;
      const uint16_t *l = lists + c * kList;
      for (uint32_t i = 0; i < v; ++i) {
        const uint64_t o = c0 + l[i] - 1;
        if (staged) st[rel + i] = o;
        else if (wbase + rel + i < boff_cap) boff[wbase + rel + i] = o;
      }
    } else {
      uint32_t n = 0;
      if (staged)
        bare_walk_chunk<kExact, true>(in, in_len, c, cand[c], n, st, rel, (uint64_t)kStageN);
      else
        bare_walk_chunk<kExact, true>(in, in_len, c, cand[c], n, boff, wbase + rel, boff_cap);
    }
  }
  if (staged) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < total; i += 64)
      if (wbase + i < boff_cap) boff[wbase + i] = st[i];
  }
}

// One thread: the chain's verdict before any block is decoded -- kGateGo,
// kGateCorrupt (a broken chain, no block, or a frame byte that is not the
// block count mod 256) or kGateCapacity (more blocks than the output can
// hold, and so than the offsets array) -- and the decoder's result slots reset.
__global__ void lz4_bare_gate(const uint8_t *__restrict__ in, unsigned long long *small,
                              uint64_t nb_cap) {
  const unsigned long long nb = small[kCtlNb], st = small[kCtlStatus];
  unsigned long long g = kGateGo;
  if (st != 0 || nb == 0 || (uint8_t)(nb & 0xFF) != in[0]) g = kGateCorrupt;
  else if (nb > nb_cap) g = kGateCapacity;
  small[kCtlLen] = 0ull;
  small[kCtlFail] = ~0ull;
  small[kCtlGate] = g;
}

// the same reset of the result pair where the caller supplies the offsets
// (lz4r_decompress_device; defined here, after the gate, to keep the code
// object's kernel order)
__global__ void lz4_decode_init(unsigned long long *result) {
  result[kResLen] = 0ull;
  result[kResFail] = ~0ull;
}

}  // namespace
