// lz4f_dec.h -- the kernels that decode standard LZ4 frames on the GPU
// (lz4r_frame_decompress_device; the host side is lz4f_gpudec.hip).  What a
// frame means is in lz4f_parse.h, shared with the host; here is only how the
// work is spread:
//
//   lz4f_walk          one wave follows the block size words from frame to
//                      frame: the block index, the frame table, the counts
//   lz4f_xxh32_items   a wave per item: the block checksums (over the input),
//                      or the content checksums (over a frame's decoded bytes)
//   lz4f_dec_sizes     a wave per data block: its decoded length from its
//                      tokens alone
//   lz4f_dec_scan      one workgroup: the blocks' output offsets and the total
//                      (scan_partials of lz4r_scan.h), the frames' content sizes
//   lz4f_dec_blocks    a wave per chain (an independent or stored block, or a
//                      linked frame's blocks in order): the sequence walk is
//                      serial, every literal run and match copy is spread over
//                      the 64 lanes
//
// A wave reads the input through a window of kWin bytes in LDS that it fills
// with coalesced 16-byte loads (Window): the parse is then a chain of LDS
// reads, wave-uniform, and the shared parsers see it as `Src`.  Workgroups
// are 4 waves with a window each and never meet at a barrier: 16 KiB of LDS
// per workgroup, so LDS admits 10 workgroups per CU and the 32-wave cap of a
// CU (8 workgroups) binds first -- full occupancy as long as a kernel stays
// within 64 VGPRs: lz4f_dec_sizes does (60), lz4f_dec_blocks takes 82 and
// runs 5 waves per SIMD, 20 per CU.
//
// Matches are served from global memory: a block maximum is up to 4 MiB and a
// linked frame's window 64 KiB, neither of which leaves room for more than two
// waves per CU in LDS.  A match reads bytes that other lanes of the same wave
// stored, so the wave waits for its stores (a workgroup-scope release and
// s_waitcnt vmcnt(0)) before it loads a source range it has written since its
// last wait, and loads the source as a workgroup-scope atomic: the CU's L1 is
// coherent for the waves of one CU, which is all this needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4f_parse.h"
#include "lz4r_scan.h"
#include "wave64.h"

namespace {

constexpr int kWin = 4096;                // bytes of a wave's input window
constexpr int kLand = 1024;               // bytes the walk fetches where a far hop lands
constexpr int kFWaves = 4;                // waves of a workgroup
constexpr int kFThreads = 64 * kFWaves;

// control words of a call (uint64 each), read back by the host
enum {
  kFNb = 0,        // data blocks of all frames
  kFNf,            // frames
  kFNsum,          // frames that carry a content checksum
  kFStatus,        // != 0: the walk or a content size says corrupt
  kFBad,           // 1 + the first block that does not decode or fails a checksum; ~0: none
  kFTotal,         // decoded bytes of all frames
  kFWords = 8
};

__device__ __forceinline__ uint32_t uniform(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// the 16 bytes at buf + g, those outside buf[0, len) as zeros
__device__ __forceinline__ uint4 window_chunk(const uint8_t *buf, size_t len, int64_t g) {
  if (g >= 0 && (uint64_t)g + 16 <= len) return *reinterpret_cast<const uint4 *>(buf + g);
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll 1
    for (int j = 4 * q; j < 4 * q + 4; ++j)
      if (g + j >= 0 && (uint64_t)(g + j) < len) w[q] |= (uint32_t)buf[g + j] << (8 * (j & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// lds[0, bytes) = buf[nb, nb + bytes), zeros outside buf[0, len); buf + nb is
// 16-byte aligned, bytes a multiple of 1024 up to kWin.  Out of line: a
// window is filled once per kWin bytes, and inlined at every read of the
// parsers it costs them half their occupancy.
__device__ __noinline__ void window_fill(const uint8_t *buf, size_t len, uint8_t *lds, int64_t nb,
                                         int bytes) {
  const int lane = threadIdx.x & 63;
  if (nb >= 0 && (uint64_t)(nb + bytes) <= len) {
    if (bytes == kWin) {
#pragma unroll
      for (int k = 0; k < kWin / 1024; ++k)
        *reinterpret_cast<uint4 *>(lds + (k * 64 + lane) * 16) =
            *reinterpret_cast<const uint4 *>(buf + nb + (k * 64 + lane) * 16);
    } else {
      for (int k = 0; k < bytes / 1024; ++k)
        *reinterpret_cast<uint4 *>(lds + (k * 64 + lane) * 16) =
            *reinterpret_cast<const uint4 *>(buf + nb + (k * 64 + lane) * 16);
    }
  } else {                                              // at either end of buf
#pragma unroll 1
    for (int k = 0; k < bytes / 1024; ++k)
      *reinterpret_cast<uint4 *>(lds + (k * 64 + lane) * 16) =
          window_chunk(buf, len, nb + (k * 64 + lane) * 16);
  }
}

// buf[0, len) seen through kWin bytes of LDS: lds[k] = buf[base + k], with
// buf + base 16-byte aligned.  Every call is the whole wave's, with uniform
// arguments.  Nothing outside buf[0, len) is read: a 16-byte chunk that
// straddles either end is read byte by byte.
// kAhead (the walk): the window after this one is loaded into registers while
// this one is in use, and becomes the window without another wait if that is
// where the walk goes next.  A hop of the walk that lands far from the window
// (two windows or more ahead, as every hop over a block of this library's
// frames does) fetches kLand bytes there, one load a lane, and no window
// ahead: what it came for is a size word, and the next hop is as far again.
// Reads that then run on past the kLand bytes get the whole window.
template <bool kAhead>
struct Window {
  const uint8_t *buf;
  size_t len;
  uint8_t *lds;
  int64_t base;
  uint32_t valid;                                       // lds[0, valid) holds buf: kWin, or kLand
  uint4 ahead[kAhead ? kWin / 1024 : 1];
  int64_t ahead_base;                                   // < 0: none

  __device__ Window(const uint8_t *b, size_t n, uint8_t *l)
      : buf(b), len(n), lds(l), base(INT64_MIN / 2), valid(kWin), ahead_base(-1) {}

  __device__ void fill(size_t i) {
    const int lane = threadIdx.x & 63;
    int64_t nb = (int64_t)i - (int64_t)(reinterpret_cast<uintptr_t>(buf + i) & 15);
    wave_sync();
    if (kAhead && (uint64_t)(nb - base) >= (uint64_t)(2 * kWin)) {     // a far hop (or the first)
      window_fill(buf, len, lds, nb, kLand);
      base = nb;
      valid = kLand;
      ahead_base = -1;
      wave_sync();
      return;
    }
    valid = kWin;
    if (kAhead && ahead_base >= 0 && nb >= ahead_base && nb < ahead_base + kWin) {
      nb = ahead_base;
#pragma unroll
      for (int k = 0; k < kWin / 1024; ++k)
        *reinterpret_cast<uint4 *>(lds + (k * 64 + lane) * 16) = ahead[k];
    } else {
      window_fill(buf, len, lds, nb, kWin);
    }
    base = nb;
    if (kAhead) {
      ahead_base = (uint64_t)(nb + 2 * kWin) <= len ? nb + kWin : -1;   // whole chunks only
      if (ahead_base >= 0) {
#pragma unroll
        for (int k = 0; k < kWin / 1024; ++k)
          ahead[k] = *reinterpret_cast<const uint4 *>(buf + ahead_base + (k * 64 + lane) * 16);
      }
    }
    wave_sync();
  }

  // byte i of buf, i < len, wave-uniform
  __device__ __forceinline__ uint32_t at(size_t i) {
    if ((uint64_t)((int64_t)i - base) >= (uint64_t)(kAhead ? valid : kWin)) fill(i);
    return uniform(lds[(int64_t)i - base]);
  }

  // [i, i + 16) in the window (kWin > 31); then raw(j) is byte j of it, per lane
  __device__ __forceinline__ void ensure16(size_t i) {
    if ((uint64_t)((int64_t)i - base) > (uint64_t)(kWin - 16)) fill(i);
  }
  __device__ __forceinline__ uint32_t raw(size_t j) const { return lds[(int64_t)j - base]; }
};

__device__ __forceinline__ void block_fails(unsigned long long *ctl, size_t b) {
  if ((threadIdx.x & 63) == 0) atomicMin(ctl + kFBad, (unsigned long long)b + 1);
}

// ---- the walk ------------------------------------------------------------------

struct IndexSink {
  Lz4fBlock *blocks;
  size_t cap_blocks;
  Lz4fFrame *frames;
  size_t cap_frames;
  bool writer;
  __device__ void block(uint64_t i, const Lz4fBlock &b) {
    if (writer && i < cap_blocks) blocks[i] = b;
  }
  __device__ void frame(uint64_t i, const Lz4fFrame &f) {
    if (writer && i < cap_frames) frames[i] = f;
  }
};

// One wave.  A hop is a dependent load: the next size word's place is known
// only when this one has arrived, so the walk costs a memory latency per data
// block whose successor lies outside the two windows, and an LDS read per
// block inside them.  The counts are exact even where the index had no room
// (the host, which reads them back, then walks again with room).  A corrupt
// walk counts no blocks.
__global__ __launch_bounds__(64) void lz4f_walk(const uint8_t *__restrict__ in, size_t in_len,
                                                Lz4fBlock *__restrict__ blocks, size_t cap_blocks,
                                                Lz4fFrame *__restrict__ frames, size_t cap_frames,
                                                unsigned long long *__restrict__ ctl) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWin];
  Window<true> w(in, in_len, lds);
  IndexSink k = {blocks, cap_blocks, frames, cap_frames, threadIdx.x == 0};
  uint64_t nb = 0, nf = 0, ns = 0;
  const int rc = lz4f_walk_frames(w, in_len, k, &nb, &nf, &ns);
  if (threadIdx.x == 0) {
    ctl[kFNb] = rc ? 0 : nb;
    ctl[kFNf] = rc ? 0 : nf;
    ctl[kFNsum] = rc ? 0 : ns;
    ctl[kFStatus] = rc ? 1 : 0;
    ctl[kFBad] = ~0ull;
    ctl[kFTotal] = 0;
  }
}

// (the kernels below run only once the index holds every block and frame)

// what the decode stages ask before they write or read the output: nothing
// said corrupt so far, and the whole output fits
__device__ __forceinline__ bool decode_gate(const unsigned long long *ctl, size_t out_cap) {
  return ctl[kFStatus] == 0 && ctl[kFBad] == ~0ull && ctl[kFTotal] <= out_cap;
}

// ---- checksums -----------------------------------------------------------------

// xxh32 of buf[p, p + n) by one wave (seed 0).  The four accumulators sit in
// lanes 0-3, a stripe is 16 bytes of the window; the digest is lz4f_xxh32.h's.
// xxh32 has no combine step: this is serial over the n bytes.
__device__ uint32_t wave_xxh32(Window<false> &w, size_t p, size_t n) {
  const int lane = threadIdx.x & 63;
  lz4f_xxh32_state st;
  lz4f_xxh32_init(&st, 0);
  uint32_t acc = st.v[lane & 3];
  const size_t stripes = n / 16;
  for (size_t s = 0; s < stripes; ++s) {
    const size_t q = p + 16 * s;
    w.ensure16(q);
    const size_t j = q + 4 * (lane & 3);
    const uint32_t word = w.raw(j) | w.raw(j + 1) << 8 | w.raw(j + 2) << 16 | w.raw(j + 3) << 24;
    acc = lz4f_round(acc, word);
  }
  for (int k = 0; k < 4; ++k) st.v[k] = (uint32_t)__builtin_amdgcn_readlane((int)acc, k);
  st.total = n;
  st.nbuf = (uint32_t)(n & 15);
  for (uint32_t k = 0; k < st.nbuf; ++k) st.buf[k] = (uint8_t)w.at(p + 16 * stripes + k);
  return lz4f_xxh32_digest(&st);
}

// the four bytes at in[pos ...), pos + 4 <= in_len (the walk saw to that)
__device__ __forceinline__ uint32_t load_le32(const uint8_t *in, size_t pos) {
  return (uint32_t)in[pos] | (uint32_t)in[pos + 1] << 8 | (uint32_t)in[pos + 2] << 16 |
         (uint32_t)in[pos + 3] << 24;
}

// kContent false: every data block whose frame flags block checksums, over its
// bytes in the input.  kContent true: every frame that carries a content
// checksum, over its decoded bytes -- one wave per frame, serial.
template <bool kContent>
__global__ __launch_bounds__(kFThreads) void lz4f_xxh32_items(
    const uint8_t *__restrict__ in, size_t in_len, const Lz4fBlock *__restrict__ blocks,
    const Lz4fFrame *__restrict__ frames, const uint64_t *__restrict__ off,
    const uint8_t *__restrict__ out, size_t out_cap, unsigned long long *__restrict__ ctl) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kFWaves][kWin];
  const size_t wave = (size_t)blockIdx.x * kFWaves + (threadIdx.x >> 6);
  const size_t nwaves = (size_t)gridDim.x * kFWaves;
  if (kContent) {
    if (!decode_gate(ctl, out_cap)) return;             // nothing was decoded
    const size_t nf = (size_t)ctl[kFNf], nb = (size_t)ctl[kFNb], total = (size_t)ctl[kFTotal];
    for (size_t f = wave; f < nf; f += nwaves) {
      const Lz4fFrame fr = frames[f];
      if (!fr.has_csum) continue;
      const size_t lo = fr.nblocks ? (size_t)off[fr.first_block] : 0;
      const size_t last = (size_t)(fr.first_block + fr.nblocks);
      const size_t hi = fr.nblocks ? (last < nb ? (size_t)off[last] : total) : 0;
      Window<false> w(out, total, lds[threadIdx.x >> 6]);
      if (wave_xxh32(w, lo, hi - lo) != load_le32(in, (size_t)fr.csum_pos))
        block_fails(ctl, (size_t)fr.first_block);
    }
  } else {
    const size_t nb = (size_t)ctl[kFNb];
    for (size_t b = wave; b < nb; b += nwaves) {
      const Lz4fBlock e = blocks[b];
      if (!(e.word & kLz4fBsum)) continue;
      const size_t n = lz4f_block_bytes(e.word);
      Window<false> w(in, in_len, lds[threadIdx.x >> 6]);
      if (wave_xxh32(w, (size_t)e.in_off, n) != load_le32(in, (size_t)e.in_off + n))
        block_fails(ctl, b);
    }
  }
}

// ---- sizes ---------------------------------------------------------------------

__global__ __launch_bounds__(kFThreads) void lz4f_dec_sizes(
    const uint8_t *__restrict__ in, size_t in_len, const Lz4fBlock *__restrict__ blocks,
    uint32_t *__restrict__ sizes, uint64_t *__restrict__ off,
    unsigned long long *__restrict__ ctl) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kFWaves][kWin];
  const size_t wave = (size_t)blockIdx.x * kFWaves + (threadIdx.x >> 6);
  const size_t nwaves = (size_t)gridDim.x * kFWaves;
  const size_t nb = (size_t)ctl[kFNb];
  for (size_t b = wave; b < nb; b += nwaves) {
    const Lz4fBlock e = blocks[b];
    uint32_t n = lz4f_block_bytes(e.word);              // a stored block: its byte count
    if (!(e.word & kLz4fStored)) {
      Window<false> w(in, in_len, lds[threadIdx.x >> 6]);
      const size_t ip = (size_t)e.in_off;
      if (lz4f_block_size(w, ip, ip + n, lz4f_block_max(e.word), &n)) {
        n = 0;
        block_fails(ctl, b);
      }
    }
    if ((threadIdx.x & 63) == 0) {
      sizes[b] = n;
      off[b] = n;
    }
  }
}

// ---- scan ----------------------------------------------------------------------

// off[b]: the sizes -> the blocks' output offsets, their sum -> ctl[kFTotal];
// then every frame's content size against its blocks' sum.
__global__ __launch_bounds__(1024) void lz4f_dec_scan(uint64_t *__restrict__ off,
                                                      const Lz4fFrame *__restrict__ frames,
                                                      unsigned long long *__restrict__ ctl) {
  const size_t nb = (size_t)ctl[kFNb], nf = (size_t)ctl[kFNf];
  scan_partials(off, nb, 0, 1, 0, nullptr, reinterpret_cast<uint64_t *>(ctl + kFTotal), nullptr);
  __syncthreads();
  const uint64_t total = ctl[kFTotal];
  for (size_t f = threadIdx.x; f < nf; f += 1024) {
    const Lz4fFrame fr = frames[f];
    if (!fr.has_want) continue;
    const size_t last = (size_t)(fr.first_block + fr.nblocks);
    const uint64_t lo = fr.first_block < nb ? off[fr.first_block] : total;
    const uint64_t hi = last < nb ? off[last] : total;
    if (hi - lo != fr.want) ctl[kFStatus] = 1;
  }
}

// ---- blocks --------------------------------------------------------------------

// n bytes from src to dst by the wave; src and dst do not overlap.  Long
// copies go as aligned 16-byte stores.
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, size_t n) {
  const size_t lane = threadIdx.x & 63;
  if (n < 256) {
    for (size_t i = lane; i < n; i += 64) dst[i] = src[i];
    return;
  }
  const size_t head = (size_t)(-reinterpret_cast<uintptr_t>(dst) & 15);
  if (lane < head) dst[lane] = src[lane];
  const size_t chunks = (n - head) / 16;
  for (size_t c = lane; c < chunks; c += 64) {
    uint4 v;
    __builtin_memcpy(&v, src + head + 16 * c, 16);
    *reinterpret_cast<uint4 *>(dst + head + 16 * c) = v;
  }
  for (size_t i = head + 16 * chunks + lane; i < n; i += 64) dst[i] = src[i];
}

// a byte another lane of this wave may have stored
__device__ __forceinline__ uint8_t load_written(const uint8_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The copies of a chain, spread over the wave's lanes.  clean: every store to
// out[0, clean) has completed.
struct WaveOut {
  const uint8_t *in;
  uint8_t *out;
  size_t clean;

  __device__ void literals(size_t op, size_t lit, uint32_t L) {
    if (L) wave_copy(out + op, in + lit, L);
  }

  // D <= op - base, so the source lies wholly before op: with D < M it is
  // periodic, byte i = out[op - D + i % D], and the whole match is one
  // parallel copy all the same
  __device__ void match(size_t op, uint32_t D, uint32_t M) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t src = op - D;
    if (src + (D < M ? D : M) > clean) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      clean = op;
    }
    if (D >= M) {
      for (uint32_t i = lane; i < M; i += 64) out[op + i] = load_written(out + src + i);
    } else {
      uint32_t r = lane % D;
      const uint32_t step = 64 % D;
      for (uint32_t i = lane; i < M; i += 64) {
        out[op + i] = load_written(out + src + r);
        r += step;
        if (r >= D) r -= D;
      }
    }
  }
};

// A wave per chain, found from the block index: an independent or stored
// block is its own chain; a linked frame's first block leads the chain of all
// its blocks and the others are skipped.  Nothing is decoded unless the whole
// output fits (decode_gate: ctl[kFTotal] <= out_cap, decided here on the
// device, with no read-back), and a block never writes past the end the sizes
// pass found for it, so nothing at or past out_cap is written.
__global__ __launch_bounds__(kFThreads) void lz4f_dec_blocks(
    const uint8_t *__restrict__ in, size_t in_len, const Lz4fBlock *__restrict__ blocks,
    const Lz4fFrame *__restrict__ frames, const uint32_t *__restrict__ sizes,
    const uint64_t *__restrict__ off, uint8_t *out, size_t out_cap,
    unsigned long long *__restrict__ ctl) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kFWaves][kWin];
  if (!decode_gate(ctl, out_cap)) return;
  const size_t wave = (size_t)blockIdx.x * kFWaves + (threadIdx.x >> 6);
  const size_t nwaves = (size_t)gridDim.x * kFWaves;
  const size_t nb = (size_t)ctl[kFNb];
  for (size_t lead = wave; lead < nb; lead += nwaves) {
    const Lz4fBlock first = blocks[lead];
    size_t count = 1;
    if (first.word & kLz4fLinked) {
      const Lz4fFrame fr = frames[first.frame];
      if (fr.first_block != lead) continue;
      count = (size_t)fr.nblocks;
    }
    const size_t base = (size_t)off[lead];
    WaveOut o = {in, out, base};
    Window<false> w(in, in_len, lds[threadIdx.x >> 6]);
    for (size_t b = lead; b < lead + count; ++b) {
      const Lz4fBlock e = blocks[b];
      const size_t ip = (size_t)e.in_off, n = lz4f_block_bytes(e.word);
      size_t op = (size_t)off[b];
      const size_t end = op + sizes[b];
      if (e.word & kLz4fStored) {
        o.literals(op, ip, (uint32_t)n);
      } else if (lz4f_decode_block(w, ip, ip + n, o, base, &op, end) || op != end) {
        block_fails(ctl, b);
        break;                                          // the rest of a chain builds on this block
      }
    }
  }
}

}  // namespace
