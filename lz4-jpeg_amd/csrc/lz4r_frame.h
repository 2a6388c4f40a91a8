// lz4r_frame.h -- the same parse as a standard LZ4 frame (LZ4 Frame Format
// 1.6.x, independent 64 KiB-class blocks, content size, no checksums): a second
// emission path over the sequence records lz4_tiles leaves (lz4r_layout.h).
// A data block of the frame = one scan group: kGT source blocks, 19,200 input
// bytes (the call's last one: what is left).  Positions below count from the
// data block's start, N is its input length.  Its sequences are its source
// blocks' records in order, under the block format's end rules:
//   1  a record with M < 4 is no match: its M bytes are literals (the
//      literal-only tail, and the reference's uint8_t quirks: a 256-long match
//      parsed as a literal, 257..259 stored as M = 1..3)
//   2  a match that starts after N - 12 is no match: its bytes are literals
//   3  a match that starts at or before N - 12 and ends after N - 5 is cut to
//      end at N - 5 (its length stays >= 7)
//   4  literal runs merge over source-block boundaries and demoted records: a
//      kept match's literals start where the previous kept match ended
//   5  token min(L,15) << 4 | min(ML-4,15); L - 15 as 255-bytes and a final
//      byte < 255; the literals; u16 distance; ML - 19 the same way
//   6  the last sequence is token, extension and literals, no offset
// Three launches per chunk in place of the native path's three:
//   lz4f_sizes   one workgroup per data block: the 64 record heads (6 KB,
//                contiguous) -> 4 + the data block's byte count.  Records
//                only, no input.
//   lz4f_scan    lz4r_scan.h's scan_partials over those counts (1/64 of the
//                native scan's items) -> every data block's stream offset; the
//                first chunk's writes the 15 header bytes the host computed,
//                the last chunk's the EndMark and the final length.
//   lz4f_emit    one workgroup per data block: its input staged in LDS, the
//                same plan again, token / extension / offset bytes by ds_or
//                into a zeroed LDS image, literal runs flattened over each
//                wave's lanes from the staged input, then emit_store
//                (lz4r_emit.h): aligned 16-B stores, nothing at or past cap.
// frame_plan is the one place that classifies and places sequences; both
// kernels call it.  No workgroup waits on another.
// HBM traffic per input byte: sizes ~0.33 B read (heads; overflow slots of
// blocks with > 23 records), emit 1 B + ~0.33 B read and <= 1.004 B written.
#pragma once
#include "lz4r_emit.h"
#include "lz4r_layout.h"
#include "lz4r_scan.h"
#include "wave64.h"

namespace {

constexpr int kFW = kEW;                               // waves per workgroup (emit_store's)
constexpr int kFrameIn = kGT * kBlk;                   // input bytes of a data block
// A kept match adds 3 + its extensions and saves >= 4, so a sequence expands
// the bytes it covers by at most L / 255; the last run adds its token and one
// more extension byte.
constexpr int kFrameBlkMax = kFrameIn + kFrameIn / 255 + 2;
constexpr int kFrameImg = (15 + 4 + kFrameBlkMax + 8 + 15) & ~15;   // lead, size, bytes, ds_or's reach
constexpr int kFrameHdr = 15;                          // magic, FLG, BD, content size, HC
constexpr uint32_t kMaxRec = 121;                      // records of one source block

// bytes of a length extension: x - 15 as 255-bytes and a final byte
__device__ __forceinline__ int ext_bytes(int x) { return x >= 15 ? (x - 15) / 255 + 1 : 0; }

// Exclusive scan (max or add) of v over the workgroup, continued from carry;
// ws: kFW words of this scan's own.  One barrier: a scan's words are read
// before the workgroup's next barrier and written again only after it.
template <bool kMax>
__device__ __forceinline__ uint32_t wg_excl(uint32_t v, uint32_t &carry, uint32_t *ws, int lane,
                                            int wv) {
  const uint32_t inc = kMax ? wave_incl_max(v) : wave_incl_add(v);
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  uint32_t pre = carry, tot = carry;
#pragma unroll
  for (int w = 0; w < kFW; ++w) {
    const uint32_t x = ws[w];
    if (w < wv) pre = kMax ? max(pre, x) : pre + x;
    tot = kMax ? max(tot, x) : tot + x;
  }
  carry = tot;
  const uint32_t up = dpp<0x138, 0xf, 0xf>(inc);       // wave_shr:1 (lane 0: 0)
  return kMax ? max(pre, up) : pre + up;
}

// The plan of one data block (all 64 kFW threads call): its nblk source
// blocks' records (heads in recst, records 23.. in the overflow slots wovf)
// take the flattened indices 0 .. T-1, index T is the last sequence.  Every
// index is classified by rules 1-3; an exclusive max-scan of the kept
// matches' ends gives each kept match its literal run's start (positions grow,
// so the maximum is the previous kept end), an exclusive sum of the sequences'
// bytes its place.  visit(kept, last, run, L, ML, D, off) is called by every
// thread for every round of 64 kFW indices: a kept sequence's literals are
// bytes [run, run + L) of the data block, its match ML bytes at distance D,
// its token at byte off of the data block's bytes.  Returns their count.
template <class Visit>
__device__ __forceinline__ uint32_t frame_plan(const int tid, const uint32_t (*recst)[kHeadW],
                                               const uint8_t *__restrict__ wovf, const int nblk,
                                               const int N, uint32_t *starts, uint32_t (*ws)[kFW],
                                               Visit &&visit) {
  const int lane = tid & 63, wv = tid >> 6;
  if (wv == 0) {                       // the blocks' record counts -> first flattened index
    const uint32_t cnt = lane < nblk ? min(recst[lane][0] >> 16, kMaxRec) : 0u;
    const uint32_t inc = wave_incl_add(cnt);
    starts[lane] = inc - cnt;
    if (lane == 63) starts[kGT] = inc;
  }
  __syncthreads();
  const int T = (int)starts[kGT];
  uint32_t cmax = 0, csum = 0;
  for (int f0 = 0; f0 <= T; f0 += 64 * kFW) {
    const int f = f0 + tid;
    bool kept = f == T;
    int start = N, endc = N;
    uint32_t D = 0;
    if (f < T) {
      int b = 0;                       // the last block that starts at or before f
#pragma unroll
      for (int s = kGT / 2; s; s >>= 1)
        if ((int)starts[b + s] <= f) b += s;
      const int k = f - (int)starts[b];
      const uint32_t r = 1 + k < kHeadW
                             ? recst[b][1 + k]
                             : reinterpret_cast<const uint32_t *>(wovf + (size_t)b * kOvf)[1 + k - kHeadW];
      const int M = (int)((r >> 9) & 255u);
      const int end = kBlk * b + (int)(r >> 19);
      D = r & 511u;
      start = end - M;
      kept = M >= 4 && start <= N - 12;          // rules 1, 2
      endc = min(end, N - 5);                    // rule 3
    }
    const int run = (int)wg_excl<true>(kept ? (uint32_t)endc : 0u, cmax, ws[0], lane, wv);
    const int L = start - run, ML = endc - start;
    const bool last = f == T;
    const int bytes = !kept ? 0 : 1 + ext_bytes(L) + L + (last ? 0 : 2 + ext_bytes(ML - 4));
    const uint32_t off = wg_excl<false>((uint32_t)bytes, csum, ws[1], lane, wv);
    visit(kept, last, run, L, ML, D, off);
  }
  return csum;
}

// the 64 record heads of a data block -> LDS (one contiguous run of 16-B loads)
__device__ __forceinline__ void load_heads(const int tid, const uint8_t *__restrict__ wheads,
                                           const int nblk, uint32_t (*recst)[kHeadW]) {
  constexpr int kPerSlot = kHeadW / 4;
  for (int i = tid; i < nblk * kPerSlot; i += 64 * kFW) {
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wheads) + i);
    reinterpret_cast<uint4 *>(&recst[0][0])[i] = make_uint4(t.x, t.y, t.z, t.w);
  }
}

// heads, ovfs: the launch chunk's; dsz[g] = 4 + the bytes of data block g of it
__global__ __launch_bounds__(64 * kFW) void lz4f_sizes(const uint8_t *__restrict__ heads,
                                                        const uint8_t *__restrict__ ovfs,
                                                        uint32_t ntiles, uint32_t last_n,
                                                        uint64_t *__restrict__ dsz) {
  __shared__ alignas(16) uint32_t recst[kGT][kHeadW];
  __shared__ uint32_t starts[kGT + 1];
  __shared__ uint32_t ws[2][kFW];
  const int tid = threadIdx.x;
  const uint32_t g = blockIdx.x, b0 = g * kGT;
  const int nblk = (int)min((uint32_t)kGT, ntiles - b0);
  const int N = (nblk - 1) * kBlk + (b0 + (uint32_t)nblk == ntiles ? (int)last_n : kBlk);
  load_heads(tid, heads + (size_t)b0 * kHead, nblk, recst);
  __syncthreads();
  const uint32_t total =
      frame_plan(tid, recst, ovfs + (size_t)b0 * kOvf, nblk, N, starts, ws,
                 [](bool, bool, int, int, int, uint32_t, uint32_t) {});
  if (tid == 0) dsz[g] = 4u + (uint64_t)total;
}

// The counts -> absolute stream offsets, in place (scan_partials: the carry
// over chunks in *len, the corrupt-index verdict in bit 63 and *verdict), and
// the frame's own bytes: the first chunk's writes the header (h0: bytes 0-7,
// h1: bytes 8-14), the last chunk's the EndMark, and adds it to the length.
__global__ __launch_bounds__(1024) void lz4f_scan(uint64_t *__restrict__ doff, size_t ng, int first,
                                                  int last, uint32_t *__restrict__ status,
                                                  uint64_t *len, uint64_t *__restrict__ verdict,
                                                  uint8_t *__restrict__ out, uint64_t cap,
                                                  uint64_t h0, uint64_t h1) {
  scan_partials(doff, ng, (uint64_t)kFrameHdr, first, last, status, len, verdict);
  if (threadIdx.x == 0) {
    if (first)
      for (uint64_t i = 0; i < (uint64_t)kFrameHdr && i < cap; ++i)
        out[i] = (uint8_t)((i < 8 ? h0 >> (8 * i) : h1 >> (8 * (i - 8))) & 255u);
    if (last) {
      const uint64_t v = *len, pos = v & ~kLenCorrupt;
      for (uint64_t i = pos; i < pos + 4 && i < cap; ++i) out[i] = 0;
      *len = v + 4;
    }
  }
}

// a length extension at image byte x: v as 255-bytes and a final byte; -> the byte after
__device__ __forceinline__ int put_ext(uint32_t *img32, int x, int v) {
  for (; v >= 255; v -= 255) or_bytes(img32, x++, 255u);
  or_bytes(img32, x++, (uint32_t)v);
  return x;
}

// in, heads, ovfs, doff: the launch chunk's (data block g of it: input bytes
// [19200 g, 19200 g + N), stream bytes from doff[g])
__global__ __launch_bounds__(64 * kFW) void lz4f_emit(const uint8_t *__restrict__ in,
                                                       const uint8_t *__restrict__ heads,
                                                       const uint8_t *__restrict__ ovfs,
                                                       uint32_t ntiles, uint32_t last_n,
                                                       const uint64_t *__restrict__ doff,
                                                       uint8_t *__restrict__ out, uint64_t cap) {
  __shared__ alignas(16) uint8_t img[kFrameImg];
  __shared__ alignas(16) uint8_t stage[kFrameIn];
  __shared__ alignas(16) uint32_t recst[kGT][kHeadW];
  __shared__ uint32_t starts[kGT + 1];
  __shared__ uint32_t ws[2][kFW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t g = blockIdx.x, b0 = g * kGT;
  const int nblk = (int)min((uint32_t)kGT, ntiles - b0);
  const int N = (nblk - 1) * kBlk + (b0 + (uint32_t)nblk == ntiles ? (int)last_n : kBlk);
  const uint64_t G0 = doff[g];
  const uint8_t *src = in + (size_t)b0 * kBlk;
  load_heads(tid, heads + (size_t)b0 * kHead, nblk, recst);
  // ---- stage: input byte p of the data block is stage[p] -----------------------
  const int n16 = ((uintptr_t)src & 15) == 0 ? N >> 4 : 0;
  for (int i = tid; i < n16; i += 64 * kFW) {
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src) + i);
    reinterpret_cast<uint4 *>(stage)[i] = make_uint4(t.x, t.y, t.z, t.w);
  }
  for (int i = (n16 << 4) + tid; i < N; i += 64 * kFW) stage[i] = src[i];   // tail / unaligned
  for (int i = tid; i < kFrameImg / 16; i += 64 * kFW)
    reinterpret_cast<uint4 *>(img)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int lead = (int)(((uintptr_t)out + G0) & 15);   // img[lead] = stream byte G0
  uint32_t *const img32 = reinterpret_cast<uint32_t *>(img);
  uint32_t total = frame_plan(
      tid, recst, ovfs + (size_t)b0 * kOvf, nblk, N, starts, ws,
      [&](bool kept, bool last, int run, int L, int ML, uint32_t D, uint32_t off) {
        int x = lead + 4 + (int)off, dst = 0;
        if (kept) {
          or_bytes(img32, x++, (uint32_t)(min(L, 15) << 4 | (last ? 0 : min(ML - 4, 15))));
          if (L >= 15) x = put_ext(img32, x, L - 15);
          dst = x;
          x += L;
          if (!last) {
            or_bytes(img32, x, D);
            if (ML - 4 >= 15) put_ext(img32, x + 2, ML - 19);
          }
        }
        // the wave's literal runs, flattened over its lanes a byte each: byte
        // j of them belongs to the run whose inclusive count first exceeds j
        const uint32_t cw = kept ? (uint32_t)L : 0u;
        const uint32_t cinc = wave_incl_add(cw);
        const int C = (int)lane63(cinc);
        for (int w0 = 0; w0 < C; w0 += 64) {
          const uint32_t j = (uint32_t)(w0 + lane);
          int o = 0;                   // the runs that end at or before byte j
#pragma unroll
          for (int s = 32; s; s >>= 1)
            if ((uint32_t)__shfl((int)cinc, o + s - 1, 64) <= j) o += s;
          const int rs = __shfl(run, o, 64), rd = __shfl(dst, o, 64);
          const int d = (int)j - (int)((uint32_t)__shfl((int)cinc, o, 64) - (uint32_t)__shfl((int)cw, o, 64));
          if ((int)j < C) img[rd + d] = stage[rs + d];
        }
      });
  // (a plan over sound records never exceeds the bound; the store below reads
  // the image only)
  total = min(total, (uint32_t)kFrameBlkMax);
  if (tid == 0) or_bytes(img32, lead, total);
  __syncthreads();
  // ---- LDS image -> stream (aligned 16-B stores) --------------------------------
  emit_store(tid, wv, lane, G0, min(G0 + 4u + total, cap), lead, img, out);
}

}  // namespace
