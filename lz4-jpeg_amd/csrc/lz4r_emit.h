// lz4r_emit.h -- the compressor's emission pass: sequence records
// (lz4r_layout.h) -> stream bytes at the offsets the scan placed them.
// lz4_emit: workgroup = 32 consecutive blocks (half a scan group of 64).
//   offsets  the blocks' stream offsets from the partials, the group sums and
//            a wave scan; also stored to boff (the decoder's side input)
//   stage    the 32 blocks' input -> LDS (the literals' source; 16-B loads)
//   bytes    each wave takes 8 blocks and flattens their sequence records over
//            the lanes (one round = 64 sequences of one or more blocks); per
//            sequence the token / size / literal-extension / offset /
//            match-extension bytes (write_sequence, LZ4.c:365-413) and per
//            block the u8 count + u16 size header (write_block, :415-425)
//            land by aligned ds_or in a zeroed LDS image of the output range,
//            and the literal runs are flattened over the lanes as aligned
//            16-byte image words funnel-shifted out of the staged input
//   store    the image -> the stream as aligned 16-B stores (the edge chunks
//            bytewise); nothing at or past `cap` is written.
// This is the emission lz4_tiles used to do one block per wave; here a round
// serves several blocks and the kernel is bound by its HBM traffic, not by
// instruction issue as lz4_tiles is.  Splitting it off lz4_tiles took that
// kernel from 3.44 to 2.97 ms per GiB, and the scratch round trip shrank from
// ~310 B of bytes to ~100 B of records per block.
// No workgroup ever waits on another (a fused decoupled look-back ran the
// waves in lock-step at the pace of the slowest block of each round).
// lz4_emit issues every global load of a workgroup (scan inputs, record
// heads, staged input) before waiting on any: one memory round trip per
// workgroup instead of three (0.91 -> 0.75 ms per GiB).
// It reads its input and the record heads and writes the stream exactly
// once: 16-B accesses with the non-temporal hint (u32x4), -1.3 % emit time
// (tools/ab_inproc.py).
#pragma once
#include "lz4r_layout.h"
#include "wave64.h"

namespace {

constexpr int kGH = 32;                              // blocks per emit workgroup
constexpr int kEW = 8;                               // waves per emit workgroup (4 blocks each)
constexpr int kRecPre = kHeadW;                      // record dwords per block staged in LDS
constexpr int kGSplit = kGT / kGH;                   // workgroups per group
constexpr int kEmitImg = kGH * kBlkOutMax + 32;      // worst case: every block 548 B
constexpr int kStagePad = 16;                        // literal words reach 15 B before a run
constexpr int kStage = kStagePad + kGH * kBlk + 32;  // ... and 16 B past its end
static_assert(kStage < (1 << 16), "stage offsets fit 16 bits");

// OR the (<= 4) bytes of v into the zeroed byte area at offset x: two
// aligned dwords (ds_or_b32), never a misaligned access
__device__ __forceinline__ void or_bytes(uint32_t *buf32, int x, uint32_t v) {
  const uint64_t w = (uint64_t)v << (8 * (x & 3));
  atomicOr(&buf32[x >> 2], (uint32_t)w);
  atomicOr(&buf32[(x >> 2) + 1], (uint32_t)(w >> 32));
}

// Records -> bytes of one emit task (lz4_emit): wave wv takes
// blocks [h0 + 4 wv, ...) of the task's [h0, h1); the image img[lead] is
// stream byte G0; block h's input is stage[kStagePad + 300 (h - h0) + p].
__device__ __forceinline__ void emit_records(const int wv, const int lane, const int h0,
                                             const int h1, const uint64_t G0, const int lead,
                                             const uint64_t *toff, uint8_t *img,
                                             const uint8_t *stage,
                                             const uint32_t (*recst)[kRecPre],
                                             uint32_t (*marks)[64], const uint4 *pmask,
                                             const uint8_t *__restrict__ wovf) {
  {
    constexpr int kBW = kGH / kEW;                   // blocks per wave
    const int bl0 = h0 + wv * kBW, bl1 = min(h1, bl0 + kBW);
    if (bl0 < bl1) {
      uint32_t *const out32 = reinterpret_cast<uint32_t *>(img);
      const int nbk = bl1 - bl0;
      // lanes 0..nbk-1: the blocks' sequence counts -> first flattened index
      const uint32_t hd = lane < nbk ? recst[bl0 - h0 + lane][0] : 0u;
      const uint32_t ns = hd >> 16;
      const uint32_t sinc = wave_incl_add(ns);
      const int Stot = (int)lane63(sinc);
      const int sst = (int)(sinc - ns);
      int st[kBW];                                 // wave-uniform block starts
#pragma unroll
      for (int i = 0; i < kBW; ++i)
        st[i] = i < nbk ? __builtin_amdgcn_readlane(sst, i) : 0x7fffffff;
      // the wave's blocks are contiguous in the image, each its 3 header bytes
      // and then its sequences' bytes (tsz counts the bytes written): sequence f
      // lands at the wave's first image byte + 3 (its block's rank + 1) + the
      // bytes of the wave's sequences before it
      int end_prev = 0, wcur = lead + (int)(toff[bl0] - G0) + 3;
      for (int f0 = 0; f0 < Stot; f0 += 64) {
        const int f = f0 + lane;
        const bool valid = f < Stot;
        int bi = 0, sb = 0;                        // the lane's block: the last start <= f
#pragma unroll
        for (int i = 1; i < kBW; ++i) {
          const bool ge = f >= st[i];
          bi += ge ? 1 : 0;
          sb = ge ? st[i] : sb;
        }
        const int k = f - sb;                      // sequence index in the block
        const int hb = bl0 + bi;
        const uint32_t *rp = reinterpret_cast<const uint32_t *>(wovf + (hb - h0) * kOvf);
        const uint32_t r =
            !valid ? 0u : (1 + k < kRecPre ? recst[hb - h0][1 + k] : rp[1 + k - kRecPre]);
        // record = the sequence's match word: dist | M << 9 | (match start +
        // M) << 19 (the literal tail: n << 19)
        const int M = (int)((r >> 9) & 255u), D = (int)(r & 511u);
        const int end = (int)(r >> 19);
        const int cpos = end - M;
        const uint32_t upv = dpp<0x138, 0xf, 0xf>((uint32_t)end);   // wave_shr:1
        const int pend = k == 0 ? 0 : (lane == 0 ? end_prev : (int)upv);   // literal run start
        end_prev = (int)lane63((uint32_t)end);
        const int L = cpos - pend;
        const int rem = (L - 15) & 255;
        const int le = L >= 15 ? (rem == 255 ? 2 : 1) : 0;         // literal-extension bytes
        const int mx = (M - 4) & 255;
        const bool mextW = M >= 4 && mx >= 15, mextS = M != 0 && mx >= 15;
        const int bytes = valid ? 5 + le + L + (mextW ? 1 : 0) : 0;
        const uint32_t inc = wave_incl_add((uint32_t)bytes);
        const int o = wcur + 3 * bi + (int)inc - bytes;               // the sequence's token
        const int ib = o - 3;                                         // (k == 0) its block's header
        const int ol = o + 3 + le;                                   // first literal byte
        if (valid) {
          const int tl = L >= 15 ? 15 : L;                            // LZ4.c:540
          const int tm = M == 0 ? 0 : (M >= 19 ? 15 : mx);            // LZ4.c:542
          const uint32_t ext = le == 0 ? 0u : (rem == 255 ? 255u : (uint32_t)rem);
          const uint32_t SZ = (uint32_t)(5 + le + L + (mextS ? 1 : 0));   // LZ4.c:546-575
          or_bytes(out32, o, (uint32_t)((tl << 4) | tm) | (SZ << 8) | (ext << 24));
          or_bytes(out32, ol + L, (uint32_t)D | (mextW ? ((uint32_t)(mx - 15) & 255u) << 16 : 0u));
          if (k == 0) {                                               // LZ4.c:417-419
            const uint32_t bh = recst[hb - h0][0];
            or_bytes(out32, ib, ((bh >> 16) & 255u) | ((((bh & 0xFFFFu) + 3u) & 0xFFFFu) << 8));
          }
        }
        // literals (LZ4.c:388), flattened over the lanes: one aligned 16-byte
        // image word per lane and pass, funnel-shifted out of five aligned
        // staged input dwords and masked to the run (16-B words: half the
        // passes of 8-B ones; two ds_or_b64 per word)
        {
          const int cw = valid && L > 0 ? ((ol + L - 1) >> 4) - (ol >> 4) + 1 : 0;
          const uint32_t cinc = wave_incl_add((uint32_t)cw);
          const int C = (int)lane63(cinc);
          const int stw = (int)dpp<0x138, 0xf, 0xf>(cinc);
          // the run, as its owning lanes use it: image word w = (ol >> 3) - stw + gw,
          // stage byte of that word's first image byte xs = 8 w + (src - ol), and
          // its bytes [ol, ol + L) of the image (two 16-bit fields per dword)
          const int src = kStagePad + kBlk * (hb - h0) + pend;
          const uint32_t rw = ((uint32_t)((ol >> 4) - stw) & 0xFFFFu) | ((uint32_t)(src - ol) << 16);
          const uint32_t rb = (uint32_t)ol | ((uint32_t)(ol + L) << 16);
          uint32_t carry = 0;                    // 1 + the last run owning a word so far
          for (int w0 = 0; w0 < C; w0 += 64) {
            wave_sync();
            marks[wv][lane] = 0u;
            if (cw > 0 && stw >= w0 && stw < w0 + 64) marks[wv][stw - w0] = (uint32_t)lane + 1u;
            wave_sync();
            const uint32_t k1 = max(wave_incl_max(marks[wv][lane]), carry);
            carry = lane63(k1);
            const int gw = w0 + lane;
            const int kr = ((int)k1 - 1) & 63;   // the run owning word gw
            const uint32_t kw = (uint32_t)__shfl((int)rw, kr, 64);
            const uint32_t kb = (uint32_t)__shfl((int)rb, kr, 64);
            if (gw < C) {
              const int t = 16 * ((int)(int16_t)(kw & 0xFFFFu) + gw);  // image word's first byte
              const int xs = t + ((int)kw >> 16);                      // its input bytes
              const uint32_t *iw = reinterpret_cast<const uint32_t *>(stage + (xs & ~3));
              const uint32_t d0 = iw[0], d1 = iw[1], d2 = iw[2], d3 = iw[3], d4 = iw[4];
              const uint32_t sh = (uint32_t)xs & 3u;
              const int lb = max((int)(kb & 0xFFFFu) - t, 0), hb = min((int)(kb >> 16) - t, 16);
              const uint4 ml = pmask[lb], mh = pmask[hb];
              const uint32_t v0 = __builtin_amdgcn_alignbyte(d1, d0, sh) & (ml.x ^ mh.x);
              const uint32_t v1 = __builtin_amdgcn_alignbyte(d2, d1, sh) & (ml.y ^ mh.y);
              const uint32_t v2 = __builtin_amdgcn_alignbyte(d3, d2, sh) & (ml.z ^ mh.z);
              const uint32_t v3 = __builtin_amdgcn_alignbyte(d4, d3, sh) & (ml.w ^ mh.w);
              atomicOr(reinterpret_cast<unsigned long long *>(img + t),
                       (unsigned long long)v1 << 32 | v0);
              atomicOr(reinterpret_cast<unsigned long long *>(img + t + 8),
                       (unsigned long long)v3 << 32 | v2);
            }
          }
        }
        wcur += (int)lane63(inc);
      }
    }
  }
}

// The task's image -> the stream (aligned 16-B stores; the two edge chunks a
// byte per lane of the last wave); nothing at or past G1 (<= cap) is written.
__device__ __forceinline__ void emit_store(const int tid, const int wv, const int lane,
                                           const uint64_t G0, const uint64_t G1, const int lead,
                                           const uint8_t *img, uint8_t *__restrict__ out) {
  if (G1 <= G0) return;
  // chunk ci covers stream bytes [F + 16 ci, F + 16 ci + 16), F = G0 - lead
  // (16-B aligned), as 32-bit offsets (the range is at most kEmitImg bytes) from
  // out + F, so the stores stay global_store (a pointer rebuilt from an integer
  // is a flat address: every flat store also counts in lgkmcnt and serialised
  // this loop behind its LDS reads)
  const uint64_t F = G0 - (uint64_t)lead;
  uint8_t *const outF = out + F;
  const uint32_t nrel = (uint32_t)(G1 - F);
  const uint32_t c0 = lead ? 1u : 0u, c1 = nrel >> 4;   // the whole chunks: [c0, c1)
  for (uint32_t ci = c0 + (uint32_t)tid; ci < c1; ci += 64 * kEW)
    __builtin_nontemporal_store(reinterpret_cast<const u32x4 *>(img)[ci],
                                reinterpret_cast<u32x4 *>(outF + 16u * ci));
  // the partial chunks at either end, a byte per lane: lanes 0-15 the first
  // chunk's bytes [lead, 16), lanes 16-31 the last one's [16 c1, nrel) (when it
  // is not the first)
  if (wv == kEW - 1 && lane < 32) {
    const uint32_t x = lane < 16 ? (uint32_t)lane : 16u * c1 + (uint32_t)(lane - 16);
    const bool own = lane < 16 ? (c0 && x >= (uint32_t)lead && x < nrel) : (c1 >= c0 && x < nrel);
    if (own) outF[x] = img[x];
  }
}

__global__ __launch_bounds__(64 * kEW) void lz4_emit(
    const uint8_t *__restrict__ in, const uint8_t *__restrict__ heads,
    const uint8_t *__restrict__ ovfs, size_t slot_base,
    const uint32_t *__restrict__ tsz, size_t ntiles, size_t g_first,
    const uint32_t *__restrict__ gsum, const uint64_t *__restrict__ part,
    uint8_t *__restrict__ out, uint64_t cap, int hdr, uint64_t nb_total, uint32_t last_n,
    uint64_t *__restrict__ boff) {
  __shared__ uint64_t toff[kGT + 1];
  __shared__ alignas(16) uint8_t img[kEmitImg];
  __shared__ alignas(16) uint8_t stage[kStage];
  __shared__ uint32_t marks[kEW][64];                // per wave: literal-run starts
  __shared__ uint4 pmask[17];                        // pmask[k]: the low k bytes of 16 set
  __shared__ uint32_t recst[kGH][kRecPre];           // each block's header + first records
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // XCD-aware order (workgroups b and b + 8 share an XCD): XCD b % 8 takes a
  // contiguous eighth of the workgroups, so neighbouring outputs' boundary
  // lines meet in one L2
  const uint32_t nwg = (uint32_t)((ntiles - g_first * kGT + kGT - 1) / kGT) * kGSplit;
  const uint32_t per = (nwg + 7) / 8;
  const uint32_t wg = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  if (wg >= nwg) return;
  const size_t g = g_first + wg / kGSplit;
  const int h0 = (int)(wg % kGSplit) * kGH;          // this workgroup: blocks [h0, h0 + kGH)
  const size_t g0 = g * kGT;
  const int nt = (int)min((size_t)kGT, ntiles - g0);
  if (h0 >= nt) return;
  const int h1 = min(nt, h0 + kGH);
  // Every global load of the workgroup is issued before any of them is
  // waited on (the scan inputs, the record heads, the staged input): one
  // memory round trip per workgroup, not three.
  const size_t b0 = g0 + h0;
  const int len = (h1 - h0 - 1) * kBlk + (g0 + h1 == nb_total ? (int)last_n : kBlk);
  const uint8_t *src = in + b0 * kBlk;
  const bool al16 = ((uintptr_t)src & 15) == 0;    // b0 is a multiple of 32: 9600 B steps
  const int n16 = al16 ? len >> 4 : 0;
  uint64_t pt = 0;
  uint32_t gs = 0, tv = 0;
  if (tid < 64) {
    // wave 0 carries the workgroup's critical path to the first barrier (its
    // scan loads, then two wave sums): raised priority until the barrier
    // (emit 0.622 -> 0.603 ms, tools/ab_inproc.py)
    __builtin_amdgcn_s_setprio(3);
    const size_t p = g0 / kPart;
    const size_t gfirst = p * 64;                  // first group of the partial
    gs = (gfirst + tid < g) ? gsum[gfirst + tid] : 0u;
    pt = part[p];                                  // part[] holds absolute offsets
    tv = tid < nt ? tsz[g0 + tid] : 0u;
  }
  constexpr int kPerSlot = kRecPre / 4;            // record heads: 32 x 96 B, contiguous
  static_assert(kGH * kPerSlot <= 64 * kEW, "one record load per thread");
  uint4 rv = make_uint4(0, 0, 0, 0);
  const int rhb = tid / kPerSlot, rj = tid % kPerSlot;
  // the workgroup's heads (one contiguous run) and overflow slots
  const uint8_t *const wheads = heads + (b0 - slot_base) * (size_t)kHead;
  const uint8_t *const wovf = ovfs + (b0 - slot_base) * (size_t)kOvf;
  if (tid < (h1 - h0) * kPerSlot) {
    const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wheads) + tid);
    rv = make_uint4(t.x, t.y, t.z, t.w);
  }
  constexpr int kSt16 = (kGH * kBlk) / 16;         // 600 16-B chunks of staged input
  constexpr int kStPer = (kSt16 + 64 * kEW - 1) / (64 * kEW);
  uint4 sv[kStPer];
#pragma unroll
  for (int k = 0; k < kStPer; ++k) {
    const int i = tid + k * 64 * kEW;
    u32x4 t = {0u, 0u, 0u, 0u};
    if (i < n16) t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src) + i);
    sv[k] = make_uint4(t.x, t.y, t.z, t.w);
  }
  // the image is zeroed in full while the loads are in flight
  for (int i = tid; i < kEmitImg / 16; i += 64 * kEW)
    reinterpret_cast<uint4 *>(img)[i] = make_uint4(0, 0, 0, 0);
  if (tid < 64) {
    // the groups before g in its partial: <= 63 sums of <= 64 blocks of
    // <= 548 B, so the total fits 32 bits -- a DPP sum, not a 64-bit
    // shuffle reduction (12 dependent ds_bpermute round trips on wave 0,
    // which every wave of the workgroup waits for at the barrier)
    const uint64_t base = pt + lane63(wave_incl_add(gs));
    const uint32_t inc = wave_incl_add(tv);
    toff[tid] = base + inc - tv;
    if (tid == 63) toff[kGT] = base + inc;
    // device-resident block offsets (relative to the first block byte) for
    // the block-parallel decoder: no host prefix sum, no host round trip
    if (h0 == 0 && tid < nt) boff[g0 + tid] = base + inc - tv - (uint64_t)hdr;
  }
  if (hdr && g == 0 && h0 == 0 && tid == 0 && cap > 0) out[0] = (uint8_t)nb_total;
  if (tid < (h1 - h0) * kPerSlot) reinterpret_cast<uint4 *>(&recst[rhb][0])[rj] = rv;
  if (tid < 17) {
    uint32_t m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = min(max(tid - 4 * j, 0), 4);
      m[j] = n == 4 ? ~0u : (1u << (8 * n)) - 1u;
    }
    pmask[tid] = make_uint4(m[0], m[1], m[2], m[3]);
  }
  // ---- stage: byte p of block h is stage[kStagePad + 300 (h - h0) + p] ----------
  {
    uint8_t *dst = stage + kStagePad;
#pragma unroll
    for (int k = 0; k < kStPer; ++k) {
      const int i = tid + k * 64 * kEW;
      if (i < n16) reinterpret_cast<uint4 *>(dst)[i] = sv[k];
    }
    for (int i = (n16 << 4) + tid; i < len; i += 64 * kEW) dst[i] = src[i];   // tail / unaligned
  }
  __syncthreads();
  __builtin_amdgcn_s_setprio(0);
  const uint64_t G0 = toff[h0];
  const int lead = (int)(((uintptr_t)out + G0) & 15);   // img[lead] = stream byte G0
  emit_records(wv, lane, h0, h1, G0, lead, toff, img, stage, recst, marks, pmask, wovf);
  __syncthreads();
  // ---- LDS image -> stream (aligned 16-B stores) --------------------------------
  emit_store(tid, wv, lane, G0, min(toff[h1], cap), lead, img, out);
}

}  // namespace
