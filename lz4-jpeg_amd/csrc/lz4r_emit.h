// lz4r_emit.h -- the compressor's emission pass: sequence records
// (lz4r_layout.h) -> stream bytes at the offsets the scan placed them.
// lz4_emit: workgroup = 32 consecutive blocks (half a scan group of 64).
//   offsets  the blocks' stream offsets from the partials, the group sums and
//            a wave scan; also stored to boff (the decoder's side input)
//   stage    the 32 blocks' input -> LDS (the literals' source; 16-B loads)
//   bytes    the 32 blocks' sequence records, block after block, take the
//            flattened indices 0 .. T-1 (T = 496 on text) and are dealt in
//            rounds of 64 to the 8 waves, round r to wave r % 8: no wave runs
//            a second, nearly empty round for its own blocks' stragglers.
//            Every wave scans the 32 counts for itself; a round finds each
//            lane's block by a max-scan over the block starts inside it, the
//            literal-run start of its first record in the record before it
//            (LDS head or overflow slot), and its first token's place with no
//            word from another wave: at a block's offset + 3 when one starts
//            there, else at the next block's offset less the round's bytes to
//            that block's end (a block that holds a whole round sums its own
//            earlier records: > 64 records, none in text).  Per sequence the
//            token / size / literal-extension / offset / match-extension bytes
//            (write_sequence, LZ4.c:365-413) and per block the u8 count + u16
//            size header (write_block, :415-425) land by aligned ds_or in a
//            zeroed LDS image of the output range, and each round's literal
//            runs are flattened over the lanes as aligned 16-byte image words
//            funnel-shifted out of the staged input
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
constexpr int kEW = 8;                               // waves per emit workgroup
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

// One record (lz4r_layout.h) of workgroup block b (0 .. kGH-1), k its index in
// the block: the head staged in LDS, or the block's overflow slot
__device__ __forceinline__ uint32_t load_record(const uint32_t (*recst)[kRecPre],
                                                const uint8_t *__restrict__ wovf, int b, int k) {
  const uint32_t *rp = reinterpret_cast<const uint32_t *>(wovf + b * kOvf);
  return 1 + k < kRecPre ? recst[b][1 + k] : rp[1 + k - kRecPre];
}

// The stream bytes of the sequence with record r whose literal run starts at
// block byte pend: token, u16 size, literal extension, literals, u16 offset,
// match extension (write_sequence, LZ4.c:365-413)
__device__ __forceinline__ int sequence_bytes(uint32_t r, int pend) {
  const int M = (int)((r >> 9) & 255u);
  const int L = (int)(r >> 19) - M - pend;
  const int le = L >= 15 ? ((((L - 15) & 255) == 255) ? 2 : 1) : 0;
  const int mx = (M - 4) & 255;
  return 5 + le + L + (M >= 4 && mx >= 15 ? 1 : 0);
}

// Records -> bytes of one emit task (lz4_emit), blocks [h0, h1) of a group:
// the task's records, block after block, take the flattened indices 0 .. T-1
// and wave wv takes the rounds wv, wv + 8, ... of 64 records each; the image
// img[lead] is stream byte G0; block h's input is
// stage[kStagePad + 300 (h - h0) + p].
__device__ __forceinline__ void emit_records(const int wv, const int lane, const int h0,
                                             const int h1, const uint64_t G0, const int lead,
                                             const uint64_t *toff, uint8_t *img,
                                             const uint8_t *stage,
                                             const uint32_t (*recst)[kRecPre],
                                             uint32_t (*marks)[64], const uint4 *pmask,
                                             const uint8_t *__restrict__ wovf) {
  uint32_t *const out32 = reinterpret_cast<uint32_t *>(img);
  // lanes 0..h1-h0-1: the blocks' sequence counts (>= 1) -> first flattened
  // index; every wave scans for itself (32 counts: cheaper than a barrier)
  const uint32_t ns = lane < h1 - h0 ? recst[lane][0] >> 16 : 0u;
  const uint32_t sinc = wave_incl_add(ns);
  const int T = (int)lane63(sinc);
  const uint32_t sst = sinc - ns;              // (the lanes past the blocks: T)
  // a block's start as one word that grows with the block: a wave max-scan
  // over the starts of a round hands every lane its block and that block's
  // first index
  const uint32_t desc = ns ? ((uint32_t)(lane + 1) << 16) | sst : 0u;
  // the task's blocks are contiguous in the image, each its 3 header bytes
  // and then its sequences' bytes (bsizes counts the bytes written): sequence f
  // of a round lands at the round's first one + 3 per block start between
  // them + the bytes of the round's sequences before it
  const int rel = lead - (int)(uint32_t)G0;    // image byte = rel + (u32) stream byte
  const int wvu = __builtin_amdgcn_readfirstlane(wv);   // (a VGPR otherwise: f0 uniform)
  const uint32_t *const toff32 = reinterpret_cast<const uint32_t *>(toff);
  for (int f0 = 64 * wvu; f0 < T; f0 += 64 * kEW) {
    const bool valid = f0 + lane < T;
    // block cb holds record f0 (k0 of it): the last start <= f0
    const int cb = __builtin_popcountll(ballot(sst <= (uint32_t)f0)) - 1;
    const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int)desc, cb);
    const int k0 = f0 - (int)(cd & 0xFFFFu);
    const int cn = __builtin_amdgcn_readlane((int)sinc, cb) - f0;   // its records from f0 on
    // the round's uniform reads, under the marks' round trip: the offset
    // of the first block boundary at or after f0, and the record before
    // f0 (where the first literal run starts: the head, or the overflow
    // slot from record 24 on)
    const int nz = k0 != 0 ? 1 : 0;
    const uint32_t tb = toff32[2 * (h0 + cb + nz)];
    // (dword k0 of the block's scratch = record k0 - 1; the slot's read on
    // lane 0 alone, as a uniform one becomes a flat load of either space)
    uint32_t rprev = recst[cb][min(k0, kRecPre - 1)];
    wave_sync();
    marks[wv][lane] = 0u;
    if (sst - (uint32_t)f0 - 1u < 63u) marks[wv][sst - (uint32_t)f0] = desc;   // starts inside
    wave_sync();
    const uint32_t bd = max(wave_incl_max(marks[wv][lane]), cd);
    const int bi = (int)(bd >> 16) - 1;        // the lane's block, of the workgroup's
    const int k = f0 + lane - (int)(bd & 0xFFFFu);   // sequence index in the block
    const int hb = h0 + bi;
    uint32_t r = recst[bi][min(1 + k, kRecPre - 1)];
    if (valid && 1 + k >= kRecPre)
      r = reinterpret_cast<const uint32_t *>(wovf + bi * kOvf)[1 + k - kRecPre];
    r = valid ? r : 0u;
    asm volatile("" : "+v"(rprev));            // (keeps the two reads apart: ds_read, global_load)
    if (lane == 0 && k0 >= kRecPre)
      rprev = reinterpret_cast<const uint32_t *>(wovf + cb * kOvf)[k0 - kRecPre];
    const int end_prev = k0 != 0 ? (int)(rprev >> 19) : 0;
    // record = the sequence's match word: dist | M << 9 | (match start +
    // M) << 19 (the literal tail: n << 19)
    const int M = (int)((r >> 9) & 255u), D = (int)(r & 511u);
    const int end = (int)(r >> 19);
    const int cpos = end - M;
    const uint32_t upv = dpp<0x138, 0xf, 0xf>((uint32_t)end);   // wave_shr:1
    const int pend = k == 0 ? 0 : (lane == 0 ? end_prev : (int)upv);   // literal run start
    const int L = cpos - pend;
    const int rem = (L - 15) & 255;
    const int le = L >= 15 ? (rem == 255 ? 2 : 1) : 0;         // literal-extension bytes
    const int mx = (M - 4) & 255;
    const bool mextW = M >= 4 && mx >= 15, mextS = M != 0 && mx >= 15;
    const int bytes = valid ? 5 + le + L + (mextW ? 1 : 0) : 0;
    const uint32_t inc = wave_incl_add((uint32_t)bytes);
    // the round's first token, with no word from another wave: block cb
    // starts here (its offset + 3), or ends in this round (the next block's
    // offset less the bytes to its end); a block with neither in the round
    // (> 64 records, none in text) sums its records before f0
    const int tail = __builtin_amdgcn_readlane((int)inc, (cn - 1) & 63);
    int first = rel + (int)tb + (nz ? -tail : 3);
    if (nz & (cn > 64 ? 1 : 0)) {
      int pre = 0, pe = 0;
      for (int j0 = 0; j0 < k0; j0 += 64) {
        const int j = j0 + lane;
        const uint32_t q = j < k0 ? load_record(recst, wovf, cb, j) : 0u;
        const uint32_t up = dpp<0x138, 0xf, 0xf>(q >> 19);
        const int qb = j < k0 ? sequence_bytes(q, lane == 0 ? pe : (int)up) : 0;
        pe = (int)lane63(q >> 19);
        pre += (int)lane63(wave_incl_add((uint32_t)qb));
      }
      first = rel + (int)toff32[2 * (h0 + cb)] + 3 + pre;
    }
    const int o = first + 3 * (bi - cb) + (int)inc - bytes;       // the sequence's token
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

// Everything per block or per group is the launch chunk's own (in, bsizes, gsum,
// part, boff point at the chunk's first block, group and partial; ntiles
// blocks, the last of last_n bytes), and what is the same for every
// workgroup comes from the host: nwg workgroups with blocks, per of them per
// XCD.  A chunk has at most 2^24 blocks (lz4r.hip kChunk), so block indices
// and the heads' byte offsets are 32-bit; the input's and the overflow
// slots' offsets are not.
__global__ __launch_bounds__(64 * kEW) void lz4_emit(
    const uint8_t *__restrict__ in, const uint8_t *__restrict__ heads,
    const uint8_t *__restrict__ ovfs, const uint16_t *__restrict__ bsizes, uint32_t ntiles,
    uint32_t nwg, uint32_t per, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, uint8_t *__restrict__ out, uint64_t cap, uint32_t hdr,
    uint32_t last_n, uint64_t *__restrict__ boff) {
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
  const uint32_t wg = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  if (wg >= nwg) return;
  const uint32_t g = wg / kGSplit;
  const int h0 = (int)(wg % kGSplit) * kGH;          // this workgroup: blocks [h0, h0 + kGH)
  const uint32_t g0 = g * kGT;
  const int nt = (int)min((uint32_t)kGT, ntiles - g0);
  if (h0 >= nt) return;
  const int h1 = min(nt, h0 + kGH);
  // Every global load of the workgroup is issued before any of them is
  // waited on (the scan inputs, the record heads, the staged input): one
  // memory round trip per workgroup, not three.
  const uint32_t b0 = g0 + (uint32_t)h0;
  const int len = (h1 - h0 - 1) * kBlk + (g0 + (uint32_t)h1 == ntiles ? (int)last_n : kBlk);
  const uint8_t *src = in + (size_t)b0 * kBlk;
  const bool al16 = ((uintptr_t)src & 15) == 0;    // b0 is a multiple of 32: 9600 B steps
  const int n16 = al16 ? len >> 4 : 0;
  uint64_t pt = 0;
  uint32_t gs = 0, tv = 0;
  if (tid < 64) {
    // wave 0 carries the workgroup's critical path to the first barrier (its
    // scan loads, then two wave sums): raised priority until the barrier
    // (emit 0.622 -> 0.603 ms, tools/ab_inproc.py)
    __builtin_amdgcn_s_setprio(3);
    const uint32_t p = g0 / kPart;
    const uint32_t gfirst = p * 64;                // first group of the partial
    gs = (gfirst + (uint32_t)tid < g) ? gsum[gfirst + (uint32_t)tid] : 0u;
    pt = part[p];                                  // part[] holds absolute offsets
    tv = tid < nt ? (uint32_t)bsizes[g0 + (uint32_t)tid] : 0u;
  }
  constexpr int kPerSlot = kRecPre / 4;            // record heads: 32 x 96 B, contiguous
  static_assert(kGH * kPerSlot <= 64 * kEW, "one record load per thread");
  uint4 rv = make_uint4(0, 0, 0, 0);
  const int rhb = tid / kPerSlot, rj = tid % kPerSlot;
  // the workgroup's heads (one contiguous run) and overflow slots
  const uint8_t *const wheads = heads + b0 * (uint32_t)kHead;
  const uint8_t *const wovf = ovfs + (size_t)b0 * kOvf;
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
    if (h0 == 0 && tid < nt) boff[g0 + (uint32_t)tid] = base + inc - tv - (uint64_t)hdr;
  }
  // (the frame byte out[0] is the scan's: lz4_scan_partials_frame)
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
