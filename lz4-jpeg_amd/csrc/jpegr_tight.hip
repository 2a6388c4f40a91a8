// jpegr_tight.hip -- the JPT1 stream's writer (format: include/jpegr.h): JPR1's
// header, index and record order, each stream's table in the tightest of three
// codings:
//   mode 0  ncodes x { i16 value, u8 length }             (JPR1's entries)
//   mode 1  ceil(ncodes / 2) bytes of nibble lengths, ncodes x i8 value
//   mode 2  ceil(ncodes / 2) bytes of nibble lengths, ncodes x i16 value
// The writer's mode is canonical: 1 when ncodes > 0, every length <= 15 and
// every value fits an i8; else 2 when ncodes > 0 and every length <= 15; else 0.
//
//   jpt_pack_sizes  a workgroup per 16 tiles, a wave per 4: entry k of a
//                   stream on lane k (the emit pass's lanes), each stream's
//                   mode from two ballots, the record size -> u32 (scan input)
//                   and the u16 index; the 16-B header
//   the index scan  (jpegr_pack_common.h, lz4r_scan.h as it is)
//   jpt_pack_emit   jpr_pack_emit's LDS image of the workgroup's output range,
//                   the modes found again from the registers it already holds
// Both kernels are copies of jpegr_pack.hip's, not shared with it: the JPR1
// kernels keep their code and their time.  The scratch is
// jpegr_pack_scratch_bytes: the modes are not stored, the emit pass ballots
// them from the table words it loads anyway.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_pack_common.h"

namespace {

// jpegr_pack.hip's run: 16 tiles per workgroup (16.6 KB of LDS image, 8
// workgroups per CU), 4 waves of 4 tiles
constexpr int kRun = 16;
constexpr int kSplit = kGT / kRun;
constexpr int kPW = 4;
constexpr int kTW = kRun / kPW;
constexpr int kImg = kRun * kRecMax + 16;
static_assert(kGT % kRun == 0 && kRun % kPW == 0 && kImg % 16 == 0, "whole workgroups per scan group");

__device__ __forceinline__ uint32_t slot_off(int c) { return c == 0 ? 0u : c == 1 ? 128u : 192u; }
__device__ __forceinline__ uint32_t meta_codes(uint32_t m, int c) { return min(m >> 24, slot_codes(c)); }
__device__ __forceinline__ uint32_t meta_bits(uint32_t m, int c) { return min(m & 0xFFFFu, slot_bits(c)); }

// table bytes of n entries in mode md
__device__ __forceinline__ uint32_t table_bytes(uint32_t n, uint32_t md) {
  return md == 0 ? 3u * n : ((n + 1u) >> 1) + md * n;
}
__device__ __forceinline__ uint32_t stream_bytes(uint32_t m, int c, uint32_t md) {
  return 4u + table_bytes(meta_codes(m, c), md) + ((meta_bits(m, c) + 7u) >> 3);
}

// a table word's disqualifiers: a length past a nibble, a value past an i8
// (a lane with no live entry holds 0, which disqualifies nothing)
__device__ __forceinline__ bool long_len(uint32_t e) { return ((e >> 16) & 255u) > 15u; }
__device__ __forceinline__ bool wide_val(uint32_t e) { return (int16_t)e != (int8_t)e; }

// the canonical modes of a tile's three streams from the wave's table words
// (tb[0], tb[1]: Y entries lane, 64 + lane; tb[2]: Cr; tb[3]: Cb), as
// Y | Cr << 2 | Cb << 4.  Wave-uniform.
__device__ __forceinline__ uint32_t tile_modes(const uint32_t (&tb)[4], uint32_t n0, uint32_t n1,
                                               uint32_t n2) {
  const bool l0 = __ballot(long_len(tb[0]) || long_len(tb[1])) != 0;
  const bool w0 = __ballot(wide_val(tb[0]) || wide_val(tb[1])) != 0;
  const bool l1 = __ballot(long_len(tb[2])) != 0, w1 = __ballot(wide_val(tb[2])) != 0;
  const bool l2 = __ballot(long_len(tb[3])) != 0, w2 = __ballot(wide_val(tb[3])) != 0;
  const uint32_t m0 = (n0 == 0 || l0) ? 0u : w0 ? 2u : 1u;
  const uint32_t m1 = (n1 == 0 || l1) ? 0u : w1 ? 2u : 1u;
  const uint32_t m2 = (n2 == 0 || l2) ? 0u : w2 ? 2u : 1u;
  return m0 | m1 << 2 | m2 << 4;
}

// the live table words of tile t on this lane (0 where not live)
__device__ __forceinline__ void load_table(const uint32_t *__restrict__ tw, int lane, uint32_t n0,
                                           uint32_t n1, uint32_t n2, uint32_t (&tb)[4]) {
  if ((uint32_t)lane < n0) tb[0] = tw[lane];
  if ((uint32_t)lane + 64u < n0) tb[1] = tw[64 + lane];
  if ((uint32_t)lane < n1) tb[2] = tw[128 + lane];
  if ((uint32_t)lane < n2) tb[3] = tw[192 + lane];
}

__global__ __launch_bounds__(64 * kPW) void jpt_pack_sizes(
    const uint32_t *__restrict__ meta, const uint32_t *__restrict__ table, size_t ntiles,
    size_t wg_base, uint32_t *__restrict__ tsz, uint8_t *__restrict__ out, uint64_t cap, uint32_t w,
    uint32_t h, uint32_t nimg) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t t0 = (wg_base + blockIdx.x) * kRun;
  if (t0 >= ntiles) return;
  const int ntl = (int)min((size_t)kRun, ntiles - t0);
  uint32_t tb[kTW][4], m[kTW][3];
#pragma unroll
  for (int i = 0; i < kTW; ++i) {                       // all 16 table loads before the first ballot
    const int j = kTW * wv + i;
#pragma unroll
    for (int q = 0; q < 4; ++q) tb[i][q] = 0u;
    m[i][0] = m[i][1] = m[i][2] = 0u;
    if (j < ntl) {
#pragma unroll
      for (int c = 0; c < 3; ++c) m[i][c] = meta[3 * (t0 + j) + c];
      load_table(table + (t0 + j) * 256, lane, meta_codes(m[i][0], 0), meta_codes(m[i][1], 1),
                 meta_codes(m[i][2], 2), tb[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    const int j = kTW * wv + i;
    if (j >= ntl) continue;
    const uint32_t md = tile_modes(tb[i], meta_codes(m[i][0], 0), meta_codes(m[i][1], 1),
                                   meta_codes(m[i][2], 2));
    if (lane == 0) {
      const size_t t = t0 + j;
      const uint32_t sz = stream_bytes(m[i][0], 0, md & 3u) + stream_bytes(m[i][1], 1, (md >> 2) & 3u) +
                          stream_bytes(m[i][2], 2, md >> 4);
      tsz[t] = sz;
      const uint64_t pos = kHdr + 2 * (uint64_t)t;      // 2-B aligned: out is 16-B aligned
      if (pos + 2 <= cap)
        *reinterpret_cast<uint16_t *>(out + pos) = (uint16_t)sz;
      else if (pos < cap)
        out[pos] = (uint8_t)sz;
    }
  }
  if (t0 == 0 && tid == 0) {
    const uint32_t hw[4] = {0x3154504Au /* "JPT1" */, w, h, nimg};
    for (uint32_t i = 0; i < (uint32_t)kHdr && i < cap; ++i) out[i] = (uint8_t)(hw[i >> 2] >> (8 * (i & 3)));
  }
}

// jpr_pack_emit (its comments hold here) with the table written by mode.
// Entry k of a stream is on lane k of one register, so the pair (2 j, 2 j + 1)
// of a length byte never straddles two registers: lane 2 j takes lane
// 2 j + 1's word by one cross-lane move and writes the byte; with an odd
// ncodes the last pair's upper lane is not live and holds 0.  Every byte of
// the range is still written once, by byte stores, with no zeroing.
__global__ __launch_bounds__(64 * kPW) void jpt_pack_emit(
    const uint8_t *__restrict__ bits, const uint32_t *__restrict__ meta,
    const uint32_t *__restrict__ table, size_t ntiles, size_t wg_base,
    const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, uint8_t *__restrict__ out, uint64_t cap) {
  __shared__ uint64_t toff[kGT + 1];
  __shared__ alignas(16) uint8_t img[kImg];
  __shared__ uint32_t smeta[kRun * 3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t wg = wg_base + blockIdx.x;
  const size_t g = wg / kSplit;
  const int h0 = (int)(wg % kSplit) * kRun;
  const size_t t0 = g * kGT + h0;                       // the workgroup's first tile
  if (t0 >= ntiles) return;
  const int ntl = (int)min((size_t)kRun, ntiles - t0);
  group_offsets(tid, g, ntiles, tsz, gsum, part, toff);
  if (tid < 3 * ntl) smeta[tid] = meta[3 * t0 + tid];
  __syncthreads();
  const uint64_t G0 = toff[h0], G1 = toff[h0 + ntl];
  const uint32_t lead = (uint32_t)(((uintptr_t)out + G0) & 15);   // img[lead] = stream byte G0

  uint32_t tb[kTW][4], bt[kTW];
  const int bc = lane < 32 ? 0 : lane < 48 ? 1 : 2;     // the channel of this lane's bits dword
  const uint32_t blocal = 4u * (uint32_t)lane - slot_off(bc);
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    const int j = kTW * wv + i;
#pragma unroll
    for (int q = 0; q < 4; ++q) tb[i][q] = 0u;
    bt[i] = 0u;
    if (j < ntl) {
      const uint32_t m0 = smeta[3 * j], m1 = smeta[3 * j + 1], m2 = smeta[3 * j + 2];
      load_table(table + (t0 + j) * 256, lane, meta_codes(m0, 0), meta_codes(m1, 1),
                 meta_codes(m2, 2), tb[i]);
      const uint32_t mb = bc == 0 ? m0 : bc == 1 ? m1 : m2;
      if (blocal < ((meta_bits(mb, bc) + 7u) >> 3))
        bt[i] = reinterpret_cast<const uint32_t *>(bits + (t0 + j) * 256)[lane];
    }
  }
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    const int j = kTW * wv + i;
    if (j >= ntl) continue;
    const uint32_t m[3] = {smeta[3 * j], smeta[3 * j + 1], smeta[3 * j + 2]};
    const uint32_t mds = tile_modes(tb[i], meta_codes(m[0], 0), meta_codes(m[1], 1), meta_codes(m[2], 2));
    const uint32_t md[3] = {mds & 3u, (mds >> 2) & 3u, mds >> 4};
    uint32_t o[3];                                      // each stream's first image byte
    o[0] = lead + (uint32_t)(toff[h0 + j] - G0);
    o[1] = o[0] + stream_bytes(m[0], 0, md[0]);
    o[2] = o[1] + stream_bytes(m[1], 1, md[1]);
    if (lane < 12) {                                    // u8 rle_len | u8 ncodes | u16 nbits | mode << 14
      const int c = lane >> 2;
      const uint32_t mc = c == 0 ? m[0] : c == 1 ? m[1] : m[2];
      const uint32_t oc = c == 0 ? o[0] : c == 1 ? o[1] : o[2];
      const uint32_t dc = c == 0 ? md[0] : c == 1 ? md[1] : md[2];
      const uint32_t hw = ((mc >> 16) & 255u) | meta_codes(mc, c) << 8 |
                          (meta_bits(mc, c) | dc << 14) << 16;
      img[oc + (lane & 3)] = (uint8_t)(hw >> (8 * (lane & 3)));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = q < 2 ? 0 : q - 1;
      const uint32_t k = (uint32_t)lane + (q == 1 ? 64u : 0u);
      const uint32_t e = tb[i][q];
      const uint32_t up = __shfl_down(e, 1);            // lane + 1's word, by every lane of the wave
      const uint32_t nc = meta_codes(m[c], c);
      if (k < nc) {
        uint8_t *p = img + o[c] + 4u;
        if (md[c] == 0) {                               // i16 value, u8 code length
          p += 3u * k;
          p[0] = (uint8_t)e;
          p[1] = (uint8_t)(e >> 8);
          p[2] = (uint8_t)(e >> 16);
        } else {
          if ((k & 1u) == 0) p[k >> 1] = (uint8_t)(((e >> 16) & 15u) | ((up >> 16) & 15u) << 4);
          p += (nc + 1u) >> 1;
          if (md[c] == 1) {
            p[k] = (uint8_t)e;
          } else {
            p[2u * k] = (uint8_t)e;
            p[2u * k + 1] = (uint8_t)(e >> 8);
          }
        }
      }
    }
    const uint32_t mb = bc == 0 ? m[0] : bc == 1 ? m[1] : m[2];
    const uint32_t ob = bc == 0 ? o[0] : bc == 1 ? o[1] : o[2];
    const uint32_t db = bc == 0 ? md[0] : bc == 1 ? md[1] : md[2];
    const uint32_t nby = (meta_bits(mb, bc) + 7u) >> 3;
    uint8_t *p = img + ob + 4u + table_bytes(meta_codes(mb, bc), db) + blocal;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
      if (blocal + b < nby) p[b] = (uint8_t)(bt[i] >> (8 * b));
  }
  __syncthreads();
  // ---- LDS image -> stream: aligned 16-B stores; the first and last partial
  // chunks, which neighbouring workgroups share, a byte per lane; nothing at
  // or past cap
  const uint64_t E = min(G1, cap);
  if (E <= G0) return;
  uint8_t *const outF = out + (G0 - lead);              // 16-B aligned
  const uint32_t nrel = (uint32_t)(E - G0) + lead;
  const uint32_t c0 = lead ? 1u : 0u, c1 = nrel >> 4;   // the whole chunks: [c0, c1)
  for (uint32_t ci = c0 + (uint32_t)tid; ci < c1; ci += 64 * kPW)
    __builtin_nontemporal_store(reinterpret_cast<const u32x4 *>(img)[ci],
                                reinterpret_cast<u32x4 *>(outF + 16u * ci));
  if (wv == kPW - 1 && lane < 32) {
    const uint32_t x = lane < 16 ? (uint32_t)lane : 16u * c1 + (uint32_t)(lane - 16);
    const bool own = lane < 16 ? (c0 && x >= lead && x < nrel) : (c1 >= c0 && x < nrel);
    if (own) outF[x] = img[x];
  }
}

}  // namespace

extern "C" int jpegr_stream_format(const uint8_t header[16], int *w, int *h, int *nimg, int *format) {
  if (!header || !w || !h || !nimg || !format) return JPEGR_ERR_ARG;
  if (header[0] != 'J' || header[1] != 'P' || (header[2] != 'R' && header[2] != 'T') ||
      header[3] != '1')
    return JPEGR_ERR_ARG;
  uint32_t v[3];
  for (int i = 0; i < 3; ++i)
    v[i] = (uint32_t)header[4 + 4 * i] | (uint32_t)header[5 + 4 * i] << 8 |
           (uint32_t)header[6 + 4 * i] << 16 | (uint32_t)header[7 + 4 * i] << 24;
  if (v[0] == 0 || v[1] == 0 || v[2] == 0 || v[0] > 0x7FFFFFFFu || v[1] > 0x7FFFFFFFu ||
      v[2] > 0x7FFFFFFFu)
    return JPEGR_ERR_ARG;
  *w = (int)v[0];
  *h = (int)v[1];
  *nimg = (int)v[2];
  *format = header[2] == 'R' ? JPEGR_STREAM_JPR1 : JPEGR_STREAM_JPT1;
  return JPEGR_OK;
}

extern "C" int jpegr_pack_tight_device(const void *d_bits, const void *d_meta, const void *d_table,
                                       int w, int h, int nimg, void *d_out, size_t cap,
                                       void *d_out_len, void *d_scratch, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_bits || !d_meta || !d_table || !d_out || !d_out_len || !d_scratch || ntiles == 0 ||
      (reinterpret_cast<uintptr_t>(d_bits) & 3) != 0 || (reinterpret_cast<uintptr_t>(d_meta) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(d_table) & 3) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_out_len) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(d_scratch) & 15) != 0)
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch s = scratch_of(d_scratch, ntiles);
  auto *meta = static_cast<const uint32_t *>(d_meta);
  auto *tab = static_cast<const uint32_t *>(d_table);
  auto *out = static_cast<uint8_t *>(d_out);
  const size_t nwg = (ntiles + kRun - 1) / kRun;
  for (size_t b = 0; b < nwg; b += kMaxWg)
    hipLaunchKernelGGL(jpt_pack_sizes, dim3((unsigned)std::min(kMaxWg, nwg - b)), dim3(64 * kPW), 0, st,
                       meta, tab, ntiles, b, s.tsz, out, (uint64_t)cap, (uint32_t)w, (uint32_t)h,
                       (uint32_t)nimg);
  scan(s, ntiles, static_cast<uint64_t *>(d_out_len), st);
  for (size_t b = 0; b < nwg; b += kMaxWg)
    hipLaunchKernelGGL(jpt_pack_emit, dim3((unsigned)std::min(kMaxWg, nwg - b)), dim3(64 * kPW), 0, st,
                       static_cast<const uint8_t *>(d_bits), meta, tab, ntiles, b, s.tsz, s.gsum, s.part,
                       out, (uint64_t)cap);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
