// jpegr_pack.hip -- the JPR stream: the entropy stage's fixed slots (256 B of
// bits, 3 meta words, 256 table words per tile) packed into one byte stream
// of variable-length tile records behind a u16 size index, and the inverse
// (format: include/jpegr.h).
//
//   pack    jpr_pack_sizes   a lane per tile: record size -> u32 (scan input)
//                            and the stream's u16 index; the 16-B header
//           lz4_scan_reduce / lz4_scan_partials (lz4r_scan.h, as they are):
//                            groups of 64 tiles, partials of 4,096; the end
//                            of the scan is the stream length
//           jpr_pack_emit    a workgroup per 16 tiles: records into an LDS
//                            image of its output range, out as 16-B stores
//   unpack  jpr_unpack_sizes index -> u32 sizes, header verdict
//           the same scan    -> the length the header and index imply
//           jpr_unpack_tiles a workgroup per 16 tiles: its input range
//                            through LDS, records checked and scattered
// No host-side state, no host read-back: every call can be captured in a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_pack_common.h"

namespace {

// tiles per workgroup (a quarter of a scan group).  The LDS image is sized for
// the worst case, 1,036 B a tile, so the run sets the occupancy: 16 tiles
// (16.6 KB, 8 workgroups per CU) pack a 4K image in 0.035 ms, 32 tiles in
// 0.051 ms, 8 tiles in 0.043 ms
constexpr int kRun = 16;
constexpr int kSplit = kGT / kRun;          // workgroups per scan group
constexpr int kPW = 4;                      // waves per workgroup
constexpr int kTW = kRun / kPW;             // tiles per wave
constexpr int kImg = kRun * kRecMax + 16;   // the range + its lead inside a 16-B chunk
static_assert(kGT % kRun == 0 && kRun % kPW == 0 && kImg % 16 == 0, "whole workgroups per scan group");

// a channel's first byte of the bits slot, first entry of the table slot
__device__ __forceinline__ uint32_t slot_off(int c) { return c == 0 ? 0u : c == 1 ? 128u : 192u; }

// what pack copies of a stream: its codes and bit bytes, clamped to the slot
// (a meta word past its slot cannot make any kernel here leave the slot)
__device__ __forceinline__ uint32_t meta_codes(uint32_t m, int c) { return min(m >> 24, slot_codes(c)); }
__device__ __forceinline__ uint32_t meta_bits(uint32_t m, int c) { return min(m & 0xFFFFu, slot_bits(c)); }
__device__ __forceinline__ uint32_t stream_bytes(uint32_t m, int c) {
  return 4u + 3u * meta_codes(m, c) + ((meta_bits(m, c) + 7u) >> 3);
}

__global__ __launch_bounds__(256) void jpr_pack_sizes(const uint32_t *__restrict__ meta,
                                                      size_t ntiles, size_t t_base,
                                                      uint32_t *__restrict__ tsz,
                                                      uint8_t *__restrict__ out, uint64_t cap,
                                                      uint32_t w, uint32_t h, uint32_t nimg) {
  const size_t t = t_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t sz = stream_bytes(meta[3 * t], 0) + stream_bytes(meta[3 * t + 1], 1) +
                      stream_bytes(meta[3 * t + 2], 2);
  tsz[t] = sz;
  const uint64_t pos = kHdr + 2 * (uint64_t)t;          // 2-B aligned: out is 16-B aligned
  if (pos + 2 <= cap)
    *reinterpret_cast<uint16_t *>(out + pos) = (uint16_t)sz;
  else if (pos < cap)
    out[pos] = (uint8_t)sz;
  if (t == 0) {
    const uint32_t hw[4] = {0x3152504Au /* "JPR1" */, w, h, nimg};
    for (uint32_t i = 0; i < (uint32_t)kHdr && i < cap; ++i) out[i] = (uint8_t)(hw[i >> 2] >> (8 * (i & 3)));
  }
}

// A workgroup's 16 tiles -> stream bytes [G0, G1).  Wave v takes tiles
// 4 v .. 4 v + 3; per tile a lane holds five dwords of the slots -- table
// words lane, 64 + lane (Y), 128 + lane (Cr), 192 + lane (Cb) and dword
// `lane` of the 256 bit bytes -- loaded only where live, all 20 issued
// before the first is used.  Every byte of the range is written once (the
// records are dense), so the image needs no zeroing and byte stores to LDS
// need no atomics.
__global__ __launch_bounds__(64 * kPW) void jpr_pack_emit(
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
      const uint32_t *tw = table + (t0 + j) * 256;
      const uint32_t n0 = meta_codes(m0, 0), n1 = meta_codes(m1, 1), n2 = meta_codes(m2, 2);
      if ((uint32_t)lane < n0) tb[i][0] = tw[lane];
      if ((uint32_t)lane + 64u < n0) tb[i][1] = tw[64 + lane];
      if ((uint32_t)lane < n1) tb[i][2] = tw[128 + lane];
      if ((uint32_t)lane < n2) tb[i][3] = tw[192 + lane];
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
    uint32_t o[3];                                      // each stream's first image byte
    o[0] = lead + (uint32_t)(toff[h0 + j] - G0);
    o[1] = o[0] + stream_bytes(m[0], 0);
    o[2] = o[1] + stream_bytes(m[1], 1);
    if (lane < 12) {                                    // u8 rle_len | u8 ncodes | u16 nbits
      const int c = lane >> 2;
      const uint32_t mc = c == 0 ? m[0] : c == 1 ? m[1] : m[2];
      const uint32_t oc = c == 0 ? o[0] : c == 1 ? o[1] : o[2];
      const uint32_t hw = ((mc >> 16) & 255u) | meta_codes(mc, c) << 8 | meta_bits(mc, c) << 16;
      img[oc + (lane & 3)] = (uint8_t)(hw >> (8 * (lane & 3)));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {                       // i16 value, u8 code length
      const int c = q < 2 ? 0 : q - 1;
      const uint32_t k = (uint32_t)lane + (q == 1 ? 64u : 0u);
      if (k < meta_codes(m[c], c)) {
        uint8_t *p = img + o[c] + 4u + 3u * k;
        const uint32_t e = tb[i][q];
        p[0] = (uint8_t)e;
        p[1] = (uint8_t)(e >> 8);
        p[2] = (uint8_t)(e >> 16);
      }
    }
    const uint32_t mb = bc == 0 ? m[0] : bc == 1 ? m[1] : m[2];
    const uint32_t ob = bc == 0 ? o[0] : bc == 1 ? o[1] : o[2];
    const uint32_t nby = (meta_bits(mb, bc) + 7u) >> 3;
    uint8_t *p = img + ob + 4u + 3u * meta_codes(mb, bc) + blocal;
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

// ---- unpack ---------------------------------------------------------------------

__global__ __launch_bounds__(256) void jpr_unpack_sizes(const uint8_t *__restrict__ in,
                                                        uint64_t in_len, size_t ntiles,
                                                        size_t t_base, uint32_t w, uint32_t h,
                                                        uint32_t nimg, uint32_t *__restrict__ tsz,
                                                        uint64_t *__restrict__ result) {
  const size_t t = t_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const uint64_t pos = kHdr + 2 * (uint64_t)t;
  const uint32_t lo = pos < in_len ? in[pos] : 0u, hi = pos + 1 < in_len ? in[pos + 1] : 0u;
  tsz[t] = lo | hi << 8;
  if (t == 0) {
    const uint32_t want[4] = {0x3152504Au, w, h, nimg};
    bool ok = in_len >= kHdr + 2 * (uint64_t)ntiles;
    for (uint32_t i = 0; ok && i < (uint32_t)kHdr; ++i)
      ok = in[i] == (uint8_t)(want[i >> 2] >> (8 * (i & 3)));
    result[1] = ok ? ~0ull : 0ull;
  }
}

// A workgroup's 16 records: its input range staged in LDS (16-B loads; the
// partial chunks at either end bytewise, so no read leaves [0, in_len)), a
// lane per tile checks the three stream headers against the slots and the
// indexed size, then wave v scatters tiles 4 v .. 4 v + 3: table words and
// bit dwords rebuilt from the record's bytes, lanes as in jpr_pack_emit.  An
// index entry over 1,036 B is malformed by itself; the window holds 16
// records of that size, and a (well-formed) record behind such an entry is
// read from the stream directly.
__global__ __launch_bounds__(64 * kPW) void jpr_unpack_tiles(
    const uint8_t *__restrict__ in, uint64_t in_len, size_t ntiles, size_t wg_base,
    const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, uint64_t *__restrict__ result,
    uint8_t *__restrict__ bits, uint32_t *__restrict__ meta, uint32_t *__restrict__ table) {
  __shared__ uint64_t toff[kGT + 1];
  __shared__ alignas(16) uint8_t img[kImg];
  __shared__ uint32_t smeta[kRun * 3];
  __shared__ uint32_t soff[kRun * 3];                   // each stream's offset from G0
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t wg = wg_base + blockIdx.x;
  const size_t g = wg / kSplit;
  const int h0 = (int)(wg % kSplit) * kRun;
  const size_t t0 = g * kGT + h0;
  if (t0 >= ntiles) return;
  const int ntl = (int)min((size_t)kRun, ntiles - t0);
  group_offsets(tid, g, ntiles, tsz, gsum, part, toff);
  const uint64_t implied = result[0], head = result[1];
  if (head == 0 || implied != in_len) {                 // the same in every workgroup
    if (tid < 3 * ntl) meta[3 * t0 + tid] = 0u;
    if (tid == 0) atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 0ull);
    return;
  }
  __syncthreads();
  // implied == in_len: every offset of the scan lies inside the stream
  const uint64_t G0 = toff[h0];
  const uint32_t wlen = (uint32_t)min(toff[h0 + ntl] - G0, (uint64_t)(kRun * kRecMax));
  const uint32_t lead = (uint32_t)(((uintptr_t)in + G0) & 15);
  {
    const uint8_t *const inF = in + (G0 - lead);        // G0 >= 16 > lead
    const uint32_t nrel = wlen + lead;
    const uint32_t c0 = lead ? 1u : 0u, c1 = nrel >> 4;
    for (uint32_t ci = c0 + (uint32_t)tid; ci < c1; ci += 64 * kPW)
      reinterpret_cast<u32x4 *>(img)[ci] =
          __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(inF + 16u * ci));
    if (wv == kPW - 1 && lane < 32) {
      const uint32_t x = lane < 16 ? (uint32_t)lane : 16u * c1 + (uint32_t)(lane - 16);
      const bool own = lane < 16 ? (c0 && x >= lead && x < nrel) : (c1 >= c0 && x < nrel);
      if (own) img[x] = inF[x];
    }
  }
  __syncthreads();
  // stream byte G0 + x
  auto rd = [&](uint32_t x) -> uint32_t {
    if (x < wlen) return img[lead + x];
    return G0 + x < in_len ? in[G0 + x] : 0u;
  };
  if (tid < ntl) {
    const uint32_t off = (uint32_t)(toff[h0 + tid] - G0);       // < 16 x 65,535
    const uint32_t size = (uint32_t)(toff[h0 + tid + 1] - toff[h0 + tid]);
    bool ok = size <= (uint32_t)kRecMax;
    uint32_t p = 0, m[3] = {0u, 0u, 0u};
    for (int c = 0; c < 3 && ok; ++c) {
      if (p + 4 > size) {
        ok = false;
        break;
      }
      const uint32_t rle = rd(off + p), nc = rd(off + p + 1);
      const uint32_t nb = rd(off + p + 2) | rd(off + p + 3) << 8;
      ok = rle <= slot_codes(c) && nc <= slot_codes(c) && nb <= slot_bits(c);
      soff[3 * tid + c] = off + p;
      m[c] = nb | rle << 16 | nc << 24;
      p += 4u + 3u * nc + ((nb + 7u) >> 3);
    }
    ok = ok && p == size;
    if (!ok) {
      m[0] = m[1] = m[2] = 0u;
      atomicMin(reinterpret_cast<unsigned long long *>(result + 1),
                1ull + (unsigned long long)(t0 + tid));
    }
    for (int c = 0; c < 3; ++c) {
      smeta[3 * tid + c] = m[c];
      meta[3 * (t0 + tid) + c] = m[c];
    }
  }
  __syncthreads();
  const int bc = lane < 32 ? 0 : lane < 48 ? 1 : 2;
  const uint32_t blocal = 4u * (uint32_t)lane - slot_off(bc);
  for (int i = 0; i < kTW; ++i) {
    const int j = kTW * wv + i;
    if (j >= ntl) break;
    const uint32_t m[3] = {smeta[3 * j], smeta[3 * j + 1], smeta[3 * j + 2]};
    if ((m[0] | m[1] | m[2]) == 0u) continue;           // malformed: ncodes = 0, slots untouched
    uint32_t *tw = table + (t0 + j) * 256;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = q < 2 ? 0 : q - 1;
      const uint32_t k = (uint32_t)lane + (q == 1 ? 64u : 0u);
      if (k < (m[c] >> 24)) {
        const uint32_t x = soff[3 * j + c] + 4u + 3u * k;
        tw[slot_off(c) + k] = rd(x) | rd(x + 1) << 8 | rd(x + 2) << 16;
      }
    }
    const uint32_t mb = bc == 0 ? m[0] : bc == 1 ? m[1] : m[2];
    const uint32_t nby = ((mb & 0xFFFFu) + 7u) >> 3;
    if (blocal < nby) {                                 // the last dword's spare bytes: 0
      const uint32_t x = soff[3 * j + bc] + 4u + 3u * (mb >> 24) + blocal;
      uint32_t v = 0;
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
        if (blocal + b < nby) v |= rd(x + b) << (8 * b);
      reinterpret_cast<uint32_t *>(bits + (t0 + j) * 256)[lane] = v;
    }
  }
}

}  // namespace

extern "C" size_t jpegr_pack_bound(int w, int h, int nimg) {
  const size_t nt = tiles_of(w, h, nimg);
  return nt ? kHdr + nt * (2 + (size_t)kRecMax) : 0;
}

extern "C" size_t jpegr_pack_scratch_bytes(size_t ntiles) {
  return scratch_of(nullptr, ntiles).bytes;
}

extern "C" int jpegr_stream_info(const uint8_t header[16], int *w, int *h, int *nimg) {
  if (!header || !w || !h || !nimg) return JPEGR_ERR_ARG;
  if (header[0] != 'J' || header[1] != 'P' || header[2] != 'R' || header[3] != '1')
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
  return JPEGR_OK;
}

extern "C" int jpegr_pack_device(const void *d_bits, const void *d_meta, const void *d_table,
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
  auto *out = static_cast<uint8_t *>(d_out);
  for (size_t b = 0; b * 256 < ntiles; b += kMaxWg) {
    const size_t n = std::min(kMaxWg, (ntiles - b * 256 + 255) / 256);
    hipLaunchKernelGGL(jpr_pack_sizes, dim3((unsigned)n), dim3(256), 0, st, meta, ntiles, b * 256,
                       s.tsz, out, (uint64_t)cap, (uint32_t)w, (uint32_t)h, (uint32_t)nimg);
  }
  scan(s, ntiles, static_cast<uint64_t *>(d_out_len), st);
  const size_t nwg = (ntiles + kRun - 1) / kRun;
  for (size_t b = 0; b < nwg; b += kMaxWg)
    hipLaunchKernelGGL(jpr_pack_emit, dim3((unsigned)std::min(kMaxWg, nwg - b)), dim3(64 * kPW), 0, st,
                       static_cast<const uint8_t *>(d_bits), meta,
                       static_cast<const uint32_t *>(d_table), ntiles, b, s.tsz, s.gsum, s.part, out,
                       (uint64_t)cap);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

extern "C" int jpegr_unpack_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                   void *d_bits, void *d_meta, void *d_table, void *d_scratch,
                                   void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_in || !d_bits || !d_meta || !d_table || !d_scratch || !d_result || ntiles == 0 ||
      (reinterpret_cast<uintptr_t>(d_bits) & 3) != 0 || (reinterpret_cast<uintptr_t>(d_meta) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(d_table) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(d_result) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(d_scratch) & 15) != 0)
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch s = scratch_of(d_scratch, ntiles);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *result = static_cast<uint64_t *>(d_result);
  for (size_t b = 0; b * 256 < ntiles; b += kMaxWg) {
    const size_t n = std::min(kMaxWg, (ntiles - b * 256 + 255) / 256);
    hipLaunchKernelGGL(jpr_unpack_sizes, dim3((unsigned)n), dim3(256), 0, st, in, (uint64_t)in_len,
                       ntiles, b * 256, (uint32_t)w, (uint32_t)h, (uint32_t)nimg, s.tsz, result);
  }
  scan(s, ntiles, result, st);
  const size_t nwg = (ntiles + kRun - 1) / kRun;
  for (size_t b = 0; b < nwg; b += kMaxWg)
    hipLaunchKernelGGL(jpr_unpack_tiles, dim3((unsigned)std::min(kMaxWg, nwg - b)), dim3(64 * kPW), 0, st,
                       in, (uint64_t)in_len, ntiles, b, s.tsz, s.gsum, s.part, result,
                       static_cast<uint8_t *>(d_bits), static_cast<uint32_t *>(d_meta),
                       static_cast<uint32_t *>(d_table));
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
