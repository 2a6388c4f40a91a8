// jpegr_pack.hip -- the JPR stream from and to slots: the entropy stage's fixed
// slots (256 B of bits, 3 meta words, 256 table words per tile) packed into one
// byte stream of variable-length tile records behind a u16 size index, in
// either format, and the inverse for JPR1 (format: include/jpegr.h).  A JPT1
// stream is JPR1's header, index and record order with each stream's table in
// the tightest of three codings:
//   mode 0  ncodes x { i16 value, u8 length }             (JPR1's entries)
//   mode 1  ceil(ncodes / 2) bytes of nibble lengths, ncodes x i8 value
//   mode 2  ceil(ncodes / 2) bytes of nibble lengths, ncodes x i16 value
// The writer's mode is canonical (table_mode): 1 when ncodes > 0, every length
// <= 15 and every value fits an i8; else 2 when ncodes > 0 and every length
// <= 15; else 0.
//
//   pack    jpr_pack_sizes   JPR1.  A lane per tile: record size -> u32 (scan
//                            input) and the stream's u16 index; the 16-B header
//           jpt_pack_sizes   JPT1: the sizes depend on the tables.  A workgroup
//                            per 16 tiles, a wave per 4: entry k of a stream on
//                            lane k (the emit pass's lanes), each stream's mode
//                            from two ballots, then as jpr_pack_sizes
//           lz4_scan_reduce / lz4_scan_partials (lz4r_scan.h, as they are):
//                            groups of 64 tiles, partials of 4,096; the end
//                            of the scan is the stream length
//           jpr_pack_emit<kTight>  a workgroup per 16 tiles: records into an
//                            LDS image of its output range, out as 16-B stores.
//                            JPT1: the modes are not stored, the kernel ballots
//                            them again from the table words it loads anyway
//   unpack  jpr_unpack_sizes index -> u32 sizes, header verdict
//           the same scan    -> the length the header and index imply
//           jpr_unpack_tiles a workgroup per 16 tiles: its input range
//                            through LDS, records checked and scattered
// One emit kernel serves both formats: with kTight == false every mode is the
// constant 0 and what is left is the JPR1 kernel.  The format's
// pieces (the table writes too, which jpegr_select.hip's re-coding shares), the
// run and the image's flush are jpegr_pack_common.h's.
// No host-side state, no host read-back: every call can be captured in a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_pack_common.h"

namespace {

__global__ __launch_bounds__(256) void jpr_pack_sizes(const uint32_t *__restrict__ meta,
                                                      size_t ntiles, size_t t_base,
                                                      uint32_t *__restrict__ tsz,
                                                      uint8_t *__restrict__ out, uint64_t cap,
                                                      uint32_t w, uint32_t h, uint32_t nimg) {
  const size_t t = t_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t sz = stream_bytes(meta[3 * t], 0, 0u) + stream_bytes(meta[3 * t + 1], 1, 0u) +
                      stream_bytes(meta[3 * t + 2], 2, 0u);
  tsz[t] = sz;
  put_index(out, cap, t, sz);
  if (t == 0) put_header(out, cap, kMagicJPR1, w, h, nimg);
}

// the live table words of a tile on this lane (0 where not live)
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
      put_index(out, cap, t, sz);
    }
  }
  if (t0 == 0 && tid == 0) put_header(out, cap, kMagicJPT1, w, h, nimg);
}

// A workgroup's 16 tiles -> stream bytes [G0, G1).  Wave v takes tiles
// 4 v .. 4 v + 3; per tile a lane holds five dwords of the slots -- table
// words lane, 64 + lane (Y), 128 + lane (Cr), 192 + lane (Cb) and dword
// `lane` of the 256 bit bytes -- loaded only where live, all 20 issued
// before the first is used.  Every byte of the range is written once (the
// records are dense), by byte stores, so the image needs no zeroing and byte
// stores to LDS need no atomics.
// JPT1 writes the table by mode (put_table_word, jpegr_pack_common.h, as the
// stream headers' put_stream_headers: jprs_select_emit re-codes with the same).
template <bool kTight>
__global__ __launch_bounds__(64 * kPW) void jpr_pack_emit(
    const uint8_t *__restrict__ bits, const uint32_t *__restrict__ meta,
    const uint32_t *__restrict__ table, size_t ntiles, size_t wg_base,
    const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, uint8_t *__restrict__ out, uint64_t cap) {
  __shared__ uint64_t toff[kGT + 1];
  __shared__ alignas(16) uint8_t img[kImg];
  __shared__ uint32_t smeta[kRun * 3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const auto [g, t0, h0, ntl] = run_of(wg_base + blockIdx.x, ntiles);
  if (t0 >= ntiles) return;
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
    uint32_t mds = 0u;
    if constexpr (kTight)
      mds = tile_modes(tb[i], meta_codes(m[0], 0), meta_codes(m[1], 1), meta_codes(m[2], 2));
    const uint32_t md[3] = {mds & 3u, (mds >> 2) & 3u, mds >> 4};
    uint32_t o[3];                                      // each stream's first image byte
    o[0] = lead + (uint32_t)(toff[h0 + j] - G0);
    o[1] = o[0] + stream_bytes(m[0], 0, md[0]);
    o[2] = o[1] + stream_bytes(m[1], 1, md[1]);
    put_stream_headers(img, o, m, md, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = word_chan(q);
      put_table_word(img + o[c] + 4u, meta_codes(m[c], c), md[c], word_entry(q, lane), tb[i][q]);
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
  image_out(img, tid, lane, wv, G0, G1, lead, out, cap);
}

// ---- unpack ---------------------------------------------------------------------

__global__ __launch_bounds__(256) void jpr_unpack_sizes(const uint8_t *__restrict__ in,
                                                        uint64_t in_len, size_t ntiles,
                                                        size_t t_base, uint32_t w, uint32_t h,
                                                        uint32_t nimg, uint32_t *__restrict__ tsz,
                                                        uint64_t *__restrict__ result) {
  const size_t t = t_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  tsz[t] = get_index(in, in_len, t);
  if (t == 0) result[1] = header_ok(in, in_len, ntiles, w, h, nimg, false) ? ~0ull : 0ull;
}

// A workgroup's 16 records: its input range staged in LDS (16-B loads; the
// partial chunks at either end bytewise, so no read leaves [0, in_len)), a
// lane per tile checks its record (record_rule), then wave v scatters tiles
// 4 v .. 4 v + 3: table words and bit dwords rebuilt from the record's bytes,
// lanes as in jpr_pack_emit.  The window holds 16 records of the largest
// well-formed size, and a (well-formed) record behind an index entry over
// that is read from the stream directly.
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
  const auto [g, t0, h0, ntl] = run_of(wg_base + blockIdx.x, ntiles);
  if (t0 >= ntiles) return;
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
    uint32_t m[3] = {0u, 0u, 0u}, md = 0u;
    if (!record_rule<false>(rd, off, size, soff + 3 * tid, m, md)) {
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

// jpegr_pack_device and jpegr_pack_tight_device: argument check, sizes, scan, emit
template <bool kTight>
int pack(const void *d_bits, const void *d_meta, const void *d_table, int w, int h, int nimg,
         void *d_out, size_t cap, void *d_out_len, void *d_scratch, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_bits || !d_meta || !d_table || !d_out || !d_out_len || !d_scratch || ntiles == 0 ||
      misaligned(d_bits, 3) || misaligned(d_meta, 3) || misaligned(d_table, 3) || misaligned(d_out, 15) ||
      misaligned(d_out_len, 7) || misaligned(d_scratch, 15))
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch s = scratch_of(d_scratch, ntiles);
  auto *bits = static_cast<const uint8_t *>(d_bits);
  auto *meta = static_cast<const uint32_t *>(d_meta);
  auto *tab = static_cast<const uint32_t *>(d_table);
  auto *out = static_cast<uint8_t *>(d_out);
  if constexpr (kTight)
    launch_chunks(ntiles, kRun, [&](size_t b, unsigned n) {
      hipLaunchKernelGGL(jpt_pack_sizes, dim3(n), dim3(64 * kPW), 0, st, meta, tab, ntiles, b, s.tsz, out,
                         (uint64_t)cap, (uint32_t)w, (uint32_t)h, (uint32_t)nimg);
    });
  else
    launch_chunks(ntiles, 256, [&](size_t b, unsigned n) {
      hipLaunchKernelGGL(jpr_pack_sizes, dim3(n), dim3(256), 0, st, meta, ntiles, b * 256, s.tsz, out,
                         (uint64_t)cap, (uint32_t)w, (uint32_t)h, (uint32_t)nimg);
    });
  scan(s, ntiles, static_cast<uint64_t *>(d_out_len), st);
  launch_chunks(ntiles, kRun, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jpr_pack_emit<kTight>, dim3(n), dim3(64 * kPW), 0, st, bits, meta, tab, ntiles, b,
                       s.tsz, s.gsum, s.part, out, (uint64_t)cap);
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
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
  if (!header || !w || !h || !nimg || header[2] != 'R') return JPEGR_ERR_ARG;
  return parse_header(header, w, h, nimg) ? JPEGR_OK : JPEGR_ERR_ARG;
}

extern "C" int jpegr_stream_format(const uint8_t header[16], int *w, int *h, int *nimg, int *format) {
  if (!header || !w || !h || !nimg || !format) return JPEGR_ERR_ARG;
  const int f = parse_header(header, w, h, nimg);
  if (f) *format = f;
  return f ? JPEGR_OK : JPEGR_ERR_ARG;
}

extern "C" int jpegr_pack_device(const void *d_bits, const void *d_meta, const void *d_table,
                                 int w, int h, int nimg, void *d_out, size_t cap,
                                 void *d_out_len, void *d_scratch, void *stream) {
  return pack<false>(d_bits, d_meta, d_table, w, h, nimg, d_out, cap, d_out_len, d_scratch, stream);
}

extern "C" int jpegr_pack_tight_device(const void *d_bits, const void *d_meta, const void *d_table,
                                       int w, int h, int nimg, void *d_out, size_t cap,
                                       void *d_out_len, void *d_scratch, void *stream) {
  return pack<true>(d_bits, d_meta, d_table, w, h, nimg, d_out, cap, d_out_len, d_scratch, stream);
}

extern "C" int jpegr_unpack_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                   void *d_bits, void *d_meta, void *d_table, void *d_scratch,
                                   void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_in || !d_bits || !d_meta || !d_table || !d_scratch || !d_result || ntiles == 0 ||
      misaligned(d_bits, 3) || misaligned(d_meta, 3) || misaligned(d_table, 3) || misaligned(d_result, 7) ||
      misaligned(d_scratch, 15))
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch s = scratch_of(d_scratch, ntiles);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *result = static_cast<uint64_t *>(d_result);
  launch_chunks(ntiles, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jpr_unpack_sizes, dim3(n), dim3(256), 0, st, in, (uint64_t)in_len, ntiles, b * 256,
                       (uint32_t)w, (uint32_t)h, (uint32_t)nimg, s.tsz, result);
  });
  scan(s, ntiles, result, st);
  launch_chunks(ntiles, kRun, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jpr_unpack_tiles, dim3(n), dim3(64 * kPW), 0, st, in, (uint64_t)in_len, ntiles, b,
                       s.tsz, s.gsum, s.part, result, static_cast<uint8_t *>(d_bits),
                       static_cast<uint32_t *>(d_meta), static_cast<uint32_t *>(d_table));
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
