// jpegr_stream.hip -- entropy decode straight from the JPR stream, JPR1 or
// JPT1 (include/jpegr.h): tiles [tile0, tile0 + ntile) of a stream to
// coefficients, no slots in between.  The format is the header's, one for the
// launch: jprs_decode branches once into the record routine of that format
// (decode_record<kTight>).  The index and header reader and the
// rule that makes a record malformed are the ones unpack uses
// (jpegr_pack_common.h: get_index, header_ok, record_rule).
//
//   jprs_sizes    index -> u32 sizes (the scan's input), the header verdict in
//                 result[1], result[2] = 0: the call's first launch initialises
//                 its own result words, the later launches follow it in stream
//                 order -- no memset, no tag, no spin
//   the index scan (jpegr_pack_common.h, lz4r_scan.h as it is) -> result[0]
//   jprs_decode   a workgroup per 64 tiles of the range, counted from tile0: a
//                 luma wave (a lane decodes its tile's Y stream) and a chroma
//                 wave (its Cr, then its Cb stream), as entropy_decode_kernel
//                 pairs them.  Each wave finishes the scan for its 64 tiles in
//                 registers; a lane then reads its record from the stream
//                 itself, byte-granular and inside the checked record.  No LDS
//                 window over the records: the decode state alone (19.3 KiB)
//                 keeps eight workgroups on a CU, and every window size tried
//                 cost more in residency than its 16-B staging saved
//                 (DESIGN 4.9).
//
// The per-stream walk is the slot decoder's (jpegr_decode_common.h:
// decode_stream / decode_stream_slow, the decode state, the carry-chain
// compare) over another source of bits: StreamSrc below reads 3-B unaligned
// or nibble-coded table entries and bit bytes with no slot behind them, so
// every read is bounded by the stream's own length instead of whole 16-B
// chunks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_decode_common.h"
#include "jpegr_pack_common.h"

namespace {

__global__ __launch_bounds__(256) void jprs_sizes(const uint8_t *__restrict__ in, uint64_t in_len,
                                                  size_t ntiles, size_t t_base, uint32_t w,
                                                  uint32_t h, uint32_t nimg,
                                                  uint32_t *__restrict__ tsz,
                                                  uint64_t *__restrict__ result) {
  const size_t t = t_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  tsz[t] = get_index(in, in_len, t);
  if (t == 0) {
    result[1] = header_ok(in, in_len, ntiles, w, h, nimg, true) ? ~0ull : 0ull;
    result[2] = 0ull;
  }
}

// A stream's bytes in the JPR stream: sp[0..4) its header, then its table
// (StreamSrc below), then nby bit bytes at pb.  The record was checked, so all
// of them lie inside it; nothing else is read: a table index is clamped to
// U - 1 and a bit byte past nby reads sp[0] instead (in bounds, and what lies
// past the bits cannot change a decode: see decode_stream's lookup).
struct BitBytes {
  const uint8_t *sp, *pb;
  int nby;
  __device__ __forceinline__ uint32_t byte(int j) const { return *(j < nby ? pb + j : sp); }
  // bit bytes j .. j + 3, the first in the top byte (MSB-first bits)
  __device__ __forceinline__ uint32_t be32(int j) const {
    return byte(j) << 24 | byte(j + 1) << 16 | byte(j + 2) << 8 | byte(j + 3);
  }
  // the 32 bits at bit p (decode_stream_slow)
  __device__ __forceinline__ uint32_t window(int p) const {
    const int bi = p >> 3, sh = p & 7;
    const uint32_t w0 = be32(bi);
    return sh ? (w0 << sh) | (byte(bi + 4) >> (8 - sh)) : w0;
  }
};

// What both walks read of a stream (decode_stream's ByteBits and table head,
// decode_stream_slow's window / len / entry).  JPR1: U table entries of 3 B.
template <bool kTight>
struct StreamSrc;

template <>
struct StreamSrc<false> : BitBytes {
  int U;
  __device__ __forceinline__ StreamSrc(const uint8_t *s, uint32_t m, uint32_t)
      : BitBytes{s, s + 4 + 3 * (m >> 24), (int)(((m & 0xFFFFu) + 7u) >> 3)}, U((int)(m >> 24)) {}
  // entry k as d_table's word: value | length << 16 (k < U)
  __device__ __forceinline__ uint32_t entry(int k) const {
    const uint8_t *e = sp + 4 + 3 * k;
    return (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16;
  }
  __device__ __forceinline__ int len(int k) const { return (int)sp[4 + 3 * k + 2]; }
  // the table's first min(U, Cap) entries, all loads issued before any is used
  template <int Cap>
  __device__ __forceinline__ void head(uint32_t (&tb)[Cap]) const {
#pragma unroll
    for (int k = 0; k < Cap; ++k) tb[k] = entry(min(k, U - 1));
  }
};

// A stream of a JPT1 record: its table by mode (0: JPR1's 3-B entries; 1, 2:
// ceil(U / 2) bytes of nibble lengths at sp + 4, then U values of 1 or 2 B at
// pv), then the bit bytes at pb.  The same rules: a table index is clamped to
// U - 1, so every read lies inside the stream's own checked bytes.
template <>
struct StreamSrc<true> : BitBytes {
  const uint8_t *pv;
  int U;
  uint32_t mode;
  __device__ __forceinline__ StreamSrc(const uint8_t *s, uint32_t m, uint32_t md)
      : BitBytes{s, nullptr, (int)(((m & 0xFFFFu) + 7u) >> 3)}, U((int)(m >> 24)), mode(md) {
    pv = s + 4 + (md ? (U + 1) >> 1 : 0);
    pb = pv + (md ? (int)md * U : 3 * U);
  }
  __device__ __forceinline__ int len(int k) const {
    return mode == 0 ? (int)sp[4 + 3 * k + 2] : (int)((sp[4 + (k >> 1)] >> (4 * (k & 1))) & 15u);
  }
  __device__ __forceinline__ uint32_t value(int k) const {     // the i16 as d_table's low half
    if (mode == 1) return (uint32_t)(uint16_t)(int8_t)pv[k];
    const uint8_t *e = pv + (mode ? 2 : 3) * k;
    return (uint32_t)e[0] | (uint32_t)e[1] << 8;
  }
  __device__ __forceinline__ uint32_t entry(int k) const { return value(k) | (uint32_t)len(k) << 16; }
  // A length byte is loaded once for its pair of entries: entry k + 1 past
  // U - 1 is never used, so the pair's upper nibble may stand for it.
  template <int Cap>
  __device__ __forceinline__ void head(uint32_t (&tb)[Cap]) const {
    static_assert(Cap % 2 == 0, "pairs of entries");
    if (mode == 1) {
#pragma unroll
      for (int k = 0; k < Cap; k += 2) {
        const uint32_t lb = sp[4 + (min(k, U - 1) >> 1)];
        tb[k] = (uint32_t)(uint16_t)(int8_t)pv[min(k, U - 1)] | (lb & 15u) << 16;
        tb[k + 1] = (uint32_t)(uint16_t)(int8_t)pv[min(k + 1, U - 1)] | (lb >> 4) << 16;
      }
    } else if (mode == 2) {
#pragma unroll
      for (int k = 0; k < Cap; k += 2) {
        const uint32_t lb = sp[4 + (min(k, U - 1) >> 1)];
        const uint8_t *e0 = pv + 2 * min(k, U - 1), *e1 = pv + 2 * min(k + 1, U - 1);
        tb[k] = (uint32_t)e0[0] | (uint32_t)e0[1] << 8 | (lb & 15u) << 16;
        tb[k + 1] = (uint32_t)e1[0] | (uint32_t)e1[1] << 8 | (lb >> 4) << 16;
      }
    } else {
#pragma unroll
      for (int k = 0; k < Cap; ++k) {
        const uint8_t *e = sp + 4 + 3 * min(k, U - 1);
        tb[k] = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16;
      }
    }
  }
};

// One wave's lanes of one channel group.  rec: the lane's record in the
// stream; so / m: its streams' offsets in the record and meta words;
// good: the record is well-formed (else its ints are 0 and nothing of it is
// read); md: the streams' table modes, Y | Cr << 2 | Cb << 4 (JPT1).  Returns
// the lane's rejected streams.
template <bool kLuma, bool kTight>
__device__ __forceinline__ uint32_t stream_decode_wave(DecLds<kLuma ? 64 : 32, kLuma ? kFastCap : kChromaCap> &S,
                                                 int lane, const uint8_t *rec, bool good,
                                                 const uint32_t (&so)[3], const uint32_t (&m)[3],
                                                 uint32_t md, int16_t *__restrict__ tile_out) {
  constexpr int Cap = kLuma ? kFastCap : kChromaCap;
  uint32_t fails = 0;
  int16_t *o = S.out[lane];
  const VRow vl{reinterpret_cast<uint8_t *>(&S.vl[0][lane])};
#pragma unroll 1
  for (int c = kLuma ? 0 : 1; c <= (kLuma ? 0 : 2); ++c) {
    const uint32_t mc = c == 0 ? m[0] : c == 1 ? m[1] : m[2];
    const uint32_t oc = c == 0 ? so[0] : c == 1 ? so[1] : so[2];
    const int n = stream_len(c);
    bool ok = false;
    if (good) {
      const StreamSrc<kTight> src(rec + oc, mc, (md >> (2 * c)) & 3u);
      const int U = (int)(mc >> 24);
      int r = U == 0 ? 0 : -1;
      if (U != 0 && U <= Cap) {
        uint32_t tb[Cap];
        src.head(tb);
        r = decode_stream<Cap, ByteBits<StreamSrc<kTight>>>(mc, tb, vl, o, n,
                                                            kLuma ? &S.bm[0][lane] : nullptr, &src);
      }
      ok = r < 0 ? decode_stream_slow(src, mc, o, n) : r != 0;
      fails += !ok;
    }
    if (!ok)                                          // a rejected stream, a malformed record: 0
      for (int j = 0; j < n; ++j) o[j] = 0;
    store_ints(o, tile_out + coef_off(c), n);
  }
  return fails;
}

// A lane's record of `size` bytes at rec, tile t of the stream: checked by
// the rule every reader shares (record_rule, jpegr_pack_common.h), whose reads
// stay inside the record; then the wave's channel group is decoded.
template <bool kTight>
__device__ __forceinline__ void decode_record(DecLds<64, kFastCap> &SY, DecLds<32, kChromaCap> &SC,
                                              int lane, int wv, const uint8_t *rec, uint32_t size,
                                              size_t t, uint64_t *__restrict__ result,
                                              int16_t *__restrict__ tile_out) {
  uint32_t so[3] = {0u, 0u, 0u}, m[3] = {0u, 0u, 0u}, md = 0u;
  const bool good = record_rule<kTight>([&](uint32_t x) -> uint32_t { return rec[x]; }, 0u, size, so, m, md);
  uint32_t fails;
  if (__builtin_amdgcn_readfirstlane(wv) == 0) {
    if (!good)
      atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 1ull + (unsigned long long)t);
    fails = stream_decode_wave<true, kTight>(SY, lane, rec, good, so, m, md, tile_out);
  } else {
    fails = stream_decode_wave<false, kTight>(SC, lane, rec, good, so, m, md, tile_out);
  }
  // the wave's rejected streams: one add, after jprs_sizes' zero in stream order
  const uint32_t f = wave_rejected(fails);
  if (f && lane == __builtin_ctzll(__ballot(1)))
    atomicAdd(reinterpret_cast<unsigned long long *>(result + 2), (unsigned long long)f);
}

__global__ __launch_bounds__(2 * kLanes) void jprs_decode(
    const uint8_t *__restrict__ in, uint64_t in_len, size_t ntiles, size_t tile0, size_t ntile,
    size_t wg_base, const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, uint64_t *__restrict__ result, int16_t *__restrict__ coef) {
  __shared__ DecLds<64, kFastCap> SY;
  __shared__ DecLds<32, kChromaCap> SC;
  const int tid = threadIdx.x, lane = tid & (kLanes - 1), wv = tid >> 6;
  const size_t first = (wg_base + blockIdx.x) * kLanes;     // of the range
  if (first >= ntile) return;
  const size_t a = tile0 + first;                           // the workgroup's first tile
  const int ntl = (int)min((size_t)kLanes, ntile - first);
  int16_t *const wg_out = coef + first * 128;
  const uint64_t implied = result[0], head = result[1];
  const uint32_t fmt = in_len >= (uint64_t)kHdr ? in[2] : 0u;   // 'R' or 'T' when head != 0
  if (head == 0 || implied != in_len) {                     // the same in every workgroup
    uint4 *dst = reinterpret_cast<uint4 *>(wg_out);
    for (int i = tid; i < ntl * 16; i += 2 * kLanes) dst[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 0ull);
    return;
  }
  // the lane's record: the scan's partial, the group sums before a's group,
  // that group's tiles before a, then a wave scan of the 64 sizes (each wave
  // for itself, in registers, all 64 lanes on: lanes past the range add 0)
  const size_t g = a / kGT, g0 = g * kGT;
  const int skip = (int)(a - g0);
  const size_t pi = g0 / kPart, gfirst = pi * 64;
  const uint32_t gs = (gfirst + lane < g) ? gsum[gfirst + lane] : 0u;
  const uint32_t sk = lane < skip ? tsz[g0 + lane] : 0u;
  const uint32_t size = lane < ntl ? tsz[a + lane] : 0u;
  // each sum < 2^32: at most 4,096 tiles of at most 65,535 B
  const uint64_t base = part[pi] + lane63(wave_incl_add(gs)) + lane63(wave_incl_add(sk));
  const uint32_t inc = wave_incl_add(size);
  if (lane >= ntl) return;
  // implied == in_len: every offset of the scan lies inside the stream
  const uint8_t *rec = in + (base + inc - size);
  int16_t *const tile_out = wg_out + (size_t)lane * 128;
  // the stream's format, from the header jprs_sizes accepted: one for the launch
  if (__builtin_amdgcn_readfirstlane(fmt) == 'T')
    decode_record<true>(SY, SC, lane, wv, rec, size, a + lane, result, tile_out);
  else
    decode_record<false>(SY, SC, lane, wv, rec, size, a + lane, result, tile_out);
}
}  // namespace

extern "C" int jpegr_stream_decode_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                          size_t tile0, size_t ntile, void *d_coef,
                                          void *d_scratch, void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_in || !d_coef || !d_scratch || !d_result || ntiles == 0 || ntile == 0 ||
      tile0 > ntiles || ntile > ntiles - tile0 ||
      (reinterpret_cast<uintptr_t>(d_coef) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_result) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(d_scratch) & 15) != 0)
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch s = scratch_of(d_scratch, ntiles);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *result = static_cast<uint64_t *>(d_result);
  launch_chunks(ntiles, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_sizes, dim3(n), dim3(256), 0, st, in, (uint64_t)in_len, ntiles, b * 256,
                       (uint32_t)w, (uint32_t)h, (uint32_t)nimg, s.tsz, result);
  });
  scan(s, ntiles, result, st);
  launch_chunks(ntile, kLanes, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_decode, dim3(n), dim3(2 * kLanes), 0, st, in, (uint64_t)in_len, ntiles, tile0,
                       ntile, b, s.tsz, s.gsum, s.part, result, static_cast<int16_t *>(d_coef));
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
