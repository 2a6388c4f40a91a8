// jpegr_thumb.hip -- 1/8-scale thumbnails from a JPR1 or JPT1 stream's DC terms
// alone (include/jpegr.h: jpegr_thumb_device): one RGBA pixel per tile, images
// [image0, image0 + nimage) of the stream, no decode state, no coefficients,
// no IDCT.  With every AC term 0 the reference's IDCT (JPEG.c:399-448) has one
// nonzero product per sample, the u = v = 0 one, whose cosines are exactly
// 1.0: every sample of a plane is round_clamp_u8(aa00 * (dc * T0) + 128), the
// tile is one colour, and that colour is the thumbnail's pixel.
//
//   jprs_sizes, the index scan   (jpegr_pack_common.h: sizes_and_scan) when
//                 the caller keeps no offsets; jprs_sizes initialises the
//                 result words
//   jprs_thumb_init   with the caller's offsets instead: the result words from
//                 the header and off[ntiles]; no sizes, no scan
//   jprs_thumb    a wave (a workgroup) per 64 consecutive tiles of the range, a
//                 lane per tile.  The lane finds its record (scan_record, or
//                 the caller's offsets, which are not trusted), checks it by
//                 record_rule, and walks each of its three streams only
//                 until the first (count >= 1, value) pair has its value:
//                 decode_stream_slow's search, cut off early.  The wave's
//                 pixels leave as one 256-B run, its DC quads as 512 B; it
//                 reports through RangeReport (jpegr_pack_common.h's, as
//                 scan_record and record_rule; through record_at and a shared
//                 table reader the call was 0.3 to 1.4 % slower).
//
// The record read.  A wave's 64 records are one contiguous span of the stream.
// JPRS_THUMB_WINDOW = 1 (shipped): the wave copies the span into a 12-KiB LDS
// window with coalesced 16-B loads and every lane reads its record's bytes
// from there; a span that does not fit (long records, offsets that are not a
// run) is read from global memory a byte at a time, inside the checked record,
// as jprs_decode's StreamSrc does.  JPRS_THUMB_WINDOW = 0: always the latter.
// Both measured: DESIGN 4.14.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpeg_tables.h"
#include "jpegr_pack_common.h"
#include "jpegr_pixel.h"

#pragma clang fp contract(off)

#ifndef JPRS_THUMB_WINDOW
#define JPRS_THUMB_WINDOW 1
#endif

namespace {

constexpr int kWave = 64;                    // tiles a wave
constexpr bool kWindow = JPRS_THUMB_WINDOW != 0;
// The window: a random image's 64 records are 9.6 KB, a smooth one's 2 to 3 KB;
// 12 KiB leave 13 waves a CU.  It holds the span from the 16-B boundary below it.
constexpr int kWinBytes = 12 * 1024;
constexpr int kStage = 4;                    // 16-B loads a lane in flight while staging (12: the same time)
constexpr int kAhead = 4;                    // table lengths read ahead of the search (8: no faster)

// the recon kernel's dequantiser step and alpha product at zigzag 0, which is
// natural index 0 of either plane
static_assert(jpegr_tables::ZZ8_POS[0] == 0 && jpegr_tables::ZZ4_POS[0] == 0, "zigzag 0 is the DC");
constexpr double kYStep = (double)jpegr_tables::LUMA_Q[0], kYAlpha = jpegr_tables::AA88[0][0];
constexpr double kCStep = (double)jpegr_tables::CHROMA_Q[0], kCAlpha = jpegr_tables::AA84[0][0];

// A plane's sample when only its DC is nonzero: jpeg_recon_kernel's
// aa * (q * step), times the two cosines 1.0, added to a sum of 0.0 -- all
// exact -- then (int)round(s + 128) clamped (JPEG.c:440).
__device__ __forceinline__ int dc_sample(int dc, double step, double alpha) {
  return round_clamp_u8(alpha * ((double)dc * step) + 128.0);
}

// zz[0] of a stream (jo_entropy_decode): the value of the first (count, value)
// pair whose count is >= 1, else 0.  rd(x): byte x of the checked record; so,
// m, mode: the stream's offset in it, its meta word and its JPT1 table mode
// (0 in a JPR1 stream), from record_rule, so every byte read lies inside the
// record.  The search per symbol is decode_stream_slow's: the codes follow from
// the lengths, the first entry in table order whose code is the window's top
// bits and fits in nbits is the symbol.  The walk ends with the DC: the rest of
// the stream is not validated.  What the prefix shows the full decoder would
// reject (no codes, no or too many RLE ints, a length of 0 or past 32, no
// code at the position) counts into fails and gives 0.
template <typename Rd>
__device__ __forceinline__ int stream_dc(Rd rd, uint32_t so, uint32_t m, uint32_t mode, int n,
                                         uint32_t &fails) {
  const int nbits = (int)(m & 0xFFFFu), R = (int)((m >> 16) & 255u), U = (int)(m >> 24);
  if (U == 0 || R == 0 || R > 2 * n) {
    ++fails;
    return 0;
  }
  if (R < 2) return 0;                                 // a count with no value
  // the table by mode (StreamSrc, jpegr_stream.hip): 3-B entries, or nibble
  // lengths then 1- or 2-B values; then the bit bytes
  const uint32_t tl = so + 4u;
  const uint32_t pv = tl + (mode ? (uint32_t)((U + 1) >> 1) : 0u);
  const uint32_t pb = pv + (mode ? mode * (uint32_t)U : 3u * (uint32_t)U);
  auto len = [&](int k) -> int {
    return mode == 0 ? (int)rd(tl + 3u * k + 2u) : (int)((rd(tl + (k >> 1)) >> (4 * (k & 1))) & 15u);
  };
  auto value = [&](int k) -> int {
    if (mode == 1) return (int)(int8_t)rd(pv + k);
    const uint32_t e = pv + (mode ? 2u : 3u) * k;
    return (int)(int16_t)(rd(e) | rd(e + 1u) << 8);
  };
  if (U == 1) {                                        // rle_len copies of the one symbol
    const int v = value(0);
    return v >= 1 ? v : 0;
  }
  const int nby = (nbits + 7) >> 3;
  auto byte = [&](int j) -> uint32_t { return j < nby ? rd(pb + j) : 0u; };
  int p = 0, pending = 0;
  bool have = false;
  for (int got = 0; got < R && p < nbits; ++got) {
    const int bi = p >> 3, sh = p & 7;
    const uint32_t w0 = byte(bi) << 24 | byte(bi + 1) << 16 | byte(bi + 2) << 8 | byte(bi + 3);
    uint32_t win = sh ? (w0 << sh) | (byte(bi + 4) >> (8 - sh)) : w0;
    if (nbits - p < 32) win &= ~0u << (32 - (nbits - p));
    // kAhead lengths are read before the first is looked at (an index past the
    // table reads its last entry again): a read per entry, each waiting for
    // the one before, was the walk's longest chain
    uint32_t code = 0;
    int plen = 0, hit = -1, L = 0;
    bool bad = false;
    for (int k0 = 0; k0 < U && hit < 0 && !bad; k0 += kAhead) {
      int Ls[kAhead];
#pragma unroll
      for (int j = 0; j < kAhead; ++j) Ls[j] = len(min(k0 + j, U - 1));
#pragma unroll
      for (int j = 0; j < kAhead; ++j) {
        const int k = k0 + j;
        if (k < U && hit < 0 && !bad) {
          L = Ls[j];
          bad = L == 0 || L > 32;
          if (!bad) {
            if (k) code = L >= plen ? (code + 1) << (L - plen) : (code + 1) >> (plen - L);
            plen = L;
            if (p + L <= nbits && (win >> (32 - L)) == code) hit = k;
          }
        }
      }
    }
    if (bad || hit < 0) {
      ++fails;
      return 0;
    }
    const int v = value(hit);
    if (!have) {
      pending = v;
      have = true;
    } else {
      if (pending >= 1) return v;
      have = false;
    }
    p += L;
  }
  return 0;
}

// The lane's record of `size` bytes, byte x of it rd(x): record_rule, then the
// three DCs.  Returns whether the record is well-formed; a malformed record's
// DCs are 0 and nothing of it is read past the rule's own reads.
template <bool kTight, typename Rd>
__device__ __forceinline__ bool record_dc(Rd rd, uint32_t size, int (&dc)[3], uint32_t &fails) {
  uint32_t so[3] = {0u, 0u, 0u}, m[3] = {0u, 0u, 0u}, md = 0u;
  if (!record_rule<kTight>(rd, 0u, size, so, m, md)) return false;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    dc[c] = stream_dc(rd, so[c], m[c], kTight ? (md >> (2 * c)) & 3u : 0u, c ? 32 : 64, fails);
  return true;
}

// The result words when the caller keeps the offsets: [0] off[ntiles], [1] the
// header's verdict and whether that length is in_len, [2] 0.
__global__ void jprs_thumb_init(const uint8_t *__restrict__ in, uint64_t in_len, size_t ntiles,
                                uint32_t w, uint32_t h, uint32_t nimg,
                                const uint64_t *__restrict__ toff, uint64_t *__restrict__ result) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint64_t implied = toff[ntiles];
  result[0] = implied;
  result[1] = header_ok(in, in_len, ntiles, w, h, nimg, true) && implied == in_len ? ~0ull : 0ull;
  result[2] = 0ull;
}

// toff: the caller's offsets (then tsz, gsum, part are not read), or nullptr
// (then the scan's).  rgba, dcq: either may be nullptr.
__global__ __launch_bounds__(kWave) void jprs_thumb(
    const uint8_t *__restrict__ in, uint64_t in_len, size_t tile0, size_t ntile, size_t wg_base,
    const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, const uint64_t *__restrict__ toff,
    uint64_t *__restrict__ result, uint32_t *__restrict__ rgba, uint2 *__restrict__ dcq) {
  __shared__ uint4 win[kWindow ? kWinBytes / 16 : 1];
  const int lane = threadIdx.x;
  const size_t first = (wg_base + blockIdx.x) * kWave;          // of the range
  if (first >= ntile) return;
  const size_t a = tile0 + first;                               // the wave's first tile
  const int ntl = (int)min((size_t)kWave, ntile - first);
  const bool on = lane < ntl;
  // the colour of all-zero coefficients
  const int grey = dc_sample(0, kYStep, kYAlpha), cgrey = dc_sample(0, kCStep, kCAlpha);
  const uint64_t implied = result[0], head = result[1];
  if (head == 0 || implied != in_len) {                         // the same in every wave
    if (on) {
      if (rgba) rgba[first + lane] = rgba_of(grey, cgrey, cgrey);
      if (dcq) dcq[first + lane] = make_uint2(0u, 0u);
    }
    if (lane == 0 && head != 0) atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 0ull);
    return;
  }
  // the lane's record: o0 its offset in the stream, size its bytes, valid
  // whether it lies in the stream with a record's size
  uint64_t o0 = 0;
  uint32_t size = 0;
  bool valid = on;
  if (toff != nullptr) {                                        // record_at's rule, spelled here
    if (on) {                                                   // a + lane < ntiles: off[.. + 1] is the caller's
      o0 = toff[a + lane];
      const uint64_t o1 = toff[a + lane + 1];
      valid = o0 <= o1 && o1 <= in_len && o1 - o0 >= kEmptyRec && o1 - o0 <= (uint64_t)kRecMax;
      size = valid ? (uint32_t)(o1 - o0) : 0u;
    }
  } else {                                                      // implied == in_len: every offset lies inside the stream
    const ScanRec r = scan_record(lane, a, ntl, tsz, gsum, part);
    o0 = r.offset();
    size = r.size;
  }
  const uint8_t *const rec = in + o0;
  uint32_t roff = 0;
  bool staged = false;
  if constexpr (kWindow) {
    // the span of the wave's valid records, [lo, hi) of the stream
    uint64_t lo = valid ? o0 : ~0ull, hi = valid ? o0 + size : 0ull;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      lo = min(lo, (uint64_t)__shfl_xor((unsigned long long)lo, d, kWave));
      hi = max(hi, (uint64_t)__shfl_xor((unsigned long long)hi, d, kWave));
    }
    const uint32_t lead = lo < hi ? (uint32_t)(reinterpret_cast<uintptr_t>(in + lo) & 15u) : 0u;
    staged = lo < hi && lo >= lead && hi - lo <= (uint64_t)(kWinBytes - 16);
    if (staged) {                                               // wave-uniform
      // 16-B chunks from the boundary below in + lo: chunk i is stream bytes
      // [s0 + 16 i, s0 + 16 i + 16), loaded whole when it ends inside the
      // stream, else (the last one only: hi <= in_len) its bytes below in_len
      const uint64_t s0 = lo - lead;
      const uint8_t *const src = in + s0;
      const uint32_t nch = (lead + (uint32_t)(hi - lo) + 15u) >> 4;
      const uint32_t nsafe = (uint32_t)min((uint64_t)nch, (in_len - s0) >> 4);
      // kStage loads a lane in flight before the first is written; a lane past
      // the last chunk loads that chunk again
#pragma unroll 1
      for (uint32_t i0 = 0; i0 < nsafe; i0 += kStage * kWave) {
        uint4 v[kStage];
#pragma unroll
        for (int k = 0; k < kStage; ++k)
          v[k] = reinterpret_cast<const uint4 *>(src)[min(i0 + k * kWave + lane, nsafe - 1u)];
#pragma unroll
        for (int k = 0; k < kStage; ++k)
          if (i0 + k * kWave + lane < nsafe) win[i0 + k * kWave + lane] = v[k];
      }
      const uint32_t x = 16u * nsafe + (uint32_t)lane;
      if (nsafe < nch && lane < 16 && s0 + x < in_len) reinterpret_cast<uint8_t *>(win)[x] = src[x];
      roff = lead + (uint32_t)(o0 - lo);                        // valid lanes: < kWinBytes
    }
    __syncthreads();
  }
  int dc[3] = {0, 0, 0};
  uint32_t fails = 0;
  bool good = false;
  // the stream's format, from the header the first launch accepted: one for the launch
  const bool tight = __builtin_amdgcn_readfirstlane((uint32_t)in[2]) == 'T';
  if (valid) {
    if (kWindow && staged) {
      const uint8_t *const wb = reinterpret_cast<const uint8_t *>(win) + roff;
      auto rd = [&](uint32_t x) -> uint32_t { return wb[x]; };
      good = tight ? record_dc<true>(rd, size, dc, fails) : record_dc<false>(rd, size, dc, fails);
    } else {
      auto rd = [&](uint32_t x) -> uint32_t { return rec[x]; };
      good = tight ? record_dc<true>(rd, size, dc, fails) : record_dc<false>(rd, size, dc, fails);
    }
  }
  const RangeReport rep{result};
  if (on) {
    if (!good) rep.malformed(a + lane);
    if (rgba)
      rgba[first + lane] = rgba_of(dc_sample(dc[0], kYStep, kYAlpha), dc_sample(dc[1], kCStep, kCAlpha),
                                   dc_sample(dc[2], kCStep, kCAlpha));
    if (dcq)
      dcq[first + lane] = make_uint2((uint32_t)(uint16_t)dc[0] | (uint32_t)(uint16_t)dc[1] << 16,
                                     (uint32_t)(uint16_t)dc[2]);
  }
  rep.rejected(fails, lane);                                    // 0 .. 3 a lane, every lane of the wave
}

}  // namespace

extern "C" size_t jpegr_thumb_scratch_bytes(size_t ntiles) { return scratch_of(nullptr, ntiles).bytes; }

extern "C" int jpegr_thumb_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                  const void *d_tile_offsets, size_t image0, size_t nimage,
                                  void *d_rgba_out, void *d_dc_out, void *d_scratch, void *d_result,
                                  void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_in || !d_result || (!d_rgba_out && !d_dc_out) || ntiles == 0 || nimage == 0 ||
      image0 > (size_t)nimg || nimage > (size_t)nimg - image0 || in_len < (size_t)kHdr ||
      (!d_tile_offsets && !d_scratch) || misaligned(d_tile_offsets, 7) || misaligned(d_rgba_out, 15) ||
      misaligned(d_dc_out, 7) || misaligned(d_result, 7) || misaligned(d_scratch, 15))
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *toff = static_cast<const uint64_t *>(d_tile_offsets);
  auto *result = static_cast<uint64_t *>(d_result);
  const size_t per = ntiles / (size_t)nimg;
  Scratch s = {nullptr, nullptr, nullptr, 0, 0};
  if (toff) {
    hipLaunchKernelGGL(jprs_thumb_init, dim3(1), dim3(kWave), 0, st, in, (uint64_t)in_len, ntiles,
                       (uint32_t)w, (uint32_t)h, (uint32_t)nimg, toff, result);
  } else {
    s = scratch_of(d_scratch, ntiles);
    sizes_and_scan<true>(in, in_len, ntiles, w, h, nimg, s, result, st);
  }
  launch_chunks(nimage * per, kWave, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_thumb, dim3(n), dim3(kWave), 0, st, in, (uint64_t)in_len, image0 * per,
                       nimage * per, b, s.tsz, s.gsum, s.part, toff, result,
                       static_cast<uint32_t *>(d_rgba_out), static_cast<uint2 *>(d_dc_out));
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
