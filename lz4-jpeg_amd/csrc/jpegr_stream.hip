// jpegr_stream.hip -- entropy decode straight from the JPR stream, JPR1 or
// JPT1 (include/jpegr.h): tiles [tile0, tile0 + ntile) of a stream to
// coefficients, no slots in between.  The format is the header's, one for the
// launch: jprs_decode branches once into the record routine of that format
// (decode_record<kTight>).  What every reader of the stream does
// is jpegr_pack_common.h's: get_index, header_ok, record_rule, scan_record,
// record_at, RangeReport, sizes_and_scan.
//
//   jprs_sizes    (jpegr_pack_common.h: the thumbnails launch it too)
//                 index -> u32 sizes (the scan's input), the header verdict in
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
//   jpegr_stream_index_device keeps that scan: jprs_sizes, the scan, and
//                 jprs_index_finish, which stores every tile's offset
//   jpegr_crop_device decodes rectangles: jprs_crop_init (the result words,
//                 every rectangle's status), jprs_crop_decode (jprs_decode's
//                 shape over the rectangles' cells, records found through the
//                 caller's offsets), then jpeg_crop_recon_kernel (jpegr.hip);
//                 the mapping is in jpegr_crop.h, the numbers in DESIGN 4.13
//   jpegr_crop_tensor_device is the same call with elements for bytes:
//                 jprs_crop_tensor_init (the capacity rule in elements),
//                 jprs_crop_decode as it is, then jpeg_crop_tensor_kernel
//                 (jpegr.hip); DESIGN 4.16
//   jpegr_crop_resize_device resamples the rectangles to one size: its own
//                 first launch and last two are jpegr_resize.hip's
//                 (jpegr_resize.h); between them jprs_crop_decode and
//                 jpeg_crop_recon_kernel as they are, on shadow rectangles
//                 whose pixels go to the scratch; DESIGN 4.17
//   jpegr_dataset_crop_tensor_device, jpegr_dataset_crop_resize_device are
//                 those two calls over many streams of different sizes and
//                 formats (jpegr_dataset.h): jprs_dataset_crop_tensor_init (or
//                 jpegr_resize.hip's dataset init) finds each rectangle's
//                 stream, jprs_dataset_crop_decode decodes lanes of both
//                 formats in one wave; the rest as it is; DESIGN 4.18
//
// The per-stream walk is the slot decoder's (jpegr_decode_common.h:
// decode_stream / decode_stream_slow, the decode state, the carry-chain
// compare) over another source of bits: StreamSrc below reads 3-B unaligned
// or nibble-coded table entries and bit bytes with no slot behind them, so
// every read is bounded by the stream's own length instead of whole 16-B
// chunks.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_crop.h"
#include "jpegr_dataset.h"
#include "jpegr_decode_common.h"
#include "jpegr_pack_common.h"
#include "jpegr_resize.h"

namespace {

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
// decode_stream_slow's window / len / entry).  The table's layout by mode is
// spelled here and in jpegr_thumb.hip's stream_dc: through one shared reader
// jprs_decode grew by 291 instructions.  JPR1: U table entries of 3 B.
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

// Where decode_record reports: the direct decode through RangeReport
// (jpegr_pack_common.h), which states the two calls.
// A crop: either failure turns the lane's rectangle bad (stat: its status
// word) and is counted into result[2], after jprs_crop_init's zero.
struct CropReport {
  uint64_t *__restrict__ result;
  uint32_t *stat;
  __device__ __forceinline__ void malformed(size_t) const {
    *stat = jpegr_crop::kBad;
    atomicAdd(reinterpret_cast<unsigned long long *>(result + 2), 1ull);
  }
  __device__ __forceinline__ void rejected(uint32_t fails, int lane) const {
    if (fails) *stat = jpegr_crop::kBad;
    RangeReport{result}.rejected(fails, lane);
  }
};

// A lane's record of `size` bytes at rec, tile t of the stream: checked by
// the rule every reader shares (record_rule, jpegr_pack_common.h), whose reads
// stay inside the record; then the wave's channel group is decoded.
template <bool kTight, typename Report>
__device__ __forceinline__ void decode_record(DecLds<64, kFastCap> &SY, DecLds<32, kChromaCap> &SC,
                                              int lane, int wv, const uint8_t *rec, uint32_t size,
                                              size_t t, const Report rep,
                                              int16_t *__restrict__ tile_out) {
  uint32_t so[3] = {0u, 0u, 0u}, m[3] = {0u, 0u, 0u}, md = 0u;
  const bool good = record_rule<kTight>([&](uint32_t x) -> uint32_t { return rec[x]; }, 0u, size, so, m, md);
  uint32_t fails;
  if (__builtin_amdgcn_readfirstlane(wv) == 0) {
    if (!good) rep.malformed(t);
    fails = stream_decode_wave<true, kTight>(SY, lane, rec, good, so, m, md, tile_out);
  } else {
    fails = stream_decode_wave<false, kTight>(SC, lane, rec, good, so, m, md, tile_out);
  }
  rep.rejected(fails, lane);
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
  // the lane's record (each wave for itself, all 64 lanes on)
  const ScanRec r = scan_record(lane, a, ntl, tsz, gsum, part);
  const uint32_t size = r.size;
  if (lane >= ntl) return;
  // implied == in_len: every offset of the scan lies inside the stream
  const uint8_t *rec = in + r.offset();
  int16_t *const tile_out = wg_out + (size_t)lane * 128;
  // the stream's format, from the header jprs_sizes accepted: one for the launch
  if (__builtin_amdgcn_readfirstlane(fmt) == 'T')
    decode_record<true>(SY, SC, lane, wv, rec, size, a + lane, RangeReport{result}, tile_out);
  else
    decode_record<false>(SY, SC, lane, wv, rec, size, a + lane, RangeReport{result}, tile_out);
}

// ---- the index, kept (jpegr_stream_index_device) ----------------------------------

// A workgroup (one wave) per scan group: group_offsets' 64 offsets, stored; the
// last group stores the total too.  The verdict: jprs_sizes' header verdict in
// result[1], cleared here when the implied length (the scan's, result[0]) is
// not in_len.
__global__ __launch_bounds__(kGT) void jprs_index_finish(
    const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, size_t ntiles, size_t g_base, uint64_t in_len,
    uint64_t *__restrict__ result, uint64_t *__restrict__ toff_out) {
  __shared__ uint64_t toff[kGT + 1];
  const int tid = threadIdx.x;
  const size_t g = g_base + blockIdx.x, g0 = g * kGT;
  if (g0 >= ntiles) return;
  group_offsets(tid, g, ntiles, tsz, gsum, part, toff);
  __syncthreads();
  const int nt = (int)min((size_t)kGT, ntiles - g0);
  if (tid < nt) toff_out[g0 + tid] = toff[tid];
  if (tid == 0 && g0 + nt == ntiles) toff_out[ntiles] = toff[nt];   // lanes past nt added 0
  if (tid == 0 && g == 0 && result[0] != in_len) result[1] = 0ull;
}

// ---- crops (jpegr_crop_device; the mapping: jpegr_crop.h) ----------------------------

// The call's first launch: resets the result words and gives every rectangle
// its status from its own fields and the header (none of the sums can wrap:
// each is a comparison against what is left).
__global__ __launch_bounds__(256) void jprs_crop_init(
    const uint8_t *__restrict__ in, uint64_t in_len, size_t ntiles, uint32_t w, uint32_t h,
    uint32_t nimg, const jpegr_rect *__restrict__ rects, size_t nrects, size_t r_base,
    uint32_t max_w, uint32_t max_h, uint64_t out_cap, uint32_t *__restrict__ status,
    uint64_t *__restrict__ result) {
  const size_t r = r_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r == 0) {
    result[0] = 0ull;
    result[1] = ~0ull;
    result[2] = 0ull;
  }
  if (r >= nrects) return;
  const jpegr_rect rc = rects[r];
  uint32_t st = jpegr_crop::kGood;
  if (!header_ok(in, in_len, ntiles, w, h, nimg, true))
    st = jpegr_crop::kBad;
  else if (rc.w == 0 || rc.h == 0)
    st = jpegr_crop::kEmpty;
  else if (rc.image >= nimg || rc.w > max_w || rc.h > max_h || rc.x > w || rc.w > w - rc.x ||
           rc.y > h || rc.h > h - rc.y || (rc.dst & 3) != 0 || rc.dst > out_cap ||
           4 * rc.w * rc.h > out_cap - rc.dst)         // w, h < 2^31: the product cannot wrap
    st = jpegr_crop::kBad;
  status[r] = st;
}

// jprs_crop_init for jpegr_crop_tensor_device: dst and out_cap count elements,
// a rectangle takes 3 w h of them, and no dst is misaligned.  (Its own text:
// jprs_crop_init stays the code it was.)
__global__ __launch_bounds__(256) void jprs_crop_tensor_init(
    const uint8_t *__restrict__ in, uint64_t in_len, size_t ntiles, uint32_t w, uint32_t h,
    uint32_t nimg, const jpegr_rect *__restrict__ rects, size_t nrects, size_t r_base,
    uint32_t max_w, uint32_t max_h, uint64_t out_cap, uint32_t *__restrict__ status,
    uint64_t *__restrict__ result) {
  const size_t r = r_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r == 0) {
    result[0] = 0ull;
    result[1] = ~0ull;
    result[2] = 0ull;
  }
  if (r >= nrects) return;
  const jpegr_rect rc = rects[r];
  uint32_t st = jpegr_crop::kGood;
  if (!header_ok(in, in_len, ntiles, w, h, nimg, true))
    st = jpegr_crop::kBad;
  else if (rc.w == 0 || rc.h == 0)
    st = jpegr_crop::kEmpty;
  else if (rc.image >= nimg || rc.w > max_w || rc.h > max_h || rc.x > w || rc.w > w - rc.x ||
           rc.y > h || rc.h > h - rc.y || rc.dst > out_cap ||
           3 * rc.w * rc.h > out_cap - rc.dst)         // w, h < 2^31: the product cannot wrap
    st = jpegr_crop::kBad;
  status[r] = st;
}

// jprs_decode's shape -- 64 items a workgroup, a luma wave and a chroma wave --
// over the rectangles' cells: item i is cell i % K of rectangle i / K.  A lane
// finds its record through toff, the caller's offsets, which are not trusted:
// the record must lie in the stream and have a record's size before a byte of
// it is read; decode_record then reads inside it only.  The ints go to the
// item's 128 int16 of the scratch.
__global__ __launch_bounds__(2 * kLanes) void jprs_crop_decode(
    const uint8_t *__restrict__ in, uint64_t in_len, uint32_t tiles_x, uint32_t tiles_y,
    const uint64_t *__restrict__ toff, const jpegr_rect *__restrict__ rects, size_t nrects,
    uint32_t K, size_t wg_base, uint32_t *status, uint64_t *__restrict__ result,
    int16_t *__restrict__ coef) {
  __shared__ DecLds<64, kFastCap> SY;
  __shared__ DecLds<32, kChromaCap> SC;
  const int tid = threadIdx.x, lane = tid & (kLanes - 1), wv = tid >> 6;
  const size_t i = (wg_base + blockIdx.x) * kLanes + lane;
  const size_t r = i / K;
  if (r >= nrects) return;
  const uint32_t cell = (uint32_t)(i - r * K);
  uint32_t *const stat = status + r;
  if (*stat != jpegr_crop::kGood) return;            // bad on its own fields, empty, or a tile failed
  const jpegr_rect rc = rects[r];
  const jpegr_crop::Grid g = jpegr_crop::grid_of(rc);
  if ((uint64_t)cell >= (uint64_t)g.gw * g.gh) return;   // an idle cell
  const uint32_t cy = cell / g.gw, cx = cell - cy * g.gw;
  // inside the image (jprs_crop_init): t < ntiles, so toff[t + 1] is the caller's
  const size_t t = (rc.image * tiles_y + g.ty0 + cy) * tiles_x + g.tx0 + cx;
  uint64_t o0;
  uint32_t size;
  if (!record_at(toff, t, in_len, o0, size)) {
    if (wv == 0) CropReport{result, stat}.malformed(t);
    return;
  }
  const uint8_t *rec = in + o0;
  int16_t *const tile_out = coef + i * 128;
  const uint32_t fmt = in[2];                         // 'R' or 'T': the header jprs_crop_init accepted
  if (__builtin_amdgcn_readfirstlane(fmt) == 'T')
    decode_record<true>(SY, SC, lane, wv, rec, size, t, CropReport{result, stat}, tile_out);
  else
    decode_record<false>(SY, SC, lane, wv, rec, size, t, CropReport{result, stat}, tile_out);
}

// ---- crops from many streams (jpegr_dataset_crop_*_device; jpegr_dataset.h) --------

// jprs_crop_tensor_init over a dataset: the rectangle's stream by bisection
// (stream_of_image, which also judges the descriptor and its header), then
// jprs_crop_tensor_init's rules against that stream's own w, h and nimg, and
// the word the decode finds the stream by.  (Its own text: the single-stream
// kernels stay the code they were.)
__global__ __launch_bounds__(256) void jprs_dataset_crop_tensor_init(
    const jpegr_stream_desc *__restrict__ ds, uint64_t nstreams, const jpegr_rect *__restrict__ rects,
    size_t nrects, size_t r_base, uint32_t max_w, uint32_t max_h, uint64_t out_cap,
    uint32_t *__restrict__ status, uint64_t *__restrict__ where, uint64_t *__restrict__ result) {
  const size_t r = r_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r == 0) {
    result[0] = 0ull;
    result[1] = ~0ull;
    result[2] = 0ull;
  }
  if (r >= nrects) return;
  const jpegr_rect rc = rects[r];
  jpegr_stream_desc d;
  uint32_t s = 0, image = 0;
  uint32_t st = jpegr_crop::kGood;
  if (!jpegr_dataset::stream_of_image(ds, nstreams, rc.image, d, s, image))
    st = jpegr_crop::kBad;
  else if (rc.w == 0 || rc.h == 0)
    st = jpegr_crop::kEmpty;
  else if (rc.w > max_w || rc.h > max_h || rc.x > d.w || rc.w > d.w - rc.x || rc.y > d.h ||
           rc.h > d.h - rc.y || rc.dst > out_cap ||
           3 * rc.w * rc.h > out_cap - rc.dst)         // w <= max_w, h <= max_h < 2^31: no wrap
    st = jpegr_crop::kBad;
  status[r] = st;
  where[r] = jpegr_dataset::word_of(s, image);         // read for a good rectangle only
}

// jprs_crop_decode over a dataset: the same items, a luma wave and a chroma
// wave; a lane takes the stream, its length, its tile grid and its offsets from
// the descriptor its rectangle's word names (s < nstreams: the init kernel
// stored it for every good rectangle, and no other is read).  A workgroup's 64
// items span several rectangles, so the format is the lane's and no longer the
// launch's: a wave runs decode_record<true> on its JPT1 lanes, then
// decode_record<false> on its JPR1 lanes, and skips by ballot the one no lane
// needs.  decode_record and what it calls use the wave's active lanes only
// (ballots over them, a lane's own LDS column, atomics), as they already do
// behind jprs_crop_decode's idle cells and bad rectangles.
__global__ __launch_bounds__(2 * kLanes) void jprs_dataset_crop_decode(
    const jpegr_stream_desc *__restrict__ ds, const uint64_t *__restrict__ where,
    const jpegr_rect *__restrict__ rects, size_t nrects, uint32_t K, size_t wg_base, uint32_t *status,
    uint64_t *__restrict__ result, int16_t *__restrict__ coef) {
  __shared__ DecLds<64, kFastCap> SY;
  __shared__ DecLds<32, kChromaCap> SC;
  const int tid = threadIdx.x, lane = tid & (kLanes - 1), wv = tid >> 6;
  const size_t i = (wg_base + blockIdx.x) * kLanes + lane;
  const size_t r = i / K;
  if (r >= nrects) return;
  const uint32_t cell = (uint32_t)(i - r * K);
  uint32_t *const stat = status + r;
  if (*stat != jpegr_crop::kGood) return;            // bad on its own fields or its stream, empty, or a tile failed
  const jpegr_rect rc = rects[r];
  const jpegr_crop::Grid g = jpegr_crop::grid_of(rc);
  if ((uint64_t)cell >= (uint64_t)g.gw * g.gh) return;   // an idle cell
  const uint32_t cy = cell / g.gw, cx = cell - cy * g.gw;
  const uint64_t wh = where[r];
  const jpegr_stream_desc d = ds[wh >> 32];
  const uint32_t tiles_x = jpegr_dataset::tiles_across(d.w), tiles_y = jpegr_dataset::tiles_across(d.h);
  // inside the image (the init kernel): t < ntiles <= 2^32, so toff[t + 1] is the caller's
  const size_t t = ((size_t)(uint32_t)wh * tiles_y + g.ty0 + cy) * tiles_x + g.tx0 + cx;
  const uint8_t *const in = static_cast<const uint8_t *>(d.d_in);
  uint64_t o0;
  uint32_t size;
  if (!record_at(static_cast<const uint64_t *>(d.d_tile_offsets), t, d.in_len, o0, size)) {
    if (wv == 0) CropReport{result, stat}.malformed(t);
    return;
  }
  const uint8_t *rec = in + o0;
  int16_t *const tile_out = coef + i * 128;
  const bool tight = in[2] == 'T';                    // 'R' or 'T': the header the init kernel accepted
  if (__ballot(tight) != 0) {
    if (tight) decode_record<true>(SY, SC, lane, wv, rec, size, t, CropReport{result, stat}, tile_out);
  }
  if (__ballot(!tight) != 0) {
    if (!tight) decode_record<false>(SY, SC, lane, wv, rec, size, t, CropReport{result, stat}, tile_out);
  }
}
}  // namespace

extern "C" int jpegr_stream_decode_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                          size_t tile0, size_t ntile, void *d_coef,
                                          void *d_scratch, void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_in || !d_coef || !d_scratch || !d_result || ntiles == 0 || ntile == 0 ||
      tile0 > ntiles || ntile > ntiles - tile0 || misaligned(d_coef, 15) || misaligned(d_result, 7) ||
      misaligned(d_scratch, 15))
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch s = scratch_of(d_scratch, ntiles);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *result = static_cast<uint64_t *>(d_result);
  sizes_and_scan<true>(in, in_len, ntiles, w, h, nimg, s, result, st);
  launch_chunks(ntile, kLanes, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_decode, dim3(n), dim3(2 * kLanes), 0, st, in, (uint64_t)in_len, ntiles, tile0,
                       ntile, b, s.tsz, s.gsum, s.part, result, static_cast<int16_t *>(d_coef));
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

extern "C" int jpegr_stream_index_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                         void *d_tile_offsets, void *d_scratch, void *d_result,
                                         void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_in || !d_tile_offsets || !d_scratch || !d_result || ntiles == 0 || misaligned(d_tile_offsets, 7) ||
      misaligned(d_result, 7) || misaligned(d_scratch, 15))
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch s = scratch_of(d_scratch, ntiles);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *result = static_cast<uint64_t *>(d_result);
  sizes_and_scan<false>(in, in_len, ntiles, w, h, nimg, s, result, st);
  launch_chunks(ntiles, kGT, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_index_finish, dim3(n), dim3(kGT), 0, st, s.tsz, s.gsum, s.part, ntiles, b,
                       (uint64_t)in_len, result, static_cast<uint64_t *>(d_tile_offsets));
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

extern "C" size_t jpegr_crop_items(int max_w, int max_h) {
  if (max_w <= 0 || max_h <= 0) return 0;
  return (size_t)jpegr_crop::crop_span((uint32_t)max_w) * jpegr_crop::crop_span((uint32_t)max_h);
}

// [256 B x K x nrects of coefficients][u32 status x nrects], whole 16-B chunks
extern "C" size_t jpegr_crop_scratch_bytes(size_t nrects, int max_w, int max_h) {
  const size_t K = jpegr_crop_items(max_w, max_h);
  if (nrects == 0 || K == 0 || K > SIZE_MAX / 512 || nrects > (SIZE_MAX - 15) / (256 * K + 4)) return 0;
  return (nrects * (256 * K + 4) + 15) & ~(size_t)15;
}

extern "C" int jpegr_crop_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                 const void *d_tile_offsets, const void *d_rects, size_t nrects,
                                 int max_w, int max_h, void *d_out, size_t out_cap,
                                 void *d_scratch, void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  const size_t K = jpegr_crop_items(max_w, max_h);
  if (!d_in || !d_tile_offsets || !d_rects || !d_out || !d_scratch || !d_result || ntiles == 0 ||
      nrects == 0 || K == 0 || max_w > w || max_h > h || in_len < (size_t)kHdr || misaligned(d_rects, 7) ||
      misaligned(d_tile_offsets, 7) || misaligned(d_result, 7) || misaligned(d_scratch, 15) ||
      misaligned(d_out, 3) ||
      nrects > kMaxWg * kLanes / K)                   // one launch_chunks pass: 2^28 items
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *rects = static_cast<const jpegr_rect *>(d_rects);
  auto *result = static_cast<uint64_t *>(d_result);
  auto *coef = static_cast<int16_t *>(d_scratch);
  auto *status = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_scratch) + nrects * K * 256);
  launch_chunks(nrects, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_crop_init, dim3(n), dim3(256), 0, st, in, (uint64_t)in_len, ntiles,
                       (uint32_t)w, (uint32_t)h, (uint32_t)nimg, rects, nrects, b * 256,
                       (uint32_t)max_w, (uint32_t)max_h, (uint64_t)out_cap, status, result);
  });
  launch_chunks(nrects * K, kLanes, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_crop_decode, dim3(n), dim3(2 * kLanes), 0, st, in, (uint64_t)in_len,
                       (uint32_t)((w + 7) / 8), (uint32_t)((h + 7) / 8),
                       static_cast<const uint64_t *>(d_tile_offsets), rects, nrects, (uint32_t)K, b,
                       status, result, coef);
  });
  return jpegr_crop_recon_launch(coef, status, rects, nrects, max_w, max_h,
                                 static_cast<uint8_t *>(d_out), result, st);
}

extern "C" int jpegr_crop_tensor_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                        const void *d_tile_offsets, const void *d_rects,
                                        size_t nrects, const void *d_flip, int max_w, int max_h,
                                        int dtype, int layout, const float *scale3,
                                        const float *bias3, void *d_out, size_t out_cap,
                                        void *d_scratch, void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  const size_t K = jpegr_crop_items(max_w, max_h);
  if (!d_in || !d_tile_offsets || !d_rects || !d_out || !d_scratch || !d_result || ntiles == 0 ||
      nrects == 0 || K == 0 || max_w > w || max_h > h || in_len < (size_t)kHdr || misaligned(d_rects, 7) ||
      misaligned(d_tile_offsets, 7) || misaligned(d_result, 7) || misaligned(d_scratch, 15) ||
      misaligned(d_out, 15) || dtype < JPEGR_DTYPE_U8 || dtype > JPEGR_DTYPE_BF16 ||
      (layout != JPEGR_LAYOUT_CHW && layout != JPEGR_LAYOUT_HWC) ||
      nrects > kMaxWg * kLanes / K)                   // one launch_chunks pass: 2^28 items
    return JPEGR_ERR_ARG;
  for (int c = 0; c < 3; ++c)
    if ((scale3 && !isfinite(scale3[c])) || (bias3 && !isfinite(bias3[c]))) return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *rects = static_cast<const jpegr_rect *>(d_rects);
  auto *result = static_cast<uint64_t *>(d_result);
  auto *coef = static_cast<int16_t *>(d_scratch);
  auto *status = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_scratch) + nrects * K * 256);
  launch_chunks(nrects, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_crop_tensor_init, dim3(n), dim3(256), 0, st, in, (uint64_t)in_len, ntiles,
                       (uint32_t)w, (uint32_t)h, (uint32_t)nimg, rects, nrects, b * 256,
                       (uint32_t)max_w, (uint32_t)max_h, (uint64_t)out_cap, status, result);
  });
  launch_chunks(nrects * K, kLanes, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_crop_decode, dim3(n), dim3(2 * kLanes), 0, st, in, (uint64_t)in_len,
                       (uint32_t)((w + 7) / 8), (uint32_t)((h + 7) / 8),
                       static_cast<const uint64_t *>(d_tile_offsets), rects, nrects, (uint32_t)K, b,
                       status, result, coef);
  });
  return jpegr_crop_tensor_launch(coef, status, rects, nrects, max_w, max_h,
                                  static_cast<const uint8_t *>(d_flip), dtype, layout, scale3, bias3,
                                  d_out, result, st);
}

extern "C" int jpegr_crop_resize_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                        const void *d_tile_offsets, const void *d_rects,
                                        size_t nrects, const void *d_flip, int max_w, int max_h,
                                        int out_w, int out_h, int filter, int dtype, int layout,
                                        const float *scale3, const float *bias3, void *d_out,
                                        size_t out_cap, void *d_scratch, void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  const size_t K = jpegr_crop_items(max_w, max_h);
  if (!d_in || !d_tile_offsets || !d_rects || !d_out || !d_scratch || !d_result || ntiles == 0 ||
      nrects == 0 || K == 0 || max_w > w || max_h > h || in_len < (size_t)kHdr || misaligned(d_rects, 7) ||
      misaligned(d_tile_offsets, 7) || misaligned(d_result, 7) || misaligned(d_scratch, 15) ||
      misaligned(d_out, 15) || dtype < JPEGR_DTYPE_U8 || dtype > JPEGR_DTYPE_BF16 ||
      (layout != JPEGR_LAYOUT_CHW && layout != JPEGR_LAYOUT_HWC) ||
      (filter != JPEGR_FILTER_BILINEAR && filter != JPEGR_FILTER_TRIANGLE) || out_w <= 0 || out_h <= 0 ||
      (long long)out_w * out_h > 0x7fffffffll / 3 ||  // a rectangle's 3 out_w out_h elements fit an int
      nrects > kMaxWg * kLanes / K)                   // one launch_chunks pass: 2^28 items
    return JPEGR_ERR_ARG;
  for (int c = 0; c < 3; ++c)
    if ((scale3 && !isfinite(scale3[c])) || (bias3 && !isfinite(bias3[c]))) return JPEGR_ERR_ARG;
  jpegr_resize::Layout L;
  if (!jpegr_resize::layout_of(nrects, max_w, max_h, out_w, out_h, L)) return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto *in = static_cast<const uint8_t *>(d_in);
  auto *rects = static_cast<const jpegr_rect *>(d_rects);
  auto *result = static_cast<uint64_t *>(d_result);
  auto *base = static_cast<uint8_t *>(d_scratch);
  auto *coef = static_cast<int16_t *>(d_scratch);
  auto *status = reinterpret_cast<uint32_t *>(base + L.status);
  auto *shadow = reinterpret_cast<const jpegr_rect *>(base + L.shadow);
  jpegr_resize_init_launch(in, in_len, ntiles, w, h, nimg, rects, nrects, max_w, max_h, out_w, out_h,
                           out_cap, L, d_scratch, result, st);
  launch_chunks(nrects * K, kLanes, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_crop_decode, dim3(n), dim3(2 * kLanes), 0, st, in, (uint64_t)in_len,
                       (uint32_t)((w + 7) / 8), (uint32_t)((h + 7) / 8),
                       static_cast<const uint64_t *>(d_tile_offsets), shadow, nrects, (uint32_t)K, b,
                       status, result, coef);
  });
  if (jpegr_crop_recon_launch(coef, status, shadow, nrects, max_w, max_h, base + L.pix, result, st) !=
      JPEGR_OK)
    return JPEGR_ERR_HIP;
  return jpegr_resize_launch(L, d_scratch, rects, nrects, out_w, out_h, filter,
                             static_cast<const uint8_t *>(d_flip), dtype, layout, scale3, bias3, d_out, st);
}

// ---- the dataset calls ------------------------------------------------

extern "C" size_t jpegr_dataset_crop_scratch_bytes(size_t nrects, int max_w, int max_h) {
  return jpegr_dataset::scratch_with_words(jpegr_crop_scratch_bytes(nrects, max_w, max_h), nrects);
}

// what both dataset calls reject of the table, before any HIP call
static bool bad_table(const void *d_streams, size_t nstreams) {
  return !d_streams || nstreams == 0 || nstreams > jpegr_dataset::kMaxStreams || misaligned(d_streams, 7);
}

// the dataset calls' second launch: jprs_crop_decode's items over `rects`
static void dataset_decode_launch(const jpegr_stream_desc *ds, const uint64_t *where, const jpegr_rect *rects,
                                  size_t nrects, size_t K, uint32_t *status, uint64_t *result,
                                  int16_t *coef, hipStream_t st) {
  launch_chunks(nrects * K, kLanes, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_dataset_crop_decode, dim3(n), dim3(2 * kLanes), 0, st, ds, where, rects, nrects,
                       (uint32_t)K, b, status, result, coef);
  });
}

extern "C" int jpegr_dataset_crop_tensor_device(const void *d_streams, size_t nstreams,
                                                const void *d_rects, size_t nrects, const void *d_flip,
                                                int max_w, int max_h, int dtype, int layout,
                                                const float *scale3, const float *bias3, void *d_out,
                                                size_t out_cap, void *d_scratch, void *d_result,
                                                void *stream) {
  const size_t K = jpegr_crop_items(max_w, max_h);
  if (bad_table(d_streams, nstreams) || !d_rects || !d_out || !d_scratch || !d_result || nrects == 0 ||
      K == 0 || misaligned(d_rects, 7) || misaligned(d_result, 7) || misaligned(d_scratch, 15) ||
      misaligned(d_out, 15) || dtype < JPEGR_DTYPE_U8 || dtype > JPEGR_DTYPE_BF16 ||
      (layout != JPEGR_LAYOUT_CHW && layout != JPEGR_LAYOUT_HWC) ||
      nrects > kMaxWg * kLanes / K)                   // one launch_chunks pass: 2^28 items
    return JPEGR_ERR_ARG;
  for (int c = 0; c < 3; ++c)
    if ((scale3 && !isfinite(scale3[c])) || (bias3 && !isfinite(bias3[c]))) return JPEGR_ERR_ARG;
  const size_t crop = jpegr_crop_scratch_bytes(nrects, max_w, max_h);
  if (jpegr_dataset::scratch_with_words(crop, nrects) == 0) return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto *ds = static_cast<const jpegr_stream_desc *>(d_streams);
  auto *rects = static_cast<const jpegr_rect *>(d_rects);
  auto *result = static_cast<uint64_t *>(d_result);
  auto *base = static_cast<uint8_t *>(d_scratch);
  auto *coef = static_cast<int16_t *>(d_scratch);
  auto *status = reinterpret_cast<uint32_t *>(base + nrects * K * 256);
  auto *where = reinterpret_cast<uint64_t *>(base + crop);
  launch_chunks(nrects, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_dataset_crop_tensor_init, dim3(n), dim3(256), 0, st, ds, (uint64_t)nstreams,
                       rects, nrects, b * 256, (uint32_t)max_w, (uint32_t)max_h, (uint64_t)out_cap, status,
                       where, result);
  });
  dataset_decode_launch(ds, where, rects, nrects, K, status, result, coef, st);
  return jpegr_crop_tensor_launch(coef, status, rects, nrects, max_w, max_h,
                                  static_cast<const uint8_t *>(d_flip), dtype, layout, scale3, bias3,
                                  d_out, result, st);
}

extern "C" int jpegr_dataset_crop_resize_device(const void *d_streams, size_t nstreams,
                                                const void *d_rects, size_t nrects, const void *d_flip,
                                                int max_w, int max_h, int out_w, int out_h, int filter,
                                                int dtype, int layout, const float *scale3,
                                                const float *bias3, void *d_out, size_t out_cap,
                                                void *d_scratch, void *d_result, void *stream) {
  const size_t K = jpegr_crop_items(max_w, max_h);
  if (bad_table(d_streams, nstreams) || !d_rects || !d_out || !d_scratch || !d_result || nrects == 0 ||
      K == 0 || misaligned(d_rects, 7) || misaligned(d_result, 7) || misaligned(d_scratch, 15) ||
      misaligned(d_out, 15) || dtype < JPEGR_DTYPE_U8 || dtype > JPEGR_DTYPE_BF16 ||
      (layout != JPEGR_LAYOUT_CHW && layout != JPEGR_LAYOUT_HWC) ||
      (filter != JPEGR_FILTER_BILINEAR && filter != JPEGR_FILTER_TRIANGLE) || out_w <= 0 || out_h <= 0 ||
      (long long)out_w * out_h > 0x7fffffffll / 3 ||  // a rectangle's 3 out_w out_h elements fit an int
      nrects > kMaxWg * kLanes / K)                   // one launch_chunks pass: 2^28 items
    return JPEGR_ERR_ARG;
  for (int c = 0; c < 3; ++c)
    if ((scale3 && !isfinite(scale3[c])) || (bias3 && !isfinite(bias3[c]))) return JPEGR_ERR_ARG;
  jpegr_resize::Layout L;
  if (!jpegr_resize::layout_of(nrects, max_w, max_h, out_w, out_h, L) ||
      jpegr_dataset::scratch_with_words(L.bytes, nrects) == 0)
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto *ds = static_cast<const jpegr_stream_desc *>(d_streams);
  auto *rects = static_cast<const jpegr_rect *>(d_rects);
  auto *result = static_cast<uint64_t *>(d_result);
  auto *base = static_cast<uint8_t *>(d_scratch);
  auto *coef = static_cast<int16_t *>(d_scratch);
  auto *status = reinterpret_cast<uint32_t *>(base + L.status);
  auto *shadow = reinterpret_cast<const jpegr_rect *>(base + L.shadow);
  auto *where = reinterpret_cast<const uint64_t *>(base + L.bytes);
  jpegr_dataset_resize_init_launch(ds, nstreams, rects, nrects, max_w, max_h, out_w, out_h, out_cap, L,
                                   d_scratch, result, st);
  dataset_decode_launch(ds, where, shadow, nrects, K, status, result, coef, st);
  if (jpegr_crop_recon_launch(coef, status, shadow, nrects, max_w, max_h, base + L.pix, result, st) !=
      JPEGR_OK)
    return JPEGR_ERR_HIP;
  return jpegr_resize_launch(L, d_scratch, rects, nrects, out_w, out_h, filter,
                             static_cast<const uint8_t *>(d_flip), dtype, layout, scale3, bias3, d_out, st);
}
