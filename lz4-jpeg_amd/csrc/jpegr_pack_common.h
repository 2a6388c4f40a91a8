// jpegr_pack_common.h -- the JPR stream's format (include/jpegr.h), once, for
// every reader and writer of it: the record bounds and the slots' fields, the
// stream header word and the JPT1 table coding, the index and the 16-B header
// (written and read), the readers' sizes launch (jprs_sizes), the rule that
// makes a record malformed, the writers' run
// of 16 tiles and its LDS image's way out to the stream, the scratch layout of
// jpegr_pack_scratch_bytes, the index scan (lz4r_scan.h as it is) and a
// workgroup's finish of that scan.  All of it is inlined into its callers; what
// that does to each kernel's code and time: profiles/jpr_writers_refactor.md.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/jpegr.h"
#include "lz4r_scan.h"

namespace {

constexpr int kRecMax = 1036;               // 516 + 260 + 260
constexpr int kHdr = 16;
constexpr uint32_t kMagicJPR1 = 0x3152504Au;   // "JPR1"
constexpr uint32_t kMagicJPT1 = 0x3154504Au;   // "JPT1"

// slot bounds of channel c (0 Y, 1 Cr, 2 Cb): table entries = RLE ints, bits
__device__ __forceinline__ uint32_t slot_codes(int c) { return c ? 64u : 128u; }
__device__ __forceinline__ uint32_t slot_bits(int c) { return c ? 512u : 1024u; }
// a channel's first byte of the bits slot, first entry of the table slot
__device__ __forceinline__ uint32_t slot_off(int c) { return c == 0 ? 0u : c == 1 ? 128u : 192u; }

// what a writer copies of a stream: its codes and bit bytes, clamped to the slot
// (a meta word past its slot cannot make any kernel here leave the slot)
__device__ __forceinline__ uint32_t meta_codes(uint32_t m, int c) { return min(m >> 24, slot_codes(c)); }
__device__ __forceinline__ uint32_t meta_bits(uint32_t m, int c) { return min(m & 0xFFFFu, slot_bits(c)); }

// table bytes of n entries in JPT1 mode md (mode 0: JPR1's 3-B entries)
__device__ __forceinline__ uint32_t table_bytes(uint32_t n, uint32_t md) {
  return md == 0 ? 3u * n : ((n + 1u) >> 1) + md * n;
}
// a stream's bytes in a record: header, table in mode md, bit bytes (JPR1: md = 0)
__device__ __forceinline__ uint32_t stream_bytes(uint32_t m, int c, uint32_t md) {
  return 4u + table_bytes(meta_codes(m, c), md) + ((meta_bits(m, c) + 7u) >> 3);
}
// a stream's header: u8 rle_len | u8 ncodes | u16 nbits, the mode in its top two bits
__device__ __forceinline__ uint32_t stream_header(uint32_t rle, uint32_t ncodes, uint32_t nbits,
                                                  uint32_t md) {
  return rle | ncodes << 8 | (nbits | md << 14) << 16;
}

// a table word's disqualifiers: a length past a nibble, a value past an i8
// (a word that is not a live entry, 0, disqualifies nothing)
__device__ __forceinline__ bool long_len(uint32_t e) { return ((e >> 16) & 255u) > 15u; }
__device__ __forceinline__ bool wide_val(uint32_t e) { return (int16_t)e != (int8_t)e; }
// the writers' canonical JPT1 mode of a table of ncodes entries
__device__ __forceinline__ uint32_t table_mode(uint32_t ncodes, bool any_long, bool any_wide) {
  return (ncodes == 0 || any_long) ? 0u : any_wide ? 2u : 1u;
}

// ---- index and header ---------------------------------------------------------

// tile t's u16 index entry, nothing at or past cap
__device__ __forceinline__ void put_index(uint8_t *out, uint64_t cap, size_t t,
                                          uint32_t sz) {
  const uint64_t pos = kHdr + 2 * (uint64_t)t;          // 2-B aligned: out is 16-B aligned
  if (pos + 2 <= cap)
    *reinterpret_cast<uint16_t *>(out + pos) = (uint16_t)sz;
  else if (pos < cap)
    out[pos] = (uint8_t)sz;
}

__device__ __forceinline__ void put_header(uint8_t *out, uint64_t cap, uint32_t magic,
                                           uint32_t w, uint32_t h, uint32_t nimg) {
  const uint32_t hw[4] = {magic, w, h, nimg};
  for (uint32_t i = 0; i < (uint32_t)kHdr && i < cap; ++i) out[i] = (uint8_t)(hw[i >> 2] >> (8 * (i & 3)));
}

// tile t's index entry, 0 for a byte at or past in_len
__device__ __forceinline__ uint32_t get_index(const uint8_t *in, uint64_t in_len, size_t t) {
  const uint64_t pos = kHdr + 2 * (uint64_t)t;
  const uint32_t lo = pos < in_len ? in[pos] : 0u, hi = pos + 1 < in_len ? in[pos + 1] : 0u;
  return lo | hi << 8;
}

// the stream holds its header and index, and the header is these dimensions'
// ("JPR1", or "JPT1" too where the reader takes it)
__device__ __forceinline__ bool header_ok(const uint8_t *in, uint64_t in_len, size_t ntiles, uint32_t w,
                                          uint32_t h, uint32_t nimg, bool accept_tight) {
  const uint32_t want[4] = {kMagicJPR1, w, h, nimg};
  bool ok = in_len >= kHdr + 2 * (uint64_t)ntiles;
  for (uint32_t i = 0; ok && i < (uint32_t)kHdr; ++i)
    ok = in[i] == (uint8_t)(want[i >> 2] >> (8 * (i & 3))) || (accept_tight && i == 2 && in[i] == 'T');
  return ok;
}

// The first launch of a call that reads a stream by its own index (the direct
// decode, the index call, the thumbnails): index -> u32 sizes, the scan's input,
// and the header verdict in result[1].  kThird: the call's result has a third
// word, cleared here (the index call has two words).
template <bool kThird>
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
    if constexpr (kThird) result[2] = 0ull;
  }
}

// ---- the record rule ----------------------------------------------------------

// A record of `size` bytes whose byte x is rd(off + x): the three stream
// headers against the slots' bounds and the indexed size.  An index entry over
// 1,036 B is malformed by itself; in a JPT1 record the table's bytes follow
// from the mode in the top two bits of the u16, and mode 3 is malformed.  A
// header is read only once it is known to lie inside the record.  Returns
// whether the record is well-formed; so[c] = off + stream c's offset in the
// record and m[c] = its meta word for every stream whose header was read, md
// the modes as Y | Cr << 2 | Cb << 4.  (The loop is spelled as jprs_decode had
// it: in this form that kernel, the hotter reader, keeps its instructions.)
template <bool kTight, typename Rd, typename So>
__device__ __forceinline__ bool record_rule(Rd rd, uint32_t off, uint32_t size, So so, uint32_t (&m)[3],
                                            uint32_t &md) {
  bool ok = size <= (uint32_t)kRecMax;
  uint32_t p = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ok = ok && p + 4 <= size;
    if (ok) {
      const uint32_t rle = rd(off + p), nc = rd(off + p + 1);
      uint32_t nb = rd(off + p + 2) | rd(off + p + 3) << 8;
      uint32_t tbytes = 3u * nc;
      if constexpr (kTight) {
        const uint32_t mode = nb >> 14;
        nb &= 0x3FFFu;
        ok = mode != 3u;
        if (mode) tbytes = table_bytes(nc, mode);
        md |= mode << (2 * c);
      }
      ok = ok && rle <= slot_codes(c) && nc <= slot_codes(c) && nb <= slot_bits(c);
      so[c] = off + p;
      m[c] = nb | rle << 16 | nc << 24;
      p += 4u + tbytes + ((nb + 7u) >> 3);
    }
  }
  return ok && p == size;
}

// ---- the scan's finish ----------------------------------------------------------

// Wave 0: the stream offsets of scan group g's 64 tiles into toff[0..64]
// (lz4_emit's finish of the scan: partial + earlier group sums + a wave scan).
__device__ __forceinline__ void group_offsets(const int tid, const size_t g, const size_t ntiles,
                                              const uint32_t *__restrict__ tsz,
                                              const uint32_t *__restrict__ gsum,
                                              const uint64_t *__restrict__ part, uint64_t *toff) {
  if (tid >= 64) return;
  const size_t g0 = g * kGT;
  const int nt = (int)min((size_t)kGT, ntiles - g0);
  const size_t p = g0 / kPart, gfirst = p * 64;
  const uint32_t gs = (gfirst + tid < g) ? gsum[gfirst + tid] : 0u;
  const uint64_t pt = part[p];
  const uint32_t tv = tid < nt ? tsz[g0 + tid] : 0u;
  // < 2^32: at most 4,096 tiles of at most 65,535 B before g in its partial
  const uint64_t base = pt + lane63(wave_incl_add(gs));
  const uint32_t inc = wave_incl_add(tv);
  toff[tid] = base + inc - tv;
  if (tid == 63) toff[kGT] = base + inc;
}

// ---- the run --------------------------------------------------------------------

// tiles per workgroup of the emit, place and unpack kernels (a quarter of a
// scan group).  The LDS image is sized for the worst case, 1,036 B a tile, so
// the run sets the occupancy: 16 tiles (16.6 KB, 8 workgroups per CU) pack a 4K
// image in 0.035 ms, 32 tiles in 0.051 ms, 8 tiles in 0.043 ms
constexpr int kRun = 16;
constexpr int kSplit = kGT / kRun;          // workgroups per scan group
constexpr int kPW = 4;                      // waves per workgroup
constexpr int kTW = kRun / kPW;             // tiles per wave
constexpr int kImg = kRun * kRecMax + 16;   // the range + its lead inside a 16-B chunk
static_assert(kGT % kRun == 0 && kRun % kPW == 0 && kImg % 16 == 0, "whole workgroups per scan group");

// workgroup wg's run: tiles t0 .. t0 + ntl - 1, which are tiles h0 .. of scan
// group g; t0 >= ntiles: none, and ntl means nothing
struct Run {
  size_t g, t0;
  int h0, ntl;
};

__device__ __forceinline__ Run run_of(size_t wg, size_t ntiles) {
  Run r;
  r.g = wg / kSplit;
  r.h0 = (int)(wg % kSplit) * kRun;
  r.t0 = r.g * kGT + r.h0;
  r.ntl = (int)min((size_t)kRun, ntiles - r.t0);
  return r;
}

// The LDS image -> the stream's bytes [G0, G1), img[lead] being byte G0 and
// lead = (out + G0) & 15: aligned 16-B stores; the first and last partial
// chunks, which neighbouring workgroups share, a byte per lane; nothing at or
// past cap.  All of the workgroup's 64 kPW threads, after the barrier behind
// the image's last write; lane and wv are the caller's own tid & 63, tid >> 6.
__device__ __forceinline__ void image_out(const uint8_t *img, int tid, int lane, int wv, uint64_t G0,
                                          uint64_t G1, uint32_t lead, uint8_t *out,
                                          uint64_t cap) {
  const uint64_t E = min(G1, cap);
  if (E > G0) {
    uint8_t *const outF = out + (G0 - lead);            // 16-B aligned
    const uint32_t nrel = (uint32_t)(E - G0) + lead;
    const uint32_t c0 = lead ? 1u : 0u, c1 = nrel >> 4; // the whole chunks: [c0, c1)
    for (uint32_t ci = c0 + (uint32_t)tid; ci < c1; ci += 64 * kPW)
      __builtin_nontemporal_store(reinterpret_cast<const u32x4 *>(img)[ci],
                                  reinterpret_cast<u32x4 *>(outF + 16u * ci));
    if (wv == kPW - 1 && lane < 32) {
      const uint32_t x = lane < 16 ? (uint32_t)lane : 16u * c1 + (uint32_t)(lane - 16);
      const bool own = lane < 16 ? (c0 && x >= lead && x < nrel) : (c1 >= c0 && x < nrel);
      if (own) outF[x] = img[x];
    }
  }
}

// ---- host -------------------------------------------------------------------------

// tiles of nimg w x h images, 0 when a dimension is not positive or the
// count passes 2^32
inline size_t tiles_of(int w, int h, int nimg) {
  if (w <= 0 || h <= 0 || nimg <= 0) return 0;
  const uint64_t per = (uint64_t)(((int64_t)w + 7) / 8) * (uint64_t)(((int64_t)h + 7) / 8);
  if (per > (1ull << 32) || per * (uint64_t)nimg > (1ull << 32)) return 0;
  return (size_t)(per * (uint64_t)nimg);
}

// a stream's 16-B header on the host: its format (JPEGR_STREAM_*) and
// dimensions, 0 when it is not a stream's
inline int parse_header(const uint8_t header[16], int *w, int *h, int *nimg) {
  if (header[0] != 'J' || header[1] != 'P' || (header[2] != 'R' && header[2] != 'T') ||
      header[3] != '1')
    return 0;
  uint32_t v[3];
  for (int i = 0; i < 3; ++i)
    v[i] = (uint32_t)header[4 + 4 * i] | (uint32_t)header[5 + 4 * i] << 8 |
           (uint32_t)header[6 + 4 * i] << 16 | (uint32_t)header[7 + 4 * i] << 24;
  if (v[0] == 0 || v[1] == 0 || v[2] == 0 || v[0] > 0x7FFFFFFFu || v[1] > 0x7FFFFFFFu ||
      v[2] > 0x7FFFFFFFu)
    return 0;
  *w = (int)v[0];
  *h = (int)v[1];
  *nimg = (int)v[2];
  return header[2] == 'R' ? JPEGR_STREAM_JPR1 : JPEGR_STREAM_JPT1;
}

// scratch: [partials u64][tile sizes u32, padded to 4][group sums u32]
struct Scratch {
  uint64_t *part;
  uint32_t *tsz, *gsum;
  size_t nparts, bytes;
};

inline Scratch scratch_of(void *base, size_t ntiles) {
  Scratch s;
  s.nparts = (ntiles + kPart - 1) / kPart;
  const size_t ngroups = (ntiles + kGT - 1) / kGT;
  const size_t part_b = (s.nparts * 8 + 15) & ~(size_t)15;
  const size_t tsz_b = ((ntiles + 3) & ~(size_t)3) * 4;
  auto *p = static_cast<uint8_t *>(base);
  s.part = reinterpret_cast<uint64_t *>(p);
  s.tsz = reinterpret_cast<uint32_t *>(p + part_b);
  s.gsum = reinterpret_cast<uint32_t *>(p + part_b + tsz_b);
  s.bytes = part_b + tsz_b + ngroups * 4;
  return s;
}

// HIP's grid limit is 2^32 work-items: launches of at most 2^22 workgroups.
// launch(first workgroup, workgroups) for each chunk of `count` things at
// `per` a workgroup.
constexpr size_t kMaxWg = (size_t)1 << 22;

template <typename F>
inline void launch_chunks(size_t count, size_t per, F launch) {
  const size_t nwg = (count + per - 1) / per;
  for (size_t b = 0; b < nwg; b += kMaxWg) launch(b, (unsigned)std::min(kMaxWg, nwg - b));
}

inline void scan(const Scratch &s, size_t ntiles, uint64_t *len, hipStream_t st) {
  hipLaunchKernelGGL(lz4_scan_reduce, dim3((unsigned)s.nparts), dim3(256), 0, st, s.tsz, ntiles,
                     (size_t)0, s.gsum, s.part);
  hipLaunchKernelGGL(lz4_scan_partials, dim3(1), dim3(1024), 0, st, s.part, s.nparts,
                     (uint64_t)kHdr + 2 * (uint64_t)ntiles, 1, 0, (uint32_t *)nullptr, len,
                     (uint64_t *)nullptr);
}

}  // namespace
