// jpegr_pack_common.h -- the JPR stream's format (include/jpegr.h), once, for
// every reader and writer of it: the record bounds and the slots' fields, the
// stream header word and the JPT1 table coding (table_bytes, bits_at; written by
// put_stream_headers, put_table_word, tile_modes), the index and the 16-B header,
// the readers' first launches (jprs_sizes, sizes_and_scan), the rules for a
// record (record_rule) and for a caller's offsets (record_at), a range decode's
// report (RangeReport), the writers' run of 16 tiles and its LDS image's way out,
// the scratch layout, the index scan (lz4r_scan.h as it is) and its finish by a
// workgroup (group_offsets) or a wave (scan_record).  The readers' pieces are
// here, not in a header of their own: each is a few lines on what stands above
// it.  All of it is inlined; what that does to each kernel's code and time:
// profiles/jpr_writers_refactor.md, profiles/stream_readers_refactor.md.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/jpegr.h"
#include "lz4r_scan.h"

namespace {

constexpr int kRecMax = 1036;               // 516 + 260 + 260
constexpr uint32_t kEmptyRec = 12;          // three streams with ncodes = 0, all bytes 0
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

// a stream's first bit byte, its header at offset so: behind its n entries in mode md
__device__ __forceinline__ uint32_t bits_at(uint32_t so, uint32_t n, uint32_t md) {
  return so + 4u + table_bytes(n, md);
}

// a table word's disqualifiers: a length past a nibble, a value past an i8
// (a word that is not a live entry, 0, disqualifies nothing)
__device__ __forceinline__ bool long_len(uint32_t e) { return ((e >> 16) & 255u) > 15u; }
__device__ __forceinline__ bool wide_val(uint32_t e) { return (int16_t)e != (int8_t)e; }
// the writers' canonical JPT1 mode of a table of ncodes entries
__device__ __forceinline__ uint32_t table_mode(uint32_t ncodes, bool any_long, bool any_wide) {
  return (ncodes == 0 || any_long) ? 0u : any_wide ? 2u : 1u;
}

// ---- a tile's table on a wave: word k of a stream on lane k ------------------------

// A wave holds a tile's table as four words a lane (value | length << 16; 0 where
// not live): Y entries lane and 64 + lane, Cr, Cb.  Word q's channel and entry:
__device__ __forceinline__ int word_chan(int q) { return q < 2 ? 0 : q - 1; }
__device__ __forceinline__ uint32_t word_entry(int q, int lane) { return (uint32_t)lane + (q == 1 ? 64u : 0u); }

// the canonical modes of a tile's three streams (n0, n1, n2 codes) from those
// words, as Y | Cr << 2 | Cb << 4.  Wave-uniform.
__device__ __forceinline__ uint32_t tile_modes(const uint32_t (&tb)[4], uint32_t n0, uint32_t n1,
                                               uint32_t n2) {
  const bool l0 = __ballot(long_len(tb[0]) || long_len(tb[1])) != 0;
  const bool w0 = __ballot(wide_val(tb[0]) || wide_val(tb[1])) != 0;
  const bool l1 = __ballot(long_len(tb[2])) != 0, w1 = __ballot(wide_val(tb[2])) != 0;
  const bool l2 = __ballot(long_len(tb[3])) != 0, w2 = __ballot(wide_val(tb[3])) != 0;
  return table_mode(n0, l0, w0) | table_mode(n1, l1, w1) << 2 | table_mode(n2, l2, w2) << 4;
}

// a record's three stream headers at img + o[c], from the meta words m (clamped
// to the slots) and the modes md, a byte per lane
__device__ __forceinline__ void put_stream_headers(uint8_t *img, const uint32_t (&o)[3], const uint32_t (&m)[3],
                                                   const uint32_t (&md)[3], int lane) {
  if (lane < 12) {
    const int c = lane >> 2;
    const uint32_t mc = c == 0 ? m[0] : c == 1 ? m[1] : m[2];
    const uint32_t oc = c == 0 ? o[0] : c == 1 ? o[1] : o[2];
    const uint32_t dc = c == 0 ? md[0] : c == 1 ? md[1] : md[2];
    const uint32_t hw = stream_header((mc >> 16) & 255u, meta_codes(mc, c), meta_bits(mc, c), dc);
    img[oc + (lane & 3)] = (uint8_t)(hw >> (8 * (lane & 3)));
  }
}

// This lane's word e, entry k of a table of nc in mode md, to the table at p (a
// stream's byte 4).  A length byte's pair (2 j, 2 j + 1) is on neighbouring lanes
// of one register: lane 2 j takes lane 2 j + 1's word (not live: 0).  A whole wave.
__device__ __forceinline__ void put_table_word(uint8_t *p, uint32_t nc, uint32_t md, uint32_t k, uint32_t e) {
  const uint32_t up = __shfl_down(e, 1);                // lane + 1's word, by every lane of the wave
  if (k < nc) {
    if (md == 0) {                                      // i16 value, u8 code length
      p += 3u * k;
      p[0] = (uint8_t)e;
      p[1] = (uint8_t)(e >> 8);
      p[2] = (uint8_t)(e >> 16);
    } else {
      if ((k & 1u) == 0) p[k >> 1] = (uint8_t)(((e >> 16) & 15u) | ((up >> 16) & 15u) << 4);
      p += (nc + 1u) >> 1;
      if (md == 1) {
        p[k] = (uint8_t)e;
      } else {
        p[2u * k] = (uint8_t)e;
        p[2u * k + 1] = (uint8_t)(e >> 8);
      }
    }
  }
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

// Tile t's record by a caller's offsets (ntiles + 1 of them, t < ntiles), which
// are not trusted: off[t] <= off[t + 1] <= in_len and a record's size, before a
// byte of it is read.  o0, size: the record, left as they are on a false.
__device__ __forceinline__ bool record_at(const uint64_t *__restrict__ toff, size_t t, uint64_t in_len,
                                          uint64_t &o0, uint32_t &size) {
  const uint64_t a = toff[t], b = toff[t + 1];
  if (!(a <= b && b <= in_len && b - a >= kEmptyRec && b - a <= (uint64_t)kRecMax)) return false;
  o0 = a;
  size = (uint32_t)(b - a);
  return true;
}

// How the direct decode and the thumbnails report: malformed(t), a lane whose
// record (tile t) fails the record rule, the first such tile into result[1];
// rejected(fails, lane), every lane of a wave with its rejected streams, one add
// a wave to result[2], after jprs_sizes' zero in stream order.
struct RangeReport {
  uint64_t *__restrict__ result;
  __device__ __forceinline__ void malformed(size_t t) const {
    atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 1ull + (unsigned long long)t);
  }
  __device__ __forceinline__ void rejected(uint32_t fails, int lane) const {
    const uint32_t f = wave_rejected(fails);
    if (f && lane == __builtin_ctzll(__ballot(1)))
      atomicAdd(reinterpret_cast<unsigned long long *>(result + 2), (unsigned long long)f);
  }
};

// ---- the scan's finish ----------------------------------------------------------

// A lane's record as the scan gives it: size, and base (the bytes before the
// wave's first tile) and inc (the wave's sizes up to and with the lane's own).
// The caller forms the offset where it uses it: summed inside scan_record,
// ahead of jprs_decode's exit of its idle lanes, that kernel had 24 instructions more.
struct ScanRec {
  uint64_t base;
  uint32_t inc, size;
  __device__ __forceinline__ uint64_t offset() const { return base + inc - size; }
};

// A wave, for itself and in registers: the record of tile a + lane, for the 64
// tiles from tile a of which the range has ntl.  The scan's partial, the group
// sums before a's group, that group's tiles before a, then a wave scan of the
// 64 sizes.  All 64 lanes are on; lanes past ntl add 0 and get size 0.
__device__ __forceinline__ ScanRec scan_record(const int lane, const size_t a, const int ntl,
                                               const uint32_t *__restrict__ tsz,
                                               const uint32_t *__restrict__ gsum,
                                               const uint64_t *__restrict__ part) {
  const size_t g = a / kGT, g0 = g * kGT;
  const int skip = (int)(a - g0);
  const size_t pi = g0 / kPart, gfirst = pi * 64;
  const uint32_t gs = (gfirst + lane < g) ? gsum[gfirst + lane] : 0u;
  const uint32_t sk = lane < skip ? tsz[g0 + lane] : 0u;
  const uint32_t size = lane < ntl ? tsz[a + lane] : 0u;
  // each sum < 2^32: at most 4,096 tiles of at most 65,535 B
  const uint64_t base = part[pi] + lane63(wave_incl_add(gs)) + lane63(wave_incl_add(sk));
  return {base, wave_incl_add(size), size};
}

// Wave 0: the stream offsets of scan group g's 64 tiles into toff[0..64]
// (lz4_emit's finish of the scan: partial + earlier group sums + a wave scan):
// scan_record without the tiles to skip, an empty scan of 16 instructions.
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

// the first launches of a call that reads a stream by its own index: jprs_sizes,
// then the scan, whose end (the length the index implies) is result[0]
template <bool kThird>
inline void sizes_and_scan(const uint8_t *in, size_t in_len, size_t ntiles, int w, int h, int nimg,
                           const Scratch &s, uint64_t *result, hipStream_t st) {
  launch_chunks(ntiles, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_sizes<kThird>, dim3(n), dim3(256), 0, st, in, (uint64_t)in_len, ntiles, b * 256,
                       (uint32_t)w, (uint32_t)h, (uint32_t)nimg, s.tsz, result);
  });
  scan(s, ntiles, result, st);
}

// an entry point's pointer test: p is not aligned to mask + 1 bytes
inline bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

}  // namespace
