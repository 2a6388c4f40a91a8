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
// The per-stream walk is a copy of jpegr_entropy.hip's decode_stream /
// decode_stream_slow, not shared with it: the source differs where the walk is
// hottest (3-B unaligned table entries, bit bytes with no slot behind them, so
// every read is bounded by the stream's own length instead of whole 16-B
// chunks), and the slot decoder keeps its code and its time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_pack_common.h"

namespace {

constexpr int kLanes = 64;
constexpr int kFastCap = 24;             // codes held in registers + LDS (luma)
constexpr int kChromaCap = 12;           // ... (chroma)

__device__ __forceinline__ int stream_len(int c) { return c == 0 ? 64 : 32; }
__device__ __forceinline__ int coef_off(int c) { return c == 0 ? 0 : c == 1 ? 64 : 96; }

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

// ---- the per-stream walk (jpegr_entropy.hip's, over a byte source) ---------------

// the decode state of one wave: see jpegr_entropy.hip's DecLds
template <int N, int Cap>
struct SDecLds {
  uint16_t vl[Cap][kLanes];                // code k: value | len << 11 (row k, the lane's u16)
  alignas(16) int16_t out[kLanes][N + 2];  // the lane's ints; rows of an odd number of dwords
  uint32_t bm[N == 64 ? 8 : 1][kLanes];    // luma: the lane's 256-bit map of code starts
};

// one lane's u16 column of a [rows][64] u16 block: entry k at byte k * 128
struct SVRow {
  typedef uint16_t __attribute__((may_alias)) HA;
  uint8_t *p;
  __device__ __forceinline__ HA &operator[](int k) const {
    return *reinterpret_cast<HA *>(p + (uint32_t)k * (2 * kLanes));
  }
};

// The number of k < Cap with h[k] > w (31-bit values): borrows of w - h[k]
// summed in two carry chains through SGPR pairs (jpegr_entropy.hip's
// count_above; each carry is read at least eight instructions after its
// write, a group of four pads with an s_nop).
template <int Cap>
__device__ __forceinline__ uint32_t scount_above(uint32_t w, const uint32_t (&h)[Cap]) {
  static_assert(Cap % 4 == 0, "groups of four");
  uint32_t a = 0, b = 0;
  if constexpr (Cap % 8 == 4) {
    uint32_t t0, t1, t2, t3;
    uint64_t c0, c1, c2, c3, d0, d1;
    asm("v_sub_co_u32_e64 %[t0], %[c0], %[w], %[h0]\n\t"
        "v_sub_co_u32_e64 %[t1], %[c1], %[w], %[h1]\n\t"
        "v_sub_co_u32_e64 %[t2], %[c2], %[w], %[h2]\n\t"
        "v_sub_co_u32_e64 %[t3], %[c3], %[w], %[h3]\n\t"
        "s_nop 1\n\t"
        "v_addc_co_u32_e64 %[a], %[d0], %[a], 0, %[c0]\n\t"
        "v_addc_co_u32_e64 %[b], %[d1], %[b], 0, %[c1]\n\t"
        "v_addc_co_u32_e64 %[a], %[d0], %[a], 0, %[c2]\n\t"
        "v_addc_co_u32_e64 %[b], %[d1], %[b], 0, %[c3]"
        : [a] "+v"(a), [b] "+v"(b), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
          [t3] "=&v"(t3), [c0] "=&s"(c0), [c1] "=&s"(c1), [c2] "=&s"(c2), [c3] "=&s"(c3),
          [d0] "=&s"(d0), [d1] "=&s"(d1)
        : [w] "v"(w), [h0] "v"(h[Cap - 4]), [h1] "v"(h[Cap - 3]), [h2] "v"(h[Cap - 2]),
          [h3] "v"(h[Cap - 1]));
  }
#pragma unroll
  for (int g = 0; g + 8 <= Cap; g += 8) {
    uint32_t t0, t1, t2, t3, t4, t5, t6, t7;
    uint64_t c0, c1, c2, c3, c4, c5, c6, c7, d0, d1;
    asm("v_sub_co_u32_e64 %[t0], %[c0], %[w], %[h0]\n\t"
        "v_sub_co_u32_e64 %[t1], %[c1], %[w], %[h1]\n\t"
        "v_sub_co_u32_e64 %[t2], %[c2], %[w], %[h2]\n\t"
        "v_sub_co_u32_e64 %[t3], %[c3], %[w], %[h3]\n\t"
        "v_sub_co_u32_e64 %[t4], %[c4], %[w], %[h4]\n\t"
        "v_sub_co_u32_e64 %[t5], %[c5], %[w], %[h5]\n\t"
        "v_sub_co_u32_e64 %[t6], %[c6], %[w], %[h6]\n\t"
        "v_sub_co_u32_e64 %[t7], %[c7], %[w], %[h7]\n\t"
        "v_addc_co_u32_e64 %[a], %[d0], %[a], 0, %[c0]\n\t"
        "v_addc_co_u32_e64 %[b], %[d1], %[b], 0, %[c1]\n\t"
        "v_addc_co_u32_e64 %[a], %[d0], %[a], 0, %[c2]\n\t"
        "v_addc_co_u32_e64 %[b], %[d1], %[b], 0, %[c3]\n\t"
        "v_addc_co_u32_e64 %[a], %[d0], %[a], 0, %[c4]\n\t"
        "v_addc_co_u32_e64 %[b], %[d1], %[b], 0, %[c5]\n\t"
        "v_addc_co_u32_e64 %[a], %[d0], %[a], 0, %[c6]\n\t"
        "v_addc_co_u32_e64 %[b], %[d1], %[b], 0, %[c7]"
        : [a] "+v"(a), [b] "+v"(b), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2),
          [t3] "=&v"(t3), [t4] "=&v"(t4), [t5] "=&v"(t5), [t6] "=&v"(t6), [t7] "=&v"(t7),
          [c0] "=&s"(c0), [c1] "=&s"(c1), [c2] "=&s"(c2), [c3] "=&s"(c3), [c4] "=&s"(c4),
          [c5] "=&s"(c5), [c6] "=&s"(c6), [c7] "=&s"(c7), [d0] "=&s"(d0), [d1] "=&s"(d1)
        : [w] "v"(w), [h0] "v"(h[g]), [h1] "v"(h[g + 1]), [h2] "v"(h[g + 2]),
          [h3] "v"(h[g + 3]), [h4] "v"(h[g + 4]), [h5] "v"(h[g + 5]), [h6] "v"(h[g + 6]),
          [h7] "v"(h[g + 7]));
  }
  return a + b;
}

// A stream's bytes in the JPR stream: sp[0..4) its header, then U table
// entries of 3 B, then nby bit bytes.  The record was checked, so all of them
// lie inside it; nothing else is read: a table index is clamped to U - 1 and
// a bit byte past nby reads sp[0] instead (in bounds, and what lies past the
// bits cannot change a decode: see lookup).
template <bool kTight>
struct StreamSrc;

template <>
struct StreamSrc<false> {
  const uint8_t *sp, *pb;
  int U, nby;
  __device__ __forceinline__ StreamSrc(const uint8_t *s, uint32_t m, uint32_t)
      : sp(s), pb(s + 4 + 3 * (m >> 24)), U((int)(m >> 24)), nby((int)(((m & 0xFFFFu) + 7u) >> 3)) {}
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
  __device__ __forceinline__ uint32_t byte(int j) const { return *(j < nby ? pb + j : sp); }
  // bit bytes j .. j + 3, the first in the top byte (MSB-first bits)
  __device__ __forceinline__ uint32_t be32(int j) const {
    return byte(j) << 24 | byte(j + 1) << 16 | byte(j + 2) << 8 | byte(j + 3);
  }
};

// A stream of a JPT1 record: its table by mode (0: JPR1's 3-B entries; 1, 2:
// ceil(U / 2) bytes of nibble lengths at sp + 4, then U values of 1 or 2 B at
// pv), then the bit bytes at pb.  The same rules: a table index is clamped to
// U - 1, so every read lies inside the stream's own checked bytes.
template <>
struct StreamSrc<true> {
  const uint8_t *sp, *pv, *pb;
  int U, nby;
  uint32_t mode;
  __device__ __forceinline__ StreamSrc(const uint8_t *s, uint32_t m, uint32_t md)
      : sp(s), U((int)(m >> 24)), nby((int)(((m & 0xFFFFu) + 7u) >> 3)), mode(md) {
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
  __device__ __forceinline__ uint32_t byte(int j) const { return *(j < nby ? pb + j : sp); }
  __device__ __forceinline__ uint32_t be32(int j) const {
    return byte(j) << 24 | byte(j + 1) << 16 | byte(j + 2) << 8 | byte(j + 3);
  }
};

// decode_stream of jpegr_entropy.hip (its comments hold there): returns 1
// (decoded), 0 (malformed) or -1 (a value or length that the u16 entries
// cannot hold, or codes that do not increase: sdecode_slow).  1 <= U <= Cap.
template <int Cap, typename Src, typename VlT>
__device__ int sdecode(const Src &S, uint32_t m, VlT vl, int16_t *__restrict__ out, int n,
                       uint32_t *bm) {
  const int nbits = (int)(m & 0xFFFF), R = (int)((m >> 16) & 255), U = (int)(m >> 24);
  if (R == 0 || R > 2 * n) return 0;
  uint32_t tb[Cap];
  S.head(tb);
  uint32_t lh[Cap];
  uint32_t code = 0, prev = 0;
  int plen = 0, lmax = 0;
  bool bad = false, wide = false;
#pragma unroll
  for (int k = 0; k < Cap; ++k) {
    lh[k] = ~0u;
    if (k < U) {
      const uint32_t e = tb[k];
      const int L = (int)((e >> 16) & 255);
      const int v = (int16_t)(e & 0xFFFF);
      bad = bad || L > 32 || (U > 1 && L == 0);
      wide = wide || L > 31 || v < -1024 || v > 1023;
      if (k) code = L >= plen ? (code + 1) << (L - plen) : (code + 1) >> (plen - L);
      plen = L;
      lmax = max(lmax, L);
      const uint32_t lc = L ? code << (32 - L) : 0;
      wide = wide || (k && lc <= prev);
      prev = lc;
      lh[k] = lc >> 1;
      vl[k] = (uint16_t)(((uint32_t)v & 0x7FFu) | ((uint32_t)L << 11));
    }
  }
  if (bad) return 0;
  if (wide) return -1;
  int idx = 0;
  auto fill = [&](int cnt, int v) {
    const int c = min(cnt, n - idx);
    out[idx] = (int16_t)v;
    for (int j = 1; j < c; ++j) {
      out[idx + j] = (int16_t)v;
      asm volatile("");
    }
    idx += max(c, 0);
  };
  auto val = [](uint32_t e) { return (int)((int32_t)(e << 21) >> 21); };
  if (U == 1) {
    const int v = val(vl[0]);
    for (int j = 0; j + 1 < R; j += 2) fill(v, v);
  } else {
    // MSB-first bit buffer: acc holds nacc valid bits, left-aligned; the next
    // 32 bits are loaded a refill ahead of their use
    uint32_t nw = S.be32(0);
    int bi = 0;
    uint64_t acc = 0;
    int nacc = 0, p = 0, got = 0;
    const uint8_t *vbase = reinterpret_cast<const uint8_t *>(&vl[Cap - 1]);
    const bool narrow = __ballot(lmax > 8) == 0;      // every code <= 8 bits
    const bool mid = __ballot(lmax > 16) == 0;        // every code <= 16 bits
    const bool use_bm = bm != nullptr && narrow;
    uint32_t pa = 0, pb = 0;
    if (use_bm) {
#pragma unroll
      for (int r = 0; r < 8; ++r) bm[r * kLanes] = 0u;
#pragma unroll
      for (int k = 0; k < Cap; ++k)
        if (k < U) {
          const uint32_t st = lh[k] >> 23;       // the code's top 8 bits
          atomicOr(&bm[(st >> 5) * kLanes], 0x80000000u >> (st & 31));
        }
      uint32_t run = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        if (r < 4) pa |= run << (8 * r);
        else pb |= run << (8 * (r - 4));
        run += __builtin_popcount(bm[r * kLanes]);
      }
    }
    auto refill = [&]() {
      if (nacc <= 32) {
        acc |= (uint64_t)nw << (32 - nacc);
        nacc += 32;
        bi += 4;
        nw = S.be32(bi);
      }
    };
    auto lookup = [&]() -> uint32_t {
      const uint32_t win = (uint32_t)(acc >> 32);
      if (use_bm) {
        const uint32_t w8 = win >> 24, j = w8 >> 5;
        const uint32_t row = bm[j * kLanes];
        const uint32_t before = __builtin_amdgcn_perm(pb, pa, j | 0x0C0C0C00u);
        const int cnt = (int)(__builtin_popcount(row >> (31 - (w8 & 31))) + before);
        return vl[cnt - 1];
      }
      const uint32_t above = scount_above<Cap>(win >> 1, lh);
      return *reinterpret_cast<const uint16_t *>(vbase - (int)(above * (2 * kLanes)));
    };
    auto take = [&](bool &bd) -> uint32_t {
      const uint32_t e = lookup();
      const int L = (int)(e >> 11);
      bd = p + L > nbits;
      bad = bad || bd;
      p = bd ? nbits : p + L;
      acc <<= L;
      nacc -= L;
      ++got;
      return e;
    };
    auto pair = [&](bool refill_each) {
      if (refill_each) refill();
      bool b0, b1;
      const uint32_t e0 = take(b0);
      if (p < nbits) {
        if (refill_each) refill();
        const uint32_t e1 = take(b1);
        if (!b1) fill(val(e0), val(e1));
      }
    };
    if (narrow) {
      while (p < nbits) {
        refill();
        pair(false);
        if (p < nbits) pair(false);
      }
    } else if (mid) {
      while (p < nbits) {
        refill();
        pair(false);
      }
    } else {
      while (p < nbits) pair(true);
    }
    if (bad || got != R) return 0;
  }
  while (idx < n) out[idx++] = 0;
  return 1;
}

// decode_stream_slow of jpegr_entropy.hip: more codes than the registers hold,
// or a table the fast walk cannot take.  The codes are regenerated from the
// stream's own table bytes for every symbol.
template <typename Src>
__device__ bool sdecode_slow(const Src &S, uint32_t m, int16_t *__restrict__ out, int n) {
  const int nbits = (int)(m & 0xFFFF), R = (int)((m >> 16) & 255), U = (int)(m >> 24);
  if (R == 0 || R > 2 * n) return false;
  int p = 0, got = 0, idx = 0, pending = 0;
  bool have = false;
  while (p < nbits) {
    const int bi = p >> 3, sh = p & 7;
    const uint32_t w0 = S.be32(bi);
    uint32_t win = sh ? (w0 << sh) | (S.byte(bi + 4) >> (8 - sh)) : w0;
    if (nbits - p < 32) win &= ~0u << (32 - (nbits - p));   // bytes past the bits are not the stream's
    uint32_t code = 0;
    int plen = 0, hit = -1, L = 0;
    for (int k = 0; k < U && hit < 0; ++k) {
      L = S.len(k);
      if (L == 0 || L > 32) return false;
      if (k) code = L >= plen ? (code + 1) << (L - plen) : (code + 1) >> (plen - L);
      plen = L;
      if ((win >> (32 - L)) == code) hit = k;
    }
    if (hit < 0 || p + L > nbits) return false;
    const int v = (int16_t)(S.entry(hit) & 0xFFFF);
    if (!have) {
      pending = v;
      have = true;
    } else {
      int cnt = pending;
      have = false;
      if (idx + cnt > n) cnt = n - idx;
      for (int j = 0; j < cnt; ++j) out[idx++] = (int16_t)v;
    }
    p += L;
    ++got;
  }
  if (got != R) return false;
  while (idx < n) out[idx++] = 0;
  return true;
}

// One wave's lanes of one channel group.  rec: the lane's record in the
// stream; so / m: its streams' offsets in the record and meta words;
// good: the record is well-formed (else its ints are 0 and nothing of it is
// read); md: the streams' table modes, Y | Cr << 2 | Cb << 4 (JPT1).  Returns
// the lane's rejected streams.
template <bool kLuma, bool kTight>
__device__ __forceinline__ uint32_t sdecode_wave(SDecLds<kLuma ? 64 : 32, kLuma ? kFastCap : kChromaCap> &S,
                                                 int lane, const uint8_t *rec, bool good,
                                                 const uint32_t (&so)[3], const uint32_t (&m)[3],
                                                 uint32_t md, int16_t *__restrict__ tile_out) {
  constexpr int Cap = kLuma ? kFastCap : kChromaCap;
  uint32_t fails = 0;
  int16_t *o = S.out[lane];
  const SVRow vl{reinterpret_cast<uint8_t *>(&S.vl[0][lane])};
#pragma unroll 1
  for (int c = kLuma ? 0 : 1; c <= (kLuma ? 0 : 2); ++c) {
    const uint32_t mc = c == 0 ? m[0] : c == 1 ? m[1] : m[2];
    const uint32_t oc = c == 0 ? so[0] : c == 1 ? so[1] : so[2];
    const int n = stream_len(c);
    bool ok = false;
    if (good) {
      const StreamSrc<kTight> src(rec + oc, mc, (md >> (2 * c)) & 3u);
      const int U = (int)(mc >> 24);
      const int r = U == 0 ? 0
                    : U <= Cap ? sdecode<Cap>(src, mc, vl, o, n, kLuma ? &S.bm[0][lane] : nullptr)
                               : -1;
      ok = r < 0 ? sdecode_slow(src, mc, o, n) : r != 0;
      fails += !ok;
    }
    if (!ok)                                          // a rejected stream, a malformed record: 0
      for (int j = 0; j < n; ++j) o[j] = 0;
    uint4 *dst = reinterpret_cast<uint4 *>(tile_out + coef_off(c));
    const uint32_t *src32 = reinterpret_cast<const uint32_t *>(o);    // 4-B aligned rows
    for (int v = 0; v < n / 8; ++v)
      dst[v] = make_uint4(src32[4 * v], src32[4 * v + 1], src32[4 * v + 2], src32[4 * v + 3]);
  }
  return fails;
}

// A lane's record of `size` bytes at rec, tile t of the stream: checked by
// the rule every reader shares (record_rule, jpegr_pack_common.h), whose reads
// stay inside the record; then the wave's channel group is decoded.
template <bool kTight>
__device__ __forceinline__ void decode_record(SDecLds<64, kFastCap> &SY, SDecLds<32, kChromaCap> &SC,
                                              int lane, int wv, const uint8_t *rec, uint32_t size,
                                              size_t t, uint64_t *__restrict__ result,
                                              int16_t *__restrict__ tile_out) {
  uint32_t so[3] = {0u, 0u, 0u}, m[3] = {0u, 0u, 0u}, md = 0u;
  const bool good = record_rule<kTight>([&](uint32_t x) -> uint32_t { return rec[x]; }, 0u, size, so, m, md);
  uint32_t fails;
  if (__builtin_amdgcn_readfirstlane(wv) == 0) {
    if (!good)
      atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 1ull + (unsigned long long)t);
    fails = sdecode_wave<true, kTight>(SY, lane, rec, good, so, m, md, tile_out);
  } else {
    fails = sdecode_wave<false, kTight>(SC, lane, rec, good, so, m, md, tile_out);
  }
  // the wave's rejected streams: one add, after jprs_sizes' zero in stream order
  const uint32_t f = (uint32_t)__popcll(__ballot(fails & 1)) + 2u * (uint32_t)__popcll(__ballot(fails & 2));
  if (f && lane == __builtin_ctzll(__ballot(1)))
    atomicAdd(reinterpret_cast<unsigned long long *>(result + 2), (unsigned long long)f);
}

__global__ __launch_bounds__(2 * kLanes) void jprs_decode(
    const uint8_t *__restrict__ in, uint64_t in_len, size_t ntiles, size_t tile0, size_t ntile,
    size_t wg_base, const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, uint64_t *__restrict__ result, int16_t *__restrict__ coef) {
  __shared__ SDecLds<64, kFastCap> SY;
  __shared__ SDecLds<32, kChromaCap> SC;
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
