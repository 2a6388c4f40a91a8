// jpegr_decode_common.h -- what the entropy stage's two decoders share: the
// wave's decode state in LDS, the carry-chain compare, the per-stream walk
// (decode_stream) and its slow form (decode_stream_slow), each over a source
// of the stream's bits, and the tail of a wave's stream (the row's 16-B
// stores; the count of rejected streams: wave64.h).  jpegr_entropy.hip decodes slots
// (SlotBits / SlotTable below: whole 16-B chunks of the stream's slot);
// jpegr_stream.hip decodes a JPR1 / JPT1 stream (ByteBits below over its
// StreamSrc: bytes of the lane's own checked record).  One walk, two sources:
// object code and time against the two copies it replaces are in
// profiles/entropy_walks_refactor.md.  Each keeps its own
// kernel, its loads ahead of the walk and its way to publish the count.
#pragma once
#include "jpegr_entropy_common.h"
#include "wave64.h"

namespace {

// Per stream up to 24 (luma) / 12 (chroma) codes, like the encoder's
// working set (more: regenerated per symbol, decode_stream_slow): the
// left-aligned codes in registers, each code's value and length in LDS as one
// u16 (value in 11 bits, two's complement, | length << 11: every value of a
// 4K image's streams fits; a stream whose values or lengths do not takes the
// slow path), one row of u16 per code.  With the decoded ints and the luma
// start map: 13.3 KiB per luma wave, 6.0 KiB per chroma wave (a lane decodes
// the tile's Cr, then its Cb stream), one of each per workgroup: a 4K image's
// 2,025 workgroups are all resident at once.
template <int N, int Cap>
struct DecLds {
  uint16_t vl[Cap][kLanes];                // code k: value | len << 11 (row k, the lane's u16)
  // the lane's decoded ints; rows of N + 2 (an odd number of dwords), so the
  // lanes' stores at one index hit 64 different banks (rows of N: 32-way)
  alignas(16) int16_t out[kLanes][N + 2];
  // luma: the lane's code starts as a 256-bit map over the 8-bit windows
  // (row r, bit 31 - i: window 32 r + i), for streams whose codes are all
  // <= 8 bits long
  uint32_t bm[N == 64 ? 8 : 1][kLanes];
};

// One lane's u16 column of a [rows][64] u16 block: entry k at byte k * 128
// (one address op per lookup; two lanes share a dword, so lanes reading
// different rows of the same bank pair conflict two-way at most)
struct VRow {
  typedef uint16_t __attribute__((may_alias)) HA;
  uint8_t *p;                                   // &block[0][lane] as bytes
  __device__ __forceinline__ HA &operator[](int k) const {
    return *reinterpret_cast<HA *>(p + (uint32_t)k * (2 * kLanes));
  }
};

// The number of k < Cap with h[k] > w (31-bit values): the borrows of
// w - h[k], taken by v_sub_co_u32 into SGPR pairs and summed by
// v_addc_co_u32 in two chains, eight codes per asm block (each carry is read
// at least eight instructions after its write: no hazard wait states; a
// group of four pads with an s_nop).
template <int Cap>
__device__ __forceinline__ uint32_t count_above(uint32_t w, const uint32_t (&h)[Cap]) {
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

// ---- where a stream's bits come from -------------------------------------------
// The fast walk takes its bits 32 at a time, MSB-first, through a cursor that
// it builds where it starts on the bits, Bits bs(n, from...): peek32(), then
// advance(), which also puts the read after it in flight.  `from` reaches the
// walk by value and the cursor is a local of the walk: with the slot cursor
// built by the caller and handed in, the slot decoder's chunk words stayed a
// vector and the call measured 1 to 7 % slower on a smooth 4K image
// (profiles/entropy_walks_refactor.md).

// A slot's bits: whole 16-B chunks of the stream's slot (n / 8 of them for n
// ints).  q0, q1: the first two chunks, loaded by the caller with the meta word.
// The next chunk is in flight.  Chunks past the bits are read too (they lie
// in the slot, and what they hold cannot change a decode: see lookup), so the
// load needs no select; the chunk index is clamped to the slot's last chunk.
struct SlotBits {
  const uint4 *src;
  int last;                                         // the slot's last chunk
  uint4 q, nxt;
  int qi, ci;
  __device__ __forceinline__ SlotBits(int n, const uint8_t *bits, uint4 q0, uint4 q1)
      : src(reinterpret_cast<const uint4 *>(bits)), last(n / 8 - 1), q(q0), nxt(q1), qi(0), ci(1) {}
  __device__ __forceinline__ uint32_t peek32() const { return __builtin_bswap32(q.x); }
  __device__ __forceinline__ void advance() {
    // the chunk's words move down as they are used (an indexed select
    // became a scratch array)
    q.x = q.y;
    q.y = q.z;
    q.z = q.w;
    if (++qi == 4) {
      qi = 0;
      q = nxt;
      ci = ci < last ? ci + 1 : ci;
      nxt = src[ci];
    }
  }
};

// The bits of a byte source (be32(j): bytes j .. j + 3, the first in the top
// byte, every read bounded by the source): the next 32 bits are loaded a
// refill ahead of their use.
template <typename Src>
struct ByteBits {
  const Src &s;
  uint32_t nw;
  int bi;
  __device__ __forceinline__ ByteBits(int, const Src *src) : s(*src), nw(src->be32(0)), bi(0) {}
  __device__ __forceinline__ uint32_t peek32() const { return nw; }
  __device__ __forceinline__ void advance() {
    bi += 4;
    nw = s.be32(bi);
  }
};

// Decode one stream: bits + table -> RLE ints (decode_huffman) -> n ints
// (inverse_RLE: counts clamped to n, zero fill).  With one code (empty bit
// string) the reference decodes nothing and keeps its RLE ints: rle_len
// copies of the symbol.  Bits, from: the cursor over the stream's bits and
// what it is built from (above); tb: the table's first Cap entries as
// d_table's words (value | length << 16; past U: unused), loaded by the
// caller; bm: the lane's start-map column (luma) or null.
// The symbol at a window is the count of codes <= it, minus one: the codes
// of a table built from a tree increase strictly (DFS order; a table whose
// codes do not is no tree and takes the slow path, which matches codes in
// table order).  When every code of the wave is <= 8 bits (a random 4K
// image's luma) the count is one row of a 256-bit map of the code starts
// plus that row's prefix count; otherwise Cap compares against the
// left-aligned codes in registers.  Only the matched entry's value | length
// is read from LDS (vl).
// The walk goes a (count, value) pair per step, so the inverse RLE's fill runs
// once per pair with every lane of the wave on it, and no lane carries a
// count across steps; the bit buffer is refilled once per one, two or four
// symbols, as the wave's longest code allows.  Every instruction of the walk
// counts: a wave issues at most one per four cycles, and two luma and two
// chroma waves share each SIMD.
// Returns 1 (decoded), 0 (malformed) or -1 (a value or length that the u16
// entries cannot hold, or codes that do not increase: the caller runs
// decode_stream_slow).
template <int Cap, typename Bits, typename VlT, typename... BitArgs>
__device__ int decode_stream(uint32_t m, const uint32_t (&tb)[Cap], VlT vl,
                             int16_t *__restrict__ out, int n, uint32_t *bm, BitArgs... from) {
  const int nbits = (int)(m & 0xFFFF), R = (int)((m >> 16) & 255), U = (int)(m >> 24);
  if (U == 0 || U > Cap || R == 0 || R > 2 * n) return 0;
  // codes from the lengths, left to right (DFS order); lh[k] = lc[k] >> 1 (a
  // code of <= 31 bits leaves bit 0 of its left-aligned form clear), all ones
  // past U: above every 31-bit window, never counted as <= it
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
  // a run of cnt copies of v at idx (clamped to the row): the first store
  // unconditionally (past the run it is overwritten by the next run or the
  // final zero fill; the row has spare slots), a loop only for longer runs
  // (an empty asm keeps the loop a loop: as a memset it compiled to three
  // nested loops whose exec-mask bookkeeping every pair paid)
  auto fill = [&](int cnt, int v) {
    const int c = min(cnt, n - idx);
    out[idx] = (int16_t)v;
    for (int j = 1; j < c; ++j) {
      out[idx + j] = (int16_t)v;
      asm volatile("");
    }
    idx += max(c, 0);
  };
  // an entry's value (11-bit two's complement) and length
  auto val = [](uint32_t e) { return (int)((int32_t)(e << 21) >> 21); };
  if (U == 1) {
    const int v = val(vl[0]);
    for (int j = 0; j + 1 < R; j += 2) fill(v, v);
  } else {
    // MSB-first bit buffer: acc holds nacc valid bits, left-aligned
    Bits bs(n, from...);
    uint64_t acc = 0;
    int nacc = 0, p = 0, got = 0;
    // s codes lie above the window, a suffix of the increasing codes: the
    // entry is k = Cap - 1 - s, at byte -128 s from entry Cap - 1
    const uint8_t *vbase = reinterpret_cast<const uint8_t *>(&vl[Cap - 1]);
    // Codes of at most 8 bits in every stream of the wave: the symbol at a
    // window is found from its top 8 bits as the count of code starts <= them
    // -- one row of the lane's 256-bit start map (LDS, built with ors) and
    // that row's prefix count (registers, a byte each) instead of Cap
    // compares.  Wave-uniform, so no lane walks both.
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
      if (nacc <= 32) {                               // refill 32 bits (codes <= 31)
        acc |= (uint64_t)bs.peek32() << (32 - nacc);
        nacc += 32;
        bs.advance();
      }
    };
    auto lookup = [&]() -> uint32_t {
      // 32 bits at p.  Bits past the end are not masked: the codes increase
      // strictly, so they are prefix-free, and a code that fits in the bits
      // left is found whatever follows them (one that does not fit is
      // malformed either way)
      const uint32_t win = (uint32_t)(acc >> 32);
      if (use_bm) {
        const uint32_t w8 = win >> 24, j = w8 >> 5;
        const uint32_t row = bm[j * kLanes];
        const uint32_t before = __builtin_amdgcn_perm(pb, pa, j | 0x0C0C0C00u);
        const int cnt = (int)(__builtin_popcount(row >> (31 - (w8 & 31))) + before);
        return vl[cnt - 1];
      }
      // borrows of win - lh[k] in two carry chains through SGPR pairs (the
      // compare-and-add form serialised every code on VCC)
      const uint32_t above = count_above<Cap>(win >> 1, lh);
      return *reinterpret_cast<const uint16_t *>(vbase - (int)(above * (2 * kLanes)));
    };
    // one symbol at p (bits in acc): its entry; a code past the end ends the
    // walk as malformed (flagged, no branch out of the loop per symbol)
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
    // a (count, value) pair: the count, then (bits left) its value and the run
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
    // a refill leaves >= 33 bits: four symbols when every code of the wave
    // is <= 8 bits, two when <= 16, else one (wave-uniform cadence)
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

// What the slow walk reads of a slot: the bits as big-endian words of the
// slot (the word past the last bit is not read), the table as d_table's words
struct SlotTable {
  const uint32_t *wds, *table;
  int nbits;
  __device__ __forceinline__ uint32_t window(int p) const {     // 32 bits at bit p
    const int wi = p >> 5, sh = p & 31;
    const uint32_t w0 = __builtin_bswap32(wds[wi]);
    const uint32_t w1 = (wi + 1) * 32 < nbits ? __builtin_bswap32(wds[wi + 1]) : 0;
    return sh ? (w0 << sh) | (w1 >> (32 - sh)) : w0;
  }
  __device__ __forceinline__ uint32_t entry(int k) const { return table[k]; }
  __device__ __forceinline__ int len(int k) const { return (int)((table[k] >> 16) & 255); }
};

// Streams with more codes than the LDS table holds (> 24 luma / 12 chroma:
// the encoder's deferred streams) or a table the fast walk cannot take: the
// codes are regenerated from the table for every symbol and searched linearly
// -- slow, rare, no storage.  S: window(p), the 32 bits at bit p (what lies
// past the stream's bits is masked here); len(k) and entry(k), code k's
// length and its d_table word.
template <typename Src>
__device__ bool decode_stream_slow(const Src &S, uint32_t m, int16_t *__restrict__ out, int n) {
  const int nbits = (int)(m & 0xFFFF), R = (int)((m >> 16) & 255), U = (int)(m >> 24);
  if (R == 0 || R > 2 * n) return false;
  // (a count may be any int16 of the table, negative ones included: whether a
  // count is pending is a flag of its own, not a sign)
  int p = 0, got = 0, idx = 0, pending = 0;
  bool have = false;
  while (p < nbits) {
    uint32_t win = S.window(p);
    if (nbits - p < 32) win &= ~0u << (32 - (nbits - p));
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

// ---- the tail of a wave's stream ------------------------------------------------

// The lane's n decoded ints, collected in its LDS row o (4-B aligned), to dst
// as 16-B stores (2-byte stores to 64 scattered streams wrote ~6x the bytes)
__device__ __forceinline__ void store_ints(const int16_t *o, int16_t *__restrict__ dst, int n) {
  uint4 *d = reinterpret_cast<uint4 *>(dst);
  const uint32_t *src = reinterpret_cast<const uint32_t *>(o);
  for (int v = 0; v < n / 8; ++v)
    d[v] = make_uint4(src[4 * v], src[4 * v + 1], src[4 * v + 2], src[4 * v + 3]);
}

}  // namespace
