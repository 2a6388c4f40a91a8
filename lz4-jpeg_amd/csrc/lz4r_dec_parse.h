// lz4r_dec_parse.h -- one lane decodes one block: the byte and slot accessors,
// the copies, the general parser decode_block (choice points, truncated
// readings; as a length finder for bare streams) and the hot path's
// decode_block_plain.
//   - every block first goes through decode_block_plain: every token read
//     plainly, the header decoded as selects and lane masks, the window's
//     bytes by v_alignbyte of selected dwords, whole 16-B stores only (the
//     slot's slack takes what passes its end); anything unusual (a reading
//     that does not fit, an inconsistent end) returns -1 and the general
//     decode_block below redoes the block;
//   - the lane reads its encoded bytes with single unaligned 8/16-byte
//     global loads (L1/L2 absorb the re-reads of the wave's ~20 KB range); a
//     sequence's distance word, up to four literal chunks past the window
//     and the next window are issued together, so the walk waits on memory
//     once per sequence of up to ~77 literals (a load per chunk, each waited for, cost 1.28 ->
//     1.18 ms per GiB: profiles/r06_dec_ab.log; two chunks instead of four, 1.068 ->
//     1.015), longer runs take four chunks per round trip, and each load runs
//     only on the lanes that need it: the vector memory address unit is the
//     bound (TA busy ~80 % of the kernel, ~45 cycles per scattered wave load,
//     profiles/r06_dec_ta_pmc.txt), and a lane with exec off costs it nothing (1.17 ->
//     1.06 ms per GiB);
//   - literals move in 16-byte chunks; a match of distance D is copied in
//     chunks of min(16, d) bytes at a distance d that grows from D (the
//     match is D-periodic, so any multiple of D up to the bytes already
//     written + D is a valid distance), with D < 8 seeded by replicating
//     its period over 8 bytes;
//   - the general path's stores within 16 bytes of the 300-B end are
//     exact-size (b64/b32/b16/b8 pieces).
// L comes from the exact u16 size field; the one ambiguous token family
// (0xFD..0xFF: L >= 15 with M = 17 / 18 / >= 19, or a truncated match
// M = 1..3 whatever L, LZ4.c:317 + :540-544) is resolved by a per-lane
// stack of choice points (registers): the plain reading is taken first and undone if the
// block does not then end exactly at its last byte with 300 decoded bytes
// (or 1..300 for the last block) and size fields summing to the block
// header's (LZ4.c:617).  A plain reading of such a token decodes >= 32
// bytes, so at most 9 choice points are ever pending; a backtrack rewrites
// the tail.  A sequence's size field equals the bytes it occupies, plus one
// for a truncated reading, so the running sum is (ip - 3) + #truncated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4r_dec_layout.h"

namespace {

constexpr int kDepth = 10;                 // choice points per lane (<= 9 needed)
constexpr int kMaxSteps = 1 << 16;         // header budget: a hostile stream cannot spin a lane

typedef uint64_t u64u __attribute__((aligned(1)));
typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint16_t u16u __attribute__((aligned(1)));

struct V16 {
  uint64_t lo, hi;
};

// The lane's encoded block in global memory; `avail` = readable bytes from p.
// kSafe: bounds-checked (only the wave holding the stream's last bytes needs
// it; everywhere else a 16-byte read past a block stays inside the stream).
template <bool kSafe>
struct Bytes {
  const uint8_t *p;
  size_t avail;

  __device__ __forceinline__ uint64_t ld8(int a) const {
    if (!kSafe || (size_t)a + 8 <= avail) return *reinterpret_cast<const u64u *>(p + a);
    uint64_t r = 0;
    for (int t = 0; t < 8; ++t)
      if ((size_t)(a + t) < avail) r |= (uint64_t)p[a + t] << (8 * t);
    return r;
  }
  __device__ __forceinline__ V16 ld16(int a) const {
    if (!kSafe || (size_t)a + 16 <= avail) {
      const u64u *q = reinterpret_cast<const u64u *>(p + a);
      return {q[0], q[1]};
    }
    return {ld8(a), ld8(a + 8)};
  }
};

// The same, unchecked, as a wave-uniform base and the lane's 32-bit offset
// from it: every load is global_load with an SGPR base and a VGPR offset,
// with no 64-bit address arithmetic on the walk's dependency chain (64-bit
// VALU issues at ~5.6 cycles per wave-instruction on gfx950, a 32-bit add at
// ~2.3: tools/valu_rate).
struct BytesW {
  const uint8_t *base;
  uint32_t off;

  __device__ __forceinline__ uint64_t ld8(int a) const {
    return *reinterpret_cast<const u64u *>(base + (off + (uint32_t)a));
  }
  __device__ __forceinline__ V16 ld16(int a) const {
    const uint32_t x = off + (uint32_t)a;
    return {*reinterpret_cast<const u64u *>(base + x), *reinterpret_cast<const u64u *>(base + x + 8u)};
  }
};

// The lane's 300-byte output slot in LDS.  Reads may run past the slot
// (into a neighbour or the slack) and are masked by the caller; writes are
// exact.
struct Slot {
  uint8_t *o;

  __device__ __forceinline__ uint64_t ld8(int a) const {
    return *reinterpret_cast<const u64u *>(o + a);
  }
  __device__ __forceinline__ V16 ld16(int a) const {
    const u64u *q = reinterpret_cast<const u64u *>(o + a);
    return {q[0], q[1]};
  }
  // v at o[a .. a+16) when that stays inside the slot, else exactly n bytes.
  // Bytes past the n meant ones land beyond the lane's write frontier and
  // are overwritten before anything reads them (output is produced in
  // order; a backtrack rewrites from the choice point on).
  __device__ __forceinline__ void st_fast(int a, V16 v, int n) const {
    if (a + 16 <= kBlk) {
      *reinterpret_cast<u64u *>(o + a) = v.lo;
      *reinterpret_cast<u64u *>(o + a + 8) = v.hi;
    } else {
      st(a, v, n);
    }
  }
  // the first n (1..16) bytes of v at o[a]
  __device__ __forceinline__ void st(int a, V16 v, int n) const {
    if (n == 16) {
      *reinterpret_cast<u64u *>(o + a) = v.lo;
      *reinterpret_cast<u64u *>(o + a + 8) = v.hi;
      return;
    }
    uint64_t w = v.lo;
    if (n & 8) {
      *reinterpret_cast<u64u *>(o + a) = w;
      a += 8;
      w = v.hi;
    }
    if (n & 4) {
      *reinterpret_cast<u32u *>(o + a) = (uint32_t)w;
      a += 4;
      w >>= 32;
    }
    if (n & 2) {
      *reinterpret_cast<u16u *>(o + a) = (uint16_t)w;
      a += 2;
      w >>= 16;
    }
    if (n & 1) o[a] = (uint8_t)w;
  }
};

// Slots kSlotS apart: 300 bytes of output and 16 of slack, so a 16-B store
// that starts inside the block never reaches the next lane's slot (no
// exact-size stores at the slot end).
constexpr int kSlotS = kBlk + 16;

// The output slot of the fast path: every store is a whole 16-B store (the
// slot's 16-B slack takes what passes its 300 bytes).
struct SlotW {
  uint8_t *o;
  __device__ __forceinline__ uint64_t ld8(int a) const {
    return *reinterpret_cast<const u64u *>(o + a);
  }
  __device__ __forceinline__ V16 ld16(int a) const {
    const u64u *q = reinterpret_cast<const u64u *>(o + a);
    return {q[0], q[1]};
  }
  __device__ __forceinline__ void st_fast(int a, V16 v, int) const {
    *reinterpret_cast<u64u *>(o + a) = v.lo;
    *reinterpret_cast<u64u *>(o + a + 8) = v.hi;
  }
};

// a slot that stores nothing and reads zeros: decode_block as a parser
struct NullSlot {
  __device__ __forceinline__ uint64_t ld8(int) const { return 0; }
  __device__ __forceinline__ V16 ld16(int) const { return {0, 0}; }
  __device__ __forceinline__ void st_fast(int, V16, int) const {}
  __device__ __forceinline__ void st(int, V16, int) const {}
};

// the low D (1..7) bytes of w repeated over 8 bytes
__device__ __forceinline__ uint64_t replicate(uint64_t w, int D) {
  uint64_t x = w & ((1ull << (8 * D)) - 1);
  x |= x << (8 * D);
  if (2 * D < 8) x |= x << (16 * D);
  if (4 * D < 8) x |= x << (32 * D);
  return x;
}

// v >> (8 * nbytes), nbytes in 0..15
__device__ __forceinline__ V16 shr_bytes(V16 v, int nbytes) {
  const int s = 8 * nbytes;
  if (s == 0) return v;
  if (s < 64) return {(v.lo >> s) | (v.hi << (64 - s)), v.hi >> s};
  return {v.hi >> (s - 64), 0};
}

__device__ __forceinline__ int litext_len(int L) {
  if (L < 15) return 0;
  return ((L - 15) & 255) == 255 ? 2 : 1;
}

// Truncated reading of the sequence at ip: match length M = alt in 1..3
// (tokens 0xFD..0xFF only); size field S = L + 5 + litext_len(L) + 1
// (LZ4.c:569-575).  e0, e1 = the two bytes after the size field.
template <typename BytesT>
__device__ bool read_truncated(const BytesT &p, int len, int ip, int Sz, int e0, int e1, int pos,
                               int alt, int &L, int &M, int &D, int &lit, int &nip) {
  const int ip0 = ip + 3;
  M = alt;
  for (int le = 0; le <= 2; ++le) {
    L = Sz - 6 - le;
    if (L < 0 || litext_len(L) != le) continue;
    if (le) {
      const int r = (L - 15) & 255;
      const bool ok = r == 255 ? (ip0 + 1 < len && e0 == 255 && e1 == 0) : (ip0 < len && e0 == r);
      if (!ok) continue;
    }
    lit = ip0 + le;
    if (lit + L + 2 > len || pos + L + M > kBlk) continue;
    D = (int)(p.ld8(lit + L) & 0xFFFF);
    if (D == 0 || D > pos + L) continue;
    nip = lit + L + 2;
    return true;
  }
  return false;
}

// choice point: k 8 | ip 11 | pos 9 | #truncated 2 | next reading 2
__device__ __forceinline__ uint32_t pack_choice(int k, int ip, int pos, int ntr, int alt) {
  return (uint32_t)k | ((uint32_t)ip << 8) | ((uint32_t)pos << 19) | ((uint32_t)ntr << 28) |
         ((uint32_t)alt << 30);
}

// literals p[lit, lit+L) -> o[pos, pos+L), 32 bytes per step
template <typename SlotT, typename BytesT>
__device__ __forceinline__ void copy_literals(const SlotT &o, int pos, const BytesT &p, int lit,
                                              int L) {
  for (int i = 0; i < L; i += 32) {
    const V16 a = p.ld16(lit + i), b = p.ld16(lit + i + 16);
    o.st_fast(pos + i, a, L - i < 16 ? L - i : 16);
    if (i + 16 < L) o.st_fast(pos + i + 16, b, L - i - 16 < 16 ? L - i - 16 : 16);
  }
}

// o[q + i] = o[q - D + i] for i < M, in order (D-periodic when D < M)
template <typename SlotT>
__device__ __forceinline__ void copy_match(const SlotT &o, int q, int D, int M) {
  int i = 0, d = D;
  if (D < 8) {                                   // seed: whole periods within 8 bytes
    const uint64_t x = replicate(o.ld8(q - D), D);
    const int per = (int)((0x76586880u >> (4 * D)) & 15u);   // 8 - 8 % D, nibble D
    i = M < per ? M : per;
    o.st_fast(q, {x, x}, i);
    d = i + D;                                   // i is a multiple of D (or M: done)
  }
  // while d < 16 every step copies d bytes, so i stays a multiple of D and the
  // next distance is i + D (no modulo); from d >= 16 on, d no longer changes
  while (i < M) {
    int n = M - i < 16 ? M - i : 16;
    if (n > d) n = d;
    o.st_fast(q + i, o.ld16(q + i - d), n);
    i += n;
    if (d < 16) d = i + D;                       // grow while short
  }
}

// Decode one block into its slot.  Returns the decoded length, or 0 if the
// block is malformed.  Each sequence is decoded from a 16-byte window h of
// the stream at ip; its distance bytes and literals come from the window
// when they lie inside it, and the next sequence's window is requested as
// soon as the next ip is known (it does not depend on the distance: the
// literal-only tail has tm = 0, so no match-extension byte either way), so
// its load overlaps this sequence's copies.
// kFindLen: the block's end is unknown (a bare stream, lz4_bare_walk's exact
// mode): `len` is the bytes readable from the block start (<= kInMax), the
// block ends at the first complete reading (300 bytes, or 1..300 ending at
// `len` when `last`), and the return value is its byte length, not the
// decoded length (0 = no reading).
template <typename BytesT, typename SlotT, bool kFindLen = false>
__device__ __forceinline__ int decode_block(const BytesT &p, int len, bool last, const SlotT &o) {
  uint32_t stk[kDepth];                              // choice points (registers; rare)
  const uint64_t h0 = p.ld8(0);
  const int nseq = (int)(h0 & 255);                  // nseq & 0xFF; <= 76 in practice
  const int want = (int)((h0 >> 8) & 0xFFFF) - 3;    // LZ4.c:617
  if (len < 3 || nseq == 0 || want < 0) return 0;
  int k = 0, ip = 3, pos = 0, ntr = 0, nch = 0, alt = 0, steps = 0;
  V16 h = p.ld16(3);
  for (;;) {
    bool ok = false;
    int L = 0, M = 0, D = 0, lit = 0, nip = 0;
    V16 hn = {0, 0};
    if (++steps > kMaxSteps) return 0;
    if (k == nseq) {
      if constexpr (kFindLen) {
        if (ip - 3 + ntr == want && (pos == kBlk || (last && ip == len && pos >= 1))) return ip;
      } else {
        if (ip == len && ip - 3 + ntr == want && (pos == kBlk || (last && pos >= 1))) return pos;
      }
    } else if (ip + 3 <= len) {
      const int tok = (int)(h.lo & 255), Sz = (int)((h.lo >> 8) & 0xFFFF);
      const int e0 = (int)((h.lo >> 24) & 255), e1 = (int)((h.lo >> 32) & 255);
      const bool fits = ip - 3 + ntr + Sz <= want;
      if (alt == 0) {
        // plain reading, branch-free: token nibbles as written (M == 0 or M >= 4)
        const int tl = tok >> 4, tm = tok & 15;
        const int mx = tm == 15 ? 1 : 0;
        const bool big = tl == 15;
        const int le = big ? (e0 == 255 ? 2 : 1) : 0;
        L = big ? Sz - 5 - le - mx : tl;
        const int r = (L - 15) & 255;
        bool okp = big ? (L >= 15 && (e0 == 255 ? (r == 255 && e1 == 0) : r == e0))
                       : Sz == L + 5 + mx;
        lit = ip + 3 + le;
        okp = okp && fits && lit + L + 2 <= len && pos + L <= kBlk;
        nip = lit + L + 2 + mx;
        hn = p.ld16(okp ? nip : ip);                 // next window, in flight during the copies
        const int off = lit + L - ip;                // distance bytes within the window?
        const uint32_t t = off + 3 <= 16 ? (uint32_t)shr_bytes(h, off).lo
                                         : (uint32_t)p.ld8(okp ? lit + L : 0);
        D = (int)(t & 0xFFFF);
        const bool hasm = D != 0;
        M = hasm ? (mx ? 19 + (int)((t >> 16) & 255) : tm + 4) : 0;
        okp = okp && (hasm ? (nip <= len && D <= pos + L && pos + L + M <= kBlk)
                           : (k + 1 == nseq && tm == 0));   // literal-only tail, LZ4.c:585-613
        ok = okp;
        if (tok >= 0xFD) {
          if (okp) {                                 // the truncated reading remains
            if (nch == kDepth) return 0;
            stk[nch++] = pack_choice(k, ip, pos, ntr, tok - 0xFC);
          } else {
            alt = tok - 0xFC;
          }
        }
      }
      if (alt != 0) {                                // truncated reading (rare)
        ok = fits && ntr < 3 &&
             read_truncated(p, len, ip, Sz, e0, e1, pos, alt, L, M, D, lit, nip);
        ntr += ok ? 1 : 0;
        if (ok) hn = p.ld16(nip);
      }
    }
    if (ok) {
      if (lit + L <= ip + 16) {                      // literals inside the window
        if (L) o.st_fast(pos, shr_bytes(h, lit - ip), L);
      } else {
        copy_literals(o, pos, p, lit, L);
      }
      if (M) copy_match(o, pos + L, D, M);
      ++k;
      ip = nip;
      h = hn;
      pos += L + M;
      alt = 0;
      continue;
    }
    // dead end: resume the most recent choice point with its other reading
    if (nch == 0) return 0;
    const uint32_t c = stk[--nch];
    k = (int)(c & 255); ip = (int)((c >> 8) & 2047); pos = (int)((c >> 19) & 511);
    ntr = (int)((c >> 28) & 3); alt = (int)(c >> 30);
    h = p.ld16(ip);
  }
}

// The common case of decode_block, for the hot path: every token read
// plainly (no choice points, no truncated readings), one loop iteration per
// sequence with no data-dependent branch but the copies' own loops, so the
// wave issues little exec-mask bookkeeping.  Returns the decoded length, or -1
// when anything is unusual -- a reading that does not fit, or a block that
// does not end consistently -- and decode_block then redoes the block: it
// takes the same plain readings first and backtracks only where they fail,
// so when this path succeeds the general one would return the same bytes.
template <typename BytesT, typename SlotT>
__device__ __forceinline__ int decode_block_plain(const BytesT &p, int len, bool last,
                                                  const SlotT &o) {
  const uint64_t h0 = p.ld8(0);
  const int nseq = (int)(h0 & 255);
  const int want = (int)((h0 >> 8) & 0xFFFF) - 3;    // LZ4.c:617
  if (len < 3 || nseq == 0 || want < 0) return -1;
  int k = 0, ip = 3, pos = 0;
  V16 h = p.ld16(3);
  bool bad = false;
  while (k < nseq) {
    // the window as dwords; bytes [o, o + 4) of it by one v_alignbyte of two
    // selected dwords (no 64-bit shifts, no branches)
    const uint32_t w0 = (uint32_t)h.lo, w1 = (uint32_t)(h.lo >> 32);
    const uint32_t w2 = (uint32_t)h.hi, w3 = (uint32_t)(h.hi >> 32);
    const int tok = (int)(w0 & 255), Sz = (int)((w0 >> 8) & 0xFFFF);
    const int e0 = (int)(w0 >> 24), e1 = (int)(w1 & 255);
    const int tl = tok >> 4, tm = tok & 15;
    const int mx = tm == 15 ? 1 : 0;
    const bool big = tl == 15;
    // the plain reading as selects and lane masks, not branches
    const bool ff = e0 == 255;
    const int le = (big ? 1 : 0) + ((big & ff) ? 1 : 0);
    const int Lb = Sz - 5 - le - mx;
    const int L = big ? Lb : tl;
    const int r = (L - 15) & 255;
    const bool okb = (L >= 15) & ((ff & (r == 255) & (e1 == 0)) | (!ff & (r == e0)));
    const bool oks = Sz == L + 5 + mx;
    bool okp = (big & okb) | (!big & oks);
    const int lit = ip + 3 + le;
    // (bitwise & and |: every test is evaluated, no short-circuit branches;
    // the size-field sum is checked once, after the walk: ip - 3 == want;
    // lit + L + 2 <= len keeps this sequence's reads inside the stream)
    okp = okp & (ip + 3 <= len) & (lit + L + 2 <= len) & (pos + L <= kBlk);
    const int nip = lit + L + 2 + mx;
    // the distance word and up to four literal chunks past the window, loaded
    // together: one wait where a long literal run waited for the distance
    // word, then for each chunk (all inside the stream: the plain path runs
    // only with kInMax + 64 bytes after the block); the next window last, so
    // that waiting for these (vmcnt counts in issue order) does not wait for it
    const int wl = min(L, ip + 16 - lit);
    const int off = lit + L - ip;                    // distance bytes within the window?
    // each load only on the lanes that need it: the vector memory address
    // unit is the decoder's bound (TA busy ~80 % of the kernel, ~45 cycles
    // per scattered wave load), and a lane with exec off costs it nothing
    uint32_t tw = 0;
    V16 c1 = {0, 0}, c2 = {0, 0}, c3 = {0, 0}, c4 = {0, 0};
    if (okp & (off + 3 > 16)) tw = (uint32_t)p.ld8(lit + L);
    if (okp & (L > wl)) c1 = p.ld16(lit + wl);
    if (okp & (L > wl + 16)) c2 = p.ld16(lit + wl + 16);
    if (okp & (L > wl + 32)) c3 = p.ld16(lit + wl + 32);
    if (okp & (L > wl + 48)) c4 = p.ld16(lit + wl + 48);
    const V16 hn = p.ld16(okp ? nip : ip);           // next window, in flight during the copies
    uint32_t t;
    {
      const int wi = off >> 2;
      const uint32_t a = wi == 0 ? w0 : wi == 1 ? w1 : wi == 2 ? w2 : w3;
      const uint32_t c = wi == 0 ? w1 : wi == 1 ? w2 : w3;
      t = __builtin_amdgcn_alignbyte(c, a, (uint32_t)off & 3u);
    }
    if (off + 3 > 16) t = tw;
    const int D = (int)(t & 0xFFFF);
    const bool hasm = D != 0;
    const int Mx = 19 + (int)((t >> 16) & 255), Ms = tm + 4;
    const int M = hasm ? (mx ? Mx : Ms) : 0;
    const bool mok = (nip <= len) & (D <= pos + L) & (pos + L + M <= kBlk);
    const bool tailok = (k + 1 == nseq) & (tm == 0);   // literal-only tail, LZ4.c:585-613
    okp = okp & ((hasm & mok) | (!hasm & tailok));
    if (!okp) {
      // a use of the chunks and the next window on this path too, so that
      // their loads are not sunk below this test (issued apart, they would be
      // waited for apart)
      asm volatile("" ::"v"(c1.lo), "v"(c1.hi), "v"(c2.lo), "v"(c2.hi), "v"(c3.lo), "v"(c3.hi),
                   "v"(c4.lo), "v"(c4.hi), "v"(hn.lo), "v"(hn.hi));
      bad = true;
      break;
    }
    // literals: the window's bytes, the two chunks, then 16 at a time.  The
    // first two stores are unconditional: they stay inside the slot and its
    // slack (pos + wl <= pos + L <= 300), and what they write past the run is
    // overwritten by the match or the next sequence before anything reads it
    {
      // the window from byte d = lit - ip (3, 4 or 5): dwords from w[d >> 2]
      const bool d4 = le > 0;                         // d = 3 + le
      const uint32_t sh = (uint32_t)(3 + le) & 3u;
      const uint32_t s0 = d4 ? w1 : w0, s1 = d4 ? w2 : w1, s2 = d4 ? w3 : w2, s3 = d4 ? 0u : w3;
      const uint32_t o0 = __builtin_amdgcn_alignbyte(s1, s0, sh);
      const uint32_t o1 = __builtin_amdgcn_alignbyte(s2, s1, sh);
      const uint32_t o2 = __builtin_amdgcn_alignbyte(s3, s2, sh);
      const uint32_t o3 = __builtin_amdgcn_alignbyte(0u, s3, sh);
      o.st_fast(pos, {(uint64_t)o1 << 32 | o0, (uint64_t)o3 << 32 | o2}, wl);
    }
    o.st_fast(pos + wl, c1, min(16, L - wl));
    if (L > wl + 16) o.st_fast(pos + wl + 16, c2, min(16, L - wl - 16));
    if (L > wl + 32) o.st_fast(pos + wl + 32, c3, min(16, L - wl - 32));
    if (L > wl + 48) o.st_fast(pos + wl + 48, c4, min(16, L - wl - 48));
    // longer runs: four chunks per memory round trip (loaded on the lanes
    // that need each, then stored), not one
    for (int i = wl + 64; i < L; i += 64) {
      V16 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = {0, 0};
        if (i + 16 * j < L) v[j] = p.ld16(lit + i + 16 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + 16 * j < L) o.st_fast(pos + i + 16 * j, v[j], min(16, L - i - 16 * j));
    }
    // match: one 16-B piece, unconditionally (with no match it writes inside
    // the slot's slack what the next sequence overwrites), then the general
    // copy when the match overlaps itself or exceeds 16 bytes
    const int q = pos + L;
    o.st_fast(q, o.ld16(q - D), M);
    if ((M > 16) | ((M > 0) & (D < 16))) copy_match(o, q, D, M);
    ++k;
    ip = nip;
    h = hn;
    pos += L + M;
  }
  if (bad || ip != len || ip - 3 != want || !(pos == kBlk || (last && pos >= 1))) return -1;
  return pos;
}

}  // namespace
