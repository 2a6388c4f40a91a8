// lz4r_tile_lds.h -- the LDS of one lz4_tiles wave (one 300-byte block) and
// the primitives tied to its layout: the bucket-head exchanges, the add-TID
// stores over its arrays and the lcp loops (used by encode_block, lz4r_tiles.h).
#pragma once
#include "lz4r_layout.h"
#include "wave64.h"

namespace {

constexpr int kHB = 10;                   // hash bits: 1024 buckets
constexpr int kH = 1 << kHB;
constexpr int kArr = 320;                // per-position arrays: every lane's five positions
                                         // (p = 5 l + r <= 319) in range, no index clamps
constexpr int kQ = kBlk + 64;            // walker queue: reads run up to 63 past the last
constexpr int kCand = 128;               // candidate list (drained when a pass could fill it)
constexpr uint32_t kEmptyHead = 0xFFFFFFFCu;   // an emptied bucket head; as an entry's
                                              // 11-bit link field it reads kNoLink
constexpr uint32_t kNoLink = 2044;       // chain end: an empty head (0x07FC), a dword-aligned
                                         // offset, so the reads past a chain's end stay aligned
static_assert(kArr >= 64 * 5, "blocked positions of all 64 lanes");
static_assert((kEmptyHead & 0x7FFu) == kNoLink && kNoLink >= 4 * kArr, "the chain-end link");

// LDS of one wave (4,976 B: 32 waves per CU).  Byte offsets in TileLds::buf:
//   [kInOff, +348)     the block (byte kInOff - 1 is read as blk[-1]) + an
//                      over-read pad (lcp reads)
//   [kQOff, +1456)     chain walkers (q), or the slow walk's sequence starts (seq)
//   [kCandOff, +512)   candidate pairs
// then ent[320] and rec[320].  While the block is indexed, the 1024 u32
// bucket heads overlay [kHeadOff, +4096) = q, cand, ent and rec[0..192), all
// dead until the index is built (ent and rec are written after the heads'
// last exchange).
constexpr int kInOff = 16;
constexpr int kQOff = 368;
constexpr int kCandOff = kQOff + 4 * kQ;
constexpr int kHeadOff = kQOff;
constexpr int kBufBytes = kHeadOff + 2 * kH > kCandOff + 4 * kCand ? kHeadOff + 2 * kH
                                                                   : kCandOff + 4 * kCand;
static_assert(kInOff + kBlk + 48 <= kQOff && kQOff % 16 == 0 && kInOff % 16 == 0 &&
                  kBlk == 75 * 4,
              "dword staging (75 dwords), aligned regions");

struct TileLds {
  alignas(16) uint8_t buf[kBufBytes];
  union {
    uint32_t ent[kArr];   // per position: link | (p == 0) << 15 | blk[p - 1] << 16 | blk[p] << 24
    uint32_t word[kArr];  // then: the first match at or after x, as its record word
  };
  uint32_t rec[kArr];     // local(p) accumulator: end << 19 | end << 9 | dist (end = p + len)
  // chain walkers: the walker's byte offset 4 p (candidate phase)
  __device__ __forceinline__ uint32_t *q() { return reinterpret_cast<uint32_t *>(buf + kQOff); }
  // per sequence, its match start (slow walk only)
  __device__ __forceinline__ uint32_t *seq() { return reinterpret_cast<uint32_t *>(buf + kQOff); }
  // candidate pairs p | j << 16 awaiting the lcp pass
  __device__ __forceinline__ uint32_t *cand() { return reinterpret_cast<uint32_t *>(buf + kCandOff); }
};

constexpr int kWordOff = kBufBytes;             // byte offset of ent / word in TileLds
constexpr int kRecOff = kBufBytes + 4 * kArr;   // byte offset of rec in TileLds
// word[] past the last match: its field (the next read's byte offset) is
// 4 * 319 > 4 n, the walk's exit, and stays inside the array
constexpr uint32_t kWordEnd = (uint32_t)(4 * (kArr - 1)) << 17;
static_assert(kHeadOff + 4 * kH <= kRecOff + 4 * 192, "u32 heads end before rec[192]");
static_assert(kRecOff + 4 * kArr <= 4976, "LDS of one wave");

// Five ds_wrxchg_rtn_b32 back to back, one wait: old = *(head base + a); *(...) = v.
// The addresses are relative to the head array (kHeadOff, the instruction's
// offset field); the LDS serves one wave's operations in order, so a later
// exchange of the same head sees the earlier.
// Each head this block uses is first emptied by the positions that hash to
// it (five ds_write_b32 of kEmptyHead, before any exchange; the LDS serves one
// wave's operations in order): a head no position of the block maps to is
// never read, so the other ~800 of the 1024 need no reset (5 scattered
// stores instead of 16 ds_write_addtid_b32 over the whole 4 KB).
__device__ __forceinline__ void xchg_rtn5(uint32_t (&old)[5], const uint32_t (&a)[5],
                                          const uint32_t (&v)[5]) {
  asm volatile(
      "ds_write_b32 %5, %15 offset:368\n\t"
      "ds_write_b32 %6, %15 offset:368\n\t"
      "ds_write_b32 %7, %15 offset:368\n\t"
      "ds_write_b32 %8, %15 offset:368\n\t"
      "ds_write_b32 %9, %15 offset:368\n\t"
      "ds_wrxchg_rtn_b32 %0, %5, %10 offset:368\n\t"
      "ds_wrxchg_rtn_b32 %1, %6, %11 offset:368\n\t"
      "ds_wrxchg_rtn_b32 %2, %7, %12 offset:368\n\t"
      "ds_wrxchg_rtn_b32 %3, %8, %13 offset:368\n\t"
      "ds_wrxchg_rtn_b32 %4, %9, %14 offset:368\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(old[0]), "=&v"(old[1]), "=&v"(old[2]), "=&v"(old[3]), "=&v"(old[4])
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]),
        "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(kEmptyHead)
      : "memory");
}

static_assert(kHeadOff == 368 && kH == 1024, "xchg_rtn5 offsets");

// ent[64 r + lane] = e[r] (the position-major entries, r = 0..4) and zero
// rec[0 .. 320) (1,280 B at kRecOff, the local(p) accumulators) with
// ds_write_addtid_b32: 10 stores of 2 LDS cycles each, one m0 set.  Called
// after the heads' last exchange (ent and rec[0 .. 192) lie under the heads).
__device__ __forceinline__ void ent_store_rec_zero_addtid(const uint32_t (&e)[5]) {
  asm volatile(
      "s_mov_b32 m0, 0\n\t"
      "s_nop 0\n\t"
      "ds_write_addtid_b32 %0 offset:%c6\n\t"
      "ds_write_addtid_b32 %1 offset:%c7\n\t"
      "ds_write_addtid_b32 %2 offset:%c8\n\t"
      "ds_write_addtid_b32 %3 offset:%c9\n\t"
      "ds_write_addtid_b32 %4 offset:%c10\n\t"
      "ds_write_addtid_b32 %5 offset:%c11\n\t"
      "ds_write_addtid_b32 %5 offset:%c12\n\t"
      "ds_write_addtid_b32 %5 offset:%c13\n\t"
      "ds_write_addtid_b32 %5 offset:%c14\n\t"
      "ds_write_addtid_b32 %5 offset:%c15"
      :
      : "v"(e[0]), "v"(e[1]), "v"(e[2]), "v"(e[3]), "v"(e[4]), "v"(0u),
        "i"(kBufBytes), "i"(kBufBytes + 256), "i"(kBufBytes + 512), "i"(kBufBytes + 768),
        "i"(kBufBytes + 1024), "i"(kRecOff), "i"(kRecOff + 256), "i"(kRecOff + 512),
        "i"(kRecOff + 768), "i"(kRecOff + 1024)
      : "memory");
}

// key[64 r + lane] = k[r] over the walker queue (kQOff), one m0 set.
__device__ __forceinline__ void keys_store_addtid(const uint32_t (&k)[5]) {
  asm volatile(
      "s_mov_b32 m0, 0\n\t"
      "s_nop 0\n\t"
      "ds_write_addtid_b32 %0 offset:%c5\n\t"
      "ds_write_addtid_b32 %1 offset:%c6\n\t"
      "ds_write_addtid_b32 %2 offset:%c7\n\t"
      "ds_write_addtid_b32 %3 offset:%c8\n\t"
      "ds_write_addtid_b32 %4 offset:%c9"
      :
      : "v"(k[0]), "v"(k[1]), "v"(k[2]), "v"(k[3]), "v"(k[4]), "i"(kQOff), "i"(kQOff + 256),
        "i"(kQOff + 512), "i"(kQOff + 768), "i"(kQOff + 1024)
      : "memory");
}

// Longest common prefix of the byte runs at a and b (a < b), capped at
// `limit` = n - b: the canonical clamp (a match never crosses the block end).
// Each operand's 16 bytes come from aligned dwords and v_alignbyte: a
// misaligned ds_read_b128 is replayed at ~64 LDS cycles, and the kernel's
// LDS array is ~80 % busy (SQ_LDS_IDX_ACTIVE), so the 4 extra VALU per
// operand pay (-1 % lz4_tiles; an earlier 8-byte funnel-shift form cost ~30
// VALU per block and lost).  Reads past the region land in its pad (>= 48 B
// past any block end; the aligned form reads at most 19 past it).
__device__ __forceinline__ int lcp(const uint8_t *d, int a, int b, int limit) {
  // a step continues only after 16 equal bytes, so both operands keep their
  // byte alignment: the shifts are loop-invariant and the dword pointers
  // advance by 16 bytes
  const uint32_t sa = (uint32_t)a & 3u, sb = (uint32_t)b & 3u;
  const uint32_t *wa = reinterpret_cast<const uint32_t *>(d + (a & ~3));
  const uint32_t *wb = reinterpret_cast<const uint32_t *>(d + (b & ~3));
  int l = 0;
  for (;;) {                              // 16 bytes per step
    // 16 bytes from five aligned dwords (two ds_read2_b32 and a ds_read_b32:
    // no misaligned replay), byte-aligned by v_alignbyte
    auto at16 = [](const uint32_t *w, uint32_t sh) {
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
      return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh),
                        __builtin_amdgcn_alignbyte(w2, w1, sh),
                        __builtin_amdgcn_alignbyte(w3, w2, sh),
                        __builtin_amdgcn_alignbyte(w4, w3, sh));
    };
    const uint4 A = at16(wa, sa), B = at16(wb, sb);
    // first differing bit of the 16 bytes: v_ffbl per dword (-1 when equal),
    // offset by 32 k with an OR (each is < 32 or all ones), min over the four
    const uint32_t m = min(min(ffbl(A.x ^ B.x), ffbl(A.y ^ B.y) | 32u),
                           min(ffbl(A.z ^ B.z) | 64u, ffbl(A.w ^ B.w) | 96u));
    l += (int)min(m >> 3, 16u);
    if (m != 0xFFFFFFFFu || l >= limit) break;
    wa += 4;
    wb += 4;
  }
  return l < limit ? l : limit;
}

// The same over the 4-gram keys (kj = &key[j], kp = &key[p], j < p): the
// 16 bytes at a position are key[x], key[x + 4], key[x + 8], key[x + 12].
// key[] covers positions 0 .. 319 and a step reads at most 12 past p + l
// < n <= 300.
__device__ __forceinline__ int lcp_keys(const uint32_t *kj, const uint32_t *kp, int limit) {
  int l = 0;
  for (;;) {
    const uint32_t a0 = kj[0], a1 = kj[4], a2 = kj[8], a3 = kj[12];
    const uint32_t b0 = kp[0], b1 = kp[4], b2 = kp[8], b3 = kp[12];
    const uint32_t m = min(min(ffbl(a0 ^ b0), ffbl(a1 ^ b1) | 32u),
                           min(ffbl(a2 ^ b2) | 64u, ffbl(a3 ^ b3) | 96u));
    l += (int)min(m >> 3, 16u);
    if (m != 0xFFFFFFFFu || l >= limit) break;
    kj += 16;
    kp += 16;
  }
  return l < limit ? l : limit;
}

// The same from global memory (kFull blocks, whose bytes are not staged in
// LDS: only a drain in the middle of the walk, when a pass could overflow the
// candidate list, uses it): 16 bytes per operand and step as one unaligned
// global_load_dwordx4 (L1/L2-resident: the block was just read).  Reads reach
// at most 15 bytes past the block end, into the next block.
__device__ __forceinline__ int lcp_global(const uint8_t *a, const uint8_t *b, int limit) {
  int l = 0;
  for (;;) {
    uint4 A, B;
    __builtin_memcpy(&A, a + l, 16);
    __builtin_memcpy(&B, b + l, 16);
    const uint32_t m = min(min(ffbl(A.x ^ B.x), ffbl(A.y ^ B.y) | 32u),
                           min(ffbl(A.z ^ B.z) | 64u, ffbl(A.w ^ B.w) | 96u));
    l += (int)min(m >> 3, 16u);
    if (m != 0xFFFFFFFFu || l >= limit) break;
  }
  return l < limit ? l : limit;
}

}  // namespace
