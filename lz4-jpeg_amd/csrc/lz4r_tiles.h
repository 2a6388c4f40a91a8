// lz4r_tiles.h -- lz4_tiles, the compressor's compute kernel, and the batch
// match finders that share its index.
//
// lz4_tiles: workgroup = one wave = a run of kTileRun consecutive 300-B blocks,
// encoded one after the other (4,976 B of LDS, <= 64 VGPRs -> 8 waves per
// SIMD; occupancy is what this LDS- and issue-bound kernel lives on).  A
// one-block wave spent its first stretch waiting for its block's bytes from
// HBM while holding one of its SIMD's 8 slots; in a run only the first block
// does, every other finds its dwords in registers, loaded while the block
// before was encoded.
//
// Reuse of the LDS by the next block of a run needs no clean-up, by the same
// argument that lets a fresh workgroup start on whatever the last one left
// there -- every array is written by a block before that block reads it, and
// the wave's LDS operations are served in program order:
//   heads     a block reads only heads its own positions hash to, and each
//             position empties its head before the first exchange (xchg_rtn5);
//             the dummy slots rec[192 + lane] that inactive positions
//             exchange with are emptied first in the same way
//   ent, rec  ent[p] stored for every position a chain can reach and rec[]
//             zeroed whole (ent_store_rec_zero_addtid) after the heads' last
//             exchange, before the walk reads either
//   queue     entries [0, qn) written, then exactly those read (reads past qn
//             are masked off by idx4 < qwr4)
//   cand      [0, ncand) written by the passes, then exactly those drained
//   keys      all 320 stored (keys_store_addtid) before a drain reads them
//   word      all 320 stored by the word pass before the walk; seq [0, Sv)
//             written by the redone walk before the records read it
//   staged    a staged block writes its n bytes and 16 zero bytes of pad
//             first; byte kInOff - 1 (blk[-1]) is any byte: position 0 is
//             left-maximal by its own bit
// and the registers a block starts from (lane, the kernel arguments, m0 and
// the priority, both set by the asm blocks that use them) do not depend on
// the block before -- but for the one state that crosses blocks on purpose,
// RecBatch: the match words of a block whose records wait for the next
// block's (a VGPR, lanes 0..31) and the number of those lanes (an SGPR).  It
// is safe because it lives in registers only (no block writes them but the
// walk, which starts at lane 32 while a block waits, and is undone when it
// runs on past lane 63), it never outlives the run (the last block of a run,
// and any block before a staged one, leaves with its round), and a round
// reads nothing from LDS.  tests/test_gpu_lz4_runs.py and
// tests/test_gpu_lz4_records_batch.py pin it against the oracle.
//
// Per block:
//   load     a lane's five positions need 14 dwords (TileKeys), straight from
//            global memory into registers -- the only read of the input; the
//            block is NOT staged in LDS, except the launch's last block, the
//            one before a last block of < 24 bytes and unaligned inputs
//            (bytewise, with a zero pad).
//   position-major (lane l owns p = 64 r + l, r = 0..4):
//     index  per-bucket chains of the 4-gram starts by a 10-bit hash: each
//            position empties its bucket's u32 head, then exchanges itself
//            into it (ds_wrxchg_rtn_b32) in ascending position order and keeps
//            the old head as its link (byte offsets 4 p), so every chain
//            strictly decreases; entry = link | (p == 0) << 15 | preceding
//            byte << 16 | own byte (the tag) << 24, stored by add-TID.
//     local  every unordered pair of a bucket is met once, by the later
//            position walking its chain (deepest walkers first); a lane
//            keeps its walker until the chain ends -- or a link fails to
//            decrease: the walk ends on any input -- and then takes the next
//            queued one.  A pair (j < p) is a candidate when the tags agree
//            and it is LEFT-MAXIMAL (j == 0 or blk[j-1] != blk[p-1]): one
//            v_xad + one compare of the two entries; a balanced lcp pass over
//            the 4-gram keys takes the longest candidate per p, ties to the
//            smallest j (LDS atomicMax of end << 19 | end << 9 | dist: the end
//            twice, so that subtracting p << 9 later leaves the record word).
//   blocked (lane l owns p = 5 l .. 5 l + 4):
//     best   a candidate that is not left-maximal is the pair (j-1, p-1)
//            shifted by one, whose match is one byte longer.  Hence
//              best(p) = lexmax over q <= p of (q + local_len(q), q - local_j(q))
//            i.e. the longest match ends furthest right and, among equals,
//            has the largest distance (= smallest source, LZ4.c:307).  A
//            running max over the lane's five and one wave max-scan give
//            best() for all p.  M = len & 0xFF (the uint8_t return, LZ4.c:317).
//     parse  word[x] = the record word (dist | M << 9 | 4 (c + M) << 17) of
//            c = the first matchable position >= x (a suffix pass over the
//            positions); the greedy parse (LZ4.c:516-583) is the walk
//            w_0 = word[0], w_{k+1} = word[c_k + M_k], one LDS read per
//            sequence.
//   records  sequence k on lane k: one packed wave scan of the bytes the block
//            takes and of its size fields; the header dword and record k
//            (lz4r_layout.h) -> the block's record scratch (a dense 96-B
//            head: header and records 0..22; an overflow slot for the rest);
//            the block's byte count -> bsizes (u16: what the scan and
//            lz4_emit read, and what the caller is handed).  Two
//            consecutive unstaged blocks of a run share one such
//            round, one on each half of the wave (RecBatch, flush_records:
//            a text block has ~15 sequences); a staged block, or one with
//            more than 31 match sequences, has a round of its own.
#pragma once
#include <type_traits>

#include "lz4r_prof.h"
#include "lz4r_tile_lds.h"

namespace {

// The dwords of a kFull block that lane l's five positions 64 r + l need,
// straight from global memory (src 4-byte aligned; d = l >> 2): dwords d and
// d + 1 for row 0 (one global_load_dwordx2), dwords 16 r + d - 1 .. + 1 for
// rows 1..4 (the dword before carries blk[p - 1]; one global_load_dwordx3
// each).  Row 4's lanes read up to 24 bytes past the block's 300.
// Held as the loads' own register tuples: carried around lz4_tiles' loop as
// single dwords, each load's result was copied out of its tuple -- and
// waited for -- right after the load was issued.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
struct TileKeys {
  u32x2 r0;      // row 0: dwords d, d + 1
  u32x3 r[4];    // row 1 + i: dwords 16 (1 + i) + d - 1, .. + d, .. + d + 1
};

// threadIdx.x, opaque to the compiler: lz4_tiles takes it once per block of
// its run, so each block derives the lane constants of its phases again (as
// a one-block workgroup does) instead of keeping them in ~60 registers
// across the loop -- the kernel has 64 (8 waves per SIMD).
__device__ __forceinline__ int block_lane() {
  int lane = threadIdx.x;
  asm volatile("" : "+v"(lane));
  __builtin_assume(lane >= 0 && lane < 64);   // (what the opaque copy forgot: LDS offsets fold)
  return lane;
}

__device__ __forceinline__ void load_keys(TileKeys &K, const uint8_t *__restrict__ src, int lane) {
  typedef u32x2 u32x2_a4 __attribute__((aligned(4)));
  typedef u32x3 u32x3_a4 __attribute__((aligned(4)));
  const uint32_t *bw = reinterpret_cast<const uint32_t *>(src) + (lane >> 2);
  K.r0 = *reinterpret_cast<const u32x2_a4 *>(bw);
#pragma unroll
  for (int r = 1; r < 5; ++r) K.r[r - 1] = *reinterpret_cast<const u32x3_a4 *>(bw + 16 * r - 1);
}

// The loaded dwords are used from here on: the compiler waits for K's loads
// at this point (and nowhere later).  lz4_tiles places it where no younger
// memory operation is in flight -- after a run's first, cold load, and in
// every block before the records are stored.  Waited for at the top of the
// next block instead, the loads' counter also held that block's record stores,
// issued after them: each block then began by waiting for the stores of the
// block before to be acknowledged (~2,000 cycles, LZ4R_PROF).
__device__ __forceinline__ void keys_arrived(TileKeys &K) {
  asm volatile("" : "+v"(K.r0), "+v"(K.r[0]), "+v"(K.r[1]), "+v"(K.r[2]), "+v"(K.r[3]));
}

// The records of two consecutive kFull blocks of a run leave in one round:
// the first block's walk writes its match words into lanes 0.. of a register,
// the second's into lanes 32.., and each block closes with a lane for its
// literal-only tail (n << 19), used or not.  A block of more than 31 match
// sequences does not fit a half and leaves alone.  The state that crosses
// blocks is the register and one SGPR; nothing of it is in LDS.
struct RecBatch {
  uint32_t seqv = 0;   // lane k: the pending block's sequence k
  uint32_t p0 = 0;     // 0: no block pending; else the lanes it takes (1 .. 32) |
                       // (it has a truncated match) << 8 | kHalf << 16 (the lane
                       // the next walk starts from)
};
constexpr int kHalf = 32;

// the inclusive sums of the lanes' values within each half of the wave
// (wave_incl_add without its last step)
__device__ __forceinline__ uint32_t half_incl_add(uint32_t v) {
  v += dpp<0x111, 0xf, 0xf>(v);
  v += dpp<0x112, 0xf, 0xf>(v);
  v += dpp<0x114, 0xf, 0xf>(v);
  v += dpp<0x118, 0xf, 0xf>(v);
  v += dpp<0x142, 0xa, 0xf>(v);
  return v;
}

// Block tb + lane's header dword = hdr, bsizes = (u16) w in the lanes
// of m, EXEC masked once around the two stores (store_lanes1's way).  The
// block index goes into the lanes' 32-bit offsets off the arrays' bases (a
// launch has at most 2^24 blocks, lz4r.hip kChunk: 96 tb < 2^31); a pointer
// per array and block cost three SALU each.
__device__ __forceinline__ void store_block_totals(uint64_t m, uint32_t tb, int lane, uint32_t hdr,
                                                   uint32_t w, uint8_t *heads, uint16_t *bsizes) {
  const uint32_t bl = tb + (uint32_t)lane;
  uint64_t save;
  asm volatile(
      "s_and_saveexec_b64 %0, %1\n\t"
      "global_store_dword %2, %4, %6\n\t"
      "global_store_short %3, %5, %7\n\t"
      "s_or_b64 exec, exec, %0"
      : "=&s"(save)
      : "s"(m), "v"(bl * (uint32_t)kHead), "v"(bl * 2u), "v"(hdr), "v"(w), "s"(heads), "s"(bsizes)
      : "memory", "scc");
}

// One records round for the block on lanes [0, f0) of wv and, when f1, the
// block after it on lanes [32, 32 + f1) (both kFull: n = kBlk); tb: the first
// block's index in the launch's arrays.  What a block leaves is what its own
// round left (encode_block): record k at dword 1 + k of the head below
// kHeadW - 1 and in the overflow slot from there on, the header dword, the
// byte count.  kFast: neither block has a truncated match.
template <bool kFast>
__device__ __forceinline__ void flush_records(const uint32_t wv, const uint32_t f0,
                                              const uint32_t f1, const uint32_t tb,
                                              uint8_t *__restrict__ heads,
                                              uint8_t *__restrict__ ovfs,
                                              uint16_t *__restrict__ bsizes, const int lane) {
  constexpr int n = kBlk;
  const int M = (int)((wv >> 9) & 255u);
  const int end = (int)(wv >> 19);
  const uint32_t cq = (uint32_t)(end - M);                          // the match start
  const uint32_t upv = dpp<0x138, 0xf, 0xf>((uint32_t)end);         // wave_shr:1
  // a block's first sequence has its literal run start at 0, not at the lane below
  const int pend = (int)sel_mask(0x0000000100000001ull, 0u, upv);
  const int L = (int)cq - pend;
  // every taken lane but a tail with no literal left (a match lane has
  // pend <= its match start < n)
  const uint64_t am = (((1ull << f0) - 1ull) | ((1ull << f1) - 1ull) << kHalf) & ballot(pend < n);
  uint32_t ws;                        // bytes | size field << 16 (kFast: the bytes are both)
  if constexpr (kFast) {
    ws = (uint32_t)(L + 5) + (L >= 15 ? 1u : 0u) + (L == 270 ? 1u : 0u) + (M >= 19 ? 1u : 0u);
  } else {
    ws = (uint32_t)(L + 5 + (L >= 15 ? 1 : 0) + (L == 270 ? 1 : 0)) * 0x10001u;
    ws += M >= 19 ? 0x10001u : 0u;
    ws += (uint32_t)(M - 1) < 3u ? 0x10000u : 0u;
  }
  const uint32_t sc = half_incl_add(sel_mask(am, ws, 0u));
  // the blocks' totals stand in the last lane of their halves -> the header
  // dword and the byte count in lane 0 (first block) and the others (second)
  const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)sc, kHalf - 1);
  const uint32_t t1 = lane63(sc);
  const uint32_t ns0 = (uint32_t)__popc((uint32_t)am), ns1 = (uint32_t)__popc((uint32_t)(am >> kHalf));
  uint32_t hdr, wb;
  if constexpr (kFast) {
    hdr = write_lane<0>(t1 | (ns1 << 16), t0 | (ns0 << 16));
    wb = (hdr & 0xFFFFu) + 3u;
  } else {
    // (opaque: as one expression the two shifts are taken for a funnel shift,
    // which only the VALU has)
    uint32_t z0 = t0 >> 16, z1 = t1 >> 16;
    asm("" : "+s"(z0));
    asm("" : "+s"(z1));
    hdr = write_lane<0>(z1 | (ns1 << 16), z0 | (ns0 << 16));
    wb = write_lane<0>((t1 & 0xFFFFu) + 3u, (t0 & 0xFFFFu) + 3u);
  }
  // record kk = lane & 31 of block lane >> 5: the head below kHeadW - 1, the
  // overflow slot from there on (store_lanes1 adds the header's 4 bytes)
  constexpr uint64_t kHeadLanes = ((1ull << (kHeadW - 1)) - 1ull) * 0x0000000100000001ull;
  // (the second half's offsets by arithmetic on lane & 32: a select by a
  // constant lane mask costs an SGPR pair the kernel does not have)
  const uint32_t x4 = 4u * (uint32_t)lane, h32 = (uint32_t)lane & (uint32_t)kHalf;
  store_lanes1(am & kHeadLanes, reinterpret_cast<uint32_t *>(heads + (size_t)tb * kHead),
               x4 - h32 * ((128 - kHead) / kHalf), wv);
  const uint64_t om = am & ~kHeadLanes;
  if (om)
    store_lanes1(om, reinterpret_cast<uint32_t *>(ovfs + (size_t)tb * kOvf) - kHeadW,
                 x4 + (h32 << 3) + (h32 >> 1), wv);
  static_assert(kOvf - 4 * kHalf == 8 * kHalf + kHalf / 2, "the second overflow slot from lane & 32");
  store_block_totals(f1 ? 3ull : 1ull, tb, lane, hdr, wb, heads, bsizes);
}
static_assert((128 - kHead) % kHalf == 0 && kHeadW - 1 < kHalf, "the second half's records");

// Encode one block (kFull: its dwords in K, the bytes at gsrc; otherwise n
// bytes staged at S.buf[kInOff]) as sequence records:
// dwords 0 .. kHeadW - 1 (header, records 0..22) at its head (heads + t kHead),
// record k >= 23 at dword k + 1 - kHeadW of its overflow slot (ovfs + t kOvf),
// and the bytes its stream takes at bsizes[t].
// kMatchesOnly: stop after the best-match scan and store every position's
// find_longest_match result to mout instead (lz4r_block_matches_device).
// next (kFull in a run, kTileRun > 1): the block whose dwords are loaded into K
// once the index has consumed this block's, and fly during the rest of the
// block -- the block the caller encodes next when that is a kFull block too,
// else this block again (gsrc; never used, but the load is unconditional: no
// branch in the index, and K has one definition per block).
// B (kFull in a run): the block's records wait for the next block's and leave
// in a round shared with them (flush_records) -- at once when flush_after (the
// caller encodes no kFull block next) or when they are the second block's.
template <bool kMatchesOnly, bool kFull>
__device__ __forceinline__ void encode_block(TileLds &S, int n_arg, const uint8_t *__restrict__ gsrc,
                                            TileKeys &K, const uint8_t *__restrict__ next,
                                            uint32_t *__restrict__ mout,
                                            uint8_t *__restrict__ heads,
                                            uint8_t *__restrict__ ovfs,
                                            uint32_t *__restrict__ status, const int lane,
                                            ProfClock &prof, RecBatch &B, const bool flush_after,
                                            uint16_t *__restrict__ bsizes, const uint32_t t) {
  // kFull: a whole 300-byte block of a 4-byte aligned input that is not the
  // launch's last (every block but one): n is a constant, only round 4's
  // lanes 41..63 hold positions past the last 4-gram start, and the block is
  // NOT staged in LDS -- each lane's 4-grams come from the dwords the caller
  // (or the block before, see next) loaded straight from gsrc into K (the 24
  // bytes past the block end that row 4 reads belong to the next block);
  // otherwise the block is staged at S.buf[kInOff] by the caller.
  const int n = kFull ? kBlk : n_arg;
  constexpr int base = kInOff;

  // ---- index: per-bucket chains of the 4-gram starts -----------------------
  // Position-major: lane l owns p_r = 64 r + l (r = 0..4; positions 297..319
  // of a full block start no 4-gram).  Round r exchanges the 64 positions
  // 64 r .. 64 r + 63 into their buckets' u32 heads (ds_wrxchg_rtn_b32, the
  // five rounds back to back, one wait) and keeps each old head as the
  // position's link.  Insertion is in ascending position order (rounds
  // ascend; within one exchange the LDS serves the lanes in ascending order),
  // so every link is a smaller byte offset than its position or empty: a
  // chain strictly decreases, and a walk that stops at the first link not
  // below the current one ends on any input -- even on a corrupted head.
  // Entry (byte offsets 4 p):  link (bits 0..10) | p == 0 (bit 15) |
  // preceding byte (16..23) | tag (24..31: the position's own byte, which
  // equal 4-grams share).  Entries are written by ds_write_addtid_b32
  // (2 LDS cycles per round instead of 4-6 for a strided store).
  const int nk = n >= 4 ? n - 3 : 0;     // positions that start a 4-gram

  bool walk[5];                          // p_r has a link (a walker)
  uint32_t qn = 0;                       // walkers queued
  uint32_t key[5];                       // p_r's 4-gram (kept for the lcp drain)
  {
    // bytes p .. p + 3 from two aligned dwords: sh = p & 3 = lane & 3
    const uint32_t sh = (uint32_t)lane & 3u;
    // (staged: the same dwords from LDS, one ds_read2_b32 per row and a
    // ds_read_b32 for the dword before)
    const uint32_t *bw = reinterpret_cast<const uint32_t *>(S.buf) + (kInOff >> 2) + (lane >> 2);
    uint32_t pt[5], adr[5], set[5];
    // inactive positions (p >= nk) exchange with a dword of rec[192 + lane]
    // (past the heads, zeroed after the exchanges; distinct per lane)
    const uint32_t dummy = (uint32_t)(kRecOff + 4 * (192 + lane) - kHeadOff);
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const uint32_t w1 = !kFull ? bw[16 * r] : r ? K.r[r ? r - 1 : 0].y : K.r0.x;
      const uint32_t w2 = !kFull ? bw[16 * r + 1] : r ? K.r[r ? r - 1 : 0].z : K.r0.y;
      key[r] = __builtin_amdgcn_alignbyte(w2, w1, sh);
      const uint32_t hv = key[r] * 2654435761u;                    // bucket = top 10 bits
      // [0, 0, blk[p - 1], blk[p]]: the entry without its link.  The tag
      // (byte 3) is the position's own first byte: any function of the 4-gram
      // serves (equal 4-grams always agree; a pair that agrees by chance is
      // a candidate whose lcp is < 4), and this one costs no hash bits
      if (r == 0) {
        // blk[p - 1] = byte 0 of the lane below's key (DPP wave_shr:1; lane 0
        // is p = 0, whose byte is the sentinel bit below)
        const uint32_t pb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key[0], 0x138, 0xf,
                                                                 0xf, false);
        pt[0] = __builtin_amdgcn_perm(pb, key[0], 0x00040C0Cu);
      } else {
        // rows 1..4: bytes 3 + sh and 4 + sh of the dword pair before (one
        // more dword in the same load, no cross-lane step)
        const uint32_t w0 = kFull ? K.r[r - 1].x : bw[16 * r - 1];
        pt[r] = __builtin_amdgcn_perm(w1, w0, 0x04030C0Cu + sh * 0x01010000u);
      }
      const int p = 64 * r + lane;
      // (full block: rounds 0..3 are all 4-gram starts)
      const bool act = (kFull && r < 4) || p < nk;
      adr[r] = act ? (hv >> (32 - kHB)) << 2 : dummy;
      set[r] = (uint32_t)(4 * p);
    }
    if (lane == 0) pt[0] |= 1u << 15;     // p = 0: left-maximal with every later position
    if (kFull && kTileRun > 1) {
      // K is consumed once key[] and pt[] exist (pinned here: computed later,
      // pt[] kept K's registers alive and the new dwords took others, copied
      // back around the loop): the next block's dwords take K's registers and
      // fly until that block's index
#pragma unroll
      for (int r = 0; r < 5; ++r) asm volatile("" : "+v"(key[r]), "+v"(pt[r]));
      load_keys(K, next, lane);
    }
    uint32_t old[5];
    xchg_rtn5(old, adr, set);
#ifdef LZ4R_STALE_HEAD
    // tools build (tools/poison_check.sh): one stale head (a forward link, as
    // a missed reset would leave) -- the walk must still end and the call
    // report LZ4R_ERR_CORRUPT
    if (lane == 7) old[2] = 4u * 250u;
#endif
    uint32_t e[5];
    int d[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      // the link field is 11 bits: kEmptyHead reads kNoLink (2044)
      e[r] = (old[r] & 0x7FFu) | pt[r];  // inactive: never read (no chain reaches it)
      // a link (not an empty head, -4 as an int); on a sound LDS an earlier
      // position -- checked below, and a walk ends at any non-decreasing link
      walk[r] = (int)old[r] >= 0;
      // a link is an earlier position (old - 4 p < 0) or an empty head
      // (kEmptyHead = -4 as an int: old - 4 p < 0 too); anything else is a
      // corrupt head.  One subtraction per position and two v_max3.
      d[r] = (int)(old[r] - set[r]);
    }
    const int y = max(max(max(d[0], d[1]), d[2]), max(d[3], d[4]));
    // (never on a sound LDS; the batch match finder has no status word)
    if (!kMatchesOnly && ballot(y >= 0)) atomicOr(status, 1u);
    // queue the walkers row by row from r = 4 down (later positions first:
    // the deepest chains start early, which keeps the walk passes near the
    // longest chain), lanes ascending within a row; the queue overlays the
    // heads, dead after the exchanges (the LDS serves the wave in order)
#pragma unroll
    for (int r = 4; r >= 0; --r) {
      const uint64_t m = ballot(walk[r]);
      // only the walkers' lanes store (EXEC = m around the store)
      lds_store_lanes<kQOff>(m, rank_below_plus(m, qn) << 2, set[r]);
      qn += (uint32_t)__popcll(m);
    }
    ent_store_rec_zero_addtid(e);        // ent[64 r + lane] = e[r]; rec[] = 0
  }
  PROF_MARK(0);                       // index + walker queue
  wave_sync();
  const int qwr = (int)qn;               // walkers queued (S.q()[0 .. qwr))
  wave_sync();

  PROF_MARK(1);                       // walker queue
  // ---- candidates: walk the chains ------------------------------------------
  // A pair (j < p) of one bucket is a candidate when the tags agree and the
  // match is left-maximal (j == 0 or blk[j-1] != blk[p-1]): with x = the two
  // entries xor'ed, exactly when 2^15 <= x < 2^24 (bits 24..31 zero: the
  // tags agree; some bit 15..23 set: the preceding bytes differ or j == 0).
  // Candidates go to a list in S.cand, drained by a balanced lcp pass with
  // LDS atomicMax into S.rec (end << 19 | end << 9 | (p - j), end = p + len:
  // the longest, ties to
  // the smallest j).
  uint32_t longm = 0;                    // this lane verified a candidate of >= 256 bytes
  {
    constexpr int kTrash = kCand - 1;
    int ncand = 0;
    const uint8_t *const entb = reinterpret_cast<const uint8_t *>(S.ent);
    auto ent_at = [&](int off) { return *reinterpret_cast<const uint32_t *>(entb + off); };
    // kKeys: the walk is over and the queue region holds every position's
    // 4-gram key (key[p] = bytes p .. p + 3 as a dword), so a 16-byte lcp
    // step is four aligned dword reads per operand (two ds_read2_b32), with
    // no byte alignment; a drain in the middle of the walk (more than 63
    // candidates) reads the staged block with v_alignbyte
    auto drain = [&](auto keys) {
      constexpr bool kKeys = decltype(keys)::value;
      wave_sync();
      for (int i = lane; i < ncand; i += 64) {
        const uint32_t pr = S.cand()[i];
        const int p = (int)(pr & 0xFFFFu) >> 2, j = (int)(pr >> 18);   // j < p: chains decrease
        const int l = kKeys ? lcp_keys(S.q() + j, S.q() + p, n - p)
                      : kFull ? lcp_global(gsrc + j, gsrc + p, n - p)
                              : lcp(S.buf, base + j, base + p, n - p);
        // (end, dist) as the best scan wants it: for one p the larger end is
        // the longer match and the larger dist the smaller source
        if (l >= 4) {
          // end << 19 | end << 9 | dist (the end twice: see the word pass)
          atomicMax(&S.rec[p], (uint32_t)(p + l) * 0x80200u | (uint32_t)(p - j));
        }
        longm |= l >= 256 ? 1u : 0u;     // (a match the uint8_t return truncates)
      }
      wave_sync();
    };
    // Persistent walkers: a lane keeps its walker (a walks, b = the next chain
    // entry) in registers until the chain ends, and an idle lane takes the
    // next queued walker.  The queue is read once, front to back: no ring,
    // no re-queue stores.  The walkers' liveness is a scalar lane mask (the
    // selects read it straight from SGPRs, written by SALU ops only).
    int qrd4 = 0;
    const int qwr4 = 4 * qwr;
    const uint8_t *const qb = reinterpret_cast<const uint8_t *>(S.q());
    int a = 0, b = 0;
    uint32_t me = 0;                       // the walker's own entry (re-read only on a take)
    uint64_t vm = 0;                       // lanes holding a walker
    // one pass: every live walker meets its next chain entry
    auto pass = [&]() {
      const uint32_t o = ent_at(b);
      const uint64_t cm = vm & ballot(((me ^ o) - (1u << 15)) < (1u << 24) - (1u << 15));
      // the pair (walker, chain entry): the entry is the earlier position
      lds_store_lanes<kCandOff>(cm, rank_below_plus(cm, (uint32_t)ncand) << 2,
                                (uint32_t)a | ((uint32_t)b << 16));
      ncand += __popcll(cm);
      const int bn = (int)(o & 2047u);
      vm &= ballot(bn < b);                // the chain ends (kNoLink, or any non-decreasing link)
      b = bn;
      if (ncand > kTrash - 64) {           // (rare: a full list drains mid-walk)
        drain(std::false_type{});
        ncand = 0;
      }
    };
    // while walkers are queued, idle lanes take them (uniform); then the
    // passes go on without the take
    while (qrd4 < qwr4) {
      const uint64_t em = ~vm;
      const int idx4 = qrd4 + (rank_below(em) << 2);
      const uint64_t nm_ = em & ballot(idx4 < qwr4);
      const uint32_t it = *reinterpret_cast<const uint32_t *>(qb + idx4);   // idx <= qwr + 63 < kQ
      a = (int)sel_mask(nm_, it, (uint32_t)a);
      vm |= nm_;
      qrd4 += 4 * __popcll(em);
      me = ent_at(a);                      // (lanes that kept their walker read the same word)
      b = (int)sel_mask(nm_, me & 2047u, (uint32_t)b);   // a new walker starts at its link
      pass();
    }
    while (vm) {                         // (unrolled by two: -0.6 % lz4_tiles)
      pass();
      if (!vm) break;
      pass();
    }
    if (ncand) {
      keys_store_addtid(key);            // the queue is dead: keys over it
      drain(std::true_type{});
    }
  }
  wave_sync();
  PROF_MARK(2);                       // candidates + lcp
  // ---- best(p) = prefix lexmax of (end, dist) -------------------------------
  // (from here on the per-position phases are BLOCKED: lane l owns
  // p = 5 l .. 5 l + 4, so a prefix over positions is a running max over the
  // lane's five plus one wave scan; the arrays in LDS are indexed by p in
  // either layout)
  const int p0 = 5 * lane;
  // blocked: a running max over the lane's five positions, one wave scan of
  // the lane totals, the exclusive prefix folded back in
  uint32_t v[5];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    // local(p) as end << 19 | end << 9 | dist; 0 without a candidate and at
    // and past n
    v[r] = S.rec[p0 + r];
    if (r) v[r] = max(v[r], v[r - 1]);
  }
  {
    const uint32_t incl = wave_incl_max(v[4]);
    const uint32_t excl = dpp<0x138, 0xf, 0xf>(incl);     // wave_shr:1, lane 0 gets 0
#pragma unroll
    for (int r = 0; r < 5; ++r) v[r] = max(v[r], excl);
  }
  if constexpr (kMatchesOnly) {
    // find_longest_match (LZ4.c:290-323) at every p: len | dist << 16, both 0
    // below MIN_MATCH_LENGTH (the uint8_t truncation is the caller's)
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int p = p0 + r;
      const int len = (int)(v[r] >> 19) - p;
      if (p < n) mout[p] = len >= 4 ? (uint32_t)len | ((v[r] & 511u) << 16) : 0u;
    }
    return;
  }
  // The scan values are end << 19 | end << 9 | dist (the lexicographic order
  // of (end, dist): the middle copy follows the end), so x = v - p << 9 =
  // end << 19 | len << 9 | dist; a match covers p when end >= p + 4 (one
  // compare of the scan value), and M = len & 0xFF (the uint8_t return,
  // LZ4.c:317).  A match starts at p when len >= 4 and M != 0 (len 256 is a
  // literal, LZ4.c:521).
  // The greedy parse (LZ4.c:516-583) at x -- 0, then the end of the previous
  // match -- takes the first matchable position c = nm(x) >= x with its M and
  // dist.  word[x] holds exactly that, as the match's own record word
  //   dist | M << 9 | (c + M) << 19
  // -- x itself when the match is not truncated (len < 256) -- whose top
  // field, as the shifted word >> 17 = 4 (c + M), is the byte offset of the
  // next word the walk reads, or kWordEnd when no match starts at or after x.
  // So the walk reads one word per sequence and needs no successor table (no
  // gathers, no second array).
  // (the word pass is instantiated for both cases below, so the match flags
  // stay lane masks in SGPRs: merged across a branch they were packed into
  // a VGPR and unpacked again, ~15 VALU)
  const uint32_t nP9 = 0u - ((uint32_t)p0 << 9);
  const uint32_t K0 = (uint32_t)(p0 + 4) << 19;
  auto word_pass = [&](auto fast) -> uint32_t {
    uint32_t rw[5];               // p's own word (where a match starts at p)
    bool mt[5];                   // a match starts at p (len >= 4, M != 0)
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const uint32_t x = v[r] + nP9 + (0u - ((uint32_t)r << 9));   // one v_add3
      const bool m4 = v[r] >= K0 + ((uint32_t)r << 19);             // len >= 4
      if constexpr (decltype(fast)::value) {
        mt[r] = m4;
        rw[r] = x;
      } else {
        const uint32_t M = __builtin_amdgcn_ubfe(x, 9, 8);
        mt[r] = m4 && M != 0u;
        rw[r] = ((M + (uint32_t)(p0 + r)) << 19) | (x & 0x1FFFFu);
      }
    }
    PROF_MARK(3);                     // best scan
    // ---- word[x] for x in [0, n]: a suffix "next match" over the positions
    uint32_t loc = kWordEnd;      // the lane's own first match word
#pragma unroll
    for (int r = 4; r >= 0; --r) loc = mt[r] ? rw[r] : loc;
    const uint64_t has = ballot(loc != kWordEnd);
    const uint64_t up = has & ~((2ull << lane) - 1ull);  // lanes above this one
    const int src = up ? ctz64(up) : lane;
    const uint32_t nx = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)loc);
    uint32_t w = up ? nx : kWordEnd;
    uint32_t wr[5];
#pragma unroll
    for (int r = 4; r >= 0; --r) wr[r] = w = mt[r] ? rw[r] : w;
#pragma unroll
    for (int r = 0; r < 5; ++r)
      S.word[p0 + r] = wr[r];            // past n: kWordEnd (no match starts there)
    return (uint32_t)__builtin_amdgcn_readlane((int)wr[0], 0);   // word[0]
  };
  // No verified candidate reached 256 bytes, so no best(p) does (a scan term
  // is a candidate shifted right, never longer): len < 256, M = len, every
  // len >= 4 is a match, and the word is x (its bits 17..18, len's bits
  // 8..9, are zero).  Otherwise the general form (M = len & 0xFF, len 256 no
  // match).  The records rounds are instantiated the same way: without a
  // truncated match no M is 1..3, so a sequence's size field is its byte
  // count and one plain wave sum gives both.
  const bool fastw = !ballot(longm != 0u);   // no truncated match: M = len, never 1..3
  const uint32_t w0 = fastw ? word_pass(std::true_type{}) : word_pass(std::false_type{});
  wave_sync();

  PROF_MARK(4);                       // word
  // ---- greedy parse = walk over the match words (LZ4.c:516-583) -------------
  // The walk is the serial part of the block: w_0 = word[0], w_{k+1} =
  // word[c_k + M_k], one LDS read per sequence; sequence k's word is kept in
  // lane k of a register (v_writelane).  The loop is one asm block: m0 is both
  // the lane select and the sequence counter, the next address is the loaded
  // word shifted in a VGPR, and the loop goes on while the word is a match,
  // i.e. its field 4 (c + M) <= 4 n (kWordEnd's is 4 * 319 > 4 n): three VALU
  // and two SALU per sequence.
  const uint32_t lim = (uint32_t)(4 * n + 1) << 17;
  // the walk into sq from lane l0 on; returns the lane after the last written
  // (not reduced mod 64: past lane 63 the writes wrap)
  auto walk_words = [&](uint32_t &sq, int l0) {
    int l1 = l0;
    if (w0 < lim) {
      static_assert(kWordOff < 65536, "ds_read offset field");
      uint32_t w = w0, va = w0 >> 17, vt;
      asm volatile(
          "s_mov_b32 m0, %7\n"
          "1:\n\t"
          "v_writelane_b32 %0, %1, m0\n\t"
          "ds_read_b32 %3, %2 offset:%c6\n\t"
          "s_add_u32 m0, m0, 1\n\t"
          "s_waitcnt lgkmcnt(0)\n\t"
          "v_readfirstlane_b32 %1, %3\n\t"
          "v_lshrrev_b32 %2, 17, %3\n\t"
          "s_cmp_lt_u32 %1, %5\n\t"
          "s_cbranch_scc1 1b\n\t"
          "s_mov_b32 %4, m0"
          : "+v"(sq), "+s"(w), "+v"(va), "=&v"(vt), "=&s"(l1)
          : "s"(lim), "i"(kWordOff), "s"(l0)
          : "scc", "memory");
    }
    return l1;
  };
  // The walk is the block's one serial chain: the wave issues it at raised
  // priority, so on a SIMD shared with waves in their parallel phases each
  // step goes first (-0.3 % lz4_tiles, tools/ab_inproc.py; raising the index,
  // candidate, scan or records phases instead measured 0.2-5 % slower)
  constexpr bool kBat = kFull && kTileRun > 1;   // the records wait in B for a shared round
  int it;
  uint32_t seqv;
  if constexpr (kBat) {
    // This block's sequences go to lanes 0.. (no block pending) or 32.. (one
    // pending), then its tail lane.  If they do not fit the half (the walk
    // wrote on past it -- over the pending block's words once its lane select
    // wrapped), the register is put back, the pending block leaves alone, and
    // the block is walked again from lane 0 and takes the one-block path below.
    const uint32_t p0 = B.p0;
    const int l0 = (int)(p0 >> 16);
    const uint32_t before = B.seqv;
    seqv = before;
    __builtin_amdgcn_s_setprio(3);
    const int l1 = walk_words(seqv, l0);
    __builtin_amdgcn_s_setprio(0);
    it = l1 - l0;
    const bool fits = it < kHalf;     // with the tail lane
    PROF_MARK(5);                     // walk
    keys_arrived(K);                  // the next block's: loaded since the index
    PROF_MARK(7);
    // the round: of the pending block and this one, of this one (none
    // pending), or of the pending one (this one does not fit).  Plain
    // integers and nested branches: as bools the conditions became lane masks,
    // two SALU each.
    uint32_t f0 = p0 & 255u, f1 = 0u, slowm = p0 & 256u, rv = before;
    if (fits) {
      rv = (lane == l1) ? (uint32_t)n << 19 : seqv;
      slowm |= fastw ? 0u : 256u;
      if (l0 == 0) {
        if (!flush_after) {           // waits for the next block
          B.seqv = rv;
          B.p0 = (uint32_t)(it + 1) | slowm | (uint32_t)kHalf << 16;
          return;
        }
        f0 = (uint32_t)(it + 1);
      } else {
        f1 = (uint32_t)(it + 1);
      }
    }
    B.p0 = 0;
    if (f0) {
      const uint32_t tb = t - (uint32_t)(l0 >> 5);   // the round's first block
      if (slowm == 0u)
        flush_records<true>(rv, f0, f1, tb, heads, ovfs, bsizes, lane);
      else
        flush_records<false>(rv, f0, f1, tb, heads, ovfs, bsizes, lane);
    }
    PROF_MARK(6);                     // records (of both blocks of a round)
    if (fits) return;
    seqv = 0;
    walk_words(seqv, 0);              // (it stays)
  } else {
    seqv = 0;
    __builtin_amdgcn_s_setprio(3);
    it = walk_words(seqv, 0);
    __builtin_amdgcn_s_setprio(0);
  }
  // Past 64 sequences (only with truncated matches) the walk is redone into S.seq.
  const bool slow = it > 64;
  int Sv_slow = 0;
  if (slow) {
    const uint8_t *const wb = reinterpret_cast<const uint8_t *>(S.word);
    for (uint32_t w = w0; w < lim;
         w = (uint32_t)__builtin_amdgcn_readfirstlane(
             (int)*reinterpret_cast<const uint32_t *>(wb + (w >> 17)))) {
      if (lane == 0) S.seq()[Sv_slow] = w;
      ++Sv_slow;
    }
    wave_sync();
  }
  PROF_MARK(5);                       // walk
  // ---- sequence records: lane kk = sequence kk -----------------------------
  // (the block alone: a staged block, or one that did not fit into the batch)
  // A round is 64 consecutive sequences; the match sequences are a prefix
  // (cpos < n), followed by the literal-only tail when the last match ends
  // before n (LZ4.c:585-612).  Rounds go on while a round is all matches.
  // The block leaves as records -- sequence k: its match word dist | M << 9 |
  // (match start + M) << 19 as the walk read it (its literal run starts where
  // sequence k - 1's match ends; the tail is n << 19) -- after a header dword,
  // the sum of the sequences' size fields | the sequence count << 16.  lz4_emit writes the bytes
  // (write_sequence / write_block, LZ4.c:365-425) straight into the stream.
  uint32_t *const head = reinterpret_cast<uint32_t *>(heads + (size_t)t * kHead);
  uint32_t *const ovf = reinterpret_cast<uint32_t *>(ovfs + (size_t)t * kOvf);
  int nseq = 0;
  int ocar = 3;                      // block header: u8 nseq, u16 size
  int szsum = 0;
  int end_prev = 0;                  // end of the previous round's last match
  // one round: sequence kk = s0 + lane has the match word wv (n << 19 -- no
  // match, M = dist = 0, ending at n -- past the matches); returns false once
  // the round holds the last sequence
  auto round = [&](auto fast, int s0, uint32_t wv) {
    const int kk = s0 + lane;
    const int M = (int)((wv >> 9) & 255u);
    const int end = (int)(wv >> 19);
    const uint32_t cq = (uint32_t)(end - M);                       // the match start
    const uint64_t ismm = ballot((int)cq < n);                     // ends with a match
    const int nm_r = __popcll(ismm);                               // a prefix of the round
    const uint32_t upv = dpp<0x138, 0xf, 0xf>((uint32_t)end);   // wave_shr:1
    const int pend = lane == 0 ? end_prev : (int)upv;             // literal run start
    end_prev = (int)lane63((uint32_t)end);
    const int L = (int)cq - pend;
    // + the tail (lane nm_r, when literals are left); the mask from ballots
    // of the compares (a ballot of a combined bool costs two VALU)
    const uint64_t am = ismm | (ballot(lane == nm_r) & ballot(pend < n));
    // bytes written (LZ4.c:365-413) | the size field (LZ4.c:546-575) << 16:
    // 5 + L + the literal-extension bytes (one from 15, two at L = 270, where
    // the uint8_t remainder is 255: LZ4.c:376-385) + a match-extension byte
    // (M >= 19); the size field also counts one for M = 1..3, which
    // write_sequence never writes (LZ4.c:393 vs :562-575)
    if constexpr (decltype(fast)::value) {
      // no M = 1..3 (no truncated match): the size fields are the bytes
      const uint32_t ws = (uint32_t)(L + 5) + (L >= 15 ? 1u : 0u) + (L == 270 ? 1u : 0u) +
                          (M >= 19 ? 1u : 0u);
      const uint32_t tot = lane63(wave_incl_add(sel_mask(am, ws, 0u)));
      ocar += (int)tot;
      szsum += (int)tot;
    } else {
      uint32_t ws = (uint32_t)(L + 5 + (L >= 15 ? 1 : 0) + (L == 270 ? 1 : 0)) * 0x10001u;
      ws += M >= 19 ? 0x10001u : 0u;
      ws += (uint32_t)(M - 1) < 3u ? 0x10000u : 0u;
      const uint32_t tot = lane63(wave_incl_add(sel_mask(am, ws, 0u)));
      ocar += (int)(tot & 0xFFFFu);
      szsum += (int)(tot >> 16);
    }
    // record dword 1 + kk (the sequence's word; the tail: n << 19): the head
    // for kk < kHeadW - 1, the overflow slot after (the same lane offset off
    // a base kHeadW dwords back)
    if (s0 == 0) {
      store_lanes1(am & ((1ull << (kHeadW - 1)) - 1), head, 4u * (uint32_t)kk, wv);
      if (am >> (kHeadW - 1)) store_lanes1(am >> (kHeadW - 1) << (kHeadW - 1), ovf - kHeadW,
                                           4u * (uint32_t)kk, wv);
    } else {
      store_lanes1(am, ovf - kHeadW, 4u * (uint32_t)kk, wv);
    }
    nseq += (int)__popcll(am);
    return nm_r == 64;
  };
  {
    // round 0 from the walk's register; more than 64 sequences (the walk's
    // register wrapped) come from the redone walk in S.seq
    const uint32_t wtail = (uint32_t)n << 19;
    const uint32_t c0 = slow ? S.seq()[lane] : (lane < it ? seqv : wtail);
    auto rounds = [&](auto fast) {
      if (round(fast, 0, c0)) {        // 64 match sequences: the tail or more follow
        for (int s0 = 64;; s0 += 64) {
          const int kk = s0 + lane;
          if (!round(fast, s0, slow && kk < Sv_slow ? S.seq()[kk] : wtail)) break;
        }
      }
    };
    if (fastw)
      rounds(std::true_type{});
    else
      rounds(std::false_type{});
  }
  PROF_MARK(6);                       // records
  // (no branch on the lane here: where it joined the batched return above,
  // the compiler took the batch state for lane-dependent and kept it in VGPRs)
  store_block_totals(1ull, t, lane, (uint32_t)szsum | ((uint32_t)nseq << 16), (uint32_t)ocar, heads,
                     bsizes);
}

// (8 waves per SIMD = 64 VGPRs: around a loop the compiler would otherwise
// keep every block-invariant lane constant in a register of its own)
template <bool kAligned>   // the input is 4-byte aligned (the host checks)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void lz4_tiles(
    const uint8_t *__restrict__ in, uint32_t nb, uint32_t per, uint32_t last_n,
    uint8_t *__restrict__ heads, uint8_t *__restrict__ ovfs, uint16_t *__restrict__ bsizes,
    uint32_t *__restrict__ status) {
  __shared__ TileLds S;
  ProfClock prof = PROF_START();
  // XCD-aware order: workgroups w and w + 8 share an XCD (observed round-robin
  // dealing), so XCD w % 8 takes the contiguous slice [(w % 8) per, ...) of
  // the blocks (per: a multiple of kTileRun) and a 128-B line shared by two
  // neighbouring blocks is fetched into one L2, not two (a speed matter only:
  // any mapping is correct).  Workgroup w takes run w / 8 of its slice.
  const uint32_t t0 = (blockIdx.x & 7u) * per + (blockIdx.x >> 3) * (uint32_t)kTileRun;
  if (t0 >= nb) return;
  const uint32_t t1 = kTileRun == 1 ? t0 + 1 : min(t0 + (uint32_t)kTileRun, nb);
  // Blocks that are not staged: the keys come straight from global memory
  // (encode_block<kFull>): row 4's lanes read 24 bytes past the block end
  // (and a mid-walk lcp drain up to 15), so only where those bytes are the
  // launch's own -- every block but the last, and the one before it when
  // the last holds at least 24 bytes: t + 2 < nb || (t + 2 == nb && last_n
  // >= 24).  A prefix of the launch's blocks: when t is one, so is t - 1.
  const uint32_t nbg = nb + (last_n >= 24 ? 1u : 0u);
  auto full = [&](uint32_t t) { return kAligned && t + 2 < nbg; };
  TileKeys K;
  RecBatch B;
  // (the block's bytes by a pointer that steps, so that `in` is not kept too)
  const uint8_t *src = in + (size_t)t0 * kBlk;
  for (uint32_t t = t0; t < t1; ++t, src += kBlk) {
    const int lane = block_lane();
    // (the last block, t == nb - 1, told from nbg: nb itself is not kept
    // through the loop -- the kernel has no scalar register to spare)
    const int n = t + 1 + (last_n >= 24 ? 1u : 0u) == nbg ? (int)last_n : kBlk;
    if (full(t)) {
      // the run's first block waits for its own loads; every other finds its
      // dwords in K, loaded during the block before (which was full too).
      // The next block is prefetched only when it is a full block itself
      // (otherwise this block's own dwords are loaded again, for nobody):
      // no byte is read that a one-block workgroup would not read
      if (t == t0) {
        load_keys(K, src, lane);
        keys_arrived(K);
        PROF_MARK(7);                    // wave start .. the first block's keys are here
      }
      const bool pf = kTileRun > 1 && t + 1 < t1 && full(t + 1);
      // (not prefetched = no kFull block follows in this run: the pending
      // records leave with this block's)
      encode_block<false, true>(S, kBlk, src, K, pf ? src + kBlk : src, nullptr, heads, ovfs,
                                status, lane, prof, B, !pf, bsizes, t);
    } else {
      // the last block (n <= 300: nothing may be read past the input), the one
      // before a last block of < 24 bytes, or an unaligned input: staged
      // bytewise, 16-B zero pad
      for (int i = lane; i < n; i += 64) S.buf[kInOff + i] = src[i];
      if (lane < 16) S.buf[kInOff + n + lane] = 0;
      wave_sync();
      if (t == t0) PROF_MARK(7);         // wave start .. the first block is staged
      encode_block<false, false>(S, n, nullptr, K, nullptr, nullptr, heads, ovfs, status, lane,
                                 prof, B, true, bsizes, t);
    }
    wave_sync();   // the next block's LDS writes stay behind this block's reads
  }
  PROF_FLUSH();
}

}  // namespace
