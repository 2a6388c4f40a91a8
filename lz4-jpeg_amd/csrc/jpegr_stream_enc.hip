// jpegr_stream_enc.hip -- the entropy encoder straight to a JPR1 / JPT1
// stream (format: include/jpegr.h), with no slots: the bytes of
// jpegr_entropy_encode_device followed by jpegr_pack_device or
// jpegr_pack_tight_device, from a scratch of the stream's own size.
//
//   jps_init           the call's own first launch: bump counters and result
//                      words to 0
//   stream_encode_lane jpegr_entropy.hip's lane-per-stream kernels (luma,
//                      then chroma with the deferred streams; the walk itself
//                      -- RLE + counts, heap seed, tree, sequence pass -- is
//                      jpegr_entropy_common.h's) with another sink: a lane's
//                      finished stream -- header, table in the format's coding,
//                      bit bytes -- lies in its LDS column as whole dwords; a
//                      wave scan of the dword counts and one atomicAdd per wave
//                      on a bump counter place it in a dense arena, and a
//                      directory entry per stream (arena dword | byte size)
//                      says where.  A stream that does not fit the arena is
//                      dropped, its size still recorded.
//   jps_sizes          a lane per tile: record size -> u32 (scan input), the
//                      u16 index, the 16-B header
//   lz4_scan_reduce / lz4_scan_partials (lz4r_scan.h, as they are)
//   jps_place          jpr_pack_emit's run of 16 tiles, LDS image of their
//                      output range and flush (jpegr_pack_common.h: run_of,
//                      image_out), each stream read from its arena position
//   jps_repair         exits at once unless the first pass dropped a stream
//                      (cap is short of the stream): then a dropped stream
//                      of a tile that starts below cap is encoded again, by
//                      one lane with the hashed encoder, straight to d_out
// Arena order varies from run to run; offsets come from the scan of the
// sizes, so the output bytes do not.  No workgroup waits for another, no
// host-side state, no host read-back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/jpegr.h"
#include "jpegr_entropy_common.h"
#include "jpegr_pack_common.h"

namespace {

constexpr uint64_t kDropped = (1ull << 48) - 1;       // a directory entry's arena dword: none

// Control words in the scratch (u64 each): kShards bump counters, 64 B apart,
// each over its own share of the arena.  A 4K image's 6,075 waves finish
// within a few microseconds of each other, and their atomics on one address
// are served one after another (measured: the chroma launch 70 us with one
// counter, 37 us with 16).  A share that fills up drops streams
// as a full arena does.
constexpr int kShards = 16;
constexpr int kDrops = 8 * kShards;                   // then: the streams dropped
constexpr int kCtrlWords = kDrops + 8;

// scratch: [scan: partials, tile sizes, group sums][control][directory: 3 u64
// per tile][per luma wave: 64 deferred lanes, then a word per luma wave][arena]
struct EncScratch {
  Scratch scan;
  uint64_t *ctrl, *dir;
  uint32_t *lists, *arena;
  uint64_t arena_dwords;
  size_t bytes;
};

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// The arena holds a stream that fits cap with every stream padded to whole
// dwords (9 B per tile) and some room for the shares' imbalance.  What does
// not fit is dropped, and place makes up for it where it matters.
inline EncScratch enc_scratch_of(void *base, size_t ntiles, size_t cap) {
  EncScratch s;
  auto *p = static_cast<uint8_t *>(base);
  s.scan = scratch_of(p, ntiles);
  size_t o = up16(s.scan.bytes);
  s.ctrl = reinterpret_cast<uint64_t *>(p + o);
  o += kCtrlWords * 8;
  s.dir = reinterpret_cast<uint64_t *>(p + o);
  o += up16(ntiles * 24);
  s.lists = reinterpret_cast<uint32_t *>(p + o);
  o += up16((ntiles + kLanes - 1) / kLanes * (kLanes + 1) * 4);
  s.arena = reinterpret_cast<uint32_t *>(p + o);
  const size_t bound = (size_t)kHdr + ntiles * (2 + (size_t)kRecMax);
  const size_t arena_b = up16(std::min(cap, bound) + 12 * ntiles + 1040);
  s.arena_dwords = arena_b / 4;
  s.bytes = o + arena_b;
  return s;
}

__global__ void jps_init(uint64_t *__restrict__ ctrl, uint64_t *__restrict__ result) {
  for (int i = threadIdx.x; i < kCtrlWords; i += blockDim.x) ctrl[i] = 0;
  if (threadIdx.x < 2) result[threadIdx.x] = 0;
}

// One working set of the hashed encoder (jpegr_entropy_common.h) and, behind
// it, what the slot encoder writes to global slots: the stream's bits, table
// and meta word.
constexpr int kBitsO = (kEnd + 3) & ~3, kTabO = kBitsO + 128, kMetaO = kTabO + 4 * kFullCap;
constexpr int kSetB = (kMetaO + 4 + 15) & ~15;          // 16-B aligned

// a stream the hashed encoder has left in a working set: what pack copies of
// it (codes and bits clamped to the slot), its table's mode and its bytes
struct Hashed {
  int rc;
  uint32_t m, nc, nb, mode, tb, size;
};

__device__ __forceinline__ Hashed hashed_encode(const int16_t *__restrict__ coef, size_t t, int cc,
                                                uint8_t *lb, bool tight) {
  const Work<GColT> ws = hashed_work(lb);
  uint32_t *const stab = reinterpret_cast<uint32_t *>(lb + kTabO);
  Hashed e;
  e.rc = encode_stream<kFullCap, 2 * kFullCap>(coef + t * 128 + coef_off(cc), stream_len(cc), ws,
                                               lb + kBitsO, bits_cap(cc), ref_bits_max(cc), stab,
                                               reinterpret_cast<uint32_t *>(lb + kMetaO));
  e.m = *reinterpret_cast<const uint32_t *>(lb + kMetaO);
  e.nc = meta_codes(e.m, cc);
  e.nb = meta_bits(e.m, cc);
  e.mode = 0;
  if (tight) {
    bool lng = false, wide = false;
    for (uint32_t i = 0; i < e.nc; ++i) {
      lng = lng || long_len(stab[i]);
      wide = wide || wide_val(stab[i]);
    }
    e.mode = table_mode(e.nc, lng, wide);
  }
  e.tb = table_bytes(e.nc, e.mode);
  e.size = 4u + e.tb + ((e.nb + 7u) >> 3);
  return e;
}

// the stream's e.size bytes to d (global or LDS), one by one
__device__ __forceinline__ void put_stream(uint8_t *d, const Hashed &e, const uint8_t *lb) {
  const uint32_t *const stab = reinterpret_cast<const uint32_t *>(lb + kTabO);
  const uint32_t hw = stream_header((e.m >> 16) & 255u, e.nc, e.nb, e.mode);
  for (uint32_t i = 0; i < 4; ++i) d[i] = (uint8_t)(hw >> (8 * i));
  uint8_t *p = d + 4;
  if (e.mode == 0u) {
    for (uint32_t i = 0; i < e.nc; ++i) {
      const uint32_t x = stab[i];
      p[3 * i] = (uint8_t)x;
      p[3 * i + 1] = (uint8_t)(x >> 8);
      p[3 * i + 2] = (uint8_t)(x >> 16);
    }
  } else {
    for (uint32_t i = 0; i < e.nc; i += 2) {
      const uint32_t up = i + 1 < e.nc ? (stab[i + 1] >> 16) & 15u : 0u;
      p[i >> 1] = (uint8_t)(((stab[i] >> 16) & 15u) | up << 4);
    }
    p += (e.nc + 1u) >> 1;
    for (uint32_t i = 0; i < e.nc; ++i) {
      const uint32_t x = stab[i];
      if (e.mode == 1u) {
        p[i] = (uint8_t)x;
      } else {
        p[2 * i] = (uint8_t)x;
        p[2 * i + 1] = (uint8_t)(x >> 8);
      }
    }
  }
  p = d + 4 + e.tb;
  const uint32_t nby = (e.nb + 7u) >> 3;
  for (uint32_t i = 0; i < nby; ++i) p[i] = lb[kBitsO + i];
}

struct EncArgs {
  const int16_t *coef;
  size_t ntiles, wg_base;
  uint64_t *dir;
  uint32_t *arena;
  uint64_t arena_dwords;
  uint64_t shard_dwords;              // the first pass: a counter's share of the arena
  uint32_t shards;                    // ... and the counters in use (<= kShards)
  uint64_t *ctrl;
  uint32_t *lists;
  unsigned long long *over;           // result[1]: streams past the reference's buffers
};

// jpegr_entropy.hip's entropy_encode_lane (its comments hold here) with the
// stream's bytes as the product.  Differences: no lane leaves before the
// wave's scan (a lane past ntiles, a lane the repair pass skips and a
// deferred lane run on with size 0); the table comes back in registers; the
// sequence pass starts at the byte phase the header and table leave, so the
// bit rows are the stream's dwords as they are, and header and table bytes are
// stored into the rows in front of them (the dead codes).
template <bool kLuma, bool kTight>
__global__ __launch_bounds__(kLanes) void stream_encode_lane(const EncArgs a) {
  constexpr int N = kLuma ? 64 : 32;
  using L = LaneLds<N>;
  constexpr int Cap = L::Cap;
  __shared__ L S;
  const int lane = threadIdx.x;
  const size_t bx = a.wg_base + blockIdx.x;
  const int c = kLuma ? 0 : 1 + (int)(bx & 1);              // channel of this wave
  const size_t lv = kLuma ? bx : bx >> 1;                   // the luma wave of these tiles
  const size_t tile = lv * kLanes + lane;
  const size_t ntiles = a.ntiles;
  if (lv * kLanes >= ntiles) return;
  const bool skip = tile >= ntiles;
  const size_t tl = skip ? ntiles - 1 : tile;               // (a skipped lane walks a live tile)
  const size_t nlw = (ntiles + kLanes - 1) / kLanes;
  uint32_t *const lst = a.lists + lv * kLanes;
  uint32_t *const lword = a.lists + nlw * kLanes + lv;
  // this wave's counter and its share [lo, hi) of the arena (dwords)
  const uint32_t shard = (uint32_t)(bx % a.shards);
  unsigned long long *const bump = reinterpret_cast<unsigned long long *>(a.ctrl + 8 * shard);
  const uint64_t lo = shard * a.shard_dwords, hi = lo + a.shard_dwords;
  auto colp = [&](uint32_t *row0) { return reinterpret_cast<uint8_t *>(row0 + lane); };
  uint8_t *const tabc = colp(&S.tab[0][0]);
  using HeapCol = typename std::conditional<L::Wide, WCol, LCol<uint16_t>>::type;
  const LaneWork<HeapCol> w{{colp(&S.sym[0][0])}, {colp(&S.heap[0][0])},
                            {colp(&S.tab[L::CodeRow][0])}, {colp(&S.tab[0][0])},
                            {colp(&S.heap[0][0])}};

  // ---- RLE (JPEG.c:767-808) + frequencies (JPEG.c:864-886) ------------------
  uint32_t lid[(N + 2) / 3];             // per position: (leaf_c + 1) | (leaf_v + 1) << 5
  const LaneRle rl = lane_rle_count<N>(a.coef + tl * 128 + coef_off(c), tabc, w.heap.p, lid);
  const int U = rl.U, R = rl.R;
  const bool defer = rl.defer && !skip;
  const uint64_t dm = __ballot(defer);                // the wave's deferred lanes
  if constexpr (kLuma) {
    // the chroma kernel's even wave 2 lv encodes them: the lane numbers
    if (defer) lst[__popcll(dm & ((1ull << lane) - 1ull))] = (uint32_t)lane;
  }

  // what the lane hands to the wave: its stream as nd dwords from LDS row
  // pointer src (row r at src + 64 r), sb bytes of them live
  uint32_t nd = 0, sb = 0;
  const uint32_t *src = &S.tab[0][lane];
  bool over = false;
  if (!defer && !skip) {
    uint32_t h0[Cap];                                   // heap entry u: count << 8 | u
    lane_heap_seed<N>(w.heap.p, w.sym.p, h0);

    // ---- heap, tree and codes (JPEG.c:913-983): the table into registers ------
    uint32_t tbl[Cap];
#pragma unroll
    for (int k = 0; k < Cap; ++k) tbl[k] = 0u;
    over = tree_codes<Cap>(w, U, tbl, h0);
    // The format's table coding.  The fast path's symbols are int8 (the key
    // range), so a JPT1 stream is mode 1 unless a length passes a nibble.
    uint32_t lmax = 0;
#pragma unroll
    for (int k = 0; k < Cap; ++k) lmax = max(lmax, tbl[k] >> 16);
    const uint32_t mode = (kTight && lmax <= 15u) ? 1u : 0u;
    const uint32_t tb = table_bytes((uint32_t)U, mode);
    const uint32_t q = (4u + tb) >> 2, ph = tb & 3u;    // the bits start at byte ph of dword q

    // ---- encoded sequence, MSB-first (JPEG.c:993-1007) ------------------------
    constexpr int nwords = N / 2;                       // bits_cap / 32
    const LCol<uint32_t> codez{colp(&S.tab[L::ZeroRow][0])};
    constexpr int BitRow = L::CodeRow + Cap;
    // rows 0 .. nwords hold the slot's bits behind up to 3 B of phase; two
    // spill rows take the bits of a stream that overflows its slot
    static_assert(BitRow + nwords + 3 <= L::Keys / 4 + L::HeapRows + Cap / 4 &&
                      offsetof(L, heap) == sizeof(S.tab) && offsetof(L, sym) == offsetof(L, heap) + sizeof(S.heap),
                  "the bit rows fit the dead rows past the codes");
    static_assert(1 + (3 * Cap + 3) / 4 <= BitRow, "header and table fit the rows before the bits");
    uint8_t *const brow = reinterpret_cast<uint8_t *>(&S) + BitRow * (4 * kLanes) + 4 * lane;
    const int nbits = lane_sequence<N, 3>(lid, codez, brow, (int)(8u * ph)) - (int)(8u * ph);
    if (nbits > ref_bits_max(c)) over = true;           // char sequence[1024] / [512]
    const uint32_t nb = (uint32_t)min(nbits, bits_cap(c));   // what the slot would hold

    // ---- header and table, into the rows before the bits (the codes are dead).
    // A row is a big-endian word, as the bit rows are: stream byte b of the
    // lane is byte 3 - (b & 3) of row b / 4 counted from row BitRow - q.
    uint8_t *const hb = brow - q * (4 * kLanes);
    auto sbyte = [&](uint32_t b) -> uint8_t & { return hb[(b >> 2) * (4 * kLanes) + (3u - (b & 3u))]; };
    *reinterpret_cast<uint32_t *>(hb) = __builtin_bswap32(stream_header((uint32_t)R, (uint32_t)U, nb, mode));
    if (mode == 0u) {
#pragma unroll
      for (int k = 0; k < Cap; ++k)
        if (k < U) {
          sbyte(4u + 3u * k) = (uint8_t)tbl[k];
          sbyte(5u + 3u * k) = (uint8_t)(tbl[k] >> 8);
          sbyte(6u + 3u * k) = (uint8_t)(tbl[k] >> 16);
        }
    } else {
      const uint32_t vb = 4u + (((uint32_t)U + 1u) >> 1);
#pragma unroll
      for (int k = 0; k < Cap; ++k)
        if (k < U) {
          // (entry k + 1 past U holds 0; Cap is even)
          if ((k & 1) == 0)
            sbyte(4u + (k >> 1)) =
                (uint8_t)(((tbl[k] >> 16) & 15u) | ((tbl[k | 1] >> 16) & 15u) << 4);
          sbyte(vb + k) = (uint8_t)tbl[k];
        }
    }
    sb = 4u + tb + ((nb + 7u) >> 3);
    nd = (sb + 3u) >> 2;
    src = reinterpret_cast<const uint32_t *>(hb);
  }

  // ---- the wave's place in the arena: a scan of the dword counts, one bump ----
  const uint32_t incl = wave_incl_add(nd);
  const uint32_t total = lane63(incl);
  const uint32_t ndmax = lane63(wave_incl_max(nd));
  if (total) {
    unsigned long long b0 = 0;
    if (lane == 0) b0 = atomicAdd(bump, (unsigned long long)total);
    const uint64_t base = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b0) |
                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b0 >> 32)) << 32;
    const uint64_t at = lo + base + incl - nd;
    const bool fits = at + nd <= hi;
    if (nd) a.dir[tile * 3 + c] = (fits ? at : kDropped) << 16 | sb;
    if (nd && !fits) atomicAdd(reinterpret_cast<unsigned long long *>(a.ctrl + kDrops), 1ull);
    uint32_t *const dst = a.arena + (fits ? at : 0);
    for (uint32_t r = 0; r < ndmax; ++r)
      if (fits && r < nd) dst[r] = __builtin_bswap32(src[r * kLanes]);
  }
  if constexpr (kLuma) {
    const uint64_t om = __ballot(over);
    if (lane == 0) *lword = (uint32_t)__popcll(dm) | (uint32_t)__popcll(om) << 8;
  } else {
    if (over) atomicAdd(a.over, 1ull);
  }

  if constexpr (!kLuma) {
    // Deferred streams: the hashed encoder over this wave's LDS, which the
    // fast path has left dead -- the wave's own, then (an even wave) those of
    // luma wave lv, whose overflowed lanes it counts.  A working set carries
    // the stream's bits, table and meta word too (the slot encoder's global
    // slots), so the dead LDS holds kSlots of them; each stream takes a bump
    // of its own and its bytes go out one by one.
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    constexpr int kSlots = (int)sizeof(L) / kSetB < 8 ? (int)sizeof(L) / kSetB : 8;
    static_assert(kSlots >= 1, "the hashed encoder's arrays fit the wave's LDS");
    const uint32_t lw = (bx & 1) ? 0u : *lword;
    const int nown = __popcll(dm), n = nown + (int)(lw & 255u);
    if (lane == 0 && (lw >> 8)) atomicAdd(a.over, (unsigned long long)(lw >> 8));
    if (lane < kSlots && lane < n) {
      uint8_t *const lb = reinterpret_cast<uint8_t *>(&S) + lane * kSetB;
      uint64_t own = dm;                              // the wave's own deferred lanes, in order
      for (int j = 0; j < lane && own; ++j) own &= own - 1;
      for (int k = lane; k < n; k += kSlots) {
        size_t t;
        int cc;
        if (k < nown) {
          t = lv * kLanes + __builtin_ctzll(own);
          cc = c;
          for (int j = 0; j < kSlots && own; ++j) own &= own - 1;
        } else {
          t = lv * kLanes + (lst[k - nown] & 63u);
          cc = 0;
        }
        if (t >= ntiles) continue;
        const Hashed e = hashed_encode(a.coef, t, cc, lb, kTight);
        if (e.rc != kOk) atomicAdd(a.over, 1ull);
        const uint32_t dws = (e.size + 3u) >> 2;
        const uint64_t at = lo + atomicAdd(bump, (unsigned long long)dws);
        const bool fits = at + dws <= hi;
        a.dir[t * 3 + cc] = (fits ? at : kDropped) << 16 | e.size;
        if (fits) put_stream(reinterpret_cast<uint8_t *>(a.arena + at), e, lb);
        else atomicAdd(reinterpret_cast<unsigned long long *>(a.ctrl + kDrops), 1ull);
      }
    }
  }
}

// jpr_pack_sizes' job with the sizes from the directory
__global__ __launch_bounds__(256) void jps_sizes(const uint64_t *__restrict__ dir, size_t ntiles,
                                                 size_t t_base, uint32_t *__restrict__ tsz,
                                                 uint8_t *__restrict__ out, uint64_t cap,
                                                 uint32_t magic, uint32_t w, uint32_t h,
                                                 uint32_t nimg) {
  const size_t t = t_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t sz = (uint32_t)(dir[3 * t] & 0xFFFFu) + (uint32_t)(dir[3 * t + 1] & 0xFFFFu) +
                      (uint32_t)(dir[3 * t + 2] & 0xFFFFu);
  tsz[t] = sz;
  put_index(out, cap, t, sz);
  if (t == 0) put_header(out, cap, magic, w, h, nimg);
}

// jpr_pack_emit's run, LDS image and flush (jpegr_pack_common.h) with each
// stream read from the arena: a stream is whole dwords at a dword address, so
// lane l takes dword l (and l + 64, ...) of each of the tile's three streams,
// the first round of all four tiles in flight before any is stored.  Only
// tiles that start below cap are read: the others' bytes are clipped anyway.
// The bytes of a stream that the arena dropped are left as the image holds
// them; jps_repair writes them afterwards.  Workgroup 0 copies the length to
// the result.
__global__ __launch_bounds__(64 * kPW) void jps_place(
    const uint64_t *__restrict__ dir, const uint32_t *__restrict__ arena, uint64_t arena_dwords,
    size_t ntiles, size_t wg_base, const uint32_t *__restrict__ tsz,
    const uint32_t *__restrict__ gsum, const uint64_t *__restrict__ part,
    uint8_t *__restrict__ out, uint64_t cap, const uint64_t *__restrict__ out_len,
    uint64_t *__restrict__ result) {
  __shared__ uint64_t toff[kGT + 1];
  __shared__ alignas(16) uint8_t img[kImg];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t wg = wg_base + blockIdx.x;
  if (wg == 0 && tid == 0) result[0] = *out_len;
  const auto [g, t0, h0, ntl] = run_of(wg, ntiles);
  if (t0 >= ntiles) return;
  group_offsets(tid, g, ntiles, tsz, gsum, part, toff);
  __syncthreads();
  const uint64_t G0 = toff[h0], G1 = toff[h0 + ntl];
  if (G0 >= cap) return;
  const uint32_t lead = (uint32_t)(((uintptr_t)out + G0) & 15);   // img[lead] = stream byte G0

  uint32_t sz[kTW][3], first[kTW][3], live = 0;       // size; dword `lane`; the streams to copy
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    const int j = kTW * wv + i;
    const bool on = j < ntl && toff[h0 + (j < ntl ? j : 0)] < cap;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint64_t d = on ? dir[3 * (t0 + j) + c] : 0ull;
      // (a size past its stream's bound or an address past the arena cannot
      // come from the encoder: such an entry is not read)
      const uint32_t s = (uint32_t)(d & 0xFFFFu);
      const bool ok = s <= (c ? 260u : 516u) && (d >> 16) + ((s + 3u) >> 2) <= arena_dwords;
      sz[i][c] = s;
      live |= (ok ? 1u : 0u) << (3 * i + c);
      first[i][c] = 0u;
      if (ok && 4u * (uint32_t)lane < s) first[i][c] = arena[(d >> 16) + lane];
    }
  }
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    const int j = kTW * wv + i;
    if (j >= ntl) continue;
    uint32_t o = lead + (uint32_t)(toff[h0 + j] - G0);  // the stream's first image byte
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t s = (live >> (3 * i + c)) & 1u ? sz[i][c] : 0u;
      for (uint32_t dw = (uint32_t)lane; 4u * dw < s; dw += 64u) {
        // (past 256 B, one stream in many: its directory entry again)
        const uint32_t v = dw < 64u ? first[i][c] : arena[(dir[3 * (t0 + j) + c] >> 16) + dw];
        uint8_t *p = img + o + 4u * dw;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b)
          if (4u * dw + b < s) p[b] = (uint8_t)(v >> (8 * b));
      }
      o += sz[i][c];
    }
  }
  __syncthreads();
  image_out(img, tid, lane, wv, G0, G1, lead, out, cap);
}

// A wave per scan group, after place, and only when the first pass dropped
// streams: lanes 0 .. kRepairSets - 1 take the group's tiles in turn; a dropped
// stream of a tile that starts below cap is encoded again by the hashed
// encoder (any stream is within its reach, and its bytes are the fast
// encoder's) and written to the stream byte by byte, below cap.  Slow, and
// only when cap is short of the stream or a counter's share ran out.
constexpr int kRepairSets = 8;

__global__ __launch_bounds__(kLanes) void jps_repair(
    const uint64_t *__restrict__ dir, const int16_t *__restrict__ coef, size_t ntiles,
    size_t g_base, const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, const uint64_t *__restrict__ ctrl, bool tight,
    uint8_t *__restrict__ out, uint64_t cap) {
  __shared__ uint64_t toff[kGT + 1];
  __shared__ alignas(16) uint8_t sets[kRepairSets][kSetB];
  __shared__ alignas(16) uint8_t stage[kRepairSets][516];
  if (ctrl[kDrops] == 0) return;                        // uniform over the launch
  const int lane = threadIdx.x;
  const size_t g = g_base + blockIdx.x;
  if (g * kGT >= ntiles) return;
  const int nt = (int)min((size_t)kGT, ntiles - g * kGT);
  group_offsets(lane, g, ntiles, tsz, gsum, part, toff);
  __syncthreads();
  if (lane >= kRepairSets) return;
  for (int j = lane; j < nt && toff[j] < cap; j += kRepairSets) {
    uint64_t o = toff[j];
    for (int c = 0; c < 3; ++c) {
      const uint64_t d = dir[3 * (g * kGT + j) + c];
      const uint32_t s = (uint32_t)(d & 0xFFFFu);
      if ((d >> 16) == kDropped && s <= (c ? 260u : 516u) && o < cap) {
        const Hashed e = hashed_encode(coef, g * kGT + j, c, sets[lane], tight);
        if (e.size == s) {
          put_stream(stage[lane], e, sets[lane]);
          const uint32_t n = (uint32_t)min((uint64_t)s, cap - o);
          for (uint32_t i = 0; i < n; ++i) out[o + i] = stage[lane][i];
        }
      }
      o += s;
    }
  }
}

template <bool kTight>
void launch_encode(const EncArgs &a0, hipStream_t st) {
  EncArgs a = a0;
  const size_t groups = (a.ntiles + kLanes - 1) / kLanes;
  launch_chunks(groups, 1, [&](size_t b, unsigned n) {
    a.wg_base = b;
    hipLaunchKernelGGL((stream_encode_lane<true, kTight>), dim3(n), dim3(kLanes), 0, st, a);
  });
  launch_chunks(2 * groups, 1, [&](size_t b, unsigned n) {
    a.wg_base = b;
    hipLaunchKernelGGL((stream_encode_lane<false, kTight>), dim3(n), dim3(kLanes), 0, st, a);
  });
}

}  // namespace

extern "C" size_t jpegr_stream_encode_scratch_bytes(size_t ntiles, size_t cap) {
  return enc_scratch_of(nullptr, ntiles, cap).bytes;
}

extern "C" int jpegr_stream_encode_device(const void *d_coef, int w, int h, int nimg, int format,
                                          void *d_out, size_t cap, void *d_out_len,
                                          void *d_scratch, void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_coef || !d_out || !d_out_len || !d_scratch || !d_result || ntiles == 0 ||
      (format != JPEGR_STREAM_JPR1 && format != JPEGR_STREAM_JPT1) ||
      (reinterpret_cast<uintptr_t>(d_coef) & 15) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_out_len) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(d_scratch) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_result) & 7) != 0)
    return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool tight = format == JPEGR_STREAM_JPT1;
  const EncScratch s = enc_scratch_of(d_scratch, ntiles, cap);
  auto *out = static_cast<uint8_t *>(d_out);
  auto *result = static_cast<uint64_t *>(d_result);
  EncArgs a;
  a.coef = static_cast<const int16_t *>(d_coef);
  a.ntiles = ntiles;
  a.wg_base = 0;
  a.dir = s.dir;
  a.arena = s.arena;
  a.arena_dwords = s.arena_dwords;
  // a counter per four luma waves, so that a small input's shares still hold streams
  a.shards = (uint32_t)std::min((size_t)kShards, std::max((size_t)1, (ntiles + 4 * kLanes - 1) / (4 * kLanes)));
  a.shard_dwords = s.arena_dwords / a.shards;
  a.ctrl = s.ctrl;
  a.lists = s.lists;
  a.over = reinterpret_cast<unsigned long long *>(result + 1);
  hipLaunchKernelGGL(jps_init, dim3(1), dim3(64), 0, st, s.ctrl, result);
  if (tight) launch_encode<true>(a, st);
  else launch_encode<false>(a, st);
  launch_chunks(ntiles, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jps_sizes, dim3(n), dim3(256), 0, st, s.dir, ntiles, b * 256, s.scan.tsz, out,
                       (uint64_t)cap, tight ? kMagicJPT1 : kMagicJPR1, (uint32_t)w, (uint32_t)h,
                       (uint32_t)nimg);
  });
  scan(s.scan, ntiles, static_cast<uint64_t *>(d_out_len), st);
  launch_chunks(ntiles, kRun, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jps_place, dim3(n), dim3(64 * kPW), 0, st, s.dir, s.arena, s.arena_dwords, ntiles, b,
                       s.scan.tsz, s.scan.gsum, s.scan.part, out, (uint64_t)cap,
                       static_cast<const uint64_t *>(d_out_len), result);
  });
  launch_chunks(ntiles, kGT, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jps_repair, dim3(n), dim3(kLanes), 0, st, s.dir, a.coef, ntiles, b, s.scan.tsz,
                       s.scan.gsum, s.scan.part, s.ctrl, tight, out, (uint64_t)cap);
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
