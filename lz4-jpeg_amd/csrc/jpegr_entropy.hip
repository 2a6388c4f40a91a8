// jpegr_entropy.hip -- the reference's JPEG entropy stage on MI355X:
// per tile and channel, RLE of the zigzagged ints and a per-stream Huffman
// code built exactly as the reference builds it, then the encoded bits; and
// the inverse (decode + inverse RLE).  Algorithms/sequential/JPEG/JPEG.c:
//   RLE                        :767-808   (count, value) ints
//   calculate_frequency        :864-886   symbols in first-occurrence order
//   heapify / build_heap       :895-936   min-heap on count (strict <, left first)
//   build_huffman_tree         :938-962   pop, pop, APPEND the merged node and
//                                          heapify its leaf index (a no-op: the
//                                          node is not sifted up)
//   assign_codes               :964-983   DFS, left '0' / right '1'
//   generate_encoded_sequence  :993-1007
//   decode_huffman             :1009-1033; inverse_RLE :810-840
// The reference keeps codes as char strings and the sequence as '0'/'1'
// chars; here the bits are packed MSB-first and the code table is the list of
// (value, code length) in the reference's codes[] (DFS) order -- leaves of a
// full binary tree listed left to right, so the codes follow from the lengths
// (code[k] = (code[k-1] + 1) shifted to len[k]; left-aligned they increase).
//
// Mapping: one LANE per stream (a stream's Huffman build is a few hundred
// dependent steps; a wave per stream would issue each serial step for 64
// lanes).  A workgroup is one wave holding 64 tiles' streams of ONE channel,
// so Y (64 ints, ~100 RLE symbols) and chroma (32 ints) never share a wave.
// The per-lane working set lives in LDS laid out dword-column-per-lane (every
// lane owns its bank whatever index it uses).  The fast encoder
// (entropy_encode_lane) maps symbols through a direct per-lane table, so its
// RLE + count walk does one LDS round trip per position instead of a probe
// chain per symbol, and keeps each emission's leaf ids in registers for the
// sequence pass: 0.25 -> 0.14 ms per 4K image.  (A wave-cooperative RLE and
// sequence -- one stream per wave step, ballots and LDS atomics -- measured
// 0.34 ms: 64 dependent steps per wave, same-address atomics serialised.)
// Streams with a symbol outside the table or more than 24 (luma) / 12
// (chroma) distinct symbols (random 4K tiles: Y <= 21, chroma <= 10) are
// encoded by the chroma kernel after its own streams, with the hashed
// encoder (room for 128) over the wave's LDS.  Two kernels per call: luma,
// then chroma.
// This file holds the slot path's kernel shells and host entry points.  The
// lane encoder's walk is jpegr_entropy_common.h's, shared with the encoder
// straight to a stream (jpegr_stream_enc.hip); the decoder's per-stream walk
// is jpegr_decode_common.h's, shared with the stream decoder
// (jpegr_stream.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../../include/jpegr.h"
#include "jpegr_decode_common.h"
#include "jpegr_entropy_common.h"

namespace {

template <bool kLuma>
__global__ __launch_bounds__(kLanes) void entropy_encode_lane(
    const int16_t *__restrict__ coef, size_t ntiles, uint8_t *__restrict__ bits,
    uint32_t *__restrict__ meta, uint32_t *__restrict__ table, uint32_t *__restrict__ lists,
    uint32_t *__restrict__ status) {
  constexpr int N = kLuma ? 64 : 32;
  using L = LaneLds<N>;
  constexpr int Cap = L::Cap;
  __shared__ L S;
  const int lane = threadIdx.x;
  const int c = kLuma ? 0 : 1 + (int)(blockIdx.x & 1);      // channel of this wave
  const size_t tile = (size_t)(kLuma ? blockIdx.x : blockIdx.x >> 1) * kLanes + lane;
  // (luma wave 0: the overflow count starts here; every later count is
  // added by the chroma kernel)
  if (kLuma && blockIdx.x == 0 && lane == 0) status[0] = 0;
  if (tile >= ntiles) return;
  // luma wave v's list and word (see the scratch layout above)
  const size_t lv = kLuma ? blockIdx.x : blockIdx.x >> 1;
  const size_t nlw = (ntiles + kLanes - 1) / kLanes;
  uint32_t *const lst = lists + lv * kLanes;
  uint32_t *const lword = lists + nlw * kLanes + lv;
  auto colp = [&](uint32_t *row0) { return reinterpret_cast<uint8_t *>(row0 + lane); };
  uint8_t *const tabc = colp(&S.tab[0][0]);
  using HeapCol = typename std::conditional<L::Wide, WCol, LCol<uint16_t>>::type;
  const LaneWork<HeapCol> w{{colp(&S.sym[0][0])}, {colp(&S.heap[0][0])},
                            {colp(&S.tab[L::CodeRow][0])}, {colp(&S.tab[0][0])},
                            {colp(&S.heap[0][0])}};

  // ---- RLE (JPEG.c:767-808) + frequencies (JPEG.c:864-886) ------------------
  uint32_t lid[(N + 2) / 3];             // per position: (leaf_c + 1) | (leaf_v + 1) << 5
  const auto [U, R, defer] = lane_rle_count<N>(coef + tile * 128 + coef_off(c), tabc, w.heap.p, lid);
  uint64_t dm = 0;                                    // (luma) the wave's deferred lanes
  if constexpr (kLuma) {
    const uint64_t act = __ballot(1);
    dm = __ballot(defer);
    if (defer) lst[__popcll(dm & ((1ull << lane) - 1ull))] = (uint32_t)(tile * 3 + c);
    if (dm == act) {                                  // (no lane left to report at the end)
      if (lane == __builtin_ctzll(act)) *lword = (uint32_t)__popcll(dm);
      return;
    }
    if (defer) return;
  } else {
    dm = __ballot(defer);                             // encoded below, after the fast path
  }
  if (!defer) {                                       // (luma: every lane left)
    uint32_t h0[Cap];                                   // heap entry u: count << 8 | u
    lane_heap_seed<N>(w.heap.p, w.sym.p, h0);

    // ---- heap, tree and codes (JPEG.c:913-983): the table is dead ------------
    bool over = tree_codes<Cap>(w, U, table + tile * kTablePerTile + bits_off(c), h0);

    // ---- encoded sequence, MSB-first (JPEG.c:993-1007) ------------------------
    uint8_t *const sout = bits + tile * kBitsPerTile + bits_off(c);
    constexpr int nwords = N / 2;                       // bits_cap / 32
    // the bit rows lie past the code table, through the dead heap and
    // symbols; two spill rows take the bits of a stream that overflows its slot
    const LCol<uint32_t> codez{colp(&S.tab[L::ZeroRow][0])};
    constexpr int BitRow = L::CodeRow + Cap;
    static_assert(BitRow + nwords + 2 <= L::Keys / 4 + L::HeapRows + Cap / 4 &&
                      offsetof(L, heap) == sizeof(S.tab) && offsetof(L, sym) == offsetof(L, heap) + sizeof(S.heap),
                  "the bit rows fit the dead rows past the codes");
    uint8_t *const brow = reinterpret_cast<uint8_t *>(&S) + BitRow * (4 * kLanes) + 4 * lane;
    auto bit_row = [&](int r) { return reinterpret_cast<uint32_t *>(brow + r * (4 * kLanes)); };
    const int nbits = lane_sequence<N, 2>(lid, codez, brow, 0);
    if (nbits > ref_bits_max(c)) over = true;           // char sequence[1024] / [512]
    // the slot's words, MSB-first bytes (16-B stores when the slot is aligned)
    {
      uint32_t wv[nwords];
#pragma unroll
      for (int r = 0; r < nwords; ++r) wv[r] = __builtin_bswap32(*bit_row(r));
      if ((reinterpret_cast<uintptr_t>(bits) & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < nwords / 4; ++k)
          reinterpret_cast<uint4 *>(sout)[k] = make_uint4(wv[4 * k], wv[4 * k + 1], wv[4 * k + 2], wv[4 * k + 3]);
      } else {
#pragma unroll
        for (int r = 0; r < nwords; ++r) reinterpret_cast<uint32_t *>(sout)[r] = wv[r];
      }
    }
    meta[tile * 3 + c] = (uint32_t)(nbits < 0xFFFF ? nbits : 0xFFFF) | ((uint32_t)R << 16) |
                         ((uint32_t)U << 24);
    if constexpr (kLuma) {
      const uint64_t om = __ballot(over);
      if (lane == __builtin_ctzll(__ballot(1)))
        *lword = (uint32_t)__popcll(dm) | (uint32_t)__popcll(om) << 8;
    } else if (over) {
      atomicAdd(&status[0], 1u);
    }
  }
  if constexpr (!kLuma) {
    // Deferred streams (a symbol outside the table or more than Cap
    // distinct): the hashed encoder over this wave's LDS, which the fast path
    // has left dead -- the wave's own, then (an even wave) those of luma wave
    // lv, whose overflowed lanes it counts.  The dead LDS holds kSlots
    // working sets, so lanes 0 .. kSlots-1 each take every kSlots-th stream
    // of the list (a 4K image whose every luma stream defers: 15.97 ms with
    // one lane, 2.50 ms with 6; profiles/r06_ent_defer_defer_y.log).
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    constexpr int kSetB = (kEnd + 15) & ~15;                // one working set, 16-B aligned
    constexpr int kSlots = (int)sizeof(L) / kSetB < 8 ? (int)sizeof(L) / kSetB : 8;
    static_assert(kSlots >= 1, "the hashed encoder's arrays fit the wave's LDS");
    const uint32_t lw = (blockIdx.x & 1) ? 0u : *lword;
    const int nown = __popcll(dm), n = nown + (int)(lw & 255u);
    if (lane == 0 && (lw >> 8)) atomicAdd(&status[0], lw >> 8);
    // (the last wave's lanes past ntiles have returned: only live lanes take a share)
    const int nlive = (int)min((size_t)kLanes, ntiles - lv * kLanes);
    const int slots = kSlots < nlive ? kSlots : nlive;
    if (lane < slots && lane < n) {
      uint8_t *const lb = reinterpret_cast<uint8_t *>(&S) + lane * kSetB;
      const Work<GColT> ws = hashed_work(lb);
      uint64_t own = dm;                              // the wave's own deferred lanes, in order
      for (int j = 0; j < lane && own; ++j) own &= own - 1;
      for (int k = lane; k < n; k += slots) {
        uint32_t sid;                                 // tile * 3 + channel
        if (k < nown) {
          sid = (uint32_t)((lv * kLanes + __builtin_ctzll(own)) * 3 + c);
          for (int j = 0; j < slots && own; ++j) own &= own - 1;
        } else {
          sid = lst[k - nown];
        }
        const size_t t = sid / 3;
        const int cc = (int)(sid % 3);
        const int rc = encode_stream<kFullCap, 2 * kFullCap>(
            coef + t * 128 + coef_off(cc), stream_len(cc), ws,
            bits + t * kBitsPerTile + bits_off(cc), bits_cap(cc), ref_bits_max(cc),
            table + t * kTablePerTile + bits_off(cc), meta + t * 3 + cc);
        if (rc != kOk) atomicAdd(&status[0], 1u);
      }
    }
  }
}

// ---- decode ------------------------------------------------------------------

// One wave's 64 tiles of one channel group: luma (a lane decodes its tile's
// Y stream) or chroma (its Cr, then its Cb stream).
template <bool kLuma>
__device__ __forceinline__ void decode_wave(DecLds<kLuma ? 64 : 32, kLuma ? kFastCap : kChromaCap> &S,
                                            int lane, size_t group,
                                            const uint8_t *__restrict__ bits,
                                            const uint32_t *__restrict__ meta,
                                            const uint32_t *__restrict__ table, size_t ntiles,
                                            int16_t *__restrict__ coef,
                                            uint32_t *__restrict__ status, uint32_t tag) {
  constexpr int Cap = kLuma ? kFastCap : kChromaCap;
  const size_t tile = group * kLanes + lane;
  if (tile >= ntiles) return;
  uint32_t fails = 0;
  int16_t *o = S.out[lane];                         // the ints, collected in LDS (store_ints)
  const VRow vl{reinterpret_cast<uint8_t *>(&S.vl[0][lane])};
#pragma unroll 1
  for (int c = kLuma ? 0 : 1; c <= (kLuma ? 0 : 2); ++c) {
    const uint32_t m = meta[tile * 3 + c];
    const uint8_t *b = bits + tile * kBitsPerTile + bits_off(c);
    const uint32_t *t = table + tile * kTablePerTile + bits_off(c);
    // the table's first Cap entries and the first two 16-B chunks of the
    // bits, loaded with the meta word (all inside the stream's slots, whatever
    // the meta word says): one wait, where a load per code under its k < U
    // test was waited for code by code
    uint32_t tb[Cap];
#pragma unroll
    for (int i = 0; i < Cap / 4; ++i) {
      const uint4 v = reinterpret_cast<const uint4 *>(t)[i];
      tb[4 * i] = v.x;
      tb[4 * i + 1] = v.y;
      tb[4 * i + 2] = v.z;
      tb[4 * i + 3] = v.w;
    }
    const uint4 q0 = reinterpret_cast<const uint4 *>(b)[0];
    const uint4 q1 = reinterpret_cast<const uint4 *>(b)[1];
    const int U = (int)(m >> 24);
    const int n = stream_len(c);
    // a foreign or corrupted meta word must not index past the stream's
    // slot: its bits (bits_cap bits) and its table (2 n entries: RLE of n ints)
    const bool sane = (int)(m & 0xFFFF) <= bits_cap(c) && U <= 2 * n;
    bool ok = false;
    if (!sane)  // a use on this path too, so the loads are not sunk past the meta test
      asm volatile("" ::"v"(tb[0]), "v"(q0.x), "v"(q1.x));
    if (sane) {
      const int r = U <= Cap ? decode_stream<Cap, SlotBits>(m, tb, vl, o, n,
                                                   kLuma ? &S.bm[0][lane] : nullptr, b, q0, q1)
                             : -1;
      const SlotTable slow{reinterpret_cast<const uint32_t *>(b), t, (int)(m & 0xFFFF)};
      ok = r < 0 ? decode_stream_slow(slow, m, o, n) : r != 0;
    } else {
      for (int j = 0; j < n; ++j) o[j] = 0;
    }
    fails += !ok;
    store_ints(o, coef + tile * 128 + coef_off(c), n);
  }
  // the wave's malformed streams, added to status[1] once workgroup 0 has
  // zeroed it for this call (status[2] = the call's tag; see the kernel)
  const uint32_t f = wave_rejected(fails);
  if (f && lane == __builtin_ctzll(__ballot(1))) {
    for (int spin = 0; spin < (1 << 22) &&
                       __hip_atomic_load(&status[2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != tag;
         ++spin)
      __builtin_amdgcn_s_sleep(2);
    atomicAdd(&status[1], f);
  }
}

// A workgroup is two waves over the same 64 tiles: wave 0 decodes their luma
// streams, wave 1 their chroma streams, each in its own LDS (12 + 6.4 KB: a
// 4K image's 2,025 workgroups are all resident at once, a luma and a chroma
// wave beside each other on every SIMD).  One launch: the luma and chroma
// kernels side by side on two streams started the chroma waves 8 us late and
// paid the fork and join.
// status[1] is zeroed here, not by a memset ahead of the launch (a dispatch
// and its gap): workgroup 0, dispatched first and waiting on nothing, zeroes
// it and then publishes the call's tag in status[2]; a wave with malformed
// streams adds them only once it reads that tag (bounded spin), so no add
// can precede the zero.
__global__ __launch_bounds__(2 * kLanes) void entropy_decode_kernel(
    const uint8_t *__restrict__ bits, const uint32_t *__restrict__ meta,
    const uint32_t *__restrict__ table, size_t ntiles, int16_t *__restrict__ coef,
    uint32_t *__restrict__ status, uint32_t tag) {
  __shared__ DecLds<64, kFastCap> SY;
  __shared__ DecLds<32, kChromaCap> SC;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status[1] = 0u;
    __threadfence();
    __hip_atomic_store(&status[2], tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int lane = threadIdx.x & (kLanes - 1);
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) < kLanes)
    decode_wave<true>(SY, lane, blockIdx.x, bits, meta, table, ntiles, coef, status, tag);
  else
    decode_wave<false>(SC, lane, blockIdx.x, bits, meta, table, ntiles, coef, status, tag);
}

// one tag per decode call (status[2]); 0 is skipped, so a zeroed status
// never matches
std::atomic<uint32_t> g_decode_tag{0};

}  // namespace

// the luma waves' deferred lists and words (the scratch layout above)
extern "C" size_t jpegr_entropy_scratch_bytes(size_t ntiles) {
  return (ntiles + kLanes - 1) / kLanes * (kLanes + 1) * sizeof(uint32_t);
}

extern "C" int jpegr_entropy_encode_device(const void *d_coef, size_t ntiles, void *d_bits,
                                           void *d_meta, void *d_table, void *d_scratch,
                                           void *d_status, void *stream) {
  if (!d_coef || !d_bits || !d_meta || !d_table || !d_scratch || !d_status || ntiles == 0 ||
      ntiles > ((size_t)1 << 32) / 3 || (reinterpret_cast<uintptr_t>(d_coef) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_bits) & 3) != 0)
    return JPEGR_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto *lists = static_cast<uint32_t *>(d_scratch);
  auto *status = static_cast<uint32_t *>(d_status);
  const unsigned groups = (unsigned)((ntiles + kLanes - 1) / kLanes);
  // (one stream: side by side, as the decoder runs, measured 0.140 -> 0.146 ms
  // per 4K image -- the encoder's luma and chroma waves contend for the same
  // LDS and issue slots, and the fork / join costs more than it overlaps)
  hipLaunchKernelGGL(entropy_encode_lane<true>, dim3(groups), dim3(kLanes), 0, s,
                     static_cast<const int16_t *>(d_coef), ntiles, static_cast<uint8_t *>(d_bits),
                     static_cast<uint32_t *>(d_meta), static_cast<uint32_t *>(d_table), lists,
                     status);
  hipLaunchKernelGGL(entropy_encode_lane<false>, dim3(groups * 2), dim3(kLanes), 0, s,
                     static_cast<const int16_t *>(d_coef), ntiles, static_cast<uint8_t *>(d_bits),
                     static_cast<uint32_t *>(d_meta), static_cast<uint32_t *>(d_table), lists,
                     status);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

extern "C" int jpegr_entropy_decode_device(const void *d_bits, const void *d_meta,
                                           const void *d_table, size_t ntiles, void *d_coef,
                                           void *d_status, void *stream) {
  if (!d_bits || !d_meta || !d_table || !d_coef || !d_status || ntiles == 0 ||
      ntiles > ((size_t)1 << 32) / 3 || (reinterpret_cast<uintptr_t>(d_coef) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_bits) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_table) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(d_status) & 3) != 0)
    return JPEGR_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t tag = ++g_decode_tag;
  if (tag == 0) tag = ++g_decode_tag;
  const unsigned groups = (unsigned)((ntiles + kLanes - 1) / kLanes);
  hipLaunchKernelGGL(entropy_decode_kernel, dim3(groups), dim3(2 * kLanes), 0, s,
                     static_cast<const uint8_t *>(d_bits), static_cast<const uint32_t *>(d_meta),
                     static_cast<const uint32_t *>(d_table), ntiles, static_cast<int16_t *>(d_coef),
                     static_cast<uint32_t *>(d_status), tag);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
