// jpegr_entropy_common.h -- the entropy stage's constants and what its
// encoders share: the per-lane LDS columns, the reference's heap / tree / code
// build (tree_codes and its sifts), the hashed encoder of one stream
// (encode_stream) with its working set's layout, the lane kernels' LDS layout
// and their walk (lane_rle_count, lane_heap_seed, lane_sequence).
// jpegr_entropy.hip (the slot encoder) and jpegr_stream_enc.hip (the encoder
// straight to a JPR1 / JPT1 stream) each keep their own kernel shell around
// these: where the lanes leave, where the table goes, and everything after the
// sequence pass.  The decoders' side is jpegr_decode_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>


namespace {

constexpr int kLanes = 64;
constexpr int kFastCap = 24;             // distinct symbols in the LDS pass (luma)
constexpr int kChromaCap = 12;           // ... (chroma)
constexpr int kFullCap = 128;            // RLE of 64 ints: <= 128 symbols

// per-tile output layout
constexpr int kBitsPerTile = 256;        // bytes: [Y 128][Cr 64][Cb 64]
constexpr int kTablePerTile = 256;       // u32 entries: [Y 128][Cr 64][Cb 64]

__device__ __forceinline__ int stream_len(int c) { return c == 0 ? 64 : 32; }
__device__ __forceinline__ int coef_off(int c) { return c == 0 ? 0 : c == 1 ? 64 : 96; }
__device__ __forceinline__ int bits_off(int c) { return c == 0 ? 0 : c == 1 ? 128 : 192; }
__device__ __forceinline__ int bits_cap(int c) { return c == 0 ? 1024 : 512; }
// the reference's sequence buffers hold 1023 / 511 chars + NUL (JPEG.c:1248, :1286)
__device__ __forceinline__ int ref_bits_max(int c) { return c == 0 ? 1023 : 511; }

// Strided view of one lane's array: element i at p[i * stride].
template <typename T>
struct Col {
  T *p;
  int stride;
  __device__ __forceinline__ T &operator[](int i) const { return p[i * stride]; }
  __device__ __forceinline__ void clear(int n) const {
    for (int i = 0; i < n; ++i) p[i * stride] = 0;
  }
  // elements i, i + 1 (16-bit) as one word
  __device__ __forceinline__ uint32_t pair(int i) const {
    return (uint32_t)(uint16_t)p[i * stride] | ((uint32_t)(uint16_t)p[(i + 1) * stride] << 16);
  }
};

// One lane's array in LDS, dword-column layout: the lane owns dword column
// `lane` of a [rows][64] u32 block and packs 4 / sizeof(T) elements per
// dword, so every lane hits its own bank whatever index it uses (a plain
// [i][lane] byte column shares a dword between 4 lanes: up to 4-way
// conflicts under divergent indices).
template <typename T>
struct LCol {
  // Every access is type-punned over u32 storage (elements of 1, 2 or 4
  // bytes, pairs read as one dword): may_alias, or type-based alias analysis
  // lets the compiler move a dword read above a half-word store of the same
  // word (it did, once a sift was unrolled without branches).
  typedef T __attribute__((may_alias)) TA;
  typedef uint32_t __attribute__((may_alias)) WA;
  uint8_t *p;                                   // &block[0][lane] as bytes
  // (indices are never negative: unsigned division is a shift and a mask)
  __device__ __forceinline__ TA &operator[](int i) const {
    constexpr uint32_t per = 4 / sizeof(T);
    const uint32_t u = (uint32_t)i;
    return *reinterpret_cast<TA *>(p + (u / per) * (4 * kLanes) + (u % per) * sizeof(T));
  }
  // zero elements [0, n) (n a multiple of 4 / sizeof(T)): whole dwords
  __device__ __forceinline__ void clear(int n) const {
    constexpr int per = 4 / (int)sizeof(T);
    for (int i = 0; i < n / per; ++i) *reinterpret_cast<WA *>(p + i * (4 * kLanes)) = 0u;
  }
  // 16-bit elements i, i + 1 (i even: one dword, one LDS read)
  __device__ __forceinline__ uint32_t pair(int i) const {
    return *reinterpret_cast<const WA *>(p + (i / 2) * (4 * kLanes));
  }
};

// One lane's working set for a stream with at most Cap distinct symbols.
template <template <typename> class A>
struct Work {
  static constexpr bool kPackLen = false;
  static constexpr bool kTopDown = false;
  A<int16_t> sym;       // [Cap]       leaf -> symbol value (the int, without +1000)
  A<uint8_t> hash;      // [Hash]      open-addressing map symbol -> leaf + 1 (0 = empty)
  A<uint16_t> heap;     // [Cap + 2]   heap entry i (count << 8 | node id) at slot i + 1,
                        //             so that children 2i+1, 2i+2 share a dword; merged
                        //             node m's children (left | right << 8) at entry
                        //             U - 1 - m, the slot the heap frees as it shrinks
  A<uint32_t> code;     // [Cap]       leaf code bits (right-aligned)
  A<uint8_t> len;       // [Cap]       leaf code length
  A<uint16_t> stk;      // [Cap + 1]   DFS stack: node | depth << 8
};

// Sift x down from index i (JPEG.c:895-911: smallest of i, left, right by
// count with strict <, left tested first), moving children up into the hole
// -- the same final arrangement as the reference's swaps.  x is passed in
// registers (slot i is not read), and each LDS round trip serves two levels:
// the children pair and both grandchildren pairs are read together.  Slots
// past MaxSlot (the array's last even slot) are clamped: such a pair is never
// used.  Returns the entry left at index i (for the root: the new minimum).
template <int MaxSlot, class W>
__device__ __forceinline__ uint16_t sift(const W &w, int size, int i, uint16_t x) {
  const int cx = x >> 8;
  uint16_t top = x;
  bool moved = false;
  for (;;) {
    const int l = 2 * i + 1, r = l + 1;
    if (l >= size) break;
    const uint32_t pc = w.heap.pair(l + 1);               // entries l, r (slots l + 1, l + 2)
    const uint32_t pgl = w.heap.pair(min(2 * l + 2, MaxSlot));   // l's children
    const uint32_t pgr = w.heap.pair(min(2 * l + 4, MaxSlot));   // r's children
    const uint16_t hl = (uint16_t)pc, hr = (uint16_t)(pc >> 16);
    int s = i, cs = cx;
    uint16_t hs = x;
    if ((hl >> 8) < cs) { s = l; cs = hl >> 8; hs = hl; }
    if (r < size && (hr >> 8) < cs) { s = r; hs = hr; }
    if (s == i) break;
    w.heap[i + 1] = hs;
    if (!moved) top = hs;
    moved = true;
    i = s;
    const int l2 = 2 * i + 1;                             // the next level, prefetched
    if (l2 >= size) break;
    const uint32_t pg = s == l ? pgl : pgr;
    const uint16_t gl = (uint16_t)pg, gr = (uint16_t)(pg >> 16);
    int s2 = i, c2 = cx;
    uint16_t h2 = x;
    if ((gl >> 8) < c2) { s2 = l2; c2 = gl >> 8; h2 = gl; }
    if (l2 + 1 < size && (gr >> 8) < c2) { s2 = l2 + 1; h2 = gr; }
    if (s2 == i) break;
    w.heap[i + 1] = h2;
    i = s2;
  }
  w.heap[i + 1] = x;
  return top;
}

// The same sift for heaps of at most Cap <= 32 entries, branch-free: a fixed
// floor(log2(Cap)) levels (the deepest any sift can go), two per LDS round
// trip, a done flag instead of a break.  Once x has landed, the remaining
// levels rewrite x at its index (idempotent).  The loop form above paid the
// exec-mask bookkeeping of every lane's own exit at every level.
template <int Cap, int kDepth, class W>
__device__ __forceinline__ uint16_t sift_depth(const W &w, int size, int i, uint16_t x,
                                               int *fi = nullptr) {
  constexpr int kMaxSlot = Cap & ~1;
  static_assert(Cap <= 31 && kDepth >= 1 && kDepth <= 4, "fixed depth");
  // counts compare as whole entries against a count with a zero id byte
  // (strict <): e < (c << 8) iff e >> 8 < c
  const uint32_t xk = x & 0xFF00u;
  uint16_t top = x;
  bool done = false;
#pragma unroll
  for (int d = 0; d < kDepth; d += 2) {
    const int l = 2 * i + 1, r = l + 1;
    const uint32_t pc = w.heap.pair(min(l + 1, kMaxSlot));      // entries l, r
    const uint32_t pgl = w.heap.pair(min(2 * l + 2, kMaxSlot));  // l's children
    const uint32_t pgr = w.heap.pair(min(2 * l + 4, kMaxSlot));  // r's children
    {
      const uint32_t hl = pc & 0xFFFFu, hr = pc >> 16;
      const bool tl = l < size && hl < xk;
      const uint32_t ck = tl ? (hl & 0xFF00u) : xk;
      const bool tr = r < size && hr < ck;
      const bool mv = !done && (tl || tr);
      const uint16_t hs = (uint16_t)(tr ? hr : hl);
      if (d == 0) top = mv ? hs : x;
      w.heap[i + 1] = mv ? hs : x;
      done = !mv;
      i = mv ? (tr ? r : l) : i;
    }
    if (d + 1 < kDepth) {
      const uint32_t pg = i == r ? pgr : pgl;                 // (unused once done)
      const int l2 = 2 * i + 1, r2 = l2 + 1;
      const uint32_t gl = pg & 0xFFFFu, gr = pg >> 16;
      const bool tl = l2 < size && gl < xk;
      const uint32_t ck = tl ? (gl & 0xFF00u) : xk;
      const bool tr = r2 < size && gr < ck;
      const bool mv = !done && (tl || tr);
      w.heap[i + 1] = mv ? (uint16_t)(tr ? gr : gl) : x;
      done = !mv;
      i = mv ? (tr ? r2 : l2) : i;
    }
  }
  w.heap[i + 1] = x;
  if (fi) *fi = i;                                    // where x landed
  return top;
}

template <int Cap, class W>
__device__ __forceinline__ uint16_t sift_fixed(const W &w, int size, int i, uint16_t x) {
  constexpr int kDepth = Cap >= 16 ? 4 : Cap >= 8 ? 3 : Cap >= 4 ? 2 : 1;   // floor(log2 Cap)
  return sift_depth<Cap, kDepth>(w, size, i, x);
}

// The same with the depth cut to what a wave-uniform bound allows: no lane
// of the wave sifts more than `levels` levels (a uniform branch picks the
// unrolled depth).
// levels a sift from index i can descend in a heap of at most s entries
__host__ __device__ constexpr int sift_levels_bound(int s, int i) {
  int d = 0;
  for (int j = i; 2 * j + 1 < s; j = 2 * j + 1) ++d;
  return d;
}

// build_heap's sifts (JPEG.c:913-936) from index I down to 0, unrolled so
// that each sift's x is the entry's initial value from registers: a sift
// from a later index moves only entries of that index's subtree, which holds
// no earlier index.  Returns, through root, the entry left at index 0.
template <int Cap, int I, class W>
__device__ __forceinline__ void build_heap_from(const W &w, int umax, int U,
                                                const uint32_t *h0, uint16_t &root) {
  if constexpr (I >= 0) {
    if (I < umax / 2) {                                 // uniform
      if (I < U / 2) {
        // the depth of index I in a heap of Cap: the levels of the wave's
        // own heaps (umax) are the same for all but small streams
        const uint16_t t =
            sift_depth<Cap, sift_levels_bound(Cap, I)>(w, U, I, (uint16_t)h0[I]);
        if (I == 0) root = t;
      }
    }
    build_heap_from<Cap, I - 1>(w, umax, U, h0, root);
  }
}

template <int Cap, class W>
__device__ __forceinline__ uint16_t sift_any(const W &w, int size, int i, uint16_t x) {
  if constexpr (Cap <= 31) return sift_fixed<Cap>(w, size, i, x);
  else return sift<Cap & ~1>(w, size, i, x);
}

// The Huffman code of one stream from its U symbols' counts, exactly as the
// reference builds it: build_heap (JPEG.c:913-936) over the frequency list in
// first-occurrence order, build_huffman_tree (:938-962: pop, pop, append the
// merged node WITHOUT sifting it up), assign_codes (:964-983: DFS, left
// first).  In: w.heap[u + 1] = count << 8 | u and w.sym[u] for u < U.  Out:
// w.code / w.len per leaf and the table (value | length << 16 per code, DFS
// order).  Returns true when a code exceeds the reference's char code[32].
// h0 (Cap <= 31): heap entry i's initial value (count << 8 | i) for i < U.
template <int Cap, class W>
__device__ __forceinline__ bool tree_codes(const W &w, int U, uint32_t *__restrict__ table,
                                           const uint32_t *h0 = nullptr) {
  int size = U, next = U;
  uint16_t root;
  int umax = 0;
  if constexpr (Cap <= 31) {
    // Every lane's heap shrinks by one per merge, so at merge step t no lane's
    // heap exceeds Umax - t (Umax: the wave's largest U): each sift runs only
    // the levels that bound allows (and build_heap's sift from index i, the
    // levels below i in a heap of Umax), picked by uniform branches.
#pragma unroll
    for (int b = 4; b >= 0; --b)
      if (__ballot(U >= (umax | (1 << b)))) umax |= 1 << b;
    root = (uint16_t)h0[0];
    build_heap_from<Cap, Cap / 2 - 1>(w, umax, U, h0, root);
    // Each pop moves the last entry to the root and sifts it.  The first pop's
    // last entry is the node the previous merge appended (in registers); the
    // second pop's is read before the first sift, which changes that index
    // (the heap's last: no children) only by landing its x there.  So each
    // merge waits on the two sifts' LDS round trips alone.
    uint16_t last = w.heap[U];                        // entry U - 1 after the build
    // Merge step t pops from heaps of at most umax - t - 1 entries: the steps
    // run in phases of one sift depth, floor(log2(umax - t - 1)) levels (the
    // second pop's heap is one smaller: the same depth serves), so no step
    // dispatches on its depth or loops to find it.
    auto merge = [&](auto depth) {
      constexpr int D = decltype(depth)::value;
      if (size > 1) {
        const uint16_t left = root;
        --size;
        const uint16_t e2 = w.heap[size];             // entry size - 1, before the sift
        int fi;
        root = sift_depth<Cap, D>(w, size, 0, last, &fi);
        const uint16_t right = root;
        const uint16_t x2 = fi == size - 1 ? last : e2;
        --size;
        root = sift_depth<Cap, D>(w, size, 0, x2);
        const uint16_t merged = (uint16_t)((((left >> 8) + (right >> 8)) << 8) | next);
        w.heap[size + 1] = merged;                                              // not sifted up
        last = merged;
        if constexpr (W::kTopDown) {
          // record of merged node m = next - U: left | right << 6 | leaves
          // under it << 12 | leaves under left << 17 (| DFS position << 22 |
          // depth << 27, or-ed in top-down)
          const int li = left & 255, ri = right & 255;
          const uint32_t rl = w.mrec[li < U ? 0 : li - U], rr = w.mrec[ri < U ? 0 : ri - U];
          const uint32_t nl = li < U ? 1u : (rl >> 12) & 31u, nr = ri < U ? 1u : (rr >> 12) & 31u;
          w.mrec[next - U] = (uint32_t)li | (uint32_t)ri << 6 | (nl + nr) << 12 | nl << 17;
        } else {
          w.heap[U - (next - U)] = (uint16_t)((left & 255) | ((right & 255) << 8));   // freed slot
        }
        ++size;
        ++next;
        if (size == 1) root = merged;
      }
    };
    int t = 0;
    if constexpr (Cap >= 17) {
      for (; umax - t - 1 >= 16; ++t) merge(std::integral_constant<int, 4>{});
    }
    if constexpr (Cap >= 9) {
      for (; umax - t - 1 >= 8; ++t) merge(std::integral_constant<int, 3>{});
    }
    for (; umax - t - 1 >= 4; ++t) merge(std::integral_constant<int, 2>{});
    for (; umax - t > 1; ++t) merge(std::integral_constant<int, 1>{});
  } else {
  for (int i = U / 2 - 1; i >= 0; --i) sift_any<Cap>(w, U, i, w.heap[i + 1]);
  root = w.heap[1];
  while (size > 1) {
    // pop, pop (the moved last entry sifted from the root; the new root is
    // known in registers), append the merged node unsifted
    const uint16_t left = root;
    --size;
    root = sift_any<Cap>(w, size, 0, w.heap[size + 1]);
    const uint16_t right = root;
    --size;
    root = sift_any<Cap>(w, size, 0, w.heap[size + 1]);
    const uint16_t merged = (uint16_t)((((left >> 8) + (right >> 8)) << 8) | next);
    w.heap[size + 1] = merged;                                              // not sifted up
    w.heap[U - (next - U)] = (uint16_t)((left & 255) | ((right & 255) << 8));   // freed slot
    ++size;
    ++next;
    if (size == 1) root = merged;
  }
  }

  // ---- codes: DFS, left first (JPEG.c:964-983) ------------------------------
  // Leaves pop in codes[] order; each code follows from the previous one:
  // code[k] = (code[k-1] + 1) moved to length len[k].  The current node stays
  // in registers: an internal node stacks its right child and descends left.
  bool over = false;
  if constexpr (W::kTopDown) {
    // Top-down instead of the DFS: merged nodes from the root down (merge
    // step t's node is m = U - 2 - t), each handing its children their depth
    // and DFS position (left: the parent's; right: + the leaves under left);
    // a leaf records (depth | leaf << 8) at its position.  U - 1 steps
    // instead of 2U - 1.  Then the leaves in DFS order give the codes as the
    // DFS does.
    static_assert(2 * Cap - 1 <= 64 && Cap <= 31, "record fields");
    if (U == 1) w.dep[0] = 0;                         // the root is leaf 0, depth 0
    for (int t = 0; t + 1 < umax; ++t) {
      if (t + 1 < U) {
        const uint32_t rc = w.mrec[U - 2 - t];
        const int li = (int)(rc & 63u), ri = (int)((rc >> 6) & 63u);
        const uint32_t pos = (rc >> 22) & 31u, dc = (rc >> 27) + 1u, nl = (rc >> 17) & 31u;
        if (li < U) w.dep[(int)pos] = (uint16_t)(dc | (uint32_t)li << 8);
        else atomicOr(&w.mrec[li - U], pos << 22 | dc << 27);
        if (ri < U) w.dep[(int)(pos + nl)] = (uint16_t)(dc | (uint32_t)ri << 8);
        else atomicOr(&w.mrec[ri - U], (pos + nl) << 22 | dc << 27);
      }
    }
    int plen = 0;
    uint32_t pcode = 0;
    uint32_t de[Cap];
    int sy[Cap];
    // (all Cap positions, no uniform branch per position: past a lane's U
    // the entries are dead rows' values and nothing is stored)
#pragma unroll
    for (int k = 0; k < Cap; ++k) de[k] = w.dep[k];
#pragma unroll
    for (int k = 0; k < Cap; ++k) sy[k] = w.sym[min((int)(de[k] >> 8), Cap - 1)];
#pragma unroll
    for (int k = 0; k < Cap; ++k) {
      const int d = (int)(de[k] & 255u), x = min((int)(de[k] >> 8), Cap - 1);
      const uint32_t t = k ? pcode + 1 : 0u;
      pcode = d >= plen ? t << (d - plen) : t >> (plen - d);
      plen = d;
      if (k < U) {
        // the code left-aligned, its length in the low 5 bits (depth <= Cap - 1
        // < 27 leaves them zero)
        w.code[x] = (d ? pcode << (32 - d) : 0u) | (uint32_t)d;
        table[k] = (uint16_t)sy[k] | ((uint32_t)d << 16);
      }
    }
    return over;
  } else {
  int sp = 0, k = 0, plen = 0;
  uint32_t pcode = 0;
  int e = root & 255;                                 // the root, depth 0
  // Both successors (the stack top, the node's children) and a leaf's symbol
  // are read at the top of every step, one LDS round trip, so a leaf step
  // does not wait on a second one before its table store.
  for (;;) {
    const int x = e & 255, d = e >> 8;
    const bool leaf = x < U;
    const int top = w.stk[sp > 0 ? sp - 1 : 0];       // a leaf's successor
    const int ch = w.heap[leaf ? 0 : 2 * U - x];      // children of merged node x - U
    const int sy = w.sym[leaf ? x : 0];               // a leaf's symbol
    if (leaf) {                                       // leaf: next entry of codes[]
      const uint32_t t = k ? pcode + 1 : 0u;
      pcode = d >= plen ? t << (d - plen) : t >> (plen - d);
      plen = d;
      if constexpr (W::kPackLen) {
        w.code[x] = pcode | (uint32_t)d << 24;        // depth <= Cap - 1 < 24
      } else {
        w.code[x] = pcode;
        w.len[x] = (uint8_t)d;
      }
      if (d > 31) over = true;                        // char code[32] (JPEG.c:861)
      table[k] = (uint16_t)sy | ((uint32_t)d << 16);
    } else {
      w.stk[sp] = (uint16_t)((ch >> 8) | ((d + 1) << 8));     // right, visited later
    }
    if (leaf && sp == 0) break;
    k += leaf ? 1 : 0;
    sp += leaf ? -1 : 1;
    e = leaf ? top : (ch & 255) | ((d + 1) << 8);              // left now
  }
  return over;
  }
}

enum : int { kOk = 0, kDefer = 1, kOverflow = 2 };

__device__ __forceinline__ int hash_slot(int s, int mask) {
  return (int)(((uint32_t)(s + 1024) * 0x9E3779B1u) >> 24) & mask;
}

// The RLE of the n ints at zz (JPEG.c:767-808): emit(count), emit(value) at
// the end of every run, in order.  The ints are read 8 at a time as 16-B
// loads, the next chunk in flight while this one is walked (a lane's stream
// is 128 or 64 contiguous bytes: one load per int, 64 lanes 256 B apart,
// was a memory round trip per int).
template <class F>
__device__ __forceinline__ void rle_walk(const int16_t *__restrict__ zz, int n, F &&emit) {
  const uint4 *src = reinterpret_cast<const uint4 *>(zz);
  uint4 nxt = src[0];
  int cur = 0, run = 0;
  for (int ch = 0; ch < n / 8; ++ch) {
    const uint4 q = nxt;
    if (ch + 1 < n / 8) nxt = src[ch + 1];
    const uint32_t wv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int16_t)(wv[j >> 1] >> (16 * (j & 1)));
      if (ch == 0 && j == 0) {
        cur = v;
        run = 1;
      } else if (v == cur) {
        ++run;
      } else {
        emit(run);
        emit(cur);
        cur = v;
        run = 1;
      }
    }
  }
  emit(run);
  emit(cur);
}

// Encode one stream of n ints at zz (global).  Writes the packed bits (slot
// of cap_bits), the table (value | len << 16 per code, DFS order) and the
// meta word (nbits | rle_len << 16 | ncodes << 24).  Returns kOk, kDefer
// (more than Cap distinct symbols; nothing written) or kOverflow (a code or
// the sequence exceeds the reference's fixed buffers; written truncated).
template <int Cap, int Hash, class W>
__device__ int encode_stream(const int16_t *__restrict__ zz, int n, const W &w,
                             uint8_t *__restrict__ bits, int cap_bits, int ref_max,
                             uint32_t *__restrict__ table, uint32_t *__restrict__ meta) {
  static_assert((Hash & (Hash - 1)) == 0 && Hash >= Cap * 4 / 3, "power of two, load <= 3/4");
  constexpr int kMask = Hash - 1;
  // symbol -> leaf through the hash (inserting new symbols in first-occurrence
  // order, JPEG.c:864-886); returns -1 when a new symbol does not fit
  int U = 0;
  auto leaf_of = [&](int s, bool insert) -> int {
    int h = hash_slot(s, kMask);
    for (;;) {
      const int e = w.hash[h];
      if (e == 0) {
        if (!insert || U == Cap) return -1;
        w.hash[h] = (uint8_t)(U + 1);
        w.sym[U] = (int16_t)s;
        w.heap[U + 1] = (uint16_t)U;                // count 0, id U
        return U++;
      }
      if (w.sym[e - 1] == s) return e - 1;
      h = (h + 1) & kMask;
    }
  };
  w.hash.clear(Hash);

  // ---- RLE (JPEG.c:767-808) + frequencies --------------------------------------
  int R = 0;
  bool defer = false;
  auto count = [&](int s) {
    const int u = leaf_of(s, true);
    if (u < 0) {
      defer = true;
      return;
    }
    w.heap[u + 1] = (uint16_t)(w.heap[u + 1] + 256);
    ++R;
  };
  rle_walk(zz, n, [&](int sy) {
    if (!defer) count(sy);
  });
  if (defer) return kDefer;

  // ---- heap, tree and codes (JPEG.c:913-983) ---------------------------------
  bool over = tree_codes<Cap>(w, U, table);

  // ---- encoded sequence, MSB-first (JPEG.c:993-1007): RLE again --------------
  uint64_t acc = 0;
  int nacc = 0, nbits = 0, word = 0;
  const int nwords = cap_bits / 32;
  uint32_t *wout = reinterpret_cast<uint32_t *>(bits);
  auto put = [&](int s) {
    const int leaf = leaf_of(s, false);
    const int L = w.len[leaf];
    if (L > 32) return;                               // flagged above; no 64-bit overshift
    acc = (acc << L) | w.code[leaf];
    nacc += L;
    nbits += L;
    if (nacc >= 32) {
      const uint32_t v = (uint32_t)(acc >> (nacc - 32));
      if (word < nwords) wout[word] = __builtin_bswap32(v);
      ++word;
      nacc -= 32;
    }
  };
  rle_walk(zz, n, put);
  if (nacc && word < nwords) wout[word] = __builtin_bswap32((uint32_t)(acc << (32 - nacc)));
  if (nbits > ref_max) over = true;                   // char sequence[1024] / [512]
  *meta = (uint32_t)(nbits < 0xFFFF ? nbits : 0xFFFF) | ((uint32_t)R << 16) |
          ((uint32_t)U << 24);
  return over ? kOverflow : kOk;
}

template <typename T>
using GColT = Col<T>;

// One working set of the hashed encoder (encode_stream<kFullCap, 2 * kFullCap>):
// kEnd bytes at a 4-B aligned lb, global or LDS
constexpr int kSymO = 0, kHashO = kSymO + 2 * kFullCap, kHeapO = kHashO + 2 * kFullCap;
constexpr int kCodeO = (kHeapO + 2 * (kFullCap + 2) + 3) & ~3, kLenO = kCodeO + 4 * kFullCap;
constexpr int kStkO = (kLenO + kFullCap + 1) & ~1, kEnd = kStkO + 2 * (kFullCap + 1);

__device__ __forceinline__ Work<GColT> hashed_work(uint8_t *lb) {
  return {{reinterpret_cast<int16_t *>(lb + kSymO), 1}, {lb + kHashO, 1},
          {reinterpret_cast<uint16_t *>(lb + kHeapO), 1},
          {reinterpret_cast<uint32_t *>(lb + kCodeO), 1}, {lb + kLenO, 1},
          {reinterpret_cast<uint16_t *>(lb + kStkO), 1}};
}

// Scratch (d_scratch): per luma wave a list of its deferred streams (64
// entries), then per luma wave a word deferred | overflowed << 8 (lanes).
// The chroma kernel reads them (its even wave 2 v: luma wave v), so no
// kernel runs before the lane kernels or after them.

// ---- the fast encoder: one lane per stream, no probing ------------------------
// Symbols index a direct per-lane table (symbol + kOff -> leaf + 1, u8), so a
// lookup is one LDS read with no probe loop: the RLE walk is unrolled over
// the stream's positions and, per position, every lane whose run ends there
// looks up BOTH its symbols (count, value) with the two reads in flight
// together (an equal pair is resolved in registers) -- one LDS round trip
// per position, where the hashed walk took up to three per symbol, for the
// wave's longest probe chain.  Counts are bumped by ds_add_u32 on the heap
// entry's half-word (no read).  Each emission's two leaf ids stay in
// registers (5 bits each, 3 positions per dword), so the sequence pass reads
// only the codes.  The table is dead after the count: the DFS stack and the
// codes overlay it.  A stream with a symbol outside the table or more than
// Cap distinct symbols is deferred: the chroma kernel encodes it with the
// hashed encoder after its own streams.
template <int N>
struct LaneLds {
  static constexpr int Cap = N == 64 ? kFastCap : kChromaCap;
  static constexpr int Keys = N == 64 ? 176 : 120;   // symbols [-Off, Keys - Off)
  static constexpr int Off = N == 64 ? 64 : 48;       // counts: 1 .. N
  static constexpr int StkRows = (Cap + 2) / 2;       // overlays of the table (dword rows)
  // a zero row, then per leaf its code left-aligned | length (leaf + 1
  // indexes from the zero row: id 0, no emission, reads a length-0 code);
  // past the codes, the sequence pass's bit rows (through heap and sym)
  static constexpr int ZeroRow = StkRows, CodeRow = StkRows + 1;
  static_assert(CodeRow + Cap <= Keys / 4, "stack and codes fit the table");
  // (the merge records, Cap - 1 rows from row 0, are dead before the codes
  // and the zero row are written; the depths by DFS position take Cap / 2
  // rows of the dead heap)
  static_assert(Off + N < Keys, "every count is a key");
  // Luma's heap takes a dword row per entry (no half-word address arithmetic
  // in the sifts; 19 KB per wave, still 8 waves per CU: a 4K image's 2,025
  // luma waves in one round); chroma's stays two entries per dword (10 KB:
  // 16 waves per CU, its 4,050 waves in one round).
  static constexpr bool Wide = N == 64;
  static constexpr int HeapRows = Wide ? Cap + 2 : (Cap + 2) / 2;
  static_assert(HeapRows >= Cap / 2, "the walk's (symbol | count) rows");
  uint32_t tab[Keys / 4][kLanes];
  uint32_t heap[HeapRows][kLanes];
  uint32_t sym[Cap / 4][kLanes];                      // int8 symbols
};

// One lane's u16 array with an element per dword row (the low half); a pair
// is two rows
struct WCol {
  typedef uint16_t __attribute__((may_alias)) TA;
  typedef uint32_t __attribute__((may_alias)) WA;
  uint8_t *p;
  __device__ __forceinline__ TA &operator[](int i) const {
    return *reinterpret_cast<TA *>(p + (uint32_t)i * (4 * kLanes));
  }
  __device__ __forceinline__ uint32_t pair(int i) const {
    const WA *q = reinterpret_cast<const WA *>(p + (uint32_t)i * (4 * kLanes));
    return __builtin_amdgcn_perm(q[kLanes], q[0], 0x05040100u);
  }
};

template <class HeapCol>
struct LaneWork {                                     // the arrays tree_codes uses
  static constexpr bool kPackLen = true;              // code and length in one dword (tree_codes)
  static constexpr bool kTopDown = true;              // codes top-down over mrec (tree_codes)
  LCol<int8_t> sym;
  HeapCol heap;
  LCol<uint32_t> code;
  LCol<uint32_t> mrec;   // merged node m's record (the dead table's rows, before the codes)
  LCol<uint16_t> dep;    // (depth | leaf << 8) by DFS position (the dead heap's rows)
};

// ---- the lane encoders' walk: what entropy_encode_lane (slots) and
// stream_encode_lane (a JPR1 / JPT1 stream) do alike, in the order they do it.
// tabc, heap, sym: the lane's columns of LaneLds<N>'s tab, heap and sym rows.

// What the RLE + count walk leaves beside the leaf ids: the distinct symbols
// (clamped to Cap), the RLE ints and whether the stream is deferred
struct LaneRle {
  int U, R;
  bool defer;
};

// RLE (JPEG.c:767-808) + frequencies (JPEG.c:864-886) of the N ints at zz:
// run k ends at position i when i == N - 1 or the next int differs; it emits
// (count, value).  Leaf ids in first-occurrence order; lid, per position:
// (leaf_c + 1) | (leaf_v + 1) << 5, three positions per dword.
template <int N>
__device__ __forceinline__ LaneRle lane_rle_count(const int16_t *zz, uint8_t *tabc,
                                                  uint8_t *heap, uint32_t (&lid)[(N + 2) / 3]) {
  using L = LaneLds<N>;
  constexpr int Cap = L::Cap, Keys = L::Keys, Off = L::Off;
  // the stream: N int16 as N / 2 packed dwords (16-B loads)
  uint32_t iw[N / 2];
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(zz);
#pragma unroll
    for (int k = 0; k < N / 8; ++k) {
      const uint4 q = src[k];
      iw[4 * k] = q.x; iw[4 * k + 1] = q.y; iw[4 * k + 2] = q.z; iw[4 * k + 3] = q.w;
    }
  }
#pragma unroll
  for (int r = 0; r < Keys / 4; ++r) *reinterpret_cast<uint32_t *>(tabc + r * (4 * kLanes)) = 0u;
  auto val = [&](int i) { return (int)(int16_t)(iw[i >> 1] >> (16 * (i & 1))); };
  auto tab_at = [&](int k) -> uint8_t & {
    return *(tabc + (k >> 2) * (4 * kLanes) + (k & 3));
  };
  uint32_t ids = 0;                      // the ids of lid's dword under way
  int U = 0, start = 0, R = 0;
  bool defer = false;
  // One exec region per position and no branch inside it: the stores are
  // unconditional and idempotent (a known symbol rewrites its table entry and
  // its symbol with the values they hold), and a count is a ds_add into the
  // zeroed heap rows, which hold (symbol | count << 8) per leaf during the
  // walk.  A stream that must be deferred runs on with clamped leaf ids over
  // its own columns (the results are dropped).
#pragma unroll
  for (int r = 0; r < Cap / 2; ++r) *reinterpret_cast<uint32_t *>(heap + r * (4 * kLanes)) = 0u;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int v = val(i);
    const bool end = i == N - 1 || val(i + 1 < N ? i + 1 : i) != v;
    if (end) {
      const int kc = i + 1 - start + Off;
      start = i + 1;
      const bool bad = (uint32_t)(v + Off) >= (uint32_t)Keys;
      const int kv = bad ? kc : v + Off;
      const int ec = tab_at(kc), ev = tab_at(kv);       // both reads in flight
      const bool same = kv == kc;
      const int lc = ec ? ec - 1 : U;
      const int nu = U + (ec ? 0 : 1);
      const int lv = same ? lc : (ev ? ev - 1 : nu);
      const int nu2 = nu + ((same || ev) ? 0 : 1);
      defer = defer || bad || nu2 > Cap;
      const int lcw = min(lc, Cap - 1), lvw = min(lv, Cap - 1);
      tab_at(kc) = (uint8_t)(lcw + 1);
      tab_at(kv) = (uint8_t)(lvw + 1);
      // leaf u's symbol and count: one u16 (symbol | count << 8) at half
      // u & 1 of dword row u >> 1, so the store and the add share an address
      uint8_t *const sc = heap + ((lcw >> 1) << 8), *const sv = heap + ((lvw >> 1) << 8);
      const int hc = (lcw & 1) << 4, hv = (lvw & 1) << 4;
      const bool fc = ec == 0, fv = !same && ev == 0;    // first occurrences
      const uint32_t ac = (fc ? (uint32_t)(uint8_t)(kc - Off) : 0u) + ((same ? 2u : 1u) << 8);
      const uint32_t av = (fv ? (uint32_t)(uint8_t)(kv - Off) : 0u) + ((same ? 0u : 1u) << 8);
      atomicAdd(reinterpret_cast<uint32_t *>(sc), ac << hc);
      atomicAdd(reinterpret_cast<uint32_t *>(sv), av << hv);
      U = min(nu2, Cap);
      R += 2;                                         // the run's (count, value)
      ids |= (uint32_t)((lcw + 1) | ((lvw + 1) << 5)) << (10 * (i % 3));
    }
    if (i % 3 == 2 || i == N - 1) {
      lid[i / 3] = ids;
      ids = 0;
    }
  }
  return {U, R, defer};
}

// The walk's (symbol | count << 8) per leaf -> the symbols (i8, 4 per dword),
// the heap entries (count << 8 | leaf at slot leaf + 1) and, in registers,
// h0: heap entry u's initial value, count << 8 | u (tree_codes)
template <int N>
__device__ __forceinline__ void lane_heap_seed(uint8_t *heap, uint8_t *sym,
                                               uint32_t (&h0)[LaneLds<N>::Cap]) {
  using L = LaneLds<N>;
  constexpr int Cap = L::Cap;
  auto row = [&](int r) { return reinterpret_cast<uint32_t *>(heap + r * (4 * kLanes)); };
  uint32_t sc[Cap / 2];
#pragma unroll
  for (int k = 0; k < Cap / 2; ++k) sc[k] = *row(k);
#pragma unroll
  for (int u = 0; u < Cap; ++u) h0[u] = ((sc[u >> 1] >> (16 * (u & 1))) & 0xFF00u) | (uint32_t)u;
#pragma unroll
  for (int j = 0; j < Cap / 4; ++j)
    *reinterpret_cast<uint32_t *>(sym + j * (4 * kLanes)) =
        __builtin_amdgcn_perm(sc[2 * j + 1], sc[2 * j], 0x06040200u);
  if constexpr (L::Wide) {
    // slot s (leaf s - 1) is row s
#pragma unroll
    for (int u = 0; u < Cap; ++u)
      *row(u + 1) = ((sc[u >> 1] >> (16 * (u & 1))) & 0xFF00u) | (uint32_t)u;
  } else {
#pragma unroll
    for (int r = 0; r < (Cap + 2) / 2; ++r) {
      // slot 2r: leaf 2r - 1 (count: byte 3 of sc[r - 1]); slot 2r + 1: leaf 2r (byte 1 of sc[r])
      const uint32_t lo = r > 0 ? (sc[r - 1] >> 16) & 0xFF00u : 0u;
      const uint32_t hi = r < Cap / 2 ? (sc[r] & 0xFF00u) << 16 : 0u;
      *row(r) = lo | hi | (uint32_t)(r > 0 ? 2 * r - 1 : 0) | (uint32_t)(2 * r) << 16;
    }
  }
}

// The encoded sequence, MSB-first (JPEG.c:993-1007), from bit pos0 of the
// lane's bit rows at brow (row r at brow + 256 r): the bits_cap / 32 rows of
// the slot, then kSpill rows (>= 2) that take what follows pos0 and the bits
// of a stream that overflows its slot.  Returns the position past the last bit.
// A leaf's code word is its code left-aligned with its length in the low
// 5 bits (codez: the zero row, then the codes, so id 0 reads a length-0
// code); the reads do not depend on the bit position, so each group of kG
// positions' code words is read while the previous group is placed.  Each
// code is or-ed into the lane's zeroed bit rows at its bit position (two
// ds_or: the word it starts in and the next).  No exec branch per code: the
// accumulator form stored each completed word under one.
template <int N, int kSpill>
__device__ __forceinline__ int lane_sequence(const uint32_t (&lid)[(N + 2) / 3],
                                             const LCol<uint32_t> codez, uint8_t *brow, int pos0) {
  constexpr int nwords = N / 2;                       // bits_cap / 32
  auto bit_row = [&](int r) { return reinterpret_cast<uint32_t *>(brow + r * (4 * kLanes)); };
  codez[0] = 0u;
#pragma unroll
  for (int r = 0; r < nwords + kSpill; ++r) *bit_row(r) = 0u;
  int pos = pos0;
  constexpr int kG = 4;
  static_assert(N % kG == 0, "whole groups");
  auto ident = [&](int i, int h) {                    // leaf + 1 of emission h at position i, 0: none
    return (lid[i / 3] >> (10 * (i % 3) + 5 * h)) & 31u;
  };
  auto fetch = [&](int g, uint32_t (&cw)[2 * kG]) {
#pragma unroll
    for (int j = 0; j < 2 * kG; ++j) {
      cw[j] = codez[(int)ident(g * kG + j / 2, j & 1)];
    }
  };
  uint32_t cur[2 * kG], nxt[2 * kG];
  fetch(0, nxt);
#pragma unroll
  for (int g = 0; g < N / kG; ++g) {
#pragma unroll
    for (int j = 0; j < 2 * kG; ++j) cur[j] = nxt[j];
    if (g + 1 < N / kG) fetch(g + 1, nxt);
#pragma unroll
    for (int j = 0; j < 2 * kG; ++j) {
      const uint32_t al = cur[j] & ~31u;
      const uint32_t o = (uint32_t)pos & 31u;
      uint32_t *const r0 = bit_row(min(pos >> 5, nwords + kSpill - 2));
      atomicOr(r0, al >> o);
      atomicOr(r0 + kLanes, __builtin_amdgcn_alignbit(al, 0u, o));   // (o = 0: none)
      pos += (int)(cur[j] & 31u);
    }
  }
  return pos;
}

}  // namespace
