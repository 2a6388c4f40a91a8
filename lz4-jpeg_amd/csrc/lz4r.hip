// lz4r.hip -- MI355X (gfx950) "LZ4" compressor, bit-exact to the reference's
// Algorithms/sequential/LZ4/LZ4.c (canonical block-clamped matches).
//
// The reference cuts the input into 300-byte blocks (LZ4.c:23, 123-177) and,
// in every block, greedily parses with an exhaustive longest-match search over
// the whole block prefix (find_longest_match, LZ4.c:290-323; strict '>' so the
// smallest i -- farthest offset -- wins ties; length truncated to uint8_t).
// Blocks are independent; the compressor is one compute kernel, a scan and
// an emission pass, each in a header of its own (one translation unit: the
// includes below are in the kernels' definition order):
//
//   lz4r_layout.h    what the kernels and run() share: the block grid, the
//                    record scratch, the scan's grouping, the error bit
//   lz4r_tiles.h     lz4_tiles: one wave per run of blocks, match finder and greedy
//                    parse -> sequence records and the block's byte count
//                    (its LDS layout and primitives: lz4r_tile_lds.h)
//   lz4r_matches.h   lz4_matches, lz4_window_matches: the batch match finders
//   lz4r_scan.h      lz4_scan_reduce16, lz4_scan_partials_frame: exclusive scan
//                    of the byte counts
//   lz4r_emit.h      lz4_emit: 32 blocks per workgroup, records -> stream bytes
//   lz4r_frame.h     lz4f_sizes, lz4f_scan, lz4f_emit: the same records as a
//                    standard LZ4 frame (the lz4r_compress_frame_* calls)
//   wave64.h         the wave-level helpers all of them use
//   lz4r_prof.h      PROF_MARK: nothing in the product, cycle counters or
//                    assembly markers in the tools builds
//   below            the host side: launch chunking, the context and its
//                    scratch, the timing ring, run() and the C ABI
//
// HBM traffic per input byte: 1 B read + ~0.35 B of records written by
// lz4_tiles; ~1 B of input + ~0.33 B of record heads read and ~1.03 B
// written by lz4_emit (+12 B/block: 2 B of size written by lz4_tiles and read
// by the scan and by lz4_emit, 8 B of offset written).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/lz4r.h"
#include "lz4r_prof.h"
#include "wave64.h"
#include "lz4r_layout.h"
#include "lz4r_tiles.h"
#include "lz4r_matches.h"
#include "lz4r_scan.h"
#include "lz4r_emit.h"
#include "lz4r_frame.h"
#include "../host/lz4f_xxh32.h"

// Launch chunking: lz4_tiles was a 64-lane workgroup per block (now per run
// of kTileRun blocks; the chunk size stayed), and a HIP
// grid may not exceed 2^32 work-items, so a call is cut into chunks of at
// most kChunk blocks (5.03 GB of input; a multiple of the scan partial, so
// every chunk starts on a gather group and a partial).  The block slots are
// sized for one chunk (10.7 GB at most) and reused; the per-block arrays and
// the scan state span the whole call.  Each chunk is a full compress ->
// scan -> gather pass that continues the stream offset the previous chunk
// left in *d_len; the per-chunk launch cost (four launches) is noise against
// the ~19 ms of encoder work in a full chunk.
#ifndef LZ4R_CHUNK_LOG2
#define LZ4R_CHUNK_LOG2 24
#endif
constexpr size_t kChunk = size_t(1) << LZ4R_CHUNK_LOG2;
static_assert(kChunk % kPart == 0, "chunks start on a scan partial");
static_assert((kChunk / 8) * 8 * 64 < (size_t(1) << 32), "chunk grid fits HIP's limit");
// largest input one call accepts (block indices are u32 in the per-call arrays)
constexpr size_t kMaxInput = size_t(1) << 40;

struct lz4r_ctx {
  int device = 0;
  size_t cap_blocks = 0;       // capacity of the per-call per-block arrays
  size_t cap_slots = 0;        // capacity of the slot scratch, in blocks (<= kChunk)
  uint16_t *bsizes = nullptr;  // encoded bytes of every block of the last call (what the
                               // scan and lz4_emit read, and lz4r_copy_block_sizes copies)
  uint64_t *boff = nullptr;    // every block's offset from the first block byte
  uint8_t *slots = nullptr;    // per-block record scratch, one chunk: cap_slots heads of
                               // kHead bytes, then cap_slots overflow slots of kOvf
  uint32_t *gsum = nullptr;    // encoded bytes per group of kGT blocks
  uint64_t *part = nullptr;    // scan partials, one per kPart blocks
  uint64_t *len = nullptr;     // default device length slot, the status word, the verdict
  uint32_t *status = nullptr;  // (len + 1) nonzero once a block saw a corrupt bucket head
  uint64_t *verdict = nullptr; // (len + 2) the last call's corrupt-index verdict (0 / 1)
  size_t last_nb = 0;
  bool last_frame = false;     // the last call wrote a standard frame: no per-block arrays
  bool checkable = false;      // a call has launched (lz4r_check has a verdict to read)
  // timing: per timed call since lz4r_set_timing(1), the call's start/end
  // events and lz4_tiles' start/end in every chunk (a ring of kTimedCalls
  // sets, so back-to-back async calls need no host wait between them)
  struct timed_set {
    hipEvent_t a = nullptr, c = nullptr;
    std::vector<hipEvent_t> tiles;   // 2 per chunk (chunk 0 starts at a: tiles[0] unused)
    size_t chunks = 0;
  };
  std::vector<timed_set> tsets;
  size_t timed_calls = 0;      // calls recorded since timing was enabled
  bool timing = false;
};
constexpr size_t kTimedCalls = 4096;

namespace {

void free_scratch(lz4r_ctx *c) {
  (void)hipFree(c->bsizes);
  (void)hipFree(c->boff);
  (void)hipFree(c->gsum);
  (void)hipFree(c->part);
  (void)hipFree(c->slots);
  c->bsizes = nullptr;
  c->boff = nullptr;
  c->slots = nullptr;
  c->gsum = nullptr;
  c->part = nullptr;
  c->cap_blocks = 0;
  c->cap_slots = 0;
}

int ensure_scratch(lz4r_ctx *c, size_t nb) {
  const size_t need_slots = std::min(nb, kChunk);
  if (nb <= c->cap_blocks && need_slots <= c->cap_slots) return LZ4R_OK;
  free_scratch(c);
  const size_t cap = nb + nb / 8 + 1024;
  const size_t cap_slots = std::min(cap, kChunk);
  const size_t parts = (cap + kPart - 1) / kPart;
  const size_t groups = (cap + kGT - 1) / kGT;
  // hipMalloc: 256-B aligned; heads and overflow slots are 16-B multiples
  if (hipMalloc(&c->slots, cap_slots * (size_t)kSlot) != hipSuccess ||
      hipMalloc(&c->bsizes, cap * sizeof(uint16_t)) != hipSuccess ||
      hipMalloc(&c->boff, cap * sizeof(uint64_t)) != hipSuccess ||
      hipMalloc(&c->gsum, groups * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&c->part, parts * sizeof(uint64_t)) != hipSuccess) {
    (void)hipGetLastError();
    free_scratch(c);
    return LZ4R_ERR_NOMEM;
  }
  c->cap_blocks = cap;
  c->cap_slots = cap_slots;
  return LZ4R_OK;
}

// A timing event: no system-scope fence when it is recorded (the events only
// time the work; the call's results reach the host by their own copies).  With
// the default fence every record writes back and invalidates the caches: four
// records cost a back-to-back call 13 us (tools/timing_cost.py).
int make_event(hipEvent_t *e) {
  return hipEventCreateWithFlags(e, hipEventDisableSystemFence) == hipSuccess ? LZ4R_OK
                                                                               : LZ4R_ERR_HIP;
}

// the event set of the next timed call (created on first use)
int next_timed_set(lz4r_ctx *c, size_t nchunks, lz4r_ctx::timed_set **out) {
  const size_t i = c->timed_calls % kTimedCalls;
  if (c->tsets.size() <= i) c->tsets.resize(i + 1);
  lz4r_ctx::timed_set &t = c->tsets[i];
  if ((!t.a && make_event(&t.a) != LZ4R_OK) || (!t.c && make_event(&t.c) != LZ4R_OK))
    return LZ4R_ERR_HIP;
  while (t.tiles.size() < 2 * nchunks) {
    hipEvent_t e = nullptr;
    if (make_event(&e) != LZ4R_OK) return LZ4R_ERR_HIP;
    t.tiles.push_back(e);
  }
  t.chunks = nchunks;
  *out = &t;
  return LZ4R_OK;
}

void destroy_events(lz4r_ctx *c) {
  for (auto &t : c->tsets) {
    if (t.a) (void)hipEventDestroy(t.a);
    if (t.c) (void)hipEventDestroy(t.c);
    for (hipEvent_t e : t.tiles) (void)hipEventDestroy(e);
  }
  c->tsets.clear();
}

// milliseconds of timed call set t: the whole call and its lz4_tiles launches
int timed_ms(const lz4r_ctx::timed_set &t, float *ms_call, float *ms_match) {
  if (hipEventSynchronize(t.c) != hipSuccess) return LZ4R_ERR_HIP;
  float a = 0.f, b = 0.f;
  if (hipEventElapsedTime(&a, t.a, t.c) != hipSuccess) return LZ4R_ERR_HIP;
  for (size_t k = 0; k < t.chunks; ++k) {
    float x = 0.f;
    if (hipEventElapsedTime(&x, k == 0 ? t.a : t.tiles[2 * k], t.tiles[2 * k + 1]) != hipSuccess)
      return LZ4R_ERR_HIP;
    b += x;
  }
  *ms_call = a;
  *ms_match = b;
  return LZ4R_OK;
}

// The header of a standard frame of n content bytes (lz4r_frame.h): magic,
// FLG 0x68 (version 01, independent blocks, content size), BD 0x40 (64 KiB
// block maximum), the size, HC = the second byte of xxh32(FLG .. size).
void frame_header(size_t n, uint8_t h[kFrameHdr]) {
  const uint8_t fixed[6] = {0x04, 0x22, 0x4D, 0x18, 0x68, 0x40};
  for (int i = 0; i < 6; ++i) h[i] = fixed[i];
  for (int i = 0; i < 8; ++i) h[6 + i] = (uint8_t)((uint64_t)n >> (8 * i));
  h[14] = (uint8_t)(lz4f_xxh32(h + 4, 10, 0) >> 8);
}

// hdr = 1: a framed stream (frame byte first).  hdr = 0: a segment of whole
// blocks for one shard of a multi-GPU job (no frame byte).  frame_out: a
// standard LZ4 frame of the same parse instead (hdr = 1).
int run(lz4r_ctx *c, const void *d_in, size_t n, void *d_out, size_t cap,
        void *d_len, int hdr, void *stream, bool frame_out = false) {
  if (!c || !d_in || !d_out || !d_len) return LZ4R_ERR_ARG;
  if (hdr && n < (size_t)kBlk) return LZ4R_ERR_TOO_SMALL;
  if (n == 0 || n > kMaxInput) return LZ4R_ERR_ARG;
  const size_t nb = (n + kBlk - 1) / kBlk;
  const size_t nchunks = (nb + kChunk - 1) / kChunk;
  int rc = ensure_scratch(c, nb);
  if (rc != LZ4R_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool timed = c->timing;
  lz4r_ctx::timed_set *ts = nullptr;
  if (timed && (rc = next_timed_set(c, nchunks, &ts)) != LZ4R_OK) return rc;
  // A timed call's events ride on its kernels' own dispatch packets
  // (hipExtLaunchKernelGGL: start / stop timestamps of the dispatch), so
  // timing adds no marker packet between the kernels: call = the first
  // lz4_tiles start .. the last lz4_emit stop.
  auto ev = [&](hipEvent_t e) { return timed ? e : nullptr; };
  const uint8_t *in = static_cast<const uint8_t *>(d_in);
  uint64_t fh0 = 0, fh1 = 0;           // the frame header, as lz4f_scan takes it
  if (frame_out) {
    uint8_t h[kFrameHdr];
    frame_header(n, h);
    for (int i = 0; i < kFrameHdr; ++i) (i < 8 ? fh0 : fh1) |= (uint64_t)h[i] << (8 * (i & 7));
  }
  // the block scratch: cap_slots heads of kHead bytes, then the overflow slots
  uint8_t *const ovfs = c->slots + c->cap_slots * (size_t)kHead;
  for (size_t k = 0; k < nchunks; ++k) {
    const size_t b0 = k * kChunk;                      // first block of the chunk
    const size_t nbc = std::min(kChunk, nb - b0);
    const size_t b1 = b0 + nbc;
    const uint32_t last_n = (uint32_t)(b1 == nb ? n - (nb - 1) * kBlk : kBlk);
    // a run of kTileRun consecutive blocks per workgroup (lz4r_tiles.h); the
    // hardware dispatcher balances the runs' uneven cost (a static
    // grid-stride split of the whole launch leaves a tail)
    // runs, then blocks, per XCD slice
    const uint32_t runs = (uint32_t)((nbc + 8 * kTileRun - 1) / (8 * kTileRun));
    const uint32_t per = runs * kTileRun;
    hipEvent_t t0 = timed ? (k == 0 ? ts->a : ts->tiles[2 * k]) : nullptr;   // chunk 0 starts the call
    hipEvent_t t1 = timed ? ts->tiles[2 * k + 1] : nullptr;
    // (every chunk starts 300 b0 bytes in: a multiple of 4)
    const auto tiles = ((uintptr_t)in & 3) == 0 ? lz4_tiles<true> : lz4_tiles<false>;
    hipExtLaunchKernelGGL(tiles, dim3(8 * runs), dim3(64), 0, s, t0, t1, 0u, in + b0 * kBlk,
                          (uint32_t)nbc, per, last_n, c->slots, ovfs, c->bsizes + b0, c->status);
    if (frame_out) {
      // the records as a standard frame (lz4r_frame.h): a data block per scan
      // group; its stream offset takes the place of the group's first block's
      // in boff (a frame call leaves no per-block arrays)
      const size_t g0 = b0 / kGT, ng = (nbc + kGT - 1) / kGT;
      const bool last = k + 1 == nchunks;
      hipLaunchKernelGGL(lz4f_sizes, dim3((unsigned)ng), dim3(64 * kFW), 0, s,
                         (const uint8_t *)c->slots, (const uint8_t *)ovfs, (uint32_t)nbc, last_n,
                         c->boff + g0);
      hipLaunchKernelGGL(lz4f_scan, dim3(1), dim3(1024), 0, s, c->boff + g0, ng, k == 0 ? 1 : 0,
                         last ? 1 : 0, c->status, static_cast<uint64_t *>(d_len), c->verdict,
                         static_cast<uint8_t *>(d_out), (uint64_t)cap, fh0, fh1);
      hipExtLaunchKernelGGL(lz4f_emit, dim3((unsigned)ng), dim3(64 * kFW), 0, s, nullptr,
                            last ? ev(ts ? ts->c : nullptr) : nullptr, 0u, in + b0 * kBlk,
                            (const uint8_t *)c->slots, (const uint8_t *)ovfs, (uint32_t)nbc, last_n,
                            (const uint64_t *)(c->boff + g0), static_cast<uint8_t *>(d_out),
                            (uint64_t)cap);
      continue;
    }
    // the chunk's own groups and partials (a chunk starts on a partial)
    const size_t p0 = b0 / kPart, np = (nbc + kPart - 1) / kPart;
    const size_t g0 = b0 / kGT, ng = (nbc + kGT - 1) / kGT;
    const int frame = hdr && k == 0 && cap > 0 ? (int)(uint8_t)nb : -1;
    hipLaunchKernelGGL(lz4_scan_reduce16, dim3((unsigned)np), dim3(256), 0, s,
                       (const uint16_t *)(c->bsizes + b0), (uint32_t)nbc, c->gsum + g0,
                       c->part + p0);
    hipLaunchKernelGGL(lz4_scan_partials_frame, dim3(1), dim3(1024), 0, s, c->part + p0, np,
                       (uint64_t)hdr, k == 0 ? 1 : 0, k + 1 == nchunks ? 1 : 0, c->status,
                       static_cast<uint64_t *>(d_len), c->verdict, static_cast<uint8_t *>(d_out),
                       frame);
    // what every lz4_emit workgroup of the launch shares: the workgroups that
    // have blocks, and how many of them an XCD takes
    const uint32_t nwg = (uint32_t)(ng * kGSplit), wper = (nwg + 7) / 8;
    hipExtLaunchKernelGGL(lz4_emit, dim3(8 * wper), dim3(64 * kEW), 0, s, nullptr,
                          k + 1 == nchunks ? ev(ts ? ts->c : nullptr) : nullptr, 0u, in + b0 * kBlk,
                          (const uint8_t *)c->slots, (const uint8_t *)ovfs,
                          (const uint16_t *)(c->bsizes + b0), (uint32_t)nbc, nwg, wper,
                          (const uint32_t *)(c->gsum + g0), (const uint64_t *)(c->part + p0),
                          static_cast<uint8_t *>(d_out), (uint64_t)cap, (uint32_t)hdr, last_n,
                          c->boff + b0);
  }
  if (timed) ++c->timed_calls;
  c->last_nb = frame_out ? 0 : nb;
  c->last_frame = frame_out;
  c->checkable = true;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess && getenv("LZ4R_DEBUG"))
    fprintf(stderr, "lz4r: %s\n", hipGetErrorString(e));
  return e == hipSuccess ? LZ4R_OK : LZ4R_ERR_HIP;
}

// the first `count` entries of a per-block array of the last call -> dst
// (host or device memory), synchronously
int copy_per_block(const lz4r_ctx *c, const void *src, size_t elem, void *dst, size_t count,
                   void *stream) {
  if (!dst || count > c->last_nb) return LZ4R_ERR_ARG;
  if (count == 0) return LZ4R_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(dst, src, count * elem, hipMemcpyDefault, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return LZ4R_ERR_HIP;
  return LZ4R_OK;
}

}  // namespace

extern "C" {

int lz4r_ctx_create(lz4r_ctx **out) {
  if (!out) return LZ4R_ERR_ARG;
  lz4r_ctx *c = new (std::nothrow) lz4r_ctx();
  if (!c) return LZ4R_ERR_NOMEM;
  if (hipGetDevice(&c->device) != hipSuccess ||
      hipMalloc(&c->len, 3 * sizeof(uint64_t)) != hipSuccess ||
      hipMemset(c->len, 0, 3 * sizeof(uint64_t)) != hipSuccess) {
    lz4r_ctx_destroy(c);
    return LZ4R_ERR_HIP;
  }
  c->status = reinterpret_cast<uint32_t *>(c->len + 1);
  c->verdict = c->len + 2;
  *out = c;
  return LZ4R_OK;
}

void lz4r_ctx_destroy(lz4r_ctx *c) {
  if (!c) return;
  free_scratch(c);
  (void)hipFree(c->len);
  destroy_events(c);
  delete c;
}

size_t lz4r_nblocks(size_t n) { return (n + kBlk - 1) / kBlk; }

size_t lz4r_launch_chunk_blocks(void) { return kChunk; }

size_t lz4r_compress_bound(size_t n) { return 1 + lz4r_nblocks(n) * (size_t)LZ4R_BLOCK_BOUND; }

int lz4r_compress_async(lz4r_ctx *c, const void *d_in, size_t n, void *d_out, size_t cap,
                        void *d_len, void *stream) {
  return run(c, d_in, n, d_out, cap, d_len, 1, stream);
}

int lz4r_compress_segment_async(lz4r_ctx *c, const void *d_in, size_t n, void *d_out,
                                size_t cap, void *d_len, int final_shard, void *stream) {
  if (!c || !d_len) return LZ4R_ERR_ARG;
  // a non-final shard must end on the 300-B grid, or the blocks after it
  // (and so the concatenated stream) would differ from the single-GPU one
  if (!final_shard && n % kBlk != 0) return LZ4R_ERR_ARG;
  if (n == 0) {                      // an empty shard (more ranks than blocks)
    c->last_nb = 0;
    c->last_frame = false;
    c->checkable = false;     // nothing launched: lz4r_check reports OK
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->timing) {          // a timed call of no launches
      lz4r_ctx::timed_set *ts = nullptr;
      const int rc = next_timed_set(c, 0, &ts);
      if (rc != LZ4R_OK) return rc;
      (void)hipEventRecord(ts->a, s);
      (void)hipEventRecord(ts->c, s);
      ++c->timed_calls;
    }
    return hipMemsetAsync(d_len, 0, sizeof(uint64_t), s) == hipSuccess ? LZ4R_OK : LZ4R_ERR_HIP;
  }
  return run(c, d_in, n, d_out, cap, d_len, 0, stream);
}

// run() into the context's own length word, then the length read back
static int run_device(lz4r_ctx *c, const void *d_in, size_t n, void *d_out, size_t cap,
                      size_t *out_len, void *stream, bool frame_out) {
  if (!c || !out_len) return LZ4R_ERR_ARG;
  int rc = run(c, d_in, n, d_out, cap, c->len, 1, stream, frame_out);
  if (rc != LZ4R_OK) return rc;
  uint64_t got = 0;                    // the length, with the corrupt flag: one read-back
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemcpyAsync(&got, c->len, sizeof(got), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    if (getenv("LZ4R_DEBUG")) fprintf(stderr, "lz4r: %s\n", hipGetErrorString(e));
    return LZ4R_ERR_HIP;
  }
  *out_len = (size_t)(got & ~kLenCorrupt);
  if (got & kLenCorrupt) return LZ4R_ERR_CORRUPT;   // a corrupt bucket head
  return *out_len > cap ? LZ4R_ERR_CAPACITY : LZ4R_OK;
}

int lz4r_compress_device(lz4r_ctx *c, const void *d_in, size_t n, void *d_out, size_t cap,
                         size_t *out_len, void *stream) {
  return run_device(c, d_in, n, d_out, cap, out_len, stream, false);
}

// Per data block of N bytes: the u32 size, and a sequence expands the bytes
// it covers by at most L / 255 (a kept match adds 3 + its extensions and saves
// >= 4), the last run by its token and one more extension byte:
// 4 + N + N / 255 + 2 <= N + 81 for N <= 19,200.  Header 15, EndMark 4.
size_t lz4r_frame_bound(size_t n) {
  return 19 + n + 100 * ((n + (size_t)kFrameIn - 1) / (size_t)kFrameIn);
}

int lz4r_compress_frame_async(lz4r_ctx *c, const void *d_in, size_t n, void *d_out, size_t cap,
                              void *d_len, void *stream) {
  return run(c, d_in, n, d_out, cap, d_len, 1, stream, true);
}

int lz4r_compress_frame_device(lz4r_ctx *c, const void *d_in, size_t n, void *d_out, size_t cap,
                               size_t *out_len, void *stream) {
  return run_device(c, d_in, n, d_out, cap, out_len, stream, true);
}

int lz4r_block_matches_device(const void *d_in, size_t n, void *d_matches, void *stream) {
  if (!d_in || !d_matches || n == 0 || n > kMaxInput) return LZ4R_ERR_ARG;
  const size_t nb = (n + kBlk - 1) / kBlk;
  const uint8_t *in = static_cast<const uint8_t *>(d_in);
  uint32_t *mo = static_cast<uint32_t *>(d_matches);
  // a grid of 64-lane workgroups stays under HIP's 2^32 work-items: launch
  // chunks of kChunk blocks, as run() does
  for (size_t b0 = 0; b0 < nb; b0 += kChunk) {
    const size_t nbc = std::min(kChunk, nb - b0);
    const uint32_t last_n = (uint32_t)(b0 + nbc == nb ? n - (nb - 1) * kBlk : kBlk);
    hipLaunchKernelGGL(lz4_matches, dim3((unsigned)nbc), dim3(64), 0,
                       static_cast<hipStream_t>(stream), in + b0 * kBlk, (uint32_t)nbc, last_n,
                       mo + b0 * kBlk);
  }
  return hipGetLastError() == hipSuccess ? LZ4R_OK : LZ4R_ERR_HIP;
}

int lz4r_window_matches_device(const void *d_in, size_t n, void *d_matches, void *stream) {
  if (!d_in || !d_matches || n == 0 || n > 0xFFFFFFFFull) return LZ4R_ERR_ARG;
  constexpr size_t kPosChunk = size_t(1) << 26;       // 2^24 workgroups of 256 per launch
  for (size_t p0 = 0; p0 < n; p0 += kPosChunk) {
    const size_t np = std::min(kPosChunk, n - p0);
    hipLaunchKernelGGL(lz4_window_matches, dim3((unsigned)((np + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_in),
                       (uint32_t)n, (uint32_t)p0, static_cast<uint32_t *>(d_matches));
  }
  return hipGetLastError() == hipSuccess ? LZ4R_OK : LZ4R_ERR_HIP;
}

int lz4r_copy_block_sizes(const lz4r_ctx *c, void *dst, size_t count, void *stream) {
  if (!c || c->last_frame) return LZ4R_ERR_ARG;
  return copy_per_block(c, c->bsizes, sizeof(uint16_t), dst, count, stream);
}

int lz4r_copy_block_offsets(const lz4r_ctx *c, void *dst, size_t count, void *stream) {
  if (!c || c->last_frame) return LZ4R_ERR_ARG;
  return copy_per_block(c, c->boff, sizeof(uint64_t), dst, count, stream);
}

int lz4r_block_offsets_device(const lz4r_ctx *c, const void **d_offsets, size_t *count) {
  if (!c || !d_offsets || !count || c->last_frame) return LZ4R_ERR_ARG;
  *d_offsets = c->boff;
  *count = c->last_nb;
  return LZ4R_OK;
}

// the host-buffer forms: copy in, compress (natively or as a frame), copy out
static int compress_host(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len,
                         bool frame_out) {
  if (!in || !out || !out_len) return LZ4R_ERR_ARG;
  if (n < (size_t)kBlk) return LZ4R_ERR_TOO_SMALL;
  lz4r_ctx *c = nullptr;
  int rc = lz4r_ctx_create(&c);
  if (rc != LZ4R_OK) return rc;
  void *din = nullptr, *dout = nullptr;
  const size_t dcap = frame_out ? lz4r_frame_bound(n) : lz4r_compress_bound(n);
  if (hipMalloc(&din, n + 16) != hipSuccess || hipMalloc(&dout, dcap) != hipSuccess) {
    (void)hipFree(din);
    lz4r_ctx_destroy(c);
    return LZ4R_ERR_NOMEM;
  }
  if (hipMemcpy(din, in, n, hipMemcpyHostToDevice) != hipSuccess) rc = LZ4R_ERR_HIP;
  size_t got = 0;
  if (rc == LZ4R_OK) rc = run_device(c, din, n, dout, dcap, &got, nullptr, frame_out);
  if (rc == LZ4R_OK) {
    *out_len = got;
    if (got > cap) rc = LZ4R_ERR_CAPACITY;
    else if (hipMemcpy(out, dout, got, hipMemcpyDeviceToHost) != hipSuccess) rc = LZ4R_ERR_HIP;
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  lz4r_ctx_destroy(c);
  return rc;
}

int lz4r_compress(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len) {
  return compress_host(in, n, out, cap, out_len, false);
}

int lz4r_compress_frame(const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len) {
  return compress_host(in, n, out, cap, out_len, true);
}

int lz4r_check(lz4r_ctx *c, void *stream) {
  if (!c) return LZ4R_ERR_ARG;
  if (!c->checkable) return LZ4R_OK;     // no launch yet (or an empty segment)
  uint64_t v = 0;                        // the context's own verdict word
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(&v, c->verdict, sizeof(v), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return LZ4R_ERR_HIP;
  return v ? LZ4R_ERR_CORRUPT : LZ4R_OK;
}

int lz4r_set_timing(lz4r_ctx *c, int enable) {
  if (!c) return LZ4R_ERR_ARG;
  c->timing = enable != 0;
  if (c->timing) c->timed_calls = 0;
  return LZ4R_OK;
}

int lz4r_last_timing(lz4r_ctx *c, float *ms_call, float *ms_match) {
  if (!c || c->timed_calls == 0) return LZ4R_ERR_ARG;
  float a = 0.f, b = 0.f;
  const int rc = timed_ms(c->tsets[(c->timed_calls - 1) % kTimedCalls], &a, &b);
  if (rc != LZ4R_OK) return rc;
  if (ms_call) *ms_call = a;
  if (ms_match) *ms_match = b;
  return LZ4R_OK;
}

int lz4r_timed_calls(lz4r_ctx *c, size_t max, float *ms_call, float *ms_match, size_t *count) {
  if (!c || !count || (max && (!ms_call || !ms_match))) return LZ4R_ERR_ARG;
  // the newest min(calls, ring, max) calls, oldest first
  const size_t n = std::min(std::min(c->timed_calls, kTimedCalls), max);
  for (size_t j = 0; j < n; ++j) {
    const size_t i = (c->timed_calls - n + j) % kTimedCalls;
    const int rc = timed_ms(c->tsets[i], &ms_call[j], &ms_match[j]);
    if (rc != LZ4R_OK) return rc;
  }
  *count = n;
  return LZ4R_OK;
}

const char *lz4r_strerror(int code) {
  switch (code) {
    case LZ4R_OK: return "ok";
    case LZ4R_ERR_ARG: return "invalid argument";
    case LZ4R_ERR_TOO_SMALL: return "input shorter than one 300-byte block";
    case LZ4R_ERR_CAPACITY: return "output buffer too small";
    case LZ4R_ERR_HIP: return "HIP runtime error";
    case LZ4R_ERR_NOMEM: return "device allocation failed";
    case LZ4R_ERR_CORRUPT: return "corrupt stream";
    default: return "unknown error";
  }
}

}  // extern "C"
