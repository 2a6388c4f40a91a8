// lz4r_gpudec.hip -- block-parallel MI355X decoder of the reference's "LZ4"
// stream (the bytes lz4r_compress / lz4_encode write).
//
// The reference decoder (LZ4_decode / interpret_frame, LZ4.c:937-1121) walks
// the stream serially and mis-parses >= 256 blocks and literal runs >= 271.
// Here every 300-byte block is decoded independently into its fixed output
// slot [300 b, 300 b + 300).  Block boundaries come from the compressor's
// per-block offsets (lz4r_copy_block_offsets): the format itself cannot be
// split in parallel (the u16 size field over-counts the truncated-length
// sequences, LZ4.c:569-575); a bare stream's are found on the device first.
//
// Mapping: one LANE per block, 32 consecutive blocks per wave (a wave per
// block would issue every serial parsing step as a full wave instruction).
// The walk is issue-bound (the divergent per-lane loop), so the kernel keeps
// LDS small for occupancy and the loop free of exec-mask bookkeeping.  One
// translation unit; the includes below are in the kernels' definition order:
//
//   lz4r_dec_layout.h  what the kernels and the host share: the block grid,
//                      the bare-stream chunking, control words and scratch
//   lz4r_dec_parse.h   a lane's block parsers (decode_block_plain, then the
//                      general decode_block) and their byte / slot accessors
//   lz4r_dec_blocks.h  lz4_decode_blocks: 32 blocks per wave into LDS slots,
//                      the wave's output stored contiguously
//   lz4r_dec_bare.h    lz4_bare_*: candidates, walk, check / fix, scan,
//                      offsets and the gate of a bare stream; lz4_decode_init
//   wave64.h           u32x4
//   below              the host side: the scratch pool, one bare-stream pass
//                      (a decode, or the index of lz4r_stream_index_device),
//                      the C ABI
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "../../include/lz4r.h"
#include "wave64.h"
#include "lz4r_scratch.h"
#include "lz4r_dec_layout.h"
#include "lz4r_dec_parse.h"
#include "lz4r_dec_blocks.h"
#include "lz4r_dec_bare.h"

extern "C" int lz4r_decompress_device(const void *d_in, size_t in_len, const void *d_block_offsets,
                                      size_t nb, void *d_out, size_t out_cap, void *d_result,
                                      void *stream) {
  if (!d_in || !d_block_offsets || !d_out || !d_result || nb == 0 || in_len < 4 ||
      nb > 0x7fffffffULL * kBPW)
    return LZ4R_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(lz4_decode_init, dim3(1), dim3(1), 0, s,
                     static_cast<unsigned long long *>(d_result));
  const unsigned grid = (unsigned)((nb + kBPW - 1) / kBPW);
  hipLaunchKernelGGL(lz4_decode_blocks, dim3(grid), dim3(kLanes), 0, s,
                     static_cast<const uint8_t *>(d_in), in_len,
                     static_cast<const uint64_t *>(d_block_offsets), nb,
                     static_cast<uint8_t *>(d_out), out_cap,
                     static_cast<unsigned long long *>(d_result), nullptr, nullptr);
  return hipGetLastError() == hipSuccess ? LZ4R_OK : LZ4R_ERR_HIP;
}

namespace {

// The bare path's per-call scratch comes from a pool of the library's own
// per device that keeps its memory (release threshold: all): from the
// default pool, whose threshold is 0, every call re-mapped its ~34 MB per GiB
// of stream after the previous call's synchronise returned it.
hipMemPool_t scratch_pool() {
  static std::mutex mu;
  static std::map<int, hipMemPool_t> pools;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> g(mu);
  auto it = pools.find(dev);
  if (it != pools.end()) return it->second;
  hipMemPoolProps props = {};
  props.allocType = hipMemAllocationTypePinned;
  props.location.type = hipMemLocationTypeDevice;
  props.location.id = dev;
  hipMemPool_t p = nullptr;
  if (hipMemPoolCreate(&p, &props) != hipSuccess) return nullptr;
  uint64_t keep = ~0ull;
  (void)hipMemPoolSetAttribute(p, hipMemPoolAttrReleaseThreshold, &keep);
  pools[dev] = p;
  return p;
}

}  // namespace

// (declared in lz4r_scratch.h: the frame decoder, lz4f_gpudec.hip, allocates from the same pool)
hipError_t lz4r_scratch_alloc(void **ptr, size_t bytes, hipStream_t s) {
  hipMemPool_t p = scratch_pool();
  return p ? hipMallocFromPoolAsync(ptr, bytes, p, s) : hipMallocAsync(ptr, bytes, s);
}

namespace {

hipError_t scratch_alloc(void **ptr, size_t bytes, hipStream_t s) {
  return lz4r_scratch_alloc(ptr, bytes, s);
}

// the control words read back after the decode -> the call's return code and
// *out_len: the gate's verdict first, then a failed block, then the capacity
// nb_out (an index call: the blocks are checked and nothing is stored): the
// block count too, and an output that holds nothing is no error
int bare_verdict(const unsigned long long *h, size_t out_cap, size_t *out_len, size_t *nb_out) {
  if (h[kCtlGate] == kGateCorrupt) return LZ4R_ERR_CORRUPT;
  if (nb_out) *nb_out = (size_t)h[kCtlNb];
  if (h[kCtlGate] == kGateCapacity) {                 // at least this much output
    *out_len = (size_t)(h[kCtlNb] - 1) * kBlk + 1;
    return LZ4R_ERR_CAPACITY;
  }
  if (h[kCtlFail] != ~0ull) return LZ4R_ERR_CORRUPT;
  *out_len = (size_t)h[kCtlLen];
  return !nb_out && h[kCtlLen] > out_cap ? LZ4R_ERR_CAPACITY : LZ4R_OK;
}

// One pass of the bare-stream decode in mode kExact; returns LZ4R_OK, or
// LZ4R_ERR_CORRUPT when the chain or a block does not hold together.
// nb_cap > 0 (the most blocks out_cap can hold; S.boff has as many), one host
// read-back: the block count stays on the device, the decoder's grid is sized
// for nb_cap and lz4_bare_gate decides on the device whether anything is
// decoded.  nb_cap 0 (an out_cap far above the stream's possible output): the
// block count is read back first and sizes both.
// index (lz4r_stream_index_device): the offsets go to the caller's array of
// nb_cap entries (0: the count is read back and is the answer), *nb_out takes
// the block count, and out / out_cap are nullptr / 0: lz4_decode_blocks then
// checks every block and stores nothing.
template <bool kExact>
int bare_pass(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, const BareScratch &S,
              size_t nb_cap, size_t *out_len, hipStream_t s, uint64_t *index = nullptr,
              size_t *nb_out = nullptr) {
  const size_t nchunks = S.nchunks;
  const unsigned ng = (unsigned)S.ng;
  hipLaunchKernelGGL(lz4_bare_cand, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, s, in,
                     in_len, nchunks, S.cand);
  hipLaunchKernelGGL(lz4_bare_walk<kExact>, dim3(ng), dim3(64), 0, s, in, in_len, nchunks, S.cand,
                     S.cnt, S.exitp, S.gsum, S.lists, S.lok);
  if (hipMemsetAsync(S.nmis, 0, sizeof(unsigned int), s) != hipSuccess) return LZ4R_ERR_HIP;
  hipLaunchKernelGGL(lz4_bare_check, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, s,
                     in_len, nchunks, S.cand, S.exitp, S.nmis, S.mis);
  hipLaunchKernelGGL(lz4_bare_fix<kExact>, dim3(1), dim3(64), 0, s, in, in_len, nchunks, S.cand,
                     S.cnt, S.exitp, S.gsum, S.nmis, S.mis, S.ctl + kCtlStatus, S.lok);
  hipLaunchKernelGGL(lz4_bare_scan, dim3(1), dim3(1024), 0, s, S.gsum, (size_t)ng, S.gbase,
                     S.ctl + kCtlNb);
  uint64_t *boff = index ? index : S.boff, *own = nullptr;
  unsigned long long h[kCtlWords] = {};
  if (nb_cap == 0) {
    // no useful bound from out_cap: read the block count (and the status) first
    if (hipMemcpyAsync(h, S.ctl, (kCtlStatus + 1) * sizeof(*h), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return LZ4R_ERR_HIP;
    if (h[kCtlStatus] != 0 || h[kCtlNb] == 0) return LZ4R_ERR_CORRUPT;
    nb_cap = (size_t)h[kCtlNb];
    if (index) {                                     // no room at all: the count is the answer
      *nb_out = nb_cap;
      return LZ4R_ERR_CAPACITY;
    }
    if (scratch_alloc(reinterpret_cast<void **>(&own), nb_cap * sizeof(uint64_t), s) !=
        hipSuccess)
      return LZ4R_ERR_NOMEM;
    boff = own;
  }
  hipLaunchKernelGGL(lz4_bare_offsets<kExact>, dim3(ng), dim3(64), 0, s, in, in_len, nchunks,
                     S.cand, S.cnt, S.gbase, boff, (uint64_t)nb_cap, S.lists, S.lok);
  hipLaunchKernelGGL(lz4_bare_gate, dim3(1), dim3(1), 0, s, in, S.ctl, (uint64_t)nb_cap);
  hipLaunchKernelGGL(lz4_decode_blocks, dim3((unsigned)((nb_cap + kBPW - 1) / kBPW)),
                     dim3(kLanes), 0, s, in, in_len, static_cast<const uint64_t *>(boff), nb_cap,
                     out, out_cap, S.ctl + kCtlLen, S.ctl + kCtlNb, S.ctl + kCtlGate);
  if (own) (void)hipFreeAsync(own, s);
  if (hipMemcpyAsync(h, S.ctl, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return LZ4R_ERR_HIP;
  return bare_verdict(h, out_cap, out_len, nb_out);
}

}  // namespace

extern "C" int lz4r_decompress_stream_device(const void *d_in, size_t in_len, void *d_out,
                                             size_t out_cap, size_t *out_len, void *stream) {
  if (!d_in || !d_out || !out_len) return LZ4R_ERR_ARG;
  *out_len = 0;
  if (in_len < 9) return LZ4R_ERR_CORRUPT;          // a frame byte and one 8-byte block at least
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *in = static_cast<const uint8_t *>(d_in);
  uint8_t *out = static_cast<uint8_t *>(d_out);
  const size_t nchunks = (in_len - 1 + kChunkB - 1) / kChunkB;
  // blocks the output can hold (every block but the last decodes to 300
  // bytes): the size of the offsets array and of the decoder's grid -- when
  // that is tighter than what the stream can hold (a block is >= 8 bytes);
  // else (an oversized out_cap) the count is read back first (nb_cap 0)
  const size_t nb_out = out_cap / kBlk + 1, nb_in = (in_len - 1) / 8 + 1;
  const size_t nb_cap = nb_out <= nb_in ? nb_out : 0;
  BareScratch S = bare_scratch_layout(nchunks, nb_cap);
  uint8_t *scr = nullptr;
  if (scratch_alloc(reinterpret_cast<void **>(&scr), S.bytes, s) != hipSuccess)
    return LZ4R_ERR_NOMEM;
  S.bind(scr);
  // fast mode (block length = its size field); the exact mode parses every
  // block and is needed only for streams with truncated matches
  int rc = bare_pass<false>(in, in_len, out, out_cap, S, nb_cap, out_len, s);
  if (rc == LZ4R_ERR_CORRUPT) rc = bare_pass<true>(in, in_len, out, out_cap, S, nb_cap, out_len, s);
  (void)hipFreeAsync(scr, s);
  if (hipStreamSynchronize(s) != hipSuccess) return LZ4R_ERR_HIP;
  return rc;
}

extern "C" int lz4r_stream_index_device(const void *d_in, size_t in_len, void *d_block_offsets,
                                        size_t cap_blocks, size_t *nb, size_t *decoded_len,
                                        void *stream) {
  if (!d_in || !d_block_offsets || !nb || !decoded_len ||
      (reinterpret_cast<uintptr_t>(d_block_offsets) & 7) != 0)
    return LZ4R_ERR_ARG;
  *nb = 0;
  *decoded_len = 0;
  if (in_len < 9) return LZ4R_ERR_CORRUPT;          // a frame byte and one 8-byte block at least
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *in = static_cast<const uint8_t *>(d_in);
  uint64_t *index = static_cast<uint64_t *>(d_block_offsets);
  const size_t nchunks = (in_len - 1 + kChunkB - 1) / kChunkB;
  // never more entries than the stream can hold blocks (a block is >= 8
  // bytes): the decoder's grid is sized by them
  const size_t nb_cap = std::min(cap_blocks, (in_len - 1) / 8 + 1);
  BareScratch S = bare_scratch_layout(nchunks, 0);  // the offsets array is the caller's
  uint8_t *scr = nullptr;
  if (scratch_alloc(reinterpret_cast<void **>(&scr), S.bytes, s) != hipSuccess)
    return LZ4R_ERR_NOMEM;
  S.bind(scr);
  int rc = bare_pass<false>(in, in_len, nullptr, 0, S, nb_cap, decoded_len, s, index, nb);
  if (rc == LZ4R_ERR_CORRUPT)
    rc = bare_pass<true>(in, in_len, nullptr, 0, S, nb_cap, decoded_len, s, index, nb);
  (void)hipFreeAsync(scr, s);
  if (hipStreamSynchronize(s) != hipSuccess) return LZ4R_ERR_HIP;
  if (rc != LZ4R_OK) *decoded_len = 0;
  if (rc != LZ4R_OK && rc != LZ4R_ERR_CAPACITY) *nb = 0;
  return rc;
}

extern "C" int lz4r_decompress_stream(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap,
                                      size_t *out_len) {
  if (!in || !out || !out_len) return LZ4R_ERR_ARG;
  void *din = nullptr, *dout = nullptr;
  if (hipMalloc(&din, in_len ? in_len : 1) != hipSuccess ||
      hipMalloc(&dout, cap ? cap : 1) != hipSuccess) {
    (void)hipFree(din);
    return LZ4R_ERR_NOMEM;
  }
  int rc = hipMemcpy(din, in, in_len, hipMemcpyHostToDevice) == hipSuccess ? LZ4R_OK
                                                                          : LZ4R_ERR_HIP;
  if (rc == LZ4R_OK) rc = lz4r_decompress_stream_device(din, in_len, dout, cap, out_len, nullptr);
  if (rc == LZ4R_OK && hipMemcpy(out, dout, *out_len, hipMemcpyDeviceToHost) != hipSuccess)
    rc = LZ4R_ERR_HIP;
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}
