// lz4f_gpudec.hip -- lz4r_frame_decompress_device: standard LZ4 frames decoded
// on the GPU, block-parallel wherever the format allows it (include/lz4r.h has
// the contract; host/lz4f_decode.c is the host decoder it agrees with).
//
//   lz4f_parse.h   what a frame means, shared with the host
//   lz4f_dec.h     the kernels
//   below          the host side: one scratch allocation, two read-backs for every input
//
//   walk -> read-back 1 (the counts; the index's size if the first guess was short)
//        -> block checksums -> sizes -> scan -> blocks -> content checksums
//        -> read-back 2 (the total, the verdict)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/lz4r.h"
#include "lz4r_scratch.h"
#include "lz4f_dec.h"

namespace {

// the call's scratch: the control words, then the block index with the
// blocks' offsets and sizes, then the frame table
struct FrameScratch {
  size_t cap_blocks, cap_frames, bytes;
  unsigned long long *ctl;
  Lz4fBlock *blocks;
  uint64_t *off;
  Lz4fFrame *frames;
  uint32_t *sizes;
  FrameScratch(size_t nb, size_t nf) : cap_blocks(nb), cap_frames(nf) {
    bytes = kFWords * sizeof(*ctl) + nb * (sizeof(*blocks) + sizeof(*off)) +
            nf * sizeof(*frames) + nb * sizeof(*sizes);
  }
  void bind(uint8_t *p) {
    ctl = reinterpret_cast<unsigned long long *>(p);
    blocks = reinterpret_cast<Lz4fBlock *>(ctl + kFWords);
    off = reinterpret_cast<uint64_t *>(blocks + cap_blocks);
    frames = reinterpret_cast<Lz4fFrame *>(off + cap_blocks);
    sizes = reinterpret_cast<uint32_t *>(frames + cap_frames);
  }
};

// workgroups of kFWaves waves for n items, a wave each: no more than fill the
// chip (256 CUs of 8 workgroups); the kernels stride
unsigned item_grid(size_t n) {
  return (unsigned)std::min<size_t>((n + kFWaves - 1) / kFWaves, 2048);
}

}  // namespace

extern "C" int lz4r_frame_decompress_device(const void *d_in, size_t in_len, void *d_out,
                                            size_t out_cap, size_t *out_len, unsigned flags,
                                            void *stream) {
  if (!d_in || !out_len || (!d_out && out_cap)) return LZ4R_ERR_ARG;
  *out_len = 0;
  if (in_len == 0) return LZ4R_ERR_CORRUPT;           // no frame at all
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *in = static_cast<const uint8_t *>(d_in);
  uint8_t *out = static_cast<uint8_t *>(d_out);
  // Room for the index: 28 bytes a data block, 40 a frame.  The format's
  // minimum (4 bytes of input for a stored block of none) would make it seven
  // times the input, so the first walk gets room for blocks of 1 KiB and frames
  // of 64 KiB on average (at least 4,096 and 64): 1/36 of the input.  The walk
  // counts everything, its counts are the first read-back, and an input with
  // more entries than that is walked again into an index of exactly their
  // number (no further read-back).
  size_t cap_blocks = std::min(in_len / 4 + 1, in_len / 1024 + 4096);
  size_t cap_frames = std::min(in_len / 11 + 1, in_len / 65536 + 64);
  unsigned long long h[kFWords] = {};
  uint8_t *scr = nullptr;
  FrameScratch S(cap_blocks, cap_frames);
  auto walk = [&]() {
    if (lz4r_scratch_alloc(reinterpret_cast<void **>(&scr), S.bytes, s) != hipSuccess) return false;
    S.bind(scr);
    hipLaunchKernelGGL(lz4f_walk, dim3(1), dim3(64), 0, s, in, in_len, S.blocks, S.cap_blocks,
                       S.frames, S.cap_frames, S.ctl);
    return true;
  };
  auto read_back = [&]() {
    return hipMemcpyAsync(h, S.ctl, sizeof(h), hipMemcpyDeviceToHost, s) == hipSuccess &&
           hipStreamSynchronize(s) == hipSuccess;
  };
  if (!walk()) return LZ4R_ERR_NOMEM;
  int rc = read_back() ? LZ4R_OK : LZ4R_ERR_HIP;                       // read-back 1: the counts
  if (rc == LZ4R_OK && h[kFStatus] != 0) rc = LZ4R_ERR_CORRUPT;
  if (rc == LZ4R_OK && (h[kFNb] > S.cap_blocks || h[kFNf] > S.cap_frames)) {
    (void)hipFreeAsync(scr, s);
    scr = nullptr;
    S = FrameScratch(std::max<size_t>((size_t)h[kFNb], 1), std::max<size_t>((size_t)h[kFNf], 1));
    if (!walk()) return LZ4R_ERR_NOMEM;
  }
  if (rc == LZ4R_OK) {
    const size_t nb = (size_t)h[kFNb], nf = (size_t)h[kFNf];
    if (nb != 0) {
      hipLaunchKernelGGL(lz4f_xxh32_items<false>, dim3(item_grid(nb)), dim3(kFThreads), 0, s, in,
                         in_len, S.blocks, S.frames, S.off, out, out_cap, S.ctl);
      hipLaunchKernelGGL(lz4f_dec_sizes, dim3(item_grid(nb)), dim3(kFThreads), 0, s, in, in_len,
                         S.blocks, S.sizes, S.off, S.ctl);
    }
    hipLaunchKernelGGL(lz4f_dec_scan, dim3(1), dim3(1024), 0, s, S.off, S.frames, S.ctl);
    // the decode stages ask on the device whether the output fits and nothing
    // is corrupt so far (decode_gate): no read-back between
    if (nb != 0) {
      hipLaunchKernelGGL(lz4f_dec_blocks, dim3(item_grid(nb)), dim3(kFThreads), 0, s, in, in_len,
                         S.blocks, S.frames, S.sizes, S.off, out, out_cap, S.ctl);
      if (h[kFNsum] != 0 && !(flags & LZ4R_FRAME_NO_CONTENT_CHECKSUM))
        hipLaunchKernelGGL(lz4f_xxh32_items<true>, dim3(item_grid(nf)), dim3(kFThreads), 0, s, in,
                           in_len, S.blocks, S.frames, S.off, out, out_cap, S.ctl);
    }
    if (!read_back())                                                  // read-back 2: total, verdict
      rc = LZ4R_ERR_HIP;
    else if (h[kFStatus] != 0 || h[kFBad] != ~0ull)
      rc = LZ4R_ERR_CORRUPT;
    else if (h[kFTotal] > out_cap) {                  // exact, and nothing was written
      *out_len = (size_t)h[kFTotal];
      rc = LZ4R_ERR_CAPACITY;
    }
  }
  (void)hipFreeAsync(scr, s);
  if (hipGetLastError() != hipSuccess && rc == LZ4R_OK) rc = LZ4R_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess && rc == LZ4R_OK) rc = LZ4R_ERR_HIP;
  if (rc == LZ4R_OK) *out_len = (size_t)h[kFTotal];
  return rc;
}

extern "C" int lz4r_frame_decompress_gpu(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap,
                                         size_t *out_len, unsigned flags) {
  if (!in || !out_len || (!out && cap)) return LZ4R_ERR_ARG;
  *out_len = 0;
  if (in_len == 0) return LZ4R_ERR_CORRUPT;
  void *din = nullptr, *dout = nullptr;
  if (hipMalloc(&din, in_len) != hipSuccess || hipMalloc(&dout, cap ? cap : 1) != hipSuccess) {
    (void)hipFree(din);
    return LZ4R_ERR_NOMEM;
  }
  int rc = hipMemcpy(din, in, in_len, hipMemcpyHostToDevice) == hipSuccess ? LZ4R_OK
                                                                          : LZ4R_ERR_HIP;
  if (rc == LZ4R_OK) rc = lz4r_frame_decompress_device(din, in_len, dout, cap, out_len, flags, nullptr);
  if (rc == LZ4R_OK && *out_len &&
      hipMemcpy(out, dout, *out_len, hipMemcpyDeviceToHost) != hipSuccess)
    rc = LZ4R_ERR_HIP;
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}
