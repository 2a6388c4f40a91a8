// lz4r_read.hip -- random access into a compressed stream: lz4r_read_device
// decodes many byte ranges in one call, each from the 300-byte blocks it
// covers (the one thing the reference's independent blocks buy).  A
// translation unit of its own beside the decoder's (lz4r_gpudec.hip), sharing
// its per-lane parsers:
//
//   lz4r_dec_layout.h  the block grid (kBlk, kInMax, kBPW, kLanes)
//   lz4r_dec_parse.h   decode_block_plain / decode_block and their accessors
//   lz4r_dec_read.h    lz4_read_items: an item (one block of one read) per
//                      lane, the items' slices stored by the whole wave
//   below              the C ABI
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lz4r.h"
#include "lz4r_dec_layout.h"
#include "lz4r_dec_parse.h"
#include "lz4r_dec_read.h"

static_assert(sizeof(lz4r_read) == 24 && sizeof(ReadReq) == sizeof(lz4r_read),
              "lz4r_read is three u64");

extern "C" size_t lz4r_read_items(size_t max_len) {
  if (max_len > SIZE_MAX - (kBlk - 2)) return 0;     // (no such read: lz4r_read_device rejects it)
  return (max_len + (kBlk - 2)) / kBlk + 1;
}

extern "C" int lz4r_read_device(const void *d_in, size_t in_len, const void *d_block_offsets,
                                size_t nb, const void *d_reads, size_t nreads, size_t max_len,
                                void *d_out, size_t out_cap, void *d_result, void *stream) {
  if (!d_in || !d_block_offsets || !d_reads || !d_out || !d_result || nb == 0 || nreads == 0 ||
      max_len == 0 || in_len < 4)
    return LZ4R_ERR_ARG;
  if (((reinterpret_cast<uintptr_t>(d_block_offsets) | reinterpret_cast<uintptr_t>(d_reads) |
        reinterpret_cast<uintptr_t>(d_result)) & 7) != 0)
    return LZ4R_ERR_ARG;
  // a workgroup (one wave) per kBPW items, at most 2^31 - 1 of them
  const size_t K = lz4r_read_items(max_len);
  const size_t max_items = 0x7fffffffULL * kBPW;
  if (K == 0 || nreads > max_items / K) return LZ4R_ERR_ARG;
  const size_t items = nreads * K;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(lz4_read_init, dim3(1), dim3(1), 0, s,
                     static_cast<unsigned long long *>(d_result));
  hipLaunchKernelGGL(lz4_read_items, dim3((unsigned)((items + kBPW - 1) / kBPW)), dim3(kLanes), 0,
                     s, static_cast<const uint8_t *>(d_in), in_len,
                     static_cast<const uint64_t *>(d_block_offsets), nb,
                     static_cast<const ReadReq *>(d_reads), nreads, max_len, K,
                     static_cast<uint8_t *>(d_out), out_cap,
                     static_cast<unsigned long long *>(d_result));
  return hipGetLastError() == hipSuccess ? LZ4R_OK : LZ4R_ERR_HIP;
}
