// jpegr_dataset.h -- what the entry points of the dataset calls
// (jpegr_dataset_crop_tensor_device, jpegr_dataset_crop_resize_device:
// include/jpegr.h) agree on.  A dataset is a device table of
// jpegr_stream_desc, one per stream; a rectangle's `image` is a dataset-wide
// index g.  The call's first launch (jprs_dataset_crop_tensor_init in
// jpegr_stream.hip, jprs_dataset_crop_resize_init in jpegr_resize.hip) finds
// each rectangle's stream, judges the rectangle against that stream alone and
// leaves a word per rectangle behind the single-stream call's scratch:
//
//   [jpegr_crop_scratch_bytes or jpegr_crop_resize_scratch_bytes, as it is]
//   [u64 x nrects: stream << 32 | the image's index in that stream]
//
// jprs_dataset_crop_decode (jpegr_stream.hip) reads the word of every good
// rectangle and takes the stream, its length, its tile grid and its offsets
// from the descriptor.  Everything behind the decode sees rectangle-local tile
// grids only and is launched as the single-stream calls launch it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_pack_common.h"
#include "jpegr_resize.h"

static_assert(sizeof(jpegr_stream_desc) == 48, "the header states 48 B");

namespace jpegr_dataset {

constexpr size_t kMaxStreams = (size_t)1 << 31;    // a stream's number fits the word's upper half

// the scratch of a call whose single-stream scratch is `base` bytes (a multiple
// of 16, not 0): the words' offset is base; 0 when the size passes SIZE_MAX
inline size_t scratch_with_words(size_t base, size_t nrects) {
  size_t a;
  if (base == 0 || __builtin_mul_overflow(nrects, sizeof(uint64_t), &a) ||
      __builtin_add_overflow(a, (size_t)15, &a) || __builtin_add_overflow(base, a & ~(size_t)15, &a))
    return 0;
  return a;
}

__device__ __forceinline__ uint64_t word_of(uint32_t s, uint32_t image) { return (uint64_t)s << 32 | image; }
__device__ __forceinline__ uint32_t tiles_across(uint32_t n) { return (uint32_t)(((uint64_t)n + 7u) >> 3); }

// The stream of dataset-wide image g: the last descriptor whose image0 is <= g
// in an ascending table, by bisection over [0, nstreams) -- every index read
// lies inside the table whatever it holds -- and then the test that the
// descriptor does contain g, so a table that is not ascending yields a stream
// that holds g or none.  Then the descriptor's own rules: dimensions and count
// not 0, at most 2^32 tiles, a header's worth of bytes, pointers present and
// the offsets 8-B aligned, and a JPR1 or JPT1 header for its w, h, nimg.  d: the
// descriptor, s: its number, image: g's index in it, all left as they are on a
// false.
__device__ __forceinline__ bool stream_of_image(const jpegr_stream_desc *__restrict__ ds, uint64_t nstreams,
                                                uint64_t g, jpegr_stream_desc &d, uint32_t &s,
                                                uint32_t &image) {
  uint64_t lo = 0, hi = nstreams;                    // nstreams >= 1
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (ds[mid].image0 <= g) lo = mid;
    else hi = mid;
  }
  const jpegr_stream_desc c = ds[lo];
  if (c.image0 > g || g - c.image0 >= (uint64_t)c.nimg) return false;    // also nimg == 0
  if (c.w == 0 || c.h == 0 || c.d_in == nullptr || c.d_tile_offsets == nullptr ||
      (reinterpret_cast<uintptr_t>(c.d_tile_offsets) & 7u) != 0 || c.in_len < (uint64_t)kHdr)
    return false;
  const uint64_t per = (uint64_t)tiles_across(c.w) * tiles_across(c.h);    // < 2^58
  if (per > (1ull << 32) || per * (uint64_t)c.nimg > (1ull << 32)) return false;
  if (!header_ok(static_cast<const uint8_t *>(c.d_in), c.in_len, (size_t)(per * c.nimg), c.w, c.h, c.nimg,
                 true))
    return false;
  d = c;
  s = (uint32_t)lo;
  image = (uint32_t)(g - c.image0);
  return true;
}

}  // namespace jpegr_dataset

// The resize call's first launch over a dataset (jprs_dataset_crop_resize_init,
// jpegr_resize.hip): the result words, every rectangle's status, shadow and
// word.  Not part of the C ABI.
__attribute__((visibility("hidden"))) void jpegr_dataset_resize_init_launch(
    const jpegr_stream_desc *d_streams, size_t nstreams, const jpegr_rect *d_rects, size_t nrects,
    int max_w, int max_h, int out_w, int out_h, size_t out_cap, const jpegr_resize::Layout &L,
    void *d_scratch, uint64_t *d_result, hipStream_t st);
