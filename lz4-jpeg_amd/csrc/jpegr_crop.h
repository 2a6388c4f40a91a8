// jpegr_crop.h -- what the two halves of jpegr_crop_device (include/jpegr.h)
// agree on: jprs_crop_init / jprs_crop_decode (jpegr_stream.hip) check the
// rectangles and decode the tiles they touch into the scratch;
// jpeg_crop_recon_kernel (jpegr_recon.h, compiled in jpegr.hip) turns the
// scratch into each rectangle's pixels, by the whole-image reconstruction's own
// dequantisation, IDCT and pixel, and counts the verdicts.
//
// A rectangle occupies K = crop_span(max_w) * crop_span(max_h) items.  Item
// r K + c is cell c of rectangle r's own gw x gh grid of tiles, row-major with
// pitch gw (tile column c % gw, tile row c / gw, counted from the rectangle's
// first tile); cells at or past gw gh are idle.  The scratch holds the items'
// 128 int16 each (jpegr_encode_device's tile layout), then one u32 status word
// per rectangle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegr.h"

namespace jpegr_crop {

// a rectangle's status word: written by jprs_crop_init from the rectangle's own
// fields and the header, turned bad by jprs_crop_decode, read by the
// reconstruction
constexpr uint32_t kGood = 0u, kBad = 1u, kEmpty = 2u;

// tile columns (rows) a crop of n pixels can touch: ceil(n / 8) + 1
__host__ __device__ inline uint32_t crop_span(uint32_t n) { return (n + 7u) / 8u + 1u; }

// a good rectangle's grid: its first tile and its span, in tiles
struct Grid {
  uint32_t tx0, ty0, gw, gh;
};
__device__ __forceinline__ Grid grid_of(const jpegr_rect &rc) {
  Grid g;
  g.tx0 = (uint32_t)(rc.x >> 3);
  g.ty0 = (uint32_t)(rc.y >> 3);
  g.gw = (uint32_t)((rc.x + rc.w - 1) >> 3) - g.tx0 + 1u;
  g.gh = (uint32_t)((rc.y + rc.h - 1) >> 3) - g.ty0 + 1u;
  return g;
}

}  // namespace jpegr_crop

// The reconstruction half (the launch: jpegr.hip): d_coef the scratch's items, d_status its
// status words; counts into result[0], atomicMin into result[1].  Not part of
// the C ABI.
__attribute__((visibility("hidden"))) int jpegr_crop_recon_launch(
    const int16_t *d_coef, const uint32_t *d_status, const jpegr_rect *d_rects, size_t nrects,
    int max_w, int max_h, uint8_t *d_out, uint64_t *d_result, hipStream_t st);

// The same for jpegr_crop_tensor_device (jpeg_crop_tensor_kernel): d_flip NULL
// or a byte per rectangle, scale3 and bias3 three floats each on the host, read
// here and passed by value; dtype and layout are the header's, already checked.
__attribute__((visibility("hidden"))) int jpegr_crop_tensor_launch(
    const int16_t *d_coef, const uint32_t *d_status, const jpegr_rect *d_rects, size_t nrects,
    int max_w, int max_h, const uint8_t *d_flip, int dtype, int layout, const float *scale3,
    const float *bias3, void *d_out, uint64_t *d_result, hipStream_t st);
