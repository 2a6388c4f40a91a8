// jpegr_resize.h -- what the two halves of jpegr_crop_resize_device
// (include/jpegr.h) agree on.  jpegr_stream.hip holds the entry point and the
// decode of the tiles; jpegr_resize.hip holds the rectangle check
// (jprs_crop_resize_init), the tap tables (jpeg_resize_weights) and the
// resampling itself (jpeg_resize_tensor_kernel).  In between,
// jpeg_crop_recon_kernel (jpegr.hip) writes every good rectangle's RGBA8 pixels
// into the scratch, through a shadow jpegr_rect whose dst is the rectangle's
// slot there.
//
// The scratch, every part at a multiple of 16 B:
//   [jpegr_crop_device's scratch: K items of 256 B and a status word a rectangle]
//   [shadow jpegr_rect x nrects]
//   [pixels: 4 max_w max_h bytes x nrects; a crop's rows are w pixels apart]
//   [taps: (lo, count) u32 pairs, out_w then out_h of them, x nrects]
//   [weights fp32 x nrects: x axis [capx][out_w] (tap-major: a wave's loads of
//    one tap are consecutive), then y axis [out_h][capy]]
// capx = 2 ceil(max_w / out_w) + 2 bounds an x window's taps: before clipping
// hi - lo < (c + s + 0.5) - (c - s + 0.5 - 1) = 2 s + 1 with s <= max(1, n / m)
// <= ceil(max_w / out_w), so hi - lo <= 2 ceil(max_w / out_w), and two more for
// the roundings of c - s and c + s.  capy likewise.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/jpegr.h"

namespace jpegr_resize {

struct Layout {
  size_t status, shadow, pix, taps, wts, bytes;   // byte offsets from the scratch, and its size
  size_t pix_slot;                                // bytes of a rectangle's pixels
  size_t wper;                                    // floats of a rectangle's weights
  uint32_t capx, capy;
};

// false: a bad argument, or a size that does not fit a size_t
inline bool layout_of(size_t nrects, int max_w, int max_h, int out_w, int out_h, Layout &L) {
  const size_t crop = jpegr_crop_scratch_bytes(nrects, max_w, max_h);   // 0: nrects, max_w or max_h
  if (crop == 0 || out_w <= 0 || out_h <= 0) return false;
  const size_t mw = (size_t)max_w, mh = (size_t)max_h, ow = (size_t)out_w, oh = (size_t)out_h;
  const size_t cx = 2 * ((mw + ow - 1) / ow) + 2, cy = 2 * ((mh + oh - 1) / oh) + 2;
  size_t per_taps, a, b;
  if (cx > 0x7fffffffu || cy > 0x7fffffffu) return false;               // the kernels count taps in u32
  L.capx = (uint32_t)cx;
  L.capy = (uint32_t)cy;
  L.status = jpegr_crop_items(max_w, max_h) * 256 * nrects;             // inside crop: no wrap
  L.shadow = crop;
  if (__builtin_mul_overflow(nrects, sizeof(jpegr_rect), &a) || __builtin_add_overflow(L.shadow, a, &L.pix))
    return false;
  if (__builtin_mul_overflow(mw * 4, mh, &L.pix_slot) || __builtin_mul_overflow(L.pix_slot, nrects, &a) ||
      __builtin_add_overflow(a, (size_t)15, &a) || __builtin_add_overflow(L.pix, a & ~(size_t)15, &L.taps))
    return false;
  per_taps = (ow + oh) * 8;
  if (__builtin_mul_overflow(per_taps, nrects, &a) || __builtin_add_overflow(a, (size_t)15, &a) ||
      __builtin_add_overflow(L.taps, a & ~(size_t)15, &L.wts))
    return false;
  if (__builtin_mul_overflow(ow, cx, &a) || __builtin_mul_overflow(oh, cy, &b) ||
      __builtin_add_overflow(a, b, &L.wper) || __builtin_mul_overflow(L.wper, (size_t)4, &a) ||
      __builtin_mul_overflow(a, nrects, &a) || __builtin_add_overflow(a, (size_t)15, &a) ||
      __builtin_add_overflow(L.wts, a & ~(size_t)15, &L.bytes))
    return false;
  return true;
}

}  // namespace jpegr_resize

// The call's first launch (jprs_crop_resize_init): the result words, every
// rectangle's status and shadow.  Not part of the C ABI.
__attribute__((visibility("hidden"))) void jpegr_resize_init_launch(
    const uint8_t *d_in, size_t in_len, size_t ntiles, int w, int h, int nimg, const jpegr_rect *d_rects,
    size_t nrects, int max_w, int max_h, int out_w, int out_h, size_t out_cap,
    const jpegr_resize::Layout &L, void *d_scratch, uint64_t *d_result, hipStream_t st);

// The call's last two launches (jpeg_resize_weights, jpeg_resize_tensor_kernel)
// over the pixels that jpeg_crop_recon_kernel left in the scratch.  d_rects: the
// caller's, for dst; filter, dtype and layout are the header's, already
// checked; scale3 and bias3 are read here and passed by value.
__attribute__((visibility("hidden"))) int jpegr_resize_launch(
    const jpegr_resize::Layout &L, void *d_scratch, const jpegr_rect *d_rects, size_t nrects, int out_w,
    int out_h, int filter, const uint8_t *d_flip, int dtype, int layout, const float *scale3,
    const float *bias3, void *d_out, hipStream_t st);
