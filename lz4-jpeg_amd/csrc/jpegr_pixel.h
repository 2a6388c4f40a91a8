// jpegr_pixel.h -- the pixel arithmetic the JPEG kernels share, each piece once:
// from a plane's fp64 sample to an RGBA8 pixel (round_clamp_u8, colour_term,
// rgba_of) for every kernel that reconstructs -- jpeg_recon_kernel and
// jpeg_crop_recon_kernel (jpegr_recon.h), the thumbnail kernel
// (jpegr_thumb.hip) -- and the reference's forward colour expressions in fp64
// (ref_y, ref_cr, ref_cb) for the encoder's slow path (jpegr_dct.h) and the
// reconstruction's untransformed tiles.  All of it is inlined into its callers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ int clamp_u8(int v) {       // JPEG.c:132-139
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The reference's forward colour expressions in fp64, in its order of
// operations: Y = (uint8_t)((0.299 R + 0.587 G) + 0.114 B) (JPEG.c:127; the
// value lies in [0, 256)), Cr and Cb = clamp((int)(... + 128.0)) (JPEG.c:157,
// 180).  The encoder evaluates them on the triples its integer path cannot
// decide, the reconstruction on the tiles the reference never transforms.
__device__ __forceinline__ int ref_y(unsigned R, unsigned G, unsigned B) {
  return (int)(uint8_t)(unsigned)(0.299 * (double)R + 0.587 * (double)G + 0.114 * (double)B);
}
__device__ __forceinline__ int ref_cr(unsigned R, unsigned G, unsigned B) {
  return clamp_u8((int)(0.439 * (double)R - 0.368 * (double)G - 0.071 * (double)B + 128.0));
}
__device__ __forceinline__ int ref_cb(unsigned R, unsigned G, unsigned B) {
  return clamp_u8((int)(-0.148 * (double)R - 0.291 * (double)G + 0.439 * (double)B + 128.0));
}

// (int)round(x) clamped to 0..255 (JPEG.c:440-446).  round() is half away
// from zero; for x >= 0 that is trunc(x) + (x - trunc(x) >= 0.5), the
// fraction exact in fp64.  A negative x clamps to 0 either way (trunc
// toward zero gives <= 0 there), as does anything at or past 255.5.
// Pinned by tests/test_gpu_jpeg_exact.py on samples an ulp either side of
// k + 0.5 and past both clamps.
__device__ __forceinline__ int round_clamp_u8(double x) {
  const int i = (int)x;                          // v_cvt_i32_f64: toward zero, saturating
  const int v = i + ((x - (double)i) >= 0.5 ? 1 : 0);
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The colour terms of assemble_image (JPEG.c:601-603): (int)(k * (double)d)
// for d = Cr - 128 or Cb - 128 in -128..127 and k in {1.402, 0.344136,
// 0.714136, 1.772}.  k d is never within 0.00104 of a nonzero integer on that
// range (k = m / 10^e with d m not a multiple of 10^e unless d = 0), and the
// fp64 product is within 1e-13 of k d, so its truncation is trunc(k d); the
// fp32 product of the rounded k is within 3e-5 of k d, so it truncates the
// same way.  Checked for all 4 x 256 cases by tests/test_tables.py.
__device__ __forceinline__ int colour_term(float k, int d) {
  return (int)(k * (float)d);
}

// assemble_image's pixel (JPEG.c:601-603) of one Y, Cr, Cb sample: R | G << 8 |
// B << 16 | 255 << 24
__device__ __forceinline__ uint32_t rgba_of(int Y, int Cr, int Cb) {
  const int R = Y + colour_term(1.402f, Cr - 128);
  const int G = Y - colour_term(0.344136f, Cb - 128) - colour_term(0.714136f, Cr - 128);
  const int B = Y + colour_term(1.772f, Cb - 128);
  return (uint32_t)clamp_u8(R) | ((uint32_t)clamp_u8(G) << 8) | ((uint32_t)clamp_u8(B) << 16) |
         (255u << 24);
}

}  // namespace
