// jpegr.hip -- MI355X (gfx950) JPEG pixel stage, one translation unit of
// per-kernel headers:
//   jpegr_dct.h    the encoder: RGBA -> Y/Cr/Cb -> 4:2:2 -> fp64 DCT-II ->
//                  quantisation -> zigzag -> int16 (jpeg_strip_kernel)
//   jpegr_recon.h  the reconstruction: dequantisation, IDCT, YCbCr -> RGBA, of
//                  whole images (jpeg_recon_kernel) and of rectangles
//                  (jpeg_crop_recon_kernel: RGBA8 rows; jpeg_crop_tensor_kernel:
//                  three channels as a tensor's elements)
// This file holds what they share -- the strip sizes, the LDS strides, the
// tables -- and the host side: the launches and the C ABI.
//
// Bit-exactness to Algorithms/sequential/JPEG/JPEG.c (x86-64, strict IEEE
// double) rests on: fp64 throughout, no contraction (built with
// -ffp-contract=off and the pragma below), the reference's summation order
// (x outer, y inner, JPEG.c:477-485), the reference's product association
// ((cv*cos_x)*cos_y, JPEG.c:483; (alpha_u*alpha_v)*sum, JPEG.c:489),
// correctly-rounded fp64 division (JPEG.c:626) and the exact cos/alpha
// values baked by gen_jpeg_tables.py.  No MFMA (fused multiply-add would
// change the rounding) and no butterfly factorisation (changes the sum).
//
// The tables are __constant__ arrays initialised at build time
// (jpeg_tables_dev.h, generated): no call uploads anything, so every launch
// here is asynchronous and capturable from the first call on every device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "jpeg_tables.h"
#include "jpeg_tables_dev.h"   // the __constant__ tables (dC8 .. dRZa), initialised
#include "jpegr_crop.h"
#include "jpegr_pixel.h"
#include "../../include/jpegr.h"

#pragma clang fp contract(off)

namespace {

using namespace jpegr_dev;

constexpr int kTiles = 32;      // tiles per workgroup strip
constexpr int kThreads = 256;    // 4 waves
// the encoder's strip (JPEGR_STRIP_TILES: tools A/B of a narrower strip)
#ifndef JPEGR_STRIP_TILES
#define JPEGR_STRIP_TILES 32
#endif
constexpr int kETiles = JPEGR_STRIP_TILES;
constexpr int kEThreads = 8 * kETiles;   // thread = (tile, row u)
static_assert(kETiles == 16 || kETiles == 32, "strip of 16 or 32 tiles");
constexpr int kYStride = 66;     // doubles per Y tile in LDS (528 B: bank skew 4)
constexpr int kCStride = 34;     // doubles per chroma tile (272 B: bank skew 4)

}  // namespace

// in definition order: both use the constants above, jpegr_pixel.h and the tables
#include "jpegr_dct.h"
#include "jpegr_recon.h"

namespace {

// nimg images of w x h pixels cut into strips of `per` tiles: a workgroup per
// strip (grid x: tile row, then strip) and image (grid y)
struct Geometry {
  int tiles_x, tiles_y, strips;
  dim3 grid;
};

bool geometry_of(int w, int h, int nimg, int per, Geometry &g) {
  if (w <= 0 || h <= 0 || nimg <= 0 || nimg > 65535) return false;
  g.tiles_x = (int)(((long long)w + 7) / 8);     // w + 7 may not wrap
  g.tiles_y = (int)(((long long)h + 7) / 8);
  g.strips = (g.tiles_x + per - 1) / per;
  const long long gx = (long long)g.tiles_y * g.strips;
  if (gx > 0x7fffffffLL) return false;
  g.grid = dim3((unsigned)gx, (unsigned)nimg);
  return true;
}

// the pointer rules of include/jpegr.h, checked before any HIP call
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// d_rgba: phase 1's loads are dword-aligned (16 B wide where w % 4 == 0); d_out:
// phase 4's uint4 stores (int16) or the raw DCT's doubles
int launch(bool raw, const void *d_rgba, int w, int h, int nimg, void *d_out,
           void *stream) {
  Geometry g;
  if (!d_rgba || !d_out || !geometry_of(w, h, nimg, kETiles, g)) return JPEGR_ERR_ARG;
  if (misaligned(d_rgba, 3) || misaligned(d_out, raw ? 7 : 15)) return JPEGR_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto kernel = raw ? jpeg_strip_kernel<true> : jpeg_strip_kernel<false>;
  hipLaunchKernelGGL(kernel, g.grid, dim3(kEThreads), 0, s, static_cast<const uint8_t *>(d_rgba),
                     w, h, g.tiles_x, g.tiles_y, g.strips, d_out);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

}  // namespace

int jpegr_crop_recon_launch(const int16_t *d_coef, const uint32_t *d_status,
                            const jpegr_rect *d_rects, size_t nrects, int max_w, int max_h,
                            uint8_t *d_out, uint64_t *d_result, hipStream_t st) {
  const uint32_t gwm = jpegr_crop::crop_span((uint32_t)max_w), ghm = jpegr_crop::crop_span((uint32_t)max_h);
  const uint32_t strips = (gwm + kTiles - 1) / kTiles;
  // at most 2^22 workgroups a launch (HIP's grid limit is 2^32 work-items)
  const size_t nwg = nrects * ghm * strips, step = (size_t)1 << 22;
  for (size_t b = 0; b < nwg; b += step)
    hipLaunchKernelGGL(jpeg_crop_recon_kernel, dim3((unsigned)(nwg - b < step ? nwg - b : step)),
                       dim3(kThreads), 0, st, d_coef, d_status, d_rects, nrects, b, gwm, ghm, strips,
                       d_out, d_result);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

namespace {

using CropTensorKernel = void (*)(const int16_t *, const uint32_t *, const jpegr_rect *, size_t, size_t,
                                  uint32_t, uint32_t, uint32_t, const uint8_t *, TensorNorm, void *,
                                  uint64_t *);

// jpeg_crop_tensor_kernel<dtype, layout>, one instance per pair
CropTensorKernel crop_tensor_kernel_of(int dtype, int layout) {
  static const CropTensorKernel k[4][2] = {
      {jpeg_crop_tensor_kernel<JPEGR_DTYPE_U8, JPEGR_LAYOUT_CHW>,
       jpeg_crop_tensor_kernel<JPEGR_DTYPE_U8, JPEGR_LAYOUT_HWC>},
      {jpeg_crop_tensor_kernel<JPEGR_DTYPE_F32, JPEGR_LAYOUT_CHW>,
       jpeg_crop_tensor_kernel<JPEGR_DTYPE_F32, JPEGR_LAYOUT_HWC>},
      {jpeg_crop_tensor_kernel<JPEGR_DTYPE_F16, JPEGR_LAYOUT_CHW>,
       jpeg_crop_tensor_kernel<JPEGR_DTYPE_F16, JPEGR_LAYOUT_HWC>},
      {jpeg_crop_tensor_kernel<JPEGR_DTYPE_BF16, JPEGR_LAYOUT_CHW>,
       jpeg_crop_tensor_kernel<JPEGR_DTYPE_BF16, JPEGR_LAYOUT_HWC>}};
  return k[dtype][layout];
}

}  // namespace

int jpegr_crop_tensor_launch(const int16_t *d_coef, const uint32_t *d_status,
                             const jpegr_rect *d_rects, size_t nrects, int max_w, int max_h,
                             const uint8_t *d_flip, int dtype, int layout, const float *scale3,
                             const float *bias3, void *d_out, uint64_t *d_result, hipStream_t st) {
  const uint32_t gwm = jpegr_crop::crop_span((uint32_t)max_w), ghm = jpegr_crop::crop_span((uint32_t)max_h);
  const uint32_t strips = (gwm + kTiles - 1) / kTiles;
  TensorNorm nm;
  for (int c = 0; c < 3; ++c) {
    nm.s[c] = scale3 ? scale3[c] : 1.0f;
    nm.b[c] = bias3 ? bias3[c] : 0.0f;
  }
  const CropTensorKernel kernel = crop_tensor_kernel_of(dtype, layout);
  // at most 2^22 workgroups a launch, as jpegr_crop_recon_launch
  const size_t nwg = nrects * ghm * strips, step = (size_t)1 << 22;
  for (size_t b = 0; b < nwg; b += step)
    hipLaunchKernelGGL(kernel, dim3((unsigned)(nwg - b < step ? nwg - b : step)), dim3(kThreads), 0, st,
                       d_coef, d_status, d_rects, nrects, b, gwm, ghm, strips, d_flip, nm, d_out,
                       d_result);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

extern "C" {

size_t jpegr_coef_count(int w, int h) {
  if (w <= 0 || h <= 0) return 0;
  return (((size_t)w + 7) / 8) * (((size_t)h + 7) / 8) * 128;
}

int jpegr_encode_device(const void *d_rgba, int w, int h, int nimg, void *d_out,
                        void *stream) {
  return launch(false, d_rgba, w, h, nimg, d_out, stream);
}

int jpegr_dct_raw_device(const void *d_rgba, int w, int h, int nimg,
                         void *d_out, void *stream) {
  return launch(true, d_rgba, w, h, nimg, d_out, stream);
}

int jpegr_encode(const uint8_t *rgba, int w, int h, int16_t *out) {
  if (!rgba || !out || w <= 0 || h <= 0) return JPEGR_ERR_ARG;
  const size_t in_b = (size_t)w * h * 4, out_b = jpegr_coef_count(w, h) * 2;
  void *din = nullptr, *dout = nullptr;
  if (hipMalloc(&din, in_b) != hipSuccess) return JPEGR_ERR_NOMEM;
  if (hipMalloc(&dout, out_b) != hipSuccess) { (void)hipFree(din); return JPEGR_ERR_NOMEM; }
  int rc = JPEGR_OK;
  if (hipMemcpy(din, rgba, in_b, hipMemcpyHostToDevice) != hipSuccess) rc = JPEGR_ERR_HIP;
  if (rc == JPEGR_OK) rc = jpegr_encode_device(din, w, h, 1, dout, nullptr);
  if (rc == JPEGR_OK && hipMemcpy(out, dout, out_b, hipMemcpyDeviceToHost) != hipSuccess)
    rc = JPEGR_ERR_HIP;
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}

int jpegr_time_device(const void *d_rgba, int w, int h, int nimg, void *d_out,
                      int iters, void *stream, float *ms_per_launch) {
  if (iters <= 0 || !ms_per_launch) return JPEGR_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess) return JPEGR_ERR_HIP;
  if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return JPEGR_ERR_HIP; }
  int rc = JPEGR_OK;
  (void)hipEventRecord(a, s);
  for (int i = 0; i < iters && rc == JPEGR_OK; ++i)
    rc = jpegr_encode_device(d_rgba, w, h, nimg, d_out, stream);
  (void)hipEventRecord(b, s);
  if (hipEventSynchronize(b) != hipSuccess) rc = JPEGR_ERR_HIP;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  *ms_per_launch = ms / iters;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return rc;
}

int jpegr_reconstruct_device(const void *d_coef, const void *d_rgba_orig, int w, int h,
                             int nimg, void *d_rgba_out, void *stream) {
  Geometry g;
  if (!d_coef || !d_rgba_out || !geometry_of(w, h, nimg, kTiles, g)) return JPEGR_ERR_ARG;
  // recon_dequant's uint4 loads; store_px4's dword stores (d_rgba_orig may be NULL)
  if (misaligned(d_coef, 15) || misaligned(d_rgba_orig, 3) || misaligned(d_rgba_out, 3))
    return JPEGR_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto kernel = d_rgba_orig ? jpeg_recon_kernel<true> : jpeg_recon_kernel<false>;
  hipLaunchKernelGGL(kernel, g.grid, dim3(kThreads), 0, s, static_cast<const int16_t *>(d_coef),
                     static_cast<const uint8_t *>(d_rgba_orig), w, h, g.tiles_x, g.tiles_y,
                     g.strips, static_cast<uint8_t *>(d_rgba_out));
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

const char *jpegr_strerror(int code) {
  switch (code) {
    case JPEGR_OK: return "ok";
    case JPEGR_ERR_ARG: return "invalid argument";
    case JPEGR_ERR_HIP: return "HIP runtime error";
    case JPEGR_ERR_NOMEM: return "device allocation failed";
    default: return "unknown error";
  }
}

}  // extern "C"
