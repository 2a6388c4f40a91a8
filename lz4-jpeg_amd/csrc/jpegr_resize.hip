// jpegr_resize.hip -- jpegr_crop_resize_device's own kernels (include/jpegr.h;
// the scratch and the split with jpegr_stream.hip: jpegr_resize.h):
//
//   jprs_crop_resize_init   the call's first launch: the result words, every
//                 rectangle's status by jprs_crop_tensor_init's rules with the
//                 capacity 3 out_w out_h and a zero-sized rectangle bad, and its
//                 shadow jpegr_rect, whose dst is its slot of RGBA8 pixels in
//                 the scratch.  jprs_crop_decode and jpeg_crop_recon_kernel then
//                 run on the shadows as they are.
//   jprs_dataset_crop_resize_init   the same for
//                 jpegr_dataset_crop_resize_device: the rectangle's stream found
//                 in the table of descriptors first (jpegr_dataset.h)
//   jpeg_resize_weights     a thread per (rectangle, axis, output index): the
//                 window and its weights in fp64 by the header's text, each
//                 weight rounded once to fp32.  Once per tap, not per pixel.
//   jpeg_resize_tensor_kernel<dtype, layout>
//                 a workgroup = one rectangle, kBand output rows, 256 output
//                 columns; a thread = one output column, all three channels of
//                 its kBand rows in registers.  Source rows in ascending order:
//                 the thread sums its column's taps of the row (`mid`, fp32,
//                 ascending x), then adds wty * mid into those of its rows whose
//                 window holds the source row -- the header's summation order
//                 with no LDS and no barrier.  Neighbouring threads' windows
//                 overlap, so the pixel loads are served from the cache; the
//                 weights of one tap are consecutive floats across a wave; the y
//                 windows and weights are the same for the whole workgroup.
//
// fp32 throughout the pixels, every product and sum rounded on its own (no
// contraction: the flag and the pragma), fp32 subnormals kept (the default mode).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/jpegr.h"
#include "jpegr_crop.h"
#include "jpegr_dataset.h"
#include "jpegr_pack_common.h"
#include "jpegr_resize.h"
#include "jpegr_tensor_elem.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBand = 8;         // output rows a workgroup owns: 24 accumulators a thread
constexpr int kCols = 256;       // output columns a workgroup owns, one a thread

__global__ __launch_bounds__(256) void jprs_crop_resize_init(
    const uint8_t *__restrict__ in, uint64_t in_len, size_t ntiles, uint32_t w, uint32_t h,
    uint32_t nimg, const jpegr_rect *__restrict__ rects, size_t nrects, size_t r_base,
    uint32_t max_w, uint32_t max_h, uint64_t elems, uint64_t out_cap, uint64_t pix_slot,
    jpegr_rect *__restrict__ shadow, uint32_t *__restrict__ status, uint64_t *__restrict__ result) {
  const size_t r = r_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r == 0) {
    result[0] = 0ull;
    result[1] = ~0ull;
    result[2] = 0ull;
  }
  if (r >= nrects) return;
  const jpegr_rect rc = rects[r];
  uint32_t st = jpegr_crop::kGood;
  if (!header_ok(in, in_len, ntiles, w, h, nimg, true) || rc.w == 0 || rc.h == 0 || rc.image >= nimg ||
      rc.w > max_w || rc.h > max_h || rc.x > w || rc.w > w - rc.x || rc.y > h || rc.h > h - rc.y ||
      rc.dst > out_cap || elems > out_cap - rc.dst)
    st = jpegr_crop::kBad;
  // a bad rectangle's shadow is never read past its status; it holds zeros
  jpegr_rect sh = {0, 0, 0, 0, 0, 0};
  if (st == jpegr_crop::kGood) {
    sh = rc;
    sh.dst = (uint64_t)r * pix_slot;
  }
  shadow[r] = sh;
  status[r] = st;
}

// jprs_crop_resize_init over a dataset (jpegr_dataset.h): the rectangle's
// stream by bisection, the same rules against that stream's own w, h and nimg,
// the shadow, and the word jprs_dataset_crop_decode finds the stream by.  (Its
// own text: jprs_crop_resize_init stays the code it was.)
__global__ __launch_bounds__(256) void jprs_dataset_crop_resize_init(
    const jpegr_stream_desc *__restrict__ ds, uint64_t nstreams, const jpegr_rect *__restrict__ rects,
    size_t nrects, size_t r_base, uint32_t max_w, uint32_t max_h, uint64_t elems, uint64_t out_cap,
    uint64_t pix_slot, jpegr_rect *__restrict__ shadow, uint32_t *__restrict__ status,
    uint64_t *__restrict__ where, uint64_t *__restrict__ result) {
  const size_t r = r_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r == 0) {
    result[0] = 0ull;
    result[1] = ~0ull;
    result[2] = 0ull;
  }
  if (r >= nrects) return;
  const jpegr_rect rc = rects[r];
  jpegr_stream_desc d;
  uint32_t s = 0, image = 0;
  uint32_t st = jpegr_crop::kGood;
  if (!jpegr_dataset::stream_of_image(ds, nstreams, rc.image, d, s, image) || rc.w == 0 || rc.h == 0 ||
      rc.w > max_w || rc.h > max_h || rc.x > d.w || rc.w > d.w - rc.x || rc.y > d.h || rc.h > d.h - rc.y ||
      rc.dst > out_cap || elems > out_cap - rc.dst)
    st = jpegr_crop::kBad;
  // a bad rectangle's shadow and word are never read past its status; they hold zeros
  jpegr_rect sh = {0, 0, 0, 0, 0, 0};
  uint64_t wh = 0;
  if (st == jpegr_crop::kGood) {
    sh = rc;
    sh.dst = (uint64_t)r * pix_slot;
    wh = jpegr_dataset::word_of(s, image);
  }
  shadow[r] = sh;
  status[r] = st;
  where[r] = wh;
}

// Entry e of the call: output index k of rectangle e / (out_w + out_h), the x
// axis for k < out_w.  The header's text, operation for operation.
__global__ __launch_bounds__(256) void jpeg_resize_weights(
    const jpegr_rect *__restrict__ shadow, const uint32_t *__restrict__ status, size_t nrects,
    size_t e_base, uint32_t out_w, uint32_t out_h, uint32_t capx, uint32_t capy, size_t wper, int filter,
    uint2 *__restrict__ taps, float *__restrict__ wts) {
  const size_t e = e_base + (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t per = out_w + out_h;
  const size_t ri = e / per;
  if (ri >= nrects || status[ri] != jpegr_crop::kGood) return;
  const uint32_t k = (uint32_t)(e - ri * per);
  const bool xaxis = k < out_w;
  const uint32_t j = xaxis ? k : k - out_w;
  const jpegr_rect rc = shadow[ri];
  const int64_t n = (int64_t)(xaxis ? rc.w : rc.h);
  const uint32_t m = xaxis ? out_w : out_h, cap = xaxis ? capx : capy;
  const double r = (double)n / (double)m;
  const double s = (filter == JPEGR_FILTER_TRIANGLE && r > 1.0) ? r : 1.0;
  const double c = ((double)j + 0.5) * r;
  const int64_t lo = max((int64_t)0, (int64_t)floor((c - s) + 0.5));
  const int64_t hi = min(n, (int64_t)floor((c + s) + 0.5));
  double tot = 0.0;
  for (int64_t x = lo; x < hi; ++x) tot = tot + fmax(0.0, 1.0 - fabs(((double)x + 0.5) - c) / s);
  float *const wr = wts + ri * wper + (xaxis ? (size_t)0 : (size_t)out_w * capx);
  // every tap of the window; `cap` is jpegr_resize.h's bound on their number,
  // so the test below is the table's edge and not a limit on the filter
  uint32_t cnt = 0;
  for (int64_t x = lo; x < hi && cnt < cap; ++x, ++cnt) {
    const double u = fmax(0.0, 1.0 - fabs(((double)x + 0.5) - c) / s);
    const float wt = (float)(u / tot);
    if (xaxis) wr[(size_t)cnt * out_w + j] = wt;
    else wr[(size_t)j * capy + cnt] = wt;
  }
  taps[ri * per + k] = make_uint2((uint32_t)lo, cnt);
}

template <int DT, int LAY>
__global__ __launch_bounds__(kCols) void jpeg_resize_tensor_kernel(
    const jpegr_rect *__restrict__ shadow, const jpegr_rect *__restrict__ rects,
    const uint32_t *__restrict__ status, size_t nrects, size_t wg_base, uint32_t out_w, uint32_t out_h,
    uint32_t bands, uint32_t chunks, uint32_t capx, uint32_t capy, size_t wper,
    const uint8_t *__restrict__ pix, const uint2 *__restrict__ taps, const float *__restrict__ wts,
    const uint8_t *__restrict__ flip, TensorNorm nm, void *__restrict__ out) {
  using E = typename TensorElem<DT>::type;
  const size_t wg = wg_base + blockIdx.x;
  const size_t per = (size_t)bands * chunks;
  const size_t ri = wg / per;
  if (ri >= nrects || status[ri] != jpegr_crop::kGood) return;
  const uint32_t rem = (uint32_t)(wg - ri * per);
  const uint32_t band = rem / chunks;
  const uint32_t j = (rem - band * chunks) * kCols + threadIdx.x;   // the resampled column
  if (j >= out_w) return;
  const jpegr_rect sh = shadow[ri];
  const size_t sw = (size_t)sh.w;                                    // the crop's pitch in pixels
  const uint32_t *const src = reinterpret_cast<const uint32_t *>(pix + sh.dst);
  const uint2 *const tp = taps + ri * ((size_t)out_w + out_h);
  const float *const wx = wts + ri * wper + j;
  const float *const wy = wts + ri * wper + (size_t)out_w * capx;
  const uint2 tx = tp[j];
  const uint32_t i0 = band * kBand;

  // the band's y windows: the same for every thread of the workgroup
  uint32_t ylo[kBand], yhi[kBand];
#pragma unroll
  for (int b = 0; b < kBand; ++b) {
    ylo[b] = yhi[b] = 0;
    if (i0 + b < out_h) {
      const uint2 t = tp[out_w + i0 + b];
      ylo[b] = t.x;
      yhi[b] = t.x + t.y;
    }
  }
  uint32_t y1 = 0;                                 // lo rises with the output index: ylo[0] is the first row
#pragma unroll
  for (int b = 0; b < kBand; ++b) y1 = max(y1, yhi[b]);

  float acc[kBand][3];
#pragma unroll
  for (int b = 0; b < kBand; ++b) acc[b][0] = acc[b][1] = acc[b][2] = 0.0f;

  for (uint32_t y = ylo[0]; y < y1; ++y) {
    bool used = false;                             // between two windows of a downscale by BILINEAR: no
#pragma unroll
    for (int b = 0; b < kBand; ++b) used |= y >= ylo[b] && y < yhi[b];
    if (!used) continue;
    const uint32_t *const row = src + (size_t)y * sw + tx.x;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    for (uint32_t t = 0; t < tx.y; ++t) {
      const uint32_t p = row[t];
      const float wt = wx[(size_t)t * out_w];
      m0 = m0 + wt * (float)(p & 255u);
      m1 = m1 + wt * (float)((p >> 8) & 255u);
      m2 = m2 + wt * (float)((p >> 16) & 255u);
    }
#pragma unroll
    for (int b = 0; b < kBand; ++b)
      if (y >= ylo[b] && y < yhi[b]) {
        const float wt = wy[(size_t)(i0 + b) * capy + (y - ylo[b])];
        acc[b][0] = acc[b][0] + wt * m0;
        acc[b][1] = acc[b][1] + wt * m1;
        acc[b][2] = acc[b][2] + wt * m2;
      }
  }

  // a row's out_w elements (3 out_w interleaved) come from consecutive threads
  const bool mirror = flip != nullptr && flip[ri] != 0;              // inside [0, nrects)
  const uint64_t jo = mirror ? (uint64_t)(out_w - 1u - j) : (uint64_t)j;
  const uint64_t plane = (uint64_t)out_w * out_h;
  E *const q = static_cast<E *>(out) + rects[ri].dst;
#pragma unroll
  for (int b = 0; b < kBand; ++b) {
    const uint64_t i = (uint64_t)i0 + b;
    if (i >= out_h) break;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const E e = tensor_elem_of<DT>(acc[b][ch], nm.s[ch], nm.b[ch]);
      if constexpr (LAY == JPEGR_LAYOUT_CHW) q[ch * plane + i * out_w + jo] = e;
      else q[3u * (i * out_w + jo) + ch] = e;
    }
  }
}

using ResizeKernel = void (*)(const jpegr_rect *, const jpegr_rect *, const uint32_t *, size_t, size_t,
                              uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, size_t,
                              const uint8_t *, const uint2 *, const float *, const uint8_t *, TensorNorm,
                              void *);

// jpeg_resize_tensor_kernel<dtype, layout>, one instance per pair
ResizeKernel resize_kernel_of(int dtype, int layout) {
  static const ResizeKernel k[4][2] = {
      {jpeg_resize_tensor_kernel<JPEGR_DTYPE_U8, JPEGR_LAYOUT_CHW>,
       jpeg_resize_tensor_kernel<JPEGR_DTYPE_U8, JPEGR_LAYOUT_HWC>},
      {jpeg_resize_tensor_kernel<JPEGR_DTYPE_F32, JPEGR_LAYOUT_CHW>,
       jpeg_resize_tensor_kernel<JPEGR_DTYPE_F32, JPEGR_LAYOUT_HWC>},
      {jpeg_resize_tensor_kernel<JPEGR_DTYPE_F16, JPEGR_LAYOUT_CHW>,
       jpeg_resize_tensor_kernel<JPEGR_DTYPE_F16, JPEGR_LAYOUT_HWC>},
      {jpeg_resize_tensor_kernel<JPEGR_DTYPE_BF16, JPEGR_LAYOUT_CHW>,
       jpeg_resize_tensor_kernel<JPEGR_DTYPE_BF16, JPEGR_LAYOUT_HWC>}};
  return k[dtype][layout];
}

}  // namespace

void jpegr_resize_init_launch(const uint8_t *d_in, size_t in_len, size_t ntiles, int w, int h, int nimg,
                              const jpegr_rect *d_rects, size_t nrects, int max_w, int max_h, int out_w,
                              int out_h, size_t out_cap, const jpegr_resize::Layout &L, void *d_scratch,
                              uint64_t *d_result, hipStream_t st) {
  auto *base = static_cast<uint8_t *>(d_scratch);
  auto *shadow = reinterpret_cast<jpegr_rect *>(base + L.shadow);
  auto *status = reinterpret_cast<uint32_t *>(base + L.status);
  const uint64_t elems = 3ull * (uint64_t)out_w * (uint64_t)out_h;
  launch_chunks(nrects, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_crop_resize_init, dim3(n), dim3(256), 0, st, d_in, (uint64_t)in_len, ntiles,
                       (uint32_t)w, (uint32_t)h, (uint32_t)nimg, d_rects, nrects, b * 256, (uint32_t)max_w,
                       (uint32_t)max_h, elems, (uint64_t)out_cap, (uint64_t)L.pix_slot, shadow, status,
                       d_result);
  });
}

void jpegr_dataset_resize_init_launch(const jpegr_stream_desc *d_streams, size_t nstreams,
                                      const jpegr_rect *d_rects, size_t nrects, int max_w, int max_h,
                                      int out_w, int out_h, size_t out_cap, const jpegr_resize::Layout &L,
                                      void *d_scratch, uint64_t *d_result, hipStream_t st) {
  auto *base = static_cast<uint8_t *>(d_scratch);
  auto *shadow = reinterpret_cast<jpegr_rect *>(base + L.shadow);
  auto *status = reinterpret_cast<uint32_t *>(base + L.status);
  auto *where = reinterpret_cast<uint64_t *>(base + L.bytes);     // behind the single-stream call's scratch
  const uint64_t elems = 3ull * (uint64_t)out_w * (uint64_t)out_h;
  launch_chunks(nrects, 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jprs_dataset_crop_resize_init, dim3(n), dim3(256), 0, st, d_streams,
                       (uint64_t)nstreams, d_rects, nrects, b * 256, (uint32_t)max_w, (uint32_t)max_h, elems,
                       (uint64_t)out_cap, (uint64_t)L.pix_slot, shadow, status, where, d_result);
  });
}

int jpegr_resize_launch(const jpegr_resize::Layout &L, void *d_scratch, const jpegr_rect *d_rects,
                        size_t nrects, int out_w, int out_h, int filter, const uint8_t *d_flip, int dtype,
                        int layout, const float *scale3, const float *bias3, void *d_out, hipStream_t st) {
  auto *base = static_cast<uint8_t *>(d_scratch);
  auto *shadow = reinterpret_cast<const jpegr_rect *>(base + L.shadow);
  auto *status = reinterpret_cast<const uint32_t *>(base + L.status);
  auto *taps = reinterpret_cast<uint2 *>(base + L.taps);
  auto *wts = reinterpret_cast<float *>(base + L.wts);
  const uint32_t ow = (uint32_t)out_w, oh = (uint32_t)out_h;
  TensorNorm nm;
  for (int c = 0; c < 3; ++c) {
    nm.s[c] = scale3 ? scale3[c] : 1.0f;
    nm.b[c] = bias3 ? bias3[c] : 0.0f;
  }
  launch_chunks(nrects * ((size_t)ow + oh), 256, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(jpeg_resize_weights, dim3(n), dim3(256), 0, st, shadow, status, nrects, b * 256, ow,
                       oh, L.capx, L.capy, L.wper, filter, taps, wts);
  });
  const uint32_t bands = (oh + kBand - 1) / kBand, chunks = (ow + kCols - 1) / kCols;
  const ResizeKernel kernel = resize_kernel_of(dtype, layout);
  launch_chunks(nrects * bands * chunks, 1, [&](size_t b, unsigned n) {
    hipLaunchKernelGGL(kernel, dim3(n), dim3(kCols), 0, st, shadow, d_rects, status, nrects, b, ow, oh,
                       bands, chunks, L.capx, L.capy, L.wper, base + L.pix, taps, wts, d_flip, nm, d_out);
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

extern "C" size_t jpegr_crop_resize_scratch_bytes(size_t nrects, int max_w, int max_h, int out_w,
                                                  int out_h) {
  jpegr_resize::Layout L;
  return jpegr_resize::layout_of(nrects, max_w, max_h, out_w, out_h, L) ? L.bytes : 0;
}

extern "C" size_t jpegr_dataset_crop_resize_scratch_bytes(size_t nrects, int max_w, int max_h, int out_w,
                                                          int out_h) {
  jpegr_resize::Layout L;
  if (!jpegr_resize::layout_of(nrects, max_w, max_h, out_w, out_h, L)) return 0;
  return jpegr_dataset::scratch_with_words(L.bytes, nrects);
}
