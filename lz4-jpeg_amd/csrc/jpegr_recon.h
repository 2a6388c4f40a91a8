// jpegr_recon.h -- the JPEG reconstruction's kernels (part of jpegr.hip, which
// defines the strip size, the LDS strides and the tables before including
// this): one text of the dequantisation, the IDCT and the pixel for whole
// images (jpeg_recon_kernel) and for rectangles (jpeg_crop_recon_kernel, the
// second half of jpegr_crop_device: jpegr_crop.h; jpeg_crop_tensor_kernel, that
// of jpegr_crop_tensor_device, which delivers elements of a tensor).
#pragma once

#include "jpegr_tensor_elem.h"

#pragma clang fp contract(off)

namespace {

// ---- reconstruction: the decode side of the reference's main --------------
// (JPEG.c:1131-1425 minus the entropy round trip, which is the identity on
// the coefficients): per tile, reverse zigzag + Inverse_quantize (:631-638),
// fp64 IDCT in the reference's order (:399-448: for each (x, y) the sum over
// u outer, v inner of (((au*av)*c)*cos_x)*cos_y, then (int)round(s + 128)
// clamped), and assemble_image's YCbCr 4:2:2 -> RGB (:553-619).  Tiles at
// index >= ceil(W*H/64) are never transformed by the reference (:1131) and
// keep their original samples: taken from `orig` when given.
//
// A workgroup of 256 threads takes a strip of up to kTiles tiles of one tile
// row, `ntiles` of them live.  Phases 1 and 2 and the pixel of phase 3 are the
// functions below, one text for jpeg_recon_kernel and jpeg_crop_recon_kernel
// (the same tables, products, summation order and round_clamp_u8:
// bit-exactness rests on that order); the loop of phase 3 addresses and clips
// per kernel.  t: the thread of 256.

// phase 1: coefficients -> dequantised, alpha-scaled doubles in LDS; tile i's
// 128 int16 at src + 128 i.
__device__ __forceinline__ void recon_dequant(const int16_t *src, int ntiles, int t,
                                              double *yac, double *crac, double *cbac) {
  // Thread t takes the 8 coefficients z0 .. z0 + 7 (z0 = 8 (t mod 16)) of
  // tiles t / 16 and 16 + t / 16, so its natural indices, quantiser steps and
  // alpha products are looked up once for both tiles.
  const int z0 = (t & 15) * 8;
  const bool luma = z0 < 64;
  double *const dst = luma ? yac : (z0 < 96 ? crac : cbac);
  const int stride = luma ? kYStride : kCStride;
  int nat[8];
  double qs[8], aa[8];
  // one load each from z-indexed tables, none depending on another (a
  // zigzag -> natural lookup followed by the step / alpha loads it indexes
  // was two dependent memory round trips at the head of every workgroup:
  // 74.4 -> 64.5 us per 4K image, tools/ab_recon_inproc.py)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    nat[j] = dRZn[z0 + j];
    qs[j] = dRZq[z0 + j];
    aa[j] = dRZa[z0 + j];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int tile = k * 16 + (t >> 4);
    if (tile < ntiles) {
      const uint4 v = *reinterpret_cast<const uint4 *>(src + tile * 128 + z0);
      const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double q = (double)(int16_t)(wv[j >> 1] >> (16 * (j & 1)));
        dst[tile * stride + nat[j]] = aa[j] * (q * qs[j]);   // JPEG.c:631-638
      }
    }
  }
}

// phase 2: IDCT, thread = (tile, x), to the strip's uint8 samples in LDS.
__device__ __forceinline__ void recon_idct(int t, const double *yac, const double *crac,
                                           const double *cbac, uint8_t *ys, uint8_t *crs,
                                           uint8_t *cbs) {
  const int tile = t >> 3, x = t & 7;
  double cx[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) cx[u] = dC8[x][u];
  {
    const double *a = yac + tile * kYStride;
    double s[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) s[y] = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const double tv = a[u * 8 + v] * cx[u];                         // (..*c)*cos_x
#pragma unroll
        for (int y = 0; y < 8; ++y) s[y] = s[y] + tv * jpegr_tables::C8[y][v];
      }
    }
#pragma unroll
    for (int y = 0; y < 8; ++y)
      ys[tile * 64 + x * 8 + y] = (uint8_t)round_clamp_u8(s[y] + 128.0);   // JPEG.c:440
  }
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const double *a = (ch == 0 ? crac : cbac) + tile * kCStride;
    double s[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) s[y] = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const double tv = a[u * 4 + v] * cx[u];
#pragma unroll
        for (int y = 0; y < 4; ++y) s[y] = s[y] + tv * jpegr_tables::C4[y][v];
      }
    }
    uint8_t *dst = (ch == 0 ? crs : cbs) + tile * 32 + x * 4;
#pragma unroll
    for (int y = 0; y < 4; ++y) dst[y] = (uint8_t)round_clamp_u8(s[y] + 128.0);
  }
}

// phase 3's pixel: the samples of column col of row r of a tile of the strip
// (chroma 4:2:2: column col uses sample col / 2)
__device__ __forceinline__ void strip_ycc(const uint8_t *ys, const uint8_t *crs,
                                          const uint8_t *cbs, int tile, int r, int col, int &Y,
                                          int &Cr, int &Cb) {
  Y = ys[tile * 64 + r * 8 + col];
  Cr = crs[tile * 32 + r * 4 + (col >> 1)];
  Cb = cbs[tile * 32 + r * 4 + (col >> 1)];
}

// phase 3's stores: a thread's four pixels, pixel k at q + 4 k where ok[k]; one
// 16-B store where all four are there and q is aligned, dwords otherwise
__device__ __forceinline__ void store_px4(uint8_t *q, const uint32_t (&px)[4],
                                          const bool (&ok)[4]) {
  if (ok[0] && ok[3] && ((((uintptr_t)q) & 15) == 0)) {
    *reinterpret_cast<uint4 *>(q) = make_uint4(px[0], px[1], px[2], px[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) reinterpret_cast<uint32_t *>(q)[k] = px[k];
  }
}

// Whole images: workgroup blockIdx.x is strip blockIdx.x % strips of tile row
// blockIdx.x / strips of image blockIdx.y.  ORIG: the tiles the reference never
// transforms take their samples from `orig` by its forward colour expressions.
template <bool ORIG>
__global__ __launch_bounds__(kThreads) void jpeg_recon_kernel(
    const int16_t *__restrict__ coef, const uint8_t *__restrict__ orig, int w, int h,
    int tiles_x, int tiles_y, int strips, uint8_t *__restrict__ out) {
  __shared__ double yac[kTiles * kYStride];     // (au*av)*(c*table), natural order
  __shared__ double crac[kTiles * kCStride];
  __shared__ double cbac[kTiles * kCStride];
  __shared__ uint8_t ys[kTiles * 64], crs[kTiles * 32], cbs[kTiles * 32];

  const int img = blockIdx.y;
  const int br = blockIdx.x / strips;
  const int bc0 = (blockIdx.x - br * strips) * kTiles;
  const int ntiles = min(kTiles, tiles_x - bc0);
  const size_t img_px = (size_t)w * (size_t)h;
  const size_t total_blocks = (img_px + 63) / 64;                    // JPEG.c:1131
  const size_t tile0 = (size_t)br * tiles_x + bc0;                   // raster index
  const int t = threadIdx.x;

  recon_dequant(coef + ((size_t)img * tiles_y * tiles_x + tile0) * 128, ntiles, t, yac, crac, cbac);
  __syncthreads();
  recon_idct(t, yac, crac, cbac, ys, crs, cbs);
  __syncthreads();

  // ---- phase 3: assemble_image (YCbCr 4:2:2 -> RGB) + coalesced stores ----
  {
    const int r = t >> 5, c = t & 31;
    const int row = br * 8 + r;
    if (row < h) {
      const uint8_t *osrc = ORIG ? orig + (size_t)img * img_px * 4 : nullptr;
      uint8_t *dst = out + (size_t)img * img_px * 4;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int lx0 = half * 128 + c * 4;          // pixel column within the strip
        uint32_t px[4];
        bool okp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int lx = lx0 + k, tile = lx >> 3, col = lx & 7;
          const int x = bc0 * 8 + lx;
          okp[k] = tile < ntiles && x < w;
          px[k] = 0;
          if (!okp[k]) continue;
          int Y, Cr, Cb;
          if (ORIG && tile0 + tile >= total_blocks) {                     // untransformed tile
            const uint8_t *p = osrc + ((size_t)row * w + x) * 4;
            Y = ref_y(p[0], p[1], p[2]);
            const int xc = bc0 * 8 + (lx & ~1) + 1;                       // odd column
            Cr = Cb = 0;
            if (xc < w) {
              const uint8_t *q = osrc + ((size_t)row * w + xc) * 4;
              Cr = ref_cr(q[0], q[1], q[2]);
              Cb = ref_cb(q[0], q[1], q[2]);
            }
          } else {
            strip_ycc(ys, crs, cbs, tile, r, col, Y, Cr, Cb);
          }
          px[k] = rgba_of(Y, Cr, Cb);
        }
        store_px4(dst + ((size_t)row * w + bc0 * 8 + lx0) * 4, px, okp);
      }
    }
  }
}

// A workgroup = a strip of up to kTiles tiles of one tile row of one
// rectangle's grid; workgroup wg of the call is rectangle wg / (ghm strips),
// grid row and strip from the remainder (ghm, strips: what a max_w x max_h
// crop can need).  A rectangle whose status is not good is skipped; the first
// workgroup of every rectangle counts it into result[0] or names it in
// result[1].  Phase 3 clips to the rectangle: image pixel (x, row) goes to
// out + dst + 4 ((row - y) w + (x - x0)).
__global__ __launch_bounds__(kThreads) void jpeg_crop_recon_kernel(
    const int16_t *__restrict__ coef, const uint32_t *__restrict__ status,
    const jpegr_rect *__restrict__ rects, size_t nrects, size_t wg_base, uint32_t gwm,
    uint32_t ghm, uint32_t strips, uint8_t *__restrict__ out, uint64_t *__restrict__ result) {
  __shared__ double yac[kTiles * kYStride];
  __shared__ double crac[kTiles * kCStride];
  __shared__ double cbac[kTiles * kCStride];
  __shared__ uint8_t ys[kTiles * 64], crs[kTiles * 32], cbs[kTiles * 32];

  const size_t wg = wg_base + blockIdx.x;
  const size_t per = (size_t)ghm * strips;
  const size_t ri = wg / per;
  if (ri >= nrects) return;
  const uint32_t rem = (uint32_t)(wg - ri * per);
  const uint32_t cy = rem / strips, bc0 = (rem - cy * strips) * kTiles;
  const int t = threadIdx.x;
  const uint32_t stat = status[ri];
  if (rem == 0 && t == 0) {
    if (stat == jpegr_crop::kBad)
      atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 1ull + (unsigned long long)ri);
    else
      atomicAdd(reinterpret_cast<unsigned long long *>(result), 1ull);
  }
  if (stat != jpegr_crop::kGood) return;
  const jpegr_rect rc = rects[ri];
  const jpegr_crop::Grid g = jpegr_crop::grid_of(rc);
  if (cy >= g.gh || bc0 >= g.gw) return;
  const int ntiles = (int)min((uint32_t)kTiles, g.gw - bc0);

  recon_dequant(coef + ((ri * gwm * ghm) + (size_t)cy * g.gw + bc0) * 128, ntiles, t, yac, crac, cbac);
  __syncthreads();
  recon_idct(t, yac, crac, cbac, ys, crs, cbs);
  __syncthreads();

  // ---- phase 3: YCbCr 4:2:2 -> RGB of the pixels inside the rectangle --------
  {
    const int r = t >> 5, c = t & 31;
    const uint64_t row = ((uint64_t)(g.ty0 + cy) << 3) + (uint64_t)r;     // image row
    if (row < rc.y || row >= rc.y + rc.h) return;
    uint8_t *const dst = out + rc.dst + (row - rc.y) * rc.w * 4;          // the crop's row
    const uint64_t sx0 = (uint64_t)(g.tx0 + bc0) << 3;                    // the strip's first column
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int lx0 = half * 128 + c * 4;            // pixel column within the strip
      uint32_t px[4];
      bool okp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int lx = lx0 + k, tile = lx >> 3, col = lx & 7;
        const uint64_t x = sx0 + (uint64_t)lx;
        okp[k] = tile < ntiles && x >= rc.x && x < rc.x + rc.w;
        px[k] = 0;
        if (!okp[k]) continue;
        int Y, Cr, Cb;
        strip_ycc(ys, crs, cbs, tile, r, col, Y, Cr, Cb);
        px[k] = rgba_of(Y, Cr, Cb);
      }
      // pixel k is column xo + k of the rectangle, stored only where that is inside
      const int64_t xo = (int64_t)(sx0 + (uint64_t)lx0) - (int64_t)rc.x;
      store_px4(dst + xo * 4, px, okp);
    }
  }
}

// ---- crops as tensors (jpegr_crop_tensor_device, include/jpegr.h) -------------
// The element, its type and the normalisation (TensorElem, tensor_elem,
// TensorNorm): jpegr_tensor_elem.h.

// B bytes (dwords wd) to p, whose address is A0 mod 16 (A0 a multiple of 4):
// from the front, the widest of 16, 8 and 4 B that the address there and the
// rest allow -- 48 B at 8 mod 16 go as 8, 16, 16, 8.
template <int A0, int B, int OFF = 0>
__device__ __forceinline__ void store_words(uint8_t *p, const uint32_t *wd) {
  if constexpr (OFF < B) {
    constexpr int pos = (A0 + OFF) & 15, rem = B - OFF;
    constexpr int n = (pos == 0 && rem >= 16) ? 16 : ((pos & 7) == 0 && rem >= 8) ? 8 : 4;
    if constexpr (n == 16)
      *reinterpret_cast<uint4 *>(p + OFF) =
          make_uint4(wd[OFF / 4], wd[OFF / 4 + 1], wd[OFF / 4 + 2], wd[OFF / 4 + 3]);
    else if constexpr (n == 8)
      *reinterpret_cast<uint2 *>(p + OFF) = make_uint2(wd[OFF / 4], wd[OFF / 4 + 1]);
    else
      *reinterpret_cast<uint32_t *>(p + OFF) = wd[OFF / 4];
    store_words<A0, B, OFF + n>(p, wd);
  }
}

// A thread's run: 4 pixels of C elements each (C = 1: a plane's; C = 3:
// interleaved), pixel m at q + C m where ok[m].  All four there and q
// dword-aligned: wide stores by the address (store_words); else the elements
// of the pixels that are there, one by one.
template <typename E, int C>
__device__ __forceinline__ void store_run(E *q, const E (&e)[4 * C], const bool (&ok)[4]) {
  constexpr int B = 4 * C * (int)sizeof(E);
  const uint32_t a = (uint32_t)(uintptr_t)q & 15u;
  if (ok[0] && ok[3] && (a & 3u) == 0) {
    uint32_t wd[B / 4];
#pragma unroll
    for (int i = 0; i < B / 4; ++i) {
      if constexpr (sizeof(E) == 4) {
        wd[i] = e[i];
      } else if constexpr (sizeof(E) == 2) {
        wd[i] = (uint32_t)e[2 * i] | ((uint32_t)e[2 * i + 1] << 16);
      } else {
        wd[i] = (uint32_t)e[4 * i] | ((uint32_t)e[4 * i + 1] << 8) | ((uint32_t)e[4 * i + 2] << 16) |
                ((uint32_t)e[4 * i + 3] << 24);
      }
      // the packed word, opaque from here on: seen through, the f16 run was
      // taken apart again and stored as short, dword at + 2, short
      if constexpr (sizeof(E) < 4) asm volatile("" : "+v"(wd[i]));
    }
    uint8_t *const p = reinterpret_cast<uint8_t *>(q);
    if (a == 0) store_words<0, B>(p, wd);
    else if (a == 8) store_words<8, B>(p, wd);
    else if (a == 4) store_words<4, B>(p, wd);
    else store_words<12, B>(p, wd);
  } else {
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (ok[m]) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) q[C * m + ch] = e[C * m + ch];
      }
  }
}

// jpeg_crop_recon_kernel's workgroup, phases 1 and 2 and verdict counting, with
// another phase 3: the pixel's R, G and B become elements of DT (tensor_elem),
// placed by LAY -- CHW: plane ch of the crop at dst + ch w h, rows of w
// elements; HWC: pixel (i, j) at dst + 3 (i w + j), dst in elements -- and
// mirrored where flip[ri] is not 0: output column j holds crop column
// w - 1 - j.  A thread's four pixels are one run in every case (store_run):
// columns xo .. xo + 3 of the crop, or, mirrored, the same four in reverse
// order at columns w - 4 - xo .. w - 1 - xo.  Consecutive lanes hold
// consecutive runs, so the stores of a wave's row are one contiguous range
// from registers, in HWC too.
template <int DT, int LAY>
__global__ __launch_bounds__(kThreads) void jpeg_crop_tensor_kernel(
    const int16_t *__restrict__ coef, const uint32_t *__restrict__ status,
    const jpegr_rect *__restrict__ rects, size_t nrects, size_t wg_base, uint32_t gwm,
    uint32_t ghm, uint32_t strips, const uint8_t *__restrict__ flip, TensorNorm nm,
    void *__restrict__ out, uint64_t *__restrict__ result) {
  using E = typename TensorElem<DT>::type;
  __shared__ double yac[kTiles * kYStride];
  __shared__ double crac[kTiles * kCStride];
  __shared__ double cbac[kTiles * kCStride];
  __shared__ uint8_t ys[kTiles * 64], crs[kTiles * 32], cbs[kTiles * 32];

  const size_t wg = wg_base + blockIdx.x;
  const size_t per = (size_t)ghm * strips;
  const size_t ri = wg / per;
  if (ri >= nrects) return;
  const uint32_t rem = (uint32_t)(wg - ri * per);
  const uint32_t cy = rem / strips, bc0 = (rem - cy * strips) * kTiles;
  const int t = threadIdx.x;
  const uint32_t stat = status[ri];
  if (rem == 0 && t == 0) {
    if (stat == jpegr_crop::kBad)
      atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 1ull + (unsigned long long)ri);
    else
      atomicAdd(reinterpret_cast<unsigned long long *>(result), 1ull);
  }
  if (stat != jpegr_crop::kGood) return;
  const jpegr_rect rc = rects[ri];
  const jpegr_crop::Grid g = jpegr_crop::grid_of(rc);
  if (cy >= g.gh || bc0 >= g.gw) return;
  const int ntiles = (int)min((uint32_t)kTiles, g.gw - bc0);
  const bool mirror = flip != nullptr && flip[ri] != 0;           // inside [0, nrects)

  recon_dequant(coef + ((ri * gwm * ghm) + (size_t)cy * g.gw + bc0) * 128, ntiles, t, yac, crac, cbac);
  __syncthreads();
  recon_idct(t, yac, crac, cbac, ys, crs, cbs);
  __syncthreads();

  // ---- phase 3: the pixels inside the rectangle, as elements --------------------
  {
    const int r = t >> 5, c = t & 31;
    const uint64_t row = ((uint64_t)(g.ty0 + cy) << 3) + (uint64_t)r;     // image row
    if (row < rc.y || row >= rc.y + rc.h) return;
    const uint64_t plane = rc.w * rc.h;                                   // w, h < 2^31
    const uint64_t row0 = rc.dst + (row - rc.y) * rc.w * (LAY == JPEGR_LAYOUT_CHW ? 1u : 3u);
    const uint64_t sx0 = (uint64_t)(g.tx0 + bc0) << 3;                    // the strip's first column
    E *const base = static_cast<E *>(out);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int lx0 = half * 128 + c * 4;            // pixel column within the strip
      uint32_t px[4];
      bool okp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int lx = lx0 + k, tile = lx >> 3, col = lx & 7;
        const uint64_t x = sx0 + (uint64_t)lx;
        okp[k] = tile < ntiles && x >= rc.x && x < rc.x + rc.w;
        px[k] = 0;
        if (!okp[k]) continue;
        int Y, Cr, Cb;
        strip_ycc(ys, crs, cbs, tile, r, col, Y, Cr, Cb);
        px[k] = rgba_of(Y, Cr, Cb);
      }
      if (!(okp[0] || okp[1] || okp[2] || okp[3])) continue;
      // the run's first column and its pixels in the order of their addresses
      // (two's complement: a run that begins left of the rectangle has its
      // missing pixels there, and those are not stored)
      const uint64_t xo = sx0 + (uint64_t)lx0 - rc.x;
      const uint64_t j0 = mirror ? rc.w - 4 - xo : xo;
      uint32_t pm[4];
      bool okm[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        pm[m] = mirror ? px[3 - m] : px[m];
        okm[m] = mirror ? okp[3 - m] : okp[m];
      }
      if constexpr (LAY == JPEGR_LAYOUT_CHW) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          E e[4];
#pragma unroll
          for (int m = 0; m < 4; ++m)
            e[m] = tensor_elem<DT>((pm[m] >> (8 * ch)) & 255u, nm.s[ch], nm.b[ch]);
          store_run<E, 1>(base + (row0 + (uint64_t)ch * plane + j0), e, okm);
        }
      } else {
        E e[12];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch)
            e[3 * m + ch] = tensor_elem<DT>((pm[m] >> (8 * ch)) & 255u, nm.s[ch], nm.b[ch]);
        }
        store_run<E, 3>(base + (row0 + 3u * j0), e, okm);
      }
    }
  }
}

}  // namespace
