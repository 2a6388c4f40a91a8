// jpegr.hip -- MI355X (gfx950) JPEG hot path: fused RGBA -> Y/Cr/Cb ->
// 4:2:2 odd-column subsample -> 8x8 / 8x4 tiles -> fp64 DCT-II -> truncating
// quantisation -> zigzag -> int16, one workgroup per 32-tile strip.
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
// Work split (per workgroup of 256 threads = 4 waves, 32 tiles of one tile
// row):
//   phase 1  every thread converts 8 pixels (2 x 16-B loads, coalesced 1 KiB
//            rows) into centred doubles in LDS: Y tiles [32][64], Cr/Cb [32][32]
//   phase 2  thread = (tile, u): Y row u, all 8 v  (64 products c*C8[x][u]
//            shared by the 8 outputs: 2.125 fp64 ops per term, exact order)
//   phase 3  thread = (tile, u): Cr and Cb row u, 4 v each
//   phase 4  the strip's 32 x 256 B of int16 leave as coalesced 16-B stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "jpeg_tables.h"
#include "jpegr_crop.h"
#include "jpegr_pixel.h"
#include "../../include/jpegr.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTiles = 32;       // tiles per workgroup strip
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

__constant__ double dC8[8][8];
__constant__ double dAA88[8][8];
__constant__ double dAA84[8][4];
__constant__ int dLQ[64];
__constant__ int dCQ[32];
__constant__ double dLK[64];    // RN(alpha_u alpha_v * RN(1 / T)): the quantisation's fast path
__constant__ double dCK[32];
__constant__ int dZZ8b[64];     // 2 * zigzag position: the int16's byte offset in the tile
__constant__ int dZZ4b[32];
__constant__ int dZZ8inv[64];   // zigzag index -> natural index
__constant__ int dZZ4inv[32];
// reconstruction, per position z of a tile's 128 zigzagged int16 ([Y 64][Cr 32][Cb 32]):
// the natural index within its plane, the quantiser step and the alpha product
// of that index -- one load each, none depending on another
__constant__ int dRZn[128];
__constant__ double dRZq[128];
__constant__ double dRZa[128];

// One pixel's contribution to the tile planes (JPEG.c:127, 157, 180;
// chroma only from odd columns: chroma_subsample JPEG.c:329-331 +
// divide_image JPEG.c:540-544).  `valid` = inside the image.
//
// The reference evaluates Y = (uint8_t)((0.299 R + 0.587 G) + 0.114 B) and
// Cr / Cb = clamp((int)(... + 128.0)) in fp64.  With N = 299 R + 587 G + 114 B
// (Cr: 439 R - 368 G - 71 B + 128000, Cb: -148 R - 291 G + 439 B + 128000;
// all positive), the fp64 value lies within 1e-13 of N / 1000 (three
// roundings of the constants, three of the products, three or four of the
// sums, each far below 2^-43 at these magnitudes), so its truncation is
// floor(N / 1000) whenever N is not a multiple of 1000 (the fraction is then
// in [0.001, 0.999]).  Those lanes take the integer path: N by 24-bit
// multiply-adds, the quotient by one v_mul_hi_u32_u24 with ceil(2^32 / 1000)
// (exact for N < 2^18), the remainder by one multiply-add.  A lane whose N is
// a multiple of 1000 (about 1 in 1000) evaluates the reference's fp64
// expression, behind a branch taken only when some lane needs it.  The
// Cr / Cb quotients stay within 16..239 for every RGB triple, so clamp_u8
// (kept because the reference has it, JPEG.c:157, 180) can never fire here.
// Pinned on all 2^24 triples: the fp64 result differs from floor(N / 1000)
// at 3464 (Y), 102 (Cr) and 35 (Cb) triples, every one a multiple of 1000
// (tests/test_jpeg_exact_inputs.py; the kernel: tests/test_gpu_jpeg_exact.py).
__device__ __forceinline__ uint32_t div1000(uint32_t N) {       // N < 2^18
  return (uint32_t)(((uint64_t)N * 4294968u) >> 32);
}

__device__ __forceinline__ void convert_pixel(uint32_t p, bool valid, int r,
                                              int px, double *ylds,
                                              double *crl, double *cbl) {
  const int tile = px >> 3, col = px & 7;
  const unsigned R = p & 255u, G = (p >> 8) & 255u, B = (p >> 16) & 255u;
  int yv = 0;
  if (valid) {
    const uint32_t N = 299u * R + 587u * G + 114u * B;
    const uint32_t q = div1000(N);
    yv = (int)q;
    if (N == 1000u * q) {                      // on an integer: the reference's fp64
      double y = 0.299 * (double)R + 0.587 * (double)G + 0.114 * (double)B;
      yv = (int)(uint8_t)(unsigned)y;          // (uint8_t) of a double in [0,256)
    }
  }
  ylds[tile * kYStride + r * 8 + col] = (double)(yv - 128);   // JPEG.c:467
  if (col & 1) {
    int crv = 0, cbv = 0;
    if (valid) {
      const uint32_t Nr = 128000u + 439u * R - 368u * G - 71u * B;   // > 0
      const uint32_t Nb = 128000u + 439u * B - 148u * R - 291u * G;  // > 0
      const uint32_t qr = div1000(Nr), qb = div1000(Nb);
      crv = clamp_u8((int)qr);
      cbv = clamp_u8((int)qb);
      if (Nr == 1000u * qr)
        crv = clamp_u8((int)(0.439 * (double)R - 0.368 * (double)G -
                             0.071 * (double)B + 128.0));
      if (Nb == 1000u * qb)
        cbv = clamp_u8((int)(-0.148 * (double)R - 0.291 * (double)G +
                             0.439 * (double)B + 128.0));
    }
    const int ci = tile * kCStride + r * 4 + (col >> 1);
    crl[ci] = (double)(crv - 128);
    cbl[ci] = (double)(cbv - 128);
  }
}

// q = (int)(coef / T) (JPEG.c:626-627, IEEE division then truncation) for a
// row of W coefficients coef = RN(aa * s) (JPEG.c:489).  The fast path is
// r = RN(s * K) with K = RN(aa * RN(1/T)) (one multiply instead of two): r
// lies within ~4 ulp of coef / T (|r| < 2^12: within 2^-39), so trunc(r) and
// trunc(coef / T) differ only when coef / T is that close to an integer; a
// lane whose r is within 2^-30 of an integer (exact quotients and zeros
// included) takes the reference's path, coef = RN(aa * s) and the IEEE
// division.  The near-integer tests collect into one SGPR lane mask (no
// per-lane flag arithmetic), and the fallback runs behind one wave-uniform
// branch, so the division sequence runs only when some lane of the wave
// needs it.
//
// Pinned by tests/test_gpu_jpeg_exact.py on tiles 128 + d + a P (P a basis
// sign pattern of (4,0), (0,4) or (4,4)), whose luma quotients lie a few ulp
// on either side of nonzero integers.  Without the fallback 27 coefficients
// of that image come out one too large.  In all 27, and in all 581 such
// cases over every d and a, r is exactly an integer and coef / T just below
// it: a band of width zero (exact integers only) gives the same output on
// that family, so the fast path is more accurate than the ~4 ulp bound above
// allows for, and the 2^-30 is margin that no known input needs.  Chroma
// reaches the band only with near-zero residues there (no 8 x 4 coefficient
// of those tiles is near a nonzero multiple of its step).
template <int W>
__device__ __forceinline__ void quantize_row(const double (&sm)[W], const double *K,
                                             const double *aa, const int *T, int (&q)[W]) {
  uint64_t slow = 0;
#pragma unroll
  for (int v = 0; v < W; ++v) {
    const double r = sm[v] * K[v];
    slow |= __builtin_amdgcn_ballot_w64(!(fabs(r - __builtin_rint(r)) > 0x1p-30));
    q[v] = (int)r;
  }
  if (slow) {
#pragma unroll
    for (int v = 0; v < W; ++v) {
      const double r = sm[v] * K[v];
      if (!(fabs(r - __builtin_rint(r)) > 0x1p-30)) q[v] = (int)((aa[v] * sm[v]) / (double)T[v]);
    }
  }
}

template <bool RAW>
__global__ __launch_bounds__(kEThreads) void jpeg_strip_kernel(
    const uint8_t *__restrict__ rgba, int w, int h, int tiles_x, int tiles_y,
    int strips, void *__restrict__ out) {
  // 16-B aligned: phase 4 reads the int16 output staged over it as uint4
  __shared__ alignas(16) double ylds[kETiles * kYStride];
  __shared__ double crl[kETiles * kCStride];
  __shared__ double cbl[kETiles * kCStride];
  // the strip's int16 output is staged over the luma samples once every
  // thread holds its coefficients in registers (34 KB of LDS: 4 WGs per CU)
  int16_t *const olds = reinterpret_cast<int16_t *>(ylds);

  const int img = blockIdx.y;
  const int br = blockIdx.x / strips;
  const int bc0 = (blockIdx.x - br * strips) * kETiles;
  const int ntiles = min(kETiles, tiles_x - bc0);
  const size_t img_px = (size_t)w * (size_t)h;
  const uint8_t *src = rgba + (size_t)img * img_px * 4;
  const int t = threadIdx.x;

  // ---- phase 1: colour conversion into LDS --------------------------------
  {
    const int r = t / kETiles;      // tile row 0..7
    const int c = t % kETiles;
    const int row = br * 8 + r;
    const bool row_ok = row < h;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int lx = half * (4 * kETiles) + c * 4;   // pixel column within the strip
      const int x = bc0 * 8 + lx;
      uint32_t p[4];
      bool ok[4];
      if (row_ok && ((w & 3) == 0) && x + 3 < w) {
        const uint4 v = *reinterpret_cast<const uint4 *>(
            src + ((size_t)row * w + x) * 4);
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        ok[0] = ok[1] = ok[2] = ok[3] = true;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ok[k] = row_ok && (x + k < w);
          p[k] = 0;
          if (ok[k]) {
            const uint8_t *q = src + ((size_t)row * w + x + k) * 4;
            p[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) convert_pixel(p[k], ok[k], r, lx + k, ylds, crl, cbl);
    }
  }
  __syncthreads();

  const int tile = t >> 3;   // 0..31
  const int u = t & 7;
  const size_t tile_g = ((size_t)img * tiles_y + br) * tiles_x + bc0 + tile;
  const bool tile_ok = tile < ntiles;

  double cx[8];
#pragma unroll
  for (int x = 0; x < 8; ++x) cx[x] = dC8[x][u];

  int qy[8], qc[2][4];
  // ---- phase 2: luma DCT row u (JPEG.c:471-491 with W=H=8) -----------------
  {
    const double *yt = ylds + tile * kYStride;
    double s[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) s[v] = 0.0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        const double tv = yt[x * 8 + y] * cx[x];                 // cv*cos_x
#pragma unroll
        for (int v = 0; v < 8; ++v)
          s[v] = s[v] + tv * jpegr_tables::C8[y][v];             // *cos_y, +=
      }
    }
    if (RAW) {
#pragma unroll
      for (int v = 0; v < 8; ++v)                                 // JPEG.c:489
        if (tile_ok) static_cast<double *>(out)[tile_g * 128 + u * 8 + v] = dAA88[u][v] * s[v];
    } else {
      quantize_row<8>(s, &dLK[u * 8], &dAA88[u][0], &dLQ[u * 8], qy);   // JPEG.c:489, 626-627
    }

  }

  // ---- phase 3: chroma DCTs row u (JPEG.c:1139-1140: width 4, height 8) ----
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const double *ct = (ch == 0 ? crl : cbl) + tile * kCStride;
    double s[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) s[v] = 0.0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const double tv = ct[x * 4 + y] * cx[x];
#pragma unroll
        for (int v = 0; v < 4; ++v) s[v] = s[v] + tv * jpegr_tables::C4[y][v];
      }
    }
    if (RAW) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (tile_ok)
          static_cast<double *>(out)[tile_g * 128 + 64 + ch * 32 + u * 4 + v] = dAA84[u][v] * s[v];
    } else {
      quantize_row<4>(s, &dCK[u * 4], &dAA84[u][0], &dCQ[u * 4], qc[ch]);
    }
  }

  if (RAW) return;
  __syncthreads();                   // every thread is done reading the samples
  {
    // zigzag (JPEG.c:693-728) by byte offsets from the tables
    uint8_t *const ob = reinterpret_cast<uint8_t *>(olds) + tile * 256;
#pragma unroll
    for (int v = 0; v < 8; ++v) *reinterpret_cast<int16_t *>(ob + dZZ8b[u * 8 + v]) = (int16_t)qy[v];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        *reinterpret_cast<int16_t *>(ob + 128 + ch * 64 + dZZ4b[u * 4 + v]) = (int16_t)qc[ch][v];
  }
  __syncthreads();

  // ---- phase 4: coalesced store of the strip's tiles -------------------------
  {
    uint8_t *dst = static_cast<uint8_t *>(out) +
                   (((size_t)img * tiles_y + br) * tiles_x + bc0) * 256;
    const int bytes = ntiles * 256;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int off = (k * kEThreads + t) * 16;
      if (off < bytes)
        *reinterpret_cast<uint4 *>(dst + off) =
            *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(olds) + off);
    }
  }
}

// ---- reconstruction: the decode side of the reference's main --------------
// (JPEG.c:1131-1425 minus the entropy round trip, which is the identity on
// the coefficients): per tile, reverse zigzag + Inverse_quantize (:631-638),
// fp64 IDCT in the reference's order (:399-448: for each (x, y) the sum over
// u outer, v inner of (((au*av)*c)*cos_x)*cos_y, then (int)round(s + 128)
// clamped), and assemble_image's YCbCr 4:2:2 -> RGB (:553-619).  Tiles at
// index >= ceil(W*H/64) are never transformed by the reference (:1131) and
// keep their original samples: taken from `orig` when given.
// Workgroup = 256 threads on a strip of 32 tiles of one tile row.
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

  // ---- phase 1: coefficients -> dequantised, alpha-scaled doubles ---------
  // Thread t takes the 8 coefficients z0 .. z0 + 7 (z0 = 8 (t mod 16)) of
  // tiles t / 16 and 16 + t / 16, so its natural indices, quantiser steps and
  // alpha products are looked up once for both tiles.
  {
    const int16_t *src = coef + ((size_t)img * tiles_y * tiles_x + tile0) * 128;
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
  __syncthreads();

  // ---- phase 2: IDCT, thread = (tile, x) ----------------------------------
  {
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
            const double R0 = p[0], G0 = p[1], B0 = p[2];
            Y = (int)(uint8_t)(unsigned)(0.299 * R0 + 0.587 * G0 + 0.114 * B0);
            const int xc = bc0 * 8 + (lx & ~1) + 1;                       // odd column
            Cr = Cb = 0;
            if (xc < w) {
              const uint8_t *q = osrc + ((size_t)row * w + xc) * 4;
              const double R = q[0], G = q[1], B = q[2];
              Cr = clamp_u8((int)(0.439 * R - 0.368 * G - 0.071 * B + 128.0));
              Cb = clamp_u8((int)(-0.148 * R - 0.291 * G + 0.439 * B + 128.0));
            }
          } else {
            Y = ys[tile * 64 + r * 8 + col];
            Cr = crs[tile * 32 + r * 4 + (col >> 1)];
            Cb = cbs[tile * 32 + r * 4 + (col >> 1)];
          }
          const int R = Y + colour_term(1.402f, Cr - 128);            // JPEG.c:601
          const int G = Y - colour_term(0.344136f, Cb - 128) -
                        colour_term(0.714136f, Cr - 128);
          const int B = Y + colour_term(1.772f, Cb - 128);
          px[k] = (uint32_t)clamp_u8(R) | ((uint32_t)clamp_u8(G) << 8) |
                  ((uint32_t)clamp_u8(B) << 16) | (255u << 24);
        }
        const int x0 = bc0 * 8 + lx0;
        uint8_t *q = dst + ((size_t)row * w + x0) * 4;
        if (okp[0] && okp[3] && ((((uintptr_t)q) & 15) == 0)) {
          *reinterpret_cast<uint4 *>(q) = make_uint4(px[0], px[1], px[2], px[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (okp[k]) reinterpret_cast<uint32_t *>(q)[k] = px[k];
        }
      }
    }
  }
}

// ---- crops: jpegr_crop_device's reconstruction half (jpegr_crop.h) -----------
// jpeg_recon_kernel's phases 1 and 2 as functions, statement for statement (the
// same tables, products, summation order and round_clamp_u8: bit-exactness
// rests on that order).  jpeg_recon_kernel itself keeps its body: calling
// these from it -- both, the IDCT alone, or only the IDCT's summation loops --
// reorders its instructions and moves its SGPR count (105 -> 97), and its code
// is not to move.  t: the thread of 256; a strip of up to kTiles
// tiles, `ntiles` of them live, tile i's 128 int16 at src + 128 i.

// phase 1: coefficients -> dequantised, alpha-scaled doubles in LDS.
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
        const int Y = ys[tile * 64 + r * 8 + col];
        const int Cr = crs[tile * 32 + r * 4 + (col >> 1)];
        const int Cb = cbs[tile * 32 + r * 4 + (col >> 1)];
        const int R = Y + colour_term(1.402f, Cr - 128);            // JPEG.c:601
        const int G = Y - colour_term(0.344136f, Cb - 128) -
                      colour_term(0.714136f, Cr - 128);
        const int B = Y + colour_term(1.772f, Cb - 128);
        px[k] = (uint32_t)clamp_u8(R) | ((uint32_t)clamp_u8(G) << 8) |
                ((uint32_t)clamp_u8(B) << 16) | (255u << 24);
      }
      // pixel k's dword, addressed only where pixel k is inside
      const int64_t xo = (int64_t)(sx0 + (uint64_t)lx0) - (int64_t)rc.x;
      if (okp[0] && okp[3] && ((((uintptr_t)dst + (uint64_t)xo * 4) & 15) == 0)) {
        *reinterpret_cast<uint4 *>(dst + xo * 4) = make_uint4(px[0], px[1], px[2], px[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (okp[k]) *reinterpret_cast<uint32_t *>(dst + (xo + k) * 4) = px[k];
      }
    }
  }
}


bool g_tables_ready[64] = {false};

hipError_t upload_tables() {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && g_tables_ready[dev]) return hipSuccess;
  using namespace jpegr_tables;
  int lq[64], cq[32], z8[64], z4[32];
  for (int i = 0; i < 64; ++i) { lq[i] = LUMA_Q[i]; z8[i] = ZZ8_POS[i]; }
  for (int i = 0; i < 32; ++i) { cq[i] = CHROMA_Q[i]; z4[i] = ZZ4_POS[i]; }
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dC8), C8, sizeof(C8))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dAA88), AA88, sizeof(AA88))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dAA84), AA84, sizeof(AA84))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dLQ), lq, sizeof(lq))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dCQ), cq, sizeof(cq))) != hipSuccess) return e;
  // K = RN(alpha_u alpha_v * RN(1 / T)), both IEEE double operations
  double lk[64], ck[32];
  for (int i = 0; i < 64; ++i) lk[i] = AA88[i / 8][i % 8] * (1.0 / (double)lq[i]);
  for (int i = 0; i < 32; ++i) ck[i] = AA84[i / 4][i % 4] * (1.0 / (double)cq[i]);
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dLK), lk, sizeof(lk))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dCK), ck, sizeof(ck))) != hipSuccess) return e;
  int z8b[64], z4b[32];
  for (int i = 0; i < 64; ++i) z8b[i] = 2 * z8[i];
  for (int i = 0; i < 32; ++i) z4b[i] = 2 * z4[i];
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dZZ8b), z8b, sizeof(z8b))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dZZ4b), z4b, sizeof(z4b))) != hipSuccess) return e;
  int i8[64], i4[32];
  for (int i = 0; i < 64; ++i) i8[ZZ8_POS[i]] = i;
  for (int i = 0; i < 32; ++i) i4[ZZ4_POS[i]] = i;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dZZ8inv), i8, sizeof(i8))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dZZ4inv), i4, sizeof(i4))) != hipSuccess) return e;
  int rzn[128];
  double rzq[128], rza[128];
  for (int z = 0; z < 128; ++z) {
    if (z < 64) {
      const int n = i8[z];
      rzn[z] = n;
      rzq[z] = (double)lq[n];
      rza[z] = AA88[n >> 3][n & 7];
    } else {
      const int n = i4[(z - 64) & 31];
      rzn[z] = n;
      rzq[z] = (double)cq[n];
      rza[z] = AA84[n >> 2][n & 3];
    }
  }
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dRZn), rzn, sizeof(rzn))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dRZq), rzq, sizeof(rzq))) != hipSuccess) return e;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(dRZa), rza, sizeof(rza))) != hipSuccess) return e;
  if (dev >= 0 && dev < 64) g_tables_ready[dev] = true;
  return hipSuccess;
}

int launch(bool raw, const void *d_rgba, int w, int h, int nimg, void *d_out,
           void *stream) {
  if (!d_rgba || !d_out || w <= 0 || h <= 0 || nimg <= 0 || nimg > 65535)
    return JPEGR_ERR_ARG;
  if (upload_tables() != hipSuccess) return JPEGR_ERR_HIP;
  const int tx = (w + 7) / 8, ty = (h + 7) / 8;
  const int strips = (tx + kETiles - 1) / kETiles;
  const long long gx = (long long)ty * strips;
  if (gx > 0x7fffffffLL) return JPEGR_ERR_ARG;
  dim3 grid((unsigned)gx, (unsigned)nimg);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (raw)
    hipLaunchKernelGGL(jpeg_strip_kernel<true>, grid, dim3(kEThreads), 0, s,
                       static_cast<const uint8_t *>(d_rgba), w, h, tx, ty, strips, d_out);
  else
    hipLaunchKernelGGL(jpeg_strip_kernel<false>, grid, dim3(kEThreads), 0, s,
                       static_cast<const uint8_t *>(d_rgba), w, h, tx, ty, strips, d_out);
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}

}  // namespace

int jpegr_crop_recon_launch(const int16_t *d_coef, const uint32_t *d_status,
                            const jpegr_rect *d_rects, size_t nrects, int max_w, int max_h,
                            uint8_t *d_out, uint64_t *d_result, hipStream_t st) {
  if (upload_tables() != hipSuccess) return JPEGR_ERR_HIP;
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

extern "C" {

size_t jpegr_coef_count(int w, int h) {
  if (w <= 0 || h <= 0) return 0;
  return (size_t)((w + 7) / 8) * (size_t)((h + 7) / 8) * 128;
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
  if (!d_coef || !d_rgba_out || w <= 0 || h <= 0 || nimg <= 0 || nimg > 65535)
    return JPEGR_ERR_ARG;
  if (upload_tables() != hipSuccess) return JPEGR_ERR_HIP;
  const int tx = (w + 7) / 8, ty = (h + 7) / 8;
  const int strips = (tx + kTiles - 1) / kTiles;
  const long long gx = (long long)ty * strips;
  if (gx > 0x7fffffffLL) return JPEGR_ERR_ARG;
  dim3 grid((unsigned)gx, (unsigned)nimg);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d_rgba_orig)
    hipLaunchKernelGGL(jpeg_recon_kernel<true>, grid, dim3(kThreads), 0, s,
                       static_cast<const int16_t *>(d_coef),
                       static_cast<const uint8_t *>(d_rgba_orig), w, h, tx, ty, strips,
                       static_cast<uint8_t *>(d_rgba_out));
  else
    hipLaunchKernelGGL(jpeg_recon_kernel<false>, grid, dim3(kThreads), 0, s,
                       static_cast<const int16_t *>(d_coef), nullptr, w, h, tx, ty, strips,
                       static_cast<uint8_t *>(d_rgba_out));
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
