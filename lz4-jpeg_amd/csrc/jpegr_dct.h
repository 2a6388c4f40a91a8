// jpegr_dct.h -- the JPEG encoder's kernel (part of jpegr.hip, which defines
// the strip sizes, the LDS strides and the tables before including this):
// fused RGBA -> Y/Cr/Cb -> 4:2:2 odd-column subsample -> 8x8 / 8x4 tiles ->
// fp64 DCT-II -> truncating quantisation -> zigzag -> int16, one workgroup per
// strip of kETiles tiles.
//
// Work split (per workgroup of 256 threads = 4 waves, 32 tiles of one tile
// row):
//   phase 1  every thread converts 8 pixels (2 x 16-B loads, coalesced 1 KiB
//            rows) into centred doubles in LDS: Y tiles [32][64], Cr/Cb [32][32]
//   phase 2  thread = (tile, u): Y row u, all 8 v  (64 products c*C8[x][u]
//            shared by the 8 outputs: 2.125 fp64 ops per term, exact order)
//   phase 3  thread = (tile, u): Cr and Cb row u, 4 v each
//   phase 4  the strip's 32 x 256 B of int16 leave as coalesced 16-B stores.
#pragma once

#pragma clang fp contract(off)

namespace {

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
    if (N == 1000u * q) yv = ref_y(R, G, B);   // on an integer: the reference's fp64
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
      if (Nr == 1000u * qr) crv = ref_cr(R, G, B);
      if (Nb == 1000u * qb) cbv = ref_cb(R, G, B);
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

}  // namespace
