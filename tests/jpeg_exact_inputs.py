"""Input builders for the JPEG kernels' exact-arithmetic tests
(tests/test_gpu_jpeg_exact.py; coverage checked on the CPU by
tests/test_jpeg_exact_inputs.py).

Three shortcuts in csrc/jpegr.hip are exact for reasons that random images
almost never exercise:
  convert_pixel    floor(N / 1000) in integers, the reference's fp64 expression
                   only where N is a multiple of 1000
  quantize_row     (int)RN(s K), the reference's (int)(RN(aa s) / T) only
                   within 2^-30 of an integer
  round_clamp_u8   truncation plus a test of the fraction against 0.5 in place
                   of (int)round(x)
The builders here make inputs that sit on those edges: every RGB triple, DCT
coefficients that are mathematically integer multiples of the quantiser step,
and reconstructed samples that are mathematically k + 0.5.
"""
import ctypes
import functools
import math

import numpy as np

_vp = ctypes.c_void_p

ZZ8 = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34,
       27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37,
       44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
ZZ4 = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 16, 13, 10, 7, 11, 14, 17, 20, 24, 21, 18, 15, 19, 22,
       25, 28, 29, 26, 23, 27, 30, 31]
LUMA_Q = [8, 6, 6, 8, 10, 14, 18, 22, 6, 6, 7, 9, 12, 20, 22, 20, 6, 7, 8, 10, 14, 22, 25, 22,
          8, 9, 10, 14, 18, 28, 27, 22, 10, 12, 14, 18, 22, 35, 33, 26, 14, 18, 22, 22, 27, 33,
          36, 30, 18, 22, 26, 28, 33, 40, 40, 34, 22, 26, 28, 30, 36, 34, 35, 33]
CHROMA_Q = [17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99,
            66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99]

# the three basis patterns whose coefficient is an exact integer: natural (u, v)
PATTERNS = [(4, 0), (0, 4), (4, 4)]
SIGNS = np.array([1, -1, -1, 1, 1, -1, -1, 1])      # sign of cos((2x+1) 4 pi / 16)

GUARD = 2.0 ** -30                                    # quantize_row's band


def dct_matrix(n):
    """D_n[u][x] = alpha_n(u) cos((2x+1) u pi / 2n): orthonormal DCT-II."""
    u = np.arange(n)[:, None]
    x = np.arange(n)[None, :]
    d = np.cos((2 * x + 1) * u * np.pi / (2 * n)) * np.sqrt(2.0 / n)
    d[0] = np.sqrt(1.0 / n)
    return d


# ---- oracle views --------------------------------------------------------
def planes(oracle, rgba):
    """jo_planes: full-resolution Y, Cr, Cb of an (h, w, 4) image."""
    h, w = rgba.shape[:2]
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    y = np.empty((h, w), np.uint8)
    cr = np.empty((h, w), np.uint8)
    cb = np.empty((h, w), np.uint8)
    oracle.L.jo_planes(a.ctypes.data_as(_vp), w, h, y.ctypes.data_as(_vp),
                       cr.ctypes.data_as(_vp), cb.ctypes.data_as(_vp))
    return y, cr, cb


def decode_tile(oracle, coef128):
    """jo_decode_tile: one tile's 128 zigzag int16 -> Y (8, 8), Cr (8, 4), Cb (8, 4)."""
    fn = oracle.L.jo_decode_tile
    fn.argtypes = [_vp, _vp, _vp, _vp]
    fn.restype = None
    c = np.ascontiguousarray(coef128, dtype=np.int16)
    y = np.empty(64, np.uint8)
    cr = np.empty(32, np.uint8)
    cb = np.empty(32, np.uint8)
    fn(c.ctypes.data_as(_vp), y.ctypes.data_as(_vp), cr.ctypes.data_as(_vp),
       cb.ctypes.data_as(_vp))
    return y.reshape(8, 8), cr.reshape(8, 4), cb.reshape(8, 4)


# ---- 1. every RGB triple ---------------------------------------------------
SLICES = 16
SLICE_PX = 1 << 20


def slice_image(k):
    """1024 x 1024 RGBA whose pixel i (raster) is triple k 2^20 + i, with
    triple index = R | G << 8 | B << 16; alpha 255."""
    idx = np.arange(k * SLICE_PX, (k + 1) * SLICE_PX, dtype=np.uint32) | np.uint32(0xFF000000)
    return idx.view(np.uint8).reshape(1024, 1024, 4).copy()      # little-endian: R, G, B, A


def doubled_slice_image(k):
    """2048 x 1024: triple i of the slice fills pixel columns 2c and 2c + 1
    (i = 1024 row + c), so the encoder's luma sees it twice and its
    odd-column chroma once."""
    return np.ascontiguousarray(np.repeat(slice_image(k), 2, axis=1))


@functools.lru_cache(maxsize=None)
def slice_planes(oracle, k):
    """jo_planes of slice_image(k), computed once per slice."""
    out = planes(oracle, slice_image(k))
    for a in out:
        a.setflags(write=False)
    return out


def colour_numerators(k):
    """convert_pixel's integer dot products for the triples of slice k."""
    i = np.arange(k * SLICE_PX, (k + 1) * SLICE_PX, dtype=np.int64)
    r, g, b = i & 255, (i >> 8) & 255, (i >> 16) & 255
    return (299 * r + 587 * g + 114 * b,
            128000 + 439 * r - 368 * g - 71 * b,
            128000 - 148 * r - 291 * g + 439 * b)


def samples_from_raw(raw, w, h):
    """Invert the raw fp64 DCT (128 doubles per tile, row-major [Y 8x8][Cr 8x4]
    [Cb 8x4], raster tiles): the raw luma block is D8 f D8^T and the raw chroma
    block D8 f D4^T, so f = D8^T raw D8 and D8^T raw D4.  Returns the centred
    samples f as planes: Y (h, w), Cr (h, w / 2), Cb (h, w / 2), unrounded."""
    tx, ty = w // 8, h // 8
    t = np.asarray(raw, dtype=np.float64).reshape(ty * tx, 128)
    d8, d4 = dct_matrix(8), dct_matrix(4)
    fy = d8.T @ t[:, :64].reshape(-1, 8, 8) @ d8
    fr = d8.T @ t[:, 64:96].reshape(-1, 8, 4) @ d4
    fb = d8.T @ t[:, 96:].reshape(-1, 8, 4) @ d4

    def plane(f, cw):
        return f.reshape(ty, tx, 8, cw).transpose(0, 2, 1, 3).reshape(ty * 8, tx * cw)
    return plane(fy, 8), plane(fr, 4), plane(fb, 4)


# ---- 2. quantiser ties -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def y_to_rgb(oracle):
    """(256, 3) lookup: a near-grey RGB triple whose jo_planes luma is exactly
    the index (a grey level v gives Y == v for only 191 of the 256 levels)."""
    g, dr, db = np.meshgrid(np.arange(256), np.arange(-4, 5), np.arange(-4, 5), indexing="ij")
    cand = np.stack([np.clip(g + dr, 0, 255), g, np.clip(g + db, 0, 255), np.full_like(g, 255)],
                    axis=-1).reshape(1, -1, 4).astype(np.uint8)
    y = planes(oracle, cand)[0].ravel()
    cost = (np.abs(cand[0, :, 0].astype(int) - cand[0, :, 1]) +
            np.abs(cand[0, :, 2].astype(int) - cand[0, :, 1]))
    lut = np.zeros((256, 3), np.uint8)
    for level in range(256):
        hit = np.flatnonzero(y == level)
        assert hit.size, f"no candidate triple has luma {level}"
        lut[level] = cand[0, hit[np.argmin(cost[hit])], :3]
    lut.setflags(write=False)
    return lut


# -40, 0, 17: near-integer quotients on both sides; -45, -3, 62: the offsets of the
# whole family (every d, every a) at which quantize_row's fast product most often
# lands on an integer while the reference's quotient lies just below it
QUANT_OFFSETS = (-45, -40, -3, 0, 17, 62)
QUANT_TILES_X = 32


def quant_tie_tiles():
    """(pattern, d, a) of every tile: luma plane 128 + d + a P, all in 0..255."""
    out = []
    for p in range(len(PATTERNS)):
        for d in QUANT_OFFSETS:
            for a in range(1, 128):
                if 0 <= 128 + d - a and 128 + d + a <= 255:
                    out.append((p, d, a))
    return out


def pattern(p):
    """8 x 8 matrix of +-1: the sign of DCT basis function PATTERNS[p]."""
    u, v = PATTERNS[p]
    rows = SIGNS if u == 4 else np.ones(8, int)
    cols = SIGNS if v == 4 else np.ones(8, int)
    return rows[:, None] * cols[None, :]


@functools.lru_cache(maxsize=None)
def quant_tie_image(oracle):
    """RGBA image of near-grey tiles whose luma planes are 128 + d + a P.  The
    luma coefficient at P's (u, v) is mathematically 8 a ((4,0), (0,4)) or 16 a
    ((4,4)) and the DC 8 d, so wherever the quantiser step divides it the fp64
    quotient coef / T lies a few ulp from an integer, on either side; every
    other luma coefficient is a rounding residue that must truncate to 0.
    Trailing tiles are flat grey 128."""
    tiles = quant_tie_tiles()
    tx = QUANT_TILES_X
    ty = (len(tiles) + tx - 1) // tx
    luma = np.full((ty * 8, tx * 8), 128, int)
    for i, (p, d, a) in enumerate(tiles):
        r, c = divmod(i, tx)
        luma[8 * r:8 * r + 8, 8 * c:8 * c + 8] = 128 + d + a * pattern(p)
    img = np.empty((ty * 8, tx * 8, 4), np.uint8)
    img[..., :3] = y_to_rgb(oracle)[luma]
    img[..., 3] = 255
    assert np.array_equal(planes(oracle, img)[0], luma)
    img.setflags(write=False)
    return img


def quotients(oracle, rgba):
    """The oracle's coef / T before truncation: (tiles, 128), row-major planes."""
    raw = oracle.jpeg_dct_raw(rgba).reshape(-1, 128)
    t = np.array(LUMA_Q + CHROMA_Q + CHROMA_Q, dtype=np.float64)
    return raw / t


def luma_fast_and_reference_quotients(oracle, rgba):
    """quantize_row's two formulas for every luma coefficient of an image whose
    sides are multiples of 8, restated in numpy: the fast path's r = RN(s K) with
    K = RN(aa RN(1 / T)), and the reference's RN(aa s) / T, from the sum s
    accumulated in the reference's order (x outer, y inner, (cv cos_x) cos_y)
    with the reference's cos / alpha expressions.  RN(aa s) is checked against
    the oracle's raw DCT bit for bit.  Returns (r, ref), each (tiles, 64)."""
    h, w = rgba.shape[:2]
    pi = 3.14159265358979323846                                   # JPEG.c:11
    c8 = [[math.cos((pi * float(2 * x + 1) * float(u)) / 16.0) for u in range(8)]
          for x in range(8)]
    al = [math.sqrt(1.0 / 8)] + [math.sqrt(2.0 / 8)] * 7
    y = planes(oracle, rgba)[0].astype(np.float64) - 128.0
    cv = y.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    raw = oracle.jpeg_dct_raw(rgba).reshape(-1, 128)
    r = np.empty((cv.shape[0], 64))
    ref = np.empty_like(r)
    for u in range(8):
        for v in range(8):
            acc = np.zeros(cv.shape[0])
            for x in range(8):
                for yy in range(8):
                    acc = acc + (cv[:, x, yy] * c8[x][u]) * c8[yy][v]
            aa = al[u] * al[v]
            t = float(LUMA_Q[u * 8 + v])
            assert np.array_equal(aa * acc, raw[:, u * 8 + v]), (u, v)
            r[:, u * 8 + v] = acc * (aa * (1.0 / t))
            ref[:, u * 8 + v] = (aa * acc) / t
    return r, ref


# ---- 3. reconstruction ties and clamps -------------------------------------
RECON_TILES_X = 40          # a full strip of 32 tiles and a partial one of 8
RECON_Q = [s * m for m in (2, 6, 10, 14, 18, 22, 26) for s in (1, -1)]     # q = 2 (mod 4)
RECON_Q0 = (-150, -131, -64, -1, 0, 37, 99, 120, 140)


@functools.lru_cache(maxsize=None)
def recon_tie_coef():
    """(coef int16 (tiles, 128) zigzag, w, h).  Luma: DC q0 and one coefficient
    q = 2 (mod 4) at (4,0), (0,4) or (4,4).  Dequantised (steps 8, 10, 10, 22)
    and inverse transformed these give 128 + q0 +- 1.25 q, or +- 2.75 q at
    (4,4): every luma sample is mathematically on a .5 tie, and q0 ranges far
    enough that some fall below 0 and some above 255.5.  Chroma: a DC and one
    low-frequency coefficient per plane, stepping through tiles with periods
    coprime to the luma's, so that Cr and Cb cover 0..255 (clamped at both
    ends) and the RGB assembly clamps at both ends.  No chroma sample is near
    a tie: every 8 x 4 basis value is irrational."""
    tiles = [(p, q, q0) for p in range(len(PATTERNS)) for q in RECON_Q for q0 in RECON_Q0]
    tx = RECON_TILES_X
    ty = (len(tiles) + tx - 1) // tx
    coef = np.zeros((ty * tx, 128), np.int16)
    inv8 = {n: z for z, n in enumerate(ZZ8)}
    for i in range(ty * tx):
        p, q, q0 = tiles[i % len(tiles)]
        u, v = PATTERNS[p]
        coef[i, 0] = q0
        coef[i, inv8[u * 8 + v]] = q
        coef[i, 64] = ((i * 7) % 23 - 11) * 4               # Cr DC: 128 + ~3.005 x
        coef[i, 64 + 1 + i % 5] = (i * 3) % 9 - 4
        coef[i, 96] = ((i * 5) % 19 - 9) * 5                # Cb DC
        coef[i, 96 + 1 + i % 4] = (i * 2) % 7 - 3
    coef.setflags(write=False)
    return coef, tx * 8, ty * 8


def recon_presums(coef):
    """Pre-rounding sample values s + 128 of every tile in plain numpy (not
    bit-exact to the reference's summation; good to ~1e-12): Y (tiles, 8, 8),
    Cr and Cb (tiles, 8, 4)."""
    d8, d4 = dct_matrix(8), dct_matrix(4)
    c = np.asarray(coef, dtype=np.float64)
    y = np.zeros((c.shape[0], 64))
    y[:, ZZ8] = c[:, :64]
    y = (y * np.array(LUMA_Q, float)).reshape(-1, 8, 8)
    out = [d8.T @ y @ d8 + 128.0]
    for o in (64, 96):
        ch = np.zeros((c.shape[0], 32))
        ch[:, ZZ4] = c[:, o:o + 32]
        ch = (ch * np.array(CHROMA_Q, float)).reshape(-1, 8, 4)
        out.append(d8.T @ ch @ d4 + 128.0)
    return out


def _trunc(k, d):
    return np.trunc(k * d.astype(np.float64)).astype(np.int64)     # (int)(k * d), fp64


def assemble_unclamped(oracle, coef, w, h):
    """The oracle's R, G, B before the final clamp, (h, w, 3) ints, for zigzag
    coefficients of a w x h image (both multiples of 8): jo_decode_tile per
    tile, then jo_reconstruct_image's assembly (YCbCr 4:2:2 -> RGB with
    truncating casts) restated in numpy."""
    tx, ty = w // 8, h // 8
    coef = np.asarray(coef).reshape(ty * tx, 128)
    ys = np.empty((ty, 8, tx, 8), np.int64)
    crs = np.empty((ty, 8, tx, 4), np.int64)
    cbs = np.empty((ty, 8, tx, 4), np.int64)
    for i in range(ty * tx):
        r, c = divmod(i, tx)
        ys[r, :, c], crs[r, :, c], cbs[r, :, c] = decode_tile(oracle, coef[i])
    y = ys.reshape(h, w)
    cr = np.repeat(crs.reshape(h, w // 2), 2, axis=1) - 128      # column c uses sample c / 2
    cb = np.repeat(cbs.reshape(h, w // 2), 2, axis=1) - 128
    out = np.stack([y + _trunc(1.402, cr),
                    y - _trunc(0.344136, cb) - _trunc(0.714136, cr),
                    y + _trunc(1.772, cb)], axis=-1)
    return out


def clamp_rgba(rgb):
    """jo_clamp of (h, w, 3) ints, alpha 255: (h, w, 4) uint8."""
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = np.clip(rgb, 0, 255)
    return out


@functools.lru_cache(maxsize=None)
def recon_unclamped(oracle):
    """assemble_unclamped of recon_tie_coef(), computed once."""
    out = assemble_unclamped(oracle, *recon_tie_coef())
    out.setflags(write=False)
    return out


def recon_expected(oracle):
    """The oracle's RGBA image for recon_tie_coef()."""
    return clamp_rgba(recon_unclamped(oracle))
