"""What a thumbnail is (include/jpegr.h: jpegr_thumb_device), in numpy over the
oracle (a helper, no tests; checked by test_jpr_thumb_model.py): pixel k of the
selected tiles is sample 0 of the tile reconstructed from its three DC terms
alone -- jo_decode_tile of the coefficients with every AC term 0, then
jo_reconstruct_image's integer colour lines (oracle/jpeg_oracle.c:359-366) --
and a stream's DC term is the value of the first (count, value) pair of its RLE
ints whose count is >= 1.  Also the call's result words."""
import functools

import numpy as np

import jpeg_exact_inputs as X

DC_AT = (0, 64, 96)                      # Y, Cr, Cb of a tile's 128 coefficients
OK = (1 << 64) - 1


def dc_only(coef):
    """The coefficients [ntiles, 128] with everything but the three DC terms 0."""
    coef = np.asarray(coef, np.int16).reshape(-1, 128)
    out = np.zeros_like(coef)
    out[:, DC_AT] = coef[:, DC_AT]
    return out


def dc_of_rle(rle):
    """zz[0] of jo_entropy_decode from a stream's RLE ints alone: the value of
    the first pair whose count is >= 1; 0 when there is none (a trailing count
    without a value is no pair).  A one-code stream is rle_len copies of its
    symbol, to which the same rule applies."""
    for i in range(0, len(rle) - 1, 2):
        if rle[i] >= 1:
            return int(np.int16(rle[i + 1]))
    return 0


def planes_of(oracle, y, cr, cb):
    """jo_decode_tile of the tile whose only nonzero coefficients are the DCs."""
    coef = np.zeros(128, np.int16)
    coef[list(DC_AT)] = (y, cr, cb)
    return X.decode_tile(oracle, coef)


@functools.lru_cache(maxsize=None)
def sample_luts(oracle):
    """(luma, chroma): the plane's sample for every int16 DC, index dc + 32768 --
    every sample of a DC-only plane is sample 0, which is asserted here for
    every DC on all three planes.  Shared: read, do not change."""
    luma = np.empty(65536, np.uint8)
    chroma = np.empty(65536, np.uint8)
    for d in range(-32768, 32768):
        y, cr, cb = planes_of(oracle, d, d, d)
        luma[d + 32768] = y[0, 0]
        chroma[d + 32768] = cr[0, 0]
        assert (y == y[0, 0]).all() and (cr == cr[0, 0]).all() and (cb == cr[0, 0]).all(), d
    luma.setflags(write=False)
    chroma.setflags(write=False)
    return luma, chroma


def _trunc(k, d):
    return np.trunc(k * d.astype(np.float64)).astype(np.int64)     # (int)(k * d), fp64


def pixels(oracle, dc):
    """RGBA [n, 4] of tiles with the DC terms dc [n, 3] = (Y, Cr, Cb)."""
    dc = np.asarray(dc, np.int64).reshape(-1, 3)
    luma, chroma = sample_luts(oracle)
    y = luma[dc[:, 0] + 32768].astype(np.int64)
    cr = chroma[dc[:, 1] + 32768].astype(np.int64) - 128
    cb = chroma[dc[:, 2] + 32768].astype(np.int64) - 128
    out = np.full((dc.shape[0], 4), 255, np.uint8)
    out[:, 0] = np.clip(y + _trunc(1.402, cr), 0, 255)
    out[:, 1] = np.clip(y - _trunc(0.344136, cb) - _trunc(0.714136, cr), 0, 255)
    out[:, 2] = np.clip(y + _trunc(1.772, cb), 0, 255)
    return out


def thumbnails(oracle, coef):
    """The thumbnail pixels [ntiles, 4] of coefficients [ntiles, 128]."""
    return pixels(oracle, np.asarray(coef).reshape(-1, 128)[:, DC_AT])


def zero_pixel(oracle):
    """The colour of all-zero coefficients: a malformed tile's, and every
    tile's under a wrong header or index."""
    return pixels(oracle, [[0, 0, 0]])[0]


def result_words(implied, in_len, header_ok, malformed=()):
    """[0] and [1] of d_result: the implied length; ~0, or 0 on a wrong header
    or length, or 1 + the first malformed tile of the range."""
    if not header_ok or implied != in_len:
        return [implied, 0]
    return [implied, 1 + min(malformed) if len(malformed) else OK]
