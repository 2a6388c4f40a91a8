"""jpegr_stream_decode_device (include/jpegr.h) rejects bad arguments before
any HIP call, so this runs without a GPU (test_jpr_format.py's pack and unpack
argument tests, for the direct decode)."""
import ctypes

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
# d_in, in_len, w, h, nimg, tile0, ntile, d_coef, d_scratch, d_result, stream
GOOD = [P, 4096, 40, 24, 3, 0, 45, P, P, P, None]        # 3 images of 5 x 3 tiles


def _call(**kw):
    names = ("d_in", "in_len", "w", "h", "nimg", "tile0", "ntile", "d_coef", "d_scratch",
             "d_result", "stream")
    args = list(GOOD)
    for k, v in kw.items():
        args[names.index(k)] = v
    return _lib.lib().jpegr_stream_decode_device(*args)


def test_null_pointers():
    for name in ("d_in", "d_coef", "d_scratch", "d_result"):
        assert _call(**{name: None}) == JPEGR_ERR_ARG, name


def test_bad_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1}):
        assert _call(**kw) == JPEGR_ERR_ARG, kw
    assert _call(w=1 << 30, h=1 << 30, nimg=1, ntile=1) == JPEGR_ERR_ARG   # more than 2^32 tiles


def test_tile_range():
    assert _call(ntile=0) == JPEGR_ERR_ARG
    assert _call(tile0=0, ntile=46) == JPEGR_ERR_ARG                  # tile0 + ntile = ntiles + 1
    assert _call(tile0=1, ntile=45) == JPEGR_ERR_ARG
    assert _call(tile0=45, ntile=1) == JPEGR_ERR_ARG
    assert _call(tile0=46, ntile=1) == JPEGR_ERR_ARG
    assert _call(tile0=(1 << 64) - 1, ntile=2) == JPEGR_ERR_ARG       # a sum that wraps
    assert _call(tile0=2, ntile=(1 << 64) - 1) == JPEGR_ERR_ARG


def test_misaligned_buffers():
    assert _call(d_coef=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG       # 8-B, not 16-B aligned
    assert _call(d_coef=ctypes.c_void_p(4098)) == JPEGR_ERR_ARG
    assert _call(d_result=ctypes.c_void_p(4100)) == JPEGR_ERR_ARG
    assert _call(d_scratch=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG


def test_binding_matches_the_header():
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["jpegr_stream_decode_device"]
    assert sig[0] is ctypes.c_int and len(sig[1]) == 11
