"""jpegr_crop_tensor_device (include/jpegr.h) rejects bad arguments before any
HIP call, so this runs without a GPU (test_jpeg_crop_args.py, for the tensor
form of the call).  A NULL d_flip, scale3 or bias3 is no error; that they get
past this check is asserted where a device is (test_gpu_jpeg_crop_tensor.py)."""
import ctypes
import math

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
NAMES = ("d_in", "in_len", "w", "h", "nimg", "d_tile_offsets", "d_rects", "nrects", "d_flip", "max_w",
         "max_h", "dtype", "layout", "scale3", "bias3", "d_out", "out_cap", "d_scratch", "d_result",
         "stream")


def floats(*v):
    return (ctypes.c_float * 3)(*v)


def good():
    return [P, 4096, 40, 24, 3, P, P, 7, P, 16, 9, 1, 0, floats(1, 1, 1), floats(0, 0, 0), P, 1 << 20, P,
            P, None]


def _crop(**kw):
    args = good()
    for k, v in kw.items():
        args[NAMES.index(k)] = v
    return _lib.lib().jpegr_crop_tensor_device(*args)


def test_null_pointers():
    for name in ("d_in", "d_tile_offsets", "d_rects", "d_out", "d_scratch", "d_result"):
        assert _crop(**{name: None}) == JPEGR_ERR_ARG, name


def test_bad_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1}):
        assert _crop(**kw) == JPEGR_ERR_ARG, kw
    assert _crop(w=1 << 30, h=1 << 30, nimg=1) == JPEGR_ERR_ARG           # more than 2^32 tiles


def test_counts_and_maxima():
    assert _crop(nrects=0) == JPEGR_ERR_ARG
    for kw in ({"max_w": 0}, {"max_h": 0}, {"max_w": -1}, {"max_h": -1},
               {"max_w": 41}, {"max_h": 25}):                              # past the image
        assert _crop(**kw) == JPEGR_ERR_ARG, kw
    assert _crop(in_len=15) == JPEGR_ERR_ARG
    assert _crop(in_len=0) == JPEGR_ERR_ARG


def test_launch_bound():
    """nrects * K may not exceed 2^28 items (2^22 workgroups of 64)."""
    k = _lib.lib().jpegr_crop_items(16, 9)
    assert k == 9
    assert _crop(nrects=(1 << 28) // k + 1) == JPEGR_ERR_ARG
    assert _crop(nrects=1 << 63) == JPEGR_ERR_ARG
    assert _crop(w=8192, h=8192, nimg=1, max_w=8192, max_h=8192, nrects=256) == JPEGR_ERR_ARG


def test_misaligned_buffers():
    for name in ("d_rects", "d_tile_offsets", "d_result"):
        assert _crop(**{name: ctypes.c_void_p(4100)}) == JPEGR_ERR_ARG, name
    assert _crop(d_scratch=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG        # 8-B, not 16-B aligned
    for a in (4097, 4098, 4100, 4104):                                    # 8-B is not enough
        assert _crop(d_out=ctypes.c_void_p(a)) == JPEGR_ERR_ARG, a


def test_dtype_and_layout():
    for d in (-1, 4):
        assert _crop(dtype=d) == JPEGR_ERR_ARG, d
    for lay in (-1, 2):
        assert _crop(layout=lay) == JPEGR_ERR_ARG, lay


def test_scale_and_bias_must_be_finite():
    for name in ("scale3", "bias3"):
        for bad in (math.nan, math.inf, -math.inf):
            for c in range(3):
                v = [0.5, 0.25, 2.0]
                v[c] = bad
                assert _crop(**{name: floats(*v)}) == JPEGR_ERR_ARG, (name, bad, c)
    # with the other one NULL too
    assert _crop(scale3=None, bias3=floats(0, math.nan, 0)) == JPEGR_ERR_ARG
    assert _crop(scale3=floats(math.inf, 1, 1), bias3=None) == JPEGR_ERR_ARG


def test_binding_matches_the_header():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    res, args = sigs["jpegr_crop_tensor_device"]
    assert res is ctypes.c_int and len(args) == 20 == len(NAMES)
    fp = ctypes.POINTER(ctypes.c_float)
    assert args[NAMES.index("scale3")] is fp and args[NAMES.index("bias3")] is fp
    assert args[NAMES.index("d_flip")] is ctypes.c_void_p
