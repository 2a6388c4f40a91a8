"""jpegr_crop_resize_device (include/jpegr.h) rejects bad arguments before any
HIP call, so this runs without a GPU (test_jpeg_crop_tensor_args.py, for the
resampling form of the call), and jpegr_crop_resize_scratch_bytes: 0 on a bad
argument, monotone in nrects.  A NULL d_flip, scale3 or bias3 is no error; that
they get past this check is asserted where a device is
(test_gpu_jpeg_crop_resize.py)."""
import ctypes
import math

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
NAMES = ("d_in", "in_len", "w", "h", "nimg", "d_tile_offsets", "d_rects", "nrects", "d_flip", "max_w",
         "max_h", "out_w", "out_h", "filter", "dtype", "layout", "scale3", "bias3", "d_out", "out_cap",
         "d_scratch", "d_result", "stream")


def floats(*v):
    return (ctypes.c_float * 3)(*v)


def good():
    return [P, 4096, 40, 24, 3, P, P, 7, P, 16, 9, 5, 7, 1, 1, 0, floats(1, 1, 1), floats(0, 0, 0), P,
            1 << 20, P, P, None]


def _crop(**kw):
    args = good()
    for k, v in kw.items():
        args[NAMES.index(k)] = v
    return _lib.lib().jpegr_crop_resize_device(*args)


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


def test_dtype_layout_and_filter():
    for d in (-1, 4):
        assert _crop(dtype=d) == JPEGR_ERR_ARG, d
    for lay in (-1, 2):
        assert _crop(layout=lay) == JPEGR_ERR_ARG, lay
    for f in (-1, 2, 1 << 20):
        assert _crop(filter=f) == JPEGR_ERR_ARG, f


def test_output_size():
    for kw in ({"out_w": 0}, {"out_h": 0}, {"out_w": -1}, {"out_h": -224}):
        assert _crop(**kw) == JPEGR_ERR_ARG, kw
    # 3 out_w out_h past INT_MAX: 26755^2 * 3 = 2^31 + 6,427 and 46341^2 > 2^31
    for ow, oh in ((26755, 26755), (46341, 46341), (0x7FFFFFFF, 0x7FFFFFFF), (0x7FFFFFFF, 1), (1, 715827883)):
        assert _crop(out_w=ow, out_h=oh) == JPEGR_ERR_ARG, (ow, oh)


def test_scale_and_bias_must_be_finite():
    for name in ("scale3", "bias3"):
        for bad in (math.nan, math.inf, -math.inf):
            for c in range(3):
                v = [0.5, 0.25, 2.0]
                v[c] = bad
                assert _crop(**{name: floats(*v)}) == JPEGR_ERR_ARG, (name, bad, c)
    assert _crop(scale3=None, bias3=floats(0, math.nan, 0)) == JPEGR_ERR_ARG
    assert _crop(scale3=floats(math.inf, 1, 1), bias3=None) == JPEGR_ERR_ARG


def test_scratch_bytes():
    """0 on a bad argument; never below jpegr_crop_scratch_bytes plus the
    pixels; a multiple of 16; monotone in nrects."""
    size = _lib.lib().jpegr_crop_resize_scratch_bytes
    crop = _lib.lib().jpegr_crop_scratch_bytes
    for args in ((0, 16, 9, 5, 7), (7, 0, 9, 5, 7), (7, 16, 0, 5, 7), (7, -1, 9, 5, 7), (7, 16, -3, 5, 7),
                 (7, 16, 9, 0, 7), (7, 16, 9, 5, 0), (7, 16, 9, -5, 7), (7, 16, 9, 5, -7),
                 (1 << 62, 16, 9, 5, 7), ((1 << 64) - 1, 1, 1, 1, 1),
                 (1 << 40, 0x7FFFFFFF, 0x7FFFFFFF, 1, 1)):
        assert size(*args) == 0, args
    last = 0
    for n in (1, 2, 3, 7, 8, 9, 255, 256, 257, 1 << 20):
        b = size(n, 16, 9, 5, 7)
        assert b % 16 == 0 and b > last
        assert b >= crop(n, 16, 9) + n * (48 + 4 * 16 * 9 + 8 * (5 + 7))
        last = b
    # and in the sizes: a larger source or output never needs less
    assert size(7, 17, 9, 5, 7) >= size(7, 16, 9, 5, 7) <= size(7, 16, 10, 5, 7)
    assert size(7, 16, 9, 224, 224) > size(7, 16, 9, 5, 7)
    assert size(256, 1920, 1080, 224, 224) < 1 << 33


def test_binding_matches_the_header():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    res, args = sigs["jpegr_crop_resize_device"]
    assert res is ctypes.c_int and len(args) == 23 == len(NAMES)
    fp = ctypes.POINTER(ctypes.c_float)
    assert args[NAMES.index("scale3")] is fp and args[NAMES.index("bias3")] is fp
    assert args[NAMES.index("d_flip")] is ctypes.c_void_p
    for name in ("out_w", "out_h", "filter", "dtype", "layout"):
        assert args[NAMES.index(name)] is ctypes.c_int, name
    res, args = sigs["jpegr_crop_resize_scratch_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_size_t] + [ctypes.c_int] * 4
