"""jpegr_dataset_crop_tensor_device and jpegr_dataset_crop_resize_device
(include/jpegr.h) reject bad arguments before any HIP call, so this runs without
a GPU (test_jpeg_crop_resize_args.py, for the calls over many streams), and
their scratch sizes: 0 on a bad argument, monotone in nrects, never below the
single-stream calls'.  What needs a stream's dimensions is judged on the device
(test_gpu_jpeg_dataset.py): a max_w wider than some stream is no argument
error here."""
import ctypes
import math

import pytest

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
TENSOR = ("d_streams", "nstreams", "d_rects", "nrects", "d_flip", "max_w", "max_h", "dtype", "layout",
          "scale3", "bias3", "d_out", "out_cap", "d_scratch", "d_result", "stream")
RESIZE = TENSOR[:7] + ("out_w", "out_h", "filter") + TENSOR[7:]
CALLS = {"jpegr_dataset_crop_tensor_device": TENSOR, "jpegr_dataset_crop_resize_device": RESIZE}


def floats(*v):
    return (ctypes.c_float * 3)(*v)


def good(names):
    vals = {"d_streams": P, "nstreams": 4, "d_rects": P, "nrects": 7, "d_flip": P, "max_w": 16, "max_h": 9,
            "out_w": 5, "out_h": 7, "filter": 1, "dtype": 1, "layout": 0, "scale3": floats(1, 1, 1),
            "bias3": floats(0, 0, 0), "d_out": P, "out_cap": 1 << 20, "d_scratch": P, "d_result": P,
            "stream": None}
    return [vals[n] for n in names]


def call(name, **kw):
    names = CALLS[name]
    args = good(names)
    for k, v in kw.items():
        args[names.index(k)] = v
    return getattr(_lib.lib(), name)(*args)


both = pytest.mark.parametrize("name", sorted(CALLS))


@both
def test_null_pointers(name):
    for arg in ("d_streams", "d_rects", "d_out", "d_scratch", "d_result"):
        assert call(name, **{arg: None}) == JPEGR_ERR_ARG, arg


@both
def test_the_table(name):
    assert call(name, nstreams=0) == JPEGR_ERR_ARG
    assert call(name, nstreams=(1 << 31) + 1) == JPEGR_ERR_ARG
    assert call(name, nstreams=1 << 63) == JPEGR_ERR_ARG
    for a in (4097, 4098, 4100):
        assert call(name, d_streams=ctypes.c_void_p(a)) == JPEGR_ERR_ARG, a


@both
def test_counts_and_maxima(name):
    assert call(name, nrects=0) == JPEGR_ERR_ARG
    for kw in ({"max_w": 0}, {"max_h": 0}, {"max_w": -1}, {"max_h": -1}):
        assert call(name, **kw) == JPEGR_ERR_ARG, kw


@both
def test_launch_bound(name):
    """nrects * K may not exceed 2^28 items (2^22 workgroups of 64)."""
    k = _lib.lib().jpegr_crop_items(16, 9)
    assert k == 9
    assert call(name, nrects=(1 << 28) // k + 1) == JPEGR_ERR_ARG
    assert call(name, nrects=1 << 63) == JPEGR_ERR_ARG
    assert call(name, max_w=8192, max_h=8192, nrects=256) == JPEGR_ERR_ARG


@both
def test_misaligned_buffers(name):
    for arg in ("d_rects", "d_result"):
        assert call(name, **{arg: ctypes.c_void_p(4100)}) == JPEGR_ERR_ARG, arg
    assert call(name, d_scratch=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG        # 8-B, not 16-B aligned
    for a in (4097, 4098, 4100, 4104):                                         # 8-B is not enough
        assert call(name, d_out=ctypes.c_void_p(a)) == JPEGR_ERR_ARG, a


@both
def test_dtype_and_layout(name):
    for d in (-1, 4):
        assert call(name, dtype=d) == JPEGR_ERR_ARG, d
    for lay in (-1, 2):
        assert call(name, layout=lay) == JPEGR_ERR_ARG, lay


def test_filter_and_output_size():
    name = "jpegr_dataset_crop_resize_device"
    for f in (-1, 2, 1 << 20):
        assert call(name, filter=f) == JPEGR_ERR_ARG, f
    for kw in ({"out_w": 0}, {"out_h": 0}, {"out_w": -1}, {"out_h": -224}):
        assert call(name, **kw) == JPEGR_ERR_ARG, kw
    for ow, oh in ((26755, 26755), (46341, 46341), (0x7FFFFFFF, 0x7FFFFFFF), (0x7FFFFFFF, 1), (1, 715827883)):
        assert call(name, out_w=ow, out_h=oh) == JPEGR_ERR_ARG, (ow, oh)


@both
def test_scale_and_bias_must_be_finite(name):
    for arg in ("scale3", "bias3"):
        for bad in (math.nan, math.inf, -math.inf):
            for c in range(3):
                v = [0.5, 0.25, 2.0]
                v[c] = bad
                assert call(name, **{arg: floats(*v)}) == JPEGR_ERR_ARG, (arg, bad, c)
    assert call(name, scale3=None, bias3=floats(0, math.nan, 0)) == JPEGR_ERR_ARG
    assert call(name, scale3=floats(math.inf, 1, 1), bias3=None) == JPEGR_ERR_ARG


def test_scratch_bytes():
    """0 on a bad argument; the single-stream scratch and a u64 a rectangle,
    whole 16-B chunks; monotone in nrects."""
    lib = _lib.lib()
    size, single = lib.jpegr_dataset_crop_scratch_bytes, lib.jpegr_crop_scratch_bytes
    for args in ((0, 16, 9), (7, 0, 9), (7, 16, 0), (7, -1, 9), (7, 16, -3), (1 << 62, 16, 9),
                 ((1 << 64) - 1, 1, 1)):
        assert size(*args) == 0, args
    last = 0
    for n in (1, 2, 3, 7, 8, 9, 255, 256, 257, 1 << 20):
        b = size(n, 16, 9)
        assert b % 16 == 0 and b > last
        assert b == single(n, 16, 9) + (8 * n + 15) // 16 * 16
        last = b
    assert size(7, 17, 9) >= size(7, 16, 9) <= size(7, 16, 10)


def test_resize_scratch_bytes():
    lib = _lib.lib()
    size, single = lib.jpegr_dataset_crop_resize_scratch_bytes, lib.jpegr_crop_resize_scratch_bytes
    for args in ((0, 16, 9, 5, 7), (7, 0, 9, 5, 7), (7, 16, 0, 5, 7), (7, -1, 9, 5, 7), (7, 16, -3, 5, 7),
                 (7, 16, 9, 0, 7), (7, 16, 9, 5, 0), (7, 16, 9, -5, 7), (7, 16, 9, 5, -7),
                 (1 << 62, 16, 9, 5, 7), ((1 << 64) - 1, 1, 1, 1, 1),
                 (1 << 40, 0x7FFFFFFF, 0x7FFFFFFF, 1, 1)):
        assert size(*args) == 0, args
    last = 0
    for n in (1, 2, 3, 7, 8, 9, 255, 256, 257, 1 << 20):
        b = size(n, 16, 9, 5, 7)
        assert b % 16 == 0 and b > last
        assert b == single(n, 16, 9, 5, 7) + (8 * n + 15) // 16 * 16
        last = b
    assert size(7, 16, 9, 224, 224) > size(7, 16, 9, 5, 7)
    assert size(256, 1920, 1080, 224, 224) < 1 << 33


def test_binding_matches_the_header():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    fp = ctypes.POINTER(ctypes.c_float)
    for name, names in CALLS.items():
        res, args = sigs[name]
        assert res is ctypes.c_int and len(args) == len(names)
        assert args[names.index("scale3")] is fp and args[names.index("bias3")] is fp
        assert args[names.index("nstreams")] is ctypes.c_size_t
        for n in ("d_streams", "d_rects", "d_flip", "d_out", "d_scratch", "d_result", "stream"):
            assert args[names.index(n)] is ctypes.c_void_p, n
        for n in names[names.index("max_w"):names.index("scale3")]:
            assert args[names.index(n)] is ctypes.c_int, n
    res, args = sigs["jpegr_dataset_crop_scratch_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_size_t] + [ctypes.c_int] * 2
    res, args = sigs["jpegr_dataset_crop_resize_scratch_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_size_t] + [ctypes.c_int] * 4


def test_the_descriptor_is_48_bytes():
    """Four 8-B fields and four u32: the layout jpeg.stream_table writes."""
    import numpy as np
    from lz4jpeg import jpeg
    t = jpeg.stream_table([(0x1000, 77, 0x2000, 5, 40, 24, 3)])
    assert t.dtype == np.uint64 and t.shape == (1, 6) and t.nbytes == 48 == jpeg.STREAM_DESC_BYTES
    want = b"".join(int(v).to_bytes(8, "little") for v in (0x1000, 77, 0x2000, 5))
    want += b"".join(int(v).to_bytes(4, "little") for v in (40, 24, 3, 0))
    assert t.tobytes() == want
