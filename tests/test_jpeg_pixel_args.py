"""The seven device calls of the JPEG pixel stage (include/jpegr.h:
jpegr_encode_device, jpegr_dct_raw_device, jpegr_reconstruct_device,
jpegr_planes_device, jpegr_dct_blocks_device, jpegr_quantize_device,
jpegr_permute_device) reject NULL pointers, bad dimensions and misaligned
pointers with JPEGR_ERR_ARG before any HIP call, so this runs without a GPU: a
call that got as far as HIP would answer JPEGR_ERR_HIP here
(test_jpeg_crop_args.py, for the pixel stage).  Each bad argument list differs
from the call's good one in one argument; a good list is never launched."""
import ctypes

import pytest

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1
A = 4096                                 # never dereferenced: every case fails first
P = ctypes.c_void_p(A)

# call -> (argument names, a good argument list)
CALLS = {
    "jpegr_encode_device": (("d_rgba", "w", "h", "nimg", "d_out_i16", "stream"),
                            [P, 40, 24, 3, P, None]),
    "jpegr_dct_raw_device": (("d_rgba", "w", "h", "nimg", "d_out_f64", "stream"),
                             [P, 40, 24, 3, P, None]),
    "jpegr_reconstruct_device": (("d_coef", "d_rgba_orig", "w", "h", "nimg", "d_rgba_out", "stream"),
                                 [P, P, 40, 24, 3, P, None]),
    "jpegr_planes_device": (("d_rgba", "w", "h", "d_y", "d_cr", "d_cb", "stream"),
                            [P, 40, 24, P, P, P, None]),
    "jpegr_dct_blocks_device": (("d_blocks", "width", "height", "nblocks", "d_out_f64", "stream"),
                                [P, 8, 8, 5, P, None]),
    "jpegr_quantize_device": (("d_coef_f64", "d_table_f64", "size", "n", "stream"),
                              [P, P, 64, 640, None]),
    "jpegr_permute_device": (("d_in_f64", "d_out_f64", "d_perm_i32", "size", "n", "stream"),
                             [P, P, P, 64, 640, None]),
}

# call -> the pointers that may not be NULL (d_rgba_orig may)
REQUIRED = {
    "jpegr_encode_device": ("d_rgba", "d_out_i16"),
    "jpegr_dct_raw_device": ("d_rgba", "d_out_f64"),
    "jpegr_reconstruct_device": ("d_coef", "d_rgba_out"),
    "jpegr_planes_device": ("d_rgba", "d_y", "d_cr", "d_cb"),
    "jpegr_dct_blocks_device": ("d_blocks", "d_out_f64"),
    "jpegr_quantize_device": ("d_coef_f64", "d_table_f64"),
    "jpegr_permute_device": ("d_in_f64", "d_out_f64", "d_perm_i32"),
}

# call -> {pointer: required alignment in bytes} (the table of include/jpegr.h;
# the planes and d_blocks take any alignment and are not listed)
ALIGN = {
    "jpegr_encode_device": {"d_rgba": 4, "d_out_i16": 16},
    "jpegr_dct_raw_device": {"d_rgba": 4, "d_out_f64": 8},
    "jpegr_reconstruct_device": {"d_coef": 16, "d_rgba_orig": 4, "d_rgba_out": 4},
    "jpegr_planes_device": {"d_rgba": 4},
    "jpegr_dct_blocks_device": {"d_out_f64": 8},
    "jpegr_quantize_device": {"d_coef_f64": 8, "d_table_f64": 8},
    "jpegr_permute_device": {"d_in_f64": 8, "d_out_f64": 8, "d_perm_i32": 4},
}

IMAGE_CALLS = ("jpegr_encode_device", "jpegr_dct_raw_device", "jpegr_reconstruct_device")
I31 = 0x7FFFFFFF


def _call(name, **kw):
    names, good = CALLS[name]
    args = list(good)
    assert set(kw) <= set(names) and kw, kw
    for k, v in kw.items():
        args[names.index(k)] = v
    return getattr(_lib.lib(), name)(*args)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_pointers(name):
    for ptr in REQUIRED[name]:
        assert _call(name, **{ptr: None}) == JPEGR_ERR_ARG, ptr


@pytest.mark.parametrize("name", IMAGE_CALLS)
def test_image_dimensions(name):
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1},
               {"nimg": 65536}, {"nimg": I31}):
        assert _call(name, **kw) == JPEGR_ERR_ARG, kw
    # 2^28 tile rows of 2^23 strips: more than 2^31 - 1 workgroups in x
    assert _call(name, w=I31, h=I31) == JPEGR_ERR_ARG
    # 2^28 tile rows of 8 strips = 2^31 workgroups: one past the limit
    assert _call(name, w=8 * 32 * 8, h=I31) == JPEGR_ERR_ARG


def test_planes_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"w": -8}, {"h": -1}):
        assert _call("jpegr_planes_device", **kw) == JPEGR_ERR_ARG, kw
    assert _call("jpegr_planes_device", w=I31, h=I31) == JPEGR_ERR_ARG     # 2^31 workgroups and more


def test_dct_blocks_dimensions():
    for kw in ({"width": 3}, {"width": 5}, {"width": 16}, {"width": 0}, {"width": -8},
               {"height": 7}, {"height": 9}, {"height": 4}, {"height": 0}, {"height": -8},
               {"nblocks": 0}, {"nblocks": -1}):
        assert _call("jpegr_dct_blocks_device", **kw) == JPEGR_ERR_ARG, kw
    # the chroma block is 8 rows of 4: width 4 is good, and only with height 8
    assert _call("jpegr_dct_blocks_device", width=4, height=4) == JPEGR_ERR_ARG


@pytest.mark.parametrize("name", ("jpegr_quantize_device", "jpegr_permute_device"))
def test_size_and_count(name):
    for kw in ({"size": 0}, {"size": -1}, {"size": -64}, {"n": 0}):
        assert _call(name, **kw) == JPEGR_ERR_ARG, kw
    assert _call(name, n=(1 << 64) - 1) == JPEGR_ERR_ARG                     # 2^31 workgroups and more


@pytest.mark.parametrize("name", sorted(CALLS))
def test_misaligned_pointers(name):
    """Every rule at the smallest offset that breaks it (+1) and at the largest
    one that still keeps the next weaker rule (+8 of 16, +4 of 8, +2 of 4)."""
    for ptr, align in ALIGN[name].items():
        for off in sorted({1, align // 2, align - 1}):
            assert _call(name, **{ptr: ctypes.c_void_p(A + off)}) == JPEGR_ERR_ARG, (ptr, off)


def test_the_tables_cover_every_pointer():
    """Every pointer argument of every call is in REQUIRED or is d_rgba_orig,
    and every aligned one is a pointer of its call."""
    for name, (names, good) in CALLS.items():
        ptrs = {n for n, g in zip(names, good) if g is P}
        assert ptrs - {"d_rgba_orig"} == set(REQUIRED[name]), name
        assert set(ALIGN[name]) <= ptrs, name
        assert A % 16 == 0


def test_coef_count():
    L = _lib.lib()
    assert L.jpegr_coef_count(1, 1) == 128
    assert L.jpegr_coef_count(8, 8) == 128
    assert L.jpegr_coef_count(9, 8) == 256
    assert L.jpegr_coef_count(0, 8) == 0
    assert L.jpegr_coef_count(8, -1) == 0
    assert L.jpegr_coef_count(I31, I31) == (1 << 28) * (1 << 28) * 128      # w + 7 does not wrap


def test_bindings_match_the_header():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for name, (names, _) in CALLS.items():
        assert sigs[name][0] is ctypes.c_int and len(sigs[name][1]) == len(names), name
