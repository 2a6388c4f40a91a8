"""jpegr_select_device (include/jpegr.h) rejects bad arguments before any HIP
call, and jpegr_select_scratch_bytes is host arithmetic, so this runs without a
GPU (test_jpeg_crop_args.py, for the stream-editing call)."""
import ctypes

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
NAMES = ("d_in", "in_len", "w", "h", "nimg", "d_tile_offsets", "d_items", "nitems", "out_w", "out_h",
         "format", "d_out", "cap", "d_out_len", "d_scratch", "d_result", "stream")
GOOD = [P, 4096, 40, 24, 3, P, P, 7, 16, 9, 0, P, 1 << 20, P, P, P, None]    # 3 images of 5 x 3 tiles


def _select(**kw):
    args = list(GOOD)
    for k, v in kw.items():
        args[NAMES.index(k)] = v
    return _lib.lib().jpegr_select_device(*args)


def test_null_pointers():
    for name in ("d_in", "d_tile_offsets", "d_items", "d_out", "d_out_len", "d_scratch", "d_result"):
        assert _select(**{name: None}) == JPEGR_ERR_ARG, name


def test_bad_source_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1}):
        assert _select(**kw) == JPEGR_ERR_ARG, kw
    assert _select(w=1 << 30, h=1 << 30, nimg=1) == JPEGR_ERR_ARG            # more than 2^32 tiles


def test_items_and_window():
    assert _select(nitems=0) == JPEGR_ERR_ARG
    assert _select(nitems=1 << 31) == JPEGR_ERR_ARG                           # past the header's count
    assert _select(nitems=1 << 63) == JPEGR_ERR_ARG
    for kw in ({"out_w": 0}, {"out_h": 0}, {"out_w": -1}, {"out_h": -8},
               {"out_w": 41}, {"out_h": 25}):                                 # past the image
        assert _select(**kw) == JPEGR_ERR_ARG, kw
    # 2^16 x 2^16 tiles an item: 2 items are 2^33 output tiles
    assert _select(w=1 << 19, h=1 << 19, nimg=1, out_w=1 << 19, out_h=1 << 19, nitems=2) == JPEGR_ERR_ARG
    assert _select(in_len=15) == JPEGR_ERR_ARG
    assert _select(in_len=0) == JPEGR_ERR_ARG


def test_format():
    for f in (3, -1, 4, 1 << 20):
        assert _select(format=f) == JPEGR_ERR_ARG, f


def test_misaligned_buffers():
    for name in ("d_items", "d_tile_offsets", "d_result", "d_out_len"):
        assert _select(**{name: ctypes.c_void_p(4100)}) == JPEGR_ERR_ARG, name
    for name in ("d_scratch", "d_out"):
        assert _select(**{name: ctypes.c_void_p(4104)}) == JPEGR_ERR_ARG, name   # 8-B, not 16-B aligned


def test_scratch_bytes():
    L = _lib.lib()
    # the index scan's scratch over the output's tiles
    assert L.jpegr_select_scratch_bytes(7, 16, 9) == L.jpegr_pack_scratch_bytes(7 * 2 * 2)
    assert L.jpegr_select_scratch_bytes(256, 224, 224) == L.jpegr_pack_scratch_bytes(256 * 28 * 28)
    for args in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, -1, 8), (1 << 31, 8, 8), (1 << 63, 8, 8),
                 (2, 1 << 19, 1 << 19)):
        assert L.jpegr_select_scratch_bytes(*args) == 0, args
    prev = 0
    for n in (1, 2, 3, 64, 65, 1000, 5000):
        cur = L.jpegr_select_scratch_bytes(n, 64, 48)
        assert cur > prev
        prev = cur


def test_bindings_match_the_header():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sigs["jpegr_select_device"][0] is ctypes.c_int and len(sigs["jpegr_select_device"][1]) == 17
    assert sigs["jpegr_select_scratch_bytes"][0] is ctypes.c_size_t
    assert len(sigs["jpegr_select_scratch_bytes"][1]) == 3
