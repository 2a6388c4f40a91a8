"""jpegr_thumb_device (include/jpegr.h) rejects bad arguments before any HIP
call, and jpegr_thumb_scratch_bytes is host arithmetic, so this runs without a
GPU (test_jpeg_crop_args.py, for the thumbnail call)."""
import ctypes

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
NAMES = ("d_in", "in_len", "w", "h", "nimg", "d_tile_offsets", "image0", "nimage", "d_rgba_out",
         "d_dc_out", "d_scratch", "d_result", "stream")
GOOD = [P, 4096, 40, 24, 3, P, 1, 2, P, P, P, P, None]        # 3 images of 5 x 3 tiles


def _thumb(**kw):
    args = list(GOOD)
    for k, v in kw.items():
        args[NAMES.index(k)] = v
    return _lib.lib().jpegr_thumb_device(*args)


def test_null_pointers():
    for name in ("d_in", "d_result"):
        assert _thumb(**{name: None}) == JPEGR_ERR_ARG, name
    assert _thumb(d_rgba_out=None, d_dc_out=None) == JPEGR_ERR_ARG
    assert _thumb(d_tile_offsets=None, d_scratch=None) == JPEGR_ERR_ARG
    # (one output alone, offsets without a scratch and a scratch without offsets
    # are good arguments: the GPU tests make those calls)


def test_bad_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1}):
        assert _thumb(**kw) == JPEGR_ERR_ARG, kw
    assert _thumb(w=1 << 30, h=1 << 30, nimg=1, image0=0, nimage=1) == JPEGR_ERR_ARG   # > 2^32 tiles


def test_image_range():
    assert _thumb(nimage=0) == JPEGR_ERR_ARG
    for image0, nimage in ((0, 4), (1, 3), (3, 1), (4, 1), (2, 2), (1 << 63, 1 << 63),
                           ((1 << 64) - 1, 2), (1, (1 << 64) - 1)):
        assert _thumb(image0=image0, nimage=nimage) == JPEGR_ERR_ARG, (image0, nimage)


def test_short_stream():
    assert _thumb(in_len=15) == JPEGR_ERR_ARG
    assert _thumb(in_len=0) == JPEGR_ERR_ARG


def test_misaligned_buffers():
    for name in ("d_tile_offsets", "d_result", "d_dc_out"):
        assert _thumb(**{name: ctypes.c_void_p(4100)}) == JPEGR_ERR_ARG, name
    assert _thumb(d_scratch=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG       # 8-B, not 16-B aligned
    assert _thumb(d_rgba_out=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG
    assert _thumb(d_rgba_out=ctypes.c_void_p(4100), d_dc_out=None) == JPEGR_ERR_ARG


def test_scratch_bytes():
    L = _lib.lib()
    for nt in (1, 63, 64, 65, 4095, 4096, 4097, 1 << 20):
        assert L.jpegr_thumb_scratch_bytes(nt) == L.jpegr_pack_scratch_bytes(nt) > 0


def test_bindings_match_the_header():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sigs["jpegr_thumb_device"][0] is ctypes.c_int and len(sigs["jpegr_thumb_device"][1]) == 13
    assert sigs["jpegr_thumb_scratch_bytes"][0] is ctypes.c_size_t
    assert len(sigs["jpegr_thumb_scratch_bytes"][1]) == 1
