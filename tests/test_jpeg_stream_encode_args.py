"""jpegr_stream_encode_device (include/jpegr.h) rejects bad arguments before
any HIP call, and jpegr_stream_encode_scratch_bytes is host arithmetic, so this
runs without a GPU (test_jpr_stream_args.py, for the direct encode)."""
import ctypes

import pytest

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1
JPR1, JPT1 = 1, 2

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
NAMES = ("d_coef", "w", "h", "nimg", "format", "d_out", "cap", "d_out_len", "d_scratch",
         "d_result", "stream")
# one bad argument per call makes it fail; the others are these
GOOD = [P, 40, 24, 3, JPR1, P, 4096, P, P, P, None]      # 3 images of 5 x 3 tiles


def _call(**kw):
    args = list(GOOD)
    for k, v in kw.items():
        args[NAMES.index(k)] = v
    return _lib.lib().jpegr_stream_encode_device(*args)


def test_symbols_exist():
    L = _lib.lib()
    assert hasattr(L, "jpegr_stream_encode_device") and hasattr(L, "jpegr_stream_encode_scratch_bytes")


def test_null_pointers():
    for name in ("d_coef", "d_out", "d_out_len", "d_scratch", "d_result"):
        for fmt in (JPR1, JPT1):
            assert _call(**{name: None}, format=fmt) == JPEGR_ERR_ARG, name


def test_bad_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1}):
        assert _call(**kw) == JPEGR_ERR_ARG, kw
    assert _call(w=1 << 30, h=1 << 30, nimg=1) == JPEGR_ERR_ARG      # more than 2^32 tiles
    assert _call(w=1 << 19, h=1 << 19, nimg=2) == JPEGR_ERR_ARG      # 2^32 per image, two images


def test_misaligned_buffers():
    assert _call(d_coef=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG       # 8-B, not 16-B aligned
    assert _call(d_coef=ctypes.c_void_p(4098)) == JPEGR_ERR_ARG
    assert _call(d_out=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG
    assert _call(d_out_len=ctypes.c_void_p(4100)) == JPEGR_ERR_ARG
    assert _call(d_scratch=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG
    assert _call(d_result=ctypes.c_void_p(4100)) == JPEGR_ERR_ARG


def test_unknown_format():
    for fmt in (0, 3, -1):
        assert _call(format=fmt) == JPEGR_ERR_ARG, fmt


TILES = (1, 64, 4160, 129600, 128 * 129600)


def _bound(nt):
    return 16 + nt * (2 + 1036)                          # jpegr_pack_bound of nt tiles


@pytest.mark.parametrize("nt", TILES)
def test_scratch_bound(nt):
    """The point of the call: the scratch is the stream's capacity and a
    small per-tile term, with nothing the size of a slot (1,292 B) per tile."""
    fn = _lib.lib().jpegr_stream_encode_scratch_bytes
    for cap in (16, _bound(nt) // 4, _bound(nt)):
        got = int(fn(nt, cap))
        assert 0 < got <= cap + 128 * nt + 4096, (nt, cap, got)


def test_scratch_is_monotone():
    fn = _lib.lib().jpegr_stream_encode_scratch_bytes
    caps = [0, 16, 17, 4096, 1 << 20, _bound(4160) // 4, _bound(4160), _bound(129600), 1 << 40]
    tiles = [1, 2, 63, 64, 65, 4096, 4097, 4160, 129600, 128 * 129600]
    for nt in tiles:
        sizes = [int(fn(nt, cap)) for cap in sorted(caps)]
        assert sizes == sorted(sizes), nt
    for cap in caps:
        sizes = [int(fn(nt, cap)) for nt in tiles]
        assert sizes == sorted(sizes), cap


def test_binding_matches_the_header():
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig["jpegr_stream_encode_device"][0] is ctypes.c_int
    assert len(sig["jpegr_stream_encode_device"][1]) == 11
    assert sig["jpegr_stream_encode_scratch_bytes"][0] is ctypes.c_size_t
    assert len(sig["jpegr_stream_encode_scratch_bytes"][1]) == 2
