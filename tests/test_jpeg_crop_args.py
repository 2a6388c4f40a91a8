"""jpegr_stream_index_device and jpegr_crop_device (include/jpegr.h) reject bad
arguments before any HIP call, and jpegr_crop_items / jpegr_crop_scratch_bytes
are host arithmetic, so this runs without a GPU (test_jpr_stream_args.py, for
the random-access calls)."""
import ctypes

from lz4jpeg import _lib

JPEGR_ERR_ARG = -1

P = ctypes.c_void_p(4096)                # never dereferenced: every case fails first
INDEX_NAMES = ("d_in", "in_len", "w", "h", "nimg", "d_tile_offsets", "d_scratch", "d_result",
               "stream")
INDEX_GOOD = [P, 4096, 40, 24, 3, P, P, P, None]              # 3 images of 5 x 3 tiles
CROP_NAMES = ("d_in", "in_len", "w", "h", "nimg", "d_tile_offsets", "d_rects", "nrects", "max_w",
              "max_h", "d_out", "out_cap", "d_scratch", "d_result", "stream")
CROP_GOOD = [P, 4096, 40, 24, 3, P, P, 7, 16, 9, P, 1 << 20, P, P, None]


def _index(**kw):
    args = list(INDEX_GOOD)
    for k, v in kw.items():
        args[INDEX_NAMES.index(k)] = v
    return _lib.lib().jpegr_stream_index_device(*args)


def _crop(**kw):
    args = list(CROP_GOOD)
    for k, v in kw.items():
        args[CROP_NAMES.index(k)] = v
    return _lib.lib().jpegr_crop_device(*args)


def test_index_null_pointers():
    for name in ("d_in", "d_tile_offsets", "d_scratch", "d_result"):
        assert _index(**{name: None}) == JPEGR_ERR_ARG, name


def test_index_bad_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1}):
        assert _index(**kw) == JPEGR_ERR_ARG, kw
    assert _index(w=1 << 30, h=1 << 30, nimg=1) == JPEGR_ERR_ARG          # more than 2^32 tiles


def test_index_misaligned_buffers():
    assert _index(d_tile_offsets=ctypes.c_void_p(4100)) == JPEGR_ERR_ARG
    assert _index(d_result=ctypes.c_void_p(4100)) == JPEGR_ERR_ARG
    assert _index(d_scratch=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG       # 8-B, not 16-B aligned


def test_crop_null_pointers():
    for name in ("d_in", "d_tile_offsets", "d_rects", "d_out", "d_scratch", "d_result"):
        assert _crop(**{name: None}) == JPEGR_ERR_ARG, name


def test_crop_bad_dimensions():
    for kw in ({"w": 0}, {"h": 0}, {"nimg": 0}, {"w": -8}, {"h": -1}, {"nimg": -1}):
        assert _crop(**kw) == JPEGR_ERR_ARG, kw
    assert _crop(w=1 << 30, h=1 << 30, nimg=1) == JPEGR_ERR_ARG           # more than 2^32 tiles


def test_crop_counts_and_maxima():
    assert _crop(nrects=0) == JPEGR_ERR_ARG
    for kw in ({"max_w": 0}, {"max_h": 0}, {"max_w": -1}, {"max_h": -1},
               {"max_w": 41}, {"max_h": 25}):                              # past the image
        assert _crop(**kw) == JPEGR_ERR_ARG, kw
    assert _crop(in_len=15) == JPEGR_ERR_ARG
    assert _crop(in_len=0) == JPEGR_ERR_ARG


def test_crop_misaligned_buffers():
    for name in ("d_rects", "d_tile_offsets", "d_result"):
        assert _crop(**{name: ctypes.c_void_p(4100)}) == JPEGR_ERR_ARG, name
    assert _crop(d_scratch=ctypes.c_void_p(4104)) == JPEGR_ERR_ARG        # 8-B, not 16-B aligned
    assert _crop(d_out=ctypes.c_void_p(4098)) == JPEGR_ERR_ARG
    assert _crop(d_out=ctypes.c_void_p(4097)) == JPEGR_ERR_ARG


def test_crop_launch_bound():
    """nrects * K may not exceed 2^28 items (2^22 workgroups of 64)."""
    k = _lib.lib().jpegr_crop_items(16, 9)
    assert k == 9
    assert _crop(nrects=(1 << 28) // k + 1) == JPEGR_ERR_ARG
    assert _crop(nrects=1 << 63) == JPEGR_ERR_ARG
    # a whole 8K x 8K image a rectangle: K = 1025^2, so 256 rectangles are too many
    assert _crop(w=8192, h=8192, nimg=1, max_w=8192, max_h=8192, nrects=256) == JPEGR_ERR_ARG


def test_crop_items():
    L = _lib.lib()
    assert L.jpegr_crop_items(1, 1) == 4
    assert L.jpegr_crop_items(8, 8) == 4
    assert L.jpegr_crop_items(9, 8) == 6
    assert L.jpegr_crop_items(224, 224) == 841
    for a, b in ((0, 8), (8, 0), (-1, 8), (8, -1), (0, 0)):
        assert L.jpegr_crop_items(a, b) == 0, (a, b)


def test_crop_scratch_bytes():
    L = _lib.lib()
    # 256 B of coefficients an item and a status word a rectangle, in whole 16-B chunks
    assert L.jpegr_crop_scratch_bytes(1, 8, 8) == 4 * 256 + 16
    assert L.jpegr_crop_scratch_bytes(256, 224, 224) == 256 * (841 * 256 + 4)
    for args in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, -1, 8), (1 << 63, 8, 8), ((1 << 64) - 1, 1, 1),
                 (1 << 54, 8, 8), (1 << 40, 0x7FFFFFFF, 0x7FFFFFFF)):
        assert L.jpegr_crop_scratch_bytes(*args) == 0, args
    prev = 0
    for n in (1, 2, 3, 64, 65, 1000):
        cur = L.jpegr_crop_scratch_bytes(n, 64, 48)
        assert cur > prev and cur % 16 == 0
        prev = cur
    for axis in (0, 1):
        prev = 0
        for m in range(1, 70):
            cur = L.jpegr_crop_scratch_bytes(5, *((m, 48) if axis == 0 else (64, m)))
            assert cur >= prev > 0 or prev == 0
            prev = cur
    assert L.jpegr_crop_scratch_bytes(5, 9, 48) > L.jpegr_crop_scratch_bytes(5, 8, 48)


def test_bindings_match_the_header():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sigs["jpegr_stream_index_device"][0] is ctypes.c_int
    assert len(sigs["jpegr_stream_index_device"][1]) == 9
    assert sigs["jpegr_crop_device"][0] is ctypes.c_int and len(sigs["jpegr_crop_device"][1]) == 15
    assert sigs["jpegr_crop_items"][0] is ctypes.c_size_t and len(sigs["jpegr_crop_items"][1]) == 2
    assert sigs["jpegr_crop_scratch_bytes"][0] is ctypes.c_size_t
    assert len(sigs["jpegr_crop_scratch_bytes"][1]) == 3
