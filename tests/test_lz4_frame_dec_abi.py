"""The GPU frame decoder's C ABI where no device is needed: the symbols are
there, argument errors come back before any HIP call, and the error strings
are what they were."""
import ctypes

from lz4jpeg import _lib


def test_symbols_exported_and_bound():
    L = _lib.lib()
    names = {n for n, _, _ in _lib.SIGNATURES}
    for name in ("lz4r_frame_decompress_device", "lz4r_frame_decompress_gpu"):
        assert name in names
        assert getattr(L, name).restype is ctypes.c_int
    assert _lib.LZ4R_FRAME_NO_CONTENT_CHECKSUM == 1


def test_null_arguments_are_refused_before_any_hip_call():
    L = _lib.lib()
    got = ctypes.c_size_t(123)
    p = ctypes.c_void_p(4096)                 # never dereferenced: the call returns first
    dev, gpu = L.lz4r_frame_decompress_device, L.lz4r_frame_decompress_gpu
    assert dev(None, 10, p, 10, ctypes.byref(got), 0, None) == _lib.LZ4R_ERR_ARG
    assert dev(p, 10, p, 10, None, 0, None) == _lib.LZ4R_ERR_ARG
    assert dev(p, 10, None, 1, ctypes.byref(got), 0, None) == _lib.LZ4R_ERR_ARG
    assert gpu(None, 10, p, 10, ctypes.byref(got), 0) == _lib.LZ4R_ERR_ARG
    assert gpu(p, 10, p, 10, None, 0) == _lib.LZ4R_ERR_ARG
    assert gpu(p, 10, None, 1, ctypes.byref(got), 0) == _lib.LZ4R_ERR_ARG
    assert got.value == 123
    # the empty input is corrupt, as on the host, and that too needs no device
    assert dev(p, 0, p, 10, ctypes.byref(got), 0, None) == _lib.LZ4R_ERR_CORRUPT
    assert got.value == 0
    got.value = 5
    assert gpu(p, 0, None, 0, ctypes.byref(got), 0) == _lib.LZ4R_ERR_CORRUPT
    assert got.value == 0
    assert L.lz4r_frame_decompress(p, 0, p, 10, ctypes.byref(got)) == _lib.LZ4R_ERR_CORRUPT


def test_strerror_unchanged():
    L = _lib.lib()
    want = {0: "ok", -1: "invalid argument", -2: "input shorter than one 300-byte block",
            -3: "output buffer too small", -4: "HIP runtime error", -5: "device allocation failed",
            -6: "corrupt stream", -7: "unknown error", 1: "unknown error"}
    assert {c: L.lz4r_strerror(c).decode() for c in want} == want
