"""The compressor's C ABI over two builds of csrc/lz4r.hip (a helper, no tests):

  "product"  lz4-jpeg_amd/lz4jpeg/liblz4jpeg.so, launch chunks of 2^24 blocks;
  "chunk12"  lz4-jpeg_amd/build/liblz4r_chunk12.so (`make chunk12`, part of
             `make all`): the same source and flags with -DLZ4R_CHUNK_LOG2=12,
             so an input of a few MB crosses launch-chunk boundaries.

Both are loaded with ctypes and given the signatures of lz4jpeg/_lib.py's
table, and both are driven through the same few calls, so every chunk test
runs on both.  A missing variant library is an error naming the make target.
"""
import ctypes
import os

import numpy as np

from lz4jpeg import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK12_PATH = os.path.join(REPO, "lz4-jpeg_amd", "build", "liblz4r_chunk12.so")
CHUNK12_TARGET = "chunk12"
CHUNK12_LOG2 = 12
NAMES = ("product", "chunk12")

# what the variant must export: the compressor's entry points (csrc/lz4r.hip)
COMPRESSOR_ENTRY_POINTS = (
    "lz4r_ctx_create", "lz4r_ctx_destroy", "lz4r_compress_bound", "lz4r_nblocks",
    "lz4r_launch_chunk_blocks", "lz4r_compress_device", "lz4r_compress_async",
    "lz4r_compress_segment_async", "lz4r_copy_block_sizes", "lz4r_copy_block_offsets",
    "lz4r_block_offsets_device", "lz4r_block_matches_device", "lz4r_window_matches_device",
    "lz4r_compress", "lz4r_check", "lz4r_set_timing", "lz4r_last_timing", "lz4r_timed_calls",
    "lz4r_strerror")

_vp = ctypes.c_void_p
_loaded = {}


class VariantMissing(RuntimeError):
    pass


def path(name):
    return {"product": _lib.LIB_PATH, "chunk12": CHUNK12_PATH}[name]


def expected_chunk_blocks(name):
    return {"product": 1 << 24, "chunk12": 1 << CHUNK12_LOG2}[name]


def load(name):
    """The ctypes handle of one build, its lz4r_* symbols typed from
    _lib.SIGNATURES (the variant holds the compressor only: every compressor
    entry point must be there, the decoder's are not)."""
    if name in _loaded:
        return _loaded[name]
    p = path(name)
    if not os.path.exists(p):
        raise VariantMissing(f"{p} is not built: run `make -C {REPO} {CHUNK12_TARGET}` "
                             "(it is part of `make all`); the chunk tests do not skip")
    handle = ctypes.CDLL(p)
    table = {n: (res, args) for n, res, args in _lib.SIGNATURES if n.startswith("lz4r_")}
    for n in COMPRESSOR_ENTRY_POINTS:
        res, args = table[n]
        fn = getattr(handle, n)          # AttributeError: the build lacks an entry point
        fn.restype = res
        fn.argtypes = args
    _loaded[name] = handle
    return handle


def _stream():
    import torch
    return _vp(torch.cuda.current_stream().cuda_stream)


def _ptr(t, off=0):
    return _vp(t.data_ptr() + off)


def chunk_blocks(name):
    return int(load(name).lz4r_launch_chunk_blocks())


def block_matches_device(name, d_in, n, d_matches):
    """lz4r_block_matches_device on torch tensors (uint8 in, int32/uint32 out);
    returns the code."""
    return load(name).lz4r_block_matches_device(_ptr(d_in), n, _ptr(d_matches), _stream())


class Ctx:
    """One lz4r context of one build.  Tensors are torch CUDA tensors; every
    call returns the C return code (the tests assert it)."""

    def __init__(self, name):
        self.name = name
        self.L = load(name)
        self.h = _vp()
        rc = self.L.lz4r_ctx_create(ctypes.byref(self.h))
        assert rc == _lib.LZ4R_OK, (name, rc)

    def close(self):
        if self.h:
            self.L.lz4r_ctx_destroy(self.h)
            self.h = _vp()

    def compress_async(self, d_in, n, d_out, cap, d_len):
        return self.L.lz4r_compress_async(self.h, _ptr(d_in), n, _ptr(d_out), cap, _ptr(d_len),
                                          _stream())

    def compress_segment_async(self, d_in, n, d_out, cap, d_len, final_shard):
        return self.L.lz4r_compress_segment_async(self.h, _ptr(d_in), n, _ptr(d_out), cap,
                                                  _ptr(d_len), 1 if final_shard else 0, _stream())

    def compress_device(self, d_in, n, d_out, cap):
        """-> (code, *out_len)"""
        got = ctypes.c_size_t(0)
        rc = self.L.lz4r_compress_device(self.h, _ptr(d_in), n, _ptr(d_out), cap,
                                         ctypes.byref(got), _stream())
        return rc, got.value

    def block_offsets(self, count):
        out = np.empty(count, dtype=np.uint64)
        rc = self.L.lz4r_copy_block_offsets(self.h, out.ctypes.data_as(_vp), count, _stream())
        assert rc == _lib.LZ4R_OK, rc
        return out

    def block_sizes(self, count):
        out = np.empty(count, dtype=np.uint16)
        rc = self.L.lz4r_copy_block_sizes(self.h, out.ctypes.data_as(_vp), count, _stream())
        assert rc == _lib.LZ4R_OK, rc
        return out

    def block_offsets_device(self):
        ptr, cnt = _vp(), ctypes.c_size_t(0)
        rc = self.L.lz4r_block_offsets_device(self.h, ctypes.byref(ptr), ctypes.byref(cnt))
        assert rc == _lib.LZ4R_OK, rc
        return ptr.value, cnt.value

    def check(self):
        return self.L.lz4r_check(self.h, _stream())

    def set_timing(self, enable):
        return self.L.lz4r_set_timing(self.h, 1 if enable else 0)

    def timed_calls(self, max_calls=64):
        a = (ctypes.c_float * max_calls)()
        b = (ctypes.c_float * max_calls)()
        cnt = ctypes.c_size_t(0)
        rc = self.L.lz4r_timed_calls(self.h, max_calls, a, b, ctypes.byref(cnt))
        assert rc == _lib.LZ4R_OK, rc
        return list(a[:cnt.value]), list(b[:cnt.value])
