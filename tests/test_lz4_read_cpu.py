"""The host side of LZ4 random access, without a GPU: lz4r_read_items' bound,
every LZ4R_ERR_ARG of lz4r_read_device and lz4r_stream_index_device (found
before any HIP call: the pointers below are never dereferenced), and the
Python model the GPU tests compare against (lz4_read_model.py) on cases
written by hand."""
import ctypes

import numpy as np

import lz4_read_model as M
from lz4jpeg import _lib

ARG = _lib.LZ4R_ERR_ARG


def test_read_items_bounds_the_blocks_of_a_read():
    L_ = _lib.lib()
    for L in range(1, 1301):
        K = L_.lz4r_read_items(L)
        assert K == M.read_items(L) == (L + 298) // 300 + 1
        covered = [(o + L - 1) // 300 + 1 for o in range(300)]
        assert max(covered) == K, (L, K, max(covered))      # <= K, with equality for some o
    assert L_.lz4r_read_items(0) == 1
    assert L_.lz4r_read_items((1 << 64) - 1) == 0           # no such read


def _read_args(**kw):
    p = ctypes.c_void_p(64)              # never dereferenced: every case fails first
    a = dict(d_in=p, in_len=1000, offs=p, nb=4, reads=p, nreads=5, max_len=300, out=p,
             out_cap=4096, res=p, stream=None)
    a.update(kw)
    return [a[k] for k in ("d_in", "in_len", "offs", "nb", "reads", "nreads", "max_len", "out",
                           "out_cap", "res", "stream")]


def test_read_device_rejects_bad_arguments_before_device():
    L = _lib.lib()
    odd = ctypes.c_void_p(68)
    cases = {
        "d_in NULL": dict(d_in=None), "offsets NULL": dict(offs=None),
        "reads NULL": dict(reads=None), "out NULL": dict(out=None), "result NULL": dict(res=None),
        "nb 0": dict(nb=0), "nreads 0": dict(nreads=0), "max_len 0": dict(max_len=0),
        "in_len 3": dict(in_len=3),
        "reads misaligned": dict(reads=odd), "offsets misaligned": dict(offs=odd),
        "result misaligned": dict(res=odd),
        # items = nreads * K; a workgroup per 32 of them, 2^31 - 1 at most
        "grid K=2": dict(nreads=((1 << 31) - 1) * 16 + 1, max_len=300),
        "grid K=11": dict(nreads=((1 << 31) - 1) * 32 // 11 + 1, max_len=3000),
        "grid overflow": dict(nreads=1 << 63, max_len=1 << 40),
        "max_len overflow": dict(max_len=(1 << 64) - 1),
    }
    for name, kw in cases.items():
        assert L.lz4r_read_device(*_read_args(**kw)) == ARG, name


def test_stream_index_device_rejects_bad_arguments_before_device():
    L = _lib.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)
    nb, n = ctypes.c_size_t(7), ctypes.c_size_t(7)
    r = (ctypes.byref(nb), ctypes.byref(n))
    assert L.lz4r_stream_index_device(None, 100, p, 10, *r, None) == ARG
    assert L.lz4r_stream_index_device(p, 100, None, 10, *r, None) == ARG
    assert L.lz4r_stream_index_device(p, 100, odd, 10, *r, None) == ARG
    assert L.lz4r_stream_index_device(p, 100, p, 10, None, r[1], None) == ARG
    assert L.lz4r_stream_index_device(p, 100, p, 10, r[0], None, None) == ARG
    # a stream too short to hold a block is corrupt, also before any HIP call
    assert L.lz4r_stream_index_device(p, 8, p, 10, *r, None) == _lib.LZ4R_ERR_CORRUPT
    assert (nb.value, n.value) == (0, 0)


# ---- the model ----------------------------------------------------------------------
PLAIN = bytes(range(256)) * 4 + bytes(193)          # 1217 bytes: 4 blocks and 17
S = 0xA5


def _exp(reads, out_cap=64, max_len=40, **kw):
    buf, got, verdict = M.expected(PLAIN, reads, out_cap, max_len, S, **kw)
    return bytes(buf), got, verdict


def test_model_good_reads():
    buf, got, verdict = _exp([(0, 3, 0), (299, 2, 4), (1216, 1, 7), (5, 0, 63), (77, 0, 1 << 63)])
    assert buf == bytes([0, 1, 2, S, 43, 44, S, 0]) + bytes([S]) * 56
    assert (got, verdict) == (6, M.OK)


def test_model_bad_on_own_fields_writes_nothing():
    for rd in [(0, 41, 0), ((1 << 64) - 2, 2, 0), ((1 << 64) - 2, 3, 0), (0, 2, 63),
               (0, 2, (1 << 64) - 1), (1500, 1, 0), (1499, 2, 0)]:
        buf, got, verdict = _exp([(10, 2, 8), rd, (20, 1, 12)])
        assert buf == bytes([S]) * 8 + bytes([10, 11, S, S, 20]) + bytes([S]) * 51, rd
        assert (got, verdict) == (3, 2), rd
        assert M.loose_ranges(PLAIN, [rd], 64, 40) == [], rd


def test_model_bad_inside_a_block():
    # past the decoded end inside the short last block; src at the decoded length
    for rd in [(1210, 8, 30), (1217, 1, 30), (1180, 40, 20)]:
        reads = [(0, 1, 0), rd, (1216, 1, 2)]
        buf, got, verdict = _exp(reads)
        assert buf[:3] == bytes([0, S, 0]) and (got, verdict) == (2, 2)
        assert M.loose_ranges(PLAIN, reads, 64, 40) == [(rd[2], rd[2] + rd[1])]
    # a malformed block: the reads that touch it, and only they
    reads = [(599, 1, 0), (599, 2, 2), (600, 1, 5), (899, 2, 7), (900, 1, 10)]
    buf, got, verdict = _exp(reads, bad_blocks=(2,))
    assert (got, verdict) == (2, 2)
    assert buf[:11] == bytes([PLAIN[599]] + [S] * 9 + [PLAIN[900]])
    assert M.loose_ranges(PLAIN, reads, 64, 40, (2,)) == [(2, 4), (5, 6), (7, 9)]


def test_model_first_bad_read_wins():
    assert _exp([(0, 1, 0), (0, 41, 0), (1217, 1, 9)])[2] == 2
    assert _exp([(1217, 1, 9), (0, 41, 0)])[2] == 1
    assert np.array_equal(M.expected(PLAIN, [], 4, 4, S)[0], np.full(4, S, np.uint8))
