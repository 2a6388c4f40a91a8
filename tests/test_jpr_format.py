"""The JPR stream format (include/jpegr.h) without a GPU: the plain-Python
restatement (tests/jpr_format.py) round-trips the crafted decoder batch and
its unpacked streams decode through the oracle; the host-only entry points;
every device entry point refuses bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import entropy_inputs as E
import jpr_format as J
import oracle_api
from lz4jpeg import _lib

JPEGR_ERR_ARG = -1


@pytest.fixture(scope="module")
def crafted(oracle):
    cb = E.crafted_batch(oracle)
    bits, meta, table, want = E.pack(cb.streams)
    nt = len(cb.streams)
    data = J.pack(bits, meta, table, 8 * nt, 8, 1)
    return cb, (bits, meta, table), data


def test_restatement_round_trips_crafted_batch(crafted):
    cb, arrays, data = crafted
    nt = len(cb.streams)
    assert nt == E.LANES * len(cb.names) == 704           # every crafted wave, whole
    assert J.header(data) == (8 * nt, 8, 1)
    sizes = np.frombuffer(data[16:16 + 2 * nt], "<u2")
    assert len(data) == 16 + 2 * nt + int(sizes.sum()) and sizes.max() <= J.RECORD_MAX
    bits, meta, table, implied, verdict = J.unpack(data, fill=0x5A)
    assert (implied, verdict) == (len(data), J.OK)
    assert J.live_equal(arrays, (bits, meta, table)) is None
    # nothing but the live bytes came from the stream
    assert J.pack(bits, meta, table, 8 * nt, 8, 1) == data


def test_unpacked_streams_decode_to_expected(crafted, oracle):
    cb, _, data = crafted
    bits, meta, table, _, verdict = J.unpack(data)
    assert verdict == J.OK
    for t, row in enumerate(cb.streams):
        for c, s in enumerate(row):
            nbits, rle_len, ncodes = J.fields(meta[t, c])
            o = J.SLOT_OFF[c]
            ents = table[t, o:o + ncodes].tolist()
            lens = [(e >> 16) & 255 for e in ents]
            vals = [int((e & 0xFFFF) ^ 0x8000) - 0x8000 for e in ents]
            codes = E.codes_from_lengths(lens) if ncodes > 1 else [0]
            e = {"table": list(zip(vals, lens, codes)), "nbits": nbits, "rle": [0] * rle_len,
                 "bits": bits[t, o:o + (nbits + 7) // 8].tobytes()}
            got = oracle_api.entropy_decode(oracle, e, E.N[c])
            assert got == s.expected.tolist(), (t, c, s.tag)


def test_crafted_batch_reaches_the_format_edges(crafted):
    cb, (_, meta, _), _ = crafted
    for c in range(3):
        nbits, ncodes = meta[:, c] & 0xFFFF, meta[:, c] >> 24
        assert np.any(nbits == J.SLOT_BITS[c]), c           # a full slot of bits
        assert np.any((ncodes == 1) & (nbits == 0)), c      # a stream of nothing but its header
    assert np.any(meta[:, 0] >> 24 == 128) and np.any(meta[:, 1] >> 24 == 64)


def test_restatement_verdicts():
    rng = np.random.default_rng(7)
    nt = 5
    bits = rng.integers(0, 256, (nt, 256)).astype(np.uint8)
    table = rng.integers(0, 1 << 24, (nt, 256)).astype(np.uint32)
    meta = np.zeros((nt, 3), np.uint32)
    for t in range(nt):
        for c in range(3):
            meta[t, c] = int(rng.integers(0, J.SLOT_BITS[c] + 1)) | \
                int(rng.integers(0, J.SLOT_CODES[c] + 1)) << 16 | \
                int(rng.integers(0, J.SLOT_CODES[c] + 1)) << 24
    data = J.pack(bits, meta, table, 40, 8, 1)
    assert J.unpack(data)[4] == J.OK
    assert J.live_equal((bits, meta, table), J.unpack(data)[:3]) is None
    assert J.unpack(data[:-1])[4] == 0
    assert J.unpack(b"JPR2" + data[4:])[4] == 0
    assert J.unpack(data, dims=(40, 16, 1))[4] == 0
    bad = bytearray(data)
    bad[16 + 2 * 3] = (bad[16 + 2 * 3] + 1) & 255           # index entry 3 raised by one
    assert J.unpack(bytes(bad))[4] == 0
    off = 16 + 2 * nt + int(np.frombuffer(data[16:16 + 2 * 2], "<u2").sum())
    bad = bytearray(data)
    bad[off + 1] = 129                                      # tile 2's luma ncodes
    _, m, _, _, verdict = J.unpack(bytes(bad))
    assert verdict == 3 and not m[2].any() and np.array_equal(m[[0, 1, 3, 4]], meta[[0, 1, 3, 4]])


def test_pack_bound_and_scratch():
    L = _lib.lib()
    assert L.jpegr_pack_bound(8, 8, 1) == 16 + 2 + 1036
    assert L.jpegr_pack_bound(3840, 2160, 2) == 16 + 2 * 480 * 270 * (2 + 1036)
    assert L.jpegr_pack_bound(0, 8, 1) == 0
    assert L.jpegr_pack_bound(8, -1, 1) == 0 and L.jpegr_pack_bound(8, 8, 0) == 0
    assert L.jpegr_pack_bound(1 << 30, 1 << 30, 1) == 0     # more than 2^32 tiles
    assert L.jpegr_pack_scratch_bytes(1) >= 8 + 4 + 4
    assert L.jpegr_pack_scratch_bytes(4097) >= 2 * 8 + 4097 * 4 + 65 * 4


def test_stream_info():
    L = _lib.lib()
    w, h, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ref = (ctypes.byref(w), ctypes.byref(h), ctypes.byref(n))
    good = b"JPR1" + (3840).to_bytes(4, "little") + (2160).to_bytes(4, "little") + \
        (3).to_bytes(4, "little")
    assert L.jpegr_stream_info(good, *ref) == 0
    assert (w.value, h.value, n.value) == (3840, 2160, 3)
    assert L.jpegr_stream_info(b"JPR2" + good[4:], *ref) == JPEGR_ERR_ARG
    assert L.jpegr_stream_info(b"jPR1" + good[4:], *ref) == JPEGR_ERR_ARG
    for k in (4, 8, 12):                                    # w, h, nimg of zero
        assert L.jpegr_stream_info(good[:k] + bytes(4) + good[k + 4:], *ref) == JPEGR_ERR_ARG
    assert L.jpegr_stream_info(None, *ref) == JPEGR_ERR_ARG
    assert L.jpegr_stream_info(good, None, ctypes.byref(h), ctypes.byref(n)) == JPEGR_ERR_ARG
    from lz4jpeg import jpeg
    assert jpeg.stream_info(good) == (3840, 2160, 3)
    with pytest.raises(jpeg.JpegError):
        jpeg.stream_info(b"JPR2" + good[4:])


def test_device_entry_points_reject_bad_arguments_before_device():
    """NULL pointers, bad dimensions and misaligned buffers are argument
    errors found before any HIP call, so this runs without a GPU."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)            # never dereferenced: every case fails first
    good = [p, p, p, 8, 8, 1, p, 4096, p, p, None]
    for i in (0, 1, 2, 6, 8, 9):
        args = list(good)
        args[i] = None
        assert L.jpegr_pack_device(*args) == JPEGR_ERR_ARG, i
    for i, v in ((3, 0), (4, 0), (5, 0), (3, -8), (6, ctypes.c_void_p(4104)),
                 (8, ctypes.c_void_p(4100))):
        args = list(good)
        args[i] = v
        assert L.jpegr_pack_device(*args) == JPEGR_ERR_ARG, (i, v)
    args = list(good)
    args[3], args[4] = 1 << 30, 1 << 30                     # more than 2^32 tiles
    assert L.jpegr_pack_device(*args) == JPEGR_ERR_ARG
    good = [p, 4096, 8, 8, 1, p, p, p, p, p, None]
    for i in (0, 5, 6, 7, 8, 9):
        args = list(good)
        args[i] = None
        assert L.jpegr_unpack_device(*args) == JPEGR_ERR_ARG, i
    for i, v in ((2, 0), (3, 0), (4, 0), (4, -1), (9, ctypes.c_void_p(4100))):
        args = list(good)
        args[i] = v
        assert L.jpegr_unpack_device(*args) == JPEGR_ERR_ARG, (i, v)
