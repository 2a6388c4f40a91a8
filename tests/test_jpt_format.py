"""The JPT1 stream format (include/jpegr.h) without a GPU: the plain-Python
restatement (tests/jpt_format.py) round-trips the crafted decoder batch and
slots on every edge of the mode rule, is never larger than JPR1, and gives the
pinned lengths on the oracle's records of an image; the host-only entry
points; the tight packer refuses bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import entropy_inputs as E
import jpr_format as J
import jpt_format as T
import jpt_inputs as I
from lz4jpeg import _lib

JPEGR_ERR_ARG = -1


@pytest.fixture(scope="module")
def crafted(oracle):
    cb = E.crafted_batch(oracle)
    bits, meta, table, _ = E.pack(cb.streams)
    return bits, meta, table


def batches(crafted):
    return {"crafted": crafted, "edges": I.edge_slots(), "random": I.random_slots(96)}


def _dims(arrays):
    return 8 * arrays[1].shape[0], 8, 1


def test_restatement_round_trips(crafted):
    for name, arrays in batches(crafted).items():
        dims = _dims(arrays)
        data = T.pack(*arrays, *dims)
        assert T.header(data) == dims and J.header(data) is None, name
        nt = arrays[1].shape[0]
        sizes = np.frombuffer(data[16:16 + 2 * nt], "<u2")
        assert len(data) == 16 + 2 * nt + int(sizes.sum()) and sizes.max() <= J.RECORD_MAX, name
        bits, meta, table, implied, verdict = T.unpack(data, fill=0x5A)
        assert (implied, verdict) == (len(data), J.OK), name
        low = (arrays[0], arrays[1], arrays[2] & 0x00FFFFFF)        # bits 24..31 are dropped
        assert J.live_equal(low, (bits, meta, table & 0x00FFFFFF)) is None, name
        assert T.pack(bits, meta, table, *dims) == data, name     # nothing but the live bytes
        recs, _, _ = T.parse(data)
        got = np.array([[s[3] for s in r] for r in recs])
        assert np.array_equal(got, T.stream_modes(*arrays)), name   # the writer's modes are canonical


def test_forced_modes_round_trip(crafted):
    """Any legal mode of a stream reads back to the same slots; mode 0 of
    every stream is the JPR1 stream but for the magic."""
    for name, arrays in batches(crafted).items():
        dims = _dims(arrays)
        canon = T.stream_modes(*arrays)
        low = (arrays[0], arrays[1], arrays[2] & 0x00FFFFFF)
        zero = T.pack(*arrays, *dims, modes=np.zeros_like(canon).tolist())
        assert zero[4:] == J.pack(*arrays, *dims)[4:] and zero[:4] == b"JPT1", name
        two = np.where(canon == 1, 2, canon)                        # mode 1 tables also fit mode 2
        for modes in (np.zeros_like(canon), two):
            data = T.pack(*arrays, *dims, modes=modes.tolist())
            bits, meta, table, implied, verdict = T.unpack(data)
            assert (implied, verdict) == (len(data), J.OK), name
            assert J.live_equal(low, (bits, meta, table)) is None, name


def test_mode_coverage(crafted):
    seen = {k: False for k in ("ncodes 0", "odd", "even", "len 15", "len 16", "-128", "127", "-129",
                               "128", "128 codes", "mode 0", "mode 1", "mode 2")}
    for arrays in batches(crafted).values():
        _, meta, table = arrays
        modes = T.stream_modes(*arrays)
        for t in range(meta.shape[0]):
            for c in range(3):
                ents = T.entries(table[t], meta[t, c], c)
                md, n = int(modes[t, c]), len(ents)
                vals, lens = [v for v, _ in ents], [L for _, L in ents]
                seen[f"mode {md}"] = True
                seen["ncodes 0"] |= n == 0 and md == 0
                seen["odd"] |= n % 2 == 1 and md != 0
                seen["even"] |= n > 0 and n % 2 == 0 and md != 0
                seen["len 15"] |= n > 0 and max(lens) == 15 and md == 1
                seen["len 16"] |= n > 0 and max(lens) == 16 and md == 0
                seen["-128"] |= n > 0 and min(vals) == -128 and md == 1
                seen["127"] |= n > 0 and max(vals) == 127 and md == 1
                seen["-129"] |= n > 0 and min(vals) == -129 and max(vals) <= 127 and md == 2
                seen["128"] |= n > 0 and max(vals) == 128 and min(vals) >= -128 and md == 2
                seen["128 codes"] |= n == 128 and md == 1
    assert all(seen.values()), seen


def test_never_larger_than_jpr1(crafted):
    for name, arrays in batches(crafted).items():
        dims = _dims(arrays)
        nt = arrays[1].shape[0]
        a = np.frombuffer(J.pack(*arrays, *dims)[16:16 + 2 * nt], "<u2")
        b = np.frombuffer(T.pack(*arrays, *dims)[16:16 + 2 * nt], "<u2")
        assert (b <= a).all(), name
        bits, meta, table = arrays
        for t in range(nt):
            for c in range(3):
                assert len(T.pack_stream(bits[t], meta[t, c], table[t], c)) <= \
                    len(J.pack_stream(bits[t], meta[t, c], table[t], c)), (name, t, c)


def test_meta_past_the_slot_is_clamped():
    bits, meta, table = I.overflow_slots()
    data = T.pack(bits, meta, table, 32, 8, 1)
    assert data == T.pack(bits, I.clamp(meta), table, 32, 8, 1)
    assert T.unpack(data)[4] == J.OK
    assert np.array_equal(T.unpack(data)[1], I.clamp(meta))


def test_restatement_verdicts():
    arrays = I.random_slots(5, seed=3)
    data = T.pack(*arrays, 40, 8, 1)
    assert T.unpack(data)[4] == J.OK
    assert T.unpack(data[:-1])[4] == 0
    assert T.unpack(b"JPR1" + data[4:])[4] == 0 and T.unpack(b"JPR2" + data[4:])[4] == 0
    assert T.unpack(data, dims=(40, 16, 1))[4] == 0
    off = 16 + 2 * 5 + int(np.frombuffer(data[16:16 + 2 * 2], "<u2").sum())
    bad = bytearray(data)
    bad[off + 3] |= 0xC0                                    # tile 2's luma mode = 3
    _, m, _, _, verdict = T.unpack(bytes(bad))
    assert verdict == 3 and not m[2].any() and np.array_equal(m[[0, 1, 3, 4]], arrays[1][[0, 1, 3, 4]])


def test_pinned_lengths(oracle):
    """The oracle's records of rand_image(512, 256, seed 1): 307,415 B as JPR1,
    218,546 B as JPT1 (150.10 and 106.70 B per tile with the index), every
    stream in mode 1."""
    img = oracle.rand_image(512, 256, seed=1)
    arrays = I.oracle_slots(oracle, oracle.jpeg_encode(img))
    assert arrays[1].shape[0] == 2048
    assert len(J.pack(*arrays, 512, 256, 1)) == 307415
    assert len(T.pack(*arrays, 512, 256, 1)) == 218546
    assert (T.stream_modes(*arrays) == 1).all()


def test_stream_format():
    L = _lib.lib()
    w, h, n, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ref = (ctypes.byref(w), ctypes.byref(h), ctypes.byref(n), ctypes.byref(f))
    tail = (3840).to_bytes(4, "little") + (2160).to_bytes(4, "little") + (3).to_bytes(4, "little")
    for magic, fmt in ((b"JPR1", 1), (b"JPT1", 2)):
        assert L.jpegr_stream_format(magic + tail, *ref) == 0
        assert (w.value, h.value, n.value, f.value) == (3840, 2160, 3, fmt)
    for magic in (b"JPR2", b"JPT2", b"jPT1", b"JPS1", b"\0\0\0\0"):
        assert L.jpegr_stream_format(magic + tail, *ref) == JPEGR_ERR_ARG, magic
    good = b"JPT1" + tail
    for k in (4, 8, 12):                                    # w, h, nimg of zero
        assert L.jpegr_stream_format(good[:k] + bytes(4) + good[k + 4:], *ref) == JPEGR_ERR_ARG
    assert L.jpegr_stream_format(None, *ref) == JPEGR_ERR_ARG
    for i in range(4):
        args = list(ref)
        args[i] = None
        assert L.jpegr_stream_format(good, *args) == JPEGR_ERR_ARG, i
    # jpegr_stream_info keeps to JPR1
    assert L.jpegr_stream_info(good, *ref[:3]) == JPEGR_ERR_ARG
    from lz4jpeg import jpeg
    assert jpeg.stream_format(good) == (3840, 2160, 3, True)
    assert jpeg.stream_format(b"JPR1" + tail) == (3840, 2160, 3, False)
    with pytest.raises(jpeg.JpegError):
        jpeg.stream_format(b"JPR2" + tail)
    with pytest.raises(jpeg.JpegError):
        jpeg.stream_info(good)


def test_pack_tight_rejects_bad_arguments_before_device():
    """NULL pointers, bad dimensions and misaligned buffers are argument
    errors found before any HIP call, so this runs without a GPU."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)            # never dereferenced: every case fails first
    good = [p, p, p, 8, 8, 1, p, 4096, p, p, None]
    for i in (0, 1, 2, 6, 8, 9):
        args = list(good)
        args[i] = None
        assert L.jpegr_pack_tight_device(*args) == JPEGR_ERR_ARG, i
    for i, v in ((3, 0), (4, 0), (5, 0), (3, -8), (0, ctypes.c_void_p(4098)),
                 (1, ctypes.c_void_p(4097)), (2, ctypes.c_void_p(4098)), (6, ctypes.c_void_p(4104)),
                 (8, ctypes.c_void_p(4100)), (9, ctypes.c_void_p(4104))):
        args = list(good)
        args[i] = v
        assert L.jpegr_pack_tight_device(*args) == JPEGR_ERR_ARG, (i, v)
    args = list(good)
    args[3], args[4] = 1 << 30, 1 << 30                     # more than 2^32 tiles
    assert L.jpegr_pack_tight_device(*args) == JPEGR_ERR_ARG
