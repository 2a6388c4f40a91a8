"""The standard-frame model (tests/lz4_frame_model.py) and the host decoder
lz4r_frame_decompress, without a GPU: the model's frames decode to their input
under the model's strict decoder, the library's host decoder and, where the
system has one, liblz4; the bound holds on the worst inputs; the host decoder
reads every variant frame and turns every damaged one into an error."""
import os
import struct
from ctypes import byref, c_size_t

import numpy as np
import pytest

import lz4_frame_model as FM
from lz4_seq_inputs import BLK, block_exact, block_packed, block_trunc
from lz4jpeg import _lib, lz4

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORRUPT, CAPACITY = _lib.LZ4R_ERR_CORRUPT, _lib.LZ4R_ERR_CAPACITY


@pytest.fixture(scope="module")
def text():
    return open(os.path.join(GOLDEN, "Metamorphosis.txt"), "rb").read()


@pytest.fixture(scope="module")
def liblz4():
    return FM.system_liblz4()


def host_decode(frame, cap, guard=64):
    """(code, *out_len, output) of lz4r_frame_decompress with `guard` bytes
    after cap that must stay as they were."""
    buf = np.frombuffer(bytes(frame), dtype=np.uint8)
    out = np.full(cap + guard, 0xA5, dtype=np.uint8)
    got = c_size_t(0)
    rc = _lib.call("lz4r_frame_decompress", buf if buf.size else np.zeros(1, np.uint8), buf.size,
                   out, cap, byref(got))
    assert (out[cap:] == 0xA5).all(), "wrote past cap"
    return rc, got.value, out[:cap].tobytes()


def rng_bytes(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def model_inputs(text):
    return {
        "text 38701": text[:38701],
        "300": text[:300],
        "19201": text[:19201], "19211": text[:19211], "19212": text[:19212],
        "19213": text[:19213],
        "zeros 700": bytes(700),
        "random 19250": rng_bytes(19250),
        "trunc 257": block_trunc(257) * 3,
    }


def test_xxh32_known_values():
    # the digest's published test values
    assert FM.xxh32(b"") == 0x02CC5D05
    assert FM.xxh32(b"a") == 0x550D7456
    assert FM.xxh32(b"abc") == 0x32D153FF
    assert FM.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


@pytest.mark.parametrize("name", ["text 38701", "300", "19201", "19211", "19212", "19213",
                                  "zeros 700", "random 19250", "trunc 257"])
def test_model_frames_decode_to_the_input(oracle, text, liblz4, name):
    plain = model_inputs(text)[name]
    frame, _ = FM.expected(oracle, plain)
    assert frame[:6] == b"\x04\x22\x4d\x18\x68\x40" and frame[-4:] == bytes(4)
    assert struct.unpack_from("<Q", frame, 6)[0] == len(plain)
    assert len(frame) <= FM.frame_bound(len(plain)) == lz4.frame_bound(len(plain))
    assert FM.decode_strict(frame) == plain
    assert host_decode(frame, len(plain)) == (0, len(plain), plain)
    assert lz4.decompress_frame(frame) == plain
    if liblz4 is not None:
        got, used, ret = FM.liblz4_decompress(liblz4, frame, len(plain) + 64)
        assert (got, used, ret) == (plain, len(frame), 0)


def test_frame_bound_on_the_worst_inputs(oracle):
    allp = block_packed(20) * 70                       # the most sequences a block can hold
    exact = block_exact(53) * 70
    for plain in (rng_bytes(3 * 19200 + 17), allp, exact):
        frame, _ = FM.expected(oracle, plain)
        assert len(frame) <= lz4.frame_bound(len(plain))
        assert FM.decode_strict(frame) == plain
    # an all-literal data block is the bound's case: 1 + 76 + 19,200 bytes
    frame, runs = FM.expected(oracle, rng_bytes(19200))
    assert runs == [[19200]] and len(frame) == 15 + 4 + 1 + 76 + 19200 + 4


def test_host_decoder_reads_every_variant(text, liblz4):
    plain = text[1000:1000 + 3 * 4096 + 123]
    for name, (frame, want) in FM.variants(plain).items():
        assert FM.decode_strict(frame) == want, name
        assert host_decode(frame, len(want)) == (0, len(want), want), name
        if liblz4 is not None:
            two = 2 if name == "two frames" else 1
            got, at = b"", 0
            for _ in range(two):
                g, used, ret = FM.liblz4_decompress(liblz4, frame[at:], len(want) + 64)
                assert ret == 0, name
                got, at = got + g, at + used
            assert (got, at) == (want, len(frame)), name


def test_host_decoder_reads_liblz4_frames(text, liblz4):
    if liblz4 is None:
        pytest.skip("no system liblz4")
    plain = text[:100000] * 2                          # four linked 64 KiB blocks
    for linked, sums in ((True, True), (False, False)):
        frame = FM.liblz4_compress(liblz4, plain, linked=linked, checksums=sums)
        assert host_decode(frame, len(plain)) == (0, len(plain), plain)
    both = FM.liblz4_compress(liblz4, plain[:777]) + FM.liblz4_compress(liblz4, plain[777:5000])
    assert host_decode(both, 5000) == (0, 5000, plain[:5000])


@pytest.fixture(scope="module")
def small(text):
    """A small frame with checksums (a damaged literal is then an error, not
    other text) of two linked blocks, and its plain text."""
    plain = text[2000:2000 + 700]
    return FM.write_variant(plain, block=400, linked=True, block_checksum=True,
                            content_checksum=True), plain


def test_every_proper_prefix_is_corrupt(small, oracle):
    frame, plain = small
    ours, _ = FM.expected(oracle, plain)
    for f in (frame, ours):
        for k in range(len(f)):
            rc, _, _ = host_decode(f[:k], len(plain))
            assert rc == CORRUPT, k


def test_every_single_byte_mutation_is_the_text_or_an_error(small):
    frame, plain = small
    for i in range(len(frame)):
        for delta in (1, 0x80, 0xFF):
            bad = bytearray(frame)
            bad[i] = (bad[i] + delta) & 255
            rc, n, out = host_decode(bad, len(plain))
            assert rc in (CORRUPT, CAPACITY) or (rc == 0 and out[:n] == plain), (i, delta, rc)


def _one_block_frame(body, n):
    return FM.header(0x68, 0x40, n) + struct.pack("<I", len(body)) + body + bytes(4)


def test_malformed_frames_are_corrupt(small, oracle):
    frame, plain = small
    ok = _one_block_frame(b"\x50hello", 5)
    assert host_decode(ok, 5) == (0, 5, b"hello")
    cases = {
        "offset before the output start": _one_block_frame(b"\x10a\x02\x00" + b"\x50hello", 10),
        "offset 0": _one_block_frame(b"\x10a\x00\x00" + b"\x50hello", 10),
        "literal run past the block end": _one_block_frame(b"\x60hello", 6),
        "block ends with a match": _one_block_frame(b"\x50hello\x01\x00", 9),
        "wrong content size": _one_block_frame(b"\x50hello", 6),
        "block over the block maximum": FM.header(0x68, 0x40, 5) + struct.pack("<I", 65537),
        "dictionary ID": FM.header(0x69, 0x40, 5) + bytes(4) + ok[15:],
        "reserved FLG bit": FM.header(0x6A, 0x40, 5) + ok[15:],
        "reserved BD bit": FM.header(0x68, 0x41, 5) + ok[15:],
        "version 2": FM.header(0xA8, 0x40, 5) + ok[15:],
        "skippable magic": b"\x50\x2a\x4d\x18" + struct.pack("<I", 4) + bytes(4),
        "legacy magic": b"\x02\x21\x4c\x18" + struct.pack("<I", 6) + b"\x50hello",
        "empty": b"",
        "trailing garbage": ok + b"\x00",
    }
    hc = bytearray(ok)
    hc[14] ^= 1
    cases["wrong header checksum"] = bytes(hc)
    cc = bytearray(frame)
    cc[-1] ^= 1
    cases["wrong content checksum"] = bytes(cc)
    for name, f in cases.items():
        assert host_decode(f, 64 if f is not cases["wrong content checksum"] else len(plain))[0] == CORRUPT, name
    with pytest.raises(lz4.Lz4Error) as e:
        lz4.decompress_frame(cases["wrong header checksum"])
    assert e.value.code == CORRUPT


def test_a_cap_one_byte_short_is_capacity(small, oracle):
    frame, plain = small
    ours, _ = FM.expected(oracle, plain)
    for f in (frame, ours, FM.write_variant(plain, stored=(0,))):
        rc, need, _ = host_decode(f, len(plain) - 1)
        assert rc == CAPACITY and len(plain) - 1 < need <= len(plain)
        assert host_decode(f, 0)[0] == CAPACITY
    with pytest.raises(lz4.Lz4Error) as e:
        lz4.decompress_frame(frame, cap=len(plain) - 1)
    assert e.value.code == CAPACITY
