"""Standard LZ4 frames decoded on the GPU (lz4r_frame_decompress_device;
csrc/lz4f_dec.h: lz4f_walk, lz4f_xxh32_items, lz4f_dec_sizes, lz4f_dec_scan,
lz4f_dec_blocks).  The expected answer is always the plain text, and agreement
with the host decoder (lz4r_frame_decompress) on the return code, the length
and the bytes.  Frames come from the compressor, from the model's writers
(tests/lz4_frame_model.py) and from blocks built by hand where a path needs a
particular sequence: periodic matches, the length extensions' thresholds,
matches across linked blocks, 5,000 small blocks, every pointer alignment,
every capacity, and a fixed list of malformed frames (tests/sanitize/
frame_dev_main.cpp takes the same parsers through every prefix and mutation on
the CPU).  Every call decodes into a buffer with 256 sentinel bytes on each
side, compared after it."""
import os
import struct
from ctypes import byref, c_size_t

import numpy as np
import pytest
import torch

import lz4_frame_model as FM
from lz4jpeg import _lib, lz4

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD, FILL = 256, 0xA5
OK, CAPACITY, CORRUPT = _lib.LZ4R_OK, _lib.LZ4R_ERR_CAPACITY, _lib.LZ4R_ERR_CORRUPT


@pytest.fixture(scope="module")
def text():
    return open(os.path.join(GOLDEN, "Metamorphosis.txt"), "rb").read()


@pytest.fixture(scope="module")
def comp(gpu):
    c = lz4.Compressor()
    yield c
    c.close()


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def host(frame, cap):
    """(return code, length, bytes) of the host decoder."""
    buf = np.frombuffer(bytes(frame), dtype=np.uint8)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    got = c_size_t(0)
    rc = _lib.call("lz4r_frame_decompress", buf if buf.size else out, buf.size, out, cap, byref(got))
    return rc, got.value, out[:got.value].tobytes() if rc == OK else b""


def device(frame, cap, verify=True, in_off=0, out_off=0):
    """(return code, *out_len, the cap bytes of the output buffer) of the GPU
    decoder; the input sits in_off and the output out_off bytes past a
    256-byte boundary, and the sentinels around the output are compared."""
    n = len(frame)
    d_in = torch.zeros(in_off + n + 16, dtype=torch.uint8, device="cuda")
    if n:
        d_in[in_off:in_off + n] = torch.from_numpy(np.frombuffer(bytes(frame), np.uint8).copy()).cuda()
    d_buf = torch.full((GUARD + out_off + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 256 == 0 and d_buf.data_ptr() % 256 == 0
    lo = GUARD + out_off
    got = c_size_t(0)
    flags = 0 if verify else _lib.LZ4R_FRAME_NO_CONTENT_CHECKSUM
    rc = _lib.call("lz4r_frame_decompress_device", d_in.data_ptr() + in_off, n,
                   d_buf.data_ptr() + lo, cap, byref(got), flags, _lib.stream_arg())
    out = d_buf.cpu().numpy()
    assert (out[:lo] == FILL).all() and (out[lo + cap:] == FILL).all(), "a sentinel was written"
    return rc, got.value, out[lo:lo + cap]


def decodes_to(frame, plain, verify=True, host_too=True, **where):
    """Both decoders turn `frame` into `plain`, given exactly its length."""
    plain = bytes(plain)
    rc, n, out = device(frame, len(plain), verify, **where)
    assert (rc, n) == (OK, len(plain))
    assert out.tobytes() == plain
    if host_too:
        assert host(frame, len(plain)) == (OK, len(plain), plain)


def is_corrupt(frame, cap=1 << 16, verify=True):
    """Both decoders call `frame` corrupt."""
    assert host(frame, cap)[0] == CORRUPT
    rc, n, _ = device(frame, cap, verify)
    assert (rc, n) == (CORRUPT, 0)


# ---- blocks built by hand ------------------------------------------------------

def seq(literals, D=None, M=None):
    """One sequence: the literals, then a match of M at distance D (none: the
    block's last sequence)."""
    L = len(literals)
    if D is None:
        return bytes([min(L, 15) << 4]) + FM.ext(L) + literals
    return (bytes([min(L, 15) << 4 | min(M - 4, 15)]) + FM.ext(L) + literals +
            struct.pack("<H", D) + FM.ext(M - 4))


def apply(out, literals, D=None, M=None):
    out += literals
    for _ in range(M or 0):
        out.append(out[-D])


def frame_of(blocks, linked=False, n=None, bd=0x40):
    """A frame of these blocks' bytes (a bytes object: compressed; a tuple
    ("stored", bytes): stored), with the content size n when given."""
    out = bytearray(FM.header(0x40 | (0 if linked else 0x20) | (0x08 if n is not None else 0), bd, n))
    for b in blocks:
        if isinstance(b, tuple):
            out += struct.pack("<I", len(b[1]) | 0x80000000) + b[1]
        else:
            out += struct.pack("<I", len(b)) + b
    return bytes(out) + b"\0\0\0\0"


# ---- this library's frames -----------------------------------------------------

def own_inputs(text):
    return {"300": text[:300], "301": text[:301], "19199": text[:19199], "19200": text[:19200],
            "19201": text[:19201], "38401": text[:38401], "text": text,
            "random": rnd(40000, 5), "zeros": bytes(40000)}


@pytest.mark.parametrize("name", ["300", "301", "19199", "19200", "19201", "38401", "text",
                                  "random", "zeros"])
def test_own_frames_round_trip(comp, text, name):
    plain = own_inputs(text)[name]
    d_in = torch.from_numpy(np.frombuffer(plain, np.uint8).copy()).cuda()
    d_frame, length = comp.compress_frame_device(d_in)
    # the Python call: no room first, the length it names, then the decode
    d_back, n = lz4.decompress_frame_device(d_frame, length)
    assert n == len(plain) and d_back.numel() == n and torch.equal(d_back, d_in)
    frame = d_frame[:length].cpu().numpy().tobytes()
    if name == "random":                                 # one literal run per data block
        assert frame[19:19 + 4] == b"\xf0\xff\xff\xff"
    decodes_to(frame, plain)
    if name == "301":
        assert lz4.decompress_frame_gpu(frame) == plain


# ---- the model's variants ------------------------------------------------------

@pytest.fixture(scope="module")
def variants(text):
    return FM.variants(text[:20000])


@pytest.mark.parametrize("name", ["independent", "linked", "stored", "checksums",
                                  "no content size", "4 MiB class", "two frames"])
def test_variants(variants, name):
    frame, plain = variants[name]
    decodes_to(frame, plain)
    if name in ("checksums", "two frames"):
        decodes_to(frame, plain, verify=False)


# ---- periodic matches ----------------------------------------------------------

@pytest.mark.parametrize("D", [1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256])
def test_periodic_matches(D):
    """A block per M: D literals, a match of M at distance D, 5 closing
    literals.  M < D, M == D and M > D (several periods, lanes past one wave's
    width) are all among them."""
    blocks, plain = [], bytearray()
    for M in (4, 18, 19, 20, 273, 274, 275, 1000):
        lits, tail = rnd(D, 1000 * D + M), rnd(5, 7 * D + M)
        blocks.append(seq(lits, D, M) + seq(tail))
        apply(plain, lits, D, M)
        apply(plain, tail)
    decodes_to(frame_of(blocks, n=len(plain)), plain)


# ---- the extensions' thresholds ------------------------------------------------

def test_literal_run_lengths():
    """A block per L: a run of L literals before a match, and again as the
    block's final run."""
    blocks, plain = [], bytearray()
    for L in (0, 14, 15, 16, 269, 270, 271, 525):
        head, run, last = rnd(20, L), rnd(L, 100 + L), rnd(L, 200 + L)
        blocks.append(seq(head, 20, 8) + seq(run, L + 8, 6) + seq(last))
        start = len(plain)
        apply(plain, head, 20, 8)
        apply(plain, run, L + 8, 6)
        apply(plain, last)
        assert len(plain) - start == 34 + 2 * L
    decodes_to(frame_of(blocks, n=len(plain)), plain)


# ---- linked frames -------------------------------------------------------------

def test_linked_match_crosses_the_previous_blocks_end():
    a, b = rnd(40, 1), rnd(10, 2)
    plain = bytearray()
    apply(plain, a)
    apply(plain, b, 20, 15)            # source [30, 45): ends in this block's literals
    apply(plain, b"", 25, 30)          # source [40, 65) from 65 on: periodic over the blocks' seam
    apply(plain, b"tail!")
    blocks = [seq(a), seq(b, 20, 15) + seq(b"", 25, 30) + seq(b"tail!")]
    decodes_to(frame_of(blocks, linked=True, n=len(plain)), plain)
    # the same blocks unlinked: the first match reaches before its block
    is_corrupt(frame_of(blocks, n=len(plain)))


def test_linked_match_at_distance_65535():
    first = rnd(65536, 3)
    plain = bytearray(first)
    apply(plain, b"", 65535, 10)
    apply(plain, b"12345")
    frame = frame_of([("stored", first), seq(b"", 65535, 10) + seq(b"12345")], linked=True,
                     n=len(plain))
    decodes_to(frame, plain)


def test_second_frame_cannot_reach_into_the_first():
    a, b = rnd(40, 4), rnd(4, 5)
    first = frame_of([seq(a)], linked=True, n=40)
    plain = bytearray(a)
    apply(plain, b, 4, 8)
    apply(plain, b"12345")
    good = frame_of([seq(b, 4, 8) + seq(b"12345")], linked=True)
    bad = frame_of([seq(b, 5, 8) + seq(b"12345")], linked=True)
    decodes_to(first + good, plain)
    is_corrupt(first + bad)


# ---- many small blocks ---------------------------------------------------------

def write_linked_small(plain, block):
    """FM.write_variant(plain, block, linked=True), byte for byte, for inputs
    below 65,535 bytes: the model rebuilds its hash table over the whole window
    for every block, minutes for 5,000 of them; this keeps one table, which
    holds the same entries (the last position of every four bytes before the
    block)."""
    assert len(plain) < 65535
    out = bytearray(FM.header(0x48, 0x40, len(plain)))
    table = {}
    for lo in range(0, len(plain), block):
        hi = min(lo + block, len(plain))
        body, anchor, p = bytearray(), lo, lo
        while p <= hi - 12:
            key = plain[p:p + 4]
            q = table.get(key)
            table[key] = p
            if q is None:
                p += 1
                continue
            ml = 4
            while p + ml < hi - 5 and plain[q + ml] == plain[p + ml]:
                ml += 1
            body += seq(plain[anchor:p], p - q, ml)
            p += ml
            anchor = p
        body += seq(plain[anchor:hi])
        for q in range(lo, hi):
            table[plain[q:q + 4]] = q
        out += struct.pack("<I", len(body)) + body
    return bytes(out) + b"\0\0\0\0"


def test_many_small_blocks(text):
    """5,000 blocks of 13 bytes: more than one round of the scan and more than
    one window of the walk."""
    plain = text[:65000]
    assert write_linked_small(text[:3000], 13) == FM.write_variant(text[:3000], block=13, linked=True)
    frames = [FM.write_variant(plain, block=13), write_linked_small(plain, 13),
              FM.write_variant(plain, block=13, stored=range(0, 5000, 3))]
    assert frames[1] != frames[0] and len(frames[1]) < len(frames[0])
    for frame in frames:
        decodes_to(frame, plain)


def test_more_blocks_than_the_first_index_holds():
    """6,000 stored blocks of no bytes take 24,000 bytes of input: more than
    the index's first size (in_len / 1024 + 4096 blocks), so the call walks a
    second time into an index of the size the first walk counted.  (The 5,000
    blocks of test_many_small_blocks take that path as well.)"""
    empty = struct.pack("<I", 0x80000000)
    body = rnd(100, 9)
    frame = FM.header(0x60, 0x40) + empty * 6000 + struct.pack("<I", len(seq(body))) + seq(body) + \
        empty * 3 + b"\0\0\0\0"
    decodes_to(frame, body)


# ---- alignment -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["linked", "independent"])
def test_misaligned_pointers(text, name):
    plain = text[1000:1000 + 9000]
    frame = FM.write_variant(plain, block=2048, linked=name == "linked")
    for k in range(16):
        decodes_to(frame, plain, in_off=k, out_off=(5 * k + 3) % 16)


# ---- capacity ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["own", "linked"])
def test_capacity(comp, text, name):
    plain = text[:30000]
    frame = comp.compress_frame(plain) if name == "own" else \
        FM.write_variant(plain, linked=True, content_checksum=True)
    n = len(plain)
    for cap in (0, n - 1):
        assert host(frame, cap)[0] == CAPACITY
        rc, need, out = device(frame, cap)
        assert (rc, need) == (CAPACITY, n)
        assert (out == FILL).all(), "written without room for the whole output"
    rc, got, out = device(frame, n)
    assert (rc, got) == (OK, n) and out.tobytes() == plain
    d_frame = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).cuda()
    with pytest.raises(lz4.Lz4Error) as e:
        lz4.decompress_frame_device(d_frame, cap=n - 1)
    assert e.value.code == CAPACITY
    d_out = torch.empty(n + 7, dtype=torch.uint8, device="cuda")
    back, got = lz4.decompress_frame_device(d_frame, d_out=d_out)
    assert back is d_out and got == n and d_out[:n].cpu().numpy().tobytes() == plain


def test_what_only_a_decode_finds_needs_the_room(text):
    """A match distance beyond its window and a wrong content checksum are
    found by decoding: with too little room the call answers with the exact
    length and writes nothing (include/lz4r.h), with that room it is corrupt.
    (The host decoder, which decodes as far as the room goes, may say corrupt
    in the first case already.)"""
    lits = rnd(20, 12)
    far = frame_of([seq(lits, 21, 8) + seq(b"12345")])
    plain = text[:5000]
    sums = bytearray(FM.write_variant(plain, block=2048, content_checksum=True))
    sums[-1] ^= 1
    for frame, n in ((far, 33), (bytes(sums), len(plain))):
        for cap in (0, n - 1):
            rc, need, out = device(frame, cap)
            assert (rc, need) == (CAPACITY, n)
            assert (out == FILL).all()
        is_corrupt(frame, cap=n)


# ---- malformed frames ----------------------------------------------------------

def test_malformed_frames(text):
    plain = text[:5000]
    n = len(plain)
    sums = FM.write_variant(plain, block=2048, block_checksum=True, content_checksum=True)
    decodes_to(sums, plain)

    def flipped(frame, at):
        b = bytearray(frame)
        b[at] ^= 0x10
        return bytes(b)

    is_corrupt(flipped(sums, 14))                        # the header checksum
    first = struct.unpack_from("<I", sums, 15)[0]
    is_corrupt(flipped(sums, 19 + first + 2))            # the first block's checksum
    is_corrupt(flipped(sums, 19 + 5))                    # ... or a byte that it covers
    wrong = flipped(sums, len(sums) - 1)                 # the content checksum
    is_corrupt(wrong)
    decodes_to(wrong, plain, verify=False, host_too=False)   # (the host decoder always looks)
    with pytest.raises(lz4.Lz4Error) as e:
        lz4.decompress_frame_gpu(wrong)
    assert e.value.code == CORRUPT
    assert lz4.decompress_frame_gpu(wrong, verify_content=False) == plain

    body = FM.write_variant(plain)[15:]
    is_corrupt(FM.header(0x68, 0x40, n + 1) + body)      # a content size off by one
    is_corrupt(FM.header(0x68, 0x40, n - 1) + body)
    decodes_to(FM.header(0x68, 0x40, n) + body, plain)
    big = rnd(65537, 11)
    is_corrupt(frame_of([("stored", big)]), cap=1 << 17)  # beyond the 64 KiB block maximum
    decodes_to(frame_of([("stored", big)], bd=0x50), big)
    good = FM.write_variant(plain)
    is_corrupt(good[:-2])                                # a truncated EndMark
    is_corrupt(good[:-4])
    is_corrupt(good + b"\0")                             # a byte after the last frame

    lits = rnd(20, 12)
    decodes_to(frame_of([seq(lits, 20, 8) + seq(b"12345")]), lits + lits[:8] + b"12345")
    is_corrupt(frame_of([seq(lits, 0, 8) + seq(b"12345")]))          # D == 0
    is_corrupt(frame_of([seq(lits, 21, 8) + seq(b"12345")]))         # D one beyond the base
    is_corrupt(frame_of([seq(lits, 20, 8)]))                         # a block ending in a match
    is_corrupt(frame_of([seq(lits, 20, 8) + b"\xf0\xff\xff"]))       # an extension off the block
    is_corrupt(frame_of([seq(lits, 20, 8) + b"\x1f" + b"x" + b"\x01\x00\xff"]))
    is_corrupt(frame_of([seq(lits, 20, 8) + b"\x50123"]))            # literals past the block
    is_corrupt(frame_of([seq(lits, 20, 8) + b"\x10x\x01"]))          # one byte left for a distance

    is_corrupt(struct.pack("<II", 0x184D2A50, 4) + b"skip" + good)   # a skippable frame
    is_corrupt(struct.pack("<II", 0x184C2102, 8) + b"\x80legacy!")   # a legacy frame
    d = bytes([0x61, 0x40]) + struct.pack("<I", 7)                   # a dictionary ID
    is_corrupt(FM.MAGIC + d + bytes([(FM.xxh32(d) >> 8) & 0xFF]) + good[7 + 8:])
    is_corrupt(FM.header(0x6A, 0x40, n) + body)                      # a reserved bit
    is_corrupt(b"")                                                  # the empty input
