"""The standard LZ4 frame the library writes (include/lz4r.h, csrc/lz4r_frame.h)
restated in plain Python (a helper, no tests, no GPU, nothing from the
package): xxh32, the expected frame of an input from the oracle's native
stream, a strict frame decoder, and writers of variant frames for the host
decoder.

  frame       04 22 4D 18 | FLG 0x68 | BD 0x40 | u64 n | HC | data block* | 00 00 00 00
  data block  u32 size | the sequences of 64 source blocks (19,200 input bytes)
Sequences of a data block of N input bytes, from its source blocks' records:
  1  a record with M < 4 is literals        2  a match starting after N - 12 is literals
  3  a match ending after N - 5 is cut      4  literal runs merge
  5  token, literal extension, literals, u16 distance, match extension
  6  the last sequence has no match
"""
import ctypes
import ctypes.util
import struct

import lz4_format
import lz4_seq_inputs

BLK = 300
GROUP = 64 * BLK                  # input bytes of a data block
MAGIC = b"\x04\x22\x4d\x18"
M32 = 0xFFFFFFFF
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


class FrameError(ValueError):
    pass


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def xxh32(data, seed=0):
    data = bytes(data)
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M32, (seed + P2) & M32, seed, (seed - P1) & M32]
        while i + 16 <= n:
            for j, w in enumerate(struct.unpack_from("<4I", data, i)):
                v[j] = (_rotl((v[j] + w * P2) & M32, 13) * P1) & M32
            i += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M32
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while i + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, i)[0] * P3) & M32, 17) * P4) & M32
        i += 4
    while i < n:
        h = (_rotl((h + data[i] * P5) & M32, 11) * P1) & M32
        i += 1
    h ^= h >> 15
    h = (h * P2) & M32
    h ^= h >> 13
    h = (h * P3) & M32
    return h ^ (h >> 16)


def ext(x):
    """x >= 15 as a length extension: x - 15 in 255-bytes and a final byte."""
    if x < 15:
        return b""
    q, r = divmod(x - 15, 255)
    return b"\xff" * q + bytes([r])


def header(flg, bd, content_size=None):
    d = bytes([flg, bd]) + (struct.pack("<Q", content_size) if content_size is not None else b"")
    return MAGIC + d + bytes([(xxh32(d) >> 8) & 0xFF])


def frame_bound(n):
    return 19 + n + 100 * ((n + GROUP - 1) // GROUP)


# ---- the expected frame --------------------------------------------------------

def kept_matches(block_seqs, N):
    """Rules 1-3 over a data block's source blocks' sequence lists ((L, D, M)
    per sequence, lz4_format.parse): the kept matches as (start, ML, D)."""
    kept = []
    for b, seqs in enumerate(block_seqs):
        pos = BLK * b
        for L, D, M in seqs:
            start = pos + L
            pos = start + M
            if M >= 4 and start <= N - 12:
                kept.append((start, min(pos, N - 5) - start, D))
    return kept


def block_of(plain, kept):
    """Rules 4-6: (the data block's bytes, the literal length of every
    sequence, the last one's included)."""
    out, runs, prev = bytearray(), [], 0
    for start, ML, D in kept:
        L = start - prev
        runs.append(L)
        out += bytes([min(L, 15) << 4 | min(ML - 4, 15)]) + ext(L) + plain[prev:start]
        out += struct.pack("<H", D) + ext(ML - 4)
        prev = start + ML
    L = len(plain) - prev
    runs.append(L)
    out += bytes([min(L, 15) << 4]) + ext(L) + plain[prev:]
    return bytes(out), runs


def frame_parts(plain, native_stream, offsets):
    """(frame bytes, per data block the literal lengths of its sequences)."""
    plain = bytes(plain)
    seqs = [r for _, r in lz4_format.parse(native_stream, list(offsets))]
    assert len(seqs) == (len(plain) + BLK - 1) // BLK
    out, runs = bytearray(header(0x68, 0x40, len(plain))), []
    for g in range(0, len(seqs), 64):
        data = plain[BLK * g:BLK * (g + 64)]
        body, r = block_of(data, kept_matches(seqs[g:g + 64], len(data)))
        out += struct.pack("<I", len(body)) + body
        runs.append(r)
    return bytes(out) + b"\0\0\0\0", runs


def frame_of(plain, native_stream, offsets):
    return frame_parts(plain, native_stream, offsets)[0]


def expected(oracle, plain):
    """frame_parts of the oracle's native stream of `plain`."""
    exp = lz4_seq_inputs.Expected(oracle, plain)
    return frame_parts(plain, exp.framed(), [int(o) for o in exp.offsets()])


# ---- a strict decoder ----------------------------------------------------------

def _read_ext(b, ip, end):
    """(value added, next ip) of a length extension; minimal by construction
    (a byte below 255 ends it), so only truncation can be wrong."""
    v = 0
    while True:
        if ip >= end:
            raise FrameError("extension past the block end")
        x = b[ip]
        ip += 1
        v += x
        if x != 255:
            return v, ip


def decode_block_strict(b, history=b"", bmax=65536):
    """One compressed block -> its bytes; matches may reach into `history`
    (a linked block's window).  Rejects what a conforming writer
    never emits: a match that reaches into the last 5 bytes, a last match
    starting after N - 12, a length whose extension is not minimal (a token
    nibble below 15 with an extension cannot be written; a nibble of 15
    always has one), a block that does not end with a literal run."""
    out = bytearray(history)
    base = len(history)
    ip, end, matches = 0, len(b), []
    while True:
        if ip >= end:
            raise FrameError("no last literal run")
        tok = b[ip]
        ip += 1
        L = tok >> 4
        if L == 15:
            a, ip = _read_ext(b, ip, end)
            L += a
        if ip + L > end:
            raise FrameError("literal run past the block end")
        out += b[ip:ip + L]
        ip += L
        if ip == end:
            if tok & 15:
                raise FrameError("match nibble in the last token")
            break
        if ip + 2 > end:
            raise FrameError("truncated distance")
        D = b[ip] | b[ip + 1] << 8
        ip += 2
        ML = (tok & 15) + 4
        if tok & 15 == 15:
            a, ip = _read_ext(b, ip, end)
            ML += a
        if D == 0 or D > len(out):
            raise FrameError("distance before the window")
        matches.append((len(out) - base, ML))
        for _ in range(ML):
            out.append(out[-D])
    N = len(out) - base
    if N > bmax:
        raise FrameError("block over the frame's block maximum (64 KiB in the library's frames)")
    for start, ML in matches:
        if start + ML > N - 5:
            raise FrameError("match reaches into the last 5 bytes")
        if start > N - 12:
            raise FrameError("match starts after N - 12")
    return bytes(out[base:])


def decode_strict(frame):
    """Frames (one or several) -> bytes, everything checked."""
    frame = bytes(frame)
    ip, out = 0, bytearray()
    if not frame:
        raise FrameError("empty")
    while ip < len(frame):
        if frame[ip:ip + 4] != MAGIC or ip + 7 > len(frame):
            raise FrameError("magic")
        flg, bd = frame[ip + 4], frame[ip + 5]
        if flg >> 6 != 1 or flg & 3 or bd & 0x8F or bd >> 4 < 4:
            raise FrameError("descriptor")
        indep, bsum, csize, csum = flg & 0x20, flg & 0x10, flg & 0x08, flg & 0x04
        bmax = 1 << (8 + 2 * (bd >> 4))
        dlen = 2 + (8 if csize else 0)
        if ip + 4 + dlen + 1 > len(frame):
            raise FrameError("truncated descriptor")
        d = frame[ip + 4:ip + 4 + dlen]
        if frame[ip + 4 + dlen] != (xxh32(d) >> 8) & 0xFF:
            raise FrameError("header checksum")
        want = struct.unpack("<Q", d[2:])[0] if csize else None
        ip += 4 + dlen + 1
        fstart = len(out)
        while True:
            if ip + 4 > len(frame):
                raise FrameError("truncated block size")
            word = struct.unpack_from("<I", frame, ip)[0]
            ip += 4
            if word == 0:
                break
            size = word & 0x7FFFFFFF
            if size > bmax or ip + size + (4 if bsum else 0) > len(frame):
                raise FrameError("block size")
            body = frame[ip:ip + size]
            ip += size
            if bsum:
                if struct.unpack_from("<I", frame, ip)[0] != xxh32(body):
                    raise FrameError("block checksum")
                ip += 4
            if word >> 31:
                out += body
            else:
                hist = b"" if indep else bytes(out[fstart:][-65535:])
                out += decode_block_strict(body, hist, bmax)
        if want is not None and want != len(out) - fstart:
            raise FrameError("content size")
        if csum:
            if ip + 4 > len(frame) or struct.unpack_from("<I", frame, ip)[0] != xxh32(out[fstart:]):
                raise FrameError("content checksum")
            ip += 4
    return bytes(out)


# ---- writers of variant frames -------------------------------------------------

def compress_block(data, lo, hi, window_lo):
    """A conforming block of data[lo:hi], greedy over a 4-byte hash, matches
    reaching back to data[window_lo] (window_lo = lo: independent)."""
    N = hi - lo
    table, out, anchor, p = {}, bytearray(), lo, lo
    if window_lo < lo:
        for q in range(max(window_lo, lo - 65535), lo):
            table[data[q:q + 4]] = q
    while p <= hi - 12:
        key = data[p:p + 4]
        q = table.get(key)
        table[key] = p
        if q is None or p - q > 65535 or q < window_lo:
            p += 1
            continue
        ml = 4
        while p + ml < hi - 5 and data[q + ml] == data[p + ml]:
            ml += 1
        L = p - anchor
        out += bytes([min(L, 15) << 4 | min(ml - 4, 15)]) + ext(L) + data[anchor:p]
        out += struct.pack("<H", p - q) + ext(ml - 4)
        p += ml
        anchor = p
    L = hi - anchor
    out += bytes([min(L, 15) << 4]) + ext(L) + data[anchor:hi]
    assert N == 0 or out
    return bytes(out)


def write_variant(plain, block=4096, linked=False, stored=(), block_checksum=False,
                  content_checksum=False, content_size=True, bd=0x40):
    """A frame of `plain` in blocks of `block` bytes; `stored`: the indices of
    blocks kept uncompressed (high bit set)."""
    plain = bytes(plain)
    flg = 0x40 | (0 if linked else 0x20) | (0x10 if block_checksum else 0) | \
        (0x08 if content_size else 0) | (0x04 if content_checksum else 0)
    out = bytearray(header(flg, bd, len(plain) if content_size else None))
    for i, lo in enumerate(range(0, len(plain), block)):
        hi = min(lo + block, len(plain))
        if i in stored:
            body, word = plain[lo:hi], (hi - lo) | 0x80000000
        else:
            body = compress_block(plain, lo, hi, 0 if linked else lo)
            word = len(body)
        out += struct.pack("<I", word) + body
        if block_checksum:
            out += struct.pack("<I", xxh32(body))
    out += b"\0\0\0\0"
    if content_checksum:
        out += struct.pack("<I", xxh32(plain))
    return bytes(out)


def variants(plain):
    """{name: (frame, what it decodes to)}"""
    return {
        "independent": (write_variant(plain), plain),
        "linked": (write_variant(plain, linked=True), plain),
        "stored": (write_variant(plain, stored=(0, 2)), plain),
        "checksums": (write_variant(plain, linked=True, block_checksum=True,
                                    content_checksum=True), plain),
        "no content size": (write_variant(plain, content_size=False), plain),
        "4 MiB class": (write_variant(plain, block=70000, bd=0x70), plain),
        "two frames": (write_variant(plain[:5000], linked=True) +
                       write_variant(plain[5000:], content_checksum=True), plain),
    }


# ---- the system's liblz4, when there is one ---------------------------------------

class _FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int),
                ("contentChecksumFlag", ctypes.c_int), ("frameType", ctypes.c_int),
                ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class _Prefs(ctypes.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", ctypes.c_int),
                ("autoFlush", ctypes.c_uint), ("favorDecSpeed", ctypes.c_uint),
                ("reserved", ctypes.c_uint * 3)]


def system_liblz4():
    """The system's liblz4 with the frame API bound, or None."""
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    L = ctypes.CDLL(name)
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    L.LZ4F_isError.argtypes = [sz]
    L.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(vp), ctypes.c_uint]
    L.LZ4F_createDecompressionContext.restype = sz
    L.LZ4F_freeDecompressionContext.argtypes = [vp]
    L.LZ4F_decompress.argtypes = [vp, vp, ctypes.POINTER(sz), vp, ctypes.POINTER(sz), vp]
    L.LZ4F_decompress.restype = sz
    L.LZ4F_compressFrameBound.argtypes = [sz, ctypes.POINTER(_Prefs)]
    L.LZ4F_compressFrameBound.restype = sz
    L.LZ4F_compressFrame.argtypes = [vp, sz, vp, sz, ctypes.POINTER(_Prefs)]
    L.LZ4F_compressFrame.restype = sz
    return L


def liblz4_decompress(L, frame, cap):
    """(decoded bytes, frame bytes consumed, the decoder's last return value:
    0 when the frame ended exactly)."""
    sz = ctypes.c_size_t
    ctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    src = ctypes.create_string_buffer(bytes(frame), len(frame))
    dst = ctypes.create_string_buffer(max(cap, 1))
    ip = op = 0
    ret = 1
    try:
        while ip < len(frame) and ret != 0:
            dn, sn = sz(cap - op), sz(len(frame) - ip)
            ret = L.LZ4F_decompress(ctx, ctypes.byref(dst, op), ctypes.byref(dn),
                                    ctypes.byref(src, ip), ctypes.byref(sn), None)
            if L.LZ4F_isError(ret):
                raise FrameError(f"LZ4F_decompress error {ret - (1 << 64)}")
            if dn.value == 0 and sn.value == 0:
                break
            op += dn.value
            ip += sn.value
    finally:
        L.LZ4F_freeDecompressionContext(ctx)
    return dst.raw[:op], ip, ret


def liblz4_compress(L, plain, linked=True, checksums=True, level=0):
    p = _Prefs()
    p.frameInfo.blockSizeID = 4                      # 64 KiB
    p.frameInfo.blockMode = 0 if linked else 1
    p.frameInfo.contentChecksumFlag = 1 if checksums else 0
    p.frameInfo.blockChecksumFlag = 1 if checksums else 0
    p.frameInfo.contentSize = len(plain)
    p.compressionLevel = level
    cap = L.LZ4F_compressFrameBound(len(plain), ctypes.byref(p))
    dst = ctypes.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(dst, cap, bytes(plain), len(plain), ctypes.byref(p))
    assert not L.LZ4F_isError(n)
    return dst.raw[:n]
