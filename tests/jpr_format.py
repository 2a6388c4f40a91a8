"""The JPR stream (include/jpegr.h) restated in plain Python: no GPU, no
torch.  pack() and unpack() work on the arrays entropy_inputs.pack returns
(bits [nt, 256] u8, meta [nt, 3] u32, table [nt, 256] u32).

  header   16 B   'J' 'P' 'R' '1' | u32 w | u32 h | u32 nimg
  index    2 B x ntiles   u16 size of each tile record
  records  per tile stream(Y) stream(Cr) stream(Cb)
  stream   u8 rle_len | u8 ncodes | u16 nbits
           ncodes x { i16 value, u8 code_length }
           ceil(nbits / 8) bytes of bits
"""
import struct

import numpy as np

MAGIC = b"JPR1"
SLOT_OFF = (0, 128, 192)              # bytes of a tile's bits, entries of its table
SLOT_CODES = (128, 64, 64)            # table entries = the most RLE ints
SLOT_BITS = (1024, 512, 512)
RECORD_MAX = sum(4 + 3 * n + b // 8 for n, b in zip(SLOT_CODES, SLOT_BITS))     # 1036
OK = (1 << 64) - 1                    # d_result[1] of a consistent stream


def ntiles_of(w, h, nimg):
    return nimg * ((w + 7) // 8) * ((h + 7) // 8)


def fields(m):
    """(nbits, rle_len, ncodes) of a meta word."""
    m = int(m)
    return m & 0xFFFF, (m >> 16) & 255, m >> 24


def pack_stream(bits_row, m, table_row, c):
    nbits, rle_len, ncodes = fields(m)
    assert ncodes <= SLOT_CODES[c] and nbits <= SLOT_BITS[c], (c, ncodes, nbits)
    o = SLOT_OFF[c]
    out = bytearray(struct.pack("<BBH", rle_len, ncodes, nbits))
    for e in table_row[o:o + ncodes].tolist():
        out += struct.pack("<HB", e & 0xFFFF, (e >> 16) & 255)
    out += bits_row[o:o + (nbits + 7) // 8].tobytes()
    return bytes(out)


def pack(bits, meta, table, w, h, nimg):
    nt = ntiles_of(w, h, nimg)
    bits = np.asarray(bits, np.uint8).reshape(nt, 256)
    meta = np.asarray(meta).astype(np.uint32).reshape(nt, 3)
    table = np.asarray(table).astype(np.uint32).reshape(nt, 256)
    recs = [b"".join(pack_stream(bits[t], meta[t, c], table[t], c) for c in range(3))
            for t in range(nt)]
    assert all(len(r) <= RECORD_MAX for r in recs)
    return (MAGIC + struct.pack("<III", w, h, nimg) +
            b"".join(struct.pack("<H", len(r)) for r in recs) + b"".join(recs))


def header(data):
    """(w, h, nimg), or None on a wrong magic or a zero dimension."""
    if len(data) < 16 or data[:4] != MAGIC:
        return None
    w, h, nimg = struct.unpack("<III", data[4:16])
    return (w, h, nimg) if w and h and nimg else None


def _parse_record(rec):
    """[(meta word, table entries, bit bytes)] x 3, or None if malformed."""
    out, p = [], 0
    for c in range(3):
        if p + 4 > len(rec):
            return None
        rle_len, ncodes, nbits = struct.unpack("<BBH", rec[p:p + 4])
        if rle_len > SLOT_CODES[c] or ncodes > SLOT_CODES[c] or nbits > SLOT_BITS[c]:
            return None
        nby = (nbits + 7) // 8
        if p + 4 + 3 * ncodes + nby > len(rec):
            return None
        ents = [v | L << 16 for v, L in struct.iter_unpack("<HB", rec[p + 4:p + 4 + 3 * ncodes])]
        out.append((nbits | rle_len << 16 | ncodes << 24, ents,
                    rec[p + 4 + 3 * ncodes:p + 4 + 3 * ncodes + nby]))
        p += 4 + 3 * ncodes + nby
    return out if p == len(rec) else None


def unpack(data, dims=None, fill=0):
    """(bits, meta, table, implied, verdict): the slot arrays (bytes and
    entries that the stream does not hold are `fill`; a malformed tile's meta
    is 0), the length the header and index imply, and d_result[1]'s verdict:
    OK, 0 (header or index wrong; dims = the (w, h, nimg) the caller expects,
    the header's own when None) or 1 + the first malformed tile."""
    data = bytes(data)
    hd = header(data)
    w, h, nimg = dims if dims is not None else (hd or (0, 0, 0))
    nt = ntiles_of(w, h, nimg)
    bits = np.full((nt, 256), fill, np.uint8)
    meta = np.zeros((nt, 3), np.uint32)
    table = np.full((nt, 256), fill * 0x01010101, np.uint32)
    idx_end = 16 + 2 * nt
    sizes = [int.from_bytes(data[16 + 2 * t:18 + 2 * t], "little") for t in range(nt)]
    implied = idx_end + sum(sizes)
    if hd != (w, h, nimg) or nt == 0 or len(data) < idx_end or implied != len(data):
        return bits, meta, table, implied, 0
    verdict, off = OK, idx_end
    for t, size in enumerate(sizes):
        rec = _parse_record(data[off:off + size]) if size <= RECORD_MAX else None
        off += size
        if rec is None:
            verdict = min(verdict, 1 + t)
            continue
        for c, (m, ents, raw) in enumerate(rec):
            o = SLOT_OFF[c]
            meta[t, c] = m
            table[t, o:o + len(ents)] = ents
            bits[t, o:o + len(raw)] = np.frombuffer(raw, np.uint8)
    return bits, meta, table, implied, verdict


def live_equal(a, b):
    """Two (bits, meta, table) triples agree on meta, on the ncodes table
    entries and on the ceil(nbits / 8) bit bytes of every stream.  Returns the
    first difference as a string, or None."""
    (ab, am, at), (bb, bm, bt) = a, b
    am = np.asarray(am).astype(np.uint32).reshape(-1, 3)
    bm = np.asarray(bm).astype(np.uint32).reshape(-1, 3)
    if am.shape != bm.shape or not np.array_equal(am, bm):
        t = np.argwhere(am != bm)[0] if am.shape == bm.shape else None
        return f"meta differs at {t}"
    nt = am.shape[0]
    ab, bb = np.asarray(ab, np.uint8).reshape(nt, 256), np.asarray(bb, np.uint8).reshape(nt, 256)
    at = np.asarray(at).astype(np.uint32).reshape(nt, 256)
    bt = np.asarray(bt).astype(np.uint32).reshape(nt, 256)
    col = np.arange(256)
    for c in range(3):
        o, cap = SLOT_OFF[c], SLOT_CODES[c]
        nbits, ncodes = am[:, c] & 0xFFFF, am[:, c] >> 24
        k = col[None, o:o + cap] - o
        live_t = k < ncodes[:, None]
        if np.any((at[:, o:o + cap] != bt[:, o:o + cap]) & live_t):
            t = int(np.argwhere((at[:, o:o + cap] != bt[:, o:o + cap]) & live_t)[0][0])
            return f"table differs: tile {t}, channel {c}"
        live_b = k < ((nbits + 7) // 8)[:, None]
        if np.any((ab[:, o:o + cap] != bb[:, o:o + cap]) & live_b):
            t = int(np.argwhere((ab[:, o:o + cap] != bb[:, o:o + cap]) & live_b)[0][0])
            return f"bits differ: tile {t}, channel {c}"
    return None
