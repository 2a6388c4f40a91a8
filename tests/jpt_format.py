"""The JPT1 stream (include/jpegr.h) restated in plain Python beside
jpr_format.py: JPR1's header, index and record order, each stream's table in
one of three codings.  No GPU, no torch; the arrays are entropy_inputs.pack's.

  header   16 B   'J' 'P' 'T' '1' | u32 w | u32 h | u32 nimg
  index    2 B x ntiles   u16 size of each tile record
  records  per tile stream(Y) stream(Cr) stream(Cb)
  stream   u8 rle_len | u8 ncodes | u16 f      nbits = f & 0x3FFF, mode = f >> 14
           table by mode
             0  ncodes x { i16 value, u8 code_length }
             1  ceil(ncodes / 2) length bytes (entry k: low nibble of byte
                k / 2 for even k, high nibble for odd k), ncodes x i8 value
             2  the same length bytes, ncodes x i16 value
             3  malformed
           ceil(nbits / 8) bytes of bits
"""
import struct

import numpy as np

from jpr_format import (OK, RECORD_MAX, SLOT_BITS, SLOT_CODES, SLOT_OFF, fields, live_equal,  # noqa: F401
                        ntiles_of)

MAGIC = b"JPT1"


def entries(table_row, m, c):
    """[(value, length)] of a stream's live table words; meta fields past the
    slot are clamped first."""
    ncodes = min(fields(m)[2], SLOT_CODES[c])
    o = SLOT_OFF[c]
    return [(int((e & 0xFFFF) ^ 0x8000) - 0x8000, (e >> 16) & 255)
            for e in table_row[o:o + ncodes].tolist()]


def canonical_mode(ents):
    """The writer's mode: 1 when there are entries, every length is <= 15 and
    every value fits an i8; else 2 when there are entries and every length is
    <= 15; else 0."""
    if not ents or any(L > 15 for _, L in ents):
        return 0
    return 1 if all(-128 <= v <= 127 for v, _ in ents) else 2


def mode_legal(ents, mode):
    if mode == 0:
        return True
    if any(L > 15 for _, L in ents):
        return False
    return mode == 2 or all(-128 <= v <= 127 for v, _ in ents)


def table_bytes(ncodes, mode):
    return 3 * ncodes if mode == 0 else (ncodes + 1) // 2 + mode * ncodes


def pack_stream(bits_row, m, table_row, c, mode=None):
    nbits, rle_len, _ = fields(m)
    nbits = min(nbits, SLOT_BITS[c])
    ents = entries(table_row, m, c)
    if mode is None:
        mode = canonical_mode(ents)
    assert mode_legal(ents, mode), (c, mode)
    out = bytearray(struct.pack("<BBH", rle_len, len(ents), nbits | mode << 14))
    if mode == 0:
        for v, L in ents:
            out += struct.pack("<hB", v, L)
    else:
        lens = [L for _, L in ents] + [0]
        out += bytes(lens[k] | lens[k + 1] << 4 for k in range(0, len(ents), 2))
        out += b"".join(struct.pack("<b" if mode == 1 else "<h", v) for v, _ in ents)
    o = SLOT_OFF[c]
    out += bits_row[o:o + (nbits + 7) // 8].tobytes()
    return bytes(out)


def pack(bits, meta, table, w, h, nimg, modes=None):
    """The JPT1 stream of the slot arrays: canonical modes, or modes[t][c]
    (None = canonical) forced per stream for crafted streams."""
    nt = ntiles_of(w, h, nimg)
    bits = np.asarray(bits, np.uint8).reshape(nt, 256)
    meta = np.asarray(meta).astype(np.uint32).reshape(nt, 3)
    table = np.asarray(table).astype(np.uint32).reshape(nt, 256)
    recs = [b"".join(pack_stream(bits[t], meta[t, c], table[t], c,
                                 None if modes is None else modes[t][c]) for c in range(3))
            for t in range(nt)]
    assert all(len(r) <= RECORD_MAX for r in recs)
    return (MAGIC + struct.pack("<III", w, h, nimg) +
            b"".join(struct.pack("<H", len(r)) for r in recs) + b"".join(recs))


def stream_modes(bits, meta, table):
    """[nt, 3] canonical modes of the slot arrays."""
    meta = np.asarray(meta).astype(np.uint32).reshape(-1, 3)
    table = np.asarray(table).astype(np.uint32).reshape(-1, 256)
    return np.array([[canonical_mode(entries(table[t], meta[t, c], c)) for c in range(3)]
                     for t in range(meta.shape[0])], np.int64).reshape(-1, 3)


def header(data):
    """(w, h, nimg), or None on a wrong magic or a zero dimension."""
    if len(data) < 16 or data[:4] != MAGIC:
        return None
    w, h, nimg = struct.unpack("<III", data[4:16])
    return (w, h, nimg) if w and h and nimg else None


def parse_record(rec):
    """[(meta word, table words, bit bytes, mode)] x 3, or None if malformed."""
    out, p = [], 0
    for c in range(3):
        if p + 4 > len(rec):
            return None
        rle_len, ncodes, f = struct.unpack("<BBH", rec[p:p + 4])
        nbits, mode = f & 0x3FFF, f >> 14
        if mode == 3 or rle_len > SLOT_CODES[c] or ncodes > SLOT_CODES[c] or nbits > SLOT_BITS[c]:
            return None
        nby, tby = (nbits + 7) // 8, table_bytes(ncodes, mode)
        if p + 4 + tby + nby > len(rec):
            return None
        tab = rec[p + 4:p + 4 + tby]
        if mode == 0:
            ents = [v | L << 16 for v, L in struct.iter_unpack("<HB", tab)]
        else:
            nlb = (ncodes + 1) // 2
            lens = [(tab[k // 2] >> (4 * (k & 1))) & 15 for k in range(ncodes)]
            vals = [x[0] & 0xFFFF for x in struct.iter_unpack("<b" if mode == 1 else "<h", tab[nlb:])]
            ents = [v | L << 16 for v, L in zip(vals, lens)]
        out.append((nbits | rle_len << 16 | ncodes << 24, ents, rec[p + 4 + tby:p + 4 + tby + nby], mode))
        p += 4 + tby + nby
    return out if p == len(rec) else None


def parse(data, dims=None):
    """(records, implied, verdict): records[t] = parse_record's list or None
    (malformed, or the header or index wrong); the length the header and
    index imply; d_result[1]'s verdict as jpr_format.unpack states it."""
    data = bytes(data)
    hd = header(data)
    w, h, nimg = dims if dims is not None else (hd or (0, 0, 0))
    nt = ntiles_of(w, h, nimg)
    idx_end = 16 + 2 * nt
    sizes = [int.from_bytes(data[16 + 2 * t:18 + 2 * t], "little") for t in range(nt)]
    implied = idx_end + sum(sizes)
    if hd != (w, h, nimg) or nt == 0 or len(data) < idx_end or implied != len(data):
        return [None] * nt, implied, 0
    verdict, off, recs = OK, idx_end, []
    for t, size in enumerate(sizes):
        rec = parse_record(data[off:off + size]) if size <= RECORD_MAX else None
        off += size
        if rec is None:
            verdict = min(verdict, 1 + t)
        recs.append(rec)
    return recs, implied, verdict


def unpack(data, dims=None, fill=0):
    """jpr_format.unpack for a JPT1 stream: (bits, meta, table, implied,
    verdict)."""
    recs, implied, verdict = parse(data, dims)
    nt = len(recs)
    bits = np.full((nt, 256), fill, np.uint8)
    meta = np.zeros((nt, 3), np.uint32)
    table = np.full((nt, 256), fill * 0x01010101, np.uint32)
    for t, rec in enumerate(recs):
        if rec is None:
            continue
        for c, (m, ents, raw, _) in enumerate(rec):
            o = SLOT_OFF[c]
            meta[t, c] = m
            table[t, o:o + len(ents)] = ents
            bits[t, o:o + len(raw)] = np.frombuffer(raw, np.uint8)
    return bits, meta, table, implied, verdict
