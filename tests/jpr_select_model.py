"""jpegr_select_device (include/jpegr.h) restated in plain Python over
jpr_format.py and jpt_format.py: which items are bad, which source tile an
output tile is, the empty record, the two re-codings and the result words.  No
GPU, no torch (a helper, no tests; checked by test_jpr_select_model.py).

An item is (image, x, y), unsigned 64-bit each; offs are the ntiles + 1 tile
offsets the caller hands in, which are not trusted.
"""
import struct

import jpr_format as J
import jpt_format as T

U64 = (1 << 64) - 1
EMPTY = bytes(12)                        # three streams with ncodes = 0
JPR1, JPT1 = 1, 2                        # JPEGR_STREAM_*
MAGIC = {JPR1: J.MAGIC, JPT1: T.MAGIC}


def source_format(data, dims):
    """JPR1 or JPT1 when data starts with that header for dims, else 0."""
    if len(data) < 16 or tuple(struct.unpack("<III", data[4:16])) != tuple(dims):
        return 0
    return {J.MAGIC: JPR1, T.MAGIC: JPT1}.get(bytes(data[:4]), 0)


def item_ok(item, dims, out_w, out_h):
    image, x, y = item
    w, h, nimg = dims
    return image < nimg and x % 8 == 0 and y % 8 == 0 and x <= w - out_w and y <= h - out_h


def source_tiles(item, dims, out_w, out_h):
    """The source tiles of a good item's output tiles, in the output's order."""
    image, x, y = item
    w, h, _ = dims
    gw, gh = (w + 7) // 8, (h + 7) // 8
    return [image * gw * gh + (y // 8 + oy) * gw + x // 8 + ox
            for oy in range((out_h + 7) // 8) for ox in range((out_w + 7) // 8)]


def offsets_ok(offs, t, in_len):
    a, b = int(offs[t]) & U64, int(offs[t + 1]) & U64
    return a <= b <= in_len and 12 <= b - a <= J.RECORD_MAX


def _tight_stream(m, ents):
    """A stream's header and table in the canonical mode: (bytes, mode)."""
    nbits, rle_len, ncodes = J.fields(m)
    pairs = [(int((e & 0xFFFF) ^ 0x8000) - 0x8000, (e >> 16) & 255) for e in ents]
    mode = T.canonical_mode(pairs)
    out = bytearray(struct.pack("<BBH", rle_len, ncodes, nbits | mode << 14))
    if mode == 0:
        for v, L in pairs:
            out += struct.pack("<hB", v, L)
    else:
        lens = [L for _, L in pairs] + [0]
        out += bytes(lens[k] | lens[k + 1] << 4 for k in range(0, ncodes, 2))
        out += b"".join(struct.pack("<b" if mode == 1 else "<h", v) for v, _ in pairs)
    return bytes(out), mode


def to_tight(rec):
    """A JPR1 record in JPT1's canonical modes, or None if the record rules
    reject it.  Also the modes it used."""
    parsed = J._parse_record(rec)
    if parsed is None:
        return None, None
    out, modes = b"", []
    for m, ents, raw in parsed:
        head, mode = _tight_stream(m, ents)
        out += head + bytes(raw)
        modes.append(mode)
    return out, modes


def to_plain(rec):
    """A JPT1 record as a JPR1 record, or None if the record rules reject it."""
    parsed = T.parse_record(rec)
    if parsed is None:
        return None
    out = b""
    for m, ents, raw, _ in parsed:
        nbits, rle_len, ncodes = J.fields(m)
        out += struct.pack("<BBH", rle_len, ncodes, nbits)
        out += b"".join(struct.pack("<HB", e & 0xFFFF, (e >> 16) & 255) for e in ents)
        out += bytes(raw)
    return out


def select(data, dims, offs, items, out_w, out_h, fmt=0, in_len=None, cap=None):
    """(the output stream's first cap bytes -- all of it when cap is None --,
    [length, verdict, empties], the modes used when re-coding to JPT1): the
    call on data[:in_len] with the arguments dims = (w, h, nimg)."""
    data = bytes(data)
    in_len = len(data) if in_len is None else in_len
    src = source_format(data[:in_len], dims)
    target = fmt or src or JPR1
    recs, verdict, empties, modes = [], J.OK, 0, []
    per_item = ((out_w + 7) // 8) * ((out_h + 7) // 8)
    for k, item in enumerate(items):
        item = tuple(int(v) & U64 for v in item)
        if not src or not item_ok(item, dims, out_w, out_h):
            verdict = min(verdict, 1 + k)
            recs += [EMPTY] * per_item
            continue
        for t in source_tiles(item, dims, out_w, out_h):
            rec = None
            if offsets_ok(offs, t, in_len):
                rec = data[int(offs[t]):int(offs[t + 1])]
                if target != src and target == JPT1:
                    rec, md = to_tight(rec)
                    modes += md or []
                elif target != src:
                    rec = to_plain(rec)
            if rec is None:
                empties += 1
                rec = EMPTY
            recs.append(rec)
    out = (MAGIC[target] + struct.pack("<III", out_w, out_h, len(items)) +
           b"".join(struct.pack("<H", len(r)) for r in recs) + b"".join(recs))
    return (out if cap is None else out[:cap]), [len(out), verdict, empties], modes


def offsets_of(data, dims):
    """The index call's offsets of a consistent stream: ntiles + 1 ints."""
    nt = J.ntiles_of(*dims)
    offs, pos = [], 16 + 2 * nt
    for t in range(nt):
        offs.append(pos)
        pos += int.from_bytes(data[16 + 2 * t:18 + 2 * t], "little")
    return offs + [pos]


def sub_arrays(arrays, tiles):
    """The slot arrays of the listed tiles, in that order."""
    return tuple(a[list(tiles)] for a in arrays)
