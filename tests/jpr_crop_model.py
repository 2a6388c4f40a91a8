"""The rectangle rules of jpegr_crop_device (include/jpegr.h) restated in numpy
(a helper, no tests; checked by test_jpr_crop_model.py): which rectangles are
good, bad or empty, which tiles a rectangle touches, and the bytes a call
leaves -- every good rectangle's pixels are the slice of the full image, at
its dst, in rows of 4 w bytes; everything else keeps what it held.

A rectangle is (image, x, y, w, h, dst), unsigned 64-bit values as ints.
"""
import numpy as np

GOOD, BAD, EMPTY = "good", "bad", "empty"
U64 = (1 << 64) - 1


def span(n):
    """Tile columns (rows) a crop of n pixels is given: ceil(n / 8) + 1."""
    return (n + 7) // 8 + 1


def items(max_w, max_h):
    return 0 if max_w <= 0 or max_h <= 0 else span(max_w) * span(max_h)


def scratch_bytes(nrects, max_w, max_h):
    k = items(max_w, max_h)
    return 0 if nrects == 0 or k == 0 else (nrects * (256 * k + 4) + 15) // 16 * 16


def classify(rect, W, H, nimg, max_w, max_h, out_cap, header_ok=True):
    """GOOD, BAD or EMPTY by the rectangle's own fields and the header (no sum
    wraps: Python's ints are exact)."""
    image, x, y, w, h, dst = rect
    if not header_ok:
        return BAD
    if w == 0 or h == 0:
        return EMPTY
    if image >= nimg or w > max_w or h > max_h or x + w > W or y + h > H:
        return BAD
    if dst % 4 != 0 or dst + 4 * w * h > out_cap:
        return BAD
    return GOOD


def touched(rect, W, H):
    """Stream tile numbers a rectangle inside the image touches: tile columns
    x / 8 .. (x + w - 1) / 8 and rows y / 8 .. (y + h - 1) / 8 of its image."""
    image, x, y, w, h, _ = rect
    tx, ty = (W + 7) // 8, (H + 7) // 8
    return [(image * ty + r) * tx + c
            for r in range(y // 8, (y + h - 1) // 8 + 1)
            for c in range(x // 8, (x + w - 1) // 8 + 1)]


def bad_offset_tiles(offs, in_len):
    """Tiles whose offsets are not off[t] <= off[t + 1] <= in_len with a size of
    12 .. 1,036 B (offs: ntiles + 1 unsigned values)."""
    o = [int(v) & U64 for v in offs]
    return {t for t in range(len(o) - 1)
            if not (o[t] <= o[t + 1] <= in_len and 12 <= o[t + 1] - o[t] <= 1036)}


def verdicts(rects, W, H, nimg, max_w, max_h, out_cap, bad_tiles=(), header_ok=True):
    """Every rectangle's class, a good one that touches a tile of bad_tiles
    turned bad."""
    bad_tiles = set(bad_tiles)
    out = []
    for rc in rects:
        c = classify(rc, W, H, nimg, max_w, max_h, out_cap, header_ok)
        if c == GOOD and bad_tiles and bad_tiles.intersection(touched(rc, W, H)):
            c = BAD
        out.append(c)
    return out


def result_words(classes):
    """d_result[0] and [1]: the rectangles delivered (empty ones too), and ~0 or
    1 + the first bad rectangle's index."""
    bad = [i for i, c in enumerate(classes) if c == BAD]
    return [sum(c != BAD for c in classes), 1 + bad[0] if bad else U64]


def expected(full, rects, classes, own, out):
    """`out` (uint8, out_cap bytes, holding what the buffer held before the
    call) with every good rectangle's bytes written: the slice of full
    [nimg, H, W, 4].  own: the classes by the rectangles' own fields and the
    header (verdicts with no bad tiles).  Returns (out, unspecified):
    unspecified marks the own output bytes of rectangles that are bad only
    because a tile failed, which may hold anything; a rectangle bad on its own
    fields writes nothing."""
    out = np.array(out, np.uint8)
    unspecified = np.zeros(out.size, bool)
    for (image, x, y, w, h, dst), c, o in zip(rects, classes, own):
        if c == GOOD:
            out[dst:dst + 4 * w * h] = full[image, y:y + h, x:x + w].reshape(-1)
        elif c == BAD and o == GOOD:
            unspecified[dst:dst + 4 * w * h] = True
    return out, unspecified
