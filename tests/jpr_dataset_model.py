"""The dataset calls' mapping and verdicts (include/jpegr.h:
jpegr_dataset_crop_tensor_device, jpegr_dataset_crop_resize_device) restated in
plain Python (a helper, no tests; checked by test_jpr_dataset_model.py).  A
stream is (image0, w, h, nimg, sound): what its descriptor says, and whether
the rest of it holds (at most 2^32 tiles aside, which tiles_ok tests: in_len
>= 16, pointers present and aligned, a header for w, h, nimg).  A rectangle is
(g, x, y, w, h, dst) with g a dataset-wide image index.  The per-stream rules
are jpr_tensor_model's and jpr_resize_model's own, given the rectangle's local
image index and its stream's own dimensions.
"""
import jpr_resize_model as R
import jpr_tensor_model as T

GOOD, BAD, EMPTY = T.GOOD, T.BAD, T.EMPTY
U64 = (1 << 64) - 1


def table_of(streams):
    """An ascending, gap-free table of (w, h, nimg) or (w, h, nimg, sound) streams."""
    out, g = [], 0
    for s in streams:
        w, h, nimg = s[:3]
        out.append((g, w, h, nimg, s[3] if len(s) > 3 else True))
        g += nimg
    return out


def bisect(table, g):
    """The kernel's search: the index it ends on, and every index it read."""
    lo, hi, read = 0, len(table), []
    assert hi >= 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        read.append(mid)
        if table[mid][0] <= g:
            lo = mid
        else:
            hi = mid
    read.append(lo)
    return lo, read


def tiles_ok(w, h, nimg):
    per = ((w + 7) // 8) * ((h + 7) // 8)
    return per <= 1 << 32 and per * nimg <= 1 << 32


def locate(table, g):
    """(s, g's index in stream s), or None: no stream contains g, or the one the
    search ends on does not, or that stream's descriptor is bad."""
    s, _ = bisect(table, g)
    image0, w, h, nimg, sound = table[s]
    if image0 > g or g - image0 >= nimg:
        return None
    if w == 0 or h == 0 or not sound or not tiles_ok(w, h, nimg):
        return None
    return s, g - image0


def _verdicts(one, table, rects, bad_tiles):
    out = []
    for rc in rects:
        at = locate(table, rc[0])
        if at is None:
            out.append(BAD)
            continue
        s, image = at
        _, w, h, nimg, _ = table[s]
        out.append(one((image,) + tuple(rc[1:]), w, h, nimg, (bad_tiles or {}).get(s, ())))
    return out


def tensor_verdicts(table, rects, max_w, max_h, out_cap, bad_tiles=None):
    """bad_tiles: {stream: its malformed tiles}."""
    return _verdicts(lambda rc, w, h, nimg, bad: T.verdicts([rc], w, h, nimg, max_w, max_h, out_cap, bad)[0],
                     table, rects, bad_tiles)


def resize_verdicts(table, rects, max_w, max_h, out_w, out_h, out_cap, bad_tiles=None):
    return _verdicts(lambda rc, w, h, nimg, bad: R.verdicts([rc], w, h, nimg, max_w, max_h, out_w, out_h,
                                                            out_cap, bad)[0],
                     table, rects, bad_tiles)


result_words = T.result_words


def split(table, rects):
    """{stream: [(the rectangle's index, the rectangle with its local image index)]}
    of the rectangles that locate() places."""
    out = {}
    for i, rc in enumerate(rects):
        at = locate(table, rc[0])
        if at is not None:
            out.setdefault(at[0], []).append((i, (at[1],) + tuple(rc[1:])))
    return out
