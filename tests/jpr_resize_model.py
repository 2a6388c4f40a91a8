"""jpegr_crop_resize_device's rules (include/jpegr.h) restated in numpy (a
helper, no tests; anchored to torch by test_jpr_resize_model.py), on top of
jpr_tensor_model.py: a rectangle is (image, x, y, w, h, dst), its w x h source
pixels are resampled to out_w x out_h, it takes 3 out_w out_h elements, and one
with w or h of 0 is bad.  Weights are fp64 rounded once to float32; the pixels
are summed in float32, one rounded product and one rounded sum a tap, in
ascending order.  Elements are bit patterns, as in jpr_tensor_model.py.
"""
import functools

import numpy as np

import jpr_crop_model as C
import jpr_tensor_model as T

GOOD, BAD = T.GOOD, T.BAD
BILINEAR, TRIANGLE = 0, 1                           # JPEGR_FILTER_*


@functools.lru_cache(maxsize=None)
def axis_taps(n, m, filt):
    """For each of the m output indices of an axis of n source pixels:
    (lo, weights), the window's first pixel and its hi - lo float32 weights.
    Python floats are fp64 and nothing here is fused."""
    r = float(n) / float(m)
    s = r if (filt == TRIANGLE and r > 1.0) else 1.0
    out = []
    for j in range(m):
        c = (float(j) + 0.5) * r
        lo = max(0, int(np.floor((c - s) + 0.5)))
        hi = min(n, int(np.floor((c + s) + 0.5)))
        u = [max(0.0, 1.0 - abs((float(x) + 0.5) - c) / s) for x in range(lo, hi)]
        tot = 0.0
        for v in u:
            tot = tot + v
        wt = np.array([v / tot for v in u], np.float64).astype(np.float32)
        wt.flags.writeable = False
        out.append((lo, wt, tot))
    return tuple(out)


def resample(px, out_w, out_h, filt):
    """px[..., h, w, 3] uint8 -> val[..., out_h, out_w, 3] float32: horizontal
    first, every tap acc = fl32(acc + fl32(wt * v)), ascending."""
    v = np.asarray(px, np.uint8).astype(np.float32)
    h, w = v.shape[-3], v.shape[-2]
    lead = v.shape[:-3]
    mid = np.empty(lead + (h, out_w, 3), np.float32)
    for j, (lo, wt, _) in enumerate(axis_taps(w, out_w, filt)):
        acc = np.zeros(lead + (h, 3), np.float32)
        for k in range(wt.size):
            acc = acc + wt[k] * v[..., :, lo + k, :]
        mid[..., :, j, :] = acc
    val = np.empty(lead + (out_h, out_w, 3), np.float32)
    for i, (lo, wt, _) in enumerate(axis_taps(h, out_h, filt)):
        acc = np.zeros(lead + (out_w, 3), np.float32)
        for k in range(wt.size):
            acc = acc + wt[k] * mid[..., lo + k, :, :]
        val[..., i, :, :] = acc
    assert mid.dtype == np.float32 and val.dtype == np.float32
    return val


def elements(val, dtype, scale3=None, bias3=None):
    """Bit patterns of resampled values val[..., 3] (channel last): U8 rounds to
    nearest-even and clamps; the others are jpr_tensor_model.elements with val
    in the byte's place."""
    val = np.asarray(val, np.float32)
    if dtype == T.U8:
        return np.clip(np.rint(val), 0.0, 255.0).astype(np.uint8)
    s = np.ones(3, np.float32) if scale3 is None else np.asarray(scale3, np.float32)
    b = np.zeros(3, np.float32) if bias3 is None else np.asarray(bias3, np.float32)
    p = val * s
    f = p + b
    assert p.dtype == np.float32 and f.dtype == np.float32
    if dtype == T.F32:
        return f.view(np.uint32)
    if dtype == T.F16:
        return f.astype(np.float16).view(np.uint16)
    return T.bf16_bits(f)


def place_elements(val, dtype, layout, flip=False, scale3=None, bias3=None):
    """val[out_h, out_w, 3] -> the 3 out_w out_h elements in the order of their
    addresses; a flip mirrors the output."""
    if flip:
        val = val[:, ::-1]
    e = elements(val, dtype, scale3, bias3)
    if layout == T.CHW:
        e = e.transpose(2, 0, 1)
    return np.ascontiguousarray(e).reshape(-1)


def crop_elements(full, rect, out_w, out_h, filt, dtype, layout, flip=False, scale3=None, bias3=None):
    """A good rectangle's elements; full: the images' RGBA8 pixels [nimg, H, W, 4]."""
    image, x, y, w, h, _ = rect
    val = resample(full[image, y:y + h, x:x + w, :3], out_w, out_h, filt)
    return place_elements(val, dtype, layout, flip, scale3, bias3)


def classify(rect, W, H, nimg, max_w, max_h, out_w, out_h, out_cap, header_ok=True):
    image, x, y, w, h, dst = rect
    if not header_ok or w == 0 or h == 0:
        return BAD
    if image >= nimg or w > max_w or h > max_h or x + w > W or y + h > H:
        return BAD
    if dst + 3 * out_w * out_h > out_cap:
        return BAD
    return GOOD


def verdicts(rects, W, H, nimg, max_w, max_h, out_w, out_h, out_cap, bad_tiles=(), header_ok=True):
    bad_tiles = set(bad_tiles)
    out = []
    for rc in rects:
        c = classify(rc, W, H, nimg, max_w, max_h, out_w, out_h, out_cap, header_ok)
        if c == GOOD and bad_tiles and bad_tiles.intersection(C.touched(rc, W, H)):
            c = BAD
        out.append(c)
    return out


result_words = C.result_words


def expected(full, rects, classes, own, out, out_w, out_h, filt, dtype, layout, flips=None, scale3=None,
             bias3=None, vals=None):
    """`out` (bit patterns, out_cap elements, what the buffer held before) with
    every good rectangle's elements written; (out, unspecified) as
    jpr_tensor_model.expected.  vals[i]: rectangle i's resampled values where
    the caller has them already (resample over a batch)."""
    out = np.array(out, T.BITS[dtype])
    unspecified = np.zeros(out.size, bool)
    n = 3 * out_w * out_h
    for i, (rc, c, o) in enumerate(zip(rects, classes, own)):
        dst = rc[5]
        flip = bool(flips[i]) if flips is not None else False
        if c == GOOD:
            if vals is not None:
                out[dst:dst + n] = place_elements(vals[i], dtype, layout, flip, scale3, bias3)
            else:
                out[dst:dst + n] = crop_elements(full, rc, out_w, out_h, filt, dtype, layout, flip, scale3,
                                                 bias3)
        elif c == BAD and o == GOOD:
            unspecified[dst:dst + n] = True
    return out, unspecified
