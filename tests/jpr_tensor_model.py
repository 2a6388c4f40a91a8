"""jpegr_crop_tensor_device's rules (include/jpegr.h) restated in numpy (a
helper, no tests; checked against torch by test_jpr_tensor_model.py), on top of
jpr_crop_model.py's slices and classes: a rectangle is (image, x, y, w, h, dst)
with dst and the capacity counted in elements, it takes 3 w h of them, and no
dst is misaligned.  Elements are handled as their bit patterns (unsigned
integers of the element's width), so that every comparison is bitwise.
"""
import numpy as np

import jpr_crop_model as C

GOOD, BAD, EMPTY = C.GOOD, C.BAD, C.EMPTY
U8, F32, F16, BF16 = 0, 1, 2, 3                     # JPEGR_DTYPE_*
CHW, HWC = 0, 1                                     # JPEGR_LAYOUT_*
BITS = {U8: np.uint8, F32: np.uint32, F16: np.uint16, BF16: np.uint16}

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalisation(mean, std):
    """scale = 1 / (255 std) and bias = -mean / std, in Python floats, rounded
    once to float32."""
    return (np.array([1.0 / (255.0 * s) for s in std], np.float32),
            np.array([0.0 - m / s for m, s in zip(mean, std)], np.float32))


def norm_sets():
    """The scale / bias pairs the tests share: ImageNet's; 1 / 255; 2^-20, whose
    f16 results are subnormal; a negative scale."""
    one = np.ones(3, np.float32)
    return {"imagenet": normalisation(IMAGENET_MEAN, IMAGENET_STD),
            "unit": normalisation((0.0,) * 3, (1.0,) * 3),
            "tiny": (one * np.float32(2.0 ** -20), 0 * one),
            "negative": (np.array([-1 / 127.5, -0.5, -3.0], np.float32),
                         np.array([1.0, 0.25, 700.0], np.float32))}


def bf16_bits(f):
    """float32 -> bfloat16 bit patterns, round to nearest-even on the float32 bits."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def elements(v, dtype, scale3=None, bias3=None):
    """Bit patterns of bytes v[..., 3] (channel last): U8 the byte; otherwise
    float32 multiply, then float32 add, then the rounding to dtype."""
    v = np.asarray(v, np.uint8)
    if dtype == U8:
        return v.copy()
    s = np.ones(3, np.float32) if scale3 is None else np.asarray(scale3, np.float32)
    b = np.zeros(3, np.float32) if bias3 is None else np.asarray(bias3, np.float32)
    p = v.astype(np.float32) * s
    f = p + b
    assert p.dtype == np.float32 and f.dtype == np.float32
    if dtype == F32:
        return f.view(np.uint32)
    if dtype == F16:
        return f.astype(np.float16).view(np.uint16)
    return bf16_bits(f)


def crop_elements(full, rect, dtype, layout, flip=False, scale3=None, bias3=None):
    """A good rectangle's 3 w h elements in the order of their addresses; full:
    the images' RGBA8 pixels [nimg, H, W, 4]."""
    image, x, y, w, h, _ = rect
    px = full[image, y:y + h, x:x + w, :3]
    if flip:
        px = px[:, ::-1]
    e = elements(px, dtype, scale3, bias3)
    if layout == CHW:
        e = e.transpose(2, 0, 1)
    return np.ascontiguousarray(e).reshape(-1)


def classify(rect, W, H, nimg, max_w, max_h, out_cap, header_ok=True):
    image, x, y, w, h, dst = rect
    if not header_ok:
        return BAD
    if w == 0 or h == 0:
        return EMPTY
    if image >= nimg or w > max_w or h > max_h or x + w > W or y + h > H:
        return BAD
    if dst + 3 * w * h > out_cap:
        return BAD
    return GOOD


def verdicts(rects, W, H, nimg, max_w, max_h, out_cap, bad_tiles=(), header_ok=True):
    bad_tiles = set(bad_tiles)
    out = []
    for rc in rects:
        c = classify(rc, W, H, nimg, max_w, max_h, out_cap, header_ok)
        if c == GOOD and bad_tiles and bad_tiles.intersection(C.touched(rc, W, H)):
            c = BAD
        out.append(c)
    return out


result_words = C.result_words


def expected(full, rects, classes, own, out, dtype, layout, flips=None, scale3=None, bias3=None):
    """`out` (bit patterns, out_cap elements, what the buffer held before) with
    every good rectangle's elements written; (out, unspecified) as
    jpr_crop_model.expected."""
    out = np.array(out, BITS[dtype])
    unspecified = np.zeros(out.size, bool)
    for i, (rc, c, o) in enumerate(zip(rects, classes, own)):
        _, _, _, w, h, dst = rc
        if c == GOOD:
            out[dst:dst + 3 * w * h] = crop_elements(full, rc, dtype, layout,
                                                     bool(flips[i]) if flips is not None else False,
                                                     scale3, bias3)
        elif c == BAD and o == GOOD:
            unspecified[dst:dst + 3 * w * h] = True
    return out, unspecified
