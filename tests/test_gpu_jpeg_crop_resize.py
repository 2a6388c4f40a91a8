"""jpegr_crop_resize_device (include/jpegr.h) on the GPU, by
test_gpu_jpeg_crop_tensor.py's method: the stream buffer is exactly the stream,
the output is a view between 4-KiB guards of a sentinel-filled tensor of the
output dtype, the whole tensor is compared bitwise (as integers of the
element's width), d_result starts as garbage.  Expected pixels come from
decompress_images_device of the same stream, through jpr_resize_model.py
(anchored to torch by test_jpr_resize_model.py).  Everything is bit-exact."""
import numpy as np
import pytest

import jpr_resize_model as R
import jpr_tensor_model as T
from jpr_gpu_lib import (FILL, GUARD, U64, dev_bytes, dev_u64, encoded_jpr, host_offsets, jpr_mutations)
from test_gpu_jpeg_crop import BIG, KINDS, SMALL, full_of, stream_of
from test_gpu_jpeg_crop_tensor import (DTYPES, IMAGENET, LAYOUT_NAME, LAYOUTS, gpu_tensor, place, sentinel,
                                       store_rects, torch_dtype)

pytestmark = pytest.mark.gpu

FILTERS = [R.BILINEAR, R.TRIANGLE]
FILTER_IDS = ["bilinear", "triangle"]
assert len(KINDS) == 4


def gpu_resize(data, dims, rects, max_w, max_h, out_w, out_h, filt, out_cap, dtype, layout, flips=None,
               scale=None, bias=None, offs=None, in_len=None):
    """(the call's out_cap output elements as bit patterns, [delivered, verdict,
    rejected] unsigned); the guards are checked here."""
    import torch
    from lz4jpeg import jpeg
    in_len = len(data) if in_len is None else in_len
    d_stream = dev_bytes(data)
    if offs is None:
        d_offs, _ = jpeg.stream_index_device(d_stream, in_len, *dims)
    else:
        d_offs = dev_u64(offs)
    es = np.dtype(T.BITS[dtype]).itemsize
    g = GUARD // es
    big = torch.full((2 * GUARD + out_cap * es,), FILL, dtype=torch.uint8, device="cuda").view(torch_dtype(dtype))
    res = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    cols = [dev_u64([rc[k] for rc in rects]) for k in range(6)]
    d_flip = None if flips is None else torch.tensor([int(f) for f in flips], dtype=torch.uint8, device="cuda")
    d_out, _, n = jpeg.crop_resize_device(
        d_stream, in_len, *dims, d_offs, *cols[:5], max_w, max_h, out_w, out_h, antialias=filt == R.TRIANGLE,
        d_dst=cols[5], d_out=big[g:g + out_cap], out_cap=out_cap, d_result=res, check=False,
        dtype=torch_dtype(dtype), layout=LAYOUT_NAME[layout],
        scale=None if scale is None else [float(v) for v in scale],
        bias=None if bias is None else [float(v) for v in bias], d_flip=d_flip)
    torch.cuda.synchronize()
    assert n is None and d_out.data_ptr() == big.data_ptr() + GUARD and d_out.data_ptr() % 16 == 0
    host = big.view(torch.uint8).cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + out_cap * es:] == FILL).all(), "guards"
    return (host[GUARD:GUARD + out_cap * es].copy().view(T.BITS[dtype]),
            [int(x) & U64 for x in res.cpu().tolist()])


def check_call(data, full, dims, rects, max_w, max_h, out_w, out_h, filt, out_cap, dtype, layout, flips=None,
               scale=None, bias=None, bad_tiles=(), offs=None, header_ok=True, vals=None):
    """One call against the model: every element of the output (the unspecified
    ones of rectangles with a failed tile aside) and the result words."""
    w, h, nimg = dims
    own = R.verdicts(rects, w, h, nimg, max_w, max_h, out_w, out_h, out_cap, header_ok=header_ok)
    classes = R.verdicts(rects, w, h, nimg, max_w, max_h, out_w, out_h, out_cap, bad_tiles,
                         header_ok=header_ok)
    want, loose = R.expected(full, rects, classes, own, sentinel(dtype, out_cap), out_w, out_h, filt, dtype,
                             layout, flips, scale, bias, vals)
    got, res = gpu_resize(data, dims, rects, max_w, max_h, out_w, out_h, filt, out_cap, dtype, layout, flips,
                          scale, bias, offs=offs)
    assert got.dtype == want.dtype
    diff = np.flatnonzero((got != want) & ~loose)
    assert diff.size == 0, f"{diff.size} elements differ, the first at {int(diff[0])}"
    assert res[:2] == R.result_words(classes), (res, R.result_words(classes))
    return classes, res


def slots(shapes, out_w, out_h, gap=1, align=None):
    """place() with every rectangle taking the output's 3 out_w out_h elements."""
    return place(shapes, gap=gap, slot=[3 * out_w * out_h] * len(shapes), align=align)


# the model's resampled values, computed once and shared by the cases that
# differ in dtype, layout and flip only: (key) -> float32 [out_h, out_w, 3]
_VALS = {}


def vals_of(key, full, shapes, out_w, out_h, filt):
    k = (key, out_w, out_h, filt)
    if k not in _VALS:
        vals = [R.resample(full[im, y:y + h, x:x + w, :3], out_w, out_h, filt) for im, x, y, w, h in shapes]
        for v in vals:
            v.flags.writeable = False
        _VALS[k] = vals
    return _VALS[k]


# ---- 1. identity ------------------------------------------------------------------------

@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["chw", "hwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32", "f16", "bf16"])
@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_IDS)
def test_identity_is_crop_tensor_device(gpu, oracle, filt, dtype, layout, flip):
    """out = (w, h): every weight is 1.0 or 0.0 and the elements are
    crop_tensor_device's for the same rectangle, bit for bit."""
    data, _ = stream_of(oracle, BIG, "rand", True)
    for im, x, y, w, h in store_rects()[0]:
        rects, cap = [(im, x, y, w, h, 3)], 3 * w * h + 5
        want, wres = gpu_tensor(data, BIG, rects, w, h, cap, dtype, layout, [flip], *IMAGENET)
        got, res = gpu_resize(data, BIG, rects, w, h, w, h, filt, cap, dtype, layout, [flip], *IMAGENET)
        assert wres == res == [1, U64, 0]
        assert np.array_equal(got, want), (im, x, y, w, h)


# ---- 2. every rectangle of the small image ------------------------------------------------

def small_vals(full, shapes, filt):
    """resample over every position of one (w, h) at once: [nimg, y, x] windows."""
    key = ("small", filt)
    if key not in _VALS:
        by = {}
        for w in range(1, 14):
            for h in range(1, 12):
                win = np.lib.stride_tricks.sliding_window_view(full[..., :3], (h, w), axis=(1, 2))
                by[w, h] = R.resample(win.transpose(0, 1, 2, 4, 5, 3), 5, 7, filt)
        _VALS[key] = by
    by = _VALS[key]
    return [by[w, h][im, y, x] for im, x, y, w, h in shapes]


@pytest.mark.parametrize("dtype,layout", [(T.F32, T.CHW), (T.U8, T.HWC)], ids=["f32-chw", "u8-hwc"])
@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_IDS)
def test_every_rectangle_of_a_small_image(gpu, oracle, filt, dtype, layout):
    """13 x 11 x 3: all 18,018 rectangles in four calls grouped by whether w
    and h exceed a tile, each to 5 x 7, every odd-indexed one mirrored, one
    element apart: every n -> 5 and n -> 7 for n = 1 .. 13, both clipped window
    ends, n < m, n = m and n > m in one call."""
    data, full = stream_of(oracle, SMALL, "rand", True)
    total = 0
    for ws, hs in ((range(1, 9), range(1, 9)), (range(9, 14), range(1, 9)),
                   (range(1, 9), range(9, 12)), (range(9, 14), range(9, 12))):
        shapes = [(im, x, y, w, h) for im in range(3) for w in ws for h in hs
                  for x in range(13 - w + 1) for y in range(11 - h + 1)]
        dsts, cap = slots(shapes, 5, 7, gap=1)
        flips = [i & 1 for i in range(len(shapes))]
        _, res = check_call(data, full, SMALL, [s + (d,) for s, d in zip(shapes, dsts)], ws[-1], hs[-1],
                            5, 7, filt, cap, dtype, layout, flips, *IMAGENET,
                            vals=small_vals(full, shapes, filt))
        assert res == [len(shapes), U64, 0]
        total += len(shapes)
    assert total == 18018


# ---- 3. shapes on the big image -------------------------------------------------------------

# to 224 x 224: the whole image (r = 2.32, 4 to 5 taps, 3 at the ends), 517 x 3 (down in x, up
# 75 x in y), 1 x 1 (a constant), odd widths across strip boundaries; to 7 x 5:
# r = 74, about 150 taps; to 1 x 1; to 523 x 3: wider than the source, out_w no
# multiple of 4 and more than one workgroup of columns
OUT_SIZES = [(224, 224), (7, 5), (1, 1), (523, 3)]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["chw", "hwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32", "f16", "bf16"])
@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_IDS)
def test_shapes(gpu, oracle, filt, dtype, layout, flip):
    data, full = stream_of(oracle, BIG, "rand", True)
    shapes, _ = store_rects()
    for out_w, out_h in OUT_SIZES:
        dsts, cap = slots(shapes, out_w, out_h, gap=3, align={4: (16, 0), 5: (16, 1)})
        rects = [s + (d,) for s, d in zip(shapes, dsts)]
        _, res = check_call(data, full, BIG, rects, 520, 520, out_w, out_h, filt, cap, dtype, layout,
                            [flip] * len(rects), *IMAGENET,
                            vals=vals_of("store", full, shapes, out_w, out_h, filt))
        assert res == [len(rects), U64, 0], (out_w, out_h)


def test_the_taps_of_the_shapes():
    """What the comment above OUT_SIZES says of the windows."""
    assert {t[1].size for t in R.axis_taps(520, 224, R.TRIANGLE)} == {3, 4, 5}
    assert max(t[1].size for t in R.axis_taps(520, 7, R.TRIANGLE)) >= 148
    assert {t[1].size for t in R.axis_taps(520, 7, R.BILINEAR)} == {2}
    assert {t[1].size for t in R.axis_taps(3, 224, R.TRIANGLE)} <= {1, 2}


# ---- 4. values ---------------------------------------------------------------------------------

VALUE_SHAPES = [(0, 1, 2, 64, 48), (1, 455, 471, 61, 47), (0, 200, 300, 33, 17)]


@pytest.mark.parametrize("name", sorted(T.norm_sets()))
@pytest.mark.parametrize("dtype", [T.F32, T.F16, T.BF16], ids=["f32", "f16", "bf16"])
def test_values(gpu, oracle, dtype, name):
    """Each scale / bias set on resampled values (to 40 x 24: down from two of
    the rectangles, up from the third).  f16 with a scale of 2^-20: subnormals
    are kept, and the reference really holds nonzero subnormals."""
    data, full = stream_of(oracle, BIG, "rand", False)
    scale, bias = T.norm_sets()[name]
    dsts, cap = slots(VALUE_SHAPES, 40, 24, gap=5)
    rects = [s + (d,) for s, d in zip(VALUE_SHAPES, dsts)]
    vals = vals_of("values", full, VALUE_SHAPES, 40, 24, R.TRIANGLE)
    assert np.unique(np.concatenate([v.reshape(-1) for v in vals])).size >= 1000   # no bytes: fractions
    if dtype == T.F16 and name == "tiny":
        ref = R.place_elements(vals[0], T.F16, T.CHW, False, scale, bias)
        assert (((ref & 0x7C00) == 0) & ((ref & 0x03FF) != 0)).any()
    _, res = check_call(data, full, BIG, rects, 64, 48, 40, 24, R.TRIANGLE, cap, dtype, T.CHW, [0, 1, 0],
                        scale, bias, vals=vals)
    assert res == [3, U64, 0]


@pytest.mark.parametrize("dtype", [T.F32, T.BF16], ids=["f32", "bf16"])
def test_null_flip_scale_and_bias(gpu, oracle, dtype):
    """They get past the argument check and mean no flip, 1.0 and 0.0."""
    data, full = stream_of(oracle, BIG, "smooth", True)
    shapes = [(0, 13, 21, 37, 9), (1, 100, 200, 64, 48)]
    dsts, cap = slots(shapes, 16, 12)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    _, res = check_call(data, full, BIG, rects, 64, 48, 16, 12, R.BILINEAR, cap, dtype, T.CHW, None, None, None)
    assert res == [2, U64, 0]
    got, _ = gpu_resize(data, BIG, rects, 64, 48, 16, 12, R.BILINEAR, cap, dtype, T.CHW, None, None, None)
    one, _ = gpu_resize(data, BIG, rects, 64, 48, 16, 12, R.BILINEAR, cap, dtype, T.CHW, [0, 0], [1.0] * 3,
                        [0.0] * 3)
    assert np.array_equal(got, one)


# ---- 5. bad among good ---------------------------------------------------------------------------

def test_bad_rectangles_among_good_ones(gpu, oracle):
    """One of each failure of a rectangle's own fields at known indices among
    good ones: they write nothing, the good ones are exact, the result words
    are the model's.  A zero-sized rectangle is bad here, not empty."""
    data, full = stream_of(oracle, BIG, "rand", False)
    ow, oh = 9, 6
    n = 3 * ow * oh
    shapes = [(0, 3, 5, 20, 10),
              (2, 0, 0, 8, 8),                      # 1: image >= nimg
              (1, 500, 500, 20, 20),
              (0, 0, 0, 65, 8),                     # 3: w > max_w
              (0, 513, 0, 8, 8),                    # 4: x + w past the image
              (0, 100, 7, 64, 48),
              (0, 7, 7, 0, 5),                      # 6: w == 0
              (1, 33, 44, 5, 6),
              (1, 7, 7, 5, 0),                      # 8: h == 0
              (0, 40, 40, 7, 5)]
    dsts, cap = slots(shapes, ow, oh, gap=1)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    cap += n                                                           # room for one more at the end
    rects.append((0, 0, 0, 8, 8, cap - n + 1))                         # 10: past out_cap by one element
    rects.append((1, 8, 8, 8, 8, cap - n))                             # 11: ends at out_cap exactly
    rects.append((0, 0, 0, 8, 8, U64 - n + 1))                         # 12: dst + 3 out_w out_h wraps to 1
    flips = [i % 3 == 0 for i in range(len(rects))]
    classes, res = check_call(data, full, BIG, rects, 64, 48, ow, oh, R.TRIANGLE, cap, T.F32, T.CHW, flips,
                              *IMAGENET)
    assert [i for i, c in enumerate(classes) if c == R.BAD] == [1, 3, 4, 6, 8, 10, 12]
    assert res == [6, 1 + 1, 0]


def test_wrong_header_makes_every_rectangle_bad(gpu, oracle):
    data, full = stream_of(oracle, BIG, "rand", False)
    shapes = [(0, 3, 5, 20, 10), (1, 0, 0, 64, 48), (1, 500, 500, 20, 20)]
    dsts, cap = slots(shapes, 9, 6)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    offs = host_offsets(data, BIG)
    for broken in (b"K" + data[1:], data[:12] + (3).to_bytes(4, "little") + data[16:]):
        _, res = check_call(broken, full, BIG, rects, 64, 48, 9, 6, R.TRIANGLE, cap, T.BF16, T.HWC, None,
                            *IMAGENET, offs=offs, header_ok=False)
        assert res == [0, 1, 0]


# ---- 6. untrusted offsets, a bad record -------------------------------------------------------------

def test_untrusted_offsets(gpu, oracle):
    """An offset past in_len: the rectangles touching the two tiles it bounds
    are bad, the others exact, the guards intact."""
    data, full = stream_of(oracle, BIG, "rand", False)
    offs = [int(v) for v in host_offsets(data, BIG)]
    e1 = 5 * 65 + 10                                                    # tile (10, 5) of image 0
    offs[e1] = len(data) + 1
    bad_tiles = {e1 - 1, e1}
    shapes = [(0, 8 * 10, 8 * 5, 8, 8), (0, 8 * 9 - 3, 8 * 5 - 3, 4, 4), (0, 8 * 11, 8 * 5, 64, 48),
              (0, 8 * 8, 8 * 5, 8, 8), (1, 8 * 10, 8 * 5, 8, 8), (0, 8 * 9 + 7, 8 * 5 + 7, 2, 2)]
    dsts, cap = slots(shapes, 9, 6, gap=1)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    classes, res = check_call(data, full, BIG, rects, 64, 48, 9, 6, R.TRIANGLE, cap, T.BF16, T.HWC,
                              [1, 0, 1, 0, 1, 0], *IMAGENET, bad_tiles=bad_tiles, offs=offs)
    assert [c == R.BAD for c in classes] == [True, True, False, False, False, True]
    assert res[2] > 0


def test_bad_record(gpu, oracle):
    """Tile 40 of a 65-tile stream with a luma ncodes of 129: the rectangles
    that touch it are bad, the others exact."""
    import torch
    good = encoded_jpr(65)
    full = full_of(dev_bytes(good))
    torch.cuda.synchronize()
    name, data, in_len, _, tile = [m for m in jpr_mutations(good) if m[4] is not None][0]
    assert tile == 40 and in_len == len(data)
    shapes = [(0, 300, 0, 20, 8), (0, 318, 2, 8, 4), (0, 320, 0, 8, 8), (0, 327, 7, 1, 1),
              (0, 328, 0, 64, 8), (0, 505, 0, 7, 8), (0, 0, 0, 64, 8), (0, 263, 1, 64, 6)]
    dsts, cap = slots(shapes, 11, 4, gap=1)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    classes, res = check_call(data, full, (520, 8, 1), rects, 64, 8, 11, 4, R.BILINEAR, cap, T.F16, T.CHW,
                              [0, 1, 0, 1, 0, 1, 0, 1], *IMAGENET, bad_tiles={40})
    assert classes.count(R.BAD) == 4 and classes.count(R.GOOD) == 4 and res[2] > 0, name


# ---- 7. graph replay ----------------------------------------------------------------------------------

def test_graph_replay(gpu, oracle):
    """One call captured and replayed twice over a re-sentinelled output: the
    same elements and result words both times, no counter accumulates.  Scale
    and bias were kernel arguments at capture."""
    import torch
    from lz4jpeg import jpeg
    data, full = stream_of(oracle, BIG, "rand", True)
    d_stream = dev_bytes(data)
    ow, oh = 24, 16
    shapes = [(0, 13, 21, 37, 9), (1, 499, 503, 21, 17), (0, 600, 0, 8, 8), (1, 7, 9, 64, 48)]
    flips = [1, 0, 1, 1]
    dsts, cap = slots(shapes, ow, oh, gap=1)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    scale, bias = IMAGENET
    cols = [dev_u64([rc[k] for rc in rects]) for k in range(6)]
    d_flip = torch.tensor(flips, dtype=torch.uint8, device="cuda")
    d_offs, _ = jpeg.stream_index_device(d_stream, len(data), *BIG)
    d_res = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(cap, dtype=torch.bfloat16, device="cuda")
    scr = torch.empty(jpeg.crop_resize_scratch_bytes(4, 64, 48, ow, oh), dtype=torch.uint8, device="cuda")

    def call():
        jpeg.crop_resize_device(d_stream, len(data), *BIG, d_offs, *cols[:5], 64, 48, ow, oh, d_dst=cols[5],
                                d_out=d_out, out_cap=cap, scratch=scr, d_result=d_res, check=False,
                                dtype=torch.bfloat16, layout="hwc", scale=[float(v) for v in scale],
                                bias=[float(v) for v in bias], d_flip=d_flip)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    classes = R.verdicts(rects, *BIG, 64, 48, ow, oh, cap)
    assert R.result_words(classes) == [3, 3]                # rectangle 2 is bad
    want, _ = R.expected(full, rects, classes, classes, sentinel(T.BF16, cap), ow, oh, R.TRIANGLE, T.BF16,
                         T.HWC, flips, scale, bias)
    for _ in range(2):
        d_out.view(torch.int16).fill_(0x5A5A)
        d_res.fill_(7)
        scr.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_out.view(torch.int16).cpu().numpy().view(np.uint16), want)
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == R.result_words(classes) + [0]


# ---- 8. wrappers ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_resized_crop_batch(gpu, oracle, dtype):
    """[n, 3, out_h, out_w] and [n, out_h, out_w, 3] against the model; max_w
    and max_h of None give what explicit maxima give; crops_resized's defaults
    and its JpegError naming the first bad rectangle."""
    import torch
    from lz4jpeg import jpeg
    code = {"float32": T.F32, "bfloat16": T.BF16}[dtype]
    dtype = getattr(torch, dtype)
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    data, full = stream_of(oracle, BIG, "rand", False)
    rd = jpeg.StreamReader(dev_bytes(data))
    ow, oh = 20, 12
    shapes = [(0, 13, 21, 37, 9), (1, 399, 403, 121, 117), (0, 4, 504, 8, 8), (1, 0, 0, 300, 200),
              (0, 100, 100, 20, 12)]
    flips = [True, False, False, True, True]
    n = len(shapes)
    cols = [dev_u64([s[k] for s in shapes]) for k in range(5)]
    d_flip = torch.tensor(flips, device="cuda")
    scale, bias = jpeg.normalisation(T.IMAGENET_MEAN, T.IMAGENET_STD)
    vals = vals_of("batch", full, shapes, ow, oh, R.TRIANGLE)
    for layout, lay, shape in (("chw", T.CHW, (n, 3, oh, ow)), ("hwc", T.HWC, (n, oh, ow, 3))):
        got = rd.resized_crop_batch(*cols, ow, oh, dtype=dtype, layout=layout, mean=T.IMAGENET_MEAN,
                                    std=T.IMAGENET_STD, d_flip=d_flip)
        assert got.shape == shape and got.dtype == dtype and got.is_contiguous()
        want = np.concatenate([R.place_elements(v, code, lay, f, scale, bias) for v, f in zip(vals, flips)])
        assert np.array_equal(got.view(ints).cpu().numpy().reshape(-1).view(T.BITS[code]), want)
        same = rd.resized_crop_batch(*cols, ow, oh, dtype=dtype, layout=layout, mean=T.IMAGENET_MEAN,
                                     std=T.IMAGENET_STD, d_flip=d_flip, max_w=300, max_h=200)
        assert torch.equal(got.view(ints), same.view(ints))
    plain = rd.resized_crop_batch(*cols, ow, oh, antialias=False)         # 1 / 255 and 0, float32, BILINEAR
    pv = vals_of("batch", full, shapes, ow, oh, R.BILINEAR)
    want = np.concatenate([R.place_elements(v, T.F32, T.CHW, False, *jpeg.normalisation()) for v in pv])
    assert plain.dtype == torch.float32
    assert np.array_equal(plain.view(torch.int32).cpu().numpy().reshape(-1).view(np.uint32), want)
    d_a, d_dst, m = rd.crops_resized(*cols, 300, 200, ow, oh, dtype=dtype)
    assert m == n and d_a.numel() == n * 3 * ow * oh and d_dst.cpu().tolist() == [3 * ow * oh * i for i in range(n)]
    cols[3] = dev_u64([37, 121, 0, 300, 20])
    with pytest.raises(jpeg.JpegError, match="jpegr_crop_resize_device: rectangle 2"):
        rd.crops_resized(*cols, 300, 200, ow, oh)
