"""jpegr_crop_tensor_device (include/jpegr.h) on the GPU, by
test_gpu_jpeg_crop.py's method: the stream buffer is exactly the stream, the
output is a view between 4-KiB guards of a sentinel-filled tensor of the output
dtype, the whole tensor is compared bitwise (as integers of the element's
width), d_result starts as garbage.  Expected pixels come from
decompress_images_device of the same stream, through jpr_tensor_model.py
(checked against torch by test_jpr_tensor_model.py).  Everything is bit-exact."""
import numpy as np
import pytest

import jpr_tensor_model as T
from jpr_gpu_lib import (FILL, GUARD, U64, dev_bytes, dev_u64, encoded_jpr, host_offsets, jpr_mutations)
from test_gpu_jpeg_crop import BIG, KINDS, SMALL, full_of, stream_of

pytestmark = pytest.mark.gpu

DTYPES = [T.U8, T.F32, T.F16, T.BF16]
LAYOUTS = [T.CHW, T.HWC]
LAYOUT_NAME = {T.CHW: "chw", T.HWC: "hwc"}


def torch_dtype(dtype):
    import torch
    return {T.U8: torch.uint8, T.F32: torch.float32, T.F16: torch.float16, T.BF16: torch.bfloat16}[dtype]


def sentinel(dtype, n):
    """n elements whose every byte is FILL, as bit patterns."""
    return np.full(n * np.dtype(T.BITS[dtype]).itemsize, FILL, np.uint8).view(T.BITS[dtype])


def place(shapes, gap=1, slot=None, align=None):
    """dst of rectangles laid out one after another, `gap` elements apart; a
    rectangle takes 3 w h elements, or slot[i] where given (one that is meant
    to fail and must write nothing); align[i]: (m, r) puts that dst at r modulo
    m.  Returns (dsts, out_cap)."""
    dsts, pos = [], 0
    for i, (_, _, _, w, h) in enumerate(shapes):
        if align and align.get(i):
            m, r = align[i]
            pos = (pos + m - 1) // m * m + r
        dsts.append(pos)
        pos += (slot[i] if slot and slot[i] is not None else 3 * w * h) + gap
    return dsts, pos


def gpu_tensor(data, dims, rects, max_w, max_h, out_cap, dtype, layout, flips=None, scale=None,
               bias=None, offs=None, in_len=None):
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
    d_out, _, n = jpeg.crop_tensor_device(
        d_stream, in_len, *dims, d_offs, *cols[:5], max_w, max_h, d_dst=cols[5], d_out=big[g:g + out_cap],
        out_cap=out_cap, d_result=res, check=False, dtype=torch_dtype(dtype), layout=LAYOUT_NAME[layout],
        scale=None if scale is None else [float(v) for v in scale],
        bias=None if bias is None else [float(v) for v in bias], d_flip=d_flip)
    torch.cuda.synchronize()
    assert n is None and d_out.data_ptr() == big.data_ptr() + GUARD and d_out.data_ptr() % 16 == 0
    host = big.view(torch.uint8).cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + out_cap * es:] == FILL).all(), "guards"
    return (host[GUARD:GUARD + out_cap * es].copy().view(T.BITS[dtype]),
            [int(x) & U64 for x in res.cpu().tolist()])


def check_call(data, full, dims, rects, max_w, max_h, out_cap, dtype, layout, flips=None, scale=None,
               bias=None, bad_tiles=(), offs=None, header_ok=True):
    """One call against the model: every element of the output (the unspecified
    ones of rectangles with a failed tile aside) and the result words."""
    w, h, nimg = dims
    own = T.verdicts(rects, w, h, nimg, max_w, max_h, out_cap, header_ok=header_ok)
    classes = T.verdicts(rects, w, h, nimg, max_w, max_h, out_cap, bad_tiles, header_ok=header_ok)
    want, loose = T.expected(full, rects, classes, own, sentinel(dtype, out_cap), dtype, layout, flips,
                             scale, bias)
    got, res = gpu_tensor(data, dims, rects, max_w, max_h, out_cap, dtype, layout, flips, scale, bias,
                          offs=offs)
    assert got.dtype == want.dtype
    diff = np.flatnonzero((got != want) & ~loose)
    assert diff.size == 0, f"{diff.size} elements differ, the first at {int(diff[0])}"
    assert res[:2] == T.result_words(classes), (res, T.result_words(classes))
    return classes, res


IMAGENET = T.norm_sets()["imagenet"]


# ---- 1. every rectangle of the small image ----------------------------------------------

@pytest.mark.parametrize("dtype,layout", [(T.F32, T.CHW), (T.U8, T.HWC)])
def test_every_rectangle_of_a_small_image(gpu, oracle, dtype, layout):
    """13 x 11 x 3: all 18,018 rectangles in four calls grouped by whether w
    and h exceed a tile, every odd-indexed one mirrored, one element apart: f32
    rows land on every 4-B phase of 16 and the guard between two crops is one
    element wide."""
    data, full = stream_of(oracle, SMALL, "rand", True)
    total = 0
    for ws, hs in ((range(1, 9), range(1, 9)), (range(9, 14), range(1, 9)),
                   (range(1, 9), range(9, 12)), (range(9, 14), range(9, 12))):
        shapes = [(im, x, y, w, h) for im in range(3) for w in ws for h in hs
                  for x in range(13 - w + 1) for y in range(11 - h + 1)]
        dsts, cap = place(shapes, gap=1)
        flips = [i & 1 for i in range(len(shapes))]
        _, res = check_call(data, full, SMALL, [s + (d,) for s, d in zip(shapes, dsts)], ws[-1], hs[-1],
                            cap, dtype, layout, flips, *IMAGENET)
        assert res == [len(shapes), U64, 0]
        total += len(shapes)
    assert total == 18018


# ---- 2. dtype x layout x flip --------------------------------------------------------------

def store_rects():
    """On 520 x 520 x 2 (66 tile columns with the spare one: a rectangle wider
    than 256 pixels reaches a third strip).  Returns (shapes, align)."""
    shapes = [(0, 13, 21, 37, 9),                  # odd x, odd w: rows on every phase
              (1, 3, 250, 517, 3),                 # x = 3 .. 519: three strips, both ends clipped mid-tile
              (1, 0, 0, 520, 520),                 # a whole image
              (0, 519, 519, 1, 1),
              (1, 100, 200, 64, 48),               # dst at a multiple of 16 B, w a multiple of 4: wide stores
              (1, 100, 200, 64, 48),               # the same one element further: none
              (0, 258, 7, 255, 2)]                 # odd w across a strip boundary
    return shapes, {4: (16, 0), 5: (16, 1)}


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["chw", "hwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32", "f16", "bf16"])
def test_dtype_layout_flip(gpu, oracle, dtype, layout, flip):
    data, full = stream_of(oracle, BIG, "rand", True)
    shapes, align = store_rects()
    dsts, cap = place(shapes, gap=3, align=align)
    assert dsts[4] % 16 == 0 and dsts[5] % 16 == 1        # elements: 16 B or more in every dtype
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    _, res = check_call(data, full, BIG, rects, 520, 520, cap, dtype, layout, [flip] * len(rects), *IMAGENET)
    assert res == [len(rects), U64, 0]


# ---- 3. agreement with the RGBA call ---------------------------------------------------------

@pytest.mark.parametrize("kind,tight", KINDS)
def test_u8_hwc_is_crop_device_without_alpha(gpu, oracle, kind, tight):
    """200 seeded rectangles with w <= 64 and h <= 48, both calls packing them
    back to back: the same bytes, the alpha removed."""
    import torch
    from lz4jpeg import jpeg
    data, _ = stream_of(oracle, BIG, kind, tight)
    rng = np.random.default_rng(2025)
    shapes = []
    for _ in range(200):
        w, h = int(rng.integers(1, 65)), int(rng.integers(1, 49))
        shapes.append((int(rng.integers(0, 2)), int(rng.integers(0, 520 - w + 1)),
                       int(rng.integers(0, 520 - h + 1)), w, h))
    rd = jpeg.StreamReader(dev_bytes(data))
    cols = [dev_u64([s[k] for s in shapes]) for k in range(5)]
    d_rgba, _, n = rd.crops(*cols, 64, 48)
    d_rgb, d_dst, m = rd.crops_tensor(*cols, 64, 48, dtype=torch.uint8, layout="hwc")
    torch.cuda.synchronize()
    npx = sum(s[3] * s[4] for s in shapes)
    assert n == m == 200 and d_rgba.numel() == 4 * npx and d_rgb.numel() == 3 * npx
    assert d_rgb.dtype == torch.uint8 and int(d_dst[-1].item()) == 3 * (npx - shapes[-1][3] * shapes[-1][4])
    rgba = d_rgba.cpu().numpy().reshape(-1, 4)
    assert (rgba[:, 3] == 255).all()
    assert np.array_equal(d_rgb.cpu().numpy().reshape(-1, 3), rgba[:, :3])


# ---- 4. values -------------------------------------------------------------------------------

VALUE_SHAPES = [(0, 1, 2, 64, 48), (1, 455, 471, 61, 47), (0, 200, 300, 33, 17)]


@pytest.mark.parametrize("name", sorted(T.norm_sets()))
@pytest.mark.parametrize("dtype", [T.F32, T.F16, T.BF16], ids=["f32", "f16", "bf16"])
def test_values(gpu, oracle, dtype, name):
    """Random images (their decoded pixels take many byte values) through each
    scale / bias set.  f16 with a scale of 2^-20: subnormals are kept, and the
    reference really holds nonzero subnormals."""
    data, full = stream_of(oracle, BIG, "rand", False)
    scale, bias = T.norm_sets()[name]
    dsts, cap = place(VALUE_SHAPES, gap=5)
    rects = [s + (d,) for s, d in zip(VALUE_SHAPES, dsts)]
    seen = np.unique(np.concatenate([full[im, y:y + h, x:x + w, :3].reshape(-1)
                                     for im, x, y, w, h in VALUE_SHAPES]))
    assert seen.size >= 128
    if dtype == T.F16 and name == "tiny":
        ref = T.crop_elements(full, rects[0], T.F16, T.CHW, False, scale, bias)
        assert (((ref & 0x7C00) == 0) & ((ref & 0x03FF) != 0)).any()
    _, res = check_call(data, full, BIG, rects, 64, 48, cap, dtype, T.CHW, [0, 1, 0], scale, bias)
    assert res == [3, U64, 0]


# ---- 5. bad among good ---------------------------------------------------------------------------

def test_bad_rectangles_among_good_ones(gpu, oracle):
    """One of each failure of a rectangle's own fields at known indices among
    good ones, and an empty one with garbage fields: they write nothing, the
    good ones are exact, the result words are the model's."""
    data, full = stream_of(oracle, BIG, "rand", False)
    shapes = [(0, 3, 5, 20, 10),
              (2, 0, 0, 8, 8),                      # 1: image >= nimg
              (1, 500, 500, 20, 20),
              (0, 0, 0, 65, 8),                     # 3: w > max_w
              (0, 513, 0, 8, 8),                    # 4: x + w past the image
              (0, 100, 7, 64, 48),
              (1 << 60, U64, 7, 0, 5),              # 6: empty, garbage elsewhere
              (1, 33, 44, 5, 6),
              (0, 0, 0, 8, 8),                      # 8: dst near 2^64 (below)
              (0, 40, 40, 7, 5)]
    bad = {1, 3, 4, 8}
    dsts, cap = place(shapes, gap=1, slot=[64 if i in bad | {6} else None for i in range(len(shapes))])
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    rects[6] = rects[6][:5] + (U64 - 1,)
    rects[8] = rects[8][:5] + (U64 - 3 * 64 + 1,)                      # dst + 3 w h wraps to 1
    cap += 3 * 64                                                      # room for one more at the end
    rects.append((0, 0, 0, 8, 8, cap - 3 * 64 + 1))                    # 10: past out_cap by one element
    rects.append((1, 8, 8, 8, 8, cap - 3 * 64))                        # 11: ends at out_cap exactly
    flips = [i % 3 == 0 for i in range(len(rects))]
    classes, res = check_call(data, full, BIG, rects, 64, 48, cap, T.F32, T.CHW, flips, *IMAGENET)
    assert [i for i, c in enumerate(classes) if c == T.BAD] == [1, 3, 4, 8, 10]
    assert classes[6] == T.EMPTY and res == [7, 1 + 1, 0]


def test_wrong_header_makes_every_rectangle_bad(gpu, oracle):
    data, full = stream_of(oracle, BIG, "rand", False)
    shapes = [(0, 3, 5, 20, 10), (1, 0, 0, 0, 0), (1, 500, 500, 20, 20)]
    dsts, cap = place(shapes)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    offs = host_offsets(data, BIG)
    for broken in (b"K" + data[1:], data[:12] + (3).to_bytes(4, "little") + data[16:]):
        _, res = check_call(broken, full, BIG, rects, 64, 48, cap, T.BF16, T.HWC, None, *IMAGENET,
                            offs=offs, header_ok=False)
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
    dsts, cap = place(shapes, gap=1)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    classes, res = check_call(data, full, BIG, rects, 64, 48, cap, T.BF16, T.HWC, [1, 0, 1, 0, 1, 0],
                              *IMAGENET, bad_tiles=bad_tiles, offs=offs)
    assert [c == T.BAD for c in classes] == [True, True, False, False, False, True]
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
    dsts, cap = place(shapes, gap=1)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    classes, res = check_call(data, full, (520, 8, 1), rects, 64, 8, cap, T.F16, T.CHW,
                              [0, 1, 0, 1, 0, 1, 0, 1], *IMAGENET, bad_tiles={40})
    assert classes.count(T.BAD) == 4 and classes.count(T.GOOD) == 4 and res[2] > 0, name


# ---- 7. NULL d_flip, scale3, bias3 ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [T.F32, T.BF16], ids=["f32", "bf16"])
def test_null_flip_scale_and_bias(gpu, oracle, dtype):
    """They get past the argument check and mean no flip, 1.0 and 0.0."""
    data, full = stream_of(oracle, BIG, "smooth", True)
    shapes = [(0, 13, 21, 37, 9), (1, 100, 200, 64, 48)]
    dsts, cap = place(shapes)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    _, res = check_call(data, full, BIG, rects, 64, 48, cap, dtype, T.CHW, None, None, None)
    assert res == [2, U64, 0]
    got, _ = gpu_tensor(data, BIG, rects, 64, 48, cap, dtype, T.CHW, None, None, None)
    one, _ = gpu_tensor(data, BIG, rects, 64, 48, cap, dtype, T.CHW, [0, 0], [1.0] * 3, [0.0] * 3)
    assert np.array_equal(got, one)
    if dtype == T.F32:                                   # the bytes themselves, as floats
        want = full[0, 21:30, 13:50, :3].transpose(2, 0, 1).astype(np.float32).reshape(-1)
        assert np.array_equal(got[:3 * 37 * 9].view(np.float32), want)


# ---- 8. graph replay ----------------------------------------------------------------------------------

def test_graph_replay(gpu, oracle):
    """The index and tensor-crop pair captured once and replayed twice, the
    rectangles and the flip bytes rewritten in place in between: both exact, no
    counter accumulates.  Scale and bias were kernel arguments at capture."""
    import torch
    from lz4jpeg import jpeg
    data, full = stream_of(oracle, BIG, "rand", True)
    d_stream = dev_bytes(data)
    nt = 2 * jpeg.tiles(520, 520)
    sets = [([(0, 13, 21, 37, 9), (1, 499, 503, 21, 17), (0, 0, 0, 0, 3), (0, 4, 504, 8, 8)], [1, 0, 1, 0]),
            ([(1, 0, 0, 64, 48), (0, 600, 0, 8, 8), (1, 7, 9, 33, 31), (0, 511, 511, 9, 9)], [0, 1, 0, 1])]
    dsts, cap = place([(0, 0, 0, 64, 48)] * 4, gap=1)
    scale, bias = IMAGENET
    cols = [torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(5)]
    d_flip = torch.zeros(4, dtype=torch.uint8, device="cuda")
    d_dst = dev_u64(dsts)
    d_offs = torch.zeros(nt + 1, dtype=torch.int64, device="cuda")
    d_ires = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    d_res = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(cap, dtype=torch.bfloat16, device="cuda")
    iscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device="cuda")
    cscr = torch.empty(jpeg.crop_scratch_bytes(4, 64, 48), dtype=torch.uint8, device="cuda")

    def call():
        jpeg.stream_index_device(d_stream, len(data), *BIG, d_offsets=d_offs, d_result=d_ires,
                                 scratch=iscr)
        jpeg.crop_tensor_device(d_stream, len(data), *BIG, d_offs, *cols, 64, 48, d_dst=d_dst,
                                d_out=d_out, out_cap=cap, scratch=cscr, d_result=d_res, check=False,
                                dtype=torch.bfloat16, layout="hwc", scale=[float(v) for v in scale],
                                bias=[float(v) for v in bias], d_flip=d_flip)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # warm-up: four empty rectangles
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for shapes, flips in sets:
        for k in range(5):
            cols[k].copy_(dev_u64([s[k] for s in shapes]))
        d_flip.copy_(torch.tensor(flips, dtype=torch.uint8))
        d_out.view(torch.int16).fill_(0x5A5A)
        g.replay()
        torch.cuda.synchronize()
        rects = [s + (d,) for s, d in zip(shapes, dsts)]
        classes = T.verdicts(rects, *BIG, 64, 48, cap)
        want, _ = T.expected(full, rects, classes, classes, sentinel(T.BF16, cap), T.BF16, T.HWC, flips,
                             scale, bias)
        assert np.array_equal(d_out.view(torch.int16).cpu().numpy().view(np.uint16), want)
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == T.result_words(classes) + [0]
        assert [int(x) & U64 for x in d_ires.cpu().tolist()] == [len(data), U64]
    assert T.result_words(classes) == [3, 2]                # the second set: rectangle 1 is bad


# ---- 9. wrappers ---------------------------------------------------------------------------------------

def test_wrappers(gpu, oracle):
    """crop_tensor_device's defaults (packed back to back; check=True and
    check=False give the same elements), its JpegError naming the first bad
    rectangle, StreamReader.crops_tensor."""
    import torch
    from lz4jpeg import jpeg
    data, full = stream_of(oracle, BIG, "smooth", True)
    rd = jpeg.StreamReader(dev_bytes(data))
    shapes = [(0, 13, 21, 37, 9), (1, 499, 503, 21, 17), (0, 0, 0, 0, 3), (0, 4, 504, 8, 8)]
    cols = [dev_u64([s[k] for s in shapes]) for k in range(5)]
    d_a, d_dst, n = rd.crops_tensor(*cols, 64, 48)
    assert n == 4 and d_a.dtype == torch.float32
    assert d_dst.cpu().tolist() == [0, 3 * 333, 3 * (333 + 357), 3 * (333 + 357)]
    assert d_a.numel() == 3 * (333 + 357 + 64)
    d_b, _, none = rd.crops_tensor(*cols, 64, 48, check=False, out_cap=d_a.numel())
    torch.cuda.synchronize()
    assert none is None and torch.equal(d_a.view(torch.int32), d_b[:d_a.numel()].view(torch.int32))
    want = np.concatenate([T.crop_elements(full, s + (0,), T.F32, T.CHW) for s in shapes])
    assert np.array_equal(d_a.view(torch.int32).cpu().numpy().view(np.uint32), want)
    flip = torch.tensor([True, False, True, True], device="cuda")
    d_c, _, n = rd.crops_tensor(*cols, 64, 48, dtype=torch.float16, layout="hwc", scale=0.5,
                                bias=(1.0, 2.0, 3.0), d_flip=flip)
    want = np.concatenate([T.crop_elements(full, s + (0,), T.F16, T.HWC, f, [0.5] * 3, [1.0, 2.0, 3.0])
                           for s, f in zip(shapes, [True, False, True, True])])
    assert n == 4 and np.array_equal(d_c.view(torch.int16).cpu().numpy().view(np.uint16), want)
    cols[1] = dev_u64([13, 499, 0, 514])
    with pytest.raises(jpeg.JpegError, match="jpegr_crop_tensor_device: rectangle 3"):
        rd.crops_tensor(*cols, 64, 48)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_crop_batch(gpu, oracle, dtype):
    """[n, 3, h, w] equal to the torch chain on StreamReader.crops' output, with
    a flip tensor; and [n, h, w, 3]."""
    import torch
    from lz4jpeg import jpeg
    dtype = getattr(torch, dtype)
    data, _ = stream_of(oracle, BIG, "rand", False)
    rd = jpeg.StreamReader(dev_bytes(data))
    n, w, h = 6, 37, 19
    rng = np.random.default_rng(5)
    d_image = dev_u64(rng.integers(0, 2, n))
    d_x, d_y = dev_u64(rng.integers(0, 520 - w + 1, n)), dev_u64(rng.integers(0, 520 - h + 1, n))
    d_flip = torch.tensor([True, False, False, True, True, False], device="cuda")
    got = rd.crop_batch(d_image, d_x, d_y, w, h, dtype=dtype, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD,
                        d_flip=d_flip)
    assert got.shape == (n, 3, h, w) and got.dtype == dtype and got.is_contiguous()
    d_rgba, _, _ = rd.crops(d_image, d_x, d_y, torch.full_like(d_x, w), torch.full_like(d_x, h), w, h)
    scale, bias = (torch.tensor(v, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
                   for v in jpeg.normalisation(T.IMAGENET_MEAN, T.IMAGENET_STD))
    x = d_rgba.view(n, h, w, 4)[..., :3].permute(0, 3, 1, 2).float().mul(scale).add(bias)
    x = torch.where(d_flip.view(n, 1, 1, 1), x.flip(3), x).to(dtype)
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(ints), x.contiguous().view(ints))
    nhwc = rd.crop_batch(d_image, d_x, d_y, w, h, dtype=dtype, layout="hwc", mean=T.IMAGENET_MEAN,
                         std=T.IMAGENET_STD, d_flip=d_flip)
    assert nhwc.shape == (n, h, w, 3)
    assert torch.equal(nhwc.view(ints), x.permute(0, 2, 3, 1).contiguous().view(ints))
    plain = rd.crop_batch(d_image, d_x, d_y, w, h)                        # 1 / 255 and 0, float32
    want = d_rgba.view(n, h, w, 4)[..., :3].permute(0, 3, 1, 2).float().mul(float(np.float32(1 / 255.0)))
    assert plain.dtype == torch.float32 and torch.equal(plain.view(torch.int32),
                                                        want.contiguous().view(torch.int32))
