"""jpegr_dataset_crop_tensor_device and jpegr_dataset_crop_resize_device
(include/jpegr.h) on the GPU, by test_gpu_jpeg_crop_resize.py's method: every
stream buffer is exactly its stream, the output is a view between 4-KiB guards
of a sentinel-filled tensor of the output dtype and is compared bitwise as a
whole, d_result starts as garbage.  The expected elements are what the
single-stream calls write for the same rectangles (local image index, the same
dst) on each stream alone -- those calls are pinned to the oracle by their own
tests -- and the verdicts are jpr_dataset_model.py's.

Four streams of the oracle's encodings: A 40 x 24 x 3 JPR1, B 24 x 40 x 2 JPT1,
C 8 x 8 x 1 JPT1 (one tile, one image), D 17 x 9 x 4 JPR1 (odd edges), with
max_w = max_h = 16: K = 9, so a workgroup's 64 items hold seven rectangles or
more and, the rectangles cycling the streams, lanes of both formats."""
import numpy as np
import pytest

import jpr_dataset_model as D
import jpr_resize_model as R
import jpr_tensor_model as T
from jpr_gpu_lib import FILL, GUARD, U64, dev_bytes, dev_u64, host_offsets
from test_gpu_jpeg_crop import stream_of
from test_gpu_jpeg_crop_resize import FILTER_IDS, FILTERS, gpu_resize
from test_gpu_jpeg_crop_tensor import (DTYPES, IMAGENET, LAYOUT_NAME, LAYOUTS, gpu_tensor, sentinel,
                                       torch_dtype)

pytestmark = pytest.mark.gpu

DIMS = {"A": (40, 24, 3), "B": (24, 40, 2), "C": (8, 8, 1), "D": (17, 9, 4)}
TIGHT = {"A": False, "B": True, "C": True, "D": False}
MAX = 16

# (image in the stream, x, y, w, h) by stream: each stream's first and last
# image, C's whole image, D's whole height at both of its odd edges (its whole
# width is 17 > MAX), 1 x 1 rectangles, corners, and one empty rectangle each
SHAPES = {
    "A": [(0, 0, 0, 16, 16), (2, 24, 8, 16, 16), (1, 3, 5, 13, 7), (0, 39, 23, 1, 1), (2, 7, 0, 16, 1),
          (1, 0, 9, 1, 15), (0, 10, 10, 0, 5), (2, 20, 3, 9, 16), (1, 17, 8, 16, 9), (0, 33, 1, 7, 11)],
    "B": [(0, 0, 0, 16, 16), (1, 8, 24, 16, 16), (0, 5, 3, 11, 13), (1, 23, 39, 1, 1), (0, 1, 20, 16, 3),
          (1, 9, 9, 15, 15), (0, 0, 0, 1, 1), (1, 3, 31, 5, 9), (0, 12, 12, 12, 16), (1, 7, 7, 0, 0)],
    "C": [(0, 0, 0, 8, 8), (0, 0, 0, 1, 1), (0, 7, 7, 1, 1), (0, 3, 2, 5, 6), (0, 0, 0, 8, 8),
          (0, 1, 0, 7, 8), (0, 0, 0, 8, 0), (0, 2, 2, 3, 3), (0, 0, 4, 8, 4), (0, 4, 0, 4, 8)],
    "D": [(0, 1, 0, 16, 9), (3, 0, 0, 16, 9), (1, 16, 8, 1, 1), (2, 5, 1, 11, 7), (0, 0, 0, 1, 9),
          (3, 9, 0, 8, 8), (1, 0, 0, 0, 0), (2, 15, 3, 2, 5), (3, 2, 2, 13, 6), (1, 8, 0, 9, 9)]}


class Entry:
    """A stream and what its descriptor says of it.  data, dims: the stream and
    its true (w, h, nimg); offs: its offsets, None for the index call's; desc:
    the descriptor's w, h, nimg; in_len: the descriptor's; shift: bytes added to
    d_tile_offsets; sound: whether the descriptor is a good one."""

    def __init__(self, data, dims, offs=None, desc=None, in_len=None, shift=0, sound=True):
        self.data, self.dims, self.offs = data, dims, offs
        self.desc = dims if desc is None else desc
        self.in_len = len(data) if in_len is None else in_len
        self.shift, self.sound = shift, sound


def entries_of(oracle, names):
    return [Entry(stream_of(oracle, DIMS[n], "rand", TIGHT[n])[0], DIMS[n]) for n in names]


def model_table(entries):
    """jpr_dataset_model's table: image0 by the true counts, the rest the descriptor's."""
    out, g = [], 0
    for e in entries:
        out.append((g, *e.desc, e.sound))
        g += e.dims[2]
    return out


def cycle(names, shapes=SHAPES, skip_empty=False):
    """The streams' rectangles taken in turn, A, B, C, D, A, ..., with dataset-wide
    image indices: [(g, x, y, w, h)].  skip_empty: 1 x 1 in an empty one's place."""
    image0, g = {}, 0
    for n in names:
        image0[n] = g
        g += DIMS[n][2]
    out = []
    for k in range(max(len(shapes[n]) for n in names)):
        for n in names:
            if k < len(shapes[n]):
                im, x, y, w, h = shapes[n][k]
                if skip_empty and (w == 0 or h == 0):
                    w = h = 1
                out.append((image0[n] + im, x, y, w, h))
    return out


def laid_out(shapes, per=None, gap=1):
    """dst one after another, `gap` elements apart; per: the elements of each
    (None: 3 w h).  Returns (rects, out_cap)."""
    rects, pos = [], 0
    for g, x, y, w, h in shapes:
        rects.append((g, x, y, w, h, pos))
        pos += (3 * w * h if per is None else per) + gap
    return rects, pos


def gpu_dataset(entries, rects, out_cap, dtype, layout, flips=None, scale=None, bias=None, resize=None,
                image0=None):
    """(the call's out_cap output elements as bit patterns, [delivered, verdict,
    rejected] unsigned) of one dataset call; resize: None for the tensor call or
    (out_w, out_h, filter).  The guards are checked here."""
    import torch
    from lz4jpeg import jpeg
    keep, rows, g = [], [], 0
    for k, e in enumerate(entries):
        d_stream = dev_bytes(e.data)
        d_offs = (jpeg.stream_index_device(d_stream, len(e.data), *e.dims)[0] if e.offs is None
                  else dev_u64(e.offs))
        keep += [d_stream, d_offs]
        rows.append((d_stream.data_ptr(), e.in_len, d_offs.data_ptr() + e.shift,
                     g if image0 is None else image0[k], *e.desc))
        g += e.dims[2]
    d_table = torch.from_numpy(jpeg.stream_table(rows).view(np.int64)).cuda()
    es = np.dtype(T.BITS[dtype]).itemsize
    gd = GUARD // es
    big = torch.full((2 * GUARD + out_cap * es,), FILL, dtype=torch.uint8, device="cuda").view(torch_dtype(dtype))
    res = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    cols = [dev_u64([rc[k] for rc in rects]) for k in range(6)]
    d_flip = None if flips is None else torch.tensor([int(f) for f in flips], dtype=torch.uint8, device="cuda")
    kw = dict(d_dst=cols[5], d_out=big[gd:gd + out_cap], out_cap=out_cap, d_result=res, check=False,
              dtype=torch_dtype(dtype), layout=LAYOUT_NAME[layout],
              scale=None if scale is None else [float(v) for v in scale],
              bias=None if bias is None else [float(v) for v in bias], d_flip=d_flip)
    if resize is None:
        d_out, _, n = jpeg.dataset_crop_tensor_device(d_table, len(entries), *cols[:5], MAX, MAX, **kw)
    else:
        d_out, _, n = jpeg.dataset_crop_resize_device(d_table, len(entries), *cols[:5], MAX, MAX, resize[0],
                                                      resize[1], antialias=resize[2] == R.TRIANGLE, **kw)
    torch.cuda.synchronize()
    del keep
    assert n is None and d_out.data_ptr() == big.data_ptr() + GUARD and d_out.data_ptr() % 16 == 0
    host = big.view(torch.uint8).cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + out_cap * es:] == FILL).all(), "guards"
    return (host[GUARD:GUARD + out_cap * es].copy().view(T.BITS[dtype]),
            [int(x) & U64 for x in res.cpu().tolist()])


def single_calls(entries, rects, out_cap, dtype, layout, flips=None, scale=None, bias=None, resize=None,
                 skip=(), table=None):
    """What the single-stream calls write into one sentinel-filled output for
    the same rectangles, each stream by a call of its own with the local image
    indices and the same dst (the streams in `skip` left out: their descriptors
    are bad); and the sum of those calls' third result words."""
    table = D.table_of([e.dims for e in entries]) if table is None else table
    fill = sentinel(dtype, out_cap)
    want, rejected = fill.copy(), 0
    for s, items in sorted(D.split(table, rects).items()):
        if s in skip:
            continue
        e = entries[s]
        local = [rc for _, rc in items]
        fl = None if flips is None else [flips[i] for i, _ in items]
        mw, mh = min(MAX, e.dims[0]), min(MAX, e.dims[1])         # these calls hold max_w to the stream
        if resize is None:
            got, res = gpu_tensor(e.data, e.dims, local, mw, mh, out_cap, dtype, layout, fl, scale, bias,
                                  offs=e.offs)
        else:
            got, res = gpu_resize(e.data, e.dims, local, mw, mh, resize[0], resize[1], resize[2], out_cap,
                                  dtype, layout, fl, scale, bias, offs=e.offs)
        wrote = got != fill
        want[wrote] = got[wrote]
        rejected += res[2]
    return want, rejected


def verdicts_of(entries, rects, out_cap, resize=None, bad_tiles=None):
    table = model_table(entries)
    if resize is None:
        return D.tensor_verdicts(table, rects, MAX, MAX, out_cap, bad_tiles)
    return D.resize_verdicts(table, rects, MAX, MAX, resize[0], resize[1], out_cap, bad_tiles)


def check_equal(entries, rects, out_cap, dtype, layout, flips, resize=None, skip=(), bad_tiles=None):
    """One dataset call against the single-stream calls and the model; returns
    (the classes, the result words)."""
    classes = verdicts_of(entries, rects, out_cap, resize, bad_tiles)
    own = verdicts_of(entries, rects, out_cap, resize)
    want, rejected = single_calls(entries, rects, out_cap, dtype, layout, flips, *IMAGENET, resize=resize,
                                  skip=skip)
    got, res = gpu_dataset(entries, rects, out_cap, dtype, layout, flips, *IMAGENET, resize=resize)
    loose = np.zeros(out_cap, bool)                    # a rectangle that failed inside a tile: its own elements
    for rc, c, o in zip(rects, classes, own):
        if c == T.BAD and o == T.GOOD:
            n = 3 * rc[3] * rc[4] if resize is None else 3 * resize[0] * resize[1]
            loose[rc[5]:rc[5] + n] = True
    diff = np.flatnonzero((got != want) & ~loose)
    assert diff.size == 0, f"{diff.size} elements differ, the first at {int(diff[0])}"
    assert res[:2] == D.result_words(classes), (res, D.result_words(classes))
    assert res[2] == rejected, (res, rejected)
    return classes, res


# ---- 1. and 2. equality with the single-stream calls; waves of one format -------------------

SETS = ["ABCD", "AD", "BC"]                            # AD: JPR1 lanes only; BC: JPT1 lanes only


@pytest.mark.parametrize("layout", LAYOUTS, ids=["chw", "hwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32", "f16", "bf16"])
@pytest.mark.parametrize("names", SETS)
def test_tensor_call_equals_the_single_stream_calls(gpu, oracle, names, dtype, layout):
    entries = entries_of(oracle, names)
    rects, cap = laid_out(cycle(names), gap=1)
    assert len(rects) == 10 * len(names)
    flips = [i % 3 != 1 for i in range(len(rects))]
    classes, res = check_equal(entries, rects, cap, dtype, layout, flips)
    assert classes.count(T.EMPTY) == len(names) and T.BAD not in classes
    assert res == [len(rects), U64, 0]


@pytest.mark.parametrize("out,dtype,layout", [((7, 5), T.F32, T.CHW), ((16, 16), T.BF16, T.HWC)],
                         ids=["7x5-f32-chw", "16x16-bf16-hwc"])
@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("names", SETS)
def test_resize_call_equals_the_single_stream_calls(gpu, oracle, names, filt, out, dtype, layout):
    """No rectangle is empty in this call: 1 x 1 rectangles stand where the
    tensor test has its empty ones."""
    entries = entries_of(oracle, names)
    rects, cap = laid_out(cycle(names, skip_empty=True), per=3 * out[0] * out[1], gap=1)
    flips = [i % 3 != 1 for i in range(len(rects))]
    classes, res = check_equal(entries, rects, cap, dtype, layout, flips, resize=(*out, filt))
    assert res == [len(rects), U64, 0] and set(classes) == {R.GOOD}


# ---- 3. per-stream rules ------------------------------------------------------------------

def ruled_entries(oracle):
    """A, B with a wrong w, C, D, then C with nimg = 0, C with in_len = 15 and D
    with misaligned offsets: streams 1, 4, 5, 6 are bad, 0, 2, 3 sound."""
    a, b, c, d = entries_of(oracle, "ABCD")
    return [a, Entry(b.data, b.dims, desc=(32, 40, 2), sound=False), c, d,
            Entry(c.data, c.dims, desc=(8, 8, 0), sound=False),
            Entry(c.data, c.dims, in_len=15, sound=False),
            Entry(d.data, d.dims, shift=4, sound=False)], (1, 4, 5, 6)


@pytest.mark.parametrize("resize", [None, (7, 5, R.TRIANGLE)], ids=["tensor", "resize"])
def test_per_stream_rules(gpu, oracle, resize):
    entries, bad_streams = ruled_entries(oracle)
    image0 = [t[0] for t in model_table(entries)]
    assert image0 == [0, 3, 5, 6, 10, 11, 12]
    total = 16
    shapes = [(0, 20, 10, 16, 12),                     # inside A's 40 x 24
              (5, 20, 10, 16, 12),                     # 1: the same aimed at C's 8 x 8
              (3, 0, 0, 8, 8), (4, 5, 5, 9, 9),        # 2, 3: B, whose descriptor states another w
              (5, 0, 0, 8, 8), (9, 1, 0, 16, 9), (2, 24, 8, 16, 16),
              (total, 0, 0, 8, 8), (1 << 63, 0, 0, 8, 8),       # 7, 8: no stream holds them
              (10, 0, 0, 8, 8),                        # 9: nimg = 0
              (11, 0, 0, 8, 8),                        # 10: in_len = 15
              (12, 0, 0, 8, 8), (15, 1, 0, 16, 9),     # 11, 12: misaligned offsets
              (6, 16, 8, 1, 1), (1, 3, 5, 13, 7), (U64, 0, 0, 1, 1)]
    rects, cap = laid_out(shapes, per=None if resize is None else 3 * resize[0] * resize[1], gap=2)
    flips = [i & 1 for i in range(len(rects))]
    classes, res = check_equal(entries, rects, cap, T.F32, T.CHW, flips, resize=resize, skip=bad_streams)
    bad = [i for i, c in enumerate(classes) if c == T.BAD]
    assert bad == [1, 2, 3, 7, 8, 9, 10, 11, 12, 15]
    assert res == [6, 1 + 1, 0]


def test_a_table_that_is_not_ascending(gpu, oracle):
    """image0 descending, and a second table with overlapping streams: a
    rectangle is delivered from a stream that contains its index, exactly, or
    is bad, as the model's bisection says; the guards hold."""
    entries = entries_of(oracle, "ABCD")
    for image0 in ([6, 5, 3, 0], [3, 0, 6, 5], [0, 0, 2, 2]):
        table = [(g, *e.dims, True) for g, e in zip(image0, entries)]
        rects, cap = laid_out([(g, 0, 0, 8, 8) for g in list(range(11)) + [1 << 63]], gap=1)
        classes = D.tensor_verdicts(table, rects, MAX, MAX, cap)
        for rc, c in zip(rects, classes):
            at = D.locate(table, rc[0])
            assert (c == T.BAD) == (at is None)
            assert at is None or table[at[0]][0] <= rc[0] < table[at[0]][0] + table[at[0]][3]
        want, _ = single_calls(entries, rects, cap, T.F32, T.HWC, None, *IMAGENET, table=table)
        got, res = gpu_dataset(entries, rects, cap, T.F32, T.HWC, None, *IMAGENET, image0=image0)
        assert np.array_equal(got, want)
        assert res == D.result_words(classes) + [0]
    assert T.GOOD in classes and T.BAD in classes


# ---- 4. a malformed tile in one stream ---------------------------------------------------------

def test_a_malformed_tile_takes_its_own_rectangles(gpu, oracle):
    """jpr_mutations' "luma ncodes = 129" on tile 6 of A (tile (1, 1) of image
    0), and an offset of B past in_len between its tiles 6 and 7: the
    rectangles that touch those tiles are bad, each through one bad tile, so the
    count of [2] is one a rectangle in the dataset call and the single-stream
    calls alike."""
    a, b, c, d = entries_of(oracle, "ABCD")
    offs_a = host_offsets(a.data, a.dims)
    broken = bytearray(a.data)
    assert broken[int(offs_a[6]) + 1] <= 128
    broken[int(offs_a[6]) + 1] = 129
    offs_b = [int(v) for v in host_offsets(b.data, b.dims)]
    offs_b[7] = len(b.data) + 1
    assert offs_b[7] > offs_b[8]
    entries = [Entry(bytes(broken), a.dims), Entry(b.data, b.dims, offs=offs_b), c, d]
    bad_tiles = {0: {6}, 1: {6, 7}}
    shapes = [(0, 8, 8, 8, 8), (3, 0, 16, 8, 8), (5, 0, 0, 8, 8), (6, 1, 0, 16, 9),
              (0, 4, 4, 8, 8), (3, 8, 16, 8, 8), (5, 3, 2, 5, 6), (9, 9, 0, 8, 8),
              (0, 16, 8, 8, 8), (3, 16, 16, 8, 8), (1, 8, 8, 8, 8), (4, 0, 16, 8, 8),
              (0, 0, 0, 8, 8), (3, 3, 10, 8, 5), (2, 4, 4, 12, 12), (4, 4, 12, 16, 10)]
    for resize in (None, (7, 5, R.BILINEAR)):
        rects, cap = laid_out(shapes, per=None if resize is None else 105, gap=1)
        classes, res = check_equal(entries, rects, cap, T.F16, T.HWC, [i & 1 for i in range(len(rects))],
                                   resize=resize, bad_tiles=bad_tiles)
        assert [i for i, c in enumerate(classes) if c == T.BAD] == [0, 1, 4, 5]
        assert res == [12, 1, 4]


# ---- 5. dst and capacity -----------------------------------------------------------------------------

@pytest.mark.parametrize("resize", [None, (7, 5, R.TRIANGLE)], ids=["tensor", "resize"])
def test_dst_and_capacity(gpu, oracle, resize):
    """Out of order, with gaps, one rectangle ending at out_cap exactly and one
    an element past it: nothing outside the good rectangles' elements changes
    (the whole output is compared, and the guards)."""
    entries = entries_of(oracle, "ABCD")
    shapes = cycle("ABCD", {n: SHAPES[n][:3] for n in "ABCD"}, skip_empty=True)
    per = [3 * w * h if resize is None else 105 for _, _, _, w, h in shapes]
    order = [7, 2, 11, 0, 5, 9, 3, 10, 1, 8, 6, 4]      # the rectangle that comes k-th in the output
    dst, pos = [0] * len(shapes), 5
    for k, i in enumerate(order):
        dst[i] = pos
        pos += per[i] + (k % 4) * 3 + 1
    cap = pos + per[0]
    rects = [s + (d,) for s, d in zip(shapes, dst)]
    rects.append(shapes[0] + (cap - per[0],))           # ends at out_cap exactly
    rects.append(shapes[1] + (cap - per[1] + 1,))       # one element past it
    rects.append(shapes[2] + (U64 - per[2] + 1,))       # dst + its elements wraps
    classes, res = check_equal(entries, rects, cap, T.U8, T.CHW, [1] * len(rects), resize=resize)
    assert [i for i, c in enumerate(classes) if c == T.BAD] == [13, 14]
    assert res == [13, 14, 0]


# ---- 6. capture and replay --------------------------------------------------------------------------

def test_graph_replay(gpu, oracle):
    """One dataset resize call on a single stream, captured (a linear capture)
    and replayed twice, the rectangles and flips rewritten in place in
    between: each replay equals the eager call on what it then reads."""
    import torch
    from lz4jpeg import jpeg
    (a,) = entries_of(oracle, "A")
    ow, oh = 7, 5
    first = [(0, 3, 5, 13, 7), (2, 24, 8, 16, 16), (1, 0, 9, 1, 15), (3, 0, 0, 8, 8)]      # the last is bad
    second = [(2, 20, 3, 9, 16), (0, 0, 0, 16, 16), (1, 17, 8, 16, 9), (1, 33, 1, 7, 11)]
    sets = [(laid_out(first, per=105, gap=1), [1, 0, 1, 1]), (laid_out(second, per=105, gap=1), [0, 0, 1, 0])]
    cap = sets[0][0][1]
    d_stream = dev_bytes(a.data)
    d_offs, _ = jpeg.stream_index_device(d_stream, len(a.data), *a.dims)
    d_table = torch.from_numpy(jpeg.stream_table(
        [(d_stream.data_ptr(), len(a.data), d_offs.data_ptr(), 0, *a.dims)]).view(np.int64)).cuda()
    cols = [dev_u64([rc[k] for rc in sets[0][0][0]]) for k in range(6)]
    d_flip = torch.tensor(sets[0][1], dtype=torch.uint8, device="cuda")
    d_res = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(cap, dtype=torch.bfloat16, device="cuda")
    scr = torch.empty(jpeg.dataset_crop_resize_scratch_bytes(4, MAX, MAX, ow, oh), dtype=torch.uint8,
                      device="cuda")
    scale, bias = IMAGENET

    def call():
        jpeg.dataset_crop_resize_device(d_table, 1, *cols[:5], MAX, MAX, ow, oh, d_dst=cols[5], d_out=d_out,
                                        out_cap=cap, scratch=scr, d_result=d_res, check=False,
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
    for (rects, _), flips in (sets[1], sets[0]):
        for k in range(6):
            cols[k].copy_(dev_u64([rc[k] for rc in rects]))
        d_flip.copy_(torch.tensor(flips, dtype=torch.uint8, device="cuda"))
        d_out.view(torch.int16).fill_(0x5A5A)
        d_res.fill_(7)
        scr.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        want, wres = gpu_dataset([a], rects, cap, T.BF16, T.HWC, flips, scale, bias, resize=(ow, oh, R.TRIANGLE))
        assert np.array_equal(d_out.view(torch.int16).cpu().numpy().view(np.uint16), want)
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == wres
    assert wres == [3, 4, 0]                                # the first set, replayed last: rectangle 3 is bad


# ---- 7. Dataset ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_dataset_batches(gpu, oracle, dtype):
    """crop_batch and resized_crop_batch equal the per-reader results put
    together in rectangle order."""
    import torch
    from lz4jpeg import jpeg
    dtype = getattr(torch, dtype)
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    readers = [jpeg.StreamReader(dev_bytes(e.data)) for e in entries_of(oracle, "ABCD")]
    ds = jpeg.Dataset(readers)
    assert ds.nimg == 10 and ds.image0.tolist() == [0, 3, 5, 6] and (ds.max_w, ds.max_h) == (40, 40)
    assert ds.sizes.tolist() == [list(DIMS[n][:2]) for n in "ABCD" for _ in range(DIMS[n][2])]
    shapes = [(g, x % (ds.sizes[g][0] - 7), y % (ds.sizes[g][1] - 7), 3 + (g + k) % 6, 2 + (3 * g + k) % 7)
              for k, (g, x, y) in enumerate([(9, 3, 1), (0, 30, 11), (5, 0, 0), (3, 9, 20), (2, 7, 7), (6, 5, 0),
                                             (4, 13, 31), (1, 0, 16), (5, 0, 0), (8, 2, 1), (0, 1, 2)])]
    n = len(shapes)
    stream = [int(np.searchsorted(ds.image0, s[0], side="right")) - 1 for s in shapes]
    cols = [dev_u64([s[k] for s in shapes]) for k in range(5)]
    d_flip = torch.tensor([k % 3 == 0 for k in range(n)], device="cuda")

    def per_reader(fn):
        """fn(reader, rows, local columns, flips) -> that reader's batch, scattered to the rectangles' places"""
        parts = [None] * n
        for s, rd in enumerate(readers):
            rows = [k for k in range(n) if stream[k] == s]
            local = [dev_u64([shapes[k][0] - int(ds.image0[s]) for k in rows])]
            local += [dev_u64([shapes[k][c] for k in rows]) for c in range(1, 5)]
            out = fn(rd, local, d_flip[rows])
            for j, k in enumerate(rows):
                parts[k] = out[j]
        return torch.stack(parts)

    kw = dict(dtype=dtype, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD)
    for layout, shape in (("chw", (n, 3, 6, 5)), ("hwc", (n, 6, 5, 3))):
        got = ds.crop_batch(*cols[:3], 5, 6, layout=layout, d_flip=d_flip, **kw)
        want = per_reader(lambda rd, loc, fl: rd.crop_batch(*loc[:3], 5, 6, layout=layout, d_flip=fl, **kw))
        assert got.shape == shape and got.dtype == dtype and got.is_contiguous()
        assert torch.equal(got.view(ints), want.view(ints))
    for layout, shape in (("chw", (n, 3, 12, 20)), ("hwc", (n, 12, 20, 3))):
        got = ds.resized_crop_batch(*cols, 20, 12, layout=layout, d_flip=d_flip, **kw)
        want = per_reader(lambda rd, loc, fl: rd.resized_crop_batch(*loc, 20, 12, layout=layout, d_flip=fl, **kw))
        assert got.shape == shape and got.dtype == dtype and got.is_contiguous()
        assert torch.equal(got.view(ints), want.view(ints))
        same = ds.resized_crop_batch(*cols, 20, 12, layout=layout, d_flip=d_flip, max_w=8, max_h=8, **kw)
        assert torch.equal(got.view(ints), same.view(ints))
    cols[0] = dev_u64([s[0] for s in shapes[:4]] + [10] + [s[0] for s in shapes[5:]])
    with pytest.raises(jpeg.JpegError, match="jpegr_dataset_crop_resize_device: rectangle 4"):
        ds.crops_resized(*cols, 20, 12)
