"""jpegr_stream_index_device and jpegr_crop_device (include/jpegr.h) on the GPU:
the kept index against the host's cumulative sum, and crops byte for byte
against the slice of what the existing path (decompress_images_device of the
same stream) gives for the whole image.  Verdicts and expected bytes come from
jpr_crop_model.py (checked by test_jpr_crop_model.py); every call's output lies
between guard bands in a sentinel-filled tensor and the whole tensor is
compared, so the gaps between crops and the guards must stay as they were."""
import functools

import numpy as np
import pytest

import jpr_crop_model as M
from jpr_gpu_lib import (FILL, GUARD, U64, dev_bytes, dev_u64, encoded_jpr, host_offsets, image,
                         jpr_mutations)

pytestmark = pytest.mark.gpu

KINDS = [("rand", False), ("rand", True), ("smooth", False), ("smooth", True)]
BIG, SMALL = (520, 520, 2), (13, 11, 3)


# ---- streams and drivers ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def stream_of(oracle, dims, kind, tight):
    """(the stream's bytes, the existing path's pixels [nimg, h, w, 4]) of nimg
    different images.  Shared: read, do not change."""
    import torch
    from lz4jpeg import jpeg
    w, h, nimg = dims
    imgs = [np.roll(image(oracle, w, h, kind, seed=1 + i), 5 * i, axis=1) for i in range(nimg)]
    d_img = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).cuda().reshape(-1)
    d_stream = jpeg.compress_device(d_img, w, h, nimg, tight=tight)
    return d_stream.cpu().numpy().tobytes(), full_of(d_stream)


def full_of(d_stream):
    from lz4jpeg import jpeg
    full, w, h, nimg = jpeg.decompress_images_device(d_stream)
    return full.cpu().numpy().reshape(nimg, h, w, 4)


def gpu_index(data, in_len, dims):
    """(offsets as uint64 [ntiles + 1], [implied, verdict] unsigned); the offsets lie
    between sentinels, the result starts as garbage."""
    import torch
    from lz4jpeg import jpeg
    nt = dims[2] * jpeg.tiles(dims[0], dims[1])
    big = torch.full((nt + 1 + 16,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    res = torch.full((2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    offs, r = jpeg.stream_index_device(dev_bytes(data), in_len, *dims, d_offsets=big[8:8 + nt + 1],
                                       d_result=res)
    torch.cuda.synchronize()
    host = big.cpu().numpy().view(np.uint64)
    assert (host[:8] == 0x5A5A5A5A5A5A5A5A).all() and (host[-8:] == 0x5A5A5A5A5A5A5A5A).all()
    return host[8:-8].copy(), [int(x) & U64 for x in res.cpu().tolist()]


def place(shapes, gap=8, slot=None):
    """dst of rectangles laid out one after another, `gap` bytes apart (a
    multiple of 4 that is not one of 16: both store widths get used).  A
    rectangle takes 4 w h bytes, or `slot` bytes where given (one that is meant
    to fail and must write nothing).  Returns (dsts, out_cap)."""
    dsts, pos = [], 0
    for i, (_, _, _, w, h) in enumerate(shapes):
        dsts.append(pos)
        pos += (slot[i] if slot and slot[i] is not None else 4 * w * h) + gap
    return dsts, pos


def gpu_crops(data, dims, rects, max_w, max_h, out_cap, offs=None, in_len=None, **kw):
    """(the call's out_cap output bytes, [delivered, verdict, rejected] unsigned):
    d_out is a view between 4-KiB guards of a tensor filled with 0x5A, the
    guards are checked here; the stream buffer is exactly the stream; the
    offsets are the index call's unless given; d_result starts as garbage."""
    import torch
    from lz4jpeg import jpeg
    in_len = len(data) if in_len is None else in_len
    d_stream = dev_bytes(data)
    if offs is None:
        d_offs, _ = jpeg.stream_index_device(d_stream, in_len, *dims)
    else:
        d_offs = dev_u64(offs)
    big = torch.full((2 * GUARD + out_cap,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    cols = [dev_u64([rc[k] for rc in rects]) for k in range(6)]
    d_out, _, n = jpeg.crop_device(d_stream, in_len, *dims, d_offs, *cols[:5], max_w, max_h,
                                   d_dst=cols[5], d_out=big[GUARD:GUARD + out_cap], out_cap=out_cap,
                                   d_result=res, check=False, **kw)
    torch.cuda.synchronize()
    assert n is None and d_out.data_ptr() == big.data_ptr() + GUARD
    host = big.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + out_cap:] == FILL).all(), "guards"
    return host[GUARD:GUARD + out_cap].copy(), [int(x) & U64 for x in res.cpu().tolist()]


def check_call(data, full, dims, rects, max_w, max_h, out_cap, bad_tiles=(), offs=None,
               header_ok=True, in_len=None):
    """One call against the model: every byte of the output (the unspecified
    ones of rectangles with a failed tile aside) and the result words.  Returns
    the classes and the result."""
    w, h, nimg = dims
    own = M.verdicts(rects, w, h, nimg, max_w, max_h, out_cap, header_ok=header_ok)
    classes = M.verdicts(rects, w, h, nimg, max_w, max_h, out_cap, bad_tiles, header_ok=header_ok)
    want, loose = M.expected(full, rects, classes, own, np.full(out_cap, FILL, np.uint8))
    got, res = gpu_crops(data, dims, rects, max_w, max_h, out_cap, offs=offs, in_len=in_len)
    diff = np.flatnonzero((got != want) & ~loose)
    assert diff.size == 0, f"{diff.size} bytes differ, the first at {int(diff[0])}"
    assert res[:2] == M.result_words(classes), (res, M.result_words(classes))
    return classes, res


# ---- the index ----------------------------------------------------------------------

@pytest.mark.parametrize("kind,tight", KINDS)
@pytest.mark.parametrize("dims", [BIG, SMALL])
def test_index(gpu, oracle, dims, kind, tight):
    """520 x 520 x 2: 4,225 tiles an image, so a 4,096-tile scan partial ends
    inside image 0 and another at 8,192 inside image 1; 13 x 11 x 3: 2 x 2 tiles,
    both edges partial."""
    data, _ = stream_of(oracle, dims, kind, tight)
    want = host_offsets(data, dims)
    offs, res = gpu_index(data, len(data), dims)
    assert np.array_equal(offs, want)
    assert int(offs[-1]) == len(data) and res == [len(data), U64]


@pytest.mark.parametrize("tight", [False, True])
def test_index_verdict_0(gpu, oracle, tight):
    data, _ = stream_of(oracle, BIG, "rand", tight)
    w, h, nimg = BIG
    want = host_offsets(data, BIG)
    offs, res = gpu_index(data, len(data) - 1, BIG)
    assert res == [len(data), 0] and np.array_equal(offs, want)        # the index is whole
    wrong_magic = b"K" + data[1:]
    assert gpu_index(wrong_magic, len(data), BIG)[1] == [len(data), 0]
    other_h = data[:8] + (h + 8).to_bytes(4, "little") + data[12:]
    assert gpu_index(other_h, len(data), BIG)[1] == [len(data), 0]
    assert gpu_index(data, len(data), (w, h + 8, nimg))[1][1] == 0      # the argument differs


# ---- exact crops ----------------------------------------------------------------------

def edge_rects():
    """The fixed list on 520 x 520 x 2 (65 x 65 tiles an image), w, h <= 64 x 48."""
    shapes = []
    for im in (0, 1):                                                  # 1 x 1 at each corner
        shapes += [(im, 0, 0, 1, 1), (im, 519, 0, 1, 1), (im, 0, 519, 1, 1), (im, 519, 519, 1, 1)]
    shapes += [(0, 13, 21, 37, 9),                                     # odd x, odd w
               (0, 4, 504, 8, 8),                                      # raster tiles 4095 | 4096
               (0, 1, 499, 17, 13),                                    # the same pair, two rows of it
               (1, 100, 200, 64, 48),                                  # image 1 only
               (1, 499, 503, 21, 17),                                  # the last column and row
               (0, 512, 512, 8, 8), (1, 456, 472, 64, 48),
               (0, 40, 40, 30, 20), (0, 44, 47, 30, 20),               # sharing tiles
               (1 << 60, U64, 7, 0, 5), (0, 1 << 63, U64 - 2, 9, 0),   # empty, garbage elsewhere
               (0, 7, 7, 64, 48), (0, 8, 8, 64, 48), (0, 1, 0, 63, 47)]
    return shapes


@pytest.mark.parametrize("kind,tight", KINDS)
def test_exact_edges(gpu, oracle, kind, tight):
    data, full = stream_of(oracle, BIG, kind, tight)
    shapes = edge_rects()
    dsts, cap = place(shapes)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    rects[-5] = rects[-5][:5] + (3,)                                   # an empty one's dst is garbage too
    classes, res = check_call(data, full, BIG, rects, 64, 48, cap)
    assert classes.count(M.EMPTY) == 2 and M.BAD not in classes
    assert res == [len(rects), U64, 0]


@pytest.mark.parametrize("kind,tight", [("rand", True), ("smooth", False)])
def test_exact_whole_image(gpu, oracle, kind, tight):
    """A whole image in one rectangle (max_w = max_h = 520: K = 66 x 66 items a
    rectangle), beside a small one that idles nearly all of its items."""
    data, full = stream_of(oracle, BIG, kind, tight)
    shapes = [(1, 0, 0, 520, 520), (0, 259, 261, 3, 2), (0, 0, 0, 520, 520)]
    dsts, cap = place(shapes)
    _, res = check_call(data, full, BIG, [s + (d,) for s, d in zip(shapes, dsts)], 520, 520, cap)
    assert res == [3, U64, 0]


@pytest.mark.parametrize("kind,tight", KINDS)
def test_exact_random(gpu, oracle, kind, tight):
    """200 seeded rectangles with w <= 64 and h <= 48, valid by construction."""
    data, full = stream_of(oracle, BIG, kind, tight)
    rng = np.random.default_rng(2024)
    shapes = []
    for _ in range(200):
        w, h = int(rng.integers(1, 65)), int(rng.integers(1, 49))
        shapes.append((int(rng.integers(0, 2)), int(rng.integers(0, 520 - w + 1)),
                       int(rng.integers(0, 520 - h + 1)), w, h))
    dsts, cap = place(shapes)
    _, res = check_call(data, full, BIG, [s + (d,) for s, d in zip(shapes, dsts)], 64, 48, cap)
    assert res == [200, U64, 0]


@pytest.mark.parametrize("kind,tight", KINDS)
def test_every_rectangle_of_a_small_image(gpu, oracle, kind, tight):
    """13 x 11 x 3: every rectangle of every size at every position, 18,018 of
    them, in four calls grouped by whether w and h exceed a tile."""
    data, full = stream_of(oracle, SMALL, kind, tight)
    total = 0
    for ws, hs in ((range(1, 9), range(1, 9)), (range(9, 14), range(1, 9)),
                   (range(1, 9), range(9, 12)), (range(9, 14), range(9, 12))):
        shapes = [(im, x, y, w, h) for im in range(3) for w in ws for h in hs
                  for x in range(13 - w + 1) for y in range(11 - h + 1)]
        dsts, cap = place(shapes, gap=4)
        _, res = check_call(data, full, SMALL, [s + (d,) for s, d in zip(shapes, dsts)],
                            ws[-1], hs[-1], cap)
        assert res == [len(shapes), U64, 0]
        total += len(shapes)
    assert total == 18018


# ---- bad rectangles, bad tiles, bad offsets ---------------------------------------------

def test_bad_rectangles_among_good_ones(gpu, oracle):
    """One of each failure of a rectangle's own fields, at known indices among
    good ones: they write nothing, the good ones are exact."""
    data, full = stream_of(oracle, BIG, "rand", False)
    good = [(0, 3, 5, 20, 10), (1, 500, 500, 20, 20), (0, 100, 7, 64, 48), (1, 33, 44, 5, 6)]
    bad = {2: (2, 0, 0, 8, 8),                      # image >= nimg
           3: (0, 0, 0, 65, 8),                     # w > max_w
           5: (0, 0, 0, 8, 49),                     # h > max_h
           6: (0, 513, 0, 8, 8),                    # x + w > W
           7: (1, 0, 519, 8, 2),                    # y + h > H
           8: (0, U64, 0, 2, 2),                    # x + w wraps
           9: (0, 0, U64 - 1, 2, 3),                # y + h wraps
           11: (0, 0, 0, 8, 8)}                     # dst: below
    shapes, it = [], iter(good)
    for i in range(len(good) + len(bad) + 3):
        shapes.append(bad[i] if i in bad else next(it, (0, 8 * i, 8 * i, 7, 5)))
    dsts, cap = place(shapes, slot=[64 if i in bad else None for i in range(len(shapes))])
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    rects[11] = rects[11][:5] + (dsts[11] + 2,)                         # dst not a multiple of 4
    rects.append((0, 0, 0, 8, 8, cap - 4 * 64 + 4))                     # dst + 4 w h = out_cap + 4
    rects.append((0, 0, 0, 8, 8, U64 - 3))                              # dst + 4 w h wraps
    rects.append((0, 0, 0, 8, 8, 1 << 40))                              # dst past out_cap
    classes, res = check_call(data, full, BIG, rects, 64, 48, cap)
    assert [i for i, c in enumerate(classes) if c == M.BAD] == sorted(bad) + [15, 16, 17]
    assert res == [7, 1 + 2, 0]


def test_wrong_header_makes_every_rectangle_bad(gpu, oracle):
    data, full = stream_of(oracle, BIG, "rand", False)
    shapes = [(0, 3, 5, 20, 10), (1, 0, 0, 0, 0), (1, 500, 500, 20, 20)]
    dsts, cap = place(shapes)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    offs = host_offsets(data, BIG)
    for broken in (b"K" + data[1:], data[:12] + (3).to_bytes(4, "little") + data[16:]):
        _, res = check_call(broken, full, BIG, rects, 64, 48, cap, offs=offs, header_ok=False)
        assert res == [0, 1, 0]


def strip_rects():
    """Rectangles on a 520 x 8 image (65 tiles in a row): four touch tile 40
    (columns 320 .. 327), two tile 64 (512 .. 519)."""
    return [(0, 300, 0, 20, 8), (0, 318, 2, 8, 4), (0, 320, 0, 8, 8), (0, 327, 7, 1, 1),
            (0, 328, 0, 64, 8), (0, 505, 0, 7, 8), (0, 500, 3, 20, 5), (0, 519, 0, 1, 8),
            (0, 0, 0, 64, 8), (0, 263, 1, 64, 6)]


def check_strip(data, full, bad_tiles):
    dims = (520, 8, 1)
    shapes = strip_rects()
    dsts, cap = place(shapes)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    classes, res = check_call(data, full, dims, rects, 64, 8, cap, bad_tiles=bad_tiles)
    assert M.BAD in classes and M.GOOD in classes and res[2] > 0
    return classes


def test_bad_records(gpu, oracle):
    """jpr_mutations' two record mutations on the 65-tile stream: rectangles
    that touch the tile are bad, the others exact."""
    import torch
    good = encoded_jpr(65)
    full = full_of(dev_bytes(good))
    torch.cuda.synchronize()
    muts = [m for m in jpr_mutations(good) if m[4] is not None]
    assert [m[4] for m in muts] == [40, 64]
    for name, data, in_len, _, tile in muts:
        assert in_len == len(data)
        classes = check_strip(data, full, {tile})
        assert classes.count(M.BAD) == (4 if tile == 40 else 2), name


def test_bad_mode_in_a_tight_stream(gpu, oracle):
    """A JPT1 stream whose tile 40 has a luma mode field of 3."""
    data, full = stream_of(oracle, (520, 8, 1), "rand", True)
    assert data[:4] == b"JPT1"
    y40 = int(host_offsets(data, (520, 8, 1))[40])
    broken = data[:y40 + 3] + bytes([data[y40 + 3] | 0xC0]) + data[y40 + 4:]
    check_strip(broken, full, {40})


def test_untrusted_offsets(gpu, oracle):
    """A good stream with a perturbed offsets array: rectangles touching a tile
    whose offsets fail the bounds are bad, the others exact, nothing is read or
    written out of bounds (the stream buffer is exactly the stream)."""
    data, full = stream_of(oracle, BIG, "rand", False)
    offs = [int(v) for v in host_offsets(data, BIG)]
    n = len(data)
    row = 65

    def tile(tx, ty, im=0):
        return (im * 65 + ty) * row + tx

    e1, e2, e3, e4, e5 = tile(10, 5), tile(30, 12), tile(20, 30), tile(50, 40), tile(5, 60, 1)
    offs[e1] = n + 1                                    # past in_len: tiles e1 - 1 and e1
    offs[e2], offs[e2 + 1] = offs[e2 + 1], offs[e2]     # a decreasing pair: tile e2
    offs[e3] = offs[e3 - 1] + 1037                      # a size of 1,037: tile e3 - 1
    offs[e4] = offs[e4 - 1] + 11                        # a size of 11: tile e4 - 1
    offs[e5] = U64                                      # all ones: tiles e5 - 1 and e5
    by_bounds = M.bad_offset_tiles(offs, n)
    assert {e1 - 1, e1, e2, e3 - 1, e4 - 1, e5 - 1, e5} <= by_bounds
    # the neighbours whose offsets pass the bounds but whose bytes are not a
    # record: two records taken for one (the streams sum to less than the
    # size), or a record entered 11 bytes in
    bad_tiles = by_bounds | {e2 - 1, e2 + 1, e3, e4}
    shapes = [(0, 8 * 10, 8 * 5, 8, 8), (0, 8 * 9 - 3, 8 * 5 - 3, 4, 4), (0, 8 * 11, 8 * 5, 64, 48),
              (0, 8 * 30 + 1, 8 * 12 + 1, 5, 5), (0, 8 * 29, 8 * 12, 8, 8), (0, 8 * 31, 8 * 12, 8, 8),
              (0, 8 * 32, 8 * 12, 8, 8), (0, 8 * 26, 8 * 13, 64, 48),
              (0, 8 * 19, 8 * 30, 8, 8), (0, 8 * 20, 8 * 30, 8, 8), (0, 8 * 21, 8 * 30, 60, 8),
              (0, 8 * 49, 8 * 40, 8, 8), (0, 8 * 50 + 7, 8 * 40, 1, 1), (0, 8 * 51, 8 * 40, 8, 8),
              (1, 8 * 4, 8 * 60, 16, 8), (1, 8 * 6, 8 * 60, 8, 8), (0, 8 * 5, 8 * 60, 8, 8),
              (1, 0, 0, 64, 48), (0, 456, 472, 64, 48)]
    dsts, cap = place(shapes)
    rects = [s + (d,) for s, d in zip(shapes, dsts)]
    classes, res = check_call(data, full, BIG, rects, 64, 48, cap, bad_tiles=bad_tiles, offs=offs)
    assert [c == M.BAD for c in classes] == [True, True, False, True, True, True, False, False,
                                             True, True, False, True, True, False, True, False,
                                             False, False, False]
    assert res[2] > 0


# ---- replay, check=False, StreamReader ----------------------------------------------------

def test_graph_replay(gpu, oracle):
    """The index and crop pair captured once and replayed twice, the rectangles
    rewritten in place in between: both exact, no counter accumulates."""
    import torch
    from lz4jpeg import jpeg
    data, full = stream_of(oracle, BIG, "rand", True)
    d_stream = dev_bytes(data)
    nt = 2 * jpeg.tiles(520, 520)
    sets = [[(0, 13, 21, 37, 9), (1, 499, 503, 21, 17), (0, 0, 0, 0, 3), (0, 4, 504, 8, 8)],
            [(1, 0, 0, 64, 48), (0, 600, 0, 8, 8), (1, 7, 9, 33, 31), (0, 511, 511, 9, 9)]]
    dsts, cap = place([(0, 0, 0, 64, 48)] * 4)
    cols = [torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(5)]
    d_dst = dev_u64(dsts)
    d_offs = torch.zeros(nt + 1, dtype=torch.int64, device="cuda")
    d_ires = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    d_res = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    iscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device="cuda")
    cscr = torch.empty(jpeg.crop_scratch_bytes(4, 64, 48), dtype=torch.uint8, device="cuda")

    def call():
        jpeg.stream_index_device(d_stream, len(data), *BIG, d_offsets=d_offs, d_result=d_ires,
                                 scratch=iscr)
        jpeg.crop_device(d_stream, len(data), *BIG, d_offs, *cols, 64, 48, d_dst=d_dst, d_out=d_out,
                         out_cap=cap, scratch=cscr, d_result=d_res, check=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # warm-up: four empty rectangles
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for shapes in sets:
        for k in range(5):
            cols[k].copy_(dev_u64([s[k] for s in shapes]))
        d_out.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        rects = [s + (d,) for s, d in zip(shapes, dsts)]
        classes = M.verdicts(rects, *BIG, 64, 48, cap)
        want, _ = M.expected(full, rects, classes, classes, np.full(cap, FILL, np.uint8))
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == M.result_words(classes) + [0]
        assert [int(x) & U64 for x in d_ires.cpu().tolist()] == [len(data), U64]
    assert M.result_words(classes) == [3, 2]                # the second set: rectangle 1 is bad


def test_wrappers(gpu, oracle):
    """crop_device's defaults (packed back to back, check=True and check=False
    give the same bytes), its JpegError naming the first bad rectangle, and
    StreamReader."""
    import torch
    from lz4jpeg import jpeg
    data, full = stream_of(oracle, BIG, "smooth", True)
    d_stream = dev_bytes(data)
    rd = jpeg.StreamReader(d_stream)
    assert (rd.w, rd.h, rd.nimg, rd.tight) == (520, 520, 2, True)
    assert np.array_equal(rd.d_offsets.cpu().numpy().view(np.uint64), host_offsets(data, BIG))
    for im, x, y, w, h in ((1, 13, 21, 37, 9), (0, 0, 0, 520, 520), (1, 519, 519, 1, 1)):
        got = rd.crop(im, x, y, w, h)
        assert got.shape == (h, w, 4) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), full[im, y:y + h, x:x + w])
    assert rd.crop(0, 5, 5, 0, 7).shape == (7, 0, 4)
    with pytest.raises(jpeg.JpegError, match="rectangle 0"):
        rd.crop(0, 519, 0, 2, 1)
    shapes = [(0, 13, 21, 37, 9), (1, 499, 503, 21, 17), (0, 0, 0, 0, 3), (0, 4, 504, 8, 8)]
    cols = [dev_u64([s[k] for s in shapes]) for k in range(5)]
    d_a, d_dst, n = rd.crops(*cols, 64, 48)
    assert n == 4 and d_dst.cpu().tolist() == [0, 4 * 333, 4 * (333 + 357), 4 * (333 + 357)]
    d_b, _, none = rd.crops(*cols, 64, 48, check=False, out_cap=d_a.numel())
    torch.cuda.synchronize()
    assert none is None and torch.equal(d_a, d_b[:d_a.numel()])
    want = np.concatenate([full[im, y:y + h, x:x + w].reshape(-1) for im, x, y, w, h in shapes])
    assert np.array_equal(d_a.cpu().numpy(), want)
    cols[1] = dev_u64([13, 499, 0, 514])
    with pytest.raises(jpeg.JpegError, match="rectangle 3"):
        rd.crops(*cols, 64, 48)
    with pytest.raises(jpeg.JpegError):
        jpeg.StreamReader(d_stream[:-1])
