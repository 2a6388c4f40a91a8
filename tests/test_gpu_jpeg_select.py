"""jpegr_select_device (include/jpegr.h) on the GPU: subsets, windows and
re-codings of a stream byte for byte against compress_device of the same
images (the encoder's coefficients of a tile-aligned window are the whole
image's) and against jpr_select_model.py (checked by test_jpr_select_model.py);
every call's output lies between guard bands in a tensor filled with 0x5A and
the bytes past the capacity are checked too."""
import functools

import numpy as np
import pytest

import jpr_format as J
import jpr_select_model as M
import jpt_format as T
import jpt_inputs as I
from jpr_gpu_lib import FILL, GUARD, U64, crafted, dev_bytes, dev_u64, image

pytestmark = pytest.mark.gpu

KINDS = [("rand", False), ("rand", True), ("smooth", False), ("smooth", True)]
A, B, SMALL, BIG = (72, 40, 5), (61, 43, 3), (24, 16, 2), (264, 264, 4)
GARBAGE = 0x5A5A5A5A5A5A5A5A


# ---- streams and drivers ----------------------------------------------------------

def compress(imgs, tight):
    """compress_device of images [n, h, w, 4], as bytes."""
    import torch
    from lz4jpeg import jpeg
    n, h, w, _ = imgs.shape
    d = torch.from_numpy(np.array(imgs)).cuda().reshape(-1)
    return jpeg.compress_device(d, w, h, n, tight=tight).cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def images_of(oracle, dims, kind):
    """nimg different images [nimg, h, w, 4].  Shared: read, do not change."""
    w, h, nimg = dims
    a = np.stack([np.roll(image(oracle, w, h, kind, seed=1 + i), 5 * i, axis=1) for i in range(nimg)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def stream_of(oracle, dims, kind, tight):
    return compress(images_of(oracle, dims, kind), tight)


def fmt_of(tight):
    return 0 if tight is None else M.JPT1 if tight else M.JPR1


def gpu_select(data, dims, items, out_w, out_h, tight=None, cap=None, offs=None, in_len=None, lead=0,
               room=None):
    """(the call's first cap output bytes, [length, verdict, empties] unsigned, the
    u64 at d_out_len): d_out is a view between 4-KiB guards of a tensor filled
    with 0x5A; the guards and the bytes from cap to the view's end are checked
    here.  The stream sits `lead` bytes into a buffer of other bytes; the offsets
    are the index call's unless given; d_result and d_out_len start as garbage."""
    import torch
    from lz4jpeg import jpeg
    in_len = len(data) if in_len is None else in_len
    buf = dev_bytes(bytes([0xA5]) * lead + bytes(data) + bytes([0xC3]) * 37)
    d_stream = buf[lead:lead + len(data)]
    if offs is None:
        d_offs, _ = jpeg.stream_index_device(d_stream, in_len, *dims)
    else:
        d_offs = dev_u64(offs)
    if room is None:
        room = jpeg.pack_bound(out_w, out_h, len(items))
    cap = room if cap is None else cap
    big = torch.full((2 * GUARD + room,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((3,), GARBAGE, dtype=torch.int64, device="cuda")
    d_len = torch.full((1,), GARBAGE, dtype=torch.int64, device="cuda")
    cols = [dev_u64([it[k] for it in items]) for k in range(3)]
    jpeg.select_device(d_stream, in_len, *dims, d_offs, *cols, out_w, out_h, tight=tight,
                       d_out=big[GUARD:GUARD + room], cap=cap, d_len=d_len, d_result=res)
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + cap:] == FILL).all(), "bytes at or past cap"
    return (host[GUARD:GUARD + cap].tobytes(), [int(x) & U64 for x in res.cpu().tolist()],
            int(d_len.item()) & U64)


def check_model(data, dims, items, out_w, out_h, tight=None, **kw):
    """One call against the model: the bytes, the result words and the length."""
    want, words, modes = M.select(data, dims, kw.get("offs") or M.offsets_of(data, dims), items, out_w,
                                  out_h, fmt_of(tight), in_len=kw.get("in_len"))
    got, res, n = gpu_select(data, dims, items, out_w, out_h, tight, **kw)
    assert res == words and n == words[0], (res, words, n)
    assert got[:n] == want, first_difference(got[:n], want)
    return want, res, modes


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return f"lengths {len(a)}, {len(b)}; the first difference at {int(d[0]) if d.size else n}"


def whole(images):
    return [(im, 0, 0) for im in images]


# ---- exact bytes ------------------------------------------------------------------------

@pytest.mark.parametrize("kind,tight", KINDS)
@pytest.mark.parametrize("dims", [A, B])
def test_identity(gpu, oracle, dims, kind, tight):
    """72 x 40 x 5: 225 tiles, four scan groups and a partial run; 61 x 43 x 3: odd edges."""
    data = stream_of(oracle, dims, kind, tight)
    for target in (None, tight):
        got, res, n = gpu_select(data, dims, whole(range(dims[2])), dims[0], dims[1], target)
        assert got[:n] == data and res == [len(data), U64, 0]


@pytest.mark.parametrize("kind", ["rand", "smooth"])
@pytest.mark.parametrize("src,target", [(False, None), (False, True), (True, False), (True, None)])
def test_subset_bytes(gpu, oracle, kind, src, target):
    order = [3, 0, 0, 4]
    data = stream_of(oracle, A, kind, src)
    want = compress(images_of(oracle, A, kind)[order], src if target is None else target)
    got, res, n = gpu_select(data, A, whole(order), A[0], A[1], target)
    assert got[:n] == want, first_difference(got[:n], want)
    assert res == [len(want), U64, 0]


@pytest.mark.parametrize("kind", ["rand", "smooth"])
@pytest.mark.parametrize("src,target", [(False, None), (False, True), (True, False), (True, None)])
def test_window_bytes(gpu, oracle, kind, src, target):
    """Windows of whole tiles, and windows that reach the right and bottom edge
    of a 61 x 43 image: the bytes of compress_device of the cropped images."""
    for dims, items, ow, oh in ((A, [(1, 8, 16), (4, 48, 0), (0, 0, 24), (1, 8, 16)], 24, 16),
                                (B, [(2, 40, 24), (0, 40, 24)], 21, 19),
                                (B, [(1, 0, 24), (2, 16, 24)], 40, 19),
                                (B, [(1, 40, 0), (1, 40, 8)], 21, 32)):
        imgs = images_of(oracle, dims, kind)
        crops = np.stack([imgs[im, y:y + oh, x:x + ow] for im, x, y in items])
        want = compress(crops, src if target is None else target)
        got, res, n = gpu_select(stream_of(oracle, dims, kind, src), dims, items, ow, oh, target)
        assert got[:n] == want, (dims, first_difference(got[:n], want))
        assert res == [len(want), U64, 0]


@pytest.mark.parametrize("kind,tight", KINDS)
def test_window_that_ends_inside_a_tile(gpu, oracle, kind, tight):
    """out_w and out_h that are no multiple of 8, in the interior: the output
    decodes to that rectangle of the decoded source."""
    from lz4jpeg import jpeg
    data = stream_of(oracle, A, kind, tight)
    full, w, h, nimg = jpeg.decompress_images_device(dev_bytes(data))
    full = full.cpu().numpy().reshape(nimg, h, w, 4)
    items, ow, oh = [(2, 8, 8), (0, 32, 16), (4, 0, 0)], 20, 13
    for target in (None, not tight):
        got, res, n = gpu_select(data, A, items, ow, oh, target)
        assert res[1:] == [U64, 0]
        px, gw, gh, gn = jpeg.decompress_images_device(dev_bytes(got[:n]))
        assert (gw, gh, gn) == (ow, oh, len(items))
        want = np.stack([full[im, y:y + oh, x:x + ow] for im, x, y in items])
        assert np.array_equal(px.cpu().numpy().reshape(gn, oh, ow, 4), want)


@pytest.mark.parametrize("tight", [False, True])
def test_every_window_of_a_small_source(gpu, oracle, tight):
    """24 x 16 x 2 (3 x 2 tiles an image): every out_w x out_h at every
    tile-aligned position of both images, a call per size, the target format
    by turns the source's, JPR1 and JPT1."""
    data = stream_of(oracle, SMALL, "rand", tight)
    offs = M.offsets_of(data, SMALL)
    calls = 0
    for ow in range(1, 25):
        for oh in range(1, 17):
            items = [(im, x, y) for im in (1, 0) for y in range(0, 16 - oh + 1, 8)
                     for x in range(0, 24 - ow + 1, 8)]
            _, res, _ = check_model(data, SMALL, items, ow, oh, (None, False, True)[(ow + oh) % 3],
                                    offs=offs)
            assert res[1:] == [U64, 0]
            calls += 1
    assert calls == 384


@pytest.mark.parametrize("count,items,ow,oh", [
    (1, [(4, 64, 32)], 8, 8), (15, [(2, 16, 8)], 40, 24), (16, [(0, 40, 8)], 32, 32),
    (17, [(k % 5, 8 * (k % 9), 8 * (k % 4)) for k in range(17)], 8, 8),
    (64, [(1, 0, 0), (3, 40, 8), (1, 8, 0), (0, 32, 8)], 32, 32),
    (65, [(k % 5, 8 * (k % 5), 8 * (k % 5)) for k in range(13)], 40, 8)])
@pytest.mark.parametrize("tight,target", [(False, None), (False, True), (True, False)])
def test_output_tile_counts(gpu, oracle, count, items, ow, oh, tight, target):
    assert len(items) * ((ow + 7) // 8) * ((oh + 7) // 8) == count
    _, res, _ = check_model(stream_of(oracle, A, "rand", tight), A, items, ow, oh, target)
    assert res[1:] == [U64, 0]


@pytest.mark.parametrize("tight,target", [(False, None), (False, True), (True, False)])
def test_output_crosses_a_scan_partial(gpu, oracle, tight, target):
    """4 images of 264 x 264 (1,089 tiles each, 4,356 in the source) selected
    five times: 5,445 output tiles, so tile 4,096 starts a scan partial on the
    output side while the source crosses one of its own."""
    data = stream_of(oracle, BIG, "rand", tight)
    _, res, _ = check_model(data, BIG, whole([3, 0, 2, 1, 3]), 264, 264, target)
    assert res[1:] == [U64, 0]


def test_crafted_batch(gpu, oracle):
    """704 tiles in one row with code lengths over 15 and wide values (records
    up to 988 B; test_edge_tables has the 1,036-B one): column ranges re-coded both ways are the restatements' packs of the
    same tiles' slot arrays."""
    arrays, _, dims = crafted(oracle)
    plain, tight = J.pack(*arrays, *dims), T.pack(*arrays, *dims)
    seen = set()
    for x0, ncol in ((0, 704), (96, 37), (431, 65), (703, 1)):
        sub = M.sub_arrays(arrays, range(x0, x0 + ncol))
        items, odims = [(0, 8 * x0, 0)], (8 * ncol, 8, 1)
        got, res, n = gpu_select(plain, dims, items, 8 * ncol, 8, True)
        want = T.pack(*sub, *odims)
        assert got[:n] == want and res == [len(want), U64, 0], first_difference(got[:n], want)
        got, res, n = gpu_select(tight, dims, items, 8 * ncol, 8, False)
        want = J.pack(*sub, *odims)
        assert got[:n] == want and res == [len(want), U64, 0], first_difference(got[:n], want)
        seen |= set(T.stream_modes(*sub).reshape(-1).tolist())
    assert seen == {0, 1, 2}


def test_edge_tables(gpu):
    """jpt_inputs.edge_slots: 16 tiles on every edge of the mode rule, one of
    them a record of 1,036 B, re-coded both ways and copied."""
    arrays, dims = I.edge_slots(), (128, 8, 1)
    plain, tight = J.pack(*arrays, *dims), T.pack(*arrays, *dims)
    assert np.frombuffer(plain[16:16 + 2 * 16], "<u2").max() == J.RECORD_MAX
    assert set(T.stream_modes(*arrays).reshape(-1).tolist()) == {0, 1, 2}
    for src, target, want in ((plain, True, tight), (tight, False, plain), (plain, None, plain),
                              (tight, None, tight)):
        got, res, n = gpu_select(src, dims, [(0, 0, 0)], 128, 8, target)
        assert got[:n] == want and res == [len(want), U64, 0], first_difference(got[:n], want)
        sub = M.sub_arrays(arrays, range(3, 9))
        got, res, n = gpu_select(src, dims, [(0, 24, 0)], 48, 8, target)
        want6 = (T.pack if want is tight else J.pack)(*sub, 48, 8, 1)
        assert got[:n] == want6 and res == [len(want6), U64, 0], first_difference(got[:n], want6)


# ---- capacity, alignment ---------------------------------------------------------------------

@pytest.mark.parametrize("tight,target", [(False, None), (False, True), (True, False)])
def test_capacity(gpu, oracle, tight, target):
    data = stream_of(oracle, A, "rand", tight)
    items = whole([2, 4, 2])
    want, words, _ = M.select(data, A, M.offsets_of(data, A), items, A[0], A[1], fmt_of(target))
    n, idx_end = len(want), 16 + 2 * 135
    for cap in (0, 15, 16, 17, idx_end - 1, idx_end + 1, idx_end + 700, n - 1, n):
        got, res, length = gpu_select(data, A, items, A[0], A[1], target, cap=cap, room=n + 64)
        assert got == want[:cap], (cap, first_difference(got, want[:cap]))
        assert res == words and length == n


@pytest.mark.parametrize("lead", [1, 7, 15])
@pytest.mark.parametrize("tight,target", [(False, None), (False, True), (True, False)])
def test_source_alignment(gpu, oracle, lead, tight, target):
    data = stream_of(oracle, B, "rand", tight)
    items = [(2, 8, 0), (0, 16, 8)]
    check_model(data, B, items, 45, 35, target, lead=lead)


# ---- bad items, bad offsets, bad records ---------------------------------------------------------

@pytest.mark.parametrize("tight,target", [(False, None), (False, True), (True, False)])
def test_bad_items_among_good_ones(gpu, oracle, tight, target):
    data = stream_of(oracle, A, "rand", tight)
    items = [(0, 8, 8), (5, 0, 0), (1, 4, 8), (1, 8, 4), (2, 56, 0), (2, 48, 16), (3, 0, 24),
             (U64, 0, 0), (0, U64 - 7, 0), (0, 8, U64 - 7), (4, 48, 16)]
    want, res, _ = check_model(data, A, items, 24, 24, target)
    assert res[1:] == [2, 0]
    sizes = np.frombuffer(want[16:16 + 2 * 9 * len(items)], "<u2").reshape(len(items), 9)
    assert [bool((s != 12).any()) for s in sizes] == [k in (0, 5, 10) for k in range(len(items))]
    for broken in (b"K" + data[1:], data[:8] + (48).to_bytes(4, "little") + data[12:]):
        _, res, _ = check_model(broken, A, items[:3], 24, 24, target, offs=M.offsets_of(data, A))
        assert res[1:] == [1, 0]
    # the arguments differ from a good header
    _, res, _ = check_model(data, (72, 40, 6), items[:1], 24, 24, target,
                            offs=M.offsets_of(data, A) + [len(data)] * 45)
    assert res[1:] == [1, 0]


@pytest.mark.parametrize("tight,target", [(False, None), (False, True), (True, False)])
def test_untrusted_offsets(gpu, oracle, tight, target):
    data = stream_of(oracle, A, "rand", tight)
    offs = M.offsets_of(data, A)
    n = len(data)
    offs[10], offs[11] = offs[11], offs[10]             # a decreasing pair
    offs[50] = offs[49] + 11                            # a size of 11
    offs[60] = offs[59] + 1037                          # a size of 1,037
    offs[100] = n + 1                                   # past in_len
    offs[150] += 11                                     # 11 bytes into a record
    offs[224] = U64
    want, res, _ = check_model(data, A, whole([0, 1, 2, 3, 4, 0]), 72, 40, target, offs=offs)
    bad = (10, 49, 59, 60, 99, 100, 223, 224, 225 + 10)     # 60 starts past its end; image 0 comes twice
    assert res[1] == U64 and res[2] >= len(bad)
    sizes = np.frombuffer(want[16:16 + 2 * 270], "<u2")
    assert all(sizes[t] == 12 for t in bad)
    if target is not None:                              # re-coding finds the record entered 11 bytes in
        assert sizes[149] == 12 and sizes[150] == 12
    good =[t for t in range(225) if t not in (9, 10, 11, 49, 50, 59, 60, 99, 100, 149, 150, 223, 224)]
    clean, _, _ = M.select(data, A, M.offsets_of(data, A), whole(range(5)), 72, 40, fmt_of(target))
    csz = np.frombuffer(clean[16:16 + 2 * 225], "<u2")
    assert all(sizes[t] == csz[t] for t in good)


def test_bad_records_while_recoding(gpu, oracle):
    """Luma ncodes = 129 in a JPR1 record and a mode of 3 in a JPT1 record: the
    re-coding writes the empty record, the copy does not look."""
    for tight, poke in ((False, lambda b, p: b[:p + 1] + bytes([129]) + b[p + 2:]),
                        (True, lambda b, p: b[:p + 3] + bytes([b[p + 3] | 0xC0]) + b[p + 4:])):
        data = stream_of(oracle, A, "rand", tight)
        offs = M.offsets_of(data, A)
        broken = poke(data, offs[70])
        items = whole([1, 0])                           # tile 70 is tile 25 of image 1: output tile 25
        want, res, _ = check_model(broken, A, items, 72, 40, not tight, offs=offs)
        assert res[1:] == [U64, 1]
        assert np.frombuffer(want[16:16 + 2 * 90], "<u2")[25] == 12
        want, res, _ = check_model(broken, A, items, 72, 40, None, offs=offs)
        assert res[1:] == [U64, 0]


# ---- replay, wrappers -----------------------------------------------------------------------------

def test_graph_replay(gpu, oracle):
    """One captured call replayed twice, the items rewritten in place in
    between: each replay's own bytes and result words, no counter accumulates."""
    import torch
    from lz4jpeg import jpeg
    data = stream_of(oracle, A, "rand", False)
    d_stream = dev_bytes(data)
    d_offs, _ = jpeg.stream_index_device(d_stream, len(data), *A)
    offs = M.offsets_of(data, A)
    sets = [[(0, 8, 8), (9, 0, 0), (3, 40, 16), (1, 0, 0)], [(4, 48, 16), (2, 0, 0), (2, 4, 0), (0, 16, 8)]]
    cols = [torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(3)]
    room = jpeg.pack_bound(24, 24, 4)
    d_out = torch.full((room,), FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    d_res = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    scr = torch.empty(jpeg.select_scratch_bytes(4, 24, 24), dtype=torch.uint8, device="cuda")

    def call():
        jpeg.select_device(d_stream, len(data), *A, d_offs, *cols, 24, 24, tight=True, d_out=d_out,
                           d_len=d_len, scratch=scr, d_result=d_res)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for items in sets:
        for k in range(3):
            cols[k].copy_(dev_u64([it[k] for it in items]))
        d_out.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        want, words, _ = M.select(data, A, offs, items, 24, 24, M.JPT1)
        assert d_out.cpu().numpy().tobytes() == want + bytes([FILL]) * (room - len(want))
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == words
        assert int(d_len.item()) == len(want)
    assert words[1:] == [3, 0]                              # the second set: item 2 is bad


def test_wrappers(gpu, oracle):
    import torch
    from lz4jpeg import jpeg
    imgs = images_of(oracle, A, "smooth")
    data = stream_of(oracle, A, "smooth", False)
    rd = jpeg.StreamReader(dev_bytes(data))
    got = rd.select([3, 0, 0, 4])
    assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == compress(imgs[[3, 0, 0, 4]], False)
    assert rd.select().cpu().numpy().tobytes() == data
    tight = rd.transcode(True)
    assert tight.cpu().numpy().tobytes() == stream_of(oracle, A, "smooth", True)
    assert jpeg.StreamReader(tight).transcode(False).cpu().numpy().tobytes() == data
    win = rd.select([1, 2], x=[8, 48], y=16, w=24, h=16, tight=True)
    crops = np.stack([imgs[1, 16:32, 8:32], imgs[2, 16:32, 48:72]])
    assert win.cpu().numpy().tobytes() == compress(crops, True)
    with pytest.raises(jpeg.JpegError, match="item 1"):
        rd.select([0, 5])
    with pytest.raises(jpeg.JpegError, match="item 0"):
        rd.select([0], x=4, w=8, h=8)
    offs = rd.d_offsets.clone()
    rd.d_offsets[7] = len(data) + 5
    with pytest.raises(jpeg.JpegError, match="malformed"):
        rd.select([0])
    rd.d_offsets = offs
    # JPR1 from JPT1 grows by more than the first guess allows: the second call
    rand =jpeg.StreamReader(dev_bytes(stream_of(oracle, A, "rand", True)))
    assert rand.transcode(False).cpu().numpy().tobytes() == stream_of(oracle, A, "rand", False)


def test_concat_streams(gpu, oracle):
    from lz4jpeg import jpeg
    for kind, tight in KINDS:
        imgs = images_of(oracle, A, kind)
        parts = [compress(imgs[:2], tight), compress(imgs[2:3], tight), compress(imgs[3:], tight)]
        got = jpeg.concat_streams([dev_bytes(p) for p in parts])
        assert got.cpu().numpy().tobytes() == stream_of(oracle, A, kind, tight)
    a, b = dev_bytes(stream_of(oracle, A, "rand", False)), dev_bytes(stream_of(oracle, A, "rand", True))
    with pytest.raises(jpeg.JpegError, match="differ"):
        jpeg.concat_streams([a, b])
    with pytest.raises(jpeg.JpegError, match="differ"):
        jpeg.concat_streams([a, dev_bytes(stream_of(oracle, B, "rand", False))])
    with pytest.raises(jpeg.JpegError):
        jpeg.concat_streams([a, a[:100]])
    with pytest.raises(jpeg.JpegError):
        jpeg.concat_streams([a[:8]])
