"""jpegr_thumb_device (include/jpegr.h) on the GPU: the DC terms against
columns 0, 64 and 96 of what jpegr_stream_decode_device gives for the same
bytes, and the pixels byte for byte against jpegr_reconstruct_device of those
coefficients with every AC term 0, taken at every eighth pixel (the definition:
jpr_thumb_model.py, checked by test_jpr_thumb_model.py).  Both outputs lie
between guard bands in sentinel-filled tensors that are compared whole; the
stream buffer is exactly the stream; d_result starts as garbage."""
import ctypes
import functools

import numpy as np
import pytest

import jpr_crop_model as CM
import jpr_thumb_model as M
from jpr_gpu_lib import (FILL, GUARD, U64, coef_dev, dev_bytes, dev_u64, encoded_jpr, gpu_decode,
                         host_offsets, image, jpr_mutations, pack_scratch, random_coef)

pytestmark = pytest.mark.gpu

DC = list(M.DC_AT)
GARBAGE = 0x5A5A5A5A5A5A5A5A


# ---- drivers ------------------------------------------------------------------------

def tiles_of(dims):
    return ((dims[0] + 7) // 8) * ((dims[1] + 7) // 8)


def stream_from_coef(coef, dims, tight, direct):
    """The stream's bytes of coefficients [ntiles, 128]: by the entropy encoder
    and pack, or by encode_stream_device."""
    import torch
    from lz4jpeg import jpeg
    w, h, nimg = dims
    d_coef = coef_dev(coef)
    if direct:
        d_out, over = jpeg.encode_stream_exact_device(d_coef, w, h, nimg, tight=tight)
        assert over == 0
        return d_out.cpu().numpy().tobytes()
    ent = jpeg.Entropy(coef.shape[0])
    ent.encode(d_coef)
    d_out, d_len = jpeg.pack_device(ent, w, h, nimg, tight=tight)
    torch.cuda.synchronize()
    assert int(ent.status[0].item()) == 0
    return d_out[:int(d_len.item())].cpu().numpy().tobytes()


def gpu_thumb(data, dims, first=0, count=None, offs=None, rgba=True, dc=True):
    """(pixels [n, 4] uint8 or None, DC quads [n, 4] int16 or None, the result
    words, unsigned) of one call on exactly these bytes.  offs: None (the call
    scans), "index" (jpegr_stream_index_device's) or ntiles + 1 values."""
    import torch
    from lz4jpeg import _lib, jpeg
    w, h, nimg = dims
    count = nimg - first if count is None else count
    n, nt = count * tiles_of(dims), nimg * tiles_of(dims)
    d_stream = dev_bytes(data)
    if isinstance(offs, str):
        d_offs, _ = jpeg.stream_index_device(d_stream, len(data), w, h, nimg)
    else:
        d_offs = None if offs is None else dev_u64(offs)
    scratch = pack_scratch(nt) if d_offs is None else None
    big_px = torch.full((2 * GUARD + 4 * n,), FILL, dtype=torch.uint8, device="cuda")
    big_dc = torch.full((2 * GUARD + 8 * n,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((3,), GARBAGE, dtype=torch.int64, device="cuda")
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o if t is not None else 0)
    rc = _lib.lib().jpegr_thumb_device(p(d_stream), len(data), w, h, nimg, p(d_offs), first, count,
                                       p(big_px, GUARD) if rgba else None,
                                       p(big_dc, GUARD) if dc else None, p(scratch), p(res),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    out = []
    for big, width, on in ((big_px, 4, rgba), (big_dc, 8, dc)):
        host = big.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[GUARD + width * n:] == FILL).all(), "guards"
        body = host[GUARD:GUARD + width * n]
        if not on:
            assert (body == FILL).all()
        out.append(body.copy() if on else None)
    px = out[0].reshape(n, 4) if rgba else None
    quads = out[1].view(np.int16).reshape(n, 4) if dc else None
    return px, quads, [int(x) & U64 for x in res.cpu().tolist()]


def pixels_of(coef, dims, count):
    """Every eighth pixel of jpegr_reconstruct_device of the coefficients with
    every AC term 0: [count * tiles, 4]."""
    from lz4jpeg import jpeg
    w, h, _ = dims
    full = jpeg.reconstruct_device(coef_dev(M.dc_only(coef)), w, h, count)
    return full.view(count, h, w, 4)[:, ::8, ::8].reshape(-1, 4).cpu().numpy()


def check_range(data, dims, want_coef, first=0, count=None, offs=None, loose=(), want_res=None):
    """One call on images [first, first + count): want_coef the whole stream's
    coefficients as the full decoder gives them; loose: tiles of the stream
    whose pixel is unspecified."""
    per = tiles_of(dims)
    count = dims[2] - first if count is None else count
    coef = want_coef[first * per:(first + count) * per]
    px, quads, res = gpu_thumb(data, dims, first, count, offs)
    keep = np.array([first * per + k not in loose for k in range(count * per)])
    assert np.array_equal(quads[keep, :3], coef[keep][:, DC]), (first, count)
    assert not quads[:, 3].any()
    assert np.array_equal(px[keep], pixels_of(coef, dims, count)[keep]), (first, count)
    if want_res is not None:
        assert res[:2] == want_res[:2] and res[2] <= want_res[2], (res, want_res)
    return px, quads, res


# ---- DC terms and pixels of ordinary streams ------------------------------------------

DIMS = (104, 40, 2)                                  # 13 x 5 tiles an image, 130 tiles: three waves


@functools.lru_cache(maxsize=None)
def mixed_coef(oracle, kind):
    """130 tiles: random coefficients, or two oracle-made images' own; among
    them all-equal tiles (luma all 64, chroma all 32: one-code streams) and
    all-zero tiles.  Shared: read, do not change."""
    if kind == "coef":
        coef = random_coef(130).copy()
    else:
        imgs = [image(oracle, 104, 40, kind, seed=3 + i) for i in range(2)]
        coef = np.concatenate([oracle.jpeg_encode(im).reshape(-1, 128) for im in imgs])
    for t in (0, 5, 63, 64, 129):
        coef[t, :64], coef[t, 64:] = 64, 32
    for t in (1, 62, 65, 128):
        coef[t] = 0
    coef[2, :64], coef[3, 64:96] = 64, 32                # one one-code stream in a tile
    coef.setflags(write=False)
    return coef


@pytest.mark.parametrize("offs", [None, "index"], ids=["scan", "offsets"])
@pytest.mark.parametrize("direct", [False, True], ids=["pack", "encode_stream"])
@pytest.mark.parametrize("tight", [False, True], ids=["JPR1", "JPT1"])
@pytest.mark.parametrize("kind", ["coef", "rand", "smooth"])
def test_dc_and_pixels(gpu, oracle, kind, tight, direct, offs):
    coef = mixed_coef(oracle, kind)
    data = stream_from_coef(coef, DIMS, tight, direct)
    assert data[:4] == (b"JPT1" if tight else b"JPR1")
    full, full_res = gpu_decode(data, len(data), DIMS)
    assert np.array_equal(full, coef) and full_res == [len(data), U64, 0]
    px, _, res = check_range(data, DIMS, full, offs=offs)
    assert res == [len(data), U64, 0]
    assert np.array_equal(px, M.thumbnails(oracle, coef))           # the model, over the oracle


def test_one_output_alone(gpu, oracle):
    coef = mixed_coef(oracle, "coef")
    data = stream_from_coef(coef, DIMS, True, True)
    px, none, res = gpu_thumb(data, DIMS, dc=False)
    assert none is None and res == [len(data), U64, 0]
    none, quads, res = gpu_thumb(data, DIMS, offs="index", rgba=False)
    assert none is None and res == [len(data), U64, 0]
    assert np.array_equal(quads[:, :3], coef[:, DC]) and np.array_equal(px, M.thumbnails(oracle, coef))


# ---- every rounding case of the one term ---------------------------------------------

def sweep_check(oracle, coef, dims, tight):
    data = stream_from_coef(coef, dims, tight, True)
    want = pixels_of(coef, dims, dims[2])
    for offs in (None, "index"):
        px, quads, res = gpu_thumb(data, dims, offs=offs)
        assert res == [len(data), U64, 0]
        assert np.array_equal(quads[:, :3], coef[:, DC])
        assert np.array_equal(px, want)
    return want


def test_luma_dc_sweep(gpu, oracle):
    """A 2048 x 2048 "image" whose 65,536 tiles take every int16 luma DC (chroma
    DC 0): both clamps and every rounding case of the luma term."""
    coef = np.zeros((65536, 128), np.int16)
    coef[:, 0] = np.random.default_rng(5).permutation(65536) - 32768
    want = sweep_check(oracle, coef, (2048, 2048, 1), False)
    assert np.array_equal(want, M.thumbnails(oracle, coef))
    assert want[:, 0].min() == 0 and want[:, 0].max() == 255 and len(set(want[:, 0].tolist())) == 256


# chroma samples are 128 + 3.005 d: d = -128 .. 127 passes both clamps with room;
# luma samples 128 + d for d = -154 .. 152 pass both by a little
GRID_CHROMA = np.arange(256) - 128
GRID_LUMA = np.round((np.arange(256) - 128) * 1.2).astype(np.int64)
GRID_FIXED = (-50, 7, 45)                            # the other chroma: below 0, inside, above 255


@pytest.mark.parametrize("swept", [64, 96], ids=["Cr", "Cb"])
def test_chroma_grid(gpu, oracle, swept):
    """256 x 256 tiles of chroma DC x luma DC, an image for each of three values
    of the other chroma DC; a JPT1 stream, whose tables are modes 1 and 2 here."""
    coef = np.zeros((3, 256, 256, 128), np.int16)
    coef[..., 0] = GRID_LUMA[None, :, None]
    coef[..., swept] = GRID_CHROMA[None, None, :]
    coef[..., 160 - swept] = np.array(GRID_FIXED)[:, None, None]
    coef = coef.reshape(-1, 128)
    want = sweep_check(oracle, coef, (2048, 2048, 3), True)
    assert np.array_equal(want, M.thumbnails(oracle, coef))
    for ch in range(3):
        assert want[:, ch].min() == 0 and want[:, ch].max() == 255


# ---- shapes at the seams -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def seam_stream(dims, tight):
    """(bytes, the full decoder's coefficients) of random coefficients.  Shared."""
    nt = dims[2] * tiles_of(dims)
    data = stream_from_coef(random_coef(nt), dims, tight, True)
    full, res = gpu_decode(data, len(data), dims)
    assert res == [len(data), U64, 0] and np.array_equal(full, random_coef(nt))
    return data, full


@pytest.mark.parametrize("offs", [None, "index"], ids=["scan", "offsets"])
def test_small_images(gpu, offs):
    """13 x 11 x 3: 4 tiles an image, both edges partial."""
    dims = (13, 11, 3)
    data, full = seam_stream(dims, False)
    for first, count in ((0, None), (0, 1), (1, 1), (2, 1), (1, 2)):
        check_range(data, dims, full, first, count, offs, want_res=[len(data), U64, 0])


@pytest.mark.parametrize("offs", [None, "index"], ids=["scan", "offsets"])
def test_ranges_inside_a_wave(gpu, offs):
    """100 images of 13 x 11: ranges that start and end inside a wave's 64 tiles."""
    dims = (13, 11, 100)
    data, full = seam_stream(dims, True)
    for first in (0, 1, 17, 99):
        for count in (1, 100 - first):
            check_range(data, dims, full, first, count, offs, want_res=[len(data), U64, 0])


@pytest.mark.parametrize("offs", [None, "index"], ids=["scan", "offsets"])
def test_across_a_scan_partial(gpu, offs):
    """70 images of 64 x 64, 4,480 tiles: images 63 and 64 are tiles 4,032 ..
    4,159, across the scan partial's boundary at 4,096."""
    dims = (64, 64, 70)
    data, full = seam_stream(dims, False)
    check_range(data, dims, full, 63, 2, offs, want_res=[len(data), U64, 0])
    check_range(data, dims, full, 0, None, offs, want_res=[len(data), U64, 0])


@pytest.mark.parametrize("offs", [None, "index"], ids=["scan", "offsets"])
def test_one_tile_past_a_wave(gpu, offs):
    dims = (520, 8, 1)
    data, full = seam_stream(dims, True)
    check_range(data, dims, full, offs=offs, want_res=[len(data), U64, 0])


# ---- malformed streams ---------------------------------------------------------------------

def tight_mutations():
    """test_gpu_jpeg_tight's list on its 65-tile JPT1 stream: (name, bytes, in_len)."""
    import test_gpu_jpeg_tight as TT
    _, _, good, _ = TT.encoded65()
    return TT._mutations(good)


def mutation_case(k):
    """(name, the stream's bytes cut to in_len, tiles whose pixel is unspecified)."""
    if k < 6:
        name, data, in_len, _, _ = jpr_mutations(encoded_jpr(65))[k]
        return name, data[:in_len], ()
    name, data, in_len = tight_mutations()[k - 6]
    # tile 41's record moves by a byte with tile 40's index entry: malformed, or
    # by chance well-formed garbage that the full decoder may reject later on
    return name, data[:in_len], ((41,) if k - 6 in (3, 4) else ())


@pytest.mark.parametrize("offs", [None, "index"], ids=["scan", "offsets"])
@pytest.mark.parametrize("k", range(15))
def test_mutations(gpu, oracle, k, offs):
    """Result words [0] and [1] are the full decoder's for the same bytes; what
    it decodes is exact here, and what it zeroes (a malformed tile, every tile
    under a wrong header or index) has the colour of all-zero coefficients."""
    dims = (520, 8, 1)
    name, data, loose = mutation_case(k)
    full, full_res = gpu_decode(data, len(data), dims)
    px, quads, res = check_range(data, dims, full, offs=offs, loose=loose, want_res=full_res)
    zero = M.zero_pixel(oracle)
    if full_res[1] == 0:
        assert (px == zero).all() and not quads.any() and res[2] == 0, name
    elif full_res[1] != U64:
        bad = full_res[1] - 1
        assert (px[bad] == zero).all() and not quads[bad].any(), name
        assert np.count_nonzero((px != zero).any(axis=1)) >= 60, name


def test_untrusted_offsets(gpu, oracle):
    """A good stream with a perturbed offsets array (test_gpu_jpeg_crop's
    perturbations): tiles whose offsets fail the bounds are malformed, their
    neighbours whose offsets pass but whose bytes are not a record are malformed
    or unspecified, every other tile is exact, [1] names the first malformed
    tile and nothing is read or written out of bounds."""
    dims = (520, 520, 2)
    data, full = seam_stream(dims, False)
    offs = [int(v) for v in host_offsets(data, dims)]
    n = len(data)
    tile = lambda tx, ty, im=0: (im * 65 + ty) * 65 + tx
    e1, e2, e3, e4, e5 = tile(10, 5), tile(30, 12), tile(20, 30), tile(50, 40), tile(5, 60, 1)
    offs[e1] = n + 1                                    # past in_len: tiles e1 - 1 and e1
    offs[e2], offs[e2 + 1] = offs[e2 + 1], offs[e2]     # a decreasing pair: tile e2
    offs[e3] = offs[e3 - 1] + 1037                      # a size of 1,037: tile e3 - 1
    offs[e4] = offs[e4 - 1] + 11                        # a size of 11: tile e4 - 1
    offs[e5] = U64                                      # all ones: tiles e5 - 1 and e5
    by_bounds = CM.bad_offset_tiles(offs, n)
    assert {e1 - 1, e1, e2, e3 - 1, e4 - 1, e5 - 1, e5} <= by_bounds
    unsure = {e2 - 1, e2 + 1, e3, e4}                   # two records taken for one, a record entered 11 B in
    want = full.copy()
    want[sorted(by_bounds)] = 0
    px, quads, res = check_range(data, dims, want, offs=offs, loose=unsure)
    assert res[0] == n and res[1] == 1 + min(by_bounds) == e1
    zero = M.zero_pixel(oracle)
    for t in by_bounds:
        assert (px[t] == zero).all() and not quads[t].any(), t
    # images 1 alone: the first malformed tile of the range
    _, _, res = check_range(data, dims, want, 1, 1, offs=offs, loose=unsure)
    assert res[:2] == [n, 1 + e5 - 1]
    offs = [int(v) for v in host_offsets(data, dims)]
    offs[-1] += 1                                       # the length the offsets imply is not in_len
    px, quads, res = gpu_thumb(data, dims, offs=offs)
    assert res == [n + 1, 0, 0] and (px == zero).all() and not quads.any()


# ---- replay, calls in flight, wrappers -------------------------------------------------------

def test_graph_replay(gpu, oracle):
    """One call captured (a linear chain) and replayed twice after the outputs
    and the result words were overwritten: the eager call's bytes both times."""
    import torch
    from lz4jpeg import jpeg
    dims = (64, 64, 70)
    data, full = seam_stream(dims, False)
    d_stream = dev_bytes(data)
    n = 2 * 64
    d_px = torch.full((4 * n,), FILL, dtype=torch.uint8, device="cuda")
    d_dc = torch.full((4 * n,), 77, dtype=torch.int16, device="cuda")
    d_res = torch.full((3,), GARBAGE, dtype=torch.int64, device="cuda")
    scratch = pack_scratch(70 * 64)

    def call():
        jpeg.thumb_device(d_stream, len(data), *dims, first=63, count=2, d_out=d_px, d_dc=d_dc,
                          scratch=scratch, d_result=d_res)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # warm-up, and the eager call
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = (d_px.cpu().numpy(), d_dc.cpu().numpy(), d_res.cpu().tolist())
    coef = full[63 * 64:65 * 64]
    assert np.array_equal(eager[1].reshape(n, 4)[:, :3], coef[:, DC])
    assert np.array_equal(eager[0].reshape(n, 4), pixels_of(coef, dims, 2))
    assert [int(x) & U64 for x in eager[2]] == [len(data), U64, 0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        d_px.fill_(FILL)
        d_dc.fill_(77)
        d_res.fill_(GARBAGE)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_px.cpu().numpy(), eager[0])
        assert np.array_equal(d_dc.cpu().numpy(), eager[1])
        assert d_res.cpu().tolist() == eager[2]


def test_two_calls_in_flight(gpu, oracle):
    """Two streams, each call with its own scratch and result, on two HIP
    streams at once."""
    import torch
    from lz4jpeg import jpeg
    cases = [((64, 64, 70), False), ((520, 520, 2), False)]
    calls = []
    for dims, tight in cases:
        data, full = seam_stream(dims, tight)
        calls.append((dims, full, dev_bytes(data), len(data), pack_scratch(dims[2] * tiles_of(dims)),
                      torch.full((3,), GARBAGE, dtype=torch.int64, device="cuda"), torch.cuda.Stream()))
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):                                      # interleaved launches
        outs = [jpeg.thumb_device(d, n, *dims, want_dc=True, scratch=scr, d_result=res, stream=st)
                for dims, _, d, n, scr, res, st in calls]
    torch.cuda.synchronize()
    for (dims, full, _, n, _, _, _), (d_out, d_dc, d_res) in zip(calls, outs):
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == [n, U64, 0]
        assert np.array_equal(d_dc.cpu().numpy().reshape(-1, 4)[:, :3], full[:, DC])
        assert np.array_equal(d_out.cpu().numpy().reshape(-1, 4), pixels_of(full, dims, dims[2]))


def test_wrappers(gpu, oracle):
    """thumbnails_device and StreamReader.thumbnails: shapes, the same pixels
    either way, JpegError on a malformed tile."""
    import torch
    from lz4jpeg import jpeg
    coef = mixed_coef(oracle, "rand")
    data = stream_from_coef(coef, DIMS, True, False)
    d_stream = dev_bytes(data)
    want = M.thumbnails(oracle, coef).reshape(2, 5, 13, 4)
    got, w, h, count = jpeg.thumbnails_device(d_stream)
    assert (w, h, count) == (104, 40, 2) and got.shape == (2, 5, 13, 4) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want)
    rd = jpeg.StreamReader(d_stream)
    for first, count in ((0, None), (1, 1), (0, 1)):
        got, _, _, k = rd.thumbnails(first, count)
        assert k == (2 - first if count is None else count)
        assert np.array_equal(got.cpu().numpy(), want[first:first + k])
        got, _, _, _ = jpeg.thumbnails_device(d_stream, first, count)
        assert np.array_equal(got.cpu().numpy(), want[first:first + k])
    with pytest.raises(ValueError):
        rd.thumbnails(2, 1)
    y70 = int(host_offsets(data, DIMS)[70])
    broken = dev_bytes(data[:y70 + 3] + bytes([data[y70 + 3] | 0xC0]) + data[y70 + 4:])   # mode 3
    with pytest.raises(jpeg.JpegError, match="verdict 71"):
        jpeg.thumbnails_device(broken)
    with pytest.raises(jpeg.JpegError, match="verdict 71"):
        jpeg.StreamReader(broken).thumbnails(1)
    got, _, _, _ = jpeg.StreamReader(broken).thumbnails(0, 1)          # image 0 does not hold tile 70
    assert np.array_equal(got.cpu().numpy(), want[:1])
