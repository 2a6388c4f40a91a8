"""jpegr_stream_decode_device (include/jpegr.h): a JPR stream decoded straight
to coefficients, whole or by tile range, with no slots in between.  Inputs come
from entropy_inputs and jpr_format; the expected coefficients are the builders'
`want` or the encoder's input, never the new code's own output.

A workgroup takes 64 tiles counted from tile0, the scan groups 64 tiles from
the stream's first and its partials 4,096: the ranges below start off both
grids, cross a partial and end in a part-filled workgroup."""
import functools

import numpy as np
import pytest

import entropy_inputs as E
import jpr_format as J
import jpt_format as T
from jpr_gpu_lib import (SENTINEL, U64, crafted, crafted_jpr, encoded, encoded_jpr, gpu_decode,
                         jpr_mutations, pack_scratch)

pytestmark = pytest.mark.gpu


def _crafted(oracle):
    """(expected coefficients, the JPR1 stream, dims) of the crafted batch."""
    _, want, dims = crafted(oracle)
    return want, crafted_jpr(oracle), dims


def _encoded(*args):
    """(coefficients, the JPR1 stream, dims) of jpr_gpu_lib.encoded(*args)."""
    _, coef, dims = encoded(*args)
    return coef, encoded_jpr(*args), dims


# ---- crafted batch ---------------------------------------------------------------

def test_crafted_whole(gpu, oracle):
    want, data, dims = _crafted(oracle)
    got, res = gpu_decode(data, len(data), dims)
    assert res == [len(data), U64, 0]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("tile0,ntile", [(1, 703), (37, 200), (63, 2)])
def test_crafted_ranges(gpu, oracle, tile0, ntile):
    want, data, dims = _crafted(oracle)
    got, res = gpu_decode(data, len(data), dims, tile0, ntile)
    assert res == [len(data), U64, 0]
    assert np.array_equal(got, want[tile0:tile0 + ntile])


# ---- scan and wave edges ---------------------------------------------------------

@pytest.mark.parametrize("nt", [1, 63, 64, 65, 4097])
def test_tile_counts(gpu, nt):
    coef, data, dims = _encoded(nt)
    ranges = [(0, nt), (0, 1), (nt - 1, 1)]
    if nt == 4097:
        ranges += [(4095, 2), (64, 64)]
    for tile0, ntile in ranges:
        got, res = gpu_decode(data, len(data), dims, tile0, ntile)
        assert res == [len(data), U64, 0], (tile0, ntile)
        assert np.array_equal(got, coef[tile0:tile0 + ntile]), (tile0, ntile)


@pytest.mark.parametrize("tight", [False, True], ids=["JPR1", "JPT1"])
def test_ranges_inside_a_later_scan_partial(gpu, tight):
    """One stream of 4,160 tiles (a 520 x 512 image), whose second scan partial
    begins at tile 4,096: a range that crosses into it from six tiles before,
    one that starts on its first tile, and its last tile alone.  Each equals the
    same tiles of the whole-stream decode, which equals the encoder's input."""
    arrays, coef, dims = encoded(4160, 520, 512)
    data = T.pack(*arrays, *dims) if tight else encoded_jpr(4160, 520, 512)
    whole, res = gpu_decode(data, len(data), dims)
    assert res == [len(data), U64, 0]
    assert np.array_equal(whole, coef)
    for tile0, ntile in ((4090, 70), (4096, 64), (4159, 1)):
        got, res = gpu_decode(data, len(data), dims, tile0, ntile)
        assert res == [len(data), U64, 0], (tile0, ntile)
        assert np.array_equal(got, whole[tile0:tile0 + ntile]), (tile0, ntile)


# ---- three images ----------------------------------------------------------------

def test_three_images(gpu):
    import torch
    from lz4jpeg import jpeg
    coef, data, dims = _encoded(45, 40, 24, 3)
    got, res = gpu_decode(data, len(data), dims, 15, 15)
    assert res == [len(data), U64, 0]
    assert np.array_equal(got, coef[15:30])
    stream = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    rgba, w, h, count = jpeg.decompress_images_device(stream, 1, 1)
    assert (w, h, count) == (40, 24, 1)
    d_one = torch.from_numpy(coef[15:30].reshape(-1).copy()).cuda()
    assert torch.equal(rgba, jpeg.reconstruct_device(d_one, 40, 24, 1))
    rgba, w, h, count = jpeg.decompress_images_device(stream)
    assert (w, h, count) == (40, 24, 3)
    ref, rw, rh, rn = jpeg.decompress_device(stream)
    assert (rw, rh, rn) == (40, 24, 3) and torch.equal(rgba, ref)
    rgba, _, _, count = jpeg.decompress_images_device(stream, 1)          # images 1 and 2
    assert count == 2 and torch.equal(rgba, ref[40 * 24 * 4:])
    with pytest.raises(ValueError):
        jpeg.decompress_images_device(stream, 3)
    bad = stream.clone()
    bad[0] = 0
    with pytest.raises(jpeg.JpegError):
        jpeg.decompress_images_device(bad)


# ---- bounds ----------------------------------------------------------------------

@pytest.mark.parametrize("tile0,ntile", [(0, None), (640, 64), (703, 1)])
def test_bytes_past_the_stream_do_not_matter(gpu, oracle, tile0, ntile):
    """in_len exact, 64 bytes of 0x00 or of 0xFF behind it (the crafted batch's
    last groups hold full slots and streams that end on a byte's last bit), and
    the stream at 0, 3 and 13 bytes off a 16-B boundary."""
    want, data, dims = _crafted(oracle)
    runs = [gpu_decode(data, len(data), dims, tile0, ntile, tail=bytes([fill]) * 64, lead=lead)
            for fill, lead in ((0x00, 0), (0xFF, 0), (0x00, 3), (0xFF, 13))]
    for got, res in runs:
        assert res == [len(data), U64, 0]
        assert np.array_equal(got, runs[0][0])
    assert np.array_equal(runs[0][0], want[tile0:] if ntile is None else want[tile0:tile0 + ntile])


# ---- header, index and record errors ---------------------------------------------

@pytest.mark.parametrize("k", range(6))
def test_malformed_streams(gpu, k):
    coef, good, dims = _encoded(65)
    name, data, in_len, verdict, bad = jpr_mutations(good)[k]
    implied, want_verdict = J.unpack(data[:in_len], dims)[3:]
    assert want_verdict == verdict, name
    got, res = gpu_decode(data, in_len, dims)
    assert res == [implied, verdict, 0], name
    if verdict == 0:
        assert not got.any(), name
    else:
        assert not got[bad].any(), name
        rest = np.arange(65) != bad
        assert np.array_equal(got[rest], coef[rest]), name


def test_malformed_record_outside_the_range(gpu):
    coef, good, dims = _encoded(65)
    name, data, in_len, verdict, bad = jpr_mutations(good)[4]
    assert (verdict, bad) == (41, 40)
    got, res = gpu_decode(data, in_len, dims, 41, 24)
    assert res == [len(data), U64, 0]
    assert np.array_equal(got, coef[41:65])
    got, res = gpu_decode(data, in_len, dims, 40, 1)        # and alone in its range
    assert res == [len(data), 41, 0] and not got.any()


# ---- entropy errors --------------------------------------------------------------

def _stream_offsets(data, nt):
    """[nt, 3] byte offsets of every stream of a consistent JPR stream."""
    sizes = np.frombuffer(data[16:16 + 2 * nt], "<u2").astype(np.int64)
    recs = 16 + 2 * nt + np.concatenate([[0], np.cumsum(sizes)])
    out = np.zeros((nt, 3), np.int64)
    for t in range(nt):
        p = int(recs[t])
        for c in range(3):
            out[t, c] = p
            p += 4 + 3 * data[p + 1] + (int.from_bytes(data[p + 2:p + 4], "little") + 7) // 8
        assert p == recs[t + 1]
    return out


def _bump_rle_len(data, offs, picks):
    """rle_len + 2 in the chosen (tile, channel) streams: well-formed records,
    streams whose symbol count no longer matches."""
    b = bytearray(data)
    for t, c in picks:
        p = int(offs[t, c])
        assert b[p + 1] > 1                                  # ncodes > 1: the bits are walked
        assert b[p] + 2 <= J.SLOT_CODES[c]                   # still inside the slot's bound
        b[p] += 2
    return bytes(b)


@functools.lru_cache(maxsize=None)
def image_stream(oracle):
    """A 512 x 384 random image: (coefficients [3072, 128], its JPR stream)."""
    import torch
    from lz4jpeg import jpeg
    w, h = 512, 384
    d_img = torch.from_numpy(oracle.rand_image(w, h, seed=1)).cuda()
    d_coef = jpeg.encode_device(d_img, w, h)
    data = jpeg.compress_device(d_img, w, h).cpu().numpy().tobytes()
    return d_coef.cpu().numpy().reshape(-1, 128).copy(), data, (w, h, 1)


def test_rejected_entropy_streams(gpu, oracle):
    import torch
    from lz4jpeg import jpeg
    coef, good, dims = image_stream(oracle)
    nt = 3072
    assert J.unpack(good, dims)[3:] == (len(good), J.OK)
    offs = _stream_offsets(good, nt)
    picks = [(0, 0), (1, 0), (63, 0), (64, 0), (nt - 1, 0), (700, 1), (1500, 2)]
    data = _bump_rle_len(good, offs, picks)
    assert len(data) == len(good) and J.unpack(data, dims)[3:] == (len(data), J.OK)
    want = coef.copy()
    for t, c in picks:
        want[t, E.COEF_OFF[c]:E.COEF_OFF[c] + E.N[c]] = 0
    for tile0, ntile in ((0, nt), (1, 1499), (64, 637), (65, 636)):
        inside = [(t, c) for t, c in picks if tile0 <= t < tile0 + ntile]
        got, res = gpu_decode(data, len(data), dims, tile0, ntile)
        assert res == [len(data), U64, len(inside)], (tile0, ntile)
        assert np.array_equal(got, want[tile0:tile0 + ntile]), (tile0, ntile)
    assert [len([p for p in picks if a <= p[0] < a + n]) for a, n in ((1, 1499), (64, 637), (65, 636))] \
        == [4, 2, 1]
    # the slot path counts the same streams
    d_stream = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    ent, d_res = jpeg.unpack_device(d_stream, len(data), *dims)
    back = torch.zeros(nt * 128, dtype=torch.int16, device="cuda")
    ent.decode(back)
    torch.cuda.synchronize()
    assert int(d_res[1].item()) == -1 and int(ent.status[1].item()) == len(picks)


# ---- graph capture ---------------------------------------------------------------

def test_graph_capture(gpu):
    """One captured decode replayed on two contents of equal length: a stream
    with one rejected entropy stream, then the clean one.  d_result[2] is this
    replay's count, not a running one."""
    import torch
    from lz4jpeg import jpeg
    coef, good, dims = _encoded(65)
    offs = _stream_offsets(good, 65)
    pick = next((t, 0) for t in range(65) if good[int(offs[t, 0]) + 1] > 1)
    bad = _bump_rle_len(good, offs, [pick])
    n = len(good)
    d_in = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_coef = torch.zeros(65 * 128, dtype=torch.int16, device="cuda")
    d_res = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    scratch = pack_scratch(65)

    def call():
        jpeg.decode_stream_device(d_in, n, *dims, d_coef=d_coef, d_result=d_res, scratch=scratch)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # warm-up on a third content (zeros)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for content, rejected in ((bad, 1), (good, 0)):
        d_in.copy_(torch.from_numpy(np.frombuffer(content, np.uint8).copy()))
        d_coef.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == [n, U64, rejected]
        want = coef.copy()
        if rejected:
            want[pick[0], :64] = 0
        assert np.array_equal(d_coef.cpu().numpy().reshape(65, 128), want)
