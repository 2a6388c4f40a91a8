"""The JPR stream on the GPU (jpegr_pack_device / jpegr_unpack_device,
include/jpegr.h) against the plain-Python restatement (tests/jpr_format.py).
All calls go through the C ABI; every comparison covers the whole batch.

Tile counts: a workgroup of either kernel takes a run of 16 tiles (measured
faster than 32), the scan groups 64 tiles and its partials 4,096, so
15 / 16 / 17, 63 / 64 / 65 and 4,096 / 4,097 sit one either side of each;
31 / 32 / 33 and 47 / 48 / 49 are the other runs' ends inside a scan group."""
import numpy as np
import pytest

import jpr_format as J
from jpr_gpu_lib import (Slots, crafted, crafted_jpr, current_stream, encoded, encoded_jpr, image,
                         jpr_mutations, pack_scratch, slot_arrays, vp)

pytestmark = pytest.mark.gpu

OK = -1                                  # ~0 read as int64
COUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 4096, 4097)


def gpu_pack(slots, w, h, nimg, cap=None, room=0, sentinel=0xEE):
    """(bytes of the whole output allocation, length word)."""
    import torch
    from lz4jpeg import _lib
    L = _lib.lib()
    bound = int(L.jpegr_pack_bound(w, h, nimg))
    out = torch.full((bound + room,), sentinel, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    scr = pack_scratch(slots.nt)
    rc = L.jpegr_pack_device(vp(slots.bits), vp(slots.meta), vp(slots.table), w, h, nimg,
                             vp(out), bound if cap is None else cap, vp(d_len), vp(scr), current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), int(d_len.item())


def gpu_unpack(data, in_len, w, h, nimg, pad=0):
    """Unpack `data`'s first in_len bytes into fresh 0x5A-filled slots;
    returns (slots, [implied, verdict])."""
    import torch
    from lz4jpeg import _lib
    nt = J.ntiles_of(w, h, nimg)
    slots = Slots(nt)
    d_in = torch.from_numpy(np.frombuffer(bytes(data) + bytes(pad), np.uint8).copy()).cuda()
    res = torch.zeros(2, dtype=torch.int64, device="cuda")
    scr = pack_scratch(nt)
    rc = _lib.lib().jpegr_unpack_device(vp(d_in), in_len, w, h, nimg, vp(slots.bits),
                                        vp(slots.meta), vp(slots.table), vp(scr), vp(res),
                                        current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return slots, [int(x) for x in res.cpu().tolist()]


def gpu_entropy_decode(slots):
    """(coefficients [nt, 128], status[1]) of jpegr_entropy_decode_device on the slots."""
    import torch
    from lz4jpeg import _lib
    out = torch.full((slots.nt * 128,), 12345, dtype=torch.int16, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = _lib.lib().jpegr_entropy_decode_device(vp(slots.bits), vp(slots.meta), vp(slots.table),
                                                slots.nt, vp(out), vp(status), current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(-1, 128), int(status[1].item())


def with_slack(bits, meta, table):
    """Every slot byte past ceil(nbits / 8) = 0xA5, every table word past
    ncodes = 0xA5A5A5A5: what jpegr.h leaves unspecified."""
    bits, table = bits.copy(), table.copy()
    col = np.arange(256)
    for c in range(3):
        o, n = J.SLOT_OFF[c], J.SLOT_CODES[c]
        k = col[None, o:o + n] - o
        nby = ((meta[:, c] & 0xFFFF) + 7) // 8
        bits[:, o:o + n][k >= nby[:, None]] = 0xA5
        table[:, o:o + n][k >= (meta[:, c] >> 24)[:, None]] = 0xA5A5A5A5
    return bits, table


def test_crafted_batch_with_slack(gpu, oracle):
    (bits, meta, table), _, _ = crafted(oracle)
    want = crafted_jpr(oracle)
    nt = bits.shape[0]
    sb, st = with_slack(bits, meta, table)
    assert not np.array_equal(sb, bits) and not np.array_equal(st, table)
    assert J.pack(sb, meta, st, 8 * nt, 8, 1) == want       # the restatement ignores the slack too
    slots = Slots(nt).load(sb, meta, st)
    got, length = gpu_pack(slots, 8 * nt, 8, 1)
    assert length == len(want)
    assert got[:length] == want
    assert set(got[length:]) <= {0xEE}                      # nothing past the stream
    assert slots.guards_intact()


@pytest.mark.parametrize("nt", COUNTS)
def test_tile_counts(gpu, nt):
    arrays, _, (w, h, nimg) = encoded(nt)
    want = encoded_jpr(nt)
    got, length = gpu_pack(Slots(nt).load(*arrays), w, h, nimg)
    assert length == len(want)
    assert got[:length] == want


def test_three_images(gpu):
    arrays, _, (w, h, nimg) = encoded(45, 40, 24, 3)
    want = encoded_jpr(45, 40, 24, 3)
    got, length = gpu_pack(Slots(45).load(*arrays), w, h, nimg)
    assert length == len(want) and got[:length] == want
    assert J.header(got) == (40, 24, 3)


def _check_round_trip(arrays, want_coef, data, dims):
    slots, (implied, verdict) = gpu_unpack(data, len(data), *dims)
    assert (implied, verdict) == (len(data), OK)
    assert slots.guards_intact()
    assert J.live_equal(arrays, slots.host()) is None
    got, failed = gpu_entropy_decode(slots)
    assert failed == 0
    assert np.array_equal(got, want_coef)


def test_round_trip_crafted(gpu, oracle):
    arrays, want, dims = crafted(oracle)
    _check_round_trip(arrays, want, crafted_jpr(oracle), dims)


def test_round_trip_4097(gpu):
    arrays, coef, dims = encoded(4097)
    _check_round_trip(arrays, coef, encoded_jpr(4097), dims)


def test_capacity(gpu):
    arrays, _, (w, h, nimg) = encoded(65)
    want = encoded_jpr(65)
    need = len(want)
    slots = Slots(65).load(*arrays)
    for cap in (need, need - 1, 16 + 2 * 30 + 1, 16):
        got, length = gpu_pack(slots, w, h, nimg, cap=cap, room=4096)
        assert length == need, cap
        assert got[:cap] == want[:cap], cap
        assert set(got[cap:]) == {0xEE}, cap


@pytest.mark.parametrize("k", range(6))
def test_malformed_streams(gpu, k):
    arrays, _, dims = encoded(65)
    name, data, in_len, verdict, bad = jpr_mutations(encoded_jpr(65))[k]
    assert J.unpack(data[:in_len], dims)[4] == verdict, name        # the restatement agrees
    slots, (implied, got) = gpu_unpack(data, in_len, *dims, pad=16)
    assert got == verdict, name
    assert implied == J.unpack(data[:in_len], dims)[3], name
    assert slots.guards_intact(), name
    if bad is not None:
        b, m, t = slots.host()
        assert not m[bad].any(), name                               # left with ncodes = 0
        rest = np.arange(65) != bad
        assert J.live_equal(tuple(a[rest] for a in arrays), (b[rest], m[rest], t[rest])) is None, name


@pytest.mark.parametrize("w,h,kind", [(40, 24, "rand"), (512, 384, "smooth")])
def test_compress_decompress(gpu, oracle, w, h, kind):
    import torch
    from lz4jpeg import jpeg
    d_img = torch.from_numpy(image(oracle, w, h, kind)).cuda()
    stream = jpeg.compress_device(d_img, w, h)
    d_coef = jpeg.encode_device(d_img, w, h)
    nt = jpeg.tiles(w, h)
    ent = jpeg.Entropy(nt)
    ent.encode(d_coef)
    torch.cuda.synchronize()
    want = J.pack(*slot_arrays(ent, nt), w, h, 1)
    assert stream.dtype == torch.uint8 and stream.cpu().numpy().tobytes() == want
    rgba, gw, gh, gn = jpeg.decompress_device(stream)
    assert (gw, gh, gn) == (w, h, 1)
    assert torch.equal(rgba, jpeg.reconstruct_device(d_coef, w, h))
    bad = stream.clone()
    bad[0] = 0
    with pytest.raises(jpeg.JpegError):
        jpeg.decompress_device(bad)
    bad = stream.clone()
    bad[16] ^= 1                                            # index entry 0: implied length off by one
    with pytest.raises(jpeg.JpegError):
        jpeg.decompress_device(bad)


def test_graph_capture(gpu):
    """pack + unpack captured in one graph; replayed on two contents (the
    second holds the first's tiles in reverse order: another stream of the
    same length, which unpack's captured in_len needs)."""
    import torch
    from lz4jpeg import jpeg
    nt, (w, h, nimg) = 65, (8 * 65, 8, 1)
    coef_a, want_a = encoded(65)[1], encoded_jpr(65)
    coef_b = np.ascontiguousarray(coef_a[::-1])
    ent, back = jpeg.Entropy(nt), jpeg.Entropy(nt)
    d_out = torch.zeros(jpeg.pack_bound(w, h, nimg), dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int64, device="cuda")
    s1, s2 = pack_scratch(nt), pack_scratch(nt)

    def both():
        jpeg.pack_device(ent, w, h, nimg, d_out=d_out, d_len=d_len, scratch=s1)
        jpeg.unpack_device(d_out, len(want_a), w, h, nimg, ent=back, d_result=d_res, scratch=s2)

    ent.encode(torch.zeros(nt * 128, dtype=torch.int16, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                              # warm-up on a third content
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for coef in (coef_a, coef_b):
        d_coef = torch.from_numpy(coef.reshape(-1)).cuda()
        ent.encode(d_coef)
        torch.cuda.synchronize()
        arrays = slot_arrays(ent, nt)
        want = J.pack(*arrays, w, h, nimg)
        assert len(want) == len(want_a)
        d_out.zero_()
        back.meta.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert int(d_len.item()) == len(want)
        assert d_out[:len(want)].cpu().numpy().tobytes() == want
        assert [int(x) for x in d_res.cpu().tolist()] == [len(want), OK]
        assert J.live_equal(arrays, slot_arrays(back, nt)) is None
        out = torch.zeros_like(d_coef)
        back.decode(out)
        torch.cuda.synchronize()
        assert int(back.status[1].item()) == 0 and torch.equal(out, d_coef)
    assert want != want_a                                   # the two replays saw different streams
