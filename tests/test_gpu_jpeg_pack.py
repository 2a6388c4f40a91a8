"""The JPR stream on the GPU (jpegr_pack_device / jpegr_unpack_device,
include/jpegr.h) against the plain-Python restatement (tests/jpr_format.py).
All calls go through the C ABI; every comparison covers the whole batch.

Tile counts: a workgroup of either kernel takes a run of 16 tiles (measured
faster than 32), the scan groups 64 tiles and its partials 4,096, so
15 / 16 / 17, 63 / 64 / 65 and 4,096 / 4,097 sit one either side of each;
31 / 32 / 33 and 47 / 48 / 49 are the other runs' ends inside a scan group."""
import ctypes
import functools

import numpy as np
import pytest

import entropy_inputs as E
import jpr_format as J

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0x5A
OK = -1                                  # ~0 read as int64
COUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 4096, 4097)


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Slots:
    """bits, meta and table of nt tiles inside one allocation, each between
    4-KiB guard regions; everything starts as 0x5A."""

    def __init__(self, nt):
        import torch
        self.nt = nt
        sizes = (nt * 256, nt * 12, nt * 1024)
        self.off, o = [], GUARD
        for s in sizes:
            self.off.append(o)
            o += (s + GUARD - 1) // GUARD * GUARD + GUARD
        self.sizes = sizes
        self.arena = torch.full((o,), FILL, dtype=torch.uint8, device="cuda")
        keep = torch.ones(o, dtype=torch.bool, device="cuda")
        for a, s in zip(self.off, sizes):
            keep[a:a + s] = False
        self.guard = keep
        self.bits, self.meta, self.table = (self.arena[a:a + s] for a, s in zip(self.off, sizes))

    def load(self, bits, meta, table):
        import torch
        self.bits.copy_(torch.from_numpy(np.ascontiguousarray(bits, np.uint8).reshape(-1)))
        self.meta.copy_(torch.from_numpy(np.ascontiguousarray(meta, np.uint32).reshape(-1).view(np.uint8)))
        self.table.copy_(torch.from_numpy(np.ascontiguousarray(table, np.uint32).reshape(-1).view(np.uint8)))
        return self

    def guards_intact(self):
        return bool((self.arena[self.guard] == FILL).all().item())

    def host(self):
        nt = self.nt
        return (self.bits.cpu().numpy().reshape(nt, 256),
                self.meta.cpu().numpy().view(np.uint32).reshape(nt, 3),
                self.table.cpu().numpy().view(np.uint32).reshape(nt, 256))


def _scratch(nt):
    import torch
    from lz4jpeg import _lib
    return torch.empty(int(_lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device="cuda")


def gpu_pack(slots, w, h, nimg, cap=None, room=0, sentinel=0xEE):
    """(bytes of the whole output allocation, length word)."""
    import torch
    from lz4jpeg import _lib
    L = _lib.lib()
    bound = int(L.jpegr_pack_bound(w, h, nimg))
    out = torch.full((bound + room,), sentinel, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    scr = _scratch(slots.nt)
    rc = L.jpegr_pack_device(_vp(slots.bits), _vp(slots.meta), _vp(slots.table), w, h, nimg,
                             _vp(out), bound if cap is None else cap, _vp(d_len), _vp(scr), _stream())
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
    scr = _scratch(nt)
    rc = _lib.lib().jpegr_unpack_device(_vp(d_in), in_len, w, h, nimg, _vp(slots.bits),
                                        _vp(slots.meta), _vp(slots.table), _vp(scr), _vp(res),
                                        _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return slots, [int(x) for x in res.cpu().tolist()]


def gpu_entropy_decode(slots):
    """(coefficients [nt, 128], status[1]) of jpegr_entropy_decode_device on the slots."""
    import torch
    from lz4jpeg import _lib
    out = torch.full((slots.nt * 128,), 12345, dtype=torch.int16, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = _lib.lib().jpegr_entropy_decode_device(_vp(slots.bits), _vp(slots.meta), _vp(slots.table),
                                                slots.nt, _vp(out), _vp(status), _stream())
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


@functools.lru_cache(maxsize=None)
def crafted(oracle):
    cb = E.crafted_batch(oracle)
    bits, meta, table, want = E.pack(cb.streams)
    nt = len(cb.streams)
    return (bits, meta, table), want, J.pack(bits, meta, table, 8 * nt, 8, 1)


@functools.lru_cache(maxsize=None)
def encoded(nt, w=None, h=None, nimg=1):
    """nt tiles of rng.integers(-3, 4) coefficients through Entropy.encode;
    the slot arrays on the host and the restatement's packing of them."""
    import torch
    from lz4jpeg import jpeg
    w, h = (8 * nt, 8) if w is None else (w, h)
    assert J.ntiles_of(w, h, nimg) == nt
    coef = np.random.default_rng(1000 + nt).integers(-3, 4, size=(nt, 128)).astype(np.int16)
    ent = jpeg.Entropy(nt)
    ent.encode(torch.from_numpy(coef.reshape(-1)).cuda())
    torch.cuda.synchronize()
    assert int(ent.status[0].item()) == 0
    arrays = (ent.bits.cpu().numpy().reshape(nt, 256),
              ent.meta.cpu().numpy().view(np.uint32).reshape(nt, 3),
              ent.table.cpu().numpy().view(np.uint32).reshape(nt, 256))
    return arrays, coef, J.pack(*arrays, w, h, nimg), (w, h, nimg)


def test_crafted_batch_with_slack(gpu, oracle):
    (bits, meta, table), _, want = crafted(oracle)
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
    arrays, _, want, (w, h, nimg) = encoded(nt)
    got, length = gpu_pack(Slots(nt).load(*arrays), w, h, nimg)
    assert length == len(want)
    assert got[:length] == want


def test_three_images(gpu):
    arrays, _, want, (w, h, nimg) = encoded(45, 40, 24, 3)
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
    arrays, want, data = crafted(oracle)
    _check_round_trip(arrays, want, data, (8 * arrays[0].shape[0], 8, 1))


def test_round_trip_4097(gpu):
    arrays, coef, data, dims = encoded(4097)
    _check_round_trip(arrays, coef, data, dims)


def test_capacity(gpu):
    arrays, _, want, (w, h, nimg) = encoded(65)
    need = len(want)
    slots = Slots(65).load(*arrays)
    for cap in (need, need - 1, 16 + 2 * 30 + 1, 16):
        got, length = gpu_pack(slots, w, h, nimg, cap=cap, room=4096)
        assert length == need, cap
        assert got[:cap] == want[:cap], cap
        assert set(got[cap:]) == {0xEE}, cap


def _mutations(good):
    """(name, bytes, in_len, verdict, malformed tile or None) of one good 65-tile stream."""
    nt = 65
    sizes = np.frombuffer(good[16:16 + 2 * nt], "<u2").astype(np.int64)
    offs = 16 + 2 * nt + np.concatenate([[0], np.cumsum(sizes)])

    def put(pos, raw):
        b = bytearray(good)
        b[pos:pos + len(raw)] = raw
        return bytes(b)

    def stream_at(t, c):                                   # offset of tile t's stream c
        p = int(offs[t])
        for _ in range(c):
            _, ncodes, nbits = good[p], good[p + 1], int.from_bytes(good[p + 2:p + 4], "little")
            p += 4 + 3 * ncodes + (nbits + 7) // 8
        return p

    i40 = 16 + 2 * 40
    return [("in_len - 1", good, len(good) - 1, 0, None),
            ("magic", put(0, b"K"), len(good), 0, None),
            ("h in the header", put(8, (16).to_bytes(4, "little")), len(good), 0, None),
            ("index entry 40 + 1", put(i40, (int(sizes[40]) + 1).to_bytes(2, "little")),
             len(good), 0, None),
            ("tile 40 luma ncodes = 129", put(stream_at(40, 0) + 1, bytes([129])), len(good), 41, 40),
            ("tile 64 Cb nbits = 513", put(stream_at(64, 2) + 2, (513).to_bytes(2, "little")),
             len(good), 65, 64)]


@pytest.mark.parametrize("k", range(6))
def test_malformed_streams(gpu, k):
    arrays, _, good, dims = encoded(65)
    name, data, in_len, verdict, bad = _mutations(good)[k]
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


def _image(oracle, w, h, kind):
    if kind == "rand":
        return oracle.rand_image(w, h, seed=1)
    yy, xx = np.mgrid[0:h, 0:w]                            # test_gpu_entropy.py's smooth image
    return np.ascontiguousarray(np.stack([(xx // 3) % 256, (yy // 2) % 256, ((xx + yy) // 5) % 256,
                                          np.full_like(xx, 255)], -1).astype(np.uint8))


@pytest.mark.parametrize("w,h,kind", [(40, 24, "rand"), (512, 384, "smooth")])
def test_compress_decompress(gpu, oracle, w, h, kind):
    import torch
    from lz4jpeg import jpeg
    d_img = torch.from_numpy(_image(oracle, w, h, kind)).cuda()
    stream = jpeg.compress_device(d_img, w, h)
    d_coef = jpeg.encode_device(d_img, w, h)
    nt = jpeg.tiles(w, h)
    ent = jpeg.Entropy(nt)
    ent.encode(d_coef)
    torch.cuda.synchronize()
    want = J.pack(ent.bits.cpu().numpy(), ent.meta.cpu().numpy().view(np.uint32),
                  ent.table.cpu().numpy().view(np.uint32), w, h, 1)
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
    _, coef_a, want_a, _ = encoded(65)
    coef_b = np.ascontiguousarray(coef_a[::-1])
    ent, back = jpeg.Entropy(nt), jpeg.Entropy(nt)
    d_out = torch.zeros(jpeg.pack_bound(w, h, nimg), dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int64, device="cuda")
    s1, s2 = _scratch(nt), _scratch(nt)

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
        arrays = (ent.bits.cpu().numpy(), ent.meta.cpu().numpy().view(np.uint32),
                  ent.table.cpu().numpy().view(np.uint32))
        want = J.pack(*arrays, w, h, nimg)
        assert len(want) == len(want_a)
        d_out.zero_()
        back.meta.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert int(d_len.item()) == len(want)
        assert d_out[:len(want)].cpu().numpy().tobytes() == want
        assert [int(x) for x in d_res.cpu().tolist()] == [len(want), OK]
        got = (back.bits.cpu().numpy(), back.meta.cpu().numpy().view(np.uint32),
               back.table.cpu().numpy().view(np.uint32))
        assert J.live_equal(arrays, got) is None
        out = torch.zeros_like(d_coef)
        back.decode(out)
        torch.cuda.synchronize()
        assert int(back.status[1].item()) == 0 and torch.equal(out, d_coef)
    assert want != want_a                                   # the two replays saw different streams
