"""jpegr_stream_encode_device (include/jpegr.h): coefficients straight to a
JPR1 / JPT1 stream, with no slots.  The expected bytes are the plain-Python
restatements' (tests/jpr_format.py, tests/jpt_format.py) over the oracle's
entropy record of every stream -- never the code under test; the GPU's
two-stage path (Entropy.encode + pack_device) is compared as a second witness.

Every run of the C call here has 4 KiB of sentinel on both sides of the
scratch it asked for and behind the output; all three are checked.

Tile counts: an encoder wave holds 64 tiles of one channel, place takes 16
tiles per workgroup, the scan groups 64 tiles and its partials 4,096."""
import ctypes
import functools

import numpy as np
import pytest

import entropy_inputs as E
import jpr_format as J
import jpt_format as T
import oracle_api
from jpr_gpu_lib import U64, coef_dev, image, random_coef, vp

pytestmark = pytest.mark.gpu

FILL, GUARD, ROOM = 0xEE, 4096, 4096
FORMATS = [False, True]                                 # tight: JPR1, JPT1


def _dims(nt):
    return (8 * nt, 8, 1)


# ---- expected bytes: the oracle's records through the restatements -----------------

def slots_of(records):
    """The slot arrays (bits [nt, 256] u8, meta [nt, 3] u32, table [nt, 256]
    u32) that hold records[tile][channel] (oracle_api.entropy's dicts)."""
    nt = len(records)
    bits = np.zeros((nt, 256), np.uint8)
    meta = np.zeros((nt, 3), np.uint32)
    table = np.zeros((nt, 256), np.uint32)
    for t, row in enumerate(records):
        for c, e in enumerate(row):
            o = J.SLOT_OFF[c]
            assert e["nbits"] <= J.SLOT_BITS[c] and len(e["table"]) <= J.SLOT_CODES[c]
            raw = np.frombuffer(e["bits"], np.uint8)
            bits[t, o:o + len(raw)] = raw
            meta[t, c] = e["nbits"] | len(e["rle"]) << 16 | len(e["table"]) << 24
            table[t, o:o + len(e["table"])] = [(v & 0xFFFF) | L << 16 for v, L, _ in e["table"]]
    return bits, meta, table


def _records(oracle, coef):
    return [[oracle_api.entropy(oracle, coef[t, E.COEF_OFF[c]:E.COEF_OFF[c] + E.N[c]])
             for c in range(3)] for t in range(coef.shape[0])]


def _want(arrays, dims, tight):
    return (T if tight else J).pack(*arrays, *dims)


@functools.lru_cache(maxsize=None)
def image_case(oracle, w, h, nimg, kind):
    """(coefficients [nt, 128] by the oracle's encoder, slot arrays of the
    oracle's entropy records) of nimg images."""
    imgs = [image(oracle, w, h, kind, seed=1 + i) for i in range(nimg)]
    coef = np.concatenate([oracle.jpeg_encode(im) for im in imgs]).reshape(-1, 128)
    return coef, slots_of(_records(oracle, coef))


@functools.lru_cache(maxsize=None)
def batch_case(oracle, name):
    return E.encoder_batch(name).coef, slots_of(E.oracle_streams(oracle, name))


@functools.lru_cache(maxsize=None)
def encoded65(oracle):
    """jpr_gpu_lib.encoded(65)'s coefficients."""
    coef = random_coef(65)
    return coef, slots_of(_records(oracle, coef))


# ---- the call ---------------------------------------------------------------------

class Run:
    """Buffers of one call: the output with ROOM sentinel bytes behind cap,
    the scratch the library asks for between two guards."""

    def __init__(self, nt, dims, tight, cap=None):
        import torch
        from lz4jpeg import _lib
        self.L = _lib.lib()
        self.dims, self.tight = dims, tight
        self.cap = int(self.L.jpegr_pack_bound(*dims)) if cap is None else cap
        self.out = torch.full((self.cap + ROOM,), FILL, dtype=torch.uint8, device="cuda")
        self.len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        self.res = torch.full((2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        self.need = int(self.L.jpegr_stream_encode_scratch_bytes(nt, self.cap))
        assert self.need <= self.cap + 128 * nt + 4096
        self.scr = torch.full((self.need + 2 * GUARD,), 0xC7, dtype=torch.uint8, device="cuda")

    def __call__(self, d_coef, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = self.L.jpegr_stream_encode_device(
            vp(d_coef), *self.dims, 2 if self.tight else 1, vp(self.out), self.cap, vp(self.len),
            vp(self.scr, GUARD), vp(self.res), ctypes.c_void_p(s.cuda_stream))
        assert rc == 0

    def result(self):
        """(bytes of out[:cap], length, result words); the guards checked."""
        host = self.out.cpu().numpy()
        assert (host[self.cap:] == FILL).all(), "a write at or past d_out + cap"
        scr = self.scr.cpu().numpy()
        assert (scr[:GUARD] == 0xC7).all() and (scr[GUARD + self.need:] == 0xC7).all(), \
            "a write outside the scratch"
        return (host[:self.cap].tobytes(), int(self.len.item()),
                [int(x) & U64 for x in self.res.cpu().tolist()])


def gpu_encode(coef, dims, tight, cap=None):
    import torch
    run = Run(coef.shape[0], dims, tight, cap)
    run(coef_dev(coef))
    torch.cuda.synchronize()
    return run.result()


def two_stage(coef, dims, tight):
    """The stream of Entropy.encode + pack_device: the second witness."""
    import torch
    from lz4jpeg import jpeg
    ent = jpeg.Entropy(coef.shape[0])
    ent.encode(coef_dev(coef))
    d_out, d_len = jpeg.pack_device(ent, *dims, tight=tight)
    torch.cuda.synchronize()
    assert int(ent.status[0].item()) == 0
    return d_out[:int(d_len.item())].cpu().numpy().tobytes()


def _check(coef, arrays, dims, tight, name=""):
    want = _want(arrays, dims, tight)
    got, length, res = gpu_encode(coef, dims, tight)
    assert length == len(want), name
    assert res == [len(want), 0], name                  # [1]: no stream overflows the reference's buffers
    assert got[:length] == want, name
    assert set(got[length:]) <= {FILL}, name            # nothing behind the stream
    assert two_stage(coef, dims, tight) == want, name
    return want


# ---- bytes ------------------------------------------------------------------------

@pytest.mark.parametrize("tight", FORMATS)
@pytest.mark.parametrize("w,h,nimg", [(8, 8, 1), (40, 24, 1), (136, 64, 1), (520, 512, 1), (72, 40, 3)])
@pytest.mark.parametrize("kind", ["rand", "smooth"])
def test_image_bytes(gpu, oracle, w, h, nimg, kind, tight):
    """520 x 512 is 4,160 tiles, past the scan's 4,096-tile partial; 72 x 40 x 3
    has its image boundaries inside a workgroup."""
    coef, arrays = image_case(oracle, w, h, nimg, kind)
    want = _check(coef, arrays, (w, h, nimg), tight)
    assert (T if tight else J).header(want) == (w, h, nimg)


@pytest.mark.parametrize("tight", FORMATS)
@pytest.mark.parametrize("name", E.encoder_batch_names())
def test_encoder_batches(gpu, oracle, name, tight):
    """umax_sweep, u_ladder, deferral, sized, values: deferred luma lanes taken
    by the chroma kernel, 0 to 64 deferred lanes, partial last waves, int16
    extremes (JPT1 mode 2), mode 1."""
    coef, arrays = batch_case(oracle, name)
    _check(coef, arrays, _dims(coef.shape[0]), tight, name)
    if tight and name in ("values", "deferral"):
        modes = set(T.stream_modes(*arrays).reshape(-1).tolist())
        assert (2 if name == "values" else 1) in modes


@pytest.mark.parametrize("tight", FORMATS)
@pytest.mark.parametrize("defer_last", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_counts(gpu, oracle, n, defer_last, tight):
    coef = E.sized(n, defer_last).coef
    _check(coef, slots_of(_records(oracle, coef)), _dims(n), tight, (n, defer_last))


# ---- capacity ---------------------------------------------------------------------

@pytest.mark.parametrize("tight", FORMATS)
def test_capacity(gpu, oracle, tight):
    """A cap short of the stream: the exact need is reported, out[:cap] is the
    stream's first cap bytes (the tiles that start below cap are encoded again
    into the arena, whatever the first pass dropped), nothing past cap."""
    coef, arrays = encoded65(oracle)
    dims = (520, 8, 1)
    want = _want(arrays, dims, tight)
    need = len(want)
    mid = 16 + 2 * 65 + int(np.frombuffer(want[16:16 + 2 * 30], "<u2").sum()) + 7   # inside record 30
    for cap in (need, need - 1, mid, 16 + 2 * 30 + 1, 16):
        got, length, res = gpu_encode(coef, dims, tight, cap=cap)
        assert length == need and res == [need, 0], cap
        assert got == want[:cap], cap


@pytest.mark.parametrize("tight", FORMATS)
def test_capacity_many_waves(gpu, oracle, tight):
    """4,160 tiles: the first pass's waves share out the arena between several
    bump counters, and a cap of exactly the stream, or short of it, leaves no
    counter more than its share."""
    coef, arrays = image_case(oracle, 520, 512, 1, "rand")
    dims = (520, 512, 1)
    want = _want(arrays, dims, tight)
    need = len(want)
    for cap in (need, need - 1, need // 2, 16 + 2 * 4160 + 5):
        got, length, res = gpu_encode(coef, dims, tight, cap=cap)
        assert length == need and res == [need, 0], cap
        assert got == want[:cap], cap


# ---- determinism, graphs, concurrency ---------------------------------------------

@pytest.mark.parametrize("tight", FORMATS)
def test_determinism(gpu, oracle, tight):
    """The arena order is free to differ from run to run; the bytes are not."""
    coef, arrays = image_case(oracle, 520, 512, 1, "rand")
    want = _want(arrays, (520, 512, 1), tight)
    for _ in range(5):
        got, length, res = gpu_encode(coef, (520, 512, 1), tight)
        assert length == len(want) and res == [len(want), 0] and got[:length] == want


@pytest.mark.parametrize("tight", FORMATS)
def test_graph_capture(gpu, oracle, tight):
    """One call captured on one stream (no parallel branches), replayed on two
    contents of the same d_coef: each replay initialises the bump counters and
    the result words itself and gives its own length and bytes."""
    import torch
    coef_a, arrays_a = encoded65(oracle)
    coef_b, arrays_b = batch_case(oracle, "size65_defer")
    dims = (520, 8, 1)
    run = Run(65, dims, tight)
    d_coef = torch.zeros(65 * 128, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(d_coef, side)                               # warm-up on a third content
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(d_coef)
    lengths = []
    for coef, arrays in ((coef_a, arrays_a), (coef_b, arrays_b), (coef_a, arrays_a)):
        want = _want(arrays, dims, tight)
        d_coef.copy_(coef_dev(coef))
        run.out.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        got, length, res = run.result()
        assert length == len(want) and res == [len(want), 0]
        assert got[:length] == want and set(got[length:]) <= {FILL}
        lengths.append(length)
    assert lengths[0] != lengths[1]


@pytest.mark.parametrize("tight", FORMATS)
def test_two_calls_in_flight(gpu, oracle, tight):
    import torch
    cases = [image_case(oracle, 520, 512, 1, "rand"), image_case(oracle, 520, 512, 1, "smooth")]
    dims = (520, 512, 1)
    runs = [Run(4160, dims, tight), Run(4160, dims, tight)]
    d_coefs = [coef_dev(c[0]) for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for run, d, s in zip(runs, d_coefs, streams):
            run(d, s)
    torch.cuda.synchronize()
    for run, (_, arrays) in zip(runs, cases):
        want = _want(arrays, dims, tight)
        got, length, res = run.result()
        assert length == len(want) and res == [len(want), 0] and got[:length] == want


# ---- round trip and the Python layer ----------------------------------------------

@pytest.mark.parametrize("tight", FORMATS)
def test_round_trip(gpu, oracle, tight):
    import torch
    from lz4jpeg import jpeg
    for coef, dims in ((image_case(oracle, 72, 40, 3, "rand")[0], (72, 40, 3)),
                       (batch_case(oracle, "values")[0], _dims(E.encoder_batch("values").coef.shape[0]))):
        assert coef.shape[0] == J.ntiles_of(*dims)
        d_coef = coef_dev(coef)
        d_out, d_len, d_res = jpeg.encode_stream_device(d_coef, *dims, tight=tight)
        n = int(d_len.item())
        assert d_res.cpu().tolist() == [n, 0]
        back, res = jpeg.decode_stream_device(d_out, n, *dims)
        assert [int(x) & U64 for x in res.cpu().tolist()] == [n, U64, 0]
        assert torch.equal(back, d_coef)


@pytest.mark.parametrize("tight", FORMATS)
def test_compress_device_direct(gpu, oracle, tight):
    import torch
    from lz4jpeg import jpeg
    w, h, nimg = 72, 40, 3
    img = np.concatenate([oracle.rand_image(w, h, seed=1 + i).reshape(-1) for i in range(nimg)])
    d_img = torch.from_numpy(img).cuda()
    direct = jpeg.compress_device(d_img, w, h, nimg, tight=tight, direct=True)
    assert torch.equal(direct, jpeg.compress_device(d_img, w, h, nimg, tight=tight))
    _, arrays = image_case(oracle, w, h, nimg, "rand")
    assert direct.cpu().numpy().tobytes() == _want(arrays, (w, h, nimg), tight)


@pytest.mark.parametrize("tight", FORMATS)
def test_exact_encode_grows(gpu, oracle, tight):
    """compress_device's direct path starts from a quarter of the bound: a
    stream past its first capacity is encoded again into exactly what the first
    call asked for."""
    from lz4jpeg import jpeg
    coef, arrays = batch_case(oracle, "size65_defer")
    want = _want(arrays, _dims(65), tight)
    for cap in (16, len(want) // 2, len(want), None):
        d_out, over = jpeg.encode_stream_exact_device(coef_dev(coef), *_dims(65), tight=tight, cap=cap)
        assert over == 0 and d_out.cpu().numpy().tobytes() == want, cap
