"""Driving the JPEG stream entry points (include/jpegr.h) on the device, and the
inputs the stream tests share (a helper, no tests): slot arrays on the host
are (bits [nt, 256] u8, meta [nt, 3] u32, table [nt, 256] u32), coefficients
[nt, 128] int16, dims (w, h, nimg).  The cached results are shared: read them,
do not change them.
"""
import ctypes
import functools

import numpy as np

import entropy_inputs as E
import jpr_format as J
import jpt_inputs as I

U64 = (1 << 64) - 1
SENTINEL = 12345                         # int16 around and under decoded coefficients
PAD = 64                                 # int16 either side of the coefficients (128 B)
GUARD = 4096
FILL = 0x5A


def vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack_scratch(nt):
    import torch
    from lz4jpeg import _lib
    return torch.empty(int(_lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device="cuda")


def to_dev(a, dtype):
    """The array's bytes as a flat uint8 tensor on the device."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1).view(np.uint8).copy()).cuda()


def dev_bytes(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()


def dev_u64(values):
    import torch
    return torch.from_numpy(np.array([int(v) & U64 for v in values], np.uint64).view(np.int64)).cuda()


def host_offsets(data, dims):
    """ntiles + 1 offsets: the cumulative sum of the u16 index from 16 + 2 ntiles."""
    nt = J.ntiles_of(*dims)
    sizes = np.frombuffer(data[16:16 + 2 * nt], "<u2").astype(np.uint64)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64) + np.uint64(16 + 2 * nt)


def coef_dev(coef):
    import torch
    return torch.from_numpy(np.array(coef, np.int16).reshape(-1)).cuda()


def slot_arrays(ent, nt):
    """The host's slot arrays of anything with bits, meta and table tensors."""
    return (ent.bits.cpu().numpy().reshape(nt, 256),
            ent.meta.cpu().numpy().view(np.uint32).reshape(nt, 3),
            ent.table.cpu().numpy().view(np.uint32).reshape(nt, 256))


def encode_slots(coef):
    """The GPU entropy encoder's slots of coefficients [nt, 128], on the host."""
    import torch
    from lz4jpeg import jpeg
    nt = coef.shape[0]
    ent = jpeg.Entropy(nt)
    ent.encode(coef_dev(coef))
    torch.cuda.synchronize()
    assert int(ent.status[0].item()) == 0
    return slot_arrays(ent, nt)


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
        self.bits.copy_(to_dev(bits, np.uint8))
        self.meta.copy_(to_dev(meta, np.uint32))
        self.table.copy_(to_dev(table, np.uint32))
        return self

    def guards_intact(self):
        return bool((self.arena[self.guard] == FILL).all().item())

    def host(self):
        return slot_arrays(self, self.nt)


def gpu_decode(data, in_len, dims, tile0=0, ntile=None, tail=b"", lead=0):
    """(coefficients [ntile, 128], [implied, verdict, rejected] as unsigned) of
    the direct decode of data[:in_len], which sits `lead` bytes into its
    buffer and is followed there by data[in_len:] + tail.  d_coef is a 16-B
    aligned view inside a sentinel-filled tensor whose sentinels are checked;
    d_result starts as garbage."""
    import torch
    from lz4jpeg import jpeg
    w, h, nimg = dims
    nt = J.ntiles_of(w, h, nimg)
    ntile = nt - tile0 if ntile is None else ntile
    buf = torch.from_numpy(np.frombuffer(bytes(lead) + bytes(data) + bytes(tail), np.uint8).copy()).cuda()
    big = torch.full((ntile * 128 + 2 * PAD,), SENTINEL, dtype=torch.int16, device="cuda")
    view = big[PAD:PAD + ntile * 128]
    assert view.data_ptr() % 16 == 0
    res = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    out, r = jpeg.decode_stream_device(buf[lead:], in_len, w, h, nimg, tile0, ntile, d_coef=view,
                                       d_result=res)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr() and r.data_ptr() == res.data_ptr()
    host = big.cpu().numpy()
    assert (host[:PAD] == SENTINEL).all() and (host[-PAD:] == SENTINEL).all()
    return host[PAD:-PAD].reshape(ntile, 128).copy(), [int(x) & U64 for x in res.cpu().tolist()]


# ---- shared inputs ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def crafted(oracle):
    """The crafted decoder batch (704 tiles): (slot arrays, expected coefficients, dims)."""
    cb = E.crafted_batch(oracle)
    bits, meta, table, want = E.pack(cb.streams)
    nt = len(cb.streams)
    assert nt == 704
    return (bits, meta, table), want, (8 * nt, 8, 1)


@functools.lru_cache(maxsize=None)
def crafted_jpr(oracle):
    """The restatement's JPR1 stream of the crafted batch."""
    arrays, _, dims = crafted(oracle)
    return J.pack(*arrays, *dims)


def random_coef(nt):
    return np.random.default_rng(1000 + nt).integers(-3, 4, size=(nt, 128)).astype(np.int16)


@functools.lru_cache(maxsize=None)
def encoded(nt, w=None, h=None, nimg=1):
    """nt tiles of rng.integers(-3, 4) coefficients through Entropy.encode:
    (slot arrays, coefficients, dims)."""
    w, h = (8 * nt, 8) if w is None else (w, h)
    assert J.ntiles_of(w, h, nimg) == nt
    coef = random_coef(nt)
    return encode_slots(coef), coef, (w, h, nimg)


@functools.lru_cache(maxsize=None)
def encoded_jpr(*args):
    """The restatement's JPR1 stream of encoded(*args)'s slots."""
    arrays, _, dims = encoded(*args)
    return J.pack(*arrays, *dims)


def image(oracle, w, h, kind, seed=1):
    return oracle.rand_image(w, h, seed=seed) if kind == "rand" else I.smooth_image(w, h)


def jpr_mutations(good):
    """(name, bytes, in_len, verdict, malformed tile or None) of one good 65-tile JPR1 stream."""
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
            ncodes, nbits = good[p + 1], int.from_bytes(good[p + 2:p + 4], "little")
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
