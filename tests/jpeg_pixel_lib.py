"""Driving the JPEG pixel stage (include/jpegr.h: encode, raw DCT, reconstruct,
planes and the block kernels) through the C ABI with explicit pointers, inside
guard arenas, and the inputs its tests share (a helper, no tests).

An arena is a uint8 device tensor: GUARD bytes, `off` more, the payload, and
at least GUARD bytes behind it.  An output arena starts as FILL everywhere;
after the call all of it comes back, the payload is compared with the
expectation and every other byte must still be FILL.  An input arena's lead
and tail hold 0x00 on one run and 0xFF on the other: bytes outside the input
must not reach the result.
"""
import ctypes

import numpy as np

import oracle_api

GUARD = 4096
FILL = 0xA5
INPUT_FILLS = (0x00, 0xFF)

# the sweep: every w mod 8 below one strip, the end of the first strip (32 tiles,
# 256 px) and the start of the second, two full strips and a ragged third
WIDTHS = tuple(range(1, 41)) + tuple(range(249, 265)) + tuple(range(505, 521))
HEIGHTS = tuple(range(1, 18))
WIDTH_GROUPS = tuple(WIDTHS[i:i + 8] for i in range(0, len(WIDTHS), 8))
NIMG = 2


def pixel_offset(w, h):
    """Bytes past a 16-B boundary at which the sweep puts its pixel pointers."""
    return 4 * ((w + h) % 4)


def tiles_of(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


def quirk_tiles(w, h):
    """Tiles at raster index >= ceil(w h / 64): never transformed by the reference."""
    return tiles_of(w, h) - min(tiles_of(w, h), (w * h + 63) // 64)


def sweep_images(oracle, w, h):
    """The sweep's batch of a geometry: NIMG distinct images, [NIMG, h, w, 4]."""
    return np.stack([oracle.rand_image(w, h, seed=1 + 7 * (1000 * h + w) + i) for i in range(NIMG)])


class Expect:
    """The oracle's answers for one geometry's batch, each as flat per-image rows."""

    def __init__(self, oracle, w, h, imgs=None, recon_only=False):
        self.w, self.h = w, h
        self.imgs = sweep_images(oracle, w, h) if imgs is None else imgs
        self.coef = np.stack([oracle.jpeg_encode(i) for i in self.imgs])            # [n, tiles*128] i16
        if not recon_only:
            self.raw = np.stack([oracle.jpeg_dct_raw(i) for i in self.imgs])        # [n, tiles*128] f64
        self.rec_orig = np.stack([oracle_api.reconstruct(oracle, i) for i in self.imgs])
        self.rec_all = np.stack([oracle_api.decode_every_tile(oracle, c, w, h) for c in self.coef])


# ---- arenas ---------------------------------------------------------------------

def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Arena:
    """nbytes of payload `off` bytes past GUARD in a tensor of `fill`; the
    allocation is 16-B aligned, so ptr % 16 == off % 16."""

    def __init__(self, nbytes, off=0, fill=FILL):
        import torch
        assert 0 <= off < GUARD
        self.nbytes, self.start, self.fill = int(nbytes), GUARD + off, fill
        total = (self.start + self.nbytes + GUARD + 255) // 256 * 256
        self.t = torch.full((total,), fill, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.start

    def vp(self, byte_off=0):
        return ctypes.c_void_p(self.ptr + byte_off)

    def load(self, a):
        """The array's bytes into the payload (an input arena, or an in-place operand)."""
        import torch
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        assert b.size <= self.nbytes
        self.t[self.start:self.start + b.size].copy_(torch.from_numpy(b.copy()))
        return self

    def host(self):
        return self.t.cpu().numpy()

    def problem(self, want, per_image=None):
        """None, or what is wrong: the first guard byte touched and its distance
        from the payload, else the first element that differs from `want` (an
        array whose bytes fill the payload; per_image: elements an image)."""
        got = self.host()
        lo, hi = self.start, self.start + self.nbytes
        lead = np.flatnonzero(got[:lo] != self.fill)
        if lead.size:                         # the one nearest to the payload first
            return (f"guard byte {lo - int(lead[-1])} B before the payload touched "
                    f"(0x{got[lead[-1]]:02x}; {lead.size} in all)")
        tail = np.flatnonzero(got[hi:] != self.fill)
        if tail.size:
            return (f"guard byte {int(tail[0])} B past the payload's end touched "
                    f"(0x{got[hi + tail[0]]:02x}; {tail.size} in all)")
        want = np.ascontiguousarray(want).reshape(-1)
        assert want.nbytes == self.nbytes, (want.nbytes, self.nbytes)
        have = got[lo:hi].view(want.dtype)
        cmp_t = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[want.dtype.itemsize]
        bad = np.flatnonzero(have.view(cmp_t) != want.view(cmp_t))      # bit for bit
        if bad.size:
            k = int(bad[0])
            where = f"element {k}" if per_image is None else \
                f"image {k // per_image} element {k % per_image}"
            return f"{where}: got {have[k]!r}, want {want[k]!r} ({bad.size} differ)"
        return None


def filled(n, dtype):
    """n elements whose bytes are all FILL: the untouched part of an expectation."""
    return np.full(n * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


# ---- drivers: the C ABI with explicit pointers ------------------------------------

def _L():
    from lz4jpeg import _lib
    return _lib.lib()


def encode(d_rgba, w, h, nimg, d_out):
    return _L().jpegr_encode_device(d_rgba, w, h, nimg, d_out, _stream())


def dct_raw(d_rgba, w, h, nimg, d_out):
    return _L().jpegr_dct_raw_device(d_rgba, w, h, nimg, d_out, _stream())


def reconstruct(d_coef, d_orig, w, h, nimg, d_out):
    return _L().jpegr_reconstruct_device(d_coef, d_orig, w, h, nimg, d_out, _stream())


def planes(d_rgba, w, h, d_y, d_cr, d_cb):
    return _L().jpegr_planes_device(d_rgba, w, h, d_y, d_cr, d_cb, _stream())


def dct_blocks(d_blocks, width, nblocks, d_out):
    return _L().jpegr_dct_blocks_device(d_blocks, width, 8, nblocks, d_out, _stream())


def quantize(d_coef, d_table, size, n):
    return _L().jpegr_quantize_device(d_coef, d_table, size, n, _stream())


def permute(d_in, d_out, d_perm, size, n):
    return _L().jpegr_permute_device(d_in, d_out, d_perm, size, n, _stream())


def run_reconstruct(coef, w, h, nimg, orig=None, off=0, in_fill=0x00):
    """jpegr_reconstruct_device on coefficients [.., 128] int16 (and the images
    `orig`, or NULL), every buffer in an arena: the output arena."""
    cin = Arena(coef.size * 2, 0, in_fill).load(np.ascontiguousarray(coef, np.int16))
    oin = None if orig is None else Arena(orig.size, off, in_fill).load(orig)
    out = Arena(nimg * w * h * 4, off)
    rc = reconstruct(cin.vp(), None if oin is None else oin.vp(), w, h, nimg, out.vp())
    assert rc == 0, rc
    return out


# ---- reconstruction on coefficients the encoder never makes ------------------------

OFFGRID_W, OFFGRID_H = 264, 16            # 33 x 2 tiles: a second strip of one tile
OFFGRID_TILES = NIMG * tiles_of(OFFGRID_W, OFFGRID_H)        # 132 a call
ROUNDING_CLASSES = ("pm3", "pm40")       # the ones that must leave samples off the clamps


def _peaks(value):
    """128 tiles, tile p zero except position p = value; the call's last 4 tiles zero."""
    c = np.zeros((OFFGRID_TILES, 128), np.int16)
    c[np.arange(128), np.arange(128)] = value
    return c


def offgrid_classes():
    """name -> coefficients [132, 128] int16 of one 264 x 16 x 2 call.  All are
    defined inputs for the reference: the largest sample magnitude is below
    32 * 32768 * 99 * 0.36 < 2^26, so (int)round(s + 128) does not overflow."""
    rng = np.random.default_rng(20261)
    shape = (OFFGRID_TILES, 128)
    flat = np.empty(shape, np.int16)
    flat[0::2] = 32767
    flat[1::2] = -32768
    return {
        "pm3": rng.integers(-3, 4, shape).astype(np.int16),
        "pm40": rng.integers(-40, 41, shape).astype(np.int16),
        "int16": rng.integers(-32768, 32768, shape).astype(np.int16),
        "peak+": _peaks(32767),
        "peak-": _peaks(-32768),
        "flat": flat,
    }


def offgrid_expect(oracle, coef):
    """decode_every_tile of each image of a class: [NIMG, h, w, 4]."""
    per = coef.reshape(NIMG, -1)
    return np.stack([oracle_api.decode_every_tile(oracle, c, OFFGRID_W, OFFGRID_H) for c in per])


def in_range_share(want):
    """The share of R, G, B bytes in 1..254 (not on a clamp)."""
    rgb = want[..., :3]
    return float(np.count_nonzero((rgb >= 1) & (rgb <= 254))) / rgb.size
