"""The pixel stage's kernels -- jpeg_strip_kernel (quantised and raw) and
jpeg_recon_kernel (with and without d_rgba_orig) -- on every small geometry at
which they take another path, under guard bands (tests/jpeg_pixel_lib.py).

The kernels branch on w mod 8 (ragged tile), w mod 4 (the 16-B load of phase 1,
store_px4's 16-B or dword stores), w mod 2 (the odd chroma column outside the
image), the 32-tile strip edge at 256 px, h mod 8, and on whether ceil(w h / 64)
is below the tile count (the tiles the reference never transforms).  The sweep
is w in 1..40, 249..264, 505..520 by h in 1..17, two distinct images a call, the
pixel pointers 4 ((w + h) mod 4) bytes past a 16-B boundary, every output in an
arena of 0xA5 whose every byte outside the payload must survive, every input
between a lead and a tail of 0x00 on one run and 0xFF on the other.  Each call
is compared with the oracle alone; the reconstruction is fed the oracle's
coefficients, not the GPU encoder's, so each kernel stands on its own.

The first three tests need no GPU: they show from the oracle alone that the
sweep reaches what it is meant to reach.
"""
import numpy as np
import pytest

import jpeg_pixel_lib as P


def test_every_width_class_meets_every_pointer_offset():
    assert len(P.WIDTHS) * len(P.HEIGHTS) == 1224
    assert [len(g) for g in P.WIDTH_GROUPS] == [8] * 9
    pairs = {(w % 8, P.pixel_offset(w, h)) for w in P.WIDTHS for h in P.HEIGHTS}
    assert pairs == {(m, o) for m in range(8) for o in (0, 4, 8, 12)}
    # and so on either side of the strip edge and in the ragged third strip
    for lo, hi in ((1, 40), (249, 256), (257, 264), (505, 512), (513, 520)):
        part = {(w % 8, P.pixel_offset(w, h)) for w in P.WIDTHS if lo <= w <= hi for h in P.HEIGHTS}
        assert len(part) == 32, (lo, hi)


def test_most_geometries_have_tiles_the_reference_never_transforms():
    n = sum(1 for w in P.WIDTHS for h in P.HEIGHTS if P.quirk_tiles(w, h) > 0)
    assert n >= 900, n
    assert P.quirk_tiles(40, 16) == 0 and P.quirk_tiles(37, 21) == 2


def test_the_two_reconstruction_expectations_differ(oracle):
    """d_rgba_orig given and NULL are different questions in at least 900 of the
    1,224 geometries: the sweep tells the two kernels apart."""
    geoms = images = 0
    for w in P.WIDTHS:
        for h in P.HEIGHTS:
            if P.quirk_tiles(w, h) == 0:
                continue                                   # the same tiles are decoded
            e = P.Expect(oracle, w, h, recon_only=True)
            d = [not np.array_equal(e.rec_orig[i], e.rec_all[i]) for i in range(P.NIMG)]
            geoms += any(d)
            images += sum(d)
    assert geoms >= 900, (geoms, images)


def _fail(w, h, call, fill, what):
    return f"{call} w={w} h={h} nimg={P.NIMG} input fill 0x{fill:02x}: {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("widths", P.WIDTH_GROUPS, ids=lambda g: f"w{g[0]}-{g[-1]}")
def test_sweep(gpu, oracle, widths):
    import torch
    for w in widths:
        for h in P.HEIGHTS:
            e = P.Expect(oracle, w, h)
            off = P.pixel_offset(w, h)
            tiles = P.tiles_of(w, h)
            npx = w * h
            assert e.imgs[1].tobytes() != e.imgs[0].tobytes()
            for fill in P.INPUT_FILLS:
                img = P.Arena(e.imgs.size, off, fill).load(e.imgs)
                coef = P.Arena(e.coef.size * 2, 0, fill).load(e.coef)
                assert img.ptr % 16 == off and coef.ptr % 16 == 0
                outs = []

                a = P.Arena(P.NIMG * tiles * 256, 0)
                assert P.encode(img.vp(), w, h, P.NIMG, a.vp()) == 0
                outs.append(("jpegr_encode_device", a, e.coef, tiles * 128))

                a = P.Arena(P.NIMG * tiles * 1024, 0)
                assert P.dct_raw(img.vp(), w, h, P.NIMG, a.vp()) == 0
                outs.append(("jpegr_dct_raw_device", a, e.raw, tiles * 128))

                a = P.Arena(P.NIMG * npx * 4, off)
                assert P.reconstruct(coef.vp(), img.vp(), w, h, P.NIMG, a.vp()) == 0
                outs.append(("jpegr_reconstruct_device(d_rgba_orig)", a, e.rec_orig, npx * 4))

                a = P.Arena(P.NIMG * npx * 4, off)
                assert P.reconstruct(coef.vp(), None, w, h, P.NIMG, a.vp()) == 0
                outs.append(("jpegr_reconstruct_device(NULL)", a, e.rec_all, npx * 4))

                torch.cuda.synchronize()
                for call, arena, want, per in outs:
                    bad = arena.problem(want, per)
                    assert bad is None, _fail(w, h, call, fill, bad)
