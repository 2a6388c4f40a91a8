"""GPU reconstruction (jpegr_reconstruct_device) == the oracle's restatement
of the reference's decode side, which is itself pinned to the reference's
whole JPEG.c pipeline (tests/test_oracle.py)."""
import numpy as np
import pytest

import oracle_api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,seed", [(8, 8, 1), (64, 48, 2), (38, 21, 3), (37, 21, 4), (1, 1, 5),
                                      (264, 17, 6), (1200, 630, 7), (3840, 2160, 8)])
def test_reconstruct_matches_oracle(gpu, oracle, w, h, seed):
    import torch
    from lz4jpeg import jpeg
    img = oracle.rand_image(w, h, seed=seed)
    d = torch.from_numpy(np.ascontiguousarray(img)).to(gpu)
    coef = jpeg.encode_device(d, w, h)
    rec = jpeg.reconstruct_device(coef, w, h, d_orig=d).cpu().numpy().reshape(h, w, 4)
    assert np.array_equal(rec, oracle_api.reconstruct(oracle, img))


def test_reconstruct_without_orig_decodes_every_tile(gpu, oracle):
    """d_orig = NULL: trailing tiles are decoded from their coefficients, so
    the result equals decoding every tile (differs from the reference only in
    the ceil(W*H/64) quirk tiles)."""
    import torch
    from lz4jpeg import jpeg
    w, h = 40, 16                     # 10 tiles, ceil(640/64) = 10: no quirk tile
    img = oracle.rand_image(w, h, seed=9)
    d = torch.from_numpy(np.ascontiguousarray(img)).to(gpu)
    coef = jpeg.encode_device(d, w, h)
    a = jpeg.reconstruct_device(coef, w, h).cpu().numpy()
    b = jpeg.reconstruct_device(coef, w, h, d_orig=d).cpu().numpy()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("w,h,nimg", [(1, 1, 1), (37, 21, 1), (264, 17, 1), (13, 11, 3)])
def test_reconstruct_without_orig_matches_oracle_tiles(gpu, oracle, w, h, nimg):
    """d_orig = NULL against the oracle, not against another kernel: every tile
    through jo_decode_tile, pixels by the reference's fp64 colour expressions
    (oracle_api.decode_every_tile).  37 x 21 has 15 tiles of which the reference
    transforms 13, and a width that is no multiple of 4 (dword stores); 264 x 17
    has 33 tiles a row, so a second strip of one tile; 13 x 11 is a batch."""
    import torch
    from lz4jpeg import jpeg
    imgs = [oracle.rand_image(w, h, seed=40 + i) for i in range(nimg)]
    d = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).to(gpu)
    coef = jpeg.encode_device(d, w, h, nimg=nimg)
    got = jpeg.reconstruct_device(coef, w, h, nimg=nimg).cpu().numpy().reshape(nimg, h, w, 4)
    per_image = coef.cpu().numpy().reshape(nimg, -1)
    for i in range(nimg):
        want = oracle_api.decode_every_tile(oracle, per_image[i], w, h)
        assert np.array_equal(got[i], want), i
        if (w, h) == (37, 21):      # the expectation reaches the two quirk tiles
            assert not np.array_equal(want, oracle_api.reconstruct(oracle, imgs[i]))


@pytest.mark.parametrize("name", ["pm3", "pm40", "int16", "peak+", "peak-", "flat"])
def test_reconstruct_coefficients_the_encoder_never_makes(gpu, oracle, name):
    """The stream decoders deliver any int16: d_orig = NULL on 264 x 16 x 2 (a
    second strip of one tile) of seeded +-3, +-40 and uniform int16
    coefficients, of tiles that are zero but for 32767 or -32768 at each of the
    128 positions, and of tiles that are all 32767 or all -32768
    (jpeg_pixel_lib.offgrid_classes), against oracle_api.decode_every_tile, the
    output in a guard arena.  All are defined inputs for the reference (samples
    below 2^26).  The two small classes must leave a quarter of the R, G, B bytes
    off the clamps, or they would say nothing about rounding."""
    import torch
    import jpeg_pixel_lib as P
    coef = P.offgrid_classes()[name]
    want = P.offgrid_expect(oracle, coef)
    if name in P.ROUNDING_CLASSES:
        assert P.in_range_share(want) >= 0.25, P.in_range_share(want)
    w, h = P.OFFGRID_W, P.OFFGRID_H
    for fill in P.INPUT_FILLS:
        out = P.run_reconstruct(coef, w, h, P.NIMG, in_fill=fill)
        torch.cuda.synchronize()
        bad = out.problem(want, w * h * 4)
        assert bad is None, f"{name}, input fill 0x{fill:02x}: {bad}"


def test_reconstruct_batch(gpu, oracle):
    import torch
    from lz4jpeg import jpeg
    w, h, n = 48, 40, 3
    imgs = [oracle.rand_image(w, h, seed=20 + i) for i in range(n)]
    d = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).to(gpu)
    coef = jpeg.encode_device(d, w, h, nimg=n)
    rec = jpeg.reconstruct_device(coef, w, h, nimg=n, d_orig=d).cpu().numpy().reshape(n, h, w, 4)
    for i in range(n):
        assert np.array_equal(rec[i], oracle_api.reconstruct(oracle, imgs[i]))
