"""The JPEG kernels' arithmetic shortcuts against the oracle on the inputs
where a shortcut and the reference's formula can part (builders and their
reasons: tests/jpeg_exact_inputs.py; what the inputs reach is counted on the
CPU by tests/test_jpeg_exact_inputs.py):

  convert_pixel's integer colour conversion and planes_kernel, on every RGB
  triple; quantize_row's one-multiply fast path, on quotients a few ulp from
  an integer; round_clamp_u8, on samples a few ulp from k + 0.5 and past both
  clamps.
"""
import ctypes

import numpy as np
import pytest

import jpeg_exact_inputs as X

pytestmark = pytest.mark.gpu

PLANES = ("Y", "Cr", "Cb")


def _triples(k, flat_idx):
    i = k * X.SLICE_PX + np.asarray(flat_idx, dtype=np.int64)
    return [(int(t & 255), int((t >> 8) & 255), int((t >> 16) & 255)) for t in i]


def _assert_planes_equal(k, got, want):
    """got / want: three (1024, 1024) planes indexed by the slice's triple."""
    for name, g, e in zip(PLANES, got, want):
        bad = np.flatnonzero(g.ravel() != e.ravel())
        if bad.size:
            first = bad[:8]
            rows = [f"RGB{t}: got {int(g.ravel()[i])}, oracle {int(e.ravel()[i])}"
                    for t, i in zip(_triples(k, first), first)]
            pytest.fail(f"{name}: {bad.size} of 2^20 triples differ in slice {k}; "
                        + "; ".join(rows))


@pytest.mark.parametrize("k", range(X.SLICES))
def test_planes_device_every_triple(gpu, oracle, k):
    """jpegr_planes_device (the plain fp64 expression on the GPU) == jo_planes,
    byte for byte, on the 2^20 triples k 2^20 ... (k + 1) 2^20 - 1."""
    import torch
    from lz4jpeg import _lib
    d = torch.from_numpy(X.slice_image(k)).to(gpu)
    out = torch.empty(3, X.SLICE_PX, dtype=torch.uint8, device=gpu)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().jpegr_planes_device(
        ctypes.c_void_p(d.data_ptr()), 1024, 1024, ctypes.c_void_p(out[0].data_ptr()),
        ctypes.c_void_p(out[1].data_ptr()), ctypes.c_void_p(out[2].data_ptr()), s)
    assert rc == 0
    got = out.cpu().numpy().reshape(3, 1024, 1024)
    _assert_planes_equal(k, got, X.slice_planes(oracle, k))


@pytest.mark.parametrize("k", range(X.SLICES))
def test_encoder_colour_every_triple(gpu, oracle, k):
    """The fused encoder's phase 1 (convert_pixel) on every triple of the
    slice, seen through the raw fp64 DCT: the integer samples are recovered by
    the inverse transform in numpy (unambiguous: the recovered values must lie
    within 1e-6 of integers; the true error is near 1e-12) and must equal
    jo_planes.  Each triple fills an even and the next odd column, so luma
    converts it twice and the odd-column chroma once.  The DCT's own
    bit-exactness is test_raw_dct_bit_exact's subject, not this test's."""
    import torch
    from lz4jpeg import jpeg
    w, h = 2048, 1024
    d = torch.from_numpy(X.doubled_slice_image(k)).to(gpu)
    raw = jpeg.dct_raw_device(d, w, h).cpu().numpy()
    fy, fr, fb = X.samples_from_raw(raw, w, h)
    for name, f in zip(PLANES, (fy, fr, fb)):
        err = np.abs(f - np.rint(f)).max()
        assert err < 1e-6, (name, err)
    y = np.rint(fy).astype(np.int64) + 128
    cr = np.rint(fr).astype(np.int64) + 128
    cb = np.rint(fb).astype(np.int64) + 128
    want = X.slice_planes(oracle, k)
    _assert_planes_equal(k, (y[:, 0::2], cr, cb), want)
    _assert_planes_equal(k, (y[:, 1::2], cr, cb), want)


def _assert_coef_equal(got, want, what):
    got, want = got.reshape(-1, 128), want.reshape(-1, 128)
    bad = np.argwhere(got != want)
    if bad.size:
        rows = []
        for t, z in bad[:8]:
            plane, idx = (("Y", z) if z < 64 else ("Cr", z - 64) if z < 96 else ("Cb", z - 96))
            rows.append(f"tile {t} {plane}[zigzag {idx}]: got {got[t, z]}, oracle {want[t, z]}")
        pytest.fail(f"{what}: {len(bad)} coefficients differ; " + "; ".join(rows))


def test_quantiser_near_integer_quotients(gpu, oracle):
    """encode_device == the oracle, element for element, on the image whose
    luma quotients coef / T lie a few ulp on either side of nonzero integers
    (where the fast path's truncation could differ from the reference's) and
    whose other coefficients are rounding residues that must give 0.  Chroma
    gets only the near-zero residues from this image: no 8 x 4 coefficient of
    these tiles is near a nonzero multiple of its step."""
    import torch
    from lz4jpeg import jpeg
    img = X.quant_tie_image(oracle)
    h, w = img.shape[:2]
    want = oracle.jpeg_encode(img)
    d = torch.from_numpy(np.array(img)).to(gpu)           # the cached image is read-only
    _assert_coef_equal(jpeg.encode_device(d, w, h).cpu().numpy(), want, "single image")
    # as a batch of two, the second copy upside down: the amplitudes then run
    # the other way through the strips, so the wave-uniform fallback branch
    # meets the guarded lanes in other waves and other mixes
    flip = np.ascontiguousarray(img[::-1])
    d2 = torch.from_numpy(np.stack([img, flip])).to(gpu)
    got = jpeg.encode_device(d2, w, h, nimg=2).cpu().numpy().reshape(2, -1)
    _assert_coef_equal(got[0], want, "batch image 0")
    _assert_coef_equal(got[1], oracle.jpeg_encode(flip), "batch image 1 (flipped)")


def test_reconstruct_ties_and_clamps(gpu, oracle):
    """reconstruct_device == jo_decode_tile + the reference's RGB assembly,
    byte for byte, on synthetic coefficients whose every luma sample is a few
    ulp from k + 0.5 (round() is half away from zero; round_clamp_u8 tests the
    fraction against 0.5), with samples below 0 and above 255.5 in all three
    planes and R, G, B past both ends of the final clamp.  Width and height
    are multiples of 8, so d_orig=None decodes every tile.  Chroma samples are
    never near a tie (irrational 8 x 4 basis values): its rounding is covered
    through the shared round_clamp_u8 only."""
    import torch
    from lz4jpeg import jpeg
    coef, w, h = X.recon_tie_coef()
    want = X.recon_expected(oracle)
    d = torch.from_numpy(np.array(coef)).to(gpu)          # the cached array is read-only
    got = jpeg.reconstruct_device(d, w, h).cpu().numpy().reshape(h, w, 4)
    bad = np.argwhere((got != want).any(axis=2))
    if bad.size:
        rows = [f"pixel ({r}, {c}) tile {r // 8 * (w // 8) + c // 8}: got {got[r, c].tolist()}, "
                f"oracle {want[r, c].tolist()}" for r, c in bad[:8]]
        pytest.fail(f"{len(bad)} of {w * h} pixels differ; " + "; ".join(rows))
