"""The inputs of tests/test_gpu_jpeg_exact.py reach the cases they are built
for.  Oracle only (no GPU): each count below says how many inputs tell a right
kernel from one whose shortcut is subtly wrong, so that a later change to a
builder cannot quietly empty the GPU tests."""
import numpy as np

import jpeg_exact_inputs as X
import oracle_api


def test_colour_fallback_is_needed_exactly_on_multiples_of_1000(oracle):
    """Over all 2^24 RGB triples the reference's fp64 truncation equals
    floor(N / 1000) wherever N is not a multiple of 1000, and differs from it
    at exactly 3464 (Y), 102 (Cr) and 35 (Cb) of the multiples: the only pixels
    at which convert_pixel's fp64 fallback decides the result.  The Cr / Cb
    quotients stay within 16..239, so its clamp cannot fire there."""
    differ = np.zeros(3, np.int64)
    multiples = np.zeros(3, np.int64)
    lo = np.full(3, 1 << 30, np.int64)
    hi = np.zeros(3, np.int64)
    for k in range(X.SLICES):
        ref = X.slice_planes(oracle, k)
        for j, n in enumerate(X.colour_numerators(k)):
            q = n // 1000
            d = ref[j].ravel() != q
            m = n % 1000 == 0
            assert not np.any(d & ~m), (k, "Y Cr Cb".split()[j])
            differ[j] += d.sum()
            multiples[j] += m.sum()
            lo[j], hi[j] = min(lo[j], q.min()), max(hi[j], q.max())
    assert differ.tolist() == [3464, 102, 35]
    assert multiples.tolist() == [16774, 16784, 16816]
    assert (lo.tolist(), hi.tolist()) == ([0, 16, 16], [255, 239, 239])


def test_div1000_multiply_high_is_exact():
    """convert_pixel's quotient (N * ceil(2^32 / 1000)) >> 32 is N // 1000 for
    every N it can see: the largest numerator is 255000 (Y) or 239945 (chroma)."""
    n = np.arange(0, 255001, dtype=np.uint64)
    assert np.array_equal((n * np.uint64(4294968)) >> np.uint64(32), n // np.uint64(1000))


def test_y_lookup_reaches_every_luma(oracle):
    lut = X.y_to_rgb(oracle)
    img = np.full((1, 256, 4), 255, np.uint8)
    img[0, :, :3] = lut
    assert np.array_equal(X.planes(oracle, img)[0].ravel(), np.arange(256))


def test_quantiser_image_has_near_integer_quotients_on_both_sides(oracle):
    """Luma: nonzero quotients coef / T within quantize_row's 2^-30 band of an
    integer, at least 50 just inside it (truncation and nearest differ) and 50
    just outside; all planes: at least 10,000 nonzero residues below 2^-30 that
    must truncate to 0.  Chroma has no near-integer quotient at all (the 8 x 4
    transform makes every such coefficient irrational): for chroma this image
    covers only the near-zero residues."""
    q = X.quotients(oracle, X.quant_tie_image(oracle))
    n = np.rint(q)
    near = (np.abs(q - n) < X.GUARD) & (n != 0)
    luma = np.zeros(128, bool)
    luma[:64] = True
    inside = near & luma & (np.abs(q) < np.abs(n))
    outside = near & luma & (np.abs(q) > np.abs(n))
    tiny = (q != 0) & (np.abs(q) < X.GUARD)
    print("luma near-integer: inside", inside.sum(), "outside", outside.sum(), "exact",
          (near & luma & (q == n)).sum(), "; chroma near-integer", (near & ~luma).sum(),
          "; tiny residues Y/Cr/Cb", tiny[:, :64].sum(), tiny[:, 64:96].sum(), tiny[:, 96:].sum())
    assert inside.sum() >= 50
    assert outside.sum() >= 50
    assert tiny.sum() >= 10000
    # the guarded quotients are not all of one coefficient: every pattern contributes
    for u, v in X.PATTERNS:
        assert (inside | outside)[:, u * 8 + v].any(), (u, v)


def test_quantiser_image_truncation_differs_from_nearest(oracle):
    """The tiles just inside their integer are where a quantiser that rounded
    (or that trusted a product a few ulp off) gives another int16 than the
    reference: the oracle's coefficient there is the integer below."""
    img = X.quant_tie_image(oracle)
    q = X.quotients(oracle, img)[:, :64]
    n = np.rint(q)
    inside = (np.abs(q - n) < X.GUARD) & (n != 0) & (np.abs(q) < np.abs(n))
    coef = oracle.jpeg_encode(img).reshape(-1, 128)[:, :64]
    nat = np.empty_like(coef)
    nat[:, X.ZZ8] = coef
    assert np.array_equal(nat[inside], (n - np.sign(n))[inside].astype(np.int16))


def test_quantiser_image_has_quotients_the_fallback_decides(oracle):
    """quantize_row's fast product RN(s K) and the reference's RN(aa s) / T,
    both restated in numpy from the oracle's samples (the restatement equals
    the oracle's raw DCT bit for bit), truncate differently at 20 or more luma
    coefficients of the image: there a kernel without the fallback is wrong.
    Every one lies inside the kernel's 2^-30 band.  In each the fast product
    is exactly an integer and the reference's quotient just below it, which is
    why a band of width zero (exact integers only) also passes the GPU test."""
    r, ref = X.luma_fast_and_reference_quotients(oracle, X.quant_tie_image(oracle))
    decided = np.trunc(r) != np.trunc(ref)
    print("fallback decides", decided.sum(), "; of these r exactly integer",
          (decided & (r == np.rint(r))).sum())
    assert decided.sum() >= 20
    assert np.all((r == np.rint(r))[decided])
    assert np.all(np.abs(r - np.rint(r))[decided] <= X.GUARD)


def test_reconstruction_tiles_sit_on_ties_and_past_both_clamps(oracle):
    """Pre-rounding luma sums of the synthetic coefficients (plain numpy; the
    1e-9 tolerance decides, not bit-exactness): at least 1000 within 1e-9 of
    k + 0.5 on each side, at least 100 below 0 and 100 above 255.5.  Chroma
    samples reach both clamps but never a tie; the assembled R, G and B each
    pass both ends of the final clamp."""
    coef, w, h = X.recon_tie_coef()
    assert w % 8 == 0 and h % 8 == 0 and coef.shape == (w // 8 * (h // 8), 128)
    y, cr, cb = X.recon_presums(coef)
    off = y - np.floor(y) - 0.5
    tie = np.abs(off) < 1e-9
    visible = (y > 0) & (y < 255)             # the rounding is not hidden by the clamp
    below, above = tie & visible & (off < 0), tie & visible & (off >= 0)
    print("luma ties below", below.sum(), "at or above", above.sum(), "; below 0", (y < 0).sum(),
          "; above 255.5", (y > 255.5).sum())
    assert tie.all()
    assert below.sum() >= 1000 and above.sum() >= 1000
    assert (y < 0).sum() >= 100 and (y > 255.5).sum() >= 100
    for c in (cr, cb):
        assert (c < 0).sum() >= 100 and (c > 255.5).sum() >= 100
        assert np.abs(c - np.floor(c) - 0.5).min() > 1e-6
    rgb = X.recon_unclamped(oracle)
    for j in range(3):
        assert (rgb[..., j] < 0).sum() >= 100 and (rgb[..., j] > 255).sum() >= 100


def test_numpy_assembly_equals_the_oracle_reconstruction(oracle):
    """The numpy restatement of the RGB assembly, fed the oracle's own
    coefficients of a random image, gives jo_reconstruct_image's pixels."""
    w, h = 64, 24
    img = oracle.rand_image(w, h, seed=31)
    rgb = X.assemble_unclamped(oracle, oracle.jpeg_encode(img), w, h)
    assert np.array_equal(X.clamp_rgba(rgb), oracle_api.reconstruct(oracle, img))


def test_samples_recovered_from_the_oracle_raw_dct(oracle):
    """samples_from_raw inverts the oracle's raw DCT to the planes' samples,
    far inside the 1e-6 that the GPU test allows before rounding."""
    w, h = 64, 24
    img = oracle.rand_image(w, h, seed=32)
    y, cr, cb = X.planes(oracle, img)
    got = X.samples_from_raw(oracle.jpeg_dct_raw(img), w, h)
    for f, want in zip(got, (y, cr[:, 1::2], cb[:, 1::2])):
        assert np.abs(f - np.rint(f)).max() < 1e-9
        assert np.array_equal(np.rint(f).astype(int) + 128, want)
