"""jpr_resize_model.py (the numpy restatement of jpegr_crop_resize_device's
values) on the CPU: anchored to torch's interpolate, which it follows up to
roundings; equal sizes are jpr_tensor_model's elements bit for bit; the windows'
properties that include/jpegr.h states; the uint8 rounding.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import jpr_resize_model as R
import jpr_tensor_model as T

# (source w, source h) -> (out_w, out_h)
SHAPES = [((13, 11), (5, 7)), ((9, 37), (16, 16)), ((317, 200), (32, 32)), ((16, 16), (47, 33)),
          ((250, 3), (7, 7)), ((400, 500), (64, 64)), ((64, 1080), (8, 8)), ((9, 9), (1, 1)),
          ((1, 1), (4, 4)), ((8, 8), (8, 8)), ((224, 224), (224, 224))]


@pytest.mark.parametrize("filt", [R.BILINEAR, R.TRIANGLE], ids=["bilinear", "triangle"])
@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{a}x{b}-{c}x{d}" for (a, b), (c, d) in SHAPES])
def test_the_model_is_torchs_bilinear(src, dst, filt):
    """Random bytes against interpolate(mode="bilinear", align_corners=False,
    antialias=<filter>): |difference| <= 1 / 64 on the 0 .. 255 scale.  The
    worst seen is 0.0022 (250 -> 7 by BILINEAR, where torch computes the source
    index in float32), a seventh of the bound; one misplaced tap gives about 1.  This anchors the
    definition; the exactness checks are the GPU tests'."""
    (w, h), (ow, oh) = src, dst
    px = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = R.resample(px, ow, oh, filt)
    assert got.shape == (oh, ow, 3) and got.dtype == np.float32
    x = torch.from_numpy(px).permute(2, 0, 1).unsqueeze(0).float()
    ref = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False,
                        antialias=filt == R.TRIANGLE)[0].permute(1, 2, 0).numpy()
    worst = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"{w}x{h} -> {ow}x{oh} filter {filt}: largest |difference| {worst:.6f}")
    assert worst <= 1.0 / 64.0
    if (w, h) == (ow, oh):
        assert worst == 0.0


@pytest.mark.parametrize("filt", [R.BILINEAR, R.TRIANGLE])
def test_equal_sizes_are_the_tensor_models_elements(filt):
    """w == out_w and h == out_h: every weight is 1.0 or 0.0, and the elements
    are jpr_tensor_model.crop_elements' for all dtypes, layouts and flips."""
    full = np.random.default_rng(7).integers(0, 256, (2, 24, 40, 4), dtype=np.uint8)
    scale, bias = T.norm_sets()["imagenet"]
    for rect in [(0, 3, 5, 13, 11, 0), (1, 0, 0, 40, 24, 0), (1, 39, 23, 1, 1, 0)]:
        w, h = rect[3], rect[4]
        for lo, wt, _ in R.axis_taps(w, w, filt) + R.axis_taps(h, h, filt):
            assert set(wt.tolist()) <= {0.0, 1.0} and wt.sum() == 1.0
        for dtype in (T.U8, T.F32, T.F16, T.BF16):
            for layout in (T.CHW, T.HWC):
                for flip in (False, True):
                    got = R.crop_elements(full, rect, w, h, filt, dtype, layout, flip, scale, bias)
                    want = T.crop_elements(full, rect, dtype, layout, flip, scale, bias)
                    assert got.dtype == want.dtype and np.array_equal(got, want), (rect, dtype, layout, flip)


def test_windows_are_never_empty():
    """hi > lo and tot >= 0.5 for all n, m in 1 .. 64, both filters; the windows
    stay inside the axis and their first pixels rise with the output index; a
    window has at most 2 ceil(n / m) + 2 taps (the weight table's pitch)."""
    for filt in (R.BILINEAR, R.TRIANGLE):
        for n in range(1, 65):
            for m in range(1, 65):
                taps = R.axis_taps(n, m, filt)
                assert len(taps) == m
                los = [lo for lo, _, _ in taps]
                assert los == sorted(los)
                for lo, wt, tot in taps:
                    assert wt.size > 0 and tot >= 0.5, (n, m, filt)
                    assert 0 <= lo and lo + wt.size <= n
                    assert wt.size <= 2 * -(-n // m) + 2
                    assert abs(float(wt.astype(np.float64).sum()) - 1.0) < 1e-6


def test_taps_are_cached_and_read_only():
    a = R.axis_taps(37, 16, R.TRIANGLE)
    assert R.axis_taps(37, 16, R.TRIANGLE) is a
    with pytest.raises(ValueError):
        a[0][1][0] = 0.0


def test_u8_rounds_ties_to_even():
    """Two pixels to one: both weights are 0.5 exactly, so (1, 2) gives 1.5 and
    (2, 3) gives 2.5; both round to 2.  255.5 would clamp: 255 and 255 stay 255."""
    for filt in (R.BILINEAR, R.TRIANGLE):
        (lo, wt, tot), = R.axis_taps(2, 1, filt)
        assert lo == 0 and wt.tolist() == [0.5, 0.5]
    px = np.array([[[1, 2, 255], [2, 3, 255]]], np.uint8)          # [h=1, w=2, 3]
    val = R.resample(px, 1, 1, R.TRIANGLE)
    assert val.reshape(-1).tolist() == [1.5, 2.5, 255.0]
    assert R.elements(val, T.U8).reshape(-1).tolist() == [2, 2, 255]
    assert R.elements(np.array([[0.5, 3.5, 255.4]], np.float32), T.U8).reshape(-1).tolist() == [0, 4, 255]
    assert R.elements(np.array([[-0.2, 255.6, 300.0]], np.float32), T.U8).reshape(-1).tolist() == [0, 255, 255]
    # not rounded to a byte before the normalisation
    assert R.elements(val, T.F32, [2.0] * 3, [0.0] * 3).view(np.float32).reshape(-1).tolist() == [3.0, 5.0, 510.0]


def test_classes():
    ok = (0, 1, 2, 5, 4, 10)
    args = (13, 11, 3, 8, 8, 5, 7)
    assert R.classify(ok, *args, 10 + 105) == R.GOOD
    assert R.classify(ok, *args, 10 + 104) == R.BAD                # one element short
    assert R.classify((0, 1, 2, 0, 4, 10), *args, 1000) == R.BAD   # nothing to resample
    assert R.classify((0, 1, 2, 5, 0, 10), *args, 1000) == R.BAD
    assert R.classify((3, 1, 2, 5, 4, 10), *args, 1000) == R.BAD
    assert R.classify((0, 9, 2, 5, 4, 10), *args, 1000) == R.BAD
    assert R.classify((0, 1, 2, 9, 4, 10), *args, 1000) == R.BAD
    assert R.classify(ok, *args, 1000, header_ok=False) == R.BAD
