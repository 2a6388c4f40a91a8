"""jpr_tensor_model.py (the numpy restatement of jpegr_crop_tensor_device's
values and placement) against torch on the CPU: the reference of a value is
torch.from_numpy(u8).float().mul(s).add(b).to(dtype), compared as bit patterns;
the reference of the placement is permute / flip.  No GPU."""
import numpy as np
import pytest
import torch

import jpr_tensor_model as T

TORCH = {T.U8: torch.uint8, T.F32: torch.float32, T.F16: torch.float16, T.BF16: torch.bfloat16}
INT = {T.U8: torch.uint8, T.F32: torch.int32, T.F16: torch.int16, T.BF16: torch.int16}


def bits_of(t, dtype):
    """A torch tensor of TORCH[dtype] as numpy bit patterns."""
    return t.contiguous().view(INT[dtype]).numpy().view(T.BITS[dtype])


ALL_BYTES = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)       # [256, 3]


@pytest.mark.parametrize("name", sorted(T.norm_sets()))
@pytest.mark.parametrize("dtype", [T.F32, T.F16, T.BF16])
def test_values_against_torch(name, dtype):
    s, b = T.norm_sets()[name]
    assert s.dtype == np.float32 and b.dtype == np.float32
    want = torch.from_numpy(ALL_BYTES).float().mul(torch.from_numpy(s)).add(torch.from_numpy(b))
    want = want.to(TORCH[dtype])
    got = T.elements(ALL_BYTES, dtype, s, b)
    assert got.dtype == T.BITS[dtype] and np.array_equal(got, bits_of(want, dtype))


def test_u8_is_the_byte_whatever_scale_and_bias():
    s, b = T.norm_sets()["negative"]
    assert np.array_equal(T.elements(ALL_BYTES, T.U8, s, b), ALL_BYTES)


def test_the_sets_are_what_they_are_meant_to_be():
    sets = T.norm_sets()
    s, b = sets["imagenet"]
    assert s[0] == np.float32(1.0 / (255.0 * 0.229)) and b[2] == np.float32(-0.406 / 0.225)
    s, b = sets["unit"]
    assert (s == np.float32(1.0 / 255.0)).all() and (b == 0).all() and not np.signbit(b).any()
    # 2^-20: v 2^-20 is below f16's smallest normal, 2^-14, for v < 64, and a multiple of its
    # subnormal step 2^-24: bytes 1 .. 63 give nonzero subnormals, the others normal numbers
    h = T.elements(ALL_BYTES, T.F16, *sets["tiny"])[:, 0]
    sub = ((h & 0x7C00) == 0) & ((h & 0x03FF) != 0)
    assert sub[1:64].all() and not sub[64:].any() and h[0] == 0
    assert (sets["negative"][0] < 0).all()


def test_none_is_one_and_zero():
    one, zero = np.ones(3, np.float32), np.zeros(3, np.float32)
    for dtype in (T.F32, T.F16, T.BF16):
        assert np.array_equal(T.elements(ALL_BYTES, dtype), T.elements(ALL_BYTES, dtype, one, zero))


def test_bf16_ties_round_to_even():
    f = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF], np.uint32).view(np.float32)
    assert T.bf16_bits(f).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F80]
    assert np.array_equal(T.bf16_bits(f), bits_of(torch.from_numpy(f).to(torch.bfloat16), T.BF16))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("layout", [T.CHW, T.HWC])
def test_placement_and_flip(layout, flip):
    """A 3 x 5 x 7 crop (channels, rows, columns) out of a larger image."""
    rng = np.random.default_rng(7)
    full = rng.integers(0, 256, size=(2, 9, 12, 4), dtype=np.uint8)
    rect = (1, 3, 2, 7, 5, 0)
    got = T.crop_elements(full, rect, T.F32, layout, flip)
    x = torch.from_numpy(full[1, 2:7, 3:10, :3].copy())                 # [5, 7, 3]
    if layout == T.CHW:
        want = x.permute(2, 0, 1)                                       # [3, 5, 7]
        want = want.flip(2) if flip else want
        assert want.shape == (3, 5, 7)
    else:
        want = x.flip(1) if flip else x
    assert np.array_equal(got, bits_of(want.float(), T.F32).reshape(-1))
    assert np.array_equal(T.crop_elements(full, rect, T.U8, layout, flip), want.contiguous().numpy().reshape(-1))


def test_capacity_counts_elements_and_no_dst_is_misaligned():
    args = (40, 24, 3, 16, 9)
    assert T.classify((0, 0, 0, 4, 2, 1), *args, out_cap=25) == T.GOOD          # 1 + 24 = 25
    assert T.classify((0, 0, 0, 4, 2, 2), *args, out_cap=25) == T.BAD
    assert T.classify((0, 0, 0, 4, 2, 3), *args, out_cap=1 << 20) == T.GOOD     # dst % 4 != 0
    assert T.classify((0, 0, 0, 4, 2, (1 << 64) - 8), *args, out_cap=1 << 20) == T.BAD
    assert T.classify((9, 1 << 63, 0, 0, 2, 3), *args, out_cap=0) == T.EMPTY
    assert T.classify((0, 0, 0, 4, 2, 0), *args, out_cap=100, header_ok=False) == T.BAD
    assert T.classify((3, 0, 0, 4, 2, 0), *args, out_cap=100) == T.BAD
    assert T.classify((0, 37, 0, 4, 2, 0), *args, out_cap=100) == T.BAD


def test_expected_writes_good_rectangles_only():
    rng = np.random.default_rng(8)
    full = rng.integers(0, 256, size=(1, 8, 8, 4), dtype=np.uint8)
    rects = [(0, 1, 1, 2, 2, 1), (0, 0, 0, 9, 1, 20), (0, 4, 4, 1, 1, 14)]
    classes = T.verdicts(rects, 8, 8, 1, 8, 8, 40)
    assert classes == [T.GOOD, T.BAD, T.GOOD]
    out, loose = T.expected(full, rects, classes, classes, np.full(40, 0x5A5A, np.uint16), T.BF16,
                            T.HWC, flips=[1, 0, 0])
    assert not loose.any() and out.dtype == np.uint16
    assert (out[:1] == 0x5A5A).all() and (out[13:14] == 0x5A5A).all() and (out[17:] == 0x5A5A).all()
    assert np.array_equal(out[1:13], T.crop_elements(full, rects[0], T.BF16, T.HWC, True))
    assert np.array_equal(out[14:17], T.elements(full[0, 4, 4, :3], T.BF16))
