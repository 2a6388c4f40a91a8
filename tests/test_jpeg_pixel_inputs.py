"""The coefficient classes that tests/test_gpu_reconstruct.py feeds
jpegr_reconstruct_device (jpeg_pixel_lib.offgrid_classes), against the oracle
alone (no GPU): their shapes and extremes, and that the two small-magnitude
classes leave at least a quarter of the R, G, B bytes off the clamps --
otherwise they would say nothing about rounding."""
import numpy as np
import pytest

import jpeg_pixel_lib as P


def test_classes_are_what_they_claim():
    cls = P.offgrid_classes()
    assert set(cls) == {"pm3", "pm40", "int16", "peak+", "peak-", "flat"}
    assert P.OFFGRID_TILES == 132 and P.tiles_of(P.OFFGRID_W, P.OFFGRID_H) == 33 * 2
    for name, c in cls.items():
        assert c.shape == (132, 128) and c.dtype == np.int16, name
    assert (cls["pm3"].min(), cls["pm3"].max()) == (-3, 3)
    assert (cls["pm40"].min(), cls["pm40"].max()) == (-40, 40)
    assert cls["int16"].min() < -32700 and cls["int16"].max() > 32700      # 16,896 draws of 65,536
    for name, v in (("peak+", 32767), ("peak-", -32768)):
        c = cls[name]
        assert np.count_nonzero(c) == 128 and all(c[p, p] == v for p in range(128))
    assert (cls["flat"][0::2] == 32767).all() and (cls["flat"][1::2] == -32768).all()
    again = P.offgrid_classes()
    assert all(np.array_equal(cls[k], again[k]) for k in cls)              # seeded


@pytest.mark.parametrize("name", P.ROUNDING_CLASSES)
def test_small_classes_stay_off_the_clamps(oracle, name):
    want = P.offgrid_expect(oracle, P.offgrid_classes()[name])
    assert want.shape == (P.NIMG, P.OFFGRID_H, P.OFFGRID_W, 4)
    assert P.in_range_share(want) >= 0.25, P.in_range_share(want)
    for ch in range(3):                                   # each of R, G, B on its own
        assert P.in_range_share(want[..., ch:ch + 1]) >= 0.25, ch
