"""jpr_thumb_model.py against the oracle alone (CPU only): a tile with only DC
terms reconstructs to uniform planes, so "the tile's colour" is well defined and
sample 0 is it; and the model's DC rule is zz[0] of the oracle's entropy
decode.  These pin the definition that test_gpu_jpeg_thumb.py rests on; they
pass without the thumbnail kernel by design."""
import json
import os

import numpy as np
import pytest

import golden_inputs
import jpr_gpu_lib
import jpr_thumb_model as M
import oracle_api

VECS = json.load(open(os.path.join(golden_inputs.GOLDEN, "entropy.json")))


def test_dc_only_planes_are_uniform(oracle):
    """Every int16 DC, on luma and on chroma: every sample of the plane is
    sample 0 (the other products of the IDCT's sum are +-0.0 and the u = v = 0
    cosines are 1.0).  sample_luts sweeps them and asserts it per DC; a few
    mixed triples here."""
    M.sample_luts(oracle)
    for y, cr, cb in ((-300, 77, -5), (32767, -32768, 1), (1, 0, -1)):
        for plane in M.planes_of(oracle, y, cr, cb):
            assert (plane == plane[0, 0]).all()


def test_sample_luts(oracle):
    """The luts: monotone in the DC, both clamps reached, 128 at 0; luma moves
    a level per DC step (alpha 1/8 x step 8), chroma sqrt(2) 17 / 8 ~ 3 levels."""
    luma, chroma = M.sample_luts(oracle)
    for lut in (luma, chroma):
        assert (np.diff(lut.astype(int)) >= 0).all()
        assert lut[0] == 0 and lut[-1] == 255 and lut[32768] == 128
    assert np.array_equal(luma[32768 - 128:32768 + 128], np.arange(256))
    assert set(np.diff(chroma[32768 - 42:32768 + 42].astype(int)).tolist()) <= {3, 4}
    assert chroma[32768 - 43] == 0 and chroma[32768 + 43] == 255      # 128 -+ 129.2
    assert M.zero_pixel(oracle).tolist() == [128, 128, 128, 255]


def test_dc_only_keeps_three_terms():
    coef = np.arange(256, dtype=np.int16).reshape(2, 128) + 1
    got = M.dc_only(coef)
    assert np.count_nonzero(got) == 6 and np.array_equal(got[:, M.DC_AT], coef[:, M.DC_AT])


@pytest.mark.parametrize("v", VECS, ids=lambda v: v["name"])
def test_dc_rule_on_reference_vectors(oracle, v):
    e = oracle_api.entropy(oracle, v["zz"])
    assert e["rc"] == 0
    assert M.dc_of_rle(e["rle"]) == oracle_api.entropy_decode(oracle, e, len(v["zz"]))[0] == v["zz"][0]


def test_dc_rule_on_crafted_streams(oracle):
    """The crafted decoder batch: its RLE lists against the ints they stand
    for, and through the oracle's own decode.  Among them are lists whose first
    count is 0 or negative, one-code streams and a count with no value."""
    import entropy_inputs as E
    (_, _, _), want, _ = jpr_gpu_lib.crafted(oracle)
    streams = E.crafted_batch(oracle).streams
    zero = negative = one = 0
    for t, row in enumerate(streams):
        for c, s in enumerate(row):
            dc = M.dc_of_rle(s.syms)
            assert dc == int(want[t, M.DC_AT[c]]), (t, c)
            zero += len(s.syms) >= 2 and s.syms[0] == 0
            negative += len(s.syms) >= 2 and s.syms[0] < 0
            one += len(s.table) == 1
            e = {"table": [(v, L, code) for (v, L), code in zip(s.table, s.codes)], "rle": s.syms,
                 "nbits": s.nbits, "bits": s.bits[:(s.nbits + 7) // 8]}
            assert oracle_api.entropy_decode(oracle, e, E.N[c])[0] == dc, (t, c)
    assert zero > 0 and negative > 0 and one > 0
    assert M.dc_of_rle([]) == 0 and M.dc_of_rle([5]) == 0 and M.dc_of_rle([0, 9, 2]) == 0
    assert M.dc_of_rle([0, 9, -3, 8, 1, -7, 4, 4]) == -7


def test_result_words():
    assert M.result_words(100, 100, True) == [100, M.OK]
    assert M.result_words(100, 100, True, {41, 7}) == [100, 8]
    assert M.result_words(100, 99, True, {41}) == [100, 0]
    assert M.result_words(100, 100, False) == [100, 0]
