"""The JPEG kernel's baked constants equal the reference's libm expressions."""
import math
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "lz4-jpeg_amd", "csrc")
PI = 3.14159265358979323846


def test_tables_header_is_generated_output():
    for args, name in (([], "jpeg_tables.h"), (["dev"], "jpeg_tables_dev.h")):
        gen = subprocess.run([sys.executable, os.path.join(CSRC, "gen_jpeg_tables.py")] + args,
                             capture_output=True, text=True, check=True).stdout
        assert open(os.path.join(CSRC, name)).read() == gen, name


def _table(name, header="jpeg_tables.h"):
    src = open(os.path.join(CSRC, header)).read()
    body = src.split(f"double {name}[")[1].split("};")[0].split("= {", 1)[1]
    return [float.fromhex(x) for x in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", body)]


def _ints(name, header="jpeg_tables.h"):
    src = open(os.path.join(CSRC, header)).read()
    body = src.split(f"int {name}[")[1].split("};")[0].split("= {", 1)[1]
    return [int(v) for v in re.findall(r"-?\d+", re.sub(r"//.*", "", body))]


DEV = "jpeg_tables_dev.h"


def test_device_tables_repeat_the_primary_ones():
    """The __constant__ copies the kernels load hold the primary tables' values."""
    for name in ("C8", "AA88", "AA84"):
        assert _table("d" + name, DEV) == _table(name), name
    assert _ints("dLQ", DEV) == _ints("LUMA_Q")
    assert _ints("dCQ", DEV) == _ints("CHROMA_Q")
    assert (len(_ints("dLQ", DEV)), len(_ints("dCQ", DEV))) == (64, 32)


def test_quantiser_fast_path_constants():
    """K[i] = RN(alpha_u alpha_v * RN(1 / T)): two IEEE double operations."""
    for k, aa, q, n in (("dLK", "AA88", "LUMA_Q", 64), ("dCK", "AA84", "CHROMA_Q", 32)):
        K, AA, Q = _table(k, DEV), _table(aa), _ints(q)
        assert len(K) == len(AA) == len(Q) == n
        for i in range(n):
            assert K[i] == AA[i] * (1.0 / Q[i]), (k, i)


def test_zigzag_byte_offsets():
    assert _ints("dZZ8b", DEV) == [2 * p for p in _ints("ZZ8_POS")]
    assert _ints("dZZ4b", DEV) == [2 * p for p in _ints("ZZ4_POS")]
    assert (len(_ints("dZZ8b", DEV)), len(_ints("dZZ4b", DEV))) == (64, 32)


def test_reconstruction_tables_by_zigzag_position():
    """For every position z of a tile's 128 zigzagged int16 ([Y 64][Cr 32][Cb 32]):
    RZn inverts the zigzag of z's plane, RZq and RZa are the step and the alpha
    product at that natural index."""
    rzn, rzq, rza = _ints("dRZn", DEV), _table("dRZq", DEV), _table("dRZa", DEV)
    assert len(rzn) == len(rzq) == len(rza) == 128
    luma = (_ints("ZZ8_POS"), _ints("LUMA_Q"), _table("AA88"))
    chroma = (_ints("ZZ4_POS"), _ints("CHROMA_Q"), _table("AA84"))
    for z in range(128):
        (pos, q, aa), zp = (luma, z) if z < 64 else (chroma, (z - 64) % 32)
        n = rzn[z]
        assert 0 <= n < len(pos) and pos[n] == zp, z
        assert rzq[z] == float(q[n]) and rza[z] == aa[n], z
    assert sorted(rzn[:64]) == list(range(64))
    assert sorted(rzn[64:96]) == sorted(rzn[96:]) == list(range(32))


def test_cos_values_match_libm_expression():
    c8 = _table("C8")
    for x in range(8):
        for u in range(8):
            assert c8[x * 8 + u] == math.cos((PI * (2 * x + 1) * u) / (2.0 * 8))


def test_survey_spot_values():
    c8 = _table("C8")
    # asymmetric last bits
    assert c8[1 * 8 + 3] == float.fromhex("-0x1.8f8b83c69a608p-3")
    assert c8[0 * 8 + 7] == float.fromhex("0x1.8f8b83c69a60dp-3")
    aa = _table("AA88")
    assert aa[0] == float.fromhex("0x1.0000000000001p-3")  # not 0.125


def test_zigzag_chroma_order():
    src = open(os.path.join(CSRC, "jpeg_tables.h")).read()
    pos = [int(v) for v in src.split("ZZ4_POS[32] = {")[1].split("}")[0].split(",")]
    order = [0] * 32
    for i, k in enumerate(pos):
        order[k] = i
    assert order == [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 16, 13, 10, 7, 11, 14, 17, 20, 24, 21, 18,
                     15, 19, 22, 25, 28, 29, 26, 23, 27, 30, 31]


def test_colour_terms_fp32_equal_fp64():
    """jpeg_recon_kernel's colour terms (assemble_image, JPEG.c:598-600): the
    truncation of the fp32 product fl32(k) * d equals the reference's (int) of
    the fp64 product k * (double)d for every d = Cr - 128 / Cb - 128 in
    -128..127 and each of the four constants, and no product lies within
    0.001 of a nonzero integer (the margin the kernel's comment relies on)."""
    import numpy as np
    d = np.arange(-128, 128)
    for k in (1.402, 0.344136, 0.714136, 1.772):
        ref = np.trunc(k * d.astype(np.float64)).astype(np.int64)
        f32 = np.trunc(np.float32(k) * d.astype(np.float32)).astype(np.int64)
        assert np.array_equal(ref, f32), k
        x = k * d[d != 0]
        assert np.min(np.abs(x - np.round(x))) > 0.001, k


def test_round_clamp_by_truncation():
    """round_clamp_u8 (jpeg_recon_kernel): (int)round(x) clamped to 0..255
    (JPEG.c:440-446) equals trunc + (fraction >= 0.5) clamped, on the values
    where the two could differ: halves, their neighbours, negatives, and
    values past 255."""
    import numpy as np
    xs = []
    for k in range(-3, 259):
        for off in (-0.5, 0.0, 0.5):
            b = k + off
            xs += [b, np.nextafter(b, -1e9), np.nextafter(b, 1e9)]
    xs += list(np.random.default_rng(1).uniform(-300, 600, 20000))
    from decimal import ROUND_HALF_UP, Decimal
    for x in xs:
        x = float(x)
        # C round(): half away from zero, on the exact binary value
        v = int(Decimal(x).quantize(Decimal(1), rounding=ROUND_HALF_UP))
        ref = min(255, max(0, v))
        i = int(x)                                   # toward zero, as v_cvt_i32_f64
        got = min(255, max(0, i + (1 if x - i >= 0.5 else 0)))
        assert got == ref, x
