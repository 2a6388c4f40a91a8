"""JPEG_dec <in.jpr> <out.png> image x y w h writes only that rectangle of what
JPEG_dec <in.jpr> <out.png> image writes (jpegr_stream_index_device +
jpegr_crop_device, include/jpegr.h); its errors are one line on stderr, exit
status 1 and no output file."""
import os
import subprocess

import numpy as np
import pytest

import pngdec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "lz4-jpeg_amd", "bin")


def dec(*args):
    return subprocess.run([os.path.join(BIN, "JPEG_dec"), *map(str, args)], capture_output=True,
                          timeout=120)


@pytest.fixture(scope="module")
def jpr(gpu, oracle, tmp_path_factory):
    """(JPEG_seq's coefficients.jpr of a 61 x 45 image, the pixels JPEG_dec gives for it)."""
    tmp = tmp_path_factory.mktemp("crop")
    w, h = 61, 45                                   # partial tiles on both edges
    src = str(tmp / "in.png")
    pngdec.write(src, oracle.rand_image(w, h, seed=7))
    out_dir = str(tmp / "out") + os.sep
    os.makedirs(out_dir)
    r = subprocess.run([os.path.join(BIN, "JPEG_seq"), src, out_dir], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    path, whole = out_dir + "coefficients.jpr", str(tmp / "whole.png")
    r = dec(path, whole, 0)
    assert r.returncode == 0, r.stderr
    full = np.asarray(pngdec.read(whole))
    assert full.shape[:2] == (h, w)
    return path, full


@pytest.mark.parametrize("rect", [(0, 0, 61, 45), (13, 7, 37, 9), (60, 44, 1, 1), (5, 40, 56, 5)])
def test_rectangle_is_the_slice(jpr, tmp_path, rect):
    path, full = jpr
    x, y, w, h = rect
    out = str(tmp_path / "crop.png")
    r = dec(path, out, 0, x, y, w, h)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    got = np.asarray(pngdec.read(out))
    assert got.shape[:2] == (h, w)
    assert np.array_equal(got, full[y:y + h, x:x + w])


@pytest.mark.parametrize("args", [(0, 60, 0, 2, 1), (0, 0, 44, 1, 2), (0, 62, 0, 1, 1), (0, 0, 0, 62, 1),
                                  (0, 0, 0, 0, 5), (0, 3, 3, 4, 0), (1, 0, 0, 4, 4),
                                  (0, 0, 0, "4x", 4), (0, -1, 0, 4, 4)])
def test_errors_exit_1_without_a_file(jpr, tmp_path, args):
    """Outside the image, zero-sized, an image past the stream's, not a number."""
    out = str(tmp_path / "none.png")
    r = dec(jpr[0], out, *args)
    assert r.returncode == 1 and r.stdout == b""
    assert len(r.stderr.strip().splitlines()) == 1
    assert not os.path.exists(out)


@pytest.mark.parametrize("extra", [(0, 1), (0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4, 5)])
def test_partial_rectangle_is_a_usage_error(jpr, tmp_path, extra):
    """5, 6 or 7 arguments (and more than 8), the program's name counted."""
    out = str(tmp_path / "none.png")
    r = dec(jpr[0], out, *extra)
    assert r.returncode == 1 and r.stdout == b"" and b"usage" in r.stderr
    assert not os.path.exists(out)


def test_bad_record_in_the_rectangle(jpr, tmp_path):
    """A bad verdict: the first tile's luma ncodes past its slot fails a
    rectangle on that tile and leaves one beside it alone."""
    path, full = jpr
    data = bytearray(open(path, "rb").read())
    nt = 8 * 6
    data[16 + 2 * nt + 1] = 129
    bad = str(tmp_path / "bad.jpr")
    open(bad, "wb").write(bytes(data))
    out = str(tmp_path / "a.png")
    r = dec(bad, out, 0, 7, 7, 1, 1)
    assert r.returncode == 1 and len(r.stderr.strip().splitlines()) == 1 and not os.path.exists(out)
    r = dec(bad, out, 0, 8, 0, 20, 20)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(pngdec.read(out)), full[0:20, 8:28])
