"""JPEG_dec <in.jpr> <out.png> <image> thumb writes that image's 1/8-scale
thumbnail, one pixel per tile (jpegr_thumb_device, include/jpegr.h): the pixels
of jpeg.thumbnails_device; its errors are one line on stderr, exit status 1 and
no output file."""
import os
import subprocess

import numpy as np
import pytest

import pngdec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "lz4-jpeg_amd", "bin")
W, H, NIMG = 40, 24, 2                               # 5 x 3 tiles an image


def dec(*args):
    return subprocess.run([os.path.join(BIN, "JPEG_dec"), *map(str, args)], capture_output=True,
                          timeout=120)


@pytest.fixture(scope="module")
def jpr(gpu, oracle, tmp_path_factory):
    """(a two-image JPT1 stream's path, thumbnails_device's pixels [2, 3, 5, 4])."""
    import torch
    from lz4jpeg import jpeg
    imgs = np.stack([oracle.rand_image(W, H, seed=11 + i) for i in range(NIMG)])
    d_stream = jpeg.compress_device(torch.from_numpy(imgs).cuda().reshape(-1), W, H, NIMG, tight=True)
    want, w, h, count = jpeg.thumbnails_device(d_stream)
    assert (w, h, count) == (W, H, NIMG) and want.shape == (NIMG, 3, 5, 4)
    path = str(tmp_path_factory.mktemp("thumb") / "two.jpr")
    open(path, "wb").write(d_stream.cpu().numpy().tobytes())
    return path, want.cpu().numpy()


@pytest.mark.parametrize("image", [0, 1])
def test_thumbnail_is_thumbnails_device(jpr, tmp_path, image):
    path, want = jpr
    out = str(tmp_path / "thumb.png")
    r = dec(path, out, image, "thumb")
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    got = np.asarray(pngdec.read(out))
    assert got.shape == (3, 5, 4)
    assert np.array_equal(got, want[image])
    assert not np.array_equal(want[0], want[1])


def test_errors_exit_1_without_a_file(jpr, tmp_path):
    """An image past the stream's, a corrupted header, a malformed tile."""
    path, _ = jpr
    data = open(path, "rb").read()
    wrong_magic, wrong_h = str(tmp_path / "magic.jpr"), str(tmp_path / "h.jpr")
    open(wrong_magic, "wb").write(b"K" + data[1:])
    open(wrong_h, "wb").write(data[:8] + (H + 8).to_bytes(4, "little") + data[12:])
    bad_tile = str(tmp_path / "tile.jpr")
    rec0 = 16 + 2 * 15 * NIMG
    open(bad_tile, "wb").write(data[:rec0 + 1] + bytes([129]) + data[rec0 + 2:])   # luma ncodes = 129
    out = str(tmp_path / "none.png")
    for args in ((path, out, NIMG, "thumb"), (wrong_magic, out, 0, "thumb"), (wrong_h, out, 0, "thumb"),
                 (bad_tile, out, 0, "thumb"), (path, out, "x", "thumb")):
        r = dec(*args)
        assert r.returncode == 1 and r.stdout == b"", args
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert not os.path.exists(out)
    r = dec(bad_tile, out, 1, "thumb")                   # image 1 does not hold the bad tile
    assert r.returncode == 0, r.stderr


def test_another_word_is_a_usage_error(jpr, tmp_path):
    out = str(tmp_path / "none.png")
    for word in ("thumbs", "THUMB", "8"):
        r = dec(jpr[0], out, 0, word)
        assert r.returncode == 1 and b"usage" in r.stderr and not os.path.exists(out)
