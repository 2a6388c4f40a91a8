"""JPEG_sel <in.jpr> <out.jpr> <jpr|jpt|same> images <i>... | tiles <w> <h>
<image:x:y>... writes the stream StreamReader.select gives (jpegr_select_device,
include/jpegr.h); JPEG_dec reads the result; its errors are one line on stderr,
exit status 1 and no output file."""
import os
import subprocess

import numpy as np
import pytest

import pngdec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "lz4-jpeg_amd", "bin")
W, H, NIMG = 40, 24, 3                               # 5 x 3 tiles an image


def run(exe, *args):
    return subprocess.run([os.path.join(BIN, exe), *map(str, args)], capture_output=True, timeout=120)


@pytest.fixture(scope="module")
def jpr(gpu, oracle, tmp_path_factory):
    """(a three-image JPR1 stream's path, its StreamReader)."""
    import torch
    from lz4jpeg import jpeg
    imgs = np.stack([oracle.rand_image(W, H, seed=21 + i) for i in range(NIMG)])
    d_stream = jpeg.compress_device(torch.from_numpy(imgs).cuda().reshape(-1), W, H, NIMG)
    path = str(tmp_path_factory.mktemp("sel") / "three.jpr")
    open(path, "wb").write(d_stream.cpu().numpy().tobytes())
    return path, jpeg.StreamReader(d_stream)


@pytest.mark.parametrize("word,tight", [("same", None), ("jpr", False), ("jpt", True)])
def test_images_form(jpr, tmp_path, word, tight):
    path, rd = jpr
    out = str(tmp_path / "out.jpr")
    r = run("JPEG_sel", path, out, word, "images", 2, 0, 2)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert open(out, "rb").read() == rd.select([2, 0, 2], tight=tight).cpu().numpy().tobytes()


@pytest.mark.parametrize("word,tight", [("same", None), ("jpt", True)])
def test_tiles_form_and_jpeg_dec_reads_it(jpr, tmp_path, word, tight):
    from lz4jpeg import jpeg
    path, rd = jpr
    out, png = str(tmp_path / "out.jpr"), str(tmp_path / "out.png")
    r = run("JPEG_sel.exe", path, out, word, "tiles", 21, 16, "1:16:8", "0:0:0")
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    want = rd.select([1, 0], x=[16, 0], y=[8, 0], w=21, h=16, tight=tight)
    assert open(out, "rb").read() == want.cpu().numpy().tobytes()
    r = run("JPEG_dec", out, png, 1)
    assert r.returncode == 0, r.stderr
    px, w, h, n = jpeg.decompress_images_device(want, 1, 1)
    assert np.array_equal(np.asarray(pngdec.read(png)), px.cpu().numpy().reshape(h, w, 4))


def test_errors_exit_1_without_a_file(jpr, tmp_path):
    """An image past the stream's, a window off the tile grid or the image, a
    corrupted header, a truncated stream, a malformed record while re-coding."""
    path, _ = jpr
    data = open(path, "rb").read()
    wrong_magic, short, bad_tile = (str(tmp_path / n) for n in ("magic.jpr", "short.jpr", "tile.jpr"))
    open(wrong_magic, "wb").write(b"K" + data[1:])
    open(short, "wb").write(data[:-1])
    rec0 = 16 + 2 * 15 * NIMG
    open(bad_tile, "wb").write(data[:rec0 + 1] + bytes([129]) + data[rec0 + 2:])   # luma ncodes = 129
    out = str(tmp_path / "none.jpr")
    for args in ((path, out, "same", "images", NIMG), (path, out, "jpt", "images", 0, 7),
                 (path, out, "same", "tiles", 8, 8, "0:4:0"), (path, out, "same", "tiles", 16, 8, "0:32:0"),
                 (path, out, "same", "tiles", 41, 8, "0:0:0"), (path, out, "same", "tiles", 0, 8, "0:0:0"),
                 (wrong_magic, out, "same", "images", 0), (short, out, "same", "images", 0),
                 (bad_tile, out, "jpt", "images", 0), (str(tmp_path / "absent.jpr"), out, "same", "images", 0)):
        r = run("JPEG_sel", *args)
        assert r.returncode == 1 and r.stdout == b"", args
        assert len(r.stderr.strip().splitlines()) == 1 and b"usage" not in r.stderr, r.stderr
        assert not os.path.exists(out), args
    r = run("JPEG_sel", bad_tile, out, "jpt", "images", 1)     # image 1 does not hold the bad tile
    assert r.returncode == 0, r.stderr


def test_other_argument_forms_are_usage_errors(jpr, tmp_path):
    path, _ = jpr
    out = str(tmp_path / "none.jpr")
    for args in ((path, out, "same", "images"), (path, out, "jpg", "images", 0),
                 (path, out, "same", "image", 0), (path, out, "same", "images", "x"),
                 (path, out, "same", "images", -1), (path, out, "same", "tiles", 8, 8),
                 (path, out, "same", "tiles", 8, 8, "0:0"), (path, out, "same", "tiles", 8, 8, "0:0:0:0"),
                 (path, out, "same", "tiles", "a", 8, "0:0:0"), (path, out), ()):
        r = run("JPEG_sel", *args)
        assert r.returncode == 1 and b"usage" in r.stderr and r.stdout == b"", args
        assert not os.path.exists(out)
