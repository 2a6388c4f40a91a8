"""JPEG_seq also writes coefficients.jpr, the packed entropy-coded stream
(include/jpegr.h), next to coefficients.bin: it unpacks and entropy-decodes
to exactly those coefficients."""
import os
import subprocess

import numpy as np
import pytest

import jpr_format as J
import pngdec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "lz4-jpeg_amd", "bin", "JPEG_seq")


def test_jpeg_seq_writes_the_packed_stream(gpu, oracle, tmp_path):
    import torch
    from lz4jpeg import jpeg
    w, h = 64, 48
    img = oracle.rand_image(w, h, seed=5)
    src = str(tmp_path / "in.png")
    pngdec.write(src, img)
    out_dir = str(tmp_path / "out") + os.sep
    os.makedirs(out_dir)
    r = subprocess.run([EXE, src, out_dir], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b""
    assert sorted(os.listdir(out_dir)) == sorted(
        ["original.png", "luminance.png", "rChrominance.png", "bChrominance.png",
         "reconstructed.png", "coefficients.bin", "coefficients.jpr"])
    data = open(out_dir + "coefficients.jpr", "rb").read()
    coef = np.fromfile(out_dir + "coefficients.bin", dtype="<i2")
    assert J.header(data) == (64, 48, 1)
    assert jpeg.stream_info(data[:16]) == (64, 48, 1)
    assert J.unpack(data)[3:] == (len(data), J.OK)
    d_stream = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    ent, d_res = jpeg.unpack_device(d_stream, len(data), w, h)
    back = torch.zeros(coef.size, dtype=torch.int16, device="cuda")
    ent.decode(back)
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().tolist()] == [len(data), -1]
    assert int(ent.status[1].item()) == 0
    assert np.array_equal(back.cpu().numpy(), coef)
