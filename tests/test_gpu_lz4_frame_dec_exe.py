"""bin/LZ4_frame -D: a frame written by the executable decodes on the GPU to
the input, and to what -d (the host decoder) gives; an error is a message and
exit status 1."""
import os
import subprocess

import pytest

import lz4_frame_model as FM

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "lz4-jpeg_amd", "bin", "LZ4_frame")
GOLDEN = os.path.join(REPO, "tests", "golden")


def run(*args):
    return subprocess.run([EXE, *args], capture_output=True, timeout=120)


def test_file_round_trip_on_the_gpu(gpu, tmp_path):
    src = os.path.join(GOLDEN, "Metamorphosis.txt")
    plain = open(src, "rb").read()
    packed, back, host_back = (str(tmp_path / n) for n in ("out.lz4", "back", "host_back"))
    assert run(src, packed).returncode == 0
    r = run("-D", packed, back)
    assert r.returncode == 0, r.stderr
    assert open(back, "rb").read() == plain
    assert run("-d", packed, host_back).returncode == 0
    assert open(host_back, "rb").read() == open(back, "rb").read()
    # another writer's frame: linked blocks and checksums
    other = str(tmp_path / "other.lz4")
    open(other, "wb").write(FM.write_variant(plain[:30000], linked=True, block_checksum=True,
                                             content_checksum=True))
    assert run("-D", other, back).returncode == 0
    assert open(back, "rb").read() == plain[:30000]
    cut = str(tmp_path / "cut.lz4")
    open(cut, "wb").write(open(packed, "rb").read()[:-5])
    r = run("-D", cut, back)
    assert r.returncode == 1 and b"LZ4_frame: cannot decode" in r.stderr
    assert open(EXE + ".exe", "rb").read() == open(EXE, "rb").read()
