"""bin/LZ4_frame: a file compressed on the GPU to a standard LZ4 frame equals
the model's frame (tests/lz4_frame_model.py), -d restores the input on the
host, and an error is a message and exit status 1."""
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


@pytest.mark.parametrize("name", ["lz4_input.txt", "Metamorphosis.txt"])
def test_file_round_trip(gpu, oracle, tmp_path, name):
    src = os.path.join(GOLDEN, name)
    plain = open(src, "rb").read()
    packed, back = str(tmp_path / "out.lz4"), str(tmp_path / "back")
    r = run(src, packed)
    assert r.returncode == 0, r.stderr
    frame = open(packed, "rb").read()
    assert frame == FM.expected(oracle, plain)[0]
    r = run("-d", packed, back)
    assert r.returncode == 0, r.stderr
    assert open(back, "rb").read() == plain
    # the twin the reference's drivers would spawn
    assert open(EXE + ".exe", "rb").read() == open(EXE, "rb").read()
    if name == "lz4_input.txt":
        cut = str(tmp_path / "cut.lz4")
        open(cut, "wb").write(frame[:-5])
        r = run("-d", cut, back)
        assert r.returncode == 1 and b"LZ4_frame: cannot decode" in r.stderr
        assert run("-d", str(tmp_path / "missing"), back).returncode == 1
        assert run(src).returncode == 1                     # usage
        small = str(tmp_path / "small")
        open(small, "wb").write(b"y" * 299)
        r = run(small, packed)
        assert r.returncode == 1 and b"input shorter" in r.stderr
