"""ASan + UBSan run of what the GPU frame decoder's kernels parse with
(csrc/lz4f_parse.h, compiled for the host): tests/sanitize/frame_dev_main.cpp,
a stand-alone program built and run by `make sanitize-frame-dev`.  It takes
every prefix and every single-byte mutation of the model's variant frames
through the device decoder's stages and through lz4r_frame_decompress, and the
verdicts must agree; no GPU needed, nothing loaded into Python.  (The kernels'
LDS window, through which they fetch the bytes the parsers ask for, is device
code and not part of this run.)"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_parsers_under_asan_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(["make", "-C", REPO, "sanitize-frame-dev"], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize-frame-dev ok (7 frames" in r.stdout
