"""ASan + UBSan run of the standard-frame host decoder (host/lz4f_decode.c):
tests/sanitize/frame_main.c, a stand-alone program built and run by
`make sanitize-frame`; no GPU needed."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_decoder_under_asan_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(["make", "-C", REPO, "sanitize-frame"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize-frame ok" in r.stdout
