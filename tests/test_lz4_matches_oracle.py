"""lz4o_matches (oracle/lz4_oracle.c), the reference of the batch match finders'
tests, pinned on the CPU: against find_longest_match (LZ4.c:290-323) written
out as a direct Python loop, against the oracle's own encoder (which uses the
uint8_t-truncated form of the same search), and against the match provider of
the sanitizer build (tests/sanitize/cpu_matches.c)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import golden_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = 300


def _lcp(a, i, p, limit):
    """common prefix of a[i:] and a[p:], at most `limit` bytes"""
    d = np.flatnonzero(a[i:i + limit] != a[p:p + limit])
    return int(d[0]) if d.size else min(limit, a.size - p)


def _python_matches(data, window=65535, max_match=1024, min_match=4):
    a = np.frombuffer(data, np.uint8)
    n = a.size
    out = np.zeros(n, np.uint32)
    for p in range(n):
        best, best_dist = 0, 0
        for i in range(max(0, p - window), p):                 # LZ4.c:295-297
            ln = _lcp(a, i, p, min(max_match, n - p))           # clamped at the block end
            if ln > best:                                       # LZ4.c:307: strict
                best, best_dist = ln, p - i
        if best >= min_match:                                   # LZ4.c:314
            out[p] = best | best_dist << 16
    return out


def _blocks():
    text = golden_inputs.lz4_input("metamorphosis_spaces")
    rng = np.random.default_rng(5)
    return {
        "text": bytes(text[4500:4800]),
        "one_value": b"q" * BLK,
        "alphabet_3": bytes(97 + x for x in rng.integers(0, 3, BLK, dtype=np.uint8)),
        "period_7": (b"abcdefg" * 43)[:BLK],
        "short_23": bytes(text[100:123]),
        "abcdabcd": b"abcdabcd",
        "one_byte": b"x",
    }


@pytest.mark.parametrize("name", list(_blocks()))
def test_against_a_direct_python_loop(oracle, name):
    data = _blocks()[name]
    want = _python_matches(data)
    got = oracle.lz4_matches(data)
    assert got.tolist() == want.tolist()
    if name == "one_value":
        assert got[1] == 299 | 1 << 16, "the length is not truncated to uint8_t"
    if name == "abcdabcd":
        assert got.tolist() == [0, 0, 0, 0, 4 | 4 << 16, 0, 0, 0]
    # a sub-range is the same entries; the block form is the pieces' own results
    assert oracle.lz4_matches(data, 3 if len(data) > 3 else 0, len(data)).tolist() == \
        want[3 if len(data) > 3 else 0:].tolist()
    if len(data) == BLK:
        assert oracle.lz4_block_matches(data + data[:77]).tolist() == \
            want.tolist() + _python_matches(data[:77]).tolist()


def test_block_form_is_per_piece(oracle):
    b = _blocks()
    data = b["text"] + b["one_value"] + b["alphabet_3"][:150]
    want = np.concatenate([oracle.lz4_matches(x) for x in
                           (b["text"], b["one_value"], b["alphabet_3"][:150])])
    assert oracle.lz4_block_matches(data).tolist() == want.tolist()


def test_window_and_cap_in_a_long_block(oracle):
    """The 1024 cap and the window's lower edge, on inputs whose answer is
    known in closed form."""
    run = b"\x07" * 2100
    got = oracle.lz4_matches(run)
    assert got.tolist() == [0] + [min(1024, 2100 - p) | p << 16 if 2100 - p >= 4 else 0
                                  for p in range(1, 2100)]
    # two copies of a 16-byte motif 65535 and 65536 bytes before their repeats
    rng = np.random.default_rng(9)
    d = bytearray(rng.integers(0, 256, 66000, dtype=np.uint8).tobytes())
    m1, m2 = bytes(range(16)), bytes(range(100, 116))
    d[10:26], d[10 + 65535:26 + 65535] = m1, m1
    d[50:66], d[50 + 65536:66 + 65536] = m2, m2
    d = bytes(d)
    assert oracle.lz4_matches(d, 10 + 65535, 11 + 65535)[0] == 16 | 65535 << 16
    assert oracle.lz4_matches(d, 50 + 65536, 51 + 65536)[0] == 0


@pytest.fixture(scope="module")
def cpu_matches(tmp_path_factory):
    """tests/sanitize/cpu_matches.c as a shared library (its function is
    hidden, lzj_host.h: a visible wrapper in the same translation unit)"""
    d = tmp_path_factory.mktemp("cpu_matches")
    src, so = d / "wrap.c", d / "libcpu_matches.so"
    src.write_text(
        '#include "%s"\n'
        "int cpu_matches_all(const uint8_t *in, size_t n, uint32_t *match) {\n"
        "  return lzj_block_matches(in, n, match);\n}\n"
        % os.path.join(REPO, "tests", "sanitize", "cpu_matches.c"))
    subprocess.run(["gcc", "-O1", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = ctypes.CDLL(str(so))
    L.cpu_matches_all.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.cpu_matches_all.restype = ctypes.c_int
    return L


def test_against_the_sanitizer_builds_match_provider(oracle, cpu_matches):
    text = golden_inputs.lz4_input("metamorphosis_spaces")
    inputs = list(_blocks().values()) + [bytes(text[7000:7301]), bytes(text[2000:3000]),
                                          (b"lz4r_7!" * 300)[:2000]]
    for data in inputs:
        a = np.frombuffer(data, np.uint8)
        got = np.zeros(a.size, np.uint32)
        assert cpu_matches.cpu_matches_all(a.ctypes.data_as(ctypes.c_void_p), a.size,
                                             got.ctypes.data_as(ctypes.c_void_p)) == 0
        assert oracle.lz4_matches(data).tolist() == got.tolist(), len(data)


def test_the_encoder_uses_the_same_search(oracle):
    """lz4o_encode_block's greedy parse, replayed over lz4o_matches with the
    uint8_t truncation (LZ4.c:317), takes the same number of sequences."""
    for data in (v for v in _blocks().values() if len(v) == BLK):
        m = oracle.lz4_matches(data)
        p, nseq, lit = 0, 0, 0
        while p < len(data):
            M = int(m[p] & 0xFFFF) & 0xFF if m[p] else 0
            if M == 0:
                p, lit = p + 1, lit + 1
            else:
                p, lit, nseq = p + M, 0, nseq + 1
        nseq += 1 if lit else 0
        enc = oracle.lz4_blocks(np.frombuffer(data, np.uint8), 0, 1)
        assert enc[0] == nseq & 0xFF
