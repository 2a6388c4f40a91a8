"""Standard LZ4 frames from the GPU (csrc/lz4r_frame.h: lz4f_sizes, lz4f_scan,
lz4f_emit) against the model (tests/lz4_frame_model.py: the oracle's native
stream passed through the frame's rules): byte equality, and the frame decoded
back by lz4r_frame_decompress.  Inputs sit where the plan can go wrong: data
blocks of 1, 11, 12 and 13 bytes, matches at a data block's end (cut, demoted,
truncated by the reference's uint8_t), literal runs at the extension
thresholds, source blocks whose records reach the overflow slots, every
pointer alignment, every capacity, the chunked path and a captured graph."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lz4_chunk_lib
import lz4_format
import lz4_frame_model as FM
from lz4_seq_inputs import BLK, block_endmatch, block_exact, block_packed, block_trunc, enc_of
from lz4jpeg import _lib, lz4

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUP = FM.GROUP


@pytest.fixture(scope="module")
def text():
    return open(os.path.join(GOLDEN, "Metamorphosis.txt"), "rb").read()


@pytest.fixture(scope="module")
def comp(gpu):
    c = lz4.Compressor()
    yield c
    c.close()


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def block_latematch():
    """Random bytes with one match of 6 at byte 290: it starts in the last 11
    bytes of a data block that this block ends (rule 2)."""
    r = rnd(BLK, 41)
    return r[:290] + r[50:56] + r[296:]


def block_longend():
    """Random bytes with one match of 20 that ends the block: at a data
    block's end it is cut to 15 (rule 3)."""
    r = rnd(BLK, 42)
    return r[:280] + r[20:40]


def specials(oracle):
    s = [block_endmatch(12), block_latematch(), block_longend(), block_trunc(256),
         block_trunc(257), block_trunc(259)]
    # what each is for, read from the oracle's own encoding
    seqs = [next(lz4_format.readings(enc_of(oracle, b))) for b in s]
    ends = [sum(L + M for L, _, M in q) for q in seqs]
    assert ends == [BLK] * 6
    assert seqs[0][-1][2] == 4, "a last match that ends the block"
    assert seqs[1] == [(290, 240, 6), (4, 0, 0)], "a match starting in the last 11 bytes"
    assert seqs[2] == [(280, 260, 20)], "a long match ending the block"
    assert seqs[3][0] == (22, 2, 255), "256 equal bytes: a literal, then a match of 255"
    assert any(M == 1 for _, _, M in seqs[4]) and any(M == 3 for _, _, M in seqs[5]), "truncated"
    return s


def text_blocks(text, first, count):
    return [text[BLK * (first + i):BLK * (first + i + 1)] for i in range(count)]


_cases = {}


def case(oracle, name, build):
    """(plain, expected frame, literal lengths per data block), built once."""
    if name not in _cases:
        plain = build()
        _cases[name] = (plain,) + FM.expected(oracle, plain)
    return _cases[name]


def gpu_frame(comp, plain, check_decode=True):
    d_in = torch.from_numpy(np.frombuffer(plain, np.uint8).copy()).cuda()
    d_out, n = comp.compress_frame_device(d_in)
    got = d_out[:n].cpu().numpy().tobytes()
    if check_decode:
        assert lz4.decompress_frame(got) == plain
    return got


@pytest.mark.parametrize("n", [300, 19200, 19201, 19211, 19212, 19213, 38701])
def test_lengths(oracle, comp, text, n):
    plain, want, _ = case(oracle, f"text {n}", lambda: text[:n])
    assert gpu_frame(comp, plain) == want


def test_golden_input(oracle, comp):
    plain = open(os.path.join(GOLDEN, "lz4_input.txt"), "rb").read()
    assert len(plain) == 350
    _, want, _ = case(oracle, "golden", lambda: plain)
    assert gpu_frame(comp, plain) == want
    assert lz4.compress_frame(plain) == want            # the host-buffer call
    assert comp.compress_frame(plain) == want


def test_special_blocks_last_and_first_of_a_data_block(oracle, comp, text):
    """Six data blocks: special i first (nothing of it is cut), 62 text blocks,
    special i + 1 last (rules 1-3 at the data block's end)."""
    def build():
        s = specials(oracle)
        return b"".join(s[i] + b"".join(text_blocks(text, 60 * i, 62)) + s[(i + 1) % 6]
                        for i in range(6))
    plain, want, runs = case(oracle, "specials in groups", build)
    assert len(plain) == 6 * GROUP
    got = gpu_frame(comp, plain)
    assert got == want
    assert FM.decode_strict(got) == plain


@pytest.mark.parametrize("i", range(6))
def test_special_block_as_the_inputs_last(oracle, comp, text, i):
    plain, want, _ = case(oracle, f"special {i} last",
                          lambda: b"".join(text_blocks(text, 5, 2)) + specials(oracle)[i])
    got = gpu_frame(comp, plain)
    assert got == want
    assert FM.decode_strict(got) == plain


@pytest.mark.parametrize("L", [14, 15, 269, 270, 525])
def test_literal_run_lengths(oracle, comp, L):
    """L literals merged over source blocks, then a match within its block."""
    def build():
        r = rnd(L, 100 + L)
        at = L % BLK                                     # the match's place in its source block
        assert at >= 12
        blockstart = L - at
        return r + r[blockstart:blockstart + 8] + rnd(2 * BLK - (L + 8) % BLK, 200 + L)
    plain, want, runs = case(oracle, f"run {L}", build)
    assert runs[0][0] == L and len(runs[0]) == 2
    assert gpu_frame(comp, plain) == want


def test_one_run_of_a_whole_data_block(oracle, comp):
    plain, want, runs = case(oracle, "random 19200", lambda: rnd(GROUP, 7))
    assert runs == [[GROUP]]
    assert want[19:19 + 77] == b"\xf0" + b"\xff" * 75 + bytes([(GROUP - 15) % 255])
    assert gpu_frame(comp, plain) == want


def test_record_counts_reach_the_overflow_slots(oracle, comp, text):
    """Source blocks of 53 and 70 records; a data block of 64 of the latter
    is the largest flattened record count."""
    def build():
        packed = [block_packed(20, s) for s in range(4)]
        assert all(enc_of(oracle, b)[0] == 70 for b in packed)
        full = b"".join(packed[i % 4] for i in range(64))
        exact = block_exact(53) * 64
        mixed = b"".join((packed[i % 4], block_exact(53), text[BLK * i:BLK * (i + 1)])[i % 3]
                         for i in range(40))
        return full + exact + mixed + text[:123]
    plain, want, _ = case(oracle, "records", build)
    got = gpu_frame(comp, plain)
    assert got == want
    assert FM.decode_strict(got) == plain


def test_misaligned_pointers(oracle, comp, text):
    plain, want, _ = case(oracle, "text 19500", lambda: text[300:300 + 19500])
    n, cap = len(plain), lz4.frame_bound(len(plain))
    src = torch.from_numpy(np.frombuffer(plain, np.uint8).copy())
    for k in range(1, 16):
        d_in = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
        d_in[k:k + n] = src.cuda()
        d_out = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        j = 16 - k if k % 2 else k                      # the output's own misalignment
        _, length = comp.compress_frame_device(d_in[k:k + n], n, d_out[j:j + cap])
        out = d_out.cpu().numpy()
        assert out[j:j + length].tobytes() == want, (k, j)
        assert (out[:j] == 0xEE).all() and (out[j + length:] == 0xEE).all(), (k, j)


def test_capacity(oracle, comp, text):
    plain, want, _ = case(oracle, "text 38701", lambda: text[:38701])
    need = len(want)
    d_in = torch.from_numpy(np.frombuffer(plain, np.uint8).copy()).cuda()
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    for cap in (0, 1, 14, 15, 16, need - 4, need - 1, need):
        d_buf = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        # (the C call: the buffer is there, the capacity is what the call is told)
        rc = _lib.call("lz4r_compress_frame_async", comp._h, d_in, len(plain), d_buf, cap, d_len,
                       _lib.stream_arg())
        assert rc == 0
        assert comp.async_length(d_len) == need, cap    # the need, whatever the capacity
        out = d_buf.cpu().numpy()
        assert out[:cap].tobytes() == want[:cap], cap
        assert (out[cap:] == 0xEE).all(), cap
    with pytest.raises(lz4.Lz4Error) as e:
        comp.compress_frame_device(d_in, len(plain), torch.empty(need - 1, dtype=torch.uint8,
                                                                 device="cuda"))
    assert e.value.code == _lib.LZ4R_ERR_CAPACITY
    with pytest.raises(lz4.InputTooSmall):
        comp.compress_frame_device(d_in, 299)


def test_one_context_alternates_native_and_frame_calls(oracle, gpu, text):
    c = lz4.Compressor()
    for n in (38701, 300, 19213, 60000, 19200):
        plain, want, _ = case(oracle, f"text {n}", lambda: text[:n])
        d_in = torch.from_numpy(np.frombuffer(plain, np.uint8).copy()).cuda()
        d_out, length = c.compress_device(d_in)
        assert d_out[:length].cpu().numpy().tobytes() == oracle.lz4_compress(plain), n
        nb = lz4.nblocks(n)
        offs = c.block_offsets(nb)
        assert c.block_offsets_device()[1] == nb
        d_out, length = c.compress_frame_device(d_in)
        assert d_out[:length].cpu().numpy().tobytes() == want, n
        with pytest.raises(lz4.Lz4Error) as e:
            c.block_offsets(nb)
        assert e.value.code == _lib.LZ4R_ERR_ARG
        with pytest.raises(lz4.Lz4Error):
            c.block_offsets_device()
        c.check()
        d_out, length = c.compress_device(d_in)          # and the native arrays are back
        assert d_out[:length].cpu().numpy().tobytes() == oracle.lz4_compress(plain), n
        assert (c.block_offsets(nb) == offs).all()
    c.close()


def test_chunked_path(oracle, gpu, text):
    """The chunk12 build: (4096 + 64 + 1) blocks + 7 bytes cross a launch chunk
    (the scan continues from the length word, the data block offsets restart
    in the scratch) and a data block in the second chunk."""
    L = lz4_chunk_lib.load("chunk12")
    assert lz4_chunk_lib.chunk_blocks("chunk12") == 4096
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.lz4r_compress_frame_async.restype = ctypes.c_int
    L.lz4r_compress_frame_async.argtypes = [vp, vp, sz, vp, sz, vp, vp]
    L.lz4r_frame_bound.restype = sz
    L.lz4r_frame_bound.argtypes = [sz]
    n = (4096 + 64 + 1) * BLK + 7
    plain, want, _ = case(oracle, "chunked", lambda: (text * (n // len(text) + 1))[:n])
    cap = L.lz4r_frame_bound(n)
    assert cap == lz4.frame_bound(n)
    ctx = lz4_chunk_lib.Ctx("chunk12")
    d_in = torch.from_numpy(np.frombuffer(plain, np.uint8).copy()).cuda()
    d_out = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):                                   # the second call: scratch in use before
        rc = L.lz4r_compress_frame_async(ctx.h, vp(d_in.data_ptr()), n, vp(d_out.data_ptr()), cap,
                                         vp(d_len.data_ptr()), stream)
        assert rc == 0
        length = int(d_len.item())
        out = d_out.cpu().numpy()
        assert length == len(want) and out[:length].tobytes() == want
        assert (out[length:] == 0xEE).all()
    assert ctx.check() == 0
    ctx.close()
    assert lz4.decompress_frame(want) == plain


def test_captured_in_a_graph(oracle, comp, text):
    a, want_a, _ = case(oracle, "text 38701", lambda: text[:38701])
    b, want_b, _ = case(oracle, "text b", lambda: text[50000:50000 + 38701])
    n, cap = len(a), lz4.frame_bound(len(a))
    d_in = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call():
        comp.compress_frame_async(d_in, n, d_out, d_len)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                           # warm-up: the scratch exists
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for plain, want in ((a, want_a), (b, want_b), (a, want_a)):
        d_in.copy_(torch.from_numpy(np.frombuffer(plain, np.uint8).copy()))
        d_out.fill_(0xEE)
        d_len.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        length = comp.async_length(d_len)
        assert d_out[:length].cpu().numpy().tobytes() == want
