"""The chunked call path of run() (csrc/lz4r.hip) against the oracle, at a
chunk size a test can afford.

A call is cut into launches of kChunk blocks.  In the product kChunk is 2^24
(5 GB of input), so everything that differs in the second and later chunks --
the input, size and record-slot bases, the scan continuing from the length
word, record slots that still hold the previous chunk's heads, a chunk's last
block staged although it is not the input's last, the timing events per chunk
-- runs in one slow test only.  `make chunk12` builds the same source with the
same flags and kChunk = 2^12 (tests/lz4_chunk_lib.py), where an input of
2.5 MB has three chunks.  Every case here runs through the C ABI of both
builds and compares, with the oracle's per-block encodings of the same bytes:
the whole stream, the length word (bit 63 clear), every device block offset
and size, and 0xEE canaries before the output and after the reported length.

lz4r_launch_chunk_blocks() is asserted first (4096 / 2^24): without it a
variant that was built without the define would pass while crossing nothing.
"""
import numpy as np
import pytest

import golden_inputs
import lz4_chunk_lib
from lz4_seq_inputs import BLK, Expected, block_types

C = 1 << lz4_chunk_lib.CHUNK12_LOG2            # blocks per chunk of the variant
THREE = (2 * C + 33, 277)                      # three chunks: the middle one is neither first nor last
# (blocks, bytes of the last block)
SIZES = [(C, BLK), (C + 1, 1), (C + 1, 23), (C + 1, 24), (C + 1, BLK), (2 * C, BLK), THREE]
PAD = 16                                       # canary bytes in front of the output
ROLES = {0: "second-to-last", 1: "last", 2: "first"}     # of a chunk: blocks kC - 2 + q


class Content:
    """2C + 33 whole blocks and the oracle's encoding of each."""

    def __init__(self, data, blocks):
        assert len(data) == BLK * len(blocks)
        self.data, self.blocks = data, blocks


class Case(Expected):
    """A prefix of a content: nb blocks, the last of last_n bytes."""

    def __init__(self, oracle, content, nb, last_n):
        super().__init__(oracle, content.data[:BLK * (nb - 1) + last_n], known=content.blocks)
        assert self.nb == nb
        self.n = len(self.data)


@pytest.fixture(scope="module")
def types(oracle):
    """The five block types of lz4_seq_inputs and their encodings; what
    each type is for is asserted from the oracle's result."""
    text = golden_inputs.lz4_input("metamorphosis_spaces")
    t = block_types(text)
    enc = [oracle.lz4_blocks(np.frombuffer(x, np.uint8), 0, 1) for x in t]
    m = [oracle.lz4_matches(x) for x in t]
    # block header: u8 sequence count, u16 size (LZ4.c:415-425)
    assert (m[0][1] & 0xFFFF) >= 256, "a match of at least 256 bytes"
    assert m[1][2] == (BLK - 2) | 2 << 16 and (m[1][2:BLK - 3] >> 16 > 2).any(), "period 2"
    assert enc[2][0] == 1 and len(enc[2]) > BLK and not m[2].any(), "one literal run"
    assert 2 < enc[3][0] <= 23, "text: a few sequences, no overflow slot"
    assert enc[4][0] > 23, "the overflow slot (records 23..) is not exercised"
    assert ((m[4] & 0xFFFF)[m[4] != 0] == 4).mean() > 0.5, "exact-4 matches"
    return t, enc


@pytest.fixture(scope="module")
def base(oracle):
    """The book, repeated, as 2C + 33 whole blocks, encoded once per module."""
    book = golden_inputs.lz4_input("metamorphosis_spaces")
    assert len(book) % BLK != 0, "the blocks must differ from lap to lap"
    nb = THREE[0]
    assert len(book) < C * BLK, "every chunk must hold more than one lap"
    data = (book * (nb * BLK // len(book) + 1))[:nb * BLK]
    buf = np.frombuffer(data, np.uint8)
    return Content(data, [oracle.lz4_blocks(buf, b, b + 1) for b in range(nb)])


def _type_at(j, k, q):
    return (j + q + 2 * k) % 5


@pytest.fixture(scope="module")
def contents(base, types):
    """Five inputs: the base with the block types at blocks kC - 2 .. kC + 1,
    k = 1, 2, rotated so that over the five every type is a chunk's
    second-to-last, last and first block."""
    t, enc = types
    out = []
    for j in range(5):
        data, blocks = bytearray(base.data), list(base.blocks)
        for k in (1, 2):
            for q in range(4):
                b, ty = k * C - 2 + q, _type_at(j, k, q)
                data[BLK * b:BLK * (b + 1)] = t[ty]
                blocks[b] = enc[ty]
        out.append(Content(bytes(data), blocks))
    # the placement, read back from the inputs
    for q in ROLES:
        for ty in range(5):
            hits = [(j, k) for j in range(5) for k in (1, 2)
                    if out[j].data[BLK * (k * C - 2 + q):BLK * (k * C - 1 + q)] == t[ty]]
            assert hits, f"type {ty} is never a chunk's {ROLES[q]} block"
    assert len({c.data for c in out}) == 5
    return out


def test_constructed_inputs_have_their_properties(oracle, contents):
    """No GPU: setting the fixtures up asserted the types' properties and
    their placement at the chunk boundaries.  Here: a case's expectation is
    the oracle's own stream of the same bytes."""
    case = Case(oracle, contents[3], C + 1, 23)
    assert case.framed() == oracle.lz4_compress(case.data)
    assert case.offsets()[C] == len(case.body()) - len(case.blocks[C])
    assert SIZES[-1] == THREE and -(-THREE[0] // C) == 3


# ---- running a case --------------------------------------------------------

@pytest.fixture(scope="module", params=lz4_chunk_lib.NAMES)
def ctx(request, gpu):
    name = request.param
    # before anything else: the build really has the chunk size it is tested for
    assert lz4_chunk_lib.chunk_blocks(name) == lz4_chunk_lib.expected_chunk_blocks(name)
    assert lz4_chunk_lib.chunk_blocks("chunk12") == C and lz4_chunk_lib.chunk_blocks(
        "product") == 1 << 24
    c = lz4_chunk_lib.Ctx(name)
    yield c
    c.close()


def _bound(nb):
    return 1 + nb * 1152


def _device_input(data, in_off=0):
    import torch
    d_buf = torch.empty(in_off + len(data), dtype=torch.uint8, device="cuda")
    assert d_buf.data_ptr() % 4 == 0
    d_in = d_buf[in_off:]
    d_in.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    return d_in


def _run(ctx, case, mode, in_off=0, out_off=0, cap=None, d_in=None):
    """One async call.  mode: "framed", "final" (segment) or "nonfinal".
    -> (the output buffer's bytes from its first canary byte, raw length
    word, where the stream starts in them)"""
    import torch
    d_in = _device_input(case.data, in_off) if d_in is None else d_in
    size = PAD + out_off + _bound(case.nb) + 64
    d_buf = torch.full((size,), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = d_buf[PAD + out_off:]
    cap = _bound(case.nb) if cap is None else cap
    d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    if mode == "framed":
        rc = ctx.compress_async(d_in, case.n, d_out, cap, d_len)
    else:
        rc = ctx.compress_segment_async(d_in, case.n, d_out, cap, d_len, mode == "final")
    assert rc == 0, (ctx.name, mode, rc)
    torch.cuda.synchronize()
    return d_buf.cpu().numpy(), int(d_len.item()) & (2 ** 64 - 1), PAD + out_off


def _verify(ctx, case, mode, buf, word, start, cap=None):
    """Everything the call left behind, against the oracle; a mismatch names
    the first differing block and the chunk it lies in."""
    hdr = 1 if mode == "framed" else 0
    want = np.frombuffer(case.framed() if hdr else case.body(), np.uint8)
    per = lz4_chunk_lib.chunk_blocks(ctx.name)
    what = f"{ctx.name}, {case.nb} blocks ({-(-case.nb // per)} chunks), {mode}"

    def where(b):
        return f"{what}: block {b} (block {b % per} of chunk {b // per})"
    assert word >> 63 == 0, f"{what}: bit 63 of the length word (a corrupt bucket head)"
    offs, sizes = ctx.block_offsets(case.nb).astype(np.int64), ctx.block_sizes(case.nb)
    want_offs, want_sizes = case.offsets(), case.sizes()
    bad = np.flatnonzero(sizes != want_sizes)
    assert not bad.size, f"{where(int(bad[0]) if bad.size else 0)}: size {sizes[bad[:1]]}, want " \
                         f"{want_sizes[bad[:1]]}"
    bad = np.flatnonzero(offs != want_offs)
    assert not bad.size, f"{where(int(bad[0]) if bad.size else 0)}: offset {offs[bad[:1]]}, want " \
                         f"{want_offs[bad[:1]]}"
    assert word == want.size, f"{what}: length word {word}, want {want.size}"
    written = min(want.size, want.size if cap is None else cap)
    got = buf[start:start + written]
    bad = np.flatnonzero(got != want[:written])
    if bad.size:
        i = int(bad[0])
        b = int(np.searchsorted(want_offs + hdr, i, side="right")) - 1
        raise AssertionError(f"{where(max(b, 0))}: stream byte {i} is {got[i]:#x}, want "
                             f"{want[i]:#x} ({bad.size} bytes differ)")
    assert (buf[:start] == 0xEE).all(), f"{what}: bytes before the output were written"
    past = np.flatnonzero(buf[start + written:] != 0xEE)
    assert not past.size, f"{what}: byte {written + int(past[0]) if past.size else 0} at or " \
                          f"past the {'capacity' if cap is not None else 'length'} was written"
    assert ctx.check() == 0, what


def _check(ctx, case, mode, **kw):
    buf, word, start = _run(ctx, case, mode, **kw)
    _verify(ctx, case, mode, buf, word, start, kw.get("cap"))


@pytest.fixture(scope="module")
def three(oracle, contents):
    return Case(oracle, contents[0], *THREE)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SIZES)), ids=[f"{nb}x{ln}" for nb, ln in SIZES])
def test_sizes(ctx, oracle, contents, i):
    nb, last_n = SIZES[i]
    case = Case(oracle, contents[i % 5], nb, last_n)
    _check(ctx, case, "framed")
    _check(ctx, case, "final")
    if last_n == BLK:
        _check(ctx, case, "nonfinal")


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(5))
def test_block_types_at_the_boundaries(ctx, oracle, contents, j):
    case = Case(oracle, contents[j], *THREE)
    _check(ctx, case, "framed")
    _check(ctx, case, "final")


@pytest.mark.gpu
@pytest.mark.parametrize("in_off", [1, 2, 3])
def test_unaligned_input(ctx, oracle, contents, in_off):
    # every block of every chunk is staged
    case = Case(oracle, contents[in_off], *THREE)
    _check(ctx, case, "framed", in_off=in_off)


@pytest.mark.gpu
@pytest.mark.parametrize("out_off", [1, 15])
def test_unaligned_output(ctx, three, out_off):
    _check(ctx, three, "framed", out_off=out_off)
    _check(ctx, three, "final", out_off=out_off)


def _caps(case):
    offs = 1 + case.offsets()                    # stream offsets of the blocks (framed)
    at_c, full = int(offs[C]), len(case.framed())
    caps = [at_c - 1, at_c, at_c + 1, int(offs[C + C // 2]) + 7, int(offs[2 * C + 10]) + 5,
            full - 1, full]
    assert caps == sorted(caps) and int(offs[2 * C]) < caps[4] < full - 1
    assert caps[2] < caps[3] < int(offs[2 * C])
    return caps


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(7))
def test_capacity(ctx, three, k):
    import torch
    cap = _caps(three)[k]
    full = len(three.framed())
    # async: every byte below cap, nothing at or past it, the full length
    buf, word, start = _run(ctx, three, "framed", cap=cap)
    _verify(ctx, three, "framed", buf, word, start, cap)
    # lz4r_compress_device: the same bytes, and the need in *out_len
    d_in = _device_input(three.data)
    d_buf = torch.full((PAD + _bound(three.nb),), 0xEE, dtype=torch.uint8, device="cuda")
    rc, need = ctx.compress_device(d_in, three.n, d_buf[PAD:], cap)
    assert need == full
    assert rc == (0 if cap >= full else -3), rc          # LZ4R_ERR_CAPACITY
    _verify(ctx, three, "framed", d_buf.cpu().numpy(), need, PAD, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("name", lz4_chunk_lib.NAMES)
def test_one_context_over_changing_sizes(gpu, oracle, contents, name):
    """Scratch that grows, cap_slots capped at a chunk, slots holding the
    records of another chunk or another call."""
    assert lz4_chunk_lib.chunk_blocks(name) == lz4_chunk_lib.expected_chunk_blocks(name)
    c = lz4_chunk_lib.Ctx(name)
    try:
        small = Case(oracle, contents[1], 100, BLK)
        for case in (small, Case(oracle, contents[1], *THREE), small,
                     Case(oracle, contents[2], C + 1, BLK), Case(oracle, contents[4], *THREE)):
            _check(c, case, "framed")
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", lz4_chunk_lib.NAMES)
def test_timing_of_chunked_calls(gpu, oracle, contents, three, name):
    import torch
    assert lz4_chunk_lib.chunk_blocks(name) == lz4_chunk_lib.expected_chunk_blocks(name)
    c = lz4_chunk_lib.Ctx(name)
    try:
        assert c.set_timing(True) == 0
        _check(c, three, "framed")
        _check(c, Case(oracle, contents[2], C + 1, 24), "final")
        ms_call, ms_match = c.timed_calls()
        assert len(ms_call) == len(ms_match) == 2
        for a, b in zip(ms_call, ms_match):
            assert 0 < b <= a, (ms_call, ms_match)
        # an empty final segment: a timed call of no launches
        d_in = _device_input(three.data[:BLK])
        d_out = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
        d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert c.compress_segment_async(d_in, 0, d_out, 64, d_len, True) == 0
        torch.cuda.synchronize()
        assert int(d_len.item()) == 0 and bool((d_out == 0xEE).all())
        ms_call, ms_match = c.timed_calls()
        assert len(ms_call) == len(ms_match) == 3 and ms_match[2] == 0, (ms_call, ms_match)
        assert c.check() == 0
    finally:
        c.close()


@pytest.mark.gpu
def test_chunked_stream_decodes(ctx, three):
    """The framed three-chunk stream and the context's own device block
    offsets, through the product's block-parallel decoder."""
    import torch
    from lz4jpeg import lz4
    buf, word, start = _run(ctx, three, "framed")
    _verify(ctx, three, "framed", buf, word, start)
    d_stream = torch.from_numpy(buf[start:start + word].copy()).cuda()
    optr, cnt = ctx.block_offsets_device()
    assert cnt == three.nb
    d_back, n = lz4.decompress_device(d_stream, word, optr, three.nb, three.n + BLK)
    assert n == three.n
    assert d_back[:n].cpu().numpy().tobytes() == three.data


@pytest.mark.gpu
@pytest.mark.parametrize("name", lz4_chunk_lib.NAMES)
def test_block_matches_second_launch(gpu, oracle, contents, types, name):
    """lz4r_block_matches_device cuts its launches like run(): 300 (C + 2) - 150
    bytes are a chunk and a second launch of two blocks, the last one short."""
    import torch
    assert lz4_chunk_lib.chunk_blocks(name) == lz4_chunk_lib.expected_chunk_blocks(name)
    n = BLK * (C + 2) - 150
    data = bytearray(contents[2].data[:n])         # types at C - 2 .. C + 1, text around them
    data[:5 * BLK] = b"".join(types[0])
    data = bytes(data)
    want = oracle.lz4_block_matches(data)
    assert want[BLK * C:].any() and want[:BLK * C].any()
    d_in = _device_input(data)
    d_m = torch.full((n + 64,), -1, dtype=torch.int32, device=gpu)
    assert lz4_chunk_lib.block_matches_device(name, d_in, n, d_m) == 0
    torch.cuda.synchronize()
    got = d_m.cpu().numpy().view(np.uint32)
    assert (got[n:] == 0xFFFFFFFF).all(), "entries past n - 1 were written"
    bad = np.flatnonzero(got[:n] != want)
    per = lz4_chunk_lib.chunk_blocks(name)
    assert not bad.size, (f"{name}: {bad.size} entries differ, first at block "
                          f"{bad[0] // BLK} (launch {bad[0] // BLK // per}) position "
                          f"{bad[0] % BLK}: got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")
