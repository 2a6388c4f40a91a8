"""The placement scan over the u16 block sizes (csrc/lz4r_scan.h,
lz4_scan_reduce16 and lz4_scan_partials_frame): a workgroup reduces one partial
of 4096 sizes (64 groups of 64, eight sizes per 16-B load, a group on eight
lanes), one workgroup scans the partials, writes the length word and, on a
framed call, the frame byte.  lz4_tiles stores the sizes once, as u16; the
scan, lz4_emit and lz4r_copy_block_sizes all read that array.

Every case compares, against the oracle's per-block encodings of the same
bytes, the whole stream (frame byte included), the length word (bit 63 clear),
lz4r_copy_block_sizes and the device block offsets (lz4_gpu_lib.check; on the
chunk12 build, whose context lz4_gpu_lib does not drive, the same comparisons
are spelled out here).

- block counts 1, 63, 64, 65, 4095, 4096, 4097 and 2 * 4096 + 1: one group,
  one partial, and one block either side of each; framed and as segments,
  with a whole and a 23-byte last block (the reduce's tail loads);
- calls of different sizes back to back on one context;
- the chunk12 build (launch chunks of 4096 blocks) on 2 * 4096 + 1 blocks: two
  chunk boundaries, the second and third scan continuing from the length word,
  every launch given its chunk's own bases;
- one length buffer reused across calls, on both builds.
"""
import numpy as np
import pytest

import golden_inputs
import lz4_chunk_lib
import lz4_gpu_lib
from lz4_gpu_lib import check
from lz4_seq_inputs import BLK, Expected

pytestmark = pytest.mark.gpu

PART = 4096                                    # blocks per scan partial (= chunk12's chunk)
COUNTS = (1, 63, 64, 65, PART - 1, PART, PART + 1, 2 * PART + 1)
assert max(COUNTS) * BLK < 3 << 20


@pytest.fixture(scope="module")
def book(oracle):
    """The book, repeated, as 2 * 4096 + 1 whole blocks, encoded once."""
    text = golden_inputs.lz4_input("metamorphosis_spaces")
    assert len(text) % BLK != 0, "the blocks must differ from lap to lap"
    nb = max(COUNTS)
    data = (text * (nb * BLK // len(text) + 1))[:nb * BLK]
    return data, Expected(oracle, data).blocks


def _case(oracle, book, nb, last_n=BLK):
    data, blocks = book
    exp = Expected(oracle, data[:BLK * (nb - 1) + last_n], known=blocks)
    assert exp.nb == nb
    return exp


@pytest.fixture(scope="module")
def comp(gpu):
    yield from lz4_gpu_lib.compressor()


@pytest.mark.parametrize("nb", COUNTS)
def test_block_counts(comp, oracle, book, nb):
    exp = _case(oracle, book, nb)
    check(comp, exp, where=(nb, "framed"))
    check(comp, exp, framed=False, where=(nb, "final"), segment=True, final_shard=True)
    check(comp, exp, framed=False, where=(nb, "shard"), segment=True, final_shard=False)
    short = _case(oracle, book, nb, 23)
    if nb > 1:                                   # (a framed call needs a whole block)
        check(comp, short, where=(nb, 23, "framed"))
    check(comp, short, framed=False, where=(nb, 23, "final"), segment=True, final_shard=True)


def test_calls_in_a_row_on_one_context(gpu, oracle, book):
    """Large, small, large: the scans of 3, 1, 2 and 3 workgroups one after
    the other, over sizes, group sums and partials the call before left."""
    from lz4jpeg.lz4 import Compressor
    c = Compressor()
    try:
        for nb in (2 * PART + 1, 1, PART + 1, 64, 2 * PART + 1, 65):
            exp = _case(oracle, book, nb)
            check(c, exp, where=nb)
            check(c, exp, framed=False, where=(nb, "segment"), segment=True, final_shard=True)
    finally:
        c.close()


def _device(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


def test_length_buffer_reused(comp, oracle, book):
    """The second call's scan starts from its own header, not from what the
    first left in the caller's length word."""
    import torch
    from lz4jpeg.lz4 import compress_bound
    d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    for nb, seg in ((PART + 1, False), (65, True), (2 * PART + 1, False), (1, True)):
        exp = _case(oracle, book, nb)
        want = exp.body() if seg else exp.framed()
        d_in = _device(exp.data)
        d_out = torch.full((compress_bound(len(exp.data)) + 64,), 0xEE, dtype=torch.uint8,
                           device="cuda")
        comp.compress_async(d_in, len(exp.data), d_out, d_len, segment=seg,
                            final_shard=True if seg else None)
        torch.cuda.synchronize()
        assert int(d_len.item()) == len(want), (nb, seg)
        got = d_out.cpu().numpy()
        assert got[:len(want)].tobytes() == want, (nb, seg)
        assert (got[len(want):] == 0xEE).all(), (nb, seg)
        assert np.array_equal(comp.block_offsets(nb).astype(np.int64), exp.offsets()), (nb, seg)
        assert np.array_equal(lz4_gpu_lib.block_sizes(comp, nb), exp.sizes()), (nb, seg)


# ---- the chunk12 build: a scan per launch chunk, continuing the length word ----

def _chunk_call(ctx, exp, mode, d_len):
    """One async call on a lz4_chunk_lib.Ctx, everything it left compared with
    the oracle; d_len: the caller's length word (whatever it holds)."""
    import torch
    want = exp.framed() if mode == "framed" else exp.body()
    n = len(exp.data)
    cap = 1 + exp.nb * 1152
    d_in = _device(exp.data)
    d_out = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    if mode == "framed":
        rc = ctx.compress_async(d_in, n, d_out, cap, d_len)
    else:
        rc = ctx.compress_segment_async(d_in, n, d_out, cap, d_len, mode == "final")
    assert rc == 0, (ctx.name, mode, rc)
    torch.cuda.synchronize()
    word = int(d_len.item()) & (2 ** 64 - 1)
    assert word >> 63 == 0, (ctx.name, mode, "bit 63 of the length word")
    assert word == len(want), (ctx.name, mode, exp.nb, word, len(want))
    assert ctx.check() == 0, (ctx.name, mode)
    got = d_out.cpu().numpy()
    assert got[:len(want)].tobytes() == want, (ctx.name, mode, exp.nb)
    assert (got[len(want):] == 0xEE).all(), (ctx.name, mode, exp.nb)
    assert np.array_equal(ctx.block_sizes(exp.nb), exp.sizes()), (ctx.name, mode, exp.nb)
    assert np.array_equal(ctx.block_offsets(exp.nb).astype(np.int64), exp.offsets()), (
        ctx.name, mode, exp.nb)


@pytest.mark.parametrize("name", lz4_chunk_lib.NAMES)
def test_two_chunk_boundaries_and_a_reused_length(gpu, oracle, book, name):
    import torch
    assert lz4_chunk_lib.chunk_blocks(name) == lz4_chunk_lib.expected_chunk_blocks(name)
    assert lz4_chunk_lib.chunk_blocks("chunk12") == PART
    c = lz4_chunk_lib.Ctx(name)
    try:
        d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        three = _case(oracle, book, 2 * PART + 1, 277)     # chunk12: three chunks
        assert -(-three.nb // PART) == 3
        for exp, mode in ((three, "framed"), (_case(oracle, book, PART), "nonfinal"),
                          (three, "final"), (_case(oracle, book, PART + 1, 1), "framed"),
                          (_case(oracle, book, 1), "final"), (three, "framed")):
            _chunk_call(c, exp, mode, d_len)
    finally:
        c.close()
