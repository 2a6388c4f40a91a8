"""lz4_tiles over runs of blocks: what one block leaves behind is what the
next block of the run starts from.

A wave encodes a run of consecutive blocks (kTileRun, csrc/lz4r_layout.h) in
one loop over one LDS allocation, and loads the next block's dwords while it
is still busy with the current one.  A one-block workgroup never had a
predecessor; here every case compares, against the oracle encoder on the same
bytes, the whole stream byte for byte, the length word (bit 63 clear) and the
device block offsets.

- run boundaries: every block count 1 .. 4 * 16 + 6 (runs of up to 16 that
  end early, end exactly, or spill one block over) crossed with the last
  block's length 1, 23, 24, 299, 300 (23 / 24: whether the block BEFORE the
  last may be read unstaged, i.e. whether it may be prefetched), plus one
  input per count that is not 4-byte aligned (the staged instantiation);
- hostile neighbours: five block types in every ordered pair at every
  position of a run of up to 16 (a de Bruijn cycle of the pairs, repeated at
  a stride coprime to the run length), framed and through the segment API.
"""
import numpy as np
import pytest

import golden_inputs

pytestmark = pytest.mark.gpu

BLK = 300
MAX_RUN = 16                      # the largest run length the A/B considered
COUNTS = range(1, 4 * MAX_RUN + 6 + 1)
LAST_N = (1, 23, 24, 299, 300)


@pytest.fixture(scope="module")
def comp(gpu):
    from lz4jpeg.lz4 import Compressor
    c = Compressor()
    yield c
    c.close()


@pytest.fixture(scope="module")
def text():
    t = golden_inputs.lz4_input("metamorphosis_spaces")
    assert len(t) >= BLK * COUNTS[-1]
    return t


class Expected:
    """The oracle's per-block encodings of one input, computed once."""

    def __init__(self, oracle, data):
        self.data = bytes(data)
        buf = np.frombuffer(self.data, dtype=np.uint8)
        self.nb = (len(self.data) + BLK - 1) // BLK
        self.blocks = [oracle.lz4_blocks(buf, b, b + 1) for b in range(self.nb)]

    def offsets(self):
        return np.concatenate(([0], np.cumsum([len(b) for b in self.blocks])[:-1])).astype(np.uint64)

    def body(self):
        return b"".join(self.blocks)

    def framed(self):
        return bytes([self.nb & 0xFF]) + self.body()


@pytest.fixture(scope="module")
def text_blocks(oracle, text):
    """Oracle encodings of the text's full blocks 0 .. COUNTS[-1] - 1 (shared:
    every run-boundary input is a prefix of the same text)."""
    return Expected(oracle, text[:BLK * COUNTS[-1]]).blocks


def _compress(comp, data, misalign=0, segment=False, final_shard=None):
    """compress_async of `data` placed `misalign` bytes into a fresh device
    buffer -> (stream bytes, raw length word, device block offsets)."""
    import torch
    from lz4jpeg.lz4 import compress_bound
    n = len(data)
    d_buf = torch.empty(misalign + n, dtype=torch.uint8, device="cuda")
    assert d_buf.data_ptr() % 4 == 0
    d_in = d_buf[misalign:]
    d_in.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    d_out = torch.full((compress_bound(n),), 0xEE, dtype=torch.uint8, device="cuda")
    d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    comp.compress_async(d_in, n, d_out, d_len, segment=segment, final_shard=final_shard)
    torch.cuda.synchronize()
    word = int(d_len.item())
    assert word >= 0, "bit 63 of the length word: a corrupt bucket head"
    nb = (n + BLK - 1) // BLK
    return d_out[:word].cpu().numpy().tobytes(), word, comp.block_offsets(nb)


def _check_text(comp, oracle, text, text_blocks, count, last_n, misalign=0):
    n = BLK * (count - 1) + last_n
    data = bytes(text[:n])
    last = text_blocks[count - 1] if last_n == BLK else oracle.lz4_blocks(
        np.frombuffer(data, dtype=np.uint8), count - 1, count)
    blocks = text_blocks[:count - 1] + [last]
    # an input shorter than one block has no framed form: a final segment
    seg = n < BLK
    want = b"".join(blocks) if seg else bytes([count & 0xFF]) + b"".join(blocks)
    got, word, offs = _compress(comp, data, misalign, segment=seg, final_shard=True if seg else None)
    where = (count, last_n, misalign)
    assert word == len(want), where
    assert got == want, where
    want_offs = np.concatenate(([0], np.cumsum([len(b) for b in blocks])[:-1]))
    assert np.array_equal(offs.astype(np.int64), want_offs), where


@pytest.mark.parametrize("count", COUNTS)
def test_run_boundaries(comp, oracle, text, text_blocks, count):
    for last_n in LAST_N:
        _check_text(comp, oracle, text, text_blocks, count, last_n)
    # not 4-byte aligned: every block of the run is staged, none prefetched
    _check_text(comp, oracle, text, text_blocks, count, LAST_N[count % len(LAST_N)],
                misalign=1 + count % 3)


def _block_types(text):
    rng = np.random.default_rng(77)
    pre = bytes(rng.permutation(256)[:40].astype(np.uint8))
    many = bytearray(pre)
    while len(many) < BLK:
        s = int(rng.integers(0, len(pre) - 4))
        many += pre[s:s + 4]
    return [
        b"\x5a" * BLK,                                    # matches of >= 256 bytes
        b"ab" * (BLK // 2),                               # period 2: the longest chains
        rng.integers(0, 256, BLK, dtype=np.uint8).tobytes(),   # no match: 300 literals
        bytes(text[9000:9000 + BLK]),                     # text
        bytes(many[:BLK]),                                # exact-4 matches back to back
    ]


def _de_bruijn_pairs(k):
    """A cyclic order of 0 .. k - 1 (length k * k) in which every ordered pair
    (a, b), a == b included, is adjacent exactly once: an Euler circuit of the
    complete digraph with loops (Hierholzer)."""
    nxt = {a: list(range(k)) for a in range(k)}
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            out.append(stack.pop())
    seq = out[::-1][:-1]
    assert len(seq) == k * k
    assert {(seq[i], seq[(i + 1) % len(seq)]) for i in range(len(seq))} == {
        (a, b) for a in range(k) for b in range(k)}
    return seq


@pytest.fixture(scope="module")
def hostile(oracle, text):
    """Every ordered pair of the five block types at every position of a run
    of up to MAX_RUN blocks: the 25-block pair cycle, closed by its first
    block and padded to 27 blocks (coprime to any power-of-two run length),
    MAX_RUN times."""
    types = _block_types(text)
    enc = [oracle.lz4_blocks(np.frombuffer(t, dtype=np.uint8), 0, 1) for t in types]
    # block header: u8 sequence count, u16 size (LZ4.c:415-425)
    assert enc[4][0] > 23, "the overflow slot (records 23..) is not exercised"
    assert enc[2][0] == 1 and len(enc[2]) > BLK, "the random block must be one literal run"
    cyc = _de_bruijn_pairs(len(types))
    period = cyc + [cyc[0], 3]
    assert len(period) == 27
    order = period * MAX_RUN
    pos = {(order[i], order[i + 1], i % MAX_RUN) for i in range(len(order) - 1)}
    assert all((a, b, p) in pos for a in range(5) for b in range(5) for p in range(MAX_RUN))
    return Expected(oracle, b"".join(types[i] for i in order))


def _check(comp, exp, want, **kw):
    got, word, offs = _compress(comp, exp.data, **kw)
    assert word == len(want)
    assert got == want
    assert np.array_equal(offs, exp.offsets())


def test_hostile_neighbours_framed(comp, hostile):
    _check(comp, hostile, hostile.framed())


@pytest.mark.parametrize("final_shard", [False, True])
def test_hostile_neighbours_segment(comp, hostile, final_shard):
    _check(comp, hostile, hostile.body(), segment=True, final_shard=final_shard)
