"""lz4_tiles' shared records round: the records of several blocks of a run
wait in one register and leave in one round (csrc/lz4r_tiles.h, RecBatch).

Every case compares, against the oracle's per-block encodings of the same
bytes, the whole stream byte for byte, the length word (bit 63 clear), the
device block offsets and, where the accessor exists, Compressor.block_sizes.
What a case covers is asserted from the oracle's own encoding (byte 0 of a
block = its sequence count), never from the code under test.

A run is the 16 consecutive blocks [16 r, 16 r + 16) of an input (kTileRun;
the host deals whole runs to the XCDs), so a scenario -- a list of blocks with
given sequence counts -- is placed at the start of a run of its own and padded
with text blocks; many scenarios make one input.

- fill levels: a pending fill c and a next block of k sequences with c + k =
  60 .. 66 (fits, fits exactly, overflows and falls back -- wherever the
  implementation draws the line near 64 lanes), c around every flush
  threshold considered (32 .. 44), blocks of 62 .. 65 sequences alone and on
  a non-empty batch (65: the redone walk through the LDS), four and more
  one-sequence blocks in a row;
- mixed forms: a block with a truncated match (M = len & 0xFF, M = 0 .. 4
  included) and a block with an overflow slot (> 23 sequences) at every
  position of a batch, beside text and beside exact-4 blocks;
- edges of the run: block counts 1, 2, 15, 16, 17, 33 with last-block lengths
  1, 23, 24, 300, one input that is not 4-byte aligned, framed and through
  the segment API.
"""
import numpy as np
import pytest

import golden_inputs

pytestmark = pytest.mark.gpu

BLK = 300
RUN = 16
THRESHOLDS = (32, 36, 38, 40, 44)     # the flush thresholds the A/B considered


# ---- blocks with a given number of sequences ---------------------------------

def block_exact(k, seed=0):
    """A block of exactly k sequences, k = 1 .. 53: 40 distinct bytes, then
    k - 1 copies of 4-grams of them, each followed by a byte value used nowhere
    else (every match is exactly 4 long), then unused values as the tail."""
    assert 1 <= k <= 53
    rng = np.random.default_rng(1000 + 64 * seed + k)
    vals = [int(v) for v in rng.permutation(256)]
    pre, unused = vals[:40], vals[40:]
    out = list(pre)
    for i in range(k - 1):
        s = (5 * i) % 37
        out += pre[s:s + 4] + [unused.pop()]
    pad = BLK - len(out)
    u = len(unused)
    assert pad <= u + u // 2
    # second pass at stride 2: no pair of the first pass comes back
    out += unused[:pad] + [unused[(2 * i + 1) % u] for i in range(max(0, pad - u))]
    assert len(out) == BLK
    return bytes(out)


def _block_dense(seed):
    rng = np.random.default_rng(seed)
    p = int(rng.integers(36, 64))
    pre = [int(v) for v in rng.permutation(256)[:p]]
    out = list(pre)
    while len(out) < BLK:
        s = int(rng.integers(0, p - 3))
        out += pre[s:s + 4]
    return bytes(out[:BLK])


def block_trunc(length):
    """20 distinct bytes, a run of length + 1 equal bytes (a match of `length`
    bytes, of which the encoder keeps length & 0xFF), distinct bytes."""
    vals = [v for v in range(256) if v != 0x5A]
    rest = BLK - 20 - (length + 1)
    assert rest >= 0
    return bytes(vals[:20]) + b"\x5a" * (length + 1) + bytes(vals[100:100 + rest])


def nseq(oracle, blk):
    return oracle.lz4_blocks(np.frombuffer(blk, dtype=np.uint8), 0, 1)[0]


@pytest.fixture(scope="module")
def blocks(oracle):
    """{sequence count: block} for 1 .. 65, each count asserted on the oracle."""
    by = {}
    for k in range(1, 54):
        by[k] = block_exact(k)
        assert nseq(oracle, by[k]) == k, k
    for seed in range(400):
        b = _block_dense(seed)
        by.setdefault(nseq(oracle, b), b)
    assert all(k in by for k in range(54, 66)), sorted(k for k in by if k > 53)
    return by


@pytest.fixture(scope="module")
def text():
    return golden_inputs.lz4_input("metamorphosis_spaces")


@pytest.fixture(scope="module")
def comp(gpu):
    from lz4jpeg.lz4 import Compressor
    c = Compressor()
    yield c
    c.close()


class Expected:
    """The oracle's per-block encodings of one input, computed once."""

    def __init__(self, oracle, data):
        self.data = bytes(data)
        buf = np.frombuffer(self.data, dtype=np.uint8)
        self.nb = (len(self.data) + BLK - 1) // BLK
        self.blocks = [oracle.lz4_blocks(buf, b, b + 1) for b in range(self.nb)]

    def counts(self):
        return [b[0] for b in self.blocks]

    def sizes(self):
        return np.array([len(b) for b in self.blocks], dtype=np.int64)

    def offsets(self):
        return np.concatenate(([0], np.cumsum(self.sizes())[:-1]))

    def body(self):
        return b"".join(self.blocks)

    def framed(self):
        return bytes([self.nb & 0xFF]) + self.body()


def _compress(comp, data, misalign=0, segment=False, final_shard=None):
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
    sizes = None
    if hasattr(comp, "block_sizes"):
        sizes = np.asarray(comp.block_sizes(nb)).astype(np.int64)
    return d_out[:word].cpu().numpy().tobytes(), word, comp.block_offsets(nb), sizes


def _check(comp, exp, framed=True, where=None, **kw):
    want = exp.framed() if framed else exp.body()
    got, word, offs, sizes = _compress(comp, exp.data, **kw)
    assert word == len(want), where
    if got != want:
        # the first block that differs, by the oracle's offsets
        o = exp.offsets() + (1 if framed else 0)
        bad = next(b for b in range(exp.nb)
                   if got[o[b]:o[b] + len(exp.blocks[b])] != exp.blocks[b])
        raise AssertionError((where, "block", bad, "of", exp.nb, "counts", exp.counts()[
            max(0, bad - 4):bad + 2]))
    assert np.array_equal(offs.astype(np.int64), exp.offsets()), where
    if sizes is not None:
        assert np.array_equal(sizes, exp.sizes()), where


def _runs(scenarios, text):
    """Each scenario at the start of a run of its own, padded with text."""
    out, pos, full = [], 0, len(text) // BLK
    for sc in scenarios:
        assert len(sc) <= RUN
        out += list(sc)
        for _ in range(RUN - len(sc)):
            out.append(bytes(text[BLK * pos:BLK * (pos + 1)]))
            pos = (pos + 1) % full
    return b"".join(out)


def _scenario_input(oracle, blocks, text, plans):
    """plans: lists of sequence counts (ints) or ready blocks (bytes)."""
    scen = [[blocks[x] if isinstance(x, int) else x for x in plan] for plan in plans]
    exp = Expected(oracle, _runs(scen, text))
    got = exp.counts()
    for r, plan in enumerate(plans):
        for i, x in enumerate(plan):
            if isinstance(x, int):
                assert got[RUN * r + i] == x, (r, i, x, got[RUN * r + i])
    return exp


# ---- 1. fill levels -----------------------------------------------------------

@pytest.mark.parametrize("total", range(60, 67))   # around the 64 lanes of the register
def test_fill_near_64_lanes(comp, oracle, blocks, text, total):
    plans = [[c, total - c] for c in (20, 31, 38)]
    plans.append([12, 12, total - 24])
    plans.append([5, 7, 9, total - 21])
    exp = _scenario_input(oracle, blocks, text, plans)
    _check(comp, exp, where=total)


@pytest.mark.parametrize("T", THRESHOLDS)
def test_fill_around_threshold(comp, oracle, blocks, text, T):
    plans = []
    for c in range(T - 2, T + 4):                # just below .. just above
        plans.append([c, 12, 12])
        plans.append([c // 2, c - c // 2, 12])
        plans.append([1, c - 1, 30])
    exp = _scenario_input(oracle, blocks, text, plans)
    _check(comp, exp, where=T)


@pytest.mark.parametrize("k", range(60, 66))       # 65: more sequences than lanes
def test_large_blocks_alone_and_on_a_batch(comp, oracle, blocks, text, k):
    plans = [[k], [10, k], [30, k, 3], [1, 1, 1, k, 20], [k, k]]
    exp = _scenario_input(oracle, blocks, text, plans)
    assert exp.counts()[0] == k
    _check(comp, exp, where=k)


def test_tiny_blocks(comp, oracle, blocks, text):
    rng = np.random.default_rng(5)
    rnd = [rng.integers(0, 256, BLK, dtype=np.uint8).tobytes() for _ in range(RUN)]
    for b in rnd:
        enc = oracle.lz4_blocks(np.frombuffer(b, dtype=np.uint8), 0, 1)
        # one literal run of 300: the L = 270-style extension bytes
        assert enc[0] == 1 and len(enc) > BLK
    plans = [rnd[:4], rnd[:5], rnd[:9], rnd[:RUN], rnd[:3] + [40], rnd[:4] + [50],
             [1] * 4, [1] * 7 + [2] * 6, [2, 1, 3, 1, 2, 1, 60]]
    exp = _scenario_input(oracle, blocks, text, plans)
    _check(comp, exp)


# ---- 2. mixed forms in one batch ------------------------------------------------

@pytest.mark.parametrize("length", (300, 256, 257, 258, 259, 260))
def test_truncated_match_in_a_batch(comp, oracle, blocks, text, length):
    """length: of the match the encoder truncates to length & 0xFF (300: the
    whole block one byte value; 256: M = 0, a literal; 257 .. 259: M = 1 .. 3,
    a size field that counts a byte nobody writes)."""
    t = b"\x5a" * BLK if length == BLK else block_trunc(length)
    many = blocks[30]                            # exact-4 matches, overflow slot
    txt = [bytes(text[9000 + BLK * i:9000 + BLK * (i + 1)]) for i in range(2)]
    plans = []
    for pos in range(4):                         # first, middle, last of a batch of four
        small = [4, 5, 6]
        plans.append(small[:pos] + [t] + small[pos:])
    plans += [[t, txt[0], txt[1]], [txt[0], t, txt[1]], [txt[0], txt[1], t], [t, many], [many, t],
              [8, t, many], [t, t, t, t, t]]
    exp = _scenario_input(oracle, blocks, text, plans)
    _check(comp, exp, where=length)


@pytest.mark.parametrize("big", (24, 25, 29))
def test_overflow_slot_at_each_batch_position(comp, oracle, blocks, text, big):
    txt = [bytes(text[6000 + BLK * i:6000 + BLK * (i + 1)]) for i in range(3)]
    plans = []
    for pos in range(4):
        small = [3, 4, 4]
        plans.append(small[:pos] + [big] + small[pos:])
    plans += [[big, big], [big, 2, big], [txt[0], big], [big, txt[1]], [2, txt[2], big],
              [23, 23, 2], [22, 24, 2]]            # 23: the last record of the head
    exp = _scenario_input(oracle, blocks, text, plans)
    _check(comp, exp, where=big)


# ---- 3. edges of the run --------------------------------------------------------

@pytest.fixture(scope="module")
def text_blocks(oracle, text):
    return Expected(oracle, text[:BLK * 33]).blocks


def _text_case(oracle, text, text_blocks, count, last_n):
    n = BLK * (count - 1) + last_n
    exp = Expected.__new__(Expected)
    exp.data = bytes(text[:n])
    exp.nb = count
    last = text_blocks[count - 1] if last_n == BLK else oracle.lz4_blocks(
        np.frombuffer(exp.data, dtype=np.uint8), count - 1, count)
    exp.blocks = text_blocks[:count - 1] + [last]
    return exp


@pytest.mark.parametrize("count", (1, 2, 15, 16, 17, 33))
def test_run_edges(comp, oracle, text, text_blocks, count):
    for last_n in (1, 23, 24, 300):
        exp = _text_case(oracle, text, text_blocks, count, last_n)
        if len(exp.data) < BLK:                  # no framed form: a final segment
            _check(comp, exp, framed=False, where=(count, last_n), segment=True, final_shard=True)
            continue
        _check(comp, exp, where=(count, last_n))
        _check(comp, exp, framed=False, where=(count, last_n, "final"), segment=True,
               final_shard=True)
        if last_n == BLK:                        # a non-final shard is whole blocks
            _check(comp, exp, framed=False, where=(count, "shard"), segment=True,
                   final_shard=False)


def test_unaligned_input(comp, oracle, blocks, text):
    """Not 4-byte aligned: every block is staged and leaves alone."""
    exp = _scenario_input(oracle, blocks, text, [[20, 43, 3], [65, 1, 1], [b"\x5a" * BLK, 30]])
    for mis in (1, 2, 3):
        _check(comp, exp, where=mis, misalign=mis)
