"""lz4_tiles' shared records round: the records of several blocks of a run
wait in one register and leave in one round (csrc/lz4r_tiles.h, RecBatch).

Every case compares, against the oracle's per-block encodings of the same
bytes, the whole stream byte for byte, the length word (bit 63 clear), the
device block offsets and sizes (lz4_gpu_lib.check).  What a case covers is
asserted from the oracle's own encoding (byte 0 of a block = its sequence
count), never from the code under test.

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
import lz4_gpu_lib
from lz4_gpu_lib import check
from lz4_seq_inputs import BLK, Expected, block_trunc, blocks_by_count, planned_input

pytestmark = pytest.mark.gpu

RUN = 16
THRESHOLDS = (32, 36, 38, 40, 44)     # the flush thresholds the A/B considered


@pytest.fixture(scope="module")
def blocks(oracle):
    """{sequence count: block} for 1 .. 65, each count asserted on the oracle."""
    return blocks_by_count(oracle)


@pytest.fixture(scope="module")
def text():
    return golden_inputs.lz4_input("metamorphosis_spaces")


@pytest.fixture(scope="module")
def comp(gpu):
    yield from lz4_gpu_lib.compressor()


def _scenario_input(oracle, blocks, text, plans):
    """plans: lists of sequence counts (ints) or ready blocks (bytes), each at
    the start of a run of its own, padded with text."""
    return planned_input(oracle, blocks, text, plans, RUN, pad_last=True)


# ---- 1. fill levels -----------------------------------------------------------

@pytest.mark.parametrize("total", range(60, 67))   # around the 64 lanes of the register
def test_fill_near_64_lanes(comp, oracle, blocks, text, total):
    plans = [[c, total - c] for c in (20, 31, 38)]
    plans.append([12, 12, total - 24])
    plans.append([5, 7, 9, total - 21])
    exp = _scenario_input(oracle, blocks, text, plans)
    check(comp, exp, where=total)


@pytest.mark.parametrize("T", THRESHOLDS)
def test_fill_around_threshold(comp, oracle, blocks, text, T):
    plans = []
    for c in range(T - 2, T + 4):                # just below .. just above
        plans.append([c, 12, 12])
        plans.append([c // 2, c - c // 2, 12])
        plans.append([1, c - 1, 30])
    exp = _scenario_input(oracle, blocks, text, plans)
    check(comp, exp, where=T)


@pytest.mark.parametrize("k", range(60, 66))       # 65: more sequences than lanes
def test_large_blocks_alone_and_on_a_batch(comp, oracle, blocks, text, k):
    plans = [[k], [10, k], [30, k, 3], [1, 1, 1, k, 20], [k, k]]
    exp = _scenario_input(oracle, blocks, text, plans)
    assert exp.counts()[0] == k
    check(comp, exp, where=k)


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
    check(comp, exp)


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
    check(comp, exp, where=length)


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
    check(comp, exp, where=big)


# ---- 3. edges of the run --------------------------------------------------------

@pytest.fixture(scope="module")
def text_blocks(oracle, text):
    return Expected(oracle, text[:BLK * 33]).blocks


@pytest.mark.parametrize("count", (1, 2, 15, 16, 17, 33))
def test_run_edges(comp, oracle, text, text_blocks, count):
    for last_n in (1, 23, 24, 300):
        exp = Expected.of_text_prefix(oracle, text, text_blocks, count, last_n)
        if len(exp.data) < BLK:                  # no framed form: a final segment
            check(comp, exp, framed=False, where=(count, last_n), segment=True, final_shard=True)
            continue
        check(comp, exp, where=(count, last_n))
        check(comp, exp, framed=False, where=(count, last_n, "final"), segment=True,
               final_shard=True)
        if last_n == BLK:                        # a non-final shard is whole blocks
            check(comp, exp, framed=False, where=(count, "shard"), segment=True,
                   final_shard=False)


def test_unaligned_input(comp, oracle, blocks, text):
    """Not 4-byte aligned: every block is staged and leaves alone."""
    exp = _scenario_input(oracle, blocks, text, [[20, 43, 3], [65, 1, 1], [b"\x5a" * BLK, 30]])
    for mis in (1, 2, 3):
        check(comp, exp, where=mis, misalign=mis)
