"""The edges of lz4_tiles' shared records round (csrc/lz4r_tiles.h, RecBatch,
flush_records): two consecutive unstaged blocks of a run leave in one round,
each on a half of the wave, a block's sequences and its tail lane on up to 32
lanes; the head's 24 dwords and the overflow slot are stored from those lanes,
the header dword and the u16 byte count by a two-lane store.

Every case compares, against the oracle's per-block encodings of the same
bytes, the whole stream, the length word, lz4r_copy_block_sizes and the device
block offsets (lz4_gpu_lib.check).  What a block is for is asserted from the
oracle's own encoding (byte 0 of a block = its sequence count).  A block whose
last sequence is its literal tail takes as many lanes as it has sequences; a
block that ends with a match (block_endmatch) takes one more, the tail lane
nobody uses.  Inputs have at most 33 blocks: one or two runs of 16.

- 30, 31 and 32 lanes (around what a half holds), in both forms, as the first
  and the second block of a pair and behind a block that waits;
- 22, 23 and 24 sequences at both positions: the head's last dword and the
  overflow slot's first;
- a pair of 1 and 31; a block with a truncated match at either position;
- a run whose last block waits with nobody after it;
- last blocks of 1, 23, 24 and 300 bytes; an unaligned input.
"""
import pytest

import golden_inputs
import lz4_gpu_lib
from lz4_gpu_lib import check
from lz4_seq_inputs import (BLK, Expected, block_endmatch, block_trunc, blocks_by_count, nseq,
                            planned_input)

pytestmark = pytest.mark.gpu

RUN = 16


@pytest.fixture(scope="module")
def blocks(oracle):
    return blocks_by_count(oracle)


@pytest.fixture(scope="module")
def endmatch(oracle):
    """{sequence count: a block of that many sequences, the last one a match
    that ends with the block} for 29 .. 31: 30 .. 32 lanes."""
    by = {}
    for k in range(28, 36):
        b = block_endmatch(k)
        by.setdefault(nseq(oracle, b), b)
    assert all(k in by for k in (29, 30, 31)), sorted(by)
    return by


@pytest.fixture(scope="module")
def text():
    return golden_inputs.lz4_input("metamorphosis_spaces")


@pytest.fixture(scope="module")
def comp(gpu):
    yield from lz4_gpu_lib.compressor()


def _inputs(oracle, blocks, text, plans, pad_last=True):
    """The plans two by two: inputs of at most 32 blocks."""
    for i in range(0, len(plans), 2):
        exp = planned_input(oracle, blocks, text, plans[i:i + 2], RUN, pad_last)
        assert exp.nb <= 33
        yield exp


def _positions(x, other=12):
    """x as the first and as the second block of a pair, twice in a pair,
    first behind a flushed pair, and second behind a block that waits."""
    return [[x, other], [other, x], [x, x], [3, 4, x, 6], [3, 4, 5, x, 6], [1, x, x, 1]]


@pytest.mark.parametrize("lanes", (30, 31, 32))
def test_fits_and_goes_alone(comp, oracle, blocks, endmatch, text, lanes):
    assert blocks[lanes][-1:] and nseq(oracle, blocks[lanes]) == lanes
    plans = _positions(lanes) + _positions(endmatch[lanes - 1])
    plans += [[lanes, endmatch[lanes - 1]], [endmatch[lanes - 1], lanes]]
    for exp in _inputs(oracle, blocks, text, plans):
        check(comp, exp, where=(lanes, exp.counts()[:6]))


@pytest.mark.parametrize("count", (22, 23, 24))
def test_head_and_overflow_boundary(comp, oracle, blocks, text, count):
    for exp in _inputs(oracle, blocks, text, _positions(count) + [[count, 31], [31, count]]):
        check(comp, exp, where=(count, exp.counts()[:6]))


def test_one_and_thirty_one(comp, oracle, blocks, text):
    for exp in _inputs(oracle, blocks, text, [[1, 31], [31, 1], [1, 31, 1, 31], [1, 1, 31]]):
        check(comp, exp, where=exp.counts()[:6])


@pytest.mark.parametrize("length", (300 - 21, 256, 258))
def test_truncated_match_at_either_position(comp, oracle, blocks, text, length):
    t = block_trunc(length)
    plans = [[t, 12], [12, t], [t, 31], [31, t], [t, 30], [30, t], [t, t], [24, t]]
    for exp in _inputs(oracle, blocks, text, plans):
        check(comp, exp, where=(length, exp.counts()[:6]))


def test_last_block_of_a_run_waits_alone(comp, oracle, blocks, text):
    """A block that leaves alone shifts the pairs: blocks 1 .. 14 of the run
    leave two by two and block 15 waits with no block of its run after it."""
    plans = [[32], [3, 32], [32, 5, 32], [31, 32, 31]]
    for exp in _inputs(oracle, blocks, text, plans):
        check(comp, exp, where=exp.counts()[:6])
    # ... and an input that ends inside a run, on a block that waits
    for count in (1, 3, 5):
        exp = planned_input(oracle, blocks, text, [[30, 22, 23, 31, 24][:count]], RUN, False)
        assert exp.nb == count
        check(comp, exp, where=("ends", count))
        check(comp, exp, framed=False, where=("ends", count, "final"), segment=True,
              final_shard=True)


@pytest.fixture(scope="module")
def text_blocks(oracle, text):
    return Expected(oracle, text[:BLK * 33]).blocks


@pytest.mark.parametrize("last_n", (1, 23, 24, 300))
def test_last_block_lengths(comp, oracle, text, text_blocks, last_n):
    for count in (2, 3, 4, 17, 33):
        exp = Expected.of_text_prefix(oracle, text, text_blocks, count, last_n)
        check(comp, exp, where=(count, last_n))
        check(comp, exp, framed=False, where=(count, last_n, "final"), segment=True,
              final_shard=True)


def test_unaligned_input(comp, oracle, blocks, endmatch, text):
    """Not 4-byte aligned: every block is staged and leaves alone."""
    plans = [[30, 31, 32, 22, 23, 24, 1, 31, endmatch[30], block_trunc(258)]]
    exp = planned_input(oracle, blocks, text, plans, RUN, True)
    for mis in (1, 2, 3):
        check(comp, exp, where=mis, misalign=mis)
