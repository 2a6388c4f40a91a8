"""The constructed LZ4 inputs (tests/lz4_seq_inputs.py) have the properties the
GPU tests build on, each read from the oracle's own encoding (lz4_format's
reading of it: sequences (L, D, M)).  No GPU."""
import numpy as np
import pytest

import golden_inputs
import lz4_format as F
from lz4_seq_inputs import (BLK, Expected, block_endmatch, block_exact, block_trunc, block_types,
                            blocks_by_count, enc_of, hostile_order, nseq, place, planned_input)


@pytest.fixture(scope="module")
def text():
    return golden_inputs.lz4_input("metamorphosis_spaces")


@pytest.fixture(scope="module")
def text_blocks(oracle, text):
    return Expected(oracle, text[:BLK * 96]).blocks


def _sequences(oracle, blk):
    return next(F.readings(enc_of(oracle, blk)))


def test_blocks_by_count_has_every_count(oracle):
    by = blocks_by_count(oracle)
    assert set(range(1, 66)) <= set(by)
    assert max(by) >= 66                       # a block that holds a whole round of 64 records
    for k, blk in by.items():
        assert len(blk) == BLK and nseq(oracle, blk) == k, k
    assert blocks_by_count(oracle) is by       # built once per oracle


@pytest.mark.parametrize("k", range(1, 54))
def test_block_exact_is_matches_of_4(oracle, k):
    seqs = _sequences(oracle, block_exact(k))
    assert len(seqs) == k
    assert all(M == 4 for _, _, M in seqs[:-1])
    assert F.is_tail(seqs[-1])                 # a literal-only tail


def test_block_endmatch_ends_on_a_match(oracle):
    seqs = _sequences(oracle, block_endmatch(12))
    L, D, M = seqs[-1]
    assert D > 0 and M >= 4 and F.decoded_len(seqs) == BLK
    assert 2 <= len(seqs) < 25


@pytest.mark.parametrize("length", (256, 257, 258, 259, 260, BLK))
def test_truncated_match(oracle, length):
    """A match of 256 or more bytes is stored as its length & 0xFF: 1 .. 3 a
    truncated match, 0 no match at all (its first byte joins the literals)."""
    blk, at = (b"\x5a" * BLK, 1) if length == BLK else (block_trunc(length), 21)
    found = int(oracle.lz4_matches(blk)[at]) & 0xFFFF
    assert found == (BLK - 1 if length == BLK else length) and found >= 256
    L, D, M = _sequences(oracle, blk)[0]
    if found & 0xFF:
        assert (L, D, M) == (at, 1, found & 0xFF)
        assert F.is_truncated((L, D, M)) == (found & 0xFF < 4)
    else:
        assert L == at + 1 and M == 255


def test_block_types(oracle, text):
    types = block_types(text)
    assert len(types) == 5 and all(len(t) == BLK for t in types)
    enc = [enc_of(oracle, t) for t in types]
    assert enc[4][0] > 23                      # the overflow slot (records 23..)
    assert enc[2][0] == 1 and len(enc[2]) > BLK   # one literal run, longer than the block
    assert types[3] == bytes(text[9000:9300])


def test_hostile_order():
    order = hostile_order(5, 16)
    assert len(order) == 27 * 16 and set(order) == set(range(5))
    seen = {(order[i], order[i + 1], i % 16) for i in range(len(order) - 1)}
    assert seen >= {(a, b, p) for a in range(5) for b in range(5) for p in range(16)}


@pytest.mark.parametrize("width,pad_last", [(16, True), (32, False)])
def test_place(oracle, text, width, pad_last):
    by = blocks_by_count(oracle)
    groups = [[by[3]], [by[5], by[7]], [by[k] for k in range(1, width + 1)], [by[9], by[2]]]
    data = place(groups, text, width, pad_last)
    assert len(data) == BLK * (width * 3 + (width if pad_last else 2))
    for g, group in enumerate(groups):
        for i, blk in enumerate(group):
            at = BLK * (width * g + i)
            assert data[at:at + BLK] == blk, (g, i)
    assert data[BLK:2 * BLK] == bytes(text[:BLK])          # the padding is the text, in order
    assert data[BLK * (width + 2):BLK * (width + 3)] == bytes(text[BLK * (width - 1):BLK * width])


def test_planned_input_checks_the_counts(oracle, text):
    by = blocks_by_count(oracle)
    exp = planned_input(oracle, by, text, [[20, by[4], 43], [65]], 16, True)
    assert exp.nb == 32 and exp.counts()[:3] == [20, 4, 43] and exp.counts()[16] == 65
    with pytest.raises(AssertionError):
        planned_input(oracle, {5: by[6]}, text, [[5]], 16, True)


@pytest.mark.parametrize("count,last_n", [(1, 1), (1, 300), (2, 23), (16, 24), (17, 299), (33, 23),
                                          (64, 1), (70, 299), (96, 300)])
def test_of_text_prefix(oracle, text, text_blocks, count, last_n):
    n = BLK * (count - 1) + last_n
    got = Expected.of_text_prefix(oracle, text, text_blocks, count, last_n)
    want = Expected(oracle, text[:n])
    assert (got.data, got.nb, got.blocks) == (want.data, want.nb, want.blocks)
    assert got.nb == count and len(got.data) == n
    assert got.counts() == want.counts() and got.body() == want.body() and got.framed() == want.framed()
    assert np.array_equal(got.sizes(), want.sizes()) and np.array_equal(got.offsets(), want.offsets())
    assert got.offsets().dtype == np.int64 and got.sizes().sum() == len(got.body())
    if n >= BLK:
        assert got.framed() == oracle.lz4_compress(got.data)
