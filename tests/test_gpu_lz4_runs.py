"""lz4_tiles over runs of blocks: what one block leaves behind is what the
next block of the run starts from.

A wave encodes a run of consecutive blocks (kTileRun, csrc/lz4r_layout.h) in
one loop over one LDS allocation, and loads the next block's dwords while it
is still busy with the current one.  A one-block workgroup never had a
predecessor; here every case compares, against the oracle encoder on the same
bytes, the whole stream byte for byte, the length word (bit 63 clear) and the
device block offsets and sizes (lz4_gpu_lib.check).

- run boundaries: every block count 1 .. 4 * 16 + 6 (runs of up to 16 that
  end early, end exactly, or spill one block over) crossed with the last
  block's length 1, 23, 24, 299, 300 (23 / 24: whether the block BEFORE the
  last may be read unstaged, i.e. whether it may be prefetched), plus one
  input per count that is not 4-byte aligned (the staged instantiation);
- hostile neighbours: five block types in every ordered pair at every
  position of a run of up to 16 (a de Bruijn cycle of the pairs, repeated at
  a stride coprime to the run length), framed and through the segment API.
"""
import pytest

import golden_inputs
import lz4_gpu_lib
from lz4_gpu_lib import check
from lz4_seq_inputs import BLK, Expected, block_types, enc_of, hostile_order

pytestmark = pytest.mark.gpu

MAX_RUN = 16                      # the largest run length the A/B considered
COUNTS = range(1, 4 * MAX_RUN + 6 + 1)
LAST_N = (1, 23, 24, 299, 300)


@pytest.fixture(scope="module")
def comp(gpu):
    yield from lz4_gpu_lib.compressor()


@pytest.fixture(scope="module")
def text():
    t = golden_inputs.lz4_input("metamorphosis_spaces")
    assert len(t) >= BLK * COUNTS[-1]
    return t


@pytest.fixture(scope="module")
def text_blocks(oracle, text):
    """Oracle encodings of the text's full blocks 0 .. COUNTS[-1] - 1 (shared:
    every run-boundary input is a prefix of the same text)."""
    return Expected(oracle, text[:BLK * COUNTS[-1]]).blocks


def _check_text(comp, oracle, text, text_blocks, count, last_n, misalign=0):
    exp = Expected.of_text_prefix(oracle, text, text_blocks, count, last_n)
    # an input shorter than one block has no framed form: a final segment
    seg = len(exp.data) < BLK
    check(comp, exp, framed=not seg, where=(count, last_n, misalign), misalign=misalign,
          segment=seg, final_shard=True if seg else None)


@pytest.mark.parametrize("count", COUNTS)
def test_run_boundaries(comp, oracle, text, text_blocks, count):
    for last_n in LAST_N:
        _check_text(comp, oracle, text, text_blocks, count, last_n)
    # not 4-byte aligned: every block of the run is staged, none prefetched
    _check_text(comp, oracle, text, text_blocks, count, LAST_N[count % len(LAST_N)],
                misalign=1 + count % 3)


@pytest.fixture(scope="module")
def hostile(oracle, text):
    """Every ordered pair of the five block types at every position of a run
    of up to MAX_RUN blocks (lz4_seq_inputs.hostile_order)."""
    types = block_types(text)
    enc = [enc_of(oracle, t) for t in types]
    # block header: u8 sequence count, u16 size (LZ4.c:415-425)
    assert enc[4][0] > 23, "the overflow slot (records 23..) is not exercised"
    assert enc[2][0] == 1 and len(enc[2]) > BLK, "the random block must be one literal run"
    order = hostile_order(len(types), MAX_RUN)
    assert len(order) == 27 * MAX_RUN
    return Expected(oracle, b"".join(types[i] for i in order))


def test_hostile_neighbours_framed(comp, hostile):
    check(comp, hostile)


@pytest.mark.parametrize("final_shard", [False, True])
def test_hostile_neighbours_segment(comp, hostile, final_shard):
    check(comp, hostile, framed=False, segment=True, final_shard=final_shard)
