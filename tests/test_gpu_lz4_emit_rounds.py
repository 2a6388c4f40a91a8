"""lz4_emit's sequence rounds: a workgroup's records are dealt to its waves in
rounds of 64 flattened records (csrc/lz4r_emit.h, emit_records).

Every case compares, against the oracle's per-block encodings of the same
bytes, the whole stream byte for byte, the length word (bit 63 clear) and the
device block offsets and sizes (lz4_gpu_lib.check).  What a case covers is
asserted from the oracle's own encoding (byte 0 of a block = its sequence
count), never from the code under test.

An emit workgroup is the 32 blocks [32 w, 32 w + 32) of a launch and a scan
group is 64 blocks, so a case is an input of 1 .. ~100 blocks: a list of
workgroup plans, each a list of blocks with given sequence counts, padded with
text blocks to 32.

- T, the workgroup's record count, at the capacity of one round per wave:
  511 .. 513, 575 .. 577, 32 (one-sequence blocks), above 1,024;
- a flattened index that is a multiple of 64 on a block's first record, on its
  last one (a match, a literal-only tail), inside a block, and a round with
  more than eight block starts;
- a block of 62 .. 65 records at index 0, at index 63, last of a workgroup,
  first of the next; a block of more than 65 that holds a whole round;
- a block with an overflow slot (> 23 records) with a round starting at its
  record 22 .. 25 (the record before it in the head / in the slot);
- edges of the launch: block counts 1 .. 96, short last blocks, framed and as
  a segment; the output offset by 0, 1, 15 bytes, the input by 1, 2, 3;
- capacity: nothing at or past `cap` is written, the length word is whole.
"""
import numpy as np
import pytest

import golden_inputs
import lz4_gpu_lib
from lz4_gpu_lib import check
from lz4_seq_inputs import BLK, Expected, block_endmatch, blocks_by_count, enc_of, nseq, planned_input

pytestmark = pytest.mark.gpu

WG = 32                                # blocks per lz4_emit workgroup
ROUND = 64                             # records per round


@pytest.fixture(scope="module")
def blocks(oracle):
    """{sequence count: block} for 1 .. 65 and whatever the packed blocks
    reach above, each count asserted on the oracle."""
    return blocks_by_count(oracle)


@pytest.fixture(scope="module")
def text():
    return golden_inputs.lz4_input("metamorphosis_spaces")


@pytest.fixture(scope="module")
def comp(gpu):
    yield from lz4_gpu_lib.compressor()


def _plan_input(oracle, blocks, text, plans):
    """plans: per workgroup, a list of sequence counts (ints) or ready blocks
    (bytes), each at the start of a workgroup of its own, padded with text
    (the last one is not padded: the input ends with it)."""
    return planned_input(oracle, blocks, text, plans, WG, pad_last=False)


def _starts(exp, w):
    """First flattened index of each block of workgroup w, and T."""
    c = exp.counts()[WG * w:WG * (w + 1)]
    s = np.concatenate(([0], np.cumsum(c)))
    return [int(v) for v in s[:-1]], int(s[-1])


def _split(total, n, lo, hi, seed):
    """n counts in [lo, hi] that sum to total."""
    rng = np.random.default_rng(seed)
    c = [lo] * n
    assert n * lo <= total <= n * hi
    for _ in range(total - n * lo):
        i = int(rng.integers(0, n))
        while c[i] == hi:
            i = (i + 1) % n
        c[i] += 1
    return c


# ---- 1. T at the workgroup's capacity -------------------------------------------

@pytest.mark.parametrize("T", (511, 512, 513, 575, 576, 577))
def test_total_at_capacity(comp, oracle, blocks, text, T):
    """T records in one workgroup: as the first and as the second of a scan
    group, two different splits, a few text blocks after them."""
    plans = [_split(T, WG, 2, 40, seed=T), _split(T, WG, 1, 53, seed=T + 1), [12, 9]]
    exp = _plan_input(oracle, blocks, text, plans)
    assert _starts(exp, 0)[1] == T and _starts(exp, 1)[1] == T
    check(comp, exp, where=T)


def test_total_32_one_sequence_blocks(comp, oracle, blocks, text):
    rng = np.random.default_rng(5)
    rnd = [rng.integers(0, 256, BLK, dtype=np.uint8).tobytes() for _ in range(WG)]
    for b in rnd:
        enc = enc_of(oracle, b)
        assert enc[0] == 1 and len(enc) > BLK      # one literal run of 300, its extension bytes
    exp = _plan_input(oracle, blocks, text, [rnd, [1] * WG, rnd[:5]])
    assert _starts(exp, 0)[1] == WG and _starts(exp, 1)[1] == WG
    check(comp, exp)


def test_total_above_1024(comp, oracle, blocks, text):
    dense = [54 + (7 * i) % 12 for i in range(WG)]         # 54 .. 65 records each
    exp = _plan_input(oracle, blocks, text, [dense, dense[::-1], dense[:3]])
    assert _starts(exp, 0)[1] > 1024 and _starts(exp, 1)[1] > 1024
    check(comp, exp)


# ---- 2. a flattened index that is a multiple of 64 ---------------------------------

def test_round_boundary_positions(comp, oracle, blocks, text):
    endm = block_endmatch(12)
    enc = enc_of(oracle, endm)
    km = enc[0]
    assert enc[-2:] != b"\0\0" and 2 <= km < 25     # the last record: a match (its offset)
    assert enc_of(oracle, blocks[35])[-2:] == b"\0\0"   # block_exact ends on a literal-only tail
    one = b"\x5a" * BLK                             # two records, both matches (truncated ones)
    assert nseq(oracle, one) == 2 and enc_of(oracle, one)[-3:-1] != b"\0\0"
    plans = [
        [30, 34, 20, 44, 50, 14],                   # blocks 2 and 4 start at 64 and 128
        [30, 35, 20, 44, 50, 13],                  # index 64, 128: a block's last record (a tail)
        [40, 25 - km, endm, 30, 45, 53 - km, endm, 5],   # ... a match: at 64 and at 192
        [30, 33, one, 62, one],                     # the last of two matches, at 64 and 128
        [50, 30, 53, 53, 53, 53],                   # 64, 128, 192, 256 inside blocks
    ]
    exp = _plan_input(oracle, blocks, text, plans[:3])
    s0, s1, s2 = (_starts(exp, w)[0] for w in range(3))
    assert s0[2] == 64 and s0[4] == 128
    assert s1[2] - 1 == 64 and s1[4] - 1 == 128
    assert s2[3] - 1 == 64 and exp.counts()[64 + 2] == km
    assert s2[7] - 1 == 192 and exp.counts()[64 + 6] == km
    check(comp, exp, where="first / last")
    exp = _plan_input(oracle, blocks, text, plans[3:])
    s0, s1 = (_starts(exp, w)[0] for w in range(2))
    assert s0[2] + 1 == 64 and s0[4] + 1 == 128 and exp.counts()[2] == 2 and exp.counts()[4] == 2
    assert all(any(a < m < a + n - 1 for a, n in zip(s1, exp.counts()[32:38]))
               for m in (64, 128, 192, 256))
    check(comp, exp, where="single / inside")


def test_many_block_starts_in_a_round(comp, oracle, blocks, text):
    plans = [
        [60, 4] + [1] * 12 + [2, 1, 3, 1, 2, 1] + [4] * 12,   # round 1: more than 8 starts
        [53, 3] + [2] * 30,                                  # 8 .. 32 starts per round
        [1] * 20 + [44] + [1] * 11,                          # 20 starts, one block across, 11 more
    ]
    exp = _plan_input(oracle, blocks, text, plans)
    for w in range(3):
        s, T = _starts(exp, w)
        per = [sum(1 for v in s if ROUND * r <= v < ROUND * (r + 1)) for r in range((T + 63) // 64)]
        assert max(per) > 8, per
    check(comp, exp)


# ---- 3. a block of 62 .. 65 records, and one that holds a whole round ------------------

@pytest.mark.parametrize("k", (62, 63, 64, 65))
def test_round_sized_block_positions(comp, oracle, blocks, text, k):
    txt = [bytes(text[BLK * i:BLK * (i + 1)]) for i in range(100, 130)]
    plans = [[k] + txt + [k],                       # at index 0; the workgroup's last block
             [k, 40, 23 + 64 - k, k],               # the next one's first; at index 63 (mod 64)
             [40, 23, k, 5]]                        # at index 63
    exp = _plan_input(oracle, blocks, text, plans)
    c = exp.counts()
    assert c[0] == k and c[31] == k and c[32] == k
    assert _starts(exp, 1)[0][3] % ROUND == 63 and _starts(exp, 2)[0][2] == 63
    check(comp, exp, where=k)


def test_block_across_a_whole_round(comp, oracle, blocks, text):
    """A block of 66 or more records that starts on a round's last lane: the
    next round holds neither its first nor its last record."""
    big = max(blocks)
    assert big >= 66, sorted(k for k in blocks if k > 60)
    plans = [[40, 23, big, 7, big],                 # rounds 0 / 1 / 2; then wherever it falls
             [big, big, big, 9],                    # a block's middle round at index 64 + ...
             [50, 40, 37, big]]                     # its whole round is the workgroup's round 2
    exp = _plan_input(oracle, blocks, text, plans)
    for w, b in ((0, 2), (2, 3)):
        s = _starts(exp, w)[0][b]
        assert s % ROUND == 63 and s + big > (s // ROUND + 2) * ROUND
    check(comp, exp, where=big)


# ---- 4. the overflow slot at a round's start ----------------------------------------

@pytest.mark.parametrize("big", (26, 30, 47))
def test_round_starts_inside_overflow(comp, oracle, blocks, text, big):
    """A round's first record is record j (counted from 0) of a block with an
    overflow slot; the record before it, the start of its literal run, is the
    head's last one (j = 23) or lies in the slot (j = 24, 25)."""
    assert big > 25
    plans = []
    for ja, jb in ((22, 23), (24, 25)):          # two such blocks per workgroup
        fill = (ja - jb - big) % ROUND or ROUND
        plans.append([ROUND - ja, big, fill, big, 3])
    exp = _plan_input(oracle, blocks, text, plans)
    for w, (ja, jb) in enumerate(((22, 23), (24, 25))):
        s = _starts(exp, w)[0]
        assert exp.counts()[WG * w + 1] == big and exp.counts()[WG * w + 3] == big
        assert -s[1] % ROUND == ja and -s[3] % ROUND == jb   # the round starts at record ja / jb
    check(comp, exp, where=big)


# ---- 5. edges of the launch ------------------------------------------------------

@pytest.fixture(scope="module")
def text_blocks(oracle, text):
    return Expected(oracle, text[:BLK * 96]).blocks


@pytest.mark.parametrize("count", (1, 31, 32, 33, 63, 64, 65, 96))
def test_launch_edges(comp, oracle, text, text_blocks, count):
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


# ---- 6. alignment ----------------------------------------------------------------

def test_output_and_input_alignment(comp, oracle, blocks, text):
    plans = [[20, 43, 3, 65, 1, 1, b"\x5a" * BLK, 30], [64, 30, 34], [17]]
    exp = _plan_input(oracle, blocks, text, plans)
    for lead in (0, 1, 15):
        check(comp, exp, where=("lead", lead), lead=lead)
        check(comp, exp, framed=False, where=("lead", lead, "segment"), lead=lead, segment=True,
               final_shard=True)
    for mis in (1, 2, 3):
        check(comp, exp, where=("misalign", mis), misalign=mis)
    check(comp, exp, where=("both", 3, 15), misalign=3, lead=15)


# ---- 7. capacity -----------------------------------------------------------------

@pytest.mark.parametrize("n,length", ((9300, 9633), (9600, 9937), (12000, None)))
def test_capacity(comp, oracle, text, n, length):
    """Every byte below cap equals the oracle's, every byte at or past it is
    untouched, and the length word still reports the full length.  The text
    from its byte 5 on: there 31 and 32 blocks make streams of 16 m + 1 bytes."""
    exp = Expected(oracle, text[5:5 + n])
    full = len(exp.framed())
    if length is not None:
        # 16 m + 1: cap = full - 1 ends on a 16-byte store chunk, full - 2 does not
        assert full == length and full % 16 == 1
    caps = {full, full - 1, full - 2}
    m = (full - 1) // 16 * 16                    # (16 m - 1, 16 m): the last partial chunk or none
    caps |= {m - 1, m}
    if exp.nb > WG:
        o = 1 + int(exp.offsets()[WG])           # block 32: the second workgroup's first byte
        caps |= {o - 1, o, o + 1}
    for cap in sorted(caps):
        check(comp, exp, where=(n, cap), cap=cap)
