"""Constructed LZ4 inputs and the oracle's expectation of them (a helper, no
tests, no GPU): blocks with a given number of sequences, block types that are
hostile neighbours, their placement in groups of consecutive blocks (lz4_tiles'
runs of 16, lz4_emit's workgroups of 32), and the oracle's per-block encodings
of one input.  What a block is for is asserted from the oracle's own encoding
(byte 0 of a block = its sequence count), never from the code under test;
tests/test_lz4_seq_inputs.py holds the properties.
"""
import functools
import math

import numpy as np

BLK = 300


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


def block_dense(seed):
    """36 .. 63 distinct bytes, then random 4-grams of them back to back."""
    rng = np.random.default_rng(seed)
    p = int(rng.integers(36, 64))
    pre = [int(v) for v in rng.permutation(256)[:p]]
    out = list(pre)
    while len(out) < BLK:
        s = int(rng.integers(0, p - 3))
        out += pre[s:s + 4]
    return bytes(out[:BLK])


def block_packed(p, seed=0):
    """p distinct bytes, then 4-grams of them back to back with no pair of
    neighbours used twice and none continuing its predecessor: (300 - p) / 4
    matches of exactly 4."""
    assert (BLK - p) % 4 == 0 and p >= 12
    rng = np.random.default_rng(7000 + seed)
    pre = [int(v) for v in rng.permutation(256)[:p]]
    out, seen, last = list(pre), set(), None
    while len(out) < BLK:
        s = int(rng.integers(0, p - 3))
        if last is not None and (s == last + 4 or (last, s) in seen or s == last):
            continue
        seen.add((last, s))
        out += pre[s:s + 4]
        last = s
    return bytes(out)


def block_endmatch(k, seed=0):
    """block_exact's form with the tail cut short by a last 4-gram copy: the
    block's last record is a match that ends with the block."""
    rng = np.random.default_rng(3000 + 64 * seed + k)
    vals = [int(v) for v in rng.permutation(256)]
    pre, unused = vals[:40], vals[40:]
    out = list(pre)
    for i in range(k - 2):
        s = (5 * i) % 37
        out += pre[s:s + 4] + [unused.pop()]
    pad = BLK - 4 - len(out)
    assert 0 <= pad <= len(unused)
    out += unused[:pad] + pre[33:37]
    assert len(out) == BLK
    return bytes(out)


def block_trunc(length):
    """20 distinct bytes, a run of length + 1 equal bytes (a match of `length`
    bytes, of which the encoder keeps length & 0xFF), distinct bytes."""
    vals = [v for v in range(256) if v != 0x5A]
    rest = BLK - 20 - (length + 1)
    assert rest >= 0
    return bytes(vals[:20]) + b"\x5a" * (length + 1) + bytes(vals[100:100 + rest])


def enc_of(oracle, blk):
    return oracle.lz4_blocks(np.frombuffer(blk, dtype=np.uint8), 0, 1)


def nseq(oracle, blk):
    return enc_of(oracle, blk)[0]


@functools.lru_cache(maxsize=None)
def blocks_by_count(oracle):
    """{sequence count: block} for 1 .. 65 and whatever the packed blocks
    reach above, each count asserted on the oracle.  One table per oracle:
    read it, do not change it."""
    by = {}
    for k in range(1, 54):
        by[k] = block_exact(k)
        assert nseq(oracle, by[k]) == k, k
    for seed in range(400):
        b = block_dense(seed)
        by.setdefault(nseq(oracle, b), b)
    assert all(k in by for k in range(54, 66)), sorted(k for k in by if k > 53)
    for p in (36, 32, 28, 24, 20):
        for seed in range(4):
            b = block_packed(p, seed)
            by.setdefault(nseq(oracle, b), b)
    return by


# ---- hostile neighbours -------------------------------------------------------

def block_types(text):
    """Five blocks that leave different things behind for the next one."""
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


def de_bruijn_pairs(k):
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


def hostile_order(ntypes, max_run):
    """Type indices with every ordered pair of the types at every position of
    a run of up to max_run blocks: the pair cycle, closed by its first block
    and padded with type 3 (the text) to a length coprime to max_run (27 for
    five types), max_run times."""
    cyc = de_bruijn_pairs(ntypes)
    period = cyc + [cyc[0], 3]
    assert math.gcd(len(period), max_run) == 1
    order = period * max_run
    pos = {(order[i], order[i + 1], i % max_run) for i in range(len(order) - 1)}
    assert all((a, b, p) in pos for a in range(ntypes) for b in range(ntypes) for p in range(max_run))
    return order


# ---- the oracle's expectation of one input ---------------------------------------

class Expected:
    """The oracle's per-block encodings of one input, computed once."""

    def __init__(self, oracle, data, known=()):
        """known: encodings somebody already has of the data's leading full
        blocks (a block's encoding depends on its own bytes only)."""
        self.data = bytes(data)
        buf = np.frombuffer(self.data, dtype=np.uint8)
        self.nb = (len(self.data) + BLK - 1) // BLK
        have = min(len(known), len(self.data) // BLK)
        self.blocks = list(known[:have]) + [oracle.lz4_blocks(buf, b, b + 1)
                                            for b in range(have, self.nb)]

    @classmethod
    def of_text_prefix(cls, oracle, text, text_blocks, count, last_n):
        """Of the text's first `count` blocks, the last one cut to last_n
        bytes; text_blocks are the encodings of the text's full blocks."""
        return cls(oracle, text[:BLK * (count - 1) + last_n], known=text_blocks)

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


# ---- blocks placed in groups -----------------------------------------------------

def place(groups, text, width, pad_last):
    """Each group of blocks at the start of `width` consecutive blocks of its
    own, padded with text blocks (the last group only if pad_last: without,
    the input ends with it)."""
    out, pos, full = [], 0, len(text) // BLK
    for g, group in enumerate(groups):
        assert 1 <= len(group) <= width
        out += list(group)
        if pad_last or g + 1 < len(groups):
            for _ in range(width - len(group)):
                out.append(bytes(text[BLK * pos:BLK * (pos + 1)]))
                pos = (pos + 1) % full
    return b"".join(out)


def planned_input(oracle, blocks, text, plans, width, pad_last):
    """plans: per group, a list of sequence counts (ints, looked up in
    `blocks`) or ready blocks (bytes).  -> Expected of the placed input; every
    given count is asserted on the oracle's encoding."""
    groups = [[blocks[x] if isinstance(x, int) else x for x in plan] for plan in plans]
    exp = Expected(oracle, place(groups, text, width, pad_last))
    got = exp.counts()
    for g, plan in enumerate(plans):
        for i, x in enumerate(plan):
            if isinstance(x, int):
                assert got[width * g + i] == x, (g, i, x, got[width * g + i])
    return exp
