"""Boundary finding of the bare path (lz4r_dec_bare.h) through
lz4r_decompress_stream_device, on streams written by hand (lz4_format.py).
The writer gives exact block sizes, so a block start, a truncated block or
bytes that only look like a block header can be put at any stream position.
Every case decodes to the constructed plaintext from the stream alone.

What a case claims about the stream -- which position a chunk's first
candidate is, how many chunks the first pass finds inconsistent, how many
block starts a chunk holds -- is asserted from the stream bytes with the
format module's restatement of the candidate rule and of the fast walk
(test_lz4_format.py, and again here before the GPU runs), never from the
decoder.

One item of the issue's list cannot be built as worded: a wave of 64 whole
chunks holds at least 64 * 8192 / 389 > 1024 blocks, since no block of 300
decoded bytes encodes to more than 389 bytes (77 sequences of 5 or 6).  The staging limit of
1024 offsets is met instead at its exact edge by streams of 1023, 1024 and
1025 blocks in one wave of chunks, and crossed by 64 full chunks.
"""
import numpy as np
import pytest

import lz4_format as F

pytestmark = pytest.mark.gpu

LIT = 309                              # bytes of a literal-only block of 300
LIT_AT = 7                             # its literals start here: header 3, token, S, one litext byte
TINY = 16                              # the smallest block of 300 decoded bytes
K_LIST = 32                            # block starts a chunk's list holds
K_STAGE = 1024                         # offsets a wave stages in LDS
K_MIS = 1024                           # inconsistent chunks listed


def _sized_table():
    """Encoded size -> sequences [(L1, 1, M), (L2, 0, 0)] of that size."""
    t = {}
    for L1 in range(1, 297):
        for L2 in range(0, 297 - L1):
            M = 300 - L1 - L2
            if not 4 <= M <= 255:
                continue
            n = 3 + 3 + len(F.litext(L1)) + L1 + 2 + (1 if M >= 19 else 0)
            if L2:
                n += 3 + len(F.litext(L2)) + L2 + 2
            t.setdefault(n, [(L1, 1, M)] + ([(L2, 0, 0)] if L2 else []))
    return t


_SIZED = _sized_table()
SIZED_MIN, SIZED_MAX = 60, 312
assert all(n in _SIZED for n in range(SIZED_MIN, SIZED_MAX + 1))


_LIT_SEQS = [(300, 0, 0)]


class Builder:
    """A stream under construction: the next block starts at self.pos."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.blocks, self.starts, self.kinds, self.seqlists = [], [], [], []
        self.pos = 1

    def add(self, blk, dec, kind="built", seqs=None):
        self.starts.append(self.pos)
        self.kinds.append(kind)
        self.seqlists.append(seqs)
        self.blocks.append((blk, dec))
        self.pos += len(blk)

    def seqs(self, seqs, kind="built", last=False):
        lits = self.rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
        self.add(*F.write_block(seqs, lits, last=last), kind=kind, seqs=seqs)

    def lit(self, n=1):
        """Literal-only blocks whose 4-grams do not repeat."""
        while n > 0:
            d = self.rng.integers(0, 256, (n, 300), dtype=np.uint8)
            w = d.astype(np.uint32)
            g = w[:, :-3] | w[:, 1:-2] << 8 | w[:, 2:-1] << 16 | w[:, 3:] << 24
            g.sort(axis=1)
            for k in np.flatnonzero((g[:, 1:] != g[:, :-1]).all(axis=1)):
                self.add(*F.write_block(_LIT_SEQS, d[k].tobytes()), kind="lit", seqs=_LIT_SEQS)
                n -= 1

    def tiny(self, n=1):
        for _ in range(n):
            self.seqs([(1, 1, 255), (0, 1, 44)], kind="tiny")
        assert self.pos - self.starts[-1] == TINY

    def sized(self, n):
        self.seqs(_SIZED[n], kind="sized")
        assert self.pos - self.starts[-1] == n

    def to(self, target):
        """Blocks up to exactly `target`: literal-only ones, then one or two
        of a chosen size."""
        gap = target - self.pos
        assert gap == 0 or gap >= SIZED_MIN, gap
        while gap > 2 * SIZED_MAX:
            self.lit()
            gap -= LIT
        if gap > SIZED_MAX:
            self.sized(gap // 2)
            gap -= gap // 2
        if gap:
            self.sized(gap)
        assert self.pos == target

    def chunk(self, c, delta=0):
        """Fill up to chunk c's first byte + delta."""
        self.to(1 + c * F.CHUNK + delta)

    def finish(self, name):
        s, offs, plain = F.write_frame(self.blocks)
        assert [1 + o for o in offs] == self.starts
        return {"name": name, "stream": bytearray(s), "offs": offs, "plain": bytearray(plain),
                "starts": self.starts,
                "kinds": self.kinds, "seqs": self.seqlists, "false": [], "trunc_first": []}


def plant(st, c, kind, rng):
    """Write bytes that pass the candidate rule into the literals of the
    literal-only block lying across chunk c's first byte, in the stream and
    in the plaintext alike.  kind 'dies': the false chain stops at its third
    header; 'rejoins': its second header's size field ends on the next true
    block start.  False when the block has no room."""
    import bisect
    s0 = 1 + c * F.CHUNK
    starts = st["starts"]
    i = bisect.bisect_right(starts, s0) - 1
    if st["kinds"][i] != "lit" or starts[i] == s0 or i + 1 >= len(starts):
        return False
    x, t = max(s0, starts[i] + LIT_AT), starts[i] + LIT
    p = 300 * i + (x - starts[i] - LIT_AT)
    while True:                                            # until no 4-gram of the block repeats
        r = [int(v) for v in 16 + rng.permutation(224)[:8]]
        if kind == "dies":
            fake = bytes([1, 8, 0, r[0], 5, 0, r[1], r[2], 1, 8, 0, r[3], r[4], r[5], r[6], r[7], 0])
        else:
            size2 = t - (x + 8)
            if size2 < 8:
                return False
            fake = bytes([1, 8, 0, r[0], 5, 0, r[1], r[2], 1, size2 & 255, size2 >> 8])
        if x + len(fake) > starts[i] + LIT_AT + 300:
            return False
        blk = bytearray(st["plain"][300 * i:300 * i + 300])
        blk[p - 300 * i:p - 300 * i + len(fake)] = fake
        if F.no_repeated_4gram(bytes(blk)):
            break
    st["stream"][x:x + len(fake)] = fake
    st["plain"][p:p + len(fake)] = fake
    st["false"].append(c)
    return True


def false_chunks(st):
    """Chunks whose first candidate lies before their first true block start."""
    s = bytes(st["stream"])
    out = []
    for c in range(1, F.nchunks(s)):
        t, x = F.first_start(st["offs"], c), F.first_candidate(s, c)
        if x is not None and (t is None or x < t):
            out.append(c)
    return out


def starts_per_chunk(st):
    n = [0] * F.nchunks(st["stream"])
    for o in st["offs"]:
        n[o // F.CHUNK] += 1
    return n


TRUNC_BLOCK = [(10, 3, 2), (0, 1, 255), (0, 1, 33)]


# ---- the streams -----------------------------------------------------------------------

def geometry_streams():
    out = []
    b = Builder(1)                                          # a true start at a chunk's first byte,
    for c, d in ((1, -1), (2, 0), (3, 1)):                 # one byte before it and one after it
        b.chunk(c, d)
        b.lit()
    b.lit(3)
    out.append(b.finish("starts at chunk edges -1 0 +1"))
    for d in (-1, 0, 1, 2):                                # in_len - 1 = 2 * 8192 + d
        b = Builder(10 + d)
        b.to(1 + 2 * F.CHUNK + d - LIT)
        b.lit()
        st = b.finish(f"stream ends {d:+d} past a chunk")
        assert len(st["stream"]) - 1 == 2 * F.CHUNK + d
        out.append(st)
    b = Builder(20)
    b.chunk(1, -9)
    b.seqs([(1, 0, 0)], last=True)
    st = b.finish("a one-byte last block ending a chunk")
    assert len(st["stream"]) - 1 == F.CHUNK and len(st["plain"]) % 300 == 1
    out.append(st)
    b = Builder(21)
    b.lit(5)
    out.append(b.finish("single chunk"))
    b = Builder(22)
    b.seqs([(300, 0, 0)], last=True)
    out.append(b.finish("single block"))
    for n in (63, 64, 65):
        b = Builder(30 + n)
        b.tiny(40)
        b.to(1 + n * F.CHUNK - 100 - LIT)
        b.lit()
        st = b.finish(f"{n} chunks")
        assert F.nchunks(st["stream"]) == n
        out.append(st)
    return out


def _lit_stream(seed, nchunk, name, lead=LIT - 120):
    """Literal-only blocks over nchunk chunks, a block lying across every
    chunk's first byte with `lead` of its bytes in the earlier chunk."""
    b = Builder(seed)
    for c in range(1, nchunk):
        b.chunk(c, -lead)
        b.lit()
    b.lit(4)
    return b.finish(name)


def false_candidate_streams():
    out = []
    rng = np.random.default_rng(5)
    plans = {
        "chunk 1": [1], "chunks 1 and 2": [1, 2], "last chunk": [5],
        "after a repaired chunk, and apart": [1, 2, 3, 5],
    }
    for kind in ("dies", "rejoins"):
        for what, chunks in plans.items():
            st = _lit_stream(40 + len(out), 6, f"false candidate, {kind}: {what}")
            for c in chunks:
                assert plant(st, c, kind, rng)
            out.append(st)
    st = _lit_stream(60, 6, "false candidates, mixed")
    for c, kind in ((1, "rejoins"), (2, "dies"), (3, "rejoins"), (4, "dies"), (5, "rejoins")):
        assert plant(st, c, kind, rng)
    out.append(st)
    return out


def exact_mode_streams(ambiguous):
    """ambiguous: (block, decoded, sequences) with plainly read 0xFD..0xFF tokens
    and no truncated sequence."""
    out = []
    rng = np.random.default_rng(6)
    for what, chunks, false in (("one chunk", [2], []), ("two chunks", [1, 3], []),
                                ("and a false candidate", [2], [4]),
                                ("and a false candidate before it", [3], [1])):
        b = Builder(70 + len(out))
        for c in range(1, 6):
            if c in chunks:
                b.chunk(c, 2 * c)
                b.seqs(TRUNC_BLOCK, kind="trunc")
                b.lit()
            else:
                b.chunk(c, -150)
                b.lit()
        b.lit(3)
        st = b.finish(f"truncated block first in its chunk: {what}")
        st["trunc_first"] = chunks
        for c in false:
            assert plant(st, c, "rejoins", rng)
        out.append(st)
    b = Builder(80)
    for k, (blk, dec, seqs) in enumerate(ambiguous):
        b.add(blk, dec, kind="ambiguous", seqs=seqs)
        b.lit(2)
    b.lit(4)
    st = b.finish("plainly read 0xFD..0xFF tokens, no truncated sequence")
    assert F.nchunks(st["stream"]) >= 3
    out.append(st)
    return out


def limit_streams():
    out = []
    rng = np.random.default_rng(7)
    for n in (K_LIST, K_LIST + 1):                         # exactly 32 and 33 starts in chunk 1
        b = Builder(90 + n)
        b.chunk(1)
        for _ in range(n - 1):
            b.sized(256 if n == K_LIST else 250)
        b.chunk(2, 0 if n == K_LIST else 58 + 250)
        b.lit(3)
        st = b.finish(f"{n} block starts in a chunk")
        assert starts_per_chunk(st)[1] == n
        out.append(st)
    for n in (K_STAGE - 1, K_STAGE, K_STAGE + 1):          # one wave of chunks at the staging limit
        b = Builder(100 + n)
        b.lit(2)
        b.tiny(n - 6)
        b.lit(4)
        st = b.finish(f"{n} blocks in one wave of chunks, hundreds in a chunk")
        assert len(st["offs"]) == n and F.nchunks(st["stream"]) <= 64
        assert max(starts_per_chunk(st)) > 300
        out.append(st)
    b = Builder(110)                                       # re-walked and over the list limit
    b.chunk(1, -100)
    b.lit()
    b.tiny(700)
    b.chunk(3, -100)
    b.lit()
    b.tiny(100)
    b.lit(2)
    st = b.finish("a re-walked chunk over the list limit")
    assert plant(st, 1, "dies", rng) and plant(st, 3, "rejoins", rng)
    n = starts_per_chunk(st)
    assert n[1] > K_LIST and n[3] > K_LIST
    out.append(st)
    return out


_big = {}
MANY = [K_MIS, K_MIS + 1, "apart"]


def many_false_stream(target):
    """About 1,100 chunks of literal-only blocks.  target 1024 or 1025: false
    candidates of the rejoining kind are planted chunk by chunk until the
    first pass's inconsistent chunks number exactly that (each makes its
    predecessor inconsistent and nothing else).  Neighbouring repairs hand
    on to each other, so one listed chunk would be enough for such a run;
    target 'apart' plants dying false candidates in every other chunk: each
    chunk and its predecessor are inconsistent, more than 1,024 in all, and
    every pair has to be found by itself."""
    if target in _big:
        return _big[target]
    if "base" not in _big:
        b = Builder(200)
        for c in range(1, 1120):
            gap = 1 + c * F.CHUNK - 150 - b.pos
            b.lit(gap // LIT - 1)
            b.chunk(c, -150)
            b.lit()
        b.lit(2)
        st = b.finish("")
        _big["base"] = (st, set(false_chunks(st)))         # what random literals give by themselves
    st, base = _big["base"]
    st = dict(st, name=f"{target} inconsistent chunks", stream=bytearray(st["stream"]),
              plain=bytearray(st["plain"]), false=[])
    rng = np.random.default_rng(8)
    if target == "apart":
        for c in range(1, F.nchunks(st["stream"]) - 1, 2):
            if not {c - 1, c, c + 1} & base:
                assert plant(st, c, "dies", rng)
    else:
        c = 1
        while len(base | set(st["false"])) < target:
            if c not in base:
                assert plant(st, c, "rejoins", rng)
            c += 1
    _big[target] = st
    return st


def all_streams(ambiguous):
    return (geometry_streams() + false_candidate_streams() + exact_mode_streams(ambiguous) +
            limit_streams() + [many_false_stream(t) for t in MANY])


def ambiguous_pairs():
    import test_gpu_decode_paths as P
    return [(c["blk"], c["dec"], c["seqs"]) for c in P.built("ambiguous")
            if not any(F.is_truncated(s) for s in c["seqs"])]


# ---- the GPU side -------------------------------------------------------------------------

def _decode(st, cap):
    import torch
    from lz4jpeg import lz4
    s = np.frombuffer(bytes(st["stream"]), dtype=np.uint8)
    d_stream = torch.from_numpy(s.copy()).cuda()
    d_out = torch.full((max(cap, 1) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _, got = lz4.decompress_stream_device(d_stream, s.size, cap, d_out=d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), got


def _check(st, caps=("tight",)):
    from lz4jpeg import lz4
    plain = np.frombuffer(bytes(st["plain"]), dtype=np.uint8)
    for cap in caps:
        if cap == "short":
            with pytest.raises(lz4.Lz4Error) as ei:
                _decode(st, plain.size - 1)
            assert ei.value.code == -3, st["name"]
            continue
        n = plain.size if cap == "tight" else 300 * (len(st["stream"]) // 8 + 8)
        out, got = _decode(st, n)
        assert got == plain.size, (st["name"], cap, got)
        if not np.array_equal(out[:got], plain):
            at = int(np.flatnonzero(out[:got] != plain)[0])
            raise AssertionError(f"{st['name']} ({cap}): byte {at} of block {at // 300}")
        assert (out[n:] == 0xA5).all(), (st["name"], cap)


CAPS = ("tight", "oversized", "short")


def test_chunk_geometry(gpu):
    for st in geometry_streams():
        _check(st)


def test_false_candidates(gpu):
    for st in false_candidate_streams():
        assert sorted(st["false"]) == false_chunks(st), st["name"]
        _check(st, CAPS)


def test_exact_mode(gpu):
    for st in exact_mode_streams(ambiguous_pairs()):
        s = bytes(st["stream"])
        for c in st["trunc_first"]:                        # the candidate skips the truncated block
            assert F.first_candidate(s, c) > F.first_start(st["offs"], c), st["name"]
        assert sorted(st["false"]) == false_chunks(st), st["name"]
        if not st["trunc_first"]:
            assert F.walk_offsets(s) == st["offs"]          # the fast pass can succeed
        _check(st, CAPS)


def test_list_and_staging_limits(gpu):
    for st in limit_streams():
        _check(st, ("tight", "oversized"))


@pytest.mark.parametrize("target", MANY)
def test_many_inconsistent_chunks(gpu, target):
    """1,024 inconsistent chunks are still listed; 1,025 make lz4_bare_fix
    check every chunk in order, and so do 1,100 that lie apart in pairs: only
    there does a chunk left out of the list stay unrepaired."""
    st = many_false_stream(target)
    falses, mis = false_chunks(st), F.fast_chain(bytes(st["stream"]))[2]
    if target == "apart":
        assert len(mis) > K_MIS + 50 and len(mis) == 2 * len(falses)
        assert all(b - a >= 2 for a, b in zip(falses, falses[1:]))
    else:
        assert len(falses) == target and len(mis) == target
    _check(st)
