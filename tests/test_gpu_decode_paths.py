"""lz4_decode_blocks through lz4r_decompress_device on streams written by hand
(lz4_format.py): the copy, parse and choice-point paths of lz4r_dec_parse.h
and the load / store paths of lz4r_dec_blocks.h, each reached on purpose.

The tables below state, as (L, D, M) sequence lists, what every class covers;
coverage is asserted from those lists (test_lz4_format.py), never from the
decoder.  Every block under test is decoded in three stream positions:

  early        more than kInMax + 64 bytes before the stream end: the
               unchecked BytesW loads and decode_block_plain
  tail         within the stream's last kInMax + 64 bytes: Bytes<true> and
               the general decode_block
  early+trunc  early, with a truncated sequence in the same block: the plain
               path declines and decode_block runs over BytesW

Text blocks from the oracle fill the rest, so the lanes of a wave hold
different kinds of block.  Every assertion is byte equality with the
constructed plaintext, the decoded length and a clean failure word.

One item of the issue's list cannot be built: a backtrack that takes effect
only after two further sequences.  A truncated sequence's plain reading is
locally valid only for token 0xFF with L >= 15 (the size field's extra count
is then read as the match-extension byte), which shifts the parse by one
byte.  The next sequence's size field S1 is then read as hi(S1) | x << 8 and
would have to lie in 5..255, so S1 >= 1280 > LZ4R_BLOCK_BOUND.  The misread
match itself (>= 19 bytes written, then rewritten) is the most a well-formed
block allows; backtrack_blocks() builds it with and without earlier choice
points pending.
"""
import ctypes

import numpy as np
import pytest

import golden_inputs
import lz4_format as F

pytestmark = pytest.mark.gpu

IN_SAFE = F.BLOCK_BOUND + 64          # kInMax + 64: blocks nearer the end are checked
OK = (1 << 64) - 1
SENTINEL = 0xA5

# ---- class tables ----------------------------------------------------------------
MATCH_D = list(range(1, 34)) + [63, 64, 65, 255, 256, 257, 280]
MATCH_M = list(range(4, 41)) + [254, 255]
MATCH_M_SHIFTED = [4, 8, 15, 16, 17, 33]          # M for match starts 1..3 past D
MATCH_ENDS = list(range(283, 301))
ENDS_D = [1, 3, 7, 8, 15, 16, 17, 33]
ENDS_M = [4, 16, 17, 40]
LIT_L = (list(range(0, 121)) + list(range(125, 132)) + list(range(189, 196)) +
         list(range(253, 260)) + list(range(268, 273)) + [284, 285] + list(range(295, 301)))
AMBIG_M = [17, 18, 19, 255]
TRUNC_L = [0, 1, 5, 14, 15, 16, 270, 271, 280]
LAST_LEN = [1, 2, 15, 16, 17, 299, 300]
WAVE_COUNTS = [1, 31, 32, 33, 64, 65]
OUT_ALIGN = [0, 1, 8, 15]
OUT_CAP_PAST = [0, 1, 15, 16, 17, 299, 300, 301]


def _fill(R, tr=False):
    """Sequences decoding R further bytes after at least one byte: matches at
    distance 1 (short to encode), a literal tail below 4 bytes; tr: a
    truncated sequence first."""
    out = []
    if tr:
        assert R >= 1
        out.append((0, 1, 1))
        R -= 1
    while R >= 4:
        m = min(R, 255)
        if 0 < R - m < 4:
            m = R - 4
        out.append((0, 1, m))
        R -= m
    if R:
        out.append((R, 0, 0))
    return out


def _case(name, seqs, where=None):
    """where: the place a truncated sequence may be added without moving or
    resizing what the block is about ('back': in the filler after it;
    'front': split off the first literal run; None: nowhere, or the block has
    one already)."""
    assert F.decoded_len(seqs) == F.BLOCK, (name, F.decoded_len(seqs))
    return {"name": name, "seqs": seqs, "where": where}


def with_truncated(case):
    """The case with a truncated sequence added (early+trunc), or None."""
    seqs, where = case["seqs"], case["where"]
    if where == "back":
        k = case["core"]
        R = F.decoded_len(seqs[k:])
        if R >= 1:
            return seqs[:k] + _fill(R, tr=True)
        where = "front"
    if where == "front":
        L, D, M = seqs[0]
        if L >= 2 and not F.is_tail(seqs[0]):            # D <= L still holds: 2 + (L - 2)
            return [(1, 1, 1), (L - 2, D, M)] + seqs[1:]
    return None


def _core(name, core, where="back"):
    """core sequences from position 0, then filler to 300 bytes."""
    c = _case(name, core + _fill(F.BLOCK - F.decoded_len(core)), where)
    c["core"] = len(core)
    return c


def match_blocks():
    out = []
    for D in MATCH_D:
        for M in MATCH_M:
            for s in range(4):
                if (s and M not in MATCH_M_SHIFTED) or D + s + M > F.BLOCK:
                    continue
                out.append(_core(f"match D{D} M{M} +{s}", [(D + s, D, M)]))
    for e in MATCH_ENDS:
        for D in ENDS_D:
            for M in ENDS_M:
                out.append(_core(f"match end{e} D{D} M{M}", [(e - M, D, M)]))
    for M in (254, 255):                                  # the longest, ending the block
        for D in (1, 7, 8, 16, 33, 300 - M):
            out.append(_core(f"match end300 D{D} M{M}", [(300 - M, D, M)]))
    for l2 in (0, 1):                                     # source: the previous match's tail
        for D2 in range(1, 18):
            for M2 in (4, 16, 17, 33):
                out.append(_core(f"match chained l{l2} D{D2} M{M2}",
                                 [(8, 8, 20), (l2, D2, M2)]))
    return out


def literal_blocks():
    """A run of L literals followed by a match at distance L (the distance
    word's place is what varies), and the same run as the literal-only tail."""
    out = []
    for L in LIT_L:
        if L == 0:
            out.append(_core("lit L0 match", [(4, 4, 4), (0, 8, 4)]))
        elif L + 4 <= F.BLOCK:
            out.append(_core(f"lit L{L} match", [(L, L, 4)]))
        R = F.BLOCK - L                                   # bytes before the tail
        if L == 0:
            continue                                      # no tail: a block ending on a match
        if R == 0:
            c = _case(f"lit L{L} tail", [(L, 0, 0)], None)
        elif R >= 6:
            pre = [(R - 4, 1, 4)] if R - 6 in (1, 2, 3) else [(2, 1, 4)] + _fill(R - 6)
            c = _case(f"lit L{L} tail", pre + [(L, 0, 0)], "front")
        elif R == 5:
            c = _case(f"lit L{L} tail", [(1, 1, 4), (L, 0, 0)], None)
        elif R >= 2:                                      # only a truncated sequence fits before it
            c = _case(f"lit L{L} tail", [(R - 1, 1, 1), (L, 0, 0)], None)
        else:
            continue                                      # L = 299: one byte cannot be a sequence
        out.append(c)
    return out


def ambiguous_blocks():
    """1..9 tokens 0xFD..0xFF meant as written (L >= 15, M = 17, 18, 19, 255),
    then an ordinary end, and then a truncated sequence."""
    out = []
    for M in AMBIG_M:
        for n in range(1, 10):
            for L in (15, 16):
                core = [(L, (1, 15, 16, 7, L)[k % 5], M) for k in range(n)]
                R = F.BLOCK - F.decoded_len(core)
                if R < 0 or (L == 16 and n not in (1, 4)):
                    continue
                out.append(_core(f"ambig M{M} x{n} L{L}", core))
                if R >= 1:
                    for m in (1, 2, 3):
                        if R >= m:
                            c = _case(f"ambig M{M} x{n} L{L} then trunc{m}",
                                      core + [(0, 1 + m, m)] + _fill(R - m), None)
                            out.append(c)
    return out


def backtrack_blocks():
    """A truncated sequence (token 0xFF, L >= 15, M = 3) whose plain reading
    is valid where it stands: 19 + the next token bytes of match are written,
    the next header then fails, and the tail is rewritten from the choice
    point.  With 0, 2 and 8 earlier choice points pending."""
    out = []
    for npre in (0, 2, 8):
        pre = [(15, (1, 15, 7)[k % 3], 17) for k in range(npre)]
        for L in (15, 17):
            for nxt in ((0, 7, 4), (1, 2, 5)):
                core = pre + [(L, 5, 3), nxt]
                R = F.BLOCK - F.decoded_len(core)
                if R < 0 or not misread_is_valid(core, npre):
                    continue
                out.append(_case(f"backtrack pre{npre} L{L} next{nxt[0]}", core + _fill_lit(R), None))
    return out


def _fill_lit(R):
    """R further bytes as literals (they overwrite what a misread wrote)."""
    return [(R, 0, 0)] if R else []


def misread_is_valid(seqs, k):
    """Is the plain reading of truncated sequence k valid where it stands?"""
    L, D, M = seqs[k]
    if not (M == 3 and L >= 15 and k + 1 < len(seqs)):
        return False
    pos = F.decoded_len(seqs[:k])
    nL, nD, nM = seqs[k + 1]
    ntok = (0xFC + nM) if 1 <= nM <= 3 else (min(nL, 15) << 4) | (0 if nM == 0 else min(nM - 4, 15))
    return pos + L + 19 + ntok <= F.BLOCK


def truncated_blocks():
    """M = 1, 2, 3 with L below 15, at 15 and from 270; first, last and up to
    three in a block."""
    out = []
    for M in (1, 2, 3):
        for L in TRUNC_L:
            if L >= 1:                                    # first: the distance needs a byte
                out.append(_case(f"trunc first L{L} M{M}",
                                 [(L, min(L, 3), M)] + _fill(F.BLOCK - L - M), None))
            a = F.BLOCK - 4 - L - M                       # last: (a, 1, 4) before it
            out.append(_case(f"trunc last L{L} M{M}", [(a, 1, 4), (L, 2, M)], None))
        out.append(_case(f"trunc x2 M{M}", [(3, 2, M), (14, 5, 3), (0, 1, 4)] +
                         _fill(F.BLOCK - 24 - M), None))
        out.append(_case(f"trunc x3 M{M}", [(15, 4, M), (0, 3, 1), (16, 9, 2)] +
                         _fill(F.BLOCK - 34 - M), None))
        out.append(_case(f"trunc x3 end M{M}", [(1, 1, 4), (270, 200, M), (1, 1, 2)] +
                         _fill(19 - M) + [(0, 1, 3)], None))
    return out


def count_blocks():
    out = [
        _case("count one literal", [(300, 0, 0)], None),
        _case("count one match", [(45, 45, 255)], "front"),
        _case("count two", [(40, 3, 200), (60, 0, 0)], "front"),
        _case("count two matches", [(10, 10, 90), (100, 7, 100)], "front"),
        # as many sequences as 300 bytes hold: 4 decoded bytes each is the least
        _case("count 75", [(1, 1, 4)] + [(0, 1 + k % 5, 4) for k in range(73)] + [(3, 0, 0)], None),
        _case("count 75 trunc", [(1, 1, 4)] + [(0, 1 + k % 4, 4) for k in range(73)] + [(0, 2, 3)],
              None),
        _case("count 77", [(1, 1, 1), (0, 1, 1), (0, 2, 1)] + [(0, 1 + k % 4, 4) for k in range(74)],
              None),
        _case("count 74", [(4, 4, 4)] + [(0, 4 + k % 4, 4) for k in range(73)], None),
    ]
    return out


def last_blocks():
    """(name, sequences) of short last blocks: literal-only and ending on a
    match (2 bytes: only a truncated match fits; 1 byte: nothing does)."""
    out = []
    for n in LAST_LEN:
        out.append((f"last {n} literal", [(n, 0, 0)]))
        if n == 2:
            out.append(("last 2 match", [(1, 1, 1)]))
        elif n >= 15:
            out.append((f"last {n} match", [(n - 9, 3, 9)] if n < 299 else [(n - 255, 44, 255)]))
    return out


CLASSES = {
    "match": match_blocks, "literal": literal_blocks, "ambiguous": ambiguous_blocks,
    "backtrack": backtrack_blocks, "truncated": truncated_blocks, "count": count_blocks,
}

# ---- streams ------------------------------------------------------------------------
_cache = {}


def text_blocks(oracle):
    """(block bytes, decoded) of 300-byte text blocks, from the oracle."""
    if "text" not in _cache:
        data = golden_inputs.lz4_input("metamorphosis_spaces")[:300 * 96]
        _cache["text"] = [(oracle.lz4_blocks(data, b, b + 1), data[300 * b:300 * b + 300])
                          for b in range(96)]
    return _cache["text"]


def _lits(seed):
    return F.Literals(np.random.default_rng(seed).integers(0, 256, 600, dtype=np.uint8).tobytes())


def built(cls):
    """Every block of a class: dicts with the written block, its decoded
    bytes and, where one fits, the same with a truncated sequence."""
    key = ("built", cls)
    if key not in _cache:
        out = []
        for i, c in enumerate(CLASSES[cls]()):
            c = dict(c)
            seed = (sorted(CLASSES).index(cls) << 16) + i
            c["blk"], c["dec"] = F.write_block(c["seqs"], _lits(seed))
            ts = with_truncated(c) if c["where"] else None
            c["tseqs"] = ts
            if ts is not None:
                c["tblk"], c["tdec"] = F.write_block(ts, _lits(seed))
            out.append(c)
        _cache[key] = out
    return _cache[key]


def _stream(blocks, name):
    s, offs, plain = F.write_frame(blocks)
    return {"name": name, "stream": s, "offs": offs, "plain": plain}


def early_stream(oracle, cls, trunc=False):
    """Every block of the class (or its truncated form), a text block after
    every seventh, and text to the end so that all of them are early."""
    text = text_blocks(oracle)
    blocks, under = [], []
    for c in built(cls):
        if trunc and c["tseqs"] is None:
            continue
        under.append(len(blocks))
        blocks.append((c["tblk"], c["tdec"]) if trunc else (c["blk"], c["dec"]))
        if len(under) % 7 == 0:
            blocks.append(text[len(blocks) % 90])
    blocks += text[90:96]
    st = _stream(blocks, f"{cls} early" + ("+trunc" if trunc else ""))
    st["under"] = under
    return st


def tail_streams(oracle, cls):
    """The class's blocks in groups that fit in the last kInMax + 64 bytes of
    a stream, each group behind a few text blocks."""
    text = text_blocks(oracle)
    out, grp, size = [], [], 0

    def flush():
        if grp:
            pre = text[len(out) % 80:len(out) % 80 + 2 + len(out) % 5]
            st = _stream(pre + [(c["blk"], c["dec"]) for c in grp], f"{cls} tail {len(out)}")
            st["under"] = list(range(len(pre), len(pre) + len(grp)))
            out.append(st)

    for c in built(cls):
        if size + len(c["blk"]) >= IN_SAFE - 1:
            flush()
            grp, size = [], 0
        grp.append(c)
        size += len(c["blk"])
    flush()
    return out


def last_block_streams(oracle):
    text = text_blocks(oracle)
    out = []
    for i, (name, seqs) in enumerate(last_blocks()):
        last = F.write_block(seqs, _lits(9000 + i), last=True)
        for npre in (0, 3, 32):
            if npre == 0 and F.decoded_len(seqs) < 1:
                continue
            out.append(_stream(text[:npre] + [last], f"{name} after {npre}"))
    return out


def wave_count_streams(oracle):
    """1, 31, 32, 33, 64 and 65 blocks: built and text blocks mixed."""
    text = text_blocks(oracle)
    mix = [(c["blk"], c["dec"]) for cls in ("ambiguous", "truncated", "count", "backtrack")
           for c in built(cls)]
    out = []
    for n in WAVE_COUNTS:
        blocks = [mix[(5 * k + n) % len(mix)] if k % 3 else text[k % 96] for k in range(n)]
        out.append(_stream(blocks, f"wave count {n}"))
    return out


def output_stream(oracle):
    """Three waves of mixed blocks with a short last block, for the output
    paths."""
    text = text_blocks(oracle)
    mix = [(c["blk"], c["dec"]) for cls in ("literal", "truncated", "count")
           for c in built(cls)]
    blocks = [mix[(7 * k) % len(mix)] if k % 2 else text[k % 96] for k in range(69)]
    blocks.append(F.write_block([(30, 7, 40), (7, 0, 0)], _lits(31337), last=True))
    return _stream(blocks, "output")


def all_streams(oracle):
    """Every stream this file decodes (the CPU tier runs the host decoder and
    the plain decoder over the same list)."""
    if "all" not in _cache:
        out = []
        for cls in CLASSES:
            out.append(early_stream(oracle, cls))
            out.append(early_stream(oracle, cls, trunc=True))
            out += tail_streams(oracle, cls)
        out += last_block_streams(oracle)
        out += wave_count_streams(oracle)
        out.append(output_stream(oracle))
        _cache["all"] = out
    return _cache["all"]


def all_built_blocks():
    """(block, decoded, sequences) of every built block, both forms."""
    out = []
    for cls in CLASSES:
        for c in built(cls):
            out.append((c["blk"], c["dec"], c["seqs"]))
            if c["tseqs"] is not None:
                out.append((c["tblk"], c["tdec"], c["tseqs"]))
    return out


# ---- the GPU side --------------------------------------------------------------------

class Runner:
    """Queues lz4r_decompress_device calls on one input, one output and one
    result tensor through the C ABI (the Python wrapper hides the result
    pair and owns the output pointer), and reads everything back once."""

    def __init__(self):
        self.jobs = []

    def add(self, st, out_cap=None, align=0, tag=None):
        self.jobs.append({"st": st, "cap": len(st["plain"]) if out_cap is None else out_cap,
                          "align": align, "tag": tag or st["name"]})

    def run(self):
        import torch
        from lz4jpeg import _lib
        L = _lib.lib()
        ins, offs = bytearray(), []
        o_at = 0
        for j in self.jobs:
            st = j["st"]
            j["in_at"], j["off_at"] = len(ins), len(offs)
            ins += st["stream"]
            offs += st["offs"]
            j["out_at"] = o_at + 64 + j["align"]           # o_at is a multiple of 16
            o_at += (64 + 16 + max(j["cap"], len(st["plain"])) + 64 + 15) & ~15
        d_in = torch.from_numpy(np.frombuffer(bytes(ins), dtype=np.uint8).copy()).cuda()
        d_offs = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
        d_out = torch.full((o_at + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((len(self.jobs), 2), dtype=torch.int64, device="cuda")
        assert d_out.data_ptr() % 16 == 0
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for k, j in enumerate(self.jobs):
            st = j["st"]
            rc = L.lz4r_decompress_device(
                ctypes.c_void_p(d_in.data_ptr() + j["in_at"]), len(st["stream"]),
                ctypes.c_void_p(d_offs.data_ptr() + 8 * j["off_at"]), len(st["offs"]),
                ctypes.c_void_p(d_out.data_ptr() + j["out_at"]), j["cap"],
                ctypes.c_void_p(d_res.data_ptr() + 16 * k), stream)
            assert rc == 0, (j["tag"], rc)
        torch.cuda.synchronize()
        self.out = d_out.cpu().numpy()
        self.res = d_res.cpu().numpy().view(np.uint64)
        self.end = o_at + 16

    def check(self):
        """Bytes below out_cap equal the plaintext, everything else still
        holds the sentinel, the length word is the whole decoded length and no
        block failed."""
        spans = []
        for k, j in enumerate(self.jobs):
            st = j["st"]
            plain = np.frombuffer(st["plain"], dtype=np.uint8)
            n = min(j["cap"], plain.size)
            assert int(self.res[k, 1]) == OK, (j["tag"], "failed block", int(self.res[k, 1]) - 1)
            assert int(self.res[k, 0]) == plain.size, (j["tag"], int(self.res[k, 0]), plain.size)
            got = self.out[j["out_at"]:j["out_at"] + n]
            if not np.array_equal(got, plain[:n]):
                at = int(np.flatnonzero(got != plain[:n])[0])
                b = at // F.BLOCK
                raise AssertionError(f"{j['tag']}: byte {at} (block {b}, byte {at - 300 * b}): "
                                     f"got {got[at]}, expected {plain[at]}")
            spans.append((j["out_at"], j["out_at"] + n))
        at = 0
        for a, b in spans:                                 # everything between the outputs
            assert (self.out[at:a] == SENTINEL).all(), ("written outside an output", at, a)
            at = b
        assert (self.out[at:self.end] == SENTINEL).all(), ("written past the last output", at)


@pytest.mark.parametrize("cls", list(CLASSES))
def test_class_early(gpu, oracle, cls):
    st = early_stream(oracle, cls)
    beg = [1 + st["offs"][b] for b in st["under"]]
    assert max(beg) + IN_SAFE <= len(st["stream"])         # all on the unchecked path
    r = Runner()
    r.add(st)
    r.run()
    r.check()


@pytest.mark.parametrize("cls", list(CLASSES))
def test_class_early_next_to_truncated(gpu, oracle, cls):
    st = early_stream(oracle, cls, trunc=True)
    if not st["under"]:
        assert all(c["where"] is None for c in built(cls))  # the class holds its own
        return
    assert max(1 + st["offs"][b] for b in st["under"]) + IN_SAFE <= len(st["stream"])
    r = Runner()
    r.add(st)
    r.run()
    r.check()


@pytest.mark.parametrize("cls", list(CLASSES))
def test_class_tail(gpu, oracle, cls):
    r = Runner()
    for st in tail_streams(oracle, cls):
        assert min(1 + st["offs"][b] for b in st["under"]) + IN_SAFE > len(st["stream"])
        r.add(st)
        r.add(st, out_cap=len(st["plain"]) + 300, align=8)
    r.run()
    r.check()


def test_last_block_lengths(gpu, oracle):
    r = Runner()
    for st in last_block_streams(oracle):
        for a in (0, 1):
            r.add(st, align=a)
    r.run()
    r.check()


def test_blocks_per_wave(gpu, oracle):
    r = Runner()
    for st in wave_count_streams(oracle):
        r.add(st)
        r.add(st, align=15)
    r.run()
    r.check()


def test_output_alignment_and_capacity(gpu, oracle):
    """d_out at 0, 1, 8 and 15 bytes from a 16-byte boundary (the v_perm
    gather only at 0), out_cap at the decoded length and at 0..301 bytes
    past the first output byte of the first and of a later wave."""
    st = output_stream(oracle)
    n = len(st["plain"])
    assert n > 2 * 9600 + 301 and n % 300
    r = Runner()
    for a in OUT_ALIGN:
        r.add(st, align=a, tag=f"output align {a} tight")
        r.add(st, out_cap=n + 40, align=a, tag=f"output align {a} roomy")
        for wave in (0, 1):
            for past in OUT_CAP_PAST:
                r.add(st, out_cap=9600 * wave + past, align=a,
                      tag=f"output align {a} wave {wave} cap +{past}")
    r.run()
    r.check()
