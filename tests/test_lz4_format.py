"""CPU tier of the hand-written LZ4 streams: the writer in lz4_format.py is
proved against the oracle and the host decoder before test_gpu_decode_paths.py
and test_gpu_bare_chain.py trust it, and the tables of those two files are
checked for what they claim to cover -- from the sequence lists and the
stream bytes, with no GPU.
"""
import numpy as np
import pytest

import golden_inputs
import lz4_format as F
import test_gpu_bare_chain as C
import test_gpu_decode_paths as P


def _host(stream):
    from lz4jpeg import lz4
    return lz4.decompress(bytes(stream))


@pytest.fixture(scope="module")
def path_streams(oracle):
    return P.all_streams(oracle)


@pytest.fixture(scope="module")
def chain_streams():
    return C.all_streams(C.ambiguous_pairs())


# ---- the writer against the oracle -------------------------------------------------

@pytest.mark.parametrize("name", golden_inputs.LZ4_EDGE_CASES + ["metamorphosis_spaces"])
def test_writer_reproduces_oracle_streams(oracle, name):
    """An oracle stream, parsed into sequences and written again, is the same
    bytes.  A block with 0xFD..0xFF tokens is written from the reading that
    decodes to what the host decoder returns for it."""
    data = golden_inputs.lz4_input(name)
    stream = oracle.lz4_compress(data)
    nb = (len(data) + 299) // 300
    sizes = [len(oracle.lz4_blocks(data, b, b + 1)) for b in range(nb)]
    offs = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    decoded = _host(stream)
    assert decoded == data
    blocks, ambiguous = [], 0
    for b, blk in enumerate(F.split(stream, offs)):
        last = b + 1 == nb
        want = decoded[300 * b:300 * b + 300]
        rs = list(F.readings(blk, last=last))
        ambiguous += len(rs) > 1
        seqs = next(r for r in rs if F.plain_decode(blk, r) == want)
        again, dec = F.write_block(seqs, F.literals_of(blk, seqs), last=last)
        assert again == blk, (name, b, seqs)
        assert dec == want
        blocks.append((again, dec))
    s2, o2, p2 = F.write_frame(blocks)
    assert (s2, o2, p2) == (stream, offs, data)
    if name in ("m_eq_1", "m_eq_2", "m_eq_3"):
        assert any(F.is_truncated(q) for blk, r in F.parse(stream, offs) for q in r) or ambiguous


def test_writer_refuses_what_the_format_cannot_hold():
    lits = bytes(range(256)) * 2
    bad = [
        [(10, 3, 0), (290, 0, 0)],                 # a match of length 0
        [(10, 3, 256), (34, 0, 0)],                # M = 256 is a literal in the encoder
        [(10, 3, 300)],
        [(10, 0, 4), (286, 0, 0)],                 # distance 0
        [(10, 11, 4), (286, 0, 0)],                # distance beyond the bytes produced
        [(0, 1, 4), (296, 0, 0)],
        [(200, 1, 101)],                           # 301 decoded bytes
        [(100, 0, 0)],                             # a short block that is not the last
        [(100, 0, 0), (200, 0, 0)],                # a literal-only sequence in the middle
        [(0, 0, 0)],                               # nothing decoded
    ]
    for seqs in bad:
        with pytest.raises(F.FormatError):
            F.write_block(seqs, lits)
    F.write_block([(100, 0, 0)], lits, last=True)
    # 1152 encoded bytes: 75 sequences of 5 decoded bytes cannot exceed it, so
    # the bound is met only through the check itself
    assert len(F.write_block([(1, 1, 4)] * 60, lits)[0]) <= F.BLOCK_BOUND
    with pytest.raises(F.FormatError):
        F.write_frame([(b"x", b"y" * 10), (b"x", b"y" * 300)])


def test_extension_byte_forms():
    assert F.litext(14) == b"" and F.litext(15) == b"\x00" and F.litext(269) == b"\xfe"
    assert F.litext(270) == b"\xff\x00" and F.litext(271) == b"\x00"
    blk, dec = F.write_block([(270, 9, 4), (26, 0, 0)], bytes(range(256)) * 2)
    assert blk[3:8] == bytes([0xF0, (270 + 5 + 2) & 255, 1, 0xFF, 0x00])
    blk, dec = F.write_block([(2, 1, 2), (296, 0, 0)], bytes(range(256)) * 2)
    assert blk[3:6] == bytes([0xFE, 2 + 5 + 1, 0]) and len(blk) == 3 + (3 + 2 + 2) + (3 + 1 + 296 + 2)


# ---- every built stream through the host decoder and the plain decoder --------------------

def test_host_decoder_on_decode_path_streams(path_streams):
    for st in path_streams:
        assert _host(st["stream"]) == st["plain"], st["name"]


def test_host_decoder_on_chain_streams(chain_streams):
    for st in chain_streams:
        assert _host(st["stream"]) == bytes(st["plain"]), st["name"]


def test_plain_decoder_on_built_blocks():
    for blk, dec, seqs in P.all_built_blocks():
        assert F.plain_decode(blk, seqs) == dec, seqs
    for name, seqs in P.last_blocks():
        blk, dec = F.write_block(seqs, bytes(range(1, 256)) * 2, last=True)
        assert F.plain_decode(blk, seqs) == dec, name


def test_plain_decoder_on_chain_streams(chain_streams):
    for st in chain_streams:
        plain = bytes(st["plain"])
        for b, blk in enumerate(F.split(bytes(st["stream"]), st["offs"])):
            assert F.plain_decode(blk, st["seqs"][b]) == plain[300 * b:300 * b + 300], \
                (st["name"], b)


def test_stream_parser_recovers_the_sequences(path_streams):
    """The first consistent reading (plain readings first, as the decoders
    take them) of every built block is the sequence list it was written from."""
    for st in path_streams[:2]:
        for b, (blk, seqs) in enumerate(F.parse(st["stream"], st["offs"])):
            assert F.plain_decode(blk, seqs) == st["plain"][300 * b:300 * b + 300]
    for blk, dec, seqs in P.all_built_blocks():
        assert next(F.readings(blk)) == [tuple(q) for q in seqs], seqs


# ---- what the decode-path tables cover -----------------------------------------------------

def _matches(cls):
    """(L, D, M, start, end) of every match of the class, truncated ones too."""
    out = []
    for c in P.built(cls):
        pos = 0
        for L, D, M in c["seqs"]:
            if M:
                out.append((L, D, M, pos + L, pos + L + M))
            pos += L + M
    return out


def test_match_class_coverage():
    ms = _matches("match")
    got = {(D, M) for L, D, M, q, e in ms}
    for D in P.MATCH_D:
        for M in P.MATCH_M:
            if D + M <= 300:
                assert (D, M) in got, (D, M)
    assert {D for D, M in got} >= set(P.MATCH_D)
    assert {M for L, D, M, q, e in ms if M in (254, 255)} == {254, 255}
    for D in P.MATCH_D:                                   # starts 0..3 past D
        assert {q - D for L, D2, M, q, e in ms if D2 == D and q == L} >= {0, 1, 2, 3}, D
    assert {e for L, D, M, q, e in ms} >= set(P.MATCH_ENDS)
    for e in P.MATCH_ENDS:                                # short, whole-chunk and longer copies
        here = {(D < 8, D < 16, M > 16) for L, D, M, q, end in ms if end == e}
        assert len(here) >= 4, e
    chained = 0
    for c in P.built("match"):                            # a source inside the previous match
        s = c["seqs"]
        if len(s) > 1 and s[0][2] >= 4 and s[1][2] >= 4 and s[1][0] + s[1][1] <= s[0][2]:
            chained += s[1][0] <= 1
    assert chained >= 100


def test_literal_class_coverage():
    runs, tails = set(), set()
    for c in P.built("literal"):
        L, D, M = c["seqs"][0]
        if c["name"] == "lit L0 match":                   # no literals: the second sequence
            assert c["seqs"][1][0] == 0 and c["seqs"][1][2] >= 4
            runs.add(0)
        elif c["name"].endswith("match"):
            assert D == L
            runs.add(L)
        last = c["seqs"][-1]
        if F.is_tail(last) and c["name"].endswith("tail"):
            tails.add(last[0])
    assert runs == {L for L in P.LIT_L if L + 4 <= 300}
    assert tails == {L for L in P.LIT_L if L not in (0, 299)}   # 299: as a last block only
    assert 299 in P.LAST_LEN
    wl = 12                                               # window literals with one litext byte
    assert any(L > wl + 64 for L in runs) and {270, 271} <= runs and 300 in tails
    for gate in (16, 32, 48, 64):                         # a run either side of every chunk gate
        assert {wl + gate, wl + gate + 1} <= runs


def test_ambiguous_class_coverage():
    counts = {}
    for c in P.built("ambiguous"):
        amb = [q for q in c["seqs"] if F.plain_ambiguous(q)]
        tr = any(F.is_truncated(q) for q in c["seqs"])
        for M in {q[2] for q in amb}:
            counts.setdefault((M, tr), set()).add(len(amb))
    for tr in (False, True):
        assert counts[(17, tr)] == set(range(1, 10))      # nine: the most 300 bytes hold
        assert counts[(18, tr)] == set(range(1, 10))
        assert counts[(19, tr)] == set(range(1, 9))
        assert counts[(255, tr)] == {1}
    for c in P.built("backtrack"):
        k = next(i for i, q in enumerate(c["seqs"]) if F.is_truncated(q))
        assert P.misread_is_valid(c["seqs"], k), c["name"]
        assert len(c["seqs"]) >= k + 3                    # two further sequences follow
    assert {sum(F.plain_ambiguous(q) for q in c["seqs"]) for c in P.built("backtrack")} == {0, 2, 8}


def test_truncated_and_count_coverage():
    seen, per_block, first, last = set(), set(), set(), set()
    for c in P.built("truncated"):
        tr = [i for i, q in enumerate(c["seqs"]) if F.is_truncated(q)]
        per_block.add(len(tr))
        for i in tr:
            L, D, M = c["seqs"][i]
            seen.add((M, "low" if L < 15 else "15" if L == 15 else "high" if L >= 270 else "mid"))
        if 0 in tr:
            first.add(c["seqs"][0][2])
        if len(c["seqs"]) - 1 in tr:
            last.add(c["seqs"][-1][2])
    assert seen >= {(M, k) for M in (1, 2, 3) for k in ("low", "15", "high")}
    assert per_block == {1, 2, 3} and first == {1, 2, 3} and last == {1, 2, 3}
    n = sorted(len(c["seqs"]) for c in P.built("count"))
    # the most: three truncated sequences of one byte (the first needs a
    # literal), then 4 bytes each: 2 + 1 + 1 + 74 * 4 = 300; without truncated
    # ones 5 + 73 * 4 + a tail of 3
    assert n[0] == 1 and 2 in n and 75 in n and n[-1] == 77
    assert sorted({F.decoded_len(s) for _, s in P.last_blocks()}) == P.LAST_LEN


def test_positions_of_the_blocks_under_test(oracle, path_streams):
    """Early blocks lie more than kInMax + 64 bytes before the stream end,
    tail blocks within it; the early+trunc form holds a truncated sequence."""
    n_early = n_tail = 0
    for st in path_streams:
        if "under" not in st:
            continue
        beg = [1 + st["offs"][b] for b in st["under"]]
        if " early" in st["name"]:
            assert all(x + P.IN_SAFE <= len(st["stream"]) for x in beg), st["name"]
            n_early += len(beg)
        else:
            assert all(x + P.IN_SAFE > len(st["stream"]) for x in beg), st["name"]
            n_tail += len(beg)
    total = sum(len(P.built(cls)) for cls in P.CLASSES)
    assert n_tail == total and n_early >= total
    for cls in P.CLASSES:
        for c in P.built(cls):
            if c["tseqs"] is not None:
                assert any(F.is_truncated(q) for q in c["tseqs"])
                assert not any(F.is_truncated(q) for q in c["seqs"])
            else:                                         # none fits, or it has its own
                assert any(F.is_truncated(q) for q in c["seqs"]) or c["where"] is None


# ---- what the chain streams claim -------------------------------------------------------------

def test_candidate_rule_on_true_blocks(oracle):
    """The rule passes at every true block start of an oracle stream without
    truncated sequences, and the fast chain of such a stream is consistent."""
    data = golden_inputs.lz4_input("metamorphosis_spaces:40000")
    stream = oracle.lz4_compress(data)
    offs = F.walk_offsets(stream)
    assert len(offs) == (len(data) + 299) // 300
    for c in range(1, F.nchunks(stream)):
        t = F.first_start(offs, c)
        assert F.candidate_at(stream, c, t - 1 - c * F.CHUNK)
        assert F.first_candidate(stream, c) <= t
    cand, ex, mis = F.fast_chain(stream)
    assert all(c in [1 + o for o in offs] for c in cand) and mis == []


def test_chain_streams_hold_what_they_claim(chain_streams):
    by = {st["name"]: st for st in chain_streams}
    for st in chain_streams:
        s = bytes(st["stream"])
        falses = C.false_chunks(st)
        if "inconsistent" not in st["name"]:
            assert falses == sorted(st["false"]), st["name"]
        for c in st["trunc_first"]:                       # the candidate skips the truncated block
            t = F.first_start(st["offs"], c)
            assert st["kinds"][st["offs"].index(t - 1)] == "trunc"
            assert F.first_candidate(s, c) == 1 + st["offs"][st["offs"].index(t - 1) + 1]
        has_trunc = any(F.is_truncated(q) for seqs in st["seqs"] for q in seqs)
        if not has_trunc:
            assert F.walk_offsets(s) == st["offs"], st["name"]     # the fast pass can succeed
        else:
            with pytest.raises((F.FormatError, IndexError)):
                assert F.walk_offsets(s) != st["offs"]
    # chunk geometry
    e = by["starts at chunk edges -1 0 +1"]
    starts = {1 + o for o in e["offs"]}
    assert {F.CHUNK, 1 + 2 * F.CHUNK, 2 + 3 * F.CHUNK} <= starts
    assert {len(by[f"stream ends {d:+d} past a chunk"]["stream"]) - 1 - 2 * F.CHUNK
            for d in (-1, 0, 1, 2)} == {-1, 0, 1, 2}
    assert {F.nchunks(st["stream"]) for st in chain_streams} >= {1, 63, 64, 65}
    # dying and rejoining false chains, in chunk 1, in neighbours, last, after a repair
    for kind in ("dies", "rejoins"):
        for what, chunks in (("chunk 1", [1]), ("chunks 1 and 2", [1, 2]), ("last chunk", [5]),
                             ("after a repaired chunk, and apart", [1, 2, 3, 5])):
            st = by[f"false candidate, {kind}: {what}"]
            s = bytes(st["stream"])
            assert st["false"] == chunks and F.nchunks(s) == 6
            for c in chunks:
                ex, starts = F.fast_walk(s, c, F.first_candidate(s, c))
                if kind == "dies":
                    assert ex == F.BAD
                else:
                    true_ex = F.fast_walk(s, c, F.first_start(st["offs"], c))[0]
                    assert ex == true_ex and len(starts) > 2
    # list and staging limits
    assert C.starts_per_chunk(by["32 block starts in a chunk"])[1] == C.K_LIST
    assert C.starts_per_chunk(by["33 block starts in a chunk"])[1] == C.K_LIST + 1
    for n in (1023, 1024, 1025):
        st = by[f"{n} blocks in one wave of chunks, hundreds in a chunk"]
        assert len(st["offs"]) == n
    st = by["64 chunks"]
    assert len([o for o in st["offs"] if o < 64 * F.CHUNK]) > C.K_STAGE
    st = by["a re-walked chunk over the list limit"]
    per = C.starts_per_chunk(st)
    assert all(per[c] > C.K_LIST for c in st["false"])
    # the first pass's inconsistent chunks at the list's limit and past it
    for target in C.MANY:
        st = by[f"{target} inconsistent chunks"]
        falses, mis = C.false_chunks(st), F.fast_chain(bytes(st["stream"]))[2]
        if target == "apart":                             # pairs that do not touch
            assert len(mis) == 2 * len(falses) > C.K_MIS + 50
            assert all(b - a >= 2 for a, b in zip(falses, falses[1:]))
        else:
            assert len(falses) == target and len(mis) == target
            assert len(st["false"]) >= 1000
        assert 9_000_000 < len(st["stream"]) < 9_400_000


# ---- oracle identity ------------------------------------------------------------------------

_same = {}


def _oracle_identical(oracle, blocks):
    """How many (block, decoded) pairs the oracle encodes to the same bytes
    (equal blocks are asked about once)."""
    n = 0
    for b, d in blocks:
        if b not in _same:
            _same[b] = oracle.lz4_blocks(d, 0, 1) == b
        n += _same[b]
    return n


def _oracle_identical_all(oracle, blocks):
    """Does the oracle encode every pair to the same bytes?  A call per
    thread over a share of the blocks."""
    from concurrent.futures import ThreadPoolExecutor

    def one(part):
        data = b"".join(d for _, d in part)
        return oracle.lz4_blocks(data, 0, len(part)) == b"".join(b for b, _ in part)

    step = max(1, (len(blocks) + 7) // 8)
    with ThreadPoolExecutor(8) as ex:
        return all(ex.map(one, [blocks[i:i + step] for i in range(0, len(blocks), step)]))


def test_oracle_identity_reported(oracle, chain_streams, capsys):
    """Reported, not required: how many built blocks the exhaustive
    longest-match encoder reproduces from their plaintext.  Required for the
    literal-only blocks of the chain streams, whose 4-grams never repeat."""
    pairs = [(blk, dec) for blk, dec, _ in P.all_built_blocks()]
    same_p, total_p = _oracle_identical(oracle, pairs), len(pairs)
    same = total = 0
    lit, lit_total = {}, 0
    for st in chain_streams:
        blks = F.split(bytes(st["stream"]), st["offs"])
        plain = bytes(st["plain"])
        rest = []
        for b, k in enumerate(st["kinds"]):
            d = plain[300 * b:300 * b + 300]
            if k == "lit":
                lit[blks[b]] = d
                lit_total += 1
            elif len(d) == 300:
                rest.append((blks[b], d))
        same, total = same + _oracle_identical(oracle, rest), total + len(rest)
    lit = list(lit.items())
    assert all(len(d) == 300 and _no_repeat(d) for _, d in lit)
    assert _oracle_identical_all(oracle, lit)
    with capsys.disabled():
        print(f"\noracle identity: {same_p} of {total_p} decode-path blocks "
              f"({100 * same_p / total_p:.1f} %), {same} of {total} other chain-stream blocks "
              f"({100 * same / total:.1f} %), all {lit_total} literal-only chain-stream blocks")


def _no_repeat(d):
    a = np.frombuffer(d, dtype=np.uint8).astype(np.uint32)
    g = a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24
    return np.unique(g).size == g.size
