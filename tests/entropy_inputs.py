"""Input builders for the entropy stage's wave-level paths
(tests/test_gpu_entropy_paths.py; what they reach is checked on the CPU by
tests/test_entropy_inputs.py).  No GPU, no torch.

csrc/jpegr_entropy.hip maps one lane to one stream and takes several
decisions per wave by ballot: the encoder's sift depths from the wave's
largest distinct-symbol count, the deferred encoder's share of kSlots working
sets, the decoder's lookup method and refill cadence from the wave's longest
code.  Images and round trips of the encoder's own output reach a narrow band
of those (random luma: 10..21 symbols, codes of 5..8 bits).  The builders here
place chosen streams in chosen lanes:

  tile t is lane t % 64 of luma wave t // 64; its Cr stream is in chroma
  wave 2 (t // 64), its Cb stream in chroma wave 2 (t // 64) + 1.

Encoder batches are int16 coefficients (any int16 is valid input); decoder
batches are bits / meta / table arrays written here from a chosen code table
and a chosen RLE list, with the expected ints computed from that list alone.
Every crafted stream is well-formed: it lies inside its slot and its rle_len
is its number of codes.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle_api

LANES = 64
N = (64, 32, 32)                      # ints per stream: Y, Cr, Cb
COEF_OFF = (0, 64, 96)                # of a tile's 128 coefficients
SLOT_OFF = (0, 128, 192)              # bytes of a tile's 256 (bits), entries (table)
SLOT_BITS = (1024, 512, 512)
CAP = (24, 12, 12)                    # distinct symbols of the fast encoder / decoder
KEY_LO = (-64, -48, -48)              # the fast encoder's direct symbol table
KEY_HI = (111, 71, 71)
KSLOTS = 6                            # working sets of the deferred encoder per wave
CHANNELS = ("Y", "Cr", "Cb")
STYLES = ("ties", "dominant", "fib")


# ---- RLE lists ---------------------------------------------------------------
def expand(pairs, n):
    """The n ints whose RLE is `pairs` [(count, value)]: adjacent runs differ."""
    assert sum(c for c, _ in pairs) == n and all(c >= 1 for c, _ in pairs), pairs
    assert all(a[1] != b[1] for a, b in zip(pairs, pairs[1:])), pairs
    out = []
    for c, v in pairs:
        out += [v] * c
    return out


def rle_of(zz):
    """[(count, value)] of a stream (the reference's RLE, restated)."""
    pairs = []
    for v in zz:
        v = int(v)
        if pairs and pairs[-1][1] == v:
            pairs[-1][0] += 1
        else:
            pairs.append([1, v])
    return [tuple(p) for p in pairs]


def distinct(pairs):
    """U: distinct ints among counts and values together."""
    return len({x for p in pairs for x in p})


def is_deferred(zz, c):
    """The fast encoder's rule: more than 24 / 12 distinct symbols, or a
    symbol outside -64..111 / -48..71."""
    pairs = rle_of(zz)
    syms = {x for p in pairs for x in p}
    return len(syms) > CAP[c] or min(syms) < KEY_LO[c] or max(syms) > KEY_HI[c]


def _arrange(freq):
    """A sequence holding symbol s freq[s] times, no two neighbours equal."""
    items = sorted(freq.items(), key=lambda kv: -kv[1])
    r = sum(freq.values())
    assert items[0][1] <= (r + 1) // 2, freq
    seq, pos = [None] * r, 0
    for s, k in items:
        for _ in range(k):
            seq[pos] = s
            pos += 2
            if pos >= r:
                pos = 1
    return seq


def _pick_values(rng, c, k, exclude):
    pool = [v for v in range(KEY_LO[c], KEY_HI[c] + 1) if v not in exclude]
    return [int(x) for x in rng.choice(pool, size=k, replace=False)]


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def pairs_with_u(c, U, style, rng):
    """An RLE list of a whole stream of channel c with exactly U distinct
    symbols, all inside the fast encoder's key range.  style shapes the
    symbol frequencies that the Huffman heap sees:
      ties      every symbol once (one twice when U is odd): the heap's
                strict-<, left-first rule decides every comparison
      dominant  one value in every other run
      fib       value frequencies 1, 1, 2, 3, 5, ...: a deep tree
    U = 1 is the run of n copies of n."""
    n = N[c]
    if U == 1:
        return [(n, n)]
    if style == "ties":
        r = (U + 1) // 2                                # runs: distinct counts 1..r-1 and the rest
        last = n - r * (r - 1) // 2
        if last >= r:
            counts = list(range(1, r)) + [last]
            vals = _pick_values(rng, c, U - r, set(counts))
            vals += counts[:r - len(vals)]              # odd U: one count is also a value
            counts = [counts[i] for i in rng.permutation(r)]
            vals = [vals[i] for i in rng.permutation(r)]
            pairs = list(zip(counts, vals))
            assert distinct(pairs) == U
            return pairs
    # counts from 1..a, U - a other symbols as values
    a = int(rng.integers(1, min(3, U - 1) + 1))
    B = _pick_values(rng, c, U - a, set(range(1, a + 1)))
    V = B if len(B) >= 2 else B + [1]
    rmin = max(len(V), a - (-(n - a * (a + 1) // 2) // a))    # 1..a once each, the rest <= a
    rmax = n - a * (a + 1) // 2 + a
    r = int(rng.integers(rmin, rmax + 1))
    counts = list(range(1, a + 1)) + [1] * (r - a)
    for _ in range(n - sum(counts)):
        room = [i for i in range(a, r) if counts[i] < a]
        counts[room[int(rng.integers(len(room)))]] += 1
    counts = [counts[i] for i in rng.permutation(r)]
    cap = (r + 1) // 2
    freq = {s: 1 for s in V}
    left = r - len(V)
    if style == "dominant":
        k = min(cap - 1, left)
        freq[V[0]] += k
        left -= k
        weights = [0] + [1] * (len(V) - 1)
    elif style == "fib":
        weights = _fib(len(V))
    else:
        weights = [1] * len(V)
    order = sorted(range(len(V)), key=lambda i: -weights[i])
    total = sum(weights) or 1
    for i in order:                                     # the weighted share, below the cap
        k = min(cap - freq[V[i]], left * weights[i] // total)
        freq[V[i]] += k
    left = r - sum(freq.values())
    i = 0
    while left:                                         # the remainder, round robin
        s = V[order[i % len(V)]]
        if freq[s] < cap:
            freq[s] += 1
            left -= 1
        i += 1
    pairs = list(zip(counts, _arrange(freq)))
    assert distinct(pairs) == U, (U, pairs)
    return pairs


def deferred_pairs(c, cause, rng, flip):
    """A stream that the fast encoder defers: by U = cap + 1, or by one value
    just outside the key range (flip: the low or the high side)."""
    if cause == "U":
        return pairs_with_u(c, CAP[c] + 1, STYLES[int(rng.integers(3))], rng)
    pairs = pairs_with_u(c, int(rng.integers(2, 9)), STYLES[int(rng.integers(3))], rng)
    k = int(rng.integers(len(pairs)))
    pairs[k] = (pairs[k][0], KEY_HI[c] + 1 if flip else KEY_LO[c] - 1)
    return pairs


# ---- encoder batches ------------------------------------------------------------
# coef: [ntiles, 128] int16; claims: {(kind, wave): {...}} with kind "luma" or
# "chroma" and the wave numbering of the module docstring.  Claim keys: umax
# (largest U of the wave), deferred (lanes the fast encoder defers), u_set.
Batch = namedtuple("Batch", "name coef claims")


def _put(coef, t, c, zz):
    coef[t, COEF_OFF[c]:COEF_OFF[c] + N[c]] = zz


def _wave(g, c):
    return ("luma", g) if c == 0 else ("chroma", 2 * g + c - 1)


def _plain(c, rng):
    """An ordinary stream: U drawn from 1..cap, never deferred."""
    U = int(rng.integers(1, CAP[c] + 1))
    return expand(pairs_with_u(c, U, STYLES[int(rng.integers(3))], rng), N[c])


def umax_sweep():
    """tree_codes' uniform sift depths: the wave's umax takes every value 1..26
    (luma; 1..14 chroma, Cr and Cb apart), which moves the merge loop's phase
    bounds (>= 16 / 8 / 4) and build_heap_from's I < umax / 2 through every
    case; lane 0 holds the maximum, lane 1 a one-symbol stream, the others
    1..min(m, cap) under three count distributions."""
    rng = np.random.default_rng(101)
    groups = 26
    coef = np.zeros((groups * LANES, 128), np.int16)
    claims = {}
    for g in range(groups):
        for c, m in enumerate((g + 1, 1 + g % 14, 1 + (g + 5) % 14)):
            for lane in range(LANES):
                U = m if lane == 0 else 1 if lane == 1 else int(rng.integers(1, min(m, CAP[c]) + 1))
                style = STYLES[(lane + g + c) % 3]
                _put(coef, g * LANES + lane, c, expand(pairs_with_u(c, U, style, rng), N[c]))
            claims[_wave(g, c)] = {"umax": m, "deferred": int(m > CAP[c])}
    return Batch("umax_sweep", coef, claims)


def u_ladder():
    """Lanes of one wave on every heap size at once: every U from 1 to the cap
    in ascending, descending and shuffled lane order, so each lane's own
    I < U / 2 and size tests differ from its neighbours' under one umax."""
    rng = np.random.default_rng(102)
    coef = np.zeros((3 * LANES, 128), np.int16)
    claims = {}
    for g in range(3):
        for c in range(3):
            us = [1 + i % CAP[c] for i in range(LANES)]
            if g == 1:
                us = us[::-1]
            elif g == 2:
                us = [us[i] for i in rng.permutation(LANES)]
            for lane, U in enumerate(us):
                _put(coef, g * LANES + lane, c,
                     expand(pairs_with_u(c, U, STYLES[(lane // CAP[c]) % 3], rng), N[c]))
            claims[_wave(g, c)] = {"umax": CAP[c], "deferred": 0,
                                   "u_set": list(range(1, CAP[c] + 1))}
    return Batch("u_ladder", coef, claims)


DEFER_COUNTS = (0, 1, 5, 6, 7, 13, 64)
CHROMA_DEFERS = ((0, 7), (1, 0), (7, 1))              # (Cr, Cb) deferred lanes per variant


def _defer_lanes(rng, k):
    return {int(x) for x in rng.permutation(LANES)[:k]}


def deferral():
    """The deferred encoder's list and slot arithmetic: luma waves with 0, 1,
    5, 6, 7, 13 and 64 deferred lanes (around kSlots = 6), deferred once by
    U = 25 and once by a value one past the key range, each beside chroma waves
    with 0, 1 and 7 deferred lanes of their own, so the even chroma wave works
    through its own list and then the luma wave's."""
    rng = np.random.default_rng(103)
    combos = [(d, cause, v) for d in DEFER_COUNTS for cause in ("U", "value") for v in range(3)]
    coef = np.zeros((len(combos) * LANES, 128), np.int16)
    claims = {}
    for g, (d, cause, v) in enumerate(combos):
        for c, k in enumerate((d,) + CHROMA_DEFERS[v]):
            lanes = _defer_lanes(rng, k)
            for lane in range(LANES):
                if lane in lanes:
                    why = cause if c == 0 else ("U", "value")[(lane + g) & 1]
                    zz = expand(deferred_pairs(c, why, rng, (lane + g) & 2), N[c])
                else:
                    zz = _plain(c, rng)
                _put(coef, g * LANES + lane, c, zz)
            claims[_wave(g, c)] = {"deferred": k}
    return Batch("deferral", coef, claims)


SIZES = (1, 3, 63, 64, 65, 67, 129)


def sized(ntiles, defer_last):
    """The last, partial wave: ntiles of 1, 3, 63, 64, 65, 67, 129; with
    defer_last every live lane of the last wave defers on all three channels
    (1 and 3 live lanes: fewer than kSlots, so the share is min(kSlots, live
    lanes)), without it no lane defers."""
    rng = np.random.default_rng(1040 + 2 * ntiles + defer_last)
    coef = np.zeros((ntiles, 128), np.int16)
    claims = {}
    last = (ntiles - 1) // LANES
    for g in range(last + 1):
        live = min(LANES, ntiles - g * LANES)
        for c in range(3):
            for lane in range(live):
                if defer_last and g == last:
                    zz = expand(deferred_pairs(c, ("U", "value")[lane & 1], rng, lane & 2), N[c])
                else:
                    zz = _plain(c, rng)
                _put(coef, g * LANES + lane, c, zz)
            claims[_wave(g, c)] = {"deferred": live if defer_last and g == last else 0,
                                   "live": live}
    return Batch(f"size{ntiles}_{'defer' if defer_last else 'plain'}", coef, claims)


WIDE_VALUES = (-32768, 32767, 1024, -1024, 1023, -1023, -1025, 0)
KEY_EDGES = ((-65, 112, -64, 111), (-49, 72, -48, 71))          # luma, chroma


def values():
    """The int16 range and the key-range edges: -32768, 32767, +-1024, +-1023,
    -1025, 0, counts equal to values.  Streams with a wide value take the hashed
    encoder and decode_stream_slow (the fast decoder keeps 11-bit values)."""
    def streams(n):
        h = n // 2
        eq = [v for k in (3, 2, 1, 5, 4, 7) for v in [k] * k]            # 22 ints, counts == values
        out = [[-32768] + [32767] * (n - 1),
               [WIDE_VALUES[i % 8] for i in range(n)],
               [v for v in WIDE_VALUES for _ in range(n // 8)],
               eq + [0] * (n - len(eq)),
               [0] * n,
               [1024] * h + [-1025] * h,
               [1023, -1024] * h,
               [-1023] * 3 + [3] * 3 + [-1024] * (n - 6)]
        return out
    luma = streams(64) + [[-64, 111] * 32, [-65] + [0] * 63, [112] + [1] * 63]
    chroma = streams(32) + [[-48, 71] * 16, [-49] + [0] * 31, [72] + [1] * 31]
    nt = len(luma)
    coef = np.zeros((nt, 128), np.int16)
    for t in range(nt):
        _put(coef, t, 0, luma[t])
        _put(coef, t, 1, chroma[t])
        _put(coef, t, 2, chroma[(t + 3) % nt])
    return Batch("values", coef, {})


def encoder_batch_names():
    names = ["umax_sweep", "u_ladder", "deferral", "values"]
    names += [f"size{n}_{k}" for n in SIZES for k in ("defer", "plain")]
    return names


@functools.lru_cache(maxsize=None)
def encoder_batch(name):
    if name.startswith("size"):
        n, kind = name[4:].split("_")
        b = sized(int(n), kind == "defer")
    else:
        b = {"umax_sweep": umax_sweep, "u_ladder": u_ladder, "deferral": deferral,
             "values": values}[name]()
    b.coef.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def oracle_streams(oracle, name):
    """oracle_api.entropy of every stream of an encoder batch, [tile][channel],
    computed once per batch."""
    coef = encoder_batch(name).coef
    return [[oracle_api.entropy(oracle, coef[t, COEF_OFF[c]:COEF_OFF[c] + N[c]])
             for c in range(3)] for t in range(coef.shape[0])]


# ---- crafted decoder streams -------------------------------------------------
def codes_from_lengths(lens):
    """The header's rule: code[0] = 0, code[k] = (code[k-1] + 1) shifted to len[k]."""
    out, code, plen = [], 0, 0
    for k, L in enumerate(lens):
        if k:
            code = (code + 1) << (L - plen) if L >= plen else (code + 1) >> (plen - L)
        plen = L
        out.append(code)
    return out


def left_aligned(lens):
    """The codes left-aligned in 32 bits; asserts that they fit their lengths
    and increase strictly (a table the header promises to decode)."""
    codes = codes_from_lengths(lens)
    la = [co << (32 - L) for co, L in zip(codes, lens)]
    assert all(1 <= L <= 32 and co < (1 << L) for co, L in zip(codes, lens)), lens
    assert all(a < b for a, b in zip(la, la[1:])), lens
    return la


def tree_lengths(U, lmax, rng):
    """DFS leaf depths of a random full binary tree with U leaves whose deepest
    leaf is at exactly lmax (U >= lmax + 1)."""
    assert U >= lmax + 1
    lens = [0]
    while max(lens) < lmax:                              # a spine down to lmax
        deepest = [i for i, d in enumerate(lens) if d == max(lens)]
        i = deepest[int(rng.integers(len(deepest)))]
        lens[i:i + 1] = [lens[i] + 1] * 2
    while len(lens) < U:
        room = [i for i, d in enumerate(lens) if d < lmax]
        i = room[int(rng.integers(len(room)))]
        lens[i:i + 1] = [lens[i] + 1] * 2
    return lens


def unary_lengths(U):
    """1, 2, ..., U - 1, U - 1: the deepest tree of U leaves."""
    return list(range(1, U)) + [U - 1]


def chain_lengths(d, L, k):
    """1, 2, ..., d, then k codes of L bits under the prefix of d ones (a
    sparse table: not a full tree, but its codes follow the rule)."""
    return list(range(1, d + 1)) + [L] * k


def inverse_rle(syms, n):
    """The ints that the RLE list stands for: counts clamped to n (zero and
    negative counts give nothing), zero fill.  From the list alone."""
    out = np.zeros(n, np.int16)
    idx = 0
    for i in range(0, len(syms) - 1, 2):
        cnt = min(int(syms[i]), n - idx)
        if cnt > 0:
            out[idx:idx + cnt] = syms[i + 1]
            idx += cnt
    return out


# table: [(value, length)]; codes: right-aligned ints; syms: the RLE list;
# bits: the whole slot's bytes; tail: bytes past the bits are not zero;
# starts: bit offset of every code
Stream = namedtuple("Stream", "c table codes syms nbits bits expected tag tail starts")


def craft(c, table, syms, tag="", tail=False):
    """Concatenate the codes of `syms` MSB-first into channel c's slot."""
    vals = [v for v, _ in table]
    lens = [L for _, L in table]
    assert len(set(vals)) == len(vals) and 1 <= len(table) <= 2 * N[c], table
    assert 1 <= len(syms) <= 2 * N[c]
    if len(table) == 1:
        assert lens == [0] and set(syms) == {vals[0]}
        codes = [0]
    else:
        left_aligned(lens)
        codes = codes_from_lengths(lens)
    at = {v: k for k, v in enumerate(vals)}
    acc, nb, starts = 0, 0, []
    for s in syms:
        k = at[int(s)]
        starts.append(nb)
        acc = (acc << lens[k]) | codes[k]
        nb += lens[k]
    cap = SLOT_BITS[c]
    assert nb <= cap, (tag, nb)
    raw = bytearray((acc << (cap - nb)).to_bytes(cap // 8, "big"))
    if tail:                                            # "bytes past it unspecified"
        for i in range((nb + 7) // 8, cap // 8):
            raw[i] = 0xA5 ^ (i * 29 & 0xFF)
    return Stream(c, [(int(v), int(L)) for v, L in table], codes, [int(s) for s in syms], nb,
                  bytes(raw), inverse_rle(syms, N[c]), tag, tail, starts)


def stream_class(s):
    """Where jpegr_entropy_decode_device sends the stream: "slow" (more codes
    than the cap, a value outside -1024..1023 or a code over 31 bits), "one"
    (a single code) or "fast" (the lanes that vote on lookup and cadence)."""
    if len(s.table) > CAP[s.c] or any(L > 31 or not -1024 <= v <= 1023 for v, L in s.table):
        return "slow"
    return "one" if len(s.table) == 1 else "fast"


def lmax(s):
    return max(L for _, L in s.table)


def from_encoder(oracle, c, zz, tag="encoder"):
    """The encoder's own stream for zz (by the oracle), through craft."""
    e = oracle_api.entropy(oracle, np.asarray(zz, np.int16))
    s = craft(c, [(v, L) for v, L, _ in e["table"]], e["rle"], tag)
    assert s.nbits == e["nbits"] and s.bits[:(s.nbits + 7) // 8] == e["bits"]
    assert s.expected.tolist() == [int(v) for v in zz]
    return s


def table_values(lens, rng, extra=()):
    """Distinct values for a table: the two longest codes get small positive
    values (so a long code is a count and the next long code its value),
    `extra` values are placed on random codes, the rest are small ints."""
    k = len(lens)
    order = sorted(range(k), key=lambda i: -lens[i])
    vals = [None] * k
    small = [1, 2, 3]
    for i, v in zip(order, small):
        vals[i] = v
    free = [i for i in range(k) if vals[i] is None]
    free = [free[i] for i in rng.permutation(len(free))]
    for i, v in zip(free, extra):
        vals[i] = v
    pool = [v for v in range(-20, 41) if v not in small and v not in extra]
    fill = rng.choice(pool, size=k, replace=False)
    j = 0
    for i in range(k):
        if vals[i] is None:
            vals[i] = int(fill[j])
            j += 1
    return list(zip(vals, lens))


def random_syms(c, table, rng, max_bits=None, max_r=None):
    """A random RLE list over the table inside the slot: it opens with the two
    longest codes back to back, counts are mostly 1..4 (so many pairs land in
    the row), now and then any value of the table: 0, negative, or past the
    row's end."""
    max_bits = SLOT_BITS[c] if max_bits is None else max_bits
    max_r = 2 * N[c] if max_r is None else max_r
    lens = {v: L for v, L in table}
    vals = [v for v, _ in table]
    by_len = sorted(vals, key=lambda v: -lens[v])
    small = [v for v in vals if 1 <= v <= 4]
    syms, nb = [by_len[0], by_len[1]], lens[by_len[0]] + lens[by_len[1]]
    assert nb <= max_bits
    misses = 0
    while misses < 8 and len(syms) + 2 <= max_r:
        cnt = small[int(rng.integers(len(small)))] if rng.random() < 0.8 else \
            vals[int(rng.integers(len(vals)))]
        v = vals[int(rng.integers(len(vals)))]
        if nb + lens[cnt] + lens[v] > max_bits:
            misses += 1
            continue
        syms += [cnt, v]
        nb += lens[cnt] + lens[v]
    return syms


def random_stream(c, lens, rng, tag, extra=(), **kw):
    table = table_values(lens, rng, extra)
    return craft(c, table, random_syms(c, table, rng, **kw), tag, tail=bool(rng.integers(2)))


def position_stream(c, L, total, tag):
    """Codes of L bits back to back to the very end of `total` bits, after a
    lead of 1-, 2- and (L - 1)-bit codes chosen so that the stream has exactly
    `total` bits and an even number of codes inside the rle_len limit (None
    where 2 n codes of at most L bits cannot reach `total`): the last code ends
    on the stream's last bit, and the L-bit codes straddle the slot's 16-byte
    chunks."""
    lens = [1, 2, L - 1, L, L, L]
    table = list(zip([3, 0, 6, 1, 2, -2], lens))
    for a in range(total // L, 0, -1):
        for z in range(3):
            for y in range(3):
                x = total - a * L - z * (L - 1) - 2 * y
                if x >= 0 and (a + x + y + z) % 2 == 0 and a + x + y + z <= 2 * N[c]:
                    longs = [(1, 2, 1, -2, 2, 1, 1)[i % 7] for i in range(a)]
                    return craft(c, table, [3] * x + [0] * y + [6] * z + longs, tag)
    return None                                          # too many codes for rle_len


def lead_stream(c, L, lead, tag):
    """`lead` one-bit codes, then L-bit codes back to back while they fit."""
    lens = [1, 2, L - 1, L, L, L]
    table = list(zip([3, 0, 6, 1, 2, -2], lens))
    a = min((SLOT_BITS[c] - lead) // L, 2 * N[c] - lead)
    a -= (a + lead) % 2
    longs = [(2, 1, 1, -2, 1, 2, 1)[i % 7] for i in range(a)]
    return craft(c, table, [3] * lead + longs, tag)


def _noise(oracle, c, rng):
    """An encoder-made stream of small ints (codes of at most 8 bits)."""
    return from_encoder(oracle, c, rng.integers(-3, 4, size=N[c]))


def _position_set(c, L):
    cap = SLOT_BITS[c]
    out = [lead_stream(c, L, lead, f"position lead {lead} L {L}") for lead in (0, 1, 31, 32)]
    out += [position_stream(c, L, cap, f"full slot L {L}"),
            position_stream(c, L, cap - 1, f"slot less one bit L {L}")]
    return [s for s in out if s is not None]


def _sparse(c, lens, rng, tag):
    """A sparse table's stream: values 1, 2 (, 3) on its codes."""
    table = list(zip([2, 1, 3][:len(lens)], lens))
    syms = []
    nb = 0
    L = {v: n for v, n in table}
    vals = [v for v, _ in table]
    while len(syms) + 2 <= 2 * N[c]:
        a, b = vals[int(rng.integers(len(vals)))], vals[int(rng.integers(len(vals)))]
        if len(syms) < 2:
            a = b = vals[-1]                              # the longest code twice, first
        if nb + L[a] + L[b] > SLOT_BITS[c]:
            break
        syms += [a, b]
        nb += L[a] + L[b]
    return craft(c, table, syms, tag)


# the tables of each longest-code class, per channel kind (0: luma, 1: chroma)
def _class_tables(kind, cls, rng):
    cap = CAP[kind]
    if cls == "narrow":                                  # longest code <= 8 bits
        t = [("tree lmax 8", tree_lengths(cap, 8, rng)), ("unary lmax 8", unary_lengths(9)),
             ("tree lmax 5", tree_lengths(cap, 5, rng)), ("tree lmax 7", tree_lengths(8, 7, rng)),
             ("two codes", [1, 1]), ("chain 8", chain_lengths(4, 8, 8))]
    elif cls == "mid":                                   # 9..16 bits
        t = [("tree lmax 9", tree_lengths(cap, 9, rng)), ("sparse 1 9", [1, 9]),
             ("sparse 1 16", [1, 16]), ("chain 16", chain_lengths(8, 16, 4)),
             ("chain 9", chain_lengths(3, 9, cap - 3)), ("unary", unary_lengths(min(cap, 17)))]
        if kind == 0:
            t += [("tree lmax 16", tree_lengths(cap, 16, rng)),
                  ("tree lmax 12", tree_lengths(cap, 12, rng))]
    else:                                                # 17..31 bits
        t = [("sparse 1 17", [1, 17]), ("sparse 2 31 31", [2, 31, 31]),
             ("chain 17", chain_lengths(8, 17, 4)), ("chain 31", chain_lengths(8, 31, 4)),
             ("chain 24", chain_lengths(cap - 4, 24, 4))]
        if kind == 0:
            t += [("unary lmax 23", unary_lengths(24)), ("tree lmax 17", tree_lengths(cap, 17, rng)),
                  ("chain 31 of 24", chain_lengths(20, 31, 4))]
    return t


CLASS_LEN = {"narrow": 8, "mid": 16, "long": 31}
CLASS_LEN2 = {"narrow": 7, "mid": 9, "long": 17}
EDGE_VALUES = (-1024, 1023)                              # the fast decoder's 11-bit values


def _class_lanes(kind_c, cls, rng):
    """64 fast-path streams of channel kind_c whose longest codes are all of
    class cls: each class table with random symbols, the position and full-slot
    streams at the class's longest and shortest lengths.  Targets decode_stream's
    two ballots: a narrow luma wave looks symbols up in the start map, every
    other wave with count_above, and the wave refills once per four, two or
    one symbol(s); the position streams put a long code on every refill and
    16-byte chunk boundary of that cadence."""
    c = kind_c
    lanes = []
    for tag, lens in _class_tables(min(c, 1), cls, rng):
        if len(lens) <= 3:
            lanes.append(_sparse(c, lens, rng, tag))
        else:
            extra = EDGE_VALUES if len(lens) >= 8 else ()
            lanes.append(random_stream(c, lens, rng, tag, extra))
            lanes.append(random_stream(c, lens, rng, tag + " again"))
    lanes += _position_set(c, CLASS_LEN[cls]) + _position_set(c, CLASS_LEN2[cls])
    tabs = [t for t in _class_tables(min(c, 1), cls, rng) if len(t[1]) > 3]
    while len(lanes) < LANES:
        tag, lens = tabs[len(lanes) % len(tabs)]
        lanes.append(random_stream(c, lens, rng, tag + " fill"))
    assert len(lanes) == LANES
    return [lanes[i] for i in rng.permutation(LANES)]


def _single_lanes(oracle, c, lane, lens, rng, tag):
    """Encoder-made streams in every lane but one, which holds `lens`: one
    lane's longest code must switch the whole wave's lookup and cadence
    (__ballot(lmax > 8), __ballot(lmax > 16)), wherever the lane sits."""
    lanes = [_noise(oracle, c, rng) for _ in range(LANES)]
    lanes[lane] = _sparse(c, lens, rng, tag) if len(lens) <= 3 else \
        random_stream(c, lens, rng, tag, EDGE_VALUES if len(lens) >= 8 else ())
    return lanes


def _slow_table(c, rng, kind):
    """Tables that decode_stream_slow takes (U > cap, a value outside the u16
    entries' 11 bits, a 32-bit code)."""
    if kind == "many":                                   # U > cap: a full tree of 2 cap leaves
        lens = tree_lengths(2 * CAP[c], 7, rng)
        return table_values(lens, rng)
    if kind == "all":                                    # every table entry of the slot used
        lens = [6 if c else 7] * (2 * N[c])
        return list(zip(range(-N[c], N[c]), lens))
    if kind == "unary32":                                # U = 32, longest code 31 bits
        return table_values(unary_lengths(32), rng)
    if kind == "code32":                                 # a 32-bit code
        return [(1, 1), (2, 32)]
    lens = tree_lengths(8, 5, rng)                       # wide values, few codes
    return table_values(lens, rng, extra=(-1025, 1024, 32767, -32767, -32768))


def _mix_lanes(oracle, c, rng):
    """Fast lanes beside U > cap lanes, wide-value lanes, a 32-bit code and
    one-code streams: decode_stream's ballots run with part of the wave on the
    slow path or past them, and decode_stream_slow sees every kind of table,
    with negative and oversized counts."""
    lanes = []
    for i in range(LANES):
        k = i % 8
        if k in (0, 5):
            lanes.append(_noise(oracle, c, rng))
        elif k == 1:
            t = _slow_table(c, rng, ("many", "all", "unary32")[(i // 8) % 3])
            lanes.append(craft(c, t, random_syms(c, t, rng), "slow: U over the cap"))
        elif k == 2:
            t = _slow_table(c, rng, "wide")
            syms = random_syms(c, t, rng, SLOT_BITS[c] - 40, 2 * N[c] - 8)
            # wide values as counts too: a negative count gives nothing, a huge one is clamped
            syms += [(-1025, 1024, -32768, 32767)[(i // 8) % 4], 3, 2, -32767, 1, 32767, 2, -1025]
            lanes.append(craft(c, t, syms, "slow: wide values"))
        elif k == 3:
            t = _slow_table(c, rng, "code32")
            lanes.append(craft(c, t, [2, 2, 1, 2, 2, 1, 1, 1, 2, 2], "slow: 32-bit code"))
        elif k == 4:
            v, r = ((5, 2), (5, 8), (40, 8), (N[c], 2), (1, 2 * N[c]), (-3, 4), (0, 6), (1023, 2))[i // 8]
            lanes.append(craft(c, [(v, 0)], [v] * r, f"one code, R = {r}"))
        elif k == 6:
            lanes.append(random_stream(c, unary_lengths(CAP[c]), rng, "fast: unary", EDGE_VALUES))
        else:
            lanes.append(random_stream(c, tree_lengths(CAP[c], 6, rng), rng, "fast: tree"))
    return lanes


def _edge_lanes(oracle, c, rng):
    """decode_stream's fill (the unconditional first store, the clamp to the
    row, idx standing still on empty runs) and its got == R test: inverse-RLE
    edges on the fast path, over a short table with values
    0, 1, 2, 3, 5, -1, -4, n, 100 (codes of 2..5 bits)."""
    n = N[c]
    table = list(zip([1, 2, 0, 3, 5, -1, -4, n, 100], [2, 2, 3, 3, 4, 4, 4, 5, 5]))
    left_aligned([L for _, L in table])
    e = [
        ("overshoot at once", [100, 5]),
        ("overshoot after part", [3, 1, 100, 2]),
        ("pairs after a full row", [n, 3, 2, 5, 1, 0, 100, -1]),
        ("exact row then pairs", [5, 1, n, 2, 3, 5]),
        ("zero counts", [0, 5, 2, 1, 0, 3, 0, 0, 1, 2]),
        ("negative counts", [-1, 5, 2, 3, -4, 1, -1, -1, 1, 5]),
        ("only empty runs", [0, 1, -4, 2, -1, 3]),
        ("R = 2", [3, 5]),
        ("R = 2, whole row", [n, -1]),
        ("R = 2, nothing", [0, 5]),
        ("R at the limit, ones", [x for i in range(n) for x in (1, (1, 2, 3, 5, -1, 0)[i % 6])]),
        ("R at the limit, mixed",
         [x for i in range(n) for x in ((1, 0, 2, -1)[i % 4], (2, 5, -4, 3, 1)[i % 5])]),
    ]
    lanes = [craft(c, table, syms, "edge: " + tag, tail=bool(i & 1)) for i, (tag, syms) in enumerate(e)]
    for v, r in ((5, 2), (5, 8), (n, 2), (2, 2 * n)):
        lanes.append(craft(c, [(v, 0)], [v] * r, f"edge: one code {v}, R = {r}"))
    while len(lanes) < LANES:
        lanes.append(_noise(oracle, c, rng))
    return [lanes[i] for i in rng.permutation(LANES)]


# A crafted wave claim: over8 / over16 = the fast lanes whose longest code
# exceeds 8 / 16 bits ("all": every fast lane), within = (lo, hi) bounds on
# every fast lane's longest code.
Crafted = namedtuple("Crafted", "streams claims names")


@functools.lru_cache(maxsize=None)
def crafted_batch(oracle):
    """Every crafted decoder wave: streams[tile][channel], claims[(group,
    channel)] and the group names.  Targets: the luma start-map lookup against
    count_above<24> (narrow against every other class), count_above<12>, the
    refill cadences of four, two and one symbol(s) and the ballots that choose
    them when a single lane (0, 31 or 63) holds the wave's only long code."""
    rng = np.random.default_rng(105)
    groups, claims, names = [], {}, []

    def add(name, per_channel, claim):
        g = len(groups)
        groups.append(per_channel)
        names.append(name)
        for c in range(3):
            claims[(g, c)] = claim[c] if isinstance(claim, (list, tuple)) else claim

    for cls, claim in (("narrow", {"over8": [], "over16": [], "within": (1, 8)}),
                       ("mid", {"over8": "all", "over16": [], "within": (9, 16)}),
                       ("long", {"over8": "all", "over16": "all", "within": (17, 31)})):
        add(cls, [_class_lanes(c, cls, rng) for c in range(3)], claim)
    # one lane over 8 bits (two symbols per refill for the whole wave) and one
    # lane over 16 (one per refill), the rest encoder-made; Cr and Cb take the
    # other class than luma so both run in each group
    # (the lone code sits on both sides of each threshold: 9, 13, 16 and 17, 23, 31 bits)
    mids = {0: (tree_lengths(24, 9, rng), [1, 9]), 31: (tree_lengths(24, 13, rng), unary_lengths(12)),
            63: (tree_lengths(24, 16, rng), chain_lengths(8, 16, 4))}
    longs = {0: (tree_lengths(24, 17, rng), chain_lengths(8, 17, 4)),
             31: (unary_lengths(24), chain_lengths(8, 19, 4)),
             63: (chain_lengths(20, 31, 4), chain_lengths(8, 31, 4))}
    for lane in (0, 31, 63):
        (mid_l, mid_c), (long_l, long_c) = mids[lane], longs[lane]
        add(f"one lane over 8 bits in lane {lane} (chroma: over 16)",
            [_single_lanes(oracle, 0, lane, mid_l, rng, "the only code over 8 bits"),
             _single_lanes(oracle, 1, lane, long_c, rng, "the only code over 16 bits"),
             _single_lanes(oracle, 2, lane, [2, 31, 31], rng, "the only code over 16 bits")],
            [{"over8": [lane], "over16": []}, {"over8": [lane], "over16": [lane]},
             {"over8": [lane], "over16": [lane]}])
        add(f"one lane over 16 bits in lane {lane} (chroma: over 8)",
            [_single_lanes(oracle, 0, lane, long_l, rng, "the only code over 16 bits"),
             _single_lanes(oracle, 1, lane, mid_c, rng, "the only code over 8 bits"),
             _single_lanes(oracle, 2, lane, [1, 9], rng, "the only code over 8 bits")],
            [{"over8": [lane], "over16": [lane]}, {"over8": [lane], "over16": []},
             {"over8": [lane], "over16": []}])
    add("fast lanes beside slow ones", [_mix_lanes(oracle, c, rng) for c in range(3)],
        {"mix": True})
    add("inverse RLE edges", [_edge_lanes(oracle, c, rng) for c in range(3)],
        {"over8": [], "over16": []})
    streams = [[groups[g][c][lane] for c in range(3)]
               for g in range(len(groups)) for lane in range(LANES)]
    return Crafted(streams, claims, names)


def pack(streams):
    """bits [nt, 256] u8, meta [nt, 3] u32, table [nt, 256] u32 and expected
    [nt, 128] int16 of streams[tile][channel] (meta = nbits | R << 16 | U << 24)."""
    nt = len(streams)
    bits = np.zeros((nt, 256), np.uint8)
    meta = np.zeros((nt, 3), np.uint32)
    table = np.zeros((nt, 256), np.uint32)
    want = np.zeros((nt, 128), np.int16)
    for t, row in enumerate(streams):
        for c, s in enumerate(row):
            assert s.c == c
            o = SLOT_OFF[c]
            bits[t, o:o + len(s.bits)] = np.frombuffer(s.bits, np.uint8)
            meta[t, c] = s.nbits | len(s.syms) << 16 | len(s.table) << 24
            table[t, o:o + len(s.table)] = [(v & 0xFFFF) | L << 16 for v, L in s.table]
            want[t, COEF_OFF[c]:COEF_OFF[c] + N[c]] = s.expected
    return bits, meta, table, want
