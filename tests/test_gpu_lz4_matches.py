"""Both batch match finders at every position, against a plain restatement of
find_longest_match (LZ4.c:290-323; oracle/lz4_oracle.c: lz4o_matches).

The compressor's output shows the match finder only where the greedy parse
lands.  lz4_matches (lz4r_block_matches_device) is the same finder -- the
index, the chain walk, the candidate pass and the best-match scan of lz4_tiles
-- reporting every position of every 300-byte block, and lz4_window_matches
(lz4r_window_matches_device) is the whole-window form for one block of any
length.  Here both are compared entry for entry with the reference on inputs
built to contest what the kernels decide: ties between sources (the smallest
source wins, LZ4.c:307), lengths above 255 (reported whole), matches that end
on or one byte before the block end, chains of many candidates, candidates
that pass the cheap tests and fail the compare, the 1024-byte cap and the
65535-byte window edge.

Every constructed input asserts the property it was built for from the
REFERENCE's result (never from a kernel's), when the fixture is set up:
test_constructed_inputs_have_their_properties runs those set-ups without a
GPU, so a wrong input fails there instead of passing vacuously.
"""
import concurrent.futures
import ctypes

import numpy as np
import pytest

import golden_inputs
import lz4_chunk_lib

BLK = 300
SENTINEL = 0xFFFFFFFF
PERIODS = (2, 3, 4, 5, 6, 7, 63, 64, 65, 150)
LAID_PERIODS = (7, 11, 13, 77)           # none divides 300
LAST_LENGTHS = (1, 2, 3, 4, 5, 8, 23, 24, 299, 300)
PLANT_AT = (1, 4, 292, 293, 294, 295, 296)


def _m(length, dist):
    return length | dist << 16


def _noise(rng, n, alphabet=256):
    return rng.integers(0, alphabet, n, dtype=np.uint8).tobytes()


def _distinct(rng, k):
    return bytes(rng.permutation(256)[:k].astype(np.uint8))


def _fibonacci_word(n, a=b"a", b=b"b"):
    x, y = a, a + b
    while len(y) < n:
        x, y = y, y + x
    return y[:n]


def _thue_morse(n, a=ord("a"), b=ord("b")):
    return bytes(b if bin(i).count("1") & 1 else a for i in range(n))


def _periodic_expect(P, n=BLK):
    """A block of period P over P distinct bytes: every source p - kP ties at
    length n - p, and the smallest one (p mod P) wins."""
    want = np.zeros(n, np.uint32)
    for p in range(P, n - 3):
        want[p] = _m(n - p, p - p % P)
    return want


class Families:
    """Whole 300-byte blocks, family after family, and the reference's
    per-position matches of all of them (computed once, never changed)."""

    def __init__(self, oracle):
        self.parts = []              # (name, first block, blocks)
        self.data = bytearray()
        rng = np.random.default_rng(2024)
        text = golden_inputs.lz4_input("metamorphosis_spaces")

        self.add("one_value", b"\x5a" * BLK + b"\x00" * BLK + b"\xff" * BLK)
        for P in PERIODS:
            self.add(f"period_{P}", (_distinct(rng, P) * (BLK // P + 1))[:BLK])
        for P in LAID_PERIODS:
            self.add(f"laid_{P}", (_distinct(rng, P) * (20 * BLK // P + 1))[:20 * BLK])
        for k in (2, 3, 4):
            self.add(f"alphabet_{k}", bytes(97 + x for x in _noise(rng, 8 * BLK, k)))
        self.add("fibonacci", _fibonacci_word(4 * BLK))
        self.add("thue_morse", _thue_morse(4 * BLK))
        x = _distinct(rng, 150)
        self.add("x_x", x + x)
        # the copy ends one byte before the block end / exactly on it, and its
        # source is not position 0
        x = _distinct(rng, 152)
        self.add("x_x_one_short", x[:3] + x[3:151] + x[3:151] + x[151:152])
        self.add("x_x_exact_end", x[:4] + x[4:152] + x[4:152])
        x = _distinct(rng, 150)
        pieces = [x[8 * i:8 * i + 8] for i in range(18)]
        order = rng.permutation(18)
        self.add("shuffled_pieces", x + b"".join(pieces[i] for i in order) + x[144:150])
        # candidates that pass the cheap tests and fail the compare: equal
        # first bytes after different bytes (1 or 3 bytes agree), and equal
        # first bytes after equal bytes (2 bytes agree)
        v = _distinct(rng, 203)
        b, w, u = v[0:1], v[1:101], v[101:201]
        self.add("near_1", b"".join(w[k:k + 1] + b + u[k:k + 1] for k in range(100)))
        self.add("near_3", b"".join(w[k:k + 1] + v[0:1] + v[201:203] for k in range(75)))
        self.add("near_2", b"".join(v[201:203] + w[k:k + 1] + u[k:k + 1] for k in range(75)))
        self.plants = []             # (block, position, length, source)
        for q in PLANT_AT:
            for ln in (4, 5):
                blk = bytearray(_distinct(rng, 256) + _distinct(rng, 44))
                s = 0 if q < 100 else 100
                for k in range(min(ln, BLK - q)):
                    blk[q + k] = blk[s + k]          # ascending: an overlapping copy repeats
                if q + ln < BLK and blk[q + ln] == blk[s + ln]:
                    blk[q + ln] ^= 0x80
                self.plants.append((len(self.data) // BLK, q, ln, s))
                self.add(f"plant_{ln}_at_{q}", bytes(blk))
        self.add("text", bytes(text[30000:30000 + 30 * BLK]))
        self.add("noise", _noise(rng, 8 * BLK))

        self.data = bytes(self.data)
        self.nb = len(self.data) // BLK
        self.ref = oracle.lz4_block_matches(self.data)
        self.ref.setflags(write=False)
        self.check_properties()

    def add(self, name, blocks):
        assert len(blocks) % BLK == 0, (name, len(blocks))
        self.parts.append((name, len(self.data) // BLK, len(blocks) // BLK))
        self.data += blocks

    def of(self, name):
        """(bytes, reference) of one family's blocks"""
        b0, nb = next((b0, nb) for n, b0, nb in self.parts if n == name)
        return (self.data[BLK * b0:BLK * (b0 + nb)],
                self.ref[BLK * b0:BLK * (b0 + nb)].reshape(nb, BLK))

    def check_properties(self):
        """What each family was built for, read from the reference's result."""
        ref = self.ref.reshape(self.nb, BLK)
        ln, dist = ref & 0xFFFF, ref >> 16
        # the last three positions of a block cannot hold a 4-byte match
        assert not ref[:, BLK - 3:].any()
        assert not ref[:, 0].any()
        _, r = self.of("one_value")
        want = np.array([0] + [_m(BLK - p, p) for p in range(1, BLK - 3)] + [0, 0, 0], np.uint32)
        assert (r == want).all(), "one value: len 300 - p at dist p (the smallest source)"
        assert (r & 0xFFFF).max() == 299, "len > 255 is reported whole"
        for P in PERIODS:
            _, r = self.of(f"period_{P}")
            assert (r[0] == _periodic_expect(P)).all(), P
            # a tie between sources a period apart was decided (for the smallest)
            assert ((r[0] >> 16) >= 2 * P).any() or P == 150, P
        for P in LAID_PERIODS:
            d, r = self.of(f"laid_{P}")
            assert len({d[BLK * b] for b in range(20)}) > 1, "the phase differs per block"
            for b in range(20):
                assert (r[b] == _periodic_expect(P)).all(), (P, b)
        # P(a 4-gram over k symbols occurred among p earlier ones) = 1 - (1 - k^-4)^p,
        # averaged over p = 16 .. 296: 0.98, 0.77, 0.43 for k = 2, 3, 4
        for k, deep in ((2, 0.9), (3, 0.6), (4, 0.3)):
            _, r = self.of(f"alphabet_{k}")
            assert (r[:, 16:BLK - 3] != 0).mean() > deep, k
        for name in ("fibonacci", "thue_morse"):
            _, r = self.of(name)
            assert (r[:, 16:BLK - 3] != 0).mean() > 0.9, name
            assert len({bytes(x) for x in r}) == 4, "the blocks differ"
        _, r = self.of("x_x")
        assert not r[0, :150].any()
        assert all(r[0, p] == _m(BLK - p, 150) for p in range(150, BLK - 3))
        _, r = self.of("x_x_one_short")
        assert not r[0, :151].any()
        assert all(r[0, p] == _m(299 - p, 148) for p in range(151, 296)) and r[0, 296] == 0
        _, r = self.of("x_x_exact_end")
        assert not r[0, :152].any()
        assert all(r[0, p] == _m(BLK - p, 148) for p in range(152, BLK - 3))
        _, r = self.of("shuffled_pieces")
        assert all((r[0, 150 + 8 * j] & 0xFFFF) >= 8 for j in range(18))
        src = np.arange(150, 294, 8) - (r[0, 150:294:8] >> 16)
        assert sorted(src.tolist()) == list(range(0, 144, 8)), "every piece has its own source"
        for name, agree in (("near_1", 1), ("near_3", 3), ("near_2", 2)):
            d, r = self.of(name)
            assert not r.any(), name
            a = np.frombuffer(d, np.uint8)
            # many positions share a first byte; the longest agreement is `agree` < 4
            first = np.bincount(a, minlength=256).max()
            assert first >= 75, (name, first)
            grams = {d[p:p + agree + 1] for p in range(BLK - agree)}
            assert len(grams) == BLK - agree, name         # no (agree + 1)-gram repeats
            assert len({d[p:p + agree] for p in range(BLK - agree + 1)}) <= BLK - agree + 1 - 74
        for blk, q, n, s in self.plants:
            assert ref[blk, q] == _m(min(n, BLK - q), q - s), (q, n, hex(ref[blk, q]))
        _, r = self.of("text")
        assert 0.1 < (r != 0).mean() < 0.95
        _, r = self.of("noise")
        assert not r.any()
        assert (ln[ref != 0] >= 4).all() and (dist[ref != 0] >= 1).all()


@pytest.fixture(scope="module")
def families(oracle):
    return Families(oracle)


def _threaded_matches(oracle, data, p0, p1, pieces=16):
    """lz4o_matches over [p0, p1), split over threads (ctypes drops the GIL)."""
    buf = np.frombuffer(bytes(data), np.uint8)
    edges = np.linspace(p0, p1, pieces + 1).astype(int)
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(lambda ab: oracle.lz4_matches(buf, int(ab[0]), int(ab[1])),
                            zip(edges[:-1], edges[1:])))
    return np.concatenate(parts)


class WindowEdge:
    """About 66,300 bytes of 256-symbol noise with planted 64-byte motifs: a
    source at distance exactly 65535 (found, dist fills 16 bits), sources at
    65536 (not found: a nearer, shorter one wins, or nothing), equal-length
    sources of which the older is outside the window (the younger wins) or
    inside it (the older wins).  Checked over [0, 1200) and [65300, n)."""
    N = 66300
    RANGES = ((0, 1200), (65300, N))

    def __init__(self, oracle):
        rng = np.random.default_rng(65535)
        d = bytearray(_noise(rng, self.N))
        mot = [_distinct(rng, 64) for _ in range(5)]

        def put(at, m):
            d[at:at + len(m)] = m
        self.A = 100 + 65535                       # the only source: 100, dist 65535
        put(100, mot[0]), put(self.A, mot[0])
        self.B = 300 + 65536                       # full source at dist 65536; 20 bytes at 40000
        put(300, mot[1]), put(self.B, mot[1]), put(40000, mot[1][:20])
        self.B2 = 500 + 65536                      # full source at dist 65536; nothing else
        put(500, mot[2]), put(self.B2, mot[2])
        self.C = 66180                             # sources 640 (dist 65540: outside) and 30000
        put(640, mot[3]), put(30000, mot[3]), put(self.C, mot[3])
        self.D = 65720                             # sources 1000 (dist 64720: inside) and 35000
        put(1000, mot[4]), put(35000, mot[4]), put(self.D, mot[4])
        self.data = bytes(d)
        self.ref = [_threaded_matches(oracle, self.data, a, b) for a, b in self.RANGES]
        for r in self.ref:
            r.setflags(write=False)
        self.check_properties()

    def at(self, p):
        a, _ = self.RANGES[1]
        return int(self.ref[1][p - a])

    def check_properties(self):
        assert not self.ref[0].any(), "first occurrences match nothing"
        # distance exactly 65535: found whole, and at the shifted positions too
        for k in range(61):
            assert self.at(self.A + k) == _m(64 - k, 65535), k
        assert self.at(self.A) >> 16 == 0xFFFF
        # distance 65536: the nearer 20-byte source wins instead
        for k in range(17):
            assert self.at(self.B + k) == _m(20 - k, self.B - 40000), k
        assert all(self.at(self.B + k) == 0 for k in range(17, 64))
        # distance 65536 and no other source: nothing
        assert all(self.at(self.B2 + k) == 0 for k in range(64))
        # equal lengths: the older source is outside the window / inside it
        assert self.C - 640 > 65535 and self.at(self.C) == _m(64, self.C - 30000)
        assert self.D - 1000 <= 65535 and self.at(self.D) == _m(64, self.D - 1000)
        tail = self.ref[1]
        assert ((tail >> 16) == 65535).sum() == 61 and (tail >> 16).max() == 65535


@pytest.fixture(scope="module")
def window_edge(oracle):
    return WindowEdge(oracle)


@pytest.fixture(scope="module")
def window_runs(oracle):
    """3000 bytes of one value and of period 7: (data, reference) each, with
    the 1024 cap, the end clamp and the tie to the smallest source asserted
    from the reference."""
    one = b"\x33" * 3000
    per = (b"lz4r_7!" * 429)[:3000]
    r1 = _threaded_matches(oracle, one, 0, 3000)
    r7 = _threaded_matches(oracle, per, 0, 3000)
    want1 = [0] + [_m(min(1024, 3000 - p), p) if 3000 - p >= 4 else 0 for p in range(1, 3000)]
    assert r1.tolist() == want1
    want7 = [0] * 7 + [_m(min(1024, 3000 - p), p - p % 7) if 3000 - p >= 4 else 0
                       for p in range(7, 3000)]
    assert r7.tolist() == want7
    for r in (r1, r7):
        assert ((r & 0xFFFF) == 1024).sum() > 1900 and (r & 0xFFFF)[2990] == 10
        r.setflags(write=False)
    return (one, r1), (per, r7)


def test_constructed_inputs_have_their_properties(families, window_edge, window_runs,
                                                  window_text):
    """No GPU: setting the fixtures up asserted every intended property of the
    constructed inputs from the reference's own result."""
    assert families.nb >= 65 + 3
    d, r = families.of("alphabet_3")
    assert window_edge.ref[1].size == WindowEdge.N - 65300
    assert len(window_runs) == 2 and r.shape == (8, BLK) and len(d) == 8 * BLK


# ---- the block finder ------------------------------------------------------

def _block_matches(gpu, data, misalign=0):
    """lz4r_block_matches_device of `data` placed `misalign` bytes into a device
    buffer -> the n entries; the 64 entries behind them must keep the sentinel."""
    import torch
    n = len(data)
    d_buf = torch.zeros(misalign + n + 64, dtype=torch.uint8, device=gpu)
    assert d_buf.data_ptr() % 4 == 0
    d_in = d_buf[misalign:misalign + n]
    d_in.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    d_m = torch.full((n + 64,), -1, dtype=torch.int32, device=gpu)
    rc = lz4_chunk_lib.block_matches_device("product", d_in, n, d_m)
    assert rc == 0
    torch.cuda.synchronize()
    got = d_m.cpu().numpy().view(np.uint32)
    assert (got[n:] == SENTINEL).all(), "entries past n - 1 were written"
    return got[:n]


def _assert_same(got, want, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        p = int(bad[0])
        raise AssertionError(
            f"{what}: {bad.size} entries differ, first at {p} (block {p // BLK}, position "
            f"{p % BLK}): got len {got[p] & 0xFFFF} dist {got[p] >> 16}, want len "
            f"{want[p] & 0xFFFF} dist {want[p] >> 16}")


@pytest.mark.gpu
def test_block_finder_all_families_one_launch(gpu, families):
    got = _block_matches(gpu, families.data)
    for name, b0, nb in families.parts:
        _assert_same(got[BLK * b0:BLK * (b0 + nb)], families.ref[BLK * b0:BLK * (b0 + nb)], name)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 2, 3, 65])
def test_block_finder_block_counts(gpu, families, nb):
    # windows of nb blocks at several places of the family input
    for b0 in (0, 3, 17, families.nb - nb):
        lo, hi = BLK * b0, BLK * (b0 + nb)
        _assert_same(_block_matches(gpu, families.data[lo:hi]), families.ref[lo:hi], (nb, b0))


def _short(families, length):
    if length == 8:
        return b"abcdabcd"
    return families.of("alphabet_3")[0][BLK:BLK + length]


@pytest.mark.gpu
@pytest.mark.parametrize("length", LAST_LENGTHS)
def test_block_finder_last_block_length(gpu, oracle, families, length):
    last = _short(families, length)
    want_last = oracle.lz4_matches(last)
    if length == 8:
        assert want_last.tolist() == [0, 0, 0, 0, _m(4, 4), 0, 0, 0]
    if length < BLK:                                       # n < 300 alone
        _assert_same(_block_matches(gpu, last), want_last, ("alone", length))
    head, href = families.of("text")
    for nfull in (1, 2):
        data = head[:BLK * nfull] + last
        want = np.concatenate((href[:nfull].ravel(), want_last))
        _assert_same(_block_matches(gpu, data), want, (nfull, length))


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_block_finder_unaligned_input(gpu, oracle, families, misalign):
    b0 = 7 * misalign
    last = _short(families, (23, 5, 299)[misalign - 1])
    data = families.data[BLK * b0:BLK * (b0 + 40)] + last
    want = np.concatenate((families.ref[BLK * b0:BLK * (b0 + 40)], oracle.lz4_matches(last)))
    _assert_same(_block_matches(gpu, data, misalign), want, misalign)


# ---- the window finder -----------------------------------------------------

def _window_matches(gpu, data):
    import torch
    from lz4jpeg import _lib
    n = len(data)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(gpu)
    d_m = torch.full((n + 64,), -1, dtype=torch.int32, device=gpu)
    rc = _lib.lib().lz4r_window_matches_device(
        ctypes.c_void_p(d_in.data_ptr()), n, ctypes.c_void_p(d_m.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    got = d_m.cpu().numpy().view(np.uint32)
    assert (got[n:] == SENTINEL).all(), "entries past n - 1 were written"
    return got[:n]


def _assert_window(got, want, p0, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        p = int(bad[0])
        raise AssertionError(
            f"{what}: {bad.size} entries differ, first at {p0 + p}: got len {got[p] & 0xFFFF} "
            f"dist {got[p] >> 16}, want len {want[p] & 0xFFFF} dist {want[p] >> 16}")


@pytest.fixture(scope="module")
def window_text(oracle):
    """n -> (n bytes of text, the reference over all of them)"""
    out = {}
    for n in (301, 1000):
        data = bytes(golden_inputs.lz4_input("metamorphosis_spaces")[12000:12000 + n])
        want = oracle.lz4_matches(data)
        assert (want != 0).sum() >= 20 and not want.all(), "text: some positions match"
        out[n] = data, want
    assert (out[1000][1][300:] >> 16).max() > 300, "a source further back than a block"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [301, 1000])
def test_window_finder_text(gpu, window_text, n):
    data, want = window_text[n]
    _assert_window(_window_matches(gpu, data), want, 0, n)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1], ids=["one_value", "period_7"])
def test_window_finder_cap_clamp_and_ties(gpu, window_runs, which):
    data, want = window_runs[which]
    _assert_window(_window_matches(gpu, data), want, 0, which)


@pytest.mark.gpu
def test_window_finder_window_edge(gpu, window_edge):
    got = _window_matches(gpu, window_edge.data)
    for (a, b), want in zip(WindowEdge.RANGES, window_edge.ref):
        _assert_window(got[a:b], want, a, "window edge")
