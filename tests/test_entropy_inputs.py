"""The batches of tests/test_gpu_entropy_paths.py hit the waves they are
built for.  Oracle only (no GPU): per wave, the distinct-symbol counts, the
number of lanes the fast encoder defers and the longest codes are computed
with the pinned oracle and compared with what each builder claims, and every
crafted decoder stream is decoded by the oracle to the ints that numpy derives
from its RLE list -- so a later change to a builder cannot quietly move the
GPU tests off their paths, and the GPU test sees well-formed input only."""
import numpy as np
import pytest

import entropy_inputs as E
import oracle_api


def _wave_streams(name, oracle):
    """{(kind, wave): [(lane, coefficients, oracle record)]} of an encoder batch."""
    coef = E.encoder_batch(name).coef
    recs = E.oracle_streams(oracle, name)
    out = {}
    for t in range(coef.shape[0]):
        for c in range(3):
            zz = coef[t, E.COEF_OFF[c]:E.COEF_OFF[c] + E.N[c]]
            out.setdefault(E._wave(t // E.LANES, c), []).append((t % E.LANES, c, zz, recs[t][c]))
    return out


def _deferred(rec, c):
    """The fast encoder's rule, restated on the oracle's RLE ints: U > 24 / 12
    or a symbol outside -64..111 / -48..71."""
    syms = set(rec["rle"])
    lo, hi = ((-64, 111), (-48, 71), (-48, 71))[c]
    return len(syms) > (24, 12, 12)[c] or min(syms) < lo or max(syms) > hi


def test_batches_stay_small(oracle):
    tiles = sum(E.encoder_batch(n).coef.shape[0] for n in E.encoder_batch_names())
    assert tiles + len(E.crafted_batch(oracle).streams) < 10000


@pytest.mark.parametrize("name", E.encoder_batch_names())
def test_encoder_batch_claims(oracle, name):
    """Per wave: umax, the ladder's set of U and the exact number of deferred
    lanes; every stream fits the reference's buffers (status[0] stays 0)."""
    batch = E.encoder_batch(name)
    waves = _wave_streams(name, oracle)
    assert set(batch.claims) <= set(waves)
    for key, lanes in waves.items():
        for lane, c, zz, rec in lanes:
            assert rec["rc"] == 0 and rec["nbits"] <= (1023, 511, 511)[c], (name, key, lane)
            assert max(L for _, L, _ in rec["table"]) <= 31, (name, key, lane)
            assert len(rec["table"]) == E.distinct(E.rle_of(zz))
            assert _deferred(rec, c) == E.is_deferred(zz, c)
        claim = batch.claims.get(key, {})
        us = [len(rec["table"]) for _, _, _, rec in lanes]
        if "umax" in claim:
            assert max(us) == claim["umax"], (name, key)
        if "u_set" in claim:
            assert sorted(set(us)) == claim["u_set"], (name, key)
        if "deferred" in claim:
            assert sum(_deferred(rec, c) for _, c, _, rec in lanes) == claim["deferred"], (name, key)
        if "live" in claim:
            assert len(lanes) == claim["live"], (name, key)


def test_sweep_reaches_every_umax_and_distribution(oracle):
    """umax 1..26 on luma and 1..14 on Cr and on Cb (never the same in one
    tile group), lane 0 holding it; one-symbol streams in every wave; heaps
    whose counts are all equal, and trees as deep as U - 1."""
    waves = _wave_streams("umax_sweep", oracle)
    claims = E.encoder_batch("umax_sweep").claims
    assert sorted(v["umax"] for k, v in claims.items() if k[0] == "luma") == list(range(1, 27))
    for parity in (0, 1):
        got = sorted(v["umax"] for k, v in claims.items() if k[0] == "chroma" and k[1] % 2 == parity)
        assert set(got) == set(range(1, 15)), parity
    flat = deep = 0
    for key, lanes in waves.items():
        assert len(lanes[0][3]["table"]) == claims[key]["umax"]
        assert any(len(rec["table"]) == 1 for _, _, _, rec in lanes), key
        for _, _, _, rec in lanes:
            rle, U = rec["rle"], len(rec["table"])
            freq = sorted(rle.count(s) for s in set(rle))
            flat += U >= 4 and freq[-2] == 1              # all counts equal but at most one
            deep += U >= 6 and max(L for _, L, _ in rec["table"]) >= 6
    for g in range(26):
        assert claims[("chroma", 2 * g)]["umax"] != claims[("chroma", 2 * g + 1)]["umax"]
    print("streams with tied counts", flat, "; with a code of 6 bits or more", deep)
    assert flat >= 200 and deep >= 200


def test_deferral_batch_counts_and_causes(oracle):
    """Luma waves with 0, 1, 5, 6, 7, 13 and 64 deferred lanes, each caused
    once by U = 25 alone and once by a value one past the key range alone,
    each beside chroma waves with 0, 1 and 7 deferred lanes on the even wave."""
    waves = _wave_streams("deferral", oracle)
    seen = set()
    for (kind, w), lanes in waves.items():
        if kind != "luma":
            continue
        by_u = sum(len(rec["table"]) > 24 for _, _, _, rec in lanes)
        by_v = sum(len(rec["table"]) <= 24 and _deferred(rec, 0) for _, _, _, rec in lanes)
        assert by_u == 0 or by_v == 0, w
        even = sum(_deferred(rec, 1) for _, _, _, rec in waves[("chroma", 2 * w)])
        seen.add((by_u + by_v, "U" if by_u else "value" if by_v else "none", even))
    for d in (1, 5, 6, 7, 13, 64):
        for cause in ("U", "value"):
            for even in (0, 1, 7):
                assert (d, cause, even) in seen, (d, cause, even)
    assert {(0, "none", e) for e in (0, 1, 7)} <= seen
    coef = E.encoder_batch("deferral").coef
    for c, sl in ((0, slice(0, 64)), (1, slice(64, 96)), (2, slice(96, 128))):
        lo, hi = E.KEY_EDGES[min(c, 1)][:2]
        assert (coef[:, sl] == lo).any() and (coef[:, sl] == hi).any(), c
        assert coef[:, sl].min() == lo and coef[:, sl].max() == hi, c


def test_sized_batches_defer_every_live_lane_of_the_last_wave(oracle):
    for n in E.SIZES:
        waves = _wave_streams(f"size{n}_defer", oracle)
        last = (n - 1) // E.LANES
        live = n - last * E.LANES
        for key in (("luma", last), ("chroma", 2 * last), ("chroma", 2 * last + 1)):
            lanes = waves[key]
            assert len(lanes) == live and all(_deferred(rec, c) for _, c, _, rec in lanes), (n, key)
        plain = _wave_streams(f"size{n}_plain", oracle)
        assert not any(_deferred(rec, c) for lanes in plain.values() for _, c, _, rec in lanes), n
    assert 1 < E.KSLOTS and 3 < E.KSLOTS < 63              # live lanes on both sides of kSlots


def test_values_batch_holds_every_named_value(oracle):
    coef = E.encoder_batch("values").coef
    for sl, edges in ((slice(0, 64), E.KEY_EDGES[0]), (slice(64, 96), E.KEY_EDGES[1]),
                      (slice(96, 128), E.KEY_EDGES[1])):
        for v in E.WIDE_VALUES + edges:
            assert (coef[:, sl] == v).any(), (sl, v)
    recs = E.oracle_streams(oracle, "values")
    for c in range(3):
        pairs = [p for row in recs for p in zip(row[c]["rle"][0::2], row[c]["rle"][1::2])]
        assert sum(a == b for a, b in pairs) >= 6, c       # counts equal to values
        assert any(not -1024 <= v <= 1023 for row in recs for v, _, _ in row[c]["table"])


# ---- crafted decoder streams --------------------------------------------------
def _crafted(oracle):
    cb = E.crafted_batch(oracle)
    groups = len(cb.names)
    lanes = {(g, c): [cb.streams[g * E.LANES + lane][c] for lane in range(E.LANES)]
             for g in range(groups) for c in range(3)}
    return cb, lanes


def test_crafted_streams_are_well_formed_and_decode_to_the_numpy_ints(oracle):
    """No stream exceeds its slot, rle_len is the number of codes, the codes
    follow the header's rule, the last byte's unused bits are zero -- and the
    oracle decodes (table, codes, bits, nbits, rle_len) to the expectation."""
    cb, _ = _crafted(oracle)
    assert len(cb.streams) == len(cb.names) * E.LANES
    for t, row in enumerate(cb.streams):
        for c, s in enumerate(row):
            where = (cb.names[t // E.LANES], t % E.LANES, E.CHANNELS[c], s.tag)
            n = E.N[c]
            assert s.c == c and 0 <= s.nbits <= E.SLOT_BITS[c] == 8 * len(s.bits), where
            assert 1 <= len(s.syms) <= 2 * n and 1 <= len(s.table) <= 2 * n, where
            lens = dict(s.table)
            assert sum(lens[v] for v in s.syms) == s.nbits, where
            assert s.codes == E.codes_from_lengths([L for _, L in s.table]), where
            if s.nbits % 8:
                assert s.bits[s.nbits // 8] & (0xFF >> (s.nbits % 8)) == 0, where
            if not s.tail:
                assert not any(s.bits[(s.nbits + 7) // 8:]), where
            rec = {"table": [(v, L, co) for (v, L), co in zip(s.table, s.codes)],
                   "bits": s.bits[:(s.nbits + 7) // 8], "nbits": s.nbits, "rle": s.syms}
            assert oracle_api.entropy_decode(oracle, rec, n) == s.expected.tolist(), where
    bits, meta, table, want = E.pack(cb.streams)
    assert ((meta & 0xFFFF) <= np.array(E.SLOT_BITS)).all()
    assert ((meta >> 16 & 255) <= 2 * np.array(E.N)).all() and (meta >> 24 <= 2 * np.array(E.N)).all()


def test_crafted_waves_have_the_longest_codes_they_claim(oracle):
    """Per wave and channel, over the lanes that vote (fast-path streams with
    more than one code): which lanes exceed 8 and 16 bits."""
    cb, lanes = _crafted(oracle)
    for key, claim in cb.claims.items():
        fast = [(i, E.lmax(s)) for i, s in enumerate(lanes[key]) if E.stream_class(s) == "fast"]
        assert len(fast) >= 16, key
        for bound, name in ((8, "over8"), (16, "over16")):
            if name in claim:
                got = [i for i, m in fast if m > bound]
                want = [i for i, _ in fast] if claim[name] == "all" else claim[name]
                assert got == want, (cb.names[key[0]], key, name)
        if "within" in claim:
            lo, hi = claim["within"]
            assert all(lo <= m <= hi for _, m in fast), key
            assert {m for _, m in fast} >= {hi}, key
    # the named tables, per channel kind
    for kind, chans in ((0, (0,)), (1, (1, 2))):
        cap = E.CAP[kind]
        tabs = {tuple(L for _, L in s.table) for row in cb.streams for s in row if s.c in chans}
        longest = {max(t) for t in tabs}
        assert {8, 9, 16, 17, 31, 32} <= longest, kind
        for t in (tuple(E.unary_lengths(cap)), (1, 9), (1, 16), (1, 17), (2, 31, 31), (1, 32)):
            assert t in tabs, (kind, t)
        assert any(len(t) > cap for t in tabs) and any(len(t) == 2 * E.N[kind] for t in tabs), kind


def lens_end(s):
    """The length of the stream's last code."""
    return dict(s.table)[s.syms[-1]]


def test_crafted_positions_and_edges(oracle):
    """In each cadence class and channel: long codes starting at bits 0, 1, 31
    and 32 and across every 16-byte boundary of the slot; a stream that fills
    the slot and one a bit short of it; the fast decoder's extreme values; the
    inverse-RLE edges; and the slow-path lanes beside fast ones."""
    cb, lanes = _crafted(oracle)
    for g, cls in enumerate(("narrow", "mid", "long")):
        assert cb.names[g] == cls
        for c in range(3):
            ss = lanes[(g, c)]
            top = E.CLASS_LEN[cls]
            starts, crossed = set(), set()
            for s in ss:
                lens = dict(s.table)
                for sym, at in zip(s.syms, s.starts):
                    if lens[sym] == top:
                        starts.add(at)
                        crossed |= {b for b in range(128, E.SLOT_BITS[c], 128) if at < b < at + top}
            assert {0, 1, 31, 32} <= starts, (cls, c)
            assert crossed == set(range(128, E.SLOT_BITS[c], 128)), (cls, c)
            nb = {s.nbits for s in ss}
            assert {E.SLOT_BITS[c], E.SLOT_BITS[c] - 1} <= nb, (cls, c)
            assert any(lens_end(s) == top for s in ss if s.nbits == E.SLOT_BITS[c]), (cls, c)
            vals = {v for s in ss for v in s.syms}
            assert {-1024, 1023} <= vals, (cls, c)
    mix = cb.names.index("fast lanes beside slow ones")
    edges = cb.names.index("inverse RLE edges")
    for c in range(3):
        n = E.N[c]
        ss = lanes[(mix, c)]
        kinds = [E.stream_class(s) for s in ss]
        assert min(kinds.count(k) for k in ("fast", "slow", "one")) >= 8, c
        wide = {v for s in ss for v in s.syms if not -1024 <= v <= 1023}
        assert wide >= {-1025, 1024, 32767, -32767, -32768}, c
        assert any(s.syms[i] < -1024 for s in ss for i in range(0, len(s.syms), 2)), c
        assert any(max(L for _, L in s.table) == 32 for s in ss), c
        assert any(len(s.table) > E.CAP[c] for s in ss), c
        es = lanes[(edges, c)]
        pairs = [list(zip(s.syms[0::2], s.syms[1::2])) for s in es if s.tag.startswith("edge")]
        assert any(sum(max(a, 0) for a, _ in p) > n for p in pairs)          # overshoot
        assert any(sum(min(max(a, 0), n) for a, _ in p[:k]) >= n             # pairs after a full row
                   for p in pairs for k in range(1, len(p)))
        assert any(a == 0 for p in pairs for a, _ in p) and any(a < 0 for p in pairs for a, _ in p)
        rs = {len(s.syms) for s in es if len(s.table) > 1}
        assert {2, 2 * n} <= rs, c
        ones = {(len(s.syms), s.nbits) for s in es + ss if len(s.table) == 1}
        assert {(2, 0), (8, 0)} <= ones, c
