"""Slot arrays for the JPT1 tests (tests/jpt_format.py): tables built to sit on
every edge of the mode rule, random slots of every mode, and the oracle's
entropy records of an image.  Plain numpy; shared by the CPU and GPU tests."""
import functools

import numpy as np

import jpr_format as J
import oracle_api

COEF_OFF = (0, 64, 96)
N = (64, 32, 32)


def _slots(nt):
    return (np.zeros((nt, 256), np.uint8), np.zeros((nt, 3), np.uint32), np.zeros((nt, 256), np.uint32))


def _put(arrays, t, c, ents, nbits, rle_len, rng, high=0):
    """Stream (t, c): table entries [(value, length)], nbits random bits."""
    bits, meta, table = arrays
    o = J.SLOT_OFF[c]
    meta[t, c] = nbits | rle_len << 16 | len(ents) << 24
    table[t, o:o + len(ents)] = [(v & 0xFFFF) | L << 16 | high << 24 for v, L in ents]
    nby = (nbits + 7) // 8
    bits[t, o:o + nby] = rng.integers(0, 256, nby)


def _table(n, rng, lens=(1, 15), vals=(-128, 127), pin=()):
    """n entries of lengths and values in the closed ranges, `pin` = entries
    placed at spread positions."""
    ents = [(int(rng.integers(vals[0], vals[1] + 1)), int(rng.integers(lens[0], lens[1] + 1)))
            for _ in range(n)]
    for i, e in enumerate(pin):
        ents[(i * 7 + n // 2) % n] = e
    return ents


@functools.lru_cache(maxsize=None)
def edge_slots():
    """(bits, meta, table) of 16 tiles -- one workgroup of the pack kernels --
    on the mode rule's edges: no codes; odd and even counts; a length of
    exactly 15 (mode 1) and of 16 (mode 0); values -128 and 127 (mode 1), -129
    and 128 (mode 2), the int16 extremes; 128-code tables in every mode, the
    last of them a record of 1,036 B; 65 and 127 codes (the second table
    register, an odd count there); table words with bits 24..31 set."""
    rng = np.random.default_rng(2024)
    a = _slots(16)
    put = functools.partial(_put, a, rng=rng)
    for c in range(3):
        put(0, c, [], 0, 0)
    put(1, 0, [(0, 1)], 0, 1)
    put(1, 1, [(5, 1), (-5, 1)], 9, 9)
    put(1, 2, [(1, 1), (2, 2), (3, 2)], 17, 10)
    put(2, 0, _table(9, rng, pin=[(3, 15)]), 100, 20)
    put(2, 1, _table(8, rng, pin=[(3, 16)]), 64, 20)
    put(2, 2, _table(6, rng, pin=[(-128, 4), (127, 5)]), 63, 20)
    put(3, 0, _table(7, rng, pin=[(-129, 4)]), 65, 20)
    put(3, 1, _table(4, rng, pin=[(128, 3)]), 1, 1)
    put(3, 2, _table(5, rng, pin=[(-32768, 15), (32767, 1)]), 512, 64)
    put(4, 0, _table(128, rng, pin=[(-128, 15), (127, 15)]), 1024, 128)
    put(4, 1, _table(64, rng, vals=(-300, 300), pin=[(128, 15)]), 512, 64)
    put(4, 2, _table(64, rng), 505, 64)
    put(5, 0, _table(128, rng, lens=(1, 32), vals=(-32768, 32767), pin=[(0, 16)]), 1024, 128)
    put(5, 1, _table(64, rng, lens=(1, 255), pin=[(1, 255)]), 512, 64)
    put(5, 2, _table(64, rng, lens=(16, 16)), 512, 64)
    put(6, 0, _table(65, rng), 300, 70)
    put(6, 1, _table(63, rng), 200, 63)
    put(6, 2, [(9, 15)], 0, 3)
    put(7, 0, _table(127, rng, vals=(-129, 128), pin=[(-129, 1), (128, 2)]), 1017, 127)
    put(7, 1, _table(1, rng, vals=(128, 128)), 0, 2)
    put(7, 2, _table(2, rng, lens=(0, 0)), 8, 2)
    for t in range(8, 16):                                  # the same shapes, dirty high bytes
        for c in range(3):
            n = int(rng.integers(0, J.SLOT_CODES[c] + 1))
            kind = (t + c) % 3
            ents = _table(n, rng, lens=(1, 15 if kind else 17),
                          vals=(-128, 127) if kind == 1 else (-2000, 2000)) if n else []
            _put(a, t, c, ents, int(rng.integers(0, J.SLOT_BITS[c] + 1)),
                 int(rng.integers(0, J.SLOT_CODES[c] + 1)), rng, high=int(rng.integers(1, 256)))
    for x in a:
        x.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_slots(nt, seed=11):
    """nt tiles of random streams, a third each aimed at modes 0, 1 and 2."""
    rng = np.random.default_rng(seed)
    a = _slots(nt)
    for t in range(nt):
        for c in range(3):
            n = int(rng.integers(0, J.SLOT_CODES[c] + 1)) if rng.integers(0, 4) else int(rng.integers(0, 4))
            kind = int(rng.integers(0, 3))
            ents = _table(n, rng, lens=(0, 15 if kind else 40),
                          vals=(-128, 127) if kind == 1 else (-32768, 32767)) if n else []
            _put(a, t, c, ents, int(rng.integers(0, J.SLOT_BITS[c] + 1)),
                 int(rng.integers(0, J.SLOT_CODES[c] + 1)), rng)
    for x in a:
        x.setflags(write=False)
    return a


def overflow_slots():
    """Four tiles whose meta fields pass their slots (ncodes 255, nbits
    65,535): both writers clamp them first."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 256, (4, 256)).astype(np.uint8)
    table = rng.integers(0, 1 << 20, (4, 256)).astype(np.uint32) & 0x000FFFFF   # lengths 0..15
    meta = np.array([[0xFF05FFFF, 0xFF05FFFF, 0xFF05FFFF], [0x81000401, 0x41000201, 0x40000200],
                     [0x80000400, 0xFF000000, 0x0000FFFF], [0x10100010, 0x10100010, 0x10100010]],
                    np.uint32)
    return bits, meta, table


def clamp(meta):
    """meta with ncodes and nbits clamped to the slots (what the packers do)."""
    meta = np.asarray(meta).astype(np.uint32).reshape(-1, 3).copy()
    for c in range(3):
        nb = np.minimum(meta[:, c] & 0xFFFF, J.SLOT_BITS[c])
        nc = np.minimum(meta[:, c] >> 24, J.SLOT_CODES[c])
        meta[:, c] = nb | (meta[:, c] & 0x00FF0000) | nc << 24
    return meta


def oracle_slots(oracle, coef):
    """The oracle's entropy records (oracle_api.entropy) of coefficients
    [nt, 128] as slot arrays."""
    coef = np.asarray(coef, np.int16).reshape(-1, 128)
    nt = coef.shape[0]
    bits, meta, table = _slots(nt)
    for t in range(nt):
        for c in range(3):
            e = oracle_api.entropy(oracle, coef[t, COEF_OFF[c]:COEF_OFF[c] + N[c]])
            o = J.SLOT_OFF[c]
            assert e["rc"] == 0 and len(e["table"]) <= J.SLOT_CODES[c] and e["nbits"] <= J.SLOT_BITS[c]
            meta[t, c] = e["nbits"] | len(e["rle"]) << 16 | len(e["table"]) << 24
            table[t, o:o + len(e["table"])] = [(v & 0xFFFF) | L << 16 for v, L, _ in e["table"]]
            bits[t, o:o + len(e["bits"])] = np.frombuffer(e["bits"], np.uint8)
    return bits, meta, table


def smooth_image(w, h):
    """tools/jpeg_pack_bench.py's smooth image."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([(xx // 3) % 256, (yy // 2) % 256, ((xx + yy) // 5) % 256,
                                          np.full_like(xx, 255)], -1).astype(np.uint8))
