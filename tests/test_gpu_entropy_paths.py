"""The entropy stage's wave-level paths against the oracle, through the C ABI
(jpeg.Entropy): batches that put chosen streams in chosen lanes (builders and
the kernel decision each one targets: tests/entropy_inputs.py; what they reach
is checked on the CPU by tests/test_entropy_inputs.py).

  encoder   every stream of every batch against oracle_api.entropy: rle_len,
            the table, nbits and the bit bytes
  round     the decoder on the encoder's output gives back the input
  crafted   the decoder on bits / meta / table written by the builders --
            code lengths, refill cadences and lookup methods that no
            encoder-made stream has -- against ints derived in numpy from the
            RLE list
"""
import functools

import numpy as np
import pytest

import entropy_inputs as E

pytestmark = pytest.mark.gpu

SENTINEL = 12345


@functools.lru_cache(maxsize=None)
def _encoded(name):
    """Encode a batch once; the outputs read back in one copy each."""
    import torch
    from lz4jpeg import jpeg
    coef = E.encoder_batch(name).coef
    d_coef = torch.from_numpy(coef.reshape(-1).copy()).cuda()
    ent = jpeg.Entropy(coef.shape[0])
    ent.encode(d_coef)
    torch.cuda.synchronize()
    nt = coef.shape[0]
    bits = ent.bits.cpu().numpy().reshape(nt, 256)
    meta = ent.meta.cpu().numpy().view(np.uint32).reshape(nt, 3)
    table = ent.table.cpu().numpy().view(np.uint32).reshape(nt, 256)
    return d_coef, ent, bits, meta, table, ent.status.cpu().numpy().copy()


def _where(name, t, c):
    return (f"{name}: tile {t}, channel {E.CHANNELS[c]}, "
            f"{'luma' if c == 0 else 'chroma'} wave {E._wave(t // E.LANES, c)[1]}, lane {t % E.LANES}")


@pytest.mark.parametrize("name", E.encoder_batch_names())
def test_encoder_matches_oracle(gpu, oracle, name):
    _, _, bits, meta, table, status = _encoded(name)
    recs = E.oracle_streams(oracle, name)
    assert int(status[0]) == 0, name
    for t, row in enumerate(recs):
        for c, a in enumerate(row):
            m, o = int(meta[t, c]), E.SLOT_OFF[c]
            nbits, rle_len, ncodes = m & 0xFFFF, (m >> 16) & 255, m >> 24
            w = _where(name, t, c)
            assert rle_len == len(a["rle"]), w
            got = [(int((e & 0xFFFF) ^ 0x8000) - 0x8000, int(e >> 16 & 255))
                   for e in table[t, o:o + ncodes].tolist()]
            assert got == [(v, L) for v, L, _ in a["table"]], w
            assert nbits == a["nbits"], w
            # (the oracle's last byte has zero low bits: equality covers them)
            assert bits[t, o:o + (nbits + 7) // 8].tobytes() == a["bits"], w


@pytest.mark.parametrize("name", E.encoder_batch_names())
def test_round_trip(gpu, name):
    import torch
    d_coef, ent, *_ = _encoded(name)
    out = torch.full_like(d_coef, SENTINEL)
    ent.decode(out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(-1, 128)
    want = E.encoder_batch(name).coef
    bad = np.argwhere(got != want)
    if bad.size:
        t, i = (int(x) for x in bad[0])
        c = 0 if i < 64 else 1 if i < 96 else 2
        pytest.fail(f"{len(bad)} ints differ; first: {_where(name, t, c)}, int {i - E.COEF_OFF[c]}: "
                    f"got {got[t, i]}, want {want[t, i]}")
    assert int(ent.status[1].item()) == 0, name


def test_crafted_decode(gpu, oracle):
    import torch
    from lz4jpeg import jpeg
    cb = E.crafted_batch(oracle)
    bits, meta, table, want = E.pack(cb.streams)
    nt = len(cb.streams)
    ent = jpeg.Entropy(nt)
    ent.bits.copy_(torch.from_numpy(bits.reshape(-1)))
    ent.meta.copy_(torch.from_numpy(meta.reshape(-1).view(np.int32)))
    ent.table.copy_(torch.from_numpy(table.reshape(-1).view(np.int32)))
    out = torch.full((nt * 128,), SENTINEL, dtype=torch.int16, device=gpu)
    ent.decode(out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(nt, 128)
    failed = int(ent.status[1].item())
    lines = []
    for t in np.unique(np.argwhere(got != want)[:, 0]):
        for c in range(3):
            sl = slice(E.COEF_OFF[c], E.COEF_OFF[c] + E.N[c])
            if not np.array_equal(got[t, sl], want[t, sl]):
                s = cb.streams[t][c]
                i = int(np.flatnonzero(got[t, sl] != want[t, sl])[0])
                lines.append(f"wave '{cb.names[t // E.LANES]}', lane {t % E.LANES}, channel "
                             f"{E.CHANNELS[c]} ({s.tag}; {len(s.table)} codes, longest "
                             f"{E.lmax(s)} bits, {s.nbits} bits): int {i} got {got[t, sl][i]}, "
                             f"want {want[t, sl][i]}")
    if lines:
        pytest.fail(f"{len(lines)} streams differ (status[1] = {failed}):\n" + "\n".join(lines[:20]))
    assert failed == 0
