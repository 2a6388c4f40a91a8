"""The block kernels (csrc/jpegr_blocks.hip) through their device API, not one
block a call through the compat functions: jpegr_dct_blocks_device,
jpegr_quantize_device, jpegr_permute_device and jpegr_planes_device on batches,
against the oracle alone, every output in a guard arena (jpeg_pixel_lib).

One 264 x 24 random image (99 tiles): its jo_planes planes cut into 99 Y blocks
(8 x 8) and 99 Cr and 99 Cb blocks (8 x 4, the odd columns), as
test_gpu_compat.py cuts two tiles.  99 blocks of 64 or 32 doubles are 25 or 13
workgroups of quantize / permute.
"""
import numpy as np
import pytest

import jpeg_exact_inputs as X
import jpeg_pixel_lib as P

pytestmark = pytest.mark.gpu

W, H, NT = 264, 24, 99
# plane -> (block width, elements, slice of a tile's 128, quantiser table, zigzag order)
PLANES = {"Y": (8, 64, slice(0, 64), X.LUMA_Q, X.ZZ8),
          "Cr": (4, 32, slice(64, 96), X.CHROMA_Q, X.ZZ4),
          "Cb": (4, 32, slice(96, 128), X.CHROMA_Q, X.ZZ4)}


@pytest.fixture(scope="module")
def case(oracle):
    """The image's blocks and the oracle's answers; shared, not to be changed."""
    img = oracle.rand_image(W, H, seed=77)
    y, cr, cb = X.planes(oracle, img)
    raw = oracle.jpeg_dct_raw(img).reshape(NT, 128)
    coef = oracle.jpeg_encode(img).reshape(NT, 128)

    def cut(p, bw):                                          # [H, 33 bw] -> [99, 8 bw]
        return np.ascontiguousarray(p.reshape(H // 8, 8, W // 8, bw).transpose(0, 2, 1, 3)).reshape(NT, 8 * bw)

    blocks = {"Y": cut(y, 8), "Cr": cut(cr[:, 1::2], 4), "Cb": cut(cb[:, 1::2], 4)}
    assert np.array_equal(blocks["Y"][34].reshape(8, 8), y[8:16, 8:16])        # tile (1, 1)
    assert np.array_equal(blocks["Cb"][34].reshape(8, 4), cb[8:16, 9:16:2])
    out = {}
    for name, (bw, n, sl, table, zz) in PLANES.items():
        zigzag = np.ascontiguousarray(coef[:, sl]).astype(np.float64)           # [99, n], zigzag order
        natural = np.empty_like(zigzag)
        natural[:, zz] = zigzag                                                 # zigzag[k] = natural[zz[k]]
        out[name] = dict(blocks=blocks[name], raw=np.ascontiguousarray(raw[:, sl]),
                         natural=natural, zigzag=zigzag)
    for d in out.values():
        for a in d.values():
            a.setflags(write=False)
    return out


def _ok(arena, want, what):
    bad = arena.problem(want)
    assert bad is None, f"{what}: {bad}"


@pytest.mark.parametrize("name", list(PLANES))
def test_dct_blocks_batches(gpu, case, name):
    """All 99 blocks of a plane, and sub-batches of 1, 2, 63, 64 and 65 blocks
    from block 7 on, bit for bit; the blocks sit at an odd address."""
    import torch
    bw, n = PLANES[name][:2]
    c = case[name]
    for fill in P.INPUT_FILLS:
        src = P.Arena(NT * n, 1, fill).load(c["blocks"])
        runs = []
        for first, count in ((0, NT), (7, 1), (7, 2), (7, 63), (7, 64), (7, 65)):
            out = P.Arena(count * n * 8, 8)                  # 8-B, not 16-B aligned
            assert P.dct_blocks(src.vp(first * n), bw, count, out.vp()) == 0
            runs.append((first, count, out))
        torch.cuda.synchronize()
        for first, count, out in runs:
            _ok(out, c["raw"][first:first + count], f"{name} blocks {first}..{first + count - 1}, "
                                                    f"input fill 0x{fill:02x}")


@pytest.mark.parametrize("name", list(PLANES))
def test_quantize_then_permute(gpu, case, name):
    """Quantize in place over the whole batch with the plane's table, then the
    zigzag permutation: the oracle's encoded tiles.  Once more with n cut to 50
    blocks and 5 elements: what lies past n keeps the arena's fill."""
    import torch
    _, n, _, table, zz = PLANES[name]
    c = case[name]
    tab = P.Arena(n * 8, 8, 0xFF).load(np.array(table, np.float64))
    perm = P.Arena(n * 4, 4, 0xFF).load(np.array(zz, np.int32))
    total = NT * n
    cutn = 50 * n + 5

    # the whole batch, the second kernel fed by the first
    q = P.Arena(total * 8, 8).load(c["raw"])
    assert P.quantize(q.vp(), tab.vp(), n, total) == 0
    z = P.Arena(total * 8, 8)
    assert P.permute(q.vp(), z.vp(), perm.vp(), n, total) == 0

    # n cut: quantize on an arena that holds only the first n doubles, permute
    # from whole quantised blocks (it reads inside the last block it starts)
    qc = P.Arena(total * 8, 8).load(c["raw"].reshape(-1)[:cutn])
    assert P.quantize(qc.vp(), tab.vp(), n, cutn) == 0
    full = P.Arena(total * 8, 8, 0x00).load(c["natural"])
    zc = P.Arena(total * 8, 8)
    assert P.permute(full.vp(), zc.vp(), perm.vp(), n, cutn) == 0
    torch.cuda.synchronize()

    _ok(q, c["natural"], f"{name} quantize")
    _ok(z, c["zigzag"], f"{name} quantize + permute")
    assert np.array_equal(c["zigzag"].astype(np.int16), c["zigzag"])           # the int16 tiles themselves
    rest = P.filled(total - cutn, np.float64)
    _ok(qc, np.concatenate([c["natural"].reshape(-1)[:cutn], rest]), f"{name} quantize, n = {cutn}")
    _ok(zc, np.concatenate([c["zigzag"].reshape(-1)[:cutn], rest]), f"{name} permute, n = {cutn}")
    _ok(tab, np.array(table, np.float64), "the table is read only")
    _ok(full, c["natural"], "permute's input is read only")


def test_planes_at_odd_addresses(gpu, oracle):
    """37 x 21 (777 pixels: four workgroups, the last ragged), d_rgba 4-B but not
    16-B aligned, the three planes at odd addresses."""
    import torch
    w, h = 37, 21
    img = oracle.rand_image(w, h, seed=78)
    want = X.planes(oracle, img)
    for fill in P.INPUT_FILLS:
        src = P.Arena(w * h * 4, 4, fill).load(img)
        outs = [P.Arena(w * h, off) for off in (1, 3, 5)]
        assert all(o.ptr % 2 == 1 for o in outs)
        assert P.planes(src.vp(), w, h, *(o.vp() for o in outs)) == 0
        torch.cuda.synchronize()
        for o, plane, nm in zip(outs, want, ("Y", "Cr", "Cb")):
            _ok(o, plane, f"{nm} plane, input fill 0x{fill:02x}")
