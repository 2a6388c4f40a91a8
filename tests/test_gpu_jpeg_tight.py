"""The JPT1 stream on the GPU (jpegr_pack_tight_device and the direct decode of
its output, include/jpegr.h) against the plain-Python restatement
(tests/jpt_format.py).  The expected bytes are the restatement's, the expected
coefficients the slot decoder's (Entropy.decode), the builders' `want` or the
encoder's input -- and, for streams the entropy decoder rejects, whose ints
the slot decoder leaves unspecified, the direct decode of the JPR1 stream of
the same slots -- never the JPT1 path's own output.

Tile counts: both pack kernels take a run of 16 tiles per workgroup, the scan
groups 64 tiles and its partials 4,096; 1, 15, 136 and 4,160 tiles sit in a
lone wave, a part-filled workgroup, past a scan group and past a partial."""
import functools
import os
import subprocess

import numpy as np
import pytest

import entropy_inputs as E
import jpr_format as J
import jpt_format as T
import jpt_inputs as I
from jpr_gpu_lib import (SENTINEL, U64, crafted, current_stream, encode_slots, encoded, gpu_decode, image,
                         pack_scratch, slot_arrays, to_dev, vp)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "lz4-jpeg_amd", "bin")


def gpu_pack_tight(arrays, w, h, nimg, cap=None, room=0, sentinel=0xEE):
    """(bytes of the whole output allocation, length word) of the C call on
    the slot arrays."""
    import torch
    from lz4jpeg import _lib
    L = _lib.lib()
    bits, meta, table = (to_dev(a, t) for a, t in zip(arrays, (np.uint8, np.uint32, np.uint32)))
    bound = int(L.jpegr_pack_bound(w, h, nimg))
    out = torch.full((bound + room,), sentinel, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    scr = pack_scratch(J.ntiles_of(w, h, nimg))
    rc = L.jpegr_pack_tight_device(vp(bits), vp(meta), vp(table), w, h, nimg, vp(out),
                                   bound if cap is None else cap, vp(d_len), vp(scr), current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), int(d_len.item())


def slot_decode(arrays):
    """(coefficients [nt, 128], status[1]) of jpegr_entropy_decode_device on the slots."""
    import torch
    from lz4jpeg import jpeg
    nt = arrays[1].shape[0]
    ent = jpeg.Entropy(nt)
    ent.bits.copy_(to_dev(arrays[0], np.uint8))
    ent.meta.copy_(to_dev(arrays[1], np.uint32).view(torch.int32))
    ent.table.copy_(to_dev(arrays[2], np.uint32).view(torch.int32))
    out = torch.full((nt * 128,), SENTINEL, dtype=torch.int16, device="cuda")
    ent.decode(out)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nt, 128), int(ent.status[1].item())


@functools.lru_cache(maxsize=None)
def image_slots(oracle, w, h, kind, nimg=1):
    """(slot arrays, coefficients) of nimg images through encode_device and Entropy.encode."""
    import torch
    from lz4jpeg import jpeg
    img = np.concatenate([image(oracle, w, h, kind, seed=1 + i).reshape(-1) for i in range(nimg)])
    d_coef = jpeg.encode_device(torch.from_numpy(img).cuda(), w, h, nimg)
    coef = d_coef.cpu().numpy().reshape(-1, 128)
    return encode_slots(coef), coef


@functools.lru_cache(maxsize=None)
def encoded65():
    """jpr_gpu_lib.encoded(65): slots, coefficients, the restatement's JPT1
    stream, dims."""
    arrays, coef, dims = encoded(65)
    return arrays, coef, T.pack(*arrays, *dims), dims


def _check_pack(arrays, dims, name=""):
    want = T.pack(*arrays, *dims)
    got, length = gpu_pack_tight(arrays, *dims)
    assert length == len(want), name
    assert got[:length] == want, name
    assert set(got[length:]) <= {0xEE}, name                # nothing past the stream
    return want


# ---- bytes -----------------------------------------------------------------------

@pytest.mark.parametrize("w,h,nimg", [(8, 8, 1), (40, 24, 1), (136, 64, 1), (520, 512, 1), (72, 40, 3)])
@pytest.mark.parametrize("kind", ["rand", "smooth"])
def test_image_bytes(gpu, oracle, w, h, nimg, kind):
    arrays, _ = image_slots(oracle, w, h, kind, nimg)
    want = _check_pack(arrays, (w, h, nimg))
    assert T.header(want) == (w, h, nimg)
    assert len(want) < len(J.pack(*arrays, w, h, nimg))


def test_batch_bytes(gpu, oracle):
    """The crafted decoder batch (long codes: mode 0), the mode rule's edges,
    random slots, and the encoder batches `values` (int16 extremes: mode 2)
    and `deferral`."""
    batches = {"crafted": crafted(oracle)[0], "edges": I.edge_slots(), "random": I.random_slots(96),
               "values": encode_slots(E.encoder_batch("values").coef),
               "deferral": encode_slots(E.encoder_batch("deferral").coef)}
    modes = {}
    for name, arrays in batches.items():
        nt = arrays[1].shape[0]
        _check_pack(arrays, (8 * nt, 8, 1), name)
        modes[name] = set(T.stream_modes(*arrays).reshape(-1).tolist())
    assert 0 in modes["crafted"] and 2 in modes["values"] and 1 in modes["deferral"], modes
    assert modes["edges"] == {0, 1, 2} and modes["random"] == {0, 1, 2}


def test_meta_past_the_slot_is_clamped(gpu):
    bits, meta, table = I.overflow_slots()
    want = T.pack(bits, I.clamp(meta), table, 32, 8, 1)
    got, length = gpu_pack_tight((bits, meta, table), 32, 8, 1)
    assert length == len(want) and got[:length] == want


def test_slack_does_not_reach_the_stream(gpu, oracle):
    """Slot bytes past ceil(nbits / 8) and table words past ncodes (0xA5) and
    bits 24..31 of the live words change nothing."""
    (bits, meta, table), _, dims = crafted(oracle)
    want = T.pack(bits, meta, table, *dims)
    sb, st = bits.copy(), table.copy() | 0xC3000000
    col = np.arange(256)
    for c in range(3):
        o, n = J.SLOT_OFF[c], J.SLOT_CODES[c]
        k = col[None, o:o + n] - o
        sb[:, o:o + n][k >= (((meta[:, c] & 0xFFFF) + 7) // 8)[:, None]] = 0xA5
        st[:, o:o + n][k >= (meta[:, c] >> 24)[:, None]] = 0xA5A5A5A5
    assert not np.array_equal(sb, bits)
    got, length = gpu_pack_tight((sb, meta, st), *dims)
    assert length == len(want) and got[:length] == want


def test_capacity(gpu):
    arrays, _, want, dims = encoded65()
    need = len(want)
    mid = 16 + 2 * 65 + int(np.frombuffer(want[16:16 + 2 * 30], "<u2").sum()) + 7   # inside record 30
    for cap in (need, need - 1, mid, 16 + 2 * 30 + 1, 16):
        got, length = gpu_pack_tight(arrays, *dims, cap=cap, room=4096)
        assert length == need, cap
        assert got[:cap] == want[:cap], cap
        assert set(got[cap:]) == {0xEE}, cap


# ---- direct decode ---------------------------------------------------------------

def test_decode_crafted(gpu, oracle):
    """The packer's own stream of the crafted batch, whole and by range,
    against the slot decoder and the builders' expected ints."""
    arrays, want, dims = crafted(oracle)
    nt = want.shape[0]
    got, length = gpu_pack_tight(arrays, *dims)
    data = got[:length]
    ref, rejected = slot_decode(arrays)
    assert rejected == 0 and np.array_equal(ref, want)
    for tile0, ntile in ((0, nt), (5, 70), (nt - 130, 130)):
        coef, res = gpu_decode(data, len(data), dims, tile0, ntile)
        assert res == [len(data), U64, 0], (tile0, ntile)
        assert np.array_equal(coef, ref[tile0:tile0 + ntile]), (tile0, ntile)


def test_decode_image_one_of_three(gpu, oracle):
    arrays, coef = image_slots(oracle, 72, 40, "rand", 3)
    dims, per = (72, 40, 3), 45
    got, length = gpu_pack_tight(arrays, *dims)
    ref, rejected = slot_decode(arrays)
    assert rejected == 0 and np.array_equal(ref, coef)
    out, res = gpu_decode(got[:length], length, dims, per, per)
    assert res == [length, U64, 0] and np.array_equal(out, ref[per:2 * per])


def test_decode_counts_rejected_streams(gpu):
    """Random slots: the entropy decoder rejects most streams.  The direct
    decode of their JPT1 stream counts what the slot decoder counts, and
    gives what the direct decode of their JPR1 stream gives (the slot decoder
    leaves a rejected stream's ints unspecified; the direct decode zeroes
    them)."""
    arrays = I.random_slots(96)
    dims = (8 * 96, 8, 1)
    data, plain = T.pack(*arrays, *dims), J.pack(*arrays, *dims)
    for tile0, ntile in ((0, 96), (5, 70)):
        _, rejected = slot_decode(tuple(a[tile0:tile0 + ntile] for a in arrays))
        assert rejected > 0
        ref, ref_res = gpu_decode(plain, len(plain), dims, tile0, ntile)
        assert ref_res == [len(plain), U64, rejected], (tile0, ntile)
        coef, res = gpu_decode(data, len(data), dims, tile0, ntile)
        assert res == [len(data), U64, rejected], (tile0, ntile)
        assert np.array_equal(coef, ref), (tile0, ntile)


def test_forced_modes_decode_identically(gpu, oracle):
    """The crafted tables in mode 0 throughout, and in mode 2 wherever the
    writer chose mode 1."""
    arrays, want, dims = crafted(oracle)
    canon = T.stream_modes(*arrays)
    assert {0, 1, 2} <= set(canon.reshape(-1).tolist())
    streams = {"mode 0": np.zeros_like(canon), "mode 2 for 1": np.where(canon == 1, 2, canon),
               "canonical": canon}
    sizes = set()
    for name, modes in streams.items():
        data = T.pack(*arrays, *dims, modes=modes.tolist())
        sizes.add(len(data))
        coef, res = gpu_decode(data, len(data), dims)
        assert res == [len(data), U64, 0], name
        assert np.array_equal(coef, want), name
    assert len(sizes) == 3


# ---- malformed streams -----------------------------------------------------------

def _mutations(good):
    """(name, bytes, in_len) of one good 65-tile JPT1 stream."""
    nt = 65
    sizes = np.frombuffer(good[16:16 + 2 * nt], "<u2").astype(np.int64)
    offs = 16 + 2 * nt + np.concatenate([[0], np.cumsum(sizes)])
    recs = T.parse(good)[0]

    def put(pos, raw, base=good):
        b = bytearray(base)
        b[pos:pos + len(raw)] = raw
        return bytes(b)

    def stream_at(t, c):
        p = int(offs[t])
        for m, ents, raw, mode in recs[t][:c]:
            p += 4 + T.table_bytes(len(ents), mode) + len(raw)
        return p

    i40 = 16 + 2 * 40
    s40 = int(sizes[40])
    shifted = put(i40, (s40 + 1).to_bytes(2, "little") + (int(sizes[41]) - 1).to_bytes(2, "little"))
    shorter = put(i40, (s40 - 1).to_bytes(2, "little") + (int(sizes[41]) + 1).to_bytes(2, "little"))
    end40 = int(offs[41])
    padded = put(i40, (1040).to_bytes(2, "little"), good[:end40] + bytes(1040 - s40) + good[end40:])
    y40 = stream_at(40, 0)
    return [("tile 40 luma mode = 3", put(y40 + 3, bytes([good[y40 + 3] | 0xC0])), len(good)),
            ("tile 64 Cb nbits = 513", put(stream_at(64, 2) + 2,
                                           (513 | recs[64][2][3] << 14).to_bytes(2, "little")), len(good)),
            ("tile 40 luma ncodes = 129", put(y40 + 1, bytes([129])), len(good)),
            ("tile 40 one byte longer than its record", shifted, len(good)),
            ("tile 40 one byte shorter than its record", shorter, len(good)),
            ("index entry 40 = 1040", padded, len(padded)),
            ("in_len - 1", good, len(good) - 1),
            ("magic JPS1", put(2, b"S"), len(good)),
            ("index entry 40 + 1", put(i40, (s40 + 1).to_bytes(2, "little")), len(good))]


@pytest.mark.parametrize("k", range(9))
def test_malformed_streams(gpu, k):
    _, coef, good, dims = encoded65()
    name, data, in_len = _mutations(good)[k]
    recs, implied, verdict = T.parse(data[:in_len], dims)
    got, res = gpu_decode(data, in_len, dims)
    assert res[:2] == [implied, verdict], name
    if verdict == 0:
        assert not got.any() and res[2] == 0, name
        return
    bad = [t for t in range(65) if recs[t] is None]
    assert k < 6 and bad[0] == (64 if k == 1 else 40) and verdict == 1 + bad[0], name
    assert not got[bad].any(), name
    # tile 41's record moves by a byte with tile 40's index entry (k = 3, 4):
    # malformed, or by chance well-formed garbage; every other tile is exact
    sure = [t for t in range(65) if t not in bad and not (k in (3, 4) and t == 41)]
    assert len(sure) >= 63 and np.array_equal(got[sure], coef[sure]), name
    if len(sure) == 64:
        assert res[2] == 0, name


def test_malformed_last_tile(gpu):
    _, coef, good, dims = encoded65()
    name, data, in_len = _mutations(good)[1]
    recs, implied, verdict = T.parse(data, dims)
    assert verdict == 65 and recs[64] is None
    got, res = gpu_decode(data, in_len, dims)
    assert res == [implied, 65, 0] and not got[64].any() and np.array_equal(got[:64], coef[:64])
    got, res = gpu_decode(data, in_len, dims, 0, 64)        # outside the range: not examined
    assert res == [implied, U64, 0] and np.array_equal(got, coef[:64])


# ---- bounds ----------------------------------------------------------------------

def test_bytes_past_the_stream_do_not_matter(gpu, oracle):
    """in_len exact and the buffer ending with the stream, then 64 bytes of
    0x00 and of 0xFF behind it, at 0, 3 and 13 bytes off a 16-B boundary."""
    arrays, want, dims = crafted(oracle)
    data = T.pack(*arrays, *dims)
    runs = [gpu_decode(data, len(data), dims, tail=tail, lead=lead)
            for lead in (0, 3, 13) for tail in (b"", bytes(64), b"\xff" * 64)]
    for got, res in runs:
        assert res == [len(data), U64, 0]
        assert np.array_equal(got, want)


# ---- end to end ------------------------------------------------------------------

def test_graph_capture(gpu):
    """Tight pack + direct decode captured in one graph, replayed on two
    contents (the second holds the first's tiles in reverse order: a stream of
    the same length, which the captured in_len needs)."""
    import torch
    from lz4jpeg import jpeg
    nt, (w, h, nimg) = 65, (520, 8, 1)
    _, coef_a, want_a, _ = encoded65()
    coef_b = np.ascontiguousarray(coef_a[::-1])
    ent = jpeg.Entropy(nt)
    d_out = torch.zeros(jpeg.pack_bound(w, h, nimg), dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_res = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    d_back = torch.zeros(nt * 128, dtype=torch.int16, device="cuda")
    s1, s2 = pack_scratch(nt), pack_scratch(nt)

    def both():
        jpeg.pack_device(ent, w, h, nimg, d_out=d_out, d_len=d_len, scratch=s1, tight=True)
        jpeg.decode_stream_device(d_out, len(want_a), w, h, nimg, d_coef=d_back, d_result=d_res,
                                  scratch=s2)

    ent.encode(torch.zeros(nt * 128, dtype=torch.int16, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                              # warm-up on a third content
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    seen = []
    for coef in (coef_a, coef_b):
        d_coef = torch.from_numpy(coef.reshape(-1)).cuda()
        ent.encode(d_coef)
        torch.cuda.synchronize()
        want = T.pack(*slot_arrays(ent, nt), w, h, nimg)
        assert len(want) == len(want_a)
        d_out.zero_()
        d_back.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert int(d_len.item()) == len(want)
        assert d_out[:len(want)].cpu().numpy().tobytes() == want
        assert [int(x) & U64 for x in d_res.cpu().tolist()] == [len(want), U64, 0]
        assert torch.equal(d_back, d_coef)
        seen.append(want)
    assert seen[0] == want_a and seen[1] != want_a


@pytest.mark.parametrize("w,h,nimg,kind", [(40, 24, 1, "rand"), (72, 40, 3, "rand"), (512, 384, 1, "smooth")])
def test_compress_decompress(gpu, oracle, w, h, nimg, kind):
    import torch
    from lz4jpeg import jpeg
    img = np.concatenate([image(oracle, w, h, kind, seed=1 + i).reshape(-1) for i in range(nimg)])
    d_img = torch.from_numpy(img).cuda()
    tight = jpeg.compress_device(d_img, w, h, nimg, tight=True)
    plain = jpeg.compress_device(d_img, w, h, nimg)
    assert jpeg.stream_format(tight[:16].cpu().numpy().tobytes()) == (w, h, nimg, True)
    assert tight.numel() < plain.numel()
    arrays, _ = image_slots(oracle, w, h, kind, nimg)
    assert tight.cpu().numpy().tobytes() == T.pack(*arrays, w, h, nimg)
    rgba, gw, gh, gn = jpeg.decompress_images_device(tight)
    ref, _, _, _ = jpeg.decompress_images_device(plain)
    assert (gw, gh, gn) == (w, h, nimg) and torch.equal(rgba, ref)
    assert torch.equal(ref, jpeg.decompress_device(plain)[0])
    if nimg > 1:
        one, _, _, count = jpeg.decompress_images_device(tight, 1, 1)
        assert count == 1 and torch.equal(one, ref[w * h * 4:2 * w * h * 4])
    with pytest.raises(jpeg.JpegError):
        jpeg.decompress_device(tight)                       # no slot form of a JPT1 stream


def test_jpeg_dec_reads_both_formats(gpu, oracle, tmp_path):
    import torch
    from lz4jpeg import jpeg
    w, h = 72, 40
    img = np.concatenate([oracle.rand_image(w, h, seed=1 + i).reshape(-1) for i in range(3)])
    d_img = torch.from_numpy(img).cuda()
    pngs = []
    for name, tight in (("plain.jpr", False), ("tight.jpr", True)):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(jpeg.compress_device(d_img, w, h, 3, tight=tight).cpu().numpy().tobytes())
        for image in ("0", "2"):
            out = path + image + ".png"
            r = subprocess.run([os.path.join(BIN, "JPEG_dec"), path, out, image], capture_output=True,
                               timeout=120)
            assert r.returncode == 0, r.stderr
            pngs.append(open(out, "rb").read())
    assert pngs[0] == pngs[2] and pngs[1] == pngs[3] and pngs[0] != pngs[1]
