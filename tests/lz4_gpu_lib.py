"""Driving lz4jpeg.lz4.Compressor on the device and comparing everything a call
left behind with lz4_seq_inputs.Expected (a helper, no tests).
"""
import ctypes

import numpy as np

from lz4_seq_inputs import BLK


def compressor():
    """For a module's `comp` fixture: `yield from lz4_gpu_lib.compressor()`."""
    from lz4jpeg.lz4 import Compressor
    c = Compressor()
    yield c
    c.close()


def block_sizes(comp, count):
    """The last call's first `count` per-block sizes as the device holds them
    (uint16; lz4r_copy_block_sizes on the compressor's handle)."""
    import torch
    from lz4jpeg import _lib
    out = np.empty(count, dtype=np.uint16)
    rc = _lib.lib().lz4r_copy_block_sizes(comp._h, out.ctypes.data_as(ctypes.c_void_p), count,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.LZ4R_OK, rc
    return out


def compress(comp, data, misalign=0, lead=0, cap=None, segment=False, final_shard=None):
    """compress_async of `data` placed `misalign` bytes into a fresh device
    buffer, its output `lead` bytes into one -> (the whole output buffer, the
    length word, the device block offsets, the device block sizes); the
    buffer is 0xEE where the call wrote nothing, ends 64 bytes behind the
    bound, and the call's capacity is `cap` (default: all of it)."""
    import torch
    from lz4jpeg.lz4 import compress_bound
    n = len(data)
    d_buf = torch.empty(misalign + n, dtype=torch.uint8, device="cuda")
    assert d_buf.data_ptr() % 4 == 0
    d_in = d_buf[misalign:]
    d_in.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    d_all = torch.full((lead + compress_bound(n) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert d_all.data_ptr() % 16 == 0
    d_out = d_all[lead:] if cap is None else d_all[lead:lead + cap]
    d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    comp.compress_async(d_in, n, d_out, d_len, segment=segment, final_shard=final_shard)
    torch.cuda.synchronize()
    word = int(d_len.item())
    assert word >= 0, "bit 63 of the length word: a corrupt bucket head"
    nb = (n + BLK - 1) // BLK
    return d_all.cpu().numpy().tobytes(), word, comp.block_offsets(nb), block_sizes(comp, nb)


def check(comp, exp, framed=True, where=None, lead=0, cap=None, **kw):
    """One call on exp.data against the oracle: the length word, every stream
    byte below the capacity (a mismatch names the first differing block), the
    0xEE before the output and past the stream or the capacity, the device
    block offsets and sizes."""
    want = exp.framed() if framed else exp.body()
    buf, word, offs, sizes = compress(comp, exp.data, lead=lead, cap=cap, **kw)
    assert word == len(want), where
    lim = len(want) if cap is None else min(cap, len(want))
    got = buf[lead:lead + lim]
    if got != want[:lim]:
        # the first block that differs, by the oracle's offsets
        o = exp.offsets() + (1 if framed else 0)
        bad = next(b for b in range(exp.nb)
                   if got[o[b]:o[b] + len(exp.blocks[b])] != exp.blocks[b][:max(0, lim - o[b])])
        raise AssertionError((where, "block", bad, "of", exp.nb, "counts", exp.counts()[
            max(0, bad - 4):bad + 2]))
    assert buf[:lead] == b"\xee" * lead, where
    assert buf[lead + lim:] == b"\xee" * (len(buf) - lead - lim), where
    assert np.array_equal(offs.astype(np.int64), exp.offsets()), where
    bad = np.flatnonzero(sizes != exp.sizes())
    assert not bad.size, (where, "block", int(bad[0]), "size", int(sizes[bad[0]]), "want",
                          int(exp.sizes()[bad[0]]))
