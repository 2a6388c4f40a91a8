"""The three writers of the JPR stream (jpegr_pack_device,
jpegr_pack_tight_device, jpegr_stream_encode_device in both formats;
include/jpegr.h) at the capacities where their shared LDS image -> stream
flush can go wrong.  The expected bytes are the plain-Python restatements'
(tests/jpr_format.py, tests/jpt_format.py) of the entropy stage's slots.

33 tiles (264 x 8, one image) are three workgroups of 16, 16 and 1 tiles: both
interior run boundaries fall inside a 16-B chunk that two workgroups share, and
the last run is a single tile.  The caps sit around the header and the index
(I = 16 + 2 * 33), and 17, 16, 15, 1 and 0 B either side of each run's first
byte and of the stream's end, so a clipped flush ends before, on and after a
chunk boundary, in a whole chunk and in either shared one."""
import numpy as np
import pytest

import jpt_format as T
from jpr_gpu_lib import Slots, coef_dev, current_stream, encoded, encoded_jpr, pack_scratch, vp

pytestmark = pytest.mark.gpu

NT, DIMS = 33, (264, 8, 1)
ROOM, FILL = 4096, 0xEE
INDEX_END = 16 + 2 * NT
WRITERS = ["pack", "pack_tight", "stream_encode", "stream_encode_tight"]


def _caps(want):
    sizes = np.frombuffer(want[16:INDEX_END], "<u2").astype(np.int64)
    offs = INDEX_END + np.concatenate([[0], np.cumsum(sizes)])
    assert int(offs[NT]) == len(want)
    caps = {0, 1, 15, 16, 17, INDEX_END - 1, INDEX_END, INDEX_END + 1}
    for g in (int(offs[16]), int(offs[32]), len(want)):
        caps |= {g + d for d in (-17, -16, -15, -1, 0, 1, 15, 16, 17)}
    return sorted(c for c in caps if c >= 0)


class Writer:
    """One writer's inputs on the device; __call__(cap) -> (bytes of the whole
    output allocation, the reported length)."""

    def __init__(self, name, arrays, coef):
        import torch
        from lz4jpeg import _lib
        self.L = _lib.lib()
        self.name, self.tight = name, name.endswith("tight")
        self.bound = int(self.L.jpegr_pack_bound(*DIMS))
        self.st = current_stream()
        if name.startswith("pack"):
            self.slots = Slots(NT).load(*arrays)
            self.scr = pack_scratch(NT)
        else:
            self.coef = coef_dev(coef)

    def __call__(self, cap):
        import torch
        out = torch.full((self.bound + ROOM,), FILL, dtype=torch.uint8, device="cuda")
        d_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        if self.name.startswith("pack"):
            fn = self.L.jpegr_pack_tight_device if self.tight else self.L.jpegr_pack_device
            s = self.slots
            rc = fn(vp(s.bits), vp(s.meta), vp(s.table), *DIMS, vp(out), cap, vp(d_len),
                    vp(self.scr), self.st)
        else:
            scr = torch.empty(int(self.L.jpegr_stream_encode_scratch_bytes(NT, cap)), dtype=torch.uint8,
                              device="cuda")
            res = torch.zeros(2, dtype=torch.int64, device="cuda")
            rc = self.L.jpegr_stream_encode_device(vp(self.coef), *DIMS, 2 if self.tight else 1, vp(out),
                                                   cap, vp(d_len), vp(scr), vp(res), self.st)
        assert rc == 0
        torch.cuda.synchronize()
        return out.cpu().numpy().tobytes(), int(d_len.item())


@pytest.mark.parametrize("name", WRITERS)
def test_caps(gpu, name):
    arrays, coef, dims = encoded(NT, *DIMS)
    assert dims == DIMS
    want = T.pack(*arrays, *DIMS) if name.endswith("tight") else encoded_jpr(NT, *DIMS)
    caps = _caps(want)
    assert len(caps) >= 30 and caps[-1] == len(want) + 17
    writer = Writer(name, arrays, coef)
    for cap in caps:
        got, length = writer(cap)
        assert length == len(want), cap
        n = min(cap, len(want))                             # (a cap past the stream: nothing behind it either)
        assert got[:n] == want[:n], cap
        assert set(got[n:]) == {FILL}, cap
