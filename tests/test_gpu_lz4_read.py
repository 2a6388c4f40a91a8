"""lz4r_read_device, lz4r_stream_index_device and lz4.Reader on the GPU.

Every comparison is byte equality with slices of the plaintext, through the
model of lz4_read_model.py: the WHOLE output buffer (pre-filled with 0xA5,
guard bytes on both sides of the call's capacity, a one-byte gap between
packed reads) and both result words.  Only the destination ranges of reads
that fail inside a block are left out (the contract leaves them unspecified).
"""
import ctypes

import numpy as np
import pytest

import golden_inputs
import lz4_format as F
import lz4_read_model as M
from test_gpu_decode_paths import WAVE_COUNTS, all_streams

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64
U64 = 1 << 64


def packed(pairs, gap=1, at=0):
    """(src, len) pairs -> (src, len, dst) reads placed one after another with
    `gap` untouched bytes between them, and the bytes they span."""
    reads = []
    for src, ln in pairs:
        reads.append((src, ln, at))
        at += ln + gap
    return reads, at


class Batch:
    """Queues lz4r_read_device calls through the C ABI on one input, one
    offsets, one reads, one output and one result tensor, reads everything
    back once and compares every call with the model."""

    def __init__(self):
        self.jobs = []

    def add(self, st, reads, max_len, out_cap=None, bad_blocks=(), offs=None, stream=None,
            align=0, tag=None):
        """st: {"stream", "offs", "plain"}; offs / stream: what the call is
        given instead (the model keeps judging by st["plain"])."""
        if out_cap is None:
            out_cap = max([d + n for _, n, d in reads if n] + [1])
        self.jobs.append({"st": st, "reads": reads, "max_len": max_len, "cap": out_cap,
                          "bad": tuple(bad_blocks), "offs": st["offs"] if offs is None else offs,
                          "stream": st["stream"] if stream is None else stream, "align": align,
                          "tag": tag or st.get("name", "")})

    def run(self):
        import torch
        from lz4jpeg import _lib
        L = _lib.lib()
        ins, offs, reads = bytearray(), [], []
        o_at = 0
        for j in self.jobs:
            j["in_at"], j["off_at"], j["rd_at"] = len(ins), len(offs), len(reads)
            ins += j["stream"]
            offs += [int(x) % U64 for x in j["offs"]]
            reads += [[x % U64 for x in rd] for rd in j["reads"]]
            j["out_at"] = o_at + GUARD + j["align"]            # o_at is a multiple of 16
            o_at += (GUARD + 16 + j["cap"] + GUARD + 15) & ~15
        d_in = torch.from_numpy(np.frombuffer(bytes(ins), dtype=np.uint8).copy()).cuda()
        d_offs = torch.from_numpy(np.asarray(offs, dtype=np.uint64).view(np.int64)).cuda()
        d_reads = torch.from_numpy(np.asarray(reads, dtype=np.uint64).reshape(-1, 3)
                                   .view(np.int64)).cuda()
        d_out = torch.full((o_at,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_res = torch.full((len(self.jobs), 2), 7, dtype=torch.int64, device="cuda")
        assert d_out.data_ptr() % 16 == 0
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for k, j in enumerate(self.jobs):
            rc = L.lz4r_read_device(
                ctypes.c_void_p(d_in.data_ptr() + j["in_at"]), len(j["stream"]),
                ctypes.c_void_p(d_offs.data_ptr() + 8 * j["off_at"]), len(j["offs"]),
                ctypes.c_void_p(d_reads.data_ptr() + 24 * j["rd_at"]), len(j["reads"]),
                j["max_len"], ctypes.c_void_p(d_out.data_ptr() + j["out_at"]), j["cap"],
                ctypes.c_void_p(d_res.data_ptr() + 16 * k), stream)
            assert rc == 0, (j["tag"], rc)
        torch.cuda.synchronize()
        self.out = d_out.cpu().numpy()
        self.res = d_res.cpu().numpy().view(np.uint64)

    def check(self):
        want = np.full(self.out.size, SENTINEL, dtype=np.uint8)
        keep = np.ones(self.out.size, dtype=bool)
        for k, j in enumerate(self.jobs):
            plain = j["st"]["plain"]
            buf, delivered, verdict = M.expected(plain, j["reads"], j["cap"], j["max_len"],
                                                 SENTINEL, j["bad"])
            want[j["out_at"]:j["out_at"] + j["cap"]] = buf
            for a, b in M.loose_ranges(plain, j["reads"], j["cap"], j["max_len"], j["bad"]):
                keep[j["out_at"] + a:j["out_at"] + b] = False
            got = (int(self.res[k, 0]), int(self.res[k, 1]))
            assert got == (delivered, verdict), (j["tag"], "result", got, (delivered, verdict))
        diff = np.flatnonzero((self.out != want) & keep)
        if diff.size:
            at = int(diff[0])
            j = max((j for j in self.jobs if j["out_at"] - GUARD - j["align"] <= at),
                    key=lambda j: j["out_at"])
            rel = at - j["out_at"]
            rd = [(k, r) for k, r in enumerate(j["reads"]) if r[2] <= rel < r[2] + r[1]]
            raise AssertionError(f"{j['tag']}: output byte {rel} of {j['cap']}: got "
                                 f"{self.out[at]}, expected {want[at]}; {diff.size} differ; "
                                 f"reads there: {rd[:3]}")


def run(st, reads, max_len, **kw):
    b = Batch()
    b.add(st, reads, max_len, **kw)
    b.run()
    b.check()


# ---- streams -------------------------------------------------------------------------
_cache = {}


def text_stream(oracle, n):
    """The first n bytes of the text, compressed by the oracle."""
    if ("text", n) not in _cache:
        data = golden_inputs.lz4_input("metamorphosis_spaces")[:n]
        assert len(data) == n
        s = oracle.lz4_compress(data)
        _cache["text", n] = {"name": f"text {n}", "stream": s, "offs": F.walk_offsets(s),
                             "plain": data}
    return _cache["text", n]


def five_blocks(oracle):
    st = text_stream(oracle, 1217)
    assert len(st["offs"]) == 5
    return st


def mixed_mib():
    """1 MiB: passages of text and runs of random bytes in turn."""
    if "mixed" not in _cache:
        from lz4jpeg import synth
        rng = np.random.default_rng(20)
        text = synth.random_passages(1 << 20, length=3000, seed=5)
        rnd = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
        pick = np.repeat(rng.integers(0, 4, (1 << 20) // 512) == 0, 512)   # a quarter random
        _cache["mixed"] = np.where(pick, rnd, text).astype(np.uint8).tobytes()
    return _cache["mixed"]


@pytest.fixture(scope="module")
def comp():
    import lz4_gpu_lib
    yield from lz4_gpu_lib.compressor()


def compressed(comp, data):
    """A stream from the GPU compressor and its offsets, on the host."""
    import torch
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    d_stream, length = comp.compress_device(d)
    offs = comp.block_offsets((len(data) + 299) // 300)
    return {"name": "compressed", "stream": d_stream[:length].cpu().numpy().tobytes(),
            "offs": [int(x) for x in offs], "plain": data}


# ---- 1. every cut ---------------------------------------------------------------------

def test_every_cut(gpu, oracle):
    """Every src of a 5-block stream with lengths around the store phase's
    and the blocks' edges: ~18 k reads in one call, destinations at every
    alignment mod 16."""
    st = five_blocks(oracle)
    n = 1217
    pairs = []
    for src in range(n):
        lens = {0, 1, 2, 3, 4, 15, 16, 17, 299, 300, 301, 599, 600, 601, n - src}
        pairs += [(src, ln) for ln in sorted({min(ln, n - src) for ln in lens})]
    reads, span = packed(pairs)
    assert {d % 16 for _, _, d in reads} == set(range(16)) and len(reads) > 15000
    run(st, reads, n, out_cap=span, align=3)


# ---- 2. parser paths ------------------------------------------------------------------

def block_reads(n):
    """One read per block (whole) and one across each block boundary."""
    nb = (n + 299) // 300
    pairs = [(300 * b, min(300, n - 300 * b)) for b in range(nb)]
    pairs += [(300 * b - 7, min(16, n - (300 * b - 7))) for b in range(1, nb)]
    return packed(pairs)[0]


def test_parser_paths(gpu, oracle):
    """Every stream of test_gpu_decode_paths (the plain path, the general path
    with choice points and truncated readings, the checked tail path) read
    through the new kernel."""
    b = Batch()
    for k, st in enumerate(all_streams(oracle)):
        b.add(st, block_reads(len(st["plain"])), 300, align=k % 16)
    b.run()
    b.check()


# ---- 3. scattered waves ---------------------------------------------------------------

def test_scattered_waves(gpu, comp):
    """A wave whose items alternate between the first and the last 4 KiB of a
    stream of more than 2 MiB: unchecked and checked loads side by side."""
    from lz4jpeg import synth
    text = synth.random_passages(300 * 3600, length=3000, seed=8).tobytes()
    st = compressed(comp, text + text)
    n = len(st["plain"])
    assert len(st["stream"]) > 2 << 20
    rng = np.random.default_rng(3)
    pairs = []
    for r in range(256):
        ln = int(rng.integers(1, 65))
        at = int(rng.integers(0, 4096 - ln + 1))
        pairs.append((at if r % 2 == 0 else n - 4096 + at, ln))
    pairs += [(n - 64, 64), (0, 64), (n - 1, 1)]
    run(st, packed(pairs)[0], 64)


# ---- 4. wave shapes -------------------------------------------------------------------

def test_wave_shapes(gpu, oracle):
    st = text_stream(oracle, 300 * 96)
    n = len(st["plain"])
    rng = np.random.default_rng(4)
    b = Batch()
    for cnt in WAVE_COUNTS:                                   # K = 2
        pairs = [(int(rng.integers(0, n - 300)), int(rng.integers(1, 301))) for _ in range(cnt)]
        b.add(st, packed(pairs)[0], 300, tag=f"{cnt} reads")
    for nblk in (33, 65):                                     # one destination across waves
        ln = 300 * (nblk - 2) + 2 * 50
        assert (250 + ln - 1) // 300 - 0 + 1 == nblk
        b.add(st, [(250, ln, 5)], ln, tag=f"{nblk} blocks")
        b.add(st, [(7, 1, 0), (250, ln, 5), (n - 1, 1, 2)], ln + 299, align=9,
              tag=f"{nblk} blocks, K larger")
    pairs = [(int(rng.integers(0, n)), 1) for _ in range(100)]
    b.add(st, packed(pairs)[0], 3000, tag="nine idle items in ten")
    pairs = [(int(rng.integers(0, n - 3000)), 3000 if k % 3 == 1 else 1) for k in range(40)]
    b.add(st, packed(pairs)[0], 3000, tag="1 and 3000 mixed")
    b.run()
    b.check()


# ---- 5. bad reads ---------------------------------------------------------------------

def test_bad_reads(gpu, oracle):
    st = five_blocks(oracle)
    n, cap = 1217, 4000
    good, span = packed([(0, 300), (293, 16), (600, 300), (1200, 17), (1216, 1), (5, 0),
                         (100, 700), (899, 2), (1199, 18)])
    assert span < cap - 800
    at = span                                                 # where a bad read would land
    bad = {
        "past the end in the last block": (1210, 8, at),
        "src at the decoded length": (1217, 1, at),
        "len = max_len + 1": (10, 701, at),
        "dst + len = out_cap + 1": (10, 20, cap + 1 - 20),
        "src + len wraps": (U64 - 10, 10, at),
        "src + len wraps to the stream": (U64 - 10, 20, at),
        "block index >= nb": (1500, 1, at),
        "last block index >= nb": (1100, 500, at),
    }
    b = Batch()
    for name, rd in bad.items():
        b.add(st, good[:3] + [rd] + good[3:], 700, out_cap=cap, tag=name)
    b.add(st, good[:2] + [bad["src at the decoded length"]] + good[2:5] +
          [bad["len = max_len + 1"]] + good[5:], 700, out_cap=cap, tag="two together")
    b.add(st, [bad["len = max_len + 1"]] + good + [bad["past the end in the last block"]], 700,
          out_cap=cap, tag="two together, the other order")
    # block 2's nseq byte zeroed: the reads that touch it are bad, all others exact
    probe = block_reads(n) + [(s, ln, 2000 + 710 * k) for k, (s, ln) in
                              enumerate([(100, 700), (0, 600), (599, 1), (900, 317)])]
    broken = bytearray(st["stream"])
    broken[1 + st["offs"][2]] = 0
    b.add(st, probe, 700, out_cap=cap + 1000, stream=bytes(broken), bad_blocks=(2,),
          tag="nseq of block 2 zeroed")
    # an offsets array with one entry past in_len: the block it starts and the
    # block it ends are malformed
    offs = list(st["offs"])
    offs[3] = len(st["stream"]) + 5
    b.add(st, probe, 700, out_cap=cap + 1000, offs=offs, bad_blocks=(2, 3),
          tag="offset past in_len")
    offs = list(st["offs"])
    offs[1] = U64 - 3                                         # 1 + offset wraps
    b.add(st, probe, 700, out_cap=cap + 1000, offs=offs, bad_blocks=(0, 1),
          tag="offset near 2^64")
    b.run()
    b.check()


# ---- 6. round trip from the compressor ---------------------------------------------------

def test_round_trip_from_compressor(gpu, comp):
    """The compressor's own offsets by their device pointer: 4096 random
    reads, then the whole stream as one read."""
    import torch
    from lz4jpeg import lz4
    data = mixed_mib()
    n = len(data)
    plain = np.frombuffer(data, dtype=np.uint8)
    d_in = torch.from_numpy(plain.copy()).cuda()
    d_stream, length = comp.compress_device(d_in)
    ptr, nb = comp.block_offsets_device()
    assert nb == (n + 299) // 300
    rng = np.random.default_rng(6)
    ln = rng.integers(1, 701, 4096)
    src = rng.integers(0, n - 700, 4096)
    d_src, d_len = torch.from_numpy(src).cuda(), torch.from_numpy(ln).cuda()
    d_out, d_dst, got = lz4.read_device(d_stream, length, ptr, nb, d_src, d_len, 700)
    assert got == int(ln.sum()) == d_out.numel()
    out, dst = d_out.cpu().numpy(), d_dst.cpu().numpy()
    assert np.array_equal(dst, np.cumsum(ln) - ln)
    want = np.concatenate([plain[s:s + k] for s, k in zip(src, ln)])
    assert np.array_equal(out, want)
    whole = torch.tensor([0], dtype=torch.int64, device="cuda")
    d_out, _, got = lz4.read_device(d_stream, length, ptr, nb, whole,
                                    torch.tensor([n], dtype=torch.int64, device="cuda"), n)
    assert got == n and torch.equal(d_out, d_in)
    with pytest.raises(lz4.Lz4Error, match="read 1"):
        lz4.read_device(d_stream, length, ptr, nb, torch.tensor([0, n - 3], device="cuda"),
                        torch.tensor([4, 4], device="cuda"), 4)


# ---- 7. the index ---------------------------------------------------------------------

def _index(d_stream, length, cap):
    import torch
    from lz4jpeg import _lib
    d_offs = torch.full((cap + 2,), -1, dtype=torch.int64, device="cuda")     # two guard entries
    nb, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = _lib.lib().lz4r_stream_index_device(
        ctypes.c_void_p(d_stream.data_ptr()), length, ctypes.c_void_p(d_offs.data_ptr()), cap,
        ctypes.byref(nb), ctypes.byref(n), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, nb.value, n.value, d_offs.cpu().numpy()


def test_index_of_built_streams(gpu, oracle):
    """Offsets, block count and decoded length of every hand-built stream
    (those with truncated matches take the exact pass), a capacity one short,
    and the bare decode of the same streams (the refactored pass)."""
    import torch
    from lz4jpeg import _lib, lz4
    for st in all_streams(oracle):
        s, offs, plain = st["stream"], st["offs"], st["plain"]
        d = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
        d_offs, nb, n = lz4.stream_index_device(d, len(s))
        assert (nb, n) == (len(offs), len(plain)), st["name"]
        assert d_offs.cpu().tolist() == list(offs), st["name"]
        rc, need, n1, got = _index(d, len(s), nb - 1)
        assert (rc, need, n1) == (_lib.LZ4R_ERR_CAPACITY, nb, 0), st["name"]
        assert got[nb - 1] == -1 and got[nb] == -1, st["name"]     # nothing past the capacity
        rc, nb2, n2, got = _index(d, len(s), nb)
        assert (rc, nb2, n2) == (0, nb, len(plain)) and got[nb] == -1, st["name"]
        d_out, m = lz4.decompress_stream_device(d, len(s), len(plain))
        assert m == len(plain) and d_out[:m].cpu().numpy().tobytes() == plain, st["name"]


def test_index_of_compressed_stream(gpu, comp):
    import torch
    from lz4jpeg import _lib, lz4
    st = compressed(comp, mixed_mib())
    s = st["stream"]
    d = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).cuda()
    d_offs, nb, n = lz4.stream_index_device(d, len(s))
    assert (nb, n) == (len(st["offs"]), len(st["plain"]))
    assert d_offs.cpu().tolist() == st["offs"]
    # the first guess of the wrapper is too small for a stream of tiny blocks
    tiny = F.write_frame([F.write_block([(1, 1, 4)] + [(0, 1, 255)] + [(0, 1, 40)], F.Literals(b"x"))
                          for _ in range(200)])
    dt = torch.from_numpy(np.frombuffer(tiny[0], dtype=np.uint8).copy()).cuda()
    assert len(tiny[0]) // 64 + 64 < 200
    t_offs, t_nb, t_n = lz4.stream_index_device(dt, len(tiny[0]))
    assert (t_nb, t_n) == (200, 60000) and t_offs.cpu().tolist() == list(tiny[1])
    # a flipped size field
    bad = bytearray(s)
    at = 1 + st["offs"][1000]
    bad[at + 1] ^= 0x10
    db = torch.from_numpy(np.frombuffer(bytes(bad), dtype=np.uint8).copy()).cuda()
    rc, nb3, n3, _ = _index(db, len(bad), nb + 8)
    assert (rc, nb3, n3) == (_lib.LZ4R_ERR_CORRUPT, 0, 0)
    with pytest.raises(lz4.Lz4Error):
        lz4.stream_index_device(db, len(bad))
    d_out, m = lz4.decompress_stream_device(d, len(s), n)
    assert m == n and d_out[:m].cpu().numpy().tobytes() == st["plain"]


# ---- 8. Reader ------------------------------------------------------------------------

def test_reader(gpu, oracle):
    import torch
    from lz4jpeg import lz4
    st = text_stream(oracle, 300 * 96 + 17)
    plain = np.frombuffer(st["plain"], dtype=np.uint8)
    n = plain.size
    d = torch.from_numpy(np.frombuffer(st["stream"], dtype=np.uint8).copy()).cuda()
    rd = lz4.Reader(d)
    assert (rd.nb, rd.decoded_length) == (97, n)
    given = lz4.Reader(d, len(st["stream"]), rd.d_offsets, rd.nb)     # the caller's offsets
    assert (given.nb, given.decoded_length) == (97, n)
    for src, ln in [(0, 1), (n - 1, 1), (300 * 96 - 5, 22), (0, n), (40, 0)]:
        got = rd.read(src, ln)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), plain[src:src + ln])
    with pytest.raises(lz4.Lz4Error, match="read 0"):
        rd.read(n - 1, 2)
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    d_out, d_dst, got = rd.read_many(empty, empty, 64)
    assert d_out.numel() == 0 and d_dst.numel() == 0 and got == 0

    # check=False: no read-back; one linear capture, replayed on two sets of reads
    nr, ml = 48, 400
    rng = np.random.default_rng(8)
    d_src = torch.zeros(nr, dtype=torch.int64, device="cuda")
    d_len = torch.ones(nr, dtype=torch.int64, device="cuda")
    d_dst = torch.arange(nr, dtype=torch.int64, device="cuda") * (ml + 1)
    d_out = torch.empty(nr * (ml + 1), dtype=torch.uint8, device="cuda")

    def call():
        return rd.read_many(d_src, d_len, ml, d_dst=d_dst, d_out=d_out, check=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call()[2] is None                              # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        src = rng.integers(0, n - ml, nr)
        ln = rng.integers(1, ml + 1, nr)
        d_src.copy_(torch.from_numpy(src))
        d_len.copy_(torch.from_numpy(ln))
        d_out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        want = np.full(nr * (ml + 1), SENTINEL, dtype=np.uint8)
        for k in range(nr):
            want[k * (ml + 1):k * (ml + 1) + ln[k]] = plain[src[k]:src[k] + ln[k]]
        assert np.array_equal(d_out.cpu().numpy(), want)
