#!/usr/bin/env python3
"""Time lz4r_compress_frame_async (a standard LZ4 frame) beside
lz4r_compress_async (the native stream) on an MI355X: same text, one process,
one run.

    python tools/lz4_frame_bench.py [--mib 1024] [--reps 15] [--seed 1] [--verify]

Corpus: --mib MiB of text (synth.random_passages_device, as
tools/lz4_read_bench.py builds its own).  Each call has a context of its own
with timing on: the library rides its events on the kernels' dispatch packets
(lz4r_set_timing), so a sample is the first lz4_tiles' start to the last
emission kernel's end, and the call less its lz4_tiles launches is the three
launches after it (sizes / scan / emit; reduce / scan / emit natively).  After
a warm-up of three calls each, --reps samples per call, the two alternated;
the median and the spread (min .. max) are printed as ms per GiB of input, then
both outputs' sizes and one JSON line.  --verify decodes the frame on the host
and compares it with the text (slow at 1 GiB).

    python tools/lz4_frame_bench.py --decode [--mib 1024] [--linked-mib 64] [--host-mib 64]

times the decoders instead, as ms per GiB of decoded bytes, side by side:
lz4r_frame_decompress_device on this library's frame of the text, on a 4 MiB-
class frame of independent blocks and on a 64 KiB-class frame of linked blocks
(both written once on the host by the system's liblz4, when there is one; the
linked one over the first --linked-mib MiB, scaled), lz4r_decompress_stream_device
on the native stream, and lz4r_frame_decompress on the host (the first
--host-mib MiB of this library's frame, scaled).  A sample is the wall time of
one call, which synchronises; three warm-up calls, then --reps samples of each.
Every output is compared with the text once.  The per-kernel split comes from
a kernel-trace run of this mode (rocprofv3 --kernel-trace --stats) at --mib 256.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lz4-jpeg_amd"))


def liblz4_frame(plain, block_id, linked):
    """`plain` (bytes-like) as one frame by the system's liblz4: block maximum
    class block_id (4: 64 KiB, 7: 4 MiB), no checksums; None without liblz4."""
    import ctypes
    import ctypes.util
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    L = ctypes.CDLL(name)

    class FrameInfo(ctypes.Structure):
        _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int),
                    ("contentChecksumFlag", ctypes.c_int), ("frameType", ctypes.c_int),
                    ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                    ("blockChecksumFlag", ctypes.c_int)]

    class Prefs(ctypes.Structure):
        _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int),
                    ("autoFlush", ctypes.c_uint), ("favorDecSpeed", ctypes.c_uint),
                    ("reserved", ctypes.c_uint * 3)]

    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    L.LZ4F_isError.argtypes = [sz]
    L.LZ4F_compressFrameBound.argtypes = [sz, ctypes.POINTER(Prefs)]
    L.LZ4F_compressFrameBound.restype = sz
    L.LZ4F_compressFrame.argtypes = [vp, sz, vp, sz, ctypes.POINTER(Prefs)]
    L.LZ4F_compressFrame.restype = sz
    p = Prefs()
    p.frameInfo.blockSizeID = block_id
    p.frameInfo.blockMode = 0 if linked else 1
    p.frameInfo.contentSize = len(plain)
    cap = L.LZ4F_compressFrameBound(len(plain), ctypes.byref(p))
    dst = ctypes.create_string_buffer(cap)
    src = (ctypes.c_char * len(plain)).from_buffer_copy(plain)
    n = L.LZ4F_compressFrame(dst, cap, src, len(plain), ctypes.byref(p))
    assert not L.LZ4F_isError(n), "LZ4F_compressFrame"
    return dst.raw[:n]


def decode_bench(args):
    from ctypes import byref, c_size_t

    import numpy as np
    import torch
    from lz4jpeg import _lib, lz4, synth
    assert torch.cuda.is_available(), "lz4_frame_bench.py needs a GPU"
    n = args.mib << 20
    n_linked, n_host = min(args.linked_mib << 20, n), min(args.host_mib << 20, n)
    d_plain = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.random_passages_device(d_plain, n, seed=args.seed)
    c = lz4.Compressor()
    d_frame, frame_len = c.compress_frame_device(d_plain)
    d_frame = d_frame[:frame_len].clone()
    d_native, native_len = c.compress_device(d_plain)
    d_native = d_native[:native_len].clone()
    c.close()
    plain = d_plain.cpu().numpy()
    d_out = torch.empty(n + 300, dtype=torch.uint8, device="cuda")

    def on_device(b):
        return None if b is None else torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()

    d_big = on_device(liblz4_frame(plain, 7, False))
    d_linked = on_device(liblz4_frame(plain[:n_linked], 4, True))
    host_frame = lz4.compress_frame(plain[:n_host].tobytes()) if n_host < n else \
        d_frame.cpu().numpy().tobytes()
    host_out = np.empty(n_host, dtype=np.uint8)
    host_in = np.frombuffer(host_frame, np.uint8)

    def frame_call(d_f, size):
        def call():
            _, got = lz4.decompress_frame_device(d_f, d_out=d_out, cap=size)
            assert got == size
        return call

    def native_call():
        _, got = lz4.decompress_stream_device(d_native, native_len, n + 300, d_out=d_out)
        assert got == n

    def host_call():
        got = c_size_t(0)
        rc = _lib.call("lz4r_frame_decompress", host_in, host_in.size, host_out, n_host, byref(got))
        assert rc == 0 and got.value == n_host

    rows = [("frame_own", "lz4r_frame_decompress_device, this library's frame", frame_call(d_frame, n),
             n, frame_len)]
    if d_big is not None:
        rows.append(("frame_4mib_independent", "the same, a 4 MiB-class independent frame (liblz4)",
                     frame_call(d_big, n), n, d_big.numel()))
        rows.append(("frame_64kib_linked", f"the same, a 64 KiB linked frame (liblz4), "
                     f"{n_linked >> 20} MiB scaled", frame_call(d_linked, n_linked), n_linked,
                     d_linked.numel()))
    else:
        print("no system liblz4: the 4 MiB-class and the linked frame are not measured")
    rows.append(("native_stream", "lz4r_decompress_stream_device, the native stream", native_call, n,
                 native_len))
    rows.append(("host_frame", f"lz4r_frame_decompress on the host, {n_host >> 20} MiB scaled",
                 host_call, n_host, len(host_frame)))
    out = {"mode": "decode", "mib": args.mib, "reps": args.reps}
    for key, label, call, size, packed in rows:
        for _ in range(3):
            call()
        if key != "host_frame":                          # the bytes, once
            torch.cuda.synchronize()
            assert torch.equal(d_out[:size], d_plain[:size]), key
        else:
            assert np.array_equal(host_out, plain[:n_host]), key
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3 * (1 << 30) / size)
        out[key + "_ms_per_gib"] = (statistics.median(ms), min(ms), max(ms))
        out[key + "_bytes"] = packed
        print(f"{label}: {statistics.median(ms):.3f} ms/GiB ({min(ms):.3f} .. {max(ms):.3f}); "
              f"{packed} B in, {size} B out")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--linked-mib", type=int, default=64)
    ap.add_argument("--host-mib", type=int, default=64)
    args = ap.parse_args()
    if args.decode:
        return decode_bench(args)

    import torch
    from lz4jpeg import lz4, synth
    assert torch.cuda.is_available(), "lz4_frame_bench.py needs a GPU"
    n = args.mib << 20
    d_plain = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.random_passages_device(d_plain, n, seed=args.seed)
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_native = torch.empty(lz4.compress_bound(n), dtype=torch.uint8, device="cuda")
    d_frame = torch.empty(lz4.frame_bound(n), dtype=torch.uint8, device="cuda")
    native, frame = lz4.Compressor(), lz4.Compressor()
    calls = {
        "native": (native, lambda: native.compress_async(d_plain, n, d_native, d_len)),
        "frame": (frame, lambda: frame.compress_frame_async(d_plain, n, d_frame, d_len)),
    }
    sizes = {}
    for name, (ctx, fn) in calls.items():
        for _ in range(3):
            fn()
        sizes[name] = ctx.async_length(d_len)
        ctx.set_timing(True)
    samples = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, (ctx, fn) in calls.items():
            fn()
            samples[name].append(ctx.last_timing())
    per_gib = (1 << 30) / n
    out = {"mib": args.mib, "reps": args.reps, "native_bytes": sizes["native"],
           "frame_bytes": sizes["frame"], "frame_over_native_bytes": sizes["frame"] / sizes["native"]}
    for name, v in samples.items():
        call = [a * per_gib for a, _ in v]
        rest = [(a - b) * per_gib for a, b in v]
        out[name + "_ms_per_gib"] = (statistics.median(call), min(call), max(call))
        out[name + "_after_tiles_ms_per_gib"] = (statistics.median(rest), min(rest), max(rest))
        c, r = out[name + "_ms_per_gib"], out[name + "_after_tiles_ms_per_gib"]
        print(f"{name:6s}: {c[0]:.4f} ms/GiB ({c[1]:.4f} .. {c[2]:.4f}), of which the three "
              f"launches after lz4_tiles {r[0]:.4f} ({r[1]:.4f} .. {r[2]:.4f})")
    out["frame_over_native_ms"] = out["frame_ms_per_gib"][0] / out["native_ms_per_gib"][0]
    print(f"sizes: native {sizes['native']} B ({sizes['native'] / n:.4f} B/B), frame "
          f"{sizes['frame']} B ({sizes['frame'] / n:.4f} B/B), frame / native "
          f"{out['frame_over_native_bytes']:.4f}; time frame / native "
          f"{out['frame_over_native_ms']:.4f}")
    if args.verify:
        back = lz4.decompress_frame(d_frame[:sizes["frame"]].cpu().numpy().tobytes(), cap=n)
        assert back == d_plain.cpu().numpy().tobytes(), "the frame does not decode to the text"
        out["verified"] = True
    print(json.dumps(out))
    native.close()
    frame.close()


if __name__ == "__main__":
    main()
