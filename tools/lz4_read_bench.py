#!/usr/bin/env python3
"""Time lz4r_read_device (batched random-access reads from a compressed
stream) on an MI355X, each batch beside what a caller had to do for the same
bytes without it: lz4r_decompress_device of the whole stream plus a torch
gather.

    python tools/lz4_read_bench.py [--mib 64] [--reps 15] [--seed 1]

Corpus: --mib MiB of text (synth.random_passages_device), compressed on the
GPU; the offsets are the compressor's own device array.  Batches: uniform
random reads (fixed seed) of 64 B, 300 B, 4 KiB and 64 KiB, as many as
deliver 1 MiB and 64 MiB, packed back to back.  Then one read of the whole
stream beside lz4r_decompress_device.

Timing: device events around `inner` back-to-back calls (as many as fill
about 5 ms, from a first estimate), after a warm-up of every shape; --reps
such samples per path, the two paths alternated; the median and the spread
(min .. max) of the samples are printed.  The read path is the C ABI call
(both of its launches) on a reads array built beforehand.  The baseline is
decompress_device(check=False) into a buffer kept across calls plus
d_full.unfold(0, L, 1).index_select(0, d_src), the cheapest gather torch
offers for equal-length ranges (no index tensor per byte); the decode alone
is printed too.  Every batch's bytes are compared between the two paths once,
outside the timed window.  One JSON line per batch.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lz4-jpeg_amd"))

SIZES = (64, 300, 4096, 65536)
DELIVER = (1 << 20, 64 << 20)


def timed(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(paths, reps):
    """paths: {name: fn}.  Warm-up, an estimate, then reps samples of each
    path in turn -> {name: (median, min, max) ms per call}."""
    inner = {}
    for name, fn in paths.items():
        for _ in range(3):
            fn()
        est = max(timed(fn, 2), 1e-3)
        inner[name] = max(1, min(200, int(5.0 / est + 0.5)))
    samples = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            samples[name].append(timed(fn, inner[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch
    from lz4jpeg import _lib, lz4, synth
    assert torch.cuda.is_available(), "lz4_read_bench.py needs a GPU"
    L = _lib.lib()
    n = args.mib << 20
    d_plain = torch.empty(n, dtype=torch.uint8, device="cuda")
    synth.random_passages_device(d_plain, n, seed=args.seed)
    comp = lz4.Compressor()
    d_stream, length = comp.compress_device(d_plain)
    offs, nb = comp.block_offsets_device()
    torch.cuda.synchronize()
    print(f"# corpus {args.mib} MiB text -> {length} B stream ({length / n:.4f} B/B), "
          f"{nb} blocks; {args.reps} samples per path, median (min .. max)")

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_res = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_full = torch.empty(n + 300, dtype=torch.uint8, device="cuda")

    def decode():
        lz4.decompress_device(d_stream, length, offs, nb, n + 300, d_out=d_full, check=False)

    def read_call(d_reads, nreads, max_len, d_out):
        rc = L.lz4r_read_device(ctypes.c_void_p(d_stream.data_ptr()), length, ctypes.c_void_p(offs),
                                nb, ctypes.c_void_p(d_reads.data_ptr()), nreads, max_len,
                                ctypes.c_void_p(d_out.data_ptr()), d_out.numel(),
                                ctypes.c_void_p(d_res.data_ptr()), stream)
        assert rc == 0, rc

    gen = torch.Generator().manual_seed(args.seed)
    for size in SIZES:
        for deliver in DELIVER:
            nreads = deliver // size
            d_src = torch.randint(0, n - size + 1, (nreads,), generator=gen).cuda()
            d_len = torch.full((nreads,), size, dtype=torch.int64, device="cuda")
            d_dst = torch.arange(nreads, dtype=torch.int64, device="cuda") * size
            d_reads = torch.stack((d_src, d_len, d_dst), dim=1).contiguous()
            d_out = torch.empty(nreads * size, dtype=torch.uint8, device="cuda")

            def read():
                read_call(d_reads, nreads, size, d_out)

            def baseline():
                decode()
                return d_full.unfold(0, size, 1).index_select(0, d_src)

            read()
            want = baseline().reshape(-1)
            torch.cuda.synchronize()
            res = [int(x) for x in d_res.cpu().tolist()]
            assert res == [nreads * size, -1], res
            assert torch.equal(d_out, want), "read != decode + gather"
            del want
            t = measure({"read": read, "decode+gather": baseline, "decode": decode}, args.reps)
            r, b, d = t["read"], t["decode+gather"], t["decode"]
            print(f"{size:6d} B x {nreads:8d} = {deliver >> 20:3d} MiB: read {r[0]:8.4f} ms "
                  f"({r[1]:.4f} .. {r[2]:.4f}), {nreads / r[0] / 1e3:9.2f} M reads/s, "
                  f"{deliver / r[0] / 1e6:8.2f} GB/s | decode+gather {b[0]:8.4f} ms "
                  f"({b[1]:.4f} .. {b[2]:.4f}), of which decode {d[0]:.4f} | "
                  f"read / baseline {r[0] / b[0]:.3f}")
            print(json.dumps({"size": size, "reads": nreads, "delivered": deliver,
                              "read_ms": r, "baseline_ms": b, "decode_ms": d,
                              "reads_per_s": nreads / r[0] * 1e3,
                              "delivered_gb_s": deliver / r[0] / 1e6,
                              "read_over_baseline": r[0] / b[0]}))

    # the whole stream as one read, beside the block decoder
    d_reads = torch.tensor([[0, n, 0]], dtype=torch.int64, device="cuda")
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")

    def whole():
        read_call(d_reads, 1, n, d_out)

    whole()
    torch.cuda.synchronize()
    assert [int(x) for x in d_res.cpu().tolist()] == [n, -1] and torch.equal(d_out, d_plain)
    t = measure({"read": whole, "decode": decode}, args.reps)
    r, d = t["read"], t["decode"]
    print(f"whole stream ({args.mib} MiB) as one read: {r[0]:.4f} ms ({r[1]:.4f} .. {r[2]:.4f}), "
          f"{n / r[0] / 1e6:.1f} GB/s | lz4r_decompress_device {d[0]:.4f} ms "
          f"({d[1]:.4f} .. {d[2]:.4f}) | ratio {r[0] / d[0]:.3f}")
    print(json.dumps({"whole_stream_mib": args.mib, "read_ms": r, "decode_ms": d,
                      "read_over_decode": r[0] / d[0]}))
    comp.close()


if __name__ == "__main__":
    main()
