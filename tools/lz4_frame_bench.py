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
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lz4-jpeg_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()

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
