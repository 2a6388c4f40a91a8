#!/usr/bin/env python3
"""Time the JPR stream stage (jpegr_pack_device / jpegr_unpack_device) and
jpeg.compress_device on an MI355X; bench.py's discipline: a clock pre-warm,
settle() on each measured call, then event-timed means over back-to-back
launches.

    python tools/jpeg_pack_bench.py [--steps K] [--once N]
                                    [--decode | --tight [--against LIB] | --direct [--against LIB]
                                     | --crop [--against LIB] | --thumb [--against LIB]
                                     | --select [--against LIB] | --tensor [--against LIB]
                                     | --resize | --dataset]

Images: bench.py's 3840x2160 random image (synth.rand_rgba_device, seed 1)
and a 3840x2160 smooth one (tests/test_gpu_entropy.py's generator).  Prints
one JSON line per image: ms per image of pack and unpack (beside the entropy
stage's encode / decode, measured in the same run), the stream's bytes per
tile and its ratio to the tile's 256 B of RGBA, and the algorithmic bytes of
each call (live slot bytes read + stream bytes written, and the reverse) with
the rate they imply.  --once N: N pack + unpack launches per image and
nothing else, for a profiler's counter passes.

--decode: the decode side only, for profiles/jpr_stream_decode.log: the direct
decode of the stream (jpegr_stream_decode_device) against the two stages it
replaces, unpack + entropy decode, all in this run after the same pre-warm
and settle, alternated over --rounds rounds so that the spread between
repeats of the same call is known before a difference is read; then one image
of an 8-image stream (the random image eight times) against the two stages
over the whole of that stream, which is the only way to that image without
the direct decode; and the device bytes a 4K decode needs either way.  With
--once N: N direct decodes per image and nothing else.

--tight: the JPT1 stream beside JPR1, for profiles/jpt_pack_bench.log: both
packs and the direct decode of each stream, alternated over --rounds rounds in
this run after the same pre-warm and settle; both streams' lengths and bytes
per tile; every output checked (the tight stream decodes to the coefficients
the entropy stage was given).  --against LIB adds the same calls -- both packs,
unpack, both direct decodes -- of a second build of the library (the parent
commit's, loaded beside the product's with RTLD_LOCAL) to the same rounds, and
prints each pair with the ratio of the medians.  With --once N: N launches of
the two packs and the two direct decodes per image and nothing else.

--direct: the encode straight to a stream (jpegr_stream_encode_device), both
formats, for profiles/jpr_stream_encode.log: beside entropy encode + pack and
entropy encode + tight pack, the stages it replaces, alternated over --rounds
rounds in this run after the same pre-warm and settle; every output checked
against the two-stage stream.  --against LIB adds the second build's entropy
encode / decode, both packs, both direct encodes and the direct decode to the
same rounds, with the ratio of the medians per pair.  Then the device memory
compress_device peaks at, direct or not, for one image and for eight.  With
--once N: N direct encodes of each format per image and nothing else.

--crop: random access (jpegr_stream_index_device + jpegr_crop_device), for
profiles/jpr_crop_bench.md: a stream of 16 images of 1920x1080, random and
smooth, JPR1 and JPT1, and 256 uniformly random 224x224 crops of it through
crop_device with the index built once outside the timed call, and with the
index call inside it; beside them what there was before: the direct decode and
reconstruction of all 16 images followed by a torch gather of the same
rectangles.  Then one rectangle per image covering the whole image against
decode + reconstruct of the same images: the price of the crop mapping where
it has nothing to save.  All in this run after the same pre-warm and settle,
alternated over --rounds rounds, event-timed; the crops' bytes are checked
against the gather's.  --against LIB times the index call and both crop calls of
this build and of a second build of the library in the same rounds, both by the
same bare C calls, outputs compared, and prints each pair's ratio of the medians.  With --once N: N crop calls per stream and
nothing else.

--thumb: 1/8-scale thumbnails from the DC terms alone (jpegr_thumb_device), for
profiles/jpr_thumb_bench.md: --crop's streams (16 images of 1920x1080, random
and smooth, JPR1 and JPT1) and four paths to the 16 thumbnails of 240x135:
thumb_device with the offsets kept (the index built once outside the timed
call), thumb_device scanning the index itself, the index call alone, and what a
caller had to do before: the direct decode and reconstruction of all 16 images
followed by torch.nn.functional.avg_pool2d(.., 8).  That baseline's pixels are
not the thumbnail's -- a mean of 64 rounded samples, AC terms included, against
the one sample of the DC-only tile -- so only the thumbnail paths' bytes are
checked, against each other and against every eighth pixel of the
reconstruction of the DC-only coefficients.  Reports each path's stream bytes
per ms and its ratio to the baseline.  --against LIB times the two thumbnail
calls of this build and of a second build (the whole library, or jpegr_thumb.hip
alone: make thumb-alt, the other form of the record read) in the same rounds,
both by the same bare C call.  All in this run after the same
pre-warm and settle, alternated over --rounds rounds, event-timed.  With
--once N: N thumbnail calls (offsets kept) per stream and nothing else.

--select: editing a stream without decoding it (jpegr_select_device), for
profiles/jpr_select_bench.md: --crop's streams and three edits of each -- 8 of
the 16 images in a shuffled order, 256 tile-aligned 224x224 windows, and the
whole stream in the other format (the first two with the source's format named
and, as sub0 / win0, with format 0) -- each beside what a caller had to do before
(decode_stream_device of the images' tile ranges and encode_stream_device; the
whole stream decoded, the windows' tiles gathered by torch and encoded; unpack +
tight pack for JPR1 -> JPT1, decode + encode for JPT1 -> JPR1) and beside a
device-to-device copy of as many bytes as the call writes.  Every output is
checked against the baseline's bytes.  The index is built once outside the timed
calls.  All in this run after the same pre-warm and settle, alternated over
--rounds rounds, event-timed.  --against LIB times the five select calls of this
build and of a second build of the library in the same rounds, both by the same
bare C call, outputs compared, and prints each pair's ratio of the medians.  With --once N: N select calls of each kind
per stream and nothing else.

--tensor: crops delivered as normalised tensors (jpegr_crop_tensor_device), for
profiles/jpr_tensor_bench.md: --crop's streams and rectangles, the index built
once outside the timed calls.  The fused call as float32 CHW and as bfloat16
CHW, ImageNet's normalisation, every second crop mirrored; beside each, in the
same rounds, crop_device followed by the torch chain it replaces (slice off the
alpha, permute, float, mul, add, to(bfloat16), where / flip); and crop_device
alone.  The fused outputs are compared bitwise with the chain's before anything
is timed.  --against LIB times crop_device of this build and of a second build
in the same rounds, both by the same bare C call, outputs compared.  All after
the same pre-warm and settle, alternated over --rounds rounds, event-timed.
With --once N: N fused calls of each dtype per stream and nothing else.

--resize: crops resampled to one size (jpegr_crop_resize_device), for
profiles/jpr_resize_bench.md: --tensor's streams; 256 rectangles drawn as
RandomResizedCrop draws them (area 8 to 100 % of the image, aspect 3/4 to 4/3,
seeded), each to 224 x 224, ImageNet's normalisation, every second one mirrored.
The fused call as float32 and as bfloat16 CHW with the TRIANGLE filter; beside
it, in the same rounds, (a) the chain it replaces: one crops_tensor call with
float32 CHW packed crops, then per crop interpolate(antialias=True) into the
batch, the flip, and to(bfloat16); and (b) crop_tensor_device of the same
rectangles alone, with no resampling, as the floor.  The fused float32 output
is compared with the chain's before anything is timed: they are not bit-equal
by design (include/jpegr.h), so the largest |difference| is reported.  With
--once N: N fused calls of each dtype per stream and nothing else.

--dataset: crops from many streams in one call
(jpegr_dataset_crop_resize_device), for DESIGN 4.18: 256 streams of different
sizes (320 .. 546 by 240 .. 420, two random images each, JPR1 and JPT1
alternating); 256 RandomResizedCrop rectangles to 224 x 224 float32 CHW, every
second one mirrored, rectangle r from stream r % S, for S = 1, 16 and 256.  One
dataset call beside the S jpegr_crop_resize_device calls that write the same
tensor (each with its own rectangles, local image indices and the same dst),
both as bare C calls on prepared rectangles, outputs compared bitwise first,
then alternated over --rounds rounds, event-timed.  With --once N: N dataset
calls per S and nothing else."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lz4-jpeg_amd"))

W, H = 3840, 2160


def settle(fn, sync, ms=60.0, chunk=8):
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < ms / 1e3:
        for _ in range(chunk):
            fn()
        n += chunk
        sync()
    return n


def smooth_image(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.stack([(xx // 3) % 256, (yy // 2) % 256, ((xx + yy) // 5) % 256,
                                          np.full_like(xx, 255)], -1).astype(np.uint8))


def timed(fn, steps, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(xs[len(xs) // 2], 4), "max": round(xs[-1], 4)}


def second_build(path):
    """A second build of the library, loaded beside the product's."""
    import ctypes
    from lz4jpeg import _lib
    handle = ctypes.CDLL(os.path.abspath(path), mode=ctypes.RTLD_LOCAL)
    for fname, res, argt in _lib.SIGNATURES:
        if hasattr(handle, fname):
            fn = getattr(handle, fname)
            fn.restype, fn.argtypes = res, argt
    return handle


def checked(rc):
    assert rc == 0, rc


def over_against(res, keys):
    for key in keys:
        res[key + "_over_against"] = round(
            res[key + "_ms"]["median"] / res["against_" + key + "_ms"]["median"], 4)


def decode_side(args, torch, jpeg, name, img, d_coef, d_out, n, back, d_res, s2, unpack):
    """The direct decode beside unpack + entropy decode: same run, alternated."""
    dev = d_coef.device
    nt = jpeg.tiles(W, H)
    lib = jpeg._lib.lib()
    pack_scratch = int(lib.jpegr_pack_scratch_bytes(nt))
    d_direct = torch.empty_like(d_coef)
    d_res3 = torch.empty(3, dtype=torch.int64, device=dev)
    s3 = torch.empty(pack_scratch, dtype=torch.uint8, device=dev)
    d_coef2 = torch.empty_like(d_coef)

    def direct():
        jpeg.decode_stream_device(d_out, n, W, H, d_coef=d_direct, d_result=d_res3, scratch=s3)

    def entropy_decode():
        back.decode(d_coef2)

    def two_stages():
        unpack()
        entropy_decode()

    if args.once:
        for _ in range(args.once):
            direct()
        torch.cuda.synchronize()
        return
    two_stages()
    direct()
    torch.cuda.synchronize()
    ok = d_res.cpu().tolist() == [n, -1] and int(back.status[1].item()) == 0 \
        and bool(torch.equal(d_coef2, d_coef)) and d_res3.cpu().tolist() == [n, -1, 0] \
        and bool(torch.equal(d_direct, d_coef))
    res = {"image": f"{name} {W}x{H}", "tiles": nt, "stream_bytes": n, "outputs_equal": ok,
           "steps": args.steps, "rounds": args.rounds}
    calls = (("unpack", unpack), ("entropy_decode", entropy_decode), ("two_stages", two_stages),
             ("stream_decode", direct))
    ms = {k: [] for k, _ in calls}
    for _ in range(args.rounds):                     # alternated: each round times every call once
        for key, fn in calls:
            settle(fn, torch.cuda.synchronize, chunk=20)
            ms[key].append(timed(fn, args.steps, torch))
    for key, _ in calls:
        res[key + "_ms"] = spread(ms[key])
    res["stream_decode_over_two_stages"] = round(
        res["stream_decode_ms"]["median"] / res["two_stages_ms"]["median"], 3)
    # device memory a decode of this image needs beside the stream and the
    # coefficients: the slots, the decoder's status and unpack's result and
    # scratch -- or the direct decode's result and scratch
    common = n + 256 * nt
    res["device_bytes_two_stages"] = common + 1292 * nt + 16 + 16 + pack_scratch
    res["device_bytes_stream_decode"] = common + 24 + pack_scratch
    print(json.dumps(res), flush=True)
    if name != "random":
        return
    # one image of an 8-image stream
    k, pick = 8, 5
    img8 = img.repeat(k)
    ent8 = jpeg.Entropy(k * nt, device=dev)
    ent8.encode(jpeg.encode_device(img8, W, H, k))
    d_out8, d_len8 = jpeg.pack_device(ent8, W, H, k)
    n8 = int(d_len8.item())
    del img8
    res8 = torch.empty(3, dtype=torch.int64, device=dev)
    res8u = torch.zeros(2, dtype=torch.int64, device=dev)
    s8 = torch.empty(int(lib.jpegr_pack_scratch_bytes(k * nt)), dtype=torch.uint8, device=dev)
    s8u = torch.empty_like(s8)
    d_all = torch.empty(k * nt * 128, dtype=torch.int16, device=dev)

    def one_image():
        jpeg.decode_stream_device(d_out8, n8, W, H, k, pick * nt, nt, d_coef=d_direct, d_result=res8,
                                  scratch=s8)

    def all_direct():
        jpeg.decode_stream_device(d_out8, n8, W, H, k, d_coef=d_all, d_result=res8, scratch=s8)

    def all_two_stages():
        jpeg.unpack_device(d_out8, n8, W, H, k, ent=ent8, d_result=res8u, scratch=s8u)
        ent8.decode(d_all)

    one_image()
    torch.cuda.synchronize()
    ok8 = res8.cpu().tolist() == [n8, -1, 0] and bool(torch.equal(d_direct, d_coef))
    out = {"image": f"random {W}x{H} x {k}", "tiles": k * nt, "stream_bytes": n8, "image_decoded": pick,
           "outputs_equal": ok8, "steps": args.steps, "rounds": args.rounds}
    calls = (("one_image_stream_decode", one_image), ("all_images_stream_decode", all_direct),
             ("all_images_two_stages", all_two_stages))
    ms = {key: [] for key, _ in calls}
    for _ in range(args.rounds):
        for key, fn in calls:
            settle(fn, torch.cuda.synchronize, chunk=4)
            ms[key].append(timed(fn, max(1, args.steps // 4), torch))
    for key, _ in calls:
        out[key + "_ms"] = spread(ms[key])
    print(json.dumps(out), flush=True)


class Calls:
    """The stream calls of one build of the library on one image's slots, each
    with buffers of its own."""

    def __init__(self, lib, torch, ent, nt, d_coef):
        import ctypes
        from lz4jpeg import _lib, jpeg
        self.lib, self.ent, self.nt, self.c = lib, ent, nt, ctypes
        for fname, res, argt in _lib.SIGNATURES:
            if fname.startswith("jpegr_") and hasattr(lib, fname):
                fn = getattr(lib, fname)
                fn.restype, fn.argtypes = res, argt
        dev = d_coef.device
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nscr = int(lib.jpegr_pack_scratch_bytes(nt))
        self.scr = [torch.empty(nscr, dtype=torch.uint8, device=dev) for _ in range(5)]
        self.out = torch.empty(int(lib.jpegr_pack_bound(W, H, 1)), dtype=torch.uint8, device=dev)
        self.out_t = torch.empty_like(self.out)
        self.len = torch.zeros(1, dtype=torch.int64, device=dev)
        self.len_t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.back = jpeg.Entropy(nt, device=dev)
        self.res2 = torch.zeros(2, dtype=torch.int64, device=dev)
        self.res3 = torch.zeros(3, dtype=torch.int64, device=dev)
        self.res3_t = torch.zeros(3, dtype=torch.int64, device=dev)
        self.coef = torch.empty_like(d_coef)
        self.coef_t = torch.empty_like(d_coef)
        self.n = self.n_t = 0

    def _p(self, t):
        return self.c.c_void_p(t.data_ptr())

    def _pack(self, fn, out, d_len, scr):
        e = self.ent
        rc = fn(self._p(e.bits), self._p(e.meta), self._p(e.table), W, H, 1, self._p(out), out.numel(),
                self._p(d_len), self._p(scr), self.st)
        assert rc == 0, rc

    def _direct(self, src, n, coef, res, scr):
        rc = self.lib.jpegr_stream_decode_device(self._p(src), n, W, H, 1, 0, self.nt, self._p(coef),
                                                 self._p(scr), self._p(res), self.st)
        assert rc == 0, rc

    def pack(self):
        self._pack(self.lib.jpegr_pack_device, self.out, self.len, self.scr[0])

    def pack_tight(self):
        self._pack(self.lib.jpegr_pack_tight_device, self.out_t, self.len_t, self.scr[1])

    def unpack(self):
        b = self.back
        rc = self.lib.jpegr_unpack_device(self._p(self.out), self.n, W, H, 1, self._p(b.bits),
                                          self._p(b.meta), self._p(b.table), self._p(self.scr[2]),
                                          self._p(self.res2), self.st)
        assert rc == 0, rc

    def direct(self):
        self._direct(self.out, self.n, self.coef, self.res3, self.scr[3])

    def direct_tight(self):
        self._direct(self.out_t, self.n_t, self.coef_t, self.res3_t, self.scr[4])


def tight_side(args, torch, jpeg, name, ent, d_coef, other):
    """JPR1 and JPT1 pack and direct decode, and the JPR1 calls of `other`
    (a second build's ctypes handle, or None): same run, alternated."""
    nt = jpeg.tiles(W, H)
    prod = Calls(jpeg._lib.lib(), torch, ent, nt, d_coef)
    prod.pack()
    prod.pack_tight()
    prod.n, prod.n_t = int(prod.len.item()), int(prod.len_t.item())
    prod.unpack()
    prod.direct()
    prod.direct_tight()
    torch.cuda.synchronize()
    if args.once:
        for _ in range(args.once):
            prod.pack()
            prod.pack_tight()
            prod.direct()
            prod.direct_tight()
        torch.cuda.synchronize()
        return
    ok = prod.res3.cpu().tolist() == [prod.n, -1, 0] and prod.res3_t.cpu().tolist() == [prod.n_t, -1, 0] \
        and bool(torch.equal(prod.coef, d_coef)) and bool(torch.equal(prod.coef_t, d_coef)) \
        and prod.res2.cpu().tolist() == [prod.n, -1] \
        and jpeg.stream_format(prod.out_t[:16].cpu().numpy().tobytes()) == (W, H, 1, True)
    res = {"image": f"{name} {W}x{H}", "tiles": nt, "jpr1_bytes": prod.n, "jpt1_bytes": prod.n_t,
           "jpr1_bytes_per_tile": round(prod.n / nt, 2), "jpt1_bytes_per_tile": round(prod.n_t / nt, 2),
           "jpt1_over_jpr1": round(prod.n_t / prod.n, 4), "outputs_equal": ok, "steps": args.steps,
           "rounds": args.rounds}
    calls = [("pack", prod.pack), ("pack_tight", prod.pack_tight), ("unpack", prod.unpack),
             ("stream_decode", prod.direct), ("stream_decode_tight", prod.direct_tight)]
    if other is not None:
        par = Calls(other, torch, ent, nt, d_coef)
        par.pack()
        par.pack_tight()
        par.n, par.n_t = int(par.len.item()), int(par.len_t.item())
        par.unpack()
        par.direct()
        par.direct_tight()
        torch.cuda.synchronize()
        res["against_outputs_equal"] = par.n == prod.n and bool(torch.equal(par.out[:par.n], prod.out[:prod.n])) \
            and par.n_t == prod.n_t and bool(torch.equal(par.out_t[:par.n_t], prod.out_t[:prod.n_t])) \
            and bool(torch.equal(par.coef, prod.coef)) and par.res3.cpu().tolist() == prod.res3.cpu().tolist() \
            and bool(torch.equal(par.coef_t, prod.coef_t)) and par.res3_t.cpu().tolist() == prod.res3_t.cpu().tolist() \
            and all(bool(torch.equal(getattr(par.back, f), getattr(prod.back, f))) for f in ("bits", "meta", "table"))
        calls += [("against_pack", par.pack), ("against_pack_tight", par.pack_tight),
                  ("against_unpack", par.unpack), ("against_stream_decode", par.direct),
                  ("against_stream_decode_tight", par.direct_tight)]
    ms = {k: [] for k, _ in calls}
    for r in range(args.rounds):                      # alternated; the order turns with the round
        for key, fn in calls[r % len(calls):] + calls[:r % len(calls)]:
            settle(fn, torch.cuda.synchronize, chunk=20)
            ms[key].append(timed(fn, args.steps, torch))
    for key, _ in calls:
        res[key + "_ms"] = spread(ms[key])
    if other is not None:
        for key in ("pack", "pack_tight", "unpack", "stream_decode", "stream_decode_tight"):
            res[key + "_over_against"] = round(
                res[key + "_ms"]["median"] / res["against_" + key + "_ms"]["median"], 4)
    print(json.dumps(res), flush=True)


class EncCalls:
    """The encode-side calls of one build of the library on one image's
    coefficients, each with buffers of its own."""

    def __init__(self, lib, torch, nt, d_coef, jpeg):
        import ctypes
        from lz4jpeg import _lib
        self.lib, self.nt, self.c, self.d_coef = lib, nt, ctypes, d_coef
        for fname, res, argt in _lib.SIGNATURES:
            if fname.startswith("jpegr_") and hasattr(lib, fname):
                fn = getattr(lib, fname)
                fn.restype, fn.argtypes = res, argt
        dev = d_coef.device
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ent = jpeg.Entropy(nt, device=dev)
        bound = int(lib.jpegr_pack_bound(W, H, 1))
        nscr = int(lib.jpegr_pack_scratch_bytes(nt))
        self.out = {k: torch.empty(bound, dtype=torch.uint8, device=dev) for k in ("r", "t", "dr", "dt")}
        self.len = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in ("r", "t", "dr", "dt")}
        self.scr = {k: torch.empty(nscr, dtype=torch.uint8, device=dev) for k in ("r", "t", "dec")}
        self.res3 = torch.zeros(3, dtype=torch.int64, device=dev)
        self.coef = torch.empty_like(d_coef)
        self.coef2 = torch.empty_like(d_coef)
        self.n = 0
        if hasattr(lib, "jpegr_stream_encode_device"):
            self.enc_scratch_bytes = int(lib.jpegr_stream_encode_scratch_bytes(nt, bound))
            self.escr = {k: torch.empty(self.enc_scratch_bytes, dtype=torch.uint8, device=dev)
                         for k in ("dr", "dt")}
            self.eres = {k: torch.zeros(2, dtype=torch.int64, device=dev) for k in ("dr", "dt")}

    def _p(self, t):
        return self.c.c_void_p(t.data_ptr())

    def entropy_encode(self):
        e = self.ent
        rc = self.lib.jpegr_entropy_encode_device(self._p(self.d_coef), self.nt, self._p(e.bits),
                                                  self._p(e.meta), self._p(e.table), self._p(e.scratch),
                                                  self._p(e.status), self.st)
        assert rc == 0, rc

    def entropy_decode(self):
        e = self.ent
        rc = self.lib.jpegr_entropy_decode_device(self._p(e.bits), self._p(e.meta), self._p(e.table),
                                                  self.nt, self._p(self.coef2), self._p(e.status), self.st)
        assert rc == 0, rc

    def _pack(self, fn, k):
        e = self.ent
        rc = fn(self._p(e.bits), self._p(e.meta), self._p(e.table), W, H, 1, self._p(self.out[k]),
                self.out[k].numel(), self._p(self.len[k]), self._p(self.scr[k]), self.st)
        assert rc == 0, rc

    def pack(self):
        self._pack(self.lib.jpegr_pack_device, "r")

    def pack_tight(self):
        self._pack(self.lib.jpegr_pack_tight_device, "t")

    def two_stage(self):
        self.entropy_encode()
        self.pack()

    def two_stage_tight(self):
        self.entropy_encode()
        self.pack_tight()

    def _direct(self, k, fmt):
        rc = self.lib.jpegr_stream_encode_device(self._p(self.d_coef), W, H, 1, fmt, self._p(self.out[k]),
                                                 self.out[k].numel(), self._p(self.len[k]),
                                                 self._p(self.escr[k]), self._p(self.eres[k]), self.st)
        assert rc == 0, rc

    def direct(self):
        self._direct("dr", 1)

    def direct_tight(self):
        self._direct("dt", 2)

    def stream_decode(self):
        rc = self.lib.jpegr_stream_decode_device(self._p(self.out["r"]), self.n, W, H, 1, 0, self.nt,
                                                 self._p(self.coef), self._p(self.scr["dec"]),
                                                 self._p(self.res3), self.st)
        assert rc == 0, rc


def peak_bytes(torch, fn):
    """Device bytes fn allocates at its peak, over what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def direct_side(args, torch, jpeg, name, img, d_coef, other):
    """The direct encode, both formats, beside entropy encode + pack / tight
    pack, and the existing calls of `other` (a second build's ctypes handle, or
    None) beside this build's: same run, alternated."""
    nt = jpeg.tiles(W, H)
    prod = EncCalls(jpeg._lib.lib(), torch, nt, d_coef, jpeg)
    prod.two_stage()
    prod.pack_tight()
    prod.direct()
    prod.direct_tight()
    torch.cuda.synchronize()
    if args.once:
        for _ in range(args.once):
            prod.direct()
            prod.direct_tight()
        torch.cuda.synchronize()
        return
    n = {k: int(v.item()) for k, v in prod.len.items()}
    prod.n = n["r"]
    prod.stream_decode()
    prod.entropy_decode()
    torch.cuda.synchronize()
    ok = n["dr"] == n["r"] and n["dt"] == n["t"] \
        and bool(torch.equal(prod.out["dr"][:n["r"]], prod.out["r"][:n["r"]])) \
        and bool(torch.equal(prod.out["dt"][:n["t"]], prod.out["t"][:n["t"]])) \
        and prod.eres["dr"].cpu().tolist() == [n["r"], 0] and prod.eres["dt"].cpu().tolist() == [n["t"], 0] \
        and bool(torch.equal(prod.coef, d_coef)) and bool(torch.equal(prod.coef2, d_coef))
    res = {"image": f"{name} {W}x{H}", "tiles": nt, "jpr1_bytes": n["r"], "jpt1_bytes": n["t"],
           "outputs_equal": ok, "steps": args.steps, "rounds": args.rounds,
           "slot_bytes": 1292 * nt, "stream_encode_scratch_bytes_at_bound": prod.enc_scratch_bytes,
           "stream_encode_scratch_bytes_at_stream": int(
               prod.lib.jpegr_stream_encode_scratch_bytes(nt, n["r"]))}
    calls = [("entropy_encode", prod.entropy_encode), ("pack", prod.pack), ("pack_tight", prod.pack_tight),
             ("two_stage", prod.two_stage), ("two_stage_tight", prod.two_stage_tight),
             ("stream_encode", prod.direct), ("stream_encode_tight", prod.direct_tight),
             ("entropy_decode", prod.entropy_decode), ("stream_decode", prod.stream_decode)]
    shared = ("entropy_encode", "pack", "pack_tight", "entropy_decode", "stream_decode",
              "stream_encode", "stream_encode_tight")
    if other is not None:
        par = EncCalls(other, torch, nt, d_coef, jpeg)
        par.stream_encode, par.stream_encode_tight = par.direct, par.direct_tight
        par.two_stage()
        par.pack_tight()
        par.direct()
        par.direct_tight()
        torch.cuda.synchronize()
        par.n = int(par.len["r"].item())
        par.stream_decode()
        par.entropy_decode()
        torch.cuda.synchronize()
        res["against_outputs_equal"] = par.n == n["r"] and int(par.len["t"].item()) == n["t"] \
            and bool(torch.equal(par.out["r"][:par.n], prod.out["r"][:par.n])) \
            and bool(torch.equal(par.out["t"][:n["t"]], prod.out["t"][:n["t"]])) \
            and bool(torch.equal(par.out["dr"][:par.n], prod.out["r"][:par.n])) \
            and bool(torch.equal(par.out["dt"][:n["t"]], prod.out["t"][:n["t"]])) \
            and bool(torch.equal(par.coef, d_coef)) and bool(torch.equal(par.coef2, d_coef))
        calls += [("against_" + k, getattr(par, k)) for k in shared]
    ms = {k: [] for k, _ in calls}
    for r in range(args.rounds):                      # alternated; the order turns with the round
        for key, fn in calls[r % len(calls):] + calls[:r % len(calls)]:
            settle(fn, torch.cuda.synchronize, chunk=20)
            ms[key].append(timed(fn, args.steps, torch))
    for key, _ in calls:
        res[key + "_ms"] = spread(ms[key])
    med = lambda k: res[k + "_ms"]["median"]
    res["stream_encode_over_two_stage"] = round(med("stream_encode") / med("two_stage"), 4)
    res["stream_encode_tight_over_two_stage_tight"] = round(
        med("stream_encode_tight") / med("two_stage_tight"), 4)
    if other is not None:
        for key in shared:
            res[key + "_over_against"] = round(med(key) / med("against_" + key), 4)
    print(json.dumps(res), flush=True)
    if name != "random":
        return
    mem = {"image": f"random {W}x{H}", "what": "peak device bytes of compress_device over its input"}
    for k in (1, 8):
        imgs = img.repeat(k)
        for tight in (False, True):
            for direct in (False, True):
                key = f"x{k}_{'jpt1' if tight else 'jpr1'}_{'direct' if direct else 'slots'}"
                mem[key] = peak_bytes(
                    torch, lambda: jpeg.compress_device(imgs, W, H, k, tight=tight, direct=direct))
        del imgs
    print(json.dumps(mem), flush=True)


CW, CH, CN = 1920, 1080, 16                  # --crop: the stream's images
CROP, NCROPS = 224, 256


def crop_side(args, torch, jpeg, synth, dev, other):
    """Crops straight from the stream beside decode-everything-and-gather."""
    nt = CN * jpeg.tiles(CW, CH)
    px = CW * CH
    rng = np.random.default_rng(7)
    im = rng.integers(0, CN, NCROPS)
    x = rng.integers(0, CW - CROP + 1, NCROPS)
    y = rng.integers(0, CH - CROP + 1, NCROPS)
    touched = int((((x + CROP - 1) // 8 - x // 8 + 1) * ((y + CROP - 1) // 8 - y // 8 + 1)).sum())
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(dev)
    full_w, full_h = t64(np.full(NCROPS, CROP)), t64(np.full(NCROPS, CROP))
    cols = [t64(im), t64(x), t64(y), full_w, full_h]
    d_dst = t64(np.arange(NCROPS) * 4 * CROP * CROP)
    cap = NCROPS * 4 * CROP * CROP
    # the gather's pixel numbers: crop r's row j, column i
    jj, ii = np.mgrid[0:CROP, 0:CROP]
    d_idx = t64(((im * px + y * CW + x)[:, None, None] + jj[None] * CW + ii[None]).reshape(-1))
    whole = [t64(np.arange(CN)), t64(np.zeros(CN)), t64(np.zeros(CN)), t64(np.full(CN, CW)),
             t64(np.full(CN, CH))]
    d_wdst = t64(np.arange(CN) * 4 * px)
    images = {}
    d_img = torch.empty(CN * px * 4, dtype=torch.uint8, device=dev)
    synth.rand_rgba_device(d_img, 0, CN * px, seed=1)
    images["random"] = d_img
    images["smooth"] = torch.from_numpy(smooth_image(CW, CH)).to(dev).reshape(-1).repeat(CN)
    d_offs = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    d_ires = torch.empty(2, dtype=torch.int64, device=dev)
    d_res, d_wres = (torch.empty(3, dtype=torch.int64, device=dev) for _ in range(2))
    d_res3 = torch.empty(3, dtype=torch.int64, device=dev)
    iscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device=dev)
    cscr_bytes = jpeg.crop_scratch_bytes(NCROPS, CROP, CROP)
    wscr_bytes = jpeg.crop_scratch_bytes(CN, CW, CH)
    cscr = torch.empty(max(cscr_bytes, wscr_bytes), dtype=torch.uint8, device=dev)
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_wout = torch.empty(CN * px * 4, dtype=torch.uint8, device=dev)
    d_coef = torch.empty(nt * 128, dtype=torch.int16, device=dev)
    for name, img in images.items():
        for tight in (False, True):
            d_stream = jpeg.compress_device(img, CW, CH, CN, tight=tight)
            n = d_stream.numel()

            def index():
                jpeg.stream_index_device(d_stream, n, CW, CH, CN, d_offsets=d_offs, d_result=d_ires,
                                         scratch=iscr)

            def crops():
                jpeg.crop_device(d_stream, n, CW, CH, CN, d_offs, *cols, CROP, CROP, d_dst=d_dst,
                                 d_out=d_out, out_cap=cap, scratch=cscr, d_result=d_res, check=False)

            def index_and_crops():
                index()
                crops()

            def decode_all():
                jpeg.decode_stream_device(d_stream, n, CW, CH, CN, d_coef=d_coef, d_result=d_res3,
                                          scratch=iscr)
                return jpeg.reconstruct_device(d_coef, CW, CH, CN)

            def decode_all_and_gather():
                return decode_all().view(torch.int32)[d_idx]

            def whole_crops():
                jpeg.crop_device(d_stream, n, CW, CH, CN, d_offs, *whole, CW, CH, d_dst=d_wdst,
                                 d_out=d_wout, out_cap=d_wout.numel(), scratch=cscr, d_result=d_wres,
                                 check=False)

            index()
            if args.once:
                for _ in range(args.once):
                    crops()
                torch.cuda.synchronize()
                continue
            crops()
            got = d_out.clone()
            want = decode_all_and_gather()
            whole_crops()
            torch.cuda.synchronize()
            ok = bool(torch.equal(got.view(torch.int32), want)) \
                and bool(torch.equal(d_wout, decode_all())) \
                and d_ires.cpu().tolist() == [n, -1] and d_res.cpu().tolist() == [NCROPS, -1, 0] \
                and d_wres.cpu().tolist() == [CN, -1, 0] and d_res3.cpu().tolist() == [n, -1, 0]
            del got, want
            res = {"stream": f"{name} {CN} x {CW}x{CH} {'JPT1' if tight else 'JPR1'}", "tiles": nt,
                   "stream_bytes": n, "crops": f"{NCROPS} of {CROP}x{CROP}", "tiles_touched": touched,
                   "touched_fraction": round(touched / nt, 4), "outputs_equal": ok,
                   "steps": args.steps, "rounds": args.rounds,
                   "crop_items": jpeg.crop_items(CROP, CROP), "crop_scratch_bytes": cscr_bytes,
                   "whole_items": jpeg.crop_items(CW, CH), "whole_scratch_bytes": wscr_bytes,
                   "decode_all_coef_bytes": nt * 256, "decode_all_rgba_bytes": CN * px * 4}
            calls = [("index", index), ("crops", crops), ("index_and_crops", index_and_crops),
                     ("decode_all_and_gather", decode_all_and_gather), ("whole_crops", whole_crops),
                     ("decode_all", decode_all)]
            paired = ("index", "crops", "whole_crops")
            if other is not None:         # the three calls of either build by the same bare C calls
                import ctypes
                vp = lambda t: ctypes.c_void_p(t.data_ptr())
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                a_offs, a_ires, a_out, a_wout = (torch.empty_like(t) for t in (d_offs, d_ires, d_out, d_wout))
                a_res, a_wres = torch.empty_like(d_res), torch.empty_like(d_wres)
                rects = torch.stack((*cols, d_dst), dim=1).contiguous()
                wrects = torch.stack((*whole, d_wdst), dim=1).contiguous()

                def index_on(lib, offs, ires):
                    checked(lib.jpegr_stream_index_device(vp(d_stream), n, CW, CH, CN, vp(offs), vp(iscr),
                                                          vp(ires), st))

                def crops_on(lib, r, mw, mh, out, res):
                    checked(lib.jpegr_crop_device(vp(d_stream), n, CW, CH, CN, vp(d_offs), vp(r), r.shape[0],
                                                  mw, mh, vp(out), out.numel(), vp(cscr), vp(res), st))

                def three(lib, offs, ires, out, res, wout, wres):
                    return {"index": lambda: index_on(lib, offs, ires),
                            "crops": lambda: crops_on(lib, rects, CROP, CROP, out, res),
                            "whole_crops": lambda: crops_on(lib, wrects, CW, CH, wout, wres)}

                mine = three(jpeg._lib.lib(), d_offs, d_ires, d_out, d_res, d_wout, d_wres)
                theirs = three(other, a_offs, a_ires, a_out, a_res, a_wout, a_wres)
                calls = [(k, mine.get(k, fn)) for k, fn in calls]
                calls += [("against_" + k, theirs[k]) for k in paired]
                for k in paired:
                    mine[k]()
                    theirs[k]()
                torch.cuda.synchronize()
                res["against_outputs_equal"] = all(
                    bool(torch.equal(a, b)) for a, b in ((a_offs, d_offs), (a_ires, d_ires), (a_out, d_out),
                                                         (a_wout, d_wout), (a_res, d_res), (a_wres, d_wres)))
            ms = {k: [] for k, _ in calls}
            for r in range(args.rounds):                  # alternated; the order turns with the round
                for key, fn in calls[r % len(calls):] + calls[:r % len(calls)]:
                    settle(fn, torch.cuda.synchronize, chunk=4)
                    ms[key].append(timed(fn, args.steps, torch))
            for key, _ in calls:
                res[key + "_ms"] = spread(ms[key])
            if other is not None:
                over_against(res, paired)
            med = lambda k: res[k + "_ms"]["median"]
            res["crops_over_decode_all_and_gather"] = round(med("crops") / med("decode_all_and_gather"), 4)
            res["index_and_crops_over_decode_all_and_gather"] = round(
                med("index_and_crops") / med("decode_all_and_gather"), 4)
            res["whole_crops_over_decode_all"] = round(med("whole_crops") / med("decode_all"), 4)
            print(json.dumps(res), flush=True)
            del d_stream


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def tensor_side(args, torch, jpeg, synth, dev, other):
    """Crops delivered as normalised tensors (jpegr_crop_tensor_device) beside
    crop_device followed by the torch chain it replaces, and crop_device alone."""
    nt = CN * jpeg.tiles(CW, CH)
    px = CW * CH
    rng = np.random.default_rng(7)                          # --crop's rectangles
    im = rng.integers(0, CN, NCROPS)
    x = rng.integers(0, CW - CROP + 1, NCROPS)
    y = rng.integers(0, CH - CROP + 1, NCROPS)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(dev)
    cols = [t64(im), t64(x), t64(y), t64(np.full(NCROPS, CROP)), t64(np.full(NCROPS, CROP))]
    d_dst4 = t64(np.arange(NCROPS) * 4 * CROP * CROP)
    d_dst3 = t64(np.arange(NCROPS) * 3 * CROP * CROP)
    cap4, cap3 = NCROPS * 4 * CROP * CROP, NCROPS * 3 * CROP * CROP
    d_flip = torch.from_numpy((np.arange(NCROPS) % 2).astype(np.uint8)).to(dev)      # half mirrored
    mask = d_flip.bool().view(NCROPS, 1, 1, 1)
    scale, bias = jpeg.normalisation(IMAGENET_MEAN, IMAGENET_STD)
    d_scale, d_bias = (torch.tensor(v, dtype=torch.float32, device=dev).view(1, 3, 1, 1) for v in (scale, bias))
    images = {}
    d_img = torch.empty(CN * px * 4, dtype=torch.uint8, device=dev)
    synth.rand_rgba_device(d_img, 0, CN * px, seed=1)
    images["random"] = d_img
    images["smooth"] = torch.from_numpy(smooth_image(CW, CH)).to(dev).reshape(-1).repeat(CN)
    d_offs = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    d_ires = torch.empty(2, dtype=torch.int64, device=dev)
    d_res, d_tres = (torch.empty(3, dtype=torch.int64, device=dev) for _ in range(2))
    iscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device=dev)
    cscr = torch.empty(jpeg.crop_scratch_bytes(NCROPS, CROP, CROP), dtype=torch.uint8, device=dev)
    d_rgba = torch.empty(cap4, dtype=torch.uint8, device=dev)
    d_f32 = torch.empty(cap3, dtype=torch.float32, device=dev)
    d_bf16 = torch.empty(cap3, dtype=torch.bfloat16, device=dev)
    for name, img in images.items():
        for tight in (False, True):
            d_stream = jpeg.compress_device(img, CW, CH, CN, tight=tight)
            n = d_stream.numel()
            jpeg.stream_index_device(d_stream, n, CW, CH, CN, d_offsets=d_offs, d_result=d_ires, scratch=iscr)

            def crops():
                jpeg.crop_device(d_stream, n, CW, CH, CN, d_offs, *cols, CROP, CROP, d_dst=d_dst4,
                                 d_out=d_rgba, out_cap=cap4, scratch=cscr, d_result=d_res, check=False)

            def tensor(d_out, dtype):
                jpeg.crop_tensor_device(d_stream, n, CW, CH, CN, d_offs, *cols, CROP, CROP, d_dst=d_dst3,
                                        d_out=d_out, out_cap=cap3, scratch=cscr, d_result=d_tres,
                                        check=False, dtype=dtype, layout="chw", scale=scale, bias=bias,
                                        d_flip=d_flip)

            def chain(dtype):
                crops()
                t = d_rgba.view(NCROPS, CROP, CROP, 4)[..., :3].permute(0, 3, 1, 2).float()
                t = t.mul(d_scale).add(d_bias)
                if dtype != torch.float32:
                    t = t.to(dtype)
                return torch.where(mask, t.flip(3), t)

            calls = [("tensor_f32", lambda: tensor(d_f32, torch.float32)),
                     ("tensor_bf16", lambda: tensor(d_bf16, torch.bfloat16)),
                     ("chain_f32", lambda: chain(torch.float32)),
                     ("chain_bf16", lambda: chain(torch.bfloat16)),
                     ("crops", crops)]
            if args.once:
                for _ in range(args.once):
                    calls[0][1]()
                    calls[1][1]()
                torch.cuda.synchronize()
                continue
            calls[0][1]()
            ok = d_tres.cpu().tolist() == [NCROPS, -1, 0]
            calls[1][1]()
            ok = ok and d_tres.cpu().tolist() == [NCROPS, -1, 0]
            ok = ok and bool(torch.equal(d_f32.view(NCROPS, 3, CROP, CROP).view(torch.int32),
                                         chain(torch.float32).contiguous().view(torch.int32)))
            ok = ok and bool(torch.equal(d_bf16.view(NCROPS, 3, CROP, CROP).view(torch.int16),
                                         chain(torch.bfloat16).contiguous().view(torch.int16)))
            ok = ok and d_ires.cpu().tolist() == [n, -1] and d_res.cpu().tolist() == [NCROPS, -1, 0]
            res = {"stream": f"{name} {CN} x {CW}x{CH} {'JPT1' if tight else 'JPR1'}",
                   "crops": f"{NCROPS} of {CROP}x{CROP}, every second one mirrored", "outputs_equal": ok,
                   "steps": args.steps, "rounds": args.rounds, "rgba_bytes": cap4, "f32_bytes": 4 * cap3,
                   "bf16_bytes": 2 * cap3}
            if other is not None:         # crop_device of either build by the same bare C call
                import ctypes
                vp = lambda t: ctypes.c_void_p(t.data_ptr())
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                a_rgba, a_res = torch.empty_like(d_rgba), torch.empty_like(d_res)
                rects = torch.stack((*cols, d_dst4), dim=1).contiguous()

                def crops_on(lib, out, r):
                    checked(lib.jpegr_crop_device(vp(d_stream), n, CW, CH, CN, vp(d_offs), vp(rects), NCROPS,
                                                  CROP, CROP, vp(out), cap4, vp(cscr), vp(r), st))

                calls += [("bare_crops", lambda: crops_on(jpeg._lib.lib(), d_rgba, d_res)),
                          ("against_bare_crops", lambda: crops_on(other, a_rgba, a_res))]
                calls[-2][1]()
                calls[-1][1]()
                torch.cuda.synchronize()
                res["against_outputs_equal"] = bool(torch.equal(a_rgba, d_rgba)) and bool(torch.equal(a_res, d_res))
            ms = {k: [] for k, _ in calls}
            for r in range(args.rounds):                  # alternated; the order turns with the round
                for key, fn in calls[r % len(calls):] + calls[:r % len(calls)]:
                    settle(fn, torch.cuda.synchronize, chunk=4)
                    ms[key].append(timed(fn, args.steps, torch))
            for key, _ in calls:
                res[key + "_ms"] = spread(ms[key])
            med = lambda k: res[k + "_ms"]["median"]
            if other is not None:
                over_against(res, ["bare_crops"])
            for d in ("f32", "bf16"):
                res[f"tensor_{d}_over_chain_{d}"] = round(med("tensor_" + d) / med("chain_" + d), 4)
                res[f"tensor_{d}_over_crops"] = round(med("tensor_" + d) / med("crops"), 4)
            print(json.dumps(res), flush=True)
            del d_stream


def random_resized_rects(rng, n, w, h, nimg):
    """n rectangles as torchvision's RandomResizedCrop.get_params draws them:
    area 8 to 100 % of the image, aspect log-uniform in 3/4 .. 4/3, ten tries,
    then the central crop of the nearest allowed aspect."""
    out = []
    for _ in range(n):
        for _ in range(10):
            area = w * h * rng.uniform(0.08, 1.0)
            ar = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
            cw, ch = int(round(np.sqrt(area * ar))), int(round(np.sqrt(area / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                x, y = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1))
                break
        else:
            if w / h < 3 / 4:
                cw, ch = w, int(round(w / (3 / 4)))
            elif w / h > 4 / 3:
                cw, ch = int(round(h * (4 / 3))), h
            else:
                cw, ch = w, h
            x, y = (w - cw) // 2, (h - ch) // 2
        out.append((int(rng.integers(0, nimg)), x, y, cw, ch))
    return out


def resize_side(args, torch, jpeg, synth, dev):
    """Crops resampled to one size (jpegr_crop_resize_device) beside the chain it
    replaces (packed float32 crops, one interpolate a crop) and beside
    crop_tensor_device of the same rectangles alone."""
    import torch.nn.functional as F
    nt = CN * jpeg.tiles(CW, CH)
    px = CW * CH
    rects = random_resized_rects(np.random.default_rng(7), NCROPS, CW, CH, CN)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(dev)
    cols = [t64([r[k] for r in rects]) for k in range(5)]
    mw, mh = max(r[3] for r in rects), max(r[4] for r in rects)
    sizes = [3 * r[3] * r[4] for r in rects]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    capp, capo = int(starts[-1]), NCROPS * 3 * CROP * CROP
    d_dstp, d_dsto = t64(starts[:-1]), t64(np.arange(NCROPS) * 3 * CROP * CROP)
    d_flip = torch.from_numpy((np.arange(NCROPS) % 2).astype(np.uint8)).to(dev)      # half mirrored
    mask = d_flip.bool().view(NCROPS, 1, 1, 1)
    scale, bias = jpeg.normalisation(IMAGENET_MEAN, IMAGENET_STD)
    images = {}
    d_img = torch.empty(CN * px * 4, dtype=torch.uint8, device=dev)
    synth.rand_rgba_device(d_img, 0, CN * px, seed=1)
    images["random"] = d_img
    images["smooth"] = torch.from_numpy(smooth_image(CW, CH)).to(dev).reshape(-1).repeat(CN)
    d_offs = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    d_ires = torch.empty(2, dtype=torch.int64, device=dev)
    d_res, d_tres = (torch.empty(3, dtype=torch.int64, device=dev) for _ in range(2))
    iscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device=dev)
    scr = torch.empty(jpeg.crop_resize_scratch_bytes(NCROPS, mw, mh, CROP, CROP), dtype=torch.uint8, device=dev)
    d_packed = torch.empty(capp, dtype=torch.float32, device=dev)
    d_batch = torch.empty(NCROPS, 3, CROP, CROP, dtype=torch.float32, device=dev)
    d_f32 = torch.empty(capo, dtype=torch.float32, device=dev)
    d_bf16 = torch.empty(capo, dtype=torch.bfloat16, device=dev)
    area = sum(r[3] * r[4] for r in rects)
    for name, img in images.items():
        for tight in (False, True):
            d_stream = jpeg.compress_device(img, CW, CH, CN, tight=tight)
            n = d_stream.numel()
            jpeg.stream_index_device(d_stream, n, CW, CH, CN, d_offsets=d_offs, d_result=d_ires, scratch=iscr)

            def packed():                                   # (b): no resampling, the crops at source scale
                jpeg.crop_tensor_device(d_stream, n, CW, CH, CN, d_offs, *cols, mw, mh, d_dst=d_dstp,
                                        d_out=d_packed, out_cap=capp, scratch=scr, d_result=d_tres,
                                        check=False, dtype=torch.float32, layout="chw", scale=scale,
                                        bias=bias)

            def fused(d_out, dtype):
                jpeg.crop_resize_device(d_stream, n, CW, CH, CN, d_offs, *cols, mw, mh, CROP, CROP,
                                        antialias=True, d_dst=d_dsto, d_out=d_out, out_cap=capo, scratch=scr,
                                        d_result=d_res, check=False, dtype=dtype, layout="chw", scale=scale,
                                        bias=bias, d_flip=d_flip)

            def chain(dtype):                               # (a)
                packed()
                for r, (_, _, _, cw, ch) in enumerate(rects):
                    src = d_packed[int(starts[r]):int(starts[r + 1])].view(1, 3, ch, cw)
                    d_batch[r:r + 1] = F.interpolate(src, size=(CROP, CROP), mode="bilinear",
                                                     align_corners=False, antialias=True)
                t = torch.where(mask, d_batch.flip(3), d_batch)
                return t if dtype == torch.float32 else t.to(dtype)

            calls = [("resize_f32", lambda: fused(d_f32, torch.float32)),
                     ("resize_bf16", lambda: fused(d_bf16, torch.bfloat16)),
                     ("chain_f32", lambda: chain(torch.float32)),
                     ("chain_bf16", lambda: chain(torch.bfloat16)),
                     ("packed_f32", packed)]
            if args.once:
                for _ in range(args.once):
                    calls[0][1]()
                    calls[1][1]()
                torch.cuda.synchronize()
                continue
            calls[0][1]()
            ok = d_res.cpu().tolist() == [NCROPS, -1, 0]
            calls[1][1]()
            ok = ok and d_res.cpu().tolist() == [NCROPS, -1, 0]
            ref = chain(torch.float32)
            ok = ok and d_tres.cpu().tolist() == [NCROPS, -1, 0] and d_ires.cpu().tolist() == [n, -1]
            # the chain normalises before it resamples, the call after: on the
            # normalised scale, and in bytes (divided by the smallest scale)
            diff = float((d_f32.view(NCROPS, 3, CROP, CROP) - ref).abs().max().item())
            res = {"stream": f"{name} {CN} x {CW}x{CH} {'JPT1' if tight else 'JPR1'}",
                   "crops": f"{NCROPS} RandomResizedCrop rectangles to {CROP}x{CROP}, every second one mirrored",
                   "max_w": mw, "max_h": mh, "source_pixels": area, "verdicts_ok": ok,
                   "max_abs_diff_f32_vs_chain": diff, "max_abs_diff_in_bytes": diff / min(scale),
                   "steps": args.steps, "rounds": args.rounds, "scratch_bytes": scr.numel(),
                   "packed_f32_bytes": 4 * capp, "out_f32_bytes": 4 * capo}
            del ref
            ms = {k: [] for k, _ in calls}
            for r in range(args.rounds):                  # alternated; the order turns with the round
                for key, fn in calls[r % len(calls):] + calls[:r % len(calls)]:
                    settle(fn, torch.cuda.synchronize, chunk=1)
                    ms[key].append(timed(fn, args.steps, torch))
            for key, _ in calls:
                res[key + "_ms"] = spread(ms[key])
            for d in ("f32", "bf16"):
                res[f"resize_{d}_over_chain_{d}"] = {
                    "median": round(res[f"resize_{d}_ms"]["median"] / res[f"chain_{d}_ms"]["median"], 4),
                    "worst": round(res[f"resize_{d}_ms"]["max"] / res[f"chain_{d}_ms"]["min"], 4)}
                res[f"resize_{d}_over_packed"] = {
                    "min": round(min(a / b for a, b in zip(ms[f"resize_{d}"], ms["packed_f32"])), 4),
                    "median": round(res[f"resize_{d}_ms"]["median"] / res["packed_f32_ms"]["median"], 4),
                    "max": round(max(a / b for a, b in zip(ms[f"resize_{d}"], ms["packed_f32"])), 4)}
            print(json.dumps(res), flush=True)
            del d_stream


def dataset_sizes(s):
    """Stream s's (w, h): 320 .. 546 by 240 .. 420, no two neighbours alike."""
    return 320 + 8 * (s % 29) + s % 3, 240 + 8 * ((7 * s) % 23) + s % 5


def dataset_side(args, torch, jpeg, synth, dev):
    """One jpegr_dataset_crop_resize_device call beside the S
    jpegr_crop_resize_device calls that write the same tensor."""
    from lz4jpeg import _lib
    nimg = 2
    scale, bias = jpeg.normalisation(IMAGENET_MEAN, IMAGENET_STD)
    scale3, bias3 = jpeg._float3(scale, "scale"), jpeg._float3(bias, "bias")
    per = 3 * CROP * CROP
    capo = NCROPS * per
    d_flip = torch.from_numpy((np.arange(NCROPS) % 2).astype(np.uint8)).to(dev)
    d_out = [torch.empty(capo, dtype=torch.float32, device=dev) for _ in range(2)]
    d_res = torch.empty(3, dtype=torch.int64, device=dev)
    d_sres = torch.empty(256, 3, dtype=torch.int64, device=dev)
    stream = jpeg.stream_arg(None)
    readers = []
    for s in range(256):
        w, h = dataset_sizes(s)
        d_img = torch.empty(nimg * w * h * 4, dtype=torch.uint8, device=dev)
        synth.rand_rgba_device(d_img, 0, nimg * w * h, seed=1 + s)
        readers.append(jpeg.StreamReader(jpeg.compress_device(d_img, w, h, nimg, tight=bool(s & 1))))
    for S in (1, 16, 256):
        rng = np.random.default_rng(7)
        ds = jpeg.Dataset(readers[:S])
        rects = []                                          # rectangle r from stream r % S
        for r in range(NCROPS):
            rd = readers[r % S]
            im, x, y, cw, ch = random_resized_rects(rng, 1, rd.w, rd.h, nimg)[0]
            rects.append((int(ds.image0[r % S]) + im, x, y, cw, ch, r * per))
        mw, mh = max(r[3] for r in rects), max(r[4] for r in rects)
        d_rects = torch.from_numpy(np.asarray(rects, np.int64)).to(dev)
        scr = torch.empty(jpeg.dataset_crop_resize_scratch_bytes(NCROPS, mw, mh, CROP, CROP), dtype=torch.uint8,
                          device=dev)
        singles = []                                        # per stream: its rectangles with local image indices
        for s in range(S):
            rows = list(range(s, NCROPS, S))
            local = [(rects[r][0] - int(ds.image0[s]),) + rects[r][1:] for r in rows]
            singles.append((readers[s], torch.from_numpy(np.asarray(local, np.int64)).to(dev), len(rows),
                            d_flip[rows].contiguous(), min(mw, readers[s].w), min(mh, readers[s].h)))

        def dataset():
            checked(_lib.call("jpegr_dataset_crop_resize_device", ds.d_table, S, d_rects, NCROPS, d_flip, mw, mh,
                              CROP, CROP, 1, 1, 0, scale3, bias3, d_out[0], capo, scr, d_res, stream))

        def per_stream():
            for s, (rd, d_loc, n, d_fl, smw, smh) in enumerate(singles):
                checked(_lib.call("jpegr_crop_resize_device", rd.d_stream, rd.length, rd.w, rd.h, rd.nimg,
                                  rd.d_offsets, d_loc, n, d_fl, smw, smh, CROP, CROP, 1, 1, 0, scale3, bias3,
                                  d_out[1], capo, scr, d_sres[s], stream))

        calls = [("dataset", dataset), ("per_stream", per_stream)]
        if args.once:
            for _ in range(args.once):
                dataset()
            torch.cuda.synchronize()
            continue
        d_out[0].fill_(-1.0)
        d_out[1].fill_(-2.0)
        dataset()
        per_stream()
        ok = d_res.cpu().tolist() == [NCROPS, -1, 0]
        ok = ok and d_sres[:S].cpu().tolist() == [[len(range(s, NCROPS, S)), -1, 0] for s in range(S)]
        steps = max(4, args.steps // max(1, S // 4))
        res = {"streams": S, "sizes": "320..546 x 240..420, JPR1 and JPT1 alternating, 2 images each",
               "crops": f"{NCROPS} RandomResizedCrop rectangles to {CROP}x{CROP} float32 CHW, every second one "
                        "mirrored", "max_w": mw, "max_h": mh, "verdicts_ok": ok,
               "outputs_equal": bool(torch.equal(d_out[0].view(torch.int32), d_out[1].view(torch.int32))),
               "steps": steps, "rounds": args.rounds, "scratch_bytes": scr.numel()}
        ms = {k: [] for k, _ in calls}
        for r in range(args.rounds):                        # alternated; the order turns with the round
            for key, fn in calls[r % 2:] + calls[:r % 2]:
                settle(fn, torch.cuda.synchronize, chunk=1)
                ms[key].append(timed(fn, steps, torch))
        for key, _ in calls:
            res[key + "_ms"] = spread(ms[key])
        res["dataset_over_per_stream"] = {
            "min": round(min(a / b for a, b in zip(ms["dataset"], ms["per_stream"])), 4),
            "median": round(res["dataset_ms"]["median"] / res["per_stream_ms"]["median"], 4),
            "max": round(max(a / b for a, b in zip(ms["dataset"], ms["per_stream"])), 4)}
        print(json.dumps(res), flush=True)


def thumb_side(args, torch, jpeg, synth, dev, other):
    """Thumbnails straight from the stream beside decode-everything-and-pool."""
    import ctypes
    per = jpeg.tiles(CW, CH)
    nt = CN * per
    px = CW * CH
    gw, gh = (CW + 7) // 8, (CH + 7) // 8
    images = {}
    d_img = torch.empty(CN * px * 4, dtype=torch.uint8, device=dev)
    synth.rand_rgba_device(d_img, 0, CN * px, seed=1)
    images["random"] = d_img
    images["smooth"] = torch.from_numpy(smooth_image(CW, CH)).to(dev).reshape(-1).repeat(CN)
    d_offs = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    d_ires = torch.empty(2, dtype=torch.int64, device=dev)
    d_res, d_res_scan, d_res3, d_res_alt = (torch.empty(3, dtype=torch.int64, device=dev) for _ in range(4))
    iscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device=dev)
    d_out, d_out_scan, d_out_alt = (torch.empty(nt * 4, dtype=torch.uint8, device=dev) for _ in range(3))
    d_coef = torch.empty(nt * 128, dtype=torch.int16, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    for name, img in images.items():
        for tight in (False, True):
            d_stream = jpeg.compress_device(img, CW, CH, CN, tight=tight)
            n = d_stream.numel()

            def index():
                jpeg.stream_index_device(d_stream, n, CW, CH, CN, d_offsets=d_offs, d_result=d_ires,
                                         scratch=iscr)

            def thumbs():
                jpeg.thumb_device(d_stream, n, CW, CH, CN, d_offsets=d_offs, d_out=d_out, d_result=d_res)

            def thumbs_scan():
                jpeg.thumb_device(d_stream, n, CW, CH, CN, d_out=d_out_scan, scratch=iscr,
                                  d_result=d_res_scan)

            def on(lib, offs, out, res):                  # the C call itself, of either build
                rc = lib.jpegr_thumb_device(vp(d_stream), n, CW, CH, CN, vp(d_offs if offs else None), 0,
                                            CN, vp(out), None, vp(iscr), vp(res),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0

            def decode_all():
                jpeg.decode_stream_device(d_stream, n, CW, CH, CN, d_coef=d_coef, d_result=d_res3,
                                          scratch=iscr)
                return jpeg.reconstruct_device(d_coef, CW, CH, CN)

            def decode_all_and_pool():
                full = decode_all().view(CN, CH, CW, 4).permute(0, 3, 1, 2).float()
                return torch.nn.functional.avg_pool2d(full, 8)

            index()
            if args.once:
                for _ in range(args.once):
                    thumbs()
                torch.cuda.synchronize()
                continue
            thumbs()
            thumbs_scan()
            decode_all()
            dc_only = torch.zeros_like(d_coef).view(nt, 128)
            dc_only[:, [0, 64, 96]] = d_coef.view(nt, 128)[:, [0, 64, 96]]
            want = jpeg.reconstruct_device(dc_only.view(-1), CW, CH, CN).view(CN, CH, CW, 4)[:, ::8, ::8]
            torch.cuda.synchronize()
            ok = bool(torch.equal(d_out.view(CN, gh, gw, 4), want)) and bool(torch.equal(d_out, d_out_scan)) \
                and d_ires.cpu().tolist() == [n, -1] and d_res.cpu().tolist() == [n, -1, 0] \
                and d_res_scan.cpu().tolist() == [n, -1, 0] and d_res3.cpu().tolist() == [n, -1, 0]
            calls = [("thumbs", thumbs), ("thumbs_scan", thumbs_scan), ("index", index),
                     ("decode_all_and_pool", decode_all_and_pool), ("decode_all", decode_all)]
            if other is not None:                         # both builds' pair by the same bare call
                mine = jpeg._lib.lib()
                calls[:2] = [("thumbs", lambda: on(mine, True, d_out, d_res)),
                             ("thumbs_scan", lambda: on(mine, False, d_out_scan, d_res_scan))]
                calls += [("alt_thumbs", lambda: on(other, True, d_out_alt, d_res_alt)),
                          ("alt_thumbs_scan", lambda: on(other, False, d_out_alt, d_res_alt))]
                for offs in (True, False):
                    on(other, offs, d_out_alt, d_res_alt)
                    torch.cuda.synchronize()
                    ok = ok and bool(torch.equal(d_out_alt, d_out)) and d_res_alt.cpu().tolist() == [n, -1, 0]
            del dc_only, want
            res = {"stream": f"{name} {CN} x {CW}x{CH} {'JPT1' if tight else 'JPR1'}", "tiles": nt,
                   "stream_bytes": n, "thumbnails": f"{CN} of {gw}x{gh}", "outputs_equal": ok,
                   "steps": args.steps, "rounds": args.rounds}
            ms = {k: [] for k, _ in calls}
            for r in range(args.rounds):                  # alternated; the order turns with the round
                for key, fn in calls[r % len(calls):] + calls[:r % len(calls)]:
                    settle(fn, torch.cuda.synchronize, chunk=4)
                    ms[key].append(timed(fn, args.steps, torch))
            for key, _ in calls:
                res[key + "_ms"] = spread(ms[key])
            med = lambda k: res[k + "_ms"]["median"]
            for key, _ in calls:
                res[key + "_stream_MB_per_ms"] = round(n / 1e6 / med(key), 2)
                if key != "decode_all_and_pool":
                    res[key + "_over_decode_all_and_pool"] = round(med(key) / med("decode_all_and_pool"), 4)
            if other is not None:
                res["thumbs_over_alt"] = round(med("thumbs") / med("alt_thumbs"), 4)
                res["thumbs_scan_over_alt"] = round(med("thumbs_scan") / med("alt_thumbs_scan"), 4)
            print(json.dumps(res), flush=True)
            del d_stream


def select_side(args, torch, jpeg, synth, dev, other):
    """Editing the stream (jpegr_select_device) beside decode + encode and a plain copy."""
    per = jpeg.tiles(CW, CH)
    nt = CN * per
    px = CW * CH
    rng = np.random.default_rng(7)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(dev)
    order = rng.permutation(CN)[:CN // 2]
    zeros = np.zeros(len(order))
    sub_cols = [t64(order), t64(zeros), t64(zeros)]
    wt = CROP // 8                                       # a window's tiles each way
    wim = rng.integers(0, CN, NCROPS)
    wx = 8 * rng.integers(0, (CW - CROP) // 8 + 1, NCROPS)
    wy = 8 * rng.integers(0, (CH - CROP) // 8 + 1, NCROPS)
    win_cols = [t64(wim), t64(wx), t64(wy)]
    gw = (CW + 7) // 8
    oy, ox = np.mgrid[0:wt, 0:wt]
    d_wtiles = t64(((wim * per + (wy // 8) * gw + wx // 8)[:, None, None] + oy[None] * gw + ox[None]).reshape(-1))
    all_cols = [t64(np.arange(CN)), t64(np.zeros(CN)), t64(np.zeros(CN))]
    nsub, nwin = len(order) * per, NCROPS * wt * wt
    images = {}
    d_img = torch.empty(CN * px * 4, dtype=torch.uint8, device=dev)
    synth.rand_rgba_device(d_img, 0, CN * px, seed=1)
    images["random"] = d_img
    images["smooth"] = torch.from_numpy(smooth_image(CW, CH)).to(dev).reshape(-1).repeat(CN)
    d_offs = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    d_ires = torch.empty(2, dtype=torch.int64, device=dev)
    iscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device=dev)
    d_coef = torch.empty(nt * 128, dtype=torch.int16, device=dev)
    d_res3 = torch.empty(3, dtype=torch.int64, device=dev)
    ent = jpeg.Entropy(nt, device=dev)
    d_ures = torch.empty(2, dtype=torch.int64, device=dev)
    for name, img in images.items():
        for tight in (False, True):
            d_stream = jpeg.compress_device(img, CW, CH, CN, tight=tight)
            n = d_stream.numel()
            cap = 2 * n                                   # JPR1 from JPT1 is 1.4 to 1.5 times the source
            jpeg.stream_index_device(d_stream, n, CW, CH, CN, d_offsets=d_offs, d_result=d_ires,
                                     scratch=iscr)
            out = {k: torch.empty(cap, dtype=torch.uint8, device=dev) for k in ("sub", "win", "all")}
            base = {k: torch.empty(cap, dtype=torch.uint8, device=dev) for k in ("sub", "win", "all")}
            d_copy = torch.empty(cap, dtype=torch.uint8, device=dev)
            lens = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in out}
            blens = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in out}
            ress = {k: torch.empty(3, dtype=torch.int64, device=dev) for k in out}
            bres = torch.empty(2, dtype=torch.int64, device=dev)
            shapes = {"sub": (sub_cols, CW, CH, tight), "win": (win_cols, CROP, CROP, tight),
                      "all": (all_cols, CW, CH, not tight),
                      # the same two with format 0, "the source's": nothing can need re-coding
                      "sub0": (sub_cols, CW, CH, None), "win0": (win_cols, CROP, CROP, None)}
            for k in ("sub0", "win0"):
                out[k] = torch.empty(cap, dtype=torch.uint8, device=dev)
                lens[k] = torch.zeros(1, dtype=torch.int64, device=dev)
                ress[k] = torch.empty(3, dtype=torch.int64, device=dev)
            scr = {k: torch.empty(jpeg.select_scratch_bytes(c[0].numel(), ow, oh), dtype=torch.uint8, device=dev)
                   for k, (c, ow, oh, _) in shapes.items()}
            escr = {k: torch.empty(jpeg.stream_encode_scratch_bytes(m, cap), dtype=torch.uint8, device=dev)
                    for k, m in (("sub", nsub), ("win", nwin), ("all", nt))}
            pscr = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device=dev)

            def select(k):
                cols, ow, oh, tg = shapes[k]
                jpeg.select_device(d_stream, n, CW, CH, CN, d_offs, *cols, ow, oh, tight=tg, d_out=out[k],
                                   d_len=lens[k], scratch=scr[k], d_result=ress[k])

            def encode(k, coef, ow, oh, count, tg):
                jpeg.encode_stream_device(coef, ow, oh, count, tight=tg, d_out=base[k], d_len=blens[k],
                                          d_result=bres, scratch=escr[k])

            def sub_today():                              # the images' tile ranges, one decode each
                for i, im in enumerate(order.tolist()):
                    jpeg.decode_stream_device(d_stream, n, CW, CH, CN, im * per, per,
                                              d_coef=d_coef[i * per * 128:(i + 1) * per * 128],
                                              d_result=d_res3, scratch=iscr)
                encode("sub", d_coef, CW, CH, len(order), tight)

            def win_today():                              # everything decoded, the windows' tiles gathered
                jpeg.decode_stream_device(d_stream, n, CW, CH, CN, d_coef=d_coef, d_result=d_res3, scratch=iscr)
                encode("win", d_coef.view(nt, 128)[d_wtiles].view(-1), CROP, CROP, NCROPS, tight)

            def all_today():
                if tight:                                 # JPT1 -> JPR1: no slot form, decode and encode
                    jpeg.decode_stream_device(d_stream, n, CW, CH, CN, d_coef=d_coef, d_result=d_res3,
                                              scratch=iscr)
                    encode("all", d_coef, CW, CH, CN, False)
                else:                                     # JPR1 -> JPT1: the slots rebuilt and packed again
                    jpeg.unpack_device(d_stream, n, CW, CH, CN, ent=ent, d_result=d_ures, scratch=iscr)
                    jpeg.pack_device(ent, CW, CH, CN, d_out=base["all"], d_len=blens["all"], scratch=pscr,
                                     tight=True)

            today = {"sub": sub_today, "win": win_today, "all": all_today}
            if args.once:
                for _ in range(args.once):
                    for k in out:
                        select(k)
                torch.cuda.synchronize()
                continue
            ok, wrote = True, {}
            for k in ("sub0", "win0"):
                select(k)
            for k in today:
                select(k)
                today[k]()
                torch.cuda.synchronize()
                m = int(lens[k].item())
                wrote[k] = m
                ok = ok and m <= cap and m == int(blens[k].item()) and ress[k].cpu().tolist() == [m, -1, 0] \
                    and bool(torch.equal(out[k][:m], base[k][:m]))
            for k in ("sub0", "win0"):
                ok = ok and ress[k].cpu().tolist() == [wrote[k[:3]], -1, 0] \
                    and bool(torch.equal(out[k][:wrote[k[:3]]], out[k[:3]][:wrote[k[:3]]]))
            names = {"sub": f"{len(order)} of {CN} images, shuffled", "win": f"{NCROPS} windows of {CROP}x{CROP}",
                     "all": "whole stream to " + ("JPR1" if tight else "JPT1")}
            res = {"stream": f"{name} {CN} x {CW}x{CH} {'JPT1' if tight else 'JPR1'}", "tiles": nt,
                   "stream_bytes": n, "outputs_equal": ok, "steps": args.steps, "rounds": args.rounds,
                   "what": names, "bytes_written": wrote,
                   "tiles_written": {"sub": nsub, "win": nwin, "all": nt}}
            sel = lambda k: (lambda: select(k))
            if other is not None:         # the five calls of either build by the same bare C call
                import ctypes
                vp = lambda t: ctypes.c_void_p(t.data_ptr())
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                items = {k: torch.stack(c[0], dim=1).contiguous() for k, c in shapes.items()}
                theirs = {k: (torch.empty_like(out[k]), torch.zeros_like(lens[k]), torch.empty_like(ress[k]))
                          for k in shapes}

                def select_on(lib, k, to):
                    _, ow, oh, tg = shapes[k]
                    checked(lib.jpegr_select_device(vp(d_stream), n, CW, CH, CN, vp(d_offs), vp(items[k]),
                                                    items[k].shape[0], ow, oh, 0 if tg is None else 2 if tg else 1,
                                                    vp(to[0]), to[0].numel(), vp(to[1]), vp(scr[k]), vp(to[2]), st))

                mine = jpeg._lib.lib()
                sel = lambda k: (lambda: select_on(mine, k, (out[k], lens[k], ress[k])))
                against = {k: (lambda k=k: select_on(other, k, theirs[k])) for k in shapes}
            calls = [(k + "_select", sel(k)) for k in ("sub0", "win0")]
            for k in today:
                calls += [(k + "_select", sel(k)), (k + "_today", today[k]),
                          (k + "_copy", lambda k=k: d_copy[:wrote[k]].copy_(out[k][:wrote[k]]))]
            if other is not None:
                calls += [("against_" + k + "_select", fn) for k, fn in against.items()]
                same = True
                for k in shapes:
                    sel(k)()
                    against[k]()
                    torch.cuda.synchronize()
                    m = wrote[k[:3]]
                    same = same and int(theirs[k][1].item()) == m and bool(torch.equal(theirs[k][2], ress[k])) \
                        and bool(torch.equal(theirs[k][0][:m], out[k][:m]))
                res["against_outputs_equal"] = same
            ms = {k: [] for k, _ in calls}
            for r in range(args.rounds):                  # alternated; the order turns with the round
                for key, fn in calls[r % len(calls):] + calls[:r % len(calls)]:
                    settle(fn, torch.cuda.synchronize, chunk=4)
                    ms[key].append(timed(fn, args.steps, torch))
            for key, _ in calls:
                res[key + "_ms"] = spread(ms[key])
            if other is not None:
                over_against(res, [k + "_select" for k in shapes])
            med = lambda k: res[k + "_ms"]["median"]
            for k in today:
                res[k + "_select_over_today"] = round(med(k + "_select") / med(k + "_today"), 4)
                res[k + "_select_over_copy"] = round(med(k + "_select") / med(k + "_copy"), 4)
                res[k + "_select_MB_per_ms"] = round(wrote[k] / 1e6 / med(k + "_select"), 2)
                res[k + "_copy_MB_per_ms"] = round(wrote[k] / 1e6 / med(k + "_copy"), 2)
            print(json.dumps(res), flush=True)
            del d_stream, out, base, d_copy, escr, scr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tight", action="store_true")
    ap.add_argument("--direct", action="store_true")
    ap.add_argument("--crop", action="store_true")
    ap.add_argument("--thumb", action="store_true")
    ap.add_argument("--select", action="store_true")
    ap.add_argument("--tensor", action="store_true")
    ap.add_argument("--resize", action="store_true")
    ap.add_argument("--dataset", action="store_true")
    ap.add_argument("--against", default=None,
                    help="with --tight, --direct, --crop, --select or --tensor: a second liblz4jpeg.so to "
                         "alternate with; with --thumb: that, or a second build of jpegr_thumb.hip "
                         "alone (make thumb-alt)")
    args = ap.parse_args()
    import torch
    from lz4jpeg import jpeg, synth
    if not torch.cuda.is_available():
        sys.exit("jpeg_pack_bench: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    if args.crop or args.thumb or args.select or args.tensor or args.resize or args.dataset:
        if not args.once:                   # clock pre-warm (bench.py run_lz4)
            d_warm = torch.zeros(256 << 20, dtype=torch.uint8, device=dev)
            settle(lambda: d_warm.add_(1), torch.cuda.synchronize, ms=100.0, chunk=16)
            del d_warm
        if args.dataset:
            dataset_side(args, torch, jpeg, synth, dev)
        elif args.resize:
            resize_side(args, torch, jpeg, synth, dev)
        elif args.tensor:
            tensor_side(args, torch, jpeg, synth, dev, second_build(args.against) if args.against else None)
        elif args.crop:
            crop_side(args, torch, jpeg, synth, dev, second_build(args.against) if args.against else None)
        elif args.select:
            select_side(args, torch, jpeg, synth, dev, second_build(args.against) if args.against else None)
        else:
            import ctypes
            thumb_side(args, torch, jpeg, synth, dev, second_build(args.against) if args.against else None)
        return
    nt = jpeg.tiles(W, H)
    images = {}
    d_img = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)
    synth.rand_rgba_device(d_img, 0, W * H, seed=1)
    images["random"] = d_img
    images["smooth"] = torch.from_numpy(smooth_image(W, H)).to(dev).reshape(-1)

    if not args.once:                       # clock pre-warm (bench.py run_lz4)
        d_warm = torch.zeros(256 << 20, dtype=torch.uint8, device=dev)
        settle(lambda: d_warm.add_(1), torch.cuda.synchronize, ms=100.0, chunk=16)
        del d_warm

    other = None
    if args.against:
        import ctypes
        other = ctypes.CDLL(os.path.abspath(args.against), mode=ctypes.RTLD_LOCAL)

    for name, img in images.items():
        d_coef = jpeg.encode_device(img, W, H)
        if args.direct:
            torch.cuda.synchronize()
            direct_side(args, torch, jpeg, name, img, d_coef, other)
            continue
        ent = jpeg.Entropy(nt, device=dev)
        ent.encode(d_coef)
        if args.tight:
            torch.cuda.synchronize()
            tight_side(args, torch, jpeg, name, ent, d_coef, other)
            continue
        back = jpeg.Entropy(nt, device=dev)
        d_out = torch.empty(jpeg.pack_bound(W, H), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_res = torch.zeros(2, dtype=torch.int64, device=dev)
        s1 = torch.empty(int(jpeg._lib.lib().jpegr_pack_scratch_bytes(nt)), dtype=torch.uint8, device=dev)
        s2 = torch.empty_like(s1)
        jpeg.pack_device(ent, W, H, d_out=d_out, d_len=d_len, scratch=s1)
        n = int(d_len.item())

        def pack():
            jpeg.pack_device(ent, W, H, d_out=d_out, d_len=d_len, scratch=s1)

        def unpack():
            jpeg.unpack_device(d_out, n, W, H, ent=back, d_result=d_res, scratch=s2)

        if args.decode:
            decode_side(args, torch, jpeg, name, img, d_coef, d_out, n, back, d_res, s2, unpack)
            continue
        if args.once:
            for _ in range(args.once):
                pack()
                unpack()
            torch.cuda.synchronize()
            continue
        unpack()
        d_coef2 = torch.empty_like(d_coef)
        back.decode(d_coef2)
        torch.cuda.synchronize()
        ok = d_res.cpu().tolist() == [n, -1] and bool(torch.equal(d_coef2, d_coef)) \
            and int(back.status[1].item()) == 0
        meta = ent.meta.to(torch.int64) & 0xFFFFFFFF
        live = 12 * nt + 4 * int((meta >> 24).sum().item()) + \
            int((((meta & 0xFFFF) + 7) // 8).sum().item())          # slot bytes that matter
        res = {"image": f"{name} {W}x{H}", "tiles": nt, "stream_bytes": n,
               "bytes_per_tile": round(n / nt, 2), "ratio_to_rgba": round(n / (256 * nt), 4),
               "roundtrip_ok": ok, "steps": args.steps}
        for key, fn in (("pack", pack), ("unpack", unpack), ("entropy_encode", lambda: ent.encode(d_coef)),
                        ("entropy_decode", lambda: back.decode(d_coef2))):
            warm = settle(fn, torch.cuda.synchronize, chunk=20)
            res[key + "_ms"] = round(timed(fn, args.steps, torch), 4)
            res[key + "_warmup"] = warm
        # pack reads the live slot bytes and writes the stream (its index twice:
        # u32 for the scan, u16 in the stream); unpack the reverse
        alg = live + n + 2 * 4 * nt
        res["algorithmic_bytes"] = alg
        res["pack_alg_gbs"] = round(alg / (res["pack_ms"] / 1e3) / 1e9, 1)
        res["unpack_alg_gbs"] = round(alg / (res["unpack_ms"] / 1e3) / 1e9, 1)
        settle(lambda: jpeg.compress_device(img, W, H), torch.cuda.synchronize, chunk=4)
        t0 = time.perf_counter()
        k = max(1, args.steps // 10)
        for _ in range(k):
            jpeg.compress_device(img, W, H)
        torch.cuda.synchronize()
        res["compress_device_ms"] = round((time.perf_counter() - t0) / k * 1e3, 4)
        res["compress_device_note"] = "host clock; allocates its buffers and reads the length back"
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
