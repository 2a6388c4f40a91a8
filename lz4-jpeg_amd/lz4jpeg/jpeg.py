"""Host-side mirror of the reference's JPEG encode hot path over the HIP path.

Reference (Algorithms/sequential/JPEG/JPEG.c main, :1110-1178): colour
matrices -> chroma_subsample -> divide_image -> discrete_cosine_transform ->
Quantize -> zigzag_pattern, per 8x8 tile.  Here one call covers a whole image
(or a batch); output int16 per tile [Y 64 zz][Cr 32 zz][Cb 32 zz], raster tiles.
"""
import ctypes
import functools

import numpy as np

from . import _lib
from ._lib import JpegError, stream_arg

_call = functools.partial(_lib.call, error=JpegError)      # a nonzero return raises


def coef_count(w, h):
    return int(_lib.call("jpegr_coef_count", w, h))


def tiles(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


# ---- what the wrappers below do before and after their calls ----------------------
def _buffer(t, n, dtype, device, short=None, in_bytes=False, floor=0):
    """The caller's tensor t or, when that is None, a new one of n `dtype`
    elements (at least `floor`).  short: the ValueError's text when t holds
    fewer than n elements -- with in_bytes, fewer bytes than n `dtype` elements
    take, whatever t's own dtype."""
    if t is None:
        import torch
        return torch.empty(max(n, floor), dtype=dtype, device=device)
    if short is not None:
        held, need = (t.numel() * t.element_size(), n * dtype.itemsize) if in_bytes else (t.numel(), n)
        if held < need:
            raise ValueError(short)
    return t


def _check_in_len(d_stream, in_len):
    if in_len > d_stream.numel():
        raise ValueError("in_len past the end of d_stream")


def _check_offsets(d_offsets, ntiles):
    if d_offsets.numel() < ntiles + 1:
        raise ValueError("d_offsets smaller than ntiles + 1")


def _image_count(first, count, nimg):
    """count, or with None the images from `first` on; the range lies in the stream."""
    if count is None:
        count = nimg - first
    if first < 0 or count <= 0 or first + count > nimg:
        raise ValueError("image range outside the stream")
    return count


def _open_stream(d_stream, who, slots=False):
    """(w, h, nimg, tight) of a stream on the device, its 16 header bytes read
    back once.  slots: for the slot form, which only JPR1 has (stream_info
    rejects every other magic)."""
    if d_stream.numel() < 16:
        raise JpegError(-1, f"{who}: shorter than a header")
    hdr = d_stream[:16].cpu().numpy().tobytes()
    return (*stream_info(hdr), False) if slots else stream_format(hdr)


def _raise_on_verdict(who, res):
    """res: a call's three result words on the host (jpegr.h): [1] the verdict,
    [2] the rejected entropy streams."""
    if res[1] != -1:
        raise JpegError(-1, f"{who}: inconsistent stream (verdict {res[1]})")
    if res[2] != 0:
        raise JpegError(-1, f"{who}: malformed entropy stream")


def encode_device(d_rgba, w, h, nimg=1, d_out=None, stream=None):
    """d_rgba: uint8 CUDA tensor of nimg*h*w*4 bytes.  Returns int16 tensor of
    nimg*coef_count(w, h) coefficients."""
    import torch
    if d_rgba.numel() < nimg * w * h * 4:
        raise ValueError("d_rgba smaller than nimg*h*w*4")
    d_out = _buffer(d_out, nimg * coef_count(w, h), torch.int16, d_rgba.device)
    _call("jpegr_encode_device", d_rgba, w, h, nimg, d_out, stream_arg(stream))
    return d_out


def dct_raw_device(d_rgba, w, h, nimg=1, stream=None):
    """Un-quantised fp64 DCT coefficients, row-major per plane, 128 per tile."""
    import torch
    d_out = torch.empty(nimg * coef_count(w, h), dtype=torch.float64, device=d_rgba.device)
    _call("jpegr_dct_raw_device", d_rgba, w, h, nimg, d_out, stream_arg(stream))
    return d_out


def time_device(d_rgba, w, h, nimg, d_out, iters, stream=None):
    ms = ctypes.c_float(0)
    _call("jpegr_time_device", d_rgba, w, h, nimg, d_out, iters, stream_arg(stream),
          ctypes.byref(ms))
    return ms.value


def encode(rgba):
    """Host API: rgba uint8 array (h, w, 4) -> int16 array (tiles, 128)."""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("rgba must be (h, w, 4) uint8")
    h, w = a.shape[:2]
    out = np.empty(coef_count(w, h), dtype=np.int16)
    _call("jpegr_encode", a, w, h, out)
    return out.reshape(-1, 128)


def reconstruct_device(d_coef, w, h, nimg=1, d_orig=None, stream=None):
    """Reconstructed RGBA8 (uint8 tensor nimg*h*w*4) from encode_device's
    coefficients: reverse zigzag, dequantisation, fp64 IDCT, YCbCr->RGB
    (JPEG.c:1408-1425).  d_orig reproduces the reference's untransformed
    trailing tiles (see jpegr.h)."""
    import torch
    out = torch.empty(nimg * w * h * 4, dtype=torch.uint8, device=d_coef.device)
    _call("jpegr_reconstruct_device", d_coef, d_orig, w, h, nimg, out, stream_arg(stream))
    return out


class Entropy:
    """Device buffers of the entropy stage for `ntiles` tiles (all images):
    bits (256 B/tile), meta (3 u32/tile), table (256 u32/tile), scratch and
    the status words (see jpegr.h: [0] encode, [1] decode, [2] the decoder's
    call tag)."""

    def __init__(self, ntiles, device="cuda"):
        import torch
        self.ntiles = ntiles
        self.bits = torch.zeros(ntiles * 256, dtype=torch.uint8, device=device)
        self.meta = torch.zeros(ntiles * 3, dtype=torch.int32, device=device)
        self.table = torch.zeros(ntiles * 256, dtype=torch.int32, device=device)
        nscr = _lib.call("jpegr_entropy_scratch_bytes", ntiles)
        self.scratch = torch.empty(nscr, dtype=torch.uint8, device=device)
        self.status = torch.zeros(4, dtype=torch.int32, device=device)

    def encode(self, d_coef, stream=None):
        """RLE + per-stream Huffman + encoded bits of every stream
        (JPEG.c:767-1097) from encode_device's coefficients."""
        _call("jpegr_entropy_encode_device", d_coef, self.ntiles, self.bits, self.meta, self.table,
              self.scratch, self.status, stream_arg(stream))

    def decode(self, d_coef_out, stream=None):
        """bits + tables -> coefficients (decode_huffman + inverse_RLE)."""
        _call("jpegr_entropy_decode_device", self.bits, self.meta, self.table, self.ntiles,
              d_coef_out, self.status, stream_arg(stream))

    def stream(self, tile, c):
        """Host view of one stream: dict(rle_len, table [(value, len)], nbits, bits)."""
        m = int(self.meta[tile * 3 + c].item()) & 0xFFFFFFFF
        nbits, rle_len, ncodes = m & 0xFFFF, (m >> 16) & 255, m >> 24
        off = (0, 128, 192)[c]
        tab = self.table[tile * 256 + off: tile * 256 + off + ncodes].cpu().numpy()
        table = [(int((e & 0xFFFF) ^ 0x8000) - 0x8000, int((e >> 16) & 255)) for e in tab.tolist()]
        raw = self.bits[tile * 256 + off: tile * 256 + off + (nbits + 7) // 8].cpu().numpy()
        return {"rle_len": rle_len, "table": table, "nbits": nbits, "bits": raw.tobytes()}


# ---- the JPR stream (include/jpegr.h): the entropy stage's output as bytes ------
PACK_RECORD_MAX = 1036
STREAM_JPR1, STREAM_JPT1 = 1, 2           # jpegr_stream_format's formats


def pack_bound(w, h, nimg=1):
    return int(_lib.call("jpegr_pack_bound", w, h, nimg))


def _pack_scratch(scratch, ntiles, device):
    """The caller's scratch, or new scratch for a stream of ntiles tiles."""
    if scratch is not None:
        return scratch
    import torch
    return torch.empty(int(_lib.call("jpegr_pack_scratch_bytes", ntiles)), dtype=torch.uint8,
                       device=device)


def pack_device(ent, w, h, nimg=1, d_out=None, stream=None, d_len=None, scratch=None, tight=False):
    """Pack an Entropy's slots into one JPR stream -- JPR1, or with tight=True
    JPT1, the tighter table coding (jpegr.h).  Returns (d_out, d_len):
    d_out a uint8 tensor (pack_bound bytes when not given), d_len a one-element
    int64 tensor holding the stream length -- or the capacity needed when that
    exceeds d_out's size, in which case nothing past d_out is written.
    Asynchronous: no read-back."""
    import torch
    if nimg * tiles(w, h) != ent.ntiles:
        raise ValueError("ent does not hold nimg * tiles(w, h) tiles")
    dev = ent.bits.device
    if d_out is None:
        d_out = torch.empty(pack_bound(w, h, nimg), dtype=torch.uint8, device=dev)
    if d_len is None:
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _pack_scratch(scratch, ent.ntiles, dev)
    _call("jpegr_pack_tight_device" if tight else "jpegr_pack_device", ent.bits, ent.meta, ent.table,
          w, h, nimg, d_out, d_out.numel(), d_len, scratch, stream_arg(stream))
    return d_out, d_len


def unpack_device(d_stream, in_len, w, h, nimg=1, ent=None, stream=None, d_result=None,
                  scratch=None):
    """A JPR stream's first in_len bytes back into an Entropy's slots.  Returns
    (Entropy, d_result): d_result two int64 on the device, [0] the length the
    header and index imply, [1] -1 (all ones) when the stream is consistent, 0
    when its header or index is wrong, 1 + t for the first malformed tile t
    (jpegr.h).  Asynchronous: no read-back."""
    import torch
    nt = nimg * tiles(w, h)
    if ent is None:
        ent = Entropy(nt, device=d_stream.device)
    elif ent.ntiles != nt:
        raise ValueError("ent does not hold nimg * tiles(w, h) tiles")
    _check_in_len(d_stream, in_len)
    if d_result is None:
        d_result = torch.zeros(2, dtype=torch.int64, device=d_stream.device)
    scratch = _pack_scratch(scratch, nt, d_stream.device)
    _call("jpegr_unpack_device", d_stream, in_len, w, h, nimg, ent.bits, ent.meta, ent.table, scratch,
          d_result, stream_arg(stream))
    return ent, d_result


def _header_ints(name, header_bytes, count):
    """The `count` ints the C function `name` reads out of a stream's first 16 bytes."""
    hdr = bytes(header_bytes[:16])
    if len(hdr) < 16:
        raise ValueError("a JPR header is 16 bytes")
    out = [ctypes.c_int() for _ in range(count)]
    _call(name, hdr, *(ctypes.byref(v) for v in out))
    return [v.value for v in out]


# two C functions, so two bodies: each error names the one that judged the header
def stream_info(header_bytes):
    """(w, h, nimg) of a JPR stream's first 16 bytes; JpegError on a wrong
    magic or a zero dimension."""
    w, h, n = _header_ints("jpegr_stream_info", header_bytes, 3)
    return w, h, n


def stream_format(header_bytes):
    """(w, h, nimg, tight) of the first 16 bytes of a JPR1 (tight False) or
    JPT1 (tight True) stream; JpegError on any other magic or a zero
    dimension."""
    w, h, n, fmt = _header_ints("jpegr_stream_format", header_bytes, 4)
    return w, h, n, fmt == STREAM_JPT1


def decode_stream_device(d_stream, in_len, w, h, nimg=1, tile0=0, ntiles=None, d_coef=None,
                         d_result=None, scratch=None, stream=None):
    """Tiles [tile0, tile0 + ntiles) of a JPR1 or JPT1 stream's first in_len bytes
    straight to coefficients (jpegr_stream_decode_device: no slots; ntiles
    None = up to the stream's last tile).  Returns (d_coef, d_result): d_coef
    int16, 128 per selected tile; d_result three int64 on the device, [0] the
    length the header and index imply, [1] -1 (all ones) when consistent, 0 on
    a wrong header or index, 1 + t for the first malformed tile t of the
    range, [2] the range's rejected entropy streams (jpegr.h).  Asynchronous:
    no read-back."""
    import torch
    nt = nimg * tiles(w, h)
    if ntiles is None:
        ntiles = nt - tile0
    _check_in_len(d_stream, in_len)
    if tile0 < 0 or ntiles <= 0 or tile0 + ntiles > nt:
        raise ValueError("tile range outside the stream")
    dev = d_stream.device
    d_coef = _buffer(d_coef, ntiles * 128, torch.int16, dev, "d_coef smaller than ntiles * 128 int16",
                     in_bytes=True)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    scratch = _pack_scratch(scratch, nt, dev)
    _call("jpegr_stream_decode_device", d_stream, in_len, w, h, nimg, tile0, ntiles, d_coef, scratch,
          d_result, stream_arg(stream))
    return d_coef, d_result


def decompress_images_device(d_stream, first=0, count=None):
    """Images [first, first + count) of a JPR1 or JPT1 stream (uint8 tensor, exactly
    the stream; count None = up to the last) -> (rgba uint8 tensor, w, h,
    count): reads the 16 header bytes back, decodes the images' tile range
    straight from the stream and reconstructs it (every tile decoded, as
    decompress_device).  The other images are not touched.  Raises JpegError
    on an inconsistent stream (d_result[1] != ~0) or a rejected entropy stream
    (d_result[2] != 0)."""
    w, h, nimg, _ = _open_stream(d_stream, "decompress_images_device")
    count = _image_count(first, count, nimg)
    per = tiles(w, h)
    d_coef, d_result = decode_stream_device(d_stream, d_stream.numel(), w, h, nimg, first * per,
                                            count * per)
    out = reconstruct_device(d_coef, w, h, count)
    _raise_on_verdict("decompress_images_device", d_result.cpu().tolist())
    return out, w, h, count


# -- random access ------------------------------------------------------------
def stream_index_device(d_stream, in_len, w, h, nimg=1, d_offsets=None, d_result=None, scratch=None,
                        stream=None):
    """The tile offsets of a JPR1 or JPT1 stream's first in_len bytes
    (jpegr_stream_index_device), what crop_device takes.  Returns (d_offsets,
    d_result): d_offsets int64, nimg * tiles(w, h) + 1 entries, entry t the
    byte offset of tile t's record and the last one the length the header and
    index imply; d_result two int64 on the device, [0] that length, [1] -1 (all
    ones) when the header is these dimensions' and the length is in_len, else
    0.  Asynchronous: no read-back."""
    import torch
    nt = nimg * tiles(w, h)
    _check_in_len(d_stream, in_len)
    dev = d_stream.device
    if d_offsets is None:
        d_offsets = torch.empty(nt + 1, dtype=torch.int64, device=dev)
    _check_offsets(d_offsets, nt)
    d_result = _buffer(d_result, 2, torch.int64, dev)
    scratch = _pack_scratch(scratch, nt, dev)
    _call("jpegr_stream_index_device", d_stream, in_len, w, h, nimg, d_offsets, scratch, d_result,
          stream_arg(stream))
    return d_offsets, d_result


def crop_items(max_w, max_h):
    """Items a crop occupies in a call with these maxima (jpegr_crop_items)."""
    return int(_lib.call("jpegr_crop_items", max_w, max_h))


def crop_scratch_bytes(nrects, max_w, max_h):
    return int(_lib.call("jpegr_crop_scratch_bytes", nrects, max_w, max_h))


def crop_device(d_stream, in_len, w, h, nimg, d_offsets, d_image, d_x, d_y, d_w, d_h, max_w, max_h,
                d_dst=None, d_out=None, out_cap=None, scratch=None, d_result=None, stream=None,
                check=True):
    """Many rectangles of a stream's images in one call (jpegr_crop_device):
    crop r delivers pixels [d_x[r], d_x[r] + d_w[r]) x [d_y[r], d_y[r] + d_h[r])
    of image d_image[r] as RGBA8 rows to d_out[d_dst[r] ...], each decoded from
    the tiles it touches only.  d_image .. d_h, d_dst: int64 tensors on the
    device; d_offsets: stream_index_device's; no d_w may exceed max_w, no d_h
    max_h (group crops of similar size per call: every crop occupies
    crop_items(max_w, max_h) items).  d_dst=None packs the crops back to back
    at 4 w h bytes each; d_out=None allocates out_cap bytes (default: the
    crops' furthest end, read back once; nrects * 4 max_w max_h with
    check=False).  Returns (d_out, d_dst, delivered); raises JpegError naming
    the first bad rectangle.  check=False does no read-back and returns None
    for the count."""
    import torch
    nrects = d_x.numel()
    if d_dst is None:
        d_len = 4 * d_w * d_h
        d_dst = torch.cumsum(d_len, 0) - d_len
    if out_cap is None:
        if d_out is not None:
            out_cap = d_out.numel()
        elif check and nrects:
            out_cap = int((d_dst + 4 * d_w * d_h).max().item())
        else:
            out_cap = nrects * 4 * max_w * max_h
    dev = d_stream.device
    d_out = _buffer(d_out, out_cap, torch.uint8, dev, floor=4)
    if nrects == 0:
        return d_out, d_dst, (0 if check else None)
    _check_in_len(d_stream, in_len)
    _check_offsets(d_offsets, nimg * tiles(w, h))
    d_rects = torch.stack((d_image, d_x, d_y, d_w, d_h, d_dst), dim=1).contiguous()
    scratch = _buffer(scratch, crop_scratch_bytes(nrects, max_w, max_h), torch.uint8, dev,
                      "scratch smaller than crop_scratch_bytes(nrects, max_w, max_h)", floor=16)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    _call("jpegr_crop_device", d_stream, in_len, w, h, nimg, d_offsets, d_rects, nrects, max_w, max_h,
          d_out, out_cap, scratch, d_result, stream_arg(stream))
    if not check:
        return d_out, d_dst, None
    n = _lib.batch_verdict(d_result, stream, JpegError, -1, "jpegr_crop_device: rectangle")
    return d_out, d_dst, n


# jpegr.h's JPEGR_LAYOUT_* by name
_LAYOUTS = {"chw": 0, "hwc": 1}


def _tensor_dtype(dtype):
    """(the torch dtype, jpegr.h's JPEGR_DTYPE_* of it); None is float32."""
    import torch
    codes = {torch.uint8: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in codes:
        raise ValueError("dtype is none of torch.uint8, float32, float16 and bfloat16")
    return dtype, codes[dtype]


def _three(v, name):
    """One value or three as a list of three Python floats."""
    try:
        vals = [float(x) for x in v]
    except TypeError:
        vals = [float(v)]
    if len(vals) == 1:
        vals = vals * 3
    if len(vals) != 3:
        raise ValueError(f"{name} is one float or three")
    return vals


def _float3(v, name):
    """None (NULL), or the call's three floats: each rounded once to float32."""
    return None if v is None else (ctypes.c_float * 3)(*_three(v, name))


def normalisation(mean=None, std=None):
    """(scale, bias), three float32 values each as Python floats, such that
    fl32(fl32(v * scale) + bias) normalises a byte v: scale = 1 / (255 std) and
    bias = -mean / std, computed in Python floats and rounded once to float32;
    None is a mean of 0 and a std of 1.  mean, std: one float or three."""
    mean = [0.0] * 3 if mean is None else _three(mean, "mean")
    std = [1.0] * 3 if std is None else _three(std, "std")
    return ([float(np.float32(1.0 / (255.0 * s))) for s in std],
            [float(np.float32(0.0 - m / s)) for m, s in zip(mean, std)])


def crop_tensor_device(d_stream, in_len, w, h, nimg, d_offsets, d_image, d_x, d_y, d_w, d_h, max_w, max_h,
                       d_dst=None, d_out=None, out_cap=None, scratch=None, d_result=None, stream=None,
                       check=True, dtype=None, layout="chw", scale=None, bias=None, d_flip=None):
    """crop_device's rectangles as what a model reads, in one call
    (jpegr_crop_tensor_device): three channels (alpha dropped) of `dtype`
    (torch.float32, the default, float16, bfloat16 or uint8), planar
    (layout="chw": [3, h, w] a crop) or interleaved ("hwc": [h, w, 3]).  Channel
    c of a pixel's byte v becomes fl32(fl32(v * scale[c]) + bias[c]), two
    rounded float32 operations -- what x.float().mul(scale).add(bias) gives --
    then rounded to nearest-even to `dtype`; uint8 delivers v and ignores both.
    scale, bias: one float or three, None for 1 and 0.  d_flip: None, or a bool
    or uint8 tensor with an entry per crop, nonzero to mirror that crop
    horizontally.  The other arguments are crop_device's, with d_dst and
    out_cap counting elements of `dtype` in d_out (a tensor of that dtype): a
    crop takes 3 w h of them, and d_dst=None packs the crops back to back.
    Returns (d_out, d_dst, delivered); raises JpegError naming the first bad
    rectangle; check=False does no read-back and returns None for the count."""
    import torch
    dtype, code = _tensor_dtype(dtype)
    if layout not in _LAYOUTS:
        raise ValueError('layout is "chw" or "hwc"')
    scale3, bias3 = _float3(scale, "scale"), _float3(bias, "bias")
    nrects = d_x.numel()
    if d_flip is not None and (d_flip.dtype not in (torch.bool, torch.uint8) or d_flip.numel() != nrects):
        raise ValueError("d_flip is a bool or uint8 tensor with one entry per crop")
    if d_out is not None and d_out.dtype != dtype:
        raise ValueError("d_out is not of the requested dtype")
    if d_dst is None:
        d_len = 3 * d_w * d_h
        d_dst = torch.cumsum(d_len, 0) - d_len
    if out_cap is None:
        if d_out is not None:
            out_cap = d_out.numel()
        elif check and nrects:
            out_cap = int((d_dst + 3 * d_w * d_h).max().item())
        else:
            out_cap = nrects * 3 * max_w * max_h
    dev = d_stream.device
    d_out = _buffer(d_out, out_cap, dtype, dev, "d_out smaller than out_cap elements", floor=4)
    if nrects == 0:
        return d_out, d_dst, (0 if check else None)
    _check_in_len(d_stream, in_len)
    _check_offsets(d_offsets, nimg * tiles(w, h))
    d_rects = torch.stack((d_image, d_x, d_y, d_w, d_h, d_dst), dim=1).contiguous()
    scratch = _buffer(scratch, crop_scratch_bytes(nrects, max_w, max_h), torch.uint8, dev,
                      "scratch smaller than crop_scratch_bytes(nrects, max_w, max_h)", floor=16)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    _call("jpegr_crop_tensor_device", d_stream, in_len, w, h, nimg, d_offsets, d_rects, nrects, d_flip,
          max_w, max_h, code, _LAYOUTS[layout], scale3, bias3, d_out, out_cap, scratch, d_result,
          stream_arg(stream))
    if not check:
        return d_out, d_dst, None
    n = _lib.batch_verdict(d_result, stream, JpegError, -1, "jpegr_crop_tensor_device: rectangle")
    return d_out, d_dst, n


def crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h):
    return int(_lib.call("jpegr_crop_resize_scratch_bytes", nrects, max_w, max_h, out_w, out_h))


def crop_resize_device(d_stream, in_len, w, h, nimg, d_offsets, d_image, d_x, d_y, d_w, d_h, max_w, max_h,
                       out_w, out_h, antialias=True, d_dst=None, d_out=None, out_cap=None, scratch=None,
                       d_result=None, stream=None, check=True, dtype=None, layout="chw", scale=None,
                       bias=None, d_flip=None):
    """crop_tensor_device's rectangles, each of its own size, resampled to
    out_w x out_h in the same call (jpegr_crop_resize_device): the half-pixel
    bilinear of interpolate(mode="bilinear", align_corners=False), with
    antialias=True (the default, JPEGR_FILTER_TRIANGLE) widening the filter by
    the scale when a rectangle is larger than the output; include/jpegr.h
    states the arithmetic, which numpy reproduces bit for bit.  The resampled
    value is normalised without being rounded to a byte first; uint8 rounds it
    to nearest-even.  d_flip mirrors the output.  A crop takes 3 out_w out_h
    elements of `dtype`, d_dst=None packs them back to back, and a rectangle
    with w or h of 0 is bad.  The scratch is crop_resize_scratch_bytes(nrects,
    max_w, max_h, out_w, out_h) bytes.  Everything else, the returns and
    check=False included, is crop_tensor_device's."""
    import torch
    dtype, code = _tensor_dtype(dtype)
    if layout not in _LAYOUTS:
        raise ValueError('layout is "chw" or "hwc"')
    if not (isinstance(out_w, int) and isinstance(out_h, int) and out_w > 0 and out_h > 0):
        raise ValueError("out_w and out_h are positive ints")
    scale3, bias3 = _float3(scale, "scale"), _float3(bias, "bias")
    nrects = d_x.numel()
    if d_flip is not None and (d_flip.dtype not in (torch.bool, torch.uint8) or d_flip.numel() != nrects):
        raise ValueError("d_flip is a bool or uint8 tensor with one entry per crop")
    if d_out is not None and d_out.dtype != dtype:
        raise ValueError("d_out is not of the requested dtype")
    per = 3 * out_w * out_h
    dev = d_stream.device
    if d_dst is None:
        d_dst = torch.arange(nrects, dtype=torch.int64, device=d_x.device) * per
    if out_cap is None:
        out_cap = d_out.numel() if d_out is not None else nrects * per
    d_out = _buffer(d_out, out_cap, dtype, dev, "d_out smaller than out_cap elements", floor=4)
    if nrects == 0:
        return d_out, d_dst, (0 if check else None)
    _check_in_len(d_stream, in_len)
    _check_offsets(d_offsets, nimg * tiles(w, h))
    d_rects = torch.stack((d_image, d_x, d_y, d_w, d_h, d_dst), dim=1).contiguous()
    scratch = _buffer(scratch, crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h), torch.uint8,
                      dev, "scratch smaller than crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h)",
                      floor=16)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    _call("jpegr_crop_resize_device", d_stream, in_len, w, h, nimg, d_offsets, d_rects, nrects, d_flip,
          max_w, max_h, out_w, out_h, 1 if antialias else 0, code, _LAYOUTS[layout], scale3, bias3, d_out,
          out_cap, scratch, d_result, stream_arg(stream))
    if not check:
        return d_out, d_dst, None
    n = _lib.batch_verdict(d_result, stream, JpegError, -1, "jpegr_crop_resize_device: rectangle")
    return d_out, d_dst, n


# -- crops from many streams ------------------------------------------------------
STREAM_DESC_BYTES = 48                    # sizeof(jpegr_stream_desc)


def stream_table(rows):
    """jpegr_stream_desc's bytes on the host: rows of (d_in, in_len,
    d_tile_offsets, image0, w, h, nimg) -- the two pointers as addresses -- to a
    uint64 array [n, 6]: the four 8-B fields, then w | h << 32 and nimg (the
    reserved word 0)."""
    rows = [tuple(int(v) for v in r) for r in rows]
    if any(len(r) != 7 for r in rows):
        raise ValueError("a row is (d_in, in_len, d_tile_offsets, image0, w, h, nimg)")
    if any(not 0 <= v < 1 << 32 for r in rows for v in r[4:]):
        raise ValueError("w, h and nimg are 32-bit")
    table = np.array([[p, n, o, i0, w | h << 32, nimg] for p, n, o, i0, w, h, nimg in rows], np.uint64)
    return table.reshape(len(rows), 6)


def dataset_crop_scratch_bytes(nrects, max_w, max_h):
    return int(_lib.call("jpegr_dataset_crop_scratch_bytes", nrects, max_w, max_h))


def dataset_crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h):
    return int(_lib.call("jpegr_dataset_crop_resize_scratch_bytes", nrects, max_w, max_h, out_w, out_h))


def _check_table(d_streams, nstreams):
    if nstreams <= 0 or d_streams.numel() * d_streams.element_size() < nstreams * STREAM_DESC_BYTES:
        raise ValueError("d_streams smaller than nstreams descriptors, or none")


def dataset_crop_tensor_device(d_streams, nstreams, d_image, d_x, d_y, d_w, d_h, max_w, max_h, d_dst=None,
                               d_out=None, out_cap=None, scratch=None, d_result=None, stream=None,
                               check=True, dtype=None, layout="chw", scale=None, bias=None, d_flip=None):
    """crop_tensor_device over many streams in one call
    (jpegr_dataset_crop_tensor_device): d_streams is a device tensor holding
    nstreams jpegr_stream_desc (stream_table's rows; the streams and offsets
    they point to are the caller's to keep alive), d_image a dataset-wide image
    index, and every rectangle is judged against its own stream's size.  max_w
    and max_h bound the rectangles only.  The scratch is
    dataset_crop_scratch_bytes(nrects, max_w, max_h) bytes.  Everything else,
    the returns and check=False included, is crop_tensor_device's."""
    import torch
    dtype, code = _tensor_dtype(dtype)
    if layout not in _LAYOUTS:
        raise ValueError('layout is "chw" or "hwc"')
    scale3, bias3 = _float3(scale, "scale"), _float3(bias, "bias")
    nrects = d_x.numel()
    if d_flip is not None and (d_flip.dtype not in (torch.bool, torch.uint8) or d_flip.numel() != nrects):
        raise ValueError("d_flip is a bool or uint8 tensor with one entry per crop")
    if d_out is not None and d_out.dtype != dtype:
        raise ValueError("d_out is not of the requested dtype")
    if d_dst is None:
        d_len = 3 * d_w * d_h
        d_dst = torch.cumsum(d_len, 0) - d_len
    if out_cap is None:
        if d_out is not None:
            out_cap = d_out.numel()
        elif check and nrects:
            out_cap = int((d_dst + 3 * d_w * d_h).max().item())
        else:
            out_cap = nrects * 3 * max_w * max_h
    dev = d_streams.device
    d_out = _buffer(d_out, out_cap, dtype, dev, "d_out smaller than out_cap elements", floor=4)
    if nrects == 0:
        return d_out, d_dst, (0 if check else None)
    _check_table(d_streams, nstreams)
    d_rects = torch.stack((d_image, d_x, d_y, d_w, d_h, d_dst), dim=1).contiguous()
    scratch = _buffer(scratch, dataset_crop_scratch_bytes(nrects, max_w, max_h), torch.uint8, dev,
                      "scratch smaller than dataset_crop_scratch_bytes(nrects, max_w, max_h)", floor=16)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    _call("jpegr_dataset_crop_tensor_device", d_streams, nstreams, d_rects, nrects, d_flip, max_w, max_h,
          code, _LAYOUTS[layout], scale3, bias3, d_out, out_cap, scratch, d_result, stream_arg(stream))
    if not check:
        return d_out, d_dst, None
    n = _lib.batch_verdict(d_result, stream, JpegError, -1, "jpegr_dataset_crop_tensor_device: rectangle")
    return d_out, d_dst, n


def dataset_crop_resize_device(d_streams, nstreams, d_image, d_x, d_y, d_w, d_h, max_w, max_h, out_w, out_h,
                               antialias=True, d_dst=None, d_out=None, out_cap=None, scratch=None,
                               d_result=None, stream=None, check=True, dtype=None, layout="chw", scale=None,
                               bias=None, d_flip=None):
    """crop_resize_device over many streams in one call
    (jpegr_dataset_crop_resize_device): d_streams, nstreams and d_image as for
    dataset_crop_tensor_device; the scratch is
    dataset_crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h)
    bytes.  Everything else is crop_resize_device's."""
    import torch
    dtype, code = _tensor_dtype(dtype)
    if layout not in _LAYOUTS:
        raise ValueError('layout is "chw" or "hwc"')
    if not (isinstance(out_w, int) and isinstance(out_h, int) and out_w > 0 and out_h > 0):
        raise ValueError("out_w and out_h are positive ints")
    scale3, bias3 = _float3(scale, "scale"), _float3(bias, "bias")
    nrects = d_x.numel()
    if d_flip is not None and (d_flip.dtype not in (torch.bool, torch.uint8) or d_flip.numel() != nrects):
        raise ValueError("d_flip is a bool or uint8 tensor with one entry per crop")
    if d_out is not None and d_out.dtype != dtype:
        raise ValueError("d_out is not of the requested dtype")
    per = 3 * out_w * out_h
    dev = d_streams.device
    if d_dst is None:
        d_dst = torch.arange(nrects, dtype=torch.int64, device=d_x.device) * per
    if out_cap is None:
        out_cap = d_out.numel() if d_out is not None else nrects * per
    d_out = _buffer(d_out, out_cap, dtype, dev, "d_out smaller than out_cap elements", floor=4)
    if nrects == 0:
        return d_out, d_dst, (0 if check else None)
    _check_table(d_streams, nstreams)
    d_rects = torch.stack((d_image, d_x, d_y, d_w, d_h, d_dst), dim=1).contiguous()
    scratch = _buffer(scratch, dataset_crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h),
                      torch.uint8, dev,
                      "scratch smaller than dataset_crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h)",
                      floor=16)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    _call("jpegr_dataset_crop_resize_device", d_streams, nstreams, d_rects, nrects, d_flip, max_w, max_h,
          out_w, out_h, 1 if antialias else 0, code, _LAYOUTS[layout], scale3, bias3, d_out, out_cap, scratch,
          d_result, stream_arg(stream))
    if not check:
        return d_out, d_dst, None
    n = _lib.batch_verdict(d_result, stream, JpegError, -1, "jpegr_dataset_crop_resize_device: rectangle")
    return d_out, d_dst, n


# -- thumbnails -----------------------------------------------------------------
def thumb_device(d_stream, in_len, w, h, nimg, first=0, count=None, d_offsets=None, d_out=None,
                 d_dc=None, want_dc=False, scratch=None, d_result=None, stream=None):
    """Images [first, first + count) of a JPR1 or JPT1 stream's first in_len
    bytes at 1/8 scale, one RGBA8 pixel per tile, from the DC terms alone
    (jpegr_thumb_device; count None = up to the last image).  d_offsets:
    stream_index_device's offsets, which spare the call its own index scan (and
    its scratch); None: the call scans.  d_out: uint8, count * tiles(w, h) * 4
    bytes (allocated when None); d_dc: int16, four per tile {Y, Cr, Cb, 0}, the
    DC terms themselves (allocated when None and want_dc; else not written).
    Returns (d_out, d_dc, d_result): d_result three int64 on the
    device, [0] the implied length, [1] -1 (all ones) when consistent, 0 on a
    wrong header or index, 1 + t for the first malformed tile t of the range,
    [2] the streams rejected inside the prefix examined (jpegr.h).
    Asynchronous: no read-back."""
    import torch
    count = _image_count(first, count, nimg)
    _check_in_len(d_stream, in_len)
    nt, n = nimg * tiles(w, h), count * tiles(w, h)
    dev = d_stream.device
    if d_offsets is not None:
        _check_offsets(d_offsets, nt)
    if d_dc is not None or want_dc:
        d_dc = _buffer(d_dc, n * 4, torch.int16, dev, "d_dc smaller than four int16 per tile",
                       in_bytes=True)
    d_out = _buffer(d_out, n * 4, torch.uint8, dev, "d_out smaller than four bytes per tile",
                    in_bytes=True)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    if d_offsets is None:
        scratch = _pack_scratch(scratch, nt, dev)
    _call("jpegr_thumb_device", d_stream, in_len, w, h, nimg, d_offsets, first, count, d_out, d_dc,
          scratch, d_result, stream_arg(stream))
    return d_out, d_dc, d_result


def _thumbnails(d_stream, w, h, nimg, first, count, d_offsets):
    if count is None:
        count = nimg - first
    d_out, _, d_result = thumb_device(d_stream, d_stream.numel(), w, h, nimg, first, count,
                                      d_offsets=d_offsets)
    _raise_on_verdict("thumbnails", d_result.cpu().tolist())
    return d_out.view(count, (h + 7) // 8, (w + 7) // 8, 4), w, h, count


def thumbnails_device(d_stream, first=0, count=None):
    """1/8-scale thumbnails of images [first, first + count) of a JPR1 or JPT1
    stream (uint8 tensor, exactly the stream; count None = up to the last) ->
    (uint8 tensor [count, ceil(h / 8), ceil(w / 8), 4], w, h, count): pixel
    (tx, ty) is pixel (8 tx, 8 ty) of the image reconstructed from its DC terms
    alone.  Reads the 16 header bytes back, then the result words; the other
    images are not touched.  Raises JpegError on an inconsistent stream
    (d_result[1] != ~0) or a stream rejected before its DC (d_result[2] != 0),
    as decompress_images_device does."""
    w, h, nimg, _ = _open_stream(d_stream, "thumbnails_device")
    return _thumbnails(d_stream, w, h, nimg, first, count, None)


# -- editing a stream without decoding it ------------------------------------------
def select_scratch_bytes(nitems, out_w, out_h):
    return int(_lib.call("jpegr_select_scratch_bytes", nitems, out_w, out_h))


def _format_arg(tight):
    return 0 if tight is None else STREAM_JPT1 if tight else STREAM_JPR1


def select_device(d_stream, in_len, w, h, nimg, d_offsets, d_image, d_x, d_y, out_w, out_h, tight=None,
                  d_out=None, d_len=None, scratch=None, d_result=None, stream=None, cap=None):
    """A new stream of d_image.numel() images of out_w x out_h from tiles of
    a JPR1 or JPT1 stream's first in_len bytes, nothing decoded
    (jpegr_select_device): image k is the tile grid of source image d_image[k]
    that starts at pixel (d_x[k], d_y[k]), both multiples of 8.  d_image, d_x,
    d_y: int64 tensors on the device; d_offsets: stream_index_device's.
    tight: None keeps the source's format, False writes JPR1, True JPT1.
    Returns (d_out, d_len, d_result): d_out a uint8 tensor (pack_bound(out_w,
    out_h, nitems) bytes when not given), d_len one int64 holding the stream
    length -- or the capacity needed when that exceeds d_out's size (or `cap`,
    a smaller capacity to write within), in which case nothing past it is
    written -- and d_result three int64, [0] the
    length again, [1] -1 (all ones) or 1 + the first bad item, [2] the tiles
    of good items written as the empty record (jpegr.h).  Asynchronous: no
    read-back."""
    import torch
    nitems = d_image.numel()
    if nitems == 0 or d_x.numel() != nitems or d_y.numel() != nitems:
        raise ValueError("d_image, d_x and d_y hold one entry per item, and at least one")
    _check_in_len(d_stream, in_len)
    _check_offsets(d_offsets, nimg * tiles(w, h))
    dev = d_stream.device
    d_items = torch.stack((d_image, d_x, d_y), dim=1).contiguous()
    if d_out is None:
        d_out = torch.empty(pack_bound(out_w, out_h, nitems), dtype=torch.uint8, device=dev)
    if cap is None:
        cap = d_out.numel()
    elif cap > d_out.numel():
        raise ValueError("cap past the end of d_out")
    if d_len is None:
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    d_result = _buffer(d_result, 3, torch.int64, dev)
    scratch = _buffer(scratch, select_scratch_bytes(nitems, out_w, out_h), torch.uint8, dev,
                      "scratch smaller than select_scratch_bytes(nitems, out_w, out_h)", floor=16)
    _call("jpegr_select_device", d_stream, in_len, w, h, nimg, d_offsets, d_items, nitems, out_w,
          out_h, _format_arg(tight), d_out, cap, d_len, scratch, d_result, stream_arg(stream))
    return d_out, d_len, d_result


def concat_streams(streams):
    """Streams (uint8 device tensors, each exactly a stream) of one w, h and
    format joined into one: a new header with the sum of the image counts, the
    indexes back to back, then the records back to back, by device copies.
    Reads each 16-B header back.  Raises JpegError when w, h or the format
    differ or a stream is shorter than its header and index."""
    import torch
    streams = list(streams)
    if not streams:
        raise ValueError("no streams")
    heads = []
    for d in streams:
        heads.append(_open_stream(d, "concat_streams"))
    w, h, _, tight = heads[0]
    if any((hw, hh, ht) != (w, h, tight) for hw, hh, _, ht in heads):
        raise JpegError(-1, "concat_streams: the streams differ in w, h or format")
    nts = [n * tiles(w, h) for _, _, n, _ in heads]
    if any(d.numel() < 16 + 2 * nt for d, nt in zip(streams, nts)):
        raise JpegError(-1, "concat_streams: shorter than its index")
    nimg = sum(n for _, _, n, _ in heads)
    if nimg > 0x7FFFFFFF:
        raise JpegError(-1, "concat_streams: too many images")
    total = 16 + sum(d.numel() - 16 for d in streams)
    out = torch.empty(total, dtype=torch.uint8, device=streams[0].device)
    head = (b"JPT1" if tight else b"JPR1") + b"".join(int(v).to_bytes(4, "little") for v in (w, h, nimg))
    out[:16].copy_(torch.frombuffer(bytearray(head), dtype=torch.uint8))
    pos = 16
    for d, nt in zip(streams, nts):
        out[pos:pos + 2 * nt].copy_(d[16:16 + 2 * nt])
        pos += 2 * nt
    for d, nt in zip(streams, nts):
        n = d.numel() - 16 - 2 * nt
        out[pos:pos + n].copy_(d[16 + 2 * nt:])
        pos += n
    return out


class StreamReader:
    """Random access into one JPR1 or JPT1 stream on the device (a uint8
    tensor, exactly the stream): the header is read back once and the index is
    built once (stream_index_device).  Raises JpegError on a stream whose
    header or index is inconsistent."""

    def __init__(self, d_stream):
        self.w, self.h, self.nimg, self.tight = _open_stream(d_stream, "StreamReader")
        self.d_stream = d_stream
        self.length = d_stream.numel()
        self.d_offsets, d_result = stream_index_device(d_stream, self.length, self.w, self.h,
                                                       self.nimg)
        # the index call has no third word: only the verdict is read back
        _raise_on_verdict("StreamReader", (None, int(d_result[1].item()), 0))

    def crop(self, image, x, y, w, h):
        """Pixels [x, x + w) x [y, y + h) of image `image`: a uint8 tensor (h, w, 4)."""
        import torch
        dev = self.d_stream.device
        if w == 0 or h == 0:
            return torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        one = [torch.tensor([v], dtype=torch.int64, device=dev) for v in (image, x, y, w, h)]
        d_out, _, _ = self.crops(*one, min(w, self.w), min(h, self.h), out_cap=4 * w * h)
        return d_out[:4 * w * h].view(h, w, 4)

    def crops(self, d_image, d_x, d_y, d_w, d_h, max_w, max_h, **kw):
        """crop_device on this stream: (d_out, d_dst, delivered)."""
        return crop_device(self.d_stream, self.length, self.w, self.h, self.nimg, self.d_offsets,
                           d_image, d_x, d_y, d_w, d_h, max_w, max_h, **kw)

    def crops_tensor(self, d_image, d_x, d_y, d_w, d_h, max_w, max_h, **kw):
        """crop_tensor_device on this stream: (d_out, d_dst, delivered)."""
        return crop_tensor_device(self.d_stream, self.length, self.w, self.h, self.nimg, self.d_offsets,
                                  d_image, d_x, d_y, d_w, d_h, max_w, max_h, **kw)

    def crop_batch(self, d_image, d_x, d_y, w, h, dtype=None, layout="chw", mean=None, std=None,
                   d_flip=None):
        """n crops of w x h pixels, crop r from (d_x[r], d_y[r]) of image
        d_image[r], as one normalised tensor of `dtype` (default float32):
        [n, 3, h, w] with layout="chw", [n, h, w, 3] with "hwc"; d_flip as for
        crop_tensor_device.  Channel c of a pixel's byte v becomes
        fl32(fl32(v * scale[c]) + bias[c]) with scale = 1 / (255 std) and
        bias = -mean / std (normalisation(): computed in Python floats, rounded
        once to float32), two rounded float32 operations, then rounded to
        `dtype`.  mean and std of None: scale 1 / 255 and bias 0.  This is not
        bit-identical to ToTensor followed by Normalize, which divide (by 255,
        then by std) where this multiplies."""
        import torch
        dtype, _ = _tensor_dtype(dtype)
        if layout not in _LAYOUTS:
            raise ValueError('layout is "chw" or "hwc"')
        scale, bias = normalisation(mean, std)
        n, dev = d_x.numel(), self.d_stream.device
        shape = (n, 3, h, w) if layout == "chw" else (n, h, w, 3)
        d_out = torch.empty(n * 3 * w * h, dtype=dtype, device=dev)
        if n and w and h:
            d_dst = torch.arange(n, dtype=torch.int64, device=dev) * (3 * w * h)
            self.crops_tensor(d_image, d_x, d_y, torch.full_like(d_x, w), torch.full_like(d_x, h), w, h,
                              d_dst=d_dst, d_out=d_out, out_cap=d_out.numel(), dtype=dtype,
                              layout=layout, scale=scale, bias=bias, d_flip=d_flip)
        return d_out.view(shape)

    def crops_resized(self, d_image, d_x, d_y, d_w, d_h, max_w, max_h, out_w, out_h, **kw):
        """crop_resize_device on this stream: (d_out, d_dst, delivered)."""
        return crop_resize_device(self.d_stream, self.length, self.w, self.h, self.nimg, self.d_offsets,
                                  d_image, d_x, d_y, d_w, d_h, max_w, max_h, out_w, out_h, **kw)

    def resized_crop_batch(self, d_image, d_x, d_y, d_w, d_h, out_w, out_h, antialias=True, dtype=None,
                           layout="chw", mean=None, std=None, d_flip=None, max_w=None, max_h=None):
        """RandomResizedCrop's batch in one call: crop r is the d_w[r] x d_h[r]
        pixels from (d_x[r], d_y[r]) of image d_image[r], resampled to
        out_w x out_h (crop_resize_device: bilinear, antialiased by default),
        normalised as crop_batch normalises and mirrored where d_flip[r] is
        not 0.  Returns [n, 3, out_h, out_w] with layout="chw" and
        [n, out_h, out_w, 3] with "hwc", of `dtype` (default float32).
        max_w, max_h: bounds on d_w and d_h; the scratch grows with them.  A
        None costs one read-back, of d_w.max() or d_h.max(), which waits for
        the device; pass both to keep the call asynchronous apart from its
        verdict.  No crops: an empty tensor of that shape, without a call."""
        import torch
        dtype, _ = _tensor_dtype(dtype)
        if layout not in _LAYOUTS:
            raise ValueError('layout is "chw" or "hwc"')
        if not (isinstance(out_w, int) and isinstance(out_h, int) and out_w > 0 and out_h > 0):
            raise ValueError("out_w and out_h are positive ints")
        scale, bias = normalisation(mean, std)
        n = d_x.numel()
        shape = (n, 3, out_h, out_w) if layout == "chw" else (n, out_h, out_w, 3)
        d_out = torch.empty(n * 3 * out_w * out_h, dtype=dtype, device=self.d_stream.device)
        if n:
            max_w = int(d_w.max().item()) if max_w is None else max_w
            max_h = int(d_h.max().item()) if max_h is None else max_h
            self.crops_resized(d_image, d_x, d_y, d_w, d_h, max_w, max_h, out_w, out_h, antialias=antialias,
                               d_out=d_out, out_cap=d_out.numel(), dtype=dtype, layout=layout, scale=scale,
                               bias=bias, d_flip=d_flip)
        return d_out.view(shape)

    def thumbnails(self, first=0, count=None):
        """thumbnails_device on this stream, through the kept offsets: (uint8
        tensor [count, ceil(h / 8), ceil(w / 8), 4], w, h, count)."""
        return _thumbnails(self.d_stream, self.w, self.h, self.nimg, first, count, self.d_offsets)

    def select(self, images=None, x=0, y=0, w=None, h=None, tight=None):
        """A uint8 tensor of exactly the new stream whose image k is the w x h
        tile window of image images[k] at pixel (x, y) -- ints, or one per
        item; both multiples of 8 -- with nothing decoded (select_device).
        images None: every image in order; w, h None: the source's; tight
        None: the source's format, False JPR1, True JPT1.  Reads the length
        back once and runs once more at the needed capacity when the first
        guess was short.  Raises JpegError on a bad item (d_result[1] != ~0)
        or a tile written as the empty record (d_result[2] != 0)."""
        import torch
        dev = self.d_stream.device
        images = list(range(self.nimg)) if images is None else [int(i) for i in images]
        n = len(images)
        if n == 0:
            raise ValueError("no images selected")
        w = self.w if w is None else w
        h = self.h if h is None else h
        if not (0 < w <= self.w and 0 < h <= self.h):
            raise ValueError("the window is larger than the image, or empty")

        def col(v):
            v = [int(a) for a in v] if hasattr(v, "__iter__") else [int(v)] * n
            if len(v) != n:
                raise ValueError("x and y hold one entry per item")
            return torch.tensor(v, dtype=torch.int64, device=dev)

        cols = (torch.tensor(images, dtype=torch.int64, device=dev), col(x), col(y))
        nt_out, nt_in = n * tiles(w, h), self.nimg * tiles(self.w, self.h)
        # the source's mean record (a quarter more: JPR1 from JPT1 grows), never past the bound
        cap = min(pack_bound(w, h, n), 16 + 2 * nt_out + 1024 + (5 * self.length * nt_out) // (4 * nt_in))
        for _ in range(2):
            d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
            _, _, d_result = select_device(self.d_stream, self.length, self.w, self.h, self.nimg,
                                           self.d_offsets, *cols, w, h, tight=tight, d_out=d_out)
            need, bad, empty = (int(v) for v in d_result.cpu().tolist())
            if bad != -1:
                raise JpegError(-1, f"jpegr_select_device: item {bad - 1}")
            if empty != 0:
                raise JpegError(-1, f"jpegr_select_device: {empty} malformed tile records")
            if need <= cap:
                return d_out[:need].clone()
            cap = need
        raise JpegError(-1, "jpegr_select_device: the needed capacity changed between two calls")

    def transcode(self, tight):
        """The whole stream in the other (or the same) format: select of everything."""
        return self.select(tight=tight)


class Dataset:
    """Many streams read as one: StreamReaders of any sizes and either format,
    in the order given, their images numbered through -- image g of the
    dataset is image g - image0[s] of reader s.  Keeps the readers (and so their
    streams and offsets) alive and builds the table of jpegr_stream_desc on
    the device once.  image0: int64 array, each reader's first index; nimg: the
    total; sizes: int64 array [nimg, 2], every image's (w, h), on the host,
    for a sampler to draw rectangles from; max_w, max_h: the largest stream's
    width and height, the default bound on a rectangle."""

    def __init__(self, readers):
        import torch
        self.readers = list(readers)
        if not self.readers:
            raise ValueError("no readers")
        counts = np.array([rd.nimg for rd in self.readers], np.int64)
        self.image0 = np.cumsum(counts) - counts
        self.nimg = int(counts.sum())
        self.sizes = np.repeat(np.array([(rd.w, rd.h) for rd in self.readers], np.int64), counts, axis=0)
        self.max_w = max(rd.w for rd in self.readers)
        self.max_h = max(rd.h for rd in self.readers)
        self.table = stream_table((rd.d_stream.data_ptr(), rd.length, rd.d_offsets.data_ptr(), i0, rd.w, rd.h,
                                   rd.nimg) for rd, i0 in zip(self.readers, self.image0))
        self.device = self.readers[0].d_stream.device
        self.d_table = torch.from_numpy(self.table.view(np.int64)).to(self.device)

    def crops_tensor(self, d_image, d_x, d_y, d_w, d_h, max_w=None, max_h=None, **kw):
        """dataset_crop_tensor_device on these streams: (d_out, d_dst, delivered)."""
        return dataset_crop_tensor_device(self.d_table, len(self.readers), d_image, d_x, d_y, d_w, d_h,
                                          self.max_w if max_w is None else max_w,
                                          self.max_h if max_h is None else max_h, **kw)

    def crops_resized(self, d_image, d_x, d_y, d_w, d_h, out_w, out_h, max_w=None, max_h=None, **kw):
        """dataset_crop_resize_device on these streams: (d_out, d_dst, delivered)."""
        return dataset_crop_resize_device(self.d_table, len(self.readers), d_image, d_x, d_y, d_w, d_h,
                                          self.max_w if max_w is None else max_w,
                                          self.max_h if max_h is None else max_h, out_w, out_h, **kw)

    def crop_batch(self, d_image, d_x, d_y, w, h, dtype=None, layout="chw", mean=None, std=None,
                   d_flip=None):
        """StreamReader.crop_batch with a dataset-wide d_image: n crops of
        w x h pixels, each from its own stream, as one [n, 3, h, w] or
        [n, h, w, 3] tensor, in one call."""
        import torch
        dtype, _ = _tensor_dtype(dtype)
        if layout not in _LAYOUTS:
            raise ValueError('layout is "chw" or "hwc"')
        scale, bias = normalisation(mean, std)
        n = d_x.numel()
        shape = (n, 3, h, w) if layout == "chw" else (n, h, w, 3)
        d_out = torch.empty(n * 3 * w * h, dtype=dtype, device=self.device)
        if n and w and h:
            d_dst = torch.arange(n, dtype=torch.int64, device=self.device) * (3 * w * h)
            self.crops_tensor(d_image, d_x, d_y, torch.full_like(d_x, w), torch.full_like(d_x, h), w, h,
                              d_dst=d_dst, d_out=d_out, out_cap=d_out.numel(), dtype=dtype,
                              layout=layout, scale=scale, bias=bias, d_flip=d_flip)
        return d_out.view(shape)

    def resized_crop_batch(self, d_image, d_x, d_y, d_w, d_h, out_w, out_h, antialias=True, dtype=None,
                           layout="chw", mean=None, std=None, d_flip=None, max_w=None, max_h=None):
        """StreamReader.resized_crop_batch with a dataset-wide d_image:
        RandomResizedCrop's batch from images of many sizes in one call.
        max_w, max_h: bounds on d_w and d_h, by default the largest stream's
        size (no read-back; the scratch and the decode's idle items grow with
        them, so pass the sampler's own bounds where it has them)."""
        import torch
        dtype, _ = _tensor_dtype(dtype)
        if layout not in _LAYOUTS:
            raise ValueError('layout is "chw" or "hwc"')
        if not (isinstance(out_w, int) and isinstance(out_h, int) and out_w > 0 and out_h > 0):
            raise ValueError("out_w and out_h are positive ints")
        scale, bias = normalisation(mean, std)
        n = d_x.numel()
        shape = (n, 3, out_h, out_w) if layout == "chw" else (n, out_h, out_w, 3)
        d_out = torch.empty(n * 3 * out_w * out_h, dtype=dtype, device=self.device)
        if n:
            self.crops_resized(d_image, d_x, d_y, d_w, d_h, out_w, out_h, max_w=max_w, max_h=max_h,
                               antialias=antialias, d_out=d_out, out_cap=d_out.numel(), dtype=dtype,
                               layout=layout, scale=scale, bias=bias, d_flip=d_flip)
        return d_out.view(shape)


def stream_encode_scratch_bytes(ntiles, cap):
    return int(_lib.call("jpegr_stream_encode_scratch_bytes", ntiles, cap))


def encode_stream_device(d_coef, w, h, nimg=1, tight=False, d_out=None, d_len=None, d_result=None,
                         scratch=None, stream=None):
    """encode_device's coefficients straight to a JPR1 (tight=True: JPT1)
    stream, with no slots (jpegr_stream_encode_device): the bytes of
    Entropy.encode + pack_device.  Returns (d_out, d_len, d_result): d_out a
    uint8 tensor (pack_bound bytes when not given), d_len one int64 holding the
    stream length -- or the capacity needed when that exceeds d_out's size, in
    which case nothing past d_out is written -- and d_result two int64, [0] the
    length again, [1] the streams that overflow the reference's buffers.
    scratch: stream_encode_scratch_bytes(ntiles, d_out.numel()) bytes.
    Asynchronous: no read-back."""
    import torch
    nt = nimg * tiles(w, h)
    dev = d_coef.device
    _buffer(d_coef, nt * 128, torch.int16, dev, "d_coef smaller than ntiles * 128 int16",
            in_bytes=True)
    if d_out is None:
        d_out = torch.empty(pack_bound(w, h, nimg), dtype=torch.uint8, device=dev)
    if d_len is None:
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    d_result = _buffer(d_result, 2, torch.int64, dev)
    scratch = _buffer(scratch, stream_encode_scratch_bytes(nt, d_out.numel()), torch.uint8, dev,
                      "scratch smaller than stream_encode_scratch_bytes(ntiles, cap)")
    _call("jpegr_stream_encode_device", d_coef, w, h, nimg, STREAM_JPT1 if tight else STREAM_JPR1,
          d_out, d_out.numel(), d_len, scratch, d_result, stream_arg(stream))
    return d_out, d_len, d_result


def encode_stream_exact_device(d_coef, w, h, nimg=1, tight=False, cap=None):
    """(a uint8 tensor of exactly the stream, the overflow count) by
    encode_stream_device into `cap` bytes -- by default a quarter of the bound,
    which holds every stream measured so far (a random 4K image takes 150 B a
    tile of the bound's 1,038) -- and, when the stream is longer, once more
    into exactly what the first call asked for.  Reads the result back."""
    import torch
    if cap is None:
        cap = 16 + nimg * tiles(w, h) * 258
    d_out = torch.empty(cap, dtype=torch.uint8, device=d_coef.device)
    _, _, d_result = encode_stream_device(d_coef, w, h, nimg, tight=tight, d_out=d_out)
    n, over = d_result.cpu().tolist()
    if n > cap:
        d_out = torch.empty(n, dtype=torch.uint8, device=d_coef.device)
        _, _, d_result = encode_stream_device(d_coef, w, h, nimg, tight=tight, d_out=d_out)
        n, over = d_result.cpu().tolist()
    return d_out[:n].clone(), over


def compress_device(d_rgba, w, h, nimg=1, tight=False, direct=False):
    """RGBA8 images -> a uint8 tensor of exactly the JPR stream (JPR1, or JPT1
    with tight=True: the same content in fewer bytes, read by
    decompress_images_device and decode_stream_device only): encode, entropy
    encode, pack; the length is read back once, then the encoder's
    status word.  Raises JpegError if a stream overflowed the reference's
    buffers (status[0] != 0).  direct=True: the same bytes by
    encode_stream_device, with no slots (d_result[1] is the status word)."""
    d_coef = encode_device(d_rgba, w, h, nimg)
    if direct:
        d_out, over = encode_stream_exact_device(d_coef, w, h, nimg, tight=tight)
        if over != 0:
            raise JpegError(-1, "compress_device: a stream overflows the reference's buffers")
        return d_out
    ent = Entropy(nimg * tiles(w, h), device=d_rgba.device)
    ent.encode(d_coef)
    d_out, d_len = pack_device(ent, w, h, nimg, tight=tight)
    n = int(d_len.item())
    if int(ent.status[0].item()) != 0:
        raise JpegError(-1, "compress_device: a stream overflows the reference's buffers")
    return d_out[:n].clone()


def decompress_device(d_stream):
    """A JPR1 stream (uint8 tensor, exactly the stream; a JPT1 stream raises
    JpegError: it has no slot form) -> (rgba uint8 tensor,
    w, h, nimg): reads the 16 header bytes back, then unpack, entropy decode
    and reconstruct.  No d_orig is passed to the reconstruction, so every tile
    is decoded (the reference leaves its trailing tiles untransformed; see
    jpegr_reconstruct_device).  Raises JpegError on an inconsistent stream
    (d_result[1] != ~0) or a malformed entropy stream (status[1] != 0)."""
    import torch
    w, h, nimg, _ = _open_stream(d_stream, "decompress_device", slots=True)
    ent, d_result = unpack_device(d_stream, d_stream.numel(), w, h, nimg)
    d_coef = torch.empty(nimg * coef_count(w, h), dtype=torch.int16, device=d_stream.device)
    ent.decode(d_coef)
    out = reconstruct_device(d_coef, w, h, nimg)
    # the slot decoder counts its rejected streams in the Entropy's status, not in d_result
    _raise_on_verdict("decompress_device", (None, int(d_result[1].item()), int(ent.status[1].item())))
    return out, w, h, nimg
