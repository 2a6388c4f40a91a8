"""What lz4jpeg's Python wrappers do around a C call, without a GPU: argument
conversion, the checks made in Python (their order and their text), a
library argument error surfacing as the module's exception, and the empty
batches that never reach the library.  Every tensor is a CPU tensor and every
call stops in Python or at the library's argument check, which comes before
any HIP call; the stream is a stub, so torch is never asked for a CUDA one."""
import numpy as np
import pytest
import torch

from lz4jpeg import _lib, jpeg, lz4, synth

W, H, NIMG = 16, 8, 2                     # two tiles an image
NT = 4


class _Stream:
    cuda_stream = 0


S = _Stream()
IN_LEN = "in_len past the end of d_stream"
OFFSETS = "d_offsets smaller than ntiles + 1"
ENT = "ent does not hold nimg * tiles(w, h) tiles"
IMAGES = "image range outside the stream"


def header(magic=b"JPR1", w=W, h=H, nimg=NIMG):
    return magic + b"".join(int(v).to_bytes(4, "little") for v in (w, h, nimg))


def u8(n=64):
    t = torch.zeros(n, dtype=torch.uint8)
    t[:16] = torch.frombuffer(bytearray(header()), dtype=torch.uint8)
    return t


def i64(*v):
    return torch.tensor(v, dtype=torch.int64)


def raises(exc, text, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc and str(e.value) == text
    return e.value


def jpeg_arg_error(name):
    return f"{name}: jpegr error -1 (invalid argument)"


def lz4_arg_error(name):
    return f"{name}: lz4r error -1 ({_lib.lib().lz4r_strerror(-1).decode()})"


# ---- 1. conversion ---------------------------------------------------------------

@pytest.mark.parametrize("as_array", [False, True])
def test_headers_as_bytes_and_arrays(as_array):
    def arg(b):
        return np.frombuffer(b, np.uint8) if as_array else b
    assert jpeg.stream_format(arg(header())) == (W, H, NIMG, False)
    assert jpeg.stream_format(arg(header(b"JPT1", 24, 40, 3))) == (24, 40, 3, True)
    assert jpeg.stream_info(arg(header() + b"tail")) == (W, H, NIMG)
    e = raises(jpeg.JpegError, jpeg_arg_error("jpegr_stream_info"), jpeg.stream_info,
               arg(header(b"JPT1")))
    assert e.code == -1
    raises(jpeg.JpegError, jpeg_arg_error("jpegr_stream_format"), jpeg.stream_format,
           arg(header(b"JPX1")))
    raises(ValueError, "a JPR header is 16 bytes", jpeg.stream_format, arg(header()[:15]))
    raises(ValueError, "a JPR header is 16 bytes", jpeg.stream_info, arg(header()[:15]))


def test_size_functions():
    assert jpeg.coef_count(3840, 2160) == 480 * 270 * 128
    assert jpeg.coef_count(9, 9) == 4 * 128 and jpeg.coef_count(0, 8) == 0
    assert jpeg.pack_bound(8, 8) == 16 + 2 + 1036
    assert jpeg.pack_bound(3840, 2160, 2) == 16 + 2 * 480 * 270 * (2 + 1036)
    assert jpeg.pack_bound(0, 8, 1) == 0
    assert type(jpeg.coef_count(9, 9)) is int and type(jpeg.pack_bound(8, 8)) is int
    assert jpeg.crop_items(9, 8) == 6 and jpeg.crop_scratch_bytes(1, 8, 8) == 4 * 256 + 16
    assert lz4.compress_bound(600) == 1 + 2 * _lib.LZ4R_BLOCK_BOUND


# ---- 2. the library's ERR_ARG as the module's error, naming the C function --------

def test_misaligned_coefficients_are_the_librarys_to_reject():
    d_coef = torch.zeros(NT * 128 + 1, dtype=torch.int16)[1:]
    assert d_coef.data_ptr() % 16 == 2
    e = raises(jpeg.JpegError, jpeg_arg_error("jpegr_stream_decode_device"),
               jpeg.decode_stream_device, u8(), 64, W, H, NIMG, d_coef=d_coef, stream=S)
    assert e.code == -1


def test_misaligned_offsets_are_the_librarys_to_reject():
    d_offsets = torch.zeros(2 * (NT + 1) + 1, dtype=torch.int32)[1:]
    assert d_offsets.data_ptr() % 8 == 4
    e = raises(jpeg.JpegError, jpeg_arg_error("jpegr_stream_index_device"),
               jpeg.stream_index_device, u8(), 64, W, H, NIMG, d_offsets=d_offsets, stream=S)
    assert e.code == -1


def test_lz4_no_blocks_is_the_librarys_to_reject():
    e = raises(lz4.Lz4Error, lz4_arg_error("lz4r_read_device"), lz4.read_device, u8(), 64,
               i64(1, 2), 0, i64(0), i64(4), 4, stream=S, check=False)
    assert e.code == -1
    e = raises(lz4.Lz4Error, lz4_arg_error("lz4r_decompress_device"), lz4.decompress_device, u8(),
               64, i64(1, 2), 0, 16, stream=S)
    assert e.code == -1
    # a raw device pointer for the offsets takes the same road
    raises(lz4.Lz4Error, lz4_arg_error("lz4r_decompress_device"), lz4.decompress_device, u8(), 64,
           i64(1, 2).data_ptr(), 0, 16, stream=S, check=False)


def test_too_small_is_still_input_too_small():
    e = raises(lz4.InputTooSmall, "lz4r_compress: lz4r error -2 "
               f"({_lib.lib().lz4r_strerror(-2).decode()})", lz4.compress, b"x" * 299)
    assert e.code == -2 and isinstance(e, lz4.Lz4Error)


# ---- 3. the checks made in Python, first and with their text -----------------------

def _rects():
    """One crop's and one selection's columns."""
    return dict(d_image=i64(0), d_x=i64(0), d_y=i64(0), d_w=i64(8), d_h=i64(8))


def _crop(d_stream=None, in_len=64, d_offsets=None, **kw):
    r = _rects()
    return jpeg.crop_device(u8() if d_stream is None else d_stream, in_len, W, H, NIMG,
                            torch.zeros(NT + 1, dtype=torch.int64) if d_offsets is None else d_offsets,
                            r["d_image"], r["d_x"], r["d_y"], r["d_w"], r["d_h"], 8, 8, stream=S, **kw)


def _select(d_stream=None, in_len=64, d_offsets=None, **kw):
    r = _rects()
    return jpeg.select_device(u8() if d_stream is None else d_stream, in_len, W, H, NIMG,
                              torch.zeros(NT + 1, dtype=torch.int64) if d_offsets is None else d_offsets,
                              r["d_image"], r["d_x"], r["d_y"], 8, 8, stream=S, **kw)


def test_in_len_past_the_tensor():
    d = u8()
    raises(ValueError, IN_LEN, jpeg.unpack_device, d, 65, W, H, NIMG, stream=S)
    raises(ValueError, IN_LEN, jpeg.decode_stream_device, d, 65, W, H, NIMG, stream=S)
    raises(ValueError, IN_LEN, jpeg.stream_index_device, d, 65, W, H, NIMG, stream=S)
    raises(ValueError, IN_LEN, _crop, d, 65)
    raises(ValueError, IN_LEN, jpeg.thumb_device, d, 65, W, H, NIMG, stream=S)
    raises(ValueError, IN_LEN, _select, d, 65)


def test_ranges_outside_the_stream():
    d = u8()
    for tile0, ntiles in ((-1, 1), (0, 0), (0, NT + 1), (NT, None), (3, 2)):
        raises(ValueError, "tile range outside the stream", jpeg.decode_stream_device, d, 64, W, H,
               NIMG, tile0, ntiles, stream=S)
    for first, count in ((-1, 1), (0, 0), (0, NIMG + 1), (NIMG, None), (1, 2)):
        raises(ValueError, IMAGES, jpeg.thumb_device, d, 64, W, H, NIMG, first, count, stream=S)
    # the range is judged before in_len in thumb_device, after it in decode_stream_device
    raises(ValueError, IMAGES, jpeg.thumb_device, d, 65, W, H, NIMG, 0, 3, stream=S)
    raises(ValueError, IN_LEN, jpeg.decode_stream_device, d, 65, W, H, NIMG, 0, NT + 1, stream=S)


def test_offsets_one_entry_short():
    short = torch.zeros(NT, dtype=torch.int64)
    raises(ValueError, OFFSETS, _crop, d_offsets=short)
    raises(ValueError, OFFSETS, jpeg.thumb_device, u8(), 64, W, H, NIMG, d_offsets=short, stream=S)
    raises(ValueError, OFFSETS, _select, d_offsets=short)
    raises(ValueError, OFFSETS, jpeg.stream_index_device, u8(), 64, W, H, NIMG, d_offsets=short,
           stream=S)
    # elements, not bytes: int32 entries are counted as entries
    raises(ValueError, OFFSETS, jpeg.stream_index_device, u8(), 64, W, H, NIMG,
           d_offsets=torch.zeros(NT, dtype=torch.int32), stream=S)


def test_buffers_one_element_short():
    d = u8()
    raises(ValueError, "d_coef smaller than ntiles * 128 int16", jpeg.decode_stream_device, d, 64, W,
           H, NIMG, 1, 2, d_coef=torch.zeros(2 * 128 - 1, dtype=torch.int16), stream=S)
    raises(ValueError, "d_coef smaller than ntiles * 128 int16", jpeg.encode_stream_device,
           torch.zeros(NT * 128 - 1, dtype=torch.int16), W, H, NIMG, stream=S)
    # bytes, not elements: the same coefficients as uint8 are enough in number but not in size
    raises(ValueError, "d_coef smaller than ntiles * 128 int16", jpeg.encode_stream_device,
           torch.zeros(NT * 128, dtype=torch.uint8), W, H, NIMG, stream=S)
    raises(ValueError, "d_out smaller than four bytes per tile", jpeg.thumb_device, d, 64, W, H, NIMG,
           1, 1, d_out=torch.zeros(2 * 4 - 1, dtype=torch.uint8), stream=S)
    raises(ValueError, "d_dc smaller than four int16 per tile", jpeg.thumb_device, d, 64, W, H, NIMG,
           d_dc=torch.zeros(NT * 4 - 1, dtype=torch.int16), stream=S)
    # d_dc is judged before d_out
    raises(ValueError, "d_dc smaller than four int16 per tile", jpeg.thumb_device, d, 64, W, H, NIMG,
           d_dc=torch.zeros(1, dtype=torch.int16), d_out=torch.zeros(1, dtype=torch.uint8), stream=S)
    raises(ValueError, "d_rgba smaller than nimg*h*w*4", jpeg.encode_device,
           torch.zeros(NIMG * W * H * 4 - 1, dtype=torch.uint8), W, H, NIMG, stream=S)


def test_scratch_one_byte_short():
    need = jpeg.crop_scratch_bytes(1, 8, 8)
    raises(ValueError, "scratch smaller than crop_scratch_bytes(nrects, max_w, max_h)", _crop,
           scratch=torch.zeros(need - 1, dtype=torch.uint8))
    need = jpeg.select_scratch_bytes(1, 8, 8)
    raises(ValueError, "scratch smaller than select_scratch_bytes(nitems, out_w, out_h)", _select,
           scratch=torch.zeros(need - 1, dtype=torch.uint8))
    d_out = torch.zeros(100, dtype=torch.uint8)
    need = jpeg.stream_encode_scratch_bytes(NT, 100)
    raises(ValueError, "scratch smaller than stream_encode_scratch_bytes(ntiles, cap)",
           jpeg.encode_stream_device, torch.zeros(NT * 128, dtype=torch.int16), W, H, NIMG,
           d_out=d_out, scratch=torch.zeros(need - 1, dtype=torch.uint8), stream=S)


def test_select_items_and_cap():
    raises(ValueError, "cap past the end of d_out", _select, d_out=torch.zeros(32, dtype=torch.uint8),
           cap=33)
    items = "d_image, d_x and d_y hold one entry per item, and at least one"
    d, offs, none = u8(), torch.zeros(NT + 1, dtype=torch.int64), i64()
    raises(ValueError, items, jpeg.select_device, d, 64, W, H, NIMG, offs, none, none, none, 8, 8,
           stream=S)
    raises(ValueError, items, jpeg.select_device, d, 65, W, H, NIMG, offs, i64(0), i64(0, 0), i64(0),
           8, 8, stream=S)


def test_entropy_of_another_tile_count():
    ent = jpeg.Entropy(NT - 1, device="cpu")
    assert (ent.bits.numel(), ent.meta.numel(), ent.table.numel(), ent.status.numel()) == \
        ((NT - 1) * 256, (NT - 1) * 3, (NT - 1) * 256, 4)
    assert not ent.bits.any() and not ent.meta.any() and not ent.table.any() and not ent.status.any()
    assert ent.scratch.numel() == _lib.lib().jpegr_entropy_scratch_bytes(NT - 1)
    raises(ValueError, ENT, jpeg.pack_device, ent, W, H, NIMG, stream=S)
    raises(ValueError, ENT, jpeg.unpack_device, u8(), 64, W, H, NIMG, ent=ent, stream=S)
    # the Entropy is judged before in_len
    raises(ValueError, ENT, jpeg.unpack_device, u8(), 65, W, H, NIMG, ent=ent, stream=S)


def test_segment_needs_final_shard():
    c = lz4.Compressor.__new__(lz4.Compressor)          # no context: the check comes first
    raises(ValueError, "compress_async(segment=True) needs final_shard=True/False", c.compress_async,
           u8(), 64, u8(), i64(0), stream=S, segment=True)


def test_synth_short_outputs():
    raises(ValueError, "rand_rgba_device: output too small", synth.rand_rgba_device,
           torch.zeros(4 * 5 - 1, dtype=torch.uint8), 0, 5, stream=S)
    raises(ValueError, "random_passages_device: output too small", synth.random_passages_device,
           torch.zeros(99, dtype=torch.uint8), 100, length=10, src=b"abcdefghijklmnopqrstuvwxyz" * 4,
           stream=S)


# ---- 4. empty batches never reach the library --------------------------------------

@pytest.mark.parametrize("check,count", [(True, 0), (False, None)])
def test_no_rectangles(check, count):
    none = i64()
    d_out, d_dst, n = jpeg.crop_device(u8(), 65, W, H, NIMG, torch.zeros(1, dtype=torch.int64), none,
                                       none, none, none, none, 8, 8, stream=S, check=check)
    assert n == count and type(n) is type(count)
    assert d_out.dtype == torch.uint8 and d_out.numel() == 4 and d_dst.numel() == 0
    mine = torch.zeros(7, dtype=torch.uint8)
    d_out, d_dst, n = jpeg.crop_device(u8(), 65, W, H, NIMG, torch.zeros(1, dtype=torch.int64), none,
                                       none, none, none, none, 8, 8, d_dst=none, d_out=mine, stream=S,
                                       check=check)
    assert d_out is mine and d_dst is none and n == count


@pytest.mark.parametrize("check,count", [(True, 0), (False, None)])
def test_no_reads(check, count):
    none = i64()
    d_out, d_dst, n = lz4.read_device(u8(), 64, i64(1), 0, none, none, 4, stream=S, check=check)
    assert n == count and type(n) is type(count)
    assert d_out.dtype == torch.uint8 and d_out.numel() == 1 and d_dst.numel() == 0
