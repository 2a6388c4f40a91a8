"""What jpeg.crop_resize_device and StreamReader.resized_crop_batch do around the
C call, without a GPU (test_py_crop_tensor_cpu.py's pattern: CPU tensors, a stub
stream, every call stops in Python or at the library's argument check)."""
import pytest
import torch

from lz4jpeg import jpeg

W, H, NIMG = 16, 8, 2
NT = 4


class _Stream:
    cuda_stream = 0


S = _Stream()


def u8(n=64):
    t = torch.zeros(n, dtype=torch.uint8)
    hdr = b"JPR1" + b"".join(int(v).to_bytes(4, "little") for v in (W, H, NIMG))
    t[:16] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8)
    return t


def i64(*v):
    return torch.tensor(v, dtype=torch.int64)


def raises(exc, text, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc and str(e.value) == text
    return e.value


def _crop(d_stream=None, in_len=64, d_offsets=None, out_w=5, out_h=7, **kw):
    return jpeg.crop_resize_device(u8() if d_stream is None else d_stream, in_len, W, H, NIMG,
                                   torch.zeros(NT + 1, dtype=torch.int64) if d_offsets is None else d_offsets,
                                   i64(0), i64(0), i64(0), i64(8), i64(8), 8, 8, out_w, out_h, stream=S, **kw)


def test_unknown_dtype_or_layout_raises_before_any_call():
    # in_len is past the tensor: that check would come next
    raises(ValueError, "dtype is none of torch.uint8, float32, float16 and bfloat16", _crop, in_len=65,
           dtype=torch.float64)
    for layout in ("nchw", "CHW", 0, None):
        raises(ValueError, 'layout is "chw" or "hwc"', _crop, in_len=65, layout=layout)


def test_output_size_is_two_positive_ints():
    for kw in ({"out_w": 0}, {"out_h": 0}, {"out_w": -5}, {"out_h": 7.0}, {"out_w": None}):
        raises(ValueError, "out_w and out_h are positive ints", _crop, in_len=65, **kw)
    raises(ValueError, "in_len past the end of d_stream", _crop, in_len=65, out_w=224, out_h=224)


def test_scale_and_bias_are_one_float_or_three():
    raises(ValueError, "scale is one float or three", _crop, in_len=65, scale=(1.0, 2.0))
    raises(ValueError, "bias is one float or three", _crop, in_len=65, bias=(1.0, 2.0, 3.0, 4.0))
    raises(ValueError, "in_len past the end of d_stream", _crop, in_len=65, scale=0.5, bias=(1, 2, 3))


def test_d_out_short_or_of_another_dtype():
    need = 3 * 5 * 7                                         # the output's size, not the source's 3 * 8 * 8
    raises(ValueError, "d_out smaller than out_cap elements", _crop,
           d_out=torch.zeros(need - 1, dtype=torch.float16), out_cap=need, dtype=torch.float16)
    raises(ValueError, "d_out is not of the requested dtype", _crop,
           d_out=torch.zeros(need, dtype=torch.float32), dtype=torch.bfloat16)
    raises(ValueError, "d_out is not of the requested dtype", _crop,
           d_out=torch.zeros(need, dtype=torch.float16))


def test_d_flip_is_a_byte_per_crop():
    text = "d_flip is a bool or uint8 tensor with one entry per crop"
    raises(ValueError, text, _crop, d_flip=torch.zeros(1, dtype=torch.int64))
    raises(ValueError, text, _crop, d_flip=torch.zeros(2, dtype=torch.bool))
    raises(ValueError, "in_len past the end of d_stream", _crop, in_len=65,
           d_flip=torch.zeros(1, dtype=torch.bool))


def test_scratch_is_the_resize_calls_own():
    """The tensor call's scratch is too small for this one."""
    small = torch.zeros(jpeg.crop_scratch_bytes(1, 8, 8), dtype=torch.uint8)
    assert jpeg.crop_resize_scratch_bytes(1, 8, 8, 5, 7) > small.numel()
    raises(ValueError, "scratch smaller than crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h)",
           _crop, scratch=small)


def test_the_librarys_argument_error_names_the_function():
    d_out = torch.zeros(3 * 35 + 4, dtype=torch.float32)[1:]               # 4-B, not 16-B aligned
    assert d_out.data_ptr() % 16 != 0
    e = raises(jpeg.JpegError, "jpegr_crop_resize_device: jpegr error -1 (invalid argument)", _crop,
               d_out=d_out)
    assert e.code == -1
    raises(jpeg.JpegError, "jpegr_crop_resize_device: jpegr error -1 (invalid argument)", _crop,
           scale=float("inf"))
    raises(jpeg.JpegError, "jpegr_crop_resize_device: jpegr error -1 (invalid argument)", _crop,
           antialias=False, bias=(0.0, 1e300, 0.0))                        # inf as a float32


@pytest.mark.parametrize("check,count", [(True, 0), (False, None)])
def test_no_rectangles(check, count):
    none = i64()
    d_out, d_dst, n = jpeg.crop_resize_device(u8(), 65, W, H, NIMG, torch.zeros(1, dtype=torch.int64),
                                              none, none, none, none, none, 8, 8, 5, 7, stream=S,
                                              check=check, dtype=torch.bfloat16)
    assert n == count and type(n) is type(count)
    assert d_out.dtype == torch.bfloat16 and d_out.numel() == 4 and d_dst.numel() == 0


def _reader():
    rd = jpeg.StreamReader.__new__(jpeg.StreamReader)                      # no stream behind it
    rd.d_stream = u8()
    return rd


def test_resized_crop_batch_rejects_before_touching_the_stream():
    rd = jpeg.StreamReader.__new__(jpeg.StreamReader)                      # no stream: the checks come first
    a = (i64(0), i64(0), i64(0), i64(8), i64(8))
    raises(ValueError, 'layout is "chw" or "hwc"', rd.resized_crop_batch, *a, 5, 7, layout="nhwc")
    raises(ValueError, "dtype is none of torch.uint8, float32, float16 and bfloat16", rd.resized_crop_batch,
           *a, 5, 7, dtype=torch.int8)
    raises(ValueError, "out_w and out_h are positive ints", rd.resized_crop_batch, *a, 0, 7)
    raises(ValueError, "mean is one float or three", rd.resized_crop_batch, *a, 5, 7, mean=(1.0, 2.0))


@pytest.mark.parametrize("layout,shape", [("chw", (0, 3, 7, 5)), ("hwc", (0, 7, 5, 3))])
def test_resized_crop_batch_of_no_crops(layout, shape):
    """An empty tensor of the right shape and dtype, without a call: the reader
    has no offsets, no length and no dimensions to make one with."""
    none = i64()
    out = _reader().resized_crop_batch(none, none, none, none, none, 5, 7, dtype=torch.float16, layout=layout)
    assert out.shape == shape and out.dtype == torch.float16
    out = _reader().resized_crop_batch(none, none, none, none, none, 5, 7, layout=layout, antialias=False)
    assert out.shape == shape and out.dtype == torch.float32
