"""What jpeg.crop_tensor_device and StreamReader.crop_batch do around the C call,
without a GPU (test_py_wrappers_cpu.py's pattern: CPU tensors, a stub stream,
every call stops in Python or at the library's argument check)."""
import numpy as np
import pytest
import torch

from lz4jpeg import jpeg

import jpr_tensor_model as T

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


def _crop(d_stream=None, in_len=64, d_offsets=None, **kw):
    return jpeg.crop_tensor_device(u8() if d_stream is None else d_stream, in_len, W, H, NIMG,
                                   torch.zeros(NT + 1, dtype=torch.int64) if d_offsets is None else d_offsets,
                                   i64(0), i64(0), i64(0), i64(8), i64(8), 8, 8, stream=S, **kw)


def test_unknown_dtype_or_layout_raises_before_any_call():
    # in_len is past the tensor: that check would come next
    raises(ValueError, "dtype is none of torch.uint8, float32, float16 and bfloat16", _crop, in_len=65,
           dtype=torch.float64)
    raises(ValueError, "dtype is none of torch.uint8, float32, float16 and bfloat16", _crop, in_len=65,
           dtype="float32")
    for layout in ("nchw", "CHW", 0, None):
        raises(ValueError, 'layout is "chw" or "hwc"', _crop, in_len=65, layout=layout)


def test_scale_and_bias_are_one_float_or_three():
    raises(ValueError, "scale is one float or three", _crop, in_len=65, scale=(1.0, 2.0))
    raises(ValueError, "bias is one float or three", _crop, in_len=65, bias=(1.0, 2.0, 3.0, 4.0))
    raises(ValueError, "in_len past the end of d_stream", _crop, in_len=65, scale=0.5, bias=(1, 2, 3))
    raises(ValueError, "in_len past the end of d_stream", _crop, in_len=65,
           scale=torch.tensor([1.0, 2.0, 3.0]), bias=np.float32(2))


def test_d_out_short_or_of_another_dtype():
    need = 3 * 8 * 8
    raises(ValueError, "d_out smaller than out_cap elements", _crop,
           d_out=torch.zeros(need - 1, dtype=torch.float16), out_cap=need, dtype=torch.float16)
    # elements, not bytes: as many bytes as 192 float16 take are not 192 float32
    raises(ValueError, "d_out is not of the requested dtype", _crop,
           d_out=torch.zeros(2 * need, dtype=torch.uint8), out_cap=need, dtype=torch.float16)
    raises(ValueError, "d_out is not of the requested dtype", _crop,
           d_out=torch.zeros(need, dtype=torch.float32), dtype=torch.bfloat16)
    # the default dtype is float32
    raises(ValueError, "d_out is not of the requested dtype", _crop,
           d_out=torch.zeros(need, dtype=torch.float16))


def test_d_flip_is_a_byte_per_crop():
    text = "d_flip is a bool or uint8 tensor with one entry per crop"
    raises(ValueError, text, _crop, d_flip=torch.zeros(1, dtype=torch.int64))
    raises(ValueError, text, _crop, d_flip=torch.zeros(2, dtype=torch.bool))
    raises(ValueError, "in_len past the end of d_stream", _crop, in_len=65,
           d_flip=torch.zeros(1, dtype=torch.bool))


def test_the_librarys_argument_error_names_the_function():
    d_out = torch.zeros(3 * 64 + 4, dtype=torch.float32)[1:]               # 4-B, not 16-B aligned
    assert d_out.data_ptr() % 16 != 0
    e = raises(jpeg.JpegError, "jpegr_crop_tensor_device: jpegr error -1 (invalid argument)", _crop,
               d_out=d_out)
    assert e.code == -1
    raises(jpeg.JpegError, "jpegr_crop_tensor_device: jpegr error -1 (invalid argument)", _crop,
           scale=float("inf"))
    raises(jpeg.JpegError, "jpegr_crop_tensor_device: jpegr error -1 (invalid argument)", _crop,
           bias=(0.0, 1e300, 0.0))                                         # inf as a float32


@pytest.mark.parametrize("check,count", [(True, 0), (False, None)])
def test_no_rectangles(check, count):
    none = i64()
    d_out, d_dst, n = jpeg.crop_tensor_device(u8(), 65, W, H, NIMG, torch.zeros(1, dtype=torch.int64),
                                              none, none, none, none, none, 8, 8, stream=S, check=check,
                                              dtype=torch.bfloat16)
    assert n == count and type(n) is type(count)
    assert d_out.dtype == torch.bfloat16 and d_out.numel() == 4 and d_dst.numel() == 0


def test_normalisation():
    """crop_batch's scale and bias: 1 / (255 std) and -mean / std, in Python
    floats, rounded once to float32."""
    scale, bias = jpeg.normalisation(T.IMAGENET_MEAN, T.IMAGENET_STD)
    ws, wb = T.normalisation(T.IMAGENET_MEAN, T.IMAGENET_STD)
    assert all(type(v) is float for v in scale + bias)
    assert np.array_equal(np.array(scale, np.float32), ws) and np.array_equal(np.array(bias, np.float32), wb)
    assert scale == [float(v) for v in ws] and bias == [float(v) for v in wb]
    assert scale[1] == float(np.float32(1.0 / (255.0 * 0.224))) and bias[0] == float(np.float32(-0.485 / 0.229))
    scale, bias = jpeg.normalisation()
    assert scale == [float(np.float32(1.0 / 255.0))] * 3 and bias == [0.0] * 3
    assert not any(np.signbit(b) for b in bias)
    scale, bias = jpeg.normalisation(0.5, 0.25)
    assert scale == [float(np.float32(1.0 / (255.0 * 0.25)))] * 3 and bias == [-2.0] * 3
    raises(ValueError, "std is one float or three", jpeg.normalisation, None, (1.0, 2.0))


def test_crop_batch_rejects_before_touching_the_stream():
    rd = jpeg.StreamReader.__new__(jpeg.StreamReader)                      # no stream: the checks come first
    raises(ValueError, 'layout is "chw" or "hwc"', rd.crop_batch, i64(0), i64(0), i64(0), 8, 8, layout="nhwc")
    raises(ValueError, "dtype is none of torch.uint8, float32, float16 and bfloat16", rd.crop_batch,
           i64(0), i64(0), i64(0), 8, 8, dtype=torch.int8)
    raises(ValueError, "mean is one float or three", rd.crop_batch, i64(0), i64(0), i64(0), 8, 8,
           mean=(1.0, 2.0))
