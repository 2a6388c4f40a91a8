"""What jpeg.Dataset, jpeg.dataset_crop_tensor_device and
jpeg.dataset_crop_resize_device do around the C calls, without a GPU
(test_py_crop_resize_cpu.py's method: CPU tensors, stub readers and a stub
stream, every call stops in Python or at the library's argument check)."""
import numpy as np
import pytest
import torch

from lz4jpeg import jpeg


class _Stream:
    cuda_stream = 0


S = _Stream()
SHAPES = [(40, 24, 3, False), (24, 40, 2, True), (8, 8, 1, True), (17, 9, 4, False)]


def i64(*v):
    return torch.tensor(v, dtype=torch.int64)


def raises(exc, text, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc and str(e.value) == text
    return e.value


def reader(w, h, nimg, tight, length=64):
    rd = jpeg.StreamReader.__new__(jpeg.StreamReader)                      # no stream behind it
    rd.w, rd.h, rd.nimg, rd.tight = w, h, nimg, tight
    rd.d_stream = torch.zeros(length, dtype=torch.uint8)
    rd.length = length
    rd.d_offsets = torch.zeros(nimg * jpeg.tiles(w, h) + 1, dtype=torch.int64)
    return rd


def dataset():
    return jpeg.Dataset([reader(*s, length=64 + i) for i, s in enumerate(SHAPES)])


def test_the_tables_bytes():
    ds = dataset()
    assert ds.table.dtype == np.uint64 and ds.table.shape == (4, 6)
    raw = b""
    for rd, image0 in zip(ds.readers, (0, 3, 5, 6)):
        raw += b"".join(int(v).to_bytes(8, "little")
                        for v in (rd.d_stream.data_ptr(), rd.length, rd.d_offsets.data_ptr(), image0))
        raw += b"".join(int(v).to_bytes(4, "little") for v in (rd.w, rd.h, rd.nimg, 0))
    assert ds.table.tobytes() == raw and len(raw) == 4 * jpeg.STREAM_DESC_BYTES
    assert ds.d_table.dtype == torch.int64 and ds.d_table.numpy().tobytes() == raw
    assert ds.d_table.data_ptr() % 8 == 0 and ds.d_table.is_contiguous()
    assert [rd.length for rd in ds.readers] == [64, 65, 66, 67]            # the readers are kept, in order


def test_image0_nimg_and_sizes():
    ds = dataset()
    assert ds.image0.tolist() == [0, 3, 5, 6] and ds.nimg == 10
    assert ds.sizes.shape == (10, 2) and not isinstance(ds.sizes, torch.Tensor)
    assert ds.sizes.tolist() == [[40, 24]] * 3 + [[24, 40]] * 2 + [[8, 8]] + [[17, 9]] * 4
    assert (ds.max_w, ds.max_h) == (40, 40)                                # the largest stream's, per axis
    one = jpeg.Dataset([reader(8, 8, 1, True)])
    assert one.image0.tolist() == [0] and one.nimg == 1 and one.sizes.tolist() == [[8, 8]]


def test_no_readers():
    raises(ValueError, "no readers", jpeg.Dataset, [])


def test_stream_table_rows():
    raises(ValueError, "a row is (d_in, in_len, d_tile_offsets, image0, w, h, nimg)", jpeg.stream_table,
           [(1, 2, 3)])
    raises(ValueError, "w, h and nimg are 32-bit", jpeg.stream_table, [(8, 64, 16, 0, 1 << 32, 8, 1)])
    raises(ValueError, "w, h and nimg are 32-bit", jpeg.stream_table, [(8, 64, 16, 0, 8, 8, -1)])
    assert jpeg.stream_table([]).shape == (0, 6)


class _Spy:
    """Stands in for the two low-level functions: what Dataset passes them."""

    def __init__(self, monkeypatch, name):
        self.calls = []
        monkeypatch.setattr(jpeg, name, lambda *a, **kw: self.calls.append((a, kw)))


def test_default_maxima_are_the_largest_streams(monkeypatch):
    ds = dataset()
    a = (i64(0), i64(0), i64(0), i64(8), i64(8))
    spy = _Spy(monkeypatch, "dataset_crop_resize_device")
    ds.resized_crop_batch(*a, 5, 7)
    ds.resized_crop_batch(*a, 5, 7, max_w=16, max_h=9)
    ds.crops_resized(*a, 5, 7)
    for (args, kw), want in zip(spy.calls, ((40, 40), (16, 9), (40, 40))):
        assert args[0] is ds.d_table and args[1] == 4
        assert args[7:11] == (*want, 5, 7), args[7:]
    assert spy.calls[0][1]["out_cap"] == 3 * 5 * 7 and spy.calls[0][1]["d_out"].numel() == 3 * 5 * 7
    spy = _Spy(monkeypatch, "dataset_crop_tensor_device")
    ds.crops_tensor(*a)
    ds.crops_tensor(*a, 8, 8)
    ds.crop_batch(*a[:3], 8, 6)                                            # a fixed size bounds itself
    assert [c[0][7:9] for c in spy.calls] == [(40, 40), (8, 8), (8, 6)]
    assert spy.calls[2][0][5].tolist() == [8] and spy.calls[2][0][6].tolist() == [6]


def _tensor(d_streams=None, nstreams=4, **kw):
    d_streams = dataset().d_table if d_streams is None else d_streams
    return jpeg.dataset_crop_tensor_device(d_streams, nstreams, i64(0), i64(0), i64(0), i64(8), i64(8), 8, 8,
                                           stream=S, **kw)


def _resize(d_streams=None, nstreams=4, out_w=5, out_h=7, **kw):
    d_streams = dataset().d_table if d_streams is None else d_streams
    return jpeg.dataset_crop_resize_device(d_streams, nstreams, i64(0), i64(0), i64(0), i64(8), i64(8), 8, 8,
                                           out_w, out_h, stream=S, **kw)


SHORT = "d_streams smaller than nstreams descriptors, or none"


@pytest.mark.parametrize("fn", [_tensor, _resize])
def test_argument_errors_before_any_call(fn):
    # nstreams is past the table: that check would come next
    raises(ValueError, "dtype is none of torch.uint8, float32, float16 and bfloat16", fn, nstreams=5,
           dtype=torch.float64)
    for layout in ("nchw", "CHW", 0, None):
        raises(ValueError, 'layout is "chw" or "hwc"', fn, nstreams=5, layout=layout)
    raises(ValueError, "scale is one float or three", fn, nstreams=5, scale=(1.0, 2.0))
    raises(ValueError, "bias is one float or three", fn, nstreams=5, bias=(1.0, 2.0, 3.0, 4.0))
    text = "d_flip is a bool or uint8 tensor with one entry per crop"
    raises(ValueError, text, fn, nstreams=5, d_flip=torch.zeros(1, dtype=torch.int64))
    raises(ValueError, text, fn, nstreams=5, d_flip=torch.zeros(2, dtype=torch.bool))
    raises(ValueError, "d_out is not of the requested dtype", fn, nstreams=5,
           d_out=torch.zeros(192, dtype=torch.float16))
    raises(ValueError, SHORT, fn, nstreams=5)
    raises(ValueError, SHORT, fn, nstreams=0)
    raises(ValueError, SHORT, fn, d_streams=torch.zeros(4 * 6 - 1, dtype=torch.int64))


def test_output_size_is_two_positive_ints():
    for kw in ({"out_w": 0}, {"out_h": 0}, {"out_w": -5}, {"out_h": 7.0}, {"out_w": None}):
        raises(ValueError, "out_w and out_h are positive ints", _resize, nstreams=5, **kw)
    ds = jpeg.Dataset.__new__(jpeg.Dataset)                                # no table: the checks come first
    a = (i64(0), i64(0), i64(0), i64(8), i64(8))
    raises(ValueError, "out_w and out_h are positive ints", ds.resized_crop_batch, *a, 0, 7)
    raises(ValueError, 'layout is "chw" or "hwc"', ds.resized_crop_batch, *a, 5, 7, layout="nhwc")
    raises(ValueError, "mean is one float or three", ds.crop_batch, *a[:3], 8, 8, mean=(1.0, 2.0))


def test_each_call_has_its_own_scratch():
    small = torch.zeros(jpeg.crop_scratch_bytes(1, 8, 8), dtype=torch.uint8)
    assert jpeg.dataset_crop_scratch_bytes(1, 8, 8) == small.numel() + 16
    raises(ValueError, "scratch smaller than dataset_crop_scratch_bytes(nrects, max_w, max_h)", _tensor,
           scratch=small)
    small = torch.zeros(jpeg.crop_resize_scratch_bytes(1, 8, 8, 5, 7), dtype=torch.uint8)
    assert jpeg.dataset_crop_resize_scratch_bytes(1, 8, 8, 5, 7) == small.numel() + 16
    raises(ValueError,
           "scratch smaller than dataset_crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h)",
           _resize, scratch=small)


def test_the_librarys_argument_error_names_the_function():
    d_out = torch.zeros(3 * 64 + 4, dtype=torch.float32)[1:]               # 4-B, not 16-B aligned
    assert d_out.data_ptr() % 16 != 0
    e = raises(jpeg.JpegError, "jpegr_dataset_crop_tensor_device: jpegr error -1 (invalid argument)", _tensor,
               d_out=d_out)
    assert e.code == -1
    raises(jpeg.JpegError, "jpegr_dataset_crop_resize_device: jpegr error -1 (invalid argument)", _resize,
           scale=float("inf"))


@pytest.mark.parametrize("check,count", [(True, 0), (False, None)])
def test_no_rectangles(check, count):
    none = i64()
    table = dataset().d_table
    d_out, d_dst, n = jpeg.dataset_crop_resize_device(table, 5, none, none, none, none, none, 8, 8, 5, 7,
                                                      stream=S, check=check, dtype=torch.bfloat16)
    assert n == count and type(n) is type(count)
    assert d_out.dtype == torch.bfloat16 and d_out.numel() == 4 and d_dst.numel() == 0
    d_out, d_dst, n = jpeg.dataset_crop_tensor_device(table, 5, none, none, none, none, none, 8, 8, stream=S,
                                                      check=check)
    assert n == count and d_out.dtype == torch.float32 and d_dst.numel() == 0


@pytest.mark.parametrize("layout,shape", [("chw", (0, 3, 7, 5)), ("hwc", (0, 7, 5, 3))])
def test_batches_of_no_crops(layout, shape):
    none = i64()
    ds = dataset()
    out = ds.resized_crop_batch(none, none, none, none, none, 5, 7, dtype=torch.float16, layout=layout)
    assert out.shape == shape and out.dtype == torch.float16
    out = ds.crop_batch(none, none, none, 5, 7, layout=layout)
    assert out.shape == shape and out.dtype == torch.float32
