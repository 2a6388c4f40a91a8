"""Host-side mirror of the reference's LZ4 encoder interface over the HIP path.

Reference (Algorithms/sequential/LZ4/LZ4.c):
  lz4_encode()         :670-742  file in -> compressed.bin  ==  compress(bytes)
  divide_input()       :123-177  300-byte blocks            ==  nblocks()/shard_blocks()
  block_encode() + find_longest_match()  run inside the HIP kernels.

Errors follow the reference's exit paths as exceptions: an input shorter than
300 bytes raises InputTooSmall (the reference prints and exit(1)s, :632-637).
Device memory and streams come from torch (plumbing only); the compute is the
C ABI in include/lz4r.h.
"""
import functools
from ctypes import byref, c_float, c_size_t, c_void_p

import numpy as np

from . import _lib
from ._lib import Lz4Error, LZ4R_BLOCK, LZ4R_BLOCK_BOUND, stream_arg  # noqa: F401

BLOCK = LZ4R_BLOCK


class InputTooSmall(Lz4Error):
    pass


def _raise(code, where):
    if code == _lib.LZ4R_ERR_TOO_SMALL:
        raise InputTooSmall(code, where)
    raise Lz4Error(code, where)


_call = functools.partial(_lib.call, error=_raise)      # a nonzero return raises


def nblocks(n):
    return (n + BLOCK - 1) // BLOCK


def compress_bound(n):
    return int(_lib.call("lz4r_compress_bound", n))


def frame_bound(n):
    """Worst-case bytes of the standard LZ4 frame of n input bytes
    (lz4r_frame_bound)."""
    return int(_lib.call("lz4r_frame_bound", n))


def _output(d_out, out_cap, device):
    """The caller's d_out, or out_cap new bytes (one at the least)."""
    if d_out is not None:
        return d_out
    import torch
    return torch.empty(max(out_cap, 1), dtype=torch.uint8, device=device)


def _offsets_arg(d_offsets):
    """Block offsets come as an int64 tensor or as the raw device pointer
    Compressor.block_offsets_device() returns."""
    return d_offsets if isinstance(d_offsets, int) else d_offsets.data_ptr()


class Compressor:
    """Owns an lz4r context (device scratch) on the current device."""

    def __init__(self):
        h = c_void_p()
        _call("lz4r_ctx_create", byref(h))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.call("lz4r_ctx_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- device API -------------------------------------------------------
    def compress_device(self, d_in, n=None, d_out=None, stream=None):
        """Compress the uint8 CUDA tensor d_in (first n bytes).  Returns
        (d_out, length): the framed stream is d_out[:length]."""
        import torch
        n = d_in.numel() if n is None else n
        if d_out is None:
            d_out = torch.empty(compress_bound(n), dtype=torch.uint8, device=d_in.device)
        got = c_size_t(0)
        _call("lz4r_compress_device", self._h, d_in, n, d_out, d_out.numel(), byref(got),
              stream_arg(stream))
        return d_out, got.value

    def compress_async(self, d_in, n, d_out, d_len, stream=None, segment=False,
                       final_shard=None):
        """Enqueue only; the uint64 length lands in d_len (1-element int64 tensor),
        with bit 63 set if the call met a corrupt LDS index: read it with
        async_length(d_len), which raises then.
        segment=True: whole blocks without the frame header (one shard);
        final_shard must then be given: only the globally last shard may end
        in a short block, a non-final shard (final_shard=False) must be a
        multiple of 300 bytes (else the concatenated stream would differ from
        the single-GPU one)."""
        if segment and final_shard is None:
            raise ValueError("compress_async(segment=True) needs final_shard=True/False")
        args = (self._h, d_in, n, d_out, d_out.numel(), d_len)
        if segment:
            _call("lz4r_compress_segment_async", *args, 1 if final_shard else 0, stream_arg(stream))
        else:
            _call("lz4r_compress_async", *args, stream_arg(stream))

    # -- standard LZ4 frames ----------------------------------------------
    def compress_frame_device(self, d_in, n=None, d_out=None, stream=None):
        """compress_device, for a standard LZ4 frame (what `lz4 -d` and liblz4
        read): returns (d_out, length), the frame is d_out[:length].  After
        it block_offsets() raises: a frame has no per-block arrays."""
        import torch
        n = d_in.numel() if n is None else n
        if d_out is None:
            d_out = torch.empty(frame_bound(n), dtype=torch.uint8, device=d_in.device)
        got = c_size_t(0)
        _call("lz4r_compress_frame_device", self._h, d_in, n, d_out, d_out.numel(), byref(got),
              stream_arg(stream))
        return d_out, got.value

    def compress_frame_async(self, d_in, n, d_out, d_len, stream=None):
        """compress_async, for a standard LZ4 frame: enqueue only (capturable
        into a graph); the length, or the need when it exceeds d_out.numel(),
        lands in d_len (read it with async_length)."""
        _call("lz4r_compress_frame_async", self._h, d_in, n, d_out, d_out.numel(), d_len,
              stream_arg(stream))

    def compress_frame(self, data):
        """bytes -> the bytes of a standard LZ4 frame."""
        import torch
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        if buf.size < BLOCK:
            raise InputTooSmall(_lib.LZ4R_ERR_TOO_SMALL, "compress_frame")
        d_out, length = self.compress_frame_device(torch.from_numpy(buf.copy()).cuda())
        return d_out[:length].cpu().numpy().tobytes()

    @staticmethod
    def async_length(d_len):
        """The length an async call stored in the int64 tensor d_len (reads it
        back: waits for torch's current stream).  Raises Lz4Error(-6) when the
        call flagged a corrupt LDS index (LZ4R_LEN_CORRUPT, bit 63: the int64
        is negative) -- the stream must not be used then."""
        v = int(d_len.item())
        if v < 0:
            raise Lz4Error(_lib.LZ4R_ERR_CORRUPT,
                           "lz4r_compress_*_async: corrupt LDS index (LZ4R_LEN_CORRUPT)")
        return v

    def block_offsets(self, count, stream=None):
        """numpy uint64 array: the last call's first `count` per-block output
        offsets (relative to the first block byte)."""
        out = np.empty(count, dtype=np.uint64)
        _call("lz4r_copy_block_offsets", self._h, out, count, stream_arg(stream))
        return out

    def block_offsets_device(self):
        """(device pointer, count) of the last call's per-block offsets, as the
        placement kernel wrote them (valid until the next call on this
        context); lz4r_block_offsets_device."""
        ptr, cnt = c_void_p(), c_size_t(0)
        _call("lz4r_block_offsets_device", self._h, byref(ptr), byref(cnt))
        return ptr.value, cnt.value

    def check(self, stream=None):
        """lz4r_check: synchronise and raise Lz4Error(-6) if the last call met
        a corrupt bucket head (compress_device and async_length check by
        themselves)."""
        _call("lz4r_check", self._h, stream_arg(stream))

    def set_timing(self, enable=True):
        """Record HIP events on the launch stream around each call and its
        match-finder/parse kernel (see last_timing)."""
        _lib.call("lz4r_set_timing", self._h, 1 if enable else 0)

    def last_timing(self):
        """(ms of the whole last call, ms of its lz4_analyze kernel)."""
        a, b = c_float(0), c_float(0)
        _call("lz4r_last_timing", self._h, byref(a), byref(b))
        return a.value, b.value

    def timed_calls(self, max_calls=4096):
        """(ms of each call, ms of its lz4_tiles launches): two lists over the
        newest calls timed since set_timing(True), oldest first (waits for
        the newest; lz4r_timed_calls)."""
        a = (c_float * max_calls)()
        b = (c_float * max_calls)()
        cnt = c_size_t(0)
        _call("lz4r_timed_calls", self._h, max_calls, a, b, byref(cnt))
        return list(a[:cnt.value]), list(b[:cnt.value])

    # -- host convenience -------------------------------------------------
    def compress(self, data):
        """bytes -> framed compressed bytes (== the reference's compressed.bin)."""
        import torch
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        if buf.size < BLOCK:
            raise InputTooSmall(_lib.LZ4R_ERR_TOO_SMALL, "compress")
        d_in = torch.from_numpy(buf.copy()).cuda()
        d_out, length = self.compress_device(d_in)
        torch.cuda.synchronize()
        return d_out[:length].cpu().numpy().tobytes()


def compress(data):
    """One-shot host API: compressed bytes of `data` (a bytes-like object)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.size
    if n < BLOCK:
        raise InputTooSmall(_lib.LZ4R_ERR_TOO_SMALL, "lz4r_compress")
    cap = 1 + nblocks(n) * LZ4R_BLOCK_BOUND
    out = np.empty(cap, dtype=np.uint8)
    got = c_size_t(0)
    _call("lz4r_compress", buf, n, out, cap, byref(got))
    return out[:got.value].tobytes()


def compress_frame(data):
    """One-shot host API: `data` as a standard LZ4 frame (lz4r_compress_frame)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.size
    if n < BLOCK:
        raise InputTooSmall(_lib.LZ4R_ERR_TOO_SMALL, "lz4r_compress_frame")
    cap = frame_bound(n)
    out = np.empty(cap, dtype=np.uint8)
    got = c_size_t(0)
    _call("lz4r_compress_frame", buf, n, out, cap, byref(got))
    return out[:got.value].tobytes()


def decompress_frame(frame_bytes, cap=None):
    """Exact host decoder of standard LZ4 frames (lz4r_frame_decompress): the
    library's own or any other writer's, one or several concatenated.  cap:
    the room for the output; by default it grows to what the decoder asks for.
    Raises Lz4Error(-6) on a malformed frame, Lz4Error(-3) when a given cap
    is too small."""
    buf = np.frombuffer(bytes(frame_bytes), dtype=np.uint8)
    room = 4 * buf.size + 65536 if cap is None else cap
    while True:
        out = np.empty(max(room, 1), dtype=np.uint8)
        got = c_size_t(0)
        rc = _lib.call("lz4r_frame_decompress", buf, buf.size, out, room, byref(got))
        if rc == _lib.LZ4R_ERR_CAPACITY and cap is None:
            room = max(got.value, 2 * room)
            continue
        if rc:
            _raise(rc, "lz4r_frame_decompress")
        return out[:got.value].tobytes()


def decompress_frame_device(d_frame, length=None, cap=None, d_out=None, verify_content=True,
                            stream=None):
    """GPU decoder of standard LZ4 frames (lz4r_frame_decompress_device): the
    first `length` bytes of the uint8 tensor d_frame, one frame or several
    concatenated, this library's or any other writer's.  Returns (d_out, n):
    the decoded bytes are d_out[:n].  cap: the room for the output (d_out's
    size when d_out is given); with neither, one call with no room asks for
    the decoded length, which is then allocated and decoded into.
    verify_content=False skips the frames' content checksums.  Raises
    Lz4Error(-6) on a malformed frame, Lz4Error(-3) when a given cap or d_out
    is too small.  Synchronises `stream`."""
    import torch
    length = d_frame.numel() if length is None else length
    flags = 0 if verify_content else _lib.LZ4R_FRAME_NO_CONTENT_CHECKSUM
    got = c_size_t(0)
    if cap is None and d_out is None:
        rc = _lib.call("lz4r_frame_decompress_device", d_frame, length, None, 0, byref(got), flags,
                       stream_arg(stream))
        if rc not in (_lib.LZ4R_OK, _lib.LZ4R_ERR_CAPACITY):
            _raise(rc, "lz4r_frame_decompress_device")
        if rc == _lib.LZ4R_OK:                           # frames of no bytes at all
            return torch.empty(0, dtype=torch.uint8, device=d_frame.device), 0
        cap = got.value
    elif cap is None:
        cap = d_out.numel()
    d_out = _output(d_out, cap, d_frame.device)
    _call("lz4r_frame_decompress_device", d_frame, length, d_out, cap, byref(got), flags,
          stream_arg(stream))
    return d_out, got.value


def decompress_frame_gpu(frame_bytes, verify_content=True):
    """Host bytes of standard LZ4 frames -> the decoded bytes, by the GPU
    decoder (decompress_frame_device after a copy in, then a copy out)."""
    import torch
    buf = np.frombuffer(bytes(frame_bytes), dtype=np.uint8)
    if buf.size == 0:
        _raise(_lib.LZ4R_ERR_CORRUPT, "lz4r_frame_decompress_device")
    d_out, n = decompress_frame_device(torch.from_numpy(buf.copy()).cuda(),
                                       verify_content=verify_content)
    return d_out[:n].cpu().numpy().tobytes()


def decompress(stream, cap=None):
    """Exact host decoder (lz4r_decompress): framed stream bytes -> original
    bytes.  Replaces LZ4_decode (LZ4.c:1038-1121); raises Lz4Error(-6) on a
    malformed stream."""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    if cap is None:
        cap = (buf.size // 5 + 1) * BLOCK
    out = np.empty(max(cap, 1), dtype=np.uint8)
    got = c_size_t(0)
    _call("lz4r_decompress", buf, buf.size, out, cap, byref(got))
    return out[:got.value].tobytes()


def decompress_device(d_stream, length, d_offsets, nb, out_cap, d_out=None, stream=None,
                      check=True):
    """Block-parallel GPU decode (lz4r_decompress_device).  d_stream: uint8
    tensor holding the framed stream (first `length` bytes); d_offsets: int64
    tensor of nb per-block offsets (Compressor.block_offsets), or the raw
    device pointer Compressor.block_offsets_device() returns.  Returns
    (d_out, decoded_length); raises Lz4Error(-6) naming the first malformed
    block.  check=False skips the result read-back (no host sync) and
    returns (d_out, None)."""
    d_out = _output(d_out, out_cap, d_stream.device)
    n = _decode_blocks(d_stream, length, d_offsets, nb, d_out, out_cap, stream, check,
                       "lz4r_decompress_device")
    if check and n > out_cap:
        raise Lz4Error(_lib.LZ4R_ERR_CAPACITY,
                       f"lz4r_decompress_device: needs {n} bytes, capacity {out_cap}")
    return d_out, n


def _decode_blocks(d_stream, length, d_offsets, nb, d_out, out_cap, stream, check, who):
    """lz4r_decompress_device; with check, the decoded length, read back, or
    Lz4Error(-6) "<who>: block <first malformed block>".  d_out None, for an
    out_cap of 0: no output, but every block is checked and counted all the
    same (the result words stand in for the output)."""
    import torch
    res = torch.empty(2, dtype=torch.int64, device=d_stream.device)
    _call("lz4r_decompress_device", d_stream, length, _offsets_arg(d_offsets), nb,
          res if d_out is None else d_out, out_cap, res, stream_arg(stream))
    if not check:
        return None
    return _lib.batch_verdict(res, stream, Lz4Error, _lib.LZ4R_ERR_CORRUPT, f"{who}: block")


def decompress_stream_device(d_stream, length, out_cap, d_out=None, stream=None):
    """GPU decode of a bare framed stream (lz4r_decompress_stream_device):
    the block boundaries are found on the device, as LZ4_decode (LZ4.c:1038)
    needs only the stream.  Returns (d_out, decoded_length); raises
    Lz4Error(-6) on a malformed stream."""
    d_out = _output(d_out, out_cap, d_stream.device)
    got = c_size_t(0)
    _call("lz4r_decompress_stream_device", d_stream, length, d_out, out_cap, byref(got),
          stream_arg(stream))
    return d_out, got.value


def decompress_stream(stream_bytes, cap=None):
    """Host-buffer form of decompress_stream_device (lz4r_decompress_stream)."""
    buf = np.frombuffer(bytes(stream_bytes), dtype=np.uint8)
    if cap is None:
        cap = (buf.size // 8 + 1) * BLOCK
    out = np.empty(max(cap, 1), dtype=np.uint8)
    got = c_size_t(0)
    _call("lz4r_decompress_stream", buf, buf.size, out, cap, byref(got))
    return out[:got.value].tobytes()


# -- random access ------------------------------------------------------------
def stream_index_device(d_stream, length, stream=None):
    """The block offsets of a bare framed stream (lz4r_stream_index_device):
    d_stream's first `length` bytes -> (d_offsets int64 tensor, nb,
    decoded_len), what read_device and decompress_device take.  Tries
    length // 64 + 64 blocks, then once more with the count the library
    names.  Raises Lz4Error(-6) on a malformed stream."""
    import torch
    cap = length // 64 + 64
    for _ in range(2):
        d_offs = torch.empty(cap, dtype=torch.int64, device=d_stream.device)
        nb, n = c_size_t(0), c_size_t(0)
        # no raise by the call itself: too small a first guess is answered, not an error
        rc = _lib.call("lz4r_stream_index_device", d_stream, length, d_offs, cap, byref(nb),
                       byref(n), stream_arg(stream))
        if rc != _lib.LZ4R_ERR_CAPACITY:
            break
        cap = nb.value
    if rc:
        _raise(rc, "lz4r_stream_index_device")
    return d_offs[:nb.value], nb.value, n.value


def read_items(max_len):
    """Lanes a read occupies in a call with this max_len (lz4r_read_items)."""
    return int(_lib.call("lz4r_read_items", max_len))


def read_device(d_stream, length, d_offsets, nb, d_src, d_len, max_len, d_dst=None, d_out=None,
                out_cap=None, stream=None, check=True):
    """Many byte ranges of the decoded stream in one call (lz4r_read_device):
    read r delivers decoded bytes [d_src[r], d_src[r] + d_len[r]) to
    d_out[d_dst[r] ...].  d_src, d_len, d_dst: int64 tensors on the device;
    d_offsets as decompress_device takes them; no d_len may exceed max_len
    (group reads of similar size per call: every read occupies
    read_items(max_len) lanes).  d_dst=None packs the reads back to back;
    d_out=None allocates out_cap bytes (default: the reads' furthest end, read
    back once; nreads * max_len with check=False).  Returns (d_out, d_dst,
    delivered_bytes); raises Lz4Error(-6) naming the first bad read.
    check=False does no read-back and returns None for the count."""
    import torch
    nreads = d_src.numel()
    if d_dst is None:
        d_dst = torch.cumsum(d_len, 0) - d_len
    if out_cap is None:
        if d_out is not None:
            out_cap = d_out.numel()
        elif check and nreads:
            out_cap = int((d_dst + d_len).max().item())
        else:
            out_cap = nreads * max_len
    d_out = _output(d_out, out_cap, d_stream.device)
    if nreads == 0:
        return d_out, d_dst, (0 if check else None)
    d_reads = torch.stack((d_src, d_len, d_dst), dim=1).contiguous()
    res = torch.empty(2, dtype=torch.int64, device=d_stream.device)
    _call("lz4r_read_device", d_stream, length, _offsets_arg(d_offsets), nb, d_reads, nreads, max_len,
          d_out, out_cap, res, stream_arg(stream))
    if not check:
        return d_out, d_dst, None
    n = _lib.batch_verdict(res, stream, Lz4Error, _lib.LZ4R_ERR_CORRUPT, "lz4r_read_device: read")
    return d_out, d_dst, n


class Reader:
    """Random access into one compressed stream on the device: the index is
    built once (stream_index_device) unless the caller has the offsets."""

    def __init__(self, d_stream, length=None, d_offsets=None, nb=None):
        self.d_stream = d_stream
        self.length = d_stream.numel() if length is None else length
        self.decoded_length = None
        if d_offsets is None:
            d_offsets, nb, self.decoded_length = stream_index_device(d_stream, self.length)
        self.d_offsets = d_offsets
        self.nb = d_offsets.numel() if nb is None else nb
        if self.decoded_length is None:
            # the block decoder with no room for output checks every block
            # and reports the decoded length
            self.decoded_length = _decode_blocks(d_stream, self.length, d_offsets, self.nb, None, 0,
                                                 None, True, "Reader")

    def read(self, src, n):
        """Decoded bytes [src, src + n) as a uint8 tensor."""
        import torch
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device=self.d_stream.device)
        d_src = torch.tensor([src], dtype=torch.int64, device=self.d_stream.device)
        d_len = torch.tensor([n], dtype=torch.int64, device=self.d_stream.device)
        d_out, _, got = read_device(self.d_stream, self.length, self.d_offsets, self.nb, d_src,
                                    d_len, n, out_cap=n)
        return d_out[:got]

    def read_many(self, d_src, d_len, max_len, **kw):
        """read_device on this stream: (d_out, d_dst, delivered_bytes)."""
        import torch
        if d_src.numel() == 0:
            return (torch.empty(0, dtype=torch.uint8, device=self.d_stream.device),
                    torch.empty(0, dtype=torch.int64, device=self.d_stream.device),
                    0 if kw.get("check", True) else None)
        return read_device(self.d_stream, self.length, self.d_offsets, self.nb, d_src, d_len,
                           max_len, **kw)
