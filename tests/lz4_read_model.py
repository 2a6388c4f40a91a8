"""What lz4r_read_device must leave behind, in plain Python (a helper, no
tests): the contract of include/lz4r.h restated over the plaintext.

A read is (src, len, dst), each in [0, 2^64).  Judged in this order:

  len == 0                          good, writes nothing (whatever src and dst)
  len > max_len                     bad on its own fields: writes nothing
  src + len >= 2^64                 the same
  dst + len > out_cap               the same
  its last block index >= nb        the same (nb = blocks of the plaintext)
  src + len > len(plain)            bad inside the (short) last block
  a block it covers is in `bad_blocks`   bad inside a block
  otherwise                         good: buffer[dst : dst + len] = plain[src : src + len]

A read that is bad inside a block may leave anything in its own destination
range; loose_ranges() lists those ranges so a test can leave them out of its
whole-buffer comparison.  Everything else is exact.
"""
import numpy as np

BLOCK = 300
OK = (1 << 64) - 1
U64 = 1 << 64

GOOD, BAD_FIELDS, BAD_BLOCK = 0, 1, 2


def read_items(max_len):
    """K(max_len): the blocks a read of max_len bytes can cover."""
    return (max_len + BLOCK - 2) // BLOCK + 1


def judge(n, read, out_cap, max_len, bad_blocks=()):
    src, ln, dst = read
    assert 0 <= src < U64 and 0 <= ln < U64 and 0 <= dst < U64
    if ln == 0:
        return GOOD
    if ln > max_len or src + ln >= U64 or dst + ln > out_cap:
        return BAD_FIELDS
    nb = (n + BLOCK - 1) // BLOCK
    b0, b1 = src // BLOCK, (src + ln - 1) // BLOCK
    if b1 >= nb:
        return BAD_FIELDS
    if src + ln > n or any(b0 <= b <= b1 for b in bad_blocks):
        return BAD_BLOCK
    return GOOD


def expected(plain, reads, out_cap, max_len, sentinel, bad_blocks=()):
    """(buffer, delivered, verdict): the out_cap output bytes (uint8 array,
    `sentinel` where nothing is written), the summed len of the good reads,
    and OK or 1 + the index of the first bad read."""
    p = np.frombuffer(bytes(plain), dtype=np.uint8)
    buf = np.full(out_cap, sentinel, dtype=np.uint8)
    delivered, verdict = 0, OK
    for k, rd in enumerate(reads):
        v = judge(p.size, rd, out_cap, max_len, bad_blocks)
        if v == GOOD:
            src, ln, dst = rd
            if ln:
                buf[dst:dst + ln] = p[src:src + ln]
            delivered += ln
        elif verdict == OK:
            verdict = k + 1
    return buf, delivered, verdict


def loose_ranges(plain, reads, out_cap, max_len, bad_blocks=()):
    """[dst, dst + len) of every read that is bad inside a block."""
    n = len(plain)
    return [(rd[2], rd[2] + rd[1]) for rd in reads
            if judge(n, rd, out_cap, max_len, bad_blocks) == BAD_BLOCK]
