"""The LZ4 stream (include/lz4r.h) restated in plain
Python: no GPU, no torch, nothing from the package.  A test states the
sequences it wants, (L, D, M) = L literals, then M bytes copied from distance
D, and knows the decoded bytes by construction.

  frame     u8 nblocks & 0xFF | block*
  block     u8 nseq & 0xFF | u16 (sum of the sequences' S) + 3 | sequence*
  sequence  u8 token | u16 S | litext(L) | L literals | u16 D | [u8 M - 19]
  token     min(L, 15) << 4 | (M - 4 if M < 19 else 15)
  litext    nothing for L < 15; r = (L - 15) & 255: [r], or [255, 0] for r = 255
  S         the bytes the sequence occupies

Three kinds of sequence:
  (L, D, M), 4 <= M <= 255   a match
  (L, 0, 0)                  the literal-only tail, last in its block
  (L, D, M), 1 <= M <= 3     a truncated match: token 0xFC + M whatever L was,
                             S counts a match-extension byte that is not
                             written (it over-counts by one)
Every block but the stream's last decodes to exactly 300 bytes, the last to
1..300.  The tokens 0xFD..0xFF are also what L >= 15 with M = 17, 18, >= 19
writes; a decoder tells them apart by which reading lets the block end
consistently.
"""

BLOCK = 300
BLOCK_BOUND = 1152                    # LZ4R_BLOCK_BOUND
CHUNK = 8192                          # stream bytes per chunk of the bare path (kChunkB)
CAND_WIN = 2 * BLOCK_BOUND + 32       # the candidate search's window (kWin)


class FormatError(ValueError):
    pass


def litext(L):
    if L < 15:
        return b""
    r = (L - 15) & 255
    return b"\xff\x00" if r == 255 else bytes([r])


def is_tail(seq):
    return seq[1] == 0 and seq[2] == 0


def is_truncated(seq):
    return 1 <= seq[2] <= 3


def plain_ambiguous(seq):
    """A match that writes a token 0xFD..0xFF and is meant as written."""
    L, D, M = seq
    return L >= 15 and M >= 17


def decoded_len(seqs):
    return sum(L + M for L, _, M in seqs)


class Literals:
    """A source of literal bytes: the bytes of `data`, taken in order."""

    def __init__(self, data):
        self.data = bytes(data)
        self.at = 0

    def take(self, n):
        if self.at + n > len(self.data):
            raise FormatError("literal source exhausted")
        b = self.data[self.at:self.at + n]
        self.at += n
        return b


def write_sequence(seq, lits):
    """The bytes of one sequence; lits = its L literal bytes."""
    L, D, M = seq
    if len(lits) != L:
        raise FormatError("literal count")
    ext = litext(L)
    if is_tail(seq):
        tok, S, tail = min(L, 15) << 4, L + 5 + len(ext), b""
    elif 4 <= M <= 255:
        big = M >= 19
        tok = (min(L, 15) << 4) | (15 if big else M - 4)
        S = L + 5 + len(ext) + (1 if big else 0)
        tail = bytes([M - 19]) if big else b""
    elif 1 <= M <= 3:
        tok, S, tail = 0xFC + M, L + 5 + len(ext) + 1, b""
    else:
        raise FormatError(f"match length {M} cannot be written")
    return bytes([tok, S & 255, S >> 8]) + ext + lits + bytes([D & 255, D >> 8]) + tail, S


def write_block(seqs, lits, last=False):
    """(block bytes, decoded bytes) of a list of sequences.  `lits`: a
    Literals source or bytes.  Raises FormatError on anything the format
    cannot hold."""
    if not isinstance(lits, Literals):
        lits = Literals(lits)
    if not 1 <= len(seqs) <= 255:
        raise FormatError("sequence count")
    out = bytearray()
    body = bytearray()
    total = 0
    for i, seq in enumerate(seqs):
        L, D, M = seq
        if L < 0 or L > BLOCK:
            raise FormatError("literal run")
        if is_tail(seq):
            if i + 1 != len(seqs):
                raise FormatError("a literal-only sequence that is not the last")
        else:
            if not 1 <= M <= 255:
                raise FormatError(f"match length {M} cannot be written")
            if D < 1 or D > len(out) + L:
                raise FormatError(f"distance {D} with {len(out) + L} bytes produced")
        lit = lits.take(L)
        out += lit
        for _ in range(M):
            out.append(out[-D])
        if len(out) > BLOCK:
            raise FormatError("more than 300 decoded bytes")
        b, S = write_sequence(seq, lit)
        body += b
        total += S
    if not out or (len(out) != BLOCK and not last):
        raise FormatError(f"{len(out)} decoded bytes")
    blk = bytes([len(seqs)]) + bytes([(total + 3) & 255, (total + 3) >> 8]) + bytes(body)
    if len(blk) > BLOCK_BOUND:
        raise FormatError("encoded size over the block bound")
    return blk, bytes(out)


def write_frame(blocks):
    """blocks: (block bytes, decoded bytes) pairs -> (stream, offsets, plain);
    offsets are relative to the first block byte, as lz4r_decompress_device
    takes them."""
    stream = bytearray([len(blocks) & 255])
    offs, plain = [], bytearray()
    for i, (b, d) in enumerate(blocks):
        if len(d) != BLOCK and i + 1 != len(blocks):
            raise FormatError("a short block that is not the last")
        offs.append(len(stream) - 1)
        stream += b
        plain += d
    return bytes(stream), offs, bytes(plain)


def plain_decode(blk, seqs):
    """The block's bytes read with its known sequence list, a byte at a time;
    nothing is guessed, every field is checked against the list."""
    if blk[0] != len(seqs) & 255:
        raise FormatError("sequence count")
    ip, out, total = 3, bytearray(), 0
    for L, D, M in seqs:
        tok = blk[ip]
        S = blk[ip + 1] | blk[ip + 2] << 8
        start = ip
        ip += 3
        ext = litext(L)
        if blk[ip:ip + len(ext)] != ext:
            raise FormatError("literal extension")
        ip += len(ext)
        out += blk[ip:ip + L]
        ip += L
        if blk[ip] | blk[ip + 1] << 8 != D:
            raise FormatError("distance")
        ip += 2
        if M >= 19:
            if blk[ip] != M - 19:
                raise FormatError("match extension")
            ip += 1
        want_tok = 0xFC + M if 1 <= M <= 3 else (min(L, 15) << 4) | (0 if M == 0 else min(M - 4, 15))
        if tok != want_tok or S != ip - start + (1 if 1 <= M <= 3 else 0):
            raise FormatError("token or size field")
        total += S
        for _ in range(M):
            out.append(out[-D])
    if ip != len(blk) or blk[1] | blk[2] << 8 != total + 3:
        raise FormatError("block size")
    return bytes(out)


def readings(blk, last=False):
    """Every consistent reading of a block as a sequence list, the plain
    reading of each 0xFD..0xFF token first (the decoders' order)."""
    nseq, want, n = blk[0], (blk[1] | blk[2] << 8) - 3, len(blk)

    def rec(k, ip, pos, ssum, acc):
        if k == nseq:
            if ip == n and ssum == want and (pos == BLOCK or (last and 1 <= pos <= BLOCK)):
                yield list(acc)
            return
        if ip + 3 > n:
            return
        tok, S = blk[ip], blk[ip + 1] | blk[ip + 2] << 8
        cands = []
        tl, tm = tok >> 4, tok & 15
        mx = 1 if tm == 15 else 0
        if tl == 15:
            le = 2 if ip + 3 < n and blk[ip + 3] == 255 else 1
            L = S - 5 - le - mx
            ok = L >= 15 and litext(L) == blk[ip + 3:ip + 3 + le]
        else:
            le, L = 0, tl
            ok = S == L + 5 + mx
        lit = ip + 3 + le
        if ok and lit + L + 2 <= n:
            D = blk[lit + L] | blk[lit + L + 1] << 8
            if D == 0:
                if k + 1 == nseq and tm == 0:
                    cands.append(((L, 0, 0), lit + L + 2))
            elif not mx:
                cands.append(((L, D, tm + 4), lit + L + 2))
            elif lit + L + 2 < n:
                cands.append(((L, D, 19 + blk[lit + L + 2]), lit + L + 3))
        if tok >= 0xFD:
            for le in (0, 1, 2):
                L = S - 6 - le
                if L < 0 or len(litext(L)) != le or litext(L) != blk[ip + 3:ip + 3 + le]:
                    continue
                lit = ip + 3 + le
                if lit + L + 2 > n:
                    continue
                D = blk[lit + L] | blk[lit + L + 1] << 8
                if D:
                    cands.append(((L, D, tok - 0xFC), lit + L + 2))
        for seq, nip in cands:
            L, D, M = seq
            if (D and D > pos + L) or pos + L + M > BLOCK or ssum + S > want:
                continue
            acc.append(seq)
            yield from rec(k + 1, nip, pos + L + M, ssum + S, acc)
            acc.pop()

    yield from rec(0, 3, 0, 0, [])


def literals_of(blk, seqs):
    """The literal bytes of a block with a known sequence list, in order."""
    ip, out = 3, bytearray()
    for L, D, M in seqs:
        ip += 3 + len(litext(L))
        out += blk[ip:ip + L]
        ip += L + 2 + (1 if M >= 19 else 0)
    return bytes(out)


def split(stream, offs):
    """The blocks of a stream with known offsets."""
    ends = [1 + o for o in offs[1:]] + [len(stream)]
    return [stream[1 + o:e] for o, e in zip(offs, ends)]


def parse(stream, offs):
    """(block bytes, first consistent reading) per block."""
    blks = split(stream, offs)
    out = []
    for i, b in enumerate(blks):
        r = next(readings(b, last=i + 1 == len(blks)), None)
        if r is None:
            raise FormatError(f"block {i} has no consistent reading")
        out.append((b, r))
    return out


def walk_offsets(stream):
    """Block offsets of a stream without truncated sequences, from the size
    fields alone."""
    offs, x = [], 1
    while x < len(stream):
        offs.append(x - 1)
        x += stream[x + 1] | stream[x + 2] << 8
    if x != len(stream):
        raise FormatError("size fields do not chain to the stream end")
    return offs


# ---- the bare path's candidate rule (lz4_bare_cand) ---------------------------

def _u16(s, a):
    return s[a] | s[a + 1] << 8


def candidate_at(stream, c, x):
    """Does offset x of chunk c's window pass the candidate rule?  A plausible
    header (1 <= nseq, 3 + 5 nseq <= size <= bound, inside the window and the
    stream), nseq size fields hopped as written that end exactly at the
    block's size, and a plausible next header or the stream end."""
    s0 = 1 + c * CHUNK
    avail = min(CAND_WIN, len(stream) - s0)
    if x + 3 > avail:
        return False
    nseq, size = stream[s0 + x], _u16(stream, s0 + x + 1)
    if not (nseq >= 1 and 3 + 5 * nseq <= size <= BLOCK_BOUND and x + size <= avail):
        return False
    y = x + 3
    for _ in range(nseq):
        S = _u16(stream, s0 + y + 1) if y + 3 <= x + size else 0
        if S < 5:
            return False
        y += S
        if y > x + size:
            return False
    if y != x + size:
        return False
    if s0 + x + size < len(stream):
        z = x + size
        return (z + 3 <= avail and stream[s0 + z] >= 1 and
                8 <= _u16(stream, s0 + z + 1) <= BLOCK_BOUND)
    return True


def first_candidate(stream, c):
    """The stream position of chunk c's candidate, or None."""
    if c == 0:
        return 1
    s0 = 1 + c * CHUNK
    avail = min(CAND_WIN, len(stream) - s0)
    for x in range(min(BLOCK_BOUND, avail)):
        if candidate_at(stream, c, x):
            return s0 + x
    return None


BAD = -1


def fast_block_len(stream, x):
    """The fast mode's block length at x: the size field of a plausible
    header, else 0."""
    if x + 3 > len(stream):
        return 0
    size = _u16(stream, x + 1)
    return size if stream[x] >= 1 and 8 <= size <= BLOCK_BOUND and x + size <= len(stream) else 0


def fast_walk(stream, c, x):
    """(exit, block starts) of chunk c walked from x by size fields: the exit
    is the first position at or past the next chunk, or BAD."""
    if x is None:
        return BAD, []
    lim, starts = 1 + (c + 1) * CHUNK, []
    while x < lim and x < len(stream):
        n = fast_block_len(stream, x)
        if n == 0:
            return BAD, starts
        starts.append(x)
        x += n
    return x, starts


def fast_chain(stream):
    """(candidates, exits, inconsistent chunks) as the fast mode's first pass
    finds them: a chunk is inconsistent when its walk dies or does not end on
    the next chunk's candidate (the last chunk's: on the stream end)."""
    nc = nchunks(stream)
    cand = [first_candidate(stream, c) for c in range(nc)]
    ex = [fast_walk(stream, c, cand[c])[0] for c in range(nc)]
    mis = [c for c in range(nc)
           if ex[c] == BAD or ex[c] != (cand[c + 1] if c + 1 < nc else len(stream))]
    return cand, ex, mis


def nchunks(stream):
    return (len(stream) - 1 + CHUNK - 1) // CHUNK


def first_start(offs, c):
    """The first true block start at or after chunk c's first byte (stream
    position), or None."""
    import bisect
    s0 = 1 + c * CHUNK
    i = bisect.bisect_left(offs, s0 - 1)
    return 1 + offs[i] if i < len(offs) else None


def no_repeated_4gram(data):
    seen = set()
    for i in range(len(data) - 3):
        g = data[i:i + 4]
        if g in seen:
            return False
        seen.add(g)
    return True
