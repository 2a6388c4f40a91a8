// lz4f_parse.h -- how a standard LZ4 frame is read, written once: the frame
// descriptor's check, the walk over the block size words, the sequence reader
// of a compressed block with every bound it can apply without looking at
// history, and a block's decode on top of it.  Everything lz4r_frame_decompress
// (host/lz4f_decode.c) calls corrupt on these levels is corrupt here.
//
// Plain C++ with no HIP in it: the functions are __host__ __device__ under
// hipcc (the kernels of lz4f_dec.h instantiate them over an LDS window) and
// ordinary inline functions in a host compiler (tests/sanitize/
// frame_dev_main.cpp instantiates them over plain memory under ASan + UBSan).
//
//   Src   where the frame's bytes come from:  uint32_t at(size_t i)
//   Sink  what the walk found:                block(i, entry), frame(i, entry)
//   Out   the copies of a decode:             literals(op, ip, L), match(op, D, M)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../host/lz4f_xxh32.h"

#if defined(__HIPCC__)
#define LZ4F_HD __host__ __device__ inline
#else
#define LZ4F_HD inline
#endif

#define LZ4F_MAGIC 0x184D2204u

// One data block, as the walk found it.  `word`: the byte count in bits 0-22
// (at most 4 MiB) and what the decoder needs of its frame beside it.
struct Lz4fBlock {
  uint64_t in_off;                 // the block's first byte (after its size word)
  uint32_t word;
  uint32_t frame;                  // the index of its frame
};
constexpr uint32_t kLz4fBytes = 0x007FFFFFu;
constexpr uint32_t kLz4fStored = 1u << 31;      // as in the frame's size word
constexpr uint32_t kLz4fLinked = 1u << 30;      // its frame's blocks are linked
constexpr uint32_t kLz4fBsum = 1u << 29;        // a block checksum follows at in_off + bytes
constexpr int kLz4fBmaxShift = 27;              // bits 27-28: block maximum 64 KiB << 2 k

LZ4F_HD uint32_t lz4f_block_bytes(uint32_t word) { return word & kLz4fBytes; }
LZ4F_HD uint32_t lz4f_block_max(uint32_t word) {
  return 65536u << (2 * ((word >> kLz4fBmaxShift) & 3u));
}

// One frame, as the walk found it
struct Lz4fFrame {
  uint64_t first_block, nblocks;   // its data blocks in the index
  uint64_t want;                   // the content size its header states (has_want)
  uint64_t csum_pos;               // where its content checksum sits (has_csum)
  uint32_t has_want, has_csum;
};

template <class Src>
LZ4F_HD uint32_t lz4f_src_le32(Src &s, size_t i) {
  return s.at(i) | s.at(i + 1) << 8 | s.at(i + 2) << 16 | s.at(i + 3) << 24;
}

// The frame header at ip: magic, FLG, BD, the content size, HC.  0, or -1
// for what the host decoder calls corrupt (skippable and legacy magics,
// another version, a reserved bit, a dictionary ID, a block maximum below
// 64 KiB, a wrong header checksum, a truncated header).
struct Lz4fDesc {
  uint32_t flg, bd;
  uint64_t want;
  size_t data;                     // the first block size word
};

template <class Src>
LZ4F_HD int lz4f_read_desc(Src &s, size_t in_len, size_t ip, Lz4fDesc *d) {
  if (in_len - ip < 7 || lz4f_src_le32(s, ip) != LZ4F_MAGIC) return -1;
  const size_t desc = ip + 4;
  const uint32_t flg = s.at(desc), bd = s.at(desc + 1);
  if ((flg >> 6) != 1 || (flg & 0x03) || (bd & 0x8F) || (bd >> 4) < 4) return -1;
  const size_t dlen = 2 + ((flg & 0x08) ? 8 : 0);
  if (in_len - desc < dlen + 1) return -1;
  uint8_t hdr[10];
  for (size_t i = 0; i < dlen; ++i) hdr[i] = (uint8_t)s.at(desc + i);
  uint64_t want = 0;
  for (size_t i = 2; i < dlen; ++i) want |= (uint64_t)hdr[i] << (8 * (i - 2));
  if (s.at(desc + dlen) != ((lz4f_xxh32(hdr, dlen, 0) >> 8) & 0xFF)) return -1;
  d->flg = flg;
  d->bd = bd;
  d->want = want;
  d->data = desc + dlen + 1;
  return 0;
}

// The block size word at ip of a frame with this block maximum: 1 and *word
// for a data block, 0 for the EndMark, -1 for a truncated word, a size
// beyond the block maximum or the input, or no room for its checksum.
template <class Src>
LZ4F_HD int lz4f_read_block_word(Src &s, size_t in_len, size_t ip, uint32_t bmax, bool bsum,
                                 uint32_t *word) {
  if (in_len - ip < 4) return -1;
  const uint32_t w = lz4f_src_le32(s, ip);
  ip += 4;
  if (w == 0) return 0;
  const size_t bsz = w & 0x7FFFFFFFu;
  if (bsz > bmax || bsz > in_len - ip || (bsum && in_len - ip - bsz < 4)) return -1;
  *word = w;
  return 1;
}

// Frame after frame to the input's end: one Sink::block per data block, one
// Sink::frame per frame, in order (the Sink may drop entries beyond its room:
// the counts are exact all the same).  0, or -1 on the first thing corrupt.
template <class Src, class Sink>
LZ4F_HD int lz4f_walk_frames(Src &s, size_t in_len, Sink &k, uint64_t *nblocks, uint64_t *nframes,
                             uint64_t *nsums) {
  size_t ip = 0;
  uint64_t nb = 0, nf = 0, ns = 0;
  if (in_len == 0) return -1;                         // no frame at all
  while (ip < in_len) {
    Lz4fDesc d;
    if (lz4f_read_desc(s, in_len, ip, &d)) return -1;
    ip = d.data;
    const bool bsum = (d.flg & 0x10) != 0;
    const uint32_t code = (d.bd >> 4) - 4;
    const uint32_t bmax = 65536u << (2 * code);
    const uint32_t tag = ((d.flg & 0x20) ? 0u : kLz4fLinked) | (bsum ? kLz4fBsum : 0u) |
                         code << kLz4fBmaxShift;
    Lz4fFrame f;
    f.first_block = nb;
    f.want = d.want;
    f.has_want = (d.flg & 0x08) != 0;
    f.has_csum = (d.flg & 0x04) != 0;
    for (;;) {
      uint32_t w = 0;
      const int r = lz4f_read_block_word(s, in_len, ip, bmax, bsum, &w);
      if (r < 0) return -1;
      ip += 4;
      if (r == 0) break;
      Lz4fBlock b;
      b.in_off = ip;
      b.word = (w & (kLz4fStored | kLz4fBytes)) | tag;
      b.frame = (uint32_t)nf;
      k.block(nb++, b);
      ip += (w & 0x7FFFFFFFu) + (bsum ? 4 : 0);
    }
    f.nblocks = nb - f.first_block;
    f.csum_pos = ip;
    if (f.has_csum) {
      if (in_len - ip < 4) return -1;
      ip += 4;
      ++ns;
    }
    k.frame(nf++, f);
  }
  *nblocks = nb;
  *nframes = nf;
  *nsums = ns;
  return 0;
}

// a length extension: bytes added until one is below 255
template <class Src>
LZ4F_HD int lz4f_read_ext(Src &s, size_t iend, size_t *ip, size_t *len) {
  for (;;) {
    if (*ip >= iend) return -1;
    const uint32_t b = s.at((*ip)++);
    *len += b;
    if (b != 255) return 0;
  }
}

// One sequence of the block that ends at iend, which may still decode `room`
// bytes: L literals at `lit`, then a match of M at distance D (M 0: the
// block's last sequence, which has none).  -1: an extension runs past the end,
// L beyond the block's remaining bytes, fewer than two bytes left for a
// distance, no last literal run, D 0, or more than `room` decoded.
struct Lz4fSeq {
  size_t lit;
  uint32_t L, D, M;
};

template <class Src>
LZ4F_HD int lz4f_read_seq(Src &s, size_t *ip_io, size_t iend, uint32_t room, Lz4fSeq *q) {
  size_t ip = *ip_io;
  if (ip >= iend) return -1;                          // a block ends with a literal run
  const uint32_t tok = s.at(ip++);
  size_t L = tok >> 4;
  if (L == 15 && lz4f_read_ext(s, iend, &ip, &L)) return -1;
  if (L > iend - ip || L > room) return -1;
  q->lit = ip;
  q->L = (uint32_t)L;
  q->D = 0;
  q->M = 0;
  ip += L;
  if (ip != iend) {
    if (iend - ip < 2) return -1;
    const uint32_t D = s.at(ip) | s.at(ip + 1) << 8;
    ip += 2;
    size_t M = (size_t)(tok & 15) + 4;
    if ((tok & 15) == 15 && lz4f_read_ext(s, iend, &ip, &M)) return -1;
    if (D == 0 || M > room - L) return -1;
    q->D = D;
    q->M = (uint32_t)M;
  }
  *ip_io = ip;
  return 0;
}

// What the compressed block in[ip, iend) decodes to, from its tokens alone
template <class Src>
LZ4F_HD int lz4f_block_size(Src &s, size_t ip, size_t iend, uint32_t bmax, uint32_t *size) {
  uint32_t n = 0;
  Lz4fSeq q;
  do {
    if (lz4f_read_seq(s, &ip, iend, bmax - n, &q)) return -1;
    n += q.L + q.M;
  } while (q.M);
  *size = n;
  return 0;
}

// The compressed block in[ip, iend) to the output from *op on and no further
// than `end`; matches reach back to `base` (the block's own start, or its
// frame's when the blocks are linked).  -1 also for a D beyond the base.  A
// block that fails may have written part of [*op, end).
template <class Src, class Out>
LZ4F_HD int lz4f_decode_block(Src &s, size_t ip, size_t iend, Out &o, size_t base, size_t *op_io,
                              size_t end) {
  size_t op = *op_io;
  Lz4fSeq q;
  do {
    if (lz4f_read_seq(s, &ip, iend, (uint32_t)(end - op), &q)) return -1;
    o.literals(op, q.lit, q.L);
    op += q.L;
    if (q.M) {
      if (q.D > op - base) return -1;
      o.match(op, q.D, q.M);
      op += q.M;
    }
  } while (q.M);
  *op_io = op;
  return 0;
}
