/* lz4f_decode.c -- lz4r_frame_decompress: an exact, bounds-checked host
 * decoder of standard LZ4 frames (LZ4 Frame Format 1.6.x; block format as in
 * lz4_Block_format.md): what lz4r_compress_frame* writes, and what any other
 * LZ4 frame writer does -- linked or independent blocks, stored blocks,
 * content size present or not, header, block and content checksums verified.
 * Concatenated frames decode to the concatenation.  Dictionary IDs, reserved
 * bits, skippable and legacy frames are LZ4R_ERR_CORRUPT.  Nothing outside
 * in[0, in_len) is read and nothing outside out[0, cap) is written. */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lz4r.h"
#include "lz4f_xxh32.h"

#define LZ4F_MAGIC 0x184D2204u

/* a length extension: bytes added until one is below 255 */
static int read_ext(const uint8_t *in, size_t iend, size_t *ip, size_t *len) {
  for (;;) {
    if (*ip >= iend) return -1;
    const uint8_t b = in[(*ip)++];
    *len += b;
    if (b != 255) return 0;
  }
}

/* One compressed block in[ip, iend) -> out from *op on; matches reach back to
 * out[base].  The block may decode to at most bmax bytes.  LZ4R_ERR_CAPACITY
 * leaves the length needed so far in *op. */
static int decode_block(const uint8_t *in, size_t ip, size_t iend, uint8_t *out, size_t cap,
                        size_t base, size_t bmax, size_t *op_io) {
  size_t op = *op_io;
  const size_t bstart = op;
  for (;;) {
    if (ip >= iend) return LZ4R_ERR_CORRUPT;          /* a block ends with a literal run */
    const uint8_t tok = in[ip++];
    size_t L = tok >> 4;
    if (L == 15 && read_ext(in, iend, &ip, &L)) return LZ4R_ERR_CORRUPT;
    if (L > iend - ip || L > bmax - (op - bstart)) return LZ4R_ERR_CORRUPT;
    if (L > cap - op) {
      *op_io = op + L;
      return LZ4R_ERR_CAPACITY;
    }
    if (L) memcpy(out + op, in + ip, L);
    op += L;
    ip += L;
    if (ip == iend) break;                            /* the last sequence: no match */
    if (iend - ip < 2) return LZ4R_ERR_CORRUPT;
    const size_t D = (size_t)in[ip] | (size_t)in[ip + 1] << 8;
    ip += 2;
    size_t M = (size_t)(tok & 15) + 4;
    if ((tok & 15) == 15 && read_ext(in, iend, &ip, &M)) return LZ4R_ERR_CORRUPT;
    if (D == 0 || D > op - base || M > bmax - (op - bstart)) return LZ4R_ERR_CORRUPT;
    if (M > cap - op) {
      *op_io = op + M;
      return LZ4R_ERR_CAPACITY;
    }
    for (size_t i = 0; i < M; ++i, ++op) out[op] = out[op - D];
  }
  *op_io = op;
  return LZ4R_OK;
}

/* One frame at in[*ip_io ...) -> out from *op_io on */
static int decode_frame(const uint8_t *in, size_t in_len, size_t *ip_io, uint8_t *out, size_t cap,
                        size_t *op_io) {
  size_t ip = *ip_io, op = *op_io;
  const size_t fstart = op;
  if (in_len - ip < 7 || lz4f_le32(in + ip) != LZ4F_MAGIC) return LZ4R_ERR_CORRUPT;
  const size_t desc = ip + 4;
  const uint8_t flg = in[desc], bd = in[desc + 1];
  /* version 01; no reserved bit; no dictionary ID */
  if ((flg >> 6) != 1 || (flg & 0x03) || (bd & 0x8F) || (bd >> 4) < 4) return LZ4R_ERR_CORRUPT;
  const int indep = flg & 0x20, bsum = flg & 0x10, csize = flg & 0x08, csum = flg & 0x04;
  const size_t bmax = (size_t)1 << (8 + 2 * (bd >> 4));       /* 64 KiB .. 4 MiB */
  const size_t dlen = 2 + (csize ? 8 : 0);
  if (in_len - desc < dlen + 1) return LZ4R_ERR_CORRUPT;
  uint64_t want = 0;
  for (int i = 0; csize && i < 8; ++i) want |= (uint64_t)in[desc + 2 + i] << (8 * i);
  if (in[desc + dlen] != ((lz4f_xxh32(in + desc, dlen, 0) >> 8) & 0xFF)) return LZ4R_ERR_CORRUPT;
  ip = desc + dlen + 1;
  lz4f_xxh32_state content;
  lz4f_xxh32_init(&content, 0);
  for (;;) {
    if (in_len - ip < 4) return LZ4R_ERR_CORRUPT;
    const uint32_t word = lz4f_le32(in + ip);
    ip += 4;
    if (word == 0) break;                             /* EndMark */
    const size_t bsz = word & 0x7FFFFFFFu;
    if (bsz > bmax || bsz > in_len - ip || (bsum && in_len - ip - bsz < 4))
      return LZ4R_ERR_CORRUPT;
    if (bsum && lz4f_le32(in + ip + bsz) != lz4f_xxh32(in + ip, bsz, 0)) return LZ4R_ERR_CORRUPT;
    const size_t bstart = op;
    if (word & 0x80000000u) {                         /* stored */
      if (bsz > cap - op) {
        *op_io = op + bsz;
        return LZ4R_ERR_CAPACITY;
      }
      if (bsz) memcpy(out + op, in + ip, bsz);
      op += bsz;
    } else {
      const int rc = decode_block(in, ip, ip + bsz, out, cap, indep ? op : fstart, bmax, &op);
      if (rc != LZ4R_OK) {
        *op_io = op;
        return rc;
      }
    }
    if (csum && op > bstart) lz4f_xxh32_update(&content, out + bstart, op - bstart);
    ip += bsz + (bsum ? 4 : 0);
  }
  if (csize && want != (uint64_t)(op - fstart)) return LZ4R_ERR_CORRUPT;
  if (csum) {
    if (in_len - ip < 4 || lz4f_le32(in + ip) != lz4f_xxh32_digest(&content))
      return LZ4R_ERR_CORRUPT;
    ip += 4;
  }
  *ip_io = ip;
  *op_io = op;
  return LZ4R_OK;
}

int lz4r_frame_decompress(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap,
                          size_t *out_len) {
  if (!in || !out_len || (!out && cap)) return LZ4R_ERR_ARG;
  size_t ip = 0, op = 0;
  *out_len = 0;
  if (in_len == 0) return LZ4R_ERR_CORRUPT;           /* no frame at all */
  while (ip < in_len) {
    const int rc = decode_frame(in, in_len, &ip, out, cap, &op);
    if (rc != LZ4R_OK) {
      if (rc == LZ4R_ERR_CAPACITY) *out_len = op;
      return rc;
    }
  }
  *out_len = op;
  return LZ4R_OK;
}
