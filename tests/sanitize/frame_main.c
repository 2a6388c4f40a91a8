/*
 * frame_main.c -- TEST INFRASTRUCTURE ONLY: host/lz4f_decode.c under ASan +
 * UBSan (`make sanitize-frame`; tests/test_sanitize_frame.py).  A stand-alone
 * program: it builds a small frame of two linked blocks with block and
 * content checksums, decodes it, then every proper prefix and every
 * single-byte mutation of it, each from a heap copy of exactly its length into
 * a heap buffer of exactly cap bytes, so a read or write one byte outside is
 * the sanitizer's to report.  Prints "sanitize-frame ok".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lz4r.h"
#include "../../lz4-jpeg_amd/host/lz4f_xxh32.h"

static void put32(uint8_t *p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

/* block 1: 26 literals, a match of 30 at distance 26, 6 literals;
 * block 2 (linked): a match of 20 at distance 62 after 1 literal, 11 literals */
static const char kText1[] = "abcdefghijklmnopqrstuvwxyz";
static size_t build(uint8_t *f, uint8_t *plain, size_t *plain_len) {
  size_t n = 0, p = 0;
  const uint8_t fixed[6] = {0x04, 0x22, 0x4D, 0x18, 0x54, 0x40};   /* linked, block + content sums */
  memcpy(f, fixed, 6);
  f[6] = (uint8_t)(lz4f_xxh32(f + 4, 2, 0) >> 8);
  n = 7;
  /* block 1 */
  uint8_t b[128];
  size_t k = 0;
  b[k++] = 0xFF;                       /* L = 15 + 11, ML = 4 + 15 + 11 */
  b[k++] = 11;
  memcpy(b + k, kText1, 26);
  k += 26;
  b[k++] = 26;
  b[k++] = 0;
  b[k++] = 11;
  b[k++] = 0x60;
  memcpy(b + k, "STUVWX", 6);
  k += 6;
  put32(f + n, (uint32_t)k);
  memcpy(f + n + 4, b, k);
  put32(f + n + 4 + k, lz4f_xxh32(b, k, 0));
  n += 8 + k;
  memcpy(plain, kText1, 26);
  p = 26;
  for (int i = 0; i < 30; ++i, ++p) plain[p] = plain[p - 26];
  memcpy(plain + p, "STUVWX", 6);
  p += 6;
  /* block 2 */
  k = 0;
  b[k++] = 0x1F;                       /* L = 1, ML = 4 + 15 + 1 */
  b[k++] = '#';
  b[k++] = 63;
  b[k++] = 0;
  b[k++] = 1;
  b[k++] = 0xB0;
  memcpy(b + k, "0123456789!", 11);
  k += 11;
  put32(f + n, (uint32_t)k);
  memcpy(f + n + 4, b, k);
  put32(f + n + 4 + k, lz4f_xxh32(b, k, 0));
  n += 8 + k;
  plain[p++] = '#';
  for (int i = 0; i < 20; ++i, ++p) plain[p] = plain[p - 63];
  memcpy(plain + p, "0123456789!", 11);
  p += 11;
  put32(f + n, 0);
  put32(f + n + 4, lz4f_xxh32(plain, p, 0));
  n += 8;
  *plain_len = p;
  return n;
}

/* decode a heap copy of exactly len bytes into exactly cap bytes */
static int run(const uint8_t *frame, size_t len, size_t cap, uint8_t **out, size_t *got) {
  uint8_t *in = (uint8_t *)malloc(len ? len : 1);
  *out = (uint8_t *)malloc(cap ? cap : 1);
  if (!in || !*out) abort();
  memcpy(in, frame, len);
  const int rc = lz4r_frame_decompress(in, len, *out, cap, got);
  free(in);
  return rc;
}

int main(void) {
  uint8_t frame[256], plain[256], *out;
  size_t plain_len = 0, got = 0;
  const size_t n = build(frame, plain, &plain_len);
  int rc = run(frame, n, plain_len, &out, &got);
  if (rc != LZ4R_OK || got != plain_len || memcmp(out, plain, plain_len) != 0) {
    fprintf(stderr, "the frame does not decode: rc %d, %zu bytes\n", rc, got);
    return 1;
  }
  free(out);
  for (size_t cap = 0; cap < plain_len; ++cap) {
    rc = run(frame, n, cap, &out, &got);
    free(out);
    if (rc != LZ4R_ERR_CAPACITY || got <= cap) {
      fprintf(stderr, "cap %zu: rc %d, need %zu\n", cap, rc, got);
      return 1;
    }
  }
  for (size_t k = 0; k < n; ++k) {
    rc = run(frame, k, plain_len, &out, &got);
    free(out);
    if (rc != LZ4R_ERR_CORRUPT) {
      fprintf(stderr, "prefix %zu: rc %d\n", k, rc);
      return 1;
    }
  }
  size_t errors = 0;
  for (size_t i = 0; i < n; ++i)
    for (int v = 0; v < 256; ++v) {
      if (v == frame[i]) continue;
      uint8_t bad[256];
      memcpy(bad, frame, n);
      bad[i] = (uint8_t)v;
      rc = run(bad, n, plain_len, &out, &got);
      const int same = rc == LZ4R_OK && got == plain_len && memcmp(out, plain, plain_len) == 0;
      free(out);
      if (rc == LZ4R_OK && !same) {
        fprintf(stderr, "mutation %zu -> %d decodes to other bytes\n", i, v);
        return 1;
      }
      errors += rc != LZ4R_OK;
    }
  printf("sanitize-frame ok (%zu bytes, %zu prefixes, %zu mutations rejected)\n", n, n, errors);
  return 0;
}
