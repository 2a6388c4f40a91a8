/*
 * LZ4_frame -- a file as a standard LZ4 frame, and back.
 *   LZ4_frame in out.lz4       compress `in` on the GPU (lz4r_compress_frame):
 *                              out.lz4 opens with `lz4 -d` and every other LZ4
 *                              frame reader
 *   LZ4_frame -d in.lz4 out    decode on the host (lz4r_frame_decompress): any
 *                              standard frame, or several concatenated
 *   LZ4_frame -D in.lz4 out    the same on the GPU (lz4r_frame_decompress_gpu)
 * Any error is one line on stderr and exit status 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lz4r.h"
#include "lzj_host.h"

static void fail(const char *what, const char *detail) {
  fprintf(stderr, "LZ4_frame: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
  exit(1);
}

static void write_file(const char *path, const uint8_t *data, size_t len) {
  FILE *f = fopen(path, "wb");
  if (!f) fail("cannot open for writing", path);
  const size_t put = len ? fwrite(data, 1, len, f) : 0;
  if (fclose(f) != 0 || put != len) fail("cannot write", path);
}

int main(int argc, char **argv) {
  const int gpu = argc == 4 && strcmp(argv[1], "-D") == 0;
  const int decode = gpu || (argc == 4 && strcmp(argv[1], "-d") == 0);
  if (!decode && argc != 3)
    fail("usage: LZ4_frame in out.lz4 | LZ4_frame -d in.lz4 out | LZ4_frame -D in.lz4 out", NULL);
  const char *src = argv[decode ? 2 : 1], *dst = argv[decode ? 3 : 2];
  uint8_t *in = NULL;
  size_t n = 0;
  if (lzj_read_file(src, &in, &n) != 0) fail("cannot read", src);
  uint8_t *out = NULL;
  size_t got = 0;
  int rc;
  if (gpu) {
    /* with no room the decoder names the decoded length, exactly */
    rc = lz4r_frame_decompress_gpu(in, n, NULL, 0, &got, 0);
    if (rc == LZ4R_ERR_CAPACITY) {
      const size_t cap = got;
      out = (uint8_t *)malloc(cap);
      if (!out) fail("out of memory", NULL);
      rc = lz4r_frame_decompress_gpu(in, n, out, cap, &got, 0);
    }
  } else if (decode) {
    /* the decoder names the length needed so far: grow until it fits */
    size_t cap = 4 * n + 65536;
    for (;;) {
      out = (uint8_t *)malloc(cap ? cap : 1);
      if (!out) fail("out of memory", NULL);
      rc = lz4r_frame_decompress(in, n, out, cap, &got);
      if (rc != LZ4R_ERR_CAPACITY) break;
      free(out);
      cap = got > 2 * cap ? got : 2 * cap;
    }
  } else {
    const size_t cap = lz4r_frame_bound(n);
    out = (uint8_t *)malloc(cap);
    if (!out) fail("out of memory", NULL);
    rc = lz4r_compress_frame(in, n, out, cap, &got);
  }
  if (rc != LZ4R_OK) fail(decode ? "cannot decode" : "cannot compress", lz4r_strerror(rc));
  write_file(dst, out, got);
  free(out);
  free(in);
  return 0;
}
