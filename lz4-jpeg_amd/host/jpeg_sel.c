/*
 * JPEG_sel -- a new JPR1 or JPT1 stream from images or tile windows of one
 * (include/jpegr.h: jpegr_select_device; nothing is decoded):
 *
 *   JPEG_sel <in.jpr> <out.jpr> <jpr|jpt|same> images <i>...
 *   JPEG_sel <in.jpr> <out.jpr> <jpr|jpt|same> tiles <w> <h> <image:x:y>...
 *
 * `images`: the listed images whole, in the order given (repeats allowed).
 * `tiles`: one w x h image per item, the tile grid of `image` that starts at
 * pixel (x, y), both multiples of 8.  jpr, jpt: the output's format (JPR1,
 * JPT1); same: the input's.  The dimensions come from the input's header
 * (jpegr_stream_format) and the records' offsets from its index
 * (jpegr_stream_index_device).  Prints nothing on stdout.  Any error -- an
 * unreadable file, a bad header or index, a bad item (d_result[1] != ~0) or a
 * bad tile (d_result[2] != 0) -- is one line on stderr, exit status 1 and no
 * output file; any other argument form is a usage error, reported the same way.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../../include/jpegr.h"

static void fail(const char *what) {
  fprintf(stderr, "JPEG_sel: %s\n", what);
  exit(1);
}

static void usage(void) {
  fail("usage: JPEG_sel <in.jpr> <out.jpr> <jpr|jpt|same> images <i>... | tiles <w> <h> <image:x:y>...");
}

/* a decimal number >= 0 that ends at `end` (a character of the caller's) */
static uint64_t number(const char **s, char end) {
  char *stop = NULL;
  if (**s < '0' || **s > '9') usage();
  const unsigned long long v = strtoull(*s, &stop, 10);
  if (*stop != end) usage();
  *s = stop + (end != '\0');
  return (uint64_t)v;
}

int main(int argc, char **argv) {
  if (argc < 6) usage();
  int format = -1;
  if (strcmp(argv[3], "jpr") == 0) format = JPEGR_STREAM_JPR1;
  if (strcmp(argv[3], "jpt") == 0) format = JPEGR_STREAM_JPT1;
  if (strcmp(argv[3], "same") == 0) format = 0;
  const int by_image = strcmp(argv[4], "images") == 0, by_tile = strcmp(argv[4], "tiles") == 0;
  if (format < 0 || (!by_image && !by_tile) || (by_tile && argc < 8)) usage();
  const int first = by_image ? 5 : 7;
  const size_t nitems = (size_t)(argc - first);
  jpegr_sel *items = calloc(nitems, sizeof *items);
  if (!items) fail("out of memory");
  uint64_t ow = 0, oh = 0;
  if (by_tile) {
    const char *a = argv[5], *b = argv[6];
    ow = number(&a, '\0');
    oh = number(&b, '\0');
  }
  for (size_t k = 0; k < nitems; ++k) {
    const char *a = argv[first + (int)k];
    if (by_image) {
      items[k].image = number(&a, '\0');
    } else {
      items[k].image = number(&a, ':');
      items[k].x = number(&a, ':');
      items[k].y = number(&a, '\0');
    }
  }

  FILE *f = fopen(argv[1], "rb");
  if (!f) fail("cannot read the input file");
  if (fseek(f, 0, SEEK_END) != 0) fail("cannot read the input file");
  const long flen = ftell(f);
  if (flen < 0 || fseek(f, 0, SEEK_SET) != 0) fail("cannot read the input file");
  if (flen < 16) fail("shorter than a JPR header");
  uint8_t *data = malloc((size_t)flen);
  if (!data) fail("out of memory");
  if (fread(data, 1, (size_t)flen, f) != (size_t)flen) fail("cannot read the input file");
  fclose(f);

  int w = 0, h = 0, nimg = 0, in_format = 0;
  if (jpegr_stream_format(data, &w, &h, &nimg, &in_format) != JPEGR_OK)
    fail("not a JPR stream (bad header)");
  const size_t per = jpegr_coef_count(w, h) / 128;          /* tiles of one image */
  const size_t ntiles = jpegr_pack_bound(w, h, nimg) ? per * (size_t)nimg : 0;
  if (per == 0 || ntiles == 0) fail("not a JPR stream (bad header)");
  if (by_image) {
    ow = (uint64_t)w;
    oh = (uint64_t)h;
  }
  if (ow == 0 || oh == 0 || ow > (uint64_t)w || oh > (uint64_t)h) fail("the window is not inside the image");
  const int out_w = (int)ow, out_h = (int)oh;
  const size_t scr_b = jpegr_select_scratch_bytes(nitems, out_w, out_h);
  if (scr_b == 0) fail("too many tiles");

  void *d_in = NULL, *d_off = NULL, *d_iscr = NULL, *d_scr = NULL, *d_res = NULL, *d_items = NULL,
       *d_out = NULL;
  if (hipMalloc(&d_in, (size_t)flen) != hipSuccess || hipMalloc(&d_off, (ntiles + 1) * 8) != hipSuccess ||
      hipMalloc(&d_iscr, jpegr_pack_scratch_bytes(ntiles)) != hipSuccess ||
      hipMalloc(&d_scr, scr_b) != hipSuccess || hipMalloc(&d_res, 48) != hipSuccess ||
      hipMalloc(&d_items, nitems * sizeof *items) != hipSuccess || hipMalloc(&d_out, 16) != hipSuccess)
    fail("device allocation failed");
  if (hipMemcpy(d_in, data, (size_t)flen, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_items, items, nitems * sizeof *items, hipMemcpyHostToDevice) != hipSuccess)
    fail("copy in");
  /* d_res: the index call's two words, the select call's three, its length */
  uint64_t *const d_ires = d_res, *const d_sres = d_ires + 2, *const d_len = d_ires + 5;
  uint64_t res[6];
  /* once into no room at all for the length, once more into exactly that */
  if (jpegr_stream_index_device(d_in, (size_t)flen, w, h, nimg, d_off, d_iscr, d_ires, NULL) != JPEGR_OK ||
      jpegr_select_device(d_in, (size_t)flen, w, h, nimg, d_off, d_items, nitems, out_w, out_h, format,
                          d_out, 0, d_len, d_scr, d_sres, NULL) != JPEGR_OK)
    fail("kernel launch");
  if (hipMemcpy(res, d_res, 48, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (res[1] != ~(uint64_t)0) fail("inconsistent stream (header or index)");
  if (res[3] != ~(uint64_t)0) fail("a bad item (an image past the stream's, or a window that is not tile-aligned inside it)");
  if (res[4] != 0) fail("inconsistent stream (a tile record)");
  const size_t need = (size_t)res[5];
  (void)hipFree(d_out);
  if (hipMalloc(&d_out, need) != hipSuccess) fail("device allocation failed");
  if (jpegr_select_device(d_in, (size_t)flen, w, h, nimg, d_off, d_items, nitems, out_w, out_h, format,
                          d_out, need, d_len, d_scr, d_sres, NULL) != JPEGR_OK)
    fail("kernel launch");
  if (hipMemcpy(res, d_res, 48, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (res[3] != ~(uint64_t)0 || res[4] != 0 || res[5] != (uint64_t)need) fail("inconsistent stream");
  uint8_t *bytes = malloc(need);
  if (!bytes) fail("out of memory");
  if (hipMemcpy(bytes, d_out, need, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  FILE *g = fopen(argv[2], "wb");
  if (!g) fail("cannot write the output file");
  const int wrote = fwrite(bytes, 1, need, g) == need;
  if (fclose(g) != 0 || !wrote) {
    remove(argv[2]);
    fail("cannot write the output file");
  }
  (void)hipFree(d_in); (void)hipFree(d_off); (void)hipFree(d_iscr); (void)hipFree(d_scr);
  (void)hipFree(d_res); (void)hipFree(d_items); (void)hipFree(d_out);
  free(bytes);
  free(items);
  free(data);
  return 0;
}
