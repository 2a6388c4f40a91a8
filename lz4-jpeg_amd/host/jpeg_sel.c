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
#include "lzj_host.h"

static void usage(void) {
  lzj_fail("usage: JPEG_sel <in.jpr> <out.jpr> <jpr|jpt|same> images <i>... | tiles <w> <h> <image:x:y>...");
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
  lzj_prog = "JPEG_sel";
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
  if (!items) lzj_fail("out of memory");
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

  lzj_jpr s;
  lzj_jpr_open(argv[1], 0, &s);
  const int w = s.w, h = s.h, nimg = s.nimg;
  if (by_image) {
    ow = (uint64_t)w;
    oh = (uint64_t)h;
  }
  if (ow == 0 || oh == 0 || ow > (uint64_t)w || oh > (uint64_t)h) lzj_fail("the window is not inside the image");
  const int out_w = (int)ow, out_h = (int)oh;
  const size_t scr_b = jpegr_select_scratch_bytes(nitems, out_w, out_h);
  if (scr_b == 0) lzj_fail("too many tiles");

  lzj_jpr_upload(&s);
  void *const d_off = lzj_device((s.ntiles + 1) * 8);
  void *const d_iscr = lzj_device(jpegr_pack_scratch_bytes(s.ntiles));
  void *const d_scr = lzj_device(scr_b), *const d_res = lzj_device(48);
  void *const d_items = lzj_device(nitems * sizeof *items), *d_out = lzj_device(16);
  if (hipMemcpy(d_items, items, nitems * sizeof *items, hipMemcpyHostToDevice) != hipSuccess)
    lzj_fail("copy in");
  /* d_res: the index call's two words, the select call's three, its length */
  uint64_t *const d_ires = d_res, *const d_sres = d_ires + 2, *const d_len = d_ires + 5;
  uint64_t res[6];
  /* once into no room at all for the length, once more into exactly that */
  if (jpegr_stream_index_device(s.d_stream, s.len, w, h, nimg, d_off, d_iscr, d_ires, NULL) != JPEGR_OK ||
      jpegr_select_device(s.d_stream, s.len, w, h, nimg, d_off, d_items, nitems, out_w, out_h, format,
                          d_out, 0, d_len, d_scr, d_sres, NULL) != JPEGR_OK)
    lzj_fail("kernel launch");
  if (hipMemcpy(res, d_res, 48, hipMemcpyDeviceToHost) != hipSuccess) lzj_fail("copy out");
  if (res[1] != ~(uint64_t)0) lzj_fail("inconsistent stream (header or index)");
  if (res[3] != ~(uint64_t)0) lzj_fail("a bad item (an image past the stream's, or a window that is not tile-aligned inside it)");
  if (res[4] != 0) lzj_fail("inconsistent stream (a tile record)");
  const size_t need = (size_t)res[5];
  (void)hipFree(d_out);
  d_out = lzj_device(need);
  if (jpegr_select_device(s.d_stream, s.len, w, h, nimg, d_off, d_items, nitems, out_w, out_h, format,
                          d_out, need, d_len, d_scr, d_sres, NULL) != JPEGR_OK)
    lzj_fail("kernel launch");
  if (hipMemcpy(res, d_res, 48, hipMemcpyDeviceToHost) != hipSuccess) lzj_fail("copy out");
  if (res[3] != ~(uint64_t)0 || res[4] != 0 || res[5] != (uint64_t)need) lzj_fail("inconsistent stream");
  uint8_t *bytes = malloc(need);
  if (!bytes) lzj_fail("out of memory");
  if (hipMemcpy(bytes, d_out, need, hipMemcpyDeviceToHost) != hipSuccess) lzj_fail("copy out");
  FILE *g = fopen(argv[2], "wb");
  if (!g) lzj_fail("cannot write the output file");
  const int wrote = fwrite(bytes, 1, need, g) == need;
  if (fclose(g) != 0 || !wrote) {
    remove(argv[2]);
    lzj_fail("cannot write the output file");
  }
  (void)hipFree(d_off); (void)hipFree(d_iscr); (void)hipFree(d_scr);
  (void)hipFree(d_res); (void)hipFree(d_items); (void)hipFree(d_out);
  free(bytes);
  free(items);
  lzj_jpr_close(&s);
  return 0;
}
