/*
 * JPEG_dec -- one image of a JPR1 or JPT1 stream (include/jpegr.h; JPEG_seq's
 * coefficients.jpr, or jpegr_pack_tight_device's output) back to pixels:
 *
 *   JPEG_dec <in.jpr> <out.png> [image [x y w h | thumb]]
 *
 * The dimensions come from the stream's header (jpegr_stream_format); image
 * `image` (default 0) is the tile range [image * tiles, (image + 1) * tiles)
 * of the stream, entropy-decoded straight from the stream's bytes
 * (jpegr_stream_decode_device: no slots) and reconstructed
 * (jpegr_reconstruct_device with no original image: every tile is decoded).
 * With x y w h, only pixels [x, x + w) x [y, y + h) of that image are written,
 * as a w x h PNG, decoded from the tiles they touch and nothing else
 * (jpegr_stream_index_device + jpegr_crop_device); a rectangle outside the
 * image, a zero-sized one or a bad verdict of either call is an error like the
 * others.  With the literal word `thumb` after the image, that image's 1/8-scale
 * thumbnail is written instead, ceil(w / 8) x ceil(h / 8) pixels, one per tile,
 * from the tiles' DC terms alone (jpegr_thumb_device: no coefficients, no
 * IDCT).  Prints nothing on stdout.  Any error -- an unreadable file, a bad header, an
 * image index out of range, an inconsistent stream (verdict other than ~0) or a
 * rejected entropy stream -- is one line on stderr, exit status 1 and no
 * output file.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "../../include/jpegr.h"
#include "lzj_host.h"

static void fail(const char *what) {
  fprintf(stderr, "JPEG_dec: %s\n", what);
  exit(1);
}

static long number(const char *s, const char *what) {
  char *end = NULL;
  const long v = strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < 0) fail(what);
  return v;
}

/* the rectangle alone, through the index and one crop */
static void crop(const void *d_in, size_t flen, int w, int h, int nimg, size_t ntiles, long image,
                 const long r[4], const char *path) {
  if (r[2] == 0 || r[3] == 0) fail("the rectangle is empty");
  if (r[0] > w || r[2] > w - r[0] || r[1] > h || r[3] > h - r[1])
    fail("the rectangle is outside the image");
  const int cw = (int)r[2], ch = (int)r[3];
  const size_t out_b = (size_t)cw * (size_t)ch * 4;
  const jpegr_rect rect = {(uint64_t)image, (uint64_t)r[0], (uint64_t)r[1], (uint64_t)cw,
                           (uint64_t)ch, 0};
  void *d_off = NULL, *d_scr = NULL, *d_cscr = NULL, *d_res = NULL, *d_rect = NULL, *d_px = NULL;
  if (hipMalloc(&d_off, (ntiles + 1) * 8) != hipSuccess ||
      hipMalloc(&d_scr, jpegr_pack_scratch_bytes(ntiles)) != hipSuccess ||
      hipMalloc(&d_cscr, jpegr_crop_scratch_bytes(1, cw, ch)) != hipSuccess ||
      hipMalloc(&d_res, 40) != hipSuccess || hipMalloc(&d_rect, sizeof rect) != hipSuccess ||
      hipMalloc(&d_px, out_b) != hipSuccess)
    fail("device allocation failed");
  if (hipMemcpy(d_rect, &rect, sizeof rect, hipMemcpyHostToDevice) != hipSuccess) fail("copy in");
  uint64_t *const d_ires = d_res, *const d_cres = d_ires + 2;
  if (jpegr_stream_index_device(d_in, flen, w, h, nimg, d_off, d_scr, d_ires, NULL) != JPEGR_OK ||
      jpegr_crop_device(d_in, flen, w, h, nimg, d_off, d_rect, 1, cw, ch, d_px, out_b, d_cscr,
                        d_cres, NULL) != JPEGR_OK)
    fail("kernel launch");
  uint64_t res[5];
  if (hipMemcpy(res, d_res, 40, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (res[1] != ~(uint64_t)0) fail("inconsistent stream (header or index)");
  if (res[3] != ~(uint64_t)0 || res[2] != 1)
    fail("inconsistent stream (a tile record or entropy stream of the rectangle)");
  uint8_t *rgba = malloc(out_b);
  if (!rgba) fail("out of memory");
  if (hipMemcpy(rgba, d_px, out_b, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (lzj_png_write(path, cw, ch, rgba) != 0) {
    remove(path);
    fail("cannot write the PNG");
  }
  (void)hipFree(d_off); (void)hipFree(d_scr); (void)hipFree(d_cscr); (void)hipFree(d_res);
  (void)hipFree(d_rect); (void)hipFree(d_px);
  free(rgba);
}

/* the image's thumbnail, a pixel a tile, through jpegr_thumb_device */
static void thumb(const void *d_in, size_t flen, int w, int h, int nimg, size_t ntiles, long image,
                  const char *path) {
  const int gw = (w + 7) / 8, gh = (h + 7) / 8;
  const size_t out_b = (size_t)gw * (size_t)gh * 4;
  void *d_scr = NULL, *d_res = NULL, *d_px = NULL;
  if (hipMalloc(&d_scr, jpegr_thumb_scratch_bytes(ntiles)) != hipSuccess ||
      hipMalloc(&d_res, 24) != hipSuccess || hipMalloc(&d_px, out_b) != hipSuccess)
    fail("device allocation failed");
  if (jpegr_thumb_device(d_in, flen, w, h, nimg, NULL, (size_t)image, 1, d_px, NULL, d_scr, d_res,
                         NULL) != JPEGR_OK)
    fail("kernel launch");
  uint64_t res[3];
  if (hipMemcpy(res, d_res, 24, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (res[1] != ~(uint64_t)0) fail("inconsistent stream (header, index or a tile record)");
  if (res[2] != 0) fail("malformed entropy stream");
  uint8_t *rgba = malloc(out_b);
  if (!rgba) fail("out of memory");
  if (hipMemcpy(rgba, d_px, out_b, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (lzj_png_write(path, gw, gh, rgba) != 0) {
    remove(path);
    fail("cannot write the PNG");
  }
  (void)hipFree(d_scr); (void)hipFree(d_res); (void)hipFree(d_px);
  free(rgba);
}

int main(int argc, char **argv) {
  const int want_thumb = argc == 5 && strcmp(argv[4], "thumb") == 0;
  if (argc != 3 && argc != 4 && argc != 8 && !want_thumb)
    fail("usage: JPEG_dec <in.jpr> <out.png> [image [x y w h | thumb]]");
  long image = 0, rect[4] = {0, 0, 0, 0};
  if (argc >= 4) image = number(argv[3], "image index is not a number >= 0");
  for (int i = 4; i < argc && !want_thumb; ++i)
    rect[i - 4] = number(argv[i], "x y w h are not numbers >= 0");
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

  int w = 0, h = 0, nimg = 0, format = 0;
  if (jpegr_stream_format(data, &w, &h, &nimg, &format) != JPEGR_OK)
    fail("not a JPR stream (bad header)");
  if (image >= nimg) fail("image index out of range");
  const size_t per = jpegr_coef_count(w, h) / 128;          /* tiles of one image */
  const size_t ntiles = jpegr_pack_bound(w, h, nimg) ? per * (size_t)nimg : 0;
  if (per == 0 || ntiles == 0) fail("not a JPR stream (bad header)");
  const size_t npx = (size_t)w * (size_t)h;

  if (argc == 8 || want_thumb) {
    void *d_stream = NULL;
    if (hipMalloc(&d_stream, (size_t)flen) != hipSuccess) fail("device allocation failed");
    if (hipMemcpy(d_stream, data, (size_t)flen, hipMemcpyHostToDevice) != hipSuccess) fail("copy in");
    if (want_thumb)
      thumb(d_stream, (size_t)flen, w, h, nimg, ntiles, image, argv[2]);
    else
      crop(d_stream, (size_t)flen, w, h, nimg, ntiles, image, rect, argv[2]);
    (void)hipFree(d_stream);
    free(data);
    return 0;
  }

  void *d_in = NULL, *d_coef = NULL, *d_scr = NULL, *d_res = NULL, *d_rgba = NULL;
  if (hipMalloc(&d_in, (size_t)flen) != hipSuccess || hipMalloc(&d_coef, per * 256) != hipSuccess ||
      hipMalloc(&d_scr, jpegr_pack_scratch_bytes(ntiles)) != hipSuccess ||
      hipMalloc(&d_res, 24) != hipSuccess || hipMalloc(&d_rgba, npx * 4) != hipSuccess)
    fail("device allocation failed");
  if (hipMemcpy(d_in, data, (size_t)flen, hipMemcpyHostToDevice) != hipSuccess) fail("copy in");
  if (jpegr_stream_decode_device(d_in, (size_t)flen, w, h, nimg, per * (size_t)image, per, d_coef,
                                 d_scr, d_res, NULL) != JPEGR_OK ||
      jpegr_reconstruct_device(d_coef, NULL, w, h, 1, d_rgba, NULL) != JPEGR_OK)
    fail("kernel launch");
  uint64_t res[3];
  if (hipMemcpy(res, d_res, 24, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (res[1] != ~(uint64_t)0) fail("inconsistent stream (header, index or a tile record)");
  if (res[2] != 0) fail("malformed entropy stream");
  uint8_t *rgba = malloc(npx * 4);
  if (!rgba) fail("out of memory");
  if (hipMemcpy(rgba, d_rgba, npx * 4, hipMemcpyDeviceToHost) != hipSuccess) fail("copy out");
  if (lzj_png_write(argv[2], w, h, rgba) != 0) {
    remove(argv[2]);
    fail("cannot write the PNG");
  }
  (void)hipFree(d_in); (void)hipFree(d_coef); (void)hipFree(d_scr); (void)hipFree(d_res);
  (void)hipFree(d_rgba);
  free(rgba);
  free(data);
  return 0;
}
