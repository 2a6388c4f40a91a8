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

static long number(const char *s, const char *what) {
  char *end = NULL;
  const long v = strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < 0) lzj_fail(what);
  return v;
}

/* pixels on the device to a PNG file, or no file */
static void write_png(const void *d_px, int pw, int ph, const char *path) {
  const size_t out_b = (size_t)pw * (size_t)ph * 4;
  uint8_t *rgba = malloc(out_b);
  if (!rgba) lzj_fail("out of memory");
  if (hipMemcpy(rgba, d_px, out_b, hipMemcpyDeviceToHost) != hipSuccess) lzj_fail("copy out");
  if (lzj_png_write(path, pw, ph, rgba) != 0) {
    remove(path);
    lzj_fail("cannot write the PNG");
  }
  free(rgba);
}

/* the rectangle alone, through the index and one crop */
static void crop(const lzj_jpr *s, long image, const long r[4], const char *path) {
  if (r[2] == 0 || r[3] == 0) lzj_fail("the rectangle is empty");
  if (r[0] > s->w || r[2] > s->w - r[0] || r[1] > s->h || r[3] > s->h - r[1])
    lzj_fail("the rectangle is outside the image");
  const int cw = (int)r[2], ch = (int)r[3];
  const size_t out_b = (size_t)cw * (size_t)ch * 4;
  const jpegr_rect rect = {(uint64_t)image, (uint64_t)r[0], (uint64_t)r[1], (uint64_t)cw,
                           (uint64_t)ch, 0};
  void *const d_off = lzj_device((s->ntiles + 1) * 8);
  void *const d_scr = lzj_device(jpegr_pack_scratch_bytes(s->ntiles));
  void *const d_cscr = lzj_device(jpegr_crop_scratch_bytes(1, cw, ch)), *const d_res = lzj_device(40);
  void *const d_rect = lzj_device(sizeof rect), *const d_px = lzj_device(out_b);
  if (hipMemcpy(d_rect, &rect, sizeof rect, hipMemcpyHostToDevice) != hipSuccess) lzj_fail("copy in");
  uint64_t *const d_ires = d_res, *const d_cres = d_ires + 2;
  if (jpegr_stream_index_device(s->d_stream, s->len, s->w, s->h, s->nimg, d_off, d_scr, d_ires,
                                NULL) != JPEGR_OK ||
      jpegr_crop_device(s->d_stream, s->len, s->w, s->h, s->nimg, d_off, d_rect, 1, cw, ch, d_px,
                        out_b, d_cscr, d_cres, NULL) != JPEGR_OK)
    lzj_fail("kernel launch");
  uint64_t res[5];
  if (hipMemcpy(res, d_res, 40, hipMemcpyDeviceToHost) != hipSuccess) lzj_fail("copy out");
  if (res[1] != ~(uint64_t)0) lzj_fail("inconsistent stream (header or index)");
  if (res[3] != ~(uint64_t)0 || res[2] != 1)
    lzj_fail("inconsistent stream (a tile record or entropy stream of the rectangle)");
  write_png(d_px, cw, ch, path);
  (void)hipFree(d_off); (void)hipFree(d_scr); (void)hipFree(d_cscr); (void)hipFree(d_res);
  (void)hipFree(d_rect); (void)hipFree(d_px);
}

/* the image's thumbnail, a pixel a tile, through jpegr_thumb_device */
static void thumb(const lzj_jpr *s, long image, const char *path) {
  const int gw = (s->w + 7) / 8, gh = (s->h + 7) / 8;
  void *const d_scr = lzj_device(jpegr_thumb_scratch_bytes(s->ntiles)), *const d_res = lzj_device(24);
  void *const d_px = lzj_device((size_t)gw * (size_t)gh * 4);
  if (jpegr_thumb_device(s->d_stream, s->len, s->w, s->h, s->nimg, NULL, (size_t)image, 1, d_px,
                         NULL, d_scr, d_res, NULL) != JPEGR_OK)
    lzj_fail("kernel launch");
  uint64_t res[3];
  if (hipMemcpy(res, d_res, 24, hipMemcpyDeviceToHost) != hipSuccess) lzj_fail("copy out");
  if (res[1] != ~(uint64_t)0) lzj_fail("inconsistent stream (header, index or a tile record)");
  if (res[2] != 0) lzj_fail("malformed entropy stream");
  write_png(d_px, gw, gh, path);
  (void)hipFree(d_scr); (void)hipFree(d_res); (void)hipFree(d_px);
}

/* the whole image: its tile range decoded straight from the stream, then reconstructed */
static void whole(const lzj_jpr *s, long image, const char *path) {
  void *const d_coef = lzj_device(s->per * 256), *const d_res = lzj_device(24);
  void *const d_scr = lzj_device(jpegr_pack_scratch_bytes(s->ntiles));
  void *const d_rgba = lzj_device((size_t)s->w * (size_t)s->h * 4);
  if (jpegr_stream_decode_device(s->d_stream, s->len, s->w, s->h, s->nimg, s->per * (size_t)image,
                                 s->per, d_coef, d_scr, d_res, NULL) != JPEGR_OK ||
      jpegr_reconstruct_device(d_coef, NULL, s->w, s->h, 1, d_rgba, NULL) != JPEGR_OK)
    lzj_fail("kernel launch");
  uint64_t res[3];
  if (hipMemcpy(res, d_res, 24, hipMemcpyDeviceToHost) != hipSuccess) lzj_fail("copy out");
  if (res[1] != ~(uint64_t)0) lzj_fail("inconsistent stream (header, index or a tile record)");
  if (res[2] != 0) lzj_fail("malformed entropy stream");
  write_png(d_rgba, s->w, s->h, path);
  (void)hipFree(d_coef); (void)hipFree(d_scr); (void)hipFree(d_res); (void)hipFree(d_rgba);
}

int main(int argc, char **argv) {
  lzj_prog = "JPEG_dec";
  const int want_thumb = argc == 5 && strcmp(argv[4], "thumb") == 0;
  if (argc != 3 && argc != 4 && argc != 8 && !want_thumb)
    lzj_fail("usage: JPEG_dec <in.jpr> <out.png> [image [x y w h | thumb]]");
  long image = 0, rect[4] = {0, 0, 0, 0};
  if (argc >= 4) image = number(argv[3], "image index is not a number >= 0");
  for (int i = 4; i < argc && !want_thumb; ++i)
    rect[i - 4] = number(argv[i], "x y w h are not numbers >= 0");
  lzj_jpr s;
  lzj_jpr_open(argv[1], image, &s);
  lzj_jpr_upload(&s);
  if (want_thumb)
    thumb(&s, image, argv[2]);
  else if (argc == 8)
    crop(&s, image, rect, argv[2]);
  else
    whole(&s, image, argv[2]);
  lzj_jpr_close(&s);
  return 0;
}
