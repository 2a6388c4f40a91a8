/*
 * JPEG_dec -- one image of a JPR1 or JPT1 stream (include/jpegr.h; JPEG_seq's
 * coefficients.jpr, or jpegr_pack_tight_device's output) back to pixels:
 *
 *   JPEG_dec <in.jpr> <out.png> [image]
 *
 * The dimensions come from the stream's header (jpegr_stream_format); image
 * `image` (default 0) is the tile range [image * tiles, (image + 1) * tiles)
 * of the stream, entropy-decoded straight from the stream's bytes
 * (jpegr_stream_decode_device: no slots) and reconstructed
 * (jpegr_reconstruct_device with no original image: every tile is decoded).
 * Prints nothing on stdout.  Any error -- an unreadable file, a bad header, an
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

int main(int argc, char **argv) {
  if (argc < 3 || argc > 4) fail("usage: JPEG_dec <in.jpr> <out.png> [image]");
  long image = 0;
  if (argc == 4) {
    char *end = NULL;
    image = strtol(argv[3], &end, 10);
    if (end == argv[3] || *end != '\0' || image < 0) fail("image index is not a number >= 0");
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

  int w = 0, h = 0, nimg = 0, format = 0;
  if (jpegr_stream_format(data, &w, &h, &nimg, &format) != JPEGR_OK)
    fail("not a JPR stream (bad header)");
  if (image >= nimg) fail("image index out of range");
  const size_t per = jpegr_coef_count(w, h) / 128;          /* tiles of one image */
  const size_t ntiles = jpegr_pack_bound(w, h, nimg) ? per * (size_t)nimg : 0;
  if (per == 0 || ntiles == 0) fail("not a JPR stream (bad header)");
  const size_t npx = (size_t)w * (size_t)h;

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
