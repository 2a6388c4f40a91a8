/* jpr_file.c -- what JPEG_dec and JPEG_sel share (lzj_host.h): how they end on
 * an error, and how they open a .jpr file: the file, its header and what
 * follows from it, and the stream on the device.  Linked into the executables
 * only, not into the library. */
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "../../include/jpegr.h"
#include "lzj_host.h"

const char *lzj_prog = "";

void lzj_fail(const char *what) {
  fprintf(stderr, "%s: %s\n", lzj_prog, what);
  exit(1);
}

void *lzj_device(size_t bytes) {
  void *d = NULL;
  if (hipMalloc(&d, bytes) != hipSuccess) lzj_fail("device allocation failed");
  return d;
}

void lzj_jpr_open(const char *path, long image, lzj_jpr *s) {
  *s = (lzj_jpr){0};
  const int rc = lzj_read_file(path, &s->data, &s->len);
  if (rc != 0) lzj_fail(rc == LZJ_FILE_NOMEM ? "out of memory" : "cannot read the input file");
  if (s->len < 16) lzj_fail("shorter than a JPR header");
  if (jpegr_stream_format(s->data, &s->w, &s->h, &s->nimg, &s->format) != JPEGR_OK)
    lzj_fail("not a JPR stream (bad header)");
  if (image >= s->nimg) lzj_fail("image index out of range");
  s->per = jpegr_coef_count(s->w, s->h) / 128;
  s->ntiles = jpegr_pack_bound(s->w, s->h, s->nimg) ? s->per * (size_t)s->nimg : 0;
  if (s->per == 0 || s->ntiles == 0) lzj_fail("not a JPR stream (bad header)");
}

void lzj_jpr_upload(lzj_jpr *s) {
  s->d_stream = lzj_device(s->len);
  if (hipMemcpy(s->d_stream, s->data, s->len, hipMemcpyHostToDevice) != hipSuccess)
    lzj_fail("copy in");
}

void lzj_jpr_close(lzj_jpr *s) {
  (void)hipFree(s->d_stream);
  free(s->data);
}
