/* read_file.c -- lzj_read_file (lzj_host.h).  Plain C with no HIP: the
 * executables link it, and so does the sanitizer program of `make sanitize`. */
#include <stdio.h>
#include <stdlib.h>

#include "lzj_host.h"

int lzj_read_file(const char *path, uint8_t **data, size_t *len) {
  *data = NULL;
  *len = 0;
  FILE *f = fopen(path, "rb");
  if (!f) return LZJ_FILE_IO;
  int rc = LZJ_FILE_IO;
  long n = -1;
  if (fseek(f, 0, SEEK_END) == 0 && (n = ftell(f)) >= 0 && fseek(f, 0, SEEK_SET) == 0) {
    uint8_t *b = malloc(n > 0 ? (size_t)n : 1);
    if (b && fread(b, 1, (size_t)n, f) == (size_t)n) {
      *data = b;
      *len = (size_t)n;
      rc = 0;
    } else {
      rc = b ? LZJ_FILE_IO : LZJ_FILE_NOMEM;
      free(b);
    }
  }
  fclose(f);
  return rc;
}
