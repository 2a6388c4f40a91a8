/* lzj_host.h -- host-side helpers of the drop-in executables and the
 * compatibility layer (not part of the C ABI in include/): PNG I/O over zlib,
 * and the match provider of the per-block LZ4 API. */
#ifndef LZJ_HOST_H
#define LZJ_HOST_H
#include <stddef.h>
#include <stdint.h>

/* RGBA8 pixels of an 8-bit non-interlaced PNG (malloc'd; caller frees).
 * 0 on success, <0 on I/O or format error. */
int lzj_png_read(const char *path, int *w, int *h, uint8_t **rgba);
/* Write w x h RGBA8 pixels as a PNG.  0 on success. */
int lzj_png_write(const char *path, int w, int h, const uint8_t *rgba);

/* The whole file at `path` (malloc'd; caller frees) and its length.  0, or
 * LZJ_FILE_IO when it cannot be opened or read, or LZJ_FILE_NOMEM; *data is
 * NULL then.  host/read_file.c: plain C, not part of the library. */
enum { LZJ_FILE_IO = -1, LZJ_FILE_NOMEM = -2 };
int lzj_read_file(const char *path, uint8_t **data, size_t *len);

/* A .jpr file opened by JPEG_dec or JPEG_sel (host/jpr_file.c): its bytes, the
 * header's fields (jpegr_stream_format), the tiles of one image and of all,
 * and, after lzj_jpr_upload, the stream on the device. */
typedef struct {
  uint8_t *data;
  size_t len;
  int w, h, nimg, format;
  size_t per, ntiles;
  void *d_stream;
} lzj_jpr;
/* Both end the program through lzj_fail on an error.  image: an image the
 * caller will ask for (0: any stream has it), judged right after the header. */
void lzj_jpr_open(const char *path, long image, lzj_jpr *s);
void lzj_jpr_upload(lzj_jpr *s);
void lzj_jpr_close(lzj_jpr *s);

/* How the two programs end on an error: "<lzj_prog>: <what>" as one line on
 * stderr, exit status 1.  main sets lzj_prog first. */
extern const char *lzj_prog;
void lzj_fail(const char *what);
/* `bytes` of device memory, or lzj_fail("device allocation failed"). */
void *lzj_device(size_t bytes);

/* Every position's longest match of the n-byte block at `in` (the
 * reference's find_longest_match, LZ4.c:290-323, matches clamped at the block
 * end): match[p] = len | dist << 16, or 0 when len < 4.  0 or an LZ4R_ERR_*
 * code.  The product's provider runs on the GPU (host/compat.c). */
__attribute__((visibility("hidden"))) int lzj_block_matches(const uint8_t *in, size_t n,
                                                          uint32_t *match);

#endif
