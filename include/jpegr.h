/*
 * jpegr.h -- C ABI of the MI355X JPEG hot path (colour conversion, 4:2:2
 * odd-column subsampling, 8x8/8x4 tiling, fp64 DCT-II, truncating
 * quantisation, zigzag), bit-exact to the reference's sequential C.
 *
 * Replaces, for a whole image (or a batch of images) at once, the reference's
 * per-tile host loop in Algorithms/sequential/JPEG/JPEG.c:
 *   build_luminance_matrix / build_rChrominance_matrix /
 *   build_bChrominance_matrix   JPEG.c:114-185
 *   chroma_subsample            JPEG.c:302-375
 *   divide_image                JPEG.c:496-550
 *   discrete_cosine_transform   JPEG.c:451-494
 *   Quantize                    JPEG.c:621-629
 *   zigzag_pattern              JPEG.c:693-728
 *   (driven by main, JPEG.c:1110-1178)
 *
 * Input: RGBA8 pixels, row-major, 4 bytes/pixel (the reference's Pixel,
 * JPEG.c:29-32; alpha ignored).  Output: per 8x8 tile, 128 int16
 * little-endian = [Y 64 zigzag][Cr 32 zigzag][Cb 32 zigzag]; tiles in raster
 * order (this layout is defined by this library: the reference keeps the
 * quantised coefficients as doubles in memory).  Pixels outside the image
 * read as 0, as divide_image's zero-initialised tiles do (JPEG.c:512-523).
 *
 * No torch types; device pointers are plain `void *` from hipMalloc (or a
 * torch tensor's data_ptr()), `stream` is a hipStream_t (NULL = default).
 * All functions return JPEGR_OK (0) or a negative JPEGR_ERR_* code.
 */
#ifndef JPEGR_H
#define JPEGR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPEGR_OK 0
#define JPEGR_ERR_ARG (-1)     /* bad dimensions / NULL pointer */
#define JPEGR_ERR_HIP (-2)     /* HIP runtime error (no GPU, launch failure) */
#define JPEGR_ERR_NOMEM (-3)   /* device allocation failed */

/* Number of int16 coefficients one w x h image produces: tiles * 128. */
size_t jpegr_coef_count(int w, int h);

/* Device API, asynchronous on `stream`.  `nimg` images of identical size,
 * contiguous (image i at d_rgba + i*w*h*4, output at d_out + i*coef_count).
 * Geometry, for these two calls and jpegr_reconstruct_device: w, h > 0, nimg
 * of 1 .. 65,535 (a grid's y extent), and at most 2^31 - 1 workgroups in x --
 * ceil(h / 8) tile rows times ceil(ceil(w / 8) / 32) strips of 32 tiles.
 * Pointers: d_rgba 4-B aligned (a pixel is loaded as a dword, four of them as
 * one 16-B load at dword alignment where w is a multiple of 4; a base that is
 * 4-B but not 16-B aligned is inside the contract); d_out_i16 16-B aligned
 * (uint4 stores); d_out_f64 8-B aligned.  A NULL pointer, a geometry outside
 * the above or a misaligned pointer: JPEGR_ERR_ARG before any HIP call.  No
 * read leaves the nimg * w * h * 4 input bytes and no write leaves the nimg *
 * jpegr_coef_count(w, h) output elements, whatever w and h are (pinned with
 * guard bands by tests/test_gpu_jpeg_geometry.py). */
int jpegr_encode_device(const void *d_rgba, int w, int h, int nimg,
                        void *d_out_i16, void *stream);

/* Same tiles, but the un-quantised fp64 DCT coefficients in row-major
 * (u*W+v) order per plane: [Y 64][Cr 32][Cb 32] doubles per tile.  This is
 * the value discrete_cosine_transform (JPEG.c:451) leaves in *coefficients;
 * exposed for bit-exact parity checks. */
int jpegr_dct_raw_device(const void *d_rgba, int w, int h, int nimg,
                         void *d_out_f64, void *stream);

/* Host convenience: copies in, runs on the current device, copies out,
 * synchronises.  `out` holds jpegr_coef_count(w, h) int16. */
int jpegr_encode(const uint8_t *rgba, int w, int h, int16_t *out);

/* Event-timed device run for measurement: runs jpegr_encode_device `iters`
 * times on `stream` bracketed by HIP events recorded on that same stream and
 * returns the mean milliseconds per launch in *ms_per_launch. */
int jpegr_time_device(const void *d_rgba, int w, int h, int nimg,
                      void *d_out_i16, int iters, void *stream,
                      float *ms_per_launch);

/* Reconstruction (the decode side of the reference's main, JPEG.c:1131-1425;
 * the RLE/Huffman round trip there is the identity on the coefficients):
 * per tile, reverse zigzag + Inverse_quantize (:631-638), fp64 IDCT in the
 * reference's order with (int)round(x + 128) clamped (:399-448), and
 * assemble_image's YCbCr 4:2:2 -> RGB (:553-619), RGBA8 out (a = 255).
 * d_coef is jpegr_encode_device's layout.  Tiles at raster index >=
 * ceil(w*h/64) are never transformed by the reference (:1131) and keep their
 * original samples: pass the source image as d_rgba_orig to reproduce that
 * (NULL decodes them like the others).  Asynchronous on `stream`.
 * d_coef holds any int16 (the stream decoders deliver any): the largest sample
 * magnitude stays below 2^26, so the rounding is defined for all of them.
 * Geometry as for jpegr_encode_device.  d_coef 16-B aligned (uint4 loads);
 * d_rgba_orig, when given, and d_rgba_out 4-B aligned (dword stores, 16-B
 * stores only where the address allows).  A NULL d_coef or d_rgba_out, a bad
 * geometry or a misaligned pointer: JPEGR_ERR_ARG before any HIP call.  No
 * write leaves the nimg * w * h * 4 bytes at d_rgba_out. */
int jpegr_reconstruct_device(const void *d_coef, const void *d_rgba_orig, int w, int h,
                             int nimg, void *d_rgba_out, void *stream);

/* Block-level kernels (jpegr_blocks.hip) behind the reference-named API in
 * lz4jpeg_compat.h, asynchronous on `stream`:
 *   jpegr_planes_device: full-resolution uint8 Y, Cr, Cb planes of an RGBA8
 *     image (build_luminance_matrix / build_r,bChrominance_matrix,
 *     JPEG.c:114-185), w*h bytes each.
 *   jpegr_dct_blocks_device: discrete_cosine_transform (JPEG.c:451-494) of
 *     nblocks planar uint8 blocks of `height` rows x `width` columns
 *     (width 8 or 4, height 8), fp64 out, u*width+v order.
 *   jpegr_quantize_device: Quantize (JPEG.c:621-629) in place on n doubles,
 *     element i divided by table[i % size] (fp64 table) and truncated.
 *   jpegr_permute_device: out[i] = in[(i/size)*size + perm[i%size]] for n
 *     doubles (zigzag_pattern, JPEG.c:693-728, with perm = its scan order).
 *     n need not be a multiple of size: elements at and past n are not
 *     written (nor, by quantize, read); permute reads `in` inside the last
 *     block it starts, so `in` holds whole blocks.
 * Pointers: jpegr_planes_device's d_rgba 4-B aligned, its three planes any
 * alignment; jpegr_dct_blocks_device's d_blocks any alignment, d_out_f64 8-B
 * aligned; the fp64 arrays of quantize and permute 8-B aligned, d_perm_i32
 * 4-B aligned.  A NULL pointer, w, h, nblocks or size <= 0, n == 0, a width
 * other than 8 and 4, a height other than 8, or a misaligned pointer:
 * JPEGR_ERR_ARG before any HIP call. */
int jpegr_planes_device(const void *d_rgba, int w, int h, void *d_y, void *d_cr,
                        void *d_cb, void *stream);
int jpegr_dct_blocks_device(const void *d_blocks, int width, int height, int nblocks,
                            void *d_out_f64, void *stream);
int jpegr_quantize_device(void *d_coef_f64, const void *d_table_f64, int size,
                          size_t n, void *stream);
int jpegr_permute_device(const void *d_in_f64, void *d_out_f64, const void *d_perm_i32,
                         int size, size_t n, void *stream);

const char *jpegr_strerror(int code);

/* Entropy stage (JPEG.c:767-1097, run by main at :1211-1349): per tile and
 * channel -- Y 64, Cr 32, Cb 32 zigzagged ints in jpegr_encode_device's
 * layout -- the RLE (count, value) ints (RLE, :767), the per-stream Huffman
 * code exactly as encode_huffman builds it (first-occurrence frequencies
 * :864, heap :895-936, tree :938 with its append-without-sift-up, DFS codes
 * :964), and the encoded sequence (:993).  Output per tile (ntiles = all
 * tiles of all images):
 *   d_bits   256 B: [Y 128][Cr 64][Cb 64] bytes, bits packed MSB-first
 *            (the reference's '0'/'1' chars); the final byte's unused low
 *            bits are 0, bytes past it unspecified
 *   d_meta   3 u32 (Y, Cr, Cb): nbits | rle_len << 16 | ncodes << 24
 *   d_table  256 u32: [Y 128][Cr 64][Cb 64]; entry k = value (int16) |
 *            code length << 16, in the reference's codes[] (DFS) order;
 *            the codes follow from the lengths: code[0] = 0, code[k] =
 *            (code[k-1] + 1) shifted left (or right) to length len[k]
 * d_coef 16-B aligned; d_bits 4-B aligned to encode, d_bits and d_table
 * 16-B aligned to decode (JPEGR_ERR_ARG otherwise).
 * d_scratch: jpegr_entropy_scratch_bytes(ntiles) device bytes.  d_status:
 * 3 u32 on the device, shared by both calls; [0] = streams whose code or
 * sequence would overflow the reference's char code[32] / sequence[1024|512]
 * buffers (undefined behaviour there; truncated here).  Asynchronous on
 * `stream`. */
size_t jpegr_entropy_scratch_bytes(size_t ntiles);
int jpegr_entropy_encode_device(const void *d_coef, size_t ntiles, void *d_bits,
                                void *d_meta, void *d_table, void *d_scratch,
                                void *d_status, void *stream);

/* Inverse: bits + table -> RLE ints (decode_huffman, :1009; a one-code
 * stream has an empty sequence and stands for rle_len copies of its symbol,
 * which the reference keeps in its RLE array) -> ints (inverse_RLE, :810:
 * counts clamped to the stream length, zero fill), written in
 * jpegr_encode_device's layout.  d_status[1] = malformed streams, set by
 * the call itself (no memset needed); d_status[2] is the call's tag, which
 * orders the kernel's own zeroing of [1] before any count is added (keep it
 * to the library; one decode at a time per status array). */
int jpegr_entropy_decode_device(const void *d_bits, const void *d_meta,
                                const void *d_table, size_t ntiles, void *d_coef,
                                void *d_status, void *stream);

/* The JPR stream: the entropy stage's output as one self-contained byte
 * stream (this library defines it; all fields little-endian, no padding):
 *   header   16 B   'J' 'P' 'R' '1' | u32 w | u32 h | u32 nimg
 *   index    2 B x ntiles   u16 size of each tile record, raster order,
 *                           images in sequence; ntiles = nimg * ceil(w/8) *
 *                           ceil(h/8)
 *   records  tile 0, tile 1, ...   each = stream(Y) stream(Cr) stream(Cb)
 *   stream   u8 rle_len | u8 ncodes | u16 nbits   (the meta word's fields)
 *            ncodes x { i16 value, u8 code_length }   the low 24 bits of
 *                           d_table's words, in the table's (DFS) order
 *            ceil(nbits / 8) bytes of bits, copied from the slot
 * Only those bytes are copied: slot bytes past the final byte and table
 * entries past ncodes do not reach the stream.  The slots bound a luma
 * stream by ncodes <= 128, nbits <= 1024 (4 + 384 + 128 = 516 B) and a
 * chroma stream by 64 and 512 (260 B): a tile record is at most 1,036 B.
 * Stream length = 16 + 2 ntiles + the sum of the sizes; a record's offset is
 * the exclusive scan of the index, so the stream decodes in parallel with no
 * side input.
 *
 * jpegr_pack_bound: 16 + ntiles * (2 + 1036), 0 on bad dimensions.
 * jpegr_pack_scratch_bytes: device scratch of either call below (16-B
 * aligned).
 * jpegr_pack_device: asynchronous on `stream`, no host read-back, nothing
 * kept on the host between calls (capturable in a graph).  Stores a u64 at
 * d_out_len (8-B aligned): the stream length, or the capacity needed when
 * that exceeds `cap`, in which case nothing at or past d_out + cap is
 * written.  d_out 16-B aligned; d_bits / d_meta / d_table as the entropy
 * encoder leaves them.  A meta field past its slot is clamped to it.  Bad
 * pointers or dimensions, or more than 2^32 tiles: JPEGR_ERR_ARG before any
 * HIP call.
 * jpegr_stream_info (host only): w, h, nimg of a header's 16 bytes;
 * JPEGR_ERR_ARG on a wrong magic or a zero dimension.
 * jpegr_unpack_device: the inverse, asynchronous on `stream`: every tile's
 * meta word, its ncodes table entries and its bit bytes (whole dwords; the
 * last one's spare bytes 0) back in the slot layout, for
 * jpegr_entropy_decode_device as it is.  d_result: two u64 on the device,
 *   [0] the length the header and index imply
 *   [1] ~0 when the stream is consistent; 0 when the header or index is
 *       wrong (magic, dimensions other than the arguments, in_len <
 *       16 + 2 ntiles, implied length != in_len; every tile's meta is then
 *       0); else 1 + t for the first tile t whose record is malformed (a
 *       stream's rle_len, ncodes or nbits past its slot, or three streams
 *       that do not sum to the indexed size); such a tile's meta words are 0
 *       (ncodes = 0), the other tiles unpack.
 * No read leaves [d_in, d_in + in_len) and every write stays inside its
 * tile's slots, whatever the bytes say. */
size_t jpegr_pack_bound(int w, int h, int nimg);
size_t jpegr_pack_scratch_bytes(size_t ntiles);
int jpegr_pack_device(const void *d_bits, const void *d_meta, const void *d_table,
                      int w, int h, int nimg, void *d_out, size_t cap,
                      void *d_out_len, void *d_scratch, void *stream);
int jpegr_stream_info(const uint8_t header[16], int *w, int *h, int *nimg);
int jpegr_unpack_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                        void *d_bits, void *d_meta, void *d_table,
                        void *d_scratch, void *d_result, void *stream);

/* Entropy decode straight from a JPR stream, whole or by tile range: tiles
 * [tile0, tile0 + ntile) of the stream in d_in[0, in_len) -- numbered in
 * raster order through all images, as the index numbers them; image i of a
 * stream is the range [i * tiles, (i + 1) * tiles) -- to ntile * 128 int16 at
 * d_coef in jpegr_encode_device's layout, tile tile0 + i at d_coef + 128 i.
 * No slots are allocated, written or read.  Asynchronous on `stream`, no host
 * read-back, nothing kept on the host between calls.
 * d_scratch: jpegr_pack_scratch_bytes(tiles of the whole stream) bytes, 16-B
 * aligned (the index scan is pack's and unpack's).  d_coef 16-B aligned; d_in
 * as for jpegr_unpack_device (any alignment).  NULL pointers, bad dimensions,
 * ntile == 0, tile0 + ntile past the stream's tile count, more than 2^32
 * tiles, a misaligned d_coef, d_scratch or d_result: JPEGR_ERR_ARG before any
 * HIP call.
 * d_result: three u64 on the device (8-B aligned), initialised by the call's
 * own first launch -- no memset before it, no tag, no spin: the call can be
 * captured in a graph and replayed, and several calls may be in flight at
 * once, each with its own d_result and d_scratch.
 *   [0] the length the header and index imply (as jpegr_unpack_device)
 *   [1] ~0 when consistent; 0 when the header or index is wrong (unpack's
 *       conditions, against the w, h, nimg arguments; every selected tile's
 *       128 ints are then 0); else 1 + t for the first tile t in
 *       [tile0, tile0 + ntile) whose record is malformed (unpack's record
 *       rules; t counts from the stream's first tile).  A malformed record's
 *       128 ints are 0; records outside the range are not examined.
 *   [2] the streams inside the range, in well-formed records, that the
 *       entropy decoder rejects (what jpegr_entropy_decode_device counts in
 *       d_status[1]): this call's count, never accumulated.  A rejected
 *       stream's 64 or 32 ints are 0; every other stream decodes exactly.
 * Whatever the bytes say, no read leaves [d_in, d_in + in_len) and no write
 * leaves [d_coef, d_coef + 256 ntile) and the scratch: table entries and bit
 * bytes are read at byte granularity inside their own checked record, never
 * as chunks that reach into the next record or past the end. */
int jpegr_stream_decode_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                               size_t tile0, size_t ntile, void *d_coef,
                               void *d_scratch, void *d_result, void *stream);

/* The JPT1 stream: JPR1 with a tighter table coding.  Header ('J' 'P' 'T' '1'
 * in place of the magic), u16 index, record order (Y, Cr, Cb), offsets by the
 * exclusive scan of the index and little-endian fields are JPR1's.  A stream:
 *   u8 rle_len | u8 ncodes | u16 f        nbits = f & 0x3FFF, mode = f >> 14
 *   table, by mode:
 *     0  ncodes x { i16 value, u8 code_length }            (JPR1's entries)
 *     1  ceil(ncodes / 2) length bytes, then ncodes x i8 value
 *     2  ceil(ncodes / 2) length bytes, then ncodes x i16 value
 *     3  malformed
 *   ceil(nbits / 8) bytes of bits, as JPR1
 * Entry k's code length is the low nibble of length byte k / 2 for even k, the
 * high nibble for odd k; with an odd ncodes the last high nibble is written
 * as 0 and ignored by readers.  Entries are in the table's (DFS) order and the
 * codes follow from the lengths as stated for d_table above; bits 24..31 of a
 * table word do not reach the stream.
 * The writer's mode is canonical, so the bytes are deterministic: mode 1 when
 * ncodes > 0, every length is <= 15 and every value is in -128..127; else
 * mode 2 when ncodes > 0 and every length is <= 15; else mode 0 (a meta field
 * past its slot is clamped first, as in jpegr_pack_device).  Readers accept
 * any of modes 0..2 on any stream.  A mode-0 stream is byte for byte a JPR1
 * stream, and modes 1 and 2 are never longer: a record is at most 1,036 B,
 * jpegr_pack_bound serves both formats, and the record rules are JPR1's (a
 * stream's rle_len, ncodes or nbits past its slot, a mode of 3, or three
 * streams that do not sum to the indexed size: malformed).
 *
 * jpegr_pack_tight_device: jpegr_pack_device's arguments and contract
 * (asynchronous, no read-back, no host state, capturable; a u64 length or
 * needed capacity at d_out_len; nothing written at or past cap; JPEGR_ERR_ARG
 * before any HIP call), writing a JPT1 stream.  d_scratch:
 * jpegr_pack_scratch_bytes.
 * jpegr_stream_format (host only): w, h, nimg and the format of a header's 16
 * bytes, JPEGR_STREAM_JPR1 or JPEGR_STREAM_JPT1; JPEGR_ERR_ARG on any other
 * magic, a zero dimension or a NULL pointer.  jpegr_stream_info keeps
 * rejecting everything but JPR1.
 * jpegr_stream_decode_device takes either format, told by the magic, with
 * every guarantee above.  jpegr_unpack_device does not: a JPT1 stream is a
 * wrong magic to it (verdict 0), so slots from a JPT1 stream are not offered,
 * and decompress_device (lz4jpeg.jpeg) raises on one. */
#define JPEGR_STREAM_JPR1 1
#define JPEGR_STREAM_JPT1 2
int jpegr_pack_tight_device(const void *d_bits, const void *d_meta, const void *d_table,
                            int w, int h, int nimg, void *d_out, size_t cap,
                            void *d_out_len, void *d_scratch, void *stream);
int jpegr_stream_format(const uint8_t header[16], int *w, int *h, int *nimg, int *format);

/* Entropy encode straight to a stream, with no slots: d_coef in
 * jpegr_encode_device's layout (16-B aligned; ntiles = nimg * ceil(w/8) *
 * ceil(h/8)) to the bytes that jpegr_entropy_encode_device followed by
 * jpegr_pack_device (format JPEGR_STREAM_JPR1) or jpegr_pack_tight_device
 * (JPEGR_STREAM_JPT1) writes -- the canonical modes, the deferred streams and
 * the clamping of a stream that overflows the reference's buffers included --
 * from a scratch of about the stream's own size instead of 1,292 B of slots
 * per tile.
 * jpegr_pack_device's contract holds: asynchronous on `stream`, no host
 * read-back, nothing kept on the host between calls (capturable in a graph, a
 * replay re-initialises every counter itself); a u64 at d_out_len (8-B
 * aligned): the stream length, or the exact capacity needed when that exceeds
 * `cap`, in which case d_out[0, cap) still holds the stream's first cap bytes
 * and nothing at or past d_out + cap is written; d_out 16-B aligned.  NULL
 * pointers, bad dimensions, more than 2^32 tiles, a format other than the two,
 * a misaligned d_coef, d_out, d_out_len, d_scratch (16 B) or d_result (8 B):
 * JPEGR_ERR_ARG before any HIP call.
 * d_result: two u64 on the device, initialised by the call itself in stream
 * order:
 *   [0] the length again
 *   [1] the streams that overflow the reference's char code[32] /
 *       sequence[1024|512] buffers (d_status[0] of the slot encoder): this
 *       call's count, never accumulated
 * d_scratch: jpegr_stream_encode_scratch_bytes(ntiles, cap) bytes, at most
 * cap + 128 ntiles + 4096 and monotone in both arguments (the finished
 * streams lie in a dense arena sized from cap, behind a directory of 24 B per
 * tile).  Several calls may be in flight at once, each with its own scratch
 * and result.  Whatever the coefficients say, no write leaves d_out[0, cap),
 * the scratch and the result words.  When cap is short of the stream, the
 * streams that the arena had no room for and that start below cap are encoded
 * a second time, a lane each, straight to d_out; otherwise that last launch
 * exits at once. */
size_t jpegr_stream_encode_scratch_bytes(size_t ntiles, size_t cap);
int jpegr_stream_encode_device(const void *d_coef, int w, int h, int nimg, int format,
                               void *d_out, size_t cap, void *d_out_len,
                               void *d_scratch, void *d_result, void *stream);

/* Random access: many rectangles of a JPR1 or JPT1 stream's images in one
 * call, each decoded from the tiles it touches and from nothing else.  Tile
 * records are independent and every tile carries its own Y, Cr and Cb, so a
 * crop needs only its own tiles' records -- and their offsets, which
 * jpegr_stream_index_device computes once for any number of crop calls.
 *
 * jpegr_stream_index_device: the index scan of pack, unpack and the direct
 * decode, kept: ntiles + 1 u64 at d_tile_offsets (8-B aligned), entry t the
 * byte offset of tile t's record from the start of the stream, entry ntiles
 * the length the header and index imply.  Takes either format.  d_scratch:
 * jpegr_pack_scratch_bytes(ntiles) bytes, 16-B aligned.  d_result: two u64
 * (8-B aligned), initialised by the call's own first launch:
 *   [0] the implied length
 *   [1] ~0 when the header is a JPR1 or JPT1 header for w, h, nimg and the
 *       implied length equals in_len; else 0
 * Asynchronous on `stream`, no host read-back, nothing kept on the host
 * (capturable).  NULL pointers, bad dimensions, more than 2^32 tiles, a
 * misaligned d_tile_offsets, d_scratch or d_result: JPEGR_ERR_ARG before any
 * HIP call.  No read leaves d_in[0, in_len).
 *
 * jpegr_crop_device: rectangle r of d_rects[0, nrects) (8-B aligned) is pixels
 * [x, x + w) x [y, y + h) of image `image`, delivered as RGBA8 rows of 4 w
 * bytes, back to back, at d_out + dst (d_out 4-B aligned).  It is decoded from
 * tile columns x / 8 .. (x + w - 1) / 8 and tile rows y / 8 .. (y + h - 1) / 8
 * of its image only, and its bytes equal that rectangle of what
 * jpegr_stream_decode_device + jpegr_reconstruct_device(d_rgba_orig = NULL)
 * give for the image (every tile transformed, alpha 255).
 * Mapping: every rectangle occupies K = jpegr_crop_items(max_w, max_h) =
 * (ceil(max_w / 8) + 1) * (ceil(max_h / 8) + 1) items, one per tile that a
 * max_w x max_h crop can touch at any position, whatever its own size: group
 * crops of similar size per call, a small crop in a call with a large max_w or
 * max_h idles most of its items.  nrects * K may not exceed 2^28 (2^22
 * workgroups of 64 items, one launch): JPEGR_ERR_ARG past that.
 * d_tile_offsets: jpegr_stream_index_device's, ntiles + 1 u64; caller memory
 * and not trusted.  d_scratch: jpegr_crop_scratch_bytes(nrects, max_w, max_h)
 * bytes, 16-B aligned: 256 B x K x nrects of coefficients in rectangle-local
 * tile grids, then a status word per rectangle (0 on a zero or overflowing
 * argument).  d_result: three u64 (8-B aligned), reset by the call's own first
 * launch -- no memset, no tag, no spin:
 *   [0] the rectangles delivered
 *   [1] ~0 when every rectangle was delivered, else 1 + the index of the
 *       first bad rectangle
 *   [2] the tile records and entropy streams found malformed or rejected among
 *       the tiles visited (diagnostic: a tile shared by two rectangles counts
 *       twice, tiles of a rectangle already found bad may go unvisited): this
 *       call's count, never accumulated
 * A rectangle is bad when image >= nimg; w > max_w or h > max_h; x + w > the
 * image's width or y + h > its height; dst is not a multiple of 4; dst + 4 w h
 * > out_cap (none of the sums wraps); the stream's header is not a JPR1 or
 * JPT1 header for w, h, nimg (every rectangle is bad then); or a tile it
 * touches has offsets that are not off[t] <= off[t + 1] <= in_len with a size
 * of 12 .. 1,036 B, a record the record rules reject, or a stream the entropy
 * decoder rejects.  w == 0 or h == 0 is a good rectangle that writes nothing,
 * whatever its other fields say.  Good rectangles are delivered exactly,
 * whatever the bad ones do.  A rectangle that fails on its own fields or on
 * the header writes nothing; one that fails inside a tile may leave
 * unspecified bytes in its own 4 w h output bytes.  Overlapping destination
 * ranges hold unspecified bytes.
 * Whatever the stream, the offsets and the rectangles say, no read leaves
 * d_in[0, in_len), d_tile_offsets[0, ntiles] and d_rects[0, nrects), and no
 * write leaves d_result, the scratch and each rectangle's own output bytes
 * within out_cap; table entries and bit bytes are read at byte granularity
 * inside the checked record, as by jpegr_stream_decode_device.
 * Asynchronous on `stream`, no host read-back, nothing kept on the host
 * (capturable); several calls may be in flight at once, each with its own
 * scratch and result.  JPEGR_ERR_ARG before any HIP call: a NULL pointer; bad
 * dimensions or more than 2^32 tiles; nrects, max_w or max_h of 0, max_w > w,
 * max_h > h; in_len < 16; d_rects, d_tile_offsets or d_result not 8-B aligned,
 * d_scratch not 16-B aligned, d_out not 4-B aligned; nrects * K > 2^28. */
typedef struct jpegr_rect { uint64_t image, x, y, w, h, dst; } jpegr_rect;

int jpegr_stream_index_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                              void *d_tile_offsets, void *d_scratch, void *d_result,
                              void *stream);
size_t jpegr_crop_items(int max_w, int max_h);
size_t jpegr_crop_scratch_bytes(size_t nrects, int max_w, int max_h);
int jpegr_crop_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                      const void *d_tile_offsets, const void *d_rects, size_t nrects,
                      int max_w, int max_h, void *d_out, size_t out_cap,
                      void *d_scratch, void *d_result, void *stream);

/* jpegr_crop_tensor_device: jpegr_crop_device's rectangles delivered as what a
 * model reads -- three channels, planar or interleaved, in its dtype,
 * normalised, optionally mirrored -- in the same three launches.  d_rects
 * (jpegr_rect as above), d_tile_offsets (untrusted), the K =
 * jpegr_crop_items(max_w, max_h) mapping, the scratch
 * (jpegr_crop_scratch_bytes), the three result words and the good / bad /
 * empty rules are jpegr_crop_device's, with one difference: dst and out_cap
 * count ELEMENTS of the output dtype from d_out (16-B aligned).  A rectangle
 * occupies 3 w h elements; it is bad when dst + 3 w h > out_cap (no sum
 * wraps); no dst is misaligned, an element offset being element-aligned.  Wide
 * stores are taken only where the address allows: odd w, or a dst that is not
 * a multiple of 16 B, is inside the contract.
 * Values: channel c (0 R, 1 G, 2 B; alpha dropped) of crop pixel (i, j) is the
 * byte v that jpegr_crop_device delivers there.  JPEGR_DTYPE_U8: the element
 * is v, scale3 and bias3 are ignored.  Otherwise
 *   f = fl32(fl32((float)v * scale3[c]) + bias3[c]),
 * two fp32 operations, each rounded, never fused: bit for bit what
 * x.float().mul(scale).add(bias) gives.  F32 stores f; F16 and BF16 store f
 * rounded to nearest-even; f32 and f16 subnormals are kept.
 * scale3, bias3: HOST pointers to three floats, read during the call and
 * passed as kernel arguments (capturable); NULL: 1.0 and 0.0.
 * d_flip: NULL, or nrects bytes on the device (any alignment, read inside
 * [0, nrects) only); a nonzero byte mirrors that crop horizontally: output
 * column j holds crop column w - 1 - j.
 * Placement: JPEGR_LAYOUT_CHW: plane c of a crop starts at dst + c w h, rows
 * of w elements; JPEGR_LAYOUT_HWC: pixel (i, j) is at dst + 3 (i w + j).
 * Equal-sized crops at dst = r * 3 w h form an [n, 3, h, w] or [n, h, w, 3]
 * tensor.
 * Good rectangles are delivered exactly, whatever the bad ones do.  No read
 * leaves d_in[0, in_len), d_tile_offsets[0, ntiles], d_rects[0, nrects) and
 * d_flip[0, nrects); no write leaves d_result, the scratch and each good
 * rectangle's own 3 w h elements within out_cap.  A rectangle bad on its own
 * fields or on the header writes nothing; one that fails inside a tile may
 * leave unspecified values in its own elements.  Overlapping destination
 * ranges hold unspecified values.
 * Asynchronous on `stream`, no host read-back, nothing kept on the host
 * (capturable and replayable).  JPEGR_ERR_ARG before any HIP call: everything
 * jpegr_crop_device rejects, with d_out 16-B aligned in place of 4-B (d_flip,
 * scale3 and bias3 may be NULL); a dtype or layout that is none of the values
 * below; a scale or bias that is not finite. */
#define JPEGR_DTYPE_U8   0
#define JPEGR_DTYPE_F32  1
#define JPEGR_DTYPE_F16  2
#define JPEGR_DTYPE_BF16 3
#define JPEGR_LAYOUT_CHW 0   /* [3][h][w] */
#define JPEGR_LAYOUT_HWC 1   /* [h][w][3] */

int jpegr_crop_tensor_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                             const void *d_tile_offsets, const void *d_rects, size_t nrects,
                             const void *d_flip, int max_w, int max_h,
                             int dtype, int layout, const float *scale3, const float *bias3,
                             void *d_out, size_t out_cap,
                             void *d_scratch, void *d_result, void *stream);

/* jpegr_crop_resize_device: rectangles of different sizes, each resampled to
 * out_w x out_h and delivered as jpegr_crop_tensor_device delivers (what
 * RandomResizedCrop, ToTensor, Normalize and a flip do), in five launches.
 * From jpegr_crop_tensor_device, unchanged: d_rects (jpegr_rect), the
 * untrusted d_tile_offsets, the K = jpegr_crop_items(max_w, max_h) mapping and
 * its 2^28 limit, d_flip, dtype, layout, the host scale3 / bias3 passed by
 * value, the three result words; asynchronous on `stream`, no read-back, no
 * host state, capturable and replayable, several calls in flight; every "no
 * read leaves / no write leaves" guarantee (the scratch here being
 * jpegr_crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h) bytes,
 * 16-B aligned), and JPEGR_ERR_ARG before any HIP call.
 * Differences.  Rectangle r's source is pixels [x, x + w) x [y, y + h) of its
 * image; each has its own w <= max_w and h <= max_h.  Its output is
 * 3 out_w out_h elements at d_out + dst (dst and out_cap count elements; d_out
 * 16-B aligned): CHW three planes of out_h rows of out_w; HWC pixel (i, j) at
 * dst + 3 (i out_w + j).  Rectangles at dst = r * 3 out_w out_h form
 * [n, 3, out_h, out_w] or [n, out_h, out_w, 3].  A rectangle is bad by
 * jpegr_crop_tensor_device's rules with the capacity rule
 * dst + 3 out_w out_h > out_cap, and also when w == 0 or h == 0 (nothing to
 * resample: no rectangle is "empty" in this call).  One that is bad on its own
 * fields or on the header writes nothing; one that fails inside a tile may
 * leave unspecified values in its own elements; good rectangles are exact
 * whatever the bad ones do.  JPEGR_ERR_ARG also for out_w or out_h <= 0,
 * 3 * out_w * out_h past INT_MAX, and a filter that is neither value below.
 * jpegr_crop_resize_scratch_bytes returns 0 on a bad argument (or a size past
 * SIZE_MAX) and is monotone in nrects.
 *
 * Values: the whole contract, bit for bit reproducible in numpy.  Per axis,
 * with n source pixels and m output pixels, in fp64, every operation rounded
 * and never fused:
 *   r  = (double)n / (double)m
 *   s  = (filter == TRIANGLE && r > 1.0) ? r : 1.0
 *   for output index j:
 *     c   = ((double)j + 0.5) * r
 *     lo  = max(0, (int64)floor((c - s) + 0.5));  hi = min(n, (int64)floor((c + s) + 0.5))
 *     u_x = max(0.0, 1.0 - fabs(((double)x + 0.5) - c) / s)     for x = lo .. hi - 1
 *     tot = ((0.0 + u_lo) + u_lo+1) + ...                       ascending x
 *     wt_x = (float)(u_x / tot)                 fp64 divide, then one rounding to fp32
 * hi > lo and tot >= 0.5 always: the pixel nearest to c is within 0.5 of it.
 * Then the pixels, per channel c (0 R, 1 G, 2 B) of the bytes v that
 * jpegr_crop_device delivers for the rectangle, in fp32, horizontal first:
 *   mid[y][j] = acc after: acc = 0.0f; for x = lo_j .. hi_j - 1 ascending:
 *                          acc = fl32(acc + fl32(wtx_x * (float)v[y][x]))
 *   val[i][j] = acc after: acc = 0.0f; for y = lo_i .. hi_i - 1 ascending:
 *                          acc = fl32(acc + fl32(wty_y * mid[y][j]))
 * A zero-weight tap changes nothing (acc + 0 = acc), so skipping it is within
 * the contract.  fp32 subnormals are kept, in weights and products alike.
 * The element: JPEGR_DTYPE_U8: val rounded to nearest-even and clamped to
 * 0 .. 255, scale3 and bias3 ignored.  Otherwise
 *   f = fl32(fl32(val * scale3[c]) + bias3[c]),
 * stored as F32, or rounded to nearest-even to F16 / BF16 exactly as
 * jpegr_crop_tensor_device does; val is not rounded to a byte first.
 * A nonzero d_flip[r] mirrors the OUTPUT: output column j holds resampled
 * column out_w - 1 - j.
 * Two consequences.  With w == out_w and h == out_h every wt is exactly 1.0 or
 * 0.0, and with either filter the elements equal jpegr_crop_tensor_device's bit
 * for bit.  And the definition is the half-pixel-centre bilinear of
 * interpolate(mode="bilinear", align_corners=False, antialias=<filter>), from
 * which it differs by roundings only (tests/test_jpr_resize_model.py). */
#define JPEGR_FILTER_BILINEAR 0   /* triangle filter, support 1: 2 taps an axis */
#define JPEGR_FILTER_TRIANGLE 1   /* antialiased: support max(1, n / m) */

size_t jpegr_crop_resize_scratch_bytes(size_t nrects, int max_w, int max_h,
                                       int out_w, int out_h);
int jpegr_crop_resize_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                             const void *d_tile_offsets, const void *d_rects, size_t nrects,
                             const void *d_flip, int max_w, int max_h,
                             int out_w, int out_h, int filter,
                             int dtype, int layout, const float *scale3, const float *bias3,
                             void *d_out, size_t out_cap,
                             void *d_scratch, void *d_result, void *stream);

/* A dataset: many streams, each with its own w x h, format and image count,
 * read by one call.  jpegr_dataset_crop_tensor_device and
 * jpegr_dataset_crop_resize_device are jpegr_crop_tensor_device and
 * jpegr_crop_resize_device with d_in, in_len, w, h, nimg and d_tile_offsets
 * replaced by d_streams and nstreams: a DEVICE array of nstreams
 * jpegr_stream_desc (8-B aligned; caller memory, read by the call's kernels
 * and never by the host; nothing is kept on the host).  A descriptor:
 *   d_in, in_len     the stream on the device, any alignment
 *   d_tile_offsets   jpegr_stream_index_device's ntiles + 1 u64 for that stream
 *                    (8-B aligned, untrusted as in the single-stream calls)
 *   image0           the dataset-wide index of the stream's image 0
 *   w, h, nimg       the stream's dimensions; reserved is ignored
 * jpegr_rect is unchanged; its `image` is a dataset-wide index g.  Rectangle r
 * belongs to the stream s with image0[s] <= g < image0[s] + nimg[s] and is
 * image g - image0[s] of it.  Callers build the table ascending in image0 and
 * gap-free (image0[s + 1] = image0[s] + nimg[s]).  The call's first launch
 * finds s by bisection over image0, a lane a rectangle, and then tests the
 * containment: an index no stream contains is a bad rectangle, and with a table
 * that is not ascending a rectangle is either delivered from a stream that does
 * contain its index or bad.
 * Values: a good rectangle's elements are bit for bit what
 * jpegr_crop_tensor_device (jpegr_crop_resize_device) writes for the same
 * rectangle, with image = g - image0[s], on stream s alone; dst, d_flip, dtype,
 * layout, scale3, bias3, filter, out_w and out_h mean what they mean there, and
 * the value sections above are the contract.
 * Good, bad, empty: the single-stream calls' rules, each judged against the
 * rectangle's OWN stream: x + w, y + h and the image index against that
 * descriptor's w, h and nimg, and the stream's 16 header bytes must be a JPR1 or
 * JPT1 header for the descriptor's w, h, nimg.  max_w and max_h bound every
 * rectangle; they are not compared with any stream's size (the host never reads
 * the table), so a max_w wider than some stream is no error.  A descriptor makes
 * every rectangle of its stream bad, and only those, when w, h or nimg is 0;
 * the stream has more than 2^32 tiles; in_len < 16; d_in or d_tile_offsets is
 * NULL or d_tile_offsets is not 8-B aligned; or the header is wrong.  A tile
 * with bad offsets, a rejected record or a rejected entropy stream turns bad
 * only the rectangles that touch it.  Good rectangles are exact whatever bad
 * rectangles, bad descriptors and other streams do.  The tensor call keeps
 * "w == 0 or h == 0 is good and writes nothing" for a rectangle whose stream is
 * found and sound; in the resize call such a rectangle is bad.
 * d_result: the three words of the single-stream calls; [0] and [2] count over
 * all streams, [1] is ~0 or 1 + the index of the first bad rectangle.
 * The scratch: jpegr_dataset_crop_scratch_bytes(nrects, max_w, max_h) or
 * jpegr_dataset_crop_resize_scratch_bytes(nrects, max_w, max_h, out_w, out_h)
 * bytes, 16-B aligned: the single-stream call's scratch and one u64 per
 * rectangle (stream << 32 | image in the stream) that the first launch hands to
 * the decode.  Both return 0 on a bad argument or a size past SIZE_MAX, are
 * monotone in nrects and never below their single-stream counterparts.
 * Whatever the table, the streams, the offsets and the rectangles say, no read
 * leaves d_streams[0, nstreams), each descriptor's d_in[0, in_len) and
 * d_tile_offsets[0, ntiles] (ntiles from the descriptor's w, h, nimg),
 * d_rects[0, nrects) and d_flip[0, nrects): the pointers in a descriptor are
 * trusted to cover those ranges, nothing else in it is trusted.  Writes are
 * limited as in the single-stream calls.
 * Asynchronous on `stream`, no host read-back, no host state: capturable and
 * replayable, several calls in flight, each with its own scratch and result.
 * The launches are the single-stream calls' (three and five), with the first
 * two replaced by their dataset forms.  JPEGR_ERR_ARG before any HIP call:
 * everything the single-stream call rejects that does not need a stream's
 * dimensions (a NULL d_rects, d_out, d_scratch or d_result; nrects, max_w or
 * max_h of 0; the alignments; nrects * K > 2^28; dtype, layout, filter, out_w,
 * out_h, scale3, bias3), and nstreams == 0 or > 2^31, and a NULL or misaligned
 * d_streams. */
typedef struct jpegr_stream_desc {
  const void *d_in;            /* the stream, device */
  uint64_t    in_len;
  const void *d_tile_offsets;  /* jpegr_stream_index_device's, ntiles + 1 u64 */
  uint64_t    image0;          /* dataset-wide index of this stream's image 0 */
  uint32_t    w, h, nimg, reserved;
} jpegr_stream_desc;           /* 48 B */

size_t jpegr_dataset_crop_scratch_bytes(size_t nrects, int max_w, int max_h);
size_t jpegr_dataset_crop_resize_scratch_bytes(size_t nrects, int max_w, int max_h,
                                               int out_w, int out_h);
int jpegr_dataset_crop_tensor_device(const void *d_streams, size_t nstreams,
                                     const void *d_rects, size_t nrects,
                                     const void *d_flip, int max_w, int max_h,
                                     int dtype, int layout, const float *scale3, const float *bias3,
                                     void *d_out, size_t out_cap,
                                     void *d_scratch, void *d_result, void *stream);
int jpegr_dataset_crop_resize_device(const void *d_streams, size_t nstreams,
                                     const void *d_rects, size_t nrects,
                                     const void *d_flip, int max_w, int max_h,
                                     int out_w, int out_h, int filter,
                                     int dtype, int layout, const float *scale3, const float *bias3,
                                     void *d_out, size_t out_cap,
                                     void *d_scratch, void *d_result, void *stream);

/* Thumbnails: images [image0, image0 + nimage) of a JPR1 or JPT1 stream at 1/8
 * scale, one RGBA8 pixel per tile, from the tiles' DC terms alone.  With
 * gw = ceil(w / 8) and gh = ceil(h / 8), pixel (tx, ty) of an image's
 * gw x gh thumbnail is pixel (8 tx, 8 ty) of what jpegr_reconstruct_device
 * (d_rgba_orig = NULL) gives for that image's coefficients with every AC term
 * set to 0 (alpha 255).  Such a tile reconstructs to one colour, so any of its
 * pixels would do; an edge tile's DC carries the encoder's zero padding, and
 * that is not corrected.  Tiles are in raster order and images in sequence:
 * the output is nimage * gw * gh consecutive pixels, pixel k that of tile
 * image0 * gw * gh + k of the stream.
 * d_rgba_out (16-B aligned, or NULL): those pixels.  d_dc_out (8-B aligned,
 * or NULL): per tile four int16 {Y, Cr, Cb, 0}, the three DC terms before any
 * arithmetic -- zz[0] of each stream: the value of its first (count, value)
 * RLE pair whose count is >= 1, else 0.  At least one of the two is given.
 * The walk of a stream stops as soon as it has the DC and does not validate
 * the rest of it:
 *   - if jpegr_stream_decode_device accepts all three streams of a tile, the
 *     tile's pixel and DC terms are exact;
 *   - a tile whose record fails the record rules, and every tile when the
 *     header or index is wrong, gets the colour of all-zero coefficients and
 *     DC terms of 0, as decode + reconstruct gives;
 *   - a stream that the full decoder rejects past its DC may still yield a DC
 *     here: that tile's pixel and DC terms are unspecified.
 * d_tile_offsets NULL: the call scans the index itself (d_scratch:
 * jpegr_thumb_scratch_bytes(tiles of the whole stream) =
 * jpegr_pack_scratch_bytes, 16-B aligned, required).  d_tile_offsets given
 * (jpegr_stream_index_device's ntiles + 1 u64, 8-B aligned): no sizes or scan
 * launch, d_scratch may be NULL.  The offsets are caller memory and not
 * trusted: a tile whose offsets are not off[t] <= off[t + 1] <= in_len with a
 * size of 12 .. 1,036 B is malformed, and the record rules apply inside that
 * size.
 * d_result: three u64 (8-B aligned), initialised by the call's own first
 * launch -- no memset, no tag, no spin:
 *   [0] the length the header and index imply, or off[ntiles] with offsets
 *   [1] ~0 when consistent; 0 on a wrong header, dimensions or implied length;
 *       else 1 + t for the first malformed tile t of the range (t counts from
 *       the stream's first tile)
 *   [2] the streams rejected inside the prefix examined (no codes, no RLE ints
 *       or more than the plane holds, a code length of 0 or past 32, no code
 *       at the bit position or only one that runs past nbits): a diagnostic,
 *       at most jpegr_stream_decode_device's count; this call's, never
 *       accumulated.  Such a stream's DC is 0.
 * Asynchronous on `stream`, no host read-back, nothing kept on the host
 * (capturable); several calls may be in flight at once, each with its own
 * scratch and result.  JPEGR_ERR_ARG before any HIP call: NULL d_in or
 * d_result, or both outputs NULL; bad dimensions or more than 2^32 tiles;
 * nimage == 0 or image0 + nimage > nimg; in_len < 16; d_rgba_out or d_scratch
 * not 16-B aligned, d_dc_out, d_tile_offsets or d_result not 8-B aligned; NULL
 * d_scratch together with NULL d_tile_offsets.
 * Whatever the stream and the offsets say, no read leaves d_in[0, in_len) and
 * d_tile_offsets[0, ntiles], and no write leaves the two outputs' nimage *
 * gw * gh * 4 and * 8 bytes, the scratch and the result words; table entries
 * and bit bytes are read inside the checked record only. */
size_t jpegr_thumb_scratch_bytes(size_t ntiles);
int jpegr_thumb_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                       const void *d_tile_offsets, size_t image0, size_t nimage,
                       void *d_rgba_out, void *d_dc_out, void *d_scratch, void *d_result,
                       void *stream);

/* Editing a stream without decoding it: a new JPR1 or JPT1 stream made of
 * tiles of an existing one.  A tile record is self-contained and a record's
 * place is the scan of the index, so a subset of a stream is a gather of
 * records behind a new index and header, and the other format is the same
 * records with each stream's table written the other way; no Huffman walk, no
 * IDCT, and the result is exact by construction.
 *
 * jpegr_select_device: the output is one well-formed stream of nitems images
 * of out_w x out_h.  Image k of it is the tile grid ceil(out_w / 8) x
 * ceil(out_h / 8) of source image items[k].image that starts at tile column
 * x / 8 and tile row y / 8, in raster order; whole images are x = y = 0,
 * out_w = w, out_h = h.  Items may repeat and come in any order.  The tiles
 * are the source's as they are: a window whose out_w is not a multiple of 8
 * and that ends inside the image keeps its last tile column whole, where an
 * encode of the cropped pixels would have padded it with zeros (and so for
 * out_h).  The header is the format's magic, out_w, out_h, nitems.
 * The target format is `format`, or the source's when format is 0 (JPR1 when
 * the source has no valid header).
 *   target == the source's   records are copied verbatim, non-canonical JPT1
 *                            modes included; only their offsets and size are
 *                            checked
 *   JPR1 -> JPT1             every stream's table in the writers' canonical mode:
 *                            the bytes jpegr_pack_tight_device writes
 *   JPT1 -> JPR1             modes 1 and 2 expanded to 3-B entries
 * In both re-codings the bit bytes and the rle_len, ncodes and nbits fields are
 * copied and the record rules are applied to the source record.
 * An item is bad when image >= nimg; x or y is not a multiple of 8;
 * x + out_w > w or y + out_h > h (no sum wraps); or the source's 16 header
 * bytes are not a JPR1 or JPT1 header for w, h, nimg (every item is bad then).
 * Every tile of a bad item is written as the empty record: 12 zero bytes, three
 * streams with ncodes = 0, which every reader turns into zero coefficients.  A
 * tile of a good item becomes the empty record too when its offsets are not
 * off[t] <= off[t + 1] <= in_len with a size of 12 .. 1,036 B (the offsets are
 * caller memory and not trusted, as for jpegr_crop_device) or, when re-coding,
 * the record rules reject the record.  Every other tile is exact, whatever the
 * bad ones do.
 * d_result: three u64 (8-B aligned), initialised by the call's own first launch
 * -- no memset, no tag, no spin:
 *   [0] the length, or the capacity needed
 *   [1] ~0, or 1 + the index of the first bad item
 *   [2] the tiles of good items written as the empty record: this call's count,
 *       never accumulated
 * The rest is jpegr_pack_device's contract: a u64 at d_out_len (8-B aligned)
 * holds the length, or the exact capacity needed when that exceeds cap, in
 * which case d_out[0, cap) holds the stream's first cap bytes and nothing at or
 * past cap is written.  d_out 16-B aligned; d_in any alignment; d_items,
 * d_tile_offsets (jpegr_stream_index_device's ntiles + 1 u64) and d_result
 * 8-B aligned; d_scratch 16-B aligned, jpegr_select_scratch_bytes(nitems,
 * out_w, out_h) bytes (0 on a bad argument).  Asynchronous on `stream`, no host
 * read-back, nothing kept on the host (capturable, replayable); several calls
 * may be in flight at once, each with its own scratch and result.  No read
 * leaves d_in[0, in_len), d_tile_offsets[0, ntiles] and d_items[0, nitems),
 * whatever they say and wherever d_in lies: a record is read as the aligned
 * dwords that lie wholly inside it and its other bytes one by one.
 * JPEGR_ERR_ARG before any HIP call: a NULL pointer; bad source dimensions or
 * more than 2^32 source tiles; nitems == 0 or past 2^31 - 1 (the header's
 * count); out_w or out_h <= 0, out_w > w, out_h > h; more than 2^32 output
 * tiles; a format other than 0, JPEGR_STREAM_JPR1 and JPEGR_STREAM_JPT1;
 * in_len < 16; a misalignment listed above.
 *
 * Joining streams of one w, h and format needs no call: a new header with the
 * sum of the image counts, the indexes back to back, then the records back to
 * back (INTEGRATION.md has the copies). */
typedef struct jpegr_sel { uint64_t image, x, y; } jpegr_sel;

size_t jpegr_select_scratch_bytes(size_t nitems, int out_w, int out_h);
int jpegr_select_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                        const void *d_tile_offsets, const void *d_items, size_t nitems,
                        int out_w, int out_h, int format, void *d_out, size_t cap,
                        void *d_out_len, void *d_scratch, void *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* JPEGR_H */
