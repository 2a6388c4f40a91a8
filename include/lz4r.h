/*
 * lz4r.h -- C ABI of the MI355X "LZ4" compressor: the reference's exhaustive
 * per-300-byte-block longest-match finder, greedy parser and custom
 * token/sequence byte emitter, bit-exact to Algorithms/sequential/LZ4/LZ4.c
 * (canonical semantics: matches are clamped at the block end).
 *
 * Entry points and the reference interface each replaces
 * (Algorithms/sequential/LZ4/LZ4.c):
 *   lz4r_compress_device / lz4r_compress   <- lz4_encode()            :670-742
 *        (divide_input :123-177, the block loop :707-721, write_output
 *         :427-441 minus the fixed file paths; the bytes written equal
 *         compressed.bin)
 *   per block inside the kernels            <- block_encode()          :506-620
 *                                              find_longest_match()    :290-323
 *                                              add_sequence_to_block() :443-459
 *                                              write_sequence/_block() :365-425
 *   lz4r_compress_segment_device            <- the same, for a run of whole
 *        blocks without the frame header byte (multi-GPU shards)
 *
 * Stream format (frame := u8 nblocks&0xFF, block*; block := u8 nseq&0xFF,
 * u16le (sum of sequence sizes + 3), sequence*).
 *
 * Errors: negative LZ4R_ERR_* codes instead of the reference's
 * perror()+exit(1).  An input shorter than one block (300 B) is
 * LZ4R_ERR_TOO_SMALL, the reference's exit(1) at LZ4.c:632-637.
 *
 * No torch types: device pointers are plain `void *`, `stream` is a
 * hipStream_t passed as `void *` (NULL = legacy default stream).  A context
 * owns the scratch buffers; one context per thread (or serialise).
 */
#ifndef LZ4R_H
#define LZ4R_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZ4R_BLOCK 300            /* DEFAULT_BLOCK_LENGTH, LZ4.c:23 */
#define LZ4R_BLOCK_BOUND 1152     /* max encoded bytes of one block */

#define LZ4R_OK 0
#define LZ4R_ERR_ARG (-1)         /* NULL pointer / bad argument */
#define LZ4R_ERR_TOO_SMALL (-2)   /* input < LZ4R_BLOCK (LZ4.c:632) */
#define LZ4R_ERR_CAPACITY (-3)    /* output buffer too small; *out_len = need */
#define LZ4R_ERR_HIP (-4)         /* HIP runtime error */
#define LZ4R_ERR_NOMEM (-5)       /* device allocation failed */
#define LZ4R_ERR_CORRUPT (-6)     /* decoder: malformed stream; compressor: corrupt LDS index */
/* bit 63 of an async call's length word: the call met a corrupt LDS index */
#define LZ4R_LEN_CORRUPT (1ull << 63)

/* Inputs up to 2^40 bytes per call; the kernels run in chunks of 2^24 blocks
 * (5.03 GB), so device scratch is ~10.7 GB of block slots at most plus
 * 16 B per block of the whole input. */

typedef struct lz4r_ctx lz4r_ctx;

/* Create a context bound to the current HIP device. */
int lz4r_ctx_create(lz4r_ctx **ctx);
void lz4r_ctx_destroy(lz4r_ctx *ctx);

/* Worst-case compressed size of n input bytes (frame header included). */
size_t lz4r_compress_bound(size_t n);
size_t lz4r_nblocks(size_t n);

/* Blocks per launch chunk of this build of the library: 2^24 in the product
 * (a longer call is cut into that many blocks per pass of the kernels, see
 * above); a test build compiled with -DLZ4R_CHUNK_LOG2=k reports 2^k, so a
 * test can tell that its input really crosses chunks.  Read-only. */
size_t lz4r_launch_chunk_blocks(void);

/* Compress n bytes at d_in (device) into d_out (device, cap bytes) on
 * `stream`, then synchronise it and return the compressed length in
 * *out_len.  Frame header included.  Bytes equal lz4_encode()'s
 * compressed.bin for the same input. */
int lz4r_compress_device(lz4r_ctx *ctx, const void *d_in, size_t n,
                         void *d_out, size_t cap, size_t *out_len,
                         void *stream);

/* Asynchronous form: enqueue only.  The compressed length (or the required
 * capacity, if larger than cap: nothing past cap is written) is stored as a
 * uint64 at d_out_len (device) when the stream reaches it.  Bit 63 of that
 * word (LZ4R_LEN_CORRUPT) is set, instead of an error return, when the call
 * met a corrupt bucket head in lz4_tiles' LDS index (see lz4r_check): the
 * caller gets the verdict in the same read-back as the length and must not
 * use the stream then.  The length is the word without that bit. */
int lz4r_compress_async(lz4r_ctx *ctx, const void *d_in, size_t n,
                        void *d_out, size_t cap, void *d_out_len,
                        void *stream);

/* A run of whole 300-byte blocks without the frame header byte, for shards
 * of a multi-GPU job; asynchronous, length at d_out_len like
 * lz4r_compress_async.  Only the globally last shard (final_shard != 0) may
 * end in a short block: a non-final shard whose n is not a multiple of 300
 * is rejected with LZ4R_ERR_ARG (its stream would differ from the single-GPU
 * one).  n == 0 (more ranks than blocks) enqueues a zero length.
 * Concatenating the segments of consecutive shards after one header byte
 * (u8 total_blocks & 0xFF) yields the single-GPU stream. */
int lz4r_compress_segment_async(lz4r_ctx *ctx, const void *d_in, size_t n,
                                void *d_out, size_t cap, void *d_out_len,
                                int final_shard, void *stream);

/* find_longest_match (LZ4.c:290-323) at every position of every 300-byte
 * block of the n bytes at d_in, in one launch, asynchronous on `stream`:
 * d_matches[300 b + p] (uint32, n entries, device) = len | dist << 16 for
 * the longest match at p of block b (the earliest source among equals,
 * LZ4.c:307; matches clamped at the block end), or 0 when len < 4
 * (MIN_MATCH_LENGTH).  len is not truncated: the reference's uint8_t return
 * value is len & 0xFF. */
int lz4r_block_matches_device(const void *d_in, size_t n, void *d_matches, void *stream);

/* find_longest_match (LZ4.c:290-323) at every position of ONE block of any
 * length n (what block_encode does for a block_length other than 300): the
 * reference's whole window (sources i >= p - WINDOW_SIZE, LZ4.c:295), match
 * length capped at MAX_MATCH_LENGTH (1024, LZ4.c:20) and at the block end.
 * d_matches[p] = len | dist << 16, or 0 when len < 4.  O(n * min(n, 65535))
 * work: a compatibility path.  Asynchronous on `stream`; n < 2^32. */
int lz4r_window_matches_device(const void *d_in, size_t n, void *d_matches, void *stream);

/* After a compress call: copy the encoded byte count (uint16) of each of the
 * first `count` blocks of the last call to `dst` (host or device memory),
 * then synchronise `stream`.  Block b's bytes start at sum(sizes[0..b)) after
 * the frame header byte.  Written by the kernel on every call (2 B/block). */
int lz4r_copy_block_sizes(const lz4r_ctx *ctx, void *dst, size_t count,
                          void *stream);

/* After a compress call: copy the first `count` per-block output offsets
 * (uint64, exclusive scan, relative to the first block byte -- add 1 for a
 * framed stream) of the last call to `dst` (host or device memory), then
 * synchronise `stream`.  The placement kernel writes them on the device as
 * it computes them (8 B/block); no host prefix sum. */
int lz4r_copy_block_offsets(const lz4r_ctx *ctx, void *dst, size_t count,
                            void *stream);

/* The same offsets in place: *d_offsets = the context's device array of the
 * last call's *count block offsets (valid until the next call on ctx; ready
 * when the call's stream reaches its end).  This is what the block-parallel
 * decoder takes, without a host round trip. */
int lz4r_block_offsets_device(const lz4r_ctx *ctx, const void **d_offsets,
                              size_t *count);

/* Decode a framed stream (bytes as lz4r_compress writes them) back to the
 * input.  Host C; replaces LZ4_decode / interpret_frame (LZ4.c:937-1121),
 * which mis-parse streams of >= 256 blocks or literal runs >= 271: blocks are
 * read until the input ends (the frame byte is checked modulo 256), literal
 * lengths come from the exact u16 size field, and the format's one
 * ambiguous token (a match of 257..259 stored as M = 1..3, LZ4.c:317) is
 * resolved per block by backtracking.  LZ4R_ERR_CAPACITY sets *out_len to
 * the length needed so far; LZ4R_ERR_CORRUPT on a malformed stream. */
int lz4r_decompress(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap,
                    size_t *out_len);

/* Block-parallel GPU decoder (csrc/lz4r_gpudec.hip), asynchronous on
 * `stream`.  d_in: the framed stream (in_len bytes, device); d_block_offsets:
 * nb uint64 offsets of each block's first byte relative to the first block
 * byte, as lz4r_copy_block_offsets returns them for the compressing call
 * (the format cannot be split without them).  Block b decodes to
 * d_out[300 b ...]; nothing at or past out_cap is written.  d_result: two
 * uint64 on the device: [0] = decoded length (if it exceeds out_cap, only
 * out_cap bytes were written), [1] = ~0 if every block was consistent, else
 * 1 + the index of the first malformed block. */
int lz4r_decompress_device(const void *d_in, size_t in_len, const void *d_block_offsets,
                           size_t nb, void *d_out, size_t out_cap, void *d_result,
                           void *stream);

/* Decode a bare framed stream on the GPU -- only the stream, as LZ4_decode
 * (LZ4.c:1038) takes the file: the block boundaries are found on the device
 * (csrc/lz4r_gpudec.hip: a candidate header per 8 KiB chunk, a lane per
 * chunk walking the size fields, one wave re-walking any chunk whose
 * predecessor does not end on its candidate), then lz4_decode_blocks checks
 * every block against them.  Streams with truncated matches (whose size
 * fields over-count, LZ4.c:569-575) take a second pass that parses every
 * block.  d_in / d_out are device pointers; synchronises `stream`;
 * *out_len = decoded length.  LZ4R_ERR_CORRUPT when the blocks do not chain
 * from the frame byte to the end of the stream or a block does not decode;
 * LZ4R_ERR_CAPACITY (with *out_len = need, or a lower bound on it when the
 * stream has more blocks than out_cap can hold) when out_cap is too small.
 * One host read-back per pass when out_cap / 300 + 1 <= (in_len - 1) / 8 + 1
 * (the output bounds the block count); a larger out_cap reads the block
 * count back first.  Device scratch: ~20 B per 8 KiB of stream + 8 B per
 * block out_cap can hold (stream-ordered allocation from a per-device pool
 * the library keeps: returned to the pool on return, not to the device, so
 * the next call does not map it again). */
int lz4r_decompress_stream_device(const void *d_in, size_t in_len, void *d_out,
                                  size_t out_cap, size_t *out_len, void *stream);

/* Host-buffer form of lz4r_decompress_stream_device (copies in and out). */
int lz4r_decompress_stream(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap,
                           size_t *out_len);

/* Random access: many byte ranges of the decoded stream in one call, each
 * decoded from the 300-byte blocks it covers and from nothing else
 * (csrc/lz4r_read.hip).  Read r delivers decoded bytes [src, src + len) to
 * d_out[dst, dst + len).  d_reads: nreads of these on the device. */
typedef struct lz4r_read { uint64_t src, len, dst; } lz4r_read;

/* Blocks a read of max_len bytes can cover, K = (max_len + 298) / 300 + 1:
 * the items every read of a call with that max_len occupies.  Host only. */
size_t lz4r_read_items(size_t max_len);

/* d_in, in_len, d_block_offsets and nb are lz4r_decompress_device's: the
 * framed stream and the nb uint64 offsets relative to the first block byte
 * (lz4r_copy_block_offsets, lz4r_block_offsets_device or
 * lz4r_stream_index_device); block nb - 1 ends at in_len and may be short.
 * Asynchronous on `stream`; no host read-back and no host state between
 * calls, so a call can be captured into a graph.  d_result: two uint64 on
 * the device, reset by the call's own first launch: [0] = the summed len of
 * the reads that were delivered, [1] = ~0 when every read was delivered, else
 * 1 + the index of the first bad read.  A read is bad when len > max_len,
 * when src + len overflows or passes the decoded length (no length argument:
 * the lane that decodes block nb - 1 knows it), when dst + len > out_cap, or
 * when a block it covers is malformed (offsets not inside [0, in_len), fewer
 * than 3 or more than LZ4R_BLOCK_BOUND bytes, or bytes that do not parse).
 * len == 0 is a good read that writes nothing, whatever its src and dst.
 * Good reads are delivered exactly whatever the bad ones do; destination
 * ranges of different reads that overlap hold unspecified bytes.  Whatever
 * the stream, the offsets and the reads say, nothing outside d_in[0, in_len),
 * d_block_offsets[0, nb) and d_reads[0, nreads) is read and nothing outside
 * d_result and each read's own d_out[dst, dst + len) within out_cap is
 * written: a read that fails on its own fields (len, overflow, capacity, a
 * block index >= nb) writes nothing, one that fails inside a block may leave
 * unspecified bytes in its own destination range.
 * Mapping: every read occupies K = lz4r_read_items(max_len) lanes, one per
 * block it may cover, so group reads of similar size per call: a batch of
 * short reads with one long one is correct but idles most lanes.
 * LZ4R_ERR_ARG, before any HIP call: a NULL pointer; nb, nreads or max_len 0;
 * in_len < 4; d_reads, d_block_offsets or d_result not 8-byte aligned;
 * nreads * K items needing more than 2^31 - 1 workgroups of 32.  d_in and
 * d_out take any alignment. */
int lz4r_read_device(const void *d_in, size_t in_len, const void *d_block_offsets,
                     size_t nb, const void *d_reads, size_t nreads, size_t max_len,
                     void *d_out, size_t out_cap, void *d_result, void *stream);

/* The block offsets of a bare framed stream, kept: the boundary search of
 * lz4r_decompress_stream_device into the caller's d_block_offsets (cap_blocks
 * uint64, device), every block then checked by the decoder writing no
 * output.  Synchronises `stream`.  LZ4R_OK: *nb blocks, *decoded_len decoded
 * bytes, and d_block_offsets[0, *nb) equal what lz4r_copy_block_offsets gave
 * the compressing call -- what lz4r_read_device and lz4r_decompress_device
 * take.  LZ4R_ERR_CAPACITY with *nb = the blocks needed when cap_blocks is
 * too small (a stream of in_len bytes has at most (in_len - 1) / 8 + 1);
 * LZ4R_ERR_CORRUPT as lz4r_decompress_stream_device.  A fast pass, then the
 * exact pass for streams with truncated matches; one host read-back each. */
int lz4r_stream_index_device(const void *d_in, size_t in_len, void *d_block_offsets,
                             size_t cap_blocks, size_t *nb, size_t *decoded_len, void *stream);

/* Host convenience wrapper around lz4r_compress_device (copies in and out). */
int lz4r_compress(const uint8_t *in, size_t n, uint8_t *out, size_t cap,
                  size_t *out_len);

/* ---- standard LZ4 frames -------------------------------------------------
 * The same parse (the reference's greedy longest-match parse of every 300-byte
 * block) written as a standard LZ4 frame, which `lz4 -d`, liblz4 and every
 * other LZ4 frame reader decode: LZ4 Frame Format 1.6.x, magic 04 22 4D 18,
 * FLG 0x68 (version 01, independent blocks, content size present, no
 * checksums, no dictionary ID), BD 0x40 (64 KiB block maximum), u64 content
 * size = n, header checksum; then one data block per 64 source blocks (19,200
 * input bytes; the last one what is left), each a u32 size and that many
 * bytes, always stored compressed (the high bit is never set, so the bytes are
 * deterministic), then the EndMark 00 00 00 00.  A data block's sequences are
 * its source blocks' matches under the block format's end rules: a match of
 * fewer than 4 stored bytes or one that starts in the data block's last 11
 * bytes becomes literals, one that reaches into its last 5 bytes is cut, and
 * literal runs merge across source blocks (csrc/lz4r_frame.h).
 *
 * Worst-case frame size of n input bytes: 19 + n + 100 per data block (header
 * 15, EndMark 4; per data block of N <= 19,200 bytes the u32 size, N / 255
 * literal-length bytes, the last token and one more extension byte: <= 81). */
size_t lz4r_frame_bound(size_t n);

/* lz4r_compress_async's and lz4r_compress_device's contracts, for a standard
 * frame: the length word holds the need when it exceeds cap (nothing at or
 * past cap is written), bit 63 is the corrupt-index verdict, n < 300 is
 * LZ4R_ERR_TOO_SMALL, d_in and d_out take any alignment, the async form
 * enqueues only (no host read-back: it can be captured into a graph).
 * A frame call leaves no per-block arrays: after it lz4r_copy_block_sizes,
 * lz4r_copy_block_offsets and lz4r_block_offsets_device, which describe native
 * streams, return LZ4R_ERR_ARG (not a stale array) until the next native call
 * on the context. */
int lz4r_compress_frame_async(lz4r_ctx *ctx, const void *d_in, size_t n,
                              void *d_out, size_t cap, void *d_out_len,
                              void *stream);
int lz4r_compress_frame_device(lz4r_ctx *ctx, const void *d_in, size_t n,
                               void *d_out, size_t cap, size_t *out_len,
                               void *stream);

/* Host-buffer form of lz4r_compress_frame_device (copies in and out). */
int lz4r_compress_frame(const uint8_t *in, size_t n, uint8_t *out, size_t cap,
                        size_t *out_len);

/* Decode standard LZ4 frames on the host (host/lz4f_decode.c): exact and
 * bounds-checked, for any conforming frame, not only this library's --
 * linked or independent blocks, stored blocks, content size present or
 * absent; the header checksum is verified, block and content checksums when
 * their flags are set.  Concatenated frames decode to the concatenation (one
 * frame per GPU shard is a valid file).  LZ4R_ERR_CORRUPT on anything
 * malformed or unsupported: an empty or truncated input, a dictionary ID, a
 * reserved bit, a skippable or legacy magic, a wrong checksum, a content size
 * that does not match.  LZ4R_ERR_CAPACITY sets *out_len to the length needed
 * so far.  Never reads outside in[0, in_len) or writes outside out[0, cap). */
int lz4r_frame_decompress(const uint8_t *in, size_t in_len, uint8_t *out,
                          size_t cap, size_t *out_len);

/* flags of lz4r_frame_decompress_device / lz4r_frame_decompress_gpu */
#define LZ4R_FRAME_NO_CONTENT_CHECKSUM 1u   /* do not verify a frame's content checksum */

/* Decode standard LZ4 frames on the GPU (csrc/lz4f_gpudec.hip), enqueued on
 * `stream`, which the call synchronises.  d_in (in_len bytes) and d_out
 * (out_cap bytes) are device pointers of any alignment.
 * Accepts every frame lz4r_frame_decompress accepts -- independent and linked
 * blocks, stored blocks, content size present or absent, block maxima from
 * 64 KiB to 4 MiB, concatenated frames -- and verifies what it verifies: the
 * header checksum, block checksums when flagged, the content size when
 * present, and the content checksum when flagged unless flags has
 * LZ4R_FRAME_NO_CONTENT_CHECKSUM (as liblz4's skipChecksums).  Everything
 * the host decoder calls corrupt is LZ4R_ERR_CORRUPT here (skippable and
 * legacy magics, dictionary IDs and reserved bits among it; in_len 0 too): for
 * every input the return code equals lz4r_frame_decompress's, and on LZ4R_OK
 * so do the bytes and *out_len.
 * Independent and stored blocks decode in parallel, a wave each; a linked
 * frame is one serial chain (frames still run side by side); a content
 * checksum is serial over its frame's decoded bytes (xxh32 has no combine
 * step), one wave per frame.
 * LZ4R_ERR_CAPACITY when the frames decode to more than out_cap bytes: then
 * *out_len is the exact decoded length of all frames, known from the blocks'
 * tokens before anything is decoded, and nothing is written.  A frame that is
 * malformed in its headers, size words, block checksums, token streams or
 * content sizes is LZ4R_ERR_CORRUPT whatever out_cap is; a match distance
 * beyond its window or a wrong content checksum is found only by decoding,
 * which needs the room: with too small an out_cap such a frame is
 * LZ4R_ERR_CAPACITY (nothing is written), and LZ4R_ERR_CORRUPT once the
 * capacity it names is given.
 * Whatever the bytes say, nothing outside d_in[0, in_len) is read and
 * nothing outside d_out[0, out_cap) and the call's own scratch is written; a
 * block that fails may leave unspecified bytes in its own output range only.
 * LZ4R_ERR_ARG, before any HIP call, for a NULL d_in or out_len, or a NULL
 * d_out with out_cap > 0.
 * Scratch: a stream-ordered allocation from the per-device pool the
 * bare-stream decoder keeps: 28 bytes per data block and 40 per frame, with
 * room for in_len / 1024 + 4096 blocks and in_len / 65536 + 64 frames (about
 * in_len / 36 + 120 KB: 30 MB for a 1 GiB input); an input with more blocks
 * or frames than that is walked a second time into an index of exactly their
 * number.
 * Host read-backs: two per call, for every input -- the walk's block and frame
 * counts, then the total length with the verdict.  Whether the output fits is
 * decided on the device between them. */
int lz4r_frame_decompress_device(const void *d_in, size_t in_len, void *d_out,
                                 size_t out_cap, size_t *out_len,
                                 unsigned flags, void *stream);

/* Host-buffer form of lz4r_frame_decompress_device (copies in and out). */
int lz4r_frame_decompress_gpu(const uint8_t *in, size_t in_len, uint8_t *out,
                              size_t cap, size_t *out_len, unsigned flags);

/* Synchronise `stream` and report whether the last compress call on ctx met
 * a corrupt bucket head in lz4_tiles' LDS index (a head that is neither empty
 * nor an earlier position of the block: never on a sound LDS; the walk ends
 * anyway, chains strictly decrease): LZ4R_ERR_CORRUPT or LZ4R_OK.  It reads a
 * verdict word the context owns, written by the call's last scan kernel
 * beside LZ4R_LEN_CORRUPT of the call's length word (so the caller's length
 * buffer may already be freed).  Every call folds the kernel's status into
 * its own length word and clears it, so an async caller that reads the
 * length needs no separate check.  lz4r_compress_device checks by itself.
 * Ordering: the verdict word is one per context and every call overwrites it,
 * whatever stream that call runs on.  Pass the stream the compress call ran
 * on, and call lz4r_check before the next compress call on this context;
 * otherwise the word read is unordered with, or belongs to, another call
 * (the length word's bit 63 has no such restriction). */
int lz4r_check(lz4r_ctx *ctx, void *stream);

/* Measurement: when enabled, every compress call records HIP events on its
 * own launch stream around the whole call and around each launch of the
 * compressor kernel lz4_tiles (one per 2^24-block chunk of the input).
 * lz4r_last_timing waits for the last call's end event and returns the
 * call's duration and the summed lz4_tiles durations in milliseconds.
 * Enabling starts a new record; each timed call has its own events (a ring
 * of the newest 4096 calls), so back-to-back async calls are timed without a
 * host wait between them: lz4r_timed_calls then waits for the newest call and
 * fills ms_call/ms_match with the newest min(calls, 4096, max) calls' times,
 * oldest first, and their number in *count. */
int lz4r_set_timing(lz4r_ctx *ctx, int enable);
int lz4r_last_timing(lz4r_ctx *ctx, float *ms_call, float *ms_match);
int lz4r_timed_calls(lz4r_ctx *ctx, size_t max, float *ms_call, float *ms_match, size_t *count);

const char *lz4r_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* LZ4R_H */
