// jpegr_select.hip -- a new stream from tiles of a JPR1 or JPT1 stream, with no
// entropy decode (include/jpegr.h: jpegr_select_device): output image k is a
// tile-aligned window of source image items[k].image, its records gathered
// from the source by the caller's offsets, behind a new header and index.  The
// target format is the source's (records copied verbatim) or the other one
// (each stream's table re-coded, its header fields and bit bytes copied).
//
//   jprs_select_sizes   target JPR1 or the source's: a lane per output tile.
//                       The tile's item and source record (locate), the output
//                       record's size -> u32 (the scan's input) and the u16
//                       index; the header; the result words' reset
//   jprs_select_sizes_tight   target JPT1: a JPR1 record's size in JPT1 depends
//                       on every table entry, so a workgroup stages 16 records
//                       in LDS and a wave takes a tile, entry k of a stream on
//                       lane k, the modes from ballots (jpt_pack_sizes' shape)
//   lz4_scan_reduce / lz4_scan_partials   the scan, over the output tiles
//   jprs_select_emit    jpr_pack_emit's structure: a workgroup of four waves
//                       per 16 output tiles, their records assembled in the
//                       LDS image of the output range, out through image_out.
//                       The 16 source records are found by 16 lanes at once and
//                       read in one round, each by aligned dwords inside the
//                       record (its edges bytewise), straight into the image
//                       (a copy) or into staging buffers, from which a wave's
//                       lanes re-code a tile at a time
// The source's format is on the device only (no read-back), so one launch
// serves the three cases: every wave reads the 16 header bytes and branches
// uniformly.  Both passes derive a tile's size from the same bytes by the same
// functions; the emit pass writes a record only when its size is the scan's.
// The format's rules are jpegr_pack_common.h's: record_at, record_rule, tile_modes,
// put_stream_headers and put_table_word (as jpr_pack_emit writes).
// No host-side state: the call can be captured in a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

#include "../../include/jpegr.h"
#include "jpegr_pack_common.h"

namespace {

constexpr int kStage = 1040;                // a record, in whole 16-B chunks
static_assert(kTW == 4, "a wave's four tiles are spelled out below");

struct Sel {
  const uint8_t *in;
  uint64_t in_len;
  const uint64_t *toff;                     // the caller's, ntiles + 1: not trusted
  const jpegr_sel *items;
  uint64_t per, opt, ntout;                 // source tiles an image, output tiles an item, output tiles
  uint32_t w, h, nimg, gw, ogw, out_w, out_h, nitems;
  int format;                               // the call's: 0 = the source's
};

// The source's format from its 16 header bytes, a byte per lane of a whole
// wave: JPEGR_STREAM_JPR1 or _JPT1 when it is a header for w, h, nimg, else 0.
__device__ __forceinline__ int source_format(const Sel &s, int lane) {
  const uint32_t word = lane < 4 ? kMagicJPR1 : lane < 8 ? s.w : lane < 12 ? s.h : s.nimg;
  const uint32_t b = lane < 16 ? (uint32_t)s.in[lane] : 0u;            // in_len >= 16
  const bool bad = lane < 16 && lane != 2 && b != ((word >> (8 * (lane & 3))) & 255u);
  const uint32_t b2 = (uint32_t)__shfl((int)b, 2);
  if (__ballot(bad) != 0) return 0;
  return b2 == 'R' ? JPEGR_STREAM_JPR1 : b2 == 'T' ? JPEGR_STREAM_JPT1 : 0;
}

// the output's format: the call's, else the source's, else (no source header) JPR1
__device__ __forceinline__ int target_format(const Sel &s, int src) {
  return s.format ? s.format : src ? src : JPEGR_STREAM_JPR1;
}

// Output tile u: its item k, and its source record [o0, o0 + size) of the
// stream.  0: found; 1: the item is bad; 2: the item is good and the tile's
// offsets are not a record's.
__device__ __forceinline__ int locate(const Sel &s, bool header, uint64_t u, uint64_t &k, uint64_t &o0,
                                      uint32_t &size) {
  k = u / s.opt;
  const uint64_t r = u - k * s.opt;
  const jpegr_sel it = s.items[k];
  // out_w <= w and out_h <= h (the host's check): neither difference wraps
  if (!header || it.image >= s.nimg || ((it.x | it.y) & 7u) != 0 || it.x > (uint64_t)(s.w - s.out_w) ||
      it.y > (uint64_t)(s.h - s.out_h))
    return 1;
  const uint64_t oy = r / s.ogw, ox = r - oy * s.ogw;
  // y / 8 + ceil(out_h / 8) <= ceil(h / 8), and so for x: t < ntiles
  const uint64_t t = it.image * s.per + ((it.y >> 3) + oy) * s.gw + (it.x >> 3) + ox;
  return record_at(s.toff, t, s.in_len, o0, size) ? 0 : 2;
}

__device__ __forceinline__ uint32_t record_bytes(const uint32_t (&m)[3], uint32_t mds) {
  return stream_bytes(m[0], 0, mds & 3u) + stream_bytes(m[1], 1, (mds >> 2) & 3u) +
         stream_bytes(m[2], 2, mds >> 4);
}

// A checked JPR1 record's table words on the wave, as jpr_pack_emit holds a
// tile's (tb[0], tb[1]: Y entries lane, 64 + lane; tb[2]: Cr; tb[3]: Cb; 0
// where not live), and from them the writers' canonical modes as
// Y | Cr << 2 | Cb << 4 (tile_modes).  A whole wave.
template <typename Rd>
__device__ __forceinline__ uint32_t plain_table(Rd rd, const uint32_t (&so)[3], const uint32_t (&m)[3],
                                                int lane, uint32_t (&tb)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = word_chan(q);
    const uint32_t k = word_entry(q, lane);
    const uint32_t x = so[c] + 4u + 3u * k;
    tb[q] = k < (m[c] >> 24) ? rd(x) | rd(x + 1) << 8 | rd(x + 2) << 16 : 0u;
  }
  return tile_modes(tb, m[0] >> 24, m[1] >> 24, m[2] >> 24);
}

// ---- sizes ----------------------------------------------------------------------

// Output tile u's size: the scan's input and the index entry; with tile 0 the
// header, and the result words that the emit pass adds to.
__device__ __forceinline__ void put_size(const Sel &s, int target, uint64_t u, uint32_t sz,
                                         uint32_t *__restrict__ tsz, uint8_t *__restrict__ out, uint64_t cap,
                                         uint64_t *__restrict__ result) {
  tsz[u] = sz;
  put_index(out, cap, u, sz);
  if (u == 0) {
    put_header(out, cap, target == JPEGR_STREAM_JPT1 ? kMagicJPT1 : kMagicJPR1, s.out_w, s.out_h, s.nitems);
    result[1] = ~0ull;
    result[2] = 0ull;
  }
}

__global__ __launch_bounds__(256) void jprs_select_sizes(const Sel s, size_t u_base,
                                                         uint32_t *__restrict__ tsz,
                                                         uint8_t *__restrict__ out, uint64_t cap,
                                                         uint64_t *__restrict__ result) {
  const int src = source_format(s, threadIdx.x & 63);
  const int target = target_format(s, src);
  const uint64_t u = u_base + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= s.ntout) return;
  uint64_t k, o0 = 0;
  uint32_t size = 0, sz = kEmptyRec;
  if (locate(s, src != 0, u, k, o0, size) == 0) {
    if (target == src) {
      sz = size;
    } else {                                              // JPT1 -> JPR1: the three headers say it
      const uint8_t *const rec = s.in + o0;
      auto rd = [&](uint32_t x) -> uint32_t { return rec[x]; };
      uint32_t so[3], m[3] = {0u, 0u, 0u}, md = 0u;
      if (record_rule<true>(rd, 0u, size, so, m, md)) sz = record_bytes(m, 0u);
    }
  }
  put_size(s, target, u, sz, tsz, out, cap, result);
}

// ---- a run's source records ------------------------------------------------------

// A workgroup's run of up to 16 output tiles, found by 16 lanes at once (one
// round of dependent loads for the run: item, offsets) and kept in LDS.
struct RunSrc {
  uint64_t o0[kRun], k[kRun];
  uint32_t size[kRun];
  int where[kRun];
};

// lanes first .. first + ntl - 1 of the workgroup find tiles t0 .. t0 + ntl - 1
__device__ __forceinline__ void locate_run(const Sel &s, bool header, uint64_t t0, int ntl, int tid, int first,
                                           RunSrc &r) {
  const int j = tid - first;
  if (j < 0 || j >= ntl) return;
  uint64_t k = 0, o0 = 0;
  uint32_t size = 0;
  r.where[j] = locate(s, header, t0 + j, k, o0, size);
  r.k[j] = k;
  r.o0[j] = o0;
  r.size[j] = size;
}

__device__ __forceinline__ void put4(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
}

// A wave's kTW records, size[i] bytes from src[i] (global, any alignment, all
// of them inside the stream; size 0: nothing) to dst[i] (LDS, any alignment):
// the aligned dwords that lie inside [src, src + size) as dwords, the up to
// three bytes before the first and after the last of them bytewise, so no load
// reaches outside the record.  A lane's first dword and edge byte of all kTW
// records are loaded before the first is written: one round of latency for
// records of up to 256 B and more, the rest of a longer one in a loop.
__device__ __forceinline__ void stage_tiles(const uint8_t *const (&src)[kTW], const uint32_t (&size)[kTW],
                                            uint8_t *const (&dst)[kTW], int lane) {
  uint32_t head[kTW], nd[kTW], ex[kTW], v[kTW], e[kTW];
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    head[i] = min(size[i], (uint32_t)(-reinterpret_cast<uintptr_t>(src[i]) & 3u));
    nd[i] = (size[i] - head[i]) >> 2;
    const uint32_t tail0 = head[i] + 4u * nd[i];
    ex[i] = (uint32_t)lane < head[i] ? (uint32_t)lane
            : (lane >= 4 && tail0 + (uint32_t)(lane - 4) < size[i]) ? tail0 + (uint32_t)(lane - 4) : ~0u;
    v[i] = e[i] = 0u;
    if (ex[i] != ~0u) e[i] = src[i][ex[i]];
    if ((uint32_t)lane < nd[i]) v[i] = *reinterpret_cast<const uint32_t *>(src[i] + head[i] + 4u * lane);
  }
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    if (ex[i] != ~0u) dst[i][ex[i]] = (uint8_t)e[i];
    if ((uint32_t)lane < nd[i]) put4(dst[i] + head[i] + 4u * lane, v[i]);
  }
#pragma unroll
  for (int i = 0; i < kTW; ++i)
    for (uint32_t d = (uint32_t)lane + 64u; d < nd[i]; d += 64u)
      put4(dst[i] + head[i] + 4u * d, *reinterpret_cast<const uint32_t *>(src[i] + head[i] + 4u * d));
}

// The staged records' verdicts and stream headers, a lane per tile (16 records
// checked at once: the rule reads each header only after the one before it).
struct RunRec {
  uint32_t so[kRun][3], m[kRun][3], md[kRun];
  int ok[kRun];
};

// tile j's stream offsets and meta words in registers (read from rr at every
// use, the re-codings took 3.5 to 6 % longer: profiles/stream_readers_refactor.md)
struct Streams {
  uint32_t so[3], m[3];
  __device__ __forceinline__ Streams(const RunRec &rr, int j)
      : so{rr.so[j][0], rr.so[j][1], rr.so[j][2]}, m{rr.m[j][0], rr.m[j][1], rr.m[j][2]} {}
};

template <bool kTightSrc>
__device__ __forceinline__ void rule_run(const RunSrc &run, const uint8_t (*stg)[kStage], int ntl, int tid,
                                         RunRec &rr) {
  if (tid >= ntl) return;
  uint32_t so[3] = {0u, 0u, 0u}, m[3] = {0u, 0u, 0u}, md = 0u;
  bool ok = run.where[tid] == 0;
  if (ok) {
    const uint8_t *const st = stg[tid];
    auto rd = [&](uint32_t x) -> uint32_t { return st[x]; };
    ok = record_rule<kTightSrc>(rd, 0u, run.size[tid], so, m, md);
  }
  rr.ok[tid] = ok;
  rr.md[tid] = md;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rr.so[tid][c] = so[c];
    rr.m[tid][c] = m[c];
  }
}

// Target JPT1.  A workgroup per 16 tiles: the run found (locate_run), then --
// unless the source is JPT1 too and the sizes are the records' own -- every
// wave's four JPR1 records staged in LDS, checked and their modes balloted.
__global__ __launch_bounds__(64 * kPW) void jprs_select_sizes_tight(const Sel s, size_t wg_base,
                                                                    uint32_t *__restrict__ tsz,
                                                                    uint8_t *__restrict__ out,
                                                                    uint64_t cap,
                                                                    uint64_t *__restrict__ result) {
  __shared__ RunSrc run;
  __shared__ RunRec rr;
  __shared__ alignas(16) uint8_t stg[kRun][kStage];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int src = source_format(s, lane);
  const int target = target_format(s, src);
  const uint64_t t0 = (wg_base + blockIdx.x) * kRun;
  if (t0 >= s.ntout) return;
  const int ntl = (int)min((uint64_t)kRun, s.ntout - t0);
  locate_run(s, src != 0, t0, ntl, tid, 0, run);
  __syncthreads();
  if (target == src || src == 0) {                      // the same in every workgroup: no re-coding
    if (tid < ntl)
      put_size(s, target, t0 + tid, run.where[tid] == 0 ? run.size[tid] : kEmptyRec, tsz, out, cap, result);
    return;
  }
  {
    const uint8_t *from[kTW];
    uint8_t *to[kTW];
    uint32_t size[kTW];
#pragma unroll
    for (int i = 0; i < kTW; ++i) {
      const int j = kTW * wv + i;
      const bool on = j < ntl && run.where[j] == 0;
      from[i] = s.in + (on ? run.o0[j] : 0);
      size[i] = on ? run.size[j] : 0u;
      to[i] = stg[j];
    }
    stage_tiles(from, size, to, lane);
  }
  __syncthreads();
  rule_run<false>(run, stg, ntl, tid, rr);
  __syncthreads();
  uint32_t sz[kTW];
#pragma unroll
  for (int i = 0; i < kTW; ++i) {                         // JPR1 -> JPT1: the four tables, then the ballots
    const int j = kTW * wv + i;                           // wave-uniform
    sz[i] = kEmptyRec;
    if (j < ntl && rr.ok[j]) {
      const uint8_t *const rec = stg[j];
      auto rd = [&](uint32_t x) -> uint32_t { return rec[x]; };
      const Streams r(rr, j);
      uint32_t tb[4];
      sz[i] = record_bytes(r.m, plain_table(rd, r.so, r.m, lane, tb));
    }
  }
  if (lane < kTW && kTW * wv + lane < ntl) {
    const uint32_t mine = lane == 0 ? sz[0] : lane == 1 ? sz[1] : lane == 2 ? sz[2] : sz[3];
    put_size(s, target, t0 + (uint64_t)(kTW * wv + lane), mine, tsz, out, cap, result);
  }
}

// ---- emit -----------------------------------------------------------------------

// where a checked record's streams begin in the image, modes omd; their headers
__device__ __forceinline__ void put_streams(const uint32_t (&m)[3], const uint32_t (&omd)[3], uint8_t *img,
                                            uint32_t o0, int lane, uint32_t (&o)[3]) {
  o[0] = o0;
  o[1] = o[0] + stream_bytes(m[0], 0, omd[0]);
  o[2] = o[1] + stream_bytes(m[1], 1, omd[1]);
  put_stream_headers(img, o, m, omd, lane);
}

// every stream's bit bytes, staged record (modes smd) to image (omd), 64 a round
__device__ __forceinline__ void put_bits(const uint8_t *st, const uint32_t (&so)[3], const uint32_t (&m)[3],
                                         const uint32_t (&smd)[3], const uint32_t (&omd)[3], uint8_t *img,
                                         const uint32_t (&o)[3], int lane) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint8_t *const from = st + bits_at(so[c], m[c] >> 24, smd[c]);
    uint8_t *const to = img + bits_at(o[c], m[c] >> 24, omd[c]);
    const uint32_t nby = ((m[c] & 0xFFFFu) + 7u) >> 3;
    for (uint32_t b = (uint32_t)lane; b < nby; b += 64u) to[b] = from[b];
  }
}

// A checked JPR1 record in st -> its JPT1 form at img + o0 (jpr_pack_emit's
// table writes; the words and the modes mds are plain_table's).
__device__ __forceinline__ void emit_tight(const uint8_t *st, const uint32_t (&so)[3], const uint32_t (&m)[3],
                                           const uint32_t (&tb)[4], uint32_t mds, uint8_t *img, uint32_t o0,
                                           int lane) {
  const uint32_t md[3] = {mds & 3u, (mds >> 2) & 3u, mds >> 4}, plain[3] = {0u, 0u, 0u};
  uint32_t o[3];
  put_streams(m, md, img, o0, lane, o);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = word_chan(q);
    put_table_word(img + o[c] + 4u, m[c] >> 24, md[c], word_entry(q, lane), tb[q]);
  }
  put_bits(st, so, m, plain, md, img, o, lane);
}

// A checked JPT1 record in st (modes mds) -> its JPR1 form at img + o0: modes
// 1 and 2 expanded to 3-B entries (an i8 to its i16), mode 0 copied.  An entry
// is read a branch a mode: through one reader shared with the thumbnails the call
// took 2 % longer (profiles/stream_readers_refactor.md).
__device__ __forceinline__ void emit_plain(const uint8_t *st, const uint32_t (&so)[3], const uint32_t (&m)[3],
                                           uint32_t mds, uint8_t *img, uint32_t o0, int lane) {
  const uint32_t md[3] = {mds & 3u, (mds >> 2) & 3u, mds >> 4}, plain[3] = {0u, 0u, 0u};
  uint32_t o[3];
  put_streams(m, plain, img, o0, lane, o);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = word_chan(q);
    const uint32_t k = word_entry(q, lane);
    const uint32_t nc = m[c] >> 24;
    if (k < nc) {
      const uint8_t *t = st + so[c] + 4u;
      uint32_t lo, hi, len;
      if (md[c] == 0) {
        lo = t[3u * k];
        hi = t[3u * k + 1];
        len = t[3u * k + 2];
      } else {
        len = (t[k >> 1] >> (4u * (k & 1u))) & 15u;
        t += (nc + 1u) >> 1;
        if (md[c] == 1) {
          lo = t[k];
          hi = (lo & 128u) ? 255u : 0u;                 // an i8 as an i16
        } else {
          lo = t[2u * k];
          hi = t[2u * k + 1];
        }
      }
      uint8_t *p = img + o[c] + 4u + 3u * k;
      p[0] = (uint8_t)lo;
      p[1] = (uint8_t)hi;
      p[2] = (uint8_t)len;
    }
  }
  put_bits(st, so, m, md, plain, img, o, lane);
}

// A workgroup's 16 output tiles -> stream bytes [G0, G1).  The run is found by
// 16 lanes of wave 1 while wave 0 finishes the scan; then wave v takes tiles
// 4 v .. 4 v + 3: their source records into LDS in one round (stage_tiles) --
// straight into the image for a copy, into the tiles' staging buffers for a
// re-coding: those are checked a lane per tile (rule_run), then the wave's 64
// lanes re-code a tile at a time.  Every byte of the range is written once
// (the records are dense), by byte stores.  A record is written only when its
// size is the scan's.  kRecode == false: the call keeps the source's format
// (format 0), so there is nothing to re-code and no staging buffers.
template <bool kRecode>
__global__ __launch_bounds__(64 * kPW, kRecode ? 4 : 6) void jprs_select_emit(
    const Sel s, size_t wg_base, const uint32_t *__restrict__ tsz, const uint32_t *__restrict__ gsum,
    const uint64_t *__restrict__ part, uint8_t *__restrict__ out, uint64_t cap,
    const uint64_t *__restrict__ out_len, uint64_t *__restrict__ result) {
  __shared__ uint64_t toff[kGT + 1];
  __shared__ RunSrc run;
  __shared__ alignas(16) uint8_t img[kImg];
  __shared__ RunRec rr;
  __shared__ alignas(16) uint8_t stg[kRecode ? kRun : 1][kRecode ? kStage : 16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int src = source_format(s, lane);
  const int target = target_format(s, src);
  const auto [g, t0, h0, ntl] = run_of(wg_base + blockIdx.x, (size_t)s.ntout);
  if (t0 >= s.ntout) return;
  if (wg_base + blockIdx.x == 0 && tid == 0) result[0] = *out_len;     // the scan's end
  group_offsets(tid, g, (size_t)s.ntout, tsz, gsum, part, toff);
  locate_run(s, src != 0, t0, ntl, tid, 64, run);
  __syncthreads();
  const uint64_t G0 = toff[h0], G1 = toff[h0 + ntl];
  const uint32_t lead = (uint32_t)(((uintptr_t)out + G0) & 15);        // img[lead] = stream byte G0
  const bool recode = kRecode && target != src && src != 0;            // the same in every workgroup

  uint32_t o[kTW], osz[kTW];
  bool done[kTW];
  {
    const uint8_t *from[kTW];
    uint8_t *to[kTW];
    uint32_t size[kTW];
#pragma unroll
    for (int i = 0; i < kTW; ++i) {
      const int j = kTW * wv + i;
      const bool on = j < ntl;
      o[i] = on ? lead + (uint32_t)(toff[h0 + j] - G0) : 0u;
      osz[i] = on ? (uint32_t)(toff[h0 + j + 1] - toff[h0 + j]) : 0u;
      const bool found = on && run.where[j] == 0;
      done[i] = found && !recode && osz[i] == run.size[j];             // the copy: straight into the image
      from[i] = s.in + (found ? run.o0[j] : 0);
      size[i] = (recode ? found : done[i]) ? run.size[j] : 0u;
      to[i] = recode ? stg[on ? j : 0] : img + o[i];
    }
    stage_tiles(from, size, to, lane);
  }
  if constexpr (kRecode) {
    if (recode) {
      __syncthreads();
      if (src == JPEGR_STREAM_JPR1)
        rule_run<false>(run, stg, ntl, tid, rr);
      else
        rule_run<true>(run, stg, ntl, tid, rr);
      __syncthreads();
      if (src == JPEGR_STREAM_JPR1) {                   // -> JPT1: the four tables and their ballots first
        uint32_t tb[kTW][4], mds[kTW];
#pragma unroll
        for (int i = 0; i < kTW; ++i) {
          const int j = kTW * wv + i;                   // wave-uniform
          mds[i] = ~0u;
          if (j < ntl && rr.ok[j]) {
            const uint8_t *const st = stg[j];
            auto rd = [&](uint32_t x) -> uint32_t { return st[x]; };
            const Streams r(rr, j);
            mds[i] = plain_table(rd, r.so, r.m, lane, tb[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < kTW; ++i) {
          const int j = kTW * wv + i;
          if (mds[i] == ~0u) continue;
          const Streams r(rr, j);
          if (record_bytes(r.m, mds[i]) == osz[i]) {
            emit_tight(stg[j], r.so, r.m, tb[i], mds[i], img, o[i], lane);
            done[i] = true;
          }
        }
      } else {                                          // -> JPR1
#pragma unroll
        for (int i = 0; i < kTW; ++i) {
          const int j = kTW * wv + i;
          if (j >= ntl || !rr.ok[j]) continue;
          const Streams r(rr, j);
          if (record_bytes(r.m, 0u) == osz[i]) {
            emit_plain(stg[j], r.so, r.m, rr.md[j], img, o[i], lane);
            done[i] = true;
          }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kTW; ++i) {
    const int j = kTW * wv + i;
    if (j >= ntl || done[i]) continue;                  // wave-uniform
    if ((uint32_t)lane < osz[i]) img[o[i] + lane] = 0;  // the empty record: osz is 12 here
    if (lane == 0) {
      if (run.where[j] == 1) {
        if (t0 + j == run.k[j] * s.opt)                 // the item's first tile speaks for it
          atomicMin(reinterpret_cast<unsigned long long *>(result + 1), 1ull + (unsigned long long)run.k[j]);
      } else {
        atomicAdd(reinterpret_cast<unsigned long long *>(result + 2), 1ull);
      }
    }
  }
  __syncthreads();
  image_out(img, tid, lane, wv, G0, G1, lead, out, cap);
}

// the output's tiles, 0 on a bad argument
inline size_t out_tiles(size_t nitems, int out_w, int out_h) {
  if (nitems == 0 || nitems > (size_t)INT_MAX) return 0;
  return tiles_of(out_w, out_h, (int)nitems);
}

}  // namespace

extern "C" size_t jpegr_select_scratch_bytes(size_t nitems, int out_w, int out_h) {
  const size_t nt = out_tiles(nitems, out_w, out_h);
  return nt ? scratch_of(nullptr, nt).bytes : 0;
}

extern "C" int jpegr_select_device(const void *d_in, size_t in_len, int w, int h, int nimg,
                                   const void *d_tile_offsets, const void *d_items, size_t nitems,
                                   int out_w, int out_h, int format, void *d_out, size_t cap,
                                   void *d_out_len, void *d_scratch, void *d_result, void *stream) {
  const size_t ntiles = tiles_of(w, h, nimg);
  if (!d_in || !d_tile_offsets || !d_items || !d_out || !d_out_len || !d_scratch || !d_result ||
      ntiles == 0 || out_w <= 0 || out_h <= 0 || out_w > w || out_h > h ||
      (format != 0 && format != JPEGR_STREAM_JPR1 && format != JPEGR_STREAM_JPT1) ||
      in_len < (size_t)kHdr || misaligned(d_out, 15) || misaligned(d_scratch, 15) ||
      misaligned(d_tile_offsets, 7) || misaligned(d_items, 7) || misaligned(d_out_len, 7) ||
      misaligned(d_result, 7))
    return JPEGR_ERR_ARG;
  const size_t ntout = out_tiles(nitems, out_w, out_h);
  if (ntout == 0) return JPEGR_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Sel s;
  s.in = static_cast<const uint8_t *>(d_in);
  s.in_len = (uint64_t)in_len;
  s.toff = static_cast<const uint64_t *>(d_tile_offsets);
  s.items = static_cast<const jpegr_sel *>(d_items);
  s.per = (uint64_t)(ntiles / (size_t)nimg);
  s.opt = (uint64_t)(ntout / nitems);
  s.ntout = (uint64_t)ntout;
  s.w = (uint32_t)w;
  s.h = (uint32_t)h;
  s.nimg = (uint32_t)nimg;
  s.gw = (uint32_t)(((int64_t)w + 7) / 8);
  s.ogw = (uint32_t)(((int64_t)out_w + 7) / 8);
  s.out_w = (uint32_t)out_w;
  s.out_h = (uint32_t)out_h;
  s.nitems = (uint32_t)nitems;
  s.format = format;
  const Scratch sc = scratch_of(d_scratch, ntout);
  auto *out = static_cast<uint8_t *>(d_out);
  auto *len = static_cast<uint64_t *>(d_out_len);
  auto *result = static_cast<uint64_t *>(d_result);
  if (format == JPEGR_STREAM_JPT1)
    launch_chunks(ntout, kRun, [&](size_t b, unsigned n) {
      hipLaunchKernelGGL(jprs_select_sizes_tight, dim3(n), dim3(64 * kPW), 0, st, s, b, sc.tsz, out,
                         (uint64_t)cap, result);
    });
  else
    launch_chunks(ntout, 256, [&](size_t b, unsigned n) {
      hipLaunchKernelGGL(jprs_select_sizes, dim3(n), dim3(256), 0, st, s, b * 256, sc.tsz, out, (uint64_t)cap,
                         result);
    });
  scan(sc, ntout, len, st);
  launch_chunks(ntout, kRun, [&](size_t b, unsigned n) {
    if (format == 0)
      hipLaunchKernelGGL(jprs_select_emit<false>, dim3(n), dim3(64 * kPW), 0, st, s, b, sc.tsz, sc.gsum, sc.part,
                         out, (uint64_t)cap, len, result);
    else
      hipLaunchKernelGGL(jprs_select_emit<true>, dim3(n), dim3(64 * kPW), 0, st, s, b, sc.tsz, sc.gsum, sc.part,
                         out, (uint64_t)cap, len, result);
  });
  return hipGetLastError() == hipSuccess ? JPEGR_OK : JPEGR_ERR_HIP;
}
