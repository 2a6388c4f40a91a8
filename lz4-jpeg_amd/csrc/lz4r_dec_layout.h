// lz4r_dec_layout.h -- what the decoder's kernels and its host side agree on:
// the block grid, the bare-stream chunking and sentinels, the control words a
// bare-stream call leaves on the device, and the carving of its scratch block.
// Plain C++ (no HIP types), so the layout is checked on the CPU
// (tests/sanitize/bare_layout.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lz4r.h"

namespace {

constexpr int kBlk = LZ4R_BLOCK;
constexpr int kInMax = LZ4R_BLOCK_BOUND;   // bytes of one encoded block (bound)
constexpr int kLanes = 64;                 // threads per workgroup (one wave)
// blocks per wave (lanes 0 .. kBPW-1 decode; all 64 lanes store the wave's
// output): 32 x 300 B of LDS lets 16 waves share a CU where 64 blocks per wave
// allowed 8 -- the walk is latency-bound, so more, narrower waves win (1 GiB:
// 64 -> 1.68 ms, 48 -> 1.68, 40 -> 1.68, 32 -> 1.59, 24 -> 1.61, 16 -> 1.95)
constexpr int kBPW = 32;

// bare streams (lz4r_dec_bare.h)
constexpr int kChunkB = 8192;                        // stream bytes per chunk
constexpr int kList = 32;                            // block starts listed per chunk by the walk
constexpr int kMisCap = 1024;                        // inconsistent chunks listed (more: all checked)
constexpr uint64_t kNone = ~0ull;                    // no candidate in the chunk
constexpr uint64_t kBad = ~0ull - 1;                 // the walk met an impossible block

// The control words of a bare-stream call: u64 each, read back in one copy of
// kCtlWords; lz4_decode_blocks' `result` is the pair at kCtlLen (kResLen,
// kResFail).  The u32 at u64 index kCtlNmis counts the inconsistent chunks.
constexpr int kCtlNb = 0;       // blocks in the stream (lz4_bare_scan)
constexpr int kCtlStatus = 1;   // 0: the chunk chain holds, else 1 + the chunk where it broke
constexpr int kCtlLen = 2;      // decoded bytes (written by the last block's lane)
constexpr int kCtlFail = 3;     // first failed block + 1 (atomicMin; ~0: none)
constexpr int kCtlGate = 4;     // lz4_bare_gate's verdict, below
constexpr int kCtlWords = 5;
constexpr int kCtlNmis = 5;
constexpr int kResLen = 0, kResFail = kCtlFail - kCtlLen;
constexpr unsigned long long kGateGo = 0;        // decode
constexpr unsigned long long kGateCorrupt = 1;   // broken chain, no block, or a wrong frame byte
constexpr unsigned long long kGateCapacity = 2;  // more blocks than the output can hold

// The scratch block of one bare-stream call: region byte offsets from the
// base and the total, from the chunk count and the offsets array's size
// (nb_cap 0: that array is allocated once the block count is known), and the
// typed pointers once bound to the allocation.  Every region starts 16-B
// aligned where it matters: lz4_bare_walk stores the lists as uint4.
struct BareScratch {
  size_t nchunks, ng;                  // chunks, waves of 64 chunks
  // byte offsets of the regions that do not simply follow their neighbour
  // (cand at 0, exitp after it; gbase after gsum), and the total
  size_t o_gsum, o_ctl, o_mis, o_cnt, o_lok, o_lists, o_boff, bytes;
  uint64_t *cand, *exitp;              // u64 per chunk: candidate start, walk exit
  unsigned long long *gsum, *gbase;    // u64 per 64 chunks: block count, its exclusive scan
  unsigned long long *ctl;             // the control words (64 B)
  unsigned int *nmis, *mis;            // ctl's u32; u32 x kMisCap: the inconsistent chunks
  uint32_t *cnt, *lok;                 // u32 per chunk: blocks, list-valid
  uint16_t *lists;                     // u16 x kList per chunk: the first block starts
  uint64_t *boff;                      // u64 x nb_cap: the block offsets

  void bind(uint8_t *base) {
    cand = reinterpret_cast<uint64_t *>(base);
    exitp = cand + nchunks;
    gsum = reinterpret_cast<unsigned long long *>(base + o_gsum);
    gbase = gsum + ng;
    ctl = reinterpret_cast<unsigned long long *>(base + o_ctl);
    nmis = reinterpret_cast<unsigned int *>(ctl + kCtlNmis);
    mis = reinterpret_cast<unsigned int *>(base + o_mis);
    cnt = reinterpret_cast<uint32_t *>(base + o_cnt);
    lok = reinterpret_cast<uint32_t *>(base + o_lok);
    lists = reinterpret_cast<uint16_t *>(base + o_lists);
    boff = reinterpret_cast<uint64_t *>(base + o_boff);
  }
};

inline BareScratch bare_scratch_layout(size_t nchunks, size_t nb_cap) {
  auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  BareScratch L = {};
  L.nchunks = nchunks;
  L.ng = (nchunks + 63) / 64;
  L.o_gsum = 16 * nchunks;
  L.o_ctl = L.o_gsum + 16 * L.ng;
  L.o_mis = L.o_ctl + 64;
  L.o_cnt = L.o_mis + 4 * (size_t)kMisCap;
  L.o_lok = al16(L.o_cnt + 4 * nchunks);
  L.o_lists = al16(L.o_lok + 4 * nchunks);
  L.o_boff = al16(L.o_lists + 2 * (size_t)kList * nchunks);
  L.bytes = L.o_boff + 8 * nb_cap;
  return L;
}

}  // namespace
