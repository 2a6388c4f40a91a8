// lz4r_layout.h -- what lz4_tiles, the scan kernels, lz4_emit and the host's
// run() agree on: the block grid, the record scratch lz4_tiles writes and
// lz4_emit reads, the scan's grouping and the length word's error bit.
// Record scratch of one block: a header dword, then a dword per sequence (<= 121).
//   header   sum of the sequences' size fields (LZ4.c:546-575) | sequence
//            count << 16
//   record   dist | M << 9 | (match start + M) << 19 -- the sequence's match;
//            its literal run starts where the previous record's match ends
//            (0 for the first).  The literal-only tail, when the last match
//            ends before the block does, is n << 19 (M = dist = 0).
#pragma once
#include <stdint.h>

#include "../../include/lz4r.h"

namespace {

constexpr int kBlk = LZ4R_BLOCK;          // 300
constexpr int kBlkOutMax = 560;           // >= 548: worst-case bytes of one block, 16-B multiple

// lz4_tiles: consecutive blocks one wave (= one workgroup) encodes, one after
// the other (a static run; DESIGN 8 has the A/B over 1, 2, 4, 8, 16).  The
// host rounds an XCD's slice of the launch up to whole runs.
#ifndef LZ4R_RUN
#define LZ4R_RUN 16
#endif
constexpr int kTileRun = LZ4R_RUN;
static_assert(kTileRun >= 1 && kTileRun <= 64, "blocks per lz4_tiles workgroup");

// The first kHeadW dwords (header + 23 records: all of a text block's but for
// ~7 % of blocks) go to a dense head array, kHead bytes per block, so lz4_emit
// reads its 32 blocks' heads as one contiguous 3 KB run of 16-B loads (no
// 128-B line per block of which ~60 B were used); records 23.. go to a
// per-block overflow slot of kOvf bytes.
constexpr int kHeadW = 24;
constexpr int kHead = 4 * kHeadW;        // 96 B
constexpr int kOvf = 400;                // records 23..120: <= 98 dwords
constexpr int kSlot = kHead + kOvf;      // scratch bytes per block
static_assert(kHead % 16 == 0 && kOvf % 16 == 0 && 4 * (121 + 1 - kHeadW) <= kOvf,
              "aligned head and overflow slots");

// placement: exclusive scan of the blocks' byte counts, then lz4_emit per group
constexpr int kGT = 64;              // blocks per scan group
constexpr int kPart = 64 * kGT;      // blocks per scan partial (64 groups)
static_assert(kPart % kGT == 0, "partials hold whole groups");

// bit 63 of the length word a call leaves: a block saw a corrupt bucket head
// (set by the call's last scan, lz4r_scan.h, read back by the host)
constexpr uint64_t kLenCorrupt = 1ull << 63;

}  // namespace
