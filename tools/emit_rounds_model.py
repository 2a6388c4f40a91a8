#!/usr/bin/env python3
"""CPU model of lz4_emit's sequence rounds: how many rounds of 64
records and literal-word iterations a workgroup of 32 blocks executes, and how
many its slowest wave runs, when

  per wave      each of the 8 waves flattens its own 4 blocks;
  flattened     the workgroup's records take indices 0 .. T-1 and round r
                (records [64 r, 64 r + 64)) goes to wave r % 8.

    python3 tools/emit_rounds_model.py [passages] [seed]

Input: `passages` (128) random 30,000-byte passages of the bench corpus (the
golden text, newlines turned to spaces), 300-byte blocks, encoded block by
block by the oracle; the literal words of a record are the aligned 16-byte
words of the framed stream its literal run touches.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "lz4-jpeg_amd"), os.path.join(REPO, "tests")]
import oracle_api  # noqa: E402
from lz4jpeg import synth  # noqa: E402

BLK, WG, WAVES, ROUND = 300, 32, 8, 64


def records(enc, at):
    """Literal-word count of each record of one encoded block whose first byte
    is stream byte `at` (text: no truncated match, so the token tells every
    field that follows it)."""
    n, out, p = enc[0], [], 3
    for _ in range(n):
        tl, tm = enc[p] >> 4, enc[p] & 15
        sz = enc[p + 1] | enc[p + 2] << 8
        le = 0 if tl < 15 else (2 if enc[p + 3] == 255 else 1)
        mext = 1 if tm == 15 else 0
        L = sz - 5 - le - mext
        ol = at + p + 3 + le
        out.append(((ol + L - 1) >> 4) - (ol >> 4) + 1 if L > 0 else 0)
        p += sz
    assert p == len(enc), (p, len(enc))
    return out


def iters(words):
    """Rounds and literal iterations of records dealt in rounds of 64."""
    r = [words[i:i + ROUND] for i in range(0, len(words), ROUND)]
    return [(1, max(1, -(-sum(x) // ROUND))) for x in r]


def main():
    passages = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    data = synth.random_passages(passages * 30000, length=30000, seed=seed)
    orc = oracle_api.load()
    nb = data.size // BLK
    per_block, at = [], 1
    for b in range(nb):
        enc = orc.lz4_blocks(data, b, b + 1)
        per_block.append(records(enc, at))
        at += len(enc)
    counts = np.array([len(x) for x in per_block])
    rows = {"per wave": [], "flattened": []}
    second = wgs_second = 0
    for w0 in range(0, nb - WG + 1, WG):
        blk = per_block[w0:w0 + WG]
        per = WG // WAVES
        waves = [iters(sum(blk[per * v:per * v + per], [])) for v in range(WAVES)]
        second += sum(len(v) > 1 for v in waves)
        wgs_second += any(len(v) > 1 for v in waves)
        rows["per wave"].append(waves)
        flat = iters(sum(blk, []))
        rows["flattened"].append([flat[v::WAVES] for v in range(WAVES)])
    nwg = len(rows["per wave"])
    T = np.add.reduceat(counts[:nwg * WG], np.arange(0, nwg * WG, WG))
    print(f"{nb} blocks, {nwg} workgroups; records per block {counts.mean():.2f} "
          f"(sigma {counts.std():.2f}); T mean {T.mean():.1f}, T > 512 in "
          f"{100 * (T > 512).mean():.0f} % of workgroups")
    print(f"second rounds today: {100 * second / (nwg * WAVES):.0f} % of waves, "
          f"{100 * wgs_second / nwg:.0f} % of workgroups")
    print("| per workgroup of 32 blocks | per wave | flattened |\n|---|---|---|")
    names = ("sequence rounds executed", "literal-word loop iterations executed",
             "slowest wave: sequence rounds", "slowest wave: literal iterations")
    vals = []
    for key in ("per wave", "flattened"):
        wg = rows[key]
        tot_r = np.mean([sum(a for v in w for a, _ in v) for w in wg])
        tot_l = np.mean([sum(c for v in w for _, c in v) for w in wg])
        max_r = np.mean([max(sum(a for a, _ in v) for v in w) for w in wg])
        max_l = np.mean([max(sum(c for _, c in v) for v in w) for w in wg])
        vals.append((tot_r, tot_l, max_r, max_l))
    for i, nme in enumerate(names):
        print(f"| {nme} | {vals[0][i]:.2f} | {vals[1][i]:.2f} |")


if __name__ == "__main__":
    main()
