/*
 * frame_dev_main.cpp -- TEST INFRASTRUCTURE ONLY: what the GPU frame decoder's
 * kernels parse with (csrc/lz4f_parse.h), compiled for the host under ASan +
 * UBSan (`make sanitize-frame-dev`; tests/test_sanitize_frame_dev.py).  A
 * stand-alone program.  It runs the stages of lz4r_frame_decompress_device in
 * their order -- walk, block checksums, sizes, offsets and content sizes, the
 * capacity, a serial copy per chain with the kernel's periodic-match formula,
 * content checksums -- over plain memory, and compares the verdict, the length
 * and the bytes with lz4r_frame_decompress (host/lz4f_decode.c).
 *
 * Inputs: the frames of tests/lz4_frame_model.py's variants() (independent,
 * linked, stored, checksums, no content size, 4 MiB class, two frames), built
 * here over a small text; every proper prefix of each; every single-byte
 * mutation of each; too small a capacity on each.  Every input is a heap copy
 * of exactly its length and every output a heap buffer of exactly the decoded
 * length, so a read or write one byte outside is the sanitizer's to report.
 * What this covers is the parsers' own arithmetic: which bytes they ask for and
 * which they copy.  How the kernels fetch those bytes (the LDS window of
 * csrc/lz4f_dec.h, with its aligned and bytewise loads at the input's ends) is
 * device code and is not run here.
 * Prints "sanitize-frame-dev ok".
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lz4r.h"
#include "../../lz4-jpeg_amd/csrc/lz4f_parse.h"

namespace {

typedef std::vector<uint8_t> Bytes;

// ---- frames, as tests/lz4_frame_model.py writes them --------------------------

void put32(Bytes &o, uint32_t v) {
  for (int i = 0; i < 4; ++i) o.push_back((uint8_t)(v >> (8 * i)));
}

void put_ext(Bytes &o, size_t x) {
  if (x < 15) return;
  for (x -= 15; x >= 255; x -= 255) o.push_back(255);
  o.push_back((uint8_t)x);
}

// a conforming block of data[lo, hi): greedy, matches reach back to window_lo
Bytes compress_block(const Bytes &d, size_t lo, size_t hi, size_t window_lo) {
  Bytes o;
  size_t anchor = lo, p = lo;
  while (p + 12 <= hi) {
    size_t best = 0, at = 0;
    for (size_t q = window_lo; q < p; ++q) {
      size_t ml = 0;
      while (p + ml + 5 < hi && d[q + ml] == d[p + ml]) ++ml;
      if (ml >= 4 && ml > best && p - q <= 65535) best = ml, at = q;
    }
    if (!best) {
      ++p;
      continue;
    }
    const size_t L = p - anchor;
    o.push_back((uint8_t)((L < 15 ? L : 15) << 4 | (best - 4 < 15 ? best - 4 : 15)));
    put_ext(o, L);
    o.insert(o.end(), d.begin() + anchor, d.begin() + p);
    o.push_back((uint8_t)(p - at));
    o.push_back((uint8_t)((p - at) >> 8));
    put_ext(o, best - 4);
    p += best;
    anchor = p;
  }
  const size_t L = hi - anchor;
  o.push_back((uint8_t)((L < 15 ? L : 15) << 4));
  put_ext(o, L);
  o.insert(o.end(), d.begin() + anchor, d.begin() + hi);
  return o;
}

struct Variant {
  size_t block = 64;
  bool linked = false, block_checksum = false, content_checksum = false, content_size = true;
  uint8_t bd = 0x40;
  std::vector<size_t> stored;
};

Bytes write_variant(const Bytes &plain, const Variant &v) {
  Bytes o = {0x04, 0x22, 0x4D, 0x18};
  const uint8_t flg = (uint8_t)(0x40 | (v.linked ? 0 : 0x20) | (v.block_checksum ? 0x10 : 0) |
                                (v.content_size ? 0x08 : 0) | (v.content_checksum ? 0x04 : 0));
  o.push_back(flg);
  o.push_back(v.bd);
  if (v.content_size)
    for (int i = 0; i < 8; ++i) o.push_back((uint8_t)((uint64_t)plain.size() >> (8 * i)));
  o.push_back((uint8_t)(lz4f_xxh32(o.data() + 4, o.size() - 4, 0) >> 8));
  size_t i = 0;
  for (size_t lo = 0; lo < plain.size(); lo += v.block, ++i) {
    const size_t hi = lo + v.block < plain.size() ? lo + v.block : plain.size();
    Bytes body;
    bool stored = false;
    for (size_t s : v.stored) stored |= s == i;
    if (stored)
      body.assign(plain.begin() + lo, plain.begin() + hi);
    else
      body = compress_block(plain, lo, hi, v.linked ? 0 : lo);
    put32(o, (uint32_t)body.size() | (stored ? 0x80000000u : 0));
    o.insert(o.end(), body.begin(), body.end());
    if (v.block_checksum) put32(o, lz4f_xxh32(body.data(), body.size(), 0));
  }
  put32(o, 0);
  if (v.content_checksum) put32(o, lz4f_xxh32(plain.data(), plain.size(), 0));
  return o;
}

// ---- the device decoder's stages over plain memory -----------------------------

struct MemSrc {
  const uint8_t *p;
  uint32_t at(size_t i) { return p[i]; }
};

struct VecSink {
  std::vector<Lz4fBlock> blocks;
  std::vector<Lz4fFrame> frames;
  void block(uint64_t i, const Lz4fBlock &b) {
    if (i != blocks.size()) abort();
    blocks.push_back(b);
  }
  void frame(uint64_t i, const Lz4fFrame &f) {
    if (i != frames.size()) abort();
    frames.push_back(f);
  }
};

struct MemOut {
  const uint8_t *in;
  uint8_t *out;
  void literals(size_t op, size_t lit, uint32_t L) {
    if (L) memcpy(out + op, in + lit, L);
  }
  // as the kernel's lanes: D < M is periodic, byte i = out[op - D + i % D]
  void match(size_t op, uint32_t D, uint32_t M) {
    for (uint32_t i = 0; i < M; ++i) out[op + i] = out[op - D + (D < M ? i % D : i)];
  }
};

// *out: a heap buffer of exactly the decoded length (nullptr: nothing decoded)
int dev_decode(const uint8_t *in, size_t in_len, size_t cap, uint8_t **out_buf, size_t *out_len,
               unsigned flags) {
  *out_buf = nullptr;
  *out_len = 0;
  MemSrc s = {in};
  VecSink k;
  uint64_t nb = 0, nf = 0, ns = 0;
  if (lz4f_walk_frames(s, in_len, k, &nb, &nf, &ns)) return LZ4R_ERR_CORRUPT;
  if (nb != k.blocks.size() || nf != k.frames.size()) abort();
  bool bad = false;
  std::vector<uint64_t> off(nb + 1, 0);
  for (size_t b = 0; b < nb; ++b) {
    const Lz4fBlock &e = k.blocks[b];
    uint32_t n = lz4f_block_bytes(e.word);
    if ((e.word & kLz4fBsum) &&
        lz4f_xxh32(in + e.in_off, n, 0) != lz4f_le32(in + e.in_off + n))
      bad = true;
    if (!(e.word & kLz4fStored) &&
        lz4f_block_size(s, (size_t)e.in_off, (size_t)e.in_off + n, lz4f_block_max(e.word), &n)) {
      n = 0;
      bad = true;
    }
    off[b + 1] = off[b] + n;
  }
  for (const Lz4fFrame &f : k.frames)
    if (f.has_want && off[f.first_block + f.nblocks] - off[f.first_block] != f.want) bad = true;
  if (bad) return LZ4R_ERR_CORRUPT;
  const size_t total = (size_t)off[nb];
  if (total > cap) {
    *out_len = total;
    return LZ4R_ERR_CAPACITY;
  }
  uint8_t *out = (uint8_t *)malloc(total ? total : 1);
  if (!out) abort();
  *out_buf = out;
  MemOut o = {in, out};
  for (size_t b = 0; b < nb; ++b) {
    const Lz4fBlock &e = k.blocks[b];
    const size_t ip = (size_t)e.in_off, n = lz4f_block_bytes(e.word);
    const size_t base = (e.word & kLz4fLinked) ? (size_t)off[k.frames[e.frame].first_block]
                                                : (size_t)off[b];
    size_t op = (size_t)off[b];
    if (e.word & kLz4fStored)
      o.literals(op, ip, (uint32_t)n);
    else if (lz4f_decode_block(s, ip, ip + n, o, base, &op, (size_t)off[b + 1]) ||
             op != off[b + 1])
      return LZ4R_ERR_CORRUPT;
  }
  if (!(flags & LZ4R_FRAME_NO_CONTENT_CHECKSUM))
    for (const Lz4fFrame &f : k.frames) {
      const size_t lo = (size_t)off[f.first_block], hi = (size_t)off[f.first_block + f.nblocks];
      if (f.has_csum && lz4f_xxh32(out + lo, hi - lo, 0) != lz4f_le32(in + f.csum_pos))
        return LZ4R_ERR_CORRUPT;
    }
  *out_len = total;
  return LZ4R_OK;
}

// ---- one input through both decoders -------------------------------------------

size_t g_ok, g_corrupt;

// the host decoder with room for anything len bytes can decode to (a byte of
// input adds at most 255 of output), so that it never answers "capacity"
void agree(const char *what, size_t index, const uint8_t *frame, size_t len) {
  uint8_t *in = (uint8_t *)malloc(len ? len : 1);
  const size_t room = 255 * len + 64;
  uint8_t *ref = (uint8_t *)malloc(room), *dev = nullptr;
  if (!in || !ref) abort();
  memcpy(in, frame, len);
  size_t ref_len = 0, dev_len = 0;
  const int want = lz4r_frame_decompress(in, len, ref, room, &ref_len);
  const int got = dev_decode(in, len, room, &dev, &dev_len, 0);
  if (got != want || (want == LZ4R_OK && (dev_len != ref_len || memcmp(dev, ref, ref_len) != 0))) {
    fprintf(stderr, "%s %zu: the host decoder says %d (%zu bytes), the device stages %d (%zu)\n",
            what, index, want, ref_len, got, dev_len);
    exit(1);
  }
  if (want != LZ4R_OK && want != LZ4R_ERR_CORRUPT) {
    fprintf(stderr, "%s %zu: rc %d\n", what, index, want);
    exit(1);
  }
  (want == LZ4R_OK ? g_ok : g_corrupt) += 1;
  free(dev);
  free(ref);
  free(in);
}

}  // namespace

int main() {
  // 330 bytes that compress: phrases repeated at several distances
  std::string t;
  const char *words[] = {"the frame ", "decoder walks ", "block after block ", "0123456789",
                         "and checks every bound ", "aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa"};
  for (int i = 0; t.size() < 330; ++i) t += words[(i * 7 + i / 3) % 6];
  const Bytes plain(t.begin(), t.begin() + 330);

  std::vector<std::pair<const char *, Bytes>> frames;
  Variant v;
  frames.push_back({"independent", write_variant(plain, v)});
  v.linked = true;
  frames.push_back({"linked", write_variant(plain, v)});
  v = Variant();
  v.stored = {0, 2};
  frames.push_back({"stored", write_variant(plain, v)});
  v = Variant();
  v.linked = v.block_checksum = v.content_checksum = true;
  frames.push_back({"checksums", write_variant(plain, v)});
  v = Variant();
  v.content_size = false;
  frames.push_back({"no content size", write_variant(plain, v)});
  v = Variant();
  v.block = 1000;
  v.bd = 0x70;
  frames.push_back({"4 MiB class", write_variant(plain, v)});
  {
    const Bytes a(plain.begin(), plain.begin() + 100), b(plain.begin() + 100, plain.end());
    v = Variant();
    v.linked = true;
    Bytes two = write_variant(a, v);
    v = Variant();
    v.content_checksum = true;
    const Bytes second = write_variant(b, v);
    two.insert(two.end(), second.begin(), second.end());
    frames.push_back({"two frames", two});
  }

  for (auto &f : frames) {
    const Bytes &fr = f.second;
    const size_t n = fr.size();
    // the frame itself: both decode it to the text
    uint8_t *dev = nullptr;
    size_t dev_len = 0;
    Bytes copy(fr);
    int rc = dev_decode(copy.data(), n, plain.size(), &dev, &dev_len, 0);
    if (rc != LZ4R_OK || dev_len != plain.size() || memcmp(dev, plain.data(), dev_len) != 0) {
      fprintf(stderr, "%s: the device stages do not decode it: rc %d, %zu bytes\n", f.first, rc,
              dev_len);
      return 1;
    }
    free(dev);
    agree(f.first, n, fr.data(), n);
    // too little room: the exact length, nothing allocated; the host agrees on the code
    for (size_t cap : {(size_t)0, plain.size() - 1}) {
      rc = dev_decode(copy.data(), n, cap, &dev, &dev_len, 0);
      Bytes small(cap ? cap : 1);
      size_t need = 0;
      const int want = lz4r_frame_decompress(copy.data(), n, small.data(), cap, &need);
      if (rc != LZ4R_ERR_CAPACITY || want != rc || dev_len != plain.size() || dev) {
        fprintf(stderr, "%s, cap %zu: rc %d (host %d), length %zu\n", f.first, cap, rc, want,
                dev_len);
        return 1;
      }
    }
    for (size_t k = 0; k < n; ++k) agree("prefix", k, fr.data(), k);
    Bytes bad(fr);
    for (size_t i = 0; i < n; ++i) {
      for (int x = 0; x < 256; ++x) {
        if (x == fr[i]) continue;
        bad[i] = (uint8_t)x;
        agree(f.first, i, bad.data(), n);
      }
      bad[i] = fr[i];
    }
  }
  // a wrong content checksum passes when the flag says not to look
  {
    Bytes fr = frames[3].second;
    fr[fr.size() - 1] ^= 1;
    uint8_t *dev = nullptr;
    size_t dev_len = 0;
    if (dev_decode(fr.data(), fr.size(), plain.size(), &dev, &dev_len, 0) != LZ4R_ERR_CORRUPT)
      return 1;
    free(dev);
    if (dev_decode(fr.data(), fr.size(), plain.size(), &dev, &dev_len,
                   LZ4R_FRAME_NO_CONTENT_CHECKSUM) != LZ4R_OK ||
        memcmp(dev, plain.data(), plain.size()) != 0)
      return 1;
    free(dev);
  }
  printf("sanitize-frame-dev ok (%zu frames; %zu inputs decode, %zu are corrupt, in both decoders)\n",
         frames.size(), g_ok, g_corrupt);
  return 0;
}
