/* lz4f_xxh32.h -- XXH32 (the xxHash 32-bit digest, as its specification states
 * it), the checksum of the LZ4 frame format: the header byte HC, block and
 * content checksums.  Plain C, one-shot and streaming (the content checksum
 * runs over a frame's blocks as they are decoded). */
#ifndef LZ4F_XXH32_H
#define LZ4F_XXH32_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define LZ4F_P1 2654435761u
#define LZ4F_P2 2246822519u
#define LZ4F_P3 3266489917u
#define LZ4F_P4 668265263u
#define LZ4F_P5 374761393u

/* every function here also compiles as device code of a HIP source (the GPU
 * frame decoder's checksums, csrc/lz4f_dec.h, are these functions) */
#if defined(__HIPCC__)
#define LZ4F_FN __host__ __device__ static inline
#else
#define LZ4F_FN static inline
#endif

typedef struct lz4f_xxh32_state {
  uint32_t v[4];
  uint8_t buf[16];
  uint32_t nbuf;
  uint64_t total;
  uint32_t seed;
} lz4f_xxh32_state;

LZ4F_FN uint32_t lz4f_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

LZ4F_FN uint32_t lz4f_le32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

LZ4F_FN uint32_t lz4f_round(uint32_t acc, uint32_t lane) {
  return lz4f_rotl(acc + lane * LZ4F_P2, 13) * LZ4F_P1;
}

LZ4F_FN void lz4f_xxh32_init(lz4f_xxh32_state *s, uint32_t seed) {
  s->v[0] = seed + LZ4F_P1 + LZ4F_P2;
  s->v[1] = seed + LZ4F_P2;
  s->v[2] = seed;
  s->v[3] = seed - LZ4F_P1;
  s->nbuf = 0;
  s->total = 0;
  s->seed = seed;
}

LZ4F_FN void lz4f_stripe(lz4f_xxh32_state *s, const uint8_t *p) {
  for (int i = 0; i < 4; ++i) s->v[i] = lz4f_round(s->v[i], lz4f_le32(p + 4 * i));
}

LZ4F_FN void lz4f_xxh32_update(lz4f_xxh32_state *s, const uint8_t *p, size_t n) {
  s->total += n;
  if (s->nbuf) {
    size_t take = 16 - s->nbuf;
    if (take > n) take = n;
    memcpy(s->buf + s->nbuf, p, take);
    s->nbuf += (uint32_t)take;
    p += take;
    n -= take;
    if (s->nbuf < 16) return;
    lz4f_stripe(s, s->buf);
    s->nbuf = 0;
  }
  for (; n >= 16; p += 16, n -= 16) lz4f_stripe(s, p);
  if (n) {
    memcpy(s->buf, p, n);
    s->nbuf = (uint32_t)n;
  }
}

LZ4F_FN uint32_t lz4f_xxh32_digest(const lz4f_xxh32_state *s) {
  uint32_t h = s->total >= 16 ? lz4f_rotl(s->v[0], 1) + lz4f_rotl(s->v[1], 7) +
                                    lz4f_rotl(s->v[2], 12) + lz4f_rotl(s->v[3], 18)
                              : s->seed + LZ4F_P5;
  h += (uint32_t)s->total;
  const uint8_t *p = s->buf;
  uint32_t n = s->nbuf;
  for (; n >= 4; p += 4, n -= 4) h = lz4f_rotl(h + lz4f_le32(p) * LZ4F_P3, 17) * LZ4F_P4;
  for (; n; ++p, --n) h = lz4f_rotl(h + *p * LZ4F_P5, 11) * LZ4F_P1;
  h ^= h >> 15;
  h *= LZ4F_P2;
  h ^= h >> 13;
  h *= LZ4F_P3;
  h ^= h >> 16;
  return h;
}

LZ4F_FN uint32_t lz4f_xxh32(const uint8_t *p, size_t n, uint32_t seed) {
  lz4f_xxh32_state s;
  lz4f_xxh32_init(&s, seed);
  lz4f_xxh32_update(&s, p, n);
  return lz4f_xxh32_digest(&s);
}

#endif /* LZ4F_XXH32_H */
