/*
 * bare_layout.cpp -- TEST INFRASTRUCTURE ONLY: the bare-stream decoder's
 * scratch layout (csrc/lz4r_dec_layout.h, plain host C++) against the layout
 * written out here independently.  Linked into build/sanitize_main and
 * called from sanitize_main.c; prints "bare scratch layout ok (<n> cases)".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../lz4-jpeg_amd/csrc/lz4r_dec_layout.h"

static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

extern "C" int bare_layout_case(void) {
  static const size_t kChunks[] = {1, 2, 3, 63, 64, 65, 1023, 1025, 131072};
  static const size_t kCaps[] = {0, 1, 5, 3579140};
  int fails = 0, cases = 0;
  for (size_t nchunks : kChunks) {
    for (size_t nb_cap : kCaps) {
      const size_t ng = (nchunks + 63) / 64;
      const size_t o_gsum = 16 * nchunks;
      const size_t o_small = o_gsum + 16 * ng;
      const size_t o_mis = o_small + 64;
      const size_t o_cnt = o_mis + 4 * (size_t)kMisCap;
      const size_t o_lok = al16(o_cnt + 4 * nchunks);
      const size_t o_lst = al16(o_lok + 4 * nchunks);
      const size_t o_boff = al16(o_lst + 2 * (size_t)kList * nchunks);
      const size_t bytes = o_boff + 8 * nb_cap;
      BareScratch S = bare_scratch_layout(nchunks, nb_cap);
      bool ok = S.nchunks == nchunks && S.ng == ng && S.o_gsum == o_gsum && S.o_ctl == o_small &&
                S.o_mis == o_mis && S.o_cnt == o_cnt && S.o_lok == o_lok && S.o_lists == o_lst &&
                S.o_boff == o_boff && S.bytes == bytes;
      /* the bound pointers, as offsets from the base of an allocation of the total */
      uint8_t *base = (uint8_t *)malloc(S.bytes);
      S.bind(base);
      auto off = [base](const void *p) { return (size_t)((const uint8_t *)p - base); };
      ok = ok && base && off(S.cand) == 0 && off(S.exitp) == 8 * nchunks &&
           off(S.gsum) == o_gsum && off(S.gbase) == o_gsum + 8 * ng && off(S.ctl) == o_small &&
           off(S.nmis) == o_small + 40 && off(S.mis) == o_mis && off(S.cnt) == o_cnt &&
           off(S.lok) == o_lok && off(S.lists) == o_lst && off(S.boff) == o_boff;
      /* lz4_bare_walk stores the lists as uint4; the u64 and u32 regions aligned as such */
      ok = ok && off(S.lists) % 16 == 0 && off(S.ctl) % 8 == 0 && off(S.boff) % 8 == 0 &&
           off(S.gsum) % 8 == 0 && off(S.mis) % 4 == 0 && off(S.cnt) % 4 == 0 &&
           off(S.lok) % 4 == 0;
      /* no two regions overlap, and the last ends at the total */
      const size_t reg[][2] = {
          {off(S.cand), 8 * nchunks}, {off(S.exitp), 8 * nchunks}, {off(S.gsum), 8 * ng},
          {off(S.gbase), 8 * ng}, {off(S.ctl), 8 * (size_t)kCtlNmis + 4},
          {off(S.mis), 4 * (size_t)kMisCap}, {off(S.cnt), 4 * nchunks}, {off(S.lok), 4 * nchunks},
          {off(S.lists), 2 * (size_t)kList * nchunks}, {off(S.boff), 8 * nb_cap}};
      const size_t nreg = sizeof reg / sizeof reg[0];
      for (size_t i = 0; i < nreg; ++i)
        ok = ok && reg[i][0] + reg[i][1] <= (i + 1 < nreg ? reg[i + 1][0] : S.bytes);
      free(base);
      if (!ok) {
        fprintf(stderr, "FAIL bare scratch layout: nchunks %zu nb_cap %zu\n", nchunks, nb_cap);
        ++fails;
      }
      ++cases;
    }
  }
  if (!fails) printf("bare scratch layout ok (%d cases)\n", cases);
  return fails;
}
