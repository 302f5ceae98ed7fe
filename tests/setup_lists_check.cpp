// CPU check of the set-up kernel's packed list counters (rtuf_numerics.h: list_counts and its three fields) against the three
// separate counters they stand for.  Plain g++, no ROCm headers.  Prints "ok <cases>" or the first failure.
#include <stdio.h>

#include "rtuf_numerics.h"

using namespace rtuf;

int main()
{
  unsigned long long cases = 0;
  // three lists that hold at most 768 entries together: every split of 768 into three fields reads back
  for (uint32_t nrec = 0; nrec <= 768; nrec++) {
    for (uint32_t ntiny = 0; nrec + ntiny <= 768; ntiny++, cases++) {
      const uint32_t nsmall = 768 - nrec - ntiny;
      const uint32_t w = list_counts(nrec, ntiny, nsmall);
      if (list_count_rec(w) != nrec || list_count_tiny(w) != ntiny || list_count_small(w) != nsmall) {
        printf("list_counts(%u, %u, %u) reads back (%u, %u, %u)\n", nrec, ntiny, nsmall, list_count_rec(w), list_count_tiny(w), list_count_small(w));
        return 1;
      }
    }
  }
  // built up by additions as the kernel's waves make them (one addition per wave and stream: 64 triangles over the three
  // fields): what the addition returns holds the three bases, and the sum the three totals
  for (uint32_t seed = 1; seed <= 1000; seed++) {
    uint32_t w = 0, r = 0, t = 0, s = 0, x = seed * 2654435761u;
    for (int wave = 0; wave < 12; wave++, cases++) {          // 12 waves of 64 triangles = 3 streams of 256
      x = x * 1664525u + 1013904223u;
      const uint32_t a = (x >> 8) % 65u, b = (x >> 16) % (65u - a), c = seed % 3u ? 64u - a - b : (x >> 24) % (65u - a - b);
      const uint32_t base = w;
      w += list_counts(a, b, c);
      if (list_count_rec(base) != r || list_count_tiny(base) != t || list_count_small(base) != s) { printf("seed %u wave %d: bases\n", seed, wave); return 1; }
      r += a; t += b; s += c;
    }
    if (r + t + s > 768u || list_count_rec(w) != r || list_count_tiny(w) != t || list_count_small(w) != s) { printf("seed %u: totals\n", seed); return 1; }
  }
  // a field at 768 (every triangle of three streams in ONE list) leaves its neighbours alone, and the hand-over of every
  // fragment-sized box to the records ("+ 1": the record field is the lowest) moves the record field only, up to 768
  {
    const uint32_t full[3] = {list_counts(768, 0, 0), list_counts(0, 768, 0), list_counts(0, 0, 768)};
    if (list_count_rec(full[0]) != 768 || list_count_tiny(full[0]) != 0 || list_count_small(full[0]) != 0) { printf("768 records\n"); return 1; }
    if (list_count_rec(full[1]) != 0 || list_count_tiny(full[1]) != 768 || list_count_small(full[1]) != 0) { printf("768 tiny\n"); return 1; }
    if (list_count_rec(full[2]) != 0 || list_count_tiny(full[2]) != 0 || list_count_small(full[2]) != 768) { printf("768 small\n"); return 1; }
    for (int which = 1; which < 3; which++) {
      uint32_t w = full[which];
      for (uint32_t i = 0; i < 768; i++, cases++) {
        if (list_count_rec(w) != i) { printf("hand-over %u lands at %u\n", i, list_count_rec(w)); return 1; }
        w += 1u;
      }
      if (list_count_rec(w) != 768 || w - 768u != full[which]) { printf("hand-over: fields\n"); return 1; }
    }
  }
  printf("ok %llu\n", cases);
  return 0;
}
