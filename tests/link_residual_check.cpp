/* Host check of the link residual tables' per-pixel arithmetic: runs the product's own functions
 * (realtime_urdf_filter_amd/csrc/rtuf_numerics.h: link_residual_class, link_residual_undrawn) on triples read from stdin and
 * prints class bits and q, for tests/test_link_residuals_cpu.py to hold against bench_support/residuals_check.py.
 * Input: a count, then per triple the bit patterns of s, v, t as hexadecimal words.  Output per triple: "<class> <q> <undrawn>".
 * Plain g++ -ffp-contract=off, no ROCm headers. */
#include <cstdio>
#include <cstdlib>

#include "rtuf_numerics.h"

int main()
{
  unsigned long n = 0;
  if (scanf("%lu", &n) != 1) return 1;
  for (unsigned long i = 0; i < n; i++) {
    unsigned s, v, t;
    if (scanf("%x %x %x", &s, &v, &t) != 3) return 1;
    int q = 0;
    const uint32_t c = rtuf::link_residual_class(rtuf::__uint_as_float(s), rtuf::__uint_as_float(v), rtuf::__uint_as_float(t), q);
    printf("%u %d %u\n", c, q, rtuf::link_residual_undrawn(rtuf::__uint_as_float(s)));
  }
  return 0;
}
