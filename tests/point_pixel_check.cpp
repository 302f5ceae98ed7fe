/* Host check of the point list batches' per-point arithmetic: runs the product's own functions
 * (realtime_urdf_filter_amd/csrc/rtuf_numerics.h: point_transform, point_pixel, point_verdict) on cases read from stdin and
 * prints the results, for tests/test_point_lists_cpu.py to hold against bench_support/points_check.py.
 * Input: a count, then per case "W H moved" in decimal and, as hexadecimal words, the bit patterns of x, y, z, fx, fy, cx, cy,
 * vmin, t and the 12 used entries of the transform (column-major order, the last row left out; read but unused when moved = 0).
 * Output per case: "<judged> <u> <v> <verdict> <x'> <y'> <z'>", the point as hexadecimal words; verdict 2 when not judged.
 * Plain g++ -ffp-contract=off, no ROCm headers; also built with -fsanitize=address,undefined,float-cast-overflow (no
 * out-of-range float may ever be converted). */
#include <cstdio>
#include <cstdlib>

#include "rtuf_numerics.h"

int main()
{
  unsigned long n = 0;
  if (scanf("%lu", &n) != 1) return 1;
  for (unsigned long i = 0; i < n; i++) {
    int W, H, moved;
    unsigned w[9], t[12];
    if (scanf("%d %d %d", &W, &H, &moved) != 3) return 1;
    for (unsigned& q : w) if (scanf("%x", &q) != 1) return 1;
    for (unsigned& q : t) if (scanf("%x", &q) != 1) return 1;
    float x = rtuf::__uint_as_float(w[0]), y = rtuf::__uint_as_float(w[1]), z = rtuf::__uint_as_float(w[2]);
    const rtuf::PointIntrinsics k = {rtuf::__uint_as_float(w[3]), rtuf::__uint_as_float(w[4]), rtuf::__uint_as_float(w[5]), rtuf::__uint_as_float(w[6])};
    float m[16] = {};
    for (int c = 0; c < 4; c++) for (int r = 0; r < 3; r++) m[4 * c + r] = rtuf::__uint_as_float(t[3 * c + r]);
    if (moved) rtuf::point_transform(m, x, y, z);
    int u = 0, v = 0;
    const bool judged = rtuf::point_pixel(x, y, z, k, W, H, u, v);
    const unsigned verdict = judged ? rtuf::point_verdict(z, rtuf::__uint_as_float(w[7]), rtuf::__uint_as_float(w[8])) : (unsigned)rtuf::kPointOutside;
    printf("%d %d %d %u %x %x %x\n", judged ? 1 : 0, u, v, verdict, rtuf::__float_as_uint(x), rtuf::__float_as_uint(y), rtuf::__float_as_uint(z));
  }
  return 0;
}
