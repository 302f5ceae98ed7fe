/* Host check of the filtered point clouds' per-pixel arithmetic: runs the product's own functions
 * (realtime_urdf_filter_amd/csrc/rtuf_numerics.h: cloud_sensor_valid, cloud_point) on cases read from stdin and prints the
 * bit patterns, for tests/test_point_clouds_cpu.py to hold against bench_support/cloud_check.py.
 * Input: a count, then per case "u v" in decimal and the bit patterns of s, kx, ky, cx, cy as hexadecimal words.
 * Output per case: "<valid> <x> <y> <z>", the last three as hexadecimal words.  Plain g++ -ffp-contract=off, no ROCm headers. */
#include <cstdio>
#include <cstdlib>

#include "rtuf_numerics.h"

int main()
{
  unsigned long n = 0;
  if (scanf("%lu", &n) != 1) return 1;
  for (unsigned long i = 0; i < n; i++) {
    int u, v;
    unsigned s, kx, ky, cx, cy;
    if (scanf("%d %d %x %x %x %x %x", &u, &v, &s, &kx, &ky, &cx, &cy) != 7) return 1;
    const rtuf::CloudIntrinsics k = {rtuf::__uint_as_float(kx), rtuf::__uint_as_float(ky), rtuf::__uint_as_float(cx), rtuf::__uint_as_float(cy)};
    float x, y, z;
    rtuf::cloud_point(u, v, rtuf::__uint_as_float(s), k, x, y, z);
    printf("%d %x %x %x\n", rtuf::cloud_sensor_valid(rtuf::__uint_as_float(s)) ? 1 : 0, rtuf::__float_as_uint(x), rtuf::__float_as_uint(y), rtuf::__float_as_uint(z));
  }
  return 0;
}
