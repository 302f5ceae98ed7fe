// Host build of the link clearance arithmetic of rtuf_numerics.h (clearance_centre, clearance_point_sphere) for
// tests/test_link_clearance_cpu.py: compiled with g++ -O2 -ffp-contract=off, no ROCm headers.
// stdin: a count, then per line 'c' + 48 doubles (link_tf, cam_tf, offset_inv as hex bit patterns) + 3 floats (centre), or
// 'p' + 7 floats (point, centre, radius).  stdout: per line the result's float bit patterns in hex (3 resp. 1).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "rtuf_numerics.h"

static float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main()
{
  long n = 0;
  if (scanf("%ld", &n) != 1) return 2;
  for (long i = 0; i < n; i++) {
    char kind = 0;
    if (scanf(" %c", &kind) != 1) return 2;
    if (kind == 'c') {
      double m[48];
      for (double& d : m) { uint64_t u; if (scanf("%" SCNx64, &u) != 1) return 2; memcpy(&d, &u, 8); }
      float c[3], out[3];
      for (float& f : c) { uint32_t u; if (scanf("%x", &u) != 1) return 2; f = f_of(u); }
      rtuf::clearance_centre(m, m + 16, m + 32, c, out);
      printf("%x %x %x\n", u_of(out[0]), u_of(out[1]), u_of(out[2]));
    } else {
      float v[7];
      for (float& f : v) { uint32_t u; if (scanf("%x", &u) != 1) return 2; f = f_of(u); }
      printf("%x\n", u_of(rtuf::clearance_point_sphere(v[0], v[1], v[2], v[3], v[4], v[5], v[6])));
    }
  }
  return 0;
}
