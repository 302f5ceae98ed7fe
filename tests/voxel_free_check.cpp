/* Host check of the voxel free space's per-voxel arithmetic: runs the product's own functions
 * (realtime_urdf_filter_amd/csrc/rtuf_numerics.h: voxel_centre, voxel_inverse_transform, point_transform, point_pixel,
 * voxel_free_test) on cases read from stdin and prints the results, for tests/test_voxel_free_cpu.py to hold against
 * bench_support/voxel_free_check.py.
 * Input: a count, then per case "moved ix iy iz W H" in decimal and, as hexadecimal words, the bit patterns of the grid's
 * origin (3) and (float)voxel_size, the 12 used entries of world_from_optical as floats (column-major order, the last row left
 * out; read but unused when moved = 0), fx, fy, cx, cy, Emin and the margin.
 * Output per case: "<invertible> <judged> <u> <v> <free>" in decimal, then as hexadecimal words the centre (3), the centre in
 * the optical frame (3) and the 12 used entries of the inverse (zeros when moved = 0 or the matrix cannot be inverted: the
 * case then ends there, judged = free = 0).
 * Plain g++ -O2 -ffp-contract=off, no ROCm headers. */
#include <cstdio>
#include <cstdlib>

#include "rtuf_numerics.h"

int main()
{
  unsigned long n = 0;
  if (scanf("%lu", &n) != 1) return 1;
  for (unsigned long i = 0; i < n; i++) {
    int moved, idx[3], W, H;
    unsigned g[4], t[12], k[4], e[2];
    if (scanf("%d %d %d %d %d %d", &moved, &idx[0], &idx[1], &idx[2], &W, &H) != 6) return 1;
    for (unsigned& q : g) if (scanf("%x", &q) != 1) return 1;
    for (unsigned& q : t) if (scanf("%x", &q) != 1) return 1;
    for (unsigned& q : k) if (scanf("%x", &q) != 1) return 1;
    for (unsigned& q : e) if (scanf("%x", &q) != 1) return 1;
    const float size = rtuf::__uint_as_float(g[3]);
    float c[3];
    for (int r = 0; r < 3; r++) c[r] = rtuf::voxel_centre(idx[r], rtuf::__uint_as_float(g[r]), size);
    float m[16] = {}, inv[16] = {};
    for (int col = 0; col < 4; col++) for (int r = 0; r < 3; r++) m[4 * col + r] = rtuf::__uint_as_float(t[3 * col + r]);
    const bool ok = !moved || rtuf::voxel_inverse_transform(m, inv);
    float x = c[0], y = c[1], z = c[2];
    int u = 0, v = 0;
    bool judged = false, is_free = false;
    if (ok) {
      if (moved) rtuf::point_transform(inv, x, y, z);
      const rtuf::PointIntrinsics intr = {rtuf::__uint_as_float(k[0]), rtuf::__uint_as_float(k[1]), rtuf::__uint_as_float(k[2]), rtuf::__uint_as_float(k[3])};
      judged = rtuf::point_pixel(x, y, z, intr, W, H, u, v);
      is_free = judged && rtuf::voxel_free_test(z, rtuf::__uint_as_float(e[0]), rtuf::__uint_as_float(e[1]));
    }
    printf("%d %d %d %d %d", ok ? 1 : 0, judged ? 1 : 0, u, v, is_free ? 1 : 0);
    for (int r = 0; r < 3; r++) printf(" %x", rtuf::__float_as_uint(c[r]));
    printf(" %x %x %x", rtuf::__float_as_uint(x), rtuf::__float_as_uint(y), rtuf::__float_as_uint(z));
    for (int col = 0; col < 4; col++) for (int r = 0; r < 3; r++) printf(" %x", rtuf::__float_as_uint(inv[4 * col + r]));
    printf("\n");
  }
  return 0;
}
