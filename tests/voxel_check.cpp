/* Host check of the voxel occupancy grids' per-point arithmetic: runs the product's own functions
 * (realtime_urdf_filter_amd/csrc/rtuf_numerics.h: point_transform, voxel_of) on cases read from stdin and prints the results,
 * for tests/test_voxel_grids_cpu.py to hold against bench_support/voxel_check.py.
 * Input: a count, then per case "moved nx ny nz" in decimal and, as hexadecimal words, the bit patterns of x, y, z, the grid's
 * origin (3) and inv, and the 12 used entries of the transform (column-major order, the last row left out; read but unused
 * when moved = 0).
 * Output per case: "<in> <index> <x'> <y'> <z'>", the index in decimal (-1 when the point is not in the grid), the world point
 * as hexadecimal words.
 * Plain g++ -O2 -ffp-contract=off, no ROCm headers. */
#include <cstdio>
#include <cstdlib>

#include "rtuf_numerics.h"

int main()
{
  unsigned long n = 0;
  if (scanf("%lu", &n) != 1) return 1;
  for (unsigned long i = 0; i < n; i++) {
    int moved;
    rtuf::VoxelGrid g{};
    unsigned w[7], t[12];
    if (scanf("%d %d %d %d", &moved, &g.nx, &g.ny, &g.nz) != 4) return 1;
    for (unsigned& q : w) if (scanf("%x", &q) != 1) return 1;
    for (unsigned& q : t) if (scanf("%x", &q) != 1) return 1;
    float x = rtuf::__uint_as_float(w[0]), y = rtuf::__uint_as_float(w[1]), z = rtuf::__uint_as_float(w[2]);
    g.ox = rtuf::__uint_as_float(w[3]); g.oy = rtuf::__uint_as_float(w[4]); g.oz = rtuf::__uint_as_float(w[5]); g.inv = rtuf::__uint_as_float(w[6]);
    float m[16] = {};
    for (int c = 0; c < 4; c++) for (int r = 0; r < 3; r++) m[4 * c + r] = rtuf::__uint_as_float(t[3 * c + r]);
    if (moved) rtuf::point_transform(m, x, y, z);
    uint32_t index = 0;
    const bool in = rtuf::voxel_of(x, y, z, g, index);
    if (in != (index != rtuf::kVoxelNone)) return 2;
    printf("%d %ld %x %x %x\n", in ? 1 : 0, in ? (long)index : -1L, rtuf::__float_as_uint(x), rtuf::__float_as_uint(y), rtuf::__float_as_uint(z));
  }
  return 0;
}
