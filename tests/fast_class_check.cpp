/* CPU check of the bit-pattern identities the tile kernel uses in place of 4-cycle-class instructions (DESIGN.md section 4,
 * docs/experiments.md R6.7).  It runs the product's own functions (realtime_urdf_filter_amd/csrc/rtuf_numerics.h) against
 * reference forms kept here -- the forms the kernels used up to round 5:
 *   1. z24_of_upper_half(z) == z24_of(z) == rintf(clamp(z) * 16777215)   for EVERY float z > 0.5 (incl. > 1, +inf); the kernels
 *                                                                          use it for z >= 0.51
 *   2. z_of_upper_half_z24(z24) == (float)(z24 + 1) * 2^-24               for every 24-bit depth >= 2^23 - 1
 *   3. edge_constant == the low 32 bits of the 64-bit edge constant, and inclusive_edge_bias == its comparison form
 *                                                                          for 120 M vertex pairs (random, near-coincident, axis-aligned)
 *   4. the walk's "right-hand pixel is outside the box" == wrap && odd width    for every box width 1..64
 * g++ -O2 -ffp-contract=off -I realtime_urdf_filter_amd/csrc; prints "ok <cases>" or the first counter-example. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "rtuf_numerics.h"

using namespace rtuf;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float flt(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static uint32_t z24_reference(float z)
{
  const float zc = fminf(fmaxf(z, 0.0f), 1.0f);
  return (uint32_t)(int32_t)rintf(zc * 16777215.0f);
}

int main(void)
{
  unsigned long long cases = 0;
  /* 1 */
  for (uint32_t u = 0x3F000001u; u <= 0x7F800000u; u++) {      /* (0.5 itself: p = 8388607.5 is below 2^23, a tie the pattern does not round) */
    const float z = flt(u);
    const uint32_t ref = z24_reference(z);
    if (z24_of_upper_half(z) != ref || z24_of(z) != ref) {
      printf("z24: z bits %08x: upper half %u, z24_of %u, reference %u\n", u, z24_of_upper_half(z), z24_of(z), ref);
      return 1;
    }
    cases++;
  }
  /* 2 */
  for (uint32_t k = 8388607u; k <= 16777215u; k++) {
    const float ref = (float)(k + 1u) * 5.9604644775390625e-08f;
    if (bits(z_of_upper_half_z24(k)) != bits(ref)) { printf("z from key: %u\n", k); return 1; }
    cases++;
  }
  /* 3 */
  uint64_t s = 88172645463325252ull;
  for (long it = 0; it < 120000000L; it++) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const uint64_t t = s * 0x9E3779B97F4A7C15ull;
    const int mode = (int)((s >> 60) & 7);
    int xi = (int)(s & 0xfffff) - 1024, yi = (int)((s >> 20) & 0xfffff) - 1024, xj, yj;
    if (mode == 0) { xj = (int)(t & 0xfffff) - 1024; yj = (int)((t >> 20) & 0xfffff) - 1024; }
    else {
      const int r = mode == 1 ? 2047 : (mode == 2 ? 255 : (mode == 3 ? 31 : 3));
      xj = xi + (mode == 5 ? 0 : (int)(t & (uint64_t)(2 * r + 1)) - r); yj = yi + (mode == 6 ? 0 : (int)((t >> 24) & (uint64_t)(2 * r + 1)) - r);
      if (xj < -1024) xj = -1024;
      if (yj < -1024) yj = -1024;
      if (xj > 1047551) xj = 1047551;
      if (yj > 1047551) yj = 1047551;
    }
    const int dcdx = yi - yj, dcdy = xi - xj;
    /* reference: the 64-bit constant, inclusive on low-x / low-row edges; inside <=> ceil(c / 256) - dcdx px + dcdy py > 0 */
    long long c = (long long)dcdx * xi - (long long)dcdy * yi;
    const int bias_cmp = (dcdx < 0 || (dcdx == 0 && dcdy > 0)) ? 1 : 0;
    c += bias_cmp;
    const int C64 = (int)(-((-c) >> 8));
    const uint32_t bias = inclusive_edge_bias(dcdx, dcdy);
    const int C32 = edge_constant(dcdx, dcdy, xi, yi);
    if ((int)bias != bias_cmp || C64 != C32) { printf("edge: %d %d %d %d: %d vs %d, bias %u vs %d\n", xi, yi, xj, yj, C64, C32, bias, bias_cmp); return 1; }
    cases++;
  }
  /* 4 (the lane-per-triangle walk of rtuf_kernels.hip: quads of a box lx0..lx1, `back` = x distance of the last quad) */
  for (int w = 1; w <= 64; w++) {
    const int lx0 = 0, lx1 = w - 1, qcols = (lx1 - lx0 + 2) >> 1, back = 2 * (qcols - 1), odd_w = ((lx1 - lx0) & 1) == 0;
    for (int px = lx0; px <= lx0 + back; px += 2) {
      const int right_old = px < lx1, wrap = px == lx0 + back;
      if (right_old != !(wrap && odd_w)) { printf("right: w %d px %d\n", w, px); return 1; }
      cases++;
    }
  }
  printf("ok %llu\n", cases);
  return 0;
}
