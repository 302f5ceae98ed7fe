/* Exhaustive CPU check of the tile kernel's depth-key encoding (KeyFmt, rtuf_kernels.hip), with the product's own functions
 * (realtime_urdf_filter_amd/csrc/rtuf_numerics.h): for every key shift key_shift_for can return and every float window z whose
 * 24-bit depth z24 = z24_of(z) lies in [exact_z_floor(shift), 2^23], near_z_from_key must give back the float itself from z24
 * and the float's low `shift` bits.
 * g++ -O2 -ffp-contract=off -I realtime_urdf_filter_amd/csrc;  prints "ok <floats checked>" or the first failure. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "rtuf_numerics.h"

using namespace rtuf;

static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main(void)
{
  /* the rule is monotone in the triangle count and changes only where the count reaches a power of two: those counts give
   * every shift it returns for any 32-bit count (the library refuses 2^29 - 1 and more; the shifts below 3 it would give
   * beyond have an empty range, 2^(26 - shift) > 2^23) */
  bool seen[33] = {false};
  for (int b = 0; b < 32; b++) seen[key_shift_for(1u << b)] = true;
  int s_lo = 32, s_hi = 0;
  for (int s = 0; s <= 32; s++)
    if (seen[s]) { s_lo = s < s_lo ? s : s_lo; s_hi = s; }
  unsigned long long checked = 0;
  /* every float from the smallest z24 any shift covers up to the first float whose z24 exceeds 2^23 */
  uint32_t first = f2u(((float)exact_z_floor(s_hi) - 1.0f) / 16777215.0f);
  for (uint32_t u = first; ; u++) {
    const float z = u2f(u);
    const uint32_t z24 = z24_of(z);
    if (z24 > (1u << 23)) break;
    for (int s = s_lo; s <= s_hi; s++) {
      if (!seen[s] || z24 < exact_z_floor(s)) continue;
      const float back = near_z_from_key(z24, u & ((1u << s) - 1u), s);
      if (f2u(back) != u) { printf("FAIL shift %d z %.9g (0x%08x) z24 %u -> 0x%08x\n", s, z, u, z24, f2u(back)); return 1; }
      checked++;
    }
  }
  int n_shifts = 0;
  for (int s = 0; s <= 32; s++) n_shifts += seen[s];
  printf("ok %llu (%d shifts, %d .. %d)\n", checked, n_shifts, s_lo, s_hi);
  return 0;
}
