// CPU check of link padding's arithmetic (tests/test_link_padding_cpu.py): link_padding_reach2 of rtuf_numerics.h -- the text the
// kernel compiles -- over a sweep of (z, pad, f), printed as bit patterns for the numpy mirror (bench_support/link_padding_check.py)
// to repeat.  Plain g++, no ROCm headers.  The sweep: window depths from the near plane to the far plane, three focal lengths,
// and for each pair paddings aimed at rho^2 = k for k = 1 .. 256 and a few ulps to either side (rho just below 1, rho^2 within
// an ulp of an integer, the clamp at 16 pixels and beyond it), besides 0, a denormal and a huge one.
//
// output: "consts <num bits> <off bits>", then one line "<z bits> <pad bits> <f bits> <R2>" per case, then "done <cases>"
#include <cstdio>
#include <initializer_list>

#include "rtuf_numerics.h"

using namespace rtuf;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main()
{
  const float z_near = 0.1f, z_far = 8.0f;
  const float num = shade_num(z_near, z_far), off = shade_off(z_near, z_far);
  printf("consts %08x %08x\n", bits(num), bits(off));
  const float zs[] = {0.0f, 3e-5f, 0.25f, 0.5f, 0.7594937f, 0.9f, 0.95f, 0.987f, 0.9999f, 1.0f, NAN};
  const float fs[] = {131.25f, 525.0f, 1050.5f};
  long cases = 0;
  auto emit = [&](float z, float pad, float f) {
    printf("%08x %08x %08x %u\n", bits(z), bits(pad), bits(f), link_padding_reach2(z, pad, f, num, off));
    cases++;
  };
  for (float z : zs)
    for (float f : fs) {
      const float d = num / (z - off);
      for (float pad : {0.0f, -0.0f, 1e-42f, 1e-3f, 0.02f, 0.05f, 1.0f, 3e38f}) emit(z, pad, f);
      for (int k = 1; k <= 260; k++) {
        float pad = sqrtf((float)k) * d / f;                    // rho^2 is about k
        if (!(pad == pad)) pad = 0.01f * (float)k;              // (z NaN: any padding, the result is 0)
        float lo = pad, hi = pad;
        emit(z, pad, f);
        for (int u = 0; u < 3; u++) {
          lo = nextafterf(lo, 0.0f);
          hi = nextafterf(hi, INFINITY);
          emit(z, lo, f);
          emit(z, hi, f);
        }
      }
    }
  printf("done %ld\n", cases);
  return 0;
}
