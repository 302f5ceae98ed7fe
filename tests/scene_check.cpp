/* CPU check of the scene planes' arithmetic (realtime_urdf_filter_amd/csrc/rtuf_numerics.h: scene_threshold, scene_filtered,
 * scene_learned), compiled for the host with plain g++ -- no ROCm headers -- and held against a numpy float32 form bit for bit by
 * tests/test_scene_planes_cpu.py.  Prints, for a grid of scene values (0, denormals, +inf, NaN among them), margins (rel = 0,
 * abs_m = 0, a rel close to 1) and sensor values around every threshold, one line per case:
 *   <scene> <abs_m> <rel> <sensor> <thr> <filtered> <learned, robot keeps> <learned, robot filters>      (floats as hex words)
 * and "done <cases>".  g++ -O2 -ffp-contract=off -I realtime_urdf_filter_amd/csrc. */
#include <stdio.h>

#include <vector>

#include "rtuf_numerics.h"

using namespace rtuf;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main()
{
  std::vector<float> scenes = {0.0f, -0.0f, from_bits(1u), from_bits(0x007fffffu), 1e-30f, 0.001f, 0.5f, 0.999f, 1.0f, 1.7f, 2.0f, 3.1415927f, 7.9f,
                               65.535f, 1e10f, 3.4e38f, -1.0f, INFINITY, -INFINITY, NAN, from_bits(0x7fc00001u)};
  for (uint32_t i = 0; i < 200; i++) scenes.push_back(0.3f + 0.0371f * (float)i);
  const float abs_ms[] = {0.0f, from_bits(1u), 1e-6f, 0.01f, 0.02f, 0.05f, 0.5f, 3.0f};
  const float rels[] = {0.0f, from_bits(1u), 0.005f, 0.01f, 0.1f, 0.5f, 0.9f, from_bits(0x3f7fffffu) /* the float below 1 */};
  long cases = 0;
  for (float sc : scenes)
    for (float a : abs_ms)
      for (float r : rels) {
        const float thr = scene_threshold(sc, a, r);
        // around the threshold, the scene value itself, and the sensor values that hold no reading
        const float sensors[] = {thr, nextafterf(thr, INFINITY), nextafterf(thr, -INFINITY), sc, 0.0f, -0.0f, -1.0f, 1.0f, from_bits(1u), INFINITY, -INFINITY, NAN};
        for (float s : sensors) {
          printf("%08x %08x %08x %08x %08x %d %08x %08x\n", bits(sc), bits(a), bits(r), bits(s), bits(thr), scene_filtered(s, sc, a, r) ? 1 : 0,
                 bits(scene_learned(sc, s, false)), bits(scene_learned(sc, s, true)));
          cases++;
        }
      }
  printf("done %ld\n", cases);
  return 0;
}
