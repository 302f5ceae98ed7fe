/* CPU check of the kernel routes with scene planes in effect (realtime_urdf_filter_amd/csrc/rtuf_routes.h, RouteFacts::scene =
 * true), over every combination of route_of's other inputs: 6 kinds x u16 x label plane x thresholds x two-kernel flag x dilation
 * 0 / > 0 x cover pass x link padding = 768.  tests/routes_check.cpp and tests/link_padding_routes_check.cpp hold the same header
 * with scene = false (their brace lists leave it so), where nothing may have changed.
 *   1. the route with scene = true equals the one with scene = false but for the scene stage: tile variant, post, tail, ok;
 *   2. the stage is set exactly for Filter / Bits / Cloud / Clearance batches, never for Render and Residual -- and never
 *      without the fact;
 *   3. a route with the stage runs something behind the tile kernel;
 *   4. route_index separates all of them: routes that differ in anything differ in their number, so every scene route's number
 *      is one no route without a scene has, and the numbers of the routes that existed before stay distinct from each other.
 * g++ -O2 -I realtime_urdf_filter_amd/csrc;  prints "ok <combinations> <scene routes> <plain routes>" or the first failure. */
#include <stdio.h>

#include <map>
#include <tuple>

#include "rtuf_routes.h"

using namespace rtuf;

namespace {

using Key = std::tuple<int, bool, bool, bool, bool, int, int, bool>;
Key key_of(const Route& r)
{
  return Key{(int)r.tile.out, r.tile.labels, r.tile.thresh, r.tile.u16, r.tile.cover, (int)r.post, (int)r.tail, r.scene};
}

}  // namespace

int main()
{
  const BatchKind kinds[] = {BatchKind::Filter, BatchKind::Bits, BatchKind::Render, BatchKind::Residual, BatchKind::Cloud, BatchKind::Clearance};
  std::map<int, Key> by_index;
  int combinations = 0, scene_routes = 0, plain_routes = 0;
  for (BatchKind kind : kinds)
    for (int m = 0; m < 128; m++) {
      const bool u16 = m & 1, labels = m & 2, thresh = m & 4, two = m & 8, dilated = m & 16, cover = m & 32, padded = m & 64;
      const Route plain = route_of(RouteFacts{kind, u16, labels, thresh, two, dilated ? 3 : 0, cover, padded, false});
      const Route with = route_of(RouteFacts{kind, u16, labels, thresh, two, dilated ? 3 : 0, cover, padded, true});
      auto fail = [&](const char* what) {
        printf("kind %d u16 %d labels %d thresh %d two_kernel %d dilated %d cover %d padded %d: %s\n", (int)kind, u16, labels, thresh, two, dilated, cover, padded, what);
        return 1;
      };
      combinations++;
      if (plain.scene) return fail("the scene stage without the fact");
      if (tile_variant_index(with.tile) != tile_variant_index(plain.tile) || with.tile.out != plain.tile.out) return fail("the tile variant changed");
      if (with.post != plain.post) return fail("post changed");
      if (with.tail != plain.tail) return fail("tail changed");
      if (with.ok != plain.ok) return fail("ok changed: a scene refuses nothing and admits nothing");
      const bool wants = kind == BatchKind::Filter || kind == BatchKind::Bits || kind == BatchKind::Cloud || kind == BatchKind::Clearance;
      if (with.scene != wants) return fail(wants ? "no scene stage" : "a scene stage on a render or residual batch");
      if (with.scene && !runs_behind_tile(with)) return fail("runs_behind_tile");
      if (with.scene && route_index(with) == route_index(plain)) return fail("route_index does not tell the scene route from the plain one");
      for (const Route& r : {plain, with}) {
        if (!r.ok) continue;
        const int i = route_index(r);
        const Key k = key_of(r);
        auto it = by_index.find(i);
        if (it == by_index.end()) { by_index.emplace(i, k); (r.scene ? scene_routes : plain_routes)++; }
        else if (it->second != k) return fail("two different routes share a route_index");
      }
    }
  // (every ok route that takes the stage has a plain twin: as many scene routes as plain routes of the four kinds -- all plain
  // routes but the render and residual ones, which the count below leaves out by construction)
  if (scene_routes == 0 || scene_routes >= plain_routes) { printf("%d scene routes, %d plain routes\n", scene_routes, plain_routes); return 1; }
  printf("ok %d %d %d\n", combinations, scene_routes, plain_routes);
  return 0;
}
