/* CPU check of the kernel routes of a point list batch (realtime_urdf_filter_amd/csrc/rtuf_routes.h, BatchKind::Points), over
 * every combination of route_of's other inputs: u16 x label plane x thresholds x two-kernel flag x dilation 0 / > 0 x cover pass
 * x padding x scene = 256.  tests/routes_check.cpp, link_padding_routes_check.cpp and scene_routes_check.cpp hold the same header
 * for the six older kinds, where nothing may have changed.
 *   1. route_of agrees with kRows below, written out from the API's text (include/rtuf.h, POINT LIST BATCHES): what is
 *      refused.  Every combination falls into exactly one row.
 *   2. every route, refused or not, is tile_render_kernel's plain float variant -- no labels, no thresholds, no 16UC1 -- with
 *      the cover pass as the context has it, nothing between it and Tail::Points, and no scene stage; that variant is legal and
 *      one the launcher names today (a render batch's): the new kind adds no variant of the tile kernel.
 *   3. route_index tells the points routes apart from one another and from every route of the six older kinds, and the enums
 *      were appended to: the older kinds and tails keep their numbers.
 * g++ -O2 -I realtime_urdf_filter_amd/csrc;  prints "ok <combinations> <points routes>" or the first failure. */
#include <stdio.h>

#include <set>

#include "rtuf_routes.h"

using namespace rtuf;

namespace {

enum { No = 0, Yes = 1, Any = -1 };
enum { Refused = 0, Ok = 1 };

// A class of combinations (u16, the two-kernel flag, the cover pass and the scene never decide; Any: either) and what becomes of it.
struct Row {
  int labels, thresh, dilated, padded;
  int ok;
  const char* why;
};
const Row kRows[] = {
  {No, No, No, No,      Ok, "tile_render_kernel, then points_filter_kernel"},
  {Yes, Any, Any, Any,  Refused, "no points call takes a label plane"},
  {No, Yes, Any, Any,   Refused, "per-link thresholds in effect: not supported yet"},
  {No, No, Yes, Any,    Refused, "silhouette_dilation_px > 0: not supported yet (radius_px is the batch's own margin)"},
  {No, No, No, Yes,     Refused, "link padding in effect: not supported yet"},
};

bool matches(int want, bool have) { return want == Any || (want == Yes) == have; }

static_assert((int)BatchKind::Filter == 0 && (int)BatchKind::Bits == 1 && (int)BatchKind::Render == 2 && (int)BatchKind::Residual == 3 &&
              (int)BatchKind::Cloud == 4 && (int)BatchKind::Clearance == 5 && (int)BatchKind::Points == 6, "BatchKind::Points is appended");
static_assert((int)Tail::None == 0 && (int)Tail::Cloud == 1 && (int)Tail::Clearance == 2 && (int)Tail::Points == 3 && kTails == 4, "Tail::Points is appended");

}  // namespace

int main()
{
  const BatchKind older[] = {BatchKind::Filter, BatchKind::Bits, BatchKind::Render, BatchKind::Residual, BatchKind::Cloud, BatchKind::Clearance};
  std::set<int> points_routes, older_routes;
  int combinations = 0;
  for (int m = 0; m < 256; m++) {
    const bool u16 = m & 1, labels = m & 2, thresh = m & 4, two = m & 8, dilated = m & 16, cover = m & 32, padded = m & 64, scene = m & 128;
    for (BatchKind kind : older) {
      const Route o = route_of(RouteFacts{kind, u16, labels, thresh, two, dilated ? 3 : 0, cover, padded, scene});
      if (o.ok) older_routes.insert(route_index(o));
      if (o.tail == Tail::Points) { printf("kind %d takes the points tail\n", (int)kind); return 1; }
    }
    const Route r = route_of(RouteFacts{BatchKind::Points, u16, labels, thresh, two, dilated ? 3 : 0, cover, padded, scene});
    const Row* row = nullptr;
    int hits = 0;
    for (const Row& q : kRows)
      if (matches(q.labels, labels) && matches(q.thresh, thresh) && matches(q.dilated, dilated) && matches(q.padded, padded)) { row = &q; hits++; }
    auto fail = [&](const char* what) {
      printf("u16 %d labels %d thresh %d two_kernel %d dilated %d cover %d padded %d scene %d: %s (%s)\n", u16, labels, thresh, two, dilated, cover, padded,
             scene, what, row ? row->why : "-");
      return 1;
    };
    if (hits != 1) return fail("not in exactly one row of the table");
    if (r.ok != (row->ok == Ok)) return fail(row->ok == Ok ? "refused, but the table admits it" : "admitted, but the table refuses it");
    combinations++;
    if (!tile_variant_legal(r.tile)) return fail("an illegal tile variant");
    if (r.tile.out != TileOut::Render || r.tile.labels || r.tile.thresh || r.tile.u16) return fail("not the plain float render variant");
    if (r.tile.cover != cover) return fail("tile cover");
    if (r.post != Post::None) return fail("post");
    if (r.tail != Tail::Points) return fail("tail");
    if (r.scene) return fail("a scene stage");
    if (!runs_behind_tile(r)) return fail("runs_behind_tile");
    // ... and but for the tail it is the route of a render batch in a context without any of the refused facts
    const Route render = route_of(RouteFacts{BatchKind::Render, false, false, false, two, 0, cover, false, scene});
    if (!render.ok || tile_variant_index(render.tile) != tile_variant_index(r.tile) || render.post != r.post || render.scene != r.scene)
      return fail("not a render batch's tile kernel");
    if (r.ok) points_routes.insert(route_index(r));
  }
  if (points_routes.size() != 2) { printf("%d distinct points route numbers (with and without the cover pass: 2)\n", (int)points_routes.size()); return 1; }
  for (int i : points_routes)
    if (older_routes.count(i)) { printf("route number %d is a points route and a route of an older kind\n", i); return 1; }
  printf("ok %d %d\n", combinations, (int)points_routes.size());
  return 0;
}
