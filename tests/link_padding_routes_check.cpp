/* CPU check of the kernel routes with link padding in effect (realtime_urdf_filter_amd/csrc/rtuf_routes.h, RouteFacts::padded =
 * true), over every combination of route_of's other inputs: 6 kinds x u16 x label plane x thresholds x two-kernel flag x dilation
 * 0 / > 0 x cover pass = 384.  tests/routes_check.cpp holds the same header with padded = false, where nothing may have changed.
 *   1. route_of agrees with kRows below, written out from the API's text (include/rtuf.h, LINK PADDING): which batches honour
 *      padding and what is refused.  Every combination falls into exactly one row.
 *   2. every route that is ok is the z-surface variant WITH the label plane (it carries the link slots), neither thresholds nor
 *      16UC1 in the tile kernel, Post::Pad behind it and the kind's usual tail; that variant is legal, and it is one the
 *      launcher names today (tile_labels_kernel<true, false>): padding adds no variant of the tile kernel.
 *   3. route_index tells the padded routes apart from one another and from every route without padding.
 * g++ -O2 -I realtime_urdf_filter_amd/csrc;  prints "ok <combinations> <padded routes>" or the first failure. */
#include <stdio.h>

#include <set>

#include "rtuf_routes.h"

using namespace rtuf;

namespace {

enum { No = 0, Yes = 1, Any = -1 };
enum { Refused = 0, Ok = 1 };
constexpr BatchKind Filter = BatchKind::Filter, Bits = BatchKind::Bits, Render = BatchKind::Render, Residual = BatchKind::Residual,
                    Cloud = BatchKind::Cloud, Clearance = BatchKind::Clearance;

// A class of combinations (u16 and the cover pass never decide; Any: either) and what becomes of it.
struct Row {
  BatchKind kind; int labels, thresh, two_kernel, dilated;
  int ok; Tail tail;
  const char* why;
};
const Row kRows[] = {
  // full planes: over the z-surface whatever the two-kernel flag says
  {Filter, No, No, Any, No,        Ok, Tail::None, "pad_compare_kernel"},
  {Filter, Yes, Any, Any, Any,     Refused, Tail::None, "the label-plane calls"},
  {Filter, No, Yes, Any, Any,      Refused, Tail::None, "per-link thresholds in effect"},
  {Filter, No, No, Any, Yes,       Refused, Tail::None, "silhouette_dilation_px > 0"},
  // mask bits: the calls still refuse the two-kernel flag
  {Bits, No, No, No, No,           Ok, Tail::None, "pad_compare_kernel<BITS>"},
  {Bits, Yes, Any, Any, Any,       Refused, Tail::None, "no mask-bits call takes a label plane"},
  {Bits, No, Yes, Any, Any,        Refused, Tail::None, "per-link thresholds in effect"},
  {Bits, No, No, Any, Yes,         Refused, Tail::None, "silhouette_dilation_px > 0"},
  {Bits, No, No, Yes, No,          Refused, Tail::None, "check_bits_call: the two-kernel flag"},
  // render and residual batches
  {Render, Any, Any, Any, Any,     Refused, Tail::None, "render batches"},
  {Residual, Any, Any, Any, Any,   Refused, Tail::None, "residual batches"},
  // clouds and clearance tables: the flag does not enter
  {Cloud, No, No, Any, No,         Ok, Tail::Cloud, "pad_compare_kernel<BITS>, then the cloud kernels"},
  {Cloud, Yes, Any, Any, Any,      Refused, Tail::None, "no cloud call takes a label plane"},
  {Cloud, No, Yes, Any, Any,       Refused, Tail::None, "per-link thresholds in effect"},
  {Cloud, No, No, Any, Yes,        Refused, Tail::None, "silhouette_dilation_px > 0"},
  {Clearance, No, No, Any, No,     Ok, Tail::Clearance, "pad_compare_kernel<BITS>, then the clearance kernels"},
  {Clearance, Yes, Any, Any, Any,  Refused, Tail::None, "no clearance call takes a label plane"},
  {Clearance, No, Yes, Any, Any,   Refused, Tail::None, "per-link thresholds in effect"},
  {Clearance, No, No, Any, Yes,    Refused, Tail::None, "silhouette_dilation_px > 0"},
};

bool matches(int want, bool have) { return want == Any || (want == Yes) == have; }

}  // namespace

int main()
{
  const BatchKind kinds[] = {Filter, Bits, Render, Residual, Cloud, Clearance};
  std::set<int> padded_routes, plain_routes;
  int combinations = 0;
  for (BatchKind kind : kinds)
    for (int m = 0; m < 64; m++) {
      const bool u16 = m & 1, labels = m & 2, thresh = m & 4, two = m & 8, dilated = m & 16, cover = m & 32;
      const RouteFacts f = {kind, u16, labels, thresh, two, dilated ? 3 : 0, cover, true};
      const Route r = route_of(f);
      const Route plain = route_of(RouteFacts{kind, u16, labels, thresh, two, dilated ? 3 : 0, cover, false});
      if (plain.ok) plain_routes.insert(route_index(plain));
      const Row* row = nullptr;
      int hits = 0;
      for (const Row& q : kRows)
        if (q.kind == kind && matches(q.labels, labels) && matches(q.thresh, thresh) && matches(q.two_kernel, two) && matches(q.dilated, dilated)) { row = &q; hits++; }
      auto fail = [&](const char* what) {
        printf("kind %d u16 %d labels %d thresh %d two_kernel %d dilated %d cover %d: %s (%s)\n", (int)kind, u16, labels, thresh, two, dilated, cover, what, row ? row->why : "-");
        return 1;
      };
      if (hits != 1) return fail("not in exactly one row of the table");
      if (r.ok != (row->ok == Ok)) return fail(row->ok == Ok ? "refused, but the table admits it" : "admitted, but the table refuses it");
      combinations++;
      if (!r.ok) continue;
      if (!tile_variant_legal(r.tile)) return fail("an ok route with an illegal tile variant");
      if (r.tile.out != TileOut::ZSurface || !r.tile.labels || r.tile.thresh || r.tile.u16) return fail("not the z-surface variant with the slot plane");
      if (r.tile.cover != cover) return fail("tile cover");
      if (r.post != Post::Pad) return fail("post");
      if (r.tail != row->tail) return fail("tail");
      if (!runs_behind_tile(r)) return fail("runs_behind_tile");
      padded_routes.insert(route_index(r));
    }
  // Filter and Bits share a route (the request's buffers tell them apart, as with dilation); Cloud and Clearance have their tails:
  // three routes, with and without the cover pass
  if (padded_routes.size() != 2 * 3) { printf("%d distinct padded route numbers\n", (int)padded_routes.size()); return 1; }
  for (int i : padded_routes)
    if (plain_routes.count(i)) { printf("route number %d is a padded route and a route without padding\n", i); return 1; }
  printf("ok %d %d\n", combinations, (int)padded_routes.size());
  return 0;
}
