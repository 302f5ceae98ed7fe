/* CPU check of the kernel routes (realtime_urdf_filter_amd/csrc/rtuf_routes.h), the product's own route_of and
 * tile_variant_legal, over every combination of route_of's inputs: 7 kinds x u16 x label plane x thresholds x two-kernel flag x
 * dilation 0 / > 0 x cover pass x link padding x scene planes = 1,792.
 *   1. route_of agrees with kRows below: one row per class of combinations, written out from what the calls of the host API
 *      refuse, in the order they name their reasons, and otherwise from which kernel the launcher comes to.  Every combination
 *      falls into exactly one row; a refused row names the reason (Route::why), and ok is nothing but why == None.
 *   2. every route that is ok has a legal tile variant, the row's output, modifiers, post, tail and scene stage.
 *   3. the variants the routes reach, the variants tile_variant_legal admits, and kKernels below -- the 22 instantiations of
 *      the six wrapper kernels the launcher has always named, each with and without the cover code -- are one and the same set:
 *      44 variants, 88 kernels with the two workgroup sizes.  Padding, the scene and point lists add none.
 *   4. the scene fact changes nothing but the scene stage, refused or not; a point list batch is a render batch's plain float
 *      route with Tail::Points, refused or not; the enums were appended to.
 *   5. tile_variant_index and route_index tell distinct variants and routes apart, and the routes are as many as counted by hand.
 * g++ -O2 -I realtime_urdf_filter_amd/csrc;  prints "ok <combinations> <variants> <kernels> <routes> <plain> <padded> <points>
 * <scene>" and "refused <Kind:Reason> ..." (the pairs the table refuses), or the first failure. */
#include <stdio.h>

#include <map>
#include <set>
#include <string>
#include <tuple>

#include "rtuf_routes.h"

using namespace rtuf;

namespace {

enum { No = 0, Yes = 1, Any = -1, Always = 2 };
constexpr BatchKind Filter = BatchKind::Filter, Bits = BatchKind::Bits, Render = BatchKind::Render, Residual = BatchKind::Residual,
                    Cloud = BatchKind::Cloud, Clearance = BatchKind::Clearance, Points = BatchKind::Points;
using Why = Refusal;
constexpr Why Fine = Refusal::None;

const char* const kKindName[] = {"Filter", "Bits", "Render", "Residual", "Cloud", "Clearance", "Points"};
const char* const kWhyName[] = {"None", "NoLabelPlane", "LabelsDilation", "LabelsPadding", "RenderDilation", "RenderPadding", "ResidualDilation",
                                "ResidualPadding", "DilationPadding", "ThreshPadding", "ThreshZSurface", "ThreshDilation", "BitsTwoKernel",
                                "PointsDilation", "PointsPadding", "PointsThresh"};
static_assert((int)Refusal::None == 0 && (int)Refusal::PointsThresh + 1 == sizeof kWhyName / sizeof *kWhyName, "one name per reason");
static_assert((int)BatchKind::Filter == 0 && (int)BatchKind::Bits == 1 && (int)BatchKind::Render == 2 && (int)BatchKind::Residual == 3 &&
              (int)BatchKind::Cloud == 4 && (int)BatchKind::Clearance == 5 && (int)BatchKind::Points == 6, "BatchKind::Points is appended");
static_assert((int)Tail::None == 0 && (int)Tail::Cloud == 1 && (int)Tail::Clearance == 2 && (int)Tail::Points == 3 && kTails == 4, "Tail::Points is appended");
static_assert((int)Post::None == 0 && (int)Post::Compare == 1 && (int)Post::Dilate == 2 && (int)Post::Pad == 3 && kPosts == 4, "Post::Pad is appended");

// A class of combinations (u16, the cover pass and the scene never decide; Any: either) and what becomes of it: the reason it
// is refused for, or Fine.  For a row that is Fine: the tile kernel's output, whether the variant takes over the label plane /
// the thresholds / 16UC1 from the inputs (No: the variant has it off whatever the input says; Always: on whatever it says),
// what runs behind the tile kernel, and whether the scene stage is among it when scene planes are in effect.
struct Row {
  BatchKind kind; int labels, thresh, two_kernel, dilated, padded;
  Why why; TileOut out; int keeps_labels, keeps_thresh, keeps_u16; Post post; Tail tail; int stage;
  const char* kernels;
};
constexpr TileOut kNoOut = TileOut::Planes;
#define REFUSED(why) Why::why, kNoOut, No, No, No, Post::None, Tail::None, No, "-"
const Row kRows[] = {
  // full planes: fused; the flag sends them over the z-surface to compare_kernel, a radius to dilate_compare_kernel, padding
  // -- whatever the flag says -- to pad_compare_kernel with the link slots in the label plane's place
  {Filter, Any, Any, No, No, No,      Fine, TileOut::Planes, Yes, Yes, Yes, Post::None, Tail::None, Yes, "tile_kernel / tile_labels_kernel / tile_thresh_kernel"},
  {Filter, Any, No, Yes, No, No,      Fine, TileOut::ZSurface, Yes, No, No, Post::Compare, Tail::None, Yes, "tile_kernel<true> / tile_labels_kernel<true>"},
  {Filter, No, No, Any, Yes, No,      Fine, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::None, Yes, "tile_kernel<true>"},
  {Filter, No, No, Any, No, Yes,      Fine, TileOut::ZSurface, Always, No, No, Post::Pad, Tail::None, Yes, "tile_labels_kernel<true>, pad_compare_kernel"},
  {Filter, Yes, Any, Any, Yes, Any,   REFUSED(LabelsDilation)},
  {Filter, Yes, Any, Any, No, Yes,    REFUSED(LabelsPadding)},
  {Filter, No, Any, Any, Yes, Yes,    REFUSED(DilationPadding)},
  {Filter, No, Yes, Any, No, Yes,     REFUSED(ThreshPadding)},
  {Filter, Any, Yes, Yes, No, No,     REFUSED(ThreshZSurface)},
  {Filter, No, Yes, Any, Yes, No,     REFUSED(ThreshZSurface)},
  // mask bits (the learn-scene batch too): fused only
  {Bits, Yes, Any, Any, Any, Any,     REFUSED(NoLabelPlane)},
  {Bits, No, Any, Yes, Any, Any,      REFUSED(BitsTwoKernel)},
  {Bits, No, Any, No, Yes, Yes,       REFUSED(DilationPadding)},
  {Bits, No, Yes, No, No, Yes,        REFUSED(ThreshPadding)},
  {Bits, No, Yes, No, Yes, No,        REFUSED(ThreshZSurface)},
  {Bits, No, Any, No, No, No,         Fine, TileOut::Bits, No, Yes, Yes, Post::None, Tail::None, Yes, "tile_bits_kernel / tile_thresh_kernel<BITS>"},
  {Bits, No, No, No, Yes, No,         Fine, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::None, Yes, "tile_kernel<true>"},
  {Bits, No, No, No, No, Yes,         Fine, TileOut::ZSurface, Always, No, No, Post::Pad, Tail::None, Yes, "tile_labels_kernel<true>, pad_compare_kernel<BITS>"},
  // virtual depth: neither thresholds nor the flag nor the scene enter
  {Render, Any, Any, Any, Yes, Any,   REFUSED(RenderDilation)},
  {Render, Yes, Any, Any, No, Yes,    REFUSED(LabelsPadding)},
  {Render, No, Any, Any, No, Yes,     REFUSED(RenderPadding)},
  {Render, Any, Any, Any, No, No,     Fine, TileOut::Render, Yes, No, Yes, Post::None, Tail::None, No, "tile_render_kernel"},
  // residual tables: thresholds are honoured, the flag and the scene do not enter
  {Residual, Yes, Any, Any, Any, Any, REFUSED(NoLabelPlane)},
  {Residual, No, Any, Any, Yes, Any,  REFUSED(ResidualDilation)},
  {Residual, No, Any, Any, No, Yes,   REFUSED(ResidualPadding)},
  {Residual, No, Any, Any, No, No,    Fine, TileOut::Residual, No, Yes, Yes, Post::None, Tail::None, No, "tile_resid_kernel"},
  // clouds and clearance tables: a mask-bits batch (the flag does not enter) with their kernels behind it
  {Cloud, Yes, Any, Any, Any, Any,    REFUSED(NoLabelPlane)},
  {Cloud, No, Yes, Any, Yes, Any,     REFUSED(ThreshDilation)},
  {Cloud, No, No, Any, Yes, Yes,      REFUSED(DilationPadding)},
  {Cloud, No, Yes, Any, No, Yes,      REFUSED(ThreshPadding)},
  {Cloud, No, Any, Any, No, No,       Fine, TileOut::Bits, No, Yes, Yes, Post::None, Tail::Cloud, Yes, "tile_bits_kernel / tile_thresh_kernel<BITS>"},
  {Cloud, No, No, Any, Yes, No,       Fine, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::Cloud, Yes, "tile_kernel<true>"},
  {Cloud, No, No, Any, No, Yes,       Fine, TileOut::ZSurface, Always, No, No, Post::Pad, Tail::Cloud, Yes, "tile_labels_kernel<true>, pad_compare_kernel<BITS>"},
  {Clearance, Yes, Any, Any, Any, Any, REFUSED(NoLabelPlane)},
  {Clearance, No, Yes, Any, Yes, Any, REFUSED(ThreshDilation)},
  {Clearance, No, No, Any, Yes, Yes,  REFUSED(DilationPadding)},
  {Clearance, No, Yes, Any, No, Yes,  REFUSED(ThreshPadding)},
  {Clearance, No, Any, Any, No, No,   Fine, TileOut::Bits, No, Yes, Yes, Post::None, Tail::Clearance, Yes, "tile_bits_kernel / tile_thresh_kernel<BITS>"},
  {Clearance, No, No, Any, Yes, No,   Fine, TileOut::ZSurface, No, No, No, Post::Dilate, Tail::Clearance, Yes, "tile_kernel<true>"},
  {Clearance, No, No, Any, No, Yes,   Fine, TileOut::ZSurface, Always, No, No, Post::Pad, Tail::Clearance, Yes, "tile_labels_kernel<true>, pad_compare_kernel<BITS>"},
  // point lists: a render batch into a float plane of the library's, the flag and the scene do not enter
  {Points, Yes, Any, Any, Any, Any,   REFUSED(NoLabelPlane)},
  {Points, No, Any, Any, Yes, Any,    REFUSED(PointsDilation)},
  {Points, No, Any, Any, No, Yes,     REFUSED(PointsPadding)},
  {Points, No, Yes, Any, No, No,      REFUSED(PointsThresh)},
  {Points, No, No, Any, No, No,       Fine, TileOut::Render, No, No, No, Post::None, Tail::Points, No, "tile_render_kernel, then points_filter_kernel"},
};

// The instantiations the tile launcher names, without the COVER and NT arguments every one of them has besides.
struct Kernel { const char* name; TileOut out; bool labels, thresh, u16; };
const Kernel kKernels[] = {
  {"tile_kernel<false, false>", TileOut::Planes, false, false, false},
  {"tile_kernel<false, true>", TileOut::Planes, false, false, true},
  {"tile_kernel<true, false>", TileOut::ZSurface, false, false, false},
  {"tile_bits_kernel<false>", TileOut::Bits, false, false, false},
  {"tile_bits_kernel<true>", TileOut::Bits, false, false, true},
  {"tile_labels_kernel<false, false>", TileOut::Planes, true, false, false},
  {"tile_labels_kernel<false, true>", TileOut::Planes, true, false, true},
  {"tile_labels_kernel<true, false>", TileOut::ZSurface, true, false, false},
  {"tile_thresh_kernel<false, false, false>", TileOut::Planes, false, true, false},      // <U16, BITS, LABELS>
  {"tile_thresh_kernel<true, false, false>", TileOut::Planes, false, true, true},
  {"tile_thresh_kernel<false, true, false>", TileOut::Bits, false, true, false},
  {"tile_thresh_kernel<true, true, false>", TileOut::Bits, false, true, true},
  {"tile_thresh_kernel<false, false, true>", TileOut::Planes, true, true, false},
  {"tile_thresh_kernel<true, false, true>", TileOut::Planes, true, true, true},
  {"tile_render_kernel<false, false>", TileOut::Render, false, false, false},            // <U16, LABELS>
  {"tile_render_kernel<true, false>", TileOut::Render, false, false, true},
  {"tile_render_kernel<false, true>", TileOut::Render, true, false, false},
  {"tile_render_kernel<true, true>", TileOut::Render, true, false, true},
  {"tile_resid_kernel<false, false>", TileOut::Residual, false, false, false},           // <U16, THRESH>
  {"tile_resid_kernel<true, false>", TileOut::Residual, false, false, true},
  {"tile_resid_kernel<false, true>", TileOut::Residual, false, true, false},
  {"tile_resid_kernel<true, true>", TileOut::Residual, false, true, true},
};
constexpr int kWorkgroupSizes = 2;       // 256 and 1,024 threads: launch_tile picks by the launch's size, not by the route

bool matches(int want, bool have) { return want == Any || (want == Yes) == have; }
bool kept(int keeps, bool have) { return keeps == Always || (keeps == Yes && have); }

using Key = std::tuple<int, bool, bool, bool, bool, int, int, bool>;
Key key_of(const Route& r) { return Key{(int)r.tile.out, r.tile.labels, r.tile.thresh, r.tile.u16, r.tile.cover, (int)r.post, (int)r.tail, r.scene}; }

}  // namespace

int main()
{
  const BatchKind kinds[] = {Filter, Bits, Render, Residual, Cloud, Clearance, Points};
  std::set<int> reached, legal, named;
  std::set<int> plain_routes, padded_routes, points_routes, scene_routes;      // route numbers, by what the route has
  std::map<int, Key> by_index;
  std::set<std::string> refused;
  int combinations = 0;
  for (BatchKind kind : kinds)
    for (int m = 0; m < 256; m++) {
      const bool u16 = m & 1, labels = m & 2, thresh = m & 4, two = m & 8, dilated = m & 16, cover = m & 32, padded = m & 64, scene = m & 128;
      const RouteFacts f = {kind, u16, labels, thresh, two, dilated ? 3 : 0, cover, padded, scene};
      const Route r = route_of(f);
      const Row* row = nullptr;
      int hits = 0;
      for (const Row& q : kRows)
        if (q.kind == kind && matches(q.labels, labels) && matches(q.thresh, thresh) && matches(q.two_kernel, two) && matches(q.dilated, dilated) && matches(q.padded, padded)) { row = &q; hits++; }
      auto fail = [&](const char* what) {
        printf("kind %s u16 %d labels %d thresh %d two_kernel %d dilated %d cover %d padded %d scene %d: %s (table: %s, %s; route_of: %s)\n", kKindName[(int)kind],
               u16, labels, thresh, two, dilated, cover, padded, scene, what, row ? kWhyName[(int)row->why] : "-", row ? row->kernels : "-", kWhyName[(int)r.why]);
        return 1;
      };
      if (hits != 1) return fail("not in exactly one row of the table");
      if (r.ok() != (r.why == Refusal::None)) return fail("ok is not why == None");
      if (r.ok() != (row->why == Fine)) return fail(row->why == Fine ? "refused, but the table admits it" : "admitted, but the table refuses it");
      if (r.why != row->why) return fail("refused for another reason");
      combinations++;
      // the scene fact: nothing but the stage, refused or not, and the stage never without the fact
      const Route bare = route_of(RouteFacts{kind, u16, labels, thresh, two, dilated ? 3 : 0, cover, padded, false});
      const bool wants = kind == Filter || kind == Bits || kind == Cloud || kind == Clearance;
      if (bare.scene) return fail("the scene stage without the fact");
      if (tile_variant_index(r.tile) != tile_variant_index(bare.tile) || r.tile.out != bare.tile.out) return fail("the scene changed the tile variant");
      if (r.post != bare.post || r.tail != bare.tail) return fail("the scene changed post or tail");
      if (r.why != bare.why) return fail("the scene refuses nothing and admits nothing");
      if (r.scene != (scene && wants)) return fail(wants ? "no scene stage" : "a scene stage on a batch that compares nothing against the scene");
      if (r.scene && (!runs_behind_tile(r) || route_index(r) == route_index(bare))) return fail("the scene route is not told from the plain one");
      if (kind == Points) {
        // refused or not: tile_render_kernel's plain float variant with the cover pass as it is, and nothing but the points
        // kernel behind it -- but for the tail, the route of a render batch in a context without any of the refused facts
        if (!tile_variant_legal(r.tile) || r.tile.out != TileOut::Render || r.tile.labels || r.tile.thresh || r.tile.u16) return fail("not the plain float render variant");
        if (r.tile.cover != cover || r.post != Post::None || r.tail != Tail::Points || r.scene || !runs_behind_tile(r)) return fail("not render, then points");
        const Route render = route_of(RouteFacts{Render, false, false, false, two, 0, cover, false, scene});
        if (!render.ok() || tile_variant_index(render.tile) != tile_variant_index(r.tile) || render.post != r.post || render.scene != r.scene)
          return fail("not a render batch's tile kernel");
      } else if (r.tail == Tail::Points) return fail("an older kind takes the points tail");
      if (!r.ok()) { refused.insert(std::string(kKindName[(int)kind]) + ":" + kWhyName[(int)r.why]); continue; }
      if (!tile_variant_legal(r.tile)) return fail("an ok route with an illegal tile variant");
      if (r.tile.out != row->out) return fail("tile output");
      if (r.tile.labels != kept(row->keeps_labels, labels)) return fail("tile labels");
      if (r.tile.thresh != kept(row->keeps_thresh, thresh)) return fail("tile thresh");
      if (r.tile.u16 != kept(row->keeps_u16, u16)) return fail("tile u16");
      if (r.tile.cover != cover) return fail("tile cover");
      if (r.post != row->post) return fail("post");
      if ((r.post == Post::Pad) != padded) return fail("Post::Pad is for padding, and padding has no other route");
      if (r.tail != row->tail) return fail("tail");
      if (r.scene != (scene && row->stage == Yes)) return fail("scene stage");
      if (runs_behind_tile(r) != (row->post != Post::None || row->tail != Tail::None || r.scene)) return fail("runs_behind_tile");
      reached.insert(tile_variant_index(r.tile));
      const int i = route_index(r);
      auto it = by_index.find(i);
      if (it == by_index.end()) by_index.emplace(i, key_of(r));
      else if (it->second != key_of(r)) return fail("two different routes share a route_index");
      (r.scene ? scene_routes : kind == Points ? points_routes : padded ? padded_routes : plain_routes).insert(i);
    }
  // every variant there could be: which are legal, and do their numbers differ
  std::set<int> all;
  for (int out = 0; out < kTileOuts; out++)
    for (int m = 0; m < 16; m++) {
      const TileVariant v = {(TileOut)out, (m & 8) != 0, (m & 4) != 0, (m & 2) != 0, (m & 1) != 0};
      const int i = tile_variant_index(v);
      if (i < 0 || i >= kTileVariantSlots || !all.insert(i).second) { printf("tile_variant_index %d: out of range or taken twice\n", i); return 1; }
      if (tile_variant_legal(v)) legal.insert(i);
    }
  for (const Kernel& k : kKernels)
    for (int cover = 0; cover < 2; cover++) {
      const TileVariant v = {k.out, k.labels, k.thresh, k.u16, cover != 0};
      if (!tile_variant_legal(v)) { printf("%s: not a legal variant\n", k.name); return 1; }
      if (!named.insert(tile_variant_index(v)).second) { printf("%s: a second kernel for one variant\n", k.name); return 1; }
    }
  if (named.size() != 44) { printf("%d named variants, not 44\n", (int)named.size()); return 1; }
  if (reached != named) { printf("the routes reach %d variants, the launcher names %d: not the same set\n", (int)reached.size(), (int)named.size()); return 1; }
  if (legal != named) { printf("%d legal variants, the launcher names %d: not the same set\n", (int)legal.size(), (int)named.size()); return 1; }
  // Routes that differ in anything differ in route_index (by_index above), so the four sets are disjoint by what they hold.
  //   plain, 66: with nothing behind the tile kernel 8 plane, 4 bits, 4 render and 4 residual variants; the z-surface with and
  //     without labels before compare, without before dilate and each of the 3 tails; the 4 bits variants before the cloud and
  //     the clearance kernels -- all with and without the cover pass: 2 * (20 + 2 + 3 + 8);
  //   padded, 6: Filter and Bits share a route (the request's buffers tell them apart, as with dilation), Cloud and Clearance
  //     have their tails -- with and without the cover pass;
  //   points, 2: with and without the cover pass;
  //   scene, 56: every plain and padded route but the 8 render and 8 residual ones has a twin with the stage: 66 - 16 + 6.
  const size_t total = plain_routes.size() + padded_routes.size() + points_routes.size() + scene_routes.size();
  if (plain_routes.size() != 2 * (20 + 2 + 3 + 8) || padded_routes.size() != 2 * 3 || points_routes.size() != 2 || scene_routes.size() != 66 - 16 + 6 ||
      by_index.size() != total || total != 130) {
    printf("%d distinct route numbers: %d plain, %d padded, %d points, %d scene\n", (int)by_index.size(), (int)plain_routes.size(), (int)padded_routes.size(),
           (int)points_routes.size(), (int)scene_routes.size());
    return 1;
  }
  printf("ok %d %d %d %d %d %d %d %d\n", combinations, (int)named.size(), (int)named.size() * kWorkgroupSizes, (int)total, (int)plain_routes.size(),
         (int)padded_routes.size(), (int)points_routes.size(), (int)scene_routes.size());
  printf("refused");
  for (const std::string& p : refused) printf(" %s", p.c_str());
  printf("\n");
  return 0;
}
