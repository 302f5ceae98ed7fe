"""CPU (-m "not gpu"): which kernels a batch runs -- its route -- is decided in one header, rtuf_routes.h.

tests/routes_check.cpp holds the library's own route_of and tile_variant_legal against a table written out by hand, for all
1,792 combinations of batch kind, 16UC1, label plane, per-link thresholds, two-kernel flag, dilation, cover pass, link padding
and scene planes -- the route, or the reason the combination is refused for -- and the variants the routes reach against the
22 x 2 instantiations of the tile kernel the launcher names (see its head comment).  The source checks below keep the host API
and the launcher from growing a second copy of the rule."""
import os
import re
import subprocess

import pytest

import enqueue_steps as ES

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "realtime_urdf_filter_amd", "csrc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("routes") / "routes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(HERE, "routes_check.cpp")])
    return exe


def test_route_of_is_the_table_for_every_combination(check):
    r = subprocess.run([check], capture_output=True, text=True, timeout=60)
    print(r.stdout.strip())
    # (1,792 combinations subsume the 384 of six kinds without padding or a scene this asserted before; 44 and 88 as before;
    # then the distinct route numbers: 130 = 66 plain + 6 padded + 2 points + 56 with the scene stage)
    assert r.returncode == 0 and r.stdout.splitlines()[0].split() == ["ok", "1792", "44", "88", "130", "66", "6", "2", "56"], r.stdout
    assert r.stdout.splitlines()[1].startswith("refused Bits:BitsTwoKernel ") and len(r.stdout.splitlines()) == 2, r.stdout


def test_the_header_is_the_one_place_that_refuses():
    """Every refusal's message stands once in the sources, in check_route's table; no other check of a call tests the facts a
    route follows from; and every batch entry point reaches check_route."""
    srcs = {n: open(os.path.join(CSRC, n)).read() for n in os.listdir(CSRC) if n.endswith((".cpp", ".h", ".hip"))}
    api = srcs["rtuf_api.cpp"]
    table = _body(api, "static int check_route(")
    messages = re.findall(r'^\s+"([^"]+)",?\s*(?://.*)?$', table, re.M)
    assert len(messages) == 15 and messages[0].startswith("internal: ") and len(set(messages)) == 15, messages
    for m in messages:
        assert sum(s.count(m) for s in srcs.values()) == 1, m
    assert sum(("not supported with" in m) for m in messages) == 13 and sum(s.count("not supported with") for s in srcs.values()) == 13
    for head in set(re.findall(r"^static int (check_\w+)\(", api, re.M)) - {"check_route"}:
        body = _body(api, "static int %s(" % head)
        for fact in ("silhouette_dilation_px", "pad_models > 0", "thresh_models", "RTUF_FLAG_TWO_KERNEL"):
            assert fact not in body, (head, fact)
    for gone in ("check_thresh_route", "check_pad_route", "subject_to_thresh_route"):
        assert gone not in api, gone
    # every batch call goes through the check of its kind, and each of those asks check_route once
    checks = ("check_filter_call(", "check_bits_call(", "check_render_call(", "check_residuals_call(", "check_cloud_call(", "check_clearance_call(",
              "check_points_call(")
    for c in checks:
        assert _body(api, "static int " + c).count("check_route(c, ") == 1, c
    assert api.count("check_route(c, ") == len(checks)


def _body(src, head):
    """The text of the function that starts with `head`, up to the closing brace in column 0."""
    start = src.index(head)
    return src[start:src.index("\n}\n", start)]


def test_the_kernels_and_the_host_take_the_route_from_the_header():
    api = open(os.path.join(CSRC, "rtuf_api.cpp")).read()
    dev = open(os.path.join(CSRC, "rtuf_kernels.hip")).read()
    hdr = open(os.path.join(CSRC, "rtuf_device.h")).read()
    for src in (api, dev, hdr):
        assert '#include "rtuf_routes.h"' in src
    routes = open(os.path.join(CSRC, "rtuf_routes.h")).read()
    assert "#include <hip" not in routes and "__device__" not in routes      # plain C++: the CPU check compiles it

    # the host asks in two places, of the same facts (route_facts): check_route, which refuses a call before it builds,
    # allocates or enqueues anything, and enqueue_batch, once, before anything of the context or the slot changes (a re-run
    # takes the stored route)
    assert api.count("route_of(") == 2 == api.count("route_of(route_facts(c, ") and api.count("RouteFacts{") == 1
    assert "route_of(route_facts(c, r)).why" in _body(api, "static int check_route(")
    enqueue = _body(api, "static int enqueue_batch(")
    ask = enqueue.index("route_of(")
    assert "rerun ? b.route" in enqueue[:ask] and enqueue.index("if (!route.ok() || !tile_variant_legal(route.tile))\n    return c->fail(RTUF_ERR_STATE") > ask
    # (before anything changes: the request and the refusal precede every step of enqueue_batch, where the changes stand)
    assert ES.CHECKS[1:] == ("route_of(", "if (!route.ok() || !tile_variant_legal(route.tile))\n    return c->fail(RTUF_ERR_STATE")
    ES.assert_checks_precede_every_change(api)
    # ... and keeps no second encoding of it: the plan's flags, the slot's saved pieces, the predicates the route replaced
    for gone in ("zroute", "b.cover_pass", "b.order_thr", "gr.compare", "gr.dilate", "gr.cloud", "gr.clearance", "takes_two_kernel",
                 "honours_dilation", "reads_thresholds", "fills_ms_compare", "enum class Kind"):
        assert gone not in api, gone
    assert "(uint64_t)route_index(route) << 32" in api      # equal argument blocks, another route: another graph
    # no stage of the host learns the kind of a batch from a pointer of the tile kernel's argument block
    issue = _body(api, "static int issue_plan(")
    assert not re.search(r"if \((!)?gr\.ta\.\w+\)", issue)
    assert "launch_tile(gr.ta, rt.tile, st)" in issue

    # the launcher goes from the variant to the kernel, and decodes no pointer
    launch = dev[dev.index("static TileKernel tile_kernel_for("):dev.index("void launch_zero_residual_rows(")]
    for gone in ("a.resid_table) {", "a.virtual_out) {", "a.order_thr) {", "a.labels) {", "a.bits) {", "a.io_u16", "two_kernel"):
        assert gone not in launch, gone
    assert "launch_tile_variant" not in dev
    cases = re.findall(r"case V\(O::(\w+), (true|false), (true|false), (true|false)\): return (tile_\w*kernel)<", launch)
    assert len(cases) == 22 and len(set(c[:4] for c in cases)) == 22
    assert sorted(set(c[4] for c in cases)) == ["tile_bits_kernel", "tile_kernel", "tile_labels_kernel", "tile_render_kernel", "tile_resid_kernel", "tile_thresh_kernel"]
    assert "default: return nullptr;" in launch and "if (!kernel) return false;" in launch
    # the kernel body refuses an instantiation the header does not admit
    assert "static_assert(tile_variant_legal(TileVariant{OUT, LABELS, THRESH, U16, COVER})" in _body(dev, "__device__ __forceinline__ void tile_body(")
