"""GPU (-m gpu, except the check of the case list): every combination the API refuses because no kernel route exists for it
(csrc/rtuf_routes.h, enum class Refusal), through the public calls.

One scene, soup_scene(1, 160, 120), three streams, and two contexts: one pipeline, and two pipelines for the forwarded error.
Labels, spheres and cloud intrinsics are set for every stream, so a call can only fail by a rule of the route table.  A case is
(kind, reason, the facts that hold): the facts are set with the public setters -- T per-link thresholds, K the two-kernel flag,
D a silhouette radius, P link padding; L is the label plane of the call itself -- and the kind's device form is called, then
its host form.  Every call must return RTUF_ERR_INVALID with the reason's message, byte for byte.  PRECEDENCE holds the states
in which two reasons of a kind's row apply at once: the earlier one of the table is reported.  After all refusals the device
outputs still hold their sentinel, rtuf_stats.device_bytes is what it was before every refused call, and a plain filter batch
on the same context gives the oracle's planes exactly."""
import os
import subprocess

import numpy as np
import pytest

import gpu_support as K
import realtime_urdf_filter_amd as R

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "realtime_urdf_filter_amd", "csrc")
INVALID = -1
LINK_LABEL = (3, 7, 7, 1, 12, 5)
N_LABELS = 13
LINK_THR = (0.30, -0.02, 0.05, 0.60, 0.0, 0.12)
LINK_PAD = (0.02,) * 6
RADIUS = 2
CAPACITY = 64
SENT = 0x5a

MESSAGE = {
    "LabelsDilation": "link labels are not supported with silhouette dilation yet",
    "LabelsPadding": "link labels are not supported with link padding yet",
    "RenderDilation": "virtual depth is not supported with silhouette dilation yet",
    "RenderPadding": "virtual depth is not supported with link padding yet",
    "ResidualDilation": "link residual tables are not supported with silhouette dilation yet",
    "ResidualPadding": "link residual tables are not supported with link padding yet",
    "DilationPadding": "silhouette dilation is not supported with link padding yet",
    "ThreshPadding": "per-link depth thresholds are not supported with link padding yet",
    "ThreshZSurface": "per-link depth thresholds are not supported with RTUF_FLAG_TWO_KERNEL or silhouette dilation yet",
    "ThreshDilation": "per-link depth thresholds are not supported with silhouette dilation yet",
    "BitsTwoKernel": "mask-bits output exists in fused mode only (RTUF_FLAG_TWO_KERNEL is set)",
    "PointsDilation": "point list batches are not supported with silhouette dilation yet (radius_px is this batch's own margin)",
    "PointsPadding": "point list batches are not supported with link padding yet",
    "PointsThresh": "point list batches are not supported with per-link depth thresholds yet",
}

# (kind, reason, facts): every reachable (kind, reason) of the route table, with the fewest facts that give it.  "learn" is the
# learn-scene call: a Bits batch of the library's own.
CASES = [
    ("filter", "LabelsDilation", "LD"), ("filter", "LabelsPadding", "LP"), ("filter", "DilationPadding", "PD"),
    ("filter", "ThreshPadding", "PT"), ("filter", "ThreshZSurface", "TK"), ("filter", "ThreshZSurface", "TD"),
    ("bits", "BitsTwoKernel", "K"), ("bits", "DilationPadding", "PD"), ("bits", "ThreshPadding", "PT"), ("bits", "ThreshZSurface", "TD"),
    ("learn", "BitsTwoKernel", "K"), ("learn", "DilationPadding", "PD"), ("learn", "ThreshPadding", "PT"), ("learn", "ThreshZSurface", "TD"),
    ("render", "RenderDilation", "D"), ("render", "LabelsPadding", "LP"), ("render", "RenderPadding", "P"),
    ("residual", "ResidualDilation", "D"), ("residual", "ResidualPadding", "P"),
    ("cloud", "ThreshDilation", "TD"), ("cloud", "DilationPadding", "PD"), ("cloud", "ThreshPadding", "PT"),
    ("clearance", "ThreshDilation", "TD"), ("clearance", "DilationPadding", "PD"), ("clearance", "ThreshPadding", "PT"),
    ("points", "PointsDilation", "D"), ("points", "PointsPadding", "P"), ("points", "PointsThresh", "T"),
]

# Two reasons of one row at once: one state per adjacent pair of the row that the setters can produce without a third, earlier
# reason of the row holding too (Filter: L&P with P&D needs L, P and D, where L&D comes first; likewise P&T with T&D in the
# Bits row and P&D with P&T in the Cloud row).  The reason named is the earlier one.
PRECEDENCE = [
    ("filter", "LabelsDilation", "LDP"),       # before labels/padding
    ("filter", "DilationPadding", "PDT"),      # before thresholds/padding
    ("filter", "ThreshPadding", "PTK"),        # before thresholds/z-surface
    ("bits", "BitsTwoKernel", "KPD"),          # before dilation/padding
    ("bits", "DilationPadding", "PDT"),        # before thresholds/padding
    ("learn", "BitsTwoKernel", "KPD"),
    ("learn", "DilationPadding", "PDT"),
    ("render", "RenderDilation", "DLP"),       # before labels/padding (labels/padding before render/padding: the case list's LP)
    ("residual", "ResidualDilation", "DP"),    # before residual/padding
    ("cloud", "ThreshDilation", "TDP"),        # before dilation/padding
    ("clearance", "ThreshDilation", "TDP"),
    ("points", "PointsDilation", "DP"),        # before points/padding
    ("points", "PointsPadding", "PT"),         # before points/thresholds
]

KIND_OF = {"filter": "Filter", "bits": "Bits", "learn": "Bits", "render": "Render", "residual": "Residual", "cloud": "Cloud",
           "clearance": "Clearance", "points": "Points"}


def test_the_cases_are_the_refusals_of_the_table(tmp_path):
    """tests/routes_check.cpp prints the (kind, reason) pairs its table refuses; but for NoLabelPlane, which no call can ask
    for, the case list meets every one of them, names no other, and has a message for every reason."""
    exe = str(tmp_path / "routes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(HERE, "routes_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines()
    line = [l for l in out if l.startswith("refused ")]
    assert len(line) == 1, out
    table = {tuple(p.split(":")) for p in line[0].split()[1:]}
    reachable = {(k, r) for k, r in table if r != "NoLabelPlane"}
    assert {k for k, r in table if r == "NoLabelPlane"} == {"Bits", "Residual", "Cloud", "Clearance", "Points"}
    assert {(KIND_OF[k], r) for k, r, _ in CASES} == reachable
    assert {(KIND_OF[k], r) for k, r, _ in PRECEDENCE} <= reachable
    assert {r for _, r in reachable} == set(MESSAGE) and len(set(MESSAGE.values())) == 14
    assert {k for k, _, _ in CASES if KIND_OF[k] != "Bits"} | {"bits", "learn"} == set(KIND_OF)


class Calls:
    """The device and host forms of every kind on one context, the device outputs filled with a sentinel."""

    def __init__(self, sc, ctx):
        torch, dev = K.torch_device()
        self.sc, self.ctx, self.torch = sc, ctx, torch
        n, shape = sc.n, (sc.n, sc.H, sc.W)
        full = lambda sh, dt=torch.uint8: torch.full(sh, SENT, dtype=dt, device=dev)
        self.d_depth = K.upload(sc.depth)
        self.d_points = torch.zeros((n, CAPACITY, 3), dtype=torch.float32, device=dev)
        self.d_counts = torch.full((n,), CAPACITY, dtype=torch.int32, device=dev)
        self.out = {"masked": full(shape + (4,)), "mask": full(shape), "labels": full(shape + (2,)), "bits": full((n, 4 * ctx.mask_bits_words())),
                    "virtual": full(shape + (4,)), "residual": full((n, N_LABELS, 64)), "cloud": full(shape + (12,)),
                    "clearance": full((n, N_LABELS, 16)), "verdict": full((n, CAPACITY))}
        self.lists = [np.full((CAPACITY, 3), 1.0, np.float32) for _ in range(n)]

    def device(self, kind, labels):
        ctx, n, d, p = self.ctx, self.sc.n, self.d_depth.data_ptr(), {k: t.data_ptr() for k, t in self.out.items()}
        if kind == "filter" and labels:
            ctx.filter_batch_device_labels(n, d, p["masked"], p["mask"], p["labels"])
        elif kind == "filter":
            ctx.filter_batch_device(n, d, p["masked"], p["mask"])
        elif kind == "bits":
            ctx.filter_batch_device_bits(n, d, p["bits"])
        elif kind == "learn":
            ctx.learn_scene_batch_device(n, d)
        elif kind == "render":
            ctx.render_batch_device(n, p["virtual"], p["labels"] if labels else None, 0.0)
        elif kind == "residual":
            ctx.link_residuals_batch_device(n, d, p["residual"], N_LABELS)
        elif kind == "cloud":
            ctx.cloud_batch_device(n, d, p["cloud"])
        elif kind == "clearance":
            ctx.link_clearance_batch_device(n, d, p["clearance"], N_LABELS, 1.5)
        else:
            ctx.points_batch_device(n, self.d_points.data_ptr(), self.d_counts.data_ptr(), CAPACITY, 0, p["verdict"])

    def host(self, kind, labels):
        ctx, sc = self.ctx, self.sc
        if kind == "filter" and labels:
            ctx.filter_batch_labels(sc.depth)
        elif kind == "filter":
            ctx.filter_batch(sc.depth)
        elif kind == "bits":
            ctx.filter_batch_bits_async(sc.depth, np.zeros((sc.n, ctx.mask_bits_words()), np.uint32))
        elif kind == "learn":
            ctx.learn_scene_batch(sc.depth)
        elif kind == "render":
            ctx.render_batch(sc.n, 0.0, labels=labels)
        elif kind == "residual":
            ctx.link_residuals_batch(sc.depth, N_LABELS)
        elif kind == "cloud":
            ctx.cloud_batch(sc.depth)
        elif kind == "clearance":
            ctx.link_clearance_batch(sc.depth, N_LABELS, 1.5)
        else:
            ctx.points_batch(self.lists, 0)

    def untouched(self):
        self.torch.cuda.synchronize()
        return [k for k, t in self.out.items() if not bool((t == SENT).all())]


def make_context(sc, **kw):
    ctx = K.cloud_context(sc, **kw)
    ctx.set_link_labels(0, np.array(LINK_LABEL, np.uint16))
    links = list(range(sc.n_links))
    ctx.set_link_spheres(0, links, [(0.0, 0.0, 0.0, 0.05)] * len(links))
    return ctx


def set_facts(ctx, sc, facts):
    K.set_radius(ctx, sc, RADIUS if "D" in facts else 0, flags=R.FLAG_TWO_KERNEL if "K" in facts else 0)
    if "T" in facts:
        ctx.set_link_thresholds(0, np.array(LINK_THR, np.float32))
    else:
        ctx.clear_link_thresholds(0)
    if "P" in facts:
        ctx.set_link_padding(0, np.array(LINK_PAD, np.float32))
    else:
        ctx.clear_link_padding(0)


def refuse(calls, kind, reason, facts, grew):
    """Both forms of the kind in the state `facts`: the code and the message; a call that changed device_bytes goes to `grew`."""
    set_facts(calls.ctx, calls.sc, facts)
    for form in (calls.device, calls.host):
        what = "%s %s %s (%s)" % (form.__name__, kind, facts, reason)
        before = calls.ctx.stats()["device_bytes"]
        with pytest.raises(R.RtufError) as e:
            form(kind, "L" in facts)
        print("%s: %d %s" % (what, e.value.code, e.value))
        assert e.value.code == INVALID and str(e.value) == "rtuf error %d: %s" % (INVALID, MESSAGE[reason]), what
        if calls.ctx.stats()["device_bytes"] != before:
            grew.append(what)


@gpu
def test_every_refusal_its_code_its_message_and_nothing_else():
    sc = K.soup_scene(1, 160, 120)
    ctx = make_context(sc)
    calls = Calls(sc, ctx)
    grew = []
    for kind, reason, facts in CASES + PRECEDENCE:
        refuse(calls, kind, reason, facts, grew)
    assert calls.untouched() == []
    # The one thing the commit before this test's did not satisfy: there a refused learn-scene call had already allocated the
    # scene planes, and a refused clearance call under padding the device copy of the spheres.
    assert grew == [], grew
    set_facts(ctx, sc, "")
    masked, mask = ctx.filter_batch(sc.depth)
    want_masked, want_mask = K.filter_expected(sc, 0)
    K.compare_planes(masked, want_masked, "the batch after the refusals", "masked")
    K.compare_labels(mask, want_mask, "the batch after the refusals", "mask")
    ctx.close()


@gpu
def test_two_pipelines_forward_the_refusal():
    sc = K.soup_scene(1, 160, 120)
    ctx = make_context(sc, pipelines=2)
    calls = Calls(sc, ctx)
    grew = []
    for kind, reason, facts in (("filter", "DilationPadding", "PD"), ("learn", "BitsTwoKernel", "K"), ("points", "PointsThresh", "T")):
        refuse(calls, kind, reason, facts, grew)
    assert calls.untouched() == [] and grew == [], grew
    set_facts(ctx, sc, "")
    for _ in range(2):                         # (one batch per pipeline)
        masked, mask = ctx.filter_batch(sc.depth)
        K.compare_planes(masked, K.filter_expected(sc, 0)[0], "the batch after the refusals, two pipelines", "masked")
        K.compare_labels(mask, K.filter_expected(sc, 0)[1], "the batch after the refusals, two pipelines", "mask")
    ctx.close()
