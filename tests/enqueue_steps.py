"""The source check two CPU tests share: enqueue_batch (rtuf_api.cpp) is the list of its steps, and nothing of the context or
the batch slot changes before its checks -- the hard stop on the launch groups, the route request and the route's refusal.

enqueue_batch calls one function per step.  So "the checks come before the first change" reads: within enqueue_batch's body
the checks precede the first call of every step function; each statement that marks such a change stands in the body of a step
function, and where one stands in enqueue_batch itself it comes behind the checks; and every step function is called from
enqueue_batch and from nowhere else, so no other path reaches those statements around the checks."""
import re

# the steps, in the order enqueue_batch calls them
STEPS = ("claim_lanes_and_timing", "upload_staged_poses", "build_plan", "launch_plan")
# the first changes a batch makes: to its slot's lanes, the context's lane counter, timing sequence and slot, and the uploads
MARKERS = ("b.lanes_used = 0;", "c->next_lane", "c->timing_seq++", "c->last_slot =", "hipMemcpyAsync")
CHECKS = ("if (n_groups > c->max_groups)", "route_of(", "if (!route.ok() || !tile_variant_legal(route.tile))\n    return c->fail(RTUF_ERR_STATE")


def body(src, head):
    """The text of the function that starts with `head`, up to the closing brace in column 0."""
    start = src.index(head)
    return src[start:src.index("\n}\n", start)]


def step_head(api, step):
    heads = re.findall(r"^static (?:int|void) %s\(" % step, api, re.M)
    assert len(heads) == 1, (step, heads)
    return heads[0]


def assert_checks_precede_every_change(api):
    enqueue = body(api, "static int enqueue_batch(")
    checked = max(enqueue.index(c) for c in CHECKS)      # (ValueError: a check is gone)
    step_bodies = {s: body(api, step_head(api, s)) for s in STEPS}
    for step in STEPS:
        call = step + "("
        # called from enqueue_batch, behind the checks, and from nowhere else (the other occurrence is its definition)
        assert enqueue.count(call) == 1 and enqueue.index(call) > checked, step
        assert api.count(call) == 2, (step, api.count(call))
    for m in MARKERS:
        assert any(m in b for b in step_bodies.values()), m
        if m in enqueue:
            assert enqueue.index(m) > checked, m
    # ... and between the last check and the first step nothing is assigned to a member of the context or the slot
    between = enqueue[checked:enqueue.index(STEPS[0] + "(")]
    assert "c->fail(" in between and not re.search(r"(\bc->\w+|\bb\.\w+)\s*(=[^=]|\+\+|--|\|=|\+=)", between), between
