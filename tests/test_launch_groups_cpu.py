"""CPU (-m "not gpu"): the launch groups a batch is split into, and the counter blocks that hold one block per group.

Every rtuf_filter_batch* entry accepts 1 <= n <= max_streams streams, and the device writes one counter block per launch
group that the host reads back.  The number of groups is not monotone in n (3 lanes, groups of 8 streams: 48 streams make 6
groups, 49 make 9), so the blocks are sized by a bound over every n, not by what a full batch makes.
tests/launch_groups_check.cpp runs the library's own functions (rtuf_groups.h) for every lane count up to 8, launch group up
to 1024 and max_streams up to 4096 (33.5 M cases, < 1 s)."""
import os
import subprocess

import pytest

import enqueue_steps as ES
import launch_groups as LG

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "realtime_urdf_filter_amd", "csrc")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_groups") / "launch_groups_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(HERE, "launch_groups_check.cpp")])
    return exe


def test_counter_blocks_bound_every_partial_batch(check):
    r = subprocess.run([check], capture_output=True, text=True, timeout=300)
    print(r.stdout.strip())
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) == 8 * 1024 * 4096


def test_the_check_finds_the_old_bound_short(check):
    """Against the bound the library used before (groups_for(max_streams)) the same check must report the partial batches
    that made more groups than a full one -- the device wrote past the counter blocks, the host read past pinned memory."""
    r = subprocess.run([check, "old"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    for line in ("lanes 3 group 8 max_streams 64: n 49 makes 9 groups, counter blocks 8",
                 "lanes 2 group 5 max_streams 33: n 32 makes 8 groups, counter blocks 7"):
        assert line in r.stdout, r.stdout
    assert int(r.stdout.split("violations ")[1]) > 0
    # the count of a brute force over lanes 2-4, group <= 64, max_streams <= 256 with the Python form of the rule
    r = subprocess.run([check, "old", "4", "64", "256"], capture_output=True, text=True, timeout=60)
    want = 0
    for lanes in range(1, 5):
        for group in range(1, 65):
            most = 0
            for m in range(1, 257):
                most = max(most, LG.groups_for(m, group, lanes))
                want += most > LG.groups_for(m, group, lanes)
    assert want == 907 and r.stdout.strip().endswith("violations %d" % want), r.stdout


@pytest.mark.parametrize("lanes,group,max_streams,n,groups", [
    (3, 8, 64, 49, 9), (3, 6, 64, 56, 12), (3, 8, 128, 121, 18), (2, 8, 72, 65, 10), (2, 5, 33, 32, 8), (3, 8, 64, 48, 6)])
def test_the_issue_table(lanes, group, max_streams, n, groups):
    """The partial batches that overran the old counter blocks, in the Python form the GPU tests use."""
    assert LG.groups_for(n, group, lanes) == groups
    assert LG.groups_for(n, group, lanes) <= LG.counter_blocks_for(max_streams, group, lanes)


def test_the_library_takes_the_rule_from_the_shared_header():
    """One body of the rule: rtuf_api.cpp calls rtuf_groups.h and keeps no copy, and sizes the counter blocks by the bound."""
    api = open(os.path.join(CSRC, "rtuf_api.cpp")).read()
    assert '#include "rtuf_groups.h"' in api
    assert "static int groups_for(const rtuf_context* c, int n) { return rtuf::groups_for(n, c->group, c->n_lanes); }" in api
    assert "c->max_groups = rtuf::counter_blocks_for(c->max_streams, c->group, c->n_lanes);" in api
    assert "kSplitMin = " not in api and "c->n_lanes) * c->n_lanes" not in api
    # the hard stop comes before the first change to the context or the batch slot: before every step of enqueue_batch, and
    # the changes stand in those steps (enqueue_steps.py)
    assert ES.CHECKS[0] == "if (n_groups > c->max_groups)"
    ES.assert_checks_precede_every_change(api)
