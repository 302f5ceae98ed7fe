"""CPU: the link label expectation (bench_support/labels_check.py) and the label entry points' place in the ABI."""
import os

import numpy as np

import golden_io
from bench_support import workloads as WL
from bench_support.labels_check import default_link_labels, expected_labels, prim_labels, workload_draws
from oracle import bindings as O
import realtime_urdf_filter_amd as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtuf.h")


def test_prims_map_through_draws_and_links():
    # three draws of 2, 0 and 3 triangles
    assert prim_labels([4, 9, 7], [2, 0, 3]).tolist() == [4, 4, 7, 7, 7]
    prim = np.array([[-2, -1, 0], [1, 2, 4]], np.int32)
    assert expected_labels(prim, [4, 9, 7], [2, 0, 3]).tolist() == [[0, 0, 4], [4, 7, 7]]


def test_default_labels_number_links_over_all_models():
    wl = WL.Workload("two models", 8, 8, 1)

    class D:
        def __init__(self, n):
            self.tris = np.zeros((n, 3), np.uint32)
    wl.models = [[[D(2)], [D(1), D(3)]], [[D(5)]]]          # model 0: links 0 (one draw), 1 (two draws); model 1: link 0
    assert default_link_labels(3).tolist() == [1, 2, 3]
    assert workload_draws(wl) == ([1, 2, 2, 3], [2, 1, 3, 5])
    assert workload_draws(wl, [0, 6, 6]) == ([0, 6, 6, 6], [2, 1, 3, 5])


def test_expectation_on_a_fixture_is_drawn_exactly_where_the_oracle_drew():
    fx = golden_io.Fixture("example_urdf_160x120")
    _, _, _, prim, _ = O.filter_frame(fx.depth, fx.projection, fx.draws, fx.offset_inv, fx.cam_tf, z_near=fx.z_near,
                                      z_far=fx.z_far, max_diff=fx.max_diff, replace_value=fx.replace_value, want_debug=True)
    lab = expected_labels(prim, np.arange(1, len(fx.draws) + 1), [len(d[4]) for d in fx.draws])
    assert ((lab > 0) == (prim >= 0)).all() and (lab > 0).any()
    assert set(np.unique(lab)) <= set(range(len(fx.draws) + 1))


def test_label_entry_points_are_declared_and_bound():
    text = open(HEADER).read()
    for name in ("rtuf_set_link_labels", "rtuf_filter_batch_device_labels", "rtuf_filter_batch_device_u16_labels",
                 "rtuf_filter_batch_labels", "rtuf_filter_batch_u16_labels"):
        assert name + "(" in text and name in R._capi.SYMBOLS, name
    for name in ("filter_batch_labels", "filter_batch_device_labels", "set_link_labels", "num_links"):
        assert callable(getattr(R.Context, name)), name
