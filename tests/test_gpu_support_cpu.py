"""The GPU tests' support module (tests/gpu_support.py) on the CPU: the shared scene builders build the scenes the test modules
built for themselves before they were moved, and OracleScene computes what the separate scene classes did.

The digests below were taken from the builders as they stood in the test modules before the move (test_silhouette_dilation_gpu,
test_link_residuals_gpu, test_virtual_depth_gpu), by a script that imported those modules and hashed, stream by stream,
scenes.scene_digest over projection, sensor plane (zeros where the scene has none), offset, camera and oracle draws."""
import hashlib

import numpy as np
import pytest

import golden_io
import gpu_support as G
import scenes as S
from oracle import bindings as O

SCENES = {
    "soup_1_160x120": (lambda: G.soup_scene(1, 160, 120), "76aebf0e4e2f529f271ad099264298b8fdbb9ae7a92aa01144466f9d091a4207"),
    "soup_2_517x389_n2": (lambda: G.soup_scene(2, 517, 389, n=2), "ad33dda8a8b882e1097471f95adc3dfd0a154e9ac634d4f141b20b379d31df83"),
    "soup_31_160x120": (lambda: G.soup_scene(31, 160, 120), "b05a807c9d7f1760a4e273807075557dd86b8956500bf0f0b678966d4ef67a85"),
    "borders": (G.border_scene, "b3950678244d434060e0647f424e1fc5ffd2fa2e27da83915acf389b83586e21"),
    "neighbours": (G.neighbour_scene, "15b6d25a9c80e368be0c7bde0634dfe78b47d741105b544c2965bd6d2ed4d404"),
    "undrawn": (G.undrawn_scene, "1a47db0c0ae55040b7eba14b2b4c640180440445b1cf2aaa4ecdf82ff9ad1eef"),
    "fixture_near_range_ties_n2": (lambda: G.fixture_scene("near_range_ties_160x120", 2), "a35e31d9d7c1cd483f17990ad5ae13b2fa534d5f360188eca13cf5a902da9ac6"),
    "small_links": (G.small_links_scene, "fd811bb99b49da95ceb53b329df17edcbaefcaac2d3032e56a86d702768d5200"),
    "wall": (G.wall_scene, "7c90936efe2d1d2ea4cf3419c6c0e26816b9dfa3b0cb7948db7e6a2a40ea33ee"),
    "near_quad": (G.near_quad_scene, "6e0aacab6060f3eebdf0eff17cfd9c2bb3aa5d06d3f7978ae2fe0ca819cd845a"),
}


def digest(sc):
    wl = sc.wl
    h = hashlib.sha256()
    for s in range(sc.n):
        depth = np.zeros((sc.H, sc.W), np.float32) if sc.depth is None else sc.depth[s]
        h.update(S.scene_digest(wl.projection[s], depth, wl.offset_inv[s], wl.cam_tf[s], wl.oracle_draws(s)))
    return h.hexdigest()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_moved_builders_build_the_same_scenes(name):
    build, want = SCENES[name]
    assert digest(build()) == want


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("build", [lambda: G.soup_scene(1, 160, 120), G.undrawn_scene], ids=["soup_1_160x120", "undrawn"])
def test_the_threaded_oracle_run_equals_the_serial_one(build):
    sc = build()
    wl = sc.wl
    for s in range(sc.n):
        om, ok, zwin, prim, _ = O.filter_frame(sc.depth[s], wl.projection[s], wl.oracle_draws(s), wl.offset_inv[s], wl.cam_tf[s], z_near=wl.near,
                                               z_far=wl.far, max_diff=wl.max_diff, replace_value=wl.replace_value, want_debug=True)
        for got, want, what in ((sc.masked, om, "masked"), (sc.mask, ok, "mask"), (sc.zwin, zwin, "zwin"), (sc.prim, prim, "prim")):
            assert same_bits(got[s], want), "stream %d: %s" % (s, what)


def test_a_scene_without_sensor_planes_has_the_same_zwin_and_prim_and_no_masked():
    with_sensor = G.soup_scene(1, 160, 120)
    without = G.OracleScene(with_sensor.wl)
    assert same_bits(without.zwin, with_sensor.zwin) and same_bits(without.prim, with_sensor.prim)
    for plane in ("masked", "mask"):
        with pytest.raises(ValueError):
            getattr(without, plane)


def test_stream_0_of_a_fixture_scene_passes_the_fixtures_own_check():
    sc = G.fixture_scene("near_range_ties_160x120", 2)
    golden_io.Fixture("near_range_ties_160x120").check(sc.masked[0], sc.mask[0])
    assert not same_bits(sc.mask[0], sc.mask[1])          # (stream 1 looks from 2 cm to the side)


@pytest.mark.parametrize("W", [160, 517])
def test_unpack_bits_inverts_pack_bits(W):
    H = 9
    m = np.random.default_rng(W).random((3, H, W)) < 0.5
    bits = np.stack([G.pack_bits(x) for x in m])
    assert bits.dtype == np.uint32 and bits.shape == (3, H * ((W + 31) // 32))
    assert np.array_equal(G.unpack_bits(bits, W, H), m)
    assert np.array_equal(G.unpack_bits(bits[1], W, H), m[1])
