"""The oracle against the REAL reference shaders on Mesa llvmpipe on the lattice scenes: exact ties of the fill rule.

tests/golden/llvmpipe/lattice_scenes_WxH.npz (written by tests/golden/generate_llvmpipe_lattice.py in the development
container) holds what llvmpipe renders for the tiny, small, records and tiles scenes -- the whole scene, and every colour class
alone, whose mask is the set of pixels that class's triangles own.  The oracle must give the same mask and the same masked
depth, and the integer rasteriser of tests/fill_rule.py the same coverage.  (Nothing is rendered here: the GL context of a
process has one size, and tests/test_oracle_vs_llvmpipe.py owns it; the generator's --check renders the stored result anew.)"""
import hashlib

import numpy as np
import pytest

import fill_rule
import lattice_scenes as L
import scenes as S
from oracle import bindings as O

_stored = {}


def stored(W, H):
    if (W, H) not in _stored:
        _stored[(W, H)] = np.load(L.llvmpipe_path(W, H))
    return _stored[(W, H)]


NAMES = [n for W, H in L.FRAMES for n in L.llvmpipe_names(W, H)]


def test_every_scene_of_every_kind_is_stored():
    for W, H in L.FRAMES:
        z = stored(W, H)
        kinds = {L.kind_of(n) for n in L.llvmpipe_names(W, H)}
        assert kinds >= {"tiny", "small", "records"} and (("tiles" in kinds) == ((W, H) != (160, 120)))
        keys = {"inputs_sha256/" + k for n in L.llvmpipe_names(W, H) for k, *_ in L.llvmpipe_frames(n)}
        assert keys == {f for f in z.files if f.startswith("inputs_sha256/")}
        assert b"llvmpipe" in bytes(z["renderer"])


@pytest.mark.parametrize("name", NAMES)
def test_lattice_scene_matches_llvmpipe(name):
    sc = L.scene(name)
    z = stored(sc.W, sc.H)
    winner = L.reference(name)[0]
    front = np.asarray(sc.zs)[np.maximum(winner, 0)] == min(sc.zs)
    n_frames = 0
    for key, P, depth, rend, draws in L.llvmpipe_frames(name):
        assert S.scene_digest(P, depth, L.IDENTITY, L.IDENTITY, draws) == bytes(z["inputs_sha256/" + key]), \
            "%s: tests/lattice_scenes.py no longer builds the scene the stored result was rendered from (tests/golden/generate_llvmpipe_lattice.py)" % key
        g_mask = np.unpackbits(z["mask_bits/" + key])[: sc.W * sc.H].reshape(sc.H, sc.W) * np.uint8(255)
        o_masked, o_mask = O.filter_frame(depth, P, draws, L.IDENTITY, L.IDENTITY, z_near=L.NEAR, z_far=L.FAR, replace_value=L.LLVMPIPE_REPLACE)
        assert (g_mask != o_mask).sum() == 0, key
        assert hashlib.sha256(np.ascontiguousarray(o_masked).tobytes()).digest() == bytes(z["masked_sha256/" + key]), key
        # ... and the integer rule: the front layer's coverage; of one colour class alone, the pixels its triangles cover
        if key.endswith("/all"):
            want = (winner >= 0) & front
        else:
            link = int(key.rsplit("link", 1)[1])
            want = np.zeros((sc.H, sc.W), bool)
            for t in np.flatnonzero((sc.colours() == link) & (np.asarray(sc.zs) == min(sc.zs))):
                got = fill_rule.triangle_coverage(sc.tris[t], sc.W, sc.H)
                if got is not None:
                    want[got[1]:got[1] + got[2].shape[0], got[0]:got[0] + got[2].shape[1]] |= got[2]
        assert np.array_equal(g_mask > 0, want), key
        n_frames += 1
    assert n_frames >= 5
