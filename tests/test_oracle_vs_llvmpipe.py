"""The oracle against the REAL reference shaders on Mesa llvmpipe, on seeded scenes that are not among the committed
fixtures.  What the reference's shaders render for them is stored as digests (tests/golden/llvmpipe/, written by
tests/golden/generate_llvmpipe_scenes.py in the development container), so the oracle is checked against it anywhere;
where the llvmpipe harness (oracle/_ref) and the reference checkout exist, the stored result is re-rendered live as well."""
import hashlib
import os

import numpy as np
import pytest

import scenes as S
from oracle import bindings as O
from oracle.ref_gl import harness as HN

W, H = 320, 240
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llvmpipe", "random_scenes_%dx%d.npz" % (W, H))

_hn = {}


def harness(w, h):
    if (w, h) not in _hn:
        if _hn:
            pytest.skip("one GL context size per process")
        _hn[(w, h)] = HN.Harness(w, h, shaders="reference" if HN.available("reference") else "standin")
    return _hn[(w, h)]


def stored(seed):
    """The reference's result for scene `seed`: (mask, sha256 of the masked depth, sha256 of the four attachments or None),
    after checking that tests/scenes.py still builds the inputs it was rendered from."""
    z = np.load(GOLDEN)
    P, depth, offinv, camtf, rend, draws = S.llvmpipe_scene(seed, W, H)
    assert S.scene_digest(P, depth, offinv, camtf, draws) == bytes(z["inputs_sha256_%d" % seed]), \
        "seed %d: tests/scenes.py no longer builds the scene the stored result was rendered from (tests/golden/generate_llvmpipe_scenes.py)" % seed
    mask = (np.unpackbits(z["mask_bits_%d" % seed])[: W * H].reshape(H, W) * 255).astype(np.uint8)
    att = "attachments_sha256_%d" % seed
    return mask, bytes(z["masked_sha256_%d" % seed]), ([bytes(x) for x in z[att]] if att in z.files else None)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


@pytest.mark.parametrize("seed", range(100, 106))
def test_random_scene_matches_llvmpipe(seed):
    P, depth, offinv, camtf, rend, draws = S.llvmpipe_scene(seed, W, H)
    g_mask, g_masked_sha, _ = stored(seed)
    if HN.available("reference"):
        masked, mask = harness(W, H).frame(depth, P, rend, offinv, camtf, replace_value=5.0)
        assert np.array_equal(mask, g_mask) and sha(masked) == g_masked_sha, "llvmpipe no longer renders the stored result"
    o_masked, o_mask = O.filter_frame(depth, P, draws, offinv, camtf, replace_value=5.0)
    assert (g_mask != o_mask).sum() == 0
    assert sha(o_masked) == g_masked_sha


@pytest.mark.skipif(not HN.available("standin"), reason="needs the llvmpipe harness: oracle/_ref (built by build() where Mesa's swrast_dri.so exists)")
def test_standin_shaders_render_exactly_what_the_reference_shaders_render():
    """oracle/ref_gl/standin_shaders/ (repo-authored; what bench.py's llvmpipe timing leg runs where the reference's files do
    not exist) against what the reference's own shader files render on the same scenes: all four colour attachments
    bit-identical -- so timing the stand-in is timing the reference's program.  The reference's side comes from the stored
    digests; where its files exist it is rendered live too, before and after the stand-in in the same GL context."""
    hn = harness(W, H)
    runs = ("reference", "standin", "reference") if HN.available("reference") else ("standin",)
    for shaders in runs:
        hn.use_shaders(shaders)
        for seed in (100, 103, 105):
            P, depth, offinv, camtf, rend, _ = S.llvmpipe_scene(seed, W, H)
            g_mask, g_masked_sha, g_att = stored(seed)
            masked, mask = hn.frame(depth, P, rend, offinv, camtf, replace_value=5.0)
            assert np.array_equal(mask, g_mask) and sha(masked) == g_masked_sha, "%s shaders, seed %d" % (shaders, seed)
            for i in range(4):
                assert sha(hn.read_attachment(i)) == g_att[i], "%s shaders: attachment %d, seed %d" % (shaders, i, seed)
    assert hn.shaders == runs[-1]
