#!/usr/bin/env python3
"""Writes tests/golden/llvmpipe/lattice_scenes_WxH.npz: what the REFERENCE's GLSL shaders (read at run time from the reference
checkout, never copied) render on Mesa llvmpipe through oracle/ref_gl for the lattice scenes of tests/lattice_scenes.py of one
frame size -- the tiny, small, records and tiles scenes at 1 m.  The sensor plane lies half a metre behind the geometry's
front layer, so the mask is the coverage.  A scene's triangles share their edges, so the mask of the whole scene shows only its
outline: every scene is also rendered one colour class (one link) at a time, which shows the pixels each class owns.
Data only, per scene and frame: the sha256 of the inputs, the mask bits and the sha256 of the masked depth.  Development
container only (needs the reference checkout); tests/test_fill_rule_llvmpipe.py then runs anywhere from the stored digests.

One frame size per process (the GL context has one size):
    python tests/golden/generate_llvmpipe_lattice.py 160 120
    python tests/golden/generate_llvmpipe_lattice.py 200 150
    python tests/golden/generate_llvmpipe_lattice.py 256 128
With --check nothing is written: the stored file is compared with what llvmpipe renders now.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lattice_scenes as L  # noqa: E402
import scenes as S  # noqa: E402

REPLACE, out_path, names, frames = L.LLVMPIPE_REPLACE, L.llvmpipe_path, L.llvmpipe_names, L.llvmpipe_frames


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def main():
    from oracle.ref_gl import harness as HN
    check = "--check" in sys.argv
    W, H = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    hn = HN.Harness(W, H, shaders="reference")
    fx = {"width": W, "height": H, "replace_value": np.float32(REPLACE), "renderer": np.frombuffer(hn.renderer().encode(), np.uint8)}
    for name in names(W, H):
        for key, P, depth, rend, draws in frames(name):
            masked, mask = hn.frame(depth, P, rend, L.IDENTITY, L.IDENTITY, z_near=L.NEAR, z_far=L.FAR, replace_value=REPLACE)
            assert set(np.unique(mask)) <= {0, 255}
            fx["inputs_sha256/" + key] = np.frombuffer(S.scene_digest(P, depth, L.IDENTITY, L.IDENTITY, draws), np.uint8)
            fx["mask_bits/" + key] = np.packbits(mask > 0)
            fx["masked_sha256/" + key] = sha(masked)
    if check:
        z = np.load(out_path(W, H))
        bad = [k for k in fx if k != "renderer" and not np.array_equal(z[k], fx[k])]
        assert not bad and set(z.files) == set(fx), bad
        print("%s: llvmpipe renders the stored result (%d arrays)" % (out_path(W, H), len(fx)))
        return
    os.makedirs(os.path.dirname(out_path(W, H)), exist_ok=True)
    np.savez_compressed(out_path(W, H), **fx)
    print("%s  %.1f KiB" % (out_path(W, H), os.path.getsize(out_path(W, H)) / 1024))


if __name__ == "__main__":
    main()
