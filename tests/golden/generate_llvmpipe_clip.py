#!/usr/bin/env python3
"""Writes tests/golden/llvmpipe/clip_scenes_WxH.npz: what the REFERENCE's GLSL shaders (read at run time from the reference
checkout, never copied) render on Mesa llvmpipe through oracle/ref_gl for the clip scenes of tests/clip_scenes.py of one frame
size -- triangles across every frustum plane and corner, on exact ties, behind the eye, and the levers whose clipped
vertices land outside the frame.  Every scene is rendered whole, one link at a time (`many` whole only) and whole once more
under a sensor plane that lies on the depth threshold of every pixel, where one ulp of z flips the mask.
Data only, per scene and frame: the sha256 of the inputs, the mask bits and the sha256 of the masked depth -- one row per
frame in three arrays, with the frames' keys in a fourth (hundreds of small arrays would triple the file).  Development
container only (needs the reference checkout); tests/test_clip_scenes_cpu.py then runs anywhere from the stored digests.

One frame size per process (the GL context has one size):
    python tests/golden/generate_llvmpipe_clip.py 160 120
    python tests/golden/generate_llvmpipe_clip.py 256 128
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

import clip_scenes as C  # noqa: E402
import scenes as S  # noqa: E402

REPLACE, out_path, names, frames = C.LLVMPIPE_REPLACE, C.llvmpipe_path, C.llvmpipe_names, C.llvmpipe_frames


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def main():
    from oracle.ref_gl import harness as HN
    check = "--check" in sys.argv
    W, H = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    hn = HN.Harness(W, H, shaders="reference")
    rows = []
    for name in names(W, H):
        for key, P, depth, offinv, camtf, rend, draws in frames(name):
            masked, mask = hn.frame(depth, P, rend, offinv, camtf, z_near=C.NEAR, z_far=C.FAR, replace_value=REPLACE)
            assert set(np.unique(mask)) <= {0, 255}
            rows.append((key, np.frombuffer(S.scene_digest(P, depth, offinv, camtf, draws), np.uint8), np.packbits(mask > 0), sha(masked)))
    fx = {"width": W, "height": H, "replace_value": np.float32(REPLACE), "renderer": np.frombuffer(hn.renderer().encode(), np.uint8),
          "keys": np.frombuffer("\n".join(r[0] for r in rows).encode(), np.uint8), "inputs_sha256": np.stack([r[1] for r in rows]),
          "mask_bits": np.stack([r[2] for r in rows]), "masked_sha256": np.stack([r[3] for r in rows])}
    if check:
        z = np.load(out_path(W, H))
        bad = [k for k in fx if k != "renderer" and not np.array_equal(z[k], fx[k])]
        assert not bad and set(z.files) == set(fx), bad
        print("%s: llvmpipe renders the stored result (%d frames)" % (out_path(W, H), len(rows)))
        return
    os.makedirs(os.path.dirname(out_path(W, H)), exist_ok=True)
    np.savez_compressed(out_path(W, H), **fx)
    print("%s  %.1f KiB" % (out_path(W, H), os.path.getsize(out_path(W, H)) / 1024))


if __name__ == "__main__":
    main()
