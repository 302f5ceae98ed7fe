#!/usr/bin/env python3
"""Writes tests/golden/llvmpipe/random_scenes_320x240.npz: what the REFERENCE's GLSL shaders (read at run time from the
reference checkout, never copied) render on Mesa llvmpipe through oracle/ref_gl for the seeded scenes of
tests/test_oracle_vs_llvmpipe.py (tests/scenes.py: llvmpipe_scene).  Data only, per seed: the sha256 of the scene's inputs,
the mask bits and the sha256 of the masked depth; for the seeds of the stand-in check also the sha256 of all four colour
attachments.  Development container only (needs the reference checkout); the tests then run anywhere from the stored digests.

Run:  python tests/golden/generate_llvmpipe_scenes.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scenes as S  # noqa: E402
from oracle.ref_gl import harness as HN  # noqa: E402

W, H = 320, 240
SEEDS = range(100, 106)
ATTACHMENT_SEEDS = (100, 103, 105)
OUT = os.path.join(HERE, "llvmpipe", "random_scenes_%dx%d.npz" % (W, H))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def main():
    hn = HN.Harness(W, H, shaders="reference")
    fx = {"width": W, "height": H, "replace_value": np.float32(5.0), "renderer": np.frombuffer(hn.renderer().encode(), np.uint8)}
    for seed in SEEDS:
        P, depth, offinv, camtf, rend, draws = S.llvmpipe_scene(seed, W, H)
        masked, mask = hn.frame(depth, P, rend, offinv, camtf, replace_value=5.0)
        assert set(np.unique(mask)) <= {0, 255}
        fx["inputs_sha256_%d" % seed] = np.frombuffer(S.scene_digest(P, depth, offinv, camtf, draws), np.uint8)
        fx["mask_bits_%d" % seed] = np.packbits(mask > 0)
        fx["masked_sha256_%d" % seed] = sha(masked)
        if seed in ATTACHMENT_SEEDS:
            fx["attachments_sha256_%d" % seed] = np.stack([sha(hn.read_attachment(i)) for i in range(4)])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **fx)
    print("%s  %.1f KiB" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
