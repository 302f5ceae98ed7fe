"""bench.py --dump-outputs without a GPU: what dump_outputs writes for a batch of outputs -- finite float32 / float64
arrays only (NaN / inf outputs as a class array beside the depth), within the size limit, every stream where they fit
and otherwise the same seeded sample every time."""
import os

import numpy as np

import bench


def fake_outputs(n, H, W, seed=3):
    rng = np.random.default_rng(seed)
    masked = rng.random((n, H, W), dtype=np.float32)
    mask = (rng.random((n, H, W)) < 0.3).astype(np.uint8)
    return masked, mask


def load(d, names):
    return {name[:-4]: np.load(os.path.join(d, name)) for name in names}


def test_small_batch_is_dumped_whole(tmp_path):
    masked, mask = fake_outputs(5, 12, 16)
    names = bench.dump_outputs(str(tmp_path), masked, mask)
    assert names == ["mask.npy", "masked_depth.npy", "masked_depth_nonfinite.npy", "streams.npy"]
    got = load(str(tmp_path), names)
    assert got["masked_depth"].dtype == np.float32 and np.array_equal(got["masked_depth"].view(np.uint32), masked.view(np.uint32))
    assert got["mask"].dtype == np.float32 and np.array_equal(got["mask"], mask.astype(np.float32))
    assert got["streams"].dtype == np.float64 and np.array_equal(got["streams"], np.arange(5))


def test_without_mask_and_16uc1_values(tmp_path):
    masked = np.array([[[0, 1], [65535, 1234]]], dtype=np.uint16)
    names = bench.dump_outputs(str(tmp_path), masked, None)
    assert names == ["masked_depth.npy", "streams.npy"]          # (16UC1 output is never NaN / inf: no class array)
    got = load(str(tmp_path), names)
    assert got["masked_depth"].dtype == np.float32 and np.array_equal(got["masked_depth"], masked.astype(np.float32))


def test_large_batch_is_a_fixed_sample_within_the_limit(tmp_path):
    n, H, W = 40, 480, 640            # 98 MB of masked depth + mask as float32
    masked, mask = fake_outputs(n, H, W)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    names = bench.dump_outputs(a, masked, mask)
    assert bench.dump_outputs(b, masked, mask) == names
    total = sum(os.path.getsize(os.path.join(a, x)) for x in names)
    assert total <= 64_000_000
    got, again = load(a, names), load(b, names)
    streams = got["streams"].astype(np.int64)
    assert 1 <= len(streams) < n and np.all(np.diff(streams) > 0) and streams[-1] < n
    assert np.array_equal(got["streams"], again["streams"])
    assert np.array_equal(got["masked_depth"], masked[streams]) and np.array_equal(got["mask"], mask[streams].astype(np.float32))


def test_nan_and_inf_outputs_are_dumped_as_finite_classes(tmp_path):
    """Unfiltered pixels carry the sensor's value, NaN and inf included: every dumped value is finite, and the depth plus
    its class array give back the output exactly."""
    masked, mask = fake_outputs(3, 8, 10)
    masked[0, 1, 2], masked[1, 3, 4], masked[2, 5, 6], masked[2, 7, 9] = np.nan, np.inf, -np.inf, np.nan
    names = bench.dump_outputs(str(tmp_path), masked, mask)
    got = load(str(tmp_path), names)
    for name, a in got.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    cls = got["masked_depth_nonfinite"]
    assert cls[0, 1, 2] == 1 and cls[1, 3, 4] == 2 and cls[2, 5, 6] == 3 and cls[2, 7, 9] == 1 and (cls != 0).sum() == 4
    back = got["masked_depth"].copy()
    back[cls == 1], back[cls == 2], back[cls == 3] = np.nan, np.inf, -np.inf
    assert np.array_equal(back, masked, equal_nan=True)
    assert np.array_equal(got["masked_depth"][cls == 0], masked[np.isfinite(masked)])


def test_frame_larger_than_the_limit_is_a_fixed_pixel_sample(tmp_path, monkeypatch):
    """Where one frame alone is over the limit, a seeded sample of one stream's pixels -- still within the limit."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    n, H, W = 4, 100, 200                 # 3 float32 planes of one frame: 240 kB, over the 200 kB limit
    masked, mask = fake_outputs(n, H, W)
    masked[1, 0, :] = np.nan
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    names = bench.dump_outputs(a, masked, mask)
    assert names == ["mask.npy", "masked_depth.npy", "masked_depth_nonfinite.npy", "pixels.npy", "streams.npy"]
    assert bench.dump_outputs(b, masked, mask) == names
    assert sum(os.path.getsize(os.path.join(a, x)) for x in names) <= 200_000
    got, again = load(a, names), load(b, names)
    for name in names:
        key = name[:-4]
        assert np.isfinite(got[key]).all() and np.array_equal(got[key], again[key]), name
    s, px = int(got["streams"][0]), got["pixels"].astype(np.int64)
    assert got["streams"].shape == (1,) and 0 <= s < n and 0 < len(px) < H * W and np.all(np.diff(px) > 0)
    want = masked[s].reshape(-1)[px]
    assert got["masked_depth"].shape == (1, len(px))
    assert np.array_equal(got["masked_depth"][0][np.isfinite(want)], want[np.isfinite(want)])
    assert np.array_equal(got["masked_depth_nonfinite"][0] == 1, np.isnan(want))
    assert np.array_equal(got["mask"][0], mask[s].reshape(-1)[px].astype(np.float32))
