"""bench.py --dump-outputs on the CPU: what bench.dump_outputs writes for a frame within the budget (the whole frame, float32) and
for a larger one (a seeded sample of pixels plus their flat indices, the same sample every run, within the budget)."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)           # only definitions run: the benchmark itself sits behind __main__
    return mod


def _frame(h, w, seed):
    return np.random.default_rng(seed).random((h, w, 4), dtype=np.float32)


def test_a_frame_within_the_budget_is_written_whole(tmp_path):
    bench = _bench()
    img = _frame(36, 64, 1)
    bench.dump_outputs(str(tmp_path / "out"), "radiance", img)
    assert os.listdir(str(tmp_path / "out")) == ["radiance.npy"]
    got = np.load(str(tmp_path / "out" / "radiance.npy"))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), img.view(np.uint32))


def test_a_larger_frame_is_sampled_the_same_way_every_run(tmp_path):
    bench = _bench()
    img = _frame(90, 160, 2)
    budget = img.nbytes // 5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "radiance", img, budget=budget)
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["radiance_sample.npy", "radiance_sample_pixel.npy"]
    sample = np.load(str(tmp_path / "a" / "radiance_sample.npy"))
    pixel = np.load(str(tmp_path / "a" / "radiance_sample_pixel.npy"))
    assert sample.dtype == np.float32 and pixel.dtype == np.float64
    assert sample.nbytes + pixel.nbytes <= budget and len(pixel) > 0.9 * budget / (16 + 8)
    idx = pixel.astype(np.int64)
    assert np.array_equal(idx, pixel) and np.all(np.diff(idx) > 0) and idx[-1] < 90 * 160
    assert np.array_equal(sample, img.reshape(-1, 4)[idx])
    for name in ("radiance_sample.npy", "radiance_sample_pixel.npy"):
        assert open(str(tmp_path / "a" / name), "rb").read() == open(str(tmp_path / "b" / name), "rb").read()
