"""bench.py --dump-outputs: the state the timed steps leave is the same from run to run (CPU part:
the option plumbing; GPU part: two runs of the plain benchmark path in this process)."""
import argparse
import glob
import os

import numpy as np
import pytest
import torch


def _args(tmp, **kw):
    base = dict(config="d4ic", steps=3, warmup=2, preheat_s=0.05, full=False, dump_outputs=str(tmp), replicas=1,
                fit_replicas=0, ref_grid_epochs=0, c5_steps=0, dp_leg_batch=0, no_cpu_baseline=True,
                no_kernel_times=True, no_north_star=True)
    base.update(kw)
    return argparse.Namespace(**base)


def _load(d):
    return dict((os.path.basename(f), np.load(f)) for f in sorted(glob.glob(os.path.join(str(d), "*.npy"))))


@pytest.mark.gpu
def test_dumped_outputs_repeat_and_do_not_depend_on_the_preheat(tmp_path):
    """Two plain runs with a (clock-dependent) preheat and one without it write bit-identical
    arrays: every state_dict entry and the Adam moments, float32 / float64, and they are the state
    of W + K steps (the Adam step counters say so), and the line keeps its headline fields."""
    import bench
    dev = torch.device("cuda", 0)
    runs = []
    for name, pre in (("a", 0.05), ("b", 0.05), ("c", 0.0)):
        a = _args(tmp_path / name, preheat_s=pre)
        out = bench.mode_fit(a, dev, 0, 1, None, {"dist": None})
        assert out["steps"] == 3 and out["warmup"] == 2 and out["full"] is False
        assert out["ms_per_step"] > 0 and abs(out["value"] - 128 * 1e3 / out["ms_per_step"]) <= 2e-3 * out["value"]
        for k in ("metric", "unit", "higher_is_better", "dtype"):
            assert k in out
        assert out["grid_search"] is None and out["north_star_config"] is None and "cpu_baseline" not in out
        runs.append(_load(tmp_path / name))
    c = bench.CONFIGS["d4ic"]
    m = bench.build_model(__import__("redcliff_amd").REDCLIFF_S_CMLP_withStateSmoothing, c, seed=0)
    want = set(k + ".npy" for k in m.state_dict()) | set(
        "adam_%s.%s.npy" % (g, k) for g in "AB" for k in ("exp_avg", "exp_avg_sq"))
    assert set(runs[0]) == want
    changed = 0
    for k, v in runs[0].items():
        assert v.dtype in (np.float32, np.float64) and np.all(np.isfinite(v)), k
        for other in runs[1:]:
            np.testing.assert_array_equal(v, other[k], err_msg=k)
        key = k[:-4]
        if key in m.state_dict() and m.state_dict()[key].dtype.is_floating_point:
            changed += int(not np.array_equal(v, m.state_dict()[key].numpy()))
    assert changed > 0  # the steps really trained the dumped model
    nbt = [v for k, v in runs[0].items() if k.endswith("num_batches_tracked.npy")]
    assert nbt and all(v.dtype == np.float64 for v in nbt)
    assert sum(v.nbytes for v in runs[0].values()) <= bench.DUMP_BYTES


def test_dump_sampling_is_fixed_and_bounded(tmp_path, monkeypatch):
    """Above DUMP_BYTES every large array is cut to a fixed seeded sample (CPU: a stand-in engine)."""
    import bench

    class Eng:
        opt = {"A": None, "B": None}

        class model:
            @staticmethod
            def state_dict():
                g = torch.Generator().manual_seed(1)
                return {"big": torch.randn(50000, generator=g), "small": torch.arange(10, dtype=torch.int64)}

    monkeypatch.setattr(bench, "DUMP_BYTES", 100000)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    bench.dump_outputs(str(tmp_path / "x"), Eng)
    bench.dump_outputs(str(tmp_path / "y"), Eng)
    x, y = _load(tmp_path / "x"), _load(tmp_path / "y")
    assert sum(v.nbytes for v in x.values()) <= 100000
    assert x["small.npy"].dtype == np.float64 and x["small.npy"].shape == (10,)
    assert x["big.npy"].dtype == np.float32 and 4096 <= x["big.npy"].size < 50000
    full = Eng.model.state_dict()["big"].numpy()
    assert np.isin(x["big.npy"], full).all()
    for k in x:
        np.testing.assert_array_equal(x[k], y[k])
