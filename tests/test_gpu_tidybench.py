"""SLARAC and QRBS on the device (csrc/rc_tidybench.hip through redcliff_tidybench_run) against the reference's
outputs in tests/golden/tidybench.npz under the bound of tests/tidybench_common.py, plus the properties of the
call itself: the pivot rule's statuses, determinism, batch independence, grouping under a small workspace budget
and the shape limits."""
import functools

import numpy as np
import pytest
import torch

import tidybench_common as C
from redcliff_amd import tidybench as tb

pytestmark = pytest.mark.gpu

CASES = [(n, a) for n in C.NAMES for a in C.algs(C.META[n])]


@functools.lru_cache(maxsize=None)
def device_run(name, alg):
    sc = C.scenario(name)
    out, info = C.call(tb, sc, alg, path="fused")
    return sc, out, info, float(np.random.rand())


@pytest.mark.parametrize("name,alg", CASES)
def test_device_route_matches_reference(name, alg):
    sc, raw, info, nxt = device_run(name, alg)
    C.check_scores(sc, alg, raw, "raw", "device")
    assert nxt == sc[alg]["next_rand"]
    # the device hands to the host exactly the fits the pivot rule names, and no others; NONFINITE never shows
    assert np.array_equal(info["status"], C.predicted_status(sc, alg))
    assert info["n_host_solved"] == sc[alg]["singular"]
    assert (info["status"] != tb.NONFINITE).all()
    ok = info["status"] == tb.OK
    assert np.allclose(info["pivot_ratio"][ok], sc["%s_pivot" % alg][ok], rtol=1e-6, atol=0)
    assert set(info["time"]) == {"draws", "upload", "kernels", "fallback", "aggregate", "total"}
    std, _ = C.call(tb, sc, alg, path="fused", post_standardise=True)
    C.check_scores(sc, alg, std, "std", "device")


@pytest.mark.parametrize("name", C.NAMES)
def test_per_fit_coefficients(name):
    """An error in single fits that the average over 201 fits would hide."""
    sc, _, info, _ = device_run(name, "slarac")
    C.check_coef(sc, info, "device", rtol=1e-12)


def test_mixed_share_of_host_solved_fits():
    sc, _, info, _ = device_run("mixed", "slarac")
    assert (info["status"] == tb.SINGULAR).sum(axis=1).tolist() == sc["slarac"]["singular_per_regime"]


@pytest.mark.parametrize("name,alg", [("pub12", "slarac"), ("pub12", "qrbs"), ("lags3", "slarac"), ("lags3", "qrbs")])
def test_two_runs_and_device_input_give_the_same_bits(name, alg):
    sc, raw, info, _ = device_run(name, alg)
    again, i2 = C.call(tb, sc, alg, path="fused")
    assert np.array_equal(raw, again) and np.array_equal(info["coef"], i2["coef"])
    assert np.array_equal(info["pivot_ratio"], i2["pivot_ratio"])
    keep = sc["series"].copy()
    dev, i3 = C.call(tb, sc, alg, series=torch.from_numpy(sc["series"]).cuda(), path="fused")
    assert np.array_equal(raw, dev) and np.array_equal(info["coef"], i3["coef"]) and np.array_equal(keep, sc["series"])


@pytest.mark.parametrize("name,alg", [("pub12", "slarac"), ("pub12", "qrbs"), ("lags3", "slarac"), ("mixed", "slarac")])
def test_a_data_set_alone_equals_it_inside_many(name, alg):
    """Regime 0 alone draws what it draws first inside the batch: its fits and scores are the same bits."""
    sc, raw, info, _ = device_run(name, alg)
    one, i1 = C.call(tb, sc, alg, path="fused", single=0)
    assert np.array_equal(one, raw[0]) and np.array_equal(i1["coef"], info["coef"][0])
    assert np.array_equal(i1["status"], info["status"][0]) and np.array_equal(i1["pivot_ratio"], info["pivot_ratio"][0])


@pytest.mark.parametrize("name,alg", [("pub12", "slarac"), ("pub12", "qrbs"), ("lags3", "qrbs")])
def test_a_small_workspace_budget_runs_groups_with_the_same_bits(name, alg, monkeypatch):
    sc, raw, info, _ = device_run(name, alg)
    assert info["groups"] == 1
    monkeypatch.setattr(tb, "WORKSPACE_BUDGET_BYTES", 40 << 10)
    got, i2 = C.call(tb, sc, alg, path="fused")
    assert i2["groups"] >= 3
    assert np.array_equal(got, raw) and np.array_equal(i2["coef"], info["coef"])
    assert np.array_equal(i2["status"], info["status"]) and np.array_equal(i2["pivot_ratio"], info["pivot_ratio"])


def test_just_outside_each_limit_takes_the_host_route(monkeypatch):
    from redcliff_amd import _native as nat
    L = nat.lib()
    assert L.redcliff_tidybench_supported(200, 32, 3) == 1
    assert L.redcliff_tidybench_supported(200, 33, 1) == 0 and b"limits" in L.redcliff_last_error()
    assert L.redcliff_tidybench_supported(200, 24, 4) == 1
    assert L.redcliff_tidybench_supported(200, 25, 4) == 0     # lags N = 100 > 96
    assert L.redcliff_tidybench_supported(200, 1, 97) == 0
    assert L.redcliff_tidybench_supported(3, 4, 3) == 0        # T <= lags
    assert L.redcliff_tidybench_ws_bytes(2, 5, 33, 1, 100) == 0
    assert L.redcliff_tidybench_ws_bytes(2, 5, 10, 1, 1024) >= 8 * 2 * 5 * 2 * (66 + 110)
    monkeypatch.delenv("REDCLIFF_TIDYBENCH_PATH", raising=False)
    rng = np.random.RandomState(5)
    np.random.seed(1)
    out, info = tb.slarac(rng.randn(120, 33), n_subsamples=2, return_info=True)
    assert info["route"] == "host" and np.isfinite(out).all()
    np.random.seed(1)
    out, info = tb.qrbs(rng.randn(300, 25), lags=4, n_resamples=2, return_info=True)
    assert info["route"] == "host" and np.isfinite(out).all()
    np.random.seed(1)
    out, info = tb.slarac(rng.randn(120, 32), n_subsamples=2, return_info=True)
    assert info["route"] == "fused" and np.isfinite(out).all()


def test_limit_shape_against_the_host_route():
    """N = 32 with lags = 3: the widest rows, 31 entries per lane and one wavefront per workgroup in the solve.
    Both routes are within 64 eps n_max kappa of the exact solution, kappa from numpy on the same draws."""
    rng = np.random.RandomState(6)
    x = rng.randn(1, 700, 32)
    sc = dict(seed=8, lags=3, n_subsamples=3, n_resamples=3, series=x, name="limit")
    for alg in ("slarac", "qrbs"):
        np.random.seed(8)
        plan = tb._slarac_plan(1, 700, 32, 3, 3, tb.DEFAULT_SUBSAMPLE_SIZES) if alg == "slarac" else tb._qrbs_plan(1, 700, 32, 3, 3)
        kap, ratio, n_max = C.analyse(tb, x, plan, 0.005)
        assert (ratio > 1e-5).all()
        dev, i1 = C.call(tb, sc, alg, path="fused")
        host, i2 = C.call(tb, sc, alg, path="host")
        assert (i1["status"] == tb.OK).all() and (i2["status"] == tb.OK).all()
        err, bound = np.abs(dev - host).max(), 2 * 64 * C.EPS * n_max * kap.max() * np.abs(host).max()
        print("limit %s: device - host %.3e bound %.3e" % (alg, err, bound))
        assert err <= bound


def test_non_finite_input_raises_on_the_device_route(monkeypatch):
    monkeypatch.setenv("REDCLIFF_TIDYBENCH_PATH", "fused")
    x = C.scenario("tiny_l1")["series"][0].copy()
    x[5, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        tb.qrbs(torch.from_numpy(x).cuda())


def test_run_tidybench_experiment_on_the_device(monkeypatch):
    monkeypatch.setenv("REDCLIFF_TIDYBENCH_PATH", "fused")
    sc = C.scenario("exp6")
    samples = [(x, y) for x, y in zip(sc["x"], sc["y"])]
    for alg in ("slarac", "qrbs"):
        np.random.seed(sc["seed"])
        preds = tb.run_tidybench_experiment(samples, alg)
        for r, p in enumerate(preds):
            ref = sc[alg + "_preds"][r]
            assert np.abs(p - ref).max() <= sc[alg]["tol"] * np.abs(ref).max()
