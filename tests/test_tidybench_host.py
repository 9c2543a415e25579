"""SLARAC and QRBS on the host route (redcliff_amd/tidybench.py) against the reference's outputs in
tests/golden/tidybench.npz, under the bound of tests/tidybench_common.py, plus the contract of the public calls:
the generator's state after a call, the regime-aware driver, the errors, and that the input is left alone."""
import functools

import numpy as np
import pytest

import tidybench_common as C
from redcliff_amd import tidybench as tb

CASES = [(n, a) for n in C.NAMES for a in C.algs(C.META[n])]


@functools.lru_cache(maxsize=None)
def host_run(name, alg, std):
    sc = C.scenario(name)
    out, info = C.call(tb, sc, alg, post_standardise=std)
    return sc, out, info, float(np.random.rand())


@pytest.mark.parametrize("name,alg", CASES)
def test_many_matches_reference_and_leaves_the_generator_where_the_reference_does(name, alg):
    sc, raw, info, nxt = host_run(name, alg, False)
    C.check_scores(sc, alg, raw, "raw", "host")
    assert nxt == sc[alg]["next_rand"]
    assert np.array_equal(info["status"], C.predicted_status(sc, alg))
    assert info["n_host_solved"] == sc[alg]["singular"]
    _, std, _, nxt = host_run(name, alg, True)
    C.check_scores(sc, alg, std, "std", "host")
    assert nxt == sc[alg]["next_rand"]


@pytest.mark.parametrize("name,alg", [c for c in CASES if c[0] in ("tiny_l1", "tiny_l2", "pub12", "lags3")])
def test_single_call_equals_the_first_problem(name, alg):
    sc, raw, info, _ = host_run(name, alg, False)
    one, i1 = C.call(tb, sc, alg, single=0)
    assert one.shape == (sc["N"], sc["N"]) and np.array_equal(one, raw[0])
    assert np.array_equal(i1["status"], info["status"][0]) and i1["pivot_ratio"].shape == info["pivot_ratio"][0].shape
    C.check_scores(sc, alg, one[None], "raw", "host single", regimes=[0])


@pytest.mark.parametrize("name", C.NAMES)
def test_per_fit_coefficients(name):
    sc, _, info, _ = host_run(name, "slarac", False)
    C.check_coef(sc, info, "host", rtol=1e-12)


def test_mixed_has_both_kinds_of_fit():
    sc, _, info, _ = host_run("mixed", "slarac", False)
    per = (info["status"] == tb.SINGULAR).sum(axis=1)
    assert per.tolist() == sc["slarac"]["singular_per_regime"]
    assert 0 < per[2] < info["status"].shape[1] and per[3] == info["status"].shape[1] and per[0] == 0
    at = sc["slarac_coef_at"]
    assert C.predicted_status(sc, "slarac")[at[:, 0], at[:, 1]].any()
    C.check_coef(sc, info, "host", only_singular=True, rtol=1e-12)


def exp6():
    sc = C.scenario("exp6")
    return sc, [(x, y) for x, y in zip(sc["x"], sc["y"])]


@pytest.mark.parametrize("alg", ["slarac", "qrbs"])
def test_run_tidybench_experiment(alg, monkeypatch):
    monkeypatch.setenv("REDCLIFF_TIDYBENCH_PATH", "host")
    sc, samples = exp6()
    np.random.seed(sc["seed"])
    preds = tb.run_tidybench_experiment(samples, alg)
    assert float(np.random.rand()) == sc[alg]["next_rand"]
    assert len(preds) == 2
    for r, p in enumerate(preds):
        ref = sc[alg + "_preds"][r]
        assert p.shape == (3, 3) and (np.diag(p) == 0).all() and (p >= 0).all()
        assert np.abs(p - ref).max() <= sc[alg]["tol"] * np.abs(ref).max()


def test_prepare_data_for_modeling():
    sc, samples = exp6()
    data, labels, masks, Tw, T, N, R = tb.prepare_data_for_modeling(samples)
    assert (Tw, T, N, R) == (20, 120, 3, 2) and np.array_equal(data, np.concatenate(sc["x"]))
    lab = np.argmax(sc["y"][:, :, 0], axis=1)
    assert np.array_equal(labels, np.repeat(sc["y"][:, :, 0], 20, axis=0))
    for r in range(R):
        assert np.array_equal(masks[r], np.repeat(lab == r, 20)[:, None] * np.ones((1, 3)))
    A = np.array([[1.0, -2.0], [3.0, -4.0]])
    assert np.array_equal(tb.get_standardized_off_diagonal_relation_predictions(A), [[0, 2], [3, 0]])
    assert np.array_equal(tb.get_standardized_off_diagonal_relation_predictions(A, transpose=True), [[0, 3], [2, 0]])


def test_lasar_and_unknown_names():
    _, samples = exp6()
    with pytest.raises(NotImplementedError, match="LARS"):
        tb.run_tidybench_experiment(samples, "lasar")
    with pytest.raises(ValueError):
        tb.run_tidybench_experiment(samples, "selvar")


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_data_raises_before_any_draw(bad, monkeypatch):
    monkeypatch.setenv("REDCLIFF_TIDYBENCH_PATH", "host")
    x = C.scenario("tiny_l1")["series"][0].copy()
    x[17, 1] = bad
    for fn in (tb.slarac, tb.qrbs):
        np.random.seed(4)
        state = np.random.get_state()[1].copy()
        with pytest.raises(ValueError, match="NaN or infinity"):
            fn(x)
        assert np.array_equal(np.random.get_state()[1], state)


def test_input_is_not_modified_and_processing_keywords(monkeypatch):
    monkeypatch.setenv("REDCLIFF_TIDYBENCH_PATH", "host")
    x = C.scenario("tiny_l1")["data"].copy()
    keep = x.copy()
    for fn, kw in ((tb.slarac, dict(n_subsamples=4)), (tb.qrbs, dict(n_resamples=5))):
        np.random.seed(9)
        got = fn(x, pre_normalise=True, post_standardise=True, post_zeroonescaling=True, post_edgeprior=True, **kw)
        assert np.array_equal(x, keep)
        np.random.seed(9)
        raw = fn((keep - keep.mean(axis=0)) / keep.std(axis=0), **kw)
        want = (raw - raw.mean()) / raw.std()
        want = (want - want.min()) / (want.max() - want.min())
        assert np.allclose(got, want / want.mean(), rtol=1e-12, atol=0)
    x32 = keep.astype(np.float32)
    np.random.seed(9)
    a = tb.slarac(x32, n_subsamples=4)
    np.random.seed(9)
    assert np.array_equal(a, tb.slarac(x32.astype(np.float64), n_subsamples=4))


def test_missing_values_drop_rows_on_the_host_route(monkeypatch):
    """missing_values is a host-route feature: auto takes the host, and a marked row leaves every fit."""
    monkeypatch.delenv("REDCLIFF_TIDYBENCH_PATH", raising=False)
    x = C.scenario("tiny_l1")["data"].copy()
    x[20, 0] = -999.0
    np.random.seed(2)
    got, info = tb.slarac(x, n_subsamples=3, missing_values=-999.0, return_info=True)
    assert info["route"] == "host" and np.isfinite(got).all() and np.abs(info["coef"]).max() < 50


def test_exports():
    import redcliff_amd
    for n in ("slarac", "qrbs", "slarac_many", "qrbs_many", "run_tidybench_experiment", "prepare_data_for_modeling",
              "get_standardized_off_diagonal_relation_predictions"):
        assert callable(getattr(redcliff_amd, n))
