"""LASAR on the host route (redcliff_amd/tidybench.py) against the reference's outputs in tests/golden/lasar.npz under
the checks of tests/lasar_common.py, plus the contract of the public calls: the generator's state after a call, the
regime-aware driver, the errors, and that the input is left alone."""
import numpy as np
import pytest

import lasar_common as C
from redcliff_amd import tidybench as tb


@pytest.mark.parametrize("name", ["tiny", "chunk", "drops", "pub10", "lags2"])
def test_host_route_matches_reference(name):
    sc = C.scenario(name)
    raw, info = C.check_all(tb, sc, "host", "host")
    assert (info["status"] == tb.OK).all() and info["n_host_solved"] == 0
    assert (info["flags"] == 0).all()
    assert sc["n_warn"] == 0 and not sc["mask_moved"]   # the reference alone is stable on the committed scenario
    if name == "drops":
        assert sc["drops"] > 0


def test_degenerate_scenario_takes_the_solver_s_other_branches_and_equals_the_fixture():
    """A repeated channel: paths take the solver's drop-for-good branch (the reference warns)."""
    assert C.META["degen"]["n_warn"] > 0
    sc = C.scenario("degen")
    raw, info = C.check_all(tb, sc, "host", "host degen")
    assert np.array_equal(info["flags"], sc["flags"]) and (info["flags"] != 0).any()
    assert np.array_equal(info["status"] == tb.DEGENERATE, info["flags"] != 0)


def test_single_call_equals_the_first_problem():
    sc = C.scenario("tiny")
    raw, info, _ = C.call(tb, sc)
    one, i1, _ = C.call(tb, sc, single=0)
    assert one.shape == (sc["N"], sc["N"]) and np.array_equal(one, raw[0])
    for k in ("coef", "status", "selected", "best_alpha", "best_index"):
        assert np.array_equal(i1[k], info[k][0])
    C.check_scores(sc, one[None], "raw", "host single", regimes=[0])


def test_run_lasar_experiment_matches_the_reference_driver(monkeypatch):
    monkeypatch.setenv("REDCLIFF_TIDYBENCH_PATH", "host")
    e = C.META["exp6"]
    np.random.seed(e["seed"])
    preds = tb.run_lasar_experiment(C.exp6_samples())
    assert float(np.random.rand()) == e["next_rand"]
    for r, p in enumerate(preds):
        ref = C.G["exp6/preds"][r]
        assert np.abs(p - ref).max() <= e["tol"] * np.abs(ref).max()
    with pytest.raises(NotImplementedError, match="LARS") as err:
        tb.run_tidybench_experiment(C.exp6_samples(), "lasar")
    assert "run_lasar_experiment" in str(err.value)


def test_errors_precede_every_draw_and_the_input_is_left_alone(monkeypatch):
    monkeypatch.setenv("REDCLIFF_TIDYBENCH_PATH", "host")
    rng = np.random.RandomState(3)
    np.random.seed(4)
    state = np.random.get_state()

    def untouched():
        return all(np.array_equal(a, b) for a, b in zip(state[1:], np.random.get_state()[1:]))

    with pytest.raises(ValueError, match="n_splits"):
        tb.lasar(rng.randn(5, 3))                      # 4 usable rows < cv
    assert untouched()
    with pytest.raises(ValueError, match="n_splits"):
        tb.lasar(rng.randn(7, 3))                      # round(0.618 * 7) = 4 rows in a subsample < cv
    assert untouched()
    x = rng.randn(40, 3)
    x[7, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        tb.lasar(x)
    assert untouched()
    with pytest.raises(TypeError):
        tb.lasar(rng.randn(40, 3), bogus=1)
    x = C.scenario("tiny")["series"][0].copy()
    keep = x.copy()
    np.random.seed(1)
    a = tb.lasar(x, n_subsamples=2, pre_normalise=True, post_standardise=True)
    assert np.array_equal(x, keep) and a.shape == (3, 3) and np.isfinite(a).all()


def test_exported_from_the_package():
    import redcliff_amd
    assert redcliff_amd.lasar is tb.lasar and redcliff_amd.lasar_many is tb.lasar_many
    assert redcliff_amd.run_lasar_experiment is tb.run_lasar_experiment
