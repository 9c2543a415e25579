"""Host route of redcliff_amd.dynotears_vanilla (the reference's loop restated on scipy's L-BFGS-B) against
tests/golden/dynotears.npz, and everything of the module that needs no GPU: the variable layout, the fixed
entries, the validity errors, the route switch, the model's pickle, the evaluation branch and the loader."""
import os
import pickle

import numpy as np
import pytest

import dynotears_common as dc
from redcliff_amd import dynotears_vanilla as dy


@pytest.fixture(autouse=True)
def host_route(monkeypatch):
    monkeypatch.setenv("REDCLIFF_DYNOTEARS_PATH", "host")


COMPARED = [n for n in dc.names() if dc.meta()["scenarios"][n]["compared"]]


@pytest.mark.parametrize("name", COMPARED)
def test_host_route_matches_reference(name):
    sc = dc.scenario(name)
    recs = [0] if sc["d"] >= 10 else range(sc["count"])   # one recording of the larger shapes keeps this quick
    for r in recs:
        X, Xl = dc.problem(sc, r)
        sm, W, A = dy.from_numpy_dynamic(X, Xl, sc["lam"], sc["lam"], **dc.tabu(sc))
        b = dc.bound(sc, r)
        assert np.abs(W - sc["W"][r]).max() <= b and np.abs(A - sc["A"][r]).max() <= b
        fixed = dc.fixed_mask(sc["d"], sc["p"], **dc.tabu(sc))
        # an entry fixed in both copies is exactly zero
        both = fixed.reshape(2 * (sc["p"] + 1), -1)
        zw = both[0].reshape(sc["d"], sc["d"])
        assert (W[zw] == 0).all() and (np.diag(W) == 0).all()
        for k in range(sc["p"]):
            assert (A[k * sc["d"]:(k + 1) * sc["d"]][both[2 + 2 * k].reshape(sc["d"], sc["d"])] == 0).all()
        assert sm.number_of_nodes() == (sc["p"] + 1) * sc["d"]
        assert sm.number_of_edges() == int((W != 0).sum() + (A != 0).sum())
        for u, v, w in sm.edges.data("weight"):
            i, lag = (int(t) for t in u.split("_lag"))
            j = int(v.split("_lag")[0])
            assert v.endswith("_lag0") and w == (W[i, j] if lag == 0 else A[(lag - 1) * sc["d"] + i, j])


def test_model_fit_matches_reference(tmp_path):
    fit = [f for f in dc.meta()["fits"] if f["scenario"] == "d5"]
    sc = dc.scenario("d5")
    for f in fit:
        model = dy.DYNOTEARS_Model(lambda_w=sc["lam"], lambda_a=sc["lam"])
        assert model.fit(str(tmp_path), sc["data"], None, lag_size=f["lag"]) is None
        assert np.abs(model.GC() - dc.golden()[f["key"]]).max() <= f["bound"]
    # the pickle the reference's loaders read
    path = os.path.join(str(tmp_path), "final_best_model.pkl")
    import torch
    back = torch.load(path, map_location="cpu", weights_only=False)
    assert isinstance(back, dy.DYNOTEARS_Model) and np.array_equal(back.GC(), model.GC()) and back.lambda_w == sc["lam"]
    again = pickle.loads(pickle.dumps(model))
    assert np.array_equal(again.GC(), model.GC()) and again.max_iter == 100 and again.tabu_edges is None
    assert model.evaluate(None, str(tmp_path), None) is None


def test_fit_many_is_one_batch_per_shape():
    sc = dc.scenario("d3")
    models = [dy.DYNOTEARS_Model(lambda_w=lam, lambda_a=lam, max_iter=3) for lam in (0.05, 0.2)]
    out = dy.fit_dynotears_baselines(models, [sc["data"], sc["data"][:2]])
    assert [i["batch"] for i in out["infos"]] == [5, 5] and out["val_losses"] == [None, None]
    single = dy.DYNOTEARS_Model(lambda_w=0.2, lambda_a=0.2, max_iter=3)
    dy.fit_dynotears_baselines([single], [sc["data"][:2]])
    assert np.array_equal(single.GC(), models[1].GC())
    assert not np.array_equal(models[0].GC()[:2], models[1].GC()[:2])
    # the divisor is the node count, as in the reference
    _, A, _ = dy.from_numpy_dynamic_many(sc["data"][:2, :-1], sc["data"][:2, 1:], 0.2, 0.2, max_iter=3)
    assert np.allclose(single.GC(), (A[0] + A[1]) / 3.0, rtol=0, atol=1e-15)


def test_reshape_layout():
    d, p = 3, 2
    nv = 2 * (p + 1) * d * d
    wa = np.arange(nv, dtype=float) ** 1.5
    view = wa.reshape(2 * (p + 1) * d, d)
    W, A = dy.reshape_wa(wa, d, p)
    assert np.array_equal(W, view[:d] - view[d:2 * d])
    for k in range(p):
        base = 2 * d + 2 * k * d
        assert np.array_equal(A[k * d:(k + 1) * d], view[base:base + d] - view[base + d:base + 2 * d])
    W2, A2 = dc.reshape_wa(wa, d, p)
    assert np.array_equal(W, W2) and np.array_equal(A, A2)


def test_fixed_mask():
    tb = dict(tabu_edges=[(0, 1, 2), (1, 3, 4), (2, 0, 1)], tabu_parent_nodes=[5], tabu_child_nodes=[6])
    for p in (1, 2):
        assert np.array_equal(dy.fixed_mask(7, p, **tb).astype(bool), dc.fixed_mask(7, p, **tb))
    m = dy.fixed_mask(4, 1).reshape(4, 4, 4)
    assert all(np.array_equal(m[k], np.eye(4)) for k in (0, 1)) and not m[2:].any()


def test_validity_errors():
    x = np.ones((6, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="X is empty"):
        dy.from_numpy_dynamic(np.ones((0, 3)), x)
    with pytest.raises(ValueError, match="Xlags is empty"):
        dy.from_numpy_dynamic(x, np.ones((6, 0)))
    with pytest.raises(ValueError, match="same number of rows"):
        dy.from_numpy_dynamic(x, np.ones((5, 3)))
    with pytest.raises(ValueError, match="multiple"):
        dy.from_numpy_dynamic(x, np.ones((6, 4)))
    with pytest.raises(ValueError, match="rho0"):
        dy.from_numpy_dynamic_many(x[None], x[None], rho0=0.0, max_iter=2)


def test_route_environment(monkeypatch):
    import torch
    x = np.random.RandomState(0).randn(1, 7, 3).astype(np.float32)
    monkeypatch.setenv("REDCLIFF_DYNOTEARS_PATH", "sideways")
    with pytest.raises(ValueError, match="fused, host or auto"):
        dy.from_numpy_dynamic_many(x[:, :-1], x[:, 1:], max_iter=1)
    monkeypatch.setenv("REDCLIFF_DYNOTEARS_PATH", "host")
    assert dy.from_numpy_dynamic_many(x[:, :-1], x[:, 1:], max_iter=1)[2]["route"] == "host"
    if not torch.cuda.is_available():
        monkeypatch.setenv("REDCLIFF_DYNOTEARS_PATH", "auto")
        assert dy.from_numpy_dynamic_many(x[:, :-1], x[:, 1:], max_iter=1)[2]["route"] == "host"
        monkeypatch.setenv("REDCLIFF_DYNOTEARS_PATH", "fused")
        with pytest.raises(RuntimeError, match="fused"):
            dy.from_numpy_dynamic_many(x[:, :-1], x[:, 1:], max_iter=1)


def test_status_and_counts_on_the_host_route():
    sc = dc.scenario("d3")
    X, Xl = dc.problem(sc, 0)
    W, A, info = dy.from_numpy_dynamic_many(X[None], Xl[None], sc["lam"], sc["lam"])
    assert info["status_names"] == ["CONVERGED"] and dc.h_of(W[0]) <= 1e-8
    assert info["counts"]["inner_solves"][0] >= info["counts"]["outer_iterations"][0] >= 1
    Xn = X.copy()
    Xn[0, 0] = np.inf
    W, A, info = dy.from_numpy_dynamic_many(Xn[None], Xl[None], sc["lam"], sc["lam"])
    assert info["status"][0] == dy.NONFINITE and np.isnan(W).all() and np.isnan(A).all()
    # strict threshold
    W, A, _ = dy.from_numpy_dynamic_many(X[None], Xl[None], sc["lam"], sc["lam"], w_threshold=0.05)
    assert not ((np.abs(A) < 0.05) & (A != 0)).any()


def test_native_argument_checks_precede_the_device():
    from redcliff_amd import _native as nat
    L = nat.lib()
    assert L.redcliff_dynotears_supported(12, 1) == 1 and L.redcliff_dynotears_supported(8, 2) == 1
    assert L.redcliff_dynotears_supported(13, 1) == 0 and L.redcliff_dynotears_supported(9, 2) == 0
    assert L.redcliff_dynotears_ws_bytes(3, 13, 1, 10) == 0 and L.redcliff_dynotears_ws_bytes(3, 12, 1, 17) == 0
    nv = 2 * 2 * 100
    assert L.redcliff_dynotears_ws_bytes(3, 10, 1, 10) >= 8 * 3 * (20 * 20 + 4 * nv + 20 * nv)
    a = nat.DynotearsArgs()
    a.P, a.d, a.p, a.m, a.max_iter, a.evals_per_launch, a.maxiter, a.maxfun, a.maxls = 1, 13, 1, 10, 1, 1, 1, 1, 1
    assert L.redcliff_dynotears_run(a, None) == -2
    a.d = 5
    a.rho_max, a.rho0, a.max_iter = 1e20, 0.0, 2
    assert L.redcliff_dynotears_run(a, None) == -1 and b"rho0" in L.redcliff_last_error()
    a.rho0 = 1.0
    assert L.redcliff_dynotears_run(a, None) == -1 and b"null" in L.redcliff_last_error()


def test_evaluation_branch():
    from redcliff_amd import evaluation
    model = dy.DYNOTEARS_Model()
    model.a_est = np.arange(9.0).reshape(3, 3)
    ests = evaluation.get_model_gc_estimates(model, "DYNOTEARS_Vanilla", 3)
    assert len(ests) == 3 and all(np.array_equal(e, model.a_est) for e in ests) and ests[0] is not model.a_est


def test_dream4_loader_as_tensors(tmp_path):
    """Whole normalised recordings [N, T, p] and the label matrix, float32, split as the *_as_matrices loader splits;
    the model fits straight from them."""
    from redcliff_amd import data as RD
    LG = np.load(os.path.join(dc.HERE, "golden", "loaders.npz"))
    for n in sorted(set(k.split("/")[2] for k in LG.files if k.startswith("d4/file/"))):
        with open(os.path.join(str(tmp_path), n), "wb") as fh:
            pickle.dump([(x, y) for x, y in zip(LG["d4/file/%s/x" % n], LG["d4/file/%s/y" % n])], fh)
    Xt, yt, Xv, yv = RD.load_normalized_DREAM4_data_train_test_split_as_tensors(str(tmp_path), train_portion=0.67)
    assert Xt.dtype == yt.dtype == Xv.dtype == yv.dtype == np.float32
    assert Xt.ndim == 3 and Xt.shape[1:] == Xv.shape[1:] and Xt.shape[0] + Xv.shape[0] == 11 and Xv.shape[0] > 0
    assert yt.shape[0] == Xt.shape[0] and yv.shape[0] == Xv.shape[0]
    for sub, X in (("train", Xt), ("validation", Xv)):
        ds = RD.NormalizedRecordingDirectory(str(tmp_path / sub), "dream4")
        want, _ = ds.materialize()
        assert np.array_equal(X, want.numpy())
    flat = RD.load_normalized_DREAM4_data_train_test_split_as_matrices(str(tmp_path), max_num_features_per_series=Xt.shape[1],
                                                                       train_portion=0.67)
    assert np.array_equal(flat[0], Xt.reshape(Xt.shape[0], -1)) and np.array_equal(flat[1], yt)
    with pytest.raises(ValueError, match="whole recordings"):
        RD.load_normalized_DREAM4_data_train_test_split_as_tensors(str(tmp_path), signal_format="original flattened")
    model = dy.DYNOTEARS_Model(lambda_w=0.3, lambda_a=0.3, max_iter=2)
    model.fit(str(tmp_path), Xt[:2, :12], None)
    assert model.GC().shape == (Xt.shape[2], Xt.shape[2]) and np.isfinite(model.GC()).all()
