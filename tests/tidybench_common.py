"""Shared by tests/test_tidybench_host.py and tests/test_gpu_tidybench.py: the scenarios of tests/golden/tidybench.npz
(written by tests/golden/make_tidybench_golden.py from the reference) and the bound both routes are held to.

The bound is ``64 eps n_max kappa`` relative to ``max |score|``: the forward error of a normal-equations solve
whose Gram matrix (condition number kappa) is a sum of n_max terms taken in another order, with 64 for the
constant.  kappa and n_max come from the fixture (the reference's draws, numpy), not from the code under test; the
fixture also records the difference the generator observed (``observed``), a few 1e-16 to 1e-14.
"""
import json
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "tidybench.npz"))
META = json.loads(str(G["meta"]))
NAMES = [n for n in META if n != "exp6"]
EPS = np.finfo(np.float64).eps
PIVOT_MIN = 1e-8


def scenario(name):
    sc = dict(META[name])
    for k in G.files:
        if k.startswith(name + "/"):
            sc[k.split("/", 1)[1]] = G[k]
    sc["name"] = name
    if "regime" in sc:
        sc["series"] = np.stack([sc["data"] * (sc["regime"] == r)[:, None] for r in range(sc["R"])])
    return sc


def algs(sc):
    return [a for a in ("slarac", "qrbs") if a in sc]


def kwargs(sc, alg):
    if alg == "slarac":
        return dict(maxlags=sc["lags"], n_subsamples=sc["n_subsamples"])
    return dict(lags=sc["lags"], n_resamples=sc["n_resamples"])


def call(tb, sc, alg, series=None, path="host", single=None, **extra):
    """One seeded call under REDCLIFF_TIDYBENCH_PATH=path: ``*_many`` over the masked series, or with ``single=r``
    a loop-free single call on regime r (seeded alike, so only regime 0 reproduces the fixture)."""
    old = os.environ.get("REDCLIFF_TIDYBENCH_PATH")
    os.environ["REDCLIFF_TIDYBENCH_PATH"] = path
    x = sc["series"] if series is None else series
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.random.seed(sc["seed"])
            kw = dict(kwargs(sc, alg), return_info=True, **extra)
            if single is None:
                out, info = (tb.slarac_many if alg == "slarac" else tb.qrbs_many)(x, **kw)
            else:
                out, info = (tb.slarac if alg == "slarac" else tb.qrbs)(x[single], **kw)
    finally:
        if old is None:
            del os.environ["REDCLIFF_TIDYBENCH_PATH"]
        else:
            os.environ["REDCLIFF_TIDYBENCH_PATH"] = old
    assert info["route"] == path
    return out, info


def check_scores(sc, alg, got, key, label, regimes=None):
    """got [R, N, N] against the fixture's ``<alg>_<key>`` under the scenario's bound, regime by regime."""
    ref = sc["%s_%s" % (alg, key)]
    tol = 64 * EPS * sc[alg]["n_max"] * sc[alg]["kappa"]
    for r in (range(sc["R"]) if regimes is None else regimes):
        if not np.isfinite(ref[r]).all():   # the standardised scores of an all-zero series are 0 / 0
            assert key == "std" and not np.abs(sc["%s_raw" % alg][r]).any()
            continue
        scale = np.abs(ref[r]).max()
        err = np.abs(got[r] - ref[r]).max()
        print("%s %s %s %s regime %d: err %.3e bound %.3e (max |score| %.3e)" % (label, sc["name"], alg, key, r, err, tol * scale, scale))
        assert err <= tol * scale


def analyse(tb, series, plan, alpha):
    """kappa [P, S] (0 where the pivot rule refuses the fit), the pivot ratios [P, S] and n_max of a plan's fits,
    in numpy from gathered rows."""
    P, S = plan.count.shape
    ratio = np.zeros((P, S))
    kap = np.zeros((P, S))
    for b in range(P):
        Z, _ = tb._lag_stack(series[b], plan.lags)
        for s in range(S):
            rows = plan.rows(b, s)
            Zs = Z if rows is None else Z[rows]
            if plan.mode == 0:
                c = int(plan.ncols[b, s])
                Gm = Zs[:, :c].T.dot(Zs[:, :c])
            else:
                X = Zs[:, 1:] - Zs[:, 1:].mean(axis=0)
                Gm = X.T.dot(X) + alpha * np.eye(X.shape[1])
            _, ratio[b, s], st = tb._pivot_cholesky(Gm)
            kap[b, s] = np.linalg.cond(Gm) if st == tb.OK else 0.0
    return kap, ratio, int(plan.eff_count().max())


def predicted_status(sc, alg):
    return (sc["%s_pivot" % alg] < PIVOT_MIN).astype(np.int32)


def check_coef(sc, info, label, only_singular=False, rtol=None):
    """Per-fit SLARAC coefficients [R, S, N, D] against the reference's, each under its own fit's bound
    (64 eps rows kappa of that fit), or with ``only_singular`` the SINGULAR fits under rtol."""
    sing = predicted_status(sc, "slarac")
    worst = 0.0
    for (r, s), ref, kap, rows in zip(sc["slarac_coef_at"], sc["slarac_coef"], sc["slarac_coef_kappa"], sc["slarac_coef_rows"]):
        got = info["coef"][r, s]
        scale = np.abs(ref).max()
        err = np.abs(got - ref).max()
        if sing[r, s]:
            if rtol is not None:
                assert err <= rtol * scale, (label, sc["name"], r, s, err, scale)
        elif not only_singular:
            bound = 64 * EPS * rows * kap * scale
            worst = max(worst, err / bound)
            assert err <= bound, (label, sc["name"], r, s, err, bound)
    print("%s %s per-fit coef: worst err / bound %.3e" % (label, sc["name"], worst))
