"""Shared by tests/test_lasar_host.py and tests/test_gpu_lasar.py: the scenarios of tests/golden/lasar.npz (written by
tests/golden/make_lasar_golden.py from the reference and sklearn) and the checks both routes are held to.

Per (regime, fit, target): the selection mask and the index of the best alpha equal the reference's, the best alpha
is within 1e-12 relative, and the refit coefficients are within ``64 eps rows kappa`` of that triple's own refit
(the bound of tests/tidybench_common.py: a normal-equations solve whose Gram matrix, condition number kappa, is a sum
of ``rows`` terms taken in another order).  Scores are within ``64 eps n_max kappa_max``.  rows and kappa come from
the fixture, not from the code under test.
"""
import json
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "lasar.npz"))
META = json.loads(str(G["meta"]))
EPS = np.finfo(np.float64).eps
_CACHE = {}


def scenario(name):
    if name not in _CACHE:
        sc = dict(META[name])
        for k in G.files:
            if k.startswith(name + "/"):
                sc[k.split("/", 1)[1]] = G[k]
        sc["name"] = name
        if "regime" in sc:
            sc["series"] = np.stack([sc["data"] * (sc["regime"] == r)[:, None] for r in range(sc["R"])])
        _CACHE[name] = sc
    return _CACHE[name]


def kwargs(sc):
    kw = dict(maxlags=sc["lags"], n_subsamples=sc["n_subsamples"])
    if sc.get("sizes"):
        kw["subsample_sizes"] = sc["sizes"]
    return kw


def call(tb, sc, path="host", series=None, single=None, **extra):
    """One seeded call under REDCLIFF_TIDYBENCH_PATH=path: ``lasar_many`` over the masked series, or with
    ``single=r`` one ``lasar`` call on regime r (seeded alike, so only regime 0 reproduces the fixture).  Returns
    (scores, info, the generator's next draw)."""
    old = os.environ.get("REDCLIFF_TIDYBENCH_PATH")
    os.environ["REDCLIFF_TIDYBENCH_PATH"] = path
    x = sc["series"] if series is None else series
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.random.seed(sc["seed"])
            kw = dict(kwargs(sc), return_info=True, **extra)
            out, info = tb.lasar_many(x, **kw) if single is None else tb.lasar(x[single], **kw)
            nxt = float(np.random.rand())
    finally:
        if old is None:
            del os.environ["REDCLIFF_TIDYBENCH_PATH"]
        else:
            os.environ["REDCLIFF_TIDYBENCH_PATH"] = old
    assert info["route"] == path
    return out, info, nxt


def check_triples(sc, info, label):
    assert (info["selected"] == sc["selected"]).all(), (label, sc["name"], "selection masks")
    # the deliberately degenerate scenario names the triples on which the reference's own best index is stable
    at = sc["index_stable"] if "index_stable" in sc else np.ones(sc["rows"].shape + (sc["N"],), dtype=bool)
    assert (info["best_index"][at] == sc["best_index"][at]).all(), (label, sc["name"], "best indices")
    ref = sc["best_alpha"][at]
    err = np.abs(info["best_alpha"][at] - ref)
    print("%s %s best_alpha: worst relative difference %.3e" % (label, sc["name"], (err / np.maximum(np.abs(ref), 1e-300)).max()))
    assert (err <= 1e-12 * np.abs(ref)).all(), (label, sc["name"], "best_alpha")
    scale = np.abs(sc["coef"]).max(axis=-1)
    bound = 64 * EPS * sc["rows"][:, :, None] * sc["kappa"] * scale
    cerr = np.abs(info["coef"] - sc["coef"]).max(axis=-1)
    print("%s %s per-triple coef: worst err / bound %.3e" % (label, sc["name"], (cerr / np.maximum(bound, 1e-300)).max()))
    assert (cerr <= bound).all(), (label, sc["name"], "refit coefficients", float((cerr - bound).max()))


def check_scores(sc, got, key, label, regimes=None):
    ref = sc[key]
    tol = 64 * EPS * sc["n_max"] * sc["kappa_max"]
    for r in (range(sc["R"]) if regimes is None else regimes):
        scale = np.abs(ref[r]).max()
        err = np.abs(got[r] - ref[r]).max()
        print("%s %s %s regime %d: err %.3e bound %.3e" % (label, sc["name"], key, r, err, tol * scale))
        assert err <= tol * scale


def check_all(tb, sc, path, label, **extra):
    raw, info, nxt = call(tb, sc, path, **extra)
    assert nxt == sc["next_rand"]
    check_triples(sc, info, label)
    check_scores(sc, raw, "raw", label)
    std, _, _ = call(tb, sc, path, post_standardise=True, **extra)
    check_scores(sc, std, "std", label)
    return raw, info


def exp6_samples():
    return [(x, y) for x, y in zip(G["exp6/x"], G["exp6/y"])]
