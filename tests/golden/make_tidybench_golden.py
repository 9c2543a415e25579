"""Write tests/golden/tidybench.npz from the reference's SLARAC and QRBS (CPU only; needs the reference tree,
sklearn and this package on the path):

    python tests/golden/make_tidybench_golden.py

Scenarios are seeded regime-switching VAR(1) series multiplied by per-regime 0/1 masks, as the evaluation scripts
build them.  Per scenario and algorithm the file holds the reference's scores (raw and post_standardise=True,
one matrix per regime, regimes run in a loop under one seed), the next ``np.random.rand()`` after the loop, and
what the bounds of tests/tidybench_common.py are made of, all computed here in numpy from the same draws:

* ``kappa``: the largest 2-norm condition number among the fits' Gram matrices that the pivot rule accepts (QRBS:
  the centred, regularised Gram matrix); ``n_max``: the largest row count;
* the per-fit pivot ratios ``min_j pivot_j / G_jj``;
* for SLARAC the reference's per-fit coefficient matrices of a selection of fits (its ``varmodel`` called under
  the same seed at the same stream position), with each selected fit's own kappa and row count;
* ``observed``: the reference-against-host-route difference relative to max |score|, for the reader.

It asserts what the tests rely on: every pivot ratio is < 1e-10 or > 1e-5; outside ``mixed`` none is below; outside
``mixed`` 64 eps n_max kappa <= 1e-8; and at least one scenario splits a fit over several chunks.
"""
import ast
import importlib
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd"))

from oracle import ref_import  # noqa: E402

if ref_import.REF_ROOT not in sys.path:
    sys.path.insert(0, ref_import.REF_ROOT)
ref_slarac = importlib.import_module("tidybench.slarac")
ref_qrbs = importlib.import_module("tidybench.qrbs")

sys.path.insert(0, os.path.dirname(HERE))
from redcliff_amd import tidybench as tb  # noqa: E402

EPS = np.finfo(np.float64).eps
CH = tb.CHUNK_ROWS

# name: N, rows per regime (the series is their concatenation), lags, SLARAC n_subsamples, QRBS n_resamples, seed
SCENARIOS = {
    "tiny_l1": dict(N=3, rows=[30, 30], lags=1, n_subsamples=5, n_resamples=7, seed=11),
    "tiny_l2": dict(N=3, rows=[30, 30], lags=2, n_subsamples=5, n_resamples=7, seed=12),
    "pub10": dict(N=10, rows=[400, 400, 400], lags=1, n_subsamples=200, n_resamples=600, seed=13),
    "pub12": dict(N=12, rows=[CH + 20, CH + 17], lags=1, n_subsamples=9, n_resamples=11, seed=14),
    "lags3": dict(N=10, rows=[400, 400, 400], lags=3, n_subsamples=9, n_resamples=11, seed=15),
    # 80, 50 and 20 non-zero rows and an empty regime (an all-zero series): well-posed and rank-deficient fits
    "mixed": dict(N=10, rows=[80, 50, 20, 0], lags=2, n_subsamples=200, n_resamples=0, seed=16),
}
COEF_FITS = 12   # SLARAC fits per regime whose reference coefficients are stored (plus SINGULAR ones in mixed)


def make_series(sc):
    """Regime-switching VAR(1): windows of 10 rows, interleaved regimes; returns the
    series [T, N] and each row's regime."""
    rng = np.random.RandomState(sc["seed"])
    N, rows = sc["N"], sc["rows"]
    A = []
    for _ in rows:
        a = 0.45 * np.eye(N) + 0.25 * rng.randn(N, N) * (rng.rand(N, N) < 2.0 / N)
        A.append(a / max(1.0, np.abs(np.linalg.eigvals(a)).max() / 0.8))
    win = 10
    todo = [r // win for r in rows]
    extra = [r - win * (r // win) for r in rows]
    order = []
    while any(todo):
        for r in range(len(rows)):
            if todo[r]:
                order.append((r, win))
                todo[r] -= 1
    order += [(r, e) for r, e in enumerate(extra) if e]
    regime = np.concatenate([np.full(n, r, dtype=np.int8) for r, n in order])
    T = len(regime)
    x = np.zeros((T, N))
    x[0] = rng.randn(N)
    for t in range(1, T):
        x[t] = A[regime[t]].dot(x[t - 1]) + rng.randn(N)
    return x, regime


def masked(x, regime, R):
    return np.stack([x * (regime == r)[:, None] for r in range(R)])


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max()) if np.abs(b).max() > 0 else float(np.abs(a - b).max())


def main():
    from tidybench_common import analyse   # reads the previous fixture on import; only the function is used
    out, meta = {}, {}
    split = False
    warnings.simplefilter("ignore")
    for name, sc in SCENARIOS.items():
        x, regime = make_series(sc)
        R, N, lags = len(sc["rows"]), sc["N"], sc["lags"]
        series = masked(x, regime, R)
        T = x.shape[0]
        m = dict(N=N, T=T, R=R, lags=lags, seed=sc["seed"], n_subsamples=sc["n_subsamples"], n_resamples=sc["n_resamples"])
        out[name + "/data"], out[name + "/regime"] = x, regime
        algs = ["slarac"] + (["qrbs"] if sc["n_resamples"] else [])
        for alg in algs:
            if alg == "slarac":
                kw = dict(maxlags=lags, n_subsamples=sc["n_subsamples"])
                ref, ours, plan_fn = ref_slarac.slarac, tb.slarac_many, (
                    lambda: tb._slarac_plan(R, T, N, lags, sc["n_subsamples"], tb.DEFAULT_SUBSAMPLE_SIZES))
            else:
                kw = dict(lags=lags, n_resamples=sc["n_resamples"])
                ref, ours, plan_fn = ref_qrbs.qrbs, tb.qrbs_many, (lambda: tb._qrbs_plan(R, T, N, lags, sc["n_resamples"]))
            np.random.seed(sc["seed"])
            raw = np.stack([ref(series[r].copy(), **kw) for r in range(R)])
            nxt = float(np.random.rand())
            np.random.seed(sc["seed"])
            std = np.stack([ref(series[r].copy(), post_standardise=True, **kw) for r in range(R)])
            np.random.seed(sc["seed"])
            plan = plan_fn()
            assert float(np.random.rand()) == nxt, "the restated draws leave the stream elsewhere than the reference"
            kap, ratio, n_max = analyse(tb, series, plan, 0.005)
            assert ((ratio < 1e-10) | (ratio > 1e-5)).all(), (name, alg, np.sort(ratio.ravel())[:8])
            sing = ratio < tb.PIVOT_MIN
            kappa = float(kap.max())
            tol = 64 * EPS * n_max * kappa
            if name != "mixed":
                assert not sing.any(), (name, alg)
                assert tol <= 1e-8, (name, alg, tol, kappa, n_max)
            os.environ["REDCLIFF_TIDYBENCH_PATH"] = "host"
            np.random.seed(sc["seed"])
            host = ours(series, **kw)
            observed = rel(host, raw)
            split = split or tb.CHUNK_ROWS < n_max
            out["%s/%s_raw" % (name, alg)], out["%s/%s_std" % (name, alg)] = raw, std
            out["%s/%s_pivot" % (name, alg)] = ratio
            m[alg] = dict(kappa=kappa, n_max=n_max, next_rand=nxt, tol=tol, observed=observed, singular=int(sing.sum()),
                          singular_per_regime=[int(v) for v in sing.sum(axis=1)])
            print("%-8s %-6s T=%d kappa=%.3g n_max=%d tol=%.2e observed=%.2e singular=%s min ok ratio=%.2e"
                  % (name, alg, T, kappa, n_max, tol, observed, m[alg]["singular_per_regime"], ratio[~sing].min()))
            if alg == "slarac":
                # the reference's per-fit coefficients: its varmodel, called as its slarac calls it
                S = 1 + sc["n_subsamples"]
                at, coefs = [], []
                np.random.seed(sc["seed"])
                for r in range(R):
                    fits = [ref_slarac.varmodel(series[r], lags)]
                    for size in np.random.choice(tb.DEFAULT_SUBSAMPLE_SIZES, sc["n_subsamples"]):
                        fits.append(ref_slarac.varmodel(series[r], lags, n_samples=int(np.round(size * T))))
                    tot = sum(np.abs(f) for f in fits)[:, 1:] / S
                    assert np.allclose(tot.reshape(N, -1, N).max(axis=1).T, raw[r], rtol=1e-13, atol=0)
                    pick = list(range(min(S, COEF_FITS))) + [int(s) for s in np.nonzero(sing[r])[0][:COEF_FITS] if s >= COEF_FITS]
                    for s in pick:
                        at.append((r, s))
                        coefs.append(fits[s])
                assert float(np.random.rand()) == nxt
                out[name + "/slarac_coef"] = np.stack(coefs)
                out[name + "/slarac_coef_at"] = np.array(at, dtype=np.int32)
                out[name + "/slarac_coef_kappa"] = np.array([kap[r, s] for r, s in at])
                out[name + "/slarac_coef_rows"] = np.array([plan.eff_count()[r, s] for r, s in at], dtype=np.int32)
        meta[name] = m
    assert split, "no scenario splits a fit over several chunks of %d rows" % CH

    # run_tidybench_experiment: six tiny samples through the reference's own driver functions
    src = open(os.path.join(ref_import.REF_ROOT, "evaluate", "eval_algs_by_d4icMSNR.py")).read()
    want = ("prepare_data_for_modeling", "get_standardized_off_diagonal_relation_predictions", "run_tidybench_experiment")
    mod = ast.Module(body=[n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in want], type_ignores=[])
    ns = {"np": np, "slarac": ref_slarac.slarac, "qrbs": ref_qrbs.qrbs, "lasar": None, "print": lambda *a, **k: None}
    exec(compile(mod, "reference_driver", "exec"), ns)
    rng = np.random.RandomState(21)
    A = [0.5 * np.eye(3) + 0.3 * np.eye(3, k=1), 0.5 * np.eye(3) + 0.3 * np.eye(3, k=-1)]
    labels = [0, 1, 0, 1, 1, 0]
    xs, v = [], rng.randn(3)
    for lab in labels:
        w = np.zeros((20, 3))
        for t in range(20):
            v = A[lab].dot(v) + rng.randn(3)
            w[t] = v
        xs.append(w)
    ys = [np.eye(2)[lab].reshape(2, 1) for lab in labels]
    samples = [(xw, yw) for xw, yw in zip(xs, ys)]
    out["exp6/x"], out["exp6/y"] = np.stack(xs), np.stack(ys)
    em = dict(seed=22)
    series = masked(np.concatenate(xs), np.repeat(labels, 20), 2)
    for alg in ("slarac", "qrbs"):
        np.random.seed(22)
        preds = np.stack(ns["run_tidybench_experiment"](samples, alg))
        nxt = float(np.random.rand())
        np.random.seed(22)
        plan = tb._slarac_plan(2, 120, 3, 1, 200, tb.DEFAULT_SUBSAMPLE_SIZES) if alg == "slarac" else tb._qrbs_plan(2, 120, 3, 1, 600)
        kap, ratio, n_max = analyse(tb, series, plan, 0.005)
        assert (ratio > 1e-5).all()
        out["exp6/%s_preds" % alg] = preds
        em[alg] = dict(kappa=float(kap.max()), n_max=n_max, next_rand=nxt, tol=64 * EPS * n_max * float(kap.max()))
        print("exp6 %s tol=%.2e" % (alg, em[alg]["tol"]))
    meta["exp6"] = em
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "tidybench.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
