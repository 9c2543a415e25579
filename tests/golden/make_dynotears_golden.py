"""Write tests/golden/dynotears.npz from the reference's DYNOTEARS (CPU only; needs the reference tree, scipy,
networkx and pandas):

    python tests/golden/make_dynotears_golden.py

causalnex is not needed: ``causalnex.structure`` is stubbed in ``sys.modules`` here (a networkx DiGraph stands in
for StructureModel; the graph object is not part of the fixture).

Scenarios are seeded stable VAR(1) recordings, z-scored per channel and cast to float32 (``make_recording``).
Per recording the file holds the reference's (W, A) and what the bound of tests/dynotears_common.py is made of,
measured on the reference alone:

* ``spread``: the largest change of (W, A) among 8 copies of the input with every float32 moved one ulp up or down;
* ``tolgap``: the change when every inner solve stops at ftol 1e-12 / gtol 1e-8 instead of scipy's defaults;
* ``warned``: whether numpy raised a floating-point warning (an overflowing line-search trial point).

Seeds are tried in order until a scenario has its recordings; a recording is kept when it raised no warning and
10 max(spread, tolgap) <= 0.1 max |reference|, which is asserted.  A recording on which the reference itself
overflows is searched among OVERFLOW_SEEDS and kept as the scenario ``overflow``, flagged ``compared = 0``; none of
the seeds tried here (1001 - 1499, scipy 1.15.3) produced one.  ``trial_overflow`` holds two D4IC-shaped recordings on
which the device's line search meets non-finite trial values, also ``compared = 0``.

Single-solve cases (one inner solve from wa = 0 at a given (rho, alpha)) are solved with scipy's L-BFGS-B on the
numpy objective of tests/dynotears_common.py, once at the defaults and once at ftol 0 / gtol 1e-8; f and the
projected-gradient norm of both are stored, and f_default - f_tight >= 1e-10 is asserted.

Whole ``DYNOTEARS_Model.fit`` results are stored for the d5 and d10 scenarios at lag_size 1 and 2, with the sum of
the recordings' bounds divided by d.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types
import warnings

import networkx as nx
import numpy as np
import scipy.optimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_import  # noqa: E402
import dynotears_common as dc  # noqa: E402


class _StructureModel(nx.DiGraph):
    def add_weighted_edges_from(self, ebunch, weight="weight", **attr):
        super().add_weighted_edges_from(ebunch, weight=weight, **attr)


def import_reference():
    import matplotlib
    matplotlib.use("Agg")
    pkg, st, tr = types.ModuleType("causalnex"), types.ModuleType("causalnex.structure"), types.ModuleType("causalnex.structure.transformers")
    st.StructureModel = _StructureModel
    tr.DynamicDataTransformer = object
    pkg.structure, st.transformers = st, tr
    sys.modules.update({"causalnex": pkg, "causalnex.structure": st, "causalnex.structure.transformers": tr})
    if "pywt" not in sys.modules:
        sys.modules["pywt"] = types.ModuleType("pywt")
    if ref_import.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REF_ROOT)
    return importlib.import_module("models.causalnex_dynotears_vanilla"), importlib.import_module("models.dynotears_vanilla")


REF, REF_MODEL = import_reference()

# name: d, rows of a problem, p, lambda, first seed, recordings, tabu
SCENARIOS = {
    "d3": dict(d=3, rows=8, p=1, lam=0.05, seed=100, count=3),
    "d5": dict(d=5, rows=11, p=1, lam=0.05, seed=200, count=3),
    "d4p2": dict(d=4, rows=14, p=2, lam=0.05, seed=300, count=3),
    "d7tabu": dict(d=7, rows=29, p=1, lam=0.05, seed=400, count=3,
                   tabu=dict(edges=[[0, 1, 2], [1, 3, 4]], parents=[5], children=[6])),
    "d10": dict(d=10, rows=20, p=1, lam=0.1, seed=500, count=3),
    "d12": dict(d=12, rows=49, p=1, lam=0.1, seed=600, count=3),
}
OVERFLOW_SEEDS = [1001] + list(range(1002, 1040))
# D4IC-shaped recordings on which the device's line search met non-finite trial values (the indices that
# scripts/dynotears_fit.py reports, its recording s has the seed 5000 + s).  They are not selected for being well posed,
# so they are not compared; the invariants are checked on them.
TRIAL_OVERFLOW_SEEDS = [5017, 5031]
SINGLE = [(0.0, 0.0), (1.0, 0.0), (1e3, 0.5)]
DEFAULTS = dict(max_iter=100, h_tol=1e-8, w_threshold=0.0)


def make_recording(seed, d, T):
    rng = np.random.RandomState(seed)
    A = (rng.rand(d, d) < 2.0 / d) * rng.randn(d, d) * 0.5 + 0.3 * np.eye(d)
    A = A / max(1.0, np.abs(np.linalg.eigvals(A)).max() / 0.8)
    x = np.zeros(d)
    out = []
    for t in range(20 + T):
        x = A @ x + 0.3 * rng.randn(d)
        if t >= 20:
            out.append(x)
    x = np.array(out)
    return ((x - x.mean(0)) / x.std(0)).astype(np.float32)


def run_ref(X, Xl, lam, tb, tight=False):
    """The reference's (W, A, warned); tight=True passes ftol 1e-12 / gtol 1e-8 to every inner solve."""
    real = REF.sopt
    if tight:
        def minimize(*a, **k):
            return scipy.optimize.minimize(*a, options=dict(ftol=1e-12, gtol=1e-8), **k)
        REF.sopt = types.SimpleNamespace(minimize=minimize)
    try:
        with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("always")
            _, W, A = REF.from_numpy_dynamic(X, Xl, lam, lam, DEFAULTS["max_iter"], DEFAULTS["h_tol"], DEFAULTS["w_threshold"],
                                             tb["tabu_edges"], tb["tabu_parent_nodes"], tb["tabu_child_nodes"])
    finally:
        REF.sopt = real
    warned = any(issubclass(w.category, RuntimeWarning) for w in caught)
    return np.array(W), np.array(A), warned


def change(a, b):
    return max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))


def measure(x, p, lam, tb, lag=1, seed=0):
    X, Xl = dc.split(x, p, lag)
    W, A, warned = run_ref(X, Xl, lam, tb)
    rng = np.random.RandomState(seed)
    spread = 0.0
    for _ in range(8):
        up = rng.rand(*x.shape) < 0.5
        y = np.where(up, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float32)
        Wc, Ac, wc = run_ref(*dc.split(y, p, lag), lam, tb)
        spread = max(spread, change((W, A), (Wc, Ac)))
        warned = warned or wc
    Wt, At, wt = run_ref(X, Xl, lam, tb, tight=True)
    return W, A, spread, change((W, A), (Wt, At)), bool(warned or wt)


def single_solve(X, Xl, lam, rho, alpha, fixed, tight):
    nv = fixed.size
    bnds = [(0, 0) if f else (0, None) for f in fixed]
    opts = dict(ftol=0.0, gtol=1e-8) if tight else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = scipy.optimize.minimize(lambda w: dc.objective(w, X, Xl, rho, alpha, lam, lam), np.zeros(nv), method="L-BFGS-B", jac=True,
                                      bounds=bnds, options=opts)
    f, g = dc.objective(res.x, X, Xl, rho, alpha, lam, lam)
    return f, dc.proj_grad_norm(res.x, g, fixed), res.x


def main():
    out, meta = {}, {"scenarios": {}, "tried": {}}
    for name, sc in SCENARIOS.items():
        d, p, lam = sc["d"], sc["p"], sc["lam"]
        tb = dc.tabu(sc)
        keep, tried, seed = [], [], sc["seed"]
        while len(keep) < sc["count"]:
            x = make_recording(seed, d, sc["rows"] + p)
            W, A, spread, tolgap, warned = measure(x, p, lam, tb, seed=seed)
            ratio = dc.MARGIN * max(spread, tolgap) / (0.1 * max(np.abs(W).max(), np.abs(A).max(), 1e-300))
            tried.append([seed, ratio, warned])
            print(name, seed, "spread %.2e tolgap %.2e ratio %.3f warned %s" % (spread, tolgap, ratio, warned), flush=True)
            if not warned and ratio <= 1.0:
                keep.append((seed, x, W, A, spread, tolgap))
            seed += 1
            assert seed < sc["seed"] + 40, name
        for k, v in zip(("seeds", "data", "W", "A", "spread", "tolgap"), zip(*keep)):
            out[name + "/" + k] = np.array(v)
        for r in range(sc["count"]):
            assert dc.MARGIN * max(keep[r][4], keep[r][5]) <= 0.1 * max(np.abs(keep[r][2]).max(), np.abs(keep[r][3]).max())
        meta["scenarios"][name] = dict(d=d, p=p, rows=sc["rows"], lam=lam, count=sc["count"], tabu=sc.get("tabu"), compared=1)
        meta["tried"][name] = tried

    # one recording whose reference run overflows in a line-search trial point: kept, not compared
    for seed in OVERFLOW_SEEDS:
        x = make_recording(seed, 10, 21)
        W, A, warned = run_ref(*dc.split(x, 1), 0.1, dc.tabu({}))
        if warned:
            print("overflow recording: seed", seed, flush=True)
            out["overflow/seeds"], out["overflow/data"], out["overflow/W"], out["overflow/A"] = np.array([seed]), x[None], W[None], A[None]
            out["overflow/spread"], out["overflow/tolgap"] = np.array([np.nan]), np.array([np.nan])
            meta["scenarios"]["overflow"] = dict(d=10, p=1, rows=20, lam=0.1, count=1, tabu=None, compared=0)
            break
    else:
        print("no overflowing recording among the seeds tried", flush=True)

    if TRIAL_OVERFLOW_SEEDS:
        xs = [make_recording(seed, 10, 21) for seed in TRIAL_OVERFLOW_SEEDS]
        refs = [run_ref(*dc.split(x, 1), 0.1, dc.tabu({})) for x in xs]
        out["trial_overflow/seeds"], out["trial_overflow/data"] = np.array(TRIAL_OVERFLOW_SEEDS), np.stack(xs)
        out["trial_overflow/W"], out["trial_overflow/A"] = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
        out["trial_overflow/spread"] = out["trial_overflow/tolgap"] = np.full(len(xs), np.nan)
        meta["scenarios"]["trial_overflow"] = dict(d=10, p=1, rows=20, lam=0.1, count=len(xs), tabu=None, compared=0,
                                                   reference_warned=[bool(r[2]) for r in refs])

    # single inner solves from wa = 0
    cases = []
    for name in ("d5", "d10"):
        sc = SCENARIOS[name]
        fixed = dc.fixed_mask(sc["d"], 1)
        for r in (0, 1):
            X, Xl = dc.split(out[name + "/data"][r], 1)
            for rho, alpha in SINGLE:
                fd, pd, _ = single_solve(X, Xl, sc["lam"], rho, alpha, fixed, False)
                ft, pt, _ = single_solve(X, Xl, sc["lam"], rho, alpha, fixed, True)
                print("single", name, r, rho, alpha, "f_def - f_tight %.2e pg_def %.2e pg_tight %.2e" % (fd - ft, pd, pt), flush=True)
                assert fd - ft >= 1e-10, (name, r, rho, alpha, fd - ft)
                cases.append(dict(scenario=name, rec=r, rho=rho, alpha=alpha, f_default=fd, f_tight=ft, pg_default=pd, pg_tight=pt))
    meta["single"] = cases

    # whole model fits
    fits = []
    for name in ("d5", "d10"):
        sc = SCENARIOS[name]
        data = out[name + "/data"]
        for lag in (1, 2):
            model = REF_MODEL.DYNOTEARS_Model(lambda_w=sc["lam"], lambda_a=sc["lam"])
            with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model.fit(tmp, data, None, lag_size=lag)
            bnd = 0.0
            for r in range(data.shape[0]):
                if lag == 1:
                    bnd += dc.MARGIN * max(out[name + "/spread"][r], out[name + "/tolgap"][r])
                else:
                    _, _, spread, tolgap, _ = measure(data[r], 1, sc["lam"], dc.tabu({}), lag=lag, seed=r)
                    bnd += dc.MARGIN * max(spread, tolgap)
            key = "fit/%s/lag%d" % (name, lag)
            out[key] = np.array(model.GC())
            fits.append(dict(scenario=name, lag=lag, key=key, bound=bnd / sc["d"]))
            print(key, "bound %.2e max |a_est| %.3f" % (bnd / sc["d"], np.abs(out[key]).max()), flush=True)
    meta["fits"] = fits
    meta["scipy"] = scipy.__version__
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(dc.PATH, **out)
    print("wrote", dc.PATH, os.path.getsize(dc.PATH), "bytes")


if __name__ == "__main__":
    main()
