"""Shared by tests/test_dirspec_host.py and tests/test_gpu_dirspec.py: the scenarios of tests/golden/dirspec.npz
(written by tests/golden/make_dirspec_golden.py from the reference) and the bounds both routes are held to.

Every bound is a figure the generator measured on the reference itself:

* >= 2 segments, float64: per window, elementwise |got - ref| <= 1e3 * max(spread, tolgap), where spread is the
  largest change of the reference's output among 8 one-ulp copies of the window and tolgap the largest change
  between the reference at tol and at tol * 1e-6.  Both are window maxima (the issue states the bound relative to
  the window's max |ds|, so one scale per window), and the factor 1e3 covers that 8 draws understate a worst
  case and that a direct-sum transform accumulates error ~F.  Iteration counts are equal where the generator
  found the reference's count robust.  A 2-segment scenario is compared only on pairs whose condition number is
  a factor 100 away from the branch threshold.
* >= 3 segments, float32: |got - ref32| <= 4 * max |ref32 - ref64| of the scenario, the reference's own
  single-precision error.
* 1 segment (the published shapes): per window ||got - ref||_F / ||ref||_F <= 10 * the largest such distance
  among the 8 one-ulp copies; finite, >= 0, exactly 0 on the diagonal.  Counts are not compared.
* power: the float64 rule without tolgap, the float32 rule.

The feature rows are float32 (the reference's items end in ``x.float()``), so the elementwise bounds on dir_spec
carry the rounding of that store on top: half a float32 ulp of the larger of |got| and |ref|.  ``power`` is
returned in float64 and carries no such term.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "dirspec.npz"))
META = json.loads(str(G["meta"]))
NAMES = list(META)


def scenario(name):
    sc = dict(META[name])
    for k in G.files:
        if k.startswith(name + "/"):
            sc[k.split("/", 1)[1]] = G[k]
    sc["csd_params"] = {"detrend": "constant", "window": "hann", "nperseg": sc["nperseg"], "noverlap": sc["noverlap"],
                        "nfft": None}
    sc["name"] = name
    return sc


def pairs(p):
    return [(a, b) for a in range(p) for b in range(a + 1, p)]


def check(sc, ds, power, status, iters, label):
    """ds [N, p, p, nf], power [N, tri, nf], status / iters [N, pairs] of one route against the fixture."""
    p, nseg, f32 = sc["p"], sc["segments"], sc["dtype"] == "float32"
    rows = sc["rows"]
    for n in range(sc["N"]):
        if n not in rows:
            assert np.isnan(ds[n]).all() and np.isnan(power[n]).all(), (label, sc["name"], "NaN window")
            assert (status[n] == 0).all() and (iters[n] == 0).all()
    for r, n in enumerate(rows):
        got, ref = ds[n].astype(np.float64), sc["ds"][r]
        gp, rp = power[n], sc["power"][r]
        assert np.isfinite(got).all() and (got >= 0).all(), (label, sc["name"])
        assert (got[np.arange(p), np.arange(p)] == 0).all()
        # power
        perr = np.abs(gp - rp).max()
        pbound = 4 * np.abs(sc["power"] - sc["p64"]).max() if f32 else 1e3 * sc["pspread"][r]
        print("%s %s window %d: power err %.3e bound %.3e" % (label, sc["name"], n, perr, pbound))
        assert perr <= pbound
        if nseg < 2:
            dist = np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel())
            bound = 10 * sc["dist"][:, r].max()
            print("%s %s window %d: frobenius %.3e bound %.3e" % (label, sc["name"], n, dist, bound))
            assert dist <= bound
            continue
        keep = np.ones(len(pairs(p)), bool) if nseg >= 3 else sc["margin"][r]
        assert not sc["singular"][r][keep].any()
        mask = np.zeros((p, p), bool)
        for q, (a, b) in enumerate(pairs(p)):
            mask[a, b] = mask[b, a] = keep[q]
        err = np.abs(got - ref)
        if f32:
            bound = 4 * np.abs(sc["ds"] - sc["ds64"]).max()
        else:
            bound = 1e3 * max(sc["spread"][r], sc["tolgap"][r])
        store = 0.5 * np.spacing(np.maximum(np.abs(got), np.abs(ref)).astype(np.float32)).astype(np.float64)
        print("%s %s window %d: ds err %.3e bound %.3e + store %.3e (max |ds| %.3e)"
              % (label, sc["name"], n, err[mask].max() if mask.any() else 0.0, bound, store.max(), np.abs(ref).max()))
        assert (err <= bound + store)[mask].all()
        if sc["max_iter"] < 1000:
            assert (status[n] == 1).all() and (iters[n] == sc["max_iter"]).all()
        else:
            sel = sc["flagged"][r] & keep
            assert (status[n][sel] == 0).all()
            assert np.array_equal(iters[n][sel], sc["iters"][r][sel]), (label, sc["name"], iters[n], sc["iters"][r])


def unpack(sc, out):
    """Feature rows [N, width] (vanilla) -> [N, p, p, nf]."""
    p = sc["p"]
    out = np.asarray(out)
    return out.reshape(out.shape[0], p, p, -1)
