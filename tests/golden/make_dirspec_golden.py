"""Generate tests/golden/dirspec.npz from the REFERENCE's directed-spectrum extraction (build container, CPU).

    python tests/golden/make_dirspec_golden.py

Every scenario is a small batch of autoregressive-noise windows X [N, T, p].  Each window goes through the
reference one at a time, as its data sets do: general_utils/time_series.py make_high_level_signal_features for
``power`` / ``freq`` and general_utils/directed_spectrum.py get_directed_spectrum (+ the same crop and frequency
scaling) for ``dir_spec``, so that max_iter and tol can be set.  Stored per scenario, besides the inputs and
the reference's outputs:

* ``iters`` / ``singular`` / ``flagged`` / ``margin`` [N, pairs]: Wilson iterations per pair, whether the
  reference warned "CPSD matrix is singular!" for it, whether its iteration count is robust (final relative
  change below tol / 10 with every earlier deciding change above 10 tol) and whether its largest condition
  number is a factor 100 away from the branch threshold;
* ``spread`` / ``pspread``: per window, the largest |output - reference| among 8 copies of the input moved by one
  ulp of its dtype (dir_spec and power), and ``dist`` [8, N], their relative Frobenius distances;
* ``tolgap`` (float64, >= 2 segments): per window max |ref(tol) - ref(tol * 1e-6)|;
* ``ds64`` / ``p64`` (float32 input): the reference's outputs on the same values in float64.

The generator asserts what the tests rely on: every single-segment pair warns "singular"; with >= 3 segments no
pair warns and every per-frequency condition number is below threshold / 100; a well-posed scenario has at
least 90 % of its pairs flagged when it has at most 3 (window, pair) problems, and FLOOR_MANY of them otherwise
(see SEEDS below for why 90 % is out of reach there).  Only arrays and a JSON description leave this script.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402

import_reference()
import importlib  # noqa: E402

DS = importlib.import_module("general_utils.directed_spectrum")
TS = importlib.import_module("general_utils.time_series")
MISC = importlib.import_module("general_utils.misc")

# name, p, N, T, nperseg, noverlap, dtype, fs, min_freq, max_freq, max_iter, tol, nan window
SCENARIOS = [
    ("ss8_p2_f32", 2, 1, 8, 8, 4, "float32", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("ss9_p3_f64", 3, 1, 9, 9, 0, "float64", 1000.0, 0.0, 600.0, 1000, 1e-6, None),
    ("pub20_p10_f32", 10, 5, 20, 20, 10, "float32", 1000.0, 0.0, 250.0, 1000, 1e-6, 2),
    ("pub50_p3_f64", 3, 1, 50, 50, 25, "float64", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("ss256_p2_f32", 2, 1, 256, 256, 128, "float32", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("two12_p3_f64", 3, 1, 20, 12, 6, "float64", 1000.0, 0.0, 600.0, 1000, 1e-6, None),
    ("wp9_p2_f64", 2, 1, 21, 9, 4, "float64", 1000.0, 0.0, 600.0, 1000, 1e-6, None),
    ("wp12_p3_f64", 3, 5, 25, 12, 6, "float64", 1000.0, 0.0, 600.0, 1000, 1e-6, 3),
    ("wp12_p3_f64_it3", 3, 1, 25, 12, 6, "float64", 1000.0, 0.0, 600.0, 3, 1e-6, None),
    ("wp12_p3_f64_tol", 3, 1, 25, 12, 6, "float64", 1000.0, 0.0, 600.0, 1000, 1e-3, None),
    ("wp20_p3_f32", 3, 5, 60, 20, 10, "float32", 1000.0, 60.0, 260.0, 1000, 1e-6, 0),
    ("wp20_p10_f32", 10, 1, 63, 20, 10, "float32", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("wp20_p10_f64", 10, 1, 63, 20, 10, "float64", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("wp50_p3_f32", 3, 1, 131, 50, 25, "float32", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("wp64_p2_f64", 2, 1, 197, 64, 0, "float64", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("wp65_p2_f32", 2, 1, 134, 65, 32, "float32", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("wp100_p2_f64", 2, 1, 207, 100, 50, "float64", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
    ("wp256_p2_f64", 2, 1, 522, 256, 128, "float64", 1000.0, 0.0, 250.0, 1000, 1e-6, None),
]


def ar_noise(rng, N, T, p):
    """Stable first-order vector autoregression with sparse cross-coupling, unit-variance channels."""
    A = 0.5 * np.eye(p) + 0.25 * (rng.rand(p, p) < 0.3) * rng.randn(p, p)
    A *= 0.8 / max(np.abs(np.linalg.eigvals(A)).max(), 0.8)
    X = np.zeros((N, T + 50, p))
    e = rng.randn(N, T + 50, p)
    for t in range(1, T + 50):
        X[:, t] = X[:, t - 1] @ A.T + e[:, t]
    X = X[:, 50:]
    return X / X.std(axis=(0, 1), keepdims=True)


class Probe:
    """Counts the reference's iterations and records its decisions, one entry per _wilson_factorize call."""

    def __init__(self):
        self.calls = []
        self._wf, self._cc = DS._wilson_factorize, DS._check_convergence

    def __enter__(self):
        probe = self

        def check(x, x0, tol):
            ok = probe._cc(x, x0, tol)
            d = np.abs(x - x0)
            a = np.abs(x)
            a[a <= 2 * np.finfo(a.dtype).eps] = 1
            cur = probe.calls[-1]
            if x.ndim == 3:
                cur["steps"].append([float((d / a).max()), None, bool(ok)])
            else:
                cur["steps"][-1][1] = float((d / a).max())
                cur["steps"][-1][2] = bool(ok)
            return ok

        def wf(cpsd, max_iter, tol, *a, **k):
            probe.calls.append({"steps": [], "cond": float(np.linalg.cond(cpsd).max()),
                                "thr": float(1 / np.finfo(cpsd.dtype).eps), "tol": tol})
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                out = probe._wf(cpsd, max_iter, tol, *a, **k)
            probe.calls[-1]["singular"] = any("singular" in str(x.message) for x in w)
            return out

        DS._wilson_factorize, DS._check_convergence = wf, check
        return self

    def __exit__(self, *exc):
        DS._wilson_factorize, DS._check_convergence = self._wf, self._cc


def robust(call):
    """The iteration count does not hinge on rounding: the last step passes both tests by 10x, every earlier
    step fails its deciding test by 10x."""
    steps, tol = call["steps"], call["tol"]
    if not steps or not steps[-1][2]:
        return False
    last = steps[-1]
    if not (last[0] < tol / 10 and last[1] is not None and last[1] < tol / 10):
        return False
    for s in steps[:-1]:
        deciding = s[0] if s[1] is None else (s[0] if s[0] >= tol else s[1])
        if not deciding > 10 * tol:
            return False
    return True


def reference_window(x, sc, tol=None):
    """x [T, p] -> (dir_spec [p, p, nf], power [tri, nf], freq, calls)."""
    _, p, N, T, nper, nov, dt, fs, fmin, fmax, max_iter, tol0, _ = sc
    tol = tol0 if tol is None else tol
    par = {"detrend": "constant", "window": "hann", "nperseg": nper, "noverlap": nov, "nfft": None}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        feats = TS.make_high_level_signal_features(x.copy(), fs=fs, min_freq=fmin, max_freq=fmax, directed_spectrum=False,
                                                   csd_params=par)
        Xw = np.expand_dims(x.copy().T, axis=0)
        with Probe() as pr:
            f, ds = DS.get_directed_spectrum(Xw, fs, max_iter=max_iter, tol=tol, csd_params=par)
    i1, i2 = np.searchsorted(f, [fmin, fmax])
    ds = ds[:, i1:i2] * f[i1:i2].reshape(1, -1, 1, 1)
    ds = np.moveaxis(ds, 1, -1)[0]
    assert np.allclose(f[i1:i2], feats["freq"])
    return ds, feats["power"][0], feats["freq"], pr.calls


def one_ulp(x, rng):
    up = rng.rand(*x.shape) < 0.5
    return np.where(up, np.nextafter(x, np.array(np.inf, x.dtype)), np.nextafter(x, np.array(-np.inf, x.dtype))).astype(x.dtype)


def frob(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def build(sc, seed):
    name, p, N, T, nper, nov, dt, fs, fmin, fmax, max_iter, tol, nan_at = sc
    rng = np.random.RandomState(seed)
    X = ar_noise(rng, N, T, p).astype(dt)
    nseg = (T - nov) // (nper - nov)
    npairs = p * (p - 1) // 2
    out = {"X": X.copy()}
    ds_all, pw_all, it_all, sg_all, fl_all, mg_all = [], [], [], [], [], []
    spread, pspread, tolgap, dist = [], [], [], []
    ds64, p64 = [], []
    for n in range(N):
        if nan_at == n:
            continue
        ds, pw, freq, calls = reference_window(X[n], sc)
        assert len(calls) == npairs
        out["freq"] = freq
        ds_all.append(ds)
        pw_all.append(pw)
        it_all.append([len(c["steps"]) for c in calls])
        sg_all.append([c["singular"] for c in calls])
        fl_all.append([robust(c) for c in calls])
        mg_all.append([c["cond"] < c["thr"] / 100 or c["cond"] > c["thr"] * 100 for c in calls])
        if nseg < 2:
            assert all(c["singular"] for c in calls), name
        if nseg >= 3:
            assert not any(c["singular"] for c in calls), name
            assert all(c["cond"] < c["thr"] / 100 for c in calls), (name, max(c["cond"] for c in calls))
        r2 = np.random.RandomState(1000 + seed + n)
        sp, ps, di = 0.0, 0.0, []
        for _ in range(8):
            d2, p2, _, _ = reference_window(one_ulp(X[n], r2), sc)
            sp = max(sp, float(np.abs(d2 - ds).max()))
            ps = max(ps, float(np.abs(p2 - pw).max()))
            di.append(frob(d2, ds))
        spread.append(sp)
        pspread.append(ps)
        dist.append(di)
        if dt == "float32":
            d64, q64, _, _ = reference_window(X[n].astype(np.float64), sc)
            ds64.append(d64)
            p64.append(q64)
        elif nseg >= 2:
            d12, _, _, _ = reference_window(X[n], sc, tol=tol * 1e-6)
            tolgap.append(float(np.abs(d12 - ds).max()))
    keep = [n for n in range(N) if n != nan_at]
    out["rows"] = np.array(keep)
    out["ds"], out["power"] = np.stack(ds_all), np.stack(pw_all)
    out["iters"], out["singular"], out["flagged"] = np.array(it_all), np.array(sg_all), np.array(fl_all)
    out["margin"] = np.array(mg_all)
    out["spread"], out["pspread"], out["dist"] = np.array(spread), np.array(pspread), np.array(dist).T
    if ds64:
        out["ds64"], out["p64"] = np.stack(ds64), np.stack(p64)
    if tolgap:
        out["tolgap"] = np.array(tolgap)
    if nan_at is not None:
        out["X"][nan_at, T // 2, p - 1] = np.nan
    ok = True
    if nseg >= 3 and max_iter >= 1000:
        ok = out["flagged"].mean() >= 0.9
    return out, ok


# Wilson's iteration converges quadratically, so a pair's last changes look like e, e^2: its count is robust
# (previous change above 10 tol, final below tol / 10) unless the previous change falls in (tol, 10 tol], about one
# decade of the three it is spread over.  Roughly two pairs in three are robust, and a scenario with many
# (window, pair) problems cannot reach 90 %: those take the best of SEEDS seeds and must reach FLOOR_MANY.
SEEDS = 24
FLOOR_MANY = 0.6


def main():
    store, meta = {}, {}
    for i, sc in enumerate(SCENARIOS):
        best = None
        for seed in range(100 * i, 100 * i + SEEDS):
            out, ok = build(sc, seed)
            if best is None or out["flagged"].mean() > best[0]["flagged"].mean():
                best = (out, seed)
            if ok:
                break
        out, seed = best
        problems = out["flagged"].size
        nseg = (sc[3] - sc[5]) // (sc[4] - sc[5])
        if nseg >= 3 and sc[10] >= 1000:
            # at tol = 1e-3 a robust count needs e > 1e-2 and e^2 < 1e-4 at once: rare, so the lower floor
            floor = 0.9 if problems <= 3 and sc[11] <= 1e-6 else FLOOR_MANY
            assert out["flagged"].mean() >= floor, (sc[0], float(out["flagged"].mean()))
        name = sc[0]
        for k, v in out.items():
            store["%s/%s" % (name, k)] = v
        meta[name] = dict(zip(("p", "N", "T", "nperseg", "noverlap", "dtype", "fs", "min_freq", "max_freq", "max_iter", "tol",
                               "nan_window"), sc[1:]))
        meta[name]["seed"] = seed
        meta[name]["segments"] = (sc[3] - sc[5]) // (sc[4] - sc[5])
        print(name, "seed", seed, "iters", out["iters"].min(), out["iters"].max(), "flagged %.2f" % out["flagged"].mean(),
              "singular %.2f" % out["singular"].mean(), "spread %.2e" % (out["spread"] / np.abs(out["ds"]).max()).max(),
              "dist %.2e" % out["dist"].max())
    # the reference's flattened layout of one window, for the layout test
    x = store["wp20_p3_f32/ds"][0]
    store["flat/in"] = x
    store["flat/out"] = MISC.flatten_directed_spectrum_features(x)
    store["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "dirspec.npz")
    np.savez_compressed(path, **store)
    print("wrote dirspec.npz (%d arrays, %d bytes)" % (len(store), os.path.getsize(path)))


if __name__ == "__main__":
    main()
