"""Time of the regime-aware SLARAC and QRBS baselines (redcliff_amd.tidybench) on one MI355X: the device route
(redcliff_tidybench_run, csrc/rc_tidybench.hip) against the host route of the same commit on the same box, one
process.

Shapes: 5 regime-masked copies of one seeded regime-switching VAR(1) series in one ``*_many`` call, default fit
counts (SLARAC 1 + 200 fits, QRBS 600 resamples) per regime:
  pub10   N 10, lags 1     pub12   N 12, lags 1     large_d   N 12, lags 5 (D = 61)
T = 40,000 rows is an ASSUMED size: 2,000 windows of 20 steps.  The aggregated pickles the evaluation scripts
read are not available here, so the row count is not the published one.
Protocol: one warm-up call, then --reps seeded calls; the median of the end-to-end wall time (the call ends in a
device synchronise and the read-back) and of each part the call reports itself: host draws, index upload, kernels
(HIP events around the native calls), SINGULAR fall-backs, host aggregation.  The host route is timed once on a
reduced fit count (--host-subsamples / --host-resamples) and scaled to the default count; the scaling is stated
in the output.  Device and host results of that reduced, equally seeded call are compared.
Writes profiles/tidybench_scores.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SHAPES = {"pub10": dict(N=10, lags=1), "pub12": dict(N=12, lags=1), "large_d": dict(N=12, lags=5)}
REGIMES, WINDOW = 5, 20


def masked_series(seed, T, N):
    rng = np.random.RandomState(seed)
    A = []
    for _ in range(REGIMES):
        a = 0.45 * np.eye(N) + 0.25 * rng.randn(N, N) * (rng.rand(N, N) < 2.0 / N)
        A.append(a / max(1.0, np.abs(np.linalg.eigvals(a)).max() / 0.8))
    regime = np.repeat(rng.randint(0, REGIMES, size=T // WINDOW), WINDOW)
    e = rng.randn(T, N)
    x = np.zeros((T, N))
    for t in range(1, T):
        x[t] = A[regime[t]].dot(x[t - 1]) + e[t]
    return np.stack([x * (regime == r)[:, None] for r in range(REGIMES)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-subsamples", type=int, default=4)
    ap.add_argument("--host-resamples", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tidybench_scores.json"))
    args = ap.parse_args()
    from redcliff_amd import _native as nat
    from redcliff_amd import tidybench as tb
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(), "rows": args.rows, "reps": args.reps,
           "regimes": REGIMES, "rows_note": "assumed size: %d windows of %d steps; the aggregated pickles are not available" %
           (args.rows // WINDOW, WINDOW), "shapes": {}}
    for name, sh in SHAPES.items():
        x = masked_series(11, args.rows, sh["N"])
        entry = dict(sh, D=sh["N"] * sh["lags"] + 1)
        for alg in ("slarac", "qrbs"):
            if alg == "slarac":
                full, few = dict(maxlags=sh["lags"]), dict(maxlags=sh["lags"], n_subsamples=args.host_subsamples)
                fn, scale = tb.slarac_many, 201.0 / (1 + args.host_subsamples)
            else:
                full, few = dict(lags=sh["lags"]), dict(lags=sh["lags"], n_resamples=args.host_resamples)
                fn, scale = tb.qrbs_many, 600.0 / args.host_resamples
            os.environ["REDCLIFF_TIDYBENCH_PATH"] = "fused"
            np.random.seed(1)
            fn(x, return_info=True, **full)
            runs = []
            for rep in range(args.reps):
                np.random.seed(2 + rep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, info = fn(x, return_info=True, **full)
                wall = time.perf_counter() - t0
                runs.append(dict(info["time"], wall=wall))
            med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
            np.random.seed(7)
            dev_few, _ = fn(x, return_info=True, **few)
            os.environ["REDCLIFF_TIDYBENCH_PATH"] = "host"
            np.random.seed(7)
            t0 = time.perf_counter()
            host_few, hinfo = fn(x, return_info=True, **few)
            host_s = time.perf_counter() - t0
            draws_few = hinfo["time"]["draws"]
            entry[alg] = {
                "fits_per_regime": int(info["status"].shape[1]), "groups": int(info["groups"]),
                "status_counts": {str(k): int((info["status"] == k).sum()) for k in (0, 1, 2)},
                "device_s": {"median": med, "samples": runs,
                             "note": "wall = the whole call; draws, upload, kernels, fallback, aggregate as the call reports them"},
                "host_s": {"fits_timed_per_regime": int(hinfo["status"].shape[1]), "seconds": host_s, "draws_seconds": draws_few,
                           "scaled_to_default_count_s": host_s * scale,
                           "note": "timed on the reduced fit count and scaled by %.2f (fits are independent and alike)" % scale},
                "host_over_device": host_s * scale / med["wall"],
                "host_fits_over_device_kernels": (host_s - draws_few) * scale / med["kernels"],
                "device_vs_host_rel_max": float(np.abs(dev_few - host_few).max() / np.abs(host_few).max()),
            }
            print(name, alg, "device %.3f s (draws %.3f upload %.3f kernels %.4f fallback %.3f aggregate %.3f); host %.2f s (scaled)"
                  % (med["wall"], med["draws"], med["upload"], med["kernels"], med["fallback"], med["aggregate"], host_s * scale))
        res["shapes"][name] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
