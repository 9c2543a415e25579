"""Time of the regime-aware LASAR baseline (redcliff_amd.tidybench.lasar_many) on one MI355X: the device route
(redcliff_lasar_run, csrc/rc_lasar.hip) against the host route of the same commit on the same box, one process.

Shapes: 5 regime-masked copies of one seeded regime-switching VAR(1) series in one ``lasar_many`` call, default
counts (1 + 100 fits of N targets, cv = 5) per regime:   pub10   N 10     pub12   N 12     (maxlags 1)
T = 40,000 rows is the ASSUMED size scripts/tidybench_scores.py uses (2,000 windows of 20 steps); the aggregated
pickles the evaluation scripts read are not available here.
Protocol: one warm-up call, then --reps seeded calls; the median of the end-to-end wall time (the call ends in a
device synchronise and the read-back) and of each part the call reports itself: host draws, index upload, kernels
(HIP events around the native calls), SINGULAR / DEGENERATE fall-backs, host aggregation.  The host route is timed
once on a reduced count (--host-subsamples) and scaled to the default count; the scaling is stated in the output.
Device and host results of that reduced, equally seeded call are compared.  Where sklearn and the reference tree are
importable the reference's own ``lasar`` is timed on the same reduced count as well.
Writes profiles/lasar_scores.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tidybench_scores import REGIMES, WINDOW, masked_series  # noqa: E402

SHAPES = {"pub10": dict(N=10), "pub12": dict(N=12)}


def reference_lasar():
    try:
        import importlib

        from oracle import ref_import
        if ref_import.REF_ROOT not in sys.path:
            sys.path.insert(0, ref_import.REF_ROOT)
        return importlib.import_module("tidybench.lasar").lasar
    except Exception:   # no sklearn or no reference tree on this box
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-subsamples", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lasar_scores.json"))
    args = ap.parse_args()
    from redcliff_amd import _native as nat
    from redcliff_amd import tidybench as tb
    ref = reference_lasar()
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(), "rows": args.rows, "reps": args.reps,
           "regimes": REGIMES, "rows_note": "assumed size: %d windows of %d steps; the aggregated pickles are not available" %
           (args.rows // WINDOW, WINDOW), "shapes": {}}
    scale = 101.0 / (1 + args.host_subsamples)
    few = dict(n_subsamples=args.host_subsamples)
    for name, sh in SHAPES.items():
        x = masked_series(11, args.rows, sh["N"])
        os.environ["REDCLIFF_TIDYBENCH_PATH"] = "fused"
        np.random.seed(1)
        tb.lasar_many(x, return_info=True)
        runs = []
        for rep in range(args.reps):
            np.random.seed(2 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, info = tb.lasar_many(x, return_info=True)
            runs.append(dict(info["time"], wall=time.perf_counter() - t0))
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        np.random.seed(7)
        dev_few, dinfo = tb.lasar_many(x, return_info=True, **few)
        os.environ["REDCLIFF_TIDYBENCH_PATH"] = "host"
        np.random.seed(7)
        t0 = time.perf_counter()
        host_few, hinfo = tb.lasar_many(x, return_info=True, **few)
        host_s = time.perf_counter() - t0
        ref_s = None
        if ref is not None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                np.random.seed(7)
                t0 = time.perf_counter()
                for r in range(REGIMES):
                    ref(x[r].copy(), **few)
                ref_s = time.perf_counter() - t0
        entry = dict(sh, maxlags=1, cv=5)
        entry.update({
            "fits_per_regime": int(info["status"].shape[1]), "groups": int(info["groups"]),
            "status_counts": {str(k): int((info["status"] == k).sum()) for k in (0, 1, 2, 3)},
            "device_s": {"median": med, "samples": runs, "host_side_share": 1.0 - med["kernels"] / med["wall"],
                         "note": "wall = the whole call; draws, upload, kernels, fallback, aggregate as the call reports them"},
            "host_s": {"fits_timed_per_regime": 1 + args.host_subsamples, "seconds": host_s, "draws_seconds": hinfo["time"]["draws"],
                       "scaled_to_default_count_s": host_s * scale,
                       "note": "timed on the reduced count and scaled by %.2f (fits are independent and alike)" % scale},
            "reference_s": None if ref_s is None else {"seconds": ref_s, "scaled_to_default_count_s": ref_s * scale},
            "host_over_device": host_s * scale / med["wall"],
            "host_fits_over_device_kernels": (host_s - hinfo["time"]["draws"]) * scale / med["kernels"],
            "device_vs_host_rel_max": float(np.abs(dev_few - host_few).max() / np.abs(host_few).max()),
            "device_vs_host_same_selection": bool((dinfo["selected"] == hinfo["selected"]).all() and
                                                  (dinfo["best_index"] == hinfo["best_index"]).all()),
        })
        print(name, "device %.3f s (draws %.3f upload %.3f kernels %.4f fallback %.3f aggregate %.3f); host %.1f s (scaled); "
              "statuses %s" % (med["wall"], med["draws"], med["upload"], med["kernels"], med["fallback"], med["aggregate"],
                               host_s * scale, entry["status_counts"]), flush=True)
        res["shapes"][name] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
