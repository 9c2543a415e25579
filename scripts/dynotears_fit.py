"""Time of the DYNOTEARS baseline (redcliff_amd.dynotears_vanilla) on one MI355X: the device route
(redcliff_dynotears_run, csrc/rc_dynotears.hip) against the host route (the reference's loop on scipy's L-BFGS-B) of
the same commit on the same box, one process.

Shapes (recordings from the generator of tests/golden/make_dynotears_golden.py: seeded stable VAR(1), z-scored per
channel, float32, resident on the device):
  d4ic   --count recordings of shape (21, 10), lambda 0.1, lag_size 1: the D4IC recording shape.  The COUNT IS AN
         ASSUMPTION (default 1,024): the D4IC data sets are not available here.
  d12    --count recordings of shape (50, 12), lambda 0.1.
  sets   15 data sets of --set-count recordings of the D4IC shape with 15 lambdas, fitted by one
         fit_dynotears_baselines call and by a loop of 15 calls.
Protocol: one warm-up call per shape, then --reps calls; median [min - max] of the device time (HIP events around
all launches of a call, which the call reports) and of the wall time of the whole call (upload of the small
per-problem arrays, launches, the read-back of the counter after every launch, download).  The host route is timed
on --host-count recordings and scaled to the count (recordings are independent and alike).  The evals_per_launch
sweep repeats the d4ic call at each value; the default is the smallest value whose device time is within 5 % of the
largest value's.  Writes profiles/dynotears_fit.json (or --out)."""
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


def mmm(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn, reps):
    fn()
    dev, wall, info = [], [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = fn()
        wall.append(time.perf_counter() - t0)
        dev.append(info["kernel_ms"] / 1e3)
    return {"device_s": mmm(dev), "wall_s": mmm(wall)}, info


def describe(info):
    ev = info["counts"]["evaluations"]
    return {
        "launches": int(info["launches"]), "evals_per_launch": int(info["evals_per_launch"]),
        "device_ms_per_launch": info["kernel_ms"] / info["launches"],
        "status_counts": {n: int((info["status"] == k).sum()) for k, n in enumerate(info["status_names_all"])},
        "evaluations": {"min": int(ev.min()), "p50": float(np.percentile(ev, 50)), "p90": float(np.percentile(ev, 90)),
                        "p99": float(np.percentile(ev, 99)), "max": int(ev.max()), "mean": float(ev.mean())},
        "inner_solves_mean": float(info["counts"]["inner_solves"].mean()),
        "problems_with_nonfinite_trial": int((info["counts"]["nonfinite_trials"] > 0).sum()),
        "nonfinite_trials": int(info["counts"]["nonfinite_trials"].sum()),
        "first_problems_with_nonfinite_trial": [int(i) for i in np.nonzero(info["counts"]["nonfinite_trials"] > 0)[0][:16]],
        "failed_line_searches": float(info["stats"]["failed_line_searches"].sum()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--set-count", type=int, default=128)
    ap.add_argument("--host-count", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep", type=int, nargs="*", default=[32, 64, 128, 256, 512, 1024, 2048, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynotears_fit.json"))
    args = ap.parse_args()
    from redcliff_amd import _native as nat
    from redcliff_amd import dynotears_vanilla as dy
    if not torch.cuda.is_available():
        raise SystemExit("dynotears_fit.py measures on the GPU; none is visible")
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(), "reps": args.reps, "count": args.count,
           "count_note": "assumed: the D4IC data sets are not available here, so the number of training recordings is not the "
                         "published one", "default_evals_per_launch": dy.DEFAULT_EVALS_PER_LAUNCH, "shapes": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    def many(data, lam, path="fused", **kw):
        os.environ["REDCLIFF_DYNOTEARS_PATH"] = path
        _, _, info = dy.from_numpy_dynamic_many(data[:, :-1], data[:, 1:], lam, lam, **kw)
        info["status_names_all"] = dy.STATUS_NAMES
        return info

    for name, (d, T) in {"d4ic": (10, 21), "d12": (12, 50)}.items():
        host = np.stack([make_recording(5000 + s, d, T) for s in range(args.count)])
        data = torch.from_numpy(host).cuda()
        t, info = timed(lambda: many(data, 0.1), args.reps)
        entry = dict(d=d, T=T, lam=0.1, recordings=args.count, **t, **describe(info))
        t0 = time.perf_counter()
        hinfo = many(host[:args.host_count], 0.1, path="host")
        hs = time.perf_counter() - t0
        scale = args.count / float(args.host_count)
        entry["host"] = {"recordings_timed": args.host_count, "seconds": hs, "scaled_to_count_s": hs * scale,
                         "evaluations_mean": float(hinfo["counts"]["evaluations"].mean()),
                         "note": "timed on %d recordings and scaled by %g" % (args.host_count, scale)}
        entry["host_scaled_over_device_wall"] = hs * scale / t["wall_s"]["median"]
        dinfo = many(data[:args.host_count], 0.1)
        diff = np.abs(dinfo["wa"] - hinfo["wa"]).max(axis=1)
        entry["device_vs_host_max_abs_per_recording"] = {
            "sorted": [float(v) for v in np.sort(diff)], "median": float(np.median(diff)), "max": float(diff.max()),
            "note": "unselected recordings: unlike the fixture's, they are not filtered for being well posed"}
        print(name, "device %.3f s [%.3f - %.3f], wall %.3f s; host %.1f s scaled; %d launches; evaluations p50 %.0f max %d" % (
            t["device_s"]["median"], t["device_s"]["min"], t["device_s"]["max"], t["wall_s"]["median"], hs * scale, entry["launches"],
            entry["evaluations"]["p50"], entry["evaluations"]["max"]), flush=True)
        if name == "d4ic":
            sweep = []
            for epl in args.sweep:
                ts, si = timed(lambda: many(data, 0.1, evals_per_launch=epl), args.reps)
                sweep.append(dict(evals_per_launch=epl, launches=int(si["launches"]), **ts))
                print("  evals_per_launch %5d: %4d launches, device %.4f s, wall %.4f s" % (epl, si["launches"], ts["device_s"]["median"],
                                                                                           ts["wall_s"]["median"]), flush=True)
            best = sweep[-1]["wall_s"]["median"]
            for s in sweep:
                s["wall_over_largest"] = s["wall_s"]["median"] / best
            ok = [s["evals_per_launch"] for s in sweep if s["wall_over_largest"] <= 1.05]
            entry["evals_per_launch_sweep"] = sweep
            entry["smallest_within_5_percent"] = min(ok) if ok else None
        res["shapes"][name] = entry
        save()
        del data

    # 15 data sets with 15 lambdas: one batch against a loop of calls
    lams = [0.01 * (k + 1) for k in range(15)]
    sets = [torch.from_numpy(np.stack([make_recording(9000 + 1000 * k + s, 10, 21) for s in range(args.set_count)])).cuda() for k in range(15)]
    os.environ["REDCLIFF_DYNOTEARS_PATH"] = "fused"

    def one_call():
        models = [dy.DYNOTEARS_Model(lambda_w=lam, lambda_a=lam) for lam in lams]
        dy.fit_dynotears_baselines(models, sets)
        return models

    def loop():
        models = [dy.DYNOTEARS_Model(lambda_w=lam, lambda_a=lam) for lam in lams]
        for m, x in zip(models, sets):
            dy.fit_dynotears_baselines([m], [x])
        return models

    walls = {"one_call": [], "loop_of_15": []}
    a = one_call()
    b = loop()
    same = all(np.array_equal(x.GC(), y.GC()) for x, y in zip(a, b))
    for _ in range(args.reps):
        for key, fn in (("one_call", one_call), ("loop_of_15", loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            walls[key].append(time.perf_counter() - t0)
    res["sets"] = {"data_sets": 15, "recordings_each": args.set_count, "lambdas": lams, "bitwise_equal": bool(same),
                   "wall_s": {k: mmm(v) for k, v in walls.items()}}
    print("15 data sets: one call %.3f s, loop of 15 calls %.3f s, equal bits %s" % (
        res["sets"]["wall_s"]["one_call"]["median"], res["sets"]["wall_s"]["loop_of_15"]["median"], same), flush=True)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
