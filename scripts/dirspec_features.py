"""Time of the directed-spectrum feature extraction (redcliff_amd.directed_spectrum_features) on one MI355X: the
device route (redcliff_dirspec_run, csrc/rc_dirspec.hip) against the host route of the same commit on the same
box, one process.

Shapes, 4,096 seeded autoregressive-noise windows each (float64, as the data sets hand them over):
  d4ic    p 10, T 20, nperseg 20, noverlap 10, fs 1000, bins in [0, 250) Hz   (train/DCSFANMF_d4IC_OBPgs1: one segment)
  synsys  p 12, T 50, nperseg 50, noverlap 25, fs 1000, bins in [0, 250) Hz   (the 12-channel synthetic systems: one segment)
  wellposed  p 10, T 60, nperseg 20, noverlap 10                              (five segments)
Protocol: one warm-up call, then --reps calls between two HIP events on the stream; median [min - max].  The host
route is timed once on the first --host-windows windows and scaled to 4,096 (it is a per-window loop; the
scaling is stated in the output).  Recorded with the times: the histogram of Wilson iterations per (window, pair),
the status counts, and the library's build id.  No per-kernel split is recorded here: the extraction has no ids in
redcliff_kernel_timing's table; a kernel trace of this script (--reps 3 --host-windows 2) gives it
(profiles/dirspec_kernel_stats.csv).
Writes profiles/dirspec_features.json (or --out)."""
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
for _p in (ROOT, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SHAPES = {
    "d4ic": dict(p=10, T=20, nperseg=20, noverlap=10),
    "synsys": dict(p=12, T=50, nperseg=50, noverlap=25),
    "wellposed": dict(p=10, T=60, nperseg=20, noverlap=10),
}
FS, FMIN, FMAX = 1000.0, 0.0, 250.0


def windows(seed, N, T, p):
    rng = np.random.RandomState(seed)
    A = 0.5 * np.eye(p) + 0.25 * (rng.rand(p, p) < 0.3) * rng.randn(p, p)
    A *= 0.8 / max(np.abs(np.linalg.eigvals(A)).max(), 0.8)
    X = np.zeros((N, T + 50, p))
    e = rng.randn(N, T + 50, p)
    for t in range(1, T + 50):
        X[:, t] = X[:, t - 1] @ A.T + e[:, t]
    X = X[:, 50:]
    return X / X.std(axis=(0, 1), keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--host-windows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dirspec_features.json"))
    args = ap.parse_args()
    from redcliff_amd import _native as nat
    from redcliff_amd import directed_spectrum as D
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(), "windows": args.windows, "reps": args.reps,
           "dtype": "float64", "shapes": {}}
    for name, sh in SHAPES.items():
        par = {"detrend": "constant", "window": "hann", "nperseg": sh["nperseg"], "noverlap": sh["noverlap"], "nfft": None}
        X = windows(11, args.windows, sh["T"], sh["p"])
        Xd = torch.from_numpy(X).cuda()
        call = lambda: D.directed_spectrum_features(Xd, FS, FMIN, FMAX, par, return_info=True)  # noqa: E731
        os.environ["REDCLIFF_DIRSPEC_PATH"] = "fused"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out, info = call()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                call()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            os.environ["REDCLIFF_DIRSPEC_PATH"] = "host"
            nh = min(args.host_windows, args.windows)
            t0 = time.perf_counter()
            hout, hinfo = D.directed_spectrum_features(X[:nh], FS, FMIN, FMAX, par, return_info=True)
            host_s = time.perf_counter() - t0
        dev = out[:nh].cpu().numpy().astype(np.float64)
        rel = float(np.linalg.norm(dev - hout) / np.linalg.norm(hout))
        its = info["iterations"].ravel()
        hist = np.bincount(its)
        res["shapes"][name] = {
            **sh, "fs": FS, "min_freq": FMIN, "max_freq": FMAX, "segments": (sh["T"] - sh["noverlap"]) // (sh["nperseg"] - sh["noverlap"]),
            "problems": int(its.size), "features_per_window": int(out.shape[1]),
            "device_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "samples": ms,
                          "note": "events around the whole call: workspace allocation, three launches (no power features asked for), status read-back"},
            "host_s": {"windows_timed": nh, "seconds": host_s, "scaled_to_all_windows_s": host_s * args.windows / nh,
                       "note": "timed on the first %d windows and scaled by %d / %d" % (nh, args.windows, nh)},
            "device_vs_host_rel_frobenius_first_windows": rel,
            "iterations_histogram": {str(i): int(c) for i, c in enumerate(hist) if c},
            "status_counts": {str(k): int((info["status"] == k).sum()) for k in (0, 1, 2)},
        }
        print(name, json.dumps(res["shapes"][name]["device_ms"]["median"]), "ms device;", host_s * args.windows / nh, "s host (scaled)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
