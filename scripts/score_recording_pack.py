"""Time of scoring whole recordings with MANY same-shape DGCNN REDCLIFF-S models on one MI355X: one
packed call (redcliff_amd.score_recordings -> redcliff_score_recording_pack, csrc/rc_score.hip)
against the loop of model.score_recording calls it replaces.

Workloads (shapes: the bench's d4ic and c4 (TST) embedders; seeded models and recordings):
  a  128 d4ic models, 8 shared recordings of 2,048 steps, scores
  b  128 d4ic models, 1 recording of 2,048 steps, scores + graph trace (graphs="sum")
  c  128 c4 models,   8 shared recordings of 2,048 steps, scores
  d    5 d4ic models, 1 recording of 131,072 steps, scores (cross-validation folds; one model
       already fills the GPU)
Routes:
  loop  [m.score_recording(X, ...) for m in models]: R calls, each with its own prologue and launch
  pack  score_recordings(models, X, ...): one prologue and one window-kernel launch for all R
Protocol (scripts/score_recording_cemb.py): per workload one warm-up of both routes, then --reps runs
of each between two HIP events on the stream, the two routes alternated; median [min - max].  The
host time a route takes to enqueue its work is recorded beside it (not gated).
Acceptance: on a, b and c the pack beats the loop by more than the two min-max spreads added
together; on d the pack is not slower than the loop by more than that sum.

Also recorded: the number of elements in which the two routes' results differ on the timed sizes
(must be 0), the packed k_score_windows time (redcliff_kernel_times), its TF/s from
bench.flops_per_window(c)["emb_fwd"] and its share of the 157.3 TF/s fp32 peak, beside the same
figures of the loop's R launches.  --single-sha FILE writes the SHA-256 of w / logits / graphs of the
single-model entry for one seeded model and recording per shape (run once per library, selected with
REDCLIFF_HIP_LIB, to show that a refactoring left redcliff_score_recording's bits alone).
Writes profiles/score_recording_pack.json (or --out)."""
import argparse
import hashlib
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

import bench  # noqa: E402

FP32_PEAK_TFLOPS = 157.3
# name: (config, R, recordings, steps, graph trace, the pack must be faster)
WORKLOADS = {
    "a": ("d4ic", 128, 8, 2048, False, True),
    "b": ("d4ic", 128, 1, 2048, True, True),
    "c": ("c4", 128, 8, 2048, False, True),
    "d": ("d4ic", 5, 1, 131072, False, False),
}


def event_ms(fn):
    """(ms between two HIP events around fn, host ms fn took to enqueue its work)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    return a.elapsed_time(b), host


def summary(s):
    return {"median_ms": statistics.median(s), "min_ms": min(s), "max_ms": max(s), "spread_ms": max(s) - min(s),
            "samples_ms": s}


def recordings(nrec, steps, F, p, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(nrec, steps + F, p).astype(np.float32)
    X[:, 1:] += 0.4 * X[:, :-1]
    return torch.from_numpy(X).cuda()


def models_of(name, R):
    import redcliff_amd
    out = []
    for s in range(R):
        m = bench.build_model(redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing, bench.CONFIGS[name], seed=s).float().cuda()
        m.eval()
        out.append(m)
    return out


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def single_sha(path):
    """SHA-256 of the single-model entry's outputs: one seeded model and recording per shape."""
    from redcliff_amd import _native as nat
    out = {"lib": os.environ.get("REDCLIFF_HIP_LIB", "in-tree"), "shapes": {}}
    for name in ("d4ic", "c4"):
        c = bench.CONFIGS[name]
        m = models_of(name, 1)[0]
        X = recordings(3, 1000, c["F"], c["p"], seed=3)
        res = m.score_recording(X, start=c["F"] + 1, count=997, graphs="sum", ignore_lag=False)
        s4 = m.score_recording(X[0], start=c["F"], count=200, stride=5)
        out["shapes"][name] = {"w": sha(res.w), "logits": sha(res.logits), "graphs": sha(res.graphs),
                               "stride5_w": sha(s4.w), "stride5_logits": sha(s4.logits)}
    out["abi"] = nat.lib().redcliff_abi_version()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--single-sha", default=None, metavar="FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_recording_pack.json"))
    args = ap.parse_args()
    from redcliff_amd import _native as nat
    from redcliff_amd import scoring
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.single_sha:
        return single_sha(args.single_sha)
    res = {"reps": args.reps, "warmup": args.warmup, "build_id": nat.build_id(), "device": torch.cuda.get_device_name(0),
           "workloads": {}}
    if os.path.exists(args.out):  # a run over part of the workloads keeps the others
        with open(args.out) as f:
            old = json.load(f)
        res["workloads"] = old.get("workloads", {})
        for k in ("single_model_bits",):
            if k in old:
                res[k] = old[k]

    def write():  # after every measurement: an interrupted run keeps what it has
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    names = args.workloads.split(",")
    cases, pool = {}, {}
    for wl in names:
        name, R, nrec, steps, trace, _ = WORKLOADS[wl]
        c = bench.CONFIGS[name]
        if (name, R) not in pool:
            pool[name, R] = models_of(name, R)
        models = pool[name, R]
        assert scoring.pack_available(models)
        X = recordings(nrec, steps, c["F"], c["p"], seed=3)
        kw = dict(start=c["F"], count=steps, graphs="sum" if trace else None)
        routes = {"loop": (lambda models=models, X=X, kw=kw: [m.score_recording(X, **kw) for m in models]),
                  "pack": (lambda models=models, X=X, kw=kw: scoring.score_recordings(models, X, **kw))}
        cases[wl] = (c, models, X, routes)
    ok = True
    for wl in names:
        # warm-up of both routes at this shape; the bits of the two routes on the timed sizes
        c, models, X, routes = cases[wl]
        last = {}
        for _ in range(max(args.warmup, 1)):
            for k, fn in routes.items():
                last[k] = fn()
        differing = 0
        for r, one in enumerate(last["loop"]):
            for a, b in zip(one, last["pack"]):
                if a is not None:
                    differing += int((a != b[r]).sum())
        name, R, nrec, steps, trace, _ = WORKLOADS[wl]
        res["workloads"][wl] = {"config": name, "R": R, "recordings": nrec, "steps": steps, "graph_trace": trace,
                                "shape": dict((k, c[k]) for k in ("p", "L", "K", "nsup", "h", "F", "n", "H")),
                                "differing_elements_between_routes": differing}
        del last
        write()
        faster = WORKLOADS[wl][5]
        q = res["workloads"][wl]
        samples = {"loop": [], "pack": []}
        host = {"loop": [], "pack": []}
        for _ in range(args.reps):  # alternated
            for k, fn in routes.items():
                ms, h = event_ms(fn)
                samples[k].append(ms)
                host[k].append(h)
        for k, s in samples.items():
            q[k] = summary(s)
            q[k]["host_enqueue_median_ms"] = statistics.median(host[k])
        a, b = q["loop"], q["pack"]
        q["loop_over_pack"] = a["median_ms"] / b["median_ms"]
        q["combined_spread_ms"] = a["spread_ms"] + b["spread_ms"]
        q["pack_faster_beyond_spread"] = bool(a["median_ms"] - b["median_ms"] > q["combined_spread_ms"])
        q["pack_not_slower_beyond_spread"] = bool(b["median_ms"] - a["median_ms"] <= q["combined_spread_ms"])
        q["accepted"] = bool((q["pack_faster_beyond_spread"] if faster else q["pack_not_slower_beyond_spread"])
                             and q["differing_elements_between_routes"] == 0)
        ok = ok and q["accepted"]
        # the kernels' own times
        nwin = R * nrec * steps
        fl = bench.flops_per_window(c)["emb_fwd"] * nwin
        q["kernels"] = {}
        for k, fn in routes.items():
            nat.kernel_timing(True)
            nat.kernel_times()
            fn()
            torch.cuda.synchronize()
            kt = nat.kernel_times()
            nat.kernel_timing(False)
            ms = kt["score"][0]
            q["kernels"][k] = {"score_launches": kt["score"][1], "score_ms": ms, "prologue_ms": kt["supports"][0],
                               "score_graphs_ms": kt["score_graphs"][0],
                               "window_kernel_tflops": fl / (ms * 1e-3) / 1e12,
                               "window_kernel_frac_of_fp32_peak": fl / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS}
        assert q["kernels"]["pack"]["score_launches"] == 1 and q["kernels"]["loop"]["score_launches"] == R
        write()
        for k in ("loop", "pack"):
            print(wl, k, "%.3f ms [%.3f - %.3f]  k_score_windows %.3f ms, %.1f TF/s" % (
                q[k]["median_ms"], q[k]["min_ms"], q[k]["max_ms"], q["kernels"][k]["score_ms"],
                q["kernels"][k]["window_kernel_tflops"]), flush=True)
        print(wl, "differing elements:", q["differing_elements_between_routes"], "accepted:", q["accepted"], flush=True)
    res["accepted"] = bool(ok)
    write()
    print("accepted:", res["accepted"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
