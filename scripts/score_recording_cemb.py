"""Time of scoring whole recordings with a cEmbedder REDCLIFF-S model on one MI355X: factor scores
(w + class scores) and graph traces (graphs="sum") of every time step.

Shapes: C1 with a cEmbedder (p=10, L=5, K=4, h=25, F=16, eh=25: scripts/cemb_step.py's shape) and the
bench's c4 dims with a cEmbedder of eh=100.  Workloads: one recording of 131,072 scored steps at
stride 1, and 64 recordings of 2,048 steps.  Routes:
  chunked  unfold + at most 512 windows per embedder / GC call (scoring._chunked_score): what
           model.score_recording runs with REDCLIFF_CEMB_PATH unset
  fused    redcliff_cemb_score_recording (csrc/rc_score_cemb.hip): REDCLIFF_CEMB_PATH=fused
Protocol (scripts/score_recording.py): warm up both routes, then --reps runs of each between two HIP
events, the two routes alternated; median [min - max].  Acceptance: fused beats chunked on scores
and on graphs, at both shapes and workloads, by more than the two min-max spreads added together.

Also recorded (not gated): k_score_cemb's own time (redcliff_kernel_times) and its TF/s from
2 pF K eh + 3 K eh FLOP per window against the 157.3 TF/s fp32 peak, and the largest difference
between the two routes' results.  --kernel-only NAME records the kernel's time and a hash of its
output for a build variant (scripts/build_variant.py with -DCS_GROUPS=1|2|4, -DCS_KU=1|4).
Writes profiles/score_recording_cemb.json (or --out)."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bench  # noqa: E402

FP32_PEAK_TFLOPS = 157.3
WORKLOADS = {"1x131072": (1, 131072), "64x2048": (64, 2048)}
ENV = "REDCLIFF_CEMB_PATH"
C4 = bench.CONFIGS["c4"]
SHAPES = {
    "c1_cemb": dict(p=10, L=5, K=4, nsup=4, h=25, F=16, eh=25),
    "c4_cemb": dict(p=C4["p"], L=C4["L"], K=C4["K"], nsup=C4["nsup"], h=C4["h"], F=C4["F"], eh=100),
}


def cemb_model(c, seed=0):
    import redcliff_amd
    eargs = [("sigmoid_eccentricity_coeff", 10.0), ("lag", c["F"]), ("hidden", [c["eh"]])]
    torch.manual_seed(seed)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(
        c["p"], c["L"], [c["h"]], c["F"], [0], c["L"], 1, c["K"], c["nsup"], bench.coeffs(c["K"], c["p"]), False,
        "cEmbedder", eargs, "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion",
        num_sims=1, training_mode="combined").float().cuda()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(s):
    return {"median_ms": statistics.median(s), "min_ms": min(s), "max_ms": max(s), "spread_ms": max(s) - min(s),
            "samples_ms": s}


def recordings(nrec, steps, F, p, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(nrec, steps + F, p).astype(np.float32)
    X[:, 1:] += 0.4 * X[:, :-1]
    return torch.from_numpy(X).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="c1_cemb,c4_cemb")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--kernel-only", default=None, metavar="VARIANT",
                    help="time k_score_cemb alone and record it under this variant name (operand-reuse experiments: "
                         "a library built with -DCS_GROUPS / -DCS_KU, selected with REDCLIFF_HIP_LIB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_recording_cemb.json"))
    args = ap.parse_args()
    from redcliff_amd import _native as nat
    from redcliff_amd import scoring
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"reps": args.reps, "warmup": args.warmup, "build_id": nat.build_id(), "device": torch.cuda.get_device_name(0),
           "configs": {}}
    if os.path.exists(args.out):  # a run over part of the configs / workloads keeps the others
        with open(args.out) as f:
            old = json.load(f)
        if args.kernel_only:  # a variant run adds its entries only (the header describes the main run)
            res = old
        else:
            res["configs"] = old.get("configs", {})

    def write():  # after every measurement: an interrupted run keeps what it has
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    def route(value, fn):
        def run():
            if value is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = value
            try:
                return fn()
            finally:
                os.environ.pop(ENV, None)
        return run

    ok = True
    for name in args.configs.split(","):
        c = SHAPES[name]
        m = cemb_model(c)
        m.eval()
        F, p, K, eh = c["F"], c["p"], c["K"], c["eh"]
        assert scoring.cemb_fused_available(m)
        out = res["configs"].setdefault(name, {})
        out["shape"] = c
        for wl in args.workloads.split(","):
            nrec, steps = WORKLOADS[wl]
            X = recordings(nrec, steps, F, p, seed=3)
            nwin = nrec * steps
            if args.kernel_only:  # one build variant (REDCLIFF_HIP_LIB): the kernel's own time and a hash of its output
                fused = route("fused", lambda: m.score_recording(X, start=F, count=steps))
                for _ in range(args.warmup):
                    fused()
                nat.kernel_timing(True)
                ms = []
                for _ in range(args.reps):
                    nat.kernel_times()
                    got = fused()
                    torch.cuda.synchronize()
                    ms.append(nat.kernel_times()["score_cemb"][0])
                nat.kernel_timing(False)
                v = summary(ms)
                fl = (2 * p * F * K * eh + 3 * K * eh) * nwin
                v["window_kernel_tflops"] = fl / (v["median_ms"] * 1e-3) / 1e12
                v["w_sha256"] = hashlib.sha256(got.w.cpu().numpy().tobytes()).hexdigest()
                out.setdefault("variants", {}).setdefault(args.kernel_only, {})[wl] = v
                write()
                print(name, wl, args.kernel_only, "k_score_cemb %.4f ms [%.4f - %.4f] %.2f TF/s %s" % (
                    v["median_ms"], v["min_ms"], v["max_ms"], v["window_kernel_tflops"], v["w_sha256"][:12]), flush=True)
                continue
            r = out[wl] = {"recordings": nrec, "steps": steps}
            for what, graphs in (("scores", None), ("graphs", "sum")):
                call = lambda: m.score_recording(X, start=F, count=steps, graphs=graphs)  # noqa: E731
                routes = {"chunked": route(None, call), "fused": route("fused", call)}
                last = {}
                for _ in range(args.warmup):
                    for k, fn in routes.items():
                        last[k] = fn()
                diff = max(float((a - b).abs().max()) for a, b in zip(last["chunked"], last["fused"]) if a is not None)
                del last
                samples = {"chunked": [], "fused": []}
                for _ in range(args.reps):  # alternated
                    for k, fn in routes.items():
                        samples[k].append(event_ms(fn))
                q = r[what] = dict((k, summary(s)) for k, s in samples.items())
                for k in routes:
                    q[k]["ms_per_1000_steps"] = q[k]["median_ms"] / nwin * 1000.0
                f, g = q["fused"], q["chunked"]
                q["max_abs_diff_between_routes"] = diff
                q["chunked_over_fused"] = g["median_ms"] / f["median_ms"]
                q["combined_spread_ms"] = f["spread_ms"] + g["spread_ms"]
                q["fused_faster_beyond_spread"] = bool(g["median_ms"] - f["median_ms"] > q["combined_spread_ms"])
                ok = ok and q["fused_faster_beyond_spread"]
                write()
                for k in ("chunked", "fused"):
                    print(name, wl, what, k, "%.3f ms [%.3f - %.3f]" % (q[k]["median_ms"], q[k]["min_ms"], q[k]["max_ms"]),
                          flush=True)
            # the kernels' own times
            nat.kernel_timing(True)
            nat.kernel_times()
            route("fused", lambda: m.score_recording(X, start=F, count=steps, graphs="sum"))()
            torch.cuda.synchronize()
            kt = nat.kernel_times()
            nat.kernel_timing(False)
            assert kt["score_cemb"][1] == 1
            fl = (2 * p * F * K * eh + 3 * K * eh) * nwin
            ms_w = kt["score_cemb"][0]
            r["kernels"] = {"score_cemb_ms": ms_w, "score_graphs_ms": kt["score_graphs"][0],
                            "window_kernel_tflops": fl / (ms_w * 1e-3) / 1e12,
                            "window_kernel_frac_of_fp32_peak": fl / (ms_w * 1e-3) / 1e12 / FP32_PEAK_TFLOPS}
            write()
            print(name, wl, "kernels", json.dumps(r["kernels"]), flush=True)
            del X
    if args.kernel_only:
        return 0
    res["accepted"] = bool(ok)
    write()
    print("accepted:", res["accepted"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
