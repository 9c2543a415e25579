"""Time of scoring whole recordings with a trained-shape DGCNN REDCLIFF-S model on one MI355X:
factor scores (w + class scores) and graph traces (graphs="sum") of every time step.

Shapes: the bench's d4ic and c4 (TST) embedders.  Workloads: one recording of 131,072 scored steps
at stride 1, and 64 recordings of 2,048 steps.  Routes:
  loop     the per-step loop of the two reference-named functions (redcliff_amd.evaluation with the
           embedder's own forward, one window per call, each result copied to the host) and, for the
           graphs, model.GC per window; timed on --loop-steps steps and reported per step, so its
           figure for the whole workload is EXTRAPOLATED
  chunked  unfold + at most 512 windows per embedder / GC call (scoring._chunked_score)
  fused    redcliff_score_recording (csrc/rc_score.hip)
Protocol (scripts/cemb_step.py): warm up, then --reps runs between two HIP events; median [min - max].
Acceptance: fused beats chunked on scores and on graphs, at both shapes and workloads, by more than
the two min-max spreads added together.

Also recorded: ms per 1,000 steps, TF/s of the window kernel from bench.flops_per_window(c)["emb_fwd"]
against the 157.3 TF/s fp32 peak, bytes written and GB/s of the graph epilogue against 8 TB/s (both from
the kernels' own HIP-event times, redcliff_kernel_times).  Writes profiles/score_recording.json (or --out)."""
import argparse
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
HBM_PEAK_GBS = 8000.0
WORKLOADS = {"1x131072": (1, 131072), "64x2048": (64, 2048)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    s = [event_ms(fn) for _ in range(reps)]
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
    ap.add_argument("--loop-steps", type=int, default=2000)
    ap.add_argument("--configs", default="d4ic,c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_recording.json"))
    args = ap.parse_args()
    import redcliff_amd
    from redcliff_amd import _native as nat
    from redcliff_amd import evaluation as ev
    from redcliff_amd import scoring
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"reps": args.reps, "warmup": args.warmup, "loop_steps": args.loop_steps, "build_id": nat.build_id(),
           "device": torch.cuda.get_device_name(0), "configs": {}}

    def write():  # after every measurement: an interrupted run keeps what it has
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    ok = True
    for name in args.configs.split(","):
        c = bench.CONFIGS[name]
        m = bench.build_model(redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing, c, seed=0).float().cuda()
        m.eval()
        F, p, K, nsup = c["F"], c["p"], c["K"], c["nsup"]
        mode = m.primary_gc_est_mode
        assert scoring.fused_available(m)
        out = res["configs"].setdefault(name, {"shape": dict((k, c[k]) for k in ("p", "L", "K", "nsup", "h", "F", "n", "H"))})
        for wl, (nrec, steps) in WORKLOADS.items():
            X = recordings(nrec, steps, F, p, seed=3)
            nwin = nrec * steps
            r = out.setdefault(wl, {"recordings": nrec, "steps": steps})
            routes = {
                ("scores", "chunked"): lambda: scoring._chunked_score(m, X, F, steps, 1, True, None, True),
                ("scores", "fused"): lambda: m.score_recording(X, start=F, count=steps),
                ("graphs", "chunked"): lambda: scoring._chunked_score(m, X, F, steps, 1, True, mode, True),
                ("graphs", "fused"): lambda: m.score_recording(X, start=F, count=steps, graphs="sum"),
            }
            for (what, route), fn in routes.items():
                s = measure(fn, args.warmup, args.reps)
                s["ms_per_1000_steps"] = s["median_ms"] / nwin * 1000.0
                r.setdefault(what, {})[route] = s
                write()
                print(name, wl, what, route, "%.3f ms [%.3f - %.3f]" % (s["median_ms"], s["min_ms"], s["max_ms"]), flush=True)
            if nrec == 1:  # the per-step loops, on the first loop-steps steps of the recording
                n = args.loop_steps
                sig = X[:, :n + F]

                def loop_scores():
                    emb = m.factor_score_embedder
                    for i in range(F, F + n):  # both reference functions: two embedder calls per step
                        emb(sig[:, i - F:i, :])[0][0, :nsup].detach().cpu().numpy()
                        emb(sig[:, i - F:i, :])[1][0, :nsup].detach().cpu().numpy()

                def loop_graphs():
                    with torch.no_grad():
                        for i in range(F, F + n):
                            sum(m.GC(mode, X=sig[:, i - F:i, :], threshold=False, ignore_lag=True)[0])
                assert p != F
                for what, fn in (("scores", loop_scores), ("graphs", loop_graphs)):
                    s = measure(fn, args.warmup, args.reps)
                    s["timed_steps"] = n
                    s["ms_per_1000_steps"] = s["median_ms"] / n * 1000.0
                    s["extrapolated_ms"] = s["median_ms"] / n * nwin  # EXTRAPOLATED to the whole recording
                    r[what]["loop"] = s
                    write()
                    print(name, wl, what, "loop", "%.3f ms per 1000 steps (extrapolated %.0f ms)" % (
                        s["ms_per_1000_steps"], s["extrapolated_ms"]), flush=True)
                # the drop-ins go through the fused kernel and agree with the loop they replace
                a = ev.obtain_factor_score_weightings_across_recording(m, sig.cpu(), nsup, 64, F)
                b = np.stack([m.factor_score_embedder(sig[:, i - F:i, :])[0][0, :nsup].detach().cpu().numpy()
                              for i in range(F, F + 64)], 1)
                r["drop_in_max_abs_diff_vs_loop"] = float(np.abs(a - b).max())
            for what in ("scores", "graphs"):
                f, g = r[what]["fused"], r[what]["chunked"]
                r[what]["chunked_over_fused"] = g["median_ms"] / f["median_ms"]
                r[what]["combined_spread_ms"] = f["spread_ms"] + g["spread_ms"]
                r[what]["fused_faster_beyond_spread"] = bool(g["median_ms"] - f["median_ms"] > r[what]["combined_spread_ms"])
                ok = ok and r[what]["fused_faster_beyond_spread"]
            # the kernels' own times
            nat.kernel_timing(True)
            nat.kernel_times()
            m.score_recording(X, start=F, count=steps, graphs="sum")
            torch.cuda.synchronize()
            kt = nat.kernel_times()
            nat.kernel_timing(False)
            Q = p * p
            fl = bench.flops_per_window(c)["emb_fwd"] * nwin
            ms_w, ms_g = kt["score"][0], kt["score_graphs"][0]
            r["kernels"] = {"score_ms": ms_w, "score_graphs_ms": ms_g, "prologue_ms": kt["supports"][0],
                            "window_kernel_tflops": fl / (ms_w * 1e-3) / 1e12,
                            "window_kernel_frac_of_fp32_peak": fl / (ms_w * 1e-3) / 1e12 / FP32_PEAK_TFLOPS,
                            "graph_bytes_written": nwin * Q * 4,
                            "graph_gbs": nwin * Q * 4 / (ms_g * 1e-3) / 1e9,
                            "graph_frac_of_hbm_peak": nwin * Q * 4 / (ms_g * 1e-3) / 1e9 / HBM_PEAK_GBS}
            write()
            print(name, wl, "kernels", json.dumps(r["kernels"]), flush=True)
            del X
    res["accepted"] = bool(ok)
    write()
    print("accepted:", res["accepted"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
