"""Step time of a cEmbedder REDCLIFF-S model on the generic path and on the fused cEmbedder chain
(REDCLIFF_CEMB_PATH=generic | fused), with the DGCNN C1(K=4) step from the same process for context.

Shape: C1 with a cEmbedder -- p=10, L=5, K=4, nsup=4, h=25, F=16, eh=25, B=128.  Phases: combined
and acclimation.  Per (path, phase): warm up, then REPS x STEPS model.batch_update calls on
device-resident batches between two HIP events on the stream (the host is part of what a fit pays
per step, and the generic path is host-bound); median and min-max over the repetitions.  The fused
chains are also timed as one C call per STEPS steps (redcliff_cemb_train_steps /
redcliff_train_steps, the way fit() runs an epoch), which takes the host out.  Launches per step are
counted last, with the torch profiler's device-kernel records of one step.

Writes profiles/cemb_step.json (or --out).  Acceptance: the fused batch_update step is faster than
the generic one by more than the two measurements' combined min-max spread."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bench  # noqa: E402

CFG = dict(p=10, L=5, K=4, nsup=4, h=25, F=16, eh=25, B=128, T=100, label_T=100, lrA=5e-4, lrB=5e-4)
EPOCH = {"acclimation": 1, "combined": 2}  # pre = 1, acc = 1


def cemb_model(seed=0):
    import redcliff_amd
    c = CFG
    eargs = [("sigmoid_eccentricity_coeff", 10.0), ("lag", c["F"]), ("hidden", [c["eh"]])]
    torch.manual_seed(seed)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(
        c["p"], c["L"], [c["h"]], c["F"], [0], c["L"], 1, c["K"], c["nsup"], bench.coeffs(c["K"], c["p"]), False,
        "cEmbedder", eargs, "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion",
        num_sims=1, training_mode="pretrain_embedder_then_acclimate_factors_then_combined", num_pretrain_epochs=1,
        num_acclimation_epochs=1).float().cuda()


def event_ms(fn, steps):
    """Milliseconds per step of fn() (which enqueues `steps` steps) between two events on the stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples),
            "spread_ms": max(samples) - min(samples), "samples_ms": samples}


def measure(fn, steps, warmup, reps):
    fn(warmup)
    return summary([event_ms(lambda: fn(steps), steps) for _ in range(reps)])


def count_launches(step):
    """Device kernels of one step (torch profiler); None when the profiler is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as exc:  # the measurement stands without the count
        print("launch count unavailable: %r" % (exc,), flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--generic-warmup", type=int, default=5, help="warm-up steps of the (slow, host-bound) generic path")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cemb_step.json"))
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    from redcliff_amd import _native as nat
    import redcliff_amd
    assert torch.cuda.is_available(), "needs the MI355X"
    B = CFG["B"]
    X, Y = bench.synth(CFG, B, seed=3)
    X, Y = X.cuda(), Y.cuda()
    res = {"shape": dict((k, CFG[k]) for k in ("p", "L", "K", "nsup", "h", "F", "eh", "B")), "steps": args.steps,
           "warmup": args.warmup, "reps": args.reps, "build_id": nat.build_id(),
           "device": torch.cuda.get_device_name(0), "phases": {}}

    def write():  # after every measurement: an interrupted run keeps what it has
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    steppers = {}
    for path in ("generic", "fused"):
        os.environ["REDCLIFF_CEMB_PATH"] = path
        m = cemb_model()
        oA, oB = bench.adam_pair(m, CFG)
        assert m.cembedder_fused_supported(B)
        m.batch_update(0, 0, X, Y, oA, oB, 1)
        for phase, epoch in EPOCH.items():
            def run(n, m=m, oA=oA, oB=oB, epoch=epoch):
                for _ in range(n):
                    m.batch_update(epoch, 0, X, Y, oA, oB, 1)
            res["phases"].setdefault(phase, {})[path] = measure(
                run, args.steps, args.generic_warmup if path == "generic" else args.warmup, args.reps)
            write()
            steppers[(path, phase)] = (lambda run=run, path=path: (os.environ.__setitem__("REDCLIFF_CEMB_PATH", path), run(1)))
            print(path, phase, res["phases"][phase][path]["median_ms"], flush=True)
        if path == "fused":  # one C call per `steps` steps (an epoch of fit())
            eng = m._cemb_fused(B)
            staged = eng.stage(X, Y)
            for phase, kind in (("acclimation", "acclimate"), ("combined", "combined")):
                def runc(n, kind=kind):
                    eng.run_steps([kind], staged, oA, oB, [0] * n, [B] * n)
                res["phases"][phase]["fused_one_call"] = measure(runc, args.steps, args.warmup, args.reps)
    # the DGCNN C1(K=4) step, for context
    c1 = bench.CONFIGS["c1k4"]
    md = bench.build_model(redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing, c1, seed=0).cuda()
    dA, dB = bench.adam_pair(md, c1)
    Xc, Yc = bench.synth(c1, c1["B"], seed=3)
    Xc, Yc = Xc.cuda(), Yc.cuda()
    md.batch_update(0, 0, Xc, Yc, dA, dB, 1)
    deng = md.engine()
    dstaged = deng.stage(Xc, Yc)
    # one statistics row per step
    stn = dict((n, dstaged["stats"].repeat(n, 1, 1).contiguous()) for n in (args.steps, args.warmup))
    for phase, epoch, kind in (("acclimation", 1, "acclimate"), ("combined", 2, "combined")):
        def rund(n, epoch=epoch):
            for _ in range(n):
                md.batch_update(epoch, 0, Xc, Yc, dA, dB, 1)

        def rundc(n, kind=kind):
            deng.run_steps([kind], dstaged, dA, dB, [0] * n, [c1["B"]] * n, stn[n])
        ph = res["phases"][phase]
        ph["dgcnn_c1k4"] = measure(rund, args.steps, args.warmup, args.reps)
        ph["dgcnn_c1k4_one_call"] = measure(rundc, args.steps, args.warmup, args.reps)
    for phase, ph in res["phases"].items():
        g, f = ph["generic"], ph["fused"]
        ph["generic_over_fused"] = g["median_ms"] / f["median_ms"]
        ph["combined_spread_ms"] = g["spread_ms"] + f["spread_ms"]
        ph["fused_faster_beyond_spread"] = bool(g["median_ms"] - f["median_ms"] > ph["combined_spread_ms"])
        ph["fused_over_dgcnn_c1k4"] = f["median_ms"] / ph["dgcnn_c1k4"]["median_ms"]
        ph["fused_over_dgcnn_c1k4_one_call"] = ph["fused_one_call"]["median_ms"] / ph["dgcnn_c1k4_one_call"]["median_ms"]
    res["accepted"] = all(ph["fused_faster_beyond_spread"] for ph in res["phases"].values())
    write()  # the timings are kept whatever the profiler does below
    if not args.no_launch_count:
        for (path, phase), step in steppers.items():
            res["phases"][phase][path]["launches_per_step"] = count_launches(step)
        write()
    print(json.dumps(dict((ph, dict((k, v if not isinstance(v, dict) else v["median_ms"]) for k, v in r.items()))
                          for ph, r in res["phases"].items()), sort_keys=True))
    print("accepted:", res["accepted"])
    return 0 if res["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
