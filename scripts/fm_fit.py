"""Time of fitting the cMLP forecasting baseline (redcliff_amd.cMLP_FM) on one MI355X: the fused
epoch launch (redcliff_fm_run, csrc/rc_fm.hip) against the generic torch-autograd route, and
fit_baselines against a loop of fits.

Shape: the D4IC baseline (p = 10, L = 2, h = 50, B = 128), 2,048 seeded windows = 16 steps per epoch;
Adam(lr 1e-3, eps 1e-4, weight decay 1e-4).
  a  one model, `--epochs` training epochs (every batch_update of the epoch, no validation or
     tracking): fused = one redcliff_fm_run per epoch, generic = 16 batch_updates per epoch with
     REDCLIFF_FM_PATH=generic
  b  15 models with per-replica data, whole fits of `--epochs` epochs (training, tracking,
     validation, the stop rule, one checkpoint at epoch 0): fit_baselines against a loop of 15 fused
     fits, including the host time to enqueue
Protocol: per workload one warm-up of both routes, then --reps runs of each between two HIP events
on the stream, the two routes alternated; median [min - max], as us per step and per epoch.
Acceptance: on a fused must beat generic by more than the two min-max spreads
added together; on b the pack must not be slower than the loop by more than that sum.
Also recorded: the kernel's own event time for one epoch launch, its GFLOP/s from the step's
multiply-adds and its share of the 157.3 TF/s fp32 peak.  Writes profiles/fm_fit.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from fit_timing import event_ms, summary  # scripts/ leads the path of a script run

FP32_PEAK_TFLOPS = 157.3
P, L, H, B, N = 10, 2, 50, 128, 2048
ADAM = dict(lr=1e-3, eps=1e-4, weight_decay=1e-4)
COEFF = {"FORECAST_COEFF": 1.0, "ADJ_L1_REG_COEFF": 0.01, "DAGNESS_REG_COEFF": 0.0, "DAGNESS_LAG_COEFF": 0.0,
         "DAGNESS_NODE_COEFF": 0.0}


def windows(seed, n=N):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, L + 1, P).astype(np.float32)
    for t in range(1, L + 1):
        X[:, t] += 0.5 * np.roll(X[:, t - 1], 1, axis=1) - 0.2 * X[:, t - 1]
    return torch.from_numpy(X)


def loader(X):
    return [(X[i:i + B], None) for i in range(0, X.shape[0], B)]


def model(seed):
    import redcliff_amd
    torch.manual_seed(seed)
    m = redcliff_amd.cMLP_FM(P, L, [H], None, L, 1, dict(COEFF)).to("cuda")
    return m, torch.optim.Adam(m.gen_model.parameters(), **ADAM)


def step_flops():
    """Multiply-adds of one batch_update counted as 2 flops: forward z and y, backward dW0, dW1, db0, dz."""
    Q = P * L
    return P * (2 * B * H * Q + 2 * B * H + 2 * B * H * Q + 2 * B * H + 2 * B * H)


def workload_a(epochs, reps):
    from redcliff_amd import cmlp_fm as F
    Xd = windows(1).cuda()
    steps = N // B
    mf, of = model(10)
    mg, og = model(10)
    pack, r = mf._slot()
    pack.bind_optimizer(r, of)
    batches = [Xd[i:i + B] for i in range(0, N, B)]

    def fused(n):
        for _ in range(n):
            pack.run(F.FM_FLAGS_TRAIN, Xd, 0, L + 1, B, N, active=[r])

    def generic(n):
        os.environ["REDCLIFF_FM_PATH"] = "generic"
        try:
            for _ in range(n):
                for bn, Xb in enumerate(batches):
                    mg.batch_update(bn, Xb, og, L, 1)
        finally:
            os.environ.pop("REDCLIFF_FM_PATH", None)

    fused(2)
    generic(2)
    tf, tg, hf, hg = [], [], [], []
    for _ in range(reps):
        ms, host = event_ms(lambda: fused(epochs))
        tf.append(ms)
        hf.append(host)
        ms, host = event_ms(lambda: generic(epochs))
        tg.append(ms)
        hg.append(host)
    kern = [event_ms(lambda: fused(1))[0] for _ in range(9)]
    k_us = 1e3 * statistics.median(kern)
    gflops = steps * step_flops() / (k_us * 1e-6) / 1e9
    sf, sg = summary(tf, epochs, steps), summary(tg, epochs, steps)
    margin = sf["spread_ms"] + sg["spread_ms"]
    return {"epochs": epochs, "steps_per_epoch": steps, "fused": sf, "generic": sg,
            "fused_host_ms": statistics.median(hf), "generic_host_ms": statistics.median(hg),
            "ratio_generic_over_fused": sg["median_ms"] / sf["median_ms"], "margin_ms": margin,
            "accepted": bool(sg["median_ms"] - sf["median_ms"] > margin),
            "kernel_event_us_per_epoch": {"median": k_us, "min": 1e3 * min(kern), "max": 1e3 * max(kern)},
            "kernel_event_us_per_step": k_us / steps, "flops_per_step": step_flops(), "kernel_gflops": gflops,
            "kernel_share_of_fp32_peak": gflops / (1e3 * FP32_PEAK_TFLOPS), "workgroups": P}


def workload_b(epochs, reps, R=15):
    import redcliff_amd
    steps = N // B
    rng = np.random.RandomState(7)
    Xtr = [loader(windows(100 + i)) for i in range(R)]
    Xva = [loader(windows(200 + i, 512)) for i in range(R)]
    GCs = [[(rng.rand(P, P, L) < 0.3).astype(np.float64) + np.eye(P)[:, :, None]] for _ in range(R)]
    kw = dict(lookback=10 ** 6, check_every=10 ** 6)

    def run(packed, tmp):
        ms_ = [model(300 + i) for i in range(R)]
        dirs = [os.path.join(tmp, "%d" % i) for i in range(R)]
        if packed:
            fn = lambda: redcliff_amd.fit_baselines([m for m, _ in ms_], [o for _, o in ms_], dirs, Xtr, Xva, GCs, L, 1,
                                                    epochs, **kw)
        else:
            fn = lambda: [m.fit(dirs[i], Xtr[i], o, L, 1, 1, epochs, verbose=0, GC=GCs[i], X_val=Xva[i], **kw)
                          for i, (m, o) in enumerate(ms_)]
        ms, host = event_ms(fn)
        return ms, host, [m for m, _ in ms_]

    with tempfile.TemporaryDirectory() as tmp:
        run(True, tmp)
        run(False, tmp)
        tp, tl, hp, hl = [], [], [], []
        differ = 0
        for _ in range(reps):
            ms, host, mp = run(True, tmp)
            tp.append(ms)
            hp.append(host)
            ms, host, ml = run(False, tmp)
            tl.append(ms)
            hl.append(host)
            for a, b in zip(mp, ml):
                sa, sb = a.state_dict(), b.state_dict()
                differ += sum(int((sa[k] != sb[k]).sum()) for k in sa)
    sp, sl = summary(tp, epochs, steps), summary(tl, epochs, steps)
    margin = sp["spread_ms"] + sl["spread_ms"]
    return {"fits": R, "epochs": epochs, "steps_per_epoch": steps, "pack": sp, "loop": sl,
            "pack_host_ms": statistics.median(hp), "loop_host_ms": statistics.median(hl),
            "ratio_loop_over_pack": sl["median_ms"] / sp["median_ms"], "margin_ms": margin,
            "accepted": bool(sp["median_ms"] - sl["median_ms"] <= margin),
            "pack_faster_by_more_than_margin": bool(sl["median_ms"] - sp["median_ms"] > margin),
            "state_elements_that_differ": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_fit.json"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(p=P, L=L, h=H, B=B, N=N), "adam": ADAM,
           "protocol": "warm-up of both routes, then %d runs of %d epochs each between HIP events, routes alternated"
                       % (args.reps, args.epochs),
           "a": workload_a(args.epochs, args.reps)}
    print(json.dumps({"a": {k: v for k, v in res["a"].items() if not isinstance(v, dict)}}), flush=True)
    res["b"] = workload_b(args.epochs, args.reps)
    print(json.dumps({"b": {k: v for k, v in res["b"].items() if not isinstance(v, dict)}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
