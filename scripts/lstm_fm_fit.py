"""Time of fitting the cLSTM forecasting baseline (redcliff_amd.cLSTM_FM) on one MI355X: the fused
epoch launch (redcliff_lstm_fm_run, csrc/rc_lstm_fm.hip) against the generic nn.LSTM / autograd
route, and fit_lstm_baselines against a loop of fits.  The method of scripts/fm_fit.py.

Shape: the D4IC baseline (p = 10, h = 25, context 2, max_input_length 4, B = 128), 2,048 seeded
recordings = 16 steps per epoch of 256 sequences each; Adam(lr 5e-4, eps 1e-4, weight decay 1e-4).
  a  one model, `--epochs` training epochs (every batch_update of the epoch, no validation):
     fused = one redcliff_lstm_fm_run per epoch, generic = 16 batch_updates per epoch with
     REDCLIFF_LSTM_FM_PATH=generic
  b  15 models with per-model data, whole fits of `--fit-epochs` epochs with check_every = 5
     (training, validation and the checkpoint on check epochs, the stop rule, the final validation):
     fit_lstm_baselines against a loop of 15 fused fits, including the host time to enqueue
Protocol: per workload one warm-up of both routes, then --reps runs of each between two HIP events
on the stream, the two routes alternated; median [min - max], as us per step and per epoch.
Acceptance: on a fused must beat generic by more than the two min-max
spreads added together; on b the pack must not be slower than the loop by more than that sum, and
the two must leave 0 differing state elements.
Also recorded: the kernel's own event time for one epoch launch, its GFLOP/s from the step's
multiply-adds and its share of the 157.3 TF/s fp32 peak.  Writes profiles/lstm_fm_fit.json (or --out)."""
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
P, H, C, TM, B, N = 10, 25, 2, 4, 128, 2048
ADAM = dict(lr=5e-4, eps=1e-4, weight_decay=1e-4)
COEFF = {"FORECAST_COEFF": 1.0, "ADJ_L1_REG_COEFF": 0.01, "DAGNESS_REG_COEFF": 0.0}


def recordings(seed, n=N):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, TM, P).astype(np.float32)
    for t in range(1, TM):
        X[:, t] += 0.5 * np.roll(X[:, t - 1], 1, axis=1) - 0.2 * X[:, t - 1]
    return torch.from_numpy(X)


def loader(X):
    return [(X[i:i + B], None) for i in range(0, X.shape[0], B)]


def model(seed):
    import redcliff_amd
    torch.manual_seed(seed)
    m = redcliff_amd.cLSTM_FM(P, H, None, C, dict(COEFF)).to("cuda")
    return m, torch.optim.Adam(m.gen_model.parameters(), **ADAM)


def step_flops():
    """Multiply-adds of one batch_update counted as 2 flops, h_{-1} = 0 left out: the gate
    pre-activations, dL/dh through Whh, dWih / dWhh, and the output layer's forward, dWl and dL/dh."""
    Bq = B * (TM - C)
    gates = 2 * Bq * 4 * H * (C * P + (C - 1) * H)
    return P * (2 * gates + 2 * Bq * (C - 1) * 4 * H * H + 3 * 2 * Bq * C * H)


def workload_a(epochs, reps):
    from redcliff_amd import clstm_fm as F
    Xd = recordings(1).cuda()
    steps = N // B
    mf, of = model(10)
    mg, og = model(10)
    pack, r = mf._slot()
    pack.bind_optimizer(r, of)
    batches = [Xd[i:i + B] for i in range(0, N, B)]

    def fused(n):
        for _ in range(n):
            pack.run(F.FLAGS_TRAIN, Xd, 0, TM, TM, C, B, N, active=[r])

    def generic(n):
        os.environ["REDCLIFF_LSTM_FM_PATH"] = "generic"
        try:
            for _ in range(n):
                run = (0., 0., 0., 0.)
                for bn, Xb in enumerate(batches):
                    run = mg.batch_update(bn, Xb, TM, C, og, *run)
        finally:
            os.environ.pop("REDCLIFF_LSTM_FM_PATH", None)

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
    Xtr = [loader(recordings(100 + i)) for i in range(R)]
    Xva = [loader(recordings(200 + i, 512)) for i in range(R)]
    kw = dict(lookback=10 ** 6, check_every=5)

    def run(packed, tmp):
        ms_ = [model(300 + i) for i in range(R)]
        dirs = [os.path.join(tmp, "%d" % i) for i in range(R)]
        if packed:
            fn = lambda: redcliff_amd.fit_lstm_baselines([m for m, _ in ms_], [o for _, o in ms_], dirs, Xtr, Xva, C, TM,
                                                         epochs, **kw)
        else:
            fn = lambda: [m.fit(dirs[i], Xtr[i], o, C, TM, 1, epochs, verbose=0, X_val=Xva[i], **kw)
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
    return {"fits": R, "epochs": epochs, "check_every": 5, "steps_per_epoch": steps, "pack": sp, "loop": sl,
            "pack_host_ms": statistics.median(hp), "loop_host_ms": statistics.median(hl),
            "ratio_loop_over_pack": sl["median_ms"] / sp["median_ms"], "margin_ms": margin,
            "accepted": bool(sp["median_ms"] - sl["median_ms"] <= margin and differ == 0),
            "pack_faster_by_more_than_margin": bool(sl["median_ms"] - sp["median_ms"] > margin),
            "state_elements_that_differ": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20, help="training epochs per run of workload a")
    ap.add_argument("--fit-epochs", type=int, default=50, help="max_iter of every fit of workload b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_fm_fit.json"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(p=P, h=H, context=C, max_input_length=TM, B=B, N=N),
           "adam": ADAM,
           "protocol": "warm-up of both routes, then %d runs (a: %d epochs, b: fits of %d epochs) each between HIP "
                       "events, routes alternated" % (args.reps, args.epochs, args.fit_epochs),
           "a": workload_a(args.epochs, args.reps)}
    print(json.dumps({"a": {k: v for k, v in res["a"].items() if not isinstance(v, dict)}}), flush=True)
    res["b"] = workload_b(args.fit_epochs, args.reps)
    print(json.dumps({"b": {k: v for k, v in res["b"].items() if not isinstance(v, dict)}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
