"""Time of fitting the NAVAR (LSTM) baseline (redcliff_amd.NAVARLSTM) on one MI355X: the fused route
(redcliff_navar_lstm_run, csrc/rc_navar_lstm.hip, one native call per epoch) against the generic route
(the reference's operations: nn.LSTM, autograd, torch Adam), and fit_navar_lstm_baselines against a loop
of fused fits.

Shape: the published one (num_nodes 10, num_hidden 256, one LSTM layer, 20 steps, batch 128, Adam lr
1e-4, lambda1 0; train/NAVAR_CLSTM_d4IC_BCTVgs1Parsim_cached_args.txt), 2,048 seeded windows = 16 steps
per epoch.
  a  one model, whole fits of `--epochs` epochs (the final causal-matrix pass and the save included):
     fused against generic (REDCLIFF_NAVAR_LSTM_PATH=generic)
  b  15 models with per-model data, whole fits of `--epochs-b` epochs: fit_navar_lstm_baselines against a
     loop of 15 fused fits, including the host time to enqueue
Protocol (scripts/navar_fit.py): per workload one warm-up of both routes, then --reps runs of each
between two HIP events on the stream, the two routes alternated; median [min - max].
Acceptance: on a fused must beat generic by more than the two min-max spreads
added together; on b the pack must not be slower than the loop by more than that sum, and the two
routes of b leave zero differing state and causal-matrix elements.
Also recorded: the event time per step of each group of launches (one-step TRAIN calls restricted by
RedcliffNavarLstmArgs.launches, after a full step has filled the workspace), the whole step's, and the
achieved TF/s of the step's recurrent products against the 157.3 TF/s fp32 matrix peak.
Writes profiles/navar_lstm_fit.json (or --out)."""
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

FP32_MATRIX_PEAK_TFLOPS = 157.3
NN, H, K, B, N = 10, 256, 20, 128, 2048  # K: LSTM steps T'
ADAM = dict(lr=1e-4)


def windows(seed, n=N):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, K + 1, NN).astype(np.float32)
    for t in range(1, K + 1):
        X[:, t] += 0.5 * np.roll(X[:, t - 1], 1, axis=1) - 0.2 * X[:, t - 1]
    return X


def model(seed):
    import redcliff_amd
    torch.manual_seed(seed)
    m = redcliff_amd.NAVARLSTM(NN, H, K).to("cuda")
    return m, torch.optim.Adam(m.parameters(), **ADAM)


def step_flops():
    """Multiply-adds of one step counted as 2 flops: per source the H x 4H recurrent product of the
    forward (K - 1 steps read a state), the dh carry and dWhh, and the output layer at the last step
    (lambda1 = 0) forward, dWfc and dh."""
    return NN * 2 * B * (3 * (K - 1) * 4 * H * H + 3 * NN * H)


def fit_one(m, o, X, tmp, epochs, seed):
    return m.fit(tmp, X, None, torch.nn.MSELoss(), o, epochs=epochs, batch_size=B, check_every=10 ** 6, lambda1=0,
                 rng=np.random.RandomState(seed))


def kernel_times(reps=5):
    """Event time per step of the whole step and of each of its launches alone (the launch mask)."""
    from redcliff_amd import navar_lstm as nv
    m, o = model(1)
    pack, r = m._slot()
    pack.bind_optimizer(r, o)
    X = torch.from_numpy(windows(2, B)).cuda()
    perm = torch.arange(B, dtype=torch.int32, device="cuda")
    mse = torch.empty(1, 1, device="cuda")
    l1 = torch.empty(1, 1, device="cuda")
    ws = pack.workspace(B, 1, K, True)
    d, hyper = pack.dims(B, K + 1), pack.hyper(0, [0])

    def call(mask):
        rc = nv.navar_lstm_run(d, nv.TRAIN, B, 1, 0, B, B, X, 0, perm, 0, pack.par, pack.m, pack.v, pack.n, hyper, mse, l1,
                          None, None, ws, launches=mask)
        assert rc == 0
    n, out = 5, {}
    for name, mask in (("step", 0), ("forward_x%d" % K, 1), ("output_and_reduction", 2), ("backward_x%d" % K, 4),
                       ("dWhh_and_adam", 8)):
        for _ in range(3):
            call(0)
        t = [event_ms(lambda: [call(mask) for _ in range(n)])[0] / n for _ in range(reps)]
        out[name + "_us"] = {"median": 1e3 * statistics.median(t), "min": 1e3 * min(t), "max": 1e3 * max(t)}
    s_us = out["step_us"]["median"]
    out.update(flops_per_step=step_flops(), step_tflops=step_flops() / (s_us * 1e-6) / 1e12,
               share_of_fp32_matrix_peak=step_flops() / (s_us * 1e-6) / 1e12 / FP32_MATRIX_PEAK_TFLOPS,
               workgroups_per_recurrent_launch=NN * ((H + 15) // 16), launches_per_step=2 * K + 5,
               workspace_mb_per_replica=4e-6 * nv.navar_lstm_ws_floats(NN, H, K, B, True))
    return out


def workload_a(epochs, reps):
    X = windows(1)
    steps = N // B

    def run(route, tmp):
        os.environ["REDCLIFF_NAVAR_LSTM_PATH"] = route
        try:
            m, o = model(10)
            return event_ms(lambda: fit_one(m, o, X, tmp, epochs, 5)) + (m,)
        finally:
            os.environ.pop("REDCLIFF_NAVAR_LSTM_PATH", None)
    with tempfile.TemporaryDirectory() as tmp:
        run("fused", tmp)
        run("generic", tmp)
        tf, tg, hf, hg = [], [], [], []
        for _ in range(reps):
            ms, host, _ = run("fused", tmp)
            tf.append(ms)
            hf.append(host)
            ms, host, _ = run("generic", tmp)
            tg.append(ms)
            hg.append(host)
    sf, sg = summary(tf, epochs, steps), summary(tg, epochs, steps)
    margin = sf["spread_ms"] + sg["spread_ms"]
    return {"epochs": epochs, "steps_per_epoch": steps, "fused": sf, "generic": sg,
            "fused_host_ms": statistics.median(hf), "generic_host_ms": statistics.median(hg),
            "ratio_generic_over_fused": sg["median_ms"] / sf["median_ms"], "margin_ms": margin,
            "accepted": bool(sg["median_ms"] - sf["median_ms"] > margin)}


def workload_b(epochs, reps, R=15):
    import redcliff_amd
    steps = N // B
    Xs = [windows(100 + i) for i in range(R)]

    def run(packed, tmp):
        ms_ = [model(300 + i) for i in range(R)]
        dirs = [os.path.join(tmp, "%d" % i) for i in range(R)]
        for d in dirs:
            os.makedirs(d, exist_ok=True)
        if packed:
            fn = lambda: redcliff_amd.fit_navar_lstm_baselines(
                [m for m, _ in ms_], dirs, Xs, torch.nn.MSELoss(), [o for _, o in ms_], epochs=epochs, batch_size=B,
                check_every=10 ** 6, lambda1=0, rngs=[np.random.RandomState(400 + i) for i in range(R)])
        else:
            fn = lambda: [fit_one(m, o, Xs[i], dirs[i], epochs, 400 + i) for i, (m, o) in enumerate(ms_)]
        ms, host = event_ms(fn)
        return ms, host, [m for m, _ in ms_]

    with tempfile.TemporaryDirectory() as tmp:
        run(True, tmp)
        run(False, tmp)
        tp, tl, hp, hl = [], [], [], []
        differ = gc_differ = 0
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
                gc_differ += int((a.GC() != b.GC()).sum())
    sp, sl = summary(tp, epochs, steps), summary(tl, epochs, steps)
    margin = sp["spread_ms"] + sl["spread_ms"]
    return {"fits": R, "epochs": epochs, "steps_per_epoch": steps, "pack": sp, "loop": sl,
            "pack_host_ms": statistics.median(hp), "loop_host_ms": statistics.median(hl),
            "ratio_loop_over_pack": sl["median_ms"] / sp["median_ms"], "margin_ms": margin,
            "accepted": bool(sp["median_ms"] - sl["median_ms"] <= margin),
            "pack_faster_by_more_than_margin": bool(sl["median_ms"] - sp["median_ms"] > margin),
            "state_elements_that_differ": differ, "causal_matrix_elements_that_differ": gc_differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--epochs-b", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "navar_lstm_fit.json"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(N=NN, H=H, Tp=K, B=B, n=N), "adam": ADAM,
           "protocol": "warm-up of both routes, then %d runs each between HIP events, routes alternated" % args.reps,
           "kernels": kernel_times()}
    print(json.dumps({"kernels": res["kernels"]}), flush=True)
    res["a"] = workload_a(args.epochs, args.reps)
    print(json.dumps({"a": {k: v for k, v in res["a"].items() if not isinstance(v, dict)}}), flush=True)
    res["b"] = workload_b(args.epochs_b, args.reps)
    print(json.dumps({"b": {k: v for k, v in res["b"].items() if not isinstance(v, dict)}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
