"""Time of fitting the supervised DGCNN baseline (redcliff_amd.DGCNN_Model) on one MI355X: the fused route
(redcliff_dgcnn_fit_run, csrc/rc_dgcnn_fit.hip, one native call per epoch) against the generic torch-autograd
route, and fit_dgcnn_baselines against a loop of fused fits.

Shapes: the two published ones, 2,048 seeded windows = 16 steps per epoch, Adam lr 1e-4, eps 1e-4, weight
decay 1e-4 (train/DGCNN_d4IC_BLgs1Parsim.py, train/DGCNN_synSysInnovGauss1030_BLgs2_mi300.py):
  d4ic  10 nodes, 2 features, 1 layer, hid 100, 5 classes, batch 128
  grid  10 nodes, 2 features, 3 layers, hid 250, 3 classes, batch 128
Workloads, each at both shapes:
  a  one model, whole fits of `--epochs` epochs (one check at epoch 0, the saves and the final evaluation
     included): fused against generic (REDCLIFF_DGCNN_PATH=generic)
  b  15 models with per-model data, whole fits of `--epochs-b` epochs: fit_dgcnn_baselines against a loop of
     15 fused fits, including the host time to enqueue
Protocol (scripts/navar_fit.py): per workload one warm-up of both routes, then --reps runs of each between
two HIP events on the stream, the two routes alternated; median [min - max].
Acceptance: the fused side must be faster by more than the two min-max spreads added
together, and the two routes of b leave zero differing state elements.
Also recorded: each kernel's event time per step (one-step TRAIN calls restricted to one of the three
launches by RedcliffDgcnnFitArgs.launches, after a full step has filled the workspace), the whole step's, and
the library's build id.  Writes profiles/dgcnn_fit.json (or --out)."""
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

SHAPES = {"d4ic": (10, 2, 1, 100, 5), "grid": (10, 2, 3, 250, 3)}  # nodes, F, layers, hid, classes
B, N, T, NVAL = 128, 2048, 4, 256
ADAM = dict(lr=1e-4, eps=1e-4, weight_decay=1e-4)


def loaders(shape, seed):
    rng = np.random.RandomState(seed)
    n, C = shape[0], shape[4]
    mk = lambda rows: (torch.from_numpy(rng.rand(rows, T, n).astype(np.float32)), torch.from_numpy(rng.rand(rows, C).astype(np.float32)))
    cut = lambda XY: [(XY[0][i:i + B], XY[1][i:i + B]) for i in range(0, len(XY[0]), B)]
    return cut(mk(N)), cut(mk(NVAL))


def model(shape, seed):
    import redcliff_amd
    torch.manual_seed(seed)
    n, F, layers, H, C = shape
    m = redcliff_amd.DGCNN_Model(n, 1, F, layers, H, C).to("cuda")
    return m, torch.optim.Adam(m.dgcnn.parameters(), **ADAM)


def step_flops(shape):
    """Multiply-adds of one step counted as 2 flops: fc1 forward, dfc1 and dR (the rest is below 2 %)."""
    n, F, layers, H, C = shape
    return 3 * 2 * B * 64 * n * H


def fit_one(m, o, tr, va, tmp, epochs):
    return m.fit(tmp, tr, o, epochs, 1, 10 ** 6, 0, None, va)


def kernel_times(shape, reps=20):
    """Event time per step of the whole step and of each of its launches alone (the launch mask)."""
    from redcliff_amd import dgcnn as dg
    m, o = model(shape, 1)
    pack, r = m._slot()
    pack.bind_optimizer(r, o)
    tr, _ = loaders(shape, 2)
    X, Y = tr[0][0].cuda(), tr[0][1].cuda()
    loss = torch.empty(1, 1, device="cuda")
    ws = pack.workspace(B, B, 1)
    d, hyper = pack.dims(B, T), pack.hyper(0, [0])

    def call(mask):
        rc = dg.dgcnn_fit_run(d, dg.TRAIN, B, 1, 0, B, B, X, 0, Y, 0, pack.par, pack.m, pack.v, pack.np_, pack.rm, pack.rv,
                              hyper, loss, None, ws, launches=mask)
        assert rc == 0
    n, out = 20, {}
    for name, mask in (("step", 0), ("k_dg_fwd", 1), ("k_dg_bwd", 2), ("k_dg_tail", 4)):
        for _ in range(3):
            call(0)
        t = [event_ms(lambda: [call(mask) for _ in range(n)])[0] / n for _ in range(reps)]
        out[name + "_us"] = {"median": 1e3 * statistics.median(t), "min": 1e3 * min(t), "max": 1e3 * max(t)}
    s_us = out["step_us"]["median"]
    out.update(flops_per_step=step_flops(shape), step_tflops=step_flops(shape) / (s_us * 1e-6) / 1e12,
               workgroups_per_launch=shape[0], note="a masked call also runs the call's statistics launch")
    return out


def workload_a(shape, epochs, reps):
    tr, va = loaders(shape, 1)
    steps = len(tr)

    def run(route, tmp):
        os.environ["REDCLIFF_DGCNN_PATH"] = route
        try:
            m, o = model(shape, 10)
            out = event_ms(lambda: fit_one(m, o, tr, va, tmp, epochs)) + (m,)
            assert ("_dg_slot" in m.__dict__) == (route == "fused")
            return out
        finally:
            os.environ.pop("REDCLIFF_DGCNN_PATH", None)
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


def workload_b(shape, epochs, reps, R=15):
    import redcliff_amd
    data = [loaders(shape, 100 + i) for i in range(R)]
    steps = len(data[0][0])

    def run(packed, tmp):
        ms_ = [model(shape, 300 + i) for i in range(R)]
        dirs = [os.path.join(tmp, "%d" % i) for i in range(R)]
        if packed:
            fn = lambda: redcliff_amd.fit_dgcnn_baselines([m for m, _ in ms_], dirs, [d[0] for d in data], [o for _, o in ms_],
                                                          epochs, 1, 10 ** 6, 0, [None] * R, [d[1] for d in data])
        else:
            fn = lambda: [fit_one(m, o, data[i][0], data[i][1], dirs[i], epochs) for i, (m, o) in enumerate(ms_)]
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
            "accepted": bool(sl["median_ms"] - sp["median_ms"] > margin and differ == 0),
            "state_elements_that_differ": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--epochs-b", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dgcnn_fit.json"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from redcliff_amd import _native as nat
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(), "B": B, "N": N, "adam": ADAM,
           "protocol": "warm-up of both routes, then %d runs each between HIP events, routes alternated" % args.reps}
    for name, shape in SHAPES.items():
        r = {"shape": dict(zip(("nodes", "F", "layers", "hid", "classes"), shape)), "kernels": kernel_times(shape)}
        print(json.dumps({name: {"kernels": r["kernels"]}}), flush=True)
        r["a"] = workload_a(shape, args.epochs, args.reps)
        print(json.dumps({name: {"a": {k: v for k, v in r["a"].items() if not isinstance(v, dict)}}}), flush=True)
        r["b"] = workload_b(shape, args.epochs_b, args.reps)
        print(json.dumps({name: {"b": {k: v for k, v in r["b"].items() if not isinstance(v, dict)}}}), flush=True)
        res[name] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
