"""Time of fitting the supervised dCSFA-NMF baseline (redcliff_amd.FullDCSFAModel_GCv2) on one MI355X: the fused
route (redcliff_dcsfa_run, csrc/rc_dcsfa.hip, one native call per optimiser epoch) against the generic
torch-autograd route at the same commit, and fit_dcsfa_baselines against a loop of fits on the same route.

Shape: the published D4IC one (train/DCSFANMF_d4IC_OBPgs1.py): 10 nodes x 5 features = 500 inputs, hidden 256,
5 components, 5 supervised networks, batch 128; 2,048 seeded rows = 16 steps per epoch, 256 held-out rows, AdamW
lr 1e-3.  pretrain_NMF is the host's on both routes and is left out (pretrain=False).
Workloads:
  a  one model, whole fits of `--epochs` epochs (the per-epoch evaluation of both sets, the best-model saves and
     the last-epoch file included): fused against generic (REDCLIFF_DCSFA_PATH)
  b  15 models with per-model data, whole fits of `--epochs-b` epochs: fit_dcsfa_baselines against a loop of 15
     fused fits, including the host time to enqueue
Protocol (scripts/dgcnn_fit.py): per workload one warm-up of both sides, then --reps runs of each between two
HIP events on the stream, the two sides alternated; median [min - max].  A side is faster when it wins by more
than the two min-max spreads added together; the two sides of b must leave zero differing state elements.
Also recorded: the event time of one optimiser epoch's native call per step, and the library's build id.
Writes profiles/dcsfa_fit.json (or --out)."""
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

NODES, FEATURES, H, K, SUP = 10, 5, 256, 5, 5
D = NODES * NODES * FEATURES
B, N, NVAL, LR = 128, 2048, 256, 1e-3
ENV = "REDCLIFF_DCSFA_PATH"


def data(seed, rows):
    rng = np.random.RandomState(seed)
    y = rng.rand(rows, SUP).astype(np.float32)
    X = (0.5 * rng.rand(rows, D) + 0.5 * (y @ rng.rand(SUP, D))).astype(np.float32)
    return X, y


def model(folder):
    import redcliff_amd
    return redcliff_amd.FullDCSFAModel_GCv2(num_nodes=NODES, num_high_level_node_features=FEATURES, n_components=K,
                                            n_sup_networks=SUP, h=H, save_folder=folder, device="cuda",
                                            sup_smoothness_weight=2.0)


def fit_one(m, tr, va, epochs, seed):
    torch.manual_seed(seed)
    m.fit(tr[0], tr[1], n_epochs=epochs, batch_size=B, lr=LR, pretrain=False, X_val=va[0], y_val=va[1])


def epoch_call_times(reps=20):
    """Event time per step of one optimiser epoch's native call (16 steps of three launches)."""
    from redcliff_amd import dcsfa_nmf as dn
    os.environ[ENV] = "fused"
    try:
        with tempfile.TemporaryDirectory() as tmp:
            m = model(tmp)
            tr, va = data(1, N), data(2, NVAL)
            fit_one(m, tr, va, 1, 3)
            pack = m.__dict__["_dc_pack"]
            dev = dn.device_data(pack.device, [tr[0]], [tr[1]], [np.ones_like(tr[1])], [np.ones((N, 1), dtype=np.float32)])
            idx = torch.randint(0, N, (1, N), dtype=torch.int32, device=pack.device)
            out = {}
            for name, fn in (("train_epoch", lambda: pack.epoch(dn.TRAIN, idx, B, dev, LR)),
                             ("eval_pass", lambda: pack.evaluate(dev))):
                for _ in range(3):
                    fn()
                t = [event_ms(fn)[0] for _ in range(reps)]
                out[name + "_us_per_step"] = {"median": 1e3 * statistics.median(t) / (N // B), "min": 1e3 * min(t) / (N // B),
                                              "max": 1e3 * max(t) / (N // B)}
            out["workgroups"] = {"k_dc_fwd": H // dn.DC_HS, "k_dc_head": 1, "k_dc_bwd": H // dn.DC_HS}
            out["flops_per_step"] = 2 * 2 * B * D * H  # the two D x H contractions (forward, dW1)
            return out
    finally:
        os.environ.pop(ENV, None)


def workload_a(epochs, reps):
    tr, va = data(1, N), data(2, NVAL)
    steps = N // B

    def run(route, tmp):
        os.environ[ENV] = route
        try:
            m = model(tmp)
            out = event_ms(lambda: fit_one(m, tr, va, epochs, 10)) + (m,)
            assert ("_dc_pack" in m.__dict__) == (route == "fused")
            return out
        finally:
            os.environ.pop(ENV, None)
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
            "fused_faster": bool(sg["median_ms"] - sf["median_ms"] > margin)}


def workload_b(epochs, reps, R=15):
    import redcliff_amd
    sets = [(data(100 + i, N), data(200 + i, NVAL)) for i in range(R)]
    steps = N // B
    seeds = [300 + i for i in range(R)]

    def run(side, tmp):
        os.environ[ENV] = "generic" if side == "generic_loop" else "fused"
        try:
            ms_ = [model(os.path.join(tmp, "%d" % i)) for i in range(R)]
            if side == "pack":
                fn = lambda: redcliff_amd.fit_dcsfa_baselines(ms_, [s[0][0] for s in sets], [s[0][1] for s in sets],
                                                              n_epochs=epochs, batch_size=B, lr=LR, pretrain=False,
                                                              X_vals=[s[1][0] for s in sets], y_vals=[s[1][1] for s in sets],
                                                              seeds=seeds)
            else:
                fn = lambda: [fit_one(m, sets[i][0], sets[i][1], epochs, seeds[i]) for i, m in enumerate(ms_)]
            ms, host = event_ms(fn)
            return ms, host, ms_
        finally:
            os.environ.pop(ENV, None)

    with tempfile.TemporaryDirectory() as tmp:
        for side in ("pack", "loop", "generic_loop"):
            run(side, tmp)
        t = {"pack": [], "loop": [], "generic_loop": []}
        host = {"pack": [], "loop": [], "generic_loop": []}
        differ = 0
        for _ in range(reps):
            kept = {}
            for side in t:
                ms, h, kept[side] = run(side, tmp)
                t[side].append(ms)
                host[side].append(h)
            for a, b in zip(kept["pack"], kept["loop"]):
                sa, sb = a.state_dict(), b.state_dict()
                differ += sum(int((sa[k] != sb[k]).sum()) for k in sa)
    s = dict((side, summary(v, epochs, steps)) for side, v in t.items())
    margin = s["pack"]["spread_ms"] + s["loop"]["spread_ms"]
    margin_g = s["pack"]["spread_ms"] + s["generic_loop"]["spread_ms"]
    return {"fits": R, "epochs": epochs, "steps_per_epoch": steps, "pack": s["pack"], "loop": s["loop"],
            "generic_loop": s["generic_loop"], "host_ms": dict((side, statistics.median(v)) for side, v in host.items()),
            "ratio_loop_over_pack": s["loop"]["median_ms"] / s["pack"]["median_ms"],
            "ratio_generic_loop_over_pack": s["generic_loop"]["median_ms"] / s["pack"]["median_ms"],
            "pack_faster_than_loop": bool(s["loop"]["median_ms"] - s["pack"]["median_ms"] > margin),
            "pack_faster_than_generic_loop": bool(s["generic_loop"]["median_ms"] - s["pack"]["median_ms"] > margin_g),
            "state_elements_that_differ": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--epochs-b", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcsfa_fit.json"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from redcliff_amd import _native as nat
    from redcliff_amd import dcsfa_nmf as dn
    res = {"device": torch.cuda.get_device_name(0), "build_id": nat.build_id(), "B": B, "N": N, "N_val": NVAL, "lr": LR,
           "shape": {"D": D, "h": H, "K": K, "sup": SUP}, "default_path": dn.DEFAULT_PATH,
           "protocol": "warm-up of every side, then %d runs each between HIP events, sides alternated" % args.reps}
    res["kernels"] = epoch_call_times()
    print(json.dumps({"kernels": res["kernels"]}), flush=True)
    res["a"] = workload_a(args.epochs, args.reps)
    print(json.dumps({"a": {k: v for k, v in res["a"].items() if not isinstance(v, dict)}}), flush=True)
    res["b"] = workload_b(args.epochs_b, args.reps)
    print(json.dumps({"b": {k: v for k, v in res["b"].items() if not isinstance(v, dict)}}), flush=True)
    res["fused_is_faster_for_one_fit_and_for_15"] = bool(res["a"]["fused_faster"] and res["b"]["pack_faster_than_generic_loop"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
