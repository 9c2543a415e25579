"""Generate tests/golden/navar_lstm.npz from the REFERENCE itself (build container only).

    python tests/golden/make_navar_lstm_golden.py

The reference's NAVARLSTM (models/navar.py:129-246) on seeded models and data; the reference is imported
as in make_navar_golden.py (oracle/ref_import.py) plus models.navar, unchanged.  Only data leaves this
script.  Keys, per scenario s in (a, b, c, d, w):
  s/meta               JSON: shapes (Tp = LSTM steps, windows have Tp + 1 rows), Adam settings, lambda1, seeds
  s/X_train            (n, Tp + 1, N) float32 windows (rows [0, Tp) the inputs, row Tp the target)
  s/perm<e>            epoch e's np.random.choice permutation under np.random.seed(seed + 200) (absent
                       when batch_size >= n: the reference draws nothing)
  s/mse, s/l1          every step's criterion value and L1 term, in order
  s/init/<key>         state_dict after seeded construction (not for w)
  s/epoch<e>/<key>     ... after epoch e of the reference's step (w: after the last epoch only, and its
                       weight_hh_l0 tensors -- 1 MB each -- as every WHH_STRIDE-th element of the flat
                       tensor, so that the file stays under the size limit of a committed file)
  s/causal             the final causal matrix (N, N)
and for scenarios a and b a whole reference fit() of a fresh seeded model under np.random.seed(seed + 300),
epochs as the scenario, check_every 2, val_proportion 0 (the reference's validation line raises with
val_proportion > 0: it compares (n, N, Tp) with (n, N)):
  s/fit0/final/<key>, s/fit0/causal, s/fit0/loss_val
Each scenario also runs in float64; the script asserts that the reference's own fp32 states deviate from
it by less than a quarter of the state bound the tests use (rtol 2e-4, atol 5e-6 * max(1, |want|max)); a
seed that fails the quarter is replaced by the next one.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402

REF = import_reference()
NV = importlib.import_module("models.navar")

WHH_STRIDE = 13
ADAM_A = dict(lr=1e-3, weight_decay=1e-4)
SCENARIOS = {
    # ragged last batch of 2; L1 gradient at every time step
    "a": dict(N=3, H=5, Tp=3, B=6, n=20, epochs=3, seed=5, lam=0.1, adam=ADAM_A),
    # nothing a multiple of 4 or 16; three unit slices
    "b": dict(N=4, H=33, Tp=5, B=16, n=40, epochs=3, seed=17, lam=0.05, adam=ADAM_A),
    # a sequence of one step (dWhh exactly 0); n a multiple of B: the empty third slice is dropped
    "c": dict(N=2, H=4, Tp=1, B=16, n=32, epochs=2, seed=9, lam=0.0, adam=ADAM_A),
    # batch_size >= n: one batch, no RNG draw
    "d": dict(N=3, H=5, Tp=3, B=300, n=10, epochs=2, seed=11, lam=0.1, adam=ADAM_A),
    # the published width (num_hidden 256, 20 steps, batch 128, lr 1e-4) on three nodes
    "w": dict(N=3, H=256, Tp=20, B=128, n=300, epochs=2, seed=21, lam=0.0, adam=dict(lr=1e-4)),
}


def windows(rng, n, T, N):
    X = rng.randn(n, T, N).astype(np.float32)
    for t in range(1, T):
        X[:, t] += 0.5 * np.roll(X[:, t - 1], 1, axis=1) - 0.2 * X[:, t - 1]
    return X


def build(cfg, dtype):
    torch.manual_seed(cfg["seed"])
    m = NV.NAVARLSTM(cfg["N"], cfg["H"], cfg["Tp"], hidden_layers=1, dropout=0).float()
    return m.double() if dtype == torch.float64 else m


def state(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


def run(cfg, Xtr, dtype):
    """The body of the reference's fit (:194-243) with every step's loss terms and every epoch's state kept."""
    m = build(cfg, dtype)  # constructed (and initialised) under the float32 default, then converted
    # the reference's forward builds its contributions as torch.zeros of the DEFAULT dtype
    # (models/navar.py:159): the float64 run needs that default to be float64, for this run only
    torch.set_default_dtype(dtype)
    try:
        return _run(m, cfg, Xtr, dtype)
    finally:
        torch.set_default_dtype(torch.float32)


def _run(m, cfg, Xtr, dtype):
    states = [state(m)]
    opt = torch.optim.Adam(m.parameters(), **cfg["adam"])
    crit = torch.nn.MSELoss()
    X = torch.from_numpy(np.swapaxes(Xtr, 2, 1)).to(dtype)
    n, B = X.size()[0], cfg["B"]
    np.random.seed(cfg["seed"] + 200)
    perms, mse, l1 = [], [], []
    for _ in range(cfg["epochs"]):
        if B < n:
            perm = np.random.choice(n, size=n, replace=False)
            perms.append(perm.copy())
            batches = [perm[i * B:(i + 1) * B] for i in range(int(n / B) + 1)]
            batches = [b for b in batches if len(b) > 0]
        else:
            batches = [np.arange(n)]
        for idx in batches:
            pred, contrib = m.forward(X[idx][:, :, :-1].to(dtype))
            lp = crit(pred[:, :, -1], X[idx][:, :, -1])
            ll = (cfg["lam"] / m.num_nodes) * torch.mean(torch.sum(torch.abs(contrib), dim=1))
            opt.zero_grad()
            (lp + ll).backward()
            opt.step()
            mse.append(float(lp.detach()))
            l1.append(float(ll.detach()))
        states.append(state(m))
    m.eval()
    _, contrib = m.forward(X[:, :, :-1])
    causal = torch.std(contrib, dim=0).view(m.num_nodes, m.num_nodes).detach().cpu().numpy()
    return states, perms, np.asarray(mse), np.asarray(l1), causal


def conditioning(s32, s64):
    worst = 0.0
    for a, b in zip(s32[1:], s64[1:]):
        for k in a:
            want = b[k].astype(np.float64)
            bound = 2e-4 * np.abs(want) + 5e-6 * max(1.0, float(np.abs(want).max()))
            worst = max(worst, float((np.abs(a[k].astype(np.float64) - want) / bound).max()))
    return worst


def whole_fit(cfg, Xtr, out, pre):
    m = build(cfg, torch.float32)
    opt = torch.optim.Adam(m.parameters(), **cfg["adam"])
    np.random.seed(cfg["seed"] + 300)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        lv = m.fit(tmp, Xtr.copy(), None, torch.nn.MSELoss(), opt, val_proportion=0.0, epochs=cfg["epochs"],
                   batch_size=cfg["B"], check_every=2, lambda1=cfg["lam"])
    for k, v in state(m).items():
        out[pre + "final/" + k] = v
    out[pre + "causal"] = np.asarray(m.GC())
    out[pre + "loss_val"] = np.asarray(float(lv), dtype=np.float64)


def main():
    out = {}
    for name, cfg in SCENARIOS.items():
        while True:
            rng = np.random.RandomState(cfg["seed"] + 100)
            Xtr = windows(rng, cfg["n"], cfg["Tp"] + 1, cfg["N"])
            s32, perms, mse, l1, causal = run(cfg, Xtr, torch.float32)
            s64, perms64, _, _, causal64 = run(cfg, Xtr, torch.float64)
            assert all(np.array_equal(a, b) for a, b in zip(perms, perms64))
            worst = conditioning(s32, s64)
            print("scenario %s seed %d: fp32 vs fp64 deviation = %.3f %% of the state bound" % (name, cfg["seed"], 100 * worst))
            if worst < 0.25:
                break
            cfg["seed"] += 1
        print("   causal fp32 vs fp64: max rel %.2e (min entry %.3g)" % (
            float(np.max(np.abs(causal - causal64) / np.abs(causal64))), float(np.abs(causal64).min())))
        pre = name + "/"
        meta = dict(cfg)
        if name == "w":
            meta["whh_stride"] = WHH_STRIDE
        out[pre + "meta"] = np.asarray(json.dumps(meta))
        out[pre + "X_train"] = Xtr
        for e, p in enumerate(perms):
            out[pre + "perm%d" % (e + 1)] = p.astype(np.int64)
        out[pre + "mse"], out[pre + "l1"], out[pre + "causal"] = mse, l1, causal
        for e, st in enumerate(s32):
            if name == "w" and e != cfg["epochs"]:
                continue
            for k, v in st.items():
                if name == "w" and k.endswith("weight_hh_l0"):
                    v = v.reshape(-1)[::WHH_STRIDE].copy()
                out[pre + ("init/" if e == 0 else "epoch%d/" % e) + k] = v
        if name in ("a", "b"):
            whole_fit(cfg, Xtr, out, pre + "fit0/")
    path = os.path.join(HERE, "navar_lstm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
