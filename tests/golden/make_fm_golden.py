"""Generate tests/golden/cmlp_fm.npz from the REFERENCE itself (build container only).

    python tests/golden/make_fm_golden.py

The reference's cMLP forecasting baseline (models/cmlp_fm.py:58-475) on seeded models and data; the
reference is imported as in make_cemb_recording_golden.py (oracle/ref_import.py) plus models.cmlp_fm.
Only data leaves this script.  Keys, per scenario s in (a, b, c):
  s/meta               JSON: shapes, coefficients, Adam settings, seeds
  s/X_train, s/X_val   (N, L + 1, p) float32 windows, batched in order in batches of B (last ragged)
  s/init/<key>         state_dict (the factors.* keys) after seeded construction
  s/epoch<e>/<key>     ... after epoch e of batch_updates with Adam(lr 1e-3, eps 1e-4, weight_decay 1e-4)
  s/val_raw, s/val_norm  validate_training's tuple after the last epoch, report_normalized_loss_components
                       False / True
and for scenario a a whole fit (max_iter 3, lookback 1, check_every 10) of a fresh seeded model:
  a/fit/GC             (n_graphs, p, p, L) true graphs
  a/fit/pkl/<key>      every key of training_meta_data_and_hyper_parameters.pkl (histories as arrays;
                       gc_factor_l1_loss_histories as its first row, the number of rows beside it)
  a/fit/final/<key>    state_dict after fit
  a/fit/final_loss     fit's return value
Each scenario also runs in float64; the script asserts that the reference's own fp32 states deviate
from it by less than a quarter of the state bound the tests use (rtol 2e-4, atol 5e-6 * max(1, |want|max)).
"""
import importlib
import json
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402

REF = import_reference()
FM = importlib.import_module("models.cmlp_fm")

ADAM = dict(lr=1e-3, eps=1e-4, weight_decay=1e-4)
SCENARIOS = {
    # ragged last batch of 2
    "a": dict(p=4, L=2, h=5, B=6, N=20, Nval=14, epochs=3, seed=5, forecast=1.0, adj=0.1),
    # the D4IC baseline shape
    "b": dict(p=10, L=2, h=50, B=128, N=300, Nval=150, epochs=2, seed=7, forecast=10.0, adj=0.01),
    # nothing a multiple of 4 or 16
    "c": dict(p=7, L=3, h=33, B=16, N=40, Nval=19, epochs=3, seed=9, forecast=0.5, adj=0.2),
}


def coeffs(cfg):
    return {"FORECAST_COEFF": cfg["forecast"], "ADJ_L1_REG_COEFF": cfg["adj"], "DAGNESS_REG_COEFF": 0.0,
            "DAGNESS_LAG_COEFF": 0.0, "DAGNESS_NODE_COEFF": 0.0}


def windows(rng, N, T, p):
    X = rng.randn(N, T, p).astype(np.float32)
    for t in range(1, T):
        X[:, t] += 0.5 * np.roll(X[:, t - 1], 1, axis=1) - 0.2 * X[:, t - 1]
    return X


def loader(X, B, dtype):
    X = torch.from_numpy(X).to(dtype)
    return [(X[i:i + B], None) for i in range(0, X.shape[0], B)]


def build(cfg, dtype):
    torch.manual_seed(cfg["seed"])
    m = FM.cMLP_FM(cfg["p"], cfg["L"], [cfg["h"]], None, cfg["L"], 1, coeffs(cfg)).float()
    return m.double() if dtype == torch.float64 else m


def fac_state(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items() if k.startswith("factors."))


def run(cfg, Xtr, Xva, dtype):
    m = build(cfg, dtype)
    states = [fac_state(m)]
    opt = torch.optim.Adam(m.gen_model.parameters(), **ADAM)
    tr, va = loader(Xtr, cfg["B"], dtype), loader(Xva, cfg["B"], dtype)
    for _ in range(cfg["epochs"]):
        for bn, (X, _) in enumerate(tr):
            m.batch_update(bn, X, opt, cfg["L"], 1)
        states.append(fac_state(m))
    raw = m.validate_training(va, cfg["L"], 1, cfg["p"], report_normalized_loss_components=False)
    nrm = m.validate_training(va, cfg["L"], 1, cfg["p"], report_normalized_loss_components=True)
    return states, np.asarray(raw, dtype=np.float64), np.asarray(nrm, dtype=np.float64)


def check_conditioning(name, s32, s64):
    worst = 0.0
    for a, b in zip(s32[1:], s64[1:]):
        for k in a:
            want = b[k].astype(np.float64)
            bound = 2e-4 * np.abs(want) + 5e-6 * max(1.0, float(np.abs(want).max()))
            worst = max(worst, float((np.abs(a[k].astype(np.float64) - want) / bound).max()))
    print("scenario %s: fp32 vs fp64 deviation = %.3f %% of the state bound" % (name, 100 * worst))
    assert worst < 0.25, (name, worst)


def as_array(v):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    if isinstance(v, dict):  # {threshold: [[...] per graph]}
        assert list(v.keys()) == [0.0]
        v = v[0.0]
    return np.asarray(v, dtype=np.float64)


def whole_fit(cfg, Xtr, Xva, out, pre):
    rng = np.random.RandomState(cfg["seed"] + 300)
    GC = [(rng.rand(cfg["p"], cfg["p"], cfg["L"]) < 0.35).astype(np.float64) for _ in range(2)]
    for g in GC:
        g[0, 0, 0], g[1, 0, :] = 1.0, 0.0  # both classes present
    m = build(cfg, torch.float32)
    opt = torch.optim.Adam(m.gen_model.parameters(), **ADAM)
    with tempfile.TemporaryDirectory() as tmp:
        final = m.fit(tmp, loader(Xtr, cfg["B"], torch.float32), opt, cfg["L"], 1, 1, 3, lookback=1, check_every=10,
                      verbose=0, GC=GC, X_val=loader(Xva, cfg["B"], torch.float32))
        with open(os.path.join(tmp, "training_meta_data_and_hyper_parameters.pkl"), "rb") as f:
            meta = pickle.load(f)
    out[pre + "GC"] = np.stack(GC)
    for k, v in meta.items():
        if k == "gc_factor_l1_loss_histories":  # one list per true graph, only the first ever filled (:312-321)
            assert all(len(row) == 0 for row in v[1:])
            out[pre + "pkl/" + k] = as_array(v[0])
            out[pre + "pkl/" + k + "_rows"] = np.asarray(len(v))
        else:
            out[pre + "pkl/" + k] = as_array(v)
    for k, v in fac_state(m).items():
        out[pre + "final/" + k] = v
    out[pre + "final_loss"] = np.asarray(final, dtype=np.float64)


def main():
    out = {}
    for name, cfg in SCENARIOS.items():
        rng = np.random.RandomState(cfg["seed"] + 100)
        Xtr = windows(rng, cfg["N"], cfg["L"] + 1, cfg["p"])
        Xva = windows(rng, cfg["Nval"], cfg["L"] + 1, cfg["p"])
        s32, raw, nrm = run(cfg, Xtr, Xva, torch.float32)
        s64, _, _ = run(cfg, Xtr, Xva, torch.float64)
        check_conditioning(name, s32, s64)
        pre = name + "/"
        out[pre + "meta"] = np.asarray(json.dumps(dict(cfg, adam=ADAM)))
        out[pre + "X_train"], out[pre + "X_val"] = Xtr, Xva
        for e, st in enumerate(s32):
            for k, v in st.items():
                out[pre + ("init/" if e == 0 else "epoch%d/" % e) + k] = v
        out[pre + "val_raw"], out[pre + "val_norm"] = raw, nrm
        if name == "a":
            whole_fit(cfg, Xtr, Xva, out, pre + "fit/")
    path = os.path.join(HERE, "cmlp_fm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
