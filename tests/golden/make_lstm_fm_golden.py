"""Generate tests/golden/clstm_fm.npz from the REFERENCE itself (build container only).

    python tests/golden/make_lstm_fm_golden.py

The reference's cLSTM forecasting baseline (models/clstm_fm.py, models/clstm.py) on seeded models and
data; the reference is imported as in make_fm_golden.py (oracle/ref_import.py) plus models.clstm_fm.
Only data leaves this script.  Keys, per scenario s in (a, b, c):
  s/meta               JSON: shapes, coefficients, Adam settings, seeds
  s/X_train, s/X_val   (N, T, p) float32 recordings, batched in order in batches of B (last ragged);
                       only rows [0, Tm) of a recording are used (scenario a stores T = 6 > Tm = 4)
  s/init/<key>         state_dict (the factors.* keys) after seeded construction
  s/epoch<e>/<key>     ... after epoch e of batch_updates with Adam(lr, eps 1e-4, weight_decay 1e-4)
  s/sums               (epochs, 4) the four running sums batch_update returned at the end of each epoch
  s/val_raw, s/val_norm  training_sim_eval's five values after the last epoch,
                       report_normalized_loss_components False / True
and for scenario a a whole fit (max_iter 12, check_every 2, lookback 1, lr FIT_LR) of a fresh seeded model:
  a/fit/pkl/<key>      every key of training_meta_data_and_hyper_parameters.pkl as numbers
  a/fit/final/<key>    state_dict after fit
  a/fit/final_loss     fit's return value
  a/fit/stop_epoch     the epoch `it` at which the fit stopped (it stops before max_iter)
Each scenario also runs in float64 (arrange_input's and init_hidden's hard-coded float32 patched here
only); the script asserts that the reference's own fp32 states deviate from it by less than a quarter
of the state bound the tests use (rtol 2e-4, atol 5e-6 * max(1, |want|max)).
"""
import contextlib
import importlib
import io
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
FM = importlib.import_module("models.clstm_fm")
CL = importlib.import_module("models.clstm")

SCENARIOS = {
    # ragged last batch of 2, recording rows past Tm
    "a": dict(p=4, h=5, C=2, Tm=4, T=6, B=6, N=20, Nval=14, epochs=3, lr=1e-3, seed=5, forecast=1.0, adj=0.1),
    # the D4IC baseline shape
    "b": dict(p=10, h=25, C=2, Tm=4, T=4, B=128, N=300, Nval=150, epochs=2, lr=5e-4, seed=7, forecast=10.0, adj=0.01),
    # nothing a multiple of 4 or 16, S = 4
    "c": dict(p=7, h=13, C=5, Tm=9, T=9, B=16, N=40, Nval=19, epochs=3, lr=1e-3, seed=9, forecast=0.5, adj=0.2),
}
FIT = dict(max_iter=12, check_every=2, lookback=1)
FIT_LR = 2e-2  # at 1e-3 .. 1e-2 ||GC||_1 falls at every check and the reference runs all 12 epochs


def adam(lr):
    return dict(lr=lr, eps=1e-4, weight_decay=1e-4)


def coeffs(cfg):
    return {"FORECAST_COEFF": cfg["forecast"], "ADJ_L1_REG_COEFF": cfg["adj"], "DAGNESS_REG_COEFF": 0.0}


def recordings(rng, N, T, p):
    X = rng.randn(N, T, p).astype(np.float32)
    for t in range(1, T):
        X[:, t] += 0.5 * np.roll(X[:, t - 1], 1, axis=1) - 0.2 * X[:, t - 1]
    return X


def loader(X, B, dtype):
    X = torch.from_numpy(X).to(dtype)
    return [(X[i:i + B], None) for i in range(0, X.shape[0], B)]


def arrange_input_any_dtype(self, data, context):
    """models/clstm_fm.py:95-112 with the data's dtype in place of the hard-coded float32."""
    n = len(data) - context
    inp = torch.zeros(n, context, data.shape[1], dtype=data.dtype, device=data.device)
    tgt = torch.zeros(n, context, data.shape[1], dtype=data.dtype, device=data.device)
    for i in range(context):
        inp[:, i, :] = data[i:n + i]
        tgt[:, i, :] = data[i + 1:n + i + 1]
    return inp.detach(), tgt.detach()


def init_hidden_any_dtype(self, batch):
    w = self.lstm.weight_ih_l0
    return (torch.zeros(1, batch, self.hidden, device=w.device, dtype=w.dtype),
            torch.zeros(1, batch, self.hidden, device=w.device, dtype=w.dtype))


@contextlib.contextmanager
def float64_patches():
    a, b = FM.cLSTM_FM.arrange_input, CL.LSTM.init_hidden
    FM.cLSTM_FM.arrange_input, CL.LSTM.init_hidden = arrange_input_any_dtype, init_hidden_any_dtype
    try:
        yield
    finally:
        FM.cLSTM_FM.arrange_input, CL.LSTM.init_hidden = a, b


def build(cfg, dtype):
    torch.manual_seed(cfg["seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        m = FM.cLSTM_FM(cfg["p"], cfg["h"], None, cfg["C"], coeffs(cfg)).float()
    return m.double() if dtype == torch.float64 else m


def fac_state(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items() if k.startswith("factors."))


def run(cfg, Xtr, Xva, dtype):
    m = build(cfg, dtype)
    states, sums = [fac_state(m)], []
    opt = torch.optim.Adam(m.gen_model.parameters(), **adam(cfg["lr"]))
    tr, va = loader(Xtr, cfg["B"], dtype), loader(Xva, cfg["B"], dtype)
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(cfg["epochs"]):
            r = (0., 0., 0., 0.)
            for bn, (X, _) in enumerate(tr):
                r = m.batch_update(bn, X, cfg["Tm"], cfg["C"], opt, *r)
            sums.append(r)
            states.append(fac_state(m))
        raw = m.training_sim_eval(va, cfg["Tm"], cfg["C"], cfg["p"], return_loss_componentwise=True)
        nrm = m.training_sim_eval(va, cfg["Tm"], cfg["C"], cfg["p"], return_loss_componentwise=True,
                                  report_normalized_loss_components=True)
    return states, np.asarray(sums, dtype=np.float64), np.asarray(raw, dtype=np.float64), np.asarray(nrm, dtype=np.float64)


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
    return np.asarray(v, dtype=np.float64)


def whole_fit(cfg, Xtr, Xva, out, pre):
    m = build(cfg, torch.float32)
    opt = torch.optim.Adam(m.gen_model.parameters(), **adam(FIT_LR))
    tr, va = loader(Xtr, cfg["B"], torch.float32), loader(Xva, cfg["B"], torch.float32)
    calls = [0]
    inner = FM.cLSTM_FM.batch_update

    def counted(self, *a, **kw):
        calls[0] += 1
        return inner(self, *a, **kw)
    FM.cLSTM_FM.batch_update = counted
    GC = [np.eye(cfg["p"])]
    try:
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            final = m.fit(tmp, tr, opt, cfg["C"], cfg["Tm"], 1, FIT["max_iter"], lookback=FIT["lookback"],
                          check_every=FIT["check_every"], verbose=0, GC=GC, X_val=va)
            with open(os.path.join(tmp, "training_meta_data_and_hyper_parameters.pkl"), "rb") as f:
                meta = pickle.load(f)
    finally:
        FM.cLSTM_FM.batch_update = inner
    assert calls[0] % len(tr) == 0
    stop = calls[0] // len(tr) - 1
    assert stop < FIT["max_iter"] - 1, "the fit must stop early (epochs run: %d)" % (stop + 1)
    for k, v in meta.items():
        out[pre + "pkl/" + k] = as_array(v)
    for k, v in fac_state(m).items():
        out[pre + "final/" + k] = v
    out[pre + "final_loss"] = np.asarray(final, dtype=np.float64)
    out[pre + "stop_epoch"] = np.asarray(stop)
    out[pre + "lr"] = np.asarray(FIT_LR)
    print("whole fit: stopped at epoch", stop, "pickle epoch", meta["epoch"], "best_loss", float(meta["best_loss"].detach()))


def main():
    out = {}
    for name, cfg in SCENARIOS.items():
        rng = np.random.RandomState(cfg["seed"] + 100)
        Xtr = recordings(rng, cfg["N"], cfg["T"], cfg["p"])
        Xva = recordings(rng, cfg["Nval"], cfg["T"], cfg["p"])
        s32, sums, raw, nrm = run(cfg, Xtr, Xva, torch.float32)
        again, _, _, _ = run(cfg, Xtr, Xva, torch.float32)
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(s32, again) for k in a), "two fp32 runs differ"
        with float64_patches():
            s64, _, _, _ = run(cfg, Xtr, Xva, torch.float64)
        check_conditioning(name, s32, s64)
        pre = name + "/"
        out[pre + "meta"] = np.asarray(json.dumps(dict(cfg, adam=adam(cfg["lr"]), fit=dict(FIT, lr=FIT_LR))))
        out[pre + "X_train"], out[pre + "X_val"] = Xtr, Xva
        for e, st in enumerate(s32):
            for k, v in st.items():
                out[pre + ("init/" if e == 0 else "epoch%d/" % e) + k] = v
        out[pre + "sums"] = sums
        out[pre + "val_raw"], out[pre + "val_norm"] = raw, nrm
        if name == "a":
            whole_fit(cfg, Xtr, Xva, out, pre + "fit/")
    path = os.path.join(HERE, "clstm_fm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
