"""Generate tests/golden/dgcnn_fit.npz (scenarios a-d) and dgcnn_fit_e.npz (scenario e) from the REFERENCE
itself (build container only).

    python tests/golden/make_dgcnn_fit_golden.py

The reference's supervised DGCNN baseline (models/dgcnn.py:63-237) on seeded models and data; the reference is
imported as in make_fm_golden.py (oracle/ref_import.py) plus models.dgcnn, unchanged (its two plotting calls
are replaced by no-ops).  Only data leaves this script.  Keys, per scenario s in (a, b, c, d, e):
  s/meta               JSON: shapes, Adam settings, seeds
  s/X, s/Y             (N, T, n) float32 windows and the raw labels ((N, C), (N, C, F + 2) or (N, C, 1))
  s/Ysel               the labels batch_update compares against, (N, C)
  s/X_val, s/Y_val     the held-out set (N // 2 windows), same label rank
  s/loss               every step's loss, in order
  s/init/<key>         state_dict after seeded construction (not for d, e: torch.manual_seed(seed) rebuilds it)
  s/epoch<e>/<key>     ... after epoch e of the reference's batch_update loop (d, e: after the last epoch only)
  s/eval               training_eval on the held-out set after the last epoch
and for scenarios a and c a whole reference fit() of a fresh seeded model (max_iter 7, check_every 2,
lookback 1, the held-out set as val_loader):
  s/fit/final/<key>, s/fit/GC (GC(threshold=False)), s/fit/loss (the returned value), s/fit/stopped_at
Loaders are lists of (X, Y) batches of B rows in order, the last one shorter when B does not divide N.
Each scenario also runs in float64; the script asserts that the reference's own fp32 states deviate from
it by less than a quarter of the state bound the tests use (rtol 2e-4, atol 5e-6 * max(1, |want|max)).
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

with contextlib.redirect_stdout(io.StringIO()):
    REF = import_reference()
    DG = importlib.import_module("models.dgcnn")
DG.plot_curve = lambda *a, **k: None
DG.plot_gc_est_comparissons_by_factor = lambda *a, **k: None

PUBLISHED = dict(lr=1e-4, eps=1e-4, weight_decay=1e-4)
SCENARIOS = {
    # ragged last batch of 2, weight decay, two layers
    "a": dict(n=3, F=2, layers=2, H=5, C=2, B=6, N=20, T=4, yrank="2d", epochs=3, seed=5,
              adam=dict(lr=1e-3, eps=1e-4, weight_decay=1e-4)),
    # three layers, nothing a multiple of 4 or 16, labels picked at index F
    "b": dict(n=5, F=3, layers=3, H=33, C=3, B=16, N=40, T=6, yrank="3d", epochs=3, seed=17, adam=dict(lr=1e-3)),
    # one layer: A has no gradient and must keep its initial bits
    "c": dict(n=4, F=2, layers=1, H=7, C=5, B=16, N=32, T=3, yrank="3d1", epochs=2, seed=9, adam=dict(lr=1e-3)),
    # the published D4IC shape
    "d": dict(n=10, F=2, layers=1, H=100, C=5, B=128, N=300, T=4, yrank="2d", epochs=2, seed=11, adam=PUBLISHED),
    # the published synthetic-systems grid shape (seed: the first of 21, 22, .. that meets the float64 rule
    # below; at 21 the reference's own fp32 run is 27 % of the bound away from its float64 run)
    "e": dict(n=10, F=2, layers=3, H=250, C=3, B=128, N=300, T=4, yrank="2d", epochs=2, seed=22, adam=PUBLISHED),
}
LAST_ONLY = ("d", "e")


def data(rng, cfg, N):
    X = rng.rand(N, cfg["T"], cfg["n"]).astype(np.float32)
    shape = {"2d": (N, cfg["C"]), "3d": (N, cfg["C"], cfg["F"] + 2), "3d1": (N, cfg["C"], 1)}[cfg["yrank"]]
    Y = rng.rand(*shape).astype(np.float32)
    Ysel = Y if cfg["yrank"] == "2d" else Y[:, :, cfg["F"] if cfg["yrank"] == "3d" else 0]
    return X, Y, np.ascontiguousarray(Ysel)


def loader(X, Y, B, dtype):
    X, Y = torch.from_numpy(X).to(dtype), torch.from_numpy(Y).to(dtype)
    return [(X[i:i + B], Y[i:i + B]) for i in range(0, X.shape[0], B)]


class Counted(DG.DGCNN_Model):
    """The reference's class, counting its batch_update calls (the epoch a fit stopped at)."""
    calls = 0

    def batch_update(self, *a, **k):
        Counted.calls += 1
        return super().batch_update(*a, **k)


def build(cfg, dtype, cls=DG.DGCNN_Model):
    torch.manual_seed(cfg["seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        m = cls(cfg["n"], 1, cfg["F"], cfg["layers"], cfg["H"], cfg["C"]).float()
    return m.double() if dtype == torch.float64 else m


def state(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


def run(cfg, tr, va, dtype):
    """The body of the reference's fit (:130-141) with every step's loss and every epoch's state kept."""
    m = build(cfg, dtype)
    states = [state(m)]
    opt = torch.optim.Adam(m.dgcnn.parameters(), **cfg["adam"])
    train_loader, val_loader = loader(tr[0], tr[1], cfg["B"], dtype), loader(va[0], va[1], cfg["B"], dtype)
    losses = []
    torch.set_default_dtype(dtype)  # the torcheeg restatement's torch.eye takes the default dtype
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(cfg["epochs"]):
                for bn, (X, Y) in enumerate(train_loader):
                    losses.append(m.batch_update(bn, X, Y, opt, 0.))
                states.append(state(m))
            ev = m.training_eval(val_loader)
    finally:
        torch.set_default_dtype(torch.float32)
    return m, opt, states, np.asarray(losses, dtype=np.float64), float(ev)


def check_conditioning(name, s32, s64):
    worst = 0.0
    for a, b in zip(s32[1:], s64[1:]):
        for k in a:
            if k.endswith("num_batches_tracked"):
                assert int(a[k]) == int(b[k])
                continue
            want = b[k].astype(np.float64)
            bound = 2e-4 * np.abs(want) + 5e-6 * max(1.0, float(np.abs(want).max()))
            worst = max(worst, float((np.abs(a[k].astype(np.float64) - want) / bound).max()))
    print("scenario %s: fp32 vs fp64 deviation = %.3f %% of the state bound" % (name, 100 * worst))
    assert worst < 0.25, (name, worst)


def whole_fit(cfg, tr, va, out, pre):
    m = build(cfg, torch.float32, Counted)
    opt = torch.optim.Adam(m.dgcnn.parameters(), **cfg["adam"])
    train_loader, val_loader = loader(tr[0], tr[1], cfg["B"], torch.float32), loader(va[0], va[1], cfg["B"], torch.float32)
    Counted.calls = 0
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        lv = m.fit(tmp, train_loader, opt, 7, 1, 2, 0, [np.zeros((cfg["n"], cfg["n"]))], val_loader)
        assert os.path.exists(os.path.join(tmp, "final_best_model.bin"))
    for k, v in state(m).items():
        out[pre + "final/" + k] = v
    out[pre + "GC"] = m.GC(threshold=False).detach().cpu().numpy().copy()
    out[pre + "loss"] = np.asarray(float(lv), dtype=np.float64)
    out[pre + "stopped_at"] = np.asarray(Counted.calls // len(train_loader) - 1, dtype=np.int64)
    print("   whole fit: stopped at it = %d, returned %.6g" % (int(out[pre + "stopped_at"]), float(lv)))


def main():
    out = {}
    for name, cfg in SCENARIOS.items():
        rng = np.random.RandomState(cfg["seed"] + 100)
        tr = data(rng, cfg, cfg["N"])
        va = data(rng, cfg, cfg["N"] // 2)
        m32, opt32, s32, loss, ev = run(cfg, tr, va, torch.float32)
        _, _, s64, loss64, ev64 = run(cfg, tr, va, torch.float64)
        check_conditioning(name, s32, s64)
        print("   loss fp32 vs fp64: max rel %.2e; eval %.2e" % (float(np.max(np.abs(loss - loss64) / np.abs(loss64))),
                                                                 abs(ev - ev64) / abs(ev64)))
        if cfg["layers"] == 1:
            assert m32.dgcnn.A.grad is None and m32.dgcnn.A not in opt32.state
            assert np.array_equal(s32[0]["dgcnn.A"], s32[-1]["dgcnn.A"])
        pre = name + "/"
        out[pre + "meta"] = np.asarray(json.dumps(cfg))
        out[pre + "X"], out[pre + "Y"], out[pre + "Ysel"] = tr
        out[pre + "X_val"], out[pre + "Y_val"] = va[0], va[1]
        out[pre + "loss"] = loss
        out[pre + "eval"] = np.asarray(ev, dtype=np.float64)
        for e, st in enumerate(s32):
            if name in LAST_ONLY and e != cfg["epochs"]:
                continue
            for k, v in st.items():
                out[pre + ("init/" if e == 0 else "epoch%d/" % e) + k] = v
        if name in ("a", "c"):
            whole_fit(cfg, tr, va, out, pre + "fit/")
    # scenario e's fc1 alone is 640 KB of incompressible floats: it gets a file of its own, so that each
    # committed file stays under 1 MiB
    for fname, keep in (("dgcnn_fit.npz", lambda k: not k.startswith("e/")), ("dgcnn_fit_e.npz", lambda k: k.startswith("e/"))):
        part = dict((k, v) for k, v in out.items() if keep(k))
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **part)
        print("wrote", path, len(part), "arrays,", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
