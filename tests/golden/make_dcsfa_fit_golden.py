"""Generate tests/golden/dcsfa_fit.npz (scenarios a-c) and dcsfa_fit_d.npz (scenario d) from the REFERENCE
itself (build container only).

    python tests/golden/make_dcsfa_fit_golden.py

The reference's dCSFA-NMF baseline (models/dcsfa_nmf.py FullDCSFAModel for scenario b,
models/dcsfa_nmf_vanillaDirSpec.py FullDCSFAModel for a, c, d) on seeded models and data; the reference is
imported through oracle/ref_import.py, unchanged.  Its own fit() runs; subclasses defined here only listen
(the sampler's drawn rows, forward's two losses, the state at the points named below) and, for the float64
run, cast.  Only data leaves this script.  Keys, per scenario s in (a, b, c, d):
  s/meta                 JSON: shapes, model arguments, fit arguments, seed
  s/X, s/y, s/pw, s/tm   inputs (N, D), labels (N, sup), y_pred_weights (N, 1), task_mask (N, sup)
  s/X_val, s/y_val       a, c: the held-out set (N // 2 rows)
  s/init/<key>           state_dict after _initialize (not for d: torch.manual_seed(seed) rebuilds it)
  s/nmf/W_nmf            W_nmf after pretrain_NMF, so that no test depends on sklearn
  s/idx                  (n_pre_epochs + n_epochs, N) every optimiser epoch's drawn rows, in order
  s/loss_pre, s/loss     (steps, 2) every step's reconstruction and prediction loss (pretrain_encoder, main loop)
  s/pre/<key>            state_dict after pretrain_encoder (not for d)
  s/epoch<e>/<key>       ... after main epoch e (d: the last one only)
  s/hist/training, recon, pred   the per-epoch histories
  s/hist/recon_f64       ... of the float64 run: what fit() computes in eval mode reads the running mean against
                         the current bias (NOISE_KEYS below), and the tests allow four times the reference's own
                         fp32-to-float64 difference there; likewise val_recon_f64 and fit/X_recon_f64, y_pred_f64, s_f64
and for scenarios a and c, whose fit runs with the held-out set:
  s/hist/val_recon, val_pred, s/fit/best_epoch, s/fit/final/<key> (the state fit() ends with),
  s/fit/GC (GC(threshold=False)), s/fit/X_recon, y_pred, s (transform of the held-out set)
Scenario b's feature count is the directed-spectrum length nodes * features * (2 nodes - 1) = 135 its class's
GC needs.  Scenario d's X lies on a grid of 1/256 so that its file compresses under 1 MiB.
Each scenario also runs in float64; the script asserts that the reference's own fp32 states deviate from it
by less than a quarter of the state bound the tests use (rtol 2e-4, atol 5e-6 * max(1, |want|max)); see
NOISE_KEYS for the two tensors no run determines that closely, and scenario d's comment for the published
shape.  s/conditioning keeps the measured fraction.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    REF = import_reference()
    DS = importlib.import_module("models.dcsfa_nmf")
    VA = importlib.import_module("models.dcsfa_nmf_vanillaDirSpec")
for _m in (DS, VA):
    _m.plot_gc_est_comparissons_by_factor = lambda *a, **k: None
    _m.plot_reconstruction_comparisson = lambda *a, **k: None

SCENARIOS = {
    # ragged last batch of 8; one unsupervised component, so the residual differs from X
    "a": dict(cls="vanilla", nodes=3, features=3, D=27, h=33, K=3, sup=2, N=40, B=16, n_pre=2, n_epochs=3, seed=3,
              val=True, model=dict(sup_smoothness_weight=2.0, sup_weight=2.0), masks=False),
    # K equals sup: the unsupervised part is empty; nothing a multiple of 16; masks and weights
    "b": dict(cls="dirspec", nodes=5, features=3, D=135, h=70, K=4, sup=4, N=72, B=34, n_pre=2, n_epochs=3, seed=7,
              val=False, model=dict(), masks=True),
    # one supervised network out of three; the denominator is always positive
    "c": dict(cls="vanilla", nodes=4, features=2, D=32, h=16, K=3, sup=1, N=48, B=16, n_pre=2, n_epochs=3, seed=9,
              val=True, model=dict(sup_smoothness_weight=0.5), masks=False),
    # the published D4IC shape.  No seed meets the float64 rule below here: of the seeds 11 .. 149 the best is
    # 24, at 36 % of the state bound (most are far over 100 %).  With 128 x 256 activations a step, some
    # pre-activation lands within rounding of LeakyReLU's kink in most runs, and fp32 and float64 then take
    # different slopes for that row of the first Linear's weight (at seed 24 they do not, but row 43 of unit 214
    # is -5.06e-6 against -1.64e-6 in the eighth step).  The rule is asserted for a-c; for d the
    # figure is printed and kept in d/conditioning, and the run must stay inside the bound itself.
    "d": dict(cls="vanilla", nodes=10, features=5, D=500, h=256, K=5, sup=5, N=300, B=128, n_pre=1, n_epochs=2, seed=24,
              val=False, model=dict(sup_smoothness_weight=2.0), masks=False),
}
LAST_ONLY = ("d",)
LOG = {}


class RecordingSampler(torch.utils.data.WeightedRandomSampler):
    def __iter__(self):
        rows = list(super().__iter__())
        LOG["idx"].append(np.asarray(rows, dtype=np.int32))
        return iter(rows)


DS.WeightedRandomSampler = RecordingSampler
VA.WeightedRandomSampler = RecordingSampler


def state(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


class Listening:
    """Mixed in ahead of a reference class: listens, and casts for the float64 run."""
    dtype = torch.float32

    def _initialize(self, dim_in):
        super()._initialize(dim_in)
        if self.dtype == torch.float64:
            self.double()
        LOG["init"] = state(self)

    def pretrain_NMF(self, X, y, nmf_max_iter=100):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            super().pretrain_NMF(X, y, nmf_max_iter)
        self.W_nmf.data = self.W_nmf.data.to(self.dtype)
        LOG["nmf"] = self.W_nmf.detach().cpu().numpy().copy()

    def pretrain_encoder(self, *a, **k):
        LOG["phase"] = "pre"
        super().pretrain_encoder(*a, **k)
        LOG["phase"] = "main"
        LOG["pre"] = state(self)

    def forward(self, X, y, task_mask, pred_weight, intercept_mask=None, avg_intercept=False):
        out = super().forward(X.to(self.dtype), y.to(self.dtype), task_mask, pred_weight.to(self.dtype), intercept_mask,
                              avg_intercept)
        LOG["loss_" + LOG["phase"]].append((float(out[0].detach()), float(out[1].detach())))
        return out

    def transform(self, X, intercept_mask=None, avg_intercept=True, return_npy=True):
        if avg_intercept is False:  # fit's look at the training set after an epoch
            LOG["epochs"].append(state(self))
        if torch.is_tensor(X):
            X = X.to(self.dtype)
        elif self.dtype == torch.float64:
            X = torch.Tensor(X).double()
        return super().transform(X, intercept_mask, avg_intercept, return_npy)


class ListeningVanilla(Listening, VA.FullDCSFAModel):
    pass


class ListeningDirSpec(Listening, DS.FullDCSFAModel):
    pass


CLASSES = {"vanilla": ListeningVanilla, "dirspec": ListeningDirSpec}


def data(rng, cfg, N, grid):
    y = rng.rand(N, cfg["sup"]).astype(np.float32)
    X = 0.5 * rng.rand(N, cfg["D"]) + 0.5 * (y @ rng.rand(cfg["sup"], cfg["D"]))
    if grid:
        X = np.round(X * 256) / 256
    return X.astype(np.float32), y


def run(cfg, tr, va, pw, tm, dtype):
    """The reference's fit() with every listened value kept."""
    LOG.clear()
    LOG.update(idx=[], loss_pre=[], loss_main=[], epochs=[], phase="main")
    cls = CLASSES[cfg["cls"]]
    Listening.dtype = dtype
    torch.manual_seed(cfg["seed"])
    np.random.seed(cfg["seed"])  # sklearn's nndsvd initialisation draws from numpy's global generator
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        m = cls(num_nodes=cfg["nodes"], num_high_level_node_features=cfg["features"], n_components=cfg["K"],
                n_sup_networks=cfg["sup"], h=cfg["h"], save_folder=tmp, device="cpu", **cfg["model"])
        kw = dict(X_val=va[0], y_val=va[1]) if cfg["val"] else {}
        m.fit(tr[0], tr[1], y_pred_weights=pw, task_mask=tm, n_epochs=cfg["n_epochs"], n_pre_epochs=cfg["n_pre"],
              batch_size=cfg["B"], lr=1e-3, pretrain=True, **kw)
        assert os.path.exists(os.path.join(tmp, "dCSFA-NMF-last-epoch.pt"))
        if cfg["val"]:
            assert os.path.exists(os.path.join(tmp, "dCSFA-NMF-best-model.pt"))
    return m, dict(LOG)


# The first Linear's bias feeds BatchNorm, which subtracts the batch mean: its gradient is identically zero
# in exact arithmetic and rounding noise in floating point, which Adam normalises to steps of the order of lr
# whenever the noise exceeds eps = 1e-8.  The bias, and the running mean that carries it, are therefore
# determined only up to Adam's largest step, lr (1 - beta1) / sqrt(1 - beta2), per optimiser step taken: the
# reference's own fp32 run is hundreds of state bounds away from its float64 run in these two tensors, at
# every seed.  They are held to that step bound (on top of the state bound), every other tensor to the rule.
NOISE_KEYS = ("encoder.0.bias", "encoder.1.running_mean")
ADAM_MAX_STEP = 1e-3 * (1 - 0.9) / np.sqrt(1 - 0.999)


def check_conditioning(name, cfg, log32, log64):
    worst, where, noise = 0.0, None, 0.0
    per_epoch = -(-cfg["N"] // cfg["B"])
    for e, (a, b) in enumerate(zip([log32["pre"]] + log32["epochs"], [log64["pre"]] + log64["epochs"])):
        steps = per_epoch * (cfg["n_pre"] + e)
        for k in a:
            if k.endswith("num_batches_tracked"):
                assert int(a[k]) == int(b[k])
                continue
            want = b[k].astype(np.float64)
            bound = 2e-4 * np.abs(want) + 5e-6 * max(1.0, float(np.abs(want).max()))
            if k in NOISE_KEYS:
                noise = max(noise, float((np.abs(a[k].astype(np.float64) - want) / (bound + steps * ADAM_MAX_STEP)).max()))
                continue
            w = float((np.abs(a[k].astype(np.float64) - want) / bound).max())
            if w > worst:
                worst, where = w, k
    print("scenario %s: fp32 vs fp64 deviation = %.3f %% of the state bound (%s); bias / running mean %.3f %% of the "
          "Adam step bound" % (name, 100 * worst, where, 100 * noise))
    assert worst < (1.0 if name in LAST_ONLY else 0.25), (name, worst, where)
    assert noise < 1.0, (name, noise)
    return worst


def main():
    out = {}
    for name, cfg in SCENARIOS.items():
        rng = np.random.RandomState(cfg["seed"] + 100)
        tr = data(rng, cfg, cfg["N"], name == "d")
        va = data(rng, cfg, cfg["N"] // 2, name == "d")
        pw = (0.5 + rng.rand(cfg["N"], 1)).astype(np.float32) if cfg["masks"] else np.ones((cfg["N"], 1), dtype=np.float32)
        tm = (rng.rand(cfg["N"], cfg["sup"]) > 0.2).astype(np.float32) if cfg["masks"] else np.ones_like(tr[1])
        m32, log = run(cfg, tr, va, pw, tm, torch.float32)
        m64, log64 = run(cfg, tr, va, pw, tm, torch.float64)
        Listening.dtype = torch.float32  # m32 is looked at below
        assert all(np.array_equal(a, b) for a, b in zip(log["idx"], log64["idx"]))
        cond = check_conditioning(name, cfg, log, log64)
        l32, l64 = np.asarray(log["loss_main"]), np.asarray(log64["loss_main"])
        print("   loss fp32 vs fp64: max rel %.2e" % float(np.max(np.abs(l32 - l64) / np.abs(l64))))
        assert np.array_equal(log["pre"]["phi_list.0"], log["init"]["phi_list.0"])  # untouched by pretrain_encoder
        assert np.array_equal(log["pre"]["W_nmf"], log["nmf"])
        pre = name + "/"
        out[pre + "meta"] = np.asarray(json.dumps(cfg))
        out[pre + "conditioning"] = np.asarray(cond, dtype=np.float64)
        out[pre + "X"], out[pre + "y"], out[pre + "pw"], out[pre + "tm"] = tr[0], tr[1], pw, tm
        if cfg["val"]:
            out[pre + "X_val"], out[pre + "y_val"] = va
        out[pre + "nmf/W_nmf"] = log["nmf"]
        out[pre + "idx"] = np.stack(log["idx"])
        assert out[pre + "idx"].shape == (cfg["n_pre"] + cfg["n_epochs"], cfg["N"])
        out[pre + "loss_pre"] = np.asarray(log["loss_pre"], dtype=np.float64)
        out[pre + "loss"] = np.asarray(log["loss_main"], dtype=np.float64)
        states = [("init/", log["init"]), ("pre/", log["pre"])] + [("epoch%d/" % e, s) for e, s in enumerate(log["epochs"])]
        for tag, st in states:
            if name in LAST_ONLY and tag != "epoch%d/" % (cfg["n_epochs"] - 1):
                continue
            for k, v in st.items():
                out[pre + tag + k] = v
        out[pre + "hist/training"] = np.asarray(m32.training_hist, dtype=np.float64)
        out[pre + "hist/recon"] = np.asarray(m32.recon_hist, dtype=np.float64)
        out[pre + "hist/pred"] = np.asarray(m32.pred_hist, dtype=np.float64)
        out[pre + "hist/recon_f64"] = np.asarray(m64.recon_hist, dtype=np.float64)
        assert np.array_equal(out[pre + "hist/pred"], np.asarray(m64.pred_hist, dtype=np.float64))
        if cfg["val"]:
            out[pre + "hist/val_recon"] = np.asarray(m32.val_recon_hist, dtype=np.float64)
            out[pre + "hist/val_pred"] = np.asarray(m32.val_pred_hist, dtype=np.float64)
            out[pre + "fit/best_epoch"] = np.asarray(m32.best_epoch, dtype=np.int64)
            for k, v in state(m32).items():
                out[pre + "fit/final/" + k] = v
            want = log["epochs"][int(m32.best_epoch)]
            assert all(np.array_equal(want[k], v) for k, v in state(m32).items())  # the reload took the best epoch
            out[pre + "fit/GC"] = np.stack(m32.GC(threshold=False))
            m32.eval()
            Xr, yp, s = m32.transform(va[0])
            out[pre + "fit/X_recon"], out[pre + "fit/y_pred"], out[pre + "fit/s"] = Xr, yp, s
            out[pre + "hist/val_recon_f64"] = np.asarray(m64.val_recon_hist, dtype=np.float64)
            assert np.array_equal(out[pre + "hist/val_pred"], np.asarray(m64.val_pred_hist, dtype=np.float64))
            assert int(m64.best_epoch) == int(m32.best_epoch)
            Listening.dtype = torch.float64
            m64.eval()
            Xr, yp, s = m64.transform(va[0])
            Listening.dtype = torch.float32
            out[pre + "fit/X_recon_f64"], out[pre + "fit/y_pred_f64"], out[pre + "fit/s_f64"] = Xr, yp, s
            print("   whole fit: best epoch %d of %d" % (int(m32.best_epoch), cfg["n_epochs"]))
        else:
            out[pre + "GC"] = np.stack(m32.GC(threshold=False))
    for fname, keep in (("dcsfa_fit.npz", lambda k: not k.startswith("d/")), ("dcsfa_fit_d.npz", lambda k: k.startswith("d/"))):
        part = dict((k, v) for k, v in out.items() if keep(k))
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **part)
        print("wrote", path, len(part), "arrays,", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
