"""Shared by test_dcsfa_fit_host.py and test_gpu_dcsfa_fit.py: the fixture of tests/golden/make_dcsfa_fit_golden.py,
a scenario run through fit_dcsfa_baselines on either route, and the state bound.

The state bound is the project's DGCNN-fit bound, rtol 2e-4 and atol 5e-6 * max(1, |want|max).  Two tensors
cannot be held to it by any implementation: the first Linear's bias feeds BatchNorm, which subtracts the batch
mean, so its gradient is identically zero in exact arithmetic and rounding noise in floating point; Adam
normalises that noise to steps of the order of lr.  The bias, and the running mean that carries it, are
determined only up to Adam's largest step lr (1 - beta1) / sqrt(1 - beta2) per optimiser step taken (the
reference's own fp32 run is hundreds of state bounds from its float64 run there, at every seed); they get that
much on top of the state bound.  In training mode everything else BatchNorm produces is invariant to the bias.
In eval mode it is not: the running mean is an average of past biases, the pre-activation carries the current
one, and what fit() computes in eval mode (recon_hist, the validation histories, transform's outputs) inherits
the noise.  The fixture records the reference's own fp32-to-float64 difference there; it is one draw of a
zero-mean noise, which falls below a quarter of its scale one time in five, and two fp32 runs each carry their
own draw, so these quantities are allowed ten times it on top of the state bound.  The binary-vector AUCs move by
1 / (2 n) when one of a class's n predictions crosses the 0.6 cut: they are allowed one such crossing per
network."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOISE_KEYS = ("encoder.0.bias", "encoder.1.running_mean")
LR = 1e-3
ADAM_MAX_STEP = LR * (1 - 0.9) / np.sqrt(1 - 0.999)

_cache = {}


def fixture(name):
    """{key: array} of scenario `name`, loaded once."""
    if name not in _cache:
        path = os.path.join(GOLDEN, "dcsfa_fit_d.npz" if name == "d" else "dcsfa_fit.npz")
        with np.load(path) as z:
            _cache[name] = dict((k[len(name) + 1:], z[k]) for k in z.files if k.startswith(name + "/"))
        _cache[name]["cfg"] = json.loads(str(_cache[name]["meta"]))
    return _cache[name]


def sub(fx, prefix):
    return dict((k[len(prefix):], v) for k, v in fx.items() if isinstance(k, str) and k.startswith(prefix))


def steps_per_epoch(cfg):
    return -(-cfg["N"] // cfg["B"])


def assert_state(got, want, steps=0, what=""):
    """got / want: {key: array}; steps: optimiser steps taken so far (the noise keys' allowance)."""
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k, w in want.items():
        g = np.asarray(got[k])
        if k.endswith("num_batches_tracked"):
            assert int(g) == int(w), (what, k)
            continue
        w64 = np.asarray(w, dtype=np.float64)
        bound = 2e-4 * np.abs(w64) + 5e-6 * max(1.0, float(np.abs(w64).max()))
        if k in NOISE_KEYS:
            bound = bound + steps * ADAM_MAX_STEP
        err = np.abs(g.astype(np.float64) - w64)
        assert g.shape == w64.shape and np.all(err <= bound), "%s %s: %.3g of the bound" % (what, k, float((err / bound).max()))


def assert_close(got, want, what="", want64=None):
    """The state bound on one array (histories, GC, transform outputs); want64: the reference's float64 run
    of an eval-mode quantity (see the module docstring)."""
    w = np.asarray(want, dtype=np.float64)
    g = np.asarray(got, dtype=np.float64)
    bound = 2e-4 * np.abs(w) + 5e-6 * max(1.0, float(np.abs(w).max()))
    if want64 is not None:
        bound = bound + 10.0 * float(np.abs(w - np.asarray(want64, dtype=np.float64)).max())
    assert g.shape == w.shape and np.all(np.abs(g - w) <= bound), "%s: %.3g of the bound" % (
        what, float((np.abs(g - w) / bound).max()))


def assert_aucs(got, y, tm, want, what=""):
    """Per-epoch AUC lists against the fixture's, one crossing of the cut allowed per network (module docstring)."""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, what
    for j in range(w.shape[1]):
        lab = np.float32(y)[np.asarray(tm)[:, j].astype(np.int64) == 1, j] >= 0.6
        step = 0.5 / min(int(lab.sum()), int((~lab).sum()))
        assert np.all(np.abs(g[:, j] - w[:, j]) <= step + 1e-9), "%s network %d: %s vs %s" % (what, j, g[:, j], w[:, j])


def state(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


def build(cfg, device, folder, **over):
    import redcliff_amd
    cls = redcliff_amd.FullDCSFAModel_GCv2 if cfg["cls"] == "vanilla" else redcliff_amd.FullDCSFAModel
    kw = dict(cfg["model"])
    kw.update(over)
    return cls(num_nodes=cfg["nodes"], num_high_level_node_features=cfg["features"], n_components=cfg["K"],
               n_sup_networks=cfg["sup"], h=cfg["h"], save_folder=str(folder), device=device, **kw)


class FixedNMF:
    """Stands in for a model's pretrain_NMF (picklable: fit saves the whole module)."""

    def __init__(self, model, W):
        self.model, self.W = model, np.asarray(W)

    def __call__(self, X, y, nmf_max_iter=100):
        prm = self.model.W_nmf
        with torch.no_grad():
            prm.data.copy_(torch.as_tensor(self.W).to(prm.device, prm.dtype))


def fixed_nmf(model, W):
    """pretrain_NMF replaced by the fixture's recorded result: no test of the fit depends on sklearn."""
    model.pretrain_NMF = FixedNMF(model, W)


def run_scenario(name, device, folder, val=None, dtype=torch.float32):
    """The scenario's fit through fit_dcsfa_baselines on the route REDCLIFF_DCSFA_PATH names.  Returns
    (model, {"pre": state, "epochs": [state, ..]})."""
    import redcliff_amd
    fx = fixture(name)
    cfg = fx["cfg"]
    m = build(cfg, device, folder)
    m.fit_dtype = dtype
    fixed_nmf(m, fx["nmf/W_nmf"])
    log = {"epochs": []}

    def cb(i, phase, epoch, model):
        if phase == "pretrain":
            log["pre"] = state(model)
        elif phase == "epoch":
            log["epochs"].append(state(model))
    use_val = cfg["val"] if val is None else val
    kw = dict(X_vals=[fx["X_val"]], y_vals=[fx["y_val"]]) if use_val else {}
    torch.manual_seed(cfg["seed"])
    redcliff_amd.fit_dcsfa_baselines([m], [fx["X"]], [fx["y"]], y_pred_weights=[fx["pw"]], task_masks=[fx["tm"]],
                                     n_epochs=cfg["n_epochs"], n_pre_epochs=cfg["n_pre"], batch_size=cfg["B"], lr=LR,
                                     pretrain=True, callback=cb, **kw)
    return m, log


def check_against_fixture(name, m, log):
    """Losses (1e-4 relative), the state after pretrain_encoder and every stored epoch, the histories."""
    fx = fixture(name)
    cfg = fx["cfg"]
    spe = steps_per_epoch(cfg)
    np.testing.assert_allclose(m.pretrain_step_losses, fx["loss_pre"], rtol=1e-4, atol=0)
    np.testing.assert_allclose(m.step_losses, fx["loss"], rtol=1e-4, atol=0)
    if sub(fx, "pre/"):
        assert_state(log["pre"], sub(fx, "pre/"), spe * cfg["n_pre"], name + " pre")
    for e in range(cfg["n_epochs"]):
        want = sub(fx, "epoch%d/" % e)
        if want:
            assert_state(log["epochs"][e], want, spe * (cfg["n_pre"] + e + 1), "%s epoch %d" % (name, e))
    assert_close(m.training_hist, fx["hist/training"], name + " training_hist")
    assert_close(m.recon_hist, fx["hist/recon"], name + " recon_hist", fx["hist/recon_f64"])
    assert_aucs(m.pred_hist, fx["y"], fx["tm"], fx["hist/pred"], name + " pred_hist")


def check_whole_fit(name, m, folder):
    """The end of a fit with validation: best epoch, the reloaded state, GC, transform, the two files."""
    fx = fixture(name)
    cfg = fx["cfg"]
    assert int(m.best_epoch) == int(fx["fit/best_epoch"])
    assert_close(m.val_recon_hist, fx["hist/val_recon"], name + " val_recon_hist", fx["hist/val_recon_f64"])
    assert_aucs(m.val_pred_hist, fx["y_val"], np.ones_like(fx["y_val"]), fx["hist/val_pred"], name + " val_pred_hist")
    total = steps_per_epoch(cfg) * (cfg["n_pre"] + cfg["n_epochs"])
    assert_state(state(m), sub(fx, "fit/final/"), total, name + " final")
    assert_close(np.stack(m.GC(threshold=False)), fx["fit/GC"], name + " GC")
    m.eval()
    Xr, yp, s = m.transform(fx["X_val"])
    assert_close(Xr, fx["fit/X_recon"], name + " X_recon", fx["fit/X_recon_f64"])
    assert_close(yp, fx["fit/y_pred"], name + " y_pred", fx["fit/y_pred_f64"])
    assert_close(s, fx["fit/s"], name + " s", fx["fit/s_f64"])
    best = torch.load(os.path.join(str(folder), "dCSFA-NMF-best-model.pt"), map_location="cpu", weights_only=False)
    last = torch.load(os.path.join(str(folder), "dCSFA-NMF-last-epoch.pt"), map_location="cpu", weights_only=False)
    assert isinstance(best, dict) and isinstance(last, torch.nn.Module)
    assert_state(dict((k, v.numpy()) for k, v in best.items()), sub(fx, "fit/final/"), total, name + " best file")
    assert_state(state(last), sub(fx, "epoch%d/" % (cfg["n_epochs"] - 1)), total, name + " last-epoch file")
    # compact clones, not views of a pack's storage
    for t in list(best.values()) + list(last.state_dict().values()):
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size()
