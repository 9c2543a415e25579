"""cMLP_FM, the cMLP forecasting baseline the paper compares REDCLIFF-S against
(models/cmlp_fm.py:58-475; built for model type "cMLP", general_utils/model_utils.py:421-442, and
fitted with one Adam, :789-809).

One ``cMLP`` (K = 1), no factor-score embedder; the loss is FORECAST_COEFF * sum_i MSE(pred[:, :, i],
target[:, :, i]) + ADJ_L1_REG_COEFF * sum ||GC(ignore_lag=True)||_1 (:156-178; the DAGness terms
are commented out in the reference and reported as None / 0).

Two routes:

* fused -- ``redcliff_fm_run`` (csrc/rc_fm.hip): the loss separates over the p channel networks, so
  one workgroup per (network, replica) keeps the network's weights and Adam moments in LDS and runs
  every batch of an epoch in ONE launch.  Taken when ``redcliff_fm_supported`` accepts the shape and
  the model has one hidden layer, no wavelets, num_sims == 1, output_length == 1,
  input_length == gen_lag and its parameters on the GPU.  The parameters and the optimizer's
  exp_avg / exp_avg_sq / step are views of packed buffers (kernels.factor_layout at K = 1).
* generic -- the reference's tensor operations restated with torch autograd over our ``cMLP`` module
  (redcliff_amd.autograd); serves every other configuration.  ``REDCLIFF_FM_PATH=generic`` forces it.

``fit_baselines`` fits many same-shape models (e.g. the 15 fold / SNR fits of the D4IC baseline
grid, train/CMLP_d4IC_BLgs1.py) with one launch per epoch; ``cMLP_FM.fit`` is that loop with a list
of one.  The training loader is uploaded once and replayed in order (the reference's loaders do not
shuffle, data/synthetic_datasets.py:272-276).
"""
import ctypes
import os
import pickle as pkl

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import kernels
from . import metrics as M
from . import packs
from .cmlp import cMLP
from .fit_loop import standalone_copy

LDS_MAX_FLOATS = 40960  # RC_LDS_MAX_FLOATS
FM_BC = 64              # windows per pass (csrc/rc_fm.h)
MAX_REPLICAS = 256
FM_FLAGS_TRAIN = nat.LOSS_FORECAST | nat.LOSS_ADJ | nat.STEP_B
FM_FLAGS_VALUES = nat.LOSS_FORECAST | nat.LOSS_ADJ | nat.VALUES


def fm_path():
    """'fused' (default) or 'generic', from REDCLIFF_FM_PATH."""
    return packs.route_from_env("REDCLIFF_FM_PATH")


def fm_lds_floats(p, L, h):
    """The workgroup's LDS footprint in floats (rc_fm_lds_floats, csrc/rc_fm.h)."""
    Q = p * L
    Qp, hp = Q | 1, h | 1
    return 3 * (h * Qp + 2 * h + 1) + h * Qp + FM_BC * (Qp + hp + 2) + Q + p + 8


def fm_shape_supported(p, L, h, Bmax=1, T=None, R=1, K=1):
    """The limits of redcliff_fm_run, restated (tests compare it with redcliff_fm_supported)."""
    T = L + 1 if T is None else T
    if min(p, L, h, Bmax, T, R, K) < 1:
        return False
    return (K == 1 and p <= 64 and h <= 128 and Bmax <= 512 and T >= L + 1 and R <= MAX_REPLICAS
            and fm_lds_floats(p, L, h) <= LDS_MAX_FLOATS)


def fm_dims(p, L, h, Bmax=1, T=None, R=1, K=1):
    return nat.Dims(R=R, Bmax=Bmax, T=L + 1 if T is None else T, p=p, L=L, K=K, h=h, F=L, n=1, H=1, M1=1, nsup=0,
                    use_sigmoid=0, sigmoid_ecc=0.0)


def fm_supported(p, L, h, Bmax=1, T=None, R=1, K=1):
    """redcliff_fm_supported: the footprint in floats, 0 outside the limits."""
    d = fm_dims(p, L, h, Bmax, T, R, K)
    return int(nat.lib().redcliff_fm_supported(ctypes.byref(d)))


def fm_run(d, flags, B, tB, row0, N, X, x_pstride, fac, fac_m, fac_v, fac_stride, hyper, sse, pen, G=None, G0=None,
           replicas=None, stream=None):
    """redcliff_fm_run on device tensors (None = a null pointer); returns its code."""
    p_ = nat.ptr
    a = nat.FMArgs()
    a.d = d
    a.flags, a.B, a.tB, a.row0, a.N = int(flags), int(B), int(tB), int(row0), int(N)
    a.X, a.x_pstride = p_(X), int(x_pstride)
    a.fac, a.fac_m, a.fac_v, a.fac_stride = p_(fac), p_(fac_m), p_(fac_v), int(fac_stride)
    a.hyper, a.sse, a.pen, a.G, a.G0 = p_(hyper), p_(sse), p_(pen), p_(G), p_(G0)
    keep = nat.replica_list(a, replicas)  # a local, so alive until the call has returned
    return nat.lib().redcliff_fm_run(ctypes.byref(a), nat.stream_or_current(stream))


class DAGNessLoss(nn.Module):
    """general_utils/metrics.py:433-443 (held by the model, unused since the DAGness terms were removed)."""

    def forward(self, W0):
        if W0.dim() == 3 and W0.size(2) == 1:
            W0 = W0[:, :, 0]
        assert W0.dim() == 2 and W0.size(0) == W0.size(1)
        return (torch.trace(torch.exp(W0 * W0)) - W0.size(0)) ** 2.


# --------------------------------------------------------------------------------------------------
class FMPack(packs.AdamPack):
    """R same-shape cMLP_FM models on the fused route (packs.AdamPack; the rows `par` are also named `fac`):
    parameters by kernels.factor_layout at K = 1, the replica's hyper-parameters beside Adam are the two
    loss coefficients, and only the reference's one plain Adam can be bound."""

    def __init__(self, models):
        m0 = models[0]
        self.p, self.L, self.h = m0.num_series, m0.gen_lag, m0.gen_hidden[0]
        for m in models:
            if (m.num_series, m.gen_lag, list(m.gen_hidden)) != (self.p, self.L, [self.h]):
                raise ValueError("an FMPack holds models of one shape")
        if not fm_supported(self.p, self.L, self.h, R=len(models)):
            nat.check(-2, "fm_supported")
        kernels.require_gpu(next(m0.parameters()), "cMLP_FM (fused)")
        self.n = kernels.factor_layout(1, self.p, self.h, self.L)["total"]
        self.allocate(models, self.n, next(m0.parameters()).device)
        self.fac = self.par
        for r, mod in enumerate(self.models):
            self.adopt_views(r, kernels.factor_views(self.fac[r], list(mod.factors), self.p, self.h, self.L))

    def check_optimizer(self, r, opt):
        packs.require_plain_adam(opt, self.params[r], "cMLP_FM", "model_utils.py:789-809")

    def replica_terms(self, r):
        m = self.models[r]
        return {"c_forecast": float(m.FORECAST_COEFF), "c_adj": float(m.ADJ_L1_REG_COEFF)}

    def run(self, flags, X, x_pstride, T, B, N, row0=0, active=None, G=None, G0=None):
        """One redcliff_fm_run over windows [row0, row0 + N) of X in batches of B for the replicas
        `active` (None: all).  Returns (sse, pen) device tensors [stepped][nsteps][p] (pen None
        without VALUES)."""
        reps = self.reps(active)
        nsteps = -(-int(N) // int(B))
        sse = torch.empty(len(reps), nsteps, self.p, device=self.device, dtype=torch.float32)
        pen = torch.empty_like(sse) if flags & nat.VALUES else None
        if not reps or N == 0:
            return sse, pen
        stepping = bool(flags & nat.STEP_B)
        if stepping:
            self.require_optimizers(reps)
        t_base = self.opt[reps[0]]["t"] if self.opt[reps[0]] else 0
        d = fm_dims(self.p, self.L, self.h, Bmax=int(B), T=int(T), R=self.R)
        rc = fm_run(d, flags, B, t_base + 1, row0, N, X, x_pstride, self.fac, self.m, self.v, self.n,
                    self.hyper(t_base, reps), sse, pen, G, G0, None if active is None else reps)
        nat.check(rc, "fm_run")
        if stepping:
            self.advance(reps, nsteps)
        return sse, pen


def _upload(loader, device, cache):
    """An iterable of (X, _) batches -> {"X": (N, T, p) device tensor, "sizes": [...]}, uploaded once."""
    key = id(loader)
    hit = cache.get(key)
    if hit is not None and hit["loader"] is loader:
        return hit
    xs = [X.to(torch.float32) for X, _ in loader]
    sizes = [int(x.shape[0]) for x in xs]
    ds = {"X": torch.cat(xs, 0).to(device).contiguous(), "sizes": sizes, "loader": loader}
    cache[key] = ds
    return ds


def _segments(sizes):
    """[(row0, N, B)] launches that replay batches of `sizes`: one when they are equal-sized except
    the last, else one per batch."""
    if not sizes:
        return []
    B = sizes[0]
    if all(s == B for s in sizes[:-1]) and sizes[-1] <= B:
        return [(0, sum(sizes), B)]
    rows = np.cumsum([0] + sizes[:-1])
    return [(int(r), int(s), int(s)) for r, s in zip(rows, sizes)]


def _val_terms(model, sse, pen, sizes, normalized):
    """The validate_training tuple (:419-475) from per-batch sums sse / pen ([batches][p])."""
    fc, ac = float(model.FORECAST_COEFF), float(model.ADJ_L1_REG_COEFF)
    af = aa = acmb = 0.
    for i, B in enumerate(sizes):
        f = fc * float(np.sum(np.asarray(sse[i], dtype=np.float64) / B))
        a = ac * float(np.sum(np.asarray(pen[i], dtype=np.float64)))
        acmb += f + a
        if normalized:
            if fc > 0.:
                f /= fc
            if ac > 0.:
                a /= ac
        af += f
        aa += a
    n = len(sizes)
    return af / n, aa / n, 0., 0., 0., acmb / n


# --------------------------------------------------------------------------------------------------
class cMLP_FM(packs.PackSlot, nn.Module):
    _slot_key, _pack_class, _unpickled = "_fm_slot", FMPack, ("_fm_data",)

    def __init__(self, num_chans, gen_lag, gen_hidden, embed_hidden_sizes, num_in_timesteps, num_out_timesteps,
                 coeff_dict, num_sims=1, wavelet_level=None, save_path=None):
        super().__init__()
        self.num_chans = num_chans
        self.num_series = num_chans * (wavelet_level + 1) if wavelet_level is not None else num_chans
        self.gen_lag = gen_lag
        self.gen_hidden = gen_hidden
        self.num_gen_hiddens = len(gen_hidden)
        self.embed_hidden_sizes = embed_hidden_sizes
        self.num_in_timesteps = num_in_timesteps
        self.num_out_timesteps = num_out_timesteps
        self.num_factors_nK = 1
        self.coeff_dict = coeff_dict
        self.FORECAST_COEFF = coeff_dict["FORECAST_COEFF"]
        self.FACTOR_SCORE_COEFF = 0.
        self.ADJ_L1_REG_COEFF = coeff_dict["ADJ_L1_REG_COEFF"]
        self.DAGNESS_REG_COEFF = coeff_dict["DAGNESS_REG_COEFF"]
        self.DAGNESS_LAG_COEFF = coeff_dict["DAGNESS_LAG_COEFF"]
        self.DAGNESS_NODE_COEFF = coeff_dict["DAGNESS_NODE_COEFF"]
        self.num_sims = num_sims
        self.wavelet_level = wavelet_level
        self.supervised_loss_fn = nn.MSELoss(reduction='mean')
        self.dagness_loss_fn = DAGNessLoss()
        self.factor_score_embedder = None
        self.factors = nn.ModuleList([cMLP(num_chans, gen_lag, gen_hidden, wavelet_level=wavelet_level,
                                           save_path=save_path) for _ in range(self.num_factors_nK)])
        self.gen_model = nn.ModuleList([self.factor_score_embedder, self.factors])

    # ------------------------------------------------------------------ route
    def _device(self):
        return next(self.parameters()).device

    def fused_eligible(self, input_length=None, output_length=None, Bmax=1, T=None):
        """The fused route serves this model (and, when given, these lengths / batch shape)."""
        if fm_path() != "fused":
            return False
        if self.num_gen_hiddens != 1 or self.wavelet_level is not None or self.num_sims != 1:
            return False
        if output_length is not None and output_length != 1:
            return False
        if input_length is not None and input_length != self.gen_lag:
            return False
        if not next(self.parameters()).is_cuda:
            return False
        p, L, h = self.num_series, self.gen_lag, self.gen_hidden[0]
        if not fm_shape_supported(p, L, h, Bmax=Bmax, T=T):
            return False
        return fm_supported(p, L, h, Bmax=Bmax, T=T) > 0

    # ------------------------------------------------------------------ reference API
    def forward(self, X):
        """X (batch, T, p) -> (x_simulations, factor_preds_over_sim, factor_weighting_preds) (:96-142)."""
        in_x = X.to(self._device())
        inputs = [in_x]
        x_simulations, factor_preds_over_sim, factor_weighting_preds = [], [], []
        for s in range(self.num_sims):
            if s > 0:
                if x_simulations[-1].size() == inputs[-1].size():
                    inputs.append(x_simulations[-1])
                else:
                    inputs.append(torch.cat([inputs[-1][:, x_simulations[-1].size()[1]:, :], x_simulations[-1]], dim=1))
            factor_preds = [f(inputs[s]) for f in self.factors]
            combined_pred = factor_preds[0]
            for pred in factor_preds[1:]:
                combined_pred = combined_pred + pred
            factor_preds_over_sim.append(factor_preds)
            factor_weighting_preds.append(None)
            x_simulations.append(combined_pred)
        return torch.cat(x_simulations, dim=1), factor_preds_over_sim, factor_weighting_preds

    def GC(self, threshold=True, ignore_lag=True, combine_wavelet_representations=False, rank_wavelets=False):
        return [f.GC(threshold=threshold, ignore_lag=ignore_lag,
                     combine_wavelet_representations=combine_wavelet_representations, rank_wavelets=rank_wavelets)
                for f in self.factors]

    def compute_loss(self, preds, targets, node_dag_scale=0.1):
        gc = self.GC(threshold=False, ignore_lag=True, combine_wavelet_representations=False, rank_wavelets=False)
        forecasting_loss = self.FORECAST_COEFF * sum([self.supervised_loss_fn(preds[:, :, i], targets[:, :, i])
                                                      for i in range(self.num_series)])
        adj_l1_penalty = self.ADJ_L1_REG_COEFF * sum([torch.norm(A, 1) for A in gc])
        combo_loss = forecasting_loss + adj_l1_penalty
        return combo_loss, [forecasting_loss, adj_l1_penalty, None, None, None]

    def batch_update(self, batch_num, X, gen_optim, input_length, output_length):
        X = X.to(self._device(), torch.float32)
        if self.fused_eligible(input_length, output_length, Bmax=int(X.shape[0]), T=int(X.shape[1])):
            pack, r = self._slot()
            pack.bind_optimizer(r, gen_optim)
            X = X.contiguous()
            pack.run(FM_FLAGS_TRAIN, X, 0, X.shape[1], X.shape[0], X.shape[0], active=[r])
            return
        for f in self.factors:
            f.train()
        gen_optim.zero_grad()
        x_sims, _, _ = self.forward(X[:, :input_length, :])
        combined_loss, _ = self.compute_loss(x_sims, X[:, input_length:input_length + (self.num_sims * output_length), :])
        combined_loss.backward()
        gen_optim.step()

    def validate_training(self, X_val, input_length, output_length, num_series, report_normalized_loss_components=False):
        ds = _upload(X_val, self._device(), self.__dict__.setdefault("_fm_data", {}))
        sizes = ds["sizes"]
        T = int(ds["X"].shape[1])
        if self.fused_eligible(input_length, output_length, Bmax=max(sizes), T=T):
            pack, r = self._slot()
            sse, pen = [], []
            for row0, N, B in _segments(sizes):
                s, q = pack.run(FM_FLAGS_VALUES, ds["X"], 0, T, B, N, row0=row0, active=[r])
                sse.append(s[0])
                pen.append(q[0])
            sse, pen = M.fetch([torch.cat(sse, 0).double(), torch.cat(pen, 0).double()])
            return _val_terms(self, sse, pen, sizes, report_normalized_loss_components)
        return self._validate_generic(ds, input_length, output_length, report_normalized_loss_components)

    def _validate_generic(self, ds, input_length, output_length, normalized):
        af = aa = acmb = 0.
        for f in self.factors:
            f.eval()
        row = 0
        with torch.no_grad():
            for B in ds["sizes"]:
                X = ds["X"][row:row + B]
                row += B
                x_sims, _, _ = self.forward(X[:, :input_length, :])
                combined, (fl, al, _, _, _) = self.compute_loss(
                    x_sims, X[:, input_length:input_length + (self.num_sims * output_length), :])
                if normalized:
                    if self.FORECAST_COEFF > 0.:
                        fl = fl / self.FORECAST_COEFF
                    if self.ADJ_L1_REG_COEFF > 0.:
                        al = al / self.ADJ_L1_REG_COEFF
                af += float(fl)
                aa += float(al)
                acmb += float(combined)
        n = len(ds["sizes"])
        return af / n, aa / n, 0., 0., 0., acmb / n

    def save_checkpoint(self, save_dir, it, best_model, avg_forecasting_loss, avg_adj_penalty, avg_dagness_reg_loss,
                        avg_dagness_lag_loss, avg_dagness_node_loss, avg_combo_loss, best_loss, best_it,
                        f1score_histories, roc_auc_histories, gc_factor_l1_loss_histories, GC, X_train=None, X_val=None,
                        input_length=None, output_length=None, num_sim_steps=None):
        """The two files of :204-225 (the plots of :227-257 are not drawn, as in our REDCLIFF-S fit)."""
        os.makedirs(save_dir, exist_ok=True)
        torch.save(standalone_copy(best_model) if isinstance(best_model, nn.Module) else best_model,
                   os.path.join(save_dir, "final_best_model.bin"))
        with open(os.path.join(save_dir, "training_meta_data_and_hyper_parameters.pkl"), "wb") as outfile:
            pkl.dump({
                "epoch": it,
                "avg_forecasting_loss": avg_forecasting_loss,
                "avg_adj_penalty": avg_adj_penalty,
                "avg_dagness_reg_loss": avg_dagness_reg_loss,
                "avg_dagness_lag_loss": avg_dagness_lag_loss,
                "avg_dagness_node_loss": avg_dagness_node_loss,
                "avg_combo_loss": avg_combo_loss,
                "best_loss": best_loss,
                "best_it": best_it,
                "f1score_histories": f1score_histories,
                "roc_auc_histories": roc_auc_histories,
                "gc_factor_l1_loss_histories": gc_factor_l1_loss_histories,
            }, outfile)
        if X_train is not None:
            raise NotImplementedError

    def fit(self, save_dir, X_train, gen_optim, input_length, output_length, num_sim_steps, max_iter, lookback=5,
            check_every=50, verbose=1, GC=None, X_val=None):
        return fit_baselines([self], [gen_optim], [save_dir], [X_train], [X_val], [GC], input_length, output_length,
                             max_iter, lookback=lookback, check_every=check_every, verbose=verbose)[0]


# --------------------------------------------------------------------------------------------------
class _Fit:
    """One model's bookkeeping of fit() (:264-416)."""

    def __init__(self, model, opt, save_dir, GC):
        self.model, self.opt, self.save_dir, self.GC = model, opt, save_dir, GC
        self.h = {k: [] for k in ("avg_forecasting_loss", "avg_adj_penalty", "avg_dagness_reg_loss",
                                  "avg_dagness_lag_loss", "avg_dagness_node_loss", "avg_combo_loss")}
        self.f1 = {0.0: [[] for _ in range(len(GC))]}
        self.roc = {0.0: [[] for _ in range(len(GC))]}
        self.l1 = [[] for _ in range(len(GC))]
        self.best_it, self.best_loss, self.best = None, np.inf, None
        self.done = False

    def record(self, it, f1, roc, l1, val, snapshot, lookback, check_every, verbose):
        """One epoch's tracking values -> histories, the stop rule (:349-357), the checkpoint (:359-400).
        Returns True when the fit stops."""
        for j in range(len(self.GC)):
            self.f1[0.0][j].append(float(f1[j]))
            self.roc[0.0][j].append(float(roc[j]))
        l1 = np.float32(l1)  # the reference's torch.norm(gc_est / max, 1) is a float32 tensor
        self.l1[0].append(np.asarray(l1))
        for k, v in zip(("avg_forecasting_loss", "avg_adj_penalty", "avg_dagness_reg_loss", "avg_dagness_lag_loss",
                         "avg_dagness_node_loss", "avg_combo_loss"), val):
            self.h[k].append(v)
        crit = float(l1 + np.float32(val[0]))  # float32 tensor + python float
        if crit < self.best_loss:
            self.best_loss, self.best_it, self.best = crit, it, snapshot()
        elif (it - self.best_it) == lookback * check_every:
            if verbose:
                print("Stopping early")
            self.done = True
            return True
        if it % check_every == 0:
            if verbose > 0:
                print(("-" * 10 + "Iter = %d" + "-" * 10) % (it + 1))
                print("Validation Loss = %f" % val[5])
            self.checkpoint(it)
        return False

    def best_module(self):
        m = standalone_copy(self.model)
        if torch.is_tensor(self.best):  # a snapshot of the packed parameters
            p, h, L = m.num_series, m.gen_hidden[0], m.gen_lag
            with torch.no_grad():
                for prm, view in kernels.factor_views(self.best, list(m.factors), p, h, L):
                    prm.copy_(view)
        elif self.best is not None:
            m.load_state_dict(self.best)
        return m

    def checkpoint(self, it):
        h = self.h
        self.model.save_checkpoint(self.save_dir, it, self.best_module(), h["avg_forecasting_loss"], h["avg_adj_penalty"],
                                   h["avg_dagness_reg_loss"], h["avg_dagness_lag_loss"], h["avg_dagness_node_loss"],
                                   h["avg_combo_loss"], self.best_loss, self.best_it, self.f1, self.roc, self.l1, self.GC)

    def history(self):
        out = dict(self.h)
        out.update(f1score_histories=self.f1, roc_auc_histories=self.roc, gc_factor_l1_loss_histories=self.l1,
                   best_loss=self.best_loss, best_it=self.best_it)
        return out


def _track_values(G, G0, GCs, gcs_cache, rows):
    """Device tracking values of the estimates G[rows] ((n, p, p, L)) against each row's true graphs:
    (vals (n, len(GC), 6 + p), l1 (n, 1)) device tensors (metrics.gc_progress_values_grouped: f1 at
    threshold 0 and ROC-AUC of the lag-summed, max-normalised estimate; gc_track_values: the L1 of the
    max-normalised lagged estimate)."""
    key = tuple(rows)
    if key not in gcs_cache:
        gcs_cache[key] = [GCs[r] for r in rows]
    n, p, _, L = G.shape
    est = G.view(n, 1, p, p, L)
    nG = len(gcs_cache[key][0])  # the one estimate is scored against every true graph (:304-309)
    vals = M.gc_progress_values_grouped(gcs_cache[key], est.expand(n, nG, p, p, L).contiguous(), 1, host=False)
    l1, _ = M.gc_track_values(est, G0.view(n, 1, p, p, 1), host=False)
    return vals, l1


def fit_baselines(models, optimizers, save_dirs, X_trains, X_vals, GCs, input_length, output_length, max_iter,
                  lookback=5, check_every=50, verbose=0):
    """cMLP_FM.fit (:264-416) for a list of same-shape models, each with its own data, true graphs,
    optimizer and save_dir.  On the fused route an epoch is one redcliff_fm_run over the still
    active models for training and one for validation; a model that stops early leaves the active
    list.  Returns the models' final validation combo losses; every model's histories are left in
    ``model.fit_history``."""
    R = len(models)
    if not (len(optimizers) == len(save_dirs) == len(X_trains) == len(X_vals) == len(GCs) == R) or R == 0:
        raise ValueError("fit_baselines: one optimizer, save_dir, loader pair and graph list per model")
    dev = models[0]._device()
    caches = [m.__dict__.setdefault("_fm_data", {}) for m in models]
    tr = [_upload(X_trains[i], dev, caches[i]) for i in range(R)]
    va = [_upload(X_vals[i], dev, caches[i]) for i in range(R)]
    same = all(t["sizes"] == tr[0]["sizes"] and t["X"].shape == tr[0]["X"].shape for t in tr) and \
        all(v["sizes"] == va[0]["sizes"] and v["X"].shape == va[0]["X"].shape for v in va) and \
        all((m.num_series, m.gen_lag, list(m.gen_hidden)) == (models[0].num_series, models[0].gen_lag,
                                                               list(models[0].gen_hidden)) for m in models)
    if R > 1 and not same:  # nothing to share: fit one after the other
        return [fit_baselines([models[i]], [optimizers[i]], [save_dirs[i]], [X_trains[i]], [X_vals[i]], [GCs[i]],
                              input_length, output_length, max_iter, lookback, check_every, verbose)[0]
                for i in range(R)]
    Ttr, Tva = int(tr[0]["X"].shape[1]), int(va[0]["X"].shape[1])
    fused = R <= MAX_REPLICAS and all(
        m.fused_eligible(input_length, output_length, Bmax=max(tr[0]["sizes"] + va[0]["sizes"]), T=min(Ttr, Tva))
        for m in models)
    fits = [_Fit(models[i], optimizers[i], save_dirs[i], GCs[i]) for i in range(R)]
    gcs_cache = {}
    if fused:
        pack, rows, _ = packs.acquire(models, optimizers, FMPack)
        p, L = pack.p, pack.L
        Xtr, xps_tr = packs.stack_upload([t["X"] for t in tr], dev)
        Xva, xps_va = packs.stack_upload([v["X"] for v in va], dev)
        G =torch.zeros(pack.R, p, p, L, device=dev, dtype=torch.float32)
        G0 = torch.zeros(pack.R, p, p, device=dev, dtype=torch.float32)
        seg_tr, seg_va = _segments(tr[0]["sizes"]), _segments(va[0]["sizes"])

        def validate(active):
            sse, pen = [], []
            for row0, N, B in seg_va:
                s, q = pack.run(FM_FLAGS_VALUES, Xva, xps_va, Tva, B, N, row0=row0, active=active)
                sse.append(s)
                pen.append(q)
            return torch.cat(sse, 1), torch.cat(pen, 1)

    for it in range(max_iter):
        live = [i for i in range(R) if not fits[i].done]
        if not live:
            break
        if verbose and it % 5 == 0:
            print("cMLP_FM.fit: now on epoch it == ", it, flush=True)
        if fused:
            active = [rows[i] for i in live]
            for si, (row0, N, B) in enumerate(seg_tr):
                last = si == len(seg_tr) - 1
                pack.run(FM_FLAGS_TRAIN, Xtr, xps_tr, Ttr, B, N, row0=row0, active=active, G=G if last else None,
                         G0=G0 if last else None)
            idx = torch.as_tensor(active, device=dev)
            vals, l1 = _track_values(G.index_select(0, idx), G0.index_select(0, idx), GCs, gcs_cache, live)
            sse, pen = validate(active)
            vals, l1, sse, pen = M.fetch([vals, l1, sse.double(), pen.double()])  # the epoch's one fetch
            for a, i in enumerate(live):
                val = _val_terms(models[i], sse[a], pen[a], va[0]["sizes"], False)
                r = rows[i]
                fits[i].record(it, vals[a, :, 0], vals[a, :, 1], l1[a, 0], val, lambda r=r: pack.fac[r].clone(),
                               lookback, check_every, verbose)
        else:
            for i in live:
                m = models[i]
                row = 0
                for bn, B in enumerate(tr[i]["sizes"]):
                    m.batch_update(bn, tr[i]["X"][row:row + B], optimizers[i], input_length, output_length)
                    row += B
                Gm, G0m = kernels.cmlp_gc_norms(list(m.factors))
                vals, l1 = _track_values(Gm, G0m, GCs, gcs_cache, [i])
                vals, l1 = M.fetch([vals, l1])
                val = m.validate_training(X_vals[i], input_length, output_length, m.num_series)
                fits[i].record(it, vals[0, :, 0], vals[0, :, 1], l1[0, 0], val,
                               lambda m=m: dict((k, v.detach().clone()) for k, v in m.state_dict().items()),
                               lookback, check_every, verbose)
    out = []
    for i in range(R):
        m, f = models[i], fits[i]
        with torch.no_grad():  # restore_parameters (general_utils/model_utils.py:309-313)
            if torch.is_tensor(f.best):
                pack.fac[rows[i]].copy_(f.best)
            elif f.best is not None:
                m.load_state_dict(f.best)
        os.makedirs(f.save_dir, exist_ok=True)
        torch.save(standalone_copy(m), os.path.join(f.save_dir, "final_best_model.bin"))
        final = m.validate_training(X_vals[i], input_length, output_length, m.num_series)[5]
        if verbose:
            print("FINAL BEST (STOPPING CRITERIA) LOSS == ", f.best_loss, flush=True)
            print("FINAL BEST (STOPPING CRITERIA) EPOCH == ", f.best_it, flush=True)
            print("FINAL VALIDATION COMBO LOSS == ", final, flush=True)
        m.fit_history = f.history()
        out.append(final)
    return out
