"""cLSTM_FM, the cLSTM forecasting baseline the paper compares REDCLIFF-S against
(models/clstm_fm.py; built for model type "cLSTM", general_utils/model_utils.py:472-481, and fitted
with one Adam, :853-874).

One ``cLSTM`` (K = 1), no factor-score embedder; the loss is FORECAST_COEFF * sum_i MSE(pred[:, :, i],
target[:, :, i]) + ADJ_L1_REG_COEFF * ||GC||_1 over the overlapping length-``context`` sequences of
rows [0, max_input_length) of every recording (the DAGness term is commented out in the reference
and reported as None / 0).

Two routes, chosen as in cmlp_fm.py:

* fused -- ``redcliff_lstm_fm_run`` (csrc/rc_lstm_fm.hip): the loss separates over the p channel
  networks, so one workgroup per (network, replica) keeps the network's weights and Adam moments in
  LDS and runs every batch of an epoch in ONE launch.  Taken when ``redcliff_lstm_fm_supported``
  accepts the shape and the model has no wavelets, num_sims == 1, no caller-supplied hidden state and
  its parameters on the GPU.  The parameters and the optimizer's exp_avg / exp_avg_sq / step are
  views of packed buffers (kernels.lstm_layout).
* generic -- the reference's tensor operations through torch's nn.LSTM and autograd; serves every
  other configuration, and the CPU.  ``REDCLIFF_LSTM_FM_PATH=generic`` forces it.

``fit_lstm_baselines`` fits many same-shape models (e.g. the 15 fold / SNR fits of
train/CLSTM_d4IC_BLgs1Parsim.py) with one launch per epoch; ``cLSTM_FM.fit`` is that loop with a list
of one.  The reference looks at losses and norms on check epochs only, so on the fused route the
epochs between make no device-to-host fetch: every epoch's per-step sums are reduced to its four
history entries on the device and fetched, together with the validation values and ||GC||_1, at the
next check (and once at the end).  The training loader is uploaded once and replayed in order.
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
from .clstm import cLSTM
from .cmlp_fm import DAGNessLoss, _segments, _upload
from .fit_loop import standalone_copy

LDS_MAX_FLOATS = 40960  # RC_LDS_MAX_FLOATS
LF_BC = 32              # sequences per pass (csrc/rc_lstm_fm.h)
MAX_P, MAX_H, MAX_C, MAX_B, MAX_REPLICAS = 64, 64, 64, 512, 256
FLAGS_TRAIN = nat.LOSS_FORECAST | nat.LOSS_ADJ | nat.STEP_B | nat.VALUES
FLAGS_VALUES = nat.LOSS_FORECAST | nat.LOSS_ADJ | nat.VALUES
HISTORY_KEYS = ("avg_forecasting_loss", "avg_adj_penalty", "avg_dagness_loss", "avg_smooth_loss")


def lstm_fm_path():
    """'fused' (default) or 'generic', from REDCLIFF_LSTM_FM_PATH."""
    return packs.route_from_env("REDCLIFF_LSTM_FM_PATH")


def lstm_fm_lds_floats(p, h, C):
    """The workgroup's LDS footprint in floats (rc_lstm_fm_lds_floats, csrc/rc_lstm_fm.h)."""
    K = p + h
    Kp, hp = K | 1, h | 1
    n = 4 * h * Kp + 9 * h + 1
    return 4 * n + LF_BC * ((((C + 1) * K) | 1) + ((4 * h * C) | 1) + ((h * C) | 1) + 2 * hp + 2 * C) + p + 16


def lstm_fm_shape_supported(p, h, C, Bmax=1, T=None, R=1):
    """The limits of redcliff_lstm_fm_run, restated (tests compare it with redcliff_lstm_fm_supported)."""
    T = C + 1 if T is None else T
    if min(p, h, C, Bmax, T, R) < 1:
        return False
    return (p <= MAX_P and h <= MAX_H and C <= MAX_C and Bmax <= MAX_B and R <= MAX_REPLICAS
            and lstm_fm_lds_floats(p, h, C) <= LDS_MAX_FLOATS)


def lstm_fm_dims(p, h, Bmax=1, T=2, R=1):
    return nat.Dims(R=R, Bmax=Bmax, T=T, p=p, L=1, K=1, h=h, F=1, n=1, H=1, M1=1, nsup=0, use_sigmoid=0,
                    sigmoid_ecc=0.0)


def lstm_fm_supported(p, h, C, Bmax=1, T=None, R=1):
    """redcliff_lstm_fm_supported: the footprint in floats, 0 outside the limits."""
    d = lstm_fm_dims(p, h, Bmax, C + 1 if T is None else T, R)
    return int(nat.lib().redcliff_lstm_fm_supported(ctypes.byref(d), int(C)))


def lstm_fm_run(d, context, tmax, flags, B, tB, row0, N, X, x_pstride, fac, fac_m, fac_v, fac_stride, hyper, sse, pen,
                G=None, replicas=None, stream=None):
    """redcliff_lstm_fm_run on device tensors (None = a null pointer); returns its code."""
    p_ = nat.ptr
    a = nat.LstmFMArgs()
    a.d = d
    a.context, a.tmax = int(context), int(tmax)
    a.flags, a.B, a.tB, a.row0, a.N = int(flags), int(B), int(tB), int(row0), int(N)
    a.X, a.x_pstride = p_(X), int(x_pstride)
    a.fac, a.fac_m, a.fac_v, a.fac_stride = p_(fac), p_(fac_m), p_(fac_v), int(fac_stride)
    a.hyper, a.sse, a.pen, a.G = p_(hyper), p_(sse), p_(pen), p_(G)
    keep = nat.replica_list(a, replicas)  # a local, so alive until the call has returned
    return nat.lib().redcliff_lstm_fm_run(ctypes.byref(a), nat.stream_or_current(stream))


# --------------------------------------------------------------------------------------------------
class LstmPack(packs.AdamPack):
    """R same-shape cLSTM_FM models on the fused route (packs.AdamPack; the rows `par` are also named `fac`):
    parameters by kernels.lstm_layout, the replica's hyper-parameters beside Adam are the two loss
    coefficients, and only the reference's one plain Adam can be bound."""

    def __init__(self, models):
        m0 = models[0]
        self.p, self.h = m0.num_series, m0.gen_hidden
        for m in models:
            if (m.num_series, m.gen_hidden) != (self.p, self.h) or m.wavelet_level is not None:
                raise ValueError("an LstmPack holds models of one shape, without wavelets")
        if not 1 <= len(models) <= MAX_REPLICAS:
            raise ValueError("an LstmPack holds 1..%d models" % MAX_REPLICAS)
        kernels.require_gpu(next(m0.parameters()), "cLSTM_FM (fused)")
        self.n = kernels.lstm_layout(self.p, self.h)["total"]
        self.allocate(models, self.n, next(m0.parameters()).device)
        self.fac = self.par
        for r, mod in enumerate(self.models):
            self.adopt_views(r, kernels.lstm_views(self.fac[r], mod.factors[0], self.p, self.h))

    def check_optimizer(self, r, opt):
        packs.require_plain_adam(opt, self.params[r], "cLSTM_FM", "model_utils.py:853-874")

    def replica_terms(self, r):
        m = self.models[r]
        return {"c_forecast": float(m.FORECAST_COEFF), "c_adj": float(m.ADJ_L1_REG_COEFF)}

    def run(self, flags, X, x_pstride, T, tmax, context, B, N, row0=0, active=None, G=None):
        """One redcliff_lstm_fm_run over recordings [row0, row0 + N) of X in batches of B for the
        replicas `active` (None: all).  Returns (sse, pen) device tensors [stepped][nsteps][p] (pen
        None without VALUES)."""
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
        d = lstm_fm_dims(self.p, self.h, Bmax=int(B), T=int(T), R=self.R)
        rc = lstm_fm_run(d, context, tmax, flags, B, t_base + 1, row0, N, X, x_pstride, self.fac,
                         self.m if stepping else None, self.v if stepping else None, self.n, self.hyper(t_base, reps),
                         sse, pen, G, None if active is None else reps)
        nat.check(rc, "lstm_fm_run")
        if stepping:
            self.advance(reps, nsteps)
        return sse, pen


def _step_scale(sizes, S, C, device):
    """Device float64 [steps]: 1 / (Bq * C) of each batch, Bq = B_i * S sequences."""
    return torch.tensor([1.0 / (B * S * C) for B in sizes], dtype=torch.float64, device=device)


def _coef(model, n, device):
    """Device float64 (4, 2): per-epoch sums (sum_steps sum_j sse / (Bq C), sum_steps sum_j pen) ->
    (avg forecasting loss, avg adjacency penalty, avg DAGness loss = 0, avg smooth loss)."""
    fc, ac = float(model.FORECAST_COEFF) / n, float(model.ADJ_L1_REG_COEFF) / n
    return torch.tensor([[fc, 0.], [0., ac], [0., 0.], [fc, ac]], dtype=torch.float64, device=device)


def _reduce(sse, pen, scale, coef):
    """One replica's per-step sums ([steps][p] each) -> its four averaged loss terms, on the device.
    Done per replica, on tensors of the single fit's shapes, so that a packed fit's values are the
    single fit's bit for bit."""
    s = torch.stack([(sse.double().sum(1) * scale).sum(), pen.double().sum()])
    return coef @ s


# --------------------------------------------------------------------------------------------------
class cLSTM_FM(packs.PackSlot, nn.Module):
    _slot_key, _pack_class, _unpickled = "_lf_slot", LstmPack, ("_lf_data",)

    def __init__(self, num_chans, gen_hidden, embed_hidden_sizes, num_in_timesteps, coeff_dict, num_sims=1,
                 wavelet_level=None, save_path=None):
        super().__init__()
        self.num_chans = num_chans
        self.num_series = num_chans * (wavelet_level + 1) if wavelet_level is not None else num_chans
        self.gen_hidden = gen_hidden
        self.embed_hidden_sizes = embed_hidden_sizes
        self.num_in_timesteps = num_in_timesteps
        self.num_factors_nK = 1
        self.coeff_dict = coeff_dict
        self.FORECAST_COEFF = coeff_dict["FORECAST_COEFF"]
        self.ADJ_L1_REG_COEFF = coeff_dict["ADJ_L1_REG_COEFF"]
        self.DAGNESS_REG_COEFF = coeff_dict["DAGNESS_REG_COEFF"]
        self.num_sims = num_sims
        self.wavelet_level = wavelet_level
        self.supervised_loss_fn = nn.MSELoss(reduction='mean')
        self.dagness_loss_fn = DAGNessLoss()
        self.factor_score_embedder = None
        self.factors = nn.ModuleList([cLSTM(num_chans, gen_hidden, wavelet_level=wavelet_level, save_path=save_path)
                                      for _ in range(self.num_factors_nK)])
        self.gen_model = nn.ModuleList([self.factor_score_embedder, self.factors])

    # ------------------------------------------------------------------ route
    def _device(self):
        return next(self.parameters()).device

    def fused_eligible(self, context, tmax, Bmax=1, T=None):
        """The fused route serves this model on sequences of `context` rows out of rows [0, tmax)."""
        if lstm_fm_path() != "fused":
            return False
        if self.wavelet_level is not None or self.num_sims != 1:
            return False
        if not next(self.parameters()).is_cuda:
            return False
        if not isinstance(context, int) or context < 1 or tmax <= context or (T is not None and tmax > T):
            return False
        p, h = self.num_series, self.gen_hidden
        if not lstm_fm_shape_supported(p, h, context, Bmax=Bmax, T=T):
            return False
        return lstm_fm_supported(p, h, context, Bmax=Bmax, T=T) > 0

    @staticmethod
    def _tmax(T, max_input_length):
        return int(T) if max_input_length is None else min(int(T), int(max_input_length))

    # ------------------------------------------------------------------ reference API
    def forward(self, X, hiddens=None):
        """X (batch, T, p) -> (combined_pred, factor_preds, factor_hiddens) (:56-81)."""
        if hiddens is None:
            hiddens = [None] * self.num_factors_nK
        factor_preds, factor_hiddens = [], []
        for f, hid in zip(self.factors, hiddens):
            pred, hidden = f(X, hid)
            factor_preds.append(pred)
            factor_hiddens.append(hidden)
        combined_pred = factor_preds[0]
        for pred in factor_preds[1:]:
            combined_pred = combined_pred + pred
        return combined_pred, factor_preds, factor_hiddens

    def GC(self, threshold=True, combine_wavelet_representations=False, rank_wavelets=False):
        return [f.GC(threshold=threshold, combine_wavelet_representations=combine_wavelet_representations,
                     rank_wavelets=rank_wavelets) for f in self.factors]

    def arrange_input(self, data, context):
        """One series (T, dim) -> its T - context overlapping sequences and their one-step-ahead
        targets, (T - context, context, dim) each (:95-112)."""
        assert context >= 1 and isinstance(context, int)
        n = len(data) - context
        inp = torch.stack([data[i:n + i] for i in range(context)], dim=1).to(torch.float32)
        tgt = torch.stack([data[i + 1:n + i + 1] for i in range(context)], dim=1).to(torch.float32)
        return inp.detach(), tgt.detach()

    def configure_context_data_and_targets(self, X, max_input_length, context):
        """(batch, T, p) recordings -> the sequences and targets of all of them, recording-major, on
        the model's device (:114-122; arrange_input for the whole batch at once)."""
        assert context >= 1 and isinstance(context, int)
        if max_input_length is not None:
            X = X[:, :max_input_length, :]
        X = X.to(self._device())
        N, T, p = X.shape
        S = T - context
        inp = torch.stack([X[:, i:S + i] for i in range(context)], dim=2).reshape(N * S, context, p)
        tgt = torch.stack([X[:, i + 1:S + i + 1] for i in range(context)], dim=2).reshape(N * S, context, p)
        return inp.to(torch.float32).detach(), tgt.to(torch.float32).detach()

    def compute_loss(self, preds, targets):
        gc = self.GC(threshold=False, combine_wavelet_representations=False, rank_wavelets=False)
        forecasting_loss = self.FORECAST_COEFF * sum([self.supervised_loss_fn(preds[:, :, i], targets[:, :, i])
                                                      for i in range(self.num_series)])
        adj_l1_penalty = self.ADJ_L1_REG_COEFF * sum([torch.norm(A, 1) for A in gc])
        smooth_loss = forecasting_loss + adj_l1_penalty
        return smooth_loss, [forecasting_loss, adj_l1_penalty, None]

    def batch_update(self, batch_num, X, max_input_length, context, gen_optim, running_forecasting_loss,
                     running_adj_penalty, running_dagness_loss, running_smooth_loss):
        tmax = self._tmax(X.shape[1], max_input_length)
        if self.fused_eligible(context, tmax, Bmax=int(X.shape[0]), T=int(X.shape[1])):
            pack, r = self._slot()
            pack.bind_optimizer(r, gen_optim)
            X = X.to(self._device(), torch.float32).contiguous()
            B, T = int(X.shape[0]), int(X.shape[1])
            sse, pen = pack.run(FLAGS_TRAIN, X, 0, T, tmax, context, B, B, active=[r])
            scale = _step_scale([B], tmax - context, context, self._device())
            f, a, _, s = M.fetch([_reduce(sse[0], pen[0], scale, _coef(self, 1, self._device()))])[0]
            return (running_forecasting_loss + float(f), running_adj_penalty + float(a), running_dagness_loss + 0.,
                    running_smooth_loss + float(s))
        X_in, X_target = self.configure_context_data_and_targets(X, max_input_length, context)
        for f in self.factors:
            f.train()
        gen_optim.zero_grad()
        x_sims, _, _ = self.forward(X_in, hiddens=None)
        smooth, (forecasting_loss, adj_l1, _) = self.compute_loss(x_sims, X_target)
        smooth.backward()
        gen_optim.step()
        return (running_forecasting_loss + forecasting_loss.detach().item(), running_adj_penalty + adj_l1.detach().item(),
                running_dagness_loss + 0., running_smooth_loss + smooth.detach().item())

    def _eval_device(self, ds, tmax, context):
        """Fused validation of an uploaded loader: device float64 [4] averaged loss terms."""
        pack, r = self._slot()
        T = int(ds["X"].shape[1])
        sse, pen = [], []
        for row0, N, B in _segments(ds["sizes"]):
            s, q = pack.run(FLAGS_VALUES, ds["X"], 0, T, tmax, context, B, N, row0=row0, active=[r])
            sse.append(s[0])
            pen.append(q[0])
        dev = self._device()
        return _reduce(torch.cat(sse, 0), torch.cat(pen, 0), _step_scale(ds["sizes"], tmax - context, context, dev),
                       _coef(self, len(ds["sizes"]), dev))

    def _terms(self, f, a, s, componentwise, normalized):
        if normalized:
            if self.FORECAST_COEFF > 0.:
                f = f / self.FORECAST_COEFF
            if self.ADJ_L1_REG_COEFF > 0.:
                a = a / self.ADJ_L1_REG_COEFF
        if componentwise:
            return f, a, 0., s, s
        return s

    def training_sim_eval(self, X_val, max_input_length, context, num_series, return_loss_componentwise=False,
                          report_normalized_loss_components=False):
        ds = _upload(X_val, self._device(), self.__dict__.setdefault("_lf_data", {}))
        T = int(ds["X"].shape[1])
        tmax = self._tmax(T, max_input_length)
        if self.fused_eligible(context, tmax, Bmax=max(ds["sizes"]), T=T):
            f, a, _, s = [float(x) for x in M.fetch([self._eval_device(ds, tmax, context)])[0]]
            return self._terms(f, a, s, return_loss_componentwise, report_normalized_loss_components)
        for fac in self.factors:
            fac.eval()
        af = aa = asm = 0.
        row = 0
        with torch.no_grad():
            for B in ds["sizes"]:
                X_in, X_target = self.configure_context_data_and_targets(ds["X"][row:row + B], max_input_length, context)
                row += B
                x_sims, _, _ = self.forward(X_in, hiddens=None)
                smooth, (fl, al, _) = self.compute_loss(x_sims, X_target)
                if report_normalized_loss_components:
                    if self.FORECAST_COEFF > 0.:
                        fl = fl / self.FORECAST_COEFF
                    if self.ADJ_L1_REG_COEFF > 0.:
                        al = al / self.ADJ_L1_REG_COEFF
                af += fl.item()
                aa += al.item()
                asm += smooth.item()
        n = len(ds["sizes"])
        return self._terms(af / n, aa / n, asm / n, return_loss_componentwise, False)

    def save_checkpoint(self, save_dir, it, best_model, avg_forecasting_loss, avg_adj_penalty, avg_dagness_loss,
                        avg_smooth_loss, best_loss, GC=None, X_train=None, input_length=None, num_sim_steps=None,
                        X_val=None):
        """The two files of :180-193 (the plots of :195-212 are not drawn, as in our other fits)."""
        os.makedirs(save_dir, exist_ok=True)
        torch.save(standalone_copy(best_model) if isinstance(best_model, nn.Module) else best_model,
                   os.path.join(save_dir, "temp_best_model_epoch" + str(it) + ".bin"))
        with open(os.path.join(save_dir, "training_meta_data_and_hyper_parameters.pkl"), "wb") as outfile:
            pkl.dump({
                "epoch": it,
                "avg_forecasting_loss": avg_forecasting_loss,
                "avg_adj_penalty": avg_adj_penalty,
                "avg_dagness_loss": avg_dagness_loss,
                "avg_smooth_loss": avg_smooth_loss,
                "best_loss": best_loss,
            }, outfile)

    def fit(self, save_dir, X_train, gen_optim, context, max_input_length, num_sim_steps, max_iter, lookback=5,
            check_every=50, verbose=1, GC=None, X_val=None):
        """GC is accepted and unused: it only feeds the reference's plots."""
        if X_val is None:
            raise ValueError("cLSTM_FM.fit needs X_val (the reference's fit evaluates it at every check)")
        return fit_lstm_baselines([self], [gen_optim], [save_dir], [X_train], [X_val], context, max_input_length,
                                  max_iter, lookback=lookback, check_every=check_every, verbose=verbose)[0]


# --------------------------------------------------------------------------------------------------
class _Fit:
    """One model's bookkeeping of fit() (:217-338)."""

    def __init__(self, model, opt, save_dir):
        self.model, self.opt, self.save_dir = model, opt, save_dir
        self.h = {k: [] for k in HISTORY_KEYS}
        self.best_it, self.best_loss, self.best = None, np.inf, None
        self.done, self.stop_epoch = False, None

    def extend(self, rows):
        """rows: [4] history entries of consecutive epochs."""
        for row in rows:
            for k, v in zip(HISTORY_KEYS, row):
                self.h[k].append(float(v))

    def check(self, it, l1, val, snapshot, lookback, check_every, verbose):
        """A check epoch (:260-324): the stop rule on curr_l1_loss alone, else the checkpoint.
        Returns True when the fit stops."""
        if verbose > 0:
            print(("-" * 10 + "Iter = %d" + "-" * 10) % (it + 1), flush=True)
            print("Validation Loss = %f" % val)
        if l1 < self.best_loss:
            self.best_loss, self.best_it, self.best = l1, it, snapshot()
        elif self.best_it is not None and (it - self.best_it) == lookback * check_every:
            if verbose:
                print("Stopping early", flush=True)
            self.done, self.stop_epoch = True, it
            return True
        self.model.save_checkpoint(self.save_dir, it, self.best_module(), self.h["avg_forecasting_loss"],
                                   self.h["avg_adj_penalty"], self.h["avg_dagness_loss"], self.h["avg_smooth_loss"],
                                   self.best_loss)
        return False

    def best_module(self):
        m = standalone_copy(self.model)
        if torch.is_tensor(self.best):  # a snapshot of the packed parameters
            with torch.no_grad():
                for prm, view in kernels.lstm_views(self.best, m.factors[0], m.num_series, m.gen_hidden):
                    prm.copy_(view)
        elif self.best is not None:
            m.load_state_dict(self.best)
        return m

    def history(self):
        out = dict(self.h)
        out.update(best_loss=self.best_loss, best_it=self.best_it, stop_epoch=self.stop_epoch)
        return out


def fit_lstm_baselines(models, optimizers, save_dirs, X_trains, X_vals, context, max_input_length, max_iter,
                       lookback=5, check_every=50, verbose=0):
    """cLSTM_FM.fit (:217-338) for a list of same-shape models, each with its own data, optimizer and
    save_dir.  On the fused route an epoch is one redcliff_lstm_fm_run over the still active models;
    a check epoch adds one for validation and the loop's only device-to-host fetch.  A model that
    stops early leaves the active list.  Returns the models' final validation losses; every model's
    histories are left in ``model.fit_history``."""
    R = len(models)
    if not (len(optimizers) == len(save_dirs) == len(X_trains) == len(X_vals) == R) or R == 0:
        raise ValueError("fit_lstm_baselines: one optimizer, save_dir and loader pair per model")
    if any(v is None for v in X_vals):
        raise ValueError("fit_lstm_baselines needs a validation loader for every model")
    dev = models[0]._device()
    caches = [m.__dict__.setdefault("_lf_data", {}) for m in models]
    tr = [_upload(X_trains[i], dev, caches[i]) for i in range(R)]
    va = [_upload(X_vals[i], dev, caches[i]) for i in range(R)]
    same = all(t["sizes"] == tr[0]["sizes"] and t["X"].shape == tr[0]["X"].shape for t in tr) and \
        all(v["sizes"] == va[0]["sizes"] and v["X"].shape == va[0]["X"].shape for v in va) and \
        all((m.num_series, m.gen_hidden) == (models[0].num_series, models[0].gen_hidden) for m in models)
    if R > 1 and not same:  # nothing to share: fit one after the other
        return [fit_lstm_baselines([models[i]], [optimizers[i]], [save_dirs[i]], [X_trains[i]], [X_vals[i]], context,
                                   max_input_length, max_iter, lookback, check_every, verbose)[0] for i in range(R)]
    Ttr, Tva = int(tr[0]["X"].shape[1]), int(va[0]["X"].shape[1])
    tm_tr, tm_va = cLSTM_FM._tmax(Ttr, max_input_length), cLSTM_FM._tmax(Tva, max_input_length)
    fused = R <= MAX_REPLICAS and all(
        m.fused_eligible(context, tm_tr, Bmax=max(tr[0]["sizes"]), T=Ttr) and
        m.fused_eligible(context, tm_va, Bmax=max(va[0]["sizes"]), T=Tva) for m in models)
    fits = [_Fit(models[i], optimizers[i], save_dirs[i]) for i in range(R)]
    if fused:
        pack, rows, _ = packs.acquire(models, optimizers, LstmPack)
        p = pack.p
        Xtr, xps_tr = packs.stack_upload([t["X"] for t in tr], dev)
        Xva, xps_va = packs.stack_upload([v["X"] for v in va], dev)
        G =torch.zeros(pack.R, p, p, device=dev, dtype=torch.float32)
        seg_tr, seg_va = _segments(tr[0]["sizes"]), _segments(va[0]["sizes"])
        sc_tr = _step_scale(tr[0]["sizes"], tm_tr - context, context, dev)
        sc_va = _step_scale(va[0]["sizes"], tm_va - context, context, dev)
        cf_tr = [_coef(m, len(tr[0]["sizes"]), dev) for m in models]
        cf_va = [_coef(m, len(va[0]["sizes"]), dev) for m in models]
        pending = [[] for _ in range(R)]  # per model: device [4] history entries not fetched yet

        def validate(live):
            sse, pen = [], []
            for row0, N, B in seg_va:
                s, q = pack.run(FLAGS_VALUES, Xva, xps_va, Tva, tm_va, context, B, N, row0=row0,
                                active=[rows[i] for i in live])
                sse.append(s)
                pen.append(q)
            sse, pen = torch.cat(sse, 1), torch.cat(pen, 1)
            return [_reduce(sse[a], pen[a], sc_va, cf_va[i]) for a, i in enumerate(live)]

        def drain(live, extra):
            """The one fetch: every pending history entry of the models `live`, then `extra`."""
            counts = [len(pending[i]) for i in live]
            got = M.fetch([x for i in live for x in pending[i]] + extra)
            o = 0
            for i, n in zip(live, counts):
                fits[i].extend(got[o:o + n])
                pending[i] = []
                o += n
            return got[o:]

    for it in range(max_iter):
        live = [i for i in range(R) if not fits[i].done]
        if not live:
            break
        if verbose:
            print("cLSTM_FM.fit: now on epoch it == ", it, flush=True)
        check = it % check_every == 0
        if fused:
            active = [rows[i] for i in live]
            sse, pen = [], []
            for si, (row0, N, B) in enumerate(seg_tr):
                s, q = pack.run(FLAGS_TRAIN, Xtr, xps_tr, Ttr, tm_tr, context, B, N, row0=row0, active=active,
                                G=G if (check and si == len(seg_tr) - 1) else None)
                sse.append(s)
                pen.append(q)
            sse, pen = torch.cat(sse, 1), torch.cat(pen, 1)
            for a, i in enumerate(live):
                pending[i].append(_reduce(sse[a], pen[a], sc_tr, cf_tr[i]))
            if not check:
                continue
            # the reference's op on the device norms; fetch() carries float64 (exact for a float32 value)
            l1 = [torch.norm(G[rows[i]], 1).double() for i in live]
            got = drain(live, validate(live) + l1)
            for a, i in enumerate(live):
                r = rows[i]
                fits[i].check(it, float(got[len(live) + a]), float(got[a][3]), lambda r=r: pack.fac[r].clone(),
                              lookback, check_every, verbose)
        else:
            for i in live:
                m = models[i]
                run, row = (0., 0., 0., 0.), 0
                for bn, B in enumerate(tr[i]["sizes"]):
                    run = m.batch_update(bn, tr[i]["X"][row:row + B], max_input_length, context, optimizers[i], *run)
                    row += B
                fits[i].extend([[v / len(tr[i]["sizes"]) for v in run]])
                if not check:
                    continue
                val = m.training_sim_eval(X_vals[i], max_input_length, context, m.num_series)
                with torch.no_grad():
                    gc = m.GC(threshold=False, combine_wavelet_representations=False, rank_wavelets=False)
                    l1 = float(sum(torch.norm(g, 1) for g in gc))
                fits[i].check(it, l1, val, lambda m=m: dict((k, v.detach().clone()) for k, v in m.state_dict().items()),
                              lookback, check_every, verbose)
    finals = []
    for i in range(R):
        m, f = models[i], fits[i]
        with torch.no_grad():  # restore_parameters (general_utils/model_utils.py:309-313)
            if torch.is_tensor(f.best):
                pack.fac[rows[i]].copy_(f.best)
            elif f.best is not None:
                m.load_state_dict(f.best)
        os.makedirs(f.save_dir, exist_ok=True)
        torch.save(standalone_copy(m), os.path.join(f.save_dir, "final_best_model.bin"))
        if fused:
            finals.append(m._eval_device(va[i], tm_va, context))
        else:
            finals.append(m.training_sim_eval(X_vals[i], max_input_length, context, m.num_series))
    if fused:  # the last fetch: the epochs since the last check and the final validation losses
        finals = [float(x[3]) for x in drain(list(range(R)), finals)]
    for i in range(R):
        if verbose:
            print("FINAL VALIDATION COMBO LOSS == ", finals[i], flush=True)
        models[i].fit_history = fits[i].history()
    return finals
