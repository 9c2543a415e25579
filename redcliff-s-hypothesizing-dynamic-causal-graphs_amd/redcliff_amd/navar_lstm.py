"""NAVAR (LSTM), the recurrent additive forecasting baseline of the paper's comparison table
(models/navar.py:129-246; model type "NAVAR_CLSTM", general_utils/model_utils.py:624-631 and :1035-;
train/NAVAR_CLSTM_d4IC_BCTVgs1Parsim.py runs 15 fits of it).

N per-source nn.LSTM(1, H) over the T' = T - 1 first rows of a window, a Linear(H, N) on every h_t; the
N x N contributions are summed over the sources into one prediction per time step.  The loss is
criterion(pred[:, :, -1], y) + (lambda1 / N) * mean over the B*T' rows of sum_c |contributions|; the
causal matrix is the standard deviation of the contributions over all n*T' rows of the training set.

Two routes, chosen by ``REDCLIFF_NAVAR_LSTM_PATH=fused|generic`` (default fused):

* fused -- ``redcliff_navar_lstm_run`` (csrc/rc_navar_lstm.hip): one native call per epoch enqueues
  every Adam step of the epoch; parameters and the optimizer's exp_avg / exp_avg_sq / step are views of
  one packed buffer per model.  Taken when ``fused_eligible`` holds.
* generic -- the reference's operations (nn.LSTM, autograd, the caller's optimizer); serves
  hidden_layers > 1, dropout, other criteria / optimizers, shapes outside the limits and the CPU.

One deliberate departure: the reference's validation line compares (n, N, T') with (n, N) and raises on
broadcasting; with val_proportion > 0 both routes use ``val_pred[:, :, -1]``, the training loss's form.

``fit_navar_lstm_baselines`` fits R same-shape models with the replica on a grid axis;
``NAVARLSTM.fit`` is that function with lists of one.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import packs
from .navar import MAX_REPLICAS, _Family, _fit_navar_family, _plain_fit, _run

LDS_MAX_FLOATS = 40960  # RC_LDS_MAX_FLOATS
MAX_N, MAX_H, MAX_TP, MAX_B = 32, 448, 64, 512  # csrc/rc_navar_lstm.h
FWD_B = 128  # windows per FORWARD chunk
TRAIN, FORWARD = 0, 1


def navar_lstm_path():
    """'fused' (default) or 'generic', from REDCLIFF_NAVAR_LSTM_PATH."""
    return packs.route_from_env("REDCLIFF_NAVAR_LSTM_PATH")


def navar_lstm_lds_floats(N, H, Tp, Bmax=1, R=1):
    """rc_navar_lstm_lds_floats (csrc/rc_navar_lstm.h) restated: the backward workgroup's LDS floats, 0
    outside the limits."""
    if min(N, H, Tp, Bmax, R) < 1:
        return 0
    if N > MAX_N or H > MAX_H or Tp > MAX_TP or Bmax > MAX_B or R > MAX_REPLICAS:
        return 0
    f = 64 * (((H + 15) // 16 * 16) | 1) + 64 * 65 + 64 * (N | 1) + 64 * 17 + 34 * N + 384
    return f if f <= LDS_MAX_FLOATS else 0


def navar_lstm_dims(N, H, Tp, Bmax=1, R=1):
    return nat.Dims(R=R, Bmax=Bmax, T=Tp + 1, p=N, L=Tp, K=1, h=H, F=1, n=1, H=1, M1=1, nsup=0, use_sigmoid=0,
                    sigmoid_ecc=0.0)


def navar_lstm_supported(N, H, Tp, Bmax=1, R=1):
    """redcliff_navar_lstm_supported: the footprint in floats, 0 outside the limits."""
    d = navar_lstm_dims(N, H, Tp, Bmax, R)
    return int(nat.lib().redcliff_navar_lstm_supported(ctypes.byref(d)))


def navar_lstm_ws_floats(N, H, Tp, B, train=True):
    """rc_navar_lstm_ws(...).total: workspace floats of one stepped replica at batch size B."""
    nS, NH = (H + 15) // 16, N * Tp * B * H
    f = 2 * NH
    if train:
        f += 4 * NH + 2 * N * nS * B * H + N * B * H + 2 * Tp * B * N * N + B * N + navar_lstm_layout(N, H)[1]
    return (f + 63) // 64 * 64


def navar_lstm_layout(N, H):
    """[(name, offset, shape)] of the packed block and its size (rc_navar_lstm_off); every entry holds
    the N sources' tensors of one kind."""
    out, at = [], 0
    for name, shp in (("Wih", (N, 4 * H, 1)), ("Whh", (N, 4 * H, H)), ("bih", (N, 4 * H)), ("bhh", (N, 4 * H)),
                      ("Wfc", (N, N, H)), ("bfc", (N, N)), ("biases", (1, N))):
        out.append((name, at, shp))
        at += int(np.prod(shp))
    return out, at


def navar_lstm_run(d, mode, B, tB, row0, n, nX, X, x_pstride, perm, perm_pstride, par, par_m, par_v, par_stride, hyper,
                   mse, l1, pred, contrib, ws, replicas=None, stream=None, launches=0):
    """redcliff_navar_lstm_run on device tensors (None = a null pointer); returns its code.  `launches` masks
    the step's launches: 1 forward | 2 output + reduction | 4 backward | 8 dWhh + Adam."""
    return _run(nat.NavarLstmArgs, "redcliff_navar_lstm_run", d, mode, B, tB, row0, n, nX, X, x_pstride, perm,
                perm_pstride, par, par_m, par_v, par_stride, hyper, mse, l1, pred, contrib, ws, replicas, stream, launches)


# --------------------------------------------------------------------------------------------------
class NavarLstmPack(packs.AdamPack):
    """R same-shape NAVARLSTM models on the fused route (packs.AdamPack): every entry of navar_lstm_layout
    holds the N sources' tensors of one kind, the replica's hyper-parameter beside Adam is c_adj = lambda1."""

    def __init__(self, models):
        m0 = models[0]
        self.N, self.H = m0.num_nodes, m0.num_hidden
        for m in models:
            if (m.num_nodes, m.num_hidden) != (self.N, self.H):
                raise ValueError("a NavarLstmPack holds models of one shape")
        if not navar_lstm_supported(self.N, self.H, 1, R=len(models)):
            nat.check(-2, "navar_lstm_supported")
        if not m0.biases.is_cuda:
            raise RuntimeError("NAVARLSTM (fused) runs on the MI355X only (HIP kernels); move the model to 'cuda'")
        self.layout, self.n = navar_lstm_layout(self.N, self.H)
        self.allocate(models, self.n, m0.biases.device)
        self.lambda1 = [0.0] * self.R
        for r, mod in enumerate(self.models):
            prms, each = [], []  # the groups' tensors one by one, each with its own layout entry
            for group, (name, off, shp) in zip(mod.packed_parameters(), self.layout):
                per = int(np.prod(shp)) // len(group)
                prms += group
                each += [(name, off + i * per, prm.shape) for i, prm in enumerate(group)]
            packs.pack_by_layout(self.par[r], prms, each)
            self.adopt(r, prms)

    def replica_terms(self, r):
        return {"c_adj": float(self.lambda1[r])}

    def workspace(self, B, nrep, Tp=1, train=True):
        return self.workspace_of(navar_lstm_ws_floats(self.N, self.H, Tp, B, train) * max(nrep, 1))

    def dims(self, B, T):
        return navar_lstm_dims(self.N, self.H, int(T) - 1, Bmax=int(B), R=self.R)

    def train(self, X, x_pstride, perm, perm_pstride, n, B, active=None, ws=None, launches=0):
        """One TRAIN call: ceil(n / B) Adam steps over perm[0 .. n) for the replicas `active` (None:
        all).  X (.., nX, T, N) float32, perm int32 on the device.  Returns (mse, l1) device tensors
        [stepped][nsteps].  A call restricted by `launches` (profiling) is no whole step and counts none."""
        reps = self.reps(active)
        nsteps = -(-int(n) // int(B))
        mse = torch.empty(len(reps), nsteps, device=self.device, dtype=torch.float32)
        l1 = torch.empty_like(mse)
        if not reps or n == 0:
            return mse, l1
        self.require_optimizers(reps)
        t_base = self.opt[reps[0]]["t"]
        T, nX = int(X.shape[-2]), int(X.shape[-3])
        ws = self.workspace(B, len(reps), T - 1, True) if ws is None else ws
        rc = navar_lstm_run(self.dims(B, T), TRAIN, B, t_base + 1, 0, n, nX, X, x_pstride, perm, perm_pstride, self.par,
                            self.m, self.v, self.n, self.hyper(t_base, reps), mse, l1, None, None, ws,
                            None if active is None else reps, launches=launches)
        nat.check(rc, "navar_lstm_run")
        if launches == 0:
            self.advance(reps, nsteps)
        return mse, l1

    def forward(self, X, x_pstride, row0, n, active=None, B=None, ws=None):
        """One FORWARD call over rows [row0, row0 + n): (pred [stepped][n][N][T'],
        contrib [stepped][n * T'][N*N])."""
        reps = self.reps(active)
        T, nX = int(X.shape[-2]), int(X.shape[-3])
        pred = torch.empty(len(reps), n, self.N, T - 1, device=self.device, dtype=torch.float32)
        contrib = torch.empty(len(reps), n * (T - 1), self.N * self.N, device=self.device, dtype=torch.float32)
        if not reps or n == 0:
            return pred, contrib
        B = min(FWD_B, int(n)) if B is None else int(B)
        ws = self.workspace(B, len(reps), T - 1, False) if ws is None else ws
        rc = navar_lstm_run(self.dims(B, T), FORWARD, B, 1, row0, n, nX, X, x_pstride, None, 0, self.par, None, None,
                            self.n, None, None, None, pred, contrib, ws, None if active is None else reps)
        nat.check(rc, "navar_lstm_run")
        return pred, contrib


# --------------------------------------------------------------------------------------------------
class NAVARLSTM(packs.PackSlot, nn.Module):
    _slot_key, _pack_class = "_nv_slot", NavarLstmPack

    def __init__(self, num_nodes, num_hidden, maxlags, hidden_layers=1, dropout=0):
        super().__init__()
        self.num_nodes = num_nodes
        self.num_hidden = num_hidden
        self.maxlags = maxlags  # accepted and unused, as in the reference
        self.hidden_layers = hidden_layers
        self.dropout_p = dropout
        self.lstm_list = nn.ModuleList()
        self.fc_list = nn.ModuleList()
        for _ in range(num_nodes):  # LSTM i then Linear i: the reference's construction (and RNG) order
            self.lstm_list.append(nn.LSTM(1, num_hidden, hidden_layers, dropout=dropout, batch_first=True))
            self.fc_list.append(nn.Linear(num_hidden, num_nodes))
        self.biases = nn.Parameter(torch.ones(1, num_nodes) * 0.0001)
        self.causal_matrix = None

    def forward(self, x):
        """x (B, N, T') -> (predictions (B, N, T'), contributions (B*T', N*N, 1)); row b*T' + t, channel
        i*N + j is the contribution of source i to target j at step t."""
        B, _, Tp = x.size()
        N = self.num_nodes
        contributions = torch.zeros((B, N * N, Tp), device=x.device, dtype=x.dtype)
        xs = x.split(1, dim=1)
        for node in range(N):
            out, _ = self.lstm_list[node](torch.transpose(xs[node], 1, 2))
            contributions[:, node * N:(node + 1) * N, :] = self.fc_list[node](out).transpose(1, 2)
        contributions = contributions.view([B, N, N, Tp])
        predictions = torch.sum(contributions, dim=1) + self.biases.transpose(0, 1)
        contributions = contributions.permute(0, 3, 1, 2)
        return predictions, contributions.reshape(-1, N * N, 1)

    def GC(self):
        return self.causal_matrix

    # ------------------------------------------------------------------ route
    def packed_parameters(self):
        """The parameters in the packed layout's order: one list of the N sources' tensors per entry."""
        ls, fs = self.lstm_list, self.fc_list
        return [[m.weight_ih_l0 for m in ls], [m.weight_hh_l0 for m in ls], [m.bias_ih_l0 for m in ls],
                [m.bias_hh_l0 for m in ls], [m.weight for m in fs], [m.bias for m in fs], [self.biases]]

    def fused_eligible(self, criterion=None, optimizer=None, T=None, Bmax=1):
        """The fused route serves this model (and, when given, this loss, optimizer and window shape)."""
        if navar_lstm_path() != "fused":
            return False
        if self.dropout_p != 0 or self.hidden_layers != 1:
            return False
        if not _plain_fit(self, criterion, optimizer):
            return False
        if not all(p.is_cuda and p.dtype == torch.float32 for p in self.parameters()):
            return False
        Tp = 1 if T is None else int(T) - 1
        if not navar_lstm_lds_floats(self.num_nodes, self.num_hidden, Tp, int(Bmax)):
            return False
        return navar_lstm_supported(self.num_nodes, self.num_hidden, Tp, int(Bmax)) > 0

    def fit(self, save_path, X_train, Y_train, criterion, optimizer, X_val=None, Y_val=None, val_proportion=0.0,
            epochs=200, batch_size=300, check_every=1000, lambda1=0, rng=None):
        return fit_navar_lstm_baselines([self], [save_path], [X_train], criterion, [optimizer],
                                        X_vals=None if X_val is None else [X_val], val_proportion=val_proportion,
                                        epochs=epochs, batch_size=batch_size, check_every=check_every, lambda1=lambda1,
                                        rngs=None if rng is None else [rng], verbose=1)[0]


_LSTM = _Family("fit_navar_lstm_baselines", NavarLstmPack, lambda m: (m.num_nodes, m.num_hidden, m.hidden_layers),
                lambda m, criterion, optimizer, T, Bmax, split: T >= 2 and Bmax <= MAX_B and m.fused_eligible(
                    criterion, optimizer, T=T, Bmax=Bmax), True)


def fit_navar_lstm_baselines(models, save_paths, X_trains, criterion, optimizers, X_vals=None, val_proportion=0.0,
                             epochs=200, batch_size=300, check_every=1000, lambda1=0, rngs=None, verbose=0):
    """NAVARLSTM.fit (models/navar.py:181-246) for a list of models: navar._fit_navar_family."""
    return _fit_navar_family(_LSTM, models, save_paths, X_trains, criterion, optimizers, X_vals, val_proportion, epochs,
                             batch_size, check_every, lambda1, rngs, verbose, False)


