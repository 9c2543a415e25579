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
import os

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from .navar import MAX_REPLICAS, NavarPack, _epoch_batches, _save

LDS_MAX_FLOATS = 40960  # RC_LDS_MAX_FLOATS
MAX_N, MAX_H, MAX_TP, MAX_B = 32, 448, 64, 512  # csrc/rc_navar_lstm.h
FWD_B = 128  # windows per FORWARD chunk
TRAIN, FORWARD = 0, 1


def navar_lstm_path():
    """'fused' (default) or 'generic', from REDCLIFF_NAVAR_LSTM_PATH."""
    v = os.environ.get("REDCLIFF_NAVAR_LSTM_PATH", "") or "fused"
    if v not in ("fused", "generic"):
        raise ValueError("REDCLIFF_NAVAR_LSTM_PATH must be 'fused' or 'generic', not %r" % v)
    return v


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
    """redcliff_navar_lstm_run on device tensors (None = a null pointer); returns its code."""
    def p_(t):
        return None if t is None else t.data_ptr()
    a = nat.NavarLstmArgs()
    a.d = d
    a.launches = int(launches)  # profiling: 1 forward | 2 output + reduction | 4 backward | 8 dWhh + Adam (0 = all)
    a.mode, a.B, a.tB, a.row0, a.N, a.nX = int(mode), int(B), int(tB), int(row0), int(n), int(nX)
    a.X, a.x_pstride, a.perm, a.perm_pstride = p_(X), int(x_pstride), p_(perm), int(perm_pstride)
    a.par, a.par_m, a.par_v, a.par_stride, a.hyper = p_(par), p_(par_m), p_(par_v), int(par_stride), p_(hyper)
    a.mse, a.l1, a.pred, a.contrib = p_(mse), p_(l1), p_(pred), p_(contrib)
    a.ws, a.ws_bytes = p_(ws), 0 if ws is None else ws.numel() * 4
    keep = None
    if replicas is not None:
        keep = (ctypes.c_int32 * max(len(replicas), 1))(*[int(r) for r in replicas])
        a.replicas = ctypes.cast(keep, ctypes.c_void_p)
        a.n_replicas = len(replicas)
    if stream is None:
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return nat.lib().redcliff_navar_lstm_run(ctypes.byref(a), stream)


# --------------------------------------------------------------------------------------------------
class NavarLstmPack(NavarPack):
    """R same-shape NAVARLSTM models on the fused route: their parameters are views of par[r], their
    optimizers' exp_avg / exp_avg_sq of m[r] / v[r].  bind_optimizer, hyper and bound are NavarPack's."""

    def __init__(self, models):
        m0 = models[0]
        self.N, self.H = m0.num_nodes, m0.num_hidden
        for m in models:
            if (m.num_nodes, m.num_hidden) != (self.N, self.H):
                raise ValueError("a NavarLstmPack holds models of one shape")
        self.models = list(models)
        self.R = len(models)
        if not navar_lstm_supported(self.N, self.H, 1, R=self.R):
            nat.check(-2, "navar_lstm_supported")
        self.device = m0.biases.device
        if not m0.biases.is_cuda:
            raise RuntimeError("NAVARLSTM (fused) runs on the MI355X only (HIP kernels); move the model to 'cuda'")
        self.layout, self.n = navar_lstm_layout(self.N, self.H)
        self.par = torch.empty(self.R, self.n, device=self.device, dtype=torch.float32)
        self.m = torch.zeros_like(self.par)
        self.v = torch.zeros_like(self.par)
        self.opt = [None] * self.R
        self.lambda1 = [0.0] * self.R
        self.hyper_key, self.hyper_dev = None, None
        self.ws = None
        self.params, self.ptrs = [], []
        with torch.no_grad():
            for r, mod in enumerate(self.models):
                groups = mod.packed_parameters()
                prms = []
                for group, (_, off, shp) in zip(groups, self.layout):
                    per = int(np.prod(shp)) // len(group)
                    for i, prm in enumerate(group):
                        view = self.par[r, off + i * per:off + (i + 1) * per].view(prm.shape)
                        view.copy_(prm.detach().to(self.device, torch.float32))
                        prm.data = view
                        prms.append(prm)
                self.params.append(prms)
                self.ptrs.append([prm.data_ptr() for prm in prms])
                mod.__dict__["_nv_slot"] = (self, r)

    def workspace(self, B, nrep, Tp=1, train=True):
        need = navar_lstm_ws_floats(self.N, self.H, Tp, B, train) * max(nrep, 1)
        if self.ws is None or self.ws.numel() < need:
            self.ws = None  # release before the larger allocation
            self.ws = torch.empty(need, device=self.device, dtype=torch.float32)
        return self.ws

    def dims(self, B, T):
        return navar_lstm_dims(self.N, self.H, int(T) - 1, Bmax=int(B), R=self.R)

    def train(self, X, x_pstride, perm, perm_pstride, n, B, active=None, ws=None, launches=0):
        """One TRAIN call: ceil(n / B) Adam steps over perm[0 .. n) for the replicas `active` (None:
        all).  X (.., nX, T, N) float32, perm int32 on the device.  Returns (mse, l1) device tensors
        [stepped][nsteps]."""
        reps = list(range(self.R)) if active is None else list(active)
        nsteps = -(-int(n) // int(B))
        mse = torch.empty(len(reps), nsteps, device=self.device, dtype=torch.float32)
        l1 = torch.empty_like(mse)
        if not reps or n == 0:
            return mse, l1
        for r in reps:
            if self.opt[r] is None:
                raise RuntimeError("bind_optimizer before a stepping call")
        t_base = self.opt[reps[0]]["t"]
        T, nX = int(X.shape[-2]), int(X.shape[-3])
        ws = self.workspace(B, len(reps), T - 1, True) if ws is None else ws
        rc = navar_lstm_run(self.dims(B, T), TRAIN, B, t_base + 1, 0, n, nX, X, x_pstride, perm, perm_pstride, self.par,
                            self.m, self.v, self.n, self.hyper(t_base, reps), mse, l1, None, None, ws,
                            None if active is None else reps, launches=launches)
        nat.check(rc, "navar_lstm_run")
        if launches == 0:
            for r in reps:
                st = self.opt[r]
                st["t"] += nsteps
                st["step"].fill_(float(st["t"]))
        return mse, l1

    def forward(self, X, x_pstride, row0, n, active=None, B=None, ws=None):
        """One FORWARD call over rows [row0, row0 + n): (pred [stepped][n][N][T'],
        contrib [stepped][n * T'][N*N])."""
        reps = list(range(self.R)) if active is None else list(active)
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
class NAVARLSTM(nn.Module):
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
        if criterion is not None and not (type(criterion) is nn.MSELoss and criterion.reduction == "mean"):
            return False
        if optimizer is not None:
            if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
                return False
            g = optimizer.param_groups[0]
            if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay", False):
                return False
            if set(id(p) for p in g["params"]) != set(id(p) for p in self.parameters()):
                return False
        if not all(p.is_cuda and p.dtype == torch.float32 for p in self.parameters()):
            return False
        Tp = 1 if T is None else int(T) - 1
        if not navar_lstm_lds_floats(self.num_nodes, self.num_hidden, Tp, int(Bmax)):
            return False
        return navar_lstm_supported(self.num_nodes, self.num_hidden, Tp, int(Bmax)) > 0

    def _slot(self):
        """(pack, row) holding this model's parameters; a pack of its own unless it sits in one."""
        slot = self.__dict__.get("_nv_slot")
        if slot is None or not slot[0].bound(slot[1]):
            NavarLstmPack([self])
            slot = self.__dict__["_nv_slot"]
        return slot

    def __getstate__(self):  # pickles (torch.save, deepcopy) carry the module, not its pack
        st = dict(self.__dict__)
        st.pop("_nv_slot", None)
        return st

    def fit(self, save_path, X_train, Y_train, criterion, optimizer, X_val=None, Y_val=None, val_proportion=0.0,
            epochs=200, batch_size=300, check_every=1000, lambda1=0, rng=None):
        return fit_navar_lstm_baselines([self], [save_path], [X_train], criterion, [optimizer],
                                        X_vals=None if X_val is None else [X_val], val_proportion=val_proportion,
                                        epochs=epochs, batch_size=batch_size, check_every=check_every, lambda1=lambda1,
                                        rngs=None if rng is None else [rng], verbose=1)[0]


def _fit_generic(model, save_path, X_train, criterion, optimizer, X_val, val_proportion, epochs, batch_size,
                 check_every, lambda1, rng, verbose):
    dev, dt = model.biases.device, model.biases.dtype
    X_train = torch.from_numpy(np.swapaxes(X_train, 2, 1)).to(dev, dt)
    if X_val is not None:
        X_val = torch.from_numpy(np.swapaxes(X_val, 2, 1)).to(dev, dt)
    n = X_train.size()[0]
    total_loss, loss_val, batch_counter = 0, 0, 0
    history = []
    # a fit leaves the model in eval mode (as the reference); a further fit of it trains again, and the
    # GPU's fused LSTM backward refuses a module in eval mode
    model.train()
    for t in range(1, epochs + 1):
        _, batches = _epoch_batches(rng, n, batch_size)
        for idx in batches:
            batch_counter += 1
            idx = torch.as_tensor(idx, device=dev, dtype=torch.long)
            xb = X_train[idx]
            X_batch, Y_batch = xb[:, :, :-1], xb[:, :, -1]
            predictions, contributions = model.forward(X_batch)
            loss_pred = criterion(predictions[:, :, -1], Y_batch)
            loss_l1 = (lambda1 / model.num_nodes) * torch.mean(torch.sum(torch.abs(contributions), dim=1))
            loss = loss_pred + loss_l1
            total_loss = total_loss + loss.detach()
            history.append((loss_pred.detach(), loss_l1.detach()))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        if t % check_every == 0:
            model.eval()
            if val_proportion > 0.0 and X_val is not None:
                with torch.no_grad():
                    val_pred, _ = model.forward(X_val[:, :, :-1])
                    loss_val = criterion(val_pred[:, :, -1], X_val[:, :, -1])  # the reference's line cannot broadcast
            model.train()
            if verbose:
                print(f'iteration {t}. Loss: {total_loss / batch_counter}  Val loss: {loss_val}')
            total_loss, batch_counter = 0, 0
    model.eval()
    with torch.no_grad():
        _, contributions = model.forward(X_train[:, :, :-1])
        model.causal_matrix = torch.std(contributions, dim=0).view(model.num_nodes, model.num_nodes).detach().cpu().numpy()
    model.step_losses = (torch.stack([h[0] for h in history]).double().cpu().numpy() if history else np.zeros(0),
                         torch.stack([h[1] for h in history]).double().cpu().numpy() if history else np.zeros(0))
    _save(model, save_path)
    return loss_val


def fit_navar_lstm_baselines(models, save_paths, X_trains, criterion, optimizers, X_vals=None, val_proportion=0.0,
                             epochs=200, batch_size=300, check_every=1000, lambda1=0, rngs=None, verbose=0):
    """NAVARLSTM.fit (models/navar.py:181-246) for a list of models, each with its own data (n, T, N),
    optimizer, save_path and RNG (None: the global numpy.random module, as the reference).  Same-shape
    models with equal n on the fused route share one native call per epoch; otherwise one fit after
    the other.  Returns the fits' loss_val; every model's per-step (mse, l1) values are left in
    ``model.step_losses``."""
    R = len(models)
    X_vals = [None] * R if X_vals is None else list(X_vals)
    rngs = [None] * R if rngs is None else list(rngs)
    lams = list(lambda1) if isinstance(lambda1, (list, tuple)) else [lambda1] * R
    if not (len(save_paths) == len(X_trains) == len(optimizers) == len(X_vals) == len(rngs) == len(lams) == R) or R == 0:
        raise ValueError("fit_navar_lstm_baselines: one save_path, training set, optimizer and rng per model")
    rngs = [np.random if g is None else g for g in rngs]
    m0 = models[0]
    shape = lambda m: (m.num_nodes, m.num_hidden, m.hidden_layers)
    same = all(shape(m) == shape(m0) for m in models) and all(x.shape == X_trains[0].shape for x in X_trains) and \
        all((v is None) == (X_vals[0] is None) and (v is None or v.shape == X_vals[0].shape) for v in X_vals)
    n, T = int(X_trains[0].shape[0]), int(X_trains[0].shape[1])
    Bmax = min(int(batch_size), n)
    fused = same and R <= MAX_REPLICAS and n > 0 and T >= 2 and Bmax <= MAX_B and all(
        m.fused_eligible(criterion, optimizers[i], T=T, Bmax=Bmax) for i, m in enumerate(models)) and \
        len(set(id(m) for m in models)) == R
    if not fused:
        if R > 1:  # nothing to share: fit one after the other (each may still take the fused route)
            return [fit_navar_lstm_baselines([models[i]], [save_paths[i]], [X_trains[i]], criterion, [optimizers[i]],
                                             [X_vals[i]], val_proportion, epochs, batch_size, check_every, lams[i],
                                             [rngs[i]], verbose)[0] for i in range(R)]
        return [_fit_generic(m0, save_paths[0], X_trains[0], criterion, optimizers[0], X_vals[0], val_proportion, epochs,
                             batch_size, check_every, lams[0], rngs[0], verbose)]
    # ---------------------------------------------------------------- fused
    if R == 1:
        pack, r0 = m0._slot()
        rows = [r0]
    else:
        pack = NavarLstmPack(models)
        rows = list(range(R))
    dev = pack.device
    for i in range(R):
        pack.bind_optimizer(rows[i], optimizers[i])
        pack.lambda1[rows[i]] = float(lams[i])
    active = None if (R > 1 or pack.R == 1) else rows

    def upload(xs):
        xs = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in xs]
        if R == 1:  # the pack may hold other rows: a zero stride serves this model's row
            return xs[0].to(dev), 0
        X = torch.stack(xs).to(dev)
        return X, X[0].numel()
    Xtr, xps = upload(X_trains)
    do_val = val_proportion > 0.0 and X_vals[0] is not None
    if do_val:
        Xva, xps_va = upload(X_vals)
        yva = Xva[..., -1, :].reshape(R, -1, pack.N)
    ident = torch.arange(n, dtype=torch.int32, device=dev) if batch_size >= n else None
    mses, l1s = [], []
    loss_val = [0] * R
    checked = 0  # epochs whose losses a check has already reported
    for t in range(1, epochs + 1):
        if ident is None:
            perms = np.stack([g.choice(n, size=n, replace=False) for g in rngs]).astype(np.int32)
            perm = torch.from_numpy(perms if R > 1 else perms[0]).to(dev)
        else:
            perm = ident
        mse, l1 = pack.train(Xtr, xps, perm, n if (R > 1 and ident is None) else 0, n, Bmax, active=active)
        mses.append(mse)
        l1s.append(l1)
        if t % check_every == 0:
            if do_val:
                pred, _ = pack.forward(Xva, xps_va, 0, int(Xva.shape[-3]), active=active)
                loss_val = [torch.nn.functional.mse_loss(pred[i][:, :, -1], yva[i]) for i in range(R)]
            if verbose:
                since = (torch.cat(mses[checked:], 1) + torch.cat(l1s[checked:], 1)).double().cpu().numpy()
                for i in range(R):
                    print(f'iteration {t}. Loss: {since[i].mean()}  Val loss: {loss_val[i]}')
            checked = len(mses)
    _, contrib = pack.forward(Xtr, xps, 0, n, active=active)
    # one reduction per model, of the shape a single fit reduces: the same bits in a pack and alone
    causal = torch.stack([torch.std(contrib[i], dim=0) for i in range(R)]).cpu().numpy()
    M = torch.cat(mses, 1).double().cpu().numpy() if mses else np.zeros((R, 0))
    L = torch.cat(l1s, 1).double().cpu().numpy() if l1s else np.zeros((R, 0))
    for i, m in enumerate(models):
        m.causal_matrix = causal[i].reshape(pack.N, pack.N)
        m.step_losses = (M[i], L[i])
        _save(m, save_paths[i])
    return loss_val
