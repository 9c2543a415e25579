"""NAVAR (MLP), the additive forecasting baseline of the paper's comparison table (models/navar.py:9-125;
model type "NAVAR_CMLP", general_utils/model_utils.py:615-623 and :1011-1034).

N per-source networks Conv1d(K) -> clamp(min=0) -> [Conv1d(H) -> clamp] -> Conv1d(H) whose N x N
contributions are summed over the sources into one prediction; the loss is criterion(pred, y) +
(lambda1 / N) * mean_b sum_c |contributions|; the causal matrix is the standard deviation of the
contributions over the training set.

Two routes, chosen by ``REDCLIFF_NAVAR_PATH=fused|generic`` (default fused):

* fused -- ``redcliff_navar_run`` (csrc/rc_navar.hip): one native call per epoch enqueues every Adam
  step of the epoch; parameters and the optimizer's exp_avg / exp_avg_sq / step are views of one packed
  buffer per model; the training set is uploaded once, an epoch uploads its permutation only, the
  per-step losses stay on the device until a check epoch.  Taken when ``fused_eligible`` holds.
* generic -- the reference's loop over ``forward`` with torch autograd and the caller's optimizer;
  serves every other configuration and the CPU.

``fit_navar_baselines`` fits R same-shape models (e.g. the 15 fold fits of
train/NAVAR_CMLP_d4IC_BCTVgs1Parsim.py) with the replica on a grid axis; ``NAVAR.fit`` is that function
with lists of one.  NAVARLSTM (models/navar.py:129-246) is redcliff_amd.navar_lstm.
"""
import collections
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import packs

LDS_MAX_FLOATS = 40960  # RC_LDS_MAX_FLOATS
NV_BC, NV_SL, NV_MISC = 64, 32, 240  # csrc/rc_navar.h
MAX_REPLICAS = 256
TRAIN, FORWARD = 0, 1


def navar_path():
    """'fused' (default) or 'generic', from REDCLIFF_NAVAR_PATH."""
    return packs.route_from_env("REDCLIFF_NAVAR_PATH")


def navar_lds_floats(N, H, K, layers=1, Bmax=1, T=None, R=1):
    """rc_navar_lds_floats (csrc/rc_navar.h) restated: the workgroup's LDS floats, 0 outside the limits."""
    T = K + 1 if T is None else T
    if min(N, H, K, Bmax, T, R) < 1:
        return 0
    if N > 32 or H > 512 or K > 64 or Bmax > 512 or R > MAX_REPLICAS or layers not in (1, 2) or T < K + 1:
        return 0
    Kp, Np = K | 1, N | 1
    big = 128 * (((H + 15) // 16 * 16) | 1) if layers == 2 else 32 * Kp
    f = NV_BC * Kp + 2 * NV_BC * 33 + 66 * N + 2 * NV_BC * Np + NV_MISC + big
    return f if f <= LDS_MAX_FLOATS else 0


def navar_ws_floats(N, H, layers, B):
    """rc_navar_ws_floats: workspace floats of one stepped replica."""
    nS = (H + NV_SL - 1) // NV_SL
    return N * nS * B * N + (N * nS * B * H if layers == 2 else 0) + 32


def navar_dims(N, H, K, layers=1, Bmax=1, T=None, R=1):
    return nat.Dims(R=R, Bmax=Bmax, T=K + 1 if T is None else T, p=N, L=K, K=1, h=H, F=K, n=layers, H=1, M1=1, nsup=0,
                    use_sigmoid=0, sigmoid_ecc=0.0)


def navar_supported(N, H, K, layers=1, Bmax=1, T=None, R=1):
    """redcliff_navar_supported: the footprint in floats, 0 outside the limits."""
    d = navar_dims(N, H, K, layers, Bmax, T, R)
    return int(nat.lib().redcliff_navar_supported(ctypes.byref(d)))


def navar_layout(N, H, K, layers):
    """[(name, offset, shape)] of the packed block and its size (rc_navar_off)."""
    out, at = [], 0
    shapes = [("W1", (N * H, 1, K)), ("b1", (N * H,))]
    if layers == 2:
        shapes += [("W2", (N * H, 1, H)), ("b2", (N * H,))]
    shapes += [("Wc", (N * N, 1, H)), ("bc", (N * N,)), ("biases", (1, N))]
    for name, shp in shapes:
        out.append((name, at, shp))
        at += int(np.prod(shp))
    return out, at


def _run(Args, entry, d, mode, B, tB, row0, n, nX, X, x_pstride, perm, perm_pstride, par, par_m, par_v, par_stride, hyper,
         mse, l1, pred, contrib, ws, replicas, stream, launches):
    """The native call `entry` of the NAVAR family (RedcliffNavarArgs and RedcliffNavarLstmArgs have the
    same fields) on device tensors (None = a null pointer); returns its code."""
    p_ = nat.ptr
    a = Args()
    a.d = d
    a.launches = int(launches)  # profiling: a mask of the step's launches (0 = all)
    a.mode, a.B, a.tB, a.row0, a.N, a.nX = int(mode), int(B), int(tB), int(row0), int(n), int(nX)
    a.X, a.x_pstride, a.perm, a.perm_pstride = p_(X), int(x_pstride), p_(perm), int(perm_pstride)
    a.par, a.par_m, a.par_v, a.par_stride, a.hyper = p_(par), p_(par_m), p_(par_v), int(par_stride), p_(hyper)
    a.mse, a.l1, a.pred, a.contrib = p_(mse), p_(l1), p_(pred), p_(contrib)
    a.ws, a.ws_bytes = p_(ws), 0 if ws is None else ws.numel() * 4
    keep = nat.replica_list(a, replicas)  # a local, so alive until the call has returned
    return getattr(nat.lib(), entry)(ctypes.byref(a), nat.stream_or_current(stream))


def navar_run(d, mode, B, tB, row0, n, nX, X, x_pstride, perm, perm_pstride, par, par_m, par_v, par_stride, hyper,
              mse, l1, pred, contrib, ws, replicas=None, stream=None, launches=0):
    """redcliff_navar_run on device tensors (None = a null pointer); returns its code.  `launches` masks the
    step's three launches."""
    return _run(nat.NavarArgs, "redcliff_navar_run", d, mode, B, tB, row0, n, nX, X, x_pstride, perm, perm_pstride, par,
                par_m, par_v, par_stride, hyper, mse, l1, pred, contrib, ws, replicas, stream, launches)


# --------------------------------------------------------------------------------------------------
class NavarPack(packs.AdamPack):
    """R same-shape NAVAR models on the fused route (packs.AdamPack): parameters by navar_layout, the
    replica's hyper-parameter beside Adam is c_adj = lambda1."""

    def __init__(self, models):
        m0 = models[0]
        self.N, self.H, self.K, self.layers = m0.num_nodes, m0.num_hidden, m0.maxlags, m0.hidden_layers
        for m in models:
            if (m.num_nodes, m.num_hidden, m.maxlags, m.hidden_layers) != (self.N, self.H, self.K, self.layers):
                raise ValueError("a NavarPack holds models of one shape")
        if not navar_supported(self.N, self.H, self.K, self.layers, R=len(models)):
            nat.check(-2, "navar_supported")
        if not m0.biases.is_cuda:
            raise RuntimeError("NAVAR (fused) runs on the MI355X only (HIP kernels); move the model to 'cuda'")
        self.layout, self.n = navar_layout(self.N, self.H, self.K, self.layers)
        self.allocate(models, self.n, m0.biases.device)
        self.lambda1 = [0.0] * self.R
        for r, mod in enumerate(self.models):
            prms = mod.packed_parameters()
            packs.pack_by_layout(self.par[r], prms, self.layout)
            self.adopt(r, prms)

    def replica_terms(self, r):
        return {"c_adj": float(self.lambda1[r])}

    def workspace(self, B, nrep):
        return self.workspace_of(navar_ws_floats(self.N, self.H, self.layers, B) * max(nrep, 1))

    def dims(self, B, T):
        return navar_dims(self.N, self.H, self.K, self.layers, Bmax=int(B), T=int(T), R=self.R)

    def train(self, X, x_pstride, perm, perm_pstride, n, B, active=None, ws=None):
        """One TRAIN call: ceil(n / B) Adam steps over perm[0 .. n) for the replicas `active` (None:
        all).  X (.., nX, T, N) float32, perm int32 on the device.  Returns (mse, l1) device tensors
        [stepped][nsteps]."""
        reps = self.reps(active)
        nsteps = -(-int(n) // int(B))
        mse = torch.empty(len(reps), nsteps, device=self.device, dtype=torch.float32)
        l1 = torch.empty_like(mse)
        if not reps or n == 0:
            return mse, l1
        self.require_optimizers(reps)
        t_base = self.opt[reps[0]]["t"]
        T, nX = int(X.shape[-2]), int(X.shape[-3])
        ws = self.workspace(B, len(reps)) if ws is None else ws
        rc = navar_run(self.dims(B, T), TRAIN, B, t_base + 1, 0, n, nX, X, x_pstride, perm, perm_pstride, self.par,
                       self.m, self.v, self.n, self.hyper(t_base, reps), mse, l1, None, None, ws,
                       None if active is None else reps)
        nat.check(rc, "navar_run")
        self.advance(reps, nsteps)
        return mse, l1

    def forward(self, X, x_pstride, row0, n, active=None, B=None, ws=None):
        """One FORWARD call over rows [row0, row0 + n): (pred [stepped][n][N], contrib [stepped][n][N*N])."""
        reps = self.reps(active)
        pred = torch.empty(len(reps), n, self.N, device=self.device, dtype=torch.float32)
        contrib = torch.empty(len(reps), n, self.N * self.N, device=self.device, dtype=torch.float32)
        if not reps or n == 0:
            return pred, contrib
        B = min(512, int(n)) if B is None else int(B)
        T, nX = int(X.shape[-2]), int(X.shape[-3])
        ws = self.workspace(B, len(reps)) if ws is None else ws
        rc = navar_run(self.dims(B, T), FORWARD, B, 1, row0, n, nX, X, x_pstride, None, 0, self.par, None, None, self.n,
                       None, None, None, pred, contrib, ws, None if active is None else reps)
        nat.check(rc, "navar_run")
        return pred, contrib


# --------------------------------------------------------------------------------------------------
def _plain_fit(model, criterion, optimizer):
    """The loss and the optimizer (when given) are the ones the family's fused steps implement: mean MSE,
    and packs.plain_adam over the model's parameters."""
    if criterion is not None and not packs.mean_mse(criterion):
        return False
    return optimizer is None or packs.plain_adam(optimizer, list(model.parameters()))


class NAVAR(packs.PackSlot, nn.Module):
    _slot_key, _pack_class = "_nv_slot", NavarPack

    def __init__(self, num_nodes, num_hidden, maxlags, hidden_layers=1, dropout=0):
        super().__init__()
        self.num_nodes = num_nodes
        self.num_hidden = num_hidden
        self.maxlags = maxlags
        self.hidden_layers = hidden_layers
        self.dropout_p = dropout
        self.first_hidden_layer = nn.Conv1d(num_nodes, num_hidden * num_nodes, kernel_size=maxlags, groups=num_nodes)
        self.dropout = nn.Dropout(p=dropout)
        self.hidden_layer_list = nn.ModuleList()
        self.dropout_list = nn.ModuleList()
        for _ in range(hidden_layers - 1):
            self.hidden_layer_list.append(nn.Conv1d(num_nodes, num_hidden * num_nodes, kernel_size=num_hidden,
                                                    groups=num_nodes))
            self.dropout_list.append(nn.Dropout(p=dropout))
        self.contributions = nn.Conv1d(num_nodes, num_nodes * num_nodes, kernel_size=num_hidden, groups=num_nodes)
        self.biases = nn.Parameter(torch.ones(1, num_nodes) * 0.0001)
        self.causal_matrix = None

    def forward(self, x):
        """x (B, N, K) -> (predictions (B, N), contributions (B, N*N, 1)); channel i*N + j is the
        contribution of source i to target j."""
        N, H = self.num_nodes, self.num_hidden
        hidden = self.first_hidden_layer(x).clamp(min=0).transpose(-1, -2).reshape([-1, N, H])
        hidden = self.dropout(hidden)
        for layer, drop in zip(self.hidden_layer_list, self.dropout_list):
            hidden = drop(layer(hidden).clamp(min=0).view([-1, N, H]))
        contributions = self.contributions(hidden).view([-1, N, N, 1])
        predictions = torch.sum(contributions, dim=1)[:, :, 0] + self.biases
        return predictions, contributions.view([-1, N * N, 1])

    def GC(self):
        return self.causal_matrix

    # ------------------------------------------------------------------ route
    def packed_parameters(self):
        """The parameters in the packed layout's order."""
        out = [self.first_hidden_layer.weight, self.first_hidden_layer.bias]
        for layer in self.hidden_layer_list:
            out += [layer.weight, layer.bias]
        return out + [self.contributions.weight, self.contributions.bias, self.biases]

    def fused_eligible(self, criterion=None, optimizer=None, T=None, Bmax=1, split_timeseries=False):
        """The fused route serves this model (and, when given, this loss, optimizer and window shape)."""
        if navar_path() != "fused":
            return False
        if self.dropout_p != 0 or self.hidden_layers not in (1, 2) or split_timeseries:
            return False
        if T is not None and T - 1 != self.maxlags:
            return False
        if not _plain_fit(self, criterion, optimizer):
            return False
        if not all(p.is_cuda and p.dtype == torch.float32 for p in self.parameters()):
            return False
        args = (self.num_nodes, self.num_hidden, self.maxlags, self.hidden_layers, int(Bmax), T)
        if not navar_lds_floats(*args):
            return False
        return navar_supported(*args) > 0

    def fit(self, save_path, X_train, Y_train, criterion, optimizer, X_val=None, Y_val=None, val_proportion=0.0,
            epochs=200, batch_size=300, split_timeseries=False, check_every=1000, lambda1=0, rng=None):
        return fit_navar_baselines([self], [save_path], [X_train], criterion, [optimizer],
                                   X_vals=None if X_val is None else [X_val], val_proportion=val_proportion,
                                   epochs=epochs, batch_size=batch_size, check_every=check_every, lambda1=lambda1,
                                   rngs=None if rng is None else [rng], split_timeseries=split_timeseries, verbose=1)[0]


def _standalone(model):
    from .fit_loop import standalone_copy
    return standalone_copy(model)


def _epoch_batches(rng, n, batch_size):
    """The reference's per-epoch batching (models/navar.py:78-87): (permutation or None, index arrays)."""
    if batch_size < n:
        perm = rng.choice(n, size=n, replace=False)
        out = []
        for i in range(int(n / batch_size) + 1):
            b = perm[i * batch_size:(i + 1) * batch_size]
            if len(b) > 0:
                out.append(b)
        return perm, out
    return None, [np.arange(n)]


def _save(model, save_path):
    torch.save(_standalone(model), os.path.join(save_path, "final_best_model.bin"))


# What tells the family's two members apart in the shared drivers: the driver's name (for its error text), the
# pack class, the shape key of models that share a pack, eligible(model, criterion, optimizer, T, Bmax,
# split_timeseries) with the member's own terms, and `recurrent`: predictions carry a time axis whose last
# step is the forecast, the data is cast to the model's dtype and a fit starts by model.train() (a fit
# leaves the model in eval mode, as the reference; the GPU's fused LSTM backward refuses such a module).
_Family = collections.namedtuple("_Family", "name pack shape eligible recurrent")


def _fit_generic(fam, model, save_path, X_train, criterion, optimizer, X_val, val_proportion, epochs, batch_size,
                 split_timeseries, check_every, lambda1, rng, verbose):
    """The reference's loop (models/navar.py:57-125 and :181-246) with torch autograd and the caller's optimizer."""
    dev, dt = model.biases.device, model.biases.dtype if fam.recurrent else None
    forecast = (lambda pred: pred[:, :, -1]) if fam.recurrent else (lambda pred: pred)
    X_train = torch.from_numpy(np.swapaxes(X_train, 2, 1)).to(dev, dt)
    if X_val is not None:
        X_val = torch.from_numpy(np.swapaxes(X_val, 2, 1)).to(dev, dt)
    n = X_train.size()[0]
    total_loss, loss_val, batch_counter = 0, 0, 0
    history = []
    if fam.recurrent:
        model.train()
    for t in range(1, epochs + 1):
        _, batches = _epoch_batches(rng, n, batch_size)
        for idx in batches:
            batch_counter += 1
            idx = torch.as_tensor(idx, device=dev, dtype=torch.long)
            xb = X_train[idx]
            X_batch, Y_batch = xb[:, :, :-1], xb[:, :, -1]
            predictions, contributions = model.forward(X_batch)
            if not split_timeseries:
                loss_pred = criterion(forecast(predictions), Y_batch)
            else:
                loss_pred = criterion(predictions[:, :, -1], Y_batch[:, :, -1])
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
                    # (NAVARLSTM: the reference's line compares (n, N, T') with (n, N) and cannot broadcast)
                    loss_val = criterion(forecast(val_pred), X_val[:, :, -1])
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


def _fit_navar_family(fam, models, save_paths, X_trains, criterion, optimizers, X_vals, val_proportion, epochs,
                      batch_size, check_every, lambda1, rngs, verbose, split_timeseries):
    """The fit of the reference's NAVAR and NAVARLSTM (models/navar.py:57-125 and :181-246) for a list of
    models of the member `fam`, each with its own data (n, T, N), optimizer, save_path and RNG (None: the
    global numpy.random module, as the reference).  Same-shape models with equal n on the fused route share
    one native call per epoch; otherwise one fit after the other.  Returns the fits' loss_val; every model's
    per-step (mse, l1) values are left in ``model.step_losses``."""
    R = len(models)
    X_vals = [None] * R if X_vals is None else list(X_vals)
    rngs = [None] * R if rngs is None else list(rngs)
    lams = list(lambda1) if isinstance(lambda1, (list, tuple)) else [lambda1] * R
    if not (len(save_paths) == len(X_trains) == len(optimizers) == len(X_vals) == len(rngs) == len(lams) == R) or R == 0:
        raise ValueError("%s: one save_path, training set, optimizer and rng per model" % fam.name)
    rngs = [np.random if g is None else g for g in rngs]
    m0 = models[0]
    same = all(fam.shape(m) == fam.shape(m0) for m in models) and all(x.shape == X_trains[0].shape for x in X_trains) and \
        all((v is None) == (X_vals[0] is None) and (v is None or v.shape == X_vals[0].shape) for v in X_vals)
    n, T = int(X_trains[0].shape[0]), int(X_trains[0].shape[1])
    Bmax = min(int(batch_size), n)
    fused = same and R <= MAX_REPLICAS and n > 0 and all(
        fam.eligible(m, criterion, optimizers[i], T, Bmax, split_timeseries) for i, m in enumerate(models)) and \
        len(set(id(m) for m in models)) == R
    if not fused:
        if R > 1:  # nothing to share: fit one after the other (each may still take the fused route)
            return [_fit_navar_family(fam, [models[i]], [save_paths[i]], [X_trains[i]], criterion, [optimizers[i]],
                                      [X_vals[i]], val_proportion, epochs, batch_size, check_every, lams[i], [rngs[i]],
                                      verbose, split_timeseries)[0] for i in range(R)]
        return [_fit_generic(fam, m0, save_paths[0], X_trains[0], criterion, optimizers[0], X_vals[0], val_proportion,
                             epochs, batch_size, split_timeseries, check_every, lams[0], rngs[0], verbose)]
    # ---------------------------------------------------------------- fused
    pack, rows, active = packs.acquire(models, optimizers, fam.pack)
    dev = pack.device
    for i in range(R):
        pack.lambda1[rows[i]] = float(lams[i])
    forecast = (lambda pred: pred[:, :, -1]) if fam.recurrent else (lambda pred: pred)

    def upload(xs):
        return packs.stack_upload([torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in xs], dev)
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
                loss_val = [torch.nn.functional.mse_loss(forecast(pred[i]), yva[i]) for i in range(R)]
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


_MLP = _Family("fit_navar_baselines", NavarPack, lambda m: (m.num_nodes, m.num_hidden, m.maxlags, m.hidden_layers),
               lambda m, criterion, optimizer, T, Bmax, split: m.fused_eligible(criterion, optimizer, T=T, Bmax=Bmax,
                                                                                split_timeseries=split), False)


def fit_navar_baselines(models, save_paths, X_trains, criterion, optimizers, X_vals=None, val_proportion=0.0, epochs=200,
                        batch_size=300, check_every=1000, lambda1=0, rngs=None, verbose=0, split_timeseries=False):
    """NAVAR.fit (models/navar.py:57-125) for a list of models: _fit_navar_family."""
    return _fit_navar_family(_MLP, models, save_paths, X_trains, criterion, optimizers, X_vals, val_proportion, epochs,
                             batch_size, check_every, lambda1, rngs, verbose, split_timeseries)
