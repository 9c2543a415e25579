"""DGCNN modules with the parameter tree of torcheeg 1.1.3 ``DGCNN`` and of the reference's
``DGCNN_Model`` wrapper (models/dgcnn.py), and the supervised DGCNN baseline's fit.

Inside a REDCLIFF-S model the DGCNN is the factor-score embedder: only the parameter tree and the
initialisation order matter there (a seeded model is identical to the reference's) and the arithmetic
runs in the gfx950 kernels of csrc/rc_embed.hip, driven by redcliff_amd.engine.  Keys produced by
``state_dict()``: ``dgcnn.A``, ``dgcnn.layer1.gc1.{i}.weight``, ``dgcnn.BN1.*``, ``dgcnn.fc1.linear.*``,
``dgcnn.fc2.linear.*`` -- identical to the reference checkpoints.

``DGCNN_Model`` is also the paper's supervised baseline (model type "DGCNN",
general_utils/model_utils.py:574-583 and :950-985; models/dgcnn.py:63-237).  Its fit has two routes,
chosen by ``REDCLIFF_DGCNN_PATH=fused|generic`` (default fused):

* fused -- ``redcliff_dgcnn_fit_run`` (csrc/rc_dgcnn_fit.hip): one native call per epoch enqueues every
  Adam step of the epoch; parameters, the optimizer's exp_avg / exp_avg_sq / step and the BatchNorm
  running statistics are views of one packed buffer per model; both loaders are iterated once,
  label-selected and uploaded once (a shuffling loader is replayed in its first epoch's order); the
  per-step losses stay on the device until a check epoch.  Taken when ``fused_eligible`` holds.
* generic -- the reference's loop over ``batch_update`` with torch autograd and the caller's optimizer;
  serves every other configuration and the CPU.

``fit_dgcnn_baselines`` fits R same-shape models with the replica on a grid axis; ``DGCNN_Model.fit``
is that function with lists of one.
"""
import ctypes
import os
import pickle as pkl

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F_

from . import _native as nat
from . import packs

M1 = 64  # torcheeg DGCNN fc1 width

LDS_MAX_FLOATS = 40960  # RC_LDS_MAX_FLOATS
DG_BC, DG_MISC = 32, 256  # csrc/rc_dgcnn_fit.h
MAX_REPLICAS = 256
TRAIN, FORWARD = 0, 1


class GraphConvolution(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        nn.init.xavier_normal_(self.weight)
        self.bias = None


class Chebynet(nn.Module):
    def __init__(self, in_channels, num_layers, out_channels):
        super().__init__()
        self.num_layers = num_layers
        self.gc1 = nn.ModuleList([GraphConvolution(in_channels, out_channels) for _ in range(num_layers)])


class Linear(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.linear = nn.Linear(in_channels, out_channels)
        nn.init.xavier_normal_(self.linear.weight)
        nn.init.zeros_(self.linear.bias)


def normalize_A(A):
    """torcheeg normalize_A (symmetry=False): D^-1/2 relu(A) D^-1/2 with the 1e-10 guard."""
    A = F_.relu(A)
    d = 1 / torch.sqrt(torch.sum(A, 1) + 1e-10)
    D = torch.diag_embed(d)
    return torch.matmul(torch.matmul(D, A), D)


class DGCNN(nn.Module):
    """torcheeg.models.DGCNN(in_channels, num_electrodes, num_layers, hid_channels, num_classes).

    Registration order (= RNG order): layer1 (Chebynet), BN1, fc1, fc2, A."""

    def __init__(self, in_channels=5, num_electrodes=62, num_layers=2, hid_channels=32, num_classes=2):
        super().__init__()
        self.in_channels = in_channels
        self.num_electrodes = num_electrodes
        self.num_layers = num_layers
        self.hid_channels = hid_channels
        self.num_classes = num_classes
        self.layer1 = Chebynet(in_channels, num_layers, hid_channels)
        self.BN1 = nn.BatchNorm1d(in_channels)
        self.fc1 = Linear(num_electrodes * hid_channels, M1)
        self.fc2 = Linear(M1, num_classes)
        self.A = nn.Parameter(torch.empty(num_electrodes, num_electrodes))
        nn.init.xavier_normal_(self.A)

    def forward(self, x):
        """x (B, num_electrodes, in_channels) -> (B, num_classes), in plain torch (any device / dtype).
        Support 0 is the identity: x itself stands for I x.  With one layer A is not used at all."""
        x = self.BN1(x.transpose(1, 2)).transpose(1, 2)
        result, S, L = None, None, None
        for i, gc in enumerate(self.layer1.gc1):
            if i == 0:
                t = x
            else:
                if i == 1:
                    L = normalize_A(self.A)
                    S = L
                else:
                    S = torch.matmul(S, L)
                t = torch.matmul(S, x)
            o = torch.matmul(t, gc.weight)
            result = o if result is None else result + o
        result = F_.relu(result).reshape(x.shape[0], -1)
        return self.fc2.linear(F_.relu(self.fc1.linear(result)))


# --------------------------------------------------------------------------------------------------
def dgcnn_path():
    """'fused' (default) or 'generic', from REDCLIFF_DGCNN_PATH."""
    return packs.route_from_env("REDCLIFF_DGCNN_PATH")


def select_labels(Y, num_features):
    """The labels batch_update / training_eval compare against (models/dgcnn.py:81-91)."""
    if Y.dim() == 3:
        if Y.size()[2] > num_features:
            return Y[:, :, num_features]
        assert Y.size()[2] == 1
        return Y[:, :, 0]
    if Y.dim() == 2:
        return Y
    raise NotImplementedError("Cannot handle ground-truth labels with Y.size() == " + str(Y.size()))


def dgcnn_fit_lds_floats(n, F, layers, H, C, Bmax=1, T=None, R=1):
    """rc_dgcnn_lds_floats (csrc/rc_dgcnn_fit.h) restated: the workgroup's LDS floats, 0 outside the limits."""
    T = F if T is None else T
    if min(n, F, layers, H, C, Bmax, T, R) < 1:
        return 0
    if n > 32 or F > 8 or layers > 4 or H > 256 or C > 16 or Bmax > 128 or R > MAX_REPLICAS or T < F:
        return 0
    Hp, nq = H | 1, layers * F
    node = (DG_MISC + Bmax * 65 + Bmax * C + C * M1 + M1 * Hp + DG_BC * Hp + DG_BC * F * n + 3 * DG_BC * nq + n * n +
            layers * n + nq * Hp)
    tail = DG_MISC + (2 * layers + 3) * n * n
    f = max(node, tail)
    return f if f <= LDS_MAX_FLOATS else 0


def dgcnn_fit_ws_floats(n, F, layers, H, C, B, N):
    """rc_dgcnn_ws(...).total: workspace floats of one stepped replica for a call over N rows."""
    nsteps = -(-int(N) // int(B))
    x = 4 * F * nsteps + n * B * M1 + n * B * H + n * layers * F * H + layers * n * n + n * 2 * F + C * M1 + C + M1
    return (x + 63) & ~63


def dgcnn_fit_dims(n, F, layers, H, C, Bmax=1, T=None, R=1):
    return nat.Dims(R=R, Bmax=Bmax, T=F if T is None else T, p=n, L=1, K=C, h=1, F=F, n=layers, H=H, M1=M1, nsup=0,
                    use_sigmoid=0, sigmoid_ecc=0.0)


def dgcnn_fit_supported(n, F, layers, H, C, Bmax=1, T=None, R=1):
    """redcliff_dgcnn_fit_supported: the footprint in floats, 0 outside the limits."""
    d = dgcnn_fit_dims(n, F, layers, H, C, Bmax, T, R)
    return int(nat.lib().redcliff_dgcnn_fit_supported(ctypes.byref(d)))


def dgcnn_fit_layout(n, F, layers, H, C):
    """[(name, offset, shape)] of the packed block and its size (rc_emb_off with M1 = 64)."""
    out, at = [], 0
    shapes = [("A", (n, n))] + [("gc%d" % i, (F, H)) for i in range(layers)]
    shapes += [("bn_w", (F,)), ("bn_b", (F,)), ("fc1W", (M1, n * H)), ("fc1b", (M1,)), ("fc2W", (C, M1)), ("fc2b", (C,))]
    for name, shp in shapes:
        out.append((name, at, shp))
        at += int(np.prod(shp))
    return out, at


def dgcnn_fit_run(d, mode, B, tB, row0, n, nX, X, x_pstride, Y, y_pstride, par, par_m, par_v, par_stride, bn_rm, bn_rv,
                  hyper, loss, pred, ws, replicas=None, stream=None, launches=0):
    """redcliff_dgcnn_fit_run on device tensors (None = a null pointer); returns its code."""
    p_ = nat.ptr
    a = nat.DgcnnFitArgs()
    a.d = d
    a.launches = int(launches)  # profiling: a mask of the step's three launches (0 = all)
    a.mode, a.B, a.tB, a.row0, a.N, a.nX = int(mode), int(B), int(tB), int(row0), int(n), int(nX)
    a.X, a.x_pstride, a.Y, a.y_pstride = p_(X), int(x_pstride), p_(Y), int(y_pstride)
    a.par, a.par_m, a.par_v, a.par_stride = p_(par), p_(par_m), p_(par_v), int(par_stride)
    a.bn_rm, a.bn_rv, a.hyper, a.loss, a.pred = p_(bn_rm), p_(bn_rv), p_(hyper), p_(loss), p_(pred)
    a.ws, a.ws_bytes = p_(ws), 0 if ws is None else ws.numel() * 4
    keep = nat.replica_list(a, replicas)  # a local, so alive until the call has returned
    return nat.lib().redcliff_dgcnn_fit_run(ctypes.byref(a), nat.stream_or_current(stream))


# --------------------------------------------------------------------------------------------------
class DgcnnFitPack(packs.AdamPack):
    """R same-shape DGCNN_Model baselines on the fused route (packs.AdamPack): parameters by dgcnn_fit_layout,
    and beside them the BatchNorm running statistics as views of rm[r] / rv[r] (`bound` watches these too);
    the replica's hyper-parameters beside Adam are BN1's eps and momentum."""

    def __init__(self, models):
        m0 = models[0]
        self.shape = m0.fit_shape()
        for m in models:
            if m.fit_shape() != self.shape:
                raise ValueError("a DgcnnFitPack holds models of one shape")
        self.n, self.F, self.layers, self.H, self.C = self.shape
        if not dgcnn_fit_supported(*self.shape, R=len(models)):
            nat.check(-2, "dgcnn_fit_supported")
        if not m0.dgcnn.A.is_cuda:
            raise RuntimeError("DGCNN_Model (fused) runs on the MI355X only (HIP kernels); move the model to 'cuda'")
        self.layout, size = dgcnn_fit_layout(*self.shape)
        self.allocate(models, size, m0.dgcnn.A.device)
        self.rm = torch.empty(self.R, self.F, device=self.device, dtype=torch.float32)
        self.rv = torch.empty_like(self.rm)
        for r, mod in enumerate(self.models):
            prms = mod.packed_parameters()
            packs.pack_by_layout(self.par[r], prms, self.layout)
            packs.adopt_bn_stats(mod.dgcnn.BN1, self.rm[r], self.rv[r])
            self.adopt(r, prms)

    def extra_pointers(self, r):
        bn = self.models[r].dgcnn.BN1
        return [bn.running_mean.data_ptr(), bn.running_var.data_ptr()]

    def stepped_parameters(self, r):
        """All of them, but A with one layer (it has no gradient)."""
        return self.params[r][1:] if self.layers == 1 else self.params[r]

    def replica_terms(self, r):
        bn = self.models[r].dgcnn.BN1
        return {"bn_eps": float(bn.eps), "bn_momentum": float(bn.momentum)}

    def workspace(self, B, n, nrep):
        return self.workspace_of(dgcnn_fit_ws_floats(*self.shape, B, n) * max(nrep, 1))

    def dims(self, B, T):
        return dgcnn_fit_dims(*self.shape, Bmax=int(B), T=int(T), R=self.R)

    def train(self, X, x_pstride, Y, y_pstride, row0, n, B, active=None, ws=None, launches=0):
        """One TRAIN call: ceil(n / B) Adam steps over rows [row0, row0 + n) for the replicas `active`
        (None: all).  X (.., nX, T, nodes), Y (.., nX, C) float32 on the device.  Returns the steps'
        losses, a device tensor [stepped][nsteps]."""
        reps = self.reps(active)
        nsteps = -(-int(n) // int(B))
        loss = torch.empty(len(reps), nsteps, device=self.device, dtype=torch.float32)
        if not reps or n == 0:
            return loss
        self.require_optimizers(reps)
        t_base = self.opt[reps[0]]["t"]
        T, nX = int(X.shape[-2]), int(X.shape[-3])
        ws = self.workspace(B, n, len(reps)) if ws is None else ws
        rc = dgcnn_fit_run(self.dims(B, T), TRAIN, B, t_base + 1, row0, n, nX, X, x_pstride, Y, y_pstride, self.par, self.m,
                           self.v, self.np_, self.rm, self.rv, self.hyper(t_base, reps), loss, None, ws,
                           None if active is None else reps, launches=launches)
        nat.check(rc, "dgcnn_fit_run")
        self.advance(reps, nsteps)
        for r in reps:
            self.models[r].dgcnn.BN1.num_batches_tracked += nsteps
        return loss

    def forward(self, X, x_pstride, Y, y_pstride, row0, n, B, active=None, ws=None):
        """One FORWARD call (eval mode) over rows [row0, row0 + n) in batches of B: (pred [stepped][n][C],
        per-batch MSE [stepped][nbatches] or None without labels)."""
        reps = self.reps(active)
        nb = -(-int(n) // int(B))
        pred = torch.empty(len(reps), n, self.C, device=self.device, dtype=torch.float32)
        mse = None if Y is None else torch.empty(len(reps), nb, device=self.device, dtype=torch.float32)
        if not reps or n == 0:
            return pred, mse
        T, nX = int(X.shape[-2]), int(X.shape[-3])
        ws = self.workspace(B, n, len(reps)) if ws is None else ws
        rc = dgcnn_fit_run(self.dims(B, T), FORWARD, B, 1, row0, n, nX, X, x_pstride, Y, y_pstride, self.par, None, None,
                           self.np_, self.rm, self.rv, self.hyper(0, ()), mse, pred, ws, None if active is None else reps)
        nat.check(rc, "dgcnn_fit_run")
        return pred, mse


# --------------------------------------------------------------------------------------------------
class DGCNN_Model(packs.PackSlot, nn.Module):
    """models/dgcnn.py:15-237: the DGCNN wrapper REDCLIFF-S embeds, and the supervised baseline with the
    reference's forward / batch_update / training_eval / save_checkpoint / fit (see the module docstring
    for the fit's two routes)."""
    _slot_key, _pack_class = "_dg_slot", DgcnnFitPack

    def __init__(self, num_channels, num_wavelets_per_chan, num_features_per_node, num_graph_conv_layers,
                 num_hidden_nodes, num_classes):
        super().__init__()
        self.num_channels = num_channels
        self.num_wavelets_per_chan = num_wavelets_per_chan
        self.num_nodes = num_channels * num_wavelets_per_chan
        self.num_features_per_node = num_features_per_node
        self.num_graph_conv_layers = num_graph_conv_layers
        self.num_hidden_nodes = num_hidden_nodes
        self.num_classes = num_classes
        self.supervised_loss_fn = nn.MSELoss(reduction="mean")
        self.dgcnn = DGCNN(num_features_per_node, self.num_nodes, num_graph_conv_layers, num_hidden_nodes, num_classes)

    def GC(self, threshold=True, combine_node_feature_edges=False):
        """models/dgcnn.py:47-61: raw A^T; with combine=True the Frobenius norm of each
        1x1 (wavelet) block, i.e. |A|^T."""
        G = self.dgcnn.A
        if combine_node_feature_edges:
            w = self.num_wavelets_per_chan
            if w == 1:
                G = torch.abs(G)
            else:
                p = self.num_channels
                G = torch.linalg.vector_norm(G.reshape(p, w, p, w), dim=(1, 3))
        G = G.T
        return (G > 0).int() if threshold else G

    def forward(self, X):
        return self.dgcnn(X)

    # ------------------------------------------------------------------ the reference's steps (generic route)
    def _inputs(self, X, Y):
        prm = self.dgcnn.A
        X = X.to(device=prm.device, dtype=prm.dtype)
        Y = Y.to(device=prm.device, dtype=prm.dtype)
        return torch.transpose(X[:, :self.num_features_per_node, :], 1, 2), select_labels(Y, self.num_features_per_node)

    def batch_update(self, batch_num, X, Y, gen_optim, running_factor_loss):
        x, y = self._inputs(X, Y)
        self.dgcnn.train()
        gen_optim.zero_grad()
        factor_loss = self.supervised_loss_fn(self.forward(x), y)
        factor_loss.backward()
        gen_optim.step()
        return running_factor_loss + factor_loss.cpu().detach().item()

    def training_eval(self, val_loader):
        avg_factor_loss = 0.
        self.dgcnn.eval()
        with torch.no_grad():
            for X, Y in val_loader:
                x, y = self._inputs(X, Y)
                avg_factor_loss += self.supervised_loss_fn(self.forward(x), y).cpu().detach().item()
        return avg_factor_loss / len(val_loader)

    def save_checkpoint(self, save_dir, it, best_model, avg_factor_loss, best_loss, GC):
        """The two files of models/dgcnn.py:104-113 (the plots of :115-118 are not drawn, as in
        cMLP_FM.save_checkpoint)."""
        os.makedirs(save_dir, exist_ok=True)
        torch.save(_standalone(best_model) if isinstance(best_model, nn.Module) else best_model,
                   os.path.join(save_dir, "temp_best_model_epoch" + str(it) + ".bin"))
        with open(os.path.join(save_dir, "training_meta_data_and_hyper_parameters.pkl"), "wb") as outfile:
            pkl.dump({"epoch": it, "avg_factor_loss": avg_factor_loss, "best_loss": best_loss}, outfile)

    def stopping_criterion(self):
        """models/dgcnn.py:160-173: ||relu-mask(1.6 A^T / max(A^T))||_1, a 0-d tensor on the model's device."""
        g = self.GC(threshold=False, combine_node_feature_edges=False).detach()
        g = 1.6 * g / torch.max(g)
        g = g * (g >= 0.)
        return torch.norm(g, 1)

    # ------------------------------------------------------------------ route
    def fit_shape(self):
        return (self.num_nodes, self.num_features_per_node, self.num_graph_conv_layers, self.num_hidden_nodes,
                self.num_classes)

    def packed_parameters(self):
        """The parameters in the packed layout's order."""
        d = self.dgcnn
        return [d.A] + [gc.weight for gc in d.layer1.gc1] + [d.BN1.weight, d.BN1.bias, d.fc1.linear.weight,
                                                             d.fc1.linear.bias, d.fc2.linear.weight, d.fc2.linear.bias]

    def fused_eligible(self, optimizer=None, T=None, Bmax=1):
        """The fused route serves this model (and, when given, this optimizer, window length and batch size)."""
        if dgcnn_path() != "fused":
            return False
        bn = self.dgcnn.BN1
        if not packs.mean_mse(self.supervised_loss_fn):
            return False
        if not (bn.affine and bn.track_running_stats and bn.momentum is not None):
            return False
        if optimizer is not None:
            mine = list(self.dgcnn.parameters())
            if not packs.plain_adam(optimizer, mine) or len(optimizer.param_groups[0]["params"]) != len(mine):
                return False
        tensors = list(self.parameters()) + [bn.running_mean, bn.running_var]
        if not all(p.is_cuda and p.dtype == torch.float32 for p in tensors):
            return False
        args = self.fit_shape() + (int(Bmax), T)
        if not dgcnn_fit_lds_floats(*args):
            return False
        return dgcnn_fit_supported(*args) > 0

    def fit(self, save_dir, train_loader, gen_optim, max_iter, lookback, check_every, verbose, GC, val_loader):
        return fit_dgcnn_baselines([self], [save_dir], [train_loader], [gen_optim], max_iter, lookback, check_every, verbose,
                                   [GC], [val_loader])[0]


def _standalone(model):
    from .fit_loop import standalone_copy
    return standalone_copy(model)


def _restore_parameters(model, best_model):
    """general_utils/model_utils.py:309-313: parameters only (the running statistics stay); copied in
    place, so a packed model's views stay views."""
    with torch.no_grad():
        for prm, best in zip(model.parameters(), best_model.parameters()):
            prm.copy_(best)


def _criterion_value(c):
    return float(c)


def _fit_generic(model, save_dir, train_loader, gen_optim, max_iter, lookback, check_every, verbose, GC, val_loader):
    """models/dgcnn.py:122-199 with torch autograd and the caller's optimizer."""
    avg_factor_loss, step_losses = [], []
    best_it, best_loss, best_model = None, np.inf, None
    for it in range(max_iter):
        running = 0.
        for batch_num, (X, Y) in enumerate(train_loader):
            before = running
            running = model.batch_update(batch_num, X, Y, gen_optim, running)
            step_losses.append(running - before)
        avg_factor_loss.append(running / len(train_loader))
        if it % check_every == 0:
            mean_val_loss = model.training_eval(val_loader)
            if verbose > 0:
                print(('-' * 10 + 'Iter = %d' + '-' * 10) % (it + 1), flush=True)
                print('Validation Loss = %f' % mean_val_loss)
                print('Factor 0 Variable usage = %.2f%%' % (100 * torch.mean(model.GC()[0].float())))
            crit = _criterion_value(model.stopping_criterion())
            if crit < best_loss:
                best_loss, best_it, best_model = crit, it, _standalone(model)
            elif (it - best_it) == lookback * check_every:
                if verbose:
                    print('Stopping early', flush=True)
                break
            model.save_checkpoint(save_dir, it, best_model, avg_factor_loss, best_loss, GC)
    _restore_parameters(model, best_model)
    os.makedirs(save_dir, exist_ok=True)
    torch.save(_standalone(model), os.path.join(save_dir, "final_best_model.bin"))
    model.avg_factor_loss, model.stopped_at = avg_factor_loss, it
    model.step_losses = np.asarray(step_losses, dtype=np.float64)
    return model.training_eval(val_loader)


def _collect(model, loader):
    """One pass over a loader: (X (N, T, nodes) float32, selected labels (N, C) float32, batch sizes), or
    None when it is empty."""
    xs, ys, sizes = [], [], []
    for X, Y in loader:
        xs.append(torch.as_tensor(X).detach().to("cpu", torch.float32))
        ys.append(select_labels(torch.as_tensor(Y).detach(), model.num_features_per_node).to("cpu", torch.float32))
        sizes.append(int(xs[-1].shape[0]))
    if not xs:
        return None
    return torch.cat(xs).contiguous(), torch.cat(ys).contiguous(), sizes


def _segments(sizes):
    """Native calls that replay batches of these sizes in order: [(row0, rows, B)].  Equal batches with a
    shorter (or equal) last one are one call; otherwise one call per batch."""
    if all(s == sizes[0] for s in sizes[:-1]) and 0 < sizes[-1] <= sizes[0]:
        return [(0, sum(sizes), sizes[0])]
    out, at = [], 0
    for s in sizes:
        out.append((at, s, s))
        at += s
    return out


def fit_dgcnn_baselines(models, save_dirs, train_loaders, optimizers, max_iter, lookback, check_every, verbose, GCs,
                        val_loaders):
    """DGCNN_Model.fit (models/dgcnn.py:122-199) for a list of models, each with its own loaders, optimizer,
    save_dir and true graph.  Same-shape models whose loaders yield the same batch sizes share one native
    call per epoch on the fused route, each with its own early stopping; otherwise one fit after the other.
    Returns the fits' final validation losses; ``model.avg_factor_loss`` (the training history),
    ``model.step_losses`` and ``model.stopped_at`` (the last epoch run) are left on every model."""
    R = len(models)
    if not (len(save_dirs) == len(train_loaders) == len(optimizers) == len(GCs) == len(val_loaders) == R) or R == 0:
        raise ValueError("fit_dgcnn_baselines: one save_dir, loader pair, optimizer and GC per model")
    m0 = models[0]
    one_by_one = lambda: [fit_dgcnn_baselines([models[i]], [save_dirs[i]], [train_loaders[i]], [optimizers[i]], max_iter,
                                              lookback, check_every, verbose, [GCs[i]], [val_loaders[i]])[0]
                          for i in range(R)]
    generic = lambda: [_fit_generic(m0, save_dirs[0], train_loaders[0], optimizers[0], max_iter, lookback, check_every,
                                    verbose, GCs[0], val_loaders[0])]
    if not all(m.fused_eligible(optimizers[i]) for i, m in enumerate(models)) or max_iter < 1:
        return one_by_one() if R > 1 else generic()
    if R > 1 and (any(m.fit_shape() != m0.fit_shape() for m in models) or len(set(id(m) for m in models)) != R or
                  R > MAX_REPLICAS):
        return one_by_one()
    tr = [_collect(m, train_loaders[i]) for i, m in enumerate(models)]
    va = [_collect(m, val_loaders[i]) for i, m in enumerate(models)]
    if R == 1 and (tr[0] is None or va[0] is None):
        return generic()
    ok = all(t is not None and v is not None for t, v in zip(tr, va))
    same = ok and all(t[2] == tr[0][2] and t[0].shape == tr[0][0].shape and t[1].shape == tr[0][1].shape for t in tr) and \
        all(v[2] == va[0][2] and v[0].shape == va[0][0].shape and v[1].shape == va[0][1].shape for v in va)
    if not same:
        return one_by_one()
    Bmax = max(tr[0][2] + va[0][2])
    Ts = (int(tr[0][0].shape[1]), int(va[0][0].shape[1]))
    good = all(x.dim() == 3 and int(x.shape[2]) == m0.num_nodes for x in (tr[0][0], va[0][0])) and \
        all(y.dim() == 2 and int(y.shape[1]) == m0.num_classes for y in (tr[0][1], va[0][1])) and \
        all(m.fused_eligible(optimizers[i], T=T, Bmax=Bmax) for i, m in enumerate(models) for T in Ts)
    if not good:
        return one_by_one() if R > 1 else generic()
    # ---------------------------------------------------------------- fused
    pack, rows, _ = packs.acquire(models, optimizers, DgcnnFitPack)
    dev = pack.device

    def upload(sets, k):
        return packs.stack_upload([s[k] for s in sets], dev)
    Xtr, xps = upload(tr, 0)
    Ytr, yps = upload(tr, 1)
    Xva, xps_va = upload(va, 0)
    Yva, yps_va = upload(va, 1)
    seg_tr, seg_va = _segments(tr[0][2]), _segments(va[0][2])
    n_tr, n_va = len(tr[0][2]), len(va[0][2])

    def act(idx):
        """The native call's active list for the fits idx (None: every row of the pack)."""
        reps = [rows[i] for i in idx]
        return None if len(reps) == pack.R else reps

    def evaluate(idx):
        """training_eval of the fits idx: the mean over batches of each batch's MSE, in doubles."""
        mses = [pack.forward(Xva, xps_va, Yva, yps_va, r0_, n_, B_, active=act(idx))[1] for r0_, n_, B_ in seg_va]
        vals = torch.cat(mses, 1).double().cpu().numpy()
        out = []
        for k in range(len(idx)):
            s = 0.
            for v in vals[k]:
                s += float(v)
            out.append(s / n_va)
        return out

    live = list(range(R))
    pending = []  # (fits, device losses [len(fits)][n_tr]) of the epochs no check has fetched yet
    hist = [[] for _ in range(R)]
    steps = [[] for _ in range(R)]
    best_it, best_loss, best_model, last_it = [None] * R, [np.inf] * R, [None] * R, [0] * R

    def drain():
        for idx, dev_loss in pending:
            vals = dev_loss.double().cpu().numpy()
            for k, i in enumerate(idx):
                s = 0.
                for v in vals[k]:
                    s += float(v)
                hist[i].append(s / n_tr)
                steps[i].extend(float(v) for v in vals[k])
        del pending[:]

    for it in range(max_iter):
        if not live:
            break
        for m in (models[i] for i in live):
            m.dgcnn.train()
        pending.append((list(live), torch.cat([pack.train(Xtr, xps, Ytr, yps, r0_, n_, B_, active=act(live))
                                               for r0_, n_, B_ in seg_tr], 1)))
        for i in live:
            last_it[i] = it
        if it % check_every == 0:
            drain()
            for m in (models[i] for i in live):
                m.dgcnn.eval()
            val = evaluate(live)
            crits = torch.stack([models[i].stopping_criterion() for i in live]).cpu().numpy()
            still = []
            for k, i in enumerate(live):
                m = models[i]
                if verbose > 0:
                    print(('-' * 10 + 'Iter = %d' + '-' * 10) % (it + 1), flush=True)
                    print('Validation Loss = %f' % val[k])
                    print('Factor 0 Variable usage = %.2f%%' % (100 * torch.mean(m.GC()[0].float())))
                crit = _criterion_value(crits[k])
                if crit < best_loss[i]:
                    best_loss[i], best_it[i], best_model[i] = crit, it, _standalone(m)
                elif (it - best_it[i]) == lookback * check_every:
                    if verbose:
                        print('Stopping early', flush=True)
                    continue
                m.save_checkpoint(save_dirs[i], it, best_model[i], list(hist[i]), best_loss[i], GCs[i])
                still.append(i)
            live = still
    drain()
    for i, m in enumerate(models):
        _restore_parameters(m, best_model[i])
        m.dgcnn.eval()
        os.makedirs(save_dirs[i], exist_ok=True)
        torch.save(_standalone(m), os.path.join(save_dirs[i], "final_best_model.bin"))
        m.avg_factor_loss, m.stopped_at = hist[i], last_it[i]
        m.step_losses = np.asarray(steps[i], dtype=np.float64)
    return evaluate(list(range(R)))
