"""The supervised dCSFA-NMF baseline of the paper's comparison (model type "DCSFANMF"): the classes of the
reference's models/dcsfa_nmf.py and models/dcsfa_nmf_vanillaDirSpec.py with the same constructor arguments
and the same parameter tree (``W_nmf``, ``encoder.0/1/3.*``, ``phi_list.i``, ``beta_list.i``).

``FullDCSFAModel`` unflattens directed-spectrum features in ``GC`` (dcsfa_nmf.py); ``FullDCSFAModel_GCv2``
has the "vanilla" ``GC`` that reshapes to (nodes, nodes, features) (dcsfa_nmf_vanillaDirSpec.py) and is the
class the D4IC driver builds.

``fit`` has two routes, chosen per call by ``REDCLIFF_DCSFA_PATH=fused|generic`` (default: DEFAULT_PATH):

* generic -- the reference's loop in plain torch (WeightedRandomSampler + DataLoader, autograd, the
  optimizer named by ``optim_name``), on any device and in ``fit_dtype``; serves every configuration.
* fused -- ``redcliff_dcsfa_run`` (csrc/rc_dcsfa.hip): one native call per optimiser epoch (a pass of
  ``pretrain_encoder`` or of the main loop) on that epoch's row indices, drawn on the host with the
  generator calls of the reference's sampler and loader in their order; X, y, the masks and the weights stay
  on the device for the whole fit, the per-epoch evaluation runs there too and returns sums and confusion
  counts, and parameters are fetched only when a file is written.  Taken when ``fused_eligible`` holds.

``fit_dcsfa_baselines`` fits R same-shape models with the replica on a grid axis; ``DcsfaNmf.fit`` is that
function with lists of one.  ``pretrain_NMF`` stays on the host (sklearn ``NMF``, scipy ``mannwhitneyu``).

Decided departures from the reference: the end-of-fit reload reads the path the best-model file
was written to; ``GC(threshold=True)`` returns ``(GC > 0).astype(int)``; a last batch of one row and a label
column with one class under the 0.6 cut raise ``ValueError`` before any step runs, on both routes.
"""
import ctypes
import os
import pickle as pkl
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.data import DataLoader, TensorDataset, WeightedRandomSampler

from . import _native as nat
from . import packs

try:
    from sklearn.decomposition import NMF
    SKLEARN_INSTALLED = True
except ImportError:  # pretrain_NMF raises; everything else works
    NMF = None
    SKLEARN_INSTALLED = False

ENV = "REDCLIFF_DCSFA_PATH"
DEFAULT_PATH = "fused"  # faster for one fit and for 15 (profiles/dcsfa_fit.json)
DC_HS, DC_BC, DC_KMAX, DC_BMAX, DC_MISC = 8, 32, 8, 128, 128  # csrc/rc_dcsfa.h
LDS_MAX_FLOATS = 40960  # RC_LDS_MAX_FLOATS
MAX_REPLICAS = 256
TRAIN, PRETRAIN, EVAL = 0, 1, 2
ADAMW = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)  # torch.optim.AdamW's defaults
LAST_EPOCH_NAME = "dCSFA-NMF-last-epoch.pt"
ONE_ROW_MSG = "a last batch of one row has no batch statistics (BatchNorm1d in training mode): %d rows in batches of %d"
ONE_CLASS_MSG = "Only one class present in y_true. ROC AUC score is not defined in that case."


def dcsfa_path():
    """'fused' or 'generic', from REDCLIFF_DCSFA_PATH (read per call)."""
    return packs.route_from_env(ENV, DEFAULT_PATH)


def unflatten_directed_spectrum_features(x_flat):
    """general_utils/misc.py:178-195: (n, m * (2n - 1)) rows of flattened directed-spectrum features ->
    (n, n, m): per feature, node j's block is its row, then column j above and below the diagonal."""
    assert len(x_flat.shape) == 2
    n = x_flat.shape[0]
    m = int(x_flat.shape[1] / (2 * n - 1))
    x = np.zeros((n, n, m))
    for i in range(m):
        c0 = i * (2 * n - 1)
        for j in range(n):
            x[j, :, i] += x_flat[j, c0:c0 + n]
            x[:j, j, i] += x_flat[j, c0 + n:c0 + n + j]
            x[j + 1:, j, i] += x_flat[j, c0 + n + j:c0 + 2 * n - 1]
    return x


def binary_auc(tp, fp, tn, fn):
    """roc_auc_score of two binary vectors from their confusion counts: (1 + TPR - FPR) / 2."""
    if tp + fn == 0 or fp + tn == 0:
        raise ValueError(ONE_CLASS_MSG)
    return (1.0 + tp / float(tp + fn) - fp / float(fp + tn)) / 2.0


def confusion_counts(label, pred):
    label, pred = np.asarray(label, dtype=bool), np.asarray(pred, dtype=bool)
    return (int(np.sum(label & pred)), int(np.sum(~label & pred)), int(np.sum(~label & ~pred)),
            int(np.sum(label & ~pred)))


def roc_auc(y_true, y_score):
    """sklearn.metrics.roc_auc_score for binary labels: the Mann-Whitney statistic with mid-ranks."""
    from scipy.stats import rankdata
    y_true = np.asarray(y_true).reshape(-1).astype(bool)
    n1, n0 = int(y_true.sum()), int((~y_true).sum())
    if n1 == 0 or n0 == 0:
        raise ValueError(ONE_CLASS_MSG)
    ranks = rankdata(np.asarray(y_score, dtype=np.float64).reshape(-1))
    return float((ranks[y_true].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


def draw_epoch_indices(weights, n):
    """The rows one epoch of DataLoader(dset, sampler=WeightedRandomSampler(weights, n)) visits, from the
    default generator: the loader's iterator draws its base seed first, then the sampler its multinomial."""
    torch.empty((), dtype=torch.int64).random_()
    return torch.multinomial(weights, n, True)


# --------------------------------------------------------------------------------------------------
def dcsfa_lds_floats(D, H, K, ns, B, R=1):
    """rc_dcsfa_lds_floats (csrc/rc_dcsfa.h) restated: the workgroup's LDS floats, 0 outside the limits."""
    if min(D, H, K, ns, B, R) < 1:
        return 0
    if K > DC_KMAX or ns > K or B > DC_BMAX or R > MAX_REPLICAS or H > 4096 or D > 4096:
        return 0
    Dp = D | 1
    fwd = DC_MISC + B + B * DC_HS + DC_HS * Dp + DC_BC * Dp
    head = DC_MISC + B + 7 * B * K + 4 * K * K + K * Dp
    bwd = DC_MISC + B + B * K + 3 * B * DC_HS + K * DC_HS
    f = max(fwd, head, bwd)
    return f if f <= LDS_MAX_FLOATS else 0


def dcsfa_supported(D, H, K, ns, B, R=1):
    """redcliff_dcsfa_supported: the footprint in floats, 0 outside the limits."""
    return int(nat.lib().redcliff_dcsfa_supported(int(D), int(H), int(K), int(ns), int(B), int(R)))


def dcsfa_ws_floats(H, K, B):
    return int(nat.lib().redcliff_dcsfa_ws_floats(int(H), int(K), int(B)))


def dcsfa_layout(D, H, K, ns):
    """[(name, offset, shape)] of the packed block and its size (rc_dcsfa_off)."""
    out, at = [], 0
    shapes = [("W_nmf", (K, D)), ("W1", (H, D)), ("b1", (H,)), ("bn_w", (H,)), ("bn_b", (H,)), ("W2", (K, H)), ("b2", (K,))]
    shapes += [("phi%d" % j, (1,)) for j in range(ns)] + [("beta%d" % j, (1, 1)) for j in range(ns)]
    for name, shp in shapes:
        out.append((name, at, shp))
        at += int(np.prod(shp))
    return out, at


class DcsfaFitPack:
    """R same-shape DcsfaNmf models on the fused route: their parameters are views of par[r], the BatchNorm
    running statistics of rm[r] / rv[r]; m / v hold AdamW's moments (as dgcnn.DgcnnFitPack)."""

    def __init__(self, models):
        m0 = models[0]
        self.shape = m0.fit_shape()
        for m in models:
            if m.fit_shape() != self.shape:
                raise ValueError("a DcsfaFitPack holds models of one shape")
        self.D, self.H, self.K, self.ns = self.shape
        self.models = list(models)
        self.R = len(models)
        if not dcsfa_supported(*self.shape, DC_BMAX, self.R):
            nat.check(-2, "dcsfa_supported")
        self.device = m0.W_nmf.device
        if not m0.W_nmf.is_cuda:
            raise RuntimeError("DcsfaNmf (fused) runs on the MI355X only (HIP kernels); move the model to 'cuda'")
        self.layout, self.np_ = dcsfa_layout(*self.shape)
        self.par = torch.empty(self.R, self.np_, device=self.device, dtype=torch.float32)
        self.m = torch.zeros_like(self.par)
        self.v = torch.zeros_like(self.par)
        self.rm = torch.empty(self.R, self.H, device=self.device, dtype=torch.float32)
        self.rv = torch.empty_like(self.rm)
        self.ws = torch.empty(self.R * dcsfa_ws_floats(self.H, self.K, DC_BMAX), device=self.device, dtype=torch.float32)
        self.t = 0
        for r, mod in enumerate(self.models):
            packs.pack_by_layout(self.par[r], mod.packed_parameters(), self.layout)
            packs.adopt_bn_stats(mod.encoder[1], self.rm[r], self.rv[r])

    def reset_optimizer(self):
        """A fresh AdamW: zero moments, step 0."""
        self.m.zero_()
        self.v.zero_()
        self.t = 0

    def _args(self, mode, B, data, lr):
        m0 = self.models[0]
        bn = m0.encoder[1]
        a = nat.DcsfaArgs()
        a.D, a.H, a.K, a.ns, a.R, a.Bmax = self.D, self.H, self.K, self.ns, self.R, DC_BMAX
        a.mode, a.B, a.tB = int(mode), int(B), self.t + 1
        X, Y, TM, PW = data
        a.N = int(X.shape[-2])
        a.X, a.Y, a.TM, a.PW = X.data_ptr(), Y.data_ptr(), TM.data_ptr(), PW.data_ptr()
        shared = X.dim() == 2
        a.x_pstride = 0 if shared else X[0].numel()
        a.y_pstride = 0 if shared else Y[0].numel()
        a.pw_pstride = 0 if shared else PW[0].numel()
        a.par, a.par_m, a.par_v, a.par_stride = self.par.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.np_
        a.bn_rm, a.bn_rv = self.rm.data_ptr(), self.rv.data_ptr()
        a.lr, a.weight_decay = float(lr), ADAMW["weight_decay"]
        a.beta1, a.beta2, a.eps = ADAMW["betas"][0], ADAMW["betas"][1], ADAMW["eps"]
        a.bn_eps, a.bn_momentum = float(bn.eps), float(bn.momentum)
        a.recon_weight, a.sup_weight = float(m0.recon_weight), float(m0.sup_weight)
        a.sup_recon_weight, a.sup_smoothness_weight = float(m0.sup_recon_weight), float(m0.sup_smoothness_weight)
        a.ws, a.ws_bytes = self.ws.data_ptr(), self.ws.numel() * 4
        return a

    def epoch(self, mode, idx, B, data, lr):
        """One optimiser epoch (TRAIN or PRETRAIN) over the drawn rows idx [R][n] (int32, on the device):
        ceil(n / B) AdamW steps in one native call.  Returns the steps' losses, a device tensor [R][nsteps][2]."""
        n = int(idx.shape[1])
        nsteps = -(-n // int(B))
        loss = torch.empty(self.R, nsteps, 2, device=self.device, dtype=torch.float32)
        a = self._args(mode, B, data, lr)
        a.n, a.idx, a.idx_pstride, a.loss = n, idx.data_ptr(), n, loss.data_ptr()
        rc = nat.lib().redcliff_dcsfa_run(ctypes.byref(a), nat.stream_or_current(None))
        nat.check(rc, "dcsfa_run")
        self.t += nsteps
        for mod in self.models:
            mod.encoder[1].num_batches_tracked += nsteps
        return loss

    def evaluate(self, data):
        """The eval pass over a whole set: (sum of squared reconstruction errors [R], confusion counts
        [R][ns][4] = TP, FP, TN, FN under the 0.6 cuts over the rows with task_mask == 1), device tensors."""
        N = int(data[0].shape[-2])
        nb = -(-N // DC_BMAX)
        ev = torch.empty(self.R, nb, 1 + 4 * self.ns, device=self.device, dtype=torch.float64)
        a = self._args(EVAL, DC_BMAX, data, 0.0)
        a.n, a.row0, a.ev = N, 0, ev.data_ptr()
        rc = nat.lib().redcliff_dcsfa_run(ctypes.byref(a), nat.stream_or_current(None))
        nat.check(rc, "dcsfa_run")
        tot = ev.sum(1)
        return tot[:, 0], tot[:, 1:].reshape(self.R, self.ns, 4)


# --------------------------------------------------------------------------------------------------
class NmfBase(nn.Module):
    """models/dcsfa_nmf.py NmfBase: the NMF decoder W_nmf (kept non-negative through a softplus), the
    reconstruction losses and the sklearn pretraining."""

    fit_dtype = torch.float32  # the generic route's dtype (a float64 run is the tests' yardstick)

    def __init__(self, n_components, device="auto", n_sup_networks=1, fixed_corr=None, recon_loss="MSE", recon_weight=1.0,
                 sup_recon_type="Residual", sup_recon_weight=1.0, sup_smoothness_weight=1, feature_groups=None,
                 group_weights=None, verbose=False):
        super().__init__()
        self.n_components = n_components
        self.n_sup_networks = n_sup_networks
        self.recon_loss = recon_loss
        self.recon_weight = recon_weight
        self.sup_recon_type = sup_recon_type
        self.sup_smoothness_weight = sup_smoothness_weight
        self.sup_recon_weight = sup_recon_weight
        self.verbose = verbose
        self.recon_loss_f = self.get_recon_loss(recon_loss)
        if fixed_corr is None:
            self.fixed_corr = ["n/a" for _ in range(self.n_sup_networks)]
        elif type(fixed_corr) != list:
            if fixed_corr.lower() not in ("positive", "negative", "n/a"):
                raise ValueError("fixed corr must be a list or in {`positive`,`negative`,`n/a`}")
            self.fixed_corr = [fixed_corr.lower()]
        else:
            assert len(fixed_corr) == self.n_sup_networks
            self.fixed_corr = fixed_corr
        self.feature_groups = feature_groups
        if feature_groups is not None and group_weights is None:
            group_weights = [(feature_groups[-1][-1] - feature_groups[0][0]) / (ub - lb) for (lb, ub) in feature_groups]
        self.group_weights = group_weights
        if device == "auto":
            self.device = "cuda" if torch.cuda.is_available() else "cpu"
        else:
            self.device = device

    def _initialize_NMF(self, dim_in):
        self.W_nmf = nn.Parameter(torch.rand(self.n_components, dim_in))
        self.to(self.device)

    @staticmethod
    def inverse_softplus(x, eps=1e-5):
        return np.log(np.exp(x + eps) - (1.0 - eps))

    def get_W_nmf(self):
        return F.softplus(self.W_nmf)

    def get_recon_loss(self, recon_loss):
        if recon_loss == "MSE":
            return nn.MSELoss()
        if recon_loss == "IS":
            raise NotImplementedError("the IS reconstruction loss (torchbd) is not part of this build")
        raise ValueError(f"{recon_loss} is not supported")

    def get_optim(self, optim_name):
        if optim_name == "AdamW":
            return torch.optim.AdamW
        if optim_name == "Adam":
            return torch.optim.Adam
        if optim_name == "SGD":
            return torch.optim.SGD
        raise ValueError(f"{optim_name} is not supported")

    @torch.no_grad()
    def pretrain_NMF(self, X, y, nmf_max_iter=100):
        """dcsfa_nmf.py:182-270 on the host: an sklearn NMF, its components ordered by how well each
        predicts the supervised tasks (Mann-Whitney AUC, the first task choosing first), stored through the
        inverse softplus as W_nmf."""
        if not SKLEARN_INSTALLED:
            raise ImportError("pretrain_NMF needs scikit-learn (sklearn.decomposition.NMF); install it or fit with "
                              "pretrain=False")
        from scipy.stats import mannwhitneyu
        self.NMF_init = NMF(n_components=self.n_components, max_iter=nmf_max_iter, init="nndsvd")
        s_NMF = self.NMF_init.fit_transform(X)
        selected = []
        order = None
        for sup_net in range(self.n_sup_networks):
            aucs = []
            for component in range(self.n_components):
                s_pos = s_NMF[y[:, sup_net] >= 0.6, component].reshape(-1, 1)
                s_neg = s_NMF[y[:, sup_net] < 0.6, component].reshape(-1, 1)
                U, _ = mannwhitneyu(s_pos, s_neg)
                aucs.append(np.squeeze(U) / (len(s_pos) * len(s_neg)))
            aucs = np.array(aucs)
            order = np.argsort(np.abs(aucs - 0.5))[::-1]
            pos_order = np.argsort(aucs)[::-1]
            neg_order = np.argsort(1 - aucs)[::-1]
            for taken in selected:
                order = order[order != taken]
                pos_order = pos_order[pos_order != taken]
                neg_order = neg_order[neg_order != taken]
            corr = self.fixed_corr[sup_net].lower()
            current = order[0] if corr == "n/a" else (pos_order[0] if corr == "positive" else neg_order[0])
            selected.append(current)
            order = order[order != current]
        self.skl_pretrain_networks_ = list(selected)
        final_order = list(selected) + [c for c in order]
        sorted_NMF = self.NMF_init.components_[final_order]
        W = torch.from_numpy(self.inverse_softplus(sorted_NMF.astype(np.float32)))
        self.W_nmf.data.copy_(W.to(self.W_nmf.device, self.W_nmf.dtype))

    def get_sup_recon(self, s):
        ns = self.n_sup_networks
        return s[:, :ns].view(-1, ns) @ self.get_W_nmf()[:ns, :].view(ns, -1)

    def get_residual_scores(self, X, s):
        """s_h = (X - s_unsup W_unsup) W_sup^T inv(W_sup W_sup^T)."""
        ns = self.n_sup_networks
        W = self.get_W_nmf()
        resid = X - s[:, ns:] @ W[ns:, :]
        w_sup = W[:ns, :].view(ns, -1)
        return resid @ w_sup.T @ torch.inverse(w_sup @ w_sup.T)

    def residual_loss_f(self, s, s_h):
        ns = self.n_sup_networks
        return torch.norm(s[:, :ns].view(-1, ns) - s_h) / (1 - self.sup_smoothness_weight * torch.exp(-torch.norm(s_h)))

    def get_weighted_recon_loss_f(self, X_pred, X_true):
        recon_loss = 0.0
        for weight, (lb, ub) in zip(self.group_weights, self.feature_groups):
            recon_loss += weight * self.recon_loss_f(X_pred[:, lb:ub], X_true[:, lb:ub])
        return recon_loss

    def eval_recon_loss(self, X_pred, X_true):
        if self.feature_groups is None:
            return self.recon_loss_f(X_pred, X_true)
        return self.get_weighted_recon_loss_f(X_pred, X_true)

    def NMF_decoder_forward(self, X, s):
        recon_loss = self.recon_weight * self.eval_recon_loss(s @ self.get_W_nmf(), X)
        if self.sup_recon_type == "Residual":
            sup_recon_loss = self.residual_loss_f(s, self.get_residual_scores(X, s))
        elif self.sup_recon_type == "All":
            sup_recon_loss = self.recon_loss_f(self.get_sup_recon(s), X)
        else:
            raise ValueError(f"{self.sup_recon_type} is not supported")
        return recon_loss + self.sup_recon_weight * sup_recon_loss

    @torch.no_grad()
    def get_comp_recon(self, s, component):
        s = torch.as_tensor(s).to(self.W_nmf.device, self.W_nmf.dtype)
        X_recon = s[:, component].view(-1, 1) @ self.get_W_nmf()[component, :].view(1, -1)
        return X_recon.detach().cpu().numpy()

    @torch.no_grad()
    def get_all_comp_recon(self, s):
        return s @ self.get_W_nmf()

    @torch.no_grad()
    def get_factor(self, component):
        return self.get_W_nmf()[component, :].detach().cpu().numpy()


class DcsfaNmf(NmfBase):
    """models/dcsfa_nmf.py DcsfaNmf: the encoder, the logistic heads and the fit (see the module docstring
    for its two routes)."""

    def __init__(self, n_components=32, device="auto", n_intercepts=1, n_sup_networks=1, optim_name="AdamW",
                 recon_loss="MSE", recon_weight=1.0, sup_weight=1.0, sup_recon_weight=1.0, use_deep_encoder=True, h=256,
                 sup_recon_type="Residual", feature_groups=None, group_weights=None, fixed_corr=None, momentum=0.9, lr=1e-3,
                 sup_smoothness_weight=1.0, save_folder="~", verbose=False):
        super().__init__(n_components, device, n_sup_networks, fixed_corr, recon_loss, recon_weight, sup_recon_type,
                         sup_recon_weight, sup_smoothness_weight, feature_groups, group_weights, verbose)
        self.n_intercepts = n_intercepts
        self.optim_name = optim_name
        self.optim_alg = self.get_optim(optim_name)
        self.pred_loss_f = nn.BCELoss
        self.sup_weight = sup_weight
        self.use_deep_encoder = use_deep_encoder
        self.h = h
        self.momentum = momentum
        self.lr = lr
        self.save_folder = save_folder

    def _initialize(self, dim_in):
        """Registration order (= RNG order): W_nmf, the encoder, the phi, the beta."""
        self.dim_in_ = dim_in
        self._initialize_NMF(dim_in)
        if self.use_deep_encoder:
            self.encoder = nn.Sequential(nn.Linear(dim_in, self.h), nn.BatchNorm1d(self.h), nn.LeakyReLU(),
                                         nn.Linear(self.h, self.n_components), nn.Softplus())
        else:
            self.encoder = nn.Sequential(nn.Linear(dim_in, self.n_components), nn.Softplus())
        self.phi_list = nn.ParameterList([nn.Parameter(torch.randn(1)) for _ in range(self.n_sup_networks)])
        self.beta_list = nn.ParameterList([nn.Parameter(torch.randn(self.n_intercepts, 1))
                                           for _ in range(self.n_sup_networks)])
        self.to(self.device, self.fit_dtype)

    def instantiate_optimizer(self):
        if self.optim_name == "SGD":
            return self.optim_alg(self.parameters(), lr=self.lr, momentum=self.momentum)
        return self.optim_alg(self.parameters(), lr=self.lr)

    def get_phi(self, sup_net=0):
        corr = self.fixed_corr[sup_net].lower()
        if corr == "n/a":
            return self.phi_list[sup_net]
        if corr == "positive":
            return F.softplus(self.phi_list[sup_net])
        if corr == "negative":
            return -1 * F.softplus(self.phi_list[sup_net])
        raise ValueError(f"Unsupported fixed_corr value: {corr}")

    def get_all_class_predictions(self, X, s, intercept_mask, avg_intercept):
        if intercept_mask is None and avg_intercept is False:
            warnings.warn("Intercept mask cannot be none and avg_intercept False... Averaging Intercepts")
            avg_intercept = True
        y_pred_list = []
        for sup_net in range(self.n_sup_networks):
            z = s[:, sup_net].view(-1, 1) * self.get_phi(sup_net)
            if self.n_intercepts == 1:
                z = z + self.beta_list[sup_net]
            elif not avg_intercept:
                z = z + intercept_mask @ self.beta_list[sup_net]
            else:
                intercept_mask = torch.ones(X.shape[0], self.n_intercepts, device=s.device, dtype=s.dtype) / self.n_intercepts
                z = z + intercept_mask @ self.beta_list[sup_net]
            y_pred_list.append(torch.sigmoid(z).squeeze().view(-1, 1))
        return torch.cat(y_pred_list, dim=1)

    def get_embedding(self, X):
        return self.encoder(X)

    def _to_model(self, t, dtype=None):
        prm = self.W_nmf
        return torch.as_tensor(t).to(prm.device, prm.dtype if dtype is None else dtype)

    def forward(self, X, y, task_mask, pred_weight, intercept_mask=None, avg_intercept=False):
        """(recon_weight * mse + sup_recon_weight * supervised reconstruction loss, sup_weight * BCE), kept
        apart so that the encoder pretraining can apply the first alone."""
        X, y, pred_weight = self._to_model(X), self._to_model(y), self._to_model(pred_weight)
        task_mask = torch.as_tensor(task_mask).to(X.device)
        if intercept_mask is not None:
            intercept_mask = self._to_model(intercept_mask)
        s = self.get_embedding(X)
        recon_loss = self.NMF_decoder_forward(X, s)
        y_pred = self.get_all_class_predictions(X, s, intercept_mask, avg_intercept)
        pred_loss = self.sup_weight * self.pred_loss_f(weight=pred_weight)(y_pred * task_mask, y * task_mask)
        return recon_loss, pred_loss

    @torch.no_grad()
    def transform(self, X, intercept_mask=None, avg_intercept=True, return_npy=True):
        """(X_recon, y_pred, s) of X with the module in its current mode."""
        X = self._to_model(X)
        if intercept_mask is not None:
            intercept_mask = self._to_model(intercept_mask)
        s = self.get_embedding(X)
        X_recon = self.get_all_comp_recon(s)
        y_pred = self.get_all_class_predictions(X, s, intercept_mask, avg_intercept)
        if return_npy:
            return X_recon.detach().cpu().numpy(), y_pred.detach().cpu().numpy(), s.detach().cpu().numpy()
        return X_recon, y_pred, s

    # ------------------------------------------------------------------ route
    def fit_shape(self):
        return (int(self.dim_in_), int(self.h), int(self.n_components), int(self.n_sup_networks))

    def packed_parameters(self):
        """The parameters in the packed layout's order."""
        e = self.encoder
        return [self.W_nmf, e[0].weight, e[0].bias, e[1].weight, e[1].bias, e[3].weight, e[3].bias] + \
            list(self.phi_list) + list(self.beta_list)

    def fused_eligible(self, batch_size=128, dim_in=None):
        """The fused route serves this model at this batch size (and feature count, before _initialize)."""
        if dcsfa_path() != "fused":
            return False
        if torch.device(self.device).type != "cuda" or self.fit_dtype != torch.float32:
            return False
        if self.optim_name != "AdamW" or self.recon_loss != "MSE" or self.sup_recon_type != "Residual":
            return False
        if not self.use_deep_encoder or self.n_intercepts != 1 or self.feature_groups is not None:
            return False
        if any(str(c).lower() != "n/a" for c in self.fixed_corr):
            return False
        K, ns = int(self.n_components), int(self.n_sup_networks)
        if not (1 <= ns <= K <= DC_KMAX) or not (1 <= int(batch_size) <= DC_BMAX):
            return False
        D = getattr(self, "dim_in_", None) if dim_in is None else dim_in
        if D is None:
            return True
        if hasattr(self, "encoder"):
            bn = self.encoder[1]
            if not (bn.affine and bn.track_running_stats and bn.momentum is not None):
                return False
            if not all(p.is_cuda and p.dtype == torch.float32 for p in self.parameters()):
                return False
        if not dcsfa_lds_floats(int(D), int(self.h), K, ns, DC_BMAX):
            return False
        return dcsfa_supported(int(D), int(self.h), K, ns, DC_BMAX) > 0

    def pretrain_encoder(self, X, y, y_pred_weights, task_mask, intercept_mask, sample_weights, n_pre_epochs=100,
                         batch_size=128):
        """dcsfa_nmf.py pretrain_encoder on the generic route: the reconstruction loss alone, W_nmf frozen."""
        self.W_nmf.requires_grad = False
        dt = self.fit_dtype
        dset = TensorDataset(torch.Tensor(X).to(dt), torch.Tensor(y).to(dt), torch.Tensor(task_mask).long(),
                             torch.Tensor(y_pred_weights).to(dt), torch.Tensor(intercept_mask))
        sampler = WeightedRandomSampler(torch.Tensor(sample_weights), len(sample_weights))
        loader = DataLoader(dset, batch_size=batch_size, sampler=sampler)
        optimizer = self.instantiate_optimizer()
        losses = []
        for _ in range(n_pre_epochs):
            for batch in loader:
                optimizer.zero_grad()
                recon_loss, pred_loss = self.forward(*batch)
                recon_loss.backward()
                optimizer.step()
                losses.append((recon_loss.item(), pred_loss.item()))
        self.W_nmf.requires_grad = True
        self.pretrain_step_losses = np.asarray(losses, dtype=np.float64).reshape(-1, 2)

    def fit(self, X, y, y_pred_weights=None, task_mask=None, intercept_mask=None, y_sample_groups=None, n_epochs=100,
            n_pre_epochs=100, nmf_max_iter=100, batch_size=128, lr=1e-3, pretrain=True, verbose=False, X_val=None,
            y_val=None, y_pred_weights_val=None, task_mask_val=None, best_model_name="dCSFA-NMF-best-model.pt"):
        fit_dcsfa_baselines([self], [X], [y], y_pred_weights=[y_pred_weights], task_masks=[task_mask],
                            intercept_masks=[intercept_mask], y_sample_groups=[y_sample_groups], n_epochs=n_epochs,
                            n_pre_epochs=n_pre_epochs, nmf_max_iter=nmf_max_iter, batch_size=batch_size, lr=lr,
                            pretrain=pretrain, verbose=verbose, X_vals=[X_val], y_vals=[y_val],
                            y_pred_weights_vals=[y_pred_weights_val], task_mask_vals=[task_mask_val],
                            best_model_name=best_model_name)
        return self

    def _load(self, path):
        got = torch.load(path, map_location=self.W_nmf.device, weights_only=False)
        if isinstance(got, nn.Module):
            got = got.state_dict()
        with torch.no_grad():  # in place: a packed model's views stay views
            own = self.state_dict()
            if set(own) != set(got):
                raise RuntimeError("state dict keys differ: %s" % sorted(set(own) ^ set(got)))
            for k, v in own.items():
                v.copy_(got[k])

    def load_last_epoch(self):
        """The last epoch's parameters, in case they are preferable to the early-stop checkpoint."""
        self._load(os.path.join(self.save_folder, LAST_EPOCH_NAME))

    def reconstruct(self, X, component=None):
        X_recon, _, s = self.transform(X)
        if component is not None:
            X_recon = self.get_comp_recon(s, component)
        return X_recon

    def predict_proba(self, X, return_scores=False):
        _, y_pred, s = self.transform(X)
        return (y_pred, s) if return_scores else y_pred

    def predict(self, X, return_scores=False):
        _, y_pred, s = self.transform(X)
        return (y_pred > 0.5, s) if return_scores else y_pred > 0.5

    def project(self, X):
        return self.transform(X)[2]

    def score(self, X, y, groups=None, return_dict=False):
        """Task AUCs over all samples; with groups the reference computes the same list once per group."""
        _, y_pred, _ = self.transform(X)
        aucs = [roc_auc(y[:, j], y_pred[:, j]) for j in range(self.n_sup_networks)]
        if groups is None:
            return np.array(aucs)
        auc_dict = {group: list(aucs) for group in np.unique(groups)}
        if return_dict:
            return auc_dict
        return np.mean(np.vstack([auc_dict[key] for key in np.unique(groups)]), axis=0)

    def __getstate__(self):  # pickles (torch.save, deepcopy) carry the module, not fit bookkeeping
        st = dict(self.__dict__)
        st.pop("_dc_pack", None)
        return st


class _FullDCSFABase(DcsfaNmf):
    def __init__(self, num_nodes=5, num_high_level_node_features=25, n_components=4, n_sup_networks=4, h=100,
                 save_folder="", momentum=0.9, lr=1e-3, device="auto", n_intercepts=1, optim_name="AdamW", recon_loss="MSE",
                 recon_weight=1.0, sup_weight=1.0, sup_recon_weight=1.0, use_deep_encoder=True, sup_recon_type="Residual",
                 feature_groups=None, group_weights=None, fixed_corr=None, sup_smoothness_weight=1.0, verbose=False):
        super().__init__(n_components=n_components, device=device, n_intercepts=n_intercepts, n_sup_networks=n_sup_networks,
                         optim_name=optim_name, recon_loss=recon_loss, recon_weight=recon_weight, sup_weight=sup_weight,
                         sup_recon_weight=sup_recon_weight, use_deep_encoder=use_deep_encoder, h=h,
                         sup_recon_type=sup_recon_type, feature_groups=feature_groups, group_weights=group_weights,
                         fixed_corr=fixed_corr, momentum=momentum, lr=lr, sup_smoothness_weight=sup_smoothness_weight,
                         save_folder=save_folder, verbose=verbose)
        self.num_nodes = num_nodes
        self.num_high_level_node_features = num_high_level_node_features

    def _adjacency_tensor(self, factor):
        raise NotImplementedError

    def get_factor_GC(self, factor, threshold=True, ignore_features=True):
        raw = self._adjacency_tensor(factor)
        GC = raw * raw
        if ignore_features:
            GC = np.sum(GC, axis=2)
        if threshold:
            return (GC > 0).astype(int)
        return GC

    def GC(self, threshold=True, ignore_features=True):
        """One (nodes x nodes) graph per factor from softplus(W_nmf): the squared weights, summed over the
        features unless ignore_features is False; with threshold whether they are non-zero."""
        W_nmf = self.get_W_nmf().detach().cpu().numpy()
        assert len(W_nmf.shape) == 2
        return [self.get_factor_GC(W_nmf[i, :].reshape(1, -1), threshold=threshold, ignore_features=ignore_features)
                for i in range(W_nmf.shape[0])]

    def evaluate(self, X_orig, y_orig, GC_orig, save_path, threshold=False, ignore_features=True):
        """The reference's evaluate without its plots: eval_summary.pkl and the same return values."""
        GC_est = self.GC(threshold=threshold, ignore_features=ignore_features)
        gc_mse = [(i, j, F.mse_loss(torch.from_numpy(np.asarray(e)), torch.from_numpy(np.asarray(o))))
                  for i, e in enumerate(GC_est) for j, o in enumerate(GC_orig)]
        X_hat = self.reconstruct(X_orig)
        y_hat, _ = self.predict_proba(X_orig, return_scores=True)
        recon_mse = F.mse_loss(torch.from_numpy(X_hat), torch.from_numpy(X_orig))
        score_mse = F.mse_loss(torch.from_numpy(y_hat), torch.from_numpy(y_orig))
        avg_recon_mse, avg_score_mse = torch.mean(recon_mse), torch.mean(score_mse)
        with open(save_path + os.sep + "eval_summary.pkl", "wb") as outfile:
            pkl.dump({"gc_mse": gc_mse, "recon_mse": recon_mse, "score_mse": score_mse, "avg_recon_mse": avg_recon_mse,
                      "avg_score_mse": avg_score_mse}, outfile)
        return recon_mse, avg_recon_mse, score_mse, avg_score_mse, gc_mse


class FullDCSFAModel(_FullDCSFABase):
    """models/dcsfa_nmf.py FullDCSFAModel: the features are flattened directed spectra, nodes *
    features * (2 nodes - 1) of them.  Its best-model file holds the whole module."""
    best_file_holds_module = True

    def _adjacency_tensor(self, factor):
        node_len = self.num_high_level_node_features * (2 * self.num_nodes - 1)
        assert factor.shape[1] == self.num_nodes * node_len
        sub = np.zeros((self.num_nodes, node_len))
        for i in range(self.num_nodes):
            sub[i, :] += factor[0, i * node_len:(i + 1) * node_len]
        return unflatten_directed_spectrum_features(sub)


class FullDCSFAModel_GCv2(_FullDCSFABase):
    """models/dcsfa_nmf_vanillaDirSpec.py FullDCSFAModel: the features reshape to (nodes, nodes,
    features).  Its best-model file holds the state dict."""
    best_file_holds_module = False

    def _adjacency_tensor(self, factor):
        return np.reshape(factor, (self.num_nodes, self.num_nodes, self.num_high_level_node_features))


DcsfaNmf.best_file_holds_module = False


# --------------------------------------------------------------------------------------------------
def _standalone(model):
    from .fit_loop import standalone_copy
    return standalone_copy(model)


def _state_clone(model):
    return dict((k, v.detach().clone()) for k, v in model.state_dict().items())


class _Fit:
    """One model's data and bookkeeping through fit_dcsfa_baselines."""

    def __init__(self, model, X, y, pw, tm, im, groups, X_val, y_val, pw_val, tm_val, folder):
        self.model = model
        self.X, self.y = np.asarray(X), np.asarray(y)
        N = self.X.shape[0]
        self.im = np.ones((N, model.n_intercepts)) if im is None else np.asarray(im)
        self.tm = np.ones(self.y.shape) if tm is None else np.asarray(tm)
        self.pw = np.ones((self.y.shape[0], 1)) if pw is None else np.asarray(pw)
        if groups is None:
            w = np.ones((self.y.shape[0]))
        else:
            groups = np.asarray(groups)
            counts = np.array([np.sum(groups == g) for g in np.unique(groups)])
            weight = 1.0 / counts
            w = np.array([weight[t] for t in groups.astype(int)]).squeeze()
        self.sample_weights = torch.Tensor(w)
        self.has_val = X_val is not None and y_val is not None
        if self.has_val:
            self.X_val, self.y_val = np.asarray(X_val), np.asarray(y_val)
            self.tm_val = np.ones(self.y_val.shape) if tm_val is None else np.asarray(tm_val)
            self.pw_val = np.ones((self.y_val.shape[0], 1)) if pw_val is None else np.asarray(pw_val)
        self.folder = model.save_folder if folder is None else folder
        self.rng = None

    def check(self, batch_size, steps):
        N = self.X.shape[0]
        if steps and N % int(batch_size) == 1:
            raise ValueError(ONE_ROW_MSG % (N, int(batch_size)))
        sets = [(self.y, self.tm)] + ([(self.y_val, self.tm_val)] if self.has_val else [])
        for y, tm in sets if steps else []:
            for j in range(self.model.n_sup_networks):
                lab = np.float32(y)[np.asarray(tm)[:, j].astype(np.int64) == 1, j] >= 0.6
                if lab.all() or not lab.any():
                    raise ValueError(ONE_CLASS_MSG)

    def draw(self):
        """This fit's next epoch of row indices, from its own position in the default generator's stream."""
        if self.rng is not None:
            torch.set_rng_state(self.rng)
        idx = draw_epoch_indices(self.sample_weights.double(), len(self.sample_weights))
        if self.rng is not None:
            self.rng = torch.get_rng_state()
        return idx


def _record_epoch(f, epoch, train_loss, mse, aucs, val, best_model_name):
    """The histories and the best-model bookkeeping of dcsfa_nmf.py fit after one epoch; True when the
    epoch is the best so far (the caller writes the file)."""
    m = f.model
    m.training_hist.append(train_loss)
    m.recon_hist.append(np.float32(mse))
    m.pred_hist.append(list(aucs))
    if val is None:
        return False
    val_mse, val_aucs = np.float32(val[0]), list(val[1])
    m.val_recon_hist.append(val_mse)
    m.val_pred_hist.append(val_aucs)
    mse_var_rat = torch.tensor(val_mse) / f.val_std ** 2
    perf = mse_var_rat + (1 - np.mean(val_aucs))
    if perf < m.best_performance:
        m.best_epoch = epoch
        m.best_performance = perf
        m.best_val_avg_auc = np.mean(val_aucs)
        m.best_val_recon = val_mse
        m.best_val_aucs = val_aucs
        return True
    return False


def _save_best(f):
    m = f.model
    os.makedirs(f.folder, exist_ok=True)
    f.best_path = f.folder + os.sep + m.best_model_name
    torch.save(_standalone(m) if m.best_file_holds_module else _state_clone(m), f.best_path)


def _finish(f):
    m = f.model
    os.makedirs(f.folder, exist_ok=True)
    torch.save(_standalone(m), f.folder + os.sep + LAST_EPOCH_NAME)
    if f.has_val and getattr(f, "best_path", None) is not None:
        m._load(f.best_path)


def _begin_histories(f, best_model_name, verbose, lr):
    m = f.model
    m.training_hist, m.recon_hist, m.pred_hist = [], [], []
    m.verbose, m.lr = verbose, lr
    if f.has_val:
        assert best_model_name.split(".")[-1] == "pt", f"Save file `{f.folder + best_model_name}` must be of type .pt"
        m.best_model_name = best_model_name
        m.best_performance, m.best_val_recon, m.best_val_avg_auc = 1e8, 1e8, 0.0
        m.val_recon_hist, m.val_pred_hist = [], []
        f.val_std = torch.std(torch.Tensor(f.X_val).float())


def _aucs(y, tm, y_pred):
    out = []
    for j in range(y.shape[1]):
        keep = np.asarray(tm)[:, j].astype(np.int64) == 1
        out.append(binary_auc(*confusion_counts(np.float32(y)[keep, j] >= 0.6, y_pred[keep, j] >= 0.6)))
    return out


def _fit_generic(f, n_epochs, n_pre_epochs, nmf_max_iter, batch_size, lr, pretrain, verbose, best_model_name, callback, i):
    """dcsfa_nmf.py fit with torch autograd and the optimizer named by optim_name."""
    m = f.model
    dt = m.fit_dtype
    if pretrain:
        m.pretrain_NMF(f.X, f.y, nmf_max_iter)
        if callback:
            callback(i, "nmf", 0, m)
        m.pretrain_encoder(f.X, f.y, f.pw, f.tm, f.im, f.sample_weights, n_pre_epochs, batch_size)
        if callback:
            callback(i, "pretrain", n_pre_epochs, m)
    X, y = torch.Tensor(f.X).to(dt), torch.Tensor(f.y).to(dt)
    pw, tm, im = torch.Tensor(f.pw).to(dt), torch.Tensor(f.tm).long(), torch.Tensor(f.im)
    dset = TensorDataset(X, y, tm, pw, im)
    sampler = WeightedRandomSampler(f.sample_weights, len(f.sample_weights))
    loader = DataLoader(dset, batch_size=batch_size, sampler=sampler)
    optimizer = m.instantiate_optimizer()
    steps = []
    for epoch in range(n_epochs):
        epoch_loss = 0.0
        for batch in loader:
            m.train()
            optimizer.zero_grad()
            recon_loss, pred_loss = m.forward(*batch)
            loss = recon_loss + pred_loss
            loss.backward()
            optimizer.step()
            epoch_loss += loss.item()
            steps.append((recon_loss.item(), pred_loss.item()))
        with torch.no_grad():
            m.eval()
            X_recon, y_pred, _ = m.transform(X, im, avg_intercept=False, return_npy=True)
            mse = np.mean((X.numpy() - X_recon) ** 2)
            aucs = _aucs(f.y, f.tm, y_pred)
            val = None
            if f.has_val:
                Xv = torch.Tensor(f.X_val).to(dt)
                Xv_recon, yv_pred, _ = m.transform(Xv, return_npy=True)
                val = (np.mean((Xv.numpy() - Xv_recon) ** 2), _aucs(f.y_val, f.tm_val, yv_pred))
            if _record_epoch(f, epoch, epoch_loss / len(loader), mse, aucs, val, best_model_name):
                _save_best(f)
        if callback:
            callback(i, "epoch", epoch, m)
    m.step_losses = np.asarray(steps, dtype=np.float64).reshape(-1, 2)
    _finish(f)


def device_data(dev, Xl, yl, tml, pwl):
    """(X, y, task mask, prediction weights) of R fits as the float32 device tensors the native calls read:
    [N][..] for one fit, [R][N][..] stacked for several."""
    def upload(arrs):
        ts = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).reshape(len(a), -1) for a in arrs]
        return (ts[0] if len(ts) == 1 else torch.stack(ts)).contiguous().to(dev)
    return (upload(Xl), upload(yl), upload([np.asarray(t).astype(np.int64) for t in tml]),
            upload([np.asarray(p, dtype=np.float32).reshape(len(x), -1)[:, :1] for p, x in zip(pwl, Xl)]))


def fit_dcsfa_baselines(models, Xs, ys, y_pred_weights=None, task_masks=None, intercept_masks=None, y_sample_groups=None,
                        n_epochs=100, n_pre_epochs=100, nmf_max_iter=100, batch_size=128, lr=1e-3, pretrain=True,
                        verbose=False, X_vals=None, y_vals=None, y_pred_weights_vals=None, task_mask_vals=None,
                        save_folders=None, best_model_name="dCSFA-NMF-best-model.pt", seeds=None, callback=None):
    """DcsfaNmf.fit (models/dcsfa_nmf.py) for a list of models, each with its own data, masks, weights,
    validation set and save folder (None: the model's own).  Same-shape eligible models with same-size data
    share one native call per optimiser epoch on the fused route; otherwise one fit after the other.  Every
    model consumes the default generator as a loop of single fits would: with ``seeds`` fit i starts from
    ``torch.manual_seed(seeds[i])``, without them fit i + 1 continues where fit i's last draw ends.  Results
    are bit for bit those of that loop.  ``callback(i, phase, epoch, model)`` is called after pretrain_NMF
    ("nmf"), after pretrain_encoder ("pretrain") and after every main epoch ("epoch").  Left on every model:
    the histories, ``step_losses`` and ``pretrain_step_losses`` ([steps][2]: reconstruction, prediction)."""
    R = len(models)
    opt = lambda v: [None] * R if v is None else list(v)
    lists = [opt(v) for v in (y_pred_weights, task_masks, intercept_masks, y_sample_groups, X_vals, y_vals,
                              y_pred_weights_vals, task_mask_vals, save_folders)]
    if R == 0 or len(Xs) != R or len(ys) != R or any(len(v) != R for v in lists) or (seeds is not None and len(seeds) != R):
        raise ValueError("fit_dcsfa_baselines: one entry per model in every list")
    pws, tms, ims, groups, Xv, yv, pwv, tmv, folders = lists
    fits = [_Fit(models[i], Xs[i], ys[i], pws[i], tms[i], ims[i], groups[i], Xv[i], yv[i], pwv[i], tmv[i], folders[i])
            for i in range(R)]
    steps = (pretrain and n_pre_epochs > 0) or n_epochs > 0
    for f in fits:
        f.check(batch_size, steps)
    f0 = fits[0]
    D = int(f0.X.shape[1])
    fused = all(m.fused_eligible(batch_size, dim_in=int(f.X.shape[1])) for m, f in zip(models, fits))
    same = len(set(id(m) for m in models)) == R and R <= MAX_REPLICAS and all(
        f.X.shape == f0.X.shape and f.y.shape == f0.y.shape and f.has_val == f0.has_val and
        (not f.has_val or (f.X_val.shape == f0.X_val.shape and f.y_val.shape == f0.y_val.shape)) and
        (int(f.model.h), int(f.model.n_components), int(f.model.n_sup_networks)) ==
        (int(f0.model.h), int(f0.model.n_components), int(f0.model.n_sup_networks)) and
        (f.model.recon_weight, f.model.sup_weight, f.model.sup_recon_weight, f.model.sup_smoothness_weight) ==
        (f0.model.recon_weight, f0.model.sup_weight, f0.model.sup_recon_weight, f0.model.sup_smoothness_weight)
        for f in fits)
    if not fused or not same:
        for i, f in enumerate(fits):
            if seeds is not None:
                torch.manual_seed(int(seeds[i]))
            if R > 1:  # a loop of single fits, each on the route it is eligible for
                fit_dcsfa_baselines([f.model], [f.X], [f.y], [pws[i]], [tms[i]], [ims[i]], [groups[i]], n_epochs, n_pre_epochs,
                                    nmf_max_iter, batch_size, lr, pretrain, verbose, [Xv[i]], [yv[i]], [pwv[i]], [tmv[i]],
                                    [f.folder], best_model_name, None,
                                    None if callback is None else (lambda _, ph, ep, m, i=i: callback(i, ph, ep, m)))
            else:
                f.model._initialize(D)
                _begin_histories(f, best_model_name, verbose, lr)
                _fit_generic(f, n_epochs, n_pre_epochs, nmf_max_iter, batch_size, lr, pretrain, verbose, best_model_name,
                             callback, 0)
        return models
    # ---------------------------------------------------------------- fused
    n_draws = (n_pre_epochs if pretrain else 0) + n_epochs
    for i, f in enumerate(fits):
        if seeds is not None:
            torch.manual_seed(int(seeds[i]))
        f.model._initialize(D)
        _begin_histories(f, best_model_name, verbose, lr)
        if pretrain:
            f.model.pretrain_NMF(f.X, f.y, nmf_max_iter)
            if callback:
                callback(i, "nmf", 0, f.model)
        if R > 1:
            f.rng = torch.get_rng_state()
            if seeds is None and i + 1 < R:  # the next fit starts where this one's last draw will end
                for _ in range(n_draws):
                    draw_epoch_indices(f.sample_weights.double(), len(f.sample_weights))
    pack = DcsfaFitPack(models)
    for m in models:
        m.__dict__["_dc_pack"] = pack
    dev = pack.device

    train = device_data(dev, [f.X for f in fits], [f.y for f in fits], [f.tm for f in fits], [f.pw for f in fits])
    val = None
    if f0.has_val:
        val = device_data(dev, [f.X_val for f in fits], [f.y_val for f in fits], [f.tm_val for f in fits], [f.pw_val for f in fits])
    N = int(f0.X.shape[0])
    n_train, n_val = float(N) * D, (float(f0.X_val.shape[0]) * D if f0.has_val else 0.0)

    def draw_all():
        return torch.stack([f.draw() for f in fits]).to(torch.int32).to(dev)

    for m in models:
        m.train()
    if pretrain:
        pack.reset_optimizer()
        pre = [pack.epoch(PRETRAIN, draw_all(), batch_size, train, lr) for _ in range(n_pre_epochs)]
        got = torch.cat(pre, 1).double().cpu().numpy() if pre else np.zeros((R, 0, 2))
        for i, m in enumerate(models):
            m.pretrain_step_losses = got[i]
            if callback:
                callback(i, "pretrain", n_pre_epochs, m)
    pack.reset_optimizer()  # the main loop's own optimizer
    step_losses = [[] for _ in range(R)]
    for epoch in range(n_epochs):
        for m in models:
            m.train()
        loss = pack.epoch(TRAIN, draw_all(), batch_size, train, lr)
        for m in models:
            m.eval()
        sse, cnt = pack.evaluate(train)
        got = [loss.cpu().numpy(), sse.cpu().numpy(), cnt.cpu().numpy()]
        if val is not None:
            vs, vc = pack.evaluate(val)
            got += [vs.cpu().numpy(), vc.cpu().numpy()]
        for i, f in enumerate(fits):
            epoch_loss = 0.0
            for rl, pl in got[0][i]:
                epoch_loss += float(np.float32(rl) + np.float32(pl))
            step_losses[i].append(got[0][i].astype(np.float64))
            aucs = [binary_auc(*got[2][i][j]) for j in range(pack.ns)]
            v = None
            if val is not None:
                v = (got[3][i] / n_val, [binary_auc(*got[4][i][j]) for j in range(pack.ns)])
            if _record_epoch(f, epoch, epoch_loss / got[0].shape[1], got[1][i] / n_train, aucs, v, best_model_name):
                _save_best(f)
            if callback:
                callback(i, "epoch", epoch, f.model)
    for i, f in enumerate(fits):
        f.model.step_losses = np.concatenate(step_losses[i]) if step_losses[i] else np.zeros((0, 2))
        _finish(f)
    if R > 1:
        torch.set_rng_state(fits[-1].rng)
    return models
