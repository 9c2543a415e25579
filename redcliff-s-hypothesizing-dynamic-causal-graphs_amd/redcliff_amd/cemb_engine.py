"""Device state and fused gfx950 training step of a REDCLIFF-S fit whose factor-score embedder is
the cEmbedder (models/redcliff_factor_score_embedders.py:183-331).

``CEmbEngine`` is ``FitEngine`` (engine.py) with the embedder group A laid out as the packed
cEmbedder parameters ``We0[K][eh][p][F] | be0[K][eh] | We1[K][eh] | be1[K]`` and the step run by
``redcliff_cemb_train_step`` (csrc/rc_cemb.hip + the matrix-core factor chain): the module
parameters are views of the packed buffers, the two ``torch.optim.Adam`` objects' moments views of
flat moment buffers with a shared step tensor, so ``state_dict()`` of the model and of the
optimizers round-trips, and a fit can move between this path and the generic one
(``REDCLIFF_CEMB_PATH``, read per call) at any step: whichever path runs next takes the
parameters, moments and step counts over from the tensors the optimizers hold.
"""
import ctypes
import os

import numpy as np
import torch

from . import _native as nat
from .engine import BMAX_LIMIT, FitEngine, _stream, select_labels, step_flags

ENV = "REDCLIFF_CEMB_PATH"
LIMITS = dict(p=64, K=16, h=128, eh=128, F=64, Bmax=BMAX_LIMIT)  # include/redcliff_hip.h; L <= F


def path_requested():
    """REDCLIFF_CEMB_PATH: 'generic' (default, also when unset) or 'fused'; read per call."""
    v = os.environ.get(ENV, "generic").strip().lower()
    if v in ("", "generic"):
        return "generic"
    if v == "fused":
        return "fused"
    raise ValueError("%s must be 'generic' or 'fused', got %r" % (ENV, v))


def cemb_layout(K, eh, p, F):
    """Offsets (floats) of the packed cEmbedder group (include/redcliff_hip.h)."""
    o = {"We0": 0}
    o["be0"] = o["We0"] + K * eh * p * F
    o["We1"] = o["be0"] + K * eh
    o["be1"] = o["We1"] + K * eh
    o["total"] = o["be1"] + K
    return o


def cemb_views(flat, networks, eh, p, F):
    """(param, view) pairs in ``parameters()`` order (network by network: layer-0 weight, bias,
    layer-1 weight, bias) mapping each cEmbedder parameter onto the packed layout."""
    K = len(networks)
    o = cemb_layout(K, eh, p, F)
    pairs = []
    for k, net in enumerate(networks):
        l0, l1 = net.layers[0], net.layers[1]
        pairs.append((l0.weight, flat[o["We0"] + k * eh * p * F:o["We0"] + (k + 1) * eh * p * F].view(eh, p, F)))
        pairs.append((l0.bias, flat[o["be0"] + k * eh:o["be0"] + (k + 1) * eh]))
        pairs.append((l1.weight, flat[o["We1"] + k * eh:o["We1"] + (k + 1) * eh].view(1, eh, 1)))
        pairs.append((l1.bias, flat[o["be1"] + k:o["be1"] + k + 1]))
    return pairs


def static_supported(model):
    """The configuration half of ``cembedder_fused_supported`` (no library call)."""
    emb = model.factor_score_embedder
    return (model.factor_score_embedder_type == "cEmbedder" and model.wavelet_level is None and model.num_sims == 1
            and len(model.gen_hidden) == 1 and len(emb.hidden) == 1
            and model.forward_pass_mode == "apply_factor_weights_after_sim_completion"
            and model.embed_lag >= model.gen_lag and emb.lag == model.embed_lag
            and model.primary_gc_est_mode == "conditional_factor_fixed_embedder"
            and "Freeze" not in model.training_mode)


def model_dims(model, Bmax=1, T=None):
    emb = model.factor_score_embedder
    F = model.embed_lag
    return nat.Dims(R=1, Bmax=int(Bmax), T=int(T if T is not None else F + 1), p=model.num_series, L=model.gen_lag,
                    K=model.num_factors_nK, h=model.gen_hidden[0], F=F, n=1, H=1, M1=1,
                    nsup=model.num_supervised_factors, use_sigmoid=int(bool(emb.use_sigmoid_restriction)),
                    sigmoid_ecc=float(emb.sigmoid_eccentricity_coeff or 0.0))


def shapes_supported(model, Bmax=1):
    """The library's own limit check (redcliff_cemb_workspace_bytes returns 0 outside it)."""
    d = model_dims(model, Bmax)
    return nat.lib().redcliff_cemb_workspace_bytes(ctypes.byref(d), int(model.factor_score_embedder.hidden[0])) != 0


class CEmbEngine(FitEngine):
    def __init__(self, model):
        self.model = model
        emb = model.factor_score_embedder
        self.cemb = emb
        self.p = model.num_series
        self.L = model.gen_lag
        self.K = model.num_factors_nK
        self.nsup = model.num_supervised_factors
        self.h = model.gen_hidden[0]
        self.F = model.embed_lag
        self.eh = int(emb.hidden[0])
        self.n = self.H = 1  # DGCNN-only dims: ignored by the cEmbedder chain
        self.Lmax = max(model.gen_lag, model.embed_lag)
        self.device = emb.networks[0].layers[0].weight.device
        self.sig = bool(emb.use_sigmoid_restriction)
        self.ecc = float(emb.sigmoid_eccentricity_coeff or 0.0)
        self._emb_layout()
        dev = self.device
        self.emb = torch.empty(self.eo["total"], device=dev, dtype=torch.float32)
        self.fac = torch.empty(self.fo["total"], device=dev, dtype=torch.float32)
        self.acc = torch.zeros(8, device=dev, dtype=torch.float64)
        self.conf = torch.zeros(max(self.nsup, 1) ** 2, device=dev, dtype=torch.int32)
        self.opt = {"A": None, "B": None}
        self.ws = self.cws = None
        self.ws_dims = None
        self.hyper_key = None
        self.hyper_dev = None
        self.dataset_cache = {}
        self.pack = None
        self.pack_index = None
        self.bind()

    # ------------------------------------------------------------------ layout / binding
    def _emb_layout(self):
        FitEngine._emb_layout(self)  # fo (factors); its DGCNN eo is replaced
        self.eo = cemb_layout(self.K, self.eh, self.p, self.F)

    def _emb_pairs(self):
        return cemb_views(self.emb, list(self.cemb.networks), self.eh, self.p, self.F)

    def bind(self, copy=True):
        with torch.no_grad():
            self.pairs = self._emb_pairs() + self._fac_pairs()
            if copy:
                views = [view for _, view in self.pairs]
                srcs = [prm.detach().to(view.device).reshape(view.shape) for prm, view in self.pairs]
                torch._foreach_copy_(views, srcs)
            for prm, view in self.pairs:
                prm.data = view
        self.bound_ptrs = [prm.data_ptr() for prm, _ in self.pairs]

    def ensure_bound(self):
        """Parameters re-pointed since the last step (the generic path's HipAdam, load_state_dict of
        a model copy, ...): take their current values, and the moments / step counts the bound
        optimizers hold now, into the packed buffers."""
        if [prm.data_ptr() for prm, _ in self.pairs] == self.bound_ptrs and all(
                self._state_is_ours(g) for g in ("A", "B")):
            return
        self.bind()
        for g in ("A", "B"):
            if self.opt[g] is not None:
                opt = self.opt[g]["opt"]
                self.opt[g] = None
                self.bind_optimizer(g, opt)

    def _state_is_ours(self, g):
        st = self.opt[g]
        if st is None:
            return True
        for prm in self._group_params(g):
            s = st["opt"].state.get(prm)
            if not s or s.get("step") is not st["step"]:
                return False
        return True

    def _group_params(self, g):
        n_emb = 4 * self.K
        pr = [prm for prm, _ in self.pairs]
        return pr[:n_emb] if g == "A" else pr[n_emb:]

    def invalidate(self):
        pass

    # ------------------------------------------------------------------ hyper-parameters
    def _hyper(self):
        m = self.model
        gA = self.opt["A"]["opt"].param_groups[0] if self.opt["A"] else None
        gB = self.opt["B"]["opt"].param_groups[0] if self.opt["B"] else None

        def adam(gr):
            if gr is None:
                return (0.0, (0.9, 0.999), 1e-8, 0.0)
            return (float(gr["lr"]), tuple(float(b) for b in gr["betas"]), float(gr["eps"]), float(gr["weight_decay"]))

        key = (m.FORECAST_COEFF, m.FACTOR_SCORE_COEFF, m.FACTOR_COS_SIM_COEFF, m.FACTOR_WEIGHT_L1_COEFF,
               getattr(m, "FACTOR_WEIGHT_SMOOTHING_PENALTY_COEFF", 0.0), m.ADJ_L1_REG_COEFF, adam(gA), adam(gB))
        if key != self.hyper_key:
            h = nat.ReplicaHyper()
            (h.c_forecast, h.c_factor, h.c_cos, h.c_fwl1, h.c_smooth, h.c_adj) = [float(x) for x in key[:6]]
            h.bn_eps, h.bn_momentum = 1e-5, 0.1  # unused: no BatchNorm
            h.A = nat.adam_hyper(*key[6])
            h.B = nat.adam_hyper(*key[7])
            raw = np.frombuffer(bytes(h), dtype=np.uint8).copy()
            self.hyper_dev = torch.from_numpy(raw).to(self.device)
            self.hyper_key = key
        return self.hyper_dev

    # ------------------------------------------------------------------ workspaces
    def dims(self, Bmax, T):
        return nat.Dims(R=1, Bmax=int(Bmax), T=int(T), p=self.p, L=self.L, K=self.K, h=self.h, F=self.F, n=1, H=1,
                        M1=1, nsup=self.nsup, use_sigmoid=int(self.sig), sigmoid_ecc=self.ecc)

    def check_device_status(self, where="check"):
        pass  # no cross-workgroup hand-off in this chain

    def workspace(self, Bmax, T):
        Bmax = max(int(Bmax), 1)
        if self.ws_dims is not None and self.ws_dims[0] >= Bmax:
            return self.dims(self.ws_dims[0], T)
        d = self.dims(Bmax, T)
        L = nat.lib()
        nb, ncb = L.redcliff_workspace_bytes(ctypes.byref(d)), L.redcliff_cemb_workspace_bytes(ctypes.byref(d), self.eh)
        if nb == 0 or ncb == 0:
            nat.check(-2, "cemb workspace_bytes")
        self.ws = torch.zeros(nb // 4, device=self.device, dtype=torch.float32)
        self.cws = torch.zeros(ncb // 4, device=self.device, dtype=torch.float32)
        self.ws_dims = (Bmax,)
        self.ws_off = nat.workspace_layout(d)
        return d

    # ------------------------------------------------------------------ data
    def stage(self, X, Y):
        """One host batch -> device tensors (X (B,T,p), labels (B,K)) and the dims."""
        X = X.to(self.device, torch.float32).contiguous()
        B, T, p = X.shape
        if p != self.p:
            raise ValueError("expected %d channels, got %d" % (self.p, p))
        lab = select_labels(Y.to(self.device), self.K, self.Lmax) if Y is not None else None
        return X, lab, self.workspace(B, T)

    def cache_dataset(self, loader):
        key = id(loader)
        if key in self.dataset_cache:
            return self.dataset_cache[key]
        xs, ys, sizes = [], [], []
        for X, Y in loader:
            xs.append(X.to(torch.float32))
            ys.append(select_labels(Y, self.K, self.Lmax) if Y is not None else torch.zeros(X.shape[0], self.K))
            sizes.append(int(X.shape[0]))
        Xall = torch.cat(xs, 0).to(self.device).contiguous()
        lab = torch.cat(ys, 0).to(self.device, torch.float32).contiguous()
        ds = {"X": Xall, "lab": lab, "rows": np.cumsum([0] + sizes[:-1]).astype(np.int64),
              "sizes": np.asarray(sizes, dtype=np.int32), "T": int(Xall.shape[1]), "Bmax": max(sizes),
              "len": len(sizes), "loader": loader}
        self.dataset_cache[key] = ds
        return ds

    # ------------------------------------------------------------------ step launch
    def _fresh_state(self):
        for g in ("A", "B"):
            st = self.opt[g]
            if st is not None:
                tv = int(float(st["step"]))
                if tv != st["t"]:
                    st["t"] = tv

    def _args(self, d, flags, X, lab):
        self._fresh_state()
        a = nat.StepArgs()
        a.d = d
        a.flags = flags
        a.n_bn_updates = 0
        stA, stB = self.opt["A"], self.opt["B"]
        a.tA = (stA["t"] + 1) if stA else 1
        a.tB = (stB["t"] + 1) if stB else 1
        a.X = X.data_ptr()
        a.labels = lab.data_ptr() if lab is not None else None
        a.emb, a.emb_stride = self.emb.data_ptr(), self.emb.numel()
        a.fac, a.fac_stride = self.fac.data_ptr(), self.fac.numel()
        a.emb_m, a.emb_v = (stA["m"].data_ptr(), stA["v"].data_ptr()) if stA else (self.emb.data_ptr(),) * 2
        a.fac_m, a.fac_v = (stB["m"].data_ptr(), stB["v"].data_ptr()) if stB else (self.fac.data_ptr(),) * 2
        a.hyper = self._hyper().data_ptr()
        a.ws, a.ws_bytes = self.ws.data_ptr(), self.ws.numel() * 4
        a.acc = self.acc.data_ptr()
        a.confusion = self.conf.data_ptr()
        ce = nat.CEmbArgs(eh=self.eh, pad_=0, ws=self.cws.data_ptr(), ws_bytes=self.cws.numel() * 4)
        return a, ce

    def _launch(self, a, ce, rows, sizes, what):
        rows_a = np.ascontiguousarray(rows, dtype=np.int64)
        sizes_a = np.ascontiguousarray(sizes, dtype=np.int32)
        nat.check(nat.lib().redcliff_cemb_train_steps(ctypes.byref(a), ctypes.byref(ce), len(rows_a),
                                                      rows_a.ctypes.data_as(ctypes.c_void_p),
                                                      sizes_a.ctypes.data_as(ctypes.c_void_p), _stream()), what)
        return len(rows_a)

    def run_steps(self, kinds, X, lab, d, rows, sizes, oA, oB):
        """Run the update kinds of one phase over consecutive batches (rows / sizes)."""
        self.ensure_bound()
        for kind in kinds:
            flags, _ = step_flags(self.model, kind, self.nsup)
            flags &= ~nat.BN_TRAIN
            if flags == 0:
                continue
            if flags & nat.STEP_A:
                self.bind_optimizer("A", oA)
            if flags & nat.STEP_B:
                self.bind_optimizer("B", oB)
            a, ce = self._args(d, flags, X, lab)
            n = self._launch(a, ce, rows, sizes, "cemb_train_steps")
            if flags & nat.STEP_A:
                self.opt["A"]["t"] += n
            if flags & nat.STEP_B:
                self.opt["B"]["t"] += n
            self._sync_steps()

    def run_values(self, X, lab, d, rows, sizes, confusion=True):
        """validate_training body over consecutive batches; returns (acc[8], confusion)."""
        self.ensure_bound()
        flags = nat.VALUES | (nat.CONFUSION if (confusion and self.nsup > 0) else 0)
        self.acc.zero_()
        self.conf.zero_()
        a, ce = self._args(d, flags, X, lab)
        self._launch(a, ce, rows, sizes, "cemb validate")
        ns = max(self.nsup, 1)
        return self.acc.cpu().numpy(), self.conf.cpu().numpy().reshape(ns, ns)
