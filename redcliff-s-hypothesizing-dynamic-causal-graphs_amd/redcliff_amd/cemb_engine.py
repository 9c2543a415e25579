"""Device state and fused gfx950 training step of a REDCLIFF-S fit whose factor-score embedder is
the cEmbedder (models/redcliff_factor_score_embedders.py:183-331).

``CEmbEngine`` is a ``PackedEngine`` (engine.py) with the embedder group A laid out as the packed
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

from . import _native as nat
from .engine import BMAX_LIMIT, PackedEngine, _stream, step_flags

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


class CEmbEngine(PackedEngine):
    WS_ERROR = (-2, "cemb workspace_bytes")

    def __init__(self, model):
        self.cemb = emb = model.factor_score_embedder
        self.eh = int(emb.hidden[0])
        self.cws = None  # the chain's second, cEmbedder-private workspace
        self._dims = model_dims(model)
        super().__init__(model, model.embed_lag, emb.networks[0].layers[0].weight.device)

    # ------------------------------------------------------------------ layout / binding
    def _emb_layout(self):
        return cemb_layout(self.K, self.eh, self.p, self.F)

    def _emb_pairs(self):
        return cemb_views(self.emb, list(self.cemb.networks), self.eh, self.p, self.F)

    def _lib_emb_params(self, d):
        return nat.lib().redcliff_cemb_param_count(ctypes.byref(d), self.eh)

    def ensure_bound(self):
        """Parameters re-pointed since the last step (the generic path's HipAdam, load_state_dict of
        a model copy, ...): take their current values, and the moments / step counts the bound
        optimizers hold now, into the packed buffers."""
        if self._params_bound() and all(self._state_is_ours(g) for g in ("A", "B")):
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

    # ------------------------------------------------------------------ workspaces
    def dims(self, Bmax, T):
        d = nat.Dims.from_buffer_copy(self._dims)  # model_dims(model), read once: every step asks for a Dims
        d.Bmax, d.T = int(Bmax), int(T)
        return d

    def _extra_workspaces(self, d):
        return {"cws": nat.lib().redcliff_cemb_workspace_bytes(ctypes.byref(d), self.eh)}

    # ------------------------------------------------------------------ step launch
    def _args(self, d, flags, X, lab):
        a = self._step_args(d, flags, X, lab)
        return a, nat.CEmbArgs(eh=self.eh, pad_=0, ws=self.cws.data_ptr(), ws_bytes=self.cws.numel() * 4)

    def run_steps(self, kinds, ds, oA, oB, rows=None, sizes=None, stats=None, d=None):
        """Run the update kinds of one phase over consecutive batches of the dataset dict `ds`
        (stage / cache_dataset): all of them, or those at rows / sizes.  There is no BatchNorm,
        so no statistics: `stats` is FitEngine.run_steps' and is ignored."""
        self.ensure_bound()
        rows, sizes, d = self._batches(ds, rows, sizes, d)
        for kind in kinds:
            flags, _ = step_flags(self.model, kind, self.nsup)
            flags &= ~nat.BN_TRAIN
            if flags == 0:
                continue
            self._bind_stepped(flags, oA, oB)
            a, ce = self._args(d, flags, ds["X"], ds["lab"])
            self._count_steps(flags, nat.train_steps(a, rows, sizes, _stream(), "cemb_train_steps", cemb=ce))
        gp = self.model.__dict__.get("_generic_path")
        if gp is not None:  # this engine's moments and step counts are the optimizers' state now
            for g, opt in (("A", oA), ("B", oB)):
                if self.opt[g] is not None and self.opt[g]["opt"] is opt:
                    gp._adams.pop(id(opt), None)

    def run_values(self, ds, d=None, confusion=True):
        """validate_training body over the batches of the dataset dict `ds`; returns (acc[8], confusion)."""
        self.ensure_bound()
        flags = nat.VALUES | (nat.CONFUSION if (confusion and self.nsup > 0) else 0)
        rows, sizes, d = self._batches(ds, None, None, d)
        self.acc.zero_()
        self.conf.zero_()
        a, ce = self._args(d, flags, ds["X"], ds["lab"])
        nat.train_steps(a, rows, sizes, _stream(), "cemb validate", cemb=ce)
        ns = max(self.nsup, 1)
        return self.acc.cpu().numpy(), self.conf.cpu().numpy().reshape(ns, ns)
