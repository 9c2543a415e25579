"""What the comparison baselines' fused routes share on the host: the replica pack whose rows
hold R same-shape models' parameters and torch.optim.Adam state (``AdamPack``), the model-side slot that
finds a model's pack, the route switch, the acquisition of a pack for a list of fits, and the packing helpers.

Plain torch and ctypes: nothing here needs a GPU (tests/test_packs_host.py runs it on CPU tensors); the
concrete packs keep their device checks.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat


def route_from_env(var, default="fused"):
    """'fused' or 'generic' from the environment variable `var` (read per call; unset or empty: `default`)."""
    v = os.environ.get(var, "") or default
    if v not in ("fused", "generic"):
        raise ValueError("%s must be 'fused' or 'generic', not %r" % (var, v))
    return v


def mean_mse(criterion):
    return type(criterion) is nn.MSELoss and criterion.reduction == "mean"


def plain_adam(optimizer, params):
    """`optimizer` is a torch.optim.Adam of one group over exactly `params`, without amsgrad, maximize or
    decoupled weight decay: the update the fused steps implement."""
    if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
        return False
    g = optimizer.param_groups[0]
    if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay", False):
        return False
    return set(id(p) for p in g["params"]) == set(id(p) for p in params)


def require_plain_adam(opt, params, what, where):
    """plain_adam as a bind-time check of the model `what` (fitted with one Adam at the reference's `where`):
    raise for what the fused step does not implement."""
    if not isinstance(opt, torch.optim.Adam):
        raise NotImplementedError("the fused %s step implements torch.optim.Adam (%s)" % (what, where))
    if len(opt.param_groups) != 1:
        raise NotImplementedError("one parameter group per optimizer expected")
    grp = opt.param_groups[0]
    if grp.get("amsgrad") or grp.get("maximize") or grp.get("decoupled_weight_decay", False):
        raise NotImplementedError("amsgrad / maximize / decoupled weight decay are not used by %s" % what)
    if set(id(x) for x in grp["params"]) != set(id(x) for x in params):
        raise ValueError("the optimizer must own exactly model.gen_model.parameters()")


def pack_by_layout(row, prms, layout):
    """Move `prms` into the packed row: each becomes the view of `row` its layout entry (name, offset,
    shape) names, with its values."""
    with torch.no_grad():
        for prm, (_, off, shp) in zip(prms, layout):
            view = row[off:off + prm.numel()].view(shp)
            view.copy_(prm.detach().to(row.device, torch.float32).reshape(shp))
            prm.data = view


def adopt_bn_stats(bn, rm, rv):
    """A BatchNorm's running statistics become the pack's rows rm / rv, with their values."""
    with torch.no_grad():
        rm.copy_(bn.running_mean)
        rv.copy_(bn.running_var)
    bn.running_mean, bn.running_var = rm, rv


def stack_upload(xs, device):
    """Host tensors, one per fit -> (device tensor, per-fit stride in elements).  A lone fit's pack may hold
    other rows: a zero stride serves this model's row."""
    if len(xs) == 1:
        return xs[0].to(device), 0
    X = torch.stack(xs).to(device)
    return X, X[0].numel()


def acquire(models, optimizers, PackClass):
    """The pack a fused fit of `models` runs in, with every optimizer bound: (pack, rows, active).  One model
    keeps the slot it has (a pack of its own unless it sits in one); several get a new PackClass.  `active`
    is the native calls' replica list: None when the fits are all of the pack's rows."""
    R = len(models)
    if R == 1:
        pack, r0 = models[0]._slot()
        rows = [r0]
    else:
        pack = PackClass(models)
        rows = list(range(R))
    for i in range(R):
        pack.bind_optimizer(rows[i], optimizers[i])
    return pack, rows, None if (R > 1 or pack.R == 1) else rows


class PackSlot:
    """Mixin of a packed nn.Module: `_slot_key` names the entry of its __dict__ that holds (pack, row),
    `_pack_class` builds a pack of one, `_unpickled` lists further keys a pickle leaves behind."""
    _slot_key, _pack_class, _unpickled = None, None, ()

    def _slot(self):
        """(pack, row) holding this model's parameters; a pack of its own unless it sits in one."""
        slot = self.__dict__.get(self._slot_key)
        if slot is None or not slot[0].bound(slot[1]):
            self._pack_class([self])
            slot = self.__dict__[self._slot_key]
        return slot

    def __getstate__(self):  # pickles (torch.save, deepcopy) carry the module, not its pack
        st = dict(self.__dict__)
        for k in (self._slot_key,) + tuple(self._unpickled):
            st.pop(k, None)
        return st


class AdamPack:
    """R same-shape models whose parameters are views of par[r] and whose torch.optim.Adam state (exp_avg,
    exp_avg_sq, step) are views of m[r], v[r] and of a per-row step tensor, so that the native calls and
    torch step the same memory.  A subclass allocates, moves its models' parameters into the rows and
    calls ``adopt`` per row; it may override the four hooks below."""

    def allocate(self, models, size, device):
        self.models = list(models)
        self.R = len(self.models)
        self.device = device
        self.np_ = int(size)
        self.par = torch.empty(self.R, self.np_, device=device, dtype=torch.float32)
        self.m = torch.zeros_like(self.par)
        self.v = torch.zeros_like(self.par)
        self.opt = [None] * self.R
        self.hyper_key, self.hyper_dev = None, None
        self.ws = None
        self.params, self.ptrs = [], []

    def adopt(self, r, prms):
        """Row r (the next one) holds `prms`: record where they point and give the model its slot."""
        self.params.append(list(prms))
        self.ptrs.append(self._pointers(r))
        mod = self.models[r]
        mod.__dict__[mod._slot_key] = (self, r)

    def adopt_views(self, r, pairs):
        """adopt for a layout given as (parameter, view of par[r]) pairs (kernels.factor_views, lstm_views):
        the parameters become those views, with their values."""
        with torch.no_grad():
            torch._foreach_copy_([v for _, v in pairs],
                                 [prm.detach().to(self.device).reshape(v.shape) for prm, v in pairs])
        for prm, view in pairs:
            prm.data = view
        self.adopt(r, [prm for prm, _ in pairs])

    # ------------------------------------------------------------------ hooks
    def extra_pointers(self, r):
        """Addresses beside the parameters' that `bound` watches."""
        return []

    def stepped_parameters(self, r):
        """The parameters Adam holds state for."""
        return self.params[r]

    def check_optimizer(self, r, opt):
        """Raise unless `opt` can be bound to row r."""

    def replica_terms(self, r):
        """{ReplicaHyper field: value} of row r beside the Adam group B (the hyper cache's key entry too)."""
        return {}

    # ------------------------------------------------------------------ binding
    def _pointers(self, r):
        return [prm.data_ptr() for prm in self.params[r]] + self.extra_pointers(r)

    def bound(self, r):
        """Model r's parameters still point where the pack put them."""
        return self._pointers(r) == self.ptrs[r]

    def _span(self, r, prm):
        off = (prm.data_ptr() - self.par[r].data_ptr()) // 4
        return slice(off, off + prm.numel())

    def bind_optimizer(self, r, opt):
        st = self.opt[r]
        if st is not None and st["opt"] is opt:
            st["t"] = int(float(st["step"][0]))  # stepped by torch in between (the generic route)
            return st
        self.check_optimizer(r, opt)
        stepped = self.stepped_parameters(r)
        step = 0
        with torch.no_grad():
            self.m[r].zero_()
            self.v[r].zero_()
            for prm in stepped:
                s = opt.state.get(prm)
                if s and "exp_avg" in s:  # resume from a torch-stepped (or another pack's) optimizer
                    self.m[r, self._span(r, prm)] = s["exp_avg"].reshape(-1)
                    self.v[r, self._span(r, prm)] = s["exp_avg_sq"].reshape(-1)
                    step = int(float(s["step"]))
        # one element per parameter, as torch increments every parameter's step: one fill_ sets them all
        st = {"opt": opt, "t": step, "step": torch.full((max(len(stepped), 1),), float(step), dtype=torch.float32)}
        for i, prm in enumerate(stepped):
            opt.state[prm] = {"step": st["step"][i], "exp_avg": self.m[r, self._span(r, prm)].view_as(prm),
                              "exp_avg_sq": self.v[r, self._span(r, prm)].view_as(prm)}
        self.opt[r] = st
        return st

    def _adam(self, r):
        st = self.opt[r]
        if st is None:
            return (0.0, (0.9, 0.999), 1e-8, 0.0)
        g = st["opt"].param_groups[0]
        return (float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"]))

    def hyper(self, t_base, reps):
        """Device RedcliffReplicaHyper[R]: replica_terms and B = Adam; the Adam step number of a replica r
        in `reps` is the launch's tB + t[r] - t_base.  Uploaded only when a value changed."""
        key = tuple((tuple(self.replica_terms(r).items()), self._adam(r),
                     (self.opt[r]["t"] - t_base) if (self.opt[r] and r in reps) else 0) for r in range(self.R))
        if key != self.hyper_key:
            raw = b""
            for terms, adam, toff in key:
                h = nat.ReplicaHyper()
                h.bn_eps, h.bn_momentum = 1e-5, 0.1  # unused without BatchNorm
                for name, value in terms:
                    setattr(h, name, value)
                h.A = nat.adam_hyper(0.0, (0.9, 0.999), 1e-8, 0.0)
                h.B = nat.adam_hyper(*adam)
                h.B.t_offset = int(toff)
                raw += bytes(h)
            self.hyper_dev = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(self.device)
            self.hyper_key = key
        return self.hyper_dev

    # ------------------------------------------------------------------ calls
    def reps(self, active):
        """The rows a call steps: `active`, or all of them for None."""
        return list(range(self.R)) if active is None else list(active)

    def require_optimizers(self, reps):
        for r in reps:
            if self.opt[r] is None:
                raise RuntimeError("bind_optimizer before a stepping call")

    def advance(self, reps, nsteps):
        """The rows `reps` have taken nsteps more Adam steps."""
        for r in reps:
            st = self.opt[r]
            st["t"] += nsteps
            st["step"].fill_(float(st["t"]))

    def workspace_of(self, floats):
        """A device workspace of at least `floats` floats: kept, and replaced only by a larger one."""
        if self.ws is None or self.ws.numel() < floats:
            self.ws = None  # release before the larger allocation
            self.ws = torch.empty(floats, device=self.device, dtype=torch.float32)
        return self.ws
