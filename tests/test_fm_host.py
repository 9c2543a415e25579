"""CPU-side checks of the cMLP forecasting baseline (redcliff_amd.cmlp_fm, csrc/rc_fm.hip): a
plain-torch restatement of the model against the reference fixture tests/golden/cmlp_fm.npz (the
GPU tests use it as their oracle for shapes the fixture lacks), the packed layout, the limit
predicate against redcliff_fm_supported, the argument and limit checks of redcliff_fm_run, the
kernel's resource metadata and the route switch.  No kernel is launched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, assert_close
from test_kernel_occupancy import _kernels

STATE_RTOL, STATE_ATOL = 2e-4, 5e-6  # the project's state bound (compare_state)
RTOL, ATOL = 1e-4, 1e-6              # validation terms and fit histories
KERNEL_IDS = ("supports", "emb_fwd", "fac_fwd", "fac_bwd", "emb_bwd", "emb_final", "fac_mix", "emb_combine", "fac_lead",
              "score", "score_graphs", "score_cemb")


# ------------------------------------------------------------------------------------------ fixture
_FIXTURE = {}


def load_fm(name):
    """(meta, {key: array}) of one scenario of cmlp_fm.npz (read once, never modified)."""
    if not _FIXTURE:
        d = np.load(os.path.join(GOLDEN, "cmlp_fm.npz"), allow_pickle=False)
        for k in d.files:
            s, rest = k.split("/", 1)
            _FIXTURE.setdefault(s, {})[rest] = d[k]
        for s in _FIXTURE:
            for v in _FIXTURE[s].values():
                v.setflags(write=False)
    sc = _FIXTURE[name]
    return json.loads(str(sc["meta"])), sc


def sub(sc, prefix):
    pre = prefix + "/"
    return dict((k[len(pre):], v) for k, v in sc.items() if k.startswith(pre))


def coeffs(meta):
    return {"FORECAST_COEFF": meta["forecast"], "ADJ_L1_REG_COEFF": meta["adj"], "DAGNESS_REG_COEFF": 0.0,
            "DAGNESS_LAG_COEFF": 0.0, "DAGNESS_NODE_COEFF": 0.0}


def batches(X, B):
    X = torch.from_numpy(np.array(X))
    return [(X[i:i + B], None) for i in range(0, X.shape[0], B)]


def compare_state_dict(tag, got, want, rtol=STATE_RTOL, atol=STATE_ATOL):
    """compare_state's bound on {key: array} dicts."""
    assert set(got) == set(want), tag
    for k in want:
        scale = max(1.0, float(np.abs(want[k]).max()))
        assert_close("%s/%s" % (tag, k), got[k], want[k], rtol, atol * scale)


# ------------------------------------------------------------------------------------------ restatement
class TorchFM:
    """models/cmlp_fm.py:96-201, 419-475 in plain torch on stacked weights W0 (p, h, p, L), b0 (p, h),
    W1 (p, h), b1 (p): network j is Conv1d(p, h, L) -> ReLU -> Conv1d(h, 1, 1) on window rows [0, L),
    the target is row L, the loss FORECAST * sum_j MSE_j + ADJ * sum_j sum_c ||W0[j][:, c, :]||_F,
    the optimizer torch.optim.Adam (element-wise, so stacking changes nothing)."""

    def __init__(self, state, forecast, adj, adam, dtype=torch.float32):
        p = 1 + max(int(k.split(".")[3]) for k in state)
        get = lambda j, s: torch.as_tensor(np.array(state["factors.0.networks.%d.layers.%s" % (j, s)])).to(dtype)
        self.W0 = torch.stack([get(j, "0.weight") for j in range(p)]).clone().requires_grad_(True)
        self.b0 = torch.stack([get(j, "0.bias") for j in range(p)]).clone().requires_grad_(True)
        self.W1 = torch.stack([get(j, "1.weight").reshape(-1) for j in range(p)]).clone().requires_grad_(True)
        self.b1 = torch.stack([get(j, "1.bias").reshape(()) for j in range(p)]).clone().requires_grad_(True)
        self.p, self.h, _, self.L = self.W0.shape
        self.forecast, self.adj = forecast, adj
        self.params = [self.W0, self.b0, self.W1, self.b1]
        self.opt = torch.optim.Adam(self.params, **adam) if adam is not None else None

    def predict(self, X):
        xin = X[:, :self.L, :].permute(0, 2, 1)  # (B, c, t)
        z = torch.einsum("jhct,bct->bjh", self.W0, xin) + self.b0
        return torch.einsum("jh,bjh->bj", self.W1, torch.relu(z)) + self.b1

    def gc(self):
        return torch.stack([torch.norm(self.W0[j], dim=(0, 2)) for j in range(self.p)])  # (j, c)

    def gc_lagged(self):
        return torch.stack([torch.norm(self.W0[j], dim=0) for j in range(self.p)])  # (j, c, t)

    def loss_terms(self, X, forecast_on=True, adj_on=True):
        res = self.predict(X) - X[:, self.L, :]
        sse = (res * res).sum(0)
        f = self.forecast * sum(sse[j] / X.shape[0] for j in range(self.p))
        a = self.adj * self.gc().sum()
        # a term that is switched off keeps a zero gradient (as a zero coefficient would), so Adam still
        # steps every parameter: weight decay and the step count go on
        return (f if forecast_on else 0. * f) + (a if adj_on else 0. * a), f, a, sse

    def batch_update(self, X, forecast_on=True, adj_on=True):
        self.opt.zero_grad()
        loss, _, _, sse = self.loss_terms(X, forecast_on, adj_on)
        loss.backward()
        self.opt.step()
        return sse.detach()

    def validate(self, loader, normalized=False):
        af = aa = acmb = 0.
        with torch.no_grad():
            for X, _ in loader:
                cmb, f, a, _ = self.loss_terms(X.to(self.W0.dtype))
                if normalized:
                    f = f / self.forecast if self.forecast > 0. else f
                    a = a / self.adj if self.adj > 0. else a
                af, aa, acmb = af + float(f), aa + float(a), acmb + float(cmb)
        n = len(loader)
        return af / n, aa / n, 0., 0., 0., acmb / n

    def state(self):
        out = {}
        for j in range(self.p):
            pre = "factors.0.networks.%d.layers." % j
            out[pre + "0.weight"] = self.W0[j].detach().numpy().copy()
            out[pre + "0.bias"] = self.b0[j].detach().numpy().copy()
            out[pre + "1.weight"] = self.W1[j].detach().numpy().reshape(1, -1, 1).copy()
            out[pre + "1.bias"] = self.b1[j].detach().numpy().reshape(1).copy()
        return out


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_torch_restatement_reproduces_the_fixture(name):
    meta, sc = load_fm(name)
    assert sc["X_train"].shape == (meta["N"], meta["L"] + 1, meta["p"])
    assert meta["adam"] == dict(lr=1e-3, eps=1e-4, weight_decay=1e-4)
    m = TorchFM(sub(sc, "init"), meta["forecast"], meta["adj"], meta["adam"])
    tr, va = batches(sc["X_train"], meta["B"]), batches(sc["X_val"], meta["B"])
    assert tr[-1][0].shape[0] == (meta["N"] % meta["B"] or meta["B"])
    for e in range(1, meta["epochs"] + 1):
        for X, _ in tr:
            m.batch_update(X)
        compare_state_dict("%s/epoch%d" % (name, e), m.state(), sub(sc, "epoch%d" % e))
    assert_close(name + "/val_raw", m.validate(va, False), sc["val_raw"], RTOL, ATOL)
    assert_close(name + "/val_norm", m.validate(va, True), sc["val_norm"], RTOL, ATOL)
    assert np.abs(sc["val_raw"][:2] - sc["val_norm"][:2]).max() > 1e-3 or meta["forecast"] == meta["adj"] == 1.0


def test_fixture_holds_a_whole_fit():
    meta, sc = load_fm("a")
    keys = set(k.split("/")[2] for k in sc if k.startswith("fit/pkl/"))
    assert keys == {"epoch", "avg_forecasting_loss", "avg_adj_penalty", "avg_dagness_reg_loss", "avg_dagness_lag_loss",
                    "avg_dagness_node_loss", "avg_combo_loss", "best_loss", "best_it", "f1score_histories",
                    "roc_auc_histories", "gc_factor_l1_loss_histories", "gc_factor_l1_loss_histories_rows"}
    assert sc["fit/GC"].shape == (2, meta["p"], meta["p"], meta["L"])
    assert set(sub(sc, "fit/final")) == set(sub(sc, "init"))
    # the first epoch of the fit is the first epoch of the batch_update run: the stop criterion
    # is its L1 of the max-normalised lagged estimate plus the validation forecasting loss
    m = TorchFM(sub(sc, "epoch1"), meta["forecast"], meta["adj"], None)
    g = m.gc_lagged().detach()
    l1 = float((g / g.max()).abs().sum())
    val = m.validate(batches(sc["X_val"], meta["B"]))
    assert_close("avg_forecasting_loss", [val[0]], sc["fit/pkl/avg_forecasting_loss"], RTOL, ATOL)
    assert_close("l1", [l1], sc["fit/pkl/gc_factor_l1_loss_histories"], RTOL, ATOL)
    assert_close("best_loss", l1 + val[0], sc["fit/pkl/best_loss"], RTOL, ATOL)


# ------------------------------------------------------------------------------------------ model / layout
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_seeded_construction_is_the_reference_init(name):
    import redcliff_amd
    meta, sc = load_fm(name)
    torch.manual_seed(meta["seed"])
    m = redcliff_amd.cMLP_FM(meta["p"], meta["L"], [meta["h"]], None, meta["L"], 1, coeffs(meta))
    sd = m.state_dict()
    want = sub(sc, "init")
    assert set(k for k in sd if k.startswith("factors.")) == set(want)
    assert set(k for k in sd if not k.startswith("factors.")) == set("gen_model.1." + k[len("factors."):] for k in want)
    for k, v in want.items():
        assert np.array_equal(sd[k].numpy(), v), k
    assert m.factor_score_embedder is None and m.gen_model[0] is None and m.gen_model[1] is m.factors
    assert m.num_factors_nK == 1 and m.FACTOR_SCORE_COEFF == 0. and m.num_series == meta["p"]
    opt = torch.optim.Adam(m.gen_model.parameters(), lr=1e-3, eps=1e-4, weight_decay=1e-4)
    assert len(opt.param_groups[0]["params"]) == 4 * meta["p"]


def test_packed_layout_is_factor_layout_in_parameter_order():
    import redcliff_amd
    from redcliff_amd import kernels
    p, L, h = 7, 3, 33
    torch.manual_seed(1)
    m = redcliff_amd.cMLP_FM(p, L, [h], None, L, 1, coeffs(dict(forecast=1., adj=1.)))
    o = kernels.factor_layout(1, p, h, L)
    assert (o["W0"], o["b0"], o["W1"], o["b1"], o["total"]) == (0, p * h * p * L, p * h * p * L + p * h,
                                                                 p * h * p * L + 2 * p * h, p * h * p * L + 2 * p * h + p)
    assert o["total"] == p * (h * p * L + 2 * h + 1)
    flat = torch.arange(o["total"], dtype=torch.float32)
    pairs = kernels.factor_views(flat, list(m.factors), p, h, L)
    params = list(m.gen_model.parameters())
    assert len(pairs) == len(params) and all(a is b for (a, _), b in zip(pairs, params))
    for j in range(p):
        W, b0, W1, b1 = [v for _, v in pairs[4 * j:4 * j + 4]]
        assert W.shape == (h, p, L) and float(W[0, 0, 0]) == o["W0"] + j * h * p * L
        assert float(W[1, 2, 1]) == o["W0"] + j * h * p * L + 1 * p * L + 2 * L + 1  # q = c*L + t
        assert float(b0[0]) == o["b0"] + j * h and float(W1[0, 0, 0]) == o["W1"] + j * h and float(b1[0]) == o["b1"] + j


# ------------------------------------------------------------------------------------------ C entries
def fm_args(d, **kw):
    """Arguments with dummy non-null pointers: every case below must be rejected (or return 0 for an
    empty call) before anything is dereferenced or launched."""
    from redcliff_amd import _native as nat
    a = nat.FMArgs()
    a.d = d
    a.flags = nat.LOSS_FORECAST | nat.LOSS_ADJ | nat.STEP_B | nat.VALUES
    a.B, a.tB, a.row0, a.N = 8, 1, 0, 20
    for f in ("X", "fac", "fac_m", "fac_v", "hyper", "sse", "pen"):
        setattr(a, f, 64)
    a.x_pstride, a.fac_stride = 0, 1000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_predicate_agrees_with_the_library_over_a_grid():
    from redcliff_amd import cmlp_fm as F
    n_yes = n_no = 0
    for p in (1, 4, 10, 12, 33, 64, 65):
        for L in (1, 2, 3, 7):
            for h in (1, 25, 50, 100, 128, 129):
                for Bmax, T, R, K in ((128, L + 1, 1, 1), (512, L + 4, 256, 1), (513, L + 1, 1, 1), (8, L, 1, 1),
                                      (8, L + 1, 257, 1), (8, L + 1, 1, 2)):
                    want = F.fm_shape_supported(p, L, h, Bmax, T, R, K)
                    got = F.fm_supported(p, L, h, Bmax, T, R, K)
                    assert (got > 0) == want, (p, L, h, Bmax, T, R, K, got)
                    if got:
                        assert got == F.fm_lds_floats(p, L, h)
                    n_yes, n_no = n_yes + bool(want), n_no + (not want)
    assert n_yes > 50 and n_no > 50
    # both sides of the LDS limit: at p = 10, L = 2 the footprint is 4*21h + 6h + 3 + 64*(23 + (h|1)) + 38
    assert F.fm_lds_floats(10, 2, 128) == 4 * 21 * 128 + 3 * 257 + 64 * (21 + 129 + 2) + 20 + 10 + 8
    edge = [(p, L, h) for p in (40, 48, 56, 64) for L in (1, 2) for h in range(1, 129)
            if F.fm_lds_floats(p, L, h) <= F.LDS_MAX_FLOATS < F.fm_lds_floats(p, L, h + 1)]
    assert edge
    for p, L, h in edge:
        assert F.fm_supported(p, L, h) == F.fm_lds_floats(p, L, h) and F.fm_supported(p, L, h + 1) == 0
    # the published baseline shapes fit
    assert F.fm_supported(10, 2, 50, 128) and F.fm_supported(12, 2, 25, 128) and F.fm_supported(10, 2, 128, 512)


def test_fm_run_argument_and_limit_checks():
    from redcliff_amd import _native as nat
    from redcliff_amd.cmlp_fm import fm_dims
    L = nat.lib()
    call = lambda a: L.redcliff_fm_run(ctypes.byref(a), None)
    good = lambda **kw: fm_dims(10, 2, 50, Bmax=128, T=3, R=3, **kw)
    EINVAL, ELIMIT = -1, -2
    assert L.redcliff_fm_run(None, None) == EINVAL
    # limits
    for d in (fm_dims(65, 2, 5, 8), fm_dims(10, 2, 129, 8), fm_dims(10, 2, 50, 513), fm_dims(10, 2, 50, 8, T=2),
              fm_dims(10, 2, 50, 8, R=257), fm_dims(10, 2, 50, 8, K=2), fm_dims(64, 2, 128, 8)):
        assert call(fm_args(d)) == ELIMIT
        assert b"limits" in L.redcliff_last_error()
        assert L.redcliff_fm_supported(ctypes.byref(d)) == 0
    assert L.redcliff_fm_supported(None) == 0
    for bad in (dict(p=0), dict(h=0), dict(L=0), dict(R=0), dict(Bmax=0)):
        d = good()
        for k, v in bad.items():
            setattr(d, k, v)
        assert call(fm_args(d)) == EINVAL
    # arguments
    for kw in (dict(X=None), dict(fac=None), dict(fac_m=None), dict(fac_v=None), dict(hyper=None), dict(sse=None),
               dict(pen=None), dict(B=0), dict(B=129), dict(N=-1), dict(row0=-1), dict(tB=0), dict(x_pstride=-1),
               dict(fac_stride=-1), dict(flags=nat.LOSS_FACTOR), dict(flags=nat.STEP_A | nat.STEP_B),
               dict(flags=nat.GRAD_ONLY | nat.VALUES)):
        assert call(fm_args(good(), **kw)) == EINVAL, kw
    # pen may be null without RC_VALUES, the moments without RC_STEP_B -- then only the empty call returns 0
    assert call(fm_args(good(), pen=None, flags=nat.LOSS_FORECAST | nat.STEP_B, N=0)) == 0
    assert call(fm_args(good(), fac_m=None, fac_v=None, flags=nat.LOSS_FORECAST | nat.VALUES, N=0)) == 0
    # the active list: strictly increasing indices < R, at most R entries
    for lst in ([0, 0], [1, 0], [0, 3], [-1], [0, 1, 2, 2]):
        arr = (ctypes.c_int32 * len(lst))(*lst)
        a = fm_args(good(), replicas=ctypes.cast(arr, ctypes.c_void_p), n_replicas=len(lst))
        assert call(a) == EINVAL, lst
        assert b"replica" in L.redcliff_last_error()
    arr = (ctypes.c_int32 * 2)(0, 2)
    assert call(fm_args(good(), replicas=ctypes.cast(arr, ctypes.c_void_p), n_replicas=-1)) == EINVAL
    # nothing to do: no launch, no error (the dummy pointers are never touched)
    assert call(fm_args(good(), N=0)) == 0
    assert call(fm_args(good(), replicas=ctypes.cast(arr, ctypes.c_void_p), n_replicas=0)) == 0


def test_fm_kernel_uses_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    mine = [k for k in ks if "k_fm_epoch" in k]
    assert len(mine) == 1, sorted(ks)
    assert ks[mine[0]]["scratch"] == 0
    assert ks[mine[0]]["vgpr"] <= 128  # two workgroups of 256 threads per CU's SIMDs at least


def test_abi_version_and_kernel_ids_are_unchanged():
    from redcliff_amd import _native as nat
    assert nat.ABI_VERSION == 10 and nat.lib().redcliff_abi_version() == 10
    assert nat.KERNEL_IDS == KERNEL_IDS
    assert "redcliff_fm_run" in nat.EXPORTED and "redcliff_fm_supported" in nat.EXPORTED
    assert ctypes.sizeof(nat.FMArgs) == ctypes.sizeof(nat.Dims) + 4 * 3 + 4 + 8 * 2 + 8 * 2 + 8 * 4 + 8 + 8 * 4 + 8 + 8


def test_route_switch(monkeypatch):
    import redcliff_amd
    from redcliff_amd import cmlp_fm as F
    monkeypatch.delenv("REDCLIFF_FM_PATH", raising=False)
    assert F.fm_path() == "fused"
    for v, want in (("fused", "fused"), ("generic", "generic"), ("", "fused")):
        monkeypatch.setenv("REDCLIFF_FM_PATH", v)
        assert F.fm_path() == want
    monkeypatch.setenv("REDCLIFF_FM_PATH", "eager")
    with pytest.raises(ValueError):
        F.fm_path()
    # a model on the CPU, with wavelets / several hidden layers / roll-outs is never on the fused route
    monkeypatch.setenv("REDCLIFF_FM_PATH", "fused")
    c = coeffs(dict(forecast=1., adj=1.))
    m = redcliff_amd.cMLP_FM(4, 2, [5], None, 2, 1, c)
    assert not m.fused_eligible(2, 1)  # parameters on the CPU
    assert redcliff_amd.cMLP_FM(4, 2, [5, 5], None, 2, 1, c).num_gen_hiddens == 2
    assert redcliff_amd.fit_baselines is F.fit_baselines
