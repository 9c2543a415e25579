"""GPU checks of the cLSTM forecasting baseline (redcliff_amd.clstm_fm, csrc/rc_lstm_fm.hip): both
routes against the reference fixture tests/golden/clstm_fm.npz, the bitwise invariants of
redcliff_lstm_fm_run (splitting, packing, the active list, guard bands, values-only calls), its
edge shapes against a float64 torch restatement kept here, and fit_lstm_baselines against the
models' own fits.  Comparisons are bitwise unless a bound is named.  The first generic-route case of a
process pays the GPU library's one-time set-up of nn.LSTM for its shape (seconds); the fused cases do not."""
import os
import pickle

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_lstm_fm_host import (RTOL, ATOL, batches, build_model, check_scenario, check_whole_fit, compare_state_dict,
                               load_lf)

pytestmark = pytest.mark.gpu


def F():
    from redcliff_amd import clstm_fm
    return clstm_fm


def nat():
    from redcliff_amd import _native
    return _native


@pytest.fixture(params=["fused", "generic"])
def route(request, monkeypatch):
    monkeypatch.setenv("REDCLIFF_LSTM_FM_PATH", request.param)
    return request.param


# ------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_batch_updates_and_validation_match_the_reference(name, route):
    meta, _ = load_lf(name)
    m = check_scenario(name, "cuda", nan_past_tmax=(name == "a"))  # a: the rows at and past Tm are never read
    assert m.fused_eligible(meta["C"], meta["Tm"], Bmax=meta["B"], T=meta["T"]) == (route == "fused")
    assert ("_lf_slot" in m.__dict__) == (route == "fused")
    prm = next(m.gen_model.parameters())
    assert prm.shape == (4 * meta["h"], meta["p"])


def test_fit_matches_the_reference(route, tmp_path):
    m = check_whole_fit("cuda", str(tmp_path))
    saved = torch.load(os.path.join(str(tmp_path), "final_best_model.bin"), weights_only=False)
    assert "_lf_slot" not in saved.__dict__  # the pickle carries the module, not its pack
    s1, s2 = m.state_dict(), saved.state_dict()
    assert all(torch.equal(s1[k], s2[k]) for k in s1)


# ------------------------------------------------------------------------------------------ restatement
def split_packed(flat, p, h):
    """{state_dict key: array} of one replica's packed block (kernels.lstm_layout)."""
    from redcliff_amd import kernels
    o = kernels.lstm_layout(p, h)
    flat = flat.detach().cpu().numpy()
    g = 4 * h
    out = {}
    for j in range(p):
        pre = "factors.0.networks.%d." % j
        out[pre + "lstm.weight_ih_l0"] = flat[o["Wih"] + j * g * p:o["Wih"] + (j + 1) * g * p].reshape(g, p).copy()
        out[pre + "lstm.weight_hh_l0"] = flat[o["Whh"] + j * g * h:o["Whh"] + (j + 1) * g * h].reshape(g, h).copy()
        out[pre + "lstm.bias_ih_l0"] = flat[o["bih"] + j * g:o["bih"] + (j + 1) * g].copy()
        out[pre + "lstm.bias_hh_l0"] = flat[o["bhh"] + j * g:o["bhh"] + (j + 1) * g].copy()
        out[pre + "linear.weight"] = flat[o["Wl"] + j * h:o["Wl"] + (j + 1) * h].reshape(1, h, 1).copy()
        out[pre + "linear.bias"] = flat[o["bl"] + j:o["bl"] + j + 1].copy()
    return out


class TorchLFM:
    """models/clstm_fm.py:56-177 in plain float64 torch on stacked weights Wih (p, 4h, p), Whh (p, 4h, h),
    bih / bhh (p, 4h), Wl (p, h), bl (p): network j is an LSTM cell (gate rows i | f | g | o, zero initial
    state) read out by Wl[j] . h_t + bl[j]; the sequences are the tmax - C overlapping windows of rows
    [0, tmax) of every recording, the loss FORECAST * sum_j MSE_j + ADJ * sum_j sum_c ||Wih[j][:, c]||_2,
    the optimizer torch.optim.Adam (element-wise, so stacking changes nothing)."""

    def __init__(self, flat, p, h, C, tmax, forecast, adj, adam):
        st = split_packed(flat, p, h)
        get = lambda j, s: torch.as_tensor(st["factors.0.networks.%d.%s" % (j, s)]).double()
        stack = lambda s, shape: torch.stack([get(j, s).reshape(shape) for j in range(p)]).clone().requires_grad_(True)
        self.Wih, self.Whh = stack("lstm.weight_ih_l0", (4 * h, p)), stack("lstm.weight_hh_l0", (4 * h, h))
        self.bih, self.bhh = stack("lstm.bias_ih_l0", (4 * h,)), stack("lstm.bias_hh_l0", (4 * h,))
        self.Wl, self.bl = stack("linear.weight", (h,)), stack("linear.bias", ())
        self.p, self.h, self.C, self.tmax, self.forecast, self.adj = p, h, C, tmax, forecast, adj
        self.params = [self.Wih, self.Whh, self.bih, self.bhh, self.Wl, self.bl]
        self.opt = torch.optim.Adam(self.params, **adam) if adam is not None else None

    def residuals(self, X):
        X = X.double()[:, :self.tmax]
        C, S, h = self.C, self.tmax - self.C, self.h
        inp = torch.stack([X[:, i:S + i] for i in range(C)], dim=2).reshape(-1, C, self.p)
        tgt = torch.stack([X[:, i + 1:S + i + 1] for i in range(C)], dim=2).reshape(-1, C, self.p)
        hh = torch.zeros(inp.shape[0], self.p, h, dtype=torch.float64)
        cc = torch.zeros_like(hh)
        ys = []
        for t in range(C):
            a = torch.einsum("jgc,qc->qjg", self.Wih, inp[:, t]) + self.bih + \
                torch.einsum("jgk,qjk->qjg", self.Whh, hh) + self.bhh
            i, f, g, o = a[..., :h], a[..., h:2 * h], a[..., 2 * h:3 * h], a[..., 3 * h:]
            cc = torch.sigmoid(f) * cc + torch.sigmoid(i) * torch.tanh(g)
            hh = torch.sigmoid(o) * torch.tanh(cc)
            ys.append(torch.einsum("jk,qjk->qj", self.Wl, hh) + self.bl)
        return torch.stack(ys, 1) - tgt  # (Bq, C, p)

    def gc(self):
        return torch.norm(self.Wih, dim=1)  # (j, c)

    def loss_terms(self, X, forecast_on=True, adj_on=True):
        res = self.residuals(X)
        sse = (res * res).sum((0, 1))
        f = self.forecast * (sse / (res.shape[0] * res.shape[1])).sum()
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

    def state(self):
        out = {}
        for j in range(self.p):
            pre = "factors.0.networks.%d." % j
            for key, t, shape in (("lstm.weight_ih_l0", self.Wih, None), ("lstm.weight_hh_l0", self.Whh, None),
                                  ("lstm.bias_ih_l0", self.bih, None), ("lstm.bias_hh_l0", self.bhh, None),
                                  ("linear.weight", self.Wl, (1, -1, 1)), ("linear.bias", self.bl, (1,))):
                v = t[j].detach().numpy().copy()
                out[pre + key] = v if shape is None else v.reshape(shape)
        return out


# ------------------------------------------------------------------------------------------ raw calls
def banded(shape, band, fill=None):
    """A tensor of `shape` inside a NaN-filled buffer with `band` floats on either side: (view, whole)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * band,), float("nan"), device="cuda", dtype=torch.float32)
    view = whole[band:band + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return view, whole


def bands_intact(whole, band):
    return bool(torch.isnan(whole[:band]).all()) and bool(torch.isnan(whole[whole.numel() - band:]).all())


class Raw:
    """Packed buffers of R replicas for direct redcliff_lstm_fm_run calls."""

    def __init__(self, p, h, C, tmax, R=1, N=20, B=8, seed=0, T=None, lrs=None, wd=1e-4, forecast=1.0, adj=0.1,
                 shared_x=False, band=0):
        self.p, self.h, self.C, self.tmax, self.R, self.N, self.B = p, h, C, tmax, R, N, B
        self.T = tmax if T is None else T
        self.n = p * (4 * h * (p + h + 2) + h + 1)
        self.lrs = lrs or [1e-3] * R
        self.wd, self.forecast, self.adj, self.band = wd, forecast, adj, band
        rng = np.random.RandomState(seed)
        fac = torch.from_numpy((0.3 * rng.randn(R, self.n)).astype(np.float32))
        X = torch.from_numpy(rng.randn(1 if shared_x else R, N, self.T, p).astype(np.float32))
        self.shared_x = shared_x
        self.fac, self.w_fac = banded((R, self.n), band, fac)
        self.m, self.w_m = banded((R, self.n), band, torch.zeros(R, self.n))
        self.v, self.w_v = banded((R, self.n), band, torch.zeros(R, self.n))
        self.X, self.w_X = banded(tuple(X.shape), band, X)
        raw = b""
        for r in range(R):
            hy = nat().ReplicaHyper()
            hy.c_forecast, hy.c_adj = forecast, adj
            hy.bn_eps, hy.bn_momentum = 1e-5, 0.1
            hy.A = nat().adam_hyper(0.0, (0.9, 0.999), 1e-8, 0.0)
            hy.B = nat().adam_hyper(self.lrs[r], (0.9, 0.999), 1e-4, wd)
            raw += bytes(hy)
        self.hyper = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
        self.wholes = [self.w_fac, self.w_m, self.w_v, self.w_X]

    def call(self, flags, row0=0, N=None, B=None, tB=1, replicas=None, want_G=False, expect=0):
        N = self.N - row0 if N is None else N
        B = self.B if B is None else B
        nrep = self.R if replicas is None else len(replicas)
        nsteps = -(-N // B)
        p = self.p
        sse, w_sse = banded((max(nrep, 1), nsteps, p), self.band)  # never a null pointer, even for an empty list
        pen, w_pen = banded((max(nrep, 1), nsteps, p), self.band)
        G, w_G = banded((self.R, p, p), self.band)
        d = F().lstm_fm_dims(p, self.h, Bmax=max(B, 1), T=self.T, R=self.R)
        rc = F().lstm_fm_run(d, self.C, self.tmax, flags, B, tB, row0, N, self.X,
                             0 if self.shared_x else self.N * self.T * p, self.fac, self.m, self.v, self.n, self.hyper,
                             sse, pen, G if want_G else None, replicas)
        assert rc == expect, (rc, nat().lib().redcliff_last_error())
        torch.cuda.synchronize()
        if self.band:
            for w in self.wholes + [w_sse, w_pen, w_G]:
                assert bands_intact(w, self.band)
        return sse, pen, G

    def snapshot(self):
        return [t.clone() for t in (self.fac, self.m, self.v)]

    def restore(self, snap):
        for t, s in zip((self.fac, self.m, self.v), snap):
            t.copy_(s)

    def oracle(self, r, lr=None):
        adam = dict(lr=self.lrs[r] if lr is None else lr, eps=1e-4, weight_decay=self.wd)
        return TorchLFM(self.fac[r], self.p, self.h, self.C, self.tmax, self.forecast, self.adj, adam)

    def x_cpu(self, r):
        return self.X[0 if self.shared_x else r].cpu()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def TRAIN():
    return F().FLAGS_TRAIN


def VALUES():
    return F().FLAGS_VALUES


def oracle_epoch(o, X, B, **kw):
    return torch.stack([o.batch_update(X[i:i + B], **kw) for i in range(0, X.shape[0], B)])


SHAPE = dict(p=7, h=13, C=3, tmax=7)  # S = 4 sequences per recording; a batch of 8 is one pass of 32


def test_epoch_call_equals_split_calls_and_single_batches():
    kw = dict(N=40, B=16, seed=3, **SHAPE)  # 64 sequences per batch = two passes, the last batch one
    raw = Raw(**kw)
    s0 = raw.snapshot()
    sse, pen, G = raw.call(TRAIN(), want_G=True)
    whole = raw.snapshot()
    # against the restatement, with the sums of squared residuals and penalties per step and the final norms
    o = Raw(**kw).oracle(0)
    want_pen = []
    want_sse = []
    X = raw.x_cpu(0)
    for i in range(0, 40, 16):
        want_pen.append(o.gc().sum(1).detach())
        want_sse.append(o.batch_update(X[i:i + 16]))
    compare_state_dict("epoch", split_packed(raw.fac[0], 7, 13), o.state())
    assert_close("sse", sse[0].cpu().numpy(), torch.stack(want_sse).numpy(), RTOL, ATOL)
    assert_close("pen", pen[0].cpu().numpy(), torch.stack(want_pen).numpy(), RTOL, ATOL)
    assert_close("G", G[0].cpu().numpy(), o.gc().detach().numpy(), RTOL, ATOL)
    # two runs agree
    raw.restore(s0)
    sse2, pen2, G2 = raw.call(TRAIN(), want_G=True)
    assert same(raw.snapshot(), whole) and torch.equal(sse, sse2) and torch.equal(G, G2) and torch.equal(pen, pen2)
    # [0, 32) + [32, 40) with tB advanced
    raw.restore(s0)
    a, _, _ = raw.call(TRAIN(), row0=0, N=32, tB=1)
    b, _, _ = raw.call(TRAIN(), row0=32, N=8, tB=3)
    assert same(raw.snapshot(), whole) and torch.equal(torch.cat([a, b], 1), sse)
    # nsteps one-batch calls
    raw.restore(s0)
    parts = [raw.call(TRAIN(), row0=r0, N=n, B=n, tB=t)[0] for t, (r0, n) in enumerate([(0, 16), (16, 16), (32, 8)], 1)]
    assert same(raw.snapshot(), whole) and torch.equal(torch.cat(parts, 1), sse)


def test_pack_equals_single_replicas_and_the_active_list():
    kw = dict(N=20, B=8, seed=5, **SHAPE)
    lrs = [1e-3, 3e-3, 1e-2]
    pack = Raw(R=3, lrs=lrs, **kw)
    s0 = pack.snapshot()
    sse, pen, G = pack.call(TRAIN(), want_G=True)
    for r in range(3):
        one = Raw(R=1, lrs=[lrs[r]], **dict(kw, seed=99))
        one.fac.copy_(s0[0][r:r + 1])
        one.X.copy_(pack.X[r:r + 1])
        s1, p1, G1 = one.call(TRAIN(), want_G=True)
        assert torch.equal(one.fac[0], pack.fac[r]) and torch.equal(one.m[0], pack.m[r])
        assert torch.equal(one.v[0], pack.v[r]) and torch.equal(s1[0], sse[r]) and torch.equal(G1[0], G[r])
        assert torch.equal(p1[0], pen[r])
    assert not torch.equal(pack.fac[0] - s0[0][0], pack.fac[2] - s0[0][2])
    # replicas = [0, 2]: replica 1 untouched, rows 0 / 1 of the outputs are replicas 0 / 2
    done = pack.snapshot()
    pack.restore(s0)
    s02, _, _ = pack.call(TRAIN(), replicas=[0, 2])
    now = pack.snapshot()
    for t0, t1, t2 in zip(s0, now, done):
        assert torch.equal(t1[1], t0[1]) and torch.equal(t1[0], t2[0]) and torch.equal(t1[2], t2[2])
    assert s02.shape[0] == 2 and torch.equal(s02[0], sse[0]) and torch.equal(s02[1], sse[2])
    # an empty list launches nothing
    before = pack.snapshot()
    pack.call(TRAIN(), replicas=[])
    assert same(pack.snapshot(), before)
    # one shared recording set (x_pstride == 0)
    sh = Raw(R=2, shared_x=True, **dict(kw, seed=6))
    f0 = sh.fac.clone()
    sh.call(TRAIN())
    for r in range(2):
        one = Raw(R=1, shared_x=True, **dict(kw, seed=6))
        one.fac.copy_(f0[r:r + 1])
        one.X.copy_(sh.X)
        one.call(TRAIN())
        assert torch.equal(one.fac[0], sh.fac[r])


@pytest.mark.parametrize("case", ["B1", "S1", "C1", "hmax", "Cmax", "p64", "wd0", "forecast_only", "adj_only"])
def test_edges_against_the_restatement(case):
    cfg = dict(N=20, B=8, seed=11, **SHAPE)
    flags, okw = TRAIN(), {}
    if case == "B1":  # four sequences per step
        cfg.update(N=3, B=1)
    elif case == "S1":  # one sequence per recording
        cfg.update(tmax=4, T=5)
    elif case == "C1":
        cfg.update(C=1, tmax=6)
    elif case == "hmax":  # the largest h the limits admit at p = 4, C = 2
        cfg.update(p=4, h=35, C=2, tmax=4, N=40, B=24)
        assert F().lstm_fm_supported(4, 35, 2, 24) and not F().lstm_fm_supported(4, 36, 2, 24)
    elif case == "Cmax":  # the longest context the limits admit at p = 4, h = 5
        cfg.update(p=4, h=5, C=34, tmax=36, N=40, B=24)
        assert F().lstm_fm_supported(4, 5, 34, 24) and not F().lstm_fm_supported(4, 5, 35, 24)
    elif case == "p64":  # the widest model
        cfg.update(p=64, h=4, C=2, tmax=4, N=20, B=12)
        assert F().lstm_fm_supported(64, 4, 2, 12) and not F().lstm_fm_supported(65, 4, 2, 12)
    elif case == "wd0":
        cfg.update(wd=0.0)
    elif case == "forecast_only":
        flags, okw = nat().LOSS_FORECAST | nat().STEP_B, dict(adj_on=False)
    elif case == "adj_only":
        flags, okw = nat().LOSS_ADJ | nat().STEP_B, dict(forecast_on=False)
    raw = Raw(**cfg)
    o = raw.oracle(0)
    sse, _, _ = raw.call(flags)
    want = oracle_epoch(o, raw.x_cpu(0), cfg["B"], **okw)
    compare_state_dict(case, split_packed(raw.fac[0], cfg["p"], cfg["h"]), o.state())
    assert_close(case + "/sse", sse[0].cpu().numpy(), want.numpy(), RTOL, ATOL * max(1.0, float(want.max())))
    assert bool(torch.isfinite(raw.fac).all())


def test_zero_input_column_has_zero_penalty_gradient():
    raw = Raw(N=8, B=8, seed=13, wd=0.0, **SHAPE)
    Wih = raw.fac[0, :7 * 52 * 7].view(7, 52, 7)
    Wih[2, :, 4] = 0.  # network 2 ignores channel 4 exactly
    Wih[5, :, 0] = 0.
    o = raw.oracle(0)
    _, _, G = raw.call(nat().LOSS_ADJ | nat().STEP_B, want_G=True)  # the penalty alone: its gradient there is 0
    assert bool(torch.isfinite(raw.fac).all()) and bool(torch.isfinite(raw.m).all())
    assert float(Wih[2, :, 4].abs().max()) == 0. and float(Wih[5, :, 0].abs().max()) == 0.
    assert float(G[0, 2, 4]) == 0. and float(G[0, 5, 0]) == 0. and int((G[0] == 0).sum()) == 2
    o.batch_update(raw.x_cpu(0), forecast_on=False)
    assert float(o.Wih.detach()[2, :, 4].abs().max()) == 0.  # as torch.norm's backward
    compare_state_dict("zero", split_packed(raw.fac[0], 7, 13), o.state())
    # the model's GC is 0 there too
    import redcliff_amd
    m = redcliff_amd.cLSTM_FM(7, 13, None, 3, {"FORECAST_COEFF": 1., "ADJ_L1_REG_COEFF": .1, "DAGNESS_REG_COEFF": 0.})
    with torch.no_grad():
        m.factors[0].networks[2].lstm.weight_ih_l0.copy_(Wih[2])
    assert int(m.GC()[0][2, 4]) == 0 and int(m.GC()[0][2].sum()) == 6
    # with the forecast term the column moves, and still matches
    raw.call(TRAIN(), tB=2)
    o.batch_update(raw.x_cpu(0))
    assert bool(torch.isfinite(raw.fac).all()) and float(Wih[2, :, 4].abs().max()) > 0.
    compare_state_dict("zero+forecast", split_packed(raw.fac[0], 7, 13), o.state())


def test_values_only_call_reads_only():
    raw = Raw(R=2, N=20, B=8, seed=17, **SHAPE)
    raw.call(TRAIN())  # non-trivial moments
    before = raw.snapshot()
    sse, pen, G = raw.call(VALUES(), want_G=True)
    assert same(raw.snapshot(), before)
    for r in range(2):
        o = raw.oracle(r)
        X = raw.x_cpu(r)
        for i, b0 in enumerate(range(0, 20, 8)):
            _, _, _, s = o.loss_terms(X[b0:b0 + 8])
            assert_close("sse", sse[r, i].cpu().numpy(), s.detach().numpy(), RTOL, ATOL)
            assert_close("pen", pen[r, i].cpu().numpy(), o.gc().sum(1).detach().numpy(), RTOL, ATOL)
        Wih = raw.fac[r, :7 * 52 * 7].view(7, 52, 7)
        assert_close("G", G[r].cpu().numpy(), torch.norm(Wih, dim=1).cpu().numpy(), 1e-6, 0)
    # the moments may be null without RC_STEP_B
    d = F().lstm_fm_dims(7, 13, Bmax=8, T=7, R=2)
    sse2, pen2 = torch.empty_like(sse), torch.empty_like(pen)
    assert F().lstm_fm_run(d, 3, 7, VALUES(), 8, 1, 0, 20, raw.X, 20 * 7 * 7, raw.fac, None, None, raw.n, raw.hyper,
                           sse2, pen2) == 0
    torch.cuda.synchronize()
    assert torch.equal(sse, sse2) and torch.equal(pen, pen2)


def test_guard_bands_stay_intact_and_change_nothing():
    kw = dict(R=2, N=20, B=8, seed=19, T=10, **SHAPE)  # T > tmax: the rows at and past tmax are never read
    plain = Raw(**kw)
    band = Raw(band=256, **kw)
    band.X[:, :, 7:, :] = float("nan")
    outs = []
    for raw in (plain, band):
        a = raw.call(TRAIN(), want_G=True)  # Raw.call asserts the bands after every launch
        b = raw.call(VALUES(), want_G=True)
        outs.append([t.clone() for t in a + b] + raw.snapshot())
    assert same(outs[0], outs[1])
    assert all(bool(torch.isfinite(t).all()) for t in outs[1])


# ------------------------------------------------------------------------------------------ fit_lstm_baselines
def test_fit_lstm_baselines_equals_the_models_own_fits(tmp_path, monkeypatch):
    import redcliff_amd
    from redcliff_amd import metrics as M
    monkeypatch.delenv("REDCLIFF_LSTM_FM_PATH", raising=False)
    meta, sc = load_lf("a")
    rng = np.random.RandomState(23)
    lrs = [meta["fit"]["lr"], 1e-3, 3e-3]  # the first is the fixture's whole fit, which stops early
    fetches = []
    inner = M.fetch

    def counted(tensors):
        fetches.append(len(tensors))
        return inner(tensors)
    monkeypatch.setattr(M, "fetch", counted)

    def setup(i, tag):
        m = build_model(dict(meta, seed=meta["seed"] + 40 * i), "cuda")
        opt = torch.optim.Adam(m.gen_model.parameters(), lr=lrs[i], eps=1e-4, weight_decay=1e-4)
        d = os.path.join(str(tmp_path), "%s%d" % (tag, i))
        return m, opt, d

    Xtr = [sc["X_train"] + (0.1 * i * rng.randn(*sc["X_train"].shape)).astype(np.float32) for i in range(3)]
    Xva = [sc["X_val"] + (0.1 * i * rng.randn(*sc["X_val"].shape)).astype(np.float32) for i in range(3)]
    kw = dict(max_iter=12, lookback=1, check_every=2)
    checks = lambda epochs: len(range(0, epochs, 2))
    own = []
    for i in range(3):
        m, opt, d = setup(i, "own")
        del fetches[:]
        loss = m.fit(d, batches(Xtr[i], meta["B"]), opt, meta["C"], meta["Tm"], 1, verbose=0,
                     X_val=batches(Xva[i], meta["B"]), **kw)
        # one fetch per check epoch plus one at the end, none on the epochs between
        assert len(fetches) == checks(len(m.fit_history["avg_smooth_loss"])) + 1, (i, fetches)
        own.append((m, opt, d, loss))
    packed = [setup(i, "pack") for i in range(3)]
    del fetches[:]
    losses = redcliff_amd.fit_lstm_baselines([m for m, _, _ in packed], [o for _, o, _ in packed],
                                             [d for _, _, d in packed], [batches(x, meta["B"]) for x in Xtr],
                                             [batches(x, meta["B"]) for x in Xva], meta["C"], meta["Tm"], **kw)
    lens = [len(m.fit_history["avg_smooth_loss"]) for m, _, _ in packed]
    print("epochs run:", lens, "best:", [m.fit_history["best_it"] for m, _, _ in packed])
    assert lens[0] == int(sc["fit/stop_epoch"]) + 1 and max(lens) == 12  # one stopped early, one ran to the end
    assert len(fetches) == checks(max(lens)) + 1, fetches
    for (m1, o1, d1, l1), (m2, o2, d2), l2 in zip(own, packed, losses):
        assert l1 == l2
        h1, h2 = m1.fit_history, m2.fit_history
        assert set(h1) == set(h2)
        for k in h1:
            assert pickle.dumps(h1[k]) == pickle.dumps(h2[k]), k
        s1, s2 = m1.state_dict(), m2.state_dict()
        assert all(torch.equal(s1[k], s2[k]) for k in s1)
        for (k1, v1), (k2, v2) in zip(o1.state_dict()["state"].items(), o2.state_dict()["state"].items()):
            assert float(v1["step"]) == float(v2["step"]) and torch.equal(v1["exp_avg"], v2["exp_avg"])
            assert torch.equal(v1["exp_avg_sq"], v2["exp_avg_sq"])
        with open(os.path.join(d1, "training_meta_data_and_hyper_parameters.pkl"), "rb") as f1, \
                open(os.path.join(d2, "training_meta_data_and_hyper_parameters.pkl"), "rb") as f2:
            assert f1.read() == f2.read()
        assert sorted(os.listdir(d1)) == sorted(os.listdir(d2))
        for name in os.listdir(d1):
            if name.endswith(".bin"):
                b1 = torch.load(os.path.join(d1, name), weights_only=False).state_dict()
                b2 = torch.load(os.path.join(d2, name), weights_only=False).state_dict()
                assert all(torch.equal(b1[k], b2[k]) for k in b1), name
