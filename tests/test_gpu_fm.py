"""GPU checks of the cMLP forecasting baseline: redcliff_fm_run (csrc/rc_fm.hip) and
redcliff_amd.cMLP_FM / fit_baselines against the reference fixture tests/golden/cmlp_fm.npz and the
plain-torch restatement of tests/test_fm_host.py (the oracle for shapes the fixture lacks).
Parity at the project's state bound, the invariances bitwise."""
import os
import pickle

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_fm_host import (RTOL, ATOL, TorchFM, batches, coeffs, compare_state_dict, load_fm, sub)

pytestmark = pytest.mark.gpu

ADAM = dict(lr=1e-3, eps=1e-4, weight_decay=1e-4)


def F():
    from redcliff_amd import cmlp_fm
    return cmlp_fm


def nat():
    from redcliff_amd import _native
    return _native


def fac_state(m):
    return dict((k, v.detach().cpu().numpy()) for k, v in m.state_dict().items() if k.startswith("factors."))


def build(meta, seed=None):
    import redcliff_amd
    torch.manual_seed(meta["seed"] if seed is None else seed)
    return redcliff_amd.cMLP_FM(meta["p"], meta["L"], [meta["h"]], None, meta["L"], 1, coeffs(meta)).to("cuda")


@pytest.fixture(params=["fused", "generic"])
def route(request, monkeypatch):
    monkeypatch.setenv("REDCLIFF_FM_PATH", request.param)
    return request.param


# ------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_batch_updates_and_validation_match_the_reference(name, route):
    meta, sc = load_fm(name)
    m = build(meta)
    assert m.fused_eligible(meta["L"], 1, Bmax=meta["B"], T=meta["L"] + 1) == (route == "fused")
    compare_state_dict("init", fac_state(m), sub(sc, "init"), 0, 0)
    opt = torch.optim.Adam(m.gen_model.parameters(), **ADAM)
    tr, va = batches(sc["X_train"], meta["B"]), batches(sc["X_val"], meta["B"])
    for e in range(1, meta["epochs"] + 1):
        for bn, (X, _) in enumerate(tr):
            m.batch_update(bn, X, opt, meta["L"], 1)
        compare_state_dict("%s/epoch%d" % (name, e), fac_state(m), sub(sc, "epoch%d" % e))
    st = opt.state[next(m.gen_model.parameters())]
    assert int(float(st["step"])) == meta["epochs"] * len(tr) and st["exp_avg"].shape == (meta["h"], meta["p"], meta["L"])
    raw = m.validate_training(va, meta["L"], 1, meta["p"])
    nrm = m.validate_training(va, meta["L"], 1, meta["p"], report_normalized_loss_components=True)
    print(name, route, "val", raw, nrm)
    assert_close(name + "/val_raw", raw, sc["val_raw"], RTOL, ATOL)
    assert_close(name + "/val_norm", nrm, sc["val_norm"], RTOL, ATOL)


def test_fit_matches_the_reference(route, tmp_path):
    meta, sc = load_fm("a")
    m = build(meta)
    opt = torch.optim.Adam(m.gen_model.parameters(), **ADAM)
    GC = [g.copy() for g in sc["fit/GC"]]
    final = m.fit(str(tmp_path), batches(sc["X_train"], meta["B"]), opt, meta["L"], 1, 1, 3, lookback=1, check_every=10,
                  verbose=0, GC=GC, X_val=batches(sc["X_val"], meta["B"]))
    with open(os.path.join(str(tmp_path), "training_meta_data_and_hyper_parameters.pkl"), "rb") as f:
        got = pickle.load(f)
    want = sub(sc, "fit/pkl")
    rows = int(want.pop("gc_factor_l1_loss_histories_rows"))
    assert set(got) == set(want)
    assert len(got["gc_factor_l1_loss_histories"]) == rows and got["gc_factor_l1_loss_histories"][1] == []
    for k in want:
        v = got[k]
        if k in ("f1score_histories", "roc_auc_histories"):
            assert list(v.keys()) == [0.0]
            v = v[0.0]
        elif k == "gc_factor_l1_loss_histories":
            v = v[0]
        print(k, np.asarray(v, dtype=np.float64), want[k])
        assert_close("fit/" + k, np.asarray(v, dtype=np.float64), want[k], RTOL, ATOL)
    # F1 counts thresholded entries: identical, not merely close
    assert np.array_equal(np.asarray(got["f1score_histories"][0.0], dtype=np.float32),
                          want["f1score_histories"].astype(np.float32))
    assert os.path.exists(os.path.join(str(tmp_path), "final_best_model.bin"))
    compare_state_dict("fit/final", fac_state(m), sub(sc, "fit/final"))
    assert_close("fit/final_loss", final, sc["fit/final_loss"], RTOL, ATOL)
    # thresholded graph of the final model == that of the reference's final weights
    ref = TorchFM(sub(sc, "fit/final"), 1., 1., None)
    assert torch.equal(m.GC()[0].cpu(), (ref.gc().detach() > 0).int())
    assert len(m.fit_history["avg_combo_loss"]) == 3 and m.fit_history["best_it"] == 2


# ------------------------------------------------------------------------------------------ raw calls
def packed_to_state(flat, p, h, L):
    flat = flat.detach().cpu().numpy()
    Q = p * L
    out = {}
    b0, W1, b1 = p * h * Q, p * h * Q + p * h, p * h * Q + 2 * p * h
    for j in range(p):
        pre = "factors.0.networks.%d.layers." % j
        out[pre + "0.weight"] = flat[j * h * Q:(j + 1) * h * Q].reshape(h, p, L).copy()
        out[pre + "0.bias"] = flat[b0 + j * h:b0 + (j + 1) * h].copy()
        out[pre + "1.weight"] = flat[W1 + j * h:W1 + (j + 1) * h].reshape(1, h, 1).copy()
        out[pre + "1.bias"] = flat[b1 + j:b1 + j + 1].copy()
    return out


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
    """Packed buffers of R replicas for direct redcliff_fm_run calls."""

    def __init__(self, p, L, h, R=1, N=40, B=16, seed=0, T=None, lrs=None, wd=1e-4, forecast=1.0, adj=0.1,
                 shared_x=False, band=0):
        self.p, self.L, self.h, self.R, self.N, self.B = p, L, h, R, N, B
        self.T = L + 1 if T is None else T
        self.n = p * (h * p * L + 2 * h + 1)
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
        p, L = self.p, self.L
        sse, w_sse = banded((max(nrep, 1), nsteps, p), self.band)  # never a null pointer, even for an empty list
        pen, w_pen = banded((max(nrep, 1), nsteps, p), self.band)
        G, w_G = banded((self.R, p, p, L), self.band)
        G0, w_G0 = banded((self.R, p, p), self.band)
        d = F().fm_dims(p, L, self.h, Bmax=max(B, 1), T=self.T, R=self.R)
        rc = F().fm_run(d, flags, B, tB, row0, N, self.X, 0 if self.shared_x else self.N * self.T * p, self.fac, self.m,
                        self.v, self.n, self.hyper, sse, pen, G if want_G else None, G0 if want_G else None, replicas)
        assert rc == expect, (rc, nat().lib().redcliff_last_error())
        torch.cuda.synchronize()
        if self.band:
            for w in self.wholes + [w_sse, w_pen, w_G, w_G0]:
                assert bands_intact(w, self.band)
        return sse, pen, G, G0

    def snapshot(self):
        return [t.clone() for t in (self.fac, self.m, self.v)]

    def restore(self, snap):
        for t, s in zip((self.fac, self.m, self.v), snap):
            t.copy_(s)

    def oracle(self, r, lr=None):
        adam = dict(lr=self.lrs[r] if lr is None else lr, eps=1e-4, weight_decay=self.wd)
        return TorchFM(packed_to_state(self.fac[r], self.p, self.h, self.L), self.forecast, self.adj, adam)

    def x_cpu(self, r):
        return self.X[0 if self.shared_x else r].cpu()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def TRAIN():
    return F().FM_FLAGS_TRAIN


def VALUES():
    return F().FM_FLAGS_VALUES


def oracle_epoch(o, X, B, **kw):
    return torch.stack([o.batch_update(X[i:i + B], **kw) for i in range(0, X.shape[0], B)])


def test_epoch_call_equals_split_calls_and_single_batches():
    raw = Raw(7, 3, 33, N=40, B=16, seed=3)
    s0 = raw.snapshot()
    sse, _, G, G0 = raw.call(TRAIN(), want_G=True)
    whole = raw.snapshot()
    # against the restatement, with the sums of squared residuals per step and the final norms
    o = Raw(7, 3, 33, N=40, B=16, seed=3).oracle(0)
    want_sse = oracle_epoch(o, raw.x_cpu(0), 16)
    compare_state_dict("epoch", packed_to_state(raw.fac[0], 7, 33, 3), o.state())
    assert_close("sse", sse[0].cpu().numpy(), want_sse.numpy(), RTOL, ATOL)
    assert_close("G", G[0].cpu().numpy(), o.gc_lagged().detach().numpy(), RTOL, ATOL)
    assert_close("G0", G0[0].cpu().numpy(), o.gc().detach().numpy(), RTOL, ATOL)
    # two runs agree
    raw.restore(s0)
    sse2, _, G2, _ = raw.call(TRAIN(), want_G=True)
    assert same(raw.snapshot(), whole) and torch.equal(sse, sse2) and torch.equal(G, G2)
    # [0, 32) + [32, 40) with tB advanced
    raw.restore(s0)
    a, _, _, _ = raw.call(TRAIN(), row0=0, N=32, tB=1)
    b, _, _, _ = raw.call(TRAIN(), row0=32, N=8, tB=3)
    assert same(raw.snapshot(), whole) and torch.equal(torch.cat([a, b], 1), sse)
    # nsteps one-batch calls
    raw.restore(s0)
    parts = [raw.call(TRAIN(), row0=r0, N=n, B=n, tB=t)[0] for t, (r0, n) in enumerate([(0, 16), (16, 16), (32, 8)], 1)]
    assert same(raw.snapshot(), whole) and torch.equal(torch.cat(parts, 1), sse)


def test_pack_equals_single_replicas_and_the_active_list():
    kw = dict(N=40, B=16, seed=5, lrs=[1e-3, 3e-3, 1e-2])
    pack = Raw(7, 3, 33, R=3, **kw)
    s0 = pack.snapshot()
    sse, _, G, _ = pack.call(TRAIN(), want_G=True)
    for r in range(3):
        one = Raw(7, 3, 33, R=1, N=40, B=16, seed=99, lrs=[kw["lrs"][r]])
        one.fac.copy_(s0[0][r:r + 1])
        one.X.copy_(pack.X[r:r + 1])
        s1, _, G1, _ = one.call(TRAIN(), want_G=True)
        assert torch.equal(one.fac[0], pack.fac[r]) and torch.equal(one.m[0], pack.m[r])
        assert torch.equal(one.v[0], pack.v[r]) and torch.equal(s1[0], sse[r]) and torch.equal(G1[0], G[r])
    assert not torch.equal(pack.fac[0] - s0[0][0], pack.fac[2] - s0[0][2])
    # replicas = [0, 2]: replica 1 untouched, rows 0 / 1 of the outputs are replicas 0 / 2
    done = pack.snapshot()
    pack.restore(s0)
    s02, _, _, _ = pack.call(TRAIN(), replicas=[0, 2])
    now = pack.snapshot()
    for t0, t1, t2 in zip(s0, now, done):
        assert torch.equal(t1[1], t0[1]) and torch.equal(t1[0], t2[0]) and torch.equal(t1[2], t2[2])
    assert s02.shape[0] == 2 and torch.equal(s02[0], sse[0]) and torch.equal(s02[1], sse[2])
    # an empty list launches nothing
    before = pack.snapshot()
    pack.call(TRAIN(), replicas=[])
    assert same(pack.snapshot(), before)
    # one shared window set (x_pstride == 0)
    sh = Raw(7, 3, 33, R=2, N=40, B=16, seed=6, shared_x=True)
    f0 = sh.fac.clone()
    sh.call(TRAIN())
    for r in range(2):
        one = Raw(7, 3, 33, R=1, N=40, B=16, seed=6, shared_x=True)
        one.fac.copy_(f0[r:r + 1])
        one.X.copy_(sh.X)
        one.call(TRAIN())
        assert torch.equal(one.fac[0], sh.fac[r])


@pytest.mark.parametrize("case", ["B1", "Bmax512_h128", "wd0", "forecast_only", "adj_only", "p64"])
def test_edges_against_the_restatement(case):
    cfg = dict(p=7, L=3, h=33, N=40, B=16, seed=11)
    flags, okw = TRAIN(), {}
    if case == "B1":
        cfg.update(N=3, B=1)
    elif case == "Bmax512_h128":  # the largest h, the largest batch: 8 passes of 64 windows
        cfg.update(p=10, L=2, h=128, N=512, B=512)
        assert F().fm_supported(10, 2, 128, 512) and not F().fm_supported(10, 2, 129, 512)
    elif case == "wd0":
        cfg.update(wd=0.0)
    elif case == "forecast_only":
        flags, okw = nat().LOSS_FORECAST | nat().STEP_B, dict(adj_on=False)
    elif case == "adj_only":
        flags, okw = nat().LOSS_ADJ | nat().STEP_B, dict(forecast_on=False)
    elif case == "p64":  # the widest model: p*L = 128 columns, the LDS limit allows h = 50
        cfg.update(p=64, L=2, h=50, N=70, B=64)
        assert F().fm_supported(64, 2, 50, 64)
    raw = Raw(**cfg)
    o = raw.oracle(0)
    sse, _, _, _ = raw.call(flags)
    want = oracle_epoch(o, raw.x_cpu(0), cfg["B"], **okw)
    compare_state_dict(case, packed_to_state(raw.fac[0], cfg["p"], cfg["h"], cfg["L"]), o.state())
    assert_close(case + "/sse", sse[0].cpu().numpy(), want.numpy(), RTOL, ATOL * max(1.0, float(want.max())))
    assert bool(torch.isfinite(raw.fac).all())


def test_zero_channel_column_has_zero_penalty_gradient():
    raw = Raw(7, 3, 33, N=16, B=16, seed=13, wd=0.0)
    W0 = raw.fac[0, :7 * 33 * 21].view(7, 33, 7, 3)
    W0[2, :, 4, :] = 0.  # network 2 ignores channel 4 exactly
    W0[5, :, 0, :] = 0.
    o = raw.oracle(0)
    raw.call(nat().LOSS_ADJ | nat().STEP_B)  # the penalty alone: its gradient there is 0, the weights stay 0
    assert bool(torch.isfinite(raw.fac).all()) and bool(torch.isfinite(raw.m).all())
    assert float(W0[2, :, 4, :].abs().max()) == 0. and float(W0[5, :, 0, :].abs().max()) == 0.
    o.batch_update(raw.x_cpu(0), forecast_on=False)
    assert float(o.W0.detach()[2, :, 4, :].abs().max()) == 0.  # as torch.norm's backward
    compare_state_dict("zero", packed_to_state(raw.fac[0], 7, 33, 3), o.state())
    # with the forecast term the column moves, and still matches
    raw.call(TRAIN(), tB=2)
    o.batch_update(raw.x_cpu(0))
    assert bool(torch.isfinite(raw.fac).all())
    compare_state_dict("zero+forecast", packed_to_state(raw.fac[0], 7, 33, 3), o.state())


def test_values_only_call_reads_only():
    raw = Raw(7, 3, 33, R=2, N=40, B=16, seed=17)
    raw.call(TRAIN())  # non-trivial moments
    before = raw.snapshot()
    sse, pen, G, G0 = raw.call(VALUES(), want_G=True)
    assert same(raw.snapshot(), before)
    for r in range(2):
        o = raw.oracle(r)
        X = raw.x_cpu(r)
        for i, b0 in enumerate(range(0, 40, 16)):
            _, _, _, s = o.loss_terms(X[b0:b0 + 16])
            assert_close("sse", sse[r, i].cpu().numpy(), s.detach().numpy(), RTOL, ATOL)
            assert_close("pen", pen[r, i].cpu().numpy(), o.gc().sum(1).detach().numpy(), RTOL, ATOL)
        assert_close("G0", G0[r].cpu().numpy(), o.gc().detach().numpy(), RTOL, ATOL)
    # the existing norms kernel sees the same graph
    from redcliff_amd import kernels
    d = kernels.factor_dims(1, 7, 3, 33, R=2)
    Gn = torch.empty(2, 7, 7, 3, device="cuda")
    G0n = torch.empty(2, 7, 7, device="cuda")
    import ctypes
    nat().check(nat().lib().redcliff_gc_norms(ctypes.byref(d), kernels.ptr(raw.fac), raw.n, kernels.ptr(Gn),
                                              kernels.ptr(G0n), kernels.current_stream()), "gc_norms")
    assert_close("G vs gc_norms", G.cpu().numpy(), Gn.cpu().numpy(), 1e-6, 0)
    assert_close("G0 vs gc_norms", G0.cpu().numpy(), G0n.cpu().numpy(), 1e-6, 0)


def test_guard_bands_stay_intact_and_change_nothing():
    kw = dict(R=2, N=40, B=16, seed=19, T=6)  # T > L + 1: the rows past the target are never read
    plain = Raw(7, 3, 33, **kw)
    band = Raw(7, 3, 33, band=256, **kw)
    band.X[:, :, 4:, :] = float("nan")
    outs = []
    for raw in (plain, band):
        a = raw.call(TRAIN(), want_G=True)  # Raw.call asserts the bands after every launch
        b = raw.call(VALUES(), want_G=True)
        written = (a[0], a[2], a[3]) + b  # a training call without RC_VALUES writes no pen
        outs.append([t.clone() for t in written] + raw.snapshot())
    assert same(outs[0], outs[1])
    assert all(bool(torch.isfinite(t).all()) for t in outs[1])


# ------------------------------------------------------------------------------------------ fit_baselines
def test_fit_baselines_equals_the_models_own_fits(tmp_path):
    import redcliff_amd
    meta, sc = load_fm("a")
    rng = np.random.RandomState(23)
    lrs = [1e-3, 0.5, 3e-3]  # the second fit overshoots and stops early

    def setup(i, tag):
        m = build(meta, seed=40 + i)
        opt = torch.optim.Adam(m.gen_model.parameters(), lr=lrs[i], eps=1e-4, weight_decay=1e-4)
        d = os.path.join(str(tmp_path), "%s%d" % (tag, i))
        return m, opt, d

    Xtr = [sc["X_train"] + (0.1 * i * rng.randn(*sc["X_train"].shape)).astype(np.float32) for i in range(3)]
    Xva = [sc["X_val"] + (0.1 * i * rng.randn(*sc["X_val"].shape)).astype(np.float32) for i in range(3)]
    GCs = [[(rng.rand(4, 4, 2) < 0.5).astype(np.float64) + np.eye(4)[:, :, None] for _ in range(2)] for _ in range(3)]
    kw = dict(max_iter=6, lookback=1, check_every=1)
    own = []
    for i in range(3):
        m, opt, d = setup(i, "own")
        loss = m.fit(d, batches(Xtr[i], meta["B"]), opt, meta["L"], 1, 1, verbose=0, GC=GCs[i],
                     X_val=batches(Xva[i], meta["B"]), **kw)
        own.append((m, opt, d, loss))
    packed = [setup(i, "pack") for i in range(3)]
    losses = redcliff_amd.fit_baselines([m for m, _, _ in packed], [o for _, o, _ in packed], [d for _, _, d in packed],
                                        [batches(x, meta["B"]) for x in Xtr], [batches(x, meta["B"]) for x in Xva], GCs,
                                        meta["L"], 1, **kw)
    lens = [len(m.fit_history["avg_combo_loss"]) for m, _, _ in packed]
    print("epochs run:", lens, "best:", [m.fit_history["best_it"] for m, _, _ in packed])
    assert min(lens) < 6 and max(lens) == 6  # one stopped early, one ran to the end
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
        b1 = torch.load(os.path.join(d1, "final_best_model.bin"), weights_only=False).state_dict()
        b2 = torch.load(os.path.join(d2, "final_best_model.bin"), weights_only=False).state_dict()
        assert all(torch.equal(b1[k], b2[k]) for k in b1)
