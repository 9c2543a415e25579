"""GPU checks of the NAVAR (LSTM) baseline: redcliff_navar_lstm_run (csrc/rc_navar_lstm.hip) and
redcliff_amd.NAVARLSTM / fit_navar_lstm_baselines against the reference fixture
tests/golden/navar_lstm.npz and the generic route run in float64 for shapes the fixture lacks.  Parity
at the project's state bound, the invariances bitwise."""
import os

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_navar_lstm_host import (ATOL, RTOL, build, check_scenario_epochs, check_whole_fit, compare_state_dict, load_nl,
                                  state_of)

pytestmark = pytest.mark.gpu

SHAPES = {"one": dict(N=3, H=5, Tp=3, n=20, B=6),      # ragged last batch of 2
          "two": dict(N=4, H=33, Tp=5, n=40, B=16)}    # three unit slices, ragged last batch of 8


def nl():
    from redcliff_amd import navar_lstm
    return navar_lstm


@pytest.fixture(params=["fused", "generic"])
def route(request, monkeypatch):
    monkeypatch.setenv("REDCLIFF_NAVAR_LSTM_PATH", request.param)
    return request.param


def windows(seed, n, T, N, R=None):
    rng = np.random.RandomState(seed)
    return rng.randn(*((n, T, N) if R is None else (R, n, T, N))).astype(np.float32)


def new_model(N, H, seed):
    from redcliff_amd import NAVARLSTM
    torch.manual_seed(seed)
    return NAVARLSTM(N, H, 1).to("cuda")


def make_pack(sh, R, seed=0, lrs=None, lams=None, wd=0.0):
    """R seeded models of shape `sh` in one NavarLstmPack, each with its own bound Adam."""
    models = [new_model(sh["N"], sh["H"], seed + r) for r in range(R)]
    pack = nl().NavarLstmPack(models)
    opts = []
    for r, m in enumerate(models):
        opts.append(torch.optim.Adam(m.parameters(), lr=(lrs or [1e-3] * R)[r], weight_decay=wd))
        pack.bind_optimizer(r, opts[-1])
        pack.lambda1[r] = (lams or [0.05] * R)[r]
    return pack, models, opts


def perms_for(R, n, seed):
    return torch.from_numpy(np.stack([np.random.RandomState(seed + r).permutation(n) for r in range(R)]).astype(np.int32)).cuda()


def snap(pack):
    return [t.clone() for t in (pack.par, pack.m, pack.v)]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "w"])
def test_scenarios_match_the_reference(name, route, tmp_path):
    meta, _ = load_nl(name)
    m = build(meta, "cuda")
    opt = torch.optim.Adam(m.parameters(), **meta["adam"])
    assert m.fused_eligible(torch.nn.MSELoss(), opt, T=meta["Tp"] + 1, Bmax=min(meta["B"], meta["n"])) == (route == "fused")
    check_scenario_epochs(name, tmp_path, "cuda")


@pytest.mark.parametrize("name", ["a", "b"])
def test_whole_fits_match_the_reference(name, route, tmp_path):
    m = check_whole_fit(name, tmp_path, "cuda")
    assert ("_nv_slot" in m.__dict__) == (route == "fused")
    saved = torch.load(os.path.join(str(tmp_path), "final_best_model.bin"), weights_only=False)
    assert "_nv_slot" not in saved.__dict__ and np.array_equal(saved.GC(), m.GC())
    for k, t in saved.state_dict().items():
        assert t.untyped_storage().nbytes() == t.numel() * 4, k  # compact clones, not views of the pack


def fit_route(monkeypatch, which, N, H, X, B, epochs, lam, adam, tmp, seed=3, mutate=None, pre=None):
    """One seeded model fitted on route `which`: 'fused', or 'oracle' = the generic route in float64 (the
    same seeded float32 initial values and data, widened).  Returns (model, optimizer)."""
    monkeypatch.setenv("REDCLIFF_NAVAR_LSTM_PATH", "generic" if which == "oracle" else which)
    m = new_model(N, H, seed)
    if which == "oracle":
        m, X = m.double(), X.astype(np.float64)
    if mutate is not None:
        with torch.no_grad():
            mutate(m)
    opt = torch.optim.Adam(m.parameters(), **adam)
    if pre is not None:
        pre(m, opt)
    m.fit(str(tmp), X, None, torch.nn.MSELoss(), opt, epochs=epochs, batch_size=B, lambda1=lam,
          rng=np.random.RandomState(seed + 50))
    assert ("_nv_slot" in m.__dict__) == (which == "fused")
    return m, opt


def compare_routes(monkeypatch, tmp, N, H, Tp, n, B, epochs=2, lam=0.05, adam=None, mutate=None, X=None):
    """The fused route against the generic route in float64 (the oracle: a float32 torch backward can
    leave rounding residue on exactly-zero gradients, which Adam amplifies)."""
    adam = dict(lr=1e-3) if adam is None else adam
    X = windows(N * 1000 + H, n, Tp + 1, N) if X is None else X
    f, fo = fit_route(monkeypatch, "fused", N, H, X, B, epochs, lam, adam, tmp, mutate=mutate)
    g, go = fit_route(monkeypatch, "oracle", N, H, X, B, epochs, lam, adam, tmp, mutate=mutate)
    assert all(np.isfinite(v).all() for v in state_of(f).values())
    compare_state_dict("fused vs generic", state_of(f), state_of(g))
    assert_close("mse", f.step_losses[0], g.step_losses[0], RTOL, ATOL)
    assert_close("l1", f.step_losses[1], g.step_losses[1], RTOL, ATOL)
    assert_close("causal", f.GC(), g.GC(), RTOL, ATOL)
    for pf, pg in zip(f.parameters(), g.parameters()):
        assert float(fo.state[pf]["step"]) == float(go.state[pg]["step"])
    return f, g


def test_published_shape_fused_against_generic(monkeypatch, tmp_path):
    """N 10, H 256, T' 20, B 128, n 300 (128, 128, 44): one epoch of three steps, Adam(lr 1e-4)."""
    compare_routes(monkeypatch, tmp_path, 10, 256, 20, 300, 128, epochs=1, lam=0.0, adam=dict(lr=1e-4))


# ------------------------------------------------------------------------------------------ bitwise invariants
@pytest.mark.parametrize("shape", ["one", "two"])
def test_two_runs_agree_and_one_call_equals_a_call_per_batch(shape):
    sh = SHAPES[shape]
    n, B = sh["n"], sh["B"]
    X = torch.from_numpy(windows(1, n, sh["Tp"] + 1, sh["N"])).cuda()
    perm = perms_for(1, n, 7)[0]
    outs = []
    for split in (False, False, True):
        pack, _, _ = make_pack(sh, 1, wd=1e-4)
        if not split:
            mse, l1 = pack.train(X, 0, perm, 0, n, B)
        else:
            parts = [pack.train(X, 0, perm[s:], 0, min(B, n - s), B) for s in range(0, n, B)]
            mse, l1 = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
        assert pack.opt[0]["t"] == -(-n // B)
        outs.append(snap(pack) + [mse, l1])
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][1], torch.zeros_like(outs[0][1]))
    assert same_bits(outs[0], outs[1]), "two runs differ"
    assert same_bits(outs[0], outs[2]), "an epoch in one call differs from one call per batch"


@pytest.mark.parametrize("shape", ["one", "two"])
def test_replicas_are_independent(shape):
    sh = SHAPES[shape]
    n, B, R = sh["n"], sh["B"], 3
    lrs, lams = [1e-3, 2e-3, 5e-4], [0.05, 0.0, 0.2]
    X = torch.from_numpy(windows(2, n, sh["Tp"] + 1, sh["N"], R)).cuda()
    perm = perms_for(R, n, 11)
    xps = X[0].numel()
    pack, _, _ = make_pack(sh, R, lrs=lrs, lams=lams)
    before = snap(pack)
    mse, l1 = pack.train(X, xps, perm, n, n, B)
    for r in range(R):  # R = 3 in one call equals three R = 1 calls
        one, _, _ = make_pack(sh, 1, seed=r, lrs=[lrs[r]], lams=[lams[r]])
        m1, l11 = one.train(X[r].contiguous(), 0, perm[r].contiguous(), 0, n, B)
        assert same_bits([t[r] for t in snap(pack)] + [mse[r], l1[r]], [t[0] for t in snap(one)] + [m1[0], l11[0]]), r
    # a replica list [0, 2] leaves replica 1 untouched and steps 0 and 2 as the full call did
    part, _, _ = make_pack(sh, R, lrs=lrs, lams=lams)
    pm, pl = part.train(X, xps, perm, n, n, B, active=[0, 2])
    assert pm.shape[0] == 2
    for t, b, full in zip(snap(part), before, snap(pack)):
        assert torch.equal(t[1], b[1]) and torch.equal(t[0], full[0]) and torch.equal(t[2], full[2])
    assert torch.equal(pm, mse[[0, 2]]) and torch.equal(pl, l1[[0, 2]])
    assert part.opt[1]["t"] == 0 and part.opt[0]["t"] == -(-n // B)
    # an empty list launches nothing
    held = snap(part)
    em, _ = part.train(X, xps, perm, n, n, B, active=[])
    assert em.shape[0] == 0 and same_bits(held, snap(part))
    # shared and per-replica window sets agree
    Xs = X[0].contiguous()
    a, _, _ = make_pack(sh, R, lrs=lrs, lams=lams)
    b, _, _ = make_pack(sh, R, lrs=lrs, lams=lams)
    ra = a.train(Xs, 0, perm, n, n, B)
    rb = b.train(torch.stack([Xs] * R).contiguous(), Xs.numel(), perm, n, n, B)
    assert same_bits(snap(a) + list(ra), snap(b) + list(rb))


@pytest.mark.parametrize("shape", ["one", "two"])
def test_forward_splits_and_only_reads(shape):
    sh = SHAPES[shape]
    n, R = 150, 2
    X = torch.from_numpy(windows(3, n, sh["Tp"] + 1, sh["N"], R)).cuda()
    pack, models, _ = make_pack(sh, R)
    pack.m.normal_()
    pack.v.uniform_()
    before = snap(pack)
    pred, contrib = pack.forward(X, X[0].numel(), 0, n, B=64)  # chunks of 64, 64, 22
    assert same_bits(before, snap(pack))
    m = 70
    p0, c0 = pack.forward(X, X[0].numel(), 0, m, B=64)
    p1, c1 = pack.forward(X, X[0].numel(), m, n - m, B=64)
    assert torch.equal(pred, torch.cat([p0, p1], 1)) and torch.equal(contrib, torch.cat([c0, c1], 1))
    for r in range(R):  # and it is the module's forward (torch's own LSTM kernels: at the loss bound)
        with torch.no_grad():
            wp, wc = models[r](X[r].transpose(1, 2)[:, :, :-1])
        assert_close("pred", pred[r].cpu().numpy(), wp.cpu().numpy(), RTOL, ATOL)
        assert_close("contrib", contrib[r].cpu().numpy(), wc[:, :, 0].cpu().numpy(), RTOL, ATOL)


def test_fit_navar_lstm_baselines_equals_three_fits(tmp_path):
    from redcliff_amd import fit_navar_lstm_baselines
    sh = SHAPES["two"]
    R, n = 3, sh["n"]
    Xs = [windows(20 + r, n, sh["Tp"] + 1, sh["N"]) for r in range(R)]
    Xv = [windows(30 + r, 12, sh["Tp"] + 1, sh["N"]) for r in range(R)]

    def fresh():
        ms = [new_model(sh["N"], sh["H"], 40 + r) for r in range(R)]
        return ms, [torch.optim.Adam(m.parameters(), lr=1e-3 * (r + 1)) for r, m in enumerate(ms)]
    pm, po = fresh()
    dirs = [str(tmp_path / ("p%d" % r)) for r in range(R)] + [str(tmp_path / ("s%d" % r)) for r in range(R)]
    for d in dirs:
        os.makedirs(d)
    kw = dict(val_proportion=0.5, epochs=3, batch_size=sh["B"], check_every=2, lambda1=0.05)
    lv_p = fit_navar_lstm_baselines(pm, dirs[:R], Xs, torch.nn.MSELoss(), po, X_vals=Xv,
                                    rngs=[np.random.RandomState(60 + r) for r in range(R)], **kw)
    assert pm[0].__dict__["_nv_slot"][0] is pm[2].__dict__["_nv_slot"][0] and pm[0].__dict__["_nv_slot"][0].R == R
    sm, so = fresh()
    for r in range(R):
        lv = sm[r].fit(dirs[R + r], Xs[r], None, torch.nn.MSELoss(), so[r], X_val=Xv[r], rng=np.random.RandomState(60 + r), **kw)
        assert float(lv) == float(lv_p[r]) and float(lv) > 0
        a, b = state_of(pm[r]), state_of(sm[r])
        assert all(np.array_equal(a[k], b[k]) for k in a)
        for x, y in zip(pm[r].parameters(), sm[r].parameters()):
            sx, sy = po[r].state[x], so[r].state[y]
            assert torch.equal(sx["exp_avg"], sy["exp_avg"]) and torch.equal(sx["exp_avg_sq"], sy["exp_avg_sq"])
            assert float(sx["step"]) == float(sy["step"]) == 9.0
        assert np.array_equal(pm[r].GC(), sm[r].GC())
        assert np.array_equal(pm[r].step_losses[0], sm[r].step_losses[0])
        la = torch.load(os.path.join(dirs[r], "final_best_model.bin"), weights_only=False)
        lb = torch.load(os.path.join(dirs[R + r], "final_best_model.bin"), weights_only=False)
        assert all(torch.equal(la.state_dict()[k], lb.state_dict()[k]) for k in la.state_dict())
        assert np.array_equal(la.GC(), lb.GC())


# ------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("case", [
    dict(tag="B1", N=3, H=5, Tp=3, n=4, B=1),
    dict(tag="ragged1", N=3, H=5, Tp=3, n=7, B=6),
    dict(tag="ragged1_pass", N=2, H=7, Tp=2, n=130, B=65),   # a second pass of one window; then 65 = 64 + 1
    dict(tag="T1", N=3, H=5, Tp=1, n=20, B=6),
    dict(tag="T2", N=3, H=5, Tp=2, n=20, B=6),
    dict(tag="H1", N=3, H=1, Tp=3, n=20, B=6),
    dict(tag="H16", N=2, H=16, Tp=3, n=20, B=6),
    dict(tag="H17", N=2, H=17, Tp=3, n=20, B=6),
    dict(tag="N1", N=1, H=5, Tp=3, n=20, B=6),
    dict(tag="N32", N=32, H=6, Tp=2, n=20, B=8),
    dict(tag="Tmax", N=2, H=5, Tp=64, n=12, B=8),
    dict(tag="Bmax", N=2, H=5, Tp=2, n=1024, B=512, epochs=1),
    dict(tag="Hmax", N=2, H=448, Tp=2, n=12, B=8),
    dict(tag="lam0", N=3, H=18, Tp=4, n=20, B=8, lam=0.0),
    dict(tag="wd0", N=3, H=34, Tp=4, n=20, B=8, adam=dict(lr=1e-3, weight_decay=0.0)),
    dict(tag="wd", N=3, H=34, Tp=4, n=20, B=8, adam=dict(lr=1e-3, weight_decay=1e-2)),
], ids=lambda c: c["tag"])
def test_edge_shapes_against_generic(case, monkeypatch, tmp_path):
    c = dict(case)
    c.pop("tag")
    compare_routes(monkeypatch, tmp_path, c.pop("N"), c.pop("H"), c.pop("Tp"), c.pop("n"), c.pop("B"), **c)


def test_limits_hold_on_both_sides():
    m = nl()
    assert m.navar_lstm_supported(2, 448, 64, 512, 256) > 0
    assert m.navar_lstm_supported(2, 449, 2, 8) == 0 and m.navar_lstm_supported(2, 5, 65, 8) == 0
    assert m.navar_lstm_supported(2, 5, 2, 513) == 0 and m.navar_lstm_supported(33, 5, 2, 8) == 0


def test_zero_contribution_has_zero_l1_gradient(monkeypatch, tmp_path):
    """A zero Wfc row with a zero bfc: that contribution is exactly 0 at every step on both routes, its
    sign term 0; only the MSE term moves it."""
    N, H, Tp = 3, 5, 3

    def mutate(m):
        m.fc_list[0].weight[1].zero_()
        m.fc_list[0].bias[1] = 0.0
    f, g = compare_routes(monkeypatch, tmp_path, N, H, Tp, 6, 300, epochs=1, lam=0.5, mutate=mutate)
    assert np.isfinite(f.GC()).all() and np.isfinite(f.step_losses[1]).all() and f.step_losses[1][0] > 0


def test_resume_from_a_torch_stepped_optimizer(monkeypatch, tmp_path):
    """One torch-stepped (generic) epoch, then a fused epoch with the same optimizer: its moments and step
    count are copied into the pack.  Adam eps 1e-4 as tests/test_gpu_navar.py, so that the float32 torch
    epoch's rounding does not move weights through Adam's normalisation."""
    sh = SHAPES["two"]
    X = windows(5, sh["n"], sh["Tp"] + 1, sh["N"])
    adam = dict(lr=1e-3, eps=1e-4)

    def torch_epoch(m, opt):  # before the fit under test
        keep = os.environ["REDCLIFF_NAVAR_LSTM_PATH"]
        monkeypatch.setenv("REDCLIFF_NAVAR_LSTM_PATH", "generic")
        Xm = X.astype(np.float64) if m.biases.dtype == torch.float64 else X
        m.fit(str(tmp_path), Xm, None, torch.nn.MSELoss(), opt, epochs=1, batch_size=sh["B"], lambda1=0.05,
              rng=np.random.RandomState(99))
        assert "_nv_slot" not in m.__dict__
        monkeypatch.setenv("REDCLIFF_NAVAR_LSTM_PATH", keep)
    f, fo = fit_route(monkeypatch, "fused", sh["N"], sh["H"], X, sh["B"], 1, 0.05, adam, tmp_path, pre=torch_epoch)
    g, go = fit_route(monkeypatch, "oracle", sh["N"], sh["H"], X, sh["B"], 1, 0.05, adam, tmp_path, pre=torch_epoch)
    compare_state_dict("resume", state_of(f), state_of(g))
    for pf, pg in zip(f.parameters(), g.parameters()):
        assert float(fo.state[pf]["step"]) == float(go.state[pg]["step"]) == 6.0
        want = go.state[pg]["exp_avg"].cpu().numpy()
        assert_close("exp_avg", fo.state[pf]["exp_avg"].cpu().numpy(), want, 1e-3, 1e-6 * float(np.abs(want).max()))


def guarded(t, band=257):
    """A copy of `t` with NaN bands on both sides: (whole buffer, view of the payload)."""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + 2 * band,), float("nan"), device="cuda", dtype=torch.float32)
    view = buf[band:band + flat.numel()]
    (view.view(torch.int32) if t.dtype == torch.int32 else view).copy_(flat)
    return buf, view


def bands_intact(buf, band=257):
    return bool(torch.isnan(buf[:band]).all() and torch.isnan(buf[-band:]).all())


@pytest.mark.parametrize("shape", ["one", "two"])
def test_nan_guard_bands(shape):
    sh = SHAPES[shape]
    N, Tp, n, B, R = sh["N"], sh["Tp"], sh["n"], sh["B"], 2
    mod = nl()
    pack, _, _ = make_pack(sh, R)
    ref, _, _ = make_pack(sh, R)
    Xh = windows(8, n + 6, Tp + 1, N, R)
    Xh[:, n:] = np.nan  # rows the permutation never names
    X = torch.from_numpy(Xh).cuda()
    perm = perms_for(R, n, 13)
    want = ref.train(X, X[0].numel(), perm, n, n, B)
    nsteps = -(-n // B)
    bufs = {}
    for k, t in (("X", X), ("perm", perm), ("par", pack.par), ("m", pack.m), ("v", pack.v)):
        bufs[k] = guarded(t)
    wsn = mod.navar_lstm_ws_floats(N, sh["H"], Tp, B, True) * R
    for k, numel in (("ws", wsn), ("mse", R * nsteps), ("l1", R * nsteps), ("pred", R * n * N * Tp),
                     ("contrib", R * n * Tp * N * N)):
        bufs[k] = guarded(torch.full((numel,), float("nan"), device="cuda"))
    d = pack.dims(B, Tp + 1)
    hyper = pack.hyper(0, [0, 1])
    rc = mod.navar_lstm_run(d, mod.TRAIN, B, 1, 0, n, n + 6, bufs["X"][1], X[0].numel(), bufs["perm"][1].view(torch.int32),
                            n, bufs["par"][1], bufs["m"][1], bufs["v"][1], pack.n, hyper, bufs["mse"][1], bufs["l1"][1],
                            None, None, bufs["ws"][1])
    assert rc == 0
    rc = mod.navar_lstm_run(d, mod.FORWARD, B, 1, 0, n, n + 6, bufs["X"][1], X[0].numel(), None, 0, bufs["par"][1], None,
                            None, pack.n, None, None, None, bufs["pred"][1], bufs["contrib"][1], bufs["ws"][1])
    assert rc == 0
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert bands_intact(buf), k
        if k not in ("X", "ws", "perm"):
            assert torch.isfinite(view).all(), k
    assert torch.equal(bufs["par"][1].view(R, -1), ref.par) and torch.equal(bufs["m"][1].view(R, -1), ref.m)
    assert torch.equal(bufs["v"][1].view(R, -1), ref.v)
    assert torch.equal(bufs["mse"][1].view(R, -1), want[0]) and torch.equal(bufs["l1"][1].view(R, -1), want[1])
