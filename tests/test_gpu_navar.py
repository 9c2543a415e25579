"""GPU checks of the NAVAR baseline: redcliff_navar_run (csrc/rc_navar.hip) and redcliff_amd.NAVAR /
fit_navar_baselines against the reference fixture tests/golden/navar.npz and the generic route (the
reference's op structure on torch) for shapes the fixture lacks.  Parity at the project's state
bound, the invariances bitwise."""
import os

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_navar_host import (ATOL, RTOL, build, check_scenario_epochs, compare_state_dict, load_navar, state_of, sub)

pytestmark = pytest.mark.gpu

SHAPES = {"one": dict(N=3, H=5, K=2, layers=1, n=20, B=6),      # ragged last batch of 2
          "two": dict(N=4, H=33, K=3, layers=2, n=40, B=16)}    # two unit slices, ragged last batch of 8


def nv():
    from redcliff_amd import navar
    return navar


@pytest.fixture(params=["fused", "generic"])
def route(request, monkeypatch):
    monkeypatch.setenv("REDCLIFF_NAVAR_PATH", request.param)
    return request.param


def windows(seed, n, T, N, R=None):
    rng = np.random.RandomState(seed)
    X = rng.randn(*((n, T, N) if R is None else (R, n, T, N))).astype(np.float32)
    return X


def new_model(N, H, K, layers, seed):
    from redcliff_amd import NAVAR
    torch.manual_seed(seed)
    return NAVAR(N, H, K, hidden_layers=layers).to("cuda")


def make_pack(sh, R, seed=0, lrs=None, lams=None, wd=0.0):
    """R seeded models of shape `sh` in one NavarPack, each with its own bound Adam."""
    models = [new_model(sh["N"], sh["H"], sh["K"], sh["layers"], seed + r) for r in range(R)]
    pack = nv().NavarPack(models)
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
    meta, _ = load_navar(name)
    m = build(meta, "cuda")
    opt = torch.optim.Adam(m.parameters(), **meta["adam"])
    assert m.fused_eligible(torch.nn.MSELoss(), opt, T=meta["K"] + 1, Bmax=min(meta["B"], meta["n"])) == (route == "fused")
    check_scenario_epochs(name, tmp_path, "cuda")


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("v", [0, 5])
def test_whole_fits_match_the_reference(name, v, route, tmp_path):
    meta, sc = load_navar(name)
    m = build(meta, "cuda")
    opt = torch.optim.Adam(m.parameters(), **meta["adam"])
    np.random.seed(meta["seed"] + 300)
    lv = m.fit(str(tmp_path), np.array(sc["X_train"]), None, torch.nn.MSELoss(), opt, X_val=np.array(sc["X_val"]),
               val_proportion=v / 10.0, epochs=meta["epochs"], batch_size=meta["B"], check_every=2, lambda1=meta["lam"])
    assert ("_nv_slot" in m.__dict__) == (route == "fused")
    pre = "fit%d" % v
    compare_state_dict("%s/%s" % (name, pre), state_of(m), sub(sc, pre + "/final"))
    assert_close("causal", m.GC(), sc[pre + "/causal"], RTOL, ATOL)
    assert_close("loss_val", float(lv), sc[pre + "/loss_val"], RTOL, ATOL)
    saved = torch.load(os.path.join(str(tmp_path), "final_best_model.bin"), weights_only=False)
    assert "_nv_slot" not in saved.__dict__ and np.array_equal(saved.GC(), m.GC())
    for k, t in saved.state_dict().items():
        assert t.untyped_storage().nbytes() == t.numel() * 4, k  # compact clones, not views of the pack


_MIN_ABS = []


def _min_abs_hook(mod, inp, out):  # module level: the saved model pickles its hooks by name
    if mod.training:
        _MIN_ABS.append(float(out.detach().abs().min()))


def fit_route(monkeypatch, which, N, H, K, layers, X, B, epochs, lam, adam, tmp, seed=3, mutate=None, pre=None):
    """One seeded model fitted on route `which`: 'fused', 'generic', or 'oracle' = the generic route in
    float64 (the same seeded float32 initial values and data, widened).  Returns (model, optimizer)."""
    monkeypatch.setenv("REDCLIFF_NAVAR_PATH", "generic" if which == "oracle" else which)
    m = new_model(N, H, K, layers, seed)
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


def compare_routes(monkeypatch, tmp, N, H, K, layers, n, B, epochs=2, lam=0.05, adam=None, mutate=None, X=None,
                   pre_oracle=None):
    """The fused route against the generic route.  The generic side runs in float64: on the GPU torch's
    float32 grouped-convolution backward leaves rounding residue (|g| ~ 1e-9) on gradients that are
    exactly zero (dead units), which Adam at its default eps = 1e-8 turns into steps of a good part of lr,
    so the float32 generic route is itself outside the state bound against float64 on such inputs
    (DESIGN 17); the float64 run is the generic route without that noise."""
    adam = dict(lr=1e-3) if adam is None else adam
    X = windows(N * 1000 + H, n, K + 1, N) if X is None else X
    f, fo = fit_route(monkeypatch, "fused", N, H, K, layers, X, B, epochs, lam, adam, tmp, mutate=mutate)
    g, go = fit_route(monkeypatch, "oracle", N, H, K, layers, X, B, epochs, lam, adam, tmp, mutate=mutate, pre=pre_oracle)
    want = state_of(g)
    assert all(np.isfinite(v).all() for v in state_of(f).values())
    compare_state_dict("fused vs generic", state_of(f), want)
    assert_close("mse", f.step_losses[0], g.step_losses[0], RTOL, ATOL)
    assert_close("l1", f.step_losses[1], g.step_losses[1], RTOL, ATOL)
    assert_close("causal", f.GC(), g.GC(), RTOL, ATOL)
    for pf, pg in zip(f.parameters(), g.parameters()):
        assert float(fo.state[pf]["step"]) == float(go.state[pg]["step"])
    return f, g


def test_published_shape_fused_against_generic(monkeypatch, tmp_path):
    """N 10, H 256, K 20, two layers, B 128, n 300 (128, 128, 44), 2 epochs, Adam(lr 1e-4) at the default eps.
    3.07 million pre-activations pass through clamp(min=0) on the way; where one lies within float32
    rounding of zero, two float32 realisations open different gates and that row of W2 moves by lr
    under Adam, whichever realisation is `right`.  The data seed is therefore the first of 0, 1, 2, ...
    whose FLOAT64 trajectory keeps every pre-activation at least 5e-7 from zero (5e-7: sqrt(256) *
    2^-24 * 0.5, a 256-term float32 product of operands below 0.5); the test re-measures that margin
    on its oracle run, so the choice does not depend on the code under test."""
    N, H, K = 10, 256, 20
    X = np.random.RandomState(3).randn(300, K + 1, N).astype(np.float32)

    def watch(m, opt):
        m.first_hidden_layer.register_forward_hook(_min_abs_hook)
        m.hidden_layer_list[0].register_forward_hook(_min_abs_hook)
    _MIN_ABS.clear()
    try:
        compare_routes(monkeypatch, tmp_path, N, H, K, 2, 300, 128, epochs=2, lam=0.0, adam=dict(lr=1e-4), X=X,
                       pre_oracle=watch)
    finally:
        print("smallest |pre-activation| of the float64 run: %.3e over %d forwards" % (min(_MIN_ABS), len(_MIN_ABS)))
    assert len(_MIN_ABS) == 12 and min(_MIN_ABS) >= 5e-7


# ------------------------------------------------------------------------------------------ bitwise invariants
@pytest.mark.parametrize("shape", ["one", "two"])
def test_two_runs_agree_and_one_call_equals_a_call_per_batch(shape):
    sh = SHAPES[shape]
    n, B = sh["n"], sh["B"]
    X = torch.from_numpy(windows(1, n, sh["K"] + 1, sh["N"])).cuda()
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
    X = torch.from_numpy(windows(2, n, sh["K"] + 1, sh["N"], R)).cuda()
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
    X = torch.from_numpy(windows(3, n, sh["K"] + 1, sh["N"], R)).cuda()
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
    for r in range(R):  # and it is the module's forward
        with torch.no_grad():
            wp, wc = models[r](X[r].transpose(1, 2)[:, :, :-1])
        assert_close("pred", pred[r].cpu().numpy(), wp.cpu().numpy(), RTOL, ATOL)
        assert_close("contrib", contrib[r].cpu().numpy(), wc[:, :, 0].cpu().numpy(), RTOL, ATOL)


def test_fit_navar_baselines_equals_three_fits(tmp_path):
    from redcliff_amd import fit_navar_baselines
    sh = SHAPES["two"]
    R, n = 3, sh["n"]
    Xs = [windows(20 + r, n, sh["K"] + 1, sh["N"]) for r in range(R)]
    Xv = [windows(30 + r, 12, sh["K"] + 1, sh["N"]) for r in range(R)]

    def fresh():
        ms = [new_model(sh["N"], sh["H"], sh["K"], sh["layers"], 40 + r) for r in range(R)]
        return ms, [torch.optim.Adam(m.parameters(), lr=1e-3 * (r + 1)) for r, m in enumerate(ms)]
    pm, po = fresh()
    dirs = [str(tmp_path / ("p%d" % r)) for r in range(R)] + [str(tmp_path / ("s%d" % r)) for r in range(R)]
    for d in dirs:
        os.makedirs(d)
    kw = dict(val_proportion=0.5, epochs=3, batch_size=sh["B"], check_every=2, lambda1=0.05)
    lv_p = fit_navar_baselines(pm, dirs[:R], Xs, torch.nn.MSELoss(), po, X_vals=Xv,
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
    dict(tag="B1", N=3, H=5, K=2, layers=1, n=4, B=1),
    dict(tag="B1_two", N=3, H=5, K=2, layers=2, n=4, B=1),
    dict(tag="ragged1", N=3, H=5, K=2, layers=2, n=7, B=6),
    dict(tag="ragged1_pass", N=2, H=7, K=3, layers=2, n=130, B=65),   # a second pass of one window; then 65 = 64 + 1
    dict(tag="H1", N=3, H=1, K=2, layers=1, n=20, B=6),
    dict(tag="H1_two", N=3, H=1, K=2, layers=2, n=20, B=6),
    dict(tag="N1", N=1, H=5, K=2, layers=2, n=20, B=6),
    dict(tag="wd0", N=3, H=34, K=4, layers=2, n=20, B=8, adam=dict(lr=1e-3, weight_decay=0.0)),
    dict(tag="wd", N=3, H=34, K=4, layers=2, n=20, B=8, adam=dict(lr=1e-3, weight_decay=1e-2)),
    dict(tag="one_layer_slices", N=5, H=70, K=64, layers=1, n=40, B=16),
    dict(tag="N32", N=32, H=16, K=2, layers=2, n=20, B=8),
], ids=lambda c: c["tag"])
def test_edge_shapes_against_generic(case, monkeypatch, tmp_path):
    c = dict(case)
    c.pop("tag")
    compare_routes(monkeypatch, tmp_path, c.pop("N"), c.pop("H"), c.pop("K"), c.pop("layers"), c.pop("n"), c.pop("B"), **c)


@pytest.mark.parametrize("layers", [1, 2])
def test_unit_with_zero_preactivation_still_gets_gradient(layers, monkeypatch, tmp_path):
    """z == 0 exactly: clamp(min=0) passes the gradient there (unlike ReLU), so the unit's bias moves."""
    N, H, K = 3, 5, 2

    def mutate(m):
        layer = m.first_hidden_layer if layers == 1 else m.hidden_layer_list[0]
        layer.weight[0 * H + 2].zero_()
        layer.bias[0 * H + 2] = 0.0
    f, g = compare_routes(monkeypatch, tmp_path, N, H, K, layers, 6, 300, epochs=1, mutate=mutate)
    for m in (f, g):
        layer = m.first_hidden_layer if layers == 1 else m.hidden_layer_list[0]
        assert float(layer.bias[2]) != 0.0 and float(layer.weight[2].abs().sum()) != 0.0


def test_zero_contribution_has_zero_l1_gradient(monkeypatch, tmp_path):
    N, H, K = 3, 5, 2

    def mutate(m):
        m.contributions.weight[0 * N + 1].zero_()
        m.contributions.bias[0 * N + 1] = 0.0
    f, g = compare_routes(monkeypatch, tmp_path, N, H, K, 2, 6, 300, epochs=1, lam=0.5, mutate=mutate)
    assert np.isfinite(f.GC()).all() and np.isfinite(f.step_losses[1]).all() and f.step_losses[1][0] > 0


def test_resume_from_a_torch_stepped_optimizer(monkeypatch, tmp_path):
    """One torch-stepped (generic, float32) epoch, then a fused epoch with the same optimizer: its moments
    and step count are copied into the pack.  Adam eps 1e-4 as tests/test_gpu_fm.py, so that the float32
    torch epoch's rounding residue on exactly-zero gradients does not move weights (compare_routes)."""
    sh = SHAPES["two"]
    X = windows(5, sh["n"], sh["K"] + 1, sh["N"])
    args = (sh["N"], sh["H"], sh["K"], sh["layers"], X, sh["B"])
    adam = dict(lr=1e-3, eps=1e-4)

    def torch_epoch(m, opt):  # before the fit under test
        keep = os.environ["REDCLIFF_NAVAR_PATH"]
        monkeypatch.setenv("REDCLIFF_NAVAR_PATH", "generic")
        Xm = X.astype(np.float64) if m.biases.dtype == torch.float64 else X
        m.fit(str(tmp_path), Xm, None, torch.nn.MSELoss(), opt, epochs=1, batch_size=sh["B"], lambda1=0.05,
              rng=np.random.RandomState(99))
        assert "_nv_slot" not in m.__dict__
        monkeypatch.setenv("REDCLIFF_NAVAR_PATH", keep)
    f, fo = fit_route(monkeypatch, "fused", *args, 1, 0.05, adam, tmp_path, pre=torch_epoch)
    g, go = fit_route(monkeypatch, "oracle", *args, 1, 0.05, adam, tmp_path, pre=torch_epoch)
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
    N, n, B, R = sh["N"], sh["n"], sh["B"], 2
    navar = nv()
    pack, _, _ = make_pack(sh, R)
    ref, _, _ = make_pack(sh, R)
    Xh = windows(8, n + 6, sh["K"] + 1, N, R)
    Xh[:, n:] = np.nan  # rows the permutation never names
    X = torch.from_numpy(Xh).cuda()
    perm = perms_for(R, n, 13)
    want = ref.train(X, X[0].numel(), perm, n, n, B)
    nsteps = -(-n // B)
    bufs = {}
    for k, t in (("X", X), ("perm", perm), ("par", pack.par), ("m", pack.m), ("v", pack.v)):
        bufs[k] = guarded(t)
    wsn = navar.navar_ws_floats(N, sh["H"], sh["layers"], B) * R
    for k, numel in (("ws", wsn), ("mse", R * nsteps), ("l1", R * nsteps), ("pred", R * n * N), ("contrib", R * n * N * N)):
        bufs[k] = guarded(torch.full((numel,), float("nan"), device="cuda"))
    d = pack.dims(B, sh["K"] + 1)
    hyper = pack.hyper(0, [0, 1])
    rc = navar.navar_run(d, navar.TRAIN, B, 1, 0, n, n + 6, bufs["X"][1], X[0].numel(), bufs["perm"][1].view(torch.int32), n,
                         bufs["par"][1], bufs["m"][1], bufs["v"][1], pack.n, hyper, bufs["mse"][1], bufs["l1"][1], None,
                         None, bufs["ws"][1])
    assert rc == 0
    rc = navar.navar_run(d, navar.FORWARD, B, 1, 0, n, n + 6, bufs["X"][1], X[0].numel(), None, 0, bufs["par"][1], None,
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


@pytest.mark.parametrize("layers,H", [(2, 272), (1, 512)])
def test_largest_batch_and_width_against_generic(layers, H, monkeypatch, tmp_path):
    navar = nv()
    assert navar.navar_supported(2, H, 2, layers, Bmax=512) > 0
    assert navar.navar_supported(2, H + 1, 2, layers, Bmax=512) == 0 and navar.navar_supported(2, H, 2, layers, Bmax=513) == 0
    compare_routes(monkeypatch, tmp_path, 2, H, 2, layers, 1024, 512, epochs=1, lam=0.01)
