"""GPU checks of the supervised DGCNN baseline's fit: redcliff_dgcnn_fit_run (csrc/rc_dgcnn_fit.hip) and
redcliff_amd.DGCNN_Model.fit / fit_dgcnn_baselines against the reference fixture tests/golden/dgcnn_fit.npz
(+ dgcnn_fit_e.npz) and the generic route (the reference's op structure on torch) run in float64 for shapes
the fixture lacks.  Parity at the project's state bound, the invariances bitwise."""
import math
import os

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_dgcnn_fit_host import (ATOL, RTOL, build, check_scenario_epochs, check_whole_fit, compare_state_dict,
                                 load_dgcnn, state_of)

pytestmark = pytest.mark.gpu

# (nodes, F, layers, hid, classes), rows, batch size, window rows
SHAPES = {"two": dict(shape=(3, 2, 2, 5, 2), N=20, B=6, T=4),      # ragged last batch of 2
          "three": dict(shape=(5, 3, 3, 33, 3), N=72, B=34, T=6),  # passes of 32 + 2 windows, ragged last batch of 4
          "one": dict(shape=(4, 2, 1, 7, 5), N=32, B=16, T=3)}     # one layer: A is left alone


def dg():
    from redcliff_amd import dgcnn
    return dgcnn


@pytest.fixture(params=["fused", "generic"])
def route(request, monkeypatch):
    monkeypatch.setenv("REDCLIFF_DGCNN_PATH", request.param)
    return request.param


def make_data(seed, N, T, n, C, R=None):
    rng = np.random.RandomState(seed)
    lead = () if R is None else (R,)
    return rng.rand(*(lead + (N, T, n))).astype(np.float32), rng.rand(*(lead + (N, C))).astype(np.float32)


def new_model(shape, seed, device="cuda"):
    from redcliff_amd import DGCNN_Model
    n, F, layers, H, C = shape
    torch.manual_seed(seed)
    return DGCNN_Model(n, 1, F, layers, H, C).to(device)


def make_pack(sh, R, seed=0, lrs=None, wds=None):
    """R seeded models of shape `sh` in one DgcnnFitPack, each with its own bound Adam."""
    models = [new_model(sh["shape"], seed + r) for r in range(R)]
    pack = dg().DgcnnFitPack(models)
    opts = []
    for r, m in enumerate(models):
        opts.append(torch.optim.Adam(m.dgcnn.parameters(), lr=(lrs or [1e-3] * R)[r], eps=1e-4,
                                     weight_decay=(wds or [1e-4] * R)[r]))
        pack.bind_optimizer(r, opts[-1])
    return pack, models, opts


def snap(pack):
    return [t.clone() for t in (pack.par, pack.m, pack.v, pack.rm, pack.rv)]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_scenarios_match_the_reference(name, route, tmp_path):
    meta, _ = load_dgcnn(name)
    m = build(meta, "cuda")
    opt = torch.optim.Adam(m.dgcnn.parameters(), **meta["adam"])
    assert m.fused_eligible(opt, T=meta["T"], Bmax=meta["B"]) == (route == "fused")
    m, opt = check_scenario_epochs(name, tmp_path, "cuda")
    assert ("_dg_slot" in m.__dict__) == (route == "fused")
    if meta["layers"] == 1:
        assert m.dgcnn.A not in opt.state
        if name == "c":
            _, sc = load_dgcnn(name)
            assert np.array_equal(state_of(m)["dgcnn.A"].view(np.int32), sc["init/dgcnn.A"].view(np.int32))


@pytest.mark.parametrize("name", ["a", "c"])
def test_whole_fits_match_the_reference(name, route, tmp_path):
    m, _ = check_whole_fit(name, tmp_path, "cuda")
    assert ("_dg_slot" in m.__dict__) == (route == "fused")
    for f in ("final_best_model.bin", "temp_best_model_epoch0.bin"):
        saved = torch.load(os.path.join(str(tmp_path), f), weights_only=False)
        assert "_dg_slot" not in saved.__dict__
        for k, t in saved.state_dict().items():
            assert t.untyped_storage().nbytes() == t.numel() * t.element_size(), k  # compact clones, not views of the pack
    final = torch.load(os.path.join(str(tmp_path), "final_best_model.bin"), weights_only=False)
    assert all(torch.equal(final.state_dict()[k], v) for k, v in m.state_dict().items())


def test_optimizer_rules_on_the_device(monkeypatch):
    monkeypatch.delenv("REDCLIFF_DGCNN_PATH", raising=False)
    m = new_model(SHAPES["two"]["shape"], 0)
    ps = list(m.dgcnn.parameters())
    assert m.fused_eligible(torch.optim.Adam(ps, lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.SGD(ps, lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.Adam(ps[:-1], lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.Adam(ps, lr=1e-3), T=4, Bmax=129)
    assert not new_model(SHAPES["two"]["shape"], 0).double().fused_eligible()


def test_pack_holds_parameters_moments_and_statistics_as_views():
    for key in ("two", "one"):
        sh = SHAPES[key]
        pack, models, opts = make_pack(sh, 2)
        for r, (m, opt) in enumerate(zip(models, opts)):
            lo, hi = pack.par[r].data_ptr(), pack.par[r].data_ptr() + pack.np_ * 4
            at = lo
            for prm in m.packed_parameters():
                assert prm.is_contiguous() and prm.data_ptr() == at
                at += prm.numel() * 4
                if sh["shape"][2] == 1 and prm is m.dgcnn.A:
                    assert prm not in opt.state
                    continue
                st = opt.state[prm]
                assert st["exp_avg"].is_contiguous() and st["exp_avg"].data_ptr() - pack.m[r].data_ptr() == prm.data_ptr() - lo
                assert st["exp_avg_sq"].data_ptr() - pack.v[r].data_ptr() == prm.data_ptr() - lo
            assert at == hi
            bn = m.dgcnn.BN1
            assert bn.running_mean.data_ptr() == pack.rm[r].data_ptr() and bn.running_var.data_ptr() == pack.rv[r].data_ptr()
            assert pack.bound(r)


# ------------------------------------------------------------------------------------------ float64 oracle
_MARGINS = []


def _margin_hook(mod, inputs):  # module level: the saved model pickles its hooks by name
    """Before a training-mode forward of the DGCNN: recomputes its two ReLU pre-activations z and, per
    element, the sum of the absolute terms a that make it up, and records min |z| / (sqrt(len) * 2^-24 * a)
    -- how many float32 roundings of its own products the closest pre-activation lies from zero
    (len = layers * F * nodes for the graph conv, nodes * hid for fc1).  An element whose terms are all
    exactly zero (a dead unit into a zero bias) is exact in any float format: 0 >= 0 holds for it."""
    if not mod.training:
        return
    from redcliff_amd.dgcnn import normalize_A
    with torch.no_grad():
        x = inputs[0]
        bn = mod.BN1
        mean, var = x.mean(dim=(0, 1)), x.var(dim=(0, 1), unbiased=False)
        xn = (x - mean) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias
        S, L = None, normalize_A(mod.A)
        Z, aZ = 0, 0
        for i, gc in enumerate(mod.layer1.gc1):
            S = None if i == 0 else (L if i == 1 else S @ L)
            t, at = (xn, xn.abs()) if i == 0 else (S @ xn, S.abs() @ xn.abs())
            Z, aZ = Z + t @ gc.weight, aZ + at @ gc.weight.abs()
        R = torch.relu(Z).reshape(x.shape[0], -1)
        W, b = mod.fc1.linear.weight, mod.fc1.linear.bias
        f1, af1 = R @ W.T + b, R @ W.abs().T + b.abs()
        n, F = x.shape[1], x.shape[2]
        for z, a, length in ((Z, aZ, len(mod.layer1.gc1) * F * n), (f1, af1, R.shape[1])):
            live = a > 0
            if bool(live.any()):
                _MARGINS.append(float((z.abs()[live] / (math.sqrt(length) * 2.0 ** -24 * a[live])).min()))


def fit_route(monkeypatch, which, shape, X, Y, B, epochs, adam, tmp, mseed=3, mutate=None, pre=None, device="cuda"):
    """One seeded model fitted `epochs` epochs (one fit() each) on route `which`: 'fused', 'generic', or
    'oracle' = the generic route in float64 (the same seeded float32 initial values and data, widened).
    Returns (model, optimizer, step losses, final validation losses, the oracle's ReLU margins)."""
    monkeypatch.setenv("REDCLIFF_DGCNN_PATH", "generic" if which == "oracle" else which)
    m = new_model(shape, mseed, device)
    if which == "oracle":
        m, X, Y = m.double(), X.astype(np.float64), Y.astype(np.float64)
        del _MARGINS[:]
        m.dgcnn.register_forward_pre_hook(_margin_hook)
    if mutate is not None:
        with torch.no_grad():
            mutate(m)
    opt = torch.optim.Adam(m.dgcnn.parameters(), **adam)
    if pre is not None:
        pre(m, opt)
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(Y)
    tr = [(Xt[i:i + B], Yt[i:i + B]) for i in range(0, len(Xt), B)]
    losses, evs = [], []
    for _ in range(epochs):
        evs.append(m.fit(str(tmp), tr, opt, 1, 1, 1, 0, None, tr[:1]))
        losses.append(m.step_losses)
    assert ("_dg_slot" in m.__dict__) == (which == "fused")
    return m, opt, np.concatenate(losses), evs, (list(_MARGINS) if which == "oracle" else None)


def compare_routes(monkeypatch, tmp, shape, N, B, T=None, epochs=2, adam=None, mutate=None, X=None, Y=None, seed=0,
                   pre=None, device="cuda"):
    """The fused route against the generic route run in float64 (on the GPU torch's float32
    backward leaves rounding residue on exactly-zero gradients, which Adam turns into steps; the float64 run
    is the generic route without that noise), at the state bound.  The data seed is the first of 0, 1, 2, ..
    whose float64 trajectory keeps every ReLU pre-activation at least one float32 rounding of its product
    away from zero (_margin_hook); the property is re-measured here on the oracle run."""
    n, F, layers, H, C = shape
    adam = dict(lr=1e-3, eps=1e-4) if adam is None else adam
    if X is None:
        X, Y = make_data(seed, N, F + 1 if T is None else T, n, C)
    g, go, gl, gev, seen = fit_route(monkeypatch, "oracle", shape, X, Y, B, epochs, adam, tmp, mutate=mutate, pre=pre,
                                     device=device)
    margin = min(seen)
    print("smallest ReLU margin of the float64 run: %.3g roundings over %d records" % (margin, len(seen)))
    assert margin >= 1.0, margin
    if device != "cuda":
        return None, g
    f, fo, fl, fev, _ = fit_route(monkeypatch, "fused", shape, X, Y, B, epochs, adam, tmp, mutate=mutate, pre=pre)
    got = state_of(f)
    assert all(np.isfinite(v).all() for v in got.values())
    compare_state_dict("fused vs generic", got, state_of(g))
    assert_close("loss", fl, gl, RTOL, ATOL)
    assert_close("eval", np.asarray(fev), np.asarray(gev), RTOL, ATOL)
    for pf, pg in zip(f.dgcnn.parameters(), g.dgcnn.parameters()):
        assert (pf in fo.state) == (pg in go.state)
        if pf in fo.state:
            assert float(fo.state[pf]["step"]) == float(go.state[pg]["step"])
    return f, g


EDGES = [
    dict(tag="B1_n2", shape=(2, 2, 2, 5, 2), N=3, B=1, seed=0),            # B * n = 2, the smallest BatchNorm allows
    dict(tag="ragged1", shape=(3, 2, 2, 5, 2), N=7, B=6, seed=0),          # a last batch of one window
    dict(tag="pass_of_1", shape=(3, 2, 3, 7, 2), N=67, B=33, seed=0),      # passes of 32 + 1 windows, then a batch of 1
    dict(tag="n1_h1_c1", shape=(1, 2, 2, 1, 1), N=12, B=4, seed=0),
    dict(tag="layers2", shape=(5, 3, 2, 18, 3), N=20, B=8, seed=0),
    dict(tag="layers3", shape=(5, 3, 3, 18, 3), N=20, B=8, seed=0),
    dict(tag="layers4", shape=(5, 3, 4, 18, 3), N=20, B=8, seed=0),
    dict(tag="wd0", shape=(4, 2, 3, 34, 2), N=20, B=8, seed=0, adam=dict(lr=1e-3, eps=1e-4, weight_decay=0.0)),
    dict(tag="wd", shape=(4, 2, 3, 34, 2), N=20, B=8, seed=0, adam=dict(lr=1e-3, eps=1e-4, weight_decay=1e-2)),
    # the largest batch, node count, width and layer count the limits allow (together: F = 1, C = 1).  A step
    # passes 1,048,576 graph-conv pre-activations through ReLU, of which some lie within rounding of zero under
    # any seed; this case is about sizes, so its model has positive graph-conv weights and a BatchNorm shift
    # of 3, which keeps all of them positive (the gates are the other cases' subject)
    dict(tag="largest", shape=(32, 1, 4, 256, 1), N=130, B=128, seed=11, epochs=1, mutate="positive"),
]
# data seeds of the cases below (the rule of compare_routes)
SEEDS = dict(gate=0, isolated=0, constant=0, resume=0)


def positive(m):
    for gc in m.dgcnn.layer1.gc1:
        gc.weight.abs_()
    m.dgcnn.BN1.bias.fill_(3.0)


@pytest.mark.parametrize("case", EDGES, ids=lambda c: c["tag"])
def test_edge_shapes_against_generic(case, monkeypatch, tmp_path):
    run_edge(case, monkeypatch, tmp_path)


def run_edge(case, monkeypatch, tmp, device="cuda"):
    c = dict(case)
    c.pop("tag")
    if c.get("mutate") == "positive":
        c["mutate"] = positive
    return compare_routes(monkeypatch, tmp, c.pop("shape"), c.pop("N"), c.pop("B"), device=device, **c)


def run_gate(monkeypatch, tmp, device="cuda"):
    def mutate(m):
        m.dgcnn.A[0, 1] = 0.0
        m.dgcnn.A[1, 2] = -0.25
    return compare_routes(monkeypatch, tmp, (4, 2, 3, 9, 2), 20, 8, adam=dict(lr=1e-3, eps=1e-4), mutate=mutate,
                          seed=SEEDS["gate"], device=device)


def test_relu_gate_of_A_passes_no_gradient_at_zero(monkeypatch, tmp_path):
    """An entry of A exactly 0 and one negative: neither receives a gradient, so without weight decay both
    keep their bits (Adam's update of a zero gradient from zero moments is zero)."""
    f, g = run_gate(monkeypatch, tmp_path)
    for m in (f, g):
        assert float(m.dgcnn.A[0, 1].detach()) == 0.0 and float(m.dgcnn.A[1, 2].detach()) == -0.25


def run_isolated(monkeypatch, tmp, device="cuda"):
    def mutate(m):
        A = m.dgcnn.A
        A[2, :] = -A[2, :].abs() - 0.01
        A[:, 2] = -A[:, 2].abs() - 0.01
    return compare_routes(monkeypatch, tmp, (4, 2, 3, 9, 2), 20, 8, adam=dict(lr=1e-3, eps=1e-4), mutate=mutate,
                          seed=SEEDS["isolated"], device=device)


def test_isolated_node(monkeypatch, tmp_path):
    """Node 2's row and column of A have no positive entry: its degree factor is 1e5 and multiplies exact zeros."""
    f, g = run_isolated(monkeypatch, tmp_path)
    assert bool((f.dgcnn.A[2, :] < 0).all()) and bool((f.dgcnn.A[:, 2] < 0).all())


def run_constant(monkeypatch, tmp, device="cuda"):
    shape, N, B = (3, 2, 2, 5, 2), 12, 6
    X, Y = make_data(SEEDS["constant"], N, 3, shape[0], shape[4])
    X[:, 1, :] = 0.375  # variance 0: the normalised feature is exactly 0
    return compare_routes(monkeypatch, tmp, shape, N, B, X=X, Y=Y, device=device)


def test_feature_constant_over_the_batch(monkeypatch, tmp_path):
    f, _ = run_constant(monkeypatch, tmp_path)
    assert float(f.dgcnn.BN1.running_var[1]) < 1.0


def run_resume(monkeypatch, tmp_path, device="cuda"):
    sh = SHAPES["three"]
    X, Y = make_data(SEEDS["resume"], sh["N"], sh["T"], sh["shape"][0], sh["shape"][4])
    B = sh["B"]

    def torch_epoch(m, opt):  # before the fit under test
        keep = os.environ["REDCLIFF_DGCNN_PATH"]
        monkeypatch.setenv("REDCLIFF_DGCNN_PATH", "generic")
        dt = m.dgcnn.A.dtype
        Xt, Yt = torch.from_numpy(X).to(dt), torch.from_numpy(Y).to(dt)
        tr = [(Xt[i:i + B], Yt[i:i + B]) for i in range(0, len(Xt), B)]
        m.fit(str(tmp_path), tr, opt, 1, 1, 1, 0, None, tr[:1])
        assert "_dg_slot" not in m.__dict__
        monkeypatch.setenv("REDCLIFF_DGCNN_PATH", keep)
    return compare_routes(monkeypatch, tmp_path, sh["shape"], sh["N"], B, X=X, Y=Y, epochs=1, pre=torch_epoch, device=device)


def test_resume_from_a_torch_stepped_optimizer(monkeypatch, tmp_path):
    """One torch-stepped (generic) epoch, then a fused epoch with the same optimizer: its moments and step
    count are copied into the pack."""
    f, g = run_resume(monkeypatch, tmp_path)
    nb = -(-SHAPES["three"]["N"] // SHAPES["three"]["B"])
    assert int(f.dgcnn.BN1.num_batches_tracked) == int(g.dgcnn.BN1.num_batches_tracked) == 2 * nb


# ------------------------------------------------------------------------------------------ bitwise invariants
@pytest.mark.parametrize("key", ["two", "three", "one"])
def test_two_runs_agree_and_one_call_equals_a_call_per_batch(key):
    sh = SHAPES[key]
    N, B = sh["N"], sh["B"]
    Xh, Yh = make_data(1, N, sh["T"], sh["shape"][0], sh["shape"][4])
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    outs = []
    for split in (False, False, True):
        pack, models, _ = make_pack(sh, 1)
        if not split:
            loss = pack.train(X, 0, Y, 0, 0, N, B)
        else:
            loss = torch.cat([pack.train(X, 0, Y, 0, s, min(B, N - s), B) for s in range(0, N, B)], 1)
        assert pack.opt[0]["t"] == -(-N // B) == int(models[0].dgcnn.BN1.num_batches_tracked)
        outs.append(snap(pack) + [loss])
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][1], torch.zeros_like(outs[0][1]))
    assert same_bits(outs[0], outs[1]), "two runs differ"
    assert same_bits(outs[0], outs[2]), "an epoch in one call differs from one call per batch"


@pytest.mark.parametrize("key", ["two", "three"])
def test_replicas_are_independent(key):
    sh = SHAPES[key]
    N, B, R = sh["N"], sh["B"], 3
    lrs, wds = [1e-3, 2e-3, 5e-4], [1e-4, 0.0, 1e-2]
    Xh, Yh = make_data(2, N, sh["T"], sh["shape"][0], sh["shape"][4], R)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    xps, yps = X[0].numel(), Y[0].numel()
    pack, _, _ = make_pack(sh, R, lrs=lrs, wds=wds)
    before = snap(pack)
    loss = pack.train(X, xps, Y, yps, 0, N, B)
    for r in range(R):  # R = 3 in one call equals three R = 1 calls
        one, _, _ = make_pack(sh, 1, seed=r, lrs=[lrs[r]], wds=[wds[r]])
        l1 = one.train(X[r].contiguous(), 0, Y[r].contiguous(), 0, 0, N, B)
        assert same_bits([t[r] for t in snap(pack)] + [loss[r]], [t[0] for t in snap(one)] + [l1[0]]), r
    # a replica list [0, 2] leaves replica 1 untouched and steps 0 and 2 as the full call did
    part, pmods, _ = make_pack(sh, R, lrs=lrs, wds=wds)
    pl = part.train(X, xps, Y, yps, 0, N, B, active=[0, 2])
    assert pl.shape[0] == 2
    for t, b, full in zip(snap(part), before, snap(pack)):
        assert torch.equal(t[1], b[1]) and torch.equal(t[0], full[0]) and torch.equal(t[2], full[2])
    assert torch.equal(pl, loss[[0, 2]])
    assert part.opt[1]["t"] == 0 and part.opt[0]["t"] == -(-N // B) and int(pmods[1].dgcnn.BN1.num_batches_tracked) == 0
    # an empty list launches nothing
    held = snap(part)
    el = part.train(X, xps, Y, yps, 0, N, B, active=[])
    assert el.shape[0] == 0 and same_bits(held, snap(part))
    # shared and per-replica data agree
    Xs, Ys = X[0].contiguous(), Y[0].contiguous()
    a, _, _ = make_pack(sh, R, lrs=lrs, wds=wds)
    b, _, _ = make_pack(sh, R, lrs=lrs, wds=wds)
    ra = a.train(Xs, 0, Ys, 0, 0, N, B)
    rb = b.train(torch.stack([Xs] * R).contiguous(), Xs.numel(), torch.stack([Ys] * R).contiguous(), Ys.numel(), 0, N, B)
    assert same_bits(snap(a) + [ra], snap(b) + [rb])


@pytest.mark.parametrize("key", ["two", "three", "one"])
def test_forward_splits_and_only_reads(key):
    sh = SHAPES[key]
    N, R, B = 150, 2, 64
    n, F, _, _, C = sh["shape"]
    Xh, Yh = make_data(3, N, sh["T"], n, C, R)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    xps, yps = X[0].numel(), Y[0].numel()
    pack, models, _ = make_pack(sh, R)
    pack.train(X, xps, Y, yps, 0, 40, 20)  # running statistics away from (0, 1)
    pack.m.normal_()
    pack.v.uniform_()
    before = snap(pack)
    pred, mse = pack.forward(X, xps, Y, yps, 0, N, B)  # batches of 64, 64, 22
    assert same_bits(before, snap(pack))
    m = 128
    p0, e0 = pack.forward(X, xps, Y, yps, 0, m, B)
    p1, e1 = pack.forward(X, xps, Y, yps, m, N - m, B)
    assert torch.equal(pred, torch.cat([p0, p1], 1)) and torch.equal(mse, torch.cat([e0, e1], 1))
    p2, e2 = pack.forward(X, xps, None, 0, 0, N, B)
    assert e2 is None and torch.equal(p2, pred)
    for r in range(R):  # and it is the module's forward in eval mode
        models[r].eval()
        with torch.no_grad():
            want = models[r](X[r][:, :F, :].transpose(1, 2))
        assert_close("pred", pred[r].cpu().numpy(), want.cpu().numpy(), RTOL, ATOL)
        wm = [float(torch.nn.functional.mse_loss(want[i:i + B], Y[r][i:i + B])) for i in range(0, N, B)]
        assert_close("mse", mse[r].cpu().numpy(), np.asarray(wm), RTOL, ATOL)


def test_fit_dgcnn_baselines_equals_three_fits(tmp_path):
    """Three same-shape models in one pack, the second with lr = 0: its stopping criterion never moves, so it
    stops at the first check after it = 0 while the pack goes on with the others."""
    from redcliff_amd import fit_dgcnn_baselines
    sh = SHAPES["three"]
    R, N, B = 3, sh["N"], sh["B"]
    n, F, _, _, C = sh["shape"]
    data = [make_data(20 + r, N, sh["T"], n, C) for r in range(R)]
    vdata = [make_data(30 + r, 40, sh["T"], n, C) for r in range(R)]
    ld = lambda XY: [(torch.from_numpy(XY[0][i:i + B]), torch.from_numpy(XY[1][i:i + B])) for i in range(0, len(XY[0]), B)]
    # weight decay far above the loss gradient: A's positive entries shrink towards zero faster than its
    # largest one does in proportion, so the criterion of models 0 and 2 keeps falling
    lrs, wds = [5e-3, 0.0, 2e-3], [1.0, 1e-4, 0.5]

    def fresh():
        ms = [new_model(sh["shape"], 40 + r) for r in range(R)]
        return ms, [torch.optim.Adam(m.dgcnn.parameters(), lr=lrs[r], eps=1e-4, weight_decay=wds[r]) for r, m in enumerate(ms)]
    pm, po = fresh()
    dirs = [str(tmp_path / ("p%d" % r)) for r in range(R)] + [str(tmp_path / ("s%d" % r)) for r in range(R)]
    lv_p = fit_dgcnn_baselines(pm, dirs[:R], [ld(d) for d in data], po, 6, 1, 1, 0, [None] * R, [ld(d) for d in vdata])
    assert pm[0].__dict__["_dg_slot"][0] is pm[2].__dict__["_dg_slot"][0] and pm[0].__dict__["_dg_slot"][0].R == R
    stopped = [m.stopped_at for m in pm]
    print("stopped at", stopped)
    assert stopped[1] == 1 and max(stopped) > 1, stopped
    sm, so = fresh()
    nb = -(-N // B)
    for r in range(R):
        lv = sm[r].fit(dirs[R + r], ld(data[r]), so[r], 6, 1, 1, 0, None, ld(vdata[r]))
        assert float(lv) == float(lv_p[r]) and float(lv) > 0
        assert sm[r].stopped_at == stopped[r] and sm[r].avg_factor_loss == pm[r].avg_factor_loss
        a, b = state_of(pm[r]), state_of(sm[r])
        assert all(np.array_equal(a[k], b[k]) for k in a)
        for x, y in zip(pm[r].dgcnn.parameters(), sm[r].dgcnn.parameters()):
            sx, sy = po[r].state[x], so[r].state[y]
            assert torch.equal(sx["exp_avg"], sy["exp_avg"]) and torch.equal(sx["exp_avg_sq"], sy["exp_avg_sq"])
            assert float(sx["step"]) == float(sy["step"]) == float((stopped[r] + 1) * nb)
        assert torch.equal(pm[r].GC(threshold=False), sm[r].GC(threshold=False))
        assert np.array_equal(pm[r].step_losses, sm[r].step_losses)
        assert sorted(os.listdir(dirs[r])) == sorted(os.listdir(dirs[R + r]))
        la = torch.load(os.path.join(dirs[r], "final_best_model.bin"), weights_only=False)
        lb = torch.load(os.path.join(dirs[R + r], "final_best_model.bin"), weights_only=False)
        assert all(torch.equal(la.state_dict()[k], lb.state_dict()[k]) for k in la.state_dict())


# ------------------------------------------------------------------------------------------ guard bands
def guarded(t, band=257):
    """A copy of `t` with NaN bands on both sides: (whole buffer, view of the payload).  The band is odd, so
    the payload is only 4-byte aligned unless the caller asks for an even one."""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + 2 * band,), float("nan"), device="cuda", dtype=torch.float32)
    view = buf[band:band + flat.numel()]
    view.copy_(flat)
    return buf, view


def bands_intact(buf, band=257):
    return bool(torch.isnan(buf[:band]).all() and torch.isnan(buf[-band:]).all())


@pytest.mark.parametrize("key", ["two", "three", "one"])
def test_nan_guard_bands(key):
    sh = SHAPES[key]
    N, B, R, T = sh["N"], sh["B"], 2, sh["T"]
    n, F, layers, H, C = sh["shape"]
    d_ = dg()
    pack, _, _ = make_pack(sh, R)
    ref, _, _ = make_pack(sh, R)
    Xh, Yh = make_data(8, N + 6, T, n, C, R)
    Xh[:, N:] = np.nan  # rows no batch names
    Yh[:, N:] = np.nan
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    want = ref.train(X, X[0].numel(), Y, Y[0].numel(), 0, N, B)
    wpred, wmse = ref.forward(X, X[0].numel(), Y, Y[0].numel(), 0, N, B)
    nsteps = -(-N // B)
    bufs = {}
    for k, t in (("X", X), ("Y", Y), ("par", pack.par), ("m", pack.m), ("v", pack.v), ("rm", pack.rm), ("rv", pack.rv)):
        bufs[k] = guarded(t)
    wsn = d_.dgcnn_fit_ws_floats(n, F, layers, H, C, B, N) * R
    for k, numel, band in (("ws", wsn, 258), ("loss", R * nsteps, 257), ("mse", R * nsteps, 257), ("pred", R * N * C, 257)):
        bufs[k] = guarded(torch.full((numel,), float("nan"), device="cuda"), band)
    d = pack.dims(B, T)
    hyper = pack.hyper(0, [0, 1])
    args = (bufs["X"][1], X[0].numel(), bufs["Y"][1], Y[0].numel(), bufs["par"][1], bufs["m"][1], bufs["v"][1], pack.np_,
            bufs["rm"][1], bufs["rv"][1], hyper)
    assert d_.dgcnn_fit_run(d, d_.TRAIN, B, 1, 0, N, N + 6, *args, bufs["loss"][1], None, bufs["ws"][1]) == 0
    assert d_.dgcnn_fit_run(d, d_.FORWARD, B, 1, 0, N, N + 6, *args, bufs["mse"][1], bufs["pred"][1], bufs["ws"][1]) == 0
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert bands_intact(buf, 258 if k == "ws" else 257), k
    got = [bufs[k][1].reshape(R, -1) for k in ("par", "m", "v", "rm", "rv")]
    assert same_bits(got + [bufs["loss"][1].reshape(R, -1)], [t.reshape(R, -1) for t in snap(ref)] + [want])
    assert torch.equal(bufs["pred"][1].reshape(R, N, C), wpred) and torch.equal(bufs["mse"][1].reshape(R, -1), wmse)
    assert all(torch.isfinite(t).all() for t in got)
