"""The fused cEmbedder training / validation step (csrc/rc_cemb.hip + the matrix-core factor chain,
redcliff_amd.cemb_engine; opt-in with REDCLIFF_CEMB_PATH=fused) against the reference's golden
vectors (tests/golden/cemb.npz) and the CPU oracle (oracle.redcliff_oracle.OCEmbedder /
OracleREDCLIFF), plus determinism, path switching, checkpoints, the fallback, guard bands and the
replica axis of the C ABI.

Tolerances are those of the suites this path sits beside: the golden schedule as
test_gpu_generic.compare_state (rtol 1e-4, atol 1e-5 x max(1, |want|max)), the oracle runs as
test_gpu_parity._three_phases_vs_oracle (state rtol 2e-4 / atol 5e-6, validation terms 1e-4 / 1e-6,
lagged conditional GC 1e-4 / 1e-5 with identical > 0 patterns)."""
import ctypes
import io

import numpy as np
import pytest
import torch

from golden_io import assert_close, batches, ctor_args, load, state
from test_gpu_generic import compare_state as golden_compare
from test_gpu_parity import compare_state as oracle_compare
from test_gpu_parity import synth

pytestmark = pytest.mark.gpu

MODE = "pretrain_embedder_then_acclimate_factors_then_combined"
SHAPES = {
    # batches 21 / 21 / 8; odd sizes across the 16-unit block edge
    "ragged": dict(p=7, L=3, K=5, nsup=2, h=19, F=9, eh=17, B=21, N=50, T=12, label_T=12, sigmoid=False),
    "sigmoid": dict(p=4, L=2, K=4, nsup=2, h=6, F=5, eh=5, B=16, N=40, T=6, label_T=1, sigmoid=True),
    # one factor: the sum over cosine pairs is empty; F == L
    "k1_feql": dict(p=3, L=3, K=1, nsup=1, h=8, F=3, eh=4, B=16, N=32, T=12, label_T=12, sigmoid=False),
    # no supervised factor; eh crosses a 32-unit block
    "unsup": dict(p=6, L=3, K=2, nsup=0, h=8, F=4, eh=33, B=16, N=32, T=12, label_T=12, sigmoid=False),
    "tstlike": dict(p=12, L=4, K=9, nsup=3, h=25, F=16, eh=25, B=32, N=72, T=20, label_T=20, sigmoid=False),
}


@pytest.fixture
def fused(monkeypatch):
    monkeypatch.setenv("REDCLIFF_CEMB_PATH", "fused")


def golden_model():
    import redcliff_amd
    d, meta = load("cemb")
    args, kw = ctor_args(meta)
    torch.manual_seed(meta["seed"])
    cls = redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing if meta["smoothing_class"] else redcliff_amd.REDCLIFF_S_CMLP
    return d, meta, cls(*args, **kw).float().cuda()


def adam_pair(m, lrA, lrB):
    oA = torch.optim.Adam(m.gen_model[0].parameters(), lr=lrA, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-4)
    oB = torch.optim.Adam(m.gen_model[1].parameters(), lr=lrB, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-4)
    return oA, oB


def snapshot(m):
    torch.cuda.synchronize()
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


def assert_same_bits(a, b, tag):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (tag, k))


def model_args(cfg, **over):
    from oracle.redcliff_oracle import reference_coeffs
    eargs = [("sigmoid_eccentricity_coeff", 10.0), ("lag", cfg["F"]), ("hidden", [over.pop("eh", cfg["eh"])])]
    args = (cfg["p"], cfg["L"], [cfg["h"]], cfg["F"], [0], cfg["L"], 1, cfg["K"], cfg["nsup"],
            reference_coeffs(cfg["K"], cfg["p"]), cfg["sigmoid"], "cEmbedder", eargs,
            "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion")
    kw = dict(num_sims=1, training_mode=MODE, num_pretrain_epochs=1, num_acclimation_epochs=1)
    kw.update(over)
    return args, kw


def hip_model(cfg, seed=0, smoothing=True, **over):
    import redcliff_amd
    args, kw = model_args(cfg, **over)
    torch.manual_seed(seed)
    cls = redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing if smoothing else redcliff_amd.REDCLIFF_S_CMLP
    return cls(*args, **kw).float().cuda()


def shape_batches(cfg):
    X, Y = synth(cfg, cfg["N"], seed=5)
    B = cfg["B"]
    return [(X[i:i + B], Y[i:i + B]) for i in range(0, X.shape[0], B)]


def run_schedule(m, bs, opts, epochs=(0, 1, 2, 2)):
    for epoch in epochs:
        for bi, (Xb, Yb) in enumerate(bs):
            m.batch_update(epoch, bi, Xb, Yb, opts[0], opts[1], 1)


# ----------------------------------------------------------------------------- 1. the new path runs
def test_fused_path_runs(fused):
    from redcliff_amd import _native as nat
    d, meta, m = golden_model()
    assert m.cembedder_fused_supported() and not m.fused_supported()
    L = nat.lib()
    assert hasattr(L, "redcliff_cemb_train_step") and L.redcliff_abi_version() == 10 == nat.ABI_VERSION
    oA, oB = adam_pair(m, meta["lrA"], meta["lrB"])
    Xb, Yb = batches(d, meta)[0]
    for epoch in sorted(set(meta["epochs"])):  # one batch_update per phase
        m.batch_update(epoch, 0, Xb, Yb, oA, oB, 1)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())  # no autograd ran
    assert m._generic()._adams == {}
    assert m.__dict__.get("_cemb_engine") is not None


# ----------------------------------------------------------------------------- 2. reference golden
def test_golden_schedule_and_validation(fused):
    d, meta, m = golden_model()
    oA, oB = adam_pair(m, meta["lrA"], meta["lrB"])
    bs = batches(d, meta)
    step = 0
    for epoch in meta["epochs"]:
        for bi, (Xb, Yb) in enumerate(bs):
            m.batch_update(epoch, bi, Xb, Yb, oA, oB, 1)
            step += 1
            golden_compare("step%d" % step, m, state(d, "step%d" % step))
    assert step == int(d["nsteps"]) == 8
    assert all(p.grad is None for p in m.parameters())
    hist = [[] for _ in range(5)] if meta["nsup"] > 0 else []
    vals = m.validate_training(bs, 1, meta["p"], *hist)
    names = ["forecast", "factor", "cos", "fw_l1", "smooth", "adj", "dag_reg", "dag_lag", "dag_node", "combo"]
    if not meta["smoothing_class"]:
        names.remove("smooth")
    seen = 0
    for n_, v in zip(names, vals):
        if ("val/" + n_) in d.files:
            assert_close("val/" + n_, v, d["val/" + n_], 1e-4, 1e-6)
            seen += 1
    assert seen >= 5


# ----------------------------------------------------------------------------- 3. oracle, edge shapes
def _vs_oracle(cfg, smoothing=True):
    from oracle.redcliff_oracle import OracleREDCLIFF, make_optimizers
    args, kw = model_args(cfg)
    torch.manual_seed(0)
    o = OracleREDCLIFF(*args, with_smoothing=smoothing, **kw)
    m = hip_model(cfg, 0, smoothing)
    assert m.cembedder_fused_supported(cfg["B"])
    bs = shape_batches(cfg)
    oA, oB = make_optimizers(o, 5e-4, 1e-4, 1e-4, 5e-4, 1e-4, 1e-4)
    hA, hB = make_optimizers(m, 5e-4, 1e-4, 1e-4, 5e-4, 1e-4, 1e-4)
    for epoch in (0, 1, 2, 2):
        for bi, (Xb, Yb) in enumerate(bs):
            o.batch_update(epoch, bi, Xb, Yb, oA, oB, 1)
            m.batch_update(epoch, bi, Xb, Yb, hA, hB, 1)
    assert all(p.grad is None for p in m.parameters())
    want = dict((k, v.detach().numpy()) for k, v in o.state_dict().items() if not k.startswith("gen_model."))
    oracle_compare("state", m, want, rtol=2e-4, atol=5e-6)
    Xv, Yv = synth(cfg, 40, seed=9)
    ov = o.validate([(Xv, Yv)])
    hv = m.validate_training([(Xv, Yv)], 1, cfg["p"], *([[] for _ in range(5)] if cfg["nsup"] > 0 else []))
    keys = ["forecast", "factor", "cos", "fw_l1", "smooth", "adj"] if smoothing else ["forecast", "factor", "cos", "fw_l1", "adj"]
    for i, k in enumerate(keys):
        assert_close("val/" + k, hv[i], ov[k], 1e-4, 1e-6)
    o.eval()
    m.eval()
    with torch.no_grad():
        go = o.GC("conditional_factor_fixed_embedder", X=Xv[:, :cfg["F"]], threshold=False, ignore_lag=False)
        gm = m.GC("conditional_factor_fixed_embedder", X=Xv[:, :cfg["F"]].cuda(), threshold=False, ignore_lag=False)
    a = np.stack([np.stack([g.numpy() for g in row]) for row in go])
    b = np.stack([np.stack([g.cpu().numpy() for g in row]) for row in gm])
    assert_close("GC", b, a, 1e-4, 1e-5)
    np.testing.assert_array_equal(b > 0, a > 0)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_three_phases_vs_oracle(name, fused):
    _vs_oracle(SHAPES[name])


def test_three_phases_vs_oracle_base_class(fused):
    """`ragged` with REDCLIFF_S_CMLP (no smoothing term in the loss or the validation tuple)."""
    _vs_oracle(SHAPES["ragged"], smoothing=False)


# ----------------------------------------------------------------------------- 4. determinism
def ragged_run():
    cfg = SHAPES["ragged"]
    m = hip_model(cfg)
    opts = adam_pair(m, 5e-4, 5e-4)
    run_schedule(m, shape_batches(cfg), opts)
    return m, opts


def test_ragged_schedule_is_deterministic(fused):
    a, b = snapshot(ragged_run()[0]), snapshot(ragged_run()[0])
    assert_same_bits(a, b, "run 1 vs run 2")


# ----------------------------------------------------------------------------- 5. path switching
@pytest.mark.parametrize("first", ["generic", "fused"])
def test_path_switch_continues_the_fit(first, monkeypatch):
    d, meta, m = golden_model()
    oA, oB = adam_pair(m, meta["lrA"], meta["lrB"])
    bs = batches(d, meta)
    other = "fused" if first == "generic" else "generic"
    step = 0
    stepped = {"A": 0, "B": 0}
    for epoch in meta["epochs"]:
        for bi, (Xb, Yb) in enumerate(bs):
            monkeypatch.setenv("REDCLIFF_CEMB_PATH", first if step < 2 else other)
            m.batch_update(epoch, bi, Xb, Yb, oA, oB, 1)
            step += 1
            if epoch < meta["pre"]:
                kinds = [g for g, key in (("A", "pretrain_embedder"), ("B", "pretrain_factor")) if key in meta["training_mode"]]
            elif "acclimate" in meta["training_mode"] and epoch < meta["pre"] + meta["acc"]:
                kinds = ["B"]
            else:
                kinds = ["A", "B"]
            for g in kinds:
                stepped[g] += 1
    assert step == 8
    golden_compare("step8", m, state(d, "step8"))
    for g, opt in (("A", oA), ("B", oB)):
        sd = opt.state_dict()
        n = len(opt.param_groups[0]["params"])
        assert sd["param_groups"][0]["params"] == list(range(n))
        assert sorted(sd["state"]) == list(range(n))
        for i, prm in enumerate(opt.param_groups[0]["params"]):
            st = sd["state"][i]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
            assert float(st["step"]) == float(stepped[g]), (g, i)
            assert st["exp_avg"].shape == prm.shape and st["exp_avg_sq"].shape == prm.shape


# ----------------------------------------------------------------------------- 6. checkpoint
def test_checkpoint_round_trip_is_bitwise(fused):
    cfg = SHAPES["sigmoid"]
    bs = shape_batches(cfg)
    m = hip_model(cfg)
    oA, oB = adam_pair(m, 5e-4, 5e-4)
    run_schedule(m, bs, (oA, oB), epochs=(0, 1, 2))
    buf = io.BytesIO()
    torch.save({"model": m, "A": oA.state_dict(), "B": oB.state_dict()}, buf)
    m.batch_update(2, 0, bs[0][0], bs[0][1], oA, oB, 1)  # the unbroken run
    want = snapshot(m)
    buf.seek(0)
    ck = torch.load(buf, map_location="cuda", weights_only=False)
    m2 = ck["model"]
    pA, pB = adam_pair(m2, 5e-4, 5e-4)
    pA.load_state_dict(ck["A"])
    pB.load_state_dict(ck["B"])
    m2.batch_update(2, 0, bs[0][0], bs[0][1], pA, pB, 1)
    assert_same_bits(snapshot(m2), want, "reloaded vs unbroken")
    for a, b in ((oA, pA), (oB, pB)):
        sa, sb = a.state_dict()["state"], b.state_dict()["state"]
        for i in sa:
            assert float(sa[i]["step"]) == float(sb[i]["step"])
            for k in ("exp_avg", "exp_avg_sq"):
                np.testing.assert_array_equal(sa[i][k].cpu().numpy(), sb[i][k].cpu().numpy())


# ----------------------------------------------------------------------------- 7. fallback
@pytest.mark.parametrize("why", ["num_sims", "eh"])
def test_outside_the_predicate_runs_generic(why, fused):
    cfg = SHAPES["sigmoid"]
    m = hip_model(cfg, num_sims=2) if why == "num_sims" else hip_model(cfg, eh=129)
    assert not m.cembedder_fused_supported(cfg["B"])
    oA, oB = adam_pair(m, 5e-4, 5e-4)
    X, Y = synth(dict(cfg, T=8), cfg["B"], seed=5)
    for epoch in (0, 1, 2):
        m.batch_update(epoch, 0, X, Y, oA, oB, 1)
    torch.cuda.synchronize()
    assert all(p.grad is not None for p in m.parameters())
    assert m.__dict__.get("_cemb_engine") is None and len(m._generic()._adams) == 2


# ----------------------------------------------------------------------------- 8. guard bands
BAND = 64
NAN_BITS = 0x7FC0BEEF


def _arm(buf, regs, total):
    iv = buf.view(torch.int32)
    assert buf.numel() >= total
    for s, n in regs:
        iv[s + n:s + n + BAND] = NAN_BITS


def _check(buf, regs, names, tag):
    iv = buf.view(torch.int32).cpu().numpy()
    for i, (s, n) in enumerate(regs):
        bad = int((iv[s + n:s + n + BAND] != NAN_BITS).sum())
        assert bad == 0, "%s: %d floats written past the end of region %s" % (tag, bad, names[i] if i < len(names) else i)


def test_guard_bands_intact_and_same_bits(fused):
    from redcliff_amd import _native as nat
    cfg = SHAPES["ragged"]
    bs = shape_batches(cfg)

    def run(guarded):
        m = hip_model(cfg)
        oA, oB = adam_pair(m, 5e-4, 5e-4)
        eng = m._cemb_fused(cfg["B"])
        d = eng.workspace(cfg["B"], cfg["T"])
        armed = None
        if guarded:
            regs, total = nat.workspace_regions(d), nat.workspace_layout(d)["total"]
            cregs, ctotal = nat.cemb_workspace_regions(d, cfg["eh"])
            assert len(cregs) == len(nat.CEMB_WS_REGIONS) and cregs[-1][0] + cregs[-1][1] + BAND <= ctotal
            _arm(eng.ws, regs, total)
            _arm(eng.cws, cregs, ctotal)
            armed = (regs, cregs)
        for bi, (Xb, Yb) in enumerate(bs):  # combined steps, full and ragged batches
            m.batch_update(2, bi, Xb, Yb, oA, oB, 1)
        vals = m.validate_training(bs, 1, cfg["p"], [], [], [], [], [])
        out = snapshot(m)
        if guarded:
            _check(eng.ws, armed[0], nat.WS_REGIONS, "shared workspace")
            _check(eng.cws, armed[1], nat.CEMB_WS_REGIONS, "cEmbedder workspace")
        for k, v in out.items():
            assert np.isfinite(v).all(), k
        return out, [float(v) for v in vals[:6]]

    plain, pv = run(False)
    prev = nat.guard_bands(BAND)
    try:
        guarded, gv = run(True)
    finally:
        nat.guard_bands(prev)
    assert_same_bits(plain, guarded, "guard bands vs production layout")
    assert pv == gv and np.isfinite(pv).all()


# ----------------------------------------------------------------------------- 9. two replicas at the ABI
def test_two_replicas_equal_two_single_calls(fused):
    from redcliff_amd import _native as nat
    cfg = SHAPES["sigmoid"]
    X, Y = synth(cfg, cfg["B"], seed=5)
    B, K = cfg["B"], cfg["K"]
    engs = []
    for seed in (0, 1):
        m = hip_model(cfg, seed)
        opts = adam_pair(m, 5e-4, 5e-4)
        eng = m._cemb_fused(B)
        eng.bind_optimizer("A", opts[0])
        eng.bind_optimizer("B", opts[1])
        engs.append((m, opts, eng))
    e0 = engs[0][2]
    staged = e0.stage(X, Y)
    Xd, lab, d = staged["X"], staged["lab"], staged["d"]
    flags = nat.LOSS_FORECAST | nat.LOSS_FACTOR | nat.LOSS_FWL1 | nat.LOSS_ADJ | nat.STEP_A | nat.STEP_B | nat.CONFUSION
    # packed copies of both fits (parameters, zero moments), stepped by one R = 2 call
    emb = torch.stack([e.emb for _, _, e in engs]).contiguous()
    fac = torch.stack([e.fac for _, _, e in engs]).contiguous()
    mom = [torch.zeros_like(emb), torch.zeros_like(emb), torch.zeros_like(fac), torch.zeros_like(fac)]
    d2 = nat.Dims(**dict((f, getattr(d, f)) for f, _ in nat.Dims._fields_))
    d2.R = 2
    L = nat.lib()
    ws = torch.zeros(L.redcliff_workspace_bytes(ctypes.byref(d2)) // 4, device="cuda")
    cws = torch.zeros(L.redcliff_cemb_workspace_bytes(ctypes.byref(d2), cfg["eh"]) // 4, device="cuda")
    assert ws.numel() > 0 and cws.numel() > 0
    conf = torch.zeros(2, cfg["nsup"] ** 2, dtype=torch.int32, device="cuda")
    a, ce = e0._args(d, flags, Xd, lab)
    a.d = d2
    a.B, a.row0 = B, 0
    a.x_rstride = a.lab_rstride = 0  # both replicas read the same batch
    a.emb, a.emb_m, a.emb_v, a.emb_stride = emb.data_ptr(), mom[0].data_ptr(), mom[1].data_ptr(), emb.shape[1]
    a.fac, a.fac_m, a.fac_v, a.fac_stride = fac.data_ptr(), mom[2].data_ptr(), mom[3].data_ptr(), fac.shape[1]
    hyper_keep = e0._hyper().repeat(2)
    a.hyper = hyper_keep.data_ptr()
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    a.confusion = conf.data_ptr()
    ce.ws, ce.ws_bytes = cws.data_ptr(), cws.numel() * 4
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nat.check(L.redcliff_cemb_train_step(ctypes.byref(a), ctypes.byref(ce), stream), "cemb_train_step R=2")
    torch.cuda.synchronize()
    for r, (m, opts, eng) in enumerate(engs):  # the same step as an R = 1 call of each fit
        eng.conf.zero_()
        eng.run_steps(["combined"], eng.stage(X, Y), opts[0], opts[1], [0], [B])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(emb[r].cpu().numpy(), eng.emb.cpu().numpy(), err_msg="replica %d embedder" % r)
        np.testing.assert_array_equal(fac[r].cpu().numpy(), eng.fac.cpu().numpy(), err_msg="replica %d factors" % r)
        np.testing.assert_array_equal(mom[0][r].cpu().numpy(), eng.opt["A"]["m"].cpu().numpy())
        np.testing.assert_array_equal(mom[1][r].cpu().numpy(), eng.opt["A"]["v"].cpu().numpy())
        np.testing.assert_array_equal(mom[2][r].cpu().numpy(), eng.opt["B"]["m"].cpu().numpy())
        np.testing.assert_array_equal(mom[3][r].cpu().numpy(), eng.opt["B"]["v"].cpu().numpy())
        np.testing.assert_array_equal(conf[r].cpu().numpy(), eng.conf.cpu().numpy())
    assert not np.array_equal(emb[0].cpu().numpy(), emb[1].cpu().numpy())


# ----------------------------------------------------------------------------- fit()'s batch loop
def test_fit_runs_its_batch_loop_on_the_fused_chain(monkeypatch):
    """fit() of a cEmbedder model goes through batch_update / validate_training (the host epoch
    loop), so REDCLIFF_CEMB_PATH=fused moves its training and validation steps onto the fused
    chain, best-model copies included.  Four epochs (pretrain, acclimate, 2 x combined) of the
    `cemb` fixture on both paths: each path is within the golden bound (rtol 1e-4, atol 1e-5 x
    scale) of the reference for this schedule, so the two agree within twice that."""
    d, meta = load("cemb")
    bs = batches(d, meta)
    out = {}
    for path in ("fused", "generic"):
        monkeypatch.setenv("REDCLIFF_CEMB_PATH", path)
        _, _, m = golden_model()
        oA, oB = adam_pair(m, meta["lrA"], meta["lrB"])
        m.fit(None, bs, oA, oB, meta["L"], 1, 1, 4, bs, lookback=1, check_every=1, verbose=0)
        out[path] = (snapshot(m), m)
    mf = out["fused"][1]
    assert mf.__dict__.get("_cemb_engine") is not None and all(p.grad is None for p in mf.parameters())
    assert out["generic"][1].__dict__.get("_cemb_engine") is None
    for k, want in out["generic"][0].items():
        scale = max(1.0, float(np.abs(want).max()))
        assert_close("fit/" + k, out["fused"][0][k], want, 2e-4, 2e-5 * scale)
