"""GPU tests of recording scoring for cEmbedder models (model.score_recording under
REDCLIFF_CEMB_PATH=fused, redcliff_amd.scoring, csrc/rc_score_cemb.hip, the drop-in functions of
redcliff_amd.evaluation) against the CPU oracle (OracleREDCLIFF / OCEmbedder) and the reference
fixture tests/golden/cemb_recording_scores.npz.

Values: golden_io.assert_close at rtol 1e-4, atol 1e-5, no outliers (the project's parity bound).
Invariants: torch.equal (bits).  Models are built by seeded construction plus a seeded perturbation
of every embedder parameter; only the fit test trains.
"""
import ctypes

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_gpu_score_recording import recording, snapshot
from test_score_cemb_host import load_cemb_scenario

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
MODES = ("conditional_factor_exclusive", "conditional_factor_fixed_embedder")
ENV = "REDCLIFF_CEMB_PATH"


@pytest.fixture
def fused(monkeypatch):
    monkeypatch.setenv(ENV, "fused")


# ----------------------------------------------------------------------------- helpers
def ctor(p, F, eh, K, nsup, sigmoid=False, L=3, h=6, num_sims=1, hidden=None):
    from oracle.redcliff_oracle import reference_coeffs
    eargs = [("sigmoid_eccentricity_coeff", 10.0), ("lag", F), ("hidden", list(hidden) if hidden else [eh])]
    args = (p, L, [h], F, [0], L, 1, K, nsup, reference_coeffs(K, p), sigmoid, "cEmbedder", eargs,
            "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion")
    return args, dict(num_sims=num_sims, training_mode="combined")


def build(seed=0, **shape):
    """Seeded construction, then every embedder parameter moved off its initial value by a seeded
    perturbation of half its own mean magnitude.  Relative, not absolute: the initialisation scales
    with the fan-in, so the scores stay O(1) at every shape (an absolute 0.1 at p F = 4096 gives raw
    scores near 7, and a graph entry, a sum of K = 16 signed terms w_k g_k that cancel, then carries
    fp32 rounding of its terms above the bound's atol of 1e-5 in the oracle itself: at the top shape
    the fp32 oracle is 1.09 x the bound away from its fp64 twin on the graphs with an absolute 0.1,
    0.07 x with this perturbation)."""
    import redcliff_amd
    args, kw = ctor(**shape)
    torch.manual_seed(seed)
    m = redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(*args, **kw).float()
    rng = np.random.RandomState(seed + 1000)
    with torch.no_grad():
        for prm in m.factor_score_embedder.parameters():
            scale = 0.5 * float(prm.abs().mean())
            prm.add_(torch.from_numpy((scale * rng.randn(*prm.shape)).astype(np.float32)))
    return m.cuda()


def oracle_twin(m, **shape):
    from oracle.redcliff_oracle import OracleREDCLIFF
    args, kw = ctor(**shape)
    o = OracleREDCLIFF(*args, **kw)
    o.load_state_dict(dict((k, v.detach().cpu()) for k, v in m.state_dict().items()))
    o.eval()
    return o


def windows(X, F, rows=None):
    """Time-major windows (N, F, p) of one recording X (T, p): row i = rows [i, i + F)."""
    win = X.unfold(0, F, 1)
    if rows is not None:
        win = win[torch.as_tensor(rows)]
    return win.transpose(1, 2).contiguous()


def oracle_scores(o, X, F, use_final_activation=True, rows=None):
    with torch.no_grad():
        w, lg = o.factor_score_embedder(windows(X, F, rows), use_final_activation)
    return w.numpy(), None if lg is None else lg.numpy()


def oracle_graphs(o, X, F, mode, ignore_lag):
    with torch.no_grad():
        gc = o.GC(mode, X=windows(X, F), threshold=False, ignore_lag=ignore_lag)
    return np.stack([sum(g).numpy() for g in gc])


class Launches:
    """Launch counts of the scoring kernels (redcliff_kernel_times) inside the block."""

    def __enter__(self):
        from redcliff_amd import _native as nat
        nat.kernel_timing(True)
        nat.kernel_times()
        self.cemb = self.dgcnn = self.graphs = None
        return self

    def __exit__(self, *exc):
        from redcliff_amd import _native as nat
        torch.cuda.synchronize()
        kt = nat.kernel_times()
        self.cemb, self.dgcnn, self.graphs = kt["score_cemb"][1], kt["score"][1], kt["score_graphs"][1]
        nat.kernel_timing(False)


def rows_budget(m):
    from redcliff_amd import _native as nat
    from redcliff_amd import scoring
    d = scoring._cemb_dims(m)
    return nat.lib().redcliff_cemb_score_supported(ctypes.byref(d), int(m.factor_score_embedder.hidden[0]))


# ----------------------------------------------------------------------------- oracle comparison
SHAPES = {
    "k1": dict(p=3, F=4, eh=5, K=1, nsup=0, L=2),
    "golden": dict(p=5, F=7, eh=6, K=3, nsup=2),                       # p F = 35 is no multiple of 4; eh < 16
    "c1_sigmoid": dict(p=10, F=16, eh=25, K=4, nsup=4, sigmoid=True, L=5, h=25),
    "unit_blocks": dict(p=6, F=4, eh=33, K=2, nsup=1),                 # a third unit block of one unit
    "p_eq_F": dict(p=7, F=7, eh=6, K=2, nsup=1),                       # time-major at p == F as everywhere
    "top": dict(p=64, F=64, eh=128, K=16, nsup=2, L=2, h=4),           # top of the limits
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_scores_and_graphs_match_oracle(fused, name):
    shape = SHAPES[name]
    F, p, K, nsup, L = shape["F"], shape["p"], shape["K"], shape["nsup"], shape.get("L", 3)
    m = build(seed=3, **shape)
    o = oracle_twin(m, **shape)
    count = 20 if name == "top" else 37
    T = F + count + 2
    X = recording(T, p)
    start = F + 1
    rows = slice(start - F, start - F + count)
    finals = (True, False) if name == "c1_sigmoid" else (True,)
    seen = []
    for ufa in finals:
        ow, ol = oracle_scores(o, X, F, ufa)
        with Launches() as ln:
            res = m.score_recording(X, start=start, count=count, use_final_activation=ufa)
        assert ln.cemb == 1 and ln.dgcnn == 0, "the cEmbedder kernel did not run"
        assert res.w.shape == (1, count, K) and res.graphs is None
        assert_close(name + "/w", res.w[0].cpu().numpy(), ow[rows], RTOL, ATOL)
        if nsup == 0:
            assert res.logits is None
        else:
            assert res.logits.shape == (1, count, nsup)
            assert_close(name + "/logits", res.logits[0].cpu().numpy(), ol[rows], RTOL, ATOL)
            seen.append(res)
    if len(seen) == 2:  # without the final activation the class scores are the raw outputs; w is unchanged
        assert torch.equal(seen[0].w, seen[1].w)
        assert_close(name + "/raw", torch.sigmoid(seen[1].logits).cpu().numpy(), seen[0].logits.cpu().numpy(), RTOL, ATOL)
        assert float((seen[0].logits - seen[1].logits).abs().max()) > 1e-3
    for mode in MODES:
        for ign in (True, False):
            og = oracle_graphs(o, X, F, mode, ign)
            with Launches() as ln:
                res = m.score_recording(X, start=start, count=count, graphs="sum", gc_est_mode=mode, ignore_lag=ign)
            assert ln.cemb == 1 and ln.dgcnn == 0 and ln.graphs == 1
            Lp = 1 if ign else (L if mode == MODES[0] else min(L, F))
            assert res.graphs.shape == (1, count, p, p, Lp)
            assert_close("%s/graphs/%s/ign%d" % (name, mode, ign), res.graphs[0].cpu().numpy(), og[rows], RTOL, ATOL)
    # the default mode is the model's primary one, and one entry is the sum over model.GC's list
    res = m.score_recording(X, start=start, count=3, graphs="sum")
    win = X[start - F:start].unsqueeze(0).cuda()
    with torch.no_grad():
        own = sum(m.GC(m.primary_gc_est_mode, X=win, threshold=False, ignore_lag=True)[0])
    assert_close(name + "/graphs/own", res.graphs[0, 0].cpu().numpy(), own.detach().cpu().numpy(), RTOL, ATOL)


# ----------------------------------------------------------------------------- tiles (golden shape)
GOLDEN_SHAPE = SHAPES["golden"]
T_TILES = 150


@pytest.fixture(scope="module")
def tile_case():
    """One model of the golden shape, three recordings inside a larger tensor (a non-contiguous
    view), the oracle's scores of every window and one long fused call (computed once, never
    modified)."""
    import os
    m = build(seed=4, **GOLDEN_SHAPE)
    o = oracle_twin(m, **GOLDEN_SHAPE)
    F = GOLDEN_SHAPE["F"]
    big = recording(T_TILES, GOLDEN_SHAPE["p"], seed=9, Nrec=6).cuda()
    X3 = big[::2]
    assert not X3.is_contiguous()
    ref = [oracle_scores(o, X3[r].cpu(), F) for r in range(3)]
    for w, lg in ref:
        w.setflags(write=False)
        lg.setflags(write=False)
    old = os.environ.get(ENV)
    os.environ[ENV] = "fused"
    try:
        with Launches() as ln:
            full = m.score_recording(X3, start=F, count=T_TILES - F + 1, graphs="sum", ignore_lag=False)
    finally:
        if old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = old
    assert ln.cemb == 1
    return m, o, X3, ref, full


def check_against(ref, res, start, count, stride, F, tag):
    rows = start - F + stride * np.arange(count)
    for r in range(res.w.shape[0]):
        assert_close(tag + "/w", res.w[r].cpu().numpy(), ref[r][0][rows], RTOL, ATOL)
        assert_close(tag + "/logits", res.logits[r].cpu().numpy(), ref[r][1][rows], RTOL, ATOL)


@pytest.mark.parametrize("count", [1, 15, 16, 17, 63, 64, 65, 129])
def test_tile_boundaries(fused, tile_case, count):
    m, _, X3, ref, full = tile_case
    F, K = GOLDEN_SHAPE["F"], GOLDEN_SHAPE["K"]
    for start in (F, F + 3):
        for X in (X3[:1], X3):
            n = X.shape[0]
            res = m.score_recording(X, start=start, count=count)
            assert res.w.shape == (n, count, K)
            sl = slice(start - F, start - F + count)
            assert torch.equal(res.w, full.w[:n, sl]) and torch.equal(res.logits, full.logits[:n, sl])
            check_against(ref, res, start, count, 1, F, "count%d/start%d/nrec%d" % (count, start, n))


def test_stride_and_last_window_at_T(fused, tile_case):
    m, _, X3, ref, full = tile_case
    F = GOLDEN_SHAPE["F"]
    start, count = F + 2, 48
    assert start + (count - 1) * 3 == T_TILES  # the last window ends exactly at T
    res = m.score_recording(X3, start=start, count=count, stride=3)
    check_against(ref, res, start, count, 3, F, "stride3")
    assert torch.equal(res.w, full.w[:, 2::3][:, :count])
    with pytest.raises(ValueError):
        m.score_recording(X3, start=start, count=count + 1, stride=3)
    # the defaults: start = F and every step that fits
    res = m.score_recording(X3[1])
    assert res.w.shape == (1, T_TILES - F + 1, GOLDEN_SHAPE["K"]) and torch.equal(res.w, full.w[1:2])
    # a 2-D recording that is a strided view (rows not contiguous) is accepted as well
    wide = torch.zeros(T_TILES, 2 * GOLDEN_SHAPE["p"], device="cuda")
    wide[:, ::2] = X3[2]
    res = m.score_recording(wide[:, ::2], start=F, count=20)
    assert torch.equal(res.w, full.w[2:3, :20])
    assert m.score_recording(X3, start=F, count=0).w.shape == (3, 0, GOLDEN_SHAPE["K"])


def test_strides_that_shrink_the_tile(fused, tile_case):
    """Strides derived from the library's row budget: one leaves a tile fewer steps than a full
    one (64), one leaves a single step per tile.  Both equal the dense call to the bit."""
    m, o, _, _, _ = tile_case
    F, p = GOLDEN_SHAPE["F"], GOLDEN_SHAPE["p"]
    budget = rows_budget(m)
    assert budget >= F + 63
    steps_per_tile = lambda stride: 64 if 63 * stride + F <= budget else (budget - F) // stride + 1
    some = (budget - F) // 40 + 1          # about 40 steps per tile
    one = budget - F + 1
    assert 1 < steps_per_tile(some) < 64 and steps_per_tile(one) == 1 and steps_per_tile(one - 1) == 2
    T = F + 2 * one + 1
    assert T * p * 4 < 1 << 20
    long = recording(T, p, seed=21)
    dense = m.score_recording(long.cuda(), start=F)
    for stride, count in ((some, steps_per_tile(some) + 5), (one, 3), (one - 1, 3)):
        with Launches() as ln:
            sparse = m.score_recording(long.cuda(), start=F, count=count, stride=stride)
        assert ln.cemb == 1
        sl = slice(0, (count - 1) * stride + 1, stride)
        assert torch.equal(dense.w[:, sl], sparse.w) and torch.equal(dense.logits[:, sl], sparse.logits)
        ow, ol = oracle_scores(o, long, F, rows=stride * np.arange(count))
        assert_close("stride%d/w" % stride, sparse.w[0].cpu().numpy(), ow, RTOL, ATOL)
        assert_close("stride%d/logits" % stride, sparse.logits[0].cpu().numpy(), ol, RTOL, ATOL)


def test_invariants_to_the_bit(fused, tile_case):
    m, _, X3, _, full = tile_case
    F = GOLDEN_SHAPE["F"]
    a, b, mid = F + 2, F + 2 + 100, F + 2 + 37  # 37 is no multiple of 16
    kw = dict(graphs="sum", ignore_lag=False)
    span = m.score_recording(X3, start=a, count=b - a, **kw)
    again = m.score_recording(X3, start=a, count=b - a, **kw)
    for x, y, f in zip(span, again, full):
        assert torch.equal(x, y), "two calls differ"
        assert torch.equal(x, f[:, 2:2 + b - a])
    lo = m.score_recording(X3, start=a, count=mid - a, **kw)
    hi = m.score_recording(X3, start=mid, count=b - mid, **kw)
    for x, l, h in zip(span, lo, hi):
        assert torch.equal(x, torch.cat([l, h], 1)), "[a, b) != [a, m) + [m, b)"
    for r in range(3):
        one = m.score_recording(X3[r], start=a, count=b - a, **kw)
        for x, y in zip(span, one):
            assert torch.equal(x[r:r + 1], y), "Nrec = 3 differs from three calls with Nrec = 1"
    s4 = m.score_recording(X3, start=a, count=25, stride=4, **kw)
    for x, y in zip(span, s4):
        assert torch.equal(x[:, 0:97:4], y), "stride 4 differs from every fourth step of stride 1"


def test_nothing_read_or_written_out_of_bounds(fused, tile_case):
    from redcliff_amd import scoring
    m, _, X3, _, _ = tile_case
    F, p, K, nsup = (GOLDEN_SHAPE[k] for k in ("F", "p", "K", "nsup"))
    T, count, start = 90, 84, F  # the first window starts at row 0, the last ends at T; two tiles
    rec = X3[0, :T].contiguous()
    tab, bias = scoring.graph_tables(m, MODES[1], True)
    plain = scoring.cemb_fused_score(m, rec.unsqueeze(0), start, count, 1, True, tab, bias)
    pad = 4096
    # NaN rows directly before and after the scored span
    xbuf = torch.full((2 * pad + T * p,), float("nan"), device="cuda")
    xbuf[pad:pad + T * p] = rec.reshape(-1)
    Xg = xbuf[pad:pad + T * p].view(1, T, p)
    sizes = (count * K, count * nsup, count * p * p)
    bufs = [torch.full((2 * pad + n,), float("nan"), device="cuda") for n in sizes]
    outs = (bufs[0][pad:pad + sizes[0]].view(1, count, K), bufs[1][pad:pad + sizes[1]].view(1, count, nsup),
            bufs[2][pad:pad + sizes[2]].view(1, count, p, p, 1))
    got = scoring.cemb_fused_score(m, Xg, start, count, 1, True, tab, bias, out=outs)
    torch.cuda.synchronize()
    for g, want, buf, n in zip(got, plain, bufs, sizes):
        assert bool(torch.isfinite(g).all())
        assert torch.equal(g, want)
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all()), "padding written"
    assert bool(torch.isnan(xbuf[:pad]).all()) and bool(torch.isnan(xbuf[pad + T * p:]).all())
    # a span strictly inside the recording, NaN in the rows next to it
    inner = rec.clone()
    first, cnt = 10, 20
    end = first + F + (cnt - 1) * 3  # start = first + F, stride 3: the call reads rows [first, end)
    assert end < T
    inner[first - 1] = float("nan")
    inner[end] = float("nan")
    res = m.score_recording(inner, start=first + F, count=cnt, stride=3)
    assert bool(torch.isfinite(res.w).all()) and bool(torch.isfinite(res.logits).all())
    want = m.score_recording(rec, start=first + F, count=cnt, stride=3)
    assert torch.equal(res.w, want.w)


# ----------------------------------------------------------------------------- non-interference
@pytest.mark.parametrize("train_path", ["fused", "generic"])
def test_scoring_in_the_middle_of_a_fit_leaves_it_bit_identical(monkeypatch, train_path):
    """Train, score, train == a twin that never scored: state dict, both optimizers' state, step
    counts.  On the generic training path the variable is switched to fused around the scoring
    call only."""
    from test_gpu_cemb_fused import SHAPES as FIT_SHAPES
    from test_gpu_cemb_fused import adam_pair, hip_model, shape_batches
    cfg = FIT_SHAPES["sigmoid"]
    rec = recording(40, cfg["p"], seed=12, Nrec=2)
    bs = shape_batches(cfg)[:2]
    snaps = []
    for interleave in (False, True):
        monkeypatch.setenv(ENV, train_path)
        m = hip_model(cfg, seed=7, training_mode="combined", num_pretrain_epochs=0, num_acclimation_epochs=0)
        opts = adam_pair(m, 1e-3, 1e-3)
        launched = 0
        for i in range(2):
            for bi, (Xb, Yb) in enumerate(bs):
                m.batch_update(0, bi, Xb, Yb, opts[0], opts[1], 1)
            if interleave:
                monkeypatch.setenv(ENV, "fused")
                with Launches() as ln:
                    m.score_recording(rec, graphs="sum" if i % 2 else None)
                monkeypatch.setenv(ENV, train_path)
                launched += ln.cemb
        assert launched == (2 if interleave else 0)
        torch.cuda.synchronize()
        snaps.append(snapshot(m, opts))
        if train_path == "fused":
            assert m.__dict__.get("_cemb_engine") is not None
    assert set(snaps[0]) == set(snaps[1])
    for k in snaps[0]:
        assert torch.equal(snaps[0][k], snaps[1][k]), k


# ----------------------------------------------------------------------------- routing
def test_routing(monkeypatch):
    from redcliff_amd import scoring
    F, count = GOLDEN_SHAPE["F"], 30
    X = recording(50, GOLDEN_SHAPE["p"], seed=3).cuda()
    m = build(seed=5, **GOLDEN_SHAPE)
    chunked = scoring._chunked_score(m, X.unsqueeze(0), F + 1, count, 1, True, MODES[1], True)
    for value in (None, "generic"):
        if value is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, value)
        with Launches() as ln:
            res = m.score_recording(X, start=F + 1, count=count, graphs="sum")
        assert ln.cemb == 0 and ln.dgcnn == 0
        for x, y in zip(res, chunked):
            assert torch.equal(x, y), "the default route changed"
    monkeypatch.setenv(ENV, "fused")
    assert scoring.cemb_fused_available(m)
    with Launches() as ln:
        res = m.score_recording(X, start=F + 1, count=count, graphs="sum")
    assert ln.cemb == 1
    for name, x, y in zip(("w", "logits", "graphs"), res, chunked):
        assert_close("fused_vs_chunked/" + name, x.cpu().numpy(), y.cpu().numpy(), RTOL, ATOL)
    # only the embedder matters: two simulation steps are outside cembedder_fused_supported()
    two = build(seed=6, **dict(GOLDEN_SHAPE, num_sims=2))
    assert not two.cembedder_fused_supported() and scoring.cemb_fused_available(two)
    with Launches() as ln:
        res = two.score_recording(X, start=F + 1, count=count)
    assert ln.cemb == 1
    want = scoring._chunked_score(two, X.unsqueeze(0), F + 1, count, 1, True, None, True)
    assert_close("num_sims2/w", res.w.cpu().numpy(), want[0].cpu().numpy(), RTOL, ATOL)
    # two hidden layers in the embedder: the chunked route, under fused as well
    deep = build(seed=7, **dict(GOLDEN_SHAPE, hidden=(6, 4)))
    assert not scoring.cemb_fused_available(deep)
    with Launches() as ln:
        res = deep.score_recording(X, start=F + 1, count=count)
    assert ln.cemb == 0
    want = scoring._chunked_score(deep, X.unsqueeze(0), F + 1, count, 1, True, None, True)
    assert torch.equal(res.w, want[0]) and torch.equal(res.logits, want[1])


# ----------------------------------------------------------------------------- drop-ins
@pytest.mark.parametrize("name", ["a", "b"])
def test_drop_ins_reproduce_the_reference_through_the_fused_kernel(fused, name):
    import redcliff_amd
    from redcliff_amd import evaluation as ev
    meta, st, rec, wts, cls = load_cemb_scenario(name)
    args, kw = ctor(**dict((k, meta[k]) for k in ("p", "F", "eh", "K", "nsup", "sigmoid", "L", "h")))
    torch.manual_seed(meta["seed"])
    m = redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(*args, **kw).float().cuda()
    m.factor_score_embedder.load_state_dict(dict((k, v.cuda()) for k, v in st.items()))
    m.eval()
    rec = torch.from_numpy(rec)
    dargs = (meta["num_supervised_factors"], meta["num_timesteps_to_score"], meta["num_timesteps_in_input_history"])
    with Launches() as ln:
        got_w = ev.obtain_factor_score_weightings_across_recording(m, rec, *dargs)
    assert ln.cemb == 1, "the drop-in did not go through the cEmbedder kernel"
    with Launches() as ln:
        got_c = ev.obtain_factor_score_classifications_across_recording(m, rec, *dargs)
    assert ln.cemb == 1, "the drop-in did not go through the cEmbedder kernel"
    assert got_w.dtype == got_c.dtype == np.float64 and got_w.shape == wts.shape
    assert_close(name + "/weightings", got_w, wts, RTOL, ATOL)
    assert_close(name + "/classifications", got_c, cls, RTOL, ATOL)
