"""GPU tests of recording scoring (model.score_recording, redcliff_amd.scoring, csrc/rc_score.hip,
the drop-in functions of redcliff_amd.evaluation) against the CPU oracle and the reference
fixture tests/golden/recording_scores.npz.

Values: golden_io.assert_close at rtol 1e-4, atol 1e-5, no outliers (the project's parity bound; a
forward pass has no discontinuity in its values).  Invariants: torch.equal (bits).
"""
import copy

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_score_recording_host import load_scenario

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
MODES = ("conditional_factor_exclusive", "conditional_factor_fixed_embedder")


# ----------------------------------------------------------------------------- helpers
def ctor(p, F, L, n, H, K, nsup, sigmoid, h=6, num_sims=1):
    from oracle.redcliff_oracle import reference_coeffs
    eargs = [("num_features_per_node", F), ("num_graph_conv_layers", n), ("num_hidden_nodes", H),
             ("sigmoid_eccentricity_coeff", 10.0)]
    args = (p, L, [h], F, [0], L, 1, K, nsup, reference_coeffs(K, p), sigmoid, "DGCNN", eargs,
            "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion")
    return args, dict(num_sims=num_sims, training_mode="combined")


def build(seed=0, **shape):
    import redcliff_amd
    args, kw = ctor(**shape)
    torch.manual_seed(seed)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(*args, **kw).float().cuda()


def optimizers(model):
    from oracle.redcliff_oracle import make_optimizers
    return make_optimizers(model, 5e-3, 1e-4, 1e-4, 5e-3, 1e-4, 1e-4)


def train_batch(model, seed=1, B=8):
    rng = np.random.RandomState(seed)
    K, p, T = model.num_factors_nK, model.num_series, model.Lmax + 2
    X = torch.from_numpy(rng.randn(B, T, p).astype(np.float32))
    Y = torch.zeros(B, K, T)
    Y[torch.arange(B), torch.from_numpy(rng.randint(0, K, B)), :] = 1.0
    return X, Y


def trained(seed=0, **shape):
    """A GPU model after two combined batch_updates: A, the weights and the BatchNorm running
    statistics are off their initial values."""
    m = build(seed, **shape)
    oA, oB = optimizers(m)
    X, Y = train_batch(m)
    for i in range(2):
        m.batch_update(0, i, X, Y, oA, oB, 1)
    return m


def oracle_twin(m, **shape):
    from oracle.redcliff_oracle import OracleREDCLIFF
    args, kw = ctor(**shape)
    o = OracleREDCLIFF(*args, **kw)
    o.load_state_dict(dict((k, v.detach().cpu()) for k, v in m.state_dict().items()))
    o.eval()
    return o


def recording(T, p, seed=5, Nrec=None):
    rng = np.random.RandomState(seed)
    X = rng.randn(*((T, p) if Nrec is None else (Nrec, T, p))).astype(np.float32)
    for t in range(2, T):
        X[..., t, :] += 0.3 * X[..., t - 1, :] - 0.1 * X[..., t - 2, :]
    return torch.from_numpy(X)


def oracle_scores(o, X, F, use_final_activation=True):
    """Oracle (w, logits) of every window of one recording X (T, p): row i = window [i, i + F),
    scored step `start + j*stride` is row start + j*stride - F.  Time-major windows at any p."""
    win = X.unfold(0, F, 1).contiguous()  # (T - F + 1, p, F): nodes x features
    with torch.no_grad():
        w, lg = o.factor_score_embedder(win, use_final_activation)
    return w.numpy(), None if lg is None else lg.numpy()


def oracle_graphs(o, X, F, mode, ignore_lag):
    win = X.unfold(0, F, 1).transpose(1, 2).contiguous()  # (N, F, p) time-major
    with torch.no_grad():
        gc = o.GC(mode, X=win, threshold=False, ignore_lag=ignore_lag)
    return np.stack([sum(g).numpy() for g in gc])


class FusedLaunches:
    """Counts redcliff_score_recording's window-kernel launches (redcliff_kernel_times)."""

    def __enter__(self):
        from redcliff_amd import _native as nat
        nat.kernel_timing(True)
        nat.kernel_times()
        self.count = None
        return self

    def __exit__(self, *exc):
        from redcliff_amd import _native as nat
        torch.cuda.synchronize()
        self.count = nat.kernel_times()["score"][1]
        nat.kernel_timing(False)


# ----------------------------------------------------------------------------- oracle comparison
SHAPES = {
    "k1_identity": dict(p=3, F=4, L=2, n=1, H=5, K=1, nsup=0, sigmoid=False),   # identity support only, no class scores
    "golden": dict(p=5, F=7, L=3, n=3, H=5, K=3, nsup=2, sigmoid=False),
    "d4ic_sigmoid": dict(p=10, F=16, L=5, n=3, H=100, K=4, nsup=4, sigmoid=True),
    "tst": dict(p=12, F=16, L=4, n=3, H=100, K=9, nsup=3, sigmoid=False),
    "p_eq_F": dict(p=7, F=7, L=3, n=2, H=6, K=2, nsup=1, sigmoid=False),        # time-major semantics at p == F
    "top": dict(p=64, F=64, L=2, n=3, H=100, K=8, nsup=2, sigmoid=False, h=4),  # top of the limits
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_scores_and_graphs_match_oracle(name):
    shape = SHAPES[name]
    F, p, K, nsup = shape["F"], shape["p"], shape["K"], shape["nsup"]
    m = trained(seed=3, **shape)
    o = oracle_twin(m, **shape)
    count = 20 if name == "top" else 37
    T = F + count + 2
    X = recording(T, p)
    start = F + 1
    rows = slice(start - F, start - F + count)
    finals = (True, False) if name == "d4ic_sigmoid" else (True,)
    seen = []
    for ufa in finals:
        ow, ol = oracle_scores(o, X, F, ufa)
        with FusedLaunches() as fl:
            res = m.score_recording(X, start=start, count=count, use_final_activation=ufa)
        assert fl.count == 1, "the fused kernel did not run"
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
            res = m.score_recording(X, start=start, count=count, graphs="sum", gc_est_mode=mode, ignore_lag=ign)
            Lp = 1 if ign else (shape["L"] if mode == MODES[0] else min(shape["L"], F))
            assert res.graphs.shape == (1, count, p, p, Lp)
            assert_close("%s/graphs/%s/ign%d" % (name, mode, ign), res.graphs[0].cpu().numpy(), og[rows], RTOL, ATOL)
    # the default mode is the model's primary one, and one entry is the sum over model.GC's list
    assert m.factor_score_embedder.training  # as batch_update left it: score_recording is inference all the same
    res = m.score_recording(X, start=start, count=3, graphs="sum")
    win = X[start - F:start].unsqueeze(0).cuda()
    m.factor_score_embedder.eval()
    with torch.no_grad():
        own = sum(m.GC(m.primary_gc_est_mode, X=win, threshold=False, ignore_lag=True)[0])
    assert_close(name + "/graphs/own", res.graphs[0, 0].cpu().numpy(), own.detach().cpu().numpy(), RTOL, ATOL)


# ----------------------------------------------------------------------------- tiles (golden shape)
GOLDEN_SHAPE = SHAPES["golden"]
T_TILES = 84


@pytest.fixture(scope="module")
def tile_case():
    """One trained model of the golden shape, three recordings inside a larger tensor, and the
    oracle's scores of every window (computed once, never modified)."""
    m = trained(seed=4, **GOLDEN_SHAPE)
    o = oracle_twin(m, **GOLDEN_SHAPE)
    big = recording(T_TILES, GOLDEN_SHAPE["p"], seed=9, Nrec=6).cuda()
    X3 = big[::2]  # non-contiguous in the recording axis
    assert not X3.is_contiguous()
    ref = [oracle_scores(o, X3[r].cpu(), GOLDEN_SHAPE["F"]) for r in range(3)]
    for w, lg in ref:
        w.setflags(write=False)
        lg.setflags(write=False)
    return m, X3, ref


def check_against(ref, res, start, count, stride, F, tag):
    Nrec = res.w.shape[0]
    rows = start - F + stride * np.arange(count)
    for r in range(Nrec):
        assert_close(tag + "/w", res.w[r].cpu().numpy(), ref[r][0][rows], RTOL, ATOL)
        assert_close(tag + "/logits", res.logits[r].cpu().numpy(), ref[r][1][rows], RTOL, ATOL)


@pytest.mark.parametrize("count", [1, 15, 16, 17, 31, 32, 33, 65])
def test_tile_boundaries(tile_case, count):
    m, X3, ref = tile_case
    F = GOLDEN_SHAPE["F"]
    for start in (F, F + 3):
        for X in (X3[:1], X3):
            res = m.score_recording(X, start=start, count=count)
            assert res.w.shape == (X.shape[0], count, GOLDEN_SHAPE["K"])
            check_against(ref, res, start, count, 1, F, "count%d/start%d/nrec%d" % (count, start, X.shape[0]))


def test_stride_and_last_window_at_T(tile_case):
    m, X3, ref = tile_case
    F = GOLDEN_SHAPE["F"]
    res = m.score_recording(X3, start=F + 3, count=9, stride=4)
    check_against(ref, res, F + 3, 9, 4, F, "stride4")
    # the last window ends exactly at T
    res = m.score_recording(X3, start=T_TILES - 16, count=17)
    check_against(ref, res, T_TILES - 16, 17, 1, F, "ends_at_T")
    with pytest.raises(ValueError):
        m.score_recording(X3, start=T_TILES - 16, count=18)
    # the defaults: start = F and every step that fits
    res = m.score_recording(X3[1])
    assert res.w.shape == (1, T_TILES - F + 1, GOLDEN_SHAPE["K"])
    check_against(ref[1:2], res, F, T_TILES - F + 1, 1, F, "defaults")
    # a 2-D recording that is a strided view (rows not contiguous) is accepted as well
    wide = torch.zeros(T_TILES, 2 * GOLDEN_SHAPE["p"], device="cuda")
    wide[:, ::2] = X3[2]
    res = m.score_recording(wide[:, ::2], start=F, count=20)
    check_against(ref[2:3], res, F, 20, 1, F, "strided_rows")
    assert m.score_recording(X3, start=F, count=0).w.shape == (3, 0, GOLDEN_SHAPE["K"])


def test_invariants_to_the_bit(tile_case):
    m, X3, _ = tile_case
    F = GOLDEN_SHAPE["F"]
    a, b, mid = F + 2, F + 2 + 50, F + 2 + 21  # 21 is no multiple of 16
    kw = dict(graphs="sum", ignore_lag=False)
    full = m.score_recording(X3, start=a, count=b - a, **kw)
    again = m.score_recording(X3, start=a, count=b - a, **kw)
    for x, y in zip(full, again):
        assert torch.equal(x, y), "two calls differ"
    lo = m.score_recording(X3, start=a, count=mid - a, **kw)
    hi = m.score_recording(X3, start=mid, count=b - mid, **kw)
    for x, l, h in zip(full, lo, hi):
        assert torch.equal(x, torch.cat([l, h], 1)), "[a, b) != [a, m) + [m, b)"
    for r in range(3):
        one = m.score_recording(X3[r], start=a, count=b - a, **kw)
        for x, y in zip(full, one):
            assert torch.equal(x[r:r + 1], y), "Nrec = 3 differs from three calls with Nrec = 1"
    s4 = m.score_recording(X3, start=a, count=13, stride=4, **kw)
    for x, y in zip(full, s4):
        assert torch.equal(x[:, 0:49:4], y), "stride 4 differs from every fourth step of stride 1"
    far = m.score_recording(X3, start=a, count=2, stride=48, **kw)
    for x, y in zip(full, far):
        assert torch.equal(x[:, 0:49:48], y)
    # a stride so large that a tile's span of rows holds fewer than 16 steps (14 at this shape)
    long = recording(3100, GOLDEN_SHAPE["p"], seed=21).cuda()
    dense = m.score_recording(long, start=F, count=2851)
    sparse = m.score_recording(long, start=F, count=16, stride=190)
    assert torch.equal(dense.w[:, ::190], sparse.w) and torch.equal(dense.logits[:, ::190], sparse.logits)


def test_nothing_read_or_written_out_of_bounds(tile_case):
    from redcliff_amd import scoring
    m, X3, _ = tile_case
    F, p, K, nsup = (GOLDEN_SHAPE[k] for k in ("F", "p", "K", "nsup"))
    T, count, start = 40, 34, F  # the last window ends at T, the first starts at row 0
    rec = X3[0, :T].contiguous()
    tab, bias = scoring.graph_tables(m, MODES[1], True)
    plain = scoring.fused_score(m, rec.unsqueeze(0), start, count, 1, True, tab, bias)
    pad = 4096
    xbuf = torch.full((2 * pad + T * p,), float("nan"), device="cuda")
    xbuf[pad:pad + T * p] = rec.reshape(-1)
    Xg = xbuf[pad:pad + T * p].view(1, T, p)
    sizes = (count * K, count * nsup, count * p * p)
    bufs = [torch.full((2 * pad + n,), float("nan"), device="cuda") for n in sizes]
    outs = (bufs[0][pad:pad + sizes[0]].view(1, count, K), bufs[1][pad:pad + sizes[1]].view(1, count, nsup),
            bufs[2][pad:pad + sizes[2]].view(1, count, p, p, 1))
    got = scoring.fused_score(m, Xg, start, count, 1, True, tab, bias, out=outs)
    torch.cuda.synchronize()
    for g, want, buf, n in zip(got, plain, bufs, sizes):
        assert bool(torch.isfinite(g).all())
        assert torch.equal(g, want)
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all()), "padding written"
    assert bool(torch.isnan(xbuf[:pad]).all()) and bool(torch.isnan(xbuf[pad + T * p:]).all())


# ----------------------------------------------------------------------------- non-interference
def snapshot(m, opts):
    st = dict((k, v.detach().clone()) for k, v in m.state_dict().items())
    for g, o in zip("AB", opts):
        for i, prm in enumerate(o.param_groups[0]["params"]):
            for k, v in o.state[prm].items():
                st["opt%s/%d/%s" % (g, i, k)] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    return st


def test_scoring_in_the_middle_of_a_fit_leaves_it_bit_identical():
    shape = GOLDEN_SHAPE
    rec = recording(40, shape["p"], seed=12, Nrec=2)
    snaps = []
    for interleave in (False, True):
        m = build(7, **shape)
        opts = optimizers(m)
        X, Y = train_batch(m)
        for i in range(5):
            m.batch_update(0, i, X, Y, opts[0], opts[1], 1)
            if interleave:
                m.score_recording(rec, graphs="sum" if i % 2 else None)
                assert m.factor_score_embedder.training  # no module state changed
        torch.cuda.synchronize()
        snaps.append(snapshot(m, opts))
    assert set(snaps[0]) == set(snaps[1])
    for k in snaps[0]:
        assert torch.equal(snaps[0][k], snaps[1][k]), k


# ----------------------------------------------------------------------------- drop-ins
def golden_model(name):
    meta, st, rec, wts, cls = load_scenario(name)
    shape = dict((k, meta[k]) for k in ("p", "F", "L", "n", "H", "K", "nsup", "sigmoid", "h"))
    m = build(meta["seed"], **shape)
    m.factor_score_embedder.load_state_dict(dict((k, v.cuda()) for k, v in st.items()))
    m.eval()
    return m, meta, torch.from_numpy(rec), wts, cls


def drop_in_args(meta):
    return meta["num_supervised_factors"], meta["num_timesteps_to_score"], meta["num_timesteps_in_input_history"]


@pytest.mark.parametrize("name", ["a", "b"])
def test_drop_ins_reproduce_the_reference_through_the_fused_kernel(name):
    from redcliff_amd import evaluation as ev
    m, meta, rec, wts, cls = golden_model(name)
    with FusedLaunches() as fl:
        got_w = ev.obtain_factor_score_weightings_across_recording(m, rec, *drop_in_args(meta))
        got_c = ev.obtain_factor_score_classifications_across_recording(m, rec, *drop_in_args(meta))
    assert fl.count == 2, "the drop-ins did not go through the fused kernel"
    assert got_w.dtype == got_c.dtype == np.float64 and got_w.shape == wts.shape
    assert_close(name + "/weightings", got_w, wts, RTOL, ATOL)
    assert_close(name + "/classifications", got_c, cls, RTOL, ATOL)


def test_drop_ins_keep_the_loop_at_p_equal_F():
    from redcliff_amd import evaluation as ev
    m, meta, rec, wts, cls = golden_model("c")
    with FusedLaunches() as fl:
        got_w = ev.obtain_factor_score_weightings_across_recording(m, rec, *drop_in_args(meta))
        got_c = ev.obtain_factor_score_classifications_across_recording(m, rec, *drop_in_args(meta))
    assert fl.count == 0
    assert_close("c/weightings", got_w, wts, RTOL, ATOL)
    assert_close("c/classifications", got_c, cls, RTOL, ATOL)


def test_drop_ins_keep_the_loop_in_training_mode():
    from redcliff_amd import evaluation as ev
    m, meta, rec, wts, _ = golden_model("a")
    m.factor_score_embedder.train()
    bn = m.factor_score_embedder.dgcnn.dgcnn.BN1
    before = int(bn.num_batches_tracked)
    nsup, steps, hist = drop_in_args(meta)
    steps = 5
    with FusedLaunches() as fl:
        got = ev.obtain_factor_score_weightings_across_recording(m, rec, nsup, steps, hist)
    assert fl.count == 0 and got.shape == (nsup, steps)
    assert int(bn.num_batches_tracked) == before + steps  # one train-mode embedder call per step, as the reference
    assert np.abs(got - wts[:, :steps]).max() > 1e-6  # batch statistics, not the running ones


# ----------------------------------------------------------------------------- fallback
def unfolded(X, F, start, count):
    return X.unfold(0, F, 1)[start - F:start - F + count]  # (count, p, F)


def test_chunked_route_for_models_outside_the_fused_kernel():
    from test_cemb_host import cpu_model
    F, count = 4, 30
    cm = cpu_model().cuda()  # cEmbedder: p = 6, F = 4
    X = recording(40, 6, seed=3).cuda()
    with FusedLaunches() as fl:
        res = cm.score_recording(X, start=F + 1, count=count)
    assert fl.count == 0
    cm.factor_score_embedder.eval()
    with torch.no_grad():
        w, lg = cm.factor_score_embedder(unfolded(X, F, F + 1, count).transpose(1, 2).contiguous())
    assert torch.equal(res.w[0], w) and torch.equal(res.logits[0], lg) and res.graphs is None
    # DGCNN with two simulation steps: outside fused_supported()
    shape = dict(GOLDEN_SHAPE, num_sims=2)
    dm = build(2, **shape)
    F = shape["F"]
    X = recording(50, shape["p"], seed=4).cuda()
    assert dm.factor_score_embedder.training
    with FusedLaunches() as fl:
        res = dm.score_recording(X, start=F, count=count, stride=1, graphs="sum")
    assert fl.count == 0 and dm.factor_score_embedder.training  # mode restored
    dm.factor_score_embedder.eval()
    win = unfolded(X, F, F, count).contiguous()
    with torch.no_grad():
        w, lg = dm.factor_score_embedder(win)
        gc = dm.GC(dm.primary_gc_est_mode, X=win.transpose(1, 2).contiguous(), threshold=False, ignore_lag=True)
    assert torch.equal(res.w[0], w) and torch.equal(res.logits[0], lg)
    assert torch.equal(res.graphs[0], torch.stack([sum(g) for g in gc]))
