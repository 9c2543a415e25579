"""GPU tests of scoring whole recordings with many models in one launch chain
(redcliff_amd.score_recordings, ReplicaPack.score_recording, redcliff_score_recording_pack in
csrc/rc_score.hip).

Invariants are bits (torch.equal): a replica's row of the packed call against that model's own
model.score_recording.  Values: golden_io.assert_close at the project's parity bound, rtol 1e-4,
atol 1e-5, no outliers, against the CPU oracle.
"""
import pytest
import torch

from golden_io import assert_close
from test_gpu_score_recording import (MODES, SHAPES, FusedLaunches, build, oracle_graphs, oracle_scores, oracle_twin,
                                      optimizers, recording, trained)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
GOLDEN = SHAPES["golden"]
T_TILES = 84
SEEDS = (11, 12, 13)


def same(a, b, what=""):
    """Two RecordingScores (or rows of them) agree to the bit."""
    for name, x, y in zip(("w", "logits", "graphs"), a, b):
        assert (x is None) == (y is None), what + name
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y), "%s %s differs" % (what, name)


def row(res, r):
    return tuple(None if t is None else t[r] for t in res)


def golden_recordings(seed=9):
    big = recording(T_TILES, GOLDEN["p"], seed=seed, Nrec=4).cuda()
    X = big[::2]  # two recordings, non-contiguous in the recording axis
    assert not X.is_contiguous()
    return X


@pytest.fixture(scope="module")
def golden_case():
    """Three trained models of the golden shape (never packed, never modified) and two recordings."""
    return [trained(seed=s, **GOLDEN) for s in SEEDS], golden_recordings()


@pytest.fixture(scope="module")
def pack_case():
    """A ReplicaPack over three trained models of the golden shape with their optimizers, the list
    call's result on the same models taken before they were packed, and per-replica recordings."""
    from redcliff_amd import ReplicaPack, score_recordings
    models = [trained(seed=s, **GOLDEN) for s in SEEDS]
    X = golden_recordings()
    listed = score_recordings(models, X, graphs="sum")
    pack = ReplicaPack(models, [optimizers(m) for m in models])
    Xs = [golden_recordings(seed=20 + r) for r in range(3)]
    return pack, models, X, listed, Xs


# ----------------------------------------------------------------------------- 1. equal to one-by-one
@pytest.mark.parametrize("count", [1, 16, 17, 37])
def test_list_call_equals_the_models_one_by_one(golden_case, count):
    from redcliff_amd import score_recordings
    models, X = golden_case
    F, K, nsup, p = (GOLDEN[k] for k in ("F", "K", "nsup", "p"))
    for start in (F, F + 3):
        with FusedLaunches() as fl:
            res = score_recordings(models, X, start=start, count=count)
        assert fl.count == 1, "one window-kernel launch for all replicas, got %s" % fl.count
        assert res.w.shape == (3, 2, count, K) and res.logits.shape == (3, 2, count, nsup) and res.graphs is None
        for r, m in enumerate(models):
            same(row(res, r), m.score_recording(X, start=start, count=count), "replica %d: " % r)
        for mode in MODES:
            for ign in (True, False):
                kw = dict(start=start, count=count, graphs="sum", gc_est_mode=mode, ignore_lag=ign)
                with FusedLaunches() as fl:
                    res = score_recordings(models, X, **kw)
                assert fl.count == 1
                assert res.graphs.shape[:5] == (3, 2, count, p, p)
                for r, m in enumerate(models):
                    same(row(res, r), m.score_recording(X, **kw), "replica %d %s ign%d: " % (r, mode, ign))


@pytest.mark.parametrize("name,count", [("d4ic_sigmoid", 37), ("top", 20)])
def test_list_call_at_other_shapes(name, count):
    from redcliff_amd import score_recordings
    shape = SHAPES[name]
    F = shape["F"]
    models = [trained(seed=s, **shape) for s in (5, 6)]
    X = recording(F + count + 2, shape["p"], seed=7).cuda()
    for ufa in ((True, False) if name == "d4ic_sigmoid" else (True,)):
        kw = dict(start=F + 1, count=count, use_final_activation=ufa, graphs="sum")
        with FusedLaunches() as fl:
            res = score_recordings(models, X, **kw)
        assert fl.count == 1
        for r, m in enumerate(models):
            same(row(res, r), m.score_recording(X, **kw), "%s replica %d ufa %s: " % (name, r, ufa))


def test_one_model_list_equals_the_single_call(golden_case):
    from redcliff_amd import score_recordings
    models, X = golden_case
    kw = dict(start=GOLDEN["F"] + 2, count=37, graphs="sum", ignore_lag=False)
    with FusedLaunches() as fl:
        res = score_recordings(models[1:2], X, **kw)
    assert fl.count == 1 and res.w.shape[0] == 1
    same(row(res, 0), models[1].score_recording(X, **kw))


# ----------------------------------------------------------------------------- 2. pack
def test_pack_equals_the_list_call_and_the_models(pack_case):
    pack, models, X, listed, _ = pack_case
    with FusedLaunches() as fl:
        res = pack.score_recording(X, graphs="sum")
    assert fl.count == 1
    same(res, listed, "pack vs list: ")
    for r, m in enumerate(models):
        same(row(res, r), m.score_recording(X, graphs="sum"), "replica %d: " % r)
    two = pack.score_recording(X, graphs="sum", active=[0, 2])
    assert two.w.shape[0] == 2
    same(row(two, 0), row(res, 0))
    same(row(two, 1), row(res, 2))
    from redcliff_amd import _native as nat
    nat.kernel_timing(True)
    nat.kernel_times()
    none = pack.score_recording(X, graphs="sum", active=[])
    torch.cuda.synchronize()
    kt = nat.kernel_times()
    nat.kernel_timing(False)
    assert all(n == 0 for _, n in kt.values()), "an empty active list launched %s" % kt
    for t, full in zip(none, res):
        assert t.shape == (0,) + tuple(full.shape[1:])


# ----------------------------------------------------------------------------- 3. per-replica recordings
def test_per_replica_recordings(pack_case, golden_case):
    from redcliff_amd import PerReplica, score_recordings
    pack, pmodels, _, _, Xs = pack_case
    models, _ = golden_case
    kw = dict(start=GOLDEN["F"] + 1, count=37, graphs="sum")
    want = [m.score_recording(x, **kw) for m, x in zip(models, Xs)]
    for Xarg in (PerReplica(Xs), torch.stack(Xs)):
        with FusedLaunches() as fl:
            res = score_recordings(models, Xarg, **kw)
        assert fl.count == 1
        for r in range(3):
            same(row(res, r), want[r], "replica %d: " % r)
    # the pack: the same per-replica data, and an active list picks the replica's own recordings
    pwant = [m.score_recording(x, **kw) for m, x in zip(pmodels, Xs)]
    res = pack.score_recording(PerReplica(Xs), **kw)
    for r in range(3):
        same(row(res, r), pwant[r], "pack replica %d: " % r)
    for Xarg in (PerReplica(Xs), torch.stack(Xs)):
        one = pack.score_recording(Xarg, active=[1], **kw)
        assert one.w.shape[0] == 1
        same(row(one, 0), pwant[1], "active=[1]: ")
    with pytest.raises(ValueError):
        score_recordings(models, PerReplica([Xs[0], Xs[1], Xs[2][:, :-1]]), **kw)
    with pytest.raises(ValueError):
        score_recordings(models, PerReplica(Xs[:2]), **kw)
    with pytest.raises(ValueError):
        pack.score_recording(torch.stack(Xs[:2]), **kw)


# ----------------------------------------------------------------------------- 4. strides and splits
def test_strides_repeats_and_splits_to_the_bit(golden_case):
    from redcliff_amd import score_recordings
    models, X = golden_case
    F = GOLDEN["F"]
    a, b, mid = F + 2, F + 2 + 50, F + 2 + 21  # 21 is no multiple of 16
    kw = dict(graphs="sum", ignore_lag=False)
    full = score_recordings(models, X, start=a, count=b - a, **kw)
    again = score_recordings(models, X, start=a, count=b - a, **kw)
    same(full, again, "two calls: ")
    lo = score_recordings(models, X, start=a, count=mid - a, **kw)
    hi = score_recordings(models, X, start=mid, count=b - mid, **kw)
    for x, l, h in zip(full, lo, hi):
        assert torch.equal(x, torch.cat([l, h], 2)), "[a, b) != [a, m) + [m, b)"
    s4 = score_recordings(models, X, start=a, count=9, stride=4, **kw)
    for x, y in zip(full, s4):
        assert y.shape[2] == 9 and torch.equal(x[:, :, 0:33:4], y), "stride 4 differs from every fourth step of stride 1"


# ----------------------------------------------------------------------------- 5. bounds
def test_nothing_read_or_written_out_of_bounds(golden_case):
    from redcliff_amd import scoring
    models, X2 = golden_case
    F, p, K, nsup = (GOLDEN[k] for k in ("F", "p", "K", "nsup"))
    R, T, count, start = 3, 40, 34, F  # the last window ends at T, the first starts at row 0
    rec = X2[0, :T].contiguous()
    with torch.no_grad():
        tab, bias = scoring._list_graph_tables(models, MODES[1], True)
    plain = scoring.fused_score_pack(models, rec.unsqueeze(0), False, start, count, 1, True, tab, bias)
    pad = 4096
    xbuf = torch.full((2 * pad + T * p,), float("nan"), device="cuda")
    xbuf[pad:pad + T * p] = rec.reshape(-1)
    Xg = xbuf[pad:pad + T * p].view(1, T, p)
    sizes = (R * count * K, R * count * nsup, R * count * p * p)
    bufs = [torch.full((2 * pad + n,), float("nan"), device="cuda") for n in sizes]
    outs = (bufs[0][pad:pad + sizes[0]].view(R, 1, count, K), bufs[1][pad:pad + sizes[1]].view(R, 1, count, nsup),
            bufs[2][pad:pad + sizes[2]].view(R, 1, count, p, p, 1))
    got = scoring.fused_score_pack(models, Xg, False, start, count, 1, True, tab, bias, out=outs)
    torch.cuda.synchronize()
    for g, want, buf, n in zip(got, plain, bufs, sizes):
        assert bool(torch.isfinite(g).all())
        assert torch.equal(g, want)
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all()), "padding written"
    assert bool(torch.isnan(xbuf[:pad]).all()) and bool(torch.isnan(xbuf[pad + T * p:]).all())
    # per-replica recordings inside one guarded buffer: replica 2's last window ends at the buffer's last row
    xbuf = torch.full((2 * pad + R * T * p,), float("nan"), device="cuda")
    Xr = xbuf[pad:pad + R * T * p].view(R, 1, T, p)
    for r in range(R):
        Xr[r, 0] = X2[r % 2, r:r + T]
    plain = scoring.fused_score_pack(models, Xr.clone(), True, start, count, 1, True, tab, bias)
    bufs = [torch.full((2 * pad + n,), float("nan"), device="cuda") for n in sizes]
    outs = (bufs[0][pad:pad + sizes[0]].view(R, 1, count, K), bufs[1][pad:pad + sizes[1]].view(R, 1, count, nsup),
            bufs[2][pad:pad + sizes[2]].view(R, 1, count, p, p, 1))
    got = scoring.fused_score_pack(models, Xr, True, start, count, 1, True, tab, bias, out=outs)
    torch.cuda.synchronize()
    for g, want, buf, n in zip(got, plain, bufs, sizes):
        assert bool(torch.isfinite(g).all()) and torch.equal(g, want)
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all()), "padding written"


# ----------------------------------------------------------------------------- 6. oracle
def test_pack_scores_and_graphs_match_the_oracle():
    from redcliff_amd import score_recordings
    shape = SHAPES["tst"]
    F, p = shape["F"], shape["p"]
    count, start = 37, F + 1
    models = [trained(seed=s, **shape) for s in (3, 8)]
    X = recording(F + count + 2, p)
    rows = slice(start - F, start - F + count)
    res = score_recordings(models, X, start=start, count=count)
    gr = dict((ign, score_recordings(models, X, start=start, count=count, graphs="sum", gc_est_mode=MODES[1],
                                     ignore_lag=ign)) for ign in (True, False))
    for r, m in enumerate(models):
        o = oracle_twin(m, **shape)
        ow, ol = oracle_scores(o, X, F)
        assert_close("tst/%d/w" % r, res.w[r, 0].cpu().numpy(), ow[rows], RTOL, ATOL)
        assert_close("tst/%d/logits" % r, res.logits[r, 0].cpu().numpy(), ol[rows], RTOL, ATOL)
        for ign in (True, False):
            og = oracle_graphs(o, X, F, MODES[1], ign)
            assert_close("tst/%d/graphs/ign%d" % (r, ign), gr[ign].graphs[r, 0].cpu().numpy(), og[rows], RTOL, ATOL)


# ----------------------------------------------------------------------------- 7. non-interference
def test_scoring_between_two_epochs_leaves_the_pack_bit_identical():
    from redcliff_amd import ReplicaPack
    from test_gpu_replicas import CFG, GRID, data, make, opts
    train = data(64 * 2 + 24, seed=3)
    rec = recording(60, CFG["p"], seed=12, Nrec=2)
    states = []
    for interleave in (False, True):
        models = [make(s, fc, adj) for s, fc, adj, _, _ in GRID]
        pack = ReplicaPack(models, [opts(m, lrB, lrA) for m, (_, _, _, lrB, lrA) in zip(models, GRID)])
        ds = pack.cache_dataset(train)
        pack.run_epoch(0, ds)
        if interleave:
            flags = [m.factor_score_embedder.training for m in models]
            fresh = [e.supports_fresh for e in pack.engines]
            steps = [pack._step_counts(r) for r in range(pack.R)]
            res = pack.score_recording(rec, graphs="sum")
            assert res.w.shape[:2] == (3, 2) and bool(torch.isfinite(res.graphs).all())
            assert [m.factor_score_embedder.training for m in models] == flags
            assert [e.supports_fresh for e in pack.engines] == fresh
            assert [pack._step_counts(r) for r in range(pack.R)] == steps
        pack.run_epoch(1, ds)
        torch.cuda.synchronize()
        states.append(dict((n, t.detach().clone()) for n, t, _ in pack._state_tensors()))
    assert set(states[0]) == set(states[1])
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k


# ----------------------------------------------------------------------------- 8. loop route
def test_loop_route_for_models_outside_the_packed_kernel():
    from redcliff_amd import score_recordings
    shape = dict(GOLDEN, num_sims=2)  # outside fused_supported(): the chunked route, model by model
    models = [build(s, **shape) for s in (2, 3)]
    F = shape["F"]
    X = recording(50, shape["p"], seed=4).cuda()
    kw = dict(start=F, count=30, graphs="sum")
    with FusedLaunches() as fl:
        res = score_recordings(models, X, **kw)
    assert fl.count == 0
    assert res.w.shape[0] == 2
    for r, m in enumerate(models):
        same(row(res, r), m.score_recording(X, **kw), "replica %d: " % r)
    other = build(4, **dict(GOLDEN, K=2))
    with pytest.raises(ValueError):
        score_recordings([models[0], other], X, **kw)
    with pytest.raises(ValueError):
        score_recordings([], X)
