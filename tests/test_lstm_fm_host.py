"""CPU-side checks of the cLSTM forecasting baseline (redcliff_amd.clstm_fm, csrc/rc_lstm_fm.hip):
seeded construction and the generic route on the CPU against the reference fixture
tests/golden/clstm_fm.npz, the packed layout, the limit predicate against
redcliff_lstm_fm_supported, the argument and limit checks of redcliff_lstm_fm_run, the kernel's
resource metadata and the route switch.  No kernel is launched."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, assert_close
from test_kernel_occupancy import _kernels

STATE_RTOL, STATE_ATOL = 2e-4, 5e-6  # the project's state bound (compare_state)
RTOL, ATOL = 1e-4, 1e-6              # running sums, validation terms and fit histories
KERNEL_IDS = ("supports", "emb_fwd", "fac_fwd", "fac_bwd", "emb_bwd", "emb_final", "fac_mix", "emb_combine", "fac_lead",
              "score", "score_graphs", "score_cemb")
PKL_KEYS = {"epoch", "avg_forecasting_loss", "avg_adj_penalty", "avg_dagness_loss", "avg_smooth_loss", "best_loss"}

# ------------------------------------------------------------------------------------------ fixture
_FIXTURE = {}


def load_lf(name):
    """(meta, {key: array}) of one scenario of clstm_fm.npz (read once, never modified)."""
    if not _FIXTURE:
        d = np.load(os.path.join(GOLDEN, "clstm_fm.npz"), allow_pickle=False)
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
    return {"FORECAST_COEFF": meta["forecast"], "ADJ_L1_REG_COEFF": meta["adj"], "DAGNESS_REG_COEFF": 0.0}


def batches(X, B):
    X = torch.from_numpy(np.array(X))
    return [(X[i:i + B], None) for i in range(0, X.shape[0], B)]


def build_model(meta, device="cpu"):
    import redcliff_amd
    torch.manual_seed(meta["seed"])
    return redcliff_amd.cLSTM_FM(meta["p"], meta["h"], None, meta["C"], coeffs(meta)).to(device)


def fac_state(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items() if k.startswith("factors."))


def compare_state_dict(tag, got, want, rtol=STATE_RTOL, atol=STATE_ATOL):
    """compare_state's bound on {key: array} dicts."""
    assert set(got) == set(want), tag
    for k in want:
        scale = max(1.0, float(np.abs(want[k]).max()))
        assert_close("%s/%s" % (tag, k), got[k], want[k], rtol, atol * scale)


def check_scenario(name, device, nan_past_tmax=False):
    """Per-epoch states, running sums and both validation tuples of a scenario, on whichever route
    the environment and `device` select."""
    meta, sc = load_lf(name)
    assert sc["X_train"].shape == (meta["N"], meta["T"], meta["p"])
    m = build_model(meta, device)
    Xtr, Xva = np.array(sc["X_train"]), np.array(sc["X_val"])
    if nan_past_tmax:
        assert meta["T"] > meta["Tm"]
        Xtr[:, meta["Tm"]:], Xva[:, meta["Tm"]:] = np.nan, np.nan
    tr, va = batches(Xtr, meta["B"]), batches(Xva, meta["B"])
    assert tr[-1][0].shape[0] == (meta["N"] % meta["B"] or meta["B"])
    opt = torch.optim.Adam(m.gen_model.parameters(), **meta["adam"])
    for e in range(1, meta["epochs"] + 1):
        run = (0., 0., 0., 0.)
        for bn, (X, _) in enumerate(tr):
            run = m.batch_update(bn, X, meta["Tm"], meta["C"], opt, *run)
        compare_state_dict("%s/epoch%d" % (name, e), fac_state(m), sub(sc, "epoch%d" % e))
        assert_close("%s/sums%d" % (name, e), run, sc["sums"][e - 1], RTOL, ATOL)
    raw = m.training_sim_eval(va, meta["Tm"], meta["C"], meta["p"], return_loss_componentwise=True)
    nrm = m.training_sim_eval(va, meta["Tm"], meta["C"], meta["p"], return_loss_componentwise=True,
                              report_normalized_loss_components=True)
    assert_close(name + "/val_raw", raw, sc["val_raw"], RTOL, ATOL)
    assert_close(name + "/val_norm", nrm, sc["val_norm"], RTOL, ATOL)
    assert m.training_sim_eval(va, meta["Tm"], meta["C"], meta["p"]) == raw[4]
    return m


def check_whole_fit(device, tmp):
    """Scenario a's whole fit: pickle entries, stop epoch, final state and returned loss."""
    meta, sc = load_lf("a")
    fit = meta["fit"]
    m = build_model(meta, device)
    opt = torch.optim.Adam(m.gen_model.parameters(), **dict(meta["adam"], lr=fit["lr"]))
    final = m.fit(tmp, batches(sc["X_train"], meta["B"]), opt, meta["C"], meta["Tm"], 1, fit["max_iter"],
                  lookback=fit["lookback"], check_every=fit["check_every"], verbose=0, GC=None,
                  X_val=batches(sc["X_val"], meta["B"]))
    with open(os.path.join(tmp, "training_meta_data_and_hyper_parameters.pkl"), "rb") as f:
        got = pickle.load(f)
    assert set(got) == PKL_KEYS == set(sub(sc, "fit/pkl"))
    for k in PKL_KEYS:
        assert_close("fit/pkl/" + k, got[k], sc["fit/pkl/" + k], RTOL, ATOL)
    stop = int(sc["fit/stop_epoch"])
    assert 0 < stop < fit["max_iter"] - 1  # the fixture holds the stop path
    assert m.fit_history["stop_epoch"] == stop and len(m.fit_history["avg_smooth_loss"]) == stop + 1
    assert m.fit_history["best_it"] == stop - fit["lookback"] * fit["check_every"]
    compare_state_dict("fit/final", fac_state(m), sub(sc, "fit/final"))
    assert_close("fit/final_loss", final, sc["fit/final_loss"], RTOL, ATOL)
    assert os.path.exists(os.path.join(tmp, "final_best_model.bin"))
    assert os.path.exists(os.path.join(tmp, "temp_best_model_epoch%d.bin" % int(got["epoch"])))
    return m


# ------------------------------------------------------------------------------------------ model / layout
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_seeded_construction_is_the_reference_init(name):
    meta, sc = load_lf(name)
    m = build_model(meta)
    sd = m.state_dict()
    want = sub(sc, "init")
    assert set(k for k in sd if k.startswith("factors.")) == set(want)
    assert set(k for k in sd if not k.startswith("factors.")) == set("gen_model.1." + k[len("factors."):] for k in want)
    assert set(k.split(".", 4)[4] for k in want) == {"lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0",
                                                       "lstm.bias_hh_l0", "linear.weight", "linear.bias"}
    for k, v in want.items():
        assert np.array_equal(sd[k].numpy(), v), k
    assert m.factor_score_embedder is None and m.gen_model[0] is None and m.gen_model[1] is m.factors
    assert m.num_factors_nK == 1 and m.num_series == meta["p"] and m.factors[0].wavelet_mask is None
    opt = torch.optim.Adam(m.gen_model.parameters(), lr=1e-3, eps=1e-4, weight_decay=1e-4)
    assert len(opt.param_groups[0]["params"]) == 6 * meta["p"]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_generic_route_on_the_cpu_reproduces_the_fixture(name, monkeypatch):
    monkeypatch.delenv("REDCLIFF_LSTM_FM_PATH", raising=False)
    check_scenario(name, "cpu")


def test_generic_route_on_the_cpu_reproduces_the_whole_fit(tmp_path, monkeypatch):
    monkeypatch.delenv("REDCLIFF_LSTM_FM_PATH", raising=False)
    check_whole_fit("cpu", str(tmp_path))


def test_fit_needs_a_validation_loader(tmp_path):
    meta, sc = load_lf("a")
    m = build_model(meta)
    opt = torch.optim.Adam(m.gen_model.parameters(), **meta["adam"])
    with pytest.raises(ValueError):
        m.fit(str(tmp_path), batches(sc["X_train"], meta["B"]), opt, meta["C"], meta["Tm"], 1, 2)


def test_gc_wavelets_and_prox():
    import redcliff_amd
    torch.manual_seed(3)
    f = redcliff_amd.cLSTM(2, 3, wavelet_level=3)
    assert f.num_series == 8 and len(f.networks) == 8 and f.wavelet_mask.shape == (8, 8)
    mask = f.wavelet_mask.cpu()
    assert float(mask[0, 0]) == pytest.approx(1.3 ** 4) and float(mask[5, 2]) == pytest.approx(1.3 ** (0 - 2))
    G = f.GC(threshold=False).cpu()
    want = torch.stack([torch.norm(n.lstm.weight_ih_l0, dim=0) for n in f.networks]).detach().cpu()
    assert torch.equal(G.detach(), want)
    assert torch.allclose(f.GC(threshold=False, rank_wavelets=True).detach().cpu(), mask * want)
    comb = f.GC(threshold=False, combine_wavelet_representations=True).detach().cpu()
    assert comb.shape == (2, 2) and float(comb[1, 0]) == pytest.approx(float(want[3:6, 0:3].sum()), rel=1e-6)
    assert f.GC().dtype == torch.int32
    pred, hidden = f(torch.randn(5, 4, 8, device=f.networks[0].lstm.weight_ih_l0.device))
    assert pred.shape == (5, 4, 8) and len(hidden) == 8 and hidden[0][0].shape == (1, 5, 3)
    f.perform_prox_update_on_GC_weights(1e3, 1.0)  # every column norm is below lam * lr
    assert float(f.GC(threshold=False).detach().abs().max()) == 0.0 and int(f.GC().sum()) == 0


def test_packed_layout_is_the_parameter_order():
    import redcliff_amd
    from redcliff_amd import kernels
    p, h = 7, 13
    torch.manual_seed(1)
    m = redcliff_amd.cLSTM_FM(p, h, None, 2, coeffs(dict(forecast=1., adj=1.)))
    o = kernels.lstm_layout(p, h)
    g = 4 * h
    assert (o["Wih"], o["Whh"], o["bih"], o["bhh"], o["Wl"], o["bl"], o["total"]) == (
        0, p * g * p, p * g * (p + h), p * g * (p + h + 1), p * g * (p + h + 2), p * g * (p + h + 2) + p * h,
        p * (g * (p + h + 2) + h + 1))
    flat = torch.arange(o["total"], dtype=torch.float32)
    pairs = kernels.lstm_views(flat, m.factors[0], p, h)
    params = list(m.gen_model.parameters())
    assert len(pairs) == len(params) == 6 * p and all(a is b for (a, _), b in zip(pairs, params))
    seen = torch.zeros(o["total"])
    for j in range(p):
        Wih, Whh, bih, bhh, Wl, bl = [v for _, v in pairs[6 * j:6 * j + 6]]
        for (prm, v) in pairs[6 * j:6 * j + 6]:
            assert prm.shape == v.shape and v.is_contiguous()
            seen[v.reshape(-1).long()] += 1
        assert float(Wih[2, 3]) == o["Wih"] + j * g * p + 2 * p + 3
        assert float(Whh[2, 3]) == o["Whh"] + j * g * h + 2 * h + 3
        assert float(bih[5]) == o["bih"] + j * g + 5 and float(bhh[5]) == o["bhh"] + j * g + 5
        assert float(Wl[0, 4, 0]) == o["Wl"] + j * h + 4 and float(bl[0]) == o["bl"] + j
    assert bool((seen == 1).all())  # every float of the block belongs to exactly one parameter


# ------------------------------------------------------------------------------------------ C entries
def lf_args(d, **kw):
    """Arguments with dummy non-null pointers: every case below must be rejected (or return 0 for an
    empty call) before anything is dereferenced or launched."""
    from redcliff_amd import _native as nat
    a = nat.LstmFMArgs()
    a.d = d
    a.context, a.tmax = 2, 4
    a.flags = nat.LOSS_FORECAST | nat.LOSS_ADJ | nat.STEP_B | nat.VALUES
    a.B, a.tB, a.row0, a.N = 8, 1, 0, 20
    for f in ("X", "fac", "fac_m", "fac_v", "hyper", "sse", "pen"):
        setattr(a, f, 64)
    a.x_pstride, a.fac_stride = 0, 10000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_predicate_agrees_with_the_library_over_a_grid():
    from redcliff_amd import clstm_fm as F
    n_yes = n_no = 0
    for p in (1, 4, 10, 12, 33, 64, 65):
        for h in (1, 5, 13, 25, 44, 64, 65):
            for C in (1, 2, 5, 27, 64, 65):
                for Bmax, R in ((128, 1), (512, 256), (513, 1), (8, 257)):
                    want = F.lstm_fm_shape_supported(p, h, C, Bmax, None, R)
                    got = F.lstm_fm_supported(p, h, C, Bmax, None, R)
                    assert (got > 0) == want, (p, h, C, Bmax, R, got)
                    if got:
                        assert got == F.lstm_fm_lds_floats(p, h, C)
                    n_yes, n_no = n_yes + bool(want), n_no + (not want)
    assert n_yes > 50 and n_no > 50
    # the footprint, spelled out at the D4IC shape: K = 35, np = 100*35 + 226
    assert F.lstm_fm_lds_floats(10, 25, 2) == 4 * 3726 + 32 * (105 + 201 + 51 + 50 + 4) + 10 + 16
    # both sides of the LDS limit in h, C and p
    edges = [(p, h, C) for p, C in ((4, 2), (10, 2), (12, 2), (7, 5)) for h in range(1, 64)
             if F.lstm_fm_lds_floats(p, h, C) <= F.LDS_MAX_FLOATS < F.lstm_fm_lds_floats(p, h + 1, C)]
    assert len(edges) == 4
    for p, h, C in edges:
        assert F.lstm_fm_supported(p, h, C) == F.lstm_fm_lds_floats(p, h, C) and F.lstm_fm_supported(p, h + 1, C) == 0
    edges = [(p, h, C) for p, h in ((4, 5), (10, 25)) for C in range(1, 64)
             if F.lstm_fm_lds_floats(p, h, C) <= F.LDS_MAX_FLOATS < F.lstm_fm_lds_floats(p, h, C + 1)]
    assert len(edges) == 2
    for p, h, C in edges:
        assert F.lstm_fm_supported(p, h, C) > 0 and F.lstm_fm_supported(p, h, C + 1) == 0
    # the explicit caps bind where the footprint does not
    assert F.lstm_fm_supported(64, 4, 2) > 0 and F.lstm_fm_supported(65, 4, 2) == 0
    assert F.lstm_fm_lds_floats(65, 4, 2) <= F.LDS_MAX_FLOATS
    assert F.lstm_fm_supported(1, 1, 64) > 0 and F.lstm_fm_supported(1, 1, 65) == 0
    assert F.lstm_fm_lds_floats(1, 1, 65) <= F.LDS_MAX_FLOATS
    # the published baseline shapes and the fixture's fit
    for p, h, C in ((10, 25, 2), (12, 25, 2), (4, 5, 2), (7, 13, 5)):
        assert F.lstm_fm_supported(p, h, C, 128) > 0


def test_lstm_fm_run_argument_and_limit_checks():
    from redcliff_amd import _native as nat
    from redcliff_amd.clstm_fm import lstm_fm_dims
    L = nat.lib()
    call = lambda a: L.redcliff_lstm_fm_run(ctypes.byref(a), None)
    good = lambda: lstm_fm_dims(10, 25, Bmax=128, T=6, R=3)
    EINVAL, ELIMIT = -1, -2
    assert L.redcliff_lstm_fm_run(None, None) == EINVAL
    # limits
    for d, kw in ((lstm_fm_dims(65, 4, 8, 6), {}), (lstm_fm_dims(10, 65, 8, 6), {}), (lstm_fm_dims(10, 25, 513, 6), {}),
                  (lstm_fm_dims(10, 25, 8, 6, R=257), {}), (lstm_fm_dims(10, 60, 8, 6), {}),
                  (lstm_fm_dims(1, 1, 8, 80), dict(context=65, tmax=70)),
                  (lstm_fm_dims(10, 25, 8, 40), dict(context=30, tmax=35))):
        assert call(lf_args(d, **kw)) == ELIMIT
        assert b"limits" in L.redcliff_last_error()
        assert L.redcliff_lstm_fm_supported(ctypes.byref(d), kw.get("context", 2)) == 0
    assert L.redcliff_lstm_fm_supported(None, 2) == 0
    for bad in (dict(p=0), dict(h=0), dict(R=0), dict(Bmax=0), dict(T=0)):
        d = good()
        for k, v in bad.items():
            setattr(d, k, v)
        assert call(lf_args(d)) == EINVAL
    # arguments
    for kw in (dict(X=None), dict(fac=None), dict(fac_m=None), dict(fac_v=None), dict(hyper=None), dict(sse=None),
               dict(pen=None), dict(B=0), dict(B=129), dict(N=-1), dict(row0=-1), dict(tB=0), dict(x_pstride=-1),
               dict(fac_stride=-1), dict(flags=nat.LOSS_FACTOR), dict(flags=nat.STEP_A | nat.STEP_B),
               dict(flags=nat.GRAD_ONLY | nat.VALUES), dict(context=0), dict(context=-1), dict(tmax=2), dict(tmax=1),
               dict(tmax=7), dict(context=4, tmax=4)):
        assert call(lf_args(good(), **kw)) == EINVAL, kw
    # pen may be null without RC_VALUES, the moments without RC_STEP_B -- then only the empty call returns 0
    assert call(lf_args(good(), pen=None, flags=nat.LOSS_FORECAST | nat.STEP_B, N=0)) == 0
    assert call(lf_args(good(), fac_m=None, fac_v=None, flags=nat.LOSS_FORECAST | nat.VALUES, N=0)) == 0
    # the active list: strictly increasing indices < R, at most R entries
    for lst in ([0, 0], [1, 0], [0, 3], [-1], [0, 1, 2, 2]):
        arr = (ctypes.c_int32 * len(lst))(*lst)
        a = lf_args(good(), replicas=ctypes.cast(arr, ctypes.c_void_p), n_replicas=len(lst))
        assert call(a) == EINVAL, lst
        assert b"replica" in L.redcliff_last_error()
    arr = (ctypes.c_int32 * 2)(0, 2)
    assert call(lf_args(good(), replicas=ctypes.cast(arr, ctypes.c_void_p), n_replicas=-1)) == EINVAL
    # nothing to do: no launch, no error (the dummy pointers are never touched)
    assert call(lf_args(good(), N=0)) == 0
    assert call(lf_args(good(), replicas=ctypes.cast(arr, ctypes.c_void_p), n_replicas=0)) == 0


def test_lstm_fm_kernel_uses_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    mine = [k for k in ks if "k_lstm_fm_epoch" in k]
    assert len(mine) == 1, sorted(ks)
    assert ks[mine[0]]["scratch"] == 0


def test_abi_version_and_kernel_ids_are_unchanged():
    from redcliff_amd import _native as nat
    assert nat.ABI_VERSION == 10 and nat.lib().redcliff_abi_version() == 10
    assert nat.KERNEL_IDS == KERNEL_IDS
    assert "redcliff_lstm_fm_run" in nat.EXPORTED and "redcliff_lstm_fm_supported" in nat.EXPORTED
    assert ctypes.sizeof(nat.LstmFMArgs) == ctypes.sizeof(nat.Dims) + 4 * 2 + 4 * 3 + 4 + 8 * 2 + 8 * 2 + 8 * 4 + 8 + 8 * 3 + 8 + 8


def test_route_switch(monkeypatch):
    import redcliff_amd
    from redcliff_amd import clstm_fm as F
    monkeypatch.delenv("REDCLIFF_LSTM_FM_PATH", raising=False)
    assert F.lstm_fm_path() == "fused"
    for v, want in (("fused", "fused"), ("generic", "generic"), ("", "fused")):
        monkeypatch.setenv("REDCLIFF_LSTM_FM_PATH", v)
        assert F.lstm_fm_path() == want
    monkeypatch.setenv("REDCLIFF_LSTM_FM_PATH", "eager")
    with pytest.raises(ValueError):
        F.lstm_fm_path()
    # a model on the CPU, with wavelets or roll-outs is never on the fused route
    monkeypatch.setenv("REDCLIFF_LSTM_FM_PATH", "fused")
    c = coeffs(dict(forecast=1., adj=1.))
    m = redcliff_amd.cLSTM_FM(4, 5, None, 2, c)
    assert not m.fused_eligible(2, 4)  # parameters on the CPU
    assert redcliff_amd.fit_lstm_baselines is F.fit_lstm_baselines
    assert redcliff_amd.cLSTM is F.cLSTM and redcliff_amd.LSTM is not None
