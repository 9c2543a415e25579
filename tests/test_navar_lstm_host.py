"""CPU-side checks of the NAVAR (LSTM) baseline (redcliff_amd.navar_lstm, csrc/rc_navar_lstm.hip) against
the reference fixture tests/golden/navar_lstm.npz: seeded construction, the generic route step by step,
the reference's RNG consumption, whole fits and the saved model, forward's shapes and row order, the
val_proportion > 0 form, the restated limit function against redcliff_navar_lstm_supported, the argument
checks of redcliff_navar_lstm_run, the kernels' resource metadata and the route switch.  No kernel is
launched."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, assert_close
from test_kernel_occupancy import _kernels

STATE_RTOL, STATE_ATOL = 2e-4, 5e-6  # the project's state bound (tests/test_fm_host.py)
RTOL, ATOL = 1e-4, 1e-6              # loss values and the causal matrix

_FIXTURE = {}


def load_nl(name):
    """(meta, {key: array}) of one scenario of navar_lstm.npz (read once, never modified)."""
    if not _FIXTURE:
        d = np.load(os.path.join(GOLDEN, "navar_lstm.npz"), allow_pickle=False)
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


def compare_state_dict(tag, got, want, rtol=STATE_RTOL, atol=STATE_ATOL, whh_stride=None):
    """The state bound; the fixture keeps scenario w's weight_hh_l0 as every whh_stride-th element."""
    assert set(got) == set(want), tag
    for k in want:
        g = got[k]
        if whh_stride and k.endswith("weight_hh_l0"):
            g = g.reshape(-1)[::whh_stride]
        scale = max(1.0, float(np.abs(want[k]).max()))
        assert_close("%s/%s" % (tag, k), g, want[k], rtol, atol * scale)


def state_of(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


def build(meta, device="cpu"):
    from redcliff_amd import NAVARLSTM
    torch.manual_seed(meta["seed"])
    return NAVARLSTM(meta["N"], meta["H"], meta["Tp"], hidden_layers=1, dropout=0).to(device)


class ReplayRNG:
    """Hands out the fixture's permutations in order (and fails on an unexpected draw)."""

    def __init__(self, perms):
        self.perms, self.at = list(perms), 0

    def choice(self, n, size=None, replace=True):
        assert size == n and replace is False and self.at < len(self.perms), "unexpected RNG draw"
        self.at += 1
        return np.array(self.perms[self.at - 1])


def perms_of(meta, sc):
    return [sc["perm%d" % e] for e in range(1, meta["epochs"] + 1) if "perm%d" % e in sc]


def fit_epochs(m, meta, sc, tmp, epochs, rng, opt=None):
    """One fit() of `epochs` epochs on the scenario's data; returns the optimizer."""
    opt = torch.optim.Adam(m.parameters(), **meta["adam"]) if opt is None else opt
    m.fit(str(tmp), np.array(sc["X_train"]), None, torch.nn.MSELoss(), opt, epochs=epochs, batch_size=meta["B"],
          check_every=1000, lambda1=meta["lam"], rng=rng)
    return opt


def check_scenario_epochs(name, tmp, device="cpu"):
    """Epoch by epoch (one fit() per epoch, the same optimizer) against the fixture."""
    meta, sc = load_nl(name)
    m = build(meta, device)
    rng = ReplayRNG(perms_of(meta, sc))
    opt, mse, l1 = None, [], []
    for e in range(1, meta["epochs"] + 1):
        opt = fit_epochs(m, meta, sc, tmp, 1, rng, opt)
        mse.append(m.step_losses[0])
        l1.append(m.step_losses[1])
        want = sub(sc, "epoch%d" % e)
        if want:
            compare_state_dict("%s/epoch%d" % (name, e), state_of(m), want, whh_stride=meta.get("whh_stride"))
    assert rng.at == len(rng.perms)
    assert_close(name + "/mse", np.concatenate(mse), sc["mse"], RTOL, ATOL)
    assert_close(name + "/l1", np.concatenate(l1), sc["l1"], RTOL, ATOL)
    assert_close(name + "/causal", m.GC(), sc["causal"], RTOL, ATOL)


def check_whole_fit(name, tmp, device="cpu"):
    meta, sc = load_nl(name)
    m = build(meta, device)
    opt = torch.optim.Adam(m.parameters(), **meta["adam"])
    np.random.seed(meta["seed"] + 300)
    lv = m.fit(str(tmp), np.array(sc["X_train"]), None, torch.nn.MSELoss(), opt, val_proportion=0.0,
               epochs=meta["epochs"], batch_size=meta["B"], check_every=2, lambda1=meta["lam"])
    compare_state_dict("%s/fit0" % name, state_of(m), sub(sc, "fit0/final"))
    assert_close("causal", m.GC(), sc["fit0/causal"], RTOL, ATOL)
    assert float(lv) == 0.0 and float(sc["fit0/loss_val"]) == 0.0
    return m


# ------------------------------------------------------------------------------------------ the class
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_seeded_construction_is_the_references(name):
    meta, sc = load_nl(name)
    got, want = state_of(build(meta)), sub(sc, "init")
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    names = [n for n, _ in build(meta).named_parameters()]
    assert names[:3] == ["biases", "lstm_list.0.weight_ih_l0", "lstm_list.0.weight_hh_l0"]
    assert len(names) == 1 + 6 * meta["N"]


def test_forward_shapes_and_row_order():
    meta, sc = load_nl("b")
    m = build(meta)
    N, Tp = meta["N"], meta["Tp"]
    x = torch.from_numpy(np.array(sc["X_train"][:5])).transpose(1, 2)[:, :, :-1]
    pred, contrib = m(x)
    assert pred.shape == (5, N, Tp) and contrib.shape == (5 * Tp, N * N, 1)
    c4 = contrib.view(5, Tp, N, N)  # row b*T' + t, channel i*N + j
    assert torch.allclose(pred, c4.sum(2).permute(0, 2, 1) + m.biases.view(1, N, 1), atol=1e-6)
    # the contribution of source i at step t is fc_i(lstm_i(x_i))[t]
    for i in (0, N - 1):
        out, _ = m.lstm_list[i](x[:, i, :].unsqueeze(-1))
        assert torch.allclose(c4[:, :, i, :], m.fc_list[i](out), atol=1e-6)
    assert m.GC() is None
    # causality in time: step t does not see the inputs after it
    x2 = x.clone()
    x2[:, :, -1] += 1.0
    pred2, _ = m(x2)
    assert torch.equal(pred2[:, :, :-1], pred[:, :, :-1]) and not torch.equal(pred2[:, :, -1], pred[:, :, -1])


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "w"])
def test_generic_route_reproduces_the_reference(name, tmp_path, monkeypatch):
    monkeypatch.setenv("REDCLIFF_NAVAR_LSTM_PATH", "generic")
    check_scenario_epochs(name, tmp_path)


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_fit_consumes_the_rng_as_the_reference(name, tmp_path):
    meta, sc = load_nl(name)
    drawn = []
    real = np.random.choice

    def spy(*a, **k):
        out = real(*a, **k)
        drawn.append(np.array(out))
        return out
    np.random.seed(meta["seed"] + 200)
    m = build(meta)
    try:
        np.random.choice = spy
        fit_epochs(m, meta, sc, tmp_path, meta["epochs"], None)
    finally:
        np.random.choice = real
    want = perms_of(meta, sc)
    assert len(drawn) == len(want)
    for g, w in zip(drawn, want):
        assert np.array_equal(g, w)
    if name == "d":
        assert len(drawn) == 0 and len(m.step_losses[0]) == meta["epochs"]
    if name == "c":
        assert len(m.step_losses[0]) == 2 * meta["epochs"]


@pytest.mark.parametrize("name", ["a", "b"])
def test_whole_fit_and_saved_model(name, tmp_path):
    m = check_whole_fit(name, tmp_path)
    # the pickle loads in a process that cannot load the native library and reproduces GC()
    np.save(os.path.join(str(tmp_path), "gc.npy"), m.GC())
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sys.modules["redcliff_amd"].__file__)))
    code = ("import sys, os, numpy as np, torch\n"
            "sys.path.insert(0, %r)\n"
            "os.environ['REDCLIFF_HIP_LIB'] = '/nonexistent/libredcliff_hip.so'\n"
            "m = torch.load(os.path.join(%r, 'final_best_model.bin'), weights_only=False)\n"
            "assert '_nv_slot' not in m.__dict__\n"
            "assert np.array_equal(m.GC(), np.load(os.path.join(%r, 'gc.npy')))\n"
            "p, c = m(torch.zeros(2, m.num_nodes, 4))\n"
            "assert p.shape == (2, m.num_nodes, 4)\n" % (pkg, str(tmp_path), str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_validation_uses_the_last_time_step(tmp_path):
    """The reference's validation line compares (n, N, T') with (n, N) and raises; with val_proportion > 0
    this port takes val_pred[:, :, -1], the training loss's form."""
    meta, sc = load_nl("a")
    m = build(meta)
    opt = torch.optim.Adam(m.parameters(), **meta["adam"])
    X = np.array(sc["X_train"])
    Xva = X[:5] * 0.5
    lv = m.fit(str(tmp_path), X, None, torch.nn.MSELoss(), opt, X_val=Xva, val_proportion=0.5, epochs=2,
               batch_size=meta["B"], check_every=2, lambda1=meta["lam"], rng=np.random.RandomState(3))
    xv = torch.from_numpy(np.swapaxes(Xva, 2, 1))
    with torch.no_grad():
        pred, _ = m(xv[:, :, :-1])
        want = torch.nn.functional.mse_loss(pred[:, :, -1], xv[:, :, -1])
    assert float(lv) > 0.0
    assert_close("loss_val", float(lv), float(want), 1e-6, 1e-7)
    # the reference's own form cannot broadcast at these shapes (N = 3, T' = 3, five windows)
    with pytest.raises(RuntimeError):
        torch.nn.MSELoss()(pred, xv[:, :, -1])


# ------------------------------------------------------------------------------------------ limits / ABI
def test_limit_function_matches_the_native_query():
    from redcliff_amd import navar_lstm as nl
    assert nl.navar_lstm_lds_floats(10, 256, 20, Bmax=128, R=15) > 0  # the published shape
    grid = [(N, H, Tp, B, R) for N in (1, 3, 10, 32, 33) for H in (1, 16, 17, 33, 256, 257, 448, 449, 512)
            for Tp in (1, 20, 64, 65) for B, R in ((1, 1), (512, 256), (513, 1), (128, 257), (128, 15))]
    seen = set()
    for N, H, Tp, B, R in grid:
        want = nl.navar_lstm_supported(N, H, Tp, B, R)
        got = nl.navar_lstm_lds_floats(N, H, Tp, B, R)
        assert got == want, (N, H, Tp, B, R, got, want)
        seen.add(got > 0)
    assert seen == {True, False}
    # both sides of every limit
    ok = (32, 448, 64, 512, 256)
    assert nl.navar_lstm_supported(*ok) > 0 and nl.navar_lstm_lds_floats(*ok) <= nl.LDS_MAX_FLOATS
    for at in range(5):
        over = list(ok)
        over[at] += 1
        assert nl.navar_lstm_supported(*over) == 0 and nl.navar_lstm_lds_floats(*over) == 0, over
        under = list(ok)
        under[at] = 0
        assert nl.navar_lstm_supported(*under) == 0 and nl.navar_lstm_lds_floats(*under) == 0, under
    # the restated workspace size
    lib = nl.nat.lib()
    for N, H, Tp, B in ((3, 5, 3, 6), (10, 256, 20, 128), (4, 33, 5, 16), (1, 1, 1, 1)):
        d = nl.navar_lstm_dims(N, H, Tp, Bmax=B)
        for train in (0, 1):
            assert lib.redcliff_navar_lstm_ws_floats(ctypes.byref(d), B, train) == nl.navar_lstm_ws_floats(N, H, Tp, B, bool(train))


def test_run_checks_arguments_before_any_launch():
    from redcliff_amd import _native as nat
    from redcliff_amd import navar_lstm as nl
    lib = nat.lib()
    a = nat.NavarLstmArgs()
    assert lib.redcliff_navar_lstm_run(None, None) == -1
    a.d = nl.navar_lstm_dims(10, 449, 20, Bmax=128)
    assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == -2
    a.d = nl.navar_lstm_dims(3, 5, 3, Bmax=8)
    a.mode, a.B, a.tB, a.N, a.nX = 0, 8, 1, 8, 8
    assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == -1  # null buffers
    for fld in ("X", "perm", "par", "par_m", "par_v", "hyper", "mse", "l1", "ws", "pred", "contrib"):
        setattr(a, fld, 4096)  # never dereferenced: every check below precedes any HIP call
    a.ws_bytes = 4
    assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == -3
    a.ws_bytes = 1 << 30
    for fld, bad in (("mode", 2), ("B", 0), ("B", 9), ("N", -1), ("tB", 0), ("x_pstride", -1), ("nX", 0), ("launches", 16)):
        keep = getattr(a, fld)
        setattr(a, fld, bad)
        assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == -1, fld
        setattr(a, fld, keep)
    a.mode, a.row0 = 1, 1  # FORWARD past the end of the set
    assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == -1
    a.mode, a.row0 = 0, 0
    reps = (ctypes.c_int32 * 2)(1, 0)
    a.d.R = 2
    a.replicas, a.n_replicas = ctypes.cast(reps, ctypes.c_void_p), 2
    assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == -1  # not increasing
    a.n_replicas = 0
    assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == 0   # an empty list launches nothing
    a.replicas, a.N = None, 0
    assert lib.redcliff_navar_lstm_run(ctypes.byref(a), None) == 0   # nothing to do
    assert nat.lib().redcliff_abi_version() == 10


def test_navar_lstm_kernels_use_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    for key in ("k_nl_fwd", "k_nl_out", "k_nl_dc", "k_nl_red", "k_nl_bwd", "k_nl_upd"):
        hits = [(n, v) for n, v in ks.items() if key in n]
        assert hits, "kernel %s not in the library" % key
        for n, v in hits:
            assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])


def test_packed_layout_covers_every_parameter_once():
    from redcliff_amd import navar_lstm as nl
    meta, _ = load_nl("b")
    m = build(meta)
    layout, total = nl.navar_lstm_layout(meta["N"], meta["H"])
    groups = m.packed_parameters()
    assert [name for name, _, _ in layout] == ["Wih", "Whh", "bih", "bhh", "Wfc", "bfc", "biases"]
    assert sum(p.numel() for g in groups for p in g) == total == sum(p.numel() for p in m.parameters())
    assert set(id(p) for g in groups for p in g) == set(id(p) for p in m.parameters())
    at = 0
    for g, (_, off, shp) in zip(groups, layout):
        assert off == at and sum(p.numel() for p in g) == int(np.prod(shp))
        at += int(np.prod(shp))


# ------------------------------------------------------------------------------------------ routes
def test_bad_route_value_raises(monkeypatch):
    from redcliff_amd import navar_lstm as nl
    monkeypatch.setenv("REDCLIFF_NAVAR_LSTM_PATH", "eager")
    with pytest.raises(ValueError):
        nl.navar_lstm_path()
    with pytest.raises(ValueError):
        build(load_nl("a")[0]).fused_eligible()
    monkeypatch.setenv("REDCLIFF_NAVAR_LSTM_PATH", "generic")
    assert nl.navar_lstm_path() == "generic"
    monkeypatch.delenv("REDCLIFF_NAVAR_LSTM_PATH")
    assert nl.navar_lstm_path() == "fused"


def ineligible_cases():
    adam = lambda ps: torch.optim.Adam(ps, lr=1e-3)
    return [("dropout", dict(hidden_layers=2, dropout=0.5), adam),
            ("two_layers", dict(hidden_layers=2), adam),
            ("sgd", {}, lambda ps: torch.optim.SGD(ps, lr=1e-3)),
            ("amsgrad", {}, lambda ps: torch.optim.Adam(ps, lr=1e-3, amsgrad=True)),
            ("cpu", {}, adam)]


@pytest.mark.parametrize("case", ineligible_cases(), ids=lambda c: c[0])
def test_ineligible_configurations_take_the_generic_route(case, tmp_path):
    from redcliff_amd import NAVARLSTM
    tag, ckw, mk = case
    torch.manual_seed(0)
    m = NAVARLSTM(3, 4, 2, **ckw)
    opt = mk(m.parameters())
    assert not m.fused_eligible(torch.nn.MSELoss(), opt, T=4, Bmax=4)
    X = np.random.RandomState(0).randn(9, 4, 3).astype(np.float32)
    before = state_of(m)
    m.fit(str(tmp_path), X, None, torch.nn.MSELoss(), opt, epochs=1, batch_size=4, rng=np.random.RandomState(1))
    assert m.GC().shape == (3, 3) and "_nv_slot" not in m.__dict__
    assert any(not np.array_equal(before[k], v) for k, v in state_of(m).items())
