"""CPU-side checks of the NAVAR baseline (redcliff_amd.navar, csrc/rc_navar.hip) against the reference
fixture tests/golden/navar.npz: seeded construction, the generic route step by step, the reference's
RNG consumption, whole fits and the saved model, the restated limit function against
redcliff_navar_supported, the argument checks of redcliff_navar_run, the kernels' resource metadata and
the route switch.  No kernel is launched."""
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


def load_navar(name):
    """(meta, {key: array}) of one scenario of navar.npz (read once, never modified)."""
    if not _FIXTURE:
        d = np.load(os.path.join(GOLDEN, "navar.npz"), allow_pickle=False)
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


def compare_state_dict(tag, got, want, rtol=STATE_RTOL, atol=STATE_ATOL):
    assert set(got) == set(want), tag
    for k in want:
        scale = max(1.0, float(np.abs(want[k]).max()))
        assert_close("%s/%s" % (tag, k), got[k], want[k], rtol, atol * scale)


def state_of(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


def build(meta, device="cpu"):
    from redcliff_amd import NAVAR
    torch.manual_seed(meta["seed"])
    return NAVAR(meta["N"], meta["H"], meta["K"], hidden_layers=meta["layers"], dropout=0).to(device)


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


def fit_epochs(m, meta, sc, tmp, epochs, rng, opt=None, device="cpu"):
    """One fit() of `epochs` epochs on the scenario's data; returns the optimizer."""
    opt = torch.optim.Adam(m.parameters(), **meta["adam"]) if opt is None else opt
    m.fit(str(tmp), np.array(sc["X_train"]), None, torch.nn.MSELoss(), opt, epochs=epochs, batch_size=meta["B"],
          check_every=1000, lambda1=meta["lam"], rng=rng)
    return opt


def check_scenario_epochs(name, tmp, device="cpu"):
    """Epoch by epoch (one fit() per epoch, the same optimizer) against the fixture."""
    meta, sc = load_navar(name)
    m = build(meta, device)
    rng = ReplayRNG(perms_of(meta, sc))
    opt, mse, l1 = None, [], []
    for e in range(1, meta["epochs"] + 1):
        opt = fit_epochs(m, meta, sc, tmp, 1, rng, opt, device)
        mse.append(m.step_losses[0])
        l1.append(m.step_losses[1])
        want = sub(sc, "epoch%d" % e)
        if want:
            compare_state_dict("%s/epoch%d" % (name, e), state_of(m), want)
    assert rng.at == len(rng.perms)
    assert_close(name + "/mse", np.concatenate(mse), sc["mse"], RTOL, ATOL)
    assert_close(name + "/l1", np.concatenate(l1), sc["l1"], RTOL, ATOL)
    assert_close(name + "/causal", m.GC(), sc["causal"], RTOL, ATOL)


# ------------------------------------------------------------------------------------------ the class
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_seeded_construction_is_the_references(name):
    meta, sc = load_navar(name)
    got, want = state_of(build(meta)), sub(sc, "init")
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def test_forward_shapes_and_additivity():
    meta, sc = load_navar("b")
    m = build(meta)
    x = torch.from_numpy(np.array(sc["X_train"][:5])).transpose(1, 2)[:, :, :-1]
    pred, contrib = m(x)
    N = meta["N"]
    assert pred.shape == (5, N) and contrib.shape == (5, N * N, 1)
    want = contrib.view(5, N, N).sum(1) + m.biases
    assert torch.allclose(pred, want, atol=1e-7)
    assert m.GC() is None


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "w"])
def test_generic_route_reproduces_the_reference(name, tmp_path, monkeypatch):
    monkeypatch.setenv("REDCLIFF_NAVAR_PATH", "generic")
    check_scenario_epochs(name, tmp_path)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_fit_consumes_the_rng_as_the_reference(name, tmp_path):
    meta, sc = load_navar(name)
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
@pytest.mark.parametrize("v", [0, 5])
def test_whole_fit_and_saved_model(name, v, tmp_path):
    meta, sc = load_navar(name)
    m = build(meta)
    opt = torch.optim.Adam(m.parameters(), **meta["adam"])
    np.random.seed(meta["seed"] + 300)
    lv = m.fit(str(tmp_path), np.array(sc["X_train"]), None, torch.nn.MSELoss(), opt, X_val=np.array(sc["X_val"]),
               val_proportion=v / 10.0, epochs=meta["epochs"], batch_size=meta["B"], check_every=2, lambda1=meta["lam"])
    pre = "fit%d" % v
    compare_state_dict("%s/%s" % (name, pre), state_of(m), sub(sc, pre + "/final"))
    assert_close("causal", m.GC(), sc[pre + "/causal"], RTOL, ATOL)
    assert_close("loss_val", float(lv), sc[pre + "/loss_val"], RTOL, ATOL)
    if v == 0:
        assert float(lv) == 0.0
    # the pickle loads in a process that cannot load the native library and reproduces GC()
    np.save(os.path.join(str(tmp_path), "gc.npy"), m.GC())
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sys.modules["redcliff_amd"].__file__)))
    code = ("import sys, os, numpy as np, torch\n"
            "sys.path.insert(0, %r)\n"
            "os.environ['REDCLIFF_HIP_LIB'] = '/nonexistent/libredcliff_hip.so'\n"
            "m = torch.load(os.path.join(%r, 'final_best_model.bin'), weights_only=False)\n"
            "assert '_nv_slot' not in m.__dict__\n"
            "assert np.array_equal(m.GC(), np.load(os.path.join(%r, 'gc.npy')))\n"
            "p, c = m(torch.zeros(2, m.num_nodes, m.maxlags))\n"
            "assert p.shape == (2, m.num_nodes)\n" % (pkg, str(tmp_path), str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True)


# ------------------------------------------------------------------------------------------ limits / ABI
def test_limit_function_matches_the_native_query():
    from redcliff_amd import navar as nv
    assert nv.navar_lds_floats(10, 256, 20, 2, Bmax=128) > 0  # the published shape
    grid = [(N, H, K, layers, B, T, R)
            for N in (1, 3, 10, 32, 33) for H in (1, 33, 256, 257, 272, 273, 512, 513) for K in (1, 20, 64, 65)
            for layers in (1, 2, 3) for B, T, R in ((1, None, 1), (512, None, 256), (513, None, 1), (128, K, 1),
                                                    (128, K + 5, 257))]
    seen = set()
    for N, H, K, layers, B, T, R in grid:
        want = nv.navar_supported(N, H, K, layers, B, T, R)
        got = nv.navar_lds_floats(N, H, K, layers, B, T, R)
        assert got == want, (N, H, K, layers, B, T, R, got, want)
        seen.add(got > 0)
    assert seen == {True, False}
    # both sides of the LDS limit with two layers at the published N, K
    assert nv.navar_lds_floats(10, 256, 20, 2) > 0 and nv.navar_lds_floats(10, 257, 20, 2) == 0
    assert nv.navar_supported(10, 256, 20, 2) > 0 and nv.navar_supported(10, 257, 20, 2) == 0
    assert nv.navar_supported(0, 5, 2) == 0 and nv.navar_supported(3, 5, 2, 0) == 0


def test_run_checks_arguments_before_any_launch():
    from redcliff_amd import _native as nat
    from redcliff_amd import navar as nv
    lib = nat.lib()
    a = nat.NavarArgs()
    assert lib.redcliff_navar_run(None, None) == -1
    a.d = nv.navar_dims(10, 257, 20, 2, Bmax=128)
    assert lib.redcliff_navar_run(ctypes.byref(a), None) == -2
    a.d = nv.navar_dims(3, 5, 2, 1, Bmax=8)
    a.mode, a.B, a.tB, a.N, a.nX = 0, 8, 1, 8, 8
    assert lib.redcliff_navar_run(ctypes.byref(a), None) == -1  # null buffers
    for fld in ("X", "perm", "par", "par_m", "par_v", "hyper", "mse", "l1", "ws", "pred", "contrib"):
        setattr(a, fld, 4096)  # never dereferenced: every check below precedes any HIP call
    a.ws_bytes = 4
    assert lib.redcliff_navar_run(ctypes.byref(a), None) == -3
    a.ws_bytes = 1 << 30
    for fld, bad in (("mode", 2), ("B", 0), ("B", 9), ("N", -1), ("tB", 0), ("x_pstride", -1), ("nX", 0)):
        keep = getattr(a, fld)
        setattr(a, fld, bad)
        assert lib.redcliff_navar_run(ctypes.byref(a), None) == -1, fld
        setattr(a, fld, keep)
    a.mode, a.row0 = 1, 1  # FORWARD past the end of the set
    assert lib.redcliff_navar_run(ctypes.byref(a), None) == -1
    a.mode, a.row0 = 0, 0
    reps = (ctypes.c_int32 * 2)(1, 0)
    a.d.R = 2
    a.replicas, a.n_replicas = ctypes.cast(reps, ctypes.c_void_p), 2
    assert lib.redcliff_navar_run(ctypes.byref(a), None) == -1  # not increasing
    a.n_replicas = 0
    assert lib.redcliff_navar_run(ctypes.byref(a), None) == 0   # an empty list launches nothing
    a.replicas, a.N = None, 0
    assert lib.redcliff_navar_run(ctypes.byref(a), None) == 0   # nothing to do
    assert nat.lib().redcliff_abi_version() == 10


def test_navar_kernels_use_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    for key in ("k_navar_fwd", "k_navar_bwd", "k_navar_in", "k_navar_out"):
        hits = [(n, v) for n, v in ks.items() if key in n]
        assert hits, "kernel %s not in the library" % key
        for n, v in hits:
            assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])


# ------------------------------------------------------------------------------------------ routes
def test_bad_route_value_raises(monkeypatch):
    from redcliff_amd import navar as nv
    monkeypatch.setenv("REDCLIFF_NAVAR_PATH", "eager")
    with pytest.raises(ValueError):
        nv.navar_path()
    with pytest.raises(ValueError):
        build(load_navar("a")[0]).fused_eligible()
    monkeypatch.setenv("REDCLIFF_NAVAR_PATH", "generic")
    assert nv.navar_path() == "generic"
    monkeypatch.delenv("REDCLIFF_NAVAR_PATH")
    assert nv.navar_path() == "fused"


def ineligible_cases():
    """(tag, constructor kwargs, optimizer factory, fit kwargs, window rows T) the fused route declines."""
    adam = lambda ps: torch.optim.Adam(ps, lr=1e-3)
    return [("dropout", dict(dropout=0.5), adam, {}, 3),
            ("three_layers", dict(hidden_layers=3), adam, {}, 3),
            ("sgd", {}, lambda ps: torch.optim.SGD(ps, lr=1e-3), {}, 3),
            ("amsgrad", {}, lambda ps: torch.optim.Adam(ps, lr=1e-3, amsgrad=True), {}, 3),
            ("split_timeseries", {}, adam, dict(split_timeseries=True), 3),
            ("short_lags", {}, adam, {}, 5)]


@pytest.mark.parametrize("case", ineligible_cases(), ids=lambda c: c[0])
def test_ineligible_configurations_take_the_generic_route(case, tmp_path):
    from redcliff_amd import NAVAR
    tag, ckw, mk, fkw, T = case
    torch.manual_seed(0)
    m = NAVAR(3, 4, 2, **ckw)
    opt = mk(m.parameters())
    assert not m.fused_eligible(torch.nn.MSELoss(), opt, T=T, Bmax=4, split_timeseries=fkw.get("split_timeseries", False))
    X = np.random.RandomState(0).randn(9, T, 3).astype(np.float32)
    before = state_of(m)
    if tag in ("split_timeseries", "short_lags"):
        # the generic route is the reference's loop, whose torch ops reject these shapes (models/navar.py:99:
        # a third index into (B, N) predictions; (B * 3, N) predictions against (B, N) targets)
        with pytest.raises((IndexError, RuntimeError)):
            m.fit(str(tmp_path), X, None, torch.nn.MSELoss(), opt, epochs=1, batch_size=4,
                  rng=np.random.RandomState(1), **fkw)
        assert "_nv_slot" not in m.__dict__
        return
    m.fit(str(tmp_path), X, None, torch.nn.MSELoss(), opt, epochs=1, batch_size=4, rng=np.random.RandomState(1), **fkw)
    assert m.GC().shape == (3, 3) and "_nv_slot" not in m.__dict__
    assert any(not np.array_equal(before[k], v) for k, v in state_of(m).items())
