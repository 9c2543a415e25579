"""CPU-side checks of the supervised DGCNN baseline's fit (redcliff_amd.dgcnn, csrc/rc_dgcnn_fit.hip) against
the reference fixture tests/golden/dgcnn_fit.npz (+ dgcnn_fit_e.npz): seeded construction, the generic route
epoch by epoch, whole fits and the files they write, label selection, the route switch, the packed layout,
the restated limit / workspace functions against the native queries, the argument checks of
redcliff_dgcnn_fit_run and the kernels' resource metadata.  No kernel is launched."""
import ctypes
import json
import os
import pickle as pkl
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, assert_close
from test_kernel_occupancy import _kernels

STATE_RTOL, STATE_ATOL = 2e-4, 5e-6  # the project's state bound (tests/test_fm_host.py)
RTOL, ATOL = 1e-4, 1e-6              # loss values

_FIXTURE = {}


def load_dgcnn(name):
    """(meta, {key: array}) of one scenario of dgcnn_fit.npz / dgcnn_fit_e.npz (read once, never modified)."""
    if not _FIXTURE:
        for fname in ("dgcnn_fit.npz", "dgcnn_fit_e.npz"):
            d = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
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
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(want[k]), (tag, k, int(got[k]), int(want[k]))
            continue
        scale = max(1.0, float(np.abs(want[k]).max()))
        assert_close("%s/%s" % (tag, k), got[k], want[k], rtol, atol * scale)


def state_of(m):
    return dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())


def build(meta, device="cpu"):
    from redcliff_amd import DGCNN_Model
    torch.manual_seed(meta["seed"])
    return DGCNN_Model(meta["n"], 1, meta["F"], meta["layers"], meta["H"], meta["C"]).to(device)


def loader(X, Y, B):
    X, Y = torch.from_numpy(np.array(X)), torch.from_numpy(np.array(Y))
    return [(X[i:i + B], Y[i:i + B]) for i in range(0, X.shape[0], B)]


def loaders(meta, sc):
    return loader(sc["X"], sc["Y"], meta["B"]), loader(sc["X_val"], sc["Y_val"], meta["B"])


def check_scenario_epochs(name, tmp, device="cpu"):
    """Epoch by epoch (one fit() of one epoch each, the same optimizer) against the fixture."""
    meta, sc = load_dgcnn(name)
    m = build(meta, device)
    opt = torch.optim.Adam(m.dgcnn.parameters(), **meta["adam"])
    tr, va = loaders(meta, sc)
    losses, ev = [], None
    for e in range(1, meta["epochs"] + 1):
        ev = m.fit(str(tmp), tr, opt, 1, 1, 1, 0, None, va)
        losses.append(m.step_losses)
        assert m.stopped_at == 0 and len(m.avg_factor_loss) == 1
        assert_close("avg_factor_loss", m.avg_factor_loss[0], float(np.mean(sc["loss"][(e - 1) * len(tr):e * len(tr)])),
                     RTOL, ATOL)
        want = sub(sc, "epoch%d" % e)
        if want:
            compare_state_dict("%s/epoch%d" % (name, e), state_of(m), want)
        assert int(m.dgcnn.BN1.num_batches_tracked) == e * len(tr)
    assert_close(name + "/loss", np.concatenate(losses), sc["loss"], RTOL, ATOL)
    assert_close(name + "/eval", float(ev), sc["eval"], RTOL, ATOL)
    return m, opt


def check_whole_fit(name, tmp, device="cpu"):
    meta, sc = load_dgcnn(name)
    m = build(meta, device)
    init = state_of(m)
    opt = torch.optim.Adam(m.dgcnn.parameters(), **meta["adam"])
    tr, va = loaders(meta, sc)
    lv = m.fit(str(tmp), tr, opt, 7, 1, 2, 0, [np.zeros((meta["n"], meta["n"]))], va)
    compare_state_dict(name + "/fit", state_of(m), sub(sc, "fit/final"))
    assert_close("GC", m.GC(threshold=False).detach().cpu().numpy(), sc["fit/GC"], STATE_RTOL, STATE_ATOL)
    assert_close("loss", float(lv), sc["fit/loss"], RTOL, ATOL)
    assert m.stopped_at == int(sc["fit/stopped_at"])
    assert len(m.avg_factor_loss) == m.stopped_at + 1
    files = sorted(os.listdir(str(tmp)))
    assert files == ["final_best_model.bin", "temp_best_model_epoch0.bin", "training_meta_data_and_hyper_parameters.pkl"]
    with open(os.path.join(str(tmp), "training_meta_data_and_hyper_parameters.pkl"), "rb") as f:
        meta_saved = pkl.load(f)
    assert meta_saved["epoch"] == 0 and len(meta_saved["avg_factor_loss"]) == 1 and set(meta_saved) == {
        "epoch", "avg_factor_loss", "best_loss"}
    if meta["layers"] == 1:
        assert np.array_equal(state_of(m)["dgcnn.A"].view(np.int32), init["dgcnn.A"].view(np.int32))
        assert m.dgcnn.A not in opt.state and len(opt.state) == len(list(m.dgcnn.parameters())) - 1
    return m, opt


# ------------------------------------------------------------------------------------------ the class
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_seeded_construction_is_the_references(name):
    meta, sc = load_dgcnn(name)
    got, want = state_of(build(meta)), sub(sc, "init")
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def test_forward_uses_x_itself_for_support_zero():
    meta, sc = load_dgcnn("c")
    m = build(meta)
    x = torch.from_numpy(np.array(sc["X"][:5]))[:, :meta["F"], :].transpose(1, 2)
    out = m(x)
    assert out.shape == (5, meta["C"])
    out.sum().backward()
    assert m.dgcnn.A.grad is None and m.dgcnn.layer1.gc1[0].weight.grad is not None
    m64 = build(load_dgcnn("b")[0]).double()
    assert m64(torch.zeros(2, 5, 3, dtype=torch.float64)).dtype == torch.float64


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_generic_route_reproduces_the_reference(name, tmp_path, monkeypatch):
    monkeypatch.setenv("REDCLIFF_DGCNN_PATH", "generic")
    m, opt = check_scenario_epochs(name, tmp_path)
    assert "_dg_slot" not in m.__dict__
    if name == "c":
        meta, sc = load_dgcnn(name)
        assert np.array_equal(state_of(m)["dgcnn.A"].view(np.int32), sc["init/dgcnn.A"].view(np.int32))
        assert m.dgcnn.A not in opt.state


@pytest.mark.parametrize("name", ["a", "c"])
def test_whole_fit_and_saved_model(name, tmp_path):
    m, _ = check_whole_fit(name, tmp_path)
    # the pickles load in a process that cannot load the native library and reproduce GC()
    np.save(os.path.join(str(tmp_path), "gc.npy"), m.GC(threshold=False).detach().numpy())
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(sys.modules["redcliff_amd"].__file__)))
    code = ("import sys, os, numpy as np, torch\n"
            "sys.path.insert(0, %r)\n"
            "os.environ['REDCLIFF_HIP_LIB'] = '/nonexistent/libredcliff_hip.so'\n"
            "for f in ('final_best_model.bin', 'temp_best_model_epoch0.bin'):\n"
            "    m = torch.load(os.path.join(%r, f), weights_only=False)\n"
            "    assert '_dg_slot' not in m.__dict__\n"
            "    assert m(torch.zeros(2, m.num_nodes, m.num_features_per_node)).shape == (2, m.num_classes)\n"
            "assert np.array_equal(m.GC(threshold=False).detach().numpy(), np.load(os.path.join(%r, 'gc.npy')))\n"
            % (pkg, str(tmp_path), str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True)


# ------------------------------------------------------------------------------------------ host logic
def test_label_selection_by_rank():
    from redcliff_amd.dgcnn import select_labels
    F = 3
    y2 = torch.arange(10.).reshape(5, 2)
    assert select_labels(y2, F) is y2
    y3 = torch.arange(5. * 2 * 6).reshape(5, 2, 6)
    assert torch.equal(select_labels(y3, F), y3[:, :, F])
    y31 = torch.arange(10.).reshape(5, 2, 1)
    assert torch.equal(select_labels(y31, F), y31[:, :, 0])
    with pytest.raises(AssertionError):
        select_labels(torch.zeros(5, 2, 2), F)  # neither longer than F nor 1 (models/dgcnn.py:86)
    for bad in (torch.zeros(5), torch.zeros(5, 2, 3, 4)):
        with pytest.raises(NotImplementedError):
            select_labels(bad, F)
    meta, sc = load_dgcnn("b")
    assert np.array_equal(select_labels(torch.from_numpy(np.array(sc["Y"])), meta["F"]).numpy(), sc["Ysel"])
    meta, sc = load_dgcnn("c")
    assert np.array_equal(select_labels(torch.from_numpy(np.array(sc["Y"])), meta["F"]).numpy(), sc["Ysel"])


def test_route_parsing(monkeypatch):
    from redcliff_amd import dgcnn as dg
    monkeypatch.setenv("REDCLIFF_DGCNN_PATH", "eager")
    with pytest.raises(ValueError):
        dg.dgcnn_path()
    with pytest.raises(ValueError):
        build(load_dgcnn("a")[0]).fused_eligible()
    monkeypatch.setenv("REDCLIFF_DGCNN_PATH", "generic")
    assert dg.dgcnn_path() == "generic"
    monkeypatch.setenv("REDCLIFF_DGCNN_PATH", "")
    assert dg.dgcnn_path() == "fused"
    monkeypatch.delenv("REDCLIFF_DGCNN_PATH")
    assert dg.dgcnn_path() == "fused"


def test_fused_route_declines_what_it_does_not_serve(monkeypatch):
    monkeypatch.delenv("REDCLIFF_DGCNN_PATH", raising=False)
    meta, _ = load_dgcnn("a")
    m = build(meta)
    adam = torch.optim.Adam(m.dgcnn.parameters(), lr=1e-3)
    assert not m.fused_eligible(adam)            # CPU parameters
    assert not m.double().fused_eligible()       # float64
    m = build(meta)
    assert not m.fused_eligible(torch.optim.SGD(m.dgcnn.parameters(), lr=1e-3))
    assert not m.fused_eligible(torch.optim.Adam(list(m.dgcnn.parameters())[:-1], lr=1e-3))  # a subset (no A)
    assert not m.fused_eligible(torch.optim.Adam(m.dgcnn.parameters(), lr=1e-3, amsgrad=True))
    # the optimizer rules themselves, apart from the device: a stand-in whose parameters report 'cuda'
    from redcliff_amd import dgcnn as dg

    class OnDevice(dg.DGCNN_Model):
        def fused_eligible(self, optimizer=None, T=None, Bmax=1):
            try:
                torch.Tensor.is_cuda = property(lambda self: True)  # shadows the base class's attribute
                return super().fused_eligible(optimizer, T, Bmax)
            finally:
                del torch.Tensor.is_cuda
    torch.manual_seed(0)
    m = OnDevice(3, 1, 2, 2, 5, 2)
    ps = list(m.dgcnn.parameters())
    assert m.fused_eligible(torch.optim.Adam(ps, lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.SGD(ps, lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.Adam(ps[:-1], lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.AdamW(ps, lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.Adam([{"params": ps[:2]}, {"params": ps[2:]}], lr=1e-3), T=4, Bmax=6)
    assert not m.fused_eligible(torch.optim.Adam(ps, lr=1e-3), T=1, Bmax=6)     # fewer rows than features
    assert not m.fused_eligible(torch.optim.Adam(ps, lr=1e-3), T=4, Bmax=129)   # outside the limits


def test_packed_layout_is_the_parameter_tree():
    from redcliff_amd import dgcnn as dg
    for name in ("a", "b", "c", "e"):
        meta, _ = load_dgcnn(name)
        m = build(meta)
        layout, total = dg.dgcnn_fit_layout(*m.fit_shape())
        prms = m.packed_parameters()
        assert len(prms) == len(layout) == len(list(m.dgcnn.parameters()))
        assert set(id(p) for p in prms) == set(id(p) for p in m.dgcnn.parameters())
        at = 0
        for prm, (_, off, shp) in zip(prms, layout):
            assert off == at and tuple(prm.shape) == tuple(shp)
            at += prm.numel()
        assert at == total
        d = dg.dgcnn_fit_dims(*m.fit_shape())
        from redcliff_amd import _native as nat
        assert int(nat.lib().redcliff_emb_param_count(ctypes.byref(d))) == total


# ------------------------------------------------------------------------------------------ limits / ABI
def test_limit_and_workspace_functions_match_the_native_queries():
    from redcliff_amd import _native as nat
    from redcliff_amd import dgcnn as dg
    assert dg.dgcnn_fit_lds_floats(10, 2, 1, 100, 5, Bmax=128) > 0   # D4IC
    assert dg.dgcnn_fit_lds_floats(10, 2, 3, 250, 3, Bmax=128) > 0   # the synthetic-systems grid
    seen = set()
    for n in (1, 3, 10, 32, 33):
        for F in (1, 2, 8, 9):
            for layers in (1, 3, 4, 5):
                for H in (1, 33, 250, 256, 257):
                    for C in (1, 5, 16, 17):
                        for B, T, R in ((1, None, 1), (128, None, 256), (129, None, 1), (128, F - 1, 1), (16, F + 3, 257)):
                            want = dg.dgcnn_fit_supported(n, F, layers, H, C, B, T, R)
                            got = dg.dgcnn_fit_lds_floats(n, F, layers, H, C, B, T, R)
                            assert got == want, (n, F, layers, H, C, B, T, R, got, want)
                            seen.add(got > 0)
                            if got and B <= 128:
                                d = dg.dgcnn_fit_dims(n, F, layers, H, C, B, T, R)
                                for N in (1, B, 3 * B + 1):
                                    assert int(nat.lib().redcliff_dgcnn_fit_ws_floats(ctypes.byref(d), B, N)) == \
                                        dg.dgcnn_fit_ws_floats(n, F, layers, H, C, B, N)
    assert seen == {True, False}
    # both sides of the LDS limit: every dimension at its maximum does not fit together
    assert dg.dgcnn_fit_lds_floats(32, 1, 4, 256, 1, Bmax=128) > 0 and dg.dgcnn_fit_lds_floats(32, 8, 4, 256, 16, Bmax=128) == 0
    assert dg.dgcnn_fit_supported(32, 8, 4, 256, 16, 128) == 0
    assert dg.dgcnn_fit_supported(0, 2, 1, 5, 2) == 0 and dg.dgcnn_fit_supported(3, 2, 0, 5, 2) == 0
    d = dg.dgcnn_fit_dims(10, 2, 3, 257, 3, 128)
    assert int(nat.lib().redcliff_dgcnn_fit_ws_floats(ctypes.byref(d), 128, 300)) == 0


def test_run_checks_arguments_before_any_launch():
    from redcliff_amd import _native as nat
    from redcliff_amd import dgcnn as dg
    lib = nat.lib()
    a = nat.DgcnnFitArgs()
    assert lib.redcliff_dgcnn_fit_run(None, None) == -1
    a.d = dg.dgcnn_fit_dims(10, 2, 3, 257, 3, Bmax=128)
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == -2
    a.d = dg.dgcnn_fit_dims(3, 2, 2, 5, 2, Bmax=8, T=4)
    a.mode, a.B, a.tB, a.N, a.nX = 0, 8, 1, 8, 8
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == -1  # null buffers
    for fld in ("X", "Y", "par", "par_m", "par_v", "bn_rm", "bn_rv", "hyper", "loss", "pred", "ws"):
        setattr(a, fld, 4096)  # never dereferenced: every check below precedes any HIP call
    a.ws_bytes = 4
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == -3
    a.ws_bytes = 1 << 30
    for fld, bad in (("mode", 2), ("B", 0), ("B", 9), ("N", -1), ("tB", 0), ("x_pstride", -1), ("y_pstride", -1),
                     ("par_stride", -1), ("nX", 0), ("row0", -1), ("row0", 1), ("launches", 8), ("launches", -1),
                     ("ws", 4100), ("X", None), ("Y", None), ("par_m", None), ("loss", None), ("hyper", None),
                     ("bn_rv", None)):
        keep = getattr(a, fld)
        setattr(a, fld, bad)
        assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == -1, fld
        setattr(a, fld, keep)
    a.mode = 1  # FORWARD: no labels is fine, no prediction buffer is not
    a.pred = None
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == -1
    a.mode, a.pred = 0, 4096
    reps = (ctypes.c_int32 * 2)(1, 0)
    a.d.R = 2
    a.replicas, a.n_replicas = ctypes.cast(reps, ctypes.c_void_p), 2
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == -1  # not increasing
    a.n_replicas = 3
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == -1  # longer than R
    a.n_replicas = 0
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == 0   # an empty list launches nothing
    a.replicas, a.N = None, 0
    assert lib.redcliff_dgcnn_fit_run(ctypes.byref(a), None) == 0   # nothing to do
    assert nat.lib().redcliff_abi_version() == 10


def test_dgcnn_fit_kernels_use_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    for key in ("k_dg_stats", "k_dg_fwd", "k_dg_bwd", "k_dg_tail", "k_dg_out"):
        hits = [(n, v) for n, v in ks.items() if key in n]
        assert hits, "kernel %s not in the library" % key
        for n, v in hits:
            assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])
