"""CPU-side checks of the dCSFA-NMF baseline (redcliff_amd.dcsfa_nmf, csrc/rc_dcsfa.hip): the generic route
against the fixture made from the reference's own classes (tests/golden/make_dcsfa_fit_golden.py), the host's
index draws, pretrain_NMF, the eligibility rules, the decided quirks, the evaluation branch and the compiled
kernels' resource metadata.  No kernel is launched here."""
import numpy as np
import pytest
import torch

import dcsfa_fit_common as C
from test_kernel_occupancy import _kernels

NEW_KERNELS = ["k_dc_fwd", "k_dc_head", "k_dc_bwd"]
SCENARIOS = ("a", "b", "c", "d")


@pytest.fixture(autouse=True)
def generic_route(monkeypatch):
    monkeypatch.setenv("REDCLIFF_DCSFA_PATH", "generic")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every scenario's generic fit on the CPU, run once."""
    import os
    out = {}
    mp = pytest.MonkeyPatch()
    mp.setenv("REDCLIFF_DCSFA_PATH", "generic")
    try:
        for name in SCENARIOS:
            folder = tmp_path_factory.mktemp("dcsfa_" + name)
            out[name] = C.run_scenario(name, "cpu", folder) + (folder,)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("name", SCENARIOS)
def test_generic_route_reproduces_the_reference(runs, name):
    m, log, _ = runs[name]
    C.check_against_fixture(name, m, log)
    fx = C.fixture(name)
    if not fx["cfg"]["val"]:
        C.assert_close(np.stack(m.GC(threshold=False)), fx["GC"], name + " GC")


@pytest.mark.parametrize("name", ("a", "c"))
def test_generic_whole_fit_with_validation(runs, name):
    m, _, folder = runs[name]
    C.check_whole_fit(name, m, folder)


@pytest.mark.parametrize("name", SCENARIOS)
def test_initialisation_and_index_draws_equal_the_fixture(name):
    """_initialize consumes the default generator as the reference's does, and draw_epoch_indices makes the
    generator calls of WeightedRandomSampler + DataLoader in their order: the rows are the fixture's."""
    from redcliff_amd import dcsfa_nmf as dn
    fx = C.fixture(name)
    cfg = fx["cfg"]
    m = C.build(cfg, "cpu", "unused")
    torch.manual_seed(cfg["seed"])
    m._initialize(cfg["D"])
    for k, v in C.sub(fx, "init/").items():
        np.testing.assert_array_equal(C.state(m)[k], v)
    w = torch.ones(cfg["N"], dtype=torch.float64)
    got = np.stack([dn.draw_epoch_indices(w, cfg["N"]).numpy() for _ in range(cfg["n_pre"] + cfg["n_epochs"])])
    np.testing.assert_array_equal(got, fx["idx"])


@pytest.mark.parametrize("name", ("a", "b", "c"))
def test_pretrain_nmf_against_the_fixture(name):
    pytest.importorskip("sklearn")
    import warnings
    fx = C.fixture(name)
    cfg = fx["cfg"]
    m = C.build(cfg, "cpu", "unused")
    m._initialize(cfg["D"])
    np.random.seed(cfg["seed"])  # sklearn's nndsvd initialisation draws from numpy's global generator
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.pretrain_NMF(fx["X"], fx["y"], 100)
    C.assert_close(m.W_nmf.detach().numpy(), fx["nmf/W_nmf"], name + " W_nmf after pretrain_NMF")


def test_pretrain_nmf_without_sklearn_raises_and_the_module_imports(monkeypatch):
    from redcliff_amd import dcsfa_nmf as dn
    cfg = C.fixture("c")["cfg"]
    m = C.build(cfg, "cpu", "unused")
    m._initialize(cfg["D"])
    monkeypatch.setattr(dn, "SKLEARN_INSTALLED", False)
    with pytest.raises(ImportError, match="scikit-learn"):
        m.pretrain_NMF(np.ones((4, cfg["D"])), np.ones((4, 1)))


def test_eligibility_rules(monkeypatch):
    from redcliff_amd import dcsfa_nmf as dn
    cfg = C.fixture("a")["cfg"]
    ok = lambda **kw: C.build(cfg, kw.pop("device", "cuda"), "unused", **kw)
    assert not ok().fused_eligible(16, dim_in=27)  # the generic route is asked for
    monkeypatch.setenv("REDCLIFF_DCSFA_PATH", "fused")
    assert dn.dcsfa_path() == "fused"
    assert ok().fused_eligible(16, dim_in=27)
    assert ok().fused_eligible(128, dim_in=500) and not ok().fused_eligible(129, dim_in=27)
    assert not ok(device="cpu").fused_eligible(16, dim_in=27)
    for kw in (dict(optim_name="Adam"), dict(optim_name="SGD"), dict(sup_recon_type="All"), dict(use_deep_encoder=False),
               dict(n_intercepts=2), dict(feature_groups=[(0, 10), (10, 27)]), dict(fixed_corr=["positive", "n/a"])):
        assert not ok(**kw).fused_eligible(16, dim_in=27), kw
    m = ok()
    m.fit_dtype = torch.float64
    assert not m.fused_eligible(16, dim_in=27)
    big = dict(cfg, K=dn.DC_KMAX + 1, sup=2)
    assert not C.build(big, "cuda", "unused").fused_eligible(16, dim_in=27)
    assert C.build(dict(cfg, K=dn.DC_KMAX), "cuda", "unused").fused_eligible(16, dim_in=27)
    assert not ok().fused_eligible(16, dim_in=2000)  # the staged rows of X exceed the LDS
    # the restated LDS formula is the library's
    for shape in ((27, 33, 3, 2, 16), (500, 256, 5, 5, 128), (996, 256, 8, 8, 128), (997, 256, 8, 8, 128), (135, 70, 4, 4, 34),
                  (27, 33, 9, 2, 16), (27, 33, 3, 4, 16), (27, 33, 3, 2, 129)):
        assert dn.dcsfa_lds_floats(*shape) == dn.dcsfa_supported(*shape), shape
    monkeypatch.setenv("REDCLIFF_DCSFA_PATH", "triton")
    with pytest.raises(ValueError):
        dn.dcsfa_path()


def test_threshold_gc_is_an_integer_array_and_dirspec_unflattens(runs):
    m, _, _ = runs["a"]
    g = m.GC(threshold=True)
    assert len(g) == 3 and all(x.dtype.kind == "i" and x.shape == (3, 3) and set(np.unique(x)) <= {0, 1} for x in g)
    mb, _, _ = runs["b"]
    gb = mb.GC(threshold=False, ignore_features=False)
    assert len(gb) == 4 and gb[0].shape == (5, 5, 3)
    from redcliff_amd.dcsfa_nmf import unflatten_directed_spectrum_features
    n, f = 3, 2
    # one entry of node 1's block at a time: its row of feature 0, then column 1 above and below the
    # diagonal of feature 1 (a feature's block is 2n - 1 = 5 long: n row entries, n - 1 column entries)
    for col, where in ((0, (1, 0, 0)), (2, (1, 2, 0)), (5 + 3, (0, 1, 1)), (5 + 3 + 1, (2, 1, 1))):
        flat = np.zeros((n, f * (2 * n - 1)))
        flat[1, col] = 1.0
        x = unflatten_directed_spectrum_features(flat)
        assert x.shape == (n, n, f) and x[where] == 1.0 and x.sum() == 1.0, (col, where)


def test_one_row_batches_and_single_class_labels_raise_before_any_step(tmp_path):
    fx = C.fixture("c")
    cfg = fx["cfg"]
    m = C.build(cfg, "cpu", tmp_path)
    C.fixed_nmf(m, fx["nmf/W_nmf"])
    with pytest.raises(ValueError, match="one row"):
        m.fit(fx["X"][:33], fx["y"][:33], n_epochs=1, n_pre_epochs=1, batch_size=16)
    assert not hasattr(m, "encoder")  # nothing was initialised, no step ran
    y1 = np.full_like(fx["y"], 0.9)
    with pytest.raises(ValueError, match="Only one class"):
        m.fit(fx["X"], y1, n_epochs=1, n_pre_epochs=1, batch_size=16)
    with pytest.raises(ValueError, match="Only one class"):
        m.fit(fx["X"], fx["y"], n_epochs=1, n_pre_epochs=1, batch_size=16, X_val=fx["X_val"], y_val=np.zeros_like(fx["y_val"]))


def test_reload_reads_the_written_path_and_load_last_epoch(runs):
    """save_folder has no trailing separator: both classes reload from where the file was written."""
    m, log, folder = runs["a"]
    assert not str(folder).endswith("/")
    best = int(m.best_epoch)
    C.assert_state(C.state(m), log["epochs"][best], 0, "the best epoch's parameters")
    keep = C.state(m)
    m.load_last_epoch()
    C.assert_state(C.state(m), log["epochs"][-1], 0, "the last epoch's parameters")
    m.load_state_dict(dict((k, torch.as_tensor(v)) for k, v in keep.items()))


def test_dirspec_class_whole_fit_reloads_its_module_file(tmp_path):
    """models/dcsfa_nmf.py saves the whole module as the best-model file; ours reloads it."""
    fx = C.fixture("b")
    cfg = fx["cfg"]
    m = C.build(cfg, "cpu", tmp_path)
    C.fixed_nmf(m, fx["nmf/W_nmf"])
    torch.manual_seed(cfg["seed"])
    m.fit(fx["X"], fx["y"], y_pred_weights=fx["pw"], task_mask=fx["tm"], n_epochs=2, n_pre_epochs=1, batch_size=cfg["B"],
          X_val=fx["X"][:40], y_val=fx["y"][:40])
    import os
    best = torch.load(os.path.join(str(tmp_path), "dCSFA-NMF-best-model.pt"), weights_only=False)
    assert isinstance(best, torch.nn.Module)
    C.assert_state(C.state(m), C.state(best), 0, "reloaded")


def test_get_model_gc_estimates_branch(runs):
    from redcliff_amd import evaluation as E
    m, _, _ = runs["c"]
    got = E.get_model_gc_estimates(m, "DCSFANMF", 3)
    want = m.GC(threshold=False, ignore_features=True)
    assert len(got) == 3
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_score_and_predict_shapes(runs):
    m, _, _ = runs["a"]
    fx = C.fixture("a")
    labels = (fx["y_val"] >= 0.6).astype(np.float64)
    s = m.score(fx["X_val"], labels)
    assert s.shape == (2,) and np.all((s >= 0) & (s <= 1))
    assert m.predict(fx["X_val"]).dtype == bool and m.project(fx["X_val"]).shape == (20, 3)
    assert m.reconstruct(fx["X_val"], component=1).shape == fx["X_val"].shape


def test_new_kernels_use_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    for key in NEW_KERNELS:
        hits = [(n, v) for n, v in ks.items() if key in n]
        assert hits, "kernel %s not in the library" % key
        for n, v in hits:
            assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])
