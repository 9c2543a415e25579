"""CPU-side checks of the fused cEmbedder path (redcliff_amd.cemb_engine, csrc/rc_cemb.hip): the
packed parameter layout, the predicate and the library's limit check, the workspace regions, and
the compiled kernels' resource metadata.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

from test_kernel_occupancy import _kernels

NEW_KERNELS = ["k_cemb_fwd", "k_cemb_tables", "k_cemb_bwd", "k_fac_mixILi128ELb1E", "k_fac_mixILi256ELb1E"]


def cpu_model(eh=5, num_sims=1, p=6, L=3, K=3, F=4, h=8, mode="pretrain_embedder_then_acclimate_factors_then_combined"):
    import redcliff_amd
    from oracle.redcliff_oracle import reference_coeffs
    eargs = [("sigmoid_eccentricity_coeff", 10.0), ("lag", F), ("hidden", [eh])]
    torch.manual_seed(3)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(
        p, L, [h], F, [0], L, 1, K, 2, reference_coeffs(K, p), False, "cEmbedder", eargs,
        "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion", num_sims=num_sims,
        training_mode=mode, num_pretrain_epochs=1, num_acclimation_epochs=1).float()


def test_packed_layout_matches_parameters_order_and_round_trips():
    from redcliff_amd import _native as nat
    from redcliff_amd import cemb_engine as ce
    K, eh, p, F = 3, 5, 6, 4
    m = cpu_model(eh=eh, p=p, K=K, F=F)
    emb = m.factor_score_embedder
    o = ce.cemb_layout(K, eh, p, F)
    total = K * eh * p * F + K * eh + K * eh + K
    assert o["total"] == total and [o[k] for k in ("We0", "be0", "We1", "be1")] == [0, K * eh * p * F, K * eh * p * F + K * eh,
                                                                                     K * eh * p * F + 2 * K * eh]
    d = ce.model_dims(m)
    assert nat.lib().redcliff_cemb_param_count(ctypes.byref(d), eh) == total
    flat = torch.full((total,), float("nan"))
    pairs = ce.cemb_views(flat, list(emb.networks), eh, p, F)
    params = list(emb.parameters())
    assert len(pairs) == len(params) == 4 * K
    assert all(a is b for (a, _), b in zip(pairs, params))  # parameters() order
    for prm, view in pairs:
        assert view.shape == prm.shape
        view.copy_(prm.detach())
    assert not torch.isnan(flat).any()  # the views tile the buffer: every float belongs to one parameter
    assert sum(prm.numel() for prm in params) == total
    for prm, view in pairs:
        np.testing.assert_array_equal(view.numpy(), prm.detach().numpy())
    # grouped by tensor kind: We0 of network k at We0 + k * eh*p*F in Conv1d order q = c*F + t
    W = torch.stack([net.layers[0].weight.detach() for net in emb.networks])
    np.testing.assert_array_equal(flat[:o["be0"]].numpy(), W.reshape(-1).numpy())
    np.testing.assert_array_equal(flat[o["be1"]:].numpy(),
                                  torch.cat([net.layers[1].bias.detach() for net in emb.networks]).numpy())


def test_predicate_and_library_limits_agree():
    from redcliff_amd import _native as nat
    from redcliff_amd import cemb_engine as ce
    m = cpu_model()
    assert m.cembedder_fused_supported() and m.cembedder_fused_supported(512) and not m.fused_supported()
    assert not cpu_model(num_sims=2).cembedder_fused_supported()
    assert not cpu_model(eh=129).cembedder_fused_supported()
    assert cpu_model(eh=128).cembedder_fused_supported()
    assert not cpu_model(L=5, F=4).cembedder_fused_supported()  # embed_lag < gen_lag
    assert not m.cembedder_fused_supported(513)
    L = nat.lib()
    d = ce.model_dims(m, 16)
    assert L.redcliff_cemb_workspace_bytes(ctypes.byref(d), 5) > 0
    assert L.redcliff_cemb_workspace_bytes(ctypes.byref(d), 129) == 0 and b"limits" in L.redcliff_last_error()
    d.p = 65
    assert L.redcliff_cemb_workspace_bytes(ctypes.byref(d), 5) == 0
    # the step entry refuses the same shapes, and the flags it does not implement
    a = nat.StepArgs()
    a.d = ce.model_dims(m, 16)
    a.B = 16
    x = nat.CEmbArgs(eh=129)
    assert L.redcliff_cemb_train_step(ctypes.byref(a), ctypes.byref(x), None) == -2
    x.eh = 5
    a.flags = nat.GRAD_ONLY
    assert L.redcliff_cemb_train_step(ctypes.byref(a), ctypes.byref(x), None) == -1
    a.flags = nat.REFRESH_SUPPORTS
    assert L.redcliff_cemb_train_step(ctypes.byref(a), ctypes.byref(x), None) == -1
    a.flags = 0
    assert L.redcliff_cemb_train_step(ctypes.byref(a), ctypes.byref(x), None) == -1 and b"null" in L.redcliff_last_error()


def test_env_variable_values(monkeypatch):
    from redcliff_amd import cemb_engine as ce
    monkeypatch.delenv(ce.ENV, raising=False)
    assert ce.path_requested() == "generic"
    for v, want in (("generic", "generic"), ("fused", "fused"), ("", "generic")):
        monkeypatch.setenv(ce.ENV, v)
        assert ce.path_requested() == want
    monkeypatch.setenv(ce.ENV, "triton")
    with pytest.raises(ValueError):
        ce.path_requested()


def test_cemb_workspace_regions_and_guard_bands():
    from redcliff_amd import _native as nat
    from redcliff_amd import cemb_engine as ce
    m = cpu_model()
    d = ce.model_dims(m, 21)
    K, p, F, Ls, eh, B = 3, 6, 4, 3, 5, 21
    shared = nat.workspace_regions(d)
    plain, total = nat.cemb_workspace_regions(d, eh)
    assert [n for _, n in plain] == [K * B * eh, K * eh, K * p * F, K * p, p * p * Ls, p * p, K * p * p * Ls, B * K]
    assert all(s % 64 == 0 for s, _ in plain) and plain[-1][0] + plain[-1][1] <= total
    assert nat.lib().redcliff_cemb_workspace_bytes(ctypes.byref(d), eh) == 4 * total
    prev = nat.guard_bands(64)
    try:
        regs, gtotal = nat.cemb_workspace_regions(d, eh)
        assert [n for _, n in regs] == [n for _, n in plain]
        for (s, n), (s2, _) in zip(regs, regs[1:]):
            assert s % 64 == 0 and s + n + 64 <= s2
        assert regs[-1][0] + regs[-1][1] + 64 <= gtotal
        assert nat.lib().redcliff_cemb_workspace_bytes(ctypes.byref(d), eh) == 4 * gtotal
    finally:
        nat.guard_bands(prev)
    assert nat.cemb_workspace_regions(d, eh) == (plain, total)
    assert nat.workspace_regions(d) == shared  # the shared layout is untouched


def test_new_kernels_use_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    for key in NEW_KERNELS:
        hits = [(n, v) for n, v in ks.items() if key in n]
        assert hits, "kernel %s not in the library" % key
        for n, v in hits:
            assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])
