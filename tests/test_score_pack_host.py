"""CPU-side checks of scoring recordings with many models in one launch chain
(redcliff_score_recording_pack, redcliff_amd.scoring.score_recordings): the argument and limit
checks of the new C entries, the kernel-timing ids and ABI version they must leave alone, the Python
argument checks, and the compiled kernels' resource metadata.  No kernel is launched."""
import ctypes

import pytest
import torch

from test_kernel_occupancy import _kernels
from test_score_recording_host import score_dims


def pack_args(d, R=3, **kw):
    """Arguments with dummy non-null pointers: every case below must be rejected (or return 0 when
    nothing is to be scored) before anything is dereferenced or launched."""
    from redcliff_amd import _native as nat
    a = nat.ScorePackArgs()
    a.d, a.R = d, R
    for f in ("emb", "bn_rm", "bn_rv", "X", "w", "logits", "ws"):
        setattr(a, f, 64)
    a.emb_stride, a.bn_stride, a.x_pstride = 100000, d.F, 0
    a.bn_eps = 1e-5
    a.Nrec, a.T, a.x_rstride = 1, 100, 0
    a.start, a.count, a.stride, a.use_final_activation = d.F, 10, 1, 1
    a.ws_bytes = nat.lib().redcliff_score_recording_pack_workspace_bytes(ctypes.byref(d), max(min(R, 256), 1))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def replica_list(*idx):
    arr = (ctypes.c_int32 * max(len(idx), 1))(*idx)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_pack_entry_argument_and_limit_checks():
    from redcliff_amd import _native as nat
    L = nat.lib()
    d = score_dims()
    single = L.redcliff_score_recording_workspace_bytes(ctypes.byref(d))
    query = lambda dd, R: L.redcliff_score_recording_pack_workspace_bytes(ctypes.byref(dd), R)
    call = lambda a: L.redcliff_score_recording_pack(ctypes.byref(a), None)

    def rejected(a, code, what):
        assert call(a) == code, what
        assert L.redcliff_last_error(), what

    # the workspace: R times the single call's; 0 outside the limits, with a message
    for R in (1, 3, 128, 256):
        assert query(d, R) == R * single
    for R in (0, -1, 257):
        assert query(d, R) == 0 and L.redcliff_last_error()
    for field, value in (("p", 65), ("F", 65), ("n", 5), ("M1", 65), ("K", 17), ("H", 900)):
        bad = score_dims()
        setattr(bad, field, value)
        if field == "K":
            bad.nsup = 4
        assert query(bad, 3) == 0, field
        assert b"limits" in L.redcliff_last_error()
        rejected(pack_args(bad), -2, field)
    # REDCLIFF_EINVAL
    assert L.redcliff_score_recording_pack(None, None) == -1
    rejected(pack_args(d, R=0), -1, "R = 0")
    rejected(pack_args(d, R=-2), -1, "R < 0")
    for kw in (dict(emb_stride=-1), dict(bn_stride=-1), dict(x_pstride=-1), dict(x_rstride=-1),
               dict(graphs=64, tab=None, Q=9), dict(graphs=64, tab=64, Q=0),
               dict(start=d.F - 1), dict(stride=0), dict(count=-1), dict(count=86), dict(start=20, count=82),
               dict(stride=4, count=23), dict(emb=None), dict(bn_rm=None), dict(bn_rv=None), dict(X=None), dict(w=None),
               dict(logits=None), dict(ws=None), dict(Nrec=0)):
        rejected(pack_args(d, **kw), -1, kw)
    # the active list: strictly increasing indices < R, at most R of them
    for idx, n in (((1, 1), 2), ((2, 1), 2), ((0, 3), 2), ((-1, 1), 2), ((0, 1, 2, 2), 4), ((0,), -1)):
        keep, ptr = replica_list(*idx)
        rejected(pack_args(d, replicas=ptr, n_replicas=n), -1, idx)
    # REDCLIFF_ELIMIT
    rejected(pack_args(d, R=257), -2, "R = 257")
    rejected(pack_args(d, Nrec=65536), -2, "Nrec = 65536")
    # REDCLIFF_EWORKSPACE: one float short of R slices, or sized for fewer replicas
    rejected(pack_args(d, ws_bytes=3 * single - 4), -3, "short workspace")
    rejected(pack_args(d, R=4, ws_bytes=3 * single), -3, "workspace of 3 replicas for 4")
    # nothing to score: 0 without a launch
    assert call(pack_args(d, count=0)) == 0
    keep, ptr = replica_list()
    assert call(pack_args(d, replicas=ptr, n_replicas=0)) == 0
    nosup = score_dims(nsup=0)
    assert call(pack_args(nosup, logits=None, count=0)) == 0  # logits may be null without supervised factors
    # a valid list and the top of R pass the checks (count == 0: still nothing is launched)
    keep, ptr = replica_list(0, 2)
    assert call(pack_args(d, replicas=ptr, n_replicas=2, count=0)) == 0
    assert call(pack_args(d, R=256, count=0, Nrec=65535)) == 0


def test_kernel_ids_and_abi_version_are_unchanged():
    from redcliff_amd import _native as nat
    assert nat.ABI_VERSION == 10 and nat.lib().redcliff_abi_version() == 10
    assert nat.KERNEL_IDS == ("supports", "emb_fwd", "fac_fwd", "fac_bwd", "emb_bwd", "emb_final", "fac_mix",
                              "emb_combine", "fac_lead", "score", "score_graphs", "score_cemb")
    assert "redcliff_score_recording_pack" in nat.EXPORTED
    assert "redcliff_score_recording_pack_workspace_bytes" in nat.EXPORTED
    # the library's own count of ids (its return value) matches
    n = len(nat.KERNEL_IDS)
    ms, cnt = (ctypes.c_double * n)(), (ctypes.c_int64 * n)()
    assert nat.lib().redcliff_kernel_times(ms, cnt, n) == n


def cpu_models(n=3, K=3, F=7):
    import redcliff_amd
    from oracle.redcliff_oracle import reference_coeffs
    p, L = 5, 3
    eargs = [("num_features_per_node", F), ("num_graph_conv_layers", 3), ("num_hidden_nodes", 5),
             ("sigmoid_eccentricity_coeff", 10.0)]
    out = []
    for s in range(n):
        torch.manual_seed(s)
        out.append(redcliff_amd.REDCLIFF_S_CMLP(p, L, [6], F, [0], L, 1, K, 2, reference_coeffs(K, p), False, "DGCNN",
                                                eargs, "conditional_factor_fixed_embedder",
                                                "apply_factor_weights_after_sim_completion", training_mode="combined"))
    return out, p, F


def test_python_argument_checks_without_a_device():
    import redcliff_amd
    from redcliff_amd import PerReplica, scoring
    assert redcliff_amd.score_recordings is scoring.score_recordings
    models, p, F = cpu_models()
    m0, R = models[0], len(models)
    X = torch.zeros(48, p)
    # the X shape rules: shared (T, p) / (Nrec, T, p), per replica PerReplica / (R, Nrec, T, p)
    Xn, per, start, count, stride = scoring._pack_window_args(m0, X, R, None, None, 1)
    assert Xn.shape == (1, 48, p) and not per and (start, count, stride) == (F, 42, 1)
    Xn, per, _, count, _ = scoring._pack_window_args(m0, torch.zeros(2, 48, p), R, 10, None, 4)
    assert Xn.shape == (2, 48, p) and not per and count == 10
    Xn, per, _, count, _ = scoring._pack_window_args(m0, PerReplica([X] * R), R, None, 5, 2)
    assert Xn.shape == (R, 1, 48, p) and per and count == 5
    Xn, per, _, count, _ = scoring._pack_window_args(m0, torch.zeros(R, 2, 48, p), R, None, None, 1)
    assert Xn.shape == (R, 2, 48, p) and per and count == 42
    bad_X = (PerReplica([X] * (R - 1)), PerReplica([X] * (R + 1)), PerReplica([X, X, torch.zeros(47, p)]),
             PerReplica([X, X, torch.zeros(48, p + 1)]), torch.zeros(R + 1, 2, 48, p), torch.zeros(R, 2, 48, p + 1),
             torch.zeros(48, p + 1), torch.zeros(1, R, 2, 48, p))
    for bad in bad_X:
        with pytest.raises(ValueError):
            scoring._pack_window_args(m0, bad, R, None, None, 1)
        with pytest.raises(ValueError):
            scoring.score_recordings(models, bad)
    for kw in (dict(start=F - 1), dict(stride=0), dict(count=-1), dict(count=43), dict(start=49, count=1)):
        with pytest.raises(ValueError):
            scoring.score_recordings(models, X, **kw)
        with pytest.raises(ValueError):
            scoring.score_recordings(models, PerReplica([X] * R), **kw)
    # graphs / mode validation, as score_recording (which keeps raising)
    with pytest.raises(ValueError):
        scoring.score_recordings(models, X, graphs="mean")
    with pytest.raises(ValueError):
        scoring.score_recordings(models, X, graphs="sum", gc_est_mode="fixed_factor_exclusive")
    with pytest.raises(ValueError):
        m0.score_recording(X, graphs="mean")
    # lists whose results could not be stacked, and the empty list
    with pytest.raises(ValueError):
        scoring.score_recordings(models[:2] + cpu_models(1, K=4)[0], X)
    with pytest.raises(ValueError):
        scoring.score_recordings([], X)
    # the active list of a pack
    assert scoring._active_indices(None, 3) == [0, 1, 2] and scoring._active_indices([2, 0], 3) == [0, 2]
    assert scoring._active_indices([], 3) == []
    for bad in ([3], [-1], [1, 1]):
        with pytest.raises(ValueError):
            scoring._active_indices(bad, 3)
    # models on the host are not for the packed kernel
    assert not scoring.pack_available(models) and not scoring.pack_available([])


def test_pack_graph_tables_restate_graph_tables():
    """The stacked tables are graph_tables' element-wise operations: same values for every mode."""
    from redcliff_amd import scoring
    R, K, p, L, F = 2, 3, 4, 3, 5
    g = torch.Generator().manual_seed(0)
    G = torch.rand(R, K, p, p, L, generator=g)
    G0 = torch.rand(R, K, p, p, generator=g)
    A = torch.randn(R, p, p, generator=g)
    ls = min(L, F)
    for mode in scoring.GRAPH_MODES:
        for ign in (True, False):
            tab, bias = scoring.pack_graph_tables(G, G0, A, mode, ign, ls)
            for r in range(R):
                fg = G0[r].view(K, p, p, 1) if ign else G[r]
                if mode == scoring.GRAPH_MODES[0]:
                    assert bias is None and torch.equal(tab[r], fg)
                    continue
                eg = A[r].T.reshape(p, p, 1)
                if not ign:
                    fg, eg = fg[..., -ls:], eg[:, :, -ls:]
                assert torch.equal(tab[r], fg) and torch.equal(bias[r], (float(K) * eg).expand(fg.shape[1:]))


def test_score_kernels_use_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    hits = [(n, v) for n, v in ks.items() if "k_score_" in n]
    assert len(hits) >= 4, "the scoring kernels are not in the library: %s" % [n for n, _ in hits]
    for n, v in hits:
        assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])
