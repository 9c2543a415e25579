"""CPU-side checks of recording scoring (redcliff_amd.scoring, csrc/rc_score.hip): the reference
fixture tests/golden/recording_scores.npz against the oracle embedder, the argument and limit
checks of the new C entries, and the compiled kernels' resource metadata.  No kernel is launched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, assert_close
from test_kernel_occupancy import _kernels

NEW_KERNELS = ["k_score_tables", "k_score_windows", "k_score_graphs"]


def load_scenario(name):
    d = np.load(os.path.join(GOLDEN, "recording_scores.npz"), allow_pickle=False)
    pre = name + "/"
    meta = json.loads(str(d[pre + "meta"]))
    st = dict((k[len(pre + "state/"):], torch.from_numpy(d[k])) for k in d.files if k.startswith(pre + "state/"))
    return meta, st, d[pre + "recording"], d[pre + "weightings"], d[pre + "classifications"]


def oracle_embedder(meta, st):
    from oracle.redcliff_oracle import ODGCNNEmbedder
    emb = ODGCNNEmbedder(meta["p"], meta["F"], meta["n"], meta["H"], 10.0, meta["sigmoid"], meta["K"], meta["nsup"])
    emb.load_state_dict(st)
    emb.eval()
    return emb


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_oracle_embedder_reproduces_the_fixture(name):
    meta, st, rec, wts, cls = load_scenario(name)
    emb = oracle_embedder(meta, st)
    F, steps, nsup = meta["F"], meta["num_timesteps_to_score"], meta["nsup"]
    assert meta["num_timesteps_in_input_history"] == F and wts.shape == cls.shape == (nsup, steps)
    assert wts.dtype == cls.dtype == np.float64
    X = torch.from_numpy(rec[0])
    win = X.unfold(0, F, 1)[:steps]  # (steps, p, F): window i = rows [i, i + F) as nodes x features
    if meta["p"] == F:
        # the reference passes (1, F, p) time-major slices, and at p == F the embedder does not
        # transpose them (models/redcliff_factor_score_embedders.py:369-371): feed them untransposed
        win = win.transpose(1, 2)
    with torch.no_grad():
        w, logits = emb(win.contiguous())
    assert_close(name + "/weightings", w[:, :nsup].numpy().T, wts, 1e-4, 1e-5)
    assert_close(name + "/classifications", logits[:, :nsup].numpy().T, cls, 1e-4, 1e-5)
    if meta["sigmoid"]:
        assert np.abs(wts - cls).max() > 1e-2  # class scores are not the weightings under the restriction
    if meta["p"] == F:  # and the transposed reading is a different function (the fixture tells them apart)
        with torch.no_grad():
            wt, _ = emb(win.transpose(1, 2).contiguous())
        assert np.abs(wt[:, :nsup].numpy().T - wts).max() > 1e-3


def score_dims(p=10, K=4, F=16, n=3, H=100, M1=64, nsup=4):
    from redcliff_amd import _native as nat
    return nat.Dims(R=1, Bmax=1, T=F, p=p, L=1, K=K, h=1, F=F, n=n, H=H, M1=M1, nsup=nsup, use_sigmoid=0,
                    sigmoid_ecc=0.0)


def score_args(d, **kw):
    """Arguments with dummy non-null pointers: every case below must be rejected (or return 0 for
    count == 0) before anything is dereferenced or launched."""
    from redcliff_amd import _native as nat
    a = nat.ScoreArgs()
    a.d = d
    for f in ("emb", "bn_rm", "bn_rv", "X", "w", "logits", "ws"):
        setattr(a, f, 64)
    a.bn_eps = 1e-5
    a.Nrec, a.T, a.x_rstride = 1, 100, 0
    a.start, a.count, a.stride, a.use_final_activation = d.F, 10, 1, 1
    a.ws_bytes = nat.lib().redcliff_score_recording_workspace_bytes(ctypes.byref(d))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_score_entry_argument_and_limit_checks():
    from redcliff_amd import _native as nat
    L = nat.lib()
    d = score_dims()
    nbytes = L.redcliff_score_recording_workspace_bytes(ctypes.byref(d))
    # S[n][p][p] | Wf[n][F][H] | Zb[p][H], each rounded up to 64 floats
    assert nbytes == 4 * (320 + 4800 + 1024)
    call = lambda a: L.redcliff_score_recording(ctypes.byref(a), None)
    # limits: the size query returns 0 with a message, the entry REDCLIFF_ELIMIT
    for field, value in (("p", 65), ("F", 65), ("n", 5), ("M1", 65), ("K", 17), ("H", 900)):
        bad = score_dims()
        setattr(bad, field, value)
        if field == "K":
            bad.nsup = 4
        assert L.redcliff_score_recording_workspace_bytes(ctypes.byref(bad)) == 0, field
        assert b"limits" in L.redcliff_last_error()
        assert call(score_args(bad)) == -2, field
    # the kernel's own LDS budget: n*F*H tables beside the staged rows
    bad = score_dims(p=64, F=64, n=4, H=128)
    assert L.redcliff_score_recording_workspace_bytes(ctypes.byref(bad)) == 0 and b"LDS" in L.redcliff_last_error()
    assert call(score_args(bad)) == -2
    # Bmax and the factor dimensions are irrelevant
    d2 = score_dims()
    d2.Bmax, d2.h, d2.L, d2.T = 100000, 4096, 999, 1
    assert L.redcliff_score_recording_workspace_bytes(ctypes.byref(d2)) == nbytes
    # the top of the limits is accepted
    assert L.redcliff_score_recording_workspace_bytes(ctypes.byref(score_dims(p=64, K=8, F=64, H=100, nsup=0))) > 0
    # invalid arguments
    assert L.redcliff_score_recording(None, None) == -1
    for kw in (dict(start=d.F - 1), dict(stride=0), dict(count=-1), dict(count=86), dict(start=20, count=82),
               dict(stride=4, count=23), dict(emb=None), dict(bn_rm=None), dict(bn_rv=None), dict(X=None), dict(w=None),
               dict(logits=None), dict(ws=None), dict(graphs=64, tab=None, Q=9), dict(graphs=64, tab=64, Q=0),
               dict(Nrec=0)):
        assert call(score_args(d, **kw)) == -1, kw
        assert L.redcliff_last_error()
    assert call(score_args(d, ws_bytes=nbytes - 4)) == -3
    bad = score_dims()
    bad.nsup = 5  # more supervised factors than factors
    assert call(score_args(bad)) == -1
    # the last window may end exactly at T; count == 0 launches nothing and returns 0
    assert call(score_args(d, count=0)) == 0
    assert call(score_args(d, start=100, count=0)) == 0
    nosup = score_dims(nsup=0)
    assert call(score_args(nosup, logits=None, count=0)) == 0  # logits may be null without supervised factors


def test_python_argument_checks():
    import redcliff_amd
    from redcliff_amd import scoring
    from oracle.redcliff_oracle import reference_coeffs
    p, L, K, F = 5, 3, 3, 7
    eargs = [("num_features_per_node", F), ("num_graph_conv_layers", 3), ("num_hidden_nodes", 5),
             ("sigmoid_eccentricity_coeff", 10.0)]
    m = redcliff_amd.REDCLIFF_S_CMLP(p, L, [6], F, [0], L, 1, K, 2, reference_coeffs(K, p), False, "DGCNN", eargs,
                                     "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion",
                                     training_mode="combined")
    assert callable(m.score_recording)  # inherited by REDCLIFF_S_CMLP
    X = torch.zeros(48, p)
    _, start, count, stride = scoring._window_args(m, X, None, None, 1)
    assert (start, count, stride) == (F, 42, 1)  # every step that fits: the last window ends at T
    assert scoring._window_args(m, X, 10, None, 4)[2] == 10
    assert scoring._window_args(m, X.unsqueeze(0).expand(3, 48, p), None, 5, 2)[0].shape == (3, 48, p)
    for kw in (dict(start=F - 1), dict(stride=0), dict(count=-1), dict(count=43), dict(start=49, count=1)):
        args = dict(start=None, count=None, stride=1)
        args.update(kw)
        with pytest.raises(ValueError):
            scoring._window_args(m, X, args["start"], args["count"], args["stride"])
    with pytest.raises(ValueError):
        scoring._window_args(m, torch.zeros(48, p + 1), None, None, 1)
    with pytest.raises(ValueError):
        m.score_recording(X, graphs="mean")
    with pytest.raises(ValueError):
        m.score_recording(X, graphs="sum", gc_est_mode="fixed_factor_exclusive")


def test_new_kernels_use_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    for key in NEW_KERNELS:
        hits = [(n, v) for n, v in ks.items() if key in n]
        assert hits, "kernel %s not in the library" % key
        for n, v in hits:
            assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])
