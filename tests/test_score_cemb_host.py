"""CPU-side checks of recording scoring for cEmbedder models (redcliff_amd.scoring,
csrc/rc_score_cemb.hip): the reference fixture tests/golden/cemb_recording_scores.npz against the
oracle embedder, the argument and limit checks of the new C entries, the predicate, the packed
parameter copy and the compiled kernel's resource metadata.  No kernel is launched."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from golden_io import GOLDEN, assert_close
from test_cemb_host import cpu_model
from test_kernel_occupancy import _kernels

RTOL, ATOL = 1e-4, 1e-5


def load_cemb_scenario(name):
    d = np.load(os.path.join(GOLDEN, "cemb_recording_scores.npz"), allow_pickle=False)
    pre = name + "/"
    meta = json.loads(str(d[pre + "meta"]))
    st = dict((k[len(pre + "state/"):], torch.from_numpy(d[k])) for k in d.files if k.startswith(pre + "state/"))
    return meta, st, d[pre + "recording"], d[pre + "weightings"], d[pre + "classifications"]


def oracle_cembedder(meta, st):
    from oracle.redcliff_oracle import OCEmbedder
    emb = OCEmbedder(meta["p"], meta["nsup"], meta["K"], meta["sigmoid"], 10.0, meta["F"], [meta["eh"]])
    emb.load_state_dict(st)
    emb.eval()
    return emb


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_oracle_cembedder_reproduces_the_fixture(name):
    meta, st, rec, wts, cls = load_cemb_scenario(name)
    emb = oracle_cembedder(meta, st)
    F, steps, nsup = meta["F"], meta["num_timesteps_to_score"], meta["nsup"]
    assert meta["num_timesteps_in_input_history"] == F and wts.shape == cls.shape == (nsup, steps)
    assert wts.dtype == cls.dtype == np.float64
    X = torch.from_numpy(rec[0])
    win = X.unfold(0, F, 1)[:steps].transpose(1, 2).contiguous()  # (steps, F, p): window i = rows [i, i + F), time-major
    with torch.no_grad():
        w, logits = emb(win)
    assert_close(name + "/weightings", w[:, :nsup].numpy().T, wts, RTOL, ATOL)
    assert_close(name + "/classifications", logits[:, :nsup].numpy().T, cls, RTOL, ATOL)
    if meta["sigmoid"]:
        assert np.abs(wts - cls).max() > 1e-2  # class scores are not the weightings under the restriction
    if meta["p"] == F:  # the cEmbedder has no p == F rule: the transposed reading is a different function
        with torch.no_grad():
            wt, _ = emb(win.transpose(1, 2).contiguous())
        assert np.abs(wt[:, :nsup].numpy().T - wts).max() > 1e-3


def cemb_score_dims(p=10, K=4, F=16, nsup=4):
    from redcliff_amd import _native as nat
    return nat.Dims(R=1, Bmax=1, T=F, p=p, L=1, K=K, h=1, F=F, n=1, H=1, M1=1, nsup=nsup, use_sigmoid=0,
                    sigmoid_ecc=0.0)


def cemb_score_args(d, eh=25, **kw):
    """Arguments with dummy non-null pointers: every case below must be rejected (or return 0 for
    count == 0) before anything is dereferenced or launched."""
    from redcliff_amd import _native as nat
    a = nat.CEmbScoreArgs()
    a.d = d
    a.eh = eh
    for f in ("emb", "X", "w", "logits"):
        setattr(a, f, 64)
    a.Nrec, a.T, a.x_rstride = 1, 100, 0
    a.start, a.count, a.stride, a.use_final_activation = d.F, 10, 1, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_cemb_score_entry_argument_and_limit_checks():
    from redcliff_amd import _native as nat
    L = nat.lib()
    d = cemb_score_dims()
    call = lambda a: L.redcliff_cemb_score_recording(ctypes.byref(a), None)
    sup = lambda dd, eh: L.redcliff_cemb_score_supported(ctypes.byref(dd), eh)
    # the query returns the rows one tile may stage: (40960 - 4096) / p
    assert sup(d, 25) == 3686
    # limits: the query returns 0 with a message, the entry REDCLIFF_ELIMIT
    for field, value in (("p", 65), ("F", 65), ("K", 17), ("eh", 129)):
        bad, eh = cemb_score_dims(), 25
        if field == "eh":
            eh = value
        else:
            setattr(bad, field, value)
        assert sup(bad, eh) == 0, field
        assert b"limits" in L.redcliff_last_error()
        assert call(cemb_score_args(bad, eh)) == -2, field
    # Bmax and the factor dimensions are irrelevant
    d2 = cemb_score_dims()
    d2.Bmax, d2.h, d2.L, d2.T, d2.n, d2.H, d2.M1 = 100000, 4096, 999, 1, 9, 9000, 900
    assert sup(d2, 25) == 3686
    # the top of the limits is accepted
    top = cemb_score_dims(p=64, K=16, F=64, nsup=0)
    assert sup(top, 128) == 576
    assert call(cemb_score_args(top, 128, logits=None, count=0, start=64)) == 0
    # invalid arguments (the list of redcliff_score_recording's test, for the fields this entry has)
    assert L.redcliff_cemb_score_recording(None, None) == -1
    for kw in (dict(start=d.F - 1), dict(stride=0), dict(count=-1), dict(count=86), dict(start=20, count=82),
               dict(stride=4, count=23), dict(emb=None), dict(X=None), dict(w=None), dict(logits=None),
               dict(graphs=64, tab=None, Q=9), dict(graphs=64, tab=64, Q=0), dict(Nrec=0), dict(eh=0)):
        assert call(cemb_score_args(d, **kw)) == -1, kw
        assert L.redcliff_last_error()
    bad = cemb_score_dims()
    bad.nsup = 5  # more supervised factors than factors
    assert call(cemb_score_args(bad)) == -1
    # the last window may end exactly at T; count == 0 launches nothing and returns 0
    assert call(cemb_score_args(d, count=0)) == 0
    assert call(cemb_score_args(d, start=100, count=0)) == 0
    nosup = cemb_score_dims(nsup=0)
    assert call(cemb_score_args(nosup, logits=None, count=0)) == 0  # logits may be null without supervised factors


def test_score_cemb_is_a_kernel_id_after_the_existing_ones():
    from redcliff_amd import _native as nat
    assert nat.KERNEL_IDS[-3:] == ("score", "score_graphs", "score_cemb") and nat.KERNEL_IDS.index("score") == 9
    assert nat.ABI_VERSION == 10


def test_new_kernel_uses_no_scratch(tmp_path):
    ks = _kernels(str(tmp_path))
    hits = [(n, v) for n, v in ks.items() if "k_score_cemb" in n]
    assert hits, "kernel k_score_cemb not in the library"
    for n, v in hits:
        assert v["scratch"] == 0, "%s: %d bytes of scratch" % (n, v["scratch"])


def _model(F=4, lag=None, hidden=(5,), wavelet_level=None, p=6, num_sims=1):
    import redcliff_amd
    from oracle.redcliff_oracle import reference_coeffs
    K, L = 3, 3
    eargs = [("sigmoid_eccentricity_coeff", 10.0), ("lag", F if lag is None else lag), ("hidden", list(hidden))]
    torch.manual_seed(3)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(
        p, L, [8], F, [0], L, 1, K, 2, reference_coeffs(K, p), False, "cEmbedder", eargs,
        "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion", num_sims=num_sims,
        wavelet_level=wavelet_level, training_mode="combined").float()


def test_predicate():
    from redcliff_amd import scoring
    ok = _model()
    assert scoring.cemb_config_supported(ok)
    assert not scoring.cemb_fused_available(ok)  # parameters on the CPU
    # only the embedder matters: a model outside cembedder_fused_supported() still qualifies
    two = _model(num_sims=2)
    assert not two.cembedder_fused_supported() and scoring.cemb_config_supported(two)
    for bad in (_model(wavelet_level=3, p=2), _model(hidden=(5, 4)), _model(lag=3)):
        assert not scoring.cemb_config_supported(bad) and not scoring.cemb_fused_available(bad)
    # a DGCNN model is not this route's
    eargs = [("num_features_per_node", 7), ("num_graph_conv_layers", 3), ("num_hidden_nodes", 5),
             ("sigmoid_eccentricity_coeff", 10.0)]
    import redcliff_amd
    from oracle.redcliff_oracle import reference_coeffs
    dg = redcliff_amd.REDCLIFF_S_CMLP(5, 3, [6], 7, [0], 3, 1, 3, 2, reference_coeffs(3, 5), False, "DGCNN", eargs,
                                      "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion",
                                      training_mode="combined")
    assert not scoring.cemb_config_supported(dg)


def test_packed_copy_equals_the_engine_layout():
    from redcliff_amd import cemb_engine as ce
    from redcliff_amd import scoring
    K, eh, p, F = 3, 5, 6, 4
    m = cpu_model(eh=eh, p=p, K=K, F=F)
    emb = m.factor_score_embedder
    rng = np.random.RandomState(0)
    with torch.no_grad():
        for prm in emb.parameters():
            prm.add_(torch.from_numpy(rng.randn(*prm.shape).astype(np.float32)))
    before = [prm.detach().clone() for prm in emb.parameters()]
    flat = scoring.cemb_packed(emb)
    o = ce.cemb_layout(K, eh, p, F)
    assert flat.shape == (o["total"],) and flat.dtype == torch.float32 and not flat.requires_grad
    want = torch.full((o["total"],), float("nan"))
    for prm, view in ce.cemb_views(want, list(emb.networks), eh, p, F):
        view.copy_(prm.detach())
    assert torch.equal(flat, want)
    # a private copy: writing to it leaves the module parameters alone, and nothing was re-pointed
    ptrs = [prm.data_ptr() for prm in emb.parameters()]
    flat.zero_()
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, emb.parameters()))
    assert ptrs == [prm.data_ptr() for prm in emb.parameters()]
