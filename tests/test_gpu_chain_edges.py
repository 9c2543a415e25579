"""Partly filled batches, tiles and k-steps of the merged backward's matrix-core chains.

The factor-update chains (activation recompute over Q = p*L, dW0 tile over the B windows;
rc_fac_bwd.h) and the node workgroups' chains (df1 over K, dZ over the fc1 width, dfc1W / dW_i /
dT over 16-window tiles; rc_embed.hip) fetch the operands of a batch of k-steps ahead of the
batch's products, from unconditional reads with zeros selected afterwards.  What can go wrong
there is a batch, a tile or a k-step that is only partly filled, so the shapes below put every
such edge on the single-fit path: Q not a multiple of 4 or of a 16- or 32-column batch (9, 35)
and above one 64-column tile (70: two dW0 column tiles, activations read back instead of
recomputed), B not a multiple of 4, 16 or 32 (5, 37) and the full tile (128), h below one
16-unit chunk (5) and with a partial last chunk (20), K = 1 and K = 5, n*F not a multiple of
16 (10, 27), H below one 16-column chunk (7) and with a partial last chunk (20).

Every shape stays inside the engine's limits (p <= 64, K <= 16, h <= 128, gen_lag <= embed_lag
<= 64, n <= 4, B <= 512) and the merged launch's conditions: vector factor path (p*L < 256),
fused embedder (p < 32), one 16-window sub-block per node workgroup (rc_emb_wpb == rc_emb_bc:
the LDS tiles fit at 16 windows and p * ceil(H / 16) groups need no window blocking), and a
grid of at most 160 workgroups against the 2 x 256 resident slots of rc_bwd_merged_grid -- so
the default run is the merged kernel and REDCLIFF_MERGE=0 (read per step) the two launches.

Per case: three combined-phase steps from a seeded model on seeded windows.  Parameters,
BatchNorm buffers and Adam moments against the CPU oracle at the three-phase tolerance of
tests/test_gpu_parity.py (rtol 2e-4, atol 5e-6 x max(1, max |want|)); merged against two
launches bit for bit; one R = 2 pack against its single fits bit for bit."""
import functools

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_gpu_parity import compare_state, synth

pytestmark = pytest.mark.gpu

RTOL3, ATOL3 = 2e-4, 5e-6  # test_gpu_parity._three_phases_vs_oracle's compare_state arguments

SHAPES = {
    "q9_b5_h5_k1_nf10_h7": dict(p=3, L=3, K=1, h=5, F=5, n=2, H=7, B=5),
    "q35_b37_h20_k5_nf27_h20": dict(p=5, L=7, K=5, h=20, F=9, n=3, H=20, B=37),
    "q9_b128_h20_k5_nf10_h20": dict(p=3, L=3, K=5, h=20, F=5, n=2, H=20, B=128),
    "q35_b128_h5_k1_nf27_h7": dict(p=5, L=7, K=1, h=5, F=9, n=3, H=7, B=128),
    "q70_b37_h20_k2_nf16_h20": dict(p=10, L=7, K=2, h=20, F=8, n=2, H=20, B=37),
}
STEPS = 3
EPOCH = 2  # combined phase (one pretrain and one acclimation epoch before it)


def config(name):
    c = dict(SHAPES[name])
    c.update(nsup=c["K"], T=max(c["L"], c["F"]) + 1, label_T=1)
    return c


def model_args(c):
    from oracle.redcliff_oracle import reference_coeffs
    eargs = [("num_features_per_node", c["F"]), ("num_graph_conv_layers", c["n"]), ("num_hidden_nodes", c["H"]),
             ("sigmoid_eccentricity_coeff", 10.0)]
    args = (c["p"], c["L"], [c["h"]], c["F"], [0], c["L"], 1, c["K"], c["nsup"], reference_coeffs(c["K"], c["p"]), False,
            "DGCNN", eargs, "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion")
    kw = dict(num_sims=1, training_mode="pretrain_embedder_then_acclimate_factors_then_combined", num_pretrain_epochs=1,
              num_acclimation_epochs=1)
    return args, kw


def hip_model(c, seed):
    import redcliff_amd
    args, kw = model_args(c)
    torch.manual_seed(seed)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(*args, **kw).cuda()


def optimizers(m):
    from oracle.redcliff_oracle import make_optimizers
    return make_optimizers(m, 5e-4, 1e-4, 1e-4, 5e-4, 1e-4, 1e-4)


def windows(c, seed=5):
    X, Y = synth(c, STEPS * c["B"], seed=seed)
    return [(X[i:i + c["B"]], Y[i:i + c["B"]]) for i in range(0, X.shape[0], c["B"])]


def snapshot(m, opts):
    """Every state_dict tensor and every Adam moment, as host arrays."""
    torch.cuda.synchronize()
    out = dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())
    for g, o in zip("AB", opts):
        for i, prm in enumerate(o.param_groups[0]["params"]):
            for kk in ("exp_avg", "exp_avg_sq"):
                out["opt%s/%d/%s" % (g, i, kk)] = o.state[prm][kk].detach().cpu().numpy().copy()
    return out


def hip_fit(c, seed=0):
    m = hip_model(c, seed)
    opts = optimizers(m)
    for bi, (Xb, Yb) in enumerate(windows(c)):
        m.batch_update(EPOCH, bi, Xb, Yb, opts[0], opts[1], 1)
    return m, opts


@functools.lru_cache(maxsize=None)
def merged_fit(name, seed=0):
    """The default (merged launch) fit of a case: run once, shared by the comparisons, never modified."""
    import os
    assert os.environ.get("REDCLIFF_MERGE") is None and os.environ.get("REDCLIFF_FAC_PATH") is None
    m, opts = hip_fit(config(name), seed)
    return m, snapshot(m, opts)


@pytest.mark.parametrize("name", list(SHAPES))
def test_chain_edges_vs_oracle(name):
    from oracle.redcliff_oracle import OracleREDCLIFF
    c = config(name)
    args, kw = model_args(c)
    torch.manual_seed(0)
    o = OracleREDCLIFF(*args, **kw)
    oopts = optimizers(o)
    for bi, (Xb, Yb) in enumerate(windows(c)):
        o.batch_update(EPOCH, bi, Xb, Yb, oopts[0], oopts[1], 1)
    m, got = merged_fit(name)
    want = dict((k, v.detach().numpy()) for k, v in o.state_dict().items() if not k.startswith("gen_model."))
    compare_state(name, m, want, rtol=RTOL3, atol=ATOL3)  # parameters and BatchNorm buffers
    nmom = 0
    for g, oo in zip("AB", oopts):
        for i, prm in enumerate(oo.param_groups[0]["params"]):
            for kk in ("exp_avg", "exp_avg_sq"):
                w = oo.state[prm][kk].detach().numpy()
                key = "opt%s/%d/%s" % (g, i, kk)
                assert got[key].shape == w.shape, key
                assert_close("%s/%s" % (name, key), got[key], w, RTOL3, ATOL3 * max(1.0, float(np.abs(w).max())))
                nmom += 1
    assert nmom == sum(1 for k in got if k.startswith("opt"))


@pytest.mark.parametrize("name", list(SHAPES))
def test_chain_edges_merged_equals_two_launches(name, monkeypatch):
    _, merged = merged_fit(name)
    monkeypatch.setenv("REDCLIFF_MERGE", "0")
    m, opts = hip_fit(config(name))
    two = snapshot(m, opts)
    assert set(two) == set(merged)
    for k in merged:
        np.testing.assert_array_equal(merged[k], two[k], err_msg="%s %s" % (name, k))


def test_chain_edges_single_equals_pack():
    """Two replicas of the partial-everything shape in one pack (the replica on blockIdx.y, still the
    merged launch: 2 x 105 workgroups) against the same two fits alone."""
    from redcliff_amd import ReplicaPack
    name = "q35_b37_h20_k5_nf27_h20"
    c = config(name)
    packed = [hip_model(c, s) for s in (0, 1)]
    popts = [optimizers(m) for m in packed]
    pack = ReplicaPack(packed, popts)
    pack.run_epoch(EPOCH, pack.cache_dataset(windows(c)))
    for r, (m, o) in enumerate(zip(packed, popts)):
        got = snapshot(m, o)
        _, want = merged_fit(name, r)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg="replica %d %s" % (r, k))
