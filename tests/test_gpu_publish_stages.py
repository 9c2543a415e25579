"""The factor leads' two-stage publish in the merged backward (rc_fac_bwd.h, rc_common.h).

A lead counts itself in twice on one counter word: stage 1 (low half) once its dL/dw partials are
in memory -- all that a node workgroup waits for -- and stage 2 (high half) once its dL/dA records
are, which the dA-reduce workgroups wait for; x_sim, G, the G0 row sums and the dL/dG / dL/dA part
run after stage 1.  In the merged launch the factor update's epilogue issues the dW0 tile's Adam
stores before the small bias / W1 reduction, which runs on lanes 0-15 (b0), 16-31 (W1) and wave 1
(b1); the two-launch form keeps the other order and lane mapping (same sums).  What can
go wrong is an ordering (a record read before it is stored, a deferred store lost) or a lane
mapping, on some shape's path, so every case below is compared bit for bit with the two-launch
form of the same build (REDCLIFF_MERGE=0, no hand-off at all), with the CPU oracle at the
tolerance of tests/test_gpu_chain_edges.py, and the device status word must stay clean.

Shapes (smallest that reach each path; all inside the merged launch's conditions, see
tests/test_gpu_chain_edges.py): B = 5 (partial 16-window block), 37 (partial last block, part 2
in nsl = 6 channel slices), 128 (the full tile); (K, p) = (4, 10) (K*p a multiple of 8: XCD-aware
order), (3, 5) (plain order), K = 1; h = 16 and h = 100 (partial last hidden chunk); p*L = 40,
64 (one full FB_QT tile) and 80 (two column tiles, stored activations, no recompute);
adjacency coefficient > 0 and = 0.  The combined step always carries the adjacency-loss flag
(engine.flags_for), so the coefficient-0 case runs the same hand-off with zero adjacency terms.
The step without the flag -- dL/dw stored inside part 1, part 2 skipped, no reduce workgroups --
is run by taking RC_LOSS_ADJ out of the combined step's flags (test_publish_stages_adjacency_flag_off:
at coefficient 0 it is the same loss, so the oracle still applies).  The pretrain epoch is an
embedder step with no factor launch at all (both sides run the same kernels; kept because it must
stay so); the step where the leads publish and return without an update (role RC_FB_ALL, no factor
step) is the combined step of a model whose factors are detached.  One R = 2 pack against its two
single fits.

Every comparison proves itself: after a merged step each replica's lead counter word holds K*p in
both halves (stage 1 low, stage 2 high; k_forward re-arms it only in the next step), after a
two-launch step it holds 0 -- so a shape that quietly fell back to two launches, or a lead that
skipped a stage, fails the test."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_gpu_parity import compare_state, synth

pytestmark = pytest.mark.gpu

RTOL3, ATOL3 = 2e-4, 5e-6  # tests/test_gpu_chain_edges.py's tolerance (test_gpu_parity's three-phase one)

SHAPES = {
    "kp40_q40_h100_b128": dict(p=10, L=4, K=4, h=100, F=20, n=2, H=30, B=128, adj=0.1),
    "kp15_q40_h16_b37_adj0": dict(p=5, L=8, K=3, h=16, F=8, n=2, H=20, B=37, adj=0.0),
    "kp15_q40_h16_b37": dict(p=5, L=8, K=3, h=16, F=8, n=2, H=20, B=37, adj=0.1),
    "kp8_q64_h16_b5_k1": dict(p=8, L=8, K=1, h=16, F=8, n=2, H=7, B=5, adj=0.1),
    "kp20_q80_h20_b37": dict(p=10, L=8, K=2, h=20, F=8, n=2, H=20, B=37, adj=0.1),
}
STEPS = 3
PRETRAIN, COMBINED = 0, 2  # epochs of the phases (one pretrain and one acclimation epoch first)


def config(name):
    c = dict(SHAPES[name])
    c.update(nsup=c["K"], T=max(c["L"], c["F"]) + 1, label_T=1)
    return c


def model_args(c):
    from oracle.redcliff_oracle import reference_coeffs
    eargs = [("num_features_per_node", c["F"]), ("num_graph_conv_layers", c["n"]), ("num_hidden_nodes", c["H"]),
             ("sigmoid_eccentricity_coeff", 10.0)]
    args = (c["p"], c["L"], [c["h"]], c["F"], [0], c["L"], 1, c["K"], c["nsup"],
            reference_coeffs(c["K"], c["p"], adj=c["adj"]), False, "DGCNN", eargs, "conditional_factor_fixed_embedder",
            "apply_factor_weights_after_sim_completion")
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
    """Every state_dict tensor (parameters, the adjacency, BatchNorm buffers) and every Adam moment."""
    torch.cuda.synchronize()
    out = dict((k, v.detach().cpu().numpy().copy()) for k, v in m.state_dict().items())
    for g, o in zip("AB", opts):
        for i, prm in enumerate(o.param_groups[0]["params"]):
            for kk in ("exp_avg", "exp_avg_sq"):
                if kk in o.state[prm]:
                    out["opt%s/%d/%s" % (g, i, kk)] = o.state[prm][kk].detach().cpu().numpy().copy()
    return out


def assert_status_clean(m, c):
    from redcliff_amd import _native as nat
    eng = m.engine()
    d = eng.dims(eng.ws_dims[0], c["T"])
    words = nat.device_status(d, eng.ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert words == [0], words
    m.check_device_status()


def lead_counter(owner, c, r=0):
    """The factor-lead counter word of replica r in the workspace of `owner` (a fit's engine or a
    pack): slot p * ceil(H / 16) of the ecnt region (rc_common.h rc_fac_lead_cnt)."""
    torch.cuda.synchronize()
    base = r * owner.ws_off["total"] + owner.ws_off["ecnt"] + c["p"] * ((c["H"] + 15) // 16)
    return int(owner.ws[base:base + 1].view(torch.int32).item()) & 0xffffffff


def published(c):
    """The counter word after a merged step: every lead counted in both halves."""
    return c["K"] * c["p"] * ((1 << 16) + 1)


@contextlib.contextmanager
def adjacency_flag_off():
    """The combined step's flags less RC_LOSS_ADJ (engine.step_flags reads engine.flags_for)."""
    from redcliff_amd import _native as nat
    from redcliff_amd import engine
    orig = engine.flags_for

    def flags_for(kind, nsup):
        flags, nbn = orig(kind, nsup)
        return flags & ~nat.LOSS_ADJ, nbn
    engine.flags_for = flags_for
    try:
        yield
    finally:
        engine.flags_for = orig


def hip_fit(c, seed=0, epoch=COMBINED, detach=False, noadj=False, counter=None):
    """counter: the lead counter word expected after the steps (published(c) for a merged launch, 0
    for two launches or no factor launch)."""
    m = hip_model(c, seed)
    if detach:
        m.__dict__["_factors_detached"] = True
    opts = optimizers(m)
    with adjacency_flag_off() if noadj else contextlib.nullcontext():
        for bi, (Xb, Yb) in enumerate(windows(c)):
            m.batch_update(epoch, bi, Xb, Yb, opts[0], opts[1], 1)
    assert_status_clean(m, c)
    if counter is not None:
        assert lead_counter(m.engine(), c) == counter, (lead_counter(m.engine(), c), counter)
    return m, opts


@functools.lru_cache(maxsize=None)
def merged_fit(name, seed=0, epoch=COMBINED, detach=False, noadj=False):
    """The default (merged launch) fit of a case: run once, shared by the comparisons, never modified.
    The counter word shows that the merged launch ran (the pretrain epoch has no factor launch)."""
    import os
    assert os.environ.get("REDCLIFF_MERGE") is None and os.environ.get("REDCLIFF_FAC_PATH") is None
    c = config(name)
    m, opts = hip_fit(c, seed, epoch, detach, noadj, counter=0 if epoch == PRETRAIN else published(c))
    return m, snapshot(m, opts)


def assert_same_bits(tag, got, want):
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (tag, k))


@pytest.mark.parametrize("name", list(SHAPES))
def test_publish_stages_merged_equals_two_launches(name, monkeypatch):
    _, merged = merged_fit(name)
    monkeypatch.setenv("REDCLIFF_MERGE", "0")
    m, opts = hip_fit(config(name), counter=0)
    assert_same_bits(name, snapshot(m, opts), merged)


def oracle_state(name):
    from oracle.redcliff_oracle import OracleREDCLIFF
    c = config(name)
    args, kw = model_args(c)
    torch.manual_seed(0)
    o = OracleREDCLIFF(*args, **kw)
    oopts = optimizers(o)
    for bi, (Xb, Yb) in enumerate(windows(c)):
        o.batch_update(COMBINED, bi, Xb, Yb, oopts[0], oopts[1], 1)
    return o, oopts


def compare_with_oracle(name, m, got, o, oopts):
    want = dict((k, v.detach().numpy()) for k, v in o.state_dict().items() if not k.startswith("gen_model."))
    compare_state(name, m, want, rtol=RTOL3, atol=ATOL3)  # parameters, the adjacency and BatchNorm buffers
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
def test_publish_stages_vs_oracle(name):
    m, got = merged_fit(name)
    compare_with_oracle(name, m, got, *oracle_state(name))


def test_publish_stages_adjacency_flag_off(monkeypatch):
    """The merged step without RC_LOSS_ADJ: the leads store dL/dw inside part 1, skip part 2 and the
    dL/dG / dL/dA part, publish both stages, and the launch has no reduce workgroups.  At adjacency
    coefficient 0 the loss is the flagged one's, so the oracle applies; merged against two launches
    bit for bit."""
    name = "kp15_q40_h16_b37_adj0"
    m, merged = merged_fit(name, noadj=True)
    compare_with_oracle(name, m, merged, *oracle_state(name))
    monkeypatch.setenv("REDCLIFF_MERGE", "0")
    m2, opts = hip_fit(config(name), noadj=True, counter=0)
    assert_same_bits(name, snapshot(m2, opts), merged)


@pytest.mark.parametrize("epoch,detach", [(PRETRAIN, False), (COMBINED, True)], ids=["pretrain", "factors_detached"])
def test_publish_stages_embedder_step_only(epoch, detach, monkeypatch):
    """Embedder steps without a factor update: the pretrain epoch, and the combined step of a model
    with detached factors, whose leads publish both stages and return."""
    name = "kp15_q40_h16_b37"
    _, merged = merged_fit(name, 0, epoch, detach)
    monkeypatch.setenv("REDCLIFF_MERGE", "0")
    m, opts = hip_fit(config(name), 0, epoch, detach, counter=0)
    assert_same_bits(name, snapshot(m, opts), merged)


def test_publish_stages_pack_equals_single_fits():
    """Two replicas in one pack (the replica on blockIdx.y, a counter word per replica) against
    the same two fits alone."""
    from redcliff_amd import ReplicaPack
    name = "kp15_q40_h16_b37"
    c = config(name)
    packed = [hip_model(c, s) for s in (0, 1)]
    popts = [optimizers(m) for m in packed]
    pack = ReplicaPack(packed, popts)
    pack.run_epoch(COMBINED, pack.cache_dataset(windows(c)))
    pack.check_device_status()
    for r in range(2):  # the pack's workspace holds both replicas' slices, a counter word each
        assert lead_counter(pack, c, r) == published(c), r
    for r, (m, o) in enumerate(zip(packed, popts)):
        _, want = merged_fit(name, r)
        assert_same_bits("replica %d" % r, snapshot(m, o), want)
