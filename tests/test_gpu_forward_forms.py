"""The forms of the single-fit forward launch (rc_forward.hip): factor products on the matrix
cores, fc1 slices as wave teams of one 512-thread workgroup.

The factor workgroups run their layer-0 products as 16x16x4 matrix-core chains over slab tiles
(Q = p*L <= 96; rows = the chunk's 16 units, columns = 16 windows, reads of the last k-steps
clamped) and sum the 16 units from the accumulator layout in the 512-thread launches, where
REDCLIFF_FWD_MFMA=0 selects the vector loop; the 256-thread launches always run the vector loop.  When a window's fc1 has at most two channel slices, one 512-thread workgroup runs the
window with the slices on its two wave teams and exchanges their sums through LDS;
REDCLIFF_EMB_FWD_TEAMS=0 selects one 256-thread workgroup per slice and the arrival counter.
Every form keeps every sum's order, so all of them give the same bits.  What can go wrong, and
the shapes that put it on the single-fit path:

  Q = p*L    9, 35 (last k-step and last operand batch partly filled), 64 (no padding column),
             70 and 96 (Q > 64: the forward stores the activations from the accumulator layout
             and the backward reads them; 96 is the slab limit), 100 (32-column tiles: the vector
             loop, in 512-thread workgroups four windows per thread: at B = 37 and at B = 160, a
             full first window tile and a second one)
  B          1, 5, 37 (a partly filled 16-window tile, waves with no tile), 128, 160 (second tile)
  h          5, 20, 100 (chunk rows past h);  K  1 and 5
  fc1        one slice (p=3, H=7), two unequal slices (p=5, H=60: 3 + 2 channels; p=10, H=30:
             6 + 4; widths 180 / 120 columns, no multiple of 64), three slices on the untouched
             split path (p=5, H=100); n = 2 and 3, odd F

Per case: three combined-phase steps (helpers of tests/test_gpu_chain_edges.py); parameters,
BatchNorm buffers and Adam moments against the CPU oracle at the three-phase bound (rtol 2e-4,
atol 5e-6 x max(1, max |want|)); the default fit against both switches off (256 threads, vector
loop, split fc1), and against the vector loop in the 512-thread launch (products off alone), bit for bit; one
R = 2 pack of a team-path shape against its single fits bit for bit; and one check, through the
slice-partial region of the workspace, of which path the launch took.  The float32 oracle
against itself in float64 (same initial state, same windows, host only) stays below a tenth of
that bound on every shape here; the worst |f32 - f64| / bound over all tensors is recorded in
ORACLE_F64_RATIO."""
import functools
import os

import numpy as np
import pytest
import torch

from golden_io import assert_close
from test_gpu_chain_edges import (ATOL3, EPOCH, RTOL3, STEPS, hip_fit, hip_model, model_args, optimizers, snapshot,
                                  windows)
from test_gpu_parity import compare_state

pytestmark = pytest.mark.gpu

SHAPES = {
    "q9_b1_h20_k5_zs1": dict(p=3, L=3, K=5, h=20, F=5, n=2, H=7, B=1, T=7),
    "q35_b37_h20_k5_zs2": dict(p=5, L=7, K=5, h=20, F=9, n=3, H=60, B=37, T=11),
    "q64_b128_h100_k1_zs1": dict(p=8, L=8, K=1, h=100, F=8, n=2, H=20, B=128, T=9),
    "q70_b5_h5_k1_zs2": dict(p=10, L=7, K=1, h=5, F=8, n=2, H=30, B=5, T=9),
    "q96_b160_h20_k1_zs1": dict(p=8, L=12, K=1, h=20, F=13, n=2, H=20, B=160, T=14),
    "q100_b37_h5_k1_zs1": dict(p=10, L=10, K=1, h=5, F=10, n=2, H=7, B=37, T=11),
    "q35_b5_h5_k1_zs3": dict(p=5, L=7, K=1, h=5, F=9, n=2, H=100, B=5, T=11),
    "q100_b160_h20_k1_zs1": dict(p=10, L=10, K=1, h=20, F=10, n=2, H=7, B=160, T=11),
}
SLICES = {"q9_b1_h20_k5_zs1": 1, "q35_b37_h20_k5_zs2": 2, "q64_b128_h100_k1_zs1": 1, "q70_b5_h5_k1_zs2": 2,
          "q96_b160_h20_k1_zs1": 1, "q100_b37_h5_k1_zs1": 1, "q35_b5_h5_k1_zs3": 3,
          "q100_b160_h20_k1_zs1": 1}
# worst |float32 oracle - float64 oracle| / bound over every compared tensor (host run, see the header)
ORACLE_F64_RATIO = {"q9_b1_h20_k5_zs1": 0.0118, "q35_b37_h20_k5_zs2": 0.0367, "q64_b128_h100_k1_zs1": 0.0248,
                    "q70_b5_h5_k1_zs2": 0.0338, "q96_b160_h20_k1_zs1": 0.0500, "q100_b37_h5_k1_zs1": 0.0227,
                    "q35_b5_h5_k1_zs3": 0.0178, "q100_b160_h20_k1_zs1": 0.0205}
PACK_CASE = "q35_b37_h20_k5_zs2"  # a team-path shape with two unequal slices
SWITCHES = ("REDCLIFF_FWD_MFMA", "REDCLIFF_EMB_FWD_TEAMS")


def config(name):
    c = dict(SHAPES[name])
    assert c["T"] > max(c["L"], c["F"]) and c["L"] <= c["F"]
    c.update(nsup=c["K"], label_T=1)
    return c


def fc1_slices(c):
    """The channel slices of fc1 (rc_emb_fwd_slice_channels: about 200 columns of p*H each)."""
    cs = min(c["p"], max(1, 200 // c["H"], (c["p"] + 63) // 64))
    return (c["p"] + cs - 1) // cs


def test_shapes_reach_their_slice_counts():
    for name in SHAPES:
        assert fc1_slices(config(name)) == SLICES[name], name


@functools.lru_cache(maxsize=None)
def oracle_fit(name):
    """The CPU oracle's state and Adam moments after the case's three steps: run once, never modified."""
    from oracle.redcliff_oracle import OracleREDCLIFF
    c = config(name)
    args, kw = model_args(c)
    torch.manual_seed(0)
    o = OracleREDCLIFF(*args, **kw)
    oopts = optimizers(o)
    for bi, (Xb, Yb) in enumerate(windows(c)):
        o.batch_update(EPOCH, bi, Xb, Yb, oopts[0], oopts[1], 1)
    want = dict((k, v.detach().numpy().copy()) for k, v in o.state_dict().items() if not k.startswith("gen_model."))
    mom = {}
    for g, oo in zip("AB", oopts):
        for i, prm in enumerate(oo.param_groups[0]["params"]):
            for kk in ("exp_avg", "exp_avg_sq"):
                mom["opt%s/%d/%s" % (g, i, kk)] = oo.state[prm][kk].detach().numpy().copy()
    return want, mom


@functools.lru_cache(maxsize=None)
def default_fit(name, seed=0):
    """The default fit of a case (matrix-core products, wave teams where they apply): run once,
    shared by the comparisons, never modified."""
    assert all(os.environ.get(k) is None for k in SWITCHES + ("REDCLIFF_MERGE", "REDCLIFF_FAC_PATH"))
    m, opts = hip_fit(config(name), seed)
    return m, snapshot(m, opts)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_forms_vs_oracle(name):
    m, got = default_fit(name)
    want, mom = oracle_fit(name)
    compare_state(name, m, want, rtol=RTOL3, atol=ATOL3)  # parameters and BatchNorm buffers
    for key, w in mom.items():
        assert got[key].shape == w.shape, key
        assert_close("%s/%s" % (name, key), got[key], w, RTOL3, ATOL3 * max(1.0, float(np.abs(w).max())))
    assert len(mom) == sum(1 for k in got if k.startswith("opt"))


# both forms off (256 threads: the vector loop, one workgroup per slice); the vector loop in the 512-thread launch
ARMS = {"off": {"REDCLIFF_FWD_MFMA": "0", "REDCLIFF_EMB_FWD_TEAMS": "0"},
        "vector512": {"REDCLIFF_FWD_MFMA": "0"}}


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_forms_equal_switched(name, arm, monkeypatch):
    _, new = default_fit(name)
    for k, v in ARMS[arm].items():
        monkeypatch.setenv(k, v)
    m, opts = hip_fit(config(name))
    old = snapshot(m, opts)
    assert set(old) == set(new)
    for k in new:
        np.testing.assert_array_equal(new[k], old[k], err_msg="%s %s %s" % (name, arm, k))


def test_forward_forms_single_equals_pack():
    """Two replicas of a two-slice shape in one pack (one window per workgroup at R = 2, so the wave
    teams) against the same two fits alone."""
    from redcliff_amd import ReplicaPack
    c = config(PACK_CASE)
    packed = [hip_model(c, s) for s in (0, 1)]
    popts = [optimizers(m) for m in packed]
    pack = ReplicaPack(packed, popts)
    pack.run_epoch(EPOCH, pack.cache_dataset(windows(c)))
    for r, (m, o) in enumerate(zip(packed, popts)):
        got = snapshot(m, o)
        _, want = default_fit(PACK_CASE, r)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg="replica %d %s" % (r, k))


def partial_region(eng, c):
    """The fc1 slice-partial region of a fit's workspace (WsOff.f1p: the region after `dgs` in layout
    order, 64 slices x Bmax x M1 floats)."""
    from redcliff_amd import _native as nat
    from redcliff_amd.dgcnn import M1
    d = eng.dims(eng.ws_dims[0], c["T"])
    regions = nat.workspace_regions(d)
    at = [i for i, (start, _) in enumerate(regions) if start == eng.ws_off["dgs"]]
    assert len(at) == 1
    start, size = regions[at[0] + 1]
    assert size == 64 * eng.ws_dims[0] * M1, (size, eng.ws_dims[0], M1)
    return eng.ws[start:start + size]


def step_with_marked_partials(c):
    """One more step of a fresh three-step fit, with the slice-partial region filled with a mark
    before it: the number of the region's floats the step overwrote."""
    m, opts = hip_fit(c)
    region = partial_region(m.engine(), c)
    region.fill_(-77.0)
    Xb, Yb = windows(c)[0]
    m.batch_update(EPOCH, STEPS, Xb, Yb, opts[0], opts[1], 1)
    torch.cuda.synchronize()
    return int((region != -77.0).sum().item())


def test_forward_forms_launch_path(monkeypatch):
    """The team launch leaves the slice-partial region untouched; the split launch writes one row of
    M1 partials per (slice, window)."""
    c = config(PACK_CASE)
    assert step_with_marked_partials(c) == 0
    monkeypatch.setenv("REDCLIFF_EMB_FWD_TEAMS", "0")
    written = step_with_marked_partials(c)
    from redcliff_amd.dgcnn import M1
    assert written == SLICES[PACK_CASE] * c["B"] * M1, written
