"""The embedder forward's fc1 weight request and refills (emb_fwd_body, rc_forward.hip).

Each wave requests the first three 64-column steps of its fc1 slice ahead of BatchNorm -- those
the slice has -- multiplies them after the graph convolution and refills a buffer only when the
slice has the column step it would hold; the workspace copies of T and R are stored from LDS after
the products, on the split path by every slice's workgroup before the early return of all but the
last.  What can go wrong is the number of column steps per slice, so the shapes are chosen for it
(slice widths follow rc_emb_fwd_slice_channels at 200 columns):

  one partial step          p=3,  H=7    21 columns
  exactly one step          p=2,  H=32   64
  exactly two steps         p=2,  H=64   128
  exactly three steps       p=6,  H=32   192 (no clamped lane)
  four steps                p=10, H=20   200 (one slice; the rotation's refill is used)
  two slices                p=8,  H=32   192 + 64;  p=14, H=20  200 + 80;  p=10, H=30  180 + 120 (D4IC's)
  three slices, split path  p=5,  H=100  200 + 200 + 100 (the deferred stores before the early return)
  weights not in LDS        p=3, n=4, F=64, H=60, T=66: by emb_fwd_floats 16,857 floats with the graph
                            convolution's weights in LDS, above the 16,384-float budget, and 1,497 without
                            (computed below, the launch's own arithmetic; the workspace shows no trace of it)

with B = 1, 5 and 37, n = 2, 3 (and 4), F odd in one case.  BatchNorm runs in training mode
throughout: the helpers step through batch_update, which has no evaluation-mode forward.

Per case: three combined-phase steps (helpers of tests/test_gpu_chain_edges.py and
tests/test_gpu_forward_forms.py); parameters, BatchNorm buffers and Adam moments against the CPU
oracle at the three-phase bound (rtol 2e-4, atol 5e-6 x max(1, max |want|)); the default launch
against REDCLIFF_EMB_FWD_TEAMS=0 bit for bit; one R = 2 pack against its single fits bit for bit,
and one R = 8 pack of the three-slice shape (four windows per workgroup, every slice on it: a
refill, then the next slice's request under the reduce-scatter) against its single fits.
The float32 oracle against itself in float64 (same initial state, same windows, host only) stays
below a tenth of that bound on every shape here; the worst |f32 - f64| / bound over all tensors
is recorded in ORACLE_F64_RATIO."""
import functools
import os

import numpy as np
import pytest

from golden_io import assert_close
from test_gpu_chain_edges import ATOL3, EPOCH, RTOL3, hip_fit, hip_model, optimizers, snapshot, windows
from test_gpu_forward_forms import fc1_slices
from test_gpu_parity import compare_state

pytestmark = pytest.mark.gpu

SHAPES = {
    "c21_b1": dict(p=3, L=3, K=2, h=5, F=5, n=2, H=7, B=1, T=7),
    "c64_b5_oddF": dict(p=2, L=3, K=1, h=5, F=7, n=3, H=32, B=5, T=8),
    "c128_b5": dict(p=2, L=3, K=1, h=5, F=5, n=2, H=64, B=5, T=7),
    "c192_b37": dict(p=6, L=3, K=1, h=5, F=5, n=2, H=32, B=37, T=7),
    "c200_b5": dict(p=10, L=3, K=1, h=5, F=5, n=3, H=20, B=5, T=7),
    "c192_64_b5": dict(p=8, L=3, K=2, h=5, F=5, n=2, H=32, B=5, T=7),
    "c200_80_b1": dict(p=14, L=3, K=1, h=5, F=5, n=2, H=20, B=1, T=7),
    "c180_120_b37": dict(p=10, L=3, K=1, h=5, F=6, n=2, H=30, B=37, T=8),
    "c200_200_100_b5": dict(p=5, L=3, K=1, h=5, F=5, n=2, H=100, B=5, T=7),
    "c180_b5_wglobal": dict(p=3, L=3, K=1, h=5, F=64, n=4, H=60, B=5, T=66),
}
# the 64-column steps of each fc1 slice
STEPS_PER_SLICE = {"c21_b1": [1], "c64_b5_oddF": [1], "c128_b5": [2], "c192_b37": [3], "c200_b5": [4],
                   "c192_64_b5": [3, 1], "c200_80_b1": [4, 2], "c180_120_b37": [3, 2], "c200_200_100_b5": [4, 4, 2],
                   "c180_b5_wglobal": [3]}
# worst |float32 oracle - float64 oracle| / bound over every compared tensor (host run, see the header)
ORACLE_F64_RATIO = {"c21_b1": 0.0258, "c64_b5_oddF": 0.0313, "c128_b5": 0.0235, "c192_b37": 0.0191, "c200_b5": 0.0504,
                    "c192_64_b5": 0.0179, "c200_80_b1": 0.0260, "c180_120_b37": 0.0186, "c200_200_100_b5": 0.0371,
                    "c180_b5_wglobal": 0.0899}
PACK_CASE = "c180_120_b37"
LDS_BUDGET_FLOATS = 16384  # RC_LDS_LIMIT_FLOATS


def config(name):
    c = dict(SHAPES[name])
    assert c["T"] > max(c["L"], c["F"]) and c["L"] <= c["F"]
    c.update(nsup=c["K"], label_T=1)
    return c


def slice_steps(c):
    cs = min(c["p"], max(1, 200 // c["H"], (c["p"] + 63) // 64))
    widths = [(min(c["p"], (z + 1) * cs) - z * cs) * c["H"] for z in range((c["p"] + cs - 1) // cs)]
    return [(w + 63) // 64 for w in widths]


def emb_fwd_floats(c, w_lds, team):
    """emb_fwd_floats of rc_forward.hip for one window per workgroup."""
    from redcliff_amd.dgcnn import M1
    pF, pH = c["p"] * c["F"], c["p"] * c["H"]
    return (pF + c["n"] * c["p"] ** 2 + (c["n"] * c["F"] * c["H"] if w_lds else 0) + c["n"] * pF + pH + M1 + c["K"] * M1 +
            M1 + c["K"] + 2 * c["F"] + (2 * M1 if team else 0))


def test_shapes_reach_their_step_counts():
    for name in SHAPES:
        c = config(name)
        assert slice_steps(c) == STEPS_PER_SLICE[name], name
        assert fc1_slices(c) == len(STEPS_PER_SLICE[name]), name
        in_lds = emb_fwd_floats(c, 1, False) <= LDS_BUDGET_FLOATS
        assert in_lds == (name != "c180_b5_wglobal"), name
    c = config("c180_b5_wglobal")
    assert emb_fwd_floats(c, 0, True) <= LDS_BUDGET_FLOATS


@functools.lru_cache(maxsize=None)
def oracle_fit(name):
    """The CPU oracle's state and Adam moments after the case's three steps: run once, never modified."""
    import torch
    from oracle.redcliff_oracle import OracleREDCLIFF
    from test_gpu_chain_edges import model_args
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
    """The default fit of a case: run once, shared by the comparisons, never modified."""
    assert all(os.environ.get(k) is None for k in ("REDCLIFF_FWD_MFMA", "REDCLIFF_EMB_FWD_TEAMS", "REDCLIFF_MERGE",
                                                   "REDCLIFF_FAC_PATH", "REDCLIFF_EMB_FWD_COLS"))
    m, opts = hip_fit(config(name), seed)
    return m, snapshot(m, opts)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_prefetch_vs_oracle(name):
    m, got = default_fit(name)
    want, mom = oracle_fit(name)
    compare_state(name, m, want, rtol=RTOL3, atol=ATOL3)  # parameters and BatchNorm buffers
    for key, w in mom.items():
        assert got[key].shape == w.shape, key
        assert_close("%s/%s" % (name, key), got[key], w, RTOL3, ATOL3 * max(1.0, float(np.abs(w).max())))
    assert len(mom) == sum(1 for k in got if k.startswith("opt"))


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_prefetch_equals_split_launch(name, monkeypatch):
    """The default launch (wave teams where a window has at most two slices) against one 256-thread
    workgroup per slice: the same bits."""
    _, new = default_fit(name)
    monkeypatch.setenv("REDCLIFF_EMB_FWD_TEAMS", "0")
    m, opts = hip_fit(config(name))
    old = snapshot(m, opts)
    assert set(old) == set(new)
    for k in new:
        np.testing.assert_array_equal(new[k], old[k], err_msg="%s %s" % (name, k))


def test_forward_prefetch_wide_pack_equals_single_fits(monkeypatch):
    """R = 8 replicas of the three-slice shape in one pack: at R >= 8 a workgroup holds four windows
    and runs every slice of them (k_forward<4, 256>), so a slice of four column steps -- one refill --
    is followed by the request of the next slice's first steps under its reduce-scatter; B = 5 leaves
    the second workgroup one window of four.  Against the same eight fits alone (the split path).
    Packs of >= 8 replicas pick the matrix-core factor path by default, whose sums are not the vector
    path's, so the factor path is pinned for both sides (as tests/test_gpu_replicas.py does): the
    embedder forward is the same launch on either."""
    from redcliff_amd import ReplicaPack
    monkeypatch.setenv("REDCLIFF_FAC_PATH", "mfma")
    name = "c200_200_100_b5"
    c = config(name)
    assert STEPS_PER_SLICE[name] == [4, 4, 2]
    packed = [hip_model(c, s) for s in range(8)]
    popts = [optimizers(m) for m in packed]
    pack = ReplicaPack(packed, popts)
    pack.run_epoch(EPOCH, pack.cache_dataset(windows(c)))
    for r, (m, o) in enumerate(zip(packed, popts)):
        got = snapshot(m, o)
        want = snapshot(*hip_fit(c, r))
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg="replica %d %s" % (r, k))


def test_forward_prefetch_single_equals_pack():
    """Two replicas of D4IC's slice widths in one pack against the same two fits alone."""
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
