"""Edges of the factor kernels' slab staging (rc_common.h RcWinSeg / RcSegC).

The factor forward and the factor backward stage a tile of lag windows by reading each batch
row's window as one contiguous slab of L*p floats (32-bit offsets from one pointer that holds
row0, Lmax - L and the tile's first row) and scattering it to column ch*L + t; the W0 chunk is
one contiguous range clipped at h.  Tiles that are not one slab range keep a per-element form.
What can go wrong there, and the shapes that put it on the single-fit path:

  unaligned slabs   odd p and odd T*p with Lmax - L > 0 (p=3 L=3 F=5 T=7; p=5 L=7 F=9 T=11)
  row0 > 0          one case through engine.cache_dataset + plan_steps over three batches
                    (batch_update alone always starts at row 0)
  B                 1, 5, 37, 128 and 160 (a second window tile: the backward's restage)
  Q = p*L           9, 35, exactly 64 (no padding column), 70 (two dW0 column tiles: the
                    backward's per-element form) and 100 (> 96: the forward's 32-column tiles)
  h                 5, 20, 100: partial W0 chunks whose rows past h must be zero
  K                 1 and 5

Every shape stays inside the engine's limits and the merged launch's conditions listed in
tests/test_gpu_chain_edges.py, whose helpers run the fits.  Per case: three combined-phase
steps; parameters, BatchNorm buffers and Adam moments against the CPU oracle at the three-phase
bound (rtol 2e-4, atol 5e-6 x max(1, max |want|)); the merged launch against REDCLIFF_MERGE=0
bit for bit; one R = 2 pack against its single fits bit for bit.  (The float32 oracle against
itself in float64 stays below a tenth of that bound on every shape here.)"""
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
    "odd_q9_b5_h5_k1": dict(p=3, L=3, K=1, h=5, F=5, n=2, H=7, B=5, T=7),
    "odd_q35_b37_h20_k5": dict(p=5, L=7, K=5, h=20, F=9, n=3, H=20, B=37, T=11),
    "odd_q9_b1_h20_k5": dict(p=3, L=3, K=5, h=20, F=5, n=2, H=20, B=1, T=7),
    "q64_b128_h100_k1": dict(p=8, L=8, K=1, h=100, F=8, n=2, H=20, B=128, T=9),
    "q70_b37_h20_k5": dict(p=10, L=7, K=5, h=20, F=8, n=2, H=20, B=37, T=9),
    "q100_b37_h5_k1": dict(p=10, L=10, K=1, h=5, F=10, n=2, H=7, B=37, T=11),
    "odd_q35_b160_h20_k1": dict(p=5, L=7, K=1, h=20, F=9, n=3, H=20, B=160, T=11),
}
DATASET_CASE = "odd_q35_b37_h20_k5"  # also run from a cached dataset: batches at rows 0, 37, 74


def config(name):
    c = dict(SHAPES[name])
    assert c["T"] > max(c["L"], c["F"])
    c.update(nsup=c["K"], label_T=1)
    return c


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
def merged_fit(name, seed=0):
    """The default (merged launch) fit of a case: run once, shared by the comparisons, never modified."""
    assert os.environ.get("REDCLIFF_MERGE") is None and os.environ.get("REDCLIFF_FAC_PATH") is None
    m, opts = hip_fit(config(name), seed)
    return m, snapshot(m, opts)


def dataset_fit(c, seed=0):
    """The same three steps from one cached dataset: steps 1 and 2 read their windows at row0 > 0."""
    m = hip_model(c, seed)
    opts = optimizers(m)
    eng = m.engine()
    ds = eng.cache_dataset(windows(c))
    assert ds["len"] == STEPS and list(ds["rows"]) == [i * c["B"] for i in range(STEPS)]
    d = eng.workspace(ds["Bmax"], ds["T"])
    eng.plan_steps("combined", ds["X"], ds["lab"], ds["stats"], d, ds["rows"], ds["sizes"], opts[0], opts[1]).run()
    return m, opts


def check_vs_oracle(name, m, got):
    want, mom = oracle_fit(name)
    compare_state(name, m, want, rtol=RTOL3, atol=ATOL3)  # parameters and BatchNorm buffers
    for key, w in mom.items():
        assert got[key].shape == w.shape, key
        assert_close("%s/%s" % (name, key), got[key], w, RTOL3, ATOL3 * max(1.0, float(np.abs(w).max())))
    assert len(mom) == sum(1 for k in got if k.startswith("opt"))


@pytest.mark.parametrize("name", list(SHAPES))
def test_stage_edges_vs_oracle(name):
    m, got = merged_fit(name)
    check_vs_oracle(name, m, got)


@pytest.mark.parametrize("name", list(SHAPES))
def test_stage_edges_merged_equals_two_launches(name, monkeypatch):
    _, merged = merged_fit(name)
    monkeypatch.setenv("REDCLIFF_MERGE", "0")
    m, opts = hip_fit(config(name))
    two = snapshot(m, opts)
    assert set(two) == set(merged)
    for k in merged:
        np.testing.assert_array_equal(merged[k], two[k], err_msg="%s %s" % (name, k))


def test_stage_edges_row0_vs_oracle():
    m, opts = dataset_fit(config(DATASET_CASE))
    check_vs_oracle(DATASET_CASE, m, snapshot(m, opts))


def test_stage_edges_row0_merged_equals_two_launches(monkeypatch):
    m, opts = dataset_fit(config(DATASET_CASE))
    merged = snapshot(m, opts)
    monkeypatch.setenv("REDCLIFF_MERGE", "0")
    m2, opts2 = dataset_fit(config(DATASET_CASE))
    two = snapshot(m2, opts2)
    assert set(two) == set(merged)
    for k in merged:
        np.testing.assert_array_equal(merged[k], two[k], err_msg=k)


def test_stage_edges_single_equals_pack():
    """Two replicas of the unaligned-slab shape in one pack (rows 0, 37, 74 of its cached dataset)
    against the same two fits alone."""
    from redcliff_amd import ReplicaPack
    c = config(DATASET_CASE)
    packed = [hip_model(c, s) for s in (0, 1)]
    popts = [optimizers(m) for m in packed]
    pack = ReplicaPack(packed, popts)
    pack.run_epoch(EPOCH, pack.cache_dataset(windows(c)))
    for r, (m, o) in enumerate(zip(packed, popts)):
        got = snapshot(m, o)
        _, want = merged_fit(DATASET_CASE, r)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg="replica %d %s" % (r, k))
