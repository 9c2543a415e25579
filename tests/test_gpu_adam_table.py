"""The Adam table of redcliff_train_steps against the same library with the table switched off.

redcliff_train_steps evaluates the Adam bias corrections of a call's steps once per chunk of
steps (k_adam_table) and the step kernels read the entry instead of evaluating two double pow per
workgroup.  The entry is what the kernels computed, so a table run must leave every state tensor
(packed parameters, both moment pairs, BatchNorm running statistics and counter) bit-identical to
the run with REDCLIFF_ADAM_TABLE=0 (read per call), to the run that crosses chunk refills
(REDCLIFF_ADAM_TABLE_SMAX=3: 8 steps = chunks of 3, 3, 2) and to redcliff_train_step called
directly step by step (which never has a table).

Shapes: the smallest at which the kernels can still go wrong -- p = 3, L = 2, K = 2, nsup = 1,
F = 4, H = 5; h = 5 (one partly filled 16-unit chunk) and 20 (two chunks, the second partly
filled); n = 2 and 3 Chebyshev layers; B = 5 and 33 windows.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = dict(p=3, L=2, K=2, nsup=1, F=4, H=5)
SHAPES = [dict(BASE, h=h, n=n, B=B) for h, n, B in itertools.product((5, 20), (2, 3), (5, 33))]
IDS = ["h%d-n%d-B%d" % (c["h"], c["n"], c["B"]) for c in SHAPES]
NSTEPS = 8
PHASES = ("pretrain_embedder", "acclimate", "combined")  # steps A only, B only, both


def make(cfg, seed, pre=1, acc=1):
    import redcliff_amd
    K, p = cfg["K"], cfg["p"]
    coeff = {"FORECAST_COEFF": 10.0, "FACTOR_SCORE_COEFF": 100.0, "FACTOR_COS_SIM_COEFF": 1.0 / sum(range(1, K)),
             "FACTOR_WEIGHT_L1_COEFF": 1e-3, "FACTOR_WEIGHT_SMOOTHING_PENALTY_COEFF": 0.0,
             "ADJ_L1_REG_COEFF": 0.1 / K / np.sqrt(p * p - 1.0), "DAGNESS_REG_COEFF": 0.0, "DAGNESS_LAG_COEFF": 0.0,
             "DAGNESS_NODE_COEFF": 0.0}
    eargs = [("num_features_per_node", cfg["F"]), ("num_graph_conv_layers", cfg["n"]),
             ("num_hidden_nodes", cfg["H"]), ("sigmoid_eccentricity_coeff", 10.0)]
    torch.manual_seed(seed)
    return redcliff_amd.REDCLIFF_S_CMLP_withStateSmoothing(
        p, cfg["L"], [cfg["h"]], cfg["F"], [0], cfg["L"], 1, K, cfg["nsup"], coeff, False, "DGCNN", eargs,
        "conditional_factor_fixed_embedder", "apply_factor_weights_after_sim_completion", num_sims=1,
        training_mode="pretrain_embedder_then_acclimate_factors_then_combined", num_pretrain_epochs=pre,
        num_acclimation_epochs=acc).cuda()


def opts(m, lrB=5e-4, lrA=2e-4):
    oA = torch.optim.Adam(m.gen_model[0].parameters(), lr=lrA, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-4)
    oB = torch.optim.Adam(m.gen_model[1].parameters(), lr=lrB, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-4)
    return oA, oB


def data(cfg, seed=3):
    rng = np.random.RandomState(seed)
    N, B = NSTEPS * cfg["B"], cfg["B"]
    X = torch.from_numpy(rng.randn(N, cfg["F"] + 1, cfg["p"]).astype(np.float32))
    Y = np.zeros((N, cfg["K"], 1), np.float32)
    Y[np.arange(N), rng.randint(0, cfg["K"], N), 0] = 10.0
    Y = torch.from_numpy(Y)
    return [(X[i:i + B], Y[i:i + B]) for i in range(0, N, B)]


def snapshot(models, optims):
    out = {}
    for r, (m, pair) in enumerate(zip(models, optims)):
        for k, t in m.state_dict().items():
            out["%d/%s" % (r, k)] = t.detach().cpu().numpy().copy()
        for g, o in zip("AB", pair):
            for i, st in o.state_dict()["state"].items():
                for kk in ("exp_avg", "exp_avg_sq"):
                    if kk in st:
                        out["%d/opt%s/%d/%s" % (r, g, i, kk)] = st[kk].detach().cpu().numpy().copy()
    return out


def set_env(monkeypatch, env):
    for k in ("REDCLIFF_ADAM_TABLE", "REDCLIFF_ADAM_TABLE_SMAX", "REDCLIFF_FAC_PATH", "REDCLIFF_FORK", "REDCLIFF_MERGE",
              "REDCLIFF_SPLIT_LEAD", "REDCLIFF_CEMB_PATH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def direct_steps(a, rows, sizes, stream, what, bn_step=0, cemb=None):
    """_native.train_steps as a host loop of redcliff_train_step calls (the C loop's arguments)."""
    from redcliff_amd import _native as nat
    assert cemb is None
    s = nat.StepArgs.from_buffer_copy(a)
    for i, (r, b) in enumerate(zip(rows, sizes)):
        s.row0, s.B = int(r), int(b)
        s.flags = a.flags if i == 0 else a.flags & ~nat.REFRESH_SUPPORTS
        s.tA = a.tA + (i if a.flags & nat.STEP_A else 0)
        s.tB = a.tB + (i if a.flags & nat.STEP_B else 0)
        if a.bn_stats:
            s.bn_stats = a.bn_stats + 8 * i * bn_step
        nat.check(nat.lib().redcliff_train_step(ctypes.byref(s), stream), what)
    return len(rows)


TRAIN_STEPS = []  # the library's own _native.train_steps


@pytest.fixture(autouse=True)
def _train_steps():
    from redcliff_amd import _native as nat
    if not TRAIN_STEPS:
        TRAIN_STEPS.append(nat.train_steps)


def run_single(cfg, monkeypatch, env, direct=False):
    """8 steps of each of the three phases, one redcliff_train_steps call per phase."""
    from redcliff_amd import _native as nat
    set_env(monkeypatch, env)
    monkeypatch.setattr(nat, "train_steps", direct_steps if direct else TRAIN_STEPS[0])
    m = make(cfg, 0)
    pair = opts(m)
    eng = m.engine()
    ds = eng.cache_dataset(data(cfg))
    for kind in PHASES:
        eng.run_steps([kind], ds, *pair)
    torch.cuda.synchronize()
    eng.check_device_status("test")
    monkeypatch.setattr(nat, "train_steps", TRAIN_STEPS[0])
    return snapshot([m], [pair])


_REF = {}


def reference(key, fn):
    """The table-off run of a scenario, computed once and shared by the tests that compare with it."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def same(got, want, tag):
    assert set(got) == set(want)
    for k, w in want.items():
        np.testing.assert_array_equal(got[k], w, err_msg="%s: %s" % (tag, k))
        if w.dtype.kind == "f":
            assert np.isfinite(w).all(), k


@pytest.mark.parametrize("cfg", SHAPES, ids=IDS)
@pytest.mark.parametrize("smax", [None, "3"], ids=["one-chunk", "refills"])
def test_table_bitwise_equals_table_off(cfg, smax, monkeypatch):
    want = reference(("single", IDS[SHAPES.index(cfg)]), lambda: run_single(cfg, monkeypatch, {"REDCLIFF_ADAM_TABLE": "0"}))
    got = run_single(cfg, monkeypatch, {} if smax is None else {"REDCLIFF_ADAM_TABLE_SMAX": smax})
    same(got, want, "table (SMAX %s)" % smax)


@pytest.mark.parametrize("cfg", SHAPES, ids=IDS)
def test_direct_train_step_untouched(cfg, monkeypatch):
    """redcliff_train_step called directly carries no table: the same bits as the table-off
    redcliff_train_steps run, whatever REDCLIFF_ADAM_TABLE says."""
    want = reference(("single", IDS[SHAPES.index(cfg)]), lambda: run_single(cfg, monkeypatch, {"REDCLIFF_ADAM_TABLE": "0"}))
    same(run_single(cfg, monkeypatch, {}, direct=True), want, "direct")
    same(run_single(cfg, monkeypatch, {"REDCLIFF_ADAM_TABLE": "0"}, direct=True), want, "direct, table off")


FORKED = {"mfma-forked": {"REDCLIFF_FAC_PATH": "mfma", "REDCLIFF_FORK": "1"},
          "split-lead": {"REDCLIFF_FAC_PATH": "vector", "REDCLIFF_MERGE": "0", "REDCLIFF_SPLIT_LEAD": "1"}}


@pytest.mark.parametrize("cfg", SHAPES, ids=IDS)
@pytest.mark.parametrize("mode", sorted(FORKED))
def test_second_stream_reads_the_table(cfg, mode, monkeypatch):
    """Steps whose factor update runs on the second stream (the forked matrix-core step, the
    split-lead step) read the B entry there: ordered behind the table launch by the step's own
    fork event, and a refill behind the previous step's join (SMAX 3: two refills)."""
    env = FORKED[mode]
    want = reference((mode, IDS[SHAPES.index(cfg)]), lambda: run_single(cfg, monkeypatch, dict(env, REDCLIFF_ADAM_TABLE="0")))
    same(run_single(cfg, monkeypatch, dict(env, REDCLIFF_ADAM_TABLE_SMAX="3")), want, mode)


def table_layout(d):
    from redcliff_amd import _native as nat
    return nat.adam_table_layout(d)


def expected_entry(group, t):
    """The Python-double formulas of torch's Adam, cast to float32 (neg_step, bc2s, eps, wd, b2, omb1, omb2)."""
    b1, b2 = (float(b) for b in group["betas"])
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return np.asarray([-(float(group["lr"]) / bc1), math.sqrt(bc2), group["eps"], group["weight_decay"], b2, 1.0 - b1,
                       1.0 - b2], dtype=np.float64).astype(np.float32)


def check_entries(tab, esz, steps, group_t, tag):
    """tab: a replica's table floats; group_t: per group (param group, step number of step i or None = unused)."""
    inexact = 0
    for i in range(steps):
        for g, (grp, t_of) in enumerate(group_t):
            got = tab[(2 * i + g) * esz:(2 * i + g) * esz + 7]
            want = expected_entry(grp, t_of(i))
            ulp = np.spacing(np.abs(want))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), \
                "%s: step %d group %s: %s vs %s" % (tag, i, "AB"[g], got, want)
            np.testing.assert_array_equal(got[2:], want[2:], err_msg="%s: the copied hyper-parameters" % tag)
            inexact += int((got != want).sum())
    return inexact


@pytest.mark.parametrize("t0", [1, 100000])
def test_table_entries_match_python_doubles(t0, monkeypatch):
    """The table read back after a call starting at step number t0: every entry within 1 float32
    ulp of the Python-double formulas (the device pow is not glibc's; the number of entries not
    exactly equal is printed).  The call steps ONE group (pretrain_embedder: A), so the other
    group's step number must not advance: its entries all carry its t0."""
    set_env(monkeypatch, {})
    cfg = SHAPES[0]
    m = make(cfg, 0)
    oA, oB = opts(m)
    eng = m.engine()
    ds = eng.cache_dataset(data(cfg))
    eng.run_steps(["acclimate"], ds, oA, oB)  # binds optimizer B (and leaves it at t = 8)
    eng.run_steps(["pretrain_embedder"], ds, oA, oB)  # binds optimizer A
    for g in "AB":
        eng.opt[g]["t"] = t0 - 1
    eng._sync_steps()
    eng.run_steps(["pretrain_embedder"], ds, oA, oB)
    torch.cuda.synchronize()
    d = eng.dims(eng.ws_dims[0], cfg["F"] + 1)
    off, smax, esz = table_layout(d)
    assert smax >= NSTEPS and esz == 8
    tab = eng.ws[off:off + NSTEPS * 2 * esz].cpu().numpy()
    n = check_entries(tab, esz, NSTEPS, [(oA.param_groups[0], lambda i: t0 + i), (oB.param_groups[0], lambda i: t0)],
                      "t0 = %d" % t0)
    print("t0 = %d: %d of %d table floats differ from the float32 of the Python doubles (all within 1 ulp)"
          % (t0, n, NSTEPS * 2 * 7))
    assert eng.opt["A"]["t"] == t0 - 1 + NSTEPS and eng.opt["B"]["t"] == t0 - 1


def run_pack(cfg, monkeypatch, env, check_table=False):
    """Two replicas with different learning rates and schedules (replica 1 pretrains one epoch
    longer), so from epoch 1 on their step numbers differ (non-zero t_offset)."""
    from redcliff_amd import ReplicaPack
    set_env(monkeypatch, env)
    models = [make(cfg, 0, pre=1), make(cfg, 1, pre=2)]
    optims = [opts(models[0], 5e-4, 2e-4), opts(models[1], 1e-4, 5e-4)]
    pack = ReplicaPack(models, optims)
    ds = pack.cache_dataset(data(cfg))
    for epoch in range(4):  # (A, A) (B, A) (A+B, B) (A+B, A+B)
        before = [[e.opt[g]["t"] if e.opt[g] is not None else 0 for g in "AB"] for e in pack.engines]
        pack.run_epoch(epoch, ds)
    torch.cuda.synchronize()
    if check_table:
        assert before[0][1] != before[1][1]  # the last epoch ran with a non-zero t_offset
        d = pack._workspace(cfg["B"], cfg["F"] + 1)
        off, _, esz = table_layout(d)
        total = pack.ws_off["total"]
        for r in range(2):
            tab = pack.ws[r * total + off:r * total + off + NSTEPS * 2 * esz].cpu().numpy()
            check_entries(tab, esz, NSTEPS, [(optims[r][g].param_groups[0], lambda i, t=before[r][g]: t + 1 + i)
                                            for g in (0, 1)], "pack replica %d" % r)
    return snapshot(models, optims)


@pytest.mark.parametrize("cfg", SHAPES, ids=IDS)
def test_mixed_schedule_pack_bitwise_equals_table_off(cfg, monkeypatch):
    want = reference(("pack", IDS[SHAPES.index(cfg)]), lambda: run_pack(cfg, monkeypatch, {"REDCLIFF_ADAM_TABLE": "0"}))
    same(run_pack(cfg, monkeypatch, {}, check_table=True), want, "pack")


@pytest.mark.parametrize("name", ["ragged", "sigmoid"])
def test_cemb_steps_table_bitwise_equals_table_off(name, monkeypatch):
    """redcliff_cemb_train_steps fills the same table (k_cemb_bwd reads the A entry, the matrix-core
    factor chain the B entry): 8 steps of each phase of the fused cEmbedder step, one chunk and
    chunks of 3, against the table switched off."""
    from test_gpu_cemb_fused import SHAPES as CEMB_SHAPES
    from test_gpu_cemb_fused import adam_pair, hip_model
    from test_gpu_parity import synth
    cfg = CEMB_SHAPES[name]

    def run(env):
        set_env(monkeypatch, dict(env, REDCLIFF_CEMB_PATH="fused"))
        m = hip_model(cfg, 0)
        pair = adam_pair(m, 2e-4, 5e-4)
        X, Y = synth(cfg, NSTEPS * cfg["B"], seed=5)
        eng = m._cemb_fused(cfg["B"])
        ds = eng.cache_dataset([(X[i:i + cfg["B"]], Y[i:i + cfg["B"]]) for i in range(0, X.shape[0], cfg["B"])])
        for kind in PHASES:
            eng.run_steps([kind], ds, *pair)
        torch.cuda.synchronize()
        return snapshot([m], [pair])

    want = run({"REDCLIFF_ADAM_TABLE": "0"})
    same(run({}), want, "cEmbedder, one chunk")
    same(run({"REDCLIFF_ADAM_TABLE_SMAX": "3"}), want, "cEmbedder, refills")
