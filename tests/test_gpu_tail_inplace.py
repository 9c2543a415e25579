"""The embedder tail whose workgroups sum the window-block partials in place (k_emb_tail: no
combine pass, no counter, no wait) against k_emb_combine + k_emb_final, bit for bit.

Every case trains through pretrain -> acclimate -> combined (5 epochs) under workspace guard
bands, once with the two launches (REDCLIFF_TAIL=0) and twice with the tail: the whole
state_dict must be equal, and the second tail run must repeat the first.  The shapes are the
smallest at which each index path of the tail can go wrong:

* D4IC-shaped, batches of 64, 64, 24: four window blocks, then a ragged two with an 8-window last
  block; two column chunks, the last with 14 columns; on the merged, two-launch and split-lead
  backward paths;
* the same shape with batches of 144 and 40: nine window blocks, one more than the eight loads a
  sum requests per round;
* n = 3, F = 16, H = 40: three chunks, the last with 8 columns, two dS rows per record, the
  Chebyshev products in the adjacency workgroup;
* p = 3, K = 2, H = 12: one partial chunk, p * p = 9, rows shorter than a lane quad, three
  BatchNorm-affine groups (no full chain of four).
"""
import numpy as np
import pytest
import torch

from test_gpu_forked import arm, check_bands, guard_bands  # noqa: F401  (guard_bands: fixture)

pytestmark = pytest.mark.gpu

D4IC = dict(p=10, L=4, K=4, nsup=4, h=100, F=20, n=2, H=30, T=21)
TAIL = "1"  # REDCLIFF_TAIL value of the one-launch tail


def make(cfg, seed):
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
        training_mode="pretrain_embedder_then_acclimate_factors_then_combined", num_pretrain_epochs=1,
        num_acclimation_epochs=1).cuda()


def data(cfg, sizes, seed):
    rng = np.random.RandomState(seed)
    N = sum(sizes)
    X = rng.randn(N, cfg["T"], cfg["p"]).astype(np.float32)
    Y = np.zeros((N, cfg["K"], 1), np.float32)
    Y[np.arange(N), rng.randint(0, cfg["K"], N), 0] = 10.0
    X, Y = torch.from_numpy(X), torch.from_numpy(Y)
    out, i = [], 0
    for b in sizes:
        out.append((X[i:i + b], Y[i:i + b]))
        i += b
    return out


def run(monkeypatch, cfg, train, tail, merge, split, guarded):
    monkeypatch.setenv("REDCLIFF_FAC_PATH", "vector")
    monkeypatch.setenv("REDCLIFF_TAIL", tail)
    for key, v in (("REDCLIFF_MERGE", merge), ("REDCLIFF_SPLIT_LEAD", split)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, v)
    m = make(cfg, 0)
    oA = torch.optim.Adam(m.gen_model[0].parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-4)
    oB = torch.optim.Adam(m.gen_model[1].parameters(), lr=5e-4, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-4)
    eng = m.engine()
    T = train[0][0].shape[1]
    eng.workspace(max(x.shape[0] for x, _ in train), T)
    armed = arm(eng.ws, eng.dims(eng.ws_dims[0], T), 1) if guarded else None
    for epoch in range(5):
        for bi, (Xb, Yb) in enumerate(train):
            m.batch_update(epoch, bi, Xb, Yb, oA, oB, 1)
    torch.cuda.synchronize()
    if guarded:
        check_bands(eng.ws, armed[0], armed[1], 1, "tail=%s merge=%s split=%s" % (tail, merge, split))
    st = {k: t.detach().cpu().numpy() for k, t in m.state_dict().items()}
    for k, v in st.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    return st


CASES = [
    ("d4ic-merged", D4IC, (64, 64, 24), "1", "0"),
    ("d4ic-two-launch", D4IC, (64, 64, 24), "0", "0"),
    ("d4ic-split-lead", D4IC, (64, 64, 24), "0", "1"),
    ("d4ic-nine-blocks", D4IC, (144, 40), None, None),
    ("n3-three-chunks", dict(D4IC, F=16, n=3, H=40), (64, 24), "0", None),
    ("p3-one-partial-chunk", dict(D4IC, p=3, K=2, nsup=2, H=12), (64, 24), None, None),
]


@pytest.mark.parametrize("name,cfg,sizes,merge,split", CASES, ids=[c[0] for c in CASES])
def test_inplace_tail_bitwise_equals_combine_and_final(name, cfg, sizes, merge, split, monkeypatch, guard_bands):
    train = data(cfg, sizes, seed=21)
    want = run(monkeypatch, cfg, train, "0", merge, split, True)
    got = run(monkeypatch, cfg, train, TAIL, merge, split, True)
    again = run(monkeypatch, cfg, train, TAIL, merge, split, False)
    assert set(got) == set(want)
    for k, w in want.items():
        np.testing.assert_array_equal(got[k], w, err_msg="%s %s" % (name, k))
        np.testing.assert_array_equal(again[k], w, err_msg="%s %s (second run)" % (name, k))
