"""Shared by tests/test_dynotears_host.py, tests/test_gpu_dynotears.py and tests/golden/make_dynotears_golden.py:
the scenarios of tests/golden/dynotears.npz, the bound both routes are held to, and a numpy evaluation of the
DYNOTEARS objective, its gradient and the projected-gradient norm that is independent of the code under test.

The bound of a recording is ``MARGIN * max(spread, tolgap)`` elementwise on (W, A): ``spread`` is the largest
change of the reference's own result among 8 copies of the float32 input moved by one ulp at random, ``tolgap``
its change when the inner solves stop at ftol 1e-12 / gtol 1e-8 instead of scipy's defaults.  Both are measured
by the generator on the reference alone.  MARGIN = 10 is the margin DESIGN section 21 uses for ill-posed shapes.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "dynotears.npz")
MARGIN = 10.0
_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(PATH)
    return _G


def meta():
    return json.loads(str(golden()["meta"]))


def scenario(name):
    sc = dict(meta()["scenarios"][name])
    G = golden()
    for k in G.files:
        if k.startswith(name + "/"):
            sc[k.split("/", 1)[1]] = G[k]
    sc["name"] = name
    return sc


def names():
    return list(meta()["scenarios"])


def problem(sc, r):
    """(X, Xlags) of recording r, float32, as the reference's callers slice them."""
    return split(sc["data"][r], sc["p"])


def split(x, p, lag=1):
    """p == 1: the model's slices (X = x[:-lag], Xlags = x[lag:], the reference's order).  p > 1: X = x[p:] and
    Xlags = [x[p-1:-1] | ... | x[:-p]], the usual lag stack."""
    if p == 1:
        return x[:-lag], x[lag:]
    T = x.shape[0]
    return x[p:], np.concatenate([x[p - k:T - k] for k in range(1, p + 1)], axis=1)


def tabu(sc):
    t = sc.get("tabu") or {}
    edges = [tuple(e) for e in t["edges"]] if t.get("edges") else None
    return dict(tabu_edges=edges, tabu_parent_nodes=t.get("parents") or None, tabu_child_nodes=t.get("children") or None)


def bound(sc, r):
    return MARGIN * max(float(sc["spread"][r]), float(sc["tolgap"][r]))


def fixed_mask(d, p, tabu_edges=None, tabu_parent_nodes=None, tabu_child_nodes=None):
    """bool [2 (p + 1) d^2]: entries whose bounds are (0, 0), in the layout of the reference's bounds list."""
    te = set(tuple(e) for e in tabu_edges) if tabu_edges else set()
    tp = set(tabu_parent_nodes) if tabu_parent_nodes else set()
    tc = set(tabu_child_nodes) if tabu_child_nodes else set()
    out = []
    for k in range(p + 1):
        blk = np.zeros((d, d), dtype=bool)
        for i in range(d):
            for j in range(d):
                blk[i, j] = (k == 0 and i == j) or (k, i, j) in te or i in tp or j in tc
        out += [blk.ravel(), blk.ravel()]
    return np.concatenate(out)


def reshape_wa(wa, d, p):
    """(W [d, d], A [p d, d]) of the variable vector: rows [0, d) of its (2 (p + 1) d, d) view are W+, rows [d, 2d)
    W-, then per lag A+ followed by A-."""
    blocks = np.asarray(wa, dtype=np.float64).reshape(2 * (p + 1), d, d)
    W = blocks[0] - blocks[1]
    A = np.concatenate([blocks[2 + 2 * k] - blocks[3 + 2 * k] for k in range(p)], axis=0)
    return W, A


def h_of(W):
    import scipy.linalg
    return float(np.trace(scipy.linalg.expm(W * W)) - W.shape[0])


def objective(wa, X, Xlags, rho, alpha, lambda_w, lambda_a):
    """(f, gradient) of the augmented Lagrangian at wa, from the residual in double."""
    import scipy.linalg
    X = np.asarray(X, dtype=np.float64)
    Xl = np.asarray(Xlags, dtype=np.float64)
    n, d = X.shape
    p = Xl.shape[1] // d
    W, A = reshape_wa(wa, d, p)
    R = X @ (np.eye(d) - W) - Xl @ A
    E = scipy.linalg.expm(W * W)
    h = np.trace(E) - d
    f = 0.5 / n * np.sum(R * R) + 0.5 * rho * h * h + alpha * h + lambda_w * wa[:2 * d * d].sum() + lambda_a * wa[2 * d * d:].sum()
    gw = -(X.T @ R) / n + (rho * h + alpha) * E.T * W * 2
    ga = (-(Xl.T @ R) / n).reshape(p, d, d)
    g = [gw.ravel() + lambda_w, -gw.ravel() + lambda_w]
    for k in range(p):
        g += [ga[k].ravel() + lambda_a, -ga[k].ravel() + lambda_a]
    return float(f), np.concatenate(g)


def proj_grad_norm(wa, g, fixed):
    """Infinity norm of the projected gradient x - P(x - g) for the bounds x >= 0 (free) and x == 0 (fixed), the
    quantity L-BFGS-B's pgtol is tested on: g where g < 0, min(x, g) elsewhere."""
    pg = np.where(fixed, 0.0, np.where(g < 0, g, np.minimum(wa, g)))
    return float(np.abs(pg).max())
