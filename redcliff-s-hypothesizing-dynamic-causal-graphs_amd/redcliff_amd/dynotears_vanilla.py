"""DYNOTEARS comparison baseline (models/dynotears_vanilla.py and models/causalnex_dynotears_vanilla.py of the
reference; Pamfil et al., "DYNOTEARS: Structure Learning from Time-Series Data", AISTATS 2020).

The reference runs one complete augmented-Lagrangian solve per training recording and sums the lagged matrices, so
a fit is hundreds to thousands of small independent problems.  Here they form one batch:

* ``from_numpy_dynamic(X, Xlags, ...)`` -> ``(sm, w_est, a_est)``, the reference's call for one problem;
* ``from_numpy_dynamic_many(X, Xlags, ...)`` -> ``(W [P, d, d], A [P, p d, d], info)`` for P problems of one shape,
  with per-problem ``lambda_w`` / ``lambda_a``;
* ``DYNOTEARS_Model`` with the reference's constructor, ``fit``, ``GC``, ``evaluate`` and pickle file;
* ``fit_dynotears_baselines(models, X_trains, ...)``: every recording of every data set (and so every lambda of a
  grid) in one batch per shape.

Variables: ``wa`` of 2 (p + 1) d^2 entries >= 0; rows [0, d) of its (2 (p + 1) d, d) view are W+, rows [d, 2d) W-,
then per lag A+ followed by A-.  Both copies of W's diagonal and the tabu entries are fixed at 0.

REDCLIFF_DYNOTEARS_PATH=fused|host|auto selects the route (auto: the device when a GPU and the library are present
and the shape is inside redcliff_dynotears_supported).  The fused route is redcliff_dynotears_run
(csrc/rc_dynotears.hip): a projected limited-memory quasi-Newton solver with L-BFGS-B's stopping rules, launched
``evals_per_launch`` evaluations at a time until no problem remains.  The host route restates the reference's loop on
``scipy.optimize.minimize(method="L-BFGS-B")``; it serves shapes outside the limits.  The two agree to within the
reference's own sensitivity to rounding and stopping tolerance (about 1e-3), not bit for bit.
"""
import os
import time
import warnings

import numpy as np

CONVERGED, MAXITER, RHO_CAP, NONFINITE = 0, 1, 2, 3
STATUS_NAMES = ("CONVERGED", "MAXITER", "RHO_CAP", "NONFINITE")
# scipy's L-BFGS-B defaults (the reference passes none)
SOLVER_DEFAULTS = dict(m=10, factr=1e7, pgtol=1e-5, maxiter=15000, maxfun=15000, maxls=20)
DEFAULT_EVALS_PER_LAUNCH = 1024   # profiles/dynotears_fit.json: the smallest value within 5 % of a single launch on a D4IC-shaped call
RHO_MAX = 1e20
COUNT_NAMES = ("outer_iterations", "inner_solves", "qn_iterations", "evaluations", "nonfinite_trials", "launches")
STAT_NAMES = ("h", "rho", "alpha", "f", "pg_norm", "failed_line_searches")


def fixed_mask(d, p, tabu_edges=None, tabu_parent_nodes=None, tabu_child_nodes=None):
    """uint8 [2 (p + 1) d^2]: 1 where the bounds are (0, 0).  (lag, i, j) in tabu_edges fixes entry [i, j] of W (lag 0)
    or of A_lag; a tabu parent fixes its row everywhere, a tabu child its column."""
    blocks = np.zeros((p + 1, d, d), dtype=bool)
    blocks[0][np.arange(d), np.arange(d)] = True
    for lag, i, j in (tabu_edges or ()):
        if 0 <= lag <= p:
            blocks[lag, i, j] = True
    for i in (tabu_parent_nodes or ()):
        blocks[:, i, :] = True
    for j in (tabu_child_nodes or ()):
        blocks[:, :, j] = True
    return np.repeat(blocks.reshape(p + 1, 1, d * d), 2, axis=1).reshape(-1).astype(np.uint8)


def reshape_wa(wa, d, p):
    """(W [d, d], A [p d, d]) of a variable vector."""
    blocks = np.asarray(wa, dtype=np.float64).reshape(2 * (p + 1), d, d)
    return blocks[0] - blocks[1], (blocks[2::2] - blocks[3::2]).reshape(p * d, d)


def device_supported(d, p):
    from . import _native as nat
    return bool(nat.lib().redcliff_dynotears_supported(int(d), int(p)))


def _route(d, p):
    forced = os.environ.get("REDCLIFF_DYNOTEARS_PATH", "") or "auto"
    if forced not in ("auto", "host", "fused"):
        raise ValueError("REDCLIFF_DYNOTEARS_PATH must be fused, host or auto")
    if forced == "host":
        return "host"
    import torch
    try:
        fused = torch.cuda.is_available() and device_supported(d, p)
    except ImportError:
        if forced == "fused":
            raise
        fused = False
    if forced == "fused" and not fused:
        raise RuntimeError("REDCLIFF_DYNOTEARS_PATH=fused: no GPU, or shape outside redcliff_dynotears_supported (d=%d p=%d)" % (d, p))
    return "fused" if fused else "host"


def _check_shapes(xs, ls):
    """The reference's validity errors (_learn_dynamic_structure), on shapes alone."""
    if int(np.prod(xs)) == 0:
        raise ValueError("Input data X is empty, cannot learn any structure")
    if int(np.prod(ls)) == 0:
        raise ValueError("Input data Xlags is empty, cannot learn any structure")
    if xs[-2] != ls[-2]:
        raise ValueError("Input data X and Xlags must have the same number of rows")
    if ls[-1] % xs[-1] != 0:
        raise ValueError("Number of columns of Xlags must be a multiple of number of columns of X")


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


# ---------------------------------------------------------------- host route

def _host_solve(X, Xl, fixed, lam_w, lam_a, max_iter, h_tol, rho0, alpha0, solver):
    """One problem by the reference's loop on scipy's L-BFGS-B; returns (wa, status, stats, counts)."""
    import scipy.linalg
    import scipy.optimize
    X = np.asarray(X, dtype=np.float64)
    Xl = np.asarray(Xl, dtype=np.float64)
    n, d = X.shape
    p = Xl.shape[1] // d
    nw = 2 * d * d
    eye = np.eye(d)
    nv = 2 * (p + 1) * d * d
    if not (np.isfinite(X).all() and np.isfinite(Xl).all()):
        return np.full(nv, np.nan), NONFINITE, [np.nan] * 6, [0] * 6
    bounds = [(0, 0) if f else (0, None) for f in fixed]
    state = dict(rho=float(rho0), alpha=float(alpha0), evals=0, its=0, solves=0)

    def h_of(W):
        return np.trace(scipy.linalg.expm(W * W)) - d

    def fun(wa):
        state["evals"] += 1
        W, A = reshape_wa(wa, d, p)
        R = X.dot(eye - W) - Xl.dot(A)
        E = scipy.linalg.expm(W * W)
        h = np.trace(E) - d
        f = 0.5 / n * np.square(np.linalg.norm(R, "fro")) + 0.5 * state["rho"] * h * h + state["alpha"] * h
        f += lam_w * wa[:nw].sum() + lam_a * wa[nw:].sum()
        gw = -1.0 / n * X.T.dot(R) + (state["rho"] * h + state["alpha"]) * E.T * W * 2
        ga = (-1.0 / n * Xl.T.dot(R)).reshape(p, d * d)
        g = np.concatenate([gw.ravel() + lam_w, -gw.ravel() + lam_w, (np.hstack((ga, -ga)) + lam_a).ravel()])
        return f, g

    opts = dict(maxcor=solver["m"], ftol=solver["factr"] * np.finfo(float).eps, gtol=solver["pgtol"], maxiter=solver["maxiter"],
                maxfun=solver["maxfun"], maxls=solver["maxls"])
    wa_est = np.zeros(nv)
    wa_new = np.zeros(nv)
    h_value = h_new = np.inf
    outer = 0
    last = None
    for _ in range(max_iter):
        while state["rho"] < RHO_MAX and (h_new > 0.25 * h_value or h_new == np.inf):
            last = scipy.optimize.minimize(fun, wa_est, method="L-BFGS-B", jac=True, bounds=bounds, options=opts)
            wa_new = last.x
            state["solves"] += 1
            state["its"] += int(last.nit)
            h_new = h_of(reshape_wa(wa_new, d, p)[0])
            if h_new > 0.25 * h_value:
                state["rho"] *= 10
        wa_est = wa_new
        h_value = h_new
        state["alpha"] += state["rho"] * h_value
        outer += 1
        if h_value <= h_tol:
            break
    status = CONVERGED if h_value <= h_tol else RHO_CAP if state["rho"] >= RHO_MAX else MAXITER
    if status != CONVERGED:
        warnings.warn("Failed to converge. Consider increasing max_iter.")
    f_last = float(last.fun) if last is not None else np.nan
    return wa_est, status, [float(h_value), state["rho"], state["alpha"], f_last, np.nan, 0.0], [outer, state["solves"], state["its"],
                                                                                                 state["evals"], 0, 0]


def _host_many(X, Xl, n_rows, lam_w, lam_a, fixed, max_iter, h_tol, rho0, alpha0, solver):
    if _is_tensor(X):
        X = X.detach().cpu().numpy()
    if _is_tensor(Xl):
        Xl = Xl.detach().cpu().numpy()
    P, _, d = X.shape
    p = Xl.shape[2] // d
    nv = 2 * (p + 1) * d * d
    wa = np.zeros((P, nv))
    status = np.zeros(P, dtype=np.int32)
    stats = np.zeros((P, 6))
    counts = np.zeros((P, 6), dtype=np.int32)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for b in range(P):
            wa[b], status[b], stats[b], counts[b] = _host_solve(X[b, :n_rows[b]], Xl[b, :n_rows[b]], fixed, lam_w[b], lam_a[b], max_iter,
                                                                h_tol, rho0, alpha0, solver)
    return wa, status, stats, counts


# ---------------------------------------------------------------- fused route

def _device_view(x, dev):
    """A device tensor whose last dimension is contiguous; a device tensor passes through without a copy."""
    import torch
    if not _is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float64)
    x = x.to(dev)
    if x.stride(-1) != 1 or x.stride(0) < 0 or x.stride(1) < 0:
        x = x.contiguous()
    return x


def _device_many(X, Xl, n_rows, lam_w, lam_a, fixed, max_iter, h_tol, rho0, alpha0, solver, evals_per_launch, device):
    import ctypes
    import torch
    from . import _native as nat
    dev = torch.device(device) if device is not None else (X.device if _is_tensor(X) and X.is_cuda else torch.device("cuda"))
    Xd = _device_view(X, dev)
    Xld = _device_view(Xl, dev)
    if Xd.dtype != Xld.dtype:
        Xd, Xld = Xd.to(torch.float64), Xld.to(torch.float64)
    P, _, d = Xd.shape
    p = Xld.shape[2] // d
    nv = 2 * (p + 1) * d * d
    L = nat.lib()
    m = int(solver["m"])
    need = int(L.redcliff_dynotears_ws_bytes(P, d, p, m))
    if need == 0:
        raise RuntimeError("redcliff_dynotears_ws_bytes: " + L.redcliff_last_error().decode(errors="replace"))
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        ws = torch.empty((need + 7) // 8, **f64)
        W = torch.empty((P, d, d), **f64)
        A = torch.empty((P, p * d, d), **f64)
        wa = torch.empty((P, nv), **f64)
        stats = torch.empty((P, 6), **f64)
        status = torch.full((P,), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros((P, 6), dtype=torch.int32, device=dev)
        remaining = torch.zeros(1, dtype=torch.int32, device=dev)
        rows_d = torch.as_tensor(np.asarray(n_rows, dtype=np.int32), device=dev)
        lw_d = torch.as_tensor(np.asarray(lam_w, dtype=np.float64), device=dev)
        la_d = torch.as_tensor(np.asarray(lam_a, dtype=np.float64), device=dev)
        fx_d = torch.as_tensor(np.asarray(fixed, dtype=np.uint8), device=dev)
        a = nat.DynotearsArgs()
        a.P, a.d, a.p = P, d, p
        a.dtype = 0 if Xd.dtype == torch.float32 else 1
        a.start, a.evals_per_launch = 1, int(evals_per_launch)
        a.max_iter, a.m, a.maxiter, a.maxfun, a.maxls = int(max_iter), m, int(solver["maxiter"]), int(solver["maxfun"]), int(solver["maxls"])
        a.h_tol, a.rho0, a.alpha0, a.rho_max = float(h_tol), float(rho0), float(alpha0), RHO_MAX
        a.factr, a.pgtol = float(solver["factr"]), float(solver["pgtol"])
        a.X, a.x_pstride, a.x_rstride = Xd.data_ptr(), Xd.stride(0), Xd.stride(1)
        a.Xlags, a.xl_pstride, a.xl_rstride = Xld.data_ptr(), Xld.stride(0), Xld.stride(1)
        a.n_rows, a.lambda_w, a.lambda_a, a.fixed = rows_d.data_ptr(), lw_d.data_ptr(), la_d.data_ptr(), fx_d.data_ptr()
        a.W, a.A, a.wa = W.data_ptr(), A.data_ptr(), wa.data_ptr()
        a.status, a.stats, a.counts, a.remaining = status.data_ptr(), stats.data_ptr(), counts.data_ptr(), remaining.data_ptr()
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 8
        stream = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # every evaluation belongs to a line search of at most maxls trials or opens an inner solve: a bound on the launches
        cap = 16 + (int(max_iter) + 25) * (int(solver["maxfun"]) + int(solver["maxls"]) + 2) // int(evals_per_launch)
        launches = 0
        e0.record()
        while True:
            nat.check(L.redcliff_dynotears_run(ctypes.byref(a), stream), "dynotears_run")
            launches += 1
            a.start = 0
            left = int(remaining.item())
            if left == 0:
                break
            if launches >= cap:
                raise RuntimeError("dynotears: %d problems unfinished after %d launches" % (left, launches))
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
    del Xd, Xld, ws
    return W.cpu().numpy(), A.cpu().numpy(), wa.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy(), counts.cpu().numpy(), launches, ms


# ---------------------------------------------------------------- public calls

def _per_problem(v, P, name):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 0:
        return np.full(P, float(v))
    if v.shape != (P,):
        raise ValueError("%s must be a scalar or one value per problem" % name)
    return np.ascontiguousarray(v)


def from_numpy_dynamic_many(X, Xlags, lambda_w=0.1, lambda_a=0.1, max_iter=100, h_tol=1e-8, w_threshold=0.0, tabu_edges=None,
                            tabu_parent_nodes=None, tabu_child_nodes=None, n_rows=None, rho0=1.0, alpha0=0.0, solver=None,
                            evals_per_launch=None, device=None):
    """P problems of one shape.  X [P, n, d] and Xlags [P, n, p d]: numpy arrays or torch tensors (host or device),
    float32 or float64; on the fused route device tensors are read in place through their strides.  lambda_w / lambda_a:
    a scalar or one value per problem.  n_rows: rows of each problem (default n).  solver: overrides of SOLVER_DEFAULTS.
    Returns (W [P, d, d], A [P, p d, d], info); info has the route, per-problem status, stats and counts, the variable
    vectors ``wa`` and the time."""
    t_all = time.perf_counter()
    xs, ls = tuple(X.shape), tuple(Xlags.shape)
    if len(xs) != 3 or len(ls) != 3 or xs[0] != ls[0]:
        raise ValueError("X and Xlags must be [P, n, d] and [P, n, p d]")
    _check_shapes(xs, ls)
    P, n, d = xs
    p = ls[2] // d
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    opts = dict(SOLVER_DEFAULTS)
    opts.update(solver or {})
    if float(rho0) == 0.0 and int(max_iter) != 1:
        raise ValueError("rho0 = 0 never grows: it is accepted with max_iter = 1 only")
    lam_w, lam_a = _per_problem(lambda_w, P, "lambda_w"), _per_problem(lambda_a, P, "lambda_a")
    rows = np.full(P, n, dtype=np.int32) if n_rows is None else np.ascontiguousarray(n_rows, dtype=np.int32)
    if rows.shape != (P,) or rows.min() < 1 or rows.max() > n:
        raise ValueError("n_rows must hold one count in [1, n] per problem")
    fixed = fixed_mask(d, p, tabu_edges, tabu_parent_nodes, tabu_child_nodes)
    route = _route(d, p)
    if route == "fused" and int(opts["m"]) > 16:
        if (os.environ.get("REDCLIFF_DYNOTEARS_PATH", "") or "auto") == "fused":
            raise RuntimeError("REDCLIFF_DYNOTEARS_PATH=fused: m = %d outside the kernel's limit of 16" % opts["m"])
        route = "host"
    info = dict(route=route, d=d, p=p, P=P)
    if route == "fused":
        epl = DEFAULT_EVALS_PER_LAUNCH if evals_per_launch is None else int(evals_per_launch)
        W, A, wa, status, stats, counts, launches, ms = _device_many(X, Xlags, rows, lam_w, lam_a, fixed, max_iter, h_tol, rho0, alpha0, opts,
                                                                     epl, device)
        info.update(launches=launches, kernel_ms=ms, evals_per_launch=epl)
    else:
        wa, status, stats, counts = _host_many(X, Xlags, rows, lam_w, lam_a, fixed, int(max_iter), float(h_tol), rho0, alpha0, opts)
        W = np.empty((P, d, d))
        A = np.empty((P, p * d, d))
        for b in range(P):
            W[b], A[b] = reshape_wa(wa[b], d, p)
    if w_threshold:
        W[np.abs(W) < w_threshold] = 0
        A[np.abs(A) < w_threshold] = 0
    info.update(status=status, status_names=[STATUS_NAMES[s] for s in status], wa=wa,
                stats={k: stats[:, i] for i, k in enumerate(STAT_NAMES)}, counts={k: counts[:, i] for i, k in enumerate(COUNT_NAMES)},
                time_s=time.perf_counter() - t_all)
    return W, A, info


def matrices_to_structure_model(w_est, a_est):
    """The learnt graph: nodes ``{var}_lag{l}``, an edge per non-zero weight.  A causalnex StructureModel when causalnex
    imports, otherwise a networkx DiGraph with the same nodes, edges and weights."""
    try:
        from causalnex.structure import StructureModel as Graph
    except ImportError:
        from networkx import DiGraph as Graph
    d = a_est.shape[1]
    names = ["%d_lag%d" % (var, lag) for lag in range(1 + a_est.shape[0] // d) for var in range(d)]
    sm = Graph()
    sm.add_nodes_from(names)
    sm.add_edges_from([(names[i], names[j], {"weight": w_est[i, j]}) for i in range(d) for j in range(d) if w_est[i, j] != 0])
    sm.add_edges_from([(names[i + d], names[j], {"weight": a_est[i, j]}) for i in range(a_est.shape[0]) for j in range(d)
                       if a_est[i, j] != 0])
    return sm


def from_numpy_dynamic(X, Xlags, lambda_w=0.1, lambda_a=0.1, max_iter=100, h_tol=1e-8, w_threshold=0.0, tabu_edges=None,
                       tabu_parent_nodes=None, tabu_child_nodes=None):
    """The reference's call: one problem, X [n, d] and Xlags [n, p d]; returns (sm, w_est, a_est)."""
    xs, ls = tuple(X.shape), tuple(Xlags.shape)
    if len(xs) != 2 or len(ls) != 2:
        raise ValueError("X and Xlags must be two-dimensional")
    _check_shapes(xs, ls)
    W, A, info = from_numpy_dynamic_many(X[None], Xlags[None], lambda_w, lambda_a, max_iter, h_tol, w_threshold, tabu_edges,
                                         tabu_parent_nodes, tabu_child_nodes)
    if info["status"][0] not in (CONVERGED, NONFINITE) and info["route"] == "fused":
        warnings.warn("Failed to converge. Consider increasing max_iter.")
    return matrices_to_structure_model(W[0], A[0]), W[0], A[0]


class DYNOTEARS_Model():
    def __init__(self, lambda_w=0.1, lambda_a=0.1, max_iter=100, h_tol=1e-8, w_threshold=0.0, tabu_edges=None, tabu_parent_nodes=None,
                 tabu_child_nodes=None):
        self.lambda_w = lambda_w
        self.lambda_a = lambda_a
        self.max_iter = max_iter
        self.h_tol = h_tol
        self.w_threshold = w_threshold
        self.tabu_edges = tabu_edges
        self.tabu_parent_nodes = tabu_parent_nodes
        self.tabu_child_nodes = tabu_child_nodes
        self.a_est = None

    def GC(self):
        return self.a_est

    def save_checkpoint(self, save_dir):
        """Writes final_best_model.pkl (the reference's version stops on an undefined name before its plot; plots are
        skipped here as in every fit of this package)."""
        import torch
        torch.save(self, os.path.join(save_dir, "final_best_model.pkl"))   # a pickle, read back by torch.load or pickle.load

    def fit(self, save_path, X_train, X_val, lag_size=1, GC_orig=None, save_a_est=True):
        return fit_dynotears_baselines([self], [X_train], [save_path], X_vals=[X_val], lag_size=lag_size, GC_origs=[GC_orig],
                                       save_a_est=save_a_est)["val_losses"][0]

    def evaluate(self, X, save_path, GC_orig, lag_size=1):
        print("dynotears_vanilla.DYNOTEARS_Model.evaluate: WARNING - evaluate function NOT implemented, returning None!!!!", flush=True)
        return None


def _group_key(model, x):
    t = lambda v: None if v is None else tuple(sorted(tuple(e) if isinstance(e, (list, tuple)) else e for e in v))  # noqa: E731
    return (tuple(x.shape[1:]), str(x.dtype), int(model.max_iter), float(model.h_tol), t(model.tabu_edges), t(model.tabu_parent_nodes),
            t(model.tabu_child_nodes))


def fit_dynotears_baselines(models, X_trains, save_paths=None, X_vals=None, lag_size=1, GC_origs=None, save_a_est=True, device=None,
                            evals_per_launch=None):
    """Fit models[i] on X_trains[i] ([recordings, T, d]).  Every recording of every data set whose shape, tabu lists,
    max_iter and h_tol agree goes into one batch (models may differ in lambda: a lambda grid is one batch).  As in the
    reference, recording s gives X = X_train[s, :-lag_size] and Xlags = X_train[s, lag_size:], the lagged matrices are
    summed and divided by the number of nodes, and final_best_model.pkl is written when a save path is given.
    Returns {"val_losses", "infos"}."""
    n = len(models)
    save_paths = save_paths if save_paths is not None else [None] * n
    X_vals = X_vals if X_vals is not None else [None] * n
    GC_origs = GC_origs if GC_origs is not None else [None] * n
    lag = int(lag_size)
    groups = {}
    for i, (model, x) in enumerate(zip(models, X_trains)):
        if len(x.shape) != 3:
            raise ValueError("X_train must be [recordings, T, d]")
        _check_shapes((x.shape[0], max(x.shape[1] - lag, 0), x.shape[2]), (x.shape[0], max(x.shape[1] - lag, 0), x.shape[2]))
        groups.setdefault(_group_key(model, x), []).append(i)
    infos = [None] * n
    for members in groups.values():
        first = models[members[0]]
        if len(members) == 1:
            data = X_trains[members[0]]
        elif all(_is_tensor(X_trains[i]) for i in members):
            import torch
            data = torch.cat([X_trains[i] for i in members], dim=0)
        else:
            data = np.concatenate([X_trains[i].detach().cpu().numpy() if _is_tensor(X_trains[i]) else np.asarray(X_trains[i]) for i in members])
        sizes = [int(X_trains[i].shape[0]) for i in members]
        lam_w = np.concatenate([np.full(s, float(models[i].lambda_w)) for i, s in zip(members, sizes)])
        lam_a = np.concatenate([np.full(s, float(models[i].lambda_a)) for i, s in zip(members, sizes)])
        _, A, info = from_numpy_dynamic_many(data[:, :-lag], data[:, lag:], lam_w, lam_a, first.max_iter, first.h_tol, 0.0, first.tabu_edges,
                                             first.tabu_parent_nodes, first.tabu_child_nodes, device=device, evals_per_launch=evals_per_launch)
        at = 0
        for i, s in zip(members, sizes):
            a = A[at:at + s].copy()
            thr = models[i].w_threshold
            if thr:
                a[np.abs(a) < thr] = 0
            d = a.shape[-1]
            total = np.zeros((d, d))
            for r in range(s):   # the reference's order of additions
                total = total + a[r]
            if save_a_est:
                models[i].a_est = total / (1.0 * d)
            infos[i] = dict(route=info["route"], status=info["status"][at:at + s], time_s=info["time_s"], batch=int(sum(sizes)),
                            counts={k: v[at:at + s] for k, v in info["counts"].items()})
            at += s
    losses = []
    for i, model in enumerate(models):
        loss = None
        if GC_origs[i] is not None:
            loss = model.evaluate(X_vals[i], save_paths[i], GC_origs[i], lag_size=lag)
        if save_paths[i] is not None:
            model.save_checkpoint(save_paths[i])
        losses.append(loss)
    return dict(val_losses=losses, infos=infos)
