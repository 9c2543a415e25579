"""The regime-aware tidybench comparison baselines: SLARAC and QRBS, and (second half of the file) LASAR.

Restated from the reference's ``tidybench/slarac.py``, ``tidybench/qrbs.py``, ``tidybench/utils.py`` and
``run_tidybench_experiment`` / ``prepare_data_for_modeling`` of ``evaluate/eval_algs_by_d4icMSNR.py``.

Both algorithms are a few hundred small regressions on bootstrap resamples of one lag-stacked series.  Every
fit is a Gram matrix over gathered rows followed by a tiny symmetric solve, so a whole batch of data sets runs
in one native call (``redcliff_tidybench_run``, csrc/rc_tidybench.hip); a numpy route computes the same on the
host.  What is random is drawn on the host from numpy's global generator with the reference's calls in the
reference's order, so a seeded call reproduces the reference's result and leaves the generator where the
reference leaves it:

* SLARAC: the full fit's effective lag; ``choice(subsample_sizes, n_subsamples)``; then per subsample
  ``randint(0, n, size=(n_samples,))`` (what ``sklearn.utils.resample`` draws) and the fit's effective lag.
* QRBS: one ``randint(0, n, size=(k,))`` per resample, k = floor(0.7 T).

The reference's "feasible lag" heuristic takes ``max(maxlags, feasiblelag)`` with ``feasiblelag <= maxlags``, so
it never changes the range the effective lag is drawn from; the draw is kept because it consumes the stream.

A fit is solved by a Cholesky factorisation that tracks ``min_j pivot_j / G_jj``.  Below ``PIVOT_MIN`` (or with
a non-positive pivot or diagonal entry) the fit is SINGULAR and is recomputed with the reference's own
operations (gathered rows, ``Z Z^T``, ``numpy.linalg.lstsq``), which returns the minimum-norm solution the
reference returns.  Regime-masked series make this case common.

REDCLIFF_TIDYBENCH_PATH=fused|host|auto selects the route (auto: the device when a GPU and the library are
present and the shape is supported).  sklearn and scipy are not imported.

LASAR (``lasar``, ``lasar_many``, ``run_lasar_experiment``) is ``tidybench/lasar.py``: per fit and target sklearn's
``LassoLarsCV`` selects the parents with a positive coefficient and a least-squares refit on them gives the scores.
Its draws are SLARAC's without the effective lags.  The device route (``redcliff_lasar_run``, csrc/rc_lasar.hip) runs
every fold path, alpha choice, final path and refit of a batch from per-fold Gram sums; the host route restates what
sklearn executes, branch by branch, and also recomputes the (series, fit, target) triples the device flags SINGULAR
or DEGENERATE.
"""
import os
import time

import numpy as np

INV_GOLDEN_RATIO = 2 / (1 + np.sqrt(5))
DEFAULT_SUBSAMPLE_SIZES = [INV_GOLDEN_RATIO ** (1 / k) for k in [1, 2, 3, 6]]
OK, SINGULAR, NONFINITE = 0, 1, 2
PIVOT_MIN = 1e-8          # TB_PIVOT_MIN of csrc/rc_tidybench.h
CHUNK_ROWS = 512          # TB_CH
WORKSPACE_BUDGET_BYTES = 256 << 20   # a larger batch runs as several calls over groups of fits (same bits)
_SLARAC, _QRBS = 0, 1


def _max_over_lags(x):
    return x.max(axis=1).T


# ----------------------------------------------------------------------------------------
# pre- and post-processing (tidybench/utils.py common_pre_post_processing)
# ----------------------------------------------------------------------------------------
def standardise(X, axis=0, keepdims=True, copy=False):
    if copy:
        X = np.copy(X)
    X -= X.mean(axis=axis, keepdims=keepdims)
    X /= X.std(axis=axis, keepdims=keepdims)
    return X


def _pop_processing(kwargs):
    return {k: bool(kwargs.pop(k, False)) for k in ("pre_normalise", "post_standardise", "post_zeroonescaling", "post_edgeprior")}


def _post(scores, proc):
    if proc["post_standardise"]:
        scores = standardise(scores, axis=None)
    if proc["post_zeroonescaling"]:
        scores = (scores - scores.min()) / (scores.max() - scores.min())
    if proc["post_edgeprior"]:
        scores /= scores.mean()
    return scores


def _host_series(datas, proc, missing_values):
    """[P, T, N] float64 host copy of the input (never the caller's memory), pre-normalised if asked, checked
    for non-finite values; and the caller's device tensor when it can be used as it is."""
    dev = None
    if hasattr(datas, "detach"):
        t = datas.detach()
        if t.is_cuda and str(t.dtype) == "torch.float64" and t.is_contiguous() and not proc["pre_normalise"]:
            dev = t
        x = t.cpu().numpy()
    else:
        x = np.asarray(datas)
    if x.ndim != 3:
        raise ValueError("data must be [T, N] (or [P, T, N] for the *_many calls)")
    if x.dtype.kind != "f":
        x = x.astype(np.float64)
    x = np.array(x, copy=True)
    if proc["pre_normalise"]:
        for b in range(x.shape[0]):   # in the data's own precision, as the reference's in-place standardise
            standardise(x[b])
    x = np.ascontiguousarray(x, dtype=np.float64)
    ok = np.isfinite(x) if missing_values is None else (np.isfinite(x) | (x == missing_values))
    if not ok.all():
        raise ValueError("Input contains NaN or infinity.")
    return x, dev


# ----------------------------------------------------------------------------------------
# the draws
# ----------------------------------------------------------------------------------------
class _Plan(object):
    """The fits of P data sets: idx [P, S, maxcnt] int32, count [P, S] (-1 = all rows in order), ncols [P, S]."""

    def __init__(self, mode, P, S, T, N, lags, maxcnt):
        self.mode, self.P, self.S, self.T, self.N, self.lags = mode, P, S, T, N, lags
        self.n = T - lags
        self.idx = np.zeros((P, S, max(maxcnt, 1)), dtype=np.int32)
        self.count = np.zeros((P, S), dtype=np.int32)
        self.ncols = np.full((P, S), lags * N + 1, dtype=np.int32)
        self.dout = lags * N + (1 if mode == _SLARAC else 0)

    def rows(self, b, s):
        c = int(self.count[b, s])
        return None if c < 0 else self.idx[b, s, :c]

    def eff_count(self):
        return np.where(self.count < 0, self.n, self.count)


def _slarac_plan(P, T, N, maxlags, n_subsamples, subsample_sizes):
    n = T - maxlags
    sizes = list(subsample_sizes)
    maxcnt = max([n] + [int(np.round(s * T)) for s in sizes]) if n_subsamples else n
    plan = _Plan(_SLARAC, P, 1 + n_subsamples, T, N, maxlags, maxcnt)
    efflags = np.arange(1, maxlags + 1)
    for b in range(P):
        plan.count[b, 0] = -1
        plan.ncols[b, 0] = np.random.choice(efflags) * N + 1
        for s, size in enumerate(np.random.choice(sizes, n_subsamples)):
            k = int(np.round(size * T))
            plan.idx[b, s + 1, :k] = np.random.randint(0, n, size=(k,))
            plan.count[b, s + 1] = k
            plan.ncols[b, s + 1] = np.random.choice(efflags) * N + 1
    return plan


def _qrbs_plan(P, T, N, lags, n_resamples):
    n = T - lags
    k = int(np.floor(T * 0.7))
    plan = _Plan(_QRBS, P, n_resamples, T, N, lags, k)
    plan.count[:] = k
    for b in range(P):
        for s in range(n_resamples):
            plan.idx[b, s] = np.random.randint(0, n, size=(k,))
    return plan


# ----------------------------------------------------------------------------------------
# host route
# ----------------------------------------------------------------------------------------
def _lag_stack(x, lags):
    """Z [n, 1 + lags N] = [1, x_{t-1}, ..., x_{t-lags}] and the rows x_t, t = lags .. T - 1."""
    T, N = x.shape
    n = T - lags
    Z = np.empty((n, 1 + lags * N))
    Z[:, 0] = 1.0
    for k in range(1, lags + 1):
        Z[:, 1 + (k - 1) * N:1 + k * N] = x[lags - k:T - k]
    return Z, x[lags:]


def _pivot_cholesky(G):
    """Upper factor U (G = U^T U) by the right-looking recurrence of k_tb_solve, min_j pivot_j / G_jj and the status.
    Stops at the first pivot the rule refuses."""
    A = np.array(G, dtype=np.float64, copy=True)
    if not np.isfinite(A).all():
        return None, 0.0, NONFINITE
    d0 = np.diag(A).copy()
    c = A.shape[0]
    ratio = np.inf
    for j in range(c):
        piv, g = A[j, j], d0[j]
        if not (g > 0.0) or not (piv > 0.0):
            return None, (piv / g if g > 0.0 else 0.0), SINGULAR
        ratio = min(ratio, piv / g)
        if piv / g < PIVOT_MIN:
            return None, ratio, SINGULAR
        d = np.sqrt(piv)
        A[j, j] = d
        A[j, j + 1:] /= d
        A[j + 1:, j + 1:] -= np.outer(A[j, j + 1:], A[j, j + 1:])
    return np.triu(A), ratio, OK


def _solve_spd(G, R):
    U, ratio, st = _pivot_cholesky(G)
    if st != OK:
        return None, ratio, st
    return np.linalg.solve(U, np.linalg.solve(U.T, R)), ratio, OK


def _weights(plan, b, s, rowok):
    rows = plan.rows(b, s)
    if rows is None:
        w = np.ones(plan.n)
    else:
        w = np.bincount(rows, minlength=plan.n).astype(np.float64)
    if rowok is not None:
        w = w * rowok
    return w


def _slarac_min_norm(x, lags, rows, c, rowok=None):
    """The reference's own operations for one fit: gather the stacked rows, form Z Z^T, lstsq (minimum norm)."""
    T, N = x.shape
    n = T - lags
    Zv = np.vstack([np.ones((1, n))] + [x.T[:, lags - k:T - k] for k in range(1, lags + 1)])
    Yt = x[lags:]
    if rows is not None:
        Zv, Yt = Zv.T[rows].T, Yt[rows]
    if rowok is not None:
        keep = rowok if rows is None else rowok[rows]
        Zv, Yt = Zv[:, keep], Yt[keep]
    Zc = Zv[:c, :]
    return np.linalg.lstsq(Zc.dot(Zc.T), Zc.dot(Yt), rcond=None)[0].T


def _qrbs_min_norm(x, lags, rows, alpha):
    Z, xt = _lag_stack(x, lags)
    X, y = Z[rows, 1:], (xt - x[lags - 1:-1])[rows]
    Xc, yc = X - X.mean(axis=0), y - y.mean(axis=0)
    G = Xc.T.dot(Xc) + alpha * np.eye(X.shape[1])
    return np.linalg.lstsq(G, Xc.T.dot(yc), rcond=None)[0].T


def _host_fits(x, plan, alpha, rowok):
    """coef [P, S, N, dout], status and pivot_ratio [P, S] by the pivot rule (SINGULAR fits are left zero)."""
    P, S, N, lags = plan.P, plan.S, plan.N, plan.lags
    coef = np.zeros((P, S, N, plan.dout))
    status = np.zeros((P, S), dtype=np.int32)
    ratio = np.zeros((P, S))
    for b in range(P):
        Z, xt = _lag_stack(x[b], lags)
        ok = None if rowok is None else rowok[b]
        if plan.mode == _QRBS:
            X, y = Z[:, 1:], xt - x[b][lags - 1:-1]
        for s in range(S):
            w = _weights(plan, b, s, ok)
            if plan.mode == _SLARAC:
                c = int(plan.ncols[b, s])
                Zc = Z[:, :c]
                wZ = w[:, None] * Zc
                B, ratio[b, s], status[b, s] = _solve_spd(Zc.T.dot(wZ), wZ.T.dot(xt))
                if B is not None:
                    coef[b, s, :, :c] = B.T
            else:
                k = w.sum()
                Xc, yc = X - w.dot(X) / k, y - w.dot(y) / k
                wX = w[:, None] * Xc
                B, ratio[b, s], status[b, s] = _solve_spd(Xc.T.dot(wX) + alpha * np.eye(X.shape[1]), wX.T.dot(yc))
                if B is not None:
                    coef[b, s] = B.T
    return coef, status, ratio


# ----------------------------------------------------------------------------------------
# device route
# ----------------------------------------------------------------------------------------
def device_supported(T, N, lags):
    """True when the library's kernels cover this shape (redcliff_tidybench_supported)."""
    from . import _native
    return bool(_native.lib().redcliff_tidybench_supported(int(T), int(N), int(lags)))


def _fit_groups(L, plan, budget):
    """[(s0, s1, max_count)]: consecutive fits whose workspace fits the budget (at least one fit per group)."""
    eff = plan.eff_count().max(axis=0)
    groups, s0 = [], 0
    while s0 < plan.S:
        s1, mc = s0 + 1, int(eff[s0])
        while s1 < plan.S:
            m2 = max(mc, int(eff[s1]))
            if int(L.redcliff_tidybench_ws_bytes(plan.P, s1 + 1 - s0, plan.N, plan.lags, m2)) > budget:
                break
            s1, mc = s1 + 1, m2
        groups.append((s0, s1, mc))
        s0 = s1
    return groups


def _device_fits(x, dev_data, plan, alpha, device, times):
    import ctypes

    import torch

    from . import _native as nat
    L = nat.lib()
    dev = torch.device(device if device is not None else (dev_data.device if dev_data is not None else "cuda"))
    P, S, N, lags = plan.P, plan.S, plan.N, plan.lags
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        data = dev_data.to(dev) if dev_data is not None else torch.from_numpy(x).to(dev)
        idx = torch.from_numpy(plan.idx).to(dev)
        count = torch.from_numpy(plan.count).to(dev)
        ncols = torch.from_numpy(plan.ncols).to(dev)
        torch.cuda.synchronize()
        times["upload"] += time.perf_counter() - t0
        coef = torch.empty((P, S, N, plan.dout), dtype=torch.float64, device=dev)
        status = torch.empty((P, S), dtype=torch.int32, device=dev)
        ratio = torch.empty((P, S), dtype=torch.float64, device=dev)
        groups = _fit_groups(L, plan, int(WORKSPACE_BUDGET_BYTES))
        nbytes = max(int(L.redcliff_tidybench_ws_bytes(P, s1 - s0, N, lags, mc)) for s0, s1, mc in groups)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        keep = []
        e0.record()
        for s0, s1, mc in groups:
            one = len(groups) == 1
            g_count = count if one else count[:, s0:s1].contiguous()
            g_ncols = ncols if one else ncols[:, s0:s1].contiguous()
            g_coef = coef if one else torch.empty((P, s1 - s0, N, plan.dout), dtype=torch.float64, device=dev)
            g_status = status if one else torch.empty((P, s1 - s0), dtype=torch.int32, device=dev)
            g_ratio = ratio if one else torch.empty((P, s1 - s0), dtype=torch.float64, device=dev)
            a = nat.TidybenchArgs()
            a.mode, a.P, a.S, a.T, a.N, a.lags, a.max_count = plan.mode, P, s1 - s0, plan.T, N, lags, mc
            a.alpha = float(alpha)
            a.data = data.data_ptr()
            a.idx = idx.data_ptr() + 4 * s0 * idx.stride(1)
            a.idx_pstride, a.idx_fstride = idx.stride(0), idx.stride(1)
            a.count, a.ncols = g_count.data_ptr(), g_ncols.data_ptr()
            a.coef, a.status, a.pivot_ratio = g_coef.data_ptr(), g_status.data_ptr(), g_ratio.data_ptr()
            a.ws, a.ws_bytes = ws.data_ptr(), nbytes
            nat.check(L.redcliff_tidybench_run(ctypes.byref(a), ctypes.c_void_p(stream)), "tidybench_run")
            if not one:
                coef[:, s0:s1].copy_(g_coef)
                status[:, s0:s1].copy_(g_status)
                ratio[:, s0:s1].copy_(g_ratio)
            keep.append((g_count, g_ncols, g_coef, g_status, g_ratio))
        e1.record()
        e1.synchronize()
        times["kernels"] += e0.elapsed_time(e1) * 1e-3
        out = coef.cpu().numpy(), status.cpu().numpy(), ratio.cpu().numpy()
    return out + (len(groups),)


# ----------------------------------------------------------------------------------------
# the two algorithms
# ----------------------------------------------------------------------------------------
def _route(T, N, lags, missing_values):
    forced = os.environ.get("REDCLIFF_TIDYBENCH_PATH", "") or "auto"
    if forced not in ("auto", "host", "fused"):
        raise ValueError("REDCLIFF_TIDYBENCH_PATH must be fused, host or auto")
    if forced == "host":
        return "host"
    fused = missing_values is None
    if fused:
        import torch
        try:
            fused = torch.cuda.is_available() and device_supported(T, N, lags)
        except ImportError:
            if forced == "fused":
                raise
            fused = False
    if forced == "fused" and not fused:
        raise RuntimeError("REDCLIFF_TIDYBENCH_PATH=fused: no GPU, missing_values given, or shape outside "
                           "redcliff_tidybench_supported (T=%d N=%d lags=%d)" % (T, N, lags))
    return "fused" if fused else "host"


def _run(mode, datas, lags, plan_fn, alpha, missing_values, proc, device, aggregate):
    times = dict.fromkeys(("draws", "upload", "kernels", "fallback", "aggregate"), 0.0)
    t_all = time.perf_counter()
    x, dev_data = _host_series(datas, proc, missing_values)
    P, T, N = x.shape
    lags = int(lags)
    if lags < 1 or T <= lags:
        raise ValueError("need 1 <= lags < T (lags=%d, T=%d)" % (lags, T))
    route = _route(T, N, lags, missing_values)
    t0 = time.perf_counter()
    plan = plan_fn(P, T, N)
    times["draws"] = time.perf_counter() - t0
    groups = 1
    if route == "fused":
        coef, status, ratio, groups = _device_fits(x, dev_data, plan, alpha, device, times)
        if (status == NONFINITE).any():
            raise RuntimeError("tidybench: %d fit(s) ended NONFINITE on the device" % int((status == NONFINITE).sum()))
    else:
        rowok = None
        if missing_values is not None:   # a sampled row is dropped when its targets or regressors hold the marker
            miss = (x == missing_values).any(axis=2)
            rowok = np.stack([~np.any([miss[b, lags - k:T - k] for k in range(lags + 1)], axis=0) for b in range(P)])
        coef, status, ratio = _host_fits(x, plan, alpha, rowok)
    t0 = time.perf_counter()
    for b, s in np.argwhere(status == SINGULAR):
        rows = plan.rows(b, s)
        ok = None if route == "fused" or missing_values is None else rowok[b]
        if mode == _SLARAC:
            c = int(plan.ncols[b, s])
            coef[b, s] = 0.0
            coef[b, s, :, :c] = _slarac_min_norm(x[b], lags, rows, c, ok)
        else:
            coef[b, s] = _qrbs_min_norm(x[b], lags, rows, alpha)
    times["fallback"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    scores = np.stack([_post(aggregate(coef[b], N), proc) for b in range(P)])
    times["aggregate"] = time.perf_counter() - t0
    times["total"] = time.perf_counter() - t_all
    info = {"route": route, "status": status, "pivot_ratio": ratio, "n_host_solved": int((status == SINGULAR).sum()),
            "time": times, "coef": coef, "groups": groups, "ncols": plan.ncols.copy(), "count": plan.count.copy()}
    return scores, info


def slarac_many(datas, maxlags=1, n_subsamples=200, subsample_sizes=DEFAULT_SUBSAMPLE_SIZES, missing_values=None,
                aggregate_lags=_max_over_lags, device=None, return_info=False, **kwargs):
    """SLARAC scores [P, N, N] of P same-shape series [P, T, N] in one native call.  The draws are made problem by
    problem, so under one seed the result equals a loop of ``slarac`` calls."""
    proc = _pop_processing(kwargs)
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))

    def aggregate(coef, N):
        scores = np.abs(coef[0])
        for s in range(1, coef.shape[0]):
            scores += np.abs(coef[s])
        scores = scores[:, 1:] / (n_subsamples + 1)
        return aggregate_lags(scores.reshape(N, -1, N))

    out = _run(_SLARAC, datas, maxlags, lambda P, T, N: _slarac_plan(P, T, N, int(maxlags), int(n_subsamples), subsample_sizes),
               0.0, missing_values, proc, device, aggregate)
    return out if return_info else out[0]


def qrbs_many(datas, lags=1, alpha=.005, q=.75, n_resamples=600, device=None, return_info=False, **kwargs):
    """QRBS scores [P, N, N] of P same-shape series [P, T, N] in one native call; equal to a loop of ``qrbs``."""
    proc = _pop_processing(kwargs)
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
    if not alpha > 0:
        raise ValueError("alpha must be positive")

    def aggregate(coef, N):
        results = np.abs(coef.reshape(coef.shape[0], N, int(lags), -1)).sum(axis=2)
        return np.quantile(results, q, axis=0).T

    out = _run(_QRBS, datas, lags, lambda P, T, N: _qrbs_plan(P, T, N, int(lags), int(n_resamples)), float(alpha), None, proc,
               device, aggregate)
    return out if return_info else out[0]


def _single(fn, data, kwargs):
    if len(getattr(data, "shape", ())) != 2:
        data = np.asarray(data)
    if len(data.shape) != 2:
        raise ValueError("data must be [T, N]")
    info = kwargs.get("return_info", False)
    out = fn(data[None], **kwargs)
    if not info:
        return out[0]
    d = dict(out[1])
    for k in ("status", "pivot_ratio", "coef", "ncols", "count"):
        d[k] = d[k][0]
    return out[0][0], d


def slarac(data, maxlags=1, n_subsamples=200, subsample_sizes=DEFAULT_SUBSAMPLE_SIZES, missing_values=None,
           aggregate_lags=_max_over_lags, **kwargs):
    """SLARAC (Subsampled Linear Auto-Regression Absolute Coefficients): data [T, N] -> scores [N, N], entry (i, j)
    for the link X_i -> X_j.  The reference's signature; ``pre_normalise``, ``post_standardise``,
    ``post_zeroonescaling`` and ``post_edgeprior`` as in its common pre- and post-processing.  The input is never
    modified.  ``return_info=True`` adds a dict: route, per-fit status and pivot_ratio, n_host_solved, time."""
    return _single(slarac_many, data, dict(kwargs, maxlags=maxlags, n_subsamples=n_subsamples, subsample_sizes=subsample_sizes,
                                           missing_values=missing_values, aggregate_lags=aggregate_lags))


def qrbs(data, lags=1, alpha=.005, q=.75, n_resamples=600, **kwargs):
    """QRBS (Quantiles of Ridge regressed Bootstrap Samples): data [T, N] -> scores [N, N], entry (i, j) for the
    link X_i -> X_j.  The reference's signature and processing keywords; see ``slarac``."""
    return _single(qrbs_many, data, dict(kwargs, lags=lags, alpha=alpha, q=q, n_resamples=n_resamples))


# ----------------------------------------------------------------------------------------
# the evaluation scripts' driver
# ----------------------------------------------------------------------------------------
def prepare_data_for_modeling(samples):
    """samples: [(window [Tw, N], one-hot regime label [R] or [R, 1])] -> (data [T, N], labels [T, R],
    {regime: 0/1 mask [T, N]}, Tw, T, N, R): the windows end to end, each row labelled and masked by its window's
    dominant regime."""
    xs = [np.asarray(s[0]) for s in samples]
    ys = [np.asarray(s[1]).reshape(1, -1) for s in samples]
    Tw, N = xs[0].shape
    R = ys[0].shape[1]
    for x, y in zip(xs, ys):
        assert x.shape == (Tw, N) and y.shape == (1, R)
    data = np.concatenate(xs, axis=0)
    labels = np.concatenate([np.repeat(y, Tw, axis=0) for y in ys], axis=0)
    dominant = np.repeat([int(np.argmax(y)) for y in ys], Tw)
    masks = {r: np.zeros(data.shape) for r in range(R)}
    for r in range(R):
        masks[r][dominant == r, :] = 1.0
    T = Tw * len(samples)
    assert data.shape == (T, N) and labels.shape == (T, R)
    return data, labels, masks, Tw, T, N, R


def get_standardized_off_diagonal_relation_predictions(A, transpose=False):
    """|A| with a zero diagonal (transposed on request)."""
    A = np.asarray(A)
    assert A.ndim == 2 and A.shape[0] == A.shape[1]
    out = np.abs(A)
    if transpose:
        out = out.T
    return out * (np.ones(out.shape) - np.eye(out.shape[0]))


def run_tidybench_experiment(samples, alg_name):
    """Regime-aware SLARAC / QRBS as the evaluation scripts run them: one score matrix per regime from the series
    masked to that regime's rows, ``post_standardise=True``, |.| with a zero diagonal.  The R masked series go
    through one ``*_many`` call."""
    if alg_name == "lasar":
        raise NotImplementedError("lasar has its own driver, run_lasar_experiment(samples): the cross-validated LARS "
                                  "paths (LassoLarsCV) run through lasar_many, not through this function (DESIGN section 24)")
    if alg_name not in ("slarac", "qrbs"):
        raise ValueError("unknown tidybench algorithm %r" % (alg_name,))
    data, _, masks, _, _, _, R = prepare_data_for_modeling(samples)
    series = np.stack([data * masks[r] for r in range(R)])
    fn = slarac_many if alg_name == "slarac" else qrbs_many
    scores = fn(series, post_standardise=True)
    return [get_standardized_off_diagonal_relation_predictions(scores[r], transpose=False) for r in range(R)]


# ========================================================================================
# LASAR (tidybench/lasar.py): LassoLarsCV variable selection per target, then a least-squares refit
# ========================================================================================
DEGENERATE = 3            # LS_DEGENERATE of csrc/rc_lasar.h: the (series, fit, target) is recomputed on the host
LARS_MAX_ITER = 500       # LassoLarsCV's max_iter
LARS_MAX_N_ALPHAS = 1000  # LassoLarsCV's max_n_alphas
_EPS = float(np.finfo(np.float64).eps)
_TINY32 = float(np.finfo(np.float32).tiny)
_EQ_TOL = float(np.finfo(np.float32).eps)
_DBL_MAX = float(np.finfo(np.float64).max)
# what a path did that the device kernels do not: any of these makes the triple DEGENERATE
F_DROP_FOR_GOOD, F_ALPHA_UP, F_AA, F_MULTI_DROP, F_KNOTS, F_XROUTE, F_ORDER = 1, 2, 4, 8, 16, 32, 64


def lasar_knot_capacity(N):
    """Knots of one path the device stores (LS_KCAP of csrc/rc_lasar.h): N additions, a few drop / re-add pairs."""
    return 2 * int(N) + 4


def _min_pos(v):
    v = v[v > 0]
    return float(v.min()) if v.size else _DBL_MAX


def _rotg(a, b):
    """BLAS rotg: (r, c, s) with [c s; -s c] [a; b] = [r; 0]."""
    roe = a if abs(a) > abs(b) else b
    scale = abs(a) + abs(b)
    if scale == 0.0:
        return 0.0, 1.0, 0.0
    r = scale * np.sqrt((a / scale) ** 2 + (b / scale) ** 2)
    if roe < 0.0:
        r = -r
    return r, a / r, b / r


def _cholesky_delete(L, n, go_out):
    """sklearn.utils.arrayfuncs.cholesky_delete on the leading n x n lower factor: remove row / column go_out."""
    for i in range(go_out, n - 1):
        L[i, :i + 2] = L[i + 1, :i + 2]
    for i in range(go_out, n - 1):
        r, c, s = _rotg(L[i, i], L[i, i + 1])
        if r < 0.0:
            r, c, s = -r, -c, -s
        L[i, i], L[i, i + 1] = r, 0.0
        for k in range(i + 1, n - 1):
            xk, yk = L[k, i], L[k, i + 1]
            L[k, i], L[k, i + 1] = c * xk + s * yk, c * yk - s * xk


def _chol_solve(L, n, b):
    """x with L L^T x = b (lower factor, leading n x n)."""
    w = np.empty(n)
    for i in range(n):
        w[i] = (b[i] - np.dot(L[i, :i], w[:i])) / L[i, i]
    for i in range(n - 1, -1, -1):
        w[i] = (w[i] - np.dot(L[i + 1:n, i], w[i + 1:n])) / L[i, i]
    return w


def _lars_path(X, y, use_gram, alpha_min=0.0):
    """sklearn's ``_lars_path_solver(method="lasso", return_path=True, eps=finfo(float).eps, max_iter=500)`` on
    centred X [n, p], y [n], restated branch by branch.  Returns the knots' alphas [K], their coefficients [K, p]
    and the F_* flags of what the path went through."""
    n_samples, p = y.size, X.shape[1]
    Cov = np.dot(X.T, y)
    if use_gram:
        Gram = np.dot(X.T, X)
        Gram_copy, Cov_copy = Gram.copy(), Cov.copy()
    else:
        Gram = None
        X = X.copy("F")
    max_features = min(LARS_MAX_ITER, p)
    alphas, coefs = [0.0], [np.zeros(p)]
    n_iter = n_active = 0
    active, indices = [], np.arange(p)
    sign_active = np.zeros(max_features)
    L = np.zeros((max_features, max_features))
    drop = False
    flags = 0 if use_gram else F_XROUTE
    while True:
        if Cov.size:
            C_idx = int(np.argmax(np.abs(Cov)))
            C_ = Cov[C_idx]
            C = np.fabs(C_)
        else:
            C = 0.0
        coef = coefs[n_iter]
        prev_alpha = alphas[n_iter - 1]
        prev_coef = coefs[n_iter - 1]
        alpha = C / n_samples
        alphas[n_iter] = alpha
        if alpha <= alpha_min + _EQ_TOL:   # early stopping
            if abs(alpha - alpha_min) > _EQ_TOL:
                if n_iter > 0:
                    ss = (prev_alpha - alpha_min) / (prev_alpha - alpha)
                    coef[:] = prev_coef + ss * (coef - prev_coef)
                alphas[n_iter] = alpha_min
            break
        if n_iter >= LARS_MAX_ITER or n_active >= p:
            break
        if not drop:
            sign_active[n_active] = np.sign(C_)
            m, n = n_active, C_idx + n_active
            Cov[C_idx], Cov[0] = Cov[0], Cov[C_idx]
            indices[n], indices[m] = indices[m], indices[n]
            Cov_not_shortened = Cov
            Cov = Cov[1:]
            if Gram is None:
                tmp = X[:, n].copy()
                X[:, n] = X[:, m]
                X[:, m] = tmp
                c = np.sqrt(np.dot(X[:, n_active], X[:, n_active])) ** 2
                L[n_active, :n_active] = np.dot(X.T[n_active], X.T[:n_active].T)
            else:
                Gram[[m, n]] = Gram[[n, m]]
                Gram[:, [m, n]] = Gram[:, [n, m]]
                c = Gram[n_active, n_active]
                L[n_active, :n_active] = Gram[n_active, :n_active]
            for i in range(n_active):   # L[:n_active, :n_active] w = L[n_active, :n_active]
                L[n_active, i] = (L[n_active, i] - np.dot(L[i, :i], L[n_active, :i])) / L[i, i]
            v = np.dot(L[n_active, :n_active], L[n_active, :n_active])
            diag = max(np.sqrt(np.abs(c - v)), _EPS)
            L[n_active, n_active] = diag
            if diag < 1e-7:   # degenerate regressor: drop it for good
                flags |= F_DROP_FOR_GOOD
                Cov = Cov_not_shortened
                Cov[0] = 0
                Cov[C_idx], Cov[0] = Cov[0], Cov[C_idx]
                continue
            active.append(int(indices[n_active]))
            n_active += 1
        if n_iter > 0 and prev_alpha < alpha:   # alpha is increasing: bail out
            flags |= F_ALPHA_UP
            break
        sa = sign_active[:n_active]
        least_squares = _chol_solve(L, n_active, sa)
        if least_squares.size == 1 and least_squares[0] == 0:
            least_squares[...] = 1
            AA = 1.0
        else:
            with np.errstate(all="ignore"):
                AA = 1.0 / np.sqrt(np.sum(least_squares * sa))
            if not np.isfinite(AA):   # L is too ill-conditioned
                flags |= F_AA
                i = 0
                L_ = L[:n_active, :n_active].copy()
                while not np.isfinite(AA):
                    L_.flat[::n_active + 1] += (2 ** i) * _EPS
                    least_squares = _chol_solve(L_, n_active, sa)
                    AA = 1.0 / np.sqrt(max(np.sum(least_squares * sa), _EPS))
                    i += 1
            least_squares *= AA
        if Gram is None:
            eq_dir = np.dot(X.T[:n_active].T, least_squares)
            corr_eq_dir = np.dot(X.T[n_active:], eq_dir)
        else:
            corr_eq_dir = np.dot(Gram[:n_active, n_active:].T, least_squares)
        np.around(corr_eq_dir, decimals=15, out=corr_eq_dir)
        g1 = _min_pos((C - Cov) / (AA - corr_eq_dir + _TINY32))
        g2 = _min_pos((C + Cov) / (AA + corr_eq_dir + _TINY32))
        gamma_ = min(g1, g2, C / AA)
        drop = False
        z = -coef[active] / (least_squares + _TINY32)
        z_pos = _min_pos(z)
        if z_pos < gamma_:   # some coefficients have changed sign
            idx = np.where(z == z_pos)[0][::-1]
            if idx.size > 1:
                flags |= F_MULTI_DROP
            sign_active[idx] = -sign_active[idx]
            gamma_ = z_pos
            drop = True
        n_iter += 1
        alphas.append(0.0)
        coefs.append(np.zeros(p))
        coef, prev_coef = coefs[n_iter], coefs[n_iter - 1]
        coef[active] = prev_coef[active] + gamma_ * least_squares
        Cov -= gamma_ * corr_eq_dir
        if drop:
            for ii in idx:
                _cholesky_delete(L, n_active, int(ii))
            n_active -= 1
            drop_idx = [active.pop(int(ii)) for ii in idx]
            if Gram is None:
                for ii in idx:
                    for i in range(int(ii), n_active):
                        tmp = X[:, i].copy()
                        X[:, i] = X[:, i + 1]
                        X[:, i + 1] = tmp
                        indices[i], indices[i + 1] = indices[i + 1], indices[i]
                residual = y - np.dot(X[:, :n_active], coef[active])
                temp = np.atleast_1d(np.dot(X.T[n_active], residual))
            else:
                for ii in idx:
                    for i in range(int(ii), n_active):
                        indices[i], indices[i + 1] = indices[i + 1], indices[i]
                        Gram[[i, i + 1]] = Gram[[i + 1, i]]
                        Gram[:, [i, i + 1]] = Gram[:, [i + 1, i]]
                temp = Cov_copy[drop_idx] - np.dot(Gram_copy[drop_idx], coef)
            Cov = np.r_[temp, Cov]
            sign_active = np.append(np.delete(sign_active, idx), [0.0] * idx.size)
    if len(alphas) > lasar_knot_capacity(p):
        flags |= F_KNOTS
    if not flags and np.any(np.diff(alphas) > 0):   # the last knot's alpha above its predecessor's, without a bail-out
        flags |= F_ORDER
    return np.array(alphas), np.array(coefs), flags


def _interp_rows(x, y, x_new):
    """scipy's ``interp1d(x, y, axis=0)(x_new)`` (linear, x sorted first), operation by operation."""
    ind = np.argsort(x, kind="mergesort")
    x, y = x[ind], y[ind]
    hi = np.searchsorted(x, x_new).clip(1, len(x) - 1).astype(int)
    lo = hi - 1
    with np.errstate(all="ignore"):
        slope = (y[hi] - y[lo]) / (x[hi] - x[lo])[:, None]
        return slope * (x_new - x[lo])[:, None] + y[lo]


def _fold_bounds(count, cv):
    """KFold(cv) without shuffling: contiguous runs, the first count % cv one row longer."""
    sizes = np.full(cv, count // cv, dtype=np.int64)
    sizes[:count % cv] += 1
    ends = np.cumsum(sizes)
    return ends - sizes, ends


def _lasso_lars_cv(X, y, cv):
    """``LassoLarsCV(cv=cv).fit(X, y)``: (coef_, intercept_, best_alpha, its index in cv_alphas_, flags)."""
    n, p = X.shape
    X = X.copy("F" if X.flags["F_CONTIGUOUS"] else "C")
    y = y.copy()
    starts, ends = _fold_bounds(n, cv)
    paths, flags = [], 0
    for f in range(cv):
        test = np.arange(starts[f], ends[f])
        train = np.concatenate([np.arange(0, starts[f]), np.arange(ends[f], n)])
        Xtr, ytr, Xte, yte = X[train], y[train], X[test], y[test]
        X_mean = Xtr.mean(axis=0)
        Xtr -= X_mean
        Xte -= X_mean
        y_mean = ytr.mean(axis=0)
        ytr -= y_mean
        yte -= y_mean
        alphas, coefs, fl = _lars_path(Xtr, ytr, Xtr.shape[0] > p)
        flags |= fl
        paths.append((alphas, (np.dot(Xte, coefs.T) - yte[:, np.newaxis]).T))
    all_alphas = np.unique(np.concatenate([a for a, _ in paths]))
    stride = int(max(1, int(len(all_alphas) / float(LARS_MAX_N_ALPHAS))))
    all_alphas = all_alphas[::stride]
    mse_path = np.empty((len(all_alphas), cv))
    for index, (alphas, residues) in enumerate(paths):
        alphas, residues = alphas[::-1], residues[::-1]
        if alphas[0] != 0:
            alphas = np.r_[0, alphas]
            residues = np.r_[residues[0, np.newaxis], residues]
        if alphas[-1] != all_alphas[-1]:
            alphas = np.r_[alphas, all_alphas[-1]]
            residues = np.r_[residues, residues[-1, np.newaxis]]
        this_residues = _interp_rows(alphas, residues, all_alphas)
        this_residues **= 2
        mse_path[:, index] = np.mean(this_residues, axis=-1)
    mask = np.all(np.isfinite(mse_path), axis=-1)
    all_alphas, mse_path = all_alphas[mask], mse_path[mask]
    i_best = int(np.argmin(mse_path.mean(axis=-1)))
    best_alpha = float(all_alphas[i_best])
    X_offset, y_offset = X.mean(axis=0), y.mean(axis=0)
    Xc, yc = X - X_offset, y - y_offset
    alphas, coefs, fl = _lars_path(Xc, yc, n > p, best_alpha)
    coef = coefs[-1]
    return coef, y_offset - np.dot(X_offset, coef), best_alpha, i_best, flags | fl


def _lasar_stack(x, lags):
    """Y [n, N] and Z [n, lags N] built with lassovar's own operations (so the memory layouts are its too)."""
    Y = x.T[:, lags:]
    Z = np.vstack([x.T[:, lags - k:-k] for k in range(1, lags + 1)])
    return Y.T, Z.T


def _lasar_host_triple(Y, Z, j, lags, cv):
    """One target of ``lassovar``: (row of scores [lags N], selected [lags N], best_alpha [lags], best index [lags],
    status, pivot ratio, flags)."""
    d = Y.shape[1]
    target = np.copy(Y[:, j])
    selected = np.full(d * lags, False)
    best_alpha, best_idx, flags = np.zeros(lags), np.zeros(lags, dtype=np.int32), 0
    for lag in range(lags):
        blk = Z[:, d * lag:d * (lag + 1)]
        coef, intercept, best_alpha[lag], best_idx[lag], fl = _lasso_lars_cv(blk, target, cv)
        flags |= fl
        selected[d * lag:d * (lag + 1)] = coef > 0
        target -= np.dot(blk, coef) + intercept
    row = np.zeros(d * lags)
    status, ratio = OK, np.inf
    if selected.any():
        ZZ = Z[:, selected]
        G, r = ZZ.T.dot(ZZ), ZZ.T.dot(Y[:, j])
        B, ratio, status = _solve_spd(G, r)
        if status == NONFINITE:
            raise RuntimeError("lasar: non-finite Gram matrix in a refit")
        if status == SINGULAR:
            B = np.linalg.lstsq(G, r, rcond=None)[0]
        row[selected] = B
    if flags:
        status = DEGENERATE
    return row, selected, best_alpha, best_idx, status, ratio, flags


def _lasar_plan(P, T, N, maxlags, n_subsamples, subsample_sizes, cv):
    n = T - maxlags
    sizes = list(subsample_sizes)
    ks = [int(np.round(s * T)) for s in sizes] if n_subsamples else []
    if min([n] + ks) < cv:   # sklearn: "Cannot have number of splits n_splits greater than the number of samples"
        raise ValueError("Cannot have number of splits n_splits=%d greater than the number of samples: n_samples=%d."
                         % (cv, min([n] + ks)))
    plan = _Plan(_SLARAC, P, 1 + n_subsamples, T, N, maxlags, max([n] + ks))
    for b in range(P):
        plan.count[b, 0] = -1
        for s, size in enumerate(np.random.choice(sizes, n_subsamples)):
            k = int(np.round(size * T))
            plan.idx[b, s + 1, :k] = np.random.randint(0, n, size=(k,))
            plan.count[b, s + 1] = k
    return plan


def lasar_device_supported(T, N, lags):
    """True when the library's LASAR kernels cover this shape (redcliff_lasar_supported)."""
    from . import _native
    return bool(_native.lib().redcliff_lasar_supported(int(T), int(N), int(lags)))


def _lasar_route(T, N, lags):
    forced = os.environ.get("REDCLIFF_TIDYBENCH_PATH", "") or "auto"
    if forced not in ("auto", "host", "fused"):
        raise ValueError("REDCLIFF_TIDYBENCH_PATH must be fused, host or auto")
    if forced == "host":
        return "host"
    import torch
    try:
        fused = torch.cuda.is_available() and lasar_device_supported(T, N, lags)
    except ImportError:
        if forced == "fused":
            raise
        fused = False
    if forced == "fused" and not fused:
        raise RuntimeError("REDCLIFF_TIDYBENCH_PATH=fused: no GPU, or shape outside redcliff_lasar_supported "
                           "(T=%d N=%d lags=%d)" % (T, N, lags))
    return "fused" if fused else "host"


def _lasar_groups(L, plan, cv, budget):
    """[(s0, s1, max_count)]: consecutive fits whose workspace fits the budget (at least one fit per group)."""
    eff = plan.eff_count().max(axis=0)
    groups, s0 = [], 0
    while s0 < plan.S:
        s1, mc = s0 + 1, int(eff[s0])
        while s1 < plan.S:
            m2 = max(mc, int(eff[s1]))
            if int(L.redcliff_lasar_ws_bytes(plan.P, s1 + 1 - s0, plan.N, plan.lags, cv, m2)) > budget:
                break
            s1, mc = s1 + 1, m2
        groups.append((s0, s1, mc))
        s0 = s1
    return groups


def _lasar_device(x, dev_data, plan, cv, device, times):
    import ctypes

    import torch

    from . import _native as nat
    L = nat.lib()
    dev = torch.device(device if device is not None else (dev_data.device if dev_data is not None else "cuda"))
    P, S, N, lags = plan.P, plan.S, plan.N, plan.lags
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        data = dev_data.to(dev) if dev_data is not None else torch.from_numpy(x).to(dev)
        idx = torch.from_numpy(plan.idx).to(dev)
        count = torch.from_numpy(plan.count).to(dev)
        torch.cuda.synchronize()
        times["upload"] += time.perf_counter() - t0
        shapes = (("coef", (P, S, N, N), torch.float64), ("best_alpha", (P, S, N), torch.float64),
                  ("best_index", (P, S, N), torch.int32), ("selected", (P, S, N), torch.int32),
                  ("status", (P, S, N), torch.int32), ("pivot_ratio", (P, S, N), torch.float64))
        out = {k: torch.empty(shp, dtype=dt, device=dev) for k, shp, dt in shapes}
        groups = _lasar_groups(L, plan, cv, int(WORKSPACE_BUDGET_BYTES))
        nbytes = max(int(L.redcliff_lasar_ws_bytes(P, s1 - s0, N, lags, cv, mc)) for s0, s1, mc in groups)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        keep = []
        e0.record()
        for s0, s1, mc in groups:
            one = len(groups) == 1
            g_count = count if one else count[:, s0:s1].contiguous()
            g = out if one else {k: torch.empty((P, s1 - s0) + shp[2:], dtype=dt, device=dev) for k, shp, dt in shapes}
            a = nat.LasarArgs()
            a.P, a.S, a.T, a.N, a.lags, a.cv, a.max_count = P, s1 - s0, plan.T, N, lags, cv, mc
            a.data = data.data_ptr()
            a.idx = idx.data_ptr() + 4 * s0 * idx.stride(1)
            a.idx_pstride, a.idx_fstride = idx.stride(0), idx.stride(1)
            a.count = g_count.data_ptr()
            a.coef, a.best_alpha, a.best_index = g["coef"].data_ptr(), g["best_alpha"].data_ptr(), g["best_index"].data_ptr()
            a.selected, a.status, a.pivot_ratio = g["selected"].data_ptr(), g["status"].data_ptr(), g["pivot_ratio"].data_ptr()
            a.ws, a.ws_bytes = ws.data_ptr(), nbytes
            nat.check(L.redcliff_lasar_run(ctypes.byref(a), ctypes.c_void_p(stream)), "lasar_run")
            if not one:
                for k in out:
                    out[k][:, s0:s1].copy_(g[k])
            keep.append((g_count, g))
        e1.record()
        e1.synchronize()
        times["kernels"] += e0.elapsed_time(e1) * 1e-3
        res = {k: v.cpu().numpy() for k, v in out.items()}
    res["groups"] = len(groups)
    return res


def lasar_many(datas, maxlags=1, n_subsamples=100, subsample_sizes=DEFAULT_SUBSAMPLE_SIZES, cv=5,
               aggregate_lags=_max_over_lags, device=None, return_info=False, **kwargs):
    """LASAR scores [P, N, N] of P same-shape series [P, T, N] in one native call.  The draws are made problem by
    problem, so under one seed the result equals a loop of ``lasar`` calls."""
    proc = _pop_processing(kwargs)
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
    times = dict.fromkeys(("draws", "upload", "kernels", "fallback", "aggregate"), 0.0)
    t_all = time.perf_counter()
    x, dev_data = _host_series(datas, proc, None)
    P, T, N = x.shape
    lags, cv, S = int(maxlags), int(cv), 1 + int(n_subsamples)
    if lags < 1 or T <= lags:
        raise ValueError("need 1 <= maxlags < T (maxlags=%d, T=%d)" % (lags, T))
    if cv < 2:
        raise ValueError("cv must be at least 2")
    route = _lasar_route(T, N, lags)
    t0 = time.perf_counter()
    plan = _lasar_plan(P, T, N, lags, int(n_subsamples), subsample_sizes, cv)
    times["draws"] = time.perf_counter() - t0
    D = lags * N
    coef = np.zeros((P, S, N, D))
    selected = np.zeros((P, S, N, D), dtype=bool)
    best_alpha = np.zeros((P, S, N, lags))
    best_index = np.zeros((P, S, N, lags), dtype=np.int32)
    status = np.zeros((P, S, N), dtype=np.int32)
    ratio = np.full((P, S, N), np.inf)
    flags = np.zeros((P, S, N), dtype=np.int32)
    groups = 1
    if route == "fused":
        res = _lasar_device(x, dev_data, plan, cv, device, times)
        groups = res["groups"]
        if (res["status"] == NONFINITE).any():
            raise RuntimeError("lasar: %d target(s) ended NONFINITE on the device" % int((res["status"] == NONFINITE).sum()))
        coef[:], status[:], ratio[:] = res["coef"], res["status"], res["pivot_ratio"]
        best_alpha[..., 0], best_index[..., 0] = res["best_alpha"], res["best_index"]
        selected[:] = (res["selected"][..., None] >> np.arange(N)) & 1
        todo = np.argwhere((status == SINGULAR) | (status == DEGENERATE))
    else:
        todo = np.argwhere(np.ones((P, S), dtype=bool))
    t0 = time.perf_counter()
    stacks = {}
    for t in todo:
        b, s = int(t[0]), int(t[1])
        if (b, s) not in stacks:
            if route == "fused":
                stacks.clear()
            Y, Z = _lasar_stack(x[b], lags)
            rows = plan.rows(b, s)
            stacks[(b, s)] = (Y, Z) if rows is None else (Y[rows], Z[rows])
        Y, Z = stacks[(b, s)]
        for j in ([int(t[2])] if route == "fused" else range(N)):
            (coef[b, s, j], selected[b, s, j], best_alpha[b, s, j], best_index[b, s, j], st, ratio[b, s, j],
             flags[b, s, j]) = _lasar_host_triple(Y, Z, j, lags, cv)
            if route == "host":
                status[b, s, j] = st
        if route == "host":
            stacks.clear()
    times["fallback" if route == "fused" else "kernels"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    scores = []
    for b in range(P):
        tot = np.abs(coef[b, 0])
        for s in range(1, S):
            tot += np.abs(coef[b, s])
        tot /= S
        scores.append(_post(aggregate_lags(tot.reshape(N, -1, N)), proc))
    scores = np.stack(scores)
    times["aggregate"] = time.perf_counter() - t0
    times["total"] = time.perf_counter() - t_all
    info = {"route": route, "status": status, "pivot_ratio": ratio, "time": times, "coef": coef, "groups": groups,
            "n_host_solved": int(len(todo)) if route == "fused" else 0, "count": plan.count.copy(), "selected": selected,
            "best_alpha": best_alpha, "best_index": best_index, "flags": flags}
    return (scores, info) if return_info else scores


def lasar(data, maxlags=1, n_subsamples=100, subsample_sizes=DEFAULT_SUBSAMPLE_SIZES, cv=5, aggregate_lags=_max_over_lags,
          **kwargs):
    """LASAR (LASso Auto-Regression): data [T, N] -> scores [N, N], entry (i, j) for the link X_i -> X_j.  The
    reference's signature and processing keywords; see ``slarac``.  Per target a cross-validated lasso path
    (sklearn's ``LassoLarsCV``) selects the parents with a positive coefficient, a least-squares refit on them gives
    the scores, averaged in absolute value over the full series and ``n_subsamples`` bootstrap subsamples."""
    if len(getattr(data, "shape", ())) != 2:
        data = np.asarray(data)
    if len(data.shape) != 2:
        raise ValueError("data must be [T, N]")
    out = lasar_many(data[None], maxlags=maxlags, n_subsamples=n_subsamples, subsample_sizes=subsample_sizes, cv=cv,
                     aggregate_lags=aggregate_lags, **kwargs)
    if not kwargs.get("return_info", False):
        return out[0]
    d = dict(out[1])
    for k in ("status", "pivot_ratio", "coef", "count", "selected", "best_alpha", "best_index", "flags"):
        d[k] = d[k][0]
    return out[0][0], d


def run_lasar_experiment(samples):
    """Regime-aware LASAR as the evaluation scripts run it: one score matrix per regime from the series masked to
    that regime's rows, ``post_standardise=True``, |.| with a zero diagonal; the R masked series go through one
    ``lasar_many`` call."""
    data, _, masks, _, _, _, R = prepare_data_for_modeling(samples)
    scores = lasar_many(np.stack([data * masks[r] for r in range(R)]), post_standardise=True)
    return [get_standardized_off_diagonal_relation_predictions(scores[r], transpose=False) for r in range(R)]
