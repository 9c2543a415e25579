"""The regime-aware tidybench comparison baselines: SLARAC and QRBS.

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
        raise NotImplementedError("lasar is not ported: it runs sklearn's cross-validated LARS path (LassoLarsCV), a "
                                  "sequential active-set algorithm with no batched native form here (DESIGN section 10)")
    if alg_name not in ("slarac", "qrbs"):
        raise ValueError("unknown tidybench algorithm %r" % (alg_name,))
    data, _, masks, _, _, _, R = prepare_data_for_modeling(samples)
    series = np.stack([data * masks[r] for r in range(R)])
    fn = slarac_many if alg_name == "slarac" else qrbs_many
    scores = fn(series, post_standardise=True)
    return [get_standardized_off_diagonal_relation_predictions(scores[r], transpose=False) for r in range(R)]
