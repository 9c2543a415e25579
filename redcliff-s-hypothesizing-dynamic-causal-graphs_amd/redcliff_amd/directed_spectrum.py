"""Directed-spectrum features: the input of the dCSFA-NMF baseline.

Restates general_utils/directed_spectrum.py (get_directed_spectrum), general_utils/time_series.py
(make_high_level_signal_features) and general_utils/misc.py (flatten_directed_spectrum_features) of the
reference, and adds the batched entry ``directed_spectrum_features`` that the ``*_as_matrices`` loaders
(redcliff_amd/data.py) are built on.

Two routes compute the same contract:

* the host route (this file, numpy): Welch spectra in double, rounded once to the input's precision, then a
  Wilson spectral factorisation per window and channel pair whose arrays carry the dtypes the reference's
  carry (float32 input: complex64 CPSD, float32 A0 / Sigma, complex128 psi / H);
* the device route (csrc/rc_dirspec.hip through redcliff_dirspec_run): one wavefront per (window, pair).

Both decide per window and per pair: the singular branch (by rule when the window has fewer than two Welch
segments, else by the closed-form condition number of the Hermitian 2x2) and its regulariser never look at
another window, which is what the reference's data sets compute by calling the extraction one window at a time.
"""
import os
import warnings

import numpy as np

DEFAULT_CSD_PARAMS = {
    "detrend": "constant",
    "window": "hann",
    "nperseg": 512,
    "noverlap": 256,
    "nfft": None,
}
"""Default parameters sent to ``scipy.signal.csd``"""

CONVERGED, MAXITER, PIVOT = 0, 1, 2
EPS_MULTIPLIER = 100
DEVICE_MAX_NPERSEG = 256


# --------------------------------------------------------------------------- spectra
def _params(csd_params):
    return {**DEFAULT_CSD_PARAMS, **(csd_params or {})}


def _standard(par, T):
    """True when the Welch parameters are the ones this project computes itself (and the device supports)."""
    nper, nov = par["nperseg"], par["noverlap"]
    return (par["detrend"] == "constant" and par["window"] == "hann" and par["nfft"] in (None, nper)
            and isinstance(nper, (int, np.integer)) and isinstance(nov, (int, np.integer))
            and 2 <= nper <= T and 0 <= nov < nper)


def _hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _spectra(x, nperseg, noverlap):
    """x [p, T] -> two-sided spectra [nseg, p, F] (complex128) of the detrended, Hann-windowed segments."""
    step = nperseg - noverlap
    nseg = (x.shape[1] - noverlap) // step
    seg = np.stack([x[:, s * step:s * step + nperseg] for s in range(nseg)]).astype(np.float64)
    seg = (seg - seg.mean(axis=-1, keepdims=True)) * _hann(nperseg)
    return np.fft.fft(seg, axis=-1)


def _cpsd_two_sided(x, fs, par):
    """The reference's csd(X[:, None], X[:, :, None], return_onesided=False) of one window x [p, T]:
    (f [F], cpsd [F, p, p]) with cpsd[f, i, j] = mean_s conj(X_j) X_i * scale, in x's precision."""
    single = x.dtype == np.float32
    if _standard(par, x.shape[1]):
        F = int(par["nperseg"])
        X = _spectra(x, F, int(par["noverlap"]))
        scale = 1.0 / (fs * np.sum(_hann(F) ** 2)) / X.shape[0]
        c = np.einsum("sif,sjf->fij", X, X.conj()) * scale
        f = np.fft.fftfreq(F, 1.0 / fs)
    else:
        from scipy.signal import csd
        f, c = csd(x[np.newaxis], x[:, np.newaxis], fs=fs, return_onesided=False, **par)
        c = np.moveaxis(c, -1, 0)
    return f, c.astype(np.complex64 if single else np.complex128)


def _n_segments(par, T):
    if not _standard(par, T):
        nper = min(int(par["nperseg"]), T)
        nov = int(par["noverlap"]) if par["noverlap"] is not None else nper // 2
        return max((T - nov) // max(nper - nov, 1), 1)
    return (T - int(par["noverlap"])) // (int(par["nperseg"]) - int(par["noverlap"]))


# --------------------------------------------------------------------------- Wilson factorisation
def _cond_hermitian_2x2(c):
    """Ratio of the singular values of the Hermitian 2x2 matrices c [F, 2, 2], in c's precision."""
    real = np.float32 if c.dtype == np.complex64 else np.float64
    a, d = c[:, 0, 0].real.astype(np.float64), c[:, 1, 1].real.astype(np.float64)
    ab = np.abs(c[:, 0, 1].astype(np.complex128))
    m, h = 0.5 * (a + d), 0.5 * (a - d)
    r = np.sqrt(h * h + ab * ab)
    hi, lo = np.abs(m + r), np.abs(m - r)
    hi, lo = np.maximum(hi, lo), np.minimum(hi, lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = (hi / lo).astype(real)
    return np.where(np.isnan(cond), np.inf, cond)


def _is_singular(c, n_segments):
    if n_segments < 2:
        return True
    eps = np.finfo(c.dtype).eps
    cond = _cond_hermitian_2x2(c) if c.shape[-1] == 2 else np.linalg.cond(c)
    return bool(np.any(cond > 1.0 / eps))


def _small_change(x, x0, tol):
    """Largest relative change below tol, in x's precision (entries of size <= 2 eps count as 1)."""
    mag = np.abs(x)
    diff = np.abs(x - x0)
    mag[mag <= 2 * np.finfo(mag.dtype).eps] = 1
    return (diff / mag).max() < tol


def _wilson(c, max_iter, tol, singular):
    """Factorise the CPSD c [F, n, n] of one window into the transfer function H [F, n, n] and the innovation
    covariance Sigma [n, n] (Wilson 1972).  Returns (H, Sigma, status, iterations); raises
    numpy.linalg.LinAlgError on a non-positive Cholesky pivot."""
    F, n = c.shape[0], c.shape[-1]
    if singular:
        # a float64 diagonal: the sum is complex128 whatever c was, as in the reference
        c = c + np.eye(n) * np.spacing(np.abs(c)).max() * EPS_MULTIPLIER
    lag0 = c.sum(axis=0, dtype=np.complex128) / F
    lag0 = lag0.astype(c.dtype)
    gamma0 = np.real((lag0 + lag0.conj().T) / 2.0)
    A0 = np.linalg.cholesky(gamma0).T.copy()
    psi = np.repeat(A0[np.newaxis], F, axis=0).astype(np.complex128)
    L = np.linalg.cholesky(c)
    half = F // 2
    eye = np.identity(n)
    status, it = MAXITER, 0
    while it < max_iter:
        it += 1
        y = np.linalg.solve(psi, L)
        g = y @ y.conj().transpose(0, 2, 1) + eye
        lags = np.fft.ifft(g, axis=0).real
        lags[0] *= 0.5
        if F % 2 == 0:
            lags[half] *= 0.5
        lags[half + 1:] = 0
        g0 = lags[0]
        skew = -np.tril(g0, -1)
        skew = skew - skew.T                      # g0 + skew is upper triangular
        psi_new = psi @ (np.fft.fft(lags, axis=0) + skew)
        A0_new = (A0 @ (g0 + skew)).astype(A0.dtype)
        done = _small_change(psi_new, psi, tol) and _small_change(A0_new, A0, tol)
        psi, A0 = psi_new, A0_new
        if done:
            status = CONVERGED
            break
    H = np.linalg.solve(A0.T[np.newaxis], psi.transpose(0, 2, 1)).transpose(0, 2, 1)
    return H, A0 @ A0.T, status, it


def _pair_spectra(H, Sigma):
    """(ds01, ds10) [F] of a 2-channel factorisation: power at channel 1 explained by channel 0's innovations
    beyond what channel 1's own explain, and the converse."""
    s00, s01, s10, s11 = Sigma[0, 0], Sigma[0, 1], Sigma[1, 0], Sigma[1, 1]
    sig1_0 = s11 - s10 * (s10 / s00)
    sig0_1 = s00 - s01 * (s01 / s11)
    ds10 = np.real(H[:, 0, 1] * sig1_0 * H[:, 0, 1].conj())
    ds01 = np.real(H[:, 1, 0] * sig0_1 * H[:, 1, 0].conj())
    return ds01, ds10


def _pairs(p):
    return [(a, b) for a in range(p) for b in range(a + 1, p)]


def _window_two_sided(x, fs, par, pairwise, max_iter, tol, warn=True):
    """x [p, T] -> (f [F], ds [F, p, p] float64 two-sided, status [npairs], iters [npairs], singular [npairs])."""
    p, T = x.shape
    f, c = _cpsd_two_sided(x, fs, par)
    nseg = _n_segments(par, T)
    ds = np.zeros((c.shape[0], p, p))
    pairs = _pairs(p)
    status = np.zeros(len(pairs), np.int32)
    iters = np.zeros(len(pairs), np.int32)
    flags = np.zeros(len(pairs), bool)
    if not pairwise:
        sing = _is_singular(c, nseg)
        H, Sigma, st, it = _wilson(c, max_iter, tol, sing)
        status[:], iters[:], flags[:] = st, it, sing
    for q, (a, b) in enumerate(pairs):
        ix = np.array([a, b])
        if pairwise:
            sub = c[:, ix][:, :, ix]
            flags[q] = _is_singular(sub, nseg)
            Hq, Sq, status[q], iters[q] = _wilson(sub, max_iter, tol, flags[q])
        else:
            Hq, Sq = H[:, ix][:, :, ix], Sigma[ix][:, ix]
        ds[:, a, b], ds[:, b, a] = _pair_spectra(Hq, Sq)
    if warn and flags.any():
        warnings.warn("CPSD matrix is singular!")
    if warn and (status == MAXITER).any():
        warnings.warn("Wilson factorization failed to converge.")
    return f, ds, status, iters, flags


def _fold(f, ds):
    """Two-sided [F, ...] -> one-sided [F // 2 + 1, ...]: interior bins doubled, the Nyquist bin only for odd F."""
    F = len(f)
    half = F // 2
    ds = ds[:half + 1].copy()
    ds[1:half] *= 2
    if F % 2 != 0:
        ds[half] *= 2
    return np.abs(f[:half + 1]), ds


def get_directed_spectrum(X, fs, pairwise=True, max_iter=1000, tol=1e-6, csd_params={}):
    """The directed spectrum of X ([n_roi, time] or [n_window, n_roi, time]), host route.

    Returns f [n_freq] and ds [n_window, n_freq, n_roi, n_roi] (float64, one-sided; ds[w, :, i, j] is the
    spectrum directed from channel i to channel j).  Unlike the reference, windows of one call do not share the
    singular-branch decision: each is treated as the data sets treat it, alone."""
    X = np.asarray(X)
    if X.ndim == 2:
        X = X[np.newaxis]
    assert X.ndim == 3, f"len({X.shape}) != 3"
    par = _params(csd_params)
    out = []
    for x in X:
        f, ds, _, _, _ = _window_two_sided(x, fs, par, pairwise, max_iter, tol)
        f1, ds1 = _fold(f, ds)
        out.append(ds1)
    return f1, np.stack(out)


def _power(x, fs, par):
    """One window x [p, T] -> (f one-sided, |CPSD| [p (p + 1) / 2, n_freq] before the crop and the scaling)."""
    p = x.shape[0]
    if _standard(par, x.shape[1]):
        F = int(par["nperseg"])
        X = _spectra(x, F, int(par["noverlap"]))
        half = F // 2
        scale = 1.0 / (fs * np.sum(_hann(F) ** 2)) / X.shape[0]
        c = np.einsum("sif,sjf->ijf", X.conj(), X)[..., :half + 1] * scale
        c[..., 1:half] *= 2
        if F % 2:
            c[..., half] *= 2
        c = c.astype(np.complex64 if x.dtype == np.float32 else np.complex128)
        f = np.arange(half + 1) * (1.0 / (F * (1.0 / fs)))
    else:
        from scipy.signal import csd
        f, c = csd(x[:, np.newaxis], x[np.newaxis], fs=fs, **par)
    mag = np.abs(c)
    rows = [mag[i, j] for i in range(p) for j in range(i + 1)]
    return f, np.stack(rows).astype(np.float64)


def make_high_level_signal_features(X, fs=1000, min_freq=0.0, max_freq=55.0, directed_spectrum=False,
                                    csd_params=DEFAULT_CSD_PARAMS, max_iter=1000, tol=1e-6):
    """Features of one window X [n_time_steps, n_channel] (host route): ``power``
    [1, n_channel (n_channel + 1) / 2, n_freq], ``freq`` [n_freq] and, with ``directed_spectrum``, ``dir_spec``
    [1, n_channel, n_channel, n_freq]; both scaled by frequency and cropped to [min_freq, max_freq).  A window
    holding a NaN gives NaN features."""
    X = np.asarray(X)
    assert X.ndim == 2 and X.shape[1] >= 1
    x = np.ascontiguousarray(X.T)
    par = _params(csd_params)
    bad = bool(np.isnan(x).any())
    if bad:  # the shapes and bins come from a stand-in window; every feature is set to NaN below
        x = np.random.RandomState(0).randn(*x.shape).astype(x.dtype)
    f, mag = _power(x, fs, par)
    i1, i2 = np.searchsorted(f, [min_freq, max_freq])
    freq = f[i1:i2]
    power = mag[np.newaxis, :, i1:i2] * freq
    if bad:
        power[:] = np.nan
    res = {"power": power, "freq": freq}
    if directed_spectrum:
        if bad:
            res["dir_spec"] = np.full((1, x.shape[0], x.shape[0], len(freq)), np.nan)
        else:
            ft, ds = get_directed_spectrum(x, fs, max_iter=max_iter, tol=tol, csd_params=par)
            ds = ds[:, i1:i2] * ft[i1:i2].reshape(1, -1, 1, 1)
            res["dir_spec"] = np.moveaxis(ds, 1, -1)
    return res


def flatten_directed_spectrum_features(x):
    """(n, n, m) -> (n, m (2n - 1)): row j holds, per feature, x[j, :] and then column j without its diagonal
    entry (the inverse of dcsfa_nmf.unflatten_directed_spectrum_features)."""
    x = np.asarray(x)
    assert x.ndim == 3 and x.shape[0] == x.shape[1]
    n, _, m = x.shape
    out = np.zeros((n, m, 2 * n - 1))
    for j in range(n):
        out[j, :, :n] = x[j].T
        out[j, :, n:] = np.delete(x[:, j, :], j, axis=0).T
    return out.reshape(n, m * (2 * n - 1))


# --------------------------------------------------------------------------- the batched entry
def _n_freq(nperseg, fs, min_freq, max_freq):
    f = np.arange(nperseg // 2 + 1) * (1.0 / (nperseg * (1.0 / fs)))
    i1, i2 = np.searchsorted(f, [min_freq, max_freq])
    return int(i1), int(max(i2, i1))


def _layout_row(ds_pf, layout):
    """ds_pf [p, p, n_f] -> the feature row of the reference's __getitem__."""
    if layout == "vanilla":
        return ds_pf.reshape(-1)
    return flatten_directed_spectrum_features(ds_pf).reshape(-1)


def _host_features(X, fs, min_freq, max_freq, par, layout, max_iter, tol, want_power):
    N, T, p = X.shape
    rows, stats, its, powers = [], [], [], []
    npairs = p * (p - 1) // 2
    for n in range(N):
        x = np.ascontiguousarray(X[n].T)
        if np.isnan(x).any():
            rows.append(None)
            stats.append(np.zeros(npairs, np.int32))
            its.append(np.zeros(npairs, np.int32))
            powers.append(None)
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f, ds, st, it, _ = _window_two_sided(x, fs, par, True, max_iter, tol, warn=False)
        f1, ds1 = _fold(f, ds)
        i1, i2 = np.searchsorted(f1, [min_freq, max_freq])
        ds1 = ds1[i1:i2] * f1[i1:i2].reshape(-1, 1, 1)
        rows.append(_layout_row(np.moveaxis(ds1, 0, -1), layout).astype(np.float32))
        stats.append(st)
        its.append(it)
        if want_power:
            fp, mag = _power(x, fs, par)
            powers.append(mag[:, i1:i2] * fp[i1:i2])
    ref = next((r for r in rows if r is not None), None)
    if ref is None:
        F = min(int(par["nperseg"]), T)
        i1, i2 = _n_freq(F, fs, min_freq, max_freq)
        width = (p * p if layout == "vanilla" else p * (2 * p - 1)) * (i2 - i1)
        ref = np.zeros(width, np.float32)
        pref = np.zeros((p * (p + 1) // 2, i2 - i1))
    else:
        pref = next((q for q in powers if q is not None), None)
    out = np.stack([np.full_like(ref, np.nan) if r is None else r for r in rows]) if N else np.zeros((0, ref.size), np.float32)
    info = {"status": np.stack(stats) if N else np.zeros((0, npairs), np.int32),
            "iterations": np.stack(its) if N else np.zeros((0, npairs), np.int32), "route": "host"}
    if want_power:
        info["power"] = np.stack([np.full_like(pref, np.nan) if q is None else q for q in powers])
    return out, info


def device_supported(T, p, par):
    """True when the library's kernels cover this shape (redcliff_dirspec_supported)."""
    if not _standard(par, T) or p < 2:
        return False
    from . import _native
    return bool(_native.lib().redcliff_dirspec_supported(int(T), int(p), int(par["nperseg"]), int(par["noverlap"])))


def _device_features(X, fs, min_freq, max_freq, par, layout, max_iter, tol, device, want_power, out=None):
    import ctypes

    import torch

    from . import _native as nat
    L = nat.lib()
    if not torch.is_tensor(X):
        X = torch.from_numpy(np.ascontiguousarray(X))
    dev = torch.device(device if device is not None else (X.device if X.is_cuda else "cuda"))
    X = X.to(dev)
    if X.stride(2) != 1 or X.stride(1) < X.shape[2] or (X.shape[0] > 1 and X.stride(0) < (X.shape[1] - 1) * X.stride(1) + X.shape[2]):
        X = X.contiguous()
    N, T, p = X.shape
    F, nov = int(par["nperseg"]), int(par["noverlap"])
    i1, i2 = _n_freq(F, fs, min_freq, max_freq)
    nf = i2 - i1
    got = L.redcliff_dirspec_nfreq(F, float(fs), float(min_freq), float(max_freq))
    if got != nf:
        raise RuntimeError("directed spectrum: the library keeps %d bins, numpy.searchsorted %d" % (got, nf))
    width = (p * p if layout == "vanilla" else p * (2 * p - 1)) * nf
    npairs = p * (p - 1) // 2
    if out is None:
        out = torch.empty((N, width), dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.shape == (N, width) and (width == 0 or out.stride(1) == 1)
    status = torch.zeros((N, npairs), dtype=torch.int32, device=dev)
    iters = torch.zeros((N, npairs), dtype=torch.int32, device=dev)
    power = torch.empty((N, p * (p + 1) // 2, nf), dtype=torch.float64, device=dev) if want_power else None
    if N > 0:
        nbytes = int(L.redcliff_dirspec_ws_bytes(N, T, p, F, nov))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        a = nat.DirspecArgs()
        a.N, a.T, a.p, a.nperseg, a.noverlap, a.max_iter = N, T, p, F, nov, int(max_iter)
        a.dtype = 0 if X.dtype == torch.float32 else 1
        a.layout = 0 if layout == "vanilla" else 1
        a.fs, a.min_freq, a.max_freq, a.tol = float(fs), float(min_freq), float(max_freq), float(tol)
        a.X, a.x_wstride, a.x_tstride = X.data_ptr(), X.stride(0) if N > 1 else T * X.stride(1), X.stride(1)
        a.out, a.out_rstride = out.data_ptr(), out.stride(0) if N > 1 else max(width, 1)
        a.power = power.data_ptr() if want_power else None
        a.ws, a.ws_bytes = ws.data_ptr(), nbytes
        a.status, a.iters = status.data_ptr(), iters.data_ptr()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            nat.check(L.redcliff_dirspec_run(ctypes.byref(a), ctypes.c_void_p(stream)), "dirspec_run")
    info = {"status": status.cpu().numpy(), "iterations": iters.cpu().numpy(), "route": "fused"}
    if want_power:
        info["power"] = power.cpu().numpy()
    return out, info


def directed_spectrum_features(X, fs, min_freq, max_freq, csd_params, layout="vanilla", max_iter=1000, tol=1e-6,
                               device=None, return_info=False, power=False):
    """The feature matrix the reference's data sets produce one item at a time.

    X: [N, T, p] float32 or float64, numpy or torch, host or device.  Returns [N, p p n_f] (``"vanilla"``) or
    [N, p n_f (2p - 1)] (``"flattened"``) float32: a torch tensor on the device from the device route, a numpy
    array from the host route.  ``return_info`` adds a dict with ``status`` and ``iterations`` [N, pairs],
    ``route`` and, with ``power=True``, ``power`` [N, p (p + 1) / 2, n_f] (float64).
    The device route runs when the library supports the shape and a GPU is present;
    REDCLIFF_DIRSPEC_PATH=host|fused overrides the choice.  A non-positive Cholesky pivot raises
    numpy.linalg.LinAlgError on either route; pairs that hit max_iter warn and keep their last iterate."""
    if layout not in ("vanilla", "flattened"):
        raise ValueError("layout must be 'vanilla' or 'flattened'")
    par = _params(csd_params)
    is_t = hasattr(X, "detach")
    shape, dt = tuple(X.shape), str(X.dtype).replace("torch.", "")
    if len(shape) != 3:
        raise ValueError("X must be [N, T, p]")
    if dt not in ("float32", "float64"):
        raise TypeError("X must be float32 or float64")
    forced = os.environ.get("REDCLIFF_DIRSPEC_PATH", "")
    if forced not in ("", "host", "fused"):
        raise ValueError("REDCLIFF_DIRSPEC_PATH must be host or fused")
    if forced == "host":
        fused = False
    else:
        import torch
        fused = torch.cuda.is_available() and device_supported(shape[1], shape[2], par)
        if forced == "fused" and not fused:
            raise RuntimeError("REDCLIFF_DIRSPEC_PATH=fused: no GPU, or shape outside redcliff_dirspec_supported "
                               "(T=%d p=%d csd_params=%r)" % (shape[1], shape[2], par))
    if fused:
        out, info = _device_features(X, fs, min_freq, max_freq, par, layout, max_iter, tol, device, power)
    else:
        Xh = X.detach().cpu().numpy() if is_t else np.asarray(X)
        out, info = _host_features(Xh, fs, min_freq, max_freq, par, layout, max_iter, tol, power)
    if (info["status"] == PIVOT).any():
        w, q = np.argwhere(info["status"] == PIVOT)[0]
        raise np.linalg.LinAlgError("directed spectrum: non-positive Cholesky pivot (window %d, pair %d)" % (w, q))
    if (info["status"] == MAXITER).any():
        warnings.warn("Wilson factorization failed to converge for %d (window, pair) problems."
                      % int((info["status"] == MAXITER).sum()))
    return (out, info) if return_info else out
