"""Directed-spectrum features on the device (csrc/rc_dirspec.hip through redcliff_dirspec_run) against the
reference's outputs in tests/golden/dirspec.npz, under the bounds of tests/dirspec_common.py, plus the properties
of the call itself: determinism, batch independence, the NaN window, the row stride and the shape limit."""
import warnings

import numpy as np
import pytest
import torch

import dirspec_common as C
from redcliff_amd import directed_spectrum as D

pytestmark = pytest.mark.gpu


def run(sc, X=None, layout="vanilla", path="fused", power=True):
    import os
    old = os.environ.get("REDCLIFF_DIRSPEC_PATH")
    os.environ["REDCLIFF_DIRSPEC_PATH"] = path
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out, info = D.directed_spectrum_features(sc["X"] if X is None else X, sc["fs"], sc["min_freq"], sc["max_freq"],
                                                     sc["csd_params"], layout=layout, max_iter=sc["max_iter"], tol=sc["tol"],
                                                     return_info=True, power=power)
    finally:
        if old is None:
            del os.environ["REDCLIFF_DIRSPEC_PATH"]
        else:
            os.environ["REDCLIFF_DIRSPEC_PATH"] = old
    assert info["route"] == path
    return (out.cpu().numpy() if torch.is_tensor(out) else out), info


@pytest.mark.parametrize("name", C.NAMES)
def test_device_route_matches_reference(name):
    sc = C.scenario(name)
    out, info = run(sc)
    assert out.dtype == np.float32
    C.check(sc, C.unpack(sc, out), info["power"], info["status"], info["iterations"], "device")


@pytest.mark.parametrize("name", ["pub20_p10_f32", "wp20_p3_f32", "wp12_p3_f64", "wp256_p2_f64"])
def test_two_runs_and_device_input_give_the_same_bits(name):
    sc = C.scenario(name)
    a, ia = run(sc)
    b, ib = run(sc)
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(ia["power"], ib["power"], equal_nan=True)
    assert np.array_equal(ia["iterations"], ib["iterations"])
    c, ic = run(sc, X=torch.from_numpy(sc["X"]).cuda())
    assert np.array_equal(a, c, equal_nan=True) and np.array_equal(ia["iterations"], ic["iterations"])


@pytest.mark.parametrize("name", ["pub20_p10_f32", "wp12_p3_f64"])
def test_a_window_alone_equals_the_window_in_a_batch(name):
    """N = 5 with one NaN window: the number of problems is no multiple of the waves per workgroup, the NaN
    window's row is NaN and its neighbours are what they are without it."""
    sc = C.scenario(name)
    both, info = run(sc)
    nan_at = sc["nan_window"]
    assert np.isnan(both[nan_at]).all() and np.isnan(info["power"][nan_at]).all()
    for n in sc["rows"]:
        alone, ia = run(sc, X=sc["X"][n:n + 1])
        assert np.array_equal(alone[0], both[n])
        assert np.array_equal(ia["iterations"][0], info["iterations"][n])
        assert np.array_equal(ia["power"][0], info["power"][n])
    healed = sc["X"].copy()
    healed[nan_at] = sc["X"][sc["rows"][0]]
    other, _ = run(sc, X=healed)
    keep = [n for n in range(sc["N"]) if n != nan_at]
    assert np.array_equal(other[keep], both[keep]) and np.array_equal(other[nan_at], both[sc["rows"][0]])


@pytest.mark.parametrize("name", ["wp20_p10_f32", "wp20_p10_f64", "wp12_p3_f64", "wp12_p3_f64_it3", "pub50_p3_f64"])
def test_statuses_and_counts_agree_with_the_host_route(name):
    sc = C.scenario(name)
    _, dev = run(sc, power=False)
    _, host = run(sc, path="host", power=False)
    if sc["segments"] >= 2:
        sel = np.zeros(dev["status"].shape, bool)
        sel[sc["rows"]] = sc["flagged"] if sc["max_iter"] >= 1000 else True
        assert np.array_equal(dev["status"][sel], host["status"][sel])
        assert np.array_equal(dev["iterations"][sel], host["iterations"][sel])
    else:   # the published regime: both report a status and a count below max_iter; the counts are not compared
        assert set(np.unique(dev["status"])) <= {0, 1} and (dev["iterations"][sc["rows"]] > 0).all()


@pytest.mark.parametrize("layout", ["vanilla", "flattened"])
def test_layouts_and_row_stride(layout):
    sc = C.scenario("wp20_p3_f32")
    host, _ = run(sc, layout=layout, path="host", power=False)
    dense, _ = run(sc, layout=layout, power=False)
    p, nf = sc["p"], len(sc["freq"])
    width = (p * p if layout == "vanilla" else p * (2 * p - 1)) * nf
    assert dense.shape == (sc["N"], width)
    van, _ = run(sc, power=False)
    for n in sc["rows"]:   # the device's flattened row is the flattening of its vanilla row
        want = van[n].reshape(p, p, nf) if layout == "vanilla" else D.flatten_directed_spectrum_features(van[n].reshape(p, p, nf))
        assert np.array_equal(dense[n], want.reshape(-1).astype(np.float32))
    assert np.allclose(dense, host, rtol=1e-4, atol=0, equal_nan=True)
    # a wider buffer: only the rows' own columns are written
    buf = torch.full((sc["N"] + 2, width + 7), -7.0, dtype=torch.float32, device="cuda")
    view = buf[1:-1, 3:3 + width]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        D._device_features(sc["X"], sc["fs"], sc["min_freq"], sc["max_freq"], D._params(sc["csd_params"]), layout, sc["max_iter"],
                           sc["tol"], None, False, out=view)
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:-1, 3:3 + width], dense, equal_nan=True)
    assert (got[0] == -7).all() and (got[-1] == -7).all() and (got[:, :3] == -7).all() and (got[:, 3 + width:] == -7).all()


def test_nperseg_above_the_limit_takes_the_host_route():
    from redcliff_amd import _native as nat
    L = nat.lib()
    assert L.redcliff_dirspec_supported(300, 2, 256, 128) == 1
    assert L.redcliff_dirspec_supported(300, 2, 257, 128) == 0 and b"limits" in L.redcliff_last_error()
    assert L.redcliff_dirspec_ws_bytes(4, 300, 2, 257, 128) == 0
    rng = np.random.RandomState(5)
    X = rng.randn(1, 257 * 3, 2)
    par = {"detrend": "constant", "window": "hann", "nperseg": 257, "noverlap": 0, "nfft": None}
    out, info = D.directed_spectrum_features(X, 1000.0, 0.0, 100.0, par, return_info=True)
    assert info["route"] == "host" and isinstance(out, np.ndarray) and np.isfinite(out).all()
    par["nperseg"] = 256
    out, info = D.directed_spectrum_features(X, 1000.0, 0.0, 100.0, par, return_info=True)
    assert info["route"] == "fused" and torch.is_tensor(out) and out.is_cuda
