"""Directed-spectrum features, host route (redcliff_amd/directed_spectrum.py) and the ``*_as_matrices`` loaders,
against the reference's own outputs in tests/golden/dirspec.npz (bounds: tests/dirspec_common.py)."""
import os
import pickle
import warnings

import numpy as np
import pytest

import dirspec_common as C
from redcliff_amd import data as RD
from redcliff_amd import dcsfa_nmf
from redcliff_amd import directed_spectrum as D

HERE = os.path.dirname(os.path.abspath(__file__))
LG = np.load(os.path.join(HERE, "golden", "loaders.npz"))


@pytest.fixture(autouse=True)
def host_route(monkeypatch):
    monkeypatch.setenv("REDCLIFF_DIRSPEC_PATH", "host")


def run_host(sc, layout="vanilla"):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, info = D.directed_spectrum_features(sc["X"], sc["fs"], sc["min_freq"], sc["max_freq"], sc["csd_params"],
                                                 layout=layout, max_iter=sc["max_iter"], tol=sc["tol"], return_info=True,
                                                 power=True)
    return out, info


@pytest.mark.parametrize("name", C.NAMES)
def test_host_route_matches_reference(name):
    sc = C.scenario(name)
    out, info = run_host(sc)
    assert out.dtype == np.float32 and info["route"] == "host"
    C.check(sc, C.unpack(sc, out), info["power"], info["status"], info["iterations"], "host")


def test_single_window_functions_return_the_reference_shapes():
    sc = C.scenario("wp9_p2_f64")     # odd F: the Nyquist bin is doubled
    x = sc["X"][0]                    # [T, p]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f, ds = D.get_directed_spectrum(x.T, sc["fs"], csd_params=sc["csd_params"])
        feats = D.make_high_level_signal_features(x, fs=sc["fs"], min_freq=sc["min_freq"], max_freq=sc["max_freq"],
                                                  directed_spectrum=True, csd_params=sc["csd_params"])
    F = sc["nperseg"]
    assert f.shape == (F // 2 + 1,) and ds.shape == (1, F // 2 + 1, 2, 2) and ds.dtype == np.float64
    assert np.allclose(f, np.arange(F // 2 + 1) * sc["fs"] / F)
    assert np.array_equal(feats["freq"], sc["freq"])
    assert feats["dir_spec"].shape == (1, 2, 2, len(sc["freq"])) and feats["power"].shape == (1, 3, len(sc["freq"]))
    scale = 1e3 * max(sc["spread"][0], sc["tolgap"][0])
    assert np.abs(feats["dir_spec"][0] - sc["ds"][0]).max() <= scale
    # the fold: two-sided bins k and F - k are equal for a real signal, so one-sided = 2 * two-sided off bin 0
    _, two, _, _, _ = D._window_two_sided(np.ascontiguousarray(x.T), sc["fs"], sc["csd_params"], True, 1000, 1e-6, warn=False)
    assert np.allclose(ds[0, 1:], 2 * two[1:F // 2 + 1]) and np.allclose(ds[0, 0], two[0])
    even = C.scenario("wp12_p3_f64")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f2, ds2 = D.get_directed_spectrum(even["X"][0].T, even["fs"], csd_params=even["csd_params"])
    _, two2, _, _, _ = D._window_two_sided(np.ascontiguousarray(even["X"][0].T), even["fs"], even["csd_params"], True, 1000,
                                           1e-6, warn=False)
    assert f2[-1] == even["fs"] / 2 and np.allclose(ds2[0, -1], two2[6])   # even F: the Nyquist bin is not doubled
    # a window with a NaN
    bad = x.copy()
    bad[3, 1] = np.nan
    feats = D.make_high_level_signal_features(bad, fs=sc["fs"], min_freq=0.0, max_freq=600.0, directed_spectrum=True,
                                              csd_params=sc["csd_params"])
    assert np.isnan(feats["dir_spec"]).all() and np.isnan(feats["power"]).all()


def test_non_pairwise_and_scipy_parameters_take_the_host_route():
    sc = C.scenario("wp12_p3_f64")
    x = sc["X"][0].T
    f, full = D.get_directed_spectrum(x, sc["fs"], pairwise=False, csd_params=sc["csd_params"])
    assert full.shape == (1, 7, 3, 3) and np.isfinite(full).all() and (full >= 0).all()
    par = dict(sc["csd_params"], nfft=16)
    f, ds = D.get_directed_spectrum(x, sc["fs"], csd_params=par)
    assert ds.shape == (1, 9, 3, 3) and np.isfinite(ds).all()
    assert not D.device_supported(x.shape[1], 3, par)
    assert not D.device_supported(x.shape[1], 3, dict(sc["csd_params"], detrend="linear"))
    assert not D.device_supported(x.shape[1], 3, dict(sc["csd_params"], window="hamming"))


def test_flatten_matches_reference_and_round_trips():
    x = C.G["flat/in"]
    flat = D.flatten_directed_spectrum_features(x)
    assert np.array_equal(flat, C.G["flat/out"])
    # the flat form holds every off-diagonal entry twice and the reference's unflatten adds both copies
    # (general_utils/misc.py:178-195), so the round trip doubles them; the diagonal of a directed spectrum is 0
    assert (x[np.arange(3), np.arange(3)] == 0).all()
    assert np.array_equal(dcsfa_nmf.unflatten_directed_spectrum_features(flat), 2 * x)
    sc = C.scenario("wp20_p3_f32")
    van, _ = run_host(sc, "vanilla")
    fl, _ = run_host(sc, "flattened")
    p, nf = sc["p"], len(sc["freq"])
    assert fl.shape == (sc["N"], p * nf * (2 * p - 1))
    for n in sc["rows"]:
        want = D.flatten_directed_spectrum_features(van[n].reshape(p, p, nf)).reshape(-1)
        assert np.array_equal(fl[n], want.astype(np.float32))


def test_batched_entry_equals_per_window_calls():
    """Point 1 of the contract: no decision crosses windows.  The batch mixes a window on the singular branch
    (its segments repeat the first, so every pair's CPSD is rank one) with a well-posed one."""
    sc = C.scenario("wp12_p3_f64")
    good = sc["X"][0]
    sing = good.copy()
    sing[0:24] = np.tile(good[0:6], (4, 1))                  # segments 0, 1, 2 (step 6) all hold the same 12 samples
    X = np.stack([sing, good, sc["X"][1]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        both, info = D.directed_spectrum_features(X, sc["fs"], 0.0, 600.0, sc["csd_params"], return_info=True)
        alone = [D.directed_spectrum_features(X[i:i + 1], sc["fs"], 0.0, 600.0, sc["csd_params"], return_info=True)
                 for i in range(3)]
    for i in range(3):
        assert np.array_equal(both[i], alone[i][0][0])
        assert np.array_equal(info["iterations"][i], alone[i][1]["iterations"][0])
    _, _, _, _, flags = D._window_two_sided(np.ascontiguousarray(sing.T), sc["fs"], sc["csd_params"], True, 1000, 1e-6,
                                            warn=False)
    _, _, _, _, flags_good = D._window_two_sided(np.ascontiguousarray(good.T), sc["fs"], sc["csd_params"], True, 1000, 1e-6,
                                                 warn=False)
    assert flags.all() and not flags_good.any()
    # the well-posed window's row is the fixture's, singular neighbour or not
    err = np.abs(both[1].reshape(3, 3, -1) - sc["ds"][0])
    store = 0.5 * np.spacing(np.abs(sc["ds"][0]).astype(np.float32) + np.abs(both[1].reshape(3, 3, -1)))
    assert (err <= 1e3 * max(sc["spread"][0], sc["tolgap"][0]) + store).all()


def test_non_psd_input_raises_linalg_error():
    c = np.zeros((8, 2, 2), complex)
    c[:, 0, 0] = 1.0
    c[:, 1, 1] = -1.0     # an indefinite "CPSD": the Cholesky factorisation must fail
    with pytest.raises(np.linalg.LinAlgError):
        D._wilson(c, 10, 1e-6, False)


# --------------------------------------------------------------------------- loaders
def rebuild(tmp, prefix, first_label_column=False):
    names = sorted(set(k.split("/")[2] for k in LG.files if k.startswith(prefix + "/file/")))
    for n in names:
        xs, ys = LG["%s/file/%s/x" % (prefix, n)], LG["%s/file/%s/y" % (prefix, n)]
        if first_label_column:
            ys = ys[:, :, 0]
        with open(os.path.join(tmp, n), "wb") as fh:
            pickle.dump([(x, y) for x, y in zip(xs, ys)], fh)


DSP = {"fs": 1000, "min_freq": 0.0, "max_freq": 250.0, "directed_spectrum": True,
       "csd_params": {"detrend": "constant", "window": "hann", "nperseg": 20, "noverlap": 10, "nfft": None}}


@pytest.mark.parametrize("fmt,layout", [("original flattened directed_spectrum vanilla", "vanilla"),
                                        ("original flattened directed_spectrum", "flattened")])
def test_dream4_as_matrices(tmp_path, fmt, layout):
    rebuild(str(tmp_path), "d4")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Xt, yt, Xv, yv = RD.load_normalized_DREAM4_data_train_test_split_as_matrices(
            str(tmp_path), signal_format=fmt, max_num_features_per_series=20, train_portion=0.67, dirspec_params=DSP)
    p, nf = 10, 5   # bins 0, 50, ..., 200 Hz
    width = p * p * nf if layout == "vanilla" else p * nf * (2 * p - 1)
    assert Xt.shape[1] == Xv.shape[1] == width and Xt.dtype == np.float32
    assert Xt.shape[0] + Xv.shape[0] == 11 and Xv.shape[0] > 0
    assert yt.shape == (Xt.shape[0], 4) and yv.shape == (Xv.shape[0], 4)
    for sub, X, y in (("train", Xt, yt), ("validation", Xv, yv)):
        ds = RD.NormalizedRecordingDirectory(str(tmp_path / sub), "dream4")
        Xn, Yn = ds.materialize(dtype=__import__("torch").float64)
        assert np.array_equal(y, Yn.numpy().astype(np.float32)) and (y.sum(axis=1) == 1).all()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = D.directed_spectrum_features(Xn[:, :20].numpy(), 1000, 0.0, 250.0, DSP["csd_params"], layout=layout)
        assert np.array_equal(X, want)
    files = lambda d: sorted(os.listdir(tmp_path / d))  # noqa: E731
    assert files("train") and files("validation") and not set(files("train")) & set(files("validation"))


def test_raw_flattened_format_and_lfp_loader(tmp_path):
    rebuild(str(tmp_path), "lfp", first_label_column=True)
    Xt, yt, Xv, yv = RD.load_normalized_lfp_data_train_test_split_as_matrices(
        str(tmp_path), signal_format="original flattened", max_num_features_per_series=7, train_portion=0.67,
        grid_search=False)
    assert Xt.shape[1] == 7 * 6 and yt.shape[1] == 3
    ds = RD.NormalizedRecordingDirectory(str(tmp_path / "train"), "lfp", grid_search=False)
    assert Xt.shape[0] == len(ds)
    assert np.array_equal(Xt[0], ds[0][0][:7].reshape(-1).numpy())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Xd, yd, _, _ = RD.load_normalized_lfp_data_train_test_split_as_matrices(
            str(tmp_path), signal_format="original flattened directed_spectrum vanilla", max_num_features_per_series=20,
            train_portion=0.67, dirspec_params=DSP, grid_search=False, average_region_map={"amy": [0, 2], "hip": [1], "pfc": [3, 4, 5]})
    assert Xd.shape == (Xt.shape[0], 3 * 3 * 5) and np.isfinite(Xd).all()
    with pytest.raises(ValueError):
        RD.load_normalized_lfp_data_train_test_split_as_matrices(str(tmp_path), signal_format="original directed_spectrum",
                                                                 dirspec_params=None)
