"""Generate tests/golden/cemb_recording_scores.npz from the REFERENCE itself (build container only).

    python tests/golden/make_cemb_recording_golden.py

The reference's two recording-scoring functions (general_utils/misc.py:57-81) run on seeded
reference models whose factor-score embedder is the cEmbedder
(models/redcliff_factor_score_embedders.py:183-331), every embedder parameter moved off its
initial value by a seeded perturbation.  The reference is imported as in make_golden.py
(oracle/ref_import.py).  Only data leaves this script.  Keys, per scenario s in (a, b, c):
  s/meta              JSON: constructor arguments and the scoring arguments
  s/state/<key>       state_dict of model.factor_score_embedder
  s/recording         (1, T, p) float32
  s/weightings        obtain_factor_score_weightings_across_recording      (nsup, steps) float64
  s/classifications   obtain_factor_score_classifications_across_recording (nsup, steps) float64
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402
from oracle.redcliff_oracle import reference_coeffs  # noqa: E402

REF = import_reference()
MISC = importlib.import_module("general_utils.misc")

BASE = dict(L=3, h=6, T=48, gc_mode="conditional_factor_fixed_embedder",
            fwd_mode="apply_factor_weights_after_sim_completion",
            training_mode="pretrain_embedder_then_acclimate_factors_then_combined", pre=1, acc=1)
SCENARIOS = {
    "a": dict(BASE, p=5, F=7, eh=6, K=3, nsup=2, sigmoid=False, seed=61, data_seed=71),
    # the sigmoid restriction: class scores differ from the weightings
    "b": dict(BASE, p=5, F=7, eh=6, K=3, nsup=2, sigmoid=True, seed=62, data_seed=72),
    # p == F: the cEmbedder reads the window time-major all the same (no transpose rule as the DGCNN's)
    "c": dict(BASE, p=7, F=7, eh=6, K=2, nsup=1, sigmoid=False, seed=63, data_seed=73),
}


def build(cfg):
    torch.manual_seed(cfg["seed"])
    eargs = [("sigmoid_eccentricity_coeff", 10.0), ("lag", cfg["F"]), ("hidden", [cfg["eh"]])]
    coeff = reference_coeffs(cfg["K"], cfg["p"])
    m = REF.redcliff_smooth.REDCLIFF_S_CMLP_withStateSmoothing(
        cfg["p"], cfg["L"], [cfg["h"]], cfg["F"], [0], cfg["L"], 1, cfg["K"], cfg["nsup"], coeff, cfg["sigmoid"],
        "cEmbedder", eargs, cfg["gc_mode"], cfg["fwd_mode"], num_sims=1, wavelet_level=None, save_path=None,
        training_mode=cfg["training_mode"], num_pretrain_epochs=cfg["pre"], num_acclimation_epochs=cfg["acc"],
        STATE_SCORE_SMOOTHING_EPSILON=0.0001).float()
    rng = np.random.RandomState(cfg["seed"] + 100)
    with torch.no_grad():
        for prm in m.factor_score_embedder.parameters():
            prm.add_(torch.from_numpy((0.1 * rng.randn(*prm.shape)).astype(np.float32)))
    m.eval()
    return m, coeff


def main():
    out = {}
    for name, cfg in SCENARIOS.items():
        m, coeff = build(cfg)
        rng = np.random.RandomState(cfg["data_seed"])
        X = rng.randn(1, cfg["T"], cfg["p"]).astype(np.float32)
        for t in range(2, cfg["T"]):
            X[:, t] += 0.3 * X[:, t - 1] - 0.1 * X[:, t - 2]
        hist = cfg["F"]
        steps = cfg["T"] - hist
        sig = torch.from_numpy(X)
        with torch.no_grad():
            wts = MISC.obtain_factor_score_weightings_across_recording(m, sig, cfg["nsup"], steps, hist)
            cls = MISC.obtain_factor_score_classifications_across_recording(m, sig, cfg["nsup"], steps, hist)
        pre = name + "/"
        for k, v in m.factor_score_embedder.state_dict().items():  # the factors play no part in the scores
            out[pre + "state/" + k] = v.detach().cpu().numpy().copy()
        out[pre + "recording"] = X
        out[pre + "weightings"] = np.asarray(wts, dtype=np.float64)
        out[pre + "classifications"] = np.asarray(cls, dtype=np.float64)
        meta = dict(cfg, coeff=coeff, num_supervised_factors=cfg["nsup"], num_timesteps_to_score=steps,
                    num_timesteps_in_input_history=hist)
        out[pre + "meta"] = np.asarray(json.dumps(meta))
    path = os.path.join(HERE, "cemb_recording_scores.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
