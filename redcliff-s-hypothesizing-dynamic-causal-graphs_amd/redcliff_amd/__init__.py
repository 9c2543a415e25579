"""MI355X-native REDCLIFF-S cMLP factor-model fitting path.

Drop-in classes for the reference's models/ modules; compute in libredcliff_hip.so
(gfx950 HIP kernels, C-ABI in include/redcliff_hip.h)."""
from .cmlp import MLP, cMLP
from .dgcnn import DGCNN, DGCNN_Model, fit_dgcnn_baselines
from .redcliff_factor_score_embedders import (DGCNN_Embedder, MLPClassifierForMultipleObjectives,
                                              MLPClassifierForSingleObjective, cEmbedder)
from .redcliff_s_cmlp import REDCLIFF_S_CMLP
from .redcliff_s_cmlp_withStateSmoothing import REDCLIFF_S_CMLP_withStateSmoothing
from .replicas import PerReplica, ReplicaPack, fit_packs, grid_packs, shard_grid
from .data_parallel import DataParallelFit
from .scoring import score_recordings
from .cmlp_fm import cMLP_FM, fit_baselines
from .clstm import LSTM, cLSTM
from .clstm_fm import cLSTM_FM, fit_lstm_baselines
from .navar import NAVAR, fit_navar_baselines
from .navar_lstm import NAVARLSTM, fit_navar_lstm_baselines
from .dcsfa_nmf import DcsfaFitPack, DcsfaNmf, FullDCSFAModel, FullDCSFAModel_GCv2, NmfBase, fit_dcsfa_baselines
from .directed_spectrum import (DEFAULT_CSD_PARAMS, directed_spectrum_features, flatten_directed_spectrum_features,
                                get_directed_spectrum, make_high_level_signal_features)
from .tidybench import (get_standardized_off_diagonal_relation_predictions, lasar, lasar_many, prepare_data_for_modeling, qrbs,
                        qrbs_many, run_lasar_experiment, run_tidybench_experiment, slarac, slarac_many)
from .dynotears_vanilla import DYNOTEARS_Model, fit_dynotears_baselines, from_numpy_dynamic, from_numpy_dynamic_many
from .data import (load_normalized_DREAM4_data_train_test_split_as_matrices,
                   load_normalized_DREAM4_data_train_test_split_as_tensors,
                   load_normalized_lfp_data_train_test_split_as_matrices)

__all__ = ["MLP", "cMLP", "DGCNN", "DGCNN_Model", "DGCNN_Embedder", "cEmbedder", "MLPClassifierForSingleObjective",
           "MLPClassifierForMultipleObjectives", "REDCLIFF_S_CMLP", "REDCLIFF_S_CMLP_withStateSmoothing", "ReplicaPack",
           "PerReplica", "fit_packs", "grid_packs", "shard_grid", "DataParallelFit",
           "score_recordings", "cMLP_FM", "fit_baselines", "LSTM", "cLSTM", "cLSTM_FM", "fit_lstm_baselines",
           "NAVAR", "fit_navar_baselines", "NAVARLSTM", "fit_navar_lstm_baselines", "fit_dgcnn_baselines",
           "NmfBase", "DcsfaNmf", "FullDCSFAModel", "FullDCSFAModel_GCv2", "DcsfaFitPack", "fit_dcsfa_baselines",
           "DEFAULT_CSD_PARAMS", "get_directed_spectrum", "make_high_level_signal_features",
           "flatten_directed_spectrum_features", "directed_spectrum_features",
           "slarac", "qrbs", "slarac_many", "qrbs_many", "lasar", "lasar_many", "run_lasar_experiment", "run_tidybench_experiment", "prepare_data_for_modeling",
           "get_standardized_off_diagonal_relation_predictions",
           "DYNOTEARS_Model", "fit_dynotears_baselines", "from_numpy_dynamic", "from_numpy_dynamic_many",
           "load_normalized_DREAM4_data_train_test_split_as_matrices",
           "load_normalized_DREAM4_data_train_test_split_as_tensors",
           "load_normalized_lfp_data_train_test_split_as_matrices"]
