/*
 * redcliff_hip.h -- C-ABI of libredcliff_hip.so, the MI355X (gfx950) implementation of the
 * REDCLIFF-S cMLP factor-model fitting hot path.
 *
 * The reference (carlson-lab/redcliff-s-hypothesizing-dynamic-causal-graphs) is pure
 * Python/PyTorch: it has no FFI of its own.  Each entry point below replaces one piece
 * of the reference's Python hot path (citations relative to the reference tree); the
 * Python host package binds them with ctypes.
 *
 * Conventions
 *  - All pointers are device pointers owned by the caller (PyTorch caching allocator).
 *    Nothing here allocates or frees device memory; scratch is a caller-supplied
 *    workspace of redcliff_workspace_bytes() bytes.
 *  - Every call is stream-ordered on the given hipStream_t (passed as void*) and does
 *    not synchronise the host.  Calls are stateless and re-entrant.
 *  - Return value: 0 on success, a negative argument-validation code, or a positive
 *    hipError_t.  redcliff_last_error() returns a thread-local message.
 *  - R "replicas" (independent fits with identical shapes, e.g. grid-search points)
 *    may be packed into one call; every per-replica buffer has an explicit stride.
 *    Training steps (redcliff_train_step), the cEmbedder chain and recording scoring
 *    (redcliff_score_recording_pack) all carry the replica on a grid axis.
 *  - fp32 throughout (the reference calls .float() on every model,
 *    general_utils/model_utils.py:392,417).
 */
#ifndef REDCLIFF_HIP_H
#define REDCLIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8: the workspace region y is laid out network-major, y[nU][K][p][Bmax] (was y[nU][Bmax][K][p])
 * 9: redcliff_factor_forward writes finished predictions y_out[r][B][K][p] (callers no longer decode
 *    the kernel-private workspace); redcliff_factor_forward_workspace_floats sizes its workspace;
 *    redcliff_step_predictions reads a step's predictions back the same way; RedcliffAdamHyper.t_offset
 *    (was padding) offsets a replica's Adam step number from the launch's
 * 10: the cEmbedder chain: redcliff_cemb_param_count / _workspace_bytes / _workspace_regions /
 *    _train_step / _train_steps and RedcliffCEmbArgs (existing entries and layouts unchanged) */
#define REDCLIFF_ABI_VERSION 10

/* error codes (negative) */
#define REDCLIFF_EINVAL (-1)  /* bad dimension / pointer                        */
#define REDCLIFF_ELIMIT (-2)  /* dimension outside what the kernels support     */
#define REDCLIFF_EWORKSPACE (-3)

/* step flags: which parts of one batch_update run (...withStateSmoothing.py:741-881) */
#define RC_BN_TRAIN      (1 << 0)  /* embedder BatchNorm in train mode (batch statistics)        */
#define RC_LOSS_FORECAST (1 << 1)  /* forecast MSE term (:629)                                   */
#define RC_LOSS_FACTOR   (1 << 2)  /* supervised factor-score MSE (:633-663)                     */
#define RC_LOSS_FWL1     (1 << 3)  /* factor-weight L1 (:666)                                    */
#define RC_LOSS_ADJ      (1 << 4)  /* lag-weighted adjacency L1 of conditional GC (:696-715)     */
#define RC_STEP_A        (1 << 5)  /* Adam step on the embedder (optimizerA)                     */
#define RC_STEP_B        (1 << 6)  /* Adam step on the factors  (optimizerB)                     */
#define RC_VALUES        (1 << 7)  /* compute loss values (validate_training, :1650-1790)        */
#define RC_CONFUSION     (1 << 8)  /* accumulate the factor-score confusion matrix (:786-803)    */
#define RC_STORE_OUTPUTS (1 << 9)  /* run the factor forward even without a loss (model.forward)  */
#define RC_REFRESH_SUPPORTS (1 << 10) /* recompute the DGCNN Chebyshev supports before the step  */
#define RC_GRAD_ONLY     (1 << 11) /* data-parallel shard: write the gradients of the RC_STEP_*
                                      groups to grad_emb / grad_fac instead of applying Adam
                                      (redcliff_adam_apply runs after the all-reduce)            */

/* Shapes shared by every call. */
typedef struct RedcliffDims {
  int32_t R;      /* replicas packed in one launch                                   */
  int32_t Bmax;   /* largest batch the workspace is sized for                         */
  int32_t T;      /* recorded time steps per window in the dataset buffer             */
  int32_t p;      /* channels (num_chans)                                            */
  int32_t L;      /* gen_lag: factor Conv1d kernel width                             */
  int32_t K;      /* num_factors                                                     */
  int32_t h;      /* factor hidden width (gen_hidden == [h])                          */
  int32_t F;      /* embed_lag == DGCNN num_features_per_node                        */
  int32_t n;      /* DGCNN Chebyshev layers                                          */
  int32_t H;      /* DGCNN hidden channels per node                                   */
  int32_t M1;     /* DGCNN fc1 width (64 in torcheeg)                                */
  int32_t nsup;   /* num_supervised_factors                                          */
  int32_t use_sigmoid;   /* use_sigmoid_restriction                                  */
  float sigmoid_ecc;     /* sigmoid_eccentricity_coeff                               */
} RedcliffDims;

/* torch.optim.Adam hyper-parameters of one parameter group.  Doubles are what torch's
 * Python side computes the bias corrections with; the fp32 copies are the scalars torch
 * applies element-wise (_single_tensor_adam / _multi_tensor_adam). */
typedef struct RedcliffAdamHyper {
  double lr, beta1, beta2;
  float eps, weight_decay;
  float beta2_f;            /* (float)beta2                                  */
  float one_minus_beta1_f;  /* (float)(1 - beta1): lerp weight               */
  float one_minus_beta2_f;  /* (float)(1 - beta2): addcmul value             */
  int32_t t_offset;         /* this replica's Adam step number minus the launch's tA / tB (packed
                               fits whose replicas stepped this group different numbers of times:
                               mixed phase schedules, ...withStateSmoothing.py:741-759); 0 otherwise */
} RedcliffAdamHyper;

/* Per-replica hyper-parameters, stored as a device array of R entries. */
typedef struct RedcliffReplicaHyper {
  float c_forecast, c_factor, c_cos, c_fwl1, c_smooth, c_adj; /* coeff_dict          */
  double bn_eps, bn_momentum;                                 /* BatchNorm1d         */
  RedcliffAdamHyper A;                                        /* optimizerA: embedder */
  RedcliffAdamHyper B;                                        /* optimizerB: factors  */
} RedcliffReplicaHyper;

/* Packed parameter layouts (floats, per replica):
 *  embedder (DGCNN): A[p][p] | gcW[n][F][H] | bn_w[F] | bn_b[F] | fc1W[M1][p*H] | fc1b[M1]
 *                    | fc2W[K][M1] | fc2b[K]
 *  factors:          W0[K][p][h][p][L] | b0[K][p][h] | W1[K][p][h] | b1[K][p]
 * (W0[k][j] is the Conv1d(p,h,L) weight of network j of factor k, models/cmlp.py:19.) */

typedef struct RedcliffStepArgs {
  RedcliffDims d;
  int32_t B;            /* windows in this batch (<= Bmax)                          */
  int32_t flags;        /* RC_* bitmask                                             */
  int32_t n_bn_updates; /* BatchNorm running-stat updates this step (3 in train phases) */
  int32_t tA, tB;       /* Adam step numbers (1-based) used for bias correction      */
  /* data: X[N][T][p] windows, labels[N][K] (already selected time index)            */
  const float* X; int64_t x_rstride; int64_t row0;
  const float* labels; int64_t lab_rstride;
  const double* bn_stats; int64_t bn_stats_rstride; /* [2][F] batch mean / biased var */
  /* parameters and Adam state                                                      */
  float* emb; float* emb_m; float* emb_v; int64_t emb_stride;
  float* fac; float* fac_m; float* fac_v; int64_t fac_stride;
  float* bn_rm; float* bn_rv;                      /* [R][F]                           */
  const RedcliffReplicaHyper* hyper;               /* device [R]                       */
  void* ws; size_t ws_bytes;                       /* workspace                        */
  double* acc;        /* [R][8] validation accumulators (may be NULL without RC_VALUES) */
  int32_t* confusion; /* [R][nsup][nsup] (may be NULL without RC_CONFUSION)              */
  /* data-parallel shards: this call processes B of the B_global windows of
   * the global batch.  Batch-mean terms (forecast MSE :629, factor MSE :638-661) and the
   * BatchNorm running-variance correction use B_global; batch sums (fw-L1, adj-L1) do not
   * scale, so the shard gradients of all ranks sum to the full-batch gradient.  bn_stats
   * must be the statistics of the GLOBAL batch.  B_global == 0 means B_global = B.       */
  int32_t B_global;
  int32_t pad_;
  float* grad_emb; float* grad_fac;  /* RC_GRAD_ONLY outputs, same layout/stride as emb / fac */
  /* Packed grid-search fits (train/REDCLIFF_S_CMLP_tst100hzRerun1024AvgReg_gsSmooth1.py:125-160,
   * one fit per grid point): the replicas this call steps, a strictly increasing HOST array of
   * n_replicas indices < R (at most 256).  A replica that stopped early (the per-fit rule of
   * ...withStateSmoothing.py:1483-1559) is left out: its parameters, Adam state, BatchNorm
   * statistics and accumulators are not touched and its workgroups are not launched.
   * NULL = all R replicas.  n_replicas == 0 launches nothing. */
  const int32_t* replicas; int32_t n_replicas;
  int32_t pad2_;
} RedcliffStepArgs;

int redcliff_abi_version(void);
const char* redcliff_last_error(void);
/* Source hash this library was compiled from: the first 16 hex digits of the SHA-256 over
 * the .hip / .h files of csrc/ and the .h files of include/ (path-sorted, name + contents) and the compile defines
 * (redcliff_amd/build.py source_hash).  Ties a pushed binary to the committed sources. */
const char* redcliff_build_id(void);

/* Workspace bytes for one launch of R replicas (all kernels share one layout). */
size_t redcliff_workspace_bytes(const RedcliffDims* d);
size_t redcliff_emb_param_count(const RedcliffDims* d);
size_t redcliff_fac_param_count(const RedcliffDims* d);

/* BatchNorm batch statistics of the embedder window X[row][Lmax-F:Lmax] for n_batches
 * consecutive batches of size B (last one may be ragged; N total windows).
 * stats[r][batch][2][F] (mean, biased variance).  Replaces the statistics half of
 * torch.nn.BatchNorm1d.forward in train mode (torcheeg DGCNN.BN1, models/dgcnn.py:37). */
int redcliff_bn_batch_stats(const RedcliffDims* d, const float* X, int64_t x_rstride, int64_t N, int32_t B,
                            double* stats, int64_t stats_rstride, void* stream);

/* normalize_A + Chebyshev supports [I, L, L^2, ...] of the DGCNN adjacency into the
 * workspace (torcheeg normalize_A / generate_cheby_adj).  Must run after any change
 * of the embedder parameters made outside redcliff_train_step. */
int redcliff_dgcnn_supports(const RedcliffDims* d, const float* emb, int64_t emb_stride, void* ws, void* stream);

/* One REDCLIFF-S batch_update (...withStateSmoothing.py:734-933) for the published
 * configuration: DGCNN embedder, conditional_factor_fixed_embedder GC, factor weights
 * applied after simulation, num_sims == 1.  With RC_VALUES and no RC_STEP_* it is the
 * per-batch body of validate_training.  Launches the fused kernel chain on `stream`. */
int redcliff_train_step(const RedcliffStepArgs* a, void* stream);

/* nsteps consecutive batch_updates of one epoch without returning to the host:
 * step i uses rows[i] / sizes[i] (host arrays) as row0 / B, bn_stats advanced by
 * i*bn_stats_step doubles, and Adam step numbers a->tA + i (a->tB + i) when the
 * corresponding RC_STEP_* flag is set.  RC_REFRESH_SUPPORTS applies to the first step. */
int redcliff_train_steps(const RedcliffStepArgs* a, int32_t nsteps, const int64_t* rows, const int32_t* sizes,
                         int32_t bn_stats_step, void* stream);
/* redcliff_train_steps / redcliff_cemb_train_steps of at least 4 steps evaluate the Adam bias
 * corrections of the call's steps once per chunk of steps (one small launch on `stream`) into a table at the end of every
 * replica's workspace slice, which the step kernels read instead of computing them per
 * workgroup; a direct redcliff_train_step computes them in the kernels.  Same device arithmetic,
 * same bits.  REDCLIFF_ADAM_TABLE=0 (read per call) switches the table off;
 * REDCLIFF_ADAM_TABLE_SMAX=n shortens the chunk (tests).  Additive: REDCLIFF_ABI_VERSION stays 10.
 * out[0] = the table's offset (floats) in a replica's slice, out[1] = steps per chunk in effect,
 * out[2] = floats per entry (neg_step bc2s eps wd b2 omb1 omb2 pad); entry (step i of the chunk,
 * group g: 0 = A, 1 = B) starts at out[0] + (2 i + g) * out[2]. */
int redcliff_adam_table_layout(const RedcliffDims* d, int64_t* out);

/* Offsets (floats, per replica) of the workspace regions: T R f1 w a y G G0 w1 dwp dAadj dWi dS
 * dgb S dZ amat lossp xsim gfc total.  Returns the number of offsets available.  The host reads
 * w (raw embedder output, [B][K]), xsim (mixed forecast, [B][p]) and G / G0 (group norms) back
 * from a step run with RC_STORE_OUTPUTS; the per-factor predictions through
 * redcliff_step_predictions (the y region itself is kernel-private partial sums). */
int redcliff_workspace_layout(const RedcliffDims* d, int64_t* out, int32_t n_out);

/* Per-factor predictions of the last RC_STORE_OUTPUTS step of the R replicas of workspace ws (sized
 * for d): y_out[r][b][k][j] (y_rstride floats between replicas), b < B.  The models' per-factor
 * outputs of forward (...withStateSmoothing.py:326-385). */
int redcliff_step_predictions(const RedcliffDims* d, int32_t B, const void* ws, float* y_out, int64_t y_rstride,
                              void* stream);

/* Device status of the R replica slices of a workspace (no reference counterpart: the
 * reference has no device code).  out[r] (host array of R u32) receives replica r's count of
 * merged-backward hand-off waits that ran out of polls since the last call (the consumer then
 * proceeded without its producers' records, so that step's results are invalid); the words are
 * cleared.  Synchronises `stream`.  Returns the number of replicas with a non-zero count (0 =
 * healthy) or a negative error code.  Callers check it where they already synchronise. */
int redcliff_device_status(const RedcliffDims* d, void* ws, uint32_t* out, void* stream);

/* Verification mode (tests only; no reference counterpart): with floats > 0 every workspace
 * region laid out afterwards is followed by a guard band of that many floats, the last band
 * also closing replica R-1's slice.  A test fills the bands with a NaN pattern; a write past
 * a region's end changes a band, a read past it puts NaN into the results.  0 = production
 * layout.  Returns the previous setting.  Process-wide: set it before sizing workspaces. */
int redcliff_debug_guard_bands(int32_t floats);
/* (start, size) pairs, in floats, of the regions of one replica's workspace slice in layout
 * order (out[2i], out[2i+1]); returns the region count. */
int redcliff_workspace_regions(const RedcliffDims* d, int64_t* out, int32_t n_pairs);

/* Stand-alone forward of K cMLPs (models/cmlp.py:90-101, MLP.forward :29-35) on B windows
 * Xwin[r][B][L][p] (x_rstride floats between the R = d->R replicas): y_out[r][b][k][j]
 * (y_rstride floats between replicas) receives the prediction of network j of factor k for
 * window b.  ws: scratch of redcliff_factor_forward_workspace_floats(d, B) floats per replica
 * (ws_rstride floats between replicas; its contents are private to the kernels). */
size_t redcliff_factor_forward_workspace_floats(const RedcliffDims* d, int32_t B);
int redcliff_factor_forward(const RedcliffDims* d, int32_t B, const float* Xwin, int64_t x_rstride, const float* fac,
                            int64_t fac_stride, float* ws, int64_t ws_rstride, float* y_out, int64_t y_rstride,
                            void* stream);

/* G[r][k][j][c][t] = ||W0[k][j][:, c, t]||_2, G0[r][k][j][c] = ||W0[k][j][:, c, :]||_F (models/cmlp.py:147-167) */
int redcliff_gc_norms(const RedcliffDims* d, const float* fac, int64_t fac_stride, float* G, float* G0, void* stream);
/* In-place proximal step on layer-0 weights, penalty 0=GL 1=GSGL 2=H (models/cmlp.py:117-144). */
int redcliff_prox(const RedcliffDims* d, float* fac, int64_t fac_stride, float lam, float lr, int32_t penalty,
                  void* stream);

/* Adam (torch.optim.Adam, coupled L2, general_utils/model_utils.py:747-762) of one
 * parameter group from a gradient buffer: group 0 = embedder (hyper[r].A), 1 = factors
 * (hyper[r].B); n floats per replica at `stride`; t = 1-based step number.  The
 * data-parallel step is  train_step(RC_GRAD_ONLY) -> all-reduce(grad) -> adam_apply. */
int redcliff_adam_apply(const RedcliffDims* d, float* params, float* exp_avg, float* exp_avg_sq, const float* grad,
                        int64_t n, int64_t stride, const RedcliffReplicaHyper* hyper, int32_t group, int32_t t,
                        void* stream);

/* The data-parallel update in one launch: with the step arguments of the RC_GRAD_ONLY shard step
 * that just ran (after grad_emb / grad_fac were all-reduced), Adam of the RC_STEP_A group
 * (n_emb floats) and the RC_STEP_B group (n_fac floats), exactly as redcliff_adam_apply with
 * t = tA / tB, plus the DGCNN Chebyshev supports of the updated A in the workspace, so the next
 * step needs no RC_REFRESH_SUPPORTS.  Replaces the optimizer steps of batch_update
 * (models/redcliff_s_cmlp_withStateSmoothing.py:741-759) for summed gradients. */
int redcliff_dp_update(const RedcliffStepArgs* a, int64_t n_emb, int64_t n_fac, void* stream);

/* Batched fp32 GEMM, row-major: C[b] = alpha * op(A[b]) op(B[b]) + beta * C[b], op = X or X^T
 * (trans flag), A/B/C of batch b at X + b * stride_x.  The contraction of the generic
 * (non-fused) path: cEmbedder / Vanilla embedders (models/redcliff_factor_score_embedders.py:
 * 51-331), num_sims > 1 roll-outs and the per-step weighting forward mode
 * (models/redcliff_s_cmlp_withStateSmoothing.py:253-323), composed on the host with autograd. */
int redcliff_gemm(int32_t trans_a, int32_t trans_b, int32_t M, int32_t N, int32_t K, float alpha, const float* A,
                  int64_t lda, int64_t stride_a, const float* B, int64_t ldb, int64_t stride_b, float beta, float* C,
                  int64_t ldc, int64_t stride_c, int32_t batch, void* stream);

/* Per-epoch GC-progress metrics of fit() for S samples x G graphs (replaces the host loops of
 * general_utils/model_utils.py:18-160 over general_utils/metrics.py:111-252, 396-430 and
 * sklearn's roc_auc_score).  One workgroup per (sample, graph), 2 <= p <= 64, Lt <= 128:
 *   est      float32 [S][nE][p][p][Lt]  GC estimates (the first G of each sample are scored)
 *   truth    float64 [2][G][p][p]       true graphs summed over lags and max-normalised,
 *                                       [0] as is, [1] with self-connections removed first
 *   eps_pow  float64 [p]                eps_pow[k] = deltaConEps ** k (host pow)
 *   out      float64 [S][G][6 + p]      f1, roc_auc, f1 (off-diagonal), roc_auc (off-diagonal),
 *                                       deltacon0, deltacon0 with directed degrees, deltaffinity,
 *                                       path-length MSE for k = 1 .. p-1
 * roc_auc is NaN where sklearn would raise (truth without negatives, NaN scores). */
int redcliff_gc_progress(int32_t S, int32_t nE, int32_t G, int32_t p, int32_t Lt, const float* est,
                         const double* truth, const double* eps_pow, double in_degree_coeff, double out_degree_coeff,
                         double* out, void* stream);
/* The same with one truth block per group of spt consecutive samples: sample s is scored against
 * truth[s / spt] ([S / spt][2][G][p][p]) -- a packed grid whose replicas fit different data sets
 * (train/REDCLIFF_S_CMLP_synSysInnovGauss1030_BSCgsSmooth3Parsim.py:66-72: one model over many
 * datasets, each with its own true graphs).  redcliff_gc_progress is spt = S. */
int redcliff_gc_progress_grouped(int32_t S, int32_t spt, int32_t nE, int32_t G, int32_t p, int32_t Lt,
                                 const float* est, const double* truth, const double* eps_pow, double in_degree_coeff,
                                 double out_degree_coeff, double* out, void* stream);

/* Per-epoch tracker statistics of fit() (replaces the host reductions of
 * general_utils/model_utils.py:163-188 (L1 tracker) and :191-209 (cosine tracker), which the
 * reference runs on float64 copies of every estimate):
 *   est      float32 [n_l1_rows][l1_len]     lagged estimates, one (sample, factor) per row
 *   l1_out   float64 [n_l1_rows]             sum |e / max(e)|
 *   nolag    float32 [n_samples][K][row_len] lag-free estimates
 *   dots_out float64 [n_samples][K][K]       upper triangle (i1 <= i2): sum (a / max a)(b / max b)
 *                                            over rows i1, i2 (the diagonal: squared norms)
 * One workgroup per row / pair, reductions in a fixed order independent of the launch size. */
int redcliff_gc_track_stats(int32_t n_l1_rows, int64_t l1_len, const float* est, double* l1_out, int32_t n_samples,
                            int32_t K, int64_t row_len, const float* nolag, double* dots_out, void* stream);

/* ---- cEmbedder chain (models/redcliff_factor_score_embedders.py:183-331) ----------------------
 * The embedder is K copies of models/cmlp.py:12-35 MLP (Conv1d(p, eh, F) -> ReLU -> Conv1d(eh, 1, 1)),
 * one per factor score, on the embedder window X[row][Lmax-F : Lmax].
 *
 * Packed cEmbedder parameter layout (floats, per replica):
 *   We0[K][eh][p][F] | be0[K][eh] | We1[K][eh] | be1[K]
 * (We0[k] is the Conv1d(p, eh, F) weight of network k: columns q = c*F + t, as the factors' W0.)
 *
 * Limits: p <= 64, K <= 16, h <= 128, eh <= 128, L <= F <= 64, Bmax <= 512, and the matrix-core
 * factor chain's LDS tiles at Bmax windows; outside them every entry below fails with
 * REDCLIFF_ELIMIT (the size queries return 0) and a redcliff_last_error message.  The n / H / M1
 * fields of RedcliffDims are ignored (pass 1, which keeps the shared workspace small). */
size_t redcliff_cemb_param_count(const RedcliffDims* d, int32_t eh);

/* Bytes of the second, cEmbedder-private workspace for d->R replicas: hidden activations
 * ha[K][Bmax][eh], the We1 snapshot, the embedder group norms g[K][p][F] / g0[K][p]
 * (models/redcliff_factor_score_embedders.py:297-326), the fixed embedder graph E[p][p][Ls] /
 * E0[p][p] (sum_k g_k g_k^T, ...withStateSmoothing.py:500-519), its per-factor gradient records
 * dE[K][p][p][Ls] and dL/dw_raw[Bmax][K].  Laid out with the shared workspace's region /
 * guard-band mechanism (redcliff_debug_guard_bands applies). */
size_t redcliff_cemb_workspace_bytes(const RedcliffDims* d, int32_t eh);
/* (start, size) pairs, in floats, of the regions of one replica's slice of that workspace in layout
 * order: ha w1 g g0 E E0 dE draw; when n_pairs allows, one more pair (slice size, 0).  Returns the
 * region count (8). */
int redcliff_cemb_workspace_regions(const RedcliffDims* d, int32_t eh, int64_t* out, int32_t n_pairs);

typedef struct RedcliffCEmbArgs {
  int32_t eh;            /* cEmbedder hidden width (hidden == [eh])                           */
  int32_t pad_;
  void* ws; size_t ws_bytes; /* the cEmbedder workspace (redcliff_cemb_workspace_bytes)        */
} RedcliffCEmbArgs;

/* One batch_update (...withStateSmoothing.py:734-933) of a model whose factor-score embedder is the
 * cEmbedder: conditional_factor_fixed_embedder GC (:500-519, :565-580), factor weights applied
 * after simulation (:326-385), num_sims == 1, the loss of :624-731.  RedcliffStepArgs as in
 * redcliff_train_step with emb / emb_m / emb_v / emb_stride the packed cEmbedder group; the bn_*
 * fields are ignored.  Flags and phases as redcliff_train_step (RC_BN_TRAIN is ignored: no
 * BatchNorm); RC_GRAD_ONLY and RC_REFRESH_SUPPORTS are rejected with REDCLIFF_EINVAL.  With
 * RC_VALUES and no RC_STEP_* it is the per-batch body of validate_training (:1650-1790).  R >= 1
 * replicas with strides and the `replicas` list as redcliff_train_step; one stream, no
 * cross-replica state, every reduction in a fixed order. */
int redcliff_cemb_train_step(const RedcliffStepArgs* a, const RedcliffCEmbArgs* e, void* stream);
/* nsteps consecutive batch_updates as redcliff_train_steps: step i uses rows[i] / sizes[i] and
 * Adam step numbers a->tA + i (a->tB + i) for the stepped groups. */
int redcliff_cemb_train_steps(const RedcliffStepArgs* a, const RedcliffCEmbArgs* e, int32_t nsteps,
                              const int64_t* rows, const int32_t* sizes, void* stream);

/* ---- scoring whole recordings (general_utils/misc.py:57-81, evaluate/eval_utils.py:953-1087) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no existing entry or layout changes.
 *
 * The DGCNN factor-score embedder in inference mode (BatchNorm running statistics) over sliding
 * windows of Nrec recordings X[r][T][p] (fp32, rows contiguous, x_rstride floats between
 * recordings): scored step j < count uses rows [start + j*stride - F, start + j*stride) as a
 * time-major window; the windows are never materialised.  Outputs, contiguous:
 *   w[r][j][K]         factor weightings (sigmoid(ecc * raw) under the sigmoid restriction, else raw)
 *   logits[r][j][nsup] class scores raw[:nsup] (sigmoid(raw) when the restriction is on and
 *                      use_final_activation != 0); may be NULL when nsup == 0
 *   graphs[r][j][Q]    optional graph trace bias[q] + sum_k w[r][j][k] tab[k][q] (k ascending) from
 *                      the caller's tab[K][Q] and bias[Q] (bias may be NULL): the conditional graph of
 *                      every scored step (...withStateSmoothing.py:481-498, :565-580) summed over factors
 * emb is the packed embedder block (layout above), bn_rm / bn_rv the running statistics [F]; the
 * call reads them only.  ws: redcliff_score_recording_workspace_bytes(d) bytes, private to the call
 * (supports and folded BatchNorm tables of the current parameters, rebuilt by every call).
 * Of RedcliffDims only p, K, F, n, H, M1, nsup, use_sigmoid and sigmoid_ecc are read.  Limits:
 * p <= 64, F <= 64, n <= 4, M1 <= 64, K <= 16, p*H, M1*H, F*H <= 8192 and n*p*(F + 15) + n*F*H + 1088
 * <= 40960 floats of LDS; outside them REDCLIFF_ELIMIT (the size query returns 0).  start < F,
 * stride < 1, count < 0, a last window that ends past T and null buffers give REDCLIFF_EINVAL;
 * count == 0 launches nothing.  Stream-ordered, no host synchronisation, no atomics: the same
 * arguments give the same bits, and a window's results do not depend on count, stride, Nrec or on
 * its position in the launch. */
typedef struct RedcliffScoreArgs {
  RedcliffDims d;
  const float* emb; const float* bn_rm; const float* bn_rv;
  double bn_eps;                         /* BatchNorm1d.eps                                   */
  const float* X; int64_t x_rstride;
  int32_t Nrec, T;
  int32_t start, count, stride;
  int32_t use_final_activation;
  float* w; float* logits;
  const float* tab; const float* bias; float* graphs;  /* graphs == NULL: no graph trace        */
  int32_t Q; int32_t pad_;
  void* ws; size_t ws_bytes;
} RedcliffScoreArgs;
size_t redcliff_score_recording_workspace_bytes(const RedcliffDims* d);
int redcliff_score_recording(const RedcliffScoreArgs* a, void* stream);

/* ---- scoring whole recordings with R same-shape models in one launch chain ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no existing entry or layout changes.
 *
 * redcliff_score_recording for R models of one shape d (grid-search points, cross-validation folds):
 * one supports launch, one table launch, one window-kernel launch on grid (tiles, Nrec, scored
 * replicas) and, with graphs, one graph launch.  Replica r reads
 *   emb + r*emb_stride                 its packed embedder block
 *   bn_rm + r*bn_stride, bn_rv + ...   its running statistics [F] (a [2][R][F] buffer: stride F)
 *   X + r*x_pstride                    its recording set [Nrec][T][p]; x_pstride == 0: all replicas score
 *                                      the same X
 *   tab + r*K*Q, bias + r*Q            its graph tables tab[R][K][Q] / bias[R][Q] (bias may be NULL)
 * replicas / n_replicas: the replicas to score, a strictly increasing HOST array of indices < R as
 * RedcliffStepArgs.replicas (NULL = all R; n_replicas == 0 launches nothing).  Outputs, contiguous,
 * i = the i-th scored replica in ascending order:
 *   w[i][rec][j][K]   logits[i][rec][j][nsup]   graphs[i][rec][j][Q]
 * ws: redcliff_score_recording_pack_workspace_bytes(d, R) bytes (R times the single call's), private
 * to the call.  A window's arithmetic and every order of sums are those of redcliff_score_recording:
 * its bits depend on the dims and the replica's own data only -- not on R, the replica's index, the
 * active list or whether X is shared -- so row i equals the single call on replica i's buffers bit
 * for bit.  Limits and return codes as redcliff_score_recording, plus: R < 1, a bad active list,
 * negative strides give REDCLIFF_EINVAL; R > 256 and Nrec > 65535 REDCLIFF_ELIMIT (the size query
 * returns 0); a short workspace REDCLIFF_EWORKSPACE.  All checks precede any HIP call. */
typedef struct RedcliffScorePackArgs {
  RedcliffDims d;                        /* d.R is not read                                   */
  int32_t R; int32_t pad0_;
  const float* emb; int64_t emb_stride;
  const float* bn_rm; const float* bn_rv; int64_t bn_stride;
  double bn_eps;                         /* BatchNorm1d.eps (shared by the replicas)          */
  const float* X; int64_t x_rstride; int64_t x_pstride;
  int32_t Nrec, T;
  int32_t start, count, stride;
  int32_t use_final_activation;
  float* w; float* logits;
  const float* tab; const float* bias; float* graphs;  /* graphs == NULL: no graph trace        */
  int32_t Q; int32_t n_replicas;
  const int32_t* replicas;
  void* ws; size_t ws_bytes;
} RedcliffScorePackArgs;
size_t redcliff_score_recording_pack_workspace_bytes(const RedcliffDims* d, int32_t R);
int redcliff_score_recording_pack(const RedcliffScorePackArgs* a, void* stream);

/* ---- scoring whole recordings of cEmbedder models (general_utils/misc.py:57-81 on the embedder of
 * models/redcliff_factor_score_embedders.py:183-273) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10.
 *
 * The cEmbedder (K networks Conv1d(p, eh, F) -> ReLU -> 1x1 Conv1d, hidden == [eh], no wavelets) over
 * the same sliding windows, with the same outputs w / logits / graphs, the same activations and the
 * same argument rules and return codes as redcliff_score_recording.  The window is read time-major at
 * every p (the cEmbedder has no p == F special case) and there is no BatchNorm:
 *   z[u]   = be0[k][u] + sum_q We0[k][u][q] X[t0 + f][c]      (q = c*F + f ascending)
 *   raw[k] = be1[k] + sum_u We1[k][u] relu(z[u])
 * emb is the packed cEmbedder block (layout above: We0 | be0 | We1 | be1); the call reads it only and
 * needs no workspace.  Of RedcliffDims only p, K, F, nsup, use_sigmoid and sigmoid_ecc are read.
 * Limits: p <= 64, F <= 64, K <= 16, eh <= 128 (p*(F + 63) + 4096 <= 40960 floats of LDS holds inside
 * them); outside them REDCLIFF_ELIMIT.  count == 0 launches nothing.  Stream-ordered, no host
 * synchronisation, no atomics: the same arguments give the same bits, and a window's results do not
 * depend on count, stride, Nrec or on its position in the launch. */
typedef struct RedcliffCEmbScoreArgs {
  RedcliffDims d;
  int32_t eh;            /* cEmbedder hidden width                                             */
  int32_t pad_;
  const float* emb;
  const float* X; int64_t x_rstride;
  int32_t Nrec, T;
  int32_t start, count, stride;
  int32_t use_final_activation;
  float* w; float* logits;
  const float* tab; const float* bias; float* graphs;  /* graphs == NULL: no graph trace        */
  int32_t Q; int32_t pad2_;
} RedcliffCEmbScoreArgs;
/* Host-only limit query: 0 outside the limits (with a redcliff_last_error message), else the number
 * of recording rows one tile can stage in LDS (a tile scores up to 64 steps, fewer when
 * (steps - 1)*stride + F would exceed this number, down to one). */
int redcliff_cemb_score_supported(const RedcliffDims* d, int32_t eh);
int redcliff_cemb_score_recording(const RedcliffCEmbScoreArgs* a, void* stream);

/* ---- the cMLP forecasting baseline cMLP_FM (models/cmlp_fm.py:96-201, 419-475) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no existing entry or layout changes.
 *
 * The model is one cMLP (K = 1) with no embedder; its loss is c_forecast * sum_i MSE(pred[:, :, i],
 * target[:, :, i]) + c_adj * sum ||GC(ignore_lag=True)||_1 (models/cmlp_fm.py:156-178), one Adam.
 * The loss separates over the p channel networks, so one launch on grid (p, stepped replicas) runs
 * nsteps = ceil(N / B) consecutive batch_updates (:180-201) of the windows X[row0 + i*B ...] (the
 * last batch may be ragged): workgroup (j, r) keeps network j's weights and Adam moments in LDS for
 * the whole call and writes them back once.  Window rows [0, L) are the input, row L the target
 * (num_sims == 1, output_length == 1, input_length == gen_lag, no wavelets).  Per step i:
 *   z[b][u] = b0[u] + sum_q W0[u][q] X[row+b][t][c]  (q = c*L + t ascending)   a = relu(z)
 *   y[b] = b1 + sum_u W1[u] a[b][u]      res[b] = y[b] - X[row+b][L][j]
 *   dy[b] = c_forecast * (2 / B_i) * res[b]                       (RC_LOSS_FORECAST)
 *   dW0[u][c][t] += c_adj * W0[u][c][t] / G0[c]                   (RC_LOSS_ADJ; 0 where G0[c] == 0)
 *   Adam of hyper[r].B at step number tB + i                      (RC_STEP_B)
 * Outputs: sse[i'][i][j] = sum_b res[b]^2 and, with RC_VALUES, pen[i'][i][j] = sum_c G0[c] at the
 * weights step i used (i' = the i'-th stepped replica in ascending order); when G / G0 are given,
 * G[r][j][c][t] / G0[r][j][c] of the final weights in redcliff_gc_norms' layout (indexed by replica).
 * Without RC_STEP_B the call is the batch body of validate_training (:419-475): parameters and
 * moments are only read.  Replica r reads X + r*x_pstride (0: all replicas fit the same set) and its
 * factor block at fac + r*fac_stride (layout above at K = 1; fac_m / fac_v alike).
 * Limits: K == 1, p <= 64, h <= 128, Bmax <= 512, T >= L + 1, R <= 256 and
 *   4*h*Qp + 3*(2h + 1) + 64*(Qp + hp + 2) + p*L + p + 8 <= 40960 floats of LDS  (Qp = p*L | 1, hp = h | 1);
 * outside them REDCLIFF_ELIMIT.  Null buffers, flags outside the four above, B < 1 or > Bmax, N < 0,
 * a bad active list, negative strides: REDCLIFF_EINVAL.  N == 0 or an empty list launches nothing.
 * All checks precede any HIP call.  Stream-ordered, no atomics, every sum in an order fixed by
 * (p, L, h) and the batch size: a replica's bits do not depend on R, the active list, or on how
 * [row0, row0 + N) is split into calls at multiples of B. */
typedef struct RedcliffFMArgs {
  RedcliffDims d;            /* R, Bmax, T, p, L, h read; K must be 1; the embedder fields are ignored */
  int32_t flags;             /* RC_LOSS_FORECAST | RC_LOSS_ADJ | RC_STEP_B | RC_VALUES             */
  int32_t B, tB;             /* batch size; Adam step number of the first step (1-based)            */
  int64_t row0, N;           /* windows [row0, row0 + N) in batches of B                             */
  const float* X; int64_t x_pstride;
  float* fac; float* fac_m; float* fac_v; int64_t fac_stride;
  const RedcliffReplicaHyper* hyper;        /* device [R]: c_forecast, c_adj, B (Adam) read          */
  float* sse; float* pen;    /* [n stepped][nsteps][p]; pen may be NULL without RC_VALUES            */
  float* G; float* G0;       /* optional final norms [R][p][p][L] / [R][p][p], may be NULL           */
  const int32_t* replicas; int32_t n_replicas;   /* as RedcliffStepArgs.replicas                    */
} RedcliffFMArgs;
/* Host-only limit query: 0 outside the limits (with a redcliff_last_error message), else the
 * workgroup's LDS footprint in floats. */
int redcliff_fm_supported(const RedcliffDims* d);
int redcliff_fm_run(const RedcliffFMArgs* a, void* stream);

/* ---- the cLSTM forecasting baseline cLSTM_FM (models/clstm_fm.py:56-177, 341-393) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout
 * changes.
 *
 * The model is one cLSTM (models/clstm.py: p networks nn.LSTM(p, h) -> Conv1d(h, 1, 1)) with no
 * embedder; its loss is c_forecast * sum_i MSE(pred[:, :, i], target[:, :, i]) + c_adj * sum_j sum_c
 * ||weight_ih_j[:, c]||_2, one Adam.  The loss separates over the p networks, so one launch on grid
 * (p, stepped replicas) runs nsteps = ceil(N / B) consecutive batch_updates (:141-177) of the
 * recordings X[row0 + i*B ...] (the last batch may be ragged): workgroup (j, r) keeps network j's
 * weights and Adam moments in LDS for the whole call and writes them back once.
 * With C = context, S = tmax - C sequences per recording, Bq = B_i * S, sequence (n, s) reads rows
 * s .. s+C of recording n in place (arrange_input, :95-112, is never materialised).  Per step i:
 *   t = 0..C-1:  a = Wih x[n][s+t] + Whh h_{t-1} + (bih + bhh)   (gate rows i | f | g | o, h_{-1} = c_{-1} = 0)
 *                c_t = sig(a_f) c_{t-1} + sig(a_i) tanh(a_g)     h_t = sig(a_o) tanh(c_t)
 *                y_t = Wl . h_t + bl                             res = y_t - x[n][s+t+1][j]
 *   dy = c_forecast * 2 / (Bq * C) * res                          (RC_LOSS_FORECAST)
 *   backward through time into dWih, dWhh, dbih = dbhh, dWl, dbl
 *   dWih[:, c] += c_adj * Wih[:, c] / G[c], G[c] = ||Wih[:, c]||_2  (RC_LOSS_ADJ; 0 where G[c] == 0)
 *   Adam of hyper[r].B at step number tB + i on each of the six tensors   (RC_STEP_B)
 * Packed layout of a replica's block (fac, fac_m, fac_v alike), each torch parameter a contiguous view:
 *   Wih[p][4h][p] | Whh[p][4h][h] | bih[p][4h] | bhh[p][4h] | Wl[p][h] | bl[p]
 * Outputs: sse[i'][i][j] = sum res^2 over the batch's Bq * C residuals and, with RC_VALUES,
 * pen[i'][i][j] = sum_c G[c] at the weights step i used (i' = the i'-th stepped replica in ascending
 * order); when G is given, G[r][j][c] of the final weights (indexed by replica).
 * Without RC_STEP_B the call is the batch body of training_sim_eval (:341-393): the parameters are
 * only read, the moments are not touched (fac_m / fac_v may be NULL).
 * X[N][T][p] is device-resident; only rows [0, tmax) of a recording are read.  Replica r reads
 * X + r*x_pstride (0: all replicas fit the same set) and its block at fac + r*fac_stride.
 * Limits: p <= 64, h <= 64, context <= 64, Bmax <= 512, R <= 256 and
 *   4*(4h*Kp + 9h + 1) + 32*(((C+1)K | 1) + (4hC | 1) + (hC | 1) + 2(h | 1) + 2C) + p + 16 <= 40960
 * floats of LDS (K = p + h, Kp = K | 1), which binds first: h <= 35 at p = 4, C = 2; h <= 33 at p = 10,
 * C = 2; h <= 18 at p = 64, C = 2; p <= 35 at h = 25, C = 2; context <= 34 at p = 4, h = 5; context <= 4
 * at p = 10, h = 25.  Outside them REDCLIFF_ELIMIT.  Null buffers, flags outside the four above,
 * B < 1 or > Bmax, N < 0, tmax <= context, tmax > T, a bad active list, negative strides:
 * REDCLIFF_EINVAL.  N == 0 or an empty list launches nothing.  All checks precede any HIP call.
 * Stream-ordered, no atomics, every sum in an order fixed by (p, h, context, tmax) and the batch size:
 * a replica's bits do not depend on R, the active list, or on how [row0, row0 + N) is split into
 * calls at multiples of B. */
typedef struct RedcliffLstmFMArgs {
  RedcliffDims d;            /* R, Bmax, T, p, h read; every other field is ignored                   */
  int32_t context, tmax;     /* sequence length C; rows [0, tmax) of a recording are used             */
  int32_t flags;             /* RC_LOSS_FORECAST | RC_LOSS_ADJ | RC_STEP_B | RC_VALUES                */
  int32_t B, tB;             /* recordings per batch; Adam step number of the first step (1-based)    */
  int64_t row0, N;           /* recordings [row0, row0 + N) in batches of B                           */
  const float* X; int64_t x_pstride;
  float* fac; float* fac_m; float* fac_v; int64_t fac_stride;
  const RedcliffReplicaHyper* hyper;        /* device [R]: c_forecast, c_adj, B (Adam) read            */
  float* sse; float* pen;    /* [n stepped][nsteps][p]; pen may be NULL without RC_VALUES              */
  float* G;                  /* optional final norms [R][p][p], may be NULL                            */
  const int32_t* replicas; int32_t n_replicas;   /* as RedcliffStepArgs.replicas                      */
} RedcliffLstmFMArgs;
/* Host-only limit query: 0 outside the limits (with a redcliff_last_error message), else the
 * workgroup's LDS footprint in floats. */
int redcliff_lstm_fm_supported(const RedcliffDims* d, int32_t context);
int redcliff_lstm_fm_run(const RedcliffLstmFMArgs* a, void* stream);

/* ---- the NAVAR (MLP) additive baseline (models/navar.py:9-125) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout
 * changes.
 *
 * N per-source networks (K lags of series i -> H units -> (H units) -> N contributions) whose
 * contributions are summed into one prediction before the loss, so the networks are NOT independent.
 * RedcliffDims carries the shape: p = N (nodes), h = H (num_hidden), L = K (maxlags), n = hidden
 * layers (1 or 2), Bmax, T >= K + 1 (rows [0, K) of a window are the lags, row K the target), R.
 * Packed layout of a replica's block (par, par_m, par_v alike), each torch parameter a contiguous view:
 *   W1[N][H][K] | b1[N][H] | (W2[N][H][H] | b2[N][H] with two layers) | Wc[N][N][H] | bc[N][N] | biases[N]
 * Arithmetic of one step over the Bi windows X[perm[q]], q in [s*B, s*B + Bi):
 *   z1 = W1_i x_i + b1_i, h1 = max(z1, 0); (z2 = W2_i h1 + b2_i, h2 = max(z2, 0)); c_ij = Wc_i[j] . h + bc_ij
 *   pred_j = sum_i c_ij (i ascending) + biases_j;  res = pred - y;  mse = sum res^2 / (Bi N)
 *   dc_ij = 2 res_j / (Bi N) + lambda1 / (N Bi) sign(c_ij) (sign(0) = 0); clamp passes the gradient where z >= 0
 *   Adam of hyper[r].B at step number tB + s (coupled weight decay); lambda1 = hyper[r].c_adj
 * REDCLIFF_NAVAR_TRAIN: nsteps = ceil(N / B) steps, three launches each on the one stream (forward
 * partials per (unit slice, source), backward + update of the last layer / contributions, update of the
 * first layer and biases); launch boundaries are the only cross-workgroup dependencies, no atomics, no
 * grid barrier.  Outputs mse[i'][s] and l1[i'][s] = (lambda1 / N) mean_b sum_ij |c_ij| (i' = the i'-th
 * stepped replica in ascending order).  perm values are clamped into [0, nX).
 * REDCLIFF_NAVAR_FORWARD: rows [row0, row0 + N) of X in order -> pred[i'][N][N nodes],
 * contrib[i'][N][N*N] (channel i*N + j); parameters are only read, par_m / par_v / hyper / perm unused.
 * Replica r reads X + r*x_pstride (0: shared), perm + r*perm_pstride (0: shared), its block at
 * par + r*par_stride.  ws: n_stepped * (N*nS*B*N + [two] N*nS*B*H + 32) floats, nS = ceil(H / 32);
 * shorter gives REDCLIFF_EWORKSPACE.
 * Limits: N <= 32, H <= 512, K <= 64, Bmax <= 512, R <= 256, layers 1 or 2, T >= K + 1 and
 *   64*(K|1) + 4224 + 66*N + 128*(N|1) + 240 + (two ? 128*(ceil16(H)|1) : 32*(K|1)) <= 40960 floats of LDS
 * (two layers: H <= 256 at N = 10, K = 20); outside them REDCLIFF_ELIMIT (the query returns 0).  Null
 * buffers, a bad mode, B < 1 or > Bmax, N < 0, row0 + N > nX in FORWARD, a bad active list, negative
 * strides: REDCLIFF_EINVAL.  N == 0 or an empty list launches nothing.  All checks precede any HIP
 * call.  Every sum's order is fixed by the shape and the batch size: a replica's bits do not depend on
 * R, the active list, or on how the steps are split into calls at multiples of B. */
#define REDCLIFF_NAVAR_TRAIN 0
#define REDCLIFF_NAVAR_FORWARD 1
typedef struct RedcliffNavarArgs {
  RedcliffDims d;            /* R, Bmax, T, p = N, h = H, L = K, n = hidden layers read               */
  int32_t mode;              /* REDCLIFF_NAVAR_TRAIN | REDCLIFF_NAVAR_FORWARD                         */
  int32_t B, tB;             /* batch size; Adam step number of the first step (1-based)              */
  int32_t launches;          /* TRAIN, for profiling: 0 = all three launches of a step, else a mask of      */
                             /* 1 = k_navar_fwd, 2 = k_navar_bwd, 4 = k_navar_in (the others are skipped)    */
  int64_t row0, N;           /* FORWARD: rows [row0, row0 + N); TRAIN: perm[0 .. N), row0 ignored      */
  int64_t nX;                /* rows of one window set                                                */
  const float* X; int64_t x_pstride;
  const int32_t* perm; int64_t perm_pstride;
  float* par; float* par_m; float* par_v; int64_t par_stride;
  const RedcliffReplicaHyper* hyper;        /* device [R]: c_adj = lambda1, B (Adam) read             */
  float* mse; float* l1;     /* TRAIN: [n stepped][nsteps]                                            */
  float* pred; float* contrib;              /* FORWARD: [n stepped][N][N nodes] / [n stepped][N][N*N]  */
  float* ws; size_t ws_bytes;
  const int32_t* replicas; int32_t n_replicas;   /* as RedcliffStepArgs.replicas                     */
} RedcliffNavarArgs;
/* Host-only limit query: 0 outside the limits (with a redcliff_last_error message), else the
 * workgroup's LDS footprint in floats. */
int redcliff_navar_supported(const RedcliffDims* d);
int redcliff_navar_run(const RedcliffNavarArgs* a, void* stream);

/* ---- the NAVAR (LSTM) additive baseline (models/navar.py:129-246, model type "NAVAR_CLSTM") ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout
 * changes.
 *
 * N per-source one-layer LSTMs (input size 1, H units) over the T' = T - 1 first rows of a window, each
 * followed by a Linear(H, N) applied at every time step; the N x N contributions are summed over the
 * sources into one prediction per time step.  RedcliffDims carries p = N, h = H, T = window rows
 * (T' = T - 1 LSTM steps, row T' the target), Bmax and R; the other fields are not read.
 * Packed layout of a replica's block (par, par_m, par_v alike), each torch parameter a contiguous view,
 * gate order i, f, g, o:
 *   Wih[N][4H] | Whh[N][4H][H] | bih[N][4H] | bhh[N][4H] | Wfc[N][N][H] | bfc[N][N] | biases[N]
 * Arithmetic of one step over the Bi windows X[perm[q]], q in [s*B, s*B + Bi):
 *   pre_t = Whh_i h_{t-1} (k ascending, fp32 matrix cores) + (Wih_i x_t + (bih_i + bhh_i)), h_{-1} = c_{-1} = 0
 *   c_t = f c_{t-1} + i g, h_t = o tanh(c_t);  con_ij(t) = Wfc_i[j] . h_t (units ascending, from bfc_ij)
 *   pred_j(t) = sum_i con_ij(t) (i ascending) + biases_j;  res_j = pred_j(T'-1) - X[row][T'][j]
 *   mse = sum res^2 / (Bi N);  l1 = (lambda1 / N) sum_{t,b,ij} |con| / (Bi T')
 *   dcon_ij(t) = [t = T'-1] 2 res_j / (Bi N) + lambda1 / (N Bi T') sign(con_ij(t)) (sign(0) = 0); with
 *   lambda1 == 0 only t = T'-1 is formed (the other terms are exact zeros)
 *   Adam of hyper[r].B at step number tB + s (coupled weight decay); lambda1 = hyper[r].c_adj
 * REDCLIFF_NAVAR_TRAIN: nsteps = ceil(N / B) steps of 2T' + 5 launches each on the one stream: T' forward
 * launches over (16-unit slice, source, replica), the output layer, the loss / small-gradient
 * reduction, T' backward launches (t descending, same grid), the dWhh product (one GEMM per source,
 * k = (t, b) ascending) and the element-wise Adam.  Launch boundaries are the only cross-workgroup
 * dependencies: no atomics, no grid barrier, no workgroup waits on another.  Outputs mse[i'][s] and
 * l1[i'][s] (i' = the i'-th stepped replica in ascending order).  perm values are clamped into [0, nX).
 * REDCLIFF_NAVAR_FORWARD: rows [row0, row0 + N) of X in order -> pred[i'][N][N nodes][T'],
 * contrib[i'][N * T'][N*N] (row b*T' + t, channel i*N + j); parameters are only read.
 * ws: n_stepped * rc_navar_lstm_ws floats (redcliff_navar_lstm_ws_floats); shorter gives
 * REDCLIFF_EWORKSPACE.
 * Limits: N <= 32, H <= 448, T' in [1, 64], Bmax <= 512, R <= 256 and
 *   64*(ceil16(H)|1) + 64*65 + 64*(N|1) + 64*17 + 34*N + 384 <= 40960 floats of LDS
 * (true everywhere inside the other limits); outside them REDCLIFF_ELIMIT (the query returns 0).
 * Argument errors as redcliff_navar_run.  All checks precede any HIP call.  Every sum's order is fixed by
 * (N, H, T', batch size): a replica's bits do not depend on R, the active list, or on how the steps are
 * split into calls at multiples of B. */
typedef struct RedcliffNavarLstmArgs {
  RedcliffDims d;            /* R, Bmax, T, p = N, h = H read                                         */
  int32_t mode;              /* REDCLIFF_NAVAR_TRAIN | REDCLIFF_NAVAR_FORWARD                         */
  int32_t B, tB;             /* batch size; Adam step number of the first step (1-based)              */
  int32_t launches;          /* TRAIN, for profiling: 0 = all launches of a step, else a mask of       */
                             /* 1 = forward, 2 = output + reduction, 4 = backward, 8 = dWhh + Adam     */
  int64_t row0, N;           /* FORWARD: rows [row0, row0 + N); TRAIN: perm[0 .. N), row0 ignored      */
  int64_t nX;                /* rows of one window set                                                */
  const float* X; int64_t x_pstride;
  const int32_t* perm; int64_t perm_pstride;
  float* par; float* par_m; float* par_v; int64_t par_stride;
  const RedcliffReplicaHyper* hyper;        /* device [R]: c_adj = lambda1, B (Adam) read             */
  float* mse; float* l1;     /* TRAIN: [n stepped][nsteps]                                            */
  float* pred; float* contrib;              /* FORWARD: [n stepped][N][N nodes][T'] / [..][N*T'][N*N]  */
  float* ws; size_t ws_bytes;
  const int32_t* replicas; int32_t n_replicas;   /* as RedcliffStepArgs.replicas                     */
} RedcliffNavarLstmArgs;
/* Host-only limit query: 0 outside the limits (with a redcliff_last_error message), else the
 * backward workgroup's LDS footprint in floats. */
int redcliff_navar_lstm_supported(const RedcliffDims* d);
/* Workspace floats of one stepped replica at batch size B (train: 1 = TRAIN, 0 = FORWARD). */
int64_t redcliff_navar_lstm_ws_floats(const RedcliffDims* d, int32_t B, int32_t train);
int redcliff_navar_lstm_run(const RedcliffNavarLstmArgs* a, void* stream);

/* ---- the supervised DGCNN baseline as a stand-alone fit (models/dgcnn.py:63-237, model type "DGCNN") ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout
 * changes.
 *
 * RedcliffDims carries the shape: p = nodes n, F = features per node, n = Chebyshev layers, H = hidden
 * channels, K = classes C, Bmax, T >= F (rows [0, F) of a window X[row][T][n] are the features), R; M1 is
 * taken as 64.  Packed layout of a replica's block (par, par_m, par_v alike), the embedder's, each torch
 * parameter a contiguous view:
 *   A[n][n] | gcW[layers][F][H] | bn_w[F] | bn_b[F] | fc1W[64][n*H] | fc1b[64] | fc2W[C][64] | fc2b[C]
 * bn_rm / bn_rv: [R][F] running statistics.  Y: [nX][C] labels, already selected.
 * Arithmetic of one step over the Bi rows [row0 + s*B, row0 + s*B + Bi):
 *   x_b[k][f] = X[row][f][k];  BatchNorm over the Bi*n values of feature f (batch statistics in double, the
 *   biased variance normalises, the unbiased one goes to the running variance with hyper[r].bn_momentum)
 *   L = (dinv_i relu(A)_ik) dinv_k, dinv_i = 1 / sqrt(sum_k relu(A)_ik + 1e-10);  S_0 = I, S_1 = L, S_i = S_{i-1} L
 *   Z_b = sum_i (S_i x_b) W_i (supports ascending), R = relu(Z), f1 = fc1 flat(R) (nodes ascending) + fc1b,
 *   out = fc2 relu(f1) + fc2b, loss = sum (out - y)^2 / (Bi C);  ReLU passes no gradient at 0
 *   Adam of hyper[r].B at step number tB + s (coupled weight decay) on every parameter; with one layer A has
 *   no gradient and is left untouched together with its moments (torch's Adam skips a parameter without one)
 * REDCLIFF_DGCNN_FIT_TRAIN: one statistics launch for the call, then nsteps = ceil(N / B) steps of three
 * launches each on the one stream (per-node forward partials; head + per-node backward + Adam on the node's
 * fc1 block; the sums over nodes, dA and Adam on the rest, running statistics).  Launch boundaries are the
 * only cross-workgroup dependencies: no atomics, no grid barrier, no workgroup waits on another.  Output
 * loss[i'][s] (i' = the i'-th stepped replica in ascending order).  num_batches_tracked is the caller's.
 * REDCLIFF_DGCNN_FIT_FORWARD: eval mode (running statistics) over rows [row0, row0 + N) in batches of B ->
 * pred[i'][N][C] and, when Y is given, loss[i'][s] = the MSE of batch s; parameters are only read, par_m /
 * par_v unused.
 * Replica r reads X + r*x_pstride (0: shared), Y + r*y_pstride (0: shared), its block at par + r*par_stride.
 * ws: n_stepped * redcliff_dgcnn_fit_ws_floats(d, B, N) floats, 8-byte aligned; shorter gives
 * REDCLIFF_EWORKSPACE.
 * Limits: nodes <= 32, F <= 8, layers <= 4, hid <= 256, classes <= 16, Bmax <= 128, R <= 256, T >= F and
 *   max(256 + Bmax*(65 + C) + 64*C + 96*(hid|1) + 32*F*n + 96*layers*F + n*n + layers*n + layers*F*(hid|1),
 *       256 + (2*layers + 3)*n*n) <= 40960 floats of LDS
 * outside them REDCLIFF_ELIMIT (the queries return 0).  Null buffers, a bad mode, B < 1 or > Bmax, N < 0,
 * row0 < 0, row0 + N > nX, a bad active list, negative strides: REDCLIFF_EINVAL.  N == 0 or an empty list
 * launches nothing.  All checks precede any HIP call.  Every sum's order is fixed by the shape and the
 * batch size: a replica's bits do not depend on R, the active list, on whether data is shared, or on how the
 * steps are split into calls at multiples of B. */
#define REDCLIFF_DGCNN_FIT_TRAIN 0
#define REDCLIFF_DGCNN_FIT_FORWARD 1
typedef struct RedcliffDgcnnFitArgs {
  RedcliffDims d;            /* R, Bmax, T, p = nodes, F, n = layers, H = hid, K = classes read          */
  int32_t mode;              /* REDCLIFF_DGCNN_FIT_TRAIN | REDCLIFF_DGCNN_FIT_FORWARD                    */
  int32_t B, tB;             /* batch size; Adam step number of the first step (1-based)                 */
  int32_t launches;          /* TRAIN, for profiling: 0 = all three launches of a step, else a mask of    */
                             /* 1 = k_dg_fwd, 2 = k_dg_bwd, 4 = k_dg_tail (the others are skipped)        */
  int64_t row0, N;           /* rows [row0, row0 + N) of X / Y                                           */
  int64_t nX;                /* rows of one window set                                                   */
  const float* X; int64_t x_pstride;
  const float* Y; int64_t y_pstride;        /* FORWARD: may be NULL (no loss)                            */
  float* par; float* par_m; float* par_v; int64_t par_stride;
  float* bn_rm; float* bn_rv;               /* [R][F]                                                    */
  const RedcliffReplicaHyper* hyper;        /* device [R]: bn_eps, bn_momentum, B (Adam) read            */
  float* loss;               /* [n stepped][nsteps]                                                      */
  float* pred;               /* FORWARD: [n stepped][N][C]                                               */
  float* ws; size_t ws_bytes;
  const int32_t* replicas; int32_t n_replicas;   /* as RedcliffStepArgs.replicas                        */
} RedcliffDgcnnFitArgs;
/* Host-only limit query: 0 outside the limits (with a redcliff_last_error message), else the
 * workgroup's LDS footprint in floats. */
int redcliff_dgcnn_fit_supported(const RedcliffDims* d);
/* Workspace floats of one stepped replica for a call over N rows at batch size B (0: outside the limits). */
int64_t redcliff_dgcnn_fit_ws_floats(const RedcliffDims* d, int32_t B, int64_t N);
int redcliff_dgcnn_fit_run(const RedcliffDgcnnFitArgs* a, void* stream);

/* The supervised dCSFA-NMF baseline (models/dcsfa_nmf.py: deep encoder, MSE reconstruction, "Residual"
 * supervised reconstruction, one intercept, no correlation constraints) as a stand-alone fit: one call
 * enqueues every AdamW step of an epoch (additive to ABI 10).
 * Each of the R models owns a packed block at par + r*par_stride (par_m / par_v: AdamW's exp_avg /
 * exp_avg_sq in the same layout):
 *   W_nmf[K][D] | W1[H][D] | b1[H] | bn_w[H] | bn_b[H] | W2[K][H] | b2[K] | phi[ns] | beta[ns]
 * bn_rm / bn_rv: [R][H] running statistics.  X [N][D], Y [N][ns], TM [N][ns] (the task mask as floats),
 * PW [N] (the prediction weights); replica r reads them at + r*stride (0: shared).
 * Arithmetic of one step over the Bi rows idx[s*B .. s*B + Bi) (indices outside [0, N) are clamped):
 *   z = x W1^T + b1 (summed in double, rounded once); BatchNorm over the batch (statistics in double, the biased variance normalises, the
 *   unbiased one goes to the running variance with bn_momentum); a = LeakyReLU(0.01); pre = a W2^T + b2
 *   (slices of 8 hidden units ascending, then b2); s = softplus(pre) (threshold 20); Wp = softplus(W_nmf);
 *   mse = sum (s Wp - x)^2 / (Bi D);  s_h = ((x - s_un Wp_un) Wp_sup^T) inv(Wp_sup Wp_sup^T);
 *   res = ||s_sup - s_h||_F / (1 - c exp(-||s_h||_F)), both norms over the whole batch;
 *   y_pred = sigmoid(s_j phi_j + beta_j); bce = mean of -PW (t log p + (1 - t) log(1 - p)), p = y_pred TM,
 *   t = Y TM, the logs clamped at -100.
 *   loss[r][s][0] = recon_weight mse + sup_recon_weight res;  loss[r][s][1] = sup_weight bce.
 * REDCLIFF_DCSFA_TRAIN differentiates their sum and applies torch.optim.AdamW (decoupled decay) at step
 * number tB + s to every parameter.  REDCLIFF_DCSFA_PRETRAIN differentiates loss[..][0] only and leaves
 * W_nmf, phi, beta and their moments untouched (they have no gradient: no decay, no state).  Both: three
 * launches per step on the one stream (per-slice forward; head; per-slice backward); launch boundaries are
 * the only cross-workgroup dependencies.  num_batches_tracked is the caller's.
 * REDCLIFF_DCSFA_EVAL: eval mode (running statistics) over rows [row0, row0 + n) in batches of B; batch s
 * writes ev[r][s][0] = its sum of squared reconstruction errors and ev[r][s][1 + 4j ..] = TP, FP, TN, FN of
 * supervised network j over the rows with TM == 1 (label Y >= 0.6, prediction y_pred >= 0.6).
 * ws: R * redcliff_dcsfa_ws_floats(H, K, B) floats, 8-byte aligned.
 * Limits: K <= 8, 1 <= ns <= K, Bmax <= 128, R <= 256, D, H <= 4096 and
 *   max(128 + 9 Bmax + 40 (D|1), 128 + Bmax + 7 Bmax K + 4 K K + K (D|1)) <= 40960 floats of LDS;
 * outside them REDCLIFF_ELIMIT (the query returns 0).  A last batch of one row (no batch statistics), null
 * buffers, a bad mode, B < 1 or > Bmax, negative strides: REDCLIFF_EINVAL.  All checks precede any HIP call.
 * Every sum's order is fixed by the shape and the batch size: a replica's bits do not depend on R. */
#define REDCLIFF_DCSFA_TRAIN 0
#define REDCLIFF_DCSFA_PRETRAIN 1
#define REDCLIFF_DCSFA_EVAL 2
typedef struct RedcliffDcsfaArgs {
  int32_t D, H, K, ns, R, Bmax;
  int32_t mode, B, tB, pad_;     /* tB: AdamW step number of the first step (1-based)                     */
  int64_t N;                     /* rows of one data set                                                  */
  int64_t n;                     /* TRAIN / PRETRAIN: drawn rows of the epoch; EVAL: rows from row0       */
  int64_t row0;                  /* EVAL only (0 otherwise)                                               */
  const float* X; int64_t x_pstride;
  const float* Y; const float* TM; int64_t y_pstride;
  const float* PW; int64_t pw_pstride;
  const int32_t* idx; int64_t idx_pstride;   /* [R][n] the epoch's drawn rows (EVAL: unused)              */
  float* par; float* par_m; float* par_v; int64_t par_stride;
  float* bn_rm; float* bn_rv;                /* [R][H]                                                    */
  double lr, weight_decay, beta1, beta2, eps, bn_eps, bn_momentum;
  float recon_weight, sup_weight, sup_recon_weight, sup_smoothness_weight;
  float* loss;                   /* TRAIN / PRETRAIN: [R][nsteps][2]                                      */
  double* ev;                    /* EVAL: [R][nbatches][1 + 4 ns]                                         */
  float* ws; size_t ws_bytes;
} RedcliffDcsfaArgs;
/* Host-only limit query: 0 outside the limits (with a redcliff_last_error message), else the workgroup's
 * LDS footprint in floats. */
int redcliff_dcsfa_supported(int32_t D, int32_t H, int32_t K, int32_t ns, int32_t Bmax, int32_t R);
int64_t redcliff_dcsfa_ws_floats(int32_t H, int32_t K, int32_t B);
int redcliff_dcsfa_run(const RedcliffDcsfaArgs* a, void* stream);

/* ---- directed-spectrum features (general_utils/directed_spectrum.py, pairwise, and
 * general_utils/time_series.py make_high_level_signal_features) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout changes.
 *
 * For each of N windows X[n][T][p] (float32 or float64; x_wstride elements between windows, x_tstride between
 * time steps, channels contiguous) the features the reference's data sets build one window at a time:
 *   Welch spectra of the nseg = (T - noverlap) / (nperseg - noverlap) segments (detrend "constant", periodic
 *   Hann window, two-sided DFT of length F = nperseg, density scaling 1 / (fs sum w^2)), in double;
 *   per channel pair a < b the 2x2 CPSD [[c_aa, c_ab], [c_ba, c_bb]], c_ab = mean_s conj(X_b) X_a, rounded once
 *   to complex64 for float32 input;
 *   the singular branch: taken by rule when nseg < 2, else when the closed-form condition number of the
 *   Hermitian 2x2 (ratio of its singular values, in the input's precision) exceeds 1 / eps at any frequency of
 *   the pair; it adds spacing(max |c|) * 100 of THAT pair and window to the diagonal and continues in double;
 *   the Wilson factorisation (at most max_iter iterations, the reference's two-stage relative-change test with
 *   tol), H = psi A0^-1, Sigma = A0 A0^T, ds[a][b] = |H_ba|^2 (S_aa - S_ab^2 / S_bb), ds[b][a] likewise;
 *   the one-sided fold (bins 1 .. F/2 - 1 doubled, the Nyquist bin only for odd F), times the bin frequency
 *   k / (F (1 / fs)), cropped to the bins [i1, i2) = searchsorted(f, [min_freq, max_freq]); n_f = i2 - i1.
 * out row n (float32, out_rstride floats between rows, only the row's own columns are written):
 *   REDCLIFF_DIRSPEC_VANILLA    [p][p][n_f]            column (i p + j) n_f + k
 *   REDCLIFF_DIRSPEC_FLATTENED  [p][n_f][2p - 1]       flatten_directed_spectrum_features, row-major
 * power (optional, may be NULL): [N][p (p + 1) / 2][n_f] doubles, |one-sided CPSD| of channel pairs
 *   (r, c <= r) at index r (r + 1) / 2 + c, times the bin frequency.
 * status / iters: [N][p (p - 1) / 2] int32 per (window, pair in the order (0,1), (0,2), ..., (p-2,p-1)):
 *   REDCLIFF_DIRSPEC_CONVERGED, _MAXITER (the features are those of the last iteration, as in the reference) or
 *   _PIVOT (a non-positive Cholesky pivot: the pair's features are NaN), and the iterations run.
 * A window holding a NaN gives a NaN row (and NaN power), runs no factorisation and reports CONVERGED, 0.
 * ws: redcliff_dirspec_ws_bytes(...) bytes, 16-byte aligned (the spectra and the NaN flags).
 * Limits: nperseg <= 256, p <= 1024, T >= nperseg > noverlap >= 0; outside them REDCLIFF_ELIMIT /
 * REDCLIFF_EINVAL and redcliff_dirspec_supported returns 0.  All checks precede any HIP call.
 * Stream-ordered, no host synchronisation, no atomics: the same arguments give the same bits, and a window's
 * row does not depend on the other windows of the call. */
#define REDCLIFF_DIRSPEC_F32 0
#define REDCLIFF_DIRSPEC_F64 1
#define REDCLIFF_DIRSPEC_VANILLA 0
#define REDCLIFF_DIRSPEC_FLATTENED 1
#define REDCLIFF_DIRSPEC_CONVERGED 0
#define REDCLIFF_DIRSPEC_MAXITER 1
#define REDCLIFF_DIRSPEC_PIVOT 2
typedef struct RedcliffDirspecArgs {
  int32_t N, T, p, nperseg, noverlap, max_iter;
  int32_t dtype, layout;
  double fs, min_freq, max_freq, tol;
  const void* X; int64_t x_wstride, x_tstride;
  float* out; int64_t out_rstride;
  double* power;
  void* ws; size_t ws_bytes;
  int32_t* status; int32_t* iters;
} RedcliffDirspecArgs;
int redcliff_dirspec_supported(int32_t T, int32_t p, int32_t nperseg, int32_t noverlap);
/* n_f for these bins (negative: an error code) */
int redcliff_dirspec_nfreq(int32_t nperseg, double fs, double min_freq, double max_freq);
size_t redcliff_dirspec_ws_bytes(int32_t N, int32_t T, int32_t p, int32_t nperseg, int32_t noverlap);
int redcliff_dirspec_run(const RedcliffDirspecArgs* a, void* stream);

/* ---- SLARAC and QRBS comparison baselines (tidybench/slarac.py, tidybench/qrbs.py) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout changes.
 *
 * One call solves P x S independent regressions: problem (b, s) is fit s of data set b.
 * data: [P][T][N] doubles.  With n = T - lags usable rows, sampled row i in [0, n) has the target time t = i + lags,
 *   the regressors z = [1, x_{t-1}, ..., x_{t-lags}] (D = lags N + 1) and the target
 *   REDCLIFF_TIDYBENCH_SLARAC: y = x_t;       REDCLIFF_TIDYBENCH_QRBS: y = x_t - x_{t-1}.
 * idx: the int32 row indices of fit (b, s) start at idx + b idx_pstride + s idx_fstride; count[b][s] of them are
 *   read.  count -1 = every row 0 .. n - 1 in order (SLARAC's fit of the full data).  max_count bounds every count
 *   (with -1 counted as n); it sizes the grid and the workspace.  An index outside [0, n), a count above max_count
 *   or below -1, or ncols outside [1, D] reads nothing out of bounds and gives the fit the status NONFINITE.
 * ncols: [P][S], SLARAC only (may be NULL for QRBS): the fit solves on the first ncols regressors (efflag N + 1).
 * SLARAC solves (Z_c Z_c^T) B = Z_c Y^T.  QRBS solves sklearn's Ridge(alpha) with an intercept:
 *   (Xc^T Xc + alpha I) W = Xc^T yc, X the lags N lag columns, both centred by the resample's own means.  The sums
 *   are accumulated on data shifted by the full series' column means, and the centring is the rank-one correction
 *   -k (mu - m)(mu - m)^T applied to those sums; sum x x^T - k mu mu^T is never formed on raw data.
 * coef: [P][S][N][Dout] doubles, Dout = D for SLARAC (intercept first) and lags N for QRBS; columns past ncols are
 *   zero; all zero unless the status is OK.
 * status: [P][S] int32.  The solve is a Cholesky factorisation in double that tracks min_j pivot_j / G_jj
 *   (pivot_ratio [P][S]); a fit with a ratio below 1e-8, a non-positive pivot or diagonal entry, or no rows is
 *   SINGULAR (the caller recomputes it with a minimum-norm solver); a non-finite sum gives NONFINITE.
 * ws: redcliff_tidybench_ws_bytes(P, S, N, lags, max_count) bytes, 16-byte aligned: the series means [P][N] and one
 *   partial of D (D + 1) / 2 + D N doubles per (fit, chunk of 512 sampled rows).
 * Limits: N <= 32, lags N <= 96, T > lags >= 1, P and S <= 65535; outside them REDCLIFF_ELIMIT / REDCLIFF_EINVAL,
 * redcliff_tidybench_supported returns 0 and _ws_bytes returns 0.  All checks precede any HIP call.
 * Stream-ordered, no host synchronisation, no atomics: rows accumulate in index order within a chunk and chunks in
 * chunk order, so the same arguments give the same bits and a problem's result does not depend on the batch. */
#define REDCLIFF_TIDYBENCH_SLARAC 0
#define REDCLIFF_TIDYBENCH_QRBS 1
#define REDCLIFF_TIDYBENCH_OK 0
#define REDCLIFF_TIDYBENCH_SINGULAR 1
#define REDCLIFF_TIDYBENCH_NONFINITE 2
typedef struct RedcliffTidybenchArgs {
  int32_t mode, P, S, T, N, lags;
  int32_t max_count, pad_;
  double alpha;                  /* QRBS only (> 0)                                                        */
  const double* data;
  const int32_t* idx; int64_t idx_pstride, idx_fstride;
  const int32_t* count;
  const int32_t* ncols;
  double* coef;
  int32_t* status;
  double* pivot_ratio;
  void* ws; size_t ws_bytes;
} RedcliffTidybenchArgs;
int redcliff_tidybench_supported(int32_t T, int32_t N, int32_t lags);
size_t redcliff_tidybench_ws_bytes(int32_t P, int32_t S, int32_t N, int32_t lags, int32_t max_count);
int redcliff_tidybench_run(const RedcliffTidybenchArgs* a, void* stream);

/* ---- LASAR comparison baseline (tidybench/lasar.py; sklearn's LassoLarsCV underneath) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout changes.
 *
 * One call runs P x S x N cross-validated lasso selections and refits (lags = 1): fit (b, s) is count[b][s] sampled
 * rows of data[b] ([P][T][N] doubles; idx, count, max_count and the strides as for redcliff_tidybench_run, count -1 =
 * every row in order), target j is channel j at time t regressed on all channels at t - 1.  KFold(cv) without
 * shuffling cuts the gathered rows into cv contiguous folds, the first count % cv one row longer.  Per target: the cv
 * fold paths of sklearn's lasso-LARS solver on the training rows' centred Gram matrix, the folds' alphas merged, the
 * mean squared held-out residual at each (the quadratic form of the linearly interpolated coefficients in the held-out
 * rows' sums), the argmin, the final path on all rows down to that alpha, and a Cholesky refit of the parents with a
 * positive coefficient on the uncentred sums under the pivot rule of redcliff_tidybench_run.
 * coef: [P][S][N][N] (target, parent), zero off the selection and unless the status is OK.  best_alpha [P][S][N];
 * best_index [P][S][N]: its index among the merged alphas with finite errors; selected [P][S][N]: bit i = parent i.
 * status [P][S][N]: OK; SINGULAR (the refit refused by the pivot rule, pivot_ratio [P][S][N] below 1e-8);
 *   DEGENERATE: a path met the solver's drop-for-good, alpha-increasing or non-finite-AA branch, dropped several
 *   coefficients in one step, stored more than 2 N + 4 knots or ended on a rising alpha, a fold trains on no more than
 *   N rows, or no alpha has a finite error (the caller recomputes the target on the host); NONFINITE: a non-finite
 *   sum, an index outside [0, T - 1), a count below cv or above max_count.
 * ws: redcliff_lasar_ws_bytes(P, S, N, lags, cv, max_count) bytes, 16-byte aligned.
 * Limits: N <= 16, lags == 1, 2 <= cv <= 8, P and S <= 65535; outside them REDCLIFF_ELIMIT / REDCLIFF_EINVAL,
 * redcliff_lasar_supported returns 0 and _ws_bytes returns 0.  All checks precede any HIP call.
 * Stream-ordered, no host synchronisation, no atomics, fixed summation orders that depend on the fit's count and cv
 * alone: the same arguments give the same bits and a target's result does not depend on the rest of the batch. */
#define REDCLIFF_LASAR_DEGENERATE 3
typedef struct RedcliffLasarArgs {
  int32_t P, S, T, N, lags, cv;
  int32_t max_count, pad_;
  const double* data;
  const int32_t* idx; int64_t idx_pstride, idx_fstride;
  const int32_t* count;
  double* coef;
  double* best_alpha;
  int32_t* best_index;
  int32_t* selected;
  int32_t* status;
  double* pivot_ratio;
  void* ws; size_t ws_bytes;
} RedcliffLasarArgs;
int redcliff_lasar_supported(int32_t T, int32_t N, int32_t lags);
size_t redcliff_lasar_ws_bytes(int32_t P, int32_t S, int32_t N, int32_t lags, int32_t cv, int32_t max_count);
int redcliff_lasar_run(const RedcliffLasarArgs* a, void* stream);

/* ---- DYNOTEARS comparison baseline (models/causalnex_dynotears_vanilla.py, models/dynotears_vanilla.py) ----
 * Purely additive entries: REDCLIFF_ABI_VERSION stays 10, no kernel id, no existing entry or layout changes.
 *
 * One call advances P independent problems (one per recording and lambda).  Problem b has n_rows[b] rows
 *   X row r:     X     + b x_pstride  + r x_rstride,  d contiguous values;
 *   Xlags row r: Xlags + b xl_pstride + r xl_rstride, p d contiguous values (lag 1 first),
 * float32 or float64 (dtype; strides in elements), so two views of one [P][T][d] buffer serve as X and Xlags.
 * Variables: wa[2 (p + 1) d^2] >= 0, viewed as (2 (p + 1) d) x d: rows [0, d) are W+, rows [d, 2d) W-, then per lag
 * the d x d block A+ followed by A-; W = W+ - W-, A = A+ - A-.  fixed[nv] (shared by the batch) marks the entries whose
 * bounds are (0, 0): both copies of W's diagonal and the tabu entries.  The problem minimises
 *   0.5/n ||X (I - W) - Xlags A||_F^2 + lambda_w[b] sum wa[:2 d^2] + lambda_a[b] sum wa[2 d^2:]   s.t. tr expm(W o W) = d
 * by the reference's augmented-Lagrangian loop (max_iter, h_tol, rho0 = 1, alpha0 = 0, rho_max = 1e20) around a
 * limited-memory projected quasi-Newton solver that stops by L-BFGS-B's rules (m pairs, factr, pgtol, maxiter,
 * maxfun, maxls; scipy's defaults are 10, 1e7, 1e-5, 15000, 15000, 20).  rho0 = 0 is accepted with max_iter = 1 only.
 * start != 0 forms the Gram matrices and resets every problem; every call then advances each unfinished problem by at
 * most evals_per_launch evaluations and stores in *remaining (device memory) how many are still unfinished: call again
 * with start = 0 and the same buffers until it reads 0.  The state between calls is in ws.
 * Outputs of a finished problem: W [P][d][d], A [P][p d][d], wa [P][nv] (may be NULL), status [P],
 *   stats [P][6]: h, rho, alpha, f and projected-gradient norm at the end of the last inner solve, failed line searches;
 *   counts [P][6]: outer iterations, inner solves, quasi-Newton iterations, evaluations, non-finite trial values, launches.
 * A non-finite Gram entry or a recording without rows gives NONFINITE and NaN outputs.  A non-finite trial value counts
 * as larger than any finite one (the step shrinks); it is counted, and x never becomes non-finite.
 * Limits: d <= 12, (p + 1) d <= 24, m <= 16; outside them REDCLIFF_ELIMIT, redcliff_dynotears_supported returns 0
 * and _ws_bytes returns 0.  All checks precede any HIP call.  Stream-ordered, no host synchronisation; every sum runs
 * in a fixed order, so the same arguments give the same bits whatever the batch and whatever evals_per_launch. */
#define REDCLIFF_DYNOTEARS_F32 0
#define REDCLIFF_DYNOTEARS_F64 1
#define REDCLIFF_DYNOTEARS_CONVERGED 0
#define REDCLIFF_DYNOTEARS_MAXITER 1
#define REDCLIFF_DYNOTEARS_RHO_CAP 2
#define REDCLIFF_DYNOTEARS_NONFINITE 3
typedef struct RedcliffDynotearsArgs {
  int32_t P, d, p, dtype;
  int32_t start, evals_per_launch;
  int32_t max_iter, m, maxiter, maxfun, maxls, pad_;
  double h_tol, rho0, alpha0, rho_max, factr, pgtol;
  const void* X; int64_t x_pstride, x_rstride;
  const void* Xlags; int64_t xl_pstride, xl_rstride;
  const int32_t* n_rows;
  const double* lambda_w;
  const double* lambda_a;
  const uint8_t* fixed;
  double* W; double* A; double* wa;
  int32_t* status;
  double* stats;
  int32_t* counts;
  int32_t* remaining;
  void* ws; size_t ws_bytes;
} RedcliffDynotearsArgs;
int redcliff_dynotears_supported(int32_t d, int32_t p);
size_t redcliff_dynotears_ws_bytes(int32_t P, int32_t d, int32_t p, int32_t m);
int redcliff_dynotears_run(const RedcliffDynotearsArgs* a, void* stream);

/* Per-kernel HIP-event timing for benchmarking: redcliff_kernel_timing(1) brackets every
 * kernel launched by redcliff_train_step with events on its stream; redcliff_kernel_times()
 * synchronises them and returns per-kernel totals (ids 0..11: supports, emb_fwd, fac_fwd,
 * fac_bwd, emb_bwd, emb_final, fac_mix, emb_combine, fac_lead, redcliff_score_recording's
 * score, score_graphs, and redcliff_cemb_score_recording's score_cemb; the launches of
 * redcliff_score_recording_pack count under supports, score and score_graphs).  Returns the number
 * of kernel ids.
 * When a single fit (R == 1) splits into two kernel chains (GEMM-shaped embedder and / or
 * matrix-core factor path), the factor chain runs on an internal second stream (one per host
 * thread and device) forked from and joined back into `stream` with events, so stream
 * ordering for the caller is unchanged.  Packed replicas run on `stream` only. */
int redcliff_kernel_timing(int32_t enable);
int redcliff_kernel_times(double* total_ms, int64_t* counts, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* REDCLIFF_HIP_H */
