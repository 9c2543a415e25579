// rc_lasar.h -- context, limits, LDS and workspace layouts of the batched LASAR fits
// (rc_lasar.hip; tidybench/lasar.py of the reference, sklearn's LassoLarsCV underneath).
#pragma once
#include "rc_common.h"
#include "rc_tidybench.h"

#define LS_NMAX 16       // N <= 16: the published shapes are N 10 and N 12
#define LS_CVMAX 8       // cross-validation folds
#define LS_WPW_PATH 4    // wavefronts (paths) per workgroup of k_ls_path
#define LS_WPW_SEL 2     // wavefronts (targets) per workgroup of k_ls_select
#define LS_MAX_ITER 500  // LassoLarsCV's max_iter (never reached: the knot capacity is smaller)

// what a path went through that the kernels leave to the host: any of these makes the target DEGENERATE
#define LS_F_DROP_FOR_GOOD 1
#define LS_F_ALPHA_UP 2
#define LS_F_AA 4
#define LS_F_MULTI_DROP 8
#define LS_F_KNOTS 16
#define LS_F_XROUTE 32
#define LS_F_ORDER 64
#define LS_F_NONFINITE 128

// knots one path may store: N additions and a few drop / re-add pairs (lasar_knot_capacity of tidybench.py)
__host__ __device__ inline int rc_ls_kcap(int N) { return 2 * N + 4; }
// One staged row is [1, z, y] = [1, x_{t-1} - mu, x_t - mu].  One set of sums: the upper triangle of [1, z]^T [1, z]
// (column-packed as in rc_tidybench.h), then [1, z]^T y [1 + N][N], then sum y_m^2 [N].
__host__ __device__ inline int rc_ls_nent(int N) { return rc_tb_nent(N, 1) + N; }
__host__ __device__ inline int rc_ls_maxchf(int64_t max_count, int cv) { return rc_tb_nchunk((max_count + cv - 1) / cv); }
// the path solver's state of one wavefront, in doubles: G, G0, L [N][N]; Cov, Cov0, sign, ls, corr [N]; indices and
// active [N] (as ints in one double each); the knots' alphas [kcap] and coefficients [kcap][N]
__host__ __device__ inline size_t rc_ls_solver_doubles(int N) { return (size_t)3 * N * N + 7 * N + (size_t)rc_ls_kcap(N) * (N + 1); }
// k_ls_select adds the merged alphas, the unique ones and their errors [cv kcap] each, and the folds' (n_test,
// n_train, train means of z [N] and of y)
__host__ __device__ inline size_t rc_ls_select_doubles(int N, int cv) {
  return rc_ls_solver_doubles(N) + (size_t)3 * cv * rc_ls_kcap(N) + (size_t)cv * (N + 3);
}

struct LsCtx {
  int P, S, T, N, cv, n, nent, ntri, maxchf, kcap, max_count;
  int64_t idx_pstride, idx_fstride;
  const double* data;
  const int32_t* idx;
  const int32_t* count;
  double* coef;          // [P][S][N][N]
  double* best_alpha;    // [P][S][N]
  int32_t* best_index;   // [P][S][N]
  int32_t* selected;     // [P][S][N] bit i: parent i selected
  int32_t* status;       // [P][S][N]
  double* pivot;         // [P][S][N]
  double* means;         // [P][N]                         (workspace)
  double* part;          // [P][S][cv][maxchf][nent]       (workspace)
  double* fsum;          // [P][S][cv][nent]               (workspace)
  double* kn_alpha;      // [P][S][N][cv][kcap]            (workspace)
  double* kn_coef;       // [P][S][N][cv][kcap][N]         (workspace)
  int32_t* kn_meta;      // [P][S][N][cv][2]: knots, flags (workspace)
};
