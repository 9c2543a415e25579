// rc_dynotears.h -- limits, per-problem state and workspace layout of the batched DYNOTEARS solves
// (rc_dynotears.hip; models/causalnex_dynotears_vanilla.py and models/dynotears_vanilla.py of the reference).
#pragma once
#include "rc_common.h"

#define DY_DMAX 12        // d <= 12
#define DY_QMAX 24        // (p + 1) d <= 24: p = 1 up to d 12, p = 2 up to d 8, p = 3 up to d 6
#define DY_NVMAX (2 * DY_QMAX * DY_DMAX)   // 576 variables
#define DY_MMAX 16        // history pairs
#define DY_THREADS 64     // one wavefront per problem: reductions are xor butterflies, no cross-wave hand-off
#define DY_TAYLOR 12      // Taylor degree of the matrix exponential at ||M / 2^s||_1 <= 1/4 (remainder < 3e-18)
#define DY_SQMAX 60       // more squarings than this: the trial value counts as non-finite

#define DY_PH_START 0     // the next evaluation is the first of an inner solve (at wa_est)
#define DY_PH_SEARCH 1    // the next evaluation is a line-search trial point P(x + t dir)

// What survives between launches, besides the vectors.  All lanes of the wavefront hold the same copy.
struct DyState {
  double f, hx, t, gd, pg, rho, alpha, h_value, h_new, f_last, pg_last, pad_[5];
  int32_t phase, done, status, ls_iter, hist_n, hist_next, steep, inner_iter, inner_evals, outer_iter;
  int32_t n_solves, n_qn, n_evals, n_nonfinite, n_launch, n_lsfail;
};
static_assert(sizeof(DyState) == 16 * 8 + 16 * 4, "DyState layout");
#define DY_STATE_DOUBLES ((int)(sizeof(DyState) / sizeof(double)))

__host__ __device__ inline int rc_dy_q(int d, int p) { return (p + 1) * d; }
__host__ __device__ inline int rc_dy_nv(int d, int p) { return 2 * (p + 1) * d * d; }
// one problem's slice, in doubles: state | S [q][q] | x, g, dir, wa_est [nv] each | s pairs [m][nv] | y pairs [m][nv]
__host__ __device__ inline size_t rc_dy_off_S() { return DY_STATE_DOUBLES; }
__host__ __device__ inline size_t rc_dy_off_vec(int d, int p) { return rc_dy_off_S() + (size_t)rc_dy_q(d, p) * rc_dy_q(d, p); }
__host__ __device__ inline size_t rc_dy_off_hist(int d, int p) { return rc_dy_off_vec(d, p) + 4 * (size_t)rc_dy_nv(d, p); }
__host__ __device__ inline size_t rc_dy_slice(int d, int p, int m) {
  return (rc_dy_off_hist(d, p) + 2 * (size_t)m * rc_dy_nv(d, p) + 7) & ~(size_t)7;
}

struct DyCtx {
  int P, d, p, q, nv, m, dtype, epl;
  int max_iter, maxiter, maxfun, maxls;
  double h_tol, rho0, alpha0, rho_max, ftol, pgtol;
  const void* X; int64_t x_ps, x_rs;
  const void* Xl; int64_t xl_ps, xl_rs;
  const int32_t* n_rows;
  const double* lambda_w;
  const double* lambda_a;
  const uint8_t* fixed;
  double* W; double* A; double* wa;
  int32_t* status; double* stats; int32_t* counts; int32_t* remaining;
  double* ws; size_t slice;
};
