// rc_tidybench.h -- context, limits, LDS and workspace layouts of the batched SLARAC / QRBS fits
// (rc_tidybench.hip; tidybench/slarac.py and tidybench/qrbs.py of the reference).
#pragma once
#include "rc_common.h"

#define TB_CH 512        // sampled rows of one Gram partial: the chunk partition depends on the fit's count alone
#define TB_TR 32         // rows staged in LDS at a time
#define TB_THREADS 256   // lanes of k_tb_gram; each owns up to TB_EPT_MAX entries of [Z^T Z | Z^T Y]
#define TB_EPT_MAX 32
#define TB_NMAX 32       // N <= 32
#define TB_LNMAX 96      // lags * N <= 96
#define TB_PIVOT_MIN 1e-8  // a fit whose min_j pivot_j / G_jj is below this is SINGULAR

// One staged row is [1, x_{t-1}, ..., x_{t-lags}, y]: Dz = 1 + lags N regressors (QRBS uses the leading 1 to
// carry the resample's shifted sums) and N targets.
__host__ __device__ inline int rc_tb_dz(int N, int lags) { return 1 + lags * N; }
__host__ __device__ inline int rc_tb_w(int N, int lags) { return 1 + lags * N + N; }
__host__ __device__ inline int rc_tb_ntri(int N, int lags) { return rc_tb_dz(N, lags) * (rc_tb_dz(N, lags) + 1) / 2; }
// entries of one partial: the upper triangle of Z^T Z (column-packed: (i <= j) at j (j + 1) / 2 + i), then Z^T Y [Dz][N]
__host__ __device__ inline int rc_tb_nent(int N, int lags) { return rc_tb_ntri(N, lags) + rc_tb_dz(N, lags) * N; }
__host__ __device__ inline size_t rc_tb_gram_lds_bytes(int N, int lags) { return sizeof(double) * TB_TR * (size_t)rc_tb_w(N, lags); }
// k_tb_solve, per wavefront: the summed partial and the diagonal before the factorisation
__host__ __device__ inline size_t rc_tb_wave_doubles(int N, int lags) { return (size_t)rc_tb_nent(N, lags) + rc_tb_dz(N, lags); }
__host__ __device__ inline int rc_tb_wpw(int N, int lags) { return rc_tb_wave_doubles(N, lags) * 8 * 4 <= 32768 ? 4 : 1; }
__host__ __device__ inline int rc_tb_nchunk(int64_t cnt) { return (int)((cnt + TB_CH - 1) / TB_CH); }

struct TbCtx {
  int P, S, T, N, lags, mode, n, Dz, W, ntri, nent, maxch, dout;
  int64_t idx_pstride, idx_fstride;
  double alpha;
  const double* data;
  const int32_t* idx;
  const int32_t* count;
  const int32_t* ncols;
  double* coef;
  int32_t* status;
  double* pivot;
  double* means;   // [P][N]   (workspace)
  double* part;    // [P][S][maxch][nent]   (workspace)
};
