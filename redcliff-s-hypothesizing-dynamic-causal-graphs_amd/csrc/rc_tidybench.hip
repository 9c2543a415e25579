// rc_tidybench.hip -- the SLARAC and QRBS comparison baselines (tidybench/slarac.py, tidybench/qrbs.py of the
// reference): every least-squares / ridge fit of a batch of data sets in one call.
//
// Problem (b, s) is fit s of data set b: count[b][s] sampled rows of data[b] (indices drawn on the host), regressed
// on the first ncols[b][s] regressors.  The regressors and the target of sampled row i are the contiguous block
// data[b][i .. i + lags] of (lags + 1) N doubles, so Z is never materialised.
//
//   k_tb_means  (data set)              QRBS only: the column means of the full series, the shift of the accumulation.
//   k_tb_gram   (chunk, fit, data set)  TB_CH sampled rows per workgroup, TB_TR at a time staged in LDS as
//        [1, x_{t-1}, .., x_{t-lags}, y] (QRBS: x shifted by the series means, y = x_t - x_{t-1}); lane-owned entries
//        of the upper triangle of Z^T Z and of Z^T Y accumulate over the staged rows in row order; one partial per
//        chunk goes to the workspace.
//   k_tb_solve  one wavefront per problem: the partials summed in chunk order, QRBS's rank-one centring correction
//        and alpha, a Cholesky factorisation of the leading block that tracks min_j pivot_j / G_jj, and the two
//        triangular solves for the N right-hand sides.
//
// Everything is double on the vector units.  No atomics and no host synchronisation: sums run in a fixed order
// that depends on the fit's own count alone, so the same arguments give the same bits and a problem's result does
// not depend on the rest of the batch.
#include <cmath>
#include <cstring>

#include "rc_tidybench.h"

namespace {

__device__ inline void tb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ inline int tb_tri(int i, int j) { return j * (j + 1) / 2 + i; }  // i <= j

// effective row count of fit q: -1 = every row in order; above the call's max_count = invalid (-2)
__device__ inline int tb_count(const TbCtx& c, int q, int maxcnt, bool* all) {
  int cnt = c.count[q];
  *all = cnt == -1;
  if (cnt == -1) cnt = c.n;
  if (cnt < 0 || cnt > maxcnt) return -2;
  return cnt;
}

__global__ __launch_bounds__(256) void k_tb_means(TbCtx c) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ng = 256 / c.N, g = tid / c.N, m = tid - g * c.N;
  const double* X = c.data + (int64_t)b * c.T * c.N;
  double v = 0.0;
  if (g < ng)
    for (int t = g; t < c.T; t += ng) v += X[(int64_t)t * c.N + m];
  red[tid] = v;
  __syncthreads();
  if (tid < c.N) {
    double s = 0.0;
    for (int k = 0; k < ng; ++k) s += red[k * c.N + tid];
    c.means[(int64_t)b * c.N + tid] = s / (double)c.T;
  }
}

template <int EPT>
__global__ __launch_bounds__(TB_THREADS) void k_tb_gram(TbCtx c, int maxcnt) {
  extern __shared__ __attribute__((aligned(16))) char tb_smem[];
  double* sh = reinterpret_cast<double*>(tb_smem);
  const int chunk = blockIdx.x, s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int q = b * c.S + s;
  bool all;
  const int cnt = tb_count(c, q, maxcnt, &all);
  const int start = chunk * TB_CH;
  if (cnt < 0 || start >= cnt) return;   // uniform over the workgroup
  const int end = start + TB_CH < cnt ? start + TB_CH : cnt;

  int ab[EPT];
  double acc[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = tid + k * TB_THREADS;
    int i = 0, j = 0;
    if (e < c.ntri) {
      j = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
      while (j * (j + 1) / 2 > e) --j;
      while ((j + 1) * (j + 2) / 2 <= e) ++j;
      i = e - j * (j + 1) / 2;
    } else if (e < c.nent) {
      const int r = e - c.ntri;
      i = r / c.N;
      j = c.Dz + (r - i * c.N);
    }
    ab[k] = i | (j << 16);
    acc[k] = 0.0;
  }

  const int N = c.N, W = c.W, Dz = c.Dz, lags = c.lags;
  const bool qrbs = c.mode == REDCLIFF_TIDYBENCH_QRBS;
  const double* X = c.data + (int64_t)b * c.T * N;
  const double* mu = c.means + (int64_t)b * N;
  const int32_t* ix = all ? nullptr : c.idx + (int64_t)b * c.idx_pstride + (int64_t)s * c.idx_fstride;
  for (int tile = start; tile < end; tile += TB_TR) {
    const int rows = end - tile < TB_TR ? end - tile : TB_TR;
    __syncthreads();
    for (int u = tid; u < rows * W; u += TB_THREADS) {
      const int r = u / W, col = u - r * W;
      const int i = all ? tile + r : ix[tile + r];
      double v;
      if ((unsigned)i >= (unsigned)c.n) {
        v = NAN;   // an index outside the series: the fit ends NONFINITE, nothing outside data[b] is read
      } else if (col == 0) {
        v = 1.0;
      } else {
        const double* blk = X + (int64_t)i * N;
        if (col < Dz) {
          const int k = (col - 1) / N, m = (col - 1) - k * N;
          v = blk[(lags - 1 - k) * N + m];
          if (qrbs) v -= mu[m];
        } else {
          const int m = col - Dz;
          v = blk[lags * N + m];
          if (qrbs) v -= blk[(lags - 1) * N + m];
        }
      }
      sh[u] = v;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const double* row = sh + r * W;
#pragma unroll
      for (int k = 0; k < EPT; ++k) acc[k] = fma(row[ab[k] & 0xffff], row[ab[k] >> 16], acc[k]);
    }
  }
  double* part = c.part + ((int64_t)q * c.maxch + chunk) * c.nent;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = tid + k * TB_THREADS;
    if (e < c.nent) part[e] = acc[k];
  }
}

__global__ __launch_bounds__(256) void k_tb_solve(TbCtx c, int maxcnt, int wpw) {
  extern __shared__ __attribute__((aligned(16))) char tb_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t q64 = (int64_t)blockIdx.x * wpw + wave;
  if (q64 >= (int64_t)c.P * c.S) return;   // no workgroup barrier below: the waves are independent
  const int q = (int)q64;
  const int N = c.N, Dz = c.Dz, ntri = c.ntri, nent = c.nent;
  double* A = reinterpret_cast<double*>(tb_smem) + (size_t)wave * rc_tb_wave_doubles(N, c.lags);
  double* R = A + ntri;
  double* dg = A + nent;
  const bool qrbs = c.mode == REDCLIFF_TIDYBENCH_QRBS;
  bool all;
  const int cnt = tb_count(c, q, maxcnt, &all);
  const int off = qrbs ? 1 : 0;
  const int nc = qrbs ? Dz - 1 : c.ncols[q];
  int bad = cnt < 0 || nc < 1 || off + nc > Dz;

  // the chunk partials, in chunk order
  const int nch = cnt > 0 ? rc_tb_nchunk(cnt) : 0;
  const double* part = c.part + (int64_t)q * c.maxch * nent;
  for (int e = lane; e < nent; e += 64) {
    double v = 0.0;
    for (int ch = 0; ch < nch; ++ch) v += part[(int64_t)ch * nent + e];
    A[e] = v;
    if (!(fabs(v) <= 1.79769313486231570815e308)) bad = 1;
  }
  bad = __any(bad);
  tb_wave_sync();

  int st = bad ? REDCLIFF_TIDYBENCH_NONFINITE : REDCLIFF_TIDYBENCH_OK;
  double ratio = 0.0;
  const int hi = off + nc;
  if (!bad && cnt == 0) st = REDCLIFF_TIDYBENCH_SINGULAR;
  if (st == REDCLIFF_TIDYBENCH_OK) {
    if (qrbs) {
      // centred on the resample's own means: sum (x - m)(x - m)^T - k d d^T with d = sum (x - m) / k, plus alpha
      const double k = (double)cnt;
      for (int j = 1; j < Dz; ++j) {
        const double sj = A[tb_tri(0, j)];
        for (int i = 1 + lane; i <= j; i += 64) {
          double v = A[tb_tri(i, j)] - A[tb_tri(0, i)] * sj / k;
          if (i == j) v += c.alpha;
          A[tb_tri(i, j)] = v;
        }
      }
      for (int e = lane; e < (Dz - 1) * N; e += 64) {
        const int j = 1 + e / N, m = e - (j - 1) * N;
        R[j * N + m] -= A[tb_tri(0, j)] * R[m] / k;
      }
    }
    tb_wave_sync();
    for (int j = off + lane; j < hi; j += 64) dg[j] = A[tb_tri(j, j)];
    tb_wave_sync();
    ratio = INFINITY;
    for (int j = off; j < hi; ++j) {
      const double piv = A[tb_tri(j, j)], g = dg[j];
      if (!(g > 0.0) || !(piv > 0.0)) {
        st = REDCLIFF_TIDYBENCH_SINGULAR;
        ratio = g > 0.0 ? piv / g : 0.0;
        break;
      }
      const double r = piv / g;
      ratio = r < ratio ? r : ratio;
      if (r < TB_PIVOT_MIN) {
        st = REDCLIFF_TIDYBENCH_SINGULAR;
        break;
      }
      const double d = sqrt(piv);
      tb_wave_sync();
      for (int i = j + 1 + lane; i < hi; i += 64) A[tb_tri(j, i)] /= d;
      if (lane == 0) A[tb_tri(j, j)] = d;
      tb_wave_sync();
      for (int i2 = j + 1; i2 < hi; ++i2) {
        const double u2 = A[tb_tri(j, i2)];
        for (int i1 = j + 1 + lane; i1 <= i2; i1 += 64) A[tb_tri(i1, i2)] -= A[tb_tri(j, i1)] * u2;
      }
      tb_wave_sync();
    }
  }
  if (st == REDCLIFF_TIDYBENCH_OK && lane < N) {
    const int m = lane;
    for (int j = off; j < hi; ++j) {   // U^T w = r
      double v = R[j * N + m];
      for (int k = off; k < j; ++k) v -= A[tb_tri(k, j)] * R[k * N + m];
      R[j * N + m] = v / A[tb_tri(j, j)];
    }
    for (int j = hi - 1; j >= off; --j) {   // U b = w
      double v = R[j * N + m];
      for (int k = j + 1; k < hi; ++k) v -= A[tb_tri(j, k)] * R[k * N + m];
      R[j * N + m] = v / A[tb_tri(j, j)];
    }
  }
  tb_wave_sync();
  const int dout = c.dout;
  double* coef = c.coef + (int64_t)q * N * dout;
  for (int e = lane; e < N * dout; e += 64) {
    const int m = e / dout, jc = e - m * dout;
    coef[e] = (st == REDCLIFF_TIDYBENCH_OK && jc < nc) ? R[(off + jc) * N + m] : 0.0;
  }
  if (lane == 0) {
    c.status[q] = st;
    c.pivot[q] = ratio;
  }
}

using GramKern = void (*)(TbCtx, int);

int tb_ctx(int32_t mode, int32_t P, int32_t S, int32_t T, int32_t N, int32_t lags, int32_t max_count, TbCtx* c) {
  memset(c, 0, sizeof(*c));
  if ((mode != REDCLIFF_TIDYBENCH_SLARAC && mode != REDCLIFF_TIDYBENCH_QRBS) || P < 0 || S < 0 || N < 1 || lags < 1 || T <= lags ||
      max_count < 0) {
    rc_set_error("tidybench: bad arguments (mode=%d P=%d S=%d T=%d N=%d lags=%d max_count=%d)", mode, P, S, T, N, lags, max_count);
    return REDCLIFF_EINVAL;
  }
  if (N > TB_NMAX || (int64_t)lags * N > TB_LNMAX || P > 65535 || S > 65535) {
    rc_set_error("tidybench: outside kernel limits (N <= %d, lags * N <= %d, P and S <= 65535; N=%d lags=%d P=%d S=%d)", TB_NMAX,
                 TB_LNMAX, N, lags, P, S);
    return REDCLIFF_ELIMIT;
  }
  c->mode = mode; c->P = P; c->S = S; c->T = T; c->N = N; c->lags = lags; c->n = T - lags;
  c->Dz = rc_tb_dz(N, lags); c->W = rc_tb_w(N, lags); c->ntri = rc_tb_ntri(N, lags); c->nent = rc_tb_nent(N, lags);
  c->maxch = rc_tb_nchunk(max_count);
  c->dout = mode == REDCLIFF_TIDYBENCH_QRBS ? lags * N : lags * N + 1;
  return 0;
}

size_t tb_means_bytes(int P, int N) { return (sizeof(double) * (size_t)P * (size_t)N + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int redcliff_tidybench_supported(int32_t T, int32_t N, int32_t lags) {
  TbCtx c;
  return tb_ctx(REDCLIFF_TIDYBENCH_SLARAC, 1, 1, T, N, lags, 0, &c) == 0 ? 1 : 0;
}

size_t redcliff_tidybench_ws_bytes(int32_t P, int32_t S, int32_t N, int32_t lags, int32_t max_count) {
  TbCtx c;
  if (tb_ctx(REDCLIFF_TIDYBENCH_SLARAC, P, S, lags + 1, N, lags, max_count, &c) != 0) return 0;
  return tb_means_bytes(P, N) + sizeof(double) * (size_t)P * (size_t)S * (size_t)c.maxch * (size_t)c.nent + 16;
}

int redcliff_tidybench_run(const RedcliffTidybenchArgs* a, void* stream) {
  if (!a) { rc_set_error("null tidybench arguments"); return REDCLIFF_EINVAL; }
  TbCtx c;
  int e = tb_ctx(a->mode, a->P, a->S, a->T, a->N, a->lags, a->max_count, &c);
  if (e) return e;
  if (a->P == 0 || a->S == 0) return 0;
  if (!a->data || !a->count || !a->coef || !a->status || !a->pivot_ratio || !a->ws || (a->max_count > 0 && !a->idx) ||
      (a->mode == REDCLIFF_TIDYBENCH_SLARAC && !a->ncols)) {
    rc_set_error("tidybench_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->idx_fstride < 0 || a->idx_pstride < 0 || (a->S > 1 && a->idx_fstride < a->max_count && a->idx_fstride != 0) ||
      !(a->alpha >= 0.0) || (a->mode == REDCLIFF_TIDYBENCH_QRBS && !(a->alpha > 0.0))) {
    rc_set_error("tidybench_run: bad strides or alpha (idx_fstride=%lld idx_pstride=%lld max_count=%d alpha=%g)",
                 (long long)a->idx_fstride, (long long)a->idx_pstride, a->max_count, a->alpha);
    return REDCLIFF_EINVAL;
  }
  const size_t need = redcliff_tidybench_ws_bytes(a->P, a->S, a->N, a->lags, a->max_count);
  if (a->ws_bytes < need) { rc_set_error("tidybench_run: workspace too small: %zu < %zu", a->ws_bytes, need); return REDCLIFF_EWORKSPACE; }
  if ((reinterpret_cast<uintptr_t>(a->ws) & 15) != 0) { rc_set_error("tidybench_run: workspace not 16-byte aligned"); return REDCLIFF_EINVAL; }
  c.idx_pstride = a->idx_pstride; c.idx_fstride = a->idx_fstride; c.alpha = a->alpha;
  c.data = a->data; c.idx = a->idx; c.count = a->count; c.ncols = a->ncols;
  c.coef = a->coef; c.status = a->status; c.pivot = a->pivot_ratio;
  c.means = static_cast<double*>(a->ws);
  c.part = reinterpret_cast<double*>(static_cast<char*>(a->ws) + tb_means_bytes(a->P, a->N));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->mode == REDCLIFF_TIDYBENCH_QRBS) {
    hipLaunchKernelGGL(k_tb_means, dim3(c.P), dim3(256), 0, s, c);
    if ((e = rc_check(hipGetLastError(), "k_tb_means"))) return e;
  }
  if (c.maxch > 0) {
    const int per = (c.nent + TB_THREADS - 1) / TB_THREADS;
    GramKern k = per <= 1 ? k_tb_gram<1> : per <= 2 ? k_tb_gram<2> : per <= 4 ? k_tb_gram<4> : per <= 8 ? k_tb_gram<8>
                 : per <= 16 ? k_tb_gram<16> : k_tb_gram<TB_EPT_MAX>;
    hipLaunchKernelGGL(k, dim3((unsigned)c.maxch, (unsigned)c.S, (unsigned)c.P), dim3(TB_THREADS), rc_tb_gram_lds_bytes(c.N, c.lags), s,
                       c, a->max_count);
    if ((e = rc_check(hipGetLastError(), "k_tb_gram"))) return e;
  }
  const int wpw = rc_tb_wpw(c.N, c.lags);
  const int64_t nprob = (int64_t)c.P * c.S;
  hipLaunchKernelGGL(k_tb_solve, dim3((unsigned)((nprob + wpw - 1) / wpw)), dim3(64 * wpw), sizeof(double) * wpw * rc_tb_wave_doubles(c.N, c.lags),
                     s, c, a->max_count, wpw);
  if ((e = rc_check(hipGetLastError(), "k_tb_solve"))) return e;
  return 0;
}

}  // extern "C"
