// rc_lasar.hip -- the LASAR comparison baseline (tidybench/lasar.py of the reference): every cross-validated lasso
// path and least-squares refit of a batch of data sets in one call (lags = 1).
//
// Fit (b, s) is count[b][s] sampled rows of data[b] (indices drawn on the host).  KFold(cv) without shuffling cuts
// the gathered rows into cv contiguous folds; everything LassoLarsCV computes per target is a function of the
// folds' sums over [1, z, y] = [1, x_{t-1} - mu, x_t - mu] (mu: the series' column means), which the N targets share.
//
//   k_ls_means   (data set)                 the column means of the full series, the shift of the accumulation.
//   k_ls_gram    (fold x chunk, fit, data set)  up to TB_CH gathered rows of one fold per workgroup, TB_TR at a time
//        staged in LDS; lane-owned entries accumulate over the staged rows in row order; one partial per chunk.
//   k_ls_fold    (fold, fit, data set)      the fold's sums: its chunks' partials in chunk order.
//   k_ls_path    one wavefront per (data set, fit, target, fold): the training sums (the other folds' sums in fold
//        order), centred on the training means, and sklearn's lasso-LARS path on that Gram matrix; the knots go to
//        the workspace.
//   k_ls_select  one wavefront per (data set, fit, target): the folds' alphas merged and de-duplicated by rank
//        counting, each fold's mean squared held-out residual at every alpha as the quadratic form of the
//        interpolated coefficients in the fold's own (test) sums, the argmin, the final path on all rows down to the
//        best alpha, the positive coefficients and their pivot-rule Cholesky refit on the uncentred sums.
//
// The path's step loop is sequential and its vectors have at most LS_NMAX entries, so one lane walks it (the
// restatement of _lars_path in tidybench.py, decision by decision) while the wavefront's other lanes build the
// matrices and evaluate the alphas; the parallelism is over the ~10^5 paths of a call.  A path that meets one of the
// solver's degenerate branches stops and flags its target DEGENERATE for the host.  Everything is double on the
// vector units, no atomics, no host synchronisation, fixed summation orders that depend on the fit's count alone.
#include <cmath>
#include <cstring>

#include "rc_lasar.h"

namespace {

constexpr double LS_EPS = 2.220446049250313e-16;       // finfo(float64).eps
constexpr double LS_TINY32 = 1.1754943508222875e-38;   // finfo(float32).tiny
constexpr double LS_EQ_TOL = 1.1920928955078125e-07;   // finfo(float32).eps
constexpr double LS_DBL_MAX = 1.79769313486231570815e308;

__device__ inline void ls_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__host__ __device__ inline int ls_tri(int i, int j) { return i <= j ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j; }
__host__ __device__ inline bool ls_finite(double v) { return fabs(v) <= LS_DBL_MAX; }

// effective row count of fit q: -1 = every row in order; outside [cv, max_count] = invalid (-2)
__device__ inline int ls_count(const LsCtx& c, int q, bool* all) {
  int cnt = c.count[q];
  *all = cnt == -1;
  if (cnt == -1) cnt = c.n;
  if (cnt < c.cv || cnt > c.max_count) return -2;
  return cnt;
}

// fold f of cnt rows: [start, start + len)
__device__ inline void ls_fold(int cnt, int cv, int f, int* start, int* len) {
  const int base = cnt / cv, rem = cnt - base * cv;
  *start = f * base + (f < rem ? f : rem);
  *len = base + (f < rem ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_ls_means(LsCtx c) {
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
__global__ __launch_bounds__(TB_THREADS) void k_ls_gram(LsCtx c) {
  extern __shared__ __attribute__((aligned(16))) char ls_smem[];
  double* sh = reinterpret_cast<double*>(ls_smem);
  const int f = blockIdx.x / c.maxchf, chunk = blockIdx.x - f * c.maxchf;
  const int s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int q = b * c.S + s;
  bool all;
  const int cnt = ls_count(c, q, &all);
  if (cnt < 0) return;   // uniform over the workgroup
  int fstart, flen;
  ls_fold(cnt, c.cv, f, &fstart, &flen);
  if (chunk * TB_CH >= flen) return;
  const int start = fstart + chunk * TB_CH;
  const int end = (chunk + 1) * TB_CH < flen ? start + TB_CH : fstart + flen;

  const int N = c.N, Dz = 1 + N, W = 1 + 2 * N, ntri = c.ntri, ncross = ntri + Dz * N;
  int ab[EPT];
  double acc[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = tid + k * TB_THREADS;
    int i = 0, j = 0;
    if (e < ntri) {
      j = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
      while (j * (j + 1) / 2 > e) --j;
      while ((j + 1) * (j + 2) / 2 <= e) ++j;
      i = e - j * (j + 1) / 2;
    } else if (e < ncross) {
      const int r = e - ntri;
      i = r / N;
      j = Dz + (r - i * N);
    } else if (e < c.nent) {
      i = j = Dz + (e - ncross);
    }
    ab[k] = i | (j << 16);
    acc[k] = 0.0;
  }

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
        const int m = col <= N ? col - 1 : col - Dz;
        v = X[(int64_t)(col <= N ? i : i + 1) * N + m] - mu[m];
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
  double* part = c.part + (((int64_t)q * c.cv + f) * c.maxchf + chunk) * c.nent;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = tid + k * TB_THREADS;
    if (e < c.nent) part[e] = acc[k];
  }
}

__global__ __launch_bounds__(256) void k_ls_fold(LsCtx c) {
  const int f = blockIdx.x, q = blockIdx.z * c.S + blockIdx.y;
  bool all;
  const int cnt = ls_count(c, q, &all);
  int fstart, flen = 0;
  if (cnt >= 0) ls_fold(cnt, c.cv, f, &fstart, &flen);
  const int nch = rc_tb_nchunk(flen);
  const double* part = c.part + ((int64_t)q * c.cv + f) * c.maxchf * c.nent;
  double* out = c.fsum + ((int64_t)q * c.cv + f) * c.nent;
  for (int e = threadIdx.x; e < c.nent; e += 256) {
    double v = 0.0;
    for (int ch = 0; ch < nch; ++ch) v += part[(int64_t)ch * c.nent + e];
    out[e] = cnt >= 0 ? v : NAN;
  }
}

// The solver's state of one wavefront in LDS (rc_ls_solver_doubles).
struct LsState {
  double *G, *G0, *L, *cov, *cov0, *sign, *ls, *corr, *idx, *act, *ka, *kc;
};

__host__ __device__ inline LsState ls_state(double* base, int p, int kcap) {
  LsState s;
  s.G = base; s.G0 = s.G + p * p; s.L = s.G0 + p * p;
  s.cov = s.L + p * p; s.cov0 = s.cov + p; s.sign = s.cov0 + p; s.ls = s.sign + p; s.corr = s.ls + p;
  s.idx = s.corr + p; s.act = s.idx + p; s.ka = s.act + p; s.kc = s.ka + kcap;
  return s;
}

// Sums of the rows outside fold `skip` (skip < 0: of all rows) into the centred Gram matrix and Cov of target j: the
// folds' sums in fold order, then sum z z^T - s s^T / n.  All lanes; returns the row count (0 with a non-finite sum).
__device__ inline int ls_build(const LsCtx& c, const double* fsum, int j, int skip, const LsState& st, int lane) {
  const int p = c.N, nent = c.nent, ntri = c.ntri;
  double nn = 0.0;
  for (int g = 0; g < c.cv; ++g)
    if (g != skip) nn += fsum[(int64_t)g * nent];
  int bad = !ls_finite(nn) || !(nn > 0.0);
  for (int e = lane; e < p * p + p; e += 64) {
    double szz = 0.0, si = 0.0, sk = 0.0;
    const bool mat = e < p * p;
    const int i = mat ? e / p : e - p * p, k = mat ? e - i * p : 0;
    const int ezz = mat ? ls_tri(1 + i, 1 + k) : ntri + (1 + i) * p + j;
    const int ek = mat ? ls_tri(0, 1 + k) : ntri + j;
    for (int g = 0; g < c.cv; ++g) {
      if (g == skip) continue;
      const double* F = fsum + (int64_t)g * nent;
      szz += F[ezz];
      si += F[ls_tri(0, 1 + i)];
      sk += F[ek];
    }
    const double v = szz - si * sk / nn;
    if (!ls_finite(v)) bad = 1;
    if (mat) {
      st.G[e] = v;
      st.G0[e] = v;
    } else {
      st.cov[i] = v;
      st.cov0[i] = v;
    }
  }
  bad = __any(bad);
  ls_wave_sync();
  return bad ? 0 : (int)nn;
}

__host__ __device__ inline double ls_min_pos(double best, double v) { return (v > 0.0 && v < best) ? v : best; }

__host__ __device__ inline void ls_swap_rc(double* G, int p, int a, int b) {
  if (a == b) return;
  for (int k = 0; k < p; ++k) { const double t = G[a * p + k]; G[a * p + k] = G[b * p + k]; G[b * p + k] = t; }
  for (int k = 0; k < p; ++k) { const double t = G[k * p + a]; G[k * p + a] = G[k * p + b]; G[k * p + b] = t; }
}

// sklearn's _lars_path_solver(method="lasso") on the Gram matrix in st, one lane.  Returns the flags; *nk = knots.
__host__ __device__ int ls_path(const LsState& st, int p, int kcap, double n_samples, double alpha_min, int* nk) {
  double *G = st.G, *L = st.L, *cov = st.cov, *sign = st.sign, *ls = st.ls, *corr = st.corr, *ka = st.ka, *kc = st.kc;
  int n_iter = 0, n_act = 0, flags = 0;
  bool drop = false;
  for (int i = 0; i < p; ++i) { st.idx[i] = (double)i; kc[i] = 0.0; sign[i] = 0.0; }
  ka[0] = 0.0;
  for (;;) {
    double C = 0.0, C_ = 0.0;
    int C_idx = 0;
    if (n_act < p) {
      double best = -1.0;
      for (int k = n_act; k < p; ++k) {
        const double a = fabs(cov[k]);
        if (a > best) { best = a; C_idx = k - n_act; }
      }
      C_ = cov[n_act + C_idx];
      C = fabs(C_);
    }
    if (!ls_finite(C)) { flags |= LS_F_NONFINITE; break; }
    double* coef = kc + n_iter * p;
    const double* prev = kc + (n_iter > 0 ? n_iter - 1 : 0) * p;
    const double prev_alpha = n_iter > 0 ? ka[n_iter - 1] : 0.0;
    const double alpha = C / n_samples;
    ka[n_iter] = alpha;
    if (alpha <= alpha_min + LS_EQ_TOL) {   // early stopping
      if (fabs(alpha - alpha_min) > LS_EQ_TOL) {
        if (n_iter > 0) {
          const double ss = (prev_alpha - alpha_min) / (prev_alpha - alpha);
          for (int i = 0; i < p; ++i) coef[i] = prev[i] + ss * (coef[i] - prev[i]);
        }
        ka[n_iter] = alpha_min;
      }
      break;
    }
    if (n_iter >= LS_MAX_ITER || n_act >= p) break;
    if (!drop) {
      sign[n_act] = C_ > 0.0 ? 1.0 : (C_ < 0.0 ? -1.0 : 0.0);
      const int m = n_act, n = C_idx + n_act;
      { const double t = cov[n]; cov[n] = cov[m]; cov[m] = t; }
      { const double t = st.idx[n]; st.idx[n] = st.idx[m]; st.idx[m] = t; }
      ls_swap_rc(G, p, m, n);
      const double cc = G[n_act * p + n_act];
      for (int i = 0; i < n_act; ++i) {
        double v = G[n_act * p + i];
        for (int k = 0; k < i; ++k) v -= L[i * p + k] * L[n_act * p + k];
        L[n_act * p + i] = v / L[i * p + i];
      }
      double v = 0.0;
      for (int k = 0; k < n_act; ++k) v += L[n_act * p + k] * L[n_act * p + k];
      double diag = sqrt(fabs(cc - v));
      diag = diag > LS_EPS ? diag : LS_EPS;
      L[n_act * p + n_act] = diag;
      if (diag < 1e-7) { flags |= LS_F_DROP_FOR_GOOD; break; }
      st.act[n_act] = st.idx[n_act];
      ++n_act;
    }
    if (n_iter > 0 && prev_alpha < alpha) { flags |= LS_F_ALPHA_UP; break; }
    // least squares solution: L L^T ls = sign
    for (int i = 0; i < n_act; ++i) {
      double v = sign[i];
      for (int k = 0; k < i; ++k) v -= L[i * p + k] * ls[k];
      ls[i] = v / L[i * p + i];
    }
    for (int i = n_act - 1; i >= 0; --i) {
      double v = ls[i];
      for (int k = i + 1; k < n_act; ++k) v -= L[k * p + i] * ls[k];
      ls[i] = v / L[i * p + i];
    }
    double AA;
    if (n_act == 1 && ls[0] == 0.0) {
      ls[0] = 1.0;
      AA = 1.0;
    } else {
      double t = 0.0;
      for (int i = 0; i < n_act; ++i) t += ls[i] * sign[i];
      AA = 1.0 / sqrt(t);
      if (!ls_finite(AA)) { flags |= LS_F_AA; break; }
      for (int i = 0; i < n_act; ++i) ls[i] *= AA;
    }
    double g1 = LS_DBL_MAX, g2 = LS_DBL_MAX;
    for (int k = n_act; k < p; ++k) {
      double v = 0.0;
      for (int i = 0; i < n_act; ++i) v += G[i * p + k] * ls[i];
      v = rint(v * 1e15) / 1e15;   // np.around(corr_eq_dir, 15)
      corr[k] = v;
      g1 = ls_min_pos(g1, (C - cov[k]) / (AA - v + LS_TINY32));
      g2 = ls_min_pos(g2, (C + cov[k]) / (AA + v + LS_TINY32));
    }
    double gamma = g1 < g2 ? g1 : g2;
    gamma = gamma < C / AA ? gamma : C / AA;
    drop = false;
    double z_pos = LS_DBL_MAX;
    for (int i = 0; i < n_act; ++i) z_pos = ls_min_pos(z_pos, -coef[(int)st.act[i]] / (ls[i] + LS_TINY32));
    int ii = -1;
    if (z_pos < gamma) {   // a coefficient changes sign
      int hits = 0;
      for (int i = 0; i < n_act; ++i)
        if (-coef[(int)st.act[i]] / (ls[i] + LS_TINY32) == z_pos) { ii = i; ++hits; }
      if (hits != 1) { flags |= LS_F_MULTI_DROP; break; }
      sign[ii] = -sign[ii];
      gamma = z_pos;
      drop = true;
    }
    ++n_iter;
    if (n_iter >= kcap) { flags |= LS_F_KNOTS; break; }
    prev = coef;
    coef = kc + n_iter * p;
    for (int i = 0; i < p; ++i) coef[i] = 0.0;
    for (int i = 0; i < n_act; ++i) coef[(int)st.act[i]] = prev[(int)st.act[i]] + gamma * ls[i];
    for (int k = n_act; k < p; ++k) cov[k] -= gamma * corr[k];
    if (drop) {
      // cholesky_delete(L[:n_act, :n_act], ii)
      for (int i = ii; i < n_act - 1; ++i)
        for (int k = 0; k < i + 2; ++k) L[i * p + k] = L[(i + 1) * p + k];
      for (int i = ii; i < n_act - 1; ++i) {
        const double a = L[i * p + i], b = L[i * p + i + 1];
        const double roe = fabs(a) > fabs(b) ? a : b, scale = fabs(a) + fabs(b);
        double r = 0.0, cs = 1.0, sn = 0.0;
        if (scale != 0.0) {
          r = scale * sqrt((a / scale) * (a / scale) + (b / scale) * (b / scale));
          if (roe < 0.0) r = -r;
          cs = a / r;
          sn = b / r;
        }
        if (r < 0.0) { r = -r; cs = -cs; sn = -sn; }
        L[i * p + i] = r;
        L[i * p + i + 1] = 0.0;
        for (int k = i + 1; k < n_act - 1; ++k) {
          const double xk = L[k * p + i], yk = L[k * p + i + 1];
          L[k * p + i] = cs * xk + sn * yk;
          L[k * p + i + 1] = cs * yk - sn * xk;
        }
      }
      --n_act;
      const int drop_idx = (int)st.act[ii];
      for (int i = ii; i < n_act; ++i) {
        st.act[i] = st.act[i + 1];
        sign[i] = sign[i + 1];
        { const double t = st.idx[i]; st.idx[i] = st.idx[i + 1]; st.idx[i + 1] = t; }
        ls_swap_rc(G, p, i, i + 1);
      }
      sign[n_act] = 0.0;
      double t = 0.0;
      for (int k = 0; k < p; ++k) t += st.G0[drop_idx * p + k] * coef[k];
      cov[n_act] = st.cov0[drop_idx] - t;
    }
  }
  for (int k = 1; k <= n_iter && !flags; ++k)
    if (ka[k] > ka[k - 1]) flags |= LS_F_ORDER;
  *nk = n_iter + 1;
  return flags;
}

__global__ __launch_bounds__(64 * LS_WPW_PATH) void k_ls_path(LsCtx c) {
  extern __shared__ __attribute__((aligned(16))) char ls_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t w64 = (int64_t)blockIdx.x * LS_WPW_PATH + wave;
  if (w64 >= (int64_t)c.P * c.S * c.N * c.cv) return;   // no workgroup barrier below: the waves are independent
  const int w = (int)w64, p = c.N, kcap = c.kcap;
  const int f = w % c.cv, j = (w / c.cv) % p, q = w / (c.cv * p);
  const LsState st = ls_state(reinterpret_cast<double*>(ls_smem) + (size_t)wave * rc_ls_solver_doubles(p), p, kcap);
  bool all;
  const int cnt = ls_count(c, q, &all);
  int flags = 0, nk = 0;
  if (cnt < 0) {
    flags = LS_F_NONFINITE;
  } else {
    const int ntr = ls_build(c, c.fsum + (int64_t)q * c.cv * c.nent, j, f, st, lane);
    if (ntr == 0) flags = LS_F_NONFINITE;
    else if (ntr <= p) flags = LS_F_XROUTE;
    else if (lane == 0) flags = ls_path(st, p, kcap, (double)ntr, 0.0, &nk);
  }
  ls_wave_sync();
  flags = __shfl(flags, 0) | (cnt < 0 ? LS_F_NONFINITE : 0);
  nk = __shfl(nk, 0);
  if (flags) nk = 0;
  double* ka = c.kn_alpha + (int64_t)w * kcap;
  double* kc = c.kn_coef + (int64_t)w * kcap * p;
  for (int e = lane; e < nk; e += 64) ka[e] = st.ka[e];
  for (int e = lane; e < nk * p; e += 64) kc[e] = st.kc[e];
  if (lane == 0) {
    c.kn_meta[2 * (int64_t)w] = nk;
    c.kn_meta[2 * (int64_t)w + 1] = flags;
  }
}

__global__ __launch_bounds__(64 * LS_WPW_SEL) void k_ls_select(LsCtx c) {
  extern __shared__ __attribute__((aligned(16))) char ls_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t t64 = (int64_t)blockIdx.x * LS_WPW_SEL + wave;
  if (t64 >= (int64_t)c.P * c.S * c.N) return;
  const int tr = (int)t64, p = c.N, kcap = c.kcap, cv = c.cv, nent = c.nent, ntri = c.ntri;
  const int j = tr % p, q = tr / p;
  double* base = reinterpret_cast<double*>(ls_smem) + (size_t)wave * rc_ls_select_doubles(p, cv);
  const LsState st = ls_state(base, p, kcap);
  double* al = base + rc_ls_solver_doubles(p);   // merged alphas
  double* un = al + cv * kcap;                   // unique, ascending
  double* er = un + cv * kcap;                   // first-occurrence marks, then the mean squared errors
  double* fs = er + cv * kcap;                   // per fold: n_test, n_train, dy, dz [p]
  const double* fsum = c.fsum + (int64_t)q * cv * nent;
  const int32_t* meta = c.kn_meta + 2 * (int64_t)tr * cv;
  const double* kna = c.kn_alpha + (int64_t)tr * cv * kcap;
  const double* knc = c.kn_coef + (int64_t)tr * cv * kcap * p;

  int flags = 0, M = 0;
  for (int f = 0; f < cv; ++f) {
    flags |= meta[2 * f + 1];
    M += meta[2 * f];
  }
  int status = REDCLIFF_TIDYBENCH_OK, best_i = 0, sel = 0;
  double best_a = 0.0, ratio = INFINITY;
  double* coef_out = c.coef + (int64_t)tr * p;
  if (lane == 0)
    for (int e = 0; e < p; ++e) coef_out[e] = 0.0;

  if (!flags) {
    // the folds' alphas, np.unique by rank counting
    int off = 0;
    for (int f = 0; f < cv; ++f) {
      const int K = meta[2 * f];
      for (int e = lane; e < K; e += 64) al[off + e] = kna[f * kcap + e];
      off += K;
    }
    ls_wave_sync();
    for (int e = lane; e < M; e += 64) {
      const double a = al[e];
      bool first = true;
      for (int k = 0; k < e; ++k) first = first && al[k] != a;
      er[e] = first ? 1.0 : 0.0;
    }
    ls_wave_sync();
    int Mu = 0;
    for (int k = 0; k < M; ++k) Mu += er[k] != 0.0;
    for (int e = lane; e < M; e += 64) {
      if (er[e] == 0.0) continue;
      const double a = al[e];
      int rank = 0;
      for (int k = 0; k < M; ++k) rank += (er[k] != 0.0 && al[k] < a);
      un[rank] = a;
    }
    // per fold: the test and training row counts and the training means
    for (int e = lane; e < cv * (p + 1); e += 64) {
      const int f = e / (p + 1), i = e - f * (p + 1);   // i == p: the target
      const int ent = i < p ? ls_tri(0, 1 + i) : ntri + j;
      double ntr = 0.0, s = 0.0;
      for (int g = 0; g < cv; ++g) {
        if (g == f) continue;
        ntr += fsum[(int64_t)g * nent];
        s += fsum[(int64_t)g * nent + ent];
      }
      if (i < p) {
        fs[f * (p + 3) + 3 + i] = s / ntr;
      } else {
        fs[f * (p + 3) + 2] = s / ntr;
        fs[f * (p + 3) + 1] = ntr;
        fs[f * (p + 3)] = fsum[(int64_t)f * nent];
      }
    }
    ls_wave_sync();
    const double amax = un[Mu - 1];
    int bad_pad = 0;
    for (int u = lane; u < Mu; u += 64) {
      const double a = un[u];
      double tot = 0.0;
      bool fin = true;
      for (int f = 0; f < cv; ++f) {
        const int K = meta[2 * f];
        const double* xa = kna + f * kcap;
        const double* xc = knc + (int64_t)f * kcap * p;
        const int pre = xa[K - 1] != 0.0 ? 1 : 0, post = xa[0] != amax ? 1 : 0, Lp = pre + K + post;
        if (Lp < 2) { bad_pad = 1; continue; }
        // padded ascending knots: t < pre: (0, last knot); t < pre + K: knot K - 1 - (t - pre); else (amax, knot 0)
        int hi = 0;
        for (int t = 0; t < Lp; ++t) {
          const double x = t < pre ? 0.0 : (t < pre + K ? xa[K - 1 - (t - pre)] : amax);
          hi += x < a;
        }
        hi = hi < 1 ? 1 : (hi > Lp - 1 ? Lp - 1 : hi);
        const int lo = hi - 1;
        const double xl = lo < pre ? 0.0 : (lo < pre + K ? xa[K - 1 - (lo - pre)] : amax);
        const double xh = hi < pre ? 0.0 : (hi < pre + K ? xa[K - 1 - (hi - pre)] : amax);
        const double* cl = xc + (lo < pre ? K - 1 : (lo < pre + K ? K - 1 - (lo - pre) : 0)) * p;
        const double* ch = xc + (hi < pre ? K - 1 : (hi < pre + K ? K - 1 - (hi - pre) : 0)) * p;
        const double dx = xh - xl, da = a - xl;
        const double* F = fsum + (int64_t)f * nent;
        const double* fm = fs + f * (p + 3);
        double q1 = 0.0, q2 = 0.0, lin = 0.0, k0 = 0.0;
        for (int i = 0; i < p; ++i) {
          const double ci = (ch[i] - cl[i]) / dx * da + cl[i];
          double r = 0.0;
          for (int k = 0; k < p; ++k) r += ((ch[k] - cl[k]) / dx * da + cl[k]) * F[ls_tri(1 + i, 1 + k)];
          q1 += ci * r;
          q2 += ci * F[ntri + (1 + i) * p + j];
          lin += ci * F[ls_tri(0, 1 + i)];
          k0 += ci * fm[3 + i];
        }
        lin -= F[ntri + j];
        k0 -= fm[2];
        const double sse = q1 - 2.0 * q2 + F[ntri + (1 + p) * p + j] - 2.0 * k0 * lin + fm[0] * k0 * k0;
        const double mse = sse / fm[0];
        fin = fin && ls_finite(mse);
        tot += mse;
      }
      er[u] = fin ? tot / (double)cv : NAN;
    }
    if (__any(bad_pad)) flags |= LS_F_AA;
    ls_wave_sync();
    if (!flags) {
      double best = INFINITY;
      int nfin = 0;
      best_i = -1;
      for (int u = 0; u < Mu; ++u) {
        const double v = er[u];
        if (!ls_finite(v)) continue;
        if (v < best) { best = v; best_i = nfin; best_a = un[u]; }
        ++nfin;
      }
      if (best_i < 0) flags |= LS_F_AA;
    }
  }
  // the final path on all rows, down to the best alpha
  int nk = 0;
  if (!flags) {
    const int nall = ls_build(c, fsum, j, -1, st, lane);
    if (nall == 0) flags |= LS_F_NONFINITE;
    else if (nall <= p) flags |= LS_F_XROUTE;
    else if (lane == 0) flags = ls_path(st, p, kcap, (double)nall, best_a, &nk);
    ls_wave_sync();
    flags = __shfl(flags, 0);
    nk = __shfl(nk, 0);
  }
  if (!flags) {
    // positive coefficients, refitted on the uncentred, unshifted columns: sum (z + mu)(z + mu)^T from the sums
    const double* cf = st.kc + (nk - 1) * p;
    int map[LS_NMAX];
    int ns = 0;
    for (int i = 0; i < p; ++i)
      if (cf[i] > 0.0) { sel |= 1 << i; map[ns++] = i; }
    const double* mu = c.means + (int64_t)(q / c.S) * p;
    double nn = 0.0;
    for (int g = 0; g < cv; ++g) nn += fsum[(int64_t)g * nent];
    double* A = st.G;     // [ns][ns], then its factor
    double* rhs = st.cov;
    double* dg = st.corr;
    ls_wave_sync();
    for (int e = lane; e < ns * ns + ns; e += 64) {
      const bool mat = e < ns * ns;
      const int a = mat ? e / ns : e - ns * ns, b = mat ? e - a * ns : 0;
      const int i = map[a], k = mat ? map[b] : 0;
      const int ezz = mat ? ls_tri(1 + i, 1 + k) : ntri + (1 + i) * p + j;
      const int ek = mat ? ls_tri(0, 1 + k) : ntri + j;
      const double mk = mat ? mu[k] : mu[j];
      double szz = 0.0, si = 0.0, sk = 0.0;
      for (int g = 0; g < cv; ++g) {
        const double* F = fsum + (int64_t)g * nent;
        szz += F[ezz];
        si += F[ls_tri(0, 1 + i)];
        sk += F[ek];
      }
      const double v = szz + mu[i] * sk + mk * si + nn * mu[i] * mk;
      if (mat) A[e] = v; else rhs[a] = v;
    }
    ls_wave_sync();
    if (lane == 0 && ns > 0) {   // the right-looking recurrence of _pivot_cholesky, then U^T w = r, U b = w
      for (int a = 0; a < ns; ++a) dg[a] = A[a * ns + a];
      for (int a = 0; a < ns; ++a) {
        const double piv = A[a * ns + a], g = dg[a];
        if (!ls_finite(piv) || !ls_finite(g)) { status = REDCLIFF_TIDYBENCH_NONFINITE; break; }
        if (!(g > 0.0) || !(piv > 0.0)) { status = REDCLIFF_TIDYBENCH_SINGULAR; ratio = g > 0.0 ? piv / g : 0.0; break; }
        const double r = piv / g;
        ratio = r < ratio ? r : ratio;
        if (r < TB_PIVOT_MIN) { status = REDCLIFF_TIDYBENCH_SINGULAR; break; }
        const double d = sqrt(piv);
        A[a * ns + a] = d;
        for (int b = a + 1; b < ns; ++b) A[a * ns + b] /= d;
        for (int b1 = a + 1; b1 < ns; ++b1)
          for (int b2 = b1; b2 < ns; ++b2) A[b1 * ns + b2] -= A[a * ns + b1] * A[a * ns + b2];
      }
      if (status == REDCLIFF_TIDYBENCH_OK) {
        for (int a = 0; a < ns; ++a) {
          double v = rhs[a];
          for (int b = 0; b < a; ++b) v -= A[b * ns + a] * rhs[b];
          rhs[a] = v / A[a * ns + a];
        }
        for (int a = ns - 1; a >= 0; --a) {
          double v = rhs[a];
          for (int b = a + 1; b < ns; ++b) v -= A[a * ns + b] * rhs[b];
          rhs[a] = v / A[a * ns + a];
        }
        for (int a = 0; a < ns; ++a) coef_out[map[a]] = rhs[a];
      }
    }
    status = __shfl(status, 0);
    ratio = __shfl(ratio, 0);
  }
  if (flags) status = (flags & LS_F_NONFINITE) ? REDCLIFF_TIDYBENCH_NONFINITE : REDCLIFF_LASAR_DEGENERATE;
  if (lane == 0) {
    c.status[tr] = status;
    c.pivot[tr] = ratio;
    c.best_alpha[tr] = best_a;
    c.best_index[tr] = best_i;
    c.selected[tr] = sel;
  }
}

using LsGramKern = void (*)(LsCtx);

int ls_ctx(int32_t P, int32_t S, int32_t T, int32_t N, int32_t lags, int32_t cv, int32_t max_count, LsCtx* c) {
  memset(c, 0, sizeof(*c));
  if (P < 0 || S < 0 || N < 1 || lags < 1 || T <= lags || cv < 2 || max_count < 0) {
    rc_set_error("lasar: bad arguments (P=%d S=%d T=%d N=%d lags=%d cv=%d max_count=%d)", P, S, T, N, lags, cv, max_count);
    return REDCLIFF_EINVAL;
  }
  if (N > LS_NMAX || lags != 1 || cv > LS_CVMAX || P > 65535 || S > 65535 ||
      (int64_t)P * S * N * cv > (int64_t)1 << 30) {
    rc_set_error("lasar: outside kernel limits (N <= %d, lags == 1, cv <= %d, P and S <= 65535, P S N cv <= 2^30; N=%d lags=%d "
                 "cv=%d P=%d S=%d)", LS_NMAX, LS_CVMAX, N, lags, cv, P, S);
    return REDCLIFF_ELIMIT;
  }
  c->P = P; c->S = S; c->T = T; c->N = N; c->cv = cv; c->n = T - lags; c->max_count = max_count;
  c->ntri = rc_tb_ntri(N, 1); c->nent = rc_ls_nent(N); c->maxchf = rc_ls_maxchf(max_count, cv); c->kcap = rc_ls_kcap(N);
  return 0;
}

size_t ls_align(size_t b) { return (b + 15) & ~(size_t)15; }

struct LsLayout { size_t means, part, fsum, kn_alpha, kn_coef, kn_meta, total; };

LsLayout ls_layout(const LsCtx& c) {
  LsLayout l;
  const size_t q = (size_t)c.P * c.S, paths = q * c.N * c.cv;
  size_t o = 0;
  l.means = o; o += ls_align(sizeof(double) * (size_t)c.P * c.N);
  l.part = o; o += ls_align(sizeof(double) * q * c.cv * (size_t)c.maxchf * c.nent);
  l.fsum = o; o += ls_align(sizeof(double) * q * c.cv * c.nent);
  l.kn_alpha = o; o += ls_align(sizeof(double) * paths * c.kcap);
  l.kn_coef = o; o += ls_align(sizeof(double) * paths * c.kcap * c.N);
  l.kn_meta = o; o += ls_align(sizeof(int32_t) * paths * 2);
  l.total = o + 16;
  return l;
}

}  // namespace

extern "C" {

int redcliff_lasar_supported(int32_t T, int32_t N, int32_t lags) {
  LsCtx c;
  return ls_ctx(1, 1, T, N, lags, 5, 0, &c) == 0 ? 1 : 0;
}

size_t redcliff_lasar_ws_bytes(int32_t P, int32_t S, int32_t N, int32_t lags, int32_t cv, int32_t max_count) {
  LsCtx c;
  if (ls_ctx(P, S, lags + 1, N, lags, cv, max_count, &c) != 0) return 0;
  return ls_layout(c).total;
}

int redcliff_lasar_run(const RedcliffLasarArgs* a, void* stream) {
  if (!a) { rc_set_error("null lasar arguments"); return REDCLIFF_EINVAL; }
  LsCtx c;
  int e = ls_ctx(a->P, a->S, a->T, a->N, a->lags, a->cv, a->max_count, &c);
  if (e) return e;
  if (a->P == 0 || a->S == 0) return 0;
  if (!a->data || !a->count || !a->coef || !a->best_alpha || !a->best_index || !a->selected || !a->status || !a->pivot_ratio ||
      !a->ws || (a->max_count > 0 && !a->idx)) {
    rc_set_error("lasar_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->idx_fstride < 0 || a->idx_pstride < 0 || (a->S > 1 && a->idx_fstride < a->max_count && a->idx_fstride != 0)) {
    rc_set_error("lasar_run: bad strides (idx_fstride=%lld idx_pstride=%lld max_count=%d)", (long long)a->idx_fstride,
                 (long long)a->idx_pstride, a->max_count);
    return REDCLIFF_EINVAL;
  }
  const LsLayout l = ls_layout(c);
  if (a->ws_bytes < l.total) { rc_set_error("lasar_run: workspace too small: %zu < %zu", a->ws_bytes, l.total); return REDCLIFF_EWORKSPACE; }
  if ((reinterpret_cast<uintptr_t>(a->ws) & 15) != 0) { rc_set_error("lasar_run: workspace not 16-byte aligned"); return REDCLIFF_EINVAL; }
  c.idx_pstride = a->idx_pstride; c.idx_fstride = a->idx_fstride;
  c.data = a->data; c.idx = a->idx; c.count = a->count;
  c.coef = a->coef; c.best_alpha = a->best_alpha; c.best_index = a->best_index; c.selected = a->selected;
  c.status = a->status; c.pivot = a->pivot_ratio;
  char* ws = static_cast<char*>(a->ws);
  c.means = reinterpret_cast<double*>(ws + l.means);
  c.part = reinterpret_cast<double*>(ws + l.part);
  c.fsum = reinterpret_cast<double*>(ws + l.fsum);
  c.kn_alpha = reinterpret_cast<double*>(ws + l.kn_alpha);
  c.kn_coef = reinterpret_cast<double*>(ws + l.kn_coef);
  c.kn_meta = reinterpret_cast<int32_t*>(ws + l.kn_meta);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_ls_means, dim3(c.P), dim3(256), 0, s, c);
  if ((e = rc_check(hipGetLastError(), "k_ls_means"))) return e;
  if (c.maxchf > 0) {
    if ((int64_t)c.maxchf * c.cv > 0x7fffffff) { rc_set_error("lasar_run: too many chunks"); return REDCLIFF_ELIMIT; }
    const int per = (c.nent + TB_THREADS - 1) / TB_THREADS;
    LsGramKern k = per <= 1 ? k_ls_gram<1> : per <= 2 ? k_ls_gram<2> : k_ls_gram<4>;
    hipLaunchKernelGGL(k, dim3((unsigned)(c.maxchf * c.cv), (unsigned)c.S, (unsigned)c.P), dim3(TB_THREADS),
                       sizeof(double) * TB_TR * (1 + 2 * c.N), s, c);
    if ((e = rc_check(hipGetLastError(), "k_ls_gram"))) return e;
  }
  hipLaunchKernelGGL(k_ls_fold, dim3((unsigned)c.cv, (unsigned)c.S, (unsigned)c.P), dim3(256), 0, s, c);
  if ((e = rc_check(hipGetLastError(), "k_ls_fold"))) return e;
  const int64_t npath = (int64_t)c.P * c.S * c.N * c.cv, ntrip = (int64_t)c.P * c.S * c.N;
  hipLaunchKernelGGL(k_ls_path, dim3((unsigned)((npath + LS_WPW_PATH - 1) / LS_WPW_PATH)), dim3(64 * LS_WPW_PATH),
                     sizeof(double) * LS_WPW_PATH * rc_ls_solver_doubles(c.N), s, c);
  if ((e = rc_check(hipGetLastError(), "k_ls_path"))) return e;
  hipLaunchKernelGGL(k_ls_select, dim3((unsigned)((ntrip + LS_WPW_SEL - 1) / LS_WPW_SEL)), dim3(64 * LS_WPW_SEL),
                     sizeof(double) * LS_WPW_SEL * rc_ls_select_doubles(c.N, c.cv), s, c);
  if ((e = rc_check(hipGetLastError(), "k_ls_select"))) return e;
  return 0;
}

}  // extern "C"
