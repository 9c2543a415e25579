// rc_dynotears.hip -- the DYNOTEARS comparison baseline (models/causalnex_dynotears_vanilla.py of the reference):
// P independent augmented-Lagrangian solves, one per recording (and per lambda), advanced together.
//
// A problem has nv = 2 (p + 1) d^2 variables wa >= 0 (W+, W-, then per lag A+, A-), some fixed at 0, and
//   f(wa) = 0.5/n ||X (I - W) - Xlags A||_F^2 + 0.5 rho h^2 + alpha h + lambda_w sum wa[:2 d^2] + lambda_a sum wa[2 d^2:],
//   h = tr expm(W o W) - d.
//
//   k_dy_gram   (problem)  S = Z^T Z, Z = [X | Xlags], in double: one lane per entry sums the rows in row order.  A
//        non-finite entry ends the problem as NONFINITE.  Also resets the problem's solver state.
//   k_dy_solve  (problem)  one wavefront per problem advances it by at most evals_per_launch evaluations of (f, grad f):
//        with B = [I - W; -A] the loss is 0.5/n sum B o (S B) and its gradient blocks are -(1/n) S B; the d x d matrix
//        exponential is scaling and squaring around a degree-12 Taylor polynomial (all terms are non-negative, so there
//        is no cancellation).  The inner solver is a limited-memory projected quasi-Newton method for the bounds
//        "== 0" and ">= 0": the two-loop recursion over the history pairs restricted to the free variables, a scaled
//        gradient step on variables within eps of their bound whose gradient pushes them onto it, and a backtracking
//        search along the projected arc P(x + t dir) that accepts on sufficient decrease (1e-3) or, once the decrease
//        is below the rounding of f, on the approximate Wolfe conditions.  It stops by L-BFGS-B's rules (relative
//        decrease <= factr eps, projected-gradient infinity norm <= pgtol, maxiter, maxfun, maxls).  A non-finite
//        trial value counts as larger than any finite one: the step shrinks, x never becomes non-finite.  The outer
//        loop (rho x10 while h does not fall to a quarter, alpha += rho h) runs in the same kernel; every inner solve
//        starts from wa_est with empty history, as the reference does.
//
// All state lives in the workspace between launches and is reloaded bit for bit, every reduction is an xor butterfly
// over the lanes' strided partial sums (the same order every time), and every branch is taken on a value all lanes
// hold alike, so the result does not depend on evals_per_launch or on the rest of the batch.  The history pairs stay
// in global memory (2 m nv doubles, 64 KB at nv 400); the iterate, gradient, direction, trial point and the small
// matrices are in LDS (40,832 bytes, sized for the limits: three to four workgroups per CU).
#include <cmath>
#include <cstring>

#include "rc_dynotears.h"

namespace {

__device__ inline double dy_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return __shfl(v, 0);
}

__device__ inline double dy_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return __shfl(v, 0);
}

struct DyLds {
  double x[DY_NVMAX], g[DY_NVMAX], dir[DY_NVMAX], xt[DY_NVMAX], gt[DY_NVMAX];
  double S[DY_QMAX * DY_QMAX];
  double B[DY_QMAX * DY_DMAX], SB[DY_QMAX * DY_DMAX];
  double Wm[DY_DMAX * DY_DMAX], Ms[DY_DMAX * DY_DMAX], E0[DY_DMAX * DY_DMAX], E1[DY_DMAX * DY_DMAX];
  double al[DY_MMAX], sy[DY_MMAX];
  uint8_t cls[DY_NVMAX];   // 0 fixed, 1 near its bound and pushed onto it, 2 free
  uint8_t fixed[DY_NVMAX];
};

template <typename T>
__global__ __launch_bounds__(256) void k_dy_gram(DyCtx c) {
  const int b = blockIdx.x;
  const int d = c.d, q = c.q, pd = c.p * c.d, nv = c.nv;
  double* ws = c.ws + (size_t)b * c.slice;
  double* S = ws + rc_dy_off_S();
  const T* X = static_cast<const T*>(c.X) + (int64_t)b * c.x_ps;
  const T* Xl = static_cast<const T*>(c.Xl) + (int64_t)b * c.xl_ps;
  const int n = c.n_rows[b];
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < q * q; e += blockDim.x) {
    const int i = e / q, j = e - i * q;
    const T* ci = i < d ? X + i : Xl + (i - d);
    const T* cj = j < d ? X + j : Xl + (j - d);
    const int64_t si = i < d ? c.x_rs : c.xl_rs, sj = j < d ? c.x_rs : c.xl_rs;
    double acc = 0.0;
    for (int r = 0; r < n; ++r) acc = fma((double)ci[r * si], (double)cj[r * sj], acc);
    S[e] = acc;
    if (!isfinite(acc)) bad = 1;
  }
  double* vec = ws + rc_dy_off_vec(d, c.p);
  for (int i = threadIdx.x; i < 4 * nv; i += blockDim.x) vec[i] = 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    DyState st;
    memset(&st, 0, sizeof(st));
    st.rho = c.rho0; st.alpha = c.alpha0;
    st.h_value = INFINITY; st.h_new = INFINITY;
    st.phase = DY_PH_START;
    if (bad || n < 1) { st.done = 1; st.status = REDCLIFF_DYNOTEARS_NONFINITE; }
    *reinterpret_cast<DyState*>(ws) = st;
  }
  if (bad || n < 1) {
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x; i < d * d; i += blockDim.x) c.W[(size_t)b * d * d + i] = nan;
    for (int i = threadIdx.x; i < pd * d; i += blockDim.x) c.A[(size_t)b * pd * d + i] = nan;
    if (c.wa) for (int i = threadIdx.x; i < nv; i += blockDim.x) c.wa[(size_t)b * nv + i] = nan;
    if (threadIdx.x == 0) {
      c.status[b] = REDCLIFF_DYNOTEARS_NONFINITE;
      for (int k = 0; k < 6; ++k) { c.stats[(size_t)b * 6 + k] = nan; c.counts[(size_t)b * 6 + k] = 0; }
    }
  }
}

// C = A B for d x d matrices in LDS; lane-owned entries, k in order
__device__ inline void dy_matmul(const double* A, const double* Bm, double* C, int d, int lane, double scale, bool add_eye) {
  for (int e = lane; e < d * d; e += DY_THREADS) {
    const int i = e / d, j = e - i * d;
    double acc = 0.0;
    for (int k = 0; k < d; ++k) acc = fma(A[i * d + k], Bm[k * d + j], acc);
    acc *= scale;
    C[e] = add_eye && i == j ? acc + 1.0 : acc;
  }
}

// f and grad f at L.xt into L.gt; returns f (non-finite when anything overflowed) and h
__device__ double dy_eval(DyLds& L, const DyCtx& c, double ninv, double rho, double alpha, double lw, double la, int lane, double* h_out) {
  const int d = c.d, p = c.p, q = c.q, nv = c.nv, dd = d * d;
  double l1w = 0.0, l1a = 0.0;
  for (int e = lane; e < dd; e += DY_THREADS) {
    const int i = e / d, j = e - i * d;
    const double w = L.xt[e] - L.xt[dd + e];
    L.Wm[e] = w;
    L.Ms[e] = w * w;
    L.B[e] = (i == j ? 1.0 : 0.0) - w;
  }
  for (int e = lane; e < p * dd; e += DY_THREADS) {
    const int k = e / dd, r = e - k * dd;
    L.B[dd + e] = -(L.xt[2 * dd + 2 * k * dd + r] - L.xt[2 * dd + 2 * k * dd + dd + r]);
  }
  for (int i = lane; i < nv; i += DY_THREADS) {
    if (i < 2 * dd) l1w += L.xt[i]; else l1a += L.xt[i];
  }
  __syncthreads();
  double loss = 0.0;
  for (int e = lane; e < q * d; e += DY_THREADS) {
    const int r = e / d, col = e - r * d;
    double acc = 0.0;
    for (int k = 0; k < q; ++k) acc = fma(L.S[r * q + k], L.B[k * d + col], acc);
    L.SB[e] = acc;
    loss = fma(L.B[e], acc, loss);
  }
  double cs = 0.0;
  if (lane < d) for (int i = 0; i < d; ++i) cs += L.Ms[i * d + lane];
  const double nrm = dy_max(cs);
  loss = dy_sum(loss);
  l1w = dy_sum(l1w);
  l1a = dy_sum(l1a);
  if (!(nrm < 1e300)) { *h_out = INFINITY; return INFINITY; }
  int s = 0;
  for (double v = nrm; v > 0.25 && s <= DY_SQMAX; v *= 0.5) ++s;
  if (s > DY_SQMAX) { *h_out = INFINITY; return INFINITY; }
  const double sc = ldexp(1.0, -s);
  for (int e = lane; e < dd; e += DY_THREADS) {
    const int i = e / d, j = e - i * d;
    const double a = L.Ms[e] * sc;
    L.Ms[e] = a;
    L.E0[e] = (i == j ? 1.0 : 0.0) + a * (1.0 / DY_TAYLOR);
  }
  __syncthreads();
  double* cur = L.E0;
  double* nxt = L.E1;
  for (int k = DY_TAYLOR - 1; k >= 1; --k) {   // Horner: T <- I + (M T) / k
    dy_matmul(L.Ms, cur, nxt, d, lane, 1.0 / k, true);
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
  for (int k = 0; k < s; ++k) {
    dy_matmul(cur, cur, nxt, d, lane, 1.0, false);
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
  const double h = dy_sum(lane < d ? cur[lane * d + lane] - 1.0 : 0.0);
  const double f = 0.5 * ninv * loss + 0.5 * rho * h * h + alpha * h + lw * l1w + la * l1a;
  const double coef = 2.0 * (rho * h + alpha);
  double bad = 0.0;
  for (int e = lane; e < dd; e += DY_THREADS) {
    const int i = e / d, j = e - i * d;
    const double gw = -ninv * L.SB[e] + coef * cur[j * d + i] * L.Wm[e];
    L.gt[e] = gw + lw;
    L.gt[dd + e] = -gw + lw;
    if (!isfinite(gw)) bad = 1.0;
  }
  for (int e = lane; e < p * dd; e += DY_THREADS) {
    const int k = e / dd, r = e - k * dd;
    const double ga = -ninv * L.SB[dd + e];
    L.gt[2 * dd + 2 * k * dd + r] = ga + la;
    L.gt[2 * dd + 2 * k * dd + dd + r] = -ga + la;
    if (!isfinite(ga)) bad = 1.0;
  }
  bad = dy_sum(bad);
  __syncthreads();
  *h_out = h;
  return bad > 0.0 ? INFINITY : f;
}

// infinity norm of x - P(x - g)
__device__ inline double dy_pgnorm(const DyLds& L, int nv, int lane) {
  double m = 0.0;
  for (int i = lane; i < nv; i += DY_THREADS) {
    if (L.fixed[i]) continue;
    const double g = L.g[i];
    m = fmax(m, g < 0.0 ? -g : fmin(L.x[i], g));
  }
  return dy_max(m);
}

// the search direction at (L.x, L.g) into L.dir; sets st.gd = g . dir (< 0), st.t and st.steep
__device__ void dy_direction(DyLds& L, const DyCtx& c, DyState& st, const double* hs, const double* hy, int lane) {
  const int nv = c.nv, m = c.m;
  const double eps_act = fmin(st.pg, 1e-3);
  for (int i = lane; i < nv; i += DY_THREADS) {
    const uint8_t k = L.fixed[i] ? 0 : (L.x[i] <= eps_act && L.g[i] > 0.0) ? 1 : 2;
    L.cls[i] = k;
    L.dir[i] = k == 2 ? L.g[i] : 0.0;
  }
  __syncthreads();
  // curvature of each pair on the free variables; a pair without positive curvature there sits this iteration out
  double gamma = 0.0;
  int nvalid = 0;
  for (int j = 0; j < st.hist_n; ++j) {
    const int slot = (st.hist_next - st.hist_n + j + m) % m;
    double sy = 0.0, yy = 0.0;
    for (int i = lane; i < nv; i += DY_THREADS) {
      if (L.cls[i] == 2) {
        const double y = hy[(size_t)slot * nv + i];
        sy = fma(hs[(size_t)slot * nv + i], y, sy);
        yy = fma(y, y, yy);
      }
    }
    sy = dy_sum(sy);
    yy = dy_sum(yy);
    const bool ok = sy > 2.2e-16 * yy && yy > 0.0;
    if (lane == 0) L.sy[j] = ok ? sy : 0.0;
    if (ok) { gamma = sy / yy; ++nvalid; }
  }
  __syncthreads();
  for (int j = st.hist_n - 1; j >= 0; --j) {
    if (L.sy[j] == 0.0) continue;
    const int slot = (st.hist_next - st.hist_n + j + m) % m;
    double a = 0.0;
    for (int i = lane; i < nv; i += DY_THREADS)
      if (L.cls[i] == 2) a = fma(hs[(size_t)slot * nv + i], L.dir[i], a);
    a = dy_sum(a) / L.sy[j];
    if (lane == 0) L.al[j] = a;
    for (int i = lane; i < nv; i += DY_THREADS)
      if (L.cls[i] == 2) L.dir[i] = fma(-a, hy[(size_t)slot * nv + i], L.dir[i]);
  }
  if (nvalid == 0) gamma = 1.0;
  for (int i = lane; i < nv; i += DY_THREADS)
    if (L.cls[i] == 2) L.dir[i] *= gamma;
  __syncthreads();
  for (int j = 0; j < st.hist_n; ++j) {
    if (L.sy[j] == 0.0) continue;
    const int slot = (st.hist_next - st.hist_n + j + m) % m;
    double bq = 0.0;
    for (int i = lane; i < nv; i += DY_THREADS)
      if (L.cls[i] == 2) bq = fma(hy[(size_t)slot * nv + i], L.dir[i], bq);
    bq = dy_sum(bq) / L.sy[j];
    const double coef = L.al[j] - bq;
    for (int i = lane; i < nv; i += DY_THREADS)
      if (L.cls[i] == 2) L.dir[i] = fma(coef, hs[(size_t)slot * nv + i], L.dir[i]);
  }
  // negate; the scaled gradient on class 1; a variable at its bound does not move below it
  double gd = 0.0, dn = 0.0;
  for (int i = lane; i < nv; i += DY_THREADS) {
    double v = L.cls[i] == 2 ? -L.dir[i] : L.cls[i] == 1 ? -gamma * L.g[i] : 0.0;
    if (L.x[i] <= 0.0 && v < 0.0) v = 0.0;
    L.dir[i] = v;
    gd = fma(L.g[i], v, gd);
    dn = fma(v, v, dn);
  }
  gd = dy_sum(gd);
  dn = dy_sum(dn);
  st.steep = nvalid == 0;
  if (!(gd < 0.0) || !isfinite(dn)) {   // not a descent direction: drop the history, projected steepest descent
    st.hist_n = 0;
    st.steep = 1;
    gd = 0.0; dn = 0.0;
    for (int i = lane; i < nv; i += DY_THREADS) {
      double v = L.fixed[i] ? 0.0 : -L.g[i];
      if (L.x[i] <= 0.0 && v < 0.0) v = 0.0;
      L.dir[i] = v;
      gd = fma(L.g[i], v, gd);
      dn = fma(v, v, dn);
    }
    gd = dy_sum(gd);
    dn = dy_sum(dn);
  }
  st.gd = gd;
  st.t = st.steep ? (dn > 0.0 ? 1.0 / sqrt(dn) : 1.0) : 1.0;
  st.ls_iter = 0;
  __syncthreads();
}

__global__ __launch_bounds__(DY_THREADS) void k_dy_solve(DyCtx c) {
  __shared__ DyLds L;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int d = c.d, p = c.p, q = c.q, nv = c.nv, dd = d * d;
  double* ws = c.ws + (size_t)b * c.slice;
  DyState st = *reinterpret_cast<const DyState*>(ws);
  if (st.done) return;
  double* gS = ws + rc_dy_off_S();
  double* gx = ws + rc_dy_off_vec(d, p);
  double* gg = gx + nv;
  double* gdir = gg + nv;
  double* gest = gdir + nv;
  double* hs = ws + rc_dy_off_hist(d, p);
  double* hy = hs + (size_t)c.m * nv;
  for (int i = lane; i < nv; i += DY_THREADS) {
    L.x[i] = gx[i]; L.g[i] = gg[i]; L.dir[i] = gdir[i];
    L.fixed[i] = c.fixed[i];
  }
  for (int i = lane; i < q * q; i += DY_THREADS) L.S[i] = gS[i];
  __syncthreads();
  const double ninv = 1.0 / (double)c.n_rows[b];
  const double lw = c.lambda_w[b], la = c.lambda_a[b];
  st.n_launch += 1;

  int evals = 0;
  while (!st.done && evals < c.epl) {
    const bool start = st.phase == DY_PH_START;
    for (int i = lane; i < nv; i += DY_THREADS)
      L.xt[i] = start ? L.x[i] : (L.fixed[i] ? 0.0 : fmax(0.0, fma(st.t, L.dir[i], L.x[i])));
    __syncthreads();
    double ht;
    const double ft = dy_eval(L, c, ninv, st.rho, st.alpha, lw, la, lane, &ht);
    ++evals; st.n_evals += 1; st.inner_evals += 1;
    bool inner_done = false;
    if (start) {
      if (!isfinite(ft)) { st.done = 1; st.status = REDCLIFF_DYNOTEARS_NONFINITE; break; }
      for (int i = lane; i < nv; i += DY_THREADS) L.g[i] = L.gt[i];
      __syncthreads();
      st.f = ft; st.hx = ht;
      st.pg = dy_pgnorm(L, nv, lane);
      if (st.pg <= c.pgtol) inner_done = true;
      else { dy_direction(L, c, st, hs, hy, lane); st.phase = DY_PH_SEARCH; }
    } else {
      double gdx = 0.0, gtdx = 0.0, sy = 0.0, yy = 0.0, ss = 0.0;
      for (int i = lane; i < nv; i += DY_THREADS) {
        const double s = L.xt[i] - L.x[i], y = L.gt[i] - L.g[i];
        gdx = fma(L.g[i], s, gdx);
        gtdx = fma(L.gt[i], s, gtdx);
        sy = fma(s, y, sy);
        yy = fma(y, y, yy);
        ss = fma(s, s, ss);
      }
      gdx = dy_sum(gdx); gtdx = dy_sum(gtdx); sy = dy_sum(sy); yy = dy_sum(yy); ss = dy_sum(ss);
      const bool finite = isfinite(ft);
      if (!finite) st.n_nonfinite += 1;
      const double fscale = fmax(fabs(st.f), 1.0);
      const bool armijo = finite && gdx < 0.0 && ft <= st.f + 1e-3 * gdx;
      const bool approx = finite && gdx < 0.0 && ft <= st.f + 1e-13 * fscale && gtdx <= -0.8 * gdx && gtdx >= gdx;
      if (armijo || approx) {
        if (sy > 2.2e-16 * yy && ss > 0.0) {
          const int slot = st.hist_next;
          for (int i = lane; i < nv; i += DY_THREADS) {
            hs[(size_t)slot * nv + i] = L.xt[i] - L.x[i];
            hy[(size_t)slot * nv + i] = L.gt[i] - L.g[i];
          }
          st.hist_next = (slot + 1) % c.m;
          if (st.hist_n < c.m) st.hist_n += 1;
        }
        for (int i = lane; i < nv; i += DY_THREADS) { L.x[i] = L.xt[i]; L.g[i] = L.gt[i]; }
        __syncthreads();
        const double fold = st.f;
        st.f = ft; st.hx = ht;
        st.inner_iter += 1; st.n_qn += 1;
        st.pg = dy_pgnorm(L, nv, lane);
        if (st.pg <= c.pgtol || fold - ft <= c.ftol * fmax(fmax(fabs(fold), fabs(ft)), 1.0) || st.inner_iter >= c.maxiter ||
            st.inner_evals >= c.maxfun)
          inner_done = true;
        else
          dy_direction(L, c, st, hs, hy, lane);
      } else {
        st.ls_iter += 1;
        if (st.inner_evals >= c.maxfun) inner_done = true;
        else if (st.ls_iter >= c.maxls) {
          st.n_lsfail += 1;
          if (st.steep) inner_done = true;   // the search failed along the projected gradient itself: this solve ends
          else { st.hist_n = 0; dy_direction(L, c, st, hs, hy, lane); }
        } else if (!finite || !(gdx < 0.0)) {
          st.t *= 0.1;
        } else {
          // minimiser of the parabola through f, its slope along the step and the trial value, kept in [0.1 t, 0.5 t]
          const double den = 2.0 * (ft - st.f - gdx);
          double r = den > 0.0 ? -gdx / den : 0.5;
          r = fmin(0.5, fmax(0.1, r));
          st.t *= r;
        }
      }
    }
    if (inner_done) {
      // the reference's outer loop, from "h_new = h(wa_new)" on
      st.n_solves += 1;
      st.f_last = st.f; st.pg_last = st.pg;
      st.h_new = st.hx;
      if (st.h_new > 0.25 * st.h_value) st.rho *= 10.0;
      const bool again = st.rho < c.rho_max && (st.h_new > 0.25 * st.h_value || st.h_new == INFINITY);
      if (!again) {
        for (int i = lane; i < nv; i += DY_THREADS) gest[i] = L.x[i];
        st.h_value = st.h_new;
        st.alpha += st.rho * st.h_value;
        st.outer_iter += 1;
        if (st.h_value <= c.h_tol) { st.done = 1; st.status = REDCLIFF_DYNOTEARS_CONVERGED; }
        else if (st.outer_iter >= c.max_iter) { st.done = 1; st.status = st.rho >= c.rho_max ? REDCLIFF_DYNOTEARS_RHO_CAP : REDCLIFF_DYNOTEARS_MAXITER; }
        else if (!(st.rho < c.rho_max)) {
          while (st.outer_iter < c.max_iter) { st.alpha += st.rho * st.h_value; st.outer_iter += 1; }
          st.done = 1; st.status = REDCLIFF_DYNOTEARS_RHO_CAP;
        }
      } else {
        __syncthreads();
        for (int i = lane; i < nv; i += DY_THREADS) L.x[i] = gest[i];
      }
      st.phase = DY_PH_START;
      st.hist_n = 0; st.hist_next = 0; st.inner_iter = 0; st.inner_evals = 0; st.ls_iter = 0;
      __syncthreads();
    }
  }

  for (int i = lane; i < nv; i += DY_THREADS) { gx[i] = L.x[i]; gg[i] = L.g[i]; gdir[i] = L.dir[i]; }
  if (st.done) {
    const bool nf = st.status == REDCLIFF_DYNOTEARS_NONFINITE;
    const double nan = __builtin_nan("");
    __syncthreads();
    for (int e = lane; e < dd; e += DY_THREADS) c.W[(size_t)b * dd + e] = nf ? nan : gest[e] - gest[dd + e];
    for (int e = lane; e < p * dd; e += DY_THREADS) {
      const int k = e / dd, r = e - k * dd;
      c.A[(size_t)b * p * dd + e] = nf ? nan : gest[2 * dd + 2 * k * dd + r] - gest[2 * dd + 2 * k * dd + dd + r];
    }
    if (c.wa) for (int i = lane; i < nv; i += DY_THREADS) c.wa[(size_t)b * nv + i] = nf ? nan : gest[i];
    if (lane == 0) {
      c.status[b] = st.status;
      double* o = c.stats + (size_t)b * 6;
      o[0] = st.h_value; o[1] = st.rho; o[2] = st.alpha; o[3] = st.f_last; o[4] = st.pg_last; o[5] = (double)st.n_lsfail;
      int32_t* k = c.counts + (size_t)b * 6;
      k[0] = st.outer_iter; k[1] = st.n_solves; k[2] = st.n_qn; k[3] = st.n_evals; k[4] = st.n_nonfinite; k[5] = st.n_launch;
    }
  } else if (lane == 0) {
    atomicAdd(c.remaining, 1);
  }
  if (lane == 0) *reinterpret_cast<DyState*>(ws) = st;
}

int dy_limits(int32_t d, int32_t p, int32_t m) {
  if (d < 1 || p < 1 || m < 1) {
    rc_set_error("dynotears: bad arguments (d=%d p=%d m=%d)", d, p, m);
    return REDCLIFF_EINVAL;
  }
  if (d > DY_DMAX || (int64_t)(p + 1) * d > DY_QMAX || m > DY_MMAX) {
    rc_set_error("dynotears: outside kernel limits (d <= %d, (p + 1) d <= %d, m <= %d; d=%d p=%d m=%d)", DY_DMAX, DY_QMAX, DY_MMAX, d, p, m);
    return REDCLIFF_ELIMIT;
  }
  return 0;
}

}  // namespace

extern "C" {

int redcliff_dynotears_supported(int32_t d, int32_t p) { return dy_limits(d, p, 1) == 0 ? 1 : 0; }

size_t redcliff_dynotears_ws_bytes(int32_t P, int32_t d, int32_t p, int32_t m) {
  if (P < 0 || dy_limits(d, p, m) != 0) return 0;
  return sizeof(double) * (size_t)P * rc_dy_slice(d, p, m) + 16;
}

int redcliff_dynotears_run(const RedcliffDynotearsArgs* a, void* stream) {
  if (!a) { rc_set_error("null dynotears arguments"); return REDCLIFF_EINVAL; }
  int e = dy_limits(a->d, a->p, a->m);
  if (e) return e;
  if (a->P < 0 || a->P > (1 << 24) || a->max_iter < 1 || a->evals_per_launch < 1 || a->maxiter < 1 || a->maxfun < 1 || a->maxls < 1 ||
      (a->dtype != REDCLIFF_DYNOTEARS_F32 && a->dtype != REDCLIFF_DYNOTEARS_F64) || !(a->h_tol >= 0.0) || !(a->rho0 >= 0.0) ||
      !std::isfinite(a->rho0) || !std::isfinite(a->alpha0) || !(a->rho_max > 0.0) || !(a->factr >= 0.0) || !(a->pgtol >= 0.0)) {
    rc_set_error("dynotears_run: bad arguments (P=%d max_iter=%d evals_per_launch=%d maxiter=%d maxfun=%d maxls=%d dtype=%d)", a->P,
                 a->max_iter, a->evals_per_launch, a->maxiter, a->maxfun, a->maxls, a->dtype);
    return REDCLIFF_EINVAL;
  }
  if (a->rho0 == 0.0 && a->max_iter != 1) {
    rc_set_error("dynotears_run: rho0 = 0 never grows; it is accepted with max_iter = 1 only");
    return REDCLIFF_EINVAL;
  }
  if (a->P == 0) return 0;
  if (!a->X || !a->Xlags || !a->n_rows || !a->lambda_w || !a->lambda_a || !a->fixed || !a->W || !a->A || !a->status || !a->stats ||
      !a->counts || !a->remaining || !a->ws) {
    rc_set_error("dynotears_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->x_pstride < 0 || a->x_rstride < 0 || a->xl_pstride < 0 || a->xl_rstride < 0) {
    rc_set_error("dynotears_run: negative stride");
    return REDCLIFF_EINVAL;
  }
  const size_t need = redcliff_dynotears_ws_bytes(a->P, a->d, a->p, a->m);
  if (a->ws_bytes < need) { rc_set_error("dynotears_run: workspace too small: %zu < %zu", a->ws_bytes, need); return REDCLIFF_EWORKSPACE; }
  if ((reinterpret_cast<uintptr_t>(a->ws) & 15) != 0) { rc_set_error("dynotears_run: workspace not 16-byte aligned"); return REDCLIFF_EINVAL; }
  DyCtx c;
  memset(&c, 0, sizeof(c));
  c.P = a->P; c.d = a->d; c.p = a->p; c.q = rc_dy_q(a->d, a->p); c.nv = rc_dy_nv(a->d, a->p); c.m = a->m; c.dtype = a->dtype;
  c.epl = a->evals_per_launch; c.max_iter = a->max_iter; c.maxiter = a->maxiter; c.maxfun = a->maxfun; c.maxls = a->maxls;
  c.h_tol = a->h_tol; c.rho0 = a->rho0; c.alpha0 = a->alpha0; c.rho_max = a->rho_max;
  c.ftol = a->factr * 2.220446049250313e-16; c.pgtol = a->pgtol;
  c.X = a->X; c.x_ps = a->x_pstride; c.x_rs = a->x_rstride; c.Xl = a->Xlags; c.xl_ps = a->xl_pstride; c.xl_rs = a->xl_rstride;
  c.n_rows = a->n_rows; c.lambda_w = a->lambda_w; c.lambda_a = a->lambda_a; c.fixed = a->fixed;
  c.W = a->W; c.A = a->A; c.wa = a->wa; c.status = a->status; c.stats = a->stats; c.counts = a->counts; c.remaining = a->remaining;
  c.ws = static_cast<double*>(a->ws); c.slice = rc_dy_slice(a->d, a->p, a->m);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->start) {
    if (a->dtype == REDCLIFF_DYNOTEARS_F32) hipLaunchKernelGGL(k_dy_gram<float>, dim3((unsigned)c.P), dim3(256), 0, s, c);
    else hipLaunchKernelGGL(k_dy_gram<double>, dim3((unsigned)c.P), dim3(256), 0, s, c);
    if ((e = rc_check(hipGetLastError(), "k_dy_gram"))) return e;
  }
  if ((e = rc_check(hipMemsetAsync(a->remaining, 0, sizeof(int32_t), s), "dynotears remaining"))) return e;
  hipLaunchKernelGGL(k_dy_solve, dim3((unsigned)c.P), dim3(DY_THREADS), 0, s, c);
  if ((e = rc_check(hipGetLastError(), "k_dy_solve"))) return e;
  return 0;
}

}  // extern "C"
