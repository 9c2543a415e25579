// rc_dirspec.hip -- directed-spectrum features (general_utils/directed_spectrum.py get_directed_spectrum with
// pairwise=True, and general_utils/time_series.py make_high_level_signal_features) for N windows in one call.
//
//   k_ds_fill     (window)                    NaN scan of the window; its feature rows start as 0 (the diagonal of
//        the directed spectrum stays 0) or, for a window holding a NaN, as NaN; the flag goes to the workspace.
//   k_ds_spectra  (window, segment, channel)  detrend="constant", the periodic Hann window, the two-sided DFT of
//        length F = nperseg as a direct sum over a twiddle table in LDS; complex double into the workspace.
//   k_ds_pair     one wavefront per (window, channel pair a < b), lane l owns frequencies l, l + 64, ...:
//        the pair's 2x2 CPSD (mean over segments of conj(X_b) X_a, density scaling), the singular branch with its
//        per-pair regulariser, _init_psi, the Wilson iteration with the _plus_operator truncation, H = psi / A0,
//        Sigma = A0 A0^T, the two directed spectra, the one-sided fold, the frequency scaling, the crop and the
//        float32 store into the feature row (either layout).
//   k_ds_power    (window, channel pair a >= b, kept bin)  |one-sided CPSD| * f, the `power` features.
//
// Precision: every operation runs in double.  With float32 input and a pair off the singular branch the values
// the reference holds in single precision (CPSD, its Cholesky factor, gamma0, h, A0, Sigma and A0's convergence
// test) are rounded to float32 where the reference assigns them.  On the singular branch the reference's
// regulariser (a float64 diagonal) promotes the CPSD to complex128, so from there on nothing is rounded.
// The transforms along frequency are direct sums in ascending order and the wave reductions are fixed
// butterflies: no atomics, no dependence on the grid, the same input gives the same bits.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "rc_dirspec.h"

namespace {

__device__ inline double ds_r32(double x) { return (double)(float)x; }

// LDS hand-off between the lanes of one wavefront: a wave's LDS operations complete in issue order, so only the
// compiler has to be kept from moving them across this point.
__device__ inline void ds_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// max over the wave, the same bits in every lane; a NaN anywhere gives +inf (numpy's max would give NaN: both
// fail every "< tol" and "> threshold" decides the other way only where the caller asks for it).
__device__ inline double ds_wave_max(double v) {
  if (v != v) v = INFINITY;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ inline double ds_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline double ds_load(const DsCtx& c, int n, int t, int ch) {
  const int64_t i = (int64_t)n * c.xws + (int64_t)t * c.xts + ch;
  return c.f32 ? (double)static_cast<const float*>(c.X)[i] : static_cast<const double*>(c.X)[i];
}

// one-sided weight of bin k <= half: the Nyquist bin is doubled only for odd F
__device__ inline double ds_fold(const DsCtx& c, int k) {
  if (k == 0) return 1.0;
  if (k < c.half) return 2.0;
  return (c.F & 1) ? 2.0 : 1.0;
}

__global__ __launch_bounds__(256) void k_ds_fill(DsCtx c, int64_t width, int64_t pwidth) {
  const int n = blockIdx.x;
  int bad = 0;
  for (int i = threadIdx.x; i < c.T * c.p; i += blockDim.x) {
    const double x = ds_load(c, n, i / c.p, i % c.p);
    bad |= (x != x);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) c.nan[n] = bad;
  const float v = bad ? NAN : 0.f;
  for (int64_t i = threadIdx.x; i < width; i += blockDim.x) c.out[(int64_t)n * c.ors + i] = v;
  if (c.power)
    for (int64_t i = threadIdx.x; i < pwidth; i += blockDim.x) c.power[(int64_t)n * pwidth + i] = bad ? (double)NAN : 0.0;
}

__global__ __launch_bounds__(64) void k_ds_spectra(DsCtx c) {
  extern __shared__ __attribute__((aligned(16))) char ds_smem[];
  double2* tw = reinterpret_cast<double2*>(ds_smem);    // [F] (cos, sin)(2 pi j / F)
  double* seg = reinterpret_cast<double*>(tw + c.F);    // [F]
  const int F = c.F;
  const int ch = blockIdx.x % c.p;
  const int s = (blockIdx.x / c.p) % c.nseg;
  const int n = blockIdx.x / (c.p * c.nseg);
  if (c.nan[n]) return;
  for (int t = threadIdx.x; t < F; t += 64) {
    seg[t] = ds_load(c, n, s * c.step + t, ch);
    double sn, cs;
    sincospi(2.0 * (double)t / (double)F, &sn, &cs);
    tw[t] = make_double2(cs, sn);
  }
  __syncthreads();
  double mean = 0.0;
  for (int t = 0; t < F; ++t) mean += seg[t];
  mean /= (double)F;
  __syncthreads();
  for (int t = threadIdx.x; t < F; t += 64) seg[t] = (seg[t] - mean) * (0.5 - 0.5 * tw[t].x);
  __syncthreads();
  double2* dst = c.spec + (((int64_t)n * c.nseg + s) * c.p + ch) * F;
  for (int f = threadIdx.x; f < F; f += 64) {
    double re = 0.0, im = 0.0;
    int idx = 0;
    for (int t = 0; t < F; ++t) {
      const double2 w = tw[idx];
      re += seg[t] * w.x;
      im -= seg[t] * w.y;
      idx += f;
      if (idx >= F) idx -= F;
    }
    dst[f] = make_double2(re, im);
  }
}

struct DsC { double re, im; };
__device__ inline DsC ds_mul(DsC a, DsC b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ inline DsC ds_add(DsC a, DsC b) { return {a.re + b.re, a.im + b.im}; }
__device__ inline DsC ds_sub(DsC a, DsC b) { return {a.re - b.re, a.im - b.im}; }
__device__ inline DsC ds_scale(DsC a, double s) { return {a.re * s, a.im * s}; }
__device__ inline DsC ds_div(DsC a, DsC b) {
  const double d = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
__device__ inline double ds_abs(DsC a) { return hypot(a.re, a.im); }

// _check_convergence's term for one complex entry, float64 rules
__device__ inline double ds_rel(DsC x, DsC x0) {
  double ab = ds_abs(x);
  const double df = ds_abs(ds_sub(x, x0));
  if (ab <= 2.0 * DBL_EPSILON) ab = 1.0;
  return df / ab;
}

// the pair's columns of one kept bin in the feature row
__device__ inline void ds_put(const DsCtx& c, float* row, int a, int b, int i, float vab, float vba) {
  const int p = c.p;
  if (c.layout == 0) {
    row[((int64_t)a * p + b) * c.nf + i] = vab;
    row[((int64_t)b * p + a) * c.nf + i] = vba;
  } else {
    const int64_t W = 2 * p - 1, m = c.nf;
    row[(int64_t)a * m * W + i * W + b] = vab;            // x[a][b] in row a's outgoing block
    row[(int64_t)b * m * W + i * W + p + a] = vab;        // ... and in row b's incoming block (a < b)
    row[(int64_t)b * m * W + i * W + a] = vba;            // x[b][a] in row b's outgoing block
    row[(int64_t)a * m * W + i * W + p + b - 1] = vba;    // ... and in row a's incoming block (b > a)
  }
}

template <int J>
__global__ __launch_bounds__(64 * DS_WAVES) void k_ds_pair(DsCtx c) {
  extern __shared__ __attribute__((aligned(16))) char ds_smem[];
  const int F = c.F, half = c.half;
  double2* tw = reinterpret_cast<double2*>(ds_smem);
  for (int t = threadIdx.x; t < F; t += blockDim.x) {
    double sn, cs;
    sincospi(2.0 * (double)t / (double)F, &sn, &cs);
    tw[t] = make_double2(cs, sn);
  }
  __syncthreads();  // the only workgroup barrier: from here on the waves are independent
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * DS_WAVES + wave;
  if (q >= (int64_t)c.N * c.npairs) return;
  const int n = (int)(q / c.npairs);
  if (c.nan[n]) {
    if (lane == 0) { c.status[q] = DS_OK; c.iters[q] = 0; }
    return;
  }
  int a = 0, rem = (int)(q % c.npairs);
  while (rem >= c.p - 1 - a) { rem -= c.p - 1 - a; ++a; }
  const int b = a + 1 + rem;
  double* gbuf = reinterpret_cast<double*>(tw + F) + (size_t)wave * rc_dirspec_wave_doubles(F);  // [F][4]
  double* gam = gbuf + 4 * (size_t)F;                                                              // [half + 1][4]
  float* row = c.out + (int64_t)n * c.ors;

  // ---- the pair's CPSD at this lane's frequencies: [[c00, c01], [conj(c01), c11]] ----
  double c00[J], c11[J];
  DsC c01[J];
  bool single = c.f32 != 0;
  double cmax = 0.0, cond = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int f = lane + 64 * j;
    c00[j] = c11[j] = 0.0;
    c01[j] = {0.0, 0.0};
    if (f < F) {
      for (int s = 0; s < c.nseg; ++s) {
        const double2 xa = c.spec[(((int64_t)n * c.nseg + s) * c.p + a) * F + f];
        const double2 xb = c.spec[(((int64_t)n * c.nseg + s) * c.p + b) * F + f];
        c00[j] += xa.x * xa.x + xa.y * xa.y;
        c11[j] += xb.x * xb.x + xb.y * xb.y;
        c01[j].re += xb.x * xa.x + xb.y * xa.y;   // conj(X_b) X_a
        c01[j].im += xb.x * xa.y - xb.y * xa.x;
      }
      c00[j] *= c.scale; c11[j] *= c.scale; c01[j] = ds_scale(c01[j], c.scale);
      if (single) { c00[j] = ds_r32(c00[j]); c11[j] = ds_r32(c11[j]); c01[j] = {ds_r32(c01[j].re), ds_r32(c01[j].im)}; }
      double ab = ds_abs(c01[j]);
      // condition number of the Hermitian 2x2: the ratio of its singular values |lambda|
      const double m = 0.5 * (c00[j] + c11[j]), d = 0.5 * (c00[j] - c11[j]);
      const double r = sqrt(d * d + ab * ab);
      double hi = fabs(m + r), lo = fabs(m - r);
      if (lo > hi) { const double t = hi; hi = lo; lo = t; }
      double cd = hi / lo;   // inf for an exactly singular matrix, NaN for a zero one
      if (single) { cd = ds_r32(cd); ab = ds_r32(ab); }
      if (cd != cd) cd = INFINITY;
      cond = fmax(cond, cd);
      cmax = fmax(cmax, fmax(ab, fmax(fabs(c00[j]), fabs(c11[j]))));
    }
  }
  cond = ds_wave_max(cond);
  const bool singular = c.nseg < 2 || cond > (single ? 1.0 / (double)FLT_EPSILON : 1.0 / DBL_EPSILON);
  if (singular) {
    cmax = ds_wave_max(cmax);
    // numpy.spacing(|cpsd|).max() * 100 in the CPSD's precision; the sum is complex128 in the reference
    const double sp = single ? (double)(nextafterf((float)cmax, INFINITY) - (float)cmax) : nextafter(cmax, (double)INFINITY) - cmax;
    const double reg = sp * 100.0;
#pragma unroll
    for (int j = 0; j < J; ++j) { c00[j] += reg; c11[j] += reg; }
    single = false;
  }

  // ---- _init_psi: gamma0 = lag 0 of the inverse transform, h = cholesky(gamma0)^T ----
  double s00 = 0.0, s11 = 0.0, s01 = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < F) { s00 += c00[j]; s11 += c11[j]; s01 += c01[j].re; }
  double g00 = ds_wave_sum(s00) / (double)F, g11 = ds_wave_sum(s11) / (double)F, g01 = ds_wave_sum(s01) / (double)F;
  if (single) { g00 = ds_r32(g00); g11 = ds_r32(g11); g01 = ds_r32(g01); }
  int bad = !(g00 > 0.0);
  double h00 = sqrt(g00), h01 = g01 / h00;
  if (single) { h00 = ds_r32(h00); h01 = ds_r32(g01 / h00); }
  double t11 = single ? ds_r32(g11 - ds_r32(h01 * h01)) : g11 - h01 * h01;
  bad |= !(t11 > 0.0);
  double h11 = sqrt(t11);
  if (single) h11 = ds_r32(h11);

  // ---- L = cholesky(cpsd) per frequency (lower: l00, l10, l11) ----
  double l00[J], l11[J];
  DsC l10[J], p00[J], p01[J], p10[J], p11[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    l00[j] = l11[j] = 1.0;
    l10[j] = {0.0, 0.0};
    if (lane + 64 * j < F) {
      bad |= !(c00[j] > 0.0);
      l00[j] = sqrt(c00[j]);
      if (single) l00[j] = ds_r32(l00[j]);
      l10[j] = {c01[j].re / l00[j], -c01[j].im / l00[j]};   // c10 / l00, c10 = conj(c01)
      if (single) l10[j] = {ds_r32(l10[j].re), ds_r32(l10[j].im)};
      double t = c11[j] - (l10[j].re * l10[j].re + l10[j].im * l10[j].im);
      if (single) t = ds_r32(t);
      bad |= !(t > 0.0);
      l11[j] = sqrt(t);
      if (single) l11[j] = ds_r32(l11[j]);
    }
    p00[j] = {h00, 0.0}; p01[j] = {h01, 0.0}; p10[j] = {0.0, 0.0}; p11[j] = {h11, 0.0};
  }
  if (__any(bad)) {   // numpy.linalg.cholesky raises: the pair's features are NaN and the status says why
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int k = lane + 64 * j;
      if (k <= half && k < F && k >= c.i1 && k < c.i2) ds_put(c, row, a, b, k - c.i1, NAN, NAN);
    }
    if (lane == 0) { c.status[q] = DS_PIVOT; c.iters[q] = 0; }
    return;
  }

  // ---- the Wilson iteration ----
  double a00 = h00, a01 = h01, a10 = 0.0, a11 = h11;
  const double invF = 1.0 / (double)F;
  const float tolf = (float)c.tol;
  int it = 0, status = DS_MAXITER;
  while (it < c.max_iter) {
    ++it;
    // g = psi^-1 cpsd psi^-* + I through Y = psi^-1 L
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int f = lane + 64 * j;
      if (f < F) {
        const DsC det = ds_sub(ds_mul(p00[j], p11[j]), ds_mul(p01[j], p10[j]));
        const DsC y00 = ds_div(ds_sub(ds_scale(p11[j], l00[j]), ds_mul(p01[j], l10[j])), det);
        const DsC y01 = ds_div(ds_scale(p01[j], -l11[j]), det);
        const DsC y10 = ds_div(ds_sub(ds_mul(p00[j], l10[j]), ds_scale(p10[j], l00[j])), det);
        const DsC y11 = ds_div(ds_scale(p00[j], l11[j]), det);
        double* g = gbuf + 4 * f;
        g[0] = y00.re * y00.re + y00.im * y00.im + (y01.re * y01.re + y01.im * y01.im) + 1.0;
        g[1] = y10.re * y10.re + y10.im * y10.im + (y11.re * y11.re + y11.im * y11.im) + 1.0;
        // g01 = y00 conj(y10) + y01 conj(y11)
        g[2] = y00.re * y10.re + y00.im * y10.im + (y01.re * y11.re + y01.im * y11.im);
        g[3] = y00.im * y10.re - y00.re * y10.im + (y01.im * y11.re - y01.re * y11.im);
      }
    }
    ds_wave_sync();
    // gamma = real(ifft(g)) at lags 0 .. floor(F / 2), half of lag 0, half of the Nyquist lag for even F
    for (int k = lane; k <= half; k += 64) {
      {
        double r00 = 0.0, r11 = 0.0, rc = 0.0, rs = 0.0;
        int idx = 0;
        for (int f = 0; f < F; ++f) {
          const double2 w = tw[idx];
          const double* g = gbuf + 4 * f;
          r00 += g[0] * w.x;
          r11 += g[1] * w.x;
          rc += g[2] * w.x;
          rs += g[3] * w.y;
          idx += k;
          if (idx >= F) idx -= F;
        }
        double wk = invF;
        if (k == 0 || (k == half && !(F & 1))) wk *= 0.5;
        double* o = gam + 4 * k;
        o[0] = r00 * wk; o[1] = (rc - rs) * wk; o[2] = (rc + rs) * wk; o[3] = r11 * wk;   // 00, 01, 10, 11
      }
    }
    ds_wave_sync();
    const double z00 = gam[0], z01 = gam[1], z10 = gam[2], z11 = gam[3];   // g0 (half of lag 0)
    double rel = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int f = lane + 64 * j;
      if (f < F) {
        DsC q00 = {0, 0}, q01 = {0, 0}, q10 = {0, 0}, q11 = {0, 0};
        int idx = 0;
        for (int k = 0; k <= half; ++k) {   // gplus = fft(truncated gamma)
          const double2 w = tw[idx];
          const double* o = gam + 4 * k;
          q00.re += o[0] * w.x; q00.im -= o[0] * w.y;
          q01.re += o[1] * w.x; q01.im -= o[1] * w.y;
          q10.re += o[2] * w.x; q10.im -= o[2] * w.y;
          q11.re += o[3] * w.x; q11.im -= o[3] * w.y;
          idx += f;
          if (idx >= F) idx -= F;
        }
        q01.re += z10;   // S = [[0, g0_10], [-g0_10, 0]] makes g0 + S upper triangular
        q10.re -= z10;
        const DsC n00 = ds_add(ds_mul(p00[j], q00), ds_mul(p01[j], q10));
        const DsC n01 = ds_add(ds_mul(p00[j], q01), ds_mul(p01[j], q11));
        const DsC n10 = ds_add(ds_mul(p10[j], q00), ds_mul(p11[j], q10));
        const DsC n11 = ds_add(ds_mul(p10[j], q01), ds_mul(p11[j], q11));
        double r = fmax(fmax(ds_rel(n00, p00[j]), ds_rel(n01, p01[j])), fmax(ds_rel(n10, p10[j]), ds_rel(n11, p11[j])));
        if (r != r) r = INFINITY;
        rel = fmax(rel, r);
        p00[j] = n00; p01[j] = n01; p10[j] = n10; p11[j] = n11;
      }
    }
    // A0 = A0 (g0 + S), g0 + S = [[z00, z01 + z10], [0, z11]]
    const double u01 = z01 + z10;
    double b00 = a00 * z00, b01 = a00 * u01 + a01 * z11, b10 = a10 * z00, b11 = a10 * u01 + a11 * z11;
    if (single) { b00 = ds_r32(b00); b01 = ds_r32(b01); b10 = ds_r32(b10); b11 = ds_r32(b11); }
    rel = ds_wave_max(rel);
    bool done = rel < c.tol;
    if (done) {
      const double nw[4] = {b00, b01, b10, b11}, od[4] = {a00, a01, a10, a11};
      if (single) {   // float32 rules: eps, the division and the comparison with float32(tol)
        float mx = 0.f;
        for (int e = 0; e < 4; ++e) {
          float ab = fabsf((float)nw[e]);
          const float df = fabsf((float)nw[e] - (float)od[e]);
          if (ab <= 2.f * FLT_EPSILON) ab = 1.f;
          const float r = df / ab;
          mx = (r != r) ? INFINITY : fmaxf(mx, r);
        }
        done = mx < tolf;
      } else {
        double mx = 0.0;
        for (int e = 0; e < 4; ++e) {
          double ab = fabs(nw[e]);
          const double df = fabs(nw[e] - od[e]);
          if (ab <= 2.0 * DBL_EPSILON) ab = 1.0;
          const double r = df / ab;
          mx = (r != r) ? (double)INFINITY : fmax(mx, r);
        }
        done = mx < c.tol;
      }
    }
    a00 = b00; a01 = b01; a10 = b10; a11 = b11;
    ds_wave_sync();
    if (done) { status = DS_OK; break; }   // wave-uniform: every lane holds the same rel and A0
  }

  // ---- H = psi A0^-1, Sigma = A0 A0^T, the directed spectra, fold, scale, crop, store ----
  const double detA = a00 * a11 - a01 * a10;
  double g_00 = a00 * a00 + a01 * a01, g_01 = a00 * a10 + a01 * a11, g_11 = a10 * a10 + a11 * a11;
  if (single) { g_00 = ds_r32(g_00); g_01 = ds_r32(g_01); g_11 = ds_r32(g_11); }
  double sig1_0, sig0_1;   // conditional covariances
  if (single) {
    sig1_0 = ds_r32(g_11 - ds_r32(g_01 * ds_r32(g_01 / g_00)));
    sig0_1 = ds_r32(g_00 - ds_r32(g_01 * ds_r32(g_01 / g_11)));
  } else {
    sig1_0 = g_11 - g_01 * (g_01 / g_00);
    sig0_1 = g_00 - g_01 * (g_01 / g_11);
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    if (k <= half && k < F && k >= c.i1 && k < c.i2) {
      const DsC H01 = ds_scale(ds_sub(ds_scale(p01[j], a00), ds_scale(p00[j], a01)), 1.0 / detA);
      const DsC H10 = ds_scale(ds_sub(ds_scale(p10[j], a11), ds_scale(p11[j], a10)), 1.0 / detA);
      const double ds10 = (H01.re * H01.re + H01.im * H01.im) * sig1_0;   // b -> a entry [b][a]
      const double ds01 = (H10.re * H10.re + H10.im * H10.im) * sig0_1;   // entry [a][b]
      const double fold = ds_fold(c, k), fk = (double)k * c.val;
      ds_put(c, row, a, b, k - c.i1, (float)(ds01 * fold * fk), (float)(ds10 * fold * fk));
    }
  }
  if (lane == 0) { c.status[q] = status; c.iters[q] = it; }
}

__global__ __launch_bounds__(256) void k_ds_power(DsCtx c) {
  const int64_t total = (int64_t)c.N * c.ntri * c.nf;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const int i = (int)(g % c.nf), tri = (int)((g / c.nf) % c.ntri), n = (int)(g / ((int64_t)c.nf * c.ntri));
  if (c.nan[n]) return;
  int r = 0;
  while ((r + 1) * (r + 2) / 2 <= tri) ++r;   // tri = r (r + 1) / 2 + col, col <= r
  const int col = tri - r * (r + 1) / 2, k = c.i1 + i;
  double re = 0.0, im = 0.0;
  for (int s = 0; s < c.nseg; ++s) {
    const double2 xr = c.spec[(((int64_t)n * c.nseg + s) * c.p + r) * c.F + k];
    const double2 xc = c.spec[(((int64_t)n * c.nseg + s) * c.p + col) * c.F + k];
    re += xr.x * xc.x + xr.y * xc.y;   // conj(X_r) X_col
    im += xr.x * xc.y - xr.y * xc.x;
  }
  const double fold = ds_fold(c, k);
  re *= c.scale * fold; im *= c.scale * fold;
  double ab;
  if (c.f32) ab = ds_r32(hypot(ds_r32(re), ds_r32(im)));
  else ab = hypot(re, im);
  c.power[g] = ab * ((double)k * c.val);
}

using PairKern = void (*)(DsCtx);

int ds_ctx(const RedcliffDirspecArgs* a, DsCtx* c) {
  memset(c, 0, sizeof(*c));
  if (a->N < 0 || a->T < 1 || a->p < 2 || a->nperseg < 2 || a->noverlap < 0 || a->noverlap >= a->nperseg ||
      a->T < a->nperseg || a->max_iter < 0 || !(a->fs > 0.0) || (a->dtype != REDCLIFF_DIRSPEC_F32 && a->dtype != REDCLIFF_DIRSPEC_F64) ||
      (a->layout != REDCLIFF_DIRSPEC_VANILLA && a->layout != REDCLIFF_DIRSPEC_FLATTENED)) {
    rc_set_error("dirspec: bad arguments (N=%d T=%d p=%d nperseg=%d noverlap=%d max_iter=%d fs=%g dtype=%d layout=%d)", a->N,
                 a->T, a->p, a->nperseg, a->noverlap, a->max_iter, a->fs, a->dtype, a->layout);
    return REDCLIFF_EINVAL;
  }
  if (a->nperseg > DS_FMAX || a->p > 1024) {
    rc_set_error("dirspec: outside kernel limits (nperseg <= %d, p <= 1024; nperseg=%d p=%d)", DS_FMAX, a->nperseg, a->p);
    return REDCLIFF_ELIMIT;
  }
  c->N = a->N; c->T = a->T; c->p = a->p; c->F = a->nperseg; c->nov = a->noverlap; c->step = a->nperseg - a->noverlap;
  c->nseg = (int)rc_dirspec_nseg(a->T, a->nperseg, a->noverlap);
  c->npairs = a->p * (a->p - 1) / 2;
  c->ntri = a->p * (a->p + 1) / 2;
  c->max_iter = a->max_iter; c->f32 = a->dtype == REDCLIFF_DIRSPEC_F32; c->layout = a->layout;
  c->half = c->F / 2;
  c->val = 1.0 / ((double)c->F * (1.0 / a->fs));
  // numpy.searchsorted(f, [min_freq, max_freq]) on the one-sided bins f_k = k * val
  int i1 = 0, i2 = 0;
  while (i1 <= c->half && (double)i1 * c->val < a->min_freq) ++i1;
  while (i2 <= c->half && (double)i2 * c->val < a->max_freq) ++i2;
  c->i1 = i1; c->i2 = i2 > i1 ? i2 : i1; c->nf = c->i2 - c->i1;
  double sw = 0.0;
  for (int t = 0; t < c->F; ++t) {
    const double w = 0.5 - 0.5 * cos(2.0 * M_PI * (double)t / (double)c->F);
    sw += w * w;
  }
  c->scale = 1.0 / (a->fs * sw) / (double)c->nseg;
  c->tol = a->tol;
  return 0;
}

}  // namespace

extern "C" {

int redcliff_dirspec_supported(int32_t T, int32_t p, int32_t nperseg, int32_t noverlap) {
  RedcliffDirspecArgs a;
  memset(&a, 0, sizeof(a));
  a.T = T; a.p = p; a.nperseg = nperseg; a.noverlap = noverlap; a.fs = 1.0;
  DsCtx c;
  return ds_ctx(&a, &c) == 0 ? 1 : 0;
}

int redcliff_dirspec_nfreq(int32_t nperseg, double fs, double min_freq, double max_freq) {
  RedcliffDirspecArgs a;
  memset(&a, 0, sizeof(a));
  a.T = nperseg; a.p = 2; a.nperseg = nperseg; a.fs = fs; a.min_freq = min_freq; a.max_freq = max_freq;
  DsCtx c;
  const int e = ds_ctx(&a, &c);
  return e ? e : c.nf;
}

size_t redcliff_dirspec_ws_bytes(int32_t N, int32_t T, int32_t p, int32_t nperseg, int32_t noverlap) {
  if (redcliff_dirspec_supported(T, p, nperseg, noverlap) == 0 || N < 0) return 0;
  return rc_dirspec_spec_bytes(N, T, p, nperseg, noverlap) + (((size_t)N * 4 + 15) & ~(size_t)15) + 16;
}

int redcliff_dirspec_run(const RedcliffDirspecArgs* a, void* stream) {
  if (!a) { rc_set_error("null dirspec arguments"); return REDCLIFF_EINVAL; }
  DsCtx c;
  int e = ds_ctx(a, &c);
  if (e) return e;
  if (a->N == 0) return 0;
  if (!a->X || !a->out || !a->ws || !a->status || !a->iters) { rc_set_error("dirspec_run: null buffer in arguments"); return REDCLIFF_EINVAL; }
  const int64_t width = a->layout == REDCLIFF_DIRSPEC_VANILLA ? (int64_t)c.p * c.p * c.nf : (int64_t)c.p * c.nf * (2 * c.p - 1);
  if (a->out_rstride < width || a->x_tstride < c.p || a->x_wstride < 0 ||
      (a->N > 1 && a->x_wstride < (int64_t)(c.T - 1) * a->x_tstride + c.p)) {
    rc_set_error("dirspec_run: bad strides (out_rstride=%lld < %lld, x_wstride=%lld, x_tstride=%lld)", (long long)a->out_rstride,
                 (long long)width, (long long)a->x_wstride, (long long)a->x_tstride);
    return REDCLIFF_EINVAL;
  }
  const size_t need = redcliff_dirspec_ws_bytes(a->N, a->T, a->p, a->nperseg, a->noverlap);
  if (a->ws_bytes < need) { rc_set_error("dirspec_run: workspace too small: %zu < %zu", a->ws_bytes, need); return REDCLIFF_EWORKSPACE; }
  if ((reinterpret_cast<uintptr_t>(a->ws) & 15) != 0) { rc_set_error("dirspec_run: workspace not 16-byte aligned"); return REDCLIFF_EINVAL; }
  const int64_t nprob = (int64_t)c.N * c.npairs, nblk = (int64_t)c.N * c.nseg * c.p;
  if (nprob / DS_WAVES + 1 > INT32_MAX || nblk > INT32_MAX || (int64_t)c.N * c.ntri * (c.nf > 0 ? c.nf : 1) / 256 + 1 > INT32_MAX) {
    rc_set_error("dirspec_run: too many problems for one call (N=%d p=%d)", c.N, c.p);
    return REDCLIFF_ELIMIT;
  }
  c.xws = a->x_wstride; c.xts = a->x_tstride; c.ors = a->out_rstride;
  c.X = a->X; c.out = a->out; c.power = a->power; c.status = a->status; c.iters = a->iters;
  c.spec = static_cast<double2*>(a->ws);
  c.nan = reinterpret_cast<int32_t*>(static_cast<char*>(a->ws) + rc_dirspec_spec_bytes(a->N, a->T, a->p, a->nperseg, a->noverlap));
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_ds_fill, dim3(c.N), dim3(256), 0, s, c, width, (int64_t)c.ntri * c.nf);
  if ((e = rc_check(hipGetLastError(), "k_ds_fill"))) return e;
  hipLaunchKernelGGL(k_ds_spectra, dim3((unsigned)nblk), dim3(64), sizeof(double) * 3 * (size_t)c.F, s, c);
  if ((e = rc_check(hipGetLastError(), "k_ds_spectra"))) return e;
  const int J = (c.F + 63) / 64;
  PairKern k = J == 1 ? k_ds_pair<1> : J == 2 ? k_ds_pair<2> : J == 3 ? k_ds_pair<3> : k_ds_pair<4>;
  hipLaunchKernelGGL(k, dim3((unsigned)((nprob + DS_WAVES - 1) / DS_WAVES)), dim3(64 * DS_WAVES), rc_dirspec_lds_bytes(c.F), s, c);
  if ((e = rc_check(hipGetLastError(), "k_ds_pair"))) return e;
  if (c.power && c.nf > 0) {
    const int64_t total = (int64_t)c.N * c.ntri * c.nf;
    hipLaunchKernelGGL(k_ds_power, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, c);
    if ((e = rc_check(hipGetLastError(), "k_ds_power"))) return e;
  }
  return 0;
}

}  // extern "C"
