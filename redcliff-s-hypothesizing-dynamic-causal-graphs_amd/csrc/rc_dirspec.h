// rc_dirspec.h -- context, limits, LDS and workspace layouts of the directed-spectrum feature extraction
// (rc_dirspec.hip; general_utils/directed_spectrum.py and make_high_level_signal_features of the reference).
#pragma once
#include "rc_common.h"

#define DS_FMAX 256   // frequencies (= nperseg) of one problem: 4 per lane
#define DS_WAVES 4    // (window, pair) problems per workgroup of k_ds_pair, one wavefront each
#define DS_OK 0       // per-(window, pair) status words
#define DS_MAXITER 1
#define DS_PIVOT 2

// Bytes of k_ds_pair's dynamic LDS: the twiddle table (cos, sin)[F], then per wave g[F] (g00, g11, Re g01,
// Im g01) and the truncated lags gamma[F/2 + 1] (4 doubles each).
__host__ __device__ inline size_t rc_dirspec_wave_doubles(int F) { return 4 * (size_t)F + 4 * (size_t)(F / 2 + 1); }
__host__ __device__ inline size_t rc_dirspec_lds_bytes(int F) {
  return sizeof(double) * (2 * (size_t)F + DS_WAVES * rc_dirspec_wave_doubles(F));
}

// Workspace: spectra [N][nseg][p][F] complex double, then the NaN flags [N] (int32).
__host__ __device__ inline int64_t rc_dirspec_nseg(int T, int nperseg, int noverlap) {
  return (T - noverlap) / (nperseg - noverlap);
}
__host__ __device__ inline size_t rc_dirspec_spec_bytes(int64_t N, int T, int p, int nperseg, int noverlap) {
  return 16 * (size_t)N * (size_t)rc_dirspec_nseg(T, nperseg, noverlap) * (size_t)p * (size_t)nperseg;
}

struct DsCtx {
  int N, T, p, F, nov, step, nseg, npairs, ntri, max_iter, f32, layout, i1, i2, nf, half;
  int64_t xws, xts, ors;
  double scale;   // 1 / (fs * sum w^2 * nseg): density scaling and the mean over segments
  double val;     // frequency of bin 1 (numpy.fft.fftfreq: 1 / (F * (1 / fs)))
  double tol;
  const void* X;
  double2* spec;
  int32_t* nan;
  float* out;
  double* power;
  int32_t* status;
  int32_t* iters;
};
