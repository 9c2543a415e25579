// rc_navar.h -- context, packed layout and limits of the NAVAR (MLP) baseline kernels (rc_navar.hip).
#pragma once
#include "rc_common.h"

#define NV_BC 64    // windows staged per pass over a batch
#define NV_SL 32    // hidden units of the last hidden layer per workgroup (the unit slice)
#define NV_MISC 240 // gb[32] | gbc[32] | gbi[32] | red[16] | rows[64] | Adam scalars, spare [64]

// Offsets (floats) of a replica's packed block:
// W1[N][H][K] | b1[N][H] | (W2[N][H][H] | b2[N][H]) | Wc[N][N][H] | bc[N][N] | biases[N]
struct NvOff {
  int64_t W1, b1, W2, b2, Wc, bc, bias, total;
};
__host__ __device__ inline NvOff rc_navar_off(int N, int H, int K, int two) {
  NvOff o;
  int64_t at = 0;
  o.W1 = at; at += (int64_t)N * H * K;
  o.b1 = at; at += (int64_t)N * H;
  o.W2 = at; at += two ? (int64_t)N * H * H : 0;
  o.b2 = at; at += two ? (int64_t)N * H : 0;
  o.Wc = at; at += (int64_t)N * N * H;
  o.bc = at; at += (int64_t)N * N;
  o.bias = at; at += N;
  o.total = at;
  return o;
}

__host__ __device__ inline int rc_navar_hp(int H) { return ((H + 15) / 16 * 16) | 1; }
__host__ __device__ inline int rc_navar_slices(int H) { return (H + NV_SL - 1) / NV_SL; }

// LDS floats of one workgroup, 0 outside the limits: the one formula behind redcliff_navar_supported,
// redcliff_navar_run and the launches (redcliff_amd/navar.py restates it).  Staged lags xs[64][K|1],
// the slice's pre-activations and their gradients 2 x [64][33], the slice's Wc columns and their
// gradient 2 x [N][33], dc and dpred 2 x [64][N|1], the small vectors, and either (two layers)
// h1[64][Hp] | W2 slice [32][Hp] | dW2 slice [32][Hp] with Hp = ceil16(H) | 1, or the dW1 slice [32][K|1].
__host__ __device__ inline int64_t rc_navar_lds_floats(int N, int H, int K, int layers, int Bmax, int T, int R) {
  if (N < 1 || H < 1 || K < 1 || Bmax < 1 || T < 1 || R < 1) return 0;
  if (N > 32 || H > 512 || K > 64 || Bmax > 512 || R > RC_MAX_ACTIVE || layers < 1 || layers > 2 || T < K + 1) return 0;
  const int64_t Kp = K | 1, Np = N | 1;
  const int64_t big = layers == 2 ? 128 * (int64_t)rc_navar_hp(H) : 32 * Kp;
  const int64_t f = NV_BC * Kp + 2 * NV_BC * 33 + 66 * (int64_t)N + 2 * NV_BC * Np + NV_MISC + big;
  return f <= RC_LDS_MAX_FLOATS ? f : 0;
}

// Workspace floats of one stepped replica: P[N][nS][B][N] | D[N][nS][B][H] (two layers) | dbiases[32].
__host__ __device__ inline int64_t rc_navar_ws_floats(int N, int H, int two, int B) {
  const int64_t nS = rc_navar_slices(H);
  return (int64_t)N * nS * B * N + (two ? (int64_t)N * nS * B * H : 0) + 32;
}

// One step (TRAIN) or one chunk of rows (FORWARD): the three launches read the same context.
struct NavarCtx {
  int N, H, K, T, two, B, Bi, mode, t, step, nsteps;  // Bi: this step's windows; t: its Adam step number
  int nrep, rident, launches;  // launches: 0 = all, else a mask of 1 fwd | 2 bwd | 4 in (profiling)
  int64_t q0;         // TRAIN: the step's first index into perm; FORWARD: the chunk's first row
  int64_t out0;       // FORWARD: the chunk's first row in pred / contrib
  int64_t nX, nout;   // rows of a window set / of the FORWARD outputs per replica
  int64_t xps, pps, fs, wss;
  const float* X; const int32_t* perm;
  float* par; float* pm; float* pv;
  const RedcliffReplicaHyper* hyp;
  float* ws;
  float* mse; float* l1; float* pred; float* contrib;
  NvOff o;
  uint8_t rmap[RC_MAX_ACTIVE];
};

int rc_launch_navar_step(const NavarCtx& c, hipStream_t s);
int rc_launch_navar_forward(const NavarCtx& c, hipStream_t s);
