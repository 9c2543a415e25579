// rc_lstm_fm.h -- context and limits of the cLSTM_FM baseline epoch kernel (rc_lstm_fm.hip), shared
// by the kernel, its launch and the C-ABI entries redcliff_lstm_fm_supported / redcliff_lstm_fm_run.
#pragma once
#include "rc_common.h"

#define LF_BC 32     // sequences staged per pass over a batch
// Explicit caps; the LDS footprint below binds first (h <= 35 at p = 4, C = 2; h <= 33 at p = 10, C = 2;
// p <= 35 at h = 25, C = 2; C <= 34 at p = 4, h = 5; C <= 4 at p = 10, h = 25).
#define LF_MAX_P 64
#define LF_MAX_H 64
#define LF_MAX_C 64
#define LF_MAX_B 512

// One launch of k_lstm_fm_epoch: grid (p, stepped replicas).
struct LstmFmCtx {
  int p, h, C, T, S, B, flags, tB, nsteps;  // S = tmax - C sequences per recording
  int nrep, rident;   // stepped replicas; rident: all R in order, else rmap
  int64_t row0, N;    // recordings [row0, row0 + N) in batches of B
  int64_t xps, fs;    // replica strides (floats) of the recording sets (0: shared) / the parameter blocks
  const float* X;
  float* fac; float* facM; float* facV;
  const RedcliffReplicaHyper* hyp;
  float* sse; float* pen;  // [nrep][nsteps][p]
  float* G;                // [R][p][p] of the final weights (may be null)
  uint8_t rmap[RC_MAX_ACTIVE];
};

// LDS floats of one workgroup (the one formula behind redcliff_lstm_fm_supported,
// redcliff_lstm_fm_run and the launch).  With K = p + h, Kp = K | 1:
//   np = 4h*Kp + 8h + h + 1   network j's [Wih | Whh] rows padded to an odd stride, bih, bhh, Wl, bl
//   4 * np                    the parameters, exp_avg, exp_avg_sq and the gradient accumulators
//   LF_BC * (zs + gs + cs + 2*(h|1) + 2C)   per staged sequence: [x_t | h_{t-1}] for t = 0..C
//                             (zs = (C+1)K | 1), the four gates per t (gs = 4hC | 1; overwritten by
//                             their pre-activation gradients in the backward), the cell state per t
//                             (cs = hC | 1), dL/dh and dL/dc carried to t-1, targets and dL/dy per t
//   p + 16                    the column norms G[c], the block-sum slots and the step's Adam scalars
__host__ __device__ inline int64_t rc_lstm_fm_lds_floats(int p, int h, int C) {
  const int64_t K = (int64_t)p + h, Kp = K | 1, hp = h | 1;
  const int64_t np = 4 * (int64_t)h * Kp + 9 * (int64_t)h + 1;
  const int64_t zs = ((int64_t)(C + 1) * K) | 1, gs = (4 * (int64_t)h * C) | 1, cs = ((int64_t)h * C) | 1;
  return 4 * np + LF_BC * (zs + gs + cs + 2 * hp + 2 * (int64_t)C) + p + 16;
}

int rc_launch_lstm_fm(const LstmFmCtx& c, hipStream_t s);
