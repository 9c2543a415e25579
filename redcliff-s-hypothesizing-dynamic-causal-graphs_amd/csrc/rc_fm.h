// rc_fm.h -- context and limits of the cMLP_FM baseline epoch kernel (rc_fm.hip), shared with the
// C-ABI entries in rc_capi.hip.
#pragma once
#include "rc_common.h"

#define FM_BC 64  // windows staged per pass over a batch

// One launch of k_fm_epoch: grid (p, stepped replicas).
struct FmCtx {
  int p, L, h, T, B, flags, tB, nsteps;
  int nrep, rident;   // stepped replicas; rident: all R in order, else rmap
  int64_t row0, N;    // windows [row0, row0 + N) in batches of B
  int64_t xps, fs;    // replica strides (floats) of the window sets (0: shared) / the factor blocks
  const float* X;
  float* fac; float* facM; float* facV;
  const RedcliffReplicaHyper* hyp;
  float* sse; float* pen;  // [nrep][nsteps][p]
  float* G; float* G0;     // [R][p][p][L] / [R][p][p] of the final weights (may be null)
  FacOff fo;
  uint8_t rmap[RC_MAX_ACTIVE];
};

// LDS floats of one workgroup (the one formula behind redcliff_fm_supported, redcliff_fm_run and the
// launch): network j's W0 rows padded to an odd stride with b0 | W1 | b1, the same again for exp_avg
// and exp_avg_sq, the dW0 accumulators, FM_BC staged windows (inputs, hidden activations, target,
// dL/dy), the group norms G[q] | G0[c] and the step's Adam scalars.
__host__ __device__ inline int64_t rc_fm_lds_floats(int p, int L, int h) {
  const int64_t Q = (int64_t)p * L, Qp = Q | 1, hp = h | 1;
  const int64_t np = h * Qp + 2 * h + 1;
  return 3 * np + h * Qp + FM_BC * (Qp + hp + 2) + Q + p + 8;
}

int rc_launch_fm(const FmCtx& c, hipStream_t s);
