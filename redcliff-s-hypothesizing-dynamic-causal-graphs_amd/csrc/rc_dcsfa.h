// rc_dcsfa.h -- context, limits, packed-parameter, LDS and workspace layouts of the dCSFA-NMF baseline fit
// (rc_dcsfa.hip).  The packed block of one model:
//   W_nmf[K][D] | W1[H][D] | b1[H] | bn_w[H] | bn_b[H] | W2[K][H] | b2[K] | phi[ns] | beta[ns]
#pragma once
#include "rc_common.h"

#define DC_HS 8      // hidden units per slice workgroup
#define DC_BC 32     // rows per pass of the slice forward's window block
#define DC_KMAX 8    // components (register arrays of the head and the slice backward)
#define DC_BMAX 128  // rows of a batch
#define DC_MISC 128  // small per-workgroup tables

struct DcOff {
  int64_t Wn, W1, b1, bnw, bnb, W2, b2, phi, beta, total;
};
__host__ __device__ inline DcOff rc_dcsfa_off(int D, int H, int K, int ns) {
  DcOff o;
  int64_t x = 0;
  o.Wn = x; x += (int64_t)K * D;
  o.W1 = x; x += (int64_t)H * D;
  o.b1 = x; x += H;
  o.bnw = x; x += H;
  o.bnb = x; x += H;
  o.W2 = x; x += (int64_t)K * H;
  o.b2 = x; x += K;
  o.phi = x; x += ns;
  o.beta = x; x += ns;
  o.total = x;
  return o;
}

__host__ __device__ inline int rc_dcsfa_slices(int H) { return (H + DC_HS - 1) / DC_HS; }

// Offsets (floats) inside one replica's workspace slice.
struct DcWs {
  int64_t a;     // [B][nsl*8]  LeakyReLU(BatchNorm) activations
  int64_t xh;    // [B][nsl*8]  normalised pre-activations (z - mean) * invstd
  int64_t inv;   // [nsl*8]     invstd of the step
  int64_t P;     // [nsl][B][K] partials of the h -> K layer per slice
  int64_t dpre;  // [B][K]      dL/d(pre-softplus scores)
  int64_t total;
};
__host__ __device__ inline DcWs rc_dcsfa_ws(int H, int K, int B) {
  DcWs w;
  const int64_t Hp = (int64_t)rc_dcsfa_slices(H) * DC_HS;
  int64_t x = 0;
  w.a = x; x += (int64_t)B * Hp;
  w.xh = x; x += (int64_t)B * Hp;
  w.inv = x; x += Hp;
  w.P = x; x += (int64_t)rc_dcsfa_slices(H) * B * K;
  w.dpre = x; x += (int64_t)B * K;
  w.total = (x + 63) & ~(int64_t)63;
  return w;
}

// LDS floats of one workgroup, 0 outside the limits: the one formula behind redcliff_dcsfa_supported,
// redcliff_dcsfa_run and the launches (redcliff_amd/dcsfa_nmf.py restates it).
//   slice forward: misc | rows [B] | z [B][8] | W1 slice [8][D|1] | the pass's rows of X [32][D|1]
//   head:          misc | rows [B] | 7 tables [B][K] | 4 matrices [K][K] | softplus(W_nmf) [K][D|1]
//   slice backward: misc | rows [B] | dpre [B][K] | a, xhat, dz [B][8] | W2 slice [K][8]
__host__ __device__ inline int64_t rc_dcsfa_lds_floats(int D, int H, int K, int ns, int B, int R) {
  if (D < 1 || H < 1 || K < 1 || ns < 1 || B < 1 || R < 1) return 0;
  if (K > DC_KMAX || ns > K || B > DC_BMAX || R > RC_MAX_ACTIVE || H > 4096 || D > 4096) return 0;
  const int64_t Dp = D | 1;
  const int64_t fwd = DC_MISC + B + (int64_t)B * DC_HS + DC_HS * Dp + DC_BC * Dp;
  const int64_t head = DC_MISC + B + 7 * (int64_t)B * K + 4 * K * K + K * Dp;
  const int64_t bwd = DC_MISC + B + (int64_t)B * K + 3 * (int64_t)B * DC_HS + K * DC_HS;
  int64_t f = fwd > head ? fwd : head;
  if (bwd > f) f = bwd;
  return f <= RC_LDS_MAX_FLOATS ? f : 0;
}

// One step (TRAIN / PRETRAIN) or one batch of rows (EVAL): every launch reads the same context.
struct DcCtx {
  int D, H, K, ns, B, Bi, mode, nsl, nrep, step;
  int64_t row0;  // EVAL: the batch's first row
  int64_t N;     // rows of X / Y / TM / PW per replica
  int64_t xps, yps, pps, ips, fs, wss, evs;
  const float* X; const float* Y; const float* TM; const float* PW;
  const int32_t* idx;
  float* par; float* pm; float* pv; float* rm; float* rv;
  float* ws; float* loss; double* ev;
  int nsteps, nev;
  float recon_w, sup_w, sup_recon_w, smooth;
  double bn_eps, bn_mom;
  float decay, neg_step, bc2s, eps, b2, omb1, omb2;  // AdamW scalars of this step
  DcOff o;
  DcWs w;
};

int rc_launch_dcsfa_step(const DcCtx& c, hipStream_t s);
int rc_launch_dcsfa_eval(const DcCtx& c, hipStream_t s);
