// rc_navar_lstm.h -- context, packed layout, workspace and limits of the NAVAR (LSTM) baseline kernels
// (rc_navar_lstm.hip).
#pragma once
#include "rc_common.h"

#define NL_BC 64  // windows per pass over a batch
#define NL_UL 16  // hidden units per workgroup (the unit slice): 64 gate rows

// Offsets (floats) of a replica's packed block, gate order i, f, g, o:
// Wih[N][4H] | Whh[N][4H][H] | bih[N][4H] | bhh[N][4H] | Wfc[N][N][H] | bfc[N][N] | biases[N]
struct NlOff {
  int64_t Wih, Whh, bih, bhh, Wfc, bfc, bias, total;
};
__host__ __device__ inline NlOff rc_navar_lstm_off(int N, int H) {
  NlOff o;
  int64_t at = 0;
  o.Wih = at; at += (int64_t)N * 4 * H;
  o.Whh = at; at += (int64_t)N * 4 * H * H;
  o.bih = at; at += (int64_t)N * 4 * H;
  o.bhh = at; at += (int64_t)N * 4 * H;
  o.Wfc = at; at += (int64_t)N * N * H;
  o.bfc = at; at += (int64_t)N * N;
  o.bias = at; at += N;
  o.total = at;
  return o;
}

__host__ __device__ inline int rc_navar_lstm_hp(int H) { return ((H + 15) / 16 * 16) | 1; }
__host__ __device__ inline int rc_navar_lstm_slices(int H) { return (H + NL_UL - 1) / NL_UL; }

// LDS floats of the backward workgroup (the largest), 0 outside the limits: the one formula behind
// redcliff_navar_lstm_supported, redcliff_navar_lstm_run and the launches (redcliff_amd/navar_lstm.py
// restates it).  The slice's 64 Whh rows Ws[64][Hp] with Hp = ceil16(H) | 1, the pass's gate gradients
// dg[64][65], its contribution gradients dcs[64][N|1], its h_t slice hs[64][17], the slice's Wfc columns
// and their gradient 2 x [N][17], and xs[64] | gb[64] | gWih[64] | Adam scalars, spare [192].
__host__ __device__ inline int64_t rc_navar_lstm_lds_floats(int N, int H, int Tp, int Bmax, int R) {
  if (N < 1 || H < 1 || Tp < 1 || Bmax < 1 || R < 1) return 0;
  if (N > 32 || H > 448 || Tp > 64 || Bmax > 512 || R > RC_MAX_ACTIVE) return 0;
  const int64_t f = 64 * (int64_t)rc_navar_lstm_hp(H) + 64 * 65 + 64 * (int64_t)(N | 1) + 64 * 17 + 34 * (int64_t)N + 384;
  return f <= RC_LDS_MAX_FLOATS ? f : 0;
}

// Regions (floats) of one stepped replica's workspace at batch size B:
// Hs[N][T'][B][H] | Cs[N][T'][B][H] | Gs[N][T'][B][4H] (TRAIN: gates, then their pre-activation
// gradients) | D[2][N][nS][B][H] (dh partials of the unit slices, double-buffered over t) |
// carry[N][B][H] (dc_t f_t) | Con[T'][B][N*N] | DC[T'][B][N*N] | Res[B][N] | G[packed block] (gradients)
struct NlWs {
  int64_t Hs, Cs, Gs, D, carry, Con, DC, Res, G, total;
};
__host__ __device__ inline NlWs rc_navar_lstm_ws(int N, int H, int Tp, int B, int train) {
  NlWs w;
  int64_t at = 0;
  const int64_t nS = rc_navar_lstm_slices(H), NH = (int64_t)N * Tp * B * H;
  w.Hs = at; at += NH;
  w.Cs = at; at += NH;
  w.Gs = at; at += train ? 4 * NH : 0;
  w.D = at; at += train ? 2 * (int64_t)N * nS * B * H : 0;
  w.carry = at; at += train ? (int64_t)N * B * H : 0;
  w.Con = at; at += train ? (int64_t)Tp * B * N * N : 0;
  w.DC = at; at += train ? (int64_t)Tp * B * N * N : 0;
  w.Res = at; at += train ? (int64_t)B * N : 0;
  w.G = at; at += train ? rc_navar_lstm_off(N, H).total : 0;
  w.total = (at + 63) & ~(int64_t)63;
  return w;
}

// One step (TRAIN) or one chunk of rows (FORWARD): every launch reads the same context.
struct NavarLstmCtx {
  int N, H, Tp, T, B, Bi, mode, at, step, nsteps;  // Bi: this step's windows; at: its Adam step number
  int nrep, rident, launches;  // launches: 0 = all, else a mask of 1 fwd | 2 out + red | 4 bwd | 8 update
  int64_t q0;         // TRAIN: the step's first index into perm; FORWARD: the chunk's first row
  int64_t out0;       // FORWARD: the chunk's first row in pred / contrib
  int64_t nX, nout;   // rows of a window set / of the FORWARD outputs per replica
  int64_t xps, pps, fs;
  const float* X; const int32_t* perm;
  float* par; float* pm; float* pv;
  const RedcliffReplicaHyper* hyp;
  float* ws;
  float* mse; float* l1; float* pred; float* contrib;
  NlOff o;
  NlWs w;
  uint8_t rmap[RC_MAX_ACTIVE];
};

int rc_launch_navar_lstm_step(const NavarLstmCtx& c, hipStream_t s);
int rc_launch_navar_lstm_forward(const NavarLstmCtx& c, hipStream_t s);
