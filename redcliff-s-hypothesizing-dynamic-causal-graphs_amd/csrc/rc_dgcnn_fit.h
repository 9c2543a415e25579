// rc_dgcnn_fit.h -- context, limits, LDS and workspace layouts of the stand-alone DGCNN baseline fit
// (rc_dgcnn_fit.hip).  The packed parameter block is the embedder's (rc_emb_off): A[n][n] |
// gcW[layers][F][H] | bn_w[F] | bn_b[F] | fc1W[64][n*H] | fc1b[64] | fc2W[C][64] | fc2b[C].
#pragma once
#include "rc_common.h"

#define DG_BC 32     // windows per pass over a batch
#define DG_M1 64     // torcheeg's fc1 width
#define DG_MISC 256  // alpha[8] beta[8] mean[8] inv[8] rs[4] .. | dinv[32] @64 | red (doubles) @128 | cd[32] @160
#define DG_QMAX 32   // layers * F, the graph-conv weight rows a thread accumulates in registers

// Offsets (floats) inside one stepped replica's workspace slice.
struct DgWs {
  int64_t st;   // [nsteps][2][F] doubles: every batch's mean / biased variance
  int64_t P;    // [n][B][64]     fc1 partials per node
  int64_t Rg;   // [n][B][H]      relu(graph conv) per node
  int64_t dW;   // [n][layers*F][H] graph-conv weight gradient partials per node
  int64_t dS;   // [layers][n][n] support gradients (row j by node j; support 0 unused)
  int64_t dgb;  // [n][2][F]      BatchNorm affine gradient partials per node
  int64_t gfc;  // fc2W[C][64] | fc2b[C] | fc1b[64] gradients
  int64_t total;
};
__host__ __device__ inline DgWs rc_dgcnn_ws(int n, int F, int nl, int H, int C, int B, int64_t nsteps) {
  DgWs w;
  int64_t x = 0;
  w.st = x; x += 4 * (int64_t)F * nsteps;
  w.P = x; x += (int64_t)n * B * DG_M1;
  w.Rg = x; x += (int64_t)n * B * H;
  w.dW = x; x += (int64_t)n * nl * F * H;
  w.dS = x; x += (int64_t)nl * n * n;
  w.dgb = x; x += (int64_t)n * 2 * F;
  w.gfc = x; x += (int64_t)C * DG_M1 + C + DG_M1;
  w.total = (x + 63) & ~(int64_t)63;
  return w;
}

// LDS floats of one workgroup, 0 outside the limits: the one formula behind redcliff_dgcnn_fit_supported,
// redcliff_dgcnn_fit_run and the launches (redcliff_amd/dgcnn.py restates it).  A node workgroup holds
// misc | f1 / df1 [Bmax][65] | out / dout [Bmax][C] | fc2W [C][64] | its fc1 block [64][H|1] | R / dZ of a
// pass [32][H|1] | the pass's raw windows [32][F*n] | T, That, dT 3 x [32][layers*F] | L [n][n] | its support
// rows [layers][n] | gcW [layers*F][H|1]; the tail workgroup misc | relu(A), L, dL and the layers' S_i and
// dS_i, (2*layers + 3) matrices [n][n].
__host__ __device__ inline int64_t rc_dgcnn_lds_floats(int n, int F, int nl, int H, int C, int Bmax, int T, int R) {
  if (n < 1 || F < 1 || nl < 1 || H < 1 || C < 1 || Bmax < 1 || T < 1 || R < 1) return 0;
  if (n > 32 || F > 8 || nl > 4 || H > 256 || C > 16 || Bmax > 128 || R > RC_MAX_ACTIVE || T < F) return 0;
  const int64_t Hp = H | 1, nq = (int64_t)nl * F;
  const int64_t node = DG_MISC + (int64_t)Bmax * 65 + (int64_t)Bmax * C + (int64_t)C * DG_M1 + DG_M1 * Hp + DG_BC * Hp +
                       (int64_t)DG_BC * F * n + 3 * DG_BC * nq + (int64_t)n * n + (int64_t)nl * n + nq * Hp;
  const int64_t tail = DG_MISC + (2 * (int64_t)nl + 3) * n * n;
  const int64_t f = node > tail ? node : tail;
  return f <= RC_LDS_MAX_FLOATS ? f : 0;
}

// One step (TRAIN) or one batch of rows (FORWARD): every launch reads the same context.
struct DgCtx {
  int n, F, nl, H, C, T, B, Bi, mode, t, step, nsteps;  // Bi: this step's windows; t: its Adam step number
  int nrep, rident, launches;  // launches: 0 = all, else a mask of 1 fwd | 2 bwd | 4 tail (profiling)
  int has_y;
  int64_t row0;       // the step's first row of X / Y
  int64_t out0;       // FORWARD: the batch's first row in pred
  int64_t nout;       // rows of pred per replica
  int64_t xps, yps, fs, wss;
  const float* X; const float* Y;
  float* par; float* pm; float* pv; float* rm; float* rv;
  const RedcliffReplicaHyper* hyp;
  float* ws;
  float* loss; float* pred;
  EmbOff o;
  DgWs w;
  uint8_t rmap[RC_MAX_ACTIVE];
};

int rc_launch_dgcnn_stats(const DgCtx& c, int64_t row0, int64_t N, hipStream_t s);
int rc_launch_dgcnn_step(const DgCtx& c, hipStream_t s);
int rc_launch_dgcnn_forward(const DgCtx& c, hipStream_t s);
