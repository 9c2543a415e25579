// rc_score_cemb.hip -- scoring whole recordings of cEmbedder models on gfx950: the K channel MLPs
// Conv1d(p, eh, F) -> ReLU -> 1x1 Conv1d of the factor-score embedder over sliding windows of
// X[Nrec][T][p].  The graph trace of the scores is rc_score.hip's k_score_graphs, unchanged.
//
// Reference: general_utils/misc.py:57-81 (one embedder call per scored step on a batch of one) and
// models/redcliff_factor_score_embedders.py:236-273 (cEmbedder.forward; models/cmlp.py:12-35 the
// networks).  Over a recording the first layer is a 1-D convolution in time: scored step j of a
// recording uses rows [start + j*stride - F, start + j*stride) as a time-major window, and the F-fold
// overlap of consecutive windows is never materialised.  The cEmbedder reads the window time-major at
// every p (no p == F special case) and has no BatchNorm.
//
// A workgroup scores a tile of up to 64 consecutive steps of one recording and stages the tile's span
// of rows, (tw - 1) stride + F of them, into LDS once, channel-major with an odd row pitch.  When a
// large stride pushes the span past the LDS budget the tile holds fewer steps, down to one.
//
// Contraction on v_mfma_f32_16x16x4_f32: rows = 16 windows, columns = one 16-unit block of one
// network, k = q = c F + f ascending in steps of 4 (the Conv1d weight order), zero-padded past eh and
// past p F.  A wave owns the (network, unit block) items wv, wv + 4, ... in ascending order; for each
// it keeps one accumulator per 16-window group of the tile (up to four: every B fragment is used for
// all of them, and the four MFMA chains are independent), then applies bias and ReLU, multiplies by
// We1 and sums the 16 unit columns in a fixed butterfly (lane distances 1, 2, 4, 8: every lane gets
// the same bits).  A wave adds the unit blocks of one network in ascending order into its own partial
// [network][step] in LDS; the four waves' partials are summed in wave order.  The order of every sum
// is a function of (p, F, eh, K) only: a window's bits do not depend on the tile's position or width,
// count, stride or Nrec.  No atomics, no scratch.
//
// Measured on the MI355X (profiles/score_recording_cemb.json, 131,072 steps, kernel time): four
// groups per tile 0.116 ms at C1 / 1.01 ms at the c4 dims with eh = 100 (37 / 45 TF/s), two groups
// 0.139 / 1.33 ms, one group 0.239 / 2.38 ms; loading the B operands of four k-steps together
// against one by one 0.116 / 1.006 against 0.117 / 1.018 ms.  The output bits of all four builds
// are identical.
#include "rc_common.h"

#ifndef CS_GROUPS
#define CS_GROUPS 4     // 16-window groups per tile (timing experiments build 1 and 2; bits do not depend on it)
#endif
#define CS_TW (16 * CS_GROUPS)  // windows per tile: 64
#define CS_WAVES 4
#ifndef CS_KU
#define CS_KU 4         // k-steps whose B operands are loaded together (the order of the products is unchanged)
#endif
#define CS_RED_FLOATS (CS_WAVES * 16 * 64)  // the waves' partials [4][K <= 16][CS_TW <= 64]
static_assert(CS_GROUPS >= 1 && CS_GROUPS <= 4, "a tile is one to four groups of 16 windows");

struct CEmbScoreCtx {
  int p, F, K, eh, nsup, use_sigmoid, ufa;
  float ecc;
  const float* emb;  // We0[K][eh][p][F] | be0[K][eh] | We1[K][eh] | be1[K]
  const float* X; int64_t xrs;  // recording stride (floats)
  int start, count, stride;
  int tw;     // scored steps per tile (<= CS_TW)
  int rowsP;  // LDS row pitch of a channel
  float* w;         // [Nrec][count][K]
  float* logits;    // [Nrec][count][nsup] or null
};

namespace {

// grid (tiles, Nrec), 256 threads.  Dynamic LDS: Xl[p][rowsP] | red[4][K][64]
__global__ __launch_bounds__(RC_BLOCK) void k_score_cemb(CEmbScoreCtx c) {
  extern __shared__ float sm[];
  const int p = c.p, F = c.F, K = c.K, eh = c.eh, pF = p * F, rowsP = c.rowsP;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int r = blockIdx.y;
  const int j0 = blockIdx.x * c.tw;
  const int nw = min(c.tw, c.count - j0);
  if (nw <= 0) return;
  const int nrows = (nw - 1) * c.stride + F;  // <= rowsP (host)
  // first row of the tile: >= 0 (start >= F); last row start + (j0 + nw - 1) stride - 1 < T (host)
  const float* Xr = c.X + (int64_t)r * c.xrs + ((int64_t)c.start + (int64_t)j0 * c.stride - F) * p;
  const int64_t KE = (int64_t)K * eh;
  const float* We0 = c.emb;
  const float* be0 = We0 + KE * pF;
  const float* We1 = be0 + KE;
  const float* be1 = We1 + KE;

  float* Xl = sm;                // [p][rowsP]
  float* red = sm + p * rowsP;   // [4][K][CS_TW]
  for (int e = tid; e < nrows * p; e += RC_BLOCK) {
    const int row = e / p, ch = e - row * p;
    Xl[ch * rowsP + row] = Xr[e];
  }
  for (int e = tid; e < CS_WAVES * K * CS_TW; e += RC_BLOCK) red[e] = 0.f;
  __syncthreads();

  const int nt = (eh + 15) >> 4, items = K * nt;
  const int ngrp = (nw + 15) >> 4;  // 16-window groups in use (uniform)
  // this lane's window row in each group, and whether that window exists
  int arow[CS_GROUPS];
  bool wrow[CS_GROUPS];
#pragma unroll
  for (int t = 0; t < CS_GROUPS; ++t) {
    wrow[t] = t * 16 + l15 < nw;
    arow[t] = wrow[t] ? (t * 16 + l15) * c.stride : 0;
  }
  const int c_first = g / F, f_first = g - c_first * F;
  float* redw = red + wv * (K * CS_TW);
  for (int it = wv; it < items; it += CS_WAVES) {
    const int k = it / nt, u0 = (it - k * nt) << 4;
    const int u = u0 + l15;
    const bool col = u < eh;
    const float* Brow = We0 + ((int64_t)k * eh + (col ? u : 0)) * pF;
    const float b0 = col ? be0[k * eh + u] : 0.f;
    const float w1 = col ? We1[k * eh + u] : 0.f;
    f32x4 acc[CS_GROUPS];
#pragma unroll
    for (int t = 0; t < CS_GROUPS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int ch = c_first, f = f_first;
    // four k-steps at a time: their B operands are in flight before the first product needs one
    for (int k0 = 0; k0 < pF; k0 += 4 * CS_KU) {
      float bv[CS_KU];
      int xo[CS_KU];
      bool kin[CS_KU];
#pragma unroll
      for (int j = 0; j < CS_KU; ++j) {
        const int kk = k0 + 4 * j + g;
        kin[j] = kk < pF;
        bv[j] = (kin[j] && col) ? Brow[kk] : 0.f;
        xo[j] = kin[j] ? ch * rowsP + f : 0;
        f += 4;
        while (f >= F) { f -= F; ++ch; }
      }
#pragma unroll
      for (int j = 0; j < CS_KU; ++j) {
        if (k0 + 4 * j < pF) {  // uniform: no product past p F
#pragma unroll
          for (int t = 0; t < CS_GROUPS; ++t) {
            if (t < ngrp) {
              const float av = (kin[j] && wrow[t]) ? Xl[xo[j] + arow[t]] : 0.f;
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[t], 0, 0, 0);
            }
          }
        }
      }
    }
    // relu(z) We1 summed over the block's 16 unit columns; rows 4 g + q of each group
#pragma unroll
    for (int t = 0; t < CS_GROUPS; ++t) {
      if (t < ngrp) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = fmaxf(acc[t][q] + b0, 0.f) * w1;
          v += __shfl_xor(v, 1);
          v += __shfl_xor(v, 2);
          v += __shfl_xor(v, 4);
          v += __shfl_xor(v, 8);
          if (l15 == 0) redw[k * CS_TW + t * 16 + 4 * g + q] += v;  // this wave's own partial: unit blocks ascending
        }
      }
    }
  }
  __syncthreads();
  const int nsup = c.nsup;
  for (int e = tid; e < nw * K; e += RC_BLOCK) {
    const int s = e / K, k = e - s * K;
    const float* rk = red + k * CS_TW + s;
    const float raw = be1[k] + (((rk[0] + rk[K * CS_TW]) + rk[2 * K * CS_TW]) + rk[3 * K * CS_TW]);
    const int64_t win = (int64_t)r * c.count + j0 + s;
    c.w[win * K + k] = c.use_sigmoid ? rc_sigmoid(c.ecc * raw) : raw;
    if (k < nsup && c.logits) c.logits[win * nsup + k] = (c.use_sigmoid && c.ufa) ? rc_sigmoid(raw) : raw;
  }
}

}  // namespace

// LDS rows per channel a tile may stage beside the waves' partials; 0 outside the kernel's limits
// (p <= 64, F <= 64, K <= 16, eh <= 128: at those a full stride-1 tile always fits).
int rc_score_cemb_rows_budget(const RedcliffDims& d, int eh) {
  if (d.p < 1 || d.F < 1 || d.K < 1 || eh < 1 || d.p > 64 || d.F > 64 || d.K > 16 || eh > 128) return 0;
  const int rows = (RC_LDS_MAX_FLOATS - CS_RED_FLOATS) / d.p;
  return rows >= d.F + CS_TW - 1 ? rows : 0;
}

int rc_launch_score_cemb(const RedcliffDims& d, int eh, const float* emb, const float* X, int64_t xrs, int Nrec,
                         int start, int count, int stride, int ufa, float* w, float* logits, hipStream_t s) {
  const int budget = rc_score_cemb_rows_budget(d, eh);
  if (budget <= 0) { rc_set_error("cemb_score_recording: dims outside kernel limits"); return REDCLIFF_ELIMIT; }
  CEmbScoreCtx c;
  c.p = d.p; c.F = d.F; c.K = d.K; c.eh = eh; c.nsup = d.nsup; c.use_sigmoid = d.use_sigmoid; c.ufa = ufa;
  c.ecc = d.sigmoid_ecc;
  c.emb = emb; c.X = X; c.xrs = xrs;
  c.start = start; c.count = count; c.stride = stride;
  c.w = w; c.logits = logits;
  // as many steps per tile as the staged span allows (the arithmetic of a window does not depend on it)
  int tw = CS_TW;
  if ((int64_t)(CS_TW - 1) * stride + d.F > budget) tw = (int)(((int64_t)budget - d.F) / stride) + 1;
  c.tw = tw;
  const int rows = (tw - 1) * stride + d.F;  // <= budget
  c.rowsP = rows | 1;                        // odd pitch
  if (c.rowsP > budget) c.rowsP = rows;
  const size_t lds = sizeof(float) * ((size_t)d.p * c.rowsP + (size_t)CS_WAVES * d.K * CS_TW);
  const int64_t tiles = ((int64_t)count + tw - 1) / tw;
  if (Nrec > 65535 || tiles > 0x7fffffff) { rc_set_error("cemb_score_recording: grid too large (Nrec <= 65535)"); return REDCLIFF_ELIMIT; }
  int e = rc_lds_optin(k_score_cemb, lds, "k_score_cemb LDS");
  if (e) return e;
  hipLaunchKernelGGL(k_score_cemb, dim3((unsigned)tiles, Nrec), dim3(RC_BLOCK), lds, s, c);
  return rc_check(hipGetLastError(), "k_score_cemb");
}
