// rc_score.hip -- scoring whole recordings on gfx950: the DGCNN factor-score embedder in inference
// mode over sliding windows of X[Nrec][T][p], and the per-step graph trace built from its output.
//
// Reference: general_utils/misc.py:57-81 (obtain_factor_score_weightings_across_recording /
// ..._classifications_across_recording: one embedder call per scored step on a batch of one) and
// models/redcliff_s_cmlp_withStateSmoothing.py:481-498, :565-580 (the conditional graph of a
// window); the embedder's arithmetic is torcheeg 1.1.3 DGCNN (oracle/torcheeg_dgcnn.py:114-120).
//
// Scored step j of a recording uses rows [start + j*stride - F, start + j*stride) as a time-major
// window; the windows are never materialised.  A workgroup scores a tile of up to 16 consecutive
// steps of one recording and stages the tile's span of rows into LDS once (tile + F - 1 rows at
// stride 1).
//
// BatchNorm (running statistics) scales by the lag index f, the Chebyshev filter mixes channels, so
// the two commute: with Y_i[t][ch] = sum_cc S_i[ch][cc] X[t][cc] formed ONCE per staged row,
//   T_i[ch][f] = alpha[f] Y_i[t0 + f][ch] + beta[f] rowsum(S_i)[ch]
//   Z[ch][hh]  = Zb[ch][hh] + sum_{i,f} Y_i[t0 + f][ch] Wf_i[f][hh]
// with the folded tables Wf_i[f][hh] = alpha[f] W_i[f][hh] and
// Zb[ch][hh] = sum_i rowsum(S_i)[ch] sum_f beta[f] W_i[f][hh], which a prologue kernel writes into
// the call's workspace (k_score_tables, after the supports of redcliff_dgcnn_supports' kernel).
//
// Contractions on v_mfma_f32_16x16x4_f32, rows = the tile's windows:
//   feature:  M = 16 windows, N = 16 hidden columns of one channel, K = n*F   (A from the staged rows)
//   fc1:      M = 16 windows, N = M1, K = the 16 relu(Z) columns just formed  (accumulated over p*H)
// A wave owns the (channel, 16-column) items wv, wv + 4, ... in ascending order and accumulates its
// own fc1 partial; the four partials are summed in wave order.  Nothing depends on the tile's
// position, count, stride or Nrec, so a window's bits do not either.  No atomics, no scratch.
//
// Packs (redcliff_score_recording_pack): the same kernels with the replica on a grid axis.  A
// workgroup of replica r reads r's embedder block, tables and recordings through replica strides
// and writes row i of the outputs, i the replica's place in the active list; everything after the
// base pointers is the single-model code, so a window's bits depend on the dims alone -- not on R,
// the replica's index, the active list or whether the recordings are shared.  The single-model
// entry is the pack of one replica with all strides 0.
#include <cstring>

#include "rc_common.h"

#define SC_TW 16        // windows per tile (MFMA rows)
#define SC_WAVES 4
#define SC_RP 17        // row pitch of a wave's relu tile
#define SC_TAIL_FLOATS (SC_WAVES * SC_TW * 64 + SC_TW * 64)  // fc1 partials of the 4 waves + relu(f1)

struct ScoreCtx {
  RedcliffDims d;
  EmbOff eo;
  const float* emb; int64_t es;  // replica stride of the embedder blocks (floats)
  const float* X; int64_t xrs;   // recording stride (floats)
  int64_t xps;                   // replica stride of the recording sets (0: shared)
  int64_t wss;                   // replica stride of S / Wf / Zb (the call's workspace)
  int start, count, stride;
  int tw;     // scored steps per tile (<= SC_TW; fewer when the stride spreads a tile's rows too far)
  int rowsP;  // LDS rows per (support, channel)
  int ufa;    // use_final_activation
  const float* S;   // [n][p][p]
  const float* Wf;  // [n][F][H]
  const float* Zb;  // [p][H]
  float* w;         // [nrep][Nrec][count][K]
  float* logits;    // [nrep][Nrec][count][nsup] or null
  // blockIdx.z = i-th active replica: replica rmap[i], or i when rident (as StepCtx)
  int rident;
  uint8_t rmap[RC_MAX_ACTIVE];
};

namespace {

// Folded tables of one call.  grid (ceil(max(n F H, p H) / 256), R): replica blockIdx.y reads its
// embedder block (stride es), running statistics (stride bns) and supports, and writes its tables
// (stride wss).
__global__ __launch_bounds__(RC_BLOCK) void k_score_tables(RedcliffDims d, EmbOff eo, const float* emb, int64_t es,
                                                           const float* rm, const float* rv, int64_t bns, float bn_eps,
                                                           const float* S, float* Wf, float* Zb, int64_t wss) {
  const int p = d.p, F = d.F, H = d.H, n = d.n;
  const int e = blockIdx.x * RC_BLOCK + threadIdx.x;
  const int64_t rep = blockIdx.y;
  emb += rep * es; rm += rep * bns; rv += rep * bns;
  S += rep * wss; Wf += rep * wss; Zb += rep * wss;
  const float* W = emb + eo.gcW;
  // torch batch_norm in eval mode: y = x * alpha + beta
  auto alpha = [&](int f) { return (1.0f / sqrtf(rv[f] + bn_eps)) * emb[eo.bnw + f]; };
  if (e < n * F * H) {
    const int f = (e / H) % F;
    Wf[e] = alpha(f) * W[e];
  }
  if (e < p * H) {
    const int ch = e / H, hh = e - ch * H;
    float z = 0.f;
    for (int i = 0; i < n; ++i) {
      float rs = 1.f;  // S_0 = I
      if (i > 0) {
        rs = 0.f;
        for (int cc = 0; cc < p; ++cc) rs += S[(i * p + ch) * p + cc];
      }
      float cb = 0.f;
      for (int f = 0; f < F; ++f) {
        const float beta = emb[eo.bnb + f] - rm[f] * alpha(f);
        cb += beta * W[(i * F + f) * H + hh];
      }
      z += rs * cb;
    }
    Zb[e] = z;
  }
}

// grid (tiles, Nrec, active replicas), 256 threads.  Dynamic LDS: Yl[n][p][rowsP] | Wl[n F][H] | relu tiles
// [4][16][SC_RP]; the first SC_TAIL_FLOATS are reused by the fc1 / fc2 tail.
__global__ __launch_bounds__(RC_BLOCK) void k_score_windows(ScoreCtx c) {
  extern __shared__ float sm[];
  const RedcliffDims& d = c.d;
  const int p = d.p, F = d.F, H = d.H, n = d.n, M1 = d.M1, K = d.K;
  const int nF = n * F, pH = p * H, rowsP = c.rowsP;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int r = blockIdx.y;
  const int j0 = blockIdx.x * c.tw;
  const int nw = min(c.tw, c.count - j0);
  if (nw <= 0) return;
  const int nrows = (nw - 1) * c.stride + F;  // <= rowsP (host)
  // first row of the tile: >= 0 (start >= F); last row start + (j0 + nw - 1) stride - 1 < T (host)
  const int ri = blockIdx.z;                                     // row of the outputs
  const int64_t rep = c.rident ? ri : (int)c.rmap[ri];           // replica
  const float* Xr = c.X + rep * c.xps + (int64_t)r * c.xrs + ((int64_t)c.start + (int64_t)j0 * c.stride - F) * p;
  const float* E = c.emb + rep * c.es;
  const float* Sg = c.S + rep * c.wss;
  const float* Wfg = c.Wf + rep * c.wss;
  const float* Zbg = c.Zb + rep * c.wss;

  float* Yl = sm;                       // [n][p][rowsP]
  float* Wl = Yl + n * p * rowsP;       // [nF][H]
  float* Rt = Wl + nF * H + wv * (SC_TW * SC_RP);  // this wave's relu tile

  for (int e = tid; e < nrows * p; e += RC_BLOCK) {
    const int row = e / p, ch = e - row * p;
    Yl[ch * rowsP + row] = Xr[e];
  }
  for (int e = tid; e < nF * H; e += RC_BLOCK) Wl[e] = Wfg[e];
  __syncthreads();
  // Y_i = S_i X for i >= 1, once per staged row (row fastest: a wave reads one S row at a time)
  for (int e = tid; e < (n - 1) * p * nrows; e += RC_BLOCK) {
    const int rem = e / nrows, row = e - rem * nrows;
    const int i1 = rem / p, ch = rem - i1 * p;
    const float* Srow = Sg + ((int64_t)(i1 + 1) * p + ch) * p;
    float v = 0.f;
    for (int cc = 0; cc < p; ++cc) v += Srow[cc] * Yl[cc * rowsP + row];
    Yl[((i1 + 1) * p + ch) * rowsP + row] = v;
  }
  __syncthreads();

  const int nt = (H + 15) >> 4, items = p * nt;
  const int MT = (M1 + 15) >> 4;
  const float* W1 = E + c.eo.fc1W;
  f32x4 facc[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) facc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool wrow = l15 < nw;
  const int i_first = g / F, f_first = g - i_first * F;
  for (int it = wv; it < items; it += SC_WAVES) {
    const int ch = it / nt, hh0 = (it - ch * nt) << 4;
    // fc1 operands of this item: B[k = 4 g + u][m = 16 mt + l15], issued before the feature product
    float bw[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = mt * 16 + l15;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int hh = hh0 + 4 * g + u;
        bw[mt][u] = (mt < MT && m < M1 && hh < H) ? W1[(int64_t)m * pH + ch * H + hh] : 0.f;
      }
    }
    // Z tile: rows = windows, columns hh0 + l15, k = i F + f ascending in steps of 4
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int i = i_first, f = f_first;
    const bool col = hh0 + l15 < H;
    for (int kk = g; kk - g < nF; kk += 4) {
      const bool kin = kk < nF;
      const float av = (kin && wrow) ? Yl[(i * p + ch) * rowsP + l15 * c.stride + f] : 0.f;
      const float bv = (kin && col) ? Wl[kk * H + hh0 + l15] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      f += 4;
      while (f >= F) { f -= F; ++i; }
    }
    const float zb = col ? Zbg[ch * H + hh0 + l15] : 0.f;
    __builtin_amdgcn_wave_barrier();  // the previous item's tile reads are done
#pragma unroll
    for (int q = 0; q < 4; ++q) Rt[(4 * g + q) * SC_RP + l15] = fmaxf(acc[q] + zb, 0.f);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float av = Rt[l15 * SC_RP + 4 * g + u];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        if (mt < MT) facc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[mt][u], facc[mt], 0, 0, 0);
    }
  }
  __syncthreads();  // Yl / Wl are dead: the tail reuses the front of the LDS
  float* red = sm;                            // [4][16][64]
  float* f1l = sm + SC_WAVES * SC_TW * 64;    // [16][64]
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int q = 0; q < 4; ++q) red[(wv * SC_TW + 4 * g + q) * 64 + mt * 16 + l15] = facc[mt][q];
  __syncthreads();
  for (int e = tid; e < SC_TW * M1; e += RC_BLOCK) {
    const int s = e / M1, m = e - s * M1;
    const float v = ((red[s * 64 + m] + red[(SC_TW + s) * 64 + m]) + red[(2 * SC_TW + s) * 64 + m]) +
                    red[(3 * SC_TW + s) * 64 + m];
    f1l[s * 64 + m] = fmaxf(v + E[c.eo.fc1b + m], 0.f);
  }
  __syncthreads();
  const int nsup = d.nsup;
  for (int e = tid; e < nw * K; e += RC_BLOCK) {
    const int s = e / K, k = e - s * K;
    const float* w2 = E + c.eo.fc2W + k * M1;
    float a = 0.f;
    for (int m = 0; m < M1; ++m) a += w2[m] * f1l[s * 64 + m];
    const float raw = a + E[c.eo.fc2b + k];
    const int64_t win = ((int64_t)ri * gridDim.y + r) * c.count + j0 + s;
    c.w[win * K + k] = d.use_sigmoid ? rc_sigmoid(d.sigmoid_ecc * raw) : raw;
    if (k < nsup && c.logits) c.logits[win * nsup + k] = (d.use_sigmoid && c.ufa) ? rc_sigmoid(raw) : raw;
  }
}

// Graph trace: out[win][q] = bias[q] + sum_k w[win][k] tab[k][q], k ascending.  One workgroup per 16
// consecutive windows of the flattened [Nrec * count] axis of one output row; grid (blocks, rows).
// Row i holds the i-th active replica, which reads its own tab[K][Q] / bias[Q] (replica stride
// K Q / Q; the single-model call is one row of replica 0).
struct GraphReps {
  int rident;
  uint8_t rmap[RC_MAX_ACTIVE];
};
__global__ __launch_bounds__(RC_BLOCK) void k_score_graphs(const float* w, const float* tab, const float* bias, float* out,
                                                           int K, int Q, int64_t nwin, GraphReps gr) {
  __shared__ float wl[SC_TW * 16];
  const int64_t w0 = (int64_t)blockIdx.x * SC_TW;
  const int nw = (int)min((int64_t)SC_TW, nwin - w0);
  if (nw <= 0) return;
  const int ri = blockIdx.y;
  const int64_t rep = gr.rident ? ri : (int)gr.rmap[ri];
  w += (int64_t)ri * nwin * K;
  out += (int64_t)ri * nwin * Q;
  tab += rep * K * Q;
  if (bias) bias += rep * Q;
  for (int e = threadIdx.x; e < nw * K; e += RC_BLOCK) wl[e] = w[w0 * K + e];
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += RC_BLOCK) {
    const float b = bias ? bias[q] : 0.f;
    for (int s = 0; s < nw; ++s) {
      float a = b;
      for (int k = 0; k < K; ++k) a += wl[s * K + k] * tab[(int64_t)k * Q + q];
      out[(w0 + s) * (int64_t)Q + q] = a;
    }
  }
}

}  // namespace

// LDS rows per (support, channel) the window kernel can hold beside its tables; 0 when not even one
// stride-1 tile fits.
int rc_score_rows_budget(const RedcliffDims& d) {
  const int64_t fixed = (int64_t)d.n * d.F * d.H + SC_WAVES * SC_TW * SC_RP;
  const int64_t rows = ((int64_t)RC_LDS_MAX_FLOATS - fixed) / ((int64_t)d.n * d.p);
  return rows >= d.F + SC_TW - 1 ? (int)(rows > (1 << 20) ? (1 << 20) : rows) : 0;
}

int rc_launch_score_tables(const RedcliffDims& d, const EmbOff& eo, const float* emb, const float* rm, const float* rv,
                           float bn_eps, const float* S, float* Wf, float* Zb, hipStream_t s, const ScoreReps* reps) {
  const int nE = d.n * d.F * d.H > d.p * d.H ? d.n * d.F * d.H : d.p * d.H;
  const int R = reps ? reps->R : 1;
  hipLaunchKernelGGL(k_score_tables, dim3((nE + RC_BLOCK - 1) / RC_BLOCK, R), dim3(RC_BLOCK), 0, s, d, eo, emb,
                     reps ? reps->es : 0, rm, rv, reps ? reps->bns : 0, bn_eps, S, Wf, Zb, reps ? reps->wss : 0);
  return rc_check(hipGetLastError(), "k_score_tables");
}

int rc_launch_score_windows(const RedcliffDims& d, const EmbOff& eo, const float* emb, const float* X, int64_t xrs,
                            int Nrec, int start, int count, int stride, int ufa, const float* S, const float* Wf,
                            const float* Zb, float* w, float* logits, hipStream_t s, const ScoreReps* reps) {
  const int budget = rc_score_rows_budget(d);
  if (budget <= 0) { rc_set_error("score_recording: LDS budget exceeded"); return REDCLIFF_ELIMIT; }
  ScoreCtx c;
  memset(&c, 0, sizeof(c));
  c.d = d; c.eo = eo; c.emb = emb; c.X = X; c.xrs = xrs;
  c.start = start; c.count = count; c.stride = stride; c.ufa = ufa;
  c.S = S; c.Wf = Wf; c.Zb = Zb; c.w = w; c.logits = logits;
  c.rident = 1;
  int nrep = 1;
  if (reps) {
    c.es = reps->es; c.xps = reps->xps; c.wss = reps->wss;
    c.rident = reps->rident;
    nrep = reps->nrep;
    if (nrep < 1 || nrep > RC_MAX_ACTIVE) { rc_set_error("score_recording: %d active replicas", nrep); return REDCLIFF_ELIMIT; }
    memcpy(c.rmap, reps->rmap, sizeof(c.rmap));
  }
  // as many steps per tile as the staged span allows (the arithmetic of a window does not depend on it)
  int tw = SC_TW;
  if ((int64_t)(SC_TW - 1) * stride + d.F > budget) tw = (int)(((int64_t)budget - d.F) / stride) + 1;
  c.tw = tw;
  const int rows = (tw - 1) * stride + d.F;
  c.rowsP = rows | 1;  // odd pitch (budget leaves the slack: fixed part rounded below)
  if ((int64_t)c.rowsP > budget) c.rowsP = rows;
  size_t lds = (size_t)d.n * d.p * c.rowsP + (size_t)d.n * d.F * d.H + SC_WAVES * SC_TW * SC_RP;
  if (lds < SC_TAIL_FLOATS) lds = SC_TAIL_FLOATS;
  lds *= sizeof(float);
  const int64_t tiles = ((int64_t)count + tw - 1) / tw;
  if (Nrec > 65535 || tiles > 0x7fffffff) { rc_set_error("score_recording: grid too large (Nrec <= 65535)"); return REDCLIFF_ELIMIT; }
  int e = rc_lds_optin(k_score_windows, lds, "k_score_windows LDS");
  if (e) return e;
  hipLaunchKernelGGL(k_score_windows, dim3((unsigned)tiles, Nrec, nrep), dim3(RC_BLOCK), lds, s, c);
  return rc_check(hipGetLastError(), "k_score_windows");
}

int rc_launch_score_graphs(const float* w, const float* tab, const float* bias, float* out, int K, int Q, int64_t nwin,
                           hipStream_t s, const ScoreReps* reps) {
  const int64_t nb = (nwin + SC_TW - 1) / SC_TW;
  if (nb > 0x7fffffff) { rc_set_error("score_recording: too many windows for the graph trace"); return REDCLIFF_ELIMIT; }
  GraphReps gr;
  memset(&gr, 0, sizeof(gr));
  gr.rident = 1;
  int nrep = 1;
  if (reps) {
    gr.rident = reps->rident;
    nrep = reps->nrep;
    if (nrep < 1 || nrep > RC_MAX_ACTIVE) { rc_set_error("score_recording: %d active replicas", nrep); return REDCLIFF_ELIMIT; }
    memcpy(gr.rmap, reps->rmap, sizeof(gr.rmap));
  }
  hipLaunchKernelGGL(k_score_graphs, dim3((unsigned)nb, nrep), dim3(RC_BLOCK), 0, s, w, tab, bias, out, K, Q, nwin, gr);
  return rc_check(hipGetLastError(), "k_score_graphs");
}
