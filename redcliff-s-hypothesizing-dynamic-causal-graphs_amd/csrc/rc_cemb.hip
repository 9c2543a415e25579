// rc_cemb.hip -- the cEmbedder (models/redcliff_factor_score_embedders.py:183-331) as the
// embedder of the fused training step: K copies of models/cmlp.py:12-35 MLP
// (Conv1d(p, eh, F) -> ReLU -> Conv1d(eh, 1, 1)) on the embedder window Xe = X[row][Lmax-F : Lmax].
//
// Kernel chain of one batch_update (...withStateSmoothing.py:734-933), one stream:
//   k_cemb_fwd     w_raw[b][k] = We1[k] . relu(We0[k] Xe[b] + be0[k]) + be1[k]  (-> ws.w, the region
//                  the factor chain mixes with), hidden activations, We1 snapshot, and the group
//                  norms g[k][c][t] / g0[k][c] of We0 (:297-326 without wavelets)
//   k_cemb_tables  E[i][j][t] = sum_k g[k][i][t] g[k][j][t] over the last Ls lags, E0 = sum_k g0 g0^T
//                  (the fixed embedder graph, ...withStateSmoothing.py:500-519)
//   the matrix-core factor chain (rc_factor_mfma.hip) with k_fac_mix<.., CE = true>
//   k_cos_values / the head workgroup (rc_embed.hip) for loss values and the confusion matrix
//   k_cemb_bwd     dL/dw_raw (rc_emb_draw), dWe0 / dbe0 / dWe1 / dbe1, the adjacency-L1 term
//                  through E and the group norms, and the Adam epilogue (rc_adam).
//
// The contractions are vector-FMA register tiles (in-order fmaf chains over q and over the
// batch): the step is launch- and latency-bound at the shapes the models use (q = p*F of
// 64..256, eh ~ 25, B <= 128: ~1 MFLOP per GEMM), and only this form was measured; see DESIGN.md.
// Every sum runs in a fixed order, there are no floating-point atomics, no kernel uses scratch.
#include "rc_common.h"

namespace {

#define CE_BT 32  // windows per forward tile
#define CE_QC 64  // contraction chunk staged per step (forward), dWe0 columns per workgroup (backward)
#define CE_UT 16  // hidden units per backward workgroup
#define CE_BC 32  // windows per backward staging step

// Xe[b][q = ch*F + t] of windows [b0, b0 + 32) x columns [q0, q0 + 64) -> Xs[bb][qq], zero padded
__device__ inline void ce_stage_x(const StepCtx& c, int r, int b0, int q0, float (*Xs)[CE_QC + 1]) {
  const RedcliffDims& d = c.d;
  const int p = d.p, F = d.F, Q = p * F;
  const float* Xg = c.X + r * c.xr + ((c.row0 + b0) * d.T + (c.Lmax - F)) * p;
  for (int e = threadIdx.x; e < CE_BT * CE_QC; e += RC_BLOCK) {
    const int bb = e >> 6, qq = e & 63, q = q0 + qq;
    float v = 0.f;
    if (b0 + bb < c.B && q < Q) {
      const int ch = q / F, t = q - ch * F;
      v = Xg[((int64_t)bb * d.T + t) * p + ch];
    }
    Xs[bb][qq] = v;
  }
}

// grid (K * nbt + K * p, R): workgroups [0, K*nbt) are (network k, tile of 32 windows); thread
// (bq = tid >> 5, ul = tid & 31) owns windows 4 bq + {0..3} x units ul + 32 {0..3}.  The last K*p
// workgroups are (network k, channel c): thread t < F the squared norm over the hidden units.
__global__ __launch_bounds__(RC_BLOCK) void k_cemb_fwd(StepCtx c, CEmbCtx e, int nbt) {
  const RedcliffDims& d = c.d;
  const int r = rc_rep(c, blockIdx.y);
  const int p = d.p, F = d.F, K = d.K, eh = e.eh, Q = p * F, B = c.B;
  const float* P = c.emb + r * c.es;
  float* ws = c.ws + r * c.wss;
  float* cw = e.ws + r * e.wss;
  const int tid = threadIdx.x;
  __shared__ float Xs[CE_BT][CE_QC + 1];
  __shared__ float Ws[128][CE_QC + 1];
  __shared__ float sq[64];
  if ((int)blockIdx.x >= K * nbt) {  // ---- group norms of We0[k][:, ch, :]
    const int idx = blockIdx.x - K * nbt, k = idx / p, ch = idx - k * p;
    const float* W = P + e.po.We0 + (int64_t)k * eh * Q + ch * F;
    if (tid < F) {
      float s = 0.f;
      for (int u = 0; u < eh; ++u) {
        const float w = W[(int64_t)u * Q + tid];
        s = __builtin_fmaf(w, w, s);
      }
      sq[tid] = s;
      cw[e.wo.g + ((int64_t)k * p + ch) * F + tid] = sqrtf(s);
    }
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int i = 0; i < F; ++i) t += sq[i];
      cw[e.wo.g0 + (int64_t)k * p + ch] = sqrtf(t);
    }
    return;
  }
  const int k = blockIdx.x / nbt, b0 = (blockIdx.x - k * nbt) * CE_BT;
  const float* W = P + e.po.We0 + (int64_t)k * eh * Q;
  const int nug = (eh + 31) >> 5;  // 32-unit groups
  const int bq = tid >> 5, ul = tid & 31;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int q0 = 0; q0 < Q; q0 += CE_QC) {
    __syncthreads();
    ce_stage_x(c, r, b0, q0, Xs);
    for (int i = tid; i < nug * 32 * CE_QC; i += RC_BLOCK) {
      const int u = i >> 6, qq = i & 63, q = q0 + qq;
      Ws[u][qq] = (u < eh && q < Q) ? W[(int64_t)u * Q + q] : 0.f;
    }
    __syncthreads();
    const int kmax = min(CE_QC, Q - q0);
    for (int qq = 0; qq < kmax; ++qq) {
      float x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = Xs[bq * 4 + i][qq];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nug) {
          const float w = Ws[ul + 32 * j][qq];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_fmaf(x[i], w, acc[i][j]);
        }
      }
    }
  }
  // ---- epilogue: bias, ReLU, output layer (per lane over its units, then the 32 lanes' butterfly)
  float bu[4], w1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int u = ul + 32 * j;
    const bool uv = u < eh;
    bu[j] = uv ? P[e.po.be0 + (int64_t)k * eh + u] : 0.f;
    w1[j] = uv ? P[e.po.We1 + (int64_t)k * eh + u] : 0.f;
    if (b0 == 0 && bq == 0 && uv) cw[e.wo.w1 + (int64_t)k * eh + u] = w1[j];
  }
  const float b1 = P[e.po.be1 + k];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + bq * 4 + i;
    float ys = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int u = ul + 32 * j;
      if (u < eh) {
        const float a = fmaxf(acc[i][j] + bu[j], 0.f);
        if (b < B) cw[e.wo.ha + ((int64_t)k * d.Bmax + b) * eh + u] = a;
        ys = __builtin_fmaf(w1[j], a, ys);
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) ys += __shfl_xor(ys, o, 64);  // within the 32-lane half
    if (ul == 0 && b < B) ws[c.wo.w + (int64_t)b * K + k] = ys + b1;
  }
}

// grid (p, R): row i of E (last Ls of the F lags) and of E0, sums over k ascending, so
// E[i][j] and E[j][i] are the same bits (a product commutes).
__global__ __launch_bounds__(RC_BLOCK) void k_cemb_tables(StepCtx c, CEmbCtx e) {
  const RedcliffDims& d = c.d;
  const int r = rc_rep(c, blockIdx.y), i = blockIdx.x;
  const int p = d.p, F = d.F, K = d.K, Ls = c.Ls;
  float* cw = e.ws + r * e.wss;
  const float* g = cw + e.wo.g;
  const float* g0 = cw + e.wo.g0;
  for (int x = threadIdx.x; x < p * Ls; x += RC_BLOCK) {
    const int j = x / Ls, t = F - Ls + (x - j * Ls);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = __builtin_fmaf(g[((int64_t)k * p + i) * F + t], g[((int64_t)k * p + j) * F + t], s);
    cw[e.wo.E + (int64_t)i * p * Ls + x] = s;
  }
  for (int j = threadIdx.x; j < p; j += RC_BLOCK) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = __builtin_fmaf(g0[k * p + i], g0[k * p + j], s);
    cw[e.wo.E0 + (int64_t)i * p + j] = s;
  }
}

// grid (K * nut * nqt, R): workgroup (network k, 16-unit tile ut, 64-column tile qt); thread
// (uu = tid >> 4, q4 = tid & 15) owns dWe0[u0 + uu][q0 + q4 + 16 {0..3}].  Every workgroup forms
// dL/dw_raw[:, k] itself (the per-channel partials of the factor chain summed in channel order,
// plus the head terms: rc_emb_draw); the batch is the contraction, in steps of 32 windows with
// dz[b][u] = [a > 0] dL/dw_raw[b] We1[u] built while staging.  The qt == 0 workgroups also form
// dbe0 / dWe1 of their units, workgroup (ut, qt) == (0, 0) dbe1.  Adam in the epilogue: every
// parameter has exactly one owning thread; We1 is read from the forward's snapshot.
// fac: the factor chain ran in this step (dwp and, with the adjacency term, the dE records are valid).
__global__ __launch_bounds__(RC_BLOCK) void k_cemb_bwd(StepCtx c, CEmbCtx e, int nut, int nqt, int fac) {
  const RedcliffDims& d = c.d;
  const int r = rc_rep(c, blockIdx.y);
  const int p = d.p, F = d.F, K = d.K, eh = e.eh, Q = p * F, B = c.B, Ls = c.Ls, nsup = d.nsup;
  const int k = blockIdx.x / (nut * nqt), rem = blockIdx.x - k * nut * nqt, ut = rem / nqt, qt = rem - ut * nqt;
  const int u0 = ut * CE_UT, q0 = qt * CE_QC;
  float* P = c.emb + r * c.es;
  float* PM = c.embM + r * c.es;
  float* PV = c.embV + r * c.es;
  const float* ws = c.ws + r * c.wss;
  float* cw = e.ws + r * e.wss;
  const RedcliffReplicaHyper& hy = c.hyp[r];
  const int tid = threadIdx.x;
  // fetched here, not ahead of the epilogue: there the two-way fetch left the kernel a 36-byte
  // private segment (no access to it, but scratch set up per dispatch).  The scalar form: 7
  // scalars live through the kernel, 75 vector registers and 6 waves as before (vector form: 81, 5)
  const RcAdamScalars as = rc_adam_scalars<true>(c, 0, r);
  const bool gw_on = fac && (c.flags & (RC_LOSS_FORECAST | RC_LOSS_ADJ));
  const bool adj = fac && (c.flags & RC_LOSS_ADJ);
  __shared__ float dyv[512];  // dL/dw_raw[b][k], zero past B
  __shared__ float dzs[CE_BC][CE_UT + 1];
  __shared__ float has[CE_BC][CE_UT + 1];
  __shared__ float Xs[CE_BC][CE_QC + 1];
  __shared__ float dgs[CE_QC];  // dL/dg[k][c][t] of the tile's columns
  __shared__ float w1s[CE_UT];
  __shared__ float red[RC_BLOCK / 64];
  for (int b = tid; b < 512; b += RC_BLOCK) {
    float v = 0.f;
    if (b < B) {
      float gw = 0.f;
      if (gw_on)
        for (int j = 0; j < p; ++j) gw += ws[c.wo.dwp + ((int64_t)j * d.Bmax + b) * K + k];
      const float raw = ws[c.wo.w + (int64_t)b * K + k];
      const float y = ((c.flags & RC_LOSS_FACTOR) && k < nsup) ? c.lab[r * c.labr + (c.row0 + b) * K + k] : 0.f;
      v = rc_emb_draw(c, r, k, raw, gw, y);
      if (ut == 0 && qt == 0) cw[e.wo.draw + (int64_t)b * K + k] = v;
    }
    dyv[b] = v;
  }
  if (tid < CE_UT) w1s[tid] = (u0 + tid < eh) ? cw[e.wo.w1 + (int64_t)k * eh + u0 + tid] : 0.f;
  if (tid < CE_QC) {
    const int q = q0 + tid, ch = q / F, t = q - ch * F, tt = t - (F - Ls);
    float s = 0.f;
    if (adj && q < Q && tt >= 0) {
      // dE = sum over the factors' records; dg[k][ch][t] = sum_j (dE[ch][j][t] + dE[j][ch][t]) g[k][j][t]
      const float* dE = cw + e.wo.dE;
      const int64_t ks = (int64_t)p * p * Ls;
      for (int j = 0; j < p; ++j) {
        float de = 0.f;
        for (int kk = 0; kk < K; ++kk)
          de += dE[kk * ks + ((int64_t)ch * p + j) * Ls + tt] + dE[kk * ks + ((int64_t)j * p + ch) * Ls + tt];
        s = __builtin_fmaf(de, cw[e.wo.g + ((int64_t)k * p + j) * F + t], s);
      }
    }
    dgs[tid] = s;
  }
  const int uu = tid >> 4, q4 = tid & 15;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float gb0 = 0.f, gw1 = 0.f;
  for (int bb0 = 0; bb0 < B; bb0 += CE_BC) {
    __syncthreads();
    for (int i = tid; i < CE_BC * CE_UT; i += RC_BLOCK) {
      const int bb = i >> 4, ux = i & 15, b = bb0 + bb, u = u0 + ux;
      const float a = (b < B && u < eh) ? cw[e.wo.ha + ((int64_t)k * d.Bmax + b) * eh + u] : 0.f;
      has[bb][ux] = a;
      dzs[bb][ux] = a > 0.f ? dyv[b] * w1s[ux] : 0.f;
    }
    ce_stage_x(c, r, bb0, q0, Xs);
    __syncthreads();
#pragma unroll 8
    for (int bb = 0; bb < CE_BC; ++bb) {
      const float dz = dzs[bb][uu];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(dz, Xs[bb][q4 + 16 * i], acc[i]);
    }
    if (qt == 0 && q4 == 0) {
      for (int bb = 0; bb < CE_BC; ++bb) {
        gb0 += dzs[bb][uu];
        gw1 = __builtin_fmaf(dyv[bb0 + bb], has[bb][uu], gw1);
      }
    }
  }
  float gb1 = 0.f;
  if (ut == 0 && qt == 0) {  // (block-uniform)
    float t = 0.f;
    for (int b = tid; b < B; b += RC_BLOCK) t += dyv[b];
    gb1 = rc_block_sum(t, red);
  }
  // ---- epilogue: + the adjacency-L1 term through E and the group norms, then Adam
  const int u = u0 + uu;
  if (u < eh) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ql = q4 + 16 * i, q = q0 + ql;
      if (q >= Q) continue;
      const int64_t idx = e.po.We0 + ((int64_t)k * eh + u) * Q + q;
      float g = acc[i];
      if (adj) {
        const int ch = q / F, t = q - ch * F;
        if (t >= F - Ls) {
          const float gn = cw[e.wo.g + ((int64_t)k * p + ch) * F + t];
          if (gn > 0.f) g += dgs[ql] * (P[idx] / gn);
        }
      }
      rc_update(c, P, PM, PV, nullptr, idx, g, as);
    }
    if (qt == 0 && q4 == 0) {
      rc_update(c, P, PM, PV, nullptr, e.po.be0 + (int64_t)k * eh + u, gb0, as);
      rc_update(c, P, PM, PV, nullptr, e.po.We1 + (int64_t)k * eh + u, gw1, as);
    }
  }
  if (ut == 0 && qt == 0 && tid == 0) rc_update(c, P, PM, PV, nullptr, e.po.be1 + k, gb1, as);
}

}  // namespace

int rc_launch_cemb_fwd(const StepCtx& c, const CEmbCtx& e, hipStream_t s) {
  const int nbt = (c.B + CE_BT - 1) / CE_BT;
  hipLaunchKernelGGL(k_cemb_fwd, dim3(c.d.K * nbt + c.d.K * c.d.p, c.nrep), dim3(RC_BLOCK), 0, s, c, e, nbt);
  return rc_check(hipGetLastError(), "k_cemb_fwd");
}

int rc_launch_cemb_tables(const StepCtx& c, const CEmbCtx& e, hipStream_t s) {
  hipLaunchKernelGGL(k_cemb_tables, dim3(c.d.p, c.nrep), dim3(RC_BLOCK), 0, s, c, e);
  return rc_check(hipGetLastError(), "k_cemb_tables");
}

int rc_launch_cemb_bwd(const StepCtx& c, const CEmbCtx& e, bool fac, hipStream_t s) {
  const int nut = (e.eh + CE_UT - 1) / CE_UT, nqt = (c.d.p * c.d.F + CE_QC - 1) / CE_QC;
  hipLaunchKernelGGL(k_cemb_bwd, dim3(c.d.K * nut * nqt, c.nrep), dim3(RC_BLOCK), 0, s, c, e, nut, nqt, (int)fac);
  return rc_check(hipGetLastError(), "k_cemb_bwd");
}
