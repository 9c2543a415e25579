// rc_fm.hip -- whole epochs of the cMLP forecasting baseline cMLP_FM (models/cmlp_fm.py:96-201,
// 419-475) in one launch: one cMLP (models/cmlp.py:12-35 networks Conv1d(p, h, L) -> ReLU ->
// Conv1d(h, 1, 1)), no embedder, loss FORECAST_COEFF * sum_i MSE(pred_i, target_i) +
// ADJ_L1_REG_COEFF * sum ||GC(ignore_lag=True)||_1, one Adam.
//
// The loss separates over the p channel networks: network j alone forms channel j of the forecast,
// its penalty touches only its own W0[j], Adam is element-wise.  So workgroup (j, replica) holds
// network j's h*p*L + 2h + 1 weights, both Adam moments and the dW0 accumulators in LDS and runs
// every batch of the epoch on them, with no other workgroup, grid barrier or host round trip; the
// weights go back to global memory once at the end.
//
// Per batch, in passes of FM_BC = 64 windows (q = c*L + t, the Conv1d weight order):
//   stage    Xs[b][q] = X[row + b][t][c], tg[b] = X[row + b][L][j]
//   forward  thread (u, 8 windows): z = sum_q W0[u][q] x[b][q] (q ascending) + b0[u], a = relu(z)
//   output   wave 0, lane b: y = sum_u W1[u] a[b][u] (u ascending) + b1, res, dy; the pass's
//            sum res^2 and sum dy by the wave butterfly, passes added in ascending order
//   dz       thread u: dW1[u], db0[u] over b ascending, dz[b][u] in place of a[b][u]
//   dW0      thread (u, 4 columns): accumulators continue over b ascending across the passes
// then the penalty gradient c_adj * W0 / G0[c] (0 where G0[c] == 0) and rc_adam on the owner thread.
// The loops over q, u and b are unrolled so that several LDS reads are in flight (one wave per SIMD
// has nothing else to hide their latency with); the fmaf chains keep their order.
// Every sum's order depends on (p, L, h) and the batch size only; no atomics, no scratch.
#include "rc_fm.h"

namespace {

// G[q] = ||W0[:, q]||_2, G0[c] = ||W0[:, c, :]||_F of the weights in LDS (sums as k_gc_norms: u
// ascending, for G0 then t ascending).  G[q] on thread q (+ 256 i), G0[c] on thread 128 + c: other
// waves than the first G columns, so the two chains run side by side.
__device__ inline void fm_norms(const float* W, int h, int Q, int Qp, int L, int p, float* gn) {
  for (int q = threadIdx.x; q < Q; q += RC_BLOCK) {
    float a = 0.f;
#pragma unroll 8
    for (int u = 0; u < h; ++u) {
      const float x = W[u * Qp + q];
      a = __builtin_fmaf(x, x, a);
    }
    gn[q] = sqrtf(a);
  }
  for (int c = (int)threadIdx.x ^ 128; c < p; c += RC_BLOCK) {
    const float* wr = W + c * L;
    float a = 0.f;
#pragma unroll 4
    for (int u = 0; u < h; ++u)
      for (int t = 0; t < L; ++t) {
        const float x = wr[u * Qp + t];
        a = __builtin_fmaf(x, x, a);
      }
    gn[Q + c] = sqrtf(a);
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_fm_epoch(FmCtx c) {
  extern __shared__ float lds[];
  const int j = blockIdx.x, ri = blockIdx.y;
  const int r = c.rident ? ri : (int)c.rmap[ri];
  const int p = c.p, L = c.L, h = c.h, T = c.T, Q = p * L, Qp = Q | 1, hp = h | 1, tid = threadIdx.x;
  const int NP = h * Qp + 2 * h + 1;
  const bool step = (c.flags & RC_STEP_B) != 0, values = (c.flags & RC_VALUES) != 0;
  const bool fc_on = (c.flags & RC_LOSS_FORECAST) != 0, adj_on = (c.flags & RC_LOSS_ADJ) != 0;
  float* W = lds;              // [h][Qp]
  float* sb0 = W + h * Qp;     // [h]
  float* sW1 = sb0 + h;        // [h]
  float* sb1 = sW1 + h;        // [1]
  float* Mo = lds + NP;        // exp_avg, at the parameters' offsets
  float* Vo = Mo + NP;         // exp_avg_sq
  float* Gr = Vo + NP;         // [h][Qp] dW0 accumulators
  float* Xs = Gr + h * Qp;     // [FM_BC][Qp]
  float* As = Xs + FM_BC * Qp; // [FM_BC][hp] a, then dz
  float* tg = As + FM_BC * hp; // [FM_BC]
  float* dys = tg + FM_BC;     // [FM_BC]
  float* gn = dys + FM_BC;     // [Q] G | [p] G0
  RcAdamScalars& as_s = *reinterpret_cast<RcAdamScalars*>(gn + Q + p);  // this step's Adam scalars
  const RedcliffReplicaHyper& hy = c.hyp[r];
  float* Pg = c.fac + (int64_t)r * c.fs;
  float* Mg = c.facM + (int64_t)r * c.fs;
  float* Vg = c.facV + (int64_t)r * c.fs;
  const int64_t oW = c.fo.W0 + (int64_t)j * h * Q, ob0 = c.fo.b0 + (int64_t)j * h, oW1 = c.fo.W1 + (int64_t)j * h,
                ob1 = c.fo.b1 + j;
  for (int e = tid; e < h * Q; e += RC_BLOCK) {
    const int u = e / Q, q = e - u * Q, l = u * Qp + q;
    W[l] = Pg[oW + e];
    if (step) { Mo[l] = Mg[oW + e]; Vo[l] = Vg[oW + e]; }
  }
  for (int u = tid; u < h; u += RC_BLOCK) {
    sb0[u] = Pg[ob0 + u];
    sW1[u] = Pg[oW1 + u];
    if (step) {
      Mo[h * Qp + u] = Mg[ob0 + u]; Vo[h * Qp + u] = Vg[ob0 + u];
      Mo[h * Qp + h + u] = Mg[oW1 + u]; Vo[h * Qp + h + u] = Vg[oW1 + u];
    }
  }
  if (tid == 0) {
    sb1[0] = Pg[ob1];
    if (step) { Mo[NP - 1] = Mg[ob1]; Vo[NP - 1] = Vg[ob1]; }
  }
  const float* Xr = c.X + (int64_t)r * c.xps;
  const int nqg = (Q + 3) >> 2;
  for (int i = 0; i < c.nsteps; ++i) {
    const int64_t rb = c.row0 + (int64_t)i * c.B;
    const int64_t left = c.N - (int64_t)i * c.B;
    const int Bi = left < (int64_t)c.B ? (int)left : c.B;
    __syncthreads();  // the weights of this step are in place
    if (adj_on || values) fm_norms(W, h, Q, Qp, L, p, gn);
    if (step) {
      if (tid == RC_BLOCK - 1) as_s = rc_adam_scalars(hy.B, c.tB + i);
      for (int e = tid; e < h * Qp; e += RC_BLOCK) Gr[e] = 0.f;
    }
    float gb0 = 0.f, gW1 = 0.f, gb1 = 0.f, sse = 0.f;
    const float dscale = hy.c_forecast * (2.f / (float)Bi);
    for (int b0 = 0; b0 < Bi; b0 += FM_BC) {
      const int nbc = Bi - b0 < FM_BC ? Bi - b0 : FM_BC;
      __syncthreads();
      for (int e = tid; e < FM_BC * Q; e += RC_BLOCK) {
        const int bb = e / Q, x = e - bb * Q, t = x / p, ch = x - t * p;
        Xs[bb * Qp + ch * L + t] = bb < nbc ? Xr[(rb + b0 + bb) * T * p + x] : 0.f;
      }
      if (tid < FM_BC) tg[tid] = tid < nbc ? Xr[((rb + b0 + tid) * T + L) * p + j] : 0.f;
      __syncthreads();
      const int nbg = (nbc + 7) >> 3;
      for (int t = tid; t < h * nbg; t += RC_BLOCK) {
        const int bg = t / h, u = t - bg * h;
        const float* w = W + u * Qp;
        const float* x = Xs + bg * 8 * Qp;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int q = 0; q < Q; ++q) {
          const float wv = w[q];
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[k] = __builtin_fmaf(wv, x[k * Qp + q], acc[k]);
        }
        const float bu = sb0[u];
#pragma unroll
        for (int k = 0; k < 8; ++k) As[(bg * 8 + k) * hp + u] = fmaxf(acc[k] + bu, 0.f);
      }
      __syncthreads();
      if (tid < FM_BC) {  // wave 0
        float res = 0.f;
        if (tid < nbc) {
          float y = 0.f;
#pragma unroll 8
          for (int u = 0; u < h; ++u) y = __builtin_fmaf(sW1[u], As[tid * hp + u], y);
          res = (y + sb1[0]) - tg[tid];
        }
        const float dyv = fc_on ? dscale * res : 0.f;
        dys[tid] = dyv;
        sse += rc_wave_sum(res * res);
        gb1 += rc_wave_sum(dyv);
      }
      if (!step) continue;
      __syncthreads();
      if (tid < h) {
        const float w1 = sW1[tid];
#pragma unroll 8
        for (int bb = 0; bb < nbc; ++bb) {
          const float a = As[bb * hp + tid], dyv = dys[bb];
          gW1 = __builtin_fmaf(dyv, a, gW1);
          const float dz = a > 0.f ? dyv * w1 : 0.f;
          gb0 += dz;
          As[bb * hp + tid] = dz;
        }
      }
      __syncthreads();
      for (int t = tid; t < h * nqg; t += RC_BLOCK) {
        const int qg = t / h, u = t - qg * h, q0 = qg * 4;
        int qi[4];
        float acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          qi[k] = q0 + k < Q ? q0 + k : Q - 1;
          acc[k] = Gr[u * Qp + qi[k]];
        }
#pragma unroll 8
        for (int bb = 0; bb < nbc; ++bb) {
          const float dz = As[bb * hp + u];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(dz, Xs[bb * Qp + qi[k]], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (q0 + k < Q) Gr[u * Qp + q0 + k] = acc[k];
      }
    }
    if (tid == 0) {
      const int64_t o = ((int64_t)ri * c.nsteps + i) * p + j;
      c.sse[o] = sse;
      if (values) {
        float s = 0.f;
        for (int ch = 0; ch < p; ++ch) s += gn[Q + ch];
        c.pen[o] = s;
      }
    }
    if (!step) continue;
    // the update: every parameter on the thread that accumulated its gradient
    const RcAdamScalars as = as_s;
    for (int t = tid; t < h * nqg; t += RC_BLOCK) {
      const int qg = t / h, u = t - qg * h, q0 = qg * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = q0 + k;
        if (q >= Q) continue;
        const int l = u * Qp + q;
        float g = Gr[l], pp = W[l], mm = Mo[l], vv = Vo[l];
        if (adj_on) {
          const float g0 = gn[Q + q / L];
          if (g0 > 0.f) g = __builtin_fmaf(hy.c_adj, pp / g0, g);
        }
        rc_adam(pp, mm, vv, g, as);
        W[l] = pp; Mo[l] = mm; Vo[l] = vv;
      }
    }
    if (tid < h) {
      int l = h * Qp + tid;
      float pp = W[l], mm = Mo[l], vv = Vo[l];
      rc_adam(pp, mm, vv, gb0, as);
      W[l] = pp; Mo[l] = mm; Vo[l] = vv;
      l += h;
      pp = W[l]; mm = Mo[l]; vv = Vo[l];
      rc_adam(pp, mm, vv, gW1, as);
      W[l] = pp; Mo[l] = mm; Vo[l] = vv;
    }
    if (tid == 0) {
      const int l = NP - 1;
      float pp = W[l], mm = Mo[l], vv = Vo[l];
      rc_adam(pp, mm, vv, gb1, as);
      W[l] = pp; Mo[l] = mm; Vo[l] = vv;
    }
  }
  __syncthreads();
  if (step) {
    for (int e = tid; e < h * Q; e += RC_BLOCK) {
      const int u = e / Q, q = e - u * Q, l = u * Qp + q;
      Pg[oW + e] = W[l]; Mg[oW + e] = Mo[l]; Vg[oW + e] = Vo[l];
    }
    for (int u = tid; u < h; u += RC_BLOCK) {
      Pg[ob0 + u] = sb0[u]; Mg[ob0 + u] = Mo[h * Qp + u]; Vg[ob0 + u] = Vo[h * Qp + u];
      Pg[oW1 + u] = sW1[u]; Mg[oW1 + u] = Mo[h * Qp + h + u]; Vg[oW1 + u] = Vo[h * Qp + h + u];
    }
    if (tid == 0) { Pg[ob1] = sb1[0]; Mg[ob1] = Mo[NP - 1]; Vg[ob1] = Vo[NP - 1]; }
  }
  if (c.G || c.G0) {  // group norms of the final weights, in redcliff_gc_norms' layout
    fm_norms(W, h, Q, Qp, L, p, gn);
    __syncthreads();
    const int64_t rj = (int64_t)r * p + j;
    if (c.G)
      for (int q = tid; q < Q; q += RC_BLOCK) c.G[rj * Q + q] = gn[q];
    if (c.G0)
      for (int ch = tid; ch < p; ch += RC_BLOCK) c.G0[rj * p + ch] = gn[Q + ch];
  }
}

}  // namespace

int rc_launch_fm(const FmCtx& c, hipStream_t s) {
  const size_t bytes = sizeof(float) * (size_t)rc_fm_lds_floats(c.p, c.L, c.h);
  int e = rc_lds_optin(k_fm_epoch, bytes, "k_fm_epoch LDS opt-in");
  if (e) return e;
  hipLaunchKernelGGL(k_fm_epoch, dim3(c.p, c.nrep), dim3(RC_BLOCK), bytes, s, c);
  return rc_check(hipGetLastError(), "k_fm_epoch");
}
