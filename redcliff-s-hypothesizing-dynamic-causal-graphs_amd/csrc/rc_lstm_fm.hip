// rc_lstm_fm.hip -- whole epochs of the cLSTM forecasting baseline cLSTM_FM (models/clstm_fm.py:56-177,
// 341-393) in one launch: one cLSTM (models/clstm.py:12-44 networks nn.LSTM(p, h) -> Conv1d(h, 1, 1)),
// no embedder, loss FORECAST_COEFF * sum_i MSE(pred_i, target_i) + ADJ_L1_REG_COEFF * sum ||GC||_1 with
// GC[j][c] = ||weight_ih_j[:, c]||_2, one Adam.
//
// The loss separates over the p channel networks exactly as cMLP_FM's does (rc_fm.hip): workgroup
// (j, replica) holds network j's 4h(p + h + 2) + h + 1 weights, both Adam moments and the gradient
// accumulators in LDS and runs every batch of the epoch on them, with no other workgroup, grid
// barrier or host round trip; the weights go back to global memory once at the end.
//
// A batch of B_i recordings is Bq = B_i * S sequences (S = tmax - C); sequence q = n*S + s reads rows
// s .. s+C of recording n in place.  Per batch, in passes of LF_BC = 32 sequences:
//   stage    zs[b][t] = [x[n][s+t] | h_{t-1}] (h_{-1} = 0), tg[b][t] = x[n][s+t+1][j]
//   forward  t = 0..C-1: thread (gate rows g and g + 2h, 8 sequences): a = sum_q [Wih|Whh][g][q] zs[b][t][q]
//            (q ascending: inputs, then hidden units) + (bih[g] + bhh[g]), sigmoid / tanh -> gs[b][t][g]
//            (rows h apart in units of 2h keep the weight reads at an odd stride across lanes);
//            thread (b, k): c_t = f c_{t-1} + i g, h_t = o tanh(c_t) -> cs[b][t][k], zs[b][t+1][p+k]
//   output   thread (b, t): y = sum_k Wl[k] h_t[k] (k ascending) + bl, res, dy; res^2 summed per thread
//            over the passes, then by the wave butterfly and over the four waves in order
//   backward t = C-1..0: thread (b, k): dh = dy Wl[k] + dh', dc = dh o (1 - tanh^2 c_t) + dc', the four
//            pre-activation gradients in place of the gates, dc' = dc f; then (t > 0)
//            thread (k, 4 sequences): dh'[b][k] = sum_g Whh[g][k] da[b][t][g] (g ascending)
//   weights  thread (gate rows g and g + 2h, 4 columns of [x | h]): accumulators continue over t ascending,
//            b ascending across the passes; db[g], dWl[k] and dbl alike on threads of their own
// then the penalty gradient c_adj * Wih / G[c] (0 where G[c] == 0) and rc_adam on every element
// (bih and bhh both with db).  sigmoid is 1 / (1 + expf(-x)) (rc_sigmoid), tanh is tanhf; tanh(c_t) is
// recomputed in the backward instead of stored.  Every sum's order depends on (p, h, C, tmax) and the
// batch size only; no atomics, no scratch.
#include <cstring>

#include "rc_lstm_fm.h"

namespace {

struct LfOff {  // offsets (floats) of network j's tensors inside a replica's packed block
  int64_t Wih, Whh, bih, bhh, Wl, bl;
};
__device__ inline LfOff lf_off(int p, int h, int j) {
  const int64_t G4 = 4 * (int64_t)h;
  LfOff o;
  o.Wih = (int64_t)j * G4 * p;
  o.Whh = (int64_t)p * G4 * p + (int64_t)j * G4 * h;
  o.bih = (int64_t)p * G4 * (p + h) + (int64_t)j * G4;
  o.bhh = o.bih + (int64_t)p * G4;
  o.Wl = (int64_t)p * G4 * (p + h + 2) + (int64_t)j * h;
  o.bl = (int64_t)p * G4 * (p + h + 2) + (int64_t)p * h + j;
  return o;
}
// LDS index l of the workgroup's parameter block -> offset in the packed block, -1 for the pad column.
__device__ inline int64_t lf_goff(int l, const LfOff& o, int p, int h, int K, int Kp) {
  const int G4 = 4 * h, oB = G4 * Kp;
  if (l < oB) {
    const int g = l / Kp, col = l - g * Kp;
    if (col >= K) return -1;
    return col < p ? o.Wih + (int64_t)g * p + col : o.Whh + (int64_t)g * h + (col - p);
  }
  l -= oB;
  if (l < G4) return o.bih + l;
  l -= G4;
  if (l < G4) return o.bhh + l;
  l -= G4;
  if (l < h) return o.Wl + l;
  return o.bl;
}

// G[c] = ||Wih[:, c]||_2 of the weights in LDS (gate rows ascending), on thread c.
__device__ inline void lf_norms(const float* W, int G4, int Kp, int p, float* gn) {
  for (int ch = threadIdx.x; ch < p; ch += RC_BLOCK) {
    float a = 0.f;
#pragma unroll 8
    for (int g = 0; g < G4; ++g) {
      const float x = W[g * Kp + ch];
      a = __builtin_fmaf(x, x, a);
    }
    gn[ch] = sqrtf(a);
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_lstm_fm_epoch(LstmFmCtx c) {
  extern __shared__ float lds[];
  const int j = blockIdx.x, ri = blockIdx.y;
  const int r = c.rident ? ri : (int)c.rmap[ri];
  const int p = c.p, h = c.h, C = c.C, T = c.T, S = c.S, tid = threadIdx.x;
  const int K = p + h, Kp = K | 1, G4 = 4 * h, hp = h | 1;
  const int oB = G4 * Kp, oWl = oB + 2 * G4, NP = oWl + h + 1;
  const int ZS = ((C + 1) * K) | 1, GS = (G4 * C) | 1, CS = (h * C) | 1;
  const bool step = (c.flags & RC_STEP_B) != 0, values = (c.flags & RC_VALUES) != 0;
  const bool fc_on = (c.flags & RC_LOSS_FORECAST) != 0, adj_on = (c.flags & RC_LOSS_ADJ) != 0;
  float* W = lds;                 // [4h][Kp] [Wih | Whh], bih[4h], bhh[4h], Wl[h], bl
  float* Mo = W + NP;             // exp_avg, at the parameters' offsets
  float* Vo = Mo + NP;            // exp_avg_sq
  float* Gr = Vo + NP;            // gradient accumulators (db at bih's offset)
  float* zs = Gr + NP;            // [LF_BC][ZS]  [x_t | h_{t-1}], t = 0..C
  float* gs = zs + LF_BC * ZS;    // [LF_BC][GS]  gates i | f | g | o per t, then their pre-activation gradients
  float* cs = gs + LF_BC * GS;    // [LF_BC][CS]  c_t
  float* dhn = cs + LF_BC * CS;   // [LF_BC][hp]  dL/dh_{t-1} through the recurrence
  float* dcn = dhn + LF_BC * hp;  // [LF_BC][hp]  dL/dc_{t-1}
  float* tg = dcn + LF_BC * hp;   // [LF_BC][C]
  float* dys = tg + LF_BC * C;    // [LF_BC][C]
  float* gn = dys + LF_BC * C;    // [p]
  float* red = gn + p;            // [4]
  RcAdamScalars& as_s = *reinterpret_cast<RcAdamScalars*>(red + 4);  // this step's Adam scalars
  const RedcliffReplicaHyper& hy = c.hyp[r];
  float* Pg = c.fac + (int64_t)r * c.fs;
  float* Mg = step ? c.facM + (int64_t)r * c.fs : nullptr;
  float* Vg = step ? c.facV + (int64_t)r * c.fs : nullptr;
  const LfOff fo = lf_off(p, h, j);
  for (int l = tid; l < NP; l += RC_BLOCK) {
    const int64_t o = lf_goff(l, fo, p, h, K, Kp);
    W[l] = o >= 0 ? Pg[o] : 0.f;
    if (step) {
      Mo[l] = o >= 0 ? Mg[o] : 0.f;
      Vo[l] = o >= 0 ? Vg[o] : 0.f;
    }
  }
  const float* Xr = c.X + (int64_t)r * c.xps;
  const int ncg = (K + 3) >> 2, nW = 2 * h * ncg, nItems = nW + G4 + h + 1;
  for (int i = 0; i < c.nsteps; ++i) {
    const int64_t rb = c.row0 + (int64_t)i * c.B;
    const int64_t left = c.N - (int64_t)i * c.B;
    const int Bi = left < (int64_t)c.B ? (int)left : c.B;
    const int Bq = Bi * S;
    __syncthreads();  // the weights of this step are in place
    if (adj_on || values) lf_norms(W, G4, Kp, p, gn);
    if (step) {
      if (tid == RC_BLOCK - 1) as_s = rc_adam_scalars(hy.B, c.tB + i);
      for (int e = tid; e < NP; e += RC_BLOCK) Gr[e] = 0.f;
    }
    float sse = 0.f;
    const float dscale = hy.c_forecast * (2.f / ((float)Bq * (float)C));
    for (int q0 = 0; q0 < Bq; q0 += LF_BC) {
      const int nbc = Bq - q0 < LF_BC ? Bq - q0 : LF_BC;
      const int nbg = (nbc + 7) >> 3, nb8 = nbg * 8;
      __syncthreads();
      // ---- stage: padded sequences (b >= nbc) read zeros
      for (int e = tid; e < LF_BC * C * p; e += RC_BLOCK) {
        const int b = e / (C * p), x = e - b * (C * p), t = x / p, ch = x - t * p;
        float v = 0.f;
        if (b < nbc) {
          const int q = q0 + b, n = q / S, s = q - n * S;
          v = Xr[((rb + n) * T + s + t) * p + ch];
        }
        zs[b * ZS + t * K + ch] = v;
      }
      for (int e = tid; e < LF_BC * C; e += RC_BLOCK) {
        const int b = e / C, t = e - b * C;
        float v = 0.f;
        if (b < nbc) {
          const int q = q0 + b, n = q / S, s = q - n * S;
          v = Xr[((rb + n) * T + s + t + 1) * p + j];
        }
        tg[e] = v;
      }
      for (int e = tid; e < LF_BC * h; e += RC_BLOCK) {
        const int b = e / h, k = e - b * h;
        zs[b * ZS + p + k] = 0.f;
      }
      __syncthreads();
      // ---- forward through time
      for (int t = 0; t < C; ++t) {
        for (int it = tid; it < 2 * h * nbg; it += RC_BLOCK) {
          const int bg = it / (2 * h), g = it - bg * (2 * h);  // gate rows g (i | f) and g + 2h (g | o)
          const float* w0 = W + g * Kp;
          const float* w1 = w0 + 2 * h * Kp;
          const float* z = zs + bg * 8 * ZS + t * K;
          float a0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          float a1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
          for (int q = 0; q < K; ++q) {
            const float wa = w0[q], wb = w1[q];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const float zv = z[k * ZS + q];
              a0[k] = __builtin_fmaf(wa, zv, a0[k]);
              a1[k] = __builtin_fmaf(wb, zv, a1[k]);
            }
          }
          const float b0 = W[oB + g] + W[oB + G4 + g], b1 = W[oB + 2 * h + g] + W[oB + G4 + 2 * h + g];
          const bool cell = g < h;  // row g + 2h is a cell-candidate row (tanh) for g < h, an output-gate row else
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float* out = gs + (bg * 8 + k) * GS + t * G4 + g;
            const float v1 = a1[k] + b1;
            out[0] = rc_sigmoid(a0[k] + b0);
            out[2 * h] = cell ? tanhf(v1) : rc_sigmoid(v1);
          }
        }
        __syncthreads();
        for (int e = tid; e < nb8 * h; e += RC_BLOCK) {
          const int b = e / h, k = e - b * h;
          const float* ga = gs + b * GS + t * G4 + k;
          const float cprev = t > 0 ? cs[b * CS + (t - 1) * h + k] : 0.f;
          const float cc = __builtin_fmaf(ga[h], cprev, ga[0] * ga[2 * h]);
          cs[b * CS + t * h + k] = cc;
          zs[b * ZS + (t + 1) * K + p + k] = ga[3 * h] * tanhf(cc);
        }
        __syncthreads();
      }
      // ---- output layer, residuals
      for (int e = tid; e < LF_BC * C; e += RC_BLOCK) {
        const int b = e / C, t = e - b * C;
        float res = 0.f;
        if (b < nbc) {
          const float* hv = zs + b * ZS + (t + 1) * K + p;
          float y = 0.f;
#pragma unroll 8
          for (int k = 0; k < h; ++k) y = __builtin_fmaf(W[oWl + k], hv[k], y);
          res = (y + W[NP - 1]) - tg[e];
        }
        dys[e] = fc_on ? dscale * res : 0.f;
        sse = __builtin_fmaf(res, res, sse);
      }
      if (!step) continue;
      __syncthreads();
      // ---- backward through time
      for (int t = C - 1; t >= 0; --t) {
        const bool carry = t < C - 1;
        for (int e = tid; e < nb8 * h; e += RC_BLOCK) {
          const int b = e / h, k = e - b * h;
          float* ga = gs + b * GS + t * G4 + k;
          const float gi = ga[0], gf = ga[h], gg = ga[2 * h], go = ga[3 * h];
          const float cprev = t > 0 ? cs[b * CS + (t - 1) * h + k] : 0.f;
          const float tc = tanhf(cs[b * CS + t * h + k]);
          float dh = dys[b * C + t] * W[oWl + k];
          if (carry) dh += dhn[b * hp + k];
          float dc = dh * go * (1.f - tc * tc);
          if (carry) dc += dcn[b * hp + k];
          ga[0] = dc * gg * gi * (1.f - gi);
          ga[h] = dc * cprev * gf * (1.f - gf);
          ga[2 * h] = dc * gi * (1.f - gg * gg);
          ga[3 * h] = dh * tc * go * (1.f - go);
          dcn[b * hp + k] = dc * gf;
        }
        __syncthreads();
        if (t == 0) break;
        for (int it = tid; it < h * (nb8 >> 2); it += RC_BLOCK) {
          const int bg = it / h, k = it - bg * h;
          const float* w = W + p + k;
          const float* da = gs + bg * 4 * GS + t * G4;
          float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
          for (int g = 0; g < G4; ++g) {
            const float wv = w[g * Kp];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[kk] = __builtin_fmaf(wv, da[kk * GS + g], acc[kk]);
          }
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) dhn[(bg * 4 + kk) * hp + k] = acc[kk];
        }
        __syncthreads();
      }
      // ---- weight gradients of the pass
      for (int it = tid; it < nItems; it += RC_BLOCK) {
        if (it < nW) {
          const int cg = it / (2 * h), g = it - cg * (2 * h), c0 = cg * 4;  // gate rows g and g + 2h
          int ci[4];
          float a0[4], a1[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            ci[k] = c0 + k < K ? c0 + k : K - 1;
            a0[k] = Gr[g * Kp + ci[k]];
            a1[k] = Gr[(g + 2 * h) * Kp + ci[k]];
          }
          for (int t = 0; t < C; ++t) {
            const float* da = gs + t * G4 + g;
            const float* z = zs + t * K;
#pragma unroll 4
            for (int b = 0; b < nbc; ++b) {
              const float d0 = da[b * GS], d1 = da[b * GS + 2 * h];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const float zv = z[b * ZS + ci[k]];
                a0[k] = __builtin_fmaf(d0, zv, a0[k]);
                a1[k] = __builtin_fmaf(d1, zv, a1[k]);
              }
            }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (c0 + k < K) {
              Gr[g * Kp + c0 + k] = a0[k];
              Gr[(g + 2 * h) * Kp + c0 + k] = a1[k];
            }
        } else if (it < nW + G4) {
          const int g = it - nW;
          float acc = Gr[oB + g];
          for (int t = 0; t < C; ++t)
#pragma unroll 4
            for (int b = 0; b < nbc; ++b) acc += gs[b * GS + t * G4 + g];
          Gr[oB + g] = acc;
        } else if (it < nW + G4 + h) {
          const int k = it - nW - G4;
          float acc = Gr[oWl + k];
          for (int t = 0; t < C; ++t)
#pragma unroll 4
            for (int b = 0; b < nbc; ++b) acc = __builtin_fmaf(dys[b * C + t], zs[b * ZS + (t + 1) * K + p + k], acc);
          Gr[oWl + k] = acc;
        } else {
          float acc = Gr[NP - 1];
          for (int e = 0; e < nbc * C; ++e) acc += dys[e];
          Gr[NP - 1] = acc;
        }
      }
    }
    sse = rc_block_sum(sse, red);
    if (tid == 0) {
      const int64_t o = ((int64_t)ri * c.nsteps + i) * p + j;
      c.sse[o] = sse;
      if (values) {
        float s = 0.f;
        for (int ch = 0; ch < p; ++ch) s += gn[ch];
        c.pen[o] = s;
      }
    }
    if (!step) continue;
    // ---- the update (rc_block_sum's barriers stand between the last accumulation and here)
    const RcAdamScalars as = as_s;
    for (int l = tid; l < NP; l += RC_BLOCK) {
      float g;
      if (l < oB) {
        const int row = l / Kp, col = l - row * Kp;
        if (col >= K) continue;
        g = Gr[l];
        if (adj_on && col < p) {
          const float g0 = gn[col];
          if (g0 > 0.f) g = __builtin_fmaf(hy.c_adj, W[l] / g0, g);
        }
      } else if (l >= oB + G4 && l < oWl) {
        g = Gr[l - G4];  // dbhh = dbih
      } else {
        g = Gr[l];
      }
      float pp = W[l], mm = Mo[l], vv = Vo[l];
      rc_adam(pp, mm, vv, g, as);
      W[l] = pp; Mo[l] = mm; Vo[l] = vv;
    }
  }
  __syncthreads();
  if (step) {
    for (int l = tid; l < NP; l += RC_BLOCK) {
      const int64_t o = lf_goff(l, fo, p, h, K, Kp);
      if (o < 0) continue;
      Pg[o] = W[l]; Mg[o] = Mo[l]; Vg[o] = Vo[l];
    }
  }
  if (c.G) {  // column norms of the final weights
    lf_norms(W, G4, Kp, p, gn);
    __syncthreads();
    const int64_t rj = (int64_t)r * p + j;
    for (int ch = tid; ch < p; ch += RC_BLOCK) c.G[rj * p + ch] = gn[ch];
  }
}

int lf_dims(const RedcliffDims* d, int context) {
  if (!d) { rc_set_error("null dims"); return REDCLIFF_EINVAL; }
  if (d->R < 1 || d->Bmax < 1 || d->T < 1 || d->p < 1 || d->h < 1 || context < 1) {
    rc_set_error("invalid dims (R=%d Bmax=%d T=%d p=%d h=%d context=%d)", d->R, d->Bmax, d->T, d->p, d->h, context);
    return REDCLIFF_EINVAL;
  }
  if (d->p > LF_MAX_P || d->h > LF_MAX_H || context > LF_MAX_C || d->Bmax > LF_MAX_B || d->R > RC_MAX_ACTIVE ||
      rc_lstm_fm_lds_floats(d->p, d->h, context) > RC_LDS_MAX_FLOATS) {
    rc_set_error("dims outside kernel limits (lstm_fm: p<=%d h<=%d context<=%d Bmax<=%d R<=%d, LDS 4*(4h*Kp + 9h + 1) + "
                 "%d*(((C+1)K|1) + (4hC|1) + (hC|1) + 2(h|1) + 2C) + p + 16 <= %d floats, K = p + h, Kp = K|1; p=%d h=%d "
                 "context=%d Bmax=%d R=%d)", LF_MAX_P, LF_MAX_H, LF_MAX_C, LF_MAX_B, RC_MAX_ACTIVE, LF_BC,
                 RC_LDS_MAX_FLOATS, d->p, d->h, context, d->Bmax, d->R);
    return REDCLIFF_ELIMIT;
  }
  return 0;
}

}  // namespace

int rc_launch_lstm_fm(const LstmFmCtx& c, hipStream_t s) {
  const size_t bytes = sizeof(float) * (size_t)rc_lstm_fm_lds_floats(c.p, c.h, c.C);
  int e = rc_lds_optin(k_lstm_fm_epoch, bytes, "k_lstm_fm_epoch LDS opt-in");
  if (e) return e;
  hipLaunchKernelGGL(k_lstm_fm_epoch, dim3(c.p, c.nrep), dim3(RC_BLOCK), bytes, s, c);
  return rc_check(hipGetLastError(), "k_lstm_fm_epoch");
}

extern "C" {

int redcliff_lstm_fm_supported(const RedcliffDims* d, int32_t context) {
  if (lf_dims(d, context) != 0) return 0;
  return (int)rc_lstm_fm_lds_floats(d->p, d->h, context);
}

int redcliff_lstm_fm_run(const RedcliffLstmFMArgs* a, void* stream) {
  if (!a) { rc_set_error("null lstm_fm arguments"); return REDCLIFF_EINVAL; }
  int e = lf_dims(&a->d, a->context);
  if (e) return e;
  const RedcliffDims& d = a->d;
  if (a->flags & ~(RC_LOSS_FORECAST | RC_LOSS_ADJ | RC_STEP_B | RC_VALUES)) {
    rc_set_error("lstm_fm_run: unsupported flags 0x%x", a->flags);
    return REDCLIFF_EINVAL;
  }
  if (!a->X || !a->fac || !a->hyper || !a->sse || ((a->flags & RC_VALUES) && !a->pen) ||
      ((a->flags & RC_STEP_B) && (!a->fac_m || !a->fac_v))) {
    rc_set_error("lstm_fm_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->B < 1 || a->B > d.Bmax || a->N < 0 || a->row0 < 0 || a->tB < 1 || a->tmax <= a->context || a->tmax > d.T) {
    rc_set_error("lstm_fm_run: bad arguments (B=%d (1..Bmax=%d) N=%lld row0=%lld tB=%d tmax=%d (context=%d < tmax <= T=%d))",
                 a->B, d.Bmax, (long long)a->N, (long long)a->row0, a->tB, a->tmax, a->context, d.T);
    return REDCLIFF_EINVAL;
  }
  if (a->x_pstride < 0 || a->fac_stride < 0) {
    rc_set_error("lstm_fm_run: negative replica stride (x_pstride=%lld fac_stride=%lld)", (long long)a->x_pstride,
                 (long long)a->fac_stride);
    return REDCLIFF_EINVAL;
  }
  const int64_t nsteps = (a->N + a->B - 1) / a->B;
  if (nsteps > INT32_MAX || (int64_t)a->B * (a->tmax - a->context) > INT32_MAX - LF_BC) {
    rc_set_error("lstm_fm_run: too many steps or sequences per batch");
    return REDCLIFF_ELIMIT;
  }
  LstmFmCtx c;
  memset(&c, 0, sizeof(c));
  if (a->replicas) {  // the rules of RedcliffStepArgs.replicas
    if (a->n_replicas < 0 || a->n_replicas > d.R) {
      rc_set_error("lstm_fm_run: active replica list of %d entries (at most R=%d)", a->n_replicas, d.R);
      return REDCLIFF_EINVAL;
    }
    for (int i = 0; i < a->n_replicas; ++i) {
      const int r = a->replicas[i];
      if (r < 0 || r >= d.R || (i > 0 && r <= a->replicas[i - 1])) {
        rc_set_error("lstm_fm_run: active replica list must be strictly increasing indices < R=%d (entry %d = %d)", d.R,
                     i, r);
        return REDCLIFF_EINVAL;
      }
      c.rmap[i] = (uint8_t)r;
    }
    c.nrep = a->n_replicas;
    c.rident = 0;
  } else {
    c.nrep = d.R;
    c.rident = 1;
  }
  if (a->N == 0 || c.nrep == 0) return 0;
  c.p = d.p; c.h = d.h; c.C = a->context; c.T = d.T; c.S = a->tmax - a->context; c.B = a->B; c.flags = a->flags;
  c.tB = a->tB; c.nsteps = (int)nsteps;
  c.row0 = a->row0; c.N = a->N; c.xps = a->x_pstride; c.fs = a->fac_stride;
  c.X = a->X; c.fac = a->fac; c.facM = a->fac_m; c.facV = a->fac_v; c.hyp = a->hyper;
  c.sse = a->sse; c.pen = a->pen; c.G = a->G;
  return rc_launch_lstm_fm(c, (hipStream_t)stream);
}

}  // extern "C"
