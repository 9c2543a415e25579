// rc_dcsfa.hip -- the supervised dCSFA-NMF baseline (models/dcsfa_nmf.py, DcsfaNmf.forward with the deep
// encoder, the MSE reconstruction, the "Residual" supervised reconstruction and one intercept) as a
// stand-alone fit:
//   z = X W1^T + b1, BatchNorm (batch statistics), LeakyReLU(0.01), pre = a W2^T + b2, s = softplus(pre),
//   X_rec = s softplus(W_nmf), mse;  s_h = (X - s_un W_un) W_sup^T inv(W_sup W_sup^T),
//   res = ||s_sup - s_h||_F / (1 - c exp(-||s_h||_F));  y_pred = sigmoid(s_j phi_j + beta_j),
//   bce = BCELoss(weight = pw)(y_pred * tm, y * tm);  torch.optim.AdamW.
// W1 (H x D, 512 KB at the published D = 500, H = 256) is far more than a workgroup's LDS, and BatchNorm's
// statistics are per hidden unit, so workgroup (slice, replica) owns DC_HS = 8 hidden units: their rows of
// W1, b1, the BatchNorm affine and running statistics, and their columns of W2.
//
//   k_dc_fwd  (slice, replica)  z of the slice's units for the whole batch (X staged 32 rows at a time; the
//        sums over the inputs, the hidden units and, in k_dc_bwd, the batch run in double and are rounded once),
//        batch statistics in double, the running-statistics update, a = LeakyReLU(BN(z)) and xhat kept for
//        the backward, and the slice's partial of the h -> K layer P[slice][b][k].
//   k_dc_head (replica)  sums P over the slices ascending + b2, softplus, the decoder and both
//        reconstruction losses, the K_sup x K_sup inverse and the gradient through it, the logistic heads
//        and the BCE, dL/d pre; AdamW on W_nmf, b2, phi and beta.  In PRETRAIN only the reconstruction loss
//        is differentiated and W_nmf, phi, beta and their moments are not touched.
//   k_dc_bwd  (slice, replica)  dW2 columns, da, LeakyReLU and BatchNorm backward, db1, dW1 of the slice
//        (each thread owns columns d of the slice's 8 rows and walks the batch ascending); AdamW on them.
//   EVAL: k_dc_fwd with the running statistics, then k_dc_head's eval branch: the batch's sum of squared
//        reconstruction errors and, per supervised network, the confusion counts under the 0.6 cuts.
//
// The launch boundaries on the one stream are the only cross-workgroup dependencies: no workgroup waits on
// another, no atomics, no grid barrier.  Every sum runs in an order fixed by the shape and the batch size.
#include <cmath>
#include <cstring>

#include "rc_dcsfa.h"

namespace {

__device__ inline float dc_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ inline float dc_dsoftplus(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }

// torch.optim.AdamW (_single_tensor_adamw) for one element: p *= 1 - lr wd; m.lerp_(g, 1 - b1);
// v = v b2 + (1 - b2) g g; p += -(lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).  The scalars are the host's.
__device__ inline void dc_adamw(const DcCtx& c, float* P, float* M, float* V, int64_t i, float g) {
  float p = P[i] * c.decay, m = M[i], v = V[i];
  m = __builtin_fmaf(c.omb1, g - m, m);
  v = __builtin_fmaf(c.omb2 * g, g, v * c.b2);
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  p = __builtin_fmaf(c.neg_step, m / denom, p);
  P[i] = p; M[i] = m; V[i] = v;
}

// the batch's rows of X: the epoch's drawn indices (clamped to the set) or consecutive rows (EVAL)
__device__ inline void dc_rows(const DcCtx& c, int r, int* rows) {
  for (int b = threadIdx.x; b < c.Bi; b += RC_BLOCK) {
    int64_t row;
    if (c.mode == REDCLIFF_DCSFA_EVAL) {
      row = c.row0 + b;
    } else {
      row = c.idx[(int64_t)r * c.ips + (int64_t)c.step * c.B + b];
    }
    if (row < 0) row = 0;
    if (row >= c.N) row = c.N - 1;
    rows[b] = (int)row;
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_dc_fwd(const DcCtx c) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, sl = blockIdx.x, r = blockIdx.y;
  const int D = c.D, H = c.H, K = c.K, Bi = c.Bi, Dp = D | 1;
  const int u0 = sl * DC_HS, nu = min(DC_HS, H - u0);
  const bool train = c.mode != REDCLIFF_DCSFA_EVAL;
  float* misc = lds;                       // alpha[8] beta[8] mean[8] inv[8]
  int* rows = reinterpret_cast<int*>(lds + DC_MISC);
  float* zs = lds + DC_MISC + c.B;         // [B][8]
  float* w1s = zs + c.B * DC_HS;           // [8][Dp]
  float* xs = w1s + DC_HS * Dp;            // [32][Dp]
  const float* P = c.par + (int64_t)r * c.fs;
  const float* X = c.X + (int64_t)r * c.xps;
  float* ws = c.ws + (int64_t)r * c.wss;
  const int Hp = c.nsl * DC_HS;

  dc_rows(c, r, rows);
  for (int u = 0; u < nu; ++u)
    for (int d = tid; d < D; d += RC_BLOCK) w1s[u * Dp + d] = P[c.o.W1 + (int64_t)(u0 + u) * D + d];
  for (int b0 = 0; b0 < Bi; b0 += DC_BC) {
    const int nb = min(DC_BC, Bi - b0);
    __syncthreads();
    for (int bb = 0; bb < nb; ++bb) {
      const float* xr = X + (int64_t)rows[b0 + bb] * D;
      for (int d = tid; d < D; d += RC_BLOCK) xs[bb * Dp + d] = xr[d];
    }
    __syncthreads();
    const int u = tid & (DC_HS - 1), bb = tid >> 3;
    if (u < nu && bb < nb) {
      const float* xv = xs + bb * Dp;
      const float* wv = w1s + u * Dp;
      // accumulated in double and rounded once: a sequential fp32 sum over D inputs is off by ~1e-6 of |z|, which
      // BatchNorm's 1 / std magnifies to more than the distance of some activation from LeakyReLU's kink
      double acc = 0.0;
      for (int d = 0; d < D; ++d) acc = fma((double)xv[d], (double)wv[d], acc);
      zs[(b0 + bb) * DC_HS + u] = (float)(acc + (double)P[c.o.b1 + u0 + u]);
    }
  }
  __syncthreads();
  if (tid < nu) {
    const int u = tid, uu = u0 + u;
    float mean, inv;
    if (train) {
      double sm = 0.0;
      for (int b = 0; b < Bi; ++b) sm += (double)zs[b * DC_HS + u];
      const double mu = sm / Bi;
      double sv = 0.0;
      for (int b = 0; b < Bi; ++b) {
        const double dz = (double)zs[b * DC_HS + u] - mu;
        sv += dz * dz;
      }
      const double var = sv / Bi;
      mean = (float)mu;
      inv = (float)(1.0 / sqrt(var + c.bn_eps));
      float* rm = c.rm + (int64_t)r * H;
      float* rv = c.rv + (int64_t)r * H;
      const double unb = Bi > 1 ? sv / (Bi - 1) : var;
      rm[uu] = (float)(c.bn_mom * mu + (1.0 - c.bn_mom) * (double)rm[uu]);
      rv[uu] = (float)(c.bn_mom * unb + (1.0 - c.bn_mom) * (double)rv[uu]);
    } else {
      mean = c.rm[(int64_t)r * H + uu];
      inv = 1.0f / sqrtf(c.rv[(int64_t)r * H + uu] + (float)c.bn_eps);
    }
    const float a = inv * P[c.o.bnw + uu];
    misc[u] = a;
    {
#pragma clang fp contract(off)
      const float ma = mean * a;  // rounded on its own, as the product x * alpha below
      misc[8 + u] = P[c.o.bnb + uu] - ma;
    }
    misc[16 + u] = mean;
    misc[24 + u] = inv;
    if (train) ws[c.w.inv + uu] = inv;
  }
  __syncthreads();
  for (int e = tid; e < Bi * DC_HS; e += RC_BLOCK) {
    const int b = e >> 3, u = e & (DC_HS - 1);
    if (u >= nu) { zs[e] = 0.f; continue; }
    const float z = zs[e];
    float y;
    {
#pragma clang fp contract(off)
      const float za = z * misc[u];  // torch: the product, then the sum
      y = za + misc[8 + u];
    }
    const float a = y > 0.f ? y : y * 0.01f;
    zs[e] = a;
    if (train) {
      ws[c.w.a + (int64_t)b * Hp + u0 + u] = a;
      ws[c.w.xh + (int64_t)b * Hp + u0 + u] = (z - misc[16 + u]) * misc[24 + u];
    }
  }
  __syncthreads();
  for (int e = tid; e < Bi * K; e += RC_BLOCK) {
    const int b = e / K, k = e - b * K;
    double p = 0.0;
    for (int u = 0; u < nu; ++u) p = fma((double)zs[b * DC_HS + u], (double)P[c.o.W2 + (int64_t)k * H + u0 + u], p);
    ws[c.w.P + ((int64_t)sl * c.B + b) * K + k] = (float)p;
  }
}

// LDS of the head workgroup
struct DcHead {
  float* misc; int* rows;
  float *spre, *s, *dse, *r1, *sh, *gsh, *dl;  // [B][K]
  float *Gm, *Mi, *Gi, *Gs;                    // [K][K]
  float* Wp;                                   // [K][D|1]
};
__device__ inline DcHead dc_head_lds(float* l, const DcCtx& c) {
  DcHead h;
  const int BK = c.B * c.K, KK = c.K * c.K;
  h.misc = l; l += DC_MISC;
  h.rows = reinterpret_cast<int*>(l); l += c.B;
  h.spre = l; l += BK; h.s = l; l += BK; h.dse = l; l += BK; h.r1 = l; l += BK; h.sh = l; l += BK; h.gsh = l; l += BK;
  h.dl = l; l += BK;
  h.Gm = l; l += KK; h.Mi = l; l += KK; h.Gi = l; l += KK; h.Gs = l; l += KK;
  h.Wp = l;
  return h;
}

__global__ __launch_bounds__(RC_BLOCK) void k_dc_head(const DcCtx c) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, r = blockIdx.x, lane = tid & 63, wv = tid >> 6;
  const int D = c.D, H = c.H, K = c.K, ns = c.ns, Bi = c.Bi, Dp = D | 1;
  const bool eval = c.mode == REDCLIFF_DCSFA_EVAL, pre = c.mode == REDCLIFF_DCSFA_PRETRAIN;
  const DcHead L = dc_head_lds(lds, c);
  double* red = reinterpret_cast<double*>(L.misc);  // 4 doubles; scalars from misc[16]
  float* sc = L.misc + 16;
  float* P = c.par + (int64_t)r * c.fs;
  float* Pm = c.pm + (int64_t)r * c.fs;
  float* Pv = c.pv + (int64_t)r * c.fs;
  const float* X = c.X + (int64_t)r * c.xps;
  const float* Y = c.Y + (int64_t)r * c.yps;
  const float* TM = c.TM + (int64_t)r * c.yps;
  const float* PW = c.PW + (int64_t)r * c.pps;
  float* ws = c.ws + (int64_t)r * c.wss;

  dc_rows(c, r, L.rows);
  for (int k = 0; k < K; ++k)
    for (int d = tid; d < D; d += RC_BLOCK) L.Wp[k * Dp + d] = dc_softplus(P[c.o.Wn + (int64_t)k * D + d]);
  for (int e = tid; e < Bi * K; e += RC_BLOCK) {
    const int b = e / K, k = e - b * K;
    double vd = 0.0;
    for (int sl = 0; sl < c.nsl; ++sl) vd += (double)ws[c.w.P + ((int64_t)sl * c.B + b) * K + k];
    const float v = (float)(vd + (double)P[c.o.b2 + k]);
    L.spre[e] = v;
    L.s[e] = dc_softplus(v);
  }
  __syncthreads();

  // pass A, a wave per row: E = s Wp - x, its square sum, E Wp^T and (x - s_un W_un) W_sup^T
  float sse = 0.f;
  for (int b = wv; b < Bi; b += RC_BLOCK / 64) {
    const float* xr = X + (int64_t)L.rows[b] * D;
    float sk[DC_KMAX], aE[DC_KMAX], aR[DC_KMAX];
#pragma unroll
    for (int k = 0; k < DC_KMAX; ++k) {
      sk[k] = k < K ? L.s[b * K + k] : 0.f;
      aE[k] = 0.f;
      aR[k] = 0.f;
    }
    for (int d = lane; d < D; d += 64) {
      const float x = xr[d];
      float wp[DC_KMAX], rec = 0.f, un = 0.f;
#pragma unroll
      for (int k = 0; k < DC_KMAX; ++k) {
        wp[k] = k < K ? L.Wp[k * Dp + d] : 0.f;
        rec = __builtin_fmaf(sk[k], wp[k], rec);
        if (k >= ns) un = __builtin_fmaf(sk[k], wp[k], un);
      }
      const float ee = rec - x, rs = x - un;
      sse = __builtin_fmaf(ee, ee, sse);
#pragma unroll
      for (int k = 0; k < DC_KMAX; ++k) {
        aE[k] = __builtin_fmaf(ee, wp[k], aE[k]);
        if (k < ns) aR[k] = __builtin_fmaf(rs, wp[k], aR[k]);
      }
    }
    if (!eval) {
#pragma unroll
      for (int k = 0; k < DC_KMAX; ++k) {
        if (k < K) {
          const float e1 = rc_wave_sum(aE[k]);
          const float e2 = rc_wave_sum(aR[k]);
          if (lane == 0) {
            L.dse[b * K + k] = e1;
            L.r1[b * K + k] = e2;
          }
        }
      }
    }
  }
  const double sse_d = rc_block_sum_d((double)sse, red);

  if (eval) {
    double* ev = c.ev + (int64_t)r * c.evs + (int64_t)c.step * (1 + 4 * ns);
    if (tid == 0) ev[0] = sse_d;
    if (tid < ns) {
      const int j = tid;
      const float phi = P[c.o.phi + j], beta = P[c.o.beta + j];
      int tp = 0, fp = 0, tn = 0, fn = 0;
      for (int b = 0; b < Bi; ++b) {
        const int64_t row = L.rows[b];
        if (TM[row * ns + j] != 1.f) continue;
        const float yp = rc_sigmoid(__builtin_fmaf(L.s[b * K + j], phi, beta));
        const bool lab = Y[row * ns + j] >= 0.6f, pr = yp >= 0.6f;
        if (lab) { if (pr) ++tp; else ++fn; } else { if (pr) ++fp; else ++tn; }
      }
      ev[1 + 4 * j] = tp; ev[2 + 4 * j] = fp; ev[3 + 4 * j] = tn; ev[4 + 4 * j] = fn;
    }
    return;
  }

  // Gram matrix of softplus(W_nmf), a wave per entry
  for (int e = wv; e < K * K; e += RC_BLOCK / 64) {
    const int i = e / K, j = e - i * K;
    float g = 0.f;
    for (int d = lane; d < D; d += 64) g = __builtin_fmaf(L.Wp[i * Dp + d], L.Wp[j * Dp + d], g);
    g = rc_wave_sum(g);
    if (lane == 0) L.Gm[e] = g;
  }
  __syncthreads();
  // inv(W_sup W_sup^T): Gauss-Jordan with partial pivoting, one thread (ns <= 8)
  if (tid == 0) {
    float* A = L.Gi;
    float* I = L.Mi;
    for (int i = 0; i < ns; ++i)
      for (int j = 0; j < ns; ++j) {
        A[i * K + j] = L.Gm[i * K + j];
        I[i * K + j] = i == j ? 1.f : 0.f;
      }
    for (int col = 0; col < ns; ++col) {
      int pv = col;
      float best = fabsf(A[col * K + col]);
      for (int i = col + 1; i < ns; ++i) {
        const float v = fabsf(A[i * K + col]);
        if (v > best) { best = v; pv = i; }
      }
      if (pv != col)
        for (int j = 0; j < ns; ++j) {
          float t = A[col * K + j]; A[col * K + j] = A[pv * K + j]; A[pv * K + j] = t;
          t = I[col * K + j]; I[col * K + j] = I[pv * K + j]; I[pv * K + j] = t;
        }
      const float d = 1.f / A[col * K + col];
      for (int j = 0; j < ns; ++j) { A[col * K + j] *= d; I[col * K + j] *= d; }
      for (int i = 0; i < ns; ++i) {
        if (i == col) continue;
        const float f = A[i * K + col];
        for (int j = 0; j < ns; ++j) {
          A[i * K + j] -= f * A[col * K + j];
          I[i * K + j] -= f * I[col * K + j];
        }
      }
    }
  }
  __syncthreads();
  // s_h = R1 Minv and the two Frobenius norms over the whole batch
  float q1 = 0.f, q2 = 0.f;
  for (int e = tid; e < Bi * ns; e += RC_BLOCK) {
    const int b = e / ns, j = e - b * ns;
    float v = 0.f;
    for (int i = 0; i < ns; ++i) v = __builtin_fmaf(L.r1[b * K + i], L.Mi[i * K + j], v);
    L.sh[b * K + j] = v;
    const float df = L.s[b * K + j] - v;
    q1 = __builtin_fmaf(df, df, q1);
    q2 = __builtin_fmaf(v, v, q2);
  }
  const double q1d = rc_block_sum_d((double)q1, red);
  const double q2d = rc_block_sum_d((double)q2, red);
  const float n1 = sqrtf((float)q1d), n2 = sqrtf((float)q2d);
  const float ex = c.smooth * expf(-n2), den = 1.f - ex;
  const float res = n1 / den;
  const float cA = n1 > 0.f ? c.sup_recon_w / (n1 * den) : 0.f;
  const float cB = n2 > 0.f ? c.sup_recon_w * (-n1 / (den * den)) * ex / n2 : 0.f;
  for (int e = tid; e < Bi * ns; e += RC_BLOCK) {
    const int b = e / ns, j = e - b * ns;
    const float v = L.sh[b * K + j];
    L.gsh[b * K + j] = __builtin_fmaf(cB, v, -cA * (L.s[b * K + j] - v));
  }
  __syncthreads();
  // dL/dMinv = R1^T G_sh
  if (tid < ns * ns) {
    const int i = tid / ns, j = tid - i * ns;
    float v = 0.f;
    for (int b = 0; b < Bi; ++b) v = __builtin_fmaf(L.r1[b * K + i], L.gsh[b * K + j], v);
    L.Gi[i * K + j] = v;
  }
  __syncthreads();
  // dL/dR1 = G_sh Minv^T (over R1), dL/dM = -Minv^T G Minv^T, symmetrised for M = W_sup W_sup^T
  for (int e = tid; e < Bi * ns; e += RC_BLOCK) {
    const int b = e / ns, i = e - b * ns;
    float v = 0.f;
    for (int j = 0; j < ns; ++j) v = __builtin_fmaf(L.gsh[b * K + j], L.Mi[i * K + j], v);
    L.r1[b * K + i] = v;
  }
  if (tid < ns * ns) {
    const int i = tid / ns, j = tid - i * ns;
    float gm = 0.f, gt = 0.f;
    for (int p = 0; p < ns; ++p)
      for (int q = 0; q < ns; ++q) {
        gm = __builtin_fmaf(L.Mi[p * K + i] * L.Gi[p * K + q], L.Mi[j * K + q], gm);
        gt = __builtin_fmaf(L.Mi[p * K + j] * L.Gi[p * K + q], L.Mi[i * K + q], gt);
      }
    L.Gs[i * K + j] = -(gm + gt);
  }
  __syncthreads();

  // the logistic heads, the BCE and dL/d pre
  const float gmse = c.recon_w * 2.f / ((float)Bi * (float)D);
  float bce = 0.f;
  for (int e = tid; e < Bi * K; e += RC_BLOCK) {
    const int b = e / K, k = e - b * K;
    const float sv = L.s[e];
    float ds = gmse * L.dse[e];
    float dl = 0.f;
    if (k < ns) {
      ds = __builtin_fmaf(cA, sv - L.sh[e], ds);
      const int64_t row = L.rows[b];
      const float phi = P[c.o.phi + k];
      const float yp = rc_sigmoid(__builtin_fmaf(sv, phi, P[c.o.beta + k]));
      const float tm = TM[row * ns + k], pw = PW[row];
      const float p = yp * tm, t = Y[row * ns + k] * tm;
      bce -= pw * (t * fmaxf(logf(p), -100.f) + (1.f - t) * fmaxf(logf(1.f - p), -100.f));
      if (!pre) {
        const float dp = c.sup_w * pw * (p - t) / fmaxf((1.f - p) * p, 1e-12f) / ((float)Bi * (float)ns);
        dl = dp * tm * yp * (1.f - yp);
        ds = __builtin_fmaf(dl, phi, ds);
      }
    } else {
      float g = 0.f;
      for (int j = 0; j < ns; ++j) g = __builtin_fmaf(L.r1[b * K + j], L.Gm[j * K + k], g);
      ds -= g;
    }
    L.dl[e] = dl;
    const float dpre = ds * dc_dsoftplus(L.spre[e]);
    L.dse[e] = dpre;
    ws[c.w.dpre + e] = dpre;
  }
  const double bce_d = rc_block_sum_d((double)bce, red);
  if (tid == 0) {
    float* lo = c.loss + ((int64_t)r * c.nsteps + c.step) * 2;
    const float mse = (float)(sse_d / ((double)Bi * (double)D));
    lo[0] = __builtin_fmaf(c.sup_recon_w, res, c.recon_w * mse);
    lo[1] = c.sup_w * (float)(bce_d / ((double)Bi * (double)ns));
  }
  __syncthreads();
  if (tid < K) {
    float g = 0.f;
    for (int b = 0; b < Bi; ++b) g += L.dse[b * K + tid];
    dc_adamw(c, P, Pm, Pv, c.o.b2 + tid, g);
  }
  if (pre) return;
  if (tid >= 64 && tid < 64 + ns) {
    const int j = tid - 64;
    float gp = 0.f, gb = 0.f;
    for (int b = 0; b < Bi; ++b) {
      const float dl = L.dl[b * K + j];
      gp = __builtin_fmaf(dl, L.s[b * K + j], gp);
      gb += dl;
    }
    dc_adamw(c, P, Pm, Pv, c.o.phi + j, gp);
    dc_adamw(c, P, Pm, Pv, c.o.beta + j, gb);
  }
  // pass B, a thread per column: dL/d softplus(W_nmf) over the batch ascending, AdamW on W_nmf
  for (int d = tid; d < D; d += RC_BLOCK) {
    float wp[DC_KMAX], acc[DC_KMAX];
#pragma unroll
    for (int k = 0; k < DC_KMAX; ++k) {
      wp[k] = k < K ? L.Wp[k * Dp + d] : 0.f;
      acc[k] = 0.f;
    }
    for (int b = 0; b < Bi; ++b) {
      const float x = X[(int64_t)L.rows[b] * D + d];
      float rec = 0.f, un = 0.f, gres = 0.f;
#pragma unroll
      for (int k = 0; k < DC_KMAX; ++k) {
        if (k < K) {
          const float sv = L.s[b * K + k];
          rec = __builtin_fmaf(sv, wp[k], rec);
          if (k >= ns) un = __builtin_fmaf(sv, wp[k], un);
          else gres = __builtin_fmaf(L.r1[b * K + k], wp[k], gres);
        }
      }
      const float ge = gmse * (rec - x), rs = x - un;
#pragma unroll
      for (int k = 0; k < DC_KMAX; ++k) {
        if (k < K) {
          const float sv = L.s[b * K + k];
          acc[k] = __builtin_fmaf(sv, ge, acc[k]);
          if (k < ns) acc[k] = __builtin_fmaf(L.r1[b * K + k], rs, acc[k]);
          else acc[k] = __builtin_fmaf(-sv, gres, acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < DC_KMAX; ++k) {
      if (k < K) {
        float g = acc[k];
        if (k < ns) {
#pragma unroll
          for (int i = 0; i < DC_KMAX; ++i)
            if (i < ns) g = __builtin_fmaf(L.Gs[k * K + i], wp[i], g);
        }
        const int64_t at = c.o.Wn + (int64_t)k * D + d;
        dc_adamw(c, P, Pm, Pv, at, g * dc_dsoftplus(P[at]));
      }
    }
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_dc_bwd(const DcCtx c) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, sl = blockIdx.x, r = blockIdx.y;
  const int D = c.D, H = c.H, K = c.K, Bi = c.Bi;
  const int u0 = sl * DC_HS, nu = min(DC_HS, H - u0), Hp = c.nsl * DC_HS;
  float* misc = lds;  // m1[8] m2[8] cf[8]
  int* rows = reinterpret_cast<int*>(lds + DC_MISC);
  float* dp = lds + DC_MISC + c.B;   // [B][K]
  float* as = dp + c.B * K;          // [B][8]
  float* xh = as + c.B * DC_HS;
  float* dz = xh + c.B * DC_HS;
  float* w2s = dz + c.B * DC_HS;     // [K][8]
  float* P = c.par + (int64_t)r * c.fs;
  float* Pm = c.pm + (int64_t)r * c.fs;
  float* Pv = c.pv + (int64_t)r * c.fs;
  const float* X = c.X + (int64_t)r * c.xps;
  const float* ws = c.ws + (int64_t)r * c.wss;

  dc_rows(c, r, rows);
  for (int e = tid; e < Bi * K; e += RC_BLOCK) dp[e] = ws[c.w.dpre + e];
  for (int e = tid; e < Bi * DC_HS; e += RC_BLOCK) {
    const int b = e >> 3, u = e & (DC_HS - 1);
    as[e] = u < nu ? ws[c.w.a + (int64_t)b * Hp + u0 + u] : 0.f;
    xh[e] = u < nu ? ws[c.w.xh + (int64_t)b * Hp + u0 + u] : 0.f;
  }
  if (tid < K * DC_HS) {
    const int k = tid >> 3, u = tid & (DC_HS - 1);
    w2s[tid] = u < nu ? P[c.o.W2 + (int64_t)k * H + u0 + u] : 0.f;
  }
  __syncthreads();
  if (tid < K * DC_HS) {
    const int k = tid >> 3, u = tid & (DC_HS - 1);
    if (u < nu) {
      double g = 0.0;
      for (int b = 0; b < Bi; ++b) g = fma((double)dp[b * K + k], (double)as[b * DC_HS + u], g);
      dc_adamw(c, P, Pm, Pv, c.o.W2 + (int64_t)k * H + u0 + u, (float)g);
    }
  }
  for (int e = tid; e < Bi * DC_HS; e += RC_BLOCK) {
    const int b = e >> 3, u = e & (DC_HS - 1);
    float da = 0.f;
    for (int k = 0; k < K; ++k) da = __builtin_fmaf(dp[b * K + k], w2s[k * DC_HS + u], da);
    dz[e] = as[e] > 0.f ? da : da * 0.01f;
  }
  __syncthreads();
  if (tid < nu) {
    const int u = tid, uu = u0 + u;
    double sdyd = 0.0, sdxd = 0.0;
    for (int b = 0; b < Bi; ++b) {
      const double dy = (double)dz[b * DC_HS + u];
      sdyd += dy;
      sdxd = fma(dy, (double)xh[b * DC_HS + u], sdxd);
    }
    const float sdy = (float)sdyd, sdx = (float)sdxd;
    misc[u] = (float)(sdyd / Bi);
    misc[8 + u] = (float)(sdxd / Bi);
    misc[16 + u] = P[c.o.bnw + uu] * ws[c.w.inv + uu];
    dc_adamw(c, P, Pm, Pv, c.o.bnw + uu, sdx);
    dc_adamw(c, P, Pm, Pv, c.o.bnb + uu, sdy);
  }
  __syncthreads();
  for (int e = tid; e < Bi * DC_HS; e += RC_BLOCK) {
    const int u = e & (DC_HS - 1);
    if (u < nu) dz[e] = (dz[e] - misc[u] - xh[e] * misc[8 + u]) * misc[16 + u];
  }
  __syncthreads();
  if (tid < nu) {
    double g = 0.0;
    for (int b = 0; b < Bi; ++b) g += (double)dz[b * DC_HS + tid];
    dc_adamw(c, P, Pm, Pv, c.o.b1 + u0 + tid, (float)g);
  }
  for (int d = tid; d < D; d += RC_BLOCK) {
    double acc[DC_HS];
#pragma unroll
    for (int u = 0; u < DC_HS; ++u) acc[u] = 0.0;
    for (int b = 0; b < Bi; ++b) {
      const double x = (double)X[(int64_t)rows[b] * D + d];
#pragma unroll
      for (int u = 0; u < DC_HS; ++u) acc[u] = fma((double)dz[b * DC_HS + u], x, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < DC_HS; ++u)
      if (u < nu) dc_adamw(c, P, Pm, Pv, c.o.W1 + (int64_t)(u0 + u) * D + d, (float)acc[u]);
  }
}

template <class Kern>
int dc_launch(Kern k, const char* what, dim3 grid, size_t bytes, const DcCtx& c, hipStream_t s) {
  static size_t opted[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
  if (dev < 0 || bytes > opted[dev]) {
    const int e = rc_lds_optin(k, bytes, what);
    if (e) return e;
    if (dev >= 0) opted[dev] = bytes;
  }
  hipLaunchKernelGGL(k, grid, dim3(RC_BLOCK), bytes, s, c);
  return rc_check(hipGetLastError(), what);
}

size_t dc_lds_bytes(const DcCtx& c) {
  return sizeof(float) * (size_t)rc_dcsfa_lds_floats(c.D, c.H, c.K, c.ns, c.B, 1);
}

}  // namespace

int rc_launch_dcsfa_step(const DcCtx& c, hipStream_t s) {
  const size_t bytes = dc_lds_bytes(c);
  const dim3 grid(c.nsl, c.nrep);
  int e = dc_launch(k_dc_fwd, "k_dc_fwd", grid, bytes, c, s);
  if (e) return e;
  if ((e = dc_launch(k_dc_head, "k_dc_head", dim3(c.nrep), bytes, c, s))) return e;
  return dc_launch(k_dc_bwd, "k_dc_bwd", grid, bytes, c, s);
}

int rc_launch_dcsfa_eval(const DcCtx& c, hipStream_t s) {
  const size_t bytes = dc_lds_bytes(c);
  const int e = dc_launch(k_dc_fwd, "k_dc_fwd", dim3(c.nsl, c.nrep), bytes, c, s);
  if (e) return e;
  return dc_launch(k_dc_head, "k_dc_head", dim3(c.nrep), bytes, c, s);
}

extern "C" {

static int dcsfa_dims(const RedcliffDcsfaArgs* a) {
  if (a->D < 1 || a->H < 1 || a->K < 1 || a->ns < 1 || a->R < 1 || a->Bmax < 1) {
    rc_set_error("invalid dims (D=%d H=%d K=%d ns=%d R=%d Bmax=%d)", a->D, a->H, a->K, a->ns, a->R, a->Bmax);
    return REDCLIFF_EINVAL;
  }
  if (rc_dcsfa_lds_floats(a->D, a->H, a->K, a->ns, a->Bmax, a->R) == 0) {
    rc_set_error("dims outside kernel limits (dcsfa: K<=%d ns<=K Bmax<=%d R<=%d D,H<=4096, LDS max(128 + 9*Bmax + 40*(D|1), "
                 "128 + Bmax + 7*Bmax*K + 4*K*K + K*(D|1)) <= %d floats; D=%d H=%d K=%d ns=%d Bmax=%d R=%d)", DC_KMAX,
                 DC_BMAX, RC_MAX_ACTIVE, RC_LDS_MAX_FLOATS, a->D, a->H, a->K, a->ns, a->Bmax, a->R);
    return REDCLIFF_ELIMIT;
  }
  return 0;
}

int redcliff_dcsfa_supported(int32_t D, int32_t H, int32_t K, int32_t ns, int32_t Bmax, int32_t R) {
  RedcliffDcsfaArgs a;
  memset(&a, 0, sizeof(a));
  a.D = D; a.H = H; a.K = K; a.ns = ns; a.Bmax = Bmax; a.R = R;
  if (dcsfa_dims(&a) != 0) return 0;
  return (int)rc_dcsfa_lds_floats(D, H, K, ns, Bmax, R);
}

int64_t redcliff_dcsfa_ws_floats(int32_t H, int32_t K, int32_t B) {
  if (H < 1 || K < 1 || B < 1) return 0;
  return rc_dcsfa_ws(H, K, B).total;
}

int redcliff_dcsfa_run(const RedcliffDcsfaArgs* a, void* stream) {
  if (!a) { rc_set_error("null dcsfa arguments"); return REDCLIFF_EINVAL; }
  int e = dcsfa_dims(a);
  if (e) return e;
  const bool eval = a->mode == REDCLIFF_DCSFA_EVAL;
  if (!eval && a->mode != REDCLIFF_DCSFA_TRAIN && a->mode != REDCLIFF_DCSFA_PRETRAIN) {
    rc_set_error("dcsfa_run: bad mode %d", a->mode);
    return REDCLIFF_EINVAL;
  }
  if (!a->X || !a->Y || !a->TM || !a->PW || !a->par || !a->ws || !a->bn_rm || !a->bn_rv ||
      (eval ? !a->ev : (!a->idx || !a->par_m || !a->par_v || !a->loss))) {
    rc_set_error("dcsfa_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->B < 1 || a->B > a->Bmax || a->N < 1 || a->N > INT32_MAX || a->n < 0 || a->row0 < 0 ||
      (eval && a->row0 + a->n > a->N) || (!eval && (a->tB < 1 || a->row0 != 0))) {
    rc_set_error("dcsfa_run: bad arguments (B=%d (1..Bmax=%d) N=%lld n=%lld row0=%lld tB=%d)", a->B, a->Bmax,
                 (long long)a->N, (long long)a->n, (long long)a->row0, a->tB);
    return REDCLIFF_EINVAL;
  }
  if (a->x_pstride < 0 || a->y_pstride < 0 || a->pw_pstride < 0 || a->idx_pstride < 0 || a->par_stride < 0) {
    rc_set_error("dcsfa_run: negative replica stride");
    return REDCLIFF_EINVAL;
  }
  if (!eval && a->idx_pstride != 0 && a->idx_pstride < a->n) {
    rc_set_error("dcsfa_run: index stride %lld shorter than the %lld drawn rows", (long long)a->idx_pstride, (long long)a->n);
    return REDCLIFF_EINVAL;
  }
  const int64_t nsteps = (a->n + a->B - 1) / a->B;
  if (nsteps > 65535) { rc_set_error("dcsfa_run: %lld steps in one call (at most 65535)", (long long)nsteps); return REDCLIFF_ELIMIT; }
  if (!eval && a->n - (nsteps - 1) * a->B == 1) {
    rc_set_error("dcsfa_run: a last batch of one row has no batch statistics");
    return REDCLIFF_EINVAL;
  }
  if ((reinterpret_cast<uintptr_t>(a->ws) & 7) != 0) { rc_set_error("dcsfa_run: workspace not 8-byte aligned"); return REDCLIFF_EINVAL; }
  DcCtx c;
  memset(&c, 0, sizeof(c));
  c.D = a->D; c.H = a->H; c.K = a->K; c.ns = a->ns; c.B = a->B; c.mode = a->mode; c.nrep = a->R;
  c.nsl = rc_dcsfa_slices(c.H);
  c.o = rc_dcsfa_off(c.D, c.H, c.K, c.ns);
  c.w = rc_dcsfa_ws(c.H, c.K, c.B);
  c.wss = c.w.total;
  if (a->par_stride < c.o.total && a->R > 1) { rc_set_error("dcsfa_run: parameter stride shorter than a block"); return REDCLIFF_EINVAL; }
  if (a->ws_bytes < sizeof(float) * (size_t)c.wss * (size_t)c.nrep) {
    rc_set_error("dcsfa_run: workspace of %zu bytes, %zu needed", a->ws_bytes, sizeof(float) * (size_t)c.wss * (size_t)c.nrep);
    return REDCLIFF_EWORKSPACE;
  }
  if (a->n == 0) return 0;
  c.N = a->N; c.xps = a->x_pstride; c.yps = a->y_pstride; c.pps = a->pw_pstride; c.ips = a->idx_pstride; c.fs = a->par_stride;
  c.X = a->X; c.Y = a->Y; c.TM = a->TM; c.PW = a->PW; c.idx = a->idx;
  c.par = a->par; c.pm = a->par_m; c.pv = a->par_v; c.rm = a->bn_rm; c.rv = a->bn_rv;
  c.ws = a->ws; c.loss = a->loss; c.ev = a->ev;
  c.nsteps = (int)nsteps; c.evs = nsteps * (1 + 4 * (int64_t)c.ns);
  c.recon_w = a->recon_weight; c.sup_w = a->sup_weight; c.sup_recon_w = a->sup_recon_weight; c.smooth = a->sup_smoothness_weight;
  c.bn_eps = a->bn_eps; c.bn_mom = a->bn_momentum;
  c.eps = (float)a->eps; c.b2 = (float)a->beta2; c.omb1 = (float)(1.0 - a->beta1); c.omb2 = (float)(1.0 - a->beta2);
  c.decay = (float)(1.0 - a->lr * a->weight_decay);
  for (int64_t st = 0; st < nsteps; ++st) {
    const int64_t left = a->n - st * a->B;
    c.step = (int)st;
    c.Bi = left < a->B ? (int)left : a->B;
    c.row0 = a->row0 + st * a->B;
    if (!eval) {
      const double t = (double)(a->tB + st);
      c.neg_step = (float)(-(a->lr / (1.0 - std::pow(a->beta1, t))));
      c.bc2s = (float)std::sqrt(1.0 - std::pow(a->beta2, t));
    }
    e = eval ? rc_launch_dcsfa_eval(c, (hipStream_t)stream) : rc_launch_dcsfa_step(c, (hipStream_t)stream);
    if (e) return e;
  }
  return 0;
}

}  // extern "C"
