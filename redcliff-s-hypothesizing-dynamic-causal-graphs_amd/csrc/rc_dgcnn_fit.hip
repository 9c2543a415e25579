// rc_dgcnn_fit.hip -- the supervised DGCNN baseline (models/dgcnn.py:63-237) as a stand-alone fit:
// BatchNorm over the F features, L = D^-1/2 relu(A) D^-1/2, supports [I, L, L L, ..],
// Z_b = sum_i (S_i x_b) W_i, ReLU, fc1 (n*H -> 64), ReLU, fc2 (64 -> C), MSE(mean), torch.optim.Adam.
// fc1 (64 x n*H, 640 KB at n = 10, H = 250) is far more than a workgroup's LDS, so workgroup (j, replica)
// owns node j: rows j of the supports and the 64 x H block of fc1 that multiplies node j's hidden units.
//
//   k_dg_stats (batch, feature, replica)  every batch's mean / biased variance in double, once per call.
//   k_dg_fwd  (node j, replica)  T_i[b][f] = S_i[j] . x_b[:, f], Z, R = relu(Z) (kept for the backward) and
//        the fc1 partial P[j][b][m] = sum_u fc1[m][j*H + u] R[b][u] on the fp32 matrix cores.
//   k_dg_bwd  (same grid)  sums P over j ascending + bias: f1, out, loss, dout, df1 (every workgroup
//        recomputes this small head; workgroup 0 writes the loss and the fc2 / bias gradients).  Then its own
//        dfc1 block (matrix cores, K = batch, accumulators kept across the passes), dR = df1 . fc1 block
//        (matrix cores, the pre-update block staged in LDS), dZ, dT_i, row j of every dS_i, its partials
//        of dW_i and of the BatchNorm dgamma / dbeta, and Adam on its fc1 block.
//   k_dg_tail (replica)  sums the partials over j ascending, chains dS_i back through the matrix powers
//        and normalize_A to dA, applies Adam to W_i, BatchNorm, the biases, fc2 and A (A only with more
//        than one layer: with one, A receives no gradient and torch's Adam leaves it alone), and updates
//        the running statistics.
//   k_dg_out  (replica; FORWARD)  the head in eval mode: predictions and the batch's MSE.
//
// The launch boundaries on the one stream are the only cross-workgroup dependencies: no workgroup waits
// on another, no atomics, no grid barrier.  Every sum runs in an order fixed by the shape and the batch
// size (windows ascending across passes, units / features / nodes ascending).
#include <cstring>

#include "rc_dgcnn_fit.h"

namespace {

struct DgL {
  float *misc, *f1s, *outs, *fc2s, *fc1s, *Rc, *xs, *Tc, *Th, *dTc, *Lm, *Srow, *Ws;
  float *alpha, *beta, *mean, *inv, *rs, *dinv, *red, *cd;
  int Hp, nq;
};

__device__ inline DgL dg_lds(float* l, const DgCtx& c) {
  DgL L;
  L.Hp = c.H | 1; L.nq = c.nl * c.F;
  L.misc = l; l += DG_MISC;
  L.alpha = L.misc; L.beta = L.misc + 8; L.mean = L.misc + 16; L.inv = L.misc + 24; L.rs = L.misc + 32;
  L.dinv = L.misc + 64; L.red = L.misc + 128; L.cd = L.misc + 160;
  L.f1s = l; l += c.B * 65;
  L.outs = l; l += c.B * c.C;
  L.fc2s = l; l += c.C * DG_M1;
  L.fc1s = l; l += DG_M1 * L.Hp;
  L.Rc = l; l += DG_BC * L.Hp;
  L.xs = l; l += DG_BC * c.F * c.n;
  L.Tc = l; l += DG_BC * L.nq;
  L.Th = l; l += DG_BC * L.nq;
  L.dTc = l; l += DG_BC * L.nq;
  L.Lm = l; l += c.n * c.n;
  L.Srow = l; l += c.nl * c.n;
  L.Ws = l;
  return L;
}

__device__ inline int dg_rep(const DgCtx& c, int i) { return c.rident ? i : (int)c.rmap[i]; }

__device__ inline void dg_adam_at(float* P, float* M, float* V, int64_t idx, float g, const RcAdamScalars& s) {
  float pp = P[idx], mm = M[idx], vv = V[idx];
  rc_adam(pp, mm, vv, g, s);
  P[idx] = pp; M[idx] = mm; V[idx] = vv;
}

// relu(A) -> dst, the degree factors -> dinv, L = (dinv_i a_ik) dinv_k -> Lm (dst may be Lm itself).
__device__ inline void dg_normalize(const DgCtx& c, const float* A, float* ar, float* dinv, float* Lm) {
  const int n = c.n, tid = threadIdx.x;
  for (int e = tid; e < n * n; e += RC_BLOCK) ar[e] = fmaxf(A[e], 0.f);
  __syncthreads();
  if (tid < n) {
    float d = 0.f;
    for (int k = 0; k < n; ++k) d += ar[tid * n + k];
    dinv[tid] = 1.f / sqrtf(d + 1e-10f);
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += RC_BLOCK) {
    const int i = e / n, k = e - i * n;
    const float a = ar[e];
    Lm[e] = (dinv[i] * a) * dinv[k];
  }
  __syncthreads();
}

// BatchNorm scale / shift of feature tid < F, formed as bn_affine_store (rc_embed.hip) forms them.
__device__ inline void dg_bn_affine(const DgCtx& c, const DgL& L, const float* Pg, const float* ws, int r) {
  const int f = threadIdx.x;
  if (f >= c.F) return;
  float mean, inv;
  if (c.mode == REDCLIFF_DGCNN_FIT_TRAIN) {
    const double* st = reinterpret_cast<const double*>(ws + c.w.st) + (int64_t)c.step * 2 * c.F;
    mean = (float)st[f];
    inv = (float)(1.0 / sqrt(st[c.F + f] + c.hyp[r].bn_eps));
  } else {
    mean = c.rm[(int64_t)r * c.F + f];
    inv = 1.0f / sqrtf(c.rv[(int64_t)r * c.F + f] + (float)c.hyp[r].bn_eps);
  }
  const float a = inv * Pg[c.o.bnw + f];
  L.alpha[f] = a;
  {
#pragma clang fp contract(off)
    const float ma = mean * a;  // rounded on its own, as dg_xn rounds x * alpha
    L.beta[f] = Pg[c.o.bnb + f] - ma;
  }
  L.mean[f] = mean;
  L.inv[f] = inv;
}

// What a node workgroup stages once: L, rows j of the supports and their sums, the BatchNorm affine, the
// graph-conv weights and the node's fc1 block.
__device__ inline void dg_stage_node(const DgCtx& c, const DgL& L, const float* Pg, const float* ws, int r, int j) {
  const int n = c.n, H = c.H, Hp = L.Hp, tid = threadIdx.x;
  dg_bn_affine(c, L, Pg, ws, r);
  for (int e = tid; e < L.nq * H; e += RC_BLOCK) {
    const int q = e / H, u = e - q * H;
    L.Ws[q * Hp + u] = Pg[c.o.gcW + e];
  }
  const float* fb = Pg + c.o.fc1W + (int64_t)j * H;
  const int64_t ld = (int64_t)n * H;
  for (int e = tid; e < DG_M1 * H; e += RC_BLOCK) {
    const int m = e / H, u = e - m * H;
    L.fc1s[m * Hp + u] = fb[m * ld + u];
  }
  dg_normalize(c, Pg + c.o.A, L.Lm, L.dinv, L.Lm);
  if (tid < n) {
    L.Srow[tid] = tid == j ? 1.f : 0.f;
    if (c.nl > 1) L.Srow[n + tid] = L.Lm[j * n + tid];
  }
  __syncthreads();
  for (int i = 2; i < c.nl; ++i) {
    if (tid < n) {
      float a = 0.f;
      for (int q = 0; q < n; ++q) a = __builtin_fmaf(L.Srow[(i - 1) * n + q], L.Lm[q * n + tid], a);
      L.Srow[i * n + tid] = a;
    }
    __syncthreads();
  }
  if (tid < c.nl) {
    float a = 0.f;
    for (int k = 0; k < n; ++k) a += L.Srow[tid * n + k];
    L.rs[tid] = a;
  }
  __syncthreads();
}

// The BatchNorm output x * alpha + beta as torch's kernel rounds it: the product, then the sum.  Fused, a
// feature that is constant over the batch (x == mean, beta = b - mean * alpha) would keep the product's
// rounding residue times 1 / sqrt(eps) where both torch and exact arithmetic give b.
__device__ inline float dg_xn(float x, float al, float be) {
#pragma clang fp contract(off)
  const float p = x * al;
  return p + be;
}

// One pass: the raw windows xs[bb][f*n + k] and T[bb][i*F + f] = S_i[j] . (alpha_f x + beta_f); with
// grads also That (the same over the normalised input, for dgamma).  Rows past the batch's end are 0.
__device__ inline void dg_pass_T(const DgCtx& c, const DgL& L, const float* Xr, int b0, int nb, bool grads) {
  const int n = c.n, F = c.F, Fn = F * n, nq = L.nq, tid = threadIdx.x;
  for (int e = tid; e < DG_BC * Fn; e += RC_BLOCK) {
    const int bb = e / Fn, q = e - bb * Fn;
    L.xs[e] = bb < nb ? Xr[(c.row0 + b0 + bb) * (int64_t)c.T * n + q] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < DG_BC * nq; e += RC_BLOCK) {
    const int bb = e / nq, q = e - bb * nq, i = q / F, f = q - i * F;
    float t = 0.f, th = 0.f;
    if (bb < nb) {
      const float* x = L.xs + bb * Fn + f * n;
      const float* s = L.Srow + i * n;
      const float al = L.alpha[f], be = L.beta[f], mu = L.mean[f], iv = L.inv[f];
      for (int k = 0; k < n; ++k) {
        const float xv = x[k];
        t = __builtin_fmaf(s[k], dg_xn(xv, al, be), t);
        if (grads) th = __builtin_fmaf(s[k], (xv - mu) * iv, th);
      }
    }
    L.Tc[e] = t;
    if (grads) L.Th[e] = th;
  }
  __syncthreads();
}

// Z[bb][u] = sum_i (sum_f T_i[bb][f] W_i[f][u]), the supports' products added in order as the reference adds them.
__device__ inline float dg_z(const DgCtx& c, const DgL& L, int bb, int u) {
  const int F = c.F;
  float z = 0.f;
  for (int i = 0; i < c.nl; ++i) {
    float zi = 0.f;
    for (int f = 0; f < F; ++f) zi = __builtin_fmaf(L.Tc[bb * L.nq + i * F + f], L.Ws[(i * F + f) * L.Hp + u], zi);
    z = i == 0 ? zi : z + zi;
  }
  return z;
}

__global__ __launch_bounds__(RC_BLOCK) void k_dg_stats(DgCtx c, int64_t row0, int64_t N) {
  const int ri = blockIdx.z, r = dg_rep(c, ri), s = blockIdx.x, f = blockIdx.y;
  const int64_t b0 = (int64_t)s * c.B;
  const int nb = (int)((N - b0) < c.B ? (N - b0) : c.B);
  const int n = c.n;
  const int64_t rs = (int64_t)c.T * n;
  const float* Xf = c.X + (int64_t)r * c.xps + (row0 + b0) * rs + (int64_t)f * n;
  __shared__ double red[8];
  const int cnt = nb * n;
  double sum = 0.0;
  for (int e = threadIdx.x; e < cnt; e += RC_BLOCK) {
    const int b = e / n, k = e - b * n;
    sum += Xf[b * rs + k];
  }
  const double mean = rc_block_sum_d(sum, red) / (double)cnt;
  double q = 0.0;
  for (int e = threadIdx.x; e < cnt; e += RC_BLOCK) {
    const int b = e / n, k = e - b * n;
    const double v = Xf[b * rs + k] - mean;
    q += v * v;
  }
  const double var = rc_block_sum_d(q, red) / (double)cnt;
  if (threadIdx.x == 0) {
    double* o = reinterpret_cast<double*>(c.ws + (int64_t)ri * c.wss + c.w.st) + (int64_t)s * 2 * c.F;
    o[f] = mean;
    o[c.F + f] = var;
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_dg_fwd(DgCtx c) {
  extern __shared__ float dg_smem[];
  const int j = blockIdx.x, ri = blockIdx.y, r = dg_rep(c, ri), tid = threadIdx.x;
  const int H = c.H, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const DgL L = dg_lds(dg_smem, c);
  const int Hp = L.Hp;
  const float* Pg = c.par + (int64_t)r * c.fs;
  float* ws = c.ws + (int64_t)ri * c.wss;
  const float* Xr = c.X + (int64_t)r * c.xps;
  const bool train = c.mode == REDCLIFF_DGCNN_FIT_TRAIN;
  dg_stage_node(c, L, Pg, ws, r, j);
  for (int b0 = 0; b0 < c.Bi; b0 += DG_BC) {
    const int nb = min(DG_BC, c.Bi - b0);
    dg_pass_T(c, L, Xr, b0, nb, false);
    for (int e = tid; e < DG_BC * H; e += RC_BLOCK) {
      const int bb = e / H, u = e - bb * H;
      float v = 0.f;
      if (bb < nb) {
        v = fmaxf(dg_z(c, L, bb, u), 0.f);
        if (train) ws[c.w.Rg + ((int64_t)j * c.B + b0 + bb) * H + u] = v;
      }
      L.Rc[bb * Hp + u] = v;
    }
    __syncthreads();
    // P[b][m] (windows x fc1 rows): wave wv owns the 16 fc1 rows m = 16 wv + .., K = H
    for (int bt = 0; bt < DG_BC / 16; ++bt) {
      if (bt * 16 >= nb) break;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* ar = L.Rc + (bt * 16 + l15) * Hp;
      const float* br = L.fc1s + (wv * 16 + l15) * Hp;
      acc = rc_mfma_chain16<4, true>(acc, H, lg, [&](int k) { return ar[k]; }, [&](int k) { return br[k]; });
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int b = b0 + bt * 16 + 4 * lg + reg;
        if (b < c.Bi) ws[c.w.P + ((int64_t)j * c.B + b) * DG_M1 + wv * 16 + l15] = acc[reg];
      }
    }
    __syncthreads();
  }
}

// The head every workgroup recomputes: f1 = sum_j P + fc1b, out = fc2 relu(f1) + fc2b, the batch's MSE;
// TRAIN: outs becomes dout and f1s becomes df1.  `lead` writes the loss (and FORWARD's predictions) and,
// in TRAIN, the fc2W / fc2b / fc1b gradients.
__device__ inline void dg_head(const DgCtx& c, const DgL& L, const float* Pg, float* ws, int r, int ri, bool lead) {
  const int Bi = c.Bi, C = c.C, n = c.n, tid = threadIdx.x;
  const bool train = c.mode == REDCLIFF_DGCNN_FIT_TRAIN;
  for (int e = tid; e < Bi * DG_M1; e += RC_BLOCK) {
    const int b = e / DG_M1, m = e - b * DG_M1;
    const float* pp = ws + c.w.P + (int64_t)b * DG_M1 + m;
    float a = pp[0];
    for (int j2 = 1; j2 < n; ++j2) a += pp[(int64_t)j2 * c.B * DG_M1];
    L.f1s[b * 65 + m] = a + Pg[c.o.fc1b + m];
  }
  for (int e = tid; e < C * DG_M1; e += RC_BLOCK) L.fc2s[e] = Pg[c.o.fc2W + e];
  __syncthreads();
  const float* Yr = c.has_y ? c.Y + (int64_t)r * c.yps + c.row0 * C : nullptr;
  const float scale = 2.f / (float)(Bi * C);
  float part = 0.f;
  for (int e = tid; e < Bi * C; e += RC_BLOCK) {
    const int b = e / C, k = e - b * C;
    float a = 0.f;
    for (int m = 0; m < DG_M1; ++m) a = __builtin_fmaf(L.fc2s[k * DG_M1 + m], fmaxf(L.f1s[b * 65 + m], 0.f), a);
    a += Pg[c.o.fc2b + k];
    if (!train && lead) c.pred[((int64_t)ri * c.nout + c.out0 + b) * C + k] = a;
    float dv = 0.f;
    if (Yr) {
      const float diff = a - Yr[e];
      part = __builtin_fmaf(diff, diff, part);
      dv = scale * diff;
    }
    L.outs[e] = dv;
  }
  const float sse = rc_block_sum(part, L.red);
  if (lead && tid == 0 && c.loss && Yr) c.loss[(int64_t)ri * c.nsteps + c.step] = sse / (float)(Bi * C);
  if (!train) return;
  if (lead) {
    float* g = ws + c.w.gfc;
    for (int e = tid; e < C * DG_M1; e += RC_BLOCK) {
      const int k = e / DG_M1, m = e - k * DG_M1;
      float a = 0.f;
      for (int b = 0; b < Bi; ++b) a = __builtin_fmaf(L.outs[b * C + k], fmaxf(L.f1s[b * 65 + m], 0.f), a);
      g[e] = a;
    }
    if (tid < C) {
      float a = 0.f;
      for (int b = 0; b < Bi; ++b) a += L.outs[b * C + tid];
      g[C * DG_M1 + tid] = a;
    }
  }
  __syncthreads();
  for (int e = tid; e < Bi * DG_M1; e += RC_BLOCK) {
    const int b = e / DG_M1, m = e - b * DG_M1;
    float a = 0.f;
    if (L.f1s[b * 65 + m] > 0.f)
      for (int k = 0; k < C; ++k) a = __builtin_fmaf(L.outs[b * C + k], L.fc2s[k * DG_M1 + m], a);
    L.f1s[b * 65 + m] = a;
  }
  __syncthreads();
  if (lead && tid < DG_M1) {
    float a = 0.f;
    for (int b = 0; b < Bi; ++b) a += L.f1s[b * 65 + tid];
    ws[c.w.gfc + C * DG_M1 + C + tid] = a;
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_dg_bwd(DgCtx c) {
  extern __shared__ float dg_smem[];
  const int j = blockIdx.x, ri = blockIdx.y, r = dg_rep(c, ri), tid = threadIdx.x;
  const int n = c.n, F = c.F, H = c.H, nl = c.nl, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const DgL L = dg_lds(dg_smem, c);
  const int Hp = L.Hp, nq = L.nq, Fn = F * n;
  float* Pg = c.par + (int64_t)r * c.fs;
  float* Mg = c.pm + (int64_t)r * c.fs;
  float* Vg = c.pv + (int64_t)r * c.fs;
  float* ws = c.ws + (int64_t)ri * c.wss;
  const float* Xr = c.X + (int64_t)r * c.xps;
  dg_stage_node(c, L, Pg, ws, r, j);
  dg_head(c, L, Pg, ws, r, ri, j == 0);
  __syncthreads();
  f32x4 acc[16];  // dfc1 block: fc1 rows 16 wv + .., 16 unit tiles
#pragma unroll
  for (int ut = 0; ut < 16; ++ut) acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
  float accW[DG_QMAX];  // dW_q[u = tid]
#pragma unroll
  for (int q = 0; q < DG_QMAX; ++q) accW[q] = 0.f;
  float accS = 0.f, accG = 0.f, accB = 0.f;  // dS_i[j][k] (tid = (i-1)*n + k), dgamma / dbeta (tid = f)
  for (int b0 = 0; b0 < c.Bi; b0 += DG_BC) {
    const int nb = min(DG_BC, c.Bi - b0);
    dg_pass_T(c, L, Xr, b0, nb, true);
    for (int e = tid; e < DG_BC * H; e += RC_BLOCK) {
      const int bb = e / H, u = e - bb * H;
      L.Rc[bb * Hp + u] = bb < nb ? ws[c.w.Rg + ((int64_t)j * c.B + b0 + bb) * H + u] : 0.f;
    }
    __syncthreads();
    // dfc1[m][u] += sum_b df1[b][m] R[b][u]: K = the pass's windows, ascending across passes
    {
      const float* ar = L.f1s + b0 * 65 + wv * 16 + l15;
#pragma unroll
      for (int ut = 0; ut < 16; ++ut) {
        if (ut * 16 < H) {
          const int u = ut * 16 + l15;
          const float* br = L.Rc + min(u, H - 1);
          const bool uok = u < H;
          acc[ut] = rc_mfma_chain16<4, true>(acc[ut], nb, lg, [&](int k) { return ar[k * 65]; },
                                             [&](int k) { return br[k * Hp]; }, [&](int k) { return k < nb; },
                                             [&](int k) { return uok && k < nb; });
        }
      }
    }
    __syncthreads();
    // dR[b][u] = sum_m df1[b][m] fc1[m][u] (pre-update block), dZ = dR where R > 0, in place of R
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int ut = wv + 4 * t4;
      if (ut * 16 < H) {
        const int u = ut * 16 + l15;
        const float* br = L.fc1s + min(u, H - 1);
        for (int bt = 0; bt < DG_BC / 16; ++bt) {
          if (bt * 16 >= nb) break;
          const float* ar = L.f1s + min(b0 + bt * 16 + l15, c.Bi - 1) * 65;
          f32x4 a = {0.f, 0.f, 0.f, 0.f};
          a = rc_mfma_chain16<4, true>(a, DG_M1, lg, [&](int k) { return ar[k]; }, [&](int k) { return br[k * Hp]; });
          if (u < H) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int bb = bt * 16 + 4 * lg + reg;
              const float rv = L.Rc[bb * Hp + u];
              L.Rc[bb * Hp + u] = (bb < nb && rv > 0.f) ? a[reg] : 0.f;
            }
          }
        }
      }
    }
    __syncthreads();
    // dT_i[bb][f] = sum_u dZ[bb][u] W_i[f][u]
    for (int e = tid; e < DG_BC * nq; e += RC_BLOCK) {
      const int bb = e / nq, q = e - bb * nq;
      float a = 0.f;
      if (bb < nb) {
        const float* dz = L.Rc + bb * Hp;
        const float* w = L.Ws + q * Hp;
        for (int u = 0; u < H; ++u) a = __builtin_fmaf(dz[u], w[u], a);
      }
      L.dTc[e] = a;
    }
    // dW_q[u] += sum_bb T_q[bb] dZ[bb][u]
    if (tid < H) {
      for (int bb = 0; bb < nb; ++bb) {
        const float dz = L.Rc[bb * Hp + tid];
#pragma unroll
        for (int q = 0; q < DG_QMAX; ++q)
          if (q < nq) accW[q] = __builtin_fmaf(L.Tc[bb * nq + q], dz, accW[q]);
      }
    }
    __syncthreads();
    // dS_i[j][k] += sum_bb sum_f dT_i[bb][f] xn[bb][k][f], i >= 1
    if (tid < (nl - 1) * n) {
      const int i = 1 + tid / n, k = tid - (i - 1) * n;
      for (int bb = 0; bb < nb; ++bb)
        for (int f = 0; f < F; ++f)
          accS = __builtin_fmaf(L.dTc[bb * nq + i * F + f], dg_xn(L.xs[bb * Fn + f * n + k], L.alpha[f], L.beta[f]), accS);
    }
    if (tid >= 128 && tid < 128 + F) {
      const int f = tid - 128;
      for (int bb = 0; bb < nb; ++bb)
        for (int i = 0; i < nl; ++i) {
          const float dt = L.dTc[bb * nq + i * F + f];
          accG = __builtin_fmaf(dt, L.Th[bb * nq + i * F + f], accG);
          accB = __builtin_fmaf(dt, L.rs[i], accB);
        }
    }
    __syncthreads();
  }
  if (tid < H) {
#pragma unroll
    for (int q = 0; q < DG_QMAX; ++q)
      if (q < nq) ws[c.w.dW + ((int64_t)j * nq + q) * H + tid] = accW[q];
  }
  if (tid < (nl - 1) * n) {
    const int i = 1 + tid / n, k = tid - (i - 1) * n;
    ws[c.w.dS + ((int64_t)i * n + j) * n + k] = accS;
  }
  if (tid >= 128 && tid < 128 + F) {
    const int f = tid - 128;
    ws[c.w.dgb + ((int64_t)j * 2) * F + f] = accG;
    ws[c.w.dgb + ((int64_t)j * 2 + 1) * F + f] = accB;
  }
  // Adam on the node's fc1 block
  const RcAdamScalars as = rc_adam_scalars(c.hyp[r].B, c.t);
  const int64_t ld = (int64_t)n * H;
#pragma unroll
  for (int ut = 0; ut < 16; ++ut) {
    const int u = ut * 16 + l15;
    if (ut * 16 < H && u < H) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int m = wv * 16 + 4 * lg + reg;
        dg_adam_at(Pg, Mg, Vg, c.o.fc1W + m * ld + (int64_t)j * H + u, acc[ut][reg], as);
      }
    }
  }
}

// dst[a][b] (+)= sum_q X[a][q] Y[q][b] over n x n matrices in LDS; tx / ty: read X / Y transposed.
__device__ inline void dg_mm(int n, float* dst, const float* X, bool tx, const float* Y, bool ty, bool add) {
  for (int e = threadIdx.x; e < n * n; e += RC_BLOCK) {
    const int a = e / n, b = e - a * n;
    float s = 0.f;
    for (int q = 0; q < n; ++q) s = __builtin_fmaf(tx ? X[q * n + a] : X[a * n + q], ty ? Y[b * n + q] : Y[q * n + b], s);
    dst[e] = add ? dst[e] + s : s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(RC_BLOCK) void k_dg_tail(DgCtx c) {
  extern __shared__ float dg_smem[];
  const int ri = blockIdx.x, r = dg_rep(c, ri), tid = threadIdx.x;
  const int n = c.n, F = c.F, H = c.H, nl = c.nl, C = c.C, nq = nl * F, nn = n * n;
  float* Pg = c.par + (int64_t)r * c.fs;
  float* Mg = c.pm + (int64_t)r * c.fs;
  float* Vg = c.pv + (int64_t)r * c.fs;
  const float* ws = c.ws + (int64_t)ri * c.wss;
  const RcAdamScalars as = rc_adam_scalars(c.hyp[r].B, c.t);
  for (int e = tid; e < nq * H; e += RC_BLOCK) {
    const float* pp = ws + c.w.dW + e;
    float g = pp[0];
    for (int j = 1; j < n; ++j) g += pp[(int64_t)j * nq * H];
    dg_adam_at(Pg, Mg, Vg, c.o.gcW + e, g, as);
  }
  if (tid < 2 * F) {
    const int which = tid / F, f = tid - which * F;
    const float* pp = ws + c.w.dgb + which * F + f;
    float g = pp[0];
    for (int j = 1; j < n; ++j) g += pp[(int64_t)j * 2 * F];
    dg_adam_at(Pg, Mg, Vg, (which ? c.o.bnb : c.o.bnw) + f, g, as);
  }
  const float* gf = ws + c.w.gfc;
  for (int e = tid; e < C * DG_M1; e += RC_BLOCK) dg_adam_at(Pg, Mg, Vg, c.o.fc2W + e, gf[e], as);
  if (tid < C) dg_adam_at(Pg, Mg, Vg, c.o.fc2b + tid, gf[C * DG_M1 + tid], as);
  if (tid >= 64 && tid < 64 + DG_M1) dg_adam_at(Pg, Mg, Vg, c.o.fc1b + (tid - 64), gf[C * DG_M1 + C + (tid - 64)], as);
  // running statistics (torch: double math, momentum * stat + (1 - momentum) * running; unbiased variance)
  if (tid >= 128 && tid < 128 + F) {
    const int f = tid - 128;
    const double* st = reinterpret_cast<const double*>(ws + c.w.st) + (int64_t)c.step * 2 * F;
    const double mom = c.hyp[r].bn_momentum, cnt = (double)c.Bi * n;
    const double var_u = st[F + f] * cnt / (cnt - 1.0);
    c.rm[(int64_t)r * F + f] = (float)(mom * st[f] + (1.0 - mom) * (double)c.rm[(int64_t)r * F + f]);
    c.rv[(int64_t)r * F + f] = (float)(mom * var_u + (1.0 - mom) * (double)c.rv[(int64_t)r * F + f]);
  }
  if (nl < 2) return;  // S_0 = I only: A has no gradient, and torch's Adam then skips it (no decay, no state)
  float* misc = dg_smem;
  float* dinv = misc + 64;
  float* cd = misc + 160;
  float* ar = dg_smem + DG_MISC;
  float* Lm = ar + nn;
  float* dL = Lm + nn;
  float* S = dL + nn;        // S[i] at S + i*nn, i in [1, nl - 2]
  float* G = S + nl * nn;    // G[i] at G + i*nn, i in [1, nl - 1]
  dg_normalize(c, Pg + c.o.A, ar, dinv, Lm);
  for (int e = tid; e < nn; e += RC_BLOCK) {
    dL[e] = 0.f;
    S[nn + e] = Lm[e];
  }
  for (int e = tid; e < (nl - 1) * nn; e += RC_BLOCK) G[nn + e] = ws[c.w.dS + nn + e];
  __syncthreads();
  for (int i = 2; i <= nl - 2; ++i) dg_mm(n, S + i * nn, S + (i - 1) * nn, false, Lm, false, false);
  for (int i = nl - 1; i >= 2; --i) {  // S_i = S_{i-1} L
    dg_mm(n, dL, S + (i - 1) * nn, true, G + i * nn, false, true);
    dg_mm(n, G + (i - 1) * nn, G + i * nn, false, Lm, true, true);
  }
  for (int e = tid; e < nn; e += RC_BLOCK) dL[e] += G[nn + e];
  __syncthreads();
  // normalize_A backward: L_ik = dinv_i a_ik dinv_k, dinv_i = (sum_k a_ik + 1e-10)^-1/2
  if (tid < n) {
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = __builtin_fmaf(dL[tid * n + k] * ar[tid * n + k], dinv[k], s);
    for (int k = 0; k < n; ++k) s = __builtin_fmaf(dL[k * n + tid] * ar[k * n + tid], dinv[k], s);
    const float di = dinv[tid];
    cd[tid] = s * (-0.5f * di * di * di);
  }
  __syncthreads();
  for (int e = tid; e < nn; e += RC_BLOCK) {
    const int i = e / n, k = e - i * n;
    const float g = Pg[c.o.A + e] > 0.f ? __builtin_fmaf(dL[e] * dinv[i], dinv[k], cd[i]) : 0.f;
    dg_adam_at(Pg, Mg, Vg, c.o.A + e, g, as);
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_dg_out(DgCtx c) {
  extern __shared__ float dg_smem[];
  const int ri = blockIdx.x, r = dg_rep(c, ri);
  const DgL L = dg_lds(dg_smem, c);
  dg_head(c, L, c.par + (int64_t)r * c.fs, c.ws + (int64_t)ri * c.wss, r, ri, true);
}

template <class Kern>
int dg_launch(Kern k, const char* what, dim3 grid, size_t bytes, const DgCtx& c, hipStream_t s) {
  // the LDS opt-in is a host call of its own: once per kernel, device and size, not once per launch
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

size_t dg_lds_bytes(const DgCtx& c) {
  return sizeof(float) * (size_t)rc_dgcnn_lds_floats(c.n, c.F, c.nl, c.H, c.C, c.B, c.F, 1);
}

}  // namespace

int rc_launch_dgcnn_stats(const DgCtx& c, int64_t row0, int64_t N, hipStream_t s) {
  hipLaunchKernelGGL(k_dg_stats, dim3(c.nsteps, c.F, c.nrep), dim3(RC_BLOCK), 0, s, c, row0, N);
  return rc_check(hipGetLastError(), "k_dg_stats");
}

int rc_launch_dgcnn_step(const DgCtx& c, hipStream_t s) {
  const size_t bytes = dg_lds_bytes(c);
  const dim3 grid(c.n, c.nrep);
  const int mask = c.launches ? c.launches : 7;
  int e = 0;
  if ((mask & 1) && (e = dg_launch(k_dg_fwd, "k_dg_fwd", grid, bytes, c, s))) return e;
  if ((mask & 2) && (e = dg_launch(k_dg_bwd, "k_dg_bwd", grid, bytes, c, s))) return e;
  if (mask & 4) e = dg_launch(k_dg_tail, "k_dg_tail", dim3(c.nrep), bytes, c, s);
  return e;
}

int rc_launch_dgcnn_forward(const DgCtx& c, hipStream_t s) {
  const size_t bytes = dg_lds_bytes(c);
  const int e = dg_launch(k_dg_fwd, "k_dg_fwd", dim3(c.n, c.nrep), bytes, c, s);
  if (e) return e;
  return dg_launch(k_dg_out, "k_dg_out", dim3(c.nrep), bytes, c, s);
}

extern "C" {

static int dgcnn_fit_dims(const RedcliffDims* d) {
  if (!d) { rc_set_error("null dims"); return REDCLIFF_EINVAL; }
  if (d->R < 1 || d->Bmax < 1 || d->T < 1 || d->p < 1 || d->F < 1 || d->n < 1 || d->H < 1 || d->K < 1) {
    rc_set_error("invalid dims (R=%d Bmax=%d T=%d p=%d F=%d n=%d H=%d K=%d)", d->R, d->Bmax, d->T, d->p, d->F, d->n, d->H,
                 d->K);
    return REDCLIFF_EINVAL;
  }
  if (rc_dgcnn_lds_floats(d->p, d->F, d->n, d->H, d->K, d->Bmax, d->T, d->R) == 0) {
    rc_set_error("dims outside kernel limits (dgcnn fit: nodes<=32 F<=8 layers<=4 hid<=256 classes<=16 Bmax<=128 R<=%d "
                 "T>=F, LDS 256 + Bmax*(65+C) + 64*C + 96*(hid|1) + 32*F*n + 96*layers*F + n*n + layers*n + "
                 "layers*F*(hid|1) <= %d floats; n=%d F=%d layers=%d hid=%d C=%d Bmax=%d T=%d R=%d)", RC_MAX_ACTIVE,
                 RC_LDS_MAX_FLOATS, d->p, d->F, d->n, d->H, d->K, d->Bmax, d->T, d->R);
    return REDCLIFF_ELIMIT;
  }
  return 0;
}

int redcliff_dgcnn_fit_supported(const RedcliffDims* d) {
  if (dgcnn_fit_dims(d) != 0) return 0;
  return (int)rc_dgcnn_lds_floats(d->p, d->F, d->n, d->H, d->K, d->Bmax, d->T, d->R);
}

int64_t redcliff_dgcnn_fit_ws_floats(const RedcliffDims* d, int32_t B, int64_t N) {
  if (dgcnn_fit_dims(d) != 0 || B < 1 || B > d->Bmax || N < 0) return 0;
  return rc_dgcnn_ws(d->p, d->F, d->n, d->H, d->K, B, (N + B - 1) / B).total;
}

int redcliff_dgcnn_fit_run(const RedcliffDgcnnFitArgs* a, void* stream) {
  if (!a) { rc_set_error("null dgcnn fit arguments"); return REDCLIFF_EINVAL; }
  int e = dgcnn_fit_dims(&a->d);
  if (e) return e;
  const RedcliffDims& d = a->d;
  const bool train = a->mode == REDCLIFF_DGCNN_FIT_TRAIN;
  if (!train && a->mode != REDCLIFF_DGCNN_FIT_FORWARD) { rc_set_error("dgcnn_fit_run: bad mode %d", a->mode); return REDCLIFF_EINVAL; }
  if (!a->X || !a->par || !a->ws || !a->hyper || !a->bn_rm || !a->bn_rv ||
      (train ? (!a->Y || !a->par_m || !a->par_v || !a->loss) : (!a->pred || (a->Y && !a->loss)))) {
    rc_set_error("dgcnn_fit_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->launches < 0 || a->launches > 7) { rc_set_error("dgcnn_fit_run: bad launch mask %d", a->launches); return REDCLIFF_EINVAL; }
  if (a->B < 1 || a->B > d.Bmax || a->N < 0 || a->nX < 1 || a->row0 < 0 || a->row0 + a->N > a->nX || (train && a->tB < 1) ||
      a->nX > INT32_MAX) {
    rc_set_error("dgcnn_fit_run: bad arguments (B=%d (1..Bmax=%d) N=%lld row0=%lld nX=%lld tB=%d)", a->B, d.Bmax,
                 (long long)a->N, (long long)a->row0, (long long)a->nX, a->tB);
    return REDCLIFF_EINVAL;
  }
  if (a->x_pstride < 0 || a->y_pstride < 0 || a->par_stride < 0) {
    rc_set_error("dgcnn_fit_run: negative replica stride");
    return REDCLIFF_EINVAL;
  }
  if ((reinterpret_cast<uintptr_t>(a->ws) & 7) != 0) { rc_set_error("dgcnn_fit_run: workspace not 8-byte aligned"); return REDCLIFF_EINVAL; }
  const int64_t nsteps = (a->N + a->B - 1) / a->B;
  if (nsteps > 65535) { rc_set_error("dgcnn_fit_run: %lld steps in one call (at most 65535)", (long long)nsteps); return REDCLIFF_ELIMIT; }
  DgCtx c;
  memset(&c, 0, sizeof(c));
  if (a->replicas) {  // the rules of RedcliffStepArgs.replicas
    if (a->n_replicas < 0 || a->n_replicas > d.R) {
      rc_set_error("dgcnn_fit_run: active replica list of %d entries (at most R=%d)", a->n_replicas, d.R);
      return REDCLIFF_EINVAL;
    }
    for (int i = 0; i < a->n_replicas; ++i) {
      const int r = a->replicas[i];
      if (r < 0 || r >= d.R || (i > 0 && r <= a->replicas[i - 1])) {
        rc_set_error("dgcnn_fit_run: active replica list must be strictly increasing indices < R=%d (entry %d = %d)", d.R, i, r);
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
  c.n = d.p; c.F = d.F; c.nl = d.n; c.H = d.H; c.C = d.K; c.T = d.T; c.B = a->B; c.mode = a->mode;
  c.nsteps = (int)nsteps; c.launches = a->launches; c.has_y = a->Y != nullptr;
  c.w = rc_dgcnn_ws(c.n, c.F, c.nl, c.H, c.C, c.B, nsteps);
  c.wss = c.w.total;
  if (a->ws_bytes < sizeof(float) * (size_t)c.wss * (size_t)c.nrep) {
    rc_set_error("dgcnn_fit_run: workspace of %zu bytes, %zu needed", a->ws_bytes, sizeof(float) * (size_t)c.wss * (size_t)c.nrep);
    return REDCLIFF_EWORKSPACE;
  }
  if (a->N == 0 || c.nrep == 0) return 0;
  c.nout = a->N; c.xps = a->x_pstride; c.yps = a->y_pstride; c.fs = a->par_stride;
  c.X = a->X; c.Y = a->Y; c.par = a->par; c.pm = a->par_m; c.pv = a->par_v; c.rm = a->bn_rm; c.rv = a->bn_rv; c.hyp = a->hyper;
  c.ws = a->ws; c.loss = a->loss; c.pred = a->pred;
  RedcliffDims ed = d;
  ed.M1 = DG_M1;
  c.o = rc_emb_off(ed);
  if (train && (e = rc_launch_dgcnn_stats(c, a->row0, a->N, (hipStream_t)stream))) return e;
  for (int64_t st = 0; st < nsteps; ++st) {
    const int64_t left = a->N - st * a->B;
    c.step = (int)st;
    c.Bi = left < a->B ? (int)left : a->B;
    c.t = a->tB + (int)st;
    c.row0 = a->row0 + st * a->B;
    c.out0 = st * a->B;
    e = train ? rc_launch_dgcnn_step(c, (hipStream_t)stream) : rc_launch_dgcnn_forward(c, (hipStream_t)stream);
    if (e) return e;
  }
  return 0;
}

}  // extern "C"
