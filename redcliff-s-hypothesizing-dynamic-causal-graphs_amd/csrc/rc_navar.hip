// rc_navar.hip -- the NAVAR (MLP) additive baseline (models/navar.py:9-125): N per-source networks
// Conv1d(K) -> clamp -> (Conv1d(H) -> clamp) -> Conv1d(H) contributions, summed over the sources into
// one prediction before the loss.  A network has H*K + H*H + N*H weights (885 KB with both Adam
// moments at H = 256), far more than a workgroup's LDS, so the weights stay in global memory (L2) and a
// workgroup owns a SLICE of NV_SL = 32 units of the last hidden layer of one source of one replica:
//
//   k_navar_fwd (slice s, source i, replica)  recomputes h1 for the pass's 64 windows, forms its 32
//        units of z2 (fp32 matrix cores: a 64 x 32 x H product per pass) and writes the slice's
//        partial contributions P[r][i][s][b][j] (bc_ij starts slice 0's chain).
//   k_navar_bwd (same grid)  sums P over s ascending, then over i ascending, + biases: res, dc.
//        Workgroup (0, 0, r) writes the step's mse / l1 and dbiases.  It recomputes its slice's
//        forward, forms dWc, dbc, dz2, db2, dW2 (matrix cores, accumulators continue across the
//        passes through LDS) and its partial dh1 D[r][i][s][b][v] = dz2 . W2 slice (matrix cores, the
//        pre-update W2 staged in LDS), then applies Adam to what it owns: its W2 rows, b2, Wc columns,
//        (slice 0) bc.  With one hidden layer the slice is of the first layer and it updates W1 / b1.
//   k_navar_in  (two layers; same grid, slices of the FIRST layer) sums D over s ascending, applies the
//        z1 >= 0 mask, forms dW1 / db1 and applies Adam; workgroup (0, 0, r) also updates biases, which
//        every workgroup of k_navar_bwd read.  With one layer only that biases update is launched.
//
// The launch boundaries on the one stream are the only cross-workgroup dependencies: no workgroup
// waits on another, no atomics, no grid barrier.  Every sum runs in an order fixed by the shape and
// the batch size (windows ascending across passes, units ascending, slices then sources ascending).
// v_mfma_f32_16x16x4_f32 is an exact in-order fmaf chain over k (rc_gemm.h), its C operand the chain's
// start, so continuing a chain through LDS between passes keeps the window order.
#include <cstring>

#include "rc_navar.h"

namespace {

struct NvLds {
  float *xs, *zs, *dzs, *Wcs, *gWc, *dcs, *dps, *gb, *gbc, *gbi, *red, *gW1, *h1s, *Ws, *Gr;
  int* rows;
  RcAdamScalars* as;
  int Kp, Np, Hp;
};

__device__ inline NvLds nv_lds(float* l, int N, int H, int K, int two) {
  NvLds L;
  L.Kp = K | 1; L.Np = N | 1; L.Hp = rc_navar_hp(H);
  L.xs = l; l += NV_BC * L.Kp;
  L.zs = l; l += NV_BC * 33;
  L.dzs = l; l += NV_BC * 33;
  L.Wcs = l; l += N * 33;
  L.gWc = l; l += N * 33;
  L.dcs = l; l += NV_BC * L.Np;
  L.dps = l; l += NV_BC * L.Np;
  L.gb = l; L.gbc = l + 32; L.gbi = l + 64; L.red = l + 96;
  L.rows = reinterpret_cast<int*>(l + 112);
  L.as = reinterpret_cast<RcAdamScalars*>(l + 176);
  l += NV_MISC;
  L.gW1 = l;  // one layer (k_navar_bwd) or k_navar_in: the dW1 slice [32][Kp]
  L.h1s = l;  // two layers: [64][Hp]
  L.Ws = L.h1s + NV_BC * L.Hp;   // [32][Hp]
  L.Gr = L.Ws + NV_SL * L.Hp;    // [32][Hp]
  return L;
}

__device__ inline float nv_z1(const float* w, const float* x, int K, float b) {
  float a = 0.f;
  for (int k = 0; k < K; ++k) a = __builtin_fmaf(w[k], x[k], a);
  return a + b;
}

__device__ inline void nv_adam_at(float* P, float* M, float* V, int64_t idx, float g, const RcAdamScalars& s) {
  float pp = P[idx], mm = M[idx], vv = V[idx];
  rc_adam(pp, mm, vv, g, s);
  P[idx] = pp; M[idx] = mm; V[idx] = vv;
}

// Rows and lags of the pass's windows: rows[b], xs[b][k] = X[row][k][i] (0 past the batch's end).
__device__ inline void nv_stage_x(const NavarCtx& c, const NvLds& L, const float* Xr, const int32_t* permr, int i,
                                  int b0, int nbc) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid < NV_BC) {
    int64_t row = 0;
    if (tid < nbc) {
      const int64_t q = c.q0 + b0 + tid;
      row = permr ? (int64_t)permr[q] : q;
      row = row < 0 ? 0 : (row >= c.nX ? c.nX - 1 : row);
    }
    L.rows[tid] = (int)row;
  }
  __syncthreads();
  for (int e = tid; e < NV_BC * c.K; e += RC_BLOCK) {
    const int b = e / c.K, k = e - b * c.K;
    L.xs[b * L.Kp + k] = b < nbc ? Xr[((int64_t)L.rows[b] * c.T + k) * c.N + i] : 0.f;
  }
  __syncthreads();
}

// The slice's pre-activations zs[b][ul] of the last hidden layer for the staged windows (0 for units
// past H); with two layers h1s[b][v] of the whole first layer on the way.
__device__ inline void nv_slice_forward(const NavarCtx& c, const NvLds& L, const float* Pg, int i, int s) {
  const int tid = threadIdx.x, H = c.H, K = c.K;
  const float* W1 = Pg + c.o.W1 + (int64_t)i * H * K;
  const float* b1 = Pg + c.o.b1 + (int64_t)i * H;
  if (c.two) {
    for (int v = tid; v < H; v += RC_BLOCK) {
      const float* w = W1 + (int64_t)v * K;
      const float bv = b1[v];
      for (int bg = 0; bg < NV_BC; bg += 8) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float* x = L.xs + bg * L.Kp;
        for (int k = 0; k < K; ++k) {
          const float wv = w[k];
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[q] = __builtin_fmaf(wv, x[q * L.Kp + k], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) L.h1s[(bg + q) * L.Hp + v] = fmaxf(acc[q] + bv, 0.f);
      }
    }
    __syncthreads();
    // z2[b][u] = sum_v h1[b][v] W2[u][v]: wave w owns windows [16w, 16w + 16) x the slice's 32 units
    const int lane = tid & 63, w = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    const float* Ar = L.h1s + (16 * w + l15) * L.Hp + kq;
    const float* B0 = L.Ws + l15 * L.Hp + kq;
    const float* B1 = L.Ws + (16 + l15) * L.Hp + kq;
    for (int kk = 0; kk < H; kk += 4) {
      const float av = Ar[kk];
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, B0[kk], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, B1[kk], a1, 0, 0, 0);
    }
    const float* b2 = Pg + c.o.b2 + (int64_t)i * H;
    const int u0 = s * NV_SL + l15, u1 = u0 + 16;
    const float bu0 = u0 < H ? b2[u0] : 0.f, bu1 = u1 < H ? b2[u1] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int b = 16 * w + 4 * kq + reg;
      L.zs[b * 33 + l15] = a0[reg] + bu0;
      L.zs[b * 33 + 16 + l15] = a1[reg] + bu1;
    }
  } else {
    for (int e = tid; e < NV_BC * NV_SL; e += RC_BLOCK) {
      const int b = e >> 5, ul = e & 31, u = s * NV_SL + ul;
      L.zs[b * 33 + ul] = u < H ? nv_z1(W1 + (int64_t)u * K, L.xs + b * L.Kp, K, b1[u]) : 0.f;
    }
  }
  __syncthreads();
}

// What a slice workgroup keeps in LDS for the whole launch: the slice's Wc columns and, with two
// layers, its W2 rows (zero past H in both directions) and zeroed h1 padding columns.
__device__ inline void nv_stage_weights(const NavarCtx& c, const NvLds& L, const float* Pg, int i, int s, bool grads) {
  const int tid = threadIdx.x, H = c.H, N = c.N;
  const float* Wc = Pg + c.o.Wc + (int64_t)i * N * H;
  for (int e = tid; e < N * 33; e += RC_BLOCK) {
    const int j = e / 33, ul = e - j * 33, u = s * NV_SL + ul;
    L.Wcs[e] = (ul < NV_SL && u < H) ? Wc[(int64_t)j * H + u] : 0.f;
    if (grads) L.gWc[e] = 0.f;
  }
  if (grads && tid < 96) L.gb[tid] = 0.f;  // gb | gbc | gbi
  if (c.two) {
    const float* W2 = Pg + c.o.W2 + (int64_t)i * H * H;
    for (int e = tid; e < NV_SL * L.Hp; e += RC_BLOCK) {
      const int ul = e / L.Hp, v = e - ul * L.Hp, u = s * NV_SL + ul;
      L.Ws[e] = (u < H && v < H) ? W2[(int64_t)u * H + v] : 0.f;
      if (grads) L.Gr[e] = 0.f;
    }
    for (int e = tid; e < NV_BC * L.Hp; e += RC_BLOCK) L.h1s[e] = 0.f;
  } else if (grads) {
    for (int e = tid; e < NV_SL * L.Kp; e += RC_BLOCK) L.gW1[e] = 0.f;
  }
}

#define NV_PROLOGUE                                                                  \
  extern __shared__ float lds[];                                                     \
  const int s = blockIdx.x, i = blockIdx.y, ri = blockIdx.z, tid = threadIdx.x;      \
  const int r = c.rident ? ri : (int)c.rmap[ri];                                     \
  const int N = c.N, H = c.H, K = c.K, nS = rc_navar_slices(H);                      \
  const NvLds L = nv_lds(lds, N, H, K, c.two);                                       \
  float* Pg = c.par + (int64_t)r * c.fs;                                             \
  const float* Xr = c.X + (int64_t)r * c.xps;                                        \
  const int32_t* permr = c.perm ? c.perm + (int64_t)r * c.pps : nullptr;             \
  float* wsr = c.ws + (int64_t)ri * c.wss;                                           \
  float* Pw = wsr;                                                                   \
  float* Dw = wsr + (int64_t)N * nS * c.B * N;                                       \
  float* GB = wsr + c.wss - 32;                                                      \
  (void)K; (void)Dw; (void)GB; (void)Pw; (void)permr; (void)Xr; (void)tid

__global__ __launch_bounds__(RC_BLOCK) void k_navar_fwd(NavarCtx c) {
  NV_PROLOGUE;
  nv_stage_weights(c, L, Pg, i, s, false);
  const float* bc = Pg + c.o.bc + (int64_t)i * N;
  float* Pis = Pw + ((int64_t)i * nS + s) * c.B * N;
  for (int b0 = 0; b0 < c.Bi; b0 += NV_BC) {
    const int nbc = c.Bi - b0 < NV_BC ? c.Bi - b0 : NV_BC;
    nv_stage_x(c, L, Xr, permr, i, b0, nbc);
    nv_slice_forward(c, L, Pg, i, s);
    for (int e = tid; e < nbc * N; e += RC_BLOCK) {
      const int b = e / N, j = e - b * N;
      float acc = s == 0 ? bc[j] : 0.f;
      for (int ul = 0; ul < NV_SL; ++ul) acc = __builtin_fmaf(L.Wcs[j * 33 + ul], fmaxf(L.zs[b * 33 + ul], 0.f), acc);
      Pis[(int64_t)(b0 + b) * N + j] = acc;
    }
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_navar_bwd(NavarCtx c) {
  NV_PROLOGUE;
  const bool lead = s == 0 && i == 0;
  const RedcliffReplicaHyper& hy = c.hyp[r];
  nv_stage_weights(c, L, Pg, i, s, true);
  if (tid == RC_BLOCK - 1) *L.as = rc_adam_scalars(hy.B, c.t);
  const float* biases = Pg + c.o.bias;
  const float dscale = 2.f / (float)(c.Bi * N);
  const float lamc = (hy.c_adj / (float)N) / (float)c.Bi;
  const int lane = tid & 63, w = tid >> 6, l15 = lane & 15, kq = lane >> 4;
  const int nvt = (H + 15) >> 4;
  float sq = 0.f, ab = 0.f;
  for (int b0 = 0; b0 < c.Bi; b0 += NV_BC) {
    const int nbc = c.Bi - b0 < NV_BC ? c.Bi - b0 : NV_BC;
    nv_stage_x(c, L, Xr, permr, i, b0, nbc);
    nv_slice_forward(c, L, Pg, i, s);
    // A. contributions of every source (slices ascending), prediction (sources ascending), residual, dc
    for (int e = tid; e < NV_BC * N; e += RC_BLOCK) {
      const int b = e / N, j = e - b * N;
      float dc = 0.f, dp = 0.f;
      if (b < nbc) {
        float pred = 0.f, own = 0.f;
        for (int i2 = 0; i2 < N; ++i2) {
          const float* pp = Pw + ((int64_t)i2 * nS * c.B + (b0 + b)) * N + j;
          float ci = pp[0];
          for (int s2 = 1; s2 < nS; ++s2) ci += pp[(int64_t)s2 * c.B * N];
          pred = i2 == 0 ? ci : pred + ci;
          if (i2 == i) own = ci;
          ab += fabsf(ci);
        }
        pred += biases[j];
        const float res = pred - Xr[((int64_t)L.rows[b] * c.T + K) * N + j];
        sq = __builtin_fmaf(res, res, sq);
        dp = dscale * res;
        dc = __builtin_fmaf(lamc, rc_sign(own), dp);
      }
      L.dcs[b * L.Np + j] = dc;
      L.dps[b * L.Np + j] = dp;
    }
    __syncthreads();
    // B. dWc slice (windows ascending, continuing), dbc, dbiases, dz of the slice
    for (int e = tid; e < N * NV_SL; e += RC_BLOCK) {
      const int j = e >> 5, ul = e & 31;
      float acc = L.gWc[j * 33 + ul];
      for (int b = 0; b < nbc; ++b) acc = __builtin_fmaf(L.dcs[b * L.Np + j], fmaxf(L.zs[b * 33 + ul], 0.f), acc);
      L.gWc[j * 33 + ul] = acc;
    }
    if (s == 0 && tid < N) {
      float acc = L.gbc[tid];
      for (int b = 0; b < nbc; ++b) acc += L.dcs[b * L.Np + tid];
      L.gbc[tid] = acc;
    }
    if (lead && tid >= 64 && tid < 64 + N) {
      const int j = tid - 64;
      float acc = L.gbi[j];
      for (int b = 0; b < nbc; ++b) acc += L.dps[b * L.Np + j];
      L.gbi[j] = acc;
    }
    for (int e = tid; e < NV_BC * NV_SL; e += RC_BLOCK) {
      const int b = e >> 5, ul = e & 31;
      float dh = 0.f;
      for (int j = 0; j < N; ++j) dh = __builtin_fmaf(L.dcs[b * L.Np + j], L.Wcs[j * 33 + ul], dh);
      L.dzs[b * 33 + ul] = (b < nbc && L.zs[b * 33 + ul] >= 0.f) ? dh : 0.f;
    }
    __syncthreads();
    // C. bias gradient of the slice's layer, its weight gradient, and (two layers) the partial dh1
    if (tid < NV_SL) {
      float acc = L.gb[tid];
      for (int b = 0; b < nbc; ++b) acc += L.dzs[b * 33 + tid];
      L.gb[tid] = acc;
    }
    if (c.two) {
      // dW2[u][v] += sum_b dz[b][u] h1[b][v]: tiles (mt, nt) of 16 x 16 dealt over the waves
      for (int t = w; t < 2 * nvt; t += 4) {
        const int mt = t & 1, nt = t >> 1;
        f32x4 acc;
        float* g = L.Gr + (mt * 16 + 4 * kq) * L.Hp + nt * 16 + l15;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) acc[reg] = g[reg * L.Hp];
        const float* Ad = L.dzs + kq * 33 + mt * 16 + l15;
        const float* Bh = L.h1s + kq * L.Hp + nt * 16 + l15;
#pragma unroll 4
        for (int kk = 0; kk < NV_BC; kk += 4)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ad[kk * 33], Bh[kk * L.Hp], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) g[reg * L.Hp] = acc[reg];
      }
      // D[b][v] = sum_{u in slice} dz[b][u] W2[u][v] (the W2 this step's forward used)
      float* Dis = Dw + ((int64_t)i * nS + s) * c.B * H;
      const float* Ad = L.dzs + (16 * w + l15) * 33 + kq;
      for (int nt = 0; nt < nvt; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* Bw = L.Ws + kq * L.Hp + nt * 16 + l15;
#pragma unroll
        for (int kk = 0; kk < NV_SL; kk += 4)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ad[kk], Bw[kk * L.Hp], acc, 0, 0, 0);
        const int v = nt * 16 + l15;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int b = 16 * w + 4 * kq + reg;
          if (b < nbc && v < H) Dis[(int64_t)(b0 + b) * H + v] = acc[reg];
        }
      }
    } else {
      for (int e = tid; e < NV_SL * K; e += RC_BLOCK) {
        const int ul = e / K, k = e - ul * K;
        float acc = L.gW1[ul * L.Kp + k];
        for (int b = 0; b < nbc; ++b) acc = __builtin_fmaf(L.dzs[b * 33 + ul], L.xs[b * L.Kp + k], acc);
        L.gW1[ul * L.Kp + k] = acc;
      }
    }
  }
  if (lead) {  // block-uniform
    const float sqs = rc_block_sum(sq, L.red);
    const float abs_ = rc_block_sum(ab, L.red);
    if (tid == 0) {
      const int64_t o = (int64_t)ri * c.nsteps + c.step;
      c.mse[o] = sqs / (float)(c.Bi * N);
      c.l1[o] = (hy.c_adj / (float)N) * (abs_ / (float)c.Bi);
    }
  }
  __syncthreads();
  if (lead && tid < N) GB[tid] = L.gbi[tid];
  // the update of what this workgroup owns
  const RcAdamScalars as = *L.as;
  float* Mg = c.pm + (int64_t)r * c.fs;
  float* Vg = c.pv + (int64_t)r * c.fs;
  for (int e = tid; e < N * NV_SL; e += RC_BLOCK) {
    const int j = e >> 5, ul = e & 31, u = s * NV_SL + ul;
    if (u < H) nv_adam_at(Pg, Mg, Vg, c.o.Wc + ((int64_t)i * N + j) * H + u, L.gWc[j * 33 + ul], as);
  }
  if (tid < NV_SL && s * NV_SL + tid < H)
    nv_adam_at(Pg, Mg, Vg, (c.two ? c.o.b2 : c.o.b1) + (int64_t)i * H + s * NV_SL + tid, L.gb[tid], as);
  if (s == 0 && tid >= 64 && tid < 64 + N) nv_adam_at(Pg, Mg, Vg, c.o.bc + (int64_t)i * N + (tid - 64), L.gbc[tid - 64], as);
  if (c.two) {
    for (int e = tid; e < NV_SL * H; e += RC_BLOCK) {
      const int ul = e / H, v = e - ul * H, u = s * NV_SL + ul;
      if (u < H) nv_adam_at(Pg, Mg, Vg, c.o.W2 + ((int64_t)i * H + u) * H + v, L.Gr[ul * L.Hp + v], as);
    }
  } else {
    for (int e = tid; e < NV_SL * K; e += RC_BLOCK) {
      const int ul = e / K, k = e - ul * K, u = s * NV_SL + ul;
      if (u < H) nv_adam_at(Pg, Mg, Vg, c.o.W1 + ((int64_t)i * H + u) * K + k, L.gW1[ul * L.Kp + k], as);
    }
  }
}

// Two layers: the first layer's slice s of source i.  One layer: launched on grid (1, 1, replicas) for
// the biases update alone.
__global__ __launch_bounds__(RC_BLOCK) void k_navar_in(NavarCtx c) {
  NV_PROLOGUE;
  const bool lead = s == 0 && i == 0;
  const RedcliffReplicaHyper& hy = c.hyp[r];
  if (tid == RC_BLOCK - 1) *L.as = rc_adam_scalars(hy.B, c.t);
  float* Mg = c.pm + (int64_t)r * c.fs;
  float* Vg = c.pv + (int64_t)r * c.fs;
  if (c.two) {
    if (tid < NV_SL) L.gb[tid] = 0.f;
    for (int e = tid; e < NV_SL * L.Kp; e += RC_BLOCK) L.gW1[e] = 0.f;
    const float* W1 = Pg + c.o.W1 + (int64_t)i * H * K;
    const float* b1 = Pg + c.o.b1 + (int64_t)i * H;
    const float* Di = Dw + (int64_t)i * nS * c.B * H;
    for (int b0 = 0; b0 < c.Bi; b0 += NV_BC) {
      const int nbc = c.Bi - b0 < NV_BC ? c.Bi - b0 : NV_BC;
      nv_stage_x(c, L, Xr, permr, i, b0, nbc);
      for (int e = tid; e < NV_BC * NV_SL; e += RC_BLOCK) {
        const int b = e >> 5, ul = e & 31, v = s * NV_SL + ul;
        float dz = 0.f;
        if (b < nbc && v < H) {
          const float z = nv_z1(W1 + (int64_t)v * K, L.xs + b * L.Kp, K, b1[v]);
          const float* dp = Di + (int64_t)(b0 + b) * H + v;
          float dh = dp[0];
          for (int s2 = 1; s2 < nS; ++s2) dh += dp[(int64_t)s2 * c.B * H];
          dz = z >= 0.f ? dh : 0.f;
        }
        L.dzs[b * 33 + ul] = dz;
      }
      __syncthreads();
      if (tid < NV_SL) {
        float acc = L.gb[tid];
        for (int b = 0; b < nbc; ++b) acc += L.dzs[b * 33 + tid];
        L.gb[tid] = acc;
      }
      for (int e = tid; e < NV_SL * K; e += RC_BLOCK) {
        const int ul = e / K, k = e - ul * K;
        float acc = L.gW1[ul * L.Kp + k];
        for (int b = 0; b < nbc; ++b) acc = __builtin_fmaf(L.dzs[b * 33 + ul], L.xs[b * L.Kp + k], acc);
        L.gW1[ul * L.Kp + k] = acc;
      }
    }
  }
  __syncthreads();
  const RcAdamScalars as = *L.as;
  if (c.two) {
    for (int e = tid; e < NV_SL * K; e += RC_BLOCK) {
      const int ul = e / K, k = e - ul * K, u = s * NV_SL + ul;
      if (u < H) nv_adam_at(Pg, Mg, Vg, c.o.W1 + ((int64_t)i * H + u) * K + k, L.gW1[ul * L.Kp + k], as);
    }
    if (tid < NV_SL && s * NV_SL + tid < H) nv_adam_at(Pg, Mg, Vg, c.o.b1 + (int64_t)i * H + s * NV_SL + tid, L.gb[tid], as);
  }
  if (lead && tid >= 64 && tid < 64 + N) nv_adam_at(Pg, Mg, Vg, c.o.bias + (tid - 64), GB[tid - 64], as);
}

// FORWARD: contrib[row][i*N + j] = sum_s P (ascending), pred[row][j] = sum_i (ascending) + biases_j.
__global__ __launch_bounds__(RC_BLOCK) void k_navar_out(NavarCtx c) {
  const int ri = blockIdx.y, r = c.rident ? ri : (int)c.rmap[ri];
  const int N = c.N, nS = rc_navar_slices(c.H);
  const float* Pw = c.ws + (int64_t)ri * c.wss;
  const float* biases = c.par + (int64_t)r * c.fs + c.o.bias;
  const int e = blockIdx.x * RC_BLOCK + threadIdx.x;
  if (e >= c.Bi * N) return;
  const int b = e / N, j = e - b * N;
  const int64_t row = (int64_t)ri * c.nout + c.out0 + b;
  float pred = 0.f;
  for (int i2 = 0; i2 < N; ++i2) {
    const float* pp = Pw + ((int64_t)i2 * nS * c.B + b) * N + j;
    float ci = pp[0];
    for (int s2 = 1; s2 < nS; ++s2) ci += pp[(int64_t)s2 * c.B * N];
    pred = i2 == 0 ? ci : pred + ci;
    c.contrib[row * N * N + (int64_t)i2 * N + j] = ci;
  }
  c.pred[row * N + j] = pred + biases[j];
}

template <class Kern>
int nv_launch(Kern k, const char* what, dim3 grid, size_t bytes, const NavarCtx& c, hipStream_t s) {
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

size_t nv_lds_bytes(const NavarCtx& c) {
  return sizeof(float) * (size_t)rc_navar_lds_floats(c.N, c.H, c.K, c.two ? 2 : 1, 1, c.K + 1, 1);
}

}  // namespace

int rc_launch_navar_step(const NavarCtx& c, hipStream_t s) {
  const size_t bytes = nv_lds_bytes(c);
  const dim3 grid(rc_navar_slices(c.H), c.N, c.nrep);
  const int mask = c.launches ? c.launches : 7;
  int e = 0;
  if ((mask & 1) && (e = nv_launch(k_navar_fwd, "k_navar_fwd", grid, bytes, c, s))) return e;
  if ((mask & 2) && (e = nv_launch(k_navar_bwd, "k_navar_bwd", grid, bytes, c, s))) return e;
  if (mask & 4) e = nv_launch(k_navar_in, "k_navar_in", c.two ? grid : dim3(1, 1, c.nrep), bytes, c, s);
  return e;
}

int rc_launch_navar_forward(const NavarCtx& c, hipStream_t s) {
  const dim3 grid(rc_navar_slices(c.H), c.N, c.nrep);
  int e = nv_launch(k_navar_fwd, "k_navar_fwd", grid, nv_lds_bytes(c), c, s);
  if (e) return e;
  hipLaunchKernelGGL(k_navar_out, dim3((c.Bi * c.N + RC_BLOCK - 1) / RC_BLOCK, c.nrep), dim3(RC_BLOCK), 0, s, c);
  return rc_check(hipGetLastError(), "k_navar_out");
}

extern "C" {

static int navar_dims(const RedcliffDims* d) {
  if (!d) { rc_set_error("null dims"); return REDCLIFF_EINVAL; }
  if (d->R < 1 || d->Bmax < 1 || d->T < 1 || d->p < 1 || d->L < 1 || d->h < 1 || d->n < 1) {
    rc_set_error("invalid dims (R=%d Bmax=%d T=%d p=%d L=%d h=%d n=%d)", d->R, d->Bmax, d->T, d->p, d->L, d->h, d->n);
    return REDCLIFF_EINVAL;
  }
  if (rc_navar_lds_floats(d->p, d->h, d->L, d->n, d->Bmax, d->T, d->R) == 0) {
    rc_set_error("dims outside kernel limits (navar: N<=32 H<=512 K<=64 Bmax<=512 R<=%d layers 1|2 T>=K+1, LDS 64*(K|1) + "
                 "4224 + 66*N + 128*(N|1) + 240 + (two ? 128*(ceil16(H)|1) : 32*(K|1)) <= %d floats; N=%d H=%d K=%d "
                 "layers=%d Bmax=%d T=%d R=%d)", RC_MAX_ACTIVE, RC_LDS_MAX_FLOATS, d->p, d->h, d->L, d->n, d->Bmax, d->T,
                 d->R);
    return REDCLIFF_ELIMIT;
  }
  return 0;
}

int redcliff_navar_supported(const RedcliffDims* d) {
  if (navar_dims(d) != 0) return 0;
  return (int)rc_navar_lds_floats(d->p, d->h, d->L, d->n, d->Bmax, d->T, d->R);
}

int redcliff_navar_run(const RedcliffNavarArgs* a, void* stream) {
  if (!a) { rc_set_error("null navar arguments"); return REDCLIFF_EINVAL; }
  int e = navar_dims(&a->d);
  if (e) return e;
  const RedcliffDims& d = a->d;
  const bool train = a->mode == REDCLIFF_NAVAR_TRAIN;
  if (!train && a->mode != REDCLIFF_NAVAR_FORWARD) { rc_set_error("navar_run: bad mode %d", a->mode); return REDCLIFF_EINVAL; }
  if (!a->X || !a->par || !a->ws ||
      (train ? (!a->perm || !a->par_m || !a->par_v || !a->hyper || !a->mse || !a->l1) : (!a->pred || !a->contrib))) {
    rc_set_error("navar_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->launches < 0 || a->launches > 7) { rc_set_error("navar_run: bad launch mask %d", a->launches); return REDCLIFF_EINVAL; }
  if (a->B < 1 || a->B > d.Bmax || a->N < 0 || a->nX < 1 || (train && a->tB < 1) ||
      (!train && (a->row0 < 0 || a->row0 + a->N > a->nX)) || a->nX > INT32_MAX) {
    rc_set_error("navar_run: bad arguments (B=%d (1..Bmax=%d) N=%lld row0=%lld nX=%lld tB=%d)", a->B, d.Bmax,
                 (long long)a->N, (long long)a->row0, (long long)a->nX, a->tB);
    return REDCLIFF_EINVAL;
  }
  if (a->x_pstride < 0 || a->perm_pstride < 0 || a->par_stride < 0) {
    rc_set_error("navar_run: negative replica stride");
    return REDCLIFF_EINVAL;
  }
  const int64_t nsteps = (a->N + a->B - 1) / a->B;
  if (nsteps > INT32_MAX / 2) { rc_set_error("navar_run: too many steps"); return REDCLIFF_ELIMIT; }
  NavarCtx c;
  memset(&c, 0, sizeof(c));
  if (a->replicas) {  // the rules of RedcliffStepArgs.replicas
    if (a->n_replicas < 0 || a->n_replicas > d.R) {
      rc_set_error("navar_run: active replica list of %d entries (at most R=%d)", a->n_replicas, d.R);
      return REDCLIFF_EINVAL;
    }
    for (int i = 0; i < a->n_replicas; ++i) {
      const int r = a->replicas[i];
      if (r < 0 || r >= d.R || (i > 0 && r <= a->replicas[i - 1])) {
        rc_set_error("navar_run: active replica list must be strictly increasing indices < R=%d (entry %d = %d)", d.R, i, r);
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
  c.N = d.p; c.H = d.h; c.K = d.L; c.T = d.T; c.two = d.n == 2; c.B = a->B; c.mode = a->mode; c.nsteps = (int)nsteps; c.launches = a->launches;
  c.wss = rc_navar_ws_floats(c.N, c.H, c.two, c.B);
  if (a->ws_bytes < sizeof(float) * (size_t)c.wss * (size_t)c.nrep) {
    rc_set_error("navar_run: workspace of %zu bytes, %zu needed", a->ws_bytes, sizeof(float) * (size_t)c.wss * (size_t)c.nrep);
    return REDCLIFF_EWORKSPACE;
  }
  if (a->N == 0 || c.nrep == 0) return 0;
  c.nX = a->nX; c.nout = a->N; c.xps = a->x_pstride; c.pps = a->perm_pstride; c.fs = a->par_stride;
  c.X = a->X; c.perm = train ? a->perm : nullptr; c.par = a->par; c.pm = a->par_m; c.pv = a->par_v; c.hyp = a->hyper;
  c.ws = a->ws; c.mse = a->mse; c.l1 = a->l1; c.pred = a->pred; c.contrib = a->contrib;
  c.o = rc_navar_off(c.N, c.H, c.K, c.two);
  for (int64_t st = 0; st < nsteps; ++st) {
    const int64_t left = a->N - st * a->B;
    c.step = (int)st;
    c.Bi = left < a->B ? (int)left : a->B;
    c.t = a->tB + (int)st;
    c.q0 = (train ? 0 : a->row0) + st * a->B;
    c.out0 = st * a->B;
    e = train ? rc_launch_navar_step(c, (hipStream_t)stream) : rc_launch_navar_forward(c, (hipStream_t)stream);
    if (e) return e;
  }
  return 0;
}

}  // extern "C"
