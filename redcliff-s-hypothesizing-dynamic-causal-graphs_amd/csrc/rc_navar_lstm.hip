// rc_navar_lstm.hip -- the NAVAR (LSTM) additive baseline (models/navar.py:129-246): N per-source
// LSTM(1, H) networks over the T' steps of a window, a Linear(H, N) on every h_t, the N x N contributions
// summed over the sources into one prediction per time step.  A source's Whh is 4H x H (1 MB at
// H = 256), so a source cannot live in one workgroup, and every unit at step t needs all H units of step
// t - 1: that dependency is a LAUNCH BOUNDARY on the one stream.  A step is 2T' + 5 launches:
//
//   k_nl_fwd (t = 0 .. T'-1; unit slice s, source i, replica)  the workgroup owns 16 hidden units = 64
//        gate rows.  It stages its Whh rows once, forms the 64 pre-activations of each window from
//        h_{t-1} (workspace) on v_mfma_f32_16x16x4_f32 -- windows are M, gate rows N, k the H units
//        ascending; wave w owns 16 windows of the pass and all four gates of the slice, so a lane holds
//        i, f, g, o of its (window, unit) -- adds Wih x_t + (bih + bhh), applies the gates and writes
//        the gates, c_t and h_t of its units.  t = 0 reads no state.
//   k_nl_out   con_ij(t) = Wfc_i[j] . h_t + bfc_ij, one thread per (t, window, i, j).
//   k_nl_dc    the prediction (sources ascending, + biases), the residual at t = T'-1 and dcon.  With
//        lambda1 == 0 only t = T'-1 is formed in TRAIN by both.
//   k_nl_red   (TRAIN; one workgroup per replica) mse, l1, dbfc, dbiases.
//   k_nl_bwd (t = T'-1 .. 0; same ownership as k_nl_fwd)  dh_t of its units = Wfc^T dcon_t + the sum
//        over slices ascending of the previous launch's partials D, the gate gradients of its units
//        (written over the gates), the carry dc_t f_t, its partial D[s][b][v] = sum over its gate rows
//        of dgate . Whh[row][v] for all v (matrix cores, the same staged rows), and its rows of dWih,
//        dbih = dbhh and its columns of dWfc, accumulated in place over the launches (t descending).
//   dWhh       one GEMM per source (rc_gemm.h): M = 4H, N = H, k = (t, b) ascending over t >= 1.
//   k_nl_upd   element-wise Adam over the packed block.
//
// No workgroup waits on another, no atomics, no grid barrier; every value a launch reads was written by
// an earlier launch or by the reading workgroup itself.  Every sum runs in an order fixed by
// (N, H, T', batch size).
#include <cstring>

#include "rc_gemm.h"
#include "rc_navar_lstm.h"

namespace {

#define NL_PROLOGUE                                                                  \
  extern __shared__ float lds[];                                                     \
  const int s = blockIdx.x, i = blockIdx.y, ri = blockIdx.z, tid = threadIdx.x;      \
  const int r = c.rident ? ri : (int)c.rmap[ri];                                     \
  const int N = c.N, H = c.H, Tp = c.Tp, Hp = rc_navar_lstm_hp(H);                   \
  const int64_t B = c.B;                                                             \
  float* Pg = c.par + (int64_t)r * c.fs;                                             \
  const float* Xr = c.X + (int64_t)r * c.xps;                                        \
  const int32_t* permr = c.perm ? c.perm + (int64_t)r * c.pps : nullptr;             \
  float* wsr = c.ws + (int64_t)ri * c.w.total;                                       \
  const int lane = tid & 63, w = tid >> 6, l15 = lane & 15, kq = lane >> 4;          \
  (void)lane; (void)Tp

// Row of window b of the step / chunk (perm values clamped into the set).
__device__ inline int64_t nl_row(const NavarLstmCtx& c, const int32_t* permr, int b) {
  const int64_t q = c.q0 + b;
  int64_t row = permr ? (int64_t)permr[q] : q;
  return row < 0 ? 0 : (row >= c.nX ? c.nX - 1 : row);
}

// Ws[(q*16 + ul)][v] = Whh_i[q*H + 16 s + ul][v], zero past H in both directions.
__device__ inline void nl_stage_whh(float* Ws, const float* Whh, int H, int Hp, int s) {
  rc_stage<8>(64 * Hp,
              [&](int e) {
                const int row = e / Hp, v = e - row * Hp, q = row >> 4, u = s * NL_UL + (row & 15);
                return (u < H && v < H) ? Whh[((int64_t)q * H + u) * H + v] : 0.f;
              },
              [&](int e, float x) { Ws[e] = x; });
}

__global__ __launch_bounds__(RC_BLOCK) void k_nl_fwd(NavarLstmCtx c, int t) {
  NL_PROLOGUE;
  float* Ws = lds;
  if (t > 0) nl_stage_whh(Ws, Pg + c.o.Whh + (int64_t)i * 4 * H * H, H, Hp, s);
  __syncthreads();
  const int u = s * NL_UL + l15;
  const bool uok = u < H;
  float wih[4], bs[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t g = (int64_t)i * 4 * H + (int64_t)q * H + u;
    wih[q] = uok ? Pg[c.o.Wih + g] : 0.f;
    bs[q] = uok ? Pg[c.o.bih + g] + Pg[c.o.bhh + g] : 0.f;
  }
  float* Hs = wsr + c.w.Hs + (int64_t)i * Tp * B * H;
  float* Cs = wsr + c.w.Cs + (int64_t)i * Tp * B * H;
  float* Gs = wsr + c.w.Gs + (int64_t)i * Tp * B * 4 * H;
  const bool train = c.mode == REDCLIFF_NAVAR_TRAIN;
  for (int b0 = 0; b0 < c.Bi; b0 += NL_BC) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    if (t > 0) {
      int ba = b0 + 16 * w + l15;
      ba = ba < c.Bi ? ba : c.Bi - 1;
      const float* Ar = Hs + ((int64_t)(t - 1) * B + ba) * H;
      const float* Bq = Ws + l15 * Hp + kq;
      // k ascending in chunks of 64: a chunk's 16 operands of h_{t-1} are requested together
      for (int k0 = 0; k0 < H; k0 += 64) {
        float av[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) av[x] = k0 + 4 * x + kq < H ? Ar[k0 + 4 * x + kq] : 0.f;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
          const int kk = k0 + 4 * x;
          if (kk < H) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], Bq[kk], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], Bq[16 * Hp + kk], a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], Bq[32 * Hp + kk], a2, 0, 0, 0);
            a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], Bq[48 * Hp + kk], a3, 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int b = b0 + 16 * w + 4 * kq + reg;
      if (b < c.Bi && uok) {
        const float x = Xr[(nl_row(c, permr, b) * c.T + t) * N + i];
        const float ig = rc_sigmoid(a0[reg] + __builtin_fmaf(wih[0], x, bs[0]));
        const float fg = rc_sigmoid(a1[reg] + __builtin_fmaf(wih[1], x, bs[1]));
        const float gg = tanhf(a2[reg] + __builtin_fmaf(wih[2], x, bs[2]));
        const float og = rc_sigmoid(a3[reg] + __builtin_fmaf(wih[3], x, bs[3]));
        const int64_t at = ((int64_t)t * B + b) * H + u;
        const float cp = t > 0 ? Cs[at - B * H] : 0.f;
        const float cn = __builtin_fmaf(fg, cp, ig * gg);
        Cs[at] = cn;
        Hs[at] = og * tanhf(cn);
        if (train) {
          float* g = Gs + ((int64_t)t * B + b) * 4 * H + u;
          g[0] = ig; g[H] = fg; g[2 * (int64_t)H] = gg; g[3 * (int64_t)H] = og;
        }
      }
    }
  }
}

// One thread per (selected time step, window, source i, target j): con_ij(t) into Con (TRAIN) or
// contrib (FORWARD).
__global__ __launch_bounds__(RC_BLOCK) void k_nl_out(NavarLstmCtx c) {
  const int ri = blockIdx.y, r = c.rident ? ri : (int)c.rmap[ri];
  const int N = c.N, H = c.H, Tp = c.Tp, NN = N * N;
  const int64_t B = c.B;
  const bool train = c.mode == REDCLIFF_NAVAR_TRAIN;
  const int64_t e = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
  if (e >= (int64_t)Tp * c.Bi * NN) return;
  const int ij = (int)(e % NN), i = ij / N;
  const int64_t tb = e / NN;
  const int b = (int)(tb % c.Bi), t = Tp - 1 - (int)(tb / c.Bi);  // the last time step first
  if (train && c.hyp[r].c_adj == 0.f && t != Tp - 1) return;
  const float* Pg = c.par + (int64_t)r * c.fs;
  float* wsr = c.ws + (int64_t)ri * c.w.total;
  const float* h = wsr + c.w.Hs + (((int64_t)i * Tp + t) * B + b) * H;
  const float* wf = Pg + c.o.Wfc + (int64_t)ij * H;
  float acc = Pg[c.o.bfc + ij];
  for (int u = 0; u < H; ++u) acc = __builtin_fmaf(wf[u], h[u], acc);
  float* con = train ? wsr + c.w.Con + ((int64_t)t * B + b) * NN
                     : c.contrib + (((int64_t)ri * c.nout + c.out0 + b) * Tp + t) * NN;
  con[ij] = acc;
}

// One thread per (selected time step, window, target j): the prediction (sources ascending, + biases);
// TRAIN: Res and DC of the workspace; FORWARD: pred.
__global__ __launch_bounds__(RC_BLOCK) void k_nl_dc(NavarLstmCtx c) {
  const int ri = blockIdx.y, r = c.rident ? ri : (int)c.rmap[ri];
  const int N = c.N, Tp = c.Tp, NN = N * N;
  const int64_t B = c.B;
  const bool train = c.mode == REDCLIFF_NAVAR_TRAIN;
  const float lam = train ? c.hyp[r].c_adj : 0.f;
  const int64_t e = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
  if (e >= (int64_t)Tp * c.Bi * N) return;
  const int j = (int)(e % N);
  const int64_t tb = e / N;
  const int b = (int)(tb % c.Bi), t = Tp - 1 - (int)(tb / c.Bi);
  if (train && lam == 0.f && t != Tp - 1) return;
  const float* Pg = c.par + (int64_t)r * c.fs;
  float* wsr = c.ws + (int64_t)ri * c.w.total;
  const float* con = train ? wsr + c.w.Con + ((int64_t)t * B + b) * NN
                           : c.contrib + (((int64_t)ri * c.nout + c.out0 + b) * Tp + t) * NN;
  float pred = con[j];
  for (int i = 1; i < N; ++i) pred += con[(int64_t)i * N + j];
  pred += Pg[c.o.bias + j];
  if (!train) {
    c.pred[(((int64_t)ri * c.nout + c.out0 + b) * N + j) * Tp + t] = pred;
    return;
  }
  float dp = 0.f;
  if (t == Tp - 1) {
    const float* Xr = c.X + (int64_t)r * c.xps;
    const int32_t* permr = c.perm + (int64_t)r * c.pps;
    const float res = pred - Xr[(nl_row(c, permr, b) * c.T + Tp) * N + j];
    wsr[c.w.Res + (int64_t)b * N + j] = res;
    dp = (2.f / (float)(c.Bi * N)) * res;
  }
  const float lamc = (lam / (float)N) / (float)(c.Bi * Tp);
  float* dc = wsr + c.w.DC + ((int64_t)t * B + b) * NN;
  for (int i = 0; i < N; ++i) dc[(int64_t)i * N + j] = __builtin_fmaf(lamc, rc_sign(con[(int64_t)i * N + j]), dp);
}

// TRAIN, one workgroup per replica: the step's mse and l1, dbfc and dbiases (into the gradient block).
__global__ __launch_bounds__(RC_BLOCK) void k_nl_red(NavarLstmCtx c) {
  __shared__ float red[16];
  const int ri = blockIdx.x, r = c.rident ? ri : (int)c.rmap[ri], tid = threadIdx.x;
  const int N = c.N, Tp = c.Tp, NN = N * N;
  const int64_t B = c.B;
  const float lam = c.hyp[r].c_adj;
  float* wsr = c.ws + (int64_t)ri * c.w.total;
  const float* Res = wsr + c.w.Res;
  const float* Con = wsr + c.w.Con;
  const float* DC = wsr + c.w.DC;
  float* G = wsr + c.w.G;
  const int t0 = lam == 0.f ? Tp - 1 : 0;
  float sq = 0.f, ab = 0.f;
  for (int e = tid; e < c.Bi * N; e += RC_BLOCK) sq = __builtin_fmaf(Res[e], Res[e], sq);
  for (int t = t0; t < Tp; ++t)
    for (int e = tid; e < c.Bi * NN; e += RC_BLOCK) ab += fabsf(Con[(int64_t)t * B * NN + e]);
  const float sqs = rc_block_sum(sq, red);
  const float abs_ = rc_block_sum(ab, red);
  if (tid == 0) {
    const int64_t o = (int64_t)ri * c.nsteps + c.step;
    c.mse[o] = sqs / (float)(c.Bi * N);
    c.l1[o] = (lam / (float)N) * (abs_ / (float)(c.Bi * Tp));
  }
  for (int e = tid; e < NN; e += RC_BLOCK) {
    float acc = 0.f;
    for (int t = t0; t < Tp; ++t) {
      const float* d = DC + (int64_t)t * B * NN + e;
      int b = 0;
      for (; b + 8 <= c.Bi; b += 8) {  // eight loads in flight, added in window order
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = d[(int64_t)(b + q) * NN];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += v[q];
      }
      for (; b < c.Bi; ++b) acc += d[(int64_t)b * NN];
    }
    G[c.o.bfc + e] = acc;
  }
  if (tid < N) {
    const float sc = 2.f / (float)(c.Bi * N);
    float acc = 0.f;
    for (int b = 0; b < c.Bi; ++b) acc += sc * Res[(int64_t)b * N + tid];
    G[c.o.bias + tid] = acc;
  }
}

__global__ __launch_bounds__(RC_BLOCK) void k_nl_bwd(NavarLstmCtx c, int t) {
  NL_PROLOGUE;
  const int nS = rc_navar_lstm_slices(H), Np = N | 1, NN = N * N;
  const bool last = t == Tp - 1;
  const bool hasdc = last || c.hyp[r].c_adj != 0.f;
  float* Ws = lds;
  float* dg = Ws + 64 * Hp;
  float* dcs = dg + 64 * 65;
  float* hs = dcs + 64 * Np;
  float* Wf = hs + 64 * 17;
  float* gWf = Wf + N * 17;
  float* xs = gWf + N * 17;
  float* gb = xs + 64;
  float* gWi = gb + 64;
  if (t > 0) nl_stage_whh(Ws, Pg + c.o.Whh + (int64_t)i * 4 * H * H, H, Hp, s);
  const float* Wfc = Pg + c.o.Wfc + (int64_t)i * N * H;
  for (int e = tid; e < N * 17; e += RC_BLOCK) {
    const int j = e / 17, ul = e - j * 17, u = s * NL_UL + ul;
    Wf[e] = (ul < NL_UL && u < H) ? Wfc[(int64_t)j * H + u] : 0.f;
    gWf[e] = 0.f;
  }
  if (tid < 64) { gb[tid] = 0.f; gWi[tid] = 0.f; }
  const float* Hs = wsr + c.w.Hs + (int64_t)i * Tp * B * H;
  const float* Cs = wsr + c.w.Cs + (int64_t)i * Tp * B * H;
  float* Gs = wsr + c.w.Gs + (int64_t)i * Tp * B * 4 * H;
  float* carry = wsr + c.w.carry + (int64_t)i * B * H;
  const float* DC = wsr + c.w.DC;
  const int64_t dbuf = (int64_t)N * nS * B * H;
  const float* Dr = wsr + c.w.D + (int64_t)((t + 1) & 1) * dbuf + (int64_t)i * nS * B * H;
  float* Dw = wsr + c.w.D + (int64_t)(t & 1) * dbuf + ((int64_t)i * nS + s) * B * H;
  const int nvt = (H + 15) >> 4;
  for (int b0 = 0; b0 < c.Bi; b0 += NL_BC) {
    const int nbc = c.Bi - b0 < NL_BC ? c.Bi - b0 : NL_BC;
    __syncthreads();
    if (tid < 64) xs[tid] = tid < nbc ? Xr[(nl_row(c, permr, b0 + tid) * c.T + t) * N + i] : 0.f;
    if (hasdc) {
      for (int e = tid; e < 64 * N; e += RC_BLOCK) {
        const int b = e / N, j = e - b * N;
        dcs[b * Np + j] = b < nbc ? DC[((int64_t)t * B + b0 + b) * NN + (int64_t)i * N + j] : 0.f;
      }
      for (int e = tid; e < 64 * NL_UL; e += RC_BLOCK) {
        const int b = e >> 4, ul = e & 15, u = s * NL_UL + ul;
        hs[b * 17 + ul] = (b < nbc && u < H) ? Hs[((int64_t)t * B + b0 + b) * H + u] : 0.f;
      }
    }
    __syncthreads();
    // 1. dh of the slice's units, the gate gradients, the carry
    for (int e = tid; e < 64 * NL_UL; e += RC_BLOCK) {
      const int b = e >> 4, ul = e & 15, u = s * NL_UL + ul;
      float di = 0.f, df = 0.f, dgg = 0.f, dov = 0.f;
      if (b < nbc && u < H) {
        float dh = 0.f;
        if (hasdc)
          for (int j = 0; j < N; ++j) dh = __builtin_fmaf(dcs[b * Np + j], Wf[j * 17 + ul], dh);
        if (!last) {
          const float* dp = Dr + (int64_t)(b0 + b) * H + u;
          float a = dp[0];
          for (int s2 = 1; s2 < nS; ++s2) a += dp[(int64_t)s2 * B * H];
          dh += a;
        }
        const int64_t at = ((int64_t)t * B + b0 + b) * H + u;
        float* g = Gs + ((int64_t)t * B + b0 + b) * 4 * H + u;
        const float ig = g[0], fg = g[H], gg = g[2 * (int64_t)H], og = g[3 * (int64_t)H];
        const float cp = t > 0 ? Cs[at - B * H] : 0.f;
        const float tc = tanhf(Cs[at]);
        float dct = dh * og * (1.f - tc * tc);
        if (!last) dct += carry[(int64_t)(b0 + b) * H + u];
        carry[(int64_t)(b0 + b) * H + u] = dct * fg;
        di = dct * gg * ig * (1.f - ig);
        df = dct * cp * fg * (1.f - fg);
        dgg = dct * ig * (1.f - gg * gg);
        dov = dh * tc * og * (1.f - og);
        g[0] = di; g[H] = df; g[2 * (int64_t)H] = dgg; g[3 * (int64_t)H] = dov;
      }
      dg[b * 65 + ul] = di;
      dg[b * 65 + 16 + ul] = df;
      dg[b * 65 + 32 + ul] = dgg;
      dg[b * 65 + 48 + ul] = dov;
    }
    __syncthreads();
    // 2. the slice's partial of dh_{t-1}: D[b][v] = sum over its 64 gate rows of dgate[b][row] Whh[row][v]
    if (t > 0) {
      const float* Ad = dg + (16 * w + l15) * 65 + kq;
      for (int nt = 0; nt < nvt; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* Bw = Ws + kq * Hp + nt * 16 + l15;
#pragma unroll
        for (int kk = 0; kk < 64; kk += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ad[kk], Bw[kk * Hp], acc, 0, 0, 0);
        const int v = nt * 16 + l15;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int b = 16 * w + 4 * kq + reg;
          if (b < nbc && v < H) Dw[(int64_t)(b0 + b) * H + v] = acc[reg];
        }
      }
    }
    // 3. the slice's rows of dbih (= dbhh), dWih and its columns of dWfc, windows ascending
    if (tid < 64) {
      float ab_ = gb[tid], aw = gWi[tid];
      for (int b = 0; b < nbc; ++b) {
        const float d = dg[b * 65 + tid];
        ab_ += d;
        aw = __builtin_fmaf(d, xs[b], aw);
      }
      gb[tid] = ab_;
      gWi[tid] = aw;
    } else if (hasdc) {
      for (int e = tid - 64; e < N * NL_UL; e += RC_BLOCK - 64) {
        const int j = e >> 4, ul = e & 15;
        float acc = gWf[j * 17 + ul];
        for (int b = 0; b < nbc; ++b) acc = __builtin_fmaf(dcs[b * Np + j], hs[b * 17 + ul], acc);
        gWf[j * 17 + ul] = acc;
      }
    }
  }
  __syncthreads();
  // the launch's sums join the gradient block (the last time step starts it): t descending
  float* G = wsr + c.w.G;
  if (tid < 64) {
    const int q = tid >> 4, u = s * NL_UL + (tid & 15);
    if (u < H) {
      const int64_t g = (int64_t)i * 4 * H + (int64_t)q * H + u;
      const float vb = last ? gb[tid] : G[c.o.bih + g] + gb[tid];
      const float vw = last ? gWi[tid] : G[c.o.Wih + g] + gWi[tid];
      G[c.o.bih + g] = vb;
      G[c.o.bhh + g] = vb;
      G[c.o.Wih + g] = vw;
    }
  } else if (hasdc) {
    for (int e = tid - 64; e < N * NL_UL; e += RC_BLOCK - 64) {
      const int j = e >> 4, ul = e & 15, u = s * NL_UL + ul;
      if (u < H) {
        const int64_t g = c.o.Wfc + ((int64_t)i * N + j) * H + u;
        G[g] = last ? gWf[j * 17 + ul] : G[g] + gWf[j * 17 + ul];
      }
    }
  }
}

// Element-wise Adam over the packed block from the gradient block (dWhh is exactly 0 when T' = 1).
__global__ __launch_bounds__(RC_BLOCK) void k_nl_upd(NavarLstmCtx c) {
  __shared__ RcAdamScalars as_;
  const int ri = blockIdx.y, r = c.rident ? ri : (int)c.rmap[ri];
  if (threadIdx.x == 0) as_ = rc_adam_scalars(c.hyp[r].B, c.at);
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
  if (e >= c.o.total) return;
  const RcAdamScalars as = as_;
  const float* G = c.ws + (int64_t)ri * c.w.total + c.w.G;
  const float g = (c.Tp == 1 && e >= c.o.Whh && e < c.o.bih) ? 0.f : G[e];
  float* P = c.par + (int64_t)r * c.fs;
  float* M = c.pm + (int64_t)r * c.fs;
  float* V = c.pv + (int64_t)r * c.fs;
  float pp = P[e], mm = M[e], vv = V[e];
  rc_adam(pp, mm, vv, g, as);
  P[e] = pp; M[e] = mm; V[e] = vv;
}

// SLOT: one opt-in record per kernel (k_nl_fwd and k_nl_bwd have the same type)
template <int SLOT, class Kern, class... A>
int nl_launch(Kern k, const char* what, dim3 grid, size_t bytes, hipStream_t s, A... args) {
  // the LDS opt-in is a host call of its own: once per kernel, device and size, not once per launch
  static size_t opted[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
  if (dev < 0 || bytes > opted[dev]) {
    const int e = rc_lds_optin(k, bytes, what);
    if (e) return e;
    if (dev >= 0) opted[dev] = bytes;
  }
  hipLaunchKernelGGL(k, grid, dim3(RC_BLOCK), bytes, s, args...);
  return rc_check(hipGetLastError(), what);
}

size_t nl_lds_bytes(const NavarLstmCtx& c) {
  return sizeof(float) * (size_t)rc_navar_lstm_lds_floats(c.N, c.H, c.Tp, 1, 1);
}

int nl_forward_launches(const NavarLstmCtx& c, hipStream_t s) {
  const dim3 grid(rc_navar_lstm_slices(c.H), c.N, c.nrep);
  const size_t bytes = sizeof(float) * 64 * (size_t)rc_navar_lstm_hp(c.H);
  for (int t = 0; t < c.Tp; ++t) {
    const int e = nl_launch<0>(k_nl_fwd, "k_nl_fwd", grid, bytes, s, c, t);
    if (e) return e;
  }
  return 0;
}

int nl_out_launch(const NavarLstmCtx& c, hipStream_t s) {
  const int64_t th = (int64_t)c.Tp * c.Bi * c.N;
  hipLaunchKernelGGL(k_nl_out, dim3((unsigned)((th * c.N + RC_BLOCK - 1) / RC_BLOCK), c.nrep), dim3(RC_BLOCK), 0, s, c);
  const int e = rc_check(hipGetLastError(), "k_nl_out");
  if (e) return e;
  hipLaunchKernelGGL(k_nl_dc, dim3((unsigned)((th + RC_BLOCK - 1) / RC_BLOCK), c.nrep), dim3(RC_BLOCK), 0, s, c);
  return rc_check(hipGetLastError(), "k_nl_dc");
}

}  // namespace

int rc_launch_navar_lstm_step(const NavarLstmCtx& c, hipStream_t s) {
  const int mask = c.launches ? c.launches : 15;
  const dim3 grid(rc_navar_lstm_slices(c.H), c.N, c.nrep);
  int e = 0;
  if ((mask & 1) && (e = nl_forward_launches(c, s))) return e;
  if (mask & 2) {
    if ((e = nl_out_launch(c, s))) return e;
    hipLaunchKernelGGL(k_nl_red, dim3(c.nrep), dim3(RC_BLOCK), 0, s, c);
    if ((e = rc_check(hipGetLastError(), "k_nl_red"))) return e;
  }
  if (mask & 4) {
    const size_t bytes = nl_lds_bytes(c);
    for (int t = c.Tp - 1; t >= 0; --t)
      if ((e = nl_launch<1>(k_nl_bwd, "k_nl_bwd", grid, bytes, s, c, t))) return e;
  }
  if (mask & 8) {
    if (c.Tp > 1) {
      // dWhh_i[g][v] = sum over t = 1 .. T'-1, b < Bi (ascending) of dgate_i[t][b][g] h_i[t-1][b][v]
      const int H = c.H, G4 = 4 * c.H;
      const int64_t B = c.B;
      RcGemm g = rc_gemm_args(1, 0, G4, H, (c.Tp - 1) * c.Bi, c.ws + c.w.Gs + B * G4, G4, (int64_t)c.Tp * B * G4,
                              c.ws + c.w.Hs, H, (int64_t)c.Tp * B * H, c.ws + c.w.G + c.o.Whh, H, (int64_t)G4 * H);
      g.Kblk = c.Bi; g.rA = B * G4; g.rB = B * H;
      g.nrep = c.nrep; g.rident = 1;  // the workspace slices are indexed by the stepped replica
      g.qA = g.qB = g.qC = c.w.total;
      if ((e = rc_gemm_launch(g, c.N, s, "navar_lstm dWhh"))) return e;
    }
    hipLaunchKernelGGL(k_nl_upd, dim3((unsigned)((c.o.total + RC_BLOCK - 1) / RC_BLOCK), c.nrep), dim3(RC_BLOCK), 0, s, c);
    e = rc_check(hipGetLastError(), "k_nl_upd");
  }
  return e;
}

int rc_launch_navar_lstm_forward(const NavarLstmCtx& c, hipStream_t s) {
  const int e = nl_forward_launches(c, s);
  return e ? e : nl_out_launch(c, s);
}

extern "C" {

static int navar_lstm_dims(const RedcliffDims* d) {
  if (!d) { rc_set_error("null dims"); return REDCLIFF_EINVAL; }
  if (d->R < 1 || d->Bmax < 1 || d->T < 2 || d->p < 1 || d->h < 1) {
    rc_set_error("invalid dims (R=%d Bmax=%d T=%d p=%d h=%d)", d->R, d->Bmax, d->T, d->p, d->h);
    return REDCLIFF_EINVAL;
  }
  if (rc_navar_lstm_lds_floats(d->p, d->h, d->T - 1, d->Bmax, d->R) == 0) {
    rc_set_error("dims outside kernel limits (navar_lstm: N<=32 H<=448 T'=T-1<=64 Bmax<=512 R<=%d, LDS 64*(ceil16(H)|1) + "
                 "4160 + 64*(N|1) + 1088 + 34*N + 384 <= %d floats; N=%d H=%d T=%d Bmax=%d R=%d)", RC_MAX_ACTIVE,
                 RC_LDS_MAX_FLOATS, d->p, d->h, d->T, d->Bmax, d->R);
    return REDCLIFF_ELIMIT;
  }
  return 0;
}

int redcliff_navar_lstm_supported(const RedcliffDims* d) {
  if (navar_lstm_dims(d) != 0) return 0;
  return (int)rc_navar_lstm_lds_floats(d->p, d->h, d->T - 1, d->Bmax, d->R);
}

int64_t redcliff_navar_lstm_ws_floats(const RedcliffDims* d, int32_t B, int32_t train) {
  if (navar_lstm_dims(d) != 0 || B < 1) return 0;
  return rc_navar_lstm_ws(d->p, d->h, d->T - 1, B, train ? 1 : 0).total;
}

int redcliff_navar_lstm_run(const RedcliffNavarLstmArgs* a, void* stream) {
  if (!a) { rc_set_error("null navar_lstm arguments"); return REDCLIFF_EINVAL; }
  int e = navar_lstm_dims(&a->d);
  if (e) return e;
  const RedcliffDims& d = a->d;
  const bool train = a->mode == REDCLIFF_NAVAR_TRAIN;
  if (!train && a->mode != REDCLIFF_NAVAR_FORWARD) { rc_set_error("navar_lstm_run: bad mode %d", a->mode); return REDCLIFF_EINVAL; }
  if (!a->X || !a->par || !a->ws ||
      (train ? (!a->perm || !a->par_m || !a->par_v || !a->hyper || !a->mse || !a->l1) : (!a->pred || !a->contrib))) {
    rc_set_error("navar_lstm_run: null buffer in arguments");
    return REDCLIFF_EINVAL;
  }
  if (a->launches < 0 || a->launches > 15) { rc_set_error("navar_lstm_run: bad launch mask %d", a->launches); return REDCLIFF_EINVAL; }
  if (a->B < 1 || a->B > d.Bmax || a->N < 0 || a->nX < 1 || (train && a->tB < 1) ||
      (!train && (a->row0 < 0 || a->row0 + a->N > a->nX)) || a->nX > INT32_MAX) {
    rc_set_error("navar_lstm_run: bad arguments (B=%d (1..Bmax=%d) N=%lld row0=%lld nX=%lld tB=%d)", a->B, d.Bmax,
                 (long long)a->N, (long long)a->row0, (long long)a->nX, a->tB);
    return REDCLIFF_EINVAL;
  }
  if (a->x_pstride < 0 || a->perm_pstride < 0 || a->par_stride < 0) {
    rc_set_error("navar_lstm_run: negative replica stride");
    return REDCLIFF_EINVAL;
  }
  const int64_t nsteps = (a->N + a->B - 1) / a->B;
  if (nsteps > INT32_MAX / 2) { rc_set_error("navar_lstm_run: too many steps"); return REDCLIFF_ELIMIT; }
  NavarLstmCtx c;
  memset(&c, 0, sizeof(c));
  if (a->replicas) {  // the rules of RedcliffStepArgs.replicas
    if (a->n_replicas < 0 || a->n_replicas > d.R) {
      rc_set_error("navar_lstm_run: active replica list of %d entries (at most R=%d)", a->n_replicas, d.R);
      return REDCLIFF_EINVAL;
    }
    for (int i = 0; i < a->n_replicas; ++i) {
      const int r = a->replicas[i];
      if (r < 0 || r >= d.R || (i > 0 && r <= a->replicas[i - 1])) {
        rc_set_error("navar_lstm_run: active replica list must be strictly increasing indices < R=%d (entry %d = %d)", d.R, i, r);
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
  c.N = d.p; c.H = d.h; c.T = d.T; c.Tp = d.T - 1; c.B = a->B; c.mode = a->mode; c.nsteps = (int)nsteps; c.launches = a->launches;
  c.w = rc_navar_lstm_ws(c.N, c.H, c.Tp, c.B, train ? 1 : 0);
  if (a->ws_bytes < sizeof(float) * (size_t)c.w.total * (size_t)c.nrep) {
    rc_set_error("navar_lstm_run: workspace of %zu bytes, %zu needed", a->ws_bytes, sizeof(float) * (size_t)c.w.total * (size_t)c.nrep);
    return REDCLIFF_EWORKSPACE;
  }
  if (a->N == 0 || c.nrep == 0) return 0;
  c.nX = a->nX; c.nout = a->N; c.xps = a->x_pstride; c.pps = a->perm_pstride; c.fs = a->par_stride;
  c.X = a->X; c.perm = train ? a->perm : nullptr; c.par = a->par; c.pm = a->par_m; c.pv = a->par_v; c.hyp = a->hyper;
  c.ws = a->ws; c.mse = a->mse; c.l1 = a->l1; c.pred = a->pred; c.contrib = a->contrib;
  c.o = rc_navar_lstm_off(c.N, c.H);
  for (int64_t st = 0; st < nsteps; ++st) {
    const int64_t left = a->N - st * a->B;
    c.step = (int)st;
    c.Bi = left < a->B ? (int)left : a->B;
    c.at = a->tB + (int)st;
    c.q0 = (train ? 0 : a->row0) + st * a->B;
    c.out0 = st * a->B;
    e = train ? rc_launch_navar_lstm_step(c, (hipStream_t)stream) : rc_launch_navar_lstm_forward(c, (hipStream_t)stream);
    if (e) return e;
  }
  return 0;
}

}  // extern "C"
