// rc_forward.hip -- forward half of the fused REDCLIFF-S step on gfx950: the DGCNN embedder
// and (vector path) the K x p factor networks, as ONE launch.
//
// The two forwards depend only on the window X and the parameters, so their workgroups share
// a grid: blocks [0, nemb) run the embedder on SB windows each, blocks [nemb, nemb + nfac) run
// one (factor, channel network, 16-unit hidden chunk) each.  One launch instead of two removes
// a kernel boundary and overlaps the two latency chains (at D4IC both are single waves of
// workgroups whose time is their own dependent global round trips).  Every workgroup issues
// all of its global loads in one multi-segment staging pass before computing.
//
// Reference: models/redcliff_factor_score_embedders.py:335-392 + models/dgcnn.py:15-64 +
// torcheeg 1.1.3 DGCNN (restated in oracle/torcheeg_dgcnn.py):
//   x_bn = BN1(x); L = D^-1/2 relu(A) D^-1/2; Z = sum_i (S_i x_bn) W_i; w = fc2(relu(fc1(vec(relu(Z)))))
// and models/cmlp.py:12-35 / :90-101 (MLP: Conv1d(p, h, L) -> ReLU -> Conv1d(h, 1, 1)),
// models/cmlp.py:147-167 (group norms of layer-0 weights, pre-update).
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "rc_common.h"

namespace {

#define FK_BT 128  // windows per factor-forward tile (16 row groups x 8)
#define FQ_MAX 96  // layer-0 contraction staged in one pass up to this length
#define RC_EMB_TEAM_NT 512  // the wave-team workgroup: two teams of four waves (emb_fwd_body)
#ifndef FF_KB
#define FF_KB 4  // k-steps per operand batch of the factor forward's chains (rc_fac_bwd.h's FB_KB)
#endif

__device__ inline int fq_tile(const RedcliffDims& d) { return d.p * d.L <= FQ_MAX ? d.p * d.L : 32; }

// ------------------------------------------------------------------------------------------
// Embedder forward of windows [bx*SB, bx*SB + SB).
//
// fc1 runs over channel slices of cs channels (columns [z*cs*H, min(p, (z+1)*cs)*H) of the p*H
// contraction, Zs = ceil(p / cs) slices): every slice's 64 lane chains are reduced on their own and
// f1 = ((part_0 + part_1) + ...) + fc1b, so the bits depend on cs only, never on how the slices are
// spread over workgroups.  zs < 0: this workgroup runs every slice of its windows.  zs >= 0 (one
// window per workgroup, the single fit): it runs slice zs only -- the Chebyshev rows, graph
// convolution and fc1 columns of its channels -- stores its fc1 partials write-through and counts
// itself in on the window's arrival counter; the workgroup that arrives last sums the partials in
// slice order and runs fc2.  No workgroup waits for another.
// NT = RC_EMB_TEAM_NT (512 threads, one window, Zs <= 2, zs < 0): wave team t (waves 4t .. 4t+3) runs
// slice t's fc1 with the lane chains of a 256-thread workgroup's four waves, the row-holding lanes
// leave the slice sums in LDS and f1 = (part_0 + part_1) + fc1b after one barrier -- the order of
// both other paths, without the store / drain / counter / reload exchange between workgroups.
// Memory round trips on a workgroup's path: the staging pass (the BatchNorm statistics among its
// loads), then the fc1 weights of the wave's first three column steps, requested when the staging
// data has landed and in flight under BatchNorm, the Chebyshev rows and the graph convolution --
// which read and write LDS only: the workspace copies of T and R are stored after the products.
template <int NBT, int NT>
__device__ __attribute__((always_inline)) void emb_fwd_body(const StepCtx& c, int bx, int SB, int w_lds, int cs, int zs, float* sm) {
  constexpr bool TEAM = NT == RC_EMB_TEAM_NT;
  constexpr int UD = NT / RC_BLOCK;  // staging loads per thread shrink with the block
  const RedcliffDims& d = c.d;
  const int r = rc_rep(c, blockIdx.y);
  const int b0 = bx * SB;
  const int nb = min(SB, c.B - b0);
  if (nb <= 0) return;
  const int Zs = cs == (int)c.mg[RC_MG_CS] ? c.fzs : (d.p + cs - 1) / cs;
  const int zlo = zs < 0 ? 0 : zs, zhi = zs < 0 ? Zs : zs + 1;
  const int ch0 = zlo * cs, ch1 = min(d.p, zhi * cs);  // channels whose T / R rows this workgroup forms
  RC_WG_MARK(c.ws, c.wo.total, RC_KID_EMB_FWD, 0);
  RC_PHASE(c.ws, c.wo.total, bx, 0);
  const int p = d.p, F = d.F, H = d.H, n = d.n, M1 = d.M1, K = d.K;
  const int pF = p * F, pH = p * H, nFH = n * F * H;
  const RcDiv32 dF(F, c.mg[RC_MG_F]), dp(p, c.mg[RC_MG_P]), dpF(pF, c.mg[RC_MG_PF]), dH(H, c.mg[RC_MG_H]);
  const float* E = c.emb + r * c.es;
  float* ws = c.ws + r * c.wss;
  const float* X = c.X + r * c.xr;
  const int tid = threadIdx.x;

  float* xs = sm;                      // [SB][p][F]   raw window, then x_bn
  float* Sl = xs + SB * pF;            // [n][p][p]
  float* Wl = Sl + n * p * p;          // [n][F][H]    (w_lds)
  float* Tl = Wl + (w_lds ? nFH : 0);  // [SB][n][p][F]
  float* Rl = Tl + SB * n * pF;        // [SB][p*H]
  float* f1l = Rl + SB * pH;           // [SB][M1]
  float* fc2s = f1l + SB * M1;         // [K][M1]
  float* fb1 = fc2s + K * M1;          // [M1]
  float* fb2 = fb1 + M1;               // [K]
  float* alpha = fb2 + K;              // [F]
  float* beta = alpha + F;             // [F]
  float* partl = beta + F;             // [2][M1]      wave teams' fc1 slice sums (TEAM)

  if (blockIdx.x == 0) {  // arrival counters of the embedder backward (they also self-reset)
    unsigned* cnt = reinterpret_cast<unsigned*>(ws + c.wo.ecnt);
    for (int e = tid; e < p * rc_nchunk(d); e += NT) cnt[e] = 0u;
  }
  // BatchNorm statistics (torch forms the scale in double in train mode): the loads only, as the
  // first segment of the staging pass.  Their conversions and the scale follow the pass behind
  // rc_keep(); a conversion folded into the load's block waits for the load there, a round trip of
  // its own in front of the staging loads.
  RC_PHASE(c.ws, c.wo.total, bx, 1);
  const bool train = c.flags & RC_BN_TRAIN;
  double st_mean = 0.0, st_var = 0.0;  // train: the batch statistics
  float rn_mean = 0.f, rn_var = 0.f;   // evaluation: the running ones
  float bw = 0.f, bb = 0.f;
  double bn_eps = 0.0;
  const float* S = ws + c.wo.S;
  const float* gw = E + c.eo.gcW;
  // Loads per thread per segment sized so that the common shapes stage in ONE round (a second
  // round is another memory latency on every workgroup's path): n p^2 <= 512 (C1(K=4) 300, TST 432),
  // n F H <= 5,120 (4,800), K M1 <= 1,024 (TST 576)
  rc_stage_all_closed(
      rc_seg_once([&]() {
        if (tid < F) {
          if (train) {
            st_mean = c.bns[r * c.bnsr + tid];
            st_var = c.bns[r * c.bnsr + F + tid];
          } else {
            rn_mean = c.rm[r * F + tid];
            rn_var = c.rv[r * F + tid];
          }
          bw = E[c.eo.bnw + tid];
          bb = E[c.eo.bnb + tid];
          bn_eps = c.hyp[r].bn_eps;  // (a load too: issued here, not in front of the scale)
        }
      }),
      rc_seg<2 / UD, NT>(n * p * p, [&](int e) { return S[e]; }, [&](int e, float v) { Sl[e] = v; }),
      rc_seg<20 / UD, NT>(w_lds ? nFH : 0, [&](int e) { return gw[e]; }, [&](int e, float v) { Wl[e] = v; }),
      // window rows are contiguous in the channel index: read (s, f, ch), store [s][ch][f]
      rc_seg<4 / UD, NT>(nb * pF, [&](int e) {
        const int s = dpF.div(e), rem = e - s * pF;
        return X[(c.row0 + b0 + s) * d.T * p + (int64_t)(c.Lmax - F) * p + rem];
      }, [&](int e, float v) {
        const int s = dpF.div(e), rem = e - s * pF, f = dp.div(rem), ch = rem - f * p;
        xs[s * pF + ch * F + f] = v;
      }),
      rc_seg<4 / UD, NT>(K * M1, [&](int e) { return E[c.eo.fc2W + e]; }, [&](int e, float v) { fc2s[e] = v; }),
      rc_seg<1, NT>(M1 + K, [&](int e) { return e < M1 ? E[c.eo.fc1b + e] : E[c.eo.fc2b + e - M1]; },
                [&](int e, float v) { fb1[e] = v; }));  // fb2 follows fb1
  RC_PHASE(c.ws, c.wo.total, bx, 2);
  // fc1 weights: the first three column steps of this wave's first slice, those the slice has, are
  // requested here -- after the staging loads have landed (a request among them is drained with them:
  // the staging waits are full waits and loads return in order) and ahead of BatchNorm, the Chebyshev
  // rows and the graph convolution, none of which touches global memory (w_lds), so the weights
  // arrive while they run and nothing waits for them before the first fc1 product.
  const float* W1 = E + c.eo.fc1W;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;  // (the wave of its team)
  const int team = TEAM ? __builtin_amdgcn_readfirstlane(tid >> 8) : 0;
  const int fz0 = TEAM ? min(team, Zs) : zlo, fz1 = TEAM ? min(team + 1, Zs) : zhi;  // this wave's fc1 slices
  const int RW = (M1 + 3) / 4, m0 = wv * RW;
  // Three buffers of column-step weights in rotation (p*H = 1,000 - 1,200 at C1 / TST is 16 - 19
  // column steps in slices of four): a buffer is refilled right after it is multiplied, when the
  // slice has the column step it would hold, and read three steps later.  No load is issued for a
  // column step the slice does not have: a wait in front of a product would include it.  (Where a
  // path with a refill meets one without, the compiler copies the buffer between registers and the
  // copy waits for the refill; slices of up to three steps, D4IC's, refill nothing, and the fourth
  // step of a 200-column slice is waited for one product later than it is requested: DESIGN 8.)
  // Rows past M1 load row M1 - 1 (their sums are never stored) and a lane past the slice's end a
  // clamped (valid) column that it multiplies by zero, so no load sits behind a condition of its own.
  auto qend = [&](int z) { return min(p, (z + 1) * cs) * H; };  // fc1 columns of slice z: [z*cs*H, qend(z))
  int qb = qend(fz0);
  auto ldw = [&](float (&w)[16], int qn) {
    const int qc = qn < qb ? qn : qb - 1;
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = W1[(int64_t)min(m0 + j, M1 - 1) * pH + qc];
  };
  float wb0[16], wb1[16], wb2[16];
  // Every earlier load has landed on every path here, and the compiler is told so: where paths with
  // different loads in flight meet (a wave with no slice issues none), its wait in front of a later
  // use of a statistics register would otherwise be counted for the path without the request and
  // drain the request on the other.
  rc_wait_loads();
  auto ldw3 = [&](int qa) {  // the first three column steps of the slice [qa, qb)
    ldw(wb0, qa + lane);
    if (qa + 64 < qb) ldw(wb1, qa + lane + 64);
    if (qa + 128 < qb) ldw(wb2, qa + lane + 128);
  };
  if (fz0 < fz1) ldw3(fz0 * cs * H);
  if (tid < F) {
    // torch CPU batch_norm: y = x * alpha + beta, alpha = invstd * gamma, beta = bias - mean * alpha
    const float mean = train ? (float)rc_keep(st_mean) : rc_keep(rn_mean);
    const double eps = rc_keep(bn_eps);
    const float inv = train ? (float)(1.0 / sqrt(rc_keep(st_var) + eps)) : 1.0f / sqrtf(rc_keep(rn_var) + (float)eps);
    const float a = inv * bw;
    alpha[tid] = a;
    beta[tid] = bb - mean * a;
  }
  __syncthreads();
  for (int e = tid; e < nb * pF; e += NT) {
    const int f = dF.mod(e);
    xs[e] = xs[e] * alpha[f] + beta[f];
  }
  __syncthreads();
  RC_PHASE(c.ws, c.wo.total, bx, 3);
  // Chebyshev filtering T_i = S_i x_bn (T_0 = x_bn exactly, as matmul(eye, x)), rows [ch0, ch1).
  // T and R go to LDS only here and in the graph convolution: a global store inside these loops
  // makes the compiler drain every load in flight (the fc1 weights) in front of the loop.  The
  // workspace copies the backward reads are stored from LDS after the fc1 products (store_TR).
  const int cF = (ch1 - ch0) * F, cH = (ch1 - ch0) * H;
  // the slice width's multipliers (host-computed for the regular, the last and the whole width)
  const int cw = ch1 - ch0;
  const int mb = cw == (int)c.mg[RC_MG_CS] ? RC_MG_CSF : (cw == (int)c.mg[RC_MG_LS] ? RC_MG_LSF : -1);
  const RcDiv32 dcF = mb >= 0 ? RcDiv32(cF, c.mg[mb]) : (cw == p ? RcDiv32(cF, c.mg[RC_MG_PF]) : RcDiv32(cF));
  const RcDiv32 dncF = mb >= 0 ? RcDiv32(n * cF, c.mg[mb + 1]) : (cw == p ? RcDiv32(n * cF, c.mg[RC_MG_NPF]) : RcDiv32(n * cF));
  const RcDiv32 dcH = mb >= 0 ? RcDiv32(cH, c.mg[mb + 2]) : (cw == p ? RcDiv32(cH, c.mg[RC_MG_PH]) : RcDiv32(cH));
  for (int e = tid; e < nb * n * cF; e += NT) {
    const int s = dncF.div(e), rs = e - s * n * cF, i = dcF.div(rs), qs = rs - i * cF;
    const int q = ch0 * F + qs, rem = i * pF + q, ch = dF.div(q), f = q - ch * F;
    float v;
    if (i == 0) {
      v = xs[s * pF + q];
    } else {
      v = 0.f;
      const float* Srow = Sl + (i * p + ch) * p;
      const float* xc = xs + s * pF + f;
      for (int cc = 0; cc < p; ++cc) v += Srow[cc] * xc[cc * F];
    }
    Tl[s * n * pF + rem] = v;
  }
  __syncthreads();
  RC_PHASE(c.ws, c.wo.total, bx, 4);  // (trace builds: the next mark is 6, after the graph convolution)
  // Z = sum_i T_i W_i ; R = relu(Z).  The loop is instantiated per address space of the weights
  // (LDS or global): through a generic pointer every weight read is a flat load, which counts as a
  // memory and an LDS access at once and ends each group of four in a full wait on both.
  auto gconv = [&](auto* Wsrc) {
    for (int e = tid; e < nb * cH; e += NT) {
      const int s = dcH.div(e), rem = ch0 * H + (e - s * cH), ch = dH.div(rem), hh = rem - ch * H;
      float a4[4] = {0.f, 0.f, 0.f, 0.f};  // four independent chains hide the LDS latency
      for (int i = 0; i < n; ++i) {
        const float* trow = Tl + (s * n + i) * pF + ch * F;
        auto* wc = Wsrc + i * F * H + hh;
        int f = 0;
        for (; f + 3 < F; f += 4) {
#pragma unroll
          for (int u = 0; u < 4; ++u) a4[u] += trow[f + u] * wc[(f + u) * H];
        }
        for (; f < F; ++f) a4[0] += trow[f] * wc[f * H];
      }
      Rl[s * pH + rem] = fmaxf((a4[0] + a4[1]) + (a4[2] + a4[3]), 0.f);
    }
  };
  if (w_lds)
    gconv(Wl);
  else
    gconv(gw);
  __syncthreads();
  // the workspace copies of T and R (read by the next launch: the kernel boundary orders them),
  // from LDS, by every workgroup that formed rows of them
  auto store_TR = [&]() {
    for (int e = tid; e < nb * n * cF; e += NT) {
      const int s = dncF.div(e), rs = e - s * n * cF, i = dcF.div(rs), rem = i * pF + ch0 * F + (rs - i * cF);
      ws[c.wo.T + (int64_t)(b0 + s) * n * pF + rem] = Tl[s * n * pF + rem];
    }
    for (int e = tid; e < nb * cH; e += NT) {
      const int s = dcH.div(e), rem = ch0 * H + (e - s * cH);
      ws[c.wo.R + (int64_t)(b0 + s) * pH + rem] = Rl[s * pH + rem];
    }
  };
  RC_PHASE(c.ws, c.wo.total, bx, 6);
  // fc1: wave wv owns rows [wv*RW, wv*RW+RW) (RW <= 16); lanes split the slice's columns.
  // Later column steps' weights are loaded while the current one is multiplied.
  // one window per workgroup (the single fit) multiplies only its own column: NB = 1 accumulators
  const int jrow = (lane >> 2) & 15, mrow = m0 + jrow;
  const bool wrow = (lane & 3) == 0 && jrow < RW && mrow < M1;  // the lane that holds row mrow's sum
  auto fc1 = [&](auto nbc) {
    constexpr int NB = decltype(nbc)::value;
    float tot[NB];  // row mrow of each window: the slice sums in slice order
    for (int z = fz0; z < fz1; ++z) {
      const int qa = z * cs * H;
      qb = qend(z);
      float acc[16][NB];
#pragma unroll
      for (int j = 0; j < 16; ++j)
#pragma unroll
        for (int s = 0; s < NB; ++s) acc[j][s] = 0.f;
      // column q of this lane (q ascending per lane: the same chains as one step per iteration).
      // A lane past the slice's end multiplies by zero instead of branching round the products: the
      // sums start at +0 and never become -0, so with finite weights adding w * 0 leaves their bits
      // (a non-finite weight in the slice's last column, which the lane that owns the column
      // multiplies anyway, makes the row's sum NaN where the branch left Inf or NaN), and with no
      // lane-dependent path round the uses of a buffer its refill waits for nothing.
      auto mul = [&](const float (&w)[16], int q) {
        const int qc = q < qb ? q : qb - 1;
        float rv[NB];
#pragma unroll
        for (int s = 0; s < NB; ++s) {
          const float x = Rl[(s < nb ? s : 0) * pH + qc];
          rv[s] = s < nb && q < qb ? x : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
          for (int s = 0; s < NB; ++s) acc[j][s] += w[j] * rv[s];
      };
      for (int q0 = qa; q0 < qb; q0 += 192) {  // wave-uniform steps of three column blocks
        const int q = q0 + lane;
        mul(wb0, q);
        if (q0 + 192 < qb) ldw(wb0, q + 192);
        if (q0 + 64 < qb) {
          mul(wb1, q + 64);
          if (q0 + 256 < qb) ldw(wb1, q + 256);
        }
        if (q0 + 128 < qb) {
          mul(wb2, q + 128);
          if (q0 + 320 < qb) ldw(wb2, q + 320);
        }
      }
      // the next slice's first column steps (the first slice's were requested ahead of BatchNorm),
      // into the same buffers, under this slice's reduce-scatter; a wave team has one slice
      if (!TEAM && z + 1 < fz1) {
        qb = qend(z + 1);
        ldw3((z + 1) * cs * H);
      }
      // reduce-scatter of the 16 row partials over the 64 lanes: 17 shuffles per window instead of
      // 16 full reductions (96); afterwards lane l holds row (l >> 2) & 15 in every lane of its quad
#pragma unroll
      for (int s = 0; s < NB; ++s) {
        if (s >= nb) break;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = acc[j][s];
#pragma unroll
        for (int half = 8; half >= 1; half >>= 1) {
          const int off = half * 4;  // lane bit that selects the kept half: 32, 16, 8, 4
          const bool hi = lane & off;
#pragma unroll
          for (int i = 0; i < half; ++i) {
            const float send = hi ? v[i] : v[i + half];
            const float keep = hi ? v[i + half] : v[i];
            v[i] = keep + __shfl_xor(send, off, 64);
          }
        }
        float t = v[0];
        t += __shfl_xor(t, 2, 64);
        t += __shfl_xor(t, 1, 64);
        tot[s] = z == fz0 ? t : tot[s] + t;
      }
    }
    if (TEAM) {  // this team's slice sums, exchanged through LDS below
      if (wrow && fz0 < fz1) partl[team * M1 + mrow] = tot[0];
    } else if (zs < 0) {  // every slice here: f1 = slice sums + bias
#pragma unroll
      for (int s = 0; s < NB; ++s) {
        if (s >= nb) break;
        if (wrow) {
          const float val = tot[s] + fb1[mrow];
          f1l[s * M1 + mrow] = val;
          ws[c.wo.f1 + (int64_t)(b0 + s) * M1 + mrow] = val;
        }
      }
    } else if (wrow) {  // this slice's partial, written through for the window's last workgroup
      rc_store_sc1(ws + c.wo.f1p + ((int64_t)zs * d.Bmax + b0) * M1 + mrow, tot[0]);
    }
  };
  fc1(std::integral_constant<int, NBT>{});  // NBT >= SB (k_forward's instantiation for this launch)
  if (TEAM) {
    __syncthreads();
    RC_PHASE(c.ws, c.wo.total, bx, 12);  // (trace builds: the teams' slice sums are in LDS)
    if (tid < M1) {
      const float val = Zs > 1 ? (partl[tid] + partl[M1 + tid]) + fb1[tid] : partl[tid] + fb1[tid];
      f1l[tid] = val;
      ws[c.wo.f1 + (int64_t)b0 * M1 + tid] = val;
    }
  } else if (zs >= 0) {  // arrival: the last of the window's Zs workgroups sums the partials and runs fc2
    __shared__ unsigned last;
    unsigned* cnt = reinterpret_cast<unsigned*>(ws + c.wo.ecnt) + p * rc_nchunk(d) + 1 + b0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its partials
    __syncthreads();
    unsigned seen = 0u;
    if (tid == 0) seen = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    store_TR();  // every slice's workgroup stores its rows, while the count's round trip is under way
    if (tid == 0) last = seen == (unsigned)(Zs - 1);
    __syncthreads();
    if (!last) return;
    if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler barrier only: the partial loads are sc1
    if (tid < M1) {
      // the slice partials' loads in flight together, eight per round (a runtime-count loop waited
      // for each load in turn), summed in slice order
      const float* part = ws + c.wo.f1p + (int64_t)b0 * M1 + tid;
      float sum = 0.f;
      for (int z0 = 0; z0 < Zs; z0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = z0 + u < Zs ? rc_load_sc1(part + (int64_t)(z0 + u) * d.Bmax * M1) : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (z0 + u < Zs) sum = z0 + u == 0 ? v[0] : sum + v[u];
      }
      const float val = sum + fb1[tid];
      f1l[tid] = val;
      ws[c.wo.f1 + (int64_t)b0 * M1 + tid] = val;
    }
  }
  __syncthreads();
  RC_PHASE(c.ws, c.wo.total, bx, 7);
  if (zs < 0) store_TR();  // beside fc2, which a few threads run (their stores' round trip runs under it)
  for (int e = tid; e < nb * K; e += NT) {
    const int s = e / K, k = e - s * K;
    const float* w2 = fc2s + k * M1;
    float a = 0.f;
    for (int m = 0; m < M1; ++m) a += w2[m] * fmaxf(f1l[s * M1 + m], 0.f);
    ws[c.wo.w + (int64_t)(b0 + s) * K + k] = a + fb2[k];
  }
  RC_PHASE(c.ws, c.wo.total, bx, 8);
  RC_WG_MARK(c.ws, c.wo.total, RC_KID_EMB_FWD, 1);
}

size_t emb_fwd_floats(const RedcliffDims& d, int SB, int w_lds, bool team = false) {
  const size_t pF = (size_t)d.p * d.F, pH = (size_t)d.p * d.H;
  return SB * pF + (size_t)d.n * d.p * d.p + (w_lds ? (size_t)d.n * d.F * d.H : 0) + SB * d.n * pF + SB * pH +
         (size_t)SB * d.M1 + (size_t)d.K * d.M1 + d.M1 + d.K + 2 * d.F + (team ? 2 * d.M1 : 0);
}

// ------------------------------------------------------------------------------------------
// Factor forward of one (factor, channel network, FAC_UC-unit hidden chunk): relu activations
// a[kj][b][u], partial outputs y[uc][kj][b] = sum_{u in chunk} W1[u] a[b][u] (+ b1 in chunk
// 0), the chunk's squared layer-0 group norms gq[uc][kj][q] and a snapshot of W1.
// The whole window block and weight chunk are staged in one pass when p*L <= FQ_MAX.
// mfma (slab tiles, Q <= FQ_MAX): the products run on the matrix cores as 16x16x4 chains (rows = the
// chunk's units, columns = a tile of 16 windows, waves take the window tiles in turn), a k-ascending
// fmaf chain per output from 0 like the vector loop's and rc_fac_bwd.h's recompute, so the same bits.
// The tile rows stay QT + 1 wide and unpadded: the reads of the last k-steps are clamped to column
// Q - 1 and zeros selected (rc_mfma_chain16<., true>).  32-column tiles (Q > FQ_MAX) keep the vector loop.
// (trace builds: phase marks 64-67 of factor workgroup 0 -- staged, group norms stored, products
// done (wave 0's first chain), outputs stored)
// MF is a template parameter so that a launch of the vector form carries none of the chains' registers.
template <int NT, bool MF>
__device__ __attribute__((always_inline)) void fac_fwd_body(const StepCtx& c, int bx, float* sm) {
  constexpr int UD = NT / RC_BLOCK, NI = FK_BT * FAC_UC / NT;  // NI: windows per thread of the vector loop
  const RedcliffDims& d = c.d;
  RC_WG_MARK(c.ws, c.wo.total, RC_KID_FAC_FWD, 0);
  const int nU = rc_nuchunk(d);
  const int r = rc_rep(c, blockIdx.y), kj = RcDiv32(nU, c.mg[RC_MG_NU]).div(bx), uc = bx - kj * nU;
  const int p = d.p, h = d.h, K = d.K;
  const int Q = p * d.L, QT = fq_tile(d), QP = QT + 1;
  const bool slab = Q <= FQ_MAX;  // QT == Q: a tile row is the window's whole slab, the W0 chunk one range
  const int u0 = uc * FAC_UC;
  const float* P = c.fac + r * c.fs;
  const float* W0 = P + c.fo.W0 + (int64_t)kj * h * Q;
  const float* b0 = P + c.fo.b0 + (int64_t)kj * h;
  const float* W1 = P + c.fo.W1 + (int64_t)kj * h;
  const float b1 = uc == 0 ? P[c.fo.b1 + kj] : 0.f;
  float* ws = c.ws + r * c.wss;
  const float* X = c.X + r * c.xr;
  const int tid = threadIdx.x, tb = tid >> 4, tu = tid & 15;
  const int u = u0 + tu;
  const RcDiv32 dQ(Q, c.mg[RC_MG_Q]);
  float* Xs = sm;                // [FK_BT][QT+1]
  float* Ws = Xs + FK_BT * QP;   // [FAC_UC][QT+1]
  const int nrow = min(FAC_UC, h - u0);  // the chunk's rows below h: nrow * Q contiguous floats of W0
  const float* W0c = W0 + u0 * Q;        // (32-bit offsets inside the factor slice, as in rc_fac_bwd.h)
  const float bu = u < h ? b0[u] : 0.f, w1 = u < h ? W1[u] : 0.f;
  // matrix-core form: lane (l15, lg) holds units u0 + 4 lg .. + 3 of window 16 tile + l15
  const bool mf = MF && slab;
  const int lane = tid & 63, fwv = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, lg = lane >> 4;
  float bu4[4], w14[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int uu = u0 + 4 * lg + reg;
    bu4[reg] = mf && uu < h ? b0[uu] : 0.f;
    w14[reg] = mf && uu < h ? W1[uu] : 0.f;
  }

  for (int bc = 0; bc < c.B; bc += FK_BT) {
    float acc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = 0.f;
    for (int q0 = 0; q0 < Q; q0 += QT) {
      if (q0 > 0 || bc > 0) __syncthreads();
      // (rows past B of the window tile are not staged: their sums are never stored)
      rc_stage_all(
          rc_win_seg<24 / UD, 5, NT>(rc_win(c, X, bc), slab, min(FK_BT, c.B - bc), q0, Xs, QP, Q),
          rc_segc<4 / UD, NT>(slab ? nrow * Q : 0, [&](int e) { return W0c[(unsigned)e]; }, [&](int e, float v) {
            const int uu = dQ.div(e);
            Ws[uu * QP + e - uu * Q] = v;
          }),
          rc_segc<2 / UD, NT>(slab ? 0 : FAC_UC * 32, [&](int e) {  // 32-column tiles (QT == 32)
            const int uu = e >> 5, q = q0 + (e & 31);
            const bool in = uu < nrow && q < Q;
            const float w = W0c[(unsigned)(in ? uu * Q + q : 0)];
            return in ? w : 0.f;
          }, [&](int e, float v) { Ws[(e >> 5) * QP + (e & 31)] = v; }));
      if (slab)  // a partial chunk: the rows past h are zero
        for (int e = nrow * QP + tid; e < FAC_UC * QP; e += NT) Ws[e] = 0.f;
      __syncthreads();
      if (bc == 0 && q0 == 0) RC_PHASE(c.ws, c.wo.total, bx, 64);
      if (bc == 0)
        for (int qq = tid; qq < QT && q0 + qq < Q; qq += NT) {
          // squared group norms of the chunk's 16 units (GC, models/cmlp.py:162-166), pre-update
          float sq = 0.f;
          for (int uu = 0; uu < FAC_UC; ++uu) {
            const float w = Ws[uu * QP + qq];
            sq += w * w;
          }
          ws[c.wo.gq + ((int64_t)uc * K * p + kj) * Q + q0 + qq] = sq;
        }
      if (bc == 0 && q0 == 0) RC_PHASE(c.ws, c.wo.total, bx, 65);
      if (mf) break;  // (slab: the one column tile; its products follow)
      const int qn = min(QT, Q - q0);
#pragma unroll 8
      for (int qq = 0; qq < qn; ++qq) {
        const float wv = Ws[tu * QP + qq];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i] = fmaf(Xs[(tb + (NT / 16) * i) * QP + qq], wv, acc[i]);  // rc_fac_bwd.h recomputes this chain
      }
    }
    if (bc == 0 && tb == 0 && u < h) ws[c.wo.w1 + (int64_t)kj * h + u] = w1;
    if (mf) {
      const float* wr = Ws + l15 * QP;  // A: unit row l15 of the chunk, k = column
      for (int bt = fwv; bt < (min(FK_BT, c.B - bc) + 15) / 16; bt += NT / 64) {
        const float* xr = Xs + (16 * bt + l15) * QP;  // B: window 16 bt + l15
        const f32x4 z = rc_mfma_chain16<FF_KB, true>(
            f32x4{0.f, 0.f, 0.f, 0.f}, Q, lg, [&](int kc) { return wr[kc]; }, [&](int kc) { return xr[kc]; });
        if (bc == 0 && bt == 0) RC_PHASE(c.ws, c.wo.total, bx, 66);
        const int b = bc + 16 * bt + l15;
        float ys[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int uu = u0 + 4 * lg + reg;
          ys[reg] = 0.f;
          if (uu < h) {
            const float a = fmaxf(z[reg] + bu4[reg], 0.f);
            if (b < c.B && !rc_fac_recompute(d)) ws[c.wo.a + ((int64_t)kj * d.Bmax + b) * h + uu] = a;
            ys[reg] = w14[reg] * a;
          }
        }
        // the vector form's butterfly over the 16 units (u ^ 8, ^ 4, ^ 2, ^ 1): unit = 4 lg + reg, so
        // the first two levels pair lane groups (lanes ^ 32, ^ 16) and the last two pair registers
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) ys[reg] += __shfl_xor(ys[reg], 32, 64);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) ys[reg] += __shfl_xor(ys[reg], 16, 64);
        const float y = (ys[0] + ys[2]) + (ys[1] + ys[3]);
        if (lg == 0 && b < c.B) ws[c.wo.y + rc_y_idx(d, uc, kj, b)] = y + b1;
      }
      continue;
    }
    if (bc == 0) RC_PHASE(c.ws, c.wo.total, bx, 66);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int b = bc + tb + (NT / 16) * i;
      float ys = 0.f;
      if (u < h) {
        const float a = fmaxf(acc[i] + bu, 0.f);
        if (b < c.B && !rc_fac_recompute(d)) ws[c.wo.a + ((int64_t)kj * d.Bmax + b) * h + u] = a;
        ys = w1 * a;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) ys += __shfl_xor(ys, o, 64);
      if (tu == 0 && b < c.B) ws[c.wo.y + rc_y_idx(d, uc, kj, b)] = ys + b1;
    }
  }
  RC_PHASE(c.ws, c.wo.total, bx, 67);
  RC_WG_MARK(c.ws, c.wo.total, RC_KID_FAC_FWD, 1);
}

size_t fac_fwd_floats(const RedcliffDims& d) {
  const int QT = d.p * d.L <= FQ_MAX ? d.p * d.L : 32;
  return (size_t)(FK_BT + FAC_UC) * (QT + 1);
}

// grid (nemb + nfac, R): embedder blocks first, then factor blocks.
// split: one (window, channel slice) per embedder workgroup (SB = 1), window-major.  NBT: the fc1
// accumulator columns (windows per workgroup, SB <= NBT): one instantiation per SB keeps the
// single fit's kernel (NBT = 1) at its own register count, not the 4-window one's.
// NT: the workgroup's threads -- RC_BLOCK, or RC_EMB_TEAM_NT when every embedder workgroup runs its
// window's (at most two) fc1 slices as wave teams; MF: the factor products on the matrix cores.
template <int NBT, int NT, bool MF>
__global__ __launch_bounds__(NT) void k_forward(StepCtx c, int SB, int w_lds, int nemb, int cs, int split) {
  extern __shared__ float sm[];
  // every step with an embedder forward re-arms the merged backward's factor-lead counter (the
  // kernel boundary orders this store before k_bwd_merged's polls)
  if (blockIdx.x == 0 && nemb > 0 && threadIdx.x == 0)
    *rc_fac_lead_cnt(c, c.ws + rc_rep(c, blockIdx.y) * c.wss) = 0u;  // published factor leads
  if ((int)blockIdx.x < nemb) {
    if (NT == RC_EMB_TEAM_NT) {
      emb_fwd_body<NBT, NT>(c, blockIdx.x, 1, w_lds, cs, -1, sm);
    } else if (split) {
      const RcDiv32 dZs = cs == (int)c.mg[RC_MG_CS] ? RcDiv32(c.fzs, c.mg[RC_MG_ZS]) : RcDiv32((c.d.p + cs - 1) / cs);
      const int Zs = dZs.d, b = dZs.div(blockIdx.x);
      emb_fwd_body<NBT, NT>(c, b, 1, w_lds, cs, blockIdx.x - b * Zs, sm);
    } else {
      emb_fwd_body<NBT, NT>(c, blockIdx.x, SB, w_lds, cs, -1, sm);
    }
  } else
    fac_fwd_body<NT, MF>(c, blockIdx.x - nemb, sm);
}

}  // namespace

// Dynamic LDS above 64 KiB (up to the CU's 160 KiB) must be opted into per kernel.
template <class Kern>
static int lds_optin(Kern k, size_t bytes, const char* what) {
  if (bytes <= RC_LDS_LIMIT_FLOATS * sizeof(float)) return 0;
  return rc_check(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)bytes), what);
}

// Channels per fc1 slice of the embedder forward (emb_fwd_body): slices of about RC_EMB_FWD_COLS
// columns of the p*H contraction (REDCLIFF_EMB_FWD_COLS overrides; 0 = one slice).  A function of
// the model's dimensions only -- never of R or the windows per workgroup -- so a packed fit and an
// independent one sum fc1 in the same slices (bit for bit).
#ifndef RC_EMB_FWD_COLS
#define RC_EMB_FWD_COLS 200
#endif
int rc_emb_fwd_slice_channels(const RedcliffDims& d) {
  static const int cols = [] {
    const char* v = getenv("REDCLIFF_EMB_FWD_COLS");
    return v ? atoi(v) : RC_EMB_FWD_COLS;
  }();
  if (cols <= 0) return d.p;
  int cs = cols / d.H > 1 ? cols / d.H : 1;
  const int cmin = (d.p + 63) / 64;  // at most 64 slices (the partial region's slots)
  if (cs < cmin) cs = cmin;
  return cs < d.p ? cs : d.p;
}

void rc_ctx_magics(StepCtx& c) {
  const RedcliffDims& d = c.d;
  const int cs = rc_emb_fwd_slice_channels(d), Zs = (d.p + cs - 1) / cs, ls = d.p - (Zs - 1) * cs;
  const long long v[RC_MG_NCH] = {d.F, d.p, (long long)d.p * d.F, (long long)d.n * d.F, d.K, d.M1, d.H, d.L, c.B,
                                (long long)d.n * d.p * d.F, (long long)d.p * d.H,
                                0, (long long)cs * d.F, (long long)d.n * cs * d.F, (long long)cs * d.H,
                                0, (long long)ls * d.F, (long long)d.n * ls * d.F, (long long)ls * d.H};
  c.ewpb = rc_emb_wpb(d);
  c.enbwm = rc_emb_nbw(d);
  c.enbw = (c.B + c.ewpb - 1) / c.ewpb;
  for (int i = 0; i < RC_MG_NCH; ++i) c.mg[i] = rc_magic32(v[i]);
  c.mg[RC_MG_NCH] = rc_magic32(rc_nchunk(d));
  c.mg[RC_MG_ENBW] = rc_magic32(c.enbw);
  c.fzs = Zs;
  c.mg[RC_MG_ZS] = rc_magic32(Zs);
  c.mg[RC_MG_Q] = rc_magic32((long long)d.p * d.L);
  c.mg[RC_MG_NU] = rc_magic32(rc_nuchunk(d));
  c.mg[RC_MG_CS] = (unsigned)cs;  // the widths themselves (the slice's width picks its slots)
  c.mg[RC_MG_LS] = (unsigned)ls;
}

// One launch of the embedder forward (with_emb) and / or the vector-path factor forward (with_fac).
int rc_launch_forward(const StepCtx& c, hipStream_t s, bool with_emb, bool with_fac, hipEvent_t stop) {
  const RedcliffDims& d = c.d;
  int SB = 1, w_lds = 1, nemb = 0, split = 0, team = 0;
  const int cs = rc_emb_fwd_slice_channels(d);
  // REDCLIFF_FWD_MFMA=0: the factor products of the 512-thread launch as the vector loop;
  // REDCLIFF_EMB_FWD_TEAMS=0: a window's fc1 slices on workgroups of their own (both read per call:
  // the same bits either way)
  const char* fmv = getenv("REDCLIFF_FWD_MFMA");
  const char* tmv = getenv("REDCLIFF_EMB_FWD_TEAMS");
  size_t lds = 0;
  if (with_emb) {
    static const int sb_env = [] {
      const char* v = getenv("REDCLIFF_EMB_SB");  // tuning knob: windows per forward workgroup
      const int x = v ? atoi(v) : 0;
      return (x >= 1 && x <= 4) ? x : 0;  // the fc1 stage holds at most 4 windows per workgroup
    }();
    // one window per workgroup keeps a single fit's forward short (latency); packed replicas
    // fill the chip anyway, and 4 windows per workgroup share one staging of the embedder
    // weights (R = 32 D4IC grid: forward 158 -> 64 us).  Per-window arithmetic does not
    // depend on SB, so packed fits stay bitwise equal to independent ones.
    SB = sb_env ? sb_env : (d.R >= 8 ? 4 : 1);
    size_t limit = RC_LDS_LIMIT_FLOATS;
    while (SB > 1 && emb_fwd_floats(d, SB, w_lds) > limit) --SB;
    if (emb_fwd_floats(d, SB, w_lds) > limit) w_lds = 0;
    if (emb_fwd_floats(d, SB, w_lds) > limit) limit = RC_LDS_MAX_FLOATS;  // large p*F: one workgroup per CU
    if (emb_fwd_floats(d, SB, w_lds) > limit) { rc_set_error("embedder forward: LDS budget exceeded"); return REDCLIFF_ELIMIT; }
    nemb = (c.B + SB - 1) / SB;
    // one window per workgroup with at most two fc1 slices: the slices as wave teams of one workgroup
    team = SB == 1 && (d.p + cs - 1) / cs <= 2 && (!tmv || strcmp(tmv, "0") != 0) &&
           emb_fwd_floats(d, SB, w_lds, true) <= limit;
    lds = emb_fwd_floats(d, SB, w_lds, team);
    if (!team && SB == 1 && cs < d.p) {  // one window per workgroup: its slices on workgroups of their own
      split = 1;
      nemb = c.B * ((d.p + cs - 1) / cs);
    }
  }
  int nfac = 0;
  if (with_fac) {
    if (d.h > 128 || d.p * d.L > 4096) { rc_set_error("factor forward: h <= 128 and p*L <= 4096 required"); return REDCLIFF_ELIMIT; }
    // (the window tiles are staged with 32-bit offsets from one pointer per workgroup, rc_win)
    if ((int64_t)d.Bmax * d.T * d.p >= (1ll << 30)) { rc_set_error("factor forward: Bmax*T*p < 2^30 required"); return REDCLIFF_ELIMIT; }
    nfac = d.K * d.p * rc_nuchunk(d);
    const size_t f = fac_fwd_floats(d);
    lds = f > lds ? f : lds;
  }
  if (nemb + nfac == 0) return 0;
  lds *= sizeof(float);
  const int nt = team ? RC_EMB_TEAM_NT : RC_BLOCK;
  // The matrix-core products run where the workgroups have eight waves (one window tile per wave at
  // B = 128).  The 256-thread launches keep the vector loop: TST's step measured slower with the
  // chains, and as an instantiation of their own they need 132 registers (3 waves).
  const int fmf = team && (!fmv || strcmp(fmv, "0") != 0);
  auto launch = [&](auto kern) {
    int e = lds_optin(kern, lds, "k_forward LDS");
    if (e) return e;
    if (stop)
      hipExtLaunchKernelGGL(kern, dim3(nemb + nfac, c.nrep), dim3(nt), lds, s, nullptr, stop, 0, c, SB, w_lds, nemb,
                            cs, split);
    else
      hipLaunchKernelGGL(kern, dim3(nemb + nfac, c.nrep), dim3(nt), lds, s, c, SB, w_lds, nemb, cs, split);
    return rc_check(hipGetLastError(), "k_forward");
  };
  if (team) return fmf ? launch(k_forward<1, RC_EMB_TEAM_NT, true>) : launch(k_forward<1, RC_EMB_TEAM_NT, false>);
  if (SB == 1) return launch(k_forward<1, RC_BLOCK, false>);
  if (SB == 2) return launch(k_forward<2, RC_BLOCK, false>);
  return launch(k_forward<4, RC_BLOCK, false>);
}

int rc_launch_fac_fwd(const StepCtx& c, hipStream_t s) { return rc_launch_forward(c, s, false, true); }
