// Fused scene-point (64-wide row) chains of a GASFM block, gfx950.
//
// Every consumer of a block's point features p [n x 64] runs in ONE kernel per direction:
//
//   tail (produces p, reference Proj2ScenePoint.forward, code/models/layers.py:418-458):
//     x = prev + W_p agg + b_p                     proj_proj2scenepoint + state skip  :438-444
//     p = x + W_m relu(LN(x)) + b_m                norm_pre_mlp, ReLU, mlp, skip      :447-454
//   hub (consumes p):
//     s  = W_A relu(LN_A(p))                       ProjectionFeatureUpdate lin_scenepoint  :924-935
//     xl = W_B p + b_B                             ViewAndScenePoint2Global scenepoint lin_l (:560-575)
//     xr = W_D (W_C relu(LN_C(p)) + b_C) + b_D     NEXT block's norm_and_proj_scenepoint2proj
//                                                  (:429) and its GATv2 lin_r (target rows)
//   plus the identity output p -> next block's state skip (:442).
//
// The point tensor is 51 MB at config 4.  aten runs these chains as ~8 kernels forward
// (LayerNorm, clamp, GEMMs, adds) and ~20 backward, re-reading p for every consumer, and
// autograd sums the four gradients of p with three more full-size adds.  Here the backward
// of the hub reads the four upstream gradients once and writes dp once (the skip gradient
// arrives as the hub's identity output), and the tail's backward writes d prev (== dx) and
// d agg in the same pass.
//
// Layout: wave = 16-row tile (tile.hpp); GEMMs on v_mfma_f32_16x16x4_f32 against weights
// staged once per workgroup in LDS as float4 slabs in the order the MFMA operands are read.  A
// tile stays in registers from its global load to its global store: the forward kernels
// (*_fwd_t_kernel) chain transposed products, the backward kernels (*_bwd_r_kernel) read every
// tensor in the layout its consumer wants; see the comment at the head of each section.
// LayerNorm statistics are recomputed from p in the backward pass.  Weight / bias / gamma /
// beta gradients leave as per-workgroup partial rows reduced by gasfm_colsum in a fixed order
// (deterministic, no atomics).
//
// History: the first generation of these kernels staged every tile through LDS (87-150 KB per
// workgroup) and ran the hub backward as two passes with an extra write + read of dp.  The
// register-resident forms measured 40.7 -> 35.4 us (tail forward), 57.2 -> 43.9 us (hub forward),
// 93.6 -> 79.6 us (tail backward) and 63 + 78 -> 116 us (hub backward, n = 200k) and replaced
// them (the kernel table; profiles/r6_ab_kernels_sched_ring.txt); the old kernels and
// their build switches are in the git history at b512b46.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "tile.hpp"

namespace gasfm {
namespace {

using namespace tile;

constexpr int FP = 64;  // n_feat_scenepoint
constexpr int FA = 32;  // n_feat_proj (aggregation / projection width)

// partial-row layouts (floats), one row per workgroup of a backward kernel
constexpr int TAIL_PART = FP * FP + FP * FA + 4 * FP;  // dWm dWp dbm dbp dgam dbet
// hub, part_a: dW_A [32 x 64] | dW_B [64 x 64] | db_B | dgamma_A | dbeta_A
constexpr int HA_WA = 0, HA_WB = HA_WA + FA * FP, HA_BB = HA_WB + FP * FP, HA_GA = HA_BB + FP, HA_BA = HA_GA + FP,
              HA_PART = HA_BA + FP;
// hub, part_c: dW_C [32 x 64] | dW_D [32 x 32] | db_C | db_D | dgamma_C | dbeta_C
constexpr int HC_WC = 0, HC_WD = HC_WC + FA * FP, HC_BC = HC_WD + FA * FA, HC_BD = HC_BC + FA, HC_GC = HC_BD + FA,
              HC_BCL = HC_GC + FP, HC_PART = HC_BCL + FP;

// ----------------------------------------------------------------------------- forward, register-resident
// Computing the TRANSPOSED products Y^T = W X^T keeps a 16-row tile in registers from load to
// store (no LDS round trip between layers): with A = W and B = X^T, v_mfma_f32_16x16x4_f32 leaves lane
// (g = lane>>4, c = lane&15) holding Y[row c][16 ot + 4 g + r] (r < 4) -- 16 features of row c --
// and those registers are exactly the B operand of the next layer when its k index is permuted
// to k = 16 u + 4 g + j at step (u, j) (any consistent k order gives the same sum).  The weights
// are staged once per workgroup pre-permuted to match, as float4 slabs read with one conflict-free
// ds_read_b128 per 4 MFMAs.  Rows load and store as float4 (64 B per row per slab).  Row
// statistics: 16 values per lane, then a sum over the 4 lane groups.  Only weights live in LDS
// (24-37 KB per workgroup), so occupancy is set by VGPRs.
#ifndef GASFM_PT_FWD_T_MINW
#define GASFM_PT_FWD_T_MINW 1
#endif
// 1: re-read the weight slabs from LDS every tile (a compiler memory barrier at the top of the
// tile loop keeps them from being hoisted into registers: ~100 fewer VGPRs, more waves per SIMD);
// 0: the compiler keeps them in VGPRs across tiles
#ifndef GASFM_PT_FWD_T_LDSW
#define GASFM_PT_FWD_T_LDSW 1
#endif
// waves per workgroup (4, 8 and 16 measured: 16 slowest, 4 and 8 within 1 us)
#ifndef GASFM_PT_FWD_T_WAVES
#define GASFM_PT_FWD_T_WAVES 4
#endif
constexpr int kWavesT = GASFM_PT_FWD_T_WAVES, kThreadsT = kWavesT * kW;

// W [O x K] (torch Linear [out, in]) -> float4 slabs Q[(ot * (K/16) + u) * 64 + 16 g + c] =
// (W[16 ot + c][16 u + 4 g + j], j < 4)
template <int O, int K, int NT>
__device__ __forceinline__ void stage_slabs(const float* __restrict__ W, float* Q) {
  Stage<O * K, NT> s;
  s.load([&](int q) { return W[q]; });
  s.store([&](int q, float v) {
    const int o = q / K, k = q % K;
    Q[(((o / 16) * (K / 16) + k / 16) * 64 + ((k % 16) / 4) * 16 + o % 16) * 4 + k % 4] = v;
  });
}

// acc[ot] += W . X^T over K = 16 KU (X as k-slabs xk[u] = X[row c][16 u + 4 g + j])
template <int OT, int KU>
__device__ __forceinline__ void layer_t(const float4* __restrict__ Q, const f32x4 (&xk)[KU], f32x4 (&acc)[OT],
                                        int lane) {
  // the OT accumulators interleaved (consecutive MFMAs independent: a dependent chain waits the
  // full pipeline latency per step), and the next k-slab's weights read from LDS while this one's
  // MFMAs run
  float4 w[OT];
#pragma unroll
  for (int ot = 0; ot < OT; ++ot) w[ot] = Q[ot * KU * 64 + lane];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    float4 wn[OT];
    if (u + 1 < KU) {
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) wn[ot] = Q[(ot * KU + u + 1) * 64 + lane];
    }
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(w[ot].x, xk[u][0], acc[ot]);
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(w[ot].y, xk[u][1], acc[ot]);
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(w[ot].z, xk[u][2], acc[ot]);
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(w[ot].w, xk[u][3], acc[ot]);
    if (u + 1 < KU) {
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) w[ot] = wn[ot];
    }
  }
}

// per-feature vector V[64] (LDS) at this lane's features 16 ot + 4 g + r
__device__ __forceinline__ f32x4 vec_at(const float* V, int ot, int g) {
  const float4 v = *reinterpret_cast<const float4*>(V + 16 * ot + 4 * g);
  return f32x4{v.x, v.y, v.z, v.w};
}

// slab u of row c (clamped to a valid row; rows past nrows are computed and not stored)
template <int W>
__device__ __forceinline__ void slabs_load(const float* __restrict__ X, int64_t row0, int nrows, f32x4 (&v)[W / 16],
                                           int lane) {
  const int c = lane & 15, g = lane >> 4;
  const float* p = X + (row0 + (c < nrows ? c : nrows - 1)) * W + 4 * g;
#pragma unroll
  for (int u = 0; u < W / 16; ++u) {
    const float4 t = *reinterpret_cast<const float4*>(p + 16 * u);
    v[u] = f32x4{t.x, t.y, t.z, t.w};
  }
}
template <int W>
__device__ __forceinline__ void slabs_store(float* __restrict__ X, int64_t row0, int nrows, const f32x4 (&v)[W / 16],
                                            int lane) {
  const int c = lane & 15, g = lane >> 4;
  if (c >= nrows) return;
  float* p = X + (row0 + c) * W + 4 * g;
#pragma unroll
  for (int u = 0; u < W / 16; ++u) *reinterpret_cast<float4*>(p + 16 * u) = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
}

// mean and rstd of the 64-wide rows held as 4 slabs per lane (row c over the 4 lane groups)
__device__ __forceinline__ void slab_stats(const f32x4 (&x)[4], float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) s += (x[u][0] + x[u][1]) + (x[u][2] + x[u][3]);
  mean = sum_groups(s) * (1.f / FP);
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) q = fmaf(x[u][j] - mean, x[u][j] - mean, q);
  rstd = rsq_normal(sum_groups(q) * (1.f / FP) + eps);
}

// One 16-row tile of the tail in registers (T layout in, T layout out): y = x + W_m relu(LN(x)) + b_m,
// x = prev + W_p agg + b_p; V = [b_p | gamma | beta | b_m] in LDS.  Shared by the tail kernel and the
// fused tail + hub kernel (the same instruction sequence: bitwise the same p).
__device__ __forceinline__ void tail_tile_t(const float4* __restrict__ WpQ, const float4* __restrict__ WmQ,
                                            const float* V, const f32x4 (&ag)[2], const f32x4 (&pv)[4], float eps,
                                            int lane, f32x4 (&y)[4]) {
  const int g = lane >> 4;
  f32x4 x[4];
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) x[ot] = vec_at(V, ot, g) + pv[ot];  // b_p + prev, then + W_p agg
  layer_t<4, 2>(WpQ, ag, x, lane);
  f32x4 gm[4], bt[4];
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) {
    gm[ot] = vec_at(V + FP, ot, g);
    bt[ot] = vec_at(V + 2 * FP, ot, g);
  }
  float mean, rstd;
  slab_stats(x, eps, mean, rstd);
  f32x4 h[4];
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int j = 0; j < 4; ++j) h[ot][j] = fmaxf(fmaf((x[ot][j] - mean) * rstd, gm[ot][j], bt[ot][j]), 0.f);
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) y[ot] = vec_at(V + 3 * FP, ot, g);  // b_m, then + W_m h
  layer_t<4, 4>(WmQ, h, y, lane);
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) y[ot] = x[ot] + y[ot];
}

// One 16-row tile of the hub on p in registers (T layout): XL = W_B p + b_B, SA = W_A relu(LN_A p),
// (HC) XR = W_D (W_C relu(LN_C p) + b_C) + b_D, stored as rows row0 .. row0 + nrows - 1.
// V = [gamma_A | beta_A | gamma_C | beta_C | b_B | b_C (32) | b_D (32)] in LDS.
template <bool HC>
__device__ __forceinline__ void hub_tile_t(const f32x4 (&p)[4], float eps, const float4* __restrict__ WAQ,
                                           const float4* __restrict__ WBQ, const float4* __restrict__ WCQ,
                                           const float4* __restrict__ WDQ, const float* V, int lane, int64_t row0,
                                           int nrows, float* __restrict__ SA, float* __restrict__ XL,
                                           float* __restrict__ XR) {
  const int g = lane >> 4;
  float mean, rstd;
  slab_stats(p, eps, mean, rstd);
  {
    f32x4 xl[4];
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) xl[ot] = vec_at(V + 4 * FP, ot, g);  // b_B, then + W_B p
    layer_t<4, 4>(WBQ, p, xl, lane);
    slabs_store<FP>(XL, row0, nrows, xl, lane);
  }
  f32x4 h[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const f32x4 gm = vec_at(V, u, g), bt = vec_at(V + FP, u, g);
#pragma unroll
    for (int j = 0; j < 4; ++j) h[u][j] = fmaxf(fmaf((p[u][j] - mean) * rstd, gm[j], bt[j]), 0.f);
  }
  {
    f32x4 sa[2] = {zero4(), zero4()};
    layer_t<2, 4>(WAQ, h, sa, lane);
    slabs_store<FA>(SA, row0, nrows, sa, lane);
  }
  if (HC) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f32x4 gm = vec_at(V + 2 * FP, u, g), bt = vec_at(V + 3 * FP, u, g);
#pragma unroll
      for (int j = 0; j < 4; ++j) h[u][j] = fmaxf(fmaf((p[u][j] - mean) * rstd, gm[j], bt[j]), 0.f);
    }
    f32x4 tq[2] = {vec_at(V + 5 * FP, 0, g), vec_at(V + 5 * FP, 1, g)};  // b_C, then + W_C h
    layer_t<2, 4>(WCQ, h, tq, lane);
    f32x4 xr[2] = {vec_at(V + 5 * FP + FA, 0, g), vec_at(V + 5 * FP + FA, 1, g)};  // b_D, then + W_D t
    layer_t<2, 2>(WDQ, tq, xr, lane);
    slabs_store<FA>(XR, row0, nrows, xr, lane);
  }
}

// weights and vectors of the hub in LDS (every thread of the workgroup takes part)
template <bool HC, int NT>
__device__ __forceinline__ void hub_stage_t(const float* __restrict__ gA, const float* __restrict__ bA,
                                            const float* __restrict__ WA, const float* __restrict__ WB,
                                            const float* __restrict__ bB, const float* __restrict__ gC,
                                            const float* __restrict__ bC, const float* __restrict__ WC,
                                            const float* __restrict__ bWC, const float* __restrict__ WD,
                                            const float* __restrict__ bD, float4* WAQ, float4* WBQ, float4* WCQ,
                                            float4* WDQ, float* V) {
  stage_slabs<FA, FP, NT>(WA, reinterpret_cast<float*>(WAQ));
  stage_slabs<FP, FP, NT>(WB, reinterpret_cast<float*>(WBQ));
  if (HC) {
    stage_slabs<FA, FP, NT>(WC, reinterpret_cast<float*>(WCQ));
    stage_slabs<FA, FA, NT>(WD, reinterpret_cast<float*>(WDQ));
  }
  if (threadIdx.x < FP) {
    V[threadIdx.x] = gA[threadIdx.x];
    V[FP + threadIdx.x] = bA[threadIdx.x];
    V[2 * FP + threadIdx.x] = HC ? gC[threadIdx.x] : 0.f;
    V[3 * FP + threadIdx.x] = HC ? bC[threadIdx.x] : 0.f;
    V[4 * FP + threadIdx.x] = bB[threadIdx.x];
    if (threadIdx.x < FA) {
      V[5 * FP + threadIdx.x] = HC ? bWC[threadIdx.x] : 0.f;
      V[5 * FP + FA + threadIdx.x] = HC ? bD[threadIdx.x] : 0.f;
    }
  }
}

template <bool PREV>
__global__ __launch_bounds__(kThreadsT, GASFM_PT_FWD_T_MINW) void point_tail_fwd_t_kernel(
    const float* __restrict__ prev, const float* __restrict__ agg, int64_t N, const float* __restrict__ Wp,
    const float* __restrict__ bp, const float* __restrict__ gam, const float* __restrict__ bet, float eps,
    const float* __restrict__ Wm, const float* __restrict__ bm, float* __restrict__ out) {
  __shared__ float4 WpQ[FP * FA / 4], WmQ[FP * FP / 4];
  __shared__ float V[4 * FP];  // b_p gamma beta b_m
  const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
  const int64_t ntiles = (N + TR - 1) / TR;
  const int64_t gw = int64_t(blockIdx.x) * kWavesT + wave, nw = int64_t(gridDim.x) * kWavesT;
  f32x4 na[2], np[4];  // next tile's rows, requested before this tile's MFMA work
  auto fetch = [&](int64_t tt) {
    const int64_t r0 = tt * TR;
    const int nr = int(N - r0 < TR ? N - r0 : TR);
    slabs_load<FA>(agg, r0, nr, na, lane);
    if (PREV) slabs_load<FP>(prev, r0, nr, np, lane);
  };
  if (gw < ntiles) fetch(gw);  // the first tile's rows fly while the weights are staged
  stage_slabs<FP, FA, kThreadsT>(Wp, reinterpret_cast<float*>(WpQ));
  stage_slabs<FP, FP, kThreadsT>(Wm, reinterpret_cast<float*>(WmQ));
  if (threadIdx.x < FP) {
    V[threadIdx.x] = bp[threadIdx.x];
    V[FP + threadIdx.x] = gam[threadIdx.x];
    V[2 * FP + threadIdx.x] = bet[threadIdx.x];
    V[3 * FP + threadIdx.x] = bm[threadIdx.x];
  }
  __syncthreads();
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t row0 = t * TR;
    const int nrows = int(N - row0 < TR ? N - row0 : TR);
    if (GASFM_PT_FWD_T_LDSW) asm volatile("" ::: "memory");
    f32x4 ag[2] = {na[0], na[1]}, pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pv[u] = PREV ? np[u] : zero4();
    if (t + nw < ntiles) fetch(t + nw);
    f32x4 y[4];
    tail_tile_t(WpQ, WmQ, V, ag, pv, eps, lane, y);
    slabs_store<FP>(out, row0, nrows, y, lane);
  }
}

template <bool HC>
__global__ __launch_bounds__(kThreadsT, GASFM_PT_FWD_T_MINW) void point_hub_fwd_t_kernel(
    const float* __restrict__ X, int64_t N, float eps, const float* __restrict__ gA, const float* __restrict__ bA,
    const float* __restrict__ WA, float* __restrict__ SA, const float* __restrict__ WB,
    const float* __restrict__ bB, float* __restrict__ XL, const float* __restrict__ gC,
    const float* __restrict__ bC, const float* __restrict__ WC, const float* __restrict__ bWC,
    const float* __restrict__ WD, const float* __restrict__ bD, float* __restrict__ XR) {
  __shared__ float4 WAQ[FA * FP / 4], WBQ[FP * FP / 4], WCQ[HC ? FA * FP / 4 : 1], WDQ[HC ? FA * FA / 4 : 1];
  __shared__ float V[5 * FP + 2 * FA];  // gamma_A beta_A gamma_C beta_C b_B | b_C b_D
  const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
  const int64_t ntiles = (N + TR - 1) / TR;
  const int64_t gw = int64_t(blockIdx.x) * kWavesT + wave, nw = int64_t(gridDim.x) * kWavesT;
  f32x4 nx[4];
  auto fetch = [&](int64_t tt) {
    const int64_t r0 = tt * TR;
    slabs_load<FP>(X, r0, int(N - r0 < TR ? N - r0 : TR), nx, lane);
  };
  if (gw < ntiles) fetch(gw);  // the first tile's rows fly while the weights are staged
  hub_stage_t<HC, kThreadsT>(gA, bA, WA, WB, bB, gC, bC, WC, bWC, WD, bD, WAQ, WBQ, WCQ, WDQ, V);
  __syncthreads();
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t row0 = t * TR;
    const int nrows = int(N - row0 < TR ? N - row0 : TR);
    if (GASFM_PT_FWD_T_LDSW) asm volatile("" ::: "memory");
    f32x4 p[4] = {nx[0], nx[1], nx[2], nx[3]};
    if (t + nw < ntiles) fetch(t + nw);
    hub_tile_t<HC>(p, eps, WAQ, WBQ, WCQ, WDQ, V, lane, row0, nrows, SA, XL, XR);
  }
}

// The tail and the hub in ONE pass (round 6): p = tail(prev, agg) stays in registers between the two
// bodies (the tail's T-layout output is the hub's T-layout input), is stored once as the block's
// point features, and feeds the hub's consumers directly: no re-read of p, one launch and one weight
// staging fewer per block.  Same tile bodies as the two kernels: bitwise the same outputs.
template <bool PREV, bool HC, int NWV>
__global__ __launch_bounds__(NWV * kW) void point_tail_hub_fwd_t_kernel(
    const float* __restrict__ prev, const float* __restrict__ agg, int64_t N, const float* __restrict__ Wp,
    const float* __restrict__ bp, const float* __restrict__ gam, const float* __restrict__ bet, float eps,
    const float* __restrict__ Wm, const float* __restrict__ bm, float* __restrict__ out, float eps_h,
    const float* __restrict__ gA, const float* __restrict__ bA, const float* __restrict__ WA, float* __restrict__ SA,
    const float* __restrict__ WB, const float* __restrict__ bB, float* __restrict__ XL,
    const float* __restrict__ gC, const float* __restrict__ bC, const float* __restrict__ WC,
    const float* __restrict__ bWC, const float* __restrict__ WD, const float* __restrict__ bD,
    float* __restrict__ XR) {
  __shared__ float4 WpQ[FP * FA / 4], WmQ[FP * FP / 4];
  __shared__ float4 WAQ[FA * FP / 4], WBQ[FP * FP / 4], WCQ[HC ? FA * FP / 4 : 1], WDQ[HC ? FA * FA / 4 : 1];
  __shared__ float VT[4 * FP];               // b_p gamma beta b_m
  __shared__ float VH[5 * FP + 2 * FA];      // the hub's vectors (hub_stage_t)
  const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
  const int64_t ntiles = (N + TR - 1) / TR;
  const int64_t gw = int64_t(blockIdx.x) * NWV + wave, nw = int64_t(gridDim.x) * NWV;
  f32x4 na[2], np[4];
  auto fetch = [&](int64_t tt) {
    const int64_t r0 = tt * TR;
    const int nr = int(N - r0 < TR ? N - r0 : TR);
    slabs_load<FA>(agg, r0, nr, na, lane);
    if (PREV) slabs_load<FP>(prev, r0, nr, np, lane);
  };
  if (gw < ntiles) fetch(gw);
  stage_slabs<FP, FA, NWV * kW>(Wp, reinterpret_cast<float*>(WpQ));
  stage_slabs<FP, FP, NWV * kW>(Wm, reinterpret_cast<float*>(WmQ));
  if (threadIdx.x < FP) {
    VT[threadIdx.x] = bp[threadIdx.x];
    VT[FP + threadIdx.x] = gam[threadIdx.x];
    VT[2 * FP + threadIdx.x] = bet[threadIdx.x];
    VT[3 * FP + threadIdx.x] = bm[threadIdx.x];
  }
  hub_stage_t<HC, NWV * kW>(gA, bA, WA, WB, bB, gC, bC, WC, bWC, WD, bD, WAQ, WBQ, WCQ, WDQ, VH);
  __syncthreads();
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t row0 = t * TR;
    const int nrows = int(N - row0 < TR ? N - row0 : TR);
    if (GASFM_PT_FWD_T_LDSW) asm volatile("" ::: "memory");
    f32x4 ag[2] = {na[0], na[1]}, pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pv[u] = PREV ? np[u] : zero4();
    if (t + nw < ntiles) fetch(t + nw);
    f32x4 p[4];
    tail_tile_t(WpQ, WmQ, VT, ag, pv, eps, lane, p);
    slabs_store<FP>(out, row0, nrows, p, lane);
    hub_tile_t<HC>(p, eps_h, WAQ, WBQ, WCQ, WDQ, VH, lane, row0, nrows, SA, XL, XR);
  }
}

// ----------------------------------------------------------------------------- backward, register-resident
// The backward needs every row tensor in two register layouts:
//   T (slab) layout  lane (g, c), f32x4 v[u]:  V[row c][16 u + 4 g + j]      (k = features along g)
//   C layout         lane (g, c), f32x4 v[ft]: V[row 4 g + r][16 ft + c]     (k = rows along g)
// A product over FEATURES (Y = X W^T) takes X in T layout; with X as the A operand the result
// lands in C layout (layer_c), with X as the B operand in T layout (layer_t).  A weight gradient
// (dW = dY^T X, K = rows) takes BOTH operands in C layout with the row index in the order 4 g + s
// at step s: no LDS at all.  So the loaded tensors are read in the layouts their consumers want
// (T: 16-B loads of 64-B row chunks; C: 4-B loads, 64 contiguous bytes per row per instruction --
// the second layout of a tensor comes from L1 / L2), the computed ones come out of the products
// in the layout needed, and only dx, consumed by both kinds of product, goes through a per-wave
// LDS transpose (16 x 64).  LDS holds the weight slabs and that transpose tile (~49 KB per
// 4-wave workgroup), and no MFMA operand of a row tile is read from LDS.
// 1: scheduling barriers between the phases of a tile (each phase's MFMAs and VALU work stay
// together); 0: none (the compiler may interleave a phase's VALU with the next phase's MFMAs)
#ifndef GASFM_PT_SCHED
#define GASFM_PT_SCHED 1
#endif
#if GASFM_PT_SCHED
#define PT_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#else
#define PT_SCHED_BARRIER() ((void)0)
#endif
// 1 wave per SIMD (~210 VGPRs + 116 AGPRs) with the next tile's rows requested one tile ahead;
// 2 waves per SIMD spills (256 VGPRs, 52 spilled): 110 vs 86 us at n = 200k without the prefetch
#ifndef GASFM_PT_BWD_R_MINW
#define GASFM_PT_BWD_R_MINW 1
#endif
constexpr int kWavesR = 4, kThreadsR = kWavesR * kW;
constexpr int LDX = FP + 4;  // transpose tile row stride: the C-layout writes of the 4 lane groups hit 4 bank quarters

// float4 slabs of W^T for W [O x K] (out index k, K index o): Q[((k/16) (O/16) + o/16) 64 + 16 ((o%16)/4)
// + k%16][o%4] = W[o][k], i.e. stage_slabs of the transpose (W is read in its own row-major order)
template <int O, int K, int NT>
__device__ __forceinline__ void stage_slabs_tr(const float* __restrict__ W, float* Q) {
  Stage<O * K, NT> s;
  s.load([&](int q) { return W[q]; });
  s.store([&](int q, float v) {
    const int o = q / K, k = q % K;
    Q[(((k / 16) * (O / 16) + o / 16) * 64 + ((o % 16) / 4) * 16 + k % 16) * 4 + o % 4] = v;
  });
}

// acc[ot] += X W^T with X (T-layout k-slabs) as the A operand: acc[ot][r] = Y[row 4 g + r][16 ot + c]
template <int OT, int KU>
__device__ __forceinline__ void layer_c(const float4* __restrict__ Q, const f32x4 (&xk)[KU], f32x4 (&acc)[OT],
                                        int lane) {
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    float4 w[OT];
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) w[ot] = Q[(ot * KU + u) * 64 + lane];
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(xk[u][0], w[ot].x, acc[ot]);
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(xk[u][1], w[ot].y, acc[ot]);
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(xk[u][2], w[ot].z, acc[ot]);
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma16(xk[u][3], w[ot].w, acc[ot]);
  }
}

// C-layout rows: v[ft][r] = X[row0 + 4 g + r][16 ft + c]; rows >= nrows read a valid row (cl_mask zeroes
// them where the values are consumed: a select right after the load would wait for it, so a load
// issued a tile ahead must not be masked in place)
template <int W>
__device__ __forceinline__ void cl_load(const float* __restrict__ X, int64_t row0, int nrows, f32x4 (&v)[W / 16],
                                        int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = 4 * g + r;
    const float* p = X + (row0 + (rr < nrows ? rr : 0)) * W + c;
#pragma unroll
    for (int ft = 0; ft < W / 16; ++ft) v[ft][r] = p[16 * ft];
  }
}
template <int NF>
__device__ __forceinline__ void cl_mask(f32x4 (&v)[NF], int nrows, int g) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int ft = 0; ft < NF; ++ft) v[ft][r] = 4 * g + r < nrows ? v[ft][r] : 0.f;
}

// C layout -> T layout of a 16 x 64 tile through the wave's LDS tile X (stride LDX)
__device__ __forceinline__ void c_to_t64(const f32x4 (&v)[4], float* X, f32x4 (&o)[4], int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ft = 0; ft < 4; ++ft)
#pragma unroll
    for (int r = 0; r < 4; ++r) X[(4 * g + r) * LDX + 16 * ft + c] = v[ft][r];
  // one wave's LDS instructions execute in order: a compiler barrier suffices (a wavefront fence
  // would also wait for the global loads in flight)
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float4 t = *reinterpret_cast<const float4*>(X + c * LDX + 16 * u + 4 * g);
    o[u] = f32x4{t.x, t.y, t.z, t.w};
  }
}

// LayerNorm statistics of the C-layout rows 4 g + r (64 features: 4 regs x 16 lanes)
__device__ __forceinline__ void cl_stats(const f32x4 (&x)[4], float eps, float (&mean)[4], float (&rstd)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mean[r] = sum16((x[0][r] + x[1][r]) + (x[2][r] + x[3][r])) * (1.f / FP);
    float q = 0.f;
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) q = fmaf(x[ot][r] - mean[r], x[ot][r] - mean[r], q);
    rstd[r] = rsq_normal(sum16(q) * (1.f / FP) + eps);
  }
}

// LayerNorm + ReLU backward of the C-layout rows (xh: normalised x, dh: gradient of relu(xh g + b));
// rows >= nrows give 0.  Accumulates dgamma / dbeta per lane feature 16 ot + c.  Packed fp32 math
// (round 5): features (16 ot + c, 16 (ot + 1) + c) of a row as one pair per v_pk_* instruction.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void cl_ln_relu_bwd(const f32x4 (&xh)[4], const f32x4 (&dh)[4], const float (&gm)[4],
                                               const float (&bt)[4], const float (&rstd)[4], int nrows, int g,
                                               float (&dg)[4], float (&db)[4], f32x4 (&dx)[4]) {
  f32x2 dg2[2] = {{dg[0], dg[1]}, {dg[2], dg[3]}}, db2[2] = {{db[0], db[1]}, {db[2], db[3]}};
  const f32x2 gm2[2] = {{gm[0], gm[1]}, {gm[2], gm[3]}}, bt2[2] = {{bt[0], bt[1]}, {bt[2], bt[3]}};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool live = 4 * g + r < nrows;
    f32x2 s1p = {0.f, 0.f}, s2p = {0.f, 0.f}, gv[2], x2[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      x2[h] = f32x2{xh[2 * h][r], xh[2 * h + 1][r]};
      const f32x2 pre = __builtin_elementwise_fma(x2[h], gm2[h], bt2[h]);
      const f32x2 dy = {(live && pre.x > 0.f) ? dh[2 * h][r] : 0.f, (live && pre.y > 0.f) ? dh[2 * h + 1][r] : 0.f};
      dg2[h] = __builtin_elementwise_fma(dy, x2[h], dg2[h]);
      db2[h] += dy;
      gv[h] = dy * gm2[h];
      s1p += gv[h];
      s2p = __builtin_elementwise_fma(gv[h], x2[h], s2p);
    }
    const float s1 = sum16(s1p.x + s1p.y) * (1.f / FP);
    const float s2 = sum16(s2p.x + s2p.y) * (1.f / FP);
    const f32x2 s1v = {s1, s1}, ms2 = {-s2, -s2}, r2 = {rstd[r], rstd[r]};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x2 t = __builtin_elementwise_fma(x2[h], ms2, gv[h] - s1v) * r2;  // rstd ((gv - s1) - xh s2)
      dx[2 * h][r] = t.x;
      dx[2 * h + 1][r] = t.y;
    }
  }
  dg[0] = dg2[0].x, dg[1] = dg2[0].y, dg[2] = dg2[1].x, dg[3] = dg2[1].y;
  db[0] = db2[0].x, db[1] = db2[0].y, db[2] = db2[1].x, db[3] = db2[1].y;
}

// dx = dout + LN_bwd(mask * (dout W_m)) (== d prev), dagg = dx W_p; partial row per workgroup in the
// TAIL_PART layout.  Per tile: x = agg W_p^T (+ b_p + prev) in C layout
// (agg T-layout as A), h = relu(LN x); dh = dout W_m in C layout (dout T-layout as A); dx (C);
// dW_m += dout^T h and dW_p += dx^T agg from C-layout registers; dx -> T layout (LDS), stored;
// dagg = dx W_p in T layout (dx as B), stored.
template <bool PREV>
__global__ __launch_bounds__(kThreadsR, GASFM_PT_BWD_R_MINW) void point_tail_bwd_r_kernel(
    const float* __restrict__ dout, const float* __restrict__ prev, const float* __restrict__ agg, int64_t N,
    const float* __restrict__ Wp, const float* __restrict__ bp, const float* __restrict__ gam,
    const float* __restrict__ bet, float eps, const float* __restrict__ Wm, float* __restrict__ dx,
    float* __restrict__ dagg, float* __restrict__ part) {
  constexpr int NRED = 64 + 32 + 16;
  constexpr int OQ = 0, OQT = FP * FA, OMT = 2 * FP * FA, OX = OMT + FP * FP, NLDS = OX + kWavesR * TR * LDX;
  __shared__ __attribute__((aligned(16))) float lds[NLDS];
  float4* WpQ = reinterpret_cast<float4*>(lds + OQ);    // slabs of W_p   (out o, k j)
  float4* WpTQ = reinterpret_cast<float4*>(lds + OQT);  // slabs of W_p^T (out j, k o)
  float4* WmTQ = reinterpret_cast<float4*>(lds + OMT);  // slabs of W_m^T (out i, k o)
  const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
  const int c = lane & 15, g = lane >> 4;
  stage_slabs<FP, FA, kThreadsR>(Wp, lds + OQ);
  stage_slabs_tr<FP, FA, kThreadsR>(Wp, lds + OQT);
  stage_slabs_tr<FP, FP, kThreadsR>(Wm, lds + OMT);
  float bpC[4], gmC[4], btC[4];
#pragma unroll
  for (int ot = 0; ot < 4; ++ot) {
    bpC[ot] = bp[16 * ot + c];
    gmC[ot] = gam[16 * ot + c];
    btC[ot] = bet[16 * ot + c];
  }
  __syncthreads();
  float* X = lds + OX + wave * TR * LDX;
  f32x4 dWm[4][4], dWp[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dWm[mt][nt] = zero4();
    dWp[mt][0] = dWp[mt][1] = zero4();
  }
  float dbm[4] = {0.f, 0.f, 0.f, 0.f}, dbp[4] = {0.f, 0.f, 0.f, 0.f};
  float dg[4] = {0.f, 0.f, 0.f, 0.f}, dbt[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (N + TR - 1) / TR;
  const int64_t gw = int64_t(blockIdx.x) * kWavesR + wave, nw = int64_t(gridDim.x) * kWavesR;
  // every row of tile t + nw is requested before tile t's work (one tile of loads in flight)
  f32x4 n_agT[2], n_dT[4], n_pC[4], n_dC[4], n_agC[2];
  auto fetch = [&](int64_t tt) {
    const int64_t r0 = tt * TR;
    const int nr = int(N - r0 < TR ? N - r0 : TR);
    slabs_load<FA>(agg, r0, nr, n_agT, lane);
    if (PREV) cl_load<FP>(prev, r0, nr, n_pC, lane);
    slabs_load<FP>(dout, r0, nr, n_dT, lane);
    cl_load<FP>(dout, r0, nr, n_dC, lane);
    cl_load<FA>(agg, r0, nr, n_agC, lane);
  };
  if (gw < ntiles) fetch(gw);
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t row0 = t * TR;
    const int nrows = int(N - row0 < TR ? N - row0 : TR);
    asm volatile("" ::: "memory");  // weight slabs re-read from LDS per tile (not hoisted into VGPRs)
    f32x4 agT[2] = {n_agT[0], n_agT[1]}, dT[4], x[4], dC[4], agC[2] = {n_agC[0], n_agC[1]};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dT[u] = n_dT[u];
      dC[u] = n_dC[u];
      x[u] = PREV ? n_pC[u] : zero4();
    }
    // unconditional (the last tile re-reads itself): a load under a branch makes the loop header
    // wait for every outstanding load
    fetch(t + nw < ntiles ? t + nw : t);
    cl_mask(dC, nrows, g);
    cl_mask(agC, nrows, g);
    if (PREV) cl_mask(x, nrows, g);
    // phase 1: x (C layout) and its LayerNorm
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) x[ot] += bpC[ot];
    layer_c<4, 2>(WpQ, agT, x, lane);
    float mean[4], rstd[4];
    cl_stats(x, eps, mean, rstd);
#pragma unroll
    for (int ot = 0; ot < 4; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[ot][r] = (x[ot][r] - mean[r]) * rstd[r];  // x_hat from here on
    PT_SCHED_BARRIER();
    // phase 2: dh = dout W_m (C layout)
    f32x4 dh[4] = {zero4(), zero4(), zero4(), zero4()};
    layer_c<4, 4>(WmTQ, dT, dh, lane);
    PT_SCHED_BARRIER();
    // phase 3: LayerNorm backward -> dx (C layout), bias sums
    f32x4 dxc[4];
    cl_ln_relu_bwd(x, dh, gmC, btC, rstd, nrows, g, dg, dbt, dxc);
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
      dxc[ot] += dC[ot];  // rows >= nrows: 0 + 0
      dbm[ot] += (dC[ot][0] + dC[ot][1]) + (dC[ot][2] + dC[ot][3]);
      dbp[ot] += (dxc[ot][0] + dxc[ot][1]) + (dxc[ot][2] + dxc[ot][3]);
    }
    PT_SCHED_BARRIER();
    // phase 4: weight gradients over the tile's rows (step s: row 4 g + s; rows past nrows: dout,
    // dx are 0); h = relu(x_hat g + b) recomputed here (not live through phases 2-3)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float hs[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) hs[nt] = fmaxf(fmaf(x[nt][s], gmC[nt], btC[nt]), 0.f);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) dWm[mt][nt] = mfma16(dC[mt][s], hs[nt], dWm[mt][nt]);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) dWp[mt][nt] = mfma16(dxc[mt][s], agC[nt][s], dWp[mt][nt]);
      }
    }
    PT_SCHED_BARRIER();
    f32x4 dxT[4];
    c_to_t64(dxc, X, dxT, lane);
    slabs_store<FP>(dx, row0, nrows, dxT, lane);
    f32x4 da[2] = {zero4(), zero4()};
    layer_t<2, 4>(WpTQ, dxT, da, lane);
    slabs_store<FA>(dagg, row0, nrows, da, lane);
    __builtin_amdgcn_wave_barrier();  // this tile's transpose reads before the next tile's writes
    asm volatile("" ::: "memory");
  }
  float v[NRED];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) v[(mt * 4 + nt) * 4 + r] = dWm[mt][nt][r];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) v[64 + (mt * 2 + nt) * 4 + r] = dWp[mt][nt][r];
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[96 + k] = dbm[k];
    v[100 + k] = dbp[k];
    v[104 + k] = dg[k];
    v[108 + k] = dbt[k];
  }
  wg_reduce_ordered<NRED, kWavesR, NLDS>(v, lds, wave, lane);
  if (wave == 0) {
    float* out = part + int64_t(blockIdx.x) * TAIL_PART;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = mt * 16 + 4 * g + r;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) out[o * FP + nt * 16 + c] = v[(mt * 4 + nt) * 4 + r];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) out[FP * FP + o * FA + nt * 16 + c] = v[64 + (mt * 2 + nt) * 4 + r];
      }
    float tt[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) tt[k] = sum_groups(v[96 + k]);
    if (g == 0) {
      float* o = out + FP * FP + FP * FA;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) o[q * FP + k * 16 + c] = tt[q * 4 + k];
    }
  }
}

// The whole hub backward in ONE register-resident pass.  Per tile:
//   t   = W_C relu(LN_C p) + b_C                     C layout (relu(LN_C p) T-layout as A)
//   dt  = dXR W_D                                    C layout (weight / bias gradients) and T layout
//                                                    (the A operand of dt W_C), both from dXR (T)
//   dp  = dXL W_B + (LN_A_bwd(mask (dSA W_A)) + (LN_C_bwd(mask (dt W_C)) + dRes))   C layout
//   dW_C += dt^T relu(LN_C p), dW_D += dXR^T t, dW_A += dSA^T relu(LN_A p), dW_B += dXL^T p
// The rows are requested one tile ahead in the T layout (the products over features); the
// C layout the weight gradients and the LayerNorm backward need is read back from a per-wave
// LDS copy of the tile (one write per row chunk, read just before use: the 256 architected VGPRs
// of a wave could not also hold a second, C-layout load of every tile).  The LayerNorm statistics
// come from the T rows and reach the C layout by lane shuffles.  dRes is read in the C layout at
// the top of its tile (before the next tile's requests), dp stored from the C layout.  Two
// partial rows per workgroup: the A / B gradients in the HA_* layout into part_a, the C / D ones
// in the HC_* layout into part_c.  Algorithmic bytes per row:
// p 256 + dSA 128 + dXL 256 + dXR 128 + dRes 256 + dp 256 = 1,280.
#ifndef GASFM_PT_HUB_BWD_R_MINW
#define GASFM_PT_HUB_BWD_R_MINW 1
#endif
constexpr int LDA = FA + 4;  // 32-wide LDS tile row stride (4 lane groups -> 4 bank quarters)

// C-layout rows out (rows >= nrows not written)
template <int W>
__device__ __forceinline__ void cl_store(float* X, int64_t row0, int nrows, const f32x4 (&v)[W / 16], int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (4 * g + r >= nrows) continue;
    float* p = X + (row0 + 4 * g + r) * W + c;
#pragma unroll
    for (int ft = 0; ft < W / 16; ++ft) p[16 * ft] = v[ft][r];
  }
}

// T-layout rows (row c, features 16 u + 4 g + j) into the wave's LDS tile (row stride LD)
template <int W, int LD>
__device__ __forceinline__ void t_to_lds(const f32x4 (&v)[W / 16], float* X, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int u = 0; u < W / 16; ++u)
    *reinterpret_cast<float4*>(X + c * LD + 16 * u + 4 * g) = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
}

template <bool HR>
__global__ __launch_bounds__(kThreadsR, GASFM_PT_HUB_BWD_R_MINW) void point_hub_bwd_r_kernel(
    const float* __restrict__ X, int64_t N, float eps, const float* __restrict__ gA, const float* __restrict__ bA,
    const float* __restrict__ WA, const float* __restrict__ WB, const float* __restrict__ gC,
    const float* __restrict__ bC, const float* __restrict__ WC, const float* __restrict__ bWC,
    const float* __restrict__ WD, const float* __restrict__ dSA, const float* __restrict__ dXL,
    const float* __restrict__ dXR, const float* dRes, float* dX, float* __restrict__ part_a,
    float* __restrict__ part_c) {
  constexpr int OC = 0, ODT = OC + FA * FP, OCT = ODT + FA * FA, OAT = OCT + FA * FP, OBT = OAT + FA * FP,
                OV = OBT + FP * FP, OT = OV + 6 * FP;
  constexpr int TW = TR * (2 * LDX + 3 * LDA);  // per wave: p, dXL (64 wide), dSA, dXR, dt (32 wide)
  constexpr int NLDS = OT + kWavesR * TW;
  constexpr int NRED = 144 + 24;
  __shared__ __attribute__((aligned(16))) float lds[NLDS];
  const float4* WCQ = reinterpret_cast<const float4*>(lds + OC);     // slabs of W_C   (out t,  k p)
  const float4* WDTQ = reinterpret_cast<const float4*>(lds + ODT);   // slabs of W_D^T (out t,  k xr)
  const float4* WCTQ = reinterpret_cast<const float4*>(lds + OCT);   // slabs of W_C^T (out p,  k t)
  const float4* WATQ = reinterpret_cast<const float4*>(lds + OAT);   // slabs of W_A^T (out p,  k sa)
  const float4* WBTQ = reinterpret_cast<const float4*>(lds + OBT);   // slabs of W_B^T (out p,  k xl)
  const float* V = lds + OV;  // gamma_C beta_C gamma_A beta_A b_C(32) (pad)
  const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
  const int c = lane & 15, g = lane >> 4;
  float* Tp = lds + OT + wave * TW;
  float* Tl = Tp + TR * LDX;
  float* Ts = Tl + TR * LDX;
  float* Tr = Ts + TR * LDA;
  float* Td = Tr + TR * LDA;  // dt's C -> T transpose
  const int64_t ntiles = (N + TR - 1) / TR;
  const int64_t gw = int64_t(blockIdx.x) * kWavesR + wave, nw = int64_t(gridDim.x) * kWavesR;
  f32x4 n_pT[4], n_rT[2], n_sT[2], n_lT[4];  // the next tile's T-layout rows
  auto fetch = [&](int64_t tt) {
    const int64_t r0 = tt * TR;
    const int nr = int(N - r0 < TR ? N - r0 : TR);
    slabs_load<FP>(X, r0, nr, n_pT, lane);
    slabs_load<FA>(dXR, r0, nr, n_rT, lane);
    slabs_load<FA>(dSA, r0, nr, n_sT, lane);
    slabs_load<FP>(dXL, r0, nr, n_lT, lane);
  };
  if (gw < ntiles) fetch(gw);  // the first tile's rows fly while the weights are staged
  stage_slabs<FA, FP, kThreadsR>(WC, lds + OC);
  stage_slabs_tr<FA, FA, kThreadsR>(WD, lds + ODT);
  stage_slabs_tr<FA, FP, kThreadsR>(WC, lds + OCT);
  stage_slabs_tr<FA, FP, kThreadsR>(WA, lds + OAT);
  stage_slabs_tr<FP, FP, kThreadsR>(WB, lds + OBT);
  if (threadIdx.x < FP) {
    lds[OV + threadIdx.x] = gC[threadIdx.x];
    lds[OV + FP + threadIdx.x] = bC[threadIdx.x];
    lds[OV + 2 * FP + threadIdx.x] = gA[threadIdx.x];
    lds[OV + 3 * FP + threadIdx.x] = bA[threadIdx.x];
    if (threadIdx.x < FA) lds[OV + 4 * FP + threadIdx.x] = bWC[threadIdx.x];
  }
  __syncthreads();
  f32x4 dWA[2][4], dWB[4][4], dWC[2][4], dWD[2][2];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    dWA[0][nt] = dWA[1][nt] = dWC[0][nt] = dWC[1][nt] = zero4();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) dWB[mt][nt] = zero4();
  }
  dWD[0][0] = dWD[0][1] = dWD[1][0] = dWD[1][1] = zero4();
  float dbB[4] = {0.f, 0.f, 0.f, 0.f}, dgA[4] = {0.f, 0.f, 0.f, 0.f}, dbA[4] = {0.f, 0.f, 0.f, 0.f};
  float dgC[4] = {0.f, 0.f, 0.f, 0.f}, dbCl[4] = {0.f, 0.f, 0.f, 0.f}, dbC[2] = {0.f, 0.f}, dbD[2] = {0.f, 0.f};
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t row0 = t * TR;
    const int nrows = int(N - row0 < TR ? N - row0 : TR);
    asm volatile("" ::: "memory");  // weight slabs re-read from LDS per tile (not hoisted into VGPRs)
    f32x4 pT[4], rT[2] = {n_rT[0], n_rT[1]}, sT[2] = {n_sT[0], n_sT[1]}, lT[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      pT[u] = n_pT[u];
      lT[u] = n_lT[u];
    }
    // dRes of this tile, then the next tile's rows (unconditional: the last tile re-reads itself;
    // a load under a branch makes the loop header wait for every outstanding load)
    f32x4 acc[4];
    if (HR) cl_load<FP>(dRes, row0, nrows, acc, lane);
    fetch(t + nw < ntiles ? t + nw : t);
    t_to_lds<FP, LDX>(pT, Tp, lane);
    t_to_lds<FP, LDX>(lT, Tl, lane);
    t_to_lds<FA, LDA>(sT, Ts, lane);
    t_to_lds<FA, LDA>(rT, Tr, lane);
    // phase 1: statistics of the row c (T layout), t = W_C relu(LN_C p) + b_C (C layout)
    float mean, rstd;
    slab_stats(pT, eps, mean, rstd);
    f32x4 tC[2] = {zero4(), zero4()};
    {
      f32x4 pc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4 gm = vec_at(V, u, g), bt = vec_at(V + FP, u, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) pc[u][j] = fmaxf(fmaf((pT[u][j] - mean) * rstd, gm[j], bt[j]), 0.f);
      }
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) tC[ft] += V[4 * FP + 16 * ft + c];
      layer_c<2, 4>(WCQ, pc, tC, lane);
    }
    // row 4 g + r's statistics, computed on lane c = 4 g + r: through the padding columns 64, 65 of
    // the wave's p tile (row c; every lane group writes the same values), not 8 lane shuffles
    *reinterpret_cast<float2*>(Tp + c * LDX + FP) = make_float2(mean, rstd);
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    float meanC[4], rstdC[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float2 st = *reinterpret_cast<const float2*>(Tp + (4 * g + r) * LDX + FP);
      meanC[r] = st.x;
      rstdC[r] = st.y;
    }
    PT_SCHED_BARRIER();
    // phase 2: dt (C and T layouts), dt W_C, LN_C backward onto dRes
    f32x4 dtC[2] = {zero4(), zero4()};
    f32x4 xh[4];
#pragma unroll
    for (int ot = 0; ot < 4; ++ot)
#pragma unroll
      for (int r = 0; r < 4; ++r) xh[ot][r] = (Tp[(4 * g + r) * LDX + 16 * ot + c] - meanC[r]) * rstdC[r];
    {
      f32x4 dtT[2] = {zero4(), zero4()}, dp[4] = {zero4(), zero4(), zero4(), zero4()}, dq[4];
      layer_c<2, 2>(WDTQ, rT, dtC, lane);
      // dt's T layout through the wave's LDS tile, not a second product (16 MFMA): the same
      // products summed in the same k order, so bitwise the layer_t result (round 5)
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) Td[(4 * g + r) * LDA + 16 * ft + c] = dtC[ft][r];
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float4 t4 = *reinterpret_cast<const float4*>(Td + c * LDA + 16 * u + 4 * g);
        dtT[u] = f32x4{t4.x, t4.y, t4.z, t4.w};
      }
      PT_SCHED_BARRIER();
      layer_c<4, 2>(WCTQ, dtT, dp, lane);
      float gm[4], bt[4];
#pragma unroll
      for (int ot = 0; ot < 4; ++ot) {
        gm[ot] = V[16 * ot + c];
        bt[ot] = V[FP + 16 * ot + c];
      }
      cl_ln_relu_bwd(xh, dp, gm, bt, rstdC, nrows, g, dgC, dbCl, dq);
#pragma unroll
      for (int ot = 0; ot < 4; ++ot) acc[ot] = HR ? dq[ot] + acc[ot] : dq[ot];
    }
    PT_SCHED_BARRIER();
    // phase 3: dSA W_A, LN_A backward; dXL W_B accumulated on top; dp stored
    {
      f32x4 dp[4] = {zero4(), zero4(), zero4(), zero4()}, da[4];
      layer_c<4, 2>(WATQ, sT, dp, lane);
      float gm[4], bt[4];
#pragma unroll
      for (int ot = 0; ot < 4; ++ot) {
        gm[ot] = V[2 * FP + 16 * ot + c];
        bt[ot] = V[3 * FP + 16 * ot + c];
      }
      cl_ln_relu_bwd(xh, dp, gm, bt, rstdC, nrows, g, dgA, dbA, da);
#pragma unroll
      for (int ot = 0; ot < 4; ++ot) acc[ot] = da[ot] + acc[ot];
    }
    PT_SCHED_BARRIER();
    layer_c<4, 4>(WBTQ, lT, acc, lane);
    cl_store<FP>(dX, row0, nrows, acc, lane);
    PT_SCHED_BARRIER();
    // phase 4: weight gradients over the tile's rows (step s: row 4 g + s, C-layout operands read
    // from the LDS copies; dead rows: the A operands are masked to 0), bias sums
    cl_mask(dtC, nrows, g);
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) dbC[ft] += (dtC[ft][0] + dtC[ft][1]) + (dtC[ft][2] + dtC[ft][3]);
    float gAv[4], bAv[4], gCv[4], bCv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      gCv[nt] = V[16 * nt + c];
      bCv[nt] = V[FP + 16 * nt + c];
      gAv[nt] = V[2 * FP + 16 * nt + c];
      bAv[nt] = V[3 * FP + 16 * nt + c];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = 4 * g + s;
      const bool live = row < nrows;
      float pa[4], pc[4], pr[4], la[4], sa[2], ra[2];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        pa[nt] = fmaxf(fmaf(xh[nt][s], gAv[nt], bAv[nt]), 0.f);
        pc[nt] = fmaxf(fmaf(xh[nt][s], gCv[nt], bCv[nt]), 0.f);
        pr[nt] = Tp[row * LDX + 16 * nt + c];
        la[nt] = live ? Tl[row * LDX + 16 * nt + c] : 0.f;
        dbB[nt] += la[nt];
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        sa[mt] = live ? Ts[row * LDA + 16 * mt + c] : 0.f;
        ra[mt] = live ? Tr[row * LDA + 16 * mt + c] : 0.f;
        dbD[mt] += ra[mt];
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          dWA[mt][nt] = mfma16(sa[mt], pa[nt], dWA[mt][nt]);
          dWC[mt][nt] = mfma16(dtC[mt][s], pc[nt], dWC[mt][nt]);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) dWD[mt][nt] = mfma16(ra[mt], tC[nt][s], dWD[mt][nt]);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) dWB[mt][nt] = mfma16(la[mt], pr[nt], dWB[mt][nt]);
    }
    __builtin_amdgcn_wave_barrier();  // this tile's LDS reads before the next tile's writes
    asm volatile("" ::: "memory");
  }
  float v[NRED];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        v[(mt * 4 + nt) * 4 + r] = dWA[mt][nt][r];
        v[96 + (mt * 4 + nt) * 4 + r] = dWC[mt][nt][r];
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) v[32 + (mt * 4 + nt) * 4 + r] = dWB[mt][nt][r];
    }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) v[128 + (mt * 2 + nt) * 4 + r] = dWD[mt][nt][r];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[144 + k] = dbB[k];
    v[148 + k] = dgA[k];
    v[152 + k] = dbA[k];
    v[156 + k] = dgC[k];
    v[160 + k] = dbCl[k];
  }
  v[164] = dbC[0];
  v[165] = dbC[1];
  v[166] = dbD[0];
  v[167] = dbD[1];
  wg_reduce_ordered<NRED, kWavesR, NLDS>(v, lds, wave, lane);
  if (wave == 0) {
    float* oa = part_a + int64_t(blockIdx.x) * HA_PART;
    float* oc = part_c + int64_t(blockIdx.x) * HC_PART;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const int o = mt * 16 + 4 * g + r;
          oa[HA_WA + o * FP + nt * 16 + c] = v[(mt * 4 + nt) * 4 + r];
          oc[HC_WC + o * FP + nt * 16 + c] = v[96 + (mt * 4 + nt) * 4 + r];
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) oa[HA_WB + (mt * 16 + 4 * g + r) * FP + nt * 16 + c] = v[32 + (mt * 4 + nt) * 4 + r];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) oc[HC_WD + (mt * 16 + 4 * g + r) * FA + nt * 16 + c] = v[128 + (mt * 2 + nt) * 4 + r];
    float tt[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) tt[k] = sum_groups(v[144 + k]);
    if (g == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        oa[HA_BB + k * 16 + c] = tt[k];
        oa[HA_GA + k * 16 + c] = tt[4 + k];
        oa[HA_BA + k * 16 + c] = tt[8 + k];
        oc[HC_GC + k * 16 + c] = tt[12 + k];
        oc[HC_BCL + k * 16 + c] = tt[16 + k];
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        oc[HC_BC + k * 16 + c] = tt[20 + k];
        oc[HC_BD + k * 16 + c] = tt[22 + k];
      }
    }
  }
}

int64_t tiles_of(int64_t N) { return (N + TR - 1) / TR; }

template <class K>
int gridT(K kernel, int64_t N) {
  return resident_grid(reinterpret_cast<const void*>(kernel), kThreadsT, 0, tiles_of(N), kWavesT);
}
template <class K>
int gridR(K kernel, int64_t N) {
  return resident_grid(reinterpret_cast<const void*>(kernel), kThreadsR, 0, tiles_of(N), kWavesR);
}
int tail_bwd_grid(int64_t N, bool has_prev) {
  return has_prev ? gridR(&point_tail_bwd_r_kernel<true>, N) : gridR(&point_tail_bwd_r_kernel<false>, N);
}
// the hub backward: both partial buffers have its grid's rows, whether dRes is given or not
int hub_r_grid(int64_t N) { return gridR(&point_hub_bwd_r_kernel<true>, N); }

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_point_tail_part_shape(int64_t N, int32_t has_prev, int32_t* cols) {
  if (cols) *cols = TAIL_PART;
  return N > 0 ? tail_bwd_grid(N, has_prev != 0) : 0;
}

// has_res is ignored: the rows do not depend on whether dRes is given
extern "C" int32_t gasfm_point_hub_part_shape(int64_t N, int32_t which, int32_t /*has_res*/, int32_t* cols) {
  if (cols) *cols = which ? HC_PART : HA_PART;
  return N > 0 ? hub_r_grid(N) : 0;
}

extern "C" int gasfm_point_tail_fwd(const float* prev, const float* agg, int64_t N, const float* Wp, const float* bp,
                                    const float* ln_w, const float* ln_b, float eps, const float* Wm,
                                    const float* bm, float* out, void* stream) {
  GASFM_REQUIRE(N >= 0, "gasfm_point_tail_fwd: N < 0");
  if (N == 0) return GASFM_OK;
  GASFM_REQUIRE(agg && Wp && bp && ln_w && ln_b && Wm && bm && out, "gasfm_point_tail_fwd: null pointer");
  GASFM_REQUIRE(aligned16(agg) && (!prev || aligned16(prev)), "gasfm_point_tail_fwd: alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (prev)
    hipLaunchKernelGGL(point_tail_fwd_t_kernel<true>, dim3(gridT(&point_tail_fwd_t_kernel<true>, N)),
                       dim3(kThreadsT), 0, st, prev, agg, N, Wp, bp, ln_w, ln_b, eps, Wm, bm, out);
  else
    hipLaunchKernelGGL(point_tail_fwd_t_kernel<false>, dim3(gridT(&point_tail_fwd_t_kernel<false>, N)),
                       dim3(kThreadsT), 0, st, prev, agg, N, Wp, bp, ln_w, ln_b, eps, Wm, bm, out);
  return launch_status("gasfm_point_tail_fwd");
}

extern "C" int gasfm_point_tail_bwd(const float* dout, const float* prev, const float* agg, int64_t N,
                                    const float* Wp, const float* bp, const float* ln_w, const float* ln_b,
                                    float eps, const float* Wm, float* dx, float* dagg, float* part, void* stream) {
  GASFM_REQUIRE(N >= 0, "gasfm_point_tail_bwd: N < 0");
  if (N == 0) return GASFM_OK;
  GASFM_REQUIRE(dout && agg && Wp && bp && ln_w && ln_b && Wm && dx && dagg && part,
                "gasfm_point_tail_bwd: null pointer");
  GASFM_REQUIRE(aligned16(dout) && aligned16(agg), "gasfm_point_tail_bwd: alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int gsz = tail_bwd_grid(N, prev != nullptr);
  if (prev)
    hipLaunchKernelGGL(point_tail_bwd_r_kernel<true>, dim3(gsz), dim3(kThreadsR), 0, st, dout, prev, agg, N, Wp, bp,
                       ln_w, ln_b, eps, Wm, dx, dagg, part);
  else
    hipLaunchKernelGGL(point_tail_bwd_r_kernel<false>, dim3(gsz), dim3(kThreadsR), 0, st, dout, prev, agg, N, Wp, bp,
                       ln_w, ln_b, eps, Wm, dx, dagg, part);
  return launch_status("gasfm_point_tail_bwd");
}

extern "C" int gasfm_point_hub_fwd(const float* X, int64_t N, float eps, const float* gA, const float* bA,
                                   const float* WA, float* SA, const float* WB, const float* bB, float* XL,
                                   const float* gC, const float* bC, const float* WC, const float* bWC,
                                   const float* WD, const float* bD, float* XR, void* stream) {
  GASFM_REQUIRE(N >= 0, "gasfm_point_hub_fwd: N < 0");
  const bool hc = gC != nullptr;
  if (N == 0) return GASFM_OK;
  GASFM_REQUIRE(X && gA && bA && WA && SA && WB && bB && XL, "gasfm_point_hub_fwd: null pointer");
  GASFM_REQUIRE(!hc || (bC && WC && bWC && WD && bD && XR), "gasfm_point_hub_fwd: null pointer (C part)");
  GASFM_REQUIRE(aligned16(X), "gasfm_point_hub_fwd: alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hc)
    hipLaunchKernelGGL(point_hub_fwd_t_kernel<true>, dim3(gridT(&point_hub_fwd_t_kernel<true>, N)), dim3(kThreadsT),
                       0, st, X, N, eps, gA, bA, WA, SA, WB, bB, XL, gC, bC, WC, bWC, WD, bD, XR);
  else
    hipLaunchKernelGGL(point_hub_fwd_t_kernel<false>, dim3(gridT(&point_hub_fwd_t_kernel<false>, N)),
                       dim3(kThreadsT), 0, st, X, N, eps, gA, bA, WA, SA, WB, bB, XL, gC, bC, WC, bWC, WD, bD, XR);
  return launch_status("gasfm_point_hub_fwd");
}

extern "C" int gasfm_point_tail_hub_fwd(const float* prev, const float* agg, int64_t N, const float* Wp,
                                        const float* bp, const float* ln_w, const float* ln_b, float eps,
                                        const float* Wm, const float* bm, float* out, float eps_h, const float* gA,
                                        const float* bA, const float* WA, float* SA, const float* WB,
                                        const float* bB, float* XL, const float* gC, const float* bC,
                                        const float* WC, const float* bWC, const float* WD, const float* bD,
                                        float* XR, void* stream) {
  GASFM_REQUIRE(N >= 0, "gasfm_point_tail_hub_fwd: N < 0");
  const bool hc = gC != nullptr;
  if (N == 0) return GASFM_OK;
  GASFM_REQUIRE(agg && Wp && bp && ln_w && ln_b && Wm && bm && out && gA && bA && WA && SA && WB && bB && XL,
                "gasfm_point_tail_hub_fwd: null pointer");
  GASFM_REQUIRE(!hc || (bC && WC && bWC && WD && bD && XR), "gasfm_point_tail_hub_fwd: null pointer (C part)");
  GASFM_REQUIRE(aligned16(agg) && (!prev || aligned16(prev)) && aligned16(out) && aligned16(SA) && aligned16(XL) &&
                    (!hc || aligned16(XR)),
                "gasfm_point_tail_hub_fwd: alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // 4-wave workgroups (two per CU by the 64 KB of staged weights: 2 waves per SIMD); 6-wave ones
  // (3 per SIMD at 156 VGPRs) measured 31.5 vs 18.3 us per rank-of-8 launch, 94.9 vs 72.5 at config 4
  // (profiles/r6_ab_tail_hub.txt)
#define GASFM_LAUNCH(PV, HCV)                                                                                  \
  hipLaunchKernelGGL((point_tail_hub_fwd_t_kernel<PV, HCV, 4>),                                                \
                     dim3(resident_grid(reinterpret_cast<const void*>(&point_tail_hub_fwd_t_kernel<PV, HCV, 4>), \
                                        4 * kW, 0, tiles_of(N), 4)),                                           \
                     dim3(4 * kW), 0, st, prev, agg, N, Wp, bp, ln_w, ln_b, eps, Wm, bm, out, eps_h, gA, bA, WA, \
                     SA, WB, bB, XL, gC, bC, WC, bWC, WD, bD, XR)
  if (prev && hc)
    GASFM_LAUNCH(true, true);
  else if (prev)
    GASFM_LAUNCH(true, false);
  else if (hc)
    GASFM_LAUNCH(false, true);
  else
    GASFM_LAUNCH(false, false);
#undef GASFM_LAUNCH
  return launch_status("gasfm_point_tail_hub_fwd");
}

extern "C" int gasfm_point_hub_bwd(const float* X, int64_t N, float eps, const float* gA, const float* bA,
                                   const float* WA, const float* WB, const float* gC, const float* bC,
                                   const float* WC, const float* bWC, const float* WD, const float* dSA,
                                   const float* dXL, const float* dXR, const float* dRes, float* dX, float* part_a,
                                   float* part_c, void* stream) {
  GASFM_REQUIRE(N >= 0, "gasfm_point_hub_bwd: N < 0");
  if (N == 0) return GASFM_OK;
  GASFM_REQUIRE(X && gA && bA && WA && WB && gC && bC && WC && bWC && WD && dSA && dXL && dXR && dX && part_a &&
                    part_c,
                "gasfm_point_hub_bwd: null pointer");
  GASFM_REQUIRE(aligned16(X) && aligned16(dSA) && aligned16(dXL) && aligned16(dXR),
                "gasfm_point_hub_bwd: alignment");
  GASFM_REQUIRE(dX != X && dX != dSA && dX != dXL && dX != dXR, "gasfm_point_hub_bwd: dX aliases an input");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int gsz = hub_r_grid(N);
  if (dRes)
    hipLaunchKernelGGL(point_hub_bwd_r_kernel<true>, dim3(gsz), dim3(kThreadsR), 0, st, X, N, eps, gA, bA, WA, WB,
                       gC, bC, WC, bWC, WD, dSA, dXL, dXR, dRes, dX, part_a, part_c);
  else
    hipLaunchKernelGGL(point_hub_bwd_r_kernel<false>, dim3(gsz), dim3(kThreadsR), 0, st, X, N, eps, gA, bA, WA, WB,
                       gC, bC, WC, bWC, WD, dSA, dXL, dXR, dRes, dX, part_a, part_c);
  return launch_status("gasfm_point_hub_bwd");
}
