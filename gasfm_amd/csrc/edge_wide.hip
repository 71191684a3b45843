// Edge epilogue of a depth conf's last block (32-wide features in, 128-wide out), gfx950.
//
// With a depth head the last GraphAttnSfMLayer (code/models/layers.py:232-261) widens the projection
// features to the head's 128: lin_proj is [128 x 34] and the residual runs through its own LayerNorm
// and a [128 x 32] skip projection (residual_skipconn_proj_norm_layer + skip_projection, layers.py:
// 214-220, 256-261), with GraphAttnSfMProjectionFeatureUpdate (layers.py:911-956) as in every block:
//   P'[e] = Wsk relu(LN_b(P[e])) + bsk
//         + scale (Wp [relu(LN_a(P[e])) | P0[e]] + bp + Sp[pt[e]] + Sv[cam[e]] + Sg),   scale = 1/4.
// Block 0's epilogue (edge_block0.hip) has this shape at width 2 -> 32; the attention half of the
// block reads 32-wide P like every block >= 1 and stays on edge_cam.hip.
//
//   edge_wide_epilogue_fwd  P' [E x 128].  Per 16-edge tile both LayerNorms are computed once from
//                           the row statistics, and both products run as ONE stacked K = 68 product
//                           [hat_b | hat_a | P0 | 0 0] x [Wsk | scale Wp]^T on v_mfma_f32_16x16x4_f32
//                           (17 k steps x 8 column tiles; the pre-scaling by 1/4 is exact).
//   edge_wide_epilogue_bwd  camera work items (contiguous edges of one camera; split items write
//                           partial slots).  From dP' [E x 128]:
//                             Q = dP' x [Wsk | scale Wp]                  (K = 128, 80 columns, 5 tiles)
//                             dP = LN_a_bwd(mask_a Q[:, 32:64]) + LN_b_bwd(mask_b Q[:, :32]),  dP0 = Q[:, 64:66]
//                             dW += dP'^T [hat_b | hat_a | P0]            (128 x 80 in the C layout:
//                                  160 accumulators per lane, held for the whole launch)
//                             dSv[cam] = scale sum dP', dbsk, dgamma / dbeta of both LayerNorms.
//                           dP is complete for this epilogue: LayerNorm backward is linear in its
//                           upstream gradient, so it adds to the attention half's dP.
//   segment_rowsum_w        out[seg] = scale sum X[perm[..]] for 128-wide rows (dSp).
//
// Tile conventions are tile.hpp's: wave = 16-edge tile, MFMA A[i = lane&15][k = lane>>4],
// B[k][j = lane&15], C[row = 4 (lane>>4) + r][col = lane&15].  LDS row strides: an A-operand tile
// == 2 mod 4 and 16 distinct banks over c (70, 130), staged weights == 16 mod 32 (144, 80): the two
// k rows of a 32-lane read group fall 16 banks apart.
//   forward   [68 x 144] weights + one 16 x 130 tile per wave (the A tile, then P' on its way to
//             whole-row stores): 39,168 + 4 x 8,320 = 72,448 B, two workgroups per CU.
//   backward  [128 x 80] weights + per wave dP' 16 x 130, [hat_b | hat_a | P0 | 0] 16 x 82, x_hat
//             16 x 34, rstd 16: 40,960 + 4 x 15,808 = 104,192 B, one workgroup per CU, one wave per
//             SIMD: the 512-entry register file is the wave's own (depth_head.hip's backward).
// Compiler's resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   edge_wide_epilogue_fwd_kernel   VGPRs 198  AGPRs  32  scratch 0  LDS  72,448 B  (2 waves / SIMD)
//   edge_wide_epilogue_bwd_kernel   VGPRs 223  AGPRs 184  scratch 0  LDS 104,192 B  (1 wave / SIMD)
//   segment_rowsum_w_kernel         VGPRs  50  AGPRs   0  scratch 0  LDS       0 B
// Weight and LayerNorm gradients leave as per-workgroup partial rows (ordered workgroup reduction)
// for gasfm_colsum: deterministic, no atomics, no host read.
#include <hip/hip_runtime.h>

#include "../../include/gasfm_edge_wide.h"
#include "common.hpp"
#include "tile.hpp"

namespace gasfm {
namespace {

using namespace tile;

constexpr int F = 32;             // input feature width
constexpr int FO = 128;           // output feature width
constexpr int NTO = FO / 16;
constexpr int KS = 68;            // forward stacked K: hat_b 32 | hat_a 32 | P0 2 | 0 0
constexpr int LDA = 70;           // forward A tile [16 x 68]
constexpr int LDB = 144;          // forward weights [68 x 128]
constexpr int LDO = 130;          // 16 x 128 tiles (P' out, dP' in)
constexpr int LD34 = 34;
constexpr int NQ = 80;            // backward: [hat_b | hat_a | P0 | 0 ...] columns, 5 MFMA tiles
constexpr int NTQ = NQ / 16;
constexpr int LDQ = 80;           // backward weights [128 x 80]
constexpr int LDH = 82;           // backward H tile [16 x 80]
constexpr int FWD_TILE = TR * LDO;
constexpr int BW_W = FO * LDQ;
constexpr int BW_WAVE = TR * LDO + TR * LDH + TR * LD34 + TR;
constexpr int BW_SCRATCH = kWaves * BW_WAVE;
static_assert(TR * LDA <= FWD_TILE, "edge_wide: the A tile lies inside the output tile");
static_assert((BW_W + kWaves * BW_WAVE) * 4 <= 160 * 1024, "edge_wide: LDS budget");

struct Affine4 {
  float4 g, b;
};
__device__ __forceinline__ Affine4 load_affine(const float* __restrict__ gam, const float* __restrict__ bet,
                                               int lane) {
  return {*reinterpret_cast<const float4*>(gam + (lane & 7) * 4), *reinterpret_cast<const float4*>(bet + (lane & 7) * 4)};
}

// Row layout of a 16 x 32 tile: lane l holds row (l>>3) + 8u (u = 0, 1), columns 4(l&7)..+3.  Rows
// >= nrows re-read row 0 of the tile and are masked where they are staged (a select right after a
// prefetching load would make the wave wait for it).
__device__ __forceinline__ void issue_rows32(const float* __restrict__ P, int64_t row0, int nrows, float4 (&v)[2],
                                             int lane) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = (lane >> 3) + 8 * u;
    v[u] = *reinterpret_cast<const float4*>(P + (row0 + (r < nrows ? r : 0)) * F + (lane & 7) * 4);
  }
}
// Row layout of a 16 x 128 tile: lane l holds row (l>>5) + 2u (u < 8), columns 4(l&31)..+3.
__device__ __forceinline__ void issue_rows128(const float* __restrict__ X, int64_t row0, int nrows, float4 (&v)[8],
                                              int lane) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int r = (lane >> 5) + 2 * u;
    v[u] = *reinterpret_cast<const float4*>(X + (row0 + (r < nrows ? r : 0)) * FO + (lane & 31) * 4);
  }
}

__device__ __forceinline__ void st2(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }

// Row statistics of the row-layout registers v[u] (3 xor steps over the row's 8 lanes): x_hat and rstd.
struct RowNorm {
  float xh[4], rstd;
};
__device__ __forceinline__ RowNorm row_norm(const float4& v, float eps) {
  const float x[4] = {v.x, v.y, v.z, v.w};
  float s = x[0] + x[1] + x[2] + x[3];
  s = group_sum<8>(s);
  const float mean = s * (1.f / F);
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) q = fmaf(x[k] - mean, x[k] - mean, q);
  q = group_sum<8>(q);
  RowNorm n;
  n.rstd = rsq_normal(q * (1.f / F) + eps);
#pragma unroll
  for (int k = 0; k < 4; ++k) n.xh[k] = (x[k] - mean) * n.rstd;
  return n;
}
// relu(x_hat g + b) of a live row, 0 of a dead one: four columns to T
__device__ __forceinline__ void st_hat(float* T, const RowNorm& n, const Affine4& af, bool live) {
  const float g[4] = {af.g.x, af.g.y, af.g.z, af.g.w}, b[4] = {af.b.x, af.b.y, af.b.z, af.b.w};
  float h[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = live ? fmaxf(fmaf(n.xh[k], g[k], b[k]), 0.f) : 0.f;
  st2(T, h[0], h[1]);
  st2(T + 2, h[2], h[3]);
}

// ================================================================================================
// forward
// ================================================================================================
__global__ __launch_bounds__(kThreads) void edge_wide_epilogue_fwd_kernel(
    const float* __restrict__ P, const float* __restrict__ P0, const int32_t* __restrict__ cam,
    const int32_t* __restrict__ pt, int64_t E, const float* __restrict__ ga, const float* __restrict__ ba,
    const float* __restrict__ gb, const float* __restrict__ bb, float eps, const float* __restrict__ Wp, int ldWp,
    const float* __restrict__ bp, const float* __restrict__ Wsk, const float* __restrict__ bsk,
    const float* __restrict__ Sp, const float* __restrict__ Sv, int64_t ldSv, const float* __restrict__ Sg,
    float scale, float* __restrict__ Pout) {
  __shared__ float Bs[KS * LDB];  // Bs[k][j]: k < 32 Wsk[j][k], 32 <= k < 64 scale Wp[j][k - 32], 64, 65 scale Wp[j][32, 33]
  __shared__ float tiles[kWaves][FWD_TILE];
  {
    Stage<FO * F, kThreads> s1, s2;
    s1.load([&](int q) { return Wsk[q]; });
    s2.load([&](int q) { return Wp[(q / F) * ldWp + q % F]; });
    s1.store([&](int q, float v) { Bs[(q % F) * LDB + q / F] = v; });
    s2.store([&](int q, float v) { Bs[(F + q % F) * LDB + q / F] = scale * v; });
    Stage<4 * FO, kThreads> s3;
    s3.load([&](int q) { return (P0 && q < 2 * FO) ? Wp[(q % FO) * ldWp + F + q / FO] : 0.f; });
    s3.store([&](int q, float v) { Bs[(2 * F + q / FO) * LDB + q % FO] = scale * v; });
  }
  __syncthreads();
  const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
  const int c = lane & 15, g = lane >> 4;
  const int cc = (lane & 7) * 4;   // 32-wide row layout
  const int co = (lane & 31) * 4;  // 128-wide row layout
  float* T = tiles[wave];
  const Affine4 afa = load_affine(ga, ba, lane), afb = load_affine(gb, bb, lane);
  float cst[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cst[k] = fmaf(bp[co + k] + Sg[co + k], scale, bsk[co + k]);
  const int64_t ntiles = (E + TR - 1) / TR;
  const int64_t gw = int64_t(blockIdx.x) * kWaves + wave, nw = int64_t(gridDim.x) * kWaves;
  auto rows_of = [&](int64_t t) { return int(E - t * TR < TR ? E - t * TR : TR); };
  // register copy of the next tile: P rows, the tile's camera ids on lanes 0..15 and point ids on
  // lanes 16..31, P0 pairs on lanes < 32 (without P0 the load reads P's first words, unused)
  float4 np[2];
  int32_t ni = 0;
  float nq = 0.f;
  const int32_t* ip = (lane & 16) ? pt : cam;
  const float* p0p = P0 ? P0 : P;
  auto issue = [&](int64_t t) {
    const int64_t row0 = t * TR;
    const int nrows = rows_of(t);
    issue_rows32(P, row0, nrows, np, lane);
    ni = ip[row0 + (c < nrows ? c : 0)];
    nq = p0p[row0 * 2 + ((lane & 31) < 2 * nrows ? (lane & 31) : 0)];
  };
  if (gw < ntiles) issue(gw);
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t row0 = t * TR;
    const int nrows = rows_of(t);
    // the tile's node-term gathers: their latency overlaps the LayerNorms and the MFMA
    float4 sp[8], sv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c0 = __builtin_amdgcn_readlane(ni, 2 * u), c1 = __builtin_amdgcn_readlane(ni, 2 * u + 1);
      const int p0 = __builtin_amdgcn_readlane(ni, 16 + 2 * u), p1 = __builtin_amdgcn_readlane(ni, 17 + 2 * u);
      const int ci = (lane & 32) ? c1 : c0, pi = (lane & 32) ? p1 : p0;
      sp[u] = *reinterpret_cast<const float4*>(Sp + int64_t(pi) * FO + co);
      sv[u] = *reinterpret_cast<const float4*>(Sv + int64_t(ci) * ldSv + co);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = (lane >> 3) + 8 * u;
      const RowNorm n = row_norm(np[u], eps);
      st_hat(T + r * LDA + cc, n, afb, r < nrows);
      st_hat(T + r * LDA + F + cc, n, afa, r < nrows);
    }
    if (lane < 32) {
      T[(lane >> 1) * LDA + 2 * F + (lane & 1)] = (P0 && lane < 2 * nrows) ? nq : 0.f;
      T[(lane >> 1) * LDA + 2 * F + 2 + (lane & 1)] = 0.f;
    }
    issue(t + nw < ntiles ? t + nw : t);  // unconditional: the last tile re-reads itself
    wave_sync();
    f32x4 acc[NTO];
#pragma unroll
    for (int nt = 0; nt < NTO; ++nt) acc[nt] = zero4();
#pragma unroll
    for (int s = 0; s < KS / 4; ++s) {
      const float a = T[c * LDA + 4 * s + g];
#pragma unroll
      for (int nt = 0; nt < NTO; ++nt) acc[nt] = mfma16(a, Bs[(4 * s + g) * LDB + nt * 16 + c], acc[nt]);
    }
    wave_sync();  // every lane has read the A tile: P' takes its place
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nt = 0; nt < NTO; ++nt) T[(4 * g + r) * LDO + nt * 16 + c] = acc[nt][r];
    wave_sync();
    float4 vo[8];
    rows_from_lds<FO, LDO>(T, vo, lane);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      vo[u].x += fmaf(sp[u].x + sv[u].x, scale, cst[0]);
      vo[u].y += fmaf(sp[u].y + sv[u].y, scale, cst[1]);
      vo[u].z += fmaf(sp[u].z + sv[u].z, scale, cst[2]);
      vo[u].w += fmaf(sp[u].w + sv[u].w, scale, cst[3]);
    }
    rows_store<FO>(Pout, FO, row0, nrows, vo, lane);
    wave_sync();
  }
}

// ================================================================================================
// backward, one wave per camera work item
// part row per workgroup: [dWp 128 x ldWp | dWsk 128 x 32 | dbsk 128 | dgamma_a 32 | dbeta_a 32 |
//                          dgamma_b 32 | dbeta_b 32]
// ================================================================================================
__global__ __launch_bounds__(kThreads) void edge_wide_epilogue_bwd_kernel(
    const gasfm_work_item* __restrict__ items, int n_items, const float* __restrict__ dPo,
    const float* __restrict__ P, const float* __restrict__ P0, const float* __restrict__ ga,
    const float* __restrict__ ba, const float* __restrict__ gb, const float* __restrict__ bb, float eps,
    const float* __restrict__ Wp, int ldWp, const float* __restrict__ Wsk, float scale, float* __restrict__ dP,
    float* __restrict__ dP0, float* __restrict__ dSv, float* __restrict__ part_dsv, float* __restrict__ part) {
  __shared__ float lds[BW_W + kWaves * BW_WAVE];
  float* Wb = lds;  // Wb[j][n]: n < 32 Wsk[j][n], 32 <= n < 64 scale Wp[j][n - 32], 64, 65 scale Wp[j][32, 33], then 0
#pragma unroll 1
  for (int q0 = 0; q0 < FO * NQ; q0 += 8 * kThreads) {
    Stage<8 * kThreads, kThreads> s;
    s.load([&](int q) {
      const int j = (q0 + q) / NQ, n = (q0 + q) % NQ;
      // one unconditional load of an in-range word, then the select (see tile.hpp load_tile)
      const float wsk = Wsk[j * F + (n < F ? n : 0)];
      const float wp = Wp[j * ldWp + (n >= F && n < F + ldWp ? n - F : 0)];
      return n < F ? wsk : (n < F + ldWp ? scale * wp : 0.f);
    });
    s.store([&](int q, float v) { Wb[((q0 + q) / NQ) * LDQ + (q0 + q) % NQ] = v; });
  }
  const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
  const int c = lane & 15, g = lane >> 4;
  const int cc = (lane & 7) * 4, co = (lane & 31) * 4;
  float* D = lds + BW_W + wave * BW_WAVE;  // dP'                      16 x 130
  float* H = D + TR * LDO;                 // hat_b | hat_a | P0 | 0   16 x 82
  float* Xh = H + TR * LDH;                // x_hat -> dP              16 x 34
  float* Rs = Xh + TR * LD34;              // rstd                     16
  for (int q = lane; q < TR * (NQ - 2 * F - 2); q += kW)  // the zero columns 66..79, written once
    H[(q / (NQ - 2 * F - 2)) * LDH + 2 * F + 2 + q % (NQ - 2 * F - 2)] = 0.f;
  __syncthreads();
  const Affine4 afa = load_affine(ga, ba, lane), afb = load_affine(gb, bb, lane);
  float gia[2], bia[2], gib[2], bib[2];  // C layout: columns nt * 16 + c
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    gia[nt] = ga[nt * 16 + c];
    bia[nt] = ba[nt * 16 + c];
    gib[nt] = gb[nt * 16 + c];
    bib[nt] = bb[nt * 16 + c];
  }
  f32x4 accW[NTO][NTQ];
#pragma unroll
  for (int mt = 0; mt < NTO; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTQ; ++nt) accW[mt][nt] = zero4();
  float x[NTO + 8];  // dbsk 8 | dgamma_a 2 | dbeta_a 2 | dgamma_b 2 | dbeta_b 2
#pragma unroll
  for (int k = 0; k < NTO + 8; ++k) x[k] = 0.f;
  // register copy of the next tile: dP' and P rows (row layouts), P0 (lanes < 2 * nrows)
  float4 nd[8], np[2];
  float nq = 0.f;
  const float* p0p = P0 ? P0 : P;
  auto issue = [&](int64_t row0, int nrows) {
    issue_rows128(dPo, row0, nrows, nd, lane);
    issue_rows32(P, row0, nrows, np, lane);
    nq = p0p[row0 * 2 + ((lane & 31) < 2 * nrows ? (lane & 31) : 0)];
  };
  auto rows_at = [](const gasfm_work_item& w, int64_t row0) { return int(w.end - row0 < TR ? w.end - row0 : TR); };
  const int gw = blockIdx.x * kWaves + wave, nw = gridDim.x * kWaves;
  gasfm_work_item w{0, 0, 0, -1};
  if (gw < n_items) {
    w = items[gw];
    if (w.begin < w.end) issue(w.begin, rows_at(w, w.begin));
  }
  for (int it = gw; it < n_items; it += nw) {
    float dsv[NTO];
#pragma unroll
    for (int mt = 0; mt < NTO; ++mt) dsv[mt] = 0.f;
    gasfm_work_item wn{0, 0, 0, -1};
    const bool more = it + nw < n_items;
    if (more) wn = items[it + nw];
    if (w.begin >= w.end && more && wn.begin < wn.end) issue(wn.begin, rows_at(wn, wn.begin));
    for (int64_t row0 = w.begin; row0 < w.end; row0 += TR) {
      const int nrows = rows_at(w, row0);
      // stage the prefetched tile
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = (lane >> 5) + 2 * u;
        const float4 v = r < nrows ? nd[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        st2(D + r * LDO + co, v.x, v.y);
        st2(D + r * LDO + co + 2, v.z, v.w);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r = (lane >> 3) + 8 * u;
        const bool live = r < nrows;
        const RowNorm n = row_norm(np[u], eps);
        st2(Xh + r * LD34 + cc, live ? n.xh[0] : 0.f, live ? n.xh[1] : 0.f);
        st2(Xh + r * LD34 + cc + 2, live ? n.xh[2] : 0.f, live ? n.xh[3] : 0.f);
        st_hat(H + r * LDH + cc, n, afb, live);
        st_hat(H + r * LDH + F + cc, n, afa, live);
        if ((lane & 7) == 0) Rs[r] = n.rstd;
      }
      if (lane < 32) H[(lane >> 1) * LDH + 2 * F + (lane & 1)] = (P0 && lane < 2 * nrows) ? nq : 0.f;
      {  // the next tile: this item's, else the next item's first; the last one re-reads itself
        int64_t r1 = row0;
        int n1 = nrows;
        if (row0 + TR < w.end) {
          r1 = row0 + TR;
          n1 = rows_at(w, r1);
        } else if (more && wn.begin < wn.end) {
          r1 = wn.begin;
          n1 = rows_at(wn, r1);
        }
        issue(r1, n1);
      }
      wave_sync();
      // Q (C layout: edge 4g + r, column nt * 16 + c) = dP' [Wsk | scale Wp]
      f32x4 acc[NTQ];
#pragma unroll
      for (int nt = 0; nt < NTQ; ++nt) acc[nt] = zero4();
#pragma unroll 4
      for (int s = 0; s < FO / 4; ++s) {
        const float a = D[c * LDO + 4 * s + g];
#pragma unroll
        for (int nt = 0; nt < NTQ; ++nt) acc[nt] = mfma16(a, Wb[(4 * s + g) * LDQ + nt * 16 + c], acc[nt]);
      }
      // dW += dP'^T [hat_b | hat_a | P0 | 0]; per-camera and overall column sums of dP'
#pragma unroll
      for (int s = 0; s < TR / 4; ++s) {
        const int row = 4 * s + g;
        float h[NTQ];
#pragma unroll
        for (int nt = 0; nt < NTQ; ++nt) h[nt] = H[row * LDH + nt * 16 + c];
#pragma unroll
        for (int mt = 0; mt < NTO; ++mt) {
          const float a = D[row * LDO + mt * 16 + c];
          dsv[mt] += a;
#pragma unroll
          for (int nt = 0; nt < NTQ; ++nt) accW[mt][nt] = mfma16(a, h[nt], accW[mt][nt]);
        }
      }
      // ReLU masks + both LayerNorm backwards in the C layout; their sum overwrites x_hat in place
      // (each lane reads then writes only its own elements)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 4 * g + r;
        float xh[2], gva[2], gvb[2];
        float a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          xh[nt] = Xh[e * LD34 + nt * 16 + c];
          const float dyb = fmaf(xh[nt], gib[nt], bib[nt]) > 0.f ? acc[nt][r] : 0.f;
          const float dya = fmaf(xh[nt], gia[nt], bia[nt]) > 0.f ? acc[2 + nt][r] : 0.f;
          x[NTO + nt] = fmaf(dya, xh[nt], x[NTO + nt]);
          x[NTO + 2 + nt] += dya;
          x[NTO + 4 + nt] = fmaf(dyb, xh[nt], x[NTO + 4 + nt]);
          x[NTO + 6 + nt] += dyb;
          gva[nt] = dya * gia[nt];
          gvb[nt] = dyb * gib[nt];
          a1 += gva[nt];
          a2 = fmaf(gva[nt], xh[nt], a2);
          b1 += gvb[nt];
          b2 = fmaf(gvb[nt], xh[nt], b2);
        }
        a1 = sum16(a1) * (1.f / F);
        a2 = sum16(a2) * (1.f / F);
        b1 = sum16(b1) * (1.f / F);
        b2 = sum16(b2) * (1.f / F);
        const float rs = Rs[e];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          Xh[e * LD34 + nt * 16 + c] = rs * (gva[nt] - a1 - xh[nt] * a2) + rs * (gvb[nt] - b1 - xh[nt] * b2);
        if (P0 && c < 2 && e < nrows) dP0[(row0 + e) * 2 + c] = acc[4][r];
      }
      wave_sync();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r = (lane >> 3) + 8 * u;
        if (r < nrows) {
          const float2 a0 = *reinterpret_cast<const float2*>(Xh + r * LD34 + cc);
          const float2 a1 = *reinterpret_cast<const float2*>(Xh + r * LD34 + cc + 2);
          *reinterpret_cast<float4*>(dP + (row0 + r) * F + cc) = make_float4(a0.x, a0.y, a1.x, a1.y);
        }
      }
      wave_sync();
    }
#pragma unroll
    for (int mt = 0; mt < NTO; ++mt) {
      x[mt] += dsv[mt];
      dsv[mt] = sum_groups(dsv[mt]);
    }
    if (g == 0) {
      float* dst = (w.slot < 0) ? dSv + int64_t(w.seg) * FO : part_dsv + int64_t(w.slot) * FO;
#pragma unroll
      for (int mt = 0; mt < NTO; ++mt) dst[mt * 16 + c] = dsv[mt] * scale;
    }
    w = wn;
  }
  // ordered workgroup reduction, 16 output rows of dW at a time through the tile scratch
  float* scratch = lds + BW_W;
  float* out = part + int64_t(blockIdx.x) * (FO * ldWp + FO * F + FO + 4 * F);
  float* oWsk = out + FO * ldWp;
#pragma unroll
  for (int mt = 0; mt < NTO; ++mt) {
    float v[NTQ * 4];
#pragma unroll
    for (int nt = 0; nt < NTQ; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[nt * 4 + r] = accW[mt][nt][r];
    wg_reduce_ordered<NTQ * 4, kWaves, BW_SCRATCH>(v, scratch, wave, lane);
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = mt * 16 + 4 * g + r;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          oWsk[j * F + nt * 16 + c] = v[nt * 4 + r];
          out[j * ldWp + nt * 16 + c] = v[(2 + nt) * 4 + r] * scale;
        }
        if (c < ldWp - F) out[j * ldWp + F + c] = v[4 * 4 + r] * scale;
      }
    }
  }
  wg_reduce_ordered<NTO + 8, kWaves, BW_SCRATCH>(x, scratch, wave, lane);
  if (wave == 0) {
    float* ob = oWsk + FO * F;
#pragma unroll
    for (int k = 0; k < NTO + 8; ++k) {
      const float t = sum_groups(x[k]);
      // dbsk: column 16 k + c; the LayerNorm sums: [dgamma_a | dbeta_a | dgamma_b | dbeta_b], 2 column tiles each
      if (g == 0) ob[k * 16 + c] = t;
    }
  }
}

// ================================================================================================
// segment_rowsum_w: out[seg] = scale * sum_{e in item} X[src_e]   (128-wide rows, optional perm)
// 32 lanes x float4 per row, 2 rows per wave step, 8 steps in flight
// ================================================================================================
__global__ __launch_bounds__(kThreads) void segment_rowsum_w_kernel(const gasfm_work_item* __restrict__ items,
                                                                   int n_items, const int32_t* __restrict__ perm,
                                                                   const float* __restrict__ X, int64_t ldX,
                                                                   float scale, float* __restrict__ out,
                                                                   float* __restrict__ part) {
  const int lane = threadIdx.x & (kW - 1);
  const int half = lane >> 5, c = (lane & 31) * 4;
  const int nw = gridDim.x * kWaves;
  for (int it = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + threadIdx.x / kW); it < n_items; it += nw) {
    const gasfm_work_item w = items[it];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e0 = w.begin; e0 < w.end; e0 += 16) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {  // unconditional loads (rows past the item re-read its last edge)
        const int e = e0 + 2 * u + half;
        const int ec = e < w.end ? e : w.end - 1;
        const int64_t s = perm ? perm[ec] : ec;
        v[u] = *reinterpret_cast<const float4*>(X + s * ldX + c);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (e0 + 2 * u + half < w.end) {
          acc.x += v[u].x;
          acc.y += v[u].y;
          acc.z += v[u].z;
          acc.w += v[u].w;
        }
      }
    }
    acc.x = xsum32(acc.x);
    acc.y = xsum32(acc.y);
    acc.z = xsum32(acc.z);
    acc.w = xsum32(acc.w);
    if (half == 0) {
      float* dst = (w.slot < 0) ? out + int64_t(w.seg) * FO : part + int64_t(w.slot) * FO;
      *reinterpret_cast<float4*>(dst + c) = make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale);
    }
  }
}

int grid_fwd(int64_t E) {
  return resident_grid(reinterpret_cast<const void*>(&edge_wide_epilogue_fwd_kernel), kThreads, 0, (E + TR - 1) / TR,
                       kWaves);
}
int grid_bwd(int n_items) {
  return resident_grid(reinterpret_cast<const void*>(&edge_wide_epilogue_bwd_kernel), kThreads, 0, n_items, kWaves);
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_edge_wide_part_shape(int32_t which, int64_t E, int32_t n_items, int32_t ldWp,
                                              int32_t* cols) {
  if (which == 0) {
    if (cols) *cols = kWaves * TR;
    return E > 0 ? grid_fwd(E) : 0;
  }
  if (cols) *cols = FO * ldWp + FO * F + FO + 4 * F;
  return n_items > 0 ? grid_bwd(n_items) : 0;
}

extern "C" int gasfm_edge_wide_epilogue_fwd(const float* P, const float* P0, const int32_t* cam, const int32_t* pt,
                                            int64_t E, const float* ln_a_w, const float* ln_a_b,
                                            const float* ln_b_w, const float* ln_b_b, float eps, const float* Wp,
                                            int32_t ldWp, const float* bp, const float* Wsk, const float* bsk,
                                            const float* Sp, const float* Sv, int64_t ldSv, const float* Sg,
                                            float scale, float* Pout, void* stream) {
  GASFM_REQUIRE(E >= 0, "gasfm_edge_wide_epilogue_fwd: E < 0");
  if (E == 0) return GASFM_OK;  // nothing to do: the pointers of empty tensors are null
  GASFM_REQUIRE(P && cam && pt && Wp && bp && Wsk && bsk && Sp && Sv && Sg && Pout,
                "gasfm_edge_wide_epilogue_fwd: null pointer");
  GASFM_REQUIRE(ln_a_w && ln_a_b && ln_b_w && ln_b_b, "gasfm_edge_wide_epilogue_fwd: both LayerNorms are required");
  GASFM_REQUIRE((P0 && ldWp == 34) || (!P0 && ldWp == 32), "gasfm_edge_wide_epilogue_fwd: ldWp=%d vs P0", ldWp);
  GASFM_REQUIRE(ldSv >= FO && ldSv % 4 == 0, "gasfm_edge_wide_epilogue_fwd: ldSv=%lld", (long long)ldSv);
  GASFM_REQUIRE(aligned16(P) && aligned16(Sp) && aligned16(Sv) && aligned16(Pout) && aligned16(ln_a_w) &&
                    aligned16(ln_a_b) && aligned16(ln_b_w) && aligned16(ln_b_b),
                "gasfm_edge_wide_epilogue_fwd: P/Sp/Sv/Pout/LayerNorm parameters not 16-byte aligned");
  hipLaunchKernelGGL(edge_wide_epilogue_fwd_kernel, dim3(grid_fwd(E)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), P, P0, cam, pt, E, ln_a_w, ln_a_b, ln_b_w, ln_b_b, eps, Wp,
                     ldWp, bp, Wsk, bsk, Sp, Sv, ldSv, Sg, scale, Pout);
  return launch_status("gasfm_edge_wide_epilogue_fwd");
}

extern "C" int gasfm_edge_wide_epilogue_bwd(const void* items, int32_t n_items, const float* dPo,
                                            const float* P, const float* P0, const float* ln_a_w,
                                            const float* ln_a_b, const float* ln_b_w, const float* ln_b_b, float eps,
                                            const float* Wp, int32_t ldWp, const float* Wsk, float scale, float* dP,
                                            float* dP0, float* dSv, float* part_dsv, float* part, void* stream) {
  if (n_items <= 0) return GASFM_OK;  // nothing to do: the pointers of empty tensors are null
  GASFM_REQUIRE(items && dPo && P && Wp && Wsk && dP && dSv && part, "gasfm_edge_wide_epilogue_bwd: null pointer");
  GASFM_REQUIRE(ln_a_w && ln_a_b && ln_b_w && ln_b_b, "gasfm_edge_wide_epilogue_bwd: both LayerNorms are required");
  GASFM_REQUIRE((P0 && dP0 && ldWp == 34) || (!P0 && ldWp == 32), "gasfm_edge_wide_epilogue_bwd: ldWp=%d vs P0 / dP0",
                ldWp);
  GASFM_REQUIRE(aligned16(dPo) && aligned16(P) && aligned16(dP) && aligned16(ln_a_w) && aligned16(ln_a_b) &&
                    aligned16(ln_b_w) && aligned16(ln_b_b),
                "gasfm_edge_wide_epilogue_bwd: dPo/P/dP/LayerNorm parameters not 16-byte aligned");
  hipLaunchKernelGGL(edge_wide_epilogue_bwd_kernel, dim3(grid_bwd(n_items)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), static_cast<const gasfm_work_item*>(items), n_items, dPo, P,
                     P0, ln_a_w, ln_a_b, ln_b_w, ln_b_b, eps, Wp, ldWp, Wsk, scale, dP, dP0, dSv, part_dsv, part);
  return launch_status("gasfm_edge_wide_epilogue_bwd");
}

extern "C" int gasfm_segment_rowsum_w(const void* items, int32_t n_items, const int32_t* perm,
                                      const float* X, int64_t ldX, float scale, float* out, float* part,
                                      void* stream) {
  if (n_items <= 0) return GASFM_OK;  // nothing to do: the pointers of empty tensors are null
  GASFM_REQUIRE(items && X && out, "gasfm_segment_rowsum_w: null pointer");
  GASFM_REQUIRE(aligned16(X) && ldX >= FO && ldX % 4 == 0 && aligned16(out) && (!part || aligned16(part)),
                "gasfm_segment_rowsum_w: alignment / ldX");
  const int g = resident_grid(reinterpret_cast<const void*>(&segment_rowsum_w_kernel), kThreads, 0, n_items, kWaves);
  hipLaunchKernelGGL(segment_rowsum_w_kernel, dim3(g), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const gasfm_work_item*>(items), n_items, perm, X, ldX, scale, out, part);
  return launch_status("gasfm_segment_rowsum_w");
}
