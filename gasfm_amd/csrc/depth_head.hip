// The depth head of GraphAttnSfMNet / SetOfSetNet as fused row-tile kernels, gfx950.
//
// Reference (code/models/graph_attn_sfm.py:153-162, layers.py:10-44 with norm=False, two hidden
// layers): depths = depth_head(P), depth_head = Linear(128,128) ReLU Linear(128,128) ReLU
// Linear(128,1) on the raw last-block projection features P [E, 128] -- no ReLU before the first
// layer, unlike the scene-point head.  aten keeps two [E, 128] activations for the backward and
// allocates as many again for their gradients (2.05 GB each at config 4).  Here:
//   depth_head_fwd     one pass over P: y1 = P W1^T + b1, y2 = relu(y1) W2^T + b2 on
//                      v_mfma_f32_16x16x4_f32 against both weights staged in LDS, then
//                      d = relu(y2) . w3 + b3 as a 16-lane reduction of the C layout; only d is written;
//   depth_head_bwd_b   dW2, db2, dW3, db3;
//   depth_head_bwd_a   dP, dW1, db1.
// Both backward kernels recompute y1 and y2 from P.  Two kernels rather than one: a 128 x 128 weight
// gradient in the C layout is 256 accumulators per lane, so dW1 and dW2 do not fit one wave together.
// The weight-gradient products take both operands straight from C-layout registers: with the MFMA's
// k index of lane group g at step s standing for tile row 4g + s, A[i][k] = g2[row][16 mt + i] and
// B[k][j] = relu(y1)[row][16 nt + j] are exactly the registers [mt][s] and [nt][s] a lane holds after
// the layer products, so no LDS traffic goes with them.  Weight and bias gradients leave as
// per-workgroup partial rows (ordered workgroup reduction) for gasfm_colsum: deterministic, no atomics.
//
// Tile conventions are point_head.hip's (tile.hpp): wave = 16-row tile, MFMA A[i = lane&15][k =
// lane>>4], B[k][j = lane&15], C[row = 4 (lane>>4) + r][col = lane&15]; weights in the natural
// [out][in] layout and the activation tile both at row stride 130 (== 2 mod 32).
//
// LDS: both weights resident, 2 x 128 x 130 x 4 = 133,120 B, leave room for three 16 x 130 tiles
// (8,320 B each) in the CU's 160 KiB.  Every kernel needs ONE tile per wave -- P, relu(y1), g2, g1
// and dP pass through it in turn, everything else lives in registers -- so a workgroup is three
// waves: 133,120 + 24,960 + 1,536 (b1, b2, w3) = 159,616 B, one workgroup per CU, one wave per SIMD
// on three of the four SIMDs.  With occupancy fixed at one wave per SIMD by the LDS, the 512-entry
// register file is the wave's own: a backward kernel keeps its 256 weight-gradient accumulators
// in AGPRs for the whole launch.
// Compiler's resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   depth_head_fwd_kernel     VGPRs  85  AGPRs  36  scratch 0  LDS 159,616 B
//   depth_head_bwd_b_kernel   VGPRs 196  AGPRs 256  scratch 0  LDS 159,616 B
//   depth_head_bwd_a_kernel   VGPRs 205  AGPRs 256  scratch 0  LDS 159,616 B
// Two things keep the backward kernels from spilling: the layer products' k loop is unrolled by 4,
// not fully (fully unrolled, the scheduler hoists LDS reads until 512 registers are gone: 848 and
// 1,200 B of scratch), and b1, b2, w3 are read from LDS per tile instead of held (24 registers).
//
// A partial row is 66 KB, as much as 128 rows of P: a backward workgroup is given at least
// kMinTiles tiles per wave (384 rows) before another one is added, which keeps the partial buffers
// below the size of dP at every E (the grid is capped at the resident workgroups: 256 rows of
// partials, 17 MB each, at config 4).
#include <hip/hip_runtime.h>

#include "../../include/gasfm_depth_head.h"
#include "common.hpp"
#include "tile.hpp"

namespace gasfm {
namespace {

using namespace tile;

constexpr int FD = 128, NTD = FD / 16;
constexpr int L130 = 130;
constexpr int kWavesD = 3, kThreadsD = kWavesD * kW;
constexpr int kMinTiles = 8;                        // backward: tiles per wave before the grid grows
constexpr int WSD = FD * L130;                      // one staged weight
constexpr int TSD = TR * L130;                      // one activation tile
constexpr int SMEM = 2 * WSD + kWavesD * TSD + 3 * FD;  // floats: W1 | W2 | one tile per wave | b1 | b2 | w3
constexpr int PART_A = FD * FD + FD;                // dW1 | db1
constexpr int PART_B = FD * FD + FD + FD + 1;       // dW2 | db2 | dW3 | db3
static_assert(SMEM * 4 <= 160 * 1024, "depth head: LDS budget");

// [128 x 128] weight into LDS rows of stride L130, 16 loads in flight per thread at a time (the whole
// weight at once would hold 86 registers): five full chunks and a tail
__device__ __forceinline__ void stage_w(const float* __restrict__ W, float* Ws) {
  constexpr int CH = 16 * kThreadsD, FULL = (FD * FD / CH) * CH;
#pragma unroll 1
  for (int q0 = 0; q0 < FULL; q0 += CH) {
    Stage<CH, kThreadsD> s;
    s.load([&](int q) { return W[q0 + q]; });
    s.store([&](int q, float v) { Ws[((q0 + q) / FD) * L130 + (q0 + q) % FD] = v; });
  }
  Stage<FD * FD - FULL, kThreadsD> s;
  s.load([&](int q) { return W[FULL + q]; });
  s.store([&](int q, float v) { Ws[((FULL + q) / FD) * L130 + (FULL + q) % FD] = v; });
}

// acc[nt] (C layout, 16 x 128) = A (16 x 128 LDS tile) . B, where B[k][j] = W[j][k] (TRANS: x W^T, a
// forward layer) or W[k][j] (dy W, a backward layer)
template <bool TRANS>
__device__ __forceinline__ void mm128(const float* A, const float* W, f32x4 (&acc)[NTD], int c, int g) {
#pragma unroll
  for (int nt = 0; nt < NTD; ++nt) acc[nt] = zero4();
#pragma unroll 4
  for (int s = 0; s < FD / 4; ++s) {
    const int k = 4 * s + g;
    const float a = A[c * L130 + k];
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) {
      const float b = TRANS ? W[(nt * 16 + c) * L130 + k] : W[k * L130 + nt * 16 + c];
      acc[nt] = mfma16(a, b, acc[nt]);
    }
  }
}

// C layout -> LDS tile, relu'd when RELU
template <bool RELU>
__device__ __forceinline__ void c_to_lds(const f32x4 (&v)[NTD], float* T, int c, int g) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) T[(4 * g + r) * L130 + nt * 16 + c] = RELU ? fmaxf(v[nt][r], 0.f) : v[nt][r];
}

// b: a bias vector in LDS (read per tile: held in registers, the three vectors would cost 24 per lane)
__device__ __forceinline__ void add_bias(f32x4 (&v)[NTD], const float* b, int c) {
#pragma unroll
  for (int nt = 0; nt < NTD; ++nt) {
    const float x = b[nt * 16 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[nt][r] += x;
  }
}

// y1 = P W1^T + b1 and y2 = relu(y1) W2^T + b2 of one tile, both in the C layout (pre-activations);
// Pc = the tile of P itself in the C layout when KEEP_P.  Rows past nrows are those of P = 0.
// The tile T is free again on return.
template <bool KEEP_P>
__device__ __forceinline__ void layers(const float* __restrict__ P, int64_t row0, int nrows, float* T,
                                       const float* W1s, const float* W2s, const float* b1, const float* b2,
                                       f32x4 (&Pc)[NTD], f32x4 (&y1)[NTD], f32x4 (&y2)[NTD],
                                       int lane, int c, int g) {
  float4 v[FD / 16];
  rows_load<FD>(P, FD, row0, nrows, v, lane);
  rows_to_lds<FD, L130>(T, v, lane);
  wave_sync();
  if constexpr (KEEP_P) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nt = 0; nt < NTD; ++nt) Pc[nt][r] = T[(4 * g + r) * L130 + nt * 16 + c];
  }
  mm128<true>(T, W1s, y1, c, g);
  add_bias(y1, b1, c);
  wave_sync();
  c_to_lds<true>(y1, T, c, g);
  wave_sync();
  mm128<true>(T, W2s, y2, c, g);
  add_bias(y2, b2, c);
  wave_sync();
}

// dd of this lane's four tile rows 4g + r (zero past nrows)
__device__ __forceinline__ void load_dd(const float* __restrict__ dd, int64_t row0, int nrows, float (&v)[4], int g) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = 4 * g + r;
    const float x = dd[row0 + (e < nrows ? e : 0)];
    v[r] = e < nrows ? x : 0.f;
  }
}

// dW[16 mt + i][16 nt + j] += sum over the tile's rows of D[row][16 mt + i] H[row][16 nt + j] (H relu'd
// when RELU), D and H in the C layout: MFMA step s takes row 4g + s from lane group g
template <bool RELU>
__device__ __forceinline__ void acc_dw(const f32x4 (&D)[NTD], const f32x4 (&H)[NTD], f32x4 (&dW)[NTD][NTD]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float h[NTD];
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) h[nt] = RELU ? fmaxf(H[nt][s], 0.f) : H[nt][s];
#pragma unroll
    for (int mt = 0; mt < NTD; ++mt)
#pragma unroll
      for (int nt = 0; nt < NTD; ++nt) dW[mt][nt] = mfma16(D[mt][s], h[nt], dW[mt][nt]);
  }
}

// The workgroup's dW [128 x 128] (rows = output features) and `NX` further per-lane sums into its
// partial row: ordered sum over the waves, 16 output rows at a time through the tile scratch.
// x[k] holds a per-lane share whose sum over the four lane groups belongs to column 16 (k % 8) + c
// of segment k / 8 (written at out[FD * FD + (k / 8) * FD ...]).
template <int NX>
__device__ __forceinline__ void reduce_store(f32x4 (&dW)[NTD][NTD], float (&x)[NX], float* scratch, float* out,
                                             int wave, int lane, int c, int g) {
#pragma unroll
  for (int mt = 0; mt < NTD; ++mt) {
    float v[NTD * 4];
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[nt * 4 + r] = dW[mt][nt][r];
    wg_reduce_ordered<NTD * 4, kWavesD, kWavesD * TSD>(v, scratch, wave, lane);
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nt = 0; nt < NTD; ++nt) out[(mt * 16 + 4 * g + r) * FD + nt * 16 + c] = v[nt * 4 + r];
    }
  }
  wg_reduce_ordered<NX, kWavesD, kWavesD * TSD>(x, scratch, wave, lane);
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const float t = sum_groups(x[k]);
      if (g == 0) out[FD * FD + (k / NTD) * FD + (k % NTD) * 16 + c] = t;
    }
  }
}

struct Setup {
  float *W1s, *W2s, *T, *b1, *b2, *w3;
  int lane, wave, c, g;
};

// stage both weights and b1, b2, w3; this wave's tile
__device__ __forceinline__ void setup(float* smem, const float* __restrict__ W1, const float* __restrict__ b1,
                                      const float* __restrict__ W2, const float* __restrict__ b2,
                                      const float* __restrict__ W3, Setup& s) {
  s.W1s = smem;
  s.W2s = smem + WSD;
  s.b1 = smem + 2 * WSD + kWavesD * TSD;
  s.b2 = s.b1 + FD;
  s.w3 = s.b2 + FD;
  stage_w(W1, s.W1s);
  stage_w(W2, s.W2s);
  if (threadIdx.x < FD) {
    s.b1[threadIdx.x] = b1[threadIdx.x];
    s.b2[threadIdx.x] = b2[threadIdx.x];
    s.w3[threadIdx.x] = W3[threadIdx.x];
  }
  __syncthreads();
  s.lane = threadIdx.x & (kW - 1);
  s.wave = threadIdx.x / kW;
  s.c = s.lane & 15;
  s.g = s.lane >> 4;
  s.T = smem + 2 * WSD + s.wave * TSD;
}

// ------------------------------------------------------------------------------------------ fwd
__global__ __launch_bounds__(kThreadsD) void depth_head_fwd_kernel(const float* __restrict__ P, int64_t E,
                                                                   const float* __restrict__ W1,
                                                                   const float* __restrict__ b1,
                                                                   const float* __restrict__ W2,
                                                                   const float* __restrict__ b2,
                                                                   const float* __restrict__ W3,
                                                                   const float* __restrict__ b3,
                                                                   float* __restrict__ d) {
  __shared__ float smem[SMEM];
  Setup u;
  setup(smem, W1, b1, W2, b2, W3, u);
  const int c = u.c, g = u.g;
  const float bv3 = b3[0];
  const int64_t ntiles = (E + TR - 1) / TR;
  for (int64_t t = int64_t(blockIdx.x) * kWavesD + u.wave; t < ntiles; t += int64_t(gridDim.x) * kWavesD) {
    const int64_t row0 = t * TR;
    const int nrows = int(E - row0 < TR ? E - row0 : TR);
    f32x4 Pc[NTD], y1[NTD], y2[NTD];
    layers<false>(P, row0, nrows, u.T, u.W1s, u.W2s, u.b1, u.b2, Pc, y1, y2, u.lane, c, g);
    float w3[NTD];
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) w3[nt] = u.w3[nt * 16 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float p = 0.f;
#pragma unroll
      for (int nt = 0; nt < NTD; ++nt) p += fmaxf(y2[nt][r], 0.f) * w3[nt];
      p = sum16(p);
      const int e = 4 * g + r;
      if (c == 0 && e < nrows) d[row0 + e] = p + bv3;
    }
  }
}

// ------------------------------------------------------------------------------------------ bwd
// g2 = (dd (x) w3) * [y2 > 0], in place of y2
__device__ __forceinline__ void make_g2(f32x4 (&y2)[NTD], const float (&ddv)[4], const float* w3, int c) {
#pragma unroll
  for (int nt = 0; nt < NTD; ++nt) {
    const float w = w3[nt * 16 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) y2[nt][r] = y2[nt][r] > 0.f ? ddv[r] * w : 0.f;
  }
}

// dW2 += g2^T relu(y1), db2 += colsum g2, dW3 += dd^T relu(y2), db3 += sum dd
__global__ __launch_bounds__(kThreadsD) void depth_head_bwd_b_kernel(
    const float* __restrict__ P, int64_t E, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
    const float* __restrict__ dd, float* __restrict__ part) {
  __shared__ float smem[SMEM];
  Setup u;
  setup(smem, W1, b1, W2, b2, W3, u);
  const int c = u.c, g = u.g;
  f32x4 dW2[NTD][NTD];
#pragma unroll
  for (int mt = 0; mt < NTD; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) dW2[mt][nt] = zero4();
  float x[2 * NTD];  // db2 | dW3
#pragma unroll
  for (int k = 0; k < 2 * NTD; ++k) x[k] = 0.f;
  float x1[1] = {0.f};  // db3
  const int64_t ntiles = (E + TR - 1) / TR;
  for (int64_t t = int64_t(blockIdx.x) * kWavesD + u.wave; t < ntiles; t += int64_t(gridDim.x) * kWavesD) {
    const int64_t row0 = t * TR;
    const int nrows = int(E - row0 < TR ? E - row0 : TR);
    f32x4 Pc[NTD], y1[NTD], y2[NTD];
    layers<false>(P, row0, nrows, u.T, u.W1s, u.W2s, u.b1, u.b2, Pc, y1, y2, u.lane, c, g);
    float ddv[4];
    load_dd(dd, row0, nrows, ddv, g);
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[NTD + nt] += ddv[r] * fmaxf(y2[nt][r], 0.f);
    // every lane of a group holds the same dd: lane c = 0 alone carries db3
    if (c == 0) x1[0] += (ddv[0] + ddv[1]) + (ddv[2] + ddv[3]);
    make_g2(y2, ddv, u.w3, c);
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) x[nt] += (y2[nt][0] + y2[nt][1]) + (y2[nt][2] + y2[nt][3]);
    acc_dw<true>(y2, y1, dW2);
  }
  float* out = part + int64_t(blockIdx.x) * PART_B;
  reduce_store(dW2, x, smem + 2 * WSD, out, u.wave, u.lane, c, g);
  wg_reduce_ordered<1, kWavesD, kWavesD * TSD>(x1, smem + 2 * WSD, u.wave, u.lane);
  if (u.wave == 0) {
    const float t = sum_groups(x1[0]);
    if (u.lane == 0) out[FD * FD + 2 * FD] = t;
  }
}

// dP = g1 W1, g1 = (g2 W2) * [y1 > 0];  dW1 += g1^T P, db1 += colsum g1
__global__ __launch_bounds__(kThreadsD) void depth_head_bwd_a_kernel(
    const float* __restrict__ P, int64_t E, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
    const float* __restrict__ dd, float* __restrict__ dP, float* __restrict__ part) {
  __shared__ float smem[SMEM];
  Setup u;
  setup(smem, W1, b1, W2, b2, W3, u);
  const int c = u.c, g = u.g;
  float* T = u.T;
  f32x4 dW1[NTD][NTD];
#pragma unroll
  for (int mt = 0; mt < NTD; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) dW1[mt][nt] = zero4();
  float x[NTD];  // db1
#pragma unroll
  for (int k = 0; k < NTD; ++k) x[k] = 0.f;
  const int64_t ntiles = (E + TR - 1) / TR;
  for (int64_t t = int64_t(blockIdx.x) * kWavesD + u.wave; t < ntiles; t += int64_t(gridDim.x) * kWavesD) {
    const int64_t row0 = t * TR;
    const int nrows = int(E - row0 < TR ? E - row0 : TR);
    f32x4 Pc[NTD], y1[NTD], y2[NTD];
    layers<true>(P, row0, nrows, T, u.W1s, u.W2s, u.b1, u.b2, Pc, y1, y2, u.lane, c, g);
    float ddv[4];
    load_dd(dd, row0, nrows, ddv, g);
    make_g2(y2, ddv, u.w3, c);  // zero on rows past nrows: dd is
    c_to_lds<false>(y2, T, c, g);
    wave_sync();
    f32x4 acc[NTD];
    mm128<false>(T, u.W2s, acc, c, g);  // g2 W2
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) y1[nt][r] = y1[nt][r] > 0.f ? acc[nt][r] : 0.f;  // g1
#pragma unroll
    for (int nt = 0; nt < NTD; ++nt) x[nt] += (y1[nt][0] + y1[nt][1]) + (y1[nt][2] + y1[nt][3]);
    acc_dw<false>(y1, Pc, dW1);
    wave_sync();
    c_to_lds<false>(y1, T, c, g);
    wave_sync();
    mm128<false>(T, u.W1s, acc, c, g);  // dP = g1 W1
    wave_sync();
    c_to_lds<false>(acc, T, c, g);
    wave_sync();
    float4 vo[FD / 16];
    rows_from_lds<FD, L130>(T, vo, u.lane);
    rows_store<FD>(dP, FD, row0, nrows, vo, u.lane);
    wave_sync();
  }
  reduce_store(dW1, x, smem + 2 * WSD, part + int64_t(blockIdx.x) * PART_A, u.wave, u.lane, c, g);
}

int grid_fwd(int64_t E) {
  return resident_grid(reinterpret_cast<const void*>(&depth_head_fwd_kernel), kThreadsD, 0, (E + TR - 1) / TR, kWavesD);
}

// One grid for both backward kernels (each is one workgroup per CU).
int grid_bwd(int64_t E) {
  const int64_t tiles = (E + TR - 1) / TR;
  const int a = resident_grid(reinterpret_cast<const void*>(&depth_head_bwd_a_kernel), kThreadsD, 0, tiles,
                              kWavesD * kMinTiles);
  const int b = resident_grid(reinterpret_cast<const void*>(&depth_head_bwd_b_kernel), kThreadsD, 0, tiles,
                              kWavesD * kMinTiles);
  return a < b ? a : b;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int32_t gasfm_depth_head_part_shape(int64_t E, int32_t which, int32_t* cols) {
  if (cols) *cols = which ? PART_B : PART_A;
  if (E <= 0) return 0;
  return grid_bwd(E);
}

extern "C" int gasfm_depth_head_fwd(const float* P, int64_t E, const float* W1, const float* b1, const float* W2,
                                    const float* b2, const float* W3, const float* b3, float* d, void* stream) {
  GASFM_REQUIRE(E >= 0, "gasfm_depth_head_fwd: E < 0");
  if (E == 0) return GASFM_OK;
  GASFM_REQUIRE(P && W1 && b1 && W2 && b2 && W3 && b3 && d, "gasfm_depth_head_fwd: null pointer");
  GASFM_REQUIRE(aligned16(P) && aligned4(W1) && aligned4(b1) && aligned4(W2) && aligned4(b2) && aligned4(W3) &&
                    aligned4(b3) && aligned4(d),
                "gasfm_depth_head_fwd: misaligned pointer (P: 16 bytes, the others: 4)");
  hipLaunchKernelGGL(depth_head_fwd_kernel, dim3(grid_fwd(E)), dim3(kThreadsD), 0,
                     reinterpret_cast<hipStream_t>(stream), P, E, W1, b1, W2, b2, W3, b3, d);
  return launch_status("gasfm_depth_head_fwd");
}

extern "C" int gasfm_depth_head_bwd(const float* P, int64_t E, const float* W1, const float* b1, const float* W2,
                                    const float* b2, const float* W3, const float* dd, float* dP, float* part_a,
                                    float* part_b, void* stream) {
  GASFM_REQUIRE(E >= 0, "gasfm_depth_head_bwd: E < 0");
  if (E == 0) return GASFM_OK;
  GASFM_REQUIRE(P && W1 && b1 && W2 && b2 && W3 && dd && dP && part_a && part_b, "gasfm_depth_head_bwd: null pointer");
  GASFM_REQUIRE(aligned16(P) && aligned16(dP) && aligned4(W1) && aligned4(b1) && aligned4(W2) && aligned4(b2) &&
                    aligned4(W3) && aligned4(dd) && aligned4(part_a) && aligned4(part_b),
                "gasfm_depth_head_bwd: misaligned pointer (P, dP: 16 bytes, the others: 4)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_bwd(E);
  hipLaunchKernelGGL(depth_head_bwd_b_kernel, dim3(grid), dim3(kThreadsD), 0, st, P, E, W1, b1, W2, b2, W3, dd,
                     part_b);
  const int s = launch_status("gasfm_depth_head_bwd_b");
  if (s != GASFM_OK) return s;
  hipLaunchKernelGGL(depth_head_bwd_a_kernel, dim3(grid), dim3(kThreadsD), 0, st, P, E, W1, b1, W2, b2, W3, dd, dP,
                     part_a);
  return launch_status("gasfm_depth_head_bwd_a");
}
