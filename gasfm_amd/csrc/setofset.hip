// Set-of-set (DPESFM baseline) layer kernels: width-general segment sums and the edge update's
// three products over the E edge rows on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
//
//   Y[e] = act((X[e] W^T + S[pt[e]] + V[cam[e]]) / 4 - cmean (+ R[e]))          gasfm_sos_edge_fwd
//   dX[e] = (mask . dY / 4)[e] W + A[cam[e]] + B[pt[e]]                          gasfm_sos_edge_dx
//   dW = (mask . dY / 4)^T X, split over E, partial matrices for gasfm_colsum    gasfm_sos_edge_dw
//   out[seg] = scale / deg(seg) * sum of (masked) rows of a plan segment         gasfm_sos_segment_sum
//
// The bias and the global row are folded into V by the caller (node-sized), cmean is the
// centring vector computed from node-sized quantities, the ReLU mask is Y > 0 of the layer's own
// output.  Everything is deterministic: no float atomics, fixed summation orders.
//
// Row-tile GEMM (forward and dX): a workgroup of 4 waves owns BM rows and all N <= 256 output
// columns; K runs in chunks of 32 staged in LDS (A chunk [BM][32], weight chunk [N][32] or
// [32][N]); each wave holds 64 rows x NCT 16-column tiles of accumulators and reuses every LDS
// operand for 4 (A) or NCT (B) MFMAs.  The weight chunk is re-read from L2 per row tile (the
// whole [256, 256] weight does not fit LDS next to the row tile).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace gasfm {
namespace sos {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int KC = 32;       // K chunk
constexpr int LDK = KC + 4;  // row stride of a [rows][KC] LDS tile (16-byte aligned rows)

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

struct Epilogue {
  const int32_t* cam;  // [E]
  const int32_t* pt;   // [E]
  const float* Gp;     // [n, N] rows gathered by pt, or null
  const float* Gc;     // [m, N] rows gathered by cam, or null
  const float* cvec;   // [N] subtracted after the scale, or null
  const float* R;      // [E, ldR] residual added last, or null
  int64_t ldR;
  float scale;         // out = scale * (acc + Gp + Gc) - cvec + R
  int relu;
};

#define kOnes make_float4(1.f, 1.f, 1.f, 1.f)  // the mask of a layer without a ReLU

__device__ __forceinline__ float4 masked(float4 v, float4 y, float s) {
  // ReLU backward: the gradient passes where the output is > 0 (a NaN output passes nothing on,
  // as torch's threshold backward does)
  v.x = y.x > 0.f ? v.x * s : 0.f;
  v.y = y.y > 0.f ? v.y * s : 0.f;
  v.z = y.z > 0.f ? v.z * s : 0.f;
  v.w = y.w > 0.f ? v.w * s : 0.f;
  return v;
}

// out[E, N] = epilogue(Aop[E, K] Bop[K, N]); Aop = A, or mask(A, Ym) * ascale when Ym != null.
// BT: Bop[k][j] = W[j * ldW + k] (forward: W is [N, K]); else Bop[k][j] = W[k * ldW + j] (dX).
// WM x WN waves, each 64 rows x NCT 16-column tiles.  K % 32 == 0 or K < 32 (scalar loads);
// N % 4 == 0 or N < 16 (scalar loads).
template <bool BT, int WM, int WN, int NCT>
__global__ __launch_bounds__(kThreads) void gemm_rows_kernel(const float* __restrict__ A, int64_t ldA,
                                                             const float* __restrict__ Ym, int64_t ldY, float ascale,
                                                             const float* __restrict__ W, int64_t ldW, int64_t E,
                                                             int K, int N, float* __restrict__ out, int64_t ldO,
                                                             Epilogue ep, int64_t ntiles) {
  constexpr int BM = WM * 64, BN = WN * NCT * 16;
  constexpr int LDB = BT ? LDK : BN + 8;
  __shared__ __attribute__((aligned(16))) float As[BM * LDK];
  __shared__ __attribute__((aligned(16))) float Bs[BT ? BN * LDK : KC * LDB];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wr = wave / WN, wc = wave % WN;
  const int li = lane & 15, lg = lane >> 4;
  const bool vecK = (K % KC) == 0;
  const bool vecN = (N % 4) == 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * BM;
    f32x4 acc[4][NCT];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += KC) {
      __syncthreads();
      // ---- A chunk [BM][KC]
      if (vecK) {
#pragma unroll 4
        for (int q = tid; q < BM * (KC / 4); q += kThreads) {
          const int r = q / (KC / 4), c = (q % (KC / 4)) * 4;
          const int64_t e = row0 + r;
          const int64_t ec = e < E ? e : E - 1;
          float4 v = *reinterpret_cast<const float4*>(A + ec * ldA + k0 + c);
          v = masked(v, Ym ? *reinterpret_cast<const float4*>(Ym + ec * ldY + k0 + c) : kOnes, ascale);
          if (e >= E) v = make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4*>(As + r * LDK + c) = v;
        }
      } else {
        for (int q = tid; q < BM * KC; q += kThreads) {
          const int r = q / KC, c = q % KC;
          const int64_t e = row0 + r;
          float v = 0.f;
          if (e < E && k0 + c < K) {
            v = A[e * ldA + k0 + c] * ascale;
            if (Ym) v = Ym[e * ldY + k0 + c] > 0.f ? v : 0.f;
          }
          As[r * LDK + c] = v;
        }
      }
      // ---- weight chunk
      if (BT) {  // Bs[j][k] = W[j][k0 + k]
        if (vecK) {
#pragma unroll 4
          for (int q = tid; q < BN * (KC / 4); q += kThreads) {
            const int j = q / (KC / 4), c = (q % (KC / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < N) v = *reinterpret_cast<const float4*>(W + int64_t(j) * ldW + k0 + c);
            *reinterpret_cast<float4*>(Bs + j * LDB + c) = v;
          }
        } else {
          for (int q = tid; q < BN * KC; q += kThreads) {
            const int j = q / KC, c = q % KC;
            Bs[j * LDB + c] = (j < N && k0 + c < K) ? W[int64_t(j) * ldW + k0 + c] : 0.f;
          }
        }
      } else {  // Bs[k][j] = W[k0 + k][j]
        if (vecN) {
#pragma unroll 4
          for (int q = tid; q < KC * (BN / 4); q += kThreads) {
            const int k = q / (BN / 4), c = (q % (BN / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + k < K && c < N) v = *reinterpret_cast<const float4*>(W + int64_t(k0 + k) * ldW + c);
            *reinterpret_cast<float4*>(Bs + k * LDB + c) = v;
          }
        } else {
          for (int q = tid; q < KC * BN; q += kThreads) {
            const int k = q / BN, c = q % BN;
            Bs[k * LDB + c] = (k0 + k < K && c < N) ? W[int64_t(k0 + k) * ldW + c] : 0.f;
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float a[4], b[NCT];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) a[rt] = As[(wr * 64 + rt * 16 + li) * LDK + kk + lg];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const int j = (wc * NCT + ct) * 16 + li;
          b[ct] = BT ? Bs[j * LDB + kk + lg] : Bs[(kk + lg) * LDB + j];
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = mfma16(a[rt], b[ct], acc[rt][ct]);
      }
    }
    // ---- epilogue: C[row = 4 lg + r][col = li] of every 16 x 16 tile
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t e = row0 + wr * 64 + rt * 16 + 4 * lg + r;
        if (e >= E) continue;
        const int64_t p = ep.Gp ? ep.pt[e] : 0;
        const int64_t c = ep.Gc ? ep.cam[e] : 0;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const int col = (wc * NCT + ct) * 16 + li;
          if (col >= N) continue;
          float v = acc[rt][ct][r];
          if (ep.Gp) v += ep.Gp[p * N + col];
          if (ep.Gc) v += ep.Gc[c * N + col];
          v *= ep.scale;
          if (ep.cvec) v -= ep.cvec[col];
          if (ep.R) v += ep.R[e * ep.ldR + col];
          if (ep.relu) v = v < 0.f ? 0.f : v;  // keeps a NaN, as torch's relu does
          out[e * ldO + col] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- dW = T^T X over a range of E
// part[s][i][j] = sum over e in split s of T[e][i] X[e][j], T = mask(dY, Ym) * ascale.
// grid (output tiles, splits); WM x WN waves, each TI x TJ 16 x 16 tiles; 32 edges per LDS chunk.
constexpr int KE = 32;

template <int WM, int WN, int TI, int TJ>
__global__ __launch_bounds__(kThreads) void dw_kernel(const float* __restrict__ dY, int64_t ldD,
                                                      const float* __restrict__ Ym, int64_t ldY, float ascale,
                                                      const float* __restrict__ X, int64_t ldX, int64_t E, int M,
                                                      int N, int tiles_j, float* __restrict__ part) {
  constexpr int BI = WM * TI * 16, BJ = WN * TJ * 16;
  constexpr int LDT = BI + 8, LDX = BJ + 8;
  __shared__ __attribute__((aligned(16))) float Ts[KE * LDT];
  __shared__ __attribute__((aligned(16))) float Xs[KE * LDX];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 15, lg = lane >> 4;
  const int i0 = (int(blockIdx.x) / tiles_j) * BI, j0 = (int(blockIdx.x) % tiles_j) * BJ;
  const int S = gridDim.y, s = blockIdx.y;
  const int64_t e0 = E * s / S, e1 = E * (s + 1) / S;
  const bool vecN = (N % 4) == 0;
  f32x4 acc[TI][TJ];
#pragma unroll
  for (int a = 0; a < TI; ++a)
#pragma unroll
    for (int b = 0; b < TJ; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t eb = e0; eb < e1; eb += KE) {
    __syncthreads();
#pragma unroll 4
    for (int q = tid; q < KE * (BI / 4); q += kThreads) {  // M % 4 == 0
      const int k = q / (BI / 4), c = (q % (BI / 4)) * 4;
      const int64_t e = eb + k;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < e1 && i0 + c < M) {
        v = *reinterpret_cast<const float4*>(dY + e * ldD + i0 + c);
        v = masked(v, Ym ? *reinterpret_cast<const float4*>(Ym + e * ldY + i0 + c) : kOnes, ascale);
      }
      *reinterpret_cast<float4*>(Ts + k * LDT + c) = v;
    }
    if (vecN) {
#pragma unroll 4
      for (int q = tid; q < KE * (BJ / 4); q += kThreads) {
        const int k = q / (BJ / 4), c = (q % (BJ / 4)) * 4;
        const int64_t e = eb + k;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < e1 && j0 + c < N) v = *reinterpret_cast<const float4*>(X + e * ldX + j0 + c);
        *reinterpret_cast<float4*>(Xs + k * LDX + c) = v;
      }
    } else {
      for (int q = tid; q < KE * BJ; q += kThreads) {
        const int k = q / BJ, c = q % BJ;
        const int64_t e = eb + k;
        Xs[k * LDX + c] = (e < e1 && j0 + c < N) ? X[e * ldX + j0 + c] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KE; kk += 4) {
      float a[TI], b[TJ];
#pragma unroll
      for (int t = 0; t < TI; ++t) a[t] = Ts[(kk + lg) * LDT + (wm * TI + t) * 16 + li];
#pragma unroll
      for (int t = 0; t < TJ; ++t) b[t] = Xs[(kk + lg) * LDX + (wn * TJ + t) * 16 + li];
#pragma unroll
      for (int ta = 0; ta < TI; ++ta)
#pragma unroll
        for (int tb = 0; tb < TJ; ++tb) acc[ta][tb] = mfma16(a[ta], b[tb], acc[ta][tb]);
    }
  }
  float* P = part + int64_t(s) * M * N;
#pragma unroll
  for (int ta = 0; ta < TI; ++ta)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + (wm * TI + ta) * 16 + 4 * lg + r;
      if (i >= M) continue;
#pragma unroll
      for (int tb = 0; tb < TJ; ++tb) {
        const int j = j0 + (wn * TJ + tb) * 16 + li;
        if (j < N) P[int64_t(i) * N + j] = acc[ta][tb][r];
      }
    }
}

// ---------------------------------------------------------------- segment sums, any width
// One wave per work item.  D >= 4 (D % 4 == 0): lpr lanes (a power of two >= D / 4) hold a row's
// float4 chunks, 64 / lpr rows per step, four steps in flight, then an xor butterfly over the
// row groups (fixed order).  D == 2: one float2 row per lane.  Complete items write out[seg],
// split items part[slot]; both scaled by scale (/ deg(seg) when seg_ptr is given).
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__global__ __launch_bounds__(kThreads) void segsum_kernel(const gasfm_work_item* __restrict__ items, int n_items,
                                                          const int32_t* __restrict__ perm,
                                                          const float* __restrict__ X, int64_t ldX,
                                                          const float* __restrict__ Ym, int64_t ldY, int D, int lpr,
                                                          float scale, const int32_t* __restrict__ seg_ptr,
                                                          float* __restrict__ out, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), nw = gridDim.x * (kThreads / 64);
  for (int it = wid; it < n_items; it += nw) {
    const gasfm_work_item w = items[it];
    float s = scale;
    if (seg_ptr) {
      const int deg = seg_ptr[w.seg + 1] - seg_ptr[w.seg];
      s = deg > 0 ? scale / float(deg) : 0.f;
    }
    float* dst = w.slot < 0 ? out + int64_t(w.seg) * D : part + int64_t(w.slot) * D;
    if (D == 2) {
      float2 acc = make_float2(0.f, 0.f);
      for (int j = w.begin + lane; j < w.end; j += 64) {
        const int64_t r = perm ? perm[j] : j;
        float2 v = *reinterpret_cast<const float2*>(X + r * ldX);
        if (Ym) {
          const float2 y = *reinterpret_cast<const float2*>(Ym + r * ldY);
          v.x = y.x > 0.f ? v.x : 0.f;
          v.y = y.y > 0.f ? v.y : 0.f;
        }
        acc.x += v.x;
        acc.y += v.y;
      }
      for (int m = 1; m < 64; m <<= 1) {
        acc.x += __shfl_xor(acc.x, m);
        acc.y += __shfl_xor(acc.y, m);
      }
      if (lane == 0) *reinterpret_cast<float2*>(dst) = make_float2(acc.x * s, acc.y * s);
      continue;
    }
    const int c4 = lane % lpr, rg = lane / lpr, RS = 64 / lpr;
    const bool active = c4 * 4 < D;
    float4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j0 = w.begin + rg; j0 < w.end; j0 += 4 * RS) {
      float4 v[4], y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u * RS;
        const int jc = j < w.end ? j : j0;
        const int64_t r = perm ? perm[jc] : jc;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        y[u] = make_float4(1.f, 1.f, 1.f, 1.f);
        if (active) {
          v[u] = *reinterpret_cast<const float4*>(X + r * ldX + c4 * 4);
          if (Ym) y[u] = *reinterpret_cast<const float4*>(Ym + r * ldY + c4 * 4);
        }
        if (j >= w.end) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = add4(acc[u], masked(v[u], y[u], 1.f));
    }
    float4 t = add4(add4(acc[0], acc[1]), add4(acc[2], acc[3]));
    for (int m = lpr; m < 64; m <<= 1) {
      t.x += __shfl_xor(t.x, m);
      t.y += __shfl_xor(t.y, m);
      t.z += __shfl_xor(t.z, m);
      t.w += __shfl_xor(t.w, m);
    }
    if (rg == 0 && active) *reinterpret_cast<float4*>(dst + c4 * 4) = make_float4(t.x * s, t.y * s, t.z * s, t.w * s);
  }
}

static bool width_ok(int d) { return d == 2 || (d >= 32 && d <= 256 && d % 32 == 0); }

template <bool BT, int WM, int WN, int NCT>
static int launch_gemm(const float* A, int64_t ldA, const float* Ym, int64_t ldY, float ascale, const float* W,
                       int64_t ldW, int64_t E, int K, int N, float* out, int64_t ldO, const Epilogue& ep,
                       hipStream_t st) {
  const int64_t ntiles = (E + WM * 64 - 1) / (WM * 64);
  auto fn = gemm_rows_kernel<BT, WM, WN, NCT>;
  const int g = resident_grid(reinterpret_cast<const void*>(fn), kThreads, 0, ntiles, 1);
  hipLaunchKernelGGL(fn, dim3(g), dim3(kThreads), 0, st, A, ldA, Ym, ldY, ascale, W, ldW, E, K, N, out, ldO, ep,
                     ntiles);
  return launch_status("gasfm_sos_edge gemm");
}

template <bool BT>
static int dispatch_gemm(const float* A, int64_t ldA, const float* Ym, int64_t ldY, float ascale, const float* W,
                         int64_t ldW, int64_t E, int K, int N, float* out, int64_t ldO, const Epilogue& ep,
                         hipStream_t st) {
#define GASFM_SOS_CASE(n)                                                                                      \
  case n:                                                                                                      \
    return launch_gemm<BT, 2, 2, n>(A, ldA, Ym, ldY, ascale, W, ldW, E, K, N, out, ldO, ep, st)
  if (N < 16) return launch_gemm<BT, 4, 1, 1>(A, ldA, Ym, ldY, ascale, W, ldW, E, K, N, out, ldO, ep, st);
  switch (N / 32) {
    GASFM_SOS_CASE(1);
    GASFM_SOS_CASE(2);
    GASFM_SOS_CASE(3);
    GASFM_SOS_CASE(4);
    GASFM_SOS_CASE(5);
    GASFM_SOS_CASE(6);
    GASFM_SOS_CASE(7);
    GASFM_SOS_CASE(8);
  }
#undef GASFM_SOS_CASE
  set_error("gasfm_sos_edge: unsupported width %d", N);
  return GASFM_ERR_UNSUPPORTED;
}

static int dw_tiles(int M, int N, int* tiles_j) {
  const int bi = N < 16 ? 256 : 128, bj = N < 16 ? 16 : 128;
  *tiles_j = (N + bj - 1) / bj;
  return ((M + bi - 1) / bi) * *tiles_j;
}

}  // namespace sos
}  // namespace gasfm

using namespace gasfm;
using namespace gasfm::sos;

extern "C" int32_t gasfm_sos_width_ok(int32_t d_in, int32_t d_out) {
  return width_ok(d_in) && width_ok(d_out) && d_out != 2 ? 1 : 0;
}

extern "C" int32_t gasfm_sos_row_tile(int32_t n_cols) { return n_cols < 16 ? 256 : 128; }

extern "C" int gasfm_sos_segment_sum(const gasfm_work_item* items, int32_t n_items, const int32_t* perm,
                                     const float* X, int64_t ldX, const float* Ym, int64_t ldY, int32_t D,
                                     float scale, const int32_t* seg_ptr, float* out, float* part, void* stream) {
  GASFM_REQUIRE(width_ok(D), "gasfm_sos_segment_sum: width %d", D);
  if (n_items <= 0) return GASFM_OK;
  GASFM_REQUIRE(items && X && out, "gasfm_sos_segment_sum: null pointer");
  const bool al = D == 2 ? (reinterpret_cast<uintptr_t>(X) % 8 == 0 && ldX % 2 == 0 &&
                            (!Ym || (reinterpret_cast<uintptr_t>(Ym) % 8 == 0 && ldY % 2 == 0)))
                         : (aligned16(X) && ldX % 4 == 0 && aligned16(out) && (!part || aligned16(part)) &&
                            (!Ym || (aligned16(Ym) && ldY % 4 == 0)));
  GASFM_REQUIRE(al, "gasfm_sos_segment_sum: alignment");
  int lpr = 1;
  while (lpr * 4 < D) lpr <<= 1;
  auto fn = segsum_kernel;
  const int g = resident_grid(reinterpret_cast<const void*>(fn), kThreads, 0, n_items, kThreads / 64);
  hipLaunchKernelGGL(fn, dim3(g), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), items, n_items, perm, X,
                     ldX, Ym, ldY, D, lpr, scale, seg_ptr, out, part);
  note_dispatch(GASFM_K_SOS_SEGSUM);
  return launch_status("gasfm_sos_segment_sum");
}

extern "C" int gasfm_sos_edge_fwd(const float* X, int64_t ldX, const float* W, int64_t E, int32_t d_in,
                                  int32_t d_out, const int32_t* cam, const int32_t* pt, const float* S,
                                  const float* V, const float* cmean, const float* R, int64_t ldR, int32_t relu,
                                  float* Y, void* stream) {
  GASFM_REQUIRE(gasfm_sos_width_ok(d_in, d_out), "gasfm_sos_edge_fwd: widths %d -> %d", d_in, d_out);
  if (E <= 0) return GASFM_OK;
  GASFM_REQUIRE(X && W && cam && pt && S && V && Y, "gasfm_sos_edge_fwd: null pointer");
  GASFM_REQUIRE(d_in == 2 || (aligned16(X) && ldX % 4 == 0 && aligned16(W)), "gasfm_sos_edge_fwd: alignment");
  const Epilogue ep{cam, pt, S, V, cmean, R, ldR, 0.25f, relu};
  note_dispatch(GASFM_K_SOS_EDGE_FWD);
  return dispatch_gemm<true>(X, ldX, nullptr, 0, 1.f, W, d_in, E, d_in, d_out, Y, d_out, ep,
                             reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gasfm_sos_edge_dx(const float* dY, const float* Ym, const float* W, int64_t E, int32_t d_in,
                                 int32_t d_out, const int32_t* cam, const int32_t* pt, const float* Ac,
                                 const float* Bp, float* dX, void* stream) {
  GASFM_REQUIRE(width_ok(d_in) && (d_out == 0 || (width_ok(d_out) && d_out != 2)),
                "gasfm_sos_edge_dx: widths %d -> %d", d_in, d_out);
  if (E <= 0) return GASFM_OK;
  GASFM_REQUIRE(dX && cam && pt && (d_out == 0 || (dY && W)), "gasfm_sos_edge_dx: null pointer");
  GASFM_REQUIRE(d_out == 0 || (aligned16(dY) && (!Ym || aligned16(Ym)) && (d_in == 2 || aligned16(W))),
                "gasfm_sos_edge_dx: alignment");
  const Epilogue ep{cam, pt, Bp, Ac, nullptr, nullptr, 0, 1.f, 0};
  note_dispatch(GASFM_K_SOS_EDGE_DX);
  return dispatch_gemm<false>(dY, d_out, Ym, d_out, 0.25f, W, d_in, E, d_out, d_in, dX, d_in, ep,
                              reinterpret_cast<hipStream_t>(stream));
}

extern "C" int32_t gasfm_sos_dw_splits(int64_t E, int32_t d_in, int32_t d_out) {
  int tj = 1;
  const int tiles = dw_tiles(d_out, d_in, &tj);
  int64_t s = (E + 1023) / 1024;
  const int64_t cap = 512 / tiles > 1 ? 512 / tiles : 1;
  if (s > cap) s = cap;
  return int32_t(s < 1 ? 1 : s);
}

extern "C" int gasfm_sos_edge_dw(const float* dY, const float* Ym, const float* X, int64_t ldX, int64_t E,
                                 int32_t d_in, int32_t d_out, int32_t splits, float* part, void* stream) {
  GASFM_REQUIRE(gasfm_sos_width_ok(d_in, d_out) && splits >= 1, "gasfm_sos_edge_dw: widths %d -> %d, splits %d",
                d_in, d_out, splits);
  GASFM_REQUIRE(part && (E == 0 || (dY && X)), "gasfm_sos_edge_dw: null pointer");
  GASFM_REQUIRE(E == 0 || (aligned16(dY) && (!Ym || aligned16(Ym)) && (d_in == 2 || (aligned16(X) && ldX % 4 == 0))),
                "gasfm_sos_edge_dw: alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int tj = 1;
  const int tiles = dw_tiles(d_out, d_in, &tj);
  note_dispatch(GASFM_K_SOS_EDGE_DW);
  if (d_in < 16) {
    hipLaunchKernelGGL((dw_kernel<4, 1, 4, 1>), dim3(tiles, splits), dim3(kThreads), 0, st, dY, int64_t(d_out), Ym,
                       int64_t(d_out), 0.25f, X, ldX, E, d_out, d_in, tj, part);
  } else {
    hipLaunchKernelGGL((dw_kernel<2, 2, 4, 4>), dim3(tiles, splits), dim3(kThreads), 0, st, dY, int64_t(d_out), Ym,
                       int64_t(d_out), 0.25f, X, ldX, E, d_out, d_in, tj, part);
  }
  return launch_status("gasfm_sos_edge_dw");
}
