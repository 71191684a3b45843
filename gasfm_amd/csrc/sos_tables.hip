// Per-step scene tables of a shape-stable union batch for SetOfSetNet (gasfm_amd/static_batch.py,
// setofset._Degrees), gfx950.
//
// The set-of-set layers of a union take the global mean, the global row and the centring vector per
// scene: they read each scene's row ranges, the scene of every row, max(E_s, 1) and deg / E_s per
// node.  For an eager union these come from the batch's host lists once; a bucket's contents change
// with every fill and a replayed graph reads nothing from the host, so here one launch writes them
// into buffers the bucket owns, from the static buffers the fill kernels have just written:
//   ptrc / ptrp [S + 1]  first camera / point row of each scene (lower bound of s in the sorted scene
//                        maps; an empty scene repeats the pointer; the last entry is M / N)
//   ptre [S + 1], Es [S] the edge offsets and max(E_s, 1)
//   deg / inv / w        per camera [M] and per point [N]: deg, 1 / deg (0 for deg == 0), deg / Es
//   sop [N], soe [E]     the scene of every point (widened) and edge row (the scene of its camera)
// Every output element is written by exactly one thread from the inputs alone (no atomics, no LDS):
// deterministic, and each fp64 value is one IEEE division of exactly representable integers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace gasfm {
namespace {

constexpr int kT = 256;

// first index in the non-decreasing key[0..n) with key[index] >= s
__device__ __forceinline__ int32_t lower_bound(const int32_t* __restrict__ key, int64_t n, int32_t s) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key[mid] < s) lo = mid + 1;
    else hi = mid;
  }
  return int32_t(lo);
}

// the scene id used as an index: held inside [0, S) whatever the map holds
__device__ __forceinline__ int32_t scene_index(int32_t s, int32_t S) { return s < 0 ? 0 : (s >= S ? S - 1 : s); }

__device__ __forceinline__ void node_row(const int32_t* __restrict__ ptr, const int32_t* __restrict__ scene,
                                         const int32_t* __restrict__ eoff, int32_t S, int64_t i, double* deg,
                                         double* inv, double* w) {
  const int32_t d = ptr[i + 1] - ptr[i];
  const int32_t s = scene_index(scene[i], S);
  const int32_t es = eoff[s + 1] - eoff[s];
  deg[i] = double(d);
  inv[i] = d > 0 ? 1.0 / double(d) : 0.0;
  w[i] = double(d) / double(es > 1 ? es : 1);
}

__global__ __launch_bounds__(kT) void sos_union_tables_kernel(gasfm_sos_tables t) {
  const int64_t nthr = int64_t(gridDim.x) * kT;
  int64_t hi = t.M > t.N ? t.M : t.N;
  hi = hi > t.E ? hi : t.E;
  hi = hi > t.S + 1 ? hi : t.S + 1;
  for (int64_t i = int64_t(blockIdx.x) * kT + threadIdx.x; i < hi; i += nthr) {
    if (i <= t.S) {
      t.ptrc[i] = lower_bound(t.soc32, t.M, int32_t(i));
      t.ptrp[i] = lower_bound(t.sop32, t.N, int32_t(i));
      t.ptre[i] = t.eoff[i];
    }
    if (i < t.S) {
      const int32_t es = t.eoff[i + 1] - t.eoff[i];
      t.Es[i] = double(es > 1 ? es : 1);
    }
    if (i < t.M) node_row(t.cam_ptr, t.soc32, t.eoff, t.S, i, t.degc, t.invc, t.wc);
    if (i < t.N) {
      node_row(t.pt_ptr, t.sop32, t.eoff, t.S, i, t.degp, t.invp, t.wp);
      t.sop[i] = t.sop32[i];
    }
    if (i < t.E) {
      const int32_t c = t.cam32[i];
      t.soe[i] = t.soc32[c < 0 ? 0 : (c >= t.M ? t.M - 1 : c)];
    }
  }
}

}  // namespace
}  // namespace gasfm

using namespace gasfm;

extern "C" int gasfm_sos_union_tables(const gasfm_sos_tables* t, void* stream) {
  GASFM_REQUIRE(t, "gasfm_sos_union_tables: null argument");
  GASFM_REQUIRE(t->S > 0 && t->M > 0 && t->N > 0 && t->E >= 0 && t->M < (int64_t(1) << 31) &&
                    t->N < (int64_t(1) << 31) && t->E < (int64_t(1) << 31),
                "gasfm_sos_union_tables: S=%d M=%lld N=%lld E=%lld", int(t->S), (long long)t->M, (long long)t->N,
                (long long)t->E);
  GASFM_REQUIRE(t->cam_ptr && t->pt_ptr && t->soc32 && t->sop32 && t->eoff && (t->cam32 || t->E == 0),
                "gasfm_sos_union_tables: null input");
  GASFM_REQUIRE(t->ptrc && t->ptrp && t->ptre && t->Es && t->degc && t->invc && t->wc && t->degp && t->invp &&
                    t->wp && t->sop && (t->soe || t->E == 0),
                "gasfm_sos_union_tables: null output");
  int64_t hi = t->M > t->N ? t->M : t->N;
  hi = hi > t->E ? hi : t->E;
  hi = hi > t->S + 1 ? hi : t->S + 1;
  int64_t blocks = (hi + kT - 1) / kT;
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(sos_union_tables_kernel, dim3(unsigned(blocks)), dim3(kT), 0,
                     reinterpret_cast<hipStream_t>(stream), *t);
  return launch_status("gasfm_sos_union_tables");
}
