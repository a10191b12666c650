// The neighbour radii and range counts under the Kraskov-Stoegbauer-Grassberger (KSG, estimator 1) mutual information of
// every (attribute, latent channel) pair on the device (gfx950); scikit-learn's _compute_mi_cc, its nextafter(radius, 0)
// rule and its counting of exact duplicates at radius 0 included.  For one pair of fp32 columns x (channel), y
// (attribute) and every row i:
//   dx_ij = |x_i - x_j|, dy_ij = |y_i - y_j|: ONE IEEE fp32 subtraction each (subnormal differences are kept: the kernels
//           run with the float mode hipcc gives them, float_denorm_mode_32 = 3), d_ij = max(dx_ij, dy_ij) for j != i;
//   eps_i = the k-th smallest d_ij over j != i, with multiplicity;
//   r_i   = the largest fp32 below eps_i (its bits minus one), 0 when eps_i == 0;
//   nx_i  = #{j != i : dx_ij <= r_i},  ny_i = #{j != i : dy_ij <= r_i}.
// The outputs are one of the distances and two counts: nothing is summed in floating point, so every cell is independent of
// the order of evaluation, of row padding and of what else is in the launch.  The library is built with -ffast-math; that
// gives the compiler nothing to re-associate here (a single subtraction, max, and ordinary compares of the results), and
// -fno-finite-math-only keeps the +inf the neighbour list starts from.  (tests/ksg_oracle.py is the plain restatement.)
//
// pti_ksg_counts, one launch: one 256-thread workgroup per (256-row tile, channel, attribute).  Thread t owns row
//   i = 256 tile + t.  Pass 1: the (x_j, y_j) run through LDS in tiles of 256 and come back as broadcast 16-byte reads, four j
//   per read; the K smallest d_ij stay in K registers, sorted, through a fully unrolled min / max chain (K is a template
//   argument: a list indexed at run time would live in scratch).  Above K = 4 the chain is entered only when d is below
//   the list's largest entry, which after the first tiles is rare for a whole wave.  Pass 2: the same tiles again, two
//   compares against r_i and two adds per j.  Self is left out BY INDEX: only the tile on the diagonal holds j == i, and
//   only that tile pays for the test.  No atomics, no workspace.
#include "pti_common.h"

namespace {

constexpr int KSG_TILE = 256;   // rows per workgroup = (x_j, y_j) per LDS tile = threads
constexpr int KSG_MAXN = 32768, KSG_MAXL = 16, KSG_MAXNA = 16, KSG_MAXK = 16;
constexpr int KSG_BRANCH_ABOVE = 4;

template <int K>
__device__ __forceinline__ void ksg_insert(float (&best)[K], float d) {
  if (K > KSG_BRANCH_ABOVE && !(d < best[K - 1])) return;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const float lo = fminf(best[t], d);
    d = fmaxf(best[t], d);
    best[t] = lo;
  }
}

template <int K, bool DIAG>
__device__ __forceinline__ void ksg_nearest_tile(const float* s_x, const float* s_y, int cnt, int self, float xi, float yi,
                                                 float (&best)[K]) {
  const float inf = __builtin_inff();
  int jb = 0;
  for (; jb + 4 <= cnt; jb += 4) {
    const f32x4 xj = *(const f32x4*)&s_x[jb];
    const f32x4 yj = *(const f32x4*)&s_y[jb];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float d = fmaxf(fabsf(xi - xj[u]), fabsf(yi - yj[u]));
      if (DIAG) d = jb + u == self ? inf : d;
      ksg_insert<K>(best, d);
    }
  }
  for (; jb < cnt; ++jb) {
    float d = fmaxf(fabsf(xi - s_x[jb]), fabsf(yi - s_y[jb]));
    if (DIAG) d = jb == self ? inf : d;
    ksg_insert<K>(best, d);
  }
}

template <bool DIAG>
__device__ __forceinline__ void ksg_count_tile(const float* s_x, const float* s_y, int cnt, int self, float xi, float yi,
                                               float r, int& nx, int& ny) {
  int jb = 0;
  for (; jb + 4 <= cnt; jb += 4) {
    const f32x4 xj = *(const f32x4*)&s_x[jb];
    const f32x4 yj = *(const f32x4*)&s_y[jb];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool other = !DIAG || jb + u != self;
      nx += (fabsf(xi - xj[u]) <= r && other) ? 1 : 0;
      ny += (fabsf(yi - yj[u]) <= r && other) ? 1 : 0;
    }
  }
  for (; jb < cnt; ++jb) {
    const bool other = !DIAG || jb != self;
    nx += (fabsf(xi - s_x[jb]) <= r && other) ? 1 : 0;
    ny += (fabsf(yi - s_y[jb]) <= r && other) ? 1 : 0;
  }
}

template <int K>
__global__ __launch_bounds__(KSG_TILE) void ksg_counts_kernel(const float* __restrict__ zt, long long ldz,
                                                              const float* __restrict__ attrs, long long lda, int n, int l,
                                                              float* __restrict__ eps, int* __restrict__ nx_out,
                                                              int* __restrict__ ny_out) {
  __shared__ __attribute__((aligned(16))) float s_x[KSG_TILE];
  __shared__ __attribute__((aligned(16))) float s_y[KSG_TILE];
  const int tid = threadIdx.x, i0 = blockIdx.x * KSG_TILE, i = i0 + tid, c = blockIdx.y, q = blockIdx.z;
  const float* __restrict__ x = zt + (long long)c * ldz;
  const float* __restrict__ y = attrs + (long long)q * lda;
  const bool live = i < n;
  const float xi = live ? x[i] : 0.f, yi = live ? y[i] : 0.f;   // a thread past the end computes on zeros and stores nothing

  float best[K];
#pragma unroll
  for (int t = 0; t < K; ++t) best[t] = __builtin_inff();
  for (int j0 = 0; j0 < n; j0 += KSG_TILE) {
    __syncthreads();   // the previous tile has been read
    if (j0 + tid < n) {
      s_x[tid] = x[j0 + tid];
      s_y[tid] = y[j0 + tid];
    }
    __syncthreads();
    const int cnt = min(KSG_TILE, n - j0);   // entries at and past cnt are never read
    if (j0 == i0) ksg_nearest_tile<K, true>(s_x, s_y, cnt, tid, xi, yi, best);
    else ksg_nearest_tile<K, false>(s_x, s_y, cnt, tid, xi, yi, best);
  }
  const float e = best[K - 1];   // k <= n - 1 real neighbours: a distance, never the list's initial value
  const unsigned eb = __float_as_uint(e);
  const float r = __uint_as_float(eb > 0u ? eb - 1u : 0u);   // e >= 0 and not a NaN: its bits order like its value

  int nx = 0, ny = 0;
  for (int j0 = 0; j0 < n; j0 += KSG_TILE) {
    __syncthreads();
    if (j0 + tid < n) {
      s_x[tid] = x[j0 + tid];
      s_y[tid] = y[j0 + tid];
    }
    __syncthreads();
    const int cnt = min(KSG_TILE, n - j0);
    if (j0 == i0) ksg_count_tile<true>(s_x, s_y, cnt, tid, xi, yi, r, nx, ny);
    else ksg_count_tile<false>(s_x, s_y, cnt, tid, xi, yi, r, nx, ny);
  }
  if (live) {
    const long long o = ((long long)q * l + c) * n + i;
    eps[o] = e;
    nx_out[o] = nx;
    ny_out[o] = ny;
  }
}

template <int K>
void ksg_launch(dim3 grid, hipStream_t s, const float* zt, long long ldz, const float* attrs, long long lda, int n, int l,
                float* eps, int* nx, int* ny) {
  PTI_LAUNCH(ksg_counts_kernel<K>, grid, dim3(KSG_TILE), 0, s, zt, ldz, attrs, lda, n, l, eps, nx, ny);
}

}  // namespace

extern "C" int pti_ksg_counts(const float* zt, int64_t ldz, const float* attrs, int64_t lda, int n, int l, int na, int k,
                              float* eps, int32_t* nx, int32_t* ny, pti_stream_t s) {
  if (!zt || !attrs || !eps || !nx || !ny) PTI_FAIL(PTI_EINVAL, "ksg_counts: null pointer");
  if (k < 1 || l < 1 || na < 1 || n < k + 1)
    PTI_FAIL(PTI_EINVAL, "ksg_counts: bad shape n=%d l=%d na=%d k=%d (k, l, na >= 1, n >= k + 1)", n, l, na, k);
  if (k > KSG_MAXK || n > KSG_MAXN || l > KSG_MAXL || na > KSG_MAXNA)
    PTI_FAIL(PTI_EUNSUPPORTED, "ksg_counts: unsupported shape n=%d l=%d na=%d k=%d (n <= %d, l <= %d, na <= %d, k <= %d)", n, l,
             na, k, KSG_MAXN, KSG_MAXL, KSG_MAXNA, KSG_MAXK);
  if (ldz < n || lda < n)
    PTI_FAIL(PTI_EINVAL, "ksg_counts: row stride below n (ldz=%lld lda=%lld n=%d)", (long long)ldz, (long long)lda, n);
  if (((uintptr_t)zt & 3) || ((uintptr_t)attrs & 3) || ((uintptr_t)eps & 3) || ((uintptr_t)nx & 3) || ((uintptr_t)ny & 3))
    PTI_FAIL(PTI_EINVAL, "ksg_counts: misaligned buffer");
  typedef void (*launch_t)(dim3, hipStream_t, const float*, long long, const float*, long long, int, int, float*, int*, int*);
  static const launch_t launch[KSG_MAXK] = {ksg_launch<1>,  ksg_launch<2>,  ksg_launch<3>,  ksg_launch<4>,
                                            ksg_launch<5>,  ksg_launch<6>,  ksg_launch<7>,  ksg_launch<8>,
                                            ksg_launch<9>,  ksg_launch<10>, ksg_launch<11>, ksg_launch<12>,
                                            ksg_launch<13>, ksg_launch<14>, ksg_launch<15>, ksg_launch<16>};
  launch[k - 1](dim3((unsigned)cdiv(n, KSG_TILE), (unsigned)l, (unsigned)na), (hipStream_t)s, zt, (long long)ldz, attrs,
                (long long)lda, n, l, eps, (int*)nx, (int*)ny);
  PTI_CHECK_LAUNCH("ksg_counts");
  return PTI_OK;
}
