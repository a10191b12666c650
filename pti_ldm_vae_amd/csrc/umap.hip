// UMAP on the device (gfx950) for the latent-space analysis: the k nearest neighbours of a distance matrix, umap-learn's
// smooth_knn_dist / compute_membership_strengths / fuzzy union as a thresholded CSR graph with an integer edge schedule,
// and one layout epoch in buffered (Jacobi) form.  3 <= N <= 8192, 2 <= k <= 256, k < N, two output columns, at most 2000
// epochs.  DESIGN.md 5l.
//
//   pti_umap_knn, one launch: one 256-thread workgroup per row.  Every entry becomes one 64-bit key in LDS
//     (neighbor_order_key, pti_common.h: integer order is the order (distance, column) and no two keys are equal).  With m = the power of two >= k: a bitonic network sorts every run of m keys (alternating
//     directions), then log2(N / m) rounds keep the m smallest of two neighbouring runs (element-wise minimum of an
//     ascending and a descending run: a bitonic run that holds them) and merge that run again.  Each round halves the
//     data, so the cost is that of sorting runs of m, not of sorting the row.  Comparisons only: exact.
//   pti_umap_graph, one memset and eight launches:
//     1. umap_rowsum_kernel / umap_mean_kernel: the fp64 sum of every row's k distances and the mean of all of them.
//     2. umap_sigma_kernel: one wavefront per row.  rho = the smallest non-zero distance; sigma by umap-learn's search in
//        fp64 (from 1, doubling while no upper bound is known, bisecting after, at most 64 rounds, stop at
//        |sum - log2 k| < 1e-5); every sum lane-strided in ascending order and folded by xor shuffles, so all lanes hold
//        the same bits and the search is wave-uniform.  Then the floor 1e-3 * mean, and the membership strengths as fp32
//        into the zeroed dense [N][N] scratch.
//     3. umap_union_kernel: w = a + a^T - a o a^T in place, one workgroup per PAIR of mirrored 32x32 tiles; the sum and
//        the product are commutative and taken in fp64, so w is symmetric bit for bit.  Per tile pair the largest w.
//     4. umap_wmax_kernel folds those maxima (a maximum has no order).
//     5. umap_count_kernel (entries of each row with w > 0 and w * n_epochs >= wmax), umap_scan_kernel (one workgroup:
//        the exclusive scan, indptr), umap_fill_kernel (one workgroup per row walks the columns in ascending blocks of
//        256 and places the kept ones by wave ballots and a running offset: ascending columns, no atomics).  A row's
//        length is whatever it is -- a point can be every other point's neighbour.  rate = floor(w * 2^20 / wmax),
//        the fp64 quotient corrected by two exact products, since the division itself is not correctly rounded under
//        the build's fast-math flags.
//   pti_umap_epoch, one launch: one wavefront per vertex, four per workgroup, lane-strided over the vertex's CSR row.  An
//     edge at position p fires in epoch e iff ((e + 1) rate >> 20) > (e rate >> 20).  Per fired edge the attraction
//     (doubled: the mirrored edge fires in the same epoch and would move this end by the same amount) and
//     negative_sample_rate repulsions from vertices drawn by lowbias32(lowbias32(seed + e) ^ (p * rate + s)).  The
//     coefficients, the clipped moves and their sums are fp64 (exp / log in fp64: an fp32 power under fast-math costs
//     more digits than the whole rest of the epoch); lanes are folded by xor shuffles; y_out = fp32(y_in + alpha * sum).
//   The transform (new rows into a fitted embedding): pti_umap_knn_cross is the kNN kernel over the [m][n]
//     distances from new rows to training rows; pti_umap_transform_graph is umap-learn's transform preamble on the regular
//     [m][k] slab (rho = 0, the same fp64 search, bipartite strengths, rates, the weighted-mean start point) in five small
//     launches; pti_umap_transform_layout runs ALL epochs in one launch, one wavefront per new row, against the frozen
//     training embedding.
// No floating-point atomics, no atomics at all; every sum has one order: results are bitwise reproducible.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int UM_MIN_N = 3;
constexpr int UM_MAX_N = 8192;
constexpr int UM_MAX_K = 256;
constexpr int UM_MAX_EPOCHS = 2000;
constexpr int UM_MAX_NEG = 64;
constexpr int UM_THREADS = 256;
constexpr int UM_TILE = 32;

typedef unsigned long long um_key;

// sum over a 256-thread workgroup, to every thread; compiles to ((w0 + w1) + w2) + w3 as written: not block_sum<4>, whose
// loop compiles to another order of these adds here (pti_common.h)
__device__ __forceinline__ double um_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  const double w = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = w;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ void um_exchange(um_key* key, int lo, int hi, bool ascending) {
  const um_key a = key[lo], b = key[hi];
  if ((a > b) == ascending) {
    key[lo] = b;
    key[hi] = a;
  }
}

// ---- neighbours ---------------------------------------------------------------------------------------------------
// np2 = the power of two >= max(n, m), m = 1 << lm = the power of two >= k
__global__ __launch_bounds__(UM_THREADS) void umap_knn_kernel(const float* __restrict__ dist, long long ldd, int n, int k,
                                                              int lm, int np2, int* __restrict__ knn_idx,
                                                              float* __restrict__ knn_dist) {
  extern __shared__ __attribute__((aligned(16))) um_key key[];
  const int i = blockIdx.x, tid = threadIdx.x, m = 1 << lm;
  for (int j = tid; j < np2; j += UM_THREADS) {
    um_key v = ~0ull;                                    // padding sorts last
    if (j < n) v = neighbor_order_key(dist[(long long)i * ldd + j], j);
    key[j] = v;
  }
  __syncthreads();
  // runs of m, run c ascending for even c
  for (int sz = 2; sz <= m; sz <<= 1)
    for (int j = sz >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < np2 / 2; t += UM_THREADS) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        um_exchange(key, lo, lo + j, (lo & sz) == 0);
      }
      __syncthreads();
    }
  // the m smallest of two neighbouring runs, merged; the survivors sit at multiples of 2 * stride
  for (int stride = m; stride < np2; stride <<= 1) {
    const int pairs = np2 / (2 * stride);
    for (int t = tid; t < pairs << lm; t += UM_THREADS) {
      const int base = 2 * stride * (t >> lm), e = t & (m - 1);
      const um_key b = key[base + stride + e];
      if (b < key[base + e]) key[base + e] = b;
    }
    __syncthreads();
    for (int j = m >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < pairs << (lm - 1); t += UM_THREADS) {
        const int q = t >> (lm - 1), e = t & ((m >> 1) - 1);
        const int lo = 2 * stride * q + (((e & ~(j - 1)) << 1) | (e & (j - 1)));
        um_exchange(key, lo, lo + j, (q & 1) == 0);
      }
      __syncthreads();
    }
  }
  for (int t = tid; t < k; t += UM_THREADS) {
    const um_key v = key[t];
    knn_idx[(long long)i * k + t] = (int)(uint32_t)v;
    knn_dist[(long long)i * k + t] = __uint_as_float((uint32_t)(v >> 32));
  }
}

// ---- graph --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UM_THREADS) void umap_rowsum_kernel(const float* __restrict__ knn_dist, int n, int k,
                                                                 double* __restrict__ rowsum) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= n) return;                                    // wave-uniform
  double s = 0.0;
  for (int t = lane; t < k; t += 64) s += (double)knn_dist[(long long)i * k + t];
  s = wave_sum(s);
  if (lane == 0) rowsum[i] = s;
}

__global__ __launch_bounds__(UM_THREADS) void umap_mean_kernel(const double* __restrict__ rowsum, int n, int k,
                                                               double* __restrict__ mean) {
  __shared__ double red[4];
  double s = 0.0;
  for (int r = threadIdx.x; r < n; r += UM_THREADS) s += rowsum[r];
  s = um_block_sum(s, red);
  if (threadIdx.x == 0) mean[0] = s / ((double)n * (double)k);
}

// umap-learn's search for sigma on one wavefront: sum_{t=1..k-1} (dd_t > 0 ? exp(-dd_t / sigma) : 1) = log2 k, from 1,
// doubling while no upper bound is known, bisecting after, at most 64 rounds, stop at 1e-5.  dd[c] belongs to slot
// lane + 64 c; the sum is lane-strided and folded by xor shuffles, so every lane returns the same bits.
__device__ __forceinline__ double um_sigma_search(const double* dd, int lane, int k) {
  const double target = log2((double)k);
  double lo = 0.0, hi = 0.0, mid = 1.0;
  bool has_hi = false;
  for (int round = 0; round < 64; ++round) {
    double psum = 0.0;
#pragma unroll
    for (int c = 0; c < UM_MAX_K / 64; ++c) {
      const int t = lane + 64 * c;
      if (t >= 1 && t < k) psum += dd[c] > 0.0 ? exp(-dd[c] / mid) : 1.0;
    }
    psum = wave_sum(psum);                            // the same bits in every lane
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) {
      hi = mid;
      has_hi = true;
      mid = (lo + hi) * 0.5;
    } else {
      lo = mid;
      mid = has_hi ? (lo + hi) * 0.5 : mid * 2.0;
    }
  }
  return mid;
}

__global__ __launch_bounds__(UM_THREADS) void umap_sigma_kernel(const int* __restrict__ knn_idx,
                                                                const float* __restrict__ knn_dist, int n, int k,
                                                                const double* __restrict__ rowsum,
                                                                const double* __restrict__ mean, float* __restrict__ rho_out,
                                                                float* __restrict__ sigma_out, float* __restrict__ dense) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= n) return;                                    // wave-uniform
  float d[UM_MAX_K / 64];
  float least = INFINITY;
#pragma unroll
  for (int c = 0; c < UM_MAX_K / 64; ++c) {
    const int t = lane + 64 * c;
    d[c] = t < k ? knn_dist[(long long)i * k + t] : 0.f;
    if (d[c] > 0.f) least = fminf(least, d[c]);
  }
  least = wave_min(least);
  const float rho = least == INFINITY ? 0.f : least;
  double dd[UM_MAX_K / 64];
#pragma unroll
  for (int c = 0; c < UM_MAX_K / 64; ++c) dd[c] = (double)d[c] - (double)rho;
  const double mid = um_sigma_search(dd, lane, k);
  const double floor_at = 1e-3 * (rho > 0.f ? rowsum[i] / (double)k : mean[0]);
  const double sigma = fmax(mid, floor_at);
  if (lane == 0) {
    rho_out[i] = rho;
    sigma_out[i] = (float)sigma;
  }
#pragma unroll
  for (int c = 0; c < UM_MAX_K / 64; ++c) {
    const int t = lane + 64 * c;
    if (t >= k) continue;
    const int j = knn_idx[(long long)i * k + t];
    if ((unsigned)j >= (unsigned)n) continue;            // not an index of this matrix: nothing is written
    const float v = j == i ? 0.f : (dd[c] > 0.0 ? (float)exp(-dd[c] / sigma) : 1.f);
    dense[(long long)i * n + j] = v;
  }
}

__device__ __forceinline__ float um_union(float a, float b) {
  return (float)(((double)a + (double)b) - (double)a * (double)b);
}

// grid (T, T); the workgroup (bx >= by) owns tile (by, bx) and its mirror (bx, by)
__global__ __launch_bounds__(UM_THREADS) void umap_union_kernel(float* __restrict__ w, int n, float* __restrict__ partial) {
  __shared__ float ta[UM_TILE][UM_TILE + 1];
  __shared__ float tb[UM_TILE][UM_TILE + 1];
  __shared__ float red[UM_THREADS / 64];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int bi = blockIdx.y, bj = blockIdx.x;
  float* dst = partial + (long long)bi * gridDim.x + bj;
  if (bj < bi) {                                         // workgroup-uniform
    if (tid == 0) dst[0] = 0.f;
    return;
  }
  const int i0 = bi * UM_TILE, j0 = bj * UM_TILE;
#pragma unroll
  for (int c = 0; c < UM_TILE / 8; ++c) {
    const int r = ty + 8 * c;
    ta[r][tx] = (i0 + r < n && j0 + tx < n) ? w[(long long)(i0 + r) * n + j0 + tx] : 0.f;
    tb[r][tx] = (j0 + r < n && i0 + tx < n) ? w[(long long)(j0 + r) * n + i0 + tx] : 0.f;
  }
  __syncthreads();
  float top = 0.f;
#pragma unroll
  for (int c = 0; c < UM_TILE / 8; ++c) {
    const int r = ty + 8 * c;
    if (i0 + r < n && j0 + tx < n) {
      const float v = um_union(ta[r][tx], tb[tx][r]);
      w[(long long)(i0 + r) * n + j0 + tx] = v;
      top = fmaxf(top, v);
    }
    if (bi != bj && j0 + r < n && i0 + tx < n) w[(long long)(j0 + r) * n + i0 + tx] = um_union(ta[tx][r], tb[r][tx]);
  }
  top = wave_max(top);
  if ((tid & 63) == 0) red[tid >> 6] = top;
  __syncthreads();
  if (tid == 0) dst[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(UM_THREADS) void umap_wmax_kernel(const float* __restrict__ partial, int count,
                                                               float* __restrict__ wmax) {
  __shared__ float red[UM_THREADS / 64];
  float top = 0.f;
  for (int t = threadIdx.x; t < count; t += UM_THREADS) top = fmaxf(top, partial[t]);
  top = wave_max(top);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = top;
  __syncthreads();
  if (threadIdx.x == 0) wmax[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// kept: a positive weight that is not below wmax / n_epochs; both products are exact in fp64
__device__ __forceinline__ bool um_kept(float w, float wmax, int n_epochs) {
  return w > 0.f && (double)w * (double)n_epochs >= (double)wmax;
}

// floor(w * 2^20 / wmax): q * wmax (45 bits) and w * 2^20 are exact in fp64, so the two tests repair a quotient that is off
__device__ __forceinline__ int um_rate(float w, float wmax) {
  const double num = (double)w * 1048576.0, den = (double)wmax;
  double q = floor(num / den);
  if (q * den > num) q -= 1.0;
  else if ((q + 1.0) * den <= num) q += 1.0;
  return (int)q;
}

__global__ __launch_bounds__(UM_THREADS) void umap_count_kernel(const float* __restrict__ w, int n, int n_epochs,
                                                                const float* __restrict__ wmax, int* __restrict__ count) {
  __shared__ int red[UM_THREADS / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float top = wmax[0];
  int c = 0;
  for (int j = tid; j < n; j += UM_THREADS) c += um_kept(w[(long long)i * n + j], top, n_epochs) ? 1 : 0;
  c = wave_sum(c);
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) count[i] = red[0] + red[1] + red[2] + red[3];
}

// one workgroup: thread t owns the rows [t * chunk, (t + 1) * chunk)
__global__ __launch_bounds__(UM_THREADS) void umap_scan_kernel(const int* __restrict__ count, int n, int* __restrict__ indptr) {
  __shared__ int sums[UM_THREADS];
  const int tid = threadIdx.x, chunk = (n + UM_THREADS - 1) / UM_THREADS;
  const int r0 = min(tid * chunk, n), r1 = min(r0 + chunk, n);
  int s = 0;
  for (int r = r0; r < r1; ++r) s += count[r];
  sums[tid] = s;
  __syncthreads();
  int before = 0;
  for (int t = 0; t < tid; ++t) before += sums[t];
  for (int r = r0; r < r1; ++r) {
    indptr[r] = before;
    before += count[r];
  }
  if (tid == UM_THREADS - 1) indptr[n] = before;         // r1 = n for the last thread: the total
}

__global__ __launch_bounds__(UM_THREADS) void umap_fill_kernel(const float* __restrict__ w, int n, int n_epochs,
                                                               const float* __restrict__ wmax, const int* __restrict__ indptr,
                                                               long long capacity, int* __restrict__ indices,
                                                               float* __restrict__ weights, int* __restrict__ rate) {
  __shared__ int wave_count[UM_THREADS / 64];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float top = wmax[0];
  long long at = indptr[i];
  for (int j0 = 0; j0 < n; j0 += UM_THREADS) {           // workgroup-uniform trip count
    const int j = j0 + tid;
    const float v = j < n ? w[(long long)i * n + j] : 0.f;
    const bool keep = j < n && um_kept(v, top, n_epochs);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    long long pos = at + __popcll(mask & ((1ull << lane) - 1ull));
    int total = 0;
#pragma unroll
    for (int q = 0; q < UM_THREADS / 64; ++q) {
      if (q < wave) pos += wave_count[q];
      total += wave_count[q];
    }
    if (keep && pos < capacity) {
      indices[pos] = j;
      weights[pos] = v;
      rate[pos] = um_rate(v, top);
    }
    at += total;
    __syncthreads();                                     // wave_count is rewritten by the next block of columns
  }
}

// ---- layout epoch ---------------------------------------------------------------------------------------------------
struct UmEpoch {
  const int* indptr;
  const int* indices;
  const int* rate;
  const float* y_in;
  float* y_out;
  long long capacity;
  double a, b, alpha;
  int n, epoch, negatives;
  uint32_t base;         // lowbias32(seed + epoch)
};

__device__ __forceinline__ double um_clip(double v) { return fmin(fmax(v, -4.0), 4.0); }

__global__ __launch_bounds__(UM_THREADS) void umap_epoch_kernel(UmEpoch u) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= u.n) return;                                  // wave-uniform
  const double yx = (double)u.y_in[2 * i], yy = (double)u.y_in[2 * i + 1];
  const long long p0 = max(u.indptr[i], 0), p1 = min((long long)u.indptr[i + 1], u.capacity);
  const unsigned long long e = (unsigned long long)u.epoch;
  double sx = 0.0, sy = 0.0;
  for (long long p = p0 + lane; p < p1; p += 64) {
    const unsigned long long r = (unsigned long long)(uint32_t)u.rate[p];
    if ((((e + 1) * r) >> 20) <= ((e * r) >> 20)) continue;
    const int j = u.indices[p];
    if ((unsigned)j < (unsigned)u.n) {
      const double dx = yx - (double)u.y_in[2 * j], dy = yy - (double)u.y_in[2 * j + 1];
      const double d2 = dx * dx + dy * dy;
      if (d2 > 0.0) {
        const double pw = exp(u.b * log(d2));
        const double g = -2.0 * u.a * u.b * (pw / d2) / (u.a * pw + 1.0);
        sx += 2.0 * um_clip(g * dx);
        sy += 2.0 * um_clip(g * dy);
      }
    }
    for (int s = 0; s < u.negatives; ++s) {
      const uint32_t h = lowbias32(u.base ^ ((uint32_t)p * (uint32_t)u.negatives + (uint32_t)s));
      const int v = (int)(((unsigned long long)h * (unsigned long long)u.n) >> 32);
      const double dx = yx - (double)u.y_in[2 * v], dy = yy - (double)u.y_in[2 * v + 1];
      const double d2 = dx * dx + dy * dy;
      if (d2 > 0.0) {
        const double g = 2.0 * u.b / ((0.001 + d2) * (u.a * exp(u.b * log(d2)) + 1.0));
        sx += um_clip(g * dx);
        sy += um_clip(g * dy);
      }
    }
  }
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  if (lane == 0) {
    u.y_out[2 * i] = (float)(yx + u.alpha * sx);
    u.y_out[2 * i + 1] = (float)(yy + u.alpha * sy);
  }
}

// ---- transform: new rows into a fitted embedding ----------------------------------------------------------------------
// One wavefront per new row.  rho = 0 for every row (umap-learn's transform runs with local_connectivity - 1 = 0), so the
// search sees the distances themselves and the floor is 1e-3 * the mean of all m k distances; the strengths are
// bipartite: a zero distance is 1, the row itself is not excluded.  The start point is the strength-weighted mean of the
// neighbours' training points over all k slots, summed in fp64 (lane-strided, xor fold).
__global__ __launch_bounds__(UM_THREADS) void umap_tsigma_kernel(const int* __restrict__ knn_idx,
                                                                 const float* __restrict__ knn_dist, int m, int k,
                                                                 const float* __restrict__ y_train, int n,
                                                                 const double* __restrict__ mean, float* __restrict__ sigma_out,
                                                                 float* __restrict__ weights, float* __restrict__ rowmax,
                                                                 float* __restrict__ y0) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= m) return;                                    // wave-uniform
  double dd[UM_MAX_K / 64];
#pragma unroll
  for (int c = 0; c < UM_MAX_K / 64; ++c) {
    const int t = lane + 64 * c;
    dd[c] = t < k ? (double)knn_dist[(long long)i * k + t] : 0.0;
  }
  const double sigma = fmax(um_sigma_search(dd, lane, k), 1e-3 * mean[0]);
  float top = 0.f;
  double sw = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
  for (int c = 0; c < UM_MAX_K / 64; ++c) {
    const int t = lane + 64 * c;
    if (t >= k) continue;
    const float v = dd[c] > 0.0 ? (float)exp(-dd[c] / sigma) : 1.f;
    weights[(long long)i * k + t] = v;
    top = fmaxf(top, v);
    const int j = knn_idx[(long long)i * k + t];
    if ((unsigned)j >= (unsigned)n) continue;            // not a training row: no part in the start point
    sw += (double)v;
    sx += (double)v * (double)y_train[2 * j];
    sy += (double)v * (double)y_train[2 * j + 1];
  }
  top = wave_max(top);
  sw = wave_sum(sw);
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  if (lane == 0) {
    sigma_out[i] = (float)sigma;
    rowmax[i] = top;
    y0[2 * i] = sw > 0.0 ? (float)(sx / sw) : 0.f;
    y0[2 * i + 1] = sw > 0.0 ? (float)(sy / sw) : 0.f;
  }
}

__global__ __launch_bounds__(UM_THREADS) void umap_trate_kernel(const float* __restrict__ weights, int count, int n_epochs,
                                                                const float* __restrict__ wmax, int* __restrict__ rate) {
  const int p = blockIdx.x * UM_THREADS + threadIdx.x;
  if (p >= count) return;
  const float v = weights[p], top = wmax[0];
  rate[p] = um_kept(v, top, n_epochs) ? um_rate(v, top) : 0;
}

struct UmTransform {
  const int* knn_idx;
  const int* rate;
  const float* y_train;
  const float* y_in;
  float* y_out;
  double a, b, initial_alpha;
  int m, k, n, n_epochs, epoch_begin, epoch_end, negatives;
  uint32_t seed;
};

// One wavefront per new row, all epochs in one launch: the row reads the frozen training embedding and itself only.  Its
// index and rate slots (at most four per lane) and its point live in registers; the point is rounded to fp32 at the end
// of every epoch, so epochs [0, T) in one launch are T launches of one epoch each, bit for bit.  The training embedding
// (at most 64 KB, read-only) is read through the caches.
__global__ __launch_bounds__(UM_THREADS) void umap_transform_kernel(UmTransform u) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= u.m) return;                                  // wave-uniform
  int idx[UM_MAX_K / 64];
  unsigned long long rate[UM_MAX_K / 64];
#pragma unroll
  for (int c = 0; c < UM_MAX_K / 64; ++c) {
    const int t = lane + 64 * c;
    idx[c] = t < u.k ? u.knn_idx[(long long)i * u.k + t] : -1;
    const int r = t < u.k ? u.rate[(long long)i * u.k + t] : 0;
    rate[c] = (unsigned)idx[c] < (unsigned)u.n && r > 0 ? (unsigned long long)r : 0ull;   // outside [0, n): never fires
  }
  float yx = u.y_in[2 * i], yy = u.y_in[2 * i + 1];
  for (int epoch = u.epoch_begin; epoch < u.epoch_end; ++epoch) {
    const unsigned long long e = (unsigned long long)epoch;
    const uint32_t base = lowbias32(u.seed + (uint32_t)epoch);
    const double px = (double)yx, py = (double)yy;
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int c = 0; c < UM_MAX_K / 64; ++c) {
      if ((((e + 1) * rate[c]) >> 20) <= ((e * rate[c]) >> 20)) continue;
      {
        const double dx = px - (double)u.y_train[2 * idx[c]], dy = py - (double)u.y_train[2 * idx[c] + 1];
        const double d2 = dx * dx + dy * dy;
        if (d2 > 0.0) {
          const double pw = exp(u.b * log(d2));
          const double g = -2.0 * u.a * u.b * (pw / d2) / (u.a * pw + 1.0);
          sx += um_clip(g * dx);
          sy += um_clip(g * dy);
        }
      }
      const uint32_t p = (uint32_t)(i * u.k + lane + 64 * c);
      for (int s = 0; s < u.negatives; ++s) {
        const uint32_t h = lowbias32(base ^ (p * (uint32_t)u.negatives + (uint32_t)s));
        const int v = (int)(((unsigned long long)h * (unsigned long long)u.n) >> 32);
        const double dx = px - (double)u.y_train[2 * v], dy = py - (double)u.y_train[2 * v + 1];
        const double d2 = dx * dx + dy * dy;
        if (d2 > 0.0) {
          const double g = 2.0 * u.b / ((0.001 + d2) * (u.a * exp(u.b * log(d2)) + 1.0));
          sx += um_clip(g * dx);
          sy += um_clip(g * dy);
        }
      }
    }
    sx = wave_sum(sx);                                // the same bits in every lane
    sy = wave_sum(sy);
    const double alpha = u.initial_alpha * (1.0 - (double)epoch / (double)u.n_epochs);
    yx = (float)(px + alpha * sx);
    yy = (float)(py + alpha * sy);
  }
  if (lane == 0) {
    u.y_out[2 * i] = yx;
    u.y_out[2 * i + 1] = yy;
  }
}

int um_pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

bool um_shape_ok(int n, int k) { return n >= UM_MIN_N && n <= UM_MAX_N && k >= 2 && k <= UM_MAX_K && k < n; }
long long um_capacity(int n, int k) {
  const long long both = 2LL * n * k, all = (long long)n * n;
  return both < all ? both : all;
}

// the checks pti_umap_knn and pti_umap_graph share; 0 when the shape is fine
int um_check_shape(const char* who, int n, int k) {
  if (n < UM_MIN_N) PTI_FAIL(PTI_EINVAL, "%s: bad dimension n=%d (at least %d rows)", who, n, UM_MIN_N);
  if (k < 2 || k >= n) PTI_FAIL(PTI_EINVAL, "%s: bad dimension k=%d (2 <= k < n=%d)", who, k, n);
  if (n > UM_MAX_N || k > UM_MAX_K)
    PTI_FAIL(PTI_EUNSUPPORTED, "%s: unsupported shape n=%d k=%d (at most %d rows, %d neighbours)", who, n, k, UM_MAX_N, UM_MAX_K);
  return PTI_OK;
}

// the checks of the transform's entry points: m new rows against n training rows; 0 when the shape is fine
int um_check_cross(const char* who, int m, int n, int k) {
  if (m < 1) PTI_FAIL(PTI_EINVAL, "%s: bad dimension m=%d (at least 1 new row)", who, m);
  if (n < UM_MIN_N) PTI_FAIL(PTI_EINVAL, "%s: bad dimension n=%d (at least %d training rows)", who, n, UM_MIN_N);
  if (k < 2 || k >= n) PTI_FAIL(PTI_EINVAL, "%s: bad dimension k=%d (2 <= k < n=%d)", who, k, n);
  if (m > UM_MAX_N || n > UM_MAX_N || k > UM_MAX_K)
    PTI_FAIL(PTI_EUNSUPPORTED, "%s: unsupported shape m=%d n=%d k=%d (at most %d rows, %d neighbours)", who, m, n, k, UM_MAX_N,
             UM_MAX_K);
  return PTI_OK;
}
int um_check_epochs(const char* who, int n_epochs) {
  if (n_epochs < 1) PTI_FAIL(PTI_EINVAL, "%s: bad dimension n_epochs=%d (at least 1)", who, n_epochs);
  if (n_epochs > UM_MAX_EPOCHS) PTI_FAIL(PTI_EUNSUPPORTED, "%s: unsupported n_epochs=%d (at most %d)", who, n_epochs, UM_MAX_EPOCHS);
  return PTI_OK;
}
bool um_cross_ok(int m, int n, int k) { return m >= 1 && m <= UM_MAX_N && um_shape_ok(n, k); }

// one workgroup per row of dist [rows][n]; the checks are the callers'
int um_launch_knn(const char* who, const float* dist, int64_t ldd, int rows, int n, int k, int* knn_idx, float* knn_dist,
                  pti_stream_t s) {
  const int m = um_pow2_at_least(k);
  int lm = 0;
  while ((1 << lm) < m) ++lm;
  const int np2 = um_pow2_at_least(n > m ? n : m);       // at most 8192 keys: 64 KB of LDS
  PTI_LAUNCH(umap_knn_kernel, dim3(rows), dim3(UM_THREADS), (size_t)np2 * sizeof(um_key), (hipStream_t)s, dist, (long long)ldd,
             n, k, lm, np2, knn_idx, knn_dist);
  PTI_CHECK_LAUNCH(who);
  return PTI_OK;
}

}  // namespace

extern "C" int pti_umap_knn(const float* dist, int64_t ldd, int n, int k, int* knn_idx, float* knn_dist, pti_stream_t s) {
  if (!dist || !knn_idx || !knn_dist) PTI_FAIL(PTI_EINVAL, "umap_knn: null pointer");
  if (int rc = um_check_shape("umap_knn", n, k)) return rc;
  if (ldd < n) PTI_FAIL(PTI_EINVAL, "umap_knn: row stride below the row length (ldd=%lld n=%d)", (long long)ldd, n);
  return um_launch_knn("umap_knn", dist, ldd, n, n, k, knn_idx, knn_dist, s);
}

extern "C" int64_t pti_umap_graph_capacity(int n, int k) { return um_shape_ok(n, k) ? um_capacity(n, k) : 0; }

extern "C" int64_t pti_umap_graph_ws_floats(int n, int k) {
  if (!um_shape_ok(n, k)) return 0;
  const long long t = cdiv(n, UM_TILE);
  return 2LL * (n + 1) + (long long)n * n + t * t + 1 + n;
}

extern "C" int pti_umap_graph(const int* knn_idx, const float* knn_dist, int n, int k, int n_epochs, int* indptr, int* indices,
                              float* weights, int* rate, int64_t capacity, float* rho, float* sigma, float* workspace,
                              pti_stream_t s) {
  if (!knn_idx || !knn_dist || !indptr || !indices || !weights || !rate || !rho || !sigma || !workspace)
    PTI_FAIL(PTI_EINVAL, "umap_graph: null pointer");
  if (int rc = um_check_shape("umap_graph", n, k)) return rc;
  if (n_epochs < 1) PTI_FAIL(PTI_EINVAL, "umap_graph: bad dimension n_epochs=%d (at least 1)", n_epochs);
  if (n_epochs > UM_MAX_EPOCHS)
    PTI_FAIL(PTI_EUNSUPPORTED, "umap_graph: unsupported n_epochs=%d (at most %d)", n_epochs, UM_MAX_EPOCHS);
  if (capacity < um_capacity(n, k))
    PTI_FAIL(PTI_EINVAL, "umap_graph: capacity %lld below min(2 n k, n^2) = %lld", (long long)capacity, um_capacity(n, k));
  if (((uintptr_t)workspace & 7) != 0) PTI_FAIL(PTI_EINVAL, "umap_graph: workspace must be 8-byte aligned");
  const int t = cdiv(n, UM_TILE), waves = cdiv(n, UM_THREADS / 64);
  double* rowsum = (double*)workspace;
  double* mean = rowsum + n;
  float* dense = (float*)(mean + 1);
  float* partial = dense + (long long)n * n;
  float* wmax = partial + (long long)t * t;
  int* count = (int*)(wmax + 1);
  hipStream_t st = (hipStream_t)s;
  if (hipMemsetAsync(dense, 0, (size_t)n * n * sizeof(float), st) != hipSuccess)
    PTI_FAIL(PTI_ELAUNCH, "umap_graph: clearing the scratch failed");
  PTI_LAUNCH(umap_rowsum_kernel, dim3(waves), dim3(UM_THREADS), 0, st, knn_dist, n, k, rowsum);
  PTI_CHECK_LAUNCH("umap_rowsum");
  PTI_LAUNCH(umap_mean_kernel, dim3(1), dim3(UM_THREADS), 0, st, (const double*)rowsum, n, k, mean);
  PTI_CHECK_LAUNCH("umap_mean");
  PTI_LAUNCH(umap_sigma_kernel, dim3(waves), dim3(UM_THREADS), 0, st, knn_idx, knn_dist, n, k, (const double*)rowsum,
             (const double*)mean, rho, sigma, dense);
  PTI_CHECK_LAUNCH("umap_sigma");
  PTI_LAUNCH(umap_union_kernel, dim3(t, t), dim3(UM_THREADS), 0, st, dense, n, partial);
  PTI_CHECK_LAUNCH("umap_union");
  PTI_LAUNCH(umap_wmax_kernel, dim3(1), dim3(UM_THREADS), 0, st, (const float*)partial, t * t, wmax);
  PTI_CHECK_LAUNCH("umap_wmax");
  PTI_LAUNCH(umap_count_kernel, dim3(n), dim3(UM_THREADS), 0, st, (const float*)dense, n, n_epochs, (const float*)wmax, count);
  PTI_CHECK_LAUNCH("umap_count");
  PTI_LAUNCH(umap_scan_kernel, dim3(1), dim3(UM_THREADS), 0, st, (const int*)count, n, indptr);
  PTI_CHECK_LAUNCH("umap_scan");
  PTI_LAUNCH(umap_fill_kernel, dim3(n), dim3(UM_THREADS), 0, st, (const float*)dense, n, n_epochs, (const float*)wmax,
             (const int*)indptr, (long long)capacity, indices, weights, rate);
  PTI_CHECK_LAUNCH("umap_fill");
  return PTI_OK;
}

extern "C" int pti_umap_epoch(const int* indptr, const int* indices, const int* rate, int64_t capacity, int n,
                              int n_components, const float* y_in, float* y_out, double a, double b, double alpha, int epoch,
                              uint32_t seed, int negative_sample_rate, pti_stream_t s) {
  if (!indptr || !indices || !rate || !y_in || !y_out) PTI_FAIL(PTI_EINVAL, "umap_epoch: null pointer");
  if (n < UM_MIN_N) PTI_FAIL(PTI_EINVAL, "umap_epoch: bad dimension n=%d (at least %d rows)", n, UM_MIN_N);
  if (n_components != 2) PTI_FAIL(PTI_EUNSUPPORTED, "umap_epoch: n_components=%d (only 2 is built)", n_components);
  if (n > UM_MAX_N) PTI_FAIL(PTI_EUNSUPPORTED, "umap_epoch: unsupported shape n=%d (at most %d rows)", n, UM_MAX_N);
  if (capacity < 0 || capacity > (int64_t)n * n)
    PTI_FAIL(PTI_EINVAL, "umap_epoch: capacity %lld outside [0, n^2]", (long long)capacity);
  if (epoch < 0) PTI_FAIL(PTI_EINVAL, "umap_epoch: bad epoch %d", epoch);
  if (epoch >= UM_MAX_EPOCHS) PTI_FAIL(PTI_EUNSUPPORTED, "umap_epoch: unsupported epoch %d (at most %d epochs)", epoch, UM_MAX_EPOCHS);
  if (negative_sample_rate < 0 || negative_sample_rate > UM_MAX_NEG)
    PTI_FAIL(PTI_EINVAL, "umap_epoch: negative_sample_rate %d outside [0, %d]", negative_sample_rate, UM_MAX_NEG);
  if (!(a > 0.0) || !(b > 0.0)) PTI_FAIL(PTI_EINVAL, "umap_epoch: a=%g and b=%g must be positive", a, b);
  if (y_in == y_out) PTI_FAIL(PTI_EINVAL, "umap_epoch: y_out must not be y_in (the embedding is double buffered)");
  UmEpoch u;
  u.indptr = indptr;
  u.indices = indices;
  u.rate = rate;
  u.y_in = y_in;
  u.y_out = y_out;
  u.capacity = capacity;
  u.a = a;
  u.b = b;
  u.alpha = alpha;
  u.n = n;
  u.epoch = epoch;
  u.negatives = negative_sample_rate;
  u.base = lowbias32(seed + (uint32_t)epoch);
  PTI_LAUNCH(umap_epoch_kernel, dim3(cdiv(n, UM_THREADS / 64)), dim3(UM_THREADS), 0, (hipStream_t)s, u);
  PTI_CHECK_LAUNCH("umap_epoch");
  return PTI_OK;
}

// ---- transform ------------------------------------------------------------------------------------------------------------
extern "C" int pti_umap_knn_cross(const float* dist, int64_t ldd, int m, int n, int k, int* knn_idx, float* knn_dist,
                                  pti_stream_t s) {
  if (!dist || !knn_idx || !knn_dist) PTI_FAIL(PTI_EINVAL, "umap_knn_cross: null pointer");
  if (int rc = um_check_cross("umap_knn_cross", m, n, k)) return rc;
  if (ldd < n) PTI_FAIL(PTI_EINVAL, "umap_knn_cross: row stride below the row length (ldd=%lld n=%d)", (long long)ldd, n);
  return um_launch_knn("umap_knn_cross", dist, ldd, m, n, k, knn_idx, knn_dist, s);
}

extern "C" int64_t pti_umap_transform_graph_ws_floats(int m, int n, int k) {
  return um_cross_ok(m, n, k) ? 2LL * (m + 1) + m + 1 : 0;
}

extern "C" int pti_umap_transform_graph(const int* knn_idx, const float* knn_dist, int m, int k, const float* y_train, int n,
                                        int n_epochs, float* sigma, float* weights, int* rate, float* y0, float* workspace,
                                        pti_stream_t s) {
  if (!knn_idx || !knn_dist || !y_train || !sigma || !weights || !rate || !y0 || !workspace)
    PTI_FAIL(PTI_EINVAL, "umap_transform_graph: null pointer");
  if (int rc = um_check_cross("umap_transform_graph", m, n, k)) return rc;
  if (int rc = um_check_epochs("umap_transform_graph", n_epochs)) return rc;
  if (((uintptr_t)workspace & 7) != 0) PTI_FAIL(PTI_EINVAL, "umap_transform_graph: workspace must be 8-byte aligned");
  const int waves = cdiv(m, UM_THREADS / 64);
  double* rowsum = (double*)workspace;
  double* mean = rowsum + m;
  float* rowmax = (float*)(mean + 1);
  float* wmax = rowmax + m;
  hipStream_t st = (hipStream_t)s;
  PTI_LAUNCH(umap_rowsum_kernel, dim3(waves), dim3(UM_THREADS), 0, st, knn_dist, m, k, rowsum);
  PTI_CHECK_LAUNCH("umap_rowsum");
  PTI_LAUNCH(umap_mean_kernel, dim3(1), dim3(UM_THREADS), 0, st, (const double*)rowsum, m, k, mean);
  PTI_CHECK_LAUNCH("umap_mean");
  PTI_LAUNCH(umap_tsigma_kernel, dim3(waves), dim3(UM_THREADS), 0, st, knn_idx, knn_dist, m, k, y_train, n, (const double*)mean,
             sigma, weights, rowmax, y0);
  PTI_CHECK_LAUNCH("umap_tsigma");
  PTI_LAUNCH(umap_wmax_kernel, dim3(1), dim3(UM_THREADS), 0, st, (const float*)rowmax, m, wmax);
  PTI_CHECK_LAUNCH("umap_wmax");
  PTI_LAUNCH(umap_trate_kernel, dim3(cdiv(m * k, UM_THREADS)), dim3(UM_THREADS), 0, st, (const float*)weights, m * k, n_epochs,
             (const float*)wmax, rate);
  PTI_CHECK_LAUNCH("umap_trate");
  return PTI_OK;
}

extern "C" int pti_umap_transform_layout(const int* knn_idx, const int* rate, int m, int k, const float* y_train, int n,
                                         const float* y_in, float* y_out, double a, double b, double initial_alpha, int n_epochs,
                                         int epoch_begin, int epoch_end, uint32_t seed, int negative_sample_rate, pti_stream_t s) {
  if (!knn_idx || !rate || !y_train || !y_in || !y_out) PTI_FAIL(PTI_EINVAL, "umap_transform_layout: null pointer");
  if (int rc = um_check_cross("umap_transform_layout", m, n, k)) return rc;
  if (int rc = um_check_epochs("umap_transform_layout", n_epochs)) return rc;
  if (epoch_begin < 0 || epoch_end < epoch_begin || epoch_end > n_epochs)
    PTI_FAIL(PTI_EINVAL, "umap_transform_layout: bad epoch range [%d, %d) of %d", epoch_begin, epoch_end, n_epochs);
  if (negative_sample_rate < 0 || negative_sample_rate > UM_MAX_NEG)
    PTI_FAIL(PTI_EINVAL, "umap_transform_layout: negative_sample_rate %d outside [0, %d]", negative_sample_rate, UM_MAX_NEG);
  if (!(a > 0.0) || !(b > 0.0)) PTI_FAIL(PTI_EINVAL, "umap_transform_layout: a=%g and b=%g must be positive", a, b);
  if (!(initial_alpha > 0.0) || !(initial_alpha <= 1e6))
    PTI_FAIL(PTI_EINVAL, "umap_transform_layout: initial_alpha=%g must be positive and finite", initial_alpha);
  if (y_train < y_out + 2LL * m && y_out < y_train + 2LL * n)
    PTI_FAIL(PTI_EINVAL, "umap_transform_layout: y_out must not overlap y_train (the training embedding is read by every row)");
  if (y_in != y_out && y_in < y_out + 2LL * m && y_out < y_in + 2LL * m)
    PTI_FAIL(PTI_EINVAL, "umap_transform_layout: y_out must be y_in itself or apart from it");
  UmTransform u;
  u.knn_idx = knn_idx;
  u.rate = rate;
  u.y_train = y_train;
  u.y_in = y_in;
  u.y_out = y_out;
  u.a = a;
  u.b = b;
  u.initial_alpha = initial_alpha;
  u.m = m;
  u.k = k;
  u.n = n;
  u.n_epochs = n_epochs;
  u.epoch_begin = epoch_begin;
  u.epoch_end = epoch_end;
  u.negatives = negative_sample_rate;
  u.seed = seed;
  PTI_LAUNCH(umap_transform_kernel, dim3(cdiv(m, UM_THREADS / 64)), dim3(UM_THREADS), 0, (hipStream_t)s, u);
  PTI_CHECK_LAUNCH("umap_transform_layout");
  return PTI_OK;
}
