// Co-ranking curves and the Shepard figure of a projection on the device (gfx950): the rank of EVERY column of every row of a
// distance matrix, and the two folds that turn two rank tables / two distance matrices into small integer histograms and
// per-row sums.  4 <= n <= 8192.  DESIGN.md 5s.
//
//   pti_full_ranks, one launch: one workgroup per row, 256 threads up to 2048 columns and 1024 above (measured: DESIGN.md
//     5s).  The row becomes pti_umap_knn's 64-bit keys in LDS (neighbor_order_key, pti_common.h), padded to a power of two
//     with all-ones keys (64 KB at n = 8192).  A bitonic network sorts the whole row; no two keys are equal, so any correct sort gives the same result.  Every thread
//     then takes the columns at its positions into registers (at most 8), the thread that meets the row's own column
//     publishes its position, and after a barrier the positions are scattered into an int16 row that REUSES the keys'
//     LDS: rank = position + 1, less one past the own column's position, 0 at the own column.  The row leaves with 16-byte
//     stores between a scalar head and tail that absorb whatever alignment the caller's row has.  Comparisons only: exact.
//   pti_coranking_fold, one launch: one 256-thread workgroup per block of 8 rows.  For every entry with both ranks in
//     [1, n - 1] (the own column, rank 0, and anything out of range are skipped and never used as an index) the bin
//     max(rho, r) of one of three n-bin LDS histograms -- equal, intrusion (r < rho), extrusion (rho < r) -- is raised by an
//     LDS integer atomic (96 KB at n = 8192); (rho - r)^2 is summed per row as int64 (wave_sum / block_sum).  A row puts at
//     most two entries into a bin, so a workgroup that flushed after ONE row would issue as many global atomics as there
//     are entries; eight rows share a flush.  Non-zero bins are ADDED to the global histograms with integer atomicAdd.
//   pti_shepard_fold, one launch: one 256-thread workgroup per block of 8 rows.  Per row the three sums of d_high^2, d_low^2
//     and d_high d_low over the other columns, each product formed in fp64 from the two fp32 values (exact): thread t adds
//     the terms at t + 256 q into accumulator q mod 4, q ascending, (a0 + a1) + (a2 + a3), the xor butterfly over the lanes,
//     ((w0 + w1) + w2) + w3 over the waves, fp-reassociation off: the bits depend on the row and n alone.  The bins x bins
//     histogram of (floor(d_high * scale[0]), floor(d_low * scale[1])), each clamped to [0, bins - 1], sits in LDS (64 KB at
//     128 bins) and is flushed like the one above.  The scales are the caller's (a DEVICE pair): a division in this
//     library is not correctly rounded under -ffast-math, one fp32 multiply is.  +inf and NaN go to the last bin.
// Integer atomics only (sums of integers have no order), no floating-point atomics, no workspace, caller's stream, no host
// synchronisation; bitwise reproducible.  The histograms ACCUMULATE: the caller zeroes them.
#include "pti_common.h"

namespace {

constexpr int CR_MIN_N = 4;
constexpr int CR_MAX_N = 8192;
constexpr int CR_MIN_BINS = 2;
constexpr int CR_MAX_BINS = 128;
constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = CR_THREADS / 64;
constexpr int CR_ROWS = 8;                                 // rows per workgroup of the two folds
constexpr int CR_SORT_WIDE = 1024;                         // threads of the workgroup that sorts a row of more than ...
constexpr int CR_SORT_WIDE_KEYS = 4096;                    // ... 2048 columns (this many keys or more); 256 below

typedef unsigned long long cr_key;

template <int CR_SORT_THREADS>
__global__ __launch_bounds__(CR_SORT_THREADS) void full_ranks_kernel(const float* __restrict__ dist, long long ldd, int n, int row0,
                                                                     int np2, short* __restrict__ out, long long ldo) {
  // sorted positions per thread at the most columns this instance is launched for: 8 either way
  constexpr int CR_SLOTS = (CR_SORT_THREADS == CR_SORT_WIDE ? CR_MAX_N : CR_SORT_WIDE_KEYS / 2) / CR_SORT_THREADS;
  extern __shared__ __attribute__((aligned(16))) cr_key cr_keys[];
  __shared__ int own_pos;
  const int r = blockIdx.x, i = row0 + r, tid = threadIdx.x;
  const float* __restrict__ row = dist + (long long)r * ldd;
  for (int j = tid; j < np2; j += CR_SORT_THREADS) {
    cr_key v = ~0ull;                                      // padding sorts last
    if (j < n) v = neighbor_order_key(row[j], j);
    cr_keys[j] = v;
  }
  __syncthreads();
  for (int sz = 2; sz <= np2; sz <<= 1)
    for (int j = sz >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < np2 / 2; t += CR_SORT_THREADS) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
        const cr_key a = cr_keys[lo], b = cr_keys[hi];
        if ((a > b) == ((lo & sz) == 0)) {
          cr_keys[lo] = b;
          cr_keys[hi] = a;
        }
      }
      __syncthreads();
    }
  // position -> column, through registers: the int16 row below lies over the keys
  int col[CR_SLOTS];
#pragma unroll
  for (int q = 0; q < CR_SLOTS; ++q) {
    const int p = tid + q * CR_SORT_THREADS;
    col[q] = p < n ? (int)(uint32_t)cr_keys[p] : -1;       // the first n positions hold the n real columns
    if (col[q] == i) own_pos = p;
  }
  __syncthreads();
  short* rank = (short*)cr_keys;
  const int own = own_pos;
#pragma unroll
  for (int q = 0; q < CR_SLOTS; ++q) {
    const int p = tid + q * CR_SORT_THREADS;
    if (col[q] >= 0) rank[col[q]] = (short)(col[q] == i ? 0 : p + 1 - (p > own ? 1 : 0));
  }
  __syncthreads();
  short* __restrict__ dst = out + (long long)r * ldo;
  int head = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 1);   // elements before the first 16-byte boundary
  if (head > n) head = n;
  const int body = (n - head) >> 3;
  if (tid < head) dst[tid] = rank[tid];
  for (int t = tid; t < body; t += CR_SORT_THREADS) {
    const int j = head + 8 * t;
    u32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (uint32_t)(uint16_t)rank[j + 2 * u] | ((uint32_t)(uint16_t)rank[j + 2 * u + 1] << 16);
    *(u32x4*)(dst + j) = v;
  }
  const int tail = head + 8 * body + tid;                  // fewer than 8 elements remain
  if (tid < 8 && tail < n) dst[tail] = rank[tail];
}

__global__ __launch_bounds__(CR_THREADS) void coranking_fold_kernel(const short* __restrict__ rank_high, long long ldh,
                                                                    const short* __restrict__ rank_low, long long ldl, int m, int n,
                                                                    unsigned* __restrict__ hist, long long* __restrict__ sqdiff) {
  extern __shared__ __attribute__((aligned(16))) unsigned cr_hist[];   // [3][n]
  __shared__ long long red[CR_WAVES];
  const int tid = threadIdx.x;
  for (int b = tid; b < 3 * n; b += CR_THREADS) cr_hist[b] = 0;
  __syncthreads();
  const int first = blockIdx.x * CR_ROWS, last = min(m, first + CR_ROWS);
  for (int r = first; r < last; ++r) {
    long long s = 0;
    for (int j = tid; j < n; j += CR_THREADS) {
      const int a = rank_high[(long long)r * ldh + j], b = rank_low[(long long)r * ldl + j];
      if (a < 1 || a > n - 1 || b < 1 || b > n - 1) continue;   // the own column; a foreign value is never an index
      const int which = a == b ? 0 : (b < a ? 1 : 2);
      atomicAdd(&cr_hist[which * n + max(a, b)], 1u);
      s += (long long)(a - b) * (a - b);
    }
    s = block_sum<CR_WAVES>(s, red);
    if (tid == 0) sqdiff[r] = s;
  }
  __syncthreads();
  for (int b = tid; b < 3 * n; b += CR_THREADS) {
    const unsigned v = cr_hist[b];
    if (v) atomicAdd(&hist[b], v);
  }
}

__device__ __forceinline__ int cr_bin(float v, float scale, int bins) {
  const float t = v * scale;
  if (!(t < (float)(bins - 1))) return bins - 1;           // the top of the range, +inf, NaN
  return t < 0.f ? 0 : (int)t;
}

__global__ __launch_bounds__(CR_THREADS) void shepard_fold_kernel(const float* __restrict__ dist_high, long long ldh,
                                                                  const float* __restrict__ dist_low, long long ldl, int n,
                                                                  const float* __restrict__ scale, int bins,
                                                                  double* __restrict__ sums, unsigned* __restrict__ hist) {
#pragma clang fp reassociate(off)
  extern __shared__ __attribute__((aligned(16))) unsigned cr_hist[];   // [bins][bins]
  __shared__ double red[3][CR_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = tid; b < bins * bins; b += CR_THREADS) cr_hist[b] = 0;
  __syncthreads();
  const float sh = scale[0], sl = scale[1];
  const int first = blockIdx.x * CR_ROWS, last = min(n, first + CR_ROWS);
  for (int r = first; r < last; ++r) {
    const float* __restrict__ rh = dist_high + (long long)r * ldh;
    const float* __restrict__ rl = dist_low + (long long)r * ldl;
    double acc[3][4] = {};
    for (int j0 = tid; j0 < n; j0 += 4 * CR_THREADS) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = j0 + q * CR_THREADS;
        if (j < n && j != r) {
          const float fh = rh[j], fl = rl[j];
          const double a = (double)fh, b = (double)fl;
          acc[0][q] += a * a;
          acc[1][q] += b * b;
          acc[2][q] += a * b;
          atomicAdd(&cr_hist[cr_bin(fh, sh, bins) * bins + cr_bin(fl, sl, bins)], 1u);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = (acc[c][0] + acc[c][1]) + (acc[c][2] + acc[c][3]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
      if (lane == 0) red[c][wave] = s;
    }
    __syncthreads();
    if (tid < 3) sums[(long long)r * 3 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    __syncthreads();                                       // red is written again for the next row
  }
  for (int b = tid; b < bins * bins; b += CR_THREADS) {
    const unsigned v = cr_hist[b];
    if (v) atomicAdd(&hist[b], v);
  }
}

// 0 when n is admitted
int cr_check_n(const char* who, int n) {
  if (n < CR_MIN_N) PTI_FAIL(PTI_EINVAL, "%s: bad dimension n=%d (at least %d rows)", who, n, CR_MIN_N);
  if (n > CR_MAX_N) PTI_FAIL(PTI_EUNSUPPORTED, "%s: unsupported shape n=%d (at most %d rows)", who, n, CR_MAX_N);
  return PTI_OK;
}

}  // namespace

extern "C" int pti_full_ranks(const float* dist, int64_t ldd, int m, int n, int row0, int16_t* out, int64_t ldo, pti_stream_t s) {
  if (!dist || !out) PTI_FAIL(PTI_EINVAL, "full_ranks: null pointer");
  if (int rc = cr_check_n("full_ranks", n)) return rc;
  if (m < 1) PTI_FAIL(PTI_EINVAL, "full_ranks: bad dimension m=%d (at least 1 row)", m);
  if (row0 < 0 || m > n || row0 > n - m)
    PTI_FAIL(PTI_EINVAL, "full_ranks: row range %d .. %lld outside the matrix of n=%d rows", row0, (long long)row0 + m - 1, n);
  if (ldd < n || ldo < n)
    PTI_FAIL(PTI_EINVAL, "full_ranks: row stride below the row length (ldd=%lld ldo=%lld n=%d)", (long long)ldd, (long long)ldo, n);
  if (((uintptr_t)dist & 3) || ((uintptr_t)out & 1)) PTI_FAIL(PTI_EINVAL, "full_ranks: misaligned buffer");
  int np2 = CR_MIN_N;
  while (np2 < n) np2 <<= 1;                               // at most 8192 keys: 64 KB of LDS
  if (np2 >= CR_SORT_WIDE_KEYS)
    PTI_LAUNCH(full_ranks_kernel<CR_SORT_WIDE>, dim3((unsigned)m), dim3(CR_SORT_WIDE), (size_t)np2 * sizeof(cr_key), (hipStream_t)s,
               dist, (long long)ldd, n, row0, np2, (short*)out, (long long)ldo);
  else
    PTI_LAUNCH(full_ranks_kernel<CR_THREADS>, dim3((unsigned)m), dim3(CR_THREADS), (size_t)np2 * sizeof(cr_key), (hipStream_t)s,
               dist, (long long)ldd, n, row0, np2, (short*)out, (long long)ldo);
  PTI_CHECK_LAUNCH("full_ranks");
  return PTI_OK;
}

extern "C" int pti_coranking_fold(const int16_t* rank_high, int64_t ldh, const int16_t* rank_low, int64_t ldl, int m, int n,
                                  uint32_t* hist, int64_t* sqdiff, pti_stream_t s) {
  if (!rank_high || !rank_low || !hist || !sqdiff) PTI_FAIL(PTI_EINVAL, "coranking_fold: null pointer");
  if (int rc = cr_check_n("coranking_fold", n)) return rc;
  if (m < 1) PTI_FAIL(PTI_EINVAL, "coranking_fold: bad dimension m=%d (at least 1 row)", m);
  if (m > n) PTI_FAIL(PTI_EINVAL, "coranking_fold: row range of m=%d rows outside the matrix of n=%d rows", m, n);
  if (ldh < n || ldl < n)
    PTI_FAIL(PTI_EINVAL, "coranking_fold: row stride below the row length (ldh=%lld ldl=%lld n=%d)", (long long)ldh, (long long)ldl,
             n);
  if (((uintptr_t)rank_high & 1) || ((uintptr_t)rank_low & 1) || ((uintptr_t)hist & 3) || ((uintptr_t)sqdiff & 7))
    PTI_FAIL(PTI_EINVAL, "coranking_fold: misaligned buffer");
  PTI_LAUNCH(coranking_fold_kernel, dim3((unsigned)cdiv(m, CR_ROWS)), dim3(CR_THREADS), (size_t)3 * n * sizeof(unsigned),
             (hipStream_t)s, (const short*)rank_high, (long long)ldh, (const short*)rank_low, (long long)ldl, m, n, (unsigned*)hist,
             (long long*)sqdiff);
  PTI_CHECK_LAUNCH("coranking_fold");
  return PTI_OK;
}

extern "C" int pti_shepard_fold(const float* dist_high, int64_t ldh, const float* dist_low, int64_t ldl, int n, const float* scale,
                                int bins, double* sums, uint32_t* hist, pti_stream_t s) {
  if (!dist_high || !dist_low || !scale || !sums || !hist) PTI_FAIL(PTI_EINVAL, "shepard_fold: null pointer");
  if (int rc = cr_check_n("shepard_fold", n)) return rc;
  if (bins < CR_MIN_BINS) PTI_FAIL(PTI_EINVAL, "shepard_fold: bad dimension bins=%d (at least %d)", bins, CR_MIN_BINS);
  if (bins > CR_MAX_BINS) PTI_FAIL(PTI_EUNSUPPORTED, "shepard_fold: unsupported bins=%d (at most %d)", bins, CR_MAX_BINS);
  if (ldh < n || ldl < n)
    PTI_FAIL(PTI_EINVAL, "shepard_fold: row stride below the row length (ldh=%lld ldl=%lld n=%d)", (long long)ldh, (long long)ldl, n);
  if (((uintptr_t)dist_high & 3) || ((uintptr_t)dist_low & 3) || ((uintptr_t)scale & 3) || ((uintptr_t)sums & 7) ||
      ((uintptr_t)hist & 3))
    PTI_FAIL(PTI_EINVAL, "shepard_fold: misaligned buffer");
  PTI_LAUNCH(shepard_fold_kernel, dim3((unsigned)cdiv(n, CR_ROWS)), dim3(CR_THREADS), (size_t)bins * bins * sizeof(unsigned),
             (hipStream_t)s, dist_high, (long long)ldh, dist_low, (long long)ldl, n, scale, bins, sums, (unsigned*)hist);
  PTI_CHECK_LAUNCH("shepard_fold");
  return PTI_OK;
}
