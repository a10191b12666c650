// Two-sample permutation tests of two groups of latent rows on the device (gfx950): the exact lower median of a distance
// matrix's upper triangle, the 16-bit integer weight matrices of the tests, and the permutation fold
//     A[p] = s_p^T W s_p,   R[p] = s_p . (W 1),   C[p] = s_p . (W^T 1)
// for P 0/1 labellings s_p of one n x n integer matrix W with entries in [0, 65535].  4 <= n <= 8192, 1 <= P <= 65536.
// DESIGN.md 5u.
//
//   pti_distance_median: an MSB-first radix select over the bit patterns of the strictly-upper-triangle entries (the bits
//     of a non-negative float order as the float does).  Four passes of eight bits: a histogram launch (one workgroup per
//     row, 256 bins in LDS, folded into 256 global counters) and a one-workgroup launch that walks the bins, fixes the next
//     byte of the answer and the rank inside the bin, and clears the counters.  The prefix and the rank stay on the device.
//   pti_two_sample_kernel: one thread per entry, the expression in fp64 from the fp32 distance, rounded once.  The energy
//     kind's scale (the matrix maximum) comes from an integer atomicMax over the bit patterns in a launch of its own.
//   pti_knn_indicator: one workgroup per row clears the row and sets the listed columns.
//   pti_permutation_forms, five launches:
//     1 split    W -> two byte planes, low and high, each biased by -128 into int8 and stored TRANSPOSED (plane[j][i], rows
//                of n_pad = n rounded up to 64 bytes) so that the k index of the product runs along memory for both MFMA
//                operands; 64 x 64 tiles through LDS, reads and writes both coalesced.  The same pass adds W's row and
//                column sums with 32-bit integer atomics (a sum is at most 8192 * 65535 < 2^30).
//     2 pad      the labellings as int8 rows of n_pad bytes, zero behind column n.
//     3 linear   one workgroup per labelling: the number of ones c, R, C; A starts at the bias term c^2 * 128 * 257.
//     4 fold     T = S . plane on v_mfma_i32_16x16x64_i8 (M = labellings, N = columns j, K = rows i), both planes in one
//                pass over S.  A workgroup of four waves owns 128 labellings x 64 columns and walks PF_JT such column tiles;
//                a wave holds 4 x 2 fragments per plane.  An i32 accumulator holds at most 8192 * 128 = 2^20 in magnitude,
//                the two planes combine as lo + 256 hi < 2^29 in i32, and the epilogue adds s[p][j] (lo + 256 hi) over the
//                wave's columns in int64.  The 16 lanes that share a labelling fold by an xor butterfly and one lane adds
//                the result to A[p] with a 64-bit integer atomic.
//     Both MFMA operands are read with the SAME (lane group, byte) -> k map, so the product does not depend on how the
//     instruction orders k inside a step; rows and columns follow the C/D map col = lane & 15, row = 4 (lane >> 4) + reg.
//   Integer arithmetic only, and integer addition is associative: every output is exact, independent of tiling, launch
//   order and the order in which the atomics land, hence bitwise reproducible.
#include "pti_common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int TS_MIN_N = 4;
constexpr int TS_MAX_N = 8192;
constexpr int TS_MAX_P = 65536;
constexpr int TS_MAX_BW = 8;
constexpr int TS_THREADS = 256;
constexpr int TS_MEDIAN_WORDS = 256 + 2;      // 256 counters, the prefix, the rank

struct ts_bandwidths {
  double b[TS_MAX_BW];
  int count;
};

// ---- median ---------------------------------------------------------------------------------------------------------
// state[256] = the bytes fixed so far, state[257] = the rank wanted among the entries that share them
__global__ __launch_bounds__(TS_THREADS) void median_hist_kernel(const float* __restrict__ dist, long long ldd, int n, int pass,
                                                                 uint32_t* __restrict__ state) {
  __shared__ uint32_t bins[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  bins[tid] = 0;
  __syncthreads();
  const uint32_t prefix = pass ? state[256] : 0u;
  const int shift = 24 - 8 * pass;
  const float* __restrict__ row = dist + (long long)i * ldd;
  for (int j = i + 1 + tid; j < n; j += TS_THREADS) {
    const uint32_t bits = neighbor_order_bits(row[j]);
    if (pass == 0 || (bits >> (shift + 8)) == prefix) atomicAdd(&bins[(bits >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (bins[tid]) atomicAdd(&state[tid], bins[tid]);
}

__global__ __launch_bounds__(TS_THREADS) void median_pick_kernel(uint32_t* __restrict__ state, int pass, uint32_t rank0,
                                                                 float* __restrict__ out) {
  __shared__ uint32_t bins[256];
  const int tid = threadIdx.x;
  bins[tid] = state[tid];
  __syncthreads();
  state[tid] = 0;                                        // ready for the next pass
  if (tid == 0) {
    uint32_t rank = pass ? state[257] : rank0, prefix = pass ? state[256] : 0u, below = 0;
    int b = 0;
    for (; b < 255; ++b) {
      if (rank < below + bins[b]) break;
      below += bins[b];
    }
    prefix = (prefix << 8) | (uint32_t)b;
    state[256] = prefix;
    state[257] = rank - below;
    if (pass == 3) *out = __uint_as_float(prefix);
  }
}

// ---- weight matrices ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void matrix_max_kernel(const float* __restrict__ dist, long long ldd, int n,
                                                                uint32_t* __restrict__ out_bits) {
  const int i = blockIdx.x;
  const float* __restrict__ row = dist + (long long)i * ldd;
  uint32_t m = 0;
  for (int j = threadIdx.x; j < n; j += TS_THREADS) m = max(m, neighbor_order_bits(row[j]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out_bits, m);
}

__global__ __launch_bounds__(TS_THREADS) void two_sample_kernel_kernel(const float* __restrict__ dist, long long ldd, int n,
                                                                       int energy, const float* __restrict__ scale_ptr,
                                                                       ts_bandwidths bw, int* __restrict__ out) {
#pragma clang fp reassociate(off)
  const int i = blockIdx.y, j = blockIdx.x * TS_THREADS + threadIdx.x;
  if (j >= n) return;
  const double scale = (double)*scale_ptr;
  int w = 0;
  if (i != j && scale > 0.0) {
    const double d = (double)dist[(long long)i * ldd + j];
    double v;
    if (energy) {
      v = 65535.0 * d / scale;
    } else {
      double acc = 0.0;
      for (int b = 0; b < bw.count; ++b) {
        const double sigma = bw.b[b] * scale;
        acc += exp(-(d * d) / (2.0 * sigma * sigma));
      }
      v = 65535.0 * (acc / (double)bw.count);
    }
    v = rint(v);
    w = v >= 65535.0 ? 65535 : (v > 0.0 ? (int)v : 0);
  }
  out[(long long)i * n + j] = w;
}

__global__ __launch_bounds__(TS_THREADS) void knn_indicator_kernel(const int* __restrict__ knn_idx, int n, int k,
                                                                   int* __restrict__ out) {
  const int i = blockIdx.x, tid = threadIdx.x;
  int* __restrict__ row = out + (long long)i * n;
  for (int j = tid; j < n; j += TS_THREADS) row[j] = 0;
  __syncthreads();
  for (int c = tid; c < k; c += TS_THREADS) {
    const int j = knn_idx[(long long)i * k + c];
    if (j >= 0 && j < n && j != i) row[j] = 1;
  }
}

// ---- permutation fold -----------------------------------------------------------------------------------------------
constexpr int PF_BM = 128;   // labellings per workgroup
constexpr int PF_BN = 64;    // columns per tile
constexpr int PF_BK = 64;    // one MFMA k-step
constexpr int PF_JT = 8;     // column tiles a workgroup walks
constexpr long long PF_BIAS = 128LL * 257LL;

__host__ __device__ inline int pf_pad(int n) { return (n + 63) & ~63; }

// one 256-thread workgroup per 64 x 64 tile of W: plane[j][i] (bytes) from w[i][j]
__global__ __launch_bounds__(TS_THREADS) void pf_split_kernel(const int* __restrict__ w, long long ldw, int n, int n_pad,
                                                              int8_t* __restrict__ lo, int8_t* __restrict__ hi,
                                                              uint32_t* __restrict__ rsum, uint32_t* __restrict__ csum) {
  __shared__ uint32_t tile[64][65];
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  uint32_t col = 0;
  for (int r = ty; r < 64; r += 4) {
    const int i = i0 + r, j = j0 + tx;
    uint32_t v = 0;
    if (i < n && j < n) v = (uint32_t)w[(long long)i * ldw + j] & 0xffffu;
    tile[r][tx] = v;
    col += v;
    const uint32_t rs = wave_sum(v);
    if (tx == 0 && i < n && rs) atomicAdd(&rsum[i], rs);
  }
  if (j0 + tx < n && col) atomicAdd(&csum[j0 + tx], col);
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {                       // r: column j of W, tx: row i of W
    const int i = i0 + tx, j = j0 + r;
    const uint32_t v = tile[tx][r];
    const bool in = i < n && j < n;                        // padding holds 0: it only ever meets a zero label
    const long long at = (long long)j * n_pad + i;
    lo[at] = in ? (int8_t)((int)(v & 255u) - 128) : (int8_t)0;
    hi[at] = in ? (int8_t)((int)(v >> 8) - 128) : (int8_t)0;
  }
}

// 16 bytes of a padded labelling per thread
__global__ __launch_bounds__(TS_THREADS) void pf_pad_kernel(const uint8_t* __restrict__ masks, int n, int n_pad, long long chunks,
                                                            int8_t* __restrict__ out) {
  const long long c = (long long)blockIdx.x * TS_THREADS + threadIdx.x;
  if (c >= chunks) return;
  const int per_row = n_pad / 16;
  const long long p = c / per_row;
  const int j0 = (int)(c % per_row) * 16;
  u32x4 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + 4 * q + u;
      if (j < n && masks[p * n + j]) word |= 1u << (8 * u);
    }
    v[q] = word;
  }
  *(u32x4*)(out + p * n_pad + j0) = v;
}

// one workgroup per labelling: R, C and the bias term of A
__global__ __launch_bounds__(TS_THREADS) void pf_linear_kernel(const int8_t* __restrict__ sp, int n, int n_pad,
                                                               const uint32_t* __restrict__ rsum,
                                                               const uint32_t* __restrict__ csum, long long* __restrict__ out) {
  __shared__ long long red[TS_THREADS / 64];
  const long long p = blockIdx.x;
  const int8_t* __restrict__ row = sp + p * n_pad;
  long long cnt = 0, r = 0, c = 0;
  for (int j = threadIdx.x; j < n; j += TS_THREADS) {
    if (row[j]) {
      cnt += 1;
      r += (long long)rsum[j];
      c += (long long)csum[j];
    }
  }
  cnt = block_sum<TS_THREADS / 64>(cnt, red);
  r = block_sum<TS_THREADS / 64>(r, red);
  c = block_sum<TS_THREADS / 64>(c, red);
  if (threadIdx.x == 0) {
    out[p * 3 + 0] = cnt * cnt * PF_BIAS;
    out[p * 3 + 1] = r;
    out[p * 3 + 2] = c;
  }
}

__global__ __launch_bounds__(TS_THREADS) void pf_fold_kernel(const int8_t* __restrict__ sp, const int8_t* __restrict__ lo,
                                                             const int8_t* __restrict__ hi, int n_pad, int P,
                                                             long long* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int p0 = blockIdx.x * PF_BM + wm * 64;
  const int tiles = n_pad / PF_BN;
  const int jt0 = blockIdx.y * PF_JT, jt1 = min(jt0 + PF_JT, tiles);

  const int8_t* arow[4];                                   // the wave's labellings; rows past P repeat the last one and are dropped
#pragma unroll
  for (int m = 0; m < 4; ++m) arow[m] = sp + (long long)min(p0 + m * 16 + fr, P - 1) * n_pad + 16 * fq;

  long long sum[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[m][r] = 0;

  for (int jt = jt0; jt < jt1; ++jt) {
    const int jw = jt * PF_BN + wn * 32;
    const int8_t* blo[2];
    const int8_t* bhi[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const long long at = (long long)(jw + f * 16 + fr) * n_pad + 16 * fq;
      blo[f] = lo + at;
      bhi[f] = hi + at;
    }
    i32x4 acc_lo[4][2], acc_hi[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        acc_lo[m][f] = i32x4{0, 0, 0, 0};
        acc_hi[m][f] = i32x4{0, 0, 0, 0};
      }
    for (int k0 = 0; k0 < n_pad; k0 += PF_BK) {
      i32x4 a[4], bl[2], bh[2];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = *(const i32x4*)(arow[m] + k0);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        bl[f] = *(const i32x4*)(blo[f] + k0);
        bh[f] = *(const i32x4*)(bhi[f] + k0);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          acc_lo[m][f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], bl[f], acc_lo[m][f], 0, 0, 0);
          acc_hi[m][f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], bh[f], acc_hi[m][f], 0, 0, 0);
        }
    }
    // C/D map: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int8_t* srow = sp + (long long)min(p0 + m * 16 + 4 * fq + r, P - 1) * n_pad;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int t = acc_lo[m][f][r] + 256 * acc_hi[m][f][r];
          if (srow[jw + f * 16 + fr]) sum[m][r] += (long long)t;
        }
      }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      long long v = sum[m][r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      const int p = p0 + m * 16 + 4 * fq + r;
      if (fr == 0 && p < P && v != 0) atomicAdd((unsigned long long*)&out[(long long)p * 3], (unsigned long long)v);
    }
}

size_t pf_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" int64_t pti_distance_median_ws_bytes(int n) {
  if (n < TS_MIN_N || n > TS_MAX_N) return 0;
  return (int64_t)TS_MEDIAN_WORDS * 4;
}

extern "C" int pti_distance_median(const float* dist, int64_t ldd, int n, float* out, void* workspace, int64_t ws_bytes,
                                   pti_stream_t s) {
  if (!dist || !out || !workspace) PTI_FAIL(PTI_EINVAL, "distance_median: null pointer");
  if (n < TS_MIN_N) PTI_FAIL(PTI_EINVAL, "distance_median: bad dimension n=%d (at least %d rows)", n, TS_MIN_N);
  if (n > TS_MAX_N) PTI_FAIL(PTI_EUNSUPPORTED, "distance_median: unsupported shape n=%d (at most %d rows)", n, TS_MAX_N);
  if (ldd < n) PTI_FAIL(PTI_EINVAL, "distance_median: row stride below the row length (ldd=%lld n=%d)", (long long)ldd, n);
  if (((uintptr_t)dist & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 3))
    PTI_FAIL(PTI_EINVAL, "distance_median: misaligned buffer");
  if (ws_bytes < pti_distance_median_ws_bytes(n)) PTI_FAIL(PTI_EINVAL, "distance_median: workspace too small");
  uint32_t* state = (uint32_t*)workspace;
  if (hipMemsetAsync(state, 0, (size_t)TS_MEDIAN_WORDS * 4, (hipStream_t)s) != hipSuccess)
    PTI_FAIL(PTI_ELAUNCH, "distance_median: memset failed");
  const long long m = (long long)n * (n - 1) / 2;
  const uint32_t rank0 = (uint32_t)((m - 1) / 2);
  for (int pass = 0; pass < 4; ++pass) {
    PTI_LAUNCH(median_hist_kernel, dim3((unsigned)(n - 1)), dim3(TS_THREADS), 0, (hipStream_t)s, dist, (long long)ldd, n, pass,
               state);
    PTI_LAUNCH(median_pick_kernel, dim3(1), dim3(TS_THREADS), 0, (hipStream_t)s, state, pass, rank0, out);
  }
  PTI_CHECK_LAUNCH("distance_median");
  return PTI_OK;
}

extern "C" int pti_two_sample_kernel(const float* dist, int64_t ldd, int n, int kind, const float* scale_or_null,
                                     const double* bandwidths, int n_bandwidths, int32_t* out, float* scale_out, pti_stream_t s) {
  if (!dist || !out || !scale_out) PTI_FAIL(PTI_EINVAL, "two_sample_kernel: null pointer");
  if (kind != 0 && kind != 1) PTI_FAIL(PTI_EINVAL, "two_sample_kernel: kind must be 0 (gaussian) or 1 (energy), got %d", kind);
  if (n < TS_MIN_N) PTI_FAIL(PTI_EINVAL, "two_sample_kernel: bad dimension n=%d (at least %d rows)", n, TS_MIN_N);
  if (n > TS_MAX_N) PTI_FAIL(PTI_EUNSUPPORTED, "two_sample_kernel: unsupported shape n=%d (at most %d rows)", n, TS_MAX_N);
  if (ldd < n) PTI_FAIL(PTI_EINVAL, "two_sample_kernel: row stride below the row length (ldd=%lld n=%d)", (long long)ldd, n);
  if (((uintptr_t)dist & 3) || ((uintptr_t)out & 3) || ((uintptr_t)scale_out & 3) || ((uintptr_t)scale_or_null & 3))
    PTI_FAIL(PTI_EINVAL, "two_sample_kernel: misaligned buffer");
  ts_bandwidths bw;
  bw.count = 0;
  for (int b = 0; b < TS_MAX_BW; ++b) bw.b[b] = 1.0;
  if (kind == 0) {
    if (!scale_or_null) PTI_FAIL(PTI_EINVAL, "two_sample_kernel: the gaussian kind needs a scale");
    if (!bandwidths || n_bandwidths < 1 || n_bandwidths > TS_MAX_BW)
      PTI_FAIL(PTI_EINVAL, "two_sample_kernel: 1 .. %d bandwidths, got %d", TS_MAX_BW, n_bandwidths);
    for (int b = 0; b < n_bandwidths; ++b) {
      if (!(bandwidths[b] > 0.0) || bandwidths[b] > 1e30)
        PTI_FAIL(PTI_EINVAL, "two_sample_kernel: bandwidth %d must be positive and finite", b);
      bw.b[b] = bandwidths[b];
    }
    bw.count = n_bandwidths;
  }
  if (scale_or_null) {
    if (scale_or_null != scale_out &&
        hipMemcpyAsync(scale_out, scale_or_null, 4, hipMemcpyDeviceToDevice, (hipStream_t)s) != hipSuccess)
      PTI_FAIL(PTI_ELAUNCH, "two_sample_kernel: copy failed");
  } else {
    if (hipMemsetAsync(scale_out, 0, 4, (hipStream_t)s) != hipSuccess) PTI_FAIL(PTI_ELAUNCH, "two_sample_kernel: memset failed");
    PTI_LAUNCH(matrix_max_kernel, dim3((unsigned)n), dim3(TS_THREADS), 0, (hipStream_t)s, dist, (long long)ldd, n,
               (uint32_t*)scale_out);
  }
  PTI_LAUNCH(two_sample_kernel_kernel, dim3((unsigned)cdiv(n, TS_THREADS), (unsigned)n), dim3(TS_THREADS), 0, (hipStream_t)s, dist,
             (long long)ldd, n, kind, (const float*)scale_out, bw, (int*)out);
  PTI_CHECK_LAUNCH("two_sample_kernel");
  return PTI_OK;
}

extern "C" int pti_knn_indicator(const int32_t* knn_idx, int n, int k, int32_t* out, pti_stream_t s) {
  if (!knn_idx || !out) PTI_FAIL(PTI_EINVAL, "knn_indicator: null pointer");
  if (n < TS_MIN_N) PTI_FAIL(PTI_EINVAL, "knn_indicator: bad dimension n=%d (at least %d rows)", n, TS_MIN_N);
  if (k < 1 || k > n) PTI_FAIL(PTI_EINVAL, "knn_indicator: bad dimension k=%d (1 .. n listed neighbours)", k);
  if (n > TS_MAX_N) PTI_FAIL(PTI_EUNSUPPORTED, "knn_indicator: unsupported shape n=%d (at most %d rows)", n, TS_MAX_N);
  if (((uintptr_t)knn_idx & 3) || ((uintptr_t)out & 3)) PTI_FAIL(PTI_EINVAL, "knn_indicator: misaligned buffer");
  PTI_LAUNCH(knn_indicator_kernel, dim3((unsigned)n), dim3(TS_THREADS), 0, (hipStream_t)s, (const int*)knn_idx, n, k, (int*)out);
  PTI_CHECK_LAUNCH("knn_indicator");
  return PTI_OK;
}

// workspace: two planes of n_pad^2 bytes, P padded labellings of n_pad bytes, the row and column sums (2 n words); each
// part starts on a 256-byte boundary
extern "C" int64_t pti_permutation_forms_ws_bytes(int n, int p) {
  if (n < TS_MIN_N || n > TS_MAX_N || p < 1 || p > TS_MAX_P) return 0;
  const size_t np = (size_t)pf_pad(n);
  return (int64_t)(2 * pf_align(np * np) + pf_align((size_t)p * np) + pf_align((size_t)2 * n * 4));
}

extern "C" int pti_permutation_forms(const int32_t* w, int64_t ldw, int n, const uint8_t* masks, int p, int64_t* out,
                                     void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!w || !masks || !out || !workspace) PTI_FAIL(PTI_EINVAL, "permutation_forms: null pointer");
  if (n < TS_MIN_N || p < 1)
    PTI_FAIL(PTI_EINVAL, "permutation_forms: bad dimension n=%d p=%d (at least %d rows, 1 labelling)", n, p, TS_MIN_N);
  if (n > TS_MAX_N || p > TS_MAX_P)
    PTI_FAIL(PTI_EUNSUPPORTED, "permutation_forms: unsupported shape n=%d p=%d (at most %d rows, %d labellings)", n, p, TS_MAX_N,
             TS_MAX_P);
  if (ldw < n) PTI_FAIL(PTI_EINVAL, "permutation_forms: row stride below the row length (ldw=%lld n=%d)", (long long)ldw, n);
  if (((uintptr_t)w & 3) || ((uintptr_t)out & 7) || ((uintptr_t)workspace & 15))
    PTI_FAIL(PTI_EINVAL, "permutation_forms: misaligned buffer");
  if (ws_bytes < pti_permutation_forms_ws_bytes(n, p)) PTI_FAIL(PTI_EINVAL, "permutation_forms: workspace too small");
  const int np = pf_pad(n);
  const size_t plane = pf_align((size_t)np * np);
  int8_t* lo = (int8_t*)workspace;
  int8_t* hi = lo + plane;
  int8_t* sp = hi + plane;
  uint32_t* rsum = (uint32_t*)(sp + pf_align((size_t)p * np));
  uint32_t* csum = rsum + n;
  hipStream_t st = (hipStream_t)s;
  if (hipMemsetAsync(rsum, 0, (size_t)2 * n * 4, st) != hipSuccess) PTI_FAIL(PTI_ELAUNCH, "permutation_forms: memset failed");
  PTI_LAUNCH(pf_split_kernel, dim3((unsigned)(np / 64), (unsigned)(np / 64)), dim3(TS_THREADS), 0, st, (const int*)w,
             (long long)ldw, n, np, lo, hi, rsum, csum);
  const long long chunks = (long long)p * (np / 16);
  PTI_LAUNCH(pf_pad_kernel, dim3((unsigned)((chunks + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0, st, masks, n, np, chunks,
             sp);
  PTI_LAUNCH(pf_linear_kernel, dim3((unsigned)p), dim3(TS_THREADS), 0, st, (const int8_t*)sp, n, np, (const uint32_t*)rsum,
             (const uint32_t*)csum, (long long*)out);
  PTI_LAUNCH(pf_fold_kernel, dim3((unsigned)cdiv(p, PF_BM), (unsigned)cdiv(np / PF_BN, PF_JT)), dim3(TS_THREADS), 0, st,
             (const int8_t*)sp, (const int8_t*)lo, (const int8_t*)hi, np, p, (long long*)out);
  PTI_CHECK_LAUNCH("permutation_forms");
  return PTI_OK;
}
