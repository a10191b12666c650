// The integer primitives under the disentanglement report of an AR-VAE on the device (gfx950): average ranks with ties, the
// moments of those ranks (Spearman's rho), and joint histograms of discretised columns (mutual information -> MIG,
// modularity).  Every result is an integer formed by counting or by 64-bit integer sums: exact, independent of the order of
// evaluation and of row padding, bitwise reproducible.  The library is built with -ffast-math, so no sign or equality of
// two FLOATS is ever taken by subtracting them: they are compared, directly or through integer keys that order like them.
// (tests/disentanglement_oracle.py is the plain restatement.)
//
// pti_tied_ranks, one launch: one 256-thread workgroup per (256-row tile, column).  Thread t owns row i = 256 tile + t and
//   adds, over ALL j, the three-way comparison of x_i with x_j; the j run through LDS in tiles of 256 (as keys) and are
//   read back as broadcast 16-byte loads, four j per read.  rank2 = n + 1 + sum_j cmp(x_i, x_j) = twice the average rank.
// pti_rank_moments, one launch: one workgroup per pair of columns a <= b; 32 x 32 -> 64-bit multiply-adds per thread, a
//   shuffle fold over the wave, an LDS fold over the four waves; the mirror cell and (a == b) the column sum ride along.
// pti_joint_histogram, three launches: (1) bin index of every value by counting the left edges not above it (fp64
//   compares); (2) one workgroup per (chunk of JH_ROWS rows, channel, group of JH_QB attributes) counts its rows into
//   [JH_QB][B][B] int32 tables in LDS with integer LDS adds and stores them as its partial; (3) the partials of all chunks
//   are added in chunk order.  A value below its first edge (or a NaN) gets bin 255 and is counted nowhere.
#include "pti_common.h"

namespace {

constexpr int DT_TILE = 256;                     // rows per workgroup = values per LDS tile = threads
constexpr int DT_MAXN = 32768, DT_MAXCOLS = 32;
constexpr int JH_MAXL = 16, JH_MAXNA = 16, JH_MAXB = 32;
constexpr int JH_QB = 8;                         // attributes per workgroup: 8 x 32 x 32 int32 = 32 KB of LDS
constexpr int JH_ROWS = 2048;                    // rows per workgroup of the counting launch
constexpr int JH_NOBIN = 255;

typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int DT_PAD_KEY = (int)0x80000000;   // below the key of every number: the key of no finite value or infinity

// The bits of x as a signed integer that orders like x: an integer COMPARISON of two keys is the float comparison of the
// two values, with -0.0 folded onto 0.0 in the bits (a float select would be a no-op under -ffast-math).  No float is
// ever subtracted; integer arithmetic is exact whatever the math flags are.
__device__ __forceinline__ int dt_key(float x) {
  int b = __float_as_int(x);
  b = (b & 0x7fffffff) == 0 ? 0 : b;
  return b ^ ((b >> 31) & 0x7fffffff);
}

// d clamped to [-1, 1].  Written as min(max(d, -1), 1) the compiler turns it back into two compares and two selects; the
// instruction has vector register operands only, so nothing needs padding around it.
__device__ __forceinline__ int dt_sign(int d) {
  int s;
  asm("v_med3_i32 %0, %1, -1, 1" : "=v"(s) : "v"(d));
  return s;
}

// 2 #{x_j < x_i} + #{x_j == x_i} = n + sum_j cmp(x_i, x_j), cmp = -1 / 0 / +1: the three-way comparison of two keys is their
// SATURATING difference clamped to [-1, 1] -- v_sub_i32 clamp, v_med3_i32, one add per pair, all in vector registers
// (two v_cmp per pair put their masks in scalar registers, and the wait states behind them cost a third of the issue slots)
__global__ __launch_bounds__(DT_TILE) void tied_ranks_kernel(const float* __restrict__ cols, long long ld, int n,
                                                             int* __restrict__ rank2) {
  __shared__ __attribute__((aligned(16))) int s_k[DT_TILE];
  const int tid = threadIdx.x, i = blockIdx.x * DT_TILE + tid;
  const float* __restrict__ col = cols + (long long)blockIdx.y * ld;
  const int ki = i < n ? dt_key(col[i]) : 0;
  int acc = 0;
  for (int j0 = 0; j0 < n; j0 += DT_TILE) {
    __syncthreads();   // the previous tile has been read
    s_k[tid] = j0 + tid < n ? dt_key(col[j0 + tid]) : DT_PAD_KEY;   // a padding entry counts +1 for every row: taken off below
    __syncthreads();
#pragma unroll 4
    for (int jb = 0; jb < DT_TILE; jb += 4) {
      const i32x4 kj = *(const i32x4*)&s_k[jb];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += dt_sign(__builtin_elementwise_sub_sat(ki, kj[u]));
    }
  }
  const int pad = (int)gridDim.x * DT_TILE - n;   // the grid holds cdiv(n, DT_TILE) row tiles, as many as there are j tiles
  if (i < n) rank2[(long long)blockIdx.y * n + i] = n + 1 + acc - pad;
}

__global__ __launch_bounds__(DT_TILE) void rank_moments_kernel(const int* __restrict__ rank2, int n, int m,
                                                               long long* __restrict__ sums, long long* __restrict__ gram) {
  __shared__ unsigned long long s_red[DT_TILE / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = blockIdx.x, b = blockIdx.y;
  if (b < a) return;   // block-uniform: the cell is written by its mirror
  const int* __restrict__ ra = rank2 + (long long)a * n;
  const int* __restrict__ rb = rank2 + (long long)b * n;
  unsigned long long dot = 0, sum = 0;
  for (int i = tid; i < n; i += DT_TILE) {
    const unsigned va = (unsigned)ra[i], vb = (unsigned)rb[i];
    dot += (unsigned long long)va * vb;   // one 32 x 32 -> 64-bit multiply-add
    sum += va;
  }
  dot = wave_sum(dot);
  sum = wave_sum(sum);
  if (lane == 0) {
    s_red[wave][0] = dot;
    s_red[wave][1] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long d = 0, s = 0;
#pragma unroll
    for (int w = 0; w < DT_TILE / 64; ++w) {
      d += s_red[w][0];
      s += s_red[w][1];
    }
    gram[(long long)a * m + b] = (long long)d;
    gram[(long long)b * m + a] = (long long)d;
    if (a == b) sums[a] = (long long)s;
  }
}

struct JhArgs {
  const float* zt;
  const float* attrs;
  long long ldz, lda;
  int n, l, na, bins, chunks;
  const double* edges_z;
  const double* edges_a;
  unsigned char* bins_z;   // [l][n]
  unsigned char* bins_a;   // [na][n]
  int* ws;                 // [chunks][na][l][bins][bins]
  int* counts;             // [na][l][bins][bins]
};

// one workgroup per (256-row tile, column): columns 0 .. l - 1 are the channels, l .. l + na - 1 the attributes
__global__ __launch_bounds__(DT_TILE) void joint_histogram_bin_kernel(JhArgs g) {
  __shared__ double s_e[JH_MAXB];
  const int tid = threadIdx.x, i = blockIdx.x * DT_TILE + tid, col = blockIdx.y;
  const bool is_z = col < g.l;
  const int k = is_z ? col : col - g.l;
  if (tid < g.bins) s_e[tid] = (is_z ? g.edges_z : g.edges_a)[k * g.bins + tid];
  __syncthreads();
  if (i >= g.n) return;
  const double x = (double)(is_z ? g.zt[k * g.ldz + i] : g.attrs[k * g.lda + i]);
  int cnt = 0;
  for (int e = 0; e < g.bins; ++e) cnt += s_e[e] <= x ? 1 : 0;
  (is_z ? g.bins_z : g.bins_a)[(long long)k * g.n + i] = (unsigned char)(cnt > 0 ? cnt - 1 : JH_NOBIN);
}

__global__ __launch_bounds__(DT_TILE) void joint_histogram_count_kernel(JhArgs g) {
  __shared__ int s_cnt[JH_QB * JH_MAXB * JH_MAXB];
  const int tid = threadIdx.x, chunk = blockIdx.x, c = blockIdx.y, q0 = blockIdx.z * JH_QB;
  const int nb = g.bins, bb = nb * nb, nq = min(JH_QB, g.na - q0);
  for (int e = tid; e < nq * bb; e += DT_TILE) s_cnt[e] = 0;
  __syncthreads();
  const int i_end = min(g.n, (chunk + 1) * JH_ROWS);
  const unsigned char* __restrict__ bz = g.bins_z + (long long)c * g.n;
  for (int i = chunk * JH_ROWS + tid; i < i_end; i += DT_TILE) {
    const int z = bz[i];
    if (z >= nb) continue;
    for (int k = 0; k < nq; ++k) {
      const int a = g.bins_a[(long long)(q0 + k) * g.n + i];
      if (a < nb) atomicAdd(&s_cnt[k * bb + a * nb + z], 1);   // an LDS integer add; the index is below nq * bb
    }
  }
  __syncthreads();
  for (int e = tid; e < nq * bb; e += DT_TILE) {
    const int k = e / bb, r = e - k * bb;
    g.ws[(((long long)chunk * g.na + q0 + k) * g.l + c) * bb + r] = s_cnt[e];
  }
}

__global__ __launch_bounds__(DT_TILE) void joint_histogram_fold_kernel(JhArgs g) {
  const long long total = (long long)g.na * g.l * g.bins * g.bins, e = (long long)blockIdx.x * DT_TILE + threadIdx.x;
  if (e >= total) return;
  int t = 0;
  for (int r = 0; r < g.chunks; ++r) t += g.ws[r * total + e];
  g.counts[e] = t;
}

bool jh_supported(int n, int l, int na, int bins) {
  return n >= 2 && n <= DT_MAXN && l >= 1 && l <= JH_MAXL && na >= 1 && na <= JH_MAXNA && bins >= 2 && bins <= JH_MAXB;
}

}  // namespace

extern "C" int pti_tied_ranks(const float* cols, int64_t ld, int n, int m, int32_t* rank2, pti_stream_t s) {
  if (!cols || !rank2) PTI_FAIL(PTI_EINVAL, "tied_ranks: null pointer");
  if (n < 2 || m < 1) PTI_FAIL(PTI_EINVAL, "tied_ranks: bad shape n=%d m=%d (n >= 2, m >= 1)", n, m);
  if (n > DT_MAXN || m > DT_MAXCOLS)
    PTI_FAIL(PTI_EUNSUPPORTED, "tied_ranks: unsupported shape n=%d m=%d (n <= %d, m <= %d)", n, m, DT_MAXN, DT_MAXCOLS);
  if (ld < n) PTI_FAIL(PTI_EINVAL, "tied_ranks: row stride below n (ld=%lld n=%d)", (long long)ld, n);
  if (((uintptr_t)cols & 3) || ((uintptr_t)rank2 & 3)) PTI_FAIL(PTI_EINVAL, "tied_ranks: misaligned buffer");
  PTI_LAUNCH(tied_ranks_kernel, dim3((unsigned)cdiv(n, DT_TILE), (unsigned)m), dim3(DT_TILE), 0, (hipStream_t)s, cols,
             (long long)ld, n, (int*)rank2);
  PTI_CHECK_LAUNCH("tied_ranks");
  return PTI_OK;
}

extern "C" int pti_rank_moments(const int32_t* rank2, int n, int m, int64_t* sums, int64_t* gram, pti_stream_t s) {
  if (!rank2 || !sums || !gram) PTI_FAIL(PTI_EINVAL, "rank_moments: null pointer");
  if (n < 2 || m < 1) PTI_FAIL(PTI_EINVAL, "rank_moments: bad shape n=%d m=%d (n >= 2, m >= 1)", n, m);
  if (n > DT_MAXN || m > DT_MAXCOLS)
    PTI_FAIL(PTI_EUNSUPPORTED, "rank_moments: unsupported shape n=%d m=%d (n <= %d, m <= %d)", n, m, DT_MAXN, DT_MAXCOLS);
  if (((uintptr_t)rank2 & 3) || ((uintptr_t)sums & 7) || ((uintptr_t)gram & 7))
    PTI_FAIL(PTI_EINVAL, "rank_moments: misaligned buffer");
  PTI_LAUNCH(rank_moments_kernel, dim3((unsigned)m, (unsigned)m), dim3(DT_TILE), 0, (hipStream_t)s, (const int*)rank2, n, m,
             (long long*)sums, (long long*)gram);
  PTI_CHECK_LAUNCH("rank_moments");
  return PTI_OK;
}

extern "C" int64_t pti_joint_histogram_ws_bytes(int n, int l, int na, int bins) {
  if (!jh_supported(n, l, na, bins)) return 0;
  return (int64_t)cdiv(n, JH_ROWS) * na * l * bins * bins * (int64_t)sizeof(int);
}

extern "C" int pti_joint_histogram(const float* zt, int64_t ldz, const float* attrs, int64_t lda, int n, int l, int na,
                                   int bins, const double* edges_z, const double* edges_a, uint8_t* bins_z,
                                   uint8_t* bins_a, int32_t* counts, void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!zt || !attrs || !edges_z || !edges_a || !bins_z || !bins_a || !counts || !workspace)
    PTI_FAIL(PTI_EINVAL, "joint_histogram: null pointer");
  if (n < 2 || l < 1 || na < 1 || bins < 2)
    PTI_FAIL(PTI_EINVAL, "joint_histogram: bad shape n=%d l=%d na=%d bins=%d (n, bins >= 2, l, na >= 1)", n, l, na, bins);
  if (!jh_supported(n, l, na, bins))
    PTI_FAIL(PTI_EUNSUPPORTED, "joint_histogram: unsupported shape n=%d l=%d na=%d bins=%d (n <= %d, l <= %d, na <= %d, bins <= %d)",
             n, l, na, bins, DT_MAXN, JH_MAXL, JH_MAXNA, JH_MAXB);
  if (ldz < n || lda < n)
    PTI_FAIL(PTI_EINVAL, "joint_histogram: row stride below n (ldz=%lld lda=%lld n=%d)", (long long)ldz, (long long)lda, n);
  if (((uintptr_t)zt & 3) || ((uintptr_t)attrs & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)edges_z & 7) ||
      ((uintptr_t)edges_a & 7))
    PTI_FAIL(PTI_EINVAL, "joint_histogram: misaligned buffer");
  if ((uintptr_t)workspace & 3) PTI_FAIL(PTI_EINVAL, "joint_histogram: workspace must be 4-byte aligned");
  if (ws_bytes < pti_joint_histogram_ws_bytes(n, l, na, bins))
    PTI_FAIL(PTI_EINVAL, "joint_histogram: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
             (long long)pti_joint_histogram_ws_bytes(n, l, na, bins));
  JhArgs g;
  g.zt = zt;
  g.attrs = attrs;
  g.ldz = ldz;
  g.lda = lda;
  g.n = n;
  g.l = l;
  g.na = na;
  g.bins = bins;
  g.chunks = cdiv(n, JH_ROWS);
  g.edges_z = edges_z;
  g.edges_a = edges_a;
  g.bins_z = bins_z;
  g.bins_a = bins_a;
  g.ws = (int*)workspace;
  g.counts = (int*)counts;
  PTI_LAUNCH(joint_histogram_bin_kernel, dim3((unsigned)cdiv(n, DT_TILE), (unsigned)(l + na)), dim3(DT_TILE), 0,
             (hipStream_t)s, g);
  PTI_CHECK_LAUNCH("joint_histogram (bins)");
  PTI_LAUNCH(joint_histogram_count_kernel, dim3((unsigned)g.chunks, (unsigned)l, (unsigned)cdiv(na, JH_QB)), dim3(DT_TILE),
             0, (hipStream_t)s, g);
  PTI_CHECK_LAUNCH("joint_histogram (counts)");
  PTI_LAUNCH(joint_histogram_fold_kernel, dim3((unsigned)cdiv(na * l * bins * bins, DT_TILE)), dim3(DT_TILE), 0,
             (hipStream_t)s, g);
  PTI_CHECK_LAUNCH("joint_histogram (fold)");
  return PTI_OK;
}
