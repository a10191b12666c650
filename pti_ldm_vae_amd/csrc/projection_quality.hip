// Rank counts and per-label distance sums over an n x n fp32 distance matrix on the device (gfx950): the two passes under the
// projection-quality report of the latent-space analysis (trustworthiness, continuity, neighbourhood preservation, kNN label
// agreement, silhouette).  3 <= n <= 8192.  DESIGN.md 5r.
//
//   pti_neighbor_ranks, one launch: one 256-thread workgroup per row i.  The row's fp32 words (neighbor_order_bits, pti_common.h) are staged
//     once in LDS, padded to a multiple of four with all-ones words (32 KB at n = 8192, so four workgroups share a compute unit).
//     The four waves take the m listed neighbours round-robin; for neighbour j a lane reads four consecutive words per step
//     (one 16-byte LDS read, lane-contiguous: conflict-free) and counts the columns l with key(i, l) < key(i, j), where key is
//     pti_umap_knn's 64-bit key, the word above the column: word_l < word_j, or equal words and l < j.  A padding word is all
//     ones and its column is >= n > j: never counted.  The lanes' counts are folded by wave_sum; the row's own column is taken
//     out afterwards (one compare), so the inner loop carries no test for it.  Integers only: exact, no order of evaluation.
//   pti_segment_row_sums, one launch: one 256-thread workgroup per row i, the waves taking the G segments round-robin.  Lane
//     t of the wave that owns segment g adds the entries at seg[g] + t + 64 q, converted to fp64 as they are loaded, into
//     accumulator q mod 4, q ascending; the four are added as (a0 + a1) + (a2 + a3) and the lanes are folded by the xor
//     butterfly 32, 16, ... 1.  Which entries meet in which add depends on the segment's length alone, so the bits of out[i][g]
//     depend on row i and that segment: not on n, G, the segment's position or the launch.  fp-reassociation is switched off
//     for these sums (the library is built with -ffast-math).  The table is read defensively: offsets are clamped to [0, n] and
//     a segment that does not ascend is empty, so nothing outside the row is read whatever the table holds.
//   pti_projection_distances, one launch: the distance matrix of the PROJECTION's rows (at most 8 coordinates), one thread
//     per entry.  The differences, their squares, the sum and the root are taken in fp64 and the result is rounded to fp32
//     once, so an entry is the fp32 nearest the true distance (up to the last bits of the fp64 root) and two entries of a row
//     are ordered as the true distances are unless they round to the same fp32 -- then the lower column goes first.  The
//     fp32 accumulation of pti_latent_pairwise (a few units in the last place) orders distances closer than that by its
//     rounding; for a picture's two coordinates the exact route costs nothing.  Symmetric bit for bit, zero diagonal.
// No atomics, no workspace, caller's stream, no host synchronisation; bitwise reproducible.
#include "pti_common.h"

namespace {

constexpr int PQ_MIN_N = 3;
constexpr int PQ_MAX_N = 8192;
constexpr int PQ_MAX_M = 256;
constexpr int PQ_MAX_G = 2048;
constexpr int PQ_MAX_COLS = 8;
constexpr int PQ_THREADS = 256;
constexpr int PQ_WAVES = PQ_THREADS / 64;

__global__ __launch_bounds__(PQ_THREADS) void neighbor_ranks_kernel(const float* __restrict__ dist, long long ldd, int n, int m,
                                                                    const int* __restrict__ nbr_idx, int* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t pq_word[];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int np4 = (n + 3) & ~3;
  const float* __restrict__ row = dist + (long long)i * ldd;
  for (int l = tid; l < np4; l += PQ_THREADS) {
    uint32_t bits = 0xffffffffu;                         // padding: never below a key of a real column
    if (l < n) bits = neighbor_order_bits(row[l]);
    pq_word[l] = bits;
  }
  __syncthreads();
  const uint32_t wi = pq_word[i];
  for (int c = wave; c < m; c += PQ_WAVES) {             // wave-uniform
    const int j = nbr_idx[(long long)i * m + c];
    int result;
    if (j < 0 || j >= n) {
      result = -1;                                       // not dereferenced
    } else if (j == i) {
      result = 0;
    } else {
      const uint32_t wj = pq_word[j];
      // one two-part test per word.  Splitting the row at j into "word <= word_j" steps, the one step that holds j and
      // "word < word_j" steps (a wave-uniform choice) was measured and is SLOWER: 344 against 271 us at n = 6000, m = 40
      int cnt = 0;
      for (int l = 4 * lane; l < np4; l += 4 * 64) {
        const u32x4 w = *(const u32x4*)&pq_word[l];
#pragma unroll
        for (int u = 0; u < 4; ++u) cnt += (w[u] < wj || (w[u] == wj && l + u < j)) ? 1 : 0;
      }
      cnt = wave_sum(cnt);
      cnt -= (wi < wj || (wi == wj && i < j)) ? 1 : 0;   // the row's own column takes no part
      result = 1 + cnt;
    }
    if (lane == 0) out[(long long)i * m + c] = result;
  }
}

__global__ __launch_bounds__(PQ_THREADS) void segment_row_sums_kernel(const float* __restrict__ dist, long long ldd, int n,
                                                                      const int* __restrict__ seg, int groups,
                                                                      double* __restrict__ out) {
#pragma clang fp reassociate(off)
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ row = dist + (long long)i * ldd;
  for (int g = wave; g < groups; g += PQ_WAVES) {        // wave-uniform
    const int lo = min(max(seg[g], 0), n), hi = min(max(seg[g + 1], 0), n);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = lo + lane;
    for (; j + 192 < hi; j += 256) {
      a0 += (double)row[j];
      a1 += (double)row[j + 64];
      a2 += (double)row[j + 128];
      a3 += (double)row[j + 192];
    }
    if (j < hi) a0 += (double)row[j];
    if (j + 64 < hi) a1 += (double)row[j + 64];
    if (j + 128 < hi) a2 += (double)row[j + 128];
    double s = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    if (lane == 0) out[(long long)i * groups + g] = s;
  }
}

// one 256-thread workgroup per (row i, block of 256 columns); a point has at most PQ_MAX_COLS coordinates
__global__ __launch_bounds__(PQ_THREADS) void projection_distances_kernel(const float* __restrict__ y, long long ldy, int n,
                                                                          int d, float* __restrict__ out, long long ldo) {
#pragma clang fp reassociate(off)
  const int i = blockIdx.y, j = blockIdx.x * PQ_THREADS + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
  for (int k = 0; k < d; ++k) {                          // ascending k on both sides of the diagonal: symmetric bit for bit
    const double t = (double)y[(long long)i * ldy + k] - (double)y[(long long)j * ldy + k];
    s += t * t;
  }
  out[(long long)i * ldo + j] = (float)sqrt(s);
}

}  // namespace

extern "C" int pti_projection_distances(const float* y, int64_t ldy, int n, int d, float* out, int64_t ldo, pti_stream_t s) {
  if (!y || !out) PTI_FAIL(PTI_EINVAL, "projection_distances: null pointer");
  if (n < 1 || d < 1) PTI_FAIL(PTI_EINVAL, "projection_distances: bad dimension n=%d d=%d (at least 1 row and 1 column)", n, d);
  if (n > PQ_MAX_N || d > PQ_MAX_COLS)
    PTI_FAIL(PTI_EUNSUPPORTED, "projection_distances: unsupported shape n=%d d=%d (at most %d rows, %d columns)", n, d, PQ_MAX_N,
             PQ_MAX_COLS);
  if (ldy < d || ldo < n)
    PTI_FAIL(PTI_EINVAL, "projection_distances: row stride below the row length (ldy=%lld d=%d ldo=%lld n=%d)", (long long)ldy, d,
             (long long)ldo, n);
  if (((uintptr_t)y & 3) || ((uintptr_t)out & 3)) PTI_FAIL(PTI_EINVAL, "projection_distances: misaligned buffer");
  PTI_LAUNCH(projection_distances_kernel, dim3((unsigned)cdiv(n, PQ_THREADS), (unsigned)n), dim3(PQ_THREADS), 0, (hipStream_t)s, y,
             (long long)ldy, n, d, out, (long long)ldo);
  PTI_CHECK_LAUNCH("projection_distances");
  return PTI_OK;
}

extern "C" int pti_neighbor_ranks(const float* dist, int64_t ldd, int n, const int32_t* nbr_idx, int m, int32_t* out,
                                  pti_stream_t s) {
  if (!dist || !nbr_idx || !out) PTI_FAIL(PTI_EINVAL, "neighbor_ranks: null pointer");
  if (n < PQ_MIN_N) PTI_FAIL(PTI_EINVAL, "neighbor_ranks: bad dimension n=%d (at least %d rows)", n, PQ_MIN_N);
  if (m < 1) PTI_FAIL(PTI_EINVAL, "neighbor_ranks: bad dimension m=%d (at least 1 listed neighbour)", m);
  if (n > PQ_MAX_N || m > PQ_MAX_M)
    PTI_FAIL(PTI_EUNSUPPORTED, "neighbor_ranks: unsupported shape n=%d m=%d (at most %d rows, %d listed neighbours)", n, m,
             PQ_MAX_N, PQ_MAX_M);
  if (ldd < n) PTI_FAIL(PTI_EINVAL, "neighbor_ranks: row stride below the row length (ldd=%lld n=%d)", (long long)ldd, n);
  if (((uintptr_t)dist & 3) || ((uintptr_t)nbr_idx & 3) || ((uintptr_t)out & 3))
    PTI_FAIL(PTI_EINVAL, "neighbor_ranks: misaligned buffer");
  const size_t lds = (size_t)((n + 3) & ~3) * sizeof(uint32_t);   // at most 32 KB
  PTI_LAUNCH(neighbor_ranks_kernel, dim3((unsigned)n), dim3(PQ_THREADS), lds, (hipStream_t)s, dist, (long long)ldd, n, m,
             (const int*)nbr_idx, (int*)out);
  PTI_CHECK_LAUNCH("neighbor_ranks");
  return PTI_OK;
}

extern "C" int pti_segment_row_sums(const float* dist, int64_t ldd, int n, const int32_t* seg, int groups, double* out,
                                    pti_stream_t s) {
  if (!dist || !seg || !out) PTI_FAIL(PTI_EINVAL, "segment_row_sums: null pointer");
  if (n < PQ_MIN_N) PTI_FAIL(PTI_EINVAL, "segment_row_sums: bad dimension n=%d (at least %d rows)", n, PQ_MIN_N);
  if (groups < 1) PTI_FAIL(PTI_EINVAL, "segment_row_sums: bad dimension groups=%d (at least 1 segment)", groups);
  if (n > PQ_MAX_N || groups > PQ_MAX_G)
    PTI_FAIL(PTI_EUNSUPPORTED, "segment_row_sums: unsupported shape n=%d groups=%d (at most %d rows, %d segments)", n, groups,
             PQ_MAX_N, PQ_MAX_G);
  if (ldd < n) PTI_FAIL(PTI_EINVAL, "segment_row_sums: row stride below the row length (ldd=%lld n=%d)", (long long)ldd, n);
  if (((uintptr_t)dist & 3) || ((uintptr_t)seg & 3) || ((uintptr_t)out & 7))
    PTI_FAIL(PTI_EINVAL, "segment_row_sums: misaligned buffer");
  PTI_LAUNCH(segment_row_sums_kernel, dim3((unsigned)n), dim3(PQ_THREADS), 0, (hipStream_t)s, dist, (long long)ldd, n,
             (const int*)seg, groups, out);
  PTI_CHECK_LAUNCH("segment_row_sums");
  return PTI_OK;
}
