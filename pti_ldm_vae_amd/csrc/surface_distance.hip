// Surface distances between two binary regions of an image (gfx950): per image and side the number of foreground and edge
// pixels, the largest squared distance from an edge pixel to the other side's edge, two order statistics of those squared
// distances (a percentile is interpolated between them on the host), how many lie within up to four tolerances, and the fp64 sum
// of the distances -- what Hausdorff, HD95, the average symmetric surface distance and surface Dice are formed from.  The
// definitions are in include/pti_vae.h ("surface distance"); DESIGN.md 5q-4 has the measurements.
//
// An exact Euclidean distance transform in two separable steps (columns, then rows), evaluated only where it is asked for:
//   launch 1 (surface_columns_kernel): grid (column tiles, n * 2), one thread per column of one (image, side).  It walks its
//     column down, forms the edge flag of every pixel from the three rows in flight (a foreground pixel with a 4-neighbour that
//     is background or outside the image) and writes g = the vertical distance to the nearest edge pixel ABOVE in the column
//     (uint16, 0xFFFF = none), then walks back up and lowers g by the distance to the nearest one BELOW.  Consecutive threads
//     take consecutive columns, so every load and store of a row is coalesced; the walk loads SD_WALK rows at a time.  The column's foreground and edge counts go to the
//     workspace as plain words; the tile-0 workgroup of an (image, side) zeroes that side's histogram and counters.
//   launch 2 (surface_rows_kernel): grid (h, n * 2), one wave per (image, side, row).  The OTHER side's g row is staged in LDS;
//     every edge pixel x of this side scans outwards, best = min(best, dx^2 + g[x -+ dx]^2), and stops once dx^2 >= best or both
//     ends left the row: at most w steps, and no column further away can hold a nearer pixel.  d^2 goes to an int32 map (-1 off
//     the edge); the row's maximum, its counts within the tolerances and a 2048-bin histogram of d^2 >> 10 are folded with
//     integer atomics (any order gives the same words); the row's fp64 sum of sqrt(d^2) -- lane: its pixels left to right, then
//     the xor butterfly -- is stored per row.
//   launch 3 (surface_select_kernel): grid (n * 2), one workgroup of 1024 threads per (image, side).  It adds the column counts,
//     finds by a prefix scan the coarse bins that hold rank_lo and rank_hi, makes one pass over the d^2 map with a 1024-bin LDS
//     histogram of the low ten bits for each of the two bins, scans those for the two order statistics, adds the row sums in
//     row order and writes the outputs.
// No floating-point atomics, no loop without a bound, and every word of the workspace that is read was written earlier in the
// same call: the outputs are bitwise reproducible and an image's rows do not depend on n or on its place in the batch.
#include <limits.h>

#include "pti_common.h"

namespace {

constexpr int SD_MAX_EDGE = PTI_MASK_COMPARE_MAX_EDGE;
constexpr int SD_COLS = PTI_SURFACE_COLUMNS;
constexpr int SD_MAX_TOL = PTI_SURFACE_MAX_TOLERANCES;
constexpr int SD_COL_THREADS = 64;       // one wave per 64 columns: small images still fill many compute units
constexpr int SD_WALK = 8;                 // rows per step of the column walk
constexpr int SD_SEL_THREADS = 1024;
constexpr int SD_SEL_WAVES = SD_SEL_THREADS / 64;
constexpr int SD_COARSE = 2048;            // bins of d^2 >> 10: d^2 <= 2 * 1023^2 = 2093058 < 2048 * 1024
constexpr int SD_FINE = 1024;              // bins of d^2 & 1023
constexpr int SD_CTR = 8;                  // per (image, side) behind the histogram: max d^2, within[4], 3 spare words
constexpr unsigned SD_NONE = 0xFFFFu;      // g: no edge pixel in this column

struct SdArgs {
  const unsigned char* m[2];   // [n][h][w] per side (may be one buffer)
  int bits[2];                 // a pixel is foreground on side s when m[s][p] & bits[s]
  double* rowsum;              // [n * 2][h]
  int* d2map;                  // [n * 2][h][w]
  int* hist;                   // [n * 2][SD_COARSE + SD_CTR]
  int* colcnt;                 // [n * 2][2][w]: foreground pixels, edge pixels of a column
  unsigned short* g;           // [n * 2][h][w]
  int* counts;                 // [n][2][SD_COLS]
  double* sums;                // [n][2]
  int tol[SD_MAX_TOL];
  int h, w, n_tol, pm;
};

__global__ __launch_bounds__(SD_COL_THREADS) void surface_columns_kernel(SdArgs a) {
  const int ps = blockIdx.y, side = ps & 1, img = ps >> 1;
  const int h = a.h, w = a.w;
  if (blockIdx.x == 0) {
    int* hs = a.hist + (size_t)ps * (SD_COARSE + SD_CTR);
    for (int i = threadIdx.x; i < SD_COARSE + SD_CTR; i += SD_COL_THREADS) hs[i] = 0;
  }
  const int x = blockIdx.x * SD_COL_THREADS + threadIdx.x;
  if (x >= w) return;
  const unsigned char* __restrict__ m = a.m[side] + (size_t)img * h * w;
  const int bits = a.bits[side];
  unsigned short* __restrict__ g = a.g + (size_t)ps * h * w;
  // The walk is bound by the latency of its loads, so it goes in steps of SD_WALK rows: all loads of a step first, at
  // clamped (always valid) addresses and without a branch, then the arithmetic and the stores.
  const bool has_l = x > 0, has_r = x < w - 1;
  const int xl = has_l ? x - 1 : x, xr = has_r ? x + 1 : x;
  int nfg = 0, nedge = 0;
  unsigned dist = SD_NONE;
  bool up = false, cur = (m[x] & bits) != 0;
  for (int y0 = 0; y0 < h; y0 += SD_WALK) {
    unsigned char vl[SD_WALK], vr[SD_WALK], vd[SD_WALK];
#pragma unroll
    for (int k = 0; k < SD_WALK; ++k) {
      const int y = min(y0 + k, h - 1), yd = min(y0 + k + 1, h - 1);
      vl[k] = m[(size_t)y * w + xl];
      vr[k] = m[(size_t)y * w + xr];
      vd[k] = m[(size_t)yd * w + x];
    }
#pragma unroll
    for (int k = 0; k < SD_WALK; ++k) {
      const int y = y0 + k;
      if (y < h) {
        const bool l = has_l & ((vl[k] & bits) != 0), r = has_r & ((vr[k] & bits) != 0);
        const bool down = (y + 1 < h) & ((vd[k] & bits) != 0);
        const bool edge = cur & !(up & down & l & r);
        nfg += cur;
        nedge += edge;
        dist = edge ? 0u : (dist == SD_NONE ? SD_NONE : dist + 1u);   // at most h - 1 < 0xFFFF
        g[(size_t)y * w + x] = (unsigned short)dist;
        up = cur;
        cur = down;
      }
    }
  }
  dist = SD_NONE;
  for (int y0 = h - 1; y0 >= 0; y0 -= SD_WALK) {   // this thread's own stores of the sweep above
    unsigned above[SD_WALK];
#pragma unroll
    for (int k = 0; k < SD_WALK; ++k) above[k] = g[(size_t)max(y0 - k, 0) * w + x];
#pragma unroll
    for (int k = 0; k < SD_WALK; ++k) {
      const int y = y0 - k;
      if (y >= 0) {
        dist = above[k] == 0u ? 0u : (dist == SD_NONE ? SD_NONE : dist + 1u);
        if (dist < above[k]) g[(size_t)y * w + x] = (unsigned short)dist;
      }
    }
  }
  int* cc = a.colcnt + (size_t)ps * 2 * w;
  cc[x] = nfg;
  cc[w + x] = nedge;
}

__global__ __launch_bounds__(64) void surface_rows_kernel(SdArgs a) {
#pragma clang fp reassociate(off)
  __shared__ unsigned short gs[SD_MAX_EDGE];
  const int y = blockIdx.x, ps = blockIdx.y, lane = threadIdx.x;
  const int h = a.h, w = a.w;
  const unsigned short* own = a.g + ((size_t)ps * h + y) * w;
  const unsigned short* oth = a.g + ((size_t)(ps ^ 1) * h + y) * w;
  int* out = a.d2map + ((size_t)ps * h + y) * w;
  for (int x = lane; x < w; x += 64) gs[x] = oth[x];
  __syncthreads();

  int mx = -1, within[SD_MAX_TOL] = {0, 0, 0, 0};
  double sum = 0.0;
  int* hs = a.hist + (size_t)ps * (SD_COARSE + SD_CTR);
  for (int x = lane; x < w; x += 64) {
    int d2 = -1;
    if (own[x] == 0) {
      int best = INT_MAX;
      for (int dx = 0; dx < w; ++dx) {
        const int dx2 = dx * dx, xl = x - dx, xr = x + dx;
        if (dx2 >= best || (xl < 0 && xr >= w)) break;
        if (xl >= 0) {
          const int gv = gs[xl];
          if (gv != (int)SD_NONE) best = min(best, dx2 + gv * gv);
        }
        if (xr < w) {
          const int gv = gs[xr];
          if (gv != (int)SD_NONE) best = min(best, dx2 + gv * gv);
        }
      }
      if (best != INT_MAX) {   // INT_MAX: the other side has no edge pixel at all; launch 3 reports the empty side
        d2 = best;
        mx = max(mx, d2);
#pragma unroll
        for (int j = 0; j < SD_MAX_TOL; ++j) within[j] += (j < a.n_tol && d2 <= a.tol[j]) ? 1 : 0;
        sum += __dsqrt_rn((double)d2);
        atomicAdd(hs + (d2 >> 10), 1);
      }
    }
    out[x] = d2;
  }
  mx = wave_max(mx);
#pragma unroll
  for (int j = 0; j < SD_MAX_TOL; ++j) within[j] = wave_sum(within[j]);
  sum = wave_sum(sum);
  if (lane == 0) {
    if (mx >= 0) atomicMax(hs + SD_COARSE, mx);
#pragma unroll
    for (int j = 0; j < SD_MAX_TOL; ++j)
      if (within[j]) atomicAdd(hs + SD_COARSE + 1 + j, within[j]);
    a.rowsum[(size_t)ps * h + y] = sum;
  }
}

// The bin of `cnt` (one per thread, bins in thread order) that holds rank k, counted from 0, and the number of entries in the
// bins before it: written by the one thread whose bin it is.  `part` holds one word per wave.
__device__ __forceinline__ void sd_find(int cnt, int k, int* part, int* bin, int* before) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  __syncthreads();   // `part` may still be read from an earlier call
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int v = 0; v < wave; ++v) base += part[v];
  const int excl = base + incl - cnt;
  if (k >= excl && k < excl + cnt) { *bin = tid; *before = excl; }
}

__global__ __launch_bounds__(SD_SEL_THREADS) void surface_select_kernel(SdArgs a) {
#pragma clang fp reassociate(off)
  __shared__ int fine[2][SD_FINE];
  __shared__ int part[SD_SEL_WAVES];
  __shared__ int tot[3];         // foreground and edge pixels of this side, edge pixels of the other
  __shared__ int sel[2][2];      // per rank: bin, entries before it
  const int ps = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int h = a.h, w = a.w;
  int* out = a.counts + (size_t)ps * SD_COLS;
  const int* hs = a.hist + (size_t)ps * (SD_COARSE + SD_CTR);

  if (tid < 3) tot[tid] = 0;
  __syncthreads();
  {
    const int* cc = a.colcnt + (size_t)ps * 2 * w;
    const int* co = a.colcnt + (size_t)(ps ^ 1) * 2 * w;
    int nfg = 0, nedge = 0, nother = 0;
    for (int x = tid; x < w; x += SD_SEL_THREADS) { nfg += cc[x]; nedge += cc[w + x]; nother += co[w + x]; }
    nfg = wave_sum(nfg); nedge = wave_sum(nedge); nother = wave_sum(nother);
    if (lane == 0) { atomicAdd(&tot[0], nfg); atomicAdd(&tot[1], nedge); atomicAdd(&tot[2], nother); }
  }
  __syncthreads();
  const int nfg = tot[0], m = tot[1];
  if (m == 0 || tot[2] == 0) {   // an empty side: nothing to measure on either side of this image
    if (tid == 0) {
      out[0] = nfg; out[1] = m; out[2] = -1; out[3] = 0; out[4] = -1; out[5] = -1;
      for (int j = 0; j < SD_MAX_TOL; ++j) out[6 + j] = 0;
      out[SD_COLS - 1] = 0;
      a.sums[ps] = 0.0;
    }
    return;
  }
  const long long r = (long long)(m - 1) * a.pm;
  const int rank[2] = {(int)(r / 1000), (int)(r / 1000) + (r % 1000 != 0 ? 1 : 0)};   // rank[1] <= m - 1

  // ---- the coarse bins of the two ranks: 2048 bins, two per thread ----
  if (tid < 4) sel[tid >> 1][tid & 1] = -1;
  const int c0 = hs[2 * tid], c1 = hs[2 * tid + 1];
  int cbin[2], cbefore[2];
  for (int k = 0; k < 2; ++k) {
    sd_find(c0 + c1, rank[k], part, &sel[k][0], &sel[k][1]);
    __syncthreads();
    const int t = sel[k][0];
    cbin[k] = -1; cbefore[k] = 0;
    if (t >= 0) {   // the pair of bins 2 t, 2 t + 1: which of the two
      const int first = hs[2 * t], left = rank[k] - sel[k][1];
      cbin[k] = left < first ? 2 * t : 2 * t + 1;
      cbefore[k] = sel[k][1] + (left < first ? 0 : first);
    }
  }
  __syncthreads();

  // ---- one pass over the d^2 map: the low ten bits of what falls into those bins ----
  fine[0][tid] = 0;
  fine[1][tid] = 0;
  if (tid < 4) sel[tid >> 1][tid & 1] = -1;
  __syncthreads();
  const int* map = a.d2map + (size_t)ps * h * w;
  const int npix = h * w;
  for (int p = tid; p < npix; p += SD_SEL_THREADS) {
    const int v = map[p];
    if (v < 0) continue;
    if ((v >> 10) == cbin[0]) atomicAdd(&fine[0][v & (SD_FINE - 1)], 1);
    if ((v >> 10) == cbin[1]) atomicAdd(&fine[1][v & (SD_FINE - 1)], 1);
  }
  __syncthreads();
  for (int k = 0; k < 2; ++k) sd_find(fine[k][tid], rank[k] - cbefore[k], part, &sel[k][0], &sel[k][1]);
  __syncthreads();
  if (tid != 0) return;
  const bool ok = cbin[0] >= 0 && cbin[1] >= 0 && sel[0][0] >= 0 && sel[1][0] >= 0;   // else the histograms disagree with the counts
  const double* rs = a.rowsum + (size_t)ps * h;
  double s = rs[0];
  for (int y = 1; y < h; ++y) s += rs[y];
  out[0] = nfg; out[1] = m; out[2] = ok ? hs[SD_COARSE] : -1; out[3] = rank[0];
  out[4] = ok ? (cbin[0] << 10) | sel[0][0] : -1;
  out[5] = ok ? (cbin[1] << 10) | sel[1][0] : -1;
  for (int j = 0; j < SD_MAX_TOL; ++j) out[6 + j] = ok ? hs[SD_COARSE + 1 + j] : 0;
  out[SD_COLS - 1] = ok ? 0 : 1;
  a.sums[ps] = ok ? s : 0.0;
}

inline bool sd_shape_ok(int n, int h, int w) { return n >= 1 && n <= 32767 && h >= 1 && w >= 1 && h <= SD_MAX_EDGE && w <= SD_MAX_EDGE; }

// byte offsets of the five regions; the total is the workspace size
struct SdLayout { int64_t rowsum, d2map, hist, colcnt, g, total; };
inline SdLayout sd_layout(int n, int h, int w) {
  const int64_t p = 2 * (int64_t)n, npix = (int64_t)h * w;
  SdLayout l;
  l.rowsum = 0;
  l.d2map = l.rowsum + p * h * (int64_t)sizeof(double);
  l.hist = l.d2map + p * npix * (int64_t)sizeof(int);
  l.colcnt = l.hist + p * (SD_COARSE + SD_CTR) * (int64_t)sizeof(int);
  l.g = l.colcnt + p * 2 * w * (int64_t)sizeof(int);
  l.total = ((l.g + p * npix * (int64_t)sizeof(unsigned short) + 7) / 8) * 8;
  return l;
}

}  // namespace

extern "C" int64_t pti_surface_distance_ws_bytes(int n, int h, int w) {
  if (!sd_shape_ok(n, h, w)) return 0;
  return sd_layout(n, h, w).total;
}

extern "C" int pti_surface_distance(const uint8_t* a, int a_bits, const uint8_t* b, int b_bits, int n, int h, int w,
                                    int percentile_pm, const int32_t* tol_d2, int n_tol, int32_t* counts, double* sums,
                                    void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!a || !b || !counts || !sums || !workspace || (n_tol > 0 && !tol_d2)) PTI_FAIL(PTI_EINVAL, "surface_distance: null pointer");
  if (n < 1 || h < 1 || w < 1) PTI_FAIL(PTI_EINVAL, "surface_distance: bad shape n=%d h=%d w=%d (all >= 1)", n, h, w);
  if (h > SD_MAX_EDGE || w > SD_MAX_EDGE)
    PTI_FAIL(PTI_EUNSUPPORTED, "surface_distance: unsupported shape h=%d w=%d (h, w <= %d)", h, w, SD_MAX_EDGE);
  if (n > 32767) PTI_FAIL(PTI_EUNSUPPORTED, "surface_distance: unsupported batch n=%d (n <= 32767)", n);
  if (a_bits < 1 || a_bits > 255 || b_bits < 1 || b_bits > 255)
    PTI_FAIL(PTI_EINVAL, "surface_distance: bad bit masks %d / %d (1 .. 255)", a_bits, b_bits);
  if (percentile_pm < 0 || percentile_pm > 1000)
    PTI_FAIL(PTI_EINVAL, "surface_distance: percentile of %d per mille (0 .. 1000)", percentile_pm);
  if (n_tol < 0 || n_tol > SD_MAX_TOL) PTI_FAIL(PTI_EINVAL, "surface_distance: %d tolerances (0 .. %d)", n_tol, SD_MAX_TOL);
  for (int j = 0; j < n_tol; ++j)
    if (tol_d2[j] < 0) PTI_FAIL(PTI_EINVAL, "surface_distance: tolerance %d is negative", j);
  if (((uintptr_t)counts & 3) || ((uintptr_t)sums & 7)) PTI_FAIL(PTI_EINVAL, "surface_distance: misaligned buffer");
  if ((uintptr_t)workspace & 7) PTI_FAIL(PTI_EINVAL, "surface_distance: workspace must be 8-byte aligned");
  const SdLayout l = sd_layout(n, h, w);
  if (ws_bytes < l.total)
    PTI_FAIL(PTI_EINVAL, "surface_distance: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)l.total);
  char* ws = (char*)workspace;
  SdArgs k;
  k.m[0] = a; k.m[1] = b;
  k.bits[0] = a_bits; k.bits[1] = b_bits;
  k.rowsum = (double*)(ws + l.rowsum);
  k.d2map = (int*)(ws + l.d2map);
  k.hist = (int*)(ws + l.hist);
  k.colcnt = (int*)(ws + l.colcnt);
  k.g = (unsigned short*)(ws + l.g);
  k.counts = (int*)counts;
  k.sums = sums;
  for (int j = 0; j < SD_MAX_TOL; ++j) k.tol[j] = j < n_tol ? tol_d2[j] : -1;
  k.h = h; k.w = w; k.n_tol = n_tol; k.pm = percentile_pm;
  const hipStream_t st = (hipStream_t)s;
  PTI_LAUNCH(surface_columns_kernel, dim3((unsigned)cdiv(w, SD_COL_THREADS), (unsigned)(2 * n)), dim3(SD_COL_THREADS), 0, st, k);
  PTI_CHECK_LAUNCH("surface_columns");
  PTI_LAUNCH(surface_rows_kernel, dim3((unsigned)h, (unsigned)(2 * n)), dim3(64), 0, st, k);
  PTI_CHECK_LAUNCH("surface_rows");
  PTI_LAUNCH(surface_select_kernel, dim3((unsigned)(2 * n)), dim3(SD_SEL_THREADS), 0, st, k);
  PTI_CHECK_LAUNCH("surface_select");
  return PTI_OK;
}
