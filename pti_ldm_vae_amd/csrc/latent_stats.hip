// Latent-space analysis on the device (gfx950): pairwise Euclidean distances / dot products of two fp32 row sets and the
// per-patient distance statistics of two groups of rows.
//
// Stands in for what the reference's analysis package does on the host with scipy / numpy per patient
// (src/pti_ldm_vae/analysis/latent_space.py:40-66: np.mean, np.std, np.linalg.norm, scipy cdist) and for the Gram matrix
// of its PCA step (latent_space.py:90-102, sklearn PCA on the [N, D] latents), with D = 4 096 .. 40 960 per row.
//
//   pti_latent_pairwise: one 256-thread workgroup per 64x64 output tile.  K-chunks of 16 columns of both operands are
//     staged k-major in LDS (double buffered, 17 KB), every thread keeps a 4x4 register micro-tile and reads its four
//     A rows / four B rows of one k as one 16-byte LDS read each.  mode 0 accumulates (a - b)^2 directly (never the
//     |a|^2 + |b|^2 - 2ab form, which loses 4 digits on latents that share an offset), mode 1 accumulates a * b.
//     The sum over D has ONE order that depends on D only: fmaf chains over 512-column slabs, the slab sums added in
//     ascending order.  A workgroup either walks all slabs itself or -- few tiles, long rows -- handles one slab and
//     stores its partial tile into a workspace that a second launch folds in the same ascending order: both routes give
//     the same bits, so entry (i, j) depends on rows i and j only, not on n1, n2, the tile it falls in or the route.
//   pti_latent_group_stats: rows grouped by patient (segment offsets on the device).  Launch 1: one thread per column
//     and patient computes the two column means, the two-pass population variances and the squared mean difference, the
//     256 columns of a workgroup are reduced in a fixed order.  Launch 2: the pairwise tile routine on the patient's
//     own block of rows, distances summed per tile.  Launch 3: one wavefront per patient folds the partials in a fixed
//     order and writes {centre distance, mean std A, mean std B, mean cross distance}.
// No atomics anywhere; partial results travel through plain vector stores.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int LP_TILE = 64;      // output tile edge
constexpr int LP_KC = 16;        // columns per staged chunk
constexpr int LP_LD = 68;        // LDS row pitch in floats: 16-byte aligned rows, staging stores at most 2-way on a bank
constexpr int LP_SLAB = 512;     // columns per fmaf chain (fixed: the summation order is a function of D only)
constexpr int LP_THREADS = 256;
constexpr int LP_SPLIT_MAX_TILES = 16;           // split D over workgroups only below this many output tiles
constexpr long long LP_SPLIT_MAX_FLOATS = 1LL << 26;
constexpr int LP_MAX_N = 1 << 21, LP_MAX_D = 1 << 24;   // grid y / z stay below 65536
constexpr int GS_COLS = 256;     // columns per workgroup of the per-column pass

struct LpOperands {
  const float* a;
  const float* b;
  const float* center;   // may be null
  long long lda, ldb;
  int na, nb;            // rows available from a / b (rows beyond are staged as zeros)
  int d;
  int vec;               // every pointer 16-byte aligned, both pitches and d multiples of 4
};

// v_sqrt_f32 itself (1 ulp), through the target builtin: under -ffast-math the library sqrt is lowered differently
// from one call site to the next (with or without the correction step), and the one-pass and the folded route must
// agree bit for bit
__device__ __forceinline__ float lp_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

__device__ __forceinline__ int lp_tiles_of(int n) { return (n + LP_TILE - 1) / LP_TILE; }

// four consecutive columns k .. k+3 of `row` of p, minus the centre; zeros for a row >= n or a column >= d
__device__ __forceinline__ f32x4 lp_fetch(const float* __restrict__ p, long long ld, int n, int row, int k,
                                          const float* __restrict__ center, int d, int vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row >= n || k >= d) return v;
  const float* src = p + (long long)row * ld + k;
  if (vec) {
    v = *(const f32x4*)src;
    if (center) v -= *(const f32x4*)(center + k);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (k + c < d) v[c] = center ? src[c] - center[k + c] : src[c];
  }
  return v;
}

// tot[i][j] (+)= sum over the columns of slabs [slab0, slab1) of f(a[row0 + ty*4 + i][k], b[col0 + tx*4 + j][k]);
// f = (a - b)^2 (MODE 0) or a * b (MODE 1).  Every slab is one fmaf chain from 0 in ascending k; the slab sums are added
// to tot in ascending order.  All 256 threads must call it (barriers inside).
template <int MODE>
__device__ __forceinline__ void lp_tile(const LpOperands& o, int row0, int col0, int slab0, int slab1, float* As, float* Bs,
                                        float (&tot)[4][4]) {
#pragma clang fp reassociate(off)
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int lr = tid >> 2, lk = (tid & 3) * 4;           // staging: row lr of the tile, columns lk .. lk+3 of the chunk
  const bool active = (row0 + ty * 4 < o.na) && (col0 + tx * 4 < o.nb);
  const int k_begin = slab0 * LP_SLAB;
  const int k_end = min(o.d, slab1 * LP_SLAB);
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  f32x4 ra = lp_fetch(o.a, o.lda, o.na, row0 + lr, k_begin + lk, o.center, o.d, o.vec);
  f32x4 rb = lp_fetch(o.b, o.ldb, o.nb, col0 + lr, k_begin + lk, o.center, o.d, o.vec);
  int buf = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    As[(lk + c) * LP_LD + lr] = ra[c];
    Bs[(lk + c) * LP_LD + lr] = rb[c];
  }
  __syncthreads();

  for (int kc = k_begin; kc < k_end; kc += LP_KC) {
    const bool has_next = kc + LP_KC < k_end;
    if (has_next) {
      ra = lp_fetch(o.a, o.lda, o.na, row0 + lr, kc + LP_KC + lk, o.center, o.d, o.vec);
      rb = lp_fetch(o.b, o.ldb, o.nb, col0 + lr, kc + LP_KC + lk, o.center, o.d, o.vec);
    }
    if (active) {
      const float* as = As + buf * (LP_KC * LP_LD) + ty * 4;
      const float* bs = Bs + buf * (LP_KC * LP_LD) + tx * 4;
#pragma unroll
      for (int kk = 0; kk < LP_KC; ++kk) {
        const f32x4 a4 = *(const f32x4*)(as + kk * LP_LD);
        const f32x4 b4 = *(const f32x4*)(bs + kk * LP_LD);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (MODE == 0) {
              const float df = a4[i] - b4[j];
              acc[i][j] = fmaf(df, df, acc[i][j]);
            } else {
              acc[i][j] = fmaf(a4[i], b4[j], acc[i][j]);
            }
          }
      }
      // end of a slab (LP_SLAB is a multiple of LP_KC and k_begin a multiple of LP_SLAB) or of the row
      if (((kc + LP_KC) % LP_SLAB) == 0 || !has_next) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            tot[i][j] = tot[i][j] + acc[i][j];
            acc[i][j] = 0.f;
          }
      }
    }
    if (has_next) {
      float* an = As + (buf ^ 1) * (LP_KC * LP_LD);
      float* bn = Bs + (buf ^ 1) * (LP_KC * LP_LD);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        an[(lk + c) * LP_LD + lr] = ra[c];
        bn[(lk + c) * LP_LD + lr] = rb[c];
      }
    }
    __syncthreads();
    buf ^= 1;
  }
}

struct LpArgs {
  LpOperands o;
  float* out;            // [n1][ldo]
  long long ldo;
  float* workspace;      // split: [slabs][n1][n2] partial sums
  int slabs, split;
};

template <int MODE>
__global__ __launch_bounds__(LP_THREADS) void latent_pairwise_tile_kernel(LpArgs p) {
  __shared__ __attribute__((aligned(16))) float As[2 * LP_KC * LP_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2 * LP_KC * LP_LD];
  const int row0 = blockIdx.y * LP_TILE, col0 = blockIdx.x * LP_TILE;
  const int slab0 = p.split ? (int)blockIdx.z : 0;
  const int slab1 = p.split ? slab0 + 1 : p.slabs;
  float tot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) tot[i][j] = 0.f;
  lp_tile<MODE>(p.o, row0, col0, slab0, slab1, As, Bs, tot);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = row0 + ty * 4 + i;
    if (r >= p.o.na) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = col0 + tx * 4 + j;
      if (c >= p.o.nb) continue;
      if (p.split)
        p.workspace[((long long)slab0 * p.o.na + r) * p.o.nb + c] = tot[i][j];
      else
        p.out[(long long)r * p.ldo + c] = MODE == 0 ? lp_sqrt(tot[i][j]) : tot[i][j];
    }
  }
}

// split route: out[r][c] = f(ws[0][r][c] + ws[1][r][c] + ...), the additions in the order lp_tile uses
__global__ __launch_bounds__(256) void latent_pairwise_fold_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                   long long ldo, int n1, int n2, int slabs, int mode) {
#pragma clang fp reassociate(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)n1 * n2;
  if (e >= plane) return;
  float tot = 0.f;
  for (int s = 0; s < slabs; ++s) tot = tot + ws[(long long)s * plane + e];
  const long long r = e / n2, c = e - r * n2;
  out[r * ldo + c] = mode == 0 ? lp_sqrt(tot) : tot;
}

long long lp_tiles(int n1, int n2) { return (long long)cdiv(n1, LP_TILE) * cdiv(n2, LP_TILE); }
bool lp_shape_ok(int n1, int n2, int d) {
  return n1 > 0 && n2 > 0 && d > 0 && n1 <= LP_MAX_N && n2 <= LP_MAX_N && d <= LP_MAX_D;
}
// a function of the shape only: which route is taken never changes a result bit
bool lp_split(int n1, int n2, int d) {
  const long long slabs = cdiv(d, LP_SLAB);
  return slabs > 1 && lp_tiles(n1, n2) <= LP_SPLIT_MAX_TILES && slabs * n1 * n2 <= LP_SPLIT_MAX_FLOATS;
}
long long lp_ws_floats(int n1, int n2, int d) {
  if (!lp_shape_ok(n1, n2, d)) return 0;
  return lp_split(n1, n2, d) ? (long long)cdiv(d, LP_SLAB) * n1 * n2 : 1;   // never 0 for a supported shape
}
int lp_aligned(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

// ---- per-patient statistics ---------------------------------------------------------------------------------------
struct GsArgs {
  LpOperands o;          // a, b: the whole matrices; na / nb: n1 / n2
  const int* seg_a;      // [e + 1] row offsets, ascending
  const int* seg_b;
  double* cols;          // [e][chunks][3]: sums over the chunk's columns of (mean_a - mean_b)^2, std_a, std_b
  double* cross;         // [e][tiles_max]: per-tile sums of distances
  int e, chunks, tiles_max;
};

// rows [lo, lo + cnt) of patient `e`; an offset table that is out of range or not ascending gives cnt = 0 (NaN row)
__device__ __forceinline__ void gs_segment(const int* seg, int e, int n, int& lo, int& cnt) {
  const int s0 = seg[e], s1 = seg[e + 1];
  const bool ok = s0 >= 0 && s1 >= s0 && s1 <= n;
  lo = ok ? s0 : 0;
  cnt = ok ? s1 - s0 : 0;
}

// one column of one side: mean over the rows, then the population std around it (two passes, as np.std)
__device__ __forceinline__ void gs_col_stats(const float* __restrict__ p, long long ld, int lo, int cnt, int col, float& mean,
                                             float& sd) {
#pragma clang fp reassociate(off)
  const float* q = p + (long long)lo * ld + col;
  float s = 0.f;
  for (int r = 0; r < cnt; ++r) s = s + q[(long long)r * ld];
  mean = __fdiv_rn(s, (float)cnt);
  float ss = 0.f;
  for (int r = 0; r < cnt; ++r) {
    const float t = q[(long long)r * ld] - mean;
    ss = fmaf(t, t, ss);
  }
  sd = cnt > 1 ? lp_sqrt(__fdiv_rn(ss, (float)cnt)) : 0.f;
}

__global__ __launch_bounds__(GS_COLS) void latent_group_cols_kernel(GsArgs g) {
  __shared__ double red[GS_COLS / 64];
  const int e = blockIdx.y, chunk = blockIdx.x;
  int lo_a, na, lo_b, nb;
  gs_segment(g.seg_a, e, g.o.na, lo_a, na);
  gs_segment(g.seg_b, e, g.o.nb, lo_b, nb);
  if (na == 0 || nb == 0) return;        // block-uniform; the finalize writes NaN without reading the partials
  const int col = chunk * GS_COLS + threadIdx.x;
  float v0 = 0.f, v1 = 0.f, v2 = 0.f;
  if (col < g.o.d) {
    float ma, sa, mb, sb;
    gs_col_stats(g.o.a, g.o.lda, lo_a, na, col, ma, sa);
    gs_col_stats(g.o.b, g.o.ldb, lo_b, nb, col, mb, sb);
    const float dm = ma - mb;
    v0 = dm * dm;
    v1 = sa;
    v2 = sb;
  }
  const double s0 = block_sum<GS_COLS / 64>((double)v0, red);
  const double s1 = block_sum<GS_COLS / 64>((double)v1, red);
  const double s2 = block_sum<GS_COLS / 64>((double)v2, red);
  if (threadIdx.x == 0) {
    double* dst = g.cols + ((long long)e * g.chunks + chunk) * 3;
    dst[0] = s0;
    dst[1] = s1;
    dst[2] = s2;
  }
}

// grid (workers, e): worker w of patient e computes the 64x64 tiles w, w + workers, ... of that patient's block of the
// distance matrix (all of D, the order of pti_latent_pairwise) and stores each tile's sum of distances
__global__ __launch_bounds__(LP_THREADS) void latent_group_cross_kernel(GsArgs g) {
  __shared__ __attribute__((aligned(16))) float As[2 * LP_KC * LP_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2 * LP_KC * LP_LD];
  __shared__ double red[LP_THREADS / 64];
  const int e = blockIdx.y;
  int lo_a, na, lo_b, nb;
  gs_segment(g.seg_a, e, g.o.na, lo_a, na);
  gs_segment(g.seg_b, e, g.o.nb, lo_b, nb);
  if (na == 0 || nb == 0) return;
  LpOperands o = g.o;
  o.a = g.o.a + (long long)lo_a * g.o.lda;
  o.b = g.o.b + (long long)lo_b * g.o.ldb;
  o.na = na;
  o.nb = nb;
  o.center = nullptr;
  const int tiles_j = lp_tiles_of(nb), tiles = lp_tiles_of(na) * tiles_j;
  const int slabs = (g.o.d + LP_SLAB - 1) / LP_SLAB;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int t = blockIdx.x; t < tiles && t < g.tiles_max; t += gridDim.x) {
    const int row0 = (t / tiles_j) * LP_TILE, col0 = (t % tiles_j) * LP_TILE;
    float tot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[i][j] = 0.f;
    lp_tile<0>(o, row0, col0, 0, slabs, As, Bs, tot);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (row0 + ty * 4 + i < na && col0 + tx * 4 + j < nb) s += (double)lp_sqrt(tot[i][j]);
    const double sum = block_sum<LP_THREADS / 64>(s, red);
    if (threadIdx.x == 0) g.cross[(long long)e * g.tiles_max + t] = sum;
    __syncthreads();                     // the staging buffers are rewritten by the next tile
  }
}

// one wavefront per patient: partials added lane-strided, then by shuffles (fixed order)
__global__ __launch_bounds__(64) void latent_group_finalize_kernel(GsArgs g, float* __restrict__ out_e4) {
  const int e = blockIdx.x, lane = threadIdx.x;
  int lo_a, na, lo_b, nb;
  gs_segment(g.seg_a, e, g.o.na, lo_a, na);
  gs_segment(g.seg_b, e, g.o.nb, lo_b, nb);
  float* o = out_e4 + 4 * (long long)e;
  if (na == 0 || nb == 0) {
    if (lane < 4) o[lane] = __builtin_nanf("");
    return;
  }
  const double* pc = g.cols + (long long)e * g.chunks * 3;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int c = lane; c < g.chunks; c += 64) {
    s0 += pc[3 * c];
    s1 += pc[3 * c + 1];
    s2 += pc[3 * c + 2];
  }
  const int tiles = min(lp_tiles_of(na) * lp_tiles_of(nb), g.tiles_max);
  const double* px = g.cross + (long long)e * g.tiles_max;
  for (int t = lane; t < tiles; t += 64) s3 += px[t];
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  s3 = wave_sum(s3);
  if (lane == 0) {
    o[0] = (float)sqrt(s0);
    o[1] = (float)(s1 / (double)g.o.d);
    o[2] = (float)(s2 / (double)g.o.d);
    o[3] = (float)(s3 / ((double)na * (double)nb));
  }
}

// doubles of workspace: [e][chunks][3] + [e][tiles_max]; 0 = unsupported
long long gs_ws_doubles(int n1, int n2, int e, int d) {
  if (!lp_shape_ok(n1, n2, d) || e <= 0 || e > 65535) return 0;
  const long long chunks = cdiv(d, GS_COLS);
  if (chunks > 0x7fffffffLL / 3) return 0;
  const long long per_patient = chunks * 3 + lp_tiles(n1, n2);
  if (per_patient > (1LL << 26) / e) return 0;
  return per_patient * e;
}

}  // namespace

extern "C" int64_t pti_latent_pairwise_ws_floats(int n1, int n2, int d) { return lp_ws_floats(n1, n2, d); }

extern "C" int pti_latent_pairwise(const float* a, int64_t lda, int n1, const float* b, int64_t ldb, int n2, int d,
                                   const float* center, int mode, float* out, int64_t ldo, float* workspace,
                                   pti_stream_t s) {
  if (!a || !b || !out || !workspace) PTI_FAIL(PTI_EINVAL, "latent_pairwise: null pointer");
  if (n1 <= 0 || n2 <= 0 || d <= 0) PTI_FAIL(PTI_EINVAL, "latent_pairwise: bad dimension n1=%d n2=%d d=%d", n1, n2, d);
  if (lda < d || ldb < d || ldo < n2)
    PTI_FAIL(PTI_EINVAL, "latent_pairwise: row stride below the row length (lda=%lld ldb=%lld d=%d, ldo=%lld n2=%d)",
             (long long)lda, (long long)ldb, d, (long long)ldo, n2);
  if (mode != 0 && mode != 1) PTI_FAIL(PTI_EUNSUPPORTED, "latent_pairwise: mode %d (0 = distance, 1 = dot product)", mode);
  if (lp_ws_floats(n1, n2, d) == 0) PTI_FAIL(PTI_EUNSUPPORTED, "latent_pairwise: unsupported shape n1=%d n2=%d d=%d", n1, n2, d);
  LpArgs p;
  p.o.a = a;
  p.o.b = b;
  p.o.center = center;
  p.o.lda = lda;
  p.o.ldb = ldb;
  p.o.na = n1;
  p.o.nb = n2;
  p.o.d = d;
  p.o.vec = lp_aligned(a) && lp_aligned(b) && lp_aligned(center) && lda % 4 == 0 && ldb % 4 == 0 && d % 4 == 0;
  p.out = out;
  p.ldo = ldo;
  p.workspace = workspace;
  p.slabs = cdiv(d, LP_SLAB);
  p.split = lp_split(n1, n2, d) ? 1 : 0;
  const dim3 grid(cdiv(n2, LP_TILE), cdiv(n1, LP_TILE), p.split ? p.slabs : 1);
  if (mode == 0)
    PTI_LAUNCH(latent_pairwise_tile_kernel<0>, grid, dim3(LP_THREADS), 0, (hipStream_t)s, p);
  else
    PTI_LAUNCH(latent_pairwise_tile_kernel<1>, grid, dim3(LP_THREADS), 0, (hipStream_t)s, p);
  PTI_CHECK_LAUNCH("latent_pairwise");
  if (p.split) {
    const long long plane = (long long)n1 * n2;
    PTI_LAUNCH(latent_pairwise_fold_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, (hipStream_t)s,
               (const float*)workspace, out, (long long)ldo, n1, n2, p.slabs, mode);
    PTI_CHECK_LAUNCH("latent_pairwise_fold");
  }
  return PTI_OK;
}

extern "C" int64_t pti_latent_group_stats_ws_floats(int n1, int n2, int e, int d) { return 2 * gs_ws_doubles(n1, n2, e, d); }

extern "C" int pti_latent_group_stats(const float* a, int64_t lda, int n1, const int32_t* seg_a, const float* b, int64_t ldb,
                                      int n2, const int32_t* seg_b, int e, int d, float* out_e4, float* workspace,
                                      pti_stream_t s) {
  if (!a || !b || !seg_a || !seg_b || !out_e4 || !workspace) PTI_FAIL(PTI_EINVAL, "latent_group_stats: null pointer");
  if (n1 <= 0 || n2 <= 0 || d <= 0 || e <= 0)
    PTI_FAIL(PTI_EINVAL, "latent_group_stats: bad dimension n1=%d n2=%d d=%d patients=%d", n1, n2, d, e);
  if (lda < d || ldb < d)
    PTI_FAIL(PTI_EINVAL, "latent_group_stats: row stride below the row length (lda=%lld ldb=%lld d=%d)", (long long)lda,
             (long long)ldb, d);
  if (((uintptr_t)workspace & 7) != 0) PTI_FAIL(PTI_EINVAL, "latent_group_stats: workspace must be 8-byte aligned");
  if (gs_ws_doubles(n1, n2, e, d) == 0)
    PTI_FAIL(PTI_EUNSUPPORTED, "latent_group_stats: unsupported shape n1=%d n2=%d d=%d patients=%d", n1, n2, d, e);
  GsArgs g;
  g.o.a = a;
  g.o.b = b;
  g.o.center = nullptr;
  g.o.lda = lda;
  g.o.ldb = ldb;
  g.o.na = n1;
  g.o.nb = n2;
  g.o.d = d;
  g.o.vec = lp_aligned(a) && lp_aligned(b) && lda % 4 == 0 && ldb % 4 == 0 && d % 4 == 0;
  g.seg_a = seg_a;
  g.seg_b = seg_b;
  g.e = e;
  g.chunks = cdiv(d, GS_COLS);
  g.tiles_max = (int)lp_tiles(n1, n2);
  g.cols = (double*)workspace;
  g.cross = g.cols + (long long)e * g.chunks * 3;
  PTI_LAUNCH(latent_group_cols_kernel, dim3(g.chunks, e), dim3(GS_COLS), 0, (hipStream_t)s, g);
  PTI_CHECK_LAUNCH("latent_group_cols");
  // enough workers that few patients with many tiles still fill the device; a worker without a tile returns at once
  int workers = cdiv(512, e);
  if (workers > g.tiles_max) workers = g.tiles_max;
  PTI_LAUNCH(latent_group_cross_kernel, dim3(workers, e), dim3(LP_THREADS), 0, (hipStream_t)s, g);
  PTI_CHECK_LAUNCH("latent_group_cross");
  PTI_LAUNCH(latent_group_finalize_kernel, dim3(e), dim3(64), 0, (hipStream_t)s, g, out_e4);
  PTI_CHECK_LAUNCH("latent_group_finalize");
  return PTI_OK;
}
