// Exact (dense, O(N^2)) t-SNE on the device (gfx950) for the latent-space analysis: the joint probabilities P of
// sklearn.manifold._t_sne._joint_probabilities and one gradient-descent iteration of sklearn's _kl_divergence +
// _gradient_descent (degrees of freedom 1, two output columns), 2 <= N <= 8192.  DESIGN.md 5k.
//
//   pti_tsne_affinities, three launches:
//     1. tsne_cond_kernel: one 256-thread workgroup per row i.  The row of squared distances sits in LDS (N floats, at
//        most 32 KB) for the whole search; sklearn's _binary_search_perplexity runs on it step for step (beta from 1, at
//        most 100 steps, stop at |H - log(perplexity)| <= 1e-5f, doubling / halving while a bound is open, bisection
//        after).  EVERYTHING of the search is fp64 -- exp, the two sums, log, beta -- as in sklearn; the sums are folded
//        in one fixed order (thread t adds j = t, t + 256, ... ascending; the 64 lanes of a wave by xor shuffles; the 4
//        waves in ascending order).  p_j|i is stored as fp32 into P's own buffer, and the fp64 sum of the stored values
//        of the row into the workspace.
//     2. tsne_joint_kernel: P_ij = max((p_j|i + p_i|j) / S, eps) in place, one workgroup per PAIR of mirrored 32x32
//        tiles (both staged in LDS before either is written), diagonal 0.  S = 2 * sum of the row sums, folded in fp64
//        in a fixed order by every workgroup.  The two addends are added in fp64, so P is symmetric bit for bit.  Per
//        tile pair the fp64 sums of P log P and of P go to the workspace ...
//     3. tsne_scalar_kernel: ... and one wavefront-ordered fold of those writes {sum P log P, sum P} (both fp64).
//   pti_tsne_step, two launches (a third, one wavefront, only in an iteration whose record the caller asks for):
//     1. tsne_forces_kernel streams P once.  One wavefront per workgroup owns 4 rows and one CHUNK of columns; a lane
//        owns 4 consecutive columns of every 256 (one 16-byte load of P per row where P allows it, the same columns by
//        scalar loads where not: the order of the sums is the same).  Per row and lane fp32 fmaf chains in ascending
//        column order for sum num, sum P num (y_i - y_j), sum num^2 (y_i - y_j); num = 1 / (1 + |y_i - y_j|^2) is a
//        correctly rounded division.  Only in an iteration with a record: sum P log num, every term and the sum in fp64
//        (-log(1 + |y_i - y_j|^2) from the fp32 distance; sklearn, too, evaluates the error only where it is read).
//        The 64 lane sums are folded in fp64 by xor shuffles and stored: per (chunk, row) the four force sums, per
//        (chunk, row block) sum num and sum P log num.
//        The grid is (row blocks) x (chunks); the number of chunks is a function of N alone (about 4096 wavefronts
//        where N allows it), so the order of every sum depends on N and on nothing else.
//     2. tsne_update_kernel: every workgroup folds Z = sum num and sum P log num over (row block, chunk) in fp64 --
//        chunks ascending, row blocks thread-strided, lanes by shuffles, waves ascending -- and then owns 64 rows:
//        chunk partials ascending in fp64, grad = 4 (exaggeration F_att - F_rep / Z), sklearn's gains / momentum update
//        in fp32, Y_out = Y_in + update.  With a record, workgroup 0 writes
//        KL = a (sum P log P + sum P (log a + log Z) - sum P log num) for P exaggerated by a, which is what sklearn
//        reports during the exploration stage.  sklearn's clamp of Q at eps is left out: it changes a gradient term by
//        at most eps * num and KL only where num / Z < 2.2e-16.
//        Every workgroup stores the fp64 sum of (gain * grad)^2 of its rows;
//     3. tsne_norm_kernel folds those in a fixed order: record[1] = |gain * grad|_2, the norm sklearn tests.
// No atomics anywhere; partial sums travel through plain vector stores; results are bitwise reproducible.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int TS_MAX_N = 8192;
constexpr int TS_THREADS = 256;
constexpr int TS_TILE = 32;          // tile edge of the symmetrisation
constexpr int TS_ROWS = 4;           // rows of one wavefront of the force pass
constexpr int TS_COLS = 256;         // columns of one wavefront iteration: 64 lanes x 4
constexpr int TS_WAVES = 4096;       // wavefronts the force pass aims at
constexpr int TS_UPD_ROWS = 64;      // rows of one workgroup of the update
constexpr float TS_EPS = 2.220446e-16f;

// fixed-order sums of two doubles per thread over a 256-thread workgroup, returned to every thread; not two
// block_sum<4> calls: both values share one pair of barriers
__device__ __forceinline__ void ts_block_sum2(double& a, double& b, double* red) {
  const int tid = threadIdx.x;
  const double wa = wave_sum(a), wb = wave_sum(b);
  __syncthreads();                       // `red` may still be read from an earlier call
  if ((tid & 63) == 0) {
    red[tid >> 6] = wa;
    red[4 + (tid >> 6)] = wb;
  }
  __syncthreads();
  a = red[0];
  b = red[4];
#pragma unroll
  for (int w = 1; w < TS_THREADS / 64; ++w) {
    a += red[w];
    b += red[4 + w];
  }
}

// ---- affinities ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_THREADS) void tsne_cond_kernel(const float* __restrict__ d2, long long ldd, int n,
                                                               double log_perp, float* __restrict__ cond, long long ldp,
                                                               double* __restrict__ rowsum) {
  __shared__ float row[TS_MAX_N];
  __shared__ double red[8];
  const int i = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < n; j += TS_THREADS) row[j] = d2[(long long)i * ldd + j];
  __syncthreads();
  const double tol = (double)1e-5f, tiny = (double)1e-8f;   // sklearn keeps both as C floats
  double beta = 1.0, beta_min = 0.0, beta_max = 0.0, beta_used = 1.0, sum = 1.0;
  bool has_min = false, has_max = false;
  for (int step = 0; step < 100; ++step) {
    double s = 0.0, sd = 0.0;
    for (int j = tid; j < n; j += TS_THREADS) {
      if (j == i) continue;
      const double d = (double)row[j];
      const double p = exp(-d * beta);
      s += p;
      sd += d * p;
    }
    ts_block_sum2(s, sd, red);           // the same bits in every thread: the search below is workgroup-uniform
    if (s == 0.0) s = tiny;
    sum = s;
    beta_used = beta;
    const double diff = log(s) + beta * (sd / s) - log_perp;
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      beta_min = beta;
      has_min = true;
      beta = has_max ? (beta + beta_max) * 0.5 : beta * 2.0;
    } else {
      beta_max = beta;
      has_max = true;
      beta = has_min ? (beta + beta_min) * 0.5 : beta * 0.5;
    }
  }
  double rs = 0.0, unused = 0.0;
  for (int j = tid; j < n; j += TS_THREADS) {
    const float p = j == i ? 0.f : (float)(exp(-(double)row[j] * beta_used) / sum);
    cond[(long long)i * ldp + j] = p;
    rs += (double)p;
  }
  ts_block_sum2(rs, unused, red);
  if (tid == 0) rowsum[i] = rs;
}

// grid (T, T); the workgroup (bx >= by) owns tile (by, bx) and its mirror (bx, by)
__global__ __launch_bounds__(TS_THREADS) void tsne_joint_kernel(float* __restrict__ p, long long ldp, int n,
                                                                const double* __restrict__ rowsum,
                                                                double* __restrict__ partial) {
  __shared__ float ta[TS_TILE][TS_TILE + 1];
  __shared__ float tb[TS_TILE][TS_TILE + 1];
  __shared__ double red[8];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int bi = blockIdx.y, bj = blockIdx.x;
  double* dst = partial + 2 * ((long long)bi * gridDim.x + bj);
  if (bj < bi) {                         // workgroup-uniform
    if (tid == 0) dst[0] = dst[1] = 0.0;
    return;
  }
  double total = 0.0, unused = 0.0;
  for (int r = tid; r < n; r += TS_THREADS) total += rowsum[r];
  ts_block_sum2(total, unused, red);
  total = fmax(2.0 * total, (double)TS_EPS);
  const int i0 = bi * TS_TILE, j0 = bj * TS_TILE;
#pragma unroll
  for (int k = 0; k < TS_TILE / 8; ++k) {
    const int r = ty + 8 * k;
    ta[r][tx] = (i0 + r < n && j0 + tx < n) ? p[(long long)(i0 + r) * ldp + j0 + tx] : 0.f;
    tb[r][tx] = (j0 + r < n && i0 + tx < n) ? p[(long long)(j0 + r) * ldp + i0 + tx] : 0.f;
  }
  __syncthreads();
  double s_plogp = 0.0, s_p = 0.0;
#pragma unroll
  for (int k = 0; k < TS_TILE / 8; ++k) {
    const int r = ty + 8 * k;
    // element (i0 + r, j0 + tx) of the tile and element (j0 + r, i0 + tx) of its mirror
    if (i0 + r < n && j0 + tx < n) {
      float v = 0.f;
      if (i0 + r != j0 + tx) v = fmaxf((float)(((double)ta[r][tx] + (double)tb[tx][r]) / total), TS_EPS);
      p[(long long)(i0 + r) * ldp + j0 + tx] = v;
      if (v > 0.f) {
        s_plogp += (double)v * log((double)v);
        s_p += (double)v;
      }
    }
    if (bi != bj && j0 + r < n && i0 + tx < n) {
      const float v = fmaxf((float)(((double)ta[tx][r] + (double)tb[r][tx]) / total), TS_EPS);
      p[(long long)(j0 + r) * ldp + i0 + tx] = v;
      s_plogp += (double)v * log((double)v);
      s_p += (double)v;
    }
  }
  ts_block_sum2(s_plogp, s_p, red);
  if (tid == 0) {
    dst[0] = s_plogp;
    dst[1] = s_p;
  }
}

__global__ __launch_bounds__(TS_THREADS) void tsne_scalar_kernel(const double* __restrict__ partial, int count,
                                                                 double* __restrict__ out2) {
  __shared__ double red[8];
  double a = 0.0, b = 0.0;
  for (int t = threadIdx.x; t < count; t += TS_THREADS) {
    a += partial[2 * t];
    b += partial[2 * t + 1];
  }
  ts_block_sum2(a, b, red);
  if (threadIdx.x == 0) {
    out2[0] = a;
    out2[1] = b;
  }
}

// ---- descent step -------------------------------------------------------------------------------------------------
struct TsPlan {
  int row_blocks;        // workgroups of the force pass along the rows (TS_ROWS rows each)
  int col_groups;        // 256-column groups of a row
  int groups_per_chunk, chunks;
  int upd_blocks;        // workgroups of the update
};

// a function of n alone
TsPlan ts_plan(int n) {
  TsPlan pl;
  pl.row_blocks = cdiv(n, TS_ROWS);
  pl.col_groups = cdiv(n, TS_COLS);
  int want = cdiv(TS_WAVES, pl.row_blocks);
  if (want > pl.col_groups) want = pl.col_groups;
  pl.groups_per_chunk = cdiv(pl.col_groups, want);
  pl.chunks = cdiv(pl.col_groups, pl.groups_per_chunk);
  pl.upd_blocks = cdiv(n, TS_UPD_ROWS);
  return pl;
}

struct TsStep {
  const float* p;
  long long ldp;
  const float* y_in;
  float* y_out;
  float* update;
  float* gains;
  const double* plogp;   // {sum P log P, sum P}
  double* record;        // {KL, |gain * grad|}
  double* rowpart;       // [chunks][n][4]: F_att x, y, F_rep x, y
  double* blocksum;      // [chunks][row_blocks][2]: sum num, sum P log num
  double* gradpart;      // [upd_blocks]
  int n, vec;
  TsPlan pl;
  float exaggeration, momentum, lr;
};

template <bool KL>
__global__ __launch_bounds__(64) void tsne_forces_kernel(TsStep a) {
#pragma clang fp reassociate(off)
  const int lane = threadIdx.x, rb = blockIdx.x, chunk = blockIdx.y;
  const int n = a.n, row0 = rb * TS_ROWS;
  float yi[TS_ROWS][2];
#pragma unroll
  for (int r = 0; r < TS_ROWS; ++r) {
    const int row = min(row0 + r, n - 1);
    yi[r][0] = a.y_in[2 * row];
    yi[r][1] = a.y_in[2 * row + 1];
  }
  float acc[TS_ROWS][5];                 // num, att x, att y, rep x, rep y
  double pl[TS_ROWS];                    // P log num (KL only)
#pragma unroll
  for (int r = 0; r < TS_ROWS; ++r) {
    pl[r] = 0.0;
#pragma unroll
    for (int v = 0; v < 5; ++v) acc[r][v] = 0.f;
  }
  const int g0 = chunk * a.pl.groups_per_chunk, g1 = min(g0 + a.pl.groups_per_chunk, a.pl.col_groups);
  for (int g = g0; g < g1; ++g) {
    const int j0 = g * TS_COLS + lane * 4;
    float yj[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool in = j0 + c < n;
      yj[c][0] = in ? a.y_in[2 * (j0 + c)] : 0.f;
      yj[c][1] = in ? a.y_in[2 * (j0 + c) + 1] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < TS_ROWS; ++r) {
      const int row = row0 + r;
      f32x4 pv = {0.f, 0.f, 0.f, 0.f};
      if (row < n) {
        const float* src = a.p + (long long)row * a.ldp + j0;
        if (a.vec && j0 + 3 < n) {
          pv = *(const f32x4*)src;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (j0 + c < n) pv[c] = src[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + c;
        const float dx = yi[r][0] - yj[c][0], dy = yi[r][1] - yj[c][1];
        const float dist = fmaf(dy, dy, dx * dx);
        const float q = __fdiv_rn(1.0f, 1.0f + dist);
        const float num = (row < n && j < n && j != row) ? q : 0.f;
        const float pn = pv[c] * num, nn = num * num;
        acc[r][0] = acc[r][0] + num;
        acc[r][1] = fmaf(pn, dx, acc[r][1]);
        acc[r][2] = fmaf(pn, dy, acc[r][2]);
        acc[r][3] = fmaf(nn, dx, acc[r][3]);
        acc[r][4] = fmaf(nn, dy, acc[r][4]);
        // log num = -log(1 + dist) in fp64, from dist itself; P is 0 on the diagonal and outside the matrix
        if (KL) pl[r] -= (double)pv[c] * log(1.0 + (double)dist);
      }
    }
  }
  double bs_num = 0.0, bs_pl = 0.0;
#pragma unroll
  for (int r = 0; r < TS_ROWS; ++r) {
    double f[5];
#pragma unroll
    for (int v = 0; v < 5; ++v) f[v] = wave_sum((double)acc[r][v]);
    bs_num += f[0];
    if (KL) bs_pl += wave_sum(pl[r]);
    if (lane == 0 && row0 + r < n) {
      double* dst = a.rowpart + ((long long)chunk * n + row0 + r) * 4;
      dst[0] = f[1];
      dst[1] = f[2];
      dst[2] = f[3];
      dst[3] = f[4];
    }
  }
  if (lane == 0) {
    double* dst = a.blocksum + ((long long)chunk * a.pl.row_blocks + rb) * 2;
    dst[0] = bs_num;
    dst[1] = bs_pl;
  }
}

__global__ __launch_bounds__(TS_THREADS) void tsne_update_kernel(TsStep a, int with_record) {
  __shared__ double red[8];
  const int tid = threadIdx.x, n = a.n;
  double z = 0.0, pl = 0.0;
  for (int b = tid; b < a.pl.row_blocks; b += TS_THREADS) {
    double zb = 0.0, pb = 0.0;
    for (int c = 0; c < a.pl.chunks; ++c) {
      const double* src = a.blocksum + ((long long)c * a.pl.row_blocks + b) * 2;
      zb += src[0];
      pb += src[1];
    }
    z += zb;
    pl += pb;
  }
  ts_block_sum2(z, pl, red);
  if (tid < 64) {
    const int row = blockIdx.x * TS_UPD_ROWS + tid;
    double gn = 0.0;
    if (row < n) {
      double f[4] = {0.0, 0.0, 0.0, 0.0};
      for (int c = 0; c < a.pl.chunks; ++c) {
        const double* src = a.rowpart + ((long long)c * n + row) * 4;
#pragma unroll
        for (int v = 0; v < 4; ++v) f[v] += src[v];
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float g = (float)(4.0 * ((double)a.exaggeration * f[k] - f[2 + k] / z));
        float u = a.update[2 * row + k], gain = a.gains[2 * row + k];
        const bool opposite = (u < 0.f && g > 0.f) || (u > 0.f && g < 0.f);   // update * grad < 0 without the underflow
        gain = opposite ? gain + 0.2f : gain * 0.8f;
        gain = fmaxf(gain, 0.01f);
        const float gg = g * gain;
        u = a.momentum * u - a.lr * gg;
        a.gains[2 * row + k] = gain;
        a.update[2 * row + k] = u;
        a.y_out[2 * row + k] = a.y_in[2 * row + k] + u;
        gn += (double)gg * (double)gg;
      }
    }
    gn = wave_sum(gn);
    if (tid == 0) a.gradpart[blockIdx.x] = gn;
  }
  if (with_record && blockIdx.x == 0 && tid == 0) {
    const double ex = (double)a.exaggeration;
    a.record[0] = ex * (a.plogp[0] + a.plogp[1] * (log(ex) + log(z)) - pl);
  }
}

__global__ __launch_bounds__(64) void tsne_norm_kernel(const double* __restrict__ gradpart, int count,
                                                       double* __restrict__ record) {
  double s = 0.0;
  for (int t = threadIdx.x; t < count; t += 64) s += gradpart[t];
  s = wave_sum(s);
  if (threadIdx.x == 0) record[1] = sqrt(s);
}

bool ts_shape_ok(int n, int n_components) { return n >= 2 && n <= TS_MAX_N && n_components == 2; }
long long ts_aff_ws_doubles(int n) {
  const long long t = cdiv(n, TS_TILE);
  return n + 2 * t * t;
}
long long ts_step_ws_doubles(int n) {
  const TsPlan pl = ts_plan(n);
  return (long long)pl.chunks * n * 4 + (long long)pl.chunks * pl.row_blocks * 2 + pl.upd_blocks;
}

}  // namespace

extern "C" int64_t pti_tsne_affinities_ws_floats(int n) { return ts_shape_ok(n, 2) ? 2 * ts_aff_ws_doubles(n) : 0; }

extern "C" int pti_tsne_affinities(const float* d2, int64_t ldd, int n, float perplexity, float* p, int64_t ldp,
                                   double* plogp2, float* workspace, pti_stream_t s) {
  if (!d2 || !p || !plogp2 || !workspace) PTI_FAIL(PTI_EINVAL, "tsne_affinities: null pointer");
  if (n < 2) PTI_FAIL(PTI_EINVAL, "tsne_affinities: bad dimension n=%d (at least 2 rows)", n);
  if (n > TS_MAX_N) PTI_FAIL(PTI_EUNSUPPORTED, "tsne_affinities: unsupported shape n=%d (at most %d rows)", n, TS_MAX_N);
  if (!(perplexity > 0.f) || !(perplexity < (float)n))
    PTI_FAIL(PTI_EINVAL, "tsne_affinities: perplexity %g must be positive and below n=%d", (double)perplexity, n);
  if (ldd < n || ldp < n)
    PTI_FAIL(PTI_EINVAL, "tsne_affinities: row stride below the row length (ldd=%lld ldp=%lld n=%d)", (long long)ldd,
             (long long)ldp, n);
  if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)plogp2 & 7) != 0)
    PTI_FAIL(PTI_EINVAL, "tsne_affinities: workspace and plogp2 must be 8-byte aligned");
  if (d2 == p) PTI_FAIL(PTI_EINVAL, "tsne_affinities: p must not be d2");
  double* rowsum = (double*)workspace;
  double* partial = rowsum + n;
  const int t = cdiv(n, TS_TILE);
  PTI_LAUNCH(tsne_cond_kernel, dim3(n), dim3(TS_THREADS), 0, (hipStream_t)s, d2, (long long)ldd, n,
             log((double)perplexity), p, (long long)ldp, rowsum);
  PTI_CHECK_LAUNCH("tsne_cond");
  PTI_LAUNCH(tsne_joint_kernel, dim3(t, t), dim3(TS_THREADS), 0, (hipStream_t)s, p, (long long)ldp, n,
             (const double*)rowsum, partial);
  PTI_CHECK_LAUNCH("tsne_joint");
  PTI_LAUNCH(tsne_scalar_kernel, dim3(1), dim3(TS_THREADS), 0, (hipStream_t)s, (const double*)partial, t * t, plogp2);
  PTI_CHECK_LAUNCH("tsne_scalar");
  return PTI_OK;
}

extern "C" int64_t pti_tsne_step_ws_floats(int n, int n_components) {
  return ts_shape_ok(n, n_components) ? 2 * ts_step_ws_doubles(n) : 0;
}

extern "C" int pti_tsne_step(const float* p, int64_t ldp, int n, int n_components, const float* y_in, float* y_out,
                             float* update, float* gains, const double* plogp2, float exaggeration, float momentum,
                             float lr, double* record, int with_record, float* workspace, pti_stream_t s) {
  if (!p || !y_in || !y_out || !update || !gains || !plogp2 || !record || !workspace)
    PTI_FAIL(PTI_EINVAL, "tsne_step: null pointer");
  if (n < 2) PTI_FAIL(PTI_EINVAL, "tsne_step: bad dimension n=%d (at least 2 rows)", n);
  if (n_components != 2) PTI_FAIL(PTI_EUNSUPPORTED, "tsne_step: n_components=%d (only 2 is built)", n_components);
  if (n > TS_MAX_N) PTI_FAIL(PTI_EUNSUPPORTED, "tsne_step: unsupported shape n=%d (at most %d rows)", n, TS_MAX_N);
  if (ldp < n) PTI_FAIL(PTI_EINVAL, "tsne_step: row stride below the row length (ldp=%lld n=%d)", (long long)ldp, n);
  if (!(exaggeration > 0.f)) PTI_FAIL(PTI_EINVAL, "tsne_step: exaggeration %g must be positive", (double)exaggeration);
  if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)plogp2 & 7) != 0 || ((uintptr_t)record & 7) != 0)
    PTI_FAIL(PTI_EINVAL, "tsne_step: workspace, plogp2 and record must be 8-byte aligned");
  if (y_in == y_out) PTI_FAIL(PTI_EINVAL, "tsne_step: y_out must not be y_in (the embedding is double buffered)");
  TsStep a;
  a.p = p;
  a.ldp = ldp;
  a.y_in = y_in;
  a.y_out = y_out;
  a.update = update;
  a.gains = gains;
  a.plogp = plogp2;
  a.record = record;
  a.n = n;
  a.vec = ((uintptr_t)p & 15) == 0 && ldp % 4 == 0;
  a.pl = ts_plan(n);
  a.rowpart = (double*)workspace;
  a.blocksum = a.rowpart + (long long)a.pl.chunks * n * 4;
  a.gradpart = a.blocksum + (long long)a.pl.chunks * a.pl.row_blocks * 2;
  a.exaggeration = exaggeration;
  a.momentum = momentum;
  a.lr = lr;
  const dim3 grid(a.pl.row_blocks, a.pl.chunks);
  if (with_record)
    PTI_LAUNCH(tsne_forces_kernel<true>, grid, dim3(64), 0, (hipStream_t)s, a);
  else
    PTI_LAUNCH(tsne_forces_kernel<false>, grid, dim3(64), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("tsne_forces");
  PTI_LAUNCH(tsne_update_kernel, dim3(a.pl.upd_blocks), dim3(TS_THREADS), 0, (hipStream_t)s, a, with_record);
  PTI_CHECK_LAUNCH("tsne_update");
  if (with_record) {
    PTI_LAUNCH(tsne_norm_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (const double*)a.gradpart, a.pl.upd_blocks, record);
    PTI_CHECK_LAUNCH("tsne_norm");
  }
  return PTI_OK;
}
