// Regression head on frozen latents, evaluation side (gfx950): the forward of LatentRegressor in eval mode fused with the
// target de-normalisation and the per-row loss, and the fold of a whole evaluation set into val_loss / MAE / MSE.
//
// Stands in for what the reference does per validation batch with a dozen small launches
// (src/pti_ldm_vae/models/regression_head.py:30-78: nn.Linear / activation / nn.Linear ...;
// src/pti_ldm_vae/utils/regression_utils.py:350-388: normalise the targets, loss_fn, de-normalise, .cpu()) and, once per
// run, on the host (src/pti_ldm_vae/utils/metrics.py:6-37).
//
//   pti_mlp_head_fwd, launch 1 (mlp_head_first_kernel): the first layer is the only one with a long K (4 096 .. 40 960).
//     A 256-thread workgroup owns 64 hidden units and a tile of up to 16 rows, so W0 is read once per row tile.  Chunks
//     of 32 columns of x and W0 are staged k-major in LDS (double buffered), loads along k are 16 bytes wide (scalar
//     when d % 4 != 0 or a base / stride is unaligned), every thread keeps one row x four units.  The sum over d has ONE
//     order that depends on d only: fmaf chains over 512-column slabs in ascending k, the slab sums added in ascending
//     order.  Route "direct": a workgroup walks all slabs and stores the sums [n][h1].  Route "split" (few workgroups,
//     several slabs): a workgroup handles one slab and stores its partial [slab][n][h1]; the tail adds the slabs in the
//     same ascending order, so both routes give the same bits.
//   launch 2 (mlp_head_tail_kernel): one workgroup per 4 rows.  Folds the slab planes, adds the bias, applies the
//     activation and keeps the row tile's activations in LDS (two buffers of 4 x 1024 floats); every further layer is one
//     wavefront per output unit (lanes stride k, a fixed shuffle tree adds the 64 lane sums); then de-normalisation
//     and the row loss on the normalised scale, summed over the targets in ascending order.
//   Row i of pred / rowloss depends on row i only: not on n, on the row's position or on the route.
//   pti_regression_metrics: one workgroup, fp64, fixed order.
// No atomics anywhere; partial results travel through plain vector stores.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int MH_ROWS = 16;      // rows per tile of the first layer
constexpr int MH_UNITS = 64;     // hidden units per workgroup of the first layer
constexpr int MH_KC = 32;        // columns per staged chunk
constexpr int MH_LDA = 20;       // LDS pitch of the x chunk (16 rows + pad), floats
constexpr int MH_LDB = 68;       // LDS pitch of the W0 chunk (64 units + pad): 16-byte aligned rows
constexpr int MH_SLAB = 512;     // columns per fmaf chain (fixed: the summation order is a function of d only)
constexpr int MH_THREADS = 256;
constexpr int MH_TR = 4;         // rows per workgroup of the tail
constexpr int MH_SPLIT_MAX_WGS = 16;             // split d over workgroups only up to this many (row tile, unit block) pairs
constexpr long long MH_SPLIT_MAX_FLOATS = 1LL << 26;
constexpr int MH_MAX_N = 1 << 24, MH_MAX_D = 1 << 24;   // grid x / z stay in range, 64-bit products cannot overflow

struct MhFirst {
  const float* x;        // [n][ldx]
  const float* w;        // W0 [h1][d]
  float* ws;             // [planes][n][h1]
  long long ldx;
  int n, d, h1;
  int slabs, split;
  int vec;               // x and W0 16-byte aligned, ldx and d multiples of 4
};

struct MhTail {
  const float* ws;       // [planes][n][h1]
  const float* params;   // W0, b0, W1, b1, ...
  const float* mean;     // [T] or null
  const float* std;      // [T] or null (both or neither)
  const float* targets;  // [n][T] or null
  float* pred;           // [n][T]
  float* rowloss;        // [n] (with targets)
  int dims[PTI_MLP_MAX_LAYERS + 1];
  int n_layers, act, loss_kind, n, planes;
};

// four consecutive columns k .. k+3 of `row` of p; zeros for a row >= rows or a column >= d
__device__ __forceinline__ f32x4 mh_fetch(const float* __restrict__ p, long long ld, int rows, int row, int k, int d, int vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row >= rows || k >= d) return v;
  const float* src = p + (long long)row * ld + k;
  if (vec) {
    v = *(const f32x4*)src;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (k + c < d) v[c] = src[c];
  }
  return v;
}

__device__ __forceinline__ float mh_act(float v, int act) {
  switch (act) {
    case 0: return fmaxf(v, 0.f);
    case 1: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));   // nn.GELU(): the exact erf form
    case 2: return v > 0.f ? v : 0.01f * v;
    default: return v > 0.f ? v : expm1f(v);
  }
}

// grid (row tiles, unit blocks, split ? slabs : 1)
__global__ __launch_bounds__(MH_THREADS) void mlp_head_first_kernel(MhFirst p) {
#pragma clang fp reassociate(off)
  __shared__ __attribute__((aligned(16))) float As[2 * MH_KC * MH_LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2 * MH_KC * MH_LDB];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * MH_ROWS, unit0 = blockIdx.y * MH_UNITS;
  const int slab0 = p.split ? (int)blockIdx.z : 0;
  const int slab1 = p.split ? slab0 + 1 : p.slabs;
  const int tx = tid & 15, ty = tid >> 4;               // compute: row ty of the tile, units tx*4 .. tx*4+3
  const int sr = tid >> 3, sk = (tid & 7) * 4;          // staging: row / unit sr (and sr + 32), columns sk .. sk+3 of the chunk
  const bool active = (row0 + ty < p.n) && (unit0 + tx * 4 < p.h1);
  const int k_begin = slab0 * MH_SLAB;
  const int k_end = min(p.d, slab1 * MH_SLAB);
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, tot[4] = {0.f, 0.f, 0.f, 0.f};

  f32x4 ra = {0.f, 0.f, 0.f, 0.f}, rb0, rb1;
  if (sr < MH_ROWS) ra = mh_fetch(p.x, p.ldx, p.n, row0 + sr, k_begin + sk, p.d, p.vec);
  rb0 = mh_fetch(p.w, p.d, p.h1, unit0 + sr, k_begin + sk, p.d, p.vec);
  rb1 = mh_fetch(p.w, p.d, p.h1, unit0 + sr + 32, k_begin + sk, p.d, p.vec);
  int buf = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (sr < MH_ROWS) As[(sk + c) * MH_LDA + sr] = ra[c];
    Bs[(sk + c) * MH_LDB + sr] = rb0[c];
    Bs[(sk + c) * MH_LDB + sr + 32] = rb1[c];
  }
  __syncthreads();

  for (int kc = k_begin; kc < k_end; kc += MH_KC) {
    const bool has_next = kc + MH_KC < k_end;
    if (has_next) {
      if (sr < MH_ROWS) ra = mh_fetch(p.x, p.ldx, p.n, row0 + sr, kc + MH_KC + sk, p.d, p.vec);
      rb0 = mh_fetch(p.w, p.d, p.h1, unit0 + sr, kc + MH_KC + sk, p.d, p.vec);
      rb1 = mh_fetch(p.w, p.d, p.h1, unit0 + sr + 32, kc + MH_KC + sk, p.d, p.vec);
    }
    if (active) {
      const float* as = As + buf * (MH_KC * MH_LDA) + ty;
      const float* bs = Bs + buf * (MH_KC * MH_LDB) + tx * 4;
#pragma unroll
      for (int kk = 0; kk < MH_KC; ++kk) {
        const float a = as[kk * MH_LDA];
        const f32x4 b4 = *(const f32x4*)(bs + kk * MH_LDB);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(a, b4[j], acc[j]);
      }
      // end of a slab (MH_SLAB is a multiple of MH_KC and k_begin a multiple of MH_SLAB) or of the row
      if (((kc + MH_KC) % MH_SLAB) == 0 || !has_next) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          tot[j] = tot[j] + acc[j];
          acc[j] = 0.f;
        }
      }
    }
    if (has_next) {
      float* an = As + (buf ^ 1) * (MH_KC * MH_LDA);
      float* bn = Bs + (buf ^ 1) * (MH_KC * MH_LDB);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (sr < MH_ROWS) an[(sk + c) * MH_LDA + sr] = ra[c];
        bn[(sk + c) * MH_LDB + sr] = rb0[c];
        bn[(sk + c) * MH_LDB + sr + 32] = rb1[c];
      }
    }
    __syncthreads();
    buf ^= 1;
  }

  const int r = row0 + ty;
  if (r >= p.n) return;
  float* dst = p.ws + ((long long)slab0 * p.n + r) * p.h1;   // direct: slab0 == 0, the one plane
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int u = unit0 + tx * 4 + j;
    if (u < p.h1) dst[u] = tot[j];
  }
}

// grid (cdiv(n, MH_TR))
__global__ __launch_bounds__(MH_THREADS) void mlp_head_tail_kernel(MhTail p) {
#pragma clang fp reassociate(off)
  __shared__ float buf[2][MH_TR][PTI_MLP_MAX_WIDTH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * MH_TR;
  const int h1 = p.dims[1];
  const float* bias = p.params + (long long)p.dims[0] * h1;

  // first layer: the slab planes in ascending order (one plane on the direct route), bias, activation
  for (int e = tid; e < MH_TR * h1; e += MH_THREADS) {
    const int r = e / h1, j = e - r * h1, row = row0 + r;
    float v = 0.f;
    if (row < p.n) {
      float tot = 0.f;
      for (int s = 0; s < p.planes; ++s) tot = tot + p.ws[((long long)s * p.n + row) * h1 + j];
      v = tot + bias[j];
      if (p.n_layers > 1) v = mh_act(v, p.act);
    }
    buf[0][r][j] = v;
  }
  __syncthreads();

  int cur = 0;
  const float* w = bias + h1;
  for (int l = 1; l < p.n_layers; ++l) {
    const int K = p.dims[l], width = p.dims[l + 1];
    const bool last = l == p.n_layers - 1;
    bias = w + (long long)K * width;
    for (int j = wave; j < width; j += MH_THREADS / 64) {       // wave-uniform
      const float* wr = w + (long long)j * K;
      float part[MH_TR];
#pragma unroll
      for (int r = 0; r < MH_TR; ++r) part[r] = 0.f;
      for (int k = lane; k < K; k += 64) {
        const float wv = wr[k];
#pragma unroll
        for (int r = 0; r < MH_TR; ++r) part[r] = fmaf(buf[cur][r][k], wv, part[r]);
      }
#pragma unroll
      for (int r = 0; r < MH_TR; ++r) part[r] = wave_sum(part[r]);
      if (lane == 0) {
        const float b = bias[j];
#pragma unroll
        for (int r = 0; r < MH_TR; ++r) {
          float v = part[r] + b;
          if (!last) v = mh_act(v, p.act);
          buf[cur ^ 1][r][j] = v;
        }
      }
    }
    __syncthreads();
    cur ^= 1;
    w = bias + width;
  }

  // de-normalisation and the loss terms on the normalised scale; buf[cur ^ 1] is free again
  const int T = p.dims[p.n_layers];
  for (int e = tid; e < MH_TR * T; e += MH_THREADS) {
    const int r = e / T, t = e - r * T, row = row0 + r;
    if (row >= p.n) continue;
    const float out = buf[cur][r][t];
    p.pred[(long long)row * T + t] = p.mean ? fmaf(out, p.std[t], p.mean[t]) : out;
    if (p.targets) {
      const float tg = p.targets[(long long)row * T + t];
      const float want = p.mean ? __fdiv_rn(tg - p.mean[t], p.std[t]) : tg;
      const float df = out - want;
      float term;
      if (p.loss_kind == 0) {
        term = df * df;
      } else {
        const float a = fabsf(df);
        term = a < 1.0f ? 0.5f * a * a : a - 0.5f;
      }
      buf[cur ^ 1][r][t] = term;
    }
  }
  __syncthreads();
  if (p.targets && tid < MH_TR && row0 + tid < p.n) {
    float s = 0.f;
    for (int t = 0; t < T; ++t) s = s + buf[cur ^ 1][tid][t];
    p.rowloss[row0 + tid] = s;
  }
}

// one workgroup; out[0] = mean over the chunks of `batch` rows of (sum rowloss / (rows * T)); out[1..T] MAE, out[T+1..2T] MSE
// per target; out[2T+1], out[2T+2] their means over the targets
__global__ __launch_bounds__(MH_THREADS) void regression_metrics_kernel(const float* __restrict__ pred,
                                                                         const float* __restrict__ targets,
                                                                         const float* __restrict__ rowloss, int n, int t,
                                                                         int batch, double* __restrict__ out) {
  __shared__ double red[MH_THREADS / 64];
  __shared__ double per_target[2 * PTI_MLP_MAX_OUT];
  const int tid = threadIdx.x;
  const int chunks = (n + batch - 1) / batch;
  double v = 0.0;
  for (int c = tid; c < chunks; c += MH_THREADS) {
    const long long lo = (long long)c * batch;
    const int rows = (int)(lo + batch <= n ? batch : n - lo);
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += (double)rowloss[lo + r];
    v += s / ((double)rows * (double)t);
  }
  const double loss = block_sum<MH_THREADS / 64>(v, red) / (double)chunks;
  for (int k = 0; k < t; ++k) {
    double sa = 0.0, sq = 0.0;
    for (int r = tid; r < n; r += MH_THREADS) {
      const double df = (double)pred[(long long)r * t + k] - (double)targets[(long long)r * t + k];
      sa += fabs(df);
      sq += df * df;
    }
    sa = block_sum<MH_THREADS / 64>(sa, red);
    sq = block_sum<MH_THREADS / 64>(sq, red);
    if (tid == 0) {
      per_target[k] = sa / (double)n;
      per_target[t + k] = sq / (double)n;
    }
  }
  __syncthreads();
  if (tid == 0) {
    out[0] = loss;
    double ma = 0.0, ms = 0.0;
    for (int k = 0; k < t; ++k) {
      out[1 + k] = per_target[k];
      out[1 + t + k] = per_target[t + k];
      ma += per_target[k];
      ms += per_target[t + k];
    }
    out[2 * t + 1] = ma / (double)t;
    out[2 * t + 2] = ms / (double)t;
  }
}

// 0 = fine, else the PTI_E* code; `why` names the reason
int mh_check_dims(int n, int d, const int32_t* dims, int n_layers, const char** why) {
  *why = "";
  if (!dims) { *why = "null pointer (dims)"; return PTI_EINVAL; }
  if (n < 1 || d < 1 || n_layers < 1) { *why = "bad dimension (n, d, n_layers must be >= 1)"; return PTI_EINVAL; }
  if (n_layers > PTI_MLP_MAX_LAYERS) { *why = "more than PTI_MLP_MAX_LAYERS layers"; return PTI_EUNSUPPORTED; }
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1) { *why = "bad dimension (a layer width < 1)"; return PTI_EINVAL; }
  if (dims[0] != d) { *why = "bad dimension (dims[0] != d)"; return PTI_EINVAL; }
  for (int l = 1; l < n_layers; ++l)
    if (dims[l] > PTI_MLP_MAX_WIDTH) { *why = "hidden width above PTI_MLP_MAX_WIDTH"; return PTI_EUNSUPPORTED; }
  if (dims[n_layers] > PTI_MLP_MAX_OUT) { *why = "more than PTI_MLP_MAX_OUT outputs"; return PTI_EUNSUPPORTED; }
  if (n > MH_MAX_N || d > MH_MAX_D) { *why = "n or d too large to index"; return PTI_EUNSUPPORTED; }
  return PTI_OK;
}

long long mh_wgs(int n, int h1) { return (long long)cdiv(n, MH_ROWS) * cdiv(h1, MH_UNITS); }
// a function of the shape only: which route is taken never changes a result bit
bool mh_split(int n, int d, int h1) {
  const long long slabs = cdiv(d, MH_SLAB);
  return slabs > 1 && mh_wgs(n, h1) <= MH_SPLIT_MAX_WGS && slabs * n * h1 <= MH_SPLIT_MAX_FLOATS;
}
long long mh_ws_floats(int n, int d, int h1) { return (mh_split(n, d, h1) ? (long long)cdiv(d, MH_SLAB) : 1LL) * n * h1; }
int mh_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int64_t pti_mlp_head_ws_floats(int n, int d, const int32_t* dims, int n_layers) {
  const char* why;
  if (mh_check_dims(n, d, dims, n_layers, &why) != PTI_OK) return 0;
  return mh_ws_floats(n, d, dims[1]);
}

extern "C" int pti_mlp_head_fwd(const float* x, int64_t ldx, int n, int d, const float* params, const int32_t* dims,
                                int n_layers, int act, const float* mean, const float* std, const float* targets,
                                int loss_kind, float* pred, float* rowloss, float* workspace, pti_stream_t s) {
  if (!x || !params || !dims || !pred || !workspace) PTI_FAIL(PTI_EINVAL, "mlp_head_fwd: null pointer");
  if ((mean == nullptr) != (std == nullptr)) PTI_FAIL(PTI_EINVAL, "mlp_head_fwd: null pointer (mean and std go together)");
  if (targets && !rowloss) PTI_FAIL(PTI_EINVAL, "mlp_head_fwd: null pointer (rowloss is required with targets)");
  const char* why;
  const int rc = mh_check_dims(n, d, dims, n_layers, &why);
  if (rc != PTI_OK) PTI_FAIL(rc, "mlp_head_fwd: %s (n=%d d=%d layers=%d)", why, n, d, n_layers);
  if (ldx < d) PTI_FAIL(PTI_EINVAL, "mlp_head_fwd: row stride below the row length (ldx=%lld d=%d)", (long long)ldx, d);
  if (act < 0 || act > 3) PTI_FAIL(PTI_EUNSUPPORTED, "mlp_head_fwd: activation %d (0 relu, 1 gelu, 2 leaky_relu, 3 elu)", act);
  if (loss_kind != 0 && loss_kind != 1) PTI_FAIL(PTI_EUNSUPPORTED, "mlp_head_fwd: loss %d (0 mse, 1 smooth_l1)", loss_kind);
  MhFirst f;
  f.x = x;
  f.w = params;
  f.ws = workspace;
  f.ldx = ldx;
  f.n = n;
  f.d = d;
  f.h1 = dims[1];
  f.slabs = cdiv(d, MH_SLAB);
  f.split = mh_split(n, d, f.h1) ? 1 : 0;
  f.vec = mh_aligned(x) && mh_aligned(params) && ldx % 4 == 0 && d % 4 == 0;
  const dim3 grid(cdiv(n, MH_ROWS), cdiv(f.h1, MH_UNITS), f.split ? f.slabs : 1);
  PTI_LAUNCH(mlp_head_first_kernel, grid, dim3(MH_THREADS), 0, (hipStream_t)s, f);
  PTI_CHECK_LAUNCH("mlp_head_first");
  MhTail t;
  t.ws = workspace;
  t.params = params;
  t.mean = mean;
  t.std = std;
  t.targets = targets;
  t.pred = pred;
  t.rowloss = rowloss;
  for (int l = 0; l <= PTI_MLP_MAX_LAYERS; ++l) t.dims[l] = l <= n_layers ? dims[l] : 0;
  t.n_layers = n_layers;
  t.act = act;
  t.loss_kind = loss_kind;
  t.n = n;
  t.planes = f.split ? f.slabs : 1;
  PTI_LAUNCH(mlp_head_tail_kernel, dim3(cdiv(n, MH_TR)), dim3(MH_THREADS), 0, (hipStream_t)s, t);
  PTI_CHECK_LAUNCH("mlp_head_tail");
  return PTI_OK;
}

extern "C" int pti_regression_metrics(const float* pred, const float* targets, const float* rowloss, int n, int t, int batch,
                                      double* out, pti_stream_t s) {
  if (!pred || !targets || !rowloss || !out) PTI_FAIL(PTI_EINVAL, "regression_metrics: null pointer");
  if (n < 1 || t < 1 || batch < 1) PTI_FAIL(PTI_EINVAL, "regression_metrics: bad dimension n=%d t=%d batch=%d", n, t, batch);
  if (t > PTI_MLP_MAX_OUT) PTI_FAIL(PTI_EUNSUPPORTED, "regression_metrics: more than PTI_MLP_MAX_OUT targets (t=%d)", t);
  if (((uintptr_t)out & 7) != 0) PTI_FAIL(PTI_EINVAL, "regression_metrics: out must be 8-byte aligned");
  PTI_LAUNCH(regression_metrics_kernel, dim3(1), dim3(MH_THREADS), 0, (hipStream_t)s, pred, targets, rowloss, n, t, batch, out);
  PTI_CHECK_LAUNCH("regression_metrics");
  return PTI_OK;
}
