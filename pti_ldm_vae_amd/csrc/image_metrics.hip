// Fused image-quality metrics of the evaluation path (gfx950): per-sample MSE, MAE, PSNR and SSIM of a pair of fp32 NCHW
// image batches in one pass over the pixels.
//
// Stands in for what the reference's vae_scripts/evaluate_vae.py:87-99 does per batch with torch ops: clamp both images,
// compute_psnr / compute_ssim (src/pti_ldm_vae/utils/eval_metrics.py:6-64) and the two plain means -- five 11x11
// conv2d calls plus a dozen elementwise kernels, each of which streams the full images through HBM again.
//
//   pass 1 (image_metrics_tile_kernel): one workgroup per 32x32 output tile of one (sample, channel) plane.
//     * the tile + a 5-pixel halo of BOTH images is staged into LDS (42x42 each) with the optional clamp applied; pixels
//       outside the image are ZERO (conv2d's zero padding, no renormalisation at the border);
//     * the 11-tap Gaussian runs separably: a row pass writes the five filtered quantities x, y, x^2, y^2, xy of the 42
//       staged rows into LDS, a column pass (four vertically adjacent pixels per thread, 14 LDS reads per quantity for
//       44 multiply-adds) finishes E[.];
//     * per pixel: sigma = E[.] - mu^2, the SSIM map value (IEEE division), (x-y)^2 and |x-y|;
//     * the three sums of the tile are reduced in fp64 through wavefront shuffles and LDS (fixed order) and stored --
//       plain vector stores -- as three floats of `workspace[plane][tile]`.
//   pass 2 (image_metrics_finalize_kernel): one wavefront per sample adds its c * tiles partial rows in a fixed order
//     (fp64), divides by c*h*w and writes {mse, mae, psnr, ssim}.
// No floating-point atomics: two runs are bitwise equal, and a sample's four numbers do not depend on the batch it is
// evaluated in or on its position there (its planes' arithmetic never looks at n).
//
// Precision: everything per pixel is fp32 like the reference (whose conv2d also accumulates in fp32); only the ORDER of
// the 121 products differs (separable).  The means over up to c*h*w pixels are accumulated in fp64 so that the result
// carries the per-pixel rounding only; PSNR's log10 is taken in fp64 from that mean.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int IM_TILE = 32;               // output tile edge
constexpr int IM_R = 5;                   // window radius (11 taps)
constexpr int IM_TAPS = 2 * IM_R + 1;
constexpr int IM_ST = IM_TILE + 2 * IM_R; // staged edge: 42
constexpr int IM_THREADS = 256;
constexpr int IM_ROWS_PER_THREAD = 4;     // column pass: IM_TILE * IM_TILE / IM_THREADS

struct ImTaps { float g[IM_TAPS]; };

struct ImArgs {
  const float* pred;
  const float* target;
  float* workspace;     // [n*c][tiles][3] = per-tile {sum (x-y)^2, sum |x-y|, sum ssim}
  int h, w, tiles_x, tiles;
  int clamp;
  float lo, hi, c1, c2;
  ImTaps taps;
};

__global__ __launch_bounds__(IM_THREADS) void image_metrics_tile_kernel(ImArgs a) {
  __shared__ float sx[IM_ST * IM_ST];
  __shared__ float sy[IM_ST * IM_ST];
  __shared__ float rp[5][IM_ST][IM_TILE];   // row-pass outputs: x, y, xx, yy, xy
  __shared__ double red[IM_THREADS / 64][3];

  const int tid = threadIdx.x;
  const long long plane = blockIdx.x / a.tiles;
  const int tile = blockIdx.x % a.tiles;
  const int ty0 = (tile / a.tiles_x) * IM_TILE, tx0 = (tile % a.tiles_x) * IM_TILE;
  const float* __restrict__ px = a.pred + plane * (long long)a.h * a.w;
  const float* __restrict__ py = a.target + plane * (long long)a.h * a.w;

  // ---- stage tile + halo (zero outside the image; clamp inside it) ----
  for (int i = tid; i < IM_ST * IM_ST; i += IM_THREADS) {
    const int r = i / IM_ST, c = i - r * IM_ST;
    const int gy = ty0 + r - IM_R, gx = tx0 + c - IM_R;
    float vx = 0.f, vy = 0.f;
    if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
      const long long o = (long long)gy * a.w + gx;
      vx = px[o];
      vy = py[o];
      if (a.clamp) {
        vx = fminf(fmaxf(vx, a.lo), a.hi);
        vy = fminf(fmaxf(vy, a.lo), a.hi);
      }
    }
    sx[i] = vx;
    sy[i] = vy;
  }
  __syncthreads();

  // ---- row pass: 42 rows x 32 columns, five quantities ----
  for (int i = tid; i < IM_ST * IM_TILE; i += IM_THREADS) {
    const int r = i / IM_TILE, c = i % IM_TILE;
    const float* rx = sx + r * IM_ST + c;
    const float* ry = sy + r * IM_ST + c;
    float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
    for (int k = 0; k < IM_TAPS; ++k) {
      const float g = a.taps.g[k], x = rx[k], y = ry[k];
      ax = fmaf(g, x, ax);
      ay = fmaf(g, y, ay);
      axx = fmaf(g, x * x, axx);
      ayy = fmaf(g, y * y, ayy);
      axy = fmaf(g, x * y, axy);
    }
    rp[0][r][c] = ax;
    rp[1][r][c] = ay;
    rp[2][r][c] = axx;
    rp[3][r][c] = ayy;
    rp[4][r][c] = axy;
  }
  __syncthreads();

  // ---- column pass: thread = column c, rows r0 .. r0+3 ----
  const int c = tid % IM_TILE, r0 = (tid / IM_TILE) * IM_ROWS_PER_THREAD;
  float e[IM_ROWS_PER_THREAD][5];
#pragma unroll
  for (int o = 0; o < IM_ROWS_PER_THREAD; ++o)
#pragma unroll
    for (int q = 0; q < 5; ++q) e[o][q] = 0.f;
#pragma unroll
  for (int j = 0; j < IM_TAPS + IM_ROWS_PER_THREAD - 1; ++j) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const float v = rp[q][r0 + j][c];
#pragma unroll
      for (int o = 0; o < IM_ROWS_PER_THREAD; ++o) {
        const int k = j - o;   // tap index of staged row r0+j for output row r0+o (ascending k per output: fixed order)
        if (k >= 0 && k < IM_TAPS) e[o][q] = fmaf(a.taps.g[k], v, e[o][q]);
      }
    }
  }

  float s_sq = 0.f, s_ab = 0.f, s_ss = 0.f;
#pragma unroll
  for (int o = 0; o < IM_ROWS_PER_THREAD; ++o) {
    const int gy = ty0 + r0 + o, gx = tx0 + c;
    if (gy < a.h && gx < a.w) {
      const float mx = e[o][0], my = e[o][1];
      const float mxx = mx * mx, myy = my * my, mxy = mx * my;
      const float vx = e[o][2] - mxx, vy = e[o][3] - myy, vxy = e[o][4] - mxy;
      const float num = (2.f * mxy + a.c1) * (2.f * vxy + a.c2);
      const float den = (mxx + myy + a.c1) * (vx + vy + a.c2);
      s_ss += __fdiv_rn(num, den);
      const float d = sx[(r0 + o + IM_R) * IM_ST + c + IM_R] - sy[(r0 + o + IM_R) * IM_ST + c + IM_R];
      s_sq = fmaf(d, d, s_sq);
      s_ab += fabsf(d);
    }
  }

  // ---- tile reduction, fp64, fixed order: shuffles inside the wave, waves 0..3 in order ----
  const double w_sq = wave_sum((double)s_sq), w_ab = wave_sum((double)s_ab), w_ss = wave_sum((double)s_ss);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = w_sq;
    red[tid >> 6][1] = w_ab;
    red[tid >> 6][2] = w_ss;
  }
  __syncthreads();
  if (tid < 3) {
    double t = red[0][tid];
#pragma unroll
    for (int wv = 1; wv < IM_THREADS / 64; ++wv) t += red[wv][tid];
    a.workspace[((long long)blockIdx.x) * 3 + tid] = (float)t;
  }
}

// one wavefront per sample: rows = c * tiles partial rows of 3 floats, added lane-strided then by shuffles (fixed order)
__global__ __launch_bounds__(64) void image_metrics_finalize_kernel(const float* __restrict__ workspace, float* __restrict__ out_n4,
                                                                    int rows, double inv_count, double range_sq) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* p = workspace + (long long)n * rows * 3;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int r = lane; r < rows; r += 64) {
    s0 += (double)p[3 * r];
    s1 += (double)p[3 * r + 1];
    s2 += (double)p[3 * r + 2];
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    const double mse = s0 * inv_count;
    float* o = out_n4 + 4 * (long long)n;
    o[0] = (float)mse;
    o[1] = (float)(s1 * inv_count);
    o[2] = (float)(10.0 * log10(range_sq / fmax(mse, 1e-12)));
    o[3] = (float)(s2 * inv_count);
  }
}

// 0 when the shape is not supported: a non-positive dimension, or more workgroups / elements than the launch can index
long long im_tiles(int h, int w) { return (long long)cdiv(h, IM_TILE) * cdiv(w, IM_TILE); }
long long im_ws_floats(int n, int c, int h, int w) {
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return 0;
  if (h > (1 << 24) || w > (1 << 24)) return 0;
  const long long tiles = im_tiles(h, w);
  const long long planes = (long long)n * c;
  if (tiles > 0x7fffffffLL / 3 / c) return 0;            // rows of one sample * 3 must fit an int
  if (planes * tiles > 0x7fffffffLL) return 0;           // grid size
  return planes * tiles * 3;
}

}  // namespace

extern "C" int64_t pti_image_metrics_ws_floats(int n, int c, int h, int w) { return im_ws_floats(n, c, h, w); }

extern "C" int pti_image_metrics(const float* pred, const float* target, int n, int c, int h, int w, int clamp, float lo,
                                 float hi, float data_range, float k1, float k2, const float* taps11, float* out_n4,
                                 float* workspace, pti_stream_t s) {
  if (!pred || !target || !taps11 || !out_n4 || !workspace) PTI_FAIL(PTI_EINVAL, "image_metrics: null pointer");
  if (im_ws_floats(n, c, h, w) == 0) PTI_FAIL(PTI_EUNSUPPORTED, "image_metrics: unsupported shape n=%d c=%d h=%d w=%d", n, c, h, w);
  if (clamp && !(lo <= hi)) PTI_FAIL(PTI_EUNSUPPORTED, "image_metrics: clamp range [%g, %g] is empty", (double)lo, (double)hi);
  ImArgs a;
  a.pred = pred;
  a.target = target;
  a.workspace = workspace;
  a.h = h;
  a.w = w;
  a.tiles_x = cdiv(w, IM_TILE);
  a.tiles = (int)im_tiles(h, w);
  a.clamp = clamp ? 1 : 0;
  a.lo = lo;
  a.hi = hi;
  a.c1 = (float)(((double)k1 * data_range) * ((double)k1 * data_range));
  a.c2 = (float)(((double)k2 * data_range) * ((double)k2 * data_range));
  for (int k = 0; k < IM_TAPS; ++k) a.taps.g[k] = taps11[k];   // host array: travels as a kernel argument
  const long long blocks = (long long)n * c * a.tiles;
  PTI_LAUNCH(image_metrics_tile_kernel, dim3((unsigned)blocks), dim3(IM_THREADS), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("image_metrics");
  const double count = (double)c * (double)h * (double)w;
  PTI_LAUNCH(image_metrics_finalize_kernel, dim3(n), dim3(64), 0, (hipStream_t)s, (const float*)workspace, out_n4,
             c * a.tiles, 1.0 / count, (double)data_range * (double)data_range);
  PTI_CHECK_LAUNCH("image_metrics_finalize");
  return PTI_OK;
}
