// Train-time geometric augmentation on the device: a smoothed random displacement field and ONE gather
// that applies it together with an affine inverse map.
//
// pti_elastic_field -- field[b][c] = alpha[b] * (G_sigma * n[b][c]), one launch, no workspace, no atomics.
//   The noise is never stored: n[b][c][y][x] is a counter-based hash of (key[b], c, y*W + x) (aug_noise below), so a
//   workgroup that owns a FT_H x FT_W output tile simply evaluates it on the tile plus a halo of `radius` pixels, at the
//   REFLECTED coordinate (scipy's mode="reflect": d c b a | a b c d | d c b a), into LDS; a row pass folds that into a
//   second LDS tile and a column pass folds the result into the output.  Both passes give every thread four neighbouring
//   outputs and slide an eight-float register window over the taps, four taps per trip: the row pass reads LDS as
//   16-byte pieces (conflict-free at full rate), the column pass reads one float per lane with consecutive lanes on
//   consecutive columns.  The taps come zero-padded to a multiple of four, and the LDS tiles are sized for the padded
//   window: cells beyond the halo hold hashes of coordinates nobody needs (finite numbers, no memory is read for them)
//   and meet a zero tap.
//   Every output is one fmaf chain over the taps in ascending order, first along x then along y: its bits depend on
//   (key, c, y, x, H, W, sigma) only -- not on the batch size, the sample's place in the batch or the tiling.
//   A sample with alpha == 0 is a block-uniform early exit that stores zeros.
//
// pti_augment_warp -- out[b][c][y][x] = bilinear sample of src[b][c] at M_b * (x + fx, y + fy, 1), taps outside the image
//   contribute zero.  One thread per output pixel computes the coordinate and the four tap weights once and loops over
//   the channels.  The coordinate is two fmaf chains: for a lattice map (entries 0 / +-1, integer offsets, no field)
//   every product and sum is an integer below 2^24, so the coordinate is exact, the weights are exactly 0 and 1, and the
//   source value comes through unchanged.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int FT_W = 64, FT_H = 16, FT_THREADS = 256;
constexpr int FIELD_MAX_RADIUS = PTI_ELASTIC_MAX_RADIUS;
constexpr int FIELD_MAX_TAPS = ((2 * FIELD_MAX_RADIUS + 1 + 3) / 4) * 4;   // 64

// uniform in [-1, 1): the top 24 bits of the hash as a signed fraction -- exact in fp32
__device__ __forceinline__ float aug_noise(uint32_t k0, uint32_t k1c, uint32_t i) {
  const uint32_t h = lowbias32(lowbias32(i + k0) ^ k1c);
  return (float)((int)(h >> 8) - 8388608) * (1.0f / 8388608.0f);
}
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

struct FieldArgs {
  const unsigned long long* keys;   // [B]
  const float* alpha;               // [B]
  float* field;                     // [B][2][H][W]
  int H, W, radius, nch;            // nch: trips of four taps, 4 * nch >= 2 * radius + 1
  float taps[FIELD_MAX_TAPS];       // taps[k] = weight of offset k - radius; zero from 2 * radius + 1 on
};

__global__ __launch_bounds__(FT_THREADS) void elastic_field_kernel(FieldArgs a) {
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x;
  const int b = blockIdx.z >> 1, c = blockIdx.z & 1;
  const int x0 = blockIdx.x * FT_W, y0 = blockIdx.y * FT_H;
  const int H = a.H, W = a.W, R = a.radius, nch = a.nch;
  float* plane = a.field + ((size_t)b * 2 + c) * (size_t)H * W;
  const float alpha = a.alpha[b];
  if (alpha == 0.0f) {   // block-uniform: no hash, no blur
    for (int i = tid; i < FT_H * FT_W; i += FT_THREADS) {
      const int y = y0 + i / FT_W, x = x0 + i % FT_W;
      if (y < H && x < W) plane[(size_t)y * W + x] = 0.0f;
    }
    return;
  }
  // tiles sized for the padded window: a thread's four outputs read 4 * nch + 4 consecutive cells
  const int NR = FT_H + 4 * nch, NP = FT_W + 4 * nch;
  float* noise = lds;              // [NR][NP]
  float* rowp = lds + NR * NP;     // [NR][FT_W]
  float* taps = rowp + NR * FT_W;  // [4 * nch]
  if (tid < 4 * nch) taps[tid] = a.taps[tid];
  const unsigned long long key = a.keys[b];
  const uint32_t k0 = (uint32_t)key, k1c = (uint32_t)(key >> 32) ^ ((uint32_t)c * 0x9e3779b9u);
  for (int i = tid; i < NR * NP; i += FT_THREADS) {
    const int ly = i / NP, lx = i - ly * NP;
    const int gy = reflect(y0 - R + ly, H), gx = reflect(x0 - R + lx, W);   // cells past the halo: any finite number does
    noise[i] = aug_noise(k0, k1c, (uint32_t)gy * (uint32_t)W + (uint32_t)gx);
  }
  __syncthreads();
  // row pass: item = (row ly, four outputs 4g .. 4g+3); output j sums taps[k] * noise[ly][4g + j + k]
  for (int i = tid; i < NR * (FT_W / 4); i += FT_THREADS) {
    const int ly = i / (FT_W / 4), g = i - ly * (FT_W / 4);
    const f32x4* src = (const f32x4*)(noise + ly * NP + 4 * g);
    f32x4 lo = src[0];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < nch; ++t) {
      const f32x4 hi = src[t + 1];
      const f32x4 w = *(const f32x4*)(taps + 4 * t);
      const float win[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[k], win[j + k], acc[j]);
      lo = hi;
    }
    *(f32x4*)(rowp + ly * FT_W + 4 * g) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  }
  __syncthreads();
  // column pass: thread = (column lx, four output rows 4m .. 4m+3); output j sums taps[k] * rowp[4m + j + k][lx]
  {
    const int lx = tid & (FT_W - 1), m = tid / FT_W;
    const float* src = rowp + (4 * m) * FT_W + lx;
    float lo[4] = {src[0], src[FT_W], src[2 * FT_W], src[3 * FT_W]};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < nch; ++t) {
      const float* nx = src + (4 * t + 4) * FT_W;
      const float hi[4] = {nx[0], nx[FT_W], nx[2 * FT_W], nx[3 * FT_W]};
      const f32x4 w = *(const f32x4*)(taps + 4 * t);
      const float win[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[k], win[j + k], acc[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) lo[j] = hi[j];
    }
    const int x = x0 + lx;
    if (x < W) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int y = y0 + 4 * m + j;
        if (y < H) plane[(size_t)y * W + x] = alpha * acc[j];
      }
    }
  }
}

struct WarpArgs {
  const float* src;     // [B][C][H][W]
  const float* mat;     // [B][6]
  const float* field;   // [B][2][H][W] or null
  float* out;           // [B][C][H][W]
  int C, H, W;
};

constexpr int WP_X = 64, WP_Y = 4;

__global__ __launch_bounds__(WP_X * WP_Y) void augment_warp_kernel(WarpArgs a) {
  const int x = blockIdx.x * WP_X + threadIdx.x, y = blockIdx.y * WP_Y + threadIdx.y, b = blockIdx.z;
  const int H = a.H, W = a.W;
  if (x >= W || y >= H) return;
  const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
  const float* m = a.mat + 6 * b;
  float qx = (float)x, qy = (float)y;
  if (a.field) {
    const float* f = a.field + (size_t)b * 2 * plane + pix;
    qx += f[0];
    qy += f[plane];
  }
  const float sx = fmaf(m[0], qx, fmaf(m[1], qy, m[2]));
  const float sy = fmaf(m[3], qx, fmaf(m[4], qy, m[5]));
  const float* src = a.src + (size_t)b * a.C * plane;
  float* out = a.out + (size_t)b * a.C * plane + pix;
  // all four taps outside (or a coordinate that is not a number): zero, and no float -> int conversion out of range
  if (!(sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H)) {
    for (int c = 0; c < a.C; ++c) out[c * plane] = 0.0f;
    return;
  }
  const float fx = floorf(sx), fy = floorf(sy);
  const int ix = (int)fx, iy = (int)fy;                 // -1 .. W-1, -1 .. H-1
  const float wx = sx - fx, wy = sy - fy;
  const bool x0in = ix >= 0, x1in = ix + 1 < W, y0in = iy >= 0, y1in = iy + 1 < H;
  const float w00 = (1.0f - wx) * (1.0f - wy), w01 = wx * (1.0f - wy), w10 = (1.0f - wx) * wy, w11 = wx * wy;
  const size_t o00 = (size_t)(y0in ? iy : 0) * W + (x0in ? ix : 0);   // clamped: never dereferenced when outside
  for (int c = 0; c < a.C; ++c) {
    const float* p = src + c * plane;
    const float v00 = (y0in && x0in) ? p[o00] : 0.0f;
    const float v01 = (y0in && x1in) ? p[(size_t)iy * W + ix + 1] : 0.0f;
    const float v10 = (y1in && x0in) ? p[(size_t)(iy + 1) * W + ix] : 0.0f;
    const float v11 = (y1in && x1in) ? p[(size_t)(iy + 1) * W + ix + 1] : 0.0f;
    out[c * plane] = fmaf(w11, v11, fmaf(w10, v10, fmaf(w01, v01, w00 * v00)));
  }
}

}  // namespace

extern "C" int pti_elastic_field(const uint64_t* keys, const float* alpha, float sigma, int b, int h, int w, float* field,
                                 pti_stream_t s) {
  if (!keys || !alpha || !field) PTI_FAIL(PTI_EINVAL, "elastic_field: null pointer");
  if (b < 1 || h < 1 || w < 1) PTI_FAIL(PTI_EINVAL, "elastic_field: bad dims (b %d, h %d, w %d)", b, h, w);
  if (!(sigma > 0.0f) || !(sigma < 1e6f)) PTI_FAIL(PTI_EINVAL, "elastic_field: sigma must be positive, got %g", (double)sigma);
  const int radius = (int)(4.0 * (double)sigma + 0.5);   // scipy.ndimage.gaussian_filter, truncate = 4.0
  if (radius > (h < w ? h : w))
    PTI_FAIL(PTI_EINVAL, "elastic_field: radius %d of sigma %g exceeds the image (%d x %d)", radius, (double)sigma, h, w);
  if (radius > FIELD_MAX_RADIUS)
    PTI_FAIL(PTI_EUNSUPPORTED, "elastic_field: radius %d of sigma %g above the built limit %d", radius, (double)sigma, FIELD_MAX_RADIUS);
  if (b > 32767 || (int64_t)h * w > (int64_t)1 << 30) PTI_FAIL(PTI_EUNSUPPORTED, "elastic_field: batch or image too large");
  FieldArgs a{};
  a.keys = (const unsigned long long*)keys; a.alpha = alpha; a.field = field;
  a.H = h; a.W = w; a.radius = radius; a.nch = (2 * radius + 1 + 3) / 4;
  // scipy's _gaussian_kernel1d in fp64: exp(-k^2 / 2 sigma^2) / sum, cast once
  double g[2 * FIELD_MAX_RADIUS + 1], sum = 0.0;
  for (int k = -radius; k <= radius; ++k) sum += g[k + radius] = exp(-0.5 * (double)k * k / ((double)sigma * (double)sigma));
  for (int k = 0; k <= 2 * radius; ++k) a.taps[k] = (float)(g[k] / sum);
  const int NR = FT_H + 4 * a.nch, NP = FT_W + 4 * a.nch;
  const size_t lds = (size_t)(NR * NP + NR * FT_W + 4 * a.nch) * sizeof(float);   // <= 62.7 KB at the radius limit
  PTI_LAUNCH(elastic_field_kernel, dim3(cdiv(w, FT_W), cdiv(h, FT_H), 2 * b), dim3(FT_THREADS), lds, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("elastic_field");
  return PTI_OK;
}

extern "C" int pti_augment_warp(const float* src, const float* mat, const float* field, int b, int c, int h, int w, float* out,
                                pti_stream_t s) {
  if (!src || !mat || !out) PTI_FAIL(PTI_EINVAL, "augment_warp: null pointer");
  if (b < 1 || c < 1 || h < 1 || w < 1) PTI_FAIL(PTI_EINVAL, "augment_warp: bad dims (b %d, c %d, h %d, w %d)", b, c, h, w);
  if (b > 65535 || cdiv(h, WP_Y) > 65535) PTI_FAIL(PTI_EUNSUPPORTED, "augment_warp: batch or height above the grid limit");
  const uintptr_t bytes = (uintptr_t)b * c * h * w * sizeof(float), s0 = (uintptr_t)src, o0 = (uintptr_t)out;
  if (s0 < o0 + bytes && o0 < s0 + bytes) PTI_FAIL(PTI_EINVAL, "augment_warp: out must not alias src (a gather reads what another thread writes)");
  WarpArgs a{src, mat, field, out, c, h, w};
  PTI_LAUNCH(augment_warp_kernel, dim3(cdiv(w, WP_X), cdiv(h, WP_Y), b), dim3(WP_X, WP_Y), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("augment_warp");
  return PTI_OK;
}
