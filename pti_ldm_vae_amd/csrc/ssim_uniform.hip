// Uniform-window SSIM of a ground-truth / cleaned-prediction image pair (gfx950): what the reference's
// analysis/metrics.py:420 asks of skimage.metrics.structural_similarity(gen, gt, data_range=gt.max() - gt.min()) -- a 7 x 7
// box window, sample covariance, a data range per pair, the mean over the image with a 3-pixel border cropped off.  The
// definition is in include/pti_vae.h ("uniform-window SSIM"); DESIGN.md 5q-3 has the measurements.
//
// skimage filters the whole image with mode='reflect' and then crops the border, so no padded pixel ever reaches the result:
// only the (h - 6)(w - 6) windows that lie inside the image count, and this kernel computes exactly those.
//
//   launch 1 (ssim_uniform_minmax_kernel, skipped when the caller gives the data range): grid (parts, n); every workgroup
//     writes the min and max of its slice of x into the workspace.  min and max have no rounding: any order gives the same bits.
//   launch 2 (ssim_uniform_tile_kernel): one workgroup of 256 threads per 32 x 32 tile of the VALID region of one image.
//     * wave 0 folds the image's <= 64 {min, max} partials into R and leaves C1, C2 in LDS;
//     * the tile plus its 3-pixel halo (38 x 38) of BOTH images is staged in LDS; rows and columns past the image edge (ragged
//       tiles only) are not read -- their slots hold 0 and feed no valid pixel;
//     * a thread owns four vertically adjacent valid pixels of one column: their windows cover a 10 x 7 patch of the staged
//       tile.  The box sum runs separably over that patch -- per staged row the 7-term sums of the five quantities, columns
//       ascending, then 7 of those per pixel, rows ascending -- and every row sum serves up to four pixels;
//     * the moments are taken ABOUT A PIXEL OF THE WINDOW ITSELF: (a, b) = the pair's values at row 5, column 3 of the patch,
//       which lies in all four windows; the sums are of dx = x - a, dy = y - b, dx^2, dy^2, dx dy.  Covariances do not depend
//       on the origin, ux = a + W(dx); with the raw moments an object far from zero (values near 100) loses five digits in
//       uxx - ux^2, with these the residuals are as small as the window's own spread;
//     * S per pixel in fp32 with IEEE division; the tile's sum is added in fp64 (thread: its 4 pixels top down, wave: xor
//       butterfly, workgroup: waves 0..3 in order) and stored as one double of workspace[image][tile].
//     LDS: consecutive lanes take consecutive columns, so a 32-lane group of a ds_read_b32 / ds_write_b32 touches 32
//     consecutive words of a 38-wide row: 32 banks, no conflict.  A thread reads its 70 staged pixels of both images itself
//     (140 reads; sharing the row sums through LDS took 116 reads and 24 writes per thread and ties the origin to the tile).
//   launch 3 (ssim_uniform_finalize_kernel): one wave per image adds its tiles lane-strided, then by the butterfly (fp64), and
//     writes {ssim, R}; R == 0 gives {0, 0}.
// No floating-point atomics; an image's two numbers depend on its own pixels alone, not on n or its place in the batch.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int SU_TILE = 32;                 // edge of a tile of the valid region
constexpr int SU_WIN = 7;                   // window edge
constexpr int SU_ST = SU_TILE + SU_WIN - 1; // staged edge: 38
constexpr int SU_THREADS = 256;
constexpr int SU_ROWS = 4;                  // vertically adjacent valid pixels per thread
constexpr int SU_PARTS = 64;                // {min, max} slots per image in the workspace
constexpr int SU_MIN_EDGE = SU_WIN, SU_MAX_EDGE = PTI_MASK_COMPARE_MAX_EDGE;

struct SuArgs {
  const float* x;
  const float* y;
  double* tile_sums;   // [n][tiles]
  float* mm;           // [n][SU_PARTS][2] = {min, max} of a slice of x; the first `parts` slots are used
  double* out;         // [n][2] = {ssim, R}
  double range;        // the caller's data range when parts == 0
  int h, w, tiles_x, tiles, parts;
};

__global__ __launch_bounds__(SU_THREADS) void ssim_uniform_minmax_kernel(SuArgs a) {
  __shared__ float red[2][SU_THREADS / 64];
  const int part = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
  const int npix = a.h * a.w;
  const int chunk = (npix + a.parts - 1) / a.parts;
  const int p0 = part * chunk, p1 = min(p0 + chunk, npix);   // never empty: parts <= cdiv(npix, 4096)
  const float* __restrict__ x = a.x + (size_t)img * npix;
  float mn = INFINITY, mx = -INFINITY;
  for (int p = p0 + tid; p < p1; p += SU_THREADS) {
    const float v = x[p];
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int wv = 1; wv < SU_THREADS / 64; ++wv) {
      mn = red[0][wv] < mn ? red[0][wv] : mn;
      mx = red[1][wv] > mx ? red[1][wv] : mx;
    }
    float* o = a.mm + ((size_t)img * SU_PARTS + part) * 2;
    o[0] = mn;
    o[1] = mx;
  }
}

// R of one image, by one whole wave (every lane returns it): the caller's value, or max - min of the partials in fp64
__device__ __forceinline__ double su_range(const SuArgs& a, int img, int lane) {
  if (a.parts == 0) return a.range;
  float mn = INFINITY, mx = -INFINITY;
  if (lane < a.parts) {
    const float* m = a.mm + ((size_t)img * SU_PARTS + lane) * 2;
    mn = m[0];
    mx = m[1];
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  return (double)mx - (double)mn;
}

__global__ __launch_bounds__(SU_THREADS) void ssim_uniform_tile_kernel(SuArgs a) {
#pragma clang fp reassociate(off)
  __shared__ float sx[SU_ST * SU_ST];
  __shared__ float sy[SU_ST * SU_ST];
  __shared__ double red[SU_THREADS / 64];
  __shared__ float cc[2];

  const int tid = threadIdx.x;
  const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
  const int ty0 = (tile / a.tiles_x) * SU_TILE, tx0 = (tile % a.tiles_x) * SU_TILE;   // valid pixel (r, q) = window rows r .. r + 6
  const float* __restrict__ px = a.x + (size_t)img * a.h * a.w;
  const float* __restrict__ py = a.y + (size_t)img * a.h * a.w;

  if (tid < 64) {
    const double R = su_range(a, img, tid);
    if (tid == 0) {
      cc[0] = (float)((0.01 * R) * (0.01 * R));
      cc[1] = (float)((0.03 * R) * (0.03 * R));
    }
  }

  // ---- stage the tile and its halo: staged (r, c) is image pixel (ty0 + r, tx0 + c) ----
  for (int i = tid; i < SU_ST * SU_ST; i += SU_THREADS) {
    const int r = i / SU_ST, c = i - r * SU_ST;
    const int gy = ty0 + r, gx = tx0 + c;
    float vx = 0.f, vy = 0.f;
    if (gy < a.h && gx < a.w) {
      const size_t o = (size_t)gy * a.w + gx;
      vx = px[o];
      vy = py[o];
    }
    sx[i] = vx;
    sy[i] = vy;
  }
  __syncthreads();

  // ---- the thread's patch: column c, valid rows r0 .. r0 + 3 -> staged rows r0 .. r0 + 9, columns c .. c + 6 ----
  const int c = tid % SU_TILE, r0 = (tid / SU_TILE) * SU_ROWS;
  const int org = (r0 + 5) * SU_ST + c + 3;       // in all four windows; inside the image whenever one of them is valid
  const float oa = sx[org], ob = sy[org];
  float e[SU_ROWS][5];
#pragma unroll
  for (int j = 0; j < SU_WIN + SU_ROWS - 1; ++j) {
    const float* rx = sx + (r0 + j) * SU_ST + c;
    const float* ry = sy + (r0 + j) * SU_ST + c;
    float v[5];   // the row's sums of dx, dy, dx^2, dy^2, dx dy, columns ascending
#pragma unroll
    for (int k = 0; k < SU_WIN; ++k) {
      const float dx = rx[k] - oa, dy = ry[k] - ob;
      if (k == 0) {
        v[0] = dx; v[1] = dy; v[2] = dx * dx; v[3] = dy * dy; v[4] = dx * dy;
      } else {
        v[0] += dx; v[1] += dy; v[2] += dx * dx; v[3] += dy * dy; v[4] += dx * dy;
      }
    }
#pragma unroll
    for (int o = 0; o < SU_ROWS; ++o) {
      const int k = j - o;   // staged row r0 + j is row k of pixel o's window: rows ascending per pixel
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        if (k == 0) e[o][q] = v[q];
        else if (k > 0 && k < SU_WIN) e[o][q] += v[q];
      }
    }
  }

  const float c1 = cc[0], c2 = cc[1];
  const float inv = 1.0f / 49.0f, cn = 49.0f / 48.0f;
  double s = 0.0;
#pragma unroll
  for (int o = 0; o < SU_ROWS; ++o) {
    if (ty0 + r0 + o < a.h - (SU_WIN - 1) && tx0 + c < a.w - (SU_WIN - 1)) {
      const float mx = e[o][0] * inv, my = e[o][1] * inv;            // means of dx, dy
      const float ux = oa + mx, uy = ob + my;
      const float vx = cn * (e[o][2] * inv - mx * mx), vy = cn * (e[o][3] * inv - my * my), vxy = cn * (e[o][4] * inv - mx * my);
      const float num = (2.f * ux * uy + c1) * (2.f * vxy + c2);
      const float den = (ux * ux + uy * uy + c1) * (vx + vy + c2);
      s += (double)__fdiv_rn(num, den);
    }
  }

  // ---- tile sum, fp64, fixed order: butterfly inside the wave, waves 0..3 in order ----
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
#pragma unroll
    for (int wv = 1; wv < SU_THREADS / 64; ++wv) t += red[wv];
    a.tile_sums[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void ssim_uniform_finalize_kernel(SuArgs a) {
#pragma clang fp reassociate(off)
  const int img = blockIdx.x, lane = threadIdx.x;
  const double R = su_range(a, img, lane);
  const double* p = a.tile_sums + (size_t)img * a.tiles;
  double s = 0.0;
  for (int t = lane; t < a.tiles; t += 64) s += p[t];
  s = wave_sum(s);
  if (lane == 0) {
    const double count = (double)(a.h - (SU_WIN - 1)) * (double)(a.w - (SU_WIN - 1));
    a.out[2 * (size_t)img] = R == 0.0 ? 0.0 : s / count;   // a flat ground truth: skimage's 0 / 0, reported as "none" by the host
    a.out[2 * (size_t)img + 1] = R;
  }
}

inline bool su_edges_ok(int h, int w) { return h >= SU_MIN_EDGE && w >= SU_MIN_EDGE && h <= SU_MAX_EDGE && w <= SU_MAX_EDGE; }
inline int su_tiles_x(int w) { return cdiv(w - (SU_WIN - 1), SU_TILE); }
inline long long su_tiles(int h, int w) { return (long long)cdiv(h - (SU_WIN - 1), SU_TILE) * su_tiles_x(w); }   // <= 1024
inline int su_parts(int h, int w) { return min(SU_PARTS, max(1, cdiv(h * w, 4096))); }

}  // namespace

extern "C" int64_t pti_ssim_uniform_ws_bytes(int n, int h, int w) {
  if (n < 1 || n > 65535 || !su_edges_ok(h, w)) return 0;
  return (int64_t)n * su_tiles(h, w) * (int64_t)sizeof(double) + (int64_t)n * SU_PARTS * 2 * (int64_t)sizeof(float);
}

extern "C" int pti_ssim_uniform(const float* x, const float* y, int n, int h, int w, double data_range, double* out,
                                void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!x || !y || !out || !workspace) PTI_FAIL(PTI_EINVAL, "ssim_uniform: null pointer");
  if (n < 1) PTI_FAIL(PTI_EINVAL, "ssim_uniform: bad batch n=%d (n >= 1)", n);
  if (!su_edges_ok(h, w))
    PTI_FAIL(PTI_EUNSUPPORTED, "ssim_uniform: unsupported shape h=%d w=%d (%d <= h, w <= %d)", h, w, SU_MIN_EDGE, SU_MAX_EDGE);
  if (n > 65535) PTI_FAIL(PTI_EUNSUPPORTED, "ssim_uniform: unsupported batch n=%d (n <= 65535)", n);
  if (data_range != data_range) PTI_FAIL(PTI_EINVAL, "ssim_uniform: data_range is NaN");
  if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)out & 7)) PTI_FAIL(PTI_EINVAL, "ssim_uniform: misaligned buffer");
  if ((uintptr_t)workspace & 7) PTI_FAIL(PTI_EINVAL, "ssim_uniform: workspace must be 8-byte aligned");
  if (ws_bytes < pti_ssim_uniform_ws_bytes(n, h, w))
    PTI_FAIL(PTI_EINVAL, "ssim_uniform: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
             (long long)pti_ssim_uniform_ws_bytes(n, h, w));
  SuArgs a;
  a.x = x;
  a.y = y;
  a.tile_sums = (double*)workspace;
  a.tiles_x = su_tiles_x(w);
  a.tiles = (int)su_tiles(h, w);
  a.mm = (float*)(a.tile_sums + (size_t)n * a.tiles);
  a.out = out;
  a.h = h;
  a.w = w;
  a.parts = data_range < 0.0 ? su_parts(h, w) : 0;
  a.range = data_range < 0.0 ? 0.0 : data_range;
  if (a.parts) {
    PTI_LAUNCH(ssim_uniform_minmax_kernel, dim3((unsigned)a.parts, (unsigned)n), dim3(SU_THREADS), 0, (hipStream_t)s, a);
    PTI_CHECK_LAUNCH("ssim_uniform_minmax");
  }
  PTI_LAUNCH(ssim_uniform_tile_kernel, dim3((unsigned)(n * a.tiles)), dim3(SU_THREADS), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("ssim_uniform_tile");
  PTI_LAUNCH(ssim_uniform_finalize_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("ssim_uniform_finalize");
  return PTI_OK;
}
