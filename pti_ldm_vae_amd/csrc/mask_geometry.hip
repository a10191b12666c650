// Mask geometry behind the AR-VAE attribute files (reference vae_scripts/compute_mask_metrics.py:38-68,176-193): for a
// batch of binary masks of mixed size, the bounding box of all foreground pixels and the width
// (last foreground column - first + 1) of a few chosen rows, in ONE launch.
//   - one workgroup per image; each wave64 takes rows round-robin; lanes stride the row's 16-byte pieces (scalar head up
//     to the first 16-byte boundary and scalar tail behind the last whole piece: offsets promise no alignment);
//   - a lane keeps the first / last foreground column it saw, a shuffle min/max folds the wave, lane 0 stores the row's
//     {first, last} into an LDS table (8 bytes x MASK_ROW_CAP rows = 32 KB);
//   - after a barrier the workgroup folds the bounding box from that table, and threads k < samples + n_bottom look
//     their row up and store its width.
// The workgroup is 1024 threads, not 256: a 512-pixel uint8 row is 32 pieces -- one load per wave and row -- and the
// default batch of 64 images is 64 workgroups on 256 CUs, so waves in flight are what hides the load latency.
// No atomics, no workspace, integers only: bitwise reproducible and independent of the image's place in the batch.
// The rows sampled inside the bounding box come from a caller-built table (see include/pti_vae.h): this library is built
// with -ffast-math and numpy's linspace truncates a float64 product, so nothing here recomputes it.
#include <limits.h>

#include "pti_common.h"

namespace {

constexpr int MASK_ROW_CAP = 4096;   // documented in include/pti_vae.h
constexpr int MASK_THREADS = 1024;
constexpr int MASK_WAVES = MASK_THREADS / 64;

struct MaskArgs {
  const void* src;
  const long long* offset;   // [B] element offset of image b
  const int* hw;             // [B][2] height, width
  const int* sample_rows;    // [max_h + 1][samples]
  const int* bottom_offsets; // [n_bottom]
  int* bbox;                 // [B][4]
  int* bbox_widths;          // [B][samples]
  int* bottom_widths;        // [B][n_bottom]
  int max_h, samples, n_bottom;
};

template <int ELEM> struct MaskElem;
template <> struct MaskElem<0> { typedef uint8_t T; };
template <> struct MaskElem<1> { typedef uint16_t T; };
template <> struct MaskElem<2> { typedef uint32_t T; };   // float32 is tested by its bit pattern

// IEEE x > 0 on the bits: independent of the denormal mode, NaN / -0.0 / negatives are background
__device__ __forceinline__ bool f32_bits_fg(uint32_t u) { return (int)u > 0 && u <= 0x7f800000u; }

template <int ELEM>
__device__ __forceinline__ bool elem_fg(typename MaskElem<ELEM>::T v) {
  if (ELEM == 2) return f32_bits_fg((uint32_t)v);
  return v != 0;
}

// first / last foreground element of one 16-byte piece whose first element is column c0
template <int ELEM>
__device__ __forceinline__ void piece_extent(const u32x4& p, int c0, int& lo, int& hi) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t d = p[k];
    if (ELEM == 2) {
      if (f32_bits_fg(d)) { lo = min(lo, c0 + k); hi = max(hi, c0 + k); }
    } else {
      // little endian: the lowest set bit of the dword lies in its first non-zero element, the highest in its last
      constexpr int BITS = ELEM == 0 ? 8 : 16, PER = 32 / BITS;
      if (d != 0) {
        lo = min(lo, c0 + k * PER + (__builtin_ctz(d) / BITS));
        hi = max(hi, c0 + k * PER + ((31 - __builtin_clz(d)) / BITS));
      }
    }
  }
}

template <int ELEM>
__global__ __launch_bounds__(MASK_THREADS) void mask_geometry_kernel(MaskArgs a) {
  typedef typename MaskElem<ELEM>::T T;
  constexpr int ES = (int)sizeof(T), EPV = 16 / ES;   // element size, elements per 16-byte piece
  __shared__ int2 rows[MASK_ROW_CAP];                 // {first, last} foreground column of every row
  __shared__ int red[4][MASK_WAVES];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.hw[2 * img], W = a.hw[2 * img + 1];
  int* bw = a.bbox_widths + (size_t)img * a.samples;
  int* tw = a.bottom_widths + (size_t)img * a.n_bottom;
  if (H < 1 || W < 1 || H > a.max_h) {   // block-uniform: a bad descriptor is reported, never read
    if (tid < 4) a.bbox[4 * img + tid] = tid < 2 ? -2 : 0;
    for (int k = tid; k < a.samples; k += MASK_THREADS) bw[k] = 0;
    for (int k = tid; k < a.n_bottom; k += MASK_THREADS) tw[k] = 0;
    return;
  }
  const T* base = (const T*)a.src + a.offset[img];

  for (int r = wave; r < H; r += MASK_WAVES) {
    const T* row = base + (size_t)r * W;
    int lo = INT_MAX, hi = -1;
    const int to_boundary = (int)((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / ES;
    const int head = min(W, to_boundary);     // < 16 elements in front of the first 16-byte boundary
    const int nvec = (W - head) / EPV;
    const int tail0 = head + nvec * EPV;      // W - tail0 < EPV elements behind the last whole piece
    if (lane < head && elem_fg<ELEM>(row[lane])) lo = hi = lane;
    const u32x4* vrow = (const u32x4*)(row + head);
    for (int v = lane; v < nvec; v += 64) piece_extent<ELEM>(vrow[v], head + v * EPV, lo, hi);
    if (tail0 + lane < W && elem_fg<ELEM>(row[tail0 + lane])) { lo = min(lo, tail0 + lane); hi = max(hi, tail0 + lane); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) rows[r] = make_int2(lo, hi);
  }
  __syncthreads();

  // bounding box: min / max over the row table
  int x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
  for (int r = tid; r < H; r += MASK_THREADS) {
    const int2 e = rows[r];
    if (e.y >= 0) {
      x0 = min(x0, e.x); x1 = max(x1, e.y);
      y0 = min(y0, r);   y1 = max(y1, r);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x0 = min(x0, __shfl_xor(x0, o, 64)); x1 = max(x1, __shfl_xor(x1, o, 64));
    y0 = min(y0, __shfl_xor(y0, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
  }
  if (lane == 0) { red[0][wave] = x0; red[1][wave] = x1; red[2][wave] = y0; red[3][wave] = y1; }
  __syncthreads();
  x0 = red[0][0]; x1 = red[1][0]; y0 = red[2][0]; y1 = red[3][0];
#pragma unroll
  for (int w = 1; w < MASK_WAVES; ++w) {
    x0 = min(x0, red[0][w]); x1 = max(x1, red[1][w]);
    y0 = min(y0, red[2][w]); y1 = max(y1, red[3][w]);
  }
  const bool empty = y1 < 0;
  const int bh = empty ? 0 : y1 - y0 + 1;
  if (tid == 0) {
    int* o = a.bbox + 4 * img;
    o[0] = empty ? -1 : x0; o[1] = empty ? -1 : y0; o[2] = empty ? 0 : x1 - x0 + 1; o[3] = bh;
  }
  for (int k = tid; k < a.samples; k += MASK_THREADS) {
    int wdt = 0;
    if (!empty) {   // bh <= H <= max_h: inside the table
      const long long r = (long long)y0 + a.sample_rows[(size_t)bh * a.samples + k];
      if (r >= 0 && r < H) { const int2 e = rows[(int)r]; wdt = e.y >= 0 ? e.y - e.x + 1 : 0; }
    }
    bw[k] = wdt;
  }
  for (int k = tid; k < a.n_bottom; k += MASK_THREADS) {
    long long r = (long long)(H - 1) - a.bottom_offsets[k];
    r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
    const int2 e = rows[(int)r];
    tw[k] = e.y >= 0 ? e.y - e.x + 1 : 0;
  }
}

}  // namespace

extern "C" int pti_mask_geometry(const void* src, const int64_t* offsets, const int32_t* hw, int b, int elem, int max_h,
                                 const int32_t* sample_rows, int samples, const int32_t* bottom_offsets, int n_bottom,
                                 int32_t* bbox_b4, int32_t* bbox_widths, int32_t* bottom_widths, pti_stream_t s) {
  if (!src || !offsets || !hw || !bbox_b4) PTI_FAIL(PTI_EINVAL, "mask_geometry: null pointer");
  if (b < 1 || samples < 0 || n_bottom < 0 || max_h < 0) PTI_FAIL(PTI_EUNSUPPORTED, "mask_geometry: bad counts (b %d, samples %d, n_bottom %d, max_h %d)", b, samples, n_bottom, max_h);
  if (elem < 0 || elem > 2) PTI_FAIL(PTI_EUNSUPPORTED, "mask_geometry: unknown elem %d (0 uint8, 1 uint16, 2 float32)", elem);
  if (max_h > MASK_ROW_CAP) PTI_FAIL(PTI_EUNSUPPORTED, "mask_geometry: max_h %d above the row cap %d", max_h, MASK_ROW_CAP);
  if (samples > 0 && (!sample_rows || !bbox_widths)) PTI_FAIL(PTI_EINVAL, "mask_geometry: null pointer (samples > 0 needs sample_rows and bbox_widths)");
  if (n_bottom > 0 && (!bottom_offsets || !bottom_widths)) PTI_FAIL(PTI_EINVAL, "mask_geometry: null pointer (n_bottom > 0 needs bottom_offsets and bottom_widths)");
  if ((uintptr_t)src & (uintptr_t)((1 << elem) - 1)) PTI_FAIL(PTI_EINVAL, "mask_geometry: src is not aligned to its element size");
  MaskArgs a{src, (const long long*)offsets, hw, sample_rows, bottom_offsets, bbox_b4, bbox_widths, bottom_widths,
             max_h, samples, n_bottom};
  hipStream_t st = (hipStream_t)s;
  if (elem == 0) PTI_LAUNCH(mask_geometry_kernel<0>, dim3(b), dim3(MASK_THREADS), 0, st, a);
  else if (elem == 1) PTI_LAUNCH(mask_geometry_kernel<1>, dim3(b), dim3(MASK_THREADS), 0, st, a);
  else PTI_LAUNCH(mask_geometry_kernel<2>, dim3(b), dim3(MASK_THREADS), 0, st, a);
  PTI_CHECK_LAUNCH("mask_geometry");
  return PTI_OK;
}
