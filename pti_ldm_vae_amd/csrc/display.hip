// Display normalisation of image planes on the device (gfx950): the arithmetic of the reference's
// normalize_batch_for_display (src/pti_ldm_vae/utils/visualization.py:6-40) -- per plane, the NON-ZERO pixels are mapped
// linearly from their low .. high percentile to 0 .. 1, clipped, floored at 1e-3 -- plus the quarter-turn rotation and the
// side-by-side canvas [input | reconstruction | |difference|] that train_vae.py:536-549,610-626 builds around it.  The
// host version copies every plane to the CPU and sorts its foreground (np.percentile); here nothing leaves the device.
//
// One workgroup per (image, source) plane, no workspace, no cross-workgroup traffic, no global atomics.  A 256 x 256
// plane is 256 KiB -- more than the LDS -- so the plane is re-read (from L2 after the first touch) five times:
//   passes 0..3: MSB-first radix SELECT, 8 bits per pass, on the order-preserving 32-bit key of the float (sign bit
//     flipped for positives, all bits for negatives).  Each wave counts into its own LDS histogram (LDS atomics contend
//     inside one wave only), the waves' tables are summed, and one wave per wanted rank scans the 256 bins with
//     shuffles and narrows its (prefix, rank inside the prefix).  Pass 0 counts every foreground pixel, so its total is
//     n and no separate counting pass is needed.  All four ranks -- floor and ceiling position of both percentiles --
//     ride the same passes: ranks that still share a prefix share a histogram slot, so the usual cost is one or two
//     slots, four at the most.  The select returns VALUES, not positions: ties need no care.
//   pass 4: map, rotate, store (fp32 and / or 8-bit), iterating over OUTPUT pixels so that stores are contiguous.
// Exact: n, the four order statistics.  fp64: the linear interpolation (numpy's "linear" method) and the map
// (v - p_low) / (p_high - p_low + 1e-8); the result is rounded to fp32 once, then floored / truncated to 8 bits.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int DP_THREADS = 512;
constexpr int DP_WAVES = DP_THREADS / 64;
constexpr int DP_RANKS = 4;    // lo / hi position of p_low, lo / hi position of p_high
constexpr int DP_BINS = 256;   // 8 bits per select pass

struct DpArgs {
  const float* a;
  const float* b;
  float* out_f32;
  uint8_t* out_u8;
  double* stats;   // [planes][3] = {n, p_low, p_high}
  int h, w, nsrc, rot_k;
  int vec4;        // h * w % 4 == 0 and a, b 16-byte aligned: every plane can be read as float4
  double low, high;
};

// ascending float order == ascending unsigned order of the key
__device__ __forceinline__ uint32_t dp_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dp_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// value `i` of the plane: source 0 = a, 1 = b, 2 = |a - b| in fp32
__device__ __forceinline__ float dp_value(const float* __restrict__ pa, const float* __restrict__ pb, int src, int i) {
  if (src == 0) return pa[i];
  if (src == 1) return pb[i];
  return fabsf(pa[i] - pb[i]);
}

__device__ __forceinline__ f32x4 dp_value4(const float* __restrict__ pa, const float* __restrict__ pb, int src, int i) {
  if (src == 0) return *(const f32x4*)(pa + i);
  if (src == 1) return *(const f32x4*)(pb + i);
  const f32x4 va = *(const f32x4*)(pa + i), vb = *(const f32x4*)(pb + i);
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = fabsf(va[k] - vb[k]);
  return v;
}

__device__ __forceinline__ void dp_count(uint32_t (*wh)[DP_BINS], float v, int np, const uint32_t* uniq, uint32_t mask,
                                         int shift) {
  if (v != 0.0f) {   // -0.0 compares equal to 0: background
    const uint32_t key = dp_key(v);
    const uint32_t bin = (key >> shift) & (DP_BINS - 1);
#pragma unroll
    for (int j = 0; j < DP_RANKS; ++j)
      if (j < np && (key & mask) == uniq[j]) atomicAdd(&wh[j][bin], 1u);
  }
}

__global__ __launch_bounds__(DP_THREADS) void display_planes_kernel(DpArgs g) {
  __shared__ __attribute__((aligned(16))) uint32_t wave_hist[DP_WAVES][DP_RANKS][DP_BINS];
  __shared__ __attribute__((aligned(16))) uint32_t hist[DP_RANKS][DP_BINS];
  __shared__ uint32_t s_prefix[DP_RANKS];   // key bits fixed so far (in place, low bits 0)
  __shared__ uint32_t s_rank[DP_RANKS];     // 0-based rank among the keys that share the prefix
  __shared__ uint32_t s_uniq[DP_RANKS];     // the distinct prefixes = histogram slots of the next pass
  __shared__ int s_slot[DP_RANKS];
  __shared__ int s_np;
  __shared__ uint32_t s_n;
  __shared__ double s_gamma[2];
  __shared__ double s_p[2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = blockIdx.x, img = plane / g.nsrc, src = plane - img * g.nsrc;
  const int hw = g.h * g.w;   // <= 2^24
  const float* __restrict__ pa = g.a + (long long)img * hw;
  const float* __restrict__ pb = g.b ? g.b + (long long)img * hw : nullptr;

  if (tid < DP_RANKS) {
    s_prefix[tid] = 0;
    s_uniq[tid] = 0;
    s_slot[tid] = 0;
  }
  if (tid == 0) s_np = 1;
  __syncthreads();

  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    const int np = s_np;
    uint32_t uniq[DP_RANKS];
#pragma unroll
    for (int j = 0; j < DP_RANKS; ++j) uniq[j] = s_uniq[j];
    for (int i = tid; i < DP_WAVES * DP_RANKS * DP_BINS; i += DP_THREADS)
      if (((i / DP_BINS) % DP_RANKS) < np) (&wave_hist[0][0][0])[i] = 0;
    __syncthreads();

    uint32_t (*wh)[DP_BINS] = wave_hist[wave];
    if (g.vec4) {
      for (int i = tid * 4; i < hw; i += DP_THREADS * 4) {
        const f32x4 v = dp_value4(pa, pb, src, i);
#pragma unroll
        for (int k = 0; k < 4; ++k) dp_count(wh, v[k], np, uniq, mask, shift);
      }
    } else {
      for (int i = tid; i < hw; i += DP_THREADS) dp_count(wh, dp_value(pa, pb, src, i), np, uniq, mask, shift);
    }
    __syncthreads();

    for (int i = tid; i < np * DP_BINS; i += DP_THREADS) {
      const int j = i / DP_BINS, bin = i % DP_BINS;
      uint32_t t = 0;
#pragma unroll
      for (int wv = 0; wv < DP_WAVES; ++wv) t += wave_hist[wv][j][bin];
      hist[j][bin] = t;
    }
    __syncthreads();

    if (pass == 0) {   // every foreground pixel was counted into slot 0: n, then the four ranks
      if (wave == 0) {
        const u32x4 c = *(const u32x4*)&hist[0][4 * lane];
        uint32_t t = c[0] + c[1] + c[2] + c[3];
        t = wave_sum(t);
        if (lane == 0) {
          s_n = t;
          for (int q = 0; q < 2; ++q) {
            double gamma = 0.0;
            uint32_t lo = 0, hi = 0;
            if (t > 0) {   // numpy's linear method: virtual index (n - 1) q / 100
              const double vi = (double)(t - 1) * (q == 0 ? g.low : g.high) / 100.0;
              double fl = floor(vi);
              fl = fmin(fmax(fl, 0.0), (double)(t - 1));
              lo = (uint32_t)fl;
              hi = lo + 1 < t ? lo + 1 : t - 1;
              gamma = fmin(fmax(vi - fl, 0.0), 1.0);
            }
            s_rank[2 * q] = lo;
            s_rank[2 * q + 1] = hi;
            s_gamma[q] = gamma;
          }
        }
      }
      __syncthreads();
      if (s_n == 0) break;   // block-uniform
    }

    if (wave < DP_RANKS) {   // one wave per rank: 4 bins per lane, inclusive scan by shuffles
      const uint32_t rank = s_rank[wave];
      const u32x4 c = *(const u32x4*)&hist[s_slot[wave]][4 * lane];
      const uint32_t t = c[0] + c[1] + c[2] + c[3];
      uint32_t incl = t;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      uint32_t below = incl - t;
      if (rank >= below && rank < incl) {   // exactly one lane: rank < total of the slot
        int k = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (k == q && rank >= below + c[q]) {
            below += c[q];
            k = q + 1;
          }
        s_prefix[wave] |= (uint32_t)(4 * lane + k) << shift;
        s_rank[wave] = rank - below;
      }
    }
    __syncthreads();
    if (tid == 0) {   // ranks that still share a prefix share a slot
      int np2 = 0;
      for (int r = 0; r < DP_RANKS; ++r) {
        int j = 0;
        while (j < np2 && s_uniq[j] != s_prefix[r]) ++j;
        if (j == np2) s_uniq[np2++] = s_prefix[r];
        s_slot[r] = j;
      }
      s_np = np2;
    }
    __syncthreads();
  }

  const uint32_t n = s_n;
  if (tid == 0) {
    double pl = 0.0, ph = 0.0;
    if (n > 0) {
      const double l0 = (double)dp_unkey(s_prefix[0]), l1 = (double)dp_unkey(s_prefix[1]);
      const double h0 = (double)dp_unkey(s_prefix[2]), h1 = (double)dp_unkey(s_prefix[3]);
      pl = l0 + (l1 - l0) * s_gamma[0];
      ph = h0 + (h1 - h0) * s_gamma[1];
    }
    s_p[0] = pl;
    s_p[1] = ph;
    double* st = g.stats + 3 * (long long)plane;
    st[0] = (double)n;
    st[1] = pl;
    st[2] = ph;
  }
  __syncthreads();

  // ---- pass 4: map, rotate, store.  (i, j) = output pixel; torch.rot90(k, dims=[H, W]) read backwards ----
  const double pl = s_p[0], den = (s_p[1] - s_p[0]) + 1e-8;
  const int ho = (g.rot_k & 1) ? g.w : g.h, wo = (g.rot_k & 1) ? g.h : g.w;
  const long long row_stride = (long long)g.nsrc * wo;
  const long long base = (long long)img * ho * row_stride + (long long)src * wo;
  for (int o = tid; o < hw; o += DP_THREADS) {
    const int i = o / wo, j = o - i * wo;
    int y, x;
    switch (g.rot_k) {
      case 0: y = i; x = j; break;
      case 1: y = j; x = g.w - 1 - i; break;
      case 2: y = g.h - 1 - i; x = g.w - 1 - j; break;
      default: y = g.h - 1 - j; x = i; break;
    }
    float r = 0.0f;
    if (n > 0) {
      const float v = dp_value(pa, pb, src, y * g.w + x);
      if (v != 0.0f) {
        const double t = ((double)v - pl) / den;
        r = (float)fmin(fmax(t, 0.0), 1.0);
        if (r < 1e-3f) r = 0.0f;
      }
    }
    const long long dst = base + (long long)i * row_stride + j;
    if (g.out_f32) g.out_f32[dst] = r;
    if (g.out_u8) g.out_u8[dst] = (uint8_t)(r * 255.0f);
  }
}

}  // namespace

extern "C" int pti_display_planes(const float* a, const float* b, int n, int h, int w, int nsrc, double low, double high,
                                  int rot_k, float* out_f32, uint8_t* out_u8, double* stats, pti_stream_t s) {
  if (!a || !stats || (!out_f32 && !out_u8)) PTI_FAIL(PTI_EINVAL, "display_planes: null pointer (a, stats, or both outputs)");
  if (nsrc < 1 || nsrc > 3) PTI_FAIL(PTI_EINVAL, "display_planes: nsrc must be 1, 2 or 3, got %d", nsrc);
  if (nsrc >= 2 && !b) PTI_FAIL(PTI_EINVAL, "display_planes: nsrc = %d needs b", nsrc);
  if (n < 1 || h < 1 || w < 1) PTI_FAIL(PTI_EINVAL, "display_planes: bad shape n=%d h=%d w=%d", n, h, w);
  if (rot_k < 0 || rot_k > 3) PTI_FAIL(PTI_EINVAL, "display_planes: rot_k must be 0..3, got %d", rot_k);
  if (!(low >= 0.0 && high <= 100.0 && low <= high))
    PTI_FAIL(PTI_EINVAL, "display_planes: percentiles must satisfy 0 <= low <= high <= 100, got %g, %g", low, high);
  if (((uintptr_t)stats & 7) || ((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)out_f32 & 3))
    PTI_FAIL(PTI_EINVAL, "display_planes: misaligned buffer");
  if (h > 4096 || w > 4096 || (long long)n * nsrc > 65535)
    PTI_FAIL(PTI_EUNSUPPORTED, "display_planes: unsupported shape n=%d h=%d w=%d nsrc=%d (h, w <= 4096, n * nsrc <= 65535)",
             n, h, w, nsrc);
  DpArgs g;
  g.a = a;
  g.b = nsrc >= 2 ? b : nullptr;
  g.out_f32 = out_f32;
  g.out_u8 = out_u8;
  g.stats = stats;
  g.h = h;
  g.w = w;
  g.nsrc = nsrc;
  g.rot_k = rot_k;
  g.vec4 = ((long long)h * w) % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)g.b & 15) == 0;
  g.low = low;
  g.high = high;
  PTI_LAUNCH(display_planes_kernel, dim3((unsigned)(n * nsrc)), dim3(DP_THREADS), 0, (hipStream_t)s, g);
  PTI_CHECK_LAUNCH("display_planes");
  return PTI_OK;
}
