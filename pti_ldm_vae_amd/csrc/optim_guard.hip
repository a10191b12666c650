// Guarded optimiser step on the flat fp32 arenas (include/pti_vae.h "guarded optimiser step"):
//   grad_norm_partials_kernel  one pass over the gradient arena: per-workgroup {sum of squares, non-finite count} in fp64
//   guard_decide_kernel        one wavefront: folds the partials, decides clip / skip, advances the control record
//   adam_guarded_kernel        adam_kernel's arithmetic (elementwise.hip) on g * (grad_scale * coef), plus the EMA of the
//                              weights in the same pass; returns at once on a skipped step
// No atomics, no host read-back: the decision travels through the control record in device memory.  Every sum has a
// written-out order (the two reduction kernels are compiled without the fast-math re-association, see below), so a
// result depends on the data, n and the arena's alignment, never on the launch.
#include "pti_common.h"

#include <math.h>

namespace {

constexpr int GUARD_THREADS = 256;            // 4 waves per workgroup
constexpr long long GUARD_GRANULE = 4096;     // elements per workgroup before the cap binds (4 x float4 per lane)
constexpr int DECIDE_PER_LANE = PTI_GRAD_GUARD_PARTIALS_CAP / 64;   // pairs per lane of the decision kernel's one wavefront
static_assert(PTI_GRAD_GUARD_PARTIALS_CAP % 64 == 0, "the decision kernel folds the partials 64 at a time");
typedef double f64x2 __attribute__((ext_vector_type(2)));

enum {   // columns of the control record (PTI_GRAD_GUARD_COLUMNS doubles; named in include/pti_vae.h)
  CTL_APPLIED = 0, CTL_SKIPPED, CTL_SUMSQ, CTL_NORM, CTL_COEF, CTL_SKIP, CTL_BIAS1, CTL_BIAS2_SQRT, CTL_EMA_DECAY, CTL_GRAD_MUL
};
static_assert(CTL_GRAD_MUL + 1 == PTI_GRAD_GUARD_COLUMNS, "control record columns");

// exponent all ones: inf or NaN.  Integer tests, so they do not depend on how the build treats isnan / isinf.
__device__ __forceinline__ bool nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool nonfinite_bits(double x) {
  return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

// The library is built with -ffast-math, which lets the compiler re-associate a floating-point sum.  The sums of the two
// reduction kernels must have the order written here: each of their bodies switches the re-association off.

__device__ __forceinline__ void guard_accumulate(float x, double& acc, unsigned& bad) {
#pragma clang fp reassociate(off)
  const double d = (double)x;     // the square of an fp32 value is exact in fp64
  acc += d * d;
  bad += nonfinite_bits(x) ? 1u : 0u;
}

// partials[2 * b] = sum of g^2 over workgroup b's share, partials[2 * b + 1] = its count of non-finite elements.
// The 16-byte body starts at the first aligned element; the up to 3 + 3 elements before and after it go to the first
// lanes of workgroup 0.  Per lane in index order, then the xor butterfly, then (w0 + w1) + (w2 + w3) over the waves.
__global__ __launch_bounds__(GUARD_THREADS) void grad_norm_partials_kernel(const float* __restrict__ g, long long n,
                                                                           double* __restrict__ partials) {
#pragma clang fp reassociate(off)
  const int tid = threadIdx.x;
  long long head = (long long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const long long nvec = (n - head) >> 2;
  const long long tail0 = head + (nvec << 2);
  const f32x4* __restrict__ gv = (const f32x4*)(g + head);
  double acc = 0.0;
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * GUARD_THREADS + tid; i < nvec; i += (long long)gridDim.x * GUARD_THREADS) {
    const f32x4 x = gv[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) guard_accumulate(x[k], acc, bad);
  }
  if (blockIdx.x == 0) {
    if (tid < head) guard_accumulate(g[tid], acc, bad);
    if (tail0 + tid < n) guard_accumulate(g[tail0 + tid], acc, bad);
  }
  acc = wave_sum(acc);
  const double cnt = wave_sum((double)bad);     // exact: integers far below 2^53
  __shared__ double red[8];
  if ((tid & 63) == 0) {
    red[tid >> 6] = acc;
    red[4 + (tid >> 6)] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    partials[2 * (long long)blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    partials[2 * (long long)blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// One wavefront.  Lane l adds partials l, l + 64, ... in that order, the butterfly adds the lanes; lane 0 decides and
// writes the record with ordinary stores.
__global__ __launch_bounds__(64) void guard_decide_kernel(const double* __restrict__ partials, int nparts, double grad_scale,
                                                          double max_norm, int skip_nonfinite, double beta1, double beta2,
                                                          double ema_decay, double* __restrict__ ctl) {
#pragma clang fp reassociate(off)
  const int lane = threadIdx.x;
  // all of the lane's pairs are loaded before the first add (one dependent load after another cost 16 memory round
  // trips at the cap); a missing pair is {0, 0}, and x + 0 is x
  f64x2 part[DECIDE_PER_LANE];
#pragma unroll
  for (int k = 0; k < DECIDE_PER_LANE; ++k) {
    const int i = lane + 64 * k;
    part[k] = i < nparts ? ((const f64x2*)partials)[i] : f64x2{0.0, 0.0};
  }
  double sumsq = 0.0, cnt = 0.0;
#pragma unroll
  for (int k = 0; k < DECIDE_PER_LANE; ++k) {
    sumsq += part[k][0];
    cnt += part[k][1];
  }
  sumsq = wave_sum(sumsq);
  cnt = wave_sum(cnt);
  if (lane != 0) return;
  const double norm = grad_scale * sqrt(sumsq);
  const bool bad = cnt > 0.0 || nonfinite_bits(norm);
  const bool skip = bad && skip_nonfinite != 0;
  double coef = 1.0;
  if (max_norm > 0.0 && !bad) {     // torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6), clamped to 1
    coef = max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  ctl[CTL_SUMSQ] = sumsq;
  ctl[CTL_NORM] = norm;
  ctl[CTL_COEF] = coef;
  ctl[CTL_SKIP] = skip ? 1.0 : 0.0;
  ctl[CTL_GRAD_MUL] = grad_scale * coef;
  if (skip) {                       // Adam's t does not advance (torch.amp.GradScaler's semantics)
    ctl[CTL_SKIPPED] = ctl[CTL_SKIPPED] + 1.0;
    return;
  }
  const double t = ctl[CTL_APPLIED] + 1.0;
  ctl[CTL_APPLIED] = t;
  ctl[CTL_BIAS1] = 1.0 - pow(beta1, t);           // as pti_adam_step's host code computes them
  ctl[CTL_BIAS2_SQRT] = sqrt(1.0 - pow(beta2, t));
  double d = 0.0;
  if (ema_decay > 0.0) {            // warm-up of the LDM code bases
    d = (1.0 + t) / (10.0 + t);
    if (d > ema_decay) d = ema_decay;
  }
  ctl[CTL_EMA_DECAY] = d;
}

// adam_kernel's arithmetic, statement for statement, on one element; the EMA follows the new parameter.  The moments are
// evaluated in the order written: re-associated, the fast-math build turns b2 * v + (1 - b2) * x into x + b2 * (v - x), which
// cancels and leaves v with up to eps / (1 - b2) = 6e-5 relative error (seen against the fp64 oracle).
template <bool EMA>
__device__ __forceinline__ void adam_guarded_one(float& p, float g, float& m, float& v, float& e, float lr, float b1, float b2,
                                                 float eps, float bc1, float bc2_sqrt, float gmul, float one_minus_d) {
#pragma clang fp reassociate(off)
  const float gr = g * gmul;
  const float mm = b1 * m + (1.f - b1) * gr;
  const float vv = b2 * v + (1.f - b2) * gr * gr;
  m = mm;
  v = vv;
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  p -= (lr / bc1) * (mm / denom);
  if (EMA) e += one_minus_d * (p - e);
}

// The record's values are the same for every lane (scalar loads).  16-byte accesses where all arenas are 16-byte aligned
// (torch's allocations are), elements one by one otherwise and for the last n % 4.
template <bool EMA>
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ ema, long long n, float lr, float b1, float b2,
                                                           float eps, const double* __restrict__ ctl) {
  if (ctl[CTL_SKIP] != 0.0) return;     // p, m, v and ema keep their bits
  const float bc1 = (float)ctl[CTL_BIAS1], bc2_sqrt = (float)ctl[CTL_BIAS2_SQRT], gmul = (float)ctl[CTL_GRAD_MUL];
  const float omd = (float)(1.0 - ctl[CTL_EMA_DECAY]);
  uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
  if (EMA) bits |= (uintptr_t)ema;
  const long long nvec = (bits & 15u) == 0 ? (n >> 2) : 0;
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (long long i = first; i < nvec; i += stride) {
    f32x4 pp = ((f32x4*)p)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i], ee = {0.f, 0.f, 0.f, 0.f};
    const f32x4 gg = ((const f32x4*)g)[i];
    if (EMA) ee = ((f32x4*)ema)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pp[k], mk = mm[k], vk = vv[k], ek = ee[k];
      adam_guarded_one<EMA>(pk, gg[k], mk, vk, ek, lr, b1, b2, eps, bc1, bc2_sqrt, gmul, omd);
      pp[k] = pk, mm[k] = mk, vv[k] = vk, ee[k] = ek;
    }
    ((f32x4*)p)[i] = pp;
    ((f32x4*)m)[i] = mm;
    ((f32x4*)v)[i] = vv;
    if (EMA) ((f32x4*)ema)[i] = ee;
  }
  for (long long e = (nvec << 2) + first; e < n; e += stride) {
    float pk = p[e], mk = m[e], vk = v[e], ek = EMA ? ema[e] : 0.f;
    adam_guarded_one<EMA>(pk, g[e], mk, vk, ek, lr, b1, b2, eps, bc1, bc2_sqrt, gmul, omd);
    p[e] = pk, m[e] = mk, v[e] = vk;
    if (EMA) ema[e] = ek;
  }
}

inline long long guard_partials(long long n) {
  if (n < 1) return 0;
  const long long b = (n + GUARD_GRANULE - 1) / GUARD_GRANULE;
  return b > PTI_GRAD_GUARD_PARTIALS_CAP ? PTI_GRAD_GUARD_PARTIALS_CAP : b;
}

}  // namespace

extern "C" int pti_grad_guard_partials(int64_t n) { return (int)guard_partials(n); }

extern "C" int pti_grad_guard(const float* g, int64_t n, double grad_scale, double max_norm, int skip_nonfinite, float beta1,
                              float beta2, double ema_decay, double* partials, double* ctl, pti_stream_t s) {
  if (!g || !partials || !ctl || n <= 0) PTI_FAIL(PTI_EINVAL, "grad_guard: bad args");
  if (((uintptr_t)g & 3) || ((uintptr_t)partials & 15) || ((uintptr_t)ctl & 7)) PTI_FAIL(PTI_EINVAL, "grad_guard: misaligned buffer");
  // written so that a NaN fails each test
  if (!(grad_scale > 0.0 && grad_scale < INFINITY)) PTI_FAIL(PTI_EINVAL, "grad_guard: grad_scale must be finite and positive");
  if (!(max_norm >= 0.0 && max_norm < INFINITY)) PTI_FAIL(PTI_EINVAL, "grad_guard: max_norm must be finite (0: no clipping)");
  if (!(ema_decay >= 0.0 && ema_decay < 1.0)) PTI_FAIL(PTI_EINVAL, "grad_guard: ema_decay must be in (0, 1) (0: no EMA)");
  if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f)) PTI_FAIL(PTI_EINVAL, "grad_guard: betas must be in [0, 1)");
  const int nparts = (int)guard_partials(n);
  PTI_LAUNCH(grad_norm_partials_kernel, dim3(nparts), dim3(GUARD_THREADS), 0, (hipStream_t)s, g, (long long)n, partials);
  PTI_CHECK_LAUNCH("grad_guard_partials");
  PTI_LAUNCH(guard_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (const double*)partials, nparts, grad_scale, max_norm,
             skip_nonfinite, (double)beta1, (double)beta2, ema_decay, ctl);
  PTI_CHECK_LAUNCH("grad_guard_decide");
  return PTI_OK;
}

extern "C" int pti_adam_step_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                                     float beta2, float eps, const double* ctl, pti_stream_t s) {
  if (!p || !g || !m || !v || !ctl || n <= 0) PTI_FAIL(PTI_EINVAL, "adam_step_guarded: bad args");
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 3) || ((uintptr_t)ctl & 7))
    PTI_FAIL(PTI_EINVAL, "adam_step_guarded: misaligned buffer");
  long long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (ema) {
    PTI_LAUNCH(adam_guarded_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, p, g, m, v, ema, (long long)n, lr,
               beta1, beta2, eps, ctl);
  } else {
    PTI_LAUNCH(adam_guarded_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, p, g, m, v, ema, (long long)n, lr,
               beta1, beta2, eps, ctl);
  }
  PTI_CHECK_LAUNCH("adam_step_guarded");
  return PTI_OK;
}
