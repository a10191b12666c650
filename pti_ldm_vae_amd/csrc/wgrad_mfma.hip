// Weight / bias gradient of the implicit-GEMM convolutions (autograd of nn.Conv2d inside MONAI's
// AEKLResBlock / AEKLDownsample / Upsample / SABlock linears; SURVEY.md §7 hard part 3) on
// v_mfma_f32_32x32x16_bf16:
//     dW[co][ci][tap] = sum_{n,p} dY[n,p,co] * A[n, p*S + tap - pad, ci],   A = prologue(x)
// GEMM view: M = co, N = ci (per tap), K = pixels.  Both operands need K (pixels) as the
// per-lane-contiguous index while NHWC memory has channels contiguous, so both MFMA fragments
// come from gfx950's transposing LDS read ds_read_b64_tr_b16 on plain [pixel][channel] tiles.
//
// One workgroup (4 waves) owns a (<=64 co) x (<=64 ci) x (K*K taps) block of dW for one SPLIT of
// the pixel tiles (split-K): each wave keeps 32co x 32ci x 9 taps = 144 accumulator VGPRs, the
// GN+SiLU prologue is recomputed in the loader exactly as the forward conv does, partial blocks
// go to a workspace slab with plain stores and pti_wgrad_reduce sums the slabs in a fixed order
// (deterministic, no float atomics) into the fp32 OIHW gradient.
#include "pti_common.h"

namespace {

constexpr int TH = 8, TW = 16;
constexpr int PTI_WGRAD_SLAB_V4 = 1 << 30;
#ifndef PTI_WGRAD_BATCH_MAX
#define PTI_WGRAD_BATCH_MAX 16
#endif
//   // flag in the slab token of pti_conv_wgrad_mfma_partials: block-ordered slabs (v4)

struct WgArgs {
  const bf16* x;
  const bf16* dy;
  const stat_t* in_stats;
  const float* gamma;
  const float* beta;
  float* slab;  // [S][KK*Cout*Cin + Cout]
  int N, H, W, Cin, Ho, Wo, Cout;
  int mode, prologue, groups;
  float eps, inv_cnt;
  int tiles_x, tiles_y, ntiles, S;
  int ci_tiles;
  long long slab_stride;
  int x_f16;   // x is a forward activation stored fp16 (converted to the bf16 MFMA operand in the loader)
  int diag;    // v4 tuning aid (PTI_WGRAD_V4_DIAG): 1 = no tile loads, 2 = no MFMA loop, 3 = neither (results are garbage)
};

template <int KS, int S_, int CO_T, int CI_T>
struct WCfg {
  static constexpr int HH = (TH - 1) * S_ + KS, HW = (TW - 1) * S_ + KS;
  static constexpr int NP = HH * HW;
  static constexpr int KK = KS * KS;
  static constexpr int PA = CI_T * 2 + (CI_T == 64 ? 64 : 0);   // halo pixel pitch (bytes)
  static constexpr int PD = CO_T * 2 + (CO_T == 64 ? 64 : 0);   // dY pixel pitch (bytes)
  static constexpr int NCA = CI_T / 8, NCD = CO_T / 8;
  static constexpr int WCO = CO_T / 32, WCI = CI_T / 32, WPX = 4 / (WCO * WCI);
  static constexpr int A_BYTES = NP * PA, D_BYTES = TH * TW * PD;
  static constexpr int HIT = (NP * NCA + 255) / 256, DIT = (TH * TW * NCD + 255) / 256;
  static constexpr int RED_BYTES = (WPX > 1) ? 32 * 32 * 4 * (WPX - 1) * WCO * WCI : 0;  // per-tap cross-wave reduce
  static constexpr int LDS_BYTES = (A_BYTES + D_BYTES) > RED_BYTES ? (A_BYTES + D_BYTES) : RED_BYTES;
};

// PLAIN: no GroupNorm prologue (every launch of the training step that takes this kernel): its code and the 16
// scale/shift registers are compiled out
template <int KS, int S_, int CO_T, int CI_T, bool PLAIN>
__global__ __launch_bounds__(256, 2) void wgrad_mfma_kernel(WgArgs a) {
  using C = WCfg<KS, S_, CO_T, CI_T>;
  const int prologue = PLAIN ? PTI_PRO_NONE : a.prologue;
  typedef short v4s __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS_BYTES];
  unsigned char* lA = smem;
  unsigned char* lD = smem + C::A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.y;  // (co,ci) tiles of one pixel split are adjacent in dispatch order: shared L2 lines
  const int cot = blockIdx.x / a.ci_tiles, cit = blockIdx.x % a.ci_tiles;
  const int wco = wave / (C::WCI * C::WPX), wci = (wave / C::WPX) % C::WCI, wpx = wave % C::WPX;

  const int pad_lo = (a.mode == PTI_CONV_S2PAD) ? 0 : (KS - 1) / 2;
  const bool twox = (a.mode == PTI_CONV_UP2);
  const int VH = twox ? 2 * a.H : a.H, VW = twox ? 2 * a.W : a.W;

  // per-lane transposed-read bases (see header comment of tr reads in DESIGN.md):
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int pk = 8 * (g >> 1) + q;                       // pixel within the 16-pixel k-block (first read)
  const int chl = 16 * (g & 1) + 4 * pp;                 // channel within the wave's 32-channel block
  const int dbase = pk * C::PD + (wco * 32 + chl) * 2;   // + row*TW*PD, second read + 4*PD
  const int abase = (pk * S_) * C::PA + (wci * 32 + chl) * 2;  // + (row*S+kh)*HW*PA + kw*PA, second + 4*S*PA

  f32x16 acc[C::KK];
#pragma unroll
  for (int t = 0; t < C::KK; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // loader geometry
  const int alc = tid % C::NCA, alp = tid / C::NCA;
  constexpr int APSTEP = 256 / C::NCA;
  const int dlc = tid % C::NCD, dlp = tid / C::NCD;
  constexpr int DPSTEP = 256 / C::NCD;
  const int cpg = a.Cin / (a.groups > 0 ? a.groups : 1);
  float bsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bsum[j] = 0.f;

  u32x4 araw[C::HIT], draw[C::DIT];
  bool aok[C::HIT];
  int cur_n = -1;
  float sc[8], sh[8];

  auto issue_loads = [&](int tile) {
    int t = tile;
    const int tx_ = t % a.tiles_x; t /= a.tiles_x;
    const int ty_ = t % a.tiles_y;
    const int n = t / a.tiles_y;
    const int oy0 = ty_ * TH, ox0 = tx_ * TW;
    const int vy0 = oy0 * S_ - pad_lo, vx0 = ox0 * S_ - pad_lo;
#pragma unroll
    for (int it = 0; it < C::HIT; ++it) {
      const int p = alp + it * APSTEP;
      const int hy = p / C::HW, hx = p - hy * C::HW;
      const int vy = vy0 + hy, vx = vx0 + hx;
      const bool v = (p < C::NP) && vy >= 0 && vy < VH && vx >= 0 && vx < VW;
      const int iy = twox ? (vy >> 1) : vy, ix = twox ? (vx >> 1) : vx;
      aok[it] = v;
      araw[it] = u32x4{0u, 0u, 0u, 0u};
      if (v) araw[it] = *(const u32x4*)(a.x + ((size_t)(n * a.H + iy) * a.W + ix) * a.Cin + cit * CI_T + alc * 8);
    }
#pragma unroll
    for (int it = 0; it < C::DIT; ++it) {
      const int p = dlp + it * DPSTEP;
      const int ty = p / TW, tx = p % TW;
      const int oy = oy0 + ty, ox = ox0 + tx;
      draw[it] = u32x4{0u, 0u, 0u, 0u};
      if (p < TH * TW && oy < a.Ho && ox < a.Wo)
        draw[it] = *(const u32x4*)(a.dy + ((size_t)(n * a.Ho + oy) * a.Wo + ox) * a.Cout + cot * CO_T + dlc * 8);
    }
    return n;
  };

  auto write_lds = [&](int n) {
    if (prologue != PTI_PRO_NONE && n != cur_n) {
      cur_n = n;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = cit * CI_T + alc * 8 + j;
        const int gg = ch / cpg;
        const float sum = stat_f(a.in_stats, (n * a.groups + gg) * 2), sq = stat_f(a.in_stats, (n * a.groups + gg) * 2 + 1);
        const float mean = sum * a.inv_cnt;
        const float rstd = rsqrtf(fmaxf(sq * a.inv_cnt - mean * mean, 0.f) + a.eps);
        sc[j] = rstd * a.gamma[ch];
        sh[j] = a.beta[ch] - mean * sc[j];
      }
    }
#pragma unroll
    for (int it = 0; it < C::HIT; ++it) {
      const int p = alp + it * APSTEP;
      if (p < C::NP) {
        u32x4 r = araw[it];
        if (prologue != PTI_PRO_NONE && aok[it]) {
          float f[8];
          unpack8f(r, f, a.x_f16);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float v = f[j] * sc[j] + sh[j];
            if (prologue == PTI_PRO_GN_SILU) v = silu_f(v);
            f[j] = v;
          }
          r = pack8(f);
        } else if (a.x_f16) {
          float f[8];
          unpack8f(r, f, true);
          r = pack8(f);
        }
        *(u32x4*)(lA + p * C::PA + alc * 16) = r;
      }
    }
#pragma unroll
    for (int it = 0; it < C::DIT; ++it) {
      const int p = dlp + it * DPSTEP;
      if (p < TH * TW) {
        *(u32x4*)(lD + p * C::PD + dlc * 16) = draw[it];
        if (cit == 0) {
          float f[8];
          unpack8(draw[it], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) bsum[j] += f[j];
        }
      }
    }
  };

  int tile = split;
  int n_next = -1;
  if (tile < a.ntiles) n_next = issue_loads(tile);
  for (; tile < a.ntiles; tile += a.S) {
    write_lds(n_next);
    __syncthreads();
    const int nxt = tile + a.S;
    if (nxt < a.ntiles) n_next = issue_loads(nxt);
    // ---- MFMAs: this wave's tile rows ----
#pragma unroll
    for (int rr = 0; rr < TH / C::WPX; ++rr) {
      const int row = wpx + rr * C::WPX;
      const unsigned char* dptr = lD + dbase + row * TW * C::PD;
      const v4s d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(dptr));
      const v4s d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(dptr + 4 * C::PD));
      bf16x8 dfrag;
      {
        typedef short v8s __attribute__((ext_vector_type(8)));
        v8s t8 = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
        dfrag = __builtin_bit_cast(bf16x8, t8);
      }
#pragma unroll
      for (int kh = 0; kh < KS; ++kh) {
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
          const unsigned char* aptr = lA + abase + ((row * S_ + kh) * C::HW + kw) * C::PA;
          const v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(aptr));
          const v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(aptr + 4 * S_ * C::PA));
          typedef short v8s __attribute__((ext_vector_type(8)));
          v8s t8 = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
          const bf16x8 afrag = __builtin_bit_cast(bf16x8, t8);
          acc[kh * KS + kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfrag, afrag, acc[kh * KS + kw], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: (cross-wave reduce when waves split pixels), write the slab [tap][co][ci] ----
  float* slab = a.slab + (size_t)split * a.slab_stride;
  const int ci = cit * CI_T + wci * 32 + (lane & 31);
  const int hsel = lane >> 5;
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int t = 0; t < C::KK; ++t) {
    if constexpr (C::WPX > 1) {
      // waves wpx>0 park their tap accumulators in LDS, wave wpx==0 of each (wco,wci) sums them
      if (wpx > 0) {
        float* dst = red + (((wco * C::WCI + wci) * (C::WPX - 1) + (wpx - 1)) * 16) * 64;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[r * 64 + lane] = acc[t][r];
      }
      __syncthreads();
      if (wpx == 0) {
#pragma unroll
        for (int o = 0; o < C::WPX - 1; ++o) {
          const float* src = red + (((wco * C::WCI + wci) * (C::WPX - 1) + o) * 16) * 64;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] += src[r * 64 + lane];
        }
      }
      __syncthreads();
    }
    if (wpx == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = cot * CO_T + wco * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
        slab[((size_t)t * a.Cout + co) * a.Cin + ci] = acc[t][r];
      }
    }
  }
  // bias partial sums: reduce the threads that share dlc (stride NCD) through LDS
  if (cit == 0) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j * 256 + tid] = bsum[j];
    __syncthreads();
    if (tid < CO_T) {
      const int lc = tid / 8, j = tid % 8;
      float s = 0.f;
      for (int k = lc; k < 256; k += C::NCD) s += red[j * 256 + k];
      slab[(size_t)C::KK * a.Cout * a.Cin + cot * CO_T + tid] = s;
    }
  }
}

// =============================================================================================
// v3 (3x3, stride-1 gathers): 32co x 32ci block per workgroup, THREE waves, wave = kernel column kw.
// Measured on v1 (144 accumulator VGPRs per wave => 2 waves/SIMD, one 20 KB tile in flight per workgroup):
// the loop is bound by HBM latency x bytes in flight (Little's law), ~2-3 TB/s.  Splitting the 9 taps over
// three waves leaves 48 accumulator VGPRs per wave => ~5 workgroups per CU, i.e. ~100 KB of loads in flight
// per CU, and removes the cross-wave accumulator reduction of the pixel-split form.
// Measured afterwards on 128->128 @64^2 (68 us with its reduce launch): loads + slabs without the MFMA loop 50 us,
// MFMA loop without loads 52 us, without loads and slabs 44 us -- neither side is near its roof (15 / 20 us) and they
// overlap only partly.  (tried: an LDS-DMA variant -- x / dy tiles by global_load_lds into a second LDS buffer, no
// staging registers, no ds_write pass, one barrier per tile, 68 VGPRs -- ran within 1 % of this kernel on every
// shape; taller tiles (16 rows) +-10 % depending on the shape; 512..2048 workgroups within +-8 %; TWO tiles in flight
// per workgroup -- a second staging register set, loads issued two iterations ahead -- costs the third wave per SIMD
// (254 VGPRs) and ran 13-22 % slower.)
// =============================================================================================
// COB = number of 32-channel co blocks per workgroup (2 when Cout % 64 == 0): every wave then feeds TWO dy fragments
// per x fragment (6 accumulators, 96 AGPRs): 52 transposing LDS reads per 48 MFMAs instead of 36 per 24, the x halo
// tile is staged once per 64 output channels instead of once per 32, and there are half as many barriers per MFMA.
template <int COB>
struct W3Cfg {
  static constexpr int TH = 8, HH = TH + 2, HW = TW + 2, NP = HH * HW;
  static constexpr int PP = 64;                                  // bytes per pixel (32 channels bf16)
  static constexpr int A_BYTES = NP * PP, DP_BYTES = TH * TW * PP;   // dy: one [pixel][32 co] plane per co block
  static constexpr int D_BYTES = COB * DP_BYTES;
  static constexpr int NT = 192;
  static constexpr int DPC = 4 * COB;                            // 16-byte pieces per dy pixel
  static constexpr int HIT = (NP * 4 + NT - 1) / NT, DIT = (TH * TW * DPC + NT - 1) / NT;
  static constexpr int LDS_BYTES = A_BYTES + D_BYTES;
};

// PLAIN: no GroupNorm prologue -- the training step's case (x is the saved, already activated bf16 tensor, or the
// fp16 stream tensor of an up-sampling conv: the loader is a copy / a format conversion); the 16 scale/shift registers
// and the normalisation code are compiled out and the kernel fits 128 VGPRs.
template <int COB, bool PLAIN>
__global__ __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(COB == 1 ? (PLAIN ? 4 : 3) : 2, COB == 1 ? (PLAIN ? 4 : 3) : 2)))
void wgrad_mfma3_kernel(WgArgs a) {   // COB 1: 3 waves/SIMD (<= 168 VGPR+AGPR), 4 when PLAIN; COB 2: 2 waves/SIMD
  using C = W3Cfg<COB>;
  const int prologue = PLAIN ? PTI_PRO_NONE : a.prologue;
  const bool x_f16 = (bool)a.x_f16;
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS_BYTES];
  unsigned char* lA = smem;
  unsigned char* lD = smem + C::A_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, kw = tid >> 6;   // wave = kernel COLUMN (see the main loop)
  // XCD-aware block order: consecutive workgroup ids go round-robin over the 8 XCDs (one L2 each), so the
  // (co, ci) blocks that stream the SAME pixel tiles (same split) are placed on the same XCD, back to back:
  // id = 8 * (tiles_cc * (split / 8) + cc) + split % 8.  Host guarantees S % 8 == 0 or S < 8 (then id = S * cc + split).
  int split, cc;
  {
    const int id = blockIdx.x, tiles_cc = a.ci_tiles * (a.Cout / (32 * COB));
    if (a.S >= 8) {
      const int k = id >> 3;
      cc = k % tiles_cc;
      split = (k / tiles_cc) * 8 + (id & 7);
    } else {
      cc = id / a.S;
      split = id % a.S;
    }
  }
  const int cot = cc / a.ci_tiles, cit = cc % a.ci_tiles;
  const int co0 = cot * 32 * COB;
  const bool twox = (a.mode == PTI_CONV_UP2);
  const int VH = twox ? 2 * a.H : a.H, VW = twox ? 2 * a.W : a.W;

  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int pk = 8 * (g >> 1) + q, chl = 16 * (g & 1) + 4 * pp;
  const int fbase = pk * C::PP + chl * 2;

  f32x16 acc[COB][3];
#pragma unroll
  for (int h = 0; h < COB; ++h)
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[h][t][r] = 0.f;
  float bsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bsum[j] = 0.f;

  const int lc = tid & 3, lp = tid >> 2;            // x: piece within a pixel / pixel index, step 48
  const int lcd = tid % C::DPC, lpd = tid / C::DPC;   // dy: piece within a pixel / pixel index, step NT / DPC
  constexpr int PSTEP = C::NT / 4, DSTEP = C::NT / C::DPC;
  const int cpg = a.Cin / (a.groups > 0 ? a.groups : 1);
  int cur_n = -1;
  float sc[8], sh[8];
  u32x4 araw[C::HIT], draw[C::DIT];
  unsigned aokm = 0;

  auto issue = [&](int tile) -> int {
    int t = tile;
    const int tx_ = t % a.tiles_x; t /= a.tiles_x;
    const int ty_ = t % a.tiles_y;
    const int n = t / a.tiles_y;
    const int oy0 = ty_ * C::TH, ox0 = tx_ * TW;
#pragma unroll
    for (int it = 0; it < C::HIT; ++it) {
      const int p = lp + it * PSTEP;
      const int hy = p / C::HW, hx = p - hy * C::HW;
      const int vy = oy0 - 1 + hy, vx = ox0 - 1 + hx;
      const bool v = (p < C::NP) && vy >= 0 && vy < VH && vx >= 0 && vx < VW;
      const int iy = twox ? (vy >> 1) : vy, ix = twox ? (vx >> 1) : vx;
      aokm = (aokm & ~(1u << it)) | ((unsigned)v << it);
      araw[it] = u32x4{0u, 0u, 0u, 0u};
      if (v) araw[it] = *(const u32x4*)(a.x + ((size_t)(n * a.H + iy) * a.W + ix) * a.Cin + cit * 32 + lc * 8);
    }
#pragma unroll
    for (int it = 0; it < C::DIT; ++it) {
      const int p = lpd + it * DSTEP;
      const int oy = oy0 + p / TW, ox = ox0 + p % TW;
      draw[it] = u32x4{0u, 0u, 0u, 0u};
      if (p < C::TH * TW && oy < a.Ho && ox < a.Wo)
        draw[it] = *(const u32x4*)(a.dy + ((size_t)(n * a.Ho + oy) * a.Wo + ox) * a.Cout + co0 + lcd * 8);
    }
    return n;
  };
  auto commit = [&](int n) {
    if (prologue != PTI_PRO_NONE && n != cur_n) {
      cur_n = n;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = cit * 32 + lc * 8 + j;
        const int gg = ch / cpg;
        const float sum = stat_f(a.in_stats, (n * a.groups + gg) * 2), sq = stat_f(a.in_stats, (n * a.groups + gg) * 2 + 1);
        const float mean = sum * a.inv_cnt;
        const float rstd = rsqrtf(fmaxf(sq * a.inv_cnt - mean * mean, 0.f) + a.eps);
        sc[j] = rstd * a.gamma[ch];
        sh[j] = a.beta[ch] - mean * sc[j];
      }
    }
#pragma unroll
    for (int it = 0; it < C::HIT; ++it) {
      const int p = lp + it * PSTEP;
      if (p < C::NP) {
        u32x4 r = araw[it];
        if (prologue != PTI_PRO_NONE && ((aokm >> it) & 1u)) {
          float f[8];
          unpack8f(r, f, x_f16);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float v = f[j] * sc[j] + sh[j];
            if (prologue == PTI_PRO_GN_SILU) v = silu_f(v);
            f[j] = v;
          }
          r = pack8(f);
        } else if (x_f16) {
          float f[8];
          unpack8f(r, f, true);
          r = pack8(f);
        }
        *(u32x4*)(lA + p * C::PP + lc * 16) = r;
      }
    }
#pragma unroll
    for (int it = 0; it < C::DIT; ++it) {
      const int p = lpd + it * DSTEP;
      if (p < C::TH * TW) {
        *(u32x4*)(lD + (lcd >> 2) * C::DP_BYTES + p * C::PP + (lcd & 3) * 16) = draw[it];
        if (cit == 0) {
          float f[8];
          unpack8(draw[it], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) bsum[j] += f[j];
        }
      }
    }
  };

  int tile = split, n_next = -1;
  if (tile < a.ntiles) n_next = issue(tile);
  for (; tile < a.ntiles; tile += a.S) {
    commit(n_next);
    __syncthreads();
    const int nxt = tile + a.S;
    if (nxt < a.ntiles) n_next = issue(nxt);
    // Wave kw walks the TH+2 halo rows once: the x fragment of halo row r (column offset kw) meets the dy
    // fragments of output rows r, r-1, r-2 for kernel rows kh = 0, 1, 2.  Each dy fragment is read once and kept for
    // three rows, each x fragment is read once: 4 transposing LDS reads per 3 MFMAs at COB = 1, 6 per 6 at COB = 2
    // (wave = kernel row needed 8 per 3: at ~120 KB of LDS traffic per tile the kernel was LDS-bound, not MFMA-bound).
    bf16x8 dfr[COB][C::TH];
#pragma unroll
    for (int r = 0; r < C::TH + 2; ++r) {
      if (r < C::TH) {
#pragma unroll
        for (int h = 0; h < COB; ++h) {
          const unsigned char* dptr = lD + h * C::DP_BYTES + fbase + r * TW * C::PP;
          const v4s d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(dptr));
          const v4s d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(dptr + 4 * C::PP));
          v8s td = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
          dfr[h][r] = __builtin_bit_cast(bf16x8, td);
        }
      }
      const unsigned char* aptr = lA + fbase + (r * C::HW + kw) * C::PP;
      const v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(aptr));
      const v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(aptr + 4 * C::PP));
      v8s ta = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      const bf16x8 afr = __builtin_bit_cast(bf16x8, ta);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int o = r - kh;          // output row whose halo row o + kh is r
        if (o >= 0 && o < C::TH) {
#pragma unroll
          for (int h = 0; h < COB; ++h)
            acc[h][kh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[h][o], afr, acc[h][kh], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: wave kw owns taps kw, 3 + kw, 6 + kw of the slab [tap][co][ci] ----
  float* slab = a.slab + (size_t)split * a.slab_stride;
  const int ci = cit * 32 + (lane & 31);
  const int hsel = lane >> 5;
#pragma unroll
  for (int h = 0; h < COB; ++h)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + h * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
        slab[((size_t)(kh * 3 + kw) * a.Cout + co) * a.Cin + ci] = acc[h][kh][r];
      }
  if (cit == 0) {   // bias partials: threads with equal lcd hold the same 8 channels
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j * C::NT + tid] = bsum[j];
    __syncthreads();
    if (tid < 32 * COB) {
      const int c8 = tid / 8, j = tid % 8;
      float sm = 0.f;
      for (int k = c8; k < C::NT; k += C::DPC) sm += red[j * C::NT + k];
      slab[(size_t)9 * a.Cout * a.Cin + co0 + tid] = sm;
    }
  }
}

// =============================================================================================
// v4 (3x3, PTI_CONV_S1, bf16 x without prologue -- the training step's saved activated inputs): 32co x 32ci block
// per workgroup like v3, but
//   * the x halo / dy tiles arrive by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write pass) into
//     a ring of four PAIRS of stages, three pairs (six tiles, 120 KB) ahead, behind a COUNTED s_waitcnt vmcnt + ONE raw
//     s_barrier per pair.  The DMA is issued from inline asm: through the builtin hipcc drains vmcnt(0) in front of
//     the next LDS read (it cannot prove that the DMA's ring slot differs from the one being read), which serialises
//     the ring -- the reason an earlier LDS-DMA variant of v3 measured no gain;
//   * EIGHT waves = two groups of four; per iteration group g takes tile 2*it + g of this workgroup's split, wave w of
//     a group the output rows 2w, 2w+1 of that 8x16 tile with all nine taps (144 accumulator registers): 18 MFMAs and
//     28 transposing LDS reads per wave and tile, two waves per SIMD on all four SIMDs (v3's three kernel-column waves
//     left one SIMD without MFMA work); the eight partial blocks are summed through LDS once, at the end, in a fixed
//     order;
//   * ONE resident workgroup per CU (the ring is the latency hiding); batched over up to 16 layers per launch (W4Batch)
//     the partial slabs are ~1024 x 37 KB = 38 MB per LAUNCH of 16 layers instead of 38..47 MB per LAYER (which
//     exceeded the 17 MB of x + dy of the 128-channel 32^2 layers more than twice, written AND re-read);
//   * out-of-image halo pixels / ragged tile edges / tiles past the end read a 16-byte zero page, so every wave issues
//     exactly 5 DMA instructions per iteration and the vmcnt arithmetic is uniform; interior tiles (no edge in reach)
//     skip the per-piece range checks;
//   * dbias rides the MFMA pipe: dy fragments times a fragment of ones (no VALU, no extra LDS traffic).
// Stage image: [x: 12 x 1 KiB = 768 pieces (720 used: 10 x 18 halo pixels x 4 pieces)][dy: 8 KiB = 128 pixels x 4].
// =============================================================================================
__device__ __attribute__((aligned(16))) unsigned int pti_wgrad_zero_page[4] = {0u, 0u, 0u, 0u};

__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

constexpr int W4_STG = 20 * 1024, W4_DP = 3, W4_NSTAGE = 2 * (W4_DP + 1), W4_IMG = 9 * 32 * 32 * 4;   // DP = pairs of tiles ahead
// "two output-channel blocks per tile" mode (jobs with Cout % 64 == 0): both wave groups work on the SAME pixel tile,
// group g on output-channel block 2*cot + g.  The x halo (12 KB) is then fetched once for two blocks: a stage is
// 12 + 2 x 8 = 28 KB for the 144 MFMAs that the pair mode feeds with 2 x 20 = 40 KB.  Ring: five 28-KB stages, four
// tiles ahead.  Measured (same box, config A batch 32): the >= 64-channel layers 582 -> 619 TFLOP/s, step -1.1 %; AR
// model 635 -> 678 TFLOP/s.  30 % fewer fill bytes bought 6-7 %: the fill is not the only bound.  What remains is the
// LDS READ side -- 28 transposing fragment reads (56 ds_read_b64_tr_b16 = 28.7 KB) per wave and tile for 18 MFMAs:
// 8 waves x 56 x 4 cycles = 1792 LDS cycles per tile pair against 8 x 18 / 4 x 32 = 1152 MFMA cycles per SIMD.  Fewer
// reads per MFMA need more accumulators per wave (an x fragment is shared by the kernel rows of up to three output rows
// and by every output-channel block a wave owns): one wave per SIMD with two blocks in 288 registers (0.44 fragments
// per MFMA instead of 0.78) is the design this points to.
// (Tried on that theory and REJECTED: reading only the kw = 0 x fragment of a halo row and shifting the kw = 1, 2
// fragments out of it in registers -- 4 v_alignbit + 1 v_permlane32_swap + two 2-byte LDS reads for the entering pixels
// per row instead of 4 transposing reads: 28 -> 12 fragment reads per wave and tile.  Bit-exact, and 1.7 % SLOWER per
// step on both models: the longer dependent chain in front of each row's MFMAs costs more than the LDS time it saves,
// so LDS read bandwidth is not the binding limit either; what remains is the per-tile critical path -- wait, barrier,
// transposing reads, 18 dependent-issue MFMAs -- with two waves per SIMD to hide it.)
constexpr int W4_STG2 = 28 * 1024, W4_DP2 = 4, W4_NST2 = W4_DP2 + 1;
constexpr int W4_LDS = (W4_NSTAGE * W4_STG > 4 * W4_IMG + 1024) ? W4_NSTAGE * W4_STG : 4 * W4_IMG + 1024;

// Up to PTI_WGRAD_BATCH_MAX independent weight-gradient problems in ONE launch (+ one slab-reduction launch): a launch
// of this kernel costs ~11 us of fixed time (dispatch, ring fill, cross-wave reduction, slab drain) next to 10..45 us of
// streaming on the training step's layers, and the layers' weight gradients do not depend on each other.
struct W4Job {
  const bf16* x; const bf16* dy; float* slab;
  long long slab_stride;
  int N, H, W, Cin, Cout, tiles_x, tiles_y, ntiles, S;
  int cob2;   // two output-channel blocks per workgroup (see W4_STG2)
};
// Workgroup placement.  The (co, ci) blocks of one pixel split of one job stream the SAME x / dy tiles, so they must
// share an XCD (one L2 per XCD; workgroup ids are dealt round-robin over the 8 XCDs: id & 7 names the XCD -- for speed
// only, a different deal would only cost bandwidth).  A "group" = (job, split) = tiles32 workgroups.  The host deals
// the groups of the whole batch over the eight XCDs (biggest first, onto the shortest list) and the kernel finds its
// (job, split, block) from id & 7, id >> 3 and the group list of that XCD.  Measured without it on the batched launch
// (S = 1..2 per job: consecutive ids = different blocks of one split, spread over all XCDs): 2.1x the algorithmic
// bytes fetched.
constexpr int W4_MAXGRP = 64;   // groups per XCD (=> at most 512 groups per launch; the batch struct must stay under the 4-KB kernarg limit)
struct W4Batch {
  W4Job job[PTI_WGRAD_BATCH_MAX];
  float* dw[PTI_WGRAD_BATCH_MAX];
  float* dbias[PTI_WGRAD_BATCH_MAX];
  int accumulate[PTI_WGRAD_BATCH_MAX];
  int first_rblk[PTI_WGRAD_BATCH_MAX + 1];   // blocks of the reduction launch
  unsigned short grp[8][W4_MAXGRP];           // job (4 bits) | split << 4
  unsigned short grp_start[8][W4_MAXGRP + 1]; // first position (id >> 3) of each group in its XCD's list
  int ngrp[8];
  int njobs, diag, nwg;
};

static_assert(sizeof(W4Batch) <= 4096 && PTI_WGRAD_BATCH_MAX <= 16, "kernarg limit / 4-bit job index of the group word");

// COB2: every job of the batch runs in the two-output-channel-block mode (see W4_STG2) -- a compile-time switch: with
// the mode as a run-time (block-uniform) flag the shared hot loop carried both address schemes and ran 20 % slower
// in either mode (same-box: 660 -> 798 us per launch).  A batch never mixes modes; the host splits the jobs.
template <bool COB2>
__global__ __launch_bounds__(512, 1) void wgrad_mfma4_kernel(W4Batch b) {
  constexpr int HWp = TW + 2, NPX = 10 * HWp, PP = 64, XB = 12 * 1024, STG = W4_STG, DP = W4_DP, NPS = DP + 1;   // NPS pair slots
  static_assert(W4_LDS <= 160 * 1024 && 5 * (DP - 1) <= 63, "ring must fit the LDS and the vmcnt counter");
  static_assert(W4_NST2 * W4_STG2 <= W4_LDS && 5 * (W4_DP2 - 1) <= 63, "two-block ring must fit as well");
  // ---- which (job, pixel split, (co,ci) block) is this workgroup? (block-uniform scalar code) ----
  const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
  const int ng = b.ngrp[xcd];
  if (ng == 0 || pos >= b.grp_start[xcd][ng]) return;                        // padding workgroup of a shorter list
  int gi = 0;
  while (gi + 1 < ng && pos >= b.grp_start[xcd][gi + 1]) ++gi;
  const unsigned gword = b.grp[xcd][gi];
  const int jb = gword & 15, split = gword >> 4, cc = pos - b.grp_start[xcd][gi];
  const W4Job& a = b.job[jb];
  const int ci_tiles = a.Cin / 32;
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  __shared__ __attribute__((aligned(16))) unsigned char smem[W4_LDS];
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = w8 >> 2, w = w8 & 3;
  const int cot = cc / ci_tiles, cit = cc % ci_tiles;
  constexpr bool cob2 = COB2;
  const int co0 = cob2 ? (2 * cot + grp) * 32 : cot * 32, ci0 = cit * 32;   // (wave-uniform in the two-block mode)
  const bool do_bias = (cit == 0);   // block-uniform

  // ---- DMA slots of this lane: 3 x pieces (instructions w, w+4, w+8 of the stage) and 2 dy pieces (w, w+4) ----
  int xhy[3], xhx[3], xrel[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = (w + 4 * k) * 64 + lane, p = i >> 2;
    xhy[k] = p < NPX ? p / HWp : 1 << 20;                    // pad pieces: never in range
    xhx[k] = p - (p / HWp) * HWp;
    xrel[k] = ((xhy[k] - 1) * a.W + xhx[k] - 1) * a.Cin * 2 + (ci0 + (i & 3) * 8) * 2;   // bytes from pixel (oy0, ox0) of sample n
  }
  int dty[2], dtx[2], drel[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = (w + 4 * k) * 64 + lane, p = i >> 2;
    dty[k] = p >> 4;
    dtx[k] = p & 15;
    drel[k] = (dty[k] * a.W + dtx[k]) * a.Cout * 2 + (co0 + (i & 3) * 8) * 2;
  }
  const unsigned char* xb = reinterpret_cast<const unsigned char*>(a.x);
  const unsigned char* db = reinterpret_cast<const unsigned char*>(a.dy);
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(pti_wgrad_zero_page);

  // One DMA slot (k = 0..2: x pieces, 3..4: dy pieces) of tile `tile` into `stage`; tiles past the end read zeros so
  // that every wave issues exactly 5 DMA instructions per iteration (uniform vmcnt arithmetic).
  struct TilePos { const unsigned char* xt; const unsigned char* dt; int oy0, ox0; bool live, interior; };
  auto locate = [&](int tile) -> TilePos {
    TilePos tp;
    tp.live = tile < a.ntiles;                                // wave-uniform
    int t = tp.live ? tile : 0;
    const int tx_ = t % a.tiles_x; t /= a.tiles_x;
    const int ty_ = t % a.tiles_y;
    const int n = t / a.tiles_y;
    tp.oy0 = ty_ * 8; tp.ox0 = tx_ * TW;
    tp.xt = xb + ((size_t)(n * a.H + tp.oy0) * a.W + tp.ox0) * a.Cin * 2;
    tp.dt = db + ((size_t)(n * a.H + tp.oy0) * a.W + tp.ox0) * a.Cout * 2;
    tp.interior = tp.oy0 >= 1 && tp.ox0 >= 1 && tp.oy0 + 9 <= a.H && tp.ox0 + 17 <= a.W;
    return tp;
  };
  auto issue_slot = [&](const TilePos& tp, int stage, int k) {   // k is a compile-time constant at every call site
    if (b.diag & 1) return;                                   // tuning aid: no tile loads
    // two-block mode: ONE stage per tile; group 0 fetches the x halo and its dy block, group 1 only its dy block
    if (cob2 && k < 3 && grp == 1) return;
    const unsigned sbase = lds0 + (cob2 ? stage * W4_STG2 + (k >= 3 ? grp * 8192 : 0) : stage * STG) + w * 1024;
    if (k < 3) {
      bool ok = tp.live && xhy[k] < 16;
      if (!tp.interior) {
        const int vy = tp.oy0 - 1 + xhy[k], vx = tp.ox0 - 1 + xhx[k];
        ok = ok && vy >= 0 && vy < a.H && vx >= 0 && vx < a.W;
      }
      glds16(ok ? tp.xt + xrel[k] : zero, sbase + k * 4096);
    } else {
      const int kk = k - 3;
      bool ok = tp.live;
      if (!tp.interior) ok = ok && tp.oy0 + dty[kk] < a.H && tp.ox0 + dtx[kk] < a.W;
      glds16(ok ? tp.dt + drel[kk] : zero, sbase + XB + kk * 4096);
    }
  };
  auto issue = [&](int tile, int stage) {
    const TilePos tp = locate(tile);
#pragma unroll
    for (int k = 0; k < 5; ++k) issue_slot(tp, stage, k);
  };

  f32x16 acc[3][3], accb;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    accb[r] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc[kh][kw][r] = 0.f;
  }
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int fbase = (8 * (g >> 1) + q) * PP + (16 * (g & 1) + 4 * pp) * 2;   // transposed-read lane base (as v3)
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.0f;

  // tiles of this split: split, split + S, ...; iteration `it` handles the pair (2 it, 2 it + 1), group g its element g
  const int ntl = a.ntiles > split ? (a.ntiles - split + a.S - 1) / a.S : 0;
  const int npair = (ntl + 1) >> 1;
  if (cob2) {
    // ---- one tile per iteration, shared by the two groups ----
#pragma unroll
    for (int s = 0; s < W4_DP2; ++s) issue(split + s * a.S, s);
  } else {
#pragma unroll
  for (int s = 0; s < DP; ++s) issue(split + (2 * s + grp) * a.S, 2 * s + grp);
  }
  // compute(pslot, ft, fstage): 18 (+2) MFMAs of this wave's two output rows of its group's tile in pair slot `pslot`;
  // this wave's five DMA pieces of the future tile `ft` are issued BETWEEN the MFMA groups (one after each halo
  // row, one at the end) instead of in front of them: a wave that queues behind a full memory pipe at a DMA
  // instruction then has MFMAs in flight, and its SIMD partner keeps the matrix pipe busy meanwhile.
  auto compute = [&](int pslot, const TilePos& ft, int fstage) {
    const unsigned char* lA = cob2 ? smem + pslot * W4_STG2 : smem + (2 * pslot + grp) * STG;
    const unsigned char* lD = lA + XB + (cob2 ? grp * 8192 : 0);
    bf16x8 dfr[2];
#pragma unroll
    for (int oi = 0; oi < 2; ++oi) {
      const unsigned char* dptr = lD + fbase + (2 * w + oi) * TW * PP;
      const v4s d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(dptr));
      const v4s d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(dptr + 4 * PP));
      const v8s td = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
      dfr[oi] = __builtin_bit_cast(bf16x8, td);
    }
    if (do_bias) {
      accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[0], ones, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[1], ones, accb, 0, 0, 0);
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {      // halo rows 2w .. 2w+3
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const unsigned char* aptr = lA + fbase + ((2 * w + rr) * HWp + kw) * PP;
        const v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(aptr));
        const v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(aptr + 4 * PP));
        const v8s ta = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        const bf16x8 afr = __builtin_bit_cast(bf16x8, ta);
#pragma unroll
        for (int oi = 0; oi < 2; ++oi) {
          const int kh = rr - oi;          // halo row 2w+rr = output row 2w+oi + kh
          if (kh >= 0 && kh < 3) acc[kh][kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[oi], afr, acc[kh][kw], 0, 0, 0);
        }
      }
      issue_slot(ft, fstage, rr);
    }
    issue_slot(ft, fstage, 4);
  };
  // ONE loop (and one inlined copy of compute(): a second call site doubled the live ranges and spilled) for both
  // modes: pair mode -- slot = pair slot, NPS slots, DP pairs ahead, group g owns stage 2*slot + g and tile 2*it + g;
  // two-block mode -- slot = stage, W4_NST2 stages, W4_DP2 tiles ahead, both groups share tile `it`.
  const int nit = cob2 ? ntl : npair, nslot = cob2 ? W4_NST2 : NPS, ahead = cob2 ? W4_DP2 : DP;
  int ps = 0;                                   // ring slot of iteration `it`
  for (int it = 0; it < nit; ++it) {
    int fs = ps + ahead;
    fs = fs >= nslot ? fs - nslot : fs;
    const int kf = cob2 ? it + ahead : 2 * (it + ahead) + grp;
    const TilePos ft = locate(kf < ntl ? split + kf * a.S : a.ntiles);
    // this wave's pieces of iteration `it` have landed (younger iterations may fly): 5 DMA instructions per wave and
    // iteration, except group 1 in the two-block mode (its two dy instructions only)
    if (!cob2) wait_vmcnt<5 * (DP - 1)>();
    else if (grp == 0) wait_vmcnt<5 * (W4_DP2 - 1)>();
    else wait_vmcnt<2 * (W4_DP2 - 1)>();
    __builtin_amdgcn_s_barrier();         // ... everyone's have, and everyone is done reading the slot refilled below
    // (the second tile of an odd last pair is a tile past the end: all zeros, it adds nothing)
    const int fstage = cob2 ? fs : 2 * fs + grp;
    if (b.diag & 2) {                     // tuning aid: loads only
#pragma unroll
      for (int k = 0; k < 5; ++k) issue_slot(ft, fstage, k);
    } else {
      compute(ps, ft, fstage);
    }
    ps = ps + 1 == nslot ? 0 : ps + 1;
  }
  wait_vmcnt<0>();                        // the zero-page pieces of the tiles past the end
  __syncthreads();                        // every wave is done with the ring: it becomes the reduction scratch

  // ---- sum the eight waves' partial blocks in a fixed order and store the slab ----
  // round 1: waves 4..7 -> images 0..3, waves 0..3 add;  round 2: waves 2,3 -> images 0,1, waves 0,1 add;
  // round 3: waves 0,1 -> images 0,1, every thread adds the two and stores.
  // Image = the block in the order [tap][ci][co quad ^ (ci & 7)][4 co]: a lane's four consecutive output channels
  // (registers 4q .. 4q+3 of a 32x32 accumulator) are one 16-byte LDS access, conflict-free through the XOR; the slab
  // keeps that order (block cc at cc * 9216 floats), wgrad_reduce4_kernel undoes it.
  float* red = reinterpret_cast<float*>(smem);               // up to four fp32 images of 9216 floats
  float* bred = red + 4 * 9216;                               // [8][32] bias partials (1 KiB behind the images)
  const int ci = lane & 31, hsel = lane >> 5;
  auto dump = [&](float* img) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
          *(f32x4*)(img + (kh * 3 + kw) * 1024 + ci * 32 + (((2 * q4 + hsel) ^ (ci & 7)) << 2)) =
              f32x4{acc[kh][kw][4 * q4], acc[kh][kw][4 * q4 + 1], acc[kh][kw][4 * q4 + 2], acc[kh][kw][4 * q4 + 3]};
  };
  auto gather = [&](const float* img) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const f32x4 v = *(const f32x4*)(img + (kh * 3 + kw) * 1024 + ci * 32 + (((2 * q4 + hsel) ^ (ci & 7)) << 2));
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[kh][kw][4 * q4 + j] += v[j];
        }
  };
  if (do_bias && ci == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) bred[w8 * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel] = accb[r];
  }
  if (b.diag & 8) return;
  if (cob2) {
    // the four waves of a group hold partial sums of ONE block (group g: output-channel block 2*cot + g) over different
    // pixel rows: waves 2,3 -> images, waves 0,1 add; wave 1 -> image, wave 0 adds and leaves the total in image g
    if (w >= 2) dump(red + (2 * grp + w - 2) * 9216);
    __syncthreads();
    if (w < 2) gather(red + (2 * grp + w) * 9216);
    __syncthreads();
    if (w == 1) dump(red + grp * 9216);
    __syncthreads();
    if (w == 0) gather(red + grp * 9216);
    __syncthreads();
    if (w == 0) dump(red + grp * 9216);
    __syncthreads();
    // blocks (2*cot, cit) and (2*cot + 1, cit) of the 32 x 32 block grid: ci_tiles blocks apart in the slab
    float* slab2 = a.slab + (size_t)split * a.slab_stride + (size_t)(2 * cot * ci_tiles + cit) * 9216;
    for (int i4 = tid; i4 < 2 * 2304; i4 += 512) {
      const int g2 = i4 >= 2304, j4 = i4 - g2 * 2304;
      *(f32x4*)(slab2 + (size_t)g2 * ci_tiles * 9216 + j4 * 4) = *(const f32x4*)(red + g2 * 9216 + j4 * 4);
    }
    if (do_bias && tid < 64) {
      const int g2 = tid >> 5;
      float sm = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) sm += bred[(g2 * 4 + k) * 32 + (tid & 31)];
      a.slab[(size_t)split * a.slab_stride + (size_t)9 * a.Cout * a.Cin + cot * 64 + tid] = sm;
    }
    return;
  }
  if (!(b.diag & 4)) {
    if (w8 >= 4) dump(red + (w8 - 4) * 9216);
    __syncthreads();
    if (w8 < 4) gather(red + w8 * 9216);
    __syncthreads();
    if (w8 == 2 || w8 == 3) dump(red + (w8 - 2) * 9216);
    __syncthreads();
    if (w8 < 2) gather(red + w8 * 9216);
    __syncthreads();
  }
  if (w8 < 2 && !(b.diag & 32)) dump(red + w8 * 9216);
  __syncthreads();
  float* slab = a.slab + (size_t)split * a.slab_stride + (size_t)cc * 9216;
  if (!(b.diag & 16))
  for (int i4 = tid; i4 < 2304; i4 += 512)
    *(f32x4*)(slab + i4 * 4) = *(const f32x4*)(red + i4 * 4) + *(const f32x4*)(red + 9216 + i4 * 4);
  if (do_bias && tid < 32) {
    float sm = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) sm += bred[k * 32 + tid];
    a.slab[(size_t)split * a.slab_stride + (size_t)9 * a.Cout * a.Cin + co0 + tid] = sm;
  }
}

// =============================================================================================
// v6 (round 3).  A workgroup's EIGHT waves (two per SIMD) each own a whole 32co x 32ci block: all nine taps (9
// accumulators = 144 registers) over ALL pixels of the wave's rows of a tile.  Two shapes (template W6Cfg):
//   A: NCB 4 x NCH 2 x NRG 1 -- 128co x 64ci per workgroup on 4 x 16-pixel tiles (jobs with Cout % 128 == 0, Cin % 64 == 0):
//      wave w8 = output-channel block w8 & 3, input-channel half w8 >> 2;
//   B: NCB 2 x NCH 2 x NRG 2 -- 64co x 64ci per workgroup on 8 x 16-pixel tiles (Cout % 64 == 0, Cin % 64 == 0): the two
//      row groups take output rows 0..3 / 4..7 of the tile and are summed through LDS once, at the end.
// Against v4's split (eight waves = pixel rows of ONE or TWO blocks):
//   * no (A) / one (B) cross-wave reduction round at the end (v4: three rounds);
//   * a stage is 30 KiB (A: 14 KiB of x halo, 6 x 18 pixels x 64 channels + 16 KiB of dy) or 40 KiB (B: 24 + 16) for
//     8 x 36 = 288 MFMAs: 107 / 142 B per MFMA against 199 B in v4's two-block mode and 284 B in its pair mode;
//   * 44 transposing reads per 36 MFMAs per wave (v4: 56 per 18), and the per-tile fixed part (counted wait, barrier,
//     first fragments) is paid once per 36 MFMAs per wave instead of once per 18;
//   * the barrier runs one tile ahead and the first fragments of tile it+1 are read at the end of tile it;
//   * the DMA slot logic is branch-free (see the slot table below).
// Stage image: [x: NCH sub-images [halo pixel ((TH+2) x 18)][32 ci]][dy: NCB sub-images [pixel (TH x 16)][32 co]] --
// every sub-image is the plain [pixel][32 channels] layout the transposing reads of v4 address.  A: 30 DMA instructions
// per stage = 4 per wave with two dummies (zero page -> the stage's 1-KiB sink), ring of four stages, three tiles ahead;
// B: 40 = 5 per wave, ring of three, two ahead.  Slab format = v4's, same reduction kernel.
// MEASURED (MI355X, batch 32, tools/bench_wgrad_v6.py, interleaved with v4 in one process; identical results run to run,
// 2e-7 from torch's fp32 weight gradient like v4): shape A 128->128@32^2 53 -> 38 us, @64^2 88 -> 66, @128^2 229 -> 185
// (675 -> 836 TFLOP/s), 256->256@64^2 225 -> 185; training step (config A, same box) -2.9 %.
// =============================================================================================
template <int NCB_, int NCH_, int NRG_>
struct W6Cfg {
  static constexpr int NCB = NCB_, NCH = NCH_, NRG = NRG_, TH_ = 4 * NRG_, HW_ = TW + 2, NPX = (TH_ + 2) * HW_;
  static constexpr int XI = (NPX + 15) / 16;                 // DMA instructions (16 pixels each) per x sub-image
  static constexpr int XSUB = XI * 1024, XB = NCH * XSUB, DSUB = TH_ * 1024, STG = XB + NCB * DSUB;
  static constexpr int NX = NCH * XI, KX = (NX + 7) / 8, ND = NCB * TH_, KD = ND / 8, NSLOT = KX + KD;
  static constexpr bool SINK = NX % 8 != 0;
  static constexpr int STGS = STG + (SINK ? 1024 : 0);
  // B's fold goes through LDS in two rounds (taps 0..4, 5..8): four 20-KiB half blocks + bias partials.  The ring is
  // kept at <= 124 KiB: a workgroup that takes the whole LDS (v4: 160 KiB) keeps every other kernel off its CU, and the
  // training step runs the data-gradient chain on the other stream (B with a four-stage 160-KiB ring: +0.2 ms per step)
  static constexpr int FOLD = NRG == 2 ? NCB * NCH * 5 * 1024 * 4 + 1024 : 0;
#ifdef W6_NST3
  static constexpr int NST = 3, DP = 2;
#else
  static constexpr int NST = (124 * 1024) / STGS >= 4 ? 4 : 3, DP = NST - 1;
#endif
  static constexpr int LDS = NST * STGS > FOLD ? NST * STGS : FOLD;
  static_assert(NCB * NCH * NRG == 8 && ND % 8 == 0 && LDS <= 160 * 1024 && NSLOT * (DP - 1) <= 63, "v6 shape");
};
using W6A = W6Cfg<4, 2, 1>;
using W6B = W6Cfg<2, 2, 2>;

#ifndef W6_VGPR_ATTR
#define W6_VGPR_ATTR
#endif
template <class C>
__global__ W6_VGPR_ATTR __launch_bounds__(512, 1) void wgrad_mfma6_kernel(W4Batch b) {
  constexpr int PP = 64, HWp = C::HW_;
  const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
  const int ng = b.ngrp[xcd];
  if (ng == 0 || pos >= b.grp_start[xcd][ng]) return;
  int gi = 0;
  while (gi + 1 < ng && pos >= b.grp_start[xcd][gi + 1]) ++gi;
  const unsigned gword = b.grp[xcd][gi];
  const int jb = gword & 15, split = gword >> 4, cc = pos - b.grp_start[xcd][gi];
  const W4Job& a = b.job[jb];
  const int ci_pairs = a.Cin / (32 * C::NCH);
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS];
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = w8 % C::NCB, ch = (w8 / C::NCB) % C::NCH, rg = w8 / (C::NCB * C::NCH);
  const int cotb = cc / ci_pairs, citb = cc % ci_pairs;
  const int co0 = cotb * 32 * C::NCB, ci0 = citb * 32 * C::NCH;
  const bool do_bias = (citb == 0) && (ch == 0);     // wave-uniform

  // ---- DMA slots of this wave (the kind of slot k is the same for every wave: no branch at the issue site) ----
  //   k < KX: x instruction xi = w8 + 8 k = 16 halo pixels (x 4 pieces) of input-channel half xi / XI; an xi past the
  //           last one (shape A: 14, 15) writes 1 KiB of zeros into the stage's sink;
  //   k >= KX: dy instruction di = w8 + 8 (k - KX) = tile row di % TH of output-channel block di / TH.
  // Per lane: pixel coordinates RELATIVE to the tile origin (halo: -1 ..), the byte offset from the tile's first pixel
  // and a validity flag; range checks against the image are done for every piece (4 VALU instructions) -- a separate
  // interior fast path cost more in branches and kernel-argument reloads (s_load + lgkmcnt(0), which also drains the
  // wave's LDS reads) than it saved.
  int H = a.H, W = a.W;
  asm volatile("" : "+s"(H), "+s"(W));          // keep them in SGPRs (otherwise re-read from the kernel arguments per use)
  int ldsoff[C::NSLOT];            // wave-uniform
  int yy[C::NSLOT], xx[C::NSLOT], rel[C::NSLOT];   // per lane
  bool pv[C::NSLOT];
  {
    const int pix = lane >> 2, piece = lane & 3;
#pragma unroll
    for (int k = 0; k < C::KX; ++k) {
      const int xi = w8 + 8 * k;
      const bool sink = xi >= C::NX;
      const int h = xi / C::XI, i = xi - C::XI * h, p = 16 * i + pix;
      ldsoff[k] = sink ? C::STG : h * C::XSUB + i * 1024;
      pv[k] = !sink && p < C::NPX;
      yy[k] = p / HWp - 1;
      xx[k] = p - (p / HWp) * HWp - 1;
      rel[k] = (yy[k] * W + xx[k]) * a.Cin * 2 + (ci0 + h * 32 + piece * 8) * 2;
    }
#pragma unroll
    for (int k = C::KX; k < C::NSLOT; ++k) {
      const int di = w8 + 8 * (k - C::KX), c = di / C::TH_, i = di % C::TH_;
      ldsoff[k] = C::XB + c * C::DSUB + i * 1024;
      pv[k] = true;
      yy[k] = i;
      xx[k] = pix;
      rel[k] = (i * W + pix) * a.Cout * 2 + (co0 + c * 32 + piece * 8) * 2;
    }
#pragma unroll
    for (int k = 0; k < C::NSLOT; ++k) ldsoff[k] = __builtin_amdgcn_readfirstlane(ldsoff[k]);
  }
  const unsigned char* xb = reinterpret_cast<const unsigned char*>(a.x);
  const unsigned char* db = reinterpret_cast<const unsigned char*>(a.dy);
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(pti_wgrad_zero_page);
  struct TilePos { const unsigned char* xt; const unsigned char* dt; int oy0, ox0; };
  auto locate = [&](int tile) -> TilePos {       // (wave-uniform; a tile past the end gets an origin outside every image)
    TilePos tp;
    const bool live = tile < a.ntiles;
    int t = live ? tile : 0;
    const int tx_ = t % a.tiles_x; t /= a.tiles_x;
    const int ty_ = t % a.tiles_y;
    const int n = t / a.tiles_y;
    tp.oy0 = live ? ty_ * C::TH_ : 1 << 24; tp.ox0 = tx_ * TW;
    const size_t pix0 = (size_t)(n * H + ty_ * C::TH_) * W + tp.ox0;
    tp.xt = xb + pix0 * a.Cin * 2;
    tp.dt = db + pix0 * a.Cout * 2;
    return tp;
  };
  auto issue_slot = [&](const TilePos& tp, int stage, int k) {     // k is a compile-time constant at every call site
    if (b.diag & 1) return;                                   // tuning aid (wrong results): no tile loads
    const unsigned sb = __builtin_amdgcn_readfirstlane(lds0 + stage * C::STGS + ldsoff[k]);   // (wave-uniform: M0)
    const bool ok = pv[k] && (unsigned)(tp.oy0 + yy[k]) < (unsigned)H && (unsigned)(tp.ox0 + xx[k]) < (unsigned)W;
    glds16(ok ? (k < C::KX ? tp.xt : tp.dt) + rel[k] : zero, sb);
  };

  f32x16 acc[3][3];
  float bsum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc[kh][kw][r] = 0.f;
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int fbase = (8 * (g >> 1) + q) * PP + (16 * (g & 1) + 4 * pp) * 2;   // transposed-read lane base (as v3 / v4)
  auto tr_frag = [&](const unsigned char* p) -> bf16x8 {
    const v4s d0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(p));
    const v4s d1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(p + 4 * PP));
    const v8s t = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
    return __builtin_bit_cast(bf16x8, t);
  };

  const int ntl = a.ntiles > split ? (a.ntiles - split + a.S - 1) / a.S : 0;
  auto tile_of = [&](int k) { return k < ntl ? split + k * a.S : a.ntiles; };   // (past the end: zeros)
#pragma unroll
  for (int s = 0; s < C::DP; ++s) {
    const TilePos tp = locate(tile_of(s));
#pragma unroll
    for (int k = 0; k < C::NSLOT; ++k) issue_slot(tp, s, k);
  }
  // first fragments of a tile: the four dy fragments of this wave's output rows (row group rg) and output-channel block,
  // and the x fragments 0, 1 (first halo row of the row group, kw 0 and 1) of this wave's input-channel half
  bf16x8 dfr[4], xcur, xq1;
  auto xfrag_at = [&](const unsigned char* lX, int f) { return tr_frag(lX + fbase + ((4 * rg + f / 3) * HWp + f % 3) * PP); };
  auto dfrag_at = [&](const unsigned char* lS, int r) { return tr_frag(lS + C::XB + cb * C::DSUB + fbase + (4 * rg + r) * TW * PP); };
  wait_vmcnt<C::NSLOT * (C::DP - 1)>();   // tile 0 has landed (this wave's pieces) ...
  __builtin_amdgcn_s_barrier();           // ... and everyone's
#pragma unroll
  for (int r = 0; r < 4; ++r) dfr[r] = dfrag_at(smem, r);
  xcur = xfrag_at(smem + ch * C::XSUB, 0);
  xq1 = xfrag_at(smem + ch * C::XSUB, 1);

  int ps = 0;
  for (int it = 0; it < ntl; ++it) {
    int fs = ps + C::DP;
    fs = fs >= C::NST ? fs - C::NST : fs;
    const int ns = ps + 1 == C::NST ? 0 : ps + 1;
    const TilePos ft = locate(tile_of(it + C::DP));
    // tile it+1 has landed for every wave (younger tiles may fly); every wave is also done reading tile it-1's slot,
    // which this iteration refills with tile it+DP
    wait_vmcnt<C::NSLOT * (C::DP - 2)>();
    __builtin_amdgcn_s_barrier();
    const unsigned char* lX = smem + ps * C::STGS + ch * C::XSUB;
    const unsigned char* lN = smem + ns * C::STGS;            // tile it+1: confirmed by the barrier above
    if (b.diag & 2) {                     // tuning aid (wrong results): loads only
#pragma unroll
      for (int k = 0; k < C::NSLOT; ++k) issue_slot(ft, fs, k);
      ps = ns;
      continue;
    }
    if (do_bias) {      // a lane of a dy fragment holds 8 pixels of ONE output channel
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32x4 dwv = __builtin_bit_cast(u32x4, dfr[r]);
        float s8 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) s8 += __uint_as_float(dwv[i] << 16) + __uint_as_float(dwv[i] & 0xffff0000u);
        bsum += s8;
      }
    }
    // 18 x fragments: halo rows 0..5 of the row group (rr) x kw; fragment f+2 is read while fragment f's MFMAs issue.
    // The tile boundary is software-pipelined: the NEXT tile's dy fragments are read during steps 11..14 (their last use
    // in this tile is step 11 + 3 kh... see dlast) and its x fragments 0, 1 take the read slots of steps 16, 17, so the
    // first MFMA of tile it+1 waits for nothing but the barrier.
    bf16x8 dnx[4];
#pragma unroll
    for (int f = 0; f < 18; ++f) {
      const int rr = f / 3, kw = f % 3;
      bf16x8 xq2 = f + 2 < 18 ? xfrag_at(lX, f + 2) : xfrag_at(lN + ch * C::XSUB, f + 2 - 18);
      // dy fragment r is last used at halo row r + 2 (kh = 2), i.e. step 3 (r + 2) + 2: the next tile's fragment r is read
      // one halo row later into its own registers (moved into dfr at the end)
      if (kw == 0 && rr >= 2) dnx[rr - 2] = dfrag_at(lN, rr - 2);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int r = rr - kh;          // halo row rr = output row r + kh
        if (r >= 0 && r < 4) acc[kh][kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[r], xcur, acc[kh][kw], 0, 0, 0);
      }
      // this wave's DMA pieces of tile it+DP, spread over the fragment steps
      if (C::NSLOT == 4) {
        if (f == 2) issue_slot(ft, fs, 0);
        if (f == 6) issue_slot(ft, fs, 1);
        if (f == 10) issue_slot(ft, fs, 2);
        if (f == 14) issue_slot(ft, fs, 3);
      } else {
        if (f == 2) issue_slot(ft, fs, 0);
        if (f == 5) issue_slot(ft, fs, 1);
        if (f == 8) issue_slot(ft, fs, 2);
        if (f == 11) issue_slot(ft, fs, 3);
        if (f == 14) issue_slot(ft, fs, C::NSLOT - 1);
      }
      if (kw == 0 && rr >= 2) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      else __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      {
        const int nm = (rr == 0 || rr == 5) ? 1 : ((rr == 1 || rr == 4) ? 2 : 3);
        if (nm == 3) __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
        else if (nm == 2) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        else __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      xcur = xq1;
      xq1 = xq2;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dfr[r] = dnx[r];
    ps = ns;
  }
  wait_vmcnt<0>();                       // the zero-page pieces of the tiles past the end

  const int ci = lane & 31, hsel = lane >> 5;
  if (do_bias) bsum += __shfl_xor(bsum, 32, 64);      // lanes l and l + 32 hold the two pixel halves of output channel l
  if constexpr (C::NRG == 2) {
    // ---- the two row groups hold partial sums of the same blocks: group 1 -> LDS images, group 0 adds (fixed order) ----
    __syncthreads();                      // every wave is done with the ring: it becomes the reduction scratch
    float* red = reinterpret_cast<float*>(smem) + (cb + C::NCB * ch) * 5120;
    float* bred = reinterpret_cast<float*>(smem) + C::NCB * C::NCH * 5120;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      if (round) __syncthreads();         // group 0 is done reading round 0's images
      if (rg == 1) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
          if ((t < 5) == (round == 0))
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
              *(f32x4*)(red + (t - 5 * round) * 1024 + ci * 32 + (((2 * q4 + hsel) ^ (ci & 7)) << 2)) =
                  f32x4{acc[t / 3][t % 3][4 * q4], acc[t / 3][t % 3][4 * q4 + 1], acc[t / 3][t % 3][4 * q4 + 2], acc[t / 3][t % 3][4 * q4 + 3]};
        if (round == 0 && do_bias && lane < 32) bred[cb * 32 + lane] = bsum;
      }
      __syncthreads();
      if (rg == 0) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
          if ((t < 5) == (round == 0))
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
              const f32x4 v = *(const f32x4*)(red + (t - 5 * round) * 1024 + ci * 32 + (((2 * q4 + hsel) ^ (ci & 7)) << 2));
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[t / 3][t % 3][4 * q4 + j] += v[j];
            }
        if (round == 0 && do_bias && lane < 32) bsum += bred[cb * 32 + lane];
      }
    }
    if (rg == 1) return;
  }
  // ---- a wave owns its 32co x 32ci x 9 block outright: store it in the slab's block order ----
  const int cc32 = (C::NCB * cotb + cb) * (a.Cin / 32) + C::NCH * citb + ch;
  float* blk = a.slab + (size_t)split * a.slab_stride + (size_t)cc32 * 9216;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
        *(f32x4*)(blk + (kh * 3 + kw) * 1024 + ci * 32 + (((2 * q4 + hsel) ^ (ci & 7)) << 2)) =
            f32x4{acc[kh][kw][4 * q4], acc[kh][kw][4 * q4 + 1], acc[kh][kw][4 * q4 + 2], acc[kh][kw][4 * q4 + 3]};
  if (do_bias && lane < 32) a.slab[(size_t)split * a.slab_stride + (size_t)9 * a.Cout * a.Cin + co0 + cb * 32 + lane] = bsum;
}

// Slab reduction of the v4 layout: slab s = [(co,ci) block cc][tap][ci][co quad ^ (ci & 7)][4 co] + Cout bias sums.
// Same fixed-order scheme as wgrad_reduce_kernel (16 float4 columns x 16 slab groups per block).
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(W4Batch b) {
  __shared__ f32x4 red[16][16];
  int jb = 0;
  while (jb + 1 < b.njobs && (int)blockIdx.x >= b.first_rblk[jb + 1]) ++jb;   // block-uniform
  const W4Job& a = b.job[jb];
  const float* __restrict__ slab = a.slab;
  float* __restrict__ dw = b.dw[jb];
  float* __restrict__ dbias = b.dbias[jb];
  const int S = a.S, Cout = a.Cout, Cin = a.Cin, accumulate = b.accumulate[jb];
  const long long stride = a.slab_stride;
  const long long total = (long long)9 * Cout * Cin;
  const int col = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const long long e = ((long long)(blockIdx.x - b.first_rblk[jb]) * 16 + col) * 4;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (e < total + Cout) {
    int k = sg;
    for (; k + 16 < S; k += 32) {
      s0 += *(const f32x4*)(slab + (size_t)k * stride + e);
      s1 += *(const f32x4*)(slab + (size_t)(k + 16) * stride + e);
    }
    if (k < S) s0 += *(const f32x4*)(slab + (size_t)k * stride + e);
  }
  red[sg][col] = s0 + s1;
  __syncthreads();
  if (sg == 0 && e < total + Cout) {
    f32x4 sum = red[0][col];
#pragma unroll
    for (int g = 1; g < 16; ++g) sum += red[g][col];
    if (e < total) {
      const int cc = (int)(e / 9216), i = (int)(e % 9216);
      const int ci_tiles = Cin / 32;
      const int co0 = (cc / ci_tiles) * 32, ci0 = (cc % ci_tiles) * 32;
      const int tap = i >> 10, ci = (i >> 5) & 31, cog = ((i >> 2) & 7) ^ (ci & 7);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t o = ((size_t)(co0 + cog * 4 + j) * Cin + ci0 + ci) * 9 + tap;
        dw[o] = accumulate ? dw[o] + sum[j] : sum[j];
      }
    } else if (dbias) {
      const int co = (int)(e - total);
#pragma unroll
      for (int j = 0; j < 4; ++j) dbias[co + j] = accumulate ? dbias[co + j] + sum[j] : sum[j];
    }
  }
}

// dW[co][ci][tap] (=|+=) sum_s slab[s][tap][co][ci];  dbias[co] (=|+=) sum_s slab[s][KK*Cout*Cin + co]
// block = 16 float4 columns (64 consecutive slab elements) x 16 slab groups: slabs are summed by 16 threads in
// parallel (fixed order => deterministic), folded through LDS, and written by the first group.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, long long stride, int S,
                                                           float* __restrict__ dw, float* __restrict__ dbias, int Cout,
                                                           int Cin, int KK, int accumulate) {
  __shared__ f32x4 red[16][16];
  const long long total = (long long)KK * Cout * Cin;   // + Cout bias entries behind it; both multiples of 4
  const int col = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const long long e = ((long long)blockIdx.x * 16 + col) * 4;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (e < total + Cout) {
    int k = sg;
    for (; k + 16 < S; k += 32) {
      s0 += *(const f32x4*)(slab + (size_t)k * stride + e);
      s1 += *(const f32x4*)(slab + (size_t)(k + 16) * stride + e);
    }
    if (k < S) s0 += *(const f32x4*)(slab + (size_t)k * stride + e);
  }
  red[sg][col] = s0 + s1;
  __syncthreads();
  if (sg == 0 && e < total + Cout) {
    f32x4 sum = red[0][col];
#pragma unroll
    for (int g = 1; g < 16; ++g) sum += red[g][col];
    if (e < total) {
      const int ci = e % Cin;
      const int co = (e / Cin) % Cout;
      const int t = e / ((long long)Cin * Cout);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t o = ((size_t)co * Cin + ci + j) * KK + t;
        dw[o] = accumulate ? dw[o] + sum[j] : sum[j];
      }
    } else if (dbias) {
      const int co = (int)(e - total);
#pragma unroll
      for (int j = 0; j < 4; ++j) dbias[co + j] = accumulate ? dbias[co + j] + sum[j] : sum[j];
    }
  }
}

template <int KS, int S_, int CO_T, int CI_T>
void launch_w(const WgArgs& a, int grid_y, hipStream_t st) {
  if (a.prologue == PTI_PRO_NONE)
    PTI_LAUNCH((wgrad_mfma_kernel<KS, S_, CO_T, CI_T, true>), dim3(grid_y, a.S), dim3(256), 0, st, a);
  else
    PTI_LAUNCH((wgrad_mfma_kernel<KS, S_, CO_T, CI_T, false>), dim3(grid_y, a.S), dim3(256), 0, st, a);
}
template <int KS, int S_>
void launch_wt(const WgArgs& a, int co_t, int ci_t, int grid_y, hipStream_t st) {
  if (co_t == 64 && ci_t == 64) launch_w<KS, S_, 64, 64>(a, grid_y, st);
  else if (co_t == 64) launch_w<KS, S_, 64, 32>(a, grid_y, st);
  else if (ci_t == 64) launch_w<KS, S_, 32, 64>(a, grid_y, st);
  else launch_w<KS, S_, 32, 32>(a, grid_y, st);
}

}  // namespace

// ---- v4 batch planning (host) -------------------------------------------------------------------------------------
// Kernel mode of a job (W4Job::cob2): 0 = pairs of tiles, 32co x 32ci per workgroup; 1 = two output-channel blocks per
// workgroup (Cout % 64 == 0); the v6 kernel: 2 = shape A, 128co x 64ci per workgroup on 4 x 16-pixel tiles (Cout % 128 ==
// 0 and Cin % 64 == 0), 3 = shape B, 64co x 64ci on 8 x 16-pixel tiles (Cout % 64 == 0 and Cin % 64 == 0).
// PTI_WGRAD_V6 (read per call: the A/B tool toggles it inside one process): 0 = never, 1 = shape A only, 2 = A and B
// wherever they fit, 3 (the default) = A, and B for layers on maps of at most 128 x 128 pixels.
// Shape B is 20-28 % faster than v4's two-block mode launch for launch (64->64@128^2 80 -> 57 us, @256^2 216 -> 166 us =
// 933 TFLOP/s).  Inside the training step (same-box interleaved A/Bs, final kernels, 256-MB workspace) it is worth
// -0.7..0.9 % on config A (its 64-channel layers sit at 128^2) and -1.1 % with three image channels, and COSTS +2..3.5 %
// on the AR model at batch 8 and 32, whose 64-channel layers are its FIRST level (256^2): those jobs run beside the
// HBM-bound first-level data-gradient chain on the other stream (and launch for launch B wins there too, 78 -> 56 us at
// batch 8), so the faster kernel takes bandwidth from the critical path.  Hence the map-size rule.  (With round 2's
// 48-MB workspace split three ways, B lost on config A as well.)
static int w6_mode(int n, int h, int w, int cin, int cout) {
  const char* e = getenv("PTI_WGRAD_V6");
  const int v = e ? atoi(e) : 3;
  if (v >= 1 && cout % 128 == 0 && cin % 64 == 0) return 2;
  if (v >= 2 && cout % 64 == 0 && cin % 64 == 0 && (v == 2 || (long long)h * w <= 128 * 128)) return 3;
  return 0;
}
static void w4_fill_job(W4Job& a, const void* x, const void* dy, int n, int h, int w, int cin, int cout, int mode) {
  a.x = (const bf16*)x; a.dy = (const bf16*)dy; a.slab = nullptr;
  a.N = n; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout;
  a.tiles_x = cdiv(w, TW); a.tiles_y = cdiv(h, mode == 2 ? W6A::TH_ : TH); a.ntiles = n * a.tiles_x * a.tiles_y;
  a.slab_stride = (long long)9 * cout * cin + cout;
  a.S = 1;
  a.cob2 = mode;
}
static bool w4_eligible(int n, int h, int w, int cin, int cout) {
  return n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0 &&
         (long long)n * h * w * cin * 2 < (1ll << 31) && (long long)n * h * w * cout * 2 < (1ll << 31);
}
// Mode of a job that the v6 rule leaves to the v4 kernel (pti_conv_wgrad_reduce fills its job with this one only).
static int w4_mode(int cout) {
  static const int cob2_env = getenv("PTI_WGRAD_V4_COB2") ? atoi(getenv("PTI_WGRAD_V4_COB2")) : 1;
  return (cob2_env && cout % 64 == 0) ? 1 : 0;
}
// The one place a job's kernel mode is decided; < 0: not a v4 / v6 job at all.  Host arithmetic only.
extern "C" int pti_conv_wgrad_batched_mode(int n, int h, int w, int cin, int cout) {
  if (!w4_eligible(n, h, w, cin, cout)) return PTI_EUNSUPPORTED;
  const int v4 = w4_mode(cout), v6 = w6_mode(n, h, w, cin, cout);
  return v6 ? v6 : v4;
}
// Tuning aid that yields GARBAGE results (see WgArgs::diag): honoured only together with the explicit second opt-in
// PTI_ALLOW_WRONG_RESULTS=1, and announced on stderr; bench.py / train_vae.py refuse to run with either variable set.
static int wgrad_diag_env() {
  const char* v = getenv("PTI_WGRAD_V4_DIAG");
  const char* ok = getenv("PTI_ALLOW_WRONG_RESULTS");
  if (!v || atoi(v) == 0) return 0;
  if (!ok || atoi(ok) != 1) {
    fprintf(stderr, "[pti] PTI_WGRAD_V4_DIAG ignored: it needs PTI_ALLOW_WRONG_RESULTS=1 (results are garbage)\n");
    return 0;
  }
  fprintf(stderr, "[pti] WRONG-RESULT DIAGNOSTIC ACTIVE: PTI_WGRAD_V4_DIAG=%s\n", v);
  return atoi(v);
}
// Pixel splits per job so that every workgroup of the launch streams about the same number of tiles and the launch has
// about `wgs` workgroups; slab carving; reduction-block ranges; the XCD group lists.  One workgroup is resident per
// CU (it owns the whole LDS); ~2048 workgroups (planned; the 256-group cap usually binds first) measured best inside the training step, where the launch
// shares the chip with the data-gradient chain on the other stream (same-box A/B: 256 13.45, 512 13.07, 1024 12.90,
// 2048 12.73..12.87 ms per step); the 256-group cap of the XCD lists bounds it from above.
// Returns the floats of workspace used, or -1 if it does not fit.
static long long w4_plan(W4Batch& b, float* workspace, long long workspace_floats) {
  static const int wgs_env = getenv("PTI_WGRAD_V4_WGS") ? atoi(getenv("PTI_WGRAD_V4_WGS")) : 2048;
  static const int diag_env = wgrad_diag_env();
  b.diag = diag_env;
  // workgroups of one pixel split: (co, ci) blocks of 32 x 32, or of 64 x 32 in the two-block mode
  auto tiles32 = [](const W4Job& a) {
    return a.cob2 == 2 ? (a.Cin / 64) * (a.Cout / 128) : a.cob2 == 3 ? (a.Cin / 64) * (a.Cout / 64)
                                                                     : (a.Cin / 32) * (a.Cout / (a.cob2 ? 64 : 32));
  };
  // v6 batches (every job in mode 2): a workgroup writes EIGHT 37-KB blocks, so the launch aims at fewer, longer
  // workgroups (PTI_WGRAD_V6_WGS, default 512 = two rounds per CU); work is counted in workgroup-tiles
  const bool m6 = b.njobs > 0 && b.job[0].cob2 >= 2;
  const char* w6e = getenv("PTI_WGRAD_V6_WGS");
  const int wgs6 = w6e && atoi(w6e) > 0 ? atoi(w6e) : 512;
  double work = 0;   // 32 x 32-block tiles of the whole launch (a two-block workgroup does two per pixel tile)
  for (int j = 0; j < b.njobs; ++j) work += (double)tiles32(b.job[j]) * (b.job[j].cob2 == 1 ? 2 : 1) * b.job[j].ntiles;
  double per_wg = work / wgs_env > 2.0 ? work / wgs_env : 2.0;   // tiles per workgroup aimed at (at least one pair)
  if (m6) per_wg = work / wgs6 > 4.0 ? work / wgs6 : 4.0;
  for (int attempt = 0;; ++attempt) {
    long long used = 0;
    int rb = 0, groups = 0;
    bool fits = true;
    for (int j = 0; j < b.njobs; ++j) {
      W4Job& a = b.job[j];
      // per_wg = pixel tiles per workgroup in the pair mode (two per iteration); a two-block workgroup takes one pixel
      // tile per iteration, so the same running time is per_wg / 2 pixel tiles: twice the splits
      int S = (int)((double)a.ntiles * (a.cob2 == 1 ? 2 : 1) / per_wg + 0.5);
      if (S > a.ntiles / (a.cob2 ? 1 : 2)) S = a.ntiles / (a.cob2 ? 1 : 2);
      if (S > 255) S = 255;
      if (S < 1) S = 1;
      if (used + (long long)S * a.slab_stride > workspace_floats) fits = false;
      a.S = S;
      a.slab = workspace + used;
      used += (long long)S * a.slab_stride;
      groups += S;
      b.first_rblk[j] = rb;
      rb += (int)((a.slab_stride / 4 + 15) / 16);
    }
    b.first_rblk[b.njobs] = rb;
    if (fits && groups <= 8 * W4_MAXGRP) {
      // deal the groups over the XCDs: biggest first onto the currently shortest list
      int len[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int x = 0; x < 8; ++x) { b.ngrp[x] = 0; b.grp_start[x][0] = 0; }
      int order[PTI_WGRAD_BATCH_MAX];
      for (int j = 0; j < b.njobs; ++j) order[j] = j;
      for (int i = 0; i < b.njobs; ++i)
        for (int j = i + 1; j < b.njobs; ++j)
          if (tiles32(b.job[order[j]]) > tiles32(b.job[order[i]])) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
      bool ok = true;
      for (int i = 0; i < b.njobs && ok; ++i) {
        const int j = order[i];
        for (int sp = 0; sp < b.job[j].S; ++sp) {
          int best = 0;
          for (int x = 1; x < 8; ++x)
            if (len[x] < len[best]) best = x;
          if (b.ngrp[best] >= W4_MAXGRP || len[best] + tiles32(b.job[j]) > 65535) { ok = false; break; }
          b.grp[best][b.ngrp[best]] = (unsigned short)((unsigned)j | ((unsigned)sp << 4));
          len[best] += tiles32(b.job[j]);
          b.grp_start[best][++b.ngrp[best]] = (unsigned short)len[best];
        }
      }
      if (ok) {
        int mx = 0;
        for (int x = 0; x < 8; ++x) mx = len[x] > mx ? len[x] : mx;
        b.nwg = 8 * mx;
        return used;
      }
    }
    if (attempt > 40) return -1;
    per_wg *= 1.25;   // fewer, longer splits
  }
}

extern "C" int64_t pti_conv_wgrad_workspace_bytes(int cout, int cin, int ksize, int splits) {
  return (int64_t)splits * ((int64_t)ksize * ksize * cout * cin + cout) * 4;
}

static int wgrad_check(const void* x, const void* dy, const int64_t* in_stats, const float* gamma, const float* beta,
                       const void* workspace, const pti_conv_desc* d) {
  if (!x || !dy || !workspace || !d) PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma: null pointer");
  if (d->cin % 32 || d->cout % 32) PTI_FAIL(PTI_EUNSUPPORTED, "conv_wgrad_mfma: cin=%d cout=%d", d->cin, d->cout);
  if (d->ksize != 1 && d->ksize != 3) PTI_FAIL(PTI_EUNSUPPORTED, "conv_wgrad_mfma: ksize");
  if (d->mode == PTI_CONV_ZINS || (d->ksize == 1 && d->mode != PTI_CONV_S1)) PTI_FAIL(PTI_EUNSUPPORTED, "conv_wgrad_mfma: mode %d", d->mode);
  if (d->prologue != PTI_PRO_NONE && (!in_stats || !gamma || !beta || d->groups <= 0 || d->cin % d->groups))
    PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma: prologue args");
  return PTI_OK;
}

extern "C" int pti_conv_wgrad_mfma_partials(const void* x, const void* dy, const int64_t* in_stats, const float* gamma,
                                            const float* beta, void* workspace, int64_t workspace_bytes,
                                            const pti_conv_desc* d, int* splits_out, pti_stream_t s) {
  if (!splits_out) PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma_partials: null splits_out");
  if (int rc = wgrad_check(x, dy, in_stats, gamma, beta, workspace, d)) return rc;
  WgArgs a;
  a.x = (const bf16*)x; a.dy = (const bf16*)dy; a.in_stats = (const stat_t*)in_stats; a.gamma = gamma; a.beta = beta;
  a.slab = (float*)workspace;
  a.N = d->n; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.Ho = d->ho; a.Wo = d->wo; a.Cout = d->cout;
  a.mode = d->mode; a.prologue = d->prologue; a.groups = d->groups; a.eps = d->eps; a.x_f16 = d->in_f16;
  static const int diag_env = wgrad_diag_env();
  a.diag = diag_env;
  a.inv_cnt = d->prologue != PTI_PRO_NONE ? 1.0f / ((float)(d->cin / d->groups) * (float)d->h * (float)d->w) : 0.f;
  a.tiles_x = cdiv(d->wo, TW); a.tiles_y = cdiv(d->ho, TH); a.ntiles = d->n * a.tiles_x * a.tiles_y;
  // Tile / split choice.  3x3 stride-1 gathers: the tap-split 32x32 kernel (v3, measured faster on every such
  // shape).  Others (1x1, stride 2): 64x64 (co,ci) tiles only when every workgroup still gets >= 16 pixel tiles at
  // ~512 workgroups, otherwise 32x32 so that fewer, longer splits keep the partial-slab traffic (S x dW) small.
  int co_t = d->cout % 64 == 0 ? 64 : 32, ci_t = d->cin % 64 == 0 ? 64 : 32;
  if ((long long)a.ntiles * (d->cout / co_t) * (d->cin / ci_t) < 16 * 512) co_t = ci_t = 32;
  const bool v3 = d->ksize == 3 && d->mode != PTI_CONV_S2PAD;
  // Two co blocks per workgroup when the GroupNorm+SiLU prologue runs in the loader (it is then done once per 64
  // output channels: 64->64@128^2 129 -> 96 us, 128->128@64^2 125 -> 94 us).  On saved, already activated inputs
  // (the training step's default) it measured 69.2 -> 67.2 / 68.0 -> 66.3 us in isolation but +0.7 % per step when
  // overlapped with the data-gradient chain (2 waves/SIMD co-schedule worse), and the nearest-2x gather ran 3-10 %
  // slower with it: those keep one block.  PTI_WGRAD_COB=1|2 forces the choice (tuning knob).
  static const int cob_env = getenv("PTI_WGRAD_COB") ? atoi(getenv("PTI_WGRAD_COB")) : 0;
  const bool cob_ok = d->cout % 64 == 0 && d->mode == PTI_CONV_S1;
  const int cob = (cob_ok && cob_env != 1 && (cob_env == 2 || d->prologue != PTI_PRO_NONE)) ? 2 : 1;
  if (v3) { ci_t = 32; co_t = 32 * cob; }
  a.ci_tiles = d->cin / ci_t;
  const int tiles_cc = (d->cout / co_t) * a.ci_tiles;
  const int kk = d->ksize * d->ksize;
  a.slab_stride = (long long)kk * d->cout * d->cin + d->cout;
  const long long smax = workspace_bytes / (a.slab_stride * 4);
  // v3: three waves per workgroup; 768 workgroups = 3 per CU measured best (512 .. 2048 within +-8 %: fewer
  // workgroups mean fewer 37-KB partial slabs to write and reduce, more mean more loads in flight); with two co
  // blocks (2 waves/SIMD) 512 = 2 per CU (768 / 1024: +25 %, 384: +17 %)
  // inputs without a prologue: the loader-free instantiation fits 128
  // VGPRs = 4 waves/SIMD, and with 1280 workgroups (5 per CU) more tiles are in flight per CU -- the kernel is bound by
  // load latency x bytes in flight: 64->64@128^2 70.3 -> 64.2 us, 128->128@64^2 70.5 -> 62.7 us, nearest-2x 64->64 231
  // -> 202 us; the single-block 32->32@256^2 shape 89.0 -> 82.5 us with 1024 workgroups (768: 83.3, 1152: 83.9).
  const bool plain = d->prologue == PTI_PRO_NONE && cob == 1;
  // 1x1 / stride-2 launches (v1 kernel): 512 workgroups by default; PTI_WGRAD_V1_WGS overrides (tuning)
  static const int v1_wgs = getenv("PTI_WGRAD_V1_WGS") ? atoi(getenv("PTI_WGRAD_V1_WGS")) : 512;
  int S = (v3 ? (cob == 2 ? 512 : (plain ? (tiles_cc == 1 ? 1024 : 1280) : 768)) : v1_wgs) / tiles_cc;
  if (S > a.ntiles / 4) S = a.ntiles / 4;
  const int scap = v3 ? (plain ? 1024 : 512) : 256;
  if (S > scap) S = scap;
  if (S < 1) S = 1;
  if (S > smax) S = (int)smax;
  if (S < 1) PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma: workspace too small (%lld bytes per split needed)", a.slab_stride * 4);
  // v4 (LDS-DMA ring, one workgroup per CU): saved bf16 inputs of plain stride-1 3x3 convs.  PTI_WGRAD_V4=0 restores
  // v3; PTI_WGRAD_V4_WGS sets the workgroup count a launch aims at (default 256).
  static const int v4_env = getenv("PTI_WGRAD_V4") ? atoi(getenv("PTI_WGRAD_V4")) : 1;
  const bool v4 = v3 && v4_env && d->prologue == PTI_PRO_NONE && !d->in_f16 && d->mode == PTI_CONV_S1 &&
                  w4_eligible(d->n, d->h, d->w, d->cin, d->cout);
  if (v4) {
    W4Batch b;
    b.njobs = 1;
    w4_fill_job(b.job[0], x, dy, d->n, d->h, d->w, d->cin, d->cout, pti_conv_wgrad_batched_mode(d->n, d->h, d->w, d->cin, d->cout));
    b.dw[0] = b.dbias[0] = nullptr;
    b.accumulate[0] = 0;
    if (w4_plan(b, (float*)workspace, workspace_bytes / 4) < 0)
      PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma: workspace too small (%lld bytes per split needed)", a.slab_stride * 4);
    if (b.job[0].cob2 == 2) PTI_LAUNCH(wgrad_mfma6_kernel<W6A>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b);
    else if (b.job[0].cob2 == 3) PTI_LAUNCH(wgrad_mfma6_kernel<W6B>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b);
    else if (b.job[0].cob2) PTI_LAUNCH(wgrad_mfma4_kernel<true>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b);
    else PTI_LAUNCH(wgrad_mfma4_kernel<false>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b);
    PTI_CHECK_LAUNCH("conv_wgrad_mfma");
    *splits_out = b.job[0].S | PTI_WGRAD_SLAB_V4;   // the reduction must know the slab layout
    return PTI_OK;
  }
  if (v3 && S >= 8) S &= ~7;   // whole rounds over the 8 XCDs (see the block-order note in the kernel)
  a.S = S;
  hipStream_t st = (hipStream_t)s;
  if (v3 && cob == 2) PTI_LAUNCH((wgrad_mfma3_kernel<2, false>), dim3(tiles_cc * S), dim3(192), 0, st, a);
  else if (v3 && plain) PTI_LAUNCH((wgrad_mfma3_kernel<1, true>), dim3(tiles_cc * S), dim3(192), 0, st, a);
  else if (v3) PTI_LAUNCH((wgrad_mfma3_kernel<1, false>), dim3(tiles_cc * S), dim3(192), 0, st, a);
  else if (d->ksize == 1) launch_wt<1, 1>(a, co_t, ci_t, tiles_cc, st);
  else launch_wt<3, 2>(a, co_t, ci_t, tiles_cc, st);
  PTI_CHECK_LAUNCH("conv_wgrad_mfma");
  *splits_out = S;
  return PTI_OK;
}

extern "C" int pti_conv_wgrad_reduce(const void* workspace, int splits, float* dw, float* dbias, int accumulate,
                                     const pti_conv_desc* d, pti_stream_t s) {
  if (!workspace || !dw || !d || splits < 1) PTI_FAIL(PTI_EINVAL, "conv_wgrad_reduce: bad arguments");
  const int kk = d->ksize * d->ksize;
  const long long total = (long long)kk * d->cout * d->cin + d->cout;
  if (splits & PTI_WGRAD_SLAB_V4) {
    if (kk != 9 || !w4_eligible(d->n, d->h, d->w, d->cin, d->cout)) PTI_FAIL(PTI_EINVAL, "conv_wgrad_reduce: block-ordered slabs are 3x3 only");
    W4Batch b;
    b.njobs = 1;
    w4_fill_job(b.job[0], nullptr, nullptr, d->n, d->h, d->w, d->cin, d->cout, w4_mode(d->cout));
    b.job[0].S = splits & ~PTI_WGRAD_SLAB_V4;
    b.job[0].slab = (float*)workspace;
    b.dw[0] = dw; b.dbias[0] = dbias; b.accumulate[0] = accumulate;
    b.diag = 0; b.nwg = 0;
    for (int x = 0; x < 8; ++x) b.ngrp[x] = 0;
    b.first_rblk[0] = 0;
    b.first_rblk[1] = (int)((total / 4 + 15) / 16);
    PTI_LAUNCH(wgrad_reduce4_kernel, dim3(b.first_rblk[1]), dim3(256), 0, (hipStream_t)s, b);
    PTI_CHECK_LAUNCH("conv_wgrad_reduce");
    return PTI_OK;
  }
  PTI_LAUNCH(wgrad_reduce_kernel, dim3((unsigned)((total / 4 + 15) / 16)), dim3(256), 0, (hipStream_t)s,
                     (const float*)workspace, total, splits, dw, dbias, d->cout, d->cin, kk, accumulate);
  PTI_CHECK_LAUNCH("conv_wgrad_reduce");
  return PTI_OK;
}

extern "C" int pti_conv_wgrad_mfma(const void* x, const void* dy, const int64_t* in_stats, const float* gamma,
                                   const float* beta, float* dw, float* dbias, void* workspace,
                                   int64_t workspace_bytes, int accumulate, const pti_conv_desc* d, pti_stream_t s) {
  if (!dw) PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma: null pointer");
  int splits = 0;
  if (int rc = pti_conv_wgrad_mfma_partials(x, dy, in_stats, gamma, beta, workspace, workspace_bytes, d, &splits, s)) return rc;
  return pti_conv_wgrad_reduce(workspace, splits, dw, dbias, accumulate, d, s);
}

extern "C" int pti_conv_wgrad_mfma_batched(const pti_wgrad_job* jobs, int njobs, void* workspace, int64_t workspace_bytes,
                                           pti_stream_t s) {
  if (!jobs || !workspace || njobs < 1 || njobs > PTI_WGRAD_BATCH_MAX)
    PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma_batched: 1..%d jobs", PTI_WGRAD_BATCH_MAX);
  // one batch per kernel mode (see w4_fill_job); each gets its own launch pair and its own part of the workspace
  W4Batch bm[4];
  bm[0].njobs = bm[1].njobs = bm[2].njobs = bm[3].njobs = 0;
  for (int j = 0; j < njobs; ++j) {
    const pti_wgrad_job& q = jobs[j];
    if (!q.x || !q.dy || !q.dw) PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma_batched: job %d has a null pointer", j);
    const int mode = pti_conv_wgrad_batched_mode(q.n, q.h, q.w, q.cin, q.cout);
    if (mode < 0)
      PTI_FAIL(PTI_EUNSUPPORTED, "conv_wgrad_mfma_batched: job %d: n=%d h=%d w=%d cin=%d cout=%d (channels must be multiples of 32, tensors < 2 GiB)",
               j, q.n, q.h, q.w, q.cin, q.cout);
    W4Job jb;
    w4_fill_job(jb, q.x, q.dy, q.n, q.h, q.w, q.cin, q.cout, mode);
    W4Batch& b = bm[mode];
    const int k = b.njobs++;
    b.job[k] = jb;
    b.dw[k] = q.dw; b.dbias[k] = q.dbias; b.accumulate[k] = q.accumulate;
  }
  float* ws = (float*)workspace;
  long long ws_floats = workspace_bytes / 4;
  const void* main_kernel = nullptr;
  // every batch gets the share of the workspace that its one-split-per-job minimum has in the call's (the same average
  // number of splits per job everywhere; what a batch does not use goes to the next one)
  long long need[4] = {0, 0, 0, 0}, need_all = 0;
  for (int m = 0; m < 4; ++m) {
    for (int j = 0; j < bm[m].njobs; ++j) need[m] += bm[m].job[j].slab_stride;
    need_all += need[m];
  }
  if (need_all > ws_floats) PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma_batched: workspace too small (%lld bytes needed for one split per job)", need_all * 4);
  const long long ws_total = ws_floats;
  for (int m = 3; m >= 0; --m) {      // the v6 batches and the widest blocks first
    W4Batch& b = bm[m];
    if (b.njobs == 0) continue;
    long long later = 0;
    for (int m2 = m - 1; m2 >= 0; --m2) later += need[m2];
    long long avail = (long long)((double)ws_total * ((double)need[m] / (double)need_all));
    if (avail < need[m]) avail = need[m];
    if (later == 0 || avail > ws_floats - later) avail = ws_floats - later;
    const long long used = w4_plan(b, ws, avail);
    if (used < 0) PTI_FAIL(PTI_EINVAL, "conv_wgrad_mfma_batched: workspace too small");
    ws += used;
    ws_floats -= used;
    const void* kfn;
    if (m == 3) { PTI_LAUNCH(wgrad_mfma6_kernel<W6B>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b); kfn = reinterpret_cast<const void*>(wgrad_mfma6_kernel<W6B>); }
    else if (m == 2) { PTI_LAUNCH(wgrad_mfma6_kernel<W6A>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b); kfn = reinterpret_cast<const void*>(wgrad_mfma6_kernel<W6A>); }
    else if (m == 1) { PTI_LAUNCH(wgrad_mfma4_kernel<true>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b); kfn = reinterpret_cast<const void*>(wgrad_mfma4_kernel<true>); }
    else { PTI_LAUNCH(wgrad_mfma4_kernel<false>, dim3(b.nwg), dim3(512), 0, (hipStream_t)s, b); kfn = reinterpret_cast<const void*>(wgrad_mfma4_kernel<false>); }
    PTI_CHECK_LAUNCH("conv_wgrad_mfma_batched");
    if (!main_kernel) main_kernel = kfn;
    PTI_LAUNCH(wgrad_reduce4_kernel, dim3(b.first_rblk[b.njobs]), dim3(256), 0, (hipStream_t)s, b);
    PTI_CHECK_LAUNCH("conv_wgrad_mfma_batched reduce");
  }
  pti_last_kernel = main_kernel;      // pti_last_kernel_name(): the call's main kernel
  return PTI_OK;
}
