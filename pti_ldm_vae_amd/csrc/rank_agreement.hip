// Attribute-ordering report of an AR-VAE on the device (gfx950): over ALL n (n - 1) / 2 unordered image pairs, for every
// (attribute q, latent channel c), how many pairs the channel orders like the attribute (concordant), the other way
// (discordant) or ties -- the five classes of include/pti_vae.h -- plus the full-set sum of the very summand
// pti_ar_vae_loss minimises per batch of 8.  (tests/ar_report_oracle.py is the plain restatement.)
//
// Launch 1, one workgroup per (256 x 256 tile of the upper triangle, group of RA_QB attributes).  Thread t owns row
// i = 256 ti + t; the j-tile's columns of z and of the group's attributes are staged in LDS once and read back as
// broadcast 16-byte loads, four j per read.  Signs are taken with compares (never a subtraction: the library is built
// with -ffast-math) and ENCODED so that one 24-bit multiply-add per (q, c) classifies the pair:
//     A = a_j > a_i ? 1 : a_j < a_i ? 2^11 : 0,   Z likewise from z,   acc[q][c] += A * Z
// A * Z is 1 (both up), 2^22 (both down) -- concordant -- or 2^11 (discordant), 0 when either side ties, so three bit
// fields of acc count them: at most 256 pairs per thread and tile, which 10 / 11 / 11 bits hold.  A column of Z = 1 and a
// row of A = 1 ride along; they give sum |sa| (per q), sum |sz| (per c) and the number of pairs, from which the three tie
// classes follow:  z_tied = sum|sa| - (C + D),  a_tied = sum|sz| - (C + D),  both = pairs - sum|sa| - sum|sz| + (C + D).
// A pair that is not one (i >= j, or either index >= n) gets A = 0 in every row and so counts nowhere.
// The loss summand (tanh(delta (z_j - z_i)) - sign(a_j - a_i))^2 is formed in fp64 from the fp32 inputs.
// Every thread's counts are unpacked, folded over the wave by shuffles and over the four waves through LDS, and stored
// as the workgroup's partial.  Launch 2 adds the partials of all tiles in one fixed order (int64 / fp64): no atomics,
// bitwise reproducible, nothing but the caller's stream.
#include <math.h>

#include "pti_common.h"

namespace {

constexpr int RA_TILE = 256;                       // rows per workgroup = columns per tile = threads
constexpr int RA_QB = 4;                           // attributes per workgroup
constexpr int RA_MAXL = 16, RA_MAXNA = 16, RA_MAXN = 32768;
constexpr unsigned RA_DOWN = 1u << 11;             // code of a negative sign
constexpr int RA_SLOT = (RA_QB + 1) * (RA_MAXL + 1) * 2;   // int32 {C, D} per workgroup, laid out for its own LP
constexpr int RA_FOLD_THREADS = 256;

struct RaArgs {
  const float* zt;
  const float* attrs;
  long long ldz, lda;
  int n, l, na, tiles, groups, npairs;
  int channels[RA_MAXNA];
  float deltas[RA_MAXNA];
  double* ws_loss;   // [npairs * groups][RA_QB]
  int* ws_cnt;       // [npairs * groups][RA_SLOT]
  long long* counts;
  double* loss_sum;
};

__device__ __forceinline__ unsigned ra_code(float vj, float vi) { return (vj > vi ? 1u : 0u) | (vj < vi ? RA_DOWN : 0u); }

// LP: the channel count rounded up to a multiple of 4; the padding channels are zeros on both sides (Z = 0)
template <int LP>
__global__ __launch_bounds__(RA_TILE) void rank_agreement_tile_kernel(RaArgs g) {
  __shared__ __attribute__((aligned(16))) float s_z[LP][RA_TILE];
  __shared__ __attribute__((aligned(16))) float s_a[RA_QB][RA_TILE];
  __shared__ int s_red[RA_TILE / 64][(RA_QB + 1) * (LP + 1) * 2];
  __shared__ double s_loss[RA_TILE / 64][RA_QB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * RA_QB;
  int ti = 0, tj = blockIdx.x;   // row ti of the triangle holds tiles - ti entries
  while (tj >= g.tiles - ti) {
    tj -= g.tiles - ti;
    ++ti;
  }
  tj += ti;
  const int i = ti * RA_TILE + tid, j0 = tj * RA_TILE;
  const bool ivalid = i < g.n;

  {   // stage column j0 + tid of the tile
    const int j = j0 + tid;
#pragma unroll
    for (int c = 0; c < LP; ++c) s_z[c][tid] = (c < g.l && j < g.n) ? g.zt[c * g.ldz + j] : 0.0f;
#pragma unroll
    for (int k = 0; k < RA_QB; ++k) s_a[k][tid] = (q0 + k < g.na && j < g.n) ? g.attrs[(q0 + k) * g.lda + j] : 0.0f;
  }
  float zi[LP], ai[RA_QB], zli[RA_QB];
  double dl[RA_QB], lacc[RA_QB];
  int ch[RA_QB];
#pragma unroll
  for (int c = 0; c < LP; ++c) zi[c] = (c < g.l && ivalid) ? g.zt[c * g.ldz + i] : 0.0f;
#pragma unroll
  for (int k = 0; k < RA_QB; ++k) {
    const bool has = q0 + k < g.na;
    ai[k] = (has && ivalid) ? g.attrs[(q0 + k) * g.lda + i] : 0.0f;
    ch[k] = has ? g.channels[q0 + k] : -1;
    dl[k] = has ? (double)g.deltas[q0 + k] : 0.0;
    zli[k] = (ch[k] >= 0 && ivalid) ? g.zt[ch[k] * g.ldz + i] : 0.0f;
    lacc[k] = 0.0;
  }
  unsigned acc[RA_QB + 1][LP + 1];
#pragma unroll
  for (int k = 0; k <= RA_QB; ++k)
#pragma unroll
    for (int c = 0; c <= LP; ++c) acc[k][c] = 0u;
  __syncthreads();

  const int jend = min(RA_TILE, g.n - j0);   // block-uniform; columns past it are staged as zeros and masked below
  for (int jb = 0; jb < jend; jb += 4) {
    f32x4 zj[LP], aj[RA_QB];
#pragma unroll
    for (int c = 0; c < LP; ++c) zj[c] = *(const f32x4*)&s_z[c][jb];
#pragma unroll
    for (int k = 0; k < RA_QB; ++k) aj[k] = *(const f32x4*)&s_a[k][jb];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + jb + u;
      const unsigned vm = (ivalid && j > i && j < g.n) ? 0xffffffffu : 0u;
      unsigned a_code[RA_QB + 1], z_code[LP + 1];
#pragma unroll
      for (int k = 0; k < RA_QB; ++k) a_code[k] = ra_code(aj[k][u], ai[k]) & vm;
      a_code[RA_QB] = vm & 1u;
#pragma unroll
      for (int c = 0; c < LP; ++c) z_code[c] = ra_code(zj[c][u], zi[c]);
      z_code[LP] = 1u;
#pragma unroll
      for (int k = 0; k <= RA_QB; ++k)
#pragma unroll
        for (int c = 0; c <= LP; ++c) acc[k][c] = __umul24(a_code[k], z_code[c]) + acc[k][c];
#pragma unroll
      for (int k = 0; k < RA_QB; ++k)
        if (ch[k] >= 0 && a_code[k] != 0u) {
          const double d = (double)s_z[ch[k]][jb + u] - (double)zli[k];
          const double e = tanh(dl[k] * d) - (a_code[k] == 1u ? 1.0 : -1.0);
          lacc[k] += e * e;
        }
    }
  }

  // unpack {C, D}, fold over the wave, then over the waves in wave order
#pragma unroll
  for (int k = 0; k <= RA_QB; ++k)
#pragma unroll
    for (int c = 0; c <= LP; ++c) {
      const unsigned v = acc[k][c];
      const int conc = wave_sum((int)((v & (RA_DOWN - 1u)) + (v >> 22)));
      const int disc = wave_sum((int)((v >> 11) & (RA_DOWN - 1u)));
      if (lane == 0) {
        s_red[wave][(k * (LP + 1) + c) * 2] = conc;
        s_red[wave][(k * (LP + 1) + c) * 2 + 1] = disc;
      }
    }
#pragma unroll
  for (int k = 0; k < RA_QB; ++k) {
    const double t = wave_sum(lacc[k]);
    if (lane == 0) s_loss[wave][k] = t;
  }
  __syncthreads();
  const long long slot = (long long)blockIdx.x * g.groups + blockIdx.y;
  for (int e = tid; e < (RA_QB + 1) * (LP + 1) * 2; e += RA_TILE) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < RA_TILE / 64; ++w) t += s_red[w][e];
    g.ws_cnt[slot * RA_SLOT + e] = t;
  }
  if (tid < RA_QB) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < RA_TILE / 64; ++w) t += s_loss[w][tid];
    g.ws_loss[slot * RA_QB + tid] = t;
  }
}

// one workgroup per (c, q): thread t adds tiles t, t + 256, ... in ascending order, then a fixed tree over the threads
__global__ __launch_bounds__(RA_FOLD_THREADS) void rank_agreement_fold_kernel(RaArgs g, int lp) {
  __shared__ long long s_v[5][RA_FOLD_THREADS];
  __shared__ double s_l[RA_FOLD_THREADS];
  const int tid = threadIdx.x, c = blockIdx.x, q = blockIdx.y;
  const int grp = q / RA_QB, k = q - grp * RA_QB;
  const int e_qc = (k * (lp + 1) + c) * 2, e_q = (k * (lp + 1) + lp) * 2;
  const int e_c = (RA_QB * (lp + 1) + c) * 2, e_all = (RA_QB * (lp + 1) + lp) * 2;
  long long conc = 0, disc = 0, na_diff = 0, nz_diff = 0, pairs = 0;
  double loss = 0.0;
  for (int p = tid; p < g.npairs; p += RA_FOLD_THREADS) {
    const long long slot = (long long)p * g.groups + grp;
    const int* __restrict__ w = g.ws_cnt + slot * RA_SLOT;
    conc += w[e_qc];
    disc += w[e_qc + 1];
    na_diff += w[e_q] + w[e_q + 1];
    nz_diff += w[e_c] + w[e_c + 1];
    pairs += w[e_all];
    if (c == 0) loss += g.ws_loss[slot * RA_QB + k];
  }
  s_v[0][tid] = conc;
  s_v[1][tid] = disc;
  s_v[2][tid] = na_diff;
  s_v[3][tid] = nz_diff;
  s_v[4][tid] = pairs;
  s_l[tid] = loss;
  __syncthreads();
  for (int s = RA_FOLD_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int r = 0; r < 5; ++r) s_v[r][tid] += s_v[r][tid + s];
      s_l[tid] += s_l[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long cd = s_v[0][0] + s_v[1][0];
    long long* out = g.counts + ((long long)q * g.l + c) * 5;
    out[0] = s_v[0][0];                              // concordant
    out[1] = s_v[1][0];                              // discordant
    out[2] = s_v[2][0] - cd;                         // z_tied
    out[3] = s_v[3][0] - cd;                         // a_tied
    out[4] = s_v[4][0] - s_v[2][0] - s_v[3][0] + cd; // both_tied
    if (c == 0) g.loss_sum[q] = s_l[0];
  }
}

bool ra_supported(int n, int l, int na) { return n >= 2 && n <= RA_MAXN && l >= 1 && l <= RA_MAXL && na >= 1 && na <= RA_MAXNA; }

}  // namespace

extern "C" int64_t pti_rank_agreement_ws_bytes(int n, int l, int na) {
  if (!ra_supported(n, l, na)) return 0;
  const int64_t tiles = cdiv(n, RA_TILE), slots = tiles * (tiles + 1) / 2 * cdiv(na, RA_QB);
  return slots * (int64_t)(RA_QB * sizeof(double) + RA_SLOT * sizeof(int));
}

extern "C" int pti_rank_agreement(const float* zt, int64_t ldz, const float* attrs, int64_t lda, int n, int l, int na,
                                  const int32_t* channels, const float* deltas, int64_t* counts, double* loss_sum,
                                  void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!zt || !attrs || !channels || !deltas || !counts || !loss_sum || !workspace)
    PTI_FAIL(PTI_EINVAL, "rank_agreement: null pointer");
  if (n < 2 || l < 1 || na < 1) PTI_FAIL(PTI_EINVAL, "rank_agreement: bad shape n=%d l=%d na=%d (n >= 2, l, na >= 1)", n, l, na);
  if (!ra_supported(n, l, na))
    PTI_FAIL(PTI_EUNSUPPORTED, "rank_agreement: unsupported shape n=%d l=%d na=%d (n <= %d, l <= %d, na <= %d)", n, l, na,
             RA_MAXN, RA_MAXL, RA_MAXNA);
  if (ldz < n || lda < n) PTI_FAIL(PTI_EINVAL, "rank_agreement: row stride below n (ldz=%lld lda=%lld n=%d)", (long long)ldz, (long long)lda, n);
  for (int q = 0; q < na; ++q)
    if (channels[q] >= l) PTI_FAIL(PTI_EINVAL, "rank_agreement: channels[%d] = %d but there are %d channels", q, channels[q], l);
  if (((uintptr_t)zt & 3) || ((uintptr_t)attrs & 3) || ((uintptr_t)counts & 7) || ((uintptr_t)loss_sum & 7))
    PTI_FAIL(PTI_EINVAL, "rank_agreement: misaligned buffer");
  if ((uintptr_t)workspace & 7) PTI_FAIL(PTI_EINVAL, "rank_agreement: workspace must be 8-byte aligned");
  if (ws_bytes < pti_rank_agreement_ws_bytes(n, l, na))
    PTI_FAIL(PTI_EINVAL, "rank_agreement: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
             (long long)pti_rank_agreement_ws_bytes(n, l, na));
  RaArgs g;
  g.zt = zt;
  g.attrs = attrs;
  g.ldz = ldz;
  g.lda = lda;
  g.n = n;
  g.l = l;
  g.na = na;
  g.tiles = cdiv(n, RA_TILE);
  g.groups = cdiv(na, RA_QB);
  g.npairs = g.tiles * (g.tiles + 1) / 2;
  for (int q = 0; q < RA_MAXNA; ++q) {
    g.channels[q] = q < na ? (channels[q] < 0 ? -1 : channels[q]) : -1;
    g.deltas[q] = q < na ? deltas[q] : 0.0f;
  }
  g.ws_loss = (double*)workspace;   // the doubles first: the int region then starts 8-byte aligned as well
  g.ws_cnt = (int*)(g.ws_loss + (long long)g.npairs * g.groups * RA_QB);
  g.counts = (long long*)counts;
  g.loss_sum = loss_sum;
  const dim3 grid((unsigned)g.npairs, (unsigned)g.groups), block(RA_TILE);
  const int lp = cdiv(l, 4) * 4;
  switch (lp) {
    case 4: PTI_LAUNCH(rank_agreement_tile_kernel<4>, grid, block, 0, (hipStream_t)s, g); break;
    case 8: PTI_LAUNCH(rank_agreement_tile_kernel<8>, grid, block, 0, (hipStream_t)s, g); break;
    case 12: PTI_LAUNCH(rank_agreement_tile_kernel<12>, grid, block, 0, (hipStream_t)s, g); break;
    default: PTI_LAUNCH(rank_agreement_tile_kernel<16>, grid, block, 0, (hipStream_t)s, g); break;
  }
  PTI_CHECK_LAUNCH("rank_agreement (tiles)");
  PTI_LAUNCH(rank_agreement_fold_kernel, dim3((unsigned)l, (unsigned)na), dim3(RA_FOLD_THREADS), 0, (hipStream_t)s, g, lp);
  PTI_CHECK_LAUNCH("rank_agreement (fold)");
  return PTI_OK;
}
