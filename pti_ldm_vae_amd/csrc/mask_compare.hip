// Shape comparison of a ground-truth / prediction image pair (reference src/pti_ldm_vae/analysis/metrics.py:143-209,
// 312-398: generate_clean_mask, dice_coefficient, iou, compute_object_dimensions, calculate_psnr): two binary masks per
// image, their 8-connected components, the largest component K, its hole-filled region F, and the counts, boxes, row
// widths and fp64 sums the report needs -- ONE launch, one workgroup of 1024 threads per image, no host synchronisation.
//
// Labelling is a union-find on an int32 parent array in the workspace (labels for 1024 x 1024 do not fit LDS):
//   parent[p] <= p always, a root has parent[p] == p, and a tree is only ever hung under a SMALLER root with an integer
//   atomicMin, so the root of a finished component is its smallest row-major index whatever the scheduling was: labels,
//   and with them every output, do not depend on the order in which waves ran.
//   A pixel links to its N neighbour, or else to NW and NE, and to W unless N and NW are both foreground (W, NW, N then
//   already hang together through their own links -- induction over the rows); that is all of 8-connectivity.
// The fill is the same union-find over the pixels OUTSIDE K under 4-connectivity, with one extra node 0 for the virtual ring
//   of background round the image: node p + 1 is pixel p, a border pixel outside K starts with parent 0.  A pixel outside K
//   whose root is not 0 cannot reach the ring: it is a hole (smaller components inside it included) and belongs to F.
// The workgroup walks the image in passes of 1024 consecutive pixels (coalesced), a __threadfence + __syncthreads between
//   dependent passes; label words are read and written with relaxed agent-scope atomics, which go to L2, so no wave reads a
//   stale line.  Every word of the workspace that is read was written earlier in the same launch.
// Every loop that follows parents or retries an atomicMin draws on a step budget: within one union both ends only ever move
//   to smaller indices, so 2 (nodes + 2) steps cannot be exceeded by a correct run.  An overrun, or a parent outside
//   [0, self], sets the image's status word (column 23) and ends that workgroup's work; nothing spins.
// fp64 sums: every thread adds its pixels in pass order, a shuffle tree folds the wave, thread 0 adds the 16 waves in order.
#include <limits.h>

#include "pti_common.h"

namespace {

constexpr int MC_MAX_EDGE = PTI_MASK_COMPARE_MAX_EDGE;
constexpr int MC_COLS = PTI_MASK_COMPARE_COLUMNS;
constexpr int MC_THREADS = 1024;
constexpr int MC_WAVES = MC_THREADS / 64;
constexpr int MC_NONE = -2;   // "no component": never equal to a parent word (background holds -1)

struct McArgs {
  const float* gt;
  const float* pred;
  int* ws;
  int* counts;      // [n][MC_COLS]
  double* sums;     // [n][3]
  long long ws_ints_per_image;
  int h, w;
  float thr;
};

struct McShared {
  unsigned long long key[2];   // (size << 32) | (0xffffffff - root) of the best component, per side
  int nfg[2], ncomp[2];
  int box[2][4];               // min x, min y, max x, max y of K
  int wid[2][3];
  int np, inter;
  int err;
  double dsum[MC_WAVES];
  float mx[2][MC_WAVES];
};

__device__ __forceinline__ int mc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mc_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mc_phase() { __threadfence(); __syncthreads(); }

// End of a pass that may have raised the error word: every thread reads it between two barriers, so that a thread which
// raises it in the NEXT pass cannot split the workgroup's view of this one.
__device__ __forceinline__ bool mc_failed(const McShared& S) {
  mc_phase();
  const int e = S.err;
  __syncthreads();
  return e != 0;
}

// The two masks.  Ordinary float compares on the loaded values: the library is built with -ffast-math, but also with
// -fno-finite-math-only (so a compare is not folded on the assumption that no NaN or infinity exists) and without
// flush-to-zero of fp32 denormals (gfx9 keeps them, and v_cmp honours the mode), and the operands are the loaded words and
// the threshold themselves -- nothing is subtracted, scaled or contracted before the compare, so there is nothing for
// fast-math to re-associate.  -t is a sign flip, exact.
template <int SIDE>
__device__ __forceinline__ bool mc_fg(const float* img, int p, float t) {
  const float v = img[p];
  return SIDE == 0 ? (v != 0.0f) : ((v > t) | (v < -t));
}

// Root of p.  `budget` is the caller's step allowance; below zero means overrun or a corrupt parent, and the result is void.
__device__ __forceinline__ int mc_find(int* L, int p, int& budget) {
  const int start = p;
  int hops = 0;
  int q = mc_ld(L + p);
  while (q != p) {
    if (q < 0 || q > p || --budget < 0) { budget = -1; return p; }
    p = q;
    q = mc_ld(L + p);
    ++hops;
  }
  if (hops > 1) atomicMin(L + start, p);   // shorten the path: an ancestor replaces an ancestor, never raises a parent
  return p;
}

__device__ __forceinline__ void mc_union(int* L, int a, int b, int budget, int* err) {
  for (;;) {
    a = mc_find(L, a, budget);
    b = mc_find(L, b, budget);
    if (budget < 0) { *err = 1; return; }
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);   // hang root a under the smaller root b
    if (old == a) return;
    // a had stopped being a root: its former parent `old` (kept, or just replaced by b) must be joined with b instead
    if (old < 0 || old > a || --budget < 0) { *err = 1; return; }
    a = old;
  }
}

// Components of one mask: parents in L, sizes in cnt.  Leaves L flat (every foreground word holds its root), the number of
// foreground pixels and of components and the best component's key in S.  Returns false on an overrun (block-uniform).
template <int SIDE>
__device__ bool mc_label(const float* img, float thr, int h, int w, int* L, int* cnt, McShared& S) {
  const int npix = h * w, tid = threadIdx.x, lane = tid & 63;
  const int budget = 2 * (npix + 2);
  int nfg = 0;
  for (int p = tid; p < npix; p += MC_THREADS) {
    const bool f = mc_fg<SIDE>(img, p, thr);
    mc_st(L + p, f ? p : -1);
    mc_st(cnt + p, 0);
    nfg += f;
  }
  nfg = wave_sum(nfg);
  if (lane == 0 && nfg) atomicAdd(&S.nfg[SIDE], nfg);
  mc_phase();

  for (int p = tid; p < npix; p += MC_THREADS) {
    if (!mc_fg<SIDE>(img, p, thr)) continue;
    const int y = p / w, x = p - y * w;
    const bool up = y > 0, lf = x > 0, rt = x < w - 1;
    const bool N = up && mc_fg<SIDE>(img, p - w, thr);
    const bool NW = up && lf && mc_fg<SIDE>(img, p - w - 1, thr);
    const bool W = lf && mc_fg<SIDE>(img, p - 1, thr);
    if (N) {
      mc_union(L, p, p - w, budget, &S.err);
    } else {
      if (NW) mc_union(L, p, p - w - 1, budget, &S.err);
      if (up && rt && mc_fg<SIDE>(img, p - w + 1, thr)) mc_union(L, p, p - w + 1, budget, &S.err);
    }
    if (W && !(N && NW)) mc_union(L, p, p - 1, budget, &S.err);
  }
  if (mc_failed(S)) return false;

  // flatten and count: the structure no longer changes but for path shortening, so find() gives the final root
  int ncomp = 0;
  for (int base = 0; base < npix; base += MC_THREADS) {
    const int p = base + tid;
    const bool f = p < npix && mc_fg<SIDE>(img, p, thr);
    int r = -1;
    if (f) {
      int b = budget;
      r = mc_find(L, p, b);
      if (b < 0) { S.err = 1; r = p; }
      if (r != p) atomicMin(L + p, r);
      ncomp += r == p;
    }
    // one add per wave for the lanes that share the first active lane's root (the inside of a blob), one each for the rest
    const unsigned long long act = __ballot(f);
    if (act) {
      const int leader = __ffsll((long long)act) - 1;
      const int r0 = __shfl(r, leader, 64);
      const unsigned long long same = __ballot(f && r == r0);
      if (lane == leader) atomicAdd(cnt + r0, (int)__popcll(same));
      if (f && r != r0) atomicAdd(cnt + r, 1);
    }
  }
  ncomp = wave_sum(ncomp);
  if (lane == 0 && ncomp) atomicAdd(&S.ncomp[SIDE], ncomp);
  if (mc_failed(S)) return false;

  // the largest component; among equals the one with the smallest root, which is its smallest row-major index
  unsigned long long key = 0;
  for (int p = tid; p < npix; p += MC_THREADS) {
    if (mc_ld(L + p) != p) continue;
    const unsigned long long k = ((unsigned long long)(unsigned)mc_ld(cnt + p) << 32) | (unsigned long long)(0xffffffffu - (unsigned)p);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k = __shfl_xor(key, o, 64);
    key = k > key ? k : key;
  }
  if (lane == 0 && key) atomicMax(&S.key[SIDE], key);
  __syncthreads();

  const int root = S.key[SIDE] ? (int)(0xffffffffu - (unsigned)(S.key[SIDE] & 0xffffffffu)) : MC_NONE;
  int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  if (root != MC_NONE) {
    for (int p = tid; p < npix; p += MC_THREADS) {
      if (mc_ld(L + p) != root) continue;
      const int y = p / w, x = p - y * w;
      x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
    }
  }
  x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
  if (lane == 0 && x1 >= 0) {
    atomicMin(&S.box[SIDE][0], x0); atomicMin(&S.box[SIDE][1], y0);
    atomicMax(&S.box[SIDE][2], x1); atomicMax(&S.box[SIDE][3], y1);
  }
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(MC_THREADS) void mask_compare_kernel(McArgs a) {
  __shared__ McShared S;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = a.h, w = a.w, npix = h * w;
  const float* gt = a.gt + (size_t)img * npix;
  const float* pred = a.pred + (size_t)img * npix;
  int* L = a.ws + (size_t)img * a.ws_ints_per_image;   // [npix] parents of the side being labelled
  int* cnt = L + npix;                                  // [npix] component sizes at their roots
  int* B = cnt + npix;                                  // [npix + 1] parents of the fill, node 0 = the ring
  int* out = a.counts + (size_t)img * MC_COLS;
  double* fo = a.sums + (size_t)img * 3;

  if (tid == 0) {
    S.key[0] = S.key[1] = 0;
    S.nfg[0] = S.nfg[1] = S.ncomp[0] = S.ncomp[1] = 0;
    for (int s = 0; s < 2; ++s) {
      S.box[s][0] = S.box[s][1] = INT_MAX;
      S.box[s][2] = S.box[s][3] = -1;
      S.wid[s][0] = S.wid[s][1] = S.wid[s][2] = 0;
    }
    S.np = S.inter = S.err = 0;
  }
  __syncthreads();

  bool ok = mc_label<0>(gt, a.thr, h, w, L, cnt, S);
  // the ground-truth side is finished with L and cnt: S holds what is kept of it
  int gbox[4] = {-1, -1, 0, 0}, gkept = 0;
  if (ok && S.key[0]) {
    gbox[0] = S.box[0][0]; gbox[1] = S.box[0][1];
    gbox[2] = S.box[0][2] - S.box[0][0] + 1; gbox[3] = S.box[0][3] - S.box[0][1] + 1;
    gkept = (int)(S.key[0] >> 32);
  }
  __syncthreads();
  ok = ok && mc_label<1>(pred, a.thr, h, w, L, cnt, S);
  int rbox[4] = {-1, -1, 0, 0}, rkept = 0, rroot = MC_NONE;
  if (ok && S.key[1]) {
    rbox[0] = S.box[1][0]; rbox[1] = S.box[1][1];
    rbox[2] = S.box[1][2] - S.box[1][0] + 1; rbox[3] = S.box[1][3] - S.box[1][1] + 1;
    rkept = (int)(S.key[1] >> 32);
    rroot = (int)(0xffffffffu - (unsigned)(S.key[1] & 0xffffffffu));
  }

  // ---- fill: 4-connected union-find over the pixels outside K(R), node 0 = outside the image ----
  const int budget = 2 * (npix + 3);
  if (ok && rroot != MC_NONE) {
    if (tid == 0) mc_st(B, 0);
    for (int p = tid; p < npix; p += MC_THREADS) {
      const int y = p / w, x = p - y * w;
      const bool border = x == 0 || y == 0 || x == w - 1 || y == h - 1;
      mc_st(B + p + 1, (border && mc_ld(L + p) != rroot) ? 0 : p + 1);
    }
    mc_phase();
    for (int p = tid; p < npix; p += MC_THREADS) {
      if (mc_ld(L + p) == rroot) continue;
      const int y = p / w, x = p - y * w;
      const bool N = y > 0 && mc_ld(L + p - w) != rroot;
      const bool W = x > 0 && mc_ld(L + p - 1) != rroot;
      const bool NW = y > 0 && x > 0 && mc_ld(L + p - w - 1) != rroot;
      if (N) mc_union(B, p + 1, p - w + 1, budget, &S.err);
      if (W && !(N && NW)) mc_union(B, p + 1, p, budget, &S.err);
    }
    ok = !mc_failed(S);
  }

  // ---- the comparison pass over P = F(R) and G ----
  const int gr0 = gbox[1] + gbox[3] / 4, gr1 = gbox[1] + gbox[3] / 2, gr2 = gbox[1] + 3 * gbox[3] / 4;
  const int rr0 = rbox[1] + rbox[3] / 4, rr1 = rbox[1] + rbox[3] / 2, rr2 = rbox[1] + 3 * rbox[3] / 4;
  int np = 0, inter = 0, gw0 = 0, gw1 = 0, gw2 = 0, rw0 = 0, rw1 = 0, rw2 = 0;
  double sq = 0.0;
  float mg = -INFINITY, mp = -INFINITY;
  if (ok) {
    for (int p = tid; p < npix; p += MC_THREADS) {
      const int y = p / w, x = p - y * w;
      const float g = gt[p], r = pred[p];
      const bool G = mc_fg<0>(gt, p, a.thr);
      bool P = false;
      if (rroot != MC_NONE) {
        P = mc_ld(L + p) == rroot;
        if (!P) {
          int b = budget;
          P = mc_find(B, p + 1, b) != 0;
          if (b < 0) { S.err = 1; P = false; }
        }
      }
      np += P; inter += P && G;
      if (G && gbox[3] > 0 && x >= gbox[0] && x < gbox[0] + gbox[2]) { gw0 += y == gr0; gw1 += y == gr1; gw2 += y == gr2; }
      if (P && x >= rbox[0] && x < rbox[0] + rbox[2]) { rw0 += y == rr0; rw1 += y == rr1; rw2 += y == rr2; }
      const float rp = P ? r : 0.0f;
      const double d = (double)g - (double)rp;
      sq += d * d;
      mg = g > mg ? g : mg;
      mp = rp > mp ? rp : mp;
    }
  }
  np = wave_sum(np); inter = wave_sum(inter);
  gw0 = wave_sum(gw0); gw1 = wave_sum(gw1); gw2 = wave_sum(gw2);
  rw0 = wave_sum(rw0); rw1 = wave_sum(rw1); rw2 = wave_sum(rw2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_xor(sq, o, 64);
    const float g2 = __shfl_xor(mg, o, 64), p2 = __shfl_xor(mp, o, 64);
    mg = g2 > mg ? g2 : mg;
    mp = p2 > mp ? p2 : mp;
  }
  if (lane == 0) {
    atomicAdd(&S.np, np); atomicAdd(&S.inter, inter);
    atomicAdd(&S.wid[0][0], gw0); atomicAdd(&S.wid[0][1], gw1); atomicAdd(&S.wid[0][2], gw2);
    atomicAdd(&S.wid[1][0], rw0); atomicAdd(&S.wid[1][1], rw1); atomicAdd(&S.wid[1][2], rw2);
    S.dsum[wave] = sq; S.mx[0][wave] = mg; S.mx[1][wave] = mp;
  }
  __syncthreads();
  if (tid != 0) return;
  if (S.err) {   // a step budget ran out: the row says so and carries nothing else
    for (int k = 0; k < MC_COLS; ++k) out[k] = 0;
    out[MC_COLS - 1] = 1;
    fo[0] = fo[1] = fo[2] = 0.0;
    return;
  }
  double tot = S.dsum[0];
  float tg = S.mx[0][0], tp = S.mx[1][0];
  for (int k = 1; k < MC_WAVES; ++k) {
    tot += S.dsum[k];
    tg = S.mx[0][k] > tg ? S.mx[0][k] : tg;
    tp = S.mx[1][k] > tp ? S.mx[1][k] : tp;
  }
  out[0] = S.nfg[0]; out[1] = S.nfg[1]; out[2] = S.ncomp[0]; out[3] = S.ncomp[1];
  out[4] = gkept; out[5] = rkept; out[6] = S.np; out[7] = S.inter; out[8] = S.np + S.nfg[0] - S.inter;
  for (int k = 0; k < 4; ++k) { out[9 + k] = gbox[k]; out[13 + k] = rbox[k]; }
  for (int k = 0; k < 3; ++k) { out[17 + k] = S.wid[0][k]; out[20 + k] = S.wid[1][k]; }
  out[23] = 0;
  fo[0] = tot; fo[1] = (double)tg; fo[2] = (double)tp;
}

inline long long mc_ws_ints(int h, int w) { return ((3LL * h * w + 1 + 1) / 2) * 2; }   // L, cnt, B (+ node 0), even

}  // namespace

extern "C" int64_t pti_mask_compare_ws_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1 || h > MC_MAX_EDGE || w > MC_MAX_EDGE) return 0;
  return (int64_t)n * mc_ws_ints(h, w) * (int64_t)sizeof(int);
}

extern "C" int pti_mask_compare(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts,
                                double* sums, void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!gt || !pred || !counts || !sums || !workspace) PTI_FAIL(PTI_EINVAL, "mask_compare: null pointer");
  if (n < 1 || h < 1 || w < 1) PTI_FAIL(PTI_EINVAL, "mask_compare: bad shape n=%d h=%d w=%d (all >= 1)", n, h, w);
  if (h > MC_MAX_EDGE || w > MC_MAX_EDGE)
    PTI_FAIL(PTI_EUNSUPPORTED, "mask_compare: unsupported shape h=%d w=%d (h, w <= %d)", h, w, MC_MAX_EDGE);
  if (!(threshold >= 0.0f)) PTI_FAIL(PTI_EINVAL, "mask_compare: threshold %g must be >= 0", (double)threshold);
  if (((uintptr_t)gt & 3) || ((uintptr_t)pred & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)sums & 7))
    PTI_FAIL(PTI_EINVAL, "mask_compare: misaligned buffer");
  if ((uintptr_t)workspace & 3) PTI_FAIL(PTI_EINVAL, "mask_compare: workspace must be 4-byte aligned");
  if (ws_bytes < pti_mask_compare_ws_bytes(n, h, w))
    PTI_FAIL(PTI_EINVAL, "mask_compare: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
             (long long)pti_mask_compare_ws_bytes(n, h, w));
  McArgs a{gt, pred, (int*)workspace, counts, sums, mc_ws_ints(h, w), h, w, threshold};
  PTI_LAUNCH(mask_compare_kernel, dim3((unsigned)n), dim3(MC_THREADS), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("mask_compare");
  return PTI_OK;
}
