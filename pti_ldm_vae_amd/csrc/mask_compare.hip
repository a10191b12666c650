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
  float* cleaned;   // [n][h][w] or null: pred inside P, 0 elsewhere (pti_mask_compare_cleaned)
  unsigned char* masks;   // [n][h][w] or null: bit 0 = G, bit 1 = P (pti_mask_compare_outputs)
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
      if (a.cleaned) a.cleaned[(size_t)img * npix + p] = rp;
      if (a.masks) a.masks[(size_t)img * npix + p] = (unsigned char)((G ? 1 : 0) | (P ? 2 : 0));
      const double d = (double)g - (double)rp;
      sq += d * d;
      mg = g > mg ? g : mg;
      mp = rp > mp ? rp : mp;
    }
  } else {   // a step budget ran out: the status column says so, the image is all background
    if (a.cleaned)
      for (int p = tid; p < npix; p += MC_THREADS) a.cleaned[(size_t)img * npix + p] = 0.0f;
    if (a.masks)
      for (int p = tid; p < npix; p += MC_THREADS) a.masks[(size_t)img * npix + p] = 0;
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

namespace {
int mc_launch(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts, double* sums,
              float* cleaned, uint8_t* masks, void* workspace, int64_t ws_bytes, pti_stream_t s) {
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
  McArgs a{gt, pred, (int*)workspace, counts, sums, cleaned, masks, mc_ws_ints(h, w), h, w, threshold};
  PTI_LAUNCH(mask_compare_kernel, dim3((unsigned)n), dim3(MC_THREADS), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("mask_compare");
  return PTI_OK;
}
}  // namespace

extern "C" int pti_mask_compare(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts,
                                double* sums, void* workspace, int64_t ws_bytes, pti_stream_t s) {
  return mc_launch(gt, pred, n, h, w, threshold, counts, sums, nullptr, nullptr, workspace, ws_bytes, s);
}

// The same launch, and the same counts and sums bit for bit, with the cleaned prediction c = pred inside P, else 0 written out:
// the second image of the pair the MSE is formed from, without a second labelling (the uniform-window SSIM reads it).
extern "C" int pti_mask_compare_cleaned(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts,
                                        double* sums, float* cleaned, void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!cleaned) PTI_FAIL(PTI_EINVAL, "mask_compare_cleaned: null pointer");
  if ((uintptr_t)cleaned & 3) PTI_FAIL(PTI_EINVAL, "mask_compare_cleaned: misaligned buffer");
  if (cleaned == gt || cleaned == pred) PTI_FAIL(PTI_EINVAL, "mask_compare_cleaned: the output must not alias an input");
  return mc_launch(gt, pred, n, h, w, threshold, counts, sums, cleaned, nullptr, workspace, ws_bytes, s);
}

// The same launch again with either optional output, both or none: cleaned as above, and masks uint8 [n][h][w] with bit 0 = G
// (gt != 0) and bit 1 = P (the filled largest component) -- the two regions the Dice is formed from, for the surface distances
// (csrc/surface_distance.hip).  cleaned != 0 is not P: a filled hole can hold zeros.
extern "C" int pti_mask_compare_outputs(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts,
                                        double* sums, float* cleaned_or_null, uint8_t* masks_or_null, void* workspace,
                                        int64_t ws_bytes, pti_stream_t s) {
  if ((uintptr_t)cleaned_or_null & 3) PTI_FAIL(PTI_EINVAL, "mask_compare_outputs: misaligned buffer");
  if (cleaned_or_null && (cleaned_or_null == gt || cleaned_or_null == pred))
    PTI_FAIL(PTI_EINVAL, "mask_compare_outputs: an output must not alias an input");
  if (masks_or_null && ((const void*)masks_or_null == (const void*)gt || (const void*)masks_or_null == (const void*)pred ||
                        (const void*)masks_or_null == (const void*)cleaned_or_null))
    PTI_FAIL(PTI_EINVAL, "mask_compare_outputs: an output must not alias an input or the other output");
  return mc_launch(gt, pred, n, h, w, threshold, counts, sums, cleaned_or_null, masks_or_null, workspace, ws_bytes, s);
}

// ---- pair registration (include/pti_vae.h "pair registration"): what the reference does to a pair BEFORE it
// measures -- straighten both sides (orientation of the object, cubic rotation), then move the prediction sideways until the
// centres of the bottom fifth agree.  Three launches, no host synchronisation between them:
//   mask_moments_kernel   grid (n, 2): one workgroup per (image, side) labels that side with mc_label, fills K as the
//                         comparison kernel does, adds the six raw moments of F(K) as int64 and writes beta, cos beta, sin
//                         beta; the prediction side also writes the cleaned prediction c
//   warp_cubic_kernel     grid (row tiles, n, 2): 4 x 4 cubic convolution about (w / 2, h / 2), replicate border
//   align_bottom_kernel   grid (n): centres of the bottom h / 5 rows, the shift, the shifted copy of the prediction
namespace {

constexpr int MM_COLS = PTI_MASK_MOMENTS_COLUMNS;
constexpr int AB_COLS = PTI_ALIGN_BOTTOM_COLUMNS;
constexpr int WC_THREADS = 256;
constexpr int WC_ROWS = 4;     // rows of one warp_cubic workgroup

struct MmArgs {
  const float* gt;
  const float* pred;
  int* ws;
  float* cleaned;       // [n][h][w]
  long long* moments;   // [n][2][MM_COLS]
  double* coeffs;       // [n][2][3]: beta, cos beta, sin beta
  long long ws_ints_per_side;
  int h, w;
  float thr;
};

// The fill of mask_compare_kernel as a function: 4-connected union-find in B over the pixels outside the component `root` of
// L, node 0 = outside the image.  Returns false on an overrun (block-uniform).
__device__ bool mc_fill(int* L, int* B, int root, int h, int w, McShared& S) {
  const int npix = h * w, tid = threadIdx.x;
  const int budget = 2 * (npix + 3);
  if (tid == 0) mc_st(B, 0);
  for (int p = tid; p < npix; p += MC_THREADS) {
    const int y = p / w, x = p - y * w;
    const bool border = x == 0 || y == 0 || x == w - 1 || y == h - 1;
    mc_st(B + p + 1, (border && mc_ld(L + p) != root) ? 0 : p + 1);
  }
  mc_phase();
  for (int p = tid; p < npix; p += MC_THREADS) {
    if (mc_ld(L + p) == root) continue;
    const int y = p / w, x = p - y * w;
    const bool N = y > 0 && mc_ld(L + p - w) != root;
    const bool W = x > 0 && mc_ld(L + p - 1) != root;
    const bool NW = y > 0 && x > 0 && mc_ld(L + p - w - 1) != root;
    if (N) mc_union(B, p + 1, p - w + 1, budget, &S.err);
    if (W && !(N && NW)) mc_union(B, p + 1, p, budget, &S.err);
  }
  return !mc_failed(S);
}

// Is pixel p part of F(K)?  K is the component `root` of L, B the finished fill.
__device__ __forceinline__ bool mc_filled(int* L, int* B, int root, int p, int npix, McShared& S) {
  if (mc_ld(L + p) == root) return true;
  int b = 2 * (npix + 3);
  const bool in = mc_find(B, p + 1, b) != 0;
  if (b < 0) { S.err = 1; return false; }
  return in;
}

__global__ __launch_bounds__(MC_THREADS) void mask_moments_kernel(MmArgs a) {
  __shared__ McShared S;
  __shared__ long long part[6][MC_WAVES];
  const int img = blockIdx.x, side = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = a.h, w = a.w, npix = h * w;
  const float* src = (side == 0 ? a.gt : a.pred) + (size_t)img * npix;
  int* L = a.ws + ((size_t)img * 2 + side) * a.ws_ints_per_side;   // the three planes of mask_compare_kernel, per side
  int* cnt = L + npix;
  int* B = cnt + npix;
  float* c = a.cleaned + (size_t)img * npix;
  long long* mo = a.moments + ((size_t)img * 2 + side) * MM_COLS;
  double* co = a.coeffs + ((size_t)img * 2 + side) * 3;

  if (tid == 0) {
    S.key[0] = S.key[1] = 0;
    S.nfg[0] = S.nfg[1] = S.ncomp[0] = S.ncomp[1] = 0;
    for (int s = 0; s < 2; ++s) {
      S.box[s][0] = S.box[s][1] = INT_MAX;
      S.box[s][2] = S.box[s][3] = -1;
    }
    S.err = 0;
  }
  __syncthreads();

  // (With a second caller the compiler keeps mc_label<0> and mc_label<1> out of line, for mask_compare_kernel too: one call
  // per side and workgroup, the loops are inside.  Its results are the same words; its time was measured again)
  bool ok = side == 0 ? mc_label<0>(src, a.thr, h, w, L, cnt, S) : mc_label<1>(src, a.thr, h, w, L, cnt, S);
  int root = MC_NONE;
  if (ok && S.key[side]) root = (int)(0xffffffffu - (unsigned)(S.key[side] & 0xffffffffu));
  if (ok && root != MC_NONE) ok = mc_fill(L, B, root, h, w, S);

  // one pass: membership of F(K), the six sums, and on the prediction side c = pred inside P, 0 elsewhere
  long long s0 = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
  for (int p = tid; p < npix; p += MC_THREADS) {
    const bool in = ok && root != MC_NONE && mc_filled(L, B, root, p, npix, S);
    if (side == 1) c[p] = in ? src[p] : 0.0f;
    if (in) {
      const long long y = p / w, x = p - y * w;
      s0 += 1; sx += x; sy += y; sxx += x * x; sxy += x * y; syy += y * y;
    }
  }
  s0 = wave_sum(s0); sx = wave_sum(sx); sy = wave_sum(sy); sxx = wave_sum(sxx); sxy = wave_sum(sxy); syy = wave_sum(syy);
  if (lane == 0) {
    part[0][wave] = s0; part[1][wave] = sx; part[2][wave] = sy; part[3][wave] = sxx; part[4][wave] = sxy; part[5][wave] = syy;
  }
  __syncthreads();
  if (tid != 0) return;
  if (S.err) {   // a step budget ran out: the row says so, carries nothing else and asks for no rotation
    for (int k = 0; k < MM_COLS; ++k) mo[k] = 0;
    mo[MM_COLS - 1] = 1;
    co[0] = 0.0; co[1] = 1.0; co[2] = 0.0;
    return;
  }
  long long m[6];
  for (int k = 0; k < 6; ++k) {
    m[k] = part[k][0];
    for (int v = 1; v < MC_WAVES; ++v) m[k] += part[k][v];
  }
  // m00 <= 2^20, m10 and m01 < 2^30, m20, m11 and m02 < 2^40 at 1024 x 1024: every product below is under 2^60, A, B, C and
  // A - C fit in 61 bits and 2 B in 62 -- plain int64, exact.
  const long long A = m[0] * m[3] - m[1] * m[1];
  const long long Bm = m[0] * m[4] - m[1] * m[2];
  const long long Cm = m[0] * m[5] - m[2] * m[2];
  double beta = 0.0, cb = 1.0, sb = 0.0;
  if (m[0] > 0) {
    if (Bm == 0) {   // decided on the integers: an upright, mirror-symmetric or round object is not rotated at all
      if (Cm < A) { beta = M_PI / 2; cb = 0.0; sb = 1.0; }   // the quarter turn's coefficients are exact, not cos(fp64 pi / 2)
    } else {
      const double theta = 0.5 * atan2((double)(2 * Bm), (double)(A - Cm));
      beta = theta > 0.0 ? theta - M_PI / 2 : theta + M_PI / 2;
      sincos(beta, &sb, &cb);
    }
  }
  for (int k = 0; k < 6; ++k) mo[k] = m[k];
  mo[6] = A; mo[7] = Bm; mo[8] = Cm; mo[9] = 0;
  co[0] = beta; co[1] = cb; co[2] = sb;
}

struct WcArgs {
  const float* src[2];
  float* dst[2];
  const double* coeffs;   // [n][2][3]
  int h, w;
};

// Keys' cubic convolution weights, a = -0.75, for the taps at -1, 0, +1, +2 of a point t in [0, 1] past tap 0.  fp32, in
// this association (the pragma keeps -ffast-math from re-associating; a multiply may still be FUSED with the add that
// follows it -- the library is built with -ffp-contract=fast, which the pragma does not undo, and the ISA has v_fma).  At
// t == 0 they are 0, 1, 0, 0 either way: every product and sum there is exact.
__device__ __forceinline__ void wc_weights(float t, float* wt) {
#pragma clang fp contract(off) reassociate(off)
  const float a = -0.75f;
  const float u = t + 1.0f, v = 1.0f - t;
  wt[0] = ((a * u - 5.0f * a) * u + 8.0f * a) * u - 4.0f * a;
  wt[1] = ((a + 2.0f) * t - (a + 3.0f)) * (t * t) + 1.0f;
  wt[2] = ((a + 2.0f) * v - (a + 3.0f)) * (v * v) + 1.0f;
  wt[3] = ((1.0f - wt[0]) - wt[1]) - wt[2];
}

__device__ __forceinline__ int wc_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// One workgroup: WC_ROWS output rows of one (image, side); consecutive threads take consecutive x (coalesced stores), the
// 16 gathers go to an image that sits in L2.  Source coordinates in fp64 from the per-image coefficients, weights and sums
// in fp32; the association of every sum is pinned and tests/mask_register_oracle.py restates it with every operation rounded
// on its own -- the kernel's fused multiply-adds round less often, so it sits between that restatement and the fp64 oracle.
__global__ __launch_bounds__(WC_THREADS) void warp_cubic_kernel(WcArgs a) {
#pragma clang fp contract(off) reassociate(off)
  const int img = blockIdx.y, side = blockIdx.z;
  const int h = a.h, w = a.w;
  const double* co = a.coeffs + ((size_t)img * 2 + side) * 3;
  const double cb = co[1], sb = co[2];
  const float* src = a.src[side] + (size_t)img * h * w;
  float* dst = a.dst[side] + (size_t)img * h * w;
  const int cx = w / 2, cy = h / 2;
  const int y0 = blockIdx.x * WC_ROWS, y1 = min(y0 + WC_ROWS, h);
  for (int y = y0; y < y1; ++y) {
    const double dy = (double)(y - cy);
    for (int x = threadIdx.x; x < w; x += WC_THREADS) {
      const double dx = (double)(x - cx);
      const double px = ((double)cx + cb * dx) - sb * dy;
      const double py = ((double)cy + sb * dx) + cb * dy;
      double fxd = floor(px), fyd = floor(py);
      const float tx = (float)(px - fxd), ty = (float)(py - fyd);
      // Further than three pixels outside, all four taps are the border pixel whatever the distance: clamping the base there
      // changes nothing and keeps the conversion to int defined for any coefficients (NaN included: fmax / fmin drop it).
      fxd = fmin(fmax(fxd, -3.0), (double)(w + 2));
      fyd = fmin(fmax(fyd, -3.0), (double)(h + 2));
      const int fx = (int)fxd, fy = (int)fyd;
      float wx[4], wy[4];
      wc_weights(tx, wx);
      wc_weights(ty, wy);
      const int x_0 = wc_clamp(fx - 1, w), x_1 = wc_clamp(fx, w), x_2 = wc_clamp(fx + 1, w), x_3 = wc_clamp(fx + 2, w);
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* row = src + (size_t)wc_clamp(fy - 1 + j, h) * w;
        r[j] = ((wx[0] * row[x_0] + wx[1] * row[x_1]) + wx[2] * row[x_2]) + wx[3] * row[x_3];
      }
      dst[(size_t)y * w + x] = ((wy[0] * r[0] + wy[1] * r[1]) + wy[2] * r[2]) + wy[3] * r[3];
    }
  }
}

struct AbArgs {
  const float* rot_gt;
  const float* rot_pred;
  float* aligned;
  int* info;   // [n][AB_COLS]
  int h, w;
};

// One workgroup per image: (count, column sum) of the non-zero pixels in the last h / 5 rows of both sides, the truncated
// centres and their difference, then the copy of the prediction moved by that many columns with zero fill.  The sums are at
// most 204 * 1024 * 1023 < 2^31: int32.
__global__ __launch_bounds__(MC_THREADS) void align_bottom_kernel(AbArgs a) {
  __shared__ int red[4][MC_WAVES];
  __shared__ int sh_shift;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = a.h, w = a.w, npix = h * w;
  const float* rg = a.rot_gt + (size_t)img * npix;
  const float* rp = a.rot_pred + (size_t)img * npix;
  float* out = a.aligned + (size_t)img * npix;
  int* info = a.info + (size_t)img * AB_COLS;
  int ng = 0, sg = 0, np = 0, sp = 0;
  for (int p = (h - h / 5) * w + tid; p < npix; p += MC_THREADS) {
    const int x = p % w;
    const bool g = mc_fg<0>(rg, p, 0.0f), r = mc_fg<0>(rp, p, 0.0f);
    ng += g; sg += g ? x : 0; np += r; sp += r ? x : 0;
  }
  ng = wave_sum(ng); sg = wave_sum(sg); np = wave_sum(np); sp = wave_sum(sp);
  if (lane == 0) { red[0][wave] = ng; red[1][wave] = sg; red[2][wave] = np; red[3][wave] = sp; }
  __syncthreads();
  if (tid == 0) {
    int t[4];
    for (int k = 0; k < 4; ++k) {
      t[k] = red[k][0];
      for (int v = 1; v < MC_WAVES; ++v) t[k] += red[k][v];
    }
    const int cg = t[0] ? t[1] / t[0] : -1, cp = t[2] ? t[3] / t[2] : -1;
    const int status = (t[0] ? 0 : 1) | (t[2] ? 0 : 2);
    const int shift = status ? 0 : cg - cp;
    info[0] = cg; info[1] = cp; info[2] = t[0]; info[3] = t[2]; info[4] = shift; info[5] = status;
    sh_shift = shift;
  }
  __syncthreads();
  const int shift = sh_shift;
  for (int p = tid; p < npix; p += MC_THREADS) {
    const int x = p % w, xs = x - shift;
    out[p] = (xs >= 0 && xs < w) ? rp[p - shift] : 0.0f;
  }
}

inline int mr_check_shape(const char* who, int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) PTI_FAIL(PTI_EINVAL, "%s: bad shape n=%d h=%d w=%d (all >= 1)", who, n, h, w);
  if (h > MC_MAX_EDGE || w > MC_MAX_EDGE)
    PTI_FAIL(PTI_EUNSUPPORTED, "%s: unsupported shape h=%d w=%d (h, w <= %d)", who, h, w, MC_MAX_EDGE);
  if (n > 65535) PTI_FAIL(PTI_EUNSUPPORTED, "%s: unsupported batch n=%d (n <= 65535)", who, n);
  return PTI_OK;
}

}  // namespace

extern "C" int64_t pti_mask_moments_ws_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1 || h > MC_MAX_EDGE || w > MC_MAX_EDGE) return 0;
  return 2 * (int64_t)n * mc_ws_ints(h, w) * (int64_t)sizeof(int);
}

extern "C" int pti_mask_moments(const float* gt, const float* pred, int n, int h, int w, float threshold, float* cleaned,
                                int64_t* moments, double* coeffs, void* workspace, int64_t ws_bytes, pti_stream_t s) {
  if (!gt || !pred || !cleaned || !moments || !coeffs || !workspace) PTI_FAIL(PTI_EINVAL, "mask_moments: null pointer");
  if (const int rc = mr_check_shape("mask_moments", n, h, w)) return rc;
  if (!(threshold >= 0.0f)) PTI_FAIL(PTI_EINVAL, "mask_moments: threshold %g must be >= 0", (double)threshold);
  if (((uintptr_t)gt & 3) || ((uintptr_t)pred & 3) || ((uintptr_t)cleaned & 3) || ((uintptr_t)moments & 7) || ((uintptr_t)coeffs & 7))
    PTI_FAIL(PTI_EINVAL, "mask_moments: misaligned buffer");
  if ((uintptr_t)workspace & 3) PTI_FAIL(PTI_EINVAL, "mask_moments: workspace must be 4-byte aligned");
  if (ws_bytes < pti_mask_moments_ws_bytes(n, h, w))
    PTI_FAIL(PTI_EINVAL, "mask_moments: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
             (long long)pti_mask_moments_ws_bytes(n, h, w));
  MmArgs a{gt, pred, (int*)workspace, cleaned, (long long*)moments, coeffs, mc_ws_ints(h, w), h, w, threshold};
  PTI_LAUNCH(mask_moments_kernel, dim3((unsigned)n, 2), dim3(MC_THREADS), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("mask_moments");
  return PTI_OK;
}

extern "C" int pti_warp_cubic(const float* gt, const float* pred, const double* coeffs, int n, int h, int w, float* out_gt,
                              float* out_pred, pti_stream_t s) {
  if (!gt || !pred || !coeffs || !out_gt || !out_pred) PTI_FAIL(PTI_EINVAL, "warp_cubic: null pointer");
  if (const int rc = mr_check_shape("warp_cubic", n, h, w)) return rc;
  if (((uintptr_t)gt & 3) || ((uintptr_t)pred & 3) || ((uintptr_t)out_gt & 3) || ((uintptr_t)out_pred & 3) || ((uintptr_t)coeffs & 7))
    PTI_FAIL(PTI_EINVAL, "warp_cubic: misaligned buffer");
  if (out_gt == gt || out_gt == pred || out_pred == gt || out_pred == pred || out_gt == out_pred)
    PTI_FAIL(PTI_EINVAL, "warp_cubic: the outputs must not alias the inputs or each other");
  WcArgs a{{gt, pred}, {out_gt, out_pred}, coeffs, h, w};
  PTI_LAUNCH(warp_cubic_kernel, dim3((unsigned)((h + WC_ROWS - 1) / WC_ROWS), (unsigned)n, 2), dim3(WC_THREADS), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("warp_cubic");
  return PTI_OK;
}

extern "C" int pti_align_bottom(const float* rot_gt, const float* rot_pred, int n, int h, int w, float* aligned, int32_t* info,
                                pti_stream_t s) {
  if (!rot_gt || !rot_pred || !aligned || !info) PTI_FAIL(PTI_EINVAL, "align_bottom: null pointer");
  if (const int rc = mr_check_shape("align_bottom", n, h, w)) return rc;
  if (h < 5) PTI_FAIL(PTI_EUNSUPPORTED, "align_bottom: unsupported shape h=%d (the bottom fifth needs h >= 5)", h);
  if (((uintptr_t)rot_gt & 3) || ((uintptr_t)rot_pred & 3) || ((uintptr_t)aligned & 3) || ((uintptr_t)info & 3))
    PTI_FAIL(PTI_EINVAL, "align_bottom: misaligned buffer");
  if (aligned == rot_pred || aligned == rot_gt) PTI_FAIL(PTI_EINVAL, "align_bottom: the output must not alias an input");
  AbArgs a{rot_gt, rot_pred, aligned, (int*)info, h, w};
  PTI_LAUNCH(align_bottom_kernel, dim3((unsigned)n), dim3(MC_THREADS), 0, (hipStream_t)s, a);
  PTI_CHECK_LAUNCH("align_bottom");
  return PTI_OK;
}
