/*
 * pti_vae.h — C-ABI of libpti_vae_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * VAE training hot path of Sukikui/PTI-LDM-VAE.
 *
 * The reference has no FFI: its only seam is the Python class pti_ldm_vae.models.VAEModel
 * (reference src/pti_ldm_vae/models/autoencoder.py:6-171), whose arithmetic is MONAI's
 * AutoencoderKL reached through torch.nn ops (autoencoder.py:3,67-79,114).  Each entry point
 * below replaces one of those implicit ATen/cuDNN kernels; the comment on each names the
 * reference call it stands in for.  Host side: pti_ldm_vae_amd/_lib.py binds them with ctypes.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes, no torch types; launches ONLY on the given stream;
 *   - never allocates, never synchronises, never throws;
 *   - returns 0 on success or a negative PTI_E* code; pti_last_error_string() explains it;
 *   - activations are NHWC bf16 (channels innermost) unless a parameter says otherwise;
 *   - "stats" buffers are int64_t[N][G][2] = Q47.16 fixed-point {sum, sum of squares} over one
 *     (sample, group) -- see the note above pti_conv_desc; consumers turn them into mean / rstd
 *     themselves (count and eps are passed along).
 */
#ifndef PTI_VAE_H
#define PTI_VAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pti_stream_t; /* hipStream_t */

#define PTI_ABI_VERSION 5   /* 5 (round 3): + pti_direct_repack, pti_pad_nchw_to_nhwc32 / pti_slice_nhwc32_to_nchw,
                                 pti_conv2d_mfma_gnbwd_chain (+ _supported), pti_gn_affine_grads, pti_gn_sums_finalize_affine
                               Still 5: pti_image_metrics / pti_image_metrics_ws_floats, and after them pti_latent_pairwise /
                               pti_latent_group_stats (+ their _ws_floats), were APPENDED (no existing entry point, structure
                               or constant changed), so a caller built against the earlier 5 keeps working.  The same holds
                               for pti_mask_geometry, appended after those.
                               Still 5: pti_mlp_head_fwd / pti_mlp_head_ws_floats / pti_regression_metrics, appended after
                               pti_mask_geometry in the same way.
                               Still 5: pti_conv_wgrad_batched_mode (a host-only query) appended in the same way.
                               Still 5: pti_tsne_affinities / pti_tsne_step (+ their _ws_floats) appended in the same way.
                               Still 5: pti_umap_knn / pti_umap_graph (+ its _capacity, _ws_floats) / pti_umap_epoch appended
                               in the same way.
                               Still 5: pti_umap_knn_cross / pti_umap_transform_graph (+ its _ws_floats) /
                               pti_umap_transform_layout appended in the same way.
                               Still 5: pti_display_planes appended in the same way.
                               Still 5: pti_mask_compare / pti_mask_compare_ws_bytes appended in the same way.
                               Still 5: pti_neighbor_ranks / pti_segment_row_sums / pti_projection_distances appended in the
                               same way.
                               Still 5: pti_full_ranks / pti_coranking_fold / pti_shepard_fold appended in the same way.
                               Still 5: pti_mask_moments (+ its _ws_bytes) / pti_warp_cubic / pti_align_bottom appended in
                               the same way.
                               Still 5: pti_ssim_uniform (+ its _ws_bytes) / pti_mask_compare_cleaned appended in the same
                               way.
                               Still 5: pti_mask_compare_outputs / pti_surface_distance (+ its _ws_bytes) appended in the same
                               way.
                               Still 5: pti_distance_median / pti_permutation_forms (+ their _ws_bytes) / pti_two_sample_kernel /
                               pti_knn_indicator appended in the same way. */

#define PTI_OK 0
#define PTI_EINVAL (-1)   /* bad pointer / dimension */
#define PTI_EUNSUPPORTED (-2) /* channel multiple / mode not built */
#define PTI_ELAUNCH (-3)  /* hipGetLastError() after launch */

/* input gather modes of the implicit-GEMM convolution */
#define PTI_CONV_S1 0   /* stride 1, pad (k-1)/2              nn.Conv2d(k, s=1, p=k//2)              */
#define PTI_CONV_S2PAD 1 /* F.pad(x,(0,1,0,1)) + 3x3 stride 2   MONAI AEKLDownsample                   */
#define PTI_CONV_UP2 2  /* nearest 2x upsample then 3x3 s1 p1  MONAI Upsample(nontrainable)+postconv  */
#define PTI_CONV_ZINS 3 /* zero-insert 2x, pad_lo 2: data-gradient of PTI_CONV_S2PAD                  */

#define PTI_PRO_NONE 0
#define PTI_PRO_GN 1      /* x -> GroupNorm affine                nn.GroupNorm                          */
#define PTI_PRO_GN_SILU 2 /* x -> GroupNorm affine -> SiLU        nn.GroupNorm + F.silu (AEKLResBlock)  */

/* GroupNorm statistics travel as int64 Q47.16 fixed-point {sum, sum of squares} per (sample, group) --           *
 * `int64_t stats[n][groups][2]`, value = integer / 65536 -- so that accumulating them with atomics is order-       *
 * independent and every result downstream is bitwise reproducible (see pti_common.h).                              */
typedef struct pti_conv_desc {
  int32_t n, h, w, cin;   /* real input tensor [n,h,w,cin]                                   */
  int32_t ho, wo, cout;   /* output tensor [n,ho,wo,cout]                                    */
  int32_t ksize;          /* 1 or 3                                                          */
  int32_t mode;           /* PTI_CONV_*                                                      */
  int32_t prologue;       /* PTI_PRO_*: applied to the input while it is staged into LDS     */
  int32_t groups;         /* GroupNorm groups of the prologue                                */
  int32_t add_residual;   /* epilogue: y += residual (same shape as y)                       */
  int32_t accum_stats;    /* epilogue: atomically add {sum,sumsq} of the stored y per        */
                          /* (sample, out-group) into out_stats; out_groups below            */
  int32_t out_groups;
  float eps;              /* GroupNorm eps of the prologue                                   */
  int32_t in_f32;         /* direct conv only: input is fp32 with explicit element strides   */
  int32_t out_f32;        /* direct conv only: output is fp32 with explicit element strides  */
  int64_t in_stride[4];   /* n,h,w,c element strides when in_f32 (else NHWC dense)           */
  int64_t out_stride[4];  /* n,h,w,c element strides when out_f32                            */
  /* 16-bit storage format of the NHWC activation operands: 0 = bf16, 1 = IEEE fp16.  The forward */
  /* pass may keep its activations in fp16 (same bytes, 8x finer rounding); MFMA operands, saved  */
  /* activated inputs, attention tensors and all gradients are bf16.  res_f16 also describes the  */
  /* GroupNorm input `gx` of pti_conv2d_mfma_gnbwd.                                               */
  int32_t in_f16, res_f16, out_f16;
  /* pti_conv2d_mfma only: y is [n][ho/2][wo/2][cout] = the 2x2 SUM pool of the conv output (the data      */
  /* gradient of nn.Upsample(nearest, 2x) + conv, fused: the full-resolution gradient is never written).   */
  int32_t pool2x2_out;
  /* pti_conv2d_mfma / _saveact only: w_packed was packed with w_f16 = 1 and the MFMA multiplies fp16 operands      */
  /* (v_mfma_f32_32x32x16_f16; same rate as bf16, 8x finer operand rounding).  Needs in_f16 = out_f16 = 1 (and      */
  /* res_f16 when a residual is added): the forward convs on fp16 storage.  Gradients always use bf16 operands.     */
  int32_t w_f16;
  /* pti_conv2d_mfma only: y = max(conv + bias [+ residual], 0) -- the ReLU of the perceptual network's Fire modules  */
  /* fused into the store.  Plain fp16 forward launches (w_f16, no prologue, stride-1 gather); refused elsewhere.     */
  int32_t relu_out;
} pti_conv_desc;

int pti_abi_version(void);
const char* pti_last_error_string(void);
/* Symbol of the (last) kernel the calling thread's most recent pti_* call launched, demangled, as the HIP runtime and
 * rocprofv3 name it; "" before the first launch.  Diagnostics: lets a caller pair its own timings with profiler rows. */
const char* pti_last_kernel_name(void);

/* ---- weights ------------------------------------------------------------------------- */
/* Bytes of the MFMA-packed bf16 image of a [cout,cin,k,k] fp32 weight (0 if unsupported).  */
int64_t pti_conv_packed_bytes(int cout, int cin, int ksize, int mode);
/* Pack fp32 OIHW master weights (nn.Conv2d.weight / nn.Linear.weight layout) into the MFMA
 * fragment order read by pti_conv2d_mfma.  transpose_flip=1 builds the data-gradient operand
 * W'[ci][co][2-kh][2-kw]; cout/cin are those of the ORIGINAL weight.  nsrc>1 concatenates
 * nsrc weights along the output channels (to_q/to_k/to_v fused into one 1x1).             */
int pti_conv_pack_weights(const float* const* w_oihw, int nsrc, void* packed, int cout, int cin,
                          int ksize, int mode, int transpose_flip, int w_f16, pti_stream_t s);

/* Batched form (one launch for all layers of the model after an optimiser step): the caller keeps a
 * table of pti_conv_pack_entry_bytes()-byte entries; pti_conv_pack_table_fill writes ONE entry into HOST
 * memory and returns its size in 256-element blocks; the caller uploads the table plus the running
 * first-block index of every entry, then launches everything with pti_conv_pack_weights_batched.   */
int pti_conv_pack_entry_bytes(void);
int pti_conv_pack_table_fill(void* host_entry, const float* w_oihw_dev, void* packed_dev, int cout,
                             int cin, int ksize, int mode, int transpose_flip, int w_f16, int64_t* nblocks);
int pti_conv_pack_weights_batched(const void* table_dev, const int* blk_first_dev, int n,
                                  int total_blocks, pti_stream_t s);

/* ---- GroupNorm statistics (nn.GroupNorm's reduction) ---------------------------------- */
/* stats[n][g] += {sum, sumsq} of x[n, :, channels of g]; stats must be zeroed by the caller. */
int pti_gn_stats(const void* x_nhwc_16bit, int64_t* stats, int n, int hw, int c, int groups,
                 int x_f16, pti_stream_t s);

/* ---- convolutions ---------------------------------------------------------------------- */
/* Implicit-GEMM 3x3 / 1x1 convolution on bf16 MFMA (v_mfma_f32_32x32x16_bf16), fp32 accumulate:
 * y = conv(prologue(x)) + bias [+ residual].  Replaces nn.Conv2d (+ the GroupNorm/SiLU in
 * front of it, + the residual add behind it) inside MONAI AEKLResBlock / AEKLDownsample /
 * Upsample / SABlock linears.  cin, cout multiples of 32.  in_stats / out_stats: int64_t[n][groups][2]
 * Q47.16 fixed-point sums (above).                                                          */
int pti_conv2d_mfma(const void* x, const void* w_packed, const float* bias, const int64_t* in_stats,
                    const float* gamma, const float* beta, const void* residual, void* y,
                    int64_t* out_stats, const pti_conv_desc* d, pti_stream_t s);

/* Same launch, plus a side output: act_out = prologue(x) as bf16 NHWC [n][h][w][cin] (the tensor autograd
 * would save for nn.Conv2d's weight gradient).  3x3 PTI_CONV_S1 with a GroupNorm(+SiLU) prologue only.  The
 * weight-gradient call then reads act_out with PTI_PRO_NONE instead of re-applying the prologue. */
int pti_conv2d_mfma_saveact(const void* x, const void* w_packed, const float* bias, const int64_t* in_stats,
                            const float* gamma, const float* beta, const void* residual, void* y,
                            int64_t* out_stats, void* act_out, const pti_conv_desc* d, pti_stream_t s);

/* Direct (VALU, fp32 math) convolution for the degenerate-channel layers (cin or cout < 32):
 * conv_in, conv_out of Encoder/Decoder.  w: fp32 [k*k][cin][cout]; see pti_conv_desc strides. */
int pti_conv2d_direct(const void* x, const float* w_tck, const float* bias, const int64_t* in_stats,
                      const float* gamma, const float* beta, void* y, const pti_conv_desc* d,
                      pti_stream_t s);

/* Derived operands of the degenerate-channel convs (conv_in / conv_out of MONAI's Encoder / Decoder) in one launch:
 * per entry, from the fp32 master weight w [cout][cin][3][3]:  w_tck [9][cin][cout] (forward operand of pti_conv2d_direct),
 * w_tck_t [9][cout][cin] with the taps reversed (its data-gradient operand), wpad = the weight copied into a zero-padded
 * master [cout'][pad_cin][3][3] (rows co < cout, columns ci < cin; the rest of the buffer is left as it is -- allocate it
 * zeroed) that the MFMA packer reads, and bpad[0..cout) = b.  Any of the outputs may be NULL. */
#define PTI_DIRECT_REPACK_MAX 8
typedef struct {
  const float* w; const float* b;
  float* w_tck; float* w_tck_t; float* wpad; float* bpad;
  int cout, cin, pad_cin, reserved;
} pti_direct_repack_entry;
typedef struct {
  pti_direct_repack_entry e[PTI_DIRECT_REPACK_MAX];
  int n;
} pti_direct_repack_table;
int pti_direct_repack(const pti_direct_repack_table* t, pti_stream_t s);

/* Weight/bias gradient of pti_conv2d_direct (autograd of nn.Conv2d for the degenerate layers):
 * dw[tap*st_tap + cw*st_cw + k*st_k] += sum_p narrow[p][k] * P(wide)[p + sgn*(tap offset)][cw]
 * for every narrow channel k < cn; wide is dense NHWC bf16 with cw channels (prologue P optional),
 * narrow is fp32/bf16 with element strides narrow_stride[n,h,w,c].  dbias_wide[cw] += column sums
 * of wide, dbias_narrow[k] += sum of narrow (either may be NULL).  Per-block partials go to `workspace`
 * (plain stores) and are summed in block order by a second launch: deterministic, += into the outputs.
 * The per-block partial size is cn * (80 * (cw / 8) + 1) floats.  The launch halves its block count until its partials
 * fit workspace_bytes; a workspace smaller than one block's partials is refused (PTI_EINVAL) before any launch.  */
int pti_wgrad_direct(const void* wide, const void* narrow, float* dw, float* dbias_wide,
                     float* dbias_narrow, const int64_t* in_stats, const float* gamma,
                     const float* beta, int n, int h, int w, int cw, int cn, int ksize, int sgn,
                     int prologue, int groups, float eps, int narrow_f32, int wide_f16,
                     const int64_t* narrow_stride, int64_t dw_stride_tap, int64_t dw_stride_cw,
                     int64_t dw_stride_k, void* workspace, int64_t workspace_bytes, pti_stream_t s);

/* ---- convolution weight gradient (autograd of nn.Conv2d, MFMA path) ----------------------- */
int64_t pti_conv_wgrad_workspace_bytes(int cout, int cin, int ksize, int splits);
/* dw[cout][cin][k][k] (fp32, OIHW) and dbias[cout] (=, or += when accumulate) from dy and the
 * SAME x / prologue / mode the forward conv saw (prologue is recomputed in the loader).  Split-K
 * partials go to `workspace` with plain stores and are summed in a fixed order (deterministic). */
int pti_conv_wgrad_mfma(const void* x, const void* dy, const int64_t* in_stats, const float* gamma,
                        const float* beta, float* dw, float* dbias, void* workspace,
                        int64_t workspace_bytes, int accumulate, const pti_conv_desc* d,
                        pti_stream_t s);
/* The same work as two calls (pti_conv_wgrad_mfma is exactly partials + reduce): the split-K partial launch,
 * which reports in *splits_out an opaque slab token (slab count, plus a flag bit for the slab layout the kernel it
 * picked writes), and the fixed-order slab reduction into dw / dbias, which takes that token as `splits`.  Lets a
 * caller time or overlap the two launches separately. */
int pti_conv_wgrad_mfma_partials(const void* x, const void* dy, const int64_t* in_stats,
                                 const float* gamma, const float* beta, void* workspace,
                                 int64_t workspace_bytes, const pti_conv_desc* d, int* splits_out,
                                 pti_stream_t s);
int pti_conv_wgrad_reduce(const void* workspace, int splits, float* dw, float* dbias,
                          int accumulate, const pti_conv_desc* d, pti_stream_t s);

/* Batched form for the training step: up to PTI_WGRAD_BATCH_MAX independent weight-gradient problems of plain
 * stride-1 3x3 convs on bf16 inputs WITHOUT prologue (x = the saved activated input) in one partial launch + one
 * reduction launch.  A launch has ~11 us of fixed cost (dispatch, ring fill, cross-wave reduction, slab drain) against
 * 10..45 us of streaming per layer, and the layers' weight gradients are independent of each other, so the engine
 * collects them while backward walks the layers and flushes a batch at a time.  Deterministic like the single form.  */
#define PTI_WGRAD_BATCH_MAX 16
typedef struct pti_wgrad_job {
  const void* x;    /* bf16 [n,h,w,cin] */
  const void* dy;   /* bf16 [n,h,w,cout] */
  float* dw;        /* fp32 [cout,cin,3,3] */
  float* dbias;     /* fp32 [cout] or NULL */
  int32_t n, h, w, cin, cout;
  int32_t accumulate;   /* += instead of = */
} pti_wgrad_job;
int pti_conv_wgrad_mfma_batched(const pti_wgrad_job* jobs, int njobs, void* workspace, int64_t workspace_bytes,
                                pti_stream_t s);
/* The kernel mode 0..3 that pti_conv_wgrad_mfma_batched files a job of this shape under (one partial launch per mode
 * present in a call, issued 3, 2, 1, 0), or a negative value for a shape it refuses.  Pure host arithmetic (reads the
 * PTI_WGRAD_V6 / PTI_WGRAD_V4_COB2 knobs the way the launch does); no GPU call.  */
int pti_conv_wgrad_batched_mode(int n, int h, int w, int cin, int cout);

/* ---- GroupNorm(+SiLU) backward, 2x2 sum pool ---------------------------------------------- */
/* dx = d/dx of act(GroupNorm(x)) given da (+ dres added), dgamma/dbeta += ; sums: float [n][c][2] scratch
 * (written, need not be zeroed); partials: float scratch of n * pti_gn_bwd_blocks(n, hw, c) * c * 2 elements;
 * stats as produced by pti_gn_stats on x.  (autograd of nn.GroupNorm+F.silu)
 * No floating-point atomics anywhere on this path: every workgroup stores its partial {sum dy, sum dy*xhat} row,
 * pti_gn_sums_finalize's kernel adds the rows in a fixed order and ONE workgroup of the apply kernel folds the
 * samples into dgamma / dbeta, so the backward pass is bitwise reproducible run to run.          */
int pti_gn_bwd_blocks(int n, int hw, int c);
int pti_gn_bwd(const void* x, const void* da, const void* dres, void* dx, const int64_t* stats,
               const float* gamma, const float* beta, float* sums, float* partials, float* dgamma,
               float* dbeta, int n, int hw, int c, int groups, float eps, int silu, int x_f16,
               pti_stream_t s);
/* Fused form used by the engine: the data-gradient conv computes dy = dA * act'(GN(gx)) in its epilogue and
 * stores, per pixel tile, the partial row gpartials[n][tile][c] = {sum dy, sum dy*xhat} (gx = the GroupNorm input,
 * same shape as the conv output; d->groups / d->eps describe that GroupNorm; d is a plain stride-1 / zero-insert
 * launch, w_packed the transposed+flipped pack; gpartials holds n * pti_conv_gnbwd_tiles(d) * cout * 2 floats).
 * pti_gn_sums_finalize(gpartials, sums, n, tiles, 2*cout) adds the tile rows up into sums[n][c][2];
 * pti_gn_bwd_apply then finishes dx = rstd*(gamma*dy - c1 - xhat*c2) [+ dres] and dgamma / dbeta +=.           */
int pti_conv_gnbwd_tiles(const pti_conv_desc* d);
/* Chained form (SURVEY 2.1 K4 "GroupNorm backward folded into the consumer's loader"): the launch's INPUT is not a
 * materialised gradient but the pair (g_in = dA * act'(GN(x_in)), x_in) of the GroupNorm ABOVE with its statistics,
 * weight and finalized sums {sum g, sum g*xhat} per (n, channel); the loader stages
 * rstd * (gamma * g - c1 - xhat * c2) -- what pti_gn_bwd_apply would have written -- and also writes it to dx_in_out
 * (bf16, same shape) for the weight gradient of the conv in between.  Everything else as pti_conv2d_mfma_gnbwd.
 * pti_conv_gnbwd_chain_supported(cin, cout, ksize): 3x3 with cin and cout multiples of 128.  The affine gradients of the
 * chained GroupNorm come from pti_gn_affine_grads (dgamma[c] += sum_n sums[n][c][1], dbeta[c] += sum_n sums[n][c][0]). */
int pti_conv_gnbwd_chain_supported(int cin, int cout, int ksize);
int pti_conv2d_mfma_gnbwd_chain(const void* g_in, const void* x_in, int x_in_f16, const int64_t* in_stats,
                                const float* in_gamma, const float* in_sums, void* dx_in_out, const void* w_packed,
                                const void* gx, const int64_t* gstats, const float* ggamma, const float* gbeta,
                                void* dy_out, float* gsums, const pti_conv_desc* d, int silu, pti_stream_t s);
int pti_gn_affine_grads(const float* sums, float* dgamma, float* dbeta, int n, int c, pti_stream_t s);
/* pti_gn_sums_finalize with pti_gn_affine_grads(affine_sums, dgamma, dbeta, n, affine_c) riding in the same launch */
int pti_gn_sums_finalize_affine(const float* partials, float* sums, int n, int tiles, int row_len, const float* affine_sums,
                                float* dgamma, float* dbeta, int affine_c, pti_stream_t s);
int pti_conv2d_mfma_gnbwd(const void* dy_in, const void* w_packed, const void* gx, const int64_t* gstats,
                          const float* ggamma, const float* gbeta, void* dy_out, float* gpartials,
                          const pti_conv_desc* d, int silu, pti_stream_t s);
int pti_gn_sums_finalize(const float* partials, float* sums, int n, int tiles, int row_len,
                         pti_stream_t s);
int pti_gn_bwd_apply(const void* x, const void* dy, const void* dres, void* dx, const int64_t* stats,
                     const float* gamma, const float* beta, const float* sums, float* dgamma,
                     float* dbeta, int n, int hw, int c, int groups, float eps, int x_f16,
                     pti_stream_t s);
/* y[n,h,w,c] = sum of the 2x2 block of x[n,2h,2w,c]: backward of nn.Upsample(nearest, 2x).     */
int pti_pool2x2_sum(const void* x, void* y, int n, int h, int w, int c, pti_stream_t s);

/* ---- mid-block self-attention (MONAI SpatialAttentionBlock -> SABlock, 1 head, dim = c) ------ */
/* qkv: bf16 [b,l,3c] (q|k|v per token, from the fused to_q/to_k/to_v 1x1 conv); o: bf16 [b,l,c] =
 * softmax(q k^T c^-0.5) v; lse2: fp32 [b,l] log2-sum-exp kept for the backward.  c in {64,128,256},
 * l % 64 == 0.  The l x l matrix is never materialised.                                          */
int pti_attention_fwd(const void* qkv, void* o, float* lse2, int b, int l, int c, pti_stream_t s);
/* dqkv: bf16 [b,l,3c] gradient w.r.t. qkv given dout (bf16 [b,l,c]); delta: fp32 [b,l] scratch.   */
int pti_attention_bwd(const void* qkv, const void* o, const void* dout, const float* lse2,
                      float* delta, void* dqkv, int b, int l, int c, pti_stream_t s);

/* ---- latent bottleneck (MONAI AutoencoderKL.encode tail / sampling / post_quant_conv) ------- */
/* h: fp32 [b,hw,l] (NHWC); eps/mu/sigma/logvar: fp32 [b,l,hw] (NCHW); zq: fp32 [b,hw,l].
 * eps NULL => deterministic z = mu.  Weights are the nn.Conv2d 1x1 masters [l][l], biases [l]. */
int pti_latent_head_fwd(const float* h, const float* eps, const float* wm, const float* bm,
                        const float* wl, const float* bl, const float* wp, const float* bp,
                        float* mu, float* sigma, float* logvar, float* zq, int b, int hw, int l,
                        pti_stream_t s);
int pti_post_quant(const float* z_nchw, const float* wp, const float* bp, float* zq_nhwc, int b,
                   int hw, int l, pti_stream_t s);
/* backward of pti_post_quant: dz (NCHW, may be NULL), gwp/gbp +=.  workspace: float scratch of
 * PTI_POST_QUANT_BWD_WS_FLOATS(l) elements (per-workgroup partials, added up in a fixed order by a second
 * launch: no float atomics, see pti_latent_head_bwd).                                             */
#define PTI_POST_QUANT_BWD_MAX_BLOCKS 256
#define PTI_POST_QUANT_BWD_WS_FLOATS(l) (PTI_POST_QUANT_BWD_MAX_BLOCKS * ((l) * (l) + (l)))
int pti_post_quant_bwd(const float* dzq_nhwc, const float* z_nchw, const float* wp, float* dz_nchw,
                       float* gwp, float* gbp, float* workspace, int b, int hw, int l,
                       pti_stream_t s);
/* backward of pti_latent_head_fwd: dh, and g* += the six 1x1-conv parameter gradients.  workspace: float scratch
 * of PTI_LATENT_BWD_WS_FLOATS(l) elements -- every workgroup stores its partial gradients there and a second
 * launch adds them up in a fixed order (no float atomics, bitwise reproducible: l == 4 -- the reference's latent
 * width -- keeps its partials in registers, other widths sum 128-element chunks in element order through LDS).   */
#define PTI_LATENT_BWD_MAX_BLOCKS 512
#define PTI_LATENT_BWD_WS_FLOATS(l) (PTI_LATENT_BWD_MAX_BLOCKS * 3 * ((l) * (l) + (l)))
int pti_latent_head_bwd(const float* h, const float* eps, const float* wm, const float* bm,
                        const float* wl, const float* bl, const float* wp, const float* bp,
                        const float* dzq, const float* dmu, const float* dsigma, float* dh,
                        float* gwm, float* gbm, float* gwl, float* gbl, float* gwp, float* gbp,
                        float* workspace, int b, int hw, int l, pti_stream_t s);

/* ---- loss step (reference src/pti_ldm_vae/models/losses.py:25-30,62-66; train_vae.py:393-394) */
/* out2[0] += mean recon loss (L1, or L2 when l2), out2[1] += mean_b KL; d_* receive the gradient
 * of recon + kl_weight*kl (NULL to skip).  third_mode 0: third used as log-variance (the
 * reference call site); 1: third is sigma, input_is_logvar=False semantics.  workspace: float scratch of
 * PTI_VAE_LOSS_WS_FLOATS elements (per-workgroup partials, added up in a fixed order by a second launch).   */
#define PTI_VAE_LOSS_MAX_BLOCKS 1024
#define PTI_VAE_LOSS_WS_FLOATS (2 * PTI_VAE_LOSS_MAX_BLOCKS)
int pti_vae_loss(const float* recon, const float* images, int64_t npix, const float* mu,
                 const float* third, int64_t nlat, int batch, float* out2, float* d_recon,
                 float* d_mu, float* d_third, float* workspace, int l2, int third_mode,
                 float kl_weight, pti_stream_t s);

/* ---- AR-VAE attribute regularisation (reference src/pti_ldm_vae/models/losses.py:69-166; train_vae.py:403-417) */
/* mu: fp32 [b,l,hw] (NCHW z_mu); attrs: fp32 [na,b] attribute values of the local batch; channels[q] / deltas[q]:
 * latent channel and tanh slope of attribute q; pair_mask: NULL = every ordered pair i != j ("all"), else uint8
 * [na,b,b] with mask[q][i][j] != 0 for the sampled pairs ("subset").  Writes per_attr[q] = mean over the selected pairs
 * with a_i != a_j of (tanh(delta (z_j - z_i)) - sign(a_j - a_i))^2 with z = mu.mean(hw) (0 when no pair qualifies) and
 * counts[q] = that number of pairs; d_mu (NULL to skip) += gamma * d(sum_q per_attr[q]) / d mu.  No atomics.        */
int pti_ar_vae_loss(const float* mu_nchw, int b, int l, int hw, const float* attrs, const int32_t* channels,
                    const float* deltas, int na, const uint8_t* pair_mask, float gamma, float* per_attr,
                    int32_t* counts, float* d_mu, pti_stream_t s);

/* ---- optimiser (torch.optim.Adam defaults, train_vae.py:301) on a flat fp32 arena ----------- */
int pti_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, int step, float grad_scale, pti_stream_t s);

/* ---- guarded optimiser step: global-norm clip, skip on a non-finite gradient, EMA of the weights ----
 * Three launches per step on the caller's stream, no atomics, no host read-back: the decision stays in `ctl`, a
 * persistent control record of PTI_GRAD_GUARD_COLUMNS doubles per optimiser (zeroed once by its owner):
 *   0 applied_steps  1 skipped_steps  2 sumsq of the last step  3 norm = grad_scale * sqrt(sumsq), before clipping
 *   4 coef           5 skip (0 | 1)   6 bias1 = 1 - beta1^t     7 bias2_sqrt = sqrt(1 - beta2^t), t = applied_steps + 1
 *   8 the EMA decay in effect         9 grad_scale * coef, the factor the step applies to g
 * (columns 0..7, 64 bytes, are what a host reads back; 8 and 9 pass values to pti_adam_step_guarded.)
 * pti_grad_guard_partials(n): workgroups of the norm pass = {sumsq, non-finite count} pairs in `partials` -- a function
 *   of n only, at most PTI_GRAD_GUARD_PARTIALS_CAP, 0 for n < 1; pure host arithmetic.
 * pti_grad_guard: g fp32 [n] (4-byte alignment suffices), partials: 2 * pti_grad_guard_partials(n) doubles of scratch, 16-byte aligned.
 *   fp64 sum of squares in a fixed order; bad = a non-finite element or a non-finite norm; skip = bad and skip_nonfinite;
 *   coef = min(1, max_norm / (norm + 1e-6)) when max_norm > 0 and not bad, else 1 (max_norm 0: no clipping).  A skipped
 *   step advances skipped_steps only; any other advances applied_steps and renews columns 6..8, the decay being
 *   min(ema_decay, (1 + t) / (10 + t)) (ema_decay 0: no EMA).
 * pti_adam_step_guarded: pti_adam_step's arithmetic on g * ctl[9] with the bias corrections of ctl[6..7]; with `ema`
 *   (NULL: none) also ema += (1 - ctl[8]) * (p_new - ema) in the same pass.  With ctl[5] set nothing is written.      */
#define PTI_GRAD_GUARD_PARTIALS_CAP 1024
#define PTI_GRAD_GUARD_COLUMNS 10
int pti_grad_guard_partials(int64_t n);
int pti_grad_guard(const float* g, int64_t n, double grad_scale, double max_norm, int skip_nonfinite, float beta1,
                   float beta2, double ema_decay, double* partials, double* ctl, pti_stream_t s);
int pti_adam_step_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                          float beta2, float eps, const double* ctl, pti_stream_t s);

/* ---- layout casts at the model boundary ------------------------------------------------------ */
int pti_cast_nchw_f32_to_nhwc_bf16(const float* x, void* y, int n, int c, int hw, pti_stream_t s);
int pti_cast_nhwc_bf16_to_nchw_f32(const void* x, float* y, int n, int c, int hw, pti_stream_t s);

/* ---- input pipeline ---------------------------------------------------- */
/* Batch form of the reference's per-sample transform chain Resize(patch_size) [MONAI default mode "area" =     *
 * adaptive average pooling] -> LocalNormalizeByMask -> float32 (data/dataloaders.py:319-329,                    *
 * data/transforms.py:8-32).  src: the raw fp32 images of the batch concatenated; offsets[b], hw[b] = {H, W}:    *
 * where image b starts and its size (device arrays); out: [b][1][hp][wp] fp32; stats: device scratch of 3*b     *
 * doubles (zeroed here).                                                                                        */
int pti_preprocess_batch(const float* src, const int64_t* offsets, const int32_t* hw, int b, int hp, int wp,
                         float* out, double* stats, pti_stream_t s);

/* ---- PatchDiscriminator + adversarial loss --------------------------------------------------------
 * Reference: vae_scripts/train_vae.py:266-279 (MONAI PatchDiscriminator(spatial_dims=2, num_layers_d=3, channels=32,
 * in_channels=1, out_channels=1, norm="INSTANCE")), :298 (PatchAdversarialLoss("least_squares")), :399-401 (generator
 * term), :447-458 (discriminator step).  A 4x4 convolution is lowered to patches x 1x1 convolution: the product, its
 * data gradient and its weight gradient run on pti_conv2d_mfma / pti_conv_wgrad_mfma (ksize 1); the entry points below
 * are the discriminator-specific passes.  Patches: bf16 [n][ho][wo][16*c], column = (ky*4 + kx)*c + channel,
 * ho = (h + 2 - 4)/stride + 1.  Normalisation tables: float [n][c][2] = {mean, rstd} (InstanceNorm2d, biased variance).
 * c in {32, 64, 128, 256}.  No floating-point atomics: results are bitwise reproducible.                              */
/* fp32 image [n][h][w] (1 channel) -> patches [n][h/2][w/2][32]: 16 taps of the 4x4 stride-2 pad-1 window + 16 zeros. */
int pti_pd_im2col_image(const float* img, void* patches, int n, int h, int w, pti_stream_t s);
/* bf16 [n][h][w][c] -> patches of act(norm(src)): norm optional ({mean,rstd} table), act = LeakyReLU(slope) if `act`. */
int pti_pd_im2col(const void* src, const float* norm, void* patches, int n, int h, int w, int c, int stride,
                  int act, float slope, pti_stream_t s);
/* nn.InstanceNorm2d statistics of y bf16 [n][hw][c] -> table [n][c][2] = {mean, 1/sqrt(var + eps)}. */
int pti_pd_in_stats(const void* y, float* table, int n, int hw, int c, float eps, pti_stream_t s);
/* Data gradient of pti_pd_im2col fused with LeakyReLU'(norm(y_prev)): g = act'(xhat) * col2im(d_patches), bf16
 * [n][h][w][c]; with a norm table also writes the InstanceNorm-backward block partials {sum g, sum g*xhat}:
 * partials float [n][pti_pd_col2im_blocks(n, h*w, c)][c][2], to be summed by pti_gn_sums_finalize(row_len = 2c).      */
int pti_pd_col2im_blocks(int n, int hw, int c);
int pti_pd_col2im(const void* d_patches, const void* y_prev, const float* norm, void* g, float* partials, int n,
                  int h, int w, int c, int stride, float slope, pti_stream_t s);
/* Gradient w.r.t. the 1-channel image from d_patches [n][h/2][w/2][32]: d_img = (accumulate ? d_img : 0) + scale * sum. */
int pti_pd_col2im_image(const void* d_patches, float* d_img, int n, int h, int w, float scale, int accumulate,
                        pti_stream_t s);
/* InstanceNorm backward, second pass: dy = rstd * (g - sums[0]/hw - xhat * sums[1]/hw); sums float [n][c][2]; dy may be g. */
int pti_pd_in_bwd_apply(const void* g, const void* y, const float* norm, const float* sums, void* dy, int n, int hw,
                        int c, pti_stream_t s);
/* PatchAdversarialLoss(criterion="least_squares"): loss_out[0] = mean((LeakyReLU_slope(logit) - target)^2) over `count`
 * 16-bit logits (element m at logits[m*stride]; slope 0.05 = MONAI's default activation, 1 = none).  loss_out must hold
 * 1 + pti_pd_lsgan_blocks(count) floats (block partials, summed in block order by a second launch).  When d_logits is
 * given, row m of bf16 [count][stride] = {grad_scale * (a_m - target) * LeakyReLU'(logit_m), 0, ...}: pass
 * grad_scale = weight * 2 / count for d(weight * loss)/d logits.                                                     */
int pti_pd_lsgan_blocks(int count);
int pti_pd_lsgan(const void* logits, int logits_f16, int stride, int count, float target, float slope,
                 float grad_scale, float* loss_out, void* d_logits, pti_stream_t s);

/* Final block of the discriminator (C -> 1 channel, 4x4, stride 1, pad 1) WITHOUT a patch matrix: with one output
 * channel the lowering above would move ~15x the bytes of its input.  The activated input LeakyReLU(norm(y_prev)) is
 * rebuilt on the fly; logits and d_logits are fp32 [n][h-1][w-1]; w is fp32 [16][c] (tap-major), bias fp32 [1].
 *   fwd:   logits = conv(act(norm(y_prev)), w) + bias
 *   dgrad: g = act'(xhat) * conv^T(d_logits, w)  (bf16 [n][h][w][c]) + InstanceNorm-backward partials as pti_pd_col2im
 *          (same pti_pd_col2im_blocks(n, h*w, c) rows)
 *   wgrad: partials float [pti_pd_final_wgrad_blocks(n,h,w)][16*c + 8] = per-block {dw[16][c], dbias, 0..}; sum the rows
 *          in block order (pti_gn_sums_finalize(partials, out, 1, blocks, 16*c + 8)).
 * pti_pd_lsgan accepts such fp32 logits with logits_f16 = 2 (stride in floats, d_logits then is float[count*stride]). */
int pti_pd_final_fwd(const void* y_prev, const float* norm, const float* w, const float* bias, float* logits, int n,
                     int h, int w_, int c, float slope, pti_stream_t s);
int pti_pd_final_dgrad(const float* d_logits, const void* y_prev, const float* norm, const float* w, void* g,
                       float* partials, int n, int h, int w_, int c, float slope, pti_stream_t s);
int pti_pd_final_wgrad_blocks(int n, int h, int w_);
int pti_pd_final_wgrad(const float* d_logits, const void* y_prev, const float* norm, float* partials, int n, int h,
                       int w_, int c, float slope, pti_stream_t s);

/* ---- LPIPS comparison tail of the perceptual term ----------------------------------------------------
 * Reference: vae_scripts/train_vae.py:299, :395-397 (monai.losses.PerceptualLoss(spatial_dims=2, network_type="squeeze")
 * = lpips.LPIPS(net="squeeze"): per feature tap normalize_tensor on both maps, squared difference, the 1x1 `lin` layer,
 * spatial mean).  a, b: fp32 NCHW feature maps [n][c][hw] of the reconstruction / the target, w: fp32 [c] (the lin
 * layer's weight).  The feature network itself stays torch ops (models/perceptual.py); this is its memory-bound tail.
 *   fwd: partials float [n][pti_lpips_tap_blocks(c, hw)] -- per-workgroup sums of sum_c w_c (a_c/(|a|+1e-10) -
 *        b_c/(|b|+1e-10))^2 over their pixels; the tap's value for sample i is sum(partials[i][:]) / hw.
 *        saved float [n][3][hw] = {|a_p|, |b_p|, sum_c w_c d_c a_c}: what the backward needs per pixel.
 *   bwd: ga [n][c][hw] = gout[i] * d value_i / d a   (gout fp32 [n]); b and w get no gradient (frozen network, target).
 * No atomics: bitwise reproducible.                                                                                   */
int pti_lpips_tap_blocks(int c, int hw);
int pti_lpips_tap_fwd(const float* a, const float* b, const float* w, float* saved, float* partials, int n, int c, int hw,
                      pti_stream_t s);
int pti_lpips_tap_bwd(const float* a, const float* b, const float* w, const float* saved, const float* gout, float* ga,
                      int n, int c, int hw, pti_stream_t s);

/* ---- trunk of the perceptual network: the passes between its convolutions ---------------------------
 * Reference: torchvision squeezenet1_1.features under lpips.LPIPS(net="squeeze") (train_vae.py:299): Fire modules and
 * MaxPool2d(kernel 3, stride 2, ceil_mode=True).  The Fire convolutions run on pti_conv2d_mfma (fp16 forward, bf16
 * data gradient); activations NHWC fp16, gradients NHWC bf16, element counts / channels multiples of 8.
 *   pti_relu_f16:        x = max(x, 0) in place.
 *   pti_relu_bwd:        g = y > 0 ? g : 0 in place (y = the ReLU OUTPUT).
 *   pti_relu_bwd_add:    g = y > 0 ? g + g2 : 0 in place (a tap's own gradient + the one arriving from later layers).
 *   pti_maxpool3s2_out:  pooled size of one spatial dimension.
 *   pti_maxpool3s2_fwd:  y [n][ho][wo][c] = max over the (clipped) 3x3 windows of x [n][h][w][c].
 *   pti_maxpool3s2_bwd:  gx (+)= gather of gy over the windows whose maximum the element is (no atomics).
 *   pti_nchw_f32_to_nhwc_f16 / pti_nhwc_bf16_add_to_nchw_f32: the trunk's boundary with torch's layout (tap 0):
 *                        y[n][p][c] = (fp16) x[n][c][p];   y[n][c][p] += (float) g[n][p][c];   c a multiple of 64.
 *   pti_lpips_tap_nhwc_*: pti_lpips_tap_* on the trunk's layout -- a, b fp16 [n][hw][c], ga bf16 [n][hw][c]; same
 *                        `saved` / `partials` contract with pti_lpips_tap_nhwc_blocks(c, hw); c = 8 * L * k with
 *                        L in {8, 16, 32, 64}, k <= 4 (0 blocks = unsupported channel count).
 *   pti_squeeze_conv1_*: the first layer (3 -> 64, 3x3, stride 2, no padding, + ReLU) for a ONE-channel image whose three
 *                        copies the reference scales per channel (ensure_three_channels + lpips ScalingLayer), folded
 *                        into a 1 -> 64 convolution: w10 fp32 [10][64] = {W'[tap][co] = sum_c W[co][c][tap] / scale_c,
 *                        b'[co] = b[co] - sum_c shift_c / scale_c * sum_tap W[co][c][tap]}.  x fp32 [n][h][w];
 *                        fwd: y fp16 [n][(h-3)/2+1][(w-3)/2+1][64] = tap 0;  bwd: dx fp32 [n][h][w] from the bf16
 *                        gradient g w.r.t. tap 0 (ReLU mask taken from t0 = y; t0 = NULL: g is already masked).           */
int pti_relu_f16(void* x, int64_t count, pti_stream_t s);
int pti_relu_bwd(void* g, const void* y, int64_t count, pti_stream_t s);
int pti_relu_bwd_add(void* g, const void* g2, const void* y, int64_t count, pti_stream_t s);
int pti_maxpool3s2_out(int h);
int pti_maxpool3s2_fwd(const void* x, void* y, int n, int h, int w, int c, pti_stream_t s);
int pti_maxpool3s2_bwd(const void* gy, const void* x, const void* y, void* gx, int n, int h, int w, int c, int accumulate,
                       pti_stream_t s);
int pti_squeeze_conv1_fwd(const float* x, const float* w10, void* y, int n, int h, int w, pti_stream_t s);
int pti_squeeze_conv1_bwd(const void* g, const void* t0, const float* w10, float* dx, int n, int h, int w, pti_stream_t s);
int pti_nchw_f32_to_nhwc_f16(const float* x, void* y, int n, int c, int hw, pti_stream_t s);
int pti_nhwc_bf16_add_to_nchw_f32(const void* g, float* y, int n, int c, int hw, pti_stream_t s);
/* Image-side boundary of the MFMA path for 2..8-channel images (csrc/narrow_pad.hip; replaces nothing in the reference:
 * conv_in / conv_out of MONAI's AutoencoderKL, src/pti_ldm_vae/models/autoencoder.py:67-79, take [N,C,H,W] fp32 images):
 *   pti_pad_nchw_to_nhwc32:   ya, yb [n][hw][32] 16-bit (fp16 if *_f16 else bf16; yb may be NULL) <- x [n][c][hw] fp32,
 *                             channels >= c written as zeros; 1 <= c <= 8.
 *   pti_slice_nhwc32_to_nchw: y [n][c][hw] fp32 <- the first c channels of x [n][hw][32] (fp16 if x_f16 else bf16). */
int pti_pad_nchw_to_nhwc32(const float* x, void* ya, void* yb, int n, int c, int hw, int a_f16, int b_f16, pti_stream_t s);
int pti_slice_nhwc32_to_nchw(const void* x, float* y, int n, int c, int hw, int x_f16, pti_stream_t s);
int pti_lpips_tap_nhwc_blocks(int c, int hw);
int pti_lpips_tap_nhwc_fwd(const void* a, const void* b, const float* w, float* saved, float* partials, int n, int c,
                           int hw, pti_stream_t s);
int pti_lpips_tap_nhwc_bwd(const void* a, const void* b, const float* w, const float* saved, const float* gout, void* ga,
                           int n, int c, int hw, pti_stream_t s);


/* ---- evaluation metrics (reference vae_scripts/evaluate_vae.py:87-99, src/pti_ldm_vae/utils/eval_metrics.py:6-64) ----
 * pred, target: fp32 NCHW [n][c][h][w] (dense).  out_n4[i] = {mse, mae, psnr, ssim} of sample i:
 *   clamp != 0: both images are clamped to [lo, hi] as they are loaded;
 *   mse / mae = mean over (c, h, w) of the squared / absolute difference;  psnr = 10 log10(data_range^2 / max(mse, 1e-12));
 *   ssim = mean over (c, h, w) of the SSIM map of an 11x11 separable window with taps taps11 (HOST array of 11 floats,
 *          copied into the launch: the Gaussian sigma 1.5 normalised to sum 1 as compute_ssim builds it), zero padding 5
 *          without renormalisation at the border, c1 = (k1 data_range)^2, c2 = (k2 data_range)^2; each channel is filtered
 *          on its own (the reference function only runs for c == 1).
 * workspace: pti_image_metrics_ws_floats(n, c, h, w) floats of device scratch (per-tile partial sums, plain stores, added
 * up in a fixed order by a second launch: no float atomics, bitwise reproducible, and a sample's result does not depend
 * on n or on its position in the batch).  pti_image_metrics_ws_floats is pure host arithmetic; 0 = unsupported shape
 * (any dimension < 1, or too large to index).  Any h, w >= 1 is supported.                                              */
int64_t pti_image_metrics_ws_floats(int n, int c, int h, int w);
int pti_image_metrics(const float* pred, const float* target, int n, int c, int h, int w, int clamp, float lo, float hi,
                      float data_range, float k1, float k2, const float* taps11, float* out_n4, float* workspace,
                      pti_stream_t s);

/* ---- latent-space analysis (reference src/pti_ldm_vae/analysis/latent_space.py:40-66 and :90-102; csrc/latent_stats.hip) ----
 * All matrices are fp32, row-major with a row stride in ELEMENTS (lda, ldb >= d; ldo >= n2); accumulation is fp32 in one
 * fixed order that depends on d only (fmaf chains over 512-column slabs, slab sums added in ascending order), no atomics:
 * results are bitwise reproducible and entry (i, j) depends on rows i and j only.
 *
 * pti_latent_pairwise: out[i][j] for rows i of a [n1][d] and j of b [n2][d] (a and b may be the same pointer):
 *   mode 0: sqrt(sum_k (a[i][k] - b[j][k])^2)   (scipy cdist, accumulated as differences);   mode 1: sum_k a[i][k] b[j][k].
 *   center (may be NULL): d floats subtracted from both operands as they are loaded; mode 1 with the column mean is the
 *   centred Gram matrix of PCA.
 *   workspace: pti_latent_pairwise_ws_floats(n1, n2, d) floats (never 0 for a supported shape; used when few output
 *   tiles meet long rows: d is then split over workgroups and a second launch folds the partial tiles in the same order).
 * pti_latent_group_stats: rows of a / b grouped by patient; seg_a, seg_b: int32 DEVICE arrays of patients + 1 ascending
 *   row offsets.  out_e4[p] = {|mean_a - mean_b|, mean over d of the population std of the patient's a rows (two-pass, as
 *   np.std; 0 for a single row), the same for b, mean of all cross distances} = compute_distance_metrics of that patient.
 *   A patient without rows on either side -- or whose offsets are not ascending or leave [0, n] -- gets four NaNs; the
 *   kernels never read outside the matrices whatever the tables hold.  Any d >= 1.
 *   workspace: pti_latent_group_stats_ws_floats(n1, n2, patients, d) floats, 8-byte aligned.
 * Both *_ws_floats are pure host arithmetic; 0 = unsupported shape (a dimension < 1 or too large to index).            */
int64_t pti_latent_pairwise_ws_floats(int n1, int n2, int d);
int pti_latent_pairwise(const float* a, int64_t lda, int n1, const float* b, int64_t ldb, int n2, int d, const float* center,
                        int mode, float* out, int64_t ldo, float* workspace, pti_stream_t s);
int64_t pti_latent_group_stats_ws_floats(int n1, int n2, int patients, int d);
int pti_latent_group_stats(const float* a, int64_t lda, int n1, const int32_t* seg_a, const float* b, int64_t ldb, int n2,
                           const int32_t* seg_b, int patients, int d, float* out_e4, float* workspace, pti_stream_t s);

/* ---- mask geometry (reference vae_scripts/compute_mask_metrics.py:38-68,176-193; csrc/mask_geometry.hip) ----
 * The per-pixel work behind the AR-VAE attribute files, for a batch of binary masks of mixed size in ONE launch (one
 * workgroup per image, no atomics, no workspace: integer results, bitwise reproducible, independent of batch position).
 *   src: the masks concatenated in their stored type -- elem 0 = uint8, 1 = uint16, 2 = float32; offsets[i]: ELEMENT
 *        offset of image i (any value: rows need no alignment beyond src's own, a multiple of the element size);
 *        hw[i] = {H, W}.  offsets / hw are device arrays, as for pti_preprocess_batch.
 *   foreground: integers != 0 (unsigned, the whole word); float32 by bit pattern, 0 < (int32) bits <= 0x7f800000, which is
 *        IEEE x > 0 whatever the denormal mode (NaN, -0.0, negatives: background; subnormals, +inf: foreground).
 *   bbox_b4[i] = {x0, y0, w, h} of all foreground pixels; {-1, -1, 0, 0} for a mask without any (its widths are all 0).
 *   The width of a row is last foreground column - first + 1 over the WHOLE row (gaps count), 0 for an empty row.
 *   bbox_widths[i][k], k < samples: width of row y0 + sample_rows[h * samples + k], where sample_rows is a device table
 *        int32 [max_h + 1][samples] built by the caller (the reference's np.linspace(0, h, samples + 2, dtype=int)
 *        truncates a float64 product and is not i*h/(samples+1): the host tabulates it, the kernel only looks it up);
 *        an entry that leaves the image gives width 0.
 *   bottom_widths[i][k], k < n_bottom: width of row clamp(H - 1 - bottom_offsets[k], 0, H - 1) (device array of offsets).
 *   samples == 0 / n_bottom == 0 are legal and the matching pointers may then be NULL.
 *   max_h: the caller's bound on every H, at most 4096 (the kernel keeps one {first, last} pair per row in LDS; above
 *        that PTI_EUNSUPPORTED).  An image with H > max_h, H < 1 or W < 1 is not read: bbox {-2, -2, 0, 0}, widths 0. */
int pti_mask_geometry(const void* src, const int64_t* offsets, const int32_t* hw, int b, int elem, int max_h,
                      const int32_t* sample_rows, int samples, const int32_t* bottom_offsets, int n_bottom,
                      int32_t* bbox_b4, int32_t* bbox_widths, int32_t* bottom_widths, pti_stream_t s);

/* ---- regression head, evaluation side (reference src/pti_ldm_vae/models/regression_head.py:30-78,
 *      src/pti_ldm_vae/utils/regression_utils.py:350-388, src/pti_ldm_vae/utils/metrics.py:6-37; csrc/regression_head.hip) ----
 * pti_mlp_head_fwd: forward of LatentRegressor in eval mode (dropout = identity) fused with the target de-normalisation
 *   and the per-row loss, two launches, no atomics.
 *   x: fp32 [n][d] with a row stride ldx >= d in ELEMENTS (torch.flatten(mu_nchw, 1)); params: ONE fp32 device buffer
 *   W0, b0, W1, b1, ... in nn.Linear layout ([out][in] row-major); dims: HOST array of n_layers + 1 widths, dims[0] == d.
 *   act between the layers: 0 relu, 1 gelu (exact erf form), 2 leaky_relu (slope 0.01), 3 elu (alpha 1).
 *   mean / std: fp32 [T] device arrays, both NULL or both set (a zero std was replaced on the host); targets: fp32 [n][T]
 *   or NULL; loss_kind: 0 MSE, 1 SmoothL1 (beta 1).
 *   pred[n][T] = out * std + mean (out without a normaliser); with targets rowloss[n] = sum_t l(out_t, (target_t - mean_t) /
 *   std_t), the loss on the NORMALISED scale as validate_one_epoch takes it (rowloss may be NULL without targets).
 *   Limits: 1 <= n_layers <= PTI_MLP_MAX_LAYERS, hidden widths <= PTI_MLP_MAX_WIDTH, T <= PTI_MLP_MAX_OUT, any d, n >= 1
 *   (up to 2^24); beyond them PTI_EUNSUPPORTED, NULL pointers / dimensions < 1 PTI_EINVAL, both before any launch.
 *   The sum over d has one order that depends on d only (fmaf chains over 512-column slabs in ascending k, slab sums added
 *   in ascending order); with few rows and a long d the slabs are split over workgroups and folded in the same order, so
 *   both routes give the same bits and row i of pred / rowloss depends on row i only (not on n, its position, the route).
 *   workspace: pti_mlp_head_ws_floats(n, d, dims, n_layers) floats (pure host arithmetic; 0 = unsupported shape).
 * pti_regression_metrics: one fixed-order fp64 fold over a whole evaluation set, pred / targets fp32 [n][t], rowloss [n]:
 *   out[0] = mean over the consecutive chunks of `batch` rows (the last may be short) of sum(rowloss) / (rows * t) -- the
 *   mean of per-batch loss means that validate_one_epoch returns, not the global mean; out[1 .. t] MAE per target,
 *   out[t+1 .. 2t] MSE per target, out[2t+1] / out[2t+2] their means over the targets (compute_regression_metrics).
 *   out: 2t + 3 doubles on the device; t <= PTI_MLP_MAX_OUT.                                                            */
#define PTI_MLP_MAX_LAYERS 8
#define PTI_MLP_MAX_WIDTH 1024
#define PTI_MLP_MAX_OUT 64
int64_t pti_mlp_head_ws_floats(int n, int d, const int32_t* dims, int n_layers);
int pti_mlp_head_fwd(const float* x, int64_t ldx, int n, int d, const float* params, const int32_t* dims, int n_layers,
                     int act, const float* mean, const float* std, const float* targets, int loss_kind, float* pred,
                     float* rowloss, float* workspace, pti_stream_t s);
int pti_regression_metrics(const float* pred, const float* targets, const float* rowloss, int n, int t, int batch,
                           double* out, pti_stream_t s);

/* ---- train-time geometric augmentation (the pipeline of the reference's src/pti_ldm_vae/data/augmentation.py as one
 *      displacement field and one gather; csrc/augment.hip) ----
 * pti_elastic_field: field[b][c] = alpha[b] * (G_sigma * n[b][c]), fp32 [B][2][H][W], channel 0 the x and channel 1 the y
 *   displacement in pixels.  One launch, no workspace, no atomics.
 *   n[b][c][y][x] is uniform in [-1, 1) and a pure function of (keys[b], c, i = y * W + x) in 32-bit arithmetic:
 *       mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16        (lowbias32)
 *       h = mix(mix(i + lo32(key)) ^ hi32(key) ^ (c * 0x9e3779b9));   n = ((h >> 8) - 2^23) / 2^23   (exact in fp32)
 *   G_sigma is scipy.ndimage.gaussian_filter(mode="reflect", truncate=4.0): radius int(4 sigma + 0.5), taps
 *   exp(-k^2 / 2 sigma^2) normalised (computed in fp64 on the host, cast once), applied along x then along y, borders by
 *   symmetric reflection d c b a | a b c d | d c b a.  Every output is one fmaf chain over the taps in ascending order
 *   per pass: a sample's field depends on its key, H, W and sigma only -- bitwise the same alone or in any batch.
 *   keys: uint64 [B] and alpha: fp32 [B] are DEVICE arrays; a sample with alpha == 0 gets zeros without the blur work.
 *   PTI_EINVAL before any launch: null pointers, dimensions < 1, sigma <= 0, radius > min(H, W) (one reflection must
 *   reach); PTI_EUNSUPPORTED: radius > PTI_ELASTIC_MAX_RADIUS (the LDS tile), B > 32767, H * W > 2^30.
 * pti_augment_warp: out[b][c][y][x] = bilinear sample of src[b][c] at s = M_b * (x + fx, y + fy, 1), pixel centres on
 *   integers, M_b = mat[b][0..5] the row-major 2x3 INVERSE map (output pixel -> source position), (fx, fy) =
 *   field[b][0..1][y][x] or 0 when field is NULL.  Taps outside the image contribute zero
 *   (scipy.ndimage.map_coordinates(order=1, mode="grid-constant", cval=0)).  One launch for the batch; the coordinate
 *   and the tap weights are computed once per pixel for all channels.  s is two fmaf chains, so a lattice map (entries
 *   0 / +-1, integer offsets, no field) gives exact integer coordinates, weights of exactly 0 and 1 and the source
 *   values unchanged.  src / out fp32 [B][C][H][W]; out must not overlap src (PTI_EINVAL, as null pointers and
 *   dimensions < 1); B > 65535: PTI_EUNSUPPORTED.                                                                       */
#define PTI_ELASTIC_MAX_RADIUS 30
int pti_elastic_field(const uint64_t* keys, const float* alpha, float sigma, int b, int h, int w, float* field,
                      pti_stream_t s);
int pti_augment_warp(const float* src, const float* mat, const float* field, int b, int c, int h, int w, float* out,
                     pti_stream_t s);

/* ---- exact t-SNE of the latent-space analysis (sklearn.manifold._t_sne: _joint_probabilities, _kl_divergence,
 *      _gradient_descent; csrc/tsne.hip) ----
 * Dense O(n^2) t-SNE with one degree of freedom into TWO columns, 2 <= n <= 8192.  No atomics; every sum has one order
 * that depends on n only, so results are bitwise reproducible.  Matrices are fp32 row-major with a row stride in ELEMENTS
 * (ldd, ldp >= n).  Refused before any launch: null pointers, n < 2, a row stride below n, a perplexity outside (0, n),
 * exaggeration <= 0, misaligned fp64 buffers, y_out == y_in, p == d2 (PTI_EINVAL); n > 8192, n_components != 2
 * (PTI_EUNSUPPORTED).
 * pti_tsne_affinities: d2 = SQUARED Euclidean distances [n][n].  Per row sklearn's _binary_search_perplexity in fp64 (beta
 *   from 1, at most 100 steps, tolerance 1e-5f on the entropy, p_ii = 0, a zero row sum replaced by 1e-8f), then
 *   p[i][j] = max((p_j|i + p_i|j) / S, 2.220446e-16) with S the fp64 sum of the symmetrised matrix, 0 on the diagonal:
 *   symmetric bit for bit.  plogp2: two DEVICE doubles {sum_ij p log p, sum_ij p}.  p doubles as the scratch of the
 *   conditional probabilities.  workspace: pti_tsne_affinities_ws_floats(n) floats, 8-byte aligned.
 * pti_tsne_step: one iteration of sklearn's _gradient_descent on y_in -> y_out (fp32 [n][2], two distinct buffers), update
 *   and gains (fp32 [n][2]) in place: num_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} num_ij,
 *   grad_i = 4 (exaggeration * sum_j p_ij num_ij (y_i - y_j) - sum_j num_ij^2 (y_i - y_j) / Z); gain += 0.2 where update and
 *   grad have opposite signs, *= 0.8 elsewhere, floored at 0.01; update = momentum * update - lr * gain * grad;
 *   y_out = y_in + update.  record: two DEVICE doubles, written only when with_record != 0 (the sum behind the KL value is
 *   fp64 work and one more single-wavefront launch folds the norm; sklearn, too, evaluates both only where it reads them):
 *   record[0] = KL(exaggeration * p || q) at y_in (q is not clamped at 2.2e-16 as sklearn's is); record[1] =
 *   |gain * grad|_2, the norm sklearn's stopping rule tests.  plogp2: as written by pti_tsne_affinities.
 *   workspace: pti_tsne_step_ws_floats(n, n_components) floats, 8-byte aligned.
 * Both *_ws_floats are pure host arithmetic; 0 = unsupported shape.                                                      */
int64_t pti_tsne_affinities_ws_floats(int n);
int pti_tsne_affinities(const float* d2, int64_t ldd, int n, float perplexity, float* p, int64_t ldp, double* plogp2,
                        float* workspace, pti_stream_t s);
int64_t pti_tsne_step_ws_floats(int n, int n_components);
int pti_tsne_step(const float* p, int64_t ldp, int n, int n_components, const float* y_in, float* y_out, float* update,
                  float* gains, const double* plogp2, float exaggeration, float momentum, float lr, double* record,
                  int with_record, float* workspace, pti_stream_t s);

/* ---- UMAP of the latent-space analysis (umap-learn: smooth_knn_dist, compute_membership_strengths, the fuzzy union with
 *      set_op_mix_ratio = local_connectivity = bandwidth = 1, optimize_layout_euclidean; csrc/umap.hip) ----
 * 3 <= n <= 8192 rows, 2 <= k <= 256 neighbours, k < n, TWO output columns, 1 <= n_epochs <= 2000.  No atomics; every sum has
 * one order: results are bitwise reproducible.  Everything runs on the caller's stream without a host synchronisation.
 * Refused before any launch: null pointers, n < 3, k outside [2, n), n_epochs < 1, a row stride below n, a capacity below
 * pti_umap_graph_capacity, a misaligned workspace, a or b <= 0, epoch < 0, a negative_sample_rate outside [0, 64],
 * y_out == y_in (PTI_EINVAL); n > 8192, k > 256, n_epochs > 2000, epoch >= 2000, n_components != 2 (PTI_EUNSUPPORTED).
 * pti_umap_knn: dist = fp32 distances [n][n], row stride ldd in ELEMENTS.  knn_idx int32 / knn_dist fp32 [n][k]: the k
 *   smallest entries of each row, ascending by (distance, column); the diagonal competes like any other entry.  Exact.
 * pti_umap_graph: per row rho = the smallest non-zero distance among the k (0 if none); sigma from umap-learn's search in
 *   fp64 on sum_{j=1..k-1} (d_j - rho > 0 ? exp(-(d_j - rho) / sigma) : 1) = log2 k (from 1, doubling while no upper bound
 *   is known, bisecting after, at most 64 rounds, stop at 1e-5), floored at 1e-3 * the row's mean distance (rho > 0) or the
 *   mean of all kNN distances (rho = 0); strengths 0 for the row itself, 1 for d - rho <= 0, exp(-(d - rho) / sigma)
 *   otherwise; w = a + a^T - a o a^T (symmetric bit for bit); entries with w * n_epochs < wmax are dropped.  CSR output:
 *   indptr int32 [n + 1] (indptr[n] = nnz, a DEVICE value), indices int32 (ascending within a row), weights fp32 and
 *   rate int32 = floor(w * 2^20 / wmax), each of `capacity` >= pti_umap_graph_capacity(n, k) = min(2 n k, n^2) entries
 *   of which the first nnz are written; rho, sigma fp32 [n].  workspace: pti_umap_graph_ws_floats(n, k) floats (a dense
 *   [n][n] scratch and a little more), 8-byte aligned.  Both queries are pure host arithmetic; 0 = unsupported shape.
 * pti_umap_epoch: one layout epoch as a Jacobi sweep, y_in -> y_out (fp32 [n][2], two distinct buffers).  The edge at CSR
 *   position p fires iff ((epoch + 1) * rate[p] >> 20) > (epoch * rate[p] >> 20).  For vertex i, with d2 = |y_i - y_j|^2,
 *     y_out[i] = y_in[i] + alpha * (2 sum_fired clip4(g_att (y_i - y_j)) + sum_fired sum_{s < rate} clip4(g_rep (y_i - y_v)))
 *     g_att = -2 a b d2^(b-1) / (a d2^b + 1),   g_rep = 2 b / ((0.001 + d2) (a d2^b + 1)),   both 0 at d2 = 0,
 *   clip4 clamps each coordinate to [-4, 4], v = (uint64(h) * n) >> 32 with
 *   h = mix(mix(seed + epoch) ^ (p * negative_sample_rate + s)) and mix the lowbias32 of pti_elastic_field.  `capacity` is
 *   the length of indices / rate: positions outside it and column indices outside [0, n) are skipped.                       */
int pti_umap_knn(const float* dist, int64_t ldd, int n, int k, int* knn_idx, float* knn_dist, pti_stream_t s);
int64_t pti_umap_graph_capacity(int n, int k);
int64_t pti_umap_graph_ws_floats(int n, int k);
int pti_umap_graph(const int* knn_idx, const float* knn_dist, int n, int k, int n_epochs, int* indptr, int* indices,
                   float* weights, int* rate, int64_t capacity, float* rho, float* sigma, float* workspace, pti_stream_t s);
int pti_umap_epoch(const int* indptr, const int* indices, const int* rate, int64_t capacity, int n, int n_components,
                   const float* y_in, float* y_out, double a, double b, double alpha, int epoch, uint32_t seed,
                   int negative_sample_rate, pti_stream_t s);

/* ---- UMAP transform: new rows into a fitted embedding (umap-learn's UMAP.transform; csrc/umap.hip) ----
 * m new rows against n training rows: 1 <= m <= 8192, 3 <= n <= 8192, 2 <= k <= 256, k < n, 1 <= n_epochs <= 2000, two
 * output columns.  No atomics, every sum has one order: bitwise reproducible.  Caller's stream, no host synchronisation.
 * Refused before any launch: null pointers, m < 1, n < 3, k outside [2, n), n_epochs < 1, a row stride below n, a
 * misaligned workspace, an epoch range outside 0 <= begin <= end <= n_epochs, a or b or initial_alpha <= 0, a
 * negative_sample_rate outside [0, 64], y_out overlapping y_train, y_out overlapping y_in without being y_in
 * (PTI_EINVAL); m or n > 8192, k > 256, n_epochs > 2000 (PTI_EUNSUPPORTED).
 * pti_umap_knn_cross: pti_umap_knn for a rectangular dist = fp32 [m][n] (new rows x training rows), row stride ldd in
 *   ELEMENTS -> knn_idx int32 / knn_dist fp32 [m][k], ascending by (distance, column).  Exact.
 * pti_umap_transform_graph: rho = 0 for every row (local_connectivity - 1 = 0); sigma from pti_umap_graph's fp64 search on
 *   sum_{t=1..k-1} (d_t > 0 ? exp(-d_t / sigma) : 1) = log2 k, floored at 1e-3 * the fp64 mean of all m k distances;
 *   weights[i][t] = d <= 0 ? 1 : exp(-d / sigma) as fp32 (bipartite: no self exclusion); wmax = the largest of them;
 *   rate[i][t] = floor(w * 2^20 / wmax) where w * n_epochs >= wmax, else 0; y0[i] = sum_t w_it Y[idx_it] / sum_t w_it
 *   over ALL k slots (umap-learn normalises before it thresholds; an index outside [0, n) takes no part), summed in
 *   fp64.  sigma fp32 [m], weights fp32 / rate int32 [m][k], y0 fp32 [m][2].  workspace:
 *   pti_umap_transform_graph_ws_floats(m, n, k) floats, 8-byte aligned (host arithmetic; 0 = unsupported shape).
 * pti_umap_transform_layout: epochs epoch_begin .. epoch_end - 1 of n_epochs in ONE launch, one wavefront per new row.
 *   Per epoch e, alpha = initial_alpha * (1 - e / n_epochs); slot t of row i fires iff rate > 0 and
 *   ((e + 1) * rate >> 20) > (e * rate >> 20); with p = i * k + t,
 *     y[i] = fp32(y[i] + alpha * sum_fired (clip4(g_att (y_i - Y[idx])) + sum_{s < negative_sample_rate} clip4(g_rep (y_i - Y[v]))))
 *   with g_att, g_rep, the hash and the d2 > 0 rule of pti_umap_epoch and v = (mix(mix(seed + e) ^ (p * negative_sample_rate
 *   + s)) * n) >> 32.  The attraction is NOT doubled: the training end does not move and there is no mirrored edge.  The
 *   rounding to fp32 after every epoch makes [0, T) in one launch bit-identical to T launches of one epoch.  A slot whose
 *   index lies outside [0, n) never fires.  y_in == y_out is allowed (a row reads only itself and y_train).            */
int pti_umap_knn_cross(const float* dist, int64_t ldd, int m, int n, int k, int* knn_idx, float* knn_dist, pti_stream_t s);
int64_t pti_umap_transform_graph_ws_floats(int m, int n, int k);
int pti_umap_transform_graph(const int* knn_idx, const float* knn_dist, int m, int k, const float* y_train, int n, int n_epochs,
                             float* sigma, float* weights, int* rate, float* y0, float* workspace, pti_stream_t s);
int pti_umap_transform_layout(const int* knn_idx, const int* rate, int m, int k, const float* y_train, int n, const float* y_in,
                              float* y_out, double a, double b, double initial_alpha, int n_epochs, int epoch_begin,
                              int epoch_end, uint32_t seed, int negative_sample_rate, pti_stream_t s);

/* ---- display normalisation of image planes (the reference's normalize_batch_for_display, src/pti_ldm_vae/utils/
 *      visualization.py:6-40, plus the rotation and the side-by-side canvas of train_vae.py:536-549,610-626;
 *      csrc/display.hip) ----
 * a, b: contiguous fp32 [n][h][w] (b may be NULL for nsrc = 1).  nsrc = 1, 2 or 3 picks the sources of image i: a[i]; a[i],
 * b[i]; a[i], b[i], fabsf(a[i] - b[i]) (formed in fp32).  Plane (i, s) is normalised on its own:
 *   foreground = v != 0 (so -0.0 is background); cnt = its size; cnt == 0: the plane is all 0 and its stats are {0, 0, 0};
 *   percentile q (numpy's linear method) of the SORTED foreground values s[0 .. cnt): vi = (cnt - 1) q / 100 in fp64,
 *   lo = floor(vi), hi = min(lo + 1, cnt - 1), p = s[lo] + (s[hi] - s[lo]) (vi - lo) in fp64 -- the order statistics are
 *   exact (a radix select on the values: ties are harmless);
 *   x = clip((v - p_low) / (p_high - p_low + 1e-8), 0, 1) in fp64, rounded to fp32 once; x < 1e-3f -> 0; background -> 0;
 *   the 8-bit value is (uint8_t)(x * 255.0f), truncated.
 * The plane is then rotated by rot_k quarter turns like torch.rot90(k = rot_k, dims = [H, W]) (0 .. 3; (ho, wo) = (h, w) for
 * even rot_k, (w, h) for odd) and stored in columns [s wo, (s + 1) wo) of image i of the canvas
 * out_f32 / out_u8 [n][ho][nsrc wo] -- torch.cat([rot90(a), rot90(b), rot90(|a - b|)], dim = 2).  Either canvas may be
 * NULL, not both; they must not overlap the inputs.  stats: fp64 [n nsrc][3] = {cnt, p_low, p_high}, always written,
 * 8-byte aligned.  low, high: percentiles, 0 <= low <= high <= 100.
 * Inputs must be FINITE: nothing is promised for NaN or Inf.  One launch, one workgroup per plane, no workspace, no
 * atomics on global memory, no host synchronisation: capturable, and bitwise reproducible.
 * Refused before any launch: null a / stats / both canvases, b missing for nsrc >= 2, nsrc outside 1 .. 3, a dimension < 1,
 * rot_k outside 0 .. 3, percentiles outside 0 <= low <= high <= 100, a misaligned buffer (PTI_EINVAL); h or w > 4096,
 * n nsrc > 65535 (PTI_EUNSUPPORTED).                                                                                      */
int pti_display_planes(const float* a, const float* b, int n, int h, int w, int nsrc, double low, double high, int rot_k,
                       float* out_f32, uint8_t* out_u8, double* stats, pti_stream_t s);

/* ---- attribute-ordering report of an AR-VAE (the full-set counterpart of pti_ar_vae_loss above; what the reference only
 *      shows by eye in vae_scripts/analyze_ar_channels.py; csrc/rank_agreement.hip) ----
 * zt: fp32 [l][ldz], CHANNEL-major per-image latent code z[c][i] (z_mu averaged over the map); attrs: fp32 [na][lda]
 * attribute values; row strides in ELEMENTS (ldz, lda >= n); channels / deltas: HOST arrays [na], copied into the launch --
 * channels[q] = the latent channel attribute q regularises (negative: no loss for that attribute), deltas[q] its tanh slope.
 * Every unordered pair i < j falls, for every (q, c), into exactly one of five classes; signs are decided by comparing the
 * two floats (>, <), never by subtracting (the library is built with -ffast-math):
 *   0 concordant: a_j != a_i, z_j != z_i, same sign       1 discordant: a_j != a_i, z_j != z_i, opposite signs
 *   2 z_tied:     a_j != a_i, z_j == z_i                   3 a_tied:     a_j == a_i, z_j != z_i        4 both_tied
 * counts: int64 [na][l][5] in that order, EXACT; the five sum to n (n - 1) / 2.
 * loss_sum: fp64 [na] = sum over the unordered pairs with a_i != a_j of (tanh(delta_q (z_j - z_i)) - sign(a_j - a_i))^2 with
 *   z of channel channels[q] (0 for a negative channel): the summand of pti_ar_vae_loss, which runs over ORDERED pairs -- the
 *   term is symmetric, so loss_sum / (concordant + discordant + z_tied) is the same mean.  The summand is formed in fp64
 *   from the fp32 inputs and added in fp64 in one fixed order.
 * Two launches (256 x 256 tiles of the upper triangle, then a fold of the per-workgroup partials in tile order): no atomics,
 * bitwise reproducible, on the caller's stream without a host synchronisation.  Inputs must be FINITE (a NaN ties).
 * workspace: pti_rank_agreement_ws_bytes(n, l, na) bytes, 8-byte aligned, ws_bytes = its size (pure host arithmetic;
 * 0 = unsupported shape).  Refused before any launch: null pointers, n < 2, l or na < 1, a row stride below n,
 * channels[q] >= l, a misaligned buffer, a misaligned or short workspace (PTI_EINVAL); n > 32768, l > 16, na > 16
 * (PTI_EUNSUPPORTED).                                                                                                   */
int64_t pti_rank_agreement_ws_bytes(int n, int l, int na);
int pti_rank_agreement(const float* zt, int64_t ldz, const float* attrs, int64_t lda, int n, int l, int na,
                       const int32_t* channels, const float* deltas, int64_t* counts, double* loss_sum, void* workspace,
                       int64_t ws_bytes, pti_stream_t s);

/* ---- disentanglement report: average ranks, their moments, joint histograms (csrc/disentanglement.hip) ----
 * Three integer primitives; every result is a count or a 64-bit integer sum, so it is EXACT, independent of the order of
 * evaluation and of row padding, and bitwise reproducible.  No two floats are ever subtracted (the library is built with
 * -ffast-math): values are compared, as floats or through their order-preserving integer keys.  All launches go to the
 * caller's stream without a host synchronisation.  Inputs must be FINITE: nothing is promised for the rank of a NaN.
 *
 * pti_tied_ranks: cols fp32 [m][ld] (row stride in ELEMENTS, ld >= n) -> rank2 int32 [m][n] (dense),
 *   rank2[c][i] = 2 #{j : x_j < x_i} + #{j : x_j == x_i} + 1 = twice the average rank (scipy rankdata "average");
 *   -0.0 ties with 0.0.  One launch, no workspace.
 * pti_rank_moments: rank2 int32 [m][n] as written above -> sums int64 [m] = sum_i rank2[a][i], gram int64 [m][m] =
 *   sum_i rank2[a][i] rank2[b][i] (64-bit products and sums).  One launch, no workspace.
 * Both refuse before any launch: null pointers, n < 2, m < 1, ld < n, a misaligned buffer (PTI_EINVAL); n > 32768, m > 32
 * (PTI_EUNSUPPORTED).                                                                                                    */
int pti_tied_ranks(const float* cols, int64_t ld, int n, int m, int32_t* rank2, pti_stream_t s);
int pti_rank_moments(const int32_t* rank2, int n, int m, int64_t* sums, int64_t* gram, pti_stream_t s);

/* pti_joint_histogram: zt fp32 [l][ldz] channel-major codes and attrs fp32 [na][lda] as in pti_rank_agreement; edges_z fp64
 * [l][bins] / edges_a fp64 [na][bins]: the LEFT edges of every column's bins, ascending (device memory).
 *   bin(x) = #{k : edges[k] <= (double)x} - 1, so the last bin is closed on the right and takes everything above it;
 *   a value below edges[0] has no bin: it is stored as 255 and counted nowhere (the caller is expected to refuse it).
 * bins_z uint8 [l][n], bins_a uint8 [na][n] (dense); counts int32 [na][l][bins][bins], indexed [q][c][bin_a][bin_z]: every
 * table sums to n; its row / column sums are the marginals.
 * Three launches: bin indices; per-workgroup tables in LDS (integer LDS adds) over chunks of 2048 rows; a fold of the chunks
 * in chunk order.  No atomics on global memory.  workspace: pti_joint_histogram_ws_bytes(n, l, na, bins) bytes, 4-byte
 * aligned, ws_bytes = its size (pure host arithmetic; 0 = unsupported shape).  Refused before any launch: null pointers,
 * n < 2, bins < 2, l or na < 1, a row stride below n, a misaligned buffer, a misaligned or short workspace (PTI_EINVAL);
 * n > 32768, l > 16, na > 16, bins > 32 (PTI_EUNSUPPORTED).                                                               */
int64_t pti_joint_histogram_ws_bytes(int n, int l, int na, int bins);
int pti_joint_histogram(const float* zt, int64_t ldz, const float* attrs, int64_t lda, int n, int l, int na, int bins,
                        const double* edges_z, const double* edges_a, uint8_t* bins_z, uint8_t* bins_a, int32_t* counts,
                        void* workspace, int64_t ws_bytes, pti_stream_t s);

/* ---- k-nearest-neighbour mutual information: radii and range counts (csrc/ksg.hip) ----
 * The integer part of the Kraskov-Stoegbauer-Grassberger estimator 1 as scikit-learn's _compute_mi_cc computes it, for every
 * (attribute q, channel c).  zt fp32 [l][ldz] and attrs fp32 [na][lda] as in pti_rank_agreement, FINITE; for the pair's
 * columns x = zt[c], y = attrs[q] and every row i:
 *   dx_ij = |x_i - x_j|, dy_ij = |y_i - y_j|, each ONE IEEE fp32 subtraction (round to nearest, subnormals kept);
 *   d_ij = max(dx_ij, dy_ij) for j != i -- self is left out by its index, so an exact duplicate of row i is a neighbour
 *   at distance 0;
 *   eps[q][c][i] = the k-th smallest d_ij, with multiplicity;         r = the largest fp32 below eps, or 0 when eps == 0;
 *   nx[q][c][i] = #{j != i : dx_ij <= r},   ny[q][c][i] = #{j != i : dy_ij <= r}.
 * eps fp32 [na][l][n], nx and ny int32 [na][l][n], dense.  Every cell is one of the distances or a count: independent of
 * the order of evaluation, of row padding and of the other columns in the call; bitwise reproducible.  One launch on the
 * caller's stream, no workspace, no atomics, no host synchronisation.  Refused before any launch: null pointers, k < 1,
 * l or na < 1, n < k + 1, a row stride below n, a misaligned buffer (PTI_EINVAL); k > 16, n > 32768, l > 16, na > 16
 * (PTI_EUNSUPPORTED).                                                                                                  */
int pti_ksg_counts(const float* zt, int64_t ldz, const float* attrs, int64_t lda, int n, int l, int na, int k, float* eps,
                   int32_t* nx, int32_t* ny, pti_stream_t s);

/* ---- shape comparison of image pairs (reference src/pti_ldm_vae/analysis/metrics.py:143-209,312-398: generate_clean_mask,
 *      dice_coefficient, iou, compute_object_dimensions, calculate_psnr; csrc/mask_compare.hip) ----
 * gt, pred: fp32 [n][h][w], dense, FINITE; 1 <= n, 1 <= h, w <= PTI_MASK_COMPARE_MAX_EDGE; threshold >= 0.
 * Per image two masks, by ordinary float compares: G = (gt != 0), R = (pred > threshold) | (pred < -threshold), so a value
 * exactly at +-threshold is background.  For a mask M:
 *   K(M): its 8-connected component with the most pixels; among equals the one that holds the smallest row-major pixel
 *         index; none for an empty M.
 *   F(M): K plus every pixel outside K that cannot reach the image border by 4-connected steps over pixels outside K (a ring
 *         of background is thought round the image) = scipy.ndimage.binary_fill_holes(K); smaller components that lie in a
 *         hole of K are part of it.                                                    P = F(R) below.
 * counts: int32 [n][PTI_MASK_COMPARE_COLUMNS], the columns in this order:
 *    0 n_gt = |G|           1 n_pred = |R|         2 components_gt       3 components_pred
 *    4 kept_gt = |K(G)|     5 kept_pred = |K(R)|   6 filled_pred = |P|   7 intersection = |P and G|   8 union = |P or G|
 *    9..12  gt_x, gt_y, gt_w, gt_h:         bounding box of K(G)     \  {-1, -1, 0, 0} when the mask is empty
 *   13..16  pred_x, pred_y, pred_w, pred_h: bounding box of K(R)     /  (the box of F(K) is the box of K)
 *   17..19  gt_width_upper / _middle / _lower:   pixels of G (the whole mask, not K(G)) in columns [x, x + w) of rows
 *           y + h / 4, y + h / 2, y + 3 h / 4 of the gt box (integer division); a COUNT, not last - first + 1
 *   20..22  pred_width_upper / _middle / _lower: the same counts of P in the pred box;   all 0 without a box
 *   23      status: 0, or 1 when a label-following loop ran out of its step budget (an internal error: every other column
 *           and all three sums of that row are then 0).  It arrives with the results: nothing is read back by the call.
 * sums: fp64 [n][3] = { sum over all pixels of (gt - pred P)^2 with the difference formed in fp64,  max(gt),  max(pred P) },
 *   pred P being pred inside P and 0 elsewhere.  The sum is added in one fixed order: bitwise reproducible.
 * One launch, one workgroup per image; labelling is a union-find with integer atomicMin on parents kept in the workspace, so
 * the root of a component is its smallest index whatever the scheduling: every result is independent of the image's place in
 * the batch and of what the workspace held before.  Runs on the caller's stream without a host synchronisation.
 * workspace: pti_mask_compare_ws_bytes(n, h, w) bytes, 4-byte aligned, ws_bytes = its size (pure host arithmetic; 0 =
 * unsupported shape).  Refused before any launch: null pointers, n, h or w < 1, a threshold that is negative or NaN, a
 * misaligned buffer, a misaligned or short workspace (PTI_EINVAL); h or w above the cap (PTI_EUNSUPPORTED).              */
#define PTI_MASK_COMPARE_MAX_EDGE 1024
#define PTI_MASK_COMPARE_COLUMNS 24
int64_t pti_mask_compare_ws_bytes(int n, int h, int w);
int pti_mask_compare(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts, double* sums,
                     void* workspace, int64_t ws_bytes, pti_stream_t s);

/* ---- projection quality of the latent-space analysis (scikit-learn: manifold.trustworthiness, metrics.silhouette_samples;
 *      csrc/projection_quality.hip) ----
 * dist: fp32 [n][n], row stride ldd in ELEMENTS (ldd >= n), used in place; 3 <= n <= 8192.
 * pti_neighbor_ranks: nbr_idx int32 [n][m] dense, 1 <= m <= 256.  With j = nbr_idx[i][c],
 *     out[i][c] = 1 + #{ l != i : key(i, l) < key(i, j) },   key(i, l) = (bits of dist[i][l], -0 taken as 0) << 32 | l,
 *   pti_umap_knn's key: equal distances go to the lower column, and { j : rank <= k } is what pti_umap_knn returns for the
 *   row once its own column is left out.  j == i gives 0; a j outside [0, n) is not dereferenced and gives -1.  out int32
 *   [n][m].  Integers only; row i of out depends on row i of dist and of nbr_idx alone.
 * pti_segment_row_sums: seg int32 DEVICE array of groups + 1 ascending offsets with seg[0] = 0 and seg[groups] = n (the
 *   seg_a convention of pti_latent_group_stats), 1 <= groups <= 2048.  out[i][g] = sum_{j = seg[g]}^{seg[g+1]-1}
 *   (double)dist[i][j], fp64 [n][groups] dense; the entries are converted as they are loaded and added in ONE order that
 *   depends on the segment's length alone, so the bits of an entry depend on row i and that segment, not on n, groups or
 *   the launch.  An empty segment gives 0.0.  The kernel clamps offsets to [0, n] and treats a segment that does not
 *   ascend as empty: it never reads outside the row; the caller checks the table's ends.
 * pti_projection_distances: y fp32 [n][d], the projection's rows (row stride ldy >= d in ELEMENTS), 1 <= n <= 8192,
 *   1 <= d <= 8.  out[i][j] = (float)sqrt(sum_k ((double)y[i][k] - (double)y[j][k])^2), fp32 [n][n] with row stride
 *   ldo >= n: formed in fp64 and rounded once, so two entries of a row are ordered as the true distances are unless they
 *   round to the same fp32.  Symmetric bit for bit, zero diagonal.  (pti_latent_pairwise accumulates in fp32; for the
 *   long latent rows that is the design, for a picture's coordinates the fp64 route is free.)
 * One launch each on the caller's stream; no workspace, no atomics, no host synchronisation; bitwise reproducible.
 * Refused before any launch: null pointers, n < 3 (pti_projection_distances: n < 1, d < 1), m < 1, groups < 1, a row
 * stride below the row length, a misaligned buffer (PTI_EINVAL); n > 8192, m > 256, groups > 2048, d > 8 (PTI_EUNSUPPORTED). */
int pti_neighbor_ranks(const float* dist, int64_t ldd, int n, const int32_t* nbr_idx, int m, int32_t* out, pti_stream_t s);
int pti_segment_row_sums(const float* dist, int64_t ldd, int n, const int32_t* seg, int groups, double* out, pti_stream_t s);
int pti_projection_distances(const float* y, int64_t ldy, int n, int d, float* out, int64_t ldo, pti_stream_t s);

/* ---- co-ranking curves and the Shepard figure of a projection (Lee & Verleysen's Q_NX / B_NX / R_NX / LCMC; Kruskal's
 *      stress-1; csrc/coranking.hip) ----
 * 4 <= n <= 8192 columns everywhere; row strides in ELEMENTS, at least n; matrices are used in place.
 * pti_full_ranks: dist fp32 [m][n] holds rows row0 .. row0 + m - 1 of an n-column distance matrix (0 <= row0, row0 + m <= n).
 *     out[r][j] = 1 + #{ l != i : key(i, l) < key(i, j) },  i = row0 + r,  out[r][i] = 0,
 *   with pti_neighbor_ranks' key (the fp32 bits, -0 taken as 0, above the column): every row of out is a permutation of
 *   0 .. n - 1.  out int16 [m][n], row stride ldo, any 2-byte alignment.  One workgroup per row sorts the row's keys in LDS.
 * pti_coranking_fold: rank_high / rank_low int16 [m][n], two such tables of the same rows.  For every entry with BOTH ranks
 *   in [1, n - 1] (anything else, the own column's 0 included, is skipped and never used as an index), with b = max of the
 *   two: hist[0][b] += 1 where they are equal, hist[1][b] += 1 where rank_low < rank_high (an intrusion), hist[2][b] += 1
 *   where rank_high < rank_low (an extrusion); hist uint32 [3][n] dense, ADDED to (the caller zeroes it; calls over row
 *   blocks compose).  sqdiff[r] = the sum over the same entries of (rank_high - rank_low)^2, int64 [m], written.
 * pti_shepard_fold: dist_high / dist_low fp32 [n][n].  sums[i] = { sum d_high^2, sum d_low^2, sum d_high d_low } over
 *   j != i, fp64 [n][3] dense, written: products formed in fp64 (exact) and added in ONE order that depends on n alone.
 *   hist[bh][bl] += 1 for every such pair, bh = (int)(d_high * scale[0]) and bl = (int)(d_low * scale[1]) in fp32, each
 *   clamped to [0, bins - 1] (+inf and NaN: the last bin); scale: a DEVICE pair of fp32; 2 <= bins <= 128; hist uint32
 *   [bins][bins] dense, ADDED to.
 * One launch each on the caller's stream; no workspace; integer atomics only, so every output is bitwise reproducible.
 * Refused before any launch: null pointers, n < 4, m < 1, a row range outside the matrix, a row stride below n, bins < 2,
 * a misaligned buffer (PTI_EINVAL); n > 8192, bins > 128 (PTI_EUNSUPPORTED). */
int pti_full_ranks(const float* dist, int64_t ldd, int m, int n, int row0, int16_t* out, int64_t ldo, pti_stream_t s);
int pti_coranking_fold(const int16_t* rank_high, int64_t ldh, const int16_t* rank_low, int64_t ldl, int m, int n, uint32_t* hist,
                       int64_t* sqdiff, pti_stream_t s);
int pti_shepard_fold(const float* dist_high, int64_t ldh, const float* dist_low, int64_t ldl, int n, const float* scale, int bins,
                     double* sums, uint32_t* hist, pti_stream_t s);

/* ---- pair registration: straighten both sides of a pair, then align the prediction (reference
 *      src/pti_ldm_vae/analysis/metrics.py:229-310: straighten_image, align_images_by_bottom_20_center; appended to
 *      csrc/mask_compare.hip) ----
 * G, R, K(.), F(.), the threshold t and the shape limits are those of "shape comparison" above; x is the column, y the row
 * (y points down); all images of a call have one shape h x w.
 * 1. Cleaned prediction: c = pred where P = F(K(R)), else 0.0f  (the reference's prediction * (mask > 0)).
 * 2. Orientation, per side: the region is F(K(G)) on side 0 (ground truth) and P on side 1 (prediction).  Its six raw moments
 *    m00, m10, m01, m20, m11, m02 are the int64 sums of 1, x, y, x^2, x y, y^2 over the region (exact), and
 *      A = m00 m20 - m10^2,  B = m00 m11 - m10 m01,  C = m00 m02 - m01^2        (int64; they fit in 61 bits at 1024 x 1024).
 *    B == 0 (decided on the integers): beta = 0 when C >= A, else beta = +pi/2 with cos beta = 0.0 and sin beta = 1.0 EXACTLY
 *    -- an upright, mirror-symmetric or round object is not rotated at all.  Otherwise theta = atan2((double)(2 B),
 *    (double)(A - C)) / 2 and beta = theta - pi/2 when theta > 0, else theta + pi/2: the rotation of least magnitude that makes
 *    the major axis vertical.  An empty region has m00 = 0 and asks for no rotation (beta = 0, cos = 1, sin = 0); the caller
 *    skips such a pair.  (The reference fits an ellipse to the largest outer contour's points: a deliberate difference.)
 * 3. Rotation about cx = w / 2, cy = h / 2 (integer division).  Output pixel (x, y) takes the source point
 *      sx = (cx + cos beta (x - cx)) - sin beta (y - cy),     sy = (cy + sin beta (x - cx)) + cos beta (y - cy)
 *    in fp64, associated as written (a product may be fused with the sum that follows it).  fx = floor(sx),
 *    tx = (float)(sx - fx), likewise y.  The output is the 4 x 4 cubic convolution over source columns fx - 1 .. fx + 2 and rows
 *    fy - 1 .. fy + 2, indices clamped to the image (replicate border), with Keys' weights for a = -0.75 in fp32:
 *      w0 = ((a (t + 1) - 5 a)(t + 1) + 8 a)(t + 1) - 4 a,   w1 = ((a + 2) t - (a + 3)) t^2 + 1,
 *      w2 = w1 of 1 - t,                                     w3 = ((1 - w0) - w1) - w2,
 *    a row is ((w0 v0 + w1 v1) + w2 v2) + w3 v3 over its columns, the pixel the same chain over the four rows; fp32, never
 *    re-associated, multiply-adds possibly fused.  At t = 0 the weights are exactly 0, 1, 0, 0: with beta = 0 (or a quarter
 *    turn's exact coefficients) the output is a copy of the source pixels, bit for bit but for a -0.0f, which comes out as
 *    +0.0f.  The WHOLE image is rotated (gt itself, and c), not only the kept component.
 * 4. Alignment: the rows used are the last h / 5.  In the rotated ground truth and the rotated prediction the mask is
 *    pixel != 0; centre = (sum of the columns of the set pixels) / (their count), integer division; shift = centre_gt -
 *    centre_pred; aligned[y][x] = rotated_pred[y][x - shift], 0.0f where x - shift leaves the row.
 *
 * pti_mask_moments: gt, pred fp32 [n][h][w] dense and finite -> cleaned fp32 [n][h][w] (rule 1),
 *   moments int64 [n][2][PTI_MASK_MOMENTS_COLUMNS], side 0 = ground truth, side 1 = prediction, the columns
 *      0 m00  1 m10  2 m01  3 m20  4 m11  5 m02  6 A  7 B  8 C  9 status (0, or 1 when a label-following loop overran its
 *      step budget: every other column of that row is then 0 and its coefficients ask for no rotation),
 *   coeffs fp64 [n][2][3] = { beta, cos beta, sin beta }.
 *   One launch, grid (n, 2): one workgroup per (image, side), same labelling, fill and step budgets as pti_mask_compare.
 *   workspace: pti_mask_moments_ws_bytes(n, h, w) bytes (twice pti_mask_compare's: three planes per image AND side), 4-byte
 *   aligned; every word read is written earlier in the same launch.
 * pti_warp_cubic: gt, pred fp32 [n][h][w] (pred is usually `cleaned`), coeffs as above (only cos and sin are read) ->
 *   out_gt, out_pred fp32 [n][h][w] (rule 3).  One launch, grid (row tiles, n, 2), no workspace.  For coefficients that are
 *   not a rotation the kernel still reads inside the images only.  The outputs must not alias the inputs.
 * pti_align_bottom: rot_gt, rot_pred fp32 [n][h][w], h >= 5 -> aligned fp32 [n][h][w] (rule 4),
 *   info int32 [n][PTI_ALIGN_BOTTOM_COLUMNS]: 0 centre_gt  1 centre_pred  2 count_gt  3 count_pred  4 shift
 *      5 status: 0, +1 when the ground truth has no set pixel in those rows, +2 when the prediction has none; a centre
 *      without pixels is -1, and with a non-zero status the shift is 0 (aligned is then a copy of rot_pred).
 *   One launch, one workgroup per image, no workspace.  aligned must not alias an input.
 * All three run on the caller's stream without a host synchronisation and are bitwise reproducible; rows do not depend on
 * their place in the batch.  Refused before any launch: null pointers, n, h or w < 1, a threshold that is negative or NaN,
 * a misaligned buffer, a misaligned or short workspace, aliased outputs (PTI_EINVAL); h or w above
 * PTI_MASK_COMPARE_MAX_EDGE, n > 65535, and for pti_align_bottom h < 5 (PTI_EUNSUPPORTED).                              */
#define PTI_MASK_MOMENTS_COLUMNS 10
#define PTI_ALIGN_BOTTOM_COLUMNS 6
int64_t pti_mask_moments_ws_bytes(int n, int h, int w);
int pti_mask_moments(const float* gt, const float* pred, int n, int h, int w, float threshold, float* cleaned, int64_t* moments,
                     double* coeffs, void* workspace, int64_t ws_bytes, pti_stream_t s);
int pti_warp_cubic(const float* gt, const float* pred, const double* coeffs, int n, int h, int w, float* out_gt, float* out_pred,
                   pti_stream_t s);
int pti_align_bottom(const float* rot_gt, const float* rot_pred, int n, int h, int w, float* aligned, int32_t* info,
                     pti_stream_t s);

/* ---- uniform-window SSIM of an image pair (reference src/pti_ldm_vae/analysis/metrics.py:420:
 *      skimage.metrics.structural_similarity(gen, gt, data_range=gt.max() - gt.min()); csrc/ssim_uniform.hip) ----
 * x (the ground truth) and y (the cleaned prediction c of "pair registration" rule 1): fp32 [n][h][w], dense, finite,
 * 7 <= h, w <= PTI_MASK_COMPARE_MAX_EDGE.  Per image:
 *   W(a)(r, q) = the mean of a over rows r-3 .. r+3 and columns q-3 .. q+3, for the VALID pixels 3 <= r < h-3, 3 <= q < w-3
 *                only.  (skimage filters the whole image with mode='reflect' and crops 3 pixels per side before it averages,
 *                so no padded pixel ever reaches its result either.)
 *   ux = W(x), uy = W(y), uxx = W(x x), uyy = W(y y), uxy = W(x y);      cn = 49/48 (sample covariance);
 *   vx = cn (uxx - ux^2), vy = cn (uyy - uy^2), vxy = cn (uxy - ux uy);
 *   R  = max(x) - min(x) over the whole image (fp32 extremes, subtracted in fp64), or data_range when it is >= 0;
 *   C1 = (0.01 R)^2, C2 = (0.03 R)^2  (formed in fp64, rounded to fp32);
 *   S  = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2));   ssim = the mean of S over the (h-6)(w-6) valid pixels.
 * Arithmetic: per pixel fp32 -- a window sum is 7 row sums (columns ascending) added rows ascending, times 1/49; products may
 * be fused with the sum that follows them; the division is IEEE.  The moments are taken about a pixel of the window: with
 * (a, b) = (x, y) at row 4 ((r - 3) / 4) + 5 (integer division), column q -- a pixel of the window of (r, q), the same for
 * the four rows r that share (r - 3) / 4 -- the sums are of dx = x - a, dy = y - b, dx^2, dy^2, dx dy; ux = a + W(dx), uy = b + W(dy), and the covariances,
 * which do not depend on the origin, are cn (W(dx^2) - W(dx)^2) and so on.  (With raw moments an object near 100 loses five
 * digits in uxx - ux^2; with these the residuals are as small as the window's own spread.)  The mean is added in fp64 in ONE order that depends on h
 * and w alone (thread, wave butterfly, waves in order, tiles lane-strided): no floating-point atomics, bitwise reproducible,
 * and an image's row does not depend on n or on its place in the batch.
 * out: fp64 [n][2] = { ssim, R }.  R == 0 (a constant x; skimage divides 0 by 0 there) gives { 0.0, 0.0 }: the caller
 * reports "none".
 * At most three launches on the caller's stream, no host synchronisation: per-image min / max of x (skipped when data_range
 * >= 0), one workgroup per 32 x 32 tile of the valid region, a fixed-order finalize; R reaches the tile pass through the
 * workspace.  No pixel outside the image is read.
 * workspace: pti_ssim_uniform_ws_bytes(n, h, w) bytes, 8-byte aligned, ws_bytes = its size (pure host arithmetic; 0 =
 * unsupported shape); every word read is written earlier in the same call.  Refused before any launch: null pointers, n < 1,
 * a NaN data_range, a misaligned buffer, a misaligned or short workspace (PTI_EINVAL); h or w outside 7 ..
 * PTI_MASK_COMPARE_MAX_EDGE, n > 65535 (PTI_EUNSUPPORTED).
 *
 * pti_mask_compare_cleaned is pti_mask_compare -- the same launch, the same counts and sums bit for bit -- that also writes
 * cleaned fp32 [n][h][w] = pred inside P, 0.0f elsewhere (all 0.0f in a row whose status is 1): the y of the SSIM above and
 * the image the MSE is formed from, without a second labelling.  cleaned must not alias gt or pred.                        */
int64_t pti_ssim_uniform_ws_bytes(int n, int h, int w);
int pti_ssim_uniform(const float* x, const float* y, int n, int h, int w, double data_range, double* out, void* workspace,
                     int64_t ws_bytes, pti_stream_t s);
int pti_mask_compare_cleaned(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts,
                             double* sums, float* cleaned, void* workspace, int64_t ws_bytes, pti_stream_t s);

/* ---- surface distance between the two regions of a pair (Hausdorff, its percentile form, the average symmetric surface
 *      distance, surface Dice; csrc/surface_distance.hip) ----
 * pti_mask_compare_outputs is pti_mask_compare -- the same launch, the same counts and sums bit for bit -- with two optional
 * outputs, either of which may be null: cleaned as for pti_mask_compare_cleaned, and masks uint8 [n][h][w] with bit 0 = G
 * (gt != 0) and bit 1 = P (the filled largest component of the prediction): exactly the two regions the Dice is formed from.
 * (cleaned != 0 is NOT P: a filled hole can hold zeros.)  masks is all 0 in a row whose status is 1.  No output may alias an
 * input or the other output.
 *
 * pti_surface_distance: a, b uint8 [n][h][w], dense; they may be the same pointer.  A pixel p is foreground on side 0 when
 * a[p] & a_bits and on side 1 when b[p] & b_bits (1 <= bits <= 255; masks of pti_mask_compare_outputs: a == b, bits 1 and 2).
 *   Edge pixel: a foreground pixel with at least one of its four neighbours not foreground; pixels outside the image count as
 *               background.  (mask ^ binary_erosion(mask) with scipy's default cross: the rule of MONAI's get_mask_edges.)
 *   Distance:   for every edge pixel p of side s, d2(p) = min |p - q|^2 over the edge pixels q of side 1 - s: an exact
 *               integer, at most 2 * 1023^2.
 * counts: int32 [n][2][PTI_SURFACE_COLUMNS], per image and side the columns
 *    0 n_fg     foreground pixels              1 n_edge   edge pixels (m)            2 max_d2   the largest d2
 *    3 rank_lo  ((m - 1) percentile_pm) / 1000 in integer arithmetic
 *    4 d2_lo    the rank_lo-th smallest d2, counted from 0
 *    5 d2_hi    the next one when ((m - 1) percentile_pm) % 1000 != 0, else d2_lo
 *    6..9 within_j  edge pixels with d2 <= tol_d2[j]; 0 for j >= n_tol           10 status  0 (1: internal inconsistency)
 *   The percentile_pm / 1000 quantile of the distances, with linear interpolation, is
 *   sqrt(d2_lo) + (((m - 1) percentile_pm) % 1000) / 1000 * (sqrt(d2_hi) - sqrt(d2_lo)).
 * sums: fp64 [n][2]: the sum of sqrt(d2), correctly rounded roots, over the side's edge pixels, added in ONE order that depends
 *   on h and w alone (lane: left to right, wave butterfly, rows in order): no floating-point atomics, bitwise reproducible.
 * An empty side: if EITHER side of an image has no edge pixel, both its rows hold max_d2 = d2_lo = d2_hi = -1, rank_lo = 0,
 *   within = 0 and sum 0.0; n_fg and n_edge stay true.
 * tol_d2: HOST array of n_tol <= PTI_SURFACE_MAX_TOLERANCES int32 >= 0, read before the call returns (for a tolerance of t
 *   pixels pass floor(t t): for an integer d2, d <= t is d2 <= floor(t^2)).  0 <= percentile_pm <= 1000.
 * Three launches on the caller's stream, no host synchronisation: a column pass (edge flags, vertical distances), a row pass
 * (one wave per row; an edge pixel scans at most w columns) and a select pass per (image, side).  An image's rows do not
 * depend on n or on its place in the batch.
 * workspace: pti_surface_distance_ws_bytes(n, h, w) bytes (12 per pixel and image, plus a few KB), 8-byte aligned, ws_bytes =
 * its size (pure host arithmetic; 0 = unsupported shape); every word read is written earlier in the same call.  Refused before
 * any launch: null pointers, n, h or w < 1, bits outside 1 .. 255, percentile_pm outside 0 .. 1000, n_tol outside 0 ..
 * PTI_SURFACE_MAX_TOLERANCES, a negative tolerance, a misaligned buffer, a misaligned or short workspace (PTI_EINVAL); h or w >
 * PTI_MASK_COMPARE_MAX_EDGE, n > 32767 (PTI_EUNSUPPORTED).                                                                */
#define PTI_SURFACE_COLUMNS 11
#define PTI_SURFACE_MAX_TOLERANCES 4
int pti_mask_compare_outputs(const float* gt, const float* pred, int n, int h, int w, float threshold, int32_t* counts,
                             double* sums, float* cleaned_or_null, uint8_t* masks_or_null, void* workspace, int64_t ws_bytes,
                             pti_stream_t s);
int64_t pti_surface_distance_ws_bytes(int n, int h, int w);
int pti_surface_distance(const uint8_t* a, int a_bits, const uint8_t* b, int b_bits, int n, int h, int w, int percentile_pm,
                         const int32_t* tol_d2, int n_tol, int32_t* counts, double* sums, void* workspace, int64_t ws_bytes,
                         pti_stream_t s);

/* ---- two-sample permutation tests of two groups of latent rows (unbiased MMD^2, energy distance, Schilling-Henze
 *      nearest-neighbour share; csrc/two_sample.hip) ----
 * 4 <= n <= 8192 everywhere; dist: fp32 [n][n] of non-negative distances, row stride ldd >= n in ELEMENTS, used in place.
 * pti_distance_median: out (one DEVICE float) = the exact lower median of the M = n (n - 1) / 2 entries above the diagonal,
 *   element (M - 1) / 2 in ascending order, by an MSB-first radix select over the entries' bit patterns (-0 taken as 0):
 *   integer histograms only, no sort, no copy of the triangle, no host synchronisation.
 *   workspace: pti_distance_median_ws_bytes(n) bytes, 4-byte aligned (0 = unsupported n); cleared by the call.
 * pti_two_sample_kernel: out int32 [n][n] dense, entries in [0, 65535], zero diagonal.  With s = the scale,
 *     kind 0 (gaussian): out = rint(65535 * mean_b exp(-d^2 / (2 (bandwidths[b] s)^2))),  s = *scale (a DEVICE float, required)
 *     kind 1 (energy):   out = rint(65535 * d / s),  s = *scale, or with scale null the maximum entry of dist, found on the
 *                        device by an integer maximum over the bit patterns
 *   evaluated in fp64 from the fp32 distance and rounded once.  A scale that is not positive gives an all-zero matrix.
 *   bandwidths: HOST array of 1 .. 8 positive values, read before the call returns (kind 0 only).  scale_out: one DEVICE
 *   float that receives the scale used; it may be the scale pointer itself.
 * pti_knn_indicator: knn_idx int32 [n][k] dense, 1 <= k <= n.  out int32 [n][n] dense: out[i][j] = 1 where j is listed in
 *   row i of knn_idx and j != i, else 0.  An index outside [0, n) is skipped, never dereferenced.
 * pti_permutation_forms: w int32 [n][n] with entries in [0, 65535] (only the low 16 bits of an entry are used), row stride
 *   ldw >= n in ELEMENTS; it need not be symmetric.  masks uint8 [p][n] dense, any value but 0 taken as 1; 1 <= p <= 65536.
 *   out int64 [p][3] = { s^T W s,  s . (W 1),  s . (W^T 1) } for every row s of masks.  W is split into two int8 byte planes
 *   and T = S . plane runs on v_mfma_i32_16x16x64_i8 with i32 accumulators (|sum| <= 2^20); the planes, the labellings and
 *   the tiles are combined in 64-bit integers.  Every output integer is exact, independent of tiling and launch order, and
 *   bitwise reproducible.
 *   workspace: pti_permutation_forms_ws_bytes(n, p) bytes (two planes of n_pad^2 bytes, p n_pad bytes of labellings, 8 n
 *   bytes of sums, n_pad = n rounded up to 64), 16-byte aligned, ws_bytes = its size (pure host arithmetic; 0 = unsupported
 *   shape); every byte read is written earlier in the same call.
 * All on the caller's stream without a host synchronisation.  Refused before any launch: null pointers, n < 4, p < 1, k
 * outside 1 .. n, a kind other than 0 / 1, a bandwidth count outside 1 .. 8 or a bandwidth that is not positive, a row stride
 * below the row length, a misaligned buffer, a short workspace (PTI_EINVAL); n > 8192, p > 65536 (PTI_EUNSUPPORTED).          */
int64_t pti_distance_median_ws_bytes(int n);
int pti_distance_median(const float* dist, int64_t ldd, int n, float* out, void* workspace, int64_t ws_bytes, pti_stream_t s);
int pti_two_sample_kernel(const float* dist, int64_t ldd, int n, int kind, const float* scale_or_null, const double* bandwidths,
                          int n_bandwidths, int32_t* out, float* scale_out, pti_stream_t s);
int pti_knn_indicator(const int32_t* knn_idx, int n, int k, int32_t* out, pti_stream_t s);
int64_t pti_permutation_forms_ws_bytes(int n, int p);
int pti_permutation_forms(const int32_t* w, int64_t ldw, int n, const uint8_t* masks, int p, int64_t* out, void* workspace,
                          int64_t ws_bytes, pti_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* PTI_VAE_H */
