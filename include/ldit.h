/*
 * ldit.h - C ABI of libldit_hip.so: the MI355X (gfx950) ViT / DiT encoder forward behind LayoutDiT's DiTBackbone.
 *
 * The reference has no FFI: its seam is the Python attribute `DiTBackbone.dit`, a HuggingFace `BeitModel`
 * (ref src/layoutdit/modeling/dit_backbone.py:26-31) whose only use is
 *     hs = self.dit(x).hidden_states            (ref src/layoutdit/modeling/dit_backbone.py:47)
 * Every entry point below replaces a piece of what that one line executes; the citations name the reference (ref:)
 * or the third-party code it delegates to (TF: = transformers models/beit/modeling_beit.py, pinned 4.49.0 at
 * ref uv.lock:1771-1772; line numbers from the installed 5.15.0 copy).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `ldit_stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - every pointer is a DEVICE pointer owned by the caller, 16-byte aligned, fp32 unless stated
 *   - the library allocates nothing and only ENQUEUES work on `stream` (asynchronous to the host; the caller synchronises)
 *     - safe to capture in a hipGraph.  Its only mutable process state: one bit per (kernel, device ordinal) recording that
 *     the kernel's dynamic-LDS limit was raised on that device (set lazily on the CURRENT device of the calling thread, which
 *     must be the device `stream` belongs to), and the diagnostic switches below (read from the environment once)
 *   - returns LDIT_OK (0) or a negative LDIT_E* code; ldit_last_error() returns a thread-local message
 *   - there is NO CPU fallback in this library: without a HIP device every compute entry point fails with LDIT_EHIP
 */
#ifndef LDIT_H
#define LDIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDIT_ABI_VERSION 6
#define LDIT_MAX_TAPS 8

enum ldit_status {
    LDIT_OK = 0,
    LDIT_EINVAL = -1,       /* bad argument (null pointer, misaligned, inconsistent geometry) */
    LDIT_EWORKSPACE = -2,   /* workspace / packed buffer too small */
    LDIT_EHIP = -3,         /* HIP runtime error (message in ldit_last_error) */
    LDIT_EUNSUPPORTED = -4  /* geometry outside what the kernels handle (see each function) */
};

enum ldit_dtype {
    LDIT_F32 = 0,  /* everything fp32 (exact-fp32 MFMA) */
    LDIT_BF16 = 1, /* GEMM / attention operands bf16, fp32 accumulation, residual stream / LayerNorm / softmax fp32; taps fp32 */
    LDIT_FP8 = 3,  /* BASELINE.json configs[4]: the four GEMMs of a layer on fp8 e4m3 (OCP) operands with per-tensor scales,
                      fp32 accumulation; attention on bf16 q|k|v; residual stream / LayerNorm / softmax fp32; taps fp32.
                      Weight scales (one per output channel) are measured by ldit_pack_weights; the four per-tensor
                      activation scales per layer come from
                      ldit_set_fp8_act_scales (calibration is the caller's job) */
    LDIT_F32X3 = 4, /* fp32 forward with every GEMM operand held as TWO bf16 planes x ~= p0 + p1 (p0 = bf16(x), p1 = bf16(x - p0):
                      16 significant bits) and every product computed as p1.q0 + p0.q1 + p0.q0 on the bf16 MFMA (16x the fp32
                      matrix rate) with fp32 accumulation - "bf16x3" -, the two products of the attention included.  Residual stream, LayerNorm,
                      softmax, erf-GELU, biases and taps are fp32 exactly as in LDIT_F32.  Whole-path error vs float64: 4.4 - 5.6e-6
                      relative L2 (LDIT_F32: 7 - 9e-7), i.e. inside the fp32 build's own parity gates (2e-5), 180x inside the north-star 1e-3.
                      The error of a dot product is 2^-17 of its TERMS: with activation outliers (LayerNorm channels x 60) the worst
                      element reaches 1.2e-3 of max(|ref|, 1) while the relative L2 stays 1.6e-5 - check parity per checkpoint. */
    LDIT_F32X6 = 5, /* the same with THREE planes (24 significant bits) and the six plane products down to 2^-24: fp32-grade error
                      (6 - 8e-7 vs float64: under the fp32 MFMA path's on every tap, at that of ATen's CPU fp32 forward) at 6 bf16 MFMAs per product */
    LDIT_MXFP8 = 6  /* LDIT_FP8's place without calibration: the four GEMMs of a layer on OCP MX operands - e4m3 codes with one
                      E8M0 (power-of-two) scale per 32 consecutive K-elements of a row, applied inside the block-scaled MFMA
                      (v_mfma_scale_f32_32x32x64_f8f6f4).  Weights are quantised by ldit_pack_weights; every activation block is
                      scaled from its own amax where it is produced (LayerNorm, attention epilogue, GELU epilogue), so there is no
                      scale state to set or to go stale, and a row's result does not depend on the other rows of the batch.
                      Attention on bf16 q|k|v; residual stream / LayerNorm / softmax fp32; taps fp32.  hidden, mlp % 128 == 0.
                      The format (everything tests against it):
                        codes [rows, K] e4m3fn, scales [rows, K / 32] bytes, row-major, no padding;
                        block exponent e = the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127]; byte = e + 127;
                          (amax = m 2^E, m in [0.5, 1): e = E - 9 if m <= 0.875 else E - 8) - nothing is clipped;
                        code = e4m3_RNE(x * 2^-e); an all-zero block has byte 0 and codes 0; a block holding Inf / NaN has byte
                          0xFF (its codes are unspecified);
                        value = code * 2^(byte - 127). */
};

/* order of the per-layer activation scales handed to ldit_set_fp8_act_scales (scale = amax / 448) */
enum ldit_fp8_act {
    LDIT_FP8_A_LN1 = 0,   /* layernorm_before output -> q|k|v GEMM */
    LDIT_FP8_A_ATTN = 1,  /* attention output        -> o_proj GEMM */
    LDIT_FP8_A_LN2 = 2,   /* layernorm_after output  -> fc1 GEMM */
    LDIT_FP8_A_GELU = 3,  /* gelu(fc1) output        -> fc2 GEMM */
    LDIT_FP8_A_COUNT = 4
};

/* epilogues of ldit_linear_f32 (what is fused behind the matmul) */
enum ldit_epilogue {
    LDIT_EPI_BIAS = 0,       /* Y = X W^T + b                         nn.Linear; TF:305-307 (q,k,v), TF:349 */
    LDIT_EPI_BIAS_GELU = 1,  /* Y = gelu_erf(X W^T + b)               TF:353-354, TF:activations.py:70-89 */
    LDIT_EPI_SCALE_RESID = 2,/* Y = R + lam (.) (X W^T + b)           TF:432-434 and TF:440-442 (LayerScale + residual) */
    /* train step, ldit_linear_bf16_ex only: */
    LDIT_EPI_F32 = 4,        /* Y fp32 = X W^T (+ b)                  dgrad into LayerNorm backward; wgrad (split-K slabs) */
    LDIT_EPI_GELU_BWD = 5,   /* Y bf16 = (X W^T) (.) aux              dgrad of fc2 times the saved GELU derivative */
    /* ldit_linear_bf16 and ldit_linear_bf16_ex only (every other linear entry refuses it with LDIT_EINVAL): */
    LDIT_EPI_BIAS_RELU = 6   /* Y bf16 = max(X W^T + b, 0)            fc6 / fc7 of the bf16 box head: relu of LDIT_EPI_BIAS's Y, bit for bit */
};

typedef void *ldit_stream;

/* Encoder geometry.  Mirrors the BeitConfig fields the path reads (TF:configuration_beit.py:72-102). */
typedef struct ldit_cfg {
    int32_t hidden;   /* C   hidden_size */
    int32_t layers;   /* L   num_hidden_layers */
    int32_t heads;    /* H   num_attention_heads ; head_dim = C / H */
    int32_t mlp;      /* F   intermediate_size */
    int32_t patch;    /* p   patch_size (square) */
    int32_t in_ch;    /* num_channels (3) */
    int32_t img_h;    /* input height, multiple of patch */
    int32_t img_w;    /* input width,  multiple of patch */
    int32_t n_taps;   /* how many hidden states the caller wants (<= LDIT_MAX_TAPS) */
    int32_t taps[LDIT_MAX_TAPS]; /* hidden-state indices, 0 = embedding output, l = after layer l
                                    (ref dit_backbone.py:33-34: d/3, d/2, 2d/3, d) */
    float ln_eps;     /* layer_norm_eps, 1e-12 for BEiT */
    int32_t dtype;    /* enum ldit_dtype */
    int32_t flags;    /* reserved, 0 */
} ldit_cfg;

/* Per-layer parameters, each exactly the tensor nn.Module.state_dict() holds (row-major [out, in] for Linear). */
typedef struct ldit_layer_weights {
    const void *ln1_w, *ln1_b;        /* layernorm_before        [C]       TF:390,426 */
    const void *wq, *bq;              /* attention q_proj        [C,C],[C] TF:305 */
    const void *wk;                   /* attention k_proj        [C,C]     TF:306 (NO bias) */
    const void *wv, *bv;              /* attention v_proj        [C,C],[C] TF:307 */
    const void *wo, *bo;              /* attention o_proj        [C,C],[C] TF:308 */
    const void *lam1;                 /* lambda_1                [C]       TF:397-403 */
    const void *ln2_w, *ln2_b;        /* layernorm_after         [C]       TF:391,438 */
    const void *w1, *b1;              /* mlp.fc1                 [F,C],[F] TF:349 */
    const void *w2, *b2;              /* mlp.fc2                 [C,F],[C] TF:350 */
    const void *lam2;                 /* lambda_2                [C] */
} ldit_layer_weights;

typedef struct ldit_weights {
    const void *patch_w;              /* embeddings.patch_embeddings.projection.weight [C,in_ch,p,p]  TF:81 */
    const void *patch_b;              /* ....projection.bias [C] */
    const void *cls;                  /* embeddings.cls_token [C]                                    TF:168 */
    const void *pos;                  /* position table for THIS input grid, [1 + (img_h/p)*(img_w/p), C]
                                         (= embeddings.position_embeddings when the grid is the table's own;
                                         otherwise the caller resamples it bicubically first, TF:113-151) */
    const ldit_layer_weights *layer;  /* HOST array of `layers` entries */
} ldit_weights;

/* ---- library ------------------------------------------------------------------------------------------------ */
int ldit_abi_version(void);
const char *ldit_last_error(void);
/* Diagnostic: the LDIT_* environment switches that force a tiling (tests reach every kernel instantiation through them; see
 * layoutdit_amd/csrc/ldit_common.h: DiagSwitches) are read ONCE, at first use; this re-reads them after the caller changed
 * one.  Not thread-safe against concurrent launches. */
int ldit_debug_reload_env(void);

/* ---- whole path: replaces `self.dit(x).hidden_states` (ref dit_backbone.py:47 ; TF:515-560) ------------------- */

/* Bytes of the packed parameter block for this geometry (one allocation the forward streams from). */
size_t ldit_packed_bytes(const ldit_cfg *cfg);

/* Gather the caller's parameter tensors into `packed` (device), fusing q/k/v into one [3C,C] matrix with bias
 * [bq ; 0 ; bv] (the key projection has no bias, TF:306).  Call again whenever parameters change. */
int ldit_pack_weights(const ldit_cfg *cfg, const ldit_weights *w, void *packed, size_t packed_bytes, ldit_stream stream);

/* LDIT_FP8 only: store the activation scales (HOST array, layers x LDIT_FP8_A_COUNT floats, all > 0) into `packed`.
 * Until this has been called after ldit_pack_weights the fp8 forward's output is undefined (scales are zero). */
int ldit_set_fp8_act_scales(const ldit_cfg *cfg, void *packed, size_t packed_bytes, const float *act_scales,
                            ldit_stream stream);

/* Scratch bytes ldit_vit_forward needs for a batch of `batch` images. */
size_t ldit_workspace_bytes(const ldit_cfg *cfg, int32_t batch);

/* Streams the forward of this (cfg, batch) runs on - host arithmetic, nothing is launched.  2: the fp32 forward of a large batch
 * runs its layers as two half-batch lanes, one on `stream` and one on an internal stream (one per device, created on first use and
 * kept), forked after the embedding and joined before the call returns to `stream`'s order: the entry points stay enqueue-only (no
 * synchronisation, no device allocation) and everything they enqueue is ordered against `stream` as if it ran there.  1: everything
 * runs on `stream` - every other build, small batches, the timed forward, and any forward enqueued on a capturing stream (a captured
 * forward is a linear graph).  The diagnostic switch LDIT_FWD_LANES=1|2 forces one lane / two lanes (fp32, batch >= 2).  0: bad cfg. */
int32_t ldit_forward_lanes(const ldit_cfg *cfg, int32_t batch);

/* x: [batch, in_ch, img_h, img_w] NCHW contiguous.  tap_out[i]: [batch, 1+P, C] row-major receives hidden state
 * cfg->taps[i] (the raw residual stream: no final LayerNorm, TF:504-506,557).  The pooler (TF:558,563-572) is not
 * computed: LayoutDiT never reads pooler_output. */
int ldit_vit_forward(const ldit_cfg *cfg, const void *packed, const void *x, int32_t batch, void *const *tap_out,
                     void *workspace, size_t workspace_bytes, ldit_stream stream);

/* The same forward fed by the detector's image list BEFORE its input transform (ref src/layoutdit/modeling/model.py:50-54:
 * GeneralizedRCNNTransform, fixed_size = (img_h, img_w) of cfg, image_mean = image_std = 0.5): `images` / `heights` / `widths` are
 * HOST arrays of `batch` entries (device pointers to [in_ch, h_i, w_i] planar images in [0, 1]; half_in != 0: fp16).  In the bf16 /
 * fp8 / split-fp32 builds the pass that writes the patch-embedding operand evaluates (bilinear(img) - mean) / std itself - no fp32
 * batch is materialised; the fp32 build, whose GEMM gathers pixels by LDS-DMA, produces the batch in its workspace first.  Either
 * way the taps EQUAL ldit_preprocess_* followed by ldit_vit_forward (one shared statement, csrc/image_blend.h). */
int ldit_vit_forward_images(const ldit_cfg *cfg, const void *packed, const void *const *images, const int32_t *heights,
                            const int32_t *widths, int32_t half_in, float mean, float std, int32_t batch, void *const *tap_out,
                            void *workspace, size_t workspace_bytes, ldit_stream stream);

/* ldit_vit_forward_images fed by uint8 images as a decoder leaves them (the pixel contract and the two layouts: ldit_preprocess_u8
 * below; `interleaved` stands where half_in stands).  Every build ldit_vit_forward_images serves, the same launches per build, fp32
 * taps, and they EQUAL ldit_preprocess_u8 followed by ldit_vit_forward. */
int ldit_vit_forward_images_u8(const ldit_cfg *cfg, const void *packed, const void *const *images, const int32_t *heights,
                               const int32_t *widths, int32_t interleaved, float mean, float std, int32_t batch, void *const *tap_out,
                               void *workspace, size_t workspace_bytes, ldit_stream stream);

/* Same, but brackets every kernel launch with HIP events on `stream`, synchronises, and ADDS the elapsed
 * milliseconds / launch counts per kernel family into ms[LDIT_K_COUNT] / launches[LDIT_K_COUNT].
 * Measurement aid for bench.py's roofline block; not for production use (it blocks the host). */
enum ldit_kernel_family {
    LDIT_K_GEMM = 0,      /* all MFMA GEMMs: patch-embed, qkv, o_proj, fc1, fc2 */
    LDIT_K_ATTENTION = 1,
    LDIT_K_LAYERNORM = 2,
    LDIT_K_OTHER = 3,
    LDIT_K_COUNT = 4
};
int ldit_vit_forward_timed(const ldit_cfg *cfg, const void *packed, const void *x, int32_t batch, void *const *tap_out,
                           void *workspace, size_t workspace_bytes, ldit_stream stream, double *ms, int64_t *launches);

/* ---- the kernels, one entry point each (unit parity tests; also usable on their own) -------------------------- */

/* Y[M,N] = epilogue(X[M,K] . W[N,K]^T).  fp32 MFMA.  K % 32 == 0, lda % 4 == 0.
 * bias[N] may be NULL (= 0).  lam[N], R[M,N] (row stride ldy) only for LDIT_EPI_SCALE_RESID; R may alias Y.
 * Y2 (optional, same shape/stride as Y) receives a second copy of the result (hidden-state tap). */
int ldit_linear_f32(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M,
                    int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2,
                    ldit_stream stream);

/* Row LayerNorm over the last axis, biased variance about the mean, y = (x-mu) rsqrt(var+eps) g + b.
 * C % 4 == 0, C <= 4096.  (nn.LayerNorm; TF:390-391,426,438) */
int ldit_layernorm_f32(const void *X, const void *gamma, const void *beta, void *Y, int64_t rows, int64_t C, float eps,
                       ldit_stream stream);

/* softmax(Q K^T * scale) V per head, no mask.  Q,K,V,O: [B, N, H*D] token-major with row strides ldq..ldo (floats);
 * head h occupies columns [h*D, (h+1)*D).  D == 64.  (TF:268-293, TF:323-338) */
int ldit_attention_f32(const void *Q, const void *K, const void *V, void *O, int64_t B, int64_t N, int64_t H,
                       int64_t D, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, ldit_stream stream);

/* Patch embedding + [cls ; patches] + position table (TF:81-90, TF:153-176).
 * x [B,in_ch,img_h,img_w] NCHW -> out [B, 1+P, C].  (in_ch*p*p) % 32 == 0, p % 4 == 0, img_w % 4 == 0. */
int ldit_embed_f32(const void *x, const void *patch_w, const void *patch_b, const void *cls, const void *pos, void *out,
                   int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream);

/* DiTBackbone tap post-processing (ref dit_backbone.py:50-61): drop CLS, view tokens as a [C,Gh,Gw] map, bilinear
 * rescale by `scale` in {4, 2, 1, 0.5} (align_corners=False).  tap [B,1+Gh*Gw,C] -> out [B,C,Gh*scale,Gw*scale] NCHW. */
int ldit_tap_to_map_f32(const void *tap, void *out, int64_t B, int64_t Gh, int64_t Gw, int64_t C, float scale,
                        ldit_stream stream);

/* Adjoint of ldit_tap_to_map_f32 (training through DiTBackbone.forward, ref dit_backbone.py:50-61 under loss.backward()):
 * dmap [B,C,Gh*scale,Gw*scale] NCHW contiguous -> dtap [B,1+Gh*Gw,C] (CLS row = 0).  Gather form, no atomics. */
int ldit_tap_to_map_bwd_f32(const void *dmap, void *dtap, int64_t B, int64_t Gh, int64_t Gw, int64_t C, float scale,
                            ldit_stream stream);

/* ---- bf16 path (first build; BASELINE configs 3-5) ------------------------------------------------------------------
 * Y[M,N] = epilogue(X[M,K] . W[N,K]^T), X and W bf16 (K-contiguous), fp32 accumulation on v_mfma_f32_32x32x16_bf16.
 * K % 64 == 0, lda % 8 == 0.  bias / lam fp32.  LDIT_EPI_BIAS, LDIT_EPI_BIAS_GELU and LDIT_EPI_BIAS_RELU write bf16 Y (the max of
 * LDIT_EPI_BIAS_RELU is taken on the fp32 value in front of the conversion: its Y is relu of LDIT_EPI_BIAS's Y bit for bit);
 * LDIT_EPI_SCALE_RESID reads the fp32 residual R (may alias Y), writes fp32 Y and the optional fp32 copy Y2. */
int ldit_linear_bf16(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M,
                     int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2,
                     ldit_stream stream);

/* softmax(Q K^T * scale) V per head; Q, K, V bf16 [B, N, H*D] token-major (row strides in bf16 elements), O bf16;
 * fp32 softmax and accumulation.  D == 64.  scale == 0 means "Q is already multiplied by scale * log2(e)" (what the packed
 * inference path delivers: ldit_pack_weights folds that factor into W_q / b_q of the bf16 and fp8 builds): the scores are then
 * exp2-domain exponents and the kernel subtracts the running maximum on the matrix pipe instead of per element. */
int ldit_attention_bf16(const void *Q, const void *K, const void *V, void *O, int64_t B, int64_t N, int64_t H, int64_t D,
                        int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, ldit_stream stream);

/* dst[i] = bf16(src[i]) (round to nearest even), n elements. */
int ldit_cast_f32_bf16(const void *src, void *dst, int64_t n, ldit_stream stream);

/* ---- split-fp32 building blocks (LDIT_F32X3 / LDIT_F32X6) ------------------------------------------------------------------
 * ldit_split_f32_planes: dst bf16 [rows, planes * cols] = the bf16 planes p0 | p1 (| p2) of src fp32 [rows, cols] (row stride lds),
 *   p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1); planes = 2 or 3; cols % 4 == 0.
 * ldit_layernorm_f32_planes: ldit_layernorm_f32 with the result written as such planes, Y bf16 [rows, planes * C].
 * ldit_linear_planes: Y = epilogue(X . W^T) for fp32 X [M,K] and W [N,K] given as planes Xp [M, planes * K] (row stride lda), Wp [N,
 *   planes * K]: the sum of 3 (planes = 2: x1 w0 + x0 w1 + x0 w0) or 6 (planes = 3: + x2 w0 + x1 w1 + x0 w2) plane products on
 *   v_mfma_f32_32x32x16_bf16 - per 64-deep k-tile, smallest first -, ONE fp32 accumulation chain per output element.  K % 64 == 0.  LDIT_EPI_BIAS and
 *   LDIT_EPI_SCALE_RESID write fp32 Y (row stride ldy); LDIT_EPI_BIAS_GELU (exact erf-GELU) writes Y as planes, bf16 [M, planes * N]. */
/* ldit_attention_planes: softmax(Q K^T) V per head on plane operands (the attention of LDIT_F32X3 / LDIT_F32X6; planes = 2 / 3).  Q, K, V
 *   point at plane 0 of their column slices of a bf16 matrix with row stride ld_in; plane s of a row lies s * plane_in elements
 *   further.  Q must already be multiplied by scale * log2(e) (ldit_pack_weights folds it into W_q / b_q of those builds).  Both
 *   products are the 3 / 6 plane products of ldit_linear_planes on the bf16 MFMA, softmax fp32.  O: bf16 [B*N, ldo], plane s of the
 *   fp32 result at column s * H * D.  D == 64. */
int ldit_attention_planes(const void *Q, const void *K, const void *V, void *O, int64_t B, int64_t N, int64_t H, int64_t D,
                          int64_t ld_in, int64_t plane_in, int64_t ldo, int32_t planes, ldit_stream stream);
int ldit_split_f32_planes(const void *src, int64_t lds, void *dst, int64_t rows, int64_t cols, int32_t planes, ldit_stream stream);
int ldit_layernorm_f32_planes(const void *X, const void *gamma, const void *beta, void *Y, int64_t rows, int64_t C, float eps,
                              int32_t planes, ldit_stream stream);
int ldit_linear_planes(const void *Xp, int64_t lda, const void *Wp, const void *bias, void *Y, int64_t ldy, int64_t M, int64_t N,
                       int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, int32_t planes, ldit_stream stream);

/* ldit_embed_f32's arithmetic on bf16 MFMA operands - the patch embedding of the bf16 / fp8 builds and of the train step
 * (TF:81-90, TF:153-176): x fp32 NCHW is rounded to a bf16 im2col matrix [B*P, in_ch*p*p] in `scratch` (that many bf16, 16-byte
 * aligned; one HBM-bound pass), multiplied with patch_w_bf16 [C, in_ch*p*p] (fp32 accumulation), bias and position rows added in
 * fp32, written to token rows 1.. of out fp32 [B, 1+P, C]; row 0 = cls + pos[0].  (in_ch*p*p) % 64 == 0, C % 4 == 0. */
int ldit_embed_bf16(const void *x, const void *patch_w_bf16, const void *patch_b, const void *cls, const void *pos, void *out,
                    void *scratch, int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream);

/* The same embedding fed by the detector's ragged image list instead of the resized batch (the input transform
 * of ref src/layoutdit/modeling/model.py:50-54 fused into the patch-embed load): `images` / `heights` / `widths` as for
 * ldit_preprocess_f32 (half_in != 0: fp16 images), img_h x img_w = the transform's fixed_size.  The pass that builds the bf16
 * im2col matrix evaluates (bilinear(img) - mean) / std itself - the statement of ldit_preprocess_f32, bit for bit - so the
 * result EQUALS ldit_preprocess_* followed by ldit_embed_bf16, without the fp32 batch in between (one launch and a write + read
 * of B * in_ch * img_h * img_w * 4 bytes less). */
int ldit_embed_bf16_images(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t half_in, float mean,
                           float std, const void *patch_w_bf16, const void *patch_b, const void *cls, const void *pos, void *out,
                           void *scratch, int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream);

/* ldit_embed_bf16_images fed by uint8 images (ldit_preprocess_u8 below: the pixel contract, the two layouts, `interleaved`): the
 * result EQUALS ldit_preprocess_u8 followed by ldit_embed_bf16.  One launch per 48 images, as its sibling. */
int ldit_embed_bf16_images_u8(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t interleaved, float mean,
                              float std, const void *patch_w_bf16, const void *patch_b, const void *cls, const void *pos, void *out,
                              void *scratch, int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream);

/* ---- fp8 (OCP e4m3) building blocks of the fp8 build (BASELINE.json configs[4]) -----------------------------------------
 * Symmetric scaling: activations per tensor (T ~= scale_T * q, scale_T = amax(T) / 448), weights per output channel
 * (W[n,:] ~= w_scales[n] * q[n,:]).
 *
 * ldit_linear_fp8:  Y = epilogue(ab_scale * w_scales[n] * (X8 . W8^T) + bias)  with X8 [M,K] (row stride lda BYTES =
 * elements) and W8 [N,K] fp8 e4m3, fp32 accumulation (v_mfma_f32_32x32x64_f8f6f4).  w_scales: device fp32 [N] or NULL
 * (then ab_scale = scale_X * scale_W, per tensor).  K % 128 == 0, lda % 16 == 0.  bias / lam fp32.  LDIT_EPI_BIAS writes bf16 Y; LDIT_EPI_BIAS_GELU writes fp8 Y =
 * sat(gelu(.) * out_inv_scale) (ldy in elements); LDIT_EPI_SCALE_RESID reads the fp32 residual R (may alias Y),
 * writes fp32 Y and the optional fp32 copy Y2. */
int ldit_linear_fp8(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M, int64_t N,
                    int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, float ab_scale,
                    float out_inv_scale, const void *w_scales, ldit_stream stream);

/* Per-output-channel weight quantisation: scales[n] = max|W[n,:]| / 448 (never 0), codes[n,:] = fp8(W[n,:] / scales[n]).
 * W fp32 [N,K] row-major, K % 4 == 0. */
int ldit_quant_rows_f32_fp8(const void *W, void *codes, void *scales, int64_t N, int64_t K, ldit_stream stream);

/* ---- MX (block-scaled e4m3) building blocks of the mxfp8 build (LDIT_MXFP8 above: the format) ------------------------------
 * ldit_quant_mx_f32_fp8: src fp32 [rows, K] (row stride lds elements, lds % 4 == 0, src 16-byte aligned) -> codes [rows, K]
 * (dense, 4-byte aligned) + scales [rows, K / 32].  K % 32 == 0. */
int ldit_quant_mx_f32_fp8(const void *src, int64_t lds, void *codes, void *scales, int64_t rows, int64_t K, ldit_stream stream);

/* ldit_linear_mxfp8:  Y = epilogue(X . W^T + bias) on MX operands: X codes [M,K] (row stride lda, lda % 128 == 0) with scales Xs
 * [M, lda / 32], W codes [N,K] with scales Ws [N, K / 32]; the block scales enter the MFMA, fp32 accumulation.  K % 128 == 0;
 * codes 16-byte aligned, scales 4-byte aligned.  LDIT_EPI_BIAS writes bf16 Y; LDIT_EPI_BIAS_GELU writes MX Y = codes [M, ldy]
 * + scales Ys [M, ldy / 32] of gelu(.) (N, ldy % 32 == 0); LDIT_EPI_SCALE_RESID: Y = R + lam (.) (.), fp32 (R may alias Y),
 * and the optional fp32 copy Y2.  Ys is ignored by the other two epilogues. */
int ldit_linear_mxfp8(const void *X, int64_t lda, const void *Xs, const void *W, const void *Ws, const void *bias, void *Y,
                      int64_t ldy, void *Ys, int64_t M, int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2,
                      ldit_stream stream);

/* ldit_layernorm_f32's statistics and affine, the row written as MX codes Y [rows, C] + scales Ys [rows, C / 32]; C % 32 == 0. */
int ldit_layernorm_mxfp8(const void *x, const void *gamma, const void *beta, void *Y, void *Ys, int64_t rows, int64_t C, float eps,
                         ldit_stream stream);

/* dst[i] = fp8_e4m3(src[i] * inv_scale), round to nearest even, SATURATING at +-448 (torch's cast yields NaN above
 * 464 instead); n elements, src 16-byte aligned, dst 4-byte aligned. */
int ldit_quant_f32_fp8(const void *src, void *dst, int64_t n, float inv_scale, ldit_stream stream);

/* *out (one device float) = max |src[i]|, i < n (0 for n == 0).  Enqueues a 4-byte memset + one kernel. */
int ldit_amax_f32(const void *src, int64_t n, void *out, ldit_stream stream);

/* Detector input transform (the step that produces `x`; ref src/layoutdit/modeling/model.py:50-54 configures
 * torchvision's GeneralizedRCNNTransform with fixed_size = (224, 224), image_mean = image_std = 0.5): for each image
 * [in_ch, h_i, w_i] in [0,1]:  (img - mean) / std, then bilinear resize (align_corners = False, no antialias) to
 * out_h x out_w, written as row i of the NCHW batch `out` [B, in_ch, out_h, out_w].  `images`, `heights`, `widths`
 * are HOST arrays of B entries (device pointers / sizes); at most 65535 images per call. */
int ldit_preprocess_f32(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t B, int32_t in_ch,
                        float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream);

/* Same with fp16 images (the reference's trainer casts images with .half() before the detector's transform,
 * ref src/layoutdit/training/trainer.py:153-155); arithmetic and output fp32. */
int ldit_preprocess_f16(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t B, int32_t in_ch,
                        float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream);

/* Same with uint8 images as a decoder leaves them.  A code c stands for (float)c / 255.0f, the correctly rounded single-precision
 * quotient (what ToTensor() computes on the CPU; c * (1 / 255) differs from it at 126 of the 256 codes), and everything after that
 * value is the statement of ldit_preprocess_f32: the result EQUALS, bit for bit, ldit_preprocess_f32 on the planar fp32 image
 * c / 255.  interleaved == 0: images[i] is planar, [in_ch, h_i, w_i] contiguous; interleaved == 1: [h_i, w_i, in_ch] contiguous
 * (channel c of pixel (y, x) at byte (y * w_i + x) * in_ch + c); any other value is LDIT_EINVAL.  images[i] may have ANY byte
 * alignment, and no byte outside [images[i], images[i] + in_ch * h_i * w_i) is read.  Output fp32, one launch per 48 images. */
int ldit_preprocess_u8(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t interleaved, int32_t B,
                       int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream);

/* ---- train-time augmentation: crop, scale jitter and flip inside the input transform -----------------------
 * A WINDOW of image i is five host integers (x0, y0, cw, ch, flip): the cw x ch pixels whose top-left one is column x0 of row y0 of
 * the page, mirrored left-right where flip == 1.  cw >= 1, ch >= 1, x0 >= 0, y0 >= 0, x0 + cw <= w_i, y0 + ch <= h_i, flip 0 or 1;
 * anything else is LDIT_EINVAL with a message that names the image, before any launch.  `windows` is a HOST array [B][5].
 *
 * ldit_preprocess_win_f32 / _f16 / _u8: ldit_preprocess_f32 / _f16 / _u8 on the windows instead of the whole pages.  With
 *   crop_i = images[i][:, y0 : y0 + ch, x0 : x0 + cw] (and .flip(-1) where flip is set), row i of `out` EQUALS, bit for bit, what the
 *   sibling without `_win` gives for a contiguous copy of crop_i: the same statement (csrc/image_blend.h) on the window's extent, the
 *   source row y0 + y, the source column x0 + x or, flipped, x0 + cw - 1 - x.  No copy is made, and no byte of a page outside its
 *   window is read.  Every other argument, the four image formats, the alignment rules and "one launch per 48 images" are the
 *   sibling's: the windows travel in the kernel arguments beside the image descriptors (no device-side table, no copy to the
 *   device).  windows == NULL: whole pages, no flip - the sibling itself.
 *
 * ldit_augment_targets_f32: the boxes of the same batch through the same windows, as the padded targets ldit_rpn_targets_f32 and
 *   ldit_roi_targets_f32 read.  gt_boxes fp32 [B, Gmax, 4] (x1, y1, x2, y2 in the page's pixels), gt_labels int32 [B, Gmax] or NULL,
 *   gt_count int32 [B] (clamped to [0, Gmax]); Gmax <= 512.  For each row g < gt_count[i], in fp32, every operation rounded once:
 *       X0 = (float)x0, Y0 = (float)y0, X1 = (float)(x0 + cw), Y1 = (float)(y0 + ch), CW = (float)cw
 *       ax1 = min(max(x1, X0), X1), ax2 = min(max(x2, X0), X1), ay1 / ay2 alike;  iw = ax2 - ax1, ih = ay2 - ay1
 *       keep = iw > 0 && ih > 0 && iw * ih >= min_visibility * ((x2 - x1) * (y2 - y1))
 *       lx1 = ax1 - X0, lx2 = ax2 - X0;  flip: (lx1, lx2) = (CW - lx2, CW - lx1);  ly1 = ay1 - Y0, ly2 = ay2 - Y0
 *       b = (lx1 * rw, ly1 * rh, lx2 * rw, ly2 * rh),  rw = (float)((double)out_w / cw), rh = (float)((double)out_h / ch)
 *       keep = keep && b.x2 - b.x1 >= min_size && b.y2 - b.y1 >= min_size
 *   The kept rows of image i are written to out_boxes [B, Gmax, 4] / out_labels int32 [B, Gmax] in their original order, out_count[i]
 *   (int32 [B]) is their number, and every row at or beyond it is zero.  gt_labels == NULL: out_labels, if given, is all zero.  Rows of
 *   the inputs at or beyond gt_count[i] are never read (they may hold NaN).  The pages' sizes are not known here: only cw, ch >= 1,
 *   x0, y0 >= 0 and flip are checked.  The outputs must not alias the inputs; boxes 16-byte aligned.  One launch per 48 images, one
 *   wave per image, no atomics, no synchronisation: capturable, and the output is a pure function of the input. */
int ldit_preprocess_win_f32(const void *const *images, const int32_t *heights, const int32_t *widths, const int32_t *windows, int32_t B,
                            int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream);
int ldit_preprocess_win_f16(const void *const *images, const int32_t *heights, const int32_t *widths, const int32_t *windows, int32_t B,
                            int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream);
int ldit_preprocess_win_u8(const void *const *images, const int32_t *heights, const int32_t *widths, const int32_t *windows,
                           int32_t interleaved, int32_t B, int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out,
                           ldit_stream stream);
int ldit_augment_targets_f32(const void *gt_boxes, const void *gt_labels, const void *gt_count, const int32_t *windows, int32_t B,
                             int32_t Gmax, int32_t out_h, int32_t out_w, float min_visibility, float min_size, void *out_boxes,
                             void *out_labels, void *out_count, ldit_stream stream);

/* ---- test-time augmentation: the views of a page merged on the device ---------------------------------------------
 * A VIEW is the batch at another size and / or mirrored left-right; its padded detections (boxes fp32 [B, D, 4], scores fp32 [B, D],
 * labels int32 [B, D], count int32 [B], as ldit_box_detections leaves them) are in the view's coordinates.  The merge is
 * ldit_tta_pool_f32 -> ldit_nms_batched_f32 (groups = the pooled labels) -> ldit_box_vote_f32: three launches, no synchronisation,
 * no atomics, capturable.  Both entries are additive (the ABI number did not move).
 *
 * ldit_tta_pool_f32: `boxes`, `scores`, `labels`, `count` are HOST arrays of V device pointers (the views by value: no stacked copy),
 *   `view_specs` a HOST array [V][3] = (W_v, H_v, flip_v), `page_sizes` a HOST array [B][2] = (ow_b, oh_b).  1 <= V <= 16,
 *   V * D <= 8192 (what the NMS takes per problem).  Pool entry v * D + d of image b, for d < count_v[b] (clamped to [0, D]), in fp32,
 *   every operation rounded once:
 *       (x1, x2) = flip_v ? ((float)W_v - x2, (float)W_v - x1) : (x1, x2)
 *       box = (x1 * rw, y1 * rh, x2 * rw, y2 * rh),  rw = (float)((double)ow_b / W_v), rh = (float)((double)oh_b / H_v)
 *   with the view's score and label beside it - an unmirrored view's boxes are those of resize_boxes bit for bit.  For
 *   d >= count_v[b] the entry is (zero box, score -inf, label 0) and the input row is never read (it may hold NaN).  Outputs:
 *   pool_boxes fp32 [B, V * D, 4] (16-byte aligned, like every view's boxes), pool_scores fp32 [B, V * D], pool_labels int32
 *   [B, V * D]; they must not alias the inputs.  One launch per 256 images (the descriptors travel in the kernel arguments).
 *
 * ldit_box_vote_f32: behind the NMS of the pool (N = V * D entries per image; keep int32 [B, D_out] = the kept pool indices, kept
 *   int32 [B] their number).  Row k < kept[b] with i = keep[b][k]: out_labels[b][k] = pool_labels[b][i], and out_boxes[b][k] is the
 *   score-weighted mean of the VOTING SET of i - every entry j of image b with pool_labels[j] == pool_labels[i], pool_scores[j] > -inf
 *   and inter / uni >= vote_thresh, the IoU formed in fp32 exactly as ldit_nms_batched_f32 forms it (area = (x2 - x1) * (y2 - y1),
 *   iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih alike, inter = iw * ih, uni = (area_a + area_b) - inter); i itself is always a
 *   member, even where its own IoU is NaN.  Per coordinate sum(s_j * b_j) / sum(s_j) with products, sums and the quotient in double
 *   and ONE rounding to fp32; the sum runs in a fixed order (per lane ascending j, then a fixed butterfly), so the result is a pure
 *   function of the input.  Rows k >= kept[b] (and rows whose index is no pool index) are zero in both outputs.  out_boxes == NULL:
 *   only the labels are gathered (the NMS's own boxes stand).  0 <= vote_thresh <= 1; boxes 16-byte aligned; one wave per row. */
int ldit_tta_pool_f32(const void *const *boxes, const void *const *scores, const void *const *labels, const void *const *count,
                      const int32_t *view_specs, const int32_t *page_sizes, int32_t V, int32_t B, int32_t D, void *pool_boxes,
                      void *pool_scores, void *pool_labels, ldit_stream stream);
int ldit_box_vote_f32(const void *pool_boxes, const void *pool_scores, const void *pool_labels, const void *keep, const void *kept,
                      int32_t B, int32_t N, int32_t D_out, float vote_thresh, void *out_boxes, void *out_labels, ldit_stream stream);

/* fp16 <-> fp32 conversion of a pixel batch / of the returned taps for an fp16 caller (round to nearest even), n elements;
 * the fp16 side 8-byte aligned, the fp32 side 16-byte aligned. */
int ldit_cast_f16_f32(const void *src, void *dst, int64_t n, ldit_stream stream);
int ldit_cast_f32_f16(const void *src, void *dst, int64_t n, ldit_stream stream);

/* ---- FPN on top of the taps (ref src/layoutdit/modeling/dit_backbone.py:65-90: torchvision FeaturePyramidNetwork([C]*4,
 * 256, extra_blocks=LastLevelMaxPool()); torchvision's source is not available offline -> parity unpinned, checked against a
 * torch restatement of its documented forward).  The 1x1 lateral convolutions run as ldit_linear_f32 on the TOKENS of each
 * tap (a 1x1 convolution commutes with the bilinear rescale of dit_backbone.py:55-59), then per level:
 *   ldit_fpn_merge_f32:    inner [B, Gh*s, Gw*s, Ch] (NHWC) = bilinear_s(lat tokens [B, 1+Gh*Gw, Ch]) + nearest(top), top NHWC
 *                          [B, top_h, top_w, Ch] or NULL (coarsest level);  s in {4, 2, 1, 0.5};  Ch % 4 == 0
 *   ldit_conv3x3_nhwc_f32: y [B, H, W, Cout] (NHWC) = conv3x3(x [B, H, W, Cin] NHWC, padding 1) + bias as an implicit-im2col
 *                          fp32 MFMA GEMM; w [Cout, 3, 3, Cin] (= torch weight.permute(0, 2, 3, 1)); Cin % 32 == 0;
 *                          zeros: >= 128 bytes of device zeros (the padding taps' DMA source).
 * LastLevelMaxPool (kernel 1, stride 2) is a strided view of the last output, no kernel. */
int ldit_fpn_merge_f32(const void *lat, const void *top, void *out, int64_t B, int64_t Gh, int64_t Gw, int64_t Ch, float scale,
                       int64_t top_h, int64_t top_w, ldit_stream stream);
int ldit_conv3x3_nhwc_f32(const void *x, const void *w, const void *bias, void *y, int64_t B, int64_t H, int64_t W, int64_t Cin,
                          int64_t Cout, const void *zeros, ldit_stream stream);
/* The same convolution on the bf16 matrix pipe (the eval-mode neck, neck_dtype="bf16"): the implicit-im2col mode of the bf16 MFMA
 * GEMM on a map that is ALREADY zero-padded.  xpad bf16 [B, H+2, W+2, Cin], exactly what ldit_pad_nhwc_f32_bf16 writes (no slack
 * rows: the highest address read is its last pixel); w bf16 [Cout, 3, 3, Cin]; bias fp32 [Cout] or NULL; y [B*H*W, Cout], row stride
 * ldy >= Cout elements: fp32 = acc + bias for LDIT_EPI_F32, bf16 for LDIT_EPI_BIAS and LDIT_EPI_BIAS_RELU (relu of LDIT_EPI_BIAS's y
 * bit for bit).  fp32 accumulation, k order (ky, kx, c) in 64-deep tiles: y equals, bit for bit, ldit_linear_bf16(_ex) with the
 * same epilogue on the materialised im2col matrix [B*H*W, 9 Cin] of xpad.  LDIT_EINVAL: null operand, xpad / w / y not 16-byte
 * aligned, empty problem, any other epilogue, ldy < Cout (every ldy >= Cout is taken: a stride the vector stores cannot take
 * goes element-wise).  LDIT_EUNSUPPORTED: Cin not a multiple of 64; padded map, output (B*H*W*ldy) or weight of 2^31 elements
 * or more (element offsets are 32 bits wide). */
int ldit_conv3x3_nhwc_bf16(const void *xpad, const void *w, const void *bias, void *y, int64_t ldy, int64_t B, int64_t H, int64_t W,
                           int64_t Cin, int64_t Cout, int32_t epilogue, ldit_stream stream);

/* ---- FPN backward (training through `self.fpn(feats)`, ref dit_backbone.py:87-90 under ref trainer.py:169-178).  The MFMA work
 * reuses entry points above and below (layoutdit_amd/modeling/dit_fpn.py sequences them): dgrad of a 3x3 convolution =
 * ldit_conv3x3_nhwc_f32 on the flipped / in-out-swapped weight; wgrad of a 3x3 convolution = nine ldit_linear_bf16_tr (wgrad
 * form) on zero-padded bf16 NHWC copies, one per tap (a tap is a constant row offset of the padded input); laterals =
 * ldit_linear_f32 / ldit_linear_bf16_tr.  New here:
 *   ldit_fpn_merge_bwd_f32:  adjoint of ldit_fpn_merge_f32.  d_inner [B, Gh*s, Gw*s, Ch] NHWC ->
 *                            d_lat [B, 1+Gh*Gw, Ch] (written; CLS row = 0; may be NULL) and d_top [B, top_h, top_w, Ch]
 *                            (ACCUMULATED into: it already holds the coarser level's own 3x3 dgrad; may be NULL).  Gather form.
 *   ldit_pad_nhwc_f32_bf16:  dst bf16 [B, H+2, W+2, C] = zero-padded copy of src fp32 [B, H, W, C] (every element written)
 *   ldit_colsum_f32:         out[n] = sum_m x[m * ldx + n] (bias gradients), two stages in a fixed order;
 *                            scratch: ldit_colsum_scratch_bytes(M, N) */
int ldit_fpn_merge_bwd_f32(const void *d_inner, void *d_lat, void *d_top, int64_t B, int64_t Gh, int64_t Gw, int64_t Ch, float scale,
                           int64_t top_h, int64_t top_w, ldit_stream stream);
int ldit_pad_nhwc_f32_bf16(const void *src, void *dst, int64_t B, int64_t H, int64_t W, int64_t C, ldit_stream stream);
size_t ldit_colsum_scratch_bytes(int64_t M, int64_t N);
int ldit_colsum_f32(const void *x, int64_t M, int64_t N, int64_t ldx, void *out, void *scratch, size_t scratch_bytes, ldit_stream stream);
/* out[n] = max_m |x[m * ldx + n]|: per-channel activation ranges for the fp8 build's calibration (the SmoothQuant-style fold of
 * DiTEncoder.calibrate_fp8: per-channel factors move LayerNorm-output outliers into the next GEMM's weight columns). Same scratch. */
int ldit_colamax_f32(const void *x, int64_t M, int64_t N, int64_t ldx, void *out, void *scratch, size_t scratch_bytes, ldit_stream stream);
/* What stands between two layers of the detector's backward under grad_dtype="bf16", in one pass over dy (and act): the ReLU's
 * backward, the bf16 copy that the dgrad and the wgrad GEMM both read, and the bias gradient.  With w = (act > 0 ? dy : 0) - a
 * SELECTION (torch's threshold_backward): a non-finite dy under a masked position gives 0, and act = +0, -0 or NaN masks -
 *   out    = bf16(w), ldit_cast_f32_bf16's conversion (to nearest even, non-finite kept)
 *   colsum = the column sums of w, bit for bit ldit_colsum_f32 on w (its device code: 512-row blocks, four accumulators per
 *            block, sequential second stage; no atomics)
 * act NULL: w = dy.  colsum NULL: no sums, scratch unused (may be NULL); else scratch: ldit_colsum_scratch_bytes(M, N) bytes.
 * Nothing is allocated; capturable; bit-reproducible.
 *   ldit_relu_bwd_bf16:          dy, act fp32 [M, N], out bf16 [M, N], row strides lddy, ldact, ldout >= N elements, any M, N >= 1
 *                                (four columns per thread where N, the strides and the addresses allow, else one).
 *   ldit_relu_bwd_pad_nhwc_bf16: dy, act fp32 [B, H, W, C], out bf16 [B, H+2, W+2, C] = the zero-padded map that
 *                                ldit_pad_nhwc_f32_bf16 writes for w (every element written, border included), colsum over
 *                                the M = B*H*W pixel rows; C % 4 == 0.
 * LDIT_EINVAL: null dy / out, colsum without scratch, empty problem, a stride below N, C % 4, misaligned operand (plain form:
 * the element size; padded form: 16 bytes, out 8).  LDIT_EWORKSPACE: scratch too small.  LDIT_EUNSUPPORTED: 2^31 rows or
 * columns or more, a padded map of 2^33 elements or more. */
int ldit_relu_bwd_bf16(const void *dy, int64_t lddy, const void *act, int64_t ldact, void *out, int64_t ldout, int64_t M, int64_t N,
                       void *colsum, void *scratch, size_t scratch_bytes, ldit_stream stream);
int ldit_relu_bwd_pad_nhwc_bf16(const void *dy, const void *act, void *out, int64_t B, int64_t H, int64_t W, int64_t C, void *colsum,
                                void *scratch, size_t scratch_bytes, ldit_stream stream);
/* The two with act as bf16 - the activation as a forward under train_dtype="bf16" of the detector saves it - so no fp32 copy of it is
 * made first.  A bf16 widens exactly: out and colsum are bit for bit those of the entry points above on the widened act.  Same
 * arguments, results and refusals; only act's element type (ldact counts bf16 elements) and alignment differ: 2 bytes in the plain
 * form (8 for its four-column path), 8 in the padded form. */
int ldit_relu_bwd_bf16_act16(const void *dy, int64_t lddy, const void *act, int64_t ldact, void *out, int64_t ldout, int64_t M, int64_t N,
                             void *colsum, void *scratch, size_t scratch_bytes, ldit_stream stream);
int ldit_relu_bwd_pad_nhwc_bf16_act16(const void *dy, const void *act, void *out, int64_t B, int64_t H, int64_t W, int64_t C, void *colsum,
                                      void *scratch, size_t scratch_bytes, ldit_stream stream);

/* ==== train step (BASELINE.json configs[2]: ViT-B/16 bs=64 bf16 forward + backward + AdamW) =============
 * Replaces, for the encoder, what the reference's loop runs through torch.autograd and torch.optim:
 *     loss_dict = self.model(images, targets) ; loss.backward() ; optimizer.step()     ref trainer.py:169-180
 *     optimizer = AdamW(params, lr = 1e-4, weight_decay = 0)                           ref trainer.py:62-68
 * bf16 build (cfg.dtype = LDIT_BF16; BASELINE asks bf16 where the reference uses fp16 autocast + GradScaler), and the mxfp8 build
 * (cfg.dtype = LDIT_MXFP8, hidden and mlp multiples of 128) as QUANTISATION-AWARE training:
 *   - the training forward IS the mxfp8 inference forward (same kernels, same tiles, same bits; extra outputs are side stores);
 *   - the backward is that forward's gradient with every MX quantiser Q taken as the identity (straight-through), computed on
 *     the bf16 backward kernels with the operands the forward multiplied: the wgrads read the dequantised activations Q(y1), Q(o),
 *     Q(y2), Q(g), the dgrads the dequantised weights Q(W).  EXACTNESS RULE: an e4m3 code has at most 4 significant bits and bf16
 *     has 8, so code 2^e is exact in bf16 for every block exponent -124 <= e <= 119 (every finite block with amax between ~2^-115
 *     and ~2^127); the dequantised operands are those values, held as bf16;
 *   - the q fold of the packed builds (W_q' = Q(qfold W_q), b_q' = qfold b_q, qfold = D^-1/2 log2 e - not a power of two, so it
 *     stays inside the quantiser): the attention backward runs in the folded convention and the W_q / b_q gradients are qfold
 *     times those of the folded tensors; the GELU derivative is that of the function the MX GELU epilogue computes;
 *   - parameter gradients and master weights stay fp32; no atomics.
 *
 * Parameters, gradients and the two AdamW moments are FLAT fp32 device blocks of ldit_flat_param_bytes(cfg) bytes, laid out
 * like the fp32 packed block: patch_w, patch_b, cls, pos, then per layer ln1_w, ln1_b, wqkv [3C,C] = [Wq;Wk;Wv],
 * bqkv [3C] = [bq;0;bv] (no key bias, TF:306: that third stays zero and receives a zero gradient), wo, bo, lam1, ln2_w,
 * ln2_b, w1, b1, w2, b2, lam2.  ldit_flat_param_layout writes the 4 + 14 L + 1 float offsets in that order (last = total).
 * The `pos` slot is the position table FOR THE INPUT GRID of cfg ([1 + P, C]); its gradient is with respect to that table (a caller
 * that resamples embeddings.position_embeddings bicubically chains the resample's own adjoint behind it, as layoutdit_amd.training does). */
size_t ldit_flat_param_bytes(const ldit_cfg *cfg);
int ldit_flat_param_layout(const ldit_cfg *cfg, int64_t *offsets, int32_t n);

/* bytes of: the activations kept between forward and backward / the backward's scratch */
size_t ldit_train_saved_bytes(const ldit_cfg *cfg, int32_t batch);
size_t ldit_train_workspace_bytes(const ldit_cfg *cfg, int32_t batch);

/* The bf16 MIRROR of the flat parameter block: element i = bf16(flat[i]), ldit_train_mirror_bytes(cfg) bytes.  It is the
 * `packed` argument of the two train-step entry points below: the forward reads a matrix K-contiguous at half its fp32
 * offset, the dgrad GEMMs read the SAME copy reduction-major through transposing LDS reads (no transposed copy exists),
 * the wgrad GEMMs need no weight; fp32 vectors are read from the flat block itself.  ldit_pack_train rebuilds it from
 * the flat block in one pass (after loading weights, or after a foreign optimizer changed them); ldit_adamw_step keeps it
 * current by itself when handed the mirror. */
size_t ldit_train_mirror_bytes(const ldit_cfg *cfg);
int ldit_pack_train(const ldit_cfg *cfg, const void *flat_params, void *mirror, size_t mirror_bytes, ldit_stream stream);
/* LDIT_MXFP8 mirror, ldit_train_mirror_bytes = A + packed_bytes(LDIT_MXFP8), A = flat_bytes / 2 rounded up to 256:
 *   [0, flat_bytes / 2)  the bf16 part as above, except that the four matrices of every layer hold their DEQUANTISED MX codes
 *                        (the q third of wqkv folded: Q(qfold W_q)) - the dgrads' operand at the same offsets;
 *   [A, ...)             the MX section, laid out as ldit_pack_weights' LDIT_MXFP8 block: codes and block scales of the four
 *                        matrices and the folded q|k|v bias [qfold bq; 0; bv], bit-identical to what ldit_pack_weights(LDIT_MXFP8)
 *                        makes from the same fp32 values (its other slots are unused).
 * ldit_pack_train builds both parts; ldit_adamw_step_mxfp8 keeps them current.
 * ldit_train_saved_bytes(LDIT_MXFP8) = the bf16 layout plus, per layer, M C bf16 (the dequantised attention output), and two
 * transient MX operands, M (C + C / 32) and M (F + F / 32) bytes (M = batch tokens, each region rounded up to 256 bytes). */

/* Training forward: as ldit_vit_forward, and keeps in `saved` what the backward needs (LayerNorm inputs and outputs, q|k|v,
 * the attention output and its log-sum-exp, the pre-LayerScale branch outputs, the MLP hidden after GELU and the GELU derivative at its pre-activation).
 * drop_scales: device fp32 [layers][2][batch] or NULL - stochastic depth (TF:360-378,432-434,440-442): the factor the
 * residual branch (0 = attention, 1 = MLP) of a layer is multiplied with for each sample, 0 or 1 / keep_prob; drawing
 * them is the caller's job.  ms / launches: as ldit_vit_forward_timed (both NULL = plain enqueue, capturable). */
int ldit_vit_forward_train(const ldit_cfg *cfg, const void *packed, const void *flat_params, const void *x, int32_t batch,
                           void *const *tap_out, const void *drop_scales, void *saved, size_t saved_bytes, ldit_stream stream,
                           double *ms, int64_t *launches);

/* Backward through stages stage_hi .. stage_lo (stage l >= 1 = encoder layer l, stage 0 = embeddings); a full backward is
 * (layers, 0).  Splitting it into consecutive descending ranges lets the caller start the gradient all-reduce of finished
 * layers while earlier ones are still being differentiated; the running gradient of the residual stream lives in
 * `workspace` between calls, so the ranges of one backward pass run in descending order on ONE workspace and every call gets the
 * same dtaps array (the gradient arriving at hidden state s < layers is summed in by the call that finishes stage s + 1, in the same
 * pass over the rows as that layer's LayerNorm backward).  dtaps[i] (device fp32 [batch, 1+P, C] or NULL) = gradient of the loss with
 * respect to hidden state cfg->taps[i].  grads: flat fp32 block, OVERWRITTEN (not accumulated) for every parameter of the stages processed.
 * drop_scales: the pointer given to the forward (NULL there = NULL here).  x: the forward's input (patch-embedding wgrad). */
int ldit_vit_backward(const ldit_cfg *cfg, const void *flat_params, const void *packed, const void *x, int32_t batch, void *const *dtaps,
                      const void *drop_scales, const void *saved, size_t saved_bytes, void *grads, size_t grads_bytes,
                      void *workspace, size_t workspace_bytes, int32_t stage_hi, int32_t stage_lo, ldit_stream stream,
                      double *ms, int64_t *launches);

/* Fused AdamW over n fp32 elements (torch.optim.AdamW semantics, decoupled weight decay), step counts from 1:
 *   g = grads * grad_scale ; p *= 1 - lr wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
 *   p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).   n % 4 == 0, all pointers 16-byte aligned.
 * bf16_mirror (optional, n bf16 elements): receives bf16(p) of the updated parameters in the same pass. */
int ldit_adamw_step(void *params, const void *grads, void *exp_avg, void *exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int32_t step, float grad_scale, void *bf16_mirror,
                    ldit_stream stream);

/* mxfp8 build: ldit_adamw_step's update of the whole flat block (same bits for master and moments), followed by one launch that
 * re-quantises the forward's operands of every layer (the launch of ldit_requant_train_mirror): afterwards `mirror` (ldit_train_mirror_bytes(cfg) bytes) equals ldit_pack_train of
 * the updated master bit for bit.  cfg->dtype == LDIT_MXFP8. */
int ldit_adamw_step_mxfp8(const ldit_cfg *cfg, void *params, const void *grads, void *exp_avg, void *exp_avg_sq, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int32_t step, float grad_scale, void *mirror, size_t mirror_bytes,
                          ldit_stream stream);

/* ---- the train variants of the mxfp8 forward's kernels, one entry point each (unit parity tests) ----
 * ldit_layernorm_mxfp8 that also writes Yd bf16 [rows, C] = the dequantised codes (8-byte aligned). */
int ldit_layernorm_mxfp8_train(const void *x, const void *gamma, const void *beta, void *Y, void *Ys, void *Yd, int64_t rows, int64_t C,
                               float eps, ldit_stream stream);
/* The bf16 attention with MX output O codes [rows, ldo] + Os [rows, ldo / 32] (ldo % 32 == 0), plus lse (fp32 [B, H, N], the
 * convention of ldit_attention_fwd_lse_bf16), Ob = bf16 O before quantisation and Od = bf16 dequantised codes (both [rows, ldo]).
 * scale == 0: Q pre-multiplied by D^-1/2 log2 e (the packed builds' fold) - lse is then log2 sum_k exp2(q'.k). */
int ldit_attention_mxfp8_train(const void *Q, const void *K, const void *V, void *O, void *Os, void *lse, void *Ob, void *Od, int64_t B,
                               int64_t N, int64_t H, int64_t D, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale,
                               ldit_stream stream);
/* ldit_linear_mxfp8 with the train step's side outputs (row stride ldy, bf16, 8-byte aligned); Y is bit-identical to ldit_linear_mxfp8's.
 * LDIT_EPI_SCALE_RESID: Ypre (optional) = the branch output before LayerScale, rowscale (optional, fp32 [M]) multiplies lam per row;
 * LDIT_EPI_BIAS_GELU: Ypre = gelu'(pre-activation), Yd = the dequantised MX output (both required). */
int ldit_linear_mxfp8_train(const void *X, int64_t lda, const void *Xs, const void *W, const void *Ws, const void *bias, void *Y,
                            int64_t ldy, void *Ys, int64_t M, int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R,
                            void *Y2, void *Ypre, const void *rowscale, void *Yd, ldit_stream stream);

/* ---- the kernels of the backward, one entry point each (unit parity tests) ---- */
/* ldit_attention_bf16 that also writes lse[b][h][q] = log2 sum_k exp2(scale log2(e) q.k)  (fp32 [B, H, N]) */
int ldit_attention_fwd_lse_bf16(const void *Q, const void *K, const void *V, void *O, void *lse, int64_t B, int64_t N, int64_t H,
                                int64_t D, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, ldit_stream stream);
/* dQ, dK, dV (bf16, row stride lddqkv) from Q, K, V (row stride ldqkv), O, dO and the forward's lse.  D == 64.  N <= 256: one
 * LDS-resident workgroup per (image, head); longer sequences: blocks of 256 rows, one launch per role (dK/dV, dQ). */
int ldit_attention_bwd_bf16(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *lse, void *dQ,
                            void *dK, void *dV, int64_t B, int64_t N, int64_t H, int64_t D, int64_t ldqkv, int64_t ldo, int64_t lddo,
                            int64_t lddqkv, float scale, ldit_stream stream);
/* LayerNorm backward: dh += d/dx ; dgamma = sum_rows dy xhat ; dbeta = sum_rows dy.  scratch: ldit_layernorm_bwd_scratch_bytes. */
size_t ldit_layernorm_bwd_scratch_bytes(int64_t rows, int64_t C);
int ldit_layernorm_bwd_f32(const void *dy, const void *x, const void *gamma, void *dh, int64_t rows, int64_t C, float eps,
                           void *dgamma, void *dbeta, void *scratch, size_t scratch_bytes, ldit_stream stream);
/* LayerNorm backward fused with the LayerScale / residual backward of the branch below it, as the train step launches it between the
 * MLP and the attention branch of a layer.  With dh' = dh + d/dx (the LayerNorm backward above, dh a += destination, in place):
 *   dz[r][c] = bf16(dh'[r][c] rs[r] lam[c]) ; dlam[c] = sum_r dh'[r][c] rs[r] z[r][c] ; dzbias[c] = sum_r dh'[r][c] rs[r] lam[c]
 * (dzbias sums the unrounded fp32 products, not the bf16 dz), rs = rowscale (fp32 [rows]) or 1 when rowscale is null.
 * dy, x, dh: fp32 [rows, C], gamma, lam: fp32 [C], 16-byte aligned; z (in), dz (out): bf16 [rows, C], 8-byte aligned; C % 4 == 0,
 * C <= 4096.  dgamma, dbeta, dlam, dzbias: fp32 [C], 16-byte aligned, overwritten (not +=).  scratch: 16-byte aligned,
 * ldit_layernorm_bwd_resid_scratch_bytes, contents irrelevant before and undefined after.  Additive to ABI 6. */
size_t ldit_layernorm_bwd_resid_scratch_bytes(int64_t rows, int64_t C);
int ldit_layernorm_bwd_resid_f32(const void *dy, const void *x, const void *gamma, const void *z, const void *lam, const void *rowscale,
                                 void *dh, void *dz, int64_t rows, int64_t C, float eps, void *dgamma, void *dbeta, void *dlam,
                                 void *dzbias, void *scratch, size_t scratch_bytes, ldit_stream stream);
/* LayerScale / residual backward on its own (the MLP branch's): h_out = h_in + rs lam (.) z  =>
 *   dz[r][c] = bf16(dh[r][c] rs[r] lam[c]) ; dlam[c] = sum_r dh[r][c] rs[r] z[r][c] ; dbias[c] = sum_r dh[r][c] rs[r] lam[c]
 * dh is only read (it passes unchanged to the residual branch).  dh: fp32 [rows, C], lam: fp32 [C], dz: bf16 [rows, C] out, all
 * 16-byte aligned; z: bf16 [rows, C], 8-byte aligned; rowscale: fp32 [rows] or null; C % 64 == 0.  dlam, dbias: fp32 [C], 16-byte
 * aligned, overwritten.  scratch: 16-byte aligned, ldit_resid_bwd_scratch_bytes.  Additive to ABI 6. */
size_t ldit_resid_bwd_scratch_bytes(int64_t rows, int64_t C);
int ldit_resid_bwd_bf16(const void *dh, const void *z, const void *lam, const void *rowscale, void *dz, int64_t rows, int64_t C,
                        void *dlam, void *dbias, void *scratch, size_t scratch_bytes, ldit_stream stream);
/* ldit_linear_bf16 with the train step's extras: Ypre (bf16 [M,N], stride ldy) receives X W^T + b before GELU / LayerScale;
 * (LDIT_EPI_BIAS_GELU: gelu'(X W^T + b) instead); rowscale (fp32 [M]) multiplies lam per row; aux (bf16 [M,N], stride
 * ldaux) is the factor LDIT_EPI_GELU_BWD multiplies the accumulator with (= that saved gelu');
 * splits > 1 (LDIT_EPI_F32 only): K is cut into `splits` ranges, range s writes its own fp32 slab Y + s M ldy, to be summed
 * with ldit_reduce_slabs_f32. */
int ldit_linear_bf16_ex(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M, int64_t N,
                        int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, void *Ypre, const void *rowscale,
                        const void *aux, int64_t ldaux, int32_t splits, ldit_stream stream);
int ldit_reduce_slabs_f32(const void *slabs, void *out, int64_t n, int32_t count, ldit_stream stream);
/* The backward's two GEMM forms on reduction-major operands (gemm_bf16_tr.hip; operands gathered by ds_read_b64_tr_b16):
 *   a_reduction_major = 0 (dgrad): Y[M,N] = epi( A[M,K] . W[K,N] ), A K-contiguous (K % 64 == 0), W row stride ldw;
 *                                  epilogues LDIT_EPI_F32, LDIT_EPI_BIAS (bf16 out), LDIT_EPI_GELU_BWD (x aux, stride N)
 *   a_reduction_major = 1 (wgrad): Y[M,N] = A[K,M]^T . W[K,N], any K (rows past K read zeros), fp32 out, optional split-K
 * zeros: >= 128 bytes of device zeros.  M, N, lda, ldw multiples of 8. */
int ldit_linear_bf16_tr(const void *A, int64_t lda, int32_t a_reduction_major, const void *W, int64_t ldw, void *Y, int64_t ldy,
                        int64_t M, int64_t N, int64_t K, int32_t epilogue, const void *aux, int32_t splits, const void *zeros,
                        ldit_stream stream);

/* ==== region proposals (torchvision RegionProposalNetwork in eval mode, which the reference runs inside FasterRCNN(...,
 * rpn_anchor_generator = AnchorGenerator(...)), ref src/layoutdit/modeling/model.py:40-55): per-level top-k on the objectness
 * logits, box decoding, clipping and the small-box filter, batched NMS, top-N per image - as three launches with fixed-size,
 * padded results: no device-to-host synchronisation, no data-dependent shape, capturable.  Inference only.  The batched NMS keyed
 * by class is also what the box head's postprocess_detections needs.  Additive to ABI 6.
 *
 * ldit_rpn_topk_f32: logits fp32 [B, Ntot], Ntot = sum of level_sizes (HOST int64[L], L <= 8, each 1 .. 16384; larger:
 *   LDIT_EUNSUPPORTED).  For every image and level l, columns [Koff_l, Koff_l + k_l) of idx_out (int32 [B, Ksum], k_l = min(k, N_l),
 *   Ksum = sum k_l) receive the positions on the concatenated axis of the level's k_l largest logits, in DESCENDING logit order, ties
 *   by ASCENDING index; -inf sorts last and NaN after -inf (a total order: the result is unique).  One workgroup per (level, image).
 * ldit_rpn_topk_chunked_f32: the arguments and the result of ldit_rpn_topk_f32 for levels of up to 2^20 = 1048576 anchors and
 *   k <= 8192 (larger: LDIT_EUNSUPPORTED).  A tournament in the same 16384-slot buffer: after a sort the level's best k_l keys so far
 *   sit in slots [0, k_l); the next 16384 - k_l anchors are written behind them (unused slots padded) and the buffer is sorted again
 *   until the level is exhausted.  The key is a total order that contains the level-local index, and the best k of a set under a
 *   total order do not depend on the chunking: the result is DEFINED as what one sort of the whole level would give, and a level
 *   that fits one chunk gets ldit_rpn_topk_f32's bits.  One workgroup per (level, image), a workgroup-uniform trip count; no
 *   workspace, no extra launch, no atomics, capturable, a pure function of its input.
 * ldit_rpn_decode_f32: for each idx[b, j] gathers anchors [Ntot, 4] (x1, y1, x2, y2), deltas [B, Ntot, 4] (dx, dy, dw, dh) and the
 *   logit, and decodes like BoxCoder(weights = (1, 1, 1, 1)):  w = x2 - x1, cx = x1 + w / 2;  dw, dh = min(., log(1000 / 16));
 *   pcx = dx w + cx, pw = exp(dw) w;  box = pc -+ p / 2 (y alike), clamped to [0, img_w] x [0, img_h];  score = sigmoid(logit).
 *   A candidate whose clamped width or height is not >= min_size, or whose score is not >= score_thresh, gets score -inf (its box is
 *   still written), and so does an index outside [0, Ntot) (box 0).  boxes_out fp32 [B, Ksum, 4], scores_out fp32 [B, Ksum].
 * ldit_nms_batched_f32: P independent problems, boxes fp32 [P, N, 4], scores fp32 [P, N], groups int32 [P, N] or NULL (one group);
 *   N <= 8192 (larger: LDIT_EUNSUPPORTED).  The semantics of torchvision batched_nms(boxes, scores, groups, iou_thr)[:max_out]:
 *     1. candidates whose score is -inf or NaN are dropped: never kept, never suppressing;
 *     2. the others are ordered by descending score, ties by ascending input index;
 *     3. greedily, a candidate is kept unless an ALREADY KEPT candidate of the SAME group has IoU > iou_thr with it;
 *     4. keep (int32 [P, max_out]) = the first max_out kept input indices in that order, padded with -1; count (int32 [P]) = how many
 *        (at most max_out); out_boxes [P, max_out, 4] / out_scores [P, max_out] (each optional) = the kept rows, padding rows zero.
 *   IoU in fp32, exactly:  area = (x2 - x1) * (y2 - y1);  iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih alike;  inter = iw * ih;
 *   iou = inter / ((areaA + areaB) - inter), no contraction, correctly rounded division;  suppressed iff iou > iou_thr.  Box
 *   coordinates are expected finite.  One workgroup per problem, no atomics: bit-reproducible.
 *   workspace: ldit_nms_workspace_bytes(P, N) bytes (currently 0: the kernel keeps its state in registers and LDS; NULL is then fine);
 *   a shorter buffer is refused with LDIT_EWORKSPACE. */
int ldit_rpn_topk_f32(const void *logits, const int64_t *level_sizes, int32_t L, int32_t B, int32_t k, void *idx_out, ldit_stream stream);
int ldit_rpn_topk_chunked_f32(const void *logits, const int64_t *level_sizes, int32_t L, int32_t B, int32_t k, void *idx_out,
                              ldit_stream stream);
int ldit_rpn_decode_f32(const void *logits, const void *deltas, const void *anchors, const void *idx, int32_t B, int64_t Ntot, int64_t Ksum,
                        float img_h, float img_w, float min_size, float score_thresh, void *boxes_out, void *scores_out,
                        ldit_stream stream);
size_t ldit_nms_workspace_bytes(int64_t P, int64_t N);
int ldit_nms_batched_f32(const void *boxes, const void *scores, const void *groups, int32_t P, int64_t N, float iou_thr, int32_t max_out,
                         void *keep, void *count, void *out_boxes, void *out_scores, void *workspace, size_t workspace_bytes,
                         ldit_stream stream);

/* ==== box head (torchvision RoIHeads in eval mode, which the reference runs inside FasterRCNN(..., box_roi_pool =
 * MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2)), ref src/layoutdit/modeling/model.py:34-55): the multi-scale RoIAlign in
 * front of the head's GEMMs and the softmax / decode / filter behind them, one launch each, on the padded proposals the region-proposal
 * stage returns: no device-to-host synchronisation (torchvision's MultiScaleRoIAlign runs one nonzero per level), no data-dependent
 * shape, no atomics, capturable, bit-reproducible.  ldit_nms_batched_f32 with the labels as groups finishes the stage.  Inference only.
 * Additive to ABI 6.
 *
 * ldit_roi_align_levels_f32: L <= 8 fp32 feature maps of C channels (C % 4 == 0) in channels-last memory, finest first.  Map l is
 *   described by HOST arrays of length L: maps[l] (device pointer, 16-byte aligned), map_h[l] x map_w[l] cells, spatial_scale[l] and
 *   the element strides stride_b / stride_y / stride_x [l] of batch, row and pixel (multiples of 4, stride_x >= C; the channel
 *   stride is 1) - so a strided view such as p5[:, :, ::2, ::2] is consumed in place.  Element (b, y, x, c) of map l is
 *   maps[l][b stride_b + y stride_y + x stride_x + c]; the caller guarantees that all of them exist.
 *   boxes fp32 [B, R, 4] (x1, y1, x2, y2 in image coordinates), count int32 [B] or NULL (all R rows valid).
 *   out fp32 [B R, P, P, C]; rows r >= count[b] are written as ZEROS.  levels_out (optional) int32 [B, R]: the level of each row,
 *   -1 for padding rows.  P = 7 with sampling_ratio = 2 is built; anything else: LDIT_EUNSUPPORTED, like C % 4 != 0 and L > 8.
 *   Level of a box (torchvision LevelMapper), in fp32:  area = (x2 - x1) * (y2 - y1);
 *     k = floor(canonical_level + log2(sqrt(area) / canonical_scale) + 1e-6), clamped to [k_min, k_max];  level = k - k_min
 *   (k_max - k_min < L; torchvision: canonical 224 / 4, k_min = -log2(spatial_scale[0]), k_max = -log2(spatial_scale[L - 1])).
 *   Pooling (torchvision roi_align, aligned = False), with s = the level's spatial_scale, in fp32:
 *     start_x = x1 s;  roi_w = max(x2 s - x1 s, 1);  bin_w = roi_w / P;  sample i of bin p at x = start_x + p bin_w + (i + 0.5) bin_w / 2
 *     (y alike).  A sample with y < -1 or y > map_h (x alike) contributes 0.  Otherwise y = max(y, 0), y_low = (int) y; if
 *     y_low >= map_h - 1 both rows are map_h - 1 and the weight is on y_low alone, else y_high = y_low + 1, ly = y - y_low, hy = 1 - ly;
 *     value = hy hx v(low, low) + hy lx v(low, high) + ly hx v(high, low) + ly lx v(high, high).  A bin is the sum of its 4 samples / 4.
 *   One workgroup per row, one wave per bin, four channels per lane.
 * ldit_roi_align_levels_bf16: the same arguments, refusals and arithmetic; out is bf16 [B R, P, P, C] - every element the fp32 entry's
 *   value rounded to bf16 (to nearest even, ldit_cast_f32_bf16's conversion) at the store, padding rows bf16 zeros; levels_out is
 *   unchanged.  The maps stay fp32.  The row is the A operand of ldit_linear_bf16 as it stands (P P C a multiple of 64 at C % 64 == 0)
 *   at half the bytes of the fp32 row.  Additive to ABI 6.
 * ldit_box_postprocess_f32: RoIHeads.postprocess_detections up to the NMS.  head fp32 [B R, ld]: the class logits in columns
 *   [0, NC), the deltas (dx, dy, dw, dh) of class c in columns [NC + 4 c, NC + 4 c + 4); ld >= 5 NC.  proposals fp32 [B, R, 4], count
 *   int32 [B] or NULL, weights HOST float[4] = the BoxCoder weights (10, 10, 5, 5).  One candidate per (proposal r, class c = 1 .. NC - 1)
 *   at index r (NC - 1) + (c - 1) - torchvision's flattening order, so the NMS's tie-break by ascending index is torchvision's:
 *   boxes_out fp32 [B, R (NC - 1), 4], scores_out fp32 [B, R (NC - 1)], labels_out int32 [B, R (NC - 1)] (= c).
 *   score = softmax over all NC logits (evaluated in double, rounded once).  box = ldit_rpn_decode_f32's arithmetic on
 *   (dx / wx, dy / wy, dw / ww, dh / wh) against the proposal (dw, dh clamped at log(1000 / 16) AFTER the division), clamped to
 *   [0, img_w] x [0, img_h].  The score becomes -inf (the box is still written) when it is not > score_thresh (STRICTLY: the RPN
 *   stage uses >=, torchvision's box head does not), when the clamped width or height is not >= min_size, or when r >= count[b]. */
int ldit_roi_align_levels_f32(const void *const *maps, const int32_t *map_h, const int32_t *map_w, const float *spatial_scale,
                              const int64_t *stride_b, const int64_t *stride_y, const int64_t *stride_x, int32_t L, int64_t C,
                              const void *boxes, const void *count, int32_t B, int64_t R, int32_t P, int32_t sampling_ratio, int32_t k_min,
                              int32_t k_max, float canonical_scale, float canonical_level, void *out, void *levels_out, ldit_stream stream);
int ldit_roi_align_levels_bf16(const void *const *maps, const int32_t *map_h, const int32_t *map_w, const float *spatial_scale,
                               const int64_t *stride_b, const int64_t *stride_y, const int64_t *stride_x, int32_t L, int64_t C,
                               const void *boxes, const void *count, int32_t B, int64_t R, int32_t P, int32_t sampling_ratio, int32_t k_min,
                               int32_t k_max, float canonical_scale, float canonical_level, void *out, void *levels_out, ldit_stream stream);
int ldit_box_postprocess_f32(const void *head, int64_t ld, const void *proposals, const void *count, int32_t B, int64_t R, int32_t NC,
                             float img_h, float img_w, const float *weights, float score_thresh, float min_size, void *boxes_out,
                             void *scores_out, void *labels_out, ldit_stream stream);

/* ==== RPN training (torchvision RegionProposalNetwork.assign_targets_to_anchors + compute_loss, which the reference reaches through
 * loss_dict = model(images, targets), ref training/trainer.py:164-183): Matcher(0.7, 0.3, allow_low_quality_matches = True),
 * BalancedPositiveNegativeSampler(256, 0.5), BoxCoder(1, 1, 1, 1).encode and the two losses, restated from their documented
 * behaviour (parity with torchvision itself unpinned, as for the region proposals).  Enqueue only: no allocation, no host
 * synchronisation, no data-dependent shape, no float atomics, capturable; every output is a pure function of the inputs.
 * Additive to ABI 6.
 *
 * ldit_rpn_targets_f32: anchors fp32 [N, 4] (x1, y1, x2, y2), gt_boxes fp32 [B, Gmax, 4], gt_count int32 [B] (clamped to
 *   [0, Gmax]), keys int32 [B, N]: the caller's random priorities, non-negative (only the low 31 bits are read).  N <= 16384,
 *   Gmax <= 512 (larger: LDIT_EUNSUPPORTED).  bg_thr > fg_thr (or a NaN), batch_size_per_image <= 0, positive_fraction outside
 *   (0, 1]: LDIT_EINVAL.  One workgroup per image.
 *   Matching.  iou(anchor, gt) in fp32 exactly as ldit_nms_batched_f32 computes it (no contraction, correctly rounded division);
 *     a quotient that is not > 0 counts as +0.  GT rows at or past gt_count[b] are never read.  GT boxes must have positive width
 *     and height (torchvision asserts it with a synchronisation; here it is the caller's contract), anchors too.
 *     1. An anchor's match is the GT of largest IoU, ties to the LOWEST GT index.
 *     2. best >= fg_thr: positive.  best < bg_thr: negative.  Otherwise ignored.
 *     3. Low-quality promotion, torchvision's literally: every anchor whose IoU with SOME GT g equals g's maximum over all anchors
 *        becomes positive with ITS OWN argmax match of rule 1 - not necessarily g.  (A GT that no anchor overlaps has maximum 0,
 *        which every anchor disjoint from it attains: torchvision promotes those too, and so does this.)
 *     4. An image with gt_count 0: every anchor negative, zero targets.
 *   matched int32 [B, N]: the GT index for a positive anchor, -1 for a negative one, -2 for an ignored one (so the label before
 *     sampling is matched >= 0 / == -1 / == -2).
 *   reg_targets fp32 [B, N, 4]: BoxCoder(1, 1, 1, 1).encode(matched GT, anchor) for every positive anchor (sampled or not), zero
 *     elsewhere:  w = x2 - x1, cx = x1 + w / 2;  (dx, dy, dw, dh) = ((gcx - acx) / aw, (gcy - acy) / ah, log(gw / aw), log(gh / ah)).
 *   Sampling.  quota = floor(batch_size_per_image * positive_fraction) (in double).  Of the positives the min(quota, #positives)
 *     smallest by (key, anchor index) are taken, of the negatives the min(batch_size_per_image - taken positives, #negatives)
 *     smallest.  With i.i.d. keys that is the distribution of torchvision's randperm sampler; with any keys it is unique.
 *   labels int32 [B, N]: 1 = sampled positive, 0 = sampled negative, -1 = not in the loss.  sampled int32 [B, 2]: positives and
 *     negatives taken.
 * ldit_rpn_targets_chunked_f32: the arguments and the four outputs of ldit_rpn_targets_f32 for N <= 2^20 = 1048576 anchors per image,
 *   batch_size_per_image <= 4096 and Gmax <= 512 (larger: LDIT_EUNSUPPORTED).  One workgroup per image; matching and regression
 *   targets stream over the anchors with the statements of ldit_rpn_targets_f32 (the IoU bits cannot differ) and labels are first
 *   written as -1 everywhere.  The sampler is a tournament in the 16384-slot sort buffer on the key (class, key & 0x7fffffff, anchor
 *   index in 20 bits) - the order of ldit_rpn_targets_f32: anchors enter 16384 - 2 batch_size_per_image at a time behind a carry;
 *   after each sort the carry kept is the first min(batch_size_per_image, positives in the buffer) positive and the first
 *   min(batch_size_per_image, negatives in the buffer) negative keys, compacted to the front; ignored anchors never enter.  After
 *   the last chunk, with P and Q the positives and negatives of the whole image, take_pos = min(quota, P) and
 *   take_neg = min(batch_size_per_image - take_pos, Q) of the carried keys get labels 1 and 0 (take_pos <= quota <=
 *   batch_size_per_image: the carry always suffices).  Where both entry points apply, all four outputs are bit-identical.
 * ldit_rpn_loss_f32: logits fp32 [B, N], deltas fp32 [B, N, 4], labels / reg_targets / sampled as above, beta >= 0.
 *   n = the sum of all 2 B entries of sampled, read on the device.  Over the anchors with label 0 or 1 (y = label):
 *     loss[0] = (1 / n) sum of max(x, 0) - x y + log1p(exp(-|x|))        (binary_cross_entropy_with_logits, mean)
 *     loss[1] = (1 / n) sum over label 1 and the 4 coordinates of smooth_l1(delta - target; beta)   (torchvision's normaliser)
 *   smooth_l1(d) = d^2 / (2 beta) when |d| < beta, else |d| - beta / 2.  n == 0: both losses 0.  No positive: loss[1] == 0 exactly.
 *   d_logits fp32 [B, N] = d loss[0] / d logits, d_deltas fp32 [B, N, 4] = d loss[1] / d deltas, written IN FULL: exactly zero where
 *   an anchor is not in the loss.  Sums run in a fixed order (per-block partials, then one workgroup in double).
 *   workspace: ldit_rpn_loss_workspace_bytes(B, N) bytes; a shorter buffer is refused with LDIT_EWORKSPACE. */
int ldit_rpn_targets_f32(const void *anchors, const void *gt_boxes, const void *gt_count, const void *keys, int32_t B, int64_t N,
                         int32_t Gmax, float fg_thr, float bg_thr, int32_t batch_size_per_image, float positive_fraction, void *labels,
                         void *matched, void *reg_targets, void *sampled, ldit_stream stream);
int ldit_rpn_targets_chunked_f32(const void *anchors, const void *gt_boxes, const void *gt_count, const void *keys, int32_t B, int64_t N,
                                 int32_t Gmax, float fg_thr, float bg_thr, int32_t batch_size_per_image, float positive_fraction,
                                 void *labels, void *matched, void *reg_targets, void *sampled, ldit_stream stream);
size_t ldit_rpn_loss_workspace_bytes(int64_t B, int64_t N);
int ldit_rpn_loss_f32(const void *logits, const void *deltas, const void *labels, const void *reg_targets, const void *sampled, int32_t B,
                      int64_t N, float beta, void *loss, void *d_logits, void *d_deltas, void *workspace, size_t workspace_bytes,
                      ldit_stream stream);

/* ==== box head training (torchvision RoIHeads.select_training_samples + fastrcnn_loss and the gradient of MultiScaleRoIAlign, the
 * other half of loss_dict = model(images, targets), ref training/trainer.py:164-183): add_gt_proposals, Matcher(0.5, 0.5,
 * allow_low_quality_matches = False), BalancedPositiveNegativeSampler(512, 0.25), BoxCoder(10, 10, 5, 5).encode, the two losses and
 * the transposed RoIAlign, restated from their documented behaviour (parity with torchvision itself unpinned, as for the RPN).
 * Enqueue only: no allocation, no host synchronisation, no data-dependent shape, no float atomics, capturable; every output is a
 * pure function of the inputs.  fp32 whatever the encoder build.  Additive to ABI 6.
 *
 * ldit_roi_targets_f32: proposals fp32 [B, R, 4] with count int32 [B] (clamped to [0, R]) - the RPN's padded train-mode output -,
 *   gt_boxes fp32 [B, Gmax, 4], gt_labels int32 [B, Gmax] (values in [1, NC)), gt_count int32 [B] (clamped to [0, Gmax]), keys int32
 *   [B, R + Gmax]: the caller's random priorities, non-negative (only the low 31 bits are read), weights HOST float[4] = the BoxCoder
 *   weights (10, 10, 5, 5).  Rows at or past count[b] / gt_count[b] are never read.  R + Gmax <= 4096 (larger: LDIT_EUNSUPPORTED).
 *   bg_thr > fg_thr (or a NaN), batch_size_per_image <= 0, positive_fraction outside (0, 1], a weight that is not > 0: LDIT_EINVAL.
 *   One workgroup per image.
 *   Candidates (add_gt_proposals).  Candidate r < R is proposal r (valid when r < count[b]), candidate R + g is GT box g (valid when
 *     g < gt_count[b]); key r resp. R + g of the image's row of keys belongs to it.
 *   Matching.  iou(candidate, gt) in fp32 exactly as ldit_nms_batched_f32 and ldit_rpn_targets_f32 compute it; a quotient that is not
 *     > 0 counts as +0.  A candidate's match is the GT of largest IoU, ties to the LOWEST GT index.  best >= fg_thr: positive, its
 *     class gt_labels[match].  best < bg_thr: background, class 0.  Otherwise (only when bg_thr < fg_thr) ignored: never sampled.
 *     No low-quality promotion.  An image with gt_count 0: every proposal background.  A GT box matches itself (IoU 1).
 *   Sampling.  The rule of ldit_rpn_targets_f32: quota = floor(batch_size_per_image * positive_fraction) (in double); of the positives
 *     the min(quota, #positives) smallest by (key, candidate index) are taken, of the background candidates the
 *     min(batch_size_per_image - taken positives, #background) smallest.
 *   Outputs, S = batch_size_per_image, all written IN FULL.  ROW ORDER: the sampled positives in ascending (key, index) order, then
 *     the sampled background rows in ascending (key, index) order, then padding.  torchvision orders the rows by candidate index;
 *     both losses are sums over the rows, so that order is NOT reproduced.
 *     rois fp32 [B, S, 4]: the candidate's box, bit for bit; padding rows zero.
 *     labels int32 [B, S]: the class of a positive row, 0 for a background row, -1 for a padding row.
 *     reg_targets fp32 [B, S, 4]: BoxCoder(wx, wy, ww, wh).encode(matched GT, candidate) for positive rows, zero elsewhere:
 *       w = x2 - x1, cx = x1 + w / 2;  (wx (gcx - cx) / w, wy (gcy - cy) / h, ww log(gw / w), wh log(gh / h)).
 *     matched int32 [B, S]: the GT index of a positive row, -1 elsewhere.  sampled int32 [B, 2]: positives and background rows taken.
 * ldit_roi_align_levels_bwd_f32: the gradient of ldit_roi_align_levels_f32 with respect to its maps.  d_out fp32 [B S, P, P, C] (the
 *   forward's output order), boxes fp32 [B, S, 4], count int32 [B] or NULL, levels int32 [B, S] AS THE FORWARD RETURNED THEM
 *   (levels_out; the level is not recomputed; a value outside [0, L) contributes nothing, like a row at or past count[b]).
 *   The L gradient maps are described like the forward's maps by HOST arrays of length L: d_maps[l] (device pointer, 16-byte
 *   aligned), map_h / map_w / spatial_scale [l] and the element strides stride_b / stride_y / stride_x [l] (multiples of 4,
 *   stride_x >= C, channel stride 1; the elements of one map must not overlap).  EVERY element (b, y, x, c) of every map is written
 *   EXACTLY ONCE, zeros included: the caller clears nothing.  A level the forward read through a strided view (`pool`) gets a
 *   gradient map of its own shape; adding it into the viewed map is the caller's business.  The forward's limits (C % 4 == 0,
 *   L <= 8, P = 7, sampling_ratio = 2).
 *   Semantics: the exact transpose of the forward - the same sample coordinates (the same fp32 expressions), the same < -1 / > n
 *   rejection, clamping to 0, last-cell rule and 1 / 4 mean:
 *     d_map[y, x, c] = (1 / 4) sum over the rows r of the level in ASCENDING r, ph = 0 .. 6, pw = 0 .. 6 (in that nesting) of
 *                      (Ay_r[ph] Ax_r[pw]) d_out[r, ph, pw, c],
 *     Ay_r[ph] = the sum over the bin's 2 samples (in sample order) of the weight the sample puts on row y (hy if y_low == y, plus ly
 *     if y_high == y), Ax alike - the forward's weights are products of one y and one x factor, so the sum over a bin's 4 samples
 *     separates.  Terms with a zero factor are skipped.  One accumulation chain per element, no atomics: bit-reproducible.
 *   A fixed grid over (image, level, 4 x 4 pixel tile); one workgroup scans the image's rows once per 256 channels.
 * ldit_box_loss_f32: torchvision fastrcnn_loss.  head_out fp32 [M, ld] in the layout of ldit_box_postprocess_f32 (logits in columns
 *   [0, NC), the deltas of class c in [NC + 4 c, NC + 4 c + 4), ld >= 5 NC), labels int32 [M], reg_targets fp32 [M, 4] and sampled
 *   int32 [B, 2] as ldit_roi_targets_f32 wrote them (M = B S), beta >= 0.  n = the sum of all 2 B entries of sampled, read on the device.
 *     loss[0] = (1 / n) sum over label >= 0 of logsumexp(logits) - logit[label]     (cross_entropy, mean; max-subtracted, in double)
 *     loss[1] = (1 / n) sum over label >= 1 and the 4 deltas OF THE ROW'S OWN CLASS of smooth_l1(delta - target; beta)
 *   n == 0: both losses 0.  No positive: loss[1] == 0 exactly.  A label >= NC is outside the contract: the row is left out.
 *   d_head fp32 [M, ld], written IN FULL, ONE buffer with the two gradients in their own column ranges: columns [0, NC) hold
 *   d loss[0] / d logits = (softmax - onehot) / n, columns [NC, 5 NC) hold d loss[1] / d deltas; the caller scales each range by its
 *   upstream scalar.  Padding columns, rows with label -1 and the deltas of every class but the row's own are
 *   exactly zero.  Sums run in a fixed order (per-block partials, then one workgroup in double).
 *   workspace: ldit_box_loss_workspace_bytes(M) bytes; a shorter buffer is refused with LDIT_EWORKSPACE. */
int ldit_roi_targets_f32(const void *proposals, const void *count, const void *gt_boxes, const void *gt_labels, const void *gt_count,
                         const void *keys, int32_t B, int64_t R, int32_t Gmax, float fg_thr, float bg_thr, int32_t batch_size_per_image,
                         float positive_fraction, const float *weights, void *rois, void *labels, void *reg_targets, void *matched,
                         void *sampled, ldit_stream stream);
int ldit_roi_align_levels_bwd_f32(const void *d_out, const void *boxes, const void *count, const void *levels, int32_t B, int64_t S,
                                  void *const *d_maps, const int32_t *map_h, const int32_t *map_w, const float *spatial_scale,
                                  const int64_t *stride_b, const int64_t *stride_y, const int64_t *stride_x, int32_t L, int64_t C, int32_t P,
                                  int32_t sampling_ratio, ldit_stream stream);
size_t ldit_box_loss_workspace_bytes(int64_t M);
int ldit_box_loss_f32(const void *head_out, int64_t ld, const void *labels, const void *reg_targets, const void *sampled, int32_t B, int64_t M,
                      int32_t NC, float beta, void *loss, void *d_head, void *workspace, size_t workspace_bytes, ldit_stream stream);

/* ---- the detector's optimizer step: one AdamW over MANY parameter tensors, every decision in device memory ----
 * The other half of the reference's iteration (ref training/trainer.py:164-183: scaler.scale(loss).backward(), scaler.step(optimizer),
 * scaler.update() with AdamW(model.parameters())) in three launches per 64 parameter tensors, with no
 * device-to-host synchronisation: the non-finite check, the skip decision, the step count, the bias corrections, the loss scale and
 * the learning rate live in one small device block.
 *
 * A SEGMENT is one parameter tensor: p, g, m (exp_avg), v (exp_avg_sq) fp32 device pointers of n elements each, unrelated
 * allocations of any length (n == 0 allowed: its pointers are not looked at) and any 4-byte alignment - 16-byte accesses are used
 * where all four pointers of a segment allow them, single elements elsewhere and for the last n % 4.  bf16_mirror (optional, n bf16
 * elements, 2-byte aligned; 8-byte for the 16-byte path) receives bf16(p) of the updated values in the same pass.  `segs` is a HOST array: the
 * segments travel in the kernel arguments, 64 per launch, so nothing is copied to the device and nothing is allocated (capturable). */
typedef struct ldit_opt_segment {
    void *p;
    const void *g;
    void *m;
    void *v;
    int64_t n;
    void *bf16_mirror;
} ldit_opt_segment;

/* The device state block (40 bytes, 4-byte aligned); the caller allocates and initialises it: all integers 0, scale = the initial
 * loss scale (1 = no loss scaling), lr = the learning rate; the other floats are written before they are read. */
typedef struct ldit_opt_state {
    int32_t found_inf;       /* ldit_grads_check_multi_f32 ORs 1 in; ldit_opt_advance consumes and clears it */
    int32_t skip;            /* this step's decision, read by ldit_adamw_multi_f32 */
    int32_t step;            /* optimizer steps taken (skipped ones not counted) */
    int32_t growth_tracker;  /* consecutive unskipped steps since the scale last changed */
    int32_t skipped_steps;
    float scale;             /* the loss scale of the NEXT backward */
    float inv_scale_used;    /* 1 / the scale the current gradients were made with */
    float lr;                /* written by the caller (a device-side store: no synchronisation) */
    float bc1;               /* 1 - beta1^step */
    float bc2_sqrt;          /* sqrt(1 - beta2^step) */
} ldit_opt_state;

/* state->found_inf |= 1 if any element of any segment's g is NaN or +-inf (only g and n of a segment are read).  One wave ballot per
 * workgroup and one integer atomic per offending workgroup; no float atomics. */
int ldit_grads_check_multi_f32(const ldit_opt_segment *segs, int32_t S, ldit_opt_state *state, ldit_stream stream);

/* One thread: torch.amp.GradScaler's step / update and the optimizer's step count.
 *   skip = found_inf ; inv_scale_used = 1 / scale ; found_inf = 0 ;
 *   not skipped: step += 1, bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step) (in double, rounded once), growth_tracker += 1 and,
 *                when it reaches growth_interval, scale *= growth_factor and growth_tracker = 0 ;
 *   skipped:     scale *= backoff_factor, growth_tracker = 0, skipped_steps += 1.
 * growth_factor >= 1, 0 < backoff_factor <= 1, growth_interval >= 1 (1, 1, any = a constant scale).  The betas are doubles here: the
 * bias corrections are those torch.optim.AdamW forms from its Python floats (1 - 0.9f^t is 2.4e-7 off 1 - 0.9^t at t = 1). */
int ldit_opt_advance(ldit_opt_state *state, double beta1, double beta2, float growth_factor, float backoff_factor, int32_t growth_interval,
                     ldit_stream stream);

/* state->skip set: nothing is written.  Otherwise ldit_adamw_step's arithmetic in its order of operations on every segment, with
 * g = grads * (grad_mul * inv_scale_used) and lr, bc1, bc2_sqrt read from the state block.  The betas are doubles: the kernel gets
 * float(beta) and float(1 - beta), each rounded once (1.0f - 0.999f is 4.7e-5 off 0.001); the step size is float(double(lr) /
 * double(bc1)) and the second moment adds (1 - beta2) * (g * g), the roundings of torch.optim.AdamW.  ceil(S' / 64) launches, S' the non-empty
 * segments. */
int ldit_adamw_multi_f32(const ldit_opt_segment *segs, int32_t S, const ldit_opt_state *state, double beta1, double beta2, float eps,
                         float weight_decay, float grad_mul, ldit_stream stream);

/* -- global-norm clipping and per-segment hyper-parameters (additive: the three entry points above are unchanged) --
 * torch.nn.utils.clip_grad_norm_ + AdamW with parameter groups, still without a synchronisation:
 *   ldit_grads_check_norm_multi_f32 -> ldit_opt_advance -> ldit_clip_finish -> ldit_adamw_groups_multi_f32.
 *
 * The clip block (16 bytes of device memory, 4-byte aligned); the caller allocates and initialises it: max_norm = the bound
 * (a device-side store changes it, no re-capture), the rest 0. */
typedef struct ldit_clip_state {
    float max_norm;          /* input: the bound on the global L2 norm of the UNSCALED gradients; +inf = never clip */
    float total_norm;        /* output of ldit_clip_finish: that norm, of this step's gradients (non-finite on a skipped step) */
    float clip_coef;         /* output: float(min(1, max_norm / (total_norm + 1e-6))), formed in double; not written on a skipped step */
    int32_t clipped_steps;   /* unskipped steps whose clip_coef was below 1 */
} ldit_clip_state;

/* Per-segment hyper-parameters of ldit_adamw_groups_multi_f32 (8 bytes), a HOST array parallel to `segs`. */
typedef struct ldit_opt_hyper {
    float lr_scale;          /* the segment's learning rate is state->lr * lr_scale (>= 0) */
    float weight_decay;      /* >= 0 */
} ldit_opt_hyper;

/* The number of partial sums ldit_grads_check_norm_multi_f32 writes for these segments: one per 1 024 elements of every segment,
 * rounded up per segment.  Host arithmetic; -1 (and a message) for a null array, a negative count or a negative length. */
int64_t ldit_grad_norm_partials(const ldit_opt_segment *segs, int32_t S);

/* ldit_grads_check_multi_f32 and the sum of squares in ONE pass over the gradients.  Blocks and paths are the check's; every
 * workgroup also writes the sum of g * g over its elements, accumulated in double (a finite fp32 square cannot overflow it), to
 * partials[k], k counting the workgroups of all launches in segment order.  The reduction order inside a workgroup is fixed (the
 * lanes of a wave by butterfly, the waves one after another): equal inputs give equal bits.  `partials` is 8-byte aligned device
 * memory of partials_len doubles; partials_len < ldit_grad_norm_partials(segs, S) is refused before any launch.  A NaN or an
 * infinity makes its partial non-finite.  No float atomics. */
int ldit_grads_check_norm_multi_f32(const ldit_opt_segment *segs, int32_t S, ldit_opt_state *state, double *partials, int64_t partials_len,
                                    ldit_stream stream);

/* One workgroup, AFTER ldit_opt_advance (it reads this step's skip and inv_scale_used): the n partials are summed in double in a
 * fixed order,  total_norm = float(sqrt(sum) * inv_scale_used)  and, unless the step is skipped,
 * clip_coef = float(min(1, max_norm / (total_norm + 1e-6))) - torch.nn.utils.clip_grad_norm_'s formula on the two floats, formed
 * in double and rounded once - and clipped_steps += 1 when clip_coef < 1.  On a skipped step (a NaN or an infinity made the norm
 * non-finite) only total_norm is written.  n == 0: a norm of 0. */
int ldit_clip_finish(const ldit_opt_state *state, ldit_clip_state *clip, const double *partials, int64_t n, ldit_stream stream);

/* ldit_adamw_multi_f32 with the learning rate state->lr * hyper[s].lr_scale and the weight decay hyper[s].weight_decay for segment
 * s, on g = grads * (clip->clip_coef * inv_scale_used), or grads * inv_scale_used when clip is NULL.  lr_scale == 1, equal
 * weight_decay and clip_coef == 1 give ldit_adamw_multi_f32(grad_mul = 1) bit for bit.  lr_scale == 0 moves m and v and leaves p as
 * it is (the decay factor is 1 - lr * weight_decay of the SCALED lr, so it is 1 as well).  48 segments per launch (their hyper-parameters
 * ride beside them in the kernel arguments). */
int ldit_adamw_groups_multi_f32(const ldit_opt_segment *segs, const ldit_opt_hyper *hyper, int32_t S, const ldit_opt_state *state,
                                const ldit_clip_state *clip, double beta1, double beta2, float eps, ldit_stream stream);

/* -- the quantisation-aware mxfp8 encoder under this step (additive): the MX operands of the train mirror, re-made in ONE launch --
 * cfg->dtype must be LDIT_MXFP8.  `flat_params` is the fp32 master in ldit_flat_param_layout, `mirror` the train mirror of
 * ldit_train_mirror_bytes(cfg).  For every layer, from the master, exactly what ldit_pack_train makes for the four matrices and the
 * fused bias: the e4m3 codes and E8M0 scales of wqkv (the q third folded), wo, w1, w2 in the MX section, their dequantised bf16 copies
 * at the matrices' offsets in the bf16 part, and [fold bq, 0, bv] in the MX section.  NOTHING else of the mirror is written: LayerNorm
 * vectors, biases, LayerScale, the embeddings and every padding byte keep what the AdamW kernels' bf16 mirror write (or the last pack)
 * left.  Run behind ldit_adamw_multi_f32 / ldit_adamw_groups_multi_f32 on a mirror that was current before the update, the mirror
 * equals a fresh ldit_pack_train of the updated master byte for byte.  `state` may be NULL; with state->skip set every workgroup
 * returns before its first store (the masters did not move, the mirror is current).  One launch whatever the layer count, no LDS, no
 * atomics, nothing allocated, capturable.  LDIT_EINVAL: null / misaligned pointers (16 bytes; the state block 4), a dtype that is not
 * LDIT_MXFP8; LDIT_EWORKSPACE: a mirror shorter than ldit_train_mirror_bytes; LDIT_EUNSUPPORTED: a geometry the train step lacks. */
int ldit_requant_train_mirror(const ldit_cfg *cfg, const void *flat_params, void *mirror, size_t mirror_bytes,
                              const ldit_opt_state *state, ldit_stream stream);

/* -- gradient accumulation and data-parallel ranks under this step (additive): the fold into one flat gradient bucket --
 * One segment: n fp32 elements of a gradient tensor g and of its slice acc of the bucket, unrelated allocations of any 4-byte
 * alignment (n == 0 allowed: its pointers are not looked at).  `segs` is a HOST array: the segments travel in the kernel arguments,
 * 127 per launch, so nothing is copied to the device and nothing is allocated (capturable).  A workgroup owns 1 024 consecutive
 * elements of one segment; 16-byte accesses where both pointers of a segment allow them, single elements elsewhere and for the last
 * n % 4. */
typedef struct ldit_acc_segment {
    void *acc;
    const void *g;
    int64_t n;
} ldit_acc_segment;

/* overwrite != 0: acc[i] = g[i] as a copy of the bits (-0.0, NaN payloads and infinities survive; acc is never read, so whatever it
 * held is legal).  overwrite == 0: acc[i] = acc[i] + g[i], one fp32 addition per element - no atomics and nothing reordered, so equal
 * inputs give equal bits.  acc and g of a segment must not overlap.  ceil(S' / 127) launches, S' the non-empty segments.
 * Refused before any launch, with a message: a null array with S > 0, a negative S or n, a null or misaligned pointer in a non-empty
 * segment (LDIT_EINVAL); a segment of more than 2^41 elements, whose grid would pass 2^31 - 1 blocks (LDIT_EUNSUPPORTED). */
int ldit_grads_accumulate_multi_f32(const ldit_acc_segment *segs, int32_t S, int32_t overwrite, ldit_stream stream);

/* -- an exponential moving average of the weights inside the update, and the exchange that evaluates on it (additive) --
 * ldit_adamw_groups_multi_f32 and, in the same launch, for every segment s with a shadow ema[s] (n fp32 elements, 4-byte aligned,
 * overlapping nothing else of the segment; NULL: the segment has none, and `ema` itself NULL: no segment has one)
 *     E = E + w * (P - E)          one fp32 multiply-add on the P the update just formed, still in registers,
 * stored beside p, m, v and the mirror.  w is formed in the kernel from the device block, in double, rounded to float once:
 *     d = ema_warmup ? min(ema_decay, (1 + step) / (10 + step)) : ema_decay ,   w = float(1 - d) ,
 * step = state->step after ldit_opt_advance: the steps TAKEN, this one included - a skipped step neither moves a shadow (state->skip
 * set: nothing at all is written) nor ages the warmup.  p, m, v and the mirror receive ldit_adamw_groups_multi_f32's bits: with
 * lr_scale == 1, one weight_decay and no clip block those of ldit_adamw_multi_f32(grad_mul = 1).  The shadow joins the alignment
 * test of the 16-byte path.  `ema` is a HOST array parallel to `segs`; the shadow pointers ride beside the segments and their
 * hyper-parameters in the kernel arguments, 52 segments per launch.  0 <= ema_decay < 1.  Refused before any launch like the call
 * above, and: ema_decay outside [0, 1), a misaligned shadow (LDIT_EINVAL). */
int ldit_adamw_ema_groups_multi_f32(const ldit_opt_segment *segs, const ldit_opt_hyper *hyper, void *const *ema, int32_t S,
                                    const ldit_opt_state *state, const ldit_clip_state *clip, double beta1, double beta2, float eps,
                                    double ema_decay, int32_t ema_warmup, ldit_stream stream);

/* One pair of the exchange: n fp32 elements at a and at b (4-byte aligned, disjoint; n == 0 allowed: its pointers are not looked at)
 * and an optional bf16 copy of a (n bf16 elements, 2-byte aligned; 8-byte for the 16-byte path). */
typedef struct ldit_swap_segment {
    void *a;
    void *b;
    int64_t n;
    void *bf16_mirror;
} ldit_swap_segment;

/* a[i] <-> b[i] for every element of every segment, moved as integers: -0.0, NaN payloads and infinities survive, and two calls
 * are the identity bit for bit.  Where a mirror is given it receives bf16(new a).  Every element is read and written by exactly one
 * thread: no atomics.  `segs` is a HOST array, 99 segments per launch in the kernel arguments; nothing is allocated (capturable).
 * Refused before any launch: a null array with S > 0, a negative S or n, a null or misaligned pointer in a non-empty segment, an odd
 * mirror address (LDIT_EINVAL); a segment of more than 2^41 elements (LDIT_EUNSUPPORTED). */
int ldit_swap_multi_f32(const ldit_swap_segment *segs, int32_t S, ldit_stream stream);

/* ---- COCO box evaluation: matching, accumulation ----
 * The arithmetic of the reference's Evaluator.score() (ref evaluation/evaluator.py:219-286, which hands a JSON file to a per-image,
 * per-category host loop) on padded device tensors: no host round trip, no allocation, no float atomics, capturable, every output a
 * pure function of the inputs.  Categories are 1 .. K.  All IoU, area, precision and recall arithmetic is double.
 *
 * ldit_coco_match: one workgroup per image.  boxes fp32 [B, D, 4] (xyxy), scores fp32 [B, D], labels int32 [B, D], count int32 [B];
 *   gt_boxes fp32 [B, G, 4], gt_labels int32 [B, G], gt_crowd uint8 [B, G] or NULL (none is a crowd), gt_area fp32 [B, G] or NULL (the
 *   box's own area (x2 - x1) (y2 - y1) in double), gt_count int32 [B].  Rows at or past a count are never read.  iou_thrs HOST double[10],
 *   area_rng HOST double[8] = (lo, hi) of the 4 area ranges: passed to the kernel by value, bit for bit.  D <= 128, G <= 128, K <= 64
 *   (larger: LDIT_EUNSUPPORTED).  The results of image b go to row image_offset + b of the caller's store of `capacity` rows of
 *   store_D >= D slots (capacity * store_D <= 2^24), every row written IN FULL:
 *     code uint8 [capacity, store_D, 4, 10]: per detection slot, area range and threshold 0 = unmatched (a false positive), 1 = matched
 *       to a non-ignored GT box (a true positive), 2 = ignored, 3 = absent: a slot at or past count[b] (or D), a label outside 1 .. K,
 *       a rank >= 100.
 *     rank int32 [capacity, store_D]: the detection's rank among those of its (image, category) by (score descending, slot ascending),
 *       -1 = absent.  scores_out fp32 / labels_out int32 [capacity, store_D]: copies (-0 stored as +0), zero where absent.
 *     npig int32 [capacity, K, 4]: the non-ignored GT boxes of (image, category, area range).
 *   Per (image, category k, area range a = [lo, hi]): the detections of k in rank order, the first 100; a GT box of k is IGNORED when
 *   it is a crowd or its area (gt_area) is < lo or > hi; the GT are scanned non-ignored first, each group by index.
 *   iou(d, g) on [x, y, w, h] with w = x2 - x1: iw = min(xd + wd, xg + wg) - max(xd, xg), ih alike; 0 if iw <= 0 or ih <= 0; else
 *   i = iw ih, u = crowd_g ? wd hd : wd hd + wg hg - i, iou = i / u.  Per threshold t, detections in rank order: best = min(t, 1 - 1e-10),
 *   m = none; scan the GT: skip one already matched at t unless it is a crowd; stop when m is a non-ignored GT and this one is ignored;
 *   skip if iou < best; else best = iou, m = g (an equal IoU replaces m).  m set: matched, code 2 if m is ignored else 1, m is taken.
 *   Unmatched: code 2 if the detection's own area is < lo or > hi, else 0.
 * ldit_coco_keys: keys int64 [n_images * store_D], one per stored slot: (category << 56) | (inverted ordered score bits << 24) |
 *   (image * store_D + rank); an absent slot gets INT64_MAX.  Ascending key order is (category, score descending, image ascending,
 *   rank ascending), a total order.  Sorting the keys (with the permutation) is the caller's business.
 * ldit_coco_accumulate: sorted_keys / sorted_index int64 [n_images * store_D]: the keys in ascending order and, for each, the index
 *   (image * store_D + slot) it came from.  rec_thrs HOST double[101] (ascending from 0), max_dets HOST int32[3] (each in [1, 100]), by
 *   value.  One workgroup per (category, area range, maxDet M, threshold t) over the category's run of the sorted detections with
 *   rank < M: npig = the sum of npig(image, k, a) over the n_images images; npig == 0: the cell is -1, detections or not.  Otherwise tp / fp =
 *   cumulative counts of codes 1 / 0 (integers), rc = tp / npig, pr = tp / (tp + fp + 2.220446049250313e-16), pr made non-increasing
 *   from the back; recall[t, k, a, M] = the last rc (0 with no detections); precision[t, r, k, a, M] = pr at the first index with
 *   rc >= rec_thrs[r], 0 if there is none.  precision fp64 [10, 101, K, 4, 3], recall fp64 [10, K, 4, 3], every element written.
 *   n_images == 0 is allowed (everything -1; the sorted arrays are not looked at). */
int ldit_coco_match(const void *boxes, const void *scores, const void *labels, const void *count, const void *gt_boxes,
                    const void *gt_labels, const void *gt_crowd, const void *gt_area, const void *gt_count, int32_t B, int32_t D, int32_t G,
                    int32_t K, const double *iou_thrs, const double *area_rng, void *code, void *rank, void *npig, void *scores_out,
                    void *labels_out, int64_t capacity, int32_t store_D, int64_t image_offset, ldit_stream stream);
int ldit_coco_keys(const void *rank, const void *scores, const void *labels, int64_t n_images, int32_t store_D, void *keys, ldit_stream stream);
int ldit_coco_accumulate(const void *sorted_keys, const void *sorted_index, const void *code, const void *rank, const void *npig,
                         int64_t n_images, int32_t store_D, int32_t K, const double *rec_thrs, const int32_t *max_dets, void *precision,
                         void *recall, ldit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* LDIT_H */
