// Host-side internals shared by api.hip (inference entry points) and api_train.hip (train step): geometry checks, the
// byte layout of the packed parameter block and of the inference workspace, per-launch HIP-event bracketing.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldit_common.h"

namespace ldit {

inline size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Geo {
    int C, L, H, F, D, p, in_ch, gh, gw, P, T, Kp;   // T tokens per image, Kp = in_ch*p*p
};

// bf16 planes per fp32 operand of the split-fp32 builds (0 = not a split build)
inline int split_planes_of(int dtype) { return dtype == LDIT_F32X3 ? 2 : dtype == LDIT_F32X6 ? 3 : 0; }

inline int geometry(const ldit_cfg *cfg, Geo &g)
{
    if (!cfg) return fail(LDIT_EINVAL, "cfg is null");
    if (cfg->dtype != LDIT_F32 && cfg->dtype != LDIT_BF16 && cfg->dtype != LDIT_FP8 && cfg->dtype != LDIT_MXFP8 && !split_planes_of(cfg->dtype))
        return fail(LDIT_EUNSUPPORTED, "dtype %d: only fp32 (0), bf16 (1), fp8 e4m3 (3), split fp32 (4, 5) and MX fp8 (6) are implemented",
                    cfg->dtype);
    g.C = cfg->hidden; g.L = cfg->layers; g.H = cfg->heads; g.F = cfg->mlp; g.p = cfg->patch; g.in_ch = cfg->in_ch;
    if (g.C <= 0 || g.L < 0 || g.H <= 0 || g.F <= 0 || g.p <= 0 || g.in_ch <= 0) return fail(LDIT_EINVAL, "cfg: non-positive dimension");
    if (g.C % g.H) return fail(LDIT_EINVAL, "cfg: hidden %d not divisible by heads %d", g.C, g.H);
    g.D = g.C / g.H;
    if (g.D != 64) return fail(LDIT_EUNSUPPORTED, "cfg: head_dim %d, only 64 is implemented", g.D);
    if (g.C % 32 || g.F % 32) return fail(LDIT_EUNSUPPORTED, "cfg: hidden and mlp must be multiples of 32");
    if ((cfg->dtype == LDIT_BF16 || split_planes_of(cfg->dtype)) && (g.C % 64 || g.F % 64))
        return fail(LDIT_EUNSUPPORTED, "cfg: bf16 needs hidden and mlp multiples of 64");
    if (cfg->dtype == LDIT_FP8 && (g.C % 128 || g.F % 128)) return fail(LDIT_EUNSUPPORTED, "cfg: fp8 needs hidden and mlp multiples of 128");
    if (cfg->dtype == LDIT_MXFP8 && (g.C % 128 || g.F % 128)) return fail(LDIT_EUNSUPPORTED, "cfg: mxfp8 needs hidden and mlp multiples of 128");
    if (cfg->img_h <= 0 || cfg->img_w <= 0 || cfg->img_h % g.p || cfg->img_w % g.p)
        return fail(LDIT_EINVAL, "cfg: image %dx%d is not a multiple of patch %d", cfg->img_h, cfg->img_w, g.p);
    g.gh = cfg->img_h / g.p; g.gw = cfg->img_w / g.p; g.P = g.gh * g.gw; g.T = g.P + 1;
    g.Kp = g.in_ch * g.p * g.p;
    if (g.Kp % 32 || g.p % 4) return fail(LDIT_EUNSUPPORTED, "cfg: in_ch*patch^2 must be a multiple of 32 and patch of 4");
    if (cfg->n_taps < 0 || cfg->n_taps > LDIT_MAX_TAPS) return fail(LDIT_EINVAL, "cfg: n_taps %d out of range", cfg->n_taps);
    for (int i = 0; i < cfg->n_taps; ++i)
        if (cfg->taps[i] < 0 || cfg->taps[i] > g.L) return fail(LDIT_EINVAL, "cfg: tap %d outside [0, %d]", cfg->taps[i], g.L);
    return LDIT_OK;
}

// Byte offsets into the packed parameter block; every offset is a multiple of 16 bytes.  In the bf16 build the four
// big matrices of a layer (fused q|k|v, o_proj, fc1, fc2) are stored as bf16, in the fp8 build as e4m3 codes; everything
// else stays fp32.  fp8 adds, per layer, one fp32 scale per output channel of each matrix (sw_*: measured and applied by
// ldit_pack_weights) and a block of 8 floats whose slots 0, 2, 4, 6 hold the activation scales a_ln1, a_attn, a_ln2,
// a_gelu (ldit_set_fp8_act_scales; the odd slots are spare).  The mxfp8 build stores the matrices as e4m3 codes too, and in
// sw_* the E8M0 block scales of each matrix ([rows, cols / 32] bytes); it has no activation scales.
struct PackedLayer { size_t ln1_w, ln1_b, wqkv, bqkv, wo, bo, lam1, ln2_w, ln2_b, w1, b1, w2, b2, lam2, scales, sw_qkv, sw_o, sw_1, sw_2; };
struct PackedMap {
    size_t patch_w, patch_b, cls, pos, total;
    size_t patch_w16;   // bf16 / fp8 builds: bf16 copy of the patch projection (the patch embedding runs on the bf16 GEMM there)
    std::vector<PackedLayer> layer;
};

inline PackedMap packed_map(const Geo &g, int dtype)
{
    PackedMap m;
    size_t o = 0;
    const size_t mat = dtype == LDIT_FP8 || dtype == LDIT_MXFP8 ? 1 : dtype == LDIT_BF16 ? 2 : split_planes_of(dtype) ? 2 * (size_t)split_planes_of(dtype) : 4;
    auto take = [&](size_t n, size_t elt) { size_t at = o; o += up(n * elt, 16); return at; };
    m.patch_w = take((size_t)g.C * g.Kp, 4);
    m.patch_b = take(g.C, 4);
    m.cls = take(g.C, 4);
    m.pos = take((size_t)g.T * g.C, 4);
    // bf16 copy of the patch projection (bf16 / fp8 builds) or its bf16 planes (split-fp32 builds): the patch embedding runs on the bf16 GEMM there
    m.patch_w16 = dtype != LDIT_F32 ? take((size_t)g.C * g.Kp, 2 * (size_t)(split_planes_of(dtype) ? split_planes_of(dtype) : 1)) : 0;
    m.layer.resize(g.L);
    for (int l = 0; l < g.L; ++l) {
        PackedLayer &pl = m.layer[l];
        pl.ln1_w = take(g.C, 4); pl.ln1_b = take(g.C, 4);
        pl.wqkv = take((size_t)3 * g.C * g.C, mat); pl.bqkv = take((size_t)3 * g.C, 4);
        pl.wo = take((size_t)g.C * g.C, mat); pl.bo = take(g.C, 4); pl.lam1 = take(g.C, 4);
        pl.ln2_w = take(g.C, 4); pl.ln2_b = take(g.C, 4);
        pl.w1 = take((size_t)g.F * g.C, mat); pl.b1 = take(g.F, 4);
        pl.w2 = take((size_t)g.C * g.F, mat); pl.b2 = take(g.C, 4); pl.lam2 = take(g.C, 4);
        pl.scales = dtype == LDIT_FP8 ? take(8, 4) : 0;
        pl.sw_qkv = dtype == LDIT_FP8 ? take((size_t)3 * g.C, 4) : 0;
        pl.sw_o = dtype == LDIT_FP8 ? take(g.C, 4) : 0;
        pl.sw_1 = dtype == LDIT_FP8 ? take(g.F, 4) : 0;
        pl.sw_2 = dtype == LDIT_FP8 ? take(g.C, 4) : 0;
        if (dtype == LDIT_MXFP8) {
            pl.sw_qkv = take((size_t)3 * g.C * (g.C / 32), 1);
            pl.sw_o = take((size_t)g.C * (g.C / 32), 1);
            pl.sw_1 = take((size_t)g.F * (g.C / 32), 1);
            pl.sw_2 = take((size_t)g.C * (g.F / 32), 1);
        }
    }
    m.total = o;
    return m;
}

struct Workspace { size_t h, y, big, total; };   // byte offsets

inline Workspace workspace_map(const Geo &g, int batch, int dtype)
{
    const size_t M = (size_t)batch * g.T;
    const size_t wide = (size_t)(3 * g.C > g.F ? 3 * g.C : g.F);
    // fp8 / mxfp8 builds: sized for their bf16 q|k|v; the fp8 buffers need less (mxfp8: codes [M, K] followed by their block
    // scales [M, K / 32] - 33/32 bytes per element)
    const size_t act = dtype == LDIT_F32 ? 4 : 2;
    Workspace w;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += up(bytes, 256); return at; };
    w.h = take(M * g.C * 4);       // residual stream (always fp32)
    if (const size_t S = (size_t)split_planes_of(dtype)) {
        // split-fp32 builds: y = the S bf16 planes of the LayerNorm / attention output; big = the S bf16 planes of q|k|v
        // ([M, S * 3C], written by EPI_BIAS_SPLIT), later the S planes of the MLP hidden - each sized on its own: nothing
        // requires F >= 3C
        w.y = take(M * g.C * 2 * S);
        const size_t qkv = M * 3 * g.C * 2 * S, hid = M * g.F * 2 * S, patches = (size_t)batch * g.P * g.Kp * 2 * S;
        w.big = take(std::max(std::max(qkv, hid), patches));
        w.total = o;
        return w;
    }
    w.y = take(M * g.C * act);     // LayerNorm output, then attention output
    size_t big = M * wide * act;   // fused q|k|v, later the MLP hidden (never live together)
    if (dtype != LDIT_F32 && big < (size_t)batch * g.P * g.Kp * 2) big = (size_t)batch * g.P * g.Kp * 2;   // before layer 0: bf16 im2col of the batch
    // fp32 build fed by an image list (ldit_vit_forward_images): the transformed fp32 batch lives here until the embedding has read it
    // (only geometries narrower than 768 columns per token need the extra room)
    if (dtype == LDIT_F32 && big < (size_t)batch * g.P * g.Kp * 4) big = (size_t)batch * g.P * g.Kp * 4;
    w.big = take(big);
    w.total = o;
    return w;
}

// Optional per-launch HIP-event bracketing (ldit_vit_forward_timed).
struct Probe {
    bool on = false;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;
    std::vector<int> fam;
    int begin(int family)
    {
        if (!on) return LDIT_OK;
        hipEvent_t a, b;
        LDIT_HIP_CHECK(hipEventCreate(&a));
        LDIT_HIP_CHECK(hipEventCreate(&b));
        ev.push_back(a); ev.push_back(b); fam.push_back(family);
        LDIT_HIP_CHECK(hipEventRecord(a, stream));
        return LDIT_OK;
    }
    int end()
    {
        if (!on) return LDIT_OK;
        LDIT_HIP_CHECK(hipEventRecord(ev.back(), stream));
        return LDIT_OK;
    }
    int collect(double *ms, int64_t *launches)
    {
        if (!on) return LDIT_OK;
        LDIT_HIP_CHECK(hipStreamSynchronize(stream));
        for (size_t i = 0; i < fam.size(); ++i) {
            float t = 0.f;
            LDIT_HIP_CHECK(hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]));
            ms[fam[i]] += (double)t;
            launches[fam[i]] += 1;
        }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear(); fam.clear();
        return LDIT_OK;
    }
};

#define LDIT_TRY(expr)                 \
    do {                               \
        int rc__ = (expr);             \
        if (rc__ != LDIT_OK) return rc__; \
    } while (0)

#define LDIT_RUN(probe, family, expr)  \
    do {                               \
        LDIT_TRY((probe).begin(family)); \
        LDIT_TRY(expr);                \
        LDIT_TRY((probe).end());       \
    } while (0)

// q fold of the packed builds (ldit_pack_weights; the mxfp8 train mirror): q' = (D^-1/2 log2 e) q - exp2-domain scores (attention_flash.hip, PRE)
inline float qfold_of(const Geo &g) { return (1.0f / sqrtf((float)g.D)) * 1.44269504088896340736f; }

// split-fp32 builds: the plane products of one output element, SMALLEST FIRST (their sum is formed at its own magnitude
// before the leading p0.q0 term arrives): bf16x3 = a1 w0 + a0 w1 + a0 w0; six products = a2 w0 + a1 w1 + a0 w2 + a1 w0 + a0 w1 + a0 w0.
// Walked per 64-deep k-tile (k-tile outermost): the operand tiles one product has just pulled through L2 serve the next one - 1-5 % on
// the q|k|v and fc1 GEMMs against whole-K segments (profiles/r03_planes_segment_order.txt), never slower.  planes < 2: an ordinary GEMM.
inline GemmExtra split_segments(int planes)
{
    GemmExtra x{};
    if (planes == 2) { x.nseg = 3; x.seg_a = 0x001u; x.seg_w = 0x010u; }
    if (planes == 3) { x.nseg = 6; x.seg_a = 0x001012u; x.seg_w = 0x010210u; }
    x.seg_inner = x.nseg != 0;
    return x;
}

// the pixels as the detector holds them before its input transform: a ragged list of [in_ch, h_i, w_i] images in [0, 1]
// (ldit_vit_forward_images: the transform is evaluated by the kernel that produces the patch-embedding operand)
struct ImgSrc {
    const void *const *images;
    const int32_t *heights, *widths;
    ImgFmt fmt;
    float mean, std;
};

// the first destination that asked for hidden state `hidden_idx` (the fc2 epilogue writes it), or null
inline float *tap_of(const ldit_cfg *cfg, void *const *taps, int hidden_idx)
{
    for (int i = 0; taps && i < cfg->n_taps; ++i)
        if (cfg->taps[i] == hidden_idx && taps[i]) return static_cast<float *>(taps[i]);
    return nullptr;
}

// hidden state `hidden_idx` to every destination that asked for it, except the one already written
// (a lane of the two-lane forward copies its own rows: `bytes` from byte `offset` of the source and of every destination)
inline int copy_taps(const ldit_cfg *cfg, void *const *taps, int hidden_idx, const float *src, const float *already, size_t bytes, hipStream_t stream,
                     size_t offset = 0)
{
    for (int i = 0; i < cfg->n_taps; ++i)
        if (cfg->taps[i] == hidden_idx && taps[i] != already)
            LDIT_HIP_CHECK(hipMemcpyAsync(static_cast<char *>(taps[i]) + offset, reinterpret_cast<const char *>(src) + offset, bytes,
                                          hipMemcpyDeviceToDevice, stream));
    return LDIT_OK;
}

// shared preamble of forward() and forward_train(): `ptrs` are the blocks named in `names` (an image list stands in for x)
inline int check_forward_args(const ldit_cfg *cfg, const Geo &g, int batch, std::initializer_list<const void *> ptrs, const char *names,
                              const ImgSrc *imgs, void *const *tap_out)
{
    if (batch <= 0) return fail(LDIT_EINVAL, "batch %d must be positive", batch);
    for (const void *p : ptrs)
        if (!p) return fail(LDIT_EINVAL, "null %s pointer", names);
    for (const void *p : ptrs)
        if (!aligned16(p)) return fail(LDIT_EINVAL, "pointers must be 16-byte aligned");
    if (imgs && (!imgs->images || !imgs->heights || !imgs->widths || !(imgs->std > 0.0f) || batch > 65535))
        return fail(LDIT_EINVAL, "image list: null array, non-positive std or more than 65535 images");
    if (cfg->n_taps && !tap_out) return fail(LDIT_EINVAL, "tap_out is null");
    for (int i = 0; i < cfg->n_taps; ++i)
        if (!tap_out[i] || !aligned16(tap_out[i])) return fail(LDIT_EINVAL, "tap_out[%d] is null or misaligned", i);
    if ((int64_t)batch * g.T * (int64_t)(g.F > 3 * g.C ? g.F : 3 * g.C) >= (1ll << 31))
        return fail(LDIT_EUNSUPPORTED, "batch %d: activation index space exceeds 2^31 elements, split the batch", batch);
    return LDIT_OK;
}

// shared preamble of the ldit_linear_* entries.  planes > 1 (ldit_linear_planes): operand rows hold that many bf16 planes and the entry
// checks its output stride itself.  Entries that map their epilogue themselves leave `epilogue` out.
inline int check_linear(const char *name, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldy, const void *Y, const void *Y2,
                        int epilogue = LDIT_EPI_BIAS, int64_t planes = 1)
{
    if (M <= 0 || N <= 0 || K <= 0) return fail(LDIT_EINVAL, "%s: empty problem", name);
    if (M * (ldy > lda ? ldy : lda) >= (1ll << 31) || N * K * planes >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "%s: operand exceeds 2^31 elements", name);
    if ((planes == 1 && ldy < N) || lda < planes * K) return fail(LDIT_EINVAL, "%s: bad leading dimension", name);
    if (!Y || !aligned16(Y) || (Y2 && !aligned16(Y2))) return fail(LDIT_EINVAL, "%s: output null or misaligned", name);
    if (epilogue < LDIT_EPI_BIAS || epilogue > LDIT_EPI_SCALE_RESID) return fail(LDIT_EINVAL, "%s: unknown epilogue %d", name, epilogue);
    return LDIT_OK;
}

// ---- the encoder layer, written once (api.hip: run_layer) for every build and for inference and training ------------------------
struct Build { int dtype; bool train; };     // train: the kernels that also store what the backward reads

// An activation operand in the build's format: fp32 or bf16 values, the bf16 planes of the split builds side by side, or e4m3 codes
struct Operand {
    void *p = nullptr;
    void *s = nullptr;     // mxfp8: its E8M0 block scales [rows, ld / 32]; fp8: its calibrated fp32 scale (device, read only); else null
    int ld = 0;            // row stride in elements, every plane counted
    int planes = 0;        // split builds: bf16 planes per value
};
inline Operand operand(const void *p, const void *s, int64_t ld, int planes = 0) { return {const_cast<void *>(p), const_cast<void *>(s), (int)ld, planes}; }

// side stores of one training GEMM: Ypre = the branch output before LayerScale (EPI_SCALE_RESID) or gelu' (EPI_BIAS_GELU), rowscale = the
// stochastic-depth row factors on lam, Yd (mxfp8) = the dequantised MX output
struct Side { void *Ypre = nullptr; const float *rowscale = nullptr; void *Yd = nullptr; };

// One layer as the schedule sees it.  Inference: h_in = h_mid = h_out and one buffer serves y1, o and y2 in turn, another q|k|v and
// then the MLP hidden; training: every tensor in its own slot of the saved block.
struct Layer {
    const float *h_in; float *h_mid, *h_out;   // residual stream before the layer, after the attention branch, after the MLP branch
    Operand y1, qkv, o, y2, hid;       // LN1 output, q|k|v, attention output, LN2 output, MLP hidden
    size_t qk_bytes;                   // from a row's q to its k, and from its k to its v
    float scale;                       // score scale; 0: q was folded when the weights were packed
    // parameters: fp32 vectors at V + v->*; matrices in the build's format at W + w->* / div (div = 2: the bf16 mirror of the flat fp32
    // block) and their scales at W + w->sw_* (fp8: fp32 per row, mxfp8: E8M0 blocks); bqkv apart (mxfp8 training reads the folded copy)
    const char *V, *W; const PackedLayer *v, *w; size_t div; const float *bqkv;
    const float *vec(size_t off) const { return reinterpret_cast<const float *>(V + off); }
    const void *mat(size_t off) const { return W + off / div; }
    float *tap;                        // second copy of h_out, or null
    // training only
    Side s_o, s_fc1, s_fc2;            // z1 + rs1; a1 (+ g dequantised, mxfp8); z2 + rs2
    float *lse; void *y1d, *y2d, *ob, *od;   // mxfp8: dequantised y1, y2; the bf16 attention output before quantisation, its dequantised codes
};

// the three places that choose a kernel by build (api.hip); everything else sees operands
int layernorm(Build b, const float *X, const float *gamma, const float *beta, const Operand &Y, void *Yd, int64_t rows, int C, float eps, hipStream_t stream);
int linear(Build b, const Operand &A, const void *W, const void *Ws, const float *bias, const Operand &Y, int M, int N, int K, int epi, const float *lam,
           const float *R, float *Y2, const Side &t, hipStream_t stream, float ab_scale = 0.f, float out_inv_scale = 0.f);
int attention(Build b, const void *Q, const void *K, const void *V, int ldq, int ldk, int ldv, const Operand &O, int B, int N, int H, int D, float scale,
              hipStream_t stream, float *lse = nullptr, void *Ob = nullptr, void *Od = nullptr, int plane_in = 0);
int run_layer(Build b, const Geo &g, int batch, float eps, const Layer &d, hipStream_t stream, Probe &probe);
constexpr int LAYER_LAUNCHES = 7;
// launch `i` (0 .. LAYER_LAUNCHES - 1) of run_layer alone: the two-lane forward alternates its lanes launch by launch
int layer_launch(int i, Build b, const Geo &g, int batch, float eps, const Layer &d, hipStream_t stream, Probe &probe);
// Lanes of the inference forward: 2 = the fp32 forward runs images [0, (batch + 1) / 2) and the rest as two lanes on two streams
// that share the chip (api.hip: forward), 1 = one stream.  Host arithmetic; honours LDIT_FWD_LANES.
int forward_lanes(int dtype, const Geo &g, int batch);
// patch embedding + CLS rows into `out`: on the fp32 GEMM straight from the NCHW batch, or on the bf16 GEMM from an im2col pass
int embed(const Geo &g, const float *x, const float *pw, const float *pb, const float *cls, const float *pos, float *out, int batch, int img_h, int img_w, hipStream_t stream, Probe &probe);
int embed_bf16(const Geo &g, const float *x, const ImgSrc *imgs, int planes, void *patches, const void *w16, const float *pb, const float *cls,
               const float *pos, float *out, int batch, int img_h, int img_w, hipStream_t stream, Probe &probe);

}  // namespace ldit
