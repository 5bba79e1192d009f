// C-ABI entry points of libldit_hip.so (declared in include/ldit.h).  Host-side sequencing only: every byte of
// arithmetic happens in the HIP kernels of this directory; there is no CPU fallback.
#include "api_internal.h"

#include <mutex>

namespace ldit {

char *err_buf()
{
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int ensure_dynamic_lds(const void *kern, int bytes, std::atomic<unsigned long long> &done)
{
    int dev = 0;
    LDIT_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (bit && (done.load(std::memory_order_relaxed) & bit)) return LDIT_OK;
    LDIT_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (bit) done.fetch_or(bit, std::memory_order_relaxed);
    return LDIT_OK;
}

int compute_units()
{
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    const bool slot = dev >= 0 && dev < 64;
    if (slot) {
        const int c = cached[dev].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    if (slot) cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

namespace {
DiagSwitches read_switches()
{
    DiagSwitches d;
    auto digit = [](const char *name, int lo, int hi) {
        const char *e = getenv(name);
        return (e && e[0] >= '0' + lo && e[0] <= '0' + hi && e[1] == 0) ? e[0] - '0' : -1;
    };
    auto is = [](const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; };
    d.gemm_tile = digit("LDIT_GEMM_TILE", 0, 7);
    if (const char *e = getenv("LDIT_GEMM_THIN_TILES")) d.thin_tiles = atol(e);
    d.panel_persist = is("LDIT_GEMM_PERSIST", '1');
    d.bf16_tile = digit("LDIT_GEMM_BF16_TILE", 2, 7);
    d.bf16_tile_env = getenv("LDIT_GEMM_BF16_TILE") != nullptr;
    d.bf16_tr_tile = digit("LDIT_GEMM_BF16_TR_TILE", 0, 9);
    d.bf16_tail_launch = is("LDIT_GEMM_BF16_TAIL_LAUNCH", '1');
    d.fp8_tile = digit("LDIT_GEMM_FP8_TILE", 0, 6);
    d.direct_epi = is("LDIT_GEMM_DIRECT_EPILOGUE", '1');
    d.seg_order = digit("LDIT_GEMM_SEG_ORDER", 0, 1);
    if (const char *e = getenv("LDIT_PLANES_TAIL_WAVES")) d.planes_tail_waves = atol(e);
    d.attn_bf16_nw = digit("LDIT_ATTN_BF16_NW", 4, 8);
    d.fwd_lanes = digit("LDIT_FWD_LANES", 1, 2);
    return d;
}
DiagSwitches &switches()
{
    static DiagSwitches d = read_switches();
    return d;
}
}  // namespace

const DiagSwitches &diag() { return switches(); }
void reload_diag() { switches() = read_switches(); }

int embed(const Geo &g, const float *x, const float *pw, const float *pb, const float *cls, const float *pos, float *out,
          int batch, int img_h, int img_w, hipStream_t stream, Probe &probe)
{
    GemmArgs a{};
    a.A = x; a.W = pw; a.Y = out; a.Y2 = nullptr; a.bias = pb; a.pos = pos;
    a.M = batch * g.P; a.N = g.C; a.K = g.Kp;
    a.lda = g.in_ch * img_h * img_w;   // per-image stride in patch mode
    a.ldy = g.C;
    a.img_h = img_h; a.img_w = img_w; a.gw = g.gw; a.patches = g.P; a.patch = g.p; a.tokens = g.T;
    LDIT_RUN(probe, LDIT_K_GEMM, launch_gemm(a, EPI_EMBED, A_PATCH, stream));
    LDIT_RUN(probe, LDIT_K_OTHER, launch_cls_rows(cls, pos, out, batch, g.T, g.C, stream));
    return LDIT_OK;
}

// One HBM-bound pass rounds the batch to a bf16 im2col matrix `patches` [B P, planes Kp] (split-fp32 builds: the bf16 planes of the
// pixels, the GEMM walks the plane products) and the bf16 MFMA GEMM multiplies it - 16x the fp32 matrix rate for 1.8 - 4.5 % of those
// steps (the fp32 kernel took 266 us of the 14.6 ms ViT-L/512 step, 60 us of the 1.6 ms fp8 step).
int embed_bf16(const Geo &g, const float *x, const ImgSrc *imgs, int planes, void *patches, const void *w16, const float *pb,
               const float *cls, const float *pos, float *out, int batch, int img_h, int img_w, hipStream_t stream, Probe &probe)
{
    if (imgs)       // normalise + bilinear resize of the ragged list INSIDE this pass - no fp32 batch in between
        LDIT_RUN(probe, LDIT_K_OTHER, launch_patches_rows_images(imgs->images, imgs->fmt, imgs->heights, imgs->widths, batch, g.in_ch,
                                                                imgs->mean, imgs->std, img_h, img_w, g.p, patches, stream, planes));
    else
        LDIT_RUN(probe, LDIT_K_OTHER, launch_patches_rows(x, patches, batch, g.in_ch, img_h, img_w, g.p, stream, planes));
    GemmExtra xe = split_segments(planes);
    xe.pos = pos; xe.patches = g.P;
    LDIT_RUN(probe, LDIT_K_GEMM, launch_gemm_bf16_ex(patches, planes * g.Kp, w16, pb, out, g.C, batch * g.P, g.C, g.Kp, EPI_EMBED, nullptr,
                                                    nullptr, nullptr, xe, stream));
    LDIT_RUN(probe, LDIT_K_OTHER, launch_cls_rows(cls, pos, out, batch, g.T, g.C, stream));
    return LDIT_OK;
}

// LayerNorm of the fp32 residual stream into the build's operand format (Yd: mxfp8 training, the dequantised copy)
int layernorm(Build b, const float *X, const float *gamma, const float *beta, const Operand &Y, void *Yd, int64_t rows, int C, float eps, hipStream_t stream)
{
    switch (b.dtype) {
        case LDIT_F32: return launch_layernorm(X, gamma, beta, static_cast<float *>(Y.p), rows, C, eps, stream);
        case LDIT_BF16: return launch_layernorm_bf16out(X, gamma, beta, Y.p, rows, C, eps, stream);
        case LDIT_FP8: return launch_layernorm_fp8out(X, gamma, beta, Y.p, rows, C, eps, static_cast<const float *>(Y.s), stream);
        case LDIT_MXFP8:
            return b.train ? launch_layernorm_mxout_train(X, gamma, beta, Y.p, Y.s, Yd, rows, C, eps, stream)
                           : launch_layernorm_mxout(X, gamma, beta, Y.p, Y.s, rows, C, eps, stream);
        case LDIT_F32X3: case LDIT_F32X6: return launch_layernorm_splitout(X, gamma, beta, Y.p, rows, C, eps, Y.planes, stream);
        default: return fail(LDIT_EUNSUPPORTED, "layernorm: no kernel for dtype %d", b.dtype);
    }
}

// Y = epi(A . W^T + bias) on the build's operand format.  Y is an operand of the build when the next launch multiplies it (q|k|v, the
// MLP hidden), else the fp32 residual stream.  ab_scale / out_inv_scale: host scales of ldit_linear_fp8 (the fp8 build reads A.s, Y.s).
int linear(Build b, const Operand &A, const void *W, const void *Ws, const float *bias, const Operand &Y, int M, int N, int K, int epi,
           const float *lam, const float *R, float *Y2, const Side &t, hipStream_t stream, float ab_scale, float out_inv_scale)
{
    switch (b.dtype) {
        case LDIT_F32: {
            GemmArgs a{};
            a.A = static_cast<const float *>(A.p); a.W = static_cast<const float *>(W); a.Y = static_cast<float *>(Y.p); a.Y2 = Y2;
            a.bias = bias; a.lam = lam; a.R = R;
            a.M = M; a.N = N; a.K = K; a.lda = A.ld; a.ldy = Y.ld;
            return launch_gemm(a, epi, A_ROWMAJOR, stream);
        }
        case LDIT_BF16: case LDIT_F32X3: case LDIT_F32X6: {
            // split-fp32 builds: the bf16 MFMA over the plane products of the operands, fp32 accumulation; an output that is an operand
            // leaves as planes [M, S N] (q pre-multiplied by scale log2 e at pack time: attention_flash.hip runs on the plane products too)
            GemmExtra x = split_segments(A.planes);
            x.Ypre = t.Ypre; x.rowscale = t.rowscale;
            if (Y.planes) { x.nsplit_out = Y.planes; epi = epi == EPI_BIAS_GELU ? EPI_GELU_SPLIT : EPI_BIAS_SPLIT; }
            return launch_gemm_bf16_ex(A.p, A.ld, W, bias, Y.p, Y.ld, M, N, K, epi, lam, R, Y2, x, stream);
        }
        case LDIT_FP8:
            return launch_gemm_fp8(A.p, A.ld, W, bias, Y.p, Y.ld, M, N, K, epi, lam, R, Y2, ab_scale, out_inv_scale,
                                   static_cast<const float *>(A.s), static_cast<const float *>(Ws), static_cast<const float *>(Y.s), stream);
        case LDIT_MXFP8:
            // the train kernel exists for the two epilogues that have side stores; q|k|v has none
            if (b.train && epi != EPI_BIAS)
                return launch_gemm_mxfp8_train(A.p, A.ld, A.s, W, Ws, bias, Y.p, Y.ld, Y.s, M, N, K, epi, lam, R, Y2, t.Ypre, t.rowscale, t.Yd, stream);
            return launch_gemm_mxfp8(A.p, A.ld, A.s, W, Ws, bias, Y.p, Y.ld, Y.s, M, N, K, epi, lam, R, Y2, stream);
        default: return fail(LDIT_EUNSUPPORTED, "linear: no kernel for dtype %d", b.dtype);
    }
}

// O = softmax(Q K^T) V per head, heads merged token-major, into the build's operand format.  Split builds: ldq = row stride of the
// q|k|v planes, plane_in = distance between a row's planes.  Training: lse, and (mxfp8) Ob / Od, the bf16 output and its dequantised codes.
int attention(Build b, const void *Q, const void *K, const void *V, int ldq, int ldk, int ldv, const Operand &O, int B, int N, int H, int D,
              float scale, hipStream_t stream, float *lse, void *Ob, void *Od, int plane_in)
{
    switch (b.dtype) {
        case LDIT_F32:
            return launch_attention(static_cast<const float *>(Q), static_cast<const float *>(K), static_cast<const float *>(V),
                                    static_cast<float *>(O.p), B, N, H, D, ldq, ldk, ldv, O.ld, scale, stream);
        case LDIT_BF16: case LDIT_FP8: case LDIT_MXFP8: case LDIT_F32X3: case LDIT_F32X6: {
            AttnArgs a{};
            a.Q = Q; a.K = K; a.V = V; a.O = O.p;
            a.B = B; a.N = N; a.H = H; a.D = D; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = O.ld;
            a.scale = scale;
            if (b.dtype == LDIT_BF16) {
                if (b.train && !lse) return fail(LDIT_EINVAL, "attention_bf16: lse is null");
                a.out = ATTN_BF16; a.lse = b.train ? lse : nullptr;
            } else if (b.dtype == LDIT_FP8) {
                a.out = ATTN_FP8; a.qscale = static_cast<const float *>(O.s);
            } else if (b.dtype == LDIT_MXFP8) {
                a.out = b.train ? ATTN_MX_TRAIN : ATTN_MX; a.Os = O.s;
                if (b.train) { a.lse = lse; a.Ob = Ob; a.Od = Od; }
            } else {
                a.out = ATTN_PLANES; a.planes = O.planes; a.plane_in = plane_in;
            }
            return launch_attention_flash(a, stream);
        }
        default: return fail(LDIT_EUNSUPPORTED, "attention: no kernel for dtype %d", b.dtype);
    }
}

// The seven launches of one encoder layer.  The residual stream, LayerNorm statistics, softmax and every accumulation are fp32 in
// every build; what the build decides is the format of the four GEMM operands and of q|k|v (Operand), behind the three dispatchers.
int layer_launch(int i, Build b, const Geo &g, int batch, float eps, const Layer &d, hipStream_t stream, Probe &probe)
{
    const int M = batch * g.T, C = g.C, F = g.F;
    const char *q = static_cast<const char *>(d.qkv.p), *k = q + d.qk_bytes, *v = k + d.qk_bytes;
    const Operand mid = operand(d.h_mid, nullptr, C), out = operand(d.h_out, nullptr, C);
    const PackedLayer &pv = *d.v, &pw = *d.w;
    switch (i) {
        case 0:   // y1 = LN1(h_in)                                                            TF:426
            LDIT_RUN(probe, LDIT_K_LAYERNORM, layernorm(b, d.h_in, d.vec(pv.ln1_w), d.vec(pv.ln1_b), d.y1, d.y1d, M, C, eps, stream));
            return LDIT_OK;
        case 1:   // qkv[:, 0:3C] = y1 . [Wq;Wk;Wv]^T + [bq;0;bv]                              TF:319-321
            LDIT_RUN(probe, LDIT_K_GEMM, linear(b, d.y1, d.mat(pw.wqkv), d.W + pw.sw_qkv, d.bqkv, d.qkv, M, 3 * C, C, EPI_BIAS, nullptr, nullptr, nullptr, Side{}, stream));
            return LDIT_OK;
        case 2:   // o = softmax(q k^T / sqrt(D)) v, heads merged token-major                  TF:323-338
            LDIT_RUN(probe, LDIT_K_ATTENTION, attention(b, q, k, v, d.qkv.ld, d.qkv.ld, d.qkv.ld, d.o, batch, g.T, g.H, g.D, d.scale, stream, d.lse, d.ob, d.od,
                                                        d.qkv.planes ? d.qkv.ld / d.qkv.planes : 0));
            return LDIT_OK;
        case 3:   // h_mid = h_in + lam1 (.) (o . Wo^T + bo)                                   TF:339, 432-434
            LDIT_RUN(probe, LDIT_K_GEMM, linear(b, d.o, d.mat(pw.wo), d.W + pw.sw_o, d.vec(pv.bo), mid, M, C, C, EPI_SCALE_RESID, d.vec(pv.lam1), d.h_in, nullptr, d.s_o, stream));
            return LDIT_OK;
        case 4:   // y2 = LN2(h_mid)                                                           TF:438
            LDIT_RUN(probe, LDIT_K_LAYERNORM, layernorm(b, d.h_mid, d.vec(pv.ln2_w), d.vec(pv.ln2_b), d.y2, d.y2d, M, C, eps, stream));
            return LDIT_OK;
        case 5:   // hid[:, 0:F] = gelu(y2 . W1^T + b1)                                        TF:353-354
            LDIT_RUN(probe, LDIT_K_GEMM, linear(b, d.y2, d.mat(pw.w1), d.W + pw.sw_1, d.vec(pv.b1), d.hid, M, F, C, EPI_BIAS_GELU, nullptr, nullptr, nullptr, d.s_fc1, stream));
            return LDIT_OK;
        case 6:   // h_out = h_mid + lam2 (.) (hid . W2^T + b2)  (+ tap copy of the new hidden state)   TF:355, 440-442
            LDIT_RUN(probe, LDIT_K_GEMM, linear(b, d.hid, d.mat(pw.w2), d.W + pw.sw_2, d.vec(pv.b2), out, M, C, F, EPI_SCALE_RESID, d.vec(pv.lam2), d.h_mid, d.tap, d.s_fc2, stream));
            return LDIT_OK;
        default: return fail(LDIT_EINVAL, "layer_launch: no launch %d", i);
    }
}

int run_layer(Build b, const Geo &g, int batch, float eps, const Layer &d, hipStream_t stream, Probe &probe)
{
    for (int i = 0; i < LAYER_LAUNCHES; ++i) LDIT_TRY(layer_launch(i, b, g, batch, eps, d, stream, probe));
    return LDIT_OK;
}

// Token rows M = batch * T from which the fp32 forward runs as two lanes.  Measured on ViT-B/16 224^2 (profiles/forward_lanes_ab.txt):
// batch 64 +2.2 .. 2.6 %, batch 48 +8.7 % in all three alternations; batch 32 a tie (+-0.3 %), batch 16 -7 %: a half-batch no
// longer fills the chip.  The smallest batch that won every time sets the bound.
constexpr int FWD_LANES_MIN_ROWS = 48 * 197;

int forward_lanes(int dtype, const Geo &g, int batch)
{
    if (dtype != LDIT_F32 || batch < 2) return 1;
    if (const int force = diag().fwd_lanes; force > 0) return force;
    return (int64_t)batch * g.T >= FWD_LANES_MIN_ROWS ? 2 : 1;
}

namespace {

// geometry of the stand-alone embedding entries (the caller has checked the divisions)
Geo embed_geo(int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C)
{
    Geo g{};
    g.C = (int)C; g.p = (int)p; g.in_ch = (int)in_ch; g.gh = (int)(img_h / p); g.gw = (int)(img_w / p);
    g.P = g.gh * g.gw; g.T = g.P + 1; g.Kp = (int)(in_ch * p * p);
    return g;
}

// ldit_embed_bf16 (the fp32 batch `x`) and ldit_embed_bf16_images (the image list `imgs`)
int embed_bf16_entry(const char *name, const void *x, const ImgSrc *imgs, const void *patch_w_bf16, const void *patch_b, const void *cls,
                     const void *pos, void *out, void *scratch, int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C,
                     ldit_stream stream)
{
    if (B <= 0 || (imgs && B > 65535) || in_ch <= 0 || img_h <= 0 || img_w <= 0 || p <= 0 || C <= 0) return fail(LDIT_EINVAL, "%s: empty problem", name);
    if (img_h % p || img_w % p)
        return fail(LDIT_EINVAL, "%s: %s %lldx%lld is not a multiple of patch %lld", name, imgs ? "target" : "image", (long long)img_h, (long long)img_w, (long long)p);
    if ((imgs ? !imgs->images || !imgs->heights || !imgs->widths : !x) || !patch_w_bf16 || !patch_b || !cls || !pos || !out || !scratch)
        return fail(LDIT_EINVAL, "%s: null operand", name);
    if (imgs && !(imgs->std > 0.0f)) return fail(LDIT_EINVAL, "%s: std must be positive", name);
    if (!aligned16(out) || !aligned16(pos) || !aligned16(scratch) || !aligned16(patch_w_bf16) || (C & 3))
        return fail(LDIT_EINVAL, "%s: out / pos / scratch / patch_w must be 16-byte aligned, C a multiple of 4", name);
    const int64_t P = (img_h / p) * (img_w / p), Kp = in_ch * p * p;
    if (Kp % 64) return fail(LDIT_EUNSUPPORTED, "%s: in_ch*p*p = %lld must be a multiple of 64", name, (long long)Kp);
    if (B * in_ch * img_h * img_w >= (1ll << 31) || B * (P + 1) * C >= (1ll << 31) || B * P * Kp >= (1ll << 31))
        return fail(LDIT_EUNSUPPORTED, "%s: operand exceeds 2^31 elements", name);
    Probe probe;
    return embed_bf16(embed_geo(in_ch, img_h, img_w, p, C), static_cast<const float *>(x), imgs, 1, scratch, patch_w_bf16,
                      static_cast<const float *>(patch_b), static_cast<const float *>(cls), static_cast<const float *>(pos), static_cast<float *>(out),
                      (int)B, (int)img_h, (int)img_w, static_cast<hipStream_t>(stream), probe);
}

// ldit_linear_f32
int linear_entry(const char *name, int dtype, const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M, int64_t N,
                 int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, ldit_stream stream)
{
    LDIT_TRY(check_linear(name, M, N, K, lda, ldy, Y, Y2, epilogue));
    return linear(Build{dtype, false}, operand(X, nullptr, lda), W, nullptr, static_cast<const float *>(bias), operand(Y, nullptr, ldy), (int)M, (int)N,
                  (int)K, epilogue, static_cast<const float *>(lam), static_cast<const float *>(R), static_cast<float *>(Y2), Side{},
                  static_cast<hipStream_t>(stream));
}

// ldit_attention_f32 / ldit_attention_bf16; qtile: query rows per workgroup of the kernel
int attention_entry(const char *name, int dtype, int64_t qtile, const void *Q, const void *K, const void *V, void *O, int64_t B, int64_t N, int64_t H,
                    int64_t D, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, ldit_stream stream)
{
    if (B <= 0 || N <= 0 || H <= 0) return fail(LDIT_EINVAL, "%s: empty problem", name);
    const int64_t ldmax = ldq > ldk ? (ldq > ldv ? ldq : ldv) : (ldk > ldv ? ldk : ldv);
    if (B * N * (ldmax > ldo ? ldmax : ldo) >= (1ll << 31) || B * H * ((N + qtile - 1) / qtile) >= (1ll << 31))
        return fail(LDIT_EUNSUPPORTED, "%s: operand exceeds 2^31 elements", name);
    if (ldq < H * D || ldk < H * D || ldv < H * D || ldo < H * D) return fail(LDIT_EINVAL, "%s: row stride smaller than H*D", name);
    return attention(Build{dtype, false}, Q, K, V, (int)ldq, (int)ldk, (int)ldv, operand(O, nullptr, ldo), (int)B, (int)N, (int)H, (int)D, scale,
                     static_cast<hipStream_t>(stream));
}

// the storage of a uint8 image list from the `interleaved` argument of the *_u8 entries (0 or 1)
int u8_format(const char *name, int32_t interleaved, ImgFmt &fmt)
{
    if (interleaved != 0 && interleaved != 1) return fail(LDIT_EINVAL, "%s: interleaved = %d (0: planar, 1: interleaved)", name, interleaved);
    fmt = interleaved ? IMG_U8_HWC : IMG_U8;
    return LDIT_OK;
}

int preprocess(ImgFmt fmt, const void *const *images, const int32_t *heights, const int32_t *widths, int32_t B, int32_t in_ch, float mean,
               float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream)
{
    if (!images || !heights || !widths || !out) return fail(LDIT_EINVAL, "preprocess: null argument");
    if (B <= 0 || B > 65535 || in_ch <= 0 || out_h <= 0 || out_w <= 0) return fail(LDIT_EINVAL, "preprocess: bad geometry");
    if (!(std > 0.0f)) return fail(LDIT_EINVAL, "preprocess: std must be positive");
    if ((int64_t)B * in_ch * out_h * out_w >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "preprocess: batch exceeds 2^31 elements");
    return launch_preprocess(images, fmt, heights, widths, B, in_ch, mean, std, out_h, out_w, static_cast<float *>(out),
                             static_cast<hipStream_t>(stream));
}

// the *_win siblings: the same checks, then the windowed kernels - or, without windows, the entry above itself
int preprocess_win(ImgFmt fmt, const void *const *images, const int32_t *heights, const int32_t *widths, const int32_t *windows, int32_t B,
                   int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream)
{
    if (!windows) return preprocess(fmt, images, heights, widths, B, in_ch, mean, std, out_h, out_w, out, stream);
    if (!images || !heights || !widths || !out) return fail(LDIT_EINVAL, "preprocess: null argument");
    if (B <= 0 || B > 65535 || in_ch <= 0 || out_h <= 0 || out_w <= 0) return fail(LDIT_EINVAL, "preprocess: bad geometry");
    if (!(std > 0.0f)) return fail(LDIT_EINVAL, "preprocess: std must be positive");
    if ((int64_t)B * in_ch * out_h * out_w >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "preprocess: batch exceeds 2^31 elements");
    for (int i = 0; i < B; ++i) {                                   // every window before the first launch
        if (!images[i] || heights[i] <= 0 || widths[i] <= 0) return fail(LDIT_EINVAL, "image %d is null or empty", i);
        LDIT_TRY(check_window(windows + (size_t)i * 5, i, heights[i], widths[i]));
    }
    return launch_preprocess_windows(images, fmt, heights, widths, windows, B, in_ch, mean, std, out_h, out_w, static_cast<float *>(out),
                                     static_cast<hipStream_t>(stream));
}

// The side stream of the two-lane forward: one non-blocking stream per device ordinal, created on first use and kept for the life
// of the process (with the dynamic-LDS bits and the CU count, the library's only per-device state).  Null: ordinal out of range.
int side_stream(hipStream_t &out)
{
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    int dev = 0;
    LDIT_HIP_CHECK(hipGetDevice(&dev));
    out = nullptr;
    if (dev < 0 || dev >= 64) return LDIT_OK;
    std::lock_guard<std::mutex> lock(mu);
    if (!streams[dev]) LDIT_HIP_CHECK(hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking));
    out = streams[dev];
    return LDIT_OK;
}

// Layers of the two-lane fp32 forward.  `full` addresses the whole batch; lane A = images [0, bA) on the caller's stream, lane B =
// the rest on `side`.  Every buffer is indexed by token row, so lane B's Layer is lane A's moved by bA * T rows (of `wide` floats in
// `big`, where q|k|v and the MLP hidden have different row lengths) - no second workspace.  The host alternates the lanes launch by
// launch so that neither queue runs dry behind the other's host work.  Both lanes start together: starting B behind A's q|k|v or
// o_proj measured 0.6 - 2.1 % SLOWER than one lane, starting together 2.2 - 2.6 % faster (profiles/forward_lanes_ab.txt).
int enqueue_lanes(const ldit_cfg *cfg, const Geo &g, const PackedMap &pm, const Layer &full, char *yb, char *bb, int batch, void *const *tap_out,
                  hipStream_t stream, hipStream_t side, hipEvent_t start, bool &forked, Probe &probe)
{
    const int C = g.C, F = g.F, bA = (batch + 1) / 2;
    const size_t wide = (size_t)(3 * C > F ? 3 * C : F);
    const char *P = full.V;
    struct Lane { Layer d; int batch; size_t row0; hipStream_t s; } lane[2] = {{full, bA, 0, stream}, {full, batch - bA, (size_t)bA * g.T, side}};
    for (Lane &n : lane) {
        float *h = const_cast<float *>(full.h_in) + n.row0 * C;
        n.d.h_in = n.d.h_mid = n.d.h_out = h;
        n.d.y1 = n.d.o = n.d.y2 = operand(yb + n.row0 * C * 4, nullptr, C);
        n.d.qkv = operand(bb + n.row0 * wide * 4, nullptr, 3 * C);
        n.d.hid = operand(bb + n.row0 * wide * 4, nullptr, F);
    }
    // the fork: lane B starts behind the embedding
    LDIT_HIP_CHECK(hipEventRecord(start, stream));
    LDIT_HIP_CHECK(hipStreamWaitEvent(side, start, 0));
    forked = true;
    for (int at = 0; at < g.L * LAYER_LAUNCHES; ++at)
        for (Lane &n : lane) {
            const int l = at / LAYER_LAUNCHES, i = at % LAYER_LAUNCHES;
            if (i == 0) {
                const PackedLayer &pl = pm.layer[l];
                n.d.v = n.d.w = &pl; n.d.bqkv = reinterpret_cast<const float *>(P + pl.bqkv);
                float *tap = tap_of(cfg, tap_out, l + 1);
                n.d.tap = tap ? tap + n.row0 * C : nullptr;
            }
            LDIT_TRY(layer_launch(i, Build{LDIT_F32, false}, g, n.batch, cfg->ln_eps, n.d, n.s, probe));
            if (i == LAYER_LAUNCHES - 1 && n.d.tap)
                LDIT_TRY(copy_taps(cfg, tap_out, l + 1, full.h_in, tap_of(cfg, tap_out, l + 1), (size_t)n.batch * g.T * C * 4, n.s, n.row0 * C * 4));
        }
    return LDIT_OK;
}

int forward(const ldit_cfg *cfg, const void *packed, const void *x, int32_t batch, void *const *tap_out, void *workspace,
            size_t ws_bytes, hipStream_t stream, Probe &probe, const ImgSrc *imgs = nullptr)
{
    Geo g;
    LDIT_TRY(geometry(cfg, g));
    LDIT_TRY(check_forward_args(cfg, g, batch, {packed, imgs ? packed : x, workspace}, "packed / x / workspace", imgs, tap_out));
    const int dt = cfg->dtype, S = split_planes_of(dt);
    const Workspace wm = workspace_map(g, batch, dt);
    if (ws_bytes < wm.total) return fail(LDIT_EWORKSPACE, "workspace %zu bytes < required %zu", ws_bytes, wm.total);
    const PackedMap pm = packed_map(g, dt);
    const char *P = static_cast<const char *>(packed);
    auto F32 = [&](size_t off) { return reinterpret_cast<const float *>(P + off); };
    char *ws = static_cast<char *>(workspace), *yb = ws + wm.y, *bb = ws + wm.big;
    float *h = reinterpret_cast<float *>(ws + wm.h);
    const int M = batch * g.T, C = g.C, F = g.F;
    const size_t act_bytes = (size_t)M * C * 4;

    // embeddings (TF:153-176).  fp32 build: the fp32 GEMM gathers the NCHW pixels itself (LDS-DMA source addresses).  Every other
    // build: the bf16 GEMM on the im2col of the batch (into `big`, free until layer 0).
    if (dt != LDIT_F32 && g.Kp % 64 == 0) {
        LDIT_TRY(embed_bf16(g, static_cast<const float *>(x), imgs, S ? S : 1, bb, P + pm.patch_w16, F32(pm.patch_b), F32(pm.cls), F32(pm.pos), h,
                            batch, cfg->img_h, cfg->img_w, stream, probe));
    } else {
        const float *xp = static_cast<const float *>(x);
        if (imgs) {
            // the fp32 GEMM gathers the NCHW pixels on its LDS-DMA operand path, where nothing can be blended: the batch is produced
            // first (same statement, image_blend.h), into `big` - free until layer 0
            const size_t pix = (size_t)batch * g.in_ch * cfg->img_h * cfg->img_w * 4;
            if (wm.total - wm.big < pix) return fail(LDIT_EUNSUPPORTED, "image list: the pixel batch does not fit the workspace of this geometry");
            xp = reinterpret_cast<const float *>(bb);
            LDIT_RUN(probe, LDIT_K_OTHER, launch_preprocess(imgs->images, imgs->fmt, imgs->heights, imgs->widths, batch, g.in_ch, imgs->mean,
                                                           imgs->std, cfg->img_h, cfg->img_w, reinterpret_cast<float *>(bb), stream));
        }
        LDIT_TRY(embed(g, xp, F32(pm.patch_w), F32(pm.patch_b), F32(pm.cls), F32(pm.pos), h, batch, cfg->img_h, cfg->img_w, stream, probe));
    }
    LDIT_TRY(copy_taps(cfg, tap_out, 0, h, nullptr, act_bytes, stream));

    // The buffers in the build's format.  y: LayerNorm output, then attention output; big: q|k|v, later the MLP hidden (never live together).
    // bf16, fp8, mxfp8: q|k|v bf16 for the bf16 attention kernel, whose epilogue - like LayerNorm's and the GELU's - writes bf16, e4m3 codes on
    // the calibrated per-tensor scales, or e4m3 codes [M, K] then one E8M0 scale per 32 channels [M, K / 32].  Split fp32: S bf16 planes per row.
    const bool mx = dt == LDIT_MXFP8;
    const int Sp = S ? S : 1;
    Layer d{};
    d.h_in = d.h_mid = d.h_out = h;
    d.V = d.W = P; d.div = 1;
    d.y1 = d.o = d.y2 = operand(yb, mx ? yb + (size_t)M * C : nullptr, Sp * C, S);
    d.qkv = operand(bb, nullptr, Sp * 3 * C, S);
    d.hid = operand(bb, mx ? bb + (size_t)M * F : nullptr, Sp * F, S);
    d.qk_bytes = (size_t)(dt == LDIT_F32 ? 4 : 2) * C;
    d.scale = dt == LDIT_F32 ? 1.0f / sqrtf((float)g.D) : 0.0f /* q pre-scaled at pack time */;

    // Two half-batch lanes on two streams (fp32, large batches: forward_lanes) - never under the probe, whose events bracket launches
    // of one stream, nor on a capturing stream, so that a captured forward stays a linear graph
    hipStream_t side = nullptr;
    if (!probe.on && g.L > 0 && forward_lanes(dt, g, batch) == 2) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        LDIT_HIP_CHECK(hipStreamIsCapturing(stream, &cap));
        if (cap == hipStreamCaptureStatusNone) LDIT_TRY(side_stream(side));
    }
    if (side) {
        if (C & 3) return fail(LDIT_EINVAL, "forward: hidden %d is not a multiple of 4, lane rows would lose their 16-byte alignment", C);
        hipEvent_t start = nullptr, done = nullptr;
        LDIT_HIP_CHECK(hipEventCreateWithFlags(&start, hipEventDisableTiming));
        if (hipError_t e = hipEventCreateWithFlags(&done, hipEventDisableTiming); e != hipSuccess) {
            (void)hipEventDestroy(start);
            return fail(LDIT_EHIP, "hipEventCreateWithFlags: %s", hipGetErrorString(e));
        }
        bool forked = false;
        int rc = enqueue_lanes(cfg, g, pm, d, yb, bb, batch, tap_out, stream, side, start, forked, probe);
        // the join, on every path out once the side stream has been given work: the caller's stream is never left unordered
        // against launches that touch its buffers
        if (forked) {
            hipError_t e = hipEventRecord(done, side);
            if (e == hipSuccess) e = hipStreamWaitEvent(stream, done, 0);
            if (e != hipSuccess && rc == LDIT_OK) rc = fail(LDIT_EHIP, "forward: joining the side stream: %s", hipGetErrorString(e));
        }
        (void)hipEventDestroy(start);
        (void)hipEventDestroy(done);
        return rc;
    }
    for (int l = 0; l < g.L; ++l) {
        const PackedLayer &pl = pm.layer[l];
        d.v = d.w = &pl; d.bqkv = F32(pl.bqkv);
        if (dt == LDIT_FP8) {     // slots 0, 2, 4, 6 of the layer's scale block
            const float *sc = F32(pl.scales);
            d.y1.s = const_cast<float *>(sc); d.o.s = const_cast<float *>(sc + 2); d.y2.s = const_cast<float *>(sc + 4); d.hid.s = const_cast<float *>(sc + 6);
        }
        d.tap = tap_of(cfg, tap_out, l + 1);
        LDIT_TRY(run_layer(Build{dt, false}, g, batch, cfg->ln_eps, d, stream, probe));
        if (d.tap) LDIT_TRY(copy_taps(cfg, tap_out, l + 1, h, d.tap, act_bytes, stream));
    }
    return LDIT_OK;
}

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_abi_version(void) { return LDIT_ABI_VERSION; }

/* diagnostic: re-read the LDIT_* switches of ldit_common.h from the environment (they are otherwise read once) */
int ldit_debug_reload_env(void)
{
    reload_diag();
    return LDIT_OK;
}

const char *ldit_last_error(void) { return err_buf(); }

size_t ldit_packed_bytes(const ldit_cfg *cfg)
{
    Geo g;
    if (geometry(cfg, g) != LDIT_OK) return 0;
    return packed_map(g, cfg->dtype).total;
}

int ldit_pack_weights(const ldit_cfg *cfg, const ldit_weights *w, void *packed, size_t packed_bytes, ldit_stream stream_)
{
    Geo g;
    LDIT_TRY(geometry(cfg, g));
    if (!w || !packed) return fail(LDIT_EINVAL, "null weights / packed pointer");
    if (!aligned16(packed)) return fail(LDIT_EINVAL, "packed must be 16-byte aligned");
    if (g.L && !w->layer) return fail(LDIT_EINVAL, "weights->layer is null");
    const PackedMap pm = packed_map(g, cfg->dtype);
    if (packed_bytes < pm.total) return fail(LDIT_EWORKSPACE, "packed buffer %zu bytes < required %zu", packed_bytes, pm.total);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char *P = static_cast<char *>(packed);
    const bool bf16 = cfg->dtype == LDIT_BF16, fp8 = cfg->dtype == LDIT_FP8, mx = cfg->dtype == LDIT_MXFP8;
    auto put = [&](size_t off, const void *src, size_t n, const char *what) -> int {      // fp32 copy
        if (!src) return fail(LDIT_EINVAL, "weights: %s is null", what);
        LDIT_HIP_CHECK(hipMemcpyAsync(P + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return LDIT_OK;
    };
    // matrix [rows, cols] at element offset elt_off of the block at `off`: fp32 copy, -> bf16, or -> fp8 codes with one
    // scale per row written to the fp32 vector at sw_off (+ row0)
    // `mul` (bf16 / fp8 builds only): a factor folded into the matrix as it is packed (bf16: into the values before the one
    // rounding; fp8: into the per-row scales).  Used for W_q: q' = (scale log2 e) q, so that the attention kernel's scores
    // are exp2-domain exponents (attention_flash.hip, PRE) - the same single rounding of q as before, no extra error.
    auto put_mat = [&](size_t off, size_t elt_off, const void *src, size_t rows, size_t cols, size_t sw_off, size_t row0,
                       const char *what, float mul = 1.0f) -> int {
        if (!src) return fail(LDIT_EINVAL, "weights: %s is null", what);
        if (const int Sp = split_planes_of(cfg->dtype)) {
            // split-fp32 builds: the matrix as Sp bf16 planes side by side per row; `elt_off` counts fp32 elements of whole rows
            if (!aligned16(src)) return fail(LDIT_EINVAL, "weights: %s must be 16-byte aligned", what);
            return launch_split_planes(static_cast<const float *>(src), (int)cols, P + off + elt_off * 2 * Sp, (int)rows, (int)cols, Sp, stream, mul);
        }
        if (!bf16 && !fp8 && !mx) return put(off + elt_off * 4, src, rows * cols, what);
        if (!aligned16(src)) return fail(LDIT_EINVAL, "weights: %s must be 16-byte aligned", what);
        // mxfp8: codes + block scales of the rows; `mul` goes into the values before they are quantised (no per-row float scale)
        if (mx)
            return launch_quant_mx(static_cast<const float *>(src), (int64_t)cols, P + off + elt_off, P + sw_off + row0 * (cols / 32),
                                   (int64_t)rows, (int)cols, mul, stream);
        if (fp8)
            return launch_quant_rows_fp8(static_cast<const float *>(src), P + off + elt_off,
                                         reinterpret_cast<float *>(P + sw_off) + row0, (int)rows, (int)cols, stream, mul);
        return launch_cvt_bf16(static_cast<const float *>(src), P + off + elt_off * 2, rows * cols, stream, mul);
    };
    // (the split-fp32 builds too: their attention runs on bf16-plane operands with exp2-domain scores, attention_flash.hip)
    const float qfold = cfg->dtype != LDIT_F32 ? qfold_of(g) : 1.0f;
    const size_t C = g.C, F = g.F;
    LDIT_TRY(put(pm.patch_w, w->patch_w, C * g.Kp, "patch_w"));
    if (bf16 || fp8 || mx) {
        if (!aligned16(w->patch_w)) return fail(LDIT_EINVAL, "weights: patch_w must be 16-byte aligned");
        LDIT_TRY(launch_cvt_bf16(static_cast<const float *>(w->patch_w), P + pm.patch_w16, C * g.Kp, stream));
    } else if (const int Sp = split_planes_of(cfg->dtype)) {
        if (!aligned16(w->patch_w)) return fail(LDIT_EINVAL, "weights: patch_w must be 16-byte aligned");
        LDIT_TRY(launch_split_planes(static_cast<const float *>(w->patch_w), g.Kp, P + pm.patch_w16, (int)C, g.Kp, Sp, stream));
    }
    LDIT_TRY(put(pm.patch_b, w->patch_b, C, "patch_b"));
    LDIT_TRY(put(pm.cls, w->cls, C, "cls"));
    LDIT_TRY(put(pm.pos, w->pos, (size_t)g.T * C, "pos"));
    for (int l = 0; l < g.L; ++l) {
        const ldit_layer_weights &s = w->layer[l];
        const PackedLayer &pl = pm.layer[l];
        LDIT_TRY(put(pl.ln1_w, s.ln1_w, C, "ln1_w"));
        LDIT_TRY(put(pl.ln1_b, s.ln1_b, C, "ln1_b"));
        if (fp8) LDIT_HIP_CHECK(hipMemsetAsync(P + pl.scales, 0, 8 * sizeof(float), stream));
        LDIT_TRY(put_mat(pl.wqkv, 0, s.wq, C, C, pl.sw_qkv, 0, "wq", qfold));
        LDIT_TRY(put_mat(pl.wqkv, C * C, s.wk, C, C, pl.sw_qkv, C, "wk"));
        LDIT_TRY(put_mat(pl.wqkv, 2 * C * C, s.wv, C, C, pl.sw_qkv, 2 * C, "wv"));
        if (!s.bq || !s.bv) return fail(LDIT_EINVAL, "weights: bq / bv is null");
        LDIT_TRY(launch_pack_qkv_bias(static_cast<const float *>(s.bq), static_cast<const float *>(s.bv),
                                      reinterpret_cast<float *>(P + pl.bqkv), g.C, stream, qfold));
        LDIT_TRY(put_mat(pl.wo, 0, s.wo, C, C, pl.sw_o, 0, "wo"));
        LDIT_TRY(put(pl.bo, s.bo, C, "bo"));
        LDIT_TRY(put(pl.lam1, s.lam1, C, "lam1"));
        LDIT_TRY(put(pl.ln2_w, s.ln2_w, C, "ln2_w"));
        LDIT_TRY(put(pl.ln2_b, s.ln2_b, C, "ln2_b"));
        LDIT_TRY(put_mat(pl.w1, 0, s.w1, F, C, pl.sw_1, 0, "w1"));
        LDIT_TRY(put(pl.b1, s.b1, F, "b1"));
        LDIT_TRY(put_mat(pl.w2, 0, s.w2, C, F, pl.sw_2, 0, "w2"));
        LDIT_TRY(put(pl.b2, s.b2, C, "b2"));
        LDIT_TRY(put(pl.lam2, s.lam2, C, "lam2"));
    }
    return LDIT_OK;
}

int ldit_set_fp8_act_scales(const ldit_cfg *cfg, void *packed, size_t packed_bytes, const float *act_scales, ldit_stream stream_)
{
    Geo g;
    LDIT_TRY(geometry(cfg, g));
    if (cfg->dtype != LDIT_FP8) return fail(LDIT_EINVAL, "set_fp8_act_scales: cfg.dtype is not LDIT_FP8");
    if (!packed || !act_scales) return fail(LDIT_EINVAL, "set_fp8_act_scales: null pointer");
    const PackedMap pm = packed_map(g, cfg->dtype);
    if (packed_bytes < pm.total) return fail(LDIT_EWORKSPACE, "packed buffer %zu bytes < required %zu", packed_bytes, pm.total);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char *P = static_cast<char *>(packed);
    for (int l = 0; l < g.L; ++l)
        for (int a = 0; a < LDIT_FP8_A_COUNT; ++a) {
            const float v = act_scales[l * LDIT_FP8_A_COUNT + a];
            if (!(v > 0.0f) || !std::isfinite(v)) return fail(LDIT_EINVAL, "set_fp8_act_scales: layer %d scale %d = %g is not positive", l, a, (double)v);
            // slots 0, 2, 4, 6 of the layer's scale block; 4-byte pageable copies complete before the call returns
            LDIT_HIP_CHECK(hipMemcpyAsync(P + pm.layer[l].scales + 8 * a, &act_scales[l * LDIT_FP8_A_COUNT + a], sizeof(float),
                                          hipMemcpyHostToDevice, stream));
        }
    return LDIT_OK;
}

int32_t ldit_forward_lanes(const ldit_cfg *cfg, int32_t batch)
{
    Geo g;
    if (batch <= 0 || geometry(cfg, g) != LDIT_OK) return 0;
    return forward_lanes(cfg->dtype, g, batch);
}

size_t ldit_workspace_bytes(const ldit_cfg *cfg, int32_t batch)
{
    Geo g;
    if (batch <= 0 || geometry(cfg, g) != LDIT_OK) return 0;
    return workspace_map(g, batch, cfg->dtype).total;
}

int ldit_vit_forward(const ldit_cfg *cfg, const void *packed, const void *x, int32_t batch, void *const *tap_out,
                     void *workspace, size_t workspace_bytes, ldit_stream stream)
{
    Probe probe;
    return forward(cfg, packed, x, batch, tap_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), probe);
}

int ldit_vit_forward_images(const ldit_cfg *cfg, const void *packed, const void *const *images, const int32_t *heights,
                            const int32_t *widths, int32_t half_in, float mean, float std, int32_t batch, void *const *tap_out,
                            void *workspace, size_t workspace_bytes, ldit_stream stream)
{
    Probe probe;
    const ImgSrc src{images, heights, widths, half_in ? IMG_F16 : IMG_F32, mean, std};
    return forward(cfg, packed, nullptr, batch, tap_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), probe, &src);
}

int ldit_vit_forward_images_u8(const ldit_cfg *cfg, const void *packed, const void *const *images, const int32_t *heights,
                               const int32_t *widths, int32_t interleaved, float mean, float std, int32_t batch, void *const *tap_out,
                               void *workspace, size_t workspace_bytes, ldit_stream stream)
{
    Probe probe;
    ImgSrc src{images, heights, widths, IMG_U8, mean, std};
    LDIT_TRY(u8_format("vit_forward_images_u8", interleaved, src.fmt));
    return forward(cfg, packed, nullptr, batch, tap_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), probe, &src);
}

int ldit_vit_forward_timed(const ldit_cfg *cfg, const void *packed, const void *x, int32_t batch, void *const *tap_out,
                           void *workspace, size_t workspace_bytes, ldit_stream stream, double *ms, int64_t *launches)
{
    if (!ms || !launches) return fail(LDIT_EINVAL, "ms / launches is null");
    Probe probe;
    probe.on = true;
    probe.stream = static_cast<hipStream_t>(stream);
    int rc = forward(cfg, packed, x, batch, tap_out, workspace, workspace_bytes, probe.stream, probe);
    int rc2 = probe.collect(ms, launches);
    return rc != LDIT_OK ? rc : rc2;
}

int ldit_linear_f32(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M,
                    int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, ldit_stream stream)
{
    return linear_entry("linear", LDIT_F32, X, lda, W, bias, Y, ldy, M, N, K, epilogue, lam, R, Y2, stream);
}

int ldit_layernorm_f32(const void *X, const void *gamma, const void *beta, void *Y, int64_t rows, int64_t C, float eps,
                       ldit_stream stream)
{
    if (C > (1 << 20)) return fail(LDIT_EINVAL, "layernorm: C out of range");
    return launch_layernorm(static_cast<const float *>(X), static_cast<const float *>(gamma), static_cast<const float *>(beta),
                            static_cast<float *>(Y), rows, (int)C, eps, static_cast<hipStream_t>(stream));
}

int ldit_attention_f32(const void *Q, const void *K, const void *V, void *O, int64_t B, int64_t N, int64_t H, int64_t D,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, ldit_stream stream)
{
    return attention_entry("attention", LDIT_F32, 128, Q, K, V, O, B, N, H, D, ldq, ldk, ldv, ldo, scale, stream);
}

int ldit_embed_f32(const void *x, const void *patch_w, const void *patch_b, const void *cls, const void *pos, void *out,
                   int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream)
{
    if (B <= 0 || in_ch <= 0 || img_h <= 0 || img_w <= 0 || p <= 0 || C <= 0) return fail(LDIT_EINVAL, "embed: empty problem");
    if (img_h % p || img_w % p) return fail(LDIT_EINVAL, "embed: image %lldx%lld is not a multiple of patch %lld", (long long)img_h, (long long)img_w, (long long)p);
    if (!x || !patch_w || !patch_b || !cls || !pos || !out) return fail(LDIT_EINVAL, "embed: null operand");
    if (!aligned16(out) || !aligned16(pos) || (C & 3)) return fail(LDIT_EINVAL, "embed: out / pos must be 16-byte aligned, C a multiple of 4");
    const Geo g = embed_geo(in_ch, img_h, img_w, p, C);
    if (B * in_ch * img_h * img_w >= (1ll << 31) || B * g.T * C >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "embed: operand exceeds 2^31 elements");
    Probe probe;
    return embed(g, static_cast<const float *>(x), static_cast<const float *>(patch_w), static_cast<const float *>(patch_b),
                 static_cast<const float *>(cls), static_cast<const float *>(pos), static_cast<float *>(out), (int)B,
                 (int)img_h, (int)img_w, static_cast<hipStream_t>(stream), probe);
}

int ldit_attention_planes(const void *Q, const void *K, const void *V, void *O, int64_t B, int64_t N, int64_t H, int64_t D,
                          int64_t ld_in, int64_t plane_in, int64_t ldo, int32_t planes, ldit_stream stream)
{
    if (planes != 2 && planes != 3) return fail(LDIT_EINVAL, "attention_planes: %d planes (2 or 3)", planes);
    if (B <= 0 || N <= 0 || H <= 0) return fail(LDIT_EINVAL, "attention_planes: empty problem");
    if (B * N * (ld_in > ldo ? ld_in : ldo) >= (1ll << 31) || B * H * ((N + 127) / 128) >= (1ll << 31))
        return fail(LDIT_EUNSUPPORTED, "attention_planes: operand exceeds 2^31 elements");
    return attention(Build{LDIT_F32X3, false}, Q, K, V, (int)ld_in, (int)ld_in, (int)ld_in, operand(O, nullptr, ldo, planes), (int)B, (int)N, (int)H,
                     (int)D, 0.0f, static_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, (int)plane_in);
}

int ldit_split_f32_planes(const void *src, int64_t lds, void *dst, int64_t rows, int64_t cols, int32_t planes, ldit_stream stream)
{
    if (rows < 0 || cols < 0 || rows * (lds > planes * cols ? lds : planes * cols) >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "split_planes: operand exceeds 2^31 elements");
    return launch_split_planes(static_cast<const float *>(src), (int)lds, dst, (int)rows, (int)cols, planes, static_cast<hipStream_t>(stream));
}

int ldit_layernorm_f32_planes(const void *X, const void *gamma, const void *beta, void *Y, int64_t rows, int64_t C, float eps,
                              int32_t planes, ldit_stream stream)
{
    if (C > (1 << 20)) return fail(LDIT_EINVAL, "layernorm: C out of range");
    return layernorm(Build{LDIT_F32X3, false}, static_cast<const float *>(X), static_cast<const float *>(gamma), static_cast<const float *>(beta),
                     operand(Y, nullptr, planes * C, planes), nullptr, rows, (int)C, eps, static_cast<hipStream_t>(stream));
}

int ldit_linear_planes(const void *Xp, int64_t lda, const void *Wp, const void *bias, void *Y, int64_t ldy, int64_t M, int64_t N,
                       int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, int32_t planes, ldit_stream stream)
{
    if (planes != 2 && planes != 3) return fail(LDIT_EINVAL, "linear_planes: %d planes (2 or 3)", planes);
    LDIT_TRY(check_linear("linear_planes", M, N, K, lda, ldy, Y, Y2, LDIT_EPI_BIAS, planes));
    GemmExtra x = split_segments(planes);
    int epi;
    if (epilogue == LDIT_EPI_BIAS) epi = EPI_F32;
    else if (epilogue == LDIT_EPI_SCALE_RESID) epi = EPI_SCALE_RESID;
    else if (epilogue == LDIT_EPI_BIAS_GELU) { epi = EPI_GELU_SPLIT; x.nsplit_out = planes; }
    else return fail(LDIT_EINVAL, "linear_planes: unknown epilogue %d", epilogue);
    if (epi != EPI_GELU_SPLIT && ldy < N) return fail(LDIT_EINVAL, "linear_planes: bad output stride");
    return launch_gemm_bf16_ex(Xp, (int)lda, Wp, static_cast<const float *>(bias), Y, (int)ldy, (int)M, (int)N, (int)K, epi,
                               static_cast<const float *>(lam), static_cast<const float *>(R), static_cast<float *>(Y2), x,
                               static_cast<hipStream_t>(stream));
}

int ldit_embed_bf16(const void *x, const void *patch_w_bf16, const void *patch_b, const void *cls, const void *pos, void *out,
                    void *scratch, int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream)
{
    return embed_bf16_entry("embed_bf16", x, nullptr, patch_w_bf16, patch_b, cls, pos, out, scratch, B, in_ch, img_h, img_w, p, C, stream);
}

int ldit_embed_bf16_images(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t half_in, float mean,
                           float std, const void *patch_w_bf16, const void *patch_b, const void *cls, const void *pos, void *out,
                           void *scratch, int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream)
{
    const ImgSrc src{images, heights, widths, half_in ? IMG_F16 : IMG_F32, mean, std};
    return embed_bf16_entry("embed_bf16_images", nullptr, &src, patch_w_bf16, patch_b, cls, pos, out, scratch, B, in_ch, img_h, img_w, p, C, stream);
}

int ldit_embed_bf16_images_u8(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t interleaved, float mean,
                              float std, const void *patch_w_bf16, const void *patch_b, const void *cls, const void *pos, void *out,
                              void *scratch, int64_t B, int64_t in_ch, int64_t img_h, int64_t img_w, int64_t p, int64_t C, ldit_stream stream)
{
    ImgSrc src{images, heights, widths, IMG_U8, mean, std};
    LDIT_TRY(u8_format("embed_bf16_images_u8", interleaved, src.fmt));
    return embed_bf16_entry("embed_bf16_images_u8", nullptr, &src, patch_w_bf16, patch_b, cls, pos, out, scratch, B, in_ch, img_h, img_w, p, C, stream);
}

int ldit_tap_to_map_f32(const void *tap, void *out, int64_t B, int64_t Gh, int64_t Gw, int64_t C, float scale,
                        ldit_stream stream)
{
    if (!tap || !out || !aligned16(tap)) return fail(LDIT_EINVAL, "tap_to_map: null or misaligned operand");
    if (B * (Gh * Gw + 1) * C >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "tap_to_map: operand exceeds 2^31 elements");
    return launch_tap_to_map(static_cast<const float *>(tap), static_cast<float *>(out), (int)B, (int)Gh, (int)Gw, (int)C,
                             scale, static_cast<hipStream_t>(stream));
}

int ldit_tap_to_map_bwd_f32(const void *dmap, void *dtap, int64_t B, int64_t Gh, int64_t Gw, int64_t C, float scale, ldit_stream stream)
{
    if (B * (Gh * Gw + 1) * C >= (1ll << 31) || (double)B * C * Gh * Gw * scale * scale >= 2147483648.0)
        return fail(LDIT_EUNSUPPORTED, "tap_to_map_bwd: operand exceeds 2^31 elements");
    return launch_tap_to_map_bwd(static_cast<const float *>(dmap), static_cast<float *>(dtap), (int)B, (int)Gh, (int)Gw, (int)C, scale,
                                 static_cast<hipStream_t>(stream));
}

int ldit_linear_bf16(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M,
                     int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, ldit_stream stream)
{
    int epi;
    switch (epilogue) {
        case LDIT_EPI_BIAS: epi = EPI_BIAS; break;
        case LDIT_EPI_BIAS_GELU: epi = EPI_BIAS_GELU; break;
        case LDIT_EPI_SCALE_RESID: epi = EPI_SCALE_RESID; break;
        case LDIT_EPI_BIAS_RELU: epi = EPI_BIAS_RELU; break;          // (the bf16 GEMM alone has it: every other entry refuses it)
        default: return fail(LDIT_EINVAL, "linear_bf16: unknown epilogue %d", epilogue);
    }
    LDIT_TRY(check_linear("linear_bf16", M, N, K, lda, ldy, Y, Y2));
    return linear(Build{LDIT_BF16, false}, operand(X, nullptr, lda), W, nullptr, static_cast<const float *>(bias), operand(Y, nullptr, ldy), (int)M,
                  (int)N, (int)K, epi, static_cast<const float *>(lam), static_cast<const float *>(R), static_cast<float *>(Y2), Side{},
                  static_cast<hipStream_t>(stream));
}

int ldit_attention_bf16(const void *Q, const void *K, const void *V, void *O, int64_t B, int64_t N, int64_t H, int64_t D,
                        int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, ldit_stream stream)
{
    return attention_entry("attention_bf16", LDIT_BF16, 256, Q, K, V, O, B, N, H, D, ldq, ldk, ldv, ldo, scale, stream);
}

int ldit_cast_f32_bf16(const void *src, void *dst, int64_t n, ldit_stream stream)
{
    if (n < 0 || (n && (!src || !dst))) return fail(LDIT_EINVAL, "cast: null operand");
    if (!aligned16(src) || (reinterpret_cast<uintptr_t>(dst) & 7u)) return fail(LDIT_EINVAL, "cast: misaligned operand");
    return launch_cvt_bf16(static_cast<const float *>(src), dst, (size_t)n, static_cast<hipStream_t>(stream));
}

int ldit_linear_fp8(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M, int64_t N,
                    int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, float ab_scale, float out_inv_scale,
                    const void *w_scales, ldit_stream stream)
{
    LDIT_TRY(check_linear("linear_fp8", M, N, K, lda, ldy, Y, Y2, epilogue));
    if (w_scales && !aligned16(w_scales)) return fail(LDIT_EINVAL, "linear_fp8: w_scales must be 16-byte aligned");
    if (!(ab_scale > 0.0f) || (epilogue == LDIT_EPI_BIAS_GELU && !(out_inv_scale > 0.0f))) return fail(LDIT_EINVAL, "linear_fp8: scales must be positive");
    return linear(Build{LDIT_FP8, false}, operand(X, nullptr, lda), W, w_scales, static_cast<const float *>(bias), operand(Y, nullptr, ldy), (int)M,
                  (int)N, (int)K, epilogue, static_cast<const float *>(lam), static_cast<const float *>(R), static_cast<float *>(Y2), Side{},
                  static_cast<hipStream_t>(stream), ab_scale, out_inv_scale);
}

int ldit_quant_rows_f32_fp8(const void *W, void *codes, void *scales, int64_t N, int64_t K, ldit_stream stream)
{
    if (N <= 0 || K <= 0 || N >= (1ll << 31) || K >= (1ll << 31)) return fail(LDIT_EINVAL, "quant_rows_fp8: bad shape");
    if (!codes || (reinterpret_cast<uintptr_t>(codes) & 3u)) return fail(LDIT_EINVAL, "quant_rows_fp8: codes null or misaligned");
    return launch_quant_rows_fp8(static_cast<const float *>(W), codes, static_cast<float *>(scales), (int)N, (int)K,
                                 static_cast<hipStream_t>(stream));
}

int ldit_quant_mx_f32_fp8(const void *src, int64_t lds, void *codes, void *scales, int64_t rows, int64_t K, ldit_stream stream)
{
    if (rows <= 0 || K <= 0 || K >= (1ll << 31) || rows * (lds > K ? lds : K) >= (1ll << 40)) return fail(LDIT_EINVAL, "quant_mx: bad shape");
    if (K % 32 || lds < K || lds % 4) return fail(LDIT_EINVAL, "quant_mx: K %% 32 == 0 and lds >= K, lds %% 4 == 0 required");
    if (!src || !codes || !scales) return fail(LDIT_EINVAL, "quant_mx: null operand");
    if (!aligned16(src) || (reinterpret_cast<uintptr_t>(codes) & 3u)) return fail(LDIT_EINVAL, "quant_mx: misaligned operand");
    return launch_quant_mx(static_cast<const float *>(src), lds, codes, scales, rows, (int)K, 1.0f, static_cast<hipStream_t>(stream));
}

int ldit_linear_mxfp8(const void *X, int64_t lda, const void *Xs, const void *W, const void *Ws, const void *bias, void *Y,
                      int64_t ldy, void *Ys, int64_t M, int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2,
                      ldit_stream stream)
{
    LDIT_TRY(check_linear("linear_mxfp8", M, N, K, lda, ldy, Y, Y2, epilogue));
    if (K % 128 || lda % 128) return fail(LDIT_EUNSUPPORTED, "linear_mxfp8: K and lda must be multiples of 128");
    if (!X || !W || !Xs || !Ws) return fail(LDIT_EINVAL, "linear_mxfp8: null operand");
    if (!aligned16(X) || !aligned16(W) || (reinterpret_cast<uintptr_t>(Xs) & 3u) || (reinterpret_cast<uintptr_t>(Ws) & 3u))
        return fail(LDIT_EINVAL, "linear_mxfp8: codes must be 16-byte aligned, scales 4-byte aligned");
    if (epilogue == LDIT_EPI_BIAS_GELU && (!Ys || N % 32 || ldy % 32))
        return fail(LDIT_EINVAL, "linear_mxfp8: the GELU epilogue writes MX: Ys needed, N and ldy multiples of 32");
    return linear(Build{LDIT_MXFP8, false}, operand(X, Xs, lda), W, Ws, static_cast<const float *>(bias), operand(Y, Ys, ldy), (int)M, (int)N, (int)K,
                  epilogue, static_cast<const float *>(lam), static_cast<const float *>(R), static_cast<float *>(Y2), Side{},
                  static_cast<hipStream_t>(stream));
}

int ldit_layernorm_mxfp8(const void *x, const void *gamma, const void *beta, void *Y, void *Ys, int64_t rows, int64_t C, float eps,
                         ldit_stream stream)
{
    if (C > 4096 || C % 32) return fail(LDIT_EINVAL, "layernorm_mxfp8: C must be a multiple of 32, at most 4096");
    return layernorm(Build{LDIT_MXFP8, false}, static_cast<const float *>(x), static_cast<const float *>(gamma), static_cast<const float *>(beta),
                     operand(Y, Ys, C), nullptr, rows, (int)C, eps, static_cast<hipStream_t>(stream));
}

int ldit_quant_f32_fp8(const void *src, void *dst, int64_t n, float inv_scale, ldit_stream stream)
{
    if (n < 0 || (n && (!src || !dst))) return fail(LDIT_EINVAL, "quant_fp8: null operand");
    if (!aligned16(src) || (reinterpret_cast<uintptr_t>(dst) & 3u)) return fail(LDIT_EINVAL, "quant_fp8: misaligned operand");
    if (!(inv_scale > 0.0f)) return fail(LDIT_EINVAL, "quant_fp8: inv_scale must be positive");
    return launch_quant_fp8(static_cast<const float *>(src), dst, (size_t)n, inv_scale, nullptr, static_cast<hipStream_t>(stream));
}

int ldit_amax_f32(const void *src, int64_t n, void *out, ldit_stream stream)
{
    if (n < 0 || !out || (n && !src)) return fail(LDIT_EINVAL, "amax: null operand");
    return launch_amax_f32(static_cast<const float *>(src), (size_t)n, static_cast<float *>(out), false, static_cast<hipStream_t>(stream));
}

int ldit_preprocess_f32(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t B, int32_t in_ch,
                        float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream)
{
    return preprocess(IMG_F32, images, heights, widths, B, in_ch, mean, std, out_h, out_w, out, stream);
}

int ldit_preprocess_f16(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t B, int32_t in_ch,
                        float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream)
{
    return preprocess(IMG_F16, images, heights, widths, B, in_ch, mean, std, out_h, out_w, out, stream);
}

int ldit_preprocess_u8(const void *const *images, const int32_t *heights, const int32_t *widths, int32_t interleaved, int32_t B,
                       int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream)
{
    ImgFmt fmt;
    LDIT_TRY(u8_format("preprocess_u8", interleaved, fmt));
    return preprocess(fmt, images, heights, widths, B, in_ch, mean, std, out_h, out_w, out, stream);
}

int ldit_preprocess_win_f32(const void *const *images, const int32_t *heights, const int32_t *widths, const int32_t *windows, int32_t B,
                            int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream)
{
    return preprocess_win(IMG_F32, images, heights, widths, windows, B, in_ch, mean, std, out_h, out_w, out, stream);
}

int ldit_preprocess_win_f16(const void *const *images, const int32_t *heights, const int32_t *widths, const int32_t *windows, int32_t B,
                            int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out, ldit_stream stream)
{
    return preprocess_win(IMG_F16, images, heights, widths, windows, B, in_ch, mean, std, out_h, out_w, out, stream);
}

int ldit_preprocess_win_u8(const void *const *images, const int32_t *heights, const int32_t *widths, const int32_t *windows,
                           int32_t interleaved, int32_t B, int32_t in_ch, float mean, float std, int32_t out_h, int32_t out_w, void *out,
                           ldit_stream stream)
{
    ImgFmt fmt;
    LDIT_TRY(u8_format("preprocess_win_u8", interleaved, fmt));
    return preprocess_win(fmt, images, heights, widths, windows, B, in_ch, mean, std, out_h, out_w, out, stream);
}

int ldit_fpn_merge_f32(const void *lat, const void *top, void *out, int64_t B, int64_t Gh, int64_t Gw, int64_t Ch, float scale,
                       int64_t top_h, int64_t top_w, ldit_stream stream)
{
    if (B * (Gh * Gw + 1) * Ch >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "fpn_merge: operand exceeds 2^31 elements");
    return launch_fpn_merge(static_cast<const float *>(lat), static_cast<const float *>(top), static_cast<float *>(out), (int)B,
                            (int)Gh, (int)Gw, (int)Ch, scale, (int)top_h, (int)top_w, static_cast<hipStream_t>(stream));
}

int ldit_conv3x3_nhwc_f32(const void *x, const void *w, const void *bias, void *y, int64_t B, int64_t H, int64_t W, int64_t Cin,
                          int64_t Cout, const void *zeros, ldit_stream stream)
{
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail(LDIT_EINVAL, "conv3x3: empty problem");
    if (B * H * W * (Cin > Cout ? Cin : Cout) >= (1ll << 31) || Cout * 9 * Cin >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "conv3x3: operand exceeds 2^31 elements");
    if (!x || !w || !y || !zeros || !aligned16(x) || !aligned16(w) || !aligned16(y) || !aligned16(zeros)) return fail(LDIT_EINVAL, "conv3x3: null or misaligned operand");
    GemmArgs a{};
    a.A = static_cast<const float *>(x); a.W = static_cast<const float *>(w); a.Y = static_cast<float *>(y);
    a.bias = static_cast<const float *>(bias);
    a.M = (int)(B * H * W); a.N = (int)Cout; a.K = (int)(9 * Cin); a.lda = (int)Cin; a.ldy = (int)Cout;
    a.conv_h = (int)H; a.conv_w = (int)W; a.conv_c = (int)Cin; a.zeros = static_cast<const float *>(zeros);
    return launch_gemm(a, EPI_BIAS, A_CONV3, static_cast<hipStream_t>(stream));
}

int ldit_conv3x3_nhwc_bf16(const void *xpad, const void *w, const void *bias, void *y, int64_t ldy, int64_t B, int64_t H, int64_t W,
                           int64_t Cin, int64_t Cout, int32_t epilogue, ldit_stream stream)
{
    int epi;
    switch (epilogue) {
        case LDIT_EPI_F32: epi = EPI_F32; break;
        case LDIT_EPI_BIAS: epi = EPI_BIAS; break;
        case LDIT_EPI_BIAS_RELU: epi = EPI_BIAS_RELU; break;
        default: return fail(LDIT_EINVAL, "conv3x3_bf16: unknown epilogue %d", epilogue);
    }
    return launch_conv3x3_bf16(xpad, w, static_cast<const float *>(bias), y, ldy, B, H, W, Cin, Cout, epi, static_cast<hipStream_t>(stream));
}

int ldit_fpn_merge_bwd_f32(const void *d_inner, void *d_lat, void *d_top, int64_t B, int64_t Gh, int64_t Gw, int64_t Ch, float scale,
                           int64_t top_h, int64_t top_w, ldit_stream stream)
{
    if (B * (Gh * Gw + 1) * Ch >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "fpn_merge_bwd: operand exceeds 2^31 elements");
    return launch_fpn_merge_bwd(static_cast<const float *>(d_inner), static_cast<float *>(d_lat), static_cast<float *>(d_top), (int)B,
                                (int)Gh, (int)Gw, (int)Ch, scale, (int)top_h, (int)top_w, static_cast<hipStream_t>(stream));
}

int ldit_pad_nhwc_f32_bf16(const void *src, void *dst, int64_t B, int64_t H, int64_t W, int64_t C, ldit_stream stream)
{
    if (B * (H + 2) * (W + 2) * C >= (1ll << 33)) return fail(LDIT_EUNSUPPORTED, "pad_nhwc: operand too large");
    return launch_pad_nhwc_bf16(static_cast<const float *>(src), dst, (int)B, (int)H, (int)W, (int)C, static_cast<hipStream_t>(stream));
}

size_t ldit_colsum_scratch_bytes(int64_t M, int64_t N) { return (M > 0 && N > 0) ? colsum_scratch_bytes(M, N) : 0; }

int ldit_colsum_f32(const void *x, int64_t M, int64_t N, int64_t ldx, void *out, void *scratch, size_t scratch_bytes, ldit_stream stream)
{
    if (N >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "colsum: too many columns");
    return launch_colsum_f32(static_cast<const float *>(x), M, (int)N, ldx, static_cast<float *>(out), static_cast<float *>(scratch),
                             scratch_bytes, false, static_cast<hipStream_t>(stream));
}

int ldit_colamax_f32(const void *x, int64_t M, int64_t N, int64_t ldx, void *out, void *scratch, size_t scratch_bytes, ldit_stream stream)
{
    if (N >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "colamax: too many columns");
    return launch_colsum_f32(static_cast<const float *>(x), M, (int)N, ldx, static_cast<float *>(out), static_cast<float *>(scratch),
                             scratch_bytes, true, static_cast<hipStream_t>(stream));
}

int ldit_relu_bwd_bf16(const void *dy, int64_t lddy, const void *act, int64_t ldact, void *out, int64_t ldout, int64_t M, int64_t N,
                       void *colsum, void *scratch, size_t scratch_bytes, ldit_stream stream)
{
    return launch_relu_bwd_bf16(static_cast<const float *>(dy), lddy, static_cast<const float *>(act), ldact, out, ldout, M, N,
                                static_cast<float *>(colsum), static_cast<float *>(scratch), scratch_bytes, static_cast<hipStream_t>(stream));
}

int ldit_relu_bwd_pad_nhwc_bf16(const void *dy, const void *act, void *out, int64_t B, int64_t H, int64_t W, int64_t C, void *colsum,
                                void *scratch, size_t scratch_bytes, ldit_stream stream)
{
    return launch_relu_bwd_pad_nhwc_bf16(static_cast<const float *>(dy), static_cast<const float *>(act), out, B, H, W, C,
                                         static_cast<float *>(colsum), static_cast<float *>(scratch), scratch_bytes,
                                         static_cast<hipStream_t>(stream));
}

int ldit_relu_bwd_bf16_act16(const void *dy, int64_t lddy, const void *act, int64_t ldact, void *out, int64_t ldout, int64_t M, int64_t N,
                             void *colsum, void *scratch, size_t scratch_bytes, ldit_stream stream)
{
    return launch_relu_bwd_bf16_act16(static_cast<const float *>(dy), lddy, act, ldact, out, ldout, M, N, static_cast<float *>(colsum),
                                      static_cast<float *>(scratch), scratch_bytes, static_cast<hipStream_t>(stream));
}

int ldit_relu_bwd_pad_nhwc_bf16_act16(const void *dy, const void *act, void *out, int64_t B, int64_t H, int64_t W, int64_t C, void *colsum,
                                      void *scratch, size_t scratch_bytes, ldit_stream stream)
{
    return launch_relu_bwd_pad_nhwc_bf16_act16(static_cast<const float *>(dy), act, out, B, H, W, C, static_cast<float *>(colsum),
                                               static_cast<float *>(scratch), scratch_bytes, static_cast<hipStream_t>(stream));
}

int ldit_cast_f16_f32(const void *src, void *dst, int64_t n, ldit_stream stream)
{
    if (n < 0 || (n && (!src || !dst))) return fail(LDIT_EINVAL, "cast: null operand");
    if ((reinterpret_cast<uintptr_t>(src) & 7u) || !aligned16(dst)) return fail(LDIT_EINVAL, "cast: misaligned operand");
    return launch_cast_f16(src, dst, (size_t)n, true, static_cast<hipStream_t>(stream));
}

int ldit_cast_f32_f16(const void *src, void *dst, int64_t n, ldit_stream stream)
{
    if (n < 0 || (n && (!src || !dst))) return fail(LDIT_EINVAL, "cast: null operand");
    if (!aligned16(src) || (reinterpret_cast<uintptr_t>(dst) & 7u)) return fail(LDIT_EINVAL, "cast: misaligned operand");
    return launch_cast_f16(src, dst, (size_t)n, false, static_cast<hipStream_t>(stream));
}

}  // extern "C"
