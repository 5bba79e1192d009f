// C-ABI entry points of the train step (BASELINE.json configs[2]: ViT-B/16 bs=64 bf16 forward + backward + AdamW;
// SURVEY.md 8(f)-3; reference loop: ref src/layoutdit/training/trainer.py:148-187, optimizer :62-76).  Host-side sequencing
// only, same rules as api.hip: enqueue-only on the caller's stream, no allocation, no CPU fallback.
//
// What is differentiated: hs = self.dit(x).hidden_states (ref dit_backbone.py:47) with respect to every encoder parameter,
// for upstream gradients arriving at the tapped hidden states.  bf16 build only: GEMM / attention operands bf16, residual
// stream, LayerNorm statistics, softmax, all accumulation and every gradient that leaves the library fp32.
//
// Parameters, gradients and optimizer state are FLAT fp32 blocks in the layout of the fp32 packed block (packed_map(F32)):
// patch_w, patch_b, cls, pos, then per layer ln1_w, ln1_b, wqkv [3C,C], bqkv [3C] (the key third stays zero: BEiT has no
// key bias, TF:306), wo, bo, lam1, ln2_w, ln2_b, w1, b1, w2, b2, lam2.  ldit_flat_param_layout reports the offsets; the
// PyTorch mirror makes its nn.Parameters views of that block (layoutdit_amd/training.py).
//
// Backward of one layer = 8 MFMA GEMMs (2x the forward's FLOPs) on gemm_bf16_tr.hip, which reads reduction-major operands
// through transposing LDS reads - nothing is transposed in memory:
//   dgrad  dX[M,K] = dY[M,N] . W[N,K]      A = dY (K-contiguous), B = W exactly as nn.Linear stores it ([reduction N][K])
//   wgrad  dW[N,K] = dY^T . X              both operands [reduction = tokens][outputs], as the forward / the dgrad left them;
//                                          K = B*N tokens is split over workgroups, fp32 slabs summed in a fixed order
// plus attention backward (attention_bwd_bf16.hip), LayerScale / LayerNorm backward with two-stage column reductions
// (train_ops.hip).  Nothing uses atomics: gradients are bit-reproducible.
#include "api_internal.h"

namespace ldit {
namespace {

// mxfp8 build (quantisation-aware training, ldit.h): y1, y2, g hold the DEQUANTISED MX operands Q(.) the forward multiplied (bf16,
// exact), o the bf16 attention output before quantisation (attention backward) and od its dequantised codes (o_proj wgrad);
// mx_c / mx_f are the forward's transient MX operands (codes [M, C] / [M, F], then their scales [M, C / 32] / [M, F / 32]).
struct SavedLayer { size_t h_in, y1, qkv, lse, o, z1, h_mid, y2, a1, g, z2, od; };
struct SavedMap {
    std::vector<SavedLayer> layer;
    size_t rowscale, h_final, total;
    size_t patches;    // bf16 im2col of the batch [B P, 3 p p]: operand of the patch-embedding GEMM (forward) and of its wgrad
    size_t mx_c = 0, mx_f = 0;
};

inline int pad64(int v) { return (v + 63) / 64 * 64; }

SavedMap saved_map(const Geo &g, int batch, int dtype)
{
    SavedMap m;
    const size_t M = (size_t)batch * g.T, C = g.C, F = g.F;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += up(bytes, 256); return at; };
    m.layer.resize(g.L);
    for (int l = 0; l < g.L; ++l) {
        SavedLayer &s = m.layer[l];
        s.h_in = take(M * C * 4);
        s.y1 = take(M * C * 2);
        s.qkv = take(M * 3 * C * 2);
        s.lse = take((size_t)batch * g.H * g.T * 4);
        s.o = take(M * C * 2);
        s.z1 = take(M * C * 2);
        s.h_mid = take(M * C * 4);
        s.y2 = take(M * C * 2);
        s.a1 = take(M * F * 2);
        s.g = take(M * F * 2);
        s.z2 = take(M * C * 2);
        s.od = dtype == LDIT_MXFP8 ? take(M * C * 2) : s.o;
    }
    m.rowscale = take((size_t)2 * (g.L > 0 ? g.L : 1) * M * 4);
    m.h_final = take(M * C * 4);
    m.patches = take((size_t)batch * g.P * g.Kp * 2);
    if (dtype == LDIT_MXFP8) {
        m.mx_c = take(M * C + M * C / 32);
        m.mx_f = take(M * F + M * F / 32);
    }
    m.total = o;
    return m;
}

constexpr int MAX_SPLITS = 8;

// K-splits of a wgrad GEMM with an Mout x Nout output over `nk` k-tiles.  The output is a handful of tiles and K = all
// tokens of the batch, so K is cut until one round of the machine is full: 128 x 128 tiles run two per CU (512 slots).
// Every split costs one more fp32 slab to write and to sum, hence as few as fill that round, at most 8.
int pick_splits(int Mout, int Nout, int nk)
{
    // (Round 4, scripts/wgrad_tiles.py: timed alone, GEMM + slab sum, the eight-wave 256 x 256 tile with K cut six to eight ways
    // wins - W2 / W1 [768 x 3072] 81.8 -> 71.4 us.  Inside the train step it loses: twice the slabs are twice the fp32 traffic of
    // the reduction, which there runs from HBM - per layer wgrad 238 -> 223 us but slab sums 28 -> 53 us, whether they are
    // queued or issued right behind their GEMM (profiles/r04_wgrad_tiles.txt).  Few splits on the small tile stay.)
    const long tiles = (long)((Mout + 127) / 128) * ((Nout + 127) / 128);
    int s = (int)(512 / tiles);
    if (s > MAX_SPLITS) s = MAX_SPLITS;
    if (s > nk) s = nk;
    if (s < 1) s = 1;
    while (s > 1 && ((nk + s - 1) / s) * (s - 1) >= nk) --s;      // no empty slab
    return s;
}

struct TrainWs {
    size_t zeros, dh, dy, dz, da1, dob, dqkv, patches;
    size_t slab[4];                 // wgrad slabs: w2 / patch_w, w1, wo, wqkv
    size_t part[10];                // partial column sums, see backward()
    size_t part_rows_tile, part_rows_ln;
    size_t total;
};

TrainWs train_ws_map(const Geo &g, int batch)
{
    TrainWs w;
    const size_t M = (size_t)batch * g.T, C = g.C, F = g.F, Mp = pad64((int)M);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += up(bytes, 256); return at; };
    w.zeros = take(256);                                  // zero page: reduction rows past the last token
    w.dh = take(M * C * 4);
    w.dy = take(M * C * 4);
    w.dz = take(M * C * 2);
    w.da1 = take(M * F * 2);
    w.dob = take(M * C * 2);
    w.dqkv = take(M * 3 * C * 2);
    w.patches = take((size_t)batch * g.P * g.Kp * 2);     // im2col of the batch, bf16 (patch-embedding wgrad)
    const size_t S = MAX_SPLITS;
    w.slab[0] = take(S * std::max(C * F, C * (size_t)g.Kp) * 4);
    w.slab[1] = take(S * F * C * 4);
    w.slab[2] = take(S * C * C * 4);
    w.slab[3] = take(S * 3 * C * C * 4);
    w.part_rows_tile = Mp / 64;
    w.part_rows_ln = (size_t)layernorm_bwd_blocks((int64_t)M);
    const size_t widths[10] = {C, C, F, C, C, C, C, 3 * C, C, C};
    const size_t part_rows = std::max(std::max(w.part_rows_ln, w.part_rows_tile), (size_t)layernorm_bwd_resid_blocks((int64_t)M));     // every buffer fits any producer
    for (int i = 0; i < 10; ++i) w.part[i] = take(part_rows * widths[i] * 4);
    w.total = o;
    return w;
}

int train_geometry(const ldit_cfg *cfg, Geo &g)
{
    if (cfg && cfg->dtype != LDIT_BF16 && cfg->dtype != LDIT_MXFP8)
        return fail(LDIT_EUNSUPPORTED, "train step: only the bf16 (LDIT_BF16) and mxfp8 (LDIT_MXFP8, quantisation-aware) builds are implemented");
    LDIT_TRY(geometry(cfg, g));     // (mxfp8: hidden and mlp multiples of 128)
    return LDIT_OK;
}

// Train mirror (ldit_train_mirror_bytes): the bf16 part - element i of the flat block at byte 2 i (bf16 of the master; in the mxfp8
// build the four matrices of a layer hold their dequantised MX codes instead, the q third folded) - then, mxfp8 only, at byte
// mirror_mx_offset the MX section laid out as packed_map(g, LDIT_MXFP8): the matrices' codes and scales and the folded q|k|v bias.
inline size_t mirror_mx_offset(const Geo &g) { return up(packed_map(g, LDIT_F32).total / 2, 256); }
inline size_t mirror_bytes(const Geo &g, int dtype)
{
    return dtype == LDIT_MXFP8 ? mirror_mx_offset(g) + packed_map(g, LDIT_MXFP8).total : packed_map(g, LDIT_F32).total / 2;
}

// the four matrices of a layer: where they start in the flat block (elements), their shape and the rows the q fold covers, and where
// their codes and scales go in the MX section (bytes)
inline void mx_layer_segs(const PackedLayer &f, const PackedLayer &x, int64_t C, int64_t F, MxRequantSeg *segs)
{
    segs[0] = {(int64_t)(f.wqkv / 4), 3 * C * C, (int)C, (int)C, (int64_t)x.wqkv, (int64_t)x.sw_qkv};
    segs[1] = {(int64_t)(f.wo / 4), C * C, (int)C, 0, (int64_t)x.wo, (int64_t)x.sw_o};
    segs[2] = {(int64_t)(f.w1 / 4), F * C, (int)C, 0, (int64_t)x.w1, (int64_t)x.sw_1};
    segs[3] = {(int64_t)(f.w2 / 4), C * F, (int)F, 0, (int64_t)x.w2, (int64_t)x.sw_2};
}

// The MX part of the mirror from the flat block: the matrices and the fused bias of ALL layers in one launch, nothing else of the
// mirror written - the bf16 part is the caller's launch before (ldit_pack_train: the convert pass, ldit_adamw_step_mxfp8: adamw_kernel,
// ldit_requant_train_mirror: the multi-tensor AdamW).  The layer comes from the grid, so every layer must be layer 0 moved by one stride
// in the flat block and one in the MX section: packed_map lays equal layers out one after another, which is checked here rather than
// assumed.  (mxfp8 geometries have hidden and mlp multiples of 128: every matrix is whole 16 384-element pieces, far inside
// launch_requant_mirror's 1024-element rule.)
int mx_requant_all_layers(const Geo &g, const float *p, void *mirror, const ldit_opt_state *state, hipStream_t stream)
{
    if (g.L == 0) return LDIT_OK;
    const PackedMap fm = packed_map(g, LDIT_F32), xm = packed_map(g, LDIT_MXFP8);
    const PackedLayer &f0 = fm.layer[0], &x0 = xm.layer[0];
    const size_t fs = g.L > 1 ? fm.layer[1].ln1_w - f0.ln1_w : 0, xs = g.L > 1 ? xm.layer[1].ln1_w - x0.ln1_w : 0;
    for (int l = 1; l < g.L; ++l) {
        const PackedLayer &f = fm.layer[l], &x = xm.layer[l];
        const size_t fo = (size_t)l * fs, xo = (size_t)l * xs;
        const bool flat = f.wqkv == f0.wqkv + fo && f.bqkv == f0.bqkv + fo && f.wo == f0.wo + fo && f.w1 == f0.w1 + fo && f.w2 == f0.w2 + fo;
        const bool mx = x.wqkv == x0.wqkv + xo && x.bqkv == x0.bqkv + xo && x.wo == x0.wo + xo && x.w1 == x0.w1 + xo && x.w2 == x0.w2 + xo &&
                        x.sw_qkv == x0.sw_qkv + xo && x.sw_o == x0.sw_o + xo && x.sw_1 == x0.sw_1 + xo && x.sw_2 == x0.sw_2 + xo;
        if (!flat || !mx) return fail(LDIT_EUNSUPPORTED, "requant_train_mirror: layer %d is not layer 0 moved by a whole stride", l);
    }
    if (fs % 16) return fail(LDIT_EUNSUPPORTED, "requant_train_mirror: layer stride %zu is not a multiple of 16 bytes", fs);
    MxRequantSeg segs[4];
    mx_layer_segs(f0, x0, g.C, g.F, segs);
    return launch_requant_mirror(p, mirror, static_cast<char *>(mirror) + mirror_mx_offset(g), state, segs, (int64_t)(fs / 4), (int64_t)xs,
                                 (int64_t)(f0.bqkv / 4), (int64_t)x0.bqkv, g.C, g.L, qfold_of(g), stream);
}

int forward_train(const ldit_cfg *cfg, const void *packed, const void *flat_params, const void *x, int32_t batch,
                  void *const *tap_out, const void *drop_scales, void *saved, size_t saved_bytes, hipStream_t stream, Probe &probe)
{
    Geo g;
    LDIT_TRY(train_geometry(cfg, g));
    LDIT_TRY(check_forward_args(cfg, g, batch, {packed, flat_params, x, saved}, "packed / flat_params / x / saved", nullptr, tap_out));
    const SavedMap sm = saved_map(g, batch, cfg->dtype);
    if (saved_bytes < sm.total) return fail(LDIT_EWORKSPACE, "saved-activation block %zu bytes < required %zu", saved_bytes, sm.total);
    // `packed` is the bf16 MIRROR of the flat fp32 block (element i of the mirror = bf16 of element i of the master): a matrix
    // sits at half its fp32 byte offset.  Every fp32 vector (and the fp32 patch projection) is read from the master itself.
    const PackedMap pm = packed_map(g, LDIT_F32);
    const char *P = static_cast<const char *>(packed), *FP = static_cast<const char *>(flat_params);
    auto F32 = [&](size_t off) { return reinterpret_cast<const float *>(FP + off); };
    char *S = static_cast<char *>(saved);
    const int M = batch * g.T, C = g.C, F = g.F;
    const size_t act_bytes = (size_t)M * C * 4;
    float *rowscale = drop_scales ? reinterpret_cast<float *>(S + sm.rowscale) : nullptr;
    if (drop_scales && g.L)
        LDIT_RUN(probe, LDIT_K_OTHER, launch_expand_rowscale(static_cast<const float *>(drop_scales), rowscale, batch, g.T, 2 * g.L, stream));
    auto h_of = [&](int l) { return reinterpret_cast<float *>(S + (l < g.L ? sm.layer[l].h_in : sm.h_final)); };

    // embeddings (TF:153-176): the batch rounded to a bf16 im2col matrix (kept in the saved block: the wgrad's operand too), then
    // the bf16 MFMA GEMM on the mirror of the patch projection - mixed precision like every other GEMM of the step (the fp32
    // kernel took 161 us of a 13.4 ms ViT-B bs=64 step).  A patch length that is not a multiple of the bf16 k-tile stays fp32.
    if (g.Kp % 64 == 0)
        LDIT_TRY(embed_bf16(g, static_cast<const float *>(x), nullptr, 1, S + sm.patches, P + pm.patch_w / 2, F32(pm.patch_b), F32(pm.cls),
                            F32(pm.pos), h_of(0), batch, cfg->img_h, cfg->img_w, stream, probe));
    else
        LDIT_TRY(embed(g, static_cast<const float *>(x), F32(pm.patch_w), F32(pm.patch_b), F32(pm.cls), F32(pm.pos), h_of(0), batch, cfg->img_h,
                       cfg->img_w, stream, probe));
    LDIT_TRY(copy_taps(cfg, tap_out, 0, h_of(0), nullptr, act_bytes, stream));

    // Every tensor of a layer in its own slot of the saved block.  bf16: the operands are the saved tensors themselves.  mxfp8
    // (quantisation-aware training): the inference forward of the mxfp8 build on the mirror's MX section, its transient MX operands in
    // mx_c / mx_f; the train variants of its kernels add side stores only - the dequantised MX operands, the pre-quantisation
    // attention output, lse, the pre-LayerScale branch outputs, gelu' - and the stochastic-depth row factors.
    const bool mx = cfg->dtype == LDIT_MXFP8;
    const PackedMap xm = mx ? packed_map(g, LDIT_MXFP8) : PackedMap{};
    const char *X = P + mirror_mx_offset(g);
    char *y8 = S + sm.mx_c, *b8 = S + sm.mx_f;
    Layer d{};
    d.qk_bytes = (size_t)2 * C;
    d.V = FP; d.W = mx ? X : P; d.div = mx ? 1 : 2;
    d.scale = mx ? 0.0f /* q folded */ : 1.0f / sqrtf((float)g.D);
    for (int l = 0; l < g.L; ++l) {
        const SavedLayer &sl = sm.layer[l];
        d.h_in = h_of(l); d.h_mid = reinterpret_cast<float *>(S + sl.h_mid); d.h_out = h_of(l + 1);
        d.v = &pm.layer[l]; d.w = mx ? &xm.layer[l] : d.v;
        d.bqkv = mx ? reinterpret_cast<const float *>(X + d.w->bqkv) /* folded */ : F32(d.v->bqkv);
        d.qkv = operand(S + sl.qkv, nullptr, 3 * C);
        d.lse = reinterpret_cast<float *>(S + sl.lse);
        d.s_o.Ypre = S + sl.z1; d.s_o.rowscale = rowscale ? rowscale + (size_t)(2 * l) * M : nullptr;
        d.s_fc1.Ypre = S + sl.a1;                       // gelu'(pre-activation), the backward's factor
        d.s_fc2.Ypre = S + sl.z2; d.s_fc2.rowscale = rowscale ? rowscale + (size_t)(2 * l + 1) * M : nullptr;
        if (mx) {
            d.y1 = d.o = d.y2 = operand(y8, y8 + (size_t)M * C, C);
            d.hid = operand(b8, b8 + (size_t)M * F, F);
            d.y1d = S + sl.y1; d.ob = S + sl.o; d.od = S + sl.od; d.y2d = S + sl.y2; d.s_fc1.Yd = S + sl.g;
        } else {
            d.y1 = operand(S + sl.y1, nullptr, C); d.o = operand(S + sl.o, nullptr, C); d.y2 = operand(S + sl.y2, nullptr, C);
            d.hid = operand(S + sl.g, nullptr, F);
        }
        d.tap = tap_of(cfg, tap_out, l + 1);
        LDIT_TRY(run_layer(Build{cfg->dtype, true}, g, batch, cfg->ln_eps, d, stream, probe));
        if (d.tap) LDIT_TRY(copy_taps(cfg, tap_out, l + 1, d.h_out, d.tap, act_bytes, stream));
    }
    return LDIT_OK;
}

// one wgrad:  out[Nout, Kout] = dY[tokens, Nout]^T . X[tokens, Kout], both operands as they lie in memory; split-K slabs
int wgrad(Probe &probe, ReduceJobs &jobs, const void *dY, int ld_dy, const void *X, int ld_x, float *out, float *slab, int Nout,
          int Kout, int tokens, const void *zeros, hipStream_t stream)
{
    GemmExtra x{};
    x.zeros = zeros;
    x.splits = pick_splits(Nout, Kout, (tokens + 63) / 64);
    float *dst = x.splits == 1 ? out : slab;
    LDIT_RUN(probe, LDIT_K_GEMM, launch_gemm_bf16_tr(dY, ld_dy, true, X, ld_x, nullptr, dst, Kout, Nout, Kout, tokens, EPI_F32, x, stream));
    if (x.splits > 1) {
        if (jobs.full()) LDIT_RUN(probe, LDIT_K_OTHER, launch_reduce_jobs(jobs, stream));
        jobs.add(slab, out, (int64_t)Nout * Kout, x.splits, (int64_t)Nout * Kout);
    }
    return LDIT_OK;
}

// one dgrad:  dX[M, Kout] = epi( dY[M, Nred] . W[Nred, Kout] ), W the bf16 copy of the nn.Linear weight as stored
int dgrad(Probe &probe, const void *dY, int Nred, const void *W, void *dX, int M, int Kout, int epi, const void *aux, const void *zeros,
          hipStream_t stream, float *colsum = nullptr)
{
    GemmExtra x{};
    x.zeros = zeros; x.aux = aux; x.ldaux = Kout; x.colsum = colsum;
    LDIT_RUN(probe, LDIT_K_GEMM, launch_gemm_bf16_tr(dY, Nred, false, W, Kout, nullptr, dX, Kout, M, Kout, Nred, epi, x, stream));
    return LDIT_OK;
}

int backward(const ldit_cfg *cfg, const void *flat_params, const void *packed, const void *x, int32_t batch, void *const *dtaps,
             const void *drop_scales, const void *saved, size_t saved_bytes, void *grads, size_t grads_bytes, void *workspace, size_t ws_bytes,
             int stage_hi, int stage_lo, hipStream_t stream, Probe &probe)
{
    Geo g;
    LDIT_TRY(train_geometry(cfg, g));
    if (batch <= 0) return fail(LDIT_EINVAL, "batch %d must be positive", batch);
    if (!flat_params || !packed || !x || !saved || !grads || !workspace) return fail(LDIT_EINVAL, "backward: null pointer");
    if (!aligned16(flat_params) || !aligned16(packed) || !aligned16(x) || !aligned16(saved) || !aligned16(grads) || !aligned16(workspace))
        return fail(LDIT_EINVAL, "backward: pointers must be 16-byte aligned");
    if (stage_hi > g.L || stage_lo < 0 || stage_lo > stage_hi) return fail(LDIT_EINVAL, "backward: stages [%d, %d] outside [0, %d]", stage_lo, stage_hi, g.L);
    const SavedMap sm = saved_map(g, batch, cfg->dtype);
    if (saved_bytes < sm.total) return fail(LDIT_EWORKSPACE, "saved-activation block %zu bytes < required %zu", saved_bytes, sm.total);
    const TrainWs wm = train_ws_map(g, batch);
    if (ws_bytes < wm.total) return fail(LDIT_EWORKSPACE, "workspace %zu bytes < required %zu", ws_bytes, wm.total);
    const PackedMap gm = packed_map(g, LDIT_F32), &pm = gm;      // vectors are read from the flat fp32 master
    if (grads_bytes < gm.total) return fail(LDIT_EWORKSPACE, "gradient block %zu bytes < required %zu", grads_bytes, gm.total);
    for (int i = 0; dtaps && i < cfg->n_taps; ++i)
        if (dtaps[i] && !aligned16(dtaps[i])) return fail(LDIT_EINVAL, "backward: dtaps[%d] misaligned", i);

    const char *P = static_cast<const char *>(flat_params), *W16 = static_cast<const char *>(packed), *S = static_cast<const char *>(saved);
    char *G = static_cast<char *>(grads), *ws = static_cast<char *>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<const float *>(P + off); };
    auto GR = [&](size_t off) { return reinterpret_cast<float *>(G + off); };
    auto PART = [&](int i) { return reinterpret_cast<float *>(ws + wm.part[i]); };
    const int M = batch * g.T, C = g.C, F = g.F, Mp = pad64(M);
    const size_t act = (size_t)M * C;
    float *dh = reinterpret_cast<float *>(ws + wm.dh), *dy = reinterpret_cast<float *>(ws + wm.dy);
    char *dz = ws + wm.dz, *da1 = ws + wm.da1, *dob = ws + wm.dob, *dqkv = ws + wm.dqkv;
    const char *zeros = ws + wm.zeros;
    LDIT_HIP_CHECK(hipMemsetAsync(ws + wm.zeros, 0, 256, stream));
    // stochastic depth: the forward left the per-row factors (expanded from drop_scales) in the saved block
    const float *rowscale = drop_scales ? reinterpret_cast<const float *>(S + sm.rowscale) : nullptr;
    // mxfp8 (straight-through backward): the forward's q was folded, q' = qfold q, and its scores are exp2-domain exponents - the
    // attention backward runs in that convention (scale ln 2: c = scale log2 e = 1), and the q rows / q bias of the fused
    // gradient come out per folded parameter: times qfold afterwards (chain rule of W_q' = qfold W_q, b_q' = qfold b_q)
    const bool mx = cfg->dtype == LDIT_MXFP8;
    const float scale = mx ? 0.693147180559945309f : 1.0f / sqrtf((float)g.D);
    const int rows_tile = (int)wm.part_rows_tile, rows_ln = (int)wm.part_rows_ln;
    const int rows_lnr = C <= 1024 ? layernorm_bwd_resid_blocks((int64_t)M) : rows_ln;     // partial rows of the fused LayerNorm + LayerScale backward
    ReduceJobs jobs;

    // Upstream gradient arriving at hidden state `st` (dtaps).  For the last hidden state it IS dh's first value (a copy; anything
    // more is added); for every other state it rides in the LayerNorm backward that completes dh for that state - layer st's
    // layernorm_before, the last kernel of iteration st + 1, in this call or the previous stage's - so dh makes no extra round trip.
    // (Stages run L .. 0 in order on one workspace: dh itself already travels from call to call.)
    auto tap_grads = [&](int st, const float *(&found)[8]) {
        int n = 0;
        for (int i = 0; dtaps && i < cfg->n_taps && n < 8; ++i)
            if (cfg->taps[i] == st && dtaps[i]) found[n++] = static_cast<const float *>(dtaps[i]);
        return n;
    };
    if (stage_hi == g.L) {
        const float *t[8];
        const int n = tap_grads(g.L, t);
        if (n == 0) LDIT_HIP_CHECK(hipMemsetAsync(dh, 0, act * 4, stream));
        else LDIT_HIP_CHECK(hipMemcpyAsync(dh, t[0], act * 4, hipMemcpyDeviceToDevice, stream));
        for (int i = 1; i < n; ++i) LDIT_RUN(probe, LDIT_K_OTHER, launch_add_inplace(dh, t[i], act, stream));
    }
    for (int st = stage_hi; st >= stage_lo; --st) {
        if (st == 0) break;
        const int l = st - 1;
        const PackedLayer &pl = pm.layer[l], &gl = gm.layer[l];
        const SavedLayer &sl = sm.layer[l];
        const float *rs1 = rowscale ? rowscale + (size_t)(2 * l) * M : nullptr, *rs2 = rowscale ? rowscale + (size_t)(2 * l + 1) * M : nullptr;

        // ---- MLP branch:  h_out = h_mid + rs2 lam2 (.) (gelu(y2 W1^T + b1) W2^T + b2) --------------------------------
        LDIT_RUN(probe, LDIT_K_OTHER, launch_resid_bwd(dh, S + sl.z2, F32(pl.lam2), rs2, dz, nullptr, M, C, Mp, PART(0), PART(1), stream));
        LDIT_TRY(wgrad(probe, jobs, dz, C, S + sl.g, F, GR(gl.w2), reinterpret_cast<float *>(ws + wm.slab[0]), C, F, M, zeros, stream));
        // da1 = (dz W2) (.) gelu'; its column sums (the fc1 bias gradient) leave the same epilogue (F a multiple of 256), else a pass
        const bool b1_fused = F % 256 == 0;
        LDIT_TRY(dgrad(probe, dz, C, W16 + gl.w2 / 2, da1, M, F, EPI_GELU_BWD, S + sl.a1, zeros, stream, b1_fused ? PART(2) : nullptr));
        if (!b1_fused) LDIT_RUN(probe, LDIT_K_OTHER, launch_colsum_bf16(da1, M, F, F, PART(2), stream));
        LDIT_TRY(wgrad(probe, jobs, da1, F, S + sl.y2, C, GR(gl.w1), reinterpret_cast<float *>(ws + wm.slab[1]), F, C, M, zeros, stream));
        LDIT_TRY(dgrad(probe, da1, F, W16 + gl.w1 / 2, dy, M, C, EPI_F32, nullptr, zeros, stream));
        // ---- attention branch:  h_mid = h_in + rs1 lam1 (.) (attn(LN1(h_in)) Wo^T + bo) --------------------------------
        // its LayerScale / residual backward rides in the LayerNorm backward that produces dh (h_mid): one pass, dh read once
        LDIT_RUN(probe, LDIT_K_LAYERNORM, launch_layernorm_bwd_resid(dy, reinterpret_cast<const float *>(S + sl.h_mid), F32(pl.ln2_w), dh, M, C,
                                                                    cfg->ln_eps, PART(3), PART(4), S + sl.z1, F32(pl.lam1), rs1, dz, PART(5),
                                                                    PART(6), stream));
        LDIT_TRY(wgrad(probe, jobs, dz, C, S + sl.od, C, GR(gl.wo), reinterpret_cast<float *>(ws + wm.slab[2]), C, C, M, zeros, stream));
        LDIT_TRY(dgrad(probe, dz, C, W16 + gl.wo / 2, dob, M, C, EPI_BIAS, nullptr, zeros, stream));
        {
            const char *qkv = S + sl.qkv;
            LDIT_RUN(probe, LDIT_K_ATTENTION,
                     launch_attention_bwd_bf16(qkv, qkv + 2 * (size_t)C, qkv + 4 * (size_t)C, S + sl.o, dob,
                                               reinterpret_cast<const float *>(S + sl.lse), dqkv, dqkv + 2 * (size_t)C,
                                               dqkv + 4 * (size_t)C, batch, g.T, g.H, g.D, 3 * C, C, C, 3 * C, scale, stream));
        }
        LDIT_RUN(probe, LDIT_K_OTHER, launch_colsum_bf16(dqkv, M, 3 * C, 3 * C, PART(7), stream));
        LDIT_TRY(wgrad(probe, jobs, dqkv, 3 * C, S + sl.y1, C, GR(gl.wqkv), reinterpret_cast<float *>(ws + wm.slab[3]), 3 * C, C, M, zeros, stream));
        LDIT_TRY(dgrad(probe, dqkv, 3 * C, W16 + gl.wqkv / 2, dy, M, C, EPI_F32, nullptr, zeros, stream));
        {
            // dh becomes the gradient at hidden state st - 1: that state's tap gradient (if any) is summed in the same pass
            const float *t[8];
            const int n = tap_grads(st - 1, t);
            LDIT_RUN(probe, LDIT_K_LAYERNORM, launch_layernorm_bwd(dy, reinterpret_cast<const float *>(S + sl.h_in), F32(pl.ln1_w), dh, M, C,
                                                                  cfg->ln_eps, PART(8), PART(9), stream, n ? t[0] : nullptr));
            for (int i = 1; i < n; ++i) LDIT_RUN(probe, LDIT_K_OTHER, launch_add_inplace(dh, t[i], act, stream));
        }
        // ---- second stage of this layer's reductions: 4 wgrad slab sums (queued above) + 10 vectors, one launch ----------
        if (jobs.n + 12 > 16) LDIT_RUN(probe, LDIT_K_OTHER, launch_reduce_jobs(jobs, stream));
        jobs.add(PART(0), GR(gl.lam2), C, rows_tile, C);
        jobs.add(PART(1), GR(gl.b2), C, rows_tile, C);
        jobs.add(PART(2), GR(gl.b1), F, F % 256 == 0 ? gemm_bf16_tr_colsum_rows(M, F) : rows_tile, F);
        jobs.add(PART(3), GR(gl.ln2_w), C, rows_lnr, C);
        jobs.add(PART(4), GR(gl.ln2_b), C, rows_lnr, C);
        jobs.add(PART(5), GR(gl.lam1), C, rows_lnr, C);
        jobs.add(PART(6), GR(gl.bo), C, rows_lnr, C);
        // q | k | v bias gradient: BEiT has no key bias (TF:306) - its slot in the fused vector is written as a sum of ZERO partial rows
        jobs.add(PART(7), GR(gl.bqkv), C, rows_tile, 3 * C);
        jobs.add(PART(7), GR(gl.bqkv) + C, C, 0, 3 * C);
        jobs.add(PART(7) + 2 * C, GR(gl.bqkv) + 2 * C, C, rows_tile, 3 * C);
        jobs.add(PART(8), GR(gl.ln1_w), C, rows_ln, C);
        jobs.add(PART(9), GR(gl.ln1_b), C, rows_ln, C);
        LDIT_RUN(probe, LDIT_K_OTHER, launch_reduce_jobs(jobs, stream));
        if (mx) {
            LDIT_RUN(probe, LDIT_K_OTHER, launch_scale_inplace(GR(gl.wqkv), (size_t)C * C, qfold_of(g), stream));
            LDIT_RUN(probe, LDIT_K_OTHER, launch_scale_inplace(GR(gl.bqkv), (size_t)C, qfold_of(g), stream));
        }
    }
    if (stage_lo == 0) {
        // ---- embeddings: h0[b, 0] = cls + pos[0];  h0[b, 1 + i] = patch_i . Wp^T + bp + pos[1 + i]  (TF:81-90, 168-172) ------
        const int Mq = batch * g.P;
        LDIT_RUN(probe, LDIT_K_OTHER, launch_embed_bwd_small(dh, GR(gm.pos), GR(gm.cls), GR(gm.patch_b), batch, g.T, C, stream));
        LDIT_RUN(probe, LDIT_K_OTHER, launch_rows_to_bf16(dh, dz, Mq, C, g.P, stream));                  // dE: patch rows of dh0, bf16
        // the bf16 im2col of the batch: the forward left it in the saved block when it ran the bf16 patch embedding
        const char *patches = S + sm.patches;
        if (g.Kp % 64 != 0) {
            LDIT_RUN(probe, LDIT_K_OTHER, launch_patches_rows(static_cast<const float *>(x), ws + wm.patches, batch, g.in_ch, cfg->img_h,
                                                             cfg->img_w, g.p, stream));
            patches = ws + wm.patches;
        }
        LDIT_TRY(wgrad(probe, jobs, dz, C, patches, g.Kp, GR(gm.patch_w), reinterpret_cast<float *>(ws + wm.slab[0]), C, g.Kp, Mq,
                       zeros, stream));
        LDIT_RUN(probe, LDIT_K_OTHER, launch_reduce_jobs(jobs, stream));
    }
    return LDIT_OK;
}

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

size_t ldit_flat_param_bytes(const ldit_cfg *cfg)
{
    Geo g;
    if (geometry(cfg, g) != LDIT_OK) return 0;
    return packed_map(g, LDIT_F32).total;
}

int ldit_flat_param_layout(const ldit_cfg *cfg, int64_t *offsets, int32_t n)
{
    Geo g;
    LDIT_TRY(geometry(cfg, g));
    const int need = 4 + 14 * g.L + 1;
    if (!offsets || n < need) return fail(LDIT_EINVAL, "flat_param_layout: need room for %d offsets", need);
    const PackedMap m = packed_map(g, LDIT_F32);
    int k = 0;
    offsets[k++] = m.patch_w / 4; offsets[k++] = m.patch_b / 4; offsets[k++] = m.cls / 4; offsets[k++] = m.pos / 4;
    for (int l = 0; l < g.L; ++l) {
        const PackedLayer &p = m.layer[l];
        const size_t o[14] = {p.ln1_w, p.ln1_b, p.wqkv, p.bqkv, p.wo, p.bo, p.lam1, p.ln2_w, p.ln2_b, p.w1, p.b1, p.w2, p.b2, p.lam2};
        for (size_t v : o) offsets[k++] = (int64_t)(v / 4);
    }
    offsets[k++] = (int64_t)(m.total / 4);
    return LDIT_OK;
}

size_t ldit_train_saved_bytes(const ldit_cfg *cfg, int32_t batch)
{
    Geo g;
    if (batch <= 0 || train_geometry(cfg, g) != LDIT_OK) return 0;
    return saved_map(g, batch, cfg->dtype).total;
}

size_t ldit_train_workspace_bytes(const ldit_cfg *cfg, int32_t batch)
{
    Geo g;
    if (batch <= 0 || train_geometry(cfg, g) != LDIT_OK) return 0;
    return train_ws_map(g, batch).total;
}

size_t ldit_train_mirror_bytes(const ldit_cfg *cfg)
{
    Geo g;
    if (train_geometry(cfg, g) != LDIT_OK) return 0;
    return mirror_bytes(g, cfg->dtype);
}

int ldit_pack_train(const ldit_cfg *cfg, const void *flat_params, void *mirror, size_t mirror_bytes, ldit_stream stream)
{
    Geo g;
    LDIT_TRY(train_geometry(cfg, g));
    if (!flat_params || !mirror) return fail(LDIT_EINVAL, "pack_train: null pointer");
    if (!aligned16(flat_params) || !aligned16(mirror)) return fail(LDIT_EINVAL, "pack_train: pointers must be 16-byte aligned");
    const size_t n = packed_map(g, LDIT_F32).total / 4;
    if (mirror_bytes < ldit::mirror_bytes(g, cfg->dtype))
        return fail(LDIT_EWORKSPACE, "train mirror %zu bytes < required %zu", mirror_bytes, ldit::mirror_bytes(g, cfg->dtype));
    // one pass: the whole flat block rounded to bf16, same element layout (matrices stay in nn.Linear's [out, in] layout: the
    // forward reads them K-contiguous, the dgrad reads the SAME copy reduction-major, the wgrad needs no weight)
    LDIT_TRY(launch_cvt_bf16(static_cast<const float *>(flat_params), mirror, n, static_cast<hipStream_t>(stream)));
    if (cfg->dtype != LDIT_MXFP8) return LDIT_OK;
    // mxfp8: each layer's matrices re-made as ldit_pack_weights(LDIT_MXFP8) makes them (codes + scales, q third folded) with their
    // dequantised codes in the bf16 part, and the folded q|k|v bias - one launch for all layers
    return mx_requant_all_layers(g, static_cast<const float *>(flat_params), mirror, /*state*/ nullptr, static_cast<hipStream_t>(stream));
}

int ldit_adamw_step_mxfp8(const ldit_cfg *cfg, void *params, const void *grads, void *exp_avg, void *exp_avg_sq, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int32_t step, float grad_scale, void *mirror, size_t mirror_bytes,
                          ldit_stream stream_)
{
    Geo g;
    LDIT_TRY(train_geometry(cfg, g));
    if (cfg->dtype != LDIT_MXFP8) return fail(LDIT_EINVAL, "adamw_step_mxfp8: cfg.dtype must be LDIT_MXFP8");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !mirror) return fail(LDIT_EINVAL, "adamw_step_mxfp8: null pointer");
    if (!aligned16(params) || !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) || !aligned16(mirror))
        return fail(LDIT_EINVAL, "adamw_step_mxfp8: pointers must be 16-byte aligned");
    if (step < 1) return fail(LDIT_EINVAL, "adamw_step_mxfp8: step counts from 1");
    if (mirror_bytes < ldit::mirror_bytes(g, LDIT_MXFP8))
        return fail(LDIT_EWORKSPACE, "train mirror %zu bytes < required %zu", mirror_bytes, ldit::mirror_bytes(g, LDIT_MXFP8));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *p = static_cast<float *>(params), *m = static_cast<float *>(exp_avg), *v = static_cast<float *>(exp_avg_sq);
    const float *gr = static_cast<const float *>(grads);
    // ldit_adamw_step over the whole block (its bf16 mirror = the embeddings' operands), then every layer's matrices re-quantised
    // from the updated master: the codes, scales, folded bias and dequantised copies a fresh ldit_pack_train would make
    LDIT_TRY(launch_adamw(p, gr, m, v, packed_map(g, LDIT_F32).total / 4, lr, beta1, beta2, eps, weight_decay, step, grad_scale, mirror, stream));
    return mx_requant_all_layers(g, p, mirror, /*state*/ nullptr, stream);
}

int ldit_requant_train_mirror(const ldit_cfg *cfg, const void *flat_params, void *mirror, size_t mirror_bytes, const ldit_opt_state *state,
                              ldit_stream stream)
{
    Geo g;
    LDIT_TRY(train_geometry(cfg, g));
    if (cfg->dtype != LDIT_MXFP8) return fail(LDIT_EINVAL, "requant_train_mirror: cfg.dtype must be LDIT_MXFP8");
    if (!flat_params || !mirror) return fail(LDIT_EINVAL, "requant_train_mirror: null pointer");
    if (!aligned16(flat_params) || !aligned16(mirror)) return fail(LDIT_EINVAL, "requant_train_mirror: pointers must be 16-byte aligned");
    if (state && (reinterpret_cast<uintptr_t>(state) & 3u)) return fail(LDIT_EINVAL, "requant_train_mirror: state block must be 4-byte aligned");
    if (mirror_bytes < ldit::mirror_bytes(g, LDIT_MXFP8))
        return fail(LDIT_EWORKSPACE, "train mirror %zu bytes < required %zu", mirror_bytes, ldit::mirror_bytes(g, LDIT_MXFP8));
    // one launch for every layer's matrices and fused bias; the rest of the mirror is the AdamW kernels' (or the last pack's)
    return mx_requant_all_layers(g, static_cast<const float *>(flat_params), mirror, state, static_cast<hipStream_t>(stream));
}

int ldit_vit_forward_train(const ldit_cfg *cfg, const void *packed, const void *flat_params, const void *x, int32_t batch,
                           void *const *tap_out, const void *drop_scales, void *saved, size_t saved_bytes, ldit_stream stream,
                           double *ms, int64_t *launches)
{
    Probe probe;
    probe.on = ms && launches;
    probe.stream = static_cast<hipStream_t>(stream);
    int rc = forward_train(cfg, packed, flat_params, x, batch, tap_out, drop_scales, saved, saved_bytes, probe.stream, probe);
    int rc2 = probe.collect(ms, launches);
    return rc != LDIT_OK ? rc : rc2;
}

int ldit_vit_backward(const ldit_cfg *cfg, const void *flat_params, const void *packed, const void *x, int32_t batch, void *const *dtaps,
                      const void *drop_scales, const void *saved, size_t saved_bytes, void *grads, size_t grads_bytes, void *workspace,
                      size_t workspace_bytes, int32_t stage_hi, int32_t stage_lo, ldit_stream stream, double *ms, int64_t *launches)
{
    Probe probe;
    probe.on = ms && launches;
    probe.stream = static_cast<hipStream_t>(stream);
    int rc = backward(cfg, flat_params, packed, x, batch, dtaps, drop_scales, saved, saved_bytes, grads, grads_bytes, workspace, workspace_bytes, stage_hi,
                      stage_lo, probe.stream, probe);
    int rc2 = probe.collect(ms, launches);
    return rc != LDIT_OK ? rc : rc2;
}

int ldit_adamw_step(void *params, const void *grads, void *exp_avg, void *exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int32_t step, float grad_scale, void *bf16_mirror, ldit_stream stream)
{
    if (n < 0) return fail(LDIT_EINVAL, "adamw: negative length");
    if (bf16_mirror && (reinterpret_cast<uintptr_t>(bf16_mirror) & 7u)) return fail(LDIT_EINVAL, "adamw: bf16 mirror misaligned");
    return launch_adamw(static_cast<float *>(params), static_cast<const float *>(grads), static_cast<float *>(exp_avg),
                        static_cast<float *>(exp_avg_sq), (size_t)n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, bf16_mirror,
                        static_cast<hipStream_t>(stream));
}

// ---- single kernels of the backward (unit parity tests) -------------------------------------------------------------------
// ---- single kernels of the mxfp8 train forward (unit parity tests) ------------------------------------------------------
int ldit_layernorm_mxfp8_train(const void *x, const void *gamma, const void *beta, void *Y, void *Ys, void *Yd, int64_t rows, int64_t C,
                               float eps, ldit_stream stream)
{
    if (rows <= 0 || C <= 0 || C > 4096 || C % 32) return fail(LDIT_EINVAL, "layernorm_mxfp8_train: bad shape");
    return layernorm(Build{LDIT_MXFP8, true}, static_cast<const float *>(x), static_cast<const float *>(gamma), static_cast<const float *>(beta),
                     operand(Y, Ys, C), Yd, rows, (int)C, eps, static_cast<hipStream_t>(stream));
}

int ldit_attention_mxfp8_train(const void *Q, const void *K, const void *V, void *O, void *Os, void *lse, void *Ob, void *Od, int64_t B,
                               int64_t N, int64_t H, int64_t D, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale,
                               ldit_stream stream)
{
    if (B <= 0 || N <= 0 || H <= 0) return fail(LDIT_EINVAL, "attention_mxfp8_train: empty problem");
    if (B * N * (ldq > ldo ? ldq : ldo) >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "attention_mxfp8_train: operand exceeds 2^31 elements");
    return attention(Build{LDIT_MXFP8, true}, Q, K, V, (int)ldq, (int)ldk, (int)ldv, operand(O, Os, ldo), (int)B, (int)N, (int)H, (int)D, scale,
                     static_cast<hipStream_t>(stream), static_cast<float *>(lse), Ob, Od);
}

int ldit_linear_mxfp8_train(const void *X, int64_t lda, const void *Xs, const void *W, const void *Ws, const void *bias, void *Y,
                            int64_t ldy, void *Ys, int64_t M, int64_t N, int64_t K, int32_t epilogue, const void *lam, const void *R,
                            void *Y2, void *Ypre, const void *rowscale, void *Yd, ldit_stream stream)
{
    if (M <= 0 || N <= 0 || K <= 0) return fail(LDIT_EINVAL, "linear_mxfp8_train: empty problem");
    if (M * (ldy > lda ? ldy : lda) >= (1ll << 31) || N * K >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "linear_mxfp8_train: operand exceeds 2^31 elements");
    if (ldy < N || lda < K) return fail(LDIT_EINVAL, "linear_mxfp8_train: bad leading dimension");
    if (K % 128 || lda % 128) return fail(LDIT_EUNSUPPORTED, "linear_mxfp8_train: K and lda must be multiples of 128");
    if (!X || !W || !Xs || !Ws || !Y) return fail(LDIT_EINVAL, "linear_mxfp8_train: null operand");
    if (!aligned16(X) || !aligned16(W) || (reinterpret_cast<uintptr_t>(Y) & 15u) || (Y2 && !aligned16(Y2)))
        return fail(LDIT_EINVAL, "linear_mxfp8_train: misaligned operand");
    int epi;
    if (epilogue == LDIT_EPI_SCALE_RESID) {
        if (!lam || !R) return fail(LDIT_EINVAL, "linear_mxfp8_train: the scale + residual epilogue needs lam and R");
        epi = EPI_SCALE_RESID;
    } else if (epilogue == LDIT_EPI_BIAS_GELU) {
        if (!Ys || N % 32 || ldy % 32) return fail(LDIT_EINVAL, "linear_mxfp8_train: the GELU epilogue writes MX: Ys needed, N and ldy multiples of 32");
        epi = EPI_BIAS_GELU;
    } else {
        return fail(LDIT_EINVAL, "linear_mxfp8_train: epilogue %d not available (scale + residual or bias + GELU)", epilogue);
    }
    return linear(Build{LDIT_MXFP8, true}, operand(X, Xs, lda), W, Ws, static_cast<const float *>(bias), operand(Y, Ys, ldy), (int)M, (int)N, (int)K, epi,
                  static_cast<const float *>(lam), static_cast<const float *>(R), static_cast<float *>(Y2),
                  Side{Ypre, static_cast<const float *>(rowscale), Yd}, static_cast<hipStream_t>(stream));
}

int ldit_attention_fwd_lse_bf16(const void *Q, const void *K, const void *V, void *O, void *lse, int64_t B, int64_t N, int64_t H,
                                int64_t D, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, ldit_stream stream)
{
    if (B <= 0 || N <= 0 || H <= 0) return fail(LDIT_EINVAL, "attention_fwd_lse: empty problem");
    if (B * N * 3 * H * D >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "attention_fwd_lse: operand exceeds 2^31 elements");
    return attention(Build{LDIT_BF16, true}, Q, K, V, (int)ldq, (int)ldk, (int)ldv, operand(O, nullptr, ldo), (int)B, (int)N, (int)H, (int)D, scale,
                     static_cast<hipStream_t>(stream), static_cast<float *>(lse));
}

int ldit_attention_bwd_bf16(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *lse, void *dQ,
                            void *dK, void *dV, int64_t B, int64_t N, int64_t H, int64_t D, int64_t ldqkv, int64_t ldo, int64_t lddo,
                            int64_t lddqkv, float scale, ldit_stream stream)
{
    if (B <= 0 || N <= 0 || H <= 0) return fail(LDIT_EINVAL, "attention_bwd: empty problem");
    if (B * N * (ldqkv > lddqkv ? ldqkv : lddqkv) >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "attention_bwd: operand exceeds 2^31 elements");
    return launch_attention_bwd_bf16(Q, K, V, O, dO, static_cast<const float *>(lse), dQ, dK, dV, (int)B, (int)N, (int)H, (int)D,
                                     (int)ldqkv, (int)ldo, (int)lddo, (int)lddqkv, scale, static_cast<hipStream_t>(stream));
}

size_t ldit_layernorm_bwd_scratch_bytes(int64_t rows, int64_t C)
{
    if (rows <= 0 || C <= 0) return 0;
    return (size_t)2 * layernorm_bwd_blocks(rows) * (size_t)C * 4;
}

int ldit_layernorm_bwd_f32(const void *dy, const void *x, const void *gamma, void *dh, int64_t rows, int64_t C, float eps,
                           void *dgamma, void *dbeta, void *scratch, size_t scratch_bytes, ldit_stream stream_)
{
    if (rows <= 0 || C <= 0 || C > 4096) return fail(LDIT_EINVAL, "layernorm_bwd: bad shape");
    if (!dgamma || !dbeta || !scratch) return fail(LDIT_EINVAL, "layernorm_bwd: null operand");
    if (scratch_bytes < ldit_layernorm_bwd_scratch_bytes(rows, C)) return fail(LDIT_EWORKSPACE, "layernorm_bwd: scratch too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int blocks = layernorm_bwd_blocks(rows);
    float *pg = static_cast<float *>(scratch), *pb = pg + (size_t)blocks * C;
    LDIT_TRY(launch_layernorm_bwd(static_cast<const float *>(dy), static_cast<const float *>(x), static_cast<const float *>(gamma),
                                  static_cast<float *>(dh), rows, (int)C, eps, pg, pb, stream));
    ReduceJobs jobs;
    jobs.add(pg, static_cast<float *>(dgamma), C, blocks, C);
    jobs.add(pb, static_cast<float *>(dbeta), C, blocks, C);
    return launch_reduce_jobs(jobs, stream);
}

// partial rows of the fused LayerNorm + LayerScale backward: the count the launcher's grid has (train_ops.hip)
static int layernorm_bwd_resid_part_rows(int64_t rows, int64_t C)
{
    return C <= 1024 ? layernorm_bwd_resid_blocks(rows) : layernorm_bwd_blocks(rows);
}

size_t ldit_layernorm_bwd_resid_scratch_bytes(int64_t rows, int64_t C)
{
    if (rows <= 0 || C <= 0) return 0;
    return (size_t)4 * layernorm_bwd_resid_part_rows(rows, C) * (size_t)C * 4;
}

int ldit_layernorm_bwd_resid_f32(const void *dy, const void *x, const void *gamma, const void *z, const void *lam, const void *rowscale,
                                 void *dh, void *dz, int64_t rows, int64_t C, float eps, void *dgamma, void *dbeta, void *dlam,
                                 void *dzbias, void *scratch, size_t scratch_bytes, ldit_stream stream_)
{
    if (rows <= 0 || C <= 0 || C > 4096) return fail(LDIT_EINVAL, "layernorm_bwd_resid: bad shape");
    if (!dgamma || !dbeta || !dlam || !dzbias || !scratch || !aligned16(scratch)) return fail(LDIT_EINVAL, "layernorm_bwd_resid: null operand or misaligned scratch");
    if (!aligned16(dy) || !aligned16(x) || !aligned16(gamma) || !aligned16(dh))
        return fail(LDIT_EINVAL, "layernorm_bwd_resid: dy, x, gamma, dh must be 16-byte aligned");
    if (scratch_bytes < ldit_layernorm_bwd_resid_scratch_bytes(rows, C)) return fail(LDIT_EWORKSPACE, "layernorm_bwd_resid: scratch too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int blocks = layernorm_bwd_resid_part_rows(rows, C);
    const size_t pn = (size_t)blocks * C;
    float *pg = static_cast<float *>(scratch), *pb = pg + pn, *pl = pb + pn, *pz = pl + pn;
    LDIT_TRY(launch_layernorm_bwd_resid(static_cast<const float *>(dy), static_cast<const float *>(x), static_cast<const float *>(gamma),
                                        static_cast<float *>(dh), rows, (int)C, eps, pg, pb, z, static_cast<const float *>(lam),
                                        static_cast<const float *>(rowscale), dz, pl, pz, stream));
    ReduceJobs jobs;
    jobs.add(pg, static_cast<float *>(dgamma), C, blocks, C);
    jobs.add(pb, static_cast<float *>(dbeta), C, blocks, C);
    jobs.add(pl, static_cast<float *>(dlam), C, blocks, C);
    jobs.add(pz, static_cast<float *>(dzbias), C, blocks, C);
    return launch_reduce_jobs(jobs, stream);
}

size_t ldit_resid_bwd_scratch_bytes(int64_t rows, int64_t C)
{
    if (rows <= 0 || C <= 0) return 0;
    return (size_t)2 * (size_t)((rows + 63) / 64) * (size_t)C * 4;
}

int ldit_resid_bwd_bf16(const void *dh, const void *z, const void *lam, const void *rowscale, void *dz, int64_t rows, int64_t C,
                        void *dlam, void *dbias, void *scratch, size_t scratch_bytes, ldit_stream stream_)
{
    if (rows <= 0 || C <= 0 || rows + 63 >= (1ll << 31) || C >= (1ll << 31)) return fail(LDIT_EINVAL, "resid_bwd: bad shape");
    if (C % 64) return fail(LDIT_EUNSUPPORTED, "resid_bwd: C=%lld must be a multiple of 64", (long long)C);
    if (!dh || !z || !lam || !dz || !dlam || !dbias || !scratch || !aligned16(scratch)) return fail(LDIT_EINVAL, "resid_bwd: null operand or misaligned scratch");
    if (!aligned16(dh) || !aligned16(lam) || !aligned16(dz) || (reinterpret_cast<uintptr_t>(z) & 7u))
        return fail(LDIT_EINVAL, "resid_bwd: dh, lam, dz must be 16-byte aligned, z 8-byte aligned");
    if (scratch_bytes < ldit_resid_bwd_scratch_bytes(rows, C)) return fail(LDIT_EWORKSPACE, "resid_bwd: scratch too small");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int Mp = (int)((rows + 63) / 64 * 64), blocks = Mp / 64;
    float *pl = static_cast<float *>(scratch), *pb = pl + (size_t)blocks * C;
    LDIT_TRY(launch_resid_bwd(static_cast<const float *>(dh), z, static_cast<const float *>(lam), static_cast<const float *>(rowscale), dz,
                              nullptr, (int)rows, (int)C, Mp, pl, pb, stream));
    ReduceJobs jobs;
    jobs.add(pl, static_cast<float *>(dlam), C, blocks, C);
    jobs.add(pb, static_cast<float *>(dbias), C, blocks, C);
    return launch_reduce_jobs(jobs, stream);
}

int ldit_linear_bf16_ex(const void *X, int64_t lda, const void *W, const void *bias, void *Y, int64_t ldy, int64_t M, int64_t N,
                        int64_t K, int32_t epilogue, const void *lam, const void *R, void *Y2, void *Ypre, const void *rowscale,
                        const void *aux, int64_t ldaux, int32_t splits, ldit_stream stream)
{
    LDIT_TRY(check_linear("linear_bf16_ex", M, N, K, lda, ldy, Y, Y2));
    int epi;
    switch (epilogue) {
        case LDIT_EPI_BIAS: epi = EPI_BIAS; break;
        case LDIT_EPI_BIAS_GELU: epi = EPI_BIAS_GELU; break;
        case LDIT_EPI_SCALE_RESID: epi = EPI_SCALE_RESID; break;
        case LDIT_EPI_F32: epi = EPI_F32; break;
        case LDIT_EPI_GELU_BWD: epi = EPI_GELU_BWD; break;
        case LDIT_EPI_BIAS_RELU: epi = EPI_BIAS_RELU; break;
        default: return fail(LDIT_EINVAL, "linear_bf16_ex: unknown epilogue %d", epilogue);
    }
    GemmExtra x{};
    x.Ypre = Ypre; x.rowscale = static_cast<const float *>(rowscale); x.aux = aux; x.ldaux = (int)ldaux; x.splits = splits < 1 ? 1 : splits;
    return launch_gemm_bf16_ex(X, (int)lda, W, static_cast<const float *>(bias), Y, (int)ldy, (int)M, (int)N, (int)K, epi,
                               static_cast<const float *>(lam), static_cast<const float *>(R), static_cast<float *>(Y2), x,
                               static_cast<hipStream_t>(stream));
}

int ldit_linear_bf16_tr(const void *A, int64_t lda, int32_t a_reduction_major, const void *W, int64_t ldw, void *Y, int64_t ldy,
                        int64_t M, int64_t N, int64_t K, int32_t epilogue, const void *aux, int32_t splits, const void *zeros,
                        ldit_stream stream)
{
    if (M <= 0 || N <= 0 || K <= 0) return fail(LDIT_EINVAL, "linear_bf16_tr: empty problem");
    if (M * ldy >= (1ll << 31) || K * (lda > ldw ? lda : ldw) >= (1ll << 31) || M * lda >= (1ll << 31))
        return fail(LDIT_EUNSUPPORTED, "linear_bf16_tr: operand exceeds 2^31 elements");
    if (ldy < N || ldw < N || lda < (a_reduction_major ? M : K)) return fail(LDIT_EINVAL, "linear_bf16_tr: bad leading dimension");
    if (!Y || !aligned16(Y)) return fail(LDIT_EINVAL, "linear_bf16_tr: output null or misaligned");
    int epi;
    switch (epilogue) {
        case LDIT_EPI_BIAS: epi = EPI_BIAS; break;
        case LDIT_EPI_F32: epi = EPI_F32; break;
        case LDIT_EPI_GELU_BWD: epi = EPI_GELU_BWD; break;
        default: return fail(LDIT_EINVAL, "linear_bf16_tr: epilogue %d not available", epilogue);
    }
    GemmExtra x{};
    x.aux = aux; x.ldaux = (int)N; x.splits = splits < 1 ? 1 : splits; x.zeros = zeros;
    return launch_gemm_bf16_tr(A, (int)lda, a_reduction_major != 0, W, (int)ldw, nullptr, Y, (int)ldy, (int)M, (int)N, (int)K, epi, x,
                               static_cast<hipStream_t>(stream));
}

int ldit_reduce_slabs_f32(const void *slabs, void *out, int64_t n, int32_t count, ldit_stream stream)
{
    if (!slabs || !out || n <= 0 || count <= 0) return fail(LDIT_EINVAL, "reduce_slabs: bad argument");
    ReduceJobs jobs;
    jobs.add(static_cast<const float *>(slabs), static_cast<float *>(out), n, count, n);
    return launch_reduce_jobs(jobs, static_cast<hipStream_t>(stream));
}

}  // extern "C"
