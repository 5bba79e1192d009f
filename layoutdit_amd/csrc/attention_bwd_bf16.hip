// Backward of the fused self-attention (train step, BASELINE configs[2]):  given Q, K, V, O (bf16, as the forward left
// them), dO (bf16) and the forward's log2-domain log-sum-exp L2[q] = log2 sum_k exp2(c s_qk), c = scale log2 e, produce
// dQ, dK, dV (bf16) per (image, head).  TF:models/beit/modeling_beit.py:268-293 differentiated:
//     P = softmax(scale Q K^T)      dV = P^T dO      dP = dO V^T      dS = P (.) (dP - delta) scale,  delta_q = sum_d dO O
//     dQ = dS K                     dK = dS^T Q
// Probabilities are recomputed from L2 (p = exp2(c s - L2), no row maximum needed), never stored.
//
// One 512-thread workgroup per (image, head) for N <= 256 tokens (the detector runs at 224 x 224 -> 197; longer sequences take
// the blocked form below), so Q, K, V and dO
// of the head live in LDS for the whole kernel (row-major 128-B rows, 16-B chunk XOR-swizzled with (row>>1)&7: b128 row
// reads for the operands that are consumed row-wise, ds_read_b64_tr_b16 for the ones consumed column-wise - one image
// serves both).  Rows past N are ZERO in all four images.  A padded query needs no mask: Q = dO = 0, delta = 0, L2 = 0, so p = 1
// (finite) and it adds nothing to dK / dV.  A padded KEY does: its score is 0, so its recomputed probability is exp2(-L2) of
// the query's row - not small when that row's logits are all very negative, and +inf once L2 < ~-128 (all logits of the row below
// ~-88 natural units), where dS = inf (0 - delta) scale times the zero K row is inf 0 = NaN in every element of that query's dQ.
// So p and dS of a padded key are made exactly 0, and full key blocks pay nothing for it:
//   phase 1 (key = lane): the lanes of padded keys read every row's L2 from Linf, an LDS array of +inf, instead of L2s: p = exp2(-inf)
//            = 0, dS = 0 (0 - delta) scale = 0 with the loop's instructions unchanged (a second instance of phase1_block for the
//            partial block does not fit the blocked kernel's registers: 256 VGPRs and 8 spilled);
//   phase 2 (key = register): dS of the padded keys is SELECTED to 0 (mask_key_regs) in phase2_block<true>, an instance of the
//            one body that only the last, partial block of 32 keys runs, peeled behind the loop over full blocks.
// No sum that was finite before changes a bit.
//
// Two phases, every product on v_mfma_f32_32x32x16_bf16 with the accumulator of the first product reused as the B operand
// of the second one (guide section 3, "An accumulator tile as the next MFMA's operand"; same trick as the forward):
//   phase 1, wave = one block of 32 keys, loop over query blocks:   S[q, key] and dP[q, key] with the key on the lane,
//            dV^T[d, key] += dO^T P,  dK^T[d, key] += Q^T dS     (A operands = transposing reads of the dO / Q images)
//   phase 2, wave = one block of 32 queries, loop over key blocks:  S^T[key, q], dP^T[key, q] with the query on the lane,
//            dQ^T[d, q] += K^T dS^T                              (A operand = transposing reads of the K image)
// S and dP are therefore computed twice (28 MFMAs per (query block, key block) pair instead of 20) - the price for
// keeping every sum inside one wave: no atomics, no cross-wave reduction, bit-reproducible.  Attention backward is 4 % of
// the train step's FLOPs.
//
// N > 256 tokens (ViT-L/16 at 512 x 512 = 1025 tokens trains too): the same two phases, BLOCKED.  The sequence is cut into
// blocks of 256 rows and the four LDS images (32 KB each, + L2 and delta) hold ONE resident block and ONE streamed block:
//   ROLE 0 (one workgroup per (image, head, KEY block)):   K, V of the block resident; every QUERY block is streamed through
//           the Q / dO / L2 / delta images and phase 1 runs on it; dK^T, dV^T stay in the waves' registers across ALL query
//           blocks and are stored once - no sum crosses a workgroup;
//   ROLE 1 (one workgroup per (image, head, QUERY block)):  Q, dO, L2, delta resident; every KEY block is streamed through the
//           K / V images and phase 2 runs on it; dQ^T stays in registers across all key blocks.
// Both kernels run the SAME staging routine and the SAME phase bodies (stage, phase1_block, phase2_block below; only where a
// row index comes from differs), so every output element is a fixed-order sum inside one wave in either form.  The blocked
// form stages synchronously (load, barrier, multiply, barrier): it exists so that long sequences CAN train; BASELINE
// configs[2] (197 tokens) runs the one-block kernel.
#include "ldit_common.h"

namespace ldit {

namespace {

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int ROWB = 128;      // bytes per image row (64 bf16)
constexpr int BR = 256;        // rows per block: all of the one-block kernel's, one resident + one streamed of the blocked one's
constexpr int LDS_MAX = 4 * BR * ROWB + 3 * BR * 4;

// one argument list for the three kernels
struct BwdArgs {
    const bf16_t *Q, *K, *V, *O, *dO;   // row strides ldqkv (Q, K, V), ldo, lddo (elements)
    const float *lse;                   // [B, H, N]
    bf16_t *dQ, *dK, *dV;               // row stride lddqkv
    int N, H, nblk, ldqkv, ldo, lddo, lddqkv;
    float scale;
};

// the operands of one (image, head): row 0, column 0 of each
struct Head {
    const bf16_t *q, *k, *v, *o, *g;    // g = dO
    const float *lse;
    bf16_t *dq, *dk, *dv;
    int N, ldqkv, ldo, lddo, lddqkv;
    __device__ __forceinline__ Head(const BwdArgs &a, int b, int head) : lse(a.lse + ((size_t)b * a.H + head) * a.N), N(a.N),
                                                                         ldqkv(a.ldqkv), ldo(a.ldo), lddo(a.lddo), lddqkv(a.lddqkv)
    {
        const size_t tok0 = (size_t)b * a.N;
        q = a.Q + tok0 * ldqkv + head * 64; k = a.K + tok0 * ldqkv + head * 64; v = a.V + tok0 * ldqkv + head * 64;
        o = a.O + tok0 * ldo + head * 64; g = a.dO + tok0 * lddo + head * 64;
        dq = a.dQ + tok0 * lddqkv + head * 64; dk = a.dK + tok0 * lddqkv + head * 64; dv = a.dV + tok0 * lddqkv + head * 64;
    }
};

// the dynamic LDS block: four images of `rows` rows and three fp32 arrays of `rows` elements
struct Lds {
    char *Qs, *Ks, *Vs, *Gs;            // Gs = dO image
    float *L2s, *dlt, *Linf;            // Linf: rows times +inf
    __device__ __forceinline__ Lds(char *smem, int rows) : Qs(smem), Ks(Qs + rows * ROWB), Vs(Ks + rows * ROWB), Gs(Vs + rows * ROWB),
                                                           L2s(reinterpret_cast<float *>(Gs + rows * ROWB)), dlt(L2s + rows), Linf(dlt + rows) {}
};

// what every product of a wave needs: its lane (c32 = lane & 31, h = lane >> 5) and the two softmax factors
struct Lane {
    int lane, c32, h;
    float c, scale;                     // c = scale log2 e
    __device__ __forceinline__ Lane(int lane_, float scale_) : lane(lane_), c32(lane_ & 31), h(lane_ >> 5), c(scale_ * 1.44269504088896340736f), scale(scale_) {}
};

__device__ __forceinline__ int img_off(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }

// 8 consecutive elements (one 16-B chunk) of image row `row`
__device__ __forceinline__ bf16x8 row_frag(const char *img, int row, int chunk)
{
    return *reinterpret_cast<const bf16x8 *>(img + img_off(row, chunk));
}

// the 4 + 4 resident fragments of a wave: its row of two images, all 64 columns
__device__ __forceinline__ void load_frags(const char *img_a, const char *img_b, int row, int h, bf16x8 (&a)[4], bf16x8 (&b)[4])
{
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        a[s] = row_frag(img_a, row, 2 * s + h);
        b[s] = row_frag(img_b, row, 2 * s + h);
    }
}

// A operand of a product that sums over the image's ROW index: lane (c = lane&31, h) gets, for element jj,
// img[row0 + 8 (jj>>2) + 4 h + (jj&3)][col0 + c] - two transposing reads (4 rows x 16 columns per 16-lane group)
__device__ __forceinline__ bf16x8 col_frag(const char *img, int row0, int col0, int lane)
{
    const int grp = lane >> 4, i16 = lane & 15;
    const int col = col0 + 16 * (grp & 1) + 4 * (i16 & 3);
    const int r = row0 + 4 * (grp >> 1) + (i16 >> 2);
    union { s16x4 v[2]; bf16x8 f; } u;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int row = r + 8 * t;
        const char *a = img + row * ROWB + (((col >> 3) ^ ((row >> 1) & 7)) << 4) + ((col & 7) << 1);
        u.v[t] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)a);
    }
    return u.f;
}

__device__ __forceinline__ bf16x8 pack8(const f32x16 &v, int s)
{
    bf16x8 o;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) o[jj] = (bf16_t)v[8 * s + jj];
    return o;
}

// Padded keys of the last, partial key block, phase 2 / ROLE 1 (phase 1 / ROLE 0 need no instruction: see Linf).  phase2_block is
// instantiated twice - TAIL = false for full blocks (the body as it always was, one scheduling region from the first MFMA to the
// last), TAIL = true for the block that reaches past N, peeled behind the loop over full blocks: a branch INSIDE the body cuts
// it in two between the softmax arithmetic and the second products (measured: +2 % at N = 197, +6 % at N = 1025).
// Phase 2 / ROLE 1: the key is the register, r <-> key (r&3) + 8 (r>>2) + 4 h of the block; nkeys of its 32 keys exist.
__device__ __forceinline__ void mask_key_regs(f32x16 &ds, int nkeys, int h)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) ds[r] = ((r & 3) + 8 * (r >> 2) + 4 * h) >= nkeys ? 0.0f : ds[r];
}

// Stage rows [r0, r0 + 256) of the head into image rows 0..255 (those below `rows`): the key side (K, V images), the query side (Q,
// dO images, L2, delta = rowsum(dO . O), Linf) or both; rows past N are zero.  16-B chunk (row, ch) per thread and pass.  All passes'
// loads (up to 4 x 5 chunks) are issued before the first LDS store: one memory round trip for the head, not one per pass.
template <bool KEYS, bool QUERIES>
__device__ __forceinline__ void stage(const Head &hd, const Lds &s, int r0, int rows, int tid)
{
    constexpr int PASSES = BR / 64;                 // 64 rows per pass
    bf16x8 q[PASSES], k[PASSES], v[PASSES], g[PASSES], o[PASSES];
    const int ch = tid & 7;
    auto chunk = [&](const bf16_t *base, int row, int ld) { return *reinterpret_cast<const bf16x8 *>(base + (size_t)row * ld + 8 * ch); };
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int row = r0 + 64 * ps + (tid >> 3);
        q[ps] = bf16x8{}; k[ps] = bf16x8{}; v[ps] = bf16x8{}; g[ps] = bf16x8{}; o[ps] = bf16x8{};
        if (row < hd.N) {
            if (QUERIES) q[ps] = chunk(hd.q, row, hd.ldqkv);
            if (KEYS) k[ps] = chunk(hd.k, row, hd.ldqkv);
            if (KEYS) v[ps] = chunk(hd.v, row, hd.ldqkv);
            if (QUERIES) g[ps] = chunk(hd.g, row, hd.lddo);
            if (QUERIES) o[ps] = chunk(hd.o, row, hd.ldo);
        }
    }
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int lrow = 64 * ps + (tid >> 3), row = r0 + lrow;
        float d = 0.0f;
        if (QUERIES) {
#pragma unroll
            for (int e = 0; e < 8; ++e) d = __builtin_fmaf((float)g[ps][e], (float)o[ps][e], d);
            d += __shfl_xor(d, 1, 64);
            d += __shfl_xor(d, 2, 64);
            d += __shfl_xor(d, 4, 64);
        }
        if (lrow < rows) {
            const int off = img_off(lrow, ch);
            if (QUERIES) *reinterpret_cast<bf16x8 *>(s.Qs + off) = q[ps];
            if (KEYS) *reinterpret_cast<bf16x8 *>(s.Ks + off) = k[ps];
            if (KEYS) *reinterpret_cast<bf16x8 *>(s.Vs + off) = v[ps];
            if (QUERIES) *reinterpret_cast<bf16x8 *>(s.Gs + off) = g[ps];
            if (QUERIES && ch == 0) {
                s.dlt[lrow] = d;
                s.L2s[lrow] = row < hd.N ? hd.lse[row] : 0.0f;
                s.Linf[lrow] = INFINITY;
            }
        }
    }
}

// Phase 1 on the 32 queries at image rows q0..: S and dP against the wave's 32 keys (kf, vf: the key on the lane), then
// dV^T += dO^T P and dK^T += Q^T dS.  L2k = L2s, or Linf on the lane of a padded key.
__device__ __forceinline__ void phase1_block(const Lds &s, int q0, const bf16x8 (&kf)[4], const bf16x8 (&vf)[4], const float *L2k,
                                             f32x16 (&dk)[2], f32x16 (&dv)[2], const Lane &w)
{
    f32x16 sc = {}, dp = {};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(s.Qs, q0 + w.c32, 2 * t + w.h), kf[t], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(s.Gs, q0 + w.c32, 2 * t + w.h), vf[t], dp, 0, 0, 0);
    }
    // register r <-> query q0 + (r&3) + 8 (r>>2) + 4 h
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 l2 = *reinterpret_cast<const f32x4 *>(L2k + q0 + 8 * g + 4 * w.h);
        const f32x4 de = *reinterpret_cast<const f32x4 *>(s.dlt + q0 + 8 * g + 4 * w.h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[4 * g + e], w.c, -l2[e]));
            sc[4 * g + e] = p;
            dp[4 * g + e] = p * (dp[4 * g + e] - de[e]) * w.scale;
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const bf16x8 pb = pack8(sc, t), db = pack8(dp, t);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(col_frag(s.Gs, q0 + 16 * t, 32 * dt, w.lane), pb, dv[dt], 0, 0, 0);
            dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(col_frag(s.Qs, q0 + 16 * t, 32 * dt, w.lane), db, dk[dt], 0, 0, 0);
        }
    }
}

// Phase 2 on the 32 keys at image rows key0.. (nkeys of them real; fewer than 32 only with TAIL): S^T and dP^T against the wave's 32
// queries (qf, gf, l2, de: the query on the lane), then dQ^T += K^T dS^T.
template <bool TAIL>
__device__ __forceinline__ void phase2_block(const Lds &s, int key0, const bf16x8 (&qf)[4], const bf16x8 (&gf)[4], float l2, float de,
                                             int nkeys, f32x16 (&dq)[2], const Lane &w)
{
    f32x16 sc = {}, dp = {};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(s.Ks, key0 + w.c32, 2 * t + w.h), qf[t], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(s.Vs, key0 + w.c32, 2 * t + w.h), gf[t], dp, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[r], w.c, -l2));
        dp[r] = p * (dp[r] - de) * w.scale;
    }
    if constexpr (TAIL) mask_key_regs(dp, nkeys, w.h);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const bf16x8 db = pack8(dp, t);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
            dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(col_frag(s.Ks, key0 + 16 * t, 32 * dt, w.lane), db, dq[dt], 0, 0, 0);
    }
}

// a transposed accumulator pair [d = register row, token = lane] to the token's 64 bf16 of `out` (row 0 of the head)
__device__ __forceinline__ void store_row(bf16_t *out, int row, int ld, const f32x16 (&acc)[2], int h)
{
    bf16_t *p = out + (size_t)row * ld + 4 * h;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bf16x4 a = {(bf16_t)acc[dt][4 * g + 0], (bf16_t)acc[dt][4 * g + 1], (bf16_t)acc[dt][4 * g + 2], (bf16_t)acc[dt][4 * g + 3]};
            *reinterpret_cast<bf16x4 *>(p + 32 * dt + 8 * g) = a;
        }
}

// N <= 256: one workgroup per (image, head), wave w owns rows 32 w .. of both phases
__global__ void __launch_bounds__(512, 2) attention_bwd_bf16(const BwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, nb = (N + 31) >> 5;
    const Lds s(smem, nb * 32);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Lane w(tid & 63, a.scale);
    const Head hd(a, blockIdx.x / a.H, blockIdx.x % a.H);

    stage<true, true>(hd, s, 0, nb * 32, tid);
    __syncthreads();
    if (wave >= nb) return;            // wave-uniform: the transposing reads below need every lane of a wave active
    const int row = wave * 32 + w.c32; // this lane's key (phase 1) and query (phase 2)

    // ================= phase 1: this wave's 32 keys; dK^T, dV^T [d = register row, key = lane] ========================
    {
        bf16x8 kf[4], vf[4];
        load_frags(s.Ks, s.Vs, row, w.h, kf, vf);
        f32x16 dk[2] = {}, dv[2] = {};
        // a padded key reads +inf for every row's L2: p = exp2(0 c - inf) = 0 and dS = 0 (delta - 0) = 0, at no cost in the loop
        const float *L2k = row < N ? s.L2s : s.Linf;
        for (int i = 0; i < nb; ++i) phase1_block(s, i * 32, kf, vf, L2k, dk, dv, w);
        if (row < N) {
            store_row(hd.dk, row, hd.lddqkv, dk, w.h);
            store_row(hd.dv, row, hd.lddqkv, dv, w.h);
        }
    }

    // ================= phase 2: this wave's 32 queries; dQ^T [d = register row, query = lane] ==========================
    {
        bf16x8 qf[4], gf[4];
        load_frags(s.Qs, s.Gs, row, w.h, qf, gf);
        const float l2 = s.L2s[row], de = s.dlt[row];
        f32x16 dq[2] = {};
        const int nfull = N >> 5;
        for (int j = 0; j < nfull; ++j) phase2_block<false>(s, j * 32, qf, gf, l2, de, 32, dq, w);
        if (nfull < nb) phase2_block<true>(s, nfull * 32, qf, gf, l2, de, N - nfull * 32, dq, w);     // the last, partial key block, peeled
        if (row < N) store_row(hd.dq, row, hd.lddqkv, dq, w.h);
    }
}

// N > 256: one workgroup per (image, head, resident block); ROLE 0 = keys resident, phase 1; ROLE 1 = queries resident, phase 2
template <int ROLE>
__global__ void __launch_bounds__(512, 2) attention_bwd_bf16_blk(const BwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Lds s(smem, BR);
    const int N = a.N, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Lane w(tid & 63, a.scale);
    const int blk = blockIdx.x % a.nblk, bh = blockIdx.x / a.nblk;
    const Head hd(a, bh / a.H, bh % a.H);
    const int r_res = blk * BR;                                  // first row of the resident block
    const int lrow = wave * 32 + w.c32, row = r_res + lrow;      // this lane's resident row: in the images, in the sequence
    const bool live = r_res + wave * 32 < N;                     // wave-uniform: this wave's 32 resident rows hold a token

    stage<ROLE == 0, ROLE == 1>(hd, s, r_res, BR, tid);
    f32x16 acc[2] = {}, dv[2] = {};                              // ROLE 0: dK^T, dV^T; ROLE 1: dQ^T (dv unused)
    const float *L2k = row < N ? s.L2s : s.Linf;                 // ROLE 0: a padded key reads +inf for every row's L2 (see the kernel above)
    for (int sb = 0; sb < a.nblk; ++sb) {
        if (sb) __syncthreads();                                 // the previous streamed block is consumed
        stage<ROLE == 1, ROLE == 0>(hd, s, sb * BR, BR, tid);
        __syncthreads();
        if (!live) continue;                                     // (every wave still reaches both barriers)
        bf16x8 fa[4], fb[4];                                     // ROLE 0: kf, vf; ROLE 1: qf, gf
        load_frags(ROLE == 0 ? s.Ks : s.Qs, ROLE == 0 ? s.Vs : s.Gs, lrow, w.h, fa, fb);
        const int left = N - sb * BR < BR ? N - sb * BR : BR;    // streamed rows that hold a token
        if (ROLE == 0) {
            for (int i = 0; i < (left + 31) >> 5; ++i) phase1_block(s, i * 32, fa, fb, L2k, acc, dv, w);
        } else {
            const float l2 = s.L2s[lrow], de = s.dlt[lrow];
            for (int j = 0; j < left >> 5; ++j) phase2_block<false>(s, j * 32, fa, fb, l2, de, 32, acc, w);
        }
    }
    // ROLE 1: the last, partial block of 32 keys of the sequence, peeled behind the loop nest (the K / V images still hold its
    // block).  Behind the full sub-blocks of the last streamed block instead it measured +1.5 % at N = 1025.
    if (ROLE == 1 && live && (N & 31)) {
        bf16x8 qf[4], gf[4];
        load_frags(s.Qs, s.Gs, lrow, w.h, qf, gf);
        const int left = N - (a.nblk - 1) * BR;
        phase2_block<true>(s, (left >> 5) * 32, qf, gf, s.L2s[lrow], s.dlt[lrow], left & 31, acc, w);
    }
    if (live && row < N) {
        store_row(ROLE == 0 ? hd.dk : hd.dq, row, hd.lddqkv, acc, w.h);
        if (ROLE == 0) store_row(hd.dv, row, hd.lddqkv, dv, w.h);
    }
}

template <void (*KERN)(BwdArgs)>
int launch(const BwdArgs &a, int grid, int lds, hipStream_t stream)
{
    LDIT_DYN_LDS(KERN, LDS_MAX);
    hipLaunchKernelGGL(KERN, dim3((unsigned)grid), dim3(512), lds, stream, a);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // namespace

int launch_attention_bwd_bf16(const void *Q, const void *K, const void *V, const void *O, const void *dO, const float *lse,
                              void *dQ, void *dK, void *dV, int B, int N, int H, int D, int ldqkv, int ldo, int lddo, int lddqkv,
                              float scale, hipStream_t stream)
{
    if (B <= 0 || N <= 0 || H <= 0) return fail(LDIT_EINVAL, "attention_bwd: empty problem");
    if (D != 64) return fail(LDIT_EUNSUPPORTED, "attention_bwd: head_dim=%d, only 64 is implemented", D);
    if (!Q || !K || !V || !O || !dO || !lse || !dQ || !dK || !dV) return fail(LDIT_EINVAL, "attention_bwd: null operand");
    if ((ldqkv | ldo | lddo) & 7 || (lddqkv & 3)) return fail(LDIT_EINVAL, "attention_bwd: row strides must be multiples of 8 (in) / 4 (out)");
    if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(O) || !aligned16(dO) ||
        ((reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dK) | reinterpret_cast<uintptr_t>(dV)) & 7u))
        return fail(LDIT_EINVAL, "attention_bwd: operands must be 16-byte (inputs) / 8-byte (outputs) aligned");
    const int nblk = (N + BR - 1) / BR;
    const BwdArgs a{static_cast<const bf16_t *>(Q), static_cast<const bf16_t *>(K), static_cast<const bf16_t *>(V),
                    static_cast<const bf16_t *>(O), static_cast<const bf16_t *>(dO), lse, static_cast<bf16_t *>(dQ),
                    static_cast<bf16_t *>(dK), static_cast<bf16_t *>(dV), N, H, nblk, ldqkv, ldo, lddo, lddqkv, scale};
    if (nblk > 1) {
        // blocked form: one launch per role, a workgroup per (image, head, 256-row block)
        if (int rc = launch<attention_bwd_bf16_blk<0>>(a, B * H * nblk, LDS_MAX, stream)) return rc;
        return launch<attention_bwd_bf16_blk<1>>(a, B * H * nblk, LDS_MAX, stream);
    }
    const int NP = ((N + 31) / 32) * 32;
    return launch<attention_bwd_bf16>(a, B * H, 4 * NP * ROWB + 3 * NP * 4, stream);
}

}  // namespace ldit
