// Fused multi-head self-attention forward on the bf16 MFMA, fp32 softmax:  O = softmax(Q K^T * scale) V  per (image, head), no mask.
// ONE kernel body (flash_body) for the bf16, fp8, mxfp8 and train builds (one bf16 plane per operand) and for the split-fp32 builds
// (two or three planes, see "Planes" below).  D = 64, any N (flash-style chunks of 64 keys with the online-softmax rescale; N = 1025
// for ViT-L at 512x512 is 17 chunks).
// Q, K, V: bf16 column slices of the fused [B*N, 3C] projection; O: [B*N, C] in the output form of the build (store_o).
//
// Same transposed formulation as attention_f32.hip, on v_mfma_f32_32x32x16_bf16:
//   S^T[key][query] = K . Q^T     A = K fragment (LDS b128: 8 consecutive d of one key), B = Q^T fragment (registers)
//   O^T[d][query]   = V^T . P^T   A = V^T fragment (two ds_read_b64_tr_b16: 4 + 4 keys of one d), B = P^T = the S^T accumulator
// A lane (query j, half h) of an S^T tile holds, in registers 8s..8s+7, the keys 16s + 8(jj>>2) + 4h + (jj&3) - packed
// pairwise to bf16 they ARE the B-operand fragment of k-step s of the second product, provided the A operand uses the
// same key order: the transposing LDS read delivers exactly that (rows = 4 consecutive keys starting at 16s + 8u + 4h,
// columns = the 16 d of the lane group), so V stays key-major in LDS, P never touches LDS and nothing is shuffled.
// K and V chunks are staged by LDS-DMA (lds_dma.h: no registers, no scatter writes) into a double buffer: chunk
// c+1 flies while chunk c is multiplied, with a single workgroup barrier per chunk.  K image: 128-B rows, 16-B chunk XOR-swizzled with (row>>1)&7 (conflict-free
// b128 reads); V image: 256-B blocks [4 keys][32 d] - one transposing read of a 32-lane half is exactly one block, i.e.
// one full sweep of the 64 banks.  Rows past N are clamped duplicates of the last key and masked to -inf.
// Softmax runs on raw scores in the exp2 domain (p = exp2(s c - m c), c = scale log2 e: one FMA + one v_exp_f32 per
// element), fp32, lane-local apart from one lane<->lane+32 exchange.  One plane: four waves (128 queries) per workgroup, 32 KB of
// LDS and 128 VGPRs: four workgroups per CU, so on every SIMD one wave's softmax VALU work overlaps another's MFMAs.
//
// Planes (include/ldit.h, LDIT_F32X3 / LDIT_F32X6): every operand of both products is held as TWO (THREE) bf16 planes
// x ~= p0 + p1 (+ p2) and every product is formed from three (six) plane products with fp32 accumulation.  Why: with the GEMMs of
// that build on the bf16 matrix pipe, the fp32-MFMA attention kernel (attention_f32.hip, 1/16 of the bf16 matrix rate, 110 us per
// ViT-B layer at bs=64) had become 16 % of the step.  The structure above, PRE only, with
//   * K and V chunks staged per plane (four / six 8-KB images per stage, 64 / 96 KB per workgroup),
//   * three (six) MFMAs per (key tile, 16-deep step): k1.q0 + k0.q1 + k0.q0, smallest first (n_products / prod_x / prod_y),
//   * P split in registers: p0 = bf16(p), p1 = bf16(p - p0) - two conversions and one subtraction per score,
//   * O written as the bf16 planes of its fp32 value (operand of the o_proj GEMM).
// Layouts: Q, K, V = plane-major column slices of the q|k|v GEMM's output [B*N, S * 3C] (plane s of a row at column s * plane_in);
// O = [B*N, S * C] (plane s at column s * H * 64).
// ONE workgroup of eight waves (256 queries) per CU: two waves per SIMD (169 / 217 registers), and one staging of a chunk serves all
// seven query tiles of a 197-token image.  (Four-wave workgroups, two per CU: 3 % slower with two planes; with three planes the LDS
// allows only one of them per CU and the kernel ran no faster than the fp32-MFMA attention: 1.42 vs 1.06 ms per ViT-B forward.)
#include <cstdlib>
#include <type_traits>

#include "ldit_common.h"
#include "lds_dma.h"

#ifdef LDIT_GEMM_STAMPS
// diagnostic build only (make dbg; scripts/attn_stamps.py): per-workgroup phase cycles of wave 0, written to a buffer
// registered by ldit_dbg_set_attn_stamps - 6 x int64 per workgroup: wait+barrier, DMA issue, S = K Q^T issue,
// softmax (incl. the wait for S), P V, kernel total
__device__ unsigned long long *g_attn_stamps = nullptr;
#define ATT_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define ATT_STAMP(var)
#endif

namespace ldit {

namespace {

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int KROWB = 128;                  // bytes per K row in LDS (64 bf16)
constexpr int KC = 64, HALF = KC * KROWB;   // keys per chunk (two 32-key tiles); one plane image of K or V
constexpr int PIECES = KC / 8;              // 1-KB DMA pieces (8 keys) per image
// (128-key chunks - 64 KB, 240 VGPRs, two workgroups per CU - measured 8-10 % slower at N = 197 and N = 1025: removed)

// The plane products of one fp32 product, smallest first (ldit.h): one plane -> x0 y0; two planes -> x1 y0 + x0 y1 + x0 y0; three
// planes -> x2 y0 + x1 y1 + x0 y2 + x1 y0 + x0 y1 + x0 y0.
constexpr int n_products(int planes) { return planes == 1 ? 1 : planes == 2 ? 3 : 6; }
constexpr int prod_x(int planes, int g) { return planes == 1 ? 0 : planes == 2 ? (g == 0 ? 1 : 0) : (g == 0 ? 2 : g == 1 ? 1 : g == 3 ? 1 : 0); }
constexpr int prod_y(int planes, int g) { return planes == 1 ? 0 : planes == 2 ? (g == 1 ? 1 : 0) : (g == 1 ? 1 : g == 2 ? 2 : g == 4 ? 1 : 0); }

// The output forms (AttnOut): what a lane does with its query row's 2 x 16 accumulators o[dt][4 g + e] = column 32 dt + 8 g + 4 h + e
// of the head.  `row` = the token row, `col` = the head's first column, `live` = the row exists (rows past N are computed, not stored).
//   ATTN_BF16      bf16 [rows, ldo]
//   ATTN_FP8       fp8 e4m3 codes of o / *qscale (operand of the fp8 o_proj GEMM; `inv` carries the factor), ldo in elements
//   ATTN_MX        MX codes + E8M0 block scales Os [rows, ldo / 32] (ldit.h, LDIT_MXFP8): a lane holds 16 columns of each 32-column
//                  block dt of its query row, lane l ^ 32 the other 16 - one exchange gives the block amax
//   ATTN_MX_TRAIN  (mxfp8 train step) also Ob, the bf16 O before quantisation (what ATTN_BF16 writes: the backward's rowsum(dO o O)
//                  operand), and Od, the bf16 dequantised codes (the o_proj wgrad's operand)
//   ATTN_PLANES    the PLANES bf16 planes of the fp32 value, plane s at column s * H * 64
template <int PLANES, AttnOut OUT>
__device__ __forceinline__ void store_o(f32x16 (&o)[2], float inv, bool live, size_t row, int col, int h, int H, void *Ov, int ldo,
                                        unsigned char *Os, bf16_t *Ob, bf16_t *Od)
{
    if constexpr (OUT == ATTN_MX || OUT == ATTN_MX_TRAIN) {
        constexpr bool TR = OUT == ATTN_MX_TRAIN;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            unsigned amax = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                o[dt][e] *= inv;
                amax = umax32(amax, __float_as_uint(o[dt][e]) & 0x7fffffffu);
            }
            if (TR && live) {
                bf16_t *ob = Ob + row * ldo + col + dt * 32 + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<bf16x4 *>(ob + 8 * g) = bf16x4{(bf16_t)o[dt][4 * g + 0], (bf16_t)o[dt][4 * g + 1],
                                                                     (bf16_t)o[dt][4 * g + 2], (bf16_t)o[dt][4 * g + 3]};
            }
            amax = umax32(amax, (unsigned)__shfl_xor((int)amax, 32, 64));
            const unsigned sb = mx_scale_byte(amax);
            const float qi = mx_inv_scale(sb);
            if (live) {
                unsigned char *op = static_cast<unsigned char *>(Ov) + row * ldo + col + dt * 32 + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned pk = pack_fp8x4(o[dt][4 * g + 0] * qi, o[dt][4 * g + 1] * qi, o[dt][4 * g + 2] * qi, o[dt][4 * g + 3] * qi);
                    *reinterpret_cast<unsigned *>(op + 8 * g) = pk;
                    if (TR) *reinterpret_cast<mx_bf16x4 *>(Od + row * ldo + col + dt * 32 + 4 * h + 8 * g) = mx_dequant_bf16x4(pk, sb);
                }
                if (h == 0) Os[row * (ldo >> 5) + ((col + dt * 32) >> 5)] = (unsigned char)sb;
            }
        }
    } else if constexpr (OUT == ATTN_FP8) {
        if (live) {
            unsigned char *op = static_cast<unsigned char *>(Ov) + row * ldo + col + 4 * h;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<unsigned *>(op + dt * 32 + 8 * g) =
                        pack_fp8x4(o[dt][4 * g + 0] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
        }
    } else if (live) {
        bf16_t *op = static_cast<bf16_t *>(Ov) + row * ldo + col + 4 * h;
        const int plane = H * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 t = {o[dt][4 * g + 0] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv};
#pragma unroll
                for (int sp = 0; sp < PLANES; ++sp) {
                    const bf16x4 pk = {(bf16_t)t[0], (bf16_t)t[1], (bf16_t)t[2], (bf16_t)t[3]};
                    *reinterpret_cast<bf16x4 *>(op + sp * plane + dt * 32 + 8 * g) = pk;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] -= (float)pk[e];
                }
            }
    }
}

// PRE (round 3): Q arrives already multiplied by scale * log2(e) (the packed inference path folds that factor into W_q / b_q at
// pack time: api.hip, ldit_pack_weights), so a raw score IS its exp2-domain exponent, and the running maximum is subtracted
// BY THE MATRIX PIPE: one extra MFMA step per key tile with an all-ones A column and B = (-m_hi, -m_lo) (the maximum split into
// two bf16 so that 2^-17 |m| is all it loses) initialises the S^T accumulators with -m_run.  p = exp2(S') then needs no
// per-element FMA: 32 of the ~180 VALU instructions of a chunk, on a kernel whose four waves per SIMD saturate instruction
// issue (PMC: SQ_ACTIVE_INST_ANY x 4 waves = 1.07 of the SIMD's cycles; MFMA pipe 32 % busy).
// PLANES > 1 is PRE only.  Row strides ldq / ldk / ldv and the plane distance plane_in are in elements.
template <int PLANES, int NW, bool PRE, AttnOut OUT>
__device__ __forceinline__ void flash_body(const bf16_t *Q, const bf16_t *K, const bf16_t *V, void *Ov, int N, int H, int ldq, int ldk,
                                           int ldv, int plane_in, int ldo, float scale, int nqg, const float *qscale, float *lse,
                                           unsigned char *Os, bf16_t *Ob, bf16_t *Od)
{
    static_assert(PRE || PLANES == 1, "plane operands come pre-scaled");
    constexpr int STAGE = 2 * PLANES * HALF, NPROD = n_products(PLANES);    // a stage: the K images of every plane, then the V images
    constexpr int PPW = PIECES / NW;                                        // DMA pieces per image and wave
    static_assert(PIECES % NW == 0, "DMA pieces must split evenly over the waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c32 = lane & 31, h = lane >> 5;
    const int bid = blockIdx.x;
    const int qg = bid % nqg, bh = bid / nqg, head = bh % H, b = bh / H;
    const int qt = qg * NW + wave;
    const bool active = qt * 32 < N;                   // wave-uniform
    const size_t tok0 = (size_t)b * N;

    // Q^T fragments per plane: lane (query c32, half h), k-step s holds Q[query][16s + 8h .. +7]
    bf16x8 qf[PLANES][4];
    {
        int qrow = qt * 32 + c32;
        qrow = qrow < N ? qrow : N - 1;
        const bf16_t *qp = Q + (tok0 + qrow) * ldq + head * 64 + 8 * h;
#pragma unroll
        for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
            for (int s = 0; s < 4; ++s) qf[pl][s] = *reinterpret_cast<const bf16x8 *>(qp + pl * plane_in + 16 * s);
        // retire these loads HERE: left pending, hipcc guards their first use inside the chunk loop with s_waitcnt vmcnt(0),
        // which would also drain the DMA of the next chunk on every iteration
#pragma unroll
        for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
            for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(qf[pl][s]));
    }

    // DMA source geometry of this lane.  K piece: 8 keys x 128 B, lane -> key lane>>3, source chunk (lane&7) ^ swizzle.
    // V piece: 8 keys x 128 B as four 256-B blocks [4 keys][32 d]: lane -> block lane>>4 (key group (lane>>5), d half
    // (lane>>4)&1), key (lane&15)>>2 of the group, 16-B piece lane&3 of the 64-B half row.
    const int kkey = lane >> 3, vkey = 4 * (lane >> 5) + ((lane & 15) >> 2);
    const int vd = 32 * ((lane >> 4) & 1) + 8 * (lane & 3);
    const bf16_t *Kh = K + tok0 * ldk + head * 64, *Vh = V + tok0 * ldv + head * 64;
    // Per-lane source offsets inside a chunk are constants of the kernel; the chunk's base address is wave-uniform and advances
    // in scalar registers, so issuing a chunk costs no vector address arithmetic (round 2 recomputed the clamp, the row
    // product and a 64-bit add per piece: ~30 VALU instructions per chunk on a kernel that is VALU-issue bound).  Only a chunk
    // that reaches past key N-1 (the short last one) takes the clamped path (rows past N = duplicates of the last key).
    // (piece u of a wave is 8 NW keys further down: the XOR swizzle term (krow >> 1) & 7 does not change, so ONE offset per
    // operand serves every piece and every plane - the step goes into the scalar base)
    static_assert((8 * NW) % 16 == 0, "pieces of one wave must share the swizzle phase");
    const unsigned koff = (unsigned)(8 * wave + kkey) * (unsigned)ldk + 8u * ((lane & 7) ^ (((8 * wave + kkey) >> 1) & 7));   // elements
    const unsigned voff = (unsigned)(8 * wave + vkey) * (unsigned)ldv + (unsigned)vd;
    auto issue = [&](int stage, int c0) {
        char *sb = smem + stage * STAGE;
        if (c0 + KC <= N) {                              // wave-uniform
            const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)((__attribute__((address_space(3))) char *)sb));
#pragma unroll
            for (int u = 0; u < PPW; ++u) {
                const int piece = wave + NW * u;
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl) {
                    const bf16_t *kbase = Kh + (size_t)(c0 + 8 * NW * u) * ldk + pl * plane_in;
                    const bf16_t *vbase = Vh + (size_t)(c0 + 8 * NW * u) * ldv + pl * plane_in;
                    glds16_sbase(kbase, 2u * koff, dst + pl * HALF + piece * 1024);
                    glds16_sbase(vbase, 2u * voff, dst + (PLANES + pl) * HALF + piece * 1024);
                }
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < PPW; ++u) {
            const int piece = wave + NW * u;
            const int krow = 8 * piece + kkey;
            int key = c0 + krow;
            key = key < N ? key : N - 1;
            int vk = c0 + 8 * piece + vkey;
            vk = vk < N ? vk : N - 1;
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) {
                glds16(Kh + (size_t)key * ldk + pl * plane_in + 8 * ((lane & 7) ^ ((krow >> 1) & 7)), sb + pl * HALF + piece * 1024);
                glds16(Vh + (size_t)vk * ldv + pl * plane_in + vd, sb + (PLANES + pl) * HALF + piece * 1024);
            }
        }
    };

    f32x16 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { o[0][e] = 0.0f; o[1][e] = 0.0f; }
    float m_run = PRE ? 0.0f : -INFINITY, l_run = 0.0f;
    const float c = scale * 1.44269504088896340736f;     // softmax in the exp2 domain (PRE: already inside q)
    const float lazy = PRE ? 8.0f : 8.0f / c;            // deferred-rescale threshold in score units (2^8 in the exp2 domain)
    // PRE: operands of the extra MFMA step.  A = 1 at k = 0, 1 for every key row; B = (-m_hi, -m_lo) at k = 0, 1 of the lane's
    // query (k = 8 h + j: only the h = 0 half carries them).
    // (the step runs on v_mfma_f32_32x32x8_bf16 - lane (row, h) supplies k = 4 h + j, j < 4 - so its operands are two registers
    // each: A = all ones, B = (-m_hi, -m_lo, 0, 0) in the h = 0 half, zeros in the other)
    // (Row sums on the matrix pipe - an all-ones A operand per 16-key step - were built and measured: 112.5 us against 106.2 us
    // at N = 1025; four more MFMAs per chunk cost more than the 16 v_pk_add_f32 they replace.  Not kept.)
    bf16x4 ones4 = {(bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f, (bf16_t)1.0f};
    bf16x4 mfrag = {(bf16_t)0.0f, (bf16_t)0.0f, (bf16_t)0.0f, (bf16_t)0.0f};
    const int sw = (c32 >> 1) & 7;
    // transposing read: lane 4q+p of a 16-lane group addresses key q, d 4p..4p+3 of the group's 16 columns
    const int vlane = 64 * ((lane & 15) >> 2) + 32 * ((lane >> 4) & 1) + 8 * (lane & 3) + 512 * h;

    const int nchunks = (N + KC - 1) / KC;
#ifdef LDIT_GEMM_STAMPS
    unsigned long long tw = 0, ti = 0, ts = 0, tx = 0, tp = 0;
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
#endif
    issue(0, 0);
    // One chunk: wait for its K/V images, start the next chunk's DMA, multiply.  Instantiated per number of live 32-key tiles
    // so that the score registers are straight-line values inside it (per-tile `if (kt < ktiles)` guards made every tile a
    // phi and cost ~40 v_mov per chunk): the loop below runs the full chunks, the short last chunk is peeled behind it (a
    // last chunk of N = 197 skips its dead tile).  Two instantiations INSIDE the loop spill at 128 registers; peeled they do not.
    auto step = [&](const int ci, auto nkt_c) {
        constexpr int NKT = decltype(nkt_c)::value;
        ATT_STAMP(t0);
        const int c0 = ci * KC;
        const int nkeys = (N - c0) < KC ? (N - c0) : KC;
        // ONE barrier per chunk: behind it every wave's pieces of chunk ci have landed AND every wave has finished
        // multiplying chunk ci-1 (program order), so the other stage is free - chunk ci+1 is issued right here and has the
        // whole of chunk ci's arithmetic to land.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        ATT_STAMP(t1);
        if (ci + 1 < nchunks) issue((ci + 1) & 1, c0 + KC);
        ATT_STAMP(t2);
#ifdef LDIT_GEMM_STAMPS
        tw += t1 - t0; ti += t2 - t1;
#endif
        if (active) {
            const char *Ks = smem + (ci & 1) * STAGE;
            const char *Vs = Ks + PLANES * HALF;
            {
                // ---- S^T = K . Q^T over the plane products, smallest first ------------------------------------------------------
                f32x16 s[NKT];
                const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
                    const char *kr = Ks + (kt * 32 + c32) * KROWB;
                    if (PRE) {
                        union { bf16x4 f; s16x4 v; } ua, ub;
                        ua.f = ones4; ub.f = mfrag;
                        s[kt] = __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(ua.v, ub.v, zero16, 0, 0, 0);      // = -m_run
                    }
#pragma unroll
                    for (int st = 0; st < 4; ++st) {
                        bf16x8 kf[PLANES];
#pragma unroll
                        for (int pl = 0; pl < PLANES; ++pl) kf[pl] = *reinterpret_cast<const bf16x8 *>(kr + pl * HALF + (((2 * st + h) ^ sw) * 16));
#pragma unroll
                        for (int g = 0; g < NPROD; ++g)
                            s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[prod_x(PLANES, g)], qf[prod_y(PLANES, g)][st],
                                                                            (PRE || st || g) ? s[kt] : zero16, 0, 0, 0);
                    }
                }
                ATT_STAMP(t3);
                // ---- mask padded keys (last chunk only: a real branch, not 2 VALU ops on every score), running max on
                //      the raw scores (scale > 0 commutes with max) ------------------------------------------------------
                if (nkeys < NKT * 32) {
#pragma unroll
                    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if ((kt * 32 + 8 * (r >> 2) + 4 * h + (r & 3)) >= nkeys) s[kt][r] = -INFINITY;
                }
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kt][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                // Deferred rescale: the running maximum only moves when a chunk beats it by more than 2^8 in the exp2
                // domain (always on the first chunk, m_run = -inf).  Until then p = exp2(c s - c m_run) may exceed 1 by up
                // to 2^8 - harmless in fp32 sums and in bf16 P (a power-of-two scale of the same mantissas) - and the 32
                // accumulator multiplies, the alpha exp2 and the l rescale are skipped behind a wave-uniform branch.
                float lsum = 0.0f;
                if constexpr (PRE) {
                    // s holds S' = score - m_run.  The maximum moves on the first chunk (m_run = 0 there: whatever the scores
                    // are, they are re-based on their own maximum) and when a chunk beats it by 2^8.  Everything still at the
                    // old maximum is moved exactly once: O, the row sum, THIS chunk's S' and the MFMA operand that carries m.
                    const bool grow = ci == 0 || mx > lazy;
                    if (__builtin_amdgcn_ballot_w64(grow)) {
                        // the new maximum as the sum of two bf16 (what the extra MFMA step can carry); d = the exact shift applied
                        const float want = grow ? m_run + mx : m_run;
                        const bf16_t hi = (bf16_t)(-want);
                        const bf16_t lo = (bf16_t)(-want - (float)hi);
                        const float m_new = -((float)hi + (float)lo);
                        const float d = m_new - m_run;                   // exactly 0 for lanes that keep m_run (same hi, lo)
                        // first chunk: O and the row sum are zero, and exp2(-d) may overflow for very negative scores
                        const float alpha = ci == 0 ? 1.0f : __builtin_amdgcn_exp2f(-d);
                        m_run = m_new;
                        if (h == 0) { mfrag[0] = hi; mfrag[1] = lo; }
                        l_run *= alpha;
#pragma unroll
                        for (int e = 0; e < 16; ++e) { o[0][e] *= alpha; o[1][e] *= alpha; }
#pragma unroll
                        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) s[kt][r] -= d;
                    }
#pragma unroll
                    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float pv = __builtin_amdgcn_exp2f(s[kt][r]);
                            s[kt][r] = pv;
                            lsum += pv;
                        }
                } else {
                    const bool grow = mx > m_run + lazy;
                    if (__builtin_amdgcn_ballot_w64(grow)) {
                        const float m_new = grow ? mx : m_run;
                        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);      // 1 for lanes that keep m_run
                        m_run = m_new;
                        l_run *= alpha;
#pragma unroll
                        for (int e = 0; e < 16; ++e) { o[0][e] *= alpha; o[1][e] *= alpha; }
                    }
                    const float mc = m_run * c;
#pragma unroll
                    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][r], c, -mc));
                            s[kt][r] = pv;
                            lsum += pv;
                        }
                }
                l_run += lsum;
                ATT_STAMP(t4);
                // ---- O^T += V^T . P^T over the plane products ---------------------------------------------------------------------
                // The transposing reads are inline asm: through the builtin, hipcc cannot tell that they do not alias the
                // LDS-DMA writes of the NEXT chunk and guards each group with s_waitcnt vmcnt(0), which would serialise
                // the double buffer.  Asm reads are invisible to the compiler's waitcnt pass, hence the explicit
                // lgkmcnt(0) and the sched_barrier that keeps the MFMAs below it.
                // A read group = the V fragments of SG 16-key steps, all in front of the group's MFMAs: one plane reads a whole key
                // tile (SG = 2), planes read per step (SG = 1) - the other grouping spills, either way round.
                constexpr int SG = PLANES == 1 ? 2 : 1;
                const unsigned vaddr = (unsigned)(uintptr_t)((__attribute__((address_space(3))) const char *)(Vs + vlane));
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
                    for (int st0 = 0; st0 < 2; st0 += SG) {
                        // block (key group, d half) = ((32 kt + 16 st + 8 u + 4 h) / 4) * 2 + dt; h is in vlane
                        s16x4 vr[SG][PLANES][2][2];        // [step][plane][dt][u]
#pragma unroll
                        for (int i = 0; i < SG; ++i)
#pragma unroll
                            for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
                                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                                    for (int u = 0; u < 2; ++u)
                                        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
                                                     : "=v"(vr[i][pl][dt][u])
                                                     : "v"(vaddr), "n"(pl * HALF + (16 * kt + 8 * (st0 + i) + 4 * u + dt) * 256));
                        // P^T fragments: p0 = bf16(p), p1 = bf16(p - p0), ...
                        bf16x8 pp[SG][PLANES];
#pragma unroll
                        for (int i = 0; i < SG; ++i)
#pragma unroll
                            for (int jj = 0; jj < 8; ++jj) {
                                float pv = s[kt][8 * (st0 + i) + jj];
#pragma unroll
                                for (int pl = 0; pl < PLANES; ++pl) {
                                    pp[i][pl][jj] = (bf16_t)pv;
                                    pv -= (float)pp[i][pl][jj];
                                }
                            }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int i = 0; i < SG; ++i)
#pragma unroll
                            for (int dt = 0; dt < 2; ++dt) {
                                union { s16x4 v[2]; bf16x8 f; } vf[PLANES];
#pragma unroll
                                for (int pl = 0; pl < PLANES; ++pl) { vf[pl].v[0] = vr[i][pl][dt][0]; vf[pl].v[1] = vr[i][pl][dt][1]; }
#pragma unroll
                                for (int g = 0; g < NPROD; ++g)
                                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[prod_x(PLANES, g)].f, pp[i][prod_y(PLANES, g)], o[dt], 0, 0, 0);
                            }
                    }
                }
#ifdef LDIT_GEMM_STAMPS
                asm volatile("s_nop 0" :: "v"(o[0][0]), "v"(o[1][0]));
                const unsigned long long t5 = __builtin_amdgcn_s_memtime();
                ts += t3 - t2; tx += t4 - t3; tp += t5 - t4;
#endif
            }
        }
    };
    const int last_tiles = (N - (nchunks - 1) * KC + 31) >> 5;
    for (int ci = 0; ci + 1 < nchunks; ++ci) step(ci, std::integral_constant<int, 2>{});
    if (last_tiles == 2) step(nchunks - 1, std::integral_constant<int, 2>{});
    else step(nchunks - 1, std::integral_constant<int, 1>{});

#ifdef LDIT_GEMM_STAMPS
    if (g_attn_stamps && wave == 0 && lane == 0) {
        unsigned long long *d = g_attn_stamps + (size_t)blockIdx.x * 6;
        d[0] = tw; d[1] = ti; d[2] = ts; d[3] = tx; d[4] = tp; d[5] = __builtin_amdgcn_s_memtime() - t_begin;
    }
#endif
    if (!active) return;
    const float l = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = OUT == ATTN_FP8 ? 1.0f / (l * qscale[0]) : 1.0f / l;
    const int qrow = qt * 32 + c32;
    // train step: log2-domain log-sum-exp of the scaled scores, L2 = log2 sum_k exp2(c s_k) = m c + log2 l, so that the
    // backward recomputes p = exp2(c s - L2) with no row maximum (layout [B, H, N])
    if (lse && h == 0 && qrow < N) lse[((size_t)b * H + head) * N + qrow] = (PRE ? m_run : m_run * c) + __builtin_amdgcn_logf(l);
    store_o<PLANES, OUT>(o, inv, qrow < N, tok0 + qrow, head * 64, h, H, Ov, ldo, Os, Ob, Od);
}

// Thin entry points, one parameter list per family.  scale: the softmax factor, applied here unless PRE.
template <int NW, bool PRE, AttnOut OUT>
__global__ void __launch_bounds__(NW * 64, 4) attention_bf16(const bf16_t *__restrict__ Q, const bf16_t *__restrict__ K,
                                                             const bf16_t *__restrict__ V, void *__restrict__ Ov,
                                                             int N, int H, int ldq, int ldk, int ldv, int ldo,
                                                             float scale, int nqg, const float *__restrict__ qscale,
                                                             float *__restrict__ lse, unsigned char *__restrict__ Os,
                                                             bf16_t *__restrict__ Ob, bf16_t *__restrict__ Od)
{
    flash_body<1, NW, PRE, OUT>(Q, K, V, Ov, N, H, ldq, ldk, ldv, 0, ldo, scale, nqg, qscale, lse, Os, Ob, Od);
}

template <int PLANES, int NW>
__global__ void __launch_bounds__(NW * 64, 2) attention_planes(const bf16_t *__restrict__ Q, const bf16_t *__restrict__ K,
                                                                const bf16_t *__restrict__ V, bf16_t *__restrict__ O, int N, int H,
                                                                int ld_in, int plane_in, int ldo, int nqg)
{
    flash_body<PLANES, NW, true, ATTN_PLANES>(Q, K, V, O, N, H, ld_in, ld_in, ld_in, plane_in, ldo, 0.0f, nqg, nullptr, nullptr, nullptr,
                                              nullptr, nullptr);
}

// LDS = two stages of (K images + V images): 32 KB per plane.
template <int PLANES, int NW, bool PRE, AttnOut OUT>
int launch_one(const AttnArgs &a, hipStream_t stream)
{
    constexpr int lds = 2 * 2 * PLANES * HALF;
    static std::atomic<unsigned long long> attr_done{0};      // per-device bookkeeping (ensure_dynamic_lds)
    const int nqt = (a.N + 31) / 32, nqg = (nqt + NW - 1) / NW;
    const dim3 grid((unsigned)(a.B * a.H * nqg)), block(NW * 64);
    const bf16_t *Q = static_cast<const bf16_t *>(a.Q), *K = static_cast<const bf16_t *>(a.K), *V = static_cast<const bf16_t *>(a.V);
    if constexpr (PLANES == 1) {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(attention_bf16<NW, PRE, OUT>), lds, attr_done)) return rc;
        hipLaunchKernelGGL((attention_bf16<NW, PRE, OUT>), grid, block, lds, stream, Q, K, V, a.O, a.N, a.H, a.ldq, a.ldk, a.ldv, a.ldo, a.scale,
                           nqg, a.qscale, a.lse, static_cast<unsigned char *>(a.Os), static_cast<bf16_t *>(a.Ob), static_cast<bf16_t *>(a.Od));
    } else {
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(attention_planes<PLANES, NW>), lds, attr_done)) return rc;
        hipLaunchKernelGGL((attention_planes<PLANES, NW>), grid, block, lds, stream, Q, K, V, static_cast<bf16_t *>(a.O), a.N, a.H, a.ldq,
                           a.plane_in, a.ldo, nqg);
    }
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

// The instantiation table.  One plane: scale == 0 means Q is pre-multiplied by scale * log2(e) (PRE, the packed inference path),
// otherwise the factor is applied in the kernel.  64-key chunks: 32 KB and 128 VGPRs -> four workgroups per CU (four waves per SIMD).
// (eight query tiles per workgroup - half the DMA pieces and K/V traffic per tile - measured equal: 108.6 vs 107.8 us at N = 1025)
// Round 3: five to eight query tiles (N = 129 .. 256: the 197 tokens of a 224 x 224 image) run as ONE eight-wave workgroup per
// (image, head) - one staging of every chunk instead of two, no half-empty second workgroup: 27.3 -> 23.5 us at bs=64, 16.2 -> 14.7 us
// at bs=32 (scripts/attn_bf16_bench.py, interleaved); long sequences stay on four-wave workgroups (N = 1025: 102.6 vs 105 us).  A
// query tile's arithmetic does not depend on its workgroup: bit-identical either way (LDIT_ATTN_BF16_NW = 4 / 8 forces one).
// Planes: always pre-scaled, always eight waves (see the header).
template <int PLANES, AttnOut OUT>
int launch_form(const AttnArgs &a, hipStream_t stream)
{
    if constexpr (PLANES > 1) return launch_one<PLANES, 8, true, OUT>(a, stream);
    else {
        const int nqt = (a.N + 31) / 32, force_nw = diag().attn_bf16_nw;
        const bool wide = force_nw == 8 || (force_nw != 4 && nqt > 4 && nqt <= 8), pre = a.scale == 0.0f;
        if (pre) return wide ? launch_one<1, 8, true, OUT>(a, stream) : launch_one<1, 4, true, OUT>(a, stream);
        return wide ? launch_one<1, 8, false, OUT>(a, stream) : launch_one<1, 4, false, OUT>(a, stream);
    }
}

}  // namespace

int launch_attention_flash(const AttnArgs &a, hipStream_t stream)
{
    const bool planes = a.out == ATTN_PLANES, fp8 = a.out == ATTN_FP8 || a.out == ATTN_MX || a.out == ATTN_MX_TRAIN;
    const char *name = planes ? "attention_planes" : "attention_bf16";
    if (planes ? (a.planes != 2 && a.planes != 3) : a.planes != 1) return fail(LDIT_EINVAL, "%s: %d planes in this output form", name, a.planes);
    // what the output form needs
    if (a.out == ATTN_FP8 && !a.qscale) return fail(LDIT_EINVAL, "attention_bf16: fp8 output needs a scale");
    if (a.out == ATTN_MX && (!a.Os || (a.ldo & 31))) return fail(LDIT_EINVAL, "attention_bf16: MX output needs block scales and ldo %% 32 == 0");
    if (a.out == ATTN_MX_TRAIN) {
        if (!a.Os || !a.lse || !a.Ob || !a.Od || (a.ldo & 31)) return fail(LDIT_EINVAL, "attention_bf16: MX train output needs Os, lse, Ob, Od and ldo %% 32 == 0");
        if ((reinterpret_cast<uintptr_t>(a.Ob) | reinterpret_cast<uintptr_t>(a.Od)) & 7u) return fail(LDIT_EINVAL, "attention_bf16: Ob / Od must be 8-byte aligned");
    }
    if (a.B <= 0 || a.N <= 0 || a.H <= 0) return fail(LDIT_EINVAL, "%s: empty problem", name);
    if (a.D != 64) return fail(LDIT_EUNSUPPORTED, "%s: head_dim=%d, only 64 is implemented", name, a.D);
    if (!a.Q || !a.K || !a.V || !a.O) return fail(LDIT_EINVAL, "%s: null operand", name);
    if ((a.ldq | a.ldk | a.ldv | a.plane_in) & 7 || (a.ldo & 3) ||
        (planes && (a.ldo < a.planes * a.H * 64 || a.ldq != a.ldk || a.ldq != a.ldv || a.ldq < (a.planes - 1) * a.plane_in + a.H * 64)))
        return fail(LDIT_EINVAL, "%s: bad strides (multiples of 8 in / 4 out, planes: one input stride, rows wide enough for the planes)", name);
    if (!aligned16(a.Q) || !aligned16(a.K) || !aligned16(a.V) || (reinterpret_cast<uintptr_t>(a.O) & (fp8 ? 3u : 7u)))
        return fail(LDIT_EINVAL, "%s: operands must be 16-byte aligned", name);
    switch (a.out) {
        case ATTN_BF16: return launch_form<1, ATTN_BF16>(a, stream);
        case ATTN_FP8: return launch_form<1, ATTN_FP8>(a, stream);
        case ATTN_MX: return launch_form<1, ATTN_MX>(a, stream);
        case ATTN_MX_TRAIN: return launch_form<1, ATTN_MX_TRAIN>(a, stream);
        case ATTN_PLANES: return a.planes == 2 ? launch_form<2, ATTN_PLANES>(a, stream) : launch_form<3, ATTN_PLANES>(a, stream);
    }
    return fail(LDIT_EINVAL, "attention: unknown output form %d", (int)a.out);
}

}  // namespace ldit

#ifdef LDIT_GEMM_STAMPS
extern "C" int ldit_dbg_set_attn_stamps(void *buf)
{
    unsigned long long *p = static_cast<unsigned long long *>(buf);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_attn_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#endif
