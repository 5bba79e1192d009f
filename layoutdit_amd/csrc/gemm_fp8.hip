// fp8 (OCP e4m3, gfx950) MFMA GEMM with per-tensor scales:  Y[M,N] = epi( sa*sw * (A8[M,K] . W8[N,K]^T) ),
// A8, W8 fp8 e4m3 (K-contiguous), fp32 accumulate.  Groundwork for BASELINE configs[4] (fp8 forward).
//
// Same skeleton as gemm_bf16.hip: K-contiguous operands -> LDS by LDS-DMA, 128-B LDS rows (128 fp8), 16-B chunk
// XOR-swizzled with (row>>1)&7, two stages, 2 x 4 waves (two per SIMD) on a 256 x 256 tile.  A lane's b128 fragment read
// holds 16 consecutive fp8 of its row: the low 8 bytes feed one v_mfma_f32_32x32x16_fp8_fp8, the high 8 bytes the next
// (a permutation of the k order applied identically to both operands), so each LDS read pays for two MFMAs.
// The non-scaled fp8 MFMA issues at the bf16 rate; what fp8 buys here is half the DMA / LDS bytes per FLOP.
// Epilogues: bias -> bf16 ; bias + erf-GELU -> fp8 (times out_inv_scale, saturated to +-448) ; R + lam (.) (.) -> fp32.
#include <cstdlib>
#include <type_traits>

#include "ldit_common.h"
#include "epilogue_rows.h"

namespace ldit {

namespace {

typedef long i64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_8 __attribute__((ext_vector_type(4)));
constexpr int BKE = 128, ROW8 = 128;

__device__ __forceinline__ void glds16q(const void *gsrc, char *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

struct GemmArgs8 {
    const unsigned char *A, *W;   // fp8 e4m3
    void *Y;                      // bf16 (BIAS) / fp8 (BIAS_GELU) / fp32 (SCALE_RESID)
    float *Y2;                    // optional fp32 tap copy (SCALE_RESID)
    const float *bias, *lam, *R;
    int M, N, K, lda, ldy;
    float ab_scale;               // per-tensor dequantisation of the accumulator: sa * sw, or sa alone when d_wrow is given
    float out_inv_scale;          // 1 / scale of the fp8 output (BIAS_GELU)
    const float *d_act, *d_out;   // device-resident sa / so: override the two host values when non-null
    const float *d_wrow;          // optional per-output-channel weight scales [N] (multiplied onto the per-tensor part)
    int direct_epi;               // LDIT_GEMM_DIRECT_EPILOGUE=1: interior tiles stored straight from the accumulators
    // MX instantiations only (block scales, ldit.h LDIT_MXFP8): E8M0 bytes [rows, ld / 32] beside A, W and the MX output of
    // BIAS_GELU; row strides in bytes (= elements / 32).  Appended last: the per-tensor instantiations read the fields above
    // at the offsets they always had.
    const unsigned char *As, *Ws;
    unsigned char *Ys;
    int ldas, ldws, ldys;
};

// The TR kernels' arguments (mxfp8 train step; a struct of their own, so that the other kernels' arguments stay as they were),
// row stride ldy: SCALE_RESID: Ypre = bf16 of the branch output before LayerScale, rowscale = per-row factor on lam (stochastic
// depth), as GemmExtra of the bf16 GEMM; BIAS_GELU: Ypre = bf16 gelu'(pre-activation) (the backward's factor), Yd = bf16 of the
// dequantised MX output (the fc2 wgrad's operand).
struct GemmArgs8T : GemmArgs8 {
    void *Ypre;
    const float *rowscale;
    void *Yd;
};
__device__ __forceinline__ void *ypre_of(const GemmArgs8 &) { return nullptr; }
__device__ __forceinline__ void *ypre_of(const GemmArgs8T &p) { return p.Ypre; }
__device__ __forceinline__ const float *rowscale_of(const GemmArgs8 &) { return nullptr; }
__device__ __forceinline__ const float *rowscale_of(const GemmArgs8T &p) { return p.rowscale; }
__device__ __forceinline__ void *yd_of(const GemmArgs8 &) { return nullptr; }
__device__ __forceinline__ void *yd_of(const GemmArgs8T &p) { return p.Yd; }

// MODE 0: tile inside the matrix, 16-B / 8-B accesses unchecked; MODE 1: columns inside, rows past M skipped (the ragged
// last row tile keeps its vector accesses - a lane owns a row, so the element-wise path does not coalesce and cost ~20 us);
// MODE 2: element-wise with checks.
template <int TM, int TN, int EPI, int MODE, bool MX = false, bool TR = false, typename PA = GemmArgs8>
__device__ __forceinline__ void store_q(const PA &p, const f32x16 (&acc)[TM][TN], int mw, int nw, int lane)
{
    const int c32 = lane & 31, h = lane >> 5;
    const bool dual = p.Y2 != nullptr;
    const float ab = p.d_act ? p.d_act[0] : p.ab_scale;
    const float oinv = (EPI == EPI_BIAS_GELU && p.d_out) ? 1.0f / p.d_out[0] : p.out_inv_scale;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        f32x4 bias[4], lam[4], abq[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = nw + j * 32 + 8 * g + 4 * h + e;
                const bool ok = MODE != 2 || n < p.N;
                bias[g][e] = (ok && p.bias) ? p.bias[n] : 0.0f;
                lam[g][e] = (EPI == EPI_SCALE_RESID && ok) ? p.lam[n] : 0.0f;
                abq[g][e] = (ok && p.d_wrow) ? ab * p.d_wrow[n] : ab;
            }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = mw + i * 32 + c32;
            if (MODE != 0 && m >= p.M) continue;
            if constexpr (MX && EPI == EPI_BIAS_GELU) {
                // MX output: the row's 32-column block j is split between this lane (columns 8 g + 4 h + e) and lane l ^ 32 -
                // one exchange completes its amax (N % 32 == 0: a block is wholly inside or wholly outside the matrix)
                f32x4 v[4], gp[TR ? 4 : 1];
                unsigned amax = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (TR) {
                            float ge, gd;
                            gelu_and_grad_lp(__builtin_fmaf(acc[i][j][4 * g + e], abq[g][e], bias[g][e]), ge, gd);
                            v[g][e] = ge;
                            gp[g][e] = gd;
                        }
                        else v[g][e] = gelu_lp(__builtin_fmaf(acc[i][j][4 * g + e], abq[g][e], bias[g][e]));
                        amax = umax32(amax, __float_as_uint(v[g][e]) & 0x7fffffffu);
                    }
                amax = umax32(amax, (unsigned)__shfl_xor((int)amax, 32, 64));
                const unsigned sb = mx_scale_byte(amax);
                const float inv = mx_inv_scale(sb);
                const int nb = nw + j * 32;
                if (MODE == 2 && nb >= p.N) continue;
                unsigned char *y = static_cast<unsigned char *>(p.Y);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned o = (unsigned)m * (unsigned)p.ldy + (unsigned)(nb + 8 * g + 4 * h);
                    const unsigned pk = pack_fp8x4(v[g][0] * inv, v[g][1] * inv, v[g][2] * inv, v[g][3] * inv);
                    *reinterpret_cast<unsigned *>(y + o) = pk;
                    if constexpr (TR) {
                        *reinterpret_cast<bf16x4_8 *>(static_cast<__bf16 *>(ypre_of(p)) + o) =
                            bf16x4_8{(__bf16)gp[g][0], (__bf16)gp[g][1], (__bf16)gp[g][2], (__bf16)gp[g][3]};
                        *reinterpret_cast<mx_bf16x4 *>(static_cast<__bf16 *>(yd_of(p)) + o) = mx_dequant_bf16x4(pk, sb);
                    }
                }
                if (h == 0) p.Ys[(unsigned)m * (unsigned)p.ldys + (unsigned)(nb >> 5)] = (unsigned char)sb;
                continue;
            }
            f32x4 res[4];
            const float rs = (TR && EPI == EPI_SCALE_RESID && rowscale_of(p)) ? rowscale_of(p)[m] : 1.0f;
            if (EPI == EPI_SCALE_RESID) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = nw + j * 32 + 8 * g + 4 * h;
                    const unsigned o = (unsigned)m * (unsigned)p.ldy + (unsigned)n;
                    if (MODE != 2) res[g] = *reinterpret_cast<const f32x4 *>(p.R + o);
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) res[g][e] = (n + e < p.N) ? p.R[o + e] : 0.0f;
                }
                asm volatile("" ::: "memory");
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = nw + j * 32 + 8 * g + 4 * h;
                const unsigned o = (unsigned)m * (unsigned)p.ldy + (unsigned)n;
                f32x4 v, pre;
                (void)pre;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = __builtin_fmaf(acc[i][j][4 * g + e], abq[g][e], bias[g][e]);
                    if (EPI == EPI_BIAS_GELU) t = gelu_lp(t);
                    if (TR && EPI == EPI_SCALE_RESID) pre[e] = t;
                    if (EPI == EPI_SCALE_RESID) {
                        if (TR && rowscale_of(p)) t = __builtin_fmaf(lam[g][e] * rs, t, res[g][e]);
                        else t = __builtin_fmaf(lam[g][e], t, res[g][e]);
                    }
                    v[e] = t;
                }
                if (TR && EPI == EPI_SCALE_RESID && ypre_of(p)) {
                    __bf16 *yp = static_cast<__bf16 *>(ypre_of(p));
                    if (MODE != 2) *reinterpret_cast<bf16x4_8 *>(yp + o) = bf16x4_8{(__bf16)pre[0], (__bf16)pre[1], (__bf16)pre[2], (__bf16)pre[3]};
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < p.N) yp[o + e] = (__bf16)pre[e];
                }
                if (EPI == EPI_SCALE_RESID) {
                    float *y = static_cast<float *>(p.Y);
                    if (MODE != 2) {
                        *reinterpret_cast<f32x4 *>(y + o) = v;
                        if (dual) *reinterpret_cast<f32x4 *>(p.Y2 + o) = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < p.N) { y[o + e] = v[e]; if (dual) p.Y2[o + e] = v[e]; }
                    }
                } else if (EPI == EPI_BIAS_GELU) {
                    unsigned char *y = static_cast<unsigned char *>(p.Y);
                    const unsigned pk = pack_fp8x4(v[0] * oinv, v[1] * oinv, v[2] * oinv, v[3] * oinv);
                    if (MODE != 2) *reinterpret_cast<unsigned *>(y + o) = pk;
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < p.N) y[o + e] = (unsigned char)(pk >> (8 * e));
                } else {
                    __bf16 *y = static_cast<__bf16 *>(p.Y);
                    if (MODE != 2) {
                        const bf16x4_8 pk = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
                        *reinterpret_cast<bf16x4_8 *>(y + o) = pk;
                    } else
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < p.N) y[o + e] = (__bf16)v[e];
                }
            }
            if (EPI == EPI_SCALE_RESID) asm volatile("" ::: "memory");
        }
    }
}

// K64 = false: v_mfma_f32_32x32x16_fp8_fp8 (bf16 rate), two per b128 fragment read, four chunk steps per k-tile.
// K64 = true : v_mfma_f32_32x32x64_f8f6f4 with e4m3 operands and unit block scales (2x the bf16 rate): a lane's operand is
//              32 consecutive fp8 of its row (two b128 reads), two chunk steps per k-tile.
// MX = true (K64 only): the same MFMA with VGPR block scales (v_mfma_scale_f32_32x32x64_f8f6f4 ..., vS, vT).  The instruction's
//              scale block b of a 64-deep step is the b-th 16 bytes of BOTH lane halves, and lane half b supplies its scale: a lane
//              therefore takes 16-B chunks h and 2 + h of the step (not 2 h, 2 h + 1), block b is then the row's 32 consecutive
//              bytes 64 c + 32 b, and lane half h's scale is byte 2 c + h of the row's k-tile dword - the dword shifted right by
//              8 h, op_sel 2 c (pinned exactly by tests/test_gpu_mxfp8.py).  A k-tile's dwords are fetched behind the hand-over
//              barrier one iteration ahead (asm loads in front of that iteration's DMA pieces, so that the counted wait at the end
//              of the iteration lets the DMA stay in flight), the per-tensor instantiations are unchanged.
// The tile kernel.  Its body (gemm_fp8_mfma_body.inc) is written once and included into two kernels, so that each is an ordinary
// kernel with its own argument: gemm_fp8_mfma (TR = false) and gemm_fp8_mfma_tr (MX, the mxfp8 train step's epilogues, GemmArgs8T).
template <int WM, int WN, int TM, int TN, int EPI, bool K64, bool MX = false>
__global__ void __launch_bounds__(64 * WM * WN, (WM * WN) / 4) gemm_fp8_mfma(const GemmArgs8 p)
{
    constexpr bool TR = false;
#include "gemm_fp8_mfma_body.inc"
}

template <int WM, int WN, int TM, int TN, int EPI>
__global__ void __launch_bounds__(64 * WM * WN, (WM * WN) / 4) gemm_fp8_mfma_tr(const GemmArgs8T p)
{
    constexpr bool K64 = true, MX = true, TR = true;
#include "gemm_fp8_mfma_body.inc"
}

template <int WM, int WN, int TM, int TN, int EPI, bool K64, bool MX = false, bool TR = false, typename PA = GemmArgs8>
int launch_q(const PA &a, hipStream_t stream)
{
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    constexpr int lds = 2 * (BM + BN) * ROW8;
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    if constexpr (TR) {
        auto kern = gemm_fp8_mfma_tr<WM, WN, TM, TN, EPI>;
        LDIT_DYN_LDS(kern, lds);
        hipLaunchKernelGGL(kern, dim3(tiles), dim3(64 * WM * WN), lds, stream, a);
    } else {
        auto kern = gemm_fp8_mfma<WM, WN, TM, TN, EPI, K64, MX>;
        LDIT_DYN_LDS(kern, lds);
        hipLaunchKernelGGL(kern, dim3(tiles), dim3(64 * WM * WN), lds, stream, a);
    }
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

// ---- tail kernel: up to 64 rows (the ragged tail peeled off by launch_gemm_fp8, or a whole problem that small) -------------
// Same scheme as gemm_bf16_tail (gemm_bf16.hip): one wave per 32 x 32 output tile walks ALL of K in order with the tile
// kernel's own instruction - v_mfma_f32_32x32x64_f8f6f4, a lane's operand = 32 consecutive fp8 of its row at k = 64 s + 32 h -
// so a peeled row gets the bits a 256 x 256 tile would have given it (the round-2 split-K kernel summed eight K slices of
// v_mfma_f32_32x32x16_fp8_fp8 products: another order AND another instruction).  Fragments straight from global memory,
// two register sets of four 64-deep steps.  MX: the lane's operand of step s is block 2 s + h of its row - one scale byte each.
template <int EPI, bool MX = false>
__global__ void __launch_bounds__(64) gemm_fp8_tail(const GemmArgs8 p)
{
    constexpr bool TR = false;
#include "gemm_fp8_tail_body.inc"
}

template <int EPI>
__global__ void __launch_bounds__(64) gemm_fp8_tail_tr(const GemmArgs8T p)
{
    constexpr bool MX = true, TR = true;
#include "gemm_fp8_tail_body.inc"
}

template <int EPI, bool MX = false, bool TR = false, typename PA = GemmArgs8>
int launch_qtail(const PA &a, hipStream_t stream)
{
    const unsigned blocks = (unsigned)(((a.N + 31) / 32) * ((a.M + 31) / 32));
    if constexpr (TR) hipLaunchKernelGGL((gemm_fp8_tail_tr<EPI>), dim3(blocks), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((gemm_fp8_tail<EPI, MX>), dim3(blocks), dim3(64), 0, stream, a);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

template <int EPI, bool MX = false, bool TR = false, typename PA = GemmArgs8>
int launch_q_tiled(const PA &a, hipStream_t stream)
{
    // LDIT_GEMM_FP8_K16=1 selects the K = 16 MFMA, LDIT_GEMM_FP8_TILE=0..2 forces a tile (both for experiments / tests)
    // (MX: the K = 16 MFMA has no block scales - the switch does not apply)
    const bool k16 = !MX && diag().fp8_k16, noskinny = diag().fp8_noskinny;
    if (a.M <= 64 && !noskinny && !k16) return launch_qtail<EPI, MX, TR>(a, stream);     // peeled tail / tiny batch (bit-identical to the K = 64 tiles)
    // Time model fitted to scripts/gemm_fp8_bench.py on ViT-B / ViT-L shapes, M = 3 k .. 25 k (profiles/README.md), in us:
    //   256 x 256 (one workgroup per CU):  strict rounds of 256 tiles, each  a[epi] + 11.3e-3 K
    //   128 x 128 (two per CU, they overlap each other's prologue / epilogue):  rounds of 256 tiles, each  r[epi] + 4.25e-3 K,
    //   but never less than one tile's own latency  5.3 + 8e-3 K.   (256 x 128 never won a shape: kept for experiments only.)
    const double a256[3] = {14.3, 16.8, 21.3}, r128[3] = {3.65, 3.85, 7.2};
    const long t256 = (long)((a.M + 255) / 256) * ((a.N + 255) / 256), t128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128);
    const double c256 = (double)((t256 + 255) / 256) * (a256[EPI] + 11.3e-3 * a.K);
    double c128 = (double)((t128 + 255) / 256) * (r128[EPI] + 4.25e-3 * a.K);
    if (c128 < 5.3 + 8e-3 * a.K) c128 = 5.3 + 8e-3 * a.K;
    int pick = c256 <= c128 ? 0 : 2;
    // Round 2: 192- and 320-row variants of the 8-wave tile against round quantisation (see gemm_bf16.hip launch_h_tiled)
    double best = c256 <= c128 ? c256 : c128;
    const double per256 = a256[EPI] + 11.3e-3 * a.K;
    for (int bm : {192, 320}) {
        if (bm == 320 && EPI == EPI_SCALE_RESID) continue;      // its residual epilogue does not fit 256 VGPRs (spills)
        const long t = (long)((a.M + bm - 1) / bm) * ((a.N + 255) / 256);
        const double c = (double)((t + 255) / 256) * per256 * (bm / 256.0) * 1.03;
        if (c < best) { best = c; pick = bm == 192 ? 3 : 4; }
    }
    if (const int force = diag().fp8_tile; force >= 0 && force <= 4) pick = force;
    if (k16 && pick > 2) pick = 0;
    if (pick == 3) return launch_q<2, 4, 3, 2, EPI, true, MX, TR>(a, stream);      // 192 x 256
    if (pick == 4 && EPI == EPI_SCALE_RESID) pick = 0;
    if constexpr (EPI != EPI_SCALE_RESID)
        if (pick == 4) return launch_q<2, 4, 5, 2, EPI, true, MX, TR>(a, stream);  // 320 x 256
    if constexpr (MX) {
        if (pick == 0) return launch_q<2, 4, 4, 2, EPI, true, true, TR>(a, stream);
        if (pick == 1) return launch_q<2, 2, 4, 2, EPI, true, true, TR>(a, stream);
        return launch_q<2, 2, 2, 2, EPI, true, true, TR>(a, stream);
    }
    if (k16) {
        if (pick == 0) return launch_q<2, 4, 4, 2, EPI, false>(a, stream);
        if (pick == 1) return launch_q<2, 2, 4, 2, EPI, false>(a, stream);
        return launch_q<2, 2, 2, 2, EPI, false>(a, stream);
    }
    if (pick == 0) return launch_q<2, 4, 4, 2, EPI, true>(a, stream);      // 256 x 256, 8 waves
    if (pick == 1) return launch_q<2, 2, 4, 2, EPI, true>(a, stream);      // 256 x 128, 4 waves
    return launch_q<2, 2, 2, 2, EPI, true>(a, stream);                     // 128 x 128, 4 waves
}

// dst[i] = fp8(src[i] * inv_scale), saturating; 4 elements per thread
__global__ void __launch_bounds__(256) quant_fp8(const float *__restrict__ src, unsigned char *__restrict__ dst, size_t n,
                                                 float inv_scale, const float *__restrict__ d_scale)
{
    if (d_scale) inv_scale = 1.0f / d_scale[0];
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(src + i);
        *reinterpret_cast<unsigned *>(dst + i) = pack_fp8x4(v[0] * inv_scale, v[1] * inv_scale, v[2] * inv_scale, v[3] * inv_scale);
    } else {
        for (size_t k = i; k < n; ++k) dst[k] = (unsigned char)pack_fp8x4(src[k] * inv_scale, 0.f, 0.f, 0.f);
    }
}

// *out = max(*out, max |src|): non-negative floats order like their bit patterns, so one integer atomicMax per block
__global__ void __launch_bounds__(256) amax_f32(const float *__restrict__ src, size_t n, unsigned *__restrict__ out)
{
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(src[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        atomicMax(out, __float_as_uint(m));
    }
}


// One wave per weight row: scale[n] = max(|W[n, :]|) / 448 (never 0), codes[n, :] = fp8(W[n, :] / scale[n]).
// Per-output-channel scales cost nothing in the GEMM (one more factor on the accumulator in the epilogue) and keep
// a few large rows from flattening all the others.
__global__ void __launch_bounds__(256) quant_rows_fp8(const float *__restrict__ W, unsigned char *__restrict__ dst,
                                                      float *__restrict__ scales, int N, int K, float mul)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(W + (size_t)row * K);
    float m = 0.0f;
    for (int i = lane; i < K / 4; i += 64) {
        const f32x4 v = w4[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    // (mul: pack-time factor on the row - scale * log2 e on W_q for the pre-scaled attention - carried by the row's scale: the
    // codes are those of the unscaled row)
    const float sc = fmaxf(m, 1e-30f) * (1.0f / 448.0f), inv = 1.0f / sc;
    if (lane == 0) scales[row] = sc * mul;
    unsigned *d4 = reinterpret_cast<unsigned *>(dst + (size_t)row * K);
    for (int i = lane; i < K / 4; i += 64) {
        const f32x4 v = w4[i];
        d4[i] = pack_fp8x4(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv);
    }
}

// MX quantisation (ldit.h, LDIT_MXFP8): eight consecutive lanes own one 32-element block of a row (4 elements each), three
// exchanges give its amax.  codes [rows, K] (dense), scales [rows, K / 32]; `mul` is folded into the values first (W_q at pack time).
__global__ void __launch_bounds__(256) quant_mx(const float *__restrict__ src, int64_t lds, unsigned char *__restrict__ codes,
                                                unsigned char *__restrict__ scales, int64_t rows, int K, float mul)
{
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, blk = gid >> 3;
    const int nb = K >> 5, q = (int)(gid & 7);
    const bool ok = blk < rows * nb;
    const int64_t b = ok ? blk : rows * nb - 1;
    const int64_t row = b / nb;
    const int col = (int)(b - row * nb) * 32 + 4 * q;
    f32x4 v = *reinterpret_cast<const f32x4 *>(src + row * lds + col);
    unsigned amax = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] *= mul;
        amax = umax32(amax, __float_as_uint(v[e]) & 0x7fffffffu);
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) amax = umax32(amax, (unsigned)__shfl_xor((int)amax, o, 64));
    const unsigned sb = mx_scale_byte(amax);
    const float inv = mx_inv_scale(sb);
    if (!ok) return;
    *reinterpret_cast<unsigned *>(codes + row * K + col) = pack_fp8x4(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv);
    if (q == 0) scales[row * nb + (col >> 5)] = (unsigned char)sb;
}

__global__ void amax_to_scale(float *p, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) p[i] = fmaxf(p[i], 1e-30f) * (1.0f / 448.0f);
}

}  // namespace

static int launch_gemm_fp8_one(const void *A, int lda, const void *W, const float *bias, void *Y, int ldy, int M, int N, int K,
                               int epi, const float *lam, const float *R, float *Y2, float ab_scale, float out_inv_scale,
                               const float *d_act, const float *d_wrow, const float *d_out, hipStream_t stream);

// A ragged tail of up to 64 rows past a multiple of the 256-row tile is peeled off into a second, tiny launch (gemm_fp8_tail;
// see launch_gemm_bf16_ex): M = 16 x 1025 = 64 x 256 + 16 would otherwise cost a whole extra round of workgroups.
int launch_gemm_fp8(const void *A, int lda, const void *W, const float *bias, void *Y, int ldy, int M, int N, int K, int epi,
                    const float *lam, const float *R, float *Y2, float ab_scale, float out_inv_scale, const float *d_act,
                    const float *d_wrow, const float *d_out, hipStream_t stream)
{
    const int rem = M % 256;
    const long nbn = (N + 255) / 256, full = ((long)M / 256 + 1) * nbn, mainp = ((long)M / 256) * nbn;
    if (rem != 0 && rem <= 64 && M > 256 && (full + 255) / 256 > (mainp + 255) / 256) {   // peel only when it saves a round
        const int main_rows = M - rem;
        const size_t out_elt = epi == EPI_SCALE_RESID ? 4 : epi == EPI_BIAS_GELU ? 1 : 2;
        int rc = launch_gemm_fp8_one(A, lda, W, bias, Y, ldy, main_rows, N, K, epi, lam, R, Y2, ab_scale, out_inv_scale, d_act, d_wrow, d_out, stream);
        if (rc != LDIT_OK) return rc;
        const char *At = static_cast<const char *>(A) + (size_t)main_rows * lda;
        char *Yt = static_cast<char *>(Y) + (size_t)main_rows * ldy * out_elt;
        return launch_gemm_fp8_one(At, lda, W, bias, Yt, ldy, rem, N, K, epi, lam, R ? R + (size_t)main_rows * ldy : nullptr,
                                   Y2 ? Y2 + (size_t)main_rows * ldy : nullptr, ab_scale, out_inv_scale, d_act, d_wrow, d_out, stream);
    }
    return launch_gemm_fp8_one(A, lda, W, bias, Y, ldy, M, N, K, epi, lam, R, Y2, ab_scale, out_inv_scale, d_act, d_wrow, d_out, stream);
}

static int launch_gemm_fp8_one(const void *A, int lda, const void *W, const float *bias, void *Y, int ldy, int M, int N, int K,
                               int epi, const float *lam, const float *R, float *Y2, float ab_scale, float out_inv_scale,
                               const float *d_act, const float *d_wrow, const float *d_out, hipStream_t stream)
{
    if (M <= 0 || N <= 0 || K <= 0) return fail(LDIT_EINVAL, "gemm_fp8: empty problem");
    if (K % BKE) return fail(LDIT_EUNSUPPORTED, "gemm_fp8: K=%d must be a multiple of %d", K, BKE);
    if (!A || !W || !Y) return fail(LDIT_EINVAL, "gemm_fp8: null operand");
    if (!aligned16(A) || !aligned16(W) || (lda & 15)) return fail(LDIT_EINVAL, "gemm_fp8: operands must be 16-byte aligned");
    GemmArgs8 a{};
    a.A = static_cast<const unsigned char *>(A); a.W = static_cast<const unsigned char *>(W); a.Y = Y; a.Y2 = Y2;
    a.bias = bias; a.lam = lam; a.R = R; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldy = ldy;
    a.ab_scale = ab_scale; a.out_inv_scale = out_inv_scale; a.d_act = d_act; a.d_wrow = d_wrow; a.d_out = d_out;
    a.direct_epi = diag().direct_epi ? 1 : 0;
    switch (epi) {
        case EPI_BIAS: return launch_q_tiled<EPI_BIAS>(a, stream);
        case EPI_BIAS_GELU: return launch_q_tiled<EPI_BIAS_GELU>(a, stream);
        case EPI_SCALE_RESID:
            if (!lam || !R) return fail(LDIT_EINVAL, "gemm_fp8: scale+residual epilogue needs lam and R");
            return launch_q_tiled<EPI_SCALE_RESID>(a, stream);
        default: return fail(LDIT_EINVAL, "gemm_fp8: unknown epilogue %d", epi);
    }
}

static int launch_gemm_mxfp8_one(const void *A, int lda, const void *As, const void *W, const void *Ws, const float *bias, void *Y,
                                 int ldy, void *Ys, int M, int N, int K, int epi, const float *lam, const float *R, float *Y2,
                                 hipStream_t stream, bool tr = false, void *Ypre = nullptr, const float *rowscale = nullptr,
                                 void *Yd = nullptr)
{
    if (M <= 0 || N <= 0 || K <= 0) return fail(LDIT_EINVAL, "gemm_mxfp8: empty problem");
    if (K % BKE) return fail(LDIT_EUNSUPPORTED, "gemm_mxfp8: K=%d must be a multiple of %d", K, BKE);
    if (!A || !W || !Y || !As || !Ws || (epi == EPI_BIAS_GELU && !Ys)) return fail(LDIT_EINVAL, "gemm_mxfp8: null operand");
    if (!aligned16(A) || !aligned16(W) || (lda % BKE) || (reinterpret_cast<uintptr_t>(As) & 3u) || (reinterpret_cast<uintptr_t>(Ws) & 3u))
        return fail(LDIT_EINVAL, "gemm_mxfp8: operands must be 16-byte aligned (scales 4-byte), lda a multiple of %d", BKE);
    if (epi == EPI_BIAS_GELU && ((N & 31) || (ldy & 31) || (reinterpret_cast<uintptr_t>(Y) & 3u)))
        return fail(LDIT_EINVAL, "gemm_mxfp8: the MX output needs N and ldy multiples of 32");
    GemmArgs8 a{};
    a.A = static_cast<const unsigned char *>(A); a.W = static_cast<const unsigned char *>(W); a.Y = Y; a.Y2 = Y2;
    a.bias = bias; a.lam = lam; a.R = R; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldy = ldy;
    a.ab_scale = 1.0f; a.out_inv_scale = 1.0f;     // every scale is a block scale inside the MFMA
    a.direct_epi = diag().direct_epi ? 1 : 0;
    a.As = static_cast<const unsigned char *>(As); a.Ws = static_cast<const unsigned char *>(Ws); a.Ys = static_cast<unsigned char *>(Ys);
    a.ldas = lda / 32; a.ldws = K / 32; a.ldys = ldy / 32;
    if (tr) {
        GemmArgs8T t{};
        static_cast<GemmArgs8 &>(t) = a;
        t.Ypre = Ypre; t.rowscale = rowscale; t.Yd = Yd;
        if (epi == EPI_BIAS_GELU) return launch_q_tiled<EPI_BIAS_GELU, true, true>(t, stream);
        if (epi == EPI_SCALE_RESID && lam && R) return launch_q_tiled<EPI_SCALE_RESID, true, true>(t, stream);
        return fail(LDIT_EINVAL, "gemm_mxfp8: train epilogue %d not available", epi);
    }
    switch (epi) {
        case EPI_BIAS: return launch_q_tiled<EPI_BIAS, true>(a, stream);
        case EPI_BIAS_GELU: return launch_q_tiled<EPI_BIAS_GELU, true>(a, stream);
        case EPI_SCALE_RESID:
            if (!lam || !R) return fail(LDIT_EINVAL, "gemm_mxfp8: scale+residual epilogue needs lam and R");
            return launch_q_tiled<EPI_SCALE_RESID, true>(a, stream);
        default: return fail(LDIT_EINVAL, "gemm_mxfp8: unknown epilogue %d", epi);
    }
}

// launch_gemm_fp8's peeling of a ragged tail of up to 64 rows, on MX operands (the scale rows move with the code rows)
static int gemm_mxfp8_peeled(const void *A, int lda, const void *As, const void *W, const void *Ws, const float *bias, void *Y, int ldy,
                             void *Ys, int M, int N, int K, int epi, const float *lam, const float *R, float *Y2, hipStream_t stream,
                             bool tr, void *Ypre, const float *rowscale, void *Yd)
{
    const int rem = M % 256;
    const long nbn = (N + 255) / 256, full = ((long)M / 256 + 1) * nbn, mainp = ((long)M / 256) * nbn;
    if (rem != 0 && rem <= 64 && M > 256 && (full + 255) / 256 > (mainp + 255) / 256) {
        const int main_rows = M - rem;
        const size_t out_elt = epi == EPI_SCALE_RESID ? 4 : epi == EPI_BIAS_GELU ? 1 : 2;
        int rc = launch_gemm_mxfp8_one(A, lda, As, W, Ws, bias, Y, ldy, Ys, main_rows, N, K, epi, lam, R, Y2, stream, tr, Ypre, rowscale, Yd);
        if (rc != LDIT_OK) return rc;
        const char *At = static_cast<const char *>(A) + (size_t)main_rows * lda;
        const char *Ast = static_cast<const char *>(As) + (size_t)main_rows * (lda / 32);
        char *Yt = static_cast<char *>(Y) + (size_t)main_rows * ldy * out_elt;
        char *Yst = Ys ? static_cast<char *>(Ys) + (size_t)main_rows * (ldy / 32) : nullptr;
        return launch_gemm_mxfp8_one(At, lda, Ast, W, Ws, bias, Yt, ldy, Yst, rem, N, K, epi, lam, R ? R + (size_t)main_rows * ldy : nullptr,
                                     Y2 ? Y2 + (size_t)main_rows * ldy : nullptr, stream, tr,
                                     Ypre ? static_cast<char *>(Ypre) + (size_t)main_rows * ldy * 2 : nullptr,
                                     rowscale ? rowscale + main_rows : nullptr, Yd ? static_cast<char *>(Yd) + (size_t)main_rows * ldy * 2 : nullptr);
    }
    return launch_gemm_mxfp8_one(A, lda, As, W, Ws, bias, Y, ldy, Ys, M, N, K, epi, lam, R, Y2, stream, tr, Ypre, rowscale, Yd);
}

int launch_gemm_mxfp8(const void *A, int lda, const void *As, const void *W, const void *Ws, const float *bias, void *Y, int ldy,
                      void *Ys, int M, int N, int K, int epi, const float *lam, const float *R, float *Y2, hipStream_t stream)
{
    return gemm_mxfp8_peeled(A, lda, As, W, Ws, bias, Y, ldy, Ys, M, N, K, epi, lam, R, Y2, stream, false, nullptr, nullptr, nullptr);
}

// mxfp8 train step (GemmArgs8, TR): SCALE_RESID with Ypre / rowscale, BIAS_GELU with gelu' (Ypre) and the dequantised output (Yd);
// the tile choice, the k-loop and the stored Y are those of launch_gemm_mxfp8
int launch_gemm_mxfp8_train(const void *A, int lda, const void *As, const void *W, const void *Ws, const float *bias, void *Y, int ldy,
                            void *Ys, int M, int N, int K, int epi, const float *lam, const float *R, float *Y2, void *Ypre,
                            const float *rowscale, void *Yd, hipStream_t stream)
{
    if (epi != EPI_SCALE_RESID && epi != EPI_BIAS_GELU) return fail(LDIT_EINVAL, "gemm_mxfp8: train epilogue %d not available", epi);
    if (epi == EPI_BIAS_GELU && (!Ypre || !Yd)) return fail(LDIT_EINVAL, "gemm_mxfp8: the GELU train epilogue needs Ypre and Yd");
    if ((reinterpret_cast<uintptr_t>(Ypre) | reinterpret_cast<uintptr_t>(Yd)) & 7u) return fail(LDIT_EINVAL, "gemm_mxfp8: Ypre / Yd must be 8-byte aligned");
    if (Ypre && (ldy & 3)) return fail(LDIT_EINVAL, "gemm_mxfp8: Ypre needs ldy %% 4 == 0");
    return gemm_mxfp8_peeled(A, lda, As, W, Ws, bias, Y, ldy, Ys, M, N, K, epi, lam, R, Y2, stream, true, Ypre, rowscale, Yd);
}

int launch_quant_mx(const float *src, int64_t lds, void *codes, void *scales, int64_t rows, int K, float mul, hipStream_t stream)
{
    if (rows <= 0 || K <= 0 || (K & 31) || lds < K || (lds & 3)) return fail(LDIT_EINVAL, "quant_mx: bad shape %lld x %d (ld %lld)", (long long)rows, K, (long long)lds);
    if (!src || !codes || !scales || !aligned16(src) || (reinterpret_cast<uintptr_t>(codes) & 3u))
        return fail(LDIT_EINVAL, "quant_mx: null or misaligned operand");
    const int64_t threads = rows * (K / 32) * 8;
    hipLaunchKernelGGL(quant_mx, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, src, lds,
                       static_cast<unsigned char *>(codes), static_cast<unsigned char *>(scales), rows, K, mul);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int launch_quant_fp8(const float *src, void *dst, size_t n, float inv_scale, const float *d_scale, hipStream_t stream)
{
    if (n == 0) return LDIT_OK;
    hipLaunchKernelGGL(quant_fp8, dim3((unsigned)((n / 4 + 255) / 256 + 1)), dim3(256), 0, stream, src,
                       static_cast<unsigned char *>(dst), n, inv_scale, d_scale);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int launch_quant_rows_fp8(const float *W, void *dst, float *scales, int N, int K, hipStream_t stream, float mul)
{
    if (N <= 0 || K <= 0 || (K & 3)) return fail(LDIT_EINVAL, "quant_rows_fp8: bad shape %d x %d", N, K);
    if (!W || !dst || !scales || !aligned16(W)) return fail(LDIT_EINVAL, "quant_rows_fp8: null or misaligned operand");
    hipLaunchKernelGGL(quant_rows_fp8, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, W, static_cast<unsigned char *>(dst),
                       scales, N, K, mul);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int launch_amax_to_scale(float *p, int n, hipStream_t stream)
{
    if (n <= 0) return LDIT_OK;
    hipLaunchKernelGGL(amax_to_scale, dim3((n + 63) / 64), dim3(64), 0, stream, p, n);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int launch_amax_f32(const float *src, size_t n, float *out, bool accumulate, hipStream_t stream)
{
    if (!accumulate) LDIT_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(float), stream));
    if (n == 0) return LDIT_OK;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(amax_f32, dim3(blocks), dim3(256), 0, stream, src, n, reinterpret_cast<unsigned *>(out));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // namespace ldit
