// Backward of the FPN stage behind DiTWithFPN (ref src/layoutdit/modeling/dit_backbone.py:87-90 under
// loss.backward(), ref src/layoutdit/training/trainer.py:169-178): the HBM-bound pieces.  The MFMA pieces reuse existing
// kernels (layoutdit_amd/modeling/dit_fpn.py sequences them):
//   dgrad of a 3x3 convolution  = the SAME implicit-im2col fp32 MFMA GEMM on the spatially flipped, in/out-swapped weight
//   wgrad of a 3x3 convolution  = nine reduction-major bf16 GEMMs (gemm_bf16_tr.hip, wgrad form), one per tap, on ZERO-PADDED
//                                 NHWC copies of dY and of the convolution's input: with both maps stored [B, H+2, W+2, C] the
//                                 tap (ky, kx) is a constant row offset (ky-1)(W+2) + (kx-1) of the input operand - the border
//                                 rows of dY are zero, so every term that the offset drags across a row or image end vanishes
//   laterals                    = ldit_linear_f32 (dgrad, on the transposed weight) / the same bf16 wgrad form
// Here:  (1) the adjoint of fpn_merge_nhwc (misc.hip): bilinear rescale of the lateral tokens + nearest top-down add,
//        (2) fp32 NHWC -> zero-padded bf16 NHWC copies for (wgrad),
//        (3) column sums (bias gradients), two stages, fixed order - no atomics anywhere, every result bit-reproducible,
//        (4) for grad_dtype="bf16" of the detector: a ReLU's backward, (2) or the plain bf16 copy, and stage 1 of (3) as one pass
//            over dy and the activation - the copy is the operand of the layer's dgrad AND wgrad GEMM.  The activation is fp32
//            or, for train_dtype="bf16" of the detector, the bf16 tensor its forward saved (the *_act16 entry points).
#include "ldit_common.h"

namespace ldit {
namespace {

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

// weight of source index g in the bilinear sample of output index o (the forward's own index arithmetic, misc.hip)
__device__ __forceinline__ float axis_w(int o, int g, int G, float inv_scale)
{
    float s = ((float)o + 0.5f) * inv_scale - 0.5f;
    s = s < 0.f ? 0.f : s;
    int i0 = (int)s;
    i0 = i0 > G - 1 ? G - 1 : i0;
    const int i1 = i0 + (i0 < G - 1);
    const float l = s - (float)i0;
    return (i0 == g ? 1.f - l : 0.f) + (i1 == g ? l : 0.f);
}

// d_lat[b, 1 + gy Gw + gx, :] = sum over the pixels of d_inner [B, Oh, Ow, Ch] whose bilinear footprint holds token (gy, gx);
// CLS row = 0.  One thread per (token, 4 channels): gather, fixed order.
__global__ void __launch_bounds__(256) fpn_merge_bwd_lat(const float *__restrict__ din, float *__restrict__ dlat, int B, int Gh, int Gw,
                                                         int Ch, int Oh, int Ow, float scale)
{
    const int c4n = Ch >> 2;
    const size_t total = (size_t)B * Gh * Gw * c4n, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % c4n);
    size_t t = idx / c4n;
    const int gx = (int)(t % Gw);
    t /= Gw;
    const int gy = (int)(t % Gh), b = (int)(t / Gh);
    const float inv = 1.0f / scale;
    int ylo = (int)floorf(scale * (float)(gy - 1)) - 1, yhi = (int)ceilf(scale * (float)(gy + 2)) + 1;
    int xlo = (int)floorf(scale * (float)(gx - 1)) - 1, xhi = (int)ceilf(scale * (float)(gx + 2)) + 1;
    ylo = ylo < 0 ? 0 : ylo; xlo = xlo < 0 ? 0 : xlo;
    yhi = yhi > Oh - 1 ? Oh - 1 : yhi; xhi = xhi > Ow - 1 ? Ow - 1 : xhi;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(din) + (size_t)b * Oh * Ow * c4n + c4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = axis_w(oy, gy, Gh, inv);
        if (wy == 0.0f) continue;
        f32x4 row = {0.f, 0.f, 0.f, 0.f};
        for (int ox = xlo; ox <= xhi; ++ox) {
            const float wx = axis_w(ox, gx, Gw, inv);
            if (wx == 0.0f) continue;
            const f32x4 v = src[(size_t)(oy * Ow + ox) * c4n];
#pragma unroll
            for (int e = 0; e < 4; ++e) row[e] += wx * v[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += wy * row[e];
    }
    f32x4 *dst = reinterpret_cast<f32x4 *>(dlat) + (size_t)b * (Gh * Gw + 1) * c4n;
    dst[(size_t)(1 + gy * Gw + gx) * c4n + c4] = acc;
    if (gy == 0 && gx == 0) dst[c4] = f32x4{0.f, 0.f, 0.f, 0.f};            // CLS row
}

// dtop[b, ty, tx, :] += sum over the pixels (oy, ox) of d_inner with nearest source (ty, tx): src = min(floor(o in/out), in-1)
__global__ void __launch_bounds__(256) fpn_merge_bwd_top(const float *__restrict__ din, float *__restrict__ dtop, int B, int Ch, int Oh,
                                                         int Ow, int Th, int Tw)
{
    const int c4n = Ch >> 2;
    const size_t total = (size_t)B * Th * Tw * c4n, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % c4n);
    size_t t = idx / c4n;
    const int tx = (int)(t % Tw);
    t /= Tw;
    const int ty = (int)(t % Th), b = (int)(t / Th);
    const float ry = (float)Th / (float)Oh, rx = (float)Tw / (float)Ow;
    auto src_of = [](int o, float r, int n) { int s = (int)floorf((float)o * r); return s > n - 1 ? n - 1 : s; };
    int ylo = (int)floorf((float)ty / ry) - 2, yhi = (int)ceilf((float)(ty + 1) / ry) + 2;
    int xlo = (int)floorf((float)tx / rx) - 2, xhi = (int)ceilf((float)(tx + 1) / rx) + 2;
    ylo = ylo < 0 ? 0 : ylo; xlo = xlo < 0 ? 0 : xlo;
    yhi = yhi > Oh - 1 ? Oh - 1 : yhi; xhi = xhi > Ow - 1 ? Ow - 1 : xhi;
    if (ty == Th - 1) yhi = Oh - 1;                  // the clamp sends everything past the end to the last source row / column
    if (tx == Tw - 1) xhi = Ow - 1;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(din) + (size_t)b * Oh * Ow * c4n + c4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oy = ylo; oy <= yhi; ++oy) {
        if (src_of(oy, ry, Th) != ty) continue;
        for (int ox = xlo; ox <= xhi; ++ox) {
            if (src_of(ox, rx, Tw) != tx) continue;
            const f32x4 v = src[(size_t)(oy * Ow + ox) * c4n];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += v[e];
        }
    }
    f32x4 *d = reinterpret_cast<f32x4 *>(dtop) + idx;
    f32x4 cur = *d;
#pragma unroll
    for (int e = 0; e < 4; ++e) cur[e] += acc[e];
    *d = cur;
}

// dst bf16 [B, H+2, W+2, C] = zero-padded copy of src fp32 [B, H, W, C]; every element of dst is written
__global__ void __launch_bounds__(256) pad_nhwc_bf16(const float *__restrict__ src, __bf16 *__restrict__ dst, int B, int H, int W, int C)
{
    const int c4n = C >> 2;
    const size_t total = (size_t)B * (H + 2) * (W + 2) * c4n, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % c4n);
    size_t t = idx / c4n;
    const int px = (int)(t % (W + 2));
    t /= (W + 2);
    const int py = (int)(t % (H + 2)), b = (int)(t / (H + 2));
    bf16x4_t o = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
    if (py >= 1 && py <= H && px >= 1 && px <= W) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(src)[((size_t)(b * H + py - 1) * W + px - 1) * c4n + c4];
        o = bf16x4_t{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    }
    reinterpret_cast<bf16x4_t *>(dst)[idx] = o;
}

constexpr int CS_ROWS = 512;

// ABSMAX = false: column sums; true: column maxima of |x| (fp8 calibration: per-channel activation ranges)
template <bool ABSMAX, typename T> __device__ __forceinline__ T cs_op(T acc, T v)
{
    if constexpr (ABSMAX) return fmaxf(acc, fabsf(v));
    else return acc + v;
}

// R consecutive rows from m on (R a multiple of 4, or 1): their terms into the four accumulators in row order - row m + r into
// s[r % 4] - with all R loads issued before the first store
template <bool ABSMAX, int R, typename T, typename Row, typename Sink> __device__ __forceinline__ void cs_rows(Row row, Sink sink, long m, T (&s)[4])
{
    T v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = row(m + r);
#pragma unroll
    for (int r = 0; r < R; ++r) sink(m + r, v[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) s[r & 3] = cs_op<ABSMAX>(s[r & 3], v[r]);
}

// One row block of a column sum, in the ONE order every column sum of this file has.  `row(m)` is called once per row m of
// [m0, m1), ascending, and yields that row's term - of one column (T = float) or of four adjacent ones (T = f32x4, each component
// its own column); `sink(m, term)` follows it for whoever also wants the term stored.  Four accumulators take rows m0 + 4 i + j
// (j = 0..3), the rows left over at the end go to the first, and the block's sum is (s0 + s1) + (s2 + s3): a fixed function of
// (M, row block).  U groups of four rows are in flight at a time - U moves loads, never a sum.
template <bool ABSMAX, int U, typename T, typename Row, typename Sink> __device__ __forceinline__ T cs_block(Row row, Sink sink, long m0, long m1)
{
    T s[4] = {};
    long m = m0;
    if constexpr (U > 1)
        for (; m + 4 * U - 1 < m1; m += 4 * U) cs_rows<ABSMAX, 4 * U>(row, sink, m, s);
    for (; m + 3 < m1; m += 4) cs_rows<ABSMAX, 4>(row, sink, m, s);
    for (; m < m1; ++m) {
        const T v = row(m);
        sink(m, v);
        s[0] = cs_op<ABSMAX>(s[0], v);
    }
    if constexpr (ABSMAX) return fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    else return (s[0] + s[1]) + (s[2] + s[3]);
}

// stage 1: part[blockIdx.x][n] = sum of rows [blockIdx.x * CS_ROWS, +CS_ROWS) of x[:, n]; a thread owns a column
template <bool ABSMAX>
__global__ void __launch_bounds__(256) colsum_stage1(const float *__restrict__ x, float *__restrict__ part, long M, int N, long ld)
{
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= N) return;
    const long m0 = (long)blockIdx.x * CS_ROWS, m1 = m0 + CS_ROWS < M ? m0 + CS_ROWS : M;
    part[(long)blockIdx.x * N + n] = cs_block<ABSMAX, 1, float>([&](long m) { return x[m * ld + n]; }, [](long, float) {}, m0, m1);
}

// ---- ReLU backward + bf16 copy + stage 1 of the column sum, one pass over dy and act (grad_dtype="bf16" of the detector) ----------
constexpr int RB_GROUPS = 4;                                         // 16 rows of dy (and act) in flight per thread
template <int V> struct cols_t { typedef float f; };                 // the V adjacent columns of a thread
template <> struct cols_t<4> { typedef f32x4 f; };

template <typename A, int V> struct act_cols_t { typedef typename cols_t<V>::f t; };    // V adjacent elements of the activation
template <> struct act_cols_t<__bf16, 1> { typedef __bf16 t; };
template <> struct act_cols_t<__bf16, 4> { typedef bf16x4_t t; };                         // one 8-byte load

// w = act > 0 ? dy : 0 - a selection (threshold_backward): a masked non-finite dy is 0, act = +-0 or NaN masks.  ACT = false: w = dy.
// A: the activation's element type, float or __bf16 - a bf16 widens exactly (subnormals kept), so the mask is that of its fp32 copy
template <int V, bool ACT, typename A> __device__ __forceinline__ typename cols_t<V>::f relu_bwd_load(const float *__restrict__ dy, const A *__restrict__ act)
{
    typedef typename cols_t<V>::f F;
    F v = *reinterpret_cast<const F *>(dy);
    if constexpr (ACT) {
        const auto a = *reinterpret_cast<const typename act_cols_t<A, V>::t *>(act);
        if constexpr (V == 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (float)a[e] > 0.f ? v[e] : 0.f;
        } else {
            v = (float)a > 0.f ? v : 0.f;
        }
    }
    return v;
}

template <int V> __device__ __forceinline__ void store_bf16(__bf16 *__restrict__ dst, typename cols_t<V>::f v)
{
    if constexpr (V == 4) *reinterpret_cast<bf16x4_t *>(dst) = bf16x4_t{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    else *dst = (__bf16)v;
}

// out[m, n] = bf16(w[m, n]); part[blockIdx.x][n] (part != nullptr) = colsum_stage1's partial of w: the grid of colsum_stage1 with V
// columns per thread and blockDim.x threads per block
template <int V, bool ACT, typename A>
__global__ void __launch_bounds__(256) relu_bwd_bf16(const float *__restrict__ dy, const A *__restrict__ act, __bf16 *__restrict__ out,
                                                     float *__restrict__ part, long M, int N, long lddy, long ldact, long ldout)
{
    typedef typename cols_t<V>::f F;
    const long n = ((long)blockIdx.y * blockDim.x + threadIdx.x) * V;
    if (n >= N) return;
    const long m0 = (long)blockIdx.x * CS_ROWS, m1 = m0 + CS_ROWS < M ? m0 + CS_ROWS : M;
    const F s = cs_block<false, RB_GROUPS, F>([&](long m) { return relu_bwd_load<V, ACT, A>(dy + m * lddy + n, act + m * ldact + n); },
                                   [&](long m, F v) { store_bf16<V>(out + m * ldout + n, v); }, m0, m1);
    if (part) *reinterpret_cast<F *>(part + (long)blockIdx.x * N + n) = s;
}

// The same into the zero-padded map of pad_nhwc_bf16, out bf16 [B, H+2, W+2, C]: row m = (b, y, x) of dy lands on pixel
// (b, y+1, x+1), and the thread that writes an interior pixel at the map's edge also writes the border pixels beside it (a corner
// goes with the corner pixel) - every element of out is written exactly once.
template <bool ACT, typename A>
__global__ void __launch_bounds__(256) relu_bwd_pad_nhwc_bf16(const float *__restrict__ dy, const A *__restrict__ act,
                                                              __bf16 *__restrict__ out, float *__restrict__ part, int M, int H, int W, int C)
{
    const int c = (blockIdx.y * blockDim.x + threadIdx.x) * 4;
    if (c >= C) return;
    const long m0 = (long)blockIdx.x * CS_ROWS, m1 = m0 + CS_ROWS < M ? m0 + CS_ROWS : (long)M;
    const long rs = (long)(W + 2) * C;                               // one padded row
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 s = cs_block<false, RB_GROUPS, f32x4>([&](long m) { return relu_bwd_load<4, ACT, A>(dy + m * C + c, act + m * C + c); },
                                           [&](long m, f32x4 v) {
        const int x = (int)m % W, t = (int)m / W, y = t % H, b = t / H;                   // (uniform over the workgroup)
        __bf16 *o = out + (((long)b * (H + 2) + y + 1) * (W + 2) + x + 1) * C + c;
        store_bf16<4>(o, v);
        if (x == 0) store_bf16<4>(o - C, zero);
        if (x == W - 1) store_bf16<4>(o + C, zero);
        if (y == 0) {
            store_bf16<4>(o - rs, zero);
            if (x == 0) store_bf16<4>(o - rs - C, zero);
            if (x == W - 1) store_bf16<4>(o - rs + C, zero);
        }
        if (y == H - 1) {
            store_bf16<4>(o + rs, zero);
            if (x == 0) store_bf16<4>(o + rs - C, zero);
            if (x == W - 1) store_bf16<4>(o + rs + C, zero);
        } }, m0, m1);
    if (part) *reinterpret_cast<f32x4 *>(part + (long)blockIdx.x * C + c) = s;
}

template <bool ABSMAX>
__global__ void __launch_bounds__(256) colsum_stage2(const float *__restrict__ part, float *__restrict__ out, int P, int N)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s = ABSMAX ? fmaxf(s, part[(long)p * N + n]) : s + part[(long)p * N + n];
    out[n] = s;
}

}  // namespace

int launch_fpn_merge_bwd(const float *din, float *dlat, float *dtop, int B, int Gh, int Gw, int Ch, float scale, int top_h, int top_w,
                         hipStream_t stream)
{
    if (B <= 0 || Gh <= 0 || Gw <= 0 || Ch <= 0 || (Ch & 3)) return fail(LDIT_EINVAL, "fpn_merge_bwd: bad geometry");
    if (!(scale == 4.0f || scale == 2.0f || scale == 1.0f || scale == 0.5f)) return fail(LDIT_EUNSUPPORTED, "fpn_merge_bwd: scale %g not in {4,2,1,0.5}", (double)scale);
    if (!din || !aligned16(din) || (dlat && !aligned16(dlat)) || (dtop && !aligned16(dtop))) return fail(LDIT_EINVAL, "fpn_merge_bwd: null or misaligned operand");
    const int Oh = (int)((float)Gh * scale), Ow = (int)((float)Gw * scale);
    if (Oh <= 0 || Ow <= 0) return fail(LDIT_EINVAL, "fpn_merge_bwd: map collapses to zero size");
    if (dtop && (top_h <= 0 || top_w <= 0)) return fail(LDIT_EINVAL, "fpn_merge_bwd: bad top size");
    if ((size_t)B * Oh * Ow * (Ch >> 2) >= (1ull << 31)) return fail(LDIT_EUNSUPPORTED, "fpn_merge_bwd: map exceeds 2^31 vectors");
    if (dlat) {
        const size_t total = (size_t)B * Gh * Gw * (Ch >> 2);
        hipLaunchKernelGGL(fpn_merge_bwd_lat, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, din, dlat, B, Gh, Gw, Ch, Oh, Ow,
                           scale);
        LDIT_HIP_CHECK(hipGetLastError());
    }
    if (dtop) {
        const size_t total = (size_t)B * top_h * top_w * (Ch >> 2);
        hipLaunchKernelGGL(fpn_merge_bwd_top, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, din, dtop, B, Ch, Oh, Ow,
                           top_h, top_w);
        LDIT_HIP_CHECK(hipGetLastError());
    }
    return LDIT_OK;
}

int launch_pad_nhwc_bf16(const float *src, void *dst, int B, int H, int W, int C, hipStream_t stream)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return fail(LDIT_EINVAL, "pad_nhwc_bf16: bad geometry");
    if (!src || !dst || !aligned16(src) || (reinterpret_cast<uintptr_t>(dst) & 7u)) return fail(LDIT_EINVAL, "pad_nhwc_bf16: null or misaligned operand");
    const size_t total = (size_t)B * (H + 2) * (W + 2) * (C >> 2);
    if (total >= (1ull << 31)) return fail(LDIT_EUNSUPPORTED, "pad_nhwc_bf16: map exceeds 2^31 vectors");
    hipLaunchKernelGGL(pad_nhwc_bf16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, static_cast<__bf16 *>(dst), B, H, W, C);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

size_t colsum_scratch_bytes(int64_t M, int64_t N) { return (size_t)((M + CS_ROWS - 1) / CS_ROWS) * (size_t)N * sizeof(float); }

int launch_colsum_f32(const float *x, int64_t M, int N, int64_t ld, float *out, float *scratch, size_t scratch_bytes, bool absmax,
                      hipStream_t stream)
{
    if (M <= 0 || N <= 0 || ld < N) return fail(LDIT_EINVAL, "colsum: bad geometry");
    if (!x || !out || !scratch) return fail(LDIT_EINVAL, "colsum: null operand");
    if (scratch_bytes < colsum_scratch_bytes(M, N)) return fail(LDIT_EWORKSPACE, "colsum: scratch %zu bytes < required %zu", scratch_bytes, colsum_scratch_bytes(M, N));
    const long P = (M + CS_ROWS - 1) / CS_ROWS;
    if (P > 65535L * 32768L) return fail(LDIT_EUNSUPPORTED, "colsum: too many rows");
    const dim3 g1((unsigned)P, (unsigned)((N + 255) / 256)), g2((unsigned)((N + 255) / 256));
    if (absmax) {
        hipLaunchKernelGGL(colsum_stage1<true>, g1, dim3(256), 0, stream, x, scratch, (long)M, N, (long)ld);
        hipLaunchKernelGGL(colsum_stage2<true>, g2, dim3(256), 0, stream, scratch, out, (int)P, N);
    } else {
        hipLaunchKernelGGL(colsum_stage1<false>, g1, dim3(256), 0, stream, x, scratch, (long)M, N, (long)ld);
        hipLaunchKernelGGL(colsum_stage2<false>, g2, dim3(256), 0, stream, scratch, out, (int)P, N);
    }
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

// threads per block for `cols` column groups: whole waves, at most 256
static unsigned relu_bwd_threads(long cols) { return cols > 128 ? 256u : cols > 64 ? 128u : 64u; }

static int relu_bwd_stage2(float *colsum, float *scratch, int64_t M, int N, hipStream_t stream)
{
    if (colsum) hipLaunchKernelGGL(colsum_stage2<false>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, scratch, colsum,
                                   (int)((M + CS_ROWS - 1) / CS_ROWS), N);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

// A: the activation's element type (float: the entry points of grad_dtype="bf16"; __bf16: their *_act16 forms); `name` heads the messages
template <typename A>
static int relu_bwd_bf16_any(const char *name, const float *dy, int64_t lddy, const A *act, int64_t ldact, void *out, int64_t ldout, int64_t M,
                             int64_t N, float *colsum, float *scratch, size_t scratch_bytes, hipStream_t stream)
{
    if (M <= 0 || N <= 0 || lddy < N || ldout < N || (act && ldact < N)) return fail(LDIT_EINVAL, "%s: bad geometry", name);
    if (!dy || !out || (colsum && !scratch)) return fail(LDIT_EINVAL, "%s: null operand", name);
    const auto addr = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    if ((addr(dy) & 3u) || (addr(act) & (sizeof(A) - 1)) || (addr(out) & 1u) || (addr(colsum) & 3u) || (addr(scratch) & 3u))
        return fail(LDIT_EINVAL, "%s: misaligned operand", name);
    if (M >= (1ll << 31) || N >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "%s: 2^31 rows or columns or more", name);
    if (colsum && scratch_bytes < colsum_scratch_bytes(M, N))
        return fail(LDIT_EWORKSPACE, "%s: scratch %zu bytes < required %zu", name, scratch_bytes, colsum_scratch_bytes(M, N));
    const unsigned P = (unsigned)((M + CS_ROWS - 1) / CS_ROWS);
    float *part = colsum ? scratch : nullptr;
    __bf16 *o = static_cast<__bf16 *>(out);
    // four columns per thread where every row of every operand starts on a vector boundary (act: four of its elements)
    const bool vec = !(N & 3) && !(lddy & 3) && !(ldout & 3) && (!act || !(ldact & 3)) && aligned16(dy) && !(addr(act) & (4 * sizeof(A) - 1)) &&
                     !(addr(out) & 7u) && (!part || aligned16(part));
    const int64_t cols = vec ? N / 4 : N;
    const unsigned th = relu_bwd_threads(cols);
    const dim3 grid(P, (unsigned)((cols + th - 1) / th));
    if (grid.y > 65535u) return fail(LDIT_EUNSUPPORTED, "%s: too many columns", name);
    auto kernel = vec ? (act ? relu_bwd_bf16<4, true, A> : relu_bwd_bf16<4, false, A>) : (act ? relu_bwd_bf16<1, true, A> : relu_bwd_bf16<1, false, A>);
    hipLaunchKernelGGL(kernel, grid, dim3(th), 0, stream, dy, act, o, part, (long)M, (int)N, (long)lddy, (long)ldact, (long)ldout);
    return relu_bwd_stage2(colsum, scratch, M, (int)N, stream);
}

template <typename A>
static int relu_bwd_pad_nhwc_bf16_any(const char *name, const float *dy, const A *act, void *out, int64_t B, int64_t H, int64_t W, int64_t C,
                                      float *colsum, float *scratch, size_t scratch_bytes, hipStream_t stream)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return fail(LDIT_EINVAL, "%s: bad geometry", name);
    if (!dy || !out || (colsum && !scratch)) return fail(LDIT_EINVAL, "%s: null operand", name);
    if (!aligned16(dy) || (reinterpret_cast<uintptr_t>(act) & (4 * sizeof(A) - 1)) || (reinterpret_cast<uintptr_t>(out) & 7u) ||
        (colsum && (!aligned16(scratch) || (reinterpret_cast<uintptr_t>(colsum) & 3u))))
        return fail(LDIT_EINVAL, "%s: misaligned operand", name);
    const int64_t lim = 1ll << 31;
    // (each factor first: the products below stay inside 64 bits)
    if (B >= lim || H >= lim || W >= lim || C >= lim || B * H >= lim || B * H * W >= lim || (B * (H + 2)) * (W + 2) >= lim ||
        (B * (H + 2)) * (W + 2) * C >= (1ll << 33))
        return fail(LDIT_EUNSUPPORTED, "%s: 2^31 pixel rows or a padded map of 2^33 elements or more", name);
    const int64_t M = B * H * W;
    if (colsum && scratch_bytes < colsum_scratch_bytes(M, C))
        return fail(LDIT_EWORKSPACE, "%s: scratch %zu bytes < required %zu", name, scratch_bytes, colsum_scratch_bytes(M, C));
    const unsigned P = (unsigned)((M + CS_ROWS - 1) / CS_ROWS), th = relu_bwd_threads(C / 4);
    if ((C / 4 + th - 1) / th > 65535) return fail(LDIT_EUNSUPPORTED, "%s: too many channels", name);
    auto kernel = act ? relu_bwd_pad_nhwc_bf16<true, A> : relu_bwd_pad_nhwc_bf16<false, A>;
    hipLaunchKernelGGL(kernel, dim3(P, (unsigned)((C / 4 + th - 1) / th)), dim3(th), 0, stream, dy, act, static_cast<__bf16 *>(out),
                       colsum ? scratch : nullptr, (int)M, (int)H, (int)W, (int)C);
    return relu_bwd_stage2(colsum, scratch, M, (int)C, stream);
}

int launch_relu_bwd_bf16(const float *dy, int64_t lddy, const float *act, int64_t ldact, void *out, int64_t ldout, int64_t M, int64_t N,
                         float *colsum, float *scratch, size_t scratch_bytes, hipStream_t stream)
{
    return relu_bwd_bf16_any("relu_bwd_bf16", dy, lddy, act, ldact, out, ldout, M, N, colsum, scratch, scratch_bytes, stream);
}

int launch_relu_bwd_pad_nhwc_bf16(const float *dy, const float *act, void *out, int64_t B, int64_t H, int64_t W, int64_t C, float *colsum,
                                  float *scratch, size_t scratch_bytes, hipStream_t stream)
{
    return relu_bwd_pad_nhwc_bf16_any("relu_bwd_pad_nhwc_bf16", dy, act, out, B, H, W, C, colsum, scratch, scratch_bytes, stream);
}

int launch_relu_bwd_bf16_act16(const float *dy, int64_t lddy, const void *act, int64_t ldact, void *out, int64_t ldout, int64_t M, int64_t N,
                               float *colsum, float *scratch, size_t scratch_bytes, hipStream_t stream)
{
    return relu_bwd_bf16_any("relu_bwd_bf16_act16", dy, lddy, static_cast<const __bf16 *>(act), ldact, out, ldout, M, N, colsum, scratch,
                             scratch_bytes, stream);
}

int launch_relu_bwd_pad_nhwc_bf16_act16(const float *dy, const void *act, void *out, int64_t B, int64_t H, int64_t W, int64_t C, float *colsum,
                                        float *scratch, size_t scratch_bytes, hipStream_t stream)
{
    return relu_bwd_pad_nhwc_bf16_any("relu_bwd_pad_nhwc_bf16_act16", dy, static_cast<const __bf16 *>(act), out, B, H, W, C, colsum, scratch,
                                      scratch_bytes, stream);
}

}  // namespace ldit
