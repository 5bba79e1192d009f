// The detector's optimizer step: the non-finite check, the loss-scale / step-count state machine and one AdamW
// over MANY unrelated parameter tensors ("segments") in a fixed number of launches, with every decision in device memory.
//
// A segment is {p, g, m, v, n, bf16_mirror}: four fp32 device pointers of n elements each (any 4-byte alignment, n >= 0) and an
// optional bf16 copy of p.  Up to OPT_SEGS segments travel BY VALUE in the kernel arguments together with a prefix table that maps
// a block index to its segment (reduce_jobs_kernel's scheme, train_ops.hip): no table is copied to the device and nothing is
// allocated, so the step neither synchronises nor breaks a graph capture.  A workgroup owns 1024 consecutive elements of ONE
// segment.  Where p, g, m and v of a segment are all 16-byte aligned (and the mirror 8-byte) a thread moves one 16-byte quad and the
// last n % 4 elements go one by one; any other segment is walked element by element, a wave on consecutive addresses.
//
// Three launches, because each needs the one before it complete on the WHOLE parameter set: the update may not touch a single element
// before every gradient element was seen finite, and the step count / bias corrections / loss scale change once per step, not per block.
//
// With global-norm clipping and parameter groups the sequence is check + sum of squares (one pass, one double
// partial per workgroup), the state machine, ldit_clip_finish (one workgroup: the norm and the clip coefficient into the 16-byte
// ldit_clip_state) and adamw_groups_multi_kernel: adamw_multi_kernel with a per-segment {lr_scale, weight_decay} beside the table.
//
// Gradient accumulation and data-parallel ranks put one launch in front of all that: grads_accumulate_kernel folds
// the gradient tensors into the slices of one flat bucket (acc = g, or acc = acc + g), 127 {acc, g, n} segments per launch by the
// same scheme, and the launches above then read the bucket's slices as their gradients.
//
// An exponential moving average of the weights is the grouped update's launch with one more fp32 pointer per
// segment beside the table: adamw_ema_groups_multi_kernel reads and writes the shadow element next to the p it just formed.
// swap_multi_kernel exchanges weights and shadows (99 {a, b, n, mirror} segments per launch) for an evaluation on the average.
#include "api_internal.h"

namespace ldit {

namespace {

typedef __bf16 bf16_t;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int OPT_SEGS = 64;              // segments per launch: 64 x 48 bytes + the prefix table stay under the 4 KB of kernel arguments
constexpr int OPT_BLOCK_ELEMS = 1024;     // elements per workgroup (256 threads x one quad)
constexpr int64_t OPT_MAX_BLOCKS = 0x7fffffff;

struct OptLaunch {
    ldit_opt_segment seg[OPT_SEGS];
    int first_block[OPT_SEGS + 1];        // first_block[j] = blocks of segments 0 .. j-1; [n] = the grid
    int n;
};
static_assert(sizeof(OptLaunch) <= 3584, "the segment table must fit the kernel-argument block beside the scalars");

constexpr int GROUP_SEGS = 48;            // the grouped update: 48 x (48 + 8) bytes + the prefix table, under the same 3584
struct GroupLaunch {
    ldit_opt_segment seg[GROUP_SEGS];
    int first_block[GROUP_SEGS + 1];
    int n;
    ldit_opt_hyper hyper[GROUP_SEGS];
};
static_assert(sizeof(GroupLaunch) <= 3584, "the segment table must fit the kernel-argument block beside the scalars");

constexpr int ACC_SEGS = 127;             // the fold into the bucket: 127 x 24 bytes + the prefix table, under the same 3584
struct AccLaunch {
    ldit_acc_segment seg[ACC_SEGS];
    int first_block[ACC_SEGS + 1];
    int n;
};
static_assert(sizeof(AccLaunch) <= 3584, "the segment table must fit the kernel-argument block beside the scalars");

constexpr int EMA_SEGS = 52;              // the update with an EMA: 52 x (48 + 8 + 8) bytes + the prefix table, under the same 3584
struct EmaLaunch {
    ldit_opt_segment seg[EMA_SEGS];
    float *ema[EMA_SEGS];                 // the segment's fp32 shadow, or null: it has none
    ldit_opt_hyper hyper[EMA_SEGS];
    int first_block[EMA_SEGS + 1];
    int n;
};
static_assert(sizeof(EmaLaunch) <= 3584, "the segment table must fit the kernel-argument block beside the scalars");

constexpr int SWAP_SEGS = 99;             // the exchange: 99 x 32 bytes + the prefix table, under the same 3584
struct SwapLaunch {
    ldit_swap_segment seg[SWAP_SEGS];
    int first_block[SWAP_SEGS + 1];
    int n;
};
static_assert(sizeof(SwapLaunch) <= 3584, "the segment table must fit the kernel-argument block beside the scalars");

template <typename T> struct launch_cap;
template <> struct launch_cap<OptLaunch> { static constexpr int value = OPT_SEGS; };
template <> struct launch_cap<GroupLaunch> { static constexpr int value = GROUP_SEGS; };
template <> struct launch_cap<AccLaunch> { static constexpr int value = ACC_SEGS; };
template <> struct launch_cap<EmaLaunch> { static constexpr int value = EMA_SEGS; };
template <> struct launch_cap<SwapLaunch> { static constexpr int value = SWAP_SEGS; };

// the segment of this block: the last j with first_block[j] <= blk (every segment in a launch has at least one block)
template <typename T>
__device__ __forceinline__ int find_segment(const T &a, int blk)
{
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk >= a.first_block[mid]) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool quad_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// ---- 1. found_inf |= "some gradient element is NaN or +-inf" -------------------------------------------------------------------
// one ballot per wave, one integer atomic per offending workgroup, no float atomics
__global__ void __launch_bounds__(256) grads_check_kernel(const OptLaunch a, ldit_opt_state *__restrict__ st)
{
    __shared__ int flag;
    const int tid = threadIdx.x;
    const int j = find_segment(a, (int)blockIdx.x);
    const float *g = static_cast<const float *>(a.seg[j].g);
    const int64_t n = a.seg[j].n;
    const int64_t base = (int64_t)((int)blockIdx.x - a.first_block[j]) * OPT_BLOCK_ELEMS;
    bool bad = false;
    if (quad_aligned(g)) {
        const int64_t i = base + 4 * tid;
        if (i + 4 <= n) {
            const f32x4 G = *reinterpret_cast<const f32x4 *>(g + i);
            bad = nonfinite(G[0]) || nonfinite(G[1]) || nonfinite(G[2]) || nonfinite(G[3]);
        } else {
            for (int64_t e = i; e < n; ++e) bad |= nonfinite(g[e]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t e = base + tid + 256 * k;
            if (e < n) bad |= nonfinite(g[e]);
        }
    }
    if (tid == 0) flag = 0;
    __syncthreads();
    if (__ballot(bad) != 0ull && (tid & 63) == 0) flag = 1;
    __syncthreads();
    if (tid == 0 && flag) atomicOr(&st->found_inf, 1);
}

// ---- 1b. the same check and, in the same pass, this workgroup's sum of squares -----------------------------------------------------
// The squares arrive loss-scaled (x 65 536 and more) and a finite fp32 square can overflow fp32, so a thread squares and adds in
// double.  Lanes of a wave by the butterfly of layernorm.hip's wave_sum, the four waves through LDS one after another by thread 0:
// a fixed order, so equal inputs give equal bits.  A NaN or an infinity makes the partial non-finite, which ldit_clip_finish passes on.
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ void __launch_bounds__(256) grads_check_norm_kernel(const OptLaunch a, ldit_opt_state *__restrict__ st, double *__restrict__ partials,
                                                               int64_t launch_base)
{
    __shared__ int flag;
    __shared__ double wave_part[4];
    const int tid = threadIdx.x;
    const int j = find_segment(a, (int)blockIdx.x);
    const float *g = static_cast<const float *>(a.seg[j].g);
    const int64_t n = a.seg[j].n;
    const int64_t base = (int64_t)((int)blockIdx.x - a.first_block[j]) * OPT_BLOCK_ELEMS;
    bool bad = false;
    double ss = 0.0;
    if (quad_aligned(g)) {
        const int64_t i = base + 4 * tid;
        if (i + 4 <= n) {
            const f32x4 G = *reinterpret_cast<const f32x4 *>(g + i);
            bad = nonfinite(G[0]) || nonfinite(G[1]) || nonfinite(G[2]) || nonfinite(G[3]);
            ss = (sq(G[0]) + sq(G[1])) + (sq(G[2]) + sq(G[3]));
        } else {
            for (int64_t e = i; e < n; ++e) {
                const float x = g[e];
                bad |= nonfinite(x);
                ss += sq(x);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t e = base + tid + 256 * k;
            if (e < n) {
                const float x = g[e];
                bad |= nonfinite(x);
                ss += sq(x);
            }
        }
    }
    ss = wave_sum_f64(ss);
    const bool wave_bad = __ballot(bad) != 0ull;     // by the whole wave, before the leaders part from it
    if (tid == 0) flag = 0;
    __syncthreads();
    if ((tid & 63) == 0) {
        wave_part[tid >> 6] = ss;
        if (wave_bad) flag = 1;
    }
    __syncthreads();
    if (tid == 0) {
        partials[launch_base + blockIdx.x] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
        if (flag) atomicOr(&st->found_inf, 1);
    }
}

// ---- 2. the state machine of torch.amp.GradScaler.step / update and of the optimizer's step count, one thread ------------------
__global__ void opt_advance_kernel(ldit_opt_state *__restrict__ st, double b1, double b2, float growth, float backoff, int interval)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int skip = st->found_inf != 0;
    st->skip = skip;
    st->inv_scale_used = 1.0f / st->scale;          // of the scale the backward ran with, before it changes below
    st->found_inf = 0;
    if (!skip) {
        const int step = st->step + 1;
        st->step = step;
        st->bc1 = (float)(1.0 - pow(b1, (double)step));
        st->bc2_sqrt = (float)sqrt(1.0 - pow(b2, (double)step));
        const int t = st->growth_tracker + 1;
        if (t >= interval) {
            st->scale = st->scale * growth;
            st->growth_tracker = 0;
        } else {
            st->growth_tracker = t;
        }
    } else {
        st->scale = st->scale * backoff;
        st->growth_tracker = 0;
        st->skipped_steps = st->skipped_steps + 1;
    }
}

// ---- 3. AdamW over the segments: adamw_kernel's statements (train_ops.hip) in its order, constants from the state block ---------
// 1 - beta arrives as its own argument, formed in double on the host and rounded once: 1.0f - 0.999f is 4.7e-5 off 0.001, which puts
// exp_avg_sq 70x further from the float64 result than torch.optim.AdamW (which hands addcmul_ the double 1 - beta2) ever is.
struct AdamwConsts { float b1, omb1, b2, omb2, eps, step, decay, bc2_sqrt, gs; };

__device__ __forceinline__ void adamw_element(float &P, const float G, float &Mo, float &Vo, const AdamwConsts &c)
{
    const float gr = G * c.gs;
    const float mo = c.b1 * Mo + c.omb1 * gr;
    const float vo = c.b2 * Vo + c.omb2 * (gr * gr);      // the square first, as torch's addcmul_(g, g, value = 1 - beta2) forms it
    const float denom = sqrtf(vo) / c.bc2_sqrt + c.eps;
    P = P * c.decay - c.step * (mo / denom);
    Mo = mo;
    Vo = vo;
}

// the constants of one segment's update from the block; lr is the segment's own learning rate (the block's, times its lr_scale)
__device__ __forceinline__ AdamwConsts adamw_consts(const ldit_opt_state *__restrict__ st, double lr, float wd, float gs, float b1, float omb1,
                                                    float b2, float omb2, float eps)
{
    AdamwConsts c;
    c.b1 = b1; c.omb1 = omb1; c.b2 = b2; c.omb2 = omb2; c.eps = eps;
    // lr and bc1 are floats in the block: their quotient is formed in double and rounded once, like torch's lr / (1 - beta1^t) on
    // Python floats - a float division rounds a second time and lands one ulp off that in about half of all cases
    c.step = (float)(lr / (double)st->bc1);
    c.decay = 1.0f - (float)lr * wd;
    c.bc2_sqrt = st->bc2_sqrt;
    c.gs = gs;
    return c;
}

// the moving average of the weights, on the P the update just formed: one fp32 multiply-add, E + w (P - E)
__device__ __forceinline__ float ema_element(const float E, const float P, const float w) { return E + w * (P - E); }

// this workgroup's 1024 elements of one segment, from element `base` on.  EMA: `shadow` (null: this segment has none) moves towards
// the new p by the weight w in the same pass; without EMA neither is looked at and the code is the update's alone.
template <bool EMA>
__device__ __forceinline__ void adamw_block(const ldit_opt_segment &sg, const int64_t base, const int tid, const AdamwConsts &c,
                                            float *shadow = nullptr, const float w = 0.0f)
{
    float *p = static_cast<float *>(sg.p), *m = static_cast<float *>(sg.m), *v = static_cast<float *>(sg.v);
    const float *g = static_cast<const float *>(sg.g);
    bf16_t *mirror = static_cast<bf16_t *>(sg.bf16_mirror);
    const int64_t n = sg.n;
    const bool vec = quad_aligned(p) && quad_aligned(g) && quad_aligned(m) && quad_aligned(v) &&
                     (reinterpret_cast<uintptr_t>(mirror) & 7u) == 0 && (!EMA || quad_aligned(shadow));
    if (vec) {
        const int64_t i = base + 4 * tid;
        if (i + 4 <= n) {
            f32x4 P = *reinterpret_cast<f32x4 *>(p + i), Mo = *reinterpret_cast<f32x4 *>(m + i), Vo = *reinterpret_cast<f32x4 *>(v + i);
            const f32x4 G = *reinterpret_cast<const f32x4 *>(g + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = P[e], me = Mo[e], ve = Vo[e];
                adamw_element(pe, G[e], me, ve, c);
                P[e] = pe; Mo[e] = me; Vo[e] = ve;
            }
            *reinterpret_cast<f32x4 *>(p + i) = P;
            if (mirror) *reinterpret_cast<bf16x4 *>(mirror + i) = bf16x4{(bf16_t)P[0], (bf16_t)P[1], (bf16_t)P[2], (bf16_t)P[3]};
            *reinterpret_cast<f32x4 *>(m + i) = Mo;
            *reinterpret_cast<f32x4 *>(v + i) = Vo;
            if (EMA && shadow) {
                f32x4 E = *reinterpret_cast<f32x4 *>(shadow + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) E[e] = ema_element(E[e], P[e], w);
                *reinterpret_cast<f32x4 *>(shadow + i) = E;
            }
        } else {
            for (int64_t e = i; e < n; ++e) {        // the last n % 4 elements of the segment
                float P = p[e], Mo = m[e], Vo = v[e];
                adamw_element(P, g[e], Mo, Vo, c);
                p[e] = P; m[e] = Mo; v[e] = Vo;
                if (mirror) mirror[e] = (bf16_t)P;
                if (EMA && shadow) shadow[e] = ema_element(shadow[e], P, w);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t e = base + tid + 256 * k;
            if (e < n) {
                float P = p[e], Mo = m[e], Vo = v[e];
                adamw_element(P, g[e], Mo, Vo, c);
                p[e] = P; m[e] = Mo; v[e] = Vo;
                if (mirror) mirror[e] = (bf16_t)P;
                if (EMA && shadow) shadow[e] = ema_element(shadow[e], P, w);
            }
        }
    }
}

__global__ void __launch_bounds__(256) adamw_multi_kernel(const OptLaunch a, const ldit_opt_state *__restrict__ st, float b1, float omb1,
                                                          float b2, float omb2, float eps, float wd, float grad_mul)
{
    if (st->skip) return;                            // a skipped step writes nothing at all
    const int j = find_segment(a, (int)blockIdx.x);
    const int64_t base = (int64_t)((int)blockIdx.x - a.first_block[j]) * OPT_BLOCK_ELEMS;
    const AdamwConsts c = adamw_consts(st, (double)st->lr, wd, grad_mul * st->inv_scale_used, b1, omb1, b2, omb2, eps);
    adamw_block<false>(a.seg[j], base, threadIdx.x, c);
}

// ---- 3b. the same update with the segment's own {lr_scale, weight_decay} and the clip coefficient in the gradient multiplier -------
// lr * lr_scale is formed in double and enters the step size unrounded; with lr_scale == 1 it is the block's lr bit for bit, with
// clip_coef == 1 (or no clip block) the multiplier is inv_scale_used bit for bit: then this IS adamw_multi_kernel(grad_mul = 1).
__global__ void __launch_bounds__(256) adamw_groups_multi_kernel(const GroupLaunch a, const ldit_opt_state *__restrict__ st,
                                                                 const ldit_clip_state *__restrict__ clip, float b1, float omb1, float b2,
                                                                 float omb2, float eps)
{
    if (st->skip) return;
    const int j = find_segment(a, (int)blockIdx.x);
    const int64_t base = (int64_t)((int)blockIdx.x - a.first_block[j]) * OPT_BLOCK_ELEMS;
    const float gs = clip ? clip->clip_coef * st->inv_scale_used : st->inv_scale_used;
    const AdamwConsts c = adamw_consts(st, (double)st->lr * (double)a.hyper[j].lr_scale, a.hyper[j].weight_decay, gs, b1, omb1, b2, omb2, eps);
    adamw_block<false>(a.seg[j], base, threadIdx.x, c);
}

// ---- 3c. the grouped update with an exponential moving average of the weights in the same launch ----------------
// The weight of this step from the block: decay, or min(decay, (1 + step) / (10 + step)) under warmup, step the count of steps TAKEN
// (opt_advance ran: this one included), so a skipped step does not age the warmup and the host needs no count.  In double, 1 - d
// rounded to float once.  Everything else is adamw_groups_multi_kernel's.
__global__ void __launch_bounds__(256) adamw_ema_groups_multi_kernel(const EmaLaunch a, const ldit_opt_state *__restrict__ st,
                                                                     const ldit_clip_state *__restrict__ clip, float b1, float omb1, float b2,
                                                                     float omb2, float eps, double ema_decay, int ema_warmup)
{
    if (st->skip) return;                            // a skipped step writes nothing at all: no shadow moves either
    const int j = find_segment(a, (int)blockIdx.x);
    const int64_t base = (int64_t)((int)blockIdx.x - a.first_block[j]) * OPT_BLOCK_ELEMS;
    const float gs = clip ? clip->clip_coef * st->inv_scale_used : st->inv_scale_used;
    const AdamwConsts c = adamw_consts(st, (double)st->lr * (double)a.hyper[j].lr_scale, a.hyper[j].weight_decay, gs, b1, omb1, b2, omb2, eps);
    const double step = (double)st->step;
    const double d = ema_warmup ? fmin(ema_decay, (1.0 + step) / (10.0 + step)) : ema_decay;
    adamw_block<true>(a.seg[j], base, threadIdx.x, c, a.ema[j], (float)(1.0 - d));
}

// ---- 2b. the global norm and the clip coefficient, one workgroup, after the state machine ------------------------------------------
// Thread t adds partials t, t + 256, ... in that order, then a tree over the 256 sums in LDS: a fixed order.
__global__ void __launch_bounds__(256) clip_finish_kernel(const ldit_opt_state *__restrict__ st, ldit_clip_state *__restrict__ clip,
                                                          const double *__restrict__ partials, int64_t n)
{
    __shared__ double part[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < n; i += 256) s += partials[i];
    part[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid != 0) return;
    const float norm = (float)(sqrt(part[0]) * (double)st->inv_scale_used);
    clip->total_norm = norm;
    if (st->skip) return;                            // a skipped step: the (non-finite) norm and nothing else
    // torch.nn.utils.clip_grad_norm_'s formula on the two floats, formed in double and rounded once
    const float coef = (float)fmin(1.0, (double)clip->max_norm / ((double)norm + 1e-6));
    clip->clip_coef = coef;
    if (coef < 1.0f) clip->clipped_steps = clip->clipped_steps + 1;
}

// ---- 0. the fold into the bucket: acc = g (the bits, acc never read) or acc = acc + g (one fp32 addition per element) --------------
// Every element is read and written by exactly one thread: no atomics, nothing to reorder, equal inputs give equal bits.  The copy
// moves integers, so -0.0, NaN payloads and infinities arrive as they left.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool OVERWRITE>
__device__ __forceinline__ void fold_element(float *acc, const float *g, const int64_t e)
{
    if (OVERWRITE) reinterpret_cast<uint32_t *>(acc)[e] = reinterpret_cast<const uint32_t *>(g)[e];
    else acc[e] = acc[e] + g[e];
}

template <bool OVERWRITE>
__global__ void __launch_bounds__(256) grads_accumulate_kernel(const AccLaunch a)
{
    const int tid = threadIdx.x;
    const int j = find_segment(a, (int)blockIdx.x);
    float *acc = static_cast<float *>(a.seg[j].acc);
    const float *g = static_cast<const float *>(a.seg[j].g);
    const int64_t n = a.seg[j].n;
    const int64_t base = (int64_t)((int)blockIdx.x - a.first_block[j]) * OPT_BLOCK_ELEMS;
    if (quad_aligned(acc) && quad_aligned(g)) {
        const int64_t i = base + 4 * tid;
        if (i + 4 <= n) {
            if (OVERWRITE) {
                *reinterpret_cast<u32x4 *>(acc + i) = *reinterpret_cast<const u32x4 *>(g + i);
            } else {
                const f32x4 A = *reinterpret_cast<const f32x4 *>(acc + i), G = *reinterpret_cast<const f32x4 *>(g + i);
                *reinterpret_cast<f32x4 *>(acc + i) = f32x4{A[0] + G[0], A[1] + G[1], A[2] + G[2], A[3] + G[3]};
            }
        } else {
            for (int64_t e = i; e < n; ++e) fold_element<OVERWRITE>(acc, g, e);      // the last n % 4 elements of the segment
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t e = base + tid + 256 * k;
            if (e < n) fold_element<OVERWRITE>(acc, g, e);
        }
    }
}

// ---- the exchange of the weights with their averages: a <-> b as integers, bf16(new a) into the mirror ---------------------------------
// Every element is read and written by exactly one thread, so two launches are the identity bit for bit.
__device__ __forceinline__ void swap_element(uint32_t *a, uint32_t *b, bf16_t *mirror, const int64_t e)
{
    const uint32_t A = a[e], B = b[e];
    a[e] = B;
    b[e] = A;
    if (mirror) mirror[e] = (bf16_t)__uint_as_float(B);
}

__global__ void __launch_bounds__(256) swap_multi_kernel(const SwapLaunch s)
{
    const int tid = threadIdx.x;
    const int j = find_segment(s, (int)blockIdx.x);
    uint32_t *a = static_cast<uint32_t *>(s.seg[j].a), *b = static_cast<uint32_t *>(s.seg[j].b);
    bf16_t *mirror = static_cast<bf16_t *>(s.seg[j].bf16_mirror);
    const int64_t n = s.seg[j].n;
    const int64_t base = (int64_t)((int)blockIdx.x - s.first_block[j]) * OPT_BLOCK_ELEMS;
    if (quad_aligned(a) && quad_aligned(b) && (reinterpret_cast<uintptr_t>(mirror) & 7u) == 0) {
        const int64_t i = base + 4 * tid;
        if (i + 4 <= n) {
            const u32x4 A = *reinterpret_cast<const u32x4 *>(a + i), B = *reinterpret_cast<const u32x4 *>(b + i);
            *reinterpret_cast<u32x4 *>(a + i) = B;
            *reinterpret_cast<u32x4 *>(b + i) = A;
            if (mirror)
                *reinterpret_cast<bf16x4 *>(mirror + i) = bf16x4{(bf16_t)__uint_as_float(B[0]), (bf16_t)__uint_as_float(B[1]),
                                                                 (bf16_t)__uint_as_float(B[2]), (bf16_t)__uint_as_float(B[3])};
        } else {
            for (int64_t e = i; e < n; ++e) swap_element(a, b, mirror, e);      // the last n % 4 elements of the segment
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t e = base + tid + 256 * k;
            if (e < n) swap_element(a, b, mirror, e);
        }
    }
}

#define LAUNCH_CHECKED(...)              \
    do {                                 \
        hipLaunchKernelGGL(__VA_ARGS__); \
        LDIT_HIP_CHECK(hipGetLastError()); \
    } while (0)

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// all: the update's view of a segment (p, g, m, v and the mirror); else the check's (g alone).  Empty segments carry no pointer.
int validate(const char *what, const ldit_opt_segment *segs, int32_t S, const void *state, bool all)
{
    if (S < 0) return fail(LDIT_EINVAL, "%s: negative segment count %d", what, S);
    if (S > 0 && !segs) return fail(LDIT_EINVAL, "%s: null segment array", what);
    if (!state) return fail(LDIT_EINVAL, "%s: null state block", what);
    if (!aligned4(state)) return fail(LDIT_EINVAL, "%s: state block must be 4-byte aligned", what);
    for (int32_t s = 0; s < S; ++s) {
        const ldit_opt_segment &q = segs[s];
        if (q.n < 0) return fail(LDIT_EINVAL, "%s: segment %d has negative length %lld", what, s, (long long)q.n);
        if (q.n == 0) continue;
        if (q.n > OPT_MAX_BLOCKS * (int64_t)OPT_BLOCK_ELEMS) return fail(LDIT_EUNSUPPORTED, "%s: segment %d longer than 2^41 elements", what, s);
        if (!q.g || (all && (!q.p || !q.m || !q.v))) return fail(LDIT_EINVAL, "%s: segment %d has a null pointer", what, s);
        if (!aligned4(q.g) || (all && (!aligned4(q.p) || !aligned4(q.m) || !aligned4(q.v))))
            return fail(LDIT_EINVAL, "%s: segment %d: fp32 pointers must be 4-byte aligned", what, s);
        if (all && (reinterpret_cast<uintptr_t>(q.bf16_mirror) & 1u)) return fail(LDIT_EINVAL, "%s: segment %d: bf16 mirror must be 2-byte aligned", what, s);
    }
    return LDIT_OK;
}

// the launches of one entry point: segments in order, the table's capacity of non-empty ones (and at most 2^31 - 1 blocks) per
// launch.  launch(a, blocks, first) - `first` the host array's index of every slot of `a`, for what rides beside the segments.
template <typename T, typename Seg, typename F>
int for_each_launch(const Seg *segs, int32_t S, F &&launch)
{
    constexpr int CAP = launch_cap<T>::value;
    T a;
    int32_t index[CAP];
    a.n = 0;
    int64_t blocks = 0;
    for (int32_t s = 0; s < S; ++s) {
        if (segs[s].n == 0) continue;
        const int64_t nb = (segs[s].n + OPT_BLOCK_ELEMS - 1) / OPT_BLOCK_ELEMS;
        if (a.n == CAP || blocks + nb > OPT_MAX_BLOCKS) {
            a.first_block[a.n] = (int)blocks;
            if (int rc = launch(a, (unsigned)blocks, index)) return rc;
            a.n = 0;
            blocks = 0;
        }
        a.seg[a.n] = segs[s];
        a.first_block[a.n] = (int)blocks;
        index[a.n] = s;
        ++a.n;
        blocks += nb;
    }
    if (a.n > 0) {
        a.first_block[a.n] = (int)blocks;
        if (int rc = launch(a, (unsigned)blocks, index)) return rc;
    }
    return LDIT_OK;
}

// one partial per workgroup of the check, over validated segments
int64_t count_partials(const ldit_opt_segment *segs, int32_t S)
{
    int64_t total = 0;
    for (int32_t s = 0; s < S; ++s) total += (segs[s].n + OPT_BLOCK_ELEMS - 1) / OPT_BLOCK_ELEMS;
    return total;
}

int need_device()
{
    int dev = 0;
    LDIT_HIP_CHECK(hipGetDevice(&dev));          // no HIP device: LDIT_EHIP, there is no CPU path
    return LDIT_OK;
}

}  // namespace

}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_grads_check_multi_f32(const ldit_opt_segment *segs, int32_t S, ldit_opt_state *state, ldit_stream stream_)
{
    LDIT_TRY(validate("grads_check_multi", segs, S, state, false));
    LDIT_TRY(need_device());
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return for_each_launch<OptLaunch>(segs, S, [&](const OptLaunch &a, unsigned blocks, const int32_t *) -> int {
        LAUNCH_CHECKED(grads_check_kernel, dim3(blocks), dim3(256), 0, stream, a, state);
        return LDIT_OK;
    });
}

int ldit_opt_advance(ldit_opt_state *state, double beta1, double beta2, float growth_factor, float backoff_factor, int32_t growth_interval,
                     ldit_stream stream)
{
    if (!state || !aligned4(state)) return fail(LDIT_EINVAL, "opt_advance: null or misaligned state block");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(LDIT_EINVAL, "opt_advance: betas must lie in [0, 1)");
    if (!(growth_factor >= 1.0f) || !(backoff_factor > 0.0f && backoff_factor <= 1.0f))
        return fail(LDIT_EINVAL, "opt_advance: growth_factor must be >= 1 and backoff_factor in (0, 1]");
    if (growth_interval < 1) return fail(LDIT_EINVAL, "opt_advance: growth_interval must be at least 1");
    LDIT_TRY(need_device());
    LAUNCH_CHECKED(opt_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, beta1, beta2, growth_factor, backoff_factor,
                   growth_interval);
    return LDIT_OK;
}

int ldit_adamw_multi_f32(const ldit_opt_segment *segs, int32_t S, const ldit_opt_state *state, double beta1, double beta2, float eps,
                         float weight_decay, float grad_mul, ldit_stream stream_)
{
    LDIT_TRY(validate("adamw_multi", segs, S, state, true));
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(LDIT_EINVAL, "adamw_multi: betas must lie in [0, 1)");
    const float b1 = (float)beta1, omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    LDIT_TRY(need_device());
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return for_each_launch<OptLaunch>(segs, S, [&](const OptLaunch &a, unsigned blocks, const int32_t *) -> int {
        LAUNCH_CHECKED(adamw_multi_kernel, dim3(blocks), dim3(256), 0, stream, a, state, b1, omb1, b2, omb2, eps, weight_decay, grad_mul);
        return LDIT_OK;
    });
}

int ldit_grads_accumulate_multi_f32(const ldit_acc_segment *segs, int32_t S, int32_t overwrite, ldit_stream stream_)
{
    const char *what = "grads_accumulate_multi";
    if (S < 0) return fail(LDIT_EINVAL, "%s: negative segment count %d", what, S);
    if (S > 0 && !segs) return fail(LDIT_EINVAL, "%s: null segment array", what);
    for (int32_t s = 0; s < S; ++s) {
        const ldit_acc_segment &q = segs[s];
        if (q.n < 0) return fail(LDIT_EINVAL, "%s: segment %d has negative length %lld", what, s, (long long)q.n);
        if (q.n == 0) continue;
        if (q.n > OPT_MAX_BLOCKS * (int64_t)OPT_BLOCK_ELEMS)
            return fail(LDIT_EUNSUPPORTED, "%s: segment %d longer than 2^41 elements: its grid exceeds 2^31 - 1 blocks", what, s);
        if (!q.acc || !q.g) return fail(LDIT_EINVAL, "%s: segment %d has a null pointer", what, s);
        if (!aligned4(q.acc) || !aligned4(q.g)) return fail(LDIT_EINVAL, "%s: segment %d: fp32 pointers must be 4-byte aligned", what, s);
    }
    LDIT_TRY(need_device());
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return for_each_launch<AccLaunch>(segs, S, [&](const AccLaunch &a, unsigned blocks, const int32_t *) -> int {
        if (overwrite) LAUNCH_CHECKED(grads_accumulate_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
        else LAUNCH_CHECKED(grads_accumulate_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
        return LDIT_OK;
    });
}

int64_t ldit_grad_norm_partials(const ldit_opt_segment *segs, int32_t S)
{
    if (S < 0) return fail(LDIT_EINVAL, "grad_norm_partials: negative segment count %d", S), -1;
    if (S > 0 && !segs) return fail(LDIT_EINVAL, "grad_norm_partials: null segment array"), -1;
    for (int32_t s = 0; s < S; ++s)
        if (segs[s].n < 0) return fail(LDIT_EINVAL, "grad_norm_partials: segment %d has negative length %lld", s, (long long)segs[s].n), -1;
    return count_partials(segs, S);
}

int ldit_grads_check_norm_multi_f32(const ldit_opt_segment *segs, int32_t S, ldit_opt_state *state, double *partials, int64_t partials_len,
                                    ldit_stream stream_)
{
    LDIT_TRY(validate("grads_check_norm_multi", segs, S, state, false));
    if (partials_len < 0) return fail(LDIT_EINVAL, "grads_check_norm_multi: negative partials_len %lld", (long long)partials_len);
    const int64_t need = count_partials(segs, S);
    if (partials_len < need)
        return fail(LDIT_EINVAL, "grads_check_norm_multi: %lld partials for segments that need %lld", (long long)partials_len, (long long)need);
    if (need > 0 && !partials) return fail(LDIT_EINVAL, "grads_check_norm_multi: null partials buffer");
    if (reinterpret_cast<uintptr_t>(partials) & 7u) return fail(LDIT_EINVAL, "grads_check_norm_multi: partials must be 8-byte aligned");
    LDIT_TRY(need_device());
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int64_t base = 0;
    return for_each_launch<OptLaunch>(segs, S, [&](const OptLaunch &a, unsigned blocks, const int32_t *) -> int {
        LAUNCH_CHECKED(grads_check_norm_kernel, dim3(blocks), dim3(256), 0, stream, a, state, partials, base);
        base += blocks;
        return LDIT_OK;
    });
}

int ldit_clip_finish(const ldit_opt_state *state, ldit_clip_state *clip, const double *partials, int64_t n, ldit_stream stream)
{
    if (!state || !aligned4(state)) return fail(LDIT_EINVAL, "clip_finish: null or misaligned state block");
    if (!clip || !aligned4(clip)) return fail(LDIT_EINVAL, "clip_finish: null or misaligned clip block");
    if (n < 0) return fail(LDIT_EINVAL, "clip_finish: negative number of partials %lld", (long long)n);
    if (n > 0 && !partials) return fail(LDIT_EINVAL, "clip_finish: null partials buffer");
    if (reinterpret_cast<uintptr_t>(partials) & 7u) return fail(LDIT_EINVAL, "clip_finish: partials must be 8-byte aligned");
    LDIT_TRY(need_device());
    LAUNCH_CHECKED(clip_finish_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), state, clip, partials, n);
    return LDIT_OK;
}

int ldit_adamw_groups_multi_f32(const ldit_opt_segment *segs, const ldit_opt_hyper *hyper, int32_t S, const ldit_opt_state *state,
                                const ldit_clip_state *clip, double beta1, double beta2, float eps, ldit_stream stream_)
{
    LDIT_TRY(validate("adamw_groups_multi", segs, S, state, true));
    if (S > 0 && !hyper) return fail(LDIT_EINVAL, "adamw_groups_multi: null hyper-parameter array");
    for (int32_t s = 0; s < S; ++s)
        if (!(hyper[s].lr_scale >= 0.0f) || !(hyper[s].weight_decay >= 0.0f))
            return fail(LDIT_EINVAL, "adamw_groups_multi: segment %d: lr_scale and weight_decay must be >= 0", s);
    if (clip && !aligned4(clip)) return fail(LDIT_EINVAL, "adamw_groups_multi: clip block must be 4-byte aligned");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(LDIT_EINVAL, "adamw_groups_multi: betas must lie in [0, 1)");
    const float b1 = (float)beta1, omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    LDIT_TRY(need_device());
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return for_each_launch<GroupLaunch>(segs, S, [&](GroupLaunch &a, unsigned blocks, const int32_t *index) -> int {
        for (int k = 0; k < a.n; ++k) a.hyper[k] = hyper[index[k]];
        for (int k = a.n; k < GROUP_SEGS; ++k) a.hyper[k] = ldit_opt_hyper{0.0f, 0.0f};
        LAUNCH_CHECKED(adamw_groups_multi_kernel, dim3(blocks), dim3(256), 0, stream, a, state, clip, b1, omb1, b2, omb2, eps);
        return LDIT_OK;
    });
}

int ldit_adamw_ema_groups_multi_f32(const ldit_opt_segment *segs, const ldit_opt_hyper *hyper, void *const *ema, int32_t S,
                                    const ldit_opt_state *state, const ldit_clip_state *clip, double beta1, double beta2, float eps,
                                    double ema_decay, int32_t ema_warmup, ldit_stream stream_)
{
    const char *what = "adamw_ema_groups_multi";
    LDIT_TRY(validate(what, segs, S, state, true));
    if (S > 0 && !hyper) return fail(LDIT_EINVAL, "%s: null hyper-parameter array", what);
    for (int32_t s = 0; s < S; ++s) {
        if (!(hyper[s].lr_scale >= 0.0f) || !(hyper[s].weight_decay >= 0.0f))
            return fail(LDIT_EINVAL, "%s: segment %d: lr_scale and weight_decay must be >= 0", what, s);
        if (ema && segs[s].n > 0 && !aligned4(ema[s])) return fail(LDIT_EINVAL, "%s: segment %d: the shadow must be 4-byte aligned", what, s);
    }
    if (clip && !aligned4(clip)) return fail(LDIT_EINVAL, "%s: clip block must be 4-byte aligned", what);
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(LDIT_EINVAL, "%s: betas must lie in [0, 1)", what);
    if (!(ema_decay >= 0.0 && ema_decay < 1.0)) return fail(LDIT_EINVAL, "%s: ema_decay must lie in [0, 1)", what);
    const float b1 = (float)beta1, omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    LDIT_TRY(need_device());
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return for_each_launch<EmaLaunch>(segs, S, [&](EmaLaunch &a, unsigned blocks, const int32_t *index) -> int {
        for (int k = 0; k < EMA_SEGS; ++k) {
            a.hyper[k] = k < a.n ? hyper[index[k]] : ldit_opt_hyper{0.0f, 0.0f};
            a.ema[k] = k < a.n && ema ? static_cast<float *>(ema[index[k]]) : nullptr;
        }
        LAUNCH_CHECKED(adamw_ema_groups_multi_kernel, dim3(blocks), dim3(256), 0, stream, a, state, clip, b1, omb1, b2, omb2, eps, ema_decay,
                       (int)(ema_warmup != 0));
        return LDIT_OK;
    });
}

int ldit_swap_multi_f32(const ldit_swap_segment *segs, int32_t S, ldit_stream stream_)
{
    const char *what = "swap_multi";
    if (S < 0) return fail(LDIT_EINVAL, "%s: negative segment count %d", what, S);
    if (S > 0 && !segs) return fail(LDIT_EINVAL, "%s: null segment array", what);
    for (int32_t s = 0; s < S; ++s) {
        const ldit_swap_segment &q = segs[s];
        if (q.n < 0) return fail(LDIT_EINVAL, "%s: segment %d has negative length %lld", what, s, (long long)q.n);
        if (q.n == 0) continue;
        if (q.n > OPT_MAX_BLOCKS * (int64_t)OPT_BLOCK_ELEMS)
            return fail(LDIT_EUNSUPPORTED, "%s: segment %d longer than 2^41 elements: its grid exceeds 2^31 - 1 blocks", what, s);
        if (!q.a || !q.b) return fail(LDIT_EINVAL, "%s: segment %d has a null pointer", what, s);
        if (!aligned4(q.a) || !aligned4(q.b)) return fail(LDIT_EINVAL, "%s: segment %d: fp32 pointers must be 4-byte aligned", what, s);
        if (reinterpret_cast<uintptr_t>(q.bf16_mirror) & 1u) return fail(LDIT_EINVAL, "%s: segment %d: bf16 mirror must be 2-byte aligned", what, s);
    }
    LDIT_TRY(need_device());
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return for_each_launch<SwapLaunch>(segs, S, [&](const SwapLaunch &a, unsigned blocks, const int32_t *) -> int {
        LAUNCH_CHECKED(swap_multi_kernel, dim3(blocks), dim3(256), 0, stream, a);
        return LDIT_OK;
    });
}

}  // extern "C"
