// Training side of the region proposal network (torchvision RegionProposalNetwork.assign_targets_to_anchors + compute_loss, which
// the reference reaches through loss_dict = model(images, targets), ref training/trainer.py:164-183): anchor matching with
// low-quality promotion, the balanced sampler, BoxCoder.encode, and the two losses with their gradients.  torchvision does this
// with nonzero, randperm and data-dependent shapes; here it is three launches with fixed-size results: no host round trip, no
// allocation, no float atomics, capturable, output a pure function of the input (ldit.h, "RPN training").
//
//   rpn_targets   one workgroup per image.  The image's GT boxes sit in LDS.  Pass 1 finds every GT's best IoU over all anchors
//                 as an INTEGER max on the bits of a non-negative float (order-independent); pass 2 recomputes the same IoUs
//                 (bit-identical), takes each anchor's argmax, thresholds, and promotes the anchors that hold some GT's best.
//                 Then the bitonic sort of proposals.hip orders the anchors by (class, key, index) - class 0 positives, 1
//                 negatives, 2 everything else - so the sampler is "the first few of each class": unique, reproducible.
//   rpn_targets_chunked  the same for an image whose anchors do not fit the sort buffer: the sampler becomes a tournament that keeps
//                 the best batch_size keys of each class between sorts.  Same outputs, bit for bit, where both apply.
//   rpn_loss      one pass over the anchors (gradients written in full, per-block partial sums in a fixed order), one final
//                 single-workgroup pass over the partials.
//
// The IoU arithmetic decides labels, and the tests compare them exactly with a float32 oracle: contraction is off for this whole
// file and the division is the correctly rounded one (the Makefile pins -fhip-fp32-correctly-rounded-divide-sqrt), as for proposals.hip.
#include "det_train_common.h"
#include "sort_lds.h"

#pragma clang fp contract(off)

namespace ldit {
namespace {

constexpr int TGT_MAX_N = SORT_MAX_N;                    // anchors per image
constexpr int TGT_MAX_G = 512;                           // GT boxes per image: 8 KiB of boxes + 2 KiB of maxima in LDS
constexpr int TGT_LDS_EXTRA = 16;                        // two counters
constexpr int TGT_LDS_PER_GT = (int)(sizeof(f32x4) + sizeof(unsigned));   // a box and its maximum
constexpr int TGT_CHUNKED_MAX_N = 1 << 20;               // anchors per image of the chunked kernel: the index field of its key
constexpr int TGT_CHUNKED_MAX_BATCH = SORT_MAX_N / 4;    // its carry of 2 batch_size keys leaves half of the buffer to a chunk
constexpr int LOSS_PER_BLOCK = 1024;                     // anchors per block of the loss pass: four per thread

// pass 1 of both target kernels: every GT's best IoU over all anchors, an integer max on the bits of a non-negative float
__device__ __forceinline__ void gt_maxima(const f32x4 *__restrict__ anchors, int N, const f32x4 *gt, unsigned *gtmax, int G)
{
    for (int i = threadIdx.x; i < N; i += SORT_THREADS) {
        const f32x4 a = anchors[i];
        const float aarea = (a.z - a.x) * (a.w - a.y);
        for (int g = 0; g < G; ++g) {
            const f32x4 q = gt[g];
            const unsigned u = __float_as_uint(iou_pair(a, aarea, q, (q.z - q.x) * (q.w - q.y)));
            if (u > gtmax[g]) atomicMax(&gtmax[g], u);
        }
    }
}

// pass 2 of both target kernels, one anchor: argmax, thresholds, promotion, regression target.  Returns the sampler's class
// (0 positive, 1 negative, 2 neither), m = the value of `matched`, t = the row of `reg_targets`.
__device__ __forceinline__ int anchor_target(const f32x4 a, const f32x4 *gt, const unsigned *gtmax, int G, float fg_thr, float bg_thr,
                                             int &m, f32x4 &t)
{
    const float aarea = (a.z - a.x) * (a.w - a.y);
    float best = -1.f;
    int arg = -1;
    bool promoted = false;
    for (int g = 0; g < G; ++g) {
        const f32x4 q = gt[g];
        const float v = iou_pair(a, aarea, q, (q.z - q.x) * (q.w - q.y));
        if (v > best) {                                              // strict: ties go to the lowest GT index
            best = v;
            arg = g;
        }
        promoted |= __float_as_uint(v) == gtmax[g];
    }
    int cls;
    if (G == 0) {
        m = -1; cls = 1;
    } else if (best >= fg_thr || promoted) {
        m = arg; cls = 0;
    } else if (best < bg_thr) {
        m = -1; cls = 1;
    } else {
        m = -2; cls = 2;
    }
    t = f32x4{0.f, 0.f, 0.f, 0.f};
    if (m >= 0) {                                                    // BoxCoder(1, 1, 1, 1).encode_single
        const f32x4 q = gt[m];
        const float ew = a.z - a.x, eh = a.w - a.y, ecx = a.x + 0.5f * ew, ecy = a.y + 0.5f * eh;
        const float gw = q.z - q.x, gh = q.w - q.y, gcx = q.x + 0.5f * gw, gcy = q.y + 0.5f * gh;
        t = f32x4{(gcx - ecx) / ew, (gcy - ecy) / eh, logf(gw / ew), logf(gh / eh)};
    }
    return cls;
}

__global__ __launch_bounds__(SORT_THREADS) void rpn_targets_kernel(const f32x4 *__restrict__ anchors, const f32x4 *__restrict__ gt_boxes,
                                                                   const int *__restrict__ gt_count, const int *__restrict__ keys_in,
                                                                   int N, int Gmax, float fg_thr, float bg_thr, int batch_size, int quota_pos,
                                                                   int *__restrict__ labels, int *__restrict__ matched,
                                                                   f32x4 *__restrict__ reg_targets, int *__restrict__ sampled)
{
    // all LDS is dynamic: n2 sort keys, Gmax boxes, Gmax maxima, two counters
    extern __shared__ __align__(16) unsigned char smem[];
    const int n2 = pow2_at_least(N);
    u64 *keys = reinterpret_cast<u64 *>(smem);
    f32x4 *gt = reinterpret_cast<f32x4 *>(smem + (size_t)n2 * sizeof(u64));
    unsigned *gtmax = reinterpret_cast<unsigned *>(smem + (size_t)n2 * sizeof(u64) + (size_t)Gmax * sizeof(f32x4));
    int *cnt = reinterpret_cast<int *>(gtmax + Gmax);                // [0] positives, [1] negatives
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    int G = gt_count[b];
    G = G < 0 ? 0 : (G > Gmax ? Gmax : G);
    gt_boxes += b * Gmax;
    keys_in += b * N; labels += b * N; matched += b * N; reg_targets += b * N;

    for (int g = tid; g < G; g += SORT_THREADS) {
        gt[g] = gt_boxes[g];
        gtmax[g] = 0u;
    }
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();

    // ---- pass 1: every GT's best IoU over all anchors ----
    gt_maxima(anchors, N, gt, gtmax, G);
    __syncthreads();

    // ---- pass 2: argmax, thresholds, promotion, regression targets, sort keys ----
    int npos = 0, nneg = 0;
    for (int i = tid; i < n2; i += SORT_THREADS) {
        if (i >= N) {
            keys[i] = ~0ull;
            continue;
        }
        f32x4 t;
        int m;
        const int cls = anchor_target(anchors[i], gt, gtmax, G, fg_thr, bg_thr, m, t);
        matched[i] = m;
        reg_targets[i] = t;
        npos += cls == 0;
        nneg += cls == 1;
        keys[i] = ((u64)cls << 48) | ((u64)((unsigned)keys_in[i] & 0x7fffffffu) << 16) | (u64)(unsigned)i;
    }
    if (npos) atomicAdd(&cnt[0], npos);                              // integer: order-independent
    if (nneg) atomicAdd(&cnt[1], nneg);
    bitonic_sort(keys, n2);                                          // starts and ends with a barrier

    // ---- the sampler: positives are sorted positions [0, P), negatives [P, P + Q) ----
    const int P = cnt[0], Q = cnt[1];
    const int take_pos = quota_pos < P ? quota_pos : P;
    const int room = batch_size - take_pos;
    const int take_neg = room < Q ? room : Q;
    for (int j = tid; j < N; j += SORT_THREADS) {                    // the N real anchors sort in front of the padding keys
        const int i = (int)(unsigned)(keys[j] & 0xffffu);
        int lab = -1;
        if (j < take_pos) lab = 1;
        else if (j >= P && j < P + take_neg) lab = 0;
        if (i < N) labels[i] = lab;
    }
    if (tid == 0) {
        sampled[2 * b] = take_pos;
        sampled[2 * b + 1] = take_neg;
    }
}

// rpn_targets_kernel for up to TGT_CHUNKED_MAX_N anchors per image.  Both passes stream over the anchors as above; the sampler is a
// tournament in a buffer of S = SORT_MAX_N keys (class : key : index, the index in 20 bits - the order of rpn_targets_kernel).
// Anchors enter S - 2 batch_size at a time behind a carry; keys of class 2 never enter.  After a sort the buffer holds its pb
// positives in [0, pb) and its qb negatives in [pb, pb + qb); the carry kept is the first min(batch_size, .) of each, and that is
// min(batch_size, seen so far) of the best of each class seen so far, which is all the sampler can ever take.  N, batch_size and
// hence the trip count are kernel arguments: workgroup-uniform, as the barriers of bitonic_sort require.
__global__ __launch_bounds__(SORT_THREADS) void rpn_targets_chunked_kernel(const f32x4 *__restrict__ anchors, const f32x4 *__restrict__ gt_boxes,
                                                                           const int *__restrict__ gt_count, const int *__restrict__ keys_in,
                                                                           int N, int Gmax, float fg_thr, float bg_thr, int batch_size,
                                                                           int quota_pos, int *__restrict__ labels, int *__restrict__ matched,
                                                                           f32x4 *__restrict__ reg_targets, int *__restrict__ sampled)
{
    // all LDS is dynamic: S sort keys, Gmax boxes, Gmax maxima, two counters
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int S = SORT_MAX_N;
    constexpr int CARRY_SLOTS = TGT_CHUNKED_MAX_BATCH / SORT_THREADS;   // carried negatives a thread moves
    u64 *keys = reinterpret_cast<u64 *>(smem);
    f32x4 *gt = reinterpret_cast<f32x4 *>(smem + (size_t)S * sizeof(u64));
    unsigned *gtmax = reinterpret_cast<unsigned *>(smem + (size_t)S * sizeof(u64) + (size_t)Gmax * sizeof(f32x4));
    int *cnt = reinterpret_cast<int *>(gtmax + Gmax);                // [0] positives, [1] negatives: of the whole image so far
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    int G = gt_count[b];
    G = G < 0 ? 0 : (G > Gmax ? Gmax : G);
    gt_boxes += b * Gmax;
    keys_in += b * N; labels += b * N; matched += b * N; reg_targets += b * N;

    for (int g = tid; g < G; g += SORT_THREADS) {
        gt[g] = gt_boxes[g];
        gtmax[g] = 0u;
    }
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();

    // ---- pass 1: every GT's best IoU over all anchors ----
    gt_maxima(anchors, N, gt, gtmax, G);
    __syncthreads();

    // ---- pass 2 and the tournament, a chunk at a time ----
    const int step = S - 2 * batch_size;                             // >= S / 2: batch_size <= TGT_CHUNKED_MAX_BATCH (host)
    int cp = 0, cn = 0;                                              // the carry: positives in [0, cp), negatives in [cp, cp + cn)
    int seen_p = 0, seen_q = 0;                                      // the counters before this chunk
    int pb = 0, P = 0, Q = 0;
    for (int pos = 0; pos < N; pos += step) {
        const int c = cp + cn;
        int npos = 0, nneg = 0;
        for (int j = tid; j < S - c; j += SORT_THREADS) {            // slots [c, c + step) take anchors, the rest padding
            const int i = pos + j;
            u64 key = ~0ull;
            if (j < step && i < N) {
                f32x4 t;
                int m;
                const int cls = anchor_target(anchors[i], gt, gtmax, G, fg_thr, bg_thr, m, t);
                matched[i] = m;
                reg_targets[i] = t;
                labels[i] = -1;                                      // the sampled ones are overwritten after the last sort
                npos += cls == 0;
                nneg += cls == 1;
                if (cls < 2) key = ((u64)cls << 51) | ((u64)((unsigned)keys_in[i] & 0x7fffffffu) << 20) | (u64)(unsigned)i;
            }
            keys[c + j] = key;
        }
        if (npos) atomicAdd(&cnt[0], npos);                          // integer: order-independent
        if (nneg) atomicAdd(&cnt[1], nneg);
        bitonic_sort(keys, S);                                       // starts and ends with a barrier
        P = cnt[0]; Q = cnt[1];
        pb = cp + (P - seen_p);                                      // positives in the buffer
        if (pos + step >= N) break;                                  // the last chunk (uniform)
        const int qb = cn + (Q - seen_q);
        cp = pb < batch_size ? pb : batch_size;
        cn = qb < batch_size ? qb : batch_size;
        seen_p = P; seen_q = Q;
        // compact the kept negatives [pb, pb + cn) to [cp, cp + cn): the regions can overlap, so read, barrier, write.  The
        // barrier also keeps the next chunk's atomicAdd behind every thread's read of the counters.
        u64 v[CARRY_SLOTS];
#pragma unroll
        for (int r = 0; r < CARRY_SLOTS; ++r) {
            const int j = tid + r * SORT_THREADS;
            v[r] = j < cn ? keys[pb + j] : ~0ull;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < CARRY_SLOTS; ++r) {
            const int j = tid + r * SORT_THREADS;
            if (j < cn) keys[cp + j] = v[r];
        }
    }

    // ---- the sampler: the buffer's positives are sorted positions [0, pb), its negatives start at pb ----
    const int take_pos = quota_pos < P ? quota_pos : P;              // <= min(batch_size, P) <= pb
    const int room = batch_size - take_pos;
    const int take_neg = room < Q ? room : Q;                        // <= min(batch_size, Q) <= the buffer's negatives
    // These stores hit addresses that OTHER threads wrote with -1 in pass 2: a barrier must separate the two (the last sort ends
    // with one; this one says so and stays if the code above it moves).
    __syncthreads();
    for (int j = tid; j < take_pos; j += SORT_THREADS) labels[(int)(unsigned)(keys[j] & 0xfffffu)] = 1;
    for (int j = tid; j < take_neg; j += SORT_THREADS) labels[(int)(unsigned)(keys[pb + j] & 0xfffffu)] = 0;
    if (tid == 0) {
        sampled[2 * b] = take_pos;
        sampled[2 * b + 1] = take_neg;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void rpn_loss_kernel(const float *__restrict__ logits, const f32x4 *__restrict__ deltas,
                                                                const int *__restrict__ labels, const f32x4 *__restrict__ reg_targets,
                                                                const int *__restrict__ sampled, int B, int N, float beta,
                                                                float *__restrict__ d_logits, f32x4 *__restrict__ d_deltas,
                                                                float *__restrict__ partial)
{
    __shared__ float red[LOSS_THREADS / 64];
    __shared__ int total_slot;
    const int total = sampled_total(sampled, B, &total_slot);
    const float inv = total > 0 ? 1.0f / (float)total : 0.f;
    const size_t b = blockIdx.y;
    const int first = blockIdx.x * LOSS_PER_BLOCK;
    float cls_sum = 0.f, box_sum = 0.f;
    for (int r = 0; r < LOSS_PER_BLOCK / LOSS_THREADS; ++r) {
        const int i = first + r * LOSS_THREADS + threadIdx.x;
        if (i >= N) break;
        const size_t e = b * N + i;
        const int lab = labels[e];
        float dl = 0.f;
        f32x4 dd = f32x4{0.f, 0.f, 0.f, 0.f};
        if (lab == 0 || lab == 1) {
            const float x = logits[e], y = (float)lab;
            const float en = expf(-fabsf(x));                        // in (0, 1]
            cls_sum += (fmaxf(x, 0.f) - x * y) + log1pf(en);
            const float sig = x >= 0.f ? 1.0f / (1.0f + en) : en / (1.0f + en);
            dl = (sig - y) * inv;
        }
        if (lab == 1) {
            const f32x4 p = deltas[e], t = reg_targets[e];
            float g[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = p[c] - t[c], ad = fabsf(d);
                if (ad < beta) {
                    box_sum += 0.5f * d * d / beta;
                    g[c] = d / beta;
                } else {
                    box_sum += ad - 0.5f * beta;
                    g[c] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                }
            }
            dd = f32x4{g[0] * inv, g[1] * inv, g[2] * inv, g[3] * inv};
        }
        d_logits[e] = dl;
        d_deltas[e] = dd;
    }
    const float cs = block_sum(cls_sum, red);
    const float bs = block_sum(box_sum, red);
    if (threadIdx.x == 0) {
        const size_t slot = b * gridDim.x + blockIdx.x;
        partial[2 * slot] = cs;
        partial[2 * slot + 1] = bs;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void rpn_loss_final_kernel(const float *__restrict__ partial, int n_partial,
                                                                      const int *__restrict__ sampled, int B, float *__restrict__ loss)
{
    __shared__ double red[2][LOSS_THREADS];
    __shared__ int total_slot;
    const int total = sampled_total(sampled, B, &total_slot);
    loss_final(partial, n_partial, total, loss, red);
}

// argument checks of both target entry points; messages begin with `who`, max_n is the entry point's limit on N
int targets_check(const char *who, const void *anchors, const void *gt_boxes, const void *gt_count, const void *keys, int B, int64_t N,
                  int Gmax, float fg_thr, float bg_thr, int batch_size, float positive_fraction, const void *labels, const void *matched,
                  const void *reg_targets, const void *sampled, int max_n)
{
    if (!anchors || !gt_boxes || !gt_count || !keys || !labels || !matched || !reg_targets || !sampled)
        return fail(LDIT_EINVAL, "%s: null argument", who);
    if (!aligned16(anchors) || !aligned16(gt_boxes) || !aligned16(gt_count) || !aligned16(keys) || !aligned16(labels) || !aligned16(matched) ||
        !aligned16(reg_targets) || !aligned16(sampled))
        return fail(LDIT_EINVAL, "%s: operands must be 16-byte aligned", who);
    if (B <= 0 || B > 65535 || N <= 0 || Gmax <= 0) return fail(LDIT_EINVAL, "%s: bad geometry (B=%d N=%lld Gmax=%d)", who, B, (long long)N, Gmax);
    if (!(fg_thr >= bg_thr)) return fail(LDIT_EINVAL, "%s: thresholds fg=%g bg=%g (bg must not exceed fg)", who, fg_thr, bg_thr);
    if (batch_size <= 0) return fail(LDIT_EINVAL, "%s: batch_size_per_image=%d", who, batch_size);
    if (!(positive_fraction > 0.f && positive_fraction <= 1.f))
        return fail(LDIT_EINVAL, "%s: positive_fraction=%g is outside (0, 1]", who, positive_fraction);
    if (N > max_n) return fail(LDIT_EUNSUPPORTED, "%s: %lld anchors per image, at most %d are handled", who, (long long)N, max_n);
    if (Gmax > TGT_MAX_G) return fail(LDIT_EUNSUPPORTED, "%s: %d GT boxes per image, at most %d are handled", who, Gmax, TGT_MAX_G);
    return LDIT_OK;
}

inline int loss_blocks(int64_t N) { return (int)((N + LOSS_PER_BLOCK - 1) / LOSS_PER_BLOCK); }

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_rpn_targets_f32(const void *anchors, const void *gt_boxes, const void *gt_count, const void *keys, int32_t B, int64_t N,
                         int32_t Gmax, float fg_thr, float bg_thr, int32_t batch_size_per_image, float positive_fraction, void *labels,
                         void *matched, void *reg_targets, void *sampled, ldit_stream stream)
{
    if (int rc = targets_check("rpn_targets", anchors, gt_boxes, gt_count, keys, B, N, Gmax, fg_thr, bg_thr, batch_size_per_image,
                               positive_fraction, labels, matched, reg_targets, sampled, TGT_MAX_N))
        return rc;
    const int quota = (int)((double)batch_size_per_image * (double)positive_fraction);
    int n2 = 2;
    while (n2 < N) n2 <<= 1;
    const int lds = n2 * (int)sizeof(u64) + Gmax * TGT_LDS_PER_GT + TGT_LDS_EXTRA;
    LDIT_DYN_LDS(rpn_targets_kernel, TGT_MAX_N * (int)sizeof(u64) + TGT_MAX_G * TGT_LDS_PER_GT + TGT_LDS_EXTRA);
    hipLaunchKernelGGL(rpn_targets_kernel, dim3((unsigned)B), dim3(SORT_THREADS), lds, static_cast<hipStream_t>(stream),
                       static_cast<const f32x4 *>(anchors), static_cast<const f32x4 *>(gt_boxes), static_cast<const int *>(gt_count),
                       static_cast<const int *>(keys), (int)N, (int)Gmax, fg_thr, bg_thr, (int)batch_size_per_image, quota,
                       static_cast<int *>(labels), static_cast<int *>(matched), static_cast<f32x4 *>(reg_targets), static_cast<int *>(sampled));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int ldit_rpn_targets_chunked_f32(const void *anchors, const void *gt_boxes, const void *gt_count, const void *keys, int32_t B, int64_t N,
                                 int32_t Gmax, float fg_thr, float bg_thr, int32_t batch_size_per_image, float positive_fraction,
                                 void *labels, void *matched, void *reg_targets, void *sampled, ldit_stream stream)
{
    if (int rc = targets_check("rpn_targets_chunked", anchors, gt_boxes, gt_count, keys, B, N, Gmax, fg_thr, bg_thr, batch_size_per_image,
                               positive_fraction, labels, matched, reg_targets, sampled, TGT_CHUNKED_MAX_N))
        return rc;
    if (batch_size_per_image > TGT_CHUNKED_MAX_BATCH)
        return fail(LDIT_EUNSUPPORTED, "rpn_targets_chunked: batch_size_per_image=%d, at most %d are handled", batch_size_per_image,
                    TGT_CHUNKED_MAX_BATCH);
    const int quota = (int)((double)batch_size_per_image * (double)positive_fraction);
    const int lds = SORT_MAX_N * (int)sizeof(u64) + Gmax * TGT_LDS_PER_GT + TGT_LDS_EXTRA;
    LDIT_DYN_LDS(rpn_targets_chunked_kernel, SORT_MAX_N * (int)sizeof(u64) + TGT_MAX_G * TGT_LDS_PER_GT + TGT_LDS_EXTRA);
    hipLaunchKernelGGL(rpn_targets_chunked_kernel, dim3((unsigned)B), dim3(SORT_THREADS), lds, static_cast<hipStream_t>(stream),
                       static_cast<const f32x4 *>(anchors), static_cast<const f32x4 *>(gt_boxes), static_cast<const int *>(gt_count),
                       static_cast<const int *>(keys), (int)N, (int)Gmax, fg_thr, bg_thr, (int)batch_size_per_image, quota,
                       static_cast<int *>(labels), static_cast<int *>(matched), static_cast<f32x4 *>(reg_targets), static_cast<int *>(sampled));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

/* one pair of partial sums per block of the first pass */
size_t ldit_rpn_loss_workspace_bytes(int64_t B, int64_t N)
{
    if (B <= 0 || N <= 0) return 0;
    const size_t bytes = (size_t)B * (size_t)loss_blocks(N) * 2 * sizeof(float);
    return (bytes + 15) & ~(size_t)15;
}

int ldit_rpn_loss_f32(const void *logits, const void *deltas, const void *labels, const void *reg_targets, const void *sampled, int32_t B,
                      int64_t N, float beta, void *loss, void *d_logits, void *d_deltas, void *workspace, size_t workspace_bytes,
                      ldit_stream stream)
{
    if (!logits || !deltas || !labels || !reg_targets || !sampled || !loss || !d_logits || !d_deltas)
        return fail(LDIT_EINVAL, "rpn_loss: null argument");
    if (!aligned16(logits) || !aligned16(deltas) || !aligned16(labels) || !aligned16(reg_targets) || !aligned16(sampled) || !aligned16(loss) ||
        !aligned16(d_logits) || !aligned16(d_deltas) || !aligned16(workspace))
        return fail(LDIT_EINVAL, "rpn_loss: operands must be 16-byte aligned");
    if (B <= 0 || B > 65535 || N <= 0) return fail(LDIT_EINVAL, "rpn_loss: bad geometry (B=%d N=%lld)", B, (long long)N);
    if (!(beta >= 0.f) || beta == __builtin_inff()) return fail(LDIT_EINVAL, "rpn_loss: beta=%g", beta);
    if ((int64_t)B * N >= (1ll << 29)) return fail(LDIT_EUNSUPPORTED, "rpn_loss: operand exceeds 2^31 elements");
    const size_t need = ldit_rpn_loss_workspace_bytes(B, N);
    if (!workspace || workspace_bytes < need) return fail(LDIT_EWORKSPACE, "rpn_loss: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int blocks = loss_blocks(N);
    hipLaunchKernelGGL(rpn_loss_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(LOSS_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(logits), static_cast<const f32x4 *>(deltas), static_cast<const int *>(labels),
                       static_cast<const f32x4 *>(reg_targets), static_cast<const int *>(sampled), (int)B, (int)N, beta,
                       static_cast<float *>(d_logits), static_cast<f32x4 *>(d_deltas), static_cast<float *>(workspace));
    LDIT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(rpn_loss_final_kernel, dim3(1), dim3(LOSS_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(workspace), blocks * (int)B, static_cast<const int *>(sampled), (int)B, static_cast<float *>(loss));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // extern "C"
