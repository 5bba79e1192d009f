// Region-proposal stage of the detector (torchvision RegionProposalNetwork.filter_proposals in eval mode, which the reference
// reaches through FasterRCNN(..., rpn_anchor_generator=...), ref src/layoutdit/modeling/model.py:40-55): per-level top-k on the
// objectness logits, box decoding + clipping + the small-box / score filter, batched NMS with a fixed-size padded result.
// Three kernels, three launches, no host round trip, no allocation, no data-dependent shape: the stage can sit in a hipGraph.
//
//   rpn_topk     one workgroup per (level, image): a bitonic sort of 8-byte keys (~rank(logit) : index) in LDS.  The key is a
//                total order - descending logit, ascending index, -inf last, NaN after -inf - so the result is unique.
//   rpn_topk_chunked  the same result for a level that does not fit the 16 384 keys of LDS: a tournament in the same buffer.
//                After a sort the level's best k keys so far sit in slots [0, k); the next 16 384 - k anchors are written behind
//                them and the buffer is sorted again.  The best k of a set under a total order do not depend on the chunking.
//   rpn_decode   one thread per selected candidate.
//   nms_batched  one workgroup per problem.  The candidates are sorted like above (invalid ones - score -inf / NaN - behind all
//                others), then every thread takes the candidates at sorted positions tid, tid + 1024, ... into REGISTERS.  Sorted
//                block b (64 positions) therefore lives in the lanes of wave b % 16, slot b / 16: that wave resolves the block
//                on its own (lane j holds box j; each still-alive box i in turn is broadcast by v_readlane and kills later
//                lanes - no barrier), writes the block's survivors to a small LDS buffer and to the output, and after ONE
//                barrier the whole workgroup applies those survivors to every later candidate.  Buffers alternate, so the next
//                block's wave may already write while slower waves still read.  The walk stops at max_out survivors.
//                No atomics anywhere: the result is a pure function of the inputs.
//
// The IoU arithmetic decides what is kept, and the tests compare decisions exactly with a float32 oracle: contraction is off
// for this whole file (areaB - iw * ih must not become an FMA) and the division is the correctly rounded one (the Makefile
// pins -fhip-fp32-correctly-rounded-divide-sqrt for this object).
#include "ldit_common.h"
#include "sort_lds.h"

#pragma clang fp contract(off)

namespace ldit {
namespace {

constexpr int PROP_THREADS = SORT_THREADS;                // 16 waves
constexpr int TOPK_MAX_N = 16384;                        // 128 KiB of keys
constexpr int TOPK_MAX_LEVELS = 8;
constexpr int TOPK_CHUNKED_MAX_N = 1 << 20;              // anchors per level of the chunked kernel
constexpr int TOPK_CHUNKED_MAX_K = SORT_MAX_N / 2;       // the carry leaves at least half of the buffer to every chunk
constexpr int NMS_MAX_N = 8192;                          // 8 candidates per thread
constexpr int NMS_SLOTS = NMS_MAX_N / PROP_THREADS;
constexpr unsigned INVALID_HI = 0xFF800000u;             // high key word of score -inf; everything at or above is not a candidate

// order-preserving bits of a score, ascending; -0 = +0; NaN below everything (-inf included)
__device__ __forceinline__ unsigned score_rank(float s)
{
    unsigned u = __float_as_uint(s);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ascending key order = descending score, ties by ascending index
__device__ __forceinline__ u64 sort_key(float s, int idx) { return ((u64)(~score_rank(s)) << 32) | (unsigned)idx; }

struct TopkLevels {
    int n_levels;
    int off[TOPK_MAX_LEVELS];    // first anchor of the level on the concatenated axis
    int n[TOPK_MAX_LEVELS];      // anchors of the level
    int kofs[TOPK_MAX_LEVELS];   // first output column of the level
    int k[TOPK_MAX_LEVELS];      // min(k, n)
};

__global__ __launch_bounds__(PROP_THREADS) void rpn_topk_kernel(const float *__restrict__ logits, int *__restrict__ idx_out,
                                                                 TopkLevels lv, int Ntot, int Ksum)
{
    extern __shared__ __align__(16) unsigned char smem[];
    u64 *keys = reinterpret_cast<u64 *>(smem);
    const int l = blockIdx.x, b = blockIdx.y;
    const int n = lv.n[l], off = lv.off[l], k = lv.k[l], kofs = lv.kofs[l];
    const int n2 = pow2_at_least(n);
    const float *src = logits + (size_t)b * Ntot + off;
    for (int i = threadIdx.x; i < n2; i += PROP_THREADS) keys[i] = i < n ? sort_key(src[i], i) : ~0ull;
    bitonic_sort(keys, n2);
    int *dst = idx_out + (size_t)b * Ksum + kofs;
    for (int j = threadIdx.x; j < k; j += PROP_THREADS) dst[j] = off + (int)(unsigned)(keys[j] & 0xffffffffu);
}

// Levels of up to TOPK_CHUNKED_MAX_N anchors in the buffer of rpn_topk_kernel.  A level that fits is one sort of the same keys: the
// bits of rpn_topk_kernel.  A larger one (then k <= TOPK_CHUNKED_MAX_K < S, checked on the host) keeps its best k keys in slots
// [0, k) and refills slots [k, S).  n, k and S depend on blockIdx alone, so the trip count is workgroup-uniform (bitonic_sort
// holds barriers).  Every refilled slot was last read before the barrier that ends the sort.
__global__ __launch_bounds__(PROP_THREADS) void rpn_topk_chunked_kernel(const float *__restrict__ logits, int *__restrict__ idx_out,
                                                                         TopkLevels lv, int Ntot, int Ksum)
{
    extern __shared__ __align__(16) unsigned char smem[];
    u64 *keys = reinterpret_cast<u64 *>(smem);
    const int l = blockIdx.x, b = blockIdx.y;
    const int n = lv.n[l], off = lv.off[l], k = lv.k[l], kofs = lv.kofs[l];
    const int S = n < SORT_MAX_N ? pow2_at_least(n) : SORT_MAX_N;
    const float *src = logits + (size_t)b * Ntot + off;
    int kept = 0;                                         // slots in front that hold the best keys so far
    for (int pos = 0; pos < n; pos += S - kept, kept = k) {
        const int room = S - kept;
        for (int j = threadIdx.x; j < room; j += PROP_THREADS) {
            const int i = pos + j;
            keys[kept + j] = i < n ? sort_key(src[i], i) : ~0ull;
        }
        bitonic_sort(keys, S);
    }
    int *dst = idx_out + (size_t)b * Ksum + kofs;
    for (int j = threadIdx.x; j < k; j += PROP_THREADS) dst[j] = off + (int)(unsigned)(keys[j] & 0xffffffffu);
}

// torchvision BoxCoder.decode_single at weights (1, 1, 1, 1), clip_boxes_to_image, remove_small_boxes, score threshold
__global__ __launch_bounds__(256) void rpn_decode_kernel(const float *__restrict__ logits, const f32x4 *__restrict__ deltas,
                                                          const f32x4 *__restrict__ anchors, const int *__restrict__ idx,
                                                          f32x4 *__restrict__ boxes_out, float *__restrict__ scores_out, int total,
                                                          int Ntot, int Ksum, float img_h, float img_w, float min_size,
                                                          float score_thresh)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = i / Ksum;
    const int a = idx[i];
    if ((unsigned)a >= (unsigned)Ntot) {                  // not an anchor: never a candidate
        boxes_out[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        scores_out[i] = -__builtin_inff();
        return;
    }
    const f32x4 an = anchors[a];
    const f32x4 d = deltas[(size_t)b * Ntot + a];
    const float lg = logits[(size_t)b * Ntot + a];
    const float clip = 4.135166556742356f;                // log(1000 / 16)
    const float w = an.z - an.x, h = an.w - an.y;
    const float cx = an.x + 0.5f * w, cy = an.y + 0.5f * h;
    const float dw = fminf(d.z, clip), dh = fminf(d.w, clip);
    const float pcx = d.x * w + cx, pcy = d.y * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    float x1 = pcx - 0.5f * pw, y1 = pcy - 0.5f * ph, x2 = pcx + 0.5f * pw, y2 = pcy + 0.5f * ph;
    x1 = fminf(fmaxf(x1, 0.f), img_w); x2 = fminf(fmaxf(x2, 0.f), img_w);
    y1 = fminf(fmaxf(y1, 0.f), img_h); y2 = fminf(fmaxf(y2, 0.f), img_h);
    float score = 1.0f / (1.0f + expf(-lg));
    if (!(x2 - x1 >= min_size) || !(y2 - y1 >= min_size) || !(score >= score_thresh)) score = -__builtin_inff();
    boxes_out[i] = f32x4{x1, y1, x2, y2};
    scores_out[i] = score;
}

// does the kept box a suppress candidate b?  fp32, in exactly this order (ldit.h)
__device__ __forceinline__ bool iou_exceeds(float ax1, float ay1, float ax2, float ay2, float aarea, float bx1, float by1, float bx2,
                                            float by2, float barea, float thr, bool skip_disjoint)
{
    const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
    const float ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
    const float inter = iw * ih;
    // inter == 0 (or NaN): the quotient is 0, -0 or NaN, none of which exceeds a threshold >= 0 - no division needed
    if (skip_disjoint && !(inter > 0.f)) return false;
    const float uni = (aarea + barea) - inter;
    return inter / uni > thr;
}

struct Survivor {
    float x1, y1, x2, y2, area;
    int grp;
};
constexpr int NMS_LDS_EXTRA = 4096;
static_assert(2 * 64 * sizeof(Survivor) + 5 * sizeof(int) <= NMS_LDS_EXTRA, "survivor buffers outgrew their LDS region");

__device__ __forceinline__ float lane_bcast(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ __launch_bounds__(PROP_THREADS) void nms_batched_kernel(const f32x4 *__restrict__ boxes, const float *__restrict__ scores,
                                                                    const int *__restrict__ groups, int N, float thr, int max_out,
                                                                    int *__restrict__ keep, int *__restrict__ count,
                                                                    f32x4 *__restrict__ out_boxes, float *__restrict__ out_scores)
{
    // all LDS is dynamic (one limit to raise): n2 keys, then the two survivor buffers and a few counters (NMS_LDS_EXTRA bytes)
    extern __shared__ __align__(16) unsigned char smem[];
    const int n2 = pow2_at_least(N);
    u64 *keys = reinterpret_cast<u64 *>(smem);
    Survivor(*surv)[64] = reinterpret_cast<Survivor(*)[64]>(smem + (size_t)n2 * sizeof(u64));
    int *surv_n = reinterpret_cast<int *>(smem + (size_t)n2 * sizeof(u64) + 2 * 64 * sizeof(Survivor));
    int *surv_total = surv_n + 2;
    int &n_valid = surv_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t p = blockIdx.x;
    boxes += p * N; scores += p * N;
    if (groups) groups += p * N;
    keep += p * max_out;
    if (out_boxes) out_boxes += p * max_out;
    if (out_scores) out_scores += p * max_out;

    // ---- order the candidates: valid ones first, by descending score then ascending index ----
    if (tid == 0) n_valid = 0;
    for (int i = tid; i < n2; i += PROP_THREADS) keys[i] = i < N ? sort_key(scores[i], i) : ~0ull;
    bitonic_sort(keys, n2);
    for (int i = tid; i < n2; i += PROP_THREADS) {
        const bool v = (unsigned)(keys[i] >> 32) < INVALID_HI;
        const bool vnext = i + 1 < n2 && (unsigned)(keys[i + 1] >> 32) < INVALID_HI;
        if (v && !vnext) n_valid = i + 1;                 // exactly one thread, or none when nothing is valid
    }
    __syncthreads();
    const int M = n_valid, nb = (M + 63) >> 6;

    // ---- sorted position tid + 1024 r -> slot r of this thread (the area is recomputed where needed: same bits, fewer registers) ----
    float x1[NMS_SLOTS], y1[NMS_SLOTS], x2[NMS_SLOTS], y2[NMS_SLOTS];
    int gr[NMS_SLOTS];
    unsigned alive = 0;
#pragma unroll
    for (int r = 0; r < NMS_SLOTS; ++r) {
        // branch-free: a slot past the valid candidates loads a clamped (in-bounds) row and simply never becomes alive
        const int pos = tid + PROP_THREADS * r;
        const unsigned raw = (unsigned)(keys[pos < n2 ? pos : n2 - 1] & 0xffffffffu);
        const int id = (int)(raw < (unsigned)N ? raw : (unsigned)N - 1u);
        const f32x4 v = boxes[id];
        x1[r] = v.x; y1[r] = v.y; x2[r] = v.z; y2[r] = v.w;
        gr[r] = groups ? groups[id] : 0;
        alive |= (pos < M ? 1u : 0u) << r;
    }

    const bool skip_disjoint = thr >= 0.f;
    int total = 0;
    for (int b = 0; b < nb && total < max_out; ++b) {                  // sorted block b = positions 64 b .. 64 b + 63
        const int buf = b & 1, w = b & 15, r = b >> 4;
        if (wave == w) {
            // resolve the block inside this wave: lane j holds position 64 b + j in its slot r
            float mx1 = x1[0], my1 = y1[0], mx2 = x2[0], my2 = y2[0];
            int mg = gr[0];
#pragma unroll
            for (int q = 1; q < NMS_SLOTS; ++q)
                if (r == q) {
                    mx1 = x1[q]; my1 = y1[q]; mx2 = x2[q]; my2 = y2[q]; mg = gr[q];
                }
            const float mar = (mx2 - mx1) * (my2 - my1);
            bool a = (alive >> r) & 1u;
#pragma unroll 1
            for (int i = 0; i < 63; ++i) {
                const u64 m = __ballot(a);
                if (!((m >> i) & 1ull)) continue;                      // box i is gone (wave-uniform)
                const float kx1 = lane_bcast(mx1, i), ky1 = lane_bcast(my1, i), kx2 = lane_bcast(mx2, i), ky2 = lane_bcast(my2, i),
                            kar = lane_bcast(mar, i);
                const int kg = __builtin_amdgcn_readlane(mg, i);
                if (a && lane > i && mg == kg && iou_exceeds(kx1, ky1, kx2, ky2, kar, mx1, my1, mx2, my2, mar, thr, skip_disjoint))
                    a = false;
            }
            const u64 m = __ballot(a);
            const int slot = __popcll(m & ((1ull << lane) - 1ull));
            if (a) {
                surv[buf][slot] = Survivor{mx1, my1, mx2, my2, mar, mg};
                const int o = total + slot;
                if (o < max_out) {
                    const int id = (int)(unsigned)(keys[64 * b + lane] & 0xffffffffu);
                    keep[o] = id;
                    if (out_boxes) out_boxes[o] = f32x4{mx1, my1, mx2, my2};
                    if (out_scores) out_scores[o] = scores[id];
                }
            }
            if (lane == 0) {
                surv_n[buf] = __popcll(m);
                surv_total[buf] = total + __popcll(m);
            }
            alive = a ? (alive | (1u << r)) : (alive & ~(1u << r));
        }
        __syncthreads();
        const int cnt = surv_n[buf];
        total = surv_total[buf];
        if (total >= max_out || b + 1 >= nb) break;                    // nothing later will be emitted (uniform)
        // the block's survivors against every later candidate of this thread
        const int first_later = 64 * (b + 1);
        unsigned later = 0;
#pragma unroll
        for (int q = 0; q < NMS_SLOTS; ++q) later |= (tid + PROP_THREADS * q >= first_later ? 1u : 0u) << q;
        unsigned cand = alive & later;
#pragma unroll 1
        for (int s = 0; s < cnt && cand; ++s) {
            const Survivor k = surv[buf][s];
#pragma unroll
            for (int q = 0; q < NMS_SLOTS; ++q)
                if (((cand >> q) & 1u) && gr[q] == k.grp &&
                    iou_exceeds(k.x1, k.y1, k.x2, k.y2, k.area, x1[q], y1[q], x2[q], y2[q], (x2[q] - x1[q]) * (y2[q] - y1[q]), thr, skip_disjoint))
                    cand &= ~(1u << q);
        }
        alive = (alive & ~later) | cand;
    }

    const int kept = total < max_out ? total : max_out;
    for (int j = kept + tid; j < max_out; j += PROP_THREADS) {
        keep[j] = -1;
        if (out_boxes) out_boxes[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (out_scores) out_scores[j] = 0.f;
    }
    if (tid == 0) count[p] = kept;
}

// host side of both top-k entry points: argument checks (messages begin with `who`), the level table, the totals and the LDS bytes
// of the largest level (at most the whole sort buffer)
int topk_levels(const char *who, const void *logits, const int64_t *level_sizes, int L, int B, int k, const void *idx_out, int max_n,
                TopkLevels &lv, int &ntot, int &ksum, int &lds)
{
    if (!logits || !idx_out || !level_sizes) return fail(LDIT_EINVAL, "%s: null argument", who);
    if (!aligned16(logits) || !aligned16(idx_out)) return fail(LDIT_EINVAL, "%s: operands must be 16-byte aligned", who);
    if (L <= 0 || B <= 0 || B > 65535 || k <= 0) return fail(LDIT_EINVAL, "%s: bad geometry (L=%d B=%d k=%d)", who, L, B, k);
    if (L > TOPK_MAX_LEVELS) return fail(LDIT_EUNSUPPORTED, "%s: %d levels, at most %d are handled", who, L, TOPK_MAX_LEVELS);
    lv.n_levels = L;
    int64_t off = 0, kofs = 0, nmax = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t n = level_sizes[l];
        if (n <= 0) return fail(LDIT_EINVAL, "%s: level %d has %lld anchors", who, l, (long long)n);
        if (n > max_n)
            return fail(LDIT_EUNSUPPORTED, "%s: level %d has %lld anchors, at most %d per level are handled", who, l, (long long)n, max_n);
        lv.off[l] = (int)off; lv.n[l] = (int)n; lv.kofs[l] = (int)kofs; lv.k[l] = (int)(k < n ? k : n);
        off += n; kofs += lv.k[l];
        nmax = n > nmax ? n : nmax;
    }
    int n2 = 2;
    while (n2 < nmax && n2 < SORT_MAX_N) n2 <<= 1;
    ntot = (int)off; ksum = (int)kofs; lds = n2 * (int)sizeof(u64);
    return LDIT_OK;
}

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_rpn_topk_f32(const void *logits, const int64_t *level_sizes, int32_t L, int32_t B, int32_t k, void *idx_out, ldit_stream stream)
{
    TopkLevels lv{};
    int ntot = 0, ksum = 0, lds = 0;
    if (int rc = topk_levels("rpn_topk", logits, level_sizes, L, B, k, idx_out, TOPK_MAX_N, lv, ntot, ksum, lds)) return rc;
    LDIT_DYN_LDS(rpn_topk_kernel, TOPK_MAX_N * (int)sizeof(u64));
    hipLaunchKernelGGL(rpn_topk_kernel, dim3((unsigned)L, (unsigned)B), dim3(PROP_THREADS), lds, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(logits), static_cast<int *>(idx_out), lv, ntot, ksum);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int ldit_rpn_topk_chunked_f32(const void *logits, const int64_t *level_sizes, int32_t L, int32_t B, int32_t k, void *idx_out,
                              ldit_stream stream)
{
    TopkLevels lv{};
    int ntot = 0, ksum = 0, lds = 0;
    if (int rc = topk_levels("rpn_topk_chunked", logits, level_sizes, L, B, k, idx_out, TOPK_CHUNKED_MAX_N, lv, ntot, ksum, lds)) return rc;
    if (k > TOPK_CHUNKED_MAX_K) return fail(LDIT_EUNSUPPORTED, "rpn_topk_chunked: k=%d, at most %d are handled", k, TOPK_CHUNKED_MAX_K);
    LDIT_DYN_LDS(rpn_topk_chunked_kernel, SORT_MAX_N * (int)sizeof(u64));
    hipLaunchKernelGGL(rpn_topk_chunked_kernel, dim3((unsigned)L, (unsigned)B), dim3(PROP_THREADS), lds, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(logits), static_cast<int *>(idx_out), lv, ntot, ksum);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int ldit_rpn_decode_f32(const void *logits, const void *deltas, const void *anchors, const void *idx, int32_t B, int64_t Ntot, int64_t Ksum,
                        float img_h, float img_w, float min_size, float score_thresh, void *boxes_out, void *scores_out,
                        ldit_stream stream)
{
    if (!logits || !deltas || !anchors || !idx || !boxes_out || !scores_out) return fail(LDIT_EINVAL, "rpn_decode: null argument");
    if (!aligned16(logits) || !aligned16(deltas) || !aligned16(anchors) || !aligned16(idx) || !aligned16(boxes_out) || !aligned16(scores_out))
        return fail(LDIT_EINVAL, "rpn_decode: operands must be 16-byte aligned");
    if (B <= 0 || Ntot <= 0 || Ksum <= 0 || !(img_h > 0.f) || !(img_w > 0.f)) return fail(LDIT_EINVAL, "rpn_decode: bad geometry");
    if (Ntot >= (1ll << 31) || (int64_t)B * Ksum >= (1ll << 31)) return fail(LDIT_EUNSUPPORTED, "rpn_decode: operand exceeds 2^31 elements");
    const int total = (int)((int64_t)B * Ksum);
    hipLaunchKernelGGL(rpn_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(logits), static_cast<const f32x4 *>(deltas), static_cast<const f32x4 *>(anchors),
                       static_cast<const int *>(idx), static_cast<f32x4 *>(boxes_out), static_cast<float *>(scores_out), total, (int)Ntot,
                       (int)Ksum, img_h, img_w, min_size, score_thresh);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

/* the candidates live in registers and the sort in LDS: no workspace */
size_t ldit_nms_workspace_bytes(int64_t P, int64_t N)
{
    (void)P; (void)N;
    return 0;
}

int ldit_nms_batched_f32(const void *boxes, const void *scores, const void *groups, int32_t P, int64_t N, float iou_thr, int32_t max_out,
                         void *keep, void *count, void *out_boxes, void *out_scores, void *workspace, size_t workspace_bytes,
                         ldit_stream stream)
{
    if (!boxes || !scores || !keep || !count) return fail(LDIT_EINVAL, "nms: null argument");
    if (!aligned16(boxes) || !aligned16(scores) || !aligned16(keep) || !aligned16(count) || !aligned16(groups) || !aligned16(out_boxes) ||
        !aligned16(out_scores) || !aligned16(workspace))
        return fail(LDIT_EINVAL, "nms: operands must be 16-byte aligned");
    if (P <= 0 || P > 65535 || N <= 0 || max_out <= 0) return fail(LDIT_EINVAL, "nms: bad geometry (P=%d N=%lld max_out=%d)", P, (long long)N, max_out);
    if (iou_thr != iou_thr) return fail(LDIT_EINVAL, "nms: iou_thr is NaN");
    if (N > NMS_MAX_N) return fail(LDIT_EUNSUPPORTED, "nms: %lld candidates per problem, at most %d are handled", (long long)N, NMS_MAX_N);
    if ((int64_t)P * (N > max_out ? N : (int64_t)max_out) >= (1ll << 29)) return fail(LDIT_EUNSUPPORTED, "nms: operand exceeds 2^31 elements");
    const size_t need = ldit_nms_workspace_bytes(P, N);
    if (need && (!workspace || workspace_bytes < need))
        return fail(LDIT_EWORKSPACE, "nms: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    int n2 = 2;
    while (n2 < N) n2 <<= 1;
    const int lds = n2 * (int)sizeof(u64) + NMS_LDS_EXTRA;
    LDIT_DYN_LDS(nms_batched_kernel, NMS_MAX_N * (int)sizeof(u64) + NMS_LDS_EXTRA);
    hipLaunchKernelGGL(nms_batched_kernel, dim3((unsigned)P), dim3(PROP_THREADS), lds, static_cast<hipStream_t>(stream),
                       static_cast<const f32x4 *>(boxes), static_cast<const float *>(scores), static_cast<const int *>(groups), (int)N, iou_thr,
                       max_out, static_cast<int *>(keep), static_cast<int *>(count), static_cast<f32x4 *>(out_boxes),
                       static_cast<float *>(out_scores));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // extern "C"
