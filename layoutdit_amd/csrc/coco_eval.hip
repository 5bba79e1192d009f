// COCO box evaluation on the device (what the reference's Evaluator.score() hands to a per-image, per-category host loop, ref
// evaluation/evaluator.py:219-286): the per-image matching of detections to GT boxes and the accumulation of the precision /
// recall table, on fixed-size padded inputs with no host round trip, no allocation and no float atomics (ldit.h, "COCO box
// evaluation").
//
//   coco_match       one workgroup per image.  The bitonic sort of sort_lds.h orders the image's detections by (category, score
//                    descending, slot ascending); a sorted position minus the start of its category's run is the detection's rank.
//                    Then one thread per (category, area range, IoU threshold) walks its category's detections in rank order and
//                    matches greedily against the category's GT boxes in LDS - the IoU is recomputed in double where it is needed
//                    rather than kept as a tile - with the taken GT boxes as a 128-bit mask in registers.  The codes are laid out in
//                    LDS and leave as whole words.
//   coco_keys        one 64-bit key per stored detection: (category, inverted score bits, image * D + rank): a total order.  The
//                    device-wide sort of the keys is the caller's (torch.sort).
//   coco_accumulate  one workgroup per (category, area range, maxDet, IoU threshold).  It scans the category's run of the sorted
//                    detections 1024 at a time with INTEGER cumulative counts of true and false positives; a true positive with
//                    counts (tp, fp) has precision tp / (tp + fp + eps), and it is the first detection at which the recall reaches
//                    every recall threshold r with need(r) <= tp, need(r) the smallest count whose recall tp / npig is >= r.  The
//                    precision sampled at r is the largest precision of any detection at or after that point, i.e. the maximum over
//                    the true positives with tp >= need(r): each true positive is folded into the LAST threshold it serves with an
//                    integer maximum of its bit pattern (non-negative doubles order like their bits), and one suffix maximum over
//                    the 101 slots finishes the column.  Counts are integers and the maximum is exact: the result does not
//                    depend on the order anything ran in.
//
// Every IoU, area, precision and recall is double; contraction is off for this whole file (the Makefile pins the flags as for
// proposals.hip): the codes are compared exactly with a float64 oracle.
#include "ldit_common.h"
#include "sort_lds.h"

#pragma clang fp contract(off)

namespace ldit {
namespace {

constexpr int CE_MAX_D = 128, CE_MAX_G = 128, CE_MAX_K = 64;
constexpr int CE_AT = 40;                                // (area range, IoU threshold) pairs: 4 x 10
constexpr int CE_KEEP = 100;                             // detections kept per (image, category): the largest maxDet
constexpr int CE_REC = 101;
constexpr int ACC_THREADS = 1024;
constexpr unsigned char CE_ABSENT = 3;
constexpr double CE_EPS = 2.220446049250313e-16;

struct MatchParams { double iou[10], lo[4], hi[4]; };
struct AccParams { double rec[CE_REC]; int max_dets[3]; };

// a float as an unsigned whose ascending order is the float's ascending order (-0 has been folded into +0 by the caller)
__device__ __forceinline__ unsigned ordered_bits(float s)
{
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct BoxD { double x, y, w, h; };

// [x, y, w, h] IoU in double; crowd: the union is the detection's own area
__device__ __forceinline__ double iou_xywh(const BoxD &d, double darea, const BoxD &g, double garea, bool crowd)
{
    const double iw = fmin(d.x + d.w, g.x + g.w) - fmax(d.x, g.x);
    if (iw <= 0.0) return 0.0;
    const double ih = fmin(d.y + d.h, g.y + g.h) - fmax(d.y, g.y);
    if (ih <= 0.0) return 0.0;
    const double i = iw * ih;
    const double u = crowd ? darea : darea + garea - i;
    return i / u;
}

__global__ __launch_bounds__(SORT_THREADS) void coco_match_kernel(const f32x4 *__restrict__ boxes, const float *__restrict__ scores,
                                                                  const int *__restrict__ labels, const int *__restrict__ count,
                                                                  const f32x4 *__restrict__ gt_boxes, const int *__restrict__ gt_labels,
                                                                  const unsigned char *__restrict__ gt_crowd, const float *__restrict__ gt_area,
                                                                  const int *__restrict__ gt_count, int D, int G, int K, int Ds, MatchParams mp,
                                                                  unsigned *__restrict__ code_out, int *__restrict__ rank_out,
                                                                  int *__restrict__ npig_out, float *__restrict__ score_out,
                                                                  int *__restrict__ label_out)
{
    __shared__ u64 keys[CE_MAX_D];
    __shared__ BoxD dbox[CE_MAX_D], gbox[CE_MAX_G];                  // detections by SORTED POSITION, GT boxes by index
    __shared__ double darea[CE_MAX_D], gbarea[CE_MAX_G], gfarea[CE_MAX_G];      // GT: the box's area (IoU) and the area field (ranges)
    __shared__ int glabel[CE_MAX_G], rank_l[CE_MAX_D], seg_lo[CE_MAX_K + 2], seg_hi[CE_MAX_K + 2];
    __shared__ unsigned char gcrowd[CE_MAX_G];
    __shared__ unsigned code_w[CE_MAX_D * CE_AT / 4];                // code [slot, a, t] as bytes
    unsigned char *code_l = reinterpret_cast<unsigned char *>(code_w);

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    int Dv = count[b], Gv = gt_count[b];
    Dv = Dv < 0 ? 0 : (Dv > D ? D : Dv);
    Gv = Gv < 0 ? 0 : (Gv > G ? G : Gv);
    boxes += b * D; scores += b * D; labels += b * D;
    gt_boxes += b * G; gt_labels += b * G;
    if (gt_crowd) gt_crowd += b * G;
    if (gt_area) gt_area += b * G;
    code_out += b * (size_t)(Ds * (CE_AT / 4)); rank_out += b * Ds; score_out += b * Ds; label_out += b * Ds;
    npig_out += b * (size_t)(K * 4);
    const int n2 = pow2_at_least(D);

    // ---- stage: sort keys of the valid detections, the GT boxes, defaults ----
    if (tid < n2) {
        u64 key = ~0ull;
        if (tid < Dv) {                                              // a row at or past the count is never read
            const int lab = labels[tid];
            if (lab >= 1 && lab <= K)
                key = ((u64)(unsigned)lab << 40) | ((u64)(~ordered_bits(scores[tid] + 0.0f)) << 8) | (u64)(unsigned)tid;
        }
        keys[tid] = key;
    }
    if (tid < CE_MAX_D) rank_l[tid] = -1;
    if (tid < CE_MAX_G) {
        int lab = 0;                                                 // no category: never matched, never counted
        if (tid < Gv) {
            const f32x4 q = gt_boxes[tid];
            const BoxD g = {(double)q.x, (double)q.y, (double)q.z - (double)q.x, (double)q.w - (double)q.y};
            gbox[tid] = g;
            gbarea[tid] = g.w * g.h;
            gfarea[tid] = gt_area ? (double)gt_area[tid] : g.w * g.h;
            gcrowd[tid] = gt_crowd ? (unsigned char)(gt_crowd[tid] != 0) : (unsigned char)0;
            lab = gt_labels[tid];
        }
        glabel[tid] = lab;
    }
    if (tid < CE_MAX_K + 2) seg_lo[tid] = seg_hi[tid] = 0;
    for (int w = tid; w < CE_MAX_D * CE_AT / 4; w += SORT_THREADS) code_w[w] = 0x01010101u * CE_ABSENT;
    bitonic_sort(keys, n2);                                          // starts and ends with a barrier

    // ---- the runs of the categories; the detections' boxes by sorted position ----
    if (tid < n2) {
        const u64 key = keys[tid];
        if (key != ~0ull) {
            const int lab = (int)(key >> 40), slot = (int)(key & 0xffu);
            const int prev = tid > 0 ? (int)(keys[tid - 1] >> 40) : 0;
            const int next = tid + 1 < n2 && keys[tid + 1] != ~0ull ? (int)(keys[tid + 1] >> 40) : 0;
            if (lab != prev) seg_lo[lab] = tid;
            if (lab != next) seg_hi[lab] = tid + 1;
            const f32x4 q = boxes[slot];
            const BoxD d = {(double)q.x, (double)q.y, (double)q.z - (double)q.x, (double)q.w - (double)q.y};
            dbox[tid] = d;
            darea[tid] = d.w * d.h;
        }
    }
    __syncthreads();
    if (tid < n2) {
        const u64 key = keys[tid];
        if (key != ~0ull) {
            const int r = tid - seg_lo[(int)(key >> 40)];
            if (r < CE_KEEP) rank_l[(int)(key & 0xffu)] = r;
        }
    }
    __syncthreads();
    if (tid < Ds) {                                                  // the store's row: slots at or past D are absent
        const int r = rank_l[tid];
        rank_out[tid] = r;
        score_out[tid] = r >= 0 ? scores[tid] + 0.0f : 0.f;
        label_out[tid] = r >= 0 ? labels[tid] : 0;
    }

    // ---- greedy matching: one thread per (category, area range, threshold) ----
    for (int u = tid; u < K * CE_AT; u += SORT_THREADS) {
        const int k = u / CE_AT + 1, at = u % CE_AT, a = at / 10, t = at % 10;
        const double lo = mp.lo[a], hi = mp.hi[a], thr = mp.iou[t];
        int np = 0;
        for (int g = 0; g < Gv; ++g)
            np += glabel[g] == k && !(gcrowd[g] || gfarea[g] < lo || gfarea[g] > hi);
        if (t == 0) npig_out[(k - 1) * 4 + a] = np;
        const int p0 = seg_lo[k];
        int nd = seg_hi[k] - p0;
        nd = nd > CE_KEEP ? CE_KEEP : nd;
        u64 taken0 = 0, taken1 = 0;                                  // GT boxes matched at this threshold, by index
        for (int j = 0; j < nd; ++j) {
            const BoxD d = dbox[p0 + j];
            const double da = darea[p0 + j];
            double best = fmin(thr, 1.0 - 1e-10);
            int m = -1;
            // the GT in their order: the non-ignored ones by index, then the ignored ones by index; a match among the first ends
            // the scan before the second
            for (int pass = 0; pass < 2 && m < 0; ++pass)
                for (int g = 0; g < Gv; ++g) {
                    if (glabel[g] != k) continue;
                    const bool crowd = gcrowd[g] != 0;
                    const bool ign = crowd || gfarea[g] < lo || gfarea[g] > hi;
                    if ((int)ign != pass) continue;
                    const bool was = ((g < 64 ? taken0 >> g : taken1 >> (g - 64)) & 1ull) != 0;
                    if (was && !crowd) continue;
                    const double v = iou_xywh(d, da, gbox[g], gbarea[g], crowd);
                    if (v < best) continue;
                    best = v;                                        // an equal IoU replaces: the later GT wins a tie
                    m = g + (pass << 8);
                }
            unsigned char c;
            if (m >= 0) {
                const int g = m & 0xff;
                if (g < 64) taken0 |= 1ull << g;
                else taken1 |= 1ull << (g - 64);
                c = (m >> 8) ? 2 : 1;
            } else {
                c = (da < lo || da > hi) ? 2 : 0;
            }
            code_l[(int)(keys[p0 + j] & 0xffu) * CE_AT + at] = c;
        }
    }
    __syncthreads();
    for (int w = tid; w < Ds * (CE_AT / 4); w += SORT_THREADS) code_out[w] = code_w[w];
}

__global__ __launch_bounds__(256) void coco_keys_kernel(const int *__restrict__ rank, const float *__restrict__ scores,
                                                        const int *__restrict__ labels, long long total, int Ds,
                                                        long long *__restrict__ keys)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int r = rank[i];
    long long key = 0x7fffffffffffffffll;                            // absent: after every category
    if (r >= 0) {
        const long long img = i / Ds;
        key = (long long)(((u64)(unsigned)labels[i] << 56) | ((u64)(~ordered_bits(scores[i])) << 24) | (u64)(img * Ds + r));
    }
    keys[i] = key;
}

__device__ __forceinline__ long long lower_bound_key(const long long *__restrict__ keys, long long n, long long v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ACC_THREADS) void coco_accumulate_kernel(const long long *__restrict__ sorted_keys,
                                                                      const long long *__restrict__ sorted_index,
                                                                      const unsigned char *__restrict__ code, const int *__restrict__ rank,
                                                                      const int *__restrict__ npig, long long n_images, int Ds, int K,
                                                                      AccParams ap, double *__restrict__ precision,
                                                                      double *__restrict__ recall)
{
    __shared__ long long seg[2];
    __shared__ int total_s;
    __shared__ long long need[CE_REC];                               // need[r]: the smallest tp with tp / npig >= rec[r]
    __shared__ u64 slot_max[CE_REC];
    __shared__ u64 wsum[ACC_THREADS / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x % 10, mi = (blockIdx.x / 10) % 3, a = (blockIdx.x / 30) % 4, k = blockIdx.x / 120;
    const int M = ap.max_dets[mi];
    const long long L = n_images * Ds;

    if (tid == 0) {
        seg[0] = lower_bound_key(sorted_keys, L, (long long)(k + 1) << 56);
        seg[1] = lower_bound_key(sorted_keys, L, (long long)(k + 2) << 56);
        total_s = 0;
    }
    if (tid < CE_REC) slot_max[tid] = 0ull;                          // the bits of +0.0
    __syncthreads();
    int part = 0;
    for (long long i = tid; i < n_images; i += ACC_THREADS) part += npig[(i * K + k) * 4 + a];
    if (part) atomicAdd(&total_s, part);                             // integer: order-independent
    __syncthreads();
    const int total = total_s;
    const size_t rcell = (((size_t)t * K + k) * 4 + a) * 3 + mi;
    if (total == 0) {                                                // no GT to find: the cell stays -1, detections or not
        if (tid < CE_REC) precision[((((size_t)t * CE_REC + tid) * K + k) * 4 + a) * 3 + mi] = -1.0;
        if (tid == 0) recall[rcell] = -1.0;
        return;
    }
    if (tid < CE_REC) {
        const double r = ap.rec[tid], n = (double)total;
        long long c = (long long)ceil(r * n);
        c = c < 0 ? 0 : (c > total ? total : c);
        while (c > 0 && (double)(c - 1) / n >= r) --c;
        while (c < total && (double)c / n < r) ++c;
        need[tid] = (double)c / n >= r ? c : (long long)total + 1;   // a threshold above 1 is never reached
    }
    __syncthreads();

    u64 carry = 0;                                                   // (true positives << 32) | false positives so far
    for (long long base = seg[0]; base < seg[1]; base += ACC_THREADS) {
        const long long j = base + tid;
        u64 v = 0;
        if (j < seg[1]) {
            const long long idx = sorted_index[j];
            const int r = rank[idx];
            if (r >= 0 && r < M) {
                const unsigned char c = code[idx * CE_AT + a * 10 + t];
                v = c == 1 ? 1ull << 32 : (c == 0 ? 1ull : 0ull);
            }
        }
        u64 s = v;                                                   // inclusive scan over the wave, then over the waves
        for (int o = 1; o < 64; o <<= 1) {
            const u64 y = __shfl_up(s, o, 64);
            if (lane >= o) s += y;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        u64 before = 0, chunk = 0;
        for (int w = 0; w < ACC_THREADS / 64; ++w) {
            const u64 x = wsum[w];
            if (w < wave) before += x;
            chunk += x;
        }
        if (v >> 32) {
            const u64 incl = carry + before + s;
            const long long tp = (long long)(incl >> 32), fp = (long long)(incl & 0xffffffffull);
            const double pr = (double)tp / ((double)tp + (double)fp + CE_EPS);
            int lo = 0, hi = CE_REC - 1;                             // the last r with need[r] <= tp (need ascends with r)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (need[mid] <= tp) lo = mid;
                else hi = mid - 1;
            }
            // integer maximum of the bits of a non-negative double
            if (need[lo] <= tp) atomicMax(&slot_max[lo], (u64)__double_as_longlong(pr));
        }
        carry += chunk;
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) {
        recall[rcell] = (double)(long long)(carry >> 32) / (double)total;
        double run = 0.0;
        for (int r = CE_REC - 1; r >= 0; --r) {
            const double x = __longlong_as_double((long long)slot_max[r]);
            run = x > run ? x : run;
            precision[((((size_t)t * CE_REC + r) * K + k) * 4 + a) * 3 + mi] = run;
        }
    }
}

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_coco_match(const void *boxes, const void *scores, const void *labels, const void *count, const void *gt_boxes,
                    const void *gt_labels, const void *gt_crowd, const void *gt_area, const void *gt_count, int32_t B, int32_t D, int32_t G,
                    int32_t K, const double *iou_thrs, const double *area_rng, void *code, void *rank, void *npig, void *scores_out,
                    void *labels_out, int64_t capacity, int32_t store_D, int64_t image_offset, ldit_stream stream)
{
    if (!boxes || !scores || !labels || !count || !gt_boxes || !gt_labels || !gt_count || !iou_thrs || !area_rng || !code || !rank || !npig ||
        !scores_out || !labels_out)
        return fail(LDIT_EINVAL, "coco_match: null argument");
    if (!aligned16(boxes) || !aligned16(scores) || !aligned16(labels) || !aligned16(count) || !aligned16(gt_boxes) || !aligned16(gt_labels) ||
        !aligned16(gt_crowd) || !aligned16(gt_area) || !aligned16(gt_count) || !aligned16(code) || !aligned16(rank) || !aligned16(npig) ||
        !aligned16(scores_out) || !aligned16(labels_out))
        return fail(LDIT_EINVAL, "coco_match: operands must be 16-byte aligned");
    if (B <= 0 || B > 65535 || D <= 0 || G <= 0 || K <= 0) return fail(LDIT_EINVAL, "coco_match: bad geometry (B=%d D=%d G=%d K=%d)", B, D, G, K);
    if (D > CE_MAX_D || G > CE_MAX_G || K > CE_MAX_K)
        return fail(LDIT_EUNSUPPORTED, "coco_match: D=%d G=%d K=%d, at most %d detections and %d GT boxes per image and %d categories are handled",
                    D, G, K, CE_MAX_D, CE_MAX_G, CE_MAX_K);
    if (store_D < D || store_D > CE_MAX_D) return fail(LDIT_EINVAL, "coco_match: the store's row of %d slots does not hold D=%d (at most %d)", store_D, D, CE_MAX_D);
    if (image_offset < 0 || capacity <= 0 || image_offset + (int64_t)B > capacity)
        return fail(LDIT_EINVAL, "coco_match: images [%lld, %lld) do not fit a store of %lld", (long long)image_offset,
                    (long long)(image_offset + B), (long long)capacity);
    if (capacity * store_D > (1ll << 24)) return fail(LDIT_EUNSUPPORTED, "coco_match: a store of %lld x %d slots exceeds 2^24", (long long)capacity, store_D);
    MatchParams mp;
    for (int i = 0; i < 10; ++i) {
        if (!(iou_thrs[i] > 0.0 && iou_thrs[i] <= 1.0)) return fail(LDIT_EINVAL, "coco_match: IoU threshold %d = %g is outside (0, 1]", i, iou_thrs[i]);
        mp.iou[i] = iou_thrs[i];
    }
    for (int i = 0; i < 4; ++i) {
        if (!(area_rng[2 * i] <= area_rng[2 * i + 1])) return fail(LDIT_EINVAL, "coco_match: area range %d is empty", i);
        mp.lo[i] = area_rng[2 * i];
        mp.hi[i] = area_rng[2 * i + 1];
    }
    const size_t off = (size_t)image_offset;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)B), dim3(SORT_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const f32x4 *>(boxes), static_cast<const float *>(scores), static_cast<const int *>(labels),
                       static_cast<const int *>(count), static_cast<const f32x4 *>(gt_boxes), static_cast<const int *>(gt_labels),
                       static_cast<const unsigned char *>(gt_crowd), static_cast<const float *>(gt_area), static_cast<const int *>(gt_count),
                       (int)D, (int)G, (int)K, (int)store_D, mp, reinterpret_cast<unsigned *>(static_cast<unsigned char *>(code) + off * store_D * CE_AT),
                       static_cast<int *>(rank) + off * store_D, static_cast<int *>(npig) + off * K * 4,
                       static_cast<float *>(scores_out) + off * store_D, static_cast<int *>(labels_out) + off * store_D);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int ldit_coco_keys(const void *rank, const void *scores, const void *labels, int64_t n_images, int32_t store_D, void *keys, ldit_stream stream)
{
    if (!rank || !scores || !labels || !keys) return fail(LDIT_EINVAL, "coco_keys: null argument");
    if (!aligned16(rank) || !aligned16(scores) || !aligned16(labels) || !aligned16(keys))
        return fail(LDIT_EINVAL, "coco_keys: operands must be 16-byte aligned");
    if (n_images <= 0 || store_D <= 0 || store_D > CE_MAX_D) return fail(LDIT_EINVAL, "coco_keys: bad geometry (images=%lld D=%d)", (long long)n_images, store_D);
    const long long total = (long long)n_images * store_D;
    if (total > (1ll << 24)) return fail(LDIT_EUNSUPPORTED, "coco_keys: %lld x %d slots exceed 2^24", (long long)n_images, store_D);
    hipLaunchKernelGGL(coco_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const int *>(rank), static_cast<const float *>(scores), static_cast<const int *>(labels), total, (int)store_D,
                       static_cast<long long *>(keys));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int ldit_coco_accumulate(const void *sorted_keys, const void *sorted_index, const void *code, const void *rank, const void *npig,
                         int64_t n_images, int32_t store_D, int32_t K, const double *rec_thrs, const int32_t *max_dets, void *precision,
                         void *recall, ldit_stream stream)
{
    if (!code || !rank || !npig || !rec_thrs || !max_dets || !precision || !recall || (n_images > 0 && (!sorted_keys || !sorted_index)))
        return fail(LDIT_EINVAL, "coco_accumulate: null argument");
    if (!aligned16(sorted_keys) || !aligned16(sorted_index) || !aligned16(code) || !aligned16(rank) || !aligned16(npig) || !aligned16(precision) ||
        !aligned16(recall))
        return fail(LDIT_EINVAL, "coco_accumulate: operands must be 16-byte aligned");
    if (n_images < 0 || store_D <= 0 || store_D > CE_MAX_D || K <= 0)
        return fail(LDIT_EINVAL, "coco_accumulate: bad geometry (images=%lld D=%d K=%d)", (long long)n_images, store_D, K);
    if (K > CE_MAX_K) return fail(LDIT_EUNSUPPORTED, "coco_accumulate: K=%d, at most %d categories are handled", K, CE_MAX_K);
    if ((long long)n_images * store_D > (1ll << 24))
        return fail(LDIT_EUNSUPPORTED, "coco_accumulate: %lld x %d slots exceed 2^24", (long long)n_images, store_D);
    AccParams ap;
    for (int i = 0; i < CE_REC; ++i) {
        if (!(rec_thrs[i] >= 0.0) || (i && rec_thrs[i] < rec_thrs[i - 1]))
            return fail(LDIT_EINVAL, "coco_accumulate: the recall thresholds must be non-negative and ascending");
        ap.rec[i] = rec_thrs[i];
    }
    for (int i = 0; i < 3; ++i) {
        if (max_dets[i] <= 0 || max_dets[i] > CE_KEEP) return fail(LDIT_EINVAL, "coco_accumulate: maxDets[%d] = %d is outside [1, %d]", i, max_dets[i], CE_KEEP);
        ap.max_dets[i] = max_dets[i];
    }
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(K * 120)), dim3(ACC_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const long long *>(sorted_keys), static_cast<const long long *>(sorted_index),
                       static_cast<const unsigned char *>(code), static_cast<const int *>(rank), static_cast<const int *>(npig),
                       (long long)n_images, (int)store_D, (int)K, ap, static_cast<double *>(precision), static_cast<double *>(recall));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // extern "C"
