// Test-time augmentation, the merge: the padded detections of V views of a batch - other sizes, a horizontal mirror -
// mapped back to the pages and pooled per image, and, behind the class-wise NMS of the pool (ldit_nms_batched_f32, proposals.hip:
// there is no second NMS here), the kept boxes refined from the pool entries that agree with them ("box voting").  Two kernels, two
// launches, no host round trip, no allocation, no atomics, capturable; the outputs are pure functions of the inputs.
//
//   tta_pool     one thread per pool slot (view v, detection d) of an image.  A slot below the view's count is unmirrored in the
//                view's coordinates and scaled to the page; a slot at or beyond it is (-inf, label 0, zero box) and its input row is
//                never read.  The view descriptors and the pages' sizes travel in the kernel arguments (no device-side table).
//   box_vote     one wave per kept detection.  The lanes stride the image's pool (read through L2: at its largest, 8192 x 24 bytes, it
//                does not fit LDS and every entry is used once per wave), each lane sums the members it meets in ascending pool
//                order in double, the wave folds the 64 partial sums in a fixed butterfly, lane 0 rounds the quotient to fp32 once.
//                The same wave gathers the kept label and zeroes the rows at or beyond the kept count.
//
// Which entry votes is compared exactly with a float32 oracle (tests/tta_oracle.py), and so are the pooled coordinates: contraction
// is off for this whole file and the fp32 division is the correctly rounded one (the Makefile pins the flags, as for the other box
// kernels).  The IoU is formed in the order of iou_exceeds (proposals.hip).
#include "ldit_common.h"

#pragma clang fp contract(off)

namespace ldit {
namespace {

constexpr int TTA_MAX_VIEWS = 16;
constexpr int TTA_MAX_IMAGES = 256;                      // images of one launch: their sizes are kernel arguments
constexpr int TTA_MAX_POOL = 8192;                       // V * D: the candidates ldit_nms_batched_f32 handles per problem
constexpr int VOTE_WAVES = 4;                            // kept detections per workgroup

struct TtaViews {
    const f32x4 *boxes[TTA_MAX_VIEWS];                   // [B, D, 4]
    const float *scores[TTA_MAX_VIEWS];                  // [B, D]
    const int *labels[TTA_MAX_VIEWS];                    // [B, D]
    const int *count[TTA_MAX_VIEWS];                     // [B]
    int W[TTA_MAX_VIEWS], H[TTA_MAX_VIEWS];
    unsigned flip;                                       // bit v: view v is mirrored left-right
    int first;                                           // first image of this launch
    int ow[TTA_MAX_IMAGES], oh[TTA_MAX_IMAGES];          // the pages of images first .. first + gridDim.z - 1
};
static_assert(sizeof(TtaViews) + 64 <= 4096, "the descriptors of one launch must fit the kernel-argument segment");

__global__ void __launch_bounds__(256) tta_pool(const TtaViews t, int V, int D, f32x4 *__restrict__ pool_boxes,
                                                float *__restrict__ pool_scores, int *__restrict__ pool_labels)
{
    const int d = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y, i = blockIdx.z;
    if (d >= D) return;
    const size_t b = (size_t)t.first + i;
    int n = t.count[v][b];
    n = n < 0 ? 0 : (n > D ? D : n);
    const size_t dst = (b * V + v) * D + d;
    if (d >= n) {                                        // the input's padding row is never read
        pool_boxes[dst] = f32x4{0.f, 0.f, 0.f, 0.f};
        pool_scores[dst] = -__builtin_inff();
        pool_labels[dst] = 0;
        return;
    }
    const size_t src = b * D + d;
    const f32x4 r = t.boxes[v][src];
    const float Wv = (float)t.W[v];
    // the ratios of resize_boxes: double quotients rounded to fp32 once
    const float rw = (float)((double)t.ow[i] / (double)t.W[v]), rh = (float)((double)t.oh[i] / (double)t.H[v]);
    float x1 = r.x, x2 = r.z;
    if ((t.flip >> v) & 1u) {
        x1 = Wv - r.z;
        x2 = Wv - r.x;
    }
    pool_boxes[dst] = f32x4{x1 * rw, r.y * rh, x2 * rw, r.w * rh};
    pool_scores[dst] = t.scores[v][src];
    pool_labels[dst] = t.labels[v][src];
}

// the sum over the wave's lanes, the same bits in every lane: a butterfly of fixed shape
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

__global__ void __launch_bounds__(64 * VOTE_WAVES) box_vote(const f32x4 *__restrict__ pool_boxes, const float *__restrict__ pool_scores,
                                                            const int *__restrict__ pool_labels, const int *__restrict__ keep,
                                                            const int *__restrict__ kept, int N, int Dout, float thr,
                                                            f32x4 *__restrict__ out_boxes, int *__restrict__ out_labels)
{
    const int lane = threadIdx.x & 63, k = blockIdx.y * VOTE_WAVES + (threadIdx.x >> 6);
    const size_t b = blockIdx.x;
    if (k >= Dout) return;                               // the whole wave; no barrier follows
    int cnt = kept[b];
    cnt = cnt < 0 ? 0 : (cnt > Dout ? Dout : cnt);
    const size_t o = b * Dout + k;
    const int id = k < cnt ? keep[o] : -1;
    if ((unsigned)id >= (unsigned)N) {                   // a padding row (or no pool index at all): zero
        if (lane == 0) {
            if (out_boxes) out_boxes[o] = f32x4{0.f, 0.f, 0.f, 0.f};
            out_labels[o] = 0;
        }
        return;
    }
    pool_boxes += b * N; pool_scores += b * N; pool_labels += b * N;
    const int kl = pool_labels[id];
    if (lane == 0) out_labels[o] = kl;
    if (!out_boxes) return;
    const f32x4 kb = pool_boxes[id];
    const float kar = (kb.z - kb.x) * (kb.w - kb.y);
    double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0, sw = 0.0;
    for (int j = lane; j < N; j += 64) {
        if (pool_labels[j] != kl) continue;
        const float s = pool_scores[j];
        if (!(s > -__builtin_inff())) continue;          // not a candidate (NaN included)
        const f32x4 c = pool_boxes[j];
        bool member = j == id;                           // the kept box itself: always, even where its own IoU is NaN
        if (!member) {
            const float car = (c.z - c.x) * (c.w - c.y);
            const float iw = fmaxf(fminf(kb.z, c.z) - fmaxf(kb.x, c.x), 0.f);
            const float ih = fmaxf(fminf(kb.w, c.w) - fmaxf(kb.y, c.y), 0.f);
            const float inter = iw * ih;
            const float uni = (kar + car) - inter;
            member = inter / uni >= thr;
        }
        if (member) {
            const double w = (double)s;
            sx1 += w * (double)c.x; sy1 += w * (double)c.y; sx2 += w * (double)c.z; sy2 += w * (double)c.w;
            sw += w;
        }
    }
    sx1 = wave_sum(sx1); sy1 = wave_sum(sy1); sx2 = wave_sum(sx2); sy2 = wave_sum(sy2); sw = wave_sum(sw);
    if (lane == 0) out_boxes[o] = f32x4{(float)(sx1 / sw), (float)(sy1 / sw), (float)(sx2 / sw), (float)(sy2 / sw)};
}

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_tta_pool_f32(const void *const *boxes, const void *const *scores, const void *const *labels, const void *const *count,
                      const int32_t *view_specs, const int32_t *page_sizes, int32_t V, int32_t B, int32_t D, void *pool_boxes,
                      void *pool_scores, void *pool_labels, ldit_stream stream)
{
    if (!boxes || !scores || !labels || !count || !view_specs || !page_sizes || !pool_boxes || !pool_scores || !pool_labels)
        return fail(LDIT_EINVAL, "tta_pool: null argument");
    if (V <= 0 || B <= 0 || D <= 0) return fail(LDIT_EINVAL, "tta_pool: bad geometry (V=%d B=%d D=%d)", V, B, D);
    if (V > TTA_MAX_VIEWS) return fail(LDIT_EINVAL, "tta_pool: %d views, at most %d are handled", V, TTA_MAX_VIEWS);
    if ((int64_t)V * D > TTA_MAX_POOL)
        return fail(LDIT_EUNSUPPORTED, "tta_pool: V * D = %lld pool entries per image, at most %d are handled", (long long)V * D, TTA_MAX_POOL);
    if ((int64_t)B * V * D >= (1ll << 29)) return fail(LDIT_EUNSUPPORTED, "tta_pool: operand exceeds 2^31 elements");
    if (!aligned16(pool_boxes)) return fail(LDIT_EINVAL, "tta_pool: boxes must be 16-byte aligned");
    TtaViews t{};
    for (int v = 0; v < V; ++v) {
        if (!boxes[v] || !scores[v] || !labels[v] || !count[v]) return fail(LDIT_EINVAL, "tta_pool: null argument (view %d)", v);
        if (!aligned16(boxes[v])) return fail(LDIT_EINVAL, "tta_pool: boxes must be 16-byte aligned (view %d)", v);
        if (boxes[v] == pool_boxes || scores[v] == pool_scores || labels[v] == pool_labels)
            return fail(LDIT_EINVAL, "tta_pool: the outputs must not alias the inputs");
        const int32_t *s = view_specs + (size_t)v * 3;
        if (s[0] <= 0 || s[1] <= 0 || (s[2] != 0 && s[2] != 1))
            return fail(LDIT_EINVAL, "tta_pool: view %d is (W=%d, H=%d, flip=%d): positive sizes and flip 0 or 1 are expected", v, s[0], s[1], s[2]);
        t.boxes[v] = static_cast<const f32x4 *>(boxes[v]); t.scores[v] = static_cast<const float *>(scores[v]);
        t.labels[v] = static_cast<const int *>(labels[v]); t.count[v] = static_cast<const int *>(count[v]);
        t.W[v] = s[0]; t.H[v] = s[1];
        t.flip |= (unsigned)s[2] << v;
    }
    for (int i = 0; i < B; ++i)                                     // every page before the first launch
        if (page_sizes[2 * (size_t)i] <= 0 || page_sizes[2 * (size_t)i + 1] <= 0)
            return fail(LDIT_EINVAL, "tta_pool: image %d is %d x %d", i, page_sizes[2 * (size_t)i], page_sizes[2 * (size_t)i + 1]);
    for (int first = 0; first < B; first += TTA_MAX_IMAGES) {
        const int n = (B - first) < TTA_MAX_IMAGES ? (B - first) : TTA_MAX_IMAGES;
        t.first = first;
        for (int i = 0; i < n; ++i) {
            t.ow[i] = page_sizes[2 * (size_t)(first + i)];
            t.oh[i] = page_sizes[2 * (size_t)(first + i) + 1];
        }
        hipLaunchKernelGGL(tta_pool, dim3((unsigned)((D + 255) / 256), (unsigned)V, (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream),
                           t, (int)V, (int)D, static_cast<f32x4 *>(pool_boxes), static_cast<float *>(pool_scores), static_cast<int *>(pool_labels));
        LDIT_HIP_CHECK(hipGetLastError());
    }
    return LDIT_OK;
}

int ldit_box_vote_f32(const void *pool_boxes, const void *pool_scores, const void *pool_labels, const void *keep, const void *kept,
                      int32_t B, int32_t N, int32_t D_out, float vote_thresh, void *out_boxes, void *out_labels, ldit_stream stream)
{
    if (!pool_boxes || !pool_scores || !pool_labels || !keep || !kept || !out_labels) return fail(LDIT_EINVAL, "box_vote: null argument");
    if (!aligned16(pool_boxes) || !aligned16(out_boxes)) return fail(LDIT_EINVAL, "box_vote: boxes must be 16-byte aligned");
    if (B <= 0 || B > 65535 || N <= 0 || D_out <= 0) return fail(LDIT_EINVAL, "box_vote: bad geometry (B=%d N=%d D_out=%d)", B, N, D_out);
    if (!(vote_thresh >= 0.f && vote_thresh <= 1.f)) return fail(LDIT_EINVAL, "box_vote: vote_thresh=%g is outside [0, 1]", vote_thresh);
    if (N > TTA_MAX_POOL) return fail(LDIT_EUNSUPPORTED, "box_vote: %d pool entries per image, at most %d are handled", N, TTA_MAX_POOL);
    if ((int64_t)B * (N > D_out ? N : D_out) >= (1ll << 29)) return fail(LDIT_EUNSUPPORTED, "box_vote: operand exceeds 2^31 elements");
    if (D_out > 65535 * VOTE_WAVES) return fail(LDIT_EUNSUPPORTED, "box_vote: D_out=%d, at most %d are handled", D_out, 65535 * VOTE_WAVES);
    if (out_boxes == pool_boxes || out_labels == pool_labels || out_labels == keep)
        return fail(LDIT_EINVAL, "box_vote: the outputs must not alias the inputs");
    hipLaunchKernelGGL(box_vote, dim3((unsigned)B, (unsigned)((D_out + VOTE_WAVES - 1) / VOTE_WAVES)), dim3(64 * VOTE_WAVES), 0,
                       static_cast<hipStream_t>(stream), static_cast<const f32x4 *>(pool_boxes), static_cast<const float *>(pool_scores),
                       static_cast<const int *>(pool_labels), static_cast<const int *>(keep), static_cast<const int *>(kept), (int)N,
                       (int)D_out, vote_thresh, static_cast<f32x4 *>(out_boxes), static_cast<int *>(out_labels));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // extern "C"
