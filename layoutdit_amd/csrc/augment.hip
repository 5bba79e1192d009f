// The target side of train-time augmentation: the padded (gt_boxes, gt_labels, gt_count) of a batch carried through
// the windows the input transform cut from the pages (misc.hip: preprocess_windows) - clip to the window, drop what is no longer
// visible, shift, mirror, scale to the batch, drop what became too small - and compacted in their original order, in ONE launch per
// 48 images: no boolean indexing, no host round trip, no atomics, capturable, output a pure function of the input.
//
//   augment_targets      one wave per image.  The wave walks the image's Gmax rows 64 at a time; a lane decides its row, the ballot of
//                        the decisions gives every kept row its place behind the rows kept so far (a prefix count: the order stays),
//                        the rows past the last kept one are zeroed.
//
// The decisions are compared exactly with a float32 oracle (tests/augment_oracle.py): contraction is off for this whole file and
// division / sqrt are the correctly rounded ones (the Makefile pins the flags, as for the other box kernels).
#include "ldit_common.h"
#include "image_blend.h"

#pragma clang fp contract(off)

namespace ldit {
namespace {

constexpr int AUG_MAX_GT = 512;                          // rows per image: the limit of ldit_rpn_targets_f32

// the windows of one launch, in the kernel arguments like the ImageList of the pixel side (no device-side table)
struct AugList {
    int x0[PRE_MAX], y0[PRE_MAX], cw[PRE_MAX], ch[PRE_MAX];
    float rw[PRE_MAX], rh[PRE_MAX];                      // float(out_w / cw), float(out_h / ch): double quotients rounded once
    uint64_t flip;
    int n, first;
};
static_assert(sizeof(AugList) + 64 <= 4096, "the descriptors of one launch must fit the kernel-argument segment");

__global__ void __launch_bounds__(64) augment_targets(const AugList a, const f32x4 *__restrict__ gt_boxes, const int *__restrict__ gt_labels,
                                                      const int *__restrict__ gt_count, int Gmax, float min_visibility, float min_size,
                                                      f32x4 *__restrict__ out_boxes, int *__restrict__ out_labels, int *__restrict__ out_count)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    const size_t b = (size_t)a.first + i;
    int G = gt_count[b];
    G = G < 0 ? 0 : (G > Gmax ? Gmax : G);
    gt_boxes += b * Gmax; out_boxes += b * Gmax;
    if (gt_labels) gt_labels += b * Gmax;
    if (out_labels) out_labels += b * Gmax;
    const float X0 = (float)a.x0[i], Y0 = (float)a.y0[i], X1 = (float)(a.x0[i] + a.cw[i]), Y1 = (float)(a.y0[i] + a.ch[i]);
    const float CW = (float)a.cw[i], rw = a.rw[i], rh = a.rh[i];
    const bool flip = (a.flip >> i) & 1;

    int kept = 0;                                        // wave-uniform: rows written so far
    for (int g0 = 0; g0 < G; g0 += 64) {
        const int g = g0 + lane;
        bool keep = false;
        f32x4 o{0.f, 0.f, 0.f, 0.f};
        int label = 0;
        if (g < G) {                                     // rows at or beyond the count are never read
            const f32x4 v = gt_boxes[g];
            const float ax1 = fminf(fmaxf(v.x, X0), X1), ax2 = fminf(fmaxf(v.z, X0), X1);
            const float ay1 = fminf(fmaxf(v.y, Y0), Y1), ay2 = fminf(fmaxf(v.w, Y0), Y1);
            const float iw = ax2 - ax1, ih = ay2 - ay1;
            keep = iw > 0.f && ih > 0.f && iw * ih >= min_visibility * ((v.z - v.x) * (v.w - v.y));
            float lx1 = ax1 - X0, lx2 = ax2 - X0;
            if (flip) {
                const float t = CW - lx2;
                lx2 = CW - lx1;
                lx1 = t;
            }
            const float ly1 = ay1 - Y0, ly2 = ay2 - Y0;
            o = f32x4{lx1 * rw, ly1 * rh, lx2 * rw, ly2 * rh};
            keep = keep && (o.z - o.x) >= min_size && (o.w - o.y) >= min_size;
            if (gt_labels) label = gt_labels[g];
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int at = kept + __popcll(mask & ((1ull << lane) - 1ull));     // at <= g: behind every row kept before it
            out_boxes[at] = o;
            if (out_labels) out_labels[at] = label;
        }
        kept += __popcll(mask);
    }
    for (int g = kept + lane; g < Gmax; g += 64) {
        out_boxes[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (out_labels) out_labels[g] = 0;
    }
    if (lane == 0) out_count[b] = kept;
}

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_augment_targets_f32(const void *gt_boxes, const void *gt_labels, const void *gt_count, const int32_t *windows, int32_t B,
                             int32_t Gmax, int32_t out_h, int32_t out_w, float min_visibility, float min_size, void *out_boxes,
                             void *out_labels, void *out_count, ldit_stream stream)
{
    if (!gt_boxes || !gt_count || !windows || !out_boxes || !out_count) return fail(LDIT_EINVAL, "augment_targets: null argument");
    if (gt_labels && !out_labels) return fail(LDIT_EINVAL, "augment_targets: gt_labels without out_labels");
    if (!aligned16(gt_boxes) || !aligned16(out_boxes)) return fail(LDIT_EINVAL, "augment_targets: boxes must be 16-byte aligned");
    if (B <= 0 || B > 65535 || Gmax <= 0 || out_h <= 0 || out_w <= 0)
        return fail(LDIT_EINVAL, "augment_targets: bad geometry (B=%d Gmax=%d out %d x %d)", B, Gmax, out_h, out_w);
    if (Gmax > AUG_MAX_GT) return fail(LDIT_EUNSUPPORTED, "augment_targets: Gmax=%d, at most %d boxes per image are handled", Gmax, AUG_MAX_GT);
    if (!(min_visibility >= 0.f) || !(min_size >= 0.f))
        return fail(LDIT_EINVAL, "augment_targets: min_visibility=%g and min_size=%g must not be negative", min_visibility, min_size);
    if (gt_boxes == out_boxes || (gt_labels && gt_labels == out_labels) || gt_count == out_count)
        return fail(LDIT_EINVAL, "augment_targets: the outputs must not alias the inputs");
    for (int i = 0; i < B; ++i)                                     // every window before the first launch; the pages are not known here
        if (int rc = check_window(windows + (size_t)i * 5, i, -1, -1)) return rc;
    for (int first = 0; first < B; first += PRE_MAX) {
        AugList a{};
        a.n = (B - first) < PRE_MAX ? (B - first) : PRE_MAX;
        a.first = first;
        for (int i = 0; i < a.n; ++i) {
            const int32_t *win = windows + (size_t)(first + i) * 5;
            a.x0[i] = win[0]; a.y0[i] = win[1]; a.cw[i] = win[2]; a.ch[i] = win[3];
            a.rw[i] = (float)((double)out_w / (double)win[2]);
            a.rh[i] = (float)((double)out_h / (double)win[3]);
            a.flip |= (uint64_t)win[4] << i;
        }
        hipLaunchKernelGGL(augment_targets, dim3((unsigned)a.n), dim3(64), 0, static_cast<hipStream_t>(stream), a,
                           static_cast<const f32x4 *>(gt_boxes), static_cast<const int *>(gt_labels), static_cast<const int *>(gt_count), (int)Gmax,
                           min_visibility, min_size, static_cast<f32x4 *>(out_boxes), static_cast<int *>(out_labels), static_cast<int *>(out_count));
        LDIT_HIP_CHECK(hipGetLastError());
    }
    return LDIT_OK;
}

}  // extern "C"
