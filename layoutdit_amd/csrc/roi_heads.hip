// Box head of the detector in eval mode (torchvision RoIHeads, which the reference reaches through FasterRCNN(..., box_roi_pool =
// MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2)), ref src/layoutdit/modeling/model.py:34-55): the two stages around
// the head's GEMMs.  Two kernels, two launches, no host round trip, no allocation, no data-dependent shape, no atomics.
//
//   roi_align_levels   MultiScaleRoIAlign forward with the level assignment fused in: torchvision runs one nonzero() per level
//                      (a host synchronisation each) on NCHW maps; here the proposals arrive padded to [B, R] with a count, the maps
//                      are channels-last (any batch / row / pixel stride: the `pool` level is the strided view p5[:, :, ::2, ::2])
//                      and every row picks its own level.  One workgroup (4 waves) per row; a wave takes the bins wave, wave + 4, ...
//                      and lane l the channels 4 l .. 4 l + 3 (+ 256 per further pass): at C = 256 every corner read and every store
//                      is one coalesced 1 KiB access.  The output row (P, P, C) is the A operand of the fc6 GEMM as it stands.
//                      Templated on the output element: the bf16 instantiation (ldit_roi_align_levels_bf16, the bf16 box head) rounds
//                      the fp32 instantiation's value at the store - 8 bytes per lane - and shares every other statement with it.
//   box_postprocess    softmax over the class logits, BoxCoder(10, 10, 5, 5).decode of the class's deltas against the proposal,
//                      clip, score / small-box / padding filter; one thread per (proposal, foreground class), candidates in
//                      torchvision's flattening order so that ldit_nms_batched_f32 keyed by label finishes the stage.
//
// The level decision and the filters are compared exactly with an oracle, the sample coordinates within a few ulps: contraction is
// off for this whole file and division / sqrt are the correctly rounded ones (the Makefile pins the flags, as for proposals.hip).
#include "ldit_common.h"

#pragma clang fp contract(off)

namespace ldit {
namespace {

constexpr int ROI_MAX_LEVELS = 8;
constexpr int ROI_THREADS = 256;                         // 4 waves

typedef __bf16 roi_bf16x4 __attribute__((ext_vector_type(4)));

// four channels of an output row: fp32 as they are (16 bytes), or rounded to bf16 (to nearest even) at the store (8 bytes)
template <typename T> struct RoiOut;
template <> struct RoiOut<float> {
    typedef f32x4 vec;
    static __device__ __forceinline__ vec pack(const f32x4 &v) { return v; }
};
template <> struct RoiOut<__bf16> {
    typedef roi_bf16x4 vec;
    static __device__ __forceinline__ vec pack(const f32x4 &v) { return vec{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]}; }
};

struct RoiLevels {
    const float *map[ROI_MAX_LEVELS];
    long long sb[ROI_MAX_LEVELS], sy[ROI_MAX_LEVELS], sx[ROI_MAX_LEVELS];   // element strides: batch, row, pixel (channel stride 1)
    int h[ROI_MAX_LEVELS], w[ROI_MAX_LEVELS];
    float scale[ROI_MAX_LEVELS];
};

// one axis of torchvision's bilinear_interpolate: index pair and weights of coordinate v on an axis of n cells; false = outside
__device__ __forceinline__ bool axis_sample(float v, int n, int &lo, int &hi, float &wlo, float &whi)
{
    if (v < -1.0f || v > (float)n) return false;
    v = fmaxf(v, 0.0f);                                  // (NaN becomes 0: the indices below stay inside the map whatever the box)
    lo = (int)v;
    if (lo >= n - 1) {
        lo = hi = n - 1;
        v = (float)lo;
    } else {
        hi = lo + 1;
    }
    whi = v - (float)lo;
    wlo = 1.0f - whi;
    return true;
}

template <int P, int S, typename T>
__global__ __launch_bounds__(ROI_THREADS) void roi_align_levels_kernel(RoiLevels lv, int L, const f32x4 *__restrict__ boxes,
                                                                        const int *__restrict__ count, T *__restrict__ out,
                                                                        int *__restrict__ levels_out, int R, int C, int k_min, int k_max,
                                                                        float canonical_scale, float canonical_level)
{
    const long long row = blockIdx.x;                    // b * R + r
    const int b = (int)(row / R), r = (int)(row - (long long)b * R);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4n = C >> 2;
    typedef typename RoiOut<T>::vec out4;
    out4 *dst = reinterpret_cast<out4 *>(out + (size_t)row * (P * P) * C);
    const bool valid = !count || r < count[b];
    if (!valid) {                                        // padding row: zeros (uniform per workgroup)
        for (int i = threadIdx.x; i < P * P * c4n; i += ROI_THREADS) dst[i] = RoiOut<T>::pack(f32x4{0.f, 0.f, 0.f, 0.f});
        if (levels_out && threadIdx.x == 0) levels_out[row] = -1;
        return;
    }
    const f32x4 bx = boxes[row];
    // LevelMapper: floor(canonical_level + log2(sqrt(area) / canonical_scale) + 1e-6), clamped, relative to the finest level
    const float area = (bx.z - bx.x) * (bx.w - bx.y);
    float k = floorf(canonical_level + log2f(sqrtf(area) / canonical_scale) + 1e-6f);
    k = fminf(fmaxf(k, (float)k_min), (float)k_max);     // NaN (a NaN box) lands on k_min
    int l = (int)k - k_min;
    l = l < 0 ? 0 : (l >= L ? L - 1 : l);
    if (levels_out && threadIdx.x == 0) levels_out[row] = l;

    // the level's descriptor: l is uniform, so these are scalar selects
    const float *map = lv.map[0];
    long long sb = lv.sb[0], sy = lv.sy[0], sx = lv.sx[0];
    int h = lv.h[0], w = lv.w[0];
    float s = lv.scale[0];
#pragma unroll
    for (int q = 1; q < ROI_MAX_LEVELS; ++q)
        if (l == q) {
            map = lv.map[q]; sb = lv.sb[q]; sy = lv.sy[q]; sx = lv.sx[q]; h = lv.h[q]; w = lv.w[q]; s = lv.scale[q];
        }
    map += (long long)b * sb;

    // roi_align(aligned = False): no half-pixel shift, extent at least one cell
    const float x1 = bx.x * s, y1 = bx.y * s, x2 = bx.z * s, y2 = bx.w * s;
    const float roi_w = fmaxf(x2 - x1, 1.0f), roi_h = fmaxf(y2 - y1, 1.0f);
    const float bin_w = roi_w / (float)P, bin_h = roi_h / (float)P;

    for (int bin = wave; bin < P * P; bin += ROI_THREADS / 64) {
        const int ph = bin / P, pw = bin - ph * P;
        int ylo[S], yhi[S], xlo[S], xhi[S];
        float wylo[S], wyhi[S], wxlo[S], wxhi[S];
        bool yin[S], xin[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const float y = y1 + (float)ph * bin_h + ((float)i + 0.5f) * bin_h / (float)S;
            const float x = x1 + (float)pw * bin_w + ((float)i + 0.5f) * bin_w / (float)S;
            ylo[i] = yhi[i] = xlo[i] = xhi[i] = 0;
            wylo[i] = wyhi[i] = wxlo[i] = wxhi[i] = 0.f;
            yin[i] = axis_sample(y, h, ylo[i], yhi[i], wylo[i], wyhi[i]);
            xin[i] = axis_sample(x, w, xlo[i], xhi[i], wxlo[i], wxhi[i]);
        }
        for (int c4 = lane; c4 < c4n; c4 += 64) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int iy = 0; iy < S; ++iy)
#pragma unroll
                for (int ix = 0; ix < S; ++ix) {
                    if (!(yin[iy] && xin[ix])) continue;                     // wave-uniform
                    const float *rlo = map + (long long)ylo[iy] * sy, *rhi = map + (long long)yhi[iy] * sy;
                    const long long olo = (long long)xlo[ix] * sx + 4 * c4, ohi = (long long)xhi[ix] * sx + 4 * c4;
                    const f32x4 v1 = *reinterpret_cast<const f32x4 *>(rlo + olo), v2 = *reinterpret_cast<const f32x4 *>(rlo + ohi);
                    const f32x4 v3 = *reinterpret_cast<const f32x4 *>(rhi + olo), v4 = *reinterpret_cast<const f32x4 *>(rhi + ohi);
                    const float w1 = wylo[iy] * wxlo[ix], w2 = wylo[iy] * wxhi[ix], w3 = wyhi[iy] * wxlo[ix], w4 = wyhi[iy] * wxhi[ix];
                    acc += w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
                }
            dst[(size_t)bin * c4n + c4] = RoiOut<T>::pack(acc / (float)(S * S));
        }
    }
}

// torchvision RoIHeads.postprocess_detections up to the NMS
__global__ __launch_bounds__(256) void box_postprocess_kernel(const float *__restrict__ head, const f32x4 *__restrict__ proposals,
                                                               const int *__restrict__ count, f32x4 *__restrict__ boxes_out,
                                                               float *__restrict__ scores_out, int *__restrict__ labels_out, int total,
                                                               int R, int NC, long long ld, float img_h, float img_w, float wx, float wy,
                                                               float ww, float wh, float score_thresh, float min_size)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int F = NC - 1;
    const int b = i / (R * F), rem = i - b * (R * F);
    const int r = rem / F, c = rem - r * F + 1;
    const long long row = (long long)b * R + r;
    const float *lg = head + row * ld;
    // softmax over all NC logits in double: the fp32 score is the rounded exact value, whatever the spread of the logits
    float m = lg[0];
    for (int j = 1; j < NC; ++j) m = fmaxf(m, lg[j]);
    double sum = 0.0;
    for (int j = 0; j < NC; ++j) sum += exp((double)lg[j] - (double)m);
    float score = (float)(exp((double)lg[c] - (double)m) / sum);
    // BoxCoder(wx, wy, ww, wh).decode_single - the arithmetic of rpn_decode_kernel after the division by the weights
    const float *d = lg + NC + 4 * c;
    const f32x4 an = proposals[row];
    const float clip = 4.135166556742356f;                // log(1000 / 16)
    const float w = an.z - an.x, h = an.w - an.y;
    const float cx = an.x + 0.5f * w, cy = an.y + 0.5f * h;
    const float dx = d[0] / wx, dy = d[1] / wy;
    const float dw = fminf(d[2] / ww, clip), dh = fminf(d[3] / wh, clip);
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    float x1 = pcx - 0.5f * pw, y1 = pcy - 0.5f * ph, x2 = pcx + 0.5f * pw, y2 = pcy + 0.5f * ph;
    x1 = fminf(fmaxf(x1, 0.f), img_w); x2 = fminf(fmaxf(x2, 0.f), img_w);
    y1 = fminf(fmaxf(y1, 0.f), img_h); y2 = fminf(fmaxf(y2, 0.f), img_h);
    const bool padding = count && r >= count[b];
    if (padding || !(score > score_thresh) || !(x2 - x1 >= min_size) || !(y2 - y1 >= min_size)) score = -__builtin_inff();
    boxes_out[i] = f32x4{x1, y1, x2, y2};
    scores_out[i] = score;
    labels_out[i] = c;
}

}  // namespace
}  // namespace ldit

using namespace ldit;

// ldit_roi_align_levels_f32 / ldit_roi_align_levels_bf16: one set of refusals, the output element decides the instantiation
template <typename T>
static int roi_align_levels_entry(const void *const *maps, const int32_t *map_h, const int32_t *map_w, const float *spatial_scale,
                                  const int64_t *stride_b, const int64_t *stride_y, const int64_t *stride_x, int32_t L, int64_t C,
                                  const void *boxes, const void *count, int32_t B, int64_t R, int32_t P, int32_t sampling_ratio, int32_t k_min,
                                  int32_t k_max, float canonical_scale, float canonical_level, void *out, void *levels_out, ldit_stream stream)
{
    if (!maps || !map_h || !map_w || !spatial_scale || !stride_b || !stride_y || !stride_x || !boxes || !out)
        return fail(LDIT_EINVAL, "roi_align_levels: null argument");
    if (L <= 0 || B <= 0 || R <= 0 || C <= 0) return fail(LDIT_EINVAL, "roi_align_levels: bad geometry (L=%d B=%d R=%lld C=%lld)", L, B, (long long)R, (long long)C);
    if (L > ROI_MAX_LEVELS) return fail(LDIT_EUNSUPPORTED, "roi_align_levels: %d levels, at most %d are handled", L, ROI_MAX_LEVELS);
    if (C % 4) return fail(LDIT_EUNSUPPORTED, "roi_align_levels: C = %lld is not a multiple of 4", (long long)C);
    if (P != 7 || sampling_ratio != 2)
        return fail(LDIT_EUNSUPPORTED, "roi_align_levels: output size %d / sampling ratio %d (7 / 2 is built)", P, sampling_ratio);
    if (k_min > k_max || k_max - k_min >= L) return fail(LDIT_EINVAL, "roi_align_levels: levels k_min=%d .. k_max=%d do not fit %d maps", k_min, k_max, L);
    if (!(canonical_scale > 0.f)) return fail(LDIT_EINVAL, "roi_align_levels: canonical_scale must be positive");
    if (!aligned16(boxes) || !aligned16(out) || !aligned16(count) || !aligned16(levels_out))
        return fail(LDIT_EINVAL, "roi_align_levels: operands must be 16-byte aligned");
    if ((int64_t)B * R >= (1ll << 31) || C >= (1ll << 20)) return fail(LDIT_EUNSUPPORTED, "roi_align_levels: operand exceeds 2^31 rows");
    RoiLevels lv{};
    for (int l = 0; l < L; ++l) {
        if (!maps[l]) return fail(LDIT_EINVAL, "roi_align_levels: map %d is null", l);
        if (!aligned16(maps[l]) || stride_b[l] % 4 || stride_y[l] % 4 || stride_x[l] % 4)
            return fail(LDIT_EINVAL, "roi_align_levels: map %d must be 16-byte aligned with strides that are multiples of 4", l);
        if (map_h[l] <= 0 || map_w[l] <= 0 || !(spatial_scale[l] > 0.f) || stride_b[l] < 0 || stride_y[l] < 0 || stride_x[l] < C)
            return fail(LDIT_EINVAL, "roi_align_levels: map %d has a bad shape, scale or stride", l);
        lv.map[l] = static_cast<const float *>(maps[l]);
        lv.h[l] = map_h[l]; lv.w[l] = map_w[l]; lv.scale[l] = spatial_scale[l];
        lv.sb[l] = stride_b[l]; lv.sy[l] = stride_y[l]; lv.sx[l] = stride_x[l];
    }
    hipLaunchKernelGGL((roi_align_levels_kernel<7, 2, T>), dim3((unsigned)((int64_t)B * R)), dim3(ROI_THREADS), 0, static_cast<hipStream_t>(stream), lv,
                       (int)L, static_cast<const f32x4 *>(boxes), static_cast<const int *>(count), static_cast<T *>(out),
                       static_cast<int *>(levels_out), (int)R, (int)C, (int)k_min, (int)k_max, canonical_scale, canonical_level);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

extern "C" {

int ldit_roi_align_levels_f32(const void *const *maps, const int32_t *map_h, const int32_t *map_w, const float *spatial_scale,
                              const int64_t *stride_b, const int64_t *stride_y, const int64_t *stride_x, int32_t L, int64_t C,
                              const void *boxes, const void *count, int32_t B, int64_t R, int32_t P, int32_t sampling_ratio, int32_t k_min,
                              int32_t k_max, float canonical_scale, float canonical_level, void *out, void *levels_out, ldit_stream stream)
{
    return roi_align_levels_entry<float>(maps, map_h, map_w, spatial_scale, stride_b, stride_y, stride_x, L, C, boxes, count, B, R, P,
                                         sampling_ratio, k_min, k_max, canonical_scale, canonical_level, out, levels_out, stream);
}

int ldit_roi_align_levels_bf16(const void *const *maps, const int32_t *map_h, const int32_t *map_w, const float *spatial_scale,
                               const int64_t *stride_b, const int64_t *stride_y, const int64_t *stride_x, int32_t L, int64_t C,
                               const void *boxes, const void *count, int32_t B, int64_t R, int32_t P, int32_t sampling_ratio, int32_t k_min,
                               int32_t k_max, float canonical_scale, float canonical_level, void *out, void *levels_out, ldit_stream stream)
{
    return roi_align_levels_entry<__bf16>(maps, map_h, map_w, spatial_scale, stride_b, stride_y, stride_x, L, C, boxes, count, B, R, P,
                                          sampling_ratio, k_min, k_max, canonical_scale, canonical_level, out, levels_out, stream);
}

int ldit_box_postprocess_f32(const void *head, int64_t ld, const void *proposals, const void *count, int32_t B, int64_t R, int32_t NC,
                             float img_h, float img_w, const float *weights, float score_thresh, float min_size, void *boxes_out,
                             void *scores_out, void *labels_out, ldit_stream stream)
{
    if (!head || !proposals || !weights || !boxes_out || !scores_out || !labels_out) return fail(LDIT_EINVAL, "box_postprocess: null argument");
    if (!aligned16(head) || !aligned16(proposals) || !aligned16(count) || !aligned16(boxes_out) || !aligned16(scores_out) || !aligned16(labels_out))
        return fail(LDIT_EINVAL, "box_postprocess: operands must be 16-byte aligned");
    if (B <= 0 || R <= 0 || NC < 2 || !(img_h > 0.f) || !(img_w > 0.f)) return fail(LDIT_EINVAL, "box_postprocess: bad geometry");
    if (ld < 5ll * NC) return fail(LDIT_EINVAL, "box_postprocess: row stride %lld is shorter than 5 * %d columns", (long long)ld, NC);
    for (int j = 0; j < 4; ++j)
        if (!(weights[j] > 0.f)) return fail(LDIT_EINVAL, "box_postprocess: box coder weights must be positive");
    if ((int64_t)B * R * (NC - 1) >= (1ll << 29) || (int64_t)B * R * ld >= (1ll << 40))
        return fail(LDIT_EUNSUPPORTED, "box_postprocess: operand exceeds 2^31 elements");
    const int total = (int)((int64_t)B * R * (NC - 1));
    hipLaunchKernelGGL(box_postprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(head), static_cast<const f32x4 *>(proposals), static_cast<const int *>(count),
                       static_cast<f32x4 *>(boxes_out), static_cast<float *>(scores_out), static_cast<int *>(labels_out), total, (int)R, (int)NC,
                       (long long)ld, img_h, img_w, weights[0], weights[1], weights[2], weights[3], score_thresh, min_size);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // extern "C"
