// The detector's input transform (ref src/layoutdit/modeling/model.py:50-54: torchvision GeneralizedRCNNTransform with fixed_size,
// image_mean = image_std = 0.5) as ONE arithmetic statement shared by every kernel that evaluates it - the stand-alone batch
// producer (misc.hip: preprocess_images) and the fused producer of the bf16 patch matrix (train_ops.hip: patches_rows_images) - so
// that both give a pixel the same bits: bilinear resize (align_corners = False, no antialias: F.interpolate(size=...)) of the
// [0, 1] image, then (v - mean) / std.  Every multiply-add is spelled out (no contraction left to the compiler).
#pragma once
#include <cstdint>
#include "ldit_common.h"

namespace ldit {

constexpr int PRE_MAX = 48;          // images per launch: their descriptors travel in the kernel arguments (no device-side table)
struct ImageList {
    const void *img[PRE_MAX];        // device pointers, logically [in_ch, h, w]: planar fp32 / fp16 / uint8, or interleaved uint8
    int h[PRE_MAX], w[PRE_MAX];
    int n, first;                    // images in this launch; index of the first one in the batch
    float mean, inv_std;
};

// What a stored sample stands for in [0, 1].  A uint8 code c stands for the correctly rounded single-precision quotient c / 255
// (what ToTensor() computes on the CPU), which these objects' `/` does not promise and c * (1 / 255) misses at 126 of the 256 codes.
// One Newton step on that product gives it: r = c - q * 255 is exact in one FMA (q * 255 needs 32 bits, the difference fits 24),
// and q + r * (1 / 255) is then rounded once; it equals the quotient at every one of the 256 codes.
__device__ __forceinline__ float pixel_unit(float v) { return v; }
__device__ __forceinline__ float pixel_unit(_Float16 v) { return (float)v; }
__device__ __forceinline__ float pixel_unit(uint8_t c)
{
    const float f = (float)c, rcp = 1.0f / 255.0f;      // the constant is folded by the front end, correctly rounded
    const float q = f * rcp;
    const float r = __builtin_fmaf(-q, 255.0f, f);
    return __builtin_fmaf(r, rcp, q);
}

struct BlendRow {                    // the two source rows of one output row and their weights
    int y0, y1;
    float ly, hy;
};

__device__ __forceinline__ BlendRow blend_row(int oy, int h, int out_h)
{
    const float sch = (float)h / (float)out_h;
    float sy = __builtin_fmaf((float)oy + 0.5f, sch, -0.5f);
    sy = sy < 0.f ? 0.f : sy;
    int y0 = (int)sy;
    y0 = y0 > h - 1 ? h - 1 : y0;
    BlendRow r;
    r.y0 = y0; r.y1 = y0 + (y0 < h - 1);
    r.ly = sy - (float)y0; r.hy = 1.f - r.ly;
    return r;
}

struct BlendCol {                    // the two source columns of one output column and their weights
    int x0, x1;
    float lx, hx;
};

__device__ __forceinline__ BlendCol blend_col(int ox, int w, int out_w)
{
    const float scw = (float)w / (float)out_w;
    float sx = __builtin_fmaf((float)ox + 0.5f, scw, -0.5f);
    sx = sx < 0.f ? 0.f : sx;
    int x0 = (int)sx;
    x0 = x0 > w - 1 ? w - 1 : x0;
    BlendCol c;
    c.x0 = x0; c.x1 = x0 + (x0 < w - 1);
    c.lx = sx - (float)x0; c.hx = 1.f - c.lx;
    return c;
}

// Train-time windows: image i of a windowed launch is the cw x ch window of its page whose top-left pixel ImageList
// img[i] points AT (the host adds the offset; h[i] / w[i] stay the page's, i.e. the plane and row strides), mirrored left-right
// where bit i of `flip` is set.  The descriptors travel in the kernel arguments beside the ImageList.
struct WindowList {
    int cw[PRE_MAX], ch[PRE_MAX];
    uint64_t flip;
};
static_assert(PRE_MAX <= 64, "one flip bit per image of a launch");

// blend_col on a window's extent; under flip window column x is source column cw - 1 - x (the weights stay with their columns, so
// blend_at evaluates the statement it evaluates on the mirrored copy)
__device__ __forceinline__ BlendCol blend_col_win(int ox, int cw, int out_w, bool flip)
{
    BlendCol c = blend_col(ox, cw, out_w);
    if (flip) { c.x0 = cw - 1 - c.x0; c.x1 = cw - 1 - c.x1; }
    return c;
}

// the normalised blend of the four samples at columns bc.x0 / bc.x1 of the source rows r0 / r1; `xs`: elements from one pixel of a
// row to the next (1 planar; in_ch interleaved, r0 / r1 then pointing at the channel wanted of the row's first pixel)
template <typename IN>
__device__ __forceinline__ float blend_at(const IN *__restrict__ r0, const IN *__restrict__ r1, const BlendCol &bc, int xs,
                                          const BlendRow &br, float mean, float inv_std)
{
    const size_t i0 = (size_t)bc.x0 * xs, i1 = (size_t)bc.x1 * xs;
    const float top = __builtin_fmaf(bc.lx, pixel_unit(r0[i1]), bc.hx * pixel_unit(r0[i0]));
    const float bot = __builtin_fmaf(bc.lx, pixel_unit(r1[i1]), bc.hx * pixel_unit(r1[i0]));
    const float v = __builtin_fmaf(br.ly, bot, br.hy * top);
    return (v - mean) * inv_std;
}

// output pixel ox of a row whose source rows are r0 / r1 (w pixels each, planar), normalised
template <typename IN>
__device__ __forceinline__ float blend_pixel(const IN *__restrict__ r0, const IN *__restrict__ r1, int ox, int w, int out_w,
                                             const BlendRow &br, float mean, float inv_std)
{
    return blend_at(r0, r1, blend_col(ox, w, out_w), 1, br, mean, inv_std);
}

}  // namespace ldit
