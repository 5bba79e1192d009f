// Device helpers shared by the two training files of the detector (rpn_train.hip: anchors against GT; roi_train.hip: proposals
// against GT): the fp32 IoU whose bits decide labels, and the fixed-order sums of the loss passes.  Both files are built with
// contraction off and the correctly rounded division (Makefile); the pragma below covers the code of this header as well.
#pragma once
#include "ldit_common.h"

#pragma clang fp contract(off)

namespace ldit {

constexpr int LOSS_THREADS = 256;                        // the workgroup of every loss pass

// IoU of a box with a GT box: fp32, in the order of ldit_nms_batched_f32 (ldit.h).  A quotient that is not > 0 counts as +0
// (disjoint boxes skip the division: 0 / positive is 0 anyway), so the bits are those of a non-negative float.
__device__ __forceinline__ float iou_pair(const f32x4 a, float aarea, const f32x4 g, float garea)
{
    const float iw = fmaxf(fminf(a.z, g.z) - fmaxf(a.x, g.x), 0.f);
    const float ih = fmaxf(fminf(a.w, g.w) - fmaxf(a.y, g.y), 0.f);
    const float inter = iw * ih;
    if (!(inter > 0.f)) return 0.f;
    const float uni = (aarea + garea) - inter;
    const float q = inter / uni;
    return q > 0.f ? q : 0.f;
}

// fixed-order sum over the workgroup; every thread gets the total
__device__ __forceinline__ float block_sum(float v, float *red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < LOSS_THREADS / 64; ++w) s += red[w];
    return s;
}

// sum of sampled[0 .. 2 B): the rows in the loss - an integer, whatever the order
__device__ __forceinline__ int sampled_total(const int *__restrict__ sampled, int B, int *slot)
{
    if (threadIdx.x == 0) *slot = 0;
    __syncthreads();
    int s = 0;
    for (int i = threadIdx.x; i < 2 * B; i += LOSS_THREADS) s += sampled[i];
    if (s) atomicAdd(slot, s);
    __syncthreads();
    return *slot;
}

// the second pass of a loss: n_partial pairs of fp32 partial sums -> loss[0 .. 1] = their sums in double / total
__device__ __forceinline__ void loss_final(const float *__restrict__ partial, int n_partial, int total, float *__restrict__ loss,
                                           double (*red)[LOSS_THREADS])
{
    double c = 0.0, x = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += LOSS_THREADS) {
        c += (double)partial[2 * i];
        x += (double)partial[2 * i + 1];
    }
    red[0][threadIdx.x] = c;
    red[1][threadIdx.x] = x;
    __syncthreads();
    for (int o = LOSS_THREADS / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = total > 0 ? (float)(red[0][0] / (double)total) : 0.f;
        loss[1] = total > 0 ? (float)(red[1][0] / (double)total) : 0.f;
    }
}

}  // namespace ldit
