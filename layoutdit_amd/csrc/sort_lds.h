// Workgroup-wide bitonic sort of 8-byte keys in LDS, shared by the region-proposal stage (proposals.hip: top-k, NMS order) and
// the RPN's target assignment (rpn_train.hip: the sampler).  A key that is a total order makes the result unique.
#pragma once
#include <hip/hip_runtime.h>

namespace ldit {

constexpr int SORT_THREADS = 1024;                       // the workgroup every caller launches: 16 waves
constexpr int SORT_MAX_N = 16384;                        // 128 KiB of keys, of the 160 KiB of LDS a CU has

typedef unsigned long long u64;

__device__ __forceinline__ int pow2_at_least(int n)
{
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// ascending bitonic sort of n (a power of two) keys in LDS by the whole workgroup; the keys must be written and the caller
// need not have synchronised; returns after a barrier
__device__ inline void bitonic_sort(u64 *keys, int n)
{
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += SORT_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const u64 a = keys[i], b = keys[p];
                if ((a > b) == ((i & k) == 0)) {
                    keys[i] = b;
                    keys[p] = a;
                }
            }
            __syncthreads();
        }
}

}  // namespace ldit
