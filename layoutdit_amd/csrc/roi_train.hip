// Training side of the box head (torchvision RoIHeads.select_training_samples + fastrcnn_loss and the gradient of
// MultiScaleRoIAlign, which the reference reaches through loss_dict = model(images, targets), ref training/trainer.py:164-183).
// torchvision does this with cat, nonzero, randperm and an atomicAdd scatter; here it is four launches with fixed-size results: no
// host round trip, no allocation, no float atomics, capturable, output a pure function of the input (ldit.h, "box head training").
//
//   roi_targets          one workgroup per image.  The candidates are the image's valid proposals followed by its GT boxes; the GT
//                        boxes and labels sit in LDS.  One pass takes each candidate's IoU argmax and class; the bitonic sort of
//                        sort_lds.h orders (class, key, index), the match riding in the low bits of the sort key; each sorted
//                        position the sampler takes then writes its own output row.
//   roi_align_levels_bwd gather form of the transposed RoIAlign: a fixed grid over (image, level, 4 x 4 pixel tile); a workgroup
//                        walks the image's rows 256 at a time, compacts IN ASCENDING ROW ORDER (ballot + prefix) those of its
//                        level whose sample footprint meets the tile, lays their per-axis aggregated weights into LDS and then
//                        sums, per pixel, Ay[ph] Ax[pw] d_out[row, ph, pw, :] with lane l on channels 4 l .. 4 l + 3.
//   box_loss             one thread per row (softmax in double, smooth-L1 of the row's own class, the row of d_head written in
//                        full), per-block partial sums in a fixed order, one final single-workgroup pass in double.
//
// The IoU decides labels and the sample coordinates must be the forward's bit for bit: contraction is off for this whole file and
// division / sqrt are the correctly rounded ones (the Makefile pins the flags, as for proposals.hip, roi_heads.hip, rpn_train.hip).
#include "det_train_common.h"
#include "sort_lds.h"

#pragma clang fp contract(off)

namespace ldit {
namespace {

constexpr int RT_MAX_N = 4096;                           // candidates per image: 32 KiB of sort keys, 12 bits of index and match
constexpr int RT_LDS_EXTRA = 16;                         // two counters

struct CoderWeights { float x, y, w, h; };

__global__ __launch_bounds__(SORT_THREADS) void roi_targets_kernel(const f32x4 *__restrict__ proposals, const int *__restrict__ count,
                                                                   const f32x4 *__restrict__ gt_boxes, const int *__restrict__ gt_labels,
                                                                   const int *__restrict__ gt_count, const int *__restrict__ keys_in, int R,
                                                                   int Gmax, float fg_thr, float bg_thr, int batch_size, int quota_pos,
                                                                   CoderWeights cw, f32x4 *__restrict__ rois, int *__restrict__ labels,
                                                                   f32x4 *__restrict__ reg_targets, int *__restrict__ matched,
                                                                   int *__restrict__ sampled)
{
    // all LDS is dynamic: n2 sort keys, Gmax boxes, Gmax labels, two counters
    extern __shared__ __align__(16) unsigned char smem[];
    const int N = R + Gmax;
    const int n2 = pow2_at_least(N);
    u64 *keys = reinterpret_cast<u64 *>(smem);
    f32x4 *gt = reinterpret_cast<f32x4 *>(smem + (size_t)n2 * sizeof(u64));
    int *gtl = reinterpret_cast<int *>(smem + (size_t)n2 * sizeof(u64) + (size_t)Gmax * sizeof(f32x4));
    int *cnt = gtl + Gmax;                                           // [0] positives, [1] negatives
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    int G = gt_count[b], Rv = count[b];
    G = G < 0 ? 0 : (G > Gmax ? Gmax : G);
    Rv = Rv < 0 ? 0 : (Rv > R ? R : Rv);
    proposals += b * R; gt_boxes += b * Gmax; gt_labels += b * Gmax; keys_in += b * N;
    rois += b * batch_size; labels += b * batch_size; reg_targets += b * batch_size; matched += b * batch_size;

    for (int g = tid; g < G; g += SORT_THREADS) {
        gt[g] = gt_boxes[g];
        gtl[g] = gt_labels[g];
    }
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();

    // ---- IoU, argmax, class, sort key: candidate i < R is proposal i, candidate R + g is GT g ----
    int npos = 0, nneg = 0;
    for (int i = tid; i < n2; i += SORT_THREADS) {
        const bool valid = i < R ? i < Rv : i - R < G;
        if (!valid) {
            keys[i] = ~0ull;
            continue;
        }
        const f32x4 a = i < R ? proposals[i] : gt[i - R];
        const float aarea = (a.z - a.x) * (a.w - a.y);
        float best = -1.f;
        int arg = 0;
        for (int g = 0; g < G; ++g) {
            const f32x4 q = gt[g];
            const float v = iou_pair(a, aarea, q, (q.z - q.x) * (q.w - q.y));
            if (v > best) {                                          // strict: ties go to the lowest GT index
                best = v;
                arg = g;
            }
        }
        int cls;                                                     // 0 positive, 1 background, 2 ignored
        if (G == 0 || best < bg_thr) cls = 1;
        else cls = best >= fg_thr ? 0 : 2;
        npos += cls == 0;
        nneg += cls == 1;
        keys[i] = ((u64)cls << 56) | ((u64)((unsigned)keys_in[i] & 0x7fffffffu) << 24) | ((u64)(unsigned)i << 12) | (u64)(unsigned)arg;
    }
    if (npos) atomicAdd(&cnt[0], npos);                              // integer: order-independent
    if (nneg) atomicAdd(&cnt[1], nneg);
    bitonic_sort(keys, n2);                                          // starts and ends with a barrier

    // ---- the sampler: positives are sorted positions [0, P), negatives [P, P + Q); output row j is its own sorted position ----
    const int P = cnt[0], Q = cnt[1];
    const int take_pos = quota_pos < P ? quota_pos : P;
    const int room = batch_size - take_pos;
    const int take_neg = room < Q ? room : Q;
    for (int j = tid; j < batch_size; j += SORT_THREADS) {
        f32x4 box = f32x4{0.f, 0.f, 0.f, 0.f}, t = f32x4{0.f, 0.f, 0.f, 0.f};
        int lab = -1, m = -1;
        if (j < take_pos + take_neg) {
            const u64 k = keys[j < take_pos ? j : P + (j - take_pos)];
            const int i = (int)((k >> 12) & 0xfffu);
            box = i < R ? proposals[i] : gt[i - R];
            lab = 0;
            if (j < take_pos) {                                      // BoxCoder(wx, wy, ww, wh).encode_single
                m = (int)(k & 0xfffu);
                lab = gtl[m];
                const f32x4 q = gt[m];
                const float ew = box.z - box.x, eh = box.w - box.y, ecx = box.x + 0.5f * ew, ecy = box.y + 0.5f * eh;
                const float gw = q.z - q.x, gh = q.w - q.y, gcx = q.x + 0.5f * gw, gcy = q.y + 0.5f * gh;
                t = f32x4{cw.x * (gcx - ecx) / ew, cw.y * (gcy - ecy) / eh, cw.w * logf(gw / ew), cw.h * logf(gh / eh)};
            }
        }
        rois[j] = box;
        labels[j] = lab;
        reg_targets[j] = t;
        matched[j] = m;
    }
    if (tid == 0) {
        sampled[2 * b] = take_pos;
        sampled[2 * b + 1] = take_neg;
    }
}

// ---- RoIAlign backward --------------------------------------------------------------------------------------------------------
constexpr int RB_MAX_LEVELS = 8;
constexpr int RB_THREADS = 256;                          // 4 waves
constexpr int RB_TILE = 4;                               // a workgroup owns RB_TILE x RB_TILE pixels of one map of one image
constexpr int RB_CHUNK = RB_THREADS;                     // rows examined per round: one per thread
constexpr int RB_P = 7, RB_S = 2;
constexpr int RB_WPR = 2 * RB_TILE * RB_P;               // aggregated weights per listed row: Ay[tile row][ph], then Ax[tile column][pw]

struct RoiGradLevels {
    float *map[RB_MAX_LEVELS];
    long long sb[RB_MAX_LEVELS], sy[RB_MAX_LEVELS], sx[RB_MAX_LEVELS];      // element strides: batch, row, pixel (channel stride 1)
    int h[RB_MAX_LEVELS], w[RB_MAX_LEVELS];
    int tile_start[RB_MAX_LEVELS + 1];                                     // first workgroup (blockIdx.x) of every level
    float scale[RB_MAX_LEVELS];
};

// the forward's axis_sample (roi_heads.hip), restated: index pair and weights of coordinate v on an axis of n cells
__device__ __forceinline__ bool axis_sample_t(float v, int n, int &lo, int &hi, float &wlo, float &whi)
{
    if (v < -1.0f || v > (float)n) return false;
    v = fmaxf(v, 0.0f);
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

// weight that bin p of an axis (start, bin) of n cells puts on cell `cell`: the sum over the bin's RB_S samples, in sample order
__device__ __forceinline__ float axis_weight(float start, float bin, int p, int n, int cell)
{
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < RB_S; ++i) {
        const float v = start + (float)p * bin + ((float)i + 0.5f) * bin / (float)RB_S;      // the forward's expression
        int lo = 0, hi = 0;
        float wlo = 0.f, whi = 0.f;
        if (!axis_sample_t(v, n, lo, hi, wlo, whi)) continue;
        if (lo == cell) a += wlo;
        if (hi == cell) a += whi;
    }
    return a;
}

// may any sample of the axis touch a cell of [c0, c0 + RB_TILE)?  Conservative (a superset): the weights decide.
__device__ __forceinline__ bool axis_meets(float start, float bin, int n, int c0)
{
    const float first = start + 0.5f * bin / (float)RB_S;
    const float last = start + (float)(RB_P - 1) * bin + ((float)(RB_S - 1) + 0.5f) * bin / (float)RB_S;
    if (!(last >= -1.0f && first <= (float)n)) return false;          // every sample outside (or a NaN box)
    const int lo = (int)fminf(fmaxf(first, 0.0f), (float)(n - 1));
    const int hi = (int)fminf(fmaxf(last, 0.0f), (float)(n - 1)) + 1;
    return lo < c0 + RB_TILE && hi >= c0;
}

__global__ __launch_bounds__(RB_THREADS) void roi_align_levels_bwd_kernel(RoiGradLevels lv, int L, const float *__restrict__ d_out,
                                                                           const f32x4 *__restrict__ boxes, const int *__restrict__ count,
                                                                           const int *__restrict__ levels, int S, int C)
{
    __shared__ float wts[RB_CHUNK * RB_WPR];             // 56 KiB
    __shared__ int list[RB_CHUNK];
    __shared__ int wave_n[RB_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    int l = 0;
    for (int q = 1; q < L; ++q)
        if ((int)blockIdx.x >= lv.tile_start[q]) l = q;
    float *map = lv.map[0];
    long long sb = lv.sb[0], sy = lv.sy[0], sx = lv.sx[0];
    int h = lv.h[0], w = lv.w[0];
    float s = lv.scale[0];
#pragma unroll
    for (int q = 1; q < RB_MAX_LEVELS; ++q)
        if (l == q) {
            map = lv.map[q]; sb = lv.sb[q]; sy = lv.sy[q]; sx = lv.sx[q]; h = lv.h[q]; w = lv.w[q]; s = lv.scale[q];
        }
    map += (long long)b * sb;
    const int tile = (int)blockIdx.x - lv.tile_start[l];
    const int tiles_x = (w + RB_TILE - 1) / RB_TILE;
    const int y0 = (tile / tiles_x) * RB_TILE, x0 = (tile % tiles_x) * RB_TILE;
    int valid_rows = S;
    if (count) {
        valid_rows = count[b];
        valid_rows = valid_rows < 0 ? 0 : (valid_rows > S ? S : valid_rows);
    }
    boxes += (size_t)b * S;
    levels += (size_t)b * S;
    const int c4n = C >> 2;
    constexpr int PIX = RB_TILE * RB_TILE / (RB_THREADS / 64);       // pixels per wave: wave, wave + 4, ...

    for (int c4 = lane; c4 - lane < c4n; c4 += 64) {                 // one pass per 256 channels (uniform trip count)
        f32x4 acc[PIX];
#pragma unroll
        for (int k = 0; k < PIX; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < valid_rows; r0 += RB_CHUNK) {
            // ---- which rows of this round are on this level and may touch the tile ----
            const int r = r0 + tid;
            bool mine = false;
            float x1 = 0.f, yy1 = 0.f, bin_w = 0.f, bin_h = 0.f;
            if (r < valid_rows && levels[r] == l) {
                const f32x4 bx = boxes[r];
                x1 = bx.x * s; yy1 = bx.y * s;                       // the forward's arithmetic
                const float x2 = bx.z * s, y2 = bx.w * s;
                const float roi_w = fmaxf(x2 - x1, 1.0f), roi_h = fmaxf(y2 - yy1, 1.0f);
                bin_w = roi_w / (float)RB_P; bin_h = roi_h / (float)RB_P;
                mine = axis_meets(yy1, bin_h, h, y0) && axis_meets(x1, bin_w, w, x0);
            }
            // ---- compact them in ascending row order: ballot within the wave, prefix over the waves ----
            const unsigned long long vote = __ballot(mine);
            __syncthreads();                                         // the previous round's list and weights are no longer read
            if (lane == 0) wave_n[wave] = __popcll(vote);
            __syncthreads();
            int pos = __popcll(vote & ((1ull << lane) - 1ull)), n_list = 0;
            for (int q = 0; q < RB_THREADS / 64; ++q) {
                if (q < wave) pos += wave_n[q];
                n_list += wave_n[q];
            }
            if (mine) {
                list[pos] = r;
                float *wt = wts + pos * RB_WPR;
                for (int k = 0; k < RB_TILE * RB_P; ++k) {
                    wt[k] = axis_weight(yy1, bin_h, k % RB_P, h, y0 + k / RB_P);
                    wt[RB_TILE * RB_P + k] = axis_weight(x1, bin_w, k % RB_P, w, x0 + k / RB_P);
                }
            }
            __syncthreads();
            // ---- per pixel: sum over the listed rows (ascending), ph, pw of Ay[ph] Ax[pw] d_out[row, ph, pw, c] ----
            if (c4 < c4n) {
#pragma unroll
                for (int k = 0; k < PIX; ++k) {
                    const int pix = wave + k * (RB_THREADS / 64);
                    const int ty = pix / RB_TILE, tx = pix % RB_TILE;
                    if (y0 + ty >= h || x0 + tx >= w) continue;
                    for (int e = 0; e < n_list; ++e) {
                        const float *ay = wts + e * RB_WPR + ty * RB_P, *ax = wts + e * RB_WPR + RB_TILE * RB_P + tx * RB_P;
                        const float *g = d_out + ((size_t)b * S + list[e]) * (RB_P * RB_P) * C + 4 * c4;
                        for (int ph = 0; ph < RB_P; ++ph) {
                            const float wy = ay[ph];
                            if (wy == 0.f) continue;                 // wave-uniform: the weights are per (row, pixel)
                            for (int pw = 0; pw < RB_P; ++pw) {
                                const float wx = ax[pw];
                                if (wx == 0.f) continue;
                                acc[k] += (wy * wx) * *reinterpret_cast<const f32x4 *>(g + (size_t)(ph * RB_P + pw) * C);
                            }
                        }
                    }
                }
            }
        }
        if (c4 < c4n) {
#pragma unroll
            for (int k = 0; k < PIX; ++k) {
                const int pix = wave + k * (RB_THREADS / 64);
                const int y = y0 + pix / RB_TILE, x = x0 + pix % RB_TILE;
                if (y < h && x < w)
                    *reinterpret_cast<f32x4 *>(map + (long long)y * sy + (long long)x * sx + 4 * c4) = acc[k] * (1.0f / (float)(RB_S * RB_S));
            }
        }
    }
}

// ---- fastrcnn_loss ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_THREADS) void box_loss_kernel(const float *__restrict__ head, const int *__restrict__ labels,
                                                                const f32x4 *__restrict__ reg_targets, const int *__restrict__ sampled,
                                                                int B, int M, int NC, long long ld, float beta, float *__restrict__ d_head,
                                                                float *__restrict__ partial)
{
    __shared__ float red[LOSS_THREADS / 64];
    __shared__ int total_slot;
    const int total = sampled_total(sampled, B, &total_slot);
    const float inv = total > 0 ? 1.0f / (float)total : 0.f;
    const int row = blockIdx.x * LOSS_THREADS + threadIdx.x;
    float cls_loss = 0.f, box_loss = 0.f;
    if (row < M) {
        const float *lg = head + (long long)row * ld;
        float *dr = d_head + (long long)row * ld;
        int lab = labels[row];
        if (lab >= NC) lab = -1;                                     // outside the contract: left out, never indexed with
        for (long long j = 0; j < ld; ++j) dr[j] = 0.f;
        if (lab >= 0) {
            // log-sum-exp max-subtracted and in double, as box_postprocess evaluates its softmax
            float m = lg[0];
            for (int j = 1; j < NC; ++j) m = fmaxf(m, lg[j]);
            double sum = 0.0;
            for (int j = 0; j < NC; ++j) sum += exp((double)lg[j] - (double)m);
            cls_loss = (float)(((double)m + log(sum)) - (double)lg[lab]);
            for (int j = 0; j < NC; ++j) {
                const float p = (float)(exp((double)lg[j] - (double)m) / sum);
                dr[j] = (p - (j == lab ? 1.0f : 0.f)) * inv;
            }
        }
        if (lab >= 1) {
            const float *p = lg + NC + 4 * lab;
            const f32x4 t = reg_targets[row];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = p[c] - t[c], ad = fabsf(d);
                float g;
                if (ad < beta) {
                    box_loss += 0.5f * d * d / beta;
                    g = d / beta;
                } else {
                    box_loss += ad - 0.5f * beta;
                    g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                }
                dr[NC + 4 * lab + c] = g * inv;
            }
        }
    }
    const float cs = block_sum(cls_loss, red);
    const float bs = block_sum(box_loss, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = cs;
        partial[2 * blockIdx.x + 1] = bs;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void box_loss_final_kernel(const float *__restrict__ partial, int n_partial,
                                                                      const int *__restrict__ sampled, int B, float *__restrict__ loss)
{
    __shared__ double red[2][LOSS_THREADS];
    __shared__ int total_slot;
    const int total = sampled_total(sampled, B, &total_slot);
    loss_final(partial, n_partial, total, loss, red);
}

inline int box_loss_blocks(int64_t M) { return (int)((M + LOSS_THREADS - 1) / LOSS_THREADS); }

}  // namespace
}  // namespace ldit

using namespace ldit;

extern "C" {

int ldit_roi_targets_f32(const void *proposals, const void *count, const void *gt_boxes, const void *gt_labels, const void *gt_count,
                         const void *keys, int32_t B, int64_t R, int32_t Gmax, float fg_thr, float bg_thr, int32_t batch_size_per_image,
                         float positive_fraction, const float *weights, void *rois, void *labels, void *reg_targets, void *matched,
                         void *sampled, ldit_stream stream)
{
    if (!proposals || !count || !gt_boxes || !gt_labels || !gt_count || !keys || !weights || !rois || !labels || !reg_targets || !matched ||
        !sampled)
        return fail(LDIT_EINVAL, "roi_targets: null argument");
    if (!aligned16(proposals) || !aligned16(count) || !aligned16(gt_boxes) || !aligned16(gt_labels) || !aligned16(gt_count) || !aligned16(keys) ||
        !aligned16(rois) || !aligned16(labels) || !aligned16(reg_targets) || !aligned16(matched) || !aligned16(sampled))
        return fail(LDIT_EINVAL, "roi_targets: operands must be 16-byte aligned");
    if (B <= 0 || B > 65535 || R <= 0 || Gmax <= 0) return fail(LDIT_EINVAL, "roi_targets: bad geometry (B=%d R=%lld Gmax=%d)", B, (long long)R, Gmax);
    if (!(fg_thr >= bg_thr)) return fail(LDIT_EINVAL, "roi_targets: thresholds fg=%g bg=%g (bg must not exceed fg)", fg_thr, bg_thr);
    if (batch_size_per_image <= 0) return fail(LDIT_EINVAL, "roi_targets: batch_size_per_image=%d", batch_size_per_image);
    if (!(positive_fraction > 0.f && positive_fraction <= 1.f))
        return fail(LDIT_EINVAL, "roi_targets: positive_fraction=%g is outside (0, 1]", positive_fraction);
    for (int j = 0; j < 4; ++j)
        if (!(weights[j] > 0.f)) return fail(LDIT_EINVAL, "roi_targets: box coder weights must be positive");
    if (R + (int64_t)Gmax > RT_MAX_N)
        return fail(LDIT_EUNSUPPORTED, "roi_targets: %lld proposals + %d GT boxes per image, at most %d candidates are handled", (long long)R, Gmax,
                    RT_MAX_N);
    const int quota = (int)((double)batch_size_per_image * (double)positive_fraction);
    const int N = (int)R + Gmax;
    int n2 = 2;
    while (n2 < N) n2 <<= 1;
    const int per_gt = (int)(sizeof(f32x4) + sizeof(int));
    const int lds = n2 * (int)sizeof(u64) + Gmax * per_gt + RT_LDS_EXTRA;
    LDIT_DYN_LDS(roi_targets_kernel, RT_MAX_N * (int)sizeof(u64) + RT_MAX_N * per_gt + RT_LDS_EXTRA);
    hipLaunchKernelGGL(roi_targets_kernel, dim3((unsigned)B), dim3(SORT_THREADS), lds, static_cast<hipStream_t>(stream),
                       static_cast<const f32x4 *>(proposals), static_cast<const int *>(count), static_cast<const f32x4 *>(gt_boxes),
                       static_cast<const int *>(gt_labels), static_cast<const int *>(gt_count), static_cast<const int *>(keys), (int)R, (int)Gmax,
                       fg_thr, bg_thr, (int)batch_size_per_image, quota, CoderWeights{weights[0], weights[1], weights[2], weights[3]},
                       static_cast<f32x4 *>(rois), static_cast<int *>(labels), static_cast<f32x4 *>(reg_targets), static_cast<int *>(matched),
                       static_cast<int *>(sampled));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

int ldit_roi_align_levels_bwd_f32(const void *d_out, const void *boxes, const void *count, const void *levels, int32_t B, int64_t S,
                                  void *const *d_maps, const int32_t *map_h, const int32_t *map_w, const float *spatial_scale,
                                  const int64_t *stride_b, const int64_t *stride_y, const int64_t *stride_x, int32_t L, int64_t C, int32_t P,
                                  int32_t sampling_ratio, ldit_stream stream)
{
    if (!d_out || !boxes || !levels || !d_maps || !map_h || !map_w || !spatial_scale || !stride_b || !stride_y || !stride_x)
        return fail(LDIT_EINVAL, "roi_align_levels_bwd: null argument");
    if (L <= 0 || B <= 0 || B > 65535 || S <= 0 || C <= 0)
        return fail(LDIT_EINVAL, "roi_align_levels_bwd: bad geometry (L=%d B=%d S=%lld C=%lld)", L, B, (long long)S, (long long)C);
    if (L > RB_MAX_LEVELS) return fail(LDIT_EUNSUPPORTED, "roi_align_levels_bwd: %d levels, at most %d are handled", L, RB_MAX_LEVELS);
    if (C % 4) return fail(LDIT_EUNSUPPORTED, "roi_align_levels_bwd: C = %lld is not a multiple of 4", (long long)C);
    if (P != RB_P || sampling_ratio != RB_S)
        return fail(LDIT_EUNSUPPORTED, "roi_align_levels_bwd: output size %d / sampling ratio %d (7 / 2 is built)", P, sampling_ratio);
    if (!aligned16(d_out) || !aligned16(boxes) || !aligned16(count) || !aligned16(levels))
        return fail(LDIT_EINVAL, "roi_align_levels_bwd: operands must be 16-byte aligned");
    if ((int64_t)B * S >= (1ll << 31) || C >= (1ll << 20)) return fail(LDIT_EUNSUPPORTED, "roi_align_levels_bwd: operand exceeds 2^31 rows");
    RoiGradLevels lv{};
    int64_t tiles = 0;
    for (int l = 0; l < L; ++l) {
        if (!d_maps[l]) return fail(LDIT_EINVAL, "roi_align_levels_bwd: map %d is null", l);
        if (!aligned16(d_maps[l]) || stride_b[l] % 4 || stride_y[l] % 4 || stride_x[l] % 4)
            return fail(LDIT_EINVAL, "roi_align_levels_bwd: map %d must be 16-byte aligned with strides that are multiples of 4", l);
        if (map_h[l] <= 0 || map_w[l] <= 0 || !(spatial_scale[l] > 0.f) || stride_b[l] < 0 || stride_y[l] < 0 || stride_x[l] < C)
            return fail(LDIT_EINVAL, "roi_align_levels_bwd: map %d has a bad shape, scale or stride", l);
        lv.map[l] = static_cast<float *>(d_maps[l]);
        lv.h[l] = map_h[l]; lv.w[l] = map_w[l]; lv.scale[l] = spatial_scale[l];
        lv.sb[l] = stride_b[l]; lv.sy[l] = stride_y[l]; lv.sx[l] = stride_x[l];
        lv.tile_start[l] = (int)tiles;
        tiles += (int64_t)((map_h[l] + RB_TILE - 1) / RB_TILE) * ((map_w[l] + RB_TILE - 1) / RB_TILE);
        if (tiles >= (1ll << 30)) return fail(LDIT_EUNSUPPORTED, "roi_align_levels_bwd: maps exceed 2^30 tiles");
    }
    for (int l = L; l <= RB_MAX_LEVELS; ++l) lv.tile_start[l] = (int)tiles;
    hipLaunchKernelGGL(roi_align_levels_bwd_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(RB_THREADS), 0, static_cast<hipStream_t>(stream), lv,
                       (int)L, static_cast<const float *>(d_out), static_cast<const f32x4 *>(boxes), static_cast<const int *>(count),
                       static_cast<const int *>(levels), (int)S, (int)C);
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

/* one pair of partial sums per block of the first pass */
size_t ldit_box_loss_workspace_bytes(int64_t M)
{
    if (M <= 0) return 0;
    const size_t bytes = (size_t)box_loss_blocks(M) * 2 * sizeof(float);
    return (bytes + 15) & ~(size_t)15;
}

int ldit_box_loss_f32(const void *head_out, int64_t ld, const void *labels, const void *reg_targets, const void *sampled, int32_t B, int64_t M,
                      int32_t NC, float beta, void *loss, void *d_head, void *workspace, size_t workspace_bytes, ldit_stream stream)
{
    if (!head_out || !labels || !reg_targets || !sampled || !loss || !d_head) return fail(LDIT_EINVAL, "box_loss: null argument");
    if (!aligned16(head_out) || !aligned16(labels) || !aligned16(reg_targets) || !aligned16(sampled) || !aligned16(loss) || !aligned16(d_head) ||
        !aligned16(workspace))
        return fail(LDIT_EINVAL, "box_loss: operands must be 16-byte aligned");
    if (B <= 0 || B > 65535 || M <= 0 || NC < 2) return fail(LDIT_EINVAL, "box_loss: bad geometry (B=%d M=%lld NC=%d)", B, (long long)M, NC);
    if (ld < 5ll * NC) return fail(LDIT_EINVAL, "box_loss: row stride %lld is shorter than 5 * %d columns", (long long)ld, NC);
    if (!(beta >= 0.f) || beta == __builtin_inff()) return fail(LDIT_EINVAL, "box_loss: beta=%g", beta);
    if (M >= (1ll << 29) || M * ld >= (1ll << 40)) return fail(LDIT_EUNSUPPORTED, "box_loss: operand exceeds 2^31 elements");
    const size_t need = ldit_box_loss_workspace_bytes(M);
    if (!workspace || workspace_bytes < need) return fail(LDIT_EWORKSPACE, "box_loss: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int blocks = box_loss_blocks(M);
    hipLaunchKernelGGL(box_loss_kernel, dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(head_out), static_cast<const int *>(labels), static_cast<const f32x4 *>(reg_targets),
                       static_cast<const int *>(sampled), (int)B, (int)M, (int)NC, (long long)ld, beta, static_cast<float *>(d_head),
                       static_cast<float *>(workspace));
    LDIT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(box_loss_final_kernel, dim3(1), dim3(LOSS_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(workspace), blocks, static_cast<const int *>(sampled), (int)B, static_cast<float *>(loss));
    LDIT_HIP_CHECK(hipGetLastError());
    return LDIT_OK;
}

}  // extern "C"
