// Training criterion of Relation-DETR (models/bricks/set_criterion.py HybridSetCriterion, models/matcher/hungarian_matcher.py):
//   rdetr_match_cost_*  the matcher's cost matrices of a stack of prediction sets, one launch;
//   rdetr_set_loss_*    varifocal class loss, L1 and GIoU of a stack of matched sets, forward and gradient in one pass
//                       (one launch + one launch that adds the per-workgroup partial sums in a fixed order).
// fp32 math throughout; logits fp32 or bf16, boxes fp32.  Row r of a stack belongs to image r % B.
#include "launch.h"

#include <math.h>

namespace rdetr {
namespace {

constexpr int kCostThreads = 256;
constexpr int kCostPerThread = 4;              // (query, gt) pairs per lane: lane-consecutive pairs are consecutive along Gmax
constexpr int kCostMaxGt = 2048;               // the image's gt table in LDS: 5 words per gt
constexpr int kLossThreads = 256;
constexpr int kLossQueries = 32;               // queries per workgroup of the loss kernel = one [6] partial sum
constexpr float kLogEps = 1e-6f;               // hungarian_matcher.py:45-46

template <typename T> __device__ __forceinline__ float load_logit(const T *p);
template <> __device__ __forceinline__ float load_logit<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float load_logit<uint16_t>(const uint16_t *p) { return bf16_bits_to_f32(*p); }

__device__ __forceinline__ void store_logit(float *p, float v) { *p = v; }
__device__ __forceinline__ void store_logit(uint16_t *p, float v) { *p = (uint16_t)f32_to_bf16_bits(v); }

// kVec consecutive logits from / to an address aligned to kVec elements
constexpr int kVec = 4;
__device__ __forceinline__ void load_logits(const float *p, float (&x)[kVec])
{
    const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
__device__ __forceinline__ void load_logits(const uint16_t *p, float (&x)[kVec])
{
    const u32x2 v = *reinterpret_cast<const u32x2 *>(p);
    x[0] = bf16_bits_to_f32(v.x & 0xffffu), x[1] = bf16_bits_to_f32(v.x >> 16);
    x[2] = bf16_bits_to_f32(v.y & 0xffffu), x[3] = bf16_bits_to_f32(v.y >> 16);
}
__device__ __forceinline__ void store_logits(float *p, const float (&d)[kVec])
{
    *reinterpret_cast<f32x4 *>(p) = f32x4{d[0], d[1], d[2], d[3]};
}
__device__ __forceinline__ void store_logits(uint16_t *p, const float (&d)[kVec])
{
    *reinterpret_cast<u32x2 *>(p) = u32x2{pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3])};
}

// sigmoid(x) and sigmoid(-x) = 1 - sigmoid(x), neither by subtraction from 1
__device__ __forceinline__ void sigmoid_pair(float x, float &p, float &q)
{
    const float e = expf(-fabsf(x));
    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
    p = x >= 0.0f ? big : small;
    q = x >= 0.0f ? small : big;
}

__device__ __forceinline__ float pow_gamma(float p, float gamma, bool square)
{
    return square ? p * p : powf(p, gamma);
}

struct Xyxy {
    float x1, y1, x2, y2;
};

__device__ __forceinline__ Xyxy to_xyxy(float cx, float cy, float w, float h)       // torchvision _box_cxcywh_to_xyxy
{
    return {cx - 0.5f * w, cy - 0.5f * h, cx + 0.5f * w, cy + 0.5f * h};
}

// IoU and GIoU of two corner boxes (torchvision box_iou / generalized_box_iou, elementwise)
__device__ __forceinline__ void iou_giou(const Xyxy &a, const Xyxy &b, float &iou, float &giou)
{
    const float area_a = (a.x2 - a.x1) * (a.y2 - a.y1), area_b = (b.x2 - b.x1) * (b.y2 - b.y1);
    const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.0f), ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.0f);
    const float inter = iw * ih, uni = area_a + area_b - inter;
    iou = inter / uni;
    const float ew = fmaxf(fmaxf(a.x2, b.x2) - fminf(a.x1, b.x1), 0.0f), eh = fmaxf(fmaxf(a.y2, b.y2) - fminf(a.y1, b.y1), 0.0f);
    const float areai = ew * eh;
    giou = iou - (areai - uni) / areai;
}

// ------------------------------------------------------------------------------------------------------------------- match cost
template <typename T>
__global__ __launch_bounds__(kCostThreads) void match_cost_kernel(const T *__restrict__ logits, long long ld_logits,
                                                                  const float *__restrict__ boxes, long long ld_boxes,
                                                                  const float *__restrict__ gt_boxes, const int *__restrict__ gt_labels,
                                                                  const int *__restrict__ gt_count, int B, int N, int C, int Gmax,
                                                                  float alpha, float gamma, float w_class, float w_bbox, float w_giou,
                                                                  float *__restrict__ cost)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *s_box = lds;                                     // [Gmax, 4]
    int *s_lab = reinterpret_cast<int *>(lds + 4 * (size_t)Gmax);      // [Gmax]
    const int r = blockIdx.y, b = r % B;
    const int count = min(max(gt_count[b], 0), Gmax);
    for (int i = threadIdx.x; i < 4 * count; i += kCostThreads) s_box[i] = gt_boxes[(long long)b * Gmax * 4 + i];
    for (int i = threadIdx.x; i < count; i += kCostThreads) s_lab[i] = gt_labels[(long long)b * Gmax + i];
    __syncthreads();

    const bool square = gamma == 2.0f;
    const long long pairs = (long long)N * Gmax;
    const T *row_logits = logits + (long long)r * ld_logits;
    const float *row_boxes = boxes + (long long)r * ld_boxes;
    float *row_cost = cost + (long long)r * pairs;
    const long long base = (long long)blockIdx.x * (kCostThreads * kCostPerThread) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCostPerThread; ++k) {
        const long long idx = base + (long long)k * kCostThreads;
        if (idx >= pairs) break;
        const int n = (int)(idx / Gmax), g = (int)(idx - (long long)n * Gmax);
        float c = 0.0f;
        if (g < count) {
            const f32x4 pb = *reinterpret_cast<const f32x4 *>(row_boxes + (long long)n * 4);
            const float gx = s_box[4 * g], gy = s_box[4 * g + 1], gw = s_box[4 * g + 2], gh = s_box[4 * g + 3];
            const int lab = s_lab[g];
            float cls = 0.0f;
            if (lab >= 0 && lab < C) {
                float p, q;
                sigmoid_pair(load_logit(row_logits + (long long)n * C + lab), p, q);
                const float neg = -(1.0f - alpha) * pow_gamma(p, gamma, square) * logf(q + kLogEps);
                const float pos = -alpha * pow_gamma(q, gamma, square) * logf(p + kLogEps);
                cls = pos - neg;
            }
            const float l1 = fabsf(pb.x - gx) + fabsf(pb.y - gy) + fabsf(pb.z - gw) + fabsf(pb.w - gh);
            float iou, giou;
            iou_giou(to_xyxy(pb.x, pb.y, pb.z, pb.w), to_xyxy(gx, gy, gw, gh), iou, giou);
            c = w_bbox * l1 + w_class * cls + w_giou * -giou;
        }
        row_cost[idx] = c;
    }
}

template <typename T>
int match_cost(const T *logits, long long ld_logits, const float *boxes, long long ld_boxes, const float *gt_boxes,
               const int *gt_labels, const int *gt_count, int R, int B, int N, int C, int Gmax, float alpha, float gamma,
               float w_class, float w_bbox, float w_giou, float *cost, void *stream)
{
    if (R < 0 || B <= 0 || N < 0 || C <= 0 || Gmax <= 0) return RDETR_ERR_INVALID_ARG;
    if (R == 0 || N == 0) return RDETR_OK;
    if (!logits || !boxes || !gt_boxes || !gt_labels || !gt_count || !cost) return RDETR_ERR_INVALID_ARG;
    if (ld_logits < (long long)N * C || ld_boxes < (long long)N * 4) return RDETR_ERR_INVALID_ARG;
    if (Gmax > kCostMaxGt || R > 65535) return RDETR_ERR_UNSUPPORTED;
    if (!aligned_to(logits, sizeof(T)) || !aligned_to(boxes, 16) || ld_boxes % 4 || !aligned_to(gt_boxes, 4) || !aligned_to(gt_labels, 4)
        || !aligned_to(gt_count, 4) || !aligned_to(cost, 4))
        return RDETR_ERR_UNSUPPORTED;
    const long long pairs = (long long)N * Gmax, per_block = kCostThreads * kCostPerThread;
    const long long blocks = (pairs + per_block - 1) / per_block;
    if (!grid_fits(blocks)) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(match_cost_kernel<T>, dim3((unsigned)blocks, (unsigned)R), dim3(kCostThreads), (size_t)Gmax * 5 * sizeof(float),
                       static_cast<hipStream_t>(stream), logits, ld_logits, boxes, ld_boxes, gt_boxes, gt_labels, gt_count, B, N, C,
                       Gmax, alpha, gamma, w_class, w_bbox, w_giou, cost);
    return launch_status();
}

// --------------------------------------------------------------------------------------------------------------------- set loss
// d min(a, b) / da and d max(a, b) / da as autograd has them: a tie gives each operand half
__device__ __forceinline__ float pick_min(float a, float b) { return a < b ? 1.0f : (a == b ? 0.5f : 0.0f); }
__device__ __forceinline__ float pick_max(float a, float b) { return a > b ? 1.0f : (a == b ? 0.5f : 0.0f); }

template <typename T>
__global__ __launch_bounds__(kLossThreads) void set_loss_kernel(const T *__restrict__ logits, long long ld_logits,
                                                                const float *__restrict__ boxes, long long ld_boxes,
                                                                const int *__restrict__ match, const float *__restrict__ gt_boxes,
                                                                const int *__restrict__ gt_labels, int B, int N, int C, int Gmax,
                                                                int n_split, float inv_a, float inv_b, float alpha, float gamma,
                                                                float *__restrict__ partials, T *__restrict__ dlogits,
                                                                float *__restrict__ dbox_l1, float *__restrict__ dbox_giou)
{
    __shared__ float s_iou[kLossQueries];
    __shared__ int s_lab[kLossQueries];                     // the matched class, -1 where the query has none
    __shared__ float s_red[kLossThreads / kWave][6];
    const int r = blockIdx.y, b = r % B, n0 = blockIdx.x * kLossQueries;
    const int nq = min(kLossQueries, N - n0);
    const int tid = threadIdx.x;
    float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // {class, L1, GIoU} of the denoising segment, then of the rest

    if (tid < nq) {
        const int n = n0 + tid;
        const float inv = n < n_split ? inv_a : inv_b;
        const int m = match[(long long)r * N + n];
        f32x4 d1 = {0.0f, 0.0f, 0.0f, 0.0f}, dg = {0.0f, 0.0f, 0.0f, 0.0f};
        float iou = 0.0f;
        int lab = -1;
        if (m >= 0 && m < Gmax) {
            const f32x4 pb = *reinterpret_cast<const f32x4 *>(boxes + (long long)r * ld_boxes + (long long)n * 4);
            const float *gp = gt_boxes + ((long long)b * Gmax + m) * 4;
            const float gx = gp[0], gy = gp[1], gw = gp[2], gh = gp[3];
            lab = gt_labels[(long long)b * Gmax + m];
            if (lab < 0 || lab >= C) lab = -1;
            const float e0 = pb.x - gx, e1 = pb.y - gy, e2 = pb.z - gw, e3 = pb.w - gh;
            const float l1 = fabsf(e0) + fabsf(e1) + fabsf(e2) + fabsf(e3);
            const auto sgn = [](float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); };
            d1 = f32x4{sgn(e0), sgn(e1), sgn(e2), sgn(e3)} * inv;

            const Xyxy p = to_xyxy(pb.x, pb.y, pb.z, pb.w), g = to_xyxy(gx, gy, gw, gh);
            const float pw = p.x2 - p.x1, ph = p.y2 - p.y1;
            const float area_p = pw * ph, area_g = (g.x2 - g.x1) * (g.y2 - g.y1);
            const float iw_raw = fminf(p.x2, g.x2) - fmaxf(p.x1, g.x1), ih_raw = fminf(p.y2, g.y2) - fmaxf(p.y1, g.y1);
            const float iw = fmaxf(iw_raw, 0.0f), ih = fmaxf(ih_raw, 0.0f);
            const float inter = iw * ih, uni = area_p + area_g - inter;
            iou = inter / uni;
            const float ew_raw = fmaxf(p.x2, g.x2) - fminf(p.x1, g.x1), eh_raw = fmaxf(p.y2, g.y2) - fminf(p.y1, g.y1);
            const float ew = fmaxf(ew_raw, 0.0f), eh = fmaxf(eh_raw, 0.0f);
            const float areai = ew * eh;
            const float giou = iou - (areai - uni) / areai;
            // giou = inter / uni - 1 + uni / areai, uni = area_p + area_g - inter
            const float g_uni = 1.0f / areai - inter / (uni * uni);
            const float g_inter = 1.0f / uni - g_uni;
            const float g_areai = -uni / (areai * areai);
            const float g_iw = iw_raw >= 0.0f ? g_inter * ih : 0.0f, g_ih = ih_raw >= 0.0f ? g_inter * iw : 0.0f;
            const float g_ew = ew_raw >= 0.0f ? g_areai * eh : 0.0f, g_eh = eh_raw >= 0.0f ? g_areai * ew : 0.0f;
            const float gx1 = -g_iw * pick_max(p.x1, g.x1) - g_ew * pick_min(p.x1, g.x1) - g_uni * ph;
            const float gx2 = g_iw * pick_min(p.x2, g.x2) + g_ew * pick_max(p.x2, g.x2) + g_uni * ph;
            const float gy1 = -g_ih * pick_max(p.y1, g.y1) - g_eh * pick_min(p.y1, g.y1) - g_uni * pw;
            const float gy2 = g_ih * pick_min(p.y2, g.y2) + g_eh * pick_max(p.y2, g.y2) + g_uni * pw;
            // loss = 1 - giou; (cx, cy, w, h) from the corners
            dg = f32x4{gx1 + gx2, gy1 + gy2, 0.5f * (gx2 - gx1), 0.5f * (gy2 - gy1)} * -inv;
            const int seg = n < n_split ? 0 : 3;
            acc[seg + 1] = l1;
            acc[seg + 2] = 1.0f - giou;
        }
        *reinterpret_cast<f32x4 *>(dbox_l1 + ((long long)r * N + n) * 4) = d1;
        *reinterpret_cast<f32x4 *>(dbox_giou + ((long long)r * N + n) * 4) = dg;
        s_iou[tid] = iou;
        s_lab[tid] = lab;
    }
    __syncthreads();

    // The tile's [nq, C] logits are one contiguous range.  Rows of C = 91 bf16 are 182 bytes, so a row start is in general not even
    // 4-byte aligned: the range is walked in 4-element vectors from its first vector-aligned input address, the few elements in
    // front of and behind them one by one.  The gradient tile has its own base; where the two disagree its vectors are stored by
    // element.
    const bool square = gamma == 2.0f;
    const T *x_tile = logits + (long long)r * ld_logits + (long long)n0 * C;
    T *d_tile = dlogits + ((long long)r * N + n0) * C;
    const int elems = nq * C;
    float cls_a = 0.0f, cls_b = 0.0f;
    const auto element = [&](int e, float x) {
        const int q = e / C, c = e - q * C;
        const bool hot = s_lab[q] == c;
        const float t = hot ? s_iou[q] : 0.0f;
        float p, one_minus_p;
        sigmoid_pair(x, p, one_minus_p);
        const float w = hot ? t : (1.0f - alpha) * pow_gamma(p, gamma, square);
        const float loss = w * (fmaxf(x, 0.0f) - x * t + log1pf(expf(-fabsf(x))));
        const bool dn = n0 + q < n_split;
        cls_a += dn ? loss : 0.0f;
        cls_b += dn ? 0.0f : loss;
        return w * (p - t) * (dn ? inv_a : inv_b);
    };
    const int lead = (int)((kVec - (reinterpret_cast<uintptr_t>(x_tile) / sizeof(T)) % kVec) % kVec);
    const int head = min(elems, lead);
    const int vectors = (elems - head) / kVec;
    const int tail = head + vectors * kVec;
    const bool store_vectors = reinterpret_cast<uintptr_t>(d_tile + head) % (kVec * sizeof(T)) == 0;
    for (int i = tid; i < head + (elems - tail); i += kLossThreads) {
        const int e = i < head ? i : tail + (i - head);
        store_logit(d_tile + e, element(e, load_logit(x_tile + e)));
    }
    for (int v = tid; v < vectors; v += kLossThreads) {
        const int e = head + v * kVec;
        float x[kVec], d[kVec];
        load_logits(x_tile + e, x);
#pragma unroll
        for (int j = 0; j < kVec; ++j) d[j] = element(e + j, x[j]);
        if (store_vectors) {
            store_logits(d_tile + e, d);
        } else {
#pragma unroll
            for (int j = 0; j < kVec; ++j) store_logit(d_tile + e + j, d[j]);
        }
    }
    acc[0] = cls_a;
    acc[3] = cls_b;

    // workgroup sum in a fixed order: lanes by xor-shuffle, then the waves in turn
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float v = acc[k];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
        acc[k] = v;
    }
    if ((tid & (kWave - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_red[tid / kWave][k] = acc[k];
    }
    __syncthreads();
    if (tid < 6) {
        float v = 0.0f;
        for (int w = 0; w < kLossThreads / kWave; ++w) v += s_red[w][tid];
        partials[((long long)r * gridDim.x + blockIdx.x) * 6 + tid] = v * (tid < 3 ? inv_a : inv_b);
    }
}

// sums[r, :] = the row's partials added in workgroup order
__global__ __launch_bounds__(kWave) void set_loss_sum_kernel(const float *__restrict__ partials, int blocks, float *__restrict__ sums)
{
    const int r = blockIdx.x, k = threadIdx.x;
    if (k >= 6) return;
    float v = 0.0f;
    for (int i = 0; i < blocks; ++i) v += partials[((long long)r * blocks + i) * 6 + k];
    sums[(long long)r * 6 + k] = v;
}

long long set_loss_workspace(int R, int N)
{
    if (R <= 0 || N <= 0) return 0;
    return (long long)R * ((N + kLossQueries - 1) / kLossQueries) * 6 * (long long)sizeof(float);
}

template <typename T>
int set_loss(const T *logits, long long ld_logits, const float *boxes, long long ld_boxes, const int *match, const float *gt_boxes,
             const int *gt_labels, int R, int B, int N, int C, int Gmax, int n_split, float inv_a, float inv_b, float alpha,
             float gamma, void *ws, long long ws_bytes, float *sums, T *dlogits, float *dbox_l1, float *dbox_giou, void *stream)
{
    if (R < 0 || B <= 0 || N < 0 || C <= 0 || Gmax <= 0 || n_split < 0 || ws_bytes < 0) return RDETR_ERR_INVALID_ARG;
    if (R == 0) return RDETR_OK;
    if (!sums) return RDETR_ERR_INVALID_ARG;
    if (N == 0) {
        return hipMemsetAsync(sums, 0, (size_t)R * 6 * sizeof(float), static_cast<hipStream_t>(stream)) == hipSuccess ? RDETR_OK
                                                                                                                        : RDETR_ERR_LAUNCH;
    }
    if (!logits || !boxes || !match || !gt_boxes || !gt_labels || !ws || !dlogits || !dbox_l1 || !dbox_giou) return RDETR_ERR_INVALID_ARG;
    if (ld_logits < (long long)N * C || ld_boxes < (long long)N * 4 || ws_bytes < set_loss_workspace(R, N)) return RDETR_ERR_INVALID_ARG;
    if (R > 65535) return RDETR_ERR_UNSUPPORTED;
    if (!aligned_to(logits, sizeof(T)) || !aligned_to(dlogits, sizeof(T)) || !aligned_to(boxes, 16) || ld_boxes % 4 || !aligned_to(match, 4)
        || !aligned_to(gt_boxes, 4) || !aligned_to(gt_labels, 4) || !aligned_to(ws, 4) || !aligned_to(sums, 4) || !aligned_to(dbox_l1, 16)
        || !aligned_to(dbox_giou, 16))
        return RDETR_ERR_UNSUPPORTED;
    const int blocks = (N + kLossQueries - 1) / kLossQueries;
    hipLaunchKernelGGL(set_loss_kernel<T>, dim3((unsigned)blocks, (unsigned)R), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                       logits, ld_logits, boxes, ld_boxes, match, gt_boxes, gt_labels, B, N, C, Gmax, n_split, inv_a, inv_b, alpha, gamma,
                       static_cast<float *>(ws), dlogits, dbox_l1, dbox_giou);
    if (launch_status() != RDETR_OK) return RDETR_ERR_LAUNCH;
    hipLaunchKernelGGL(set_loss_sum_kernel, dim3((unsigned)R), dim3(kWave), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *>(ws), blocks, sums);
    return launch_status();
}

}  // namespace
}  // namespace rdetr

extern "C" {

int rdetr_match_cost_f32(const float *logits, long long ld_logits, const float *boxes, long long ld_boxes, const float *gt_boxes,
                         const int *gt_labels, const int *gt_count, int R, int B, int N, int C, int Gmax, float alpha, float gamma,
                         float w_class, float w_bbox, float w_giou, float *cost, void *stream)
{
    return rdetr::match_cost<float>(logits, ld_logits, boxes, ld_boxes, gt_boxes, gt_labels, gt_count, R, B, N, C, Gmax, alpha, gamma,
                                    w_class, w_bbox, w_giou, cost, stream);
}

int rdetr_match_cost_bf16(const uint16_t *logits, long long ld_logits, const float *boxes, long long ld_boxes, const float *gt_boxes,
                          const int *gt_labels, const int *gt_count, int R, int B, int N, int C, int Gmax, float alpha, float gamma,
                          float w_class, float w_bbox, float w_giou, float *cost, void *stream)
{
    return rdetr::match_cost<uint16_t>(logits, ld_logits, boxes, ld_boxes, gt_boxes, gt_labels, gt_count, R, B, N, C, Gmax, alpha, gamma,
                                       w_class, w_bbox, w_giou, cost, stream);
}

long long rdetr_set_loss_workspace_bytes(int R, int N) { return rdetr::set_loss_workspace(R, N); }

int rdetr_set_loss_f32(const float *logits, long long ld_logits, const float *boxes, long long ld_boxes, const int *match,
                       const float *gt_boxes, const int *gt_labels, int R, int B, int N, int C, int Gmax, int n_split, float inv_norm_a,
                       float inv_norm_b, float alpha, float gamma, void *ws, long long ws_bytes, float *sums, float *dlogits,
                       float *dbox_l1, float *dbox_giou, void *stream)
{
    return rdetr::set_loss<float>(logits, ld_logits, boxes, ld_boxes, match, gt_boxes, gt_labels, R, B, N, C, Gmax, n_split, inv_norm_a,
                                  inv_norm_b, alpha, gamma, ws, ws_bytes, sums, dlogits, dbox_l1, dbox_giou, stream);
}

int rdetr_set_loss_bf16(const uint16_t *logits, long long ld_logits, const float *boxes, long long ld_boxes, const int *match,
                        const float *gt_boxes, const int *gt_labels, int R, int B, int N, int C, int Gmax, int n_split, float inv_norm_a,
                        float inv_norm_b, float alpha, float gamma, void *ws, long long ws_bytes, float *sums, uint16_t *dlogits,
                        float *dbox_l1, float *dbox_giou, void *stream)
{
    return rdetr::set_loss<uint16_t>(logits, ld_logits, boxes, ld_boxes, match, gt_boxes, gt_labels, R, B, N, C, Gmax, n_split,
                                     inv_norm_a, inv_norm_b, alpha, gamma, ws, ws_bytes, sums, dlogits, dbox_l1, dbox_giou, stream);
}

}  // extern "C"
