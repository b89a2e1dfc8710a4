// Contrastive denoising query generator of Relation-DETR (models/bricks/denoising.py:180-331, GenerateCDNQueries):
//   rdetr_cdn_queries_*         noised label queries (an embedding gather), noised logit-space box queries and the noised labels of
//                               every slot of [B, Ndn], padding written as zeros, one launch;
//   rdetr_cdn_mask              the [T, T] visibility mask of the denoising groups, one launch;
//   rdetr_cdn_embed_backward_*  the gradient of the label embedding: per class the rows of its slots added in ascending order;
//   rdetr_cdn_noise             the four draws of a key, written out (the keyed path of rdetr_cdn_queries_* never stores them).
// Slot (b, j), i = j / max_gt, t = j % max_gt: padding when t >= G_b, else flat row r = i * G + off[b] + t of the reference's
// repeated ground truth, gt off[b] + t, copy i positive when even and negative when odd.  fp32 math in the reference's operation
// order (the build has -ffp-contract=off).
#include "cdn_noise.h"
#include "launch.h"

#include <math.h>

namespace rdetr {
namespace {

constexpr int kCdnThreads = 256;
constexpr int kCdnVecBytes = 16;               // every embedding row moves as 16-byte vectors
constexpr int kMaskPerThread = 4;              // mask bytes per lane, stored as one dword
constexpr float kSigmoidEps = 1e-3f;           // util/misc.py:31-35

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__device__ __forceinline__ float inverse_sigmoid(float x)
{
    x = clamp01(x);
    return logf(fmaxf(x, kSigmoidEps) / fmaxf(1.0f - x, kSigmoidEps));
}

template <typename T>
__global__ __launch_bounds__(kCdnThreads) void cdn_queries_kernel(
    const long long *__restrict__ gt_labels, const float *__restrict__ gt_boxes, const int *__restrict__ gt_offset, int B, int G, int max_gt,
    int groups, int C, int d, float label_noise_prob, float box_noise_scale, const T *__restrict__ embed,
    const float *__restrict__ label_u, const long long *__restrict__ label_r, const float *__restrict__ box_sign,
    const float *__restrict__ box_u, int keyed, unsigned long long key, T *__restrict__ label_query, float *__restrict__ box_query,
    int *__restrict__ noised_label)
{
    const int vecs = d / (kCdnVecBytes / (int)sizeof(T));                       // 16-byte vectors per embedding row
    const int n_dn = 2 * groups * max_gt;
    const long long idx = (long long)blockIdx.x * kCdnThreads + threadIdx.x;
    const long long slot = idx / vecs;
    if (slot >= (long long)B * n_dn) return;
    const int v = (int)(idx - slot * vecs);
    const int b = (int)(slot / n_dn), j = (int)(slot - (long long)b * n_dn);
    const int i = j / max_gt, t = j - i * max_gt;
    const int off = gt_offset[b], count = gt_offset[b + 1] - off;
    const bool real = t < count && off >= 0 && off + t < G;                     // a bad offset table makes padding, never an index
    const int g = off + t;

    CdnDraws draw = {};
    if (real && keyed) draw = cdn_draws(key, (uint32_t)((long long)i * G + g), C);

    long long label = -1;
    if (real) {
        label = gt_labels[g];
        if (label_noise_prob > 0.0f) {
            const long long r = (long long)i * G + g;
            const float u = keyed ? draw.label_u : label_u[r];
            const long long other = keyed ? (long long)draw.label_r : label_r[r];
            label = u < label_noise_prob * 0.5f ? other : label;
        }
        if (label < 0 || label >= C) label = -1;                                 // never an index: a zero row
    }
    u32x4 row = {0u, 0u, 0u, 0u};
    if (label >= 0) row = reinterpret_cast<const u32x4 *>(embed + label * d)[v];
    reinterpret_cast<u32x4 *>(label_query + slot * d)[v] = row;
    if (v != 0) return;

    noised_label[slot] = (int)label;
    f32x4 out = {0.0f, 0.0f, 0.0f, 0.0f};
    if (real) {
        const f32x4 gt = *reinterpret_cast<const f32x4 *>(gt_boxes + (long long)g * 4);
        float q[4] = {gt.x, gt.y, gt.z, gt.w};                                  // cx, cy, w, h
        if (box_noise_scale > 0.0f) {
            float sign[4], u[4];
            if (keyed) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sign[k] = draw.box_sign[k], u[k] = draw.box_u[k];
            } else {
                const long long r = (long long)i * G + g;
                const f32x4 s = *reinterpret_cast<const f32x4 *>(box_sign + r * 4), w = *reinterpret_cast<const f32x4 *>(box_u + r * 4);
                sign[0] = s.x, sign[1] = s.y, sign[2] = s.z, sign[3] = s.w;
                u[0] = w.x, u[1] = w.y, u[2] = w.z, u[3] = w.w;
            }
            const float shift = (i & 1) ? 1.0f : 0.0f;                           // the negative copies: noise in [1, 2)
            const float diff[4] = {gt.z / 2.0f, gt.w / 2.0f, gt.z / 2.0f, gt.w / 2.0f};
            float xyxy[4] = {gt.x - 0.5f * gt.z, gt.y - 0.5f * gt.w, gt.x + 0.5f * gt.z, gt.y + 0.5f * gt.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float part = (u[k] + shift) * (sign[k] * 2.0f - 1.0f);
                xyxy[k] = clamp01(xyxy[k] + (part * diff[k]) * box_noise_scale);
            }
            q[0] = (xyxy[0] + xyxy[2]) / 2.0f, q[1] = (xyxy[1] + xyxy[3]) / 2.0f;
            q[2] = xyxy[2] - xyxy[0], q[3] = xyxy[3] - xyxy[1];                 // may be negative on a negative copy: the clamps decide
        }
        out = f32x4{inverse_sigmoid(q[0]), inverse_sigmoid(q[1]), inverse_sigmoid(q[2]), inverse_sigmoid(q[3])};
    }
    *reinterpret_cast<f32x4 *>(box_query + slot * 4) = out;
}

template <typename T>
int cdn_queries(const long long *gt_labels, const float *gt_boxes, const int *gt_offset, int B, int G, int max_gt, int groups, int C,
                int d, float label_noise_prob, float box_noise_scale, const T *embed, const float *label_u, const long long *label_r,
                const float *box_sign, const float *box_u, int keyed, unsigned long long key, T *label_query, float *box_query,
                int *noised_label, void *stream)
{
    if (B <= 0 || G < 0 || max_gt < 0 || max_gt > G || groups < 1 || C <= 0 || d <= 0) return RDETR_ERR_INVALID_ARG;
    if (max_gt == 0) return RDETR_OK;                                            // no slot at all: nothing to write
    if (!gt_labels || !gt_boxes || !gt_offset || !embed || !label_query || !box_query || !noised_label) return RDETR_ERR_INVALID_ARG;
    const bool need_label = label_noise_prob > 0.0f, need_box = box_noise_scale > 0.0f;
    if (!keyed && ((need_label && (!label_u || !label_r)) || (need_box && (!box_sign || !box_u)))) return RDETR_ERR_INVALID_ARG;
    const int per_vec = kCdnVecBytes / (int)sizeof(T);
    if (d % per_vec) return RDETR_ERR_UNSUPPORTED;
    const long long n_dn = 2LL * groups * max_gt, flat_rows = 2LL * groups * G;
    if (n_dn > 0x7fffffffLL || flat_rows > 0x7fffffffLL || (long long)B * n_dn > 0x7fffffffLL) return RDETR_ERR_UNSUPPORTED;
    if (!aligned_to(embed, 16) || !aligned_to(label_query, 16) || !aligned_to(gt_boxes, 16) || !aligned_to(box_query, 16)
        || !aligned_to(gt_labels, 8) || !aligned_to(gt_offset, 4) || !aligned_to(noised_label, 4))
        return RDETR_ERR_UNSUPPORTED;
    if (!keyed && ((need_label && (!aligned_to(label_u, 4) || !aligned_to(label_r, 8)))
                   || (need_box && (!aligned_to(box_sign, 16) || !aligned_to(box_u, 16)))))
        return RDETR_ERR_UNSUPPORTED;
    const long long work = (long long)B * n_dn * (d / per_vec);
    const long long blocks = (work + kCdnThreads - 1) / kCdnThreads;
    if (!grid_fits(blocks)) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cdn_queries_kernel<T>, dim3((unsigned)blocks), dim3(kCdnThreads), 0, static_cast<hipStream_t>(stream), gt_labels,
                       gt_boxes, gt_offset, B, G, max_gt, groups, C, d, label_noise_prob, box_noise_scale, embed, label_u, label_r, box_sign,
                       box_u, keyed, key, label_query, box_query, noised_label);
    return launch_status();
}

// ------------------------------------------------------------------------------------------------------------------------- mask
__global__ __launch_bounds__(kCdnThreads) void cdn_mask_kernel(int n_dn, int group_size, int T, unsigned char *__restrict__ mask)
{
    const long long total = (long long)T * T;
    const long long e0 = ((long long)blockIdx.x * kCdnThreads + threadIdx.x) * kMaskPerThread;
    if (e0 >= total) return;
    unsigned int packed = 0u;
#pragma unroll
    for (int k = 0; k < kMaskPerThread; ++k) {
        const long long e = e0 + k;
        if (e >= total) break;
        const int r = (int)(e / T), c = (int)(e - (long long)r * T);
        // a column of the denoising part is hidden from the matching queries and from every other group
        const bool hidden = c < n_dn && (r >= n_dn || r / group_size != c / group_size);
        packed |= (hidden ? 1u : 0u) << (8 * k);
    }
    if (e0 + kMaskPerThread <= total) {
        *reinterpret_cast<unsigned int *>(mask + e0) = packed;
    } else {
        for (int k = 0; e0 + k < total; ++k) mask[e0 + k] = (unsigned char)((packed >> (8 * k)) & 0xffu);
    }
}

int cdn_mask(int groups, int group_size, int num_queries, unsigned char *mask, void *stream)
{
    if (groups < 1 || group_size < 0 || num_queries < 0) return RDETR_ERR_INVALID_ARG;
    const long long n_dn = (long long)groups * group_size, T = n_dn + num_queries;
    if (T == 0) return RDETR_OK;
    if (!mask) return RDETR_ERR_INVALID_ARG;
    if (T > 46340) return RDETR_ERR_UNSUPPORTED;                                 // T * T stays below 2^31
    if (!aligned_to(mask, 4)) return RDETR_ERR_UNSUPPORTED;
    const long long per_block = (long long)kCdnThreads * kMaskPerThread;
    const long long blocks = (T * T + per_block - 1) / per_block;
    hipLaunchKernelGGL(cdn_mask_kernel, dim3((unsigned)blocks), dim3(kCdnThreads), 0, static_cast<hipStream_t>(stream), (int)n_dn,
                       group_size > 0 ? group_size : 1, (int)T, mask);
    return launch_status();
}

// ----------------------------------------------------------------------------------------------------- label embedding gradient
// One wave per (class, 64 vectors of the row): the slots' labels are walked in ascending order, the address uniform over the wave,
// and the rows of this class added into a compensated fp32 accumulator -- a fixed order, so the same bits on every run; the
// compensation keeps an element whose rows cancel as accurate as one whose rows do not (up to 200 rows meet in one class).
constexpr int kGradThreads = kWave;
constexpr int kGradVec = 4;                    // columns per lane

__device__ __forceinline__ void load_grad(const float *p, float (&x)[kGradVec])
{
    const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
__device__ __forceinline__ void load_grad(const uint16_t *p, float (&x)[kGradVec])
{
    const u32x2 v = *reinterpret_cast<const u32x2 *>(p);
    x[0] = bf16_bits_to_f32(v.x & 0xffffu), x[1] = bf16_bits_to_f32(v.x >> 16);
    x[2] = bf16_bits_to_f32(v.y & 0xffffu), x[3] = bf16_bits_to_f32(v.y >> 16);
}
__device__ __forceinline__ void store_grad(float *p, const float (&a)[kGradVec])
{
    *reinterpret_cast<f32x4 *>(p) = f32x4{a[0], a[1], a[2], a[3]};
}
__device__ __forceinline__ void store_grad(uint16_t *p, const float (&a)[kGradVec])
{
    *reinterpret_cast<u32x2 *>(p) = u32x2{pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3])};
}

template <typename T>
__global__ __launch_bounds__(kGradThreads) void cdn_embed_backward_kernel(const T *__restrict__ grad_label_query,
                                                                          const int *__restrict__ noised_label, int rows, int d,
                                                                          T *__restrict__ grad_embed)
{
    const int c = blockIdx.x;
    const int col = (blockIdx.y * kGradThreads + threadIdx.x) * kGradVec;
    if (col >= d) return;
    float acc[kGradVec] = {0.0f, 0.0f, 0.0f, 0.0f}, lost[kGradVec] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int row = 0; row < rows; ++row) {
        if (noised_label[row] != c) continue;
        float x[kGradVec];
        load_grad(grad_label_query + (long long)row * d + col, x);
#pragma unroll
        for (int k = 0; k < kGradVec; ++k) {                                     // Kahan: `lost` carries what the last add rounded away
            const float y = x[k] - lost[k], t = acc[k] + y;
            lost[k] = (t - acc[k]) - y;
            acc[k] = t;
        }
    }
    store_grad(grad_embed + (long long)c * d + col, acc);
}

template <typename T>
int cdn_embed_backward(const T *grad_label_query, const int *noised_label, int rows, int C, int d, T *grad_embed, void *stream)
{
    if (rows < 0 || C <= 0 || d <= 0 || !grad_embed) return RDETR_ERR_INVALID_ARG;
    if (rows > 0 && (!grad_label_query || !noised_label)) return RDETR_ERR_INVALID_ARG;
    if (d % (kCdnVecBytes / (int)sizeof(T))) return RDETR_ERR_UNSUPPORTED;
    if (!aligned_to(grad_embed, 16) || (rows > 0 && (!aligned_to(grad_label_query, 16) || !aligned_to(noised_label, 4))))
        return RDETR_ERR_UNSUPPORTED;
    const int per_block = kGradThreads * kGradVec;
    const int chunks = (d + per_block - 1) / per_block;
    if (chunks > 65535) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cdn_embed_backward_kernel<T>, dim3((unsigned)C, (unsigned)chunks), dim3(kGradThreads), 0,
                       static_cast<hipStream_t>(stream), grad_label_query, noised_label, rows, d, grad_embed);
    return launch_status();
}

// ------------------------------------------------------------------------------------------------------------------------ noise
__global__ __launch_bounds__(kCdnThreads) void cdn_noise_kernel(unsigned long long key, int Q, int C, float *__restrict__ label_u,
                                                                long long *__restrict__ label_r, float *__restrict__ box_sign,
                                                                float *__restrict__ box_u)
{
    const long long r = (long long)blockIdx.x * kCdnThreads + threadIdx.x;
    if (r >= Q) return;
    const CdnDraws draw = cdn_draws(key, (uint32_t)r, C);
    label_u[r] = draw.label_u;
    label_r[r] = draw.label_r;
    *reinterpret_cast<f32x4 *>(box_sign + r * 4) = f32x4{draw.box_sign[0], draw.box_sign[1], draw.box_sign[2], draw.box_sign[3]};
    *reinterpret_cast<f32x4 *>(box_u + r * 4) = f32x4{draw.box_u[0], draw.box_u[1], draw.box_u[2], draw.box_u[3]};
}

int cdn_noise(unsigned long long key, int Q, int C, float *label_u, long long *label_r, float *box_sign, float *box_u, void *stream)
{
    if (Q < 0 || C <= 0) return RDETR_ERR_INVALID_ARG;
    if (Q == 0) return RDETR_OK;
    if (!label_u || !label_r || !box_sign || !box_u) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(label_u, 4) || !aligned_to(label_r, 8) || !aligned_to(box_sign, 16) || !aligned_to(box_u, 16)) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cdn_noise_kernel, dim3((unsigned)((Q + kCdnThreads - 1) / kCdnThreads)), dim3(kCdnThreads), 0,
                       static_cast<hipStream_t>(stream), key, Q, C, label_u, label_r, box_sign, box_u);
    return launch_status();
}

}  // namespace
}  // namespace rdetr

extern "C" {

int rdetr_cdn_queries_f32(const long long *gt_labels, const float *gt_boxes, const int *gt_offset, int B, int G, int max_gt, int groups,
                          int C, int d, float label_noise_prob, float box_noise_scale, const float *embed, const float *label_u,
                          const long long *label_r, const float *box_sign, const float *box_u, int keyed, unsigned long long key,
                          float *label_query, float *box_query, int *noised_label, void *stream)
{
    return rdetr::cdn_queries<float>(gt_labels, gt_boxes, gt_offset, B, G, max_gt, groups, C, d, label_noise_prob, box_noise_scale, embed,
                                     label_u, label_r, box_sign, box_u, keyed, key, label_query, box_query, noised_label, stream);
}

int rdetr_cdn_queries_bf16(const long long *gt_labels, const float *gt_boxes, const int *gt_offset, int B, int G, int max_gt, int groups,
                           int C, int d, float label_noise_prob, float box_noise_scale, const uint16_t *embed, const float *label_u,
                           const long long *label_r, const float *box_sign, const float *box_u, int keyed, unsigned long long key,
                           uint16_t *label_query, float *box_query, int *noised_label, void *stream)
{
    return rdetr::cdn_queries<uint16_t>(gt_labels, gt_boxes, gt_offset, B, G, max_gt, groups, C, d, label_noise_prob, box_noise_scale, embed,
                                        label_u, label_r, box_sign, box_u, keyed, key, label_query, box_query, noised_label, stream);
}

int rdetr_cdn_mask(int groups, int group_size, int num_queries, unsigned char *mask, void *stream)
{
    return rdetr::cdn_mask(groups, group_size, num_queries, mask, stream);
}

int rdetr_cdn_embed_backward_f32(const float *grad_label_query, const int *noised_label, int rows, int C, int d, float *grad_embed,
                                 void *stream)
{
    return rdetr::cdn_embed_backward<float>(grad_label_query, noised_label, rows, C, d, grad_embed, stream);
}

int rdetr_cdn_embed_backward_bf16(const uint16_t *grad_label_query, const int *noised_label, int rows, int C, int d, uint16_t *grad_embed,
                                  void *stream)
{
    return rdetr::cdn_embed_backward<uint16_t>(grad_label_query, noised_label, rows, C, d, grad_embed, stream);
}

int rdetr_cdn_noise(unsigned long long key, int Q, int C, float *label_u, long long *label_r, float *box_sign, float *box_u, void *stream)
{
    return rdetr::cdn_noise(key, Q, C, label_u, label_r, box_sign, box_u, stream);
}

}  // extern "C"
