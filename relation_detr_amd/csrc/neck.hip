// The neck's GroupNorm over a whole pyramid, the per-level padding masks and the sine position encoding
// (models/necks/channel_mapper.py, models/detectors/base_detector.py:153-165, models/bricks/position_encoding.py:9-68).
//
// GroupNorm, forward, two launches whatever the level count:
//   gn_moments_kernel     one workgroup per kGnChunk elements of one (level, image, group): the chunk's (count, mean, M2), mean first
//                         and M2 about it, written with plain stores
//   gn_normalize_kernel   prologue: the group's triples combined in index order with Chan's formula; then y, and mean / rstd
// GroupNorm, backward, two launches:
//   gn_bwd_partial_kernel per (level, image, channel, chunk of the channel's pixels): sum dy and sum dy * xhat
//   gn_bwd_dx_kernel      per chunk of a group: s1, s2 from the partials in index order, then dx; the workgroups behind them
//                         add the same partials over chunks, then images, into dgamma / dbeta
// A workgroup owns its chunk whatever the grid, every sum has a fixed order and nothing is handed over inside a launch, so the
// bits repeat from run to run.  The level tables travel in the kernels' argument blocks, as in glue.hip.
//
// Masks: torch's nearest rule src = min(floor(dst * (float(in) / float(out))), in - 1) on the image mask, the inclusive count of
// valid pixels down each column (one lane per column) and along each row (one wave per row, ballot + popcount).
// Position encoding: one lane per (pixel, frequency) writes the sin and the cos channel; every step is one fp32 IEEE operation in
// the reference's order and dim_t comes from the caller, because a padded column's argument is about -3e6 rad and one ulp of dim_t
// moves it by 0.2 rad.
#include "launch.h"

namespace rdetr {
namespace {

constexpr int kGnThreads = 256;
constexpr int kGnPer = 16;                          // elements per lane
constexpr int kGnChunk = kGnThreads * kGnPer;       // elements of one chunk
constexpr int kMaxLevels = 8;
constexpr int kMaxGroupChannels = 16;

struct GnLevels {
    const void *x[kMaxLevels];                      // [B, C, hw]
    const void *dy[kMaxLevels];                     // backward only
    void *y[kMaxLevels];                            // forward: y, backward: dx
    const void *gamma[kMaxLevels], *beta[kMaxLevels];
    int hw[kMaxLevels];
    int gchunks[kMaxLevels], gblock0[kMaxLevels + 1];   // chunks per group, prefix of B * G * gchunks
    int cchunks[kMaxLevels], cblock0[kMaxLevels + 1];   // chunks per channel, prefix of B * C * cchunks
};

template <typename T> __device__ __forceinline__ float load_as_f32(const T *p, long long i);
template <> __device__ __forceinline__ float load_as_f32<float>(const float *p, long long i) { return p[i]; }
template <> __device__ __forceinline__ float load_as_f32<unsigned short>(const unsigned short *p, long long i)
{
    return bf16_bits_to_f32(p[i]);
}
__device__ __forceinline__ void store_from_f32(float *p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void store_from_f32(unsigned short *p, long long i, float v) { p[i] = (unsigned short)f32_to_bf16_bits(v); }

__device__ __forceinline__ float load_param(const void *p, int i, int is_bf16)
{
    return is_bf16 ? bf16_bits_to_f32(static_cast<const unsigned short *>(p)[i]) : static_cast<const float *>(p)[i];
}

// the sum over the workgroup, the same value in every lane: lanes by shuffle, the four waves in a fixed tree
__device__ __forceinline__ float block_sum(float v, float *s_red)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    __syncthreads();                                // s_red may still be read from the previous sum
    if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__device__ __forceinline__ int level_of(const int *block0, int L, int bid)
{
    int l = 0;
    while (l + 1 < L && bid >= block0[l + 1]) ++l;  // uniform over the workgroup
    return l;
}

struct Moments {
    float n, mean, m2;
};

// Chan's combination of a group's chunk triples, in index order
__device__ __forceinline__ Moments combine_chunks(const float *__restrict__ triples, int chunks)
{
    Moments a = {triples[0], triples[1], triples[2]};
    for (int j = 1; j < chunks; ++j) {
        const float nb = triples[3 * j], mb = triples[3 * j + 1], m2b = triples[3 * j + 2];
        const float n = a.n + nb, delta = mb - a.mean;
        a.mean = a.mean + delta * (nb / n);
        a.m2 = (a.m2 + m2b) + (delta * delta) * (a.n * (nb / n));
        a.n = n;
    }
    return a;
}

template <typename T>
__global__ __launch_bounds__(kGnThreads) void gn_moments_kernel(GnLevels lv, int L, int group_channels, float *__restrict__ ws)
{
    __shared__ float s_red[kGnThreads / kWave];
    const int bid = blockIdx.x, tid = threadIdx.x;
    const int l = level_of(lv.gblock0, L, bid);
    const int local = bid - lv.gblock0[l];
    const int chunks = lv.gchunks[l], bg = local / chunks, ck = local % chunks;
    const int n = group_channels * lv.hw[l], first = ck * kGnChunk;
    const int cnt = min(kGnChunk, n - first);
    const T *x = static_cast<const T *>(lv.x[l]) + (long long)bg * n + first;
    float v[kGnPer], sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kGnPer; ++k) {
        const int i = tid + k * kGnThreads;
        v[k] = i < cnt ? load_as_f32(x, i) : 0.0f;
        sum += v[k];
    }
    const float mean = block_sum(sum, s_red) / (float)cnt;
    float m2 = 0.0f;
#pragma unroll
    for (int k = 0; k < kGnPer; ++k) {
        const float d = v[k] - mean;
        if (tid + k * kGnThreads < cnt) m2 += d * d;
    }
    m2 = block_sum(m2, s_red);
    if (tid == 0) {
        ws[3 * (long long)bid] = (float)cnt;
        ws[3 * (long long)bid + 1] = mean;
        ws[3 * (long long)bid + 2] = m2;
    }
}

template <typename T>
__global__ __launch_bounds__(kGnThreads) void gn_normalize_kernel(GnLevels lv, int L, int BG, int G, int group_channels, float eps, int params_bf16,
                                                                  const float *__restrict__ ws, float *__restrict__ mean_out,
                                                                  float *__restrict__ rstd_out)
{
    const int bid = blockIdx.x, tid = threadIdx.x;
    const int l = level_of(lv.gblock0, L, bid);
    const int local = bid - lv.gblock0[l];
    const int chunks = lv.gchunks[l], bg = local / chunks, ck = local % chunks;
    const int hw = lv.hw[l], n = group_channels * hw, first = ck * kGnChunk;
    const int cnt = min(kGnChunk, n - first);
    const Moments m = combine_chunks(ws + 3 * ((long long)lv.gblock0[l] + (long long)bg * chunks), chunks);
    const float mean = m.mean, rstd = 1.0f / sqrtf(m.m2 / m.n + eps);
    if (ck == 0 && tid == 0) {
        mean_out[(long long)l * BG + bg] = mean;
        rstd_out[(long long)l * BG + bg] = rstd;
    }
    const int c0 = (bg % G) * group_channels;
    const T *x = static_cast<const T *>(lv.x[l]) + (long long)bg * n + first;
    T *y = static_cast<T *>(lv.y[l]) + (long long)bg * n + first;
#pragma unroll 4
    for (int k = 0; k < kGnPer; ++k) {
        const int i = tid + k * kGnThreads;
        if (i >= cnt) break;
        const int c = c0 + (first + i) / hw;
        const float g = load_param(lv.gamma[l], c, params_bf16), b = load_param(lv.beta[l], c, params_bf16);
        store_from_f32(y, i, (load_as_f32(x, i) - mean) * rstd * g + b);
    }
}

template <typename T>
__global__ __launch_bounds__(kGnThreads) void gn_bwd_partial_kernel(GnLevels lv, int L, int C, int G, int B,
                                                                    const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                    float *__restrict__ ws)
{
    __shared__ float s_red[kGnThreads / kWave];
    const int bid = blockIdx.x, tid = threadIdx.x;
    const int l = level_of(lv.cblock0, L, bid);
    const int local = bid - lv.cblock0[l];
    const int chunks = lv.cchunks[l], bc = local / chunks, ck = local % chunks;
    const int hw = lv.hw[l], first = ck * kGnChunk;
    const int cnt = min(kGnChunk, hw - first);
    const int b = bc / C, g = (bc % C) / (C / G);
    const float mu = mean[((long long)l * B + b) * G + g], rs = rstd[((long long)l * B + b) * G + g];
    const T *x = static_cast<const T *>(lv.x[l]) + (long long)bc * hw + first;
    const T *dy = static_cast<const T *>(lv.dy[l]) + (long long)bc * hw + first;
    float a1 = 0.0f, a2 = 0.0f;
#pragma unroll 4
    for (int k = 0; k < kGnPer; ++k) {
        const int i = tid + k * kGnThreads;
        if (i >= cnt) break;
        const float d = load_as_f32(dy, i), xh = (load_as_f32(x, i) - mu) * rs;
        a1 += d;
        a2 += d * xh;
    }
    a1 = block_sum(a1, s_red);
    a2 = block_sum(a2, s_red);
    if (tid == 0) {
        ws[2 * (long long)bid] = a1;
        ws[2 * (long long)bid + 1] = a2;
    }
}

template <typename T>
__global__ __launch_bounds__(kGnThreads) void gn_bwd_dx_kernel(GnLevels lv, int L, int C, int G, int B, int params_bf16, int dx_blocks,
                                                               const float *__restrict__ mean, const float *__restrict__ rstd,
                                                               const float *__restrict__ ws, float *__restrict__ dgamma,
                                                               float *__restrict__ dbeta)
{
    __shared__ float s_c1[kMaxGroupChannels], s_c2[kMaxGroupChannels];
    const int bid = blockIdx.x, tid = threadIdx.x;
    if (bid >= dx_blocks) {                          // the parameter gradients: one lane per (level, channel)
        const int t = (bid - dx_blocks) * kGnThreads + tid;
        if (t >= L * C) return;
        const int l = t / C, c = t % C, chunks = lv.cchunks[l];
        float db = 0.0f, dg = 0.0f;
        for (int b = 0; b < B; ++b) {
            const float *p = ws + 2 * ((long long)lv.cblock0[l] + ((long long)b * C + c) * chunks);
            float b1 = 0.0f, b2 = 0.0f;
            for (int j = 0; j < chunks; ++j) {
                b1 += p[2 * j];
                b2 += p[2 * j + 1];
            }
            db += b1;
            dg += b2;
        }
        dbeta[t] = db;
        dgamma[t] = dg;
        return;
    }
    const int l = level_of(lv.gblock0, L, bid);
    const int local = bid - lv.gblock0[l];
    const int chunks = lv.gchunks[l], bg = local / chunks, ck = local % chunks;
    const int gc = C / G, hw = lv.hw[l], n = gc * hw, first = ck * kGnChunk;
    const int cnt = min(kGnChunk, n - first);
    const int b = bg / G, c0 = (bg % G) * gc;
    if (tid < gc) {
        const int cchunks = lv.cchunks[l];
        const float *p = ws + 2 * ((long long)lv.cblock0[l] + ((long long)b * C + c0 + tid) * cchunks);
        float b1 = 0.0f, b2 = 0.0f;
        for (int j = 0; j < cchunks; ++j) {
            b1 += p[2 * j];
            b2 += p[2 * j + 1];
        }
        const float g = load_param(lv.gamma[l], c0 + tid, params_bf16);
        s_c1[tid] = g * b1;
        s_c2[tid] = g * b2;
    }
    __syncthreads();
    float s1 = 0.0f, s2 = 0.0f;
    for (int t = 0; t < gc; ++t) {
        s1 += s_c1[t];
        s2 += s_c2[t];
    }
    const float mu = mean[(long long)l * B * G + bg], rs = rstd[(long long)l * B * G + bg], inv_n = 1.0f / (float)n;
    const T *x = static_cast<const T *>(lv.x[l]) + (long long)bg * n + first;
    const T *dy = static_cast<const T *>(lv.dy[l]) + (long long)bg * n + first;
    T *dx = static_cast<T *>(lv.y[l]) + (long long)bg * n + first;
#pragma unroll 4
    for (int k = 0; k < kGnPer; ++k) {
        const int i = tid + k * kGnThreads;
        if (i >= cnt) break;
        const float g = load_param(lv.gamma[l], c0 + (first + i) / hw, params_bf16);
        const float xh = (load_as_f32(x, i) - mu) * rs;
        store_from_f32(dx, i, rs * (load_as_f32(dy, i) * g - (s1 + xh * s2) * inv_n));
    }
}

// ------------------------------------------------------------------------------------------------------------ masks and position
struct PyrOut {
    void *out[kMaxLevels];                           // masks: u8 [B, h, w]; position: [B, 2F, h, w]
    int h[kMaxLevels], w[kMaxLevels];
    long long off[kMaxLevels];                       // the level's first element in the packed count buffers: B * (pixels before it)
    int tiles[kMaxLevels], block0[kMaxLevels + 1];   // position only: 256-pixel tiles per plane, prefix of B * F * tiles
};

template <typename M>
__global__ __launch_bounds__(256) void pyramid_masks_kernel(const M *__restrict__ src, int H, int W, PyrOut lv, long long total,
                                                            int *__restrict__ cum)
{
    const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int h = lv.h[l], w = lv.w[l];
    const float sh = (float)H / (float)h, sw = (float)W / (float)w;
    const M *m = src + (long long)b * H * W;
    auto padded = [&](int y, int x) {
        const int sy = min((int)floorf((float)y * sh), H - 1), sx = min((int)floorf((float)x * sw), W - 1);
        return m[(long long)sy * W + sx] != (M)0;
    };
    int *cy = cum + lv.off[l] + (long long)b * h * w, *cx = cy + total;
    if (blockIdx.z == 0) {                           // the mask and the counts down the columns
        unsigned char *out = static_cast<unsigned char *>(lv.out[l]) + (long long)b * h * w;
        for (int x = tid; x < w; x += 256) {
            int run = 0;
            for (int y = 0; y < h; ++y) {
                const bool p = padded(y, x);
                out[y * w + x] = p ? 1 : 0;
                run += p ? 0 : 1;
                cy[y * w + x] = run;
            }
        }
    } else {                                         // the counts along the rows: a wave per row
        const int lane = tid & (kWave - 1);
        for (int y = tid / kWave; y < h; y += 256 / kWave) {
            int carry = 0;
            for (int x0 = 0; x0 < w; x0 += kWave) {
                const int x = x0 + lane;
                const bool valid = x < w && !padded(y, x);
                const unsigned long long bal = __ballot(valid);
                if (x < w) cx[y * w + x] = carry + __popcll(bal & (~0ull >> (kWave - 1 - lane)));
                carry += __popcll(bal);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pyramid_sine_pos_kernel(const int *__restrict__ cum, long long total, PyrOut lv, int L, int F,
                                                               const float *__restrict__ dim_t, int normalize, float scale, float eps,
                                                               float offset)
{
    const int bid = blockIdx.x;
    const int l = level_of(lv.block0, L, bid);
    const int local = bid - lv.block0[l];
    const int tiles = lv.tiles[l], tile = local % tiles, j = (local / tiles) % F, b = local / (tiles * F);
    const int h = lv.h[l], w = lv.w[l], hw = h * w;
    const int p = tile * 256 + (int)threadIdx.x;
    if (p >= hw) return;
    const int half = j >= F / 2 ? 1 : 0, k = j - half * (F / 2);
    const int y = p / w, x = p - y * w;
    const int *base = cum + lv.off[l] + (long long)b * hw + (half ? total : 0);
    float e = (float)base[p] + offset;
    if (normalize) {
        const int last = half ? base[y * w + (w - 1)] : base[(h - 1) * w + x];
        e = e / ((float)last + eps) * scale;
    }
    const float a = e / dim_t[k];
    float s, c;
    sincosf(a, &s, &c);
    T *out = static_cast<T *>(lv.out[l]) + ((long long)b * 2 * F + (long long)half * F + 2 * k) * hw;
    store_from_f32(out, p, s);
    store_from_f32(out, (long long)hw + p, c);
}

// fills the group / channel chunk tables; RDETR_OK or the refusal
int gn_levels(const int *level_hw, int L, int B, int C, int G, GnLevels *lv, long long *fwd_blocks, long long *bwd_blocks)
{
    if (!level_hw || L <= 0 || B <= 0 || C <= 0 || G <= 0) return RDETR_ERR_INVALID_ARG;
    if (L > kMaxLevels || C % G || C / G > kMaxGroupChannels || B > 65535) return RDETR_ERR_UNSUPPORTED;
    long long gb = 0, cb = 0;
    for (int l = 0; l < L; ++l) {
        const long long h = level_hw[2 * l], w = level_hw[2 * l + 1];
        if (h <= 0 || w <= 0) return RDETR_ERR_INVALID_ARG;
        if (h * w * (C / G) > (1ll << 30)) return RDETR_ERR_UNSUPPORTED;
        const long long hw = h * w, n = hw * (C / G);
        lv->hw[l] = (int)hw;
        lv->gchunks[l] = (int)((n + kGnChunk - 1) / kGnChunk);
        lv->cchunks[l] = (int)((hw + kGnChunk - 1) / kGnChunk);
        lv->gblock0[l] = (int)gb;
        lv->cblock0[l] = (int)cb;
        gb += (long long)B * G * lv->gchunks[l];
        cb += (long long)B * C * lv->cchunks[l];
        if (gb > (1ll << 30) || cb > (1ll << 30)) return RDETR_ERR_UNSUPPORTED;
    }
    for (int l = L; l <= kMaxLevels; ++l) {
        lv->gblock0[l] = (int)gb;
        lv->cblock0[l] = (int)cb;
    }
    *fwd_blocks = gb;
    *bwd_blocks = cb;
    return RDETR_OK;
}

long long neck_workspace(long long fwd_blocks, long long bwd_blocks)
{
    const long long a = 3 * fwd_blocks, b = 2 * bwd_blocks;
    return (a > b ? a : b) * (long long)sizeof(float);
}

template <typename T>
int group_norm_levels(const void *const *x, const void *const *gamma, const void *const *beta, const int *level_hw, int L, int B, int C,
                      int G, float eps, int params_bf16, void *ws, long long ws_bytes, void *const *y, float *mean, float *rstd,
                      void *stream)
{
    GnLevels lv = {};
    long long fb = 0, bb = 0;
    const int st = gn_levels(level_hw, L, B, C, G, &lv, &fb, &bb);
    if (st != RDETR_OK) return st;
    if (!x || !gamma || !beta || !y || !mean || !rstd || !ws || ws_bytes < neck_workspace(fb, bb)) return RDETR_ERR_INVALID_ARG;
    if (!(eps > 0.0f) || (params_bf16 != 0 && params_bf16 != 1)) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(ws, 4) || !aligned_to(mean, 4) || !aligned_to(rstd, 4)) return RDETR_ERR_UNSUPPORTED;
    for (int l = 0; l < L; ++l) {
        if (!x[l] || !gamma[l] || !beta[l] || !y[l]) return RDETR_ERR_INVALID_ARG;
        const unsigned pa = params_bf16 ? 2 : 4;
        if (!aligned_to(x[l], sizeof(T)) || !aligned_to(y[l], sizeof(T)) || !aligned_to(gamma[l], pa) || !aligned_to(beta[l], pa))
            return RDETR_ERR_UNSUPPORTED;
        lv.x[l] = x[l];
        lv.y[l] = y[l];
        lv.gamma[l] = gamma[l];
        lv.beta[l] = beta[l];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gn_moments_kernel<T>, dim3((unsigned)fb), dim3(kGnThreads), 0, s, lv, L, C / G, static_cast<float *>(ws));
    hipLaunchKernelGGL(gn_normalize_kernel<T>, dim3((unsigned)fb), dim3(kGnThreads), 0, s, lv, L, B * G, G, C / G, eps, params_bf16,
                       static_cast<const float *>(ws), mean, rstd);
    return launch_status();
}

template <typename T>
int group_norm_levels_backward(const void *const *dy, const void *const *x, const void *const *gamma, const float *mean, const float *rstd,
                               const int *level_hw, int L, int B, int C, int G, int params_bf16, void *ws, long long ws_bytes,
                               void *const *dx, float *dgamma, float *dbeta, void *stream)
{
    GnLevels lv = {};
    long long fb = 0, bb = 0;
    const int st = gn_levels(level_hw, L, B, C, G, &lv, &fb, &bb);
    if (st != RDETR_OK) return st;
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || !ws || ws_bytes < neck_workspace(fb, bb))
        return RDETR_ERR_INVALID_ARG;
    if (params_bf16 != 0 && params_bf16 != 1) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(ws, 4) || !aligned_to(mean, 4) || !aligned_to(rstd, 4) || !aligned_to(dgamma, 4) || !aligned_to(dbeta, 4))
        return RDETR_ERR_UNSUPPORTED;
    for (int l = 0; l < L; ++l) {
        if (!dy[l] || !x[l] || !gamma[l] || !dx[l]) return RDETR_ERR_INVALID_ARG;
        if (!aligned_to(x[l], sizeof(T)) || !aligned_to(dy[l], sizeof(T)) || !aligned_to(dx[l], sizeof(T)) ||
            !aligned_to(gamma[l], params_bf16 ? 2 : 4))
            return RDETR_ERR_UNSUPPORTED;
        lv.x[l] = x[l];
        lv.dy[l] = dy[l];
        lv.y[l] = dx[l];
        lv.gamma[l] = gamma[l];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long param_blocks = ((long long)L * C + kGnThreads - 1) / kGnThreads;
    hipLaunchKernelGGL(gn_bwd_partial_kernel<T>, dim3((unsigned)bb), dim3(kGnThreads), 0, s, lv, L, C, G, B, mean, rstd, static_cast<float *>(ws));
    hipLaunchKernelGGL(gn_bwd_dx_kernel<T>, dim3((unsigned)(fb + param_blocks)), dim3(kGnThreads), 0, s, lv, L, C, G, B, params_bf16, (int)fb,
                       mean, rstd, static_cast<const float *>(ws), dgamma, dbeta);
    return launch_status();
}

// the levels' sizes and their offsets in the packed count buffers; RDETR_OK or the refusal
int pyr_levels(const int *level_hw, int L, int B, PyrOut *lv, long long *total)
{
    if (!level_hw || L <= 0 || B <= 0) return RDETR_ERR_INVALID_ARG;
    if (L > kMaxLevels || B > 65535) return RDETR_ERR_UNSUPPORTED;
    long long off = 0;
    for (int l = 0; l < L; ++l) {
        const long long h = level_hw[2 * l], w = level_hw[2 * l + 1];
        if (h <= 0 || w <= 0) return RDETR_ERR_INVALID_ARG;
        if (h * w > (1ll << 24)) return RDETR_ERR_UNSUPPORTED;
        lv->h[l] = (int)h;
        lv->w[l] = (int)w;
        lv->off[l] = off;
        off += (long long)B * h * w;
    }
    *total = off;
    return RDETR_OK;
}

template <typename T>
int pyramid_sine_pos(const int *cum, const int *level_hw, int L, int B, int F, const float *dim_t, int normalize, float scale, float eps,
                     float offset, void *const *out, void *stream)
{
    PyrOut lv = {};
    long long total = 0;
    const int st = pyr_levels(level_hw, L, B, &lv, &total);
    if (st != RDETR_OK) return st;
    if (!cum || !dim_t || !out || F <= 0) return RDETR_ERR_INVALID_ARG;
    if (F % 2 || !aligned_to(cum, 4) || !aligned_to(dim_t, 4)) return RDETR_ERR_UNSUPPORTED;
    long long blocks = 0;
    for (int l = 0; l < L; ++l) {
        if (!out[l]) return RDETR_ERR_INVALID_ARG;
        if (!aligned_to(out[l], sizeof(T))) return RDETR_ERR_UNSUPPORTED;
        lv.out[l] = out[l];
        lv.tiles[l] = (lv.h[l] * lv.w[l] + 255) / 256;
        lv.block0[l] = (int)blocks;
        blocks += (long long)B * F * lv.tiles[l];
        if (blocks > (1ll << 30)) return RDETR_ERR_UNSUPPORTED;
    }
    for (int l = L; l <= kMaxLevels; ++l) lv.block0[l] = (int)blocks;
    hipLaunchKernelGGL(pyramid_sine_pos_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), cum, total, lv, L, F,
                       dim_t, normalize, scale, eps, offset);
    return launch_status();
}

}  // namespace
}  // namespace rdetr

extern "C" {

long long rdetr_neck_workspace_bytes(const int *level_hw, int L, int B, int C, int G)
{
    rdetr::GnLevels lv = {};
    long long fb = 0, bb = 0;
    if (rdetr::gn_levels(level_hw, L, B, C, G, &lv, &fb, &bb) != RDETR_OK) return -1;
    return rdetr::neck_workspace(fb, bb);
}

int rdetr_group_norm_levels_f32(const void *const *x, const void *const *gamma, const void *const *beta, const int *level_hw, int L, int B,
                                int C, int G, float eps, void *ws, long long ws_bytes, void *const *y, float *mean, float *rstd, void *stream)
{
    return rdetr::group_norm_levels<float>(x, gamma, beta, level_hw, L, B, C, G, eps, 0, ws, ws_bytes, y, mean, rstd, stream);
}

int rdetr_group_norm_levels_bf16(const void *const *x, const void *const *gamma, const void *const *beta, int params_bf16, const int *level_hw,
                                 int L, int B, int C, int G, float eps, void *ws, long long ws_bytes, void *const *y, float *mean, float *rstd,
                                 void *stream)
{
    return rdetr::group_norm_levels<unsigned short>(x, gamma, beta, level_hw, L, B, C, G, eps, params_bf16, ws, ws_bytes, y, mean, rstd,
                                                    stream);
}

int rdetr_group_norm_levels_backward_f32(const void *const *dy, const void *const *x, const void *const *gamma, const float *mean,
                                         const float *rstd, const int *level_hw, int L, int B, int C, int G, void *ws, long long ws_bytes,
                                         void *const *dx, float *dgamma, float *dbeta, void *stream)
{
    return rdetr::group_norm_levels_backward<float>(dy, x, gamma, mean, rstd, level_hw, L, B, C, G, 0, ws, ws_bytes, dx, dgamma, dbeta, stream);
}

int rdetr_group_norm_levels_backward_bf16(const void *const *dy, const void *const *x, const void *const *gamma, int params_bf16,
                                          const float *mean, const float *rstd, const int *level_hw, int L, int B, int C, int G, void *ws,
                                          long long ws_bytes, void *const *dx, float *dgamma, float *dbeta, void *stream)
{
    return rdetr::group_norm_levels_backward<unsigned short>(dy, x, gamma, mean, rstd, level_hw, L, B, C, G, params_bf16, ws, ws_bytes, dx,
                                                             dgamma, dbeta, stream);
}

int rdetr_pyramid_masks(const void *mask, int mask_is_f32, int B, int H, int W, const int *level_hw, int L, void *const *level_masks,
                        int *cum, void *stream)
{
    using namespace rdetr;
    PyrOut lv = {};
    long long total = 0;
    const int st = pyr_levels(level_hw, L, B, &lv, &total);
    if (st != RDETR_OK) return st;
    if (!mask || !level_masks || !cum || H <= 0 || W <= 0 || (mask_is_f32 != 0 && mask_is_f32 != 1)) return RDETR_ERR_INVALID_ARG;
    if ((long long)H * W > (1ll << 30) || !aligned_to(cum, 4) || (mask_is_f32 && !aligned_to(mask, 4))) return RDETR_ERR_UNSUPPORTED;
    for (int l = 0; l < L; ++l) {
        if (!level_masks[l]) return RDETR_ERR_INVALID_ARG;
        lv.out[l] = level_masks[l];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)L, (unsigned)B, 2);
    if (mask_is_f32)
        hipLaunchKernelGGL(pyramid_masks_kernel<float>, grid, dim3(256), 0, s, static_cast<const float *>(mask), H, W, lv, total, cum);
    else
        hipLaunchKernelGGL(pyramid_masks_kernel<unsigned char>, grid, dim3(256), 0, s, static_cast<const unsigned char *>(mask), H, W, lv, total,
                           cum);
    return launch_status();
}

int rdetr_pyramid_sine_pos_f32(const int *cum, const int *level_hw, int L, int B, int F, const float *dim_t, int normalize, float scale,
                               float eps, float offset, void *const *out, void *stream)
{
    return rdetr::pyramid_sine_pos<float>(cum, level_hw, L, B, F, dim_t, normalize, scale, eps, offset, out, stream);
}

int rdetr_pyramid_sine_pos_bf16(const int *cum, const int *level_hw, int L, int B, int F, const float *dim_t, int normalize, float scale,
                                float eps, float offset, void *const *out, void *stream)
{
    return rdetr::pyramid_sine_pos<unsigned short>(cum, level_hw, L, B, F, dim_t, normalize, scale, eps, offset, out, stream);
}

}  // extern "C"
