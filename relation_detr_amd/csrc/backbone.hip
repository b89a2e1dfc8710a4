// The ResNet backbone's epilogues: what follows each library convolution when the norm is a FrozenBatchNorm2d
// (models/bricks/misc.py: x * scale + bias as separate passes; models/backbones/resnet.py: relu, out += identity, maxpool).
//
//   frozen_bn_act            out = act(x * scale[c] + shift[c] (+ residual))              one read of each operand, one write
//   frozen_bn_act_backward   dx = (dy * [y > 0]) * scale[c], dres = dy * [y > 0]          from the saved OUTPUT: x is not needed, so the
//                                                                                         forward may always run in place
//   stem_pool                out = maxpool3x3/s2/p1(relu(x * scale[c] + shift[c]))        the stem's tail, 1.25 passes of the map
//
// All three are memory bound.  Every tensor is read and written in 16-byte pieces (4 fp32, 8 bf16) on the 16-byte grid of its base:
//   NCHW            a workgroup walks (plane, chunk of 256 pieces) items, so scale and shift are one scalar load per item; a plane
//                   whose H * W is no multiple of the piece starts off the grid, its head (up to the next grid point) and tail are
//                   scalars taken by the lanes of the plane's first chunk
//   channels-last   the tensor is one flat [B * H * W, C] run; with C a multiple of the piece a lane's channels are one run of
//                   scale / shift (vector loads), its first channel carried along the grid-stride loop; any other C takes the
//                   channel of each element modulo C
// Grids are capped at 8 workgroups per CU and stride over the rest.  fp32 arithmetic is one rounded multiply and one rounded add
// per step (__fmul_rn / __fadd_rn: never an FMA), which is what makes the fp32 results torch's bit for bit.
#include <math.h>

#include "launch.h"

namespace rdetr {
namespace {

constexpr int kThreads = 256;
constexpr int kGroupsPerCu = 8;

enum { kForward = 0, kBackward = 1 };
enum { kUniform = 0, kRun = 1, kModulo = 2 };       // how a piece's channels lie: one channel, a run of V, (c + j) % C

struct EwArgs {
    const void *a, *b;          // forward: x, residual (nullable); backward: dy, y (NULL with relu off)
    const float *scale, *shift;
    void *o1, *o2;              // forward: out, -; backward: dx, dres (nullable)
};

template <typename T> struct PieceOf { static constexpr int n = 16 / (int)sizeof(T); };

// V values of T as floats; V is 1 or the 16-byte piece
template <int V> __device__ __forceinline__ void load_n(const float *p, float *v)
{
    if constexpr (V == 1) {
        v[0] = p[0];
    } else {
        const f32x4 u = *reinterpret_cast<const f32x4 *>(p);
        v[0] = u.x, v[1] = u.y, v[2] = u.z, v[3] = u.w;
    }
}
template <int V> __device__ __forceinline__ void load_n(const unsigned short *p, float *v)
{
    if constexpr (V == 1) {
        v[0] = bf16_bits_to_f32(p[0]);
    } else {
        const u32x4 u = *reinterpret_cast<const u32x4 *>(p);
        const unsigned int w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = bf16_bits_to_f32(w[k] & 0xffffu);
            v[2 * k + 1] = __builtin_bit_cast(float, w[k] & 0xffff0000u);
        }
    }
}
template <int V> __device__ __forceinline__ void store_n(float *p, const float *v)
{
    if constexpr (V == 1)
        p[0] = v[0];
    else
        *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
}
template <int V> __device__ __forceinline__ void store_n(unsigned short *p, const float *v)
{
    if constexpr (V == 1)
        p[0] = (unsigned short)f32_to_bf16_bits(v[0]);
    else
        *reinterpret_cast<u32x4 *>(p) =
            u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
}

// relu as torch's: a NaN stays (the compare is false), everything below zero becomes +0
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.0f ? 0.0f : v; }

__device__ __forceinline__ float bn_value(float x, float s, float h) { return __fadd_rn(__fmul_rn(x, s), h); }

// V elements from element index i on; ch: the piece's one channel (kUniform) or the channel of its first element
template <typename T, int MODE, bool RELU, int CH, int V>
__device__ __forceinline__ void ew_piece(const EwArgs &g, long long i, int ch, int C)
{
    const T *a = static_cast<const T *>(g.a) + i, *b = static_cast<const T *>(g.b);
    float s[V], h[V], va[V], vb[V], r1[V], r2[V];
    if constexpr (CH == kRun && V > 1) {
#pragma unroll
        for (int k = 0; k < V; k += 4) {
            load_n<4>(g.scale + ch + k, s + k);
            if (MODE == kForward) load_n<4>(g.shift + ch + k, h + k);
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int c = CH == kModulo ? (ch + j) % C : ch;
            s[j] = g.scale[c];
            if (MODE == kForward) h[j] = g.shift[c];
        }
    }
    load_n<V>(a, va);
    if (b) load_n<V>(b + i, vb);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if constexpr (MODE == kForward) {
            float v = bn_value(va[j], s[j], h[j]);
            if (b) v = __fadd_rn(v, vb[j]);
            r1[j] = RELU ? relu_keep_nan(v) : v;
        } else {
            const float m = RELU ? (vb[j] <= 0.0f ? 0.0f : va[j]) : va[j];      // threshold_backward: a NaN output passes dy on
            r2[j] = m;
            r1[j] = __fmul_rn(m, s[j]);
        }
    }
    store_n<V>(static_cast<T *>(g.o1) + i, r1);
    if (MODE == kBackward && g.o2) store_n<V>(static_cast<T *>(g.o2) + i, r2);
}

template <typename T, int MODE, bool RELU>
__global__ __launch_bounds__(kThreads) void ew_nchw_kernel(EwArgs g, int C, int HW, int chunks, int items)
{
    constexpr int V = PieceOf<T>::n;
    for (unsigned item = blockIdx.x; item < (unsigned)items; item += gridDim.x) {      // items < 2^31: the sum cannot wrap
        const int plane = (int)(item / (unsigned)chunks), k = (int)(item - (unsigned)plane * (unsigned)chunks);      // uniform over the workgroup
        const int c = plane % C;
        const long long start = (long long)plane * HW, end = start + HW;
        long long a0 = (start + V - 1) / V * V;                         // the plane's first point on the 16-byte grid
        a0 = a0 < end ? a0 : end;
        const int nv = (int)((end - a0) / V);
        const int v = k * kThreads + (int)threadIdx.x;
        if (v < nv) ew_piece<T, MODE, RELU, kUniform, V>(g, a0 + (long long)v * V, c, C);
        if (k == 0) {
            const int head = (int)(a0 - start), tail = (int)(end - a0) - nv * V, t = kThreads - 1 - (int)threadIdx.x;
            if (t < head)
                ew_piece<T, MODE, RELU, kUniform, 1>(g, start + t, c, C);
            else if (t < head + tail)
                ew_piece<T, MODE, RELU, kUniform, 1>(g, a0 + (long long)nv * V + (t - head), c, C);
        }
    }
}

template <typename T, int MODE, bool RELU, int CH>
__global__ __launch_bounds__(kThreads) void ew_nhwc_kernel(EwArgs g, int C, long long numel)
{
    constexpr int V = PieceOf<T>::n;
    const long long nv = numel / V, stride = (long long)gridDim.x * kThreads;
    long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
    int c = (int)(v * V % C);
    const int step = (int)(stride * V % C);
    for (; v < nv; v += stride) {
        ew_piece<T, MODE, RELU, CH, V>(g, v * V, c, C);
        c += step;
        c = c >= C ? c - C : c;
    }
    if (blockIdx.x == 0 && (long long)threadIdx.x < numel - nv * V) {
        const long long i = nv * V + threadIdx.x;
        ew_piece<T, MODE, RELU, kUniform, 1>(g, i, (int)(i % C), C);
    }
}

inline unsigned capped_grid(long long groups)
{
    const long long cap = (long long)device_cu_count() * kGroupsPerCu;
    return (unsigned)(groups < 1 ? 1 : (groups < cap ? groups : cap));
}

template <typename T, int MODE, bool RELU>
int launch_ew(const EwArgs &g, int B, int C, int H, int W, int channels_last, hipStream_t stream)
{
    constexpr int V = PieceOf<T>::n;
    const long long numel = (long long)B * C * H * W;
    if (channels_last) {
        const unsigned grid = capped_grid((numel / V + kThreads - 1) / kThreads);
        if (C % V == 0)
            hipLaunchKernelGGL((ew_nhwc_kernel<T, MODE, RELU, kRun>), dim3(grid), dim3(kThreads), 0, stream, g, C, numel);
        else
            hipLaunchKernelGGL((ew_nhwc_kernel<T, MODE, RELU, kModulo>), dim3(grid), dim3(kThreads), 0, stream, g, C, numel);
    } else {
        const int HW = H * W;                                           // < 2^31 with numel
        const int chunks = HW / V / kThreads + (HW / V % kThreads != 0 || HW < V ? 1 : 0);
        const long long items = (long long)B * C * chunks;
        if (!grid_fits(items)) return RDETR_ERR_UNSUPPORTED;
        hipLaunchKernelGGL((ew_nchw_kernel<T, MODE, RELU>), dim3(capped_grid(items)), dim3(kThreads), 0, stream, g, C, HW, chunks, (int)items);
    }
    return launch_status();
}

// ---- the stem's tail ------------------------------------------------------------------------------------------------------------
// One lane, V channels of one output pixel (channels-last, C a multiple of the piece: every load and the store are 16 bytes) or one
// output element (V = 1: channels-last with any other C, and NCHW rows that stem_pool_rows_kernel below does not take).  The up to nine inputs of a window are read where they lie; a
// neighbouring lane's window shares six of them, which the L1 serves.
template <typename T, int V, bool NHWC>
__global__ __launch_bounds__(kThreads) void stem_pool_kernel(const T *__restrict__ x, const float *__restrict__ scale,
                                                             const float *__restrict__ shift, int C, int H, int W, int OH, int OW,
                                                             unsigned total, T *__restrict__ out)
{
    const unsigned G = C / V;                                           // channel groups of one pixel
    const unsigned stride = gridDim.x * kThreads;                       // total < 2^31 and the grid is capped: i + stride cannot wrap
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
        int c, ox, oy;
        long long base, step_x, step_y;                                 // of the input: element (b, c.., 0, 0) and its strides
        if (NHWC) {
            const unsigned g = i % G;
            unsigned t = i / G;
            ox = (int)(t % (unsigned)OW), t /= (unsigned)OW;
            oy = (int)(t % (unsigned)OH);
            c = (int)g * V;
            base = (long long)(t / (unsigned)OH) * H * W * C + c, step_x = C, step_y = (long long)W * C;
        } else {
            ox = (int)(i % (unsigned)OW);
            unsigned t = i / (unsigned)OW;
            oy = (int)(t % (unsigned)OH);
            const unsigned plane = t / (unsigned)OH;
            c = (int)(plane % (unsigned)C);
            base = (long long)plane * H * W, step_x = 1, step_y = W;
        }
        float s[V], h[V], m[V], v[V];
#pragma unroll
        for (int k = 0; k < V; k += (V > 1 ? 4 : 1)) {
            load_n<(V > 1 ? 4 : 1)>(scale + c + k, s + k);
            load_n<(V > 1 ? 4 : 1)>(shift + c + k, h + k);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) m[j] = -INFINITY;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int y = 2 * oy + dy;
            if (y < 0 || y >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = 2 * ox + dx;
                if (xx < 0 || xx >= W) continue;                        // padding never wins: it is never looked at
                load_n<V>(x + base + y * step_y + xx * step_x, v);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float r = relu_keep_nan(bn_value(v[j], s[j], h[j]));
                    m[j] = (r > m[j] || r != r) ? r : m[j];             // torch's max_pool2d: a NaN takes the window
                }
            }
        }
        store_n<V>(out + (long long)i * V, m);
    }
}

// NCHW with W a multiple of 8 (every batch the front end pads is): one lane, four neighbouring outputs of a row.  Their windows span
// the nine columns 8g - 1 .. 8g + 7: one scalar and 32 bytes (fp32) or 16 bytes (bf16) of vector loads per input row, all inside
// the row, and one 16- or 8-byte store.  The column left of the row (g = 0) is padding and enters as -inf, which never wins.
__device__ __forceinline__ void store4(float *p, const float *v) { *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void store4(unsigned short *p, const float *v)
{
    *reinterpret_cast<u32x2 *>(p) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}

template <typename T>
__global__ __launch_bounds__(kThreads) void stem_pool_rows_kernel(const T *__restrict__ x, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, int C, int H, int W, int OH,
                                                                  unsigned total, T *__restrict__ out)
{
    constexpr int V = PieceOf<T>::n;
    const unsigned GW = (unsigned)W / 8, stride = gridDim.x * kThreads;
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
        const unsigned g = i % GW, t = i / GW, oy = t % (unsigned)OH, plane = t / (unsigned)OH;
        const float s = scale[plane % (unsigned)C], h = shift[plane % (unsigned)C];
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int y = 2 * (int)oy + dy;
            if (y < 0 || y >= H) continue;
            const T *row = x + ((long long)plane * H + y) * W + 8 * g;
            float v[9], r[9];
#pragma unroll
            for (int k = 0; k < 8; k += V) load_n<V>(row + k, v + 1 + k);
            r[0] = -INFINITY;
            if (g > 0) {
                load_n<1>(row - 1, v);
                r[0] = relu_keep_nan(bn_value(v[0], s, h));
            }
#pragma unroll
            for (int j = 1; j < 9; ++j) r[j] = relu_keep_nan(bn_value(v[j], s, h));
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int j = 2 * o; j <= 2 * o + 2; ++j) m[o] = (r[j] > m[o] || r[j] != r[j]) ? r[j] : m[o];
        }
        store4(out + (long long)i * 4, m);
    }
}

template <typename T>
int launch_stem_pool(const void *x, const float *scale, const float *shift, int B, int C, int H, int W, int channels_last, void *out,
                     hipStream_t stream)
{
    constexpr int V = PieceOf<T>::n;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const long long outputs = (long long)B * C * OH * OW;
    const T *xp = static_cast<const T *>(x);
    T *op = static_cast<T *>(out);
    if (channels_last && C % V == 0) {
        const long long total = outputs / V;
        hipLaunchKernelGGL((stem_pool_kernel<T, V, true>), dim3(capped_grid((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, xp,
                           scale, shift, C, H, W, OH, OW, (unsigned)total, op);
    } else if (channels_last) {
        hipLaunchKernelGGL((stem_pool_kernel<T, 1, true>), dim3(capped_grid((outputs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           xp, scale, shift, C, H, W, OH, OW, (unsigned)outputs, op);
    } else if (W % 8 == 0) {
        const long long total = outputs / 4;                            // OW = W / 2 is a multiple of 4
        hipLaunchKernelGGL((stem_pool_rows_kernel<T>), dim3(capped_grid((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, xp, scale,
                           shift, C, H, W, OH, (unsigned)total, op);
    } else {
        hipLaunchKernelGGL((stem_pool_kernel<T, 1, false>), dim3(capped_grid((outputs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                           xp, scale, shift, C, H, W, OH, OW, (unsigned)outputs, op);
    }
    return launch_status();
}

// ---- operand checks -------------------------------------------------------------------------------------------------------------
inline bool overlaps(const void *p, const void *q, long long bytes_p, long long bytes_q)
{
    if (!p || !q) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)bytes_q && b < a + (uintptr_t)bytes_p;
}

inline int shape_status(int B, int C, int H, int W, int flags)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (flags & ~1)) return RDETR_ERR_INVALID_ARG;
    return RDETR_OK;
}

inline bool too_large(int B, int C, int H, int W) { return (long long)B * C * H * W >= (1ll << 31); }

template <typename T>
int frozen_bn_act(const void *x, const float *scale, const float *shift, const void *residual, int B, int C, int H, int W,
                  int channels_last, int relu, void *out, void *stream)
{
    if (!x || !scale || !shift || !out) return RDETR_ERR_INVALID_ARG;
    if (const int s = shape_status(B, C, H, W, channels_last | relu)) return s;
    if (too_large(B, C, H, W)) return RDETR_ERR_UNSUPPORTED;
    const long long bytes = (long long)B * C * H * W * (long long)sizeof(T);
    if (overlaps(residual, out, bytes, bytes) || (x != out && overlaps(x, out, bytes, bytes))) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, x, scale, shift, residual, out)) return RDETR_ERR_UNSUPPORTED;
    const EwArgs g = {x, residual, scale, shift, out, nullptr};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return relu ? launch_ew<T, kForward, true>(g, B, C, H, W, channels_last, s) : launch_ew<T, kForward, false>(g, B, C, H, W, channels_last, s);
}

template <typename T>
int frozen_bn_act_backward(const void *dy, const void *y, const float *scale, int B, int C, int H, int W, int channels_last, int relu,
                           void *dx, void *dres, void *stream)
{
    if (!dy || !scale || !dx) return RDETR_ERR_INVALID_ARG;
    if (const int s = shape_status(B, C, H, W, channels_last | relu)) return s;
    if (relu && !y) return RDETR_ERR_INVALID_ARG;
    if (too_large(B, C, H, W)) return RDETR_ERR_UNSUPPORTED;
    const long long bytes = (long long)B * C * H * W * (long long)sizeof(T);
    if (overlaps(dres, dx, bytes, bytes) || overlaps(y, dx, bytes, bytes) || overlaps(y, dres, bytes, bytes)) return RDETR_ERR_INVALID_ARG;
    if ((dy != dx && overlaps(dy, dx, bytes, bytes)) || overlaps(dy, dres, bytes, bytes)) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, dy, y, scale, dx, dres)) return RDETR_ERR_UNSUPPORTED;
    const EwArgs g = {dy, relu ? y : nullptr, scale, nullptr, dx, dres};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return relu ? launch_ew<T, kBackward, true>(g, B, C, H, W, channels_last, s) : launch_ew<T, kBackward, false>(g, B, C, H, W, channels_last, s);
}

template <typename T>
int stem_pool(const void *x, const float *scale, const float *shift, int B, int C, int H, int W, int channels_last, void *out, void *stream)
{
    if (!x || !scale || !shift || !out) return RDETR_ERR_INVALID_ARG;
    if (const int s = shape_status(B, C, H, W, channels_last)) return s;
    if (too_large(B, C, H, W)) return RDETR_ERR_UNSUPPORTED;
    const long long in_bytes = (long long)B * C * H * W * (long long)sizeof(T);
    const long long out_bytes = (long long)B * C * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * (long long)sizeof(T);
    if (overlaps(x, out, in_bytes, out_bytes)) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, x, scale, shift, out)) return RDETR_ERR_UNSUPPORTED;
    return launch_stem_pool<T>(x, scale, shift, B, C, H, W, channels_last, out, static_cast<hipStream_t>(stream));
}

}  // namespace
}  // namespace rdetr

extern "C" int rdetr_frozen_bn_act_f32(const void *x, const float *scale, const float *shift, const void *residual, int B, int C, int H,
                                       int W, int channels_last, int relu, void *out, void *stream)
{
    return rdetr::frozen_bn_act<float>(x, scale, shift, residual, B, C, H, W, channels_last, relu, out, stream);
}

extern "C" int rdetr_frozen_bn_act_bf16(const void *x, const float *scale, const float *shift, const void *residual, int B, int C, int H,
                                        int W, int channels_last, int relu, void *out, void *stream)
{
    return rdetr::frozen_bn_act<unsigned short>(x, scale, shift, residual, B, C, H, W, channels_last, relu, out, stream);
}

extern "C" int rdetr_frozen_bn_act_backward_f32(const void *dy, const void *y, const float *scale, int B, int C, int H, int W,
                                                int channels_last, int relu, void *dx, void *dres, void *stream)
{
    return rdetr::frozen_bn_act_backward<float>(dy, y, scale, B, C, H, W, channels_last, relu, dx, dres, stream);
}

extern "C" int rdetr_frozen_bn_act_backward_bf16(const void *dy, const void *y, const float *scale, int B, int C, int H, int W,
                                                 int channels_last, int relu, void *dx, void *dres, void *stream)
{
    return rdetr::frozen_bn_act_backward<unsigned short>(dy, y, scale, B, C, H, W, channels_last, relu, dx, dres, stream);
}

extern "C" int rdetr_stem_pool_f32(const void *x, const float *scale, const float *shift, int B, int C, int H, int W, int channels_last,
                                   void *out, void *stream)
{
    return rdetr::stem_pool<float>(x, scale, shift, B, C, H, W, channels_last, out, stream);
}

extern "C" int rdetr_stem_pool_bf16(const void *x, const float *scale, const float *shift, int B, int C, int H, int W, int channels_last,
                                    void *out, void *stream)
{
    return rdetr::stem_pool<unsigned short>(x, scale, shift, B, C, H, W, channels_last, out, stream);
}
