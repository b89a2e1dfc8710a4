// The image front end: a list of [3, h, w] device images -> the padded, normalised batch and its padding mask, one launch
// (models/detectors/base_detector.py: EvalResize -> ConvertImageDtype -> Normalize -> image_list_from_tensors -> construct_mask).
//
// One workgroup owns a 16 x 64 tile of one image's padded output, all three channels; a lane owns one 16-byte piece of a tile row
// (4 fp32 or 8 bf16 pixels, so 256 or 128 lanes).  Three kinds of tile:
//   padding   y0 >= oh or x0 >= ow: zeros to the batch, ones to the mask, nothing is read
//   copy      oh == h and ow == w (training mode, no resize): the lane's pixels straight from the source, as vectors where the
//             address allows
//   resample  torch's antialiased bilinear filter, separable as torch's own CPU kernel runs it:
//               1. the tile's 64 column and 16 row tap tables, in fp64, one lane per column / row, weights rounded to fp32
//               2. horizontal pass: every source row the tile's rows touch, filtered to the tile's 64 columns, fp32, into LDS;
//                  a lane keeps its column's weights in registers and walks down the rows, the wave reads one contiguous run
//               3. vertical pass: the lane's pixels from the LDS rows, 16 bytes per read
// then, per value: uint8 sources round half to even and look (q / 255 - mean) / std up in a 3 x 256 LDS table built with the three
// fp32 operations torch runs; fp32 sources (v - mean) / std, or v with normalise off; pixels outside (oh, ow) are +0 and their mask
// byte 1.  Every store is 16 bytes per lane, the mask 4 or 8 bytes per lane.
//
// The LDS rows of pass 2 are what bounds the downscale: scale * 15 + 2 * scale + 3 rows of 3 x 64 floats, 104 KiB at scale 8
// (RDETR_IMAGE_MAX_DOWNSCALE) beside 9 KiB of tables, of the CU's 160 KiB.  The launch asks for what the batch's largest vertical
// scale needs: 14 KiB at the 480 -> 800 upscale, 64 KiB from scale 4.6 on.
// The image descriptors travel in the kernel's argument block, as the level tables of neck.hip do.
#include "launch.h"

namespace rdetr {
namespace {

constexpr int kTileH = 16, kTileW = 64;
constexpr int kMaxTaps = 2 * RDETR_IMAGE_MAX_DOWNSCALE + 2;      // hi - lo <= floor(2 * support) + 1
constexpr int kRegTaps = 4;

struct ImageTable {
    rdetr_image_desc img[RDETR_IMAGE_MAX_IMAGES];
};

// LDS rows the horizontal pass may need for one tile: hi(last row) - lo(first row) <= scale * (kTileH - 1) + 2 * support + 1
inline int patch_rows_cap(int n_in, int n_out)
{
    const double scale = (double)n_in / (double)n_out, support = scale > 1.0 ? scale : 1.0;
    return (int)(scale * (kTileH - 1) + 2.0 * support) + 3;
}

// torch's antialias taps of output index o for n_in -> n_out (aten/src/ATen/native/cpu/UpSampleKernel.cpp, triangle filter), in fp64:
// the first tap, the tap count, and the normalised weights rounded to fp32 at w[j * stride]
__device__ __forceinline__ void filter_taps(int o, int n_in, int n_out, int *lo_out, int *n_taps, float *w, int stride)
{
    const double scale = (double)n_in / (double)n_out;
    const double support = scale > 1.0 ? scale : 1.0, inv = 1.0 / support;
    const double center = scale * ((double)o + 0.5);
    const int lo = max((int)(center - support + 0.5), 0);
    const int hi = min((int)(center + support + 0.5), n_in);
    const int n = min(hi - lo, kMaxTaps);
    double total = 0.0;
    for (int j = 0; j < n; ++j) total += fmax(0.0, 1.0 - fabs(((double)(lo + j) - center + 0.5) * inv));
    for (int j = 0; j < n; ++j) w[j * stride] = (float)(fmax(0.0, 1.0 - fabs(((double)(lo + j) - center + 0.5) * inv)) / total);
    *lo_out = lo;
    *n_taps = n;
}

__device__ __forceinline__ bool aligned_dev(const void *p, unsigned a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

__device__ __forceinline__ float as_f32(unsigned char v) { return (float)v; }
__device__ __forceinline__ float as_f32(float v) { return v; }

// PX pixels of one source row into dst; the first `valid` exist, the rest read as 0.  Whole and aligned pieces move as vectors.
template <int PX> __device__ __forceinline__ void load_pixels(const unsigned char *p, int valid, float *dst)
{
    if (valid == PX && aligned_dev(p, 4)) {
#pragma unroll
        for (int k = 0; k < PX; k += 4) {
            const unsigned int u = *reinterpret_cast<const unsigned int *>(p + k);
            dst[k] = (float)(u & 255u);
            dst[k + 1] = (float)((u >> 8) & 255u);
            dst[k + 2] = (float)((u >> 16) & 255u);
            dst[k + 3] = (float)(u >> 24);
        }
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) dst[k] = k < valid ? (float)p[k] : 0.0f;
    }
}
template <int PX> __device__ __forceinline__ void load_pixels(const float *p, int valid, float *dst)
{
    if (valid == PX && aligned_dev(p, 16)) {
#pragma unroll
        for (int k = 0; k < PX; k += 4) {
            const f32x4 u = *reinterpret_cast<const f32x4 *>(p + k);
            dst[k] = u.x;
            dst[k + 1] = u.y;
            dst[k + 2] = u.z;
            dst[k + 3] = u.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) dst[k] = k < valid ? p[k] : 0.0f;
    }
}

// 4 fp32 or 8 bf16 values as one 16-byte store
__device__ __forceinline__ void store16(float *p, const float *v) { *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void store16(unsigned short *p, const float *v)
{
    *reinterpret_cast<u32x4 *>(p) = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
}

template <typename S, typename O>
__global__ __launch_bounds__(16 * kTileW / (16 / (int)sizeof(O))) void image_batch_kernel(ImageTable tab, int Hp, int Wp, float m0, float m1,
                                                                                          float m2, float d0, float d1, float d2, int normalize,
                                                                                          int channels_last, int rows_cap, O *__restrict__ out,
                                                                                          unsigned char *__restrict__ mask)
{
    constexpr int PX = 16 / (int)sizeof(O);             // pixels of one lane
    constexpr int LX = kTileW / PX;                     // lanes along a tile row
    constexpr int THREADS = LX * kTileH;
    constexpr bool kU8 = sizeof(S) == 1;
    extern __shared__ __attribute__((aligned(16))) float s_rows[];      // [3][rows][kTileW], the horizontal pass's output
    __shared__ float s_norm[kU8 ? 3 * 256 : 1];
    __shared__ float s_xw[kMaxTaps * kTileW], s_yw[kMaxTaps * kTileH];
    __shared__ int s_xlo[kTileW], s_xn[kTileW], s_ylo[kTileH], s_yn[kTileH];

    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const rdetr_image_desc im = tab.img[b];
    const S *src = static_cast<const S *>(im.src);
    const int lx = tid % LX, ly = tid / LX;
    const int x = x0 + lx * PX, y = y0 + ly;            // the lane's first pixel
    const float mean[3] = {m0, m1, m2}, stdv[3] = {d0, d1, d2};

    float v[3][PX];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < PX; ++p) v[c][p] = 0.0f;
    const bool tile_padding = y0 >= im.oh || x0 >= im.ow;        // uniform over the workgroup
    const bool lane_inside = y < im.oh && x < im.ow;
    const int valid = lane_inside ? min(PX, im.ow - x) : 0;     // the lane's pixels inside the image

    if (!tile_padding) {
        if (kU8) {
            for (int i = tid; i < 3 * 256; i += THREADS) {
                const int c = i >> 8;
                const float mc = c == 0 ? m0 : (c == 1 ? m1 : m2), dc = c == 0 ? d0 : (c == 1 ? d1 : d2);
                s_norm[i] = ((float)(i & 255) / 255.0f - mc) / dc;
            }
        }
        if (im.oh == im.h && im.ow == im.w) {
            if (lane_inside) {
#pragma unroll
                for (int c = 0; c < 3; ++c) load_pixels<PX>(src + c * im.channel_stride + (long long)y * im.row_stride + x, valid, v[c]);
            }
            if (kU8) __syncthreads();
        } else {
            const int nx = min(kTileW, im.ow - x0), ny = min(kTileH, im.oh - y0);
            if (tid < nx)
                filter_taps(x0 + tid, im.w, im.ow, &s_xlo[tid], &s_xn[tid], &s_xw[tid], kTileW);
            else if (tid >= kTileW && tid < kTileW + ny)
                filter_taps(y0 + tid - kTileW, im.h, im.oh, &s_ylo[tid - kTileW], &s_yn[tid - kTileW], &s_yw[tid - kTileW], kTileH);
            __syncthreads();
            const int r0 = s_ylo[0];
            const int rows = min(s_ylo[ny - 1] + s_yn[ny - 1] - r0, rows_cap);
            {
                const int col = tid & (kTileW - 1);
                if (col < nx) {
                    const int n = s_xn[col];
                    float w[kRegTaps];                  // the first taps in registers; beyond them (downscales past 1.5) from LDS
#pragma unroll
                    for (int i = 0; i < kRegTaps; ++i) w[i] = i < n ? s_xw[i * kTileW + col] : 0.0f;
                    for (int c = 0; c < 3; ++c) {
                        const S *p = src + c * im.channel_stride + (long long)r0 * im.row_stride + s_xlo[col];
                        for (int r = tid / kTileW; r < rows; r += THREADS / kTileW) {
                            const S *q = p + (long long)r * im.row_stride;
                            float acc = 0.0f;
#pragma unroll
                            for (int i = 0; i < kRegTaps; ++i) acc = fmaf(w[i], as_f32(q[max(min(i, n - 1), 0)]), acc);      // weight 0 behind tap n
                            for (int i = kRegTaps; i < n; ++i) acc = fmaf(s_xw[i * kTileW + col], as_f32(q[i]), acc);
                            s_rows[(c * rows + r) * kTileW + col] = acc;
                        }
                    }
                }
            }
            __syncthreads();
            if (lane_inside) {
                const int first = s_ylo[ly] - r0, n = s_yn[ly];
                for (int j = 0; j < n && first + j < rows; ++j) {
                    const float wy = s_yw[j * kTileH + ly];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float *t = &s_rows[(c * rows + first + j) * kTileW + lx * PX];
#pragma unroll
                        for (int p = 0; p < PX; p += 4) {
                            const f32x4 u = *reinterpret_cast<const f32x4 *>(t + p);
                            v[c][p] = fmaf(wy, u.x, v[c][p]);
                            v[c][p + 1] = fmaf(wy, u.y, v[c][p + 1]);
                            v[c][p + 2] = fmaf(wy, u.z, v[c][p + 2]);
                            v[c][p + 3] = fmaf(wy, u.w, v[c][p + 3]);
                        }
                    }
                }
                if (kU8) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int p = 0; p < PX; ++p) v[c][p] = fminf(fmaxf(rintf(v[c][p]), 0.0f), 255.0f);
                }
            }
        }
        // the lane's values -> what the batch holds; the columns of s_rows at or behind ow were never written and are dropped here
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                float r = v[c][p];
                if (kU8)
                    r = s_norm[c * 256 + (p < valid ? (int)r : 0)];
                else if (normalize)
                    r = (r - mean[c]) / stdv[c];
                v[c][p] = p < valid ? r : 0.0f;
            }
    }

    if (y >= Hp || x >= Wp) return;                     // Wp is a multiple of 8: a lane's piece is inside or outside as a whole
    if (channels_last) {
        float e[3 * PX];
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) e[p * 3 + c] = v[c][p];
        O *o = out + (((long long)b * Hp + y) * Wp + x) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) store16(o + k * PX, e + k * PX);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) store16(out + (((long long)b * 3 + c) * Hp + y) * Wp + x, v[c]);
    }
    unsigned int m[PX / 4];
#pragma unroll
    for (int k = 0; k < PX / 4; ++k)
        m[k] = (4 * k < valid ? 0u : 1u) | (4 * k + 1 < valid ? 0u : 1u << 8) | (4 * k + 2 < valid ? 0u : 1u << 16) | (4 * k + 3 < valid ? 0u : 1u << 24);
    unsigned int *mo = reinterpret_cast<unsigned int *>(mask + ((long long)b * Hp + y) * Wp + x);
#pragma unroll
    for (int k = 0; k < PX / 4; ++k) mo[k] = m[k];
}

template <typename S, typename O>
int launch_image_batch(const ImageTable &tab, int B, int Hp, int Wp, const float *mean, const float *stdv, int normalize, int channels_last,
                       int rows_cap, void *out, void *mask, hipStream_t stream)
{
    constexpr int threads = 16 * kTileW / (16 / (int)sizeof(O));
    const dim3 grid((unsigned)((Wp + kTileW - 1) / kTileW), (unsigned)((Hp + kTileH - 1) / kTileH), (unsigned)B);
    const size_t lds = (size_t)3 * rows_cap * kTileW * sizeof(float);
    if (ensure_dynamic_lds<image_batch_kernel<S, O>>(3 * patch_rows_cap(RDETR_IMAGE_MAX_DOWNSCALE, 1) * kTileW * (int)sizeof(float)) != RDETR_OK)
        return RDETR_ERR_LAUNCH;
    hipLaunchKernelGGL((image_batch_kernel<S, O>), grid, dim3(threads), lds, stream, tab, Hp, Wp, mean[0], mean[1], mean[2], stdv[0], stdv[1],
                       stdv[2], normalize, channels_last, rows_cap, static_cast<O *>(out), static_cast<unsigned char *>(mask));
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The augmentation's geometry: window(resize(flip(src), (rh, rw))) per image, the tile kinds, taps and tail of the kernel above.
//   flip      the taps are those of the flipped image; tap i of column x is read at source column w - 1 - (lo + i), so a wave still
//             reads one contiguous run, its lanes in descending address order, and the fp32 sum runs in the flipped image's order.
//             The copy tile loads the lane's run as the same vectors and reverses it in registers.
//   window    tile (x0, y0) of the window is tile (left + x0, top + y0) of the virtual image: the tap tables are built for those
//             columns and rows, so only the source rows that the window's rows touch are filtered.
//   kToU8     the rounded values of the tile go through LDS as bytes and leave as 16-byte stores, 192 of the 256 lanes one each.
struct WindowTable {
    rdetr_image_window_desc img[RDETR_IMAGE_MAX_IMAGES];
};

template <typename S, typename O, bool kToU8>
__global__ __launch_bounds__(16 * kTileW / (16 / (int)sizeof(O))) void image_window_kernel(WindowTable tab, int Hp, int Wp, float m0, float m1,
                                                                                           float m2, float d0, float d1, float d2, int normalize,
                                                                                           int channels_last, int rows_cap, O *__restrict__ out,
                                                                                           unsigned char *__restrict__ mask)
{
    constexpr int PX = 16 / (int)sizeof(O);
    constexpr int LX = kTileW / PX;
    constexpr int THREADS = LX * kTileH;
    constexpr bool kU8 = sizeof(S) == 1;
    static_assert(!kToU8 || (kU8 && PX == 4), "the uint8 destination: uint8 sources, four pixels per lane");
    extern __shared__ __attribute__((aligned(16))) float s_rows[];
    __shared__ float s_norm[kU8 && !kToU8 ? 3 * 256 : 1];
    __shared__ __attribute__((aligned(16))) unsigned int s_q[kToU8 ? 3 * kTileH * kTileW / 4 : 4];
    __shared__ float s_xw[kMaxTaps * kTileW], s_yw[kMaxTaps * kTileH];
    __shared__ int s_xlo[kTileW], s_xn[kTileW], s_ylo[kTileH], s_yn[kTileH];

    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const rdetr_image_window_desc im = tab.img[b];
    const S *src = static_cast<const S *>(im.src);
    const int lx = tid % LX, ly = tid / LX;
    const int x = x0 + lx * PX, y = y0 + ly;            // the lane's first pixel, in the window
    const float mean[3] = {m0, m1, m2}, stdv[3] = {d0, d1, d2};

    float v[3][PX];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < PX; ++p) v[c][p] = 0.0f;
    const bool tile_padding = y0 >= im.oh || x0 >= im.ow;        // uniform over the workgroup
    if (kToU8 && tile_padding) return;                          // the uint8 destination has no padding
    const bool lane_inside = y < im.oh && x < im.ow;
    const int valid = lane_inside ? min(PX, im.ow - x) : 0;

    if (!tile_padding) {
        if (kU8 && !kToU8) {
            for (int i = tid; i < 3 * 256; i += THREADS) {
                const int c = i >> 8;
                const float mc = c == 0 ? m0 : (c == 1 ? m1 : m2), dc = c == 0 ? d0 : (c == 1 ? d1 : d2);
                s_norm[i] = ((float)(i & 255) / 255.0f - mc) / dc;
            }
        }
        if (im.rh == im.h && im.rw == im.w) {
            if (lane_inside) {
                const long long row = (long long)(im.top + y) * im.row_stride;
                const int vx = im.left + x;                     // the lane's first column of the (flipped) image
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const S *p = src + c * im.channel_stride + row;
                    if (!im.flip) {
                        load_pixels<PX>(p + vx, valid, v[c]);
                    } else if (valid == PX) {                   // columns w - 1 - vx down to w - PX - vx: one run, reversed
                        float t[PX];
                        load_pixels<PX>(p + (im.w - PX - vx), PX, t);
#pragma unroll
                        for (int k = 0; k < PX; ++k) v[c][k] = t[PX - 1 - k];
                    } else {
#pragma unroll
                        for (int k = 0; k < PX; ++k) v[c][k] = k < valid ? as_f32(p[im.w - 1 - vx - k]) : 0.0f;
                    }
                }
            }
            if (kU8) __syncthreads();
        } else {
            const int nx = min(kTileW, im.ow - x0), ny = min(kTileH, im.oh - y0);
            if (tid < nx)
                filter_taps(im.left + x0 + tid, im.w, im.rw, &s_xlo[tid], &s_xn[tid], &s_xw[tid], kTileW);
            else if (tid >= kTileW && tid < kTileW + ny)
                filter_taps(im.top + y0 + tid - kTileW, im.h, im.rh, &s_ylo[tid - kTileW], &s_yn[tid - kTileW], &s_yw[tid - kTileW], kTileH);
            __syncthreads();
            const int r0 = s_ylo[0];
            const int rows = min(s_ylo[ny - 1] + s_yn[ny - 1] - r0, rows_cap);
            {
                const int col = tid & (kTileW - 1);
                if (col < nx) {
                    const int n = s_xn[col];
                    const int step = im.flip ? -1 : 1;
                    const int first_col = im.flip ? im.w - 1 - s_xlo[col] : s_xlo[col];
                    float w[kRegTaps];
#pragma unroll
                    for (int i = 0; i < kRegTaps; ++i) w[i] = i < n ? s_xw[i * kTileW + col] : 0.0f;
                    for (int c = 0; c < 3; ++c) {
                        const S *p = src + c * im.channel_stride + (long long)r0 * im.row_stride + first_col;
                        for (int r = tid / kTileW; r < rows; r += THREADS / kTileW) {
                            const S *q = p + (long long)r * im.row_stride;
                            float acc = 0.0f;
#pragma unroll
                            for (int i = 0; i < kRegTaps; ++i) acc = fmaf(w[i], as_f32(q[step * max(min(i, n - 1), 0)]), acc);
                            for (int i = kRegTaps; i < n; ++i) acc = fmaf(s_xw[i * kTileW + col], as_f32(q[step * i]), acc);
                            s_rows[(c * rows + r) * kTileW + col] = acc;
                        }
                    }
                }
            }
            __syncthreads();
            if (lane_inside) {
                const int first = s_ylo[ly] - r0, n = s_yn[ly];
                for (int j = 0; j < n && first + j < rows; ++j) {
                    const float wy = s_yw[j * kTileH + ly];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float *t = &s_rows[(c * rows + first + j) * kTileW + lx * PX];
#pragma unroll
                        for (int p = 0; p < PX; p += 4) {
                            const f32x4 u = *reinterpret_cast<const f32x4 *>(t + p);
                            v[c][p] = fmaf(wy, u.x, v[c][p]);
                            v[c][p + 1] = fmaf(wy, u.y, v[c][p + 1]);
                            v[c][p + 2] = fmaf(wy, u.z, v[c][p + 2]);
                            v[c][p + 3] = fmaf(wy, u.w, v[c][p + 3]);
                        }
                    }
                }
                if (kU8) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int p = 0; p < PX; ++p) v[c][p] = fminf(fmaxf(rintf(v[c][p]), 0.0f), 255.0f);
                }
            }
        }
        if (kToU8) {
            // bytes of the tile through LDS; columns at or behind ow hold 0.  A piece starts inside the row stride (the host checked
            // dst_row_stride >= ow rounded up to 16), so the stores stay inside the destination's rows.
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned int word = 0u;
#pragma unroll
                for (int p = 0; p < PX; ++p) word |= (p < valid ? (unsigned int)v[c][p] : 0u) << (8 * p);
                s_q[(c * kTileH + ly) * (kTileW / 4) + lx] = word;
            }
            __syncthreads();
            if (tid < 3 * kTileH * (kTileW / 16)) {
                const int c = tid / (kTileH * (kTileW / 16)), row = tid / (kTileW / 16) % kTileH, piece = tid % (kTileW / 16);
                const int yy = y0 + row, xx = x0 + piece * 16;
                if (yy < im.oh && xx < im.ow) {
                    unsigned char *d = static_cast<unsigned char *>(im.dst) + c * im.dst_channel_stride + (long long)yy * im.dst_row_stride + xx;
                    *reinterpret_cast<u32x4 *>(d) = *reinterpret_cast<const u32x4 *>(&s_q[(c * kTileH + row) * (kTileW / 4) + piece * 4]);
                }
            }
            return;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                float r = v[c][p];
                if (kU8)
                    r = s_norm[c * 256 + (p < valid ? (int)r : 0)];
                else if (normalize)
                    r = (r - mean[c]) / stdv[c];
                v[c][p] = p < valid ? r : 0.0f;
            }
    }

    if (y >= Hp || x >= Wp) return;
    if (channels_last) {
        float e[3 * PX];
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) e[p * 3 + c] = v[c][p];
        O *o = out + (((long long)b * Hp + y) * Wp + x) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) store16(o + k * PX, e + k * PX);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) store16(out + (((long long)b * 3 + c) * Hp + y) * Wp + x, v[c]);
    }
    unsigned int m[PX / 4];
#pragma unroll
    for (int k = 0; k < PX / 4; ++k)
        m[k] = (4 * k < valid ? 0u : 1u) | (4 * k + 1 < valid ? 0u : 1u << 8) | (4 * k + 2 < valid ? 0u : 1u << 16) | (4 * k + 3 < valid ? 0u : 1u << 24);
    unsigned int *mo = reinterpret_cast<unsigned int *>(mask + ((long long)b * Hp + y) * Wp + x);
#pragma unroll
    for (int k = 0; k < PX / 4; ++k) mo[k] = m[k];
}

template <typename S, typename O, bool kToU8>
int launch_image_window(const WindowTable &tab, int B, int Hp, int Wp, const float *mean, const float *stdv, int normalize, int channels_last,
                        int rows_cap, void *out, void *mask, hipStream_t stream)
{
    constexpr int threads = 16 * kTileW / (16 / (int)sizeof(O));
    const dim3 grid((unsigned)((Wp + kTileW - 1) / kTileW), (unsigned)((Hp + kTileH - 1) / kTileH), (unsigned)B);
    const size_t lds = (size_t)3 * rows_cap * kTileW * sizeof(float);
    if (ensure_dynamic_lds<image_window_kernel<S, O, kToU8>>(3 * patch_rows_cap(RDETR_IMAGE_MAX_DOWNSCALE, 1) * kTileW * (int)sizeof(float)) !=
        RDETR_OK)
        return RDETR_ERR_LAUNCH;
    hipLaunchKernelGGL((image_window_kernel<S, O, kToU8>), grid, dim3(threads), lds, stream, tab, Hp, Wp, mean[0], mean[1], mean[2], stdv[0],
                       stdv[1], stdv[2], normalize, channels_last, rows_cap, static_cast<O *>(out), static_cast<unsigned char *>(mask));
    return launch_status();
}

}  // namespace
}  // namespace rdetr

extern "C" int rdetr_image_batch(const rdetr_image_desc *images, int B, int src_is_u8, int Hp, int Wp, const float *mean, const float *std,
                                 int normalize, int out_bf16, int channels_last, void *out, void *mask, void *stream)
{
    using namespace rdetr;
    if (B < 0 || Hp <= 0 || Wp <= 0 || !out || !mask) return RDETR_ERR_INVALID_ARG;
    if ((src_is_u8 | normalize | out_bf16 | channels_last) & ~1) return RDETR_ERR_INVALID_ARG;
    if (B > 0 && !images) return RDETR_ERR_INVALID_ARG;
    if (normalize && (!mean || !std || std[0] == 0.0f || std[1] == 0.0f || std[2] == 0.0f)) return RDETR_ERR_INVALID_ARG;
    for (int i = 0; i < B; ++i) {
        const rdetr_image_desc &im = images[i];
        if (!im.src || im.h <= 0 || im.w <= 0 || im.oh <= 0 || im.ow <= 0 || im.row_stride < 0 || im.channel_stride < 0)
            return RDETR_ERR_INVALID_ARG;
        if (im.oh > Hp || im.ow > Wp) return RDETR_ERR_INVALID_ARG;
    }
    if (B > RDETR_IMAGE_MAX_IMAGES || Wp % 8 != 0 || Hp > (1 << 20) || Wp > (1 << 20) || !aligned_to(out, 16) || !aligned_to(mask, 8))
        return RDETR_ERR_UNSUPPORTED;
    if (src_is_u8 && !normalize) return RDETR_ERR_UNSUPPORTED;      // raw values are for float images that arrive normalised
    ImageTable tab = {};
    int rows_cap = 1;
    for (int i = 0; i < B; ++i) {
        const rdetr_image_desc &im = images[i];
        if (!src_is_u8 && !aligned_to(im.src, 4)) return RDETR_ERR_UNSUPPORTED;
        if ((long long)im.h > (long long)RDETR_IMAGE_MAX_DOWNSCALE * im.oh || (long long)im.w > (long long)RDETR_IMAGE_MAX_DOWNSCALE * im.ow)
            return RDETR_ERR_UNSUPPORTED;
        if (im.h != im.oh || im.w != im.ow) rows_cap = rows_cap > patch_rows_cap(im.h, im.oh) ? rows_cap : patch_rows_cap(im.h, im.oh);
        tab.img[i] = im;
    }
    if (B == 0) return RDETR_OK;
    static const float zero[3] = {0.0f, 0.0f, 0.0f}, one[3] = {1.0f, 1.0f, 1.0f};
    const float *m = normalize ? mean : zero, *d = normalize ? std : one;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (src_is_u8)
        return out_bf16 ? launch_image_batch<unsigned char, unsigned short>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s)
                        : launch_image_batch<unsigned char, float>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s);
    return out_bf16 ? launch_image_batch<float, unsigned short>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s)
                    : launch_image_batch<float, float>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s);
}

extern "C" int rdetr_augment_image_batch(const rdetr_image_window_desc *images, int B, int src_is_u8, int out_mode, int Hp, int Wp,
                                         const float *mean, const float *std, int normalize, int out_bf16, int channels_last, void *out,
                                         void *mask, void *stream)
{
    using namespace rdetr;
    if (out_mode != RDETR_IMAGE_OUT_BATCH && out_mode != RDETR_IMAGE_OUT_U8) return RDETR_ERR_INVALID_ARG;
    const bool to_u8 = out_mode == RDETR_IMAGE_OUT_U8;
    if (B < 0 || (src_is_u8 & ~1)) return RDETR_ERR_INVALID_ARG;
    if (!to_u8) {
        if (Hp <= 0 || Wp <= 0 || !out || !mask) return RDETR_ERR_INVALID_ARG;
        if ((normalize | out_bf16 | channels_last) & ~1) return RDETR_ERR_INVALID_ARG;
        if (normalize && (!mean || !std || std[0] == 0.0f || std[1] == 0.0f || std[2] == 0.0f)) return RDETR_ERR_INVALID_ARG;
    }
    if (B > 0 && !images) return RDETR_ERR_INVALID_ARG;
    int grid_h = 1, grid_w = 1;                         // U8 mode: the largest window
    for (int i = 0; i < B; ++i) {
        const rdetr_image_window_desc &im = images[i];
        if (!im.src || im.h <= 0 || im.w <= 0 || im.rh <= 0 || im.rw <= 0 || im.oh <= 0 || im.ow <= 0 || im.row_stride < 0 ||
            im.channel_stride < 0 || (im.flip & ~1))
            return RDETR_ERR_INVALID_ARG;
        if (im.top < 0 || im.left < 0 || (long long)im.top + im.oh > im.rh || (long long)im.left + im.ow > im.rw) return RDETR_ERR_INVALID_ARG;
        if (to_u8) {
            if (!im.dst || im.dst_row_stride < 0 || im.dst_channel_stride < 0) return RDETR_ERR_INVALID_ARG;
            grid_h = grid_h > im.oh ? grid_h : im.oh;
            grid_w = grid_w > im.ow ? grid_w : im.ow;
        } else if (im.oh > Hp || im.ow > Wp) {
            return RDETR_ERR_INVALID_ARG;
        }
    }
    if (B > RDETR_IMAGE_MAX_IMAGES) return RDETR_ERR_UNSUPPORTED;
    if (to_u8) {
        if (!src_is_u8 || grid_h > (1 << 20) || grid_w > (1 << 20)) return RDETR_ERR_UNSUPPORTED;
    } else {
        if (Wp % 8 != 0 || Hp > (1 << 20) || Wp > (1 << 20) || !aligned_to(out, 16) || !aligned_to(mask, 8)) return RDETR_ERR_UNSUPPORTED;
        if (src_is_u8 && !normalize) return RDETR_ERR_UNSUPPORTED;
    }
    WindowTable tab = {};
    int rows_cap = 1;
    for (int i = 0; i < B; ++i) {
        const rdetr_image_window_desc &im = images[i];
        if (!src_is_u8 && !aligned_to(im.src, 4)) return RDETR_ERR_UNSUPPORTED;
        if ((long long)im.h > (long long)RDETR_IMAGE_MAX_DOWNSCALE * im.rh || (long long)im.w > (long long)RDETR_IMAGE_MAX_DOWNSCALE * im.rw)
            return RDETR_ERR_UNSUPPORTED;
        if (to_u8 && (!aligned_to(im.dst, 16) || im.dst_row_stride % 16 != 0 || im.dst_channel_stride % 16 != 0 ||
                      im.dst_row_stride < ((long long)im.ow + 15) / 16 * 16))
            return RDETR_ERR_UNSUPPORTED;
        if (im.h != im.rh || im.w != im.rw) rows_cap = rows_cap > patch_rows_cap(im.h, im.rh) ? rows_cap : patch_rows_cap(im.h, im.rh);
        tab.img[i] = im;
    }
    if (B == 0) return RDETR_OK;
    static const float zero[3] = {0.0f, 0.0f, 0.0f}, one[3] = {1.0f, 1.0f, 1.0f};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (to_u8) return launch_image_window<unsigned char, float, true>(tab, B, grid_h, grid_w, zero, one, 0, 0, rows_cap, nullptr, nullptr, s);
    const float *m = normalize ? mean : zero, *d = normalize ? std : one;
    if (src_is_u8)
        return out_bf16 ? launch_image_window<unsigned char, unsigned short, false>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s)
                        : launch_image_window<unsigned char, float, false>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s);
    return out_bf16 ? launch_image_window<float, unsigned short, false>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s)
                    : launch_image_window<float, float, false>(tab, B, Hp, Wp, m, d, normalize, channels_last, rows_cap, out, mask, s);
}
