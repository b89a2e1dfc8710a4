// Residual add + LayerNorm in one pass, for the rows either side of the hot-path kernels (gfx950).
//
// Replaces the pairs  `x + sublayer(x)` -> nn.LayerNorm  of the reference's encoder / decoder layers
// (models/bricks/relation_transformer.py:262-276 encoder layer, :452-478 decoder layer, :360 decoder norm):
// two elementwise passes + a normalisation pass (5 tensor traversals) become one read of each operand and one write.
//
//   C = 256 (the model's embed_dim): half a wavefront per row, a lane owns 8 consecutive channels (16-byte bf16 / 2 x 16-byte
//   fp32 accesses), four rows per wave in flight; any other C <= 8192: one wavefront per row, strided scalar loop.
//   Statistics in fp32, two-pass in registers (mean, then the variance of the centred values), biased variance and
//   1/sqrt(var + eps) as torch.nn.functional.layer_norm; the sum x + r is NOT rounded to the storage type first.
// Bound: HBM (3 x rows x C x sizeof(T) bytes per call).
//
// Training (C = 256 only, further down): the same forward body that also stores {mean, rstd} per row, and the backward from them --
// dx for both operands in one pass over dy, x and r, dgamma / dbeta through per-workgroup partials summed in a fixed order.
#include "launch.h"
#include "rows256.h"

namespace rdetr {

template <typename T> struct LnIO;
template <> struct LnIO<float> {
    static __device__ __forceinline__ void load4(const float *p, float (&v)[4])
    {
        const f32x4 r = *reinterpret_cast<const f32x4 *>(p);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
    static __device__ __forceinline__ void store4(float *p, const float (&v)[4])
    {
        *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
    }
    static __device__ __forceinline__ float load1(const float *p) { return *p; }
    static __device__ __forceinline__ void store1(float *p, float v) { *p = v; }
};
template <> struct LnIO<uint16_t> {
    static __device__ __forceinline__ void load4(const uint16_t *p, float (&v)[4])
    {
        const u32x2 r = *reinterpret_cast<const u32x2 *>(p);
        v[0] = __builtin_bit_cast(float, r.x << 16); v[1] = __builtin_bit_cast(float, r.x & 0xffff0000u);
        v[2] = __builtin_bit_cast(float, r.y << 16); v[3] = __builtin_bit_cast(float, r.y & 0xffff0000u);
    }
    static __device__ __forceinline__ void store4(uint16_t *p, const float (&v)[4])
    {
        u32x2 o;
        o.x = f32_to_bf16_bits(v[0]) | (f32_to_bf16_bits(v[1]) << 16);
        o.y = f32_to_bf16_bits(v[2]) | (f32_to_bf16_bits(v[3]) << 16);
        *reinterpret_cast<u32x2 *>(p) = o;
    }
    static __device__ __forceinline__ float load1(const uint16_t *p) { return bf16_bits_to_f32(*p); }
    static __device__ __forceinline__ void store1(uint16_t *p, float v) { *p = (uint16_t)f32_to_bf16_bits(v); }
};

__device__ __forceinline__ float ln_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T> __device__ __forceinline__ float ln_round(float v);
template <> __device__ __forceinline__ float ln_round<float>(float v) { return v; }
template <> __device__ __forceinline__ float ln_round<uint16_t>(float v) { return bf16_bits_to_f32((uint16_t)f32_to_bf16_bits(v)); }

constexpr int kLnWaves = 4;
constexpr int kLnRowsPerWave = 4;          // C = 256 kernel: half a wave per row (32 lanes x 8 channels), 2 rows per half

template <typename T> struct LnIO8;
template <> struct LnIO8<float> {
    static __device__ __forceinline__ void load(const float *p, float (&v)[8])
    {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p), b = *reinterpret_cast<const f32x4 *>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ void store(float *p, const float (&v)[8])
    {
        *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4 *>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
};
template <> struct LnIO8<uint16_t> {
    static __device__ __forceinline__ void load(const uint16_t *p, float (&v)[8])
    {
        row256_widen8(*reinterpret_cast<const u32x4 *>(p), v);
    }
    static __device__ __forceinline__ void store(uint16_t *p, const float (&v)[8])
    {
        // two converts and an OR per pair, not pack_bf16x2's one packed convert (same bits): that spelling is the kernels' measured code
        u32x4 o;
        o.x = f32_to_bf16_bits(v[0]) | (f32_to_bf16_bits(v[1]) << 16);
        o.y = f32_to_bf16_bits(v[2]) | (f32_to_bf16_bits(v[3]) << 16);
        o.z = f32_to_bf16_bits(v[4]) | (f32_to_bf16_bits(v[5]) << 16);
        o.w = f32_to_bf16_bits(v[6]) | (f32_to_bf16_bits(v[7]) << 16);
        *reinterpret_cast<u32x4 *>(p) = o;
    }
};

// C == 256: a half wave owns a row (a lane 8 consecutive channels = one 16-byte bf16 access), a wave works on 4 rows with
// all of their loads issued before the first use (the one-row-per-wave version kept 1.5 KB in flight per wave and reached
// 3.7 TB/s; HBM needs more outstanding bytes than that).
// kStats (the training forward): additionally the row's mean and 1/sqrt(var + eps) as fp32 into stats[row] = {mean, rstd}, what the
// backward kernel below starts from.  The arithmetic is the one body, so `out` has the same bits with and without.
// TR / TP / TO (the mixed-precision training forward): the residual's, the parameters' and the output's storage type where they
// differ from x's; every value is widened to fp32 as it is loaded, so the arithmetic below is the same for every combination.
template <typename T, bool kStats, typename TR = T, typename TP = T, typename TO = T>
__device__ __forceinline__ void add_layernorm256_body(const T *__restrict__ x, const TR *__restrict__ r, const TP *__restrict__ gamma,
                                                      const TP *__restrict__ beta, long long rows, long long ldx, long long ldr,
                                                      long long ldo, float eps, TO *__restrict__ out, const TO *__restrict__ pos,
                                                      long long ldp, TO *__restrict__ out2, long long ldo2, float *__restrict__ stats)
{
    const int lane = threadIdx.x & 63, half = lane >> 5, c = (lane & 31) * 8;
    const long long row0 = ((long long)blockIdx.x * kLnWaves + (threadIdx.x >> 6)) * kLnRowsPerWave + half;
    float v[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long row = row0 + 2 * i;
        if (row < rows) {
            LnIO8<T>::load(x + row * ldx + c, v[i]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[i][k] = 0.f;
        }
    }
    if (r) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long row = row0 + 2 * i;
            if (row < rows) {
                float t[8];
                LnIO8<TR>::load(r + row * ldr + c, t);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[i][k] += t[k];
            }
        }
    }
    float g[8], b[8];
    LnIO8<TP>::load(gamma + c, g);
    LnIO8<TP>::load(beta + c, b);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long row = row0 + 2 * i;
        // same summation tree per lane as the 4-channel version would not be required: statistics are fp32 either way.
        // rt_normalise (csrc/rowtail.hip) repeats this block operation for operation: change the two together (rows256.h)
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[i][k];
        const float mean = row256_half_sum(s) * (1.0f / 256.0f);
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[i][k] -= mean;
            sq += v[i][k] * v[i][k];
        }
        const float rstd = 1.0f / sqrtf(row256_half_sum(sq) * (1.0f / 256.0f) + eps);
        float y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) y[k] = v[i][k] * rstd * g[k] + b[k];
        if (row < rows) {
            LnIO8<TO>::store(out + row * ldo + c, y);
            if constexpr (kStats) {
                if ((lane & 31) == 0) *reinterpret_cast<f32x2 *>(stats + row * 2) = f32x2{mean, rstd};
            }
            if (out2) {                      // out2 = out + pos, from the STORED (rounded) normalised values: the bits of a separate add
                float pv[8];
                LnIO8<TO>::load(pos + row * ldp + c, pv);
#pragma unroll
                for (int k = 0; k < 8; ++k) pv[k] += ln_round<TO>(y[k]);
                LnIO8<TO>::store(out2 + row * ldo2 + c, pv);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kLnWaves *kWave) void add_layernorm256_kernel(const T *__restrict__ x, const T *__restrict__ r,
                                                                           const T *__restrict__ gamma,
                                                                           const T *__restrict__ beta, long long rows,
                                                                           long long ldx, long long ldr, long long ldo,
                                                                           float eps, T *__restrict__ out,
                                                                           const T *__restrict__ pos, long long ldp,
                                                                           T *__restrict__ out2, long long ldo2)
{
    add_layernorm256_body<T, false>(x, r, gamma, beta, rows, ldx, ldr, ldo, eps, out, pos, ldp, out2, ldo2, nullptr);
}

template <typename T>
__global__ __launch_bounds__(kLnWaves *kWave) void add_layernorm256_train_kernel(const T *__restrict__ x, const T *__restrict__ r,
                                                                                 const T *__restrict__ gamma,
                                                                                 const T *__restrict__ beta, long long rows,
                                                                                 long long ldx, long long ldr, long long ldo,
                                                                                 float eps, T *__restrict__ out,
                                                                                 float *__restrict__ stats)
{
    add_layernorm256_body<T, true, T, T, T>(x, r, gamma, beta, rows, ldx, ldr, ldo, eps, out, nullptr, 0, nullptr, 0, stats);
}

// Mixed-precision training forward (bf16 autocast over fp32 parameters): x and the residual each fp32 or bf16, gamma / beta / out fp32
template <typename TX, typename TR>
__global__ __launch_bounds__(kLnWaves *kWave) void add_layernorm256_train_mixed_kernel(const TX *__restrict__ x, const TR *__restrict__ r,
                                                                                       const float *__restrict__ gamma,
                                                                                       const float *__restrict__ beta, long long rows,
                                                                                       long long ldx, long long ldr, long long ldo,
                                                                                       float eps, float *__restrict__ out,
                                                                                       float *__restrict__ stats)
{
    add_layernorm256_body<TX, true, TR, float, float>(x, r, gamma, beta, rows, ldx, ldr, ldo, eps, out, nullptr, 0, nullptr, 0, stats);
}

template <typename T>
__global__ __launch_bounds__(kLnWaves *kWave) void add_layernorm_generic_kernel(const T *__restrict__ x, const T *__restrict__ r,
                                                                                const T *__restrict__ gamma,
                                                                                const T *__restrict__ beta, long long rows,
                                                                                int C, long long ldx, long long ldr,
                                                                                long long ldo, float eps, T *__restrict__ out,
                                                                                const T *__restrict__ pos, long long ldp,
                                                                                T *__restrict__ out2, long long ldo2)
{
    const long long row = (long long)blockIdx.x * kLnWaves + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const T *xr = x + row * ldx, *rr = r ? r + row * ldr : nullptr;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += LnIO<T>::load1(xr + c) + (rr ? LnIO<T>::load1(rr + c) : 0.f);
    const float mean = ln_wave_sum(s) / (float)C;
    float sq = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = LnIO<T>::load1(xr + c) + (rr ? LnIO<T>::load1(rr + c) : 0.f) - mean;
        sq += d * d;
    }
    const float rstd = 1.0f / sqrtf(ln_wave_sum(sq) / (float)C + eps);
    for (int c = lane; c < C; c += 64) {
        const float d = LnIO<T>::load1(xr + c) + (rr ? LnIO<T>::load1(rr + c) : 0.f) - mean;
        const float y = d * rstd * LnIO<T>::load1(gamma + c) + LnIO<T>::load1(beta + c);
        LnIO<T>::store1(out + row * ldo + c, y);
        if (out2) LnIO<T>::store1(out2 + row * ldo2 + c, ln_round<T>(y) + LnIO<T>::load1(pos + row * ldp + c));
    }
}

template <typename T>
static int add_layernorm(const T *x, const T *r, const T *gamma, const T *beta, long long rows, int C, long long ldx,
                         long long ldr, long long ldo, float eps, T *out, hipStream_t stream, const T *pos = nullptr,
                         long long ldp = 0, T *out2 = nullptr, long long ldo2 = 0)
{
    if (rows < 0 || C <= 0 || C > 8192 || ldx < C || ldo < C || (r && ldr < C)) return RDETR_ERR_INVALID_ARG;
    if ((out2 != nullptr) != (pos != nullptr) || (out2 && (ldp < C || ldo2 < C))) return RDETR_ERR_INVALID_ARG;
    if (rows == 0) return RDETR_OK;
    if (!x || !gamma || !beta || !out) return RDETR_ERR_INVALID_ARG;
    const long long nblk = (rows + kLnWaves - 1) / kLnWaves;
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    const long long nblk256 = (rows + kLnWaves * kLnRowsPerWave - 1) / (kLnWaves * kLnRowsPerWave);
    constexpr int eb = (int)sizeof(T);
    if (C == 256 && rows_ok(x, ldx, C, eb) && rows_ok(out, ldo, C, eb) && all_aligned(16, gamma, beta) && (!r || rows_ok(r, ldr, C, eb)) &&
        (!out2 || (rows_ok(pos, ldp, C, eb) && rows_ok(out2, ldo2, C, eb))))
        hipLaunchKernelGGL((add_layernorm256_kernel<T>), dim3((unsigned)nblk256), dim3(kLnWaves * kWave), 0, stream, x, r, gamma,
                           beta, rows, ldx, ldr, ldo, eps, out, pos, ldp, out2, ldo2);
    else
        hipLaunchKernelGGL((add_layernorm_generic_kernel<T>), dim3((unsigned)nblk), dim3(kLnWaves * kWave), 0, stream, x, r,
                           gamma, beta, rows, C, ldx, ldr, ldo, eps, out, pos, ldp, out2, ldo2);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- training
// Forward with the row statistics kept, C == 256 only: the vectorised kernel or RDETR_ERR_UNSUPPORTED (no generic-C route).
template <typename T>
static int add_layernorm_train(const T *x, const T *r, const T *gamma, const T *beta, long long rows, int C, long long ldx,
                               long long ldr, long long ldo, float eps, T *out, float *stats, hipStream_t stream)
{
    if (rows < 0 || C <= 0 || ldx < C || ldo < C || (r && ldr < C)) return RDETR_ERR_INVALID_ARG;
    if (C != 256) return RDETR_ERR_UNSUPPORTED;
    if (rows == 0) return RDETR_OK;
    if (!x || !gamma || !beta || !out || !stats) return RDETR_ERR_INVALID_ARG;
    const long long nblk = (rows + kLnWaves * kLnRowsPerWave - 1) / (kLnWaves * kLnRowsPerWave);
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    constexpr int eb = (int)sizeof(T);
    if (!(rows_ok(x, ldx, C, eb) && rows_ok(out, ldo, C, eb) && all_aligned(16, gamma, beta) && (!r || rows_ok(r, ldr, C, eb)) &&
          aligned_to(stats, 8)))
        return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((add_layernorm256_train_kernel<T>), dim3((unsigned)nblk), dim3(kLnWaves * kWave), 0, stream, x, r, gamma, beta,
                       rows, ldx, ldr, ldo, eps, out, stats);
    return launch_status();
}

// Backward of out = LayerNorm(x + r) * gamma + beta from the saved {mean, rstd}, C == 256, the forward's layout (half a wave per
// row, a lane 8 channels, a wave 4 rows with every load issued before the first use):
//     xhat = (x + r - mean) * rstd   (the sum in fp32, not rounded, as the forward formed it)      g = dy * gamma
//     dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat))       -- ONE tensor: the gradient of x and of r
//     dgamma = sum_rows dy * xhat                                 dbeta = sum_rows dy
// A bounded grid (kLnBwdMaxBlocks) walks the 16-row blocks with a grid stride; a lane keeps its 8 + 8 fp32 partial sums of dgamma /
// dbeta in registers across trips, the workgroup adds its 8 half-waves through LDS in index order and writes ONE [2, 256] partial;
// ln_param_grad_kernel then adds the partials in index order.  No atomics: the same bits every run.
// Bound: HBM (4 x rows x C x sizeof(T) bytes; the partials are at most 2 MiB).
constexpr int kLnBwdMaxBlocks = 4 * kCus;  // 4 workgroups (16 waves) on each CU: 24 KB of bf16 loads per CU and trip

// T is the type of dy, gamma and dx; TX / TR those of x and the residual (all T in the same-dtype kernels).  kTwin (the
// mixed-precision backward, T = float): dx may be null, and dxb, where it is not null, receives the same values rounded to bf16 (RNE)
// in the same pass -- the gradient of a bf16 operand beside the fp32 one.
template <typename T, bool kParams, typename TX, typename TR, bool kTwin>
__device__ __forceinline__ void add_layernorm256_bwd_body(const T *__restrict__ dy, long long lddy, const TX *__restrict__ x,
                                                          long long ldx, const TR *__restrict__ r, long long ldr,
                                                          const T *__restrict__ gamma, const float *__restrict__ stats, long long rows,
                                                          long long nblk, T *__restrict__ dx, uint16_t *__restrict__ dxb,
                                                          float *__restrict__ partial)
{
    __shared__ float red[kLnWaves * 2][2][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, c = (lane & 31) * 8;
    float g[8], ag[8], ab[8];
    LnIO8<T>::load(gamma + c, g);
#pragma unroll
    for (int k = 0; k < 8; ++k) ag[k] = ab[k] = 0.f;
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long long row0 = (blk * kLnWaves + wave) * kLnRowsPerWave + half;
        float d[2][8], v[2][8], mean[2], rstd[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long row = row0 + 2 * i;
            if (row < rows) {
                LnIO8<T>::load(dy + row * lddy + c, d[i]);
                LnIO8<TX>::load(x + row * ldx + c, v[i]);
                const f32x2 st = *reinterpret_cast<const f32x2 *>(stats + row * 2);
                mean[i] = st.x;
                rstd[i] = st.y;
            } else {                         // a row past the end: dy = 0 adds nothing to the parameter sums, nothing is stored
#pragma unroll
                for (int k = 0; k < 8; ++k) d[i][k] = v[i][k] = 0.f;
                mean[i] = rstd[i] = 0.f;
            }
        }
        if (r) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const long long row = row0 + 2 * i;
                if (row < rows) {
                    float t[8];
                    LnIO8<TR>::load(r + row * ldr + c, t);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[i][k] += t[k];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long row = row0 + 2 * i;
            float gg[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                v[i][k] = (v[i][k] - mean[i]) * rstd[i];              // xhat
                gg[k] = d[i][k] * g[k];
                s1 += gg[k];
                s2 += gg[k] * v[i][k];
            }
            const float m1 = row256_half_sum(s1) * (1.0f / 256.0f), m2 = row256_half_sum(s2) * (1.0f / 256.0f);
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = rstd[i] * (gg[k] - m1 - v[i][k] * m2);
            if constexpr (kTwin) {
                if (row < rows) {
                    if (dx) LnIO8<T>::store(dx + row * 256 + c, o);
                    if (dxb) LnIO8<uint16_t>::store(dxb + row * 256 + c, o);
                }
            } else {
                if (row < rows) LnIO8<T>::store(dx + row * 256 + c, o);
            }
            if constexpr (kParams) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    ag[k] += d[i][k] * v[i][k];
                    ab[k] += d[i][k];
                }
            }
        }
    }
    if constexpr (kParams) {
        const int hw = wave * 2 + half;
        *reinterpret_cast<f32x4 *>(&red[hw][0][c]) = f32x4{ag[0], ag[1], ag[2], ag[3]};
        *reinterpret_cast<f32x4 *>(&red[hw][0][c + 4]) = f32x4{ag[4], ag[5], ag[6], ag[7]};
        *reinterpret_cast<f32x4 *>(&red[hw][1][c]) = f32x4{ab[0], ab[1], ab[2], ab[3]};
        *reinterpret_cast<f32x4 *>(&red[hw][1][c + 4]) = f32x4{ab[4], ab[5], ab[6], ab[7]};
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {                              // 256 threads, 512 sums: (which, channel) = (j, threadIdx.x)
            float s = 0.f;
#pragma unroll
            for (int h = 0; h < kLnWaves * 2; ++h) s += red[h][j][threadIdx.x];
            partial[(long long)blockIdx.x * 512 + j * 256 + threadIdx.x] = s;
        }
    }
}

template <typename T, bool kParams>
__global__ __launch_bounds__(kLnWaves *kWave) void add_layernorm256_bwd_kernel(const T *__restrict__ dy, long long lddy,
                                                                               const T *__restrict__ x, long long ldx,
                                                                               const T *__restrict__ r, long long ldr,
                                                                               const T *__restrict__ gamma,
                                                                               const float *__restrict__ stats, long long rows,
                                                                               long long nblk, T *__restrict__ dx,
                                                                               float *__restrict__ partial)
{
    add_layernorm256_bwd_body<T, kParams, T, T, false>(dy, lddy, x, ldx, r, ldr, gamma, stats, rows, nblk, dx, nullptr, partial);
}

template <typename TX, typename TR, bool kParams>
__global__ __launch_bounds__(kLnWaves *kWave) void add_layernorm256_bwd_mixed_kernel(const float *__restrict__ dy, long long lddy,
                                                                                     const TX *__restrict__ x, long long ldx,
                                                                                     const TR *__restrict__ r, long long ldr,
                                                                                     const float *__restrict__ gamma,
                                                                                     const float *__restrict__ stats, long long rows,
                                                                                     long long nblk, float *__restrict__ dx,
                                                                                     uint16_t *__restrict__ dxb,
                                                                                     float *__restrict__ partial)
{
    add_layernorm256_bwd_body<float, kParams, TX, TR, true>(dy, lddy, x, ldx, r, ldr, gamma, stats, rows, nblk, dx, dxb, partial);
}

// dgamma / dbeta from the workgroups' partials [n, 2, 256]: one workgroup, thread t owns (which, channel) = (t / 256, t % 256) and
// adds the n values in index order.  One CU reads up to 2 MiB here, so the loop is bound by the loads it keeps in flight: 32 per
// thread, and the next 32 are issued before the current ones are added (an index past the end reads the last partial and adds 0).
constexpr int kLnGradBatch = 32;

template <typename T>
__global__ __launch_bounds__(512) void ln_param_grad_kernel(const float *__restrict__ partial, int n, T *__restrict__ dgamma,
                                                            T *__restrict__ dbeta)
{
    const int t = threadIdx.x;
    const float *col = partial + t;
    float cur[kLnGradBatch], nxt[kLnGradBatch], s = 0.f;
#pragma unroll
    for (int j = 0; j < kLnGradBatch; ++j) cur[j] = col[(long long)(j < n ? j : n - 1) * 512];
    for (int p0 = 0; p0 < n; p0 += kLnGradBatch) {
        const int q0 = p0 + kLnGradBatch;
        if (q0 < n) {
#pragma unroll
            for (int j = 0; j < kLnGradBatch; ++j) nxt[j] = col[(long long)(q0 + j < n ? q0 + j : n - 1) * 512];
        }
#pragma unroll
        for (int j = 0; j < kLnGradBatch; ++j) s += p0 + j < n ? cur[j] : 0.f;
#pragma unroll
        for (int j = 0; j < kLnGradBatch; ++j) cur[j] = nxt[j];
    }
    LnIO<T>::store1((t < 256 ? dgamma : dbeta) + (t & 255), s);
}

static long long ln_backward_blocks(long long rows)
{
    const long long nblk = (rows + kLnWaves * kLnRowsPerWave - 1) / (kLnWaves * kLnRowsPerWave);
    return nblk < kLnBwdMaxBlocks ? nblk : kLnBwdMaxBlocks;
}

template <typename T>
static int add_layernorm_backward(const T *dy, long long lddy, const T *x, long long ldx, const T *r, long long ldr, const T *gamma,
                                  const float *stats, long long rows, int C, void *workspace, long long workspace_bytes, T *dx,
                                  T *dgamma, T *dbeta, hipStream_t stream)
{
    if (rows < 0 || C <= 0 || lddy < C || ldx < C || (r && ldr < C) || workspace_bytes < 0) return RDETR_ERR_INVALID_ARG;
    if ((dgamma != nullptr) != (dbeta != nullptr)) return RDETR_ERR_INVALID_ARG;
    if (C != 256) return RDETR_ERR_UNSUPPORTED;
    if (rows == 0) return RDETR_OK;
    if (!dy || !x || !gamma || !stats || !dx) return RDETR_ERR_INVALID_ARG;
    const long long nblk = (rows + kLnWaves * kLnRowsPerWave - 1) / (kLnWaves * kLnRowsPerWave), grid = ln_backward_blocks(rows);
    if (dgamma && (!workspace || workspace_bytes < grid * 512 * (long long)sizeof(float))) return RDETR_ERR_INVALID_ARG;
    constexpr int eb = (int)sizeof(T);
    if (!(rows_ok(dy, lddy, C, eb) && rows_ok(x, ldx, C, eb) && all_aligned(16, dx, gamma) && (!r || rows_ok(r, ldr, C, eb)) &&
          aligned_to(stats, 8) && (!dgamma || aligned_to(workspace, 16))))
        return RDETR_ERR_UNSUPPORTED;
    if (dgamma) {
        float *partial = static_cast<float *>(workspace);
        hipLaunchKernelGGL((add_layernorm256_bwd_kernel<T, true>), dim3((unsigned)grid), dim3(kLnWaves * kWave), 0, stream, dy, lddy, x,
                           ldx, r, ldr, gamma, stats, rows, nblk, dx, partial);
        if (launch_status() != RDETR_OK) return RDETR_ERR_LAUNCH;
        hipLaunchKernelGGL((ln_param_grad_kernel<T>), dim3(1), dim3(512), 0, stream, partial, (int)grid, dgamma, dbeta);
    } else {
        hipLaunchKernelGGL((add_layernorm256_bwd_kernel<T, false>), dim3((unsigned)grid), dim3(kLnWaves * kWave), 0, stream, dy, lddy, x,
                           ldx, r, ldr, gamma, stats, rows, nblk, dx, static_cast<float *>(nullptr));
    }
    return launch_status();
}

// ------------------------------------------------------------------------------------------------- mixed-precision training
// The routes above under bf16 autocast over fp32 parameters: x and the residual are each fp32 or bf16 (the residual stream is
// fp32, a sublayer's linear output bf16), gamma / beta / out / dy fp32.  One launcher per direction, instantiated for the four
// operand-type pairs; the argument checks are those of the same-dtype routes with each operand on its own 16-byte grid.

template <typename TX, typename TR>
static void ln_train_mixed_launch(const void *x, const void *r, const float *gamma, const float *beta, long long rows, long long ldx,
                                  long long ldr, long long ldo, float eps, float *out, float *stats, unsigned nblk, hipStream_t stream)
{
    hipLaunchKernelGGL((add_layernorm256_train_mixed_kernel<TX, TR>), dim3(nblk), dim3(kLnWaves * kWave), 0, stream,
                       static_cast<const TX *>(x), static_cast<const TR *>(r), gamma, beta, rows, ldx, ldr, ldo, eps, out, stats);
}

static int add_layernorm_train_mixed(const void *x, bool xb, long long ldx, const void *r, bool rb, long long ldr, const float *gamma,
                                     const float *beta, long long rows, int C, float eps, float *out, long long ldo, float *stats,
                                     hipStream_t stream)
{
    if (rows < 0 || C <= 0 || ldx < C || ldo < C || (r && ldr < C)) return RDETR_ERR_INVALID_ARG;
    if (C != 256) return RDETR_ERR_UNSUPPORTED;
    if (rows == 0) return RDETR_OK;
    if (!x || !gamma || !beta || !out || !stats) return RDETR_ERR_INVALID_ARG;
    const long long nblk = (rows + kLnWaves * kLnRowsPerWave - 1) / (kLnWaves * kLnRowsPerWave);
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    if (!(rows_ok(x, ldx, C, xb ? 2 : 4) && rows_ok(out, ldo, C, 4) && (!r || rows_ok(r, ldr, C, rb ? 2 : 4)) && all_aligned(16, gamma, beta) &&
          aligned_to(stats, 8)))
        return RDETR_ERR_UNSUPPORTED;
    auto *launch = xb ? (rb ? ln_train_mixed_launch<uint16_t, uint16_t> : ln_train_mixed_launch<uint16_t, float>)
                      : (rb ? ln_train_mixed_launch<float, uint16_t> : ln_train_mixed_launch<float, float>);
    launch(x, r, gamma, beta, rows, ldx, ldr, ldo, eps, out, stats, (unsigned)nblk, stream);
    return launch_status();
}

template <typename TX, typename TR>
static void ln_bwd_mixed_launch(const float *dy, long long lddy, const void *x, long long ldx, const void *r, long long ldr,
                                const float *gamma, const float *stats, long long rows, long long nblk, float *dx, uint16_t *dxb,
                                float *partial, unsigned grid, hipStream_t stream)
{
    if (partial)
        hipLaunchKernelGGL((add_layernorm256_bwd_mixed_kernel<TX, TR, true>), dim3(grid), dim3(kLnWaves * kWave), 0, stream, dy, lddy,
                           static_cast<const TX *>(x), ldx, static_cast<const TR *>(r), ldr, gamma, stats, rows, nblk, dx, dxb, partial);
    else
        hipLaunchKernelGGL((add_layernorm256_bwd_mixed_kernel<TX, TR, false>), dim3(grid), dim3(kLnWaves * kWave), 0, stream, dy, lddy,
                           static_cast<const TX *>(x), ldx, static_cast<const TR *>(r), ldr, gamma, stats, rows, nblk, dx, dxb, partial);
}

static int add_layernorm_backward_mixed(const float *dy, long long lddy, const void *x, bool xb, long long ldx, const void *r, bool rb,
                                        long long ldr, const float *gamma, const float *stats, long long rows, int C, void *workspace,
                                        long long workspace_bytes, float *dx, uint16_t *dxb, float *dgamma, float *dbeta,
                                        hipStream_t stream)
{
    if (rows < 0 || C <= 0 || lddy < C || ldx < C || (r && ldr < C) || workspace_bytes < 0) return RDETR_ERR_INVALID_ARG;
    if ((dgamma != nullptr) != (dbeta != nullptr)) return RDETR_ERR_INVALID_ARG;
    if (C != 256) return RDETR_ERR_UNSUPPORTED;
    if (rows == 0) return RDETR_OK;
    if (!dy || !x || !gamma || !stats) return RDETR_ERR_INVALID_ARG;
    // a gradient for every operand in its own type: the bf16 twin where an operand is bf16, the fp32 tensor where one is fp32
    const bool any_bf16 = xb || (r && rb), any_f32 = !xb || (r && !rb);
    if ((any_bf16 && !dxb) || (any_f32 && !dx)) return RDETR_ERR_INVALID_ARG;
    const long long nblk = (rows + kLnWaves * kLnRowsPerWave - 1) / (kLnWaves * kLnRowsPerWave), grid = ln_backward_blocks(rows);
    if (dgamma && (!workspace || workspace_bytes < grid * 512 * (long long)sizeof(float))) return RDETR_ERR_INVALID_ARG;
    if (!(rows_ok(dy, lddy, C, 4) && rows_ok(x, ldx, C, xb ? 2 : 4) && (!r || rows_ok(r, ldr, C, rb ? 2 : 4)) && all_aligned(16, gamma, dx, dxb) &&
          aligned_to(stats, 8) && (!dgamma || aligned_to(workspace, 16))))
        return RDETR_ERR_UNSUPPORTED;
    float *partial = dgamma ? static_cast<float *>(workspace) : nullptr;
    auto *launch = xb ? (rb ? ln_bwd_mixed_launch<uint16_t, uint16_t> : ln_bwd_mixed_launch<uint16_t, float>)
                      : (rb ? ln_bwd_mixed_launch<float, uint16_t> : ln_bwd_mixed_launch<float, float>);
    launch(dy, lddy, x, ldx, r, ldr, gamma, stats, rows, nblk, dx, dxb, partial, (unsigned)grid, stream);
    if (dgamma) {
        if (launch_status() != RDETR_OK) return RDETR_ERR_LAUNCH;
        hipLaunchKernelGGL((ln_param_grad_kernel<float>), dim3(1), dim3(512), 0, stream, partial, (int)grid, dgamma, dbeta);
    }
    return launch_status();
}

}  // namespace rdetr

extern "C" int rdetr_add_layernorm_train_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                                             long long rows, int C, long long ldx, long long ldr, long long ldo, float eps, float *out,
                                             float *stats, void *stream)
{
    return rdetr::add_layernorm_train<float>(x, residual, gamma, beta, rows, C, ldx, ldr, ldo, eps, out, stats,
                                             static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_train_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma, const uint16_t *beta,
                                              long long rows, int C, long long ldx, long long ldr, long long ldo, float eps,
                                              uint16_t *out, float *stats, void *stream)
{
    return rdetr::add_layernorm_train<uint16_t>(x, residual, gamma, beta, rows, C, ldx, ldr, ldo, eps, out, stats,
                                                static_cast<hipStream_t>(stream));
}

extern "C" long long rdetr_add_layernorm_backward_workspace_bytes(long long rows)
{
    return rows <= 0 ? 0 : rdetr::ln_backward_blocks(rows) * 512 * (long long)sizeof(float);
}

extern "C" int rdetr_add_layernorm_backward_f32(const float *dy, long long lddy, const float *x, long long ldx, const float *residual,
                                                long long ldr, const float *gamma, const float *stats, long long rows, int C,
                                                void *workspace, long long workspace_bytes, float *dx, float *dgamma, float *dbeta,
                                                void *stream)
{
    return rdetr::add_layernorm_backward<float>(dy, lddy, x, ldx, residual, ldr, gamma, stats, rows, C, workspace, workspace_bytes, dx,
                                                dgamma, dbeta, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_backward_bf16(const uint16_t *dy, long long lddy, const uint16_t *x, long long ldx,
                                                 const uint16_t *residual, long long ldr, const uint16_t *gamma, const float *stats,
                                                 long long rows, int C, void *workspace, long long workspace_bytes, uint16_t *dx,
                                                 uint16_t *dgamma, uint16_t *dbeta, void *stream)
{
    return rdetr::add_layernorm_backward<uint16_t>(dy, lddy, x, ldx, residual, ldr, gamma, stats, rows, C, workspace, workspace_bytes,
                                                   dx, dgamma, dbeta, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_train_mixed(const void *x, int x_is_bf16, long long ldx, const void *residual, int r_is_bf16,
                                               long long ldr, const float *gamma, const float *beta, long long rows, int C, float eps,
                                               float *out, long long ldo, float *stats, void *stream)
{
    return rdetr::add_layernorm_train_mixed(x, x_is_bf16 != 0, ldx, residual, r_is_bf16 != 0, ldr, gamma, beta, rows, C, eps, out, ldo,
                                            stats, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_backward_mixed(const float *dy, long long lddy, const void *x, int x_is_bf16, long long ldx,
                                                  const void *residual, int r_is_bf16, long long ldr, const float *gamma,
                                                  const float *stats, long long rows, int C, void *workspace, long long workspace_bytes,
                                                  float *dx, uint16_t *dx_bf16, float *dgamma, float *dbeta, void *stream)
{
    return rdetr::add_layernorm_backward_mixed(dy, lddy, x, x_is_bf16 != 0, ldx, residual, r_is_bf16 != 0, ldr, gamma, stats, rows, C,
                                               workspace, workspace_bytes, dx, dx_bf16, dgamma, dbeta, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                                       long long rows, int C, float eps, float *out, void *stream)
{
    return rdetr::add_layernorm<float>(x, residual, gamma, beta, rows, C, C, C, C, eps, out, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_strided_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                                               long long rows, int C, long long ldx, long long ldr, long long ldo, float eps,
                                               float *out, void *stream)
{
    return rdetr::add_layernorm<float>(x, residual, gamma, beta, rows, C, ldx, ldr, ldo, eps, out, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma,
                                        const uint16_t *beta, long long rows, int C, float eps, uint16_t *out, void *stream)
{
    return rdetr::add_layernorm<uint16_t>(x, residual, gamma, beta, rows, C, C, C, C, eps, out, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_strided_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma,
                                                const uint16_t *beta, long long rows, int C, long long ldx, long long ldr,
                                                long long ldo, float eps, uint16_t *out, void *stream)
{
    return rdetr::add_layernorm<uint16_t>(x, residual, gamma, beta, rows, C, ldx, ldr, ldo, eps, out,
                                          static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_add_layernorm_pos_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                                           const float *pos, long long rows, int C, long long ldx, long long ldr, long long ldo,
                                           long long ldp, long long ldo2, float eps, float *out, float *out2, void *stream)
{
    if (!pos || !out2) return RDETR_ERR_INVALID_ARG;
    return rdetr::add_layernorm<float>(x, residual, gamma, beta, rows, C, ldx, ldr, ldo, eps, out, static_cast<hipStream_t>(stream),
                                       pos, ldp, out2, ldo2);
}

extern "C" int rdetr_add_layernorm_pos_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma,
                                            const uint16_t *beta, const uint16_t *pos, long long rows, int C, long long ldx,
                                            long long ldr, long long ldo, long long ldp, long long ldo2, float eps, uint16_t *out,
                                            uint16_t *out2, void *stream)
{
    if (!pos || !out2) return RDETR_ERR_INVALID_ARG;
    return rdetr::add_layernorm<uint16_t>(x, residual, gamma, beta, rows, C, ldx, ldr, ldo, eps, out,
                                          static_cast<hipStream_t>(stream), pos, ldp, out2, ldo2);
}
