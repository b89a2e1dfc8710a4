// Fused feed-forward block for bf16 activations with embed_dim 256 on gfx950:
//     out = (relu(X W1^T + b1)) W2^T + b2          X [M, 256], W1 [F, 256], W2 [256, F], F = d_ffn (a multiple of 64)
// i.e. linear2(relu(linear1(x))) of the encoder / decoder layers (models/bricks/relation_transformer.py:226-233, 272-275) without
// the [M, F] round trip through HBM (732 MB per encoder layer at B = 4: written by one library GEMM, read by the next).
//
//   workgroup   512 threads = 8 waves, persistent over tiles of 256 rows; a wave owns 32 rows for the whole block
//   hidden dim  walked in chunks of 64 units; the chunk's slices of W1 (64 x 256) and W2 (256 x 64) are brought L2 -> LDS by
//               LDS-DMA in MFMA-fragment order (one instruction = one 1-KiB A fragment), double buffered, one barrier per chunk
//   GEMM 1      H^T[hidden x rows] = W1c X^T: A = W1 fragments (LDS), B = X^T from registers (loaded once per row tile).  The
//               chunk's hidden units are permuted over the tiles so that after two tiles lane (row, g) holds hidden units
//               32 u + 8 g .. + 7 of its row -- which, after bias + ReLU + rounding to bf16, IS the B operand of
//   GEMM 2      out^T[256 x rows] += W2c H^T with k = those 32 hidden units: nothing moves between lanes, H never leaves
//               registers.  The 256 outputs are permuted over the 16 tiles the same way, so a lane ends with 8 consecutive
//               outputs per tile pair = one 16-byte store.
//   math        v_mfma_f32_16x16x32_bf16, fp32 accumulation; H is rounded to bf16 exactly where the unfused path stores it
// Bound: MFMA (4096 per 32 rows and wave); LDS reads at half their peak beside it.
// Training (bf16): the same body (ffn_k256_body.h) also stores H for the backward, and, with (dY, W2^T, W1^T) in the places of
// (X, W1, W2) and a masking epilogue instead of bias + ReLU, computes dH and dX (ffn_k256_train_kernel).
#include <cstdlib>
#include <utility>

#include "launch.h"

namespace rdetr {

typedef __bf16 ffn_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kFfnK = 256;                 // embed_dim: K of GEMM 1, N of GEMM 2
constexpr int kFfnThreads = 512;
constexpr int kFfnWaves = kFfnThreads / 64;
constexpr int kFfnRows = 32;               // rows per wave
constexpr int kFfnHC = 64;                 // hidden units per chunk
constexpr int kFfnW1Bytes = kFfnHC * kFfnK * 2;          // 32 KiB: [4 tiles][8 k-steps][64 lanes] x 16 B
constexpr int kFfnW2Bytes = kFfnK * kFfnHC * 2;          // 32 KiB: [16 out tiles][2 k-steps][64 lanes] x 16 B
constexpr int kFfnBufBytes = kFfnW1Bytes + kFfnW2Bytes;
constexpr int kFfnMaxLdsBytes = 2 * kFfnBufBytes + (4096 + 3 * kFfnK) * 4;      // dynamic LDS at the largest F served

// fn(integral_constant<0>) ... fn(integral_constant<N - 1>)
template <int... I, class Fn>
__device__ __forceinline__ void ffn_static_for(std::integer_sequence<int, I...>, Fn &&fn)
{
    (fn(std::integral_constant<int, I>{}), ...);
}

// slot of a 16-wide tile sequence that carries index i (i = 32 u + 8 g + 4 e + r  <->  tile 2u + e, row 4g + r)
__device__ __forceinline__ int ffn_index(int tile, int m) { return 32 * (tile >> 1) + 8 * (m >> 2) + 4 * (tile & 1) + (m & 3); }

// 0xffff in each half whose bf16 is > 0 (as int16: min(max(h, 0), 1) is 0 or 1; 0 - that is the mask)
__device__ __forceinline__ unsigned int positive_bf16x2(unsigned int packed)
{
    const s16x2_t one = {1, 1}, zero = {0, 0};
    const s16x2_t b = __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(s16x2_t, packed), zero), one);
    return __builtin_bit_cast(unsigned int, zero - b);
}

// pack_bf16x2 as a conversion of the pair: the two scalar conversions of pack_bf16x2 become two v_cvt_pk_bf16_f32 and a v_perm_b32
// in the chunk loop, this form one v_cvt_pk_bf16_f32 with both sources (the same rounding of each half)
__device__ __forceinline__ unsigned int ffn_pack_bf16x2(float a, float b)
{
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(f32x2{a, b}, bf16x2_t));
}

// what the kernel body does around the two GEMMs
constexpr int kFfnInfer = 0;               // out only (rdetr_ffn_k256_bf16, rdetr_ffn_ln_k256_bf16)
constexpr int kFfnTrain = 1;               // ... and the hidden activations H [M, F] stored for backward
constexpr int kFfnBwd = 2;                 // data gradient: x = dY, packed = (W2^T, W1^T), no biases; the hidden epilogue rounds
                                           // dY W2, zeroes it where the saved H is not positive, stores it as dH: out = dX

// Step order of the inference kernels (ffn_k256_body.h): the activations cut into slices behind the MFMAs of the next 16 steps and
// the weight stream of the next chunk issued piece by piece.  The development library (make dev) gives them the order of the
// training kernels instead, each activation whole at one step and the 8 pieces back to back: its component-timing bits are
// branches, and the spread loop has no register left for a branch (one around each piece sent 22 registers to scratch).  Without
// a bit set that kernel runs the schedule the spread order replaced (profiles/r22/README.md).
#ifdef RDETR_DEV
constexpr bool kFfnSpread = false;
#else
constexpr bool kFfnSpread = true;
#endif
constexpr int kFfnDmaFirst = 3, kFfnDmaEvery = 2;          // piece i of the next chunk goes out after step First + i Every
static_assert(kFfnDmaFirst >= 3 && kFfnDmaEvery >= 1 && kFfnDmaFirst + 7 * kFfnDmaEvery < 64, "pieces inside the chunk, behind its barrier");

// H / dH are addressed through a buffer resource (SGPRs): the 16-row block's first row and the chunk's column are the scalar
// offset, the lane's row and column inside the block a 32-bit vector offset -- no 64-bit row pointers inside the chunk loop, which
// has no registers to spare.  A row at or beyond M carries kFfnNoRow instead: with at most 2^31 - 1 bytes behind the resource
// (the launchers refuse more) that offset, with or without the scalar part (itself inside the resource) added, lies beyond the
// end without wrapping, and the hardware drops the access.
constexpr unsigned kFfnNoRow = 0x80000000u;

template <bool LN>
__global__ __launch_bounds__(kFfnThreads) void ffn_k256_kernel(const uint16_t *__restrict__ x, long long ldx,
                                                               const uint16_t *__restrict__ packed, const uint16_t *__restrict__ b1,
                                                               const uint16_t *__restrict__ b2,
                                                               long long M, int F, uint16_t *__restrict__ out, long long ldo, int dbg_arg,
                                                               const uint16_t *__restrict__ gamma, const uint16_t *__restrict__ beta,
                                                               float eps, const uint16_t *__restrict__ pos, long long ldp,
                                                               uint16_t *__restrict__ out2, long long ldo2)
{
    constexpr int MODE = kFfnInfer;
    constexpr bool XF32 = false, DXF32 = false;
    uint16_t *const hid = nullptr, *const dhid = nullptr, *const xlp = nullptr;
    constexpr long long ldh = 0, ldd = 0, ldxl = 0;
    const float *const xf = nullptr;
    float *const outf = nullptr;
#include "ffn_k256_body.h"
}

// MODE = kFfnTrain: out and H = relu(bf16(x W1^T + b1)) [M, F] (hid, ldh).  MODE = kFfnBwd: x = dY, packed = (W2^T, W1^T), hid = the
// saved H (read), dhid = dH [M, F] (written), out = dX
template <int MODE>
__global__ __launch_bounds__(kFfnThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void ffn_k256_train_kernel(const uint16_t *__restrict__ x, long long ldx,
                                                                     const uint16_t *__restrict__ packed, const uint16_t *__restrict__ b1,
                                                                     const uint16_t *__restrict__ b2, long long M, int F,
                                                                     uint16_t *__restrict__ out, long long ldo, uint16_t *hid, long long ldh,
                                                                     uint16_t *dhid, long long ldd)
{
    constexpr bool LN = false;
    [[maybe_unused]] constexpr int dbg_arg = 0;
    constexpr float eps = 0.f;
    constexpr long long ldp = 0, ldo2 = 0;
    const uint16_t *const gamma = nullptr, *const beta = nullptr, *const pos = nullptr;
    uint16_t *const out2 = nullptr;
    constexpr bool XF32 = false, DXF32 = false;
    uint16_t *const xlp = nullptr;
    constexpr long long ldxl = 0;
    const float *const xf = nullptr;
    float *const outf = nullptr;
#include "ffn_k256_body.h"
}

// The training kernels with fp32 at one end of the block (bf16 autocast over an fp32 residual stream).  MODE = kFfnTrain: the rows
// are read as fp32 (xin), rounded to bf16 on the way into the registers and stored as xlp [M, 256]; from there on the kernel above,
// so out and hid have its bits on the rounded x.  MODE = kFfnBwd: dX leaves as the unrounded fp32 accumulators (outp); dH as above.
template <int MODE>
__global__ __launch_bounds__(kFfnThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void ffn_k256_train_f32_kernel(const void *__restrict__ xin, long long ldx,
                                                                     const uint16_t *__restrict__ packed, const uint16_t *__restrict__ b1,
                                                                     const uint16_t *__restrict__ b2, long long M, int F,
                                                                     void *__restrict__ outp, long long ldo, uint16_t *hid, long long ldh,
                                                                     uint16_t *dhid, long long ldd, uint16_t *__restrict__ xlp, long long ldxl)
{
    constexpr bool LN = false;
    [[maybe_unused]] constexpr int dbg_arg = 0;
    constexpr float eps = 0.f;
    constexpr long long ldp = 0, ldo2 = 0;
    const uint16_t *const gamma = nullptr, *const beta = nullptr, *const pos = nullptr;
    uint16_t *const out2 = nullptr;
    constexpr bool XF32 = MODE == kFfnTrain, DXF32 = MODE == kFfnBwd;
    const uint16_t *const x = static_cast<const uint16_t *>(xin);
    const float *const xf = static_cast<const float *>(xin);
    uint16_t *const out = static_cast<uint16_t *>(outp);
    float *const outf = static_cast<float *>(outp);
#include "ffn_k256_body.h"
}

// Weights -> fragment order, once per weight update: packed[chunk][fragment f][lane][8 bf16] with, for lane (m = lane & 15,
// kb = lane >> 4):  f < 32: W1[64 chunk + index(f >> 3, m)][32 (f & 7) + 8 kb ..]   (GEMM 1: tile f >> 3, k-step f & 7)
//                   f >= 32: W2[index((f - 32) >> 1, m)][64 chunk + 32 (f & 1) + 8 kb ..]   (GEMM 2: out tile, k-step)
__global__ __launch_bounds__(256) void ffn_pack_kernel(const uint16_t *__restrict__ w1, const uint16_t *__restrict__ w2, int F,
                                                       u32x4 *__restrict__ packed)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;                           // one 16-byte piece
    const int total = (F / kFfnHC) * 64 * 64;
    if (idx >= total) return;
    const int c = idx >> 12, f = (idx >> 6) & 63, l = idx & 63, m = l & 15, kb = l >> 4;
    const uint16_t *src;
    if (f < 32) src = w1 + (size_t)(c * kFfnHC + ffn_index(f >> 3, m)) * kFfnK + 32 * (f & 7) + 8 * kb;
    else src = w2 + (size_t)ffn_index((f - 32) >> 1, m) * F + c * kFfnHC + 32 * (f & 1) + 8 * kb;
    packed[idx] = *reinterpret_cast<const u32x4 *>(src);
}

// The same fragment order from fp32 weights read through element strides (rows, columns), rounded to bf16 (RNE) on the way: the
// forward's (w1, w2) as they lie, and the backward's (w2^T, w1^T) read in place -- no bf16 copies, no transposes.
//   workgroup (c, half)  one chunk's 64 x 256 slice of W1 (half 0) or 256 x 64 slice of W2 (half 1), through LDS:
//   load    consecutive threads walk the dimension whose stride is smaller (`row_fast`: a transposed view), so a wave reads whole
//           256-byte runs either way; rows that are contiguous, 16-byte aligned floats (`vec`) take 16-byte loads.  The values are
//           rounded here and kept as bf16 [rows][cols + 2]: an odd number of banks per row, whichever way the tile is written
//   store   a thread gathers its 16-byte pieces (8 consecutive columns of one row) from LDS: the stores stay the 1-KiB fragments
// The workgroups behind the last chunk round the biases: dst[0 .. F) = b1, dst[F .. F + 256) = b2.
constexpr int kFfnPackLd1 = kFfnK + 2, kFfnPackLd2 = kFfnHC + 2;           // bf16 elements per LDS row of the W1 / W2 tile

__global__ __launch_bounds__(256) void ffn_pack_f32_kernel(const float *__restrict__ w1, long long rs1, long long cs1, int mode1,
                                                           const float *__restrict__ w2, long long rs2, long long cs2, int mode2,
                                                           const float *__restrict__ b1, const float *__restrict__ b2, int F,
                                                           u32x4 *__restrict__ packed, uint16_t *__restrict__ biases)
{
    __shared__ __attribute__((aligned(16))) uint16_t tile[kFfnK * kFfnPackLd2];            // >= 64 * kFfnPackLd1
    static_assert(kFfnK * kFfnPackLd2 >= kFfnHC * kFfnPackLd1, "one LDS tile serves both halves");
    const int t = threadIdx.x, nchunks = F / kFfnHC;
    if ((int)blockIdx.x >= 2 * nchunks) {
        const int i = ((int)blockIdx.x - 2 * nchunks) * 256 + t;
        if (biases && i < F + kFfnK) biases[i] = (uint16_t)f32_to_bf16_bits(i < F ? b1[i] : b2[i - F]);
        return;
    }
    const int c = blockIdx.x >> 1, half = blockIdx.x & 1;
    // the tile: `rows` x `cols` elements from (row0, col0) of the matrix; cols = 1 << lc, rows = 1 << lr
    const float *src = half ? w2 + (long long)c * kFfnHC * cs2 : w1 + (long long)c * kFfnHC * rs1;
    const long long rs = half ? rs2 : rs1, cs = half ? cs2 : cs1;
    const int mode = half ? mode2 : mode1, lc = half ? 6 : 8, lr = half ? 8 : 6, ld = half ? kFfnPackLd2 : kFfnPackLd1;
    if (mode == 2) {                                                      // contiguous, aligned rows: 16-byte loads
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int e = i * 256 + t, row = e >> (lc - 2), col = (e & ((1 << (lc - 2)) - 1)) * 4;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(src + row * rs + col);
            unsigned *q = reinterpret_cast<unsigned *>(&tile[row * ld + col]);             // 4-byte aligned only: two stores
            q[0] = pack_bf16x2(v.x, v.y);
            q[1] = pack_bf16x2(v.z, v.w);
        }
    } else {
#pragma unroll 8
        for (int i = 0; i < 64; ++i) {
            const int e = i * 256 + t;
            const int row = mode == 1 ? e & ((1 << lr) - 1) : e >> lc, col = mode == 1 ? e >> lr : e & ((1 << lc) - 1);
            tile[row * ld + col] = (uint16_t)f32_to_bf16_bits(src[row * rs + col * cs]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = j * 256 + t, f = p >> 6, l = p & 63, m = l & 15, kb = l >> 4;          // fragment f of this half, lane l
        const int row = half ? ffn_index(f >> 1, m) : ffn_index(f >> 3, m), col = half ? 32 * (f & 1) + 8 * kb : 32 * (f & 7) + 8 * kb;
        const unsigned *q = reinterpret_cast<const unsigned *>(&tile[row * ld + col]);     // 4-byte aligned: ld and col are even
        packed[(size_t)c * 4096 + half * 2048 + p] = u32x4{q[0], q[1], q[2], q[3]};
    }
}

}  // namespace rdetr

using namespace rdetr;

// packed <- (w1 [F, 256], w2 [256, F]) in the fragment order rdetr_ffn_k256_bf16 streams (2 * 256 * F bf16 elements)
extern "C" int rdetr_ffn_k256_pack_bf16(const uint16_t *w1, const uint16_t *w2, int F, uint16_t *packed, void *stream)
{
    if (F <= 0) return RDETR_ERR_INVALID_ARG;
    if ((F % kFfnHC) || F > 4096) return RDETR_ERR_UNSUPPORTED;
    if (!w1 || !w2 || !packed) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, w1, w2, packed)) return RDETR_ERR_UNSUPPORTED;
    const int total = (F / kFfnHC) * 64 * 64;
    hipLaunchKernelGGL(ffn_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w1, w2, F,
                       reinterpret_cast<u32x4 *>(packed));
    return launch_status();
}

// packed <- fp32 (w1 [F, 256], w2 [256, F]) given by element strides (row, column), rounded to bf16: the bits of
// rdetr_ffn_k256_pack_bf16 on the rounded, contiguous matrices.  b1 [F], b2 [256] (fp32, contiguous) -> biases_bf16 [F + 256]
// = (b1, b2); the three are given together or not at all.
extern "C" int rdetr_ffn_k256_pack_f32(const float *w1, long long w1_row_stride, long long w1_col_stride, const float *w2,
                                       long long w2_row_stride, long long w2_col_stride, const float *b1, const float *b2, int F,
                                       uint16_t *packed, uint16_t *biases_bf16, void *stream)
{
    if (F <= 0 || w1_row_stride < 1 || w1_col_stride < 1 || w2_row_stride < 1 || w2_col_stride < 1) return RDETR_ERR_INVALID_ARG;
    if ((F % kFfnHC) || F > 4096) return RDETR_ERR_UNSUPPORTED;
    if (!w1 || !w2 || !packed) return RDETR_ERR_INVALID_ARG;
    if ((b1 != nullptr) != (b2 != nullptr) || (b1 != nullptr) != (biases_bf16 != nullptr)) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(packed, 16) || !all_aligned(4, w1, w2, b1, b2) || !aligned_to(biases_bf16, 2)) return RDETR_ERR_UNSUPPORTED;
    // how a tile is walked: 2 = rows of contiguous 16-byte aligned floats, 1 = down the columns (a transposed view), 0 = along the rows
    auto mode = [](const float *w, long long rs, long long cs) {
        if (cs == 1 && aligned_to(w, 16) && rs % 4 == 0) return 2;
        return rs < cs ? 1 : 0;
    };
    const int blocks = 2 * (F / kFfnHC) + (biases_bf16 ? (F + kFfnK + 255) / 256 : 0);
    hipLaunchKernelGGL(ffn_pack_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), w1, w1_row_stride,
                       w1_col_stride, mode(w1, w1_row_stride, w1_col_stride), w2, w2_row_stride, w2_col_stride,
                       mode(w2, w2_row_stride, w2_col_stride), b1, b2, F, reinterpret_cast<u32x4 *>(packed), biases_bf16);
    return launch_status();
}

#ifdef RDETR_DEV
// development builds only (make dev): component-timing mask of ffn_k256_kernel (WRONG results)
static int g_ffn_dbg = 0;
extern "C" void rdetr_dev_set_ffn_dbg(int v) { g_ffn_dbg = v; }
#endif

// out[M, 256] = relu(x[M, 256] w1[F, 256]^T + b1[F]) w2[256, F]^T + b2[256] with (w1, w2) packed by rdetr_ffn_k256_pack_bf16; bf16
// storage, fp32 accumulation, the hidden activations rounded to bf16 (as the unfused path stores them).  F % 64 == 0, <= 4096.
static int ffn_launch(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2, long long M,
                      int F, uint16_t *out, long long ldo, const uint16_t *gamma, const uint16_t *beta, float eps, const uint16_t *pos,
                      long long ldp, uint16_t *out2, long long ldo2, void *stream)
{
    if (M < 0 || F <= 0) return RDETR_ERR_INVALID_ARG;
    if (const int s = rows_status({{x, ldx, kFfnK, 2}, {out, ldo, kFfnK, 2}})) return s;
    if ((F % kFfnHC) || F > 4096) return RDETR_ERR_UNSUPPORTED;
    if (M == 0) return RDETR_OK;
    if (!x || !packed || !b1 || !b2 || !out) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(packed, 16)) return RDETR_ERR_UNSUPPORTED;
    const int lds = 2 * kFfnBufBytes + (F + 3 * kFfnK) * 4;
    if (ensure_dynamic_lds<ffn_k256_kernel<false>>(kFfnMaxLdsBytes) || ensure_dynamic_lds<ffn_k256_kernel<true>>(kFfnMaxLdsBytes))
        return RDETR_ERR_LAUNCH;
    const long long ntiles = (M + kFfnWaves * kFfnRows - 1) / (kFfnWaves * kFfnRows);
    const long long gx = ntiles < kCus ? ntiles : kCus;
#ifdef RDETR_DEV
    const int dbg = g_ffn_dbg;
#else
    const int dbg = 0;
#endif
    if (gamma)
        hipLaunchKernelGGL(ffn_k256_kernel<true>, dim3((unsigned)gx), dim3(kFfnThreads), (size_t)lds, static_cast<hipStream_t>(stream), x,
                           ldx, packed, b1, b2, M, F, out, ldo, dbg, gamma, beta, eps, pos, ldp, out2, ldo2);
    else
        hipLaunchKernelGGL(ffn_k256_kernel<false>, dim3((unsigned)gx), dim3(kFfnThreads), (size_t)lds, static_cast<hipStream_t>(stream), x,
                           ldx, packed, b1, b2, M, F, out, ldo, dbg, gamma, beta, eps, pos, ldp, out2, ldo2);
    return launch_status();
}

extern "C" int rdetr_ffn_k256_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                                   long long M, int F, uint16_t *out, long long ldo, void *stream)
{
    return ffn_launch(x, ldx, packed, b1, b2, M, F, out, ldo, nullptr, nullptr, 0.f, nullptr, 0, nullptr, 0, stream);
}

// out = LayerNorm(x + ffn(x)) (gamma, beta [256], eps) from the same kernel -- the end of an encoder / decoder layer
// (relation_transformer.py:272-276); with pos / out2 (both or neither): out2 = out + pos, the next layer's query + query_pos.
extern "C" int rdetr_ffn_ln_k256_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *b1,
                                      const uint16_t *b2, const uint16_t *gamma, const uint16_t *beta, float eps,
                                      const uint16_t *pos, long long ldp, long long M, int F, uint16_t *out, long long ldo,
                                      uint16_t *out2, long long ldo2, void *stream)
{
    if (!gamma || !beta || (pos != nullptr) != (out2 != nullptr)) return RDETR_ERR_INVALID_ARG;
    if (pos)
        if (const int s = rows_status({{pos, ldp, kFfnK, 2}, {out2, ldo2, kFfnK, 2}})) return s;
    return ffn_launch(x, ldx, packed, b1, b2, M, F, out, ldo, gamma, beta, eps, pos, ldp, out2, ldo2, stream);
}

// Shared argument checks and launch of the training kernels (the status conventions of ffn_launch: refusal before any HIP call).
// f32: the forward reads fp32 x and also writes xlp; the backward writes fp32 dx (`out`) -- ld in elements of the respective type
static int ffn_train_launch(bool bwd, bool f32, const void *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                            long long M, int F, void *out, long long ldo, uint16_t *hid, long long ldh, uint16_t *dhid,
                            long long ldd, uint16_t *xlp, long long ldxl, void *stream)
{
    const bool xf32 = f32 && !bwd, of32 = f32 && bwd;
    if (M < 0 || F <= 0) return RDETR_ERR_INVALID_ARG;
    // dH and xlp are absent (NULL, stride 0) outside the backward / the fp32-x forward: rows of no elements there
    if (const int s = rows_status({{x, ldx, kFfnK, xf32 ? 4 : 2}, {out, ldo, kFfnK, of32 ? 4 : 2}, {hid, ldh, F, 2}, {dhid, ldd, bwd ? F : 0, 2},
                                   {xlp, ldxl, xf32 ? kFfnK : 0, 2}}))
        return s;
    if ((F % kFfnHC) || F > 4096) return RDETR_ERR_UNSUPPORTED;
    if (M == 0) return RDETR_OK;
    if (!x || !packed || !out || !hid || (bwd ? !dhid : (!b1 || !b2)) || (xf32 && !xlp)) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(packed, 16)) return RDETR_ERR_UNSUPPORTED;
    // H / dH are addressed with 32-bit byte offsets whose top bit marks "no such row" (kFfnNoRow)
    if (M * ldh * 2 > 0x7fffffffLL || (bwd && M * ldd * 2 > 0x7fffffffLL)) return RDETR_ERR_UNSUPPORTED;
    const int lds = 2 * kFfnBufBytes + (F + 3 * kFfnK) * 4;
    if (ensure_dynamic_lds<ffn_k256_train_kernel<kFfnTrain>>(kFfnMaxLdsBytes) || ensure_dynamic_lds<ffn_k256_train_kernel<kFfnBwd>>(kFfnMaxLdsBytes) ||
        ensure_dynamic_lds<ffn_k256_train_f32_kernel<kFfnTrain>>(kFfnMaxLdsBytes) ||
        ensure_dynamic_lds<ffn_k256_train_f32_kernel<kFfnBwd>>(kFfnMaxLdsBytes))
        return RDETR_ERR_LAUNCH;
    const long long ntiles = (M + kFfnWaves * kFfnRows - 1) / (kFfnWaves * kFfnRows);
    const long long gx = ntiles < kCus ? ntiles : kCus;
    const dim3 grid((unsigned)gx), block(kFfnThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint16_t *xb = static_cast<const uint16_t *>(x);
    uint16_t *ob = static_cast<uint16_t *>(out);
    if (f32 && bwd)
        hipLaunchKernelGGL(ffn_k256_train_f32_kernel<kFfnBwd>, grid, block, (size_t)lds, s, x, ldx, packed, b1, b2, M, F, out, ldo, hid, ldh,
                           dhid, ldd, xlp, ldxl);
    else if (f32)
        hipLaunchKernelGGL(ffn_k256_train_f32_kernel<kFfnTrain>, grid, block, (size_t)lds, s, x, ldx, packed, b1, b2, M, F, out, ldo, hid, ldh,
                           dhid, ldd, xlp, ldxl);
    else if (bwd)
        hipLaunchKernelGGL(ffn_k256_train_kernel<kFfnBwd>, grid, block, (size_t)lds, s, xb, ldx, packed, b1, b2, M, F, ob, ldo, hid, ldh, dhid, ldd);
    else
        hipLaunchKernelGGL(ffn_k256_train_kernel<kFfnTrain>, grid, block, (size_t)lds, s, xb, ldx, packed, b1, b2, M, F, ob, ldo, hid, ldh, dhid, ldd);
    return launch_status();
}

// Training forward: rdetr_ffn_k256_bf16 (the same out bits) that also stores the hidden activations
// hid[M, F] = relu(bf16(x w1^T + b1)) (ldh >= F, ldh % 8 == 0, 16-byte aligned; M * ldh * 2 < 2^31) for the backward.
extern "C" int rdetr_ffn_k256_train_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                                         long long M, int F, uint16_t *out, long long ldo, uint16_t *hid, long long ldh, void *stream)
{
    return ffn_train_launch(false, false, x, ldx, packed, b1, b2, M, F, out, ldo, hid, ldh, nullptr, 0, nullptr, 0, stream);
}

// Data gradient of the block: dh[M, F] = bf16(dy w2) where hid > 0, else 0;  dx[M, 256] = dh w1 (fp32 over all of F, rounded once).
// packed_t = rdetr_ffn_k256_pack_bf16(w2^T [F, 256], w1^T [256, F]); hid as the training forward stored it.  No atomics.
extern "C" int rdetr_ffn_k256_backward_bf16(const uint16_t *dy, long long lddy, const uint16_t *packed_t, const uint16_t *hid,
                                            long long ldh, long long M, int F, uint16_t *dh, long long ldd, uint16_t *dx, long long lddx,
                                            void *stream)
{
    return ffn_train_launch(true, false, dy, lddy, packed_t, nullptr, nullptr, M, F, dx, lddx, const_cast<uint16_t *>(hid), ldh, dh, ldd, nullptr, 0, stream);
}

// rdetr_ffn_k256_train_bf16 for fp32 rows x [M, 256] (ldx % 4 == 0): they are rounded to bf16 (RNE) as they are loaded, and the
// rounded rows are also stored as xlp [M, 256] bf16 (ldxl % 8 == 0) -- out and hid have the bits of rdetr_ffn_k256_train_bf16 on xlp.
extern "C" int rdetr_ffn_k256_train_xf32_bf16(const float *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                                              long long M, int F, uint16_t *out, long long ldo, uint16_t *hid, long long ldh, uint16_t *xlp,
                                              long long ldxl, void *stream)
{
    return ffn_train_launch(false, true, x, ldx, packed, b1, b2, M, F, out, ldo, hid, ldh, nullptr, 0, xlp, ldxl, stream);
}

// rdetr_ffn_k256_backward_bf16 whose dx [M, 256] (lddx % 4 == 0) is the fp32 sum over all of F, not rounded; dh as there.
extern "C" int rdetr_ffn_k256_backward_dxf32_bf16(const uint16_t *dy, long long lddy, const uint16_t *packed_t, const uint16_t *hid,
                                                  long long ldh, long long M, int F, uint16_t *dh, long long ldd, float *dx, long long lddx,
                                                  void *stream)
{
    return ffn_train_launch(true, true, dy, lddy, packed_t, nullptr, nullptr, M, F, dx, lddx, const_cast<uint16_t *>(hid), ldh, dh, ldd, nullptr, 0,
                            stream);
}
