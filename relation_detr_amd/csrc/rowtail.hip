// A decoder layer's "attention output projection -> + residual -> LayerNorm" tails as ONE kernel each (bf16, K = 256 -> 256, gfx950):
//     proj   = bf16(x W^T + b)                        fp32 accumulation, one rounding, as the library GEMM stores it
//     out    = bf16(LayerNorm(residual + proj; g, b, eps))                          relation_transformer.py:452-471
//     out_p  = bf16(out + pos)                        optional: the cross-attention's query + query_pos
// for the short row counts of the decoder (B x 900 queries), where the 256-row tiles of linear_ln_k256_kernel (csrc/linear.hip)
// would leave 8 workgroups.  It takes the place of a library GEMM followed by an add_layernorm256 pass that does nothing but
// re-read the [rows, 256] tensor the previous launch has just written:
//     self_attn.out_proj  + norm2 (+ query_pos)       2 launches -> 1
//     cross_attn.output_proj + norm1                  2 launches -> 1
//
//   workgroup  8 waves x 32 rows (two 16-row N blocks that share every weight fragment): 57 workgroups at 1,800 rows.  Wave w owns
//              output columns 32 w .. 32 w + 31 (tile pair w of the packed order) for all the workgroup's rows, as csrc/mlp.hip.
//   weights    packed in fragment order (rdetr_linear_pack_k256_bf16).  A fragment is needed by exactly one wave and goes
//              global -> registers -> MFMA: the wave's 16 fragments are requested at the top of the kernel.
//   x          the B operand of a k-step is the same for all eight waves: wave w loads k-step w for both row blocks (a lane's 8
//              consecutive k = 16 bytes of its row, the operand's own layout) and writes it to an LDS image
//              [row block][k-step][lane] (1-KiB rows, conflict-free); one barrier, every wave reads all 8 k-steps, one k-step ahead
//              of its MFMAs.
//   operands   everything the two epilogues read (residual, bias, gamma, beta, pos) is requested behind the weights at the top, so
//              that the kernel waits for memory once.
//   epilogue   a lane (row, g) ends holding columns 32 w + 8 g .. + 7 of its two rows: bias added, rounded to bf16, the residual
//              added in fp32 (NOT rounded again, as add_layernorm256 forms x + r) and written to one [32][256 + 4] fp32 LDS
//              image (the 4 floats of padding put the 16 rows of a tile into different banks).  One __syncthreads(); then
//              a half wave normalises a row -- a lane owns 8 consecutive channels, fp32 two-pass statistics -- with the
//              arithmetic of add_layernorm256_body (csrc/layernorm.hip), operation for operation: for the same sums `out` has
//              rdetr_add_layernorm_*'s bits.  out_p adds pos to the ROUNDED out.
//   rows       a row count that is no multiple of 32: rows past the last read the last row instead (unconditional loads; a row of
//              the MFMA's N dimension never reaches another row's outputs) and store nothing.
//   measured   (tools/time_rowtail.py, graph replay, us per call, alternating, 5 runs each; profiles/r19/time_rowtail.txt) 600 /
//              1,800 / 3,600 rows: with pos 5.8 / 6.0 / 6.2 against library GEMM + add_layernorm256 8.1 / 8.7 / 10.4; without
//              5.4 / 5.5 / 5.6 against 7.7 / 8.2 / 9.8.  Against linear_ln_k256_kernel: 5.5 vs 15.1 at 1,800 rows, 8.9 vs 16.5 at
//              14,400, 15.3 vs 16.9 at 28,800, 21.0 vs 18.4 at 44,646: ops.linear_ln_k256 switches kernels at 28,800 rows.
//              In the stack (profiles/r19/decoder_chain_by_kernel.txt) 6.9 / 6.5 us against 6.4 + 8.1 for the two launches
//              replaced; step 3.584 -> 3.543 ms (profiles/r19/ab_stack.txt).
//   resources  (hipcc -Rpass-analysis=kernel-resource-usage) with / without pos: 123 / 115 VGPRs, no AGPRs, no scratch, no spills,
//              48.5 KiB static LDS, 4 waves per SIMD by registers (3 workgroups per CU by LDS).
//   dropped    * every wave reading its x operands straight from global memory (a ring of four two-k-step stages): the eight
//                waves' reads of the same 64-byte row pieces all go through the one L1 at 64 bytes per clock -- 11.2 us at 1,800
//                rows, slower than the sequence replaced (profiles/r19/time_rowtail_first.txt).
//              * the third tail, linear2 + norm3 + the decoder's own norm (K = d_ffn = 2048, a second LayerNorm of the rounded
//                row in the same epilogue; eight weight slabs, two register sets of fragments, x double-buffered in LDS): correct,
//                but 18.1 / 18.3 / 21.3 us at 600 / 1,800 / 3,600 rows against 12.9 / 16.1 / 18.7 for the library GEMM + two
//                add_layernorm256 passes (profiles/r19/time_rowtail_with_ffn_tail.txt).  A 32-row workgroup pulls all of W2
//                (1 MiB) through its own L1: 7-8 us at 64 bytes per clock before any latency, on 57 of 256 CUs; the library
//                kernel splits K over the idle CUs.  Taken out again, with its instantiations.
#include "launch.h"
#include "rows256.h"

namespace rdetr {

typedef __bf16 rt_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kRtWaves = 8, kRtThreads = kRtWaves * 64;
constexpr int kRtRows = 32;                                // rows per workgroup: two 16-row N blocks
constexpr int kRtLd = 256 + 4;                             // fp32 row pitch of the LDS image
constexpr int kRtXImg = 2 * 8 * 64;                        // x in u32x4: [row block][k-step][lane], 16 KiB

// this wave's 16 fragments of the packed weight (tiles 2 w, 2 w + 1), in the order the MFMAs take them
struct RtFrags { u32x4 f[16]; };                           // f[2 s + e]: k-step s, tile e

// the loads are issued at the top of the kernel and widened (row256_widen8) where they are used
__device__ __forceinline__ u32x4 rt_load8(const uint16_t *p) { return *reinterpret_cast<const u32x4 *>(p); }

__device__ __forceinline__ void rt_store8(uint16_t *p, const float (&v)[8])
{
    *reinterpret_cast<u32x4 *>(p) = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
}

// y = LayerNorm(v) * g + b over the 256 channels a half wave holds (8 per lane): the statistics block of add_layernorm256_body
// (csrc/layernorm.hip) operation for operation -- a COPY, see rows256.h; change the two together
__device__ __forceinline__ void rt_normalise(float (&v)[8], const float (&g)[8], const float (&b)[8], float eps, float (&y)[8])
{
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
    const float mean = row256_half_sum(s) * (1.0f / 256.0f);
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] -= mean;
        sq += v[k] * v[k];
    }
    const float rstd = 1.0f / sqrtf(row256_half_sum(sq) * (1.0f / 256.0f) + eps);
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = v[k] * rstd * g[k] + b[k];
}

struct RtArgs {
    const uint16_t *x, *packed, *bias, *res, *gamma, *beta, *pos;
    uint16_t *out, *out_pos;
    long long ldx, ldr, ldp, ldo, ldop, M;
    float eps;
};

template <bool kPos>
__global__ __launch_bounds__(kRtThreads) void linear_ln_rows_kernel(RtArgs a)
{
    __shared__ __attribute__((aligned(16))) u32x4 xs[kRtXImg];
    __shared__ __attribute__((aligned(16))) float img[kRtRows * kRtLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * kRtRows;

    // this wave's 16 weight fragments, then its share of x: k-step `wave` for both row blocks -- lane (row, g) its 8 k = 16 bytes,
    // the B operand's own layout (rows past the last read the last row)
    RtFrags w;
    {
        const u32x4 *wp = reinterpret_cast<const u32x4 *>(a.packed) + (size_t)wave * 16 * 64 + lane;
#pragma unroll
        for (int i = 0; i < 16; ++i) w.f[i] = wp[((i & 1) * 8 + (i >> 1)) * 64];
    }
    long long rr[2];
    u32x4 xr[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        rr[cb] = row0 + 16 * cb + col < a.M ? row0 + 16 * cb + col : a.M - 1;
        xr[cb] = rt_load8(a.x + rr[cb] * a.ldx + 32 * wave + 8 * g);
    }
    // the lane's residual columns and bias in the MFMA layout (lane (row, g): columns 32 w + 8 g .. + 7), and, in the normalising
    // layout (lane (half, l): row 2 w + half (+ 16), channels 8 l .. + 7), the LayerNorm parameters and pos
    const int c0 = 32 * wave + 8 * g;
    const int half = lane >> 5, c = (lane & 31) * 8;
    u32x4 rv[2], pr[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) rv[cb] = rt_load8(a.res + rr[cb] * a.ldr + c0);
    const u32x4 bq = a.bias ? rt_load8(a.bias + c0) : u32x4{0u, 0u, 0u, 0u};
    const u32x4 gq = rt_load8(a.gamma + c), tq = rt_load8(a.beta + c);
    if (kPos) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long row = row0 + 16 * i + 2 * wave + half;
            pr[i] = rt_load8(a.pos + (row < a.M ? row : a.M - 1) * a.ldp + c);
        }
    }
    __builtin_amdgcn_sched_barrier(0);                     // the loads are issued HERE, not sunk to their uses
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) xs[(cb * 8 + wave) * 64 + lane] = xr[cb];
    __syncthreads();                                       // every wave's k-step of x

    f32x4 acc[2][2];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[e][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
        // every output sums its k-steps in ascending order; the B operands come from LDS one k-step ahead of their MFMAs
        const u32x4 *xi = xs + lane;
        u32x4 xb[2][2];
        xb[0][0] = xi[0];
        xb[0][1] = xi[8 * 64];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (s + 1 < 8) {
                xb[(s + 1) & 1][0] = xi[(s + 1) * 64];
                xb[(s + 1) & 1][1] = xi[(8 + s + 1) * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    acc[e][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(rt_bf16x8, w.f[2 * s + e]),
                                                                         __builtin_bit_cast(rt_bf16x8, xb[s & 1][cb]), acc[e][cb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // bias, one rounding to bf16, + residual in fp32 -> the LDS image.  Lane (row, g): tile e holds columns c0 + 4 e .. + 3
    {
        float bb[8];
        row256_widen8(bq, bb);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float rf[8];
            row256_widen8(rv[cb], rf);
            const f32x4 lo = acc[0][cb], hi = acc[1][cb];
            const float o[8] = {lo.x + bb[0], lo.y + bb[1], lo.z + bb[2], lo.w + bb[3], hi.x + bb[4], hi.y + bb[5], hi.z + bb[6], hi.w + bb[7]};
            float s[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) s[k] = bf16_bits_to_f32(f32_to_bf16_bits(o[k])) + rf[k];
            float *dst = img + (16 * cb + col) * kRtLd + c0;
            *reinterpret_cast<f32x4 *>(dst) = f32x4{s[0], s[1], s[2], s[3]};
            *reinterpret_cast<f32x4 *>(dst + 4) = f32x4{s[4], s[5], s[6], s[7]};
        }
    }
    __syncthreads();                                       // every wave's columns of the 32 rows

    // a half wave per row, two rows per half: rows 2 wave + half and 16 + 2 wave + half of the block
    float gm[8], bt[8];
    row256_widen8(gq, gm);
    row256_widen8(tq, bt);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int lr = 16 * i + 2 * wave + half;
        const long long row = row0 + lr;
        const bool ok = row < a.M;
        float v[8], y[8];
        const f32x4 v0 = *reinterpret_cast<const f32x4 *>(img + lr * kRtLd + c), v1 = *reinterpret_cast<const f32x4 *>(img + lr * kRtLd + c + 4);
        v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
        rt_normalise(v, gm, bt, a.eps, y);                 // the shuffles run in every lane; only valid rows store
        if (ok) rt_store8(a.out + row * a.ldo + c, y);
        if (kPos && ok) {
            float pv[8];
            row256_widen8(pr[i], pv);
#pragma unroll
            for (int k = 0; k < 8; ++k) pv[k] += bf16_bits_to_f32(f32_to_bf16_bits(y[k]));        // out as stored
            rt_store8(a.out_pos + row * a.ldop + c, pv);
        }
    }
}

}  // namespace rdetr

using namespace rdetr;

// out [M, 256] = LayerNorm(residual + bf16(x [M, 256] W^T + bias); gamma, beta, eps) and, with pos, out_pos = out + pos, for short M
// (32 rows per workgroup).  `packed`: W [256, 256] packed by rdetr_linear_pack_k256_bf16.  pos == NULL selects the variant without
// out_pos (which is then ignored).  All bf16; row strides in elements, multiples of 8, bases and the parameter vectors 16-byte
// aligned (else RDETR_ERR_UNSUPPORTED); bias nullable.
extern "C" int rdetr_linear_ln_rows_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *bias,
                                         const uint16_t *residual, long long ldr, const uint16_t *gamma, const uint16_t *beta, float eps,
                                         const uint16_t *pos, long long ldp, long long M, uint16_t *out, long long ldo, uint16_t *out_pos,
                                         long long ldop, void *stream)
{
    const bool has_pos = pos != nullptr;
    if (M < 0) return RDETR_ERR_INVALID_ARG;
    if (const int s = has_pos ? rows_status({{x, ldx, 256, 2}, {residual, ldr, 256, 2}, {out, ldo, 256, 2}, {pos, ldp, 256, 2}, {out_pos, ldop, 256, 2}})
                              : rows_status({{x, ldx, 256, 2}, {residual, ldr, 256, 2}, {out, ldo, 256, 2}}))
        return s;
    if (M == 0) return RDETR_OK;
    if (!x || !packed || !residual || !gamma || !beta || !out || (has_pos && !out_pos)) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, packed, bias, gamma, beta)) return RDETR_ERR_UNSUPPORTED;
    const long long nblk = (M + kRtRows - 1) / kRtRows;
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    const RtArgs a = {x, packed, bias, residual, gamma, beta, pos, out, out_pos, ldx, ldr, ldp, ldo, ldop, M, eps};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (has_pos)
        hipLaunchKernelGGL(linear_ln_rows_kernel<true>, dim3((unsigned)nblk), dim3(kRtThreads), 0, st, a);
    else
        hipLaunchKernelGGL(linear_ln_rows_kernel<false>, dim3((unsigned)nblk), dim3(kRtThreads), 0, st, a);
    return launch_status();
}
