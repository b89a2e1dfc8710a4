// Conventions shared by the four decoder self-attention files (attn.hip, attn_bwd.hip, attn_rel.hip, attn_rel_bwd.hip; gfx950):
// the MFMA operand casts, the wave-private LDS fence, the transposed operand read, the key-mask / key-tail rule, the backward's
// view of the row log-sum-exp, the host-side alignment test and the Di = rowsum(dO o O) launch.  Only what is identical in all
// its users lives here; the soft-max and dS bodies differ per kernel on purpose and stay in their files.
#pragma once
#include "launch.h"

namespace rdetr {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 x) { return __builtin_bit_cast(bf16x8, x); }

// Orders a wave's own LDS writes and reads of an image that is private to the wave (no workgroup barrier)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One transposed 64-bit read (ds_read_b64_tr_b16) of a row-major bf16 LDS image with a row stride of kStride bytes (96 at every
// call site: conflict-free): lane (c = lane & 15, g = lane >> 4) gets column 16 cb + c of rows row0 + 4 g + j, j = 0..3 -- the
// A operand [m = column][k = 4 g + j] of a K = 16 MFMA.  Lane 4 q' + p of its 16-lane group supplies row row0 + 4 g + q',
// columns 16 cb + 4 p .. + 3.  Every lane of the wave must execute it (EXEC all ones).
template <int kStride>
__device__ __forceinline__ u32x2 tr_rows4(const unsigned char *img, int row0, int cb, int lane)
{
    const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const unsigned char *a0 = img + (row0 + 4 * g + tq) * kStride + cb * 32 + tp * 8;
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(a0)));
}
// ... and of rows row0 + 16 (j >> 2) + 4 g + (j & 3), j = 0..7: the A operand [16 x 32] of a K = 32 MFMA, with the key permutation
// k = 8 g + j  <->  row 16 (j >> 2) + 4 g + (j & 3) that the lanes' own P / dS values have (a sum over keys does not care)
template <int kStride>
__device__ __forceinline__ u32x4 tr_rows8(const unsigned char *img, int row0, int cb, int lane)
{
    const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const unsigned char *a0 = img + (row0 + 4 * g + tq) * kStride + cb * 32 + tp * 8;           // one address, two reads 16 rows apart
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(a0 + 16 * kStride));
    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
    return u32x4{l2.x, l2.y, h2.x, h2.y};
}

// lse2 of a row as the backward uses it: a fully masked row (-inf) becomes +inf, so that exp2(z - lse2) = 0 for all its keys
__device__ __forceinline__ float bwd_lse(float l2) { return l2 == -__builtin_inff() ? __builtin_inff() : l2; }

// The key-mask / key-tail rule of the family: t holds the bias of keys kk .. kk + 3 of one query; a bool-masked key (mask_row =
// the query's row of the [N, M] mask, or null) and a key past the end get -inf, i.e. P = 0 in the forward and dS = 0 in the backward
__device__ __forceinline__ void mask_keys(f32x4 &t, int kk, int M, const unsigned char *mask_row)
{
    if (mask_row) {
        if (kk + 0 < M && mask_row[kk + 0]) t.x = -__builtin_inff();
        if (kk + 1 < M && mask_row[kk + 1]) t.y = -__builtin_inff();
        if (kk + 2 < M && mask_row[kk + 2]) t.z = -__builtin_inff();
        if (kk + 3 < M && mask_row[kk + 3]) t.w = -__builtin_inff();
    }
    if (kk + 0 >= M) t.x = -__builtin_inff();          // keys past the end never take part
    if (kk + 1 >= M) t.y = -__builtin_inff();
    if (kk + 2 >= M) t.z = -__builtin_inff();
    if (kk + 3 >= M) t.w = -__builtin_inff();
}

// The refusals both backward entry points share, in their order: row strides shorter than the H * D columns and a short
// workspace are invalid arguments; operands the kernels' 16- / 8-byte accesses cannot take are unsupported.  RDETR_OK otherwise.
inline int attention_bwd_layout_status(const void *q, const void *k, const void *v, const void *out, const void *dout, const void *lse,
                                       const void *workspace, const void *dq, const void *dk, const void *dv, int ldq, int ldk, int ldv,
                                       int ldo, int lddo, int lddq, int lddk, int lddv, long long span, long long workspace_bytes,
                                       long long workspace_need)
{
    if (ldq < span || ldk < span || ldv < span || ldo < span || lddo < span || lddq < span || lddk < span || lddv < span)
        return RDETR_ERR_INVALID_ARG;
    if (workspace_bytes < workspace_need) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(q, 16) || !aligned_to(k, 16) || !aligned_to(v, 16) || !aligned_to(dout, 16) || ldq % 8 || ldk % 8 || ldv % 8 || lddo % 8)
        return RDETR_ERR_UNSUPPORTED;
    if (!aligned_to(out, 8) || !aligned_to(dq, 8) || !aligned_to(dk, 8) || !aligned_to(dv, 8) || ldo % 4 || lddq % 4 || lddk % 4 || lddv % 4)
        return RDETR_ERR_UNSUPPORTED;
    if (!aligned_to(lse, 4) || !aligned_to(workspace, 16)) return RDETR_ERR_UNSUPPORTED;
    return RDETR_OK;
}

// Di = rowsum(dO o O) per (image, head, query) of head dim 32, fp32 [B*H, N]: the first piece of both backwards' workspaces
// (kernel and launcher in csrc/attn_bwd.hip; the caller checks the launch status)
inline long long attention_di_bytes(int B, int H, int N) { return ((long long)B * H * N * 4 + 255) / 256 * 256; }
void launch_attention_bwd_di(const uint16_t *out, int ldo, const uint16_t *dout, int lddo, int B, int H, int N, float *di,
                             hipStream_t stream);

}  // namespace rdetr
