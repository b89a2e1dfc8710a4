// Pieces of the 256-channel row arithmetic -- half a wavefront per row, 8 consecutive channels per lane -- that
// add_layernorm256_body (layernorm.hip) and the fused projection + LayerNorm tail (rowtail.hip) share.  Only what leaves both
// files' gfx950 code as it was is here: the statistics block and the bf16 store stay written out in each file (as calls into this
// header they change layernorm.hip's register allocation and instruction order), and rowtail.hip's copy must follow layernorm.hip's.
// Other lane layouts (linear_ln_k256_kernel, ffn_k256_body.h) have their own arithmetic.
#pragma once
#include "common.h"

namespace rdetr {

// sum over the 32 lanes of a half wave
__device__ __forceinline__ float row256_half_sum(float v)
{
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// 8 bf16 in one 16-byte register set -> fp32
__device__ __forceinline__ void row256_widen8(const u32x4 &r, float (&v)[8])
{
    v[0] = __builtin_bit_cast(float, r.x << 16); v[1] = __builtin_bit_cast(float, r.x & 0xffff0000u);
    v[2] = __builtin_bit_cast(float, r.y << 16); v[3] = __builtin_bit_cast(float, r.y & 0xffff0000u);
    v[4] = __builtin_bit_cast(float, r.z << 16); v[5] = __builtin_bit_cast(float, r.z & 0xffff0000u);
    v[6] = __builtin_bit_cast(float, r.w << 16); v[7] = __builtin_bit_cast(float, r.w & 0xffff0000u);
}

}  // namespace rdetr
