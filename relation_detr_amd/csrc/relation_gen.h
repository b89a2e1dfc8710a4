// The generator of the in-kernel position-relation bias  relu(W . feat(box_q, box_k) + b) * log2(e)  (gfx950): everything the
// forward (csrc/attn_rel.hip) and its backward (csrc/attn_rel_bwd.hip) must agree on, defined once.  The backward takes the
// ReLU's active set and P = exp2(z - lse2) from the bias it regenerates, so both sides run THESE statements: the same pair sets
// of one query x 16 keys, hardware log2 / sin / cos in revolutions, features and key-table entries rounded to bf16, W as hi + lo
// bf16 parts, the same four MFMAs in the same order.  How a kernel schedules the calls (which wave takes which pair sets, how
// many chains are in flight) is its own business.
//
// Per 16 x 64 chunk the pairs are "pair sets" (one query x 16 consecutive keys), each projected by MFMAs
//   bias^T[key][head] = A[key][:] . B[:][head]  (v_mfma_f32_16x16x32_bf16, B in hi + lo bf16 parts):
//     distance coordinates (x, y; 32 features): lane (key = lane & 15, g = lane >> 4) computes the 8 features the A fragment wants
//               from it -- coordinate g >> 1, frequencies 4 (g & 1) .. + 3: one log2, 4 x (v_sin, v_cos);  B = W[:, 0:32]
//     size-ratio coordinates (w, h; 32 features): log(w_q / w_k) = a_q - a_k, and sin / cos (a_q - a_k) are bilinear in per-box
//               terms, so their projection is the dot product of the KEY's 32 values (sin a_k, cos a_k) (A, once per key) with
//               per-(query, head) coefficients U (B, once per query tile): no per-pair arithmetic at all
// Everything that feeds the soft-max is produced in the log2 domain: W, b scaled by log2(e) (ReLU commutes).
#pragma once
#include <cmath>

#include "attn_common.h"

namespace rdetr {

constexpr int kRelD = 32, kRelH = 8, kRelTileQ = 16, kRelChunk = 64, kRelWaves = 16, kRelF = 16;
constexpr int kRelQStride = 68;                                 // floats per (head, query) row of a bias tile: 64 keys + 4 (banks)
constexpr int kRelHeadStride = kRelTileQ * kRelQStride + 4;     // floats per head (+4: the 8 heads' b128 writes hit 8 bank groups)
constexpr int kRelBiasBuf = kRelH * kRelHeadStride;             // floats per bias tile [head][query][key]
constexpr int kRelQC = 4;                                       // floats per query: x, y, 1/(w+eps), 1/(h+eps)
constexpr int kRelWBytes = 2 * 64 * 16;                         // W fragments: hi, lo x 64 lanes x u32x4
constexpr int kRelUBytes = kRelTileQ * 2 * 64 * 16;             // U fragments: 16 queries x (hi, lo) x 64 lanes x u32x4

struct RelFreq {
    float cf[8];        // ln 2 * scale / (temperature^(2k/F) * 2 pi): log2 of the encoding -> revolutions
};

inline RelFreq rel_freq(int F, float rel_scale, float temperature)
{
    RelFreq fr;
    for (int i = 0; i < F / 2; ++i) {
        const double dim_t = (double)powf(temperature, (float)i * 2.0f / (float)F);       // get_dim_t, position_encoding.py:101-105
        fr.cf[i] = (float)(0.6931471805599453 * (double)rel_scale / (dim_t * 6.283185307179586));
    }
    return fr;
}

// W[:, 0:32] (distance features) as MFMA B fragments, hi / lo bf16 parts: the weights are NOT rounded to bf16, their lo part
// carries the remainder through a second MFMA.  Threads 0-127 of the workgroup.
__device__ __forceinline__ void build_w_fragments(int tid, const float *__restrict__ Wp, u32x4 *wfr)
{
    if (tid < 128) {
        const int part = tid >> 6, l = tid & 63, head = l & 15, gg = l >> 4;
        unsigned int o[4] = {0u, 0u, 0u, 0u};
        if (head < kRelH) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float w0 = Wp[head * 64 + 8 * gg + 2 * j] * kLog2e, w1 = Wp[head * 64 + 8 * gg + 2 * j + 1] * kLog2e;
                if (part) {
                    w0 -= bf16_bits_to_f32(f32_to_bf16_bits(w0));
                    w1 -= bf16_bits_to_f32(f32_to_bf16_bits(w1));
                }
                o[j] = pack_bf16x2(w0, w1);
            }
        }
        wfr[tid] = u32x4{o[0], o[1], o[2], o[3]};
    }
}

// Per-query constants of the two distance coordinates and the size-ratio coefficients U of the 16 queries from q0 on (all 1024
// threads of the workgroup).  Size-ratio coordinates: sin / cos (a_q - a_k) are bilinear in the per-box tables, so their
// projection is a 32-term dot product of the KEY's table entries (sin a_k, cos a_k) with per-(query, head) coefficients
//   U[sin entry] = -W_sin cos a_q + W_cos sin a_q,   U[cos entry] = W_sin sin a_q + W_cos cos a_q
// -> one more MFMA K-step whose B operand belongs to the query; thread = (query, fragment lane), hi and lo parts
__device__ __forceinline__ void build_query_tile(int tid, int b, int q0, int N, const float *__restrict__ src,
                                                 const float *__restrict__ Wp, float eps, const RelFreq &fr, float *qc, u32x4 *ufr)
{
    if (tid < kRelTileQ) {
        const int qi = q0 + tid < N ? q0 + tid : N - 1;
        const f32x4 s = *reinterpret_cast<const f32x4 *>(src + ((size_t)b * N + qi) * 4);
        float *r = qc + tid * kRelQC;
        r[0] = s.x; r[1] = s.y; r[2] = 1.0f / (s.z + eps); r[3] = 1.0f / (s.w + eps);
    }
    const int qq = tid >> 6, l = tid & 63, head = l & 15, gg = l >> 4, cc = gg >> 1, k0 = 4 * (gg & 1);
    const int qi = q0 + qq < N ? q0 + qq : N - 1;
    unsigned int hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
    if (head < kRelH) {
        const float l2 = __builtin_amdgcn_logf(src[((size_t)b * N + qi) * 4 + 2 + cc] + eps);      // angle a_q = log(size + eps) * scale / dim_t
        const float *wrow = Wp + head * 64 + 32 + 16 * cc + 2 * k0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = l2 * fr.cf[k0 + j];
            const float ss = __builtin_amdgcn_sinf(x), sc = __builtin_amdgcn_cosf(x);
            const float ws = wrow[2 * j] * kLog2e, wc = wrow[2 * j + 1] * kLog2e;
            const float us = __builtin_fmaf(wc, ss, -(ws * sc)), uc = __builtin_fmaf(ws, ss, wc * sc);
            hi[j] = pack_bf16x2(us, uc);
            lo[j] = pack_bf16x2(us - bf16_bits_to_f32(hi[j] & 0xffffu), uc - bf16_bits_to_f32(hi[j] >> 16));
        }
    }
    ufr[(qq * 2 + 0) * 64 + l] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    ufr[(qq * 2 + 1) * 64 + l] = u32x4{lo[0], lo[1], lo[2], lo[3]};
}

// (sin a_q, cos a_q) of slot m = 8 * (size coordinate) + frequency of the query box sb: the angle build_query_tile puts into U,
// for the backward's combination of the size-ratio half of grad_weight
__device__ __forceinline__ f32x2 query_size_sincos(const float *sb, int m, float eps, const RelFreq &fr)
{
    const float x = __builtin_amdgcn_logf(sb[2 + (m >> 3)] + eps) * fr.cf[m & 7];
    return f32x2{__builtin_amdgcn_sinf(x), __builtin_amdgcn_cosf(x)};
}

// The key side of a wave's pair sets: lane (key = lane & 15, g) -> its box's distance coordinate, and (sin a_k, cos a_k) of this
// lane's size coordinate and frequencies = the A fragment of the table K-step
struct RelKey {
    float tcoord;
    u32x4 a1;
};
__device__ __forceinline__ RelKey key_side(const f32x4 &kbox, int g, float eps, const RelFreq &fr)
{
    const int c01 = g >> 1, fsel = g & 1;
    const float cf0 = fr.cf[4 * fsel + 0], cf1 = fr.cf[4 * fsel + 1], cf2 = fr.cf[4 * fsel + 2], cf3 = fr.cf[4 * fsel + 3];
    RelKey r;
    r.tcoord = c01 ? kbox.y : kbox.x;
    const float l2k = __builtin_amdgcn_logf((c01 ? kbox.w : kbox.z) + eps);
    const float y0 = l2k * cf0, y1 = l2k * cf1, y2 = l2k * cf2, y3 = l2k * cf3;
    r.a1 = u32x4{pack_bf16x2(__builtin_amdgcn_sinf(y0), __builtin_amdgcn_cosf(y0)),
                 pack_bf16x2(__builtin_amdgcn_sinf(y1), __builtin_amdgcn_cosf(y1)),
                 pack_bf16x2(__builtin_amdgcn_sinf(y2), __builtin_amdgcn_cosf(y2)),
                 pack_bf16x2(__builtin_amdgcn_sinf(y3), __builtin_amdgcn_cosf(y3))};
    return r;
}

// One pair set (query qq of the tile x the lane's key): features, projection and ReLU.  Returns the distance feature fragment
// (the backward reduces grad_weight from it); lane (head = lane & 15 < 8, g) writes relu(bias) * log2(e) of keys 4 g .. 4 g + 3
// to dst + qq * kRelQStride.
__device__ __forceinline__ u32x4 pair_set(int qq, int lane, int g, const RelKey &ks, const float *qc, const u32x4 *wfr, const u32x4 *ufr,
                                          float bph, const RelFreq &fr, float *dst)
{
    const int c01 = g >> 1, fsel = g & 1;
    const float cf0 = fr.cf[4 * fsel + 0], cf1 = fr.cf[4 * fsel + 1], cf2 = fr.cf[4 * fsel + 2], cf3 = fr.cf[4 * fsel + 3];
    const u32x4 w0h = wfr[lane], w0l = wfr[64 + lane];
    const float *qr = qc + qq * kRelQC;
    const float sc = qr[c01], inv = qr[2 + c01];
    const u32x4 uh = ufr[(qq * 2 + 0) * 64 + lane], ul = ufr[(qq * 2 + 1) * 64 + lane];
    // distance coordinate: log(|c_q - c_k| / (size_q + eps) + 1), as log2; the frequency factors carry ln 2 * scale / dim_t
    const float e2 = __builtin_amdgcn_logf(__builtin_fmaf(__builtin_fabsf(sc - ks.tcoord), inv, 1.0f));
    const float x0 = e2 * cf0, x1 = e2 * cf1, x2 = e2 * cf2, x3 = e2 * cf3;
    u32x4 a0;
    a0.x = pack_bf16x2(__builtin_amdgcn_sinf(x0), __builtin_amdgcn_cosf(x0));
    a0.y = pack_bf16x2(__builtin_amdgcn_sinf(x1), __builtin_amdgcn_cosf(x1));
    a0.z = pack_bf16x2(__builtin_amdgcn_sinf(x2), __builtin_amdgcn_cosf(x2));
    a0.w = pack_bf16x2(__builtin_amdgcn_sinf(x3), __builtin_amdgcn_cosf(x3));
    f32x4 acc = {bph, bph, bph, bph};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ks.a1), as_bf16x8(uh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ks.a1), as_bf16x8(ul), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a0), as_bf16x8(w0h), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a0), as_bf16x8(w0l), acc, 0, 0, 0);
    // lane (head = lane & 15, g) holds keys 4 g .. 4 g + 3 of the pair set: relu(bias) * log2(e)
    acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
    if ((lane & 15) < kRelH) *reinterpret_cast<f32x4 *>(dst + qq * kRelQStride) = acc;
    return a0;
}

}  // namespace rdetr
