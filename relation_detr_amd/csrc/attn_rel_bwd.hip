// Backward of the decoder self-attention that GENERATES its position-relation bias (csrc/attn_rel.hip), bf16 training (gfx950).
//
// Differentiates  out = softmax(Q K^T * scale + relu(W . feat(box_q, box_k) + b) [, bool mask]) V  with respect to Q, K, V and the
// 1x1 projection (W [8, 64], b [8]) from the forward's row log-sum-exp.  Replaces, on the training path, the chain
// rdetr_relation_bias_f32 -> (out > 0) -> masked_fill_ -> rdetr_relation_attention_backward_bf16 (bias read twice, dbias
// written) -> rdetr_relation_bias_backward_f32: no [B*H, N, M]-sized tensor is read or written.  Boxes carry no gradient
// (models/bricks/relation_transformer.py:527-529).
//
// The bias is regenerated with the FORWARD kernel's arithmetic, instruction for instruction (pair sets of one query x 16 keys,
// hardware log2 / sin / cos in revolutions, features and key-table entries rounded to bf16, W as hi + lo bf16 parts, the same
// four MFMAs in the same order, everything pre-multiplied by log2 e): z = S * scale * log2e + bias, P = exp2(z - lse2) are the
// forward's values and the ReLU's active set is the forward's.  The generator below must stay in step with attn_rel.hip.
//
//   di      Di = rowsum(dO o O) per (image, head, query), fp32 workspace
//   dq      grid = (ceil(N / 16) query tiles, B), 16 waves that own 16 queries for ALL 8 heads and sweep the keys in chunks of 64,
//           three phases per chunk separated by workgroup barriers:
//             F  every wave generates 4 pair sets (key block w >> 2, queries 4 (w & 3) ..) into the LDS bias tile
//                [head][query][key] and keeps their feature fragments in registers
//             A  wave (head = w & 7, key half = w >> 3): S^T, dP^T (A = K / V rows from global memory, B = the lane's query row
//                of Q / dO), P, dS = P o (dP - Di), dQ^T += K^T dS^T (K^T through ds_read_b64_tr_b16 of a wave-private image),
//                and g = dS where the bias is > 0, else 0, written over the bias entries it just read
//             G  every wave reads g back for its own pair sets (the lane that wrote a bias entry reads that entry) and reduces
//                it on the matrix cores:  distance half  gradW^T[ch][head] += feat^T[ch][pair] . g[pair][head]  (K = 32 pairs,
//                feat^T through the transposed read of a wave-private image of the fragments it kept);  size-ratio half
//                T^T[entry][head] += table^T[entry][key] . g[key][head] per query (K = 16 keys, v_mfma_f32_16x16x16_bf16), and
//                after the sweep the per-query combination with (sin a_q, cos a_q): no per-pair transcendental for this half
//           one 520-float record (gradW [8][64], gradb [8]) per workgroup, summed over its waves in a fixed order
//   dkv     grid = (ceil(M / 64) key chunks, B), the same 16 waves sweeping the QUERY tiles: the per-tile prologue of the forward
//           (query constants, size-ratio coefficients), phase F as above, then wave (head = w & 7, key blocks 2 (w >> 3) + {0, 1})
//           with the key on the lane: S = Q K^T, dP = dO V^T (A = Q / dO rows of the tile, B = the wave's K / V rows, registers),
//           dV^T += dO^T P, dK^T += Q^T dS with K = the tile's 16 queries (v_mfma_f32_16x16x16_bf16).  From 16 query tiles on,
//           the sweep is split four ways over blockIdx.z (one workgroup per 64 keys and image leaves most of the device
//           idle): fp32 partials in the workspace, added in split order by a small kernel
//   reduce  grad_weight / grad_bias = the records in workgroup order, one wave per output, fixed-order tree
// Deterministic: no float atomics, every output element written exactly once.  Masking as csrc/attn_bwd.hip: masked keys and keys
// past M give P = 0 and dS = 0; a fully masked row (lse2 = -inf) has P = 0 for all keys.
// The pair transcendentals are evaluated twice here (dq, dkv) + once in the forward, at the hardware rate.
#include <type_traits>

#include "common.h"

namespace rdetr {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int kAbD = 32, kAbH = 8, kAbTileQ = 16, kAbChunk = 64, kAbWaves = 16, kAbF = 16;
constexpr int kAbQStride = 68;                                  // the forward's bias tile: floats per (head, query) row
constexpr int kAbHeadStride = kAbTileQ * kAbQStride + 4;
constexpr int kAbBiasBuf = kAbH * kAbHeadStride;
constexpr int kAbQC = 4;
constexpr int kAbTS = 96;                                       // image row stride in bytes (conflict-free transposed reads)
constexpr int kAbImgRows = 48;                                  // rows 0-31: K rows (phase A) / feature fragments (phase G); 32-47: key table
constexpr int kAbImg = kAbImgRows * kAbTS;
constexpr int kAbRecord = kAbH * 64 + kAbH;                     // 520 floats per workgroup
constexpr int kAbLdsBias = 0, kAbLdsQC = kAbBiasBuf * 4, kAbLdsW = kAbLdsQC + kAbTileQ * kAbQC * 4, kAbLdsU = kAbLdsW + 2 * 64 * 16,
              kAbLdsImg = kAbLdsU + kAbTileQ * 2 * 64 * 16, kAbLdsBytesDq = kAbLdsImg + kAbWaves * kAbImg,        // 140.4 KiB
              kAbLdsBytesDkv = kAbLdsImg;                                                                          // 68.4 KiB
static_assert(kAbWaves * kAbImg >= kAbWaves * kAbRecord * 4, "the record reduction reuses the images");
static_assert(kAbWaves * kAbImg >= kAbH * 2 * 64 * 16, "the dQ reduction reuses the images");
constexpr float kAbLog2e = 1.4426950408889634f;

struct AbFreq {
    float cf[8];        // ln 2 * scale / (temperature^(2k/F) * 2 pi): log2 of the encoding -> revolutions (attn_rel.hip::RelFreq)
};

__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 x) { return __builtin_bit_cast(bf16x8, x); }
__device__ __forceinline__ s16x4 as_s16x4(u32x2 x) { return __builtin_bit_cast(s16x4, x); }

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One transposed 64-bit read of a row-major bf16 image (stride kAbTS): lane (c = lane & 15, g) gets column 16 cb + c of rows
// row0 + 4 g + j, j = 0..3 -- the A operand [m = column][k = 4 g + j] of a K = 16 MFMA.  EXEC all ones.
__device__ __forceinline__ u32x2 tr_rows4(const unsigned char *img, int row0, int cb, int lane)
{
    const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const unsigned char *a0 = img + (row0 + 4 * g + tq) * kAbTS + cb * 32 + tp * 8;
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(a0)));
}
// ... and of rows row0 + 16 (j >> 2) + 4 g + (j & 3), j = 0..7: the A operand of a K = 32 MFMA (csrc/attn_bwd.hip::tr_operand)
__device__ __forceinline__ u32x4 tr_rows8(const unsigned char *img, int row0, int cb, int lane)
{
    const u32x2 lo = tr_rows4(img, row0, cb, lane), hi = tr_rows4(img, row0 + 16, cb, lane);
    return u32x4{lo.x, lo.y, hi.x, hi.y};
}

__device__ __forceinline__ float bwd_lse(float l2) { return l2 == -__builtin_inff() ? __builtin_inff() : l2; }

// W[:, 0:32] (distance features) as MFMA B fragments, hi / lo bf16 parts -- attn_rel.hip's prologue
__device__ __forceinline__ void build_w_fragments(int tid, const float *__restrict__ Wp, u32x4 *wfr)
{
    if (tid < 128) {
        const int part = tid >> 6, l = tid & 63, head = l & 15, gg = l >> 4;
        unsigned int o[4] = {0u, 0u, 0u, 0u};
        if (head < kAbH) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float w0 = Wp[head * 64 + 8 * gg + 2 * j] * kAbLog2e, w1 = Wp[head * 64 + 8 * gg + 2 * j + 1] * kAbLog2e;
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

// per-query constants and size-ratio coefficients U of the 16 queries from q0 on -- attn_rel.hip's prologue (1024 threads)
__device__ __forceinline__ void build_query_tile(int tid, int b, int q0, int N, const float *__restrict__ src,
                                                 const float *__restrict__ Wp, float eps, const AbFreq &fr, float *qc, u32x4 *ufr)
{
    if (tid < kAbTileQ) {
        const int qi = q0 + tid < N ? q0 + tid : N - 1;
        const f32x4 s = *reinterpret_cast<const f32x4 *>(src + ((size_t)b * N + qi) * 4);
        float *r = qc + tid * kAbQC;
        r[0] = s.x; r[1] = s.y; r[2] = 1.0f / (s.z + eps); r[3] = 1.0f / (s.w + eps);
    }
    const int qq = tid >> 6, l = tid & 63, head = l & 15, gg = l >> 4, cc = gg >> 1, k0 = 4 * (gg & 1);
    const int qi = q0 + qq < N ? q0 + qq : N - 1;
    unsigned int hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
    if (head < kAbH) {
        const float l2 = __builtin_amdgcn_logf(src[((size_t)b * N + qi) * 4 + 2 + cc] + eps);
        const float *wrow = Wp + head * 64 + 32 + 16 * cc + 2 * k0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = l2 * fr.cf[k0 + j];
            const float ss = __builtin_amdgcn_sinf(x), sc = __builtin_amdgcn_cosf(x);
            const float ws = wrow[2 * j] * kAbLog2e, wc = wrow[2 * j + 1] * kAbLog2e;
            const float us = __builtin_fmaf(wc, ss, -(ws * sc)), uc = __builtin_fmaf(ws, ss, wc * sc);
            hi[j] = pack_bf16x2(us, uc);
            lo[j] = pack_bf16x2(us - bf16_bits_to_f32(hi[j] & 0xffffu), uc - bf16_bits_to_f32(hi[j] >> 16));
        }
    }
    ufr[(qq * 2 + 0) * 64 + l] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    ufr[(qq * 2 + 1) * 64 + l] = u32x4{lo[0], lo[1], lo[2], lo[3]};
}

// The key side of a wave's pair sets: lane (key = lane & 15, g) -> its distance coordinate and the table fragment (sin a_k, cos a_k)
struct AbKey {
    float tcoord;
    u32x4 a1;
};
__device__ __forceinline__ AbKey key_side(const f32x4 &kbox, int g, float eps, const AbFreq &fr)
{
    const int c01 = g >> 1, fsel = g & 1;
    const float cf0 = fr.cf[4 * fsel + 0], cf1 = fr.cf[4 * fsel + 1], cf2 = fr.cf[4 * fsel + 2], cf3 = fr.cf[4 * fsel + 3];
    AbKey r;
    r.tcoord = c01 ? kbox.y : kbox.x;
    const float l2k = __builtin_amdgcn_logf((c01 ? kbox.w : kbox.z) + eps);
    const float y0 = l2k * cf0, y1 = l2k * cf1, y2 = l2k * cf2, y3 = l2k * cf3;
    r.a1 = u32x4{pack_bf16x2(__builtin_amdgcn_sinf(y0), __builtin_amdgcn_cosf(y0)),
                 pack_bf16x2(__builtin_amdgcn_sinf(y1), __builtin_amdgcn_cosf(y1)),
                 pack_bf16x2(__builtin_amdgcn_sinf(y2), __builtin_amdgcn_cosf(y2)),
                 pack_bf16x2(__builtin_amdgcn_sinf(y3), __builtin_amdgcn_cosf(y3))};
    return r;
}

// One pair set (query qq of the tile x the lane's key): the forward's features, projection and ReLU.  Returns the distance feature
// fragment; lane (head = lane & 15 < 8, g) writes relu(bias) * log2(e) of keys 4 g .. 4 g + 3 to dst + qq * kAbQStride.
__device__ __forceinline__ u32x4 pair_set(int qq, int lane, int g, const AbKey &ks, const float *qc, const u32x4 *wfr, const u32x4 *ufr,
                                          float bph, const AbFreq &fr, float *dst)
{
    const int c01 = g >> 1, fsel = g & 1;
    const float cf0 = fr.cf[4 * fsel + 0], cf1 = fr.cf[4 * fsel + 1], cf2 = fr.cf[4 * fsel + 2], cf3 = fr.cf[4 * fsel + 3];
    const u32x4 w0h = wfr[lane], w0l = wfr[64 + lane];
    const float *qr = qc + qq * kAbQC;
    const float sc = qr[c01], inv = qr[2 + c01];
    const u32x4 uh = ufr[(qq * 2 + 0) * 64 + lane], ul = ufr[(qq * 2 + 1) * 64 + lane];
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
    acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
    if ((lane & 15) < kAbH) *reinterpret_cast<f32x4 *>(dst + qq * kAbQStride) = acc;
    return a0;
}

// Di = rowsum(dO o O) per (image, head, query): one thread per (b, q, h), fixed order over the 32 columns (csrc/attn_bwd.hip)
__global__ __launch_bounds__(256) void relation_attention_boxes_bwd_di_kernel(const uint16_t *__restrict__ out, int ldo,
                                                                              const uint16_t *__restrict__ dout, int lddo, int N,
                                                                              long long total, float *__restrict__ di)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int h = (int)(idx % kAbH);
    const long long bq = idx / kAbH;                         // b * N + q
    const long long b = bq / N, qi = bq - b * N;
    const u32x2 *o = reinterpret_cast<const u32x2 *>(out + bq * ldo + h * kAbD);
    const u32x2 *d = reinterpret_cast<const u32x2 *>(dout + bq * lddo + h * kAbD);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kAbD / 4; ++i) {
        const u32x2 a = o[i], c = d[i];
        s += bf16_bits_to_f32(a.x & 0xffffu) * bf16_bits_to_f32(c.x & 0xffffu);
        s += bf16_bits_to_f32(a.x >> 16) * bf16_bits_to_f32(c.x >> 16);
        s += bf16_bits_to_f32(a.y & 0xffffu) * bf16_bits_to_f32(c.y & 0xffffu);
        s += bf16_bits_to_f32(a.y >> 16) * bf16_bits_to_f32(c.y >> 16);
    }
    di[(b * kAbH + h) * N + qi] = s;
}

// dQ of 16 queries x 8 heads, and this query tile's contribution to grad_weight / grad_bias; see the header comment
__global__ __launch_bounds__(kAbWaves *kWave) void relation_attention_boxes_bwd_dq_kernel(
    const uint16_t *__restrict__ q, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v, int ldq, int ldk, int ldv,
    const uint16_t *__restrict__ dout, int lddo, const float *__restrict__ lse2, const float *__restrict__ di,
    const float *__restrict__ src, const float *__restrict__ tgt, const float *__restrict__ Wp, const float *__restrict__ bp,
    const unsigned char *__restrict__ mask, int N, int M, float scale_log2e, float scale, float eps, AbFreq fr,
    uint16_t *__restrict__ dq, int lddq, float *__restrict__ records)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ab_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, q0 = blockIdx.x * kAbTileQ;
    float *bias_lds = reinterpret_cast<float *>(ab_lds + kAbLdsBias);
    float *qc = reinterpret_cast<float *>(ab_lds + kAbLdsQC);
    u32x4 *wfr = reinterpret_cast<u32x4 *>(ab_lds + kAbLdsW);
    u32x4 *ufr = reinterpret_cast<u32x4 *>(ab_lds + kAbLdsU);
    unsigned char *img = ab_lds + kAbLdsImg + wave * kAbImg;

    build_w_fragments(tid, Wp, wfr);
    build_query_tile(tid, b, q0, N, src, Wp, eps, fr, qc, ufr);
    __syncthreads();

    // ---- feature role: key block kbw of a chunk, queries qbase .. qbase + 3 of the tile ----
    const int kbw = wave >> 2, qbase = (wave & 3) * 4;
    const float bph = (bp && ql < kAbH) ? bp[ql] * kAbLog2e : 0.f;
    float *dst = bias_lds + ql * kAbHeadStride + 16 * kbw + 4 * g;       // + qq * kAbQStride: this lane's 4 keys of a pair set
    f32x4 gw[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};                // gradW^T[ch = 16 cb + 4 g + r][head = ql], channels 0-31
    f32x4 tacc[4][2];                                                    // T^T[entry = 16 cb + 4 g + r][head = ql] of query qbase + i
#pragma unroll
    for (int i = 0; i < 4; ++i) tacc[i][0] = tacc[i][1] = f32x4{0, 0, 0, 0};
    float gbsum = 0.f;

    // ---- attention role: head h, keys 32 pair .. + 31 of a chunk ----
    const int h = wave & 7, pair = wave >> 3;
    const int qi = q0 + ql;
    const bool qok = qi < N;
    const int qcl = qok ? qi : N - 1;
    const size_t bh = (size_t)b * kAbH + h;
    const u32x4 qfrag = *reinterpret_cast<const u32x4 *>(q + ((size_t)b * N + qcl) * ldq + h * kAbD + g * 8);
    const u32x4 dofrag = *reinterpret_cast<const u32x4 *>(dout + ((size_t)b * N + qcl) * lddo + h * kAbD + g * 8);
    const float l2 = qok ? bwd_lse(lse2[bh * N + qcl]) : __builtin_inff();
    const float dd = di[bh * N + qcl];
    const unsigned char *mask_row = mask ? mask + (size_t)qcl * M : nullptr;
    const uint16_t *kbase = k + (size_t)b * M * ldk + h * kAbD;
    const uint16_t *vbase = v + (size_t)b * M * ldv + h * kAbD;
    // K / V rows through buffer loads: rows past the last key come back as zeros from the descriptor's range check
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(kbase), 0,
                                                                         (unsigned)((M - 1) * ldk + kAbD) * 2u, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(vbase), 0,
                                                                         (unsigned)((M - 1) * ldv + kAbD) * 2u, 0x00020000);
    const unsigned kvo = (unsigned)(ql * ldk + g * 8) * 2u, vvo = (unsigned)(ql * ldv + g * 8) * 2u;
    f32x4 dqacc[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};             // dQ^T[d = 16 cb + 4 g + r][q = ql]

    const int nch = (M + kAbChunk - 1) / kAbChunk;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
        const int key0 = c * kAbChunk;
        // this chunk's K / V rows of the attention role: in flight across phase F
        u32x4 kf[2], vf[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            kf[half] = __builtin_amdgcn_raw_buffer_load_b128(krs, kvo, (unsigned)((key0 + 32 * pair + 16 * half) * ldk) * 2u, 0);
            vf[half] = __builtin_amdgcn_raw_buffer_load_b128(vrs, vvo, (unsigned)((key0 + 32 * pair + 16 * half) * ldv) * 2u, 0);
        }

        // ---- F ----
        const int fkey = key0 + 16 * kbw + ql < M ? key0 + 16 * kbw + ql : M - 1;
        const AbKey ks = key_side(*reinterpret_cast<const f32x4 *>(tgt + ((size_t)b * M + fkey) * 4), g, eps, fr);
        u32x4 a0[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a0[i] = pair_set(qbase + i, lane, g, ks, qc, wfr, ufr, bph, fr, dst);
        *reinterpret_cast<u32x4 *>(img + (32 + ql) * kAbTS + 16 * g) = ks.a1;          // the key table [key][entry], read back in phase G
        __syncthreads();

        // ---- A ----
        {
#pragma unroll
            for (int half = 0; half < 2; ++half) *reinterpret_cast<u32x4 *>(img + (16 * half + ql) * kAbTS + 16 * g) = kf[half];
            wave_sync();
            f32x4 dsv[2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int kb = 2 * pair + half;
                float *brow = bias_lds + h * kAbHeadStride + ql * kAbQStride + 16 * kb + 4 * g;
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(kf[half]), as_bf16x8(qfrag), s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(vf[half]), as_bf16x8(dofrag), dp, 0, 0, 0);
                const f32x4 t0 = *reinterpret_cast<const f32x4 *>(brow);                // relu(bias) * log2(e): >= 0
                f32x4 t = t0;
                const int kk = key0 + 16 * kb + 4 * g;
                if (mask_row != nullptr || key0 + kAbChunk > M) {                       // wave-uniform; the forward's statements
                    if (mask_row) {
                        if (kk + 0 < M && mask_row[kk + 0]) t.x = -__builtin_inff();
                        if (kk + 1 < M && mask_row[kk + 1]) t.y = -__builtin_inff();
                        if (kk + 2 < M && mask_row[kk + 2]) t.z = -__builtin_inff();
                        if (kk + 3 < M && mask_row[kk + 3]) t.w = -__builtin_inff();
                    }
                    if (kk + 0 >= M) t.x = -__builtin_inff();                           // keys past the end never take part
                    if (kk + 1 >= M) t.y = -__builtin_inff();
                    if (kk + 2 >= M) t.z = -__builtin_inff();
                    if (kk + 3 >= M) t.w = -__builtin_inff();
                }
                f32x4 ds, gg;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = __builtin_fmaf(s[r], scale_log2e, t[r]);
                    const float p = __builtin_amdgcn_exp2f(z - l2);
                    ds[r] = p == 0.f ? 0.f : p * (dp[r] - dd);
                    gg[r] = t0[r] > 0.f ? ds[r] : 0.f;                                  // ReLU': the regenerated bias is > 0
                }
                dsv[half] = ds;
                *reinterpret_cast<f32x4 *>(brow) = gg;
            }
            const u32x4 sf = {pack_bf16x2(dsv[0].x, dsv[0].y), pack_bf16x2(dsv[0].z, dsv[0].w), pack_bf16x2(dsv[1].x, dsv[1].y),
                              pack_bf16x2(dsv[1].z, dsv[1].w)};
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const u32x4 tk = tr_rows8(img, 0, cb, lane);
                dqacc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(tk), as_bf16x8(sf), dqacc[cb], 0, 0, 0);
            }
        }
        __syncthreads();

        // ---- G ----
        {
            const u32x2 ta[2] = {tr_rows4(img, 32, 0, lane), tr_rows4(img, 32, 1, lane)};
#pragma unroll
            for (int i0 = 0; i0 < 4; i0 += 2) {
                f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
                if (ql < kAbH) {
                    g0 = *reinterpret_cast<const f32x4 *>(dst + (qbase + i0) * kAbQStride);
                    g1 = *reinterpret_cast<const f32x4 *>(dst + (qbase + i0 + 1) * kAbQStride);
                }
                gbsum += ((g0.x + g0.y) + (g0.z + g0.w)) + ((g1.x + g1.y) + (g1.z + g1.w));
                const u32x4 gf = {pack_bf16x2(g0.x, g0.y), pack_bf16x2(g0.z, g0.w), pack_bf16x2(g1.x, g1.y), pack_bf16x2(g1.z, g1.w)};
                wave_sync();                                                            // the image's previous readers are done
                *reinterpret_cast<u32x4 *>(img + ql * kAbTS + 16 * g) = a0[i0];
                *reinterpret_cast<u32x4 *>(img + (16 + ql) * kAbTS + 16 * g) = a0[i0 + 1];
                wave_sync();
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const u32x4 tf = tr_rows8(img, 0, cb, lane);
                    gw[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(tf), as_bf16x8(gf), gw[cb], 0, 0, 0);
                    tacc[i0][cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(as_s16x4(ta[cb]), as_s16x4(u32x2{gf.x, gf.y}),
                                                                             tacc[i0][cb], 0, 0, 0);
                    tacc[i0 + 1][cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(as_s16x4(ta[cb]), as_s16x4(u32x2{gf.z, gf.w}),
                                                                                 tacc[i0 + 1][cb], 0, 0, 0);
                }
            }
            wave_sync();                                                                // before phase A rewrites the image
        }
        // no workgroup barrier here: phase F of the next chunk writes the bias entries THIS lane has just read
    }

    // ---- size-ratio half: combine T with (sin a_q, cos a_q) of the wave's 4 queries ----
    // lane (head, g) holds entries 16 cb + 4 g + r = (Ts, Tc) of the (coordinate, frequency) slots m = 8 cb + 2 g, m + 1;
    //   d/dW_sin = sin a_q Tc - cos a_q Ts,   d/dW_cos = cos a_q Tc + sin a_q Ts
    f32x4 gs[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qx = q0 + qbase + i;
        if (qx < N) {
            const float *sb = src + ((size_t)b * N + qx) * 4;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
                for (int mm = 0; mm < 2; ++mm) {
                    const int m = 8 * cb + 2 * g + mm;
                    const float x = __builtin_amdgcn_logf(sb[2 + (m >> 3)] + eps) * fr.cf[m & 7];
                    const float sq = __builtin_amdgcn_sinf(x), cq = __builtin_amdgcn_cosf(x);
                    const float ts = tacc[i][cb][2 * mm], tc = tacc[i][cb][2 * mm + 1];
                    gs[cb][2 * mm] += __builtin_fmaf(sq, tc, -(cq * ts));
                    gs[cb][2 * mm + 1] += __builtin_fmaf(cq, tc, sq * ts);
                }
            }
        }
    }

    // ---- epilogue: dQ (the two key halves of a head added in a fixed order), then the workgroup's record ----
    __syncthreads();                                                                    // every wave is done with its image
    float *red = reinterpret_cast<float *>(ab_lds + kAbLdsImg);
    if (pair == 1) {
        *reinterpret_cast<f32x4 *>(red + ((h * 2 + 0) * 64 + lane) * 4) = dqacc[0];
        *reinterpret_cast<f32x4 *>(red + ((h * 2 + 1) * 64 + lane) * 4) = dqacc[1];
    }
    __syncthreads();
    if (pair == 0 && qok) {
        uint16_t *o = dq + ((size_t)b * N + qi) * lddq + h * kAbD + 4 * g;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const f32x4 o1 = *reinterpret_cast<const f32x4 *>(red + ((h * 2 + cb) * 64 + lane) * 4);
            const f32x4 a = dqacc[cb] + o1;
            *reinterpret_cast<u32x2 *>(o + 16 * cb) = u32x2{pack_bf16x2(a.x * scale, a.y * scale), pack_bf16x2(a.z * scale, a.w * scale)};
        }
    }
    __syncthreads();
    gbsum += __shfl_xor(gbsum, 16, 64);
    gbsum += __shfl_xor(gbsum, 32, 64);
    if (ql < kAbH) {
        float *r = red + wave * kAbRecord;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                r[ql * 64 + 16 * cb + 4 * g + rr] = gw[cb][rr];
                r[ql * 64 + 32 + 16 * cb + 4 * g + rr] = gs[cb][rr];
            }
        if (g == 0) r[kAbH * 64 + ql] = gbsum;
    }
    __syncthreads();
    if (tid < kAbRecord) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < kAbWaves; ++w) s += red[w * kAbRecord + tid];
        records[((size_t)b * gridDim.x + blockIdx.x) * kAbRecord + tid] = s;
    }
}

// dK, dV of 64 keys x 8 heads; see the header comment.  kSplit: blockIdx.z sweeps its share of the query tiles and writes fp32
// partials [split][b * M + key][dK 256 | dV 256] (unscaled) for relation_attention_boxes_bwd_dkv_reduce_kernel
template <bool kSplit>
__global__ __launch_bounds__(kAbWaves *kWave) void relation_attention_boxes_bwd_dkv_kernel(
    const uint16_t *__restrict__ q, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v, int ldq, int ldk, int ldv,
    const uint16_t *__restrict__ dout, int lddo, const float *__restrict__ lse2, const float *__restrict__ di,
    const float *__restrict__ src, const float *__restrict__ tgt, const float *__restrict__ Wp, const float *__restrict__ bp,
    const unsigned char *__restrict__ mask, int N, int M, float scale_log2e, float scale, float eps, AbFreq fr,
    uint16_t *__restrict__ dk, int lddk, uint16_t *__restrict__ dv, int lddv, float *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ab_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kl = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, key0 = blockIdx.x * kAbChunk;
    float *bias_lds = reinterpret_cast<float *>(ab_lds + kAbLdsBias);
    float *qc = reinterpret_cast<float *>(ab_lds + kAbLdsQC);
    u32x4 *wfr = reinterpret_cast<u32x4 *>(ab_lds + kAbLdsW);
    u32x4 *ufr = reinterpret_cast<u32x4 *>(ab_lds + kAbLdsU);

    build_w_fragments(tid, Wp, wfr);

    // ---- feature role: key block kbw of the workgroup's chunk (fixed), queries qbase .. qbase + 3 of every tile ----
    const int kbw = wave >> 2, qbase = (wave & 3) * 4;
    const float bph = (bp && kl < kAbH) ? bp[kl] * kAbLog2e : 0.f;
    float *dst = bias_lds + kl * kAbHeadStride + 16 * kbw + 4 * g;
    const int fkey = key0 + 16 * kbw + kl < M ? key0 + 16 * kbw + kl : M - 1;
    const AbKey ks = key_side(*reinterpret_cast<const f32x4 *>(tgt + ((size_t)b * M + fkey) * 4), g, eps, fr);

    // ---- attention role: head h, key blocks 2 pair + {0, 1}; the lane's keys ----
    const int h = wave & 7, pair = wave >> 3;
    const size_t bh = (size_t)b * kAbH + h;
    u32x4 kfrag[2], vfrag[2];
    bool kok[2];
    int keyv[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        keyv[half] = key0 + 32 * pair + 16 * half + kl;
        kok[half] = keyv[half] < M;
        const int kc = kok[half] ? keyv[half] : M - 1;
        kfrag[half] = *reinterpret_cast<const u32x4 *>(k + ((size_t)b * M + kc) * ldk + h * kAbD + g * 8);
        vfrag[half] = *reinterpret_cast<const u32x4 *>(v + ((size_t)b * M + kc) * ldv + h * kAbD + g * 8);
    }
    f32x4 acc_dk[2][2], acc_dv[2][2];                                    // [half][cb]: [d = 16 cb + 4 g + r][key = kl]
#pragma unroll
    for (int i = 0; i < 2; ++i) acc_dk[i][0] = acc_dk[i][1] = acc_dv[i][0] = acc_dv[i][1] = f32x4{0, 0, 0, 0};

    const int ntile = (N + kAbTileQ - 1) / kAbTileQ;
    const int tper = kSplit ? (ntile + (int)gridDim.z - 1) / (int)gridDim.z : ntile;
    const int tbeg = kSplit ? (int)blockIdx.z * tper : 0, tend = tbeg + tper < ntile ? tbeg + tper : ntile;
#pragma unroll 1
    for (int t = tbeg; t < tend; ++t) {
        const int q0 = t * kAbTileQ;
        // the tile's operands of the attention role, in flight across the prologue and phase F
        const int qrow = q0 + kl < N ? q0 + kl : N - 1;
        const u32x4 aq = *reinterpret_cast<const u32x4 *>(q + ((size_t)b * N + qrow) * ldq + h * kAbD + g * 8);      // Q / dO rows: A of S, dP
        const u32x4 ad = *reinterpret_cast<const u32x4 *>(dout + ((size_t)b * N + qrow) * lddo + h * kAbD + g * 8);
        unsigned short tq[2][4], td[2][4];                              // Q^T / dO^T [d = 16 cb + kl][query 4 g + j]: A of dK^T, dV^T
        float lq[4], dq_[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int qx = q0 + 4 * g + j;
            const bool ok = qx < N;
            const size_t row = (size_t)b * N + (ok ? qx : N - 1);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const unsigned short a = q[row * ldq + h * kAbD + 16 * cb + kl], d = dout[row * lddo + h * kAbD + 16 * cb + kl];
                tq[cb][j] = ok ? a : (unsigned short)0;
                td[cb][j] = ok ? d : (unsigned short)0;
            }
            lq[j] = ok ? bwd_lse(lse2[bh * N + qx]) : __builtin_inff();                 // queries past N: P = 0
            dq_[j] = ok ? di[bh * N + qx] : 0.f;
        }

        build_query_tile(tid, b, q0, N, src, Wp, eps, fr, qc, ufr);
        __syncthreads();
        // ---- F ----
#pragma unroll
        for (int i = 0; i < 4; ++i) (void)pair_set(qbase + i, lane, g, ks, qc, wfr, ufr, bph, fr, dst);
        __syncthreads();
        // ---- A ----
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int kb = 2 * pair + half;
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(aq), as_bf16x8(kfrag[half]), s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ad), as_bf16x8(vfrag[half]), dp, 0, 0, 0);
            float pv[4], dsv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = 4 * g + r, qx = q0 + ql;
                float tb = bias_lds[h * kAbHeadStride + ql * kAbQStride + 16 * kb + kl];
                if (!kok[half] || (mask && qx < N && mask[(size_t)qx * M + keyv[half]])) tb = -__builtin_inff();
                const float z = __builtin_fmaf(s[r], scale_log2e, tb);
                const float p = __builtin_amdgcn_exp2f(z - lq[r]);
                pv[r] = p;
                dsv[r] = p == 0.f ? 0.f : p * (dp[r] - dq_[r]);
            }
            const u32x2 pf = {pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3])};
            const u32x2 sf = {pack_bf16x2(dsv[0], dsv[1]), pack_bf16x2(dsv[2], dsv[3])};
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const u32x2 tdo = {(unsigned)td[cb][0] | ((unsigned)td[cb][1] << 16), (unsigned)td[cb][2] | ((unsigned)td[cb][3] << 16)};
                const u32x2 tqq = {(unsigned)tq[cb][0] | ((unsigned)tq[cb][1] << 16), (unsigned)tq[cb][2] | ((unsigned)tq[cb][3] << 16)};
                acc_dv[half][cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(as_s16x4(tdo), as_s16x4(pf), acc_dv[half][cb], 0, 0, 0);
                acc_dk[half][cb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(as_s16x4(tqq), as_s16x4(sf), acc_dk[half][cb], 0, 0, 0);
            }
        }
        __syncthreads();                                                                // the next tile rewrites qc, U and the bias tile
    }
    if constexpr (kSplit) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (kok[half]) {
                float *pp = part + (((size_t)blockIdx.z * gridDim.y + b) * M + keyv[half]) * (2 * kAbH * kAbD) + h * kAbD + 4 * g;
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    *reinterpret_cast<f32x4 *>(pp + 16 * cb) = acc_dk[half][cb];
                    *reinterpret_cast<f32x4 *>(pp + kAbH * kAbD + 16 * cb) = acc_dv[half][cb];
                }
            }
        }
        return;
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (kok[half]) {                                                                // lane (key, g) holds d = 16 cb + 4 g + r of its key
            uint16_t *pk = dk + ((size_t)b * M + keyv[half]) * lddk + h * kAbD + 4 * g;
            uint16_t *pvv = dv + ((size_t)b * M + keyv[half]) * lddv + h * kAbD + 4 * g;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const f32x4 a = acc_dk[half][cb], c = acc_dv[half][cb];
                *reinterpret_cast<u32x2 *>(pk + 16 * cb) = u32x2{pack_bf16x2(a.x * scale, a.y * scale), pack_bf16x2(a.z * scale, a.w * scale)};
                *reinterpret_cast<u32x2 *>(pvv + 16 * cb) = u32x2{pack_bf16x2(c.x, c.y), pack_bf16x2(c.z, c.w)};
            }
        }
    }
}

// grad_weight[h][ch] / grad_bias[h] = the sum of the workgroup records, in workgroup order.  One wave per output, lanes stride over
// the records, fixed-order shuffle tree: the same bits from run to run (csrc/relation_bwd.hip).
__global__ __launch_bounds__(kWave) void relation_attention_boxes_bwd_reduce_kernel(const float *__restrict__ records, int nrec,
                                                                                   float *__restrict__ grad_weight,
                                                                                   float *__restrict__ grad_bias)
{
    const int o = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int x = lane; x < nrec; x += kWave) s += records[(size_t)x * kAbRecord + o];
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (lane == 0) {
        if (o < kAbH * 64) grad_weight[o] = s;
        else if (grad_bias) grad_bias[o - kAbH * 64] = s;
    }
}

// dK / dV = the splits' partials added in split order; thread = (b * M + key, dK | dV, 4 columns)
__global__ __launch_bounds__(256) void relation_attention_boxes_bwd_dkv_reduce_kernel(const float *__restrict__ part, int nsplit,
                                                                                       long long rows, float scale,
                                                                                       uint16_t *__restrict__ dk, int lddk,
                                                                                       uint16_t *__restrict__ dv, int lddv)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * 128) return;
    const long long row = idx >> 7;
    const int which = (int)(idx >> 6) & 1, col = ((int)idx & 63) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int sp = 0; sp < nsplit; ++sp)
        a += *reinterpret_cast<const f32x4 *>(part + ((size_t)sp * rows + row) * 512 + which * 256 + col);
    const float f = which ? 1.0f : scale;
    uint16_t *o = which ? dv + row * lddv + col : dk + row * lddk + col;
    *reinterpret_cast<u32x2 *>(o) = u32x2{pack_bf16x2(a.x * f, a.y * f), pack_bf16x2(a.z * f, a.w * f)};
}

// the dkv kernel has one workgroup per 64 keys and image: too few for the device at decoder sizes, so the query sweep is split
int dkv_splits(int N)
{
    const int ntile = (N + kAbTileQ - 1) / kAbTileQ;
    return ntile >= 16 ? 4 : 1;
}

long long di_bytes(int B, int H, int N) { return ((long long)B * H * N * 4 + 255) / 256 * 256; }

}  // namespace

}  // namespace rdetr

extern "C" long long rdetr_relation_attention_boxes_backward_workspace_bytes(int B, int H, int N, int M)
{
    using namespace rdetr;
    if (B <= 0 || H <= 0 || N <= 0 || M <= 0) return 0;
    // Di fp32 [B*H, N], one 520-float record per (image, 16-query tile), fp32 dK / dV partials of the split query sweep
    const int ns = dkv_splits(N);
    return di_bytes(B, H, N) + (long long)B * ((N + kAbTileQ - 1) / kAbTileQ) * kAbRecord * 4 +
           (ns > 1 ? (long long)ns * B * M * 2 * kAbH * kAbD * 4 : 0);
}

extern "C" int rdetr_relation_attention_boxes_backward_bf16(
    const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv, const uint16_t *out, int ldo, const float *lse,
    const uint16_t *dout, int lddo, const float *src_boxes, const float *tgt_boxes, const float *proj_weight, const float *proj_bias,
    const uint8_t *bool_mask, int B, int H, int D, int N, int M, int F, float rel_scale, float temperature, float eps, float attn_scale,
    void *workspace, long long workspace_bytes, uint16_t *dq, int lddq, uint16_t *dk, int lddk, uint16_t *dv, int lddv,
    float *grad_weight, float *grad_bias, void *stream)
{
    using namespace rdetr;
    if (B <= 0 || H <= 0 || N <= 0 || M <= 0 || D <= 0 || F <= 0) return RDETR_ERR_INVALID_ARG;
    if (!q || !k || !v || !out || !lse || !dout || !src_boxes || !tgt_boxes || !proj_weight || !workspace || !dq || !dk || !dv ||
        !grad_weight)
        return RDETR_ERR_INVALID_ARG;
    if (D != kAbD || H != kAbH || F != kAbF) return RDETR_ERR_UNSUPPORTED;
    const long long span = (long long)H * D;
    if (ldq < span || ldk < span || ldv < span || ldo < span || lddo < span || lddq < span || lddk < span || lddv < span)
        return RDETR_ERR_INVALID_ARG;
    if (workspace_bytes < rdetr_relation_attention_boxes_backward_workspace_bytes(B, H, N, M)) return RDETR_ERR_INVALID_ARG;
    auto al = [](const void *p, unsigned a) { return reinterpret_cast<uintptr_t>(p) % a == 0; };
    if (!al(q, 16) || !al(k, 16) || !al(v, 16) || !al(dout, 16) || ldq % 8 || ldk % 8 || ldv % 8 || lddo % 8) return RDETR_ERR_UNSUPPORTED;
    if (!al(out, 8) || !al(dq, 8) || !al(dk, 8) || !al(dv, 8) || ldo % 4 || lddq % 4 || lddk % 4 || lddv % 4) return RDETR_ERR_UNSUPPORTED;
    if (!al(lse, 4) || !al(workspace, 16) || !al(src_boxes, 16) || !al(tgt_boxes, 16) || !al(proj_weight, 4) || !al(grad_weight, 4) ||
        (proj_bias && !al(proj_bias, 4)) || (grad_bias && !al(grad_bias, 4)))
        return RDETR_ERR_UNSUPPORTED;
    if (B > 65535 || (long long)M * (ldk > ldv ? ldk : ldv) * 2 >= (1ll << 31)) return RDETR_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    AbFreq fr;
    for (int i = 0; i < F / 2; ++i) {
        const double dim_t = (double)powf(temperature, (float)i * 2.0f / (float)F);       // get_dim_t, position_encoding.py:101-105
        fr.cf[i] = (float)(0.6931471805599453 * (double)rel_scale / (dim_t * 6.283185307179586));
    }
    static const hipError_t attr_dq = hipFuncSetAttribute(reinterpret_cast<const void *>(relation_attention_boxes_bwd_dq_kernel),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, kAbLdsBytesDq);
    static const hipError_t attr_dkv = hipFuncSetAttribute(reinterpret_cast<const void *>(relation_attention_boxes_bwd_dkv_kernel<false>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, kAbLdsBytesDkv);
    static const hipError_t attr_dkvs = hipFuncSetAttribute(reinterpret_cast<const void *>(relation_attention_boxes_bwd_dkv_kernel<true>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, kAbLdsBytesDkv);
    if (attr_dq != hipSuccess || attr_dkv != hipSuccess || attr_dkvs != hipSuccess) return RDETR_ERR_LAUNCH;
    float *di = static_cast<float *>(workspace);
    float *records = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + di_bytes(B, H, N));
    const float sl = attn_scale * kAbLog2e;
    const long long rows = (long long)B * H * N;
    const int qtiles = (N + kAbTileQ - 1) / kAbTileQ, kchunks = (M + kAbChunk - 1) / kAbChunk;
    hipLaunchKernelGGL(relation_attention_boxes_bwd_di_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, out, ldo, dout,
                       lddo, N, rows, di);
    hipLaunchKernelGGL(relation_attention_boxes_bwd_dq_kernel, dim3((unsigned)qtiles, (unsigned)B), dim3(kAbWaves * kWave), kAbLdsBytesDq,
                       st, q, k, v, ldq, ldk, ldv, dout, lddo, lse, di, src_boxes, tgt_boxes, proj_weight, proj_bias, bool_mask, N, M, sl,
                       attn_scale, eps, fr, dq, lddq, records);
    const int ns = dkv_splits(N);
    if (ns > 1) {
        float *part = records + (size_t)B * qtiles * kAbRecord;
        const long long krows = (long long)B * M;
        hipLaunchKernelGGL(relation_attention_boxes_bwd_dkv_kernel<true>, dim3((unsigned)kchunks, (unsigned)B, (unsigned)ns),
                           dim3(kAbWaves * kWave), kAbLdsBytesDkv, st, q, k, v, ldq, ldk, ldv, dout, lddo, lse, di, src_boxes, tgt_boxes,
                           proj_weight, proj_bias, bool_mask, N, M, sl, attn_scale, eps, fr, dk, lddk, dv, lddv, part);
        hipLaunchKernelGGL(relation_attention_boxes_bwd_dkv_reduce_kernel, dim3((unsigned)((krows * 128 + 255) / 256)), dim3(256), 0, st,
                           part, ns, krows, attn_scale, dk, lddk, dv, lddv);
    } else {
        hipLaunchKernelGGL(relation_attention_boxes_bwd_dkv_kernel<false>, dim3((unsigned)kchunks, (unsigned)B), dim3(kAbWaves * kWave),
                           kAbLdsBytesDkv, st, q, k, v, ldq, ldk, ldv, dout, lddo, lse, di, src_boxes, tgt_boxes, proj_weight,
                           proj_bias, bool_mask, N, M, sl, attn_scale, eps, fr, dk, lddk, dv, lddv, nullptr);
    }
    hipLaunchKernelGGL(relation_attention_boxes_bwd_reduce_kernel, dim3(kAbRecord), dim3(kWave), 0, st, records, B * qtiles, grad_weight,
                       grad_bias);
    return launch_status();
}
