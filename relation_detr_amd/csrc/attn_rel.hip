// Decoder self-attention that GENERATES its position-relation bias: softmax(Q K^T * scale + relu(W . feat(box_q, box_k) + b)) V
// in one kernel (gfx950) -- SURVEY.md section 8 f1 as written.
//
// Replaces, for bf16 inference, PositionRelationEmbedding.forward (models/bricks/relation_transformer.py:520-532) followed by the
// nn.MultiheadAttention call that takes its result as a float attn_mask (:369-374, :452-461): the [B, 8, N, N] fp32 bias (26 MB per
// image and layer at N = 900) is never written to or read from HBM, and the 64 -> 8 projection of the sine features moves from 512
// VALU FMAs per (query, key) pair onto the matrix cores.
//
//   grid      = (ceil(N / 16) query tiles, B images); workgroup = 16 waves that own 16 queries for ALL 8 heads, so that the sine
//               features of a (query, key) pair are computed once and shared by the heads
//   keys      = chunks of 64.  Per chunk the 16 x 64 pairs are 64 "pair sets" (one query x 16 consecutive keys), each projected by
//               four MFMAs, ReLU'd and written to LDS as [head][query][key] fp32, pre-multiplied by log2(e) for the soft-max:
//               the generator of csrc/relation_gen.h, which the backward (csrc/attn_rel_bwd.hip) runs too -- the arithmetic of
//               the bias is defined there, once; this file owns the schedule
//               waves 8-15 compute 8 pair sets each per chunk; waves 0-7 run the attention of head = wave for the chunk whose bias
//               tile the feature waves finished one barrier earlier (two bias tiles in LDS: one barrier per chunk).  Disjoint
//               roles in two separate loops keep either path inside the 128 VGPRs a 16-wave workgroup has
//   attention = as csrc/attn.hip (transposed products, online soft-max in the log2 domain, P rounded to bf16, V^T through
//               ds_read_b64_tr_b16; the mask rule and the transposed read are csrc/attn_common.h's), one wave per head over all
//               keys; K fragments come straight from global memory into registers, V through a wave-private LDS image; the
//               soft-max denominator is the MFMA product ones . P^T of the rounded P
//   numerics  = the features / table entries are rounded to bf16 (2^-9) for the projection, the weights are not (hi + lo split);
//               the angles use the hardware log2 / sin / cos (|angle| < 256 revolutions for any box of size >= 1e-5).  This is the
//               bf16 inference path: its results are held to the same 2^-7 bound against the fp32 oracle as the materialised-bias
//               attention kernel.  bf16 training can take the same route (kLse below + csrc/attn_rel_bwd.hip,
//               Options.rel_train_fused); fp32 runs and training by default keep rdetr_relation_bias_f32 (reference op order,
//               IEEE division, Cody-Waite sin / cos).
//   cost      = VALU-bound (one wave-instruction per clock and CU): ~50 issue slots per pair set, 36 of them the quarter-rate
//               log2 / sin / cos, + ~160 per head and chunk for the soft-max
#include <type_traits>

#include "relation_gen.h"

namespace rdetr {

constexpr int kArVS = 96;                                       // V image row stride in bytes (conflict-free transposed reads)
constexpr int kArVImg = kRelChunk * kArVS;                      // one attention wave's V chunk image
constexpr int kArLdsBias = 0, kArLdsV = 2 * kRelBiasBuf * 4, kArLdsQC = kArLdsV + kRelH * kArVImg,
              kArLdsW = kArLdsQC + kRelTileQ * kRelQC * 4, kArLdsU = kArLdsW + kRelWBytes,
              kArLdsBytes = kArLdsU + kRelUBytes;               // 150.5 KiB

// kLse (training forward): also write the row's log-sum-exp in the log2 domain, lse2[(b * 8 + head) * N + q] = log2(sum_key exp2(z))
// (-inf for a fully masked row) -- what csrc/attn_rel_bwd.hip differentiates from.  Same out bits either way.
template <bool kLse = false>
__global__ __launch_bounds__(kRelWaves *kWave) void relation_attention_boxes_kernel(
    const uint16_t *__restrict__ q, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v, int ldq, int ldk, int ldv,
    const float *__restrict__ src, const float *__restrict__ tgt,
    const float *__restrict__ Wp, const float *__restrict__ bp, const unsigned char *__restrict__ mask, int N, int M,
    float scale_log2e, float eps, RelFreq fr, uint16_t *__restrict__ out, int ldo, int dbg_arg, float *__restrict__ lse2)
{
#ifdef RDETR_DEV
    const int dbg = dbg_arg;                 // development builds: component-timing mask (tools/attn_rel_components.py)
#else
    constexpr int dbg = 0;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char ar_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, q0 = blockIdx.x * kRelTileQ;
    float *bias_lds = reinterpret_cast<float *>(ar_lds + kArLdsBias);
    float *qc = reinterpret_cast<float *>(ar_lds + kArLdsQC);
    u32x4 *wfr = reinterpret_cast<u32x4 *>(ar_lds + kArLdsW);
    u32x4 *ufr = reinterpret_cast<u32x4 *>(ar_lds + kArLdsU);

    // ---- prologue (csrc/relation_gen.h): W fragments, per-query constants and size-ratio coefficients U, all in the log2 domain ----
    build_w_fragments(tid, Wp, wfr);
    build_query_tile(tid, b, q0, N, src, Wp, eps, fr, qc, ufr);
    __syncthreads();

    // ---- roles ----
    const bool att = wave < kRelH;
    const int kbw = (wave & 7) >> 1;                  // feature waves: the 16-key block of a chunk this wave computes features for
    const int qbase = (wave & 1) * 8;                 // ... for these 8 queries of the tile
    const float bph = (bp && ql < kRelH) ? bp[ql] * kLog2e : 0.f;
    const int nch = (M + kRelChunk - 1) / kRelChunk;

    // this lane's key of a chunk (fetched one chunk ahead)
    auto load_key = [&](int chunk) {
        const int key = chunk * kRelChunk + 16 * kbw + ql < M ? chunk * kRelChunk + 16 * kbw + ql : M - 1;
        return *reinterpret_cast<const f32x4 *>(tgt + ((size_t)b * M + key) * 4);
    };
    auto pair_sets = [&](auto nps_c, int buf, const f32x4 &kbox) {
        constexpr int NPS = decltype(nps_c)::value;
        float *dst = bias_lds + buf * kRelBiasBuf + ql * kRelHeadStride + 16 * kbw + 4 * g;
        const RelKey ks = key_side(kbox, g, eps, fr);                               // once per chunk
#pragma unroll 1
        for (int i0 = 0; i0 < NPS; i0 += 4)
#pragma unroll
        for (int i1 = 0; i1 < 4; ++i1)                                              // four independent chains in flight
            (void)pair_set(qbase + i0 + i1, lane, g, ks, qc, wfr, ufr, bph, fr, dst);
    };
    auto features = [&](int buf, const f32x4 &kbox) { pair_sets(std::integral_constant<int, 8>{}, buf, kbox); };

    // ---- pipeline: the feature waves produce the bias tile of chunk c + 1 while the heads consume chunk c.  Two loops with the
    //      same number of workgroup barriers (the branch is wave-uniform): a wave's registers hold only its own role's state ----
    if (!att) {
        f32x4 kc = load_key(0);
        features(0, kc);
        if (nch > 1) kc = load_key(1);
        __syncthreads();
        for (int c = 0; c < nch; ++c) {
            if (c + 1 < nch && !(dbg & 1)) features((c + 1) & 1, kc);
            if (c + 2 < nch) kc = load_key(c + 2);              // in flight across the barrier
            __syncthreads();
        }
        return;
    }

    // ---- attention state (waves 0-7: head = wave) ----
    const int h = wave;
    const int qi = q0 + ql;
    const bool qok = qi < N;
    const int qcl = qok ? qi : N - 1;
    unsigned char *lds_v = ar_lds + kArLdsV + wave * kArVImg;
    const uint16_t *kbase = k + (size_t)b * M * ldk + h * kRelD;
    const uint16_t *vbase = v + (size_t)b * M * ldv + h * kRelD;
    const unsigned char *mask_row = mask ? mask + (size_t)qcl * M : nullptr;
    u32x4 qfrag = {0, 0, 0, 0}, kf[4], vr[4];
    float m_run = -__builtin_inff(), l_run = 0.f;
    f32x4 oacc[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};

    // K / V rows through buffer loads: one per-lane offset for all chunks, the chunk's position in the scalar offset, and rows past
    // the last key come back as zeros from the descriptor's range check (no address arithmetic or bounds tests in the loop)
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(kbase), 0,
                                                                         (unsigned)((M - 1) * ldk + kRelD) * 2u, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(vbase), 0,
                                                                         (unsigned)((M - 1) * ldv + kRelD) * 2u, 0x00020000);
    const unsigned kvo = (unsigned)(ql * ldk + g * 8) * 2u, vvo = (unsigned)((lane >> 2) * ldv + (lane & 3) * 8) * 2u;
    auto load_k = [&](int key0) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
            kf[kb] = __builtin_amdgcn_raw_buffer_load_b128(krs, kvo, (unsigned)((key0 + 16 * kb) * ldk) * 2u, 0);
    };
    auto load_v = [&](int key0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            vr[i] = __builtin_amdgcn_raw_buffer_load_b128(vrs, vvo, (unsigned)((key0 + 16 * i) * ldv) * 2u, 0);
    };
    auto store_v = [&] {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            *reinterpret_cast<u32x4 *>(lds_v + (idx >> 2) * kArVS + (idx & 3) * 16) = vr[i];
        }
    };

    auto attention = [&](int c, int buf) {
        const int key0 = c * kRelChunk;
        const bool more = c + 1 < nch;
        if (more) load_v(key0 + kRelChunk);
        const float *brow = bias_lds + buf * kRelBiasBuf + h * kRelHeadStride + ql * kRelQStride + 4 * g;
        f32x4 s[4];
        float m_loc = -__builtin_inff();
        const bool edge = mask_row != nullptr || key0 + kRelChunk > M;              // wave-uniform: masks and the key tail are rare
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(kf[kb]), as_bf16x8(qfrag), z, 0, 0, 0);
            f32x4 t = *reinterpret_cast<const f32x4 *>(brow + 16 * kb);             // already in the log2 domain
            if (edge) mask_keys(t, key0 + 16 * kb + 4 * g, M, mask_row);
            z.x = __builtin_fmaf(z.x, scale_log2e, t.x);
            z.y = __builtin_fmaf(z.y, scale_log2e, t.y);
            z.z = __builtin_fmaf(z.z, scale_log2e, t.z);
            z.w = __builtin_fmaf(z.w, scale_log2e, t.w);
            s[kb] = z;
            m_loc = fmaxf(m_loc, fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w)));
        }
        if (more) load_k(key0 + kRelChunk);                      // the S^T products have consumed this chunk's fragments
        m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 16, 64));
        m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 32, 64));
        const float m_new = fmaxf(m_run, m_loc);
        const float m_safe = (m_new == -__builtin_inff()) ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);
        m_run = m_new;
        u32x4 pf[2];
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
            float p[8];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const f32x4 z = s[2 * pair + half];
                p[4 * half + 0] = __builtin_amdgcn_exp2f(z.x - m_safe);
                p[4 * half + 1] = __builtin_amdgcn_exp2f(z.y - m_safe);
                p[4 * half + 2] = __builtin_amdgcn_exp2f(z.z - m_safe);
                p[4 * half + 3] = __builtin_amdgcn_exp2f(z.w - m_safe);
            }
            pf[pair] = u32x4{pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(p[4], p[5]), pack_bf16x2(p[6], p[7])};
        }
        // the row sums of P (as rounded for the PV product) on the matrix core: ones . P^T -> every accumulator row holds the sum
        {
            const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
            f32x4 ls = {0.f, 0.f, 0.f, 0.f};
            ls = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ones), as_bf16x8(pf[0]), ls, 0, 0, 0);
            ls = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ones), as_bf16x8(pf[1]), ls, 0, 0, 0);
            l_run = __builtin_fmaf(l_run, alpha, ls.x);
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            oacc[cb].x *= alpha; oacc[cb].y *= alpha; oacc[cb].z *= alpha; oacc[cb].w *= alpha;
        }
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const u32x4 vf = tr_rows8<kArVS>(lds_v, 32 * pair, cb, lane);
                oacc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(vf), as_bf16x8(pf[pair]), oacc[cb], 0, 0, 0);
            }
        }
        wave_sync();                                            // this wave is done with its V image
        if (more) store_v();
        wave_sync();
    };

    qfrag = *reinterpret_cast<const u32x4 *>(q + ((size_t)b * N + qcl) * ldq + h * kRelD + g * 8);
    load_k(0);
    load_v(0);
    store_v();
    wave_sync();
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (!(dbg & 2)) attention(c, c & 1);
        __syncthreads();
    }

    if (qok) {
        const float inv = 1.0f / l_run;                            // 0 / 0 = NaN for a fully masked row, as torch.softmax
        uint16_t *o = out + ((size_t)b * N + qi) * ldo + h * kRelD + 4 * g;
        *reinterpret_cast<u32x2 *>(o) = u32x2{pack_bf16x2(oacc[0].x * inv, oacc[0].y * inv), pack_bf16x2(oacc[0].z * inv, oacc[0].w * inv)};
        *reinterpret_cast<u32x2 *>(o + 16) = u32x2{pack_bf16x2(oacc[1].x * inv, oacc[1].y * inv), pack_bf16x2(oacc[1].z * inv, oacc[1].w * inv)};
        if constexpr (kLse) {
            if (g == 0) lse2[((size_t)b * kRelH + h) * N + qi] = m_run + log2f(l_run);     // l = 0: -inf, like m_run of a fully masked row
        }
    }
}

}  // namespace rdetr

#ifdef RDETR_DEV
// development builds only (make dev): 1 = feature waves idle, 2 = attention waves idle (WRONG results, component timing)
static int g_ar_dbg = 0;
extern "C" void rdetr_dev_set_attn_rel_dbg(int v) { g_ar_dbg = v; }
#define RDETR_AR_DBG g_ar_dbg
#else
#define RDETR_AR_DBG 0
#endif

// Launch of the kernel above for the inference (kLse = false) and training (kLse = true) entry points
template <bool kLse>
static int launch_relation_attention_boxes(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                           const float *src_boxes, const float *tgt_boxes, const float *proj_weight,
                                           const float *proj_bias, const uint8_t *bool_mask, int B, int H, int D, int N, int M, int F,
                                           float rel_scale, float temperature, float eps, float attn_scale, uint16_t *out, int ldo,
                                           float *lse, void *stream)
{
    using namespace rdetr;
    if (B < 0 || H <= 0 || N < 0 || M < 0 || F <= 0) return RDETR_ERR_INVALID_ARG;
    if (kLse) {                                     // the training entries take no empty problem and check the row strides
        const long long span = (long long)H * D;
        if (B == 0 || N == 0 || M == 0 || D <= 0 || ldq < span || ldk < span || ldv < span || ldo < span) return RDETR_ERR_INVALID_ARG;
    }
    if (D != kRelD || H != kRelH || F != kRelF) return RDETR_ERR_UNSUPPORTED;
    if (B == 0 || N == 0) return RDETR_OK;
    if (M == 0) return RDETR_ERR_INVALID_ARG;
    if (!q || !k || !v || !out || !src_boxes || !tgt_boxes || !proj_weight || (kLse && !lse)) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(q, 16) || !aligned_to(k, 16) || !aligned_to(v, 16) || !aligned_to(out, 8) || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4 ||
        !aligned_to(src_boxes, 16) || !aligned_to(tgt_boxes, 16) || (kLse && !aligned_to(lse, 4)))
        return RDETR_ERR_UNSUPPORTED;
    if (B > 65535 || (long long)M * (ldk > ldv ? ldk : ldv) * 2 >= (1ll << 31)) return RDETR_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RelFreq fr = rel_freq(F, rel_scale, temperature);
    if (const int s = ensure_dynamic_lds<relation_attention_boxes_kernel<kLse>>(kArLdsBytes)) return s;
    hipLaunchKernelGGL(relation_attention_boxes_kernel<kLse>, dim3((unsigned)((N + kRelTileQ - 1) / kRelTileQ), (unsigned)B),
                       dim3(kRelWaves * kWave), kArLdsBytes, st, q, k, v, ldq, ldk, ldv, src_boxes, tgt_boxes,
                       proj_weight, proj_bias, bool_mask, N, M, attn_scale * kLog2e, eps, fr, out, ldo, RDETR_AR_DBG, lse);
    return launch_status();
}

extern "C" int rdetr_relation_attention_boxes_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                                   const float *src_boxes, const float *tgt_boxes, const float *proj_weight,
                                                   const float *proj_bias, const uint8_t *bool_mask, int B, int H,
                                                   int D, int N, int M, int F, float rel_scale, float temperature, float eps,
                                                   float attn_scale, uint16_t *out, int ldo, void *stream)
{
    return launch_relation_attention_boxes<false>(q, k, v, ldq, ldk, ldv, src_boxes, tgt_boxes, proj_weight, proj_bias, bool_mask, B, H, D,
                                                  N, M, F, rel_scale, temperature, eps, attn_scale, out, ldo, nullptr, stream);
}

extern "C" int rdetr_relation_attention_boxes_train_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk,
                                                         int ldv, const float *src_boxes, const float *tgt_boxes,
                                                         const float *proj_weight, const float *proj_bias, const uint8_t *bool_mask,
                                                         int B, int H, int D, int N, int M, int F, float rel_scale, float temperature,
                                                         float eps, float attn_scale, uint16_t *out, int ldo, float *lse, void *stream)
{
    return launch_relation_attention_boxes<true>(q, k, v, ldq, ldk, ldv, src_boxes, tgt_boxes, proj_weight, proj_bias, bool_mask, B, H, D,
                                                 N, M, F, rel_scale, temperature, eps, attn_scale, out, ldo, lse, stream);
}
