// Backward of the fused decoder self-attention (csrc/attn.hip) for bf16 training, FlashAttention-2 shaped (gfx950).
//
// Differentiates out = softmax(X) V with X = Q K^T * scale + bias (bias fp32 [B*H, N, M] or none, bool mask [N, M] or none),
// from the forward's per-row log-sum-exp (log2 domain, written by relation_attention_kernel<S, true>) instead of a saved
// [B*H, N, M] probability tensor:
//   P = exp2(S * scale * log2e + bias * log2e - lse2)     the forward's own arithmetic for the exponent, in fp32
//   dP = dO V^T,  Di = rowsum(dO o O),  dS = P o (dP - Di)  (= dX = dbias),  dV = P^T dO,  dK = scale dS^T Q,  dQ = scale dS K
// Three launches, no float atomics (every output element is written by exactly one lane, sums run in a fixed order, so the
// same inputs give the same bits on every run):
//   di   : Di per (image, head, query), fp32 workspace [B*H, N]
//   dkv  : grid = (ceil(M / 64) key tiles, B * H), 4 waves of 16 keys each.  The workgroup sweeps all queries in chunks of 64
//          (Q, dO, lse2, Di staged once per chunk in LDS for its 4 waves) and keeps dK^T, dV^T of its keys in fp32 registers;
//          with a dbias pointer it also writes dS (each element once).
//   dq   : grid = (ceil(N / 64) query tiles, B * H), 4 waves of 16 queries each, sweeping all keys in chunks of 64 (K, V staged);
//          recomputes dS the same way (or, in a development build, reads it back from dbias).
// MFMA = v_mfma_f32_16x16x32_bf16, head dim 32 = one K step, with the lane layout of the forward kernel (csrc/attn.hip):
//   dkv  "key on the lane":  S[q][key] = Q[q][:] . K[key][:]   A = Q rows (ds_read_b128), B = K rows of the wave's keys (registers)
//                            dP[q][key] = dO[q][:] . V[key][:]  A = dO rows, B = V rows
//          -> lane (key = lane & 15, g = lane >> 4) holds queries 16 qb + 4 g + r of ITS key: the lane's P / dS values are already
//          the B operand of  dV^T[d][key] += sum_q dO^T[d][q] P[q][key]  and  dK^T[d][key] += sum_q Q^T[d][q] dS[q][key], whose A
//          operands come from ds_read_b64_tr_b16 of the row-major Q / dO images with the forward's key permutation
//          k = 8 g + j  <->  query 32 pair + 16 (j >> 2) + 4 g + (j & 3).
//   dq   the forward's transposed products: S^T[key][q] (A = K rows, B = Q of the lane's query), dP^T[key][q] (A = V rows,
//          B = dO of the lane's query) -> dQ^T[d][q] += K^T[d][key] dS^T[key][q] with K^T through the transposed read.
// dS is rounded to bf16 as an MFMA operand (P for dV too), accumulation in fp32.  LDS images: stride 80 B for the ds_read_b128 row
// reads, 96 B for the transposed reads (conflict-free, as in the forward), one copy of each tile per kind of read.
// Masking: -inf bias entries, bool-masked keys and keys past M give P = 0 and dS = 0; a fully masked row (lse2 = -inf) is
// treated as P = 0 for all of its keys, so its gradients stay inside its own (image, head).
// The mask rule, the transposed read and bwd_lse are csrc/attn_common.h's; the Di kernel here also serves csrc/attn_rel_bwd.hip
// (launch_attention_bwd_di), as does the entry point's stride / alignment check (attention_bwd_layout_status).
#include <cstdlib>

#include "attn_common.h"

namespace rdetr {

constexpr int kBwD = 32;                 // head dim
constexpr int kBwTile = 64;              // keys per dkv workgroup, queries per dq workgroup, rows of a staged chunk
constexpr int kBwRS = 80, kBwTS = 96;    // LDS row strides in bytes: row reads (ds_read_b128), transposed reads (ds_read_b64_tr_b16)

// Di = rowsum(dO o O) per (image, head, query): one thread per (b, q, h), fixed order over the 32 columns
__global__ __launch_bounds__(256) void relation_attention_bwd_di_kernel(const uint16_t *__restrict__ out, int ldo,
                                                                        const uint16_t *__restrict__ dout, int lddo, int H, int N,
                                                                        long long total, float *__restrict__ di)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int h = (int)(idx % H);
    const long long bq = idx / H;                            // b * N + q
    const long long b = bq / N, qi = bq - b * N;
    const u32x2 *o = reinterpret_cast<const u32x2 *>(out + bq * ldo + h * kBwD);
    const u32x2 *d = reinterpret_cast<const u32x2 *>(dout + bq * lddo + h * kBwD);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kBwD / 4; ++i) {
        const u32x2 a = o[i], c = d[i];
        s += bf16_bits_to_f32(a.x & 0xffffu) * bf16_bits_to_f32(c.x & 0xffffu);
        s += bf16_bits_to_f32(a.x >> 16) * bf16_bits_to_f32(c.x >> 16);
        s += bf16_bits_to_f32(a.y & 0xffffu) * bf16_bits_to_f32(c.y & 0xffffu);
        s += bf16_bits_to_f32(a.y >> 16) * bf16_bits_to_f32(c.y >> 16);
    }
    di[(b * H + h) * N + qi] = s;
}

void launch_attention_bwd_di(const uint16_t *out, int ldo, const uint16_t *dout, int lddo, int B, int H, int N, float *di,
                             hipStream_t stream)
{
    const long long rows = (long long)B * H * N;
    hipLaunchKernelGGL(relation_attention_bwd_di_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, out, ldo, dout,
                       lddo, H, N, rows, di);
}

// dK, dV (and dbias = dS) of 64 keys of one (image, head); see the header comment
template <bool kDbias>
__global__ __launch_bounds__(256) void relation_attention_bwd_dkv_kernel(
    const uint16_t *__restrict__ q, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v, int ldq, int ldk, int ldv,
    const uint16_t *__restrict__ dout, int lddo, const float *__restrict__ lse2, const float *__restrict__ di,
    const float *__restrict__ bias, const unsigned char *__restrict__ mask, int H, int N, int M, float scale_log2e, float scale,
    uint16_t *__restrict__ dk, int lddk, uint16_t *__restrict__ dv, int lddv, float *__restrict__ dbias)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kBwTile * (2 * kBwRS + 2 * kBwTS) + 2 * kBwTile * 4];
    unsigned char *qa = lds, *da = qa + kBwTile * kBwRS, *qt = da + kBwTile * kBwRS, *dt = qt + kBwTile * kBwTS;
    float *lse_s = reinterpret_cast<float *>(dt + kBwTile * kBwTS), *di_s = lse_s + kBwTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kl = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int key = blockIdx.x * kBwTile + 16 * wave + kl;
    const bool kok = key < M;
    const int kc = kok ? key : M - 1;

    // B operands of S and dP: rows of the lane's key, d = 8 g + j
    const u32x4 kfrag = *reinterpret_cast<const u32x4 *>(k + ((size_t)b * M + kc) * ldk + h * kBwD + g * 8);
    const u32x4 vfrag = *reinterpret_cast<const u32x4 *>(v + ((size_t)b * M + kc) * ldv + h * kBwD + g * 8);

    // staging of one chunk of 64 queries: thread -> (row = tid >> 2, 16-byte piece = tid & 3); threads 0..63 also take lse2 / Di
    const int srow = tid >> 2, spiece = tid & 3;
    const uint16_t *qbase = q + (size_t)b * N * ldq + h * kBwD + spiece * 8;
    const uint16_t *dbase = dout + (size_t)b * N * lddo + h * kBwD + spiece * 8;
    const float *lse_row = lse2 + (size_t)bh * N, *di_row = di + (size_t)bh * N;
    u32x4 qr, dr;
    float lr = 0.f, dir = 0.f;
    auto load_chunk = [&](int c0) {
        const int qq = c0 + srow;
        if (qq < N) {
            qr = *reinterpret_cast<const u32x4 *>(qbase + (size_t)qq * ldq);
            dr = *reinterpret_cast<const u32x4 *>(dbase + (size_t)qq * lddo);
        } else {
            qr = u32x4{0, 0, 0, 0};
            dr = u32x4{0, 0, 0, 0};
        }
        if (tid < kBwTile) {
            const int qx = c0 + tid;
            lr = qx < N ? bwd_lse(lse_row[qx]) : __builtin_inff();     // queries past N: P = 0
            dir = qx < N ? di_row[qx] : 0.f;
        }
    };
    auto store_chunk = [&] {
        *reinterpret_cast<u32x4 *>(qa + srow * kBwRS + spiece * 16) = qr;
        *reinterpret_cast<u32x4 *>(qt + srow * kBwTS + spiece * 16) = qr;
        *reinterpret_cast<u32x4 *>(da + srow * kBwRS + spiece * 16) = dr;
        *reinterpret_cast<u32x4 *>(dt + srow * kBwTS + spiece * 16) = dr;
        if (tid < kBwTile) {
            lse_s[tid] = lr;
            di_s[tid] = dir;
        }
    };
    // bias / mask of the lane's 16 (query, key) pairs of a chunk: queries c0 + 16 qb + 4 g + r, its key (forward's rules)
    const float *bias_col = bias ? bias + (size_t)bh * N * M + kc : nullptr;
    const unsigned char *mask_col = mask ? mask + kc : nullptr;
    auto load_bias = [&](int c0, float (&bz)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int qq = c0 + 16 * (i >> 2) + 4 * g + (i & 3);
            float t = 0.f;
            if (qq < N) {
                if (bias_col) t = bias_col[(size_t)qq * M];
                if (mask_col && mask_col[(size_t)qq * M]) t = -__builtin_inff();
            }
            if (!kok) t = -__builtin_inff();
            bz[i] = t;
        }
    };

    f32x4 acc_dk[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}}, acc_dv[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};   // [d][key]
    const int nchunks = (N + kBwTile - 1) / kBwTile;
    float bcur[16], bnext[16];
    load_chunk(0);
    load_bias(0, bcur);
    for (int c = 0; c < nchunks; ++c) {
        const int c0 = c * kBwTile;
        __syncthreads();                                     // every wave is done with the previous chunk's images
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunks) {
            load_chunk(c0 + kBwTile);
            load_bias(c0 + kBwTile, bnext);
        }
        float pdv[16], dsv[16];
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            const u32x4 aq = *reinterpret_cast<const u32x4 *>(qa + (16 * qb + kl) * kBwRS + g * 16);
            const u32x4 ad = *reinterpret_cast<const u32x4 *>(da + (16 * qb + kl) * kBwRS + g * 16);
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(aq), as_bf16x8(kfrag), s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ad), as_bf16x8(vfrag), dp, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = 16 * qb + 4 * g + r, i = 4 * qb + r;
                const float z = s[r] * scale_log2e + bcur[i] * kLog2e;
                const float p = __builtin_amdgcn_exp2f(z - lse_s[ql]);
                const float ds = p == 0.f ? 0.f : p * (dp[r] - di_s[ql]);
                pdv[i] = p;
                dsv[i] = ds;
                if constexpr (kDbias) {
                    const int qq = c0 + ql;
                    if (kok && qq < N) dbias[((size_t)bh * N + qq) * M + key] = ds;
                }
            }
        }
        // B operands [k = 8 g + j][key]: j = 4 half + r <-> query 32 pair + 16 half + 4 g + r
        u32x4 pf[2], sf[2];
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
            const int i0 = 8 * pair;
            pf[pair] = u32x4{pack_bf16x2(pdv[i0 + 0], pdv[i0 + 1]), pack_bf16x2(pdv[i0 + 2], pdv[i0 + 3]), pack_bf16x2(pdv[i0 + 4], pdv[i0 + 5]),
                             pack_bf16x2(pdv[i0 + 6], pdv[i0 + 7])};
            sf[pair] = u32x4{pack_bf16x2(dsv[i0 + 0], dsv[i0 + 1]), pack_bf16x2(dsv[i0 + 2], dsv[i0 + 3]),
                             pack_bf16x2(dsv[i0 + 4], dsv[i0 + 5]), pack_bf16x2(dsv[i0 + 6], dsv[i0 + 7])};
        }
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const u32x4 tdo = tr_rows8<kBwTS>(dt, 32 * pair, cb, lane);
                acc_dv[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(tdo), as_bf16x8(pf[pair]), acc_dv[cb], 0, 0, 0);
                const u32x4 tq = tr_rows8<kBwTS>(qt, 32 * pair, cb, lane);
                acc_dk[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(tq), as_bf16x8(sf[pair]), acc_dk[cb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) bcur[i] = bnext[i];
    }
    if (kok) {                                               // lane (key, g) holds d = 16 cb + 4 g + r of its key
        uint16_t *pk = dk + ((size_t)b * M + key) * lddk + h * kBwD + 4 * g;
        uint16_t *pv = dv + ((size_t)b * M + key) * lddv + h * kBwD + 4 * g;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const f32x4 a = acc_dk[cb], c = acc_dv[cb];
            *reinterpret_cast<u32x2 *>(pk + 16 * cb) = u32x2{pack_bf16x2(a.x * scale, a.y * scale), pack_bf16x2(a.z * scale, a.w * scale)};
            *reinterpret_cast<u32x2 *>(pv + 16 * cb) = u32x2{pack_bf16x2(c.x, c.y), pack_bf16x2(c.z, c.w)};
        }
    }
}

// dQ of 64 queries of one (image, head); kReadDs: dS read back from dbias (written by the dkv kernel) instead of recomputed
template <bool kReadDs>
__global__ __launch_bounds__(256) void relation_attention_bwd_dq_kernel(
    const uint16_t *__restrict__ q, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v, int ldq, int ldk, int ldv,
    const uint16_t *__restrict__ dout, int lddo, const float *__restrict__ lse2, const float *__restrict__ di,
    const float *__restrict__ bias, const unsigned char *__restrict__ mask, const float *__restrict__ ds_in, int H, int N, int M,
    float scale_log2e, float scale, uint16_t *__restrict__ dq, int lddq)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kBwTile * (2 * kBwRS + kBwTS)];
    unsigned char *ka = lds, *va = ka + kBwTile * kBwRS, *kt = va + kBwTile * kBwRS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int qi = blockIdx.x * kBwTile + 16 * wave + ql;
    const bool qok = qi < N;
    const int qc = qok ? qi : N - 1;

    // B operands of S^T and dP^T: the lane's query row of Q / dO, d = 8 g + j
    const u32x4 qfrag = *reinterpret_cast<const u32x4 *>(q + ((size_t)b * N + qc) * ldq + h * kBwD + g * 8);
    const u32x4 dofrag = *reinterpret_cast<const u32x4 *>(dout + ((size_t)b * N + qc) * lddo + h * kBwD + g * 8);
    const float l2 = qok ? bwd_lse(lse2[(size_t)bh * N + qc]) : __builtin_inff();
    const float dd = di[(size_t)bh * N + qc];

    const int srow = tid >> 2, spiece = tid & 3;
    const uint16_t *kbase = k + (size_t)b * M * ldk + h * kBwD + spiece * 8;
    const uint16_t *vbase = v + (size_t)b * M * ldv + h * kBwD + spiece * 8;
    u32x4 kr, vr;
    auto load_chunk = [&](int key0) {
        const int key = key0 + srow;
        if (key < M) {
            kr = *reinterpret_cast<const u32x4 *>(kbase + (size_t)key * ldk);
            if constexpr (!kReadDs) vr = *reinterpret_cast<const u32x4 *>(vbase + (size_t)key * ldv);
        } else {
            kr = u32x4{0, 0, 0, 0};
            vr = u32x4{0, 0, 0, 0};
        }
    };
    auto store_chunk = [&] {
        *reinterpret_cast<u32x4 *>(kt + srow * kBwTS + spiece * 16) = kr;
        if constexpr (!kReadDs) {
            *reinterpret_cast<u32x4 *>(ka + srow * kBwRS + spiece * 16) = kr;
            *reinterpret_cast<u32x4 *>(va + srow * kBwRS + spiece * 16) = vr;
        }
    };
    // bias / mask (or dS) of the lane's 16 (query, key) pairs of a chunk: keys key0 + 16 kb + 4 g + r of its query (forward's rules)
    const float *row = (kReadDs ? ds_in : bias) ? (kReadDs ? ds_in : bias) + ((size_t)bh * N + qc) * M : nullptr;
    const unsigned char *mask_row = mask ? mask + (size_t)qc * M : nullptr;
    const bool vec_row = (M % 4 == 0) && (reinterpret_cast<uintptr_t>(row) % 16 == 0);
    auto load_bias = [&](int key0, f32x4 (&bz)[4]) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int kk = key0 + 16 * kb + 4 * g;
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            if (row) {
                if (vec_row) {
                    if (kk < M) t = *reinterpret_cast<const f32x4 *>(row + kk);
                } else {
                    t.x = kk + 0 < M ? row[kk + 0] : 0.f;
                    t.y = kk + 1 < M ? row[kk + 1] : 0.f;
                    t.z = kk + 2 < M ? row[kk + 2] : 0.f;
                    t.w = kk + 3 < M ? row[kk + 3] : 0.f;
                }
            }
            if constexpr (kReadDs) {
                if (!qok) t = f32x4{0.f, 0.f, 0.f, 0.f};        // dS read back: keys past M are 0 already
            } else {
                mask_keys(t, kk, M, mask_row);
            }
            bz[kb] = t;
        }
    };

    f32x4 acc[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};   // dQ^T[d = 16 cb + 4 g + r][q]
    const int nchunks = (M + kBwTile - 1) / kBwTile;
    f32x4 bcur[4], bnext[4];
    load_chunk(0);
    load_bias(0, bcur);
    for (int c = 0; c < nchunks; ++c) {
        const int key0 = c * kBwTile;
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunks) {
            load_chunk(key0 + kBwTile);
            load_bias(key0 + kBwTile, bnext);
        }
        f32x4 dsv[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            if constexpr (kReadDs) {
                dsv[kb] = bcur[kb];
            } else {
                const u32x4 kf = *reinterpret_cast<const u32x4 *>(ka + (16 * kb + ql) * kBwRS + g * 16);
                const u32x4 vf = *reinterpret_cast<const u32x4 *>(va + (16 * kb + ql) * kBwRS + g * 16);
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(kf), as_bf16x8(qfrag), s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(vf), as_bf16x8(dofrag), dp, 0, 0, 0);
                f32x4 t;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = s[r] * scale_log2e + bcur[kb][r] * kLog2e;
                    const float p = __builtin_amdgcn_exp2f(z - l2);
                    t[r] = p == 0.f ? 0.f : p * (dp[r] - dd);
                }
                dsv[kb] = t;
            }
        }
        u32x4 sf[2];
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
            const f32x4 a = dsv[2 * pair], c2 = dsv[2 * pair + 1];
            sf[pair] = u32x4{pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(c2.x, c2.y), pack_bf16x2(c2.z, c2.w)};
        }
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const u32x4 tk = tr_rows8<kBwTS>(kt, 32 * pair, cb, lane);
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(tk), as_bf16x8(sf[pair]), acc[cb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) bcur[kb] = bnext[kb];
    }
    if (qok) {
        uint16_t *o = dq + ((size_t)b * N + qi) * lddq + h * kBwD + 4 * g;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const f32x4 a = acc[cb];
            *reinterpret_cast<u32x2 *>(o + 16 * cb) = u32x2{pack_bf16x2(a.x * scale, a.y * scale), pack_bf16x2(a.z * scale, a.w * scale)};
        }
    }
}

}  // namespace rdetr

#ifdef RDETR_DEV
// development builds only (make dev): dQ kernel variant, 0 = the shipped choice, 1 = recompute dS, 2 = read dS back from dbias
static int g_bwd_dq_mode = 0;
extern "C" void rdetr_dev_set_attn_bwd_dq(int v) { g_bwd_dq_mode = v; }
#define RDETR_BWD_DQ_MODE g_bwd_dq_mode
#else
#define RDETR_BWD_DQ_MODE 0
#endif

extern "C" long long rdetr_relation_attention_backward_workspace_bytes(int B, int H, int N)
{
    if (B <= 0 || H <= 0 || N <= 0) return 0;
    return rdetr::attention_di_bytes(B, H, N);                // Di, fp32 [B*H, N]
}

extern "C" int rdetr_relation_attention_backward_bf16(
    const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv, const uint16_t *out, int ldo, const float *lse,
    const uint16_t *dout, int lddo, const float *bias, const uint8_t *bool_mask, int B, int H, int D, int N, int M, float scale,
    void *workspace, long long workspace_bytes, uint16_t *dq, int lddq, uint16_t *dk, int lddk, uint16_t *dv, int lddv, float *dbias,
    void *stream)
{
    using namespace rdetr;
    if (B <= 0 || H <= 0 || N <= 0 || M <= 0) return RDETR_ERR_INVALID_ARG;
    if (!q || !k || !v || !out || !lse || !dout || !workspace || !dq || !dk || !dv) return RDETR_ERR_INVALID_ARG;
    if (D != kBwD) return RDETR_ERR_UNSUPPORTED;
    const int lay = attention_bwd_layout_status(q, k, v, out, dout, lse, workspace, dq, dk, dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv,
                                                (long long)H * D, workspace_bytes,
                                                rdetr_relation_attention_backward_workspace_bytes(B, H, N));
    if (lay != RDETR_OK) return lay;
    if ((bias && !aligned_to(bias, 4)) || (dbias && !aligned_to(dbias, 4))) return RDETR_ERR_UNSUPPORTED;
    const long long bh = (long long)B * H;
    if (bh > 65535) return RDETR_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *di = static_cast<float *>(workspace);
    const float sl = scale * kLog2e;
    launch_attention_bwd_di(out, ldo, dout, lddo, B, H, N, di, st);
    const dim3 gk((unsigned)((M + kBwTile - 1) / kBwTile), (unsigned)bh), gq((unsigned)((N + kBwTile - 1) / kBwTile), (unsigned)bh);
    if (dbias)
        hipLaunchKernelGGL(relation_attention_bwd_dkv_kernel<true>, gk, dim3(256), 0, st, q, k, v, ldq, ldk, ldv, dout, lddo, lse, di, bias,
                           bool_mask, H, N, M, sl, scale, dk, lddk, dv, lddv, dbias);
    else
        hipLaunchKernelGGL(relation_attention_bwd_dkv_kernel<false>, gk, dim3(256), 0, st, q, k, v, ldq, ldk, ldv, dout, lddo, lse, di,
                           bias, bool_mask, H, N, M, sl, scale, dk, lddk, dv, lddv, nullptr);
    // dQ recomputes dS by default: reading dbias back moves the same bytes as the bias it replaces
    const bool read_ds = dbias && RDETR_BWD_DQ_MODE == 2;
    if (read_ds)
        hipLaunchKernelGGL(relation_attention_bwd_dq_kernel<true>, gq, dim3(256), 0, st, q, k, v, ldq, ldk, ldv, dout, lddo, lse, di,
                           nullptr, nullptr, dbias, H, N, M, sl, scale, dq, lddq);
    else
        hipLaunchKernelGGL(relation_attention_bwd_dq_kernel<false>, gq, dim3(256), 0, st, q, k, v, ldq, ldk, ldv, dout, lddo, lse, di,
                           bias, bool_mask, nullptr, H, N, M, sl, scale, dq, lddq);
    return launch_status();
}
