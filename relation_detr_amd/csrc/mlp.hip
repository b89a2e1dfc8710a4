// The decoder's box head as ONE kernel (bf16, embed_dim 256, gfx950):
//     delta = W3 relu(W2 relu(W1 x + b1) + b2) + b3                        MLP(256, 256, 4, 3)   models/bricks/basic.py:6-24
//     out   = sigmoid(delta + inverse_sigmoid(reference))                                        relation_transformer.py:363-381
// for the two inputs a decoder layer feeds it -- the normalised layer output (the layer's boxes) and the layer output itself (the
// next layer's reference points) -- i.e. six library GEMMs of 1,800 rows and two refine launches of the decoder's dependency chain
// (~8 us each whatever their size) in one launch.
//
//   workgroup  8 waves x (16 kMlpNB) rows of the concatenated row space: rows [0, M) are input A, [M, 2M) input B (source and
//              output pointer are chosen per row, so a block may straddle the seam).  The waves split the OUTPUT COLUMNS of the
//              hidden layers: wave w owns tile pair w (columns 32 w .. 32 w + 31) for all the workgroup's rows.
//   weights    W1, W2 packed in fragment order (rdetr_linear_pack_k256_bf16).  A fragment is needed by exactly one wave of the
//              workgroup and goes global -> registers -> MFMA (no LDS staging, no LDS-DMA, no barrier around it): both layers'
//              16 fragments per wave are requested at the top of the kernel, W2's land behind layer 1.
//   layers     with the output permutation of csrc/ffn.hip a lane (row, g) ends tile pair u holding outputs 32 u + 8 g .. + 7 of
//              its row, which -- biased, ReLU'd, rounded to bf16 as the unfused path stores them -- ARE the lane's B operand of
//              the next layer's k-step u: each wave writes its pair to an LDS image [row block][u][lane] (1-KiB rows,
//              conflict-free), one __syncthreads(), every wave reads all 8 k-steps.  One image per hidden layer, each written
//              once per launch, so nothing can be overwritten under a reader.
//   last layer W3 [4, 256] as one zero-padded tile of fragments built in registers by wave 0, which runs it over the 8 k-steps
//              of the second image; lanes g == 0 hold the row's 4 outputs, add the bias, round to bf16 (as the library GEMM
//              stores them), refine against the fp32 reference box and store fp32.
//   class head (box_head_cls_k256_kernel, rdetr_box_head_cls_k256_bf16) class_head[i](x) for the rows of input A, a 256 -> C library
//              GEMM of the decoder's chain, on the layer-1 operand the kernel already holds: the waves that own columns < C take
//              their 16 fragments of Wc (zero-padded to [256, 256], packed) into the registers W1 has left, run the block after
//              their layer-1 image is written, and add the bias, round to bf16 and store columns < C (2-byte stores: C = 91 rows
//              are 182 bytes) after the barrier.  The last layer's operands (W3, reference) are requested after the class block
//              instead of at the top, so that everything still fits 256 VGPRs.  Boxes are bit for bit the plain kernel's.
//   arithmetic every output accumulates the same v_mfma_f32_16x16x32_bf16 products in the same k-step order (s = 0 .. 7) with
//              the same rounding points as the row-split kernel this replaces: results are bit-identical to it.
//   history    the previous kernel gave every wave 32 rows and ALL 256 columns: 15 workgroups for 2 x 1,800 rows, both weights
//              through LDS-DMA into 128 KiB of LDS and read from there by all 8 waves; 22.7 us per call in the stack.
//   measured   (tools/time_box_head.py, graph replay, us per call; profiles/r09/time_chain_kernels.txt) two-stage call 1 x 1,800
//              rows 9.1; decoder layer 2 x 600 / 2 x 1,800 / 2 x 3,600 rows 10.0 / 10.1 / 10.4; the row-split kernel in the same
//              call 19.9 and 20.8 / 21.1 / 21.2; the unfused sequence 19.3 and 29.2 / 29.9 / 34.1.  In the step together with
//              csrc/qpos.hip: 3.90-3.95 -> 3.76-3.79 ms (ab_stack_chain_kernels.txt).
//              With the class head, C = 91 (profiles/r12/time_absorbed_kernels.txt, alternating, 5 runs each) 2 x 600 / 2 x 1,800 /
//              2 x 3,600 rows: 11.2 / 11.3 / 11.6 against this kernel followed by the library GEMM it absorbs 13.8 / 14.1 / 14.8.  In
//              the step (profiles/r12/decoder_chain_by_kernel.txt) 12.7 us against 11.8 + 5.8.
//   resources  (hipcc -Rpass-analysis=kernel-resource-usage) 224 VGPRs, no AGPRs, no scratch, no spills, 32 KiB static LDS (was
//              138 KiB dynamic), 2 waves per SIMD = one 8-wave workgroup per CU.
//              With the class head: 244 VGPRs, no AGPRs, no scratch, 32 KiB LDS, 2 waves per SIMD (with the last layer's operands
//              requested at the top as in the plain kernel: 256 VGPRs and 104 bytes of scratch per lane).
//   dropped    16 rows per workgroup (kMlpNB = 1, 180 VGPRs, 225 workgroups at 2 x 1,800 rows): 6.5 and 6.9 / 7.1 / 12.7 us
//              isolated -- faster while one launch has the chip to itself, slower than 32 rows once the workgroups outnumber
//              the CUs, which is the stack's situation (both image groups' launches coincide) -- and the step does not tell them
//              apart (1036-1063 vs 1055-1063 images/s, ab_candidates.txt); 32 rows moves half the weight bytes from L2.
#include "launch.h"

namespace rdetr {

typedef __bf16 mlp_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kMlpWaves = 8, kMlpThreads = kMlpWaves * 64;
constexpr int kMlpNB = 2, kMlpRows = 16 * kMlpNB;         // 16-row N blocks per workgroup (they share every A fragment): 113 workgroups at 2 x 1,800 rows
constexpr int kMlpImg = kMlpNB * 8 * 64;                  // one exchange image in u32x4: [row block][u][lane]

// the class head a decoder layer runs on input A (rdetr_box_head_cls_k256_bf16)
struct MlpCls {
    const uint16_t *pwc, *bias;                                               // [C, 256] zero-padded to [256, 256] and packed; bias [C]
    uint16_t *out;                                                            // [M, C], row stride ld
    long long ld;
    int C;
};

template <bool kCls>
__device__ __forceinline__ void box_head_k256_body(
    const uint16_t *__restrict__ xa, long long lda, const uint16_t *__restrict__ xb, long long ldb, const uint16_t *__restrict__ pw1,
    const uint16_t *__restrict__ b1, const uint16_t *__restrict__ pw2, const uint16_t *__restrict__ b2, const uint16_t *__restrict__ w3,
    const uint16_t *__restrict__ b3, const float *__restrict__ ref, int ref_is_logit, float eps, long long M,
    float *__restrict__ out_a, float *__restrict__ out_b, const MlpCls &cl)
{
    __shared__ __attribute__((aligned(16))) u32x4 img[2 * kMlpImg];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const long long total = xb ? 2 * M : M;
    const long long row0 = (long long)blockIdx.x * kMlpRows + col;

    u32x4 x[kMlpNB][8];                                                       // the layer's input: B operand, k-step s
#pragma unroll
    for (int cb = 0; cb < kMlpNB; ++cb) {
        // rows >= total read the last row instead (unconditional loads); a row of the MFMA's N dimension never reaches another
        // row's outputs, and they store nothing
        const long long r = row0 + 16 * cb < total ? row0 + 16 * cb : total - 1;
        const uint16_t *p = r < M ? xa + r * lda : xb + (r - M) * ldb;
#pragma unroll
        for (int s = 0; s < 8; ++s) x[cb][s] = *reinterpret_cast<const u32x4 *>(p + 32 * s + 8 * g);
    }
    // this wave's 16 fragments of a packed [256, 256] weight (tiles 2 w, 2 w + 1), in the order the MFMAs take them: k-step s, tile e
    struct Frags { u32x4 f[16]; };
    auto fetch = [&](const uint16_t *packed, Frags &w) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(packed) + (size_t)wave * 16 * 64 + lane;
#pragma unroll
        for (int i = 0; i < 16; ++i) w.f[i] = p[((i & 1) * 8 + (i >> 1)) * 64];
        __builtin_amdgcn_sched_barrier(0);                                    // the loads are issued HERE, not sunk to their MFMAs
    };
    Frags w1, w2;
    fetch(pw1, w1);
    fetch(pw2, w2);
    // the 8 bias values of the lane's outputs of pair `wave`, as bf16 pairs (2-byte loads: a bias needs no alignment)
    auto bias_of = [&](const uint16_t *bias) {
        const uint16_t *p = bias + 32 * wave + 8 * g;
        return u32x4{p[0] | (unsigned)p[1] << 16, p[2] | (unsigned)p[3] << 16, p[4] | (unsigned)p[5] << 16, p[6] | (unsigned)p[7] << 16};
    };
    const u32x4 bb1 = bias_of(b1), bb2 = bias_of(b2);
    // the last layer's operands, requested now so that they are there when wave 0 gets to it: W3 [4, 256] as one zero-padded tile,
    // fragment (k-step s, lane (m, kb)) = W3[m][32 s + 8 kb ..] for m < 4, zeros otherwise (m = col, kb = g); the reference boxes
    u32x4 w3f[8];
    f32x4 rf[kMlpNB];
    auto fetch_last = [&] {
        const uint16_t *w3row = w3 + (col < 4 ? col : 0) * 256 + 8 * g;
#pragma unroll
        for (int s = 0; s < 8; ++s) w3f[s] = *reinterpret_cast<const u32x4 *>(w3row + 32 * s);
#pragma unroll
        for (int cb = 0; cb < kMlpNB; ++cb) {
            const long long r = row0 + 16 * cb < total ? row0 + 16 * cb : total - 1;
            rf[cb] = *reinterpret_cast<const f32x4 *>(ref + (r < M ? r : r - M) * 4);
        }
    };
    if (!kCls) fetch_last();                                                  // kCls: after the class block, whose fragments need the registers
    const f32x4 bb3 = {bf16_bits_to_f32(b3[0]), bf16_bits_to_f32(b3[1]), bf16_bits_to_f32(b3[2]), bf16_bits_to_f32(b3[3])};
    __builtin_amdgcn_sched_barrier(0);

    auto mm = [&](const u32x4 &a, const u32x4 &bq, const f32x4 &c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mlp_bf16x8, a), __builtin_bit_cast(mlp_bf16x8, bq), c, 0, 0, 0);
    };
    // one hidden layer, this wave's tile pair: relu(W x + b) rounded to bf16 into the layer's exchange image
    auto hidden = [&](const Frags &w, const u32x4 &bb, const u32x4 (&xin)[kMlpNB][8], u32x4 *out, auto &&after_mfma) {
        f32x4 acc[2][kMlpNB];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int cb = 0; cb < kMlpNB; ++cb) acc[e][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int cb = 0; cb < kMlpNB; ++cb) acc[i & 1][cb] = mm(w.f[i], xin[cb][i >> 1], acc[i & 1][cb]);
        __builtin_amdgcn_sched_barrier(0);
        after_mfma();
        const f32x4 blo = {bf16_bits_to_f32(bb.x & 0xffffu), __builtin_bit_cast(float, bb.x & 0xffff0000u),
                           bf16_bits_to_f32(bb.y & 0xffffu), __builtin_bit_cast(float, bb.y & 0xffff0000u)};
        const f32x4 bhi = {bf16_bits_to_f32(bb.z & 0xffffu), __builtin_bit_cast(float, bb.z & 0xffff0000u),
                           bf16_bits_to_f32(bb.w & 0xffffu), __builtin_bit_cast(float, bb.w & 0xffff0000u)};
#pragma unroll
        for (int cb = 0; cb < kMlpNB; ++cb) {
            const f32x4 lo = acc[0][cb] + blo, hi = acc[1][cb] + bhi;
            out[(cb * 8 + wave) * 64 + lane] = u32x4{relu_bf16x2(pack_bf16x2(lo.x, lo.y)), relu_bf16x2(pack_bf16x2(lo.z, lo.w)),
                                                     relu_bf16x2(pack_bf16x2(hi.x, hi.y)), relu_bf16x2(pack_bf16x2(hi.z, hi.w))};
        }
    };
    auto gather = [&](const u32x4 *in, u32x4 (&y)[kMlpNB][8]) {
#pragma unroll
        for (int cb = 0; cb < kMlpNB; ++cb)
#pragma unroll
            for (int s = 0; s < 8; ++s) y[cb][s] = in[(cb * 8 + s) * 64 + lane];
    };

    u32x4 y[kMlpNB][8];
    // class head: logits = Wc x + bc for the rows of input A, columns 32 wave .. + 31 < C.  The waves that own such columns take
    // Wc's fragments into the registers W1 has just left, run the block on the layer-1 operand after layer 1's exchange image
    // is written, and store after the barrier (the other waves do not wait for the stores)
    const bool cls = kCls && 32 * wave < cl.C && (long long)blockIdx.x * kMlpRows < M;     // uniform per wave
    f32x4 cacc[2][kMlpNB];
    hidden(w1, bb1, x, img, [&] { if (cls) fetch(cl.pwc, w1); });
    if (cls) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int cb = 0; cb < kMlpNB; ++cb) cacc[e][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int cb = 0; cb < kMlpNB; ++cb) cacc[i & 1][cb] = mm(w1.f[i], x[cb][i >> 1], cacc[i & 1][cb]);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                                          // every wave's columns of hidden layer 1
    if (cls) {
        const int c0 = 32 * wave + 8 * g;                                     // the lane's 8 columns: tile 0 holds c0 .. + 3, tile 1 c0 + 4 .. + 7
        float bc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) bc[k] = c0 + k < cl.C ? bf16_bits_to_f32(cl.bias[c0 + k]) : 0.f;
#pragma unroll
        for (int cb = 0; cb < kMlpNB; ++cb) {
            const long long r = row0 + 16 * cb;
            if (r >= M) continue;
            const f32x4 lo = cacc[0][cb], hi = cacc[1][cb];
            const float o[8] = {lo.x + bc[0], lo.y + bc[1], lo.z + bc[2], lo.w + bc[3], hi.x + bc[4], hi.y + bc[5], hi.z + bc[6], hi.w + bc[7]};
            uint16_t *dst = cl.out + r * cl.ld + c0;                          // C = 91 rows are 182 bytes: 2-byte stores
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (c0 + k < cl.C) dst[k] = f32_to_bf16_bits(o[k]);
        }
    }
    if (kCls) {
        fetch_last();
        __builtin_amdgcn_sched_barrier(0);
    }
    gather(img, y);
    hidden(w2, bb2, y, img + kMlpImg, [] {});
    __syncthreads();                                                          // ... of hidden layer 2
    if (wave != 0) return;                                                    // no barrier below

    // last layer: one tile, k = the 256 hidden units; lane (row, g = 0) ends holding outputs 0 .. 3
    gather(img + kMlpImg, y);
    f32x4 d[kMlpNB];
#pragma unroll
    for (int cb = 0; cb < kMlpNB; ++cb) d[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const u32x4 a = col < 4 ? w3f[s] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int cb = 0; cb < kMlpNB; ++cb) d[cb] = mm(a, y[cb][s], d[cb]);
    }
    if (g == 0) {
        const f32x4 bb = bb3;
#pragma unroll
        for (int cb = 0; cb < kMlpNB; ++cb) {
            const long long r = row0 + 16 * cb;
            if (r >= total) continue;
            const long long q = r < M ? r : r - M;
            const float dl[4] = {d[cb].x + bb.x, d[cb].y + bb.y, d[cb].z + bb.z, d[cb].w + bb.w};
            const float rv[4] = {rf[cb].x, rf[cb].y, rf[cb].z, rf[cb].w};
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float lg = rv[k];                                             // the reference already in logit space ...
                if (!ref_is_logit) {                                          // ... or a box: inverse_sigmoid (util/misc.py:31-35)
                    float xx = fminf(fmaxf(rv[k], 0.f), 1.f);
                    if (rv[k] != rv[k]) xx = rv[k];
                    const float x1 = fmaxf(xx, eps), x2 = fmaxf(1.f - xx, eps);
                    lg = logf(x1 / x2);
                }
                const float z = bf16_bits_to_f32(f32_to_bf16_bits(dl[k])) + lg;   // delta as the bf16 the GEMM would store
                o[k] = 1.f / (1.f + expf(-z));
            }
            *reinterpret_cast<f32x4 *>((r < M ? out_a : out_b) + q * 4) = f32x4{o[0], o[1], o[2], o[3]};
        }
    }
}


__global__ __launch_bounds__(kMlpThreads) void box_head_k256_kernel(
    const uint16_t *__restrict__ xa, long long lda, const uint16_t *__restrict__ xb, long long ldb, const uint16_t *__restrict__ pw1,
    const uint16_t *__restrict__ b1, const uint16_t *__restrict__ pw2, const uint16_t *__restrict__ b2, const uint16_t *__restrict__ w3,
    const uint16_t *__restrict__ b3, const float *__restrict__ ref, int ref_is_logit, float eps, long long M,
    float *__restrict__ out_a, float *__restrict__ out_b)
{
    box_head_k256_body<false>(xa, lda, xb, ldb, pw1, b1, pw2, b2, w3, b3, ref, ref_is_logit, eps, M, out_a, out_b, MlpCls{});
}

__global__ __launch_bounds__(kMlpThreads) void box_head_cls_k256_kernel(
    const uint16_t *__restrict__ xa, long long lda, const uint16_t *__restrict__ xb, long long ldb, const uint16_t *__restrict__ pw1,
    const uint16_t *__restrict__ b1, const uint16_t *__restrict__ pw2, const uint16_t *__restrict__ b2, const uint16_t *__restrict__ w3,
    const uint16_t *__restrict__ b3, const float *__restrict__ ref, int ref_is_logit, float eps, long long M,
    float *__restrict__ out_a, float *__restrict__ out_b, MlpCls cl)
{
    box_head_k256_body<true>(xa, lda, xb, ldb, pw1, b1, pw2, b2, w3, b3, ref, ref_is_logit, eps, M, out_a, out_b, cl);
}

}  // namespace rdetr

using namespace rdetr;

// out_a [M, 4] (and out_b [M, 4] when xb is given) = sigmoid(MLP3(x) + inverse_sigmoid(reference [M, 4])): the decoder's box head
// and box refinement for one or two [M, 256] bf16 inputs (row strides lda / ldb in elements).  pw1 / pw2: the two [256, 256]
// hidden weights packed by rdetr_linear_pack_k256_bf16; w3 [4, 256], b1 / b2 [256], b3 [4] bf16; reference / outputs fp32.
// reference_is_logit != 0: `reference` is added as it is (the two-stage proposals, relation_transformer.py:89-90, come as logits).
extern "C" int rdetr_box_head_k256_bf16(const uint16_t *xa, long long lda, const uint16_t *xb, long long ldb, const uint16_t *pw1,
                                        const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2, const uint16_t *w3, const uint16_t *b3,
                                        const float *reference, int reference_is_logit, float eps, long long M, float *out_a, float *out_b,
                                        void *stream)
{
    if (M < 0) return RDETR_ERR_INVALID_ARG;
    if (const int s = xb ? rows_status({{xa, lda, 256, 2}, {xb, ldb, 256, 2}}) : rows_status({{xa, lda, 256, 2}})) return s;
    if (M == 0) return RDETR_OK;
    if (!xa || !pw1 || !b1 || !pw2 || !b2 || !w3 || !b3 || !reference || !out_a || (xb && !out_b)) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, pw1, pw2, w3, reference, out_a) || (xb && !aligned_to(out_b, 16))) return RDETR_ERR_UNSUPPORTED;
    const long long total = xb ? 2 * M : M, nblk = (total + kMlpRows - 1) / kMlpRows;
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(box_head_k256_kernel, dim3((unsigned)nblk), dim3(kMlpThreads), 0, static_cast<hipStream_t>(stream), xa,
                       lda, xb, ldb, pw1, b1, pw2, b2, w3, b3, reference, reference_is_logit, eps, M, out_a, out_b);
    return launch_status();
}

// rdetr_box_head_k256_bf16 plus the layer's class head on input A, in the same launch:
//     out_cls [M, C] = xa Wc^T + bc     (bf16, row stride ldc elements, any alignment)
// pwc: class_head.weight [C, 256] zero-padded to [256, 256] and packed by rdetr_linear_pack_k256_bf16; bc bf16 [C]; 1 <= C <= 256.
// out_a / out_b are bit for bit what rdetr_box_head_k256_bf16 writes.
extern "C" int rdetr_box_head_cls_k256_bf16(const uint16_t *xa, long long lda, const uint16_t *xb, long long ldb, const uint16_t *pw1,
                                            const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2, const uint16_t *w3, const uint16_t *b3,
                                            const float *reference, int reference_is_logit, float eps, const uint16_t *pwc, const uint16_t *bc,
                                            int C, long long M, float *out_a, float *out_b, uint16_t *out_cls, long long ldc, void *stream)
{
    if (M < 0 || C < 1 || ldc < C) return RDETR_ERR_INVALID_ARG;
    if (const int s = xb ? rows_status({{xa, lda, 256, 2}, {xb, ldb, 256, 2}}) : rows_status({{xa, lda, 256, 2}})) return s;
    if (C > 256) return RDETR_ERR_UNSUPPORTED;
    if (M == 0) return RDETR_OK;
    if (!xa || !pw1 || !b1 || !pw2 || !b2 || !w3 || !b3 || !reference || !out_a || (xb && !out_b) || !pwc || !bc || !out_cls)
        return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, pw1, pw2, w3, reference, out_a, pwc) || (xb && !aligned_to(out_b, 16)) || !all_aligned(2, out_cls, bc))
        return RDETR_ERR_UNSUPPORTED;
    const long long total = xb ? 2 * M : M, nblk = (total + kMlpRows - 1) / kMlpRows;
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    const MlpCls cl = {pwc, bc, out_cls, ldc, C};
    hipLaunchKernelGGL(box_head_cls_k256_kernel, dim3((unsigned)nblk), dim3(kMlpThreads), 0, static_cast<hipStream_t>(stream), xa,
                       lda, xb, ldb, pw1, b1, pw2, b2, w3, b3, reference, reference_is_logit, eps, M, out_a, out_b, cl);
    return launch_status();
}
