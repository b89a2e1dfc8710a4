// The decoder layer's query position as ONE kernel (bf16, embed_dim 256, gfx950):
//     query_pos = ref_point_head(sine_embed)                 MLP(512, 256, 256, 2)      relation_transformer.py:294, 343-344
//     query_pos = query_pos * query_scale(query)             MLP(256, 256, 256, 2)      relation_transformer.py:345-347 (layers >= 1)
//     qpp       = query + query_pos                          what the layer's self-attention takes as q = k  (:452-455)
// i.e. four library GEMMs of 1,800 rows + the product / sum launch of the decoder's dependency chain (~6 us each whatever their
// size, and the two MLPs are independent branches a single stream serialises) in one launch.
//
//   workgroup  16 rows x kQpWaves waves; the waves split the OUTPUT COLUMNS of every layer: wave w owns the tile pairs
//              u = kQpPairs w .. + kQpPairs - 1 (columns 32 u .. 32 u + 31) for all 16 rows.  1,800 rows are 113 workgroups.
//   weights    five [256, 256] blocks packed in fragment order (rdetr_linear_pack_k256_bf16; the 512-input layer as its two K
//              halves).  A fragment is needed by exactly one wave of the workgroup and goes global -> registers -> MFMA: no LDS
//              staging, no barrier around it.  Two register sets; the set a block has just consumed is refilled with the block
//              after the next behind a sched_barrier, so 16-32 coalesced 1-KiB loads per wave are in flight under every block's
//              MFMAs and the waits hipcc places are the counted in-order ones (vmcnt(n) per fragment, never a drain).
//   inputs     every wave loads the B operand of the workgroup's rows itself (emb 16 k-steps, query 8: L1 / L2 hits after the
//              first wave).
//   layers     with the output permutation of csrc/ffn.hip / csrc/mlp.hip lane (row, g) ends tile pair u holding outputs
//              32 u + 8 g .. + 7 of its row, which -- biased, ReLU'd, rounded to bf16 as the unfused path stores them -- ARE the
//              lane's B operand of the next layer's k-step u.  Both MLPs' first layers run first (they are independent), each
//              wave writes its pairs to an LDS image [u][lane] (1-KiB rows, conflict-free), ONE __syncthreads(), every wave reads
//              all 8 k-steps of both images.  Each image is written once per launch, so nothing can be overwritten under a reader.
//   in-proj    (query_pos_inproj_k256_kernel, rdetr_query_pos_inproj_k256_bf16) the layer's self-attention projects exactly this
//              kernel's outputs: q | k = (query + query_pos) [Wq ; Wk]^T + b, v = query Wv^T + b (relation_transformer.py:452-455),
//              two library GEMMs of the decoder's chain.  Three more packed blocks in the same two register sets: Wv is fetched
//              into the set the last ref_point_head block leaves, Wq into the one the last block before the sum leaves; every wave
//              writes its columns of query + query_pos (bf16, as stored) to a third image, runs the v block on the `query`
//              fragments it already holds while the others arrive (Wk fetched under it), ONE more __syncthreads(), then the q and
//              k blocks on the image; bias, one rounding to bf16, one 16-byte store per lane and pair.  out_pos / out_qpp are bit
//              for bit the plain kernel's.
//   arithmetic every output accumulates the same v_mfma_f32_16x16x32_bf16 products in the same k-step order as the row-split
//              kernel this replaces (s = 0 .. 7; K = 512 as half a then half b into one accumulator) with the same rounding
//              points (hidden activations, query_pos, the scale, their product, the sum): results are bit-identical to it, and
//              the unfused sequence's up to the summation order inside a dot product.
//   history    the previous kernel gave every wave 16 rows and ALL 256 columns: 29 workgroups at 1,800 rows, every weight half
//              staged in LDS and read from it by all 4 waves, 20 workgroup barriers; 21.7 us (17.4 without the LDS fragment
//              reads, 14.1 without the weight stream).  LDS-DMA for the staging was 25-28 us (100-350 cycles of issue per DMA
//              instruction behind its M0 write).
//   measured   (tools/time_qpos.py, graph replay, us per call; profiles/r09/time_chain_kernels.txt) rows 600 / 1,800 / 3,600:
//              12.1 / 12.4 / 12.9 (layer 0, no scale branch: 8.5 / 8.7 / 9.1); the row-split kernel in the same call 21.6 / 21.7 /
//              22.0 (14.6 / 14.8 / 15.0); the unfused sequence 20.8 / 22.7 / 29.1.  In the step (bench.py, both image groups'
//              launches side by side) together with csrc/mlp.hip: 3.90-3.95 -> 3.76-3.79 ms (ab_stack_chain_kernels.txt).
//              With the in-projection (profiles/r12/time_absorbed_kernels.txt, alternating, 5 runs each) rows 600 / 1,800 / 3,600:
//              16.0 / 16.6 / 17.3 (layer 0: 13.7 / 14.3 / 15.2) against this kernel followed by the two library GEMMs it absorbs
//              21.3 / 22.2 / 24.6 (17.7 / 18.5 / 21.0): about 1.4 us per extra block, 5.6 us less per layer at 1,800 rows.  In the step
//              (profiles/r12/decoder_chain_by_kernel.txt, ab_stack.txt) 18.2 us against 13.7 + 7.0 + 6.2, 15 launches per decoder
//              layer and image group instead of 18, and together with csrc/mlp.hip 3.725 -> 3.610 ms.
//   resources  (hipcc -Rpass-analysis=kernel-resource-usage) scaled / layer 0: 242 / 204 VGPRs, no AGPRs, no scratch, no spills,
//              16 / 8 KiB LDS, 2 waves per SIMD = one 8-wave workgroup per CU.  With the in-projection: 250 / 252 VGPRs, no AGPRs,
//              no scratch, 24 / 16 KiB LDS, 2 waves per SIMD (layer 0 loads `query` only after emb's registers are free: loaded
//              at the top it cost 116 bytes of scratch per lane).
//   dropped    4 waves x 2 tile pairs (kQpWaves = 4): both 32-fragment sets no longer fit 256 VGPRs, hipcc parks 80-168 of them in
//              AGPRs (v_accvgpr traffic, 1 wave per SIMD): 13.2 / 13.4 / 14.1 us and 0.5-1 % less in the step
//              (ab_candidates.txt).  32 rows per workgroup (two N blocks sharing each A fragment) was not built: the second block's
//              inputs (96 VGPRs) do not fit beside two fragment sets at 8 waves, and with one set the loads no longer overlap
//              the MFMAs of the previous block.  Loads under a lane mask for the rows >= M (`rok ? load : 0`): hipcc branches
//              around every one and put a vmcnt(0) between them.
#include "launch.h"

namespace rdetr {

namespace {

typedef __bf16 qp_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kQpWaves = 8, kQpThreads = kQpWaves * 64, kQpRows = 16;        // 16 rows per workgroup: 113 workgroups at 1,800 rows
constexpr int kQpPairs = 8 / kQpWaves;                                        // tile pairs (32 output columns each) per wave
constexpr int kQpFrags = kQpPairs * 16;                                       // fragments per wave and [256, 256] block
constexpr int kQpImg = 8 * 64;                                                // one exchange image in u32x4: [u][lane], 8 KiB
static_assert(kQpWaves == 4 || kQpWaves == 8, "the 8 tile pairs are dealt over 4 or 8 waves");

// the self-attention in-projection a layer runs on the kernel's outputs (rdetr_query_pos_inproj_k256_bf16)
struct QpInProj {
    const uint16_t *pwq, *pwk, *pwv, *bias;                                   // three packed [256, 256] blocks; bias [768] = q | k | v
    uint16_t *qk, *v;                                                         // [M, 512] = q | k and [M, 256]
    long long ldqk, ldv;
};

template <bool kScaled, bool kInProj>
__device__ __forceinline__ void query_pos_k256_body(
    const uint16_t *__restrict__ emb, long long lde, const uint16_t *__restrict__ query, long long ldq,
    const uint16_t *__restrict__ pw1a, const uint16_t *__restrict__ pw1b, const uint16_t *__restrict__ b1, const uint16_t *__restrict__ pw2,
    const uint16_t *__restrict__ b2, const uint16_t *__restrict__ pv1, const uint16_t *__restrict__ c1, const uint16_t *__restrict__ pv2,
    const uint16_t *__restrict__ c2, long long M, uint16_t *__restrict__ out_pos, uint16_t *__restrict__ out_qpp, const QpInProj &ip)
{
    __shared__ __attribute__((aligned(16))) u32x4 img[((kScaled ? 2 : 1) + (kInProj ? 1 : 0)) * kQpImg];
    u32x4 *const img_qpp = img + (kScaled ? 2 : 1) * kQpImg;                  // kInProj: the third exchange image, query + query_pos
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const int u0 = kQpPairs * wave;                                           // this wave's first tile pair (uniform)
    const long long row = (long long)blockIdx.x * kQpRows + col;
    const bool rok = row < M;
    // rows >= M read the last row instead (unconditional loads: a load under a lane mask costs a branch and, under register
    // pressure, a vmcnt(0)); a row of the MFMA's N dimension never reaches another row's outputs, and they store nothing
    const long long lrow = rok ? row : M - 1;

    // this wave's fragments of a packed block, in the order the MFMAs take them: pair uu, k-step s, tile e
    struct Frags { u32x4 f[kQpFrags]; };
    auto fetch = [&](const uint16_t *packed, Frags &w) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(packed) + (size_t)u0 * 16 * 64 + lane;
#pragma unroll
        for (int i = 0; i < kQpFrags; ++i) {
            const int uu = i >> 4, s = (i >> 1) & 7, e = i & 1;
            w.f[i] = p[((2 * uu + e) * 8 + s) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);                                    // the loads are issued HERE, not sunk to their MFMAs
    };
    auto mm = [&](const u32x4 &a, const u32x4 &bq, const f32x4 &c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(qp_bf16x8, a), __builtin_bit_cast(qp_bf16x8, bq), c, 0, 0, 0);
    };
    auto block = [&](const Frags &w, const u32x4 *xin, f32x4 (&acc)[kQpPairs][2]) {
#pragma unroll
        for (int i = 0; i < kQpFrags; ++i) {
            const int uu = i >> 4, s = (i >> 1) & 7, e = i & 1;
            acc[uu][e] = mm(w.f[i], xin[s], acc[uu][e]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto zero = [&](f32x4 (&acc)[kQpPairs][2]) {
#pragma unroll
        for (int uu = 0; uu < kQpPairs; ++uu) acc[uu][0] = acc[uu][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // the 8 bias values of the lane's outputs of pair u0 + uu, as bf16 pairs (2-byte loads: a bias needs no alignment)
    auto bias_of = [&](const uint16_t *bias, u32x4 (&bb)[kQpPairs]) {
#pragma unroll
        for (int uu = 0; uu < kQpPairs; ++uu) {
            const uint16_t *p = bias + 32 * (u0 + uu) + 8 * g;
            bb[uu] = u32x4{p[0] | (unsigned)p[1] << 16, p[2] | (unsigned)p[3] << 16, p[4] | (unsigned)p[5] << 16, p[6] | (unsigned)p[7] << 16};
        }
    };
    // biased (+ ReLU'd) and rounded to bf16: outputs 32 u + 8 g .. + 7 of the lane's row, u = u0 + uu
    auto finish = [&](const f32x4 (&acc)[kQpPairs][2], const u32x4 (&bb)[kQpPairs], bool relu, u32x4 (&y)[kQpPairs]) {
#pragma unroll
        for (int uu = 0; uu < kQpPairs; ++uu) {
            const u32x4 b = bb[uu];
            const f32x4 lo = acc[uu][0] + f32x4{bf16_bits_to_f32(b.x & 0xffffu), __builtin_bit_cast(float, b.x & 0xffff0000u),
                                                bf16_bits_to_f32(b.y & 0xffffu), __builtin_bit_cast(float, b.y & 0xffff0000u)};
            const f32x4 hi = acc[uu][1] + f32x4{bf16_bits_to_f32(b.z & 0xffffu), __builtin_bit_cast(float, b.z & 0xffff0000u),
                                                bf16_bits_to_f32(b.w & 0xffffu), __builtin_bit_cast(float, b.w & 0xffff0000u)};
            u32x4 p = {pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w)};
            if (relu) p = u32x4{relu_bf16x2(p.x), relu_bf16x2(p.y), relu_bf16x2(p.z), relu_bf16x2(p.w)};
            y[uu] = p;
        }
    };

    Frags wa, wb;
    u32x4 xe[16], xq[8];                                                      // B operands: k-step s = columns 32 s + 8 g .. + 7 of the lane's row
#pragma unroll
    for (int s = 0; s < 16; ++s) xe[s] = *reinterpret_cast<const u32x4 *>(emb + lrow * lde + 32 * s + 8 * g);
    fetch(pw1a, wa);
    fetch(pw1b, wb);
    if (kScaled) {
#pragma unroll
        for (int s = 0; s < 8; ++s) xq[s] = *reinterpret_cast<const u32x4 *>(query + lrow * ldq + 32 * s + 8 * g);
    }
    u32x4 bb1[kQpPairs], bb2[kQpPairs], cc1[kQpPairs], cc2[kQpPairs], qown[kQpPairs];
    bias_of(b1, bb1);
    bias_of(b2, bb2);
    if (kScaled) {
        bias_of(c1, cc1);
        bias_of(c2, cc2);
    }
#pragma unroll
    for (int uu = 0; uu < kQpPairs; ++uu)                                     // the wave's own columns of `query`, for query + query_pos
        qown[uu] = *reinterpret_cast<const u32x4 *>(query + lrow * ldq + 32 * (u0 + uu) + 8 * g);
    __builtin_amdgcn_sched_barrier(0);

    f32x4 acc[kQpPairs][2];
    u32x4 y[kQpPairs], pos[kQpPairs], h[8];
    // ---- first layers: ref_point_head.layers[0] (K = 512 = two packed blocks), query_scale.layers[0] ---------------------------
    zero(acc);
    block(wa, xe, acc);
    if (kScaled) fetch(pv1, wa); else fetch(pw2, wa);
    block(wb, xe + 8, acc);
    finish(acc, bb1, true, y);
#pragma unroll
    for (int uu = 0; uu < kQpPairs; ++uu) img[(u0 + uu) * 64 + lane] = y[uu];
    if (kScaled) {
        fetch(pw2, wb);
        zero(acc);
        block(wa, xq, acc);
        fetch(pv2, wa);
        finish(acc, cc1, true, y);
#pragma unroll
        for (int uu = 0; uu < kQpPairs; ++uu) img[kQpImg + (u0 + uu) * 64 + lane] = y[uu];
    } else if (kInProj) {                                                     // layer 0 reads `query` only now, in the registers emb has left
        fetch(ip.pwv, wb);
#pragma unroll
        for (int s = 0; s < 8; ++s) xq[s] = *reinterpret_cast<const u32x4 *>(query + lrow * ldq + 32 * s + 8 * g);
    }
    __syncthreads();                                                          // the one hand-over: every wave's columns of both hidden layers
    // ---- second layers -------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int s = 0; s < 8; ++s) h[s] = img[s * 64 + lane];
    zero(acc);
    block(kScaled ? wb : wa, h, acc);
    if (kInProj) fetch(kScaled ? ip.pwv : ip.pwq, kScaled ? wb : wa);         // in-projection: Wv into wb, Wq into wa, as each is freed
    finish(acc, bb2, false, pos);
    if (kScaled) {
        u32x4 sc[kQpPairs];
#pragma unroll
        for (int s = 0; s < 8; ++s) h[s] = img[kQpImg + s * 64 + lane];
        zero(acc);
        block(wa, h, acc);
        if (kInProj) fetch(ip.pwq, wa);
        finish(acc, cc2, false, sc);
        // query_pos * scale, rounded to bf16 as torch's bf16 multiply (fp32 product of the two bf16 values, one rounding)
#pragma unroll
        for (int uu = 0; uu < kQpPairs; ++uu) {
            const unsigned a[4] = {pos[uu].x, pos[uu].y, pos[uu].z, pos[uu].w}, b[4] = {sc[uu].x, sc[uu].y, sc[uu].z, sc[uu].w};
            unsigned o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o[k] = pack_bf16x2(bf16_bits_to_f32(a[k] & 0xffffu) * bf16_bits_to_f32(b[k] & 0xffffu),
                                   __builtin_bit_cast(float, a[k] & 0xffff0000u) * __builtin_bit_cast(float, b[k] & 0xffff0000u));
            pos[uu] = u32x4{o[0], o[1], o[2], o[3]};
        }
    }
    // query + query_pos of pair uu, rounded to bf16 as torch's bf16 add
    auto sum_of = [&](int uu) {
        const unsigned a[4] = {pos[uu].x, pos[uu].y, pos[uu].z, pos[uu].w}, q[4] = {qown[uu].x, qown[uu].y, qown[uu].z, qown[uu].w};
        unsigned o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[k] = pack_bf16x2(bf16_bits_to_f32(q[k] & 0xffffu) + bf16_bits_to_f32(a[k] & 0xffffu),
                               __builtin_bit_cast(float, q[k] & 0xffff0000u) + __builtin_bit_cast(float, a[k] & 0xffff0000u));
        return u32x4{o[0], o[1], o[2], o[3]};
    };
    if (!kInProj) {
        if (rok) {
#pragma unroll
            for (int uu = 0; uu < kQpPairs; ++uu) {
                const int u = u0 + uu;
                *reinterpret_cast<u32x4 *>(out_pos + row * 256 + 32 * u + 8 * g) = pos[uu];
                *reinterpret_cast<u32x4 *>(out_qpp + row * 256 + 32 * u + 8 * g) = sum_of(uu);
            }
        }
        return;
    }
    u32x4 qpp[kQpPairs];                                                      // every lane's, rows >= M included: it is the next B operand
#pragma unroll
    for (int uu = 0; uu < kQpPairs; ++uu) qpp[uu] = sum_of(uu);
    if (rok) {
#pragma unroll
        for (int uu = 0; uu < kQpPairs; ++uu) {
            *reinterpret_cast<u32x4 *>(out_pos + row * 256 + 32 * (u0 + uu) + 8 * g) = pos[uu];
            *reinterpret_cast<u32x4 *>(out_qpp + row * 256 + 32 * (u0 + uu) + 8 * g) = qpp[uu];
        }
    }
    // ---- the layer's self-attention in-projection (relation_transformer.py:452-455 -> nn.MultiheadAttention): q | k = Wq | Wk
    //      (query + query_pos) + b, v = Wv query + b.  v needs nothing of this kernel's, so its block runs while the other waves'
    //      columns of query + query_pos arrive in the third image; Wk is fetched under it ---------------------------------------
#pragma unroll
    for (int uu = 0; uu < kQpPairs; ++uu) img_qpp[(u0 + uu) * 64 + lane] = qpp[uu];
    u32x4 bq[kQpPairs], bk[kQpPairs], bv[kQpPairs];
    bias_of(ip.bias, bq);
    bias_of(ip.bias + 256, bk);
    bias_of(ip.bias + 512, bv);
    auto store = [&](uint16_t *out, long long ld, const u32x4 (&val)[kQpPairs]) {
        if (rok) {
#pragma unroll
            for (int uu = 0; uu < kQpPairs; ++uu) *reinterpret_cast<u32x4 *>(out + row * ld + 32 * (u0 + uu) + 8 * g) = val[uu];
        }
    };
    zero(acc);
    block(wb, xq, acc);
    fetch(ip.pwk, wb);
    finish(acc, bv, false, y);
    store(ip.v, ip.ldv, y);
    __syncthreads();                                                          // every wave's columns of query + query_pos
#pragma unroll
    for (int s = 0; s < 8; ++s) h[s] = img_qpp[s * 64 + lane];
    zero(acc);
    block(wa, h, acc);
    finish(acc, bq, false, y);
    store(ip.qk, ip.ldqk, y);
    zero(acc);
    block(wb, h, acc);
    finish(acc, bk, false, y);
    store(ip.qk + 256, ip.ldqk, y);
}

template <bool kScaled>
__global__ __launch_bounds__(kQpThreads) void query_pos_k256_kernel(
    const uint16_t *__restrict__ emb, long long lde, const uint16_t *__restrict__ query, long long ldq,
    const uint16_t *__restrict__ pw1a, const uint16_t *__restrict__ pw1b, const uint16_t *__restrict__ b1, const uint16_t *__restrict__ pw2,
    const uint16_t *__restrict__ b2, const uint16_t *__restrict__ pv1, const uint16_t *__restrict__ c1, const uint16_t *__restrict__ pv2,
    const uint16_t *__restrict__ c2, long long M, uint16_t *__restrict__ out_pos, uint16_t *__restrict__ out_qpp)
{
    query_pos_k256_body<kScaled, false>(emb, lde, query, ldq, pw1a, pw1b, b1, pw2, b2, pv1, c1, pv2, c2, M, out_pos, out_qpp, QpInProj{});
}

template <bool kScaled>
__global__ __launch_bounds__(kQpThreads) void query_pos_inproj_k256_kernel(
    const uint16_t *__restrict__ emb, long long lde, const uint16_t *__restrict__ query, long long ldq,
    const uint16_t *__restrict__ pw1a, const uint16_t *__restrict__ pw1b, const uint16_t *__restrict__ b1, const uint16_t *__restrict__ pw2,
    const uint16_t *__restrict__ b2, const uint16_t *__restrict__ pv1, const uint16_t *__restrict__ c1, const uint16_t *__restrict__ pv2,
    const uint16_t *__restrict__ c2, long long M, uint16_t *__restrict__ out_pos, uint16_t *__restrict__ out_qpp, QpInProj ip)
{
    query_pos_k256_body<kScaled, true>(emb, lde, query, ldq, pw1a, pw1b, b1, pw2, b2, pv1, c1, pv2, c2, M, out_pos, out_qpp, ip);
}

}  // namespace

}  // namespace rdetr

using namespace rdetr;

// out_pos [M, 256] = MLP2(emb [M, 512]) (* MLP2'(query [M, 256]) when pv1 / c1 / pv2 / c2 are given), out_qpp = query + out_pos; bf16.
// pw1a / pw1b: the K halves [:, :256] / [:, 256:] of ref_point_head.layers[0].weight [256, 512]; pw2, pv1, pv2: [256, 256] weights;
// all five packed by rdetr_linear_pack_k256_bf16.  b1, b2, c1, c2: bf16 [256].  Row strides lde / ldq in elements.
extern "C" int rdetr_query_pos_k256_bf16(const uint16_t *emb, long long lde, const uint16_t *query, long long ldq, const uint16_t *pw1a,
                                         const uint16_t *pw1b, const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2, const uint16_t *pv1,
                                         const uint16_t *c1, const uint16_t *pv2, const uint16_t *c2, long long M, uint16_t *out_pos,
                                         uint16_t *out_qpp, void *stream)
{
    if (M < 0) return RDETR_ERR_INVALID_ARG;
    if (const int s = rows_status({{emb, lde, 512, 2}, {query, ldq, 256, 2}})) return s;
    if (M == 0) return RDETR_OK;
    if (!emb || !query || !pw1a || !pw1b || !b1 || !pw2 || !b2 || !out_pos || !out_qpp) return RDETR_ERR_INVALID_ARG;
    const bool any = pv1 || c1 || pv2 || c2, all = pv1 && c1 && pv2 && c2;
    if (any && !all) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, pw1a, pw1b, pw2, pv1, pv2, out_pos, out_qpp)) return RDETR_ERR_UNSUPPORTED;
    const long long nblk = (M + kQpRows - 1) / kQpRows;
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    if (all)
        hipLaunchKernelGGL(query_pos_k256_kernel<true>, dim3((unsigned)nblk), dim3(kQpThreads), 0, static_cast<hipStream_t>(stream), emb, lde,
                           query, ldq, pw1a, pw1b, b1, pw2, b2, pv1, c1, pv2, c2, M, out_pos, out_qpp);
    else
        hipLaunchKernelGGL(query_pos_k256_kernel<false>, dim3((unsigned)nblk), dim3(kQpThreads), 0, static_cast<hipStream_t>(stream), emb, lde,
                           query, ldq, pw1a, pw1b, b1, pw2, b2, pv1, c1, pv2, c2, M, out_pos, out_qpp);
    return launch_status();
}

// rdetr_query_pos_k256_bf16 plus the in-projection of the layer's self-attention on its outputs, in the same launch:
//     out_qk [M, 512] = out_qpp [Wq ; Wk]^T + bias[:512],  out_v [M, 256] = query Wv^T + bias[512:]     (bf16, row strides ldqk / ldv)
// pwq / pwk / pwv: in_proj_weight[:256] / [256:512] / [512:] packed by rdetr_linear_pack_k256_bf16; bias bf16 [768].  out_qk is
// computed from out_qpp as stored (bf16); out_pos / out_qpp are bit for bit what rdetr_query_pos_k256_bf16 writes.
extern "C" int rdetr_query_pos_inproj_k256_bf16(const uint16_t *emb, long long lde, const uint16_t *query, long long ldq, const uint16_t *pw1a,
                                                const uint16_t *pw1b, const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2,
                                                const uint16_t *pv1, const uint16_t *c1, const uint16_t *pv2, const uint16_t *c2,
                                                const uint16_t *pwq, const uint16_t *pwk, const uint16_t *pwv, const uint16_t *bias, long long M,
                                                uint16_t *out_pos, uint16_t *out_qpp, uint16_t *out_qk, long long ldqk, uint16_t *out_v,
                                                long long ldv, void *stream)
{
    if (M < 0) return RDETR_ERR_INVALID_ARG;
    if (const int s = rows_status({{emb, lde, 512, 2}, {query, ldq, 256, 2}, {out_qk, ldqk, 512, 2}, {out_v, ldv, 256, 2}})) return s;
    if (M == 0) return RDETR_OK;
    if (!emb || !query || !pw1a || !pw1b || !b1 || !pw2 || !b2 || !out_pos || !out_qpp || !pwq || !pwk || !pwv || !bias || !out_qk || !out_v)
        return RDETR_ERR_INVALID_ARG;
    const bool any = pv1 || c1 || pv2 || c2, all = pv1 && c1 && pv2 && c2;
    if (any && !all) return RDETR_ERR_INVALID_ARG;
    if (!all_aligned(16, pw1a, pw1b, pw2, pv1, pv2, out_pos, out_qpp, pwq, pwk, pwv)) return RDETR_ERR_UNSUPPORTED;
    const long long nblk = (M + kQpRows - 1) / kQpRows;
    if (!grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    const QpInProj ip = {pwq, pwk, pwv, bias, out_qk, out_v, ldqk, ldv};
    if (all)
        hipLaunchKernelGGL(query_pos_inproj_k256_kernel<true>, dim3((unsigned)nblk), dim3(kQpThreads), 0, static_cast<hipStream_t>(stream),
                           emb, lde, query, ldq, pw1a, pw1b, b1, pw2, b2, pv1, c1, pv2, c2, M, out_pos, out_qpp, ip);
    else
        hipLaunchKernelGGL(query_pos_inproj_k256_kernel<false>, dim3((unsigned)nblk), dim3(kQpThreads), 0, static_cast<hipStream_t>(stream),
                           emb, lde, query, ldq, pw1a, pw1b, b1, pw2, b2, pv1, c1, pv2, c2, M, out_pos, out_qpp, ip);
    return launch_status();
}
