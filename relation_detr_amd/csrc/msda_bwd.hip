// Multi-scale deformable attention, backward (fp32; fused-producer form fp32 and bf16) -- hand-written for gfx950 (MI355X).
//
// Replaces ms_deformable_col2im_cuda and, for head_dim 32, its kernel
// ms_deformable_col2im_gpu_kernel_shm_blocksize_aware_reduce_v1<T,32>
// (models/bricks/ops/cuda/ms_deform_im2col_cuda.cuh:290-392,1129-1150: block = 32 threads = one
// (b,q,head), 4 atomicAdd per thread per point, thread 0 serially sums 32 partials for the
// location / weight gradients).
//
// ONE BODY, TWO PRODUCERS.  One wavefront owns one head and two consecutive queries, one channel per lane.  The body is defined
// once and used by every instantiation:
//   * bwd_prologue    -- level table into LDS, logical block -> (image, head, wave, query of the pair, channel);
//   * bwd_stage_point -- lane (pair, c) turns point c of its query (pixel coordinates, weight) into what the loop reads from LDS:
//                        four corner byte offsets (0x80000000 = no row, dropped by the buffer range check), {hy, hx, ly, lx} and
//                        {weight, W_l, H_l, inside}; "inside a level" and the NaN rule live here, and so do the records of the
//                        deterministic mode;
//   * bwd_point_loop  -- per point the 4 corner rows are re-gathered (needed for d/dloc and d/dweight), `w_corner * g * weight` is
//                        scattered into grad_value with hardware fp32 atomics whose wave instruction covers two full 128-byte
//                        head rows, and the sums over D = 32 channels are 32-lane xor-shuffle reductions instead of a
//                        shared-memory pass; lane c leaves with point c's (d/dweight, d/dx, d/dy).
// A producer is what surrounds them: how a lane obtains (x, y, weight) and what it does with the three sums.
// msda_bwd_wave_kernel (materialised) loads location and weight and stores the sums; msda_bwd_fused_kernel recomputes both from
// raw offsets / logits / reference points as the forward did, then runs the softmax backward and the chain rule onto them.
// BwdPlane<T, HM> is the addressing of one (image, head) plane: fp32 or bf16 value, [B,S,H,D] or head-major.
//
// Float atomics make grad_value's summation order run-dependent (as in the reference).  DETERMINISTIC mode (DET; SURVEY section 8
// f4 "deterministic alternative to atomics"): bwd_stage_point writes one (grad_value-row key, weight) record per sample corner and
// the loop does not add; the records are sorted by key with a stable radix sort (hipCUB / rocPRIM, caller-provided temporary
// storage) and `msda_bwd_segment_sum_kernel` adds each row's records in sorted = original sample order -- the same bits from run
// to run.  Every other gradient is a shuffle-tree sum inside a wave: the same bits in both modes.
#include <hipcub/hipcub.hpp>

#include "launch.h"

namespace rdetr {

constexpr int kBH = 8, kBD = 32, kBP = 4, kBMaxL = 8, kBWaves = 4;
constexpr unsigned kBInvalid = 0x80000000u;
constexpr unsigned kBPixelBytes = kBH * kBD * 4, kBHeadBytes = kBD * 4;

struct BwdLevels {
    int h[kBMaxL], w[kBMaxL], start[kBMaxL];
};

// sum over the 32 lanes of one (query, head) row (lanes 0-31 / 32-63 reduce independently)
__device__ __forceinline__ float sum32(float v)
{
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    return v;
}

// The block's LDS: the level table and, per wave, [point][pair]: corner offsets | {hy, hx, ly, lx} | {weight (0 if outside), W_l,
// H_l, inside}
struct BwdShared {
    BwdLevels lvl;
    u32x4 st_off[kBWaves][kBMaxL * kBP * 2];
    f32x4 st_frac[kBWaves][kBMaxL * kBP * 2];
    f32x4 st_misc[kBWaves][kBMaxL * kBP * 2];
};

// Where a lane works.  One wavefront = ONE head x TWO consecutive queries; lane = pair*32 + c, one channel per lane (and, in the
// set-up, one point per lane).  Every atomic wave instruction therefore adds two full 128-byte head rows (the access shape that
// runs at the chip-wide float-atomic rate, MI355X_MICROARCH.md "Global float atomics"; the first version, 4 channels per lane
// x 8 heads, added 8 x 32 sparse bytes per instruction and reached 0.36 TB/s).
struct BwdLane {
    int b, m, wave, pair, c, q;     // image, head, wave of the block, query of the wave's two, channel, query index
    bool qok;                       // q < Nq
};

// level table -> LDS; logical block -> (image b, head m, tile of 2*kBWaves consecutive queries)
__device__ __forceinline__ BwdLane bwd_prologue(BwdShared &sh, const int64_t *__restrict__ shapes, const int64_t *__restrict__ level_start,
                                                int L, int Nq, int tiles_per_image, int nblk)
{
    const int tid = threadIdx.x;
    if (tid < L) {
        sh.lvl.h[tid] = (int)shapes[2 * tid];
        sh.lvl.w[tid] = (int)shapes[2 * tid + 1];
        sh.lvl.start[tid] = (int)level_start[tid];
    }
    __syncthreads();

    const int logical = xcd_contiguous_block(blockIdx.x, nblk);
    const int bm = logical / tiles_per_image;
    const int tile = logical - bm * tiles_per_image;
    const int b = bm / kBH, m = bm - b * kBH;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, pair = lane >> 5, c = lane & 31;
    const int q = (tile * kBWaves + wave) * 2 + pair;
    return BwdLane{b, m, wave, pair, c, q, q < Nq};
}

// The plane of (image b, head m) in value (T: fp32, or bf16 loaded two bytes per lane and converted) and in the fp32 grad_value.
// [B,S,H,D]: a pixel is 1 KiB of grad_value (sizeof(T) * 256 bytes of value) and the descriptors run from the head's first row to
// the end of the image.  HM, head-major [B,H,S,D] -- an addressing matter only: the plane starts at ((b*H + m) * S) * D, a pixel is
// one 128-byte grad row (64 bytes of bf16 value) and the descriptors cover exactly that plane (an out-of-level corner and anything
// past pixel S-1 is dropped, it cannot land in the next head's plane).  Offsets are grad_value byte offsets at pixel pitch kPix,
// shifted right by one for a bf16 value (the invalid offset 0x80000000 stays out of range).
template <typename T, bool HM>
struct BwdPlane {
    static constexpr bool kBf16 = sizeof(T) == 2;
    static constexpr unsigned kPix = HM ? kBHeadBytes : kBPixelBytes;     // bytes from one pixel's grad_value row to the next
    __amdgpu_buffer_rsrc_t rs_v, rs_g;
    unsigned lane_off, lane_off_v;

    __device__ __forceinline__ BwdPlane(const T *value, float *grad_value, const BwdLane &ln, int S)
    {
        const size_t plane = HM ? ((size_t)ln.b * kBH + ln.m) * (size_t)S * kBD : (size_t)ln.b * S * (kBH * kBD) + (size_t)ln.m * kBD;
        const unsigned nrec = HM ? (unsigned)S * kBHeadBytes : (unsigned)S * kBPixelBytes - (unsigned)ln.m * kBHeadBytes;
        rs_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(value) + plane, 0, kBf16 ? nrec / 2 : nrec, 0x00020000);
        rs_g = __builtin_amdgcn_make_buffer_rsrc(grad_value + plane, 0, nrec, 0x00020000);
        lane_off = (unsigned)ln.c * 4u;
        lane_off_v = (unsigned)ln.c * (unsigned)sizeof(T);
    }
    __device__ __forceinline__ float load(unsigned off) const
    {
        if constexpr (kBf16)
            return bf16_bits_to_f32(__builtin_amdgcn_raw_buffer_load_b16(rs_v, (off >> 1) + lane_off_v, 0, 0));
        else
            return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_v, off + lane_off_v, 0, 0));
    }
    __device__ __forceinline__ void add(float v, unsigned off) const
    {
        __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, rs_g, off + lane_off, 0, 0);
    }
};

// Lane (pair, c) stages point c of its query: (x, y) in pixel coordinates of level l = c / P, `weight` its attention weight.
// Returns whether the point is inside its level (false for a NaN location, whose every derived value is then selected to 0).
// DET: also one record per corner: key = the row of grad_value it adds to -- (image, pixel, head), or head-major (image, head,
// pixel); all ones: no row --, weight = bilinear weight * attention weight; the record's position (hrow + c) * 4 + corner IS its
// identity (query, head, point, corner).
template <bool DET, bool HM>
__device__ __forceinline__ bool bwd_stage_point(BwdShared &sh, const BwdLane &ln, float x, float y, float weight, int S, size_t hrow,
                                                unsigned *__restrict__ rec_key, unsigned *__restrict__ rec_id, float *__restrict__ rec_w)
{
    constexpr unsigned kPix = HM ? kBHeadBytes : kBPixelBytes;
    const int l = ln.c / kBP;
    const int h = sh.lvl.h[l], w = sh.lvl.w[l];
    const bool inside = ln.qok && (y > -1.f) && (x > -1.f) && (y < (float)h) && (x < (float)w);
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = inside ? (int)xf : 0, y0 = inside ? (int)yf : 0;
    const float lx = inside ? x - xf : 0.f, ly = inside ? y - yf : 0.f;   // NaN-safe
    const bool okx0 = inside && x0 >= 0, okx1 = inside && x0 + 1 <= w - 1;
    const bool oky0 = y0 >= 0, oky1 = y0 + 1 <= h - 1;
    const unsigned base = (unsigned)(sh.lvl.start[l] + y0 * w + x0) * kPix;
    const unsigned rowb = (unsigned)w * kPix;
    u32x4 o;
    o.x = (okx0 && oky0) ? base : kBInvalid;
    o.y = (okx1 && oky0) ? base + kPix : kBInvalid;
    o.z = (okx0 && oky1) ? base + rowb : kBInvalid;
    o.w = (okx1 && oky1) ? base + rowb + kPix : kBInvalid;
    const float a = inside ? weight : 0.f;
    sh.st_off[ln.wave][ln.c * 2 + ln.pair] = o;
    sh.st_frac[ln.wave][ln.c * 2 + ln.pair] = f32x4{1.f - ly, 1.f - lx, ly, lx};
    sh.st_misc[ln.wave][ln.c * 2 + ln.pair] = f32x4{a, (float)w, (float)h, inside ? 1.f : 0.f};
    if constexpr (DET) {
        if (ln.qok) {
            const unsigned rbase = HM ? (unsigned)(((size_t)ln.b * kBH + ln.m) * (size_t)S) : (unsigned)((size_t)ln.b * S) * kBH + (unsigned)ln.m;
            const float hy = 1.f - ly, hx = 1.f - lx;
            auto key = [&](unsigned ob) { return ob == kBInvalid ? 0xffffffffu : rbase + (ob / kPix) * (HM ? 1u : (unsigned)kBH); };
            const size_t rec = (hrow + ln.c) * 4;
            *reinterpret_cast<u32x4 *>(rec_key + rec) = u32x4{key(o.x), key(o.y), key(o.z), key(o.w)};
            *reinterpret_cast<u32x4 *>(rec_id + rec) = u32x4{(unsigned)rec, (unsigned)rec + 1u, (unsigned)rec + 2u, (unsigned)rec + 3u};
            *reinterpret_cast<f32x4 *>(rec_w + rec) = f32x4{(hy * hx) * a, (hy * lx) * a, (ly * hx) * a, (ly * lx) * a};
        }
    }
    return inside;
}

// what a wave's lanes staged becomes visible to the wave
__device__ __forceinline__ void bwd_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct BwdSums {
    float s, gx, gy;                // d loss / d weight, d loss / d (normalised x), d loss / d (normalised y)
};

// Every lane (channel c, top gradient g) walks the LP staged points of its query; -> the sums of point `c`, kept by lane c of the pair
template <bool DET, typename Plane>
__device__ __forceinline__ BwdSums bwd_point_loop(const BwdShared &sh, const BwdLane &ln, const Plane &pl, int LP, float g)
{
    const u32x4 *soff = sh.st_off[ln.wave];
    const f32x4 *sfrac = sh.st_frac[ln.wave];
    const f32x4 *smisc = sh.st_misc[ln.wave];
    BwdSums my{0.f, 0.f, 0.f};

#pragma nounroll
    for (int pt = 0; pt < LP; ++pt) {
        const u32x4 o = soff[pt * 2 + ln.pair];
        const f32x4 fr = sfrac[pt * 2 + ln.pair];      // hy, hx, ly, lx
        const f32x4 mi = smisc[pt * 2 + ln.pair];      // weight (0 if outside), W, H, inside
        const float v00 = pl.load(o.x), v01 = pl.load(o.y), v10 = pl.load(o.z), v11 = pl.load(o.w);
        const float hy = fr.x, hx = fr.y, ly = fr.z, lx = fr.w;
        const float ga = g * mi.x;                                   // top_grad * weight
        if constexpr (!DET) {
            pl.add((hy * hx) * ga, o.x);
            pl.add((hy * lx) * ga, o.y);
            pl.add((ly * hx) * ga, o.z);
            pl.add((ly * lx) * ga, o.w);
        }
        // d/dx and d/dy of the bilinear sample (ms_deform_im2col_cuda.cuh:102-141)
        const float dxs = hy * (v01 - v00) + ly * (v11 - v10);
        const float dys = hx * (v10 - v00) + lx * (v11 - v01);
        const float smp = (hy * hx) * v00 + (hy * lx) * v01 + (ly * hx) * v10 + (ly * lx) * v11;
        const float s = sum32(g * smp) * mi.w;                       // grad wrt the weight
        const float gx = sum32(ga * dxs) * mi.y;                     // * W_l
        const float gy = sum32(ga * dys) * mi.z;                     // * H_l
        if (ln.c == pt) {
            my.s = s;
            my.gx = gx;
            my.gy = gy;
        }
    }
    return my;
}

// Materialised producer: sampling locations and attention weights as the reference operator takes them; the sums are the result.
template <bool DET>
__global__ __launch_bounds__(kBWaves *kWave) void msda_bwd_wave_kernel(
    const float *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ level_start,
    const float *__restrict__ loc, const float *__restrict__ attn, const float *__restrict__ grad_out, int S, int L,
    int Nq, int tiles_per_image, int nblk, float *__restrict__ grad_value, float *__restrict__ grad_loc,
    float *__restrict__ grad_attn, unsigned *__restrict__ rec_key, unsigned *__restrict__ rec_id, float *__restrict__ rec_w)
{
    const int LP = L * kBP;
    __shared__ BwdShared sh;
    const BwdLane ln = bwd_prologue(sh, shapes, level_start, L, Nq, tiles_per_image, nblk);
    const BwdPlane<float, false> pl(value, grad_value, ln, S);
    const int c = ln.c;
    const size_t row = (size_t)ln.b * Nq + (ln.qok ? ln.q : 0);
    const size_t hrow = (row * kBH + ln.m) * (size_t)LP;

    if (c < LP) {
        const f32x2 xy = *reinterpret_cast<const f32x2 *>(loc + (hrow + c) * 2);
        const float a = attn[hrow + c];
        const int l = c / kBP;
        const int h = sh.lvl.h[l], w = sh.lvl.w[l];
        const float x = xy.x * (float)w - 0.5f, y = xy.y * (float)h - 0.5f;
        bwd_stage_point<DET, false>(sh, ln, x, y, a, S, hrow, rec_key, rec_id, rec_w);
    }
    bwd_wave_fence();

    const float g = grad_out[row * (kBH * kBD) + ln.m * kBD + c];
    const BwdSums my = bwd_point_loop<DET>(sh, ln, pl, LP, g);
    if (ln.qok && c < LP) {                                           // 16-20 contiguous floats per query-head
        grad_attn[hrow + c] = my.s;
        *reinterpret_cast<f32x2 *>(grad_loc + (hrow + c) * 2) = f32x2{my.gx, my.gy};
    }
}

__device__ __forceinline__ float ld_f32(const float *p) { return *p; }
__device__ __forceinline__ float ld_f32(const uint16_t *p) { return bf16_bits_to_f32(*p); }
__device__ __forceinline__ f32x2 ld_f32x2(const float *p) { return *reinterpret_cast<const f32x2 *>(p); }
__device__ __forceinline__ f32x2 ld_f32x2(const uint16_t *p)
{
    const unsigned u = *reinterpret_cast<const unsigned *>(p);
    return f32x2{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
}
__device__ __forceinline__ void st_val(float *p, float v) { *p = v; }
__device__ __forceinline__ void st_val(uint16_t *p, float v) { *p = (uint16_t)f32_to_bf16_bits(v); }
__device__ __forceinline__ void st_val2(float *p, float x, float y) { *reinterpret_cast<f32x2 *>(p) = f32x2{x, y}; }
__device__ __forceinline__ void st_val2(uint16_t *p, float x, float y) { *reinterpret_cast<unsigned *>(p) = pack_bf16x2(x, y); }

// Fused producer (rdetr_msda_backward_fused_*): the inputs of the fused forward (raw offsets and logits in value's dtype, reference
// points) instead of materialised locations / weights.
//   * set-up: lane (pair, c) recomputes the soft-maxed weight and the sampling location of point c (L*P <= 32: both queries in 64
//     lanes, lanes c >= L*P are -inf padding slots) with the arithmetic of the forward kernel for that dtype (msda_fwd.hip: fp32
//     expf and divisions; bf16 the hardware exp2 and products with reciprocals), max and sum by xor-shuffles, so the backward
//     differentiates the weights and locations the forward used;
//   * closing step, in the set-up layout (coalesced rows): softmax backward grad_logit_k = w_k (s_k - sum_j w_j s_j) with
//     s_k = <grad_out, sample_k>, the location chain rule onto the offsets, and per-level sums onto the reference point.
// Every sum except grad_value's is a fixed shuffle tree: grad_offsets / grad_logits / grad_ref are the same bits in both modes.
// HM (rdetr_msda_backward_fused_hm_bf16): value and grad_value are head-major (BwdPlane), and the raw producer inputs and their
// gradients take row strides (elements), so that each pair can be two column slices of one [B*Nq, 3*H*L*P] buffer.
template <typename T, bool DET, bool HM>
__global__ __launch_bounds__(kBWaves *kWave) void msda_bwd_fused_kernel(
    const T *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ level_start,
    const T *__restrict__ offsets, const T *__restrict__ logits, const float *__restrict__ ref, int ref_dim,
    const T *__restrict__ grad_out, int S, int L, int Nq, int tiles_per_image, int nblk, float *__restrict__ grad_value,
    T *__restrict__ grad_offsets, T *__restrict__ grad_logits, float *__restrict__ grad_ref, unsigned *__restrict__ rec_key,
    unsigned *__restrict__ rec_id, float *__restrict__ rec_w, int ld_off, int ld_lg, int ld_goff, int ld_glg)
{
    constexpr bool kBf16 = sizeof(T) == 2;
    const int LP = L * kBP;
    __shared__ BwdShared sh;
    const BwdLane ln = bwd_prologue(sh, shapes, level_start, L, Nq, tiles_per_image, nblk);
    const BwdPlane<T, HM> pl(value, grad_value, ln, S);
    const int m = ln.m, c = ln.c;
    const bool qok = ln.qok;

    const size_t row = (size_t)ln.b * Nq + (qok ? ln.q : 0);
    const size_t hrow = (row * kBH + m) * (size_t)LP;
    // this (query, head)'s LP logits / 2*LP offsets and their gradients: dense rows, or (HM) rows ld_* elements apart
    const size_t i_lg = HM ? row * (size_t)ld_lg + (size_t)(m * LP) : hrow;
    const size_t i_off = HM ? row * (size_t)ld_off + (size_t)(m * LP) * 2 : hrow * 2;
    const size_t i_glg = HM ? row * (size_t)ld_glg + (size_t)(m * LP) : hrow;
    const size_t i_goff = HM ? row * (size_t)ld_goff + (size_t)(m * LP) * 2 : hrow * 2;

    // ---- set-up: lane (pair, c) = point c of its query; softmax over the 32 lanes of the pair -------------------------------
    const bool pok = c < LP;
    const int l = pok ? c / kBP : 0;
    const int h = sh.lvl.h[l], w = sh.lvl.w[l];
    const float lg = pok ? ld_f32(logits + i_lg + c) : -__builtin_inff();
    const f32x2 off = pok ? ld_f32x2(offsets + i_off + c * 2) : f32x2{0.f, 0.f};
    float mx = lg;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float e = kBf16 ? __builtin_amdgcn_exp2f((lg - mx) * 1.44269504088896341f) : expf(lg - mx);    // 0 for padding
    const float sum = sum32(e);
    const float wk = kBf16 ? e * (1.0f / sum) : e / sum;
    const float *rp = ref + (row * L + l) * (size_t)ref_dim;
    const f32x4 rc = ref_dim == 2 ? f32x4{rp[0], rp[1], 0.f, 0.f} : f32x4{rp[0], rp[1], rp[2], rp[3]};
    f32x2 xy;
    if (ref_dim == 2) {
        if (kBf16 && (L == 4 || L == 5)) {             // the forward's 4- and 5-level bf16 kernels multiply by reciprocals
            xy.x = rc.x + off.x * (1.0f / (float)w);
            xy.y = rc.y + off.y * (1.0f / (float)h);
        } else {
            xy.x = rc.x + off.x / (float)w;
            xy.y = rc.y + off.y / (float)h;
        }
    } else {
        xy.x = rc.x + off.x * (1.0f / kBP) * rc.z * 0.5f;
        xy.y = rc.y + off.y * (1.0f / kBP) * rc.w * 0.5f;
    }
    const float x = xy.x * (float)w - 0.5f, y = xy.y * (float)h - 0.5f;
    const bool inside = pok && bwd_stage_point<DET, HM>(sh, ln, x, y, wk, S, hrow, rec_key, rec_id, rec_w);
    bwd_wave_fence();

    const float g = ld_f32(grad_out + row * (kBH * kBD) + m * kBD + c);
    const BwdSums my = bwd_point_loop<DET>(sh, ln, pl, LP, g);
    const float my_s = my.s, my_gx = my.gx, my_gy = my.gy;

    // ---- closing step, lane = point: softmax backward, offsets, reference-point partials ------------------------------------
    const float tot = sum32(wk * my_s);                               // padding lanes: 0 * 0
    const float g_logit = wk * (my_s - tot);
    float gox, goy, rz = 0.f, rw = 0.f;
    if (ref_dim == 2) {
        gox = my_gx / (float)w;
        goy = my_gy / (float)h;
    } else {
        gox = my_gx * rc.z * (0.5f / kBP);
        goy = my_gy * rc.w * (0.5f / kBP);
        rz = inside ? my_gx * off.x * (0.5f / kBP) : 0.f;             // NaN offsets of outside points contribute nothing
        rw = inside ? my_gy * off.y * (0.5f / kBP) : 0.f;
    }
    // sum over the P = 4 points of a level (lanes 4l .. 4l+3)
    float rx = my_gx, ry = my_gy;
#pragma unroll
    for (int o = 1; o < kBP; o <<= 1) {
        rx += __shfl_xor(rx, o, 64);
        ry += __shfl_xor(ry, o, 64);
        rz += __shfl_xor(rz, o, 64);
        rw += __shfl_xor(rw, o, 64);
    }
    if (qok && pok) {
        st_val(grad_logits + i_glg + c, g_logit);
        st_val2(grad_offsets + i_goff + c * 2, gox, goy);
        if (grad_ref && (c & (kBP - 1)) == 0) {
            float *gr = grad_ref + ((row * kBH + m) * L + l) * (size_t)ref_dim;
            if (ref_dim == 2)
                *reinterpret_cast<f32x2 *>(gr) = f32x2{rx, ry};
            else
                *reinterpret_cast<f32x4 *>(gr) = f32x4{rx, ry, rz, rw};
        }
    }
}

// Deterministic mode, second half: grad_value row r = (image, pixel, head) is the sum of ITS records in sorted order.  Half a wave
// per row (lane = channel); the segment [lo, hi) of the sorted keys by binary search (uniform per half wave); the record gives the
// weight and, through its position, the (image, query, head) row of grad_out (fp32, or bf16 for the fused bf16 backward).  Every
// row is written (empty segment: zeros), so grad_value needs no zero-initialisation in this mode.
template <typename G>
__global__ __launch_bounds__(256) void msda_bwd_segment_sum_kernel(const unsigned *__restrict__ skey, const unsigned *__restrict__ sid,
                                                                  const float *__restrict__ rec_w, const G *__restrict__ grad_out,
                                                                  long long nrec, long long nrows, int LP, float *__restrict__ grad_value)
{
    const long long r = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int c = threadIdx.x & 31;
    if (r >= nrows) return;
    auto lower = [&](unsigned k) {                                              // first i with skey[i] >= k
        long long lo = 0, hi = nrec;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (skey[mid] < k) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const long long lo = lower((unsigned)r), hi = lower((unsigned)r + 1u);
    float acc = 0.f;
    for (long long i = lo; i < hi; ++i) {
        const unsigned id = sid[i];
        const unsigned rowhm = (id >> 2) / (unsigned)LP;                       // (image * Nq + query) * 8 + head
        acc = __builtin_fmaf(rec_w[id], ld_f32(grad_out + (size_t)rowhm * kBD + c), acc);
    }
    grad_value[(size_t)r * kBD + c] = acc;
}

// Generic fallback: one thread per (b, q, head, point), loops over D; any (H, D, L, P).
__global__ __launch_bounds__(256) void msda_bwd_generic_kernel(
    const float *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ level_start,
    const float *__restrict__ loc, const float *__restrict__ attn, const float *__restrict__ grad_out, int S, int H,
    int D, int L, int Nq, int P, long long total, float *__restrict__ grad_value, float *__restrict__ grad_loc,
    float *__restrict__ grad_attn)
{
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (long long)gridDim.x * blockDim.x) {
        const int l = (int)((k / P) % L);
        const long long r = k / ((long long)L * P);          // (b*Nq + q)*H + m
        const int m = (int)(r % H);
        const long long bq = r / H;
        const long long b = bq / Nq;
        const long long pix = (long long)H * D;
        const int h = (int)shapes[2 * l], w = (int)shapes[2 * l + 1];
        const float x = loc[2 * k] * (float)w - 0.5f, y = loc[2 * k + 1] * (float)h - 0.5f;
        float g_a = 0.f, g_x = 0.f, g_y = 0.f;
        if ((y > -1.f) && (x > -1.f) && (y < (float)h) && (x < (float)w)) {
            const float a = attn[k];
            const float xf = floorf(x), yf = floorf(y);
            const int x0 = (int)xf, y0 = (int)yf;
            const float lx = x - xf, ly = y - yf, hx = 1.f - lx, hy = 1.f - ly;
            const bool k00 = y0 >= 0 && x0 >= 0, k01 = y0 >= 0 && x0 + 1 <= w - 1;
            const bool k10 = y0 + 1 <= h - 1 && x0 >= 0, k11 = y0 + 1 <= h - 1 && x0 + 1 <= w - 1;
            const long long o00 = b * S * pix + (level_start[l] + (long long)y0 * w + x0) * pix + (long long)m * D;
            const long long o01 = o00 + pix, o10 = o00 + (long long)w * pix, o11 = o10 + pix;
            const float *go = grad_out + bq * pix + (long long)m * D;
            for (int c = 0; c < D; ++c) {
                const float gc = go[c], ga = gc * a;
                const float v00 = k00 ? value[o00 + c] : 0.f, v01 = k01 ? value[o01 + c] : 0.f;
                const float v10 = k10 ? value[o10 + c] : 0.f, v11 = k11 ? value[o11 + c] : 0.f;
                if (k00) atomicAdd(grad_value + o00 + c, hy * hx * ga);
                if (k01) atomicAdd(grad_value + o01 + c, hy * lx * ga);
                if (k10) atomicAdd(grad_value + o10 + c, ly * hx * ga);
                if (k11) atomicAdd(grad_value + o11 + c, ly * lx * ga);
                g_a += gc * (hy * hx * v00 + hy * lx * v01 + ly * hx * v10 + ly * lx * v11);
                g_x += ga * (hy * (v01 - v00) + ly * (v11 - v10));
                g_y += ga * (hx * (v10 - v00) + lx * (v11 - v01));
            }
            g_x *= (float)w;
            g_y *= (float)h;
        }
        grad_attn[k] = g_a;
        grad_loc[2 * k] = g_x;
        grad_loc[2 * k + 1] = g_y;
    }
}

}  // namespace rdetr

using namespace rdetr;

// ---- host pipeline: one grid rule, one deterministic-workspace layout, one sort + segment-sum tail -----------------------------
namespace {
// one block = one head x 2*kBWaves queries; false: more blocks than a grid dimension holds
bool bwd_grid(int B, int Nq, int &tiles, int &nblk)
{
    tiles = (Nq + 2 * kBWaves - 1) / (2 * kBWaves);
    const long long n = (long long)B * kBH * tiles;
    nblk = (int)n;
    return n <= 0x7fffffffll;
}

struct DetLayout {
    long long nrec, nrows;
    size_t off_key, off_id, off_w, off_skey, off_sid, off_tmp, tmp_bytes, total;
    int key_bits;
};
// workspace = rec_key | rec_id | rec_w | sorted_key | sorted_id | radix-sort temporary storage (sizes from hipCUB itself: a
// host-side query, nothing is launched)
bool det_layout(int B, int S, int L, int Nq, DetLayout &d)
{
    d.nrec = (long long)B * Nq * kBH * L * kBP * 4;
    d.nrows = (long long)B * S * kBH;
    if (d.nrec >= (1ll << 31) || d.nrows >= 0xffffffffll) return false;
    d.key_bits = 32;                                                            // the all-ones "no row" key needs every bit
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t n4 = up((size_t)d.nrec * 4);
    d.off_key = 0; d.off_id = n4; d.off_w = 2 * n4; d.off_skey = 3 * n4; d.off_sid = 4 * n4; d.off_tmp = 5 * n4;
    d.tmp_bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, d.tmp_bytes, (const unsigned *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr,
                                           (unsigned *)nullptr, (int)d.nrec, 0, d.key_bits, (hipStream_t)0) != hipSuccess)
        return false;
    d.total = d.off_tmp + up(d.tmp_bytes);
    return true;
}

struct DetPtrs {
    unsigned *rec_key, *rec_id;
    float *rec_w;
    unsigned *skey, *sid;
    void *tmp;
};
DetPtrs det_pointers(void *workspace, const DetLayout &d)
{
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    return DetPtrs{reinterpret_cast<unsigned *>(ws + d.off_key), reinterpret_cast<unsigned *>(ws + d.off_id),
                   reinterpret_cast<float *>(ws + d.off_w), reinterpret_cast<unsigned *>(ws + d.off_skey),
                   reinterpret_cast<unsigned *>(ws + d.off_sid), ws + d.off_tmp};
}

// Deterministic mode after the records are written: sort them by key, then every row of grad_value = the sum of its records.
// No records (nrec == 0): nothing to sort, every row is zero.
template <typename G>
int det_sort_and_sum(const DetLayout &d, const DetPtrs &p, const G *grad_out, int L, float *grad_value, hipStream_t st)
{
    size_t tmp = d.tmp_bytes;
    if (d.nrec > 0 && hipcub::DeviceRadixSort::SortPairs(p.tmp, tmp, p.rec_key, p.skey, p.rec_id, p.sid, (int)d.nrec, 0, d.key_bits, st) != hipSuccess)
        return RDETR_ERR_LAUNCH;
    hipLaunchKernelGGL(msda_bwd_segment_sum_kernel<G>, dim3((unsigned)((d.nrows + 7) / 8)), dim3(256), 0, st, p.skey, p.sid, p.rec_w, grad_out,
                       d.nrec, d.nrows, L * kBP, grad_value);
    return launch_status();
}

// what both materialised entries need of their operands besides grad_value: every pointer present ...
bool wave_operands_present(const void *value, const void *shapes, const void *level_start, const void *loc, const void *attn,
                           const void *grad_out, const void *grad_loc, const void *grad_attn)
{
    return value && shapes && level_start && loc && attn && grad_out && grad_loc && grad_attn;
}
// ... and, for msda_bwd_wave_kernel, the alignment of its vector accesses and a plane within a buffer descriptor's 2 GiB
bool wave_operands_fit(const void *value, const void *grad_out, const void *grad_value, const void *loc, const void *grad_loc, int S)
{
    return aligned_to(value, 16) && aligned_to(grad_out, 16) && aligned_to(grad_value, 16) && aligned_to(loc, 8) &&
           aligned_to(grad_loc, 8) && (long long)S * kBPixelBytes < (1ll << 31);
}
}  // namespace

extern "C" int rdetr_msda_backward_f32(const float *value, const int64_t *spatial_shapes,
                                       const int64_t *level_start_index, const float *sampling_loc,
                                       const float *attn_weight, const float *grad_out, int B, int S, int H, int D,
                                       int L, int Nq, int P, float *grad_value, float *grad_sampling_loc,
                                       float *grad_attn_weight, void *stream)
{
    if (B < 0 || S < 0 || Nq < 0 || H <= 0 || D <= 0 || L <= 0 || P <= 0) return RDETR_ERR_INVALID_ARG;
    if (B == 0 || Nq == 0) return RDETR_OK;
    if (!wave_operands_present(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, grad_sampling_loc,
                               grad_attn_weight) || !grad_value || S == 0)
        return RDETR_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (H == kBH && D == kBD && P == kBP && L <= kBMaxL && wave_operands_fit(value, grad_out, grad_value, sampling_loc, grad_sampling_loc, S)) {
        int tiles, nblk;
        if (!bwd_grid(B, Nq, tiles, nblk)) return RDETR_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(msda_bwd_wave_kernel<false>, dim3((unsigned)nblk), dim3(kBWaves * kWave), 0, st, value,
                           spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, S, L, Nq, tiles,
                           nblk, grad_value, grad_sampling_loc, grad_attn_weight, nullptr, nullptr, nullptr);
        return launch_status();
    }
    const long long total = (long long)B * Nq * H * L * P;
    const long long want = (total + 255) / 256;
    hipLaunchKernelGGL(msda_bwd_generic_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, st, value,
                       spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, S, H, D, L, Nq, P, total,
                       grad_value, grad_sampling_loc, grad_attn_weight);
    return launch_status();
}

// ---- deterministic mode --------------------------------------------------------------------------------------------------------
extern "C" long long rdetr_msda_backward_det_workspace_bytes(int B, int S, int H, int D, int L, int Nq, int P)
{
    if (B <= 0 || S <= 0 || Nq <= 0 || H != kBH || D != kBD || P != kBP || L <= 0 || L > kBMaxL) return 0;
    DetLayout d;
    return det_layout(B, S, L, Nq, d) ? (long long)d.total : -1;
}

extern "C" int rdetr_msda_backward_det_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                           const float *sampling_loc, const float *attn_weight, const float *grad_out, int B, int S,
                                           int H, int D, int L, int Nq, int P, void *workspace, long long workspace_bytes,
                                           float *grad_value, float *grad_sampling_loc, float *grad_attn_weight, void *stream)
{
    if (B < 0 || S < 0 || Nq < 0 || H <= 0 || D <= 0 || L <= 0 || P <= 0) return RDETR_ERR_INVALID_ARG;
    if (H != kBH || D != kBD || P != kBP || L > kBMaxL) return RDETR_ERR_UNSUPPORTED;
    if (!grad_value) return RDETR_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (B == 0 || S == 0) return RDETR_OK;
    if (Nq == 0) {                                                              // no records: every row of grad_value is zero
        DetLayout none{};
        none.nrows = (long long)B * S * kBH;
        return det_sort_and_sum<float>(none, DetPtrs{}, nullptr, L, grad_value, st);
    }
    if (!wave_operands_present(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, grad_sampling_loc,
                               grad_attn_weight) || !workspace)
        return RDETR_ERR_INVALID_ARG;
    if (!wave_operands_fit(value, grad_out, grad_value, sampling_loc, grad_sampling_loc, S) || !aligned_to(workspace, 16))
        return RDETR_ERR_UNSUPPORTED;
    DetLayout d;
    if (!det_layout(B, S, L, Nq, d)) return RDETR_ERR_UNSUPPORTED;
    if (workspace_bytes < (long long)d.total) return RDETR_ERR_INVALID_ARG;
    const DetPtrs p = det_pointers(workspace, d);
    int tiles, nblk;
    if (!bwd_grid(B, Nq, tiles, nblk)) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(msda_bwd_wave_kernel<true>, dim3((unsigned)nblk), dim3(kBWaves * kWave), 0, st, value, spatial_shapes,
                       level_start_index, sampling_loc, attn_weight, grad_out, S, L, Nq, tiles, nblk, grad_value, grad_sampling_loc,
                       grad_attn_weight, p.rec_key, p.rec_id, p.rec_w);
    if (launch_status() != RDETR_OK) return RDETR_ERR_LAUNCH;
    return det_sort_and_sum(d, p, grad_out, L, grad_value, st);
}

// ---- fused-producer backward ---------------------------------------------------------------------------------------------------
// HM: head-major value / grad_value and row strides (elements, 0 = dense) for the producer inputs and their gradients
template <typename T, bool HM = false>
static int msda_backward_fused(const T *value, const int64_t *shapes, const int64_t *level_start, const T *offsets, const T *logits,
                               const float *ref, int ref_dim, const T *grad_out, int B, int S, int H, int D, int L, int Nq, int P,
                               void *workspace, long long workspace_bytes, float *grad_value, T *grad_offsets, T *grad_logits,
                               float *grad_ref_partial, hipStream_t st, int ld_off = 0, int ld_lg = 0, int ld_goff = 0, int ld_glg = 0)
{
    if (B < 0 || S < 0 || Nq < 0 || H <= 0 || D <= 0 || L <= 0 || P <= 0 || workspace_bytes < 0) return RDETR_ERR_INVALID_ARG;
    if (ref_dim != 2 && ref_dim != 4) return RDETR_ERR_INVALID_ARG;
    if constexpr (HM) {
        const long long n_lg = (long long)H * L * P;
        auto bad = [](int ld, long long n) { return ld < 0 || (ld && ld < n); };
        if (bad(ld_off, 2 * n_lg) || bad(ld_lg, n_lg) || bad(ld_goff, 2 * n_lg) || bad(ld_glg, n_lg) || ld_off % 2 || ld_goff % 2)
            return RDETR_ERR_INVALID_ARG;
        if (!ld_off) ld_off = (int)(2 * n_lg);
        if (!ld_lg) ld_lg = (int)n_lg;
        if (!ld_goff) ld_goff = (int)(2 * n_lg);
        if (!ld_glg) ld_glg = (int)n_lg;
    }
    if (B == 0 || Nq == 0) return RDETR_OK;
    if (!value || !shapes || !level_start || !offsets || !logits || !ref || !grad_out || !grad_value || !grad_offsets || !grad_logits ||
        S == 0)
        return RDETR_ERR_INVALID_ARG;
    if (H != kBH || D != kBD || P != kBP || L > kBMaxL) return RDETR_ERR_UNSUPPORTED;
    if (!(aligned_to(value, 16) && aligned_to(grad_value, 16) && aligned_to(grad_out, sizeof(T)) && aligned_to(offsets, 2 * sizeof(T)) &&
          aligned_to(logits, sizeof(T)) && aligned_to(grad_offsets, 2 * sizeof(T)) && aligned_to(grad_logits, sizeof(T)) &&
          aligned_to(ref, 16) && aligned_to(grad_ref_partial, 16) && aligned_to(workspace, 16)))
        return HM ? RDETR_ERR_UNSUPPORTED : RDETR_ERR_INVALID_ARG;
    if ((long long)S * (HM ? kBHeadBytes : kBPixelBytes) >= (1ll << 31)) return RDETR_ERR_UNSUPPORTED;
    int tiles, nblk;
    if (!bwd_grid(B, Nq, tiles, nblk)) return RDETR_ERR_UNSUPPORTED;
    if (!workspace) {
        hipLaunchKernelGGL((msda_bwd_fused_kernel<T, false, HM>), dim3((unsigned)nblk), dim3(kBWaves * kWave), 0, st, value, shapes,
                           level_start, offsets, logits, ref, ref_dim, grad_out, S, L, Nq, tiles, nblk, grad_value, grad_offsets,
                           grad_logits, grad_ref_partial, nullptr, nullptr, nullptr, ld_off, ld_lg, ld_goff, ld_glg);
        return launch_status();
    }
    // deterministic mode: the workspace of rdetr_msda_backward_det_f32 (same record count).  Records + sorted copies are 20 bytes
    // per sample corner: a workspace below that is refused before hipCUB is asked for its temporary storage
    const long long ncorner = (long long)B * Nq * kBH * L * kBP * 4;
    if (ncorner >= (1ll << 31)) return RDETR_ERR_UNSUPPORTED;
    if (workspace_bytes < ncorner * 20) return RDETR_ERR_INVALID_ARG;
    DetLayout d;
    if (!det_layout(B, S, L, Nq, d)) return RDETR_ERR_UNSUPPORTED;
    if (workspace_bytes < (long long)d.total) return RDETR_ERR_INVALID_ARG;
    const DetPtrs p = det_pointers(workspace, d);
    hipLaunchKernelGGL((msda_bwd_fused_kernel<T, true, HM>), dim3((unsigned)nblk), dim3(kBWaves * kWave), 0, st, value, shapes, level_start,
                       offsets, logits, ref, ref_dim, grad_out, S, L, Nq, tiles, nblk, grad_value, grad_offsets, grad_logits,
                       grad_ref_partial, p.rec_key, p.rec_id, p.rec_w, ld_off, ld_lg, ld_goff, ld_glg);
    if (launch_status() != RDETR_OK) return RDETR_ERR_LAUNCH;
    return det_sort_and_sum(d, p, grad_out, L, grad_value, st);
}

extern "C" int rdetr_msda_backward_fused_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                             const float *sampling_offsets, const float *attn_logits, const float *reference_points,
                                             int ref_dim, const float *grad_out, int B, int S, int H, int D, int L, int Nq, int P,
                                             void *workspace, long long workspace_bytes, float *grad_value, float *grad_offsets,
                                             float *grad_logits, float *grad_ref_partial, void *stream)
{
    return msda_backward_fused<float>(value, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points, ref_dim,
                                      grad_out, B, S, H, D, L, Nq, P, workspace, workspace_bytes, grad_value, grad_offsets, grad_logits,
                                      grad_ref_partial, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_msda_backward_fused_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                              const uint16_t *sampling_offsets, const uint16_t *attn_logits, const float *reference_points,
                                              int ref_dim, const uint16_t *grad_out, int B, int S, int H, int D, int L, int Nq, int P,
                                              void *workspace, long long workspace_bytes, float *grad_value, uint16_t *grad_offsets,
                                              uint16_t *grad_logits, float *grad_ref_partial, void *stream)
{
    return msda_backward_fused<uint16_t>(value, spatial_shapes, level_start_index, sampling_offsets, attn_logits, reference_points,
                                         ref_dim, grad_out, B, S, H, D, L, Nq, P, workspace, workspace_bytes, grad_value, grad_offsets,
                                         grad_logits, grad_ref_partial, static_cast<hipStream_t>(stream));
}

extern "C" int rdetr_msda_backward_fused_hm_bf16(const uint16_t *value_bhsd, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                                 const uint16_t *sampling_offsets, int ld_offsets, const uint16_t *attn_logits,
                                                 int ld_logits, const float *reference_points, int ref_dim, const uint16_t *grad_out,
                                                 int B, int S, int H, int D, int L, int Nq, int P, void *workspace,
                                                 long long workspace_bytes, float *grad_value_bhsd, uint16_t *grad_offsets,
                                                 int ld_grad_offsets, uint16_t *grad_logits, int ld_grad_logits, float *grad_ref_partial,
                                                 void *stream)
{
    return msda_backward_fused<uint16_t, true>(value_bhsd, spatial_shapes, level_start_index, sampling_offsets, attn_logits,
                                               reference_points, ref_dim, grad_out, B, S, H, D, L, Nq, P, workspace, workspace_bytes,
                                               grad_value_bhsd, grad_offsets, grad_logits, grad_ref_partial,
                                               static_cast<hipStream_t>(stream), ld_offsets, ld_logits, ld_grad_offsets, ld_grad_logits);
}
