// Swin's shifted-window attention between the qkv and the proj GEMM, fused: one launch per block (gfx950).
//
// Replaces the chain around softmax(Q K^T * scale + bias) V of models/backbones/swin.py:133-221 -- zero-pad to a window
// multiple, torch.roll, window partition, the qkv permute, q * scale, the [B*nW, heads, N, N] scores, + relative position bias,
// + the shift mask, softmax, P V, transpose, window reverse, roll back, unpad + contiguous -- by one kernel that reads q, k, v
// where the qkv GEMM of the UNPADDED map left them and writes the result at the token's own row, as the proj GEMM reads it.
//
//   geometry  = pH = ceil(H / wh) wh, pW likewise.  Window (wy, wx) of the rolled frame holds the positions (y, x) = (wy wh + ri,
//               wx ww + ci); position (y, x) is the token of source position ((y + sh) % pH, (x + sw) % pW).  A source position
//               outside H x W is a PADDING token: the reference pads before the qkv linear, so its k / v are the linear's bias row
//               (k_pad / v_pad; zeros when null).  Padding tokens TAKE PART AS KEYS -- nothing masks them -- and their own outputs
//               are not stored.  That is not the key-tail rule of attn_common.h: only the rows N = wh ww .. of the last 64-key
//               chunk are excluded (-inf).
//   bias      = table[(ri - rj + wh - 1) (2 ww - 1) + (ci - cj + ww - 1), head], index arithmetic here: the head's column of the
//               table goes to LDS once per workgroup (times log2 e), a key's  rj (2 ww - 1) + cj  and region id once per key
//   mask      = when sh + sw > 0: -100 (not -inf) between tokens of different regions; region = 3 hr + wr on rolled-frame
//               coordinates, hr = 0 below pH - wh, 1 below pH - sh, else 2 (a dimension without shift is split at a window
//               boundary only, which no window sees)
//   workgroup = one (image, window, head): 4 waves.  The window's K and V rows (N <= 192: kChunks chunks of 64 keys) are staged once
//               in LDS by all four waves, 16 bytes per lane and row piece; wave w then takes the 16-query tiles w, w + 4, ... on
//               its own (no further workgroup barrier).  At N = 49 that is one tile per wave and 11 KiB of K / V: eight workgroups
//               fit a CU, the wave limit.  Heads run fastest in the logical block id and the id is made XCD-contiguous, so the
//               heads that share a token row's cache lines meet in one L2.
//   MFMA      = v_mfma_f32_16x16x32_bf16 with the transposed products and the lane layout of csrc/attn.hip: lane (q = lane & 15,
//               g = lane >> 4) holds keys 16 kb + 4 g + r of ITS query, so a row's soft-max statistics sit in 4 lanes.
//   softmax   = all of a row's logits are in registers (at most 3 chunks): one maximum, one sum, fp32; P rounded to bf16 for the
//               P V product, fp32 accumulation, as attn.hip does.
//   store     = a wave's 16 x 32 tile goes through a wave-private LDS image so that every lane stores 16 bytes of one token row.
// Forward only.
#include "attn_common.h"

namespace rdetr {

constexpr int kWinD = 32;                          // head dim
constexpr int kWinTileQ = 16, kWinChunk = 64, kWinWaves = 4;
constexpr int kWinKS = 80, kWinVS = 96;            // LDS row strides in bytes, as attn.hip
constexpr int kWinOS = 80;                         // the output tile's
constexpr int kWinMaxN = 144;                      // keys of a window: three chunks
constexpr int kWinTable = 576;                     // (2 wh - 1)(2 ww - 1) <= (2 sqrt(144) - 1)^2 = 529 entries
constexpr float kWinMask = -100.0f;

struct WinGeom {
    int H, W, wh, ww, sh, sw, pH, pW, nwx, nwin;   // nwin = windows of one image
};

// source row of window token r (< N) of window (wy, wx): the token's index in [0, H W), or -1 for a padding token; its region id
__device__ __forceinline__ int win_source(const WinGeom &g, int wy, int wx, int r, int &region)
{
    const int ri = r / g.ww, ci = r - ri * g.ww;
    const int y = wy * g.wh + ri, x = wx * g.ww + ci;
    const int hr = y < g.pH - g.wh ? 0 : (y < g.pH - g.sh ? 1 : 2), wr = x < g.pW - g.ww ? 0 : (x < g.pW - g.sw ? 1 : 2);
    region = 3 * hr + wr;
    int sy = y + g.sh, sx = x + g.sw;
    if (sy >= g.pH) sy -= g.pH;
    if (sx >= g.pW) sx -= g.pW;
    return (sy < g.H && sx < g.W) ? sy * g.W + sx : -1;
}

template <int kChunks, bool kTableBf16>
__global__ __launch_bounds__(kWinWaves *kWave) void window_attention_kernel(
    const uint16_t *__restrict__ q, const uint16_t *__restrict__ k, const uint16_t *__restrict__ v, int ldq, int ldk, int ldv,
    const uint16_t *__restrict__ k_pad, const uint16_t *__restrict__ v_pad, const void *__restrict__ table, int heads, WinGeom geo,
    float scale_log2e, uint16_t *__restrict__ out, int ldo, int nblk)
{
    constexpr int kRows = kChunks * kWinChunk;
    __shared__ __attribute__((aligned(16))) unsigned char lds_k[kRows * kWinKS];
    __shared__ __attribute__((aligned(16))) unsigned char lds_v[kRows * kWinVS];
    __shared__ __attribute__((aligned(16))) unsigned char lds_o[kWinWaves * kWinTileQ * kWinOS];
    __shared__ __attribute__((aligned(16))) int key_code[kRows];          // rj (2 ww - 1) + cj | region << 16
    __shared__ float tab[kWinTable];                                      // the head's column of the table, times log2 e

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    const int id = xcd_contiguous_block(blockIdx.x, nblk);
    const int h = id % heads, bw = id / heads, b = bw / geo.nwin, win = bw - b * geo.nwin;
    const int wy = win / geo.nwx, wx = win - wy * geo.nwx;
    const int N = geo.wh * geo.ww, span = 2 * geo.ww - 1, T = (2 * geo.wh - 1) * span;
    const bool shifted = geo.sh + geo.sw > 0;
    const size_t image = (size_t)b * geo.H * geo.W;

    // ---- stage: the table column, every key's code, the window's K and V rows (padding tokens: the pad row; rows N..: zeros)
    for (int i = tid; i < T; i += kWinWaves * kWave) {
        float t;
        if constexpr (kTableBf16)
            t = bf16_bits_to_f32(reinterpret_cast<const uint16_t *>(table)[(size_t)i * heads + h]);
        else
            t = reinterpret_cast<const float *>(table)[(size_t)i * heads + h];
        tab[i] = t * kLog2e;
    }
    const uint16_t *kpad = k_pad ? k_pad + h * kWinD : nullptr, *vpad = v_pad ? v_pad + h * kWinD : nullptr;
    u32x4 kr[kChunks], vr[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int idx = tid + c * kWinWaves * kWave, row = idx >> 2, piece = idx & 3;
        kr[c] = u32x4{0, 0, 0, 0};
        vr[c] = u32x4{0, 0, 0, 0};
        int code = 0;
        if (row < N) {
            int region;
            const int src = win_source(geo, wy, wx, row, region);
            const int rj = row / geo.ww, cj = row - rj * geo.ww;
            code = (rj * span + cj) | (region << 16);
            const uint16_t *kp = src >= 0 ? k + (image + src) * ldk + h * kWinD : kpad;
            const uint16_t *vp = src >= 0 ? v + (image + src) * ldv + h * kWinD : vpad;
            if (kp) kr[c] = *reinterpret_cast<const u32x4 *>(kp + piece * 8);
            if (vp) vr[c] = *reinterpret_cast<const u32x4 *>(vp + piece * 8);
        }
        if (piece == 0) key_code[row] = code;
    }
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const int idx = tid + c * kWinWaves * kWave, row = idx >> 2, piece = idx & 3;
        *reinterpret_cast<u32x4 *>(lds_k + row * kWinKS + piece * 16) = kr[c];
        *reinterpret_cast<u32x4 *>(lds_v + row * kWinVS + piece * 16) = vr[c];
    }
    __syncthreads();

    // ---- the wave's query tiles
    unsigned char *my_o = lds_o + wave * kWinTileQ * kWinOS;
    const int tiles = (N + kWinTileQ - 1) / kWinTileQ;
    for (int tile = wave; tile < tiles; tile += kWinWaves) {               // uniform per wave
        // the lane's query: row qr of the window (clamped: a row past N computes, and stores nothing)
        const int qr = min(tile * kWinTileQ + ql, N - 1);
        int qregion;
        const int qsrc = win_source(geo, wy, wx, qr, qregion);
        const int qi = qr / geo.ww, qcode = qi * span + (qr - qi * geo.ww) + (geo.wh - 1) * span + geo.ww - 1;
        u32x4 qfrag = {0, 0, 0, 0};                                       // B operand of the S^T product, B[k = d = 8 g + j][col = q]
        if (qsrc >= 0) qfrag = *reinterpret_cast<const u32x4 *>(q + (image + qsrc) * ldq + h * kWinD + g * 8);

        // S^T = K Q^T, logits in the log2 domain: (s * scale + bias + mask) * log2(e)
        f32x4 s[kChunks][4];
        float m = -__builtin_inff();
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const int key = c * kWinChunk + 16 * kb + 4 * g;          // this lane's keys key .. key + 3
                const u32x4 kf = *reinterpret_cast<const u32x4 *>(lds_k + (c * kWinChunk + 16 * kb + ql) * kWinKS + g * 16);
                const u32x4 codes = *reinterpret_cast<const u32x4 *>(key_code + key);
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
                z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(kf), as_bf16x8(qfrag), z, 0, 0, 0);
                const unsigned cd[4] = {codes.x, codes.y, codes.z, codes.w};
                float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float bias = tab[qcode - (int)(cd[r] & 0xffffu)];     // keys past N carry code 0: the index stays inside the table
                    if (shifted && (int)(cd[r] >> 16) != qregion) bias += kWinMask * kLog2e;
                    zz[r] = key + r < N ? zz[r] * scale_log2e + bias : -__builtin_inff();      // the key-tail rule
                    m = fmaxf(m, zz[r]);
                }
                s[c][kb] = f32x4{zz[0], zz[1], zz[2], zz[3]};
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));                              // finite: key 0 always takes part

        // P = exp2(z - m), bf16 for the P V product; O^T += V^T P^T
        float l = 0.f;
        f32x4 acc[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};            // O^T[d = 16 cb + 4 g + r][q]
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
#pragma unroll
            for (int pair = 0; pair < 2; ++pair) {
                float p[8];
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const f32x4 z = s[c][2 * pair + half];
                    p[4 * half + 0] = __builtin_amdgcn_exp2f(z.x - m);
                    p[4 * half + 1] = __builtin_amdgcn_exp2f(z.y - m);
                    p[4 * half + 2] = __builtin_amdgcn_exp2f(z.z - m);
                    p[4 * half + 3] = __builtin_amdgcn_exp2f(z.w - m);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) l += p[j];
                const u32x4 pf = {pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(p[4], p[5]), pack_bf16x2(p[6], p[7])};
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const u32x4 vf = tr_rows8<kWinVS>(lds_v + c * kWinChunk * kWinVS, 32 * pair, cb, lane);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(vf), as_bf16x8(pf), acc[cb], 0, 0, 0);
                }
            }
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;

        // the tile through the wave's LDS image: row ql, columns 4 g .. and 16 + 4 g ..; then 16 bytes of one token row per lane
        *reinterpret_cast<u32x2 *>(my_o + ql * kWinOS + 8 * g) =
            u32x2{pack_bf16x2(acc[0].x * inv, acc[0].y * inv), pack_bf16x2(acc[0].z * inv, acc[0].w * inv)};
        *reinterpret_cast<u32x2 *>(my_o + ql * kWinOS + 32 + 8 * g) =
            u32x2{pack_bf16x2(acc[1].x * inv, acc[1].y * inv), pack_bf16x2(acc[1].z * inv, acc[1].w * inv)};
        wave_sync();
        const int orow = lane >> 2, opiece = lane & 3, otok = tile * kWinTileQ + orow;
        if (otok < N) {
            int unused;
            const int osrc = win_source(geo, wy, wx, otok, unused);
            if (osrc >= 0)                                                // a padding token's output is not stored
                *reinterpret_cast<u32x4 *>(out + (image + osrc) * ldo + h * kWinD + opiece * 8) =
                    *reinterpret_cast<const u32x4 *>(my_o + orow * kWinOS + opiece * 16);
        }
        wave_sync();                                                      // the image is free for the wave's next tile
    }
}

template <int kChunks>
static void launch_window_attention(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                    const uint16_t *k_pad, const uint16_t *v_pad, const void *table, bool table_bf16, int heads,
                                    const WinGeom &geo, float scale, uint16_t *out, int ldo, int nblk, hipStream_t st)
{
    const float sl = scale * kLog2e;
    if (table_bf16)
        hipLaunchKernelGGL((window_attention_kernel<kChunks, true>), dim3((unsigned)nblk), dim3(kWinWaves * kWave), 0, st, q, k, v, ldq, ldk,
                           ldv, k_pad, v_pad, table, heads, geo, sl, out, ldo, nblk);
    else
        hipLaunchKernelGGL((window_attention_kernel<kChunks, false>), dim3((unsigned)nblk), dim3(kWinWaves * kWave), 0, st, q, k, v, ldq, ldk,
                           ldv, k_pad, v_pad, table, heads, geo, sl, out, ldo, nblk);
}

}  // namespace rdetr

extern "C" int rdetr_window_attention_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                           const uint16_t *k_pad, const uint16_t *v_pad, const void *table, int table_bf16, int B,
                                           int heads, int D, int H, int W, int wh, int ww, int sh, int sw, float scale,
                                           uint16_t *out, int ldo, void *stream)
{
    using namespace rdetr;
    if (B < 0 || heads <= 0 || H < 0 || W < 0 || wh < 0 || ww < 0 || sh < 0 || sw < 0) return RDETR_ERR_INVALID_ARG;
    if (table_bf16 != 0 && table_bf16 != 1) return RDETR_ERR_INVALID_ARG;
    if ((long long)wh * ww == 0) return RDETR_ERR_INVALID_ARG;
    if (D != kWinD || (long long)wh * ww > kWinMaxN) return RDETR_ERR_UNSUPPORTED;
    if (sh >= wh || sw >= ww) return RDETR_ERR_INVALID_ARG;
    if (B == 0 || H == 0 || W == 0) return RDETR_OK;
    if (!q || !k || !v || !out || !table) return RDETR_ERR_INVALID_ARG;
    const long long C = (long long)heads * kWinD;
    const int st = rows_status({{q, ldq, C, 2}, {k, ldk, C, 2}, {v, ldv, C, 2}, {out, ldo, C, 2}});
    if (st != RDETR_OK) return st;
    if (!all_aligned(16, k_pad, v_pad) || !aligned_to(table, table_bf16 ? 2 : 4)) return RDETR_ERR_UNSUPPORTED;
    WinGeom geo;
    geo.H = H, geo.W = W, geo.wh = wh, geo.ww = ww, geo.sh = sh, geo.sw = sw;
    const long long nwy = ((long long)H + wh - 1) / wh, nwx = ((long long)W + ww - 1) / ww;
    const long long nblk = (long long)B * nwy * nwx * heads;
    if (nwy * wh > 0x3fffffffll || nwx * ww > 0x3fffffffll || (long long)H * W > 0x7fffffffll || !grid_fits(nblk)) return RDETR_ERR_UNSUPPORTED;
    geo.pH = (int)(nwy * wh), geo.pW = (int)(nwx * ww), geo.nwx = (int)nwx, geo.nwin = (int)(nwy * nwx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int N = wh * ww;
    if (N <= kWinChunk)
        launch_window_attention<1>(q, k, v, ldq, ldk, ldv, k_pad, v_pad, table, table_bf16 != 0, heads, geo, scale, out, ldo, (int)nblk, s);
    else if (N <= 2 * kWinChunk)
        launch_window_attention<2>(q, k, v, ldq, ldk, ldv, k_pad, v_pad, table, table_bf16 != 0, heads, geo, scale, out, ldo, (int)nblk, s);
    else
        launch_window_attention<3>(q, k, v, ldq, ldk, ldv, k_pad, v_pad, table, table_bf16 != 0, heads, geo, scale, out, ldo, (int)nblk, s);
    return launch_status();
}
