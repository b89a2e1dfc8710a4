// The optimizer step of the reference's training loop (util/engine.py:57-61): clip_grad_norm_ and AdamW over the whole parameter
// set in three launches, whatever the tensor count.  One table in device memory drives all of them: per tensor the addresses and
// the step's scalars, and a chunk map that sends chunk c to (tensor, first element); a chunk never crosses a tensor.
//
//   grad_sqnorm_kernel   one fp32 partial sum of squares per chunk
//   clip_coef_kernel     one workgroup: the partials added in index order in fp64 -> {total_norm, coef}
//   adamw_step_kernel    g = grad * coef, decoupled decay, both moments, the bias-corrected update; the gradient is only read
//
// No atomics: a chunk belongs to one workgroup whatever the grid, every sum has a fixed order, so the bits repeat from run to run.
// The arithmetic is torch's single-tensor AdamW (torch/optim/adam.py, _single_tensor_adam) element by element in fp32, under the
// makefile's -ffp-contract=off and HIP's correctly rounded division and square root.
#include "launch.h"

namespace rdetr {
namespace {

constexpr int kOptThreads = 256;
constexpr int kOptWaves = kOptThreads / kWave;
constexpr int kOptGridCap = 8 * kCus;        // 8 workgroups per CU: the grid walks the chunks with this stride beyond it
constexpr int kCoefThreads = 256;

static_assert(sizeof(rdetr_optim_tensor) == 40 && sizeof(rdetr_optim_step) == 40 && sizeof(rdetr_optim_chunk) == 16, "table layout");

struct ChunkView {
    long long first;                         // element offset of the chunk in its tensor
    int n;                                   // elements of the chunk, 0: nothing to do
    int t;                                   // tensor
};

// chunk c of the map, or n = 0 for an entry that names no tensor or lies outside its tensor
__device__ __forceinline__ ChunkView chunk_view(const rdetr_optim_tensor *__restrict__ tensors, const rdetr_optim_chunk *__restrict__ map,
                                                int c, int n_tensors, int chunk)
{
    ChunkView cv;
    cv.first = map[c].first;
    cv.t = map[c].tensor;
    cv.n = 0;
    if (cv.t < 0 || cv.t >= n_tensors || cv.first < 0) return cv;
    const long long left = tensors[cv.t].numel - cv.first;
    cv.n = left <= 0 ? 0 : (left < chunk ? (int)left : chunk);
    return cv;
}

__device__ __forceinline__ bool is_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__global__ __launch_bounds__(kOptThreads) void grad_sqnorm_kernel(const rdetr_optim_tensor *__restrict__ tensors,
                                                                 const rdetr_optim_step *__restrict__ steps,
                                                                 const rdetr_optim_chunk *__restrict__ map, int n_tensors, int n_chunks,
                                                                 int chunk, float *__restrict__ partials)
{
    __shared__ float s_red[kOptWaves];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ChunkView cv = chunk_view(tensors, map, c, n_tensors, chunk);
        const float *g = cv.n > 0 ? static_cast<const float *>(steps[cv.t].grad) : nullptr;
        if (g == nullptr) {                                                    // no gradient: the tensor is skipped
            if (tid == 0) partials[c] = 0.0f;
            continue;
        }
        g += cv.first;
        // per-lane chains, one per vector component, in element order
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        if (is_aligned16(g)) {
            const int nvec = cv.n >> 2;
            const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
            for (int i = tid; i < nvec; i += kOptThreads) {
                const f32x4 x = g4[i];
                a0 += x[0] * x[0];
                a1 += x[1] * x[1];
                a2 += x[2] * x[2];
                a3 += x[3] * x[3];
            }
            const int i = (nvec << 2) + tid;                                   // the numel % 4 tail
            if (i < cv.n) a0 += g[i] * g[i];
        } else {
            for (int i = tid; i < cv.n; i += kOptThreads) a0 += g[i] * g[i];
        }
        float v = (a0 + a1) + (a2 + a3);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
        if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = v;
        __syncthreads();
        if (tid == 0) {
            float s = s_red[0];
#pragma unroll
            for (int w = 1; w < kOptWaves; ++w) s += s_red[w];
            partials[c] = s;
        }
        __syncthreads();                                                       // s_red is reused by the next chunk
    }
}

// out = {total_norm, min(1, max_norm / (total_norm + 1e-6))}: clip_grad_norm_'s coefficient.  Thread t adds a contiguous run of the
// partials in index order, thread 0 then adds the runs in index order, all in fp64.  A NaN norm gives a NaN coefficient, as in torch.
__global__ __launch_bounds__(kCoefThreads) void clip_coef_kernel(const float *__restrict__ partials, int n_chunks, float max_norm,
                                                                 float *__restrict__ out)
{
    __shared__ double s_run[kCoefThreads];
    const int tid = threadIdx.x;
    const int per = (n_chunks + kCoefThreads - 1) / kCoefThreads;
    const int lo = tid * per, hi = min(n_chunks, lo + per);
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += (double)partials[i];
    s_run[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int t = 0; t < kCoefThreads; ++t) total += s_run[t];
        const float norm = (float)sqrt(total);
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.0f ? 1.0f : c;
    }
}

struct Moments {
    float p, m, v;
};

// torch's single-tensor AdamW on one element: param.mul_(1 - lr * wd); exp_avg.lerp_(g, 1 - beta1);
// exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2); param.addcdiv_(exp_avg, sqrt(exp_avg_sq) / sqrt(bc2) + eps, value=-lr / bc1)
__device__ __forceinline__ Moments adamw_element(float g, float p, float m, float v, float coef, const rdetr_optim_step &s)
{
    g = g * coef;
    Moments r;
    p = p * s.decay;
    r.m = m + s.one_minus_beta1 * (g - m);
    r.v = v * s.beta2 + (s.one_minus_beta2 * g) * g;
    const float denom = sqrtf(r.v) / s.bias2_sqrt + s.eps;
    r.p = p - s.step_size * (r.m / denom);
    return r;
}

__global__ __launch_bounds__(kOptThreads) void adamw_step_kernel(const rdetr_optim_tensor *__restrict__ tensors,
                                                                const rdetr_optim_step *__restrict__ steps,
                                                                const rdetr_optim_chunk *__restrict__ map, int n_tensors, int n_chunks,
                                                                int chunk, const float *__restrict__ norm_coef)
{
    const int tid = threadIdx.x;
    const float coef = norm_coef ? norm_coef[1] : 1.0f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ChunkView cv = chunk_view(tensors, map, c, n_tensors, chunk);
        if (cv.n <= 0) continue;
        const rdetr_optim_step s = steps[cv.t];
        const rdetr_optim_tensor tt = tensors[cv.t];
        if (s.grad == nullptr || !tt.param || !tt.exp_avg || !tt.exp_avg_sq) continue;
        const float *g = static_cast<const float *>(s.grad) + cv.first;
        float *p = static_cast<float *>(tt.param) + cv.first;
        float *m = static_cast<float *>(tt.exp_avg) + cv.first;
        float *v = static_cast<float *>(tt.exp_avg_sq) + cv.first;
        if (tt.aligned16 && is_aligned16(g) && is_aligned16(p) && is_aligned16(m) && is_aligned16(v)) {
            const int nvec = cv.n >> 2;
            const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
            f32x4 *p4 = reinterpret_cast<f32x4 *>(p), *m4 = reinterpret_cast<f32x4 *>(m), *v4 = reinterpret_cast<f32x4 *>(v);
            for (int i = tid; i < nvec; i += kOptThreads) {
                const f32x4 gx = g4[i];
                f32x4 px = p4[i], mx = m4[i], vx = v4[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const Moments r = adamw_element(gx[j], px[j], mx[j], vx[j], coef, s);
                    px[j] = r.p;
                    mx[j] = r.m;
                    vx[j] = r.v;
                }
                p4[i] = px;
                m4[i] = mx;
                v4[i] = vx;
            }
            const int i = (nvec << 2) + tid;                                   // the numel % 4 tail
            if (i < cv.n) {
                const Moments r = adamw_element(g[i], p[i], m[i], v[i], coef, s);
                p[i] = r.p;
                m[i] = r.m;
                v[i] = r.v;
            }
        } else {
            for (int i = tid; i < cv.n; i += kOptThreads) {
                const Moments r = adamw_element(g[i], p[i], m[i], v[i], coef, s);
                p[i] = r.p;
                m[i] = r.m;
                v[i] = r.v;
            }
        }
    }
}

long long optim_workspace(int chunks) { return chunks <= 0 ? 0 : ((long long)chunks + 2) * (long long)sizeof(float); }

// what the two table-driven launches share: RDETR_OK with *grid set, or the refusal
int table_args(const void *tensors, const void *steps, const void *map, int n_tensors, int n_chunks, int chunk, int max_blocks, unsigned *grid)
{
    if (n_tensors < 0 || n_chunks < 0 || chunk <= 0) return RDETR_ERR_INVALID_ARG;
    if (n_chunks == 0) return RDETR_OK;
    if (!tensors || !steps || !map || n_tensors == 0) return RDETR_ERR_INVALID_ARG;
    if (chunk % 4) return RDETR_ERR_UNSUPPORTED;                               // a chunk starts on a 16-byte boundary of its tensor
    if (!aligned_to(tensors, 8) || !aligned_to(steps, 8) || !aligned_to(map, 8)) return RDETR_ERR_UNSUPPORTED;
    const int cap = max_blocks > 0 ? max_blocks : kOptGridCap;
    *grid = (unsigned)(n_chunks < cap ? n_chunks : cap);
    return RDETR_OK;
}

}  // namespace
}  // namespace rdetr

extern "C" {

long long rdetr_optim_workspace_bytes(int chunks) { return rdetr::optim_workspace(chunks); }

int rdetr_grad_sqnorm_f32(const rdetr_optim_tensor *tensors, const rdetr_optim_step *steps, const rdetr_optim_chunk *chunk_map, int n_tensors,
                          int n_chunks, int chunk, int max_blocks, void *ws, long long ws_bytes, void *stream)
{
    using namespace rdetr;
    unsigned grid = 0;
    const int st = table_args(tensors, steps, chunk_map, n_tensors, n_chunks, chunk, max_blocks, &grid);
    if (st != RDETR_OK || n_chunks == 0) return st;
    if (!ws || ws_bytes < optim_workspace(n_chunks)) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(ws, 4)) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), tensors, steps, chunk_map,
                       n_tensors, n_chunks, chunk, static_cast<float *>(ws));
    return launch_status();
}

int rdetr_grad_clip_coef(void *ws, long long ws_bytes, int n_chunks, float max_norm, void *stream)
{
    using namespace rdetr;
    if (n_chunks < 0 || !ws || ws_bytes < (long long)(2 * sizeof(float)) || ws_bytes < optim_workspace(n_chunks)) return RDETR_ERR_INVALID_ARG;
    if (!aligned_to(ws, 4)) return RDETR_ERR_UNSUPPORTED;
    float *partials = static_cast<float *>(ws);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(kCoefThreads), 0, static_cast<hipStream_t>(stream), partials, n_chunks, max_norm,
                       partials + n_chunks);
    return launch_status();
}

int rdetr_adamw_step_f32(const rdetr_optim_tensor *tensors, const rdetr_optim_step *steps, const rdetr_optim_chunk *chunk_map, int n_tensors,
                         int n_chunks, int chunk, int max_blocks, const float *norm_coef, void *stream)
{
    using namespace rdetr;
    unsigned grid = 0;
    const int st = table_args(tensors, steps, chunk_map, n_tensors, n_chunks, chunk, max_blocks, &grid);
    if (st != RDETR_OK || n_chunks == 0) return st;
    if (norm_coef && !aligned_to(norm_coef, 4)) return RDETR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(adamw_step_kernel, dim3(grid), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), tensors, steps, chunk_map,
                       n_tensors, n_chunks, chunk, norm_coef);
    return launch_status();
}

}  // extern "C"
