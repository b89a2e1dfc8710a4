// The matcher's assignment on the device (models/matcher/hungarian_matcher.py:72-100, scipy.optimize.linear_sum_assignment):
//   rdetr_assign_match  solves the rectangular linear sum assignment of every row of a cost stack [R, N, Gmax] exactly and writes
//                       the match table set_loss reads, the fixed denoising matches in front of it; one launch, one workgroup a row.
// The shortest-augmenting-path method scipy runs (Crouse, "On implementing 2D rectangular assignment algorithms", 2016), in its
// arithmetic: fp64 duals and path costs over the fp32 costs, so the optimum is scipy's wherever it is unique.  Row r of a stack
// belongs to image r % B.
#include "launch.h"

#include <math.h>

namespace rdetr {
namespace {

#ifndef RDETR_ASSIGN_THREADS
#define RDETR_ASSIGN_THREADS 512               // the fastest of 128 ... 1024 at the criterion shapes (profiles/r20); a multiple of 64
#endif
constexpr int kAssignThreads = RDETR_ASSIGN_THREADS;
constexpr int kAssignWaves = kAssignThreads / kWave;
constexpr int kAssignMaxSide = 2048;           // queries, and target copies (Gmax * repeat), of one problem
constexpr int kAssignPerLane = kAssignMaxSide / kAssignThreads;        // long-side elements of one lane
constexpr int kAssignLongBytes = 28;           // per long-side element: path cost, v (fp64), predecessor, assigned row, visited
constexpr int kAssignShortBytes = 24;          // per short-side element: u, path cost when reached (fp64), assigned column, visited
constexpr int kAssigned = 1 << 30;             // key bit of a column that has a row: among equal minima a free column goes first

size_t assign_lds_bytes(int n_long, int n_short)
{
    return (size_t)n_long * kAssignLongBytes + (size_t)n_short * kAssignShortBytes;
}

// A candidate column of a search step: its path cost, its index (with kAssigned set where it has a row) and that row or -1.
struct Candidate {
    double val;
    int key, row;
};

// a <- the smaller of the two, by value and then by key: a total order, so the result is the same for any lane and wave count
__device__ __forceinline__ void take_min(Candidate &a, const Candidate &o)
{
    if (o.val < a.val || (o.val == a.val && o.key < a.key)) a = o;
}

// one DPP exchange inside the rows of 16 lanes (every lane has a source lane, so nothing is left unwritten) and the minimum
template <int kCtrl> __device__ __forceinline__ void dpp_min(Candidate &a)
{
    const int lo = __double2loint(a.val), hi = __double2hiint(a.val);
    Candidate o;
    o.val = __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, kCtrl, 0xf, 0xf, false),
                             __builtin_amdgcn_update_dpp(lo, lo, kCtrl, 0xf, 0xf, false));
    o.key = __builtin_amdgcn_update_dpp(a.key, a.key, kCtrl, 0xf, 0xf, false);
    o.row = __builtin_amdgcn_update_dpp(a.row, a.row, kCtrl, 0xf, 0xf, false);
    take_min(a, o);
}

// the wave's minimum in every lane: quad_perm [1,0,3,2] and [2,3,0,1], row_ror 4 and 8 leave each row of 16 with its own, and the
// four rows' are read from their first lanes.  No LDS round trip: this runs once per search step, on the critical path.
__device__ __forceinline__ Candidate wave_min(Candidate a)
{
    dpp_min<0xB1>(a);
    dpp_min<0x4E>(a);
    dpp_min<0x124>(a);
    dpp_min<0x128>(a);
    const int lo = __double2loint(a.val), hi = __double2hiint(a.val);
    Candidate m;
#pragma unroll
    for (int row = 0; row < kWave / 16; ++row) {
        Candidate o;
        o.val = __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * row), __builtin_amdgcn_readlane(lo, 16 * row));
        o.key = __builtin_amdgcn_readlane(a.key, 16 * row);
        o.row = __builtin_amdgcn_readlane(a.row, 16 * row);
        if (row == 0) m = o;
        else take_min(m, o);
    }
    return m;
}

// One workgroup solves one row.  The SHORT side of the problem (ns = min(N, g * repeat) elements, index s) is iterated over, one
// augmentation each; the LONG side (nl = max, index l) is what a search scans.  copies <= N: short = target copy k (gt k % g),
// long = query; otherwise short = query, long = target copy.  Element l (s) belongs to lane l (s) % kAssignThreads throughout: its
// path cost, predecessor, dual and visited flag are read and written by that lane only, but for the visit marks of the short side,
// which lane 0 sets in front of a step's barrier, and the assignment itself, which one lane flips behind a search's last one.
__global__ __launch_bounds__(kAssignThreads) void assign_match_kernel(const float *__restrict__ cost, const int *__restrict__ gt_count,
                                                                      int B, int N, int Gmax, int repeat, int skip, int dn_max_gt,
                                                                      int n_long, int n_short, int *__restrict__ match,
                                                                      long long ld_match, int *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double *s_spc = reinterpret_cast<double *>(lds_raw);                   // [n_long] shortest path cost to the column
    double *s_v = s_spc + n_long;                                          // [n_long] column dual
    double *s_u = s_v + n_long;                                            // [n_short] row dual
    double *s_reach = s_u + n_short;                                       // [n_short] path cost at which the search reached the row
    int *s_path = reinterpret_cast<int *>(s_reach + n_short);              // [n_long] the row the column was reached from
    int *s_row4col = s_path + n_long;                                      // [n_long] assigned row or -1
    int *s_sc = s_row4col + n_long;                                        // [n_long] visited in this search
    int *s_col4row = s_sc + n_long;                                        // [n_short] assigned column or -1
    int *s_sr = s_col4row + n_short;                                       // [n_short] visited in this search
    __shared__ double s_red_val[2][kAssignWaves];
    __shared__ int s_red_key[2][kAssignWaves], s_red_row[2][kAssignWaves];

    const int r = blockIdx.x, b = r % B, tid = threadIdx.x;
    const int g = min(max(gt_count[b], 0), Gmax);
    const float *row_cost = cost + (long long)r * N * Gmax;
    int *row_match = match + (long long)r * ld_match;

    // the denoising queries: group grp, slot t -> gt t
    for (int e = tid; e < skip; e += kAssignThreads) {
        const int t = e % dn_max_gt;
        row_match[e] = t < g ? t : -1;
    }
    row_match += skip;
    const int copies = g * repeat;                                         // <= kAssignMaxSide: checked by the host
    const bool by_query = copies > N;                                      // the short side is the queries
    const int ns = by_query ? N : copies, nl = by_query ? copies : N;
    if (ns == 0) {
        for (int q = tid; q < N; q += kAssignThreads) row_match[q] = -1;
        if (tid == 0) status[r] = 0;
        return;
    }

    for (int l = tid; l < nl; l += kAssignThreads) s_v[l] = 0.0, s_row4col[l] = -1, s_spc[l] = INFINITY, s_sc[l] = 0;
    for (int s = tid; s < ns; s += kAssignThreads) s_u[s] = 0.0, s_col4row[s] = -1, s_sr[s] = 0;
    __syncthreads();

    bool failed = false;
    int parity = 0;
#ifdef RDETR_DEV
    int longest = 0, steps = 0;                 // rows of the longest augmenting path, search steps in all: status bits 8-15, 16-30
#endif
    for (int cur = 0; cur < ns; ++cur) {
        // ---- the search: Dijkstra from row cur to the first column without a row; at most cur + 1 <= ns rows are visited
        int i = cur, sink = -1;
        double min_val = 0.0;
        for (int step = 0; step <= ns; ++step) {
            if (tid == 0) s_sr[i] = 1, s_reach[i] = min_val;               // = the path cost of the row's column: scipy's spc[col4row[i]]
            const double ui = s_u[i];
            const float *src = by_query ? row_cost + (long long)i * Gmax : row_cost + i % g;
            // the lane's costs and state first, all loads in flight together (the costs come through L2, a cache line a lane in
            // the usual orientation: DESIGN.md has what staging them transposed was measured to give), then the relaxations
            float c[kAssignPerLane];
            double spc[kAssignPerLane], v[kAssignPerLane];
            int seen[kAssignPerLane], row[kAssignPerLane];
            int lm = by_query ? tid % g : 0;
#pragma unroll
            for (int k = 0; k < kAssignPerLane; ++k) {
                const int l = tid + k * kAssignThreads;
                const bool live = l < nl;
                c[k] = live ? src[by_query ? lm : (long long)l * Gmax] : 0.0f;
                seen[k] = live ? s_sc[l] : 1;
                spc[k] = live ? s_spc[l] : 0.0, v[k] = live ? s_v[l] : 0.0, row[k] = live ? s_row4col[l] : 0;
                lm += kAssignThreads % g;                                  // (l + threads) % g without a division
                lm -= lm >= g ? g : 0;
            }
            Candidate best = {INFINITY, 0x7fffffff, -1};
#pragma unroll
            for (int k = 0; k < kAssignPerLane; ++k) {
                const int l = tid + k * kAssignThreads;
                if (seen[k]) continue;
                // scipy's expression, in its order; a cost that is not finite makes the minimum -inf, which ends the row below
                const double red = fabsf(c[k]) < INFINITY ? min_val + (double)c[k] - ui - v[k] : -INFINITY;
                double cost_l = spc[k];
                if (red < cost_l) {
                    cost_l = red;
                    s_spc[l] = red;
                    s_path[l] = i;
                }
                take_min(best, Candidate{cost_l, row[k] < 0 ? l : l | kAssigned, row[k]});
            }
            // arg-min of the workgroup: inside the waves in registers, then the waves through LDS (two buffers: one barrier a step)
            best = wave_min(best);
            if ((tid & (kWave - 1)) == 0) {
                s_red_val[parity][tid / kWave] = best.val;
                s_red_key[parity][tid / kWave] = best.key;
                s_red_row[parity][tid / kWave] = best.row;
            }
            __syncthreads();
            best = Candidate{s_red_val[parity][0], s_red_key[parity][0], s_red_row[parity][0]};
#pragma unroll
            for (int w = 1; w < kAssignWaves; ++w) take_min(best, Candidate{s_red_val[parity][w], s_red_key[parity][w], s_red_row[parity][w]});
            parity ^= 1;
            min_val = best.val;
#ifdef RDETR_DEV
            ++steps;
            longest = max(longest, step + 1);
#endif
            if (!(fabs(min_val) < INFINITY)) break;                        // NaN or an infinity in the costs: uniform over the workgroup
            const int j = best.key & (kAssigned - 1);
            if (j % kAssignThreads == tid) s_sc[j] = 1;
            if (!(best.key & kAssigned)) {
                sink = j;
                break;
            }
            i = best.row;
        }
        if (sink < 0) {
            failed = true;
            break;
        }
        // ---- one lane flips the path (at most ns links) while every lane updates the duals of its own visited elements, scipy's
        // expressions, and resets its search state.  Every s_sr, s_reach, s_spc and s_path store of the search is in front of its
        // last barrier; the flip touches the assignment alone, which nothing else reads here.
        if (tid == kAssignThreads - 1) {
            int j = sink;
            for (int k = 0; k < ns; ++k) {
                const int row = s_path[j];
                s_row4col[j] = row;
                const int next = s_col4row[row];
                s_col4row[row] = j;
                j = next;
                if (row == cur || j < 0) break;
            }
        }
        for (int s = tid; s < ns; s += kAssignThreads) {
            if (s_sr[s]) s_u[s] += min_val - s_reach[s], s_sr[s] = 0;
        }
        for (int l = tid; l < nl; l += kAssignThreads) {
            if (s_sc[l]) s_v[l] -= min_val - s_spc[l], s_sc[l] = 0;
            s_spc[l] = INFINITY;
        }
        __syncthreads();
    }

    if (failed) {
        for (int q = tid; q < N; q += kAssignThreads) row_match[q] = -1;
    } else if (by_query) {
        for (int q = tid; q < N; q += kAssignThreads) row_match[q] = s_col4row[q] % g;       // every query has a copy
    } else {
        for (int q = tid; q < N; q += kAssignThreads) row_match[q] = s_row4col[q] < 0 ? -1 : s_row4col[q] % g;
    }
#ifdef RDETR_DEV
    if (tid == 0) status[r] = (failed ? 1 : 0) | min(longest, 255) << 8 | steps << 16;
#else
    if (tid == 0) status[r] = failed ? 1 : 0;
#endif
}

int assign_match(const float *cost, const int *gt_count, int R, int B, int N, int Gmax, int repeat, int skip, int dn_groups,
                 int dn_max_gt, int *match, long long ld_match, int *status, void *stream)
{
    if (R < 0 || B <= 0 || N < 0 || Gmax <= 0 || repeat < 1 || skip < 0 || dn_groups < 0 || dn_max_gt < 0) return RDETR_ERR_INVALID_ARG;
    if (R == 0) return RDETR_OK;
    if (!cost || !gt_count || !match || !status) return RDETR_ERR_INVALID_ARG;
    if (R % B || (long long)dn_groups * dn_max_gt != skip || ld_match < (long long)skip + N) return RDETR_ERR_INVALID_ARG;
    if (N > kAssignMaxSide || (long long)Gmax * repeat > kAssignMaxSide) return RDETR_ERR_UNSUPPORTED;
    if (!all_aligned(4, cost, gt_count, match, status)) return RDETR_ERR_UNSUPPORTED;
    const int copies = Gmax * repeat;                                      // a row's count is on the device: size for the largest
    const int n_long = N > copies ? N : copies, n_short = N > copies ? copies : N;
    const size_t lds = assign_lds_bytes(n_long, n_short);
    if (const int s = ensure_dynamic_lds<assign_match_kernel>((int)assign_lds_bytes(kAssignMaxSide, kAssignMaxSide))) return s;
    hipLaunchKernelGGL(assign_match_kernel, dim3((unsigned)R), dim3(kAssignThreads), lds, static_cast<hipStream_t>(stream), cost,
                       gt_count, B, N, Gmax, repeat, skip, dn_max_gt > 0 ? dn_max_gt : 1, n_long, n_short, match, ld_match, status);
    return launch_status();
}

}  // namespace
}  // namespace rdetr

extern "C" int rdetr_assign_match(const float *cost, const int *gt_count, int R, int B, int N, int Gmax, int repeat, int skip,
                                  int dn_groups, int dn_max_gt, int *match, long long ld_match, int *status, void *stream)
{
    return rdetr::assign_match(cost, gt_count, R, B, N, Gmax, repeat, skip, dn_groups, dn_max_gt, match, ld_match, status, stream);
}
