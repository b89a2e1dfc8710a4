/*
 * relation_detr_amd.h -- C ABI of librelation_detr_amd.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the Relation-DETR hot path.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer (hipMalloc / torch tensor.data_ptr()) unless marked host;
 *   - tensors are contiguous, row-major; the caller allocates every output;
 *   - the library never allocates, never synchronises and keeps no global state: a call only
 *     enqueues kernels on `stream` (a hipStream_t passed as void*; NULL = the default stream),
 *     so calls are re-entrant across streams and capturable in a hipGraph;
 *   - return value: RDETR_OK (0) or a negative rdetr_status; rdetr_status_string() explains it.
 *     Unlike the reference (kernel-launch errors are printf'd and ignored,
 *     models/bricks/ops/cuda/ms_deform_im2col_cuda.cuh:937-941) launch errors are returned.
 */
#ifndef RELATION_DETR_AMD_H
#define RELATION_DETR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDETR_ABI_VERSION 3

typedef enum rdetr_status {
    RDETR_OK = 0,
    RDETR_ERR_INVALID_ARG = -1,   /* null pointer, negative size, misaligned pointer */
    RDETR_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels are built for */
    RDETR_ERR_LAUNCH = -3         /* hipGetLastError() != hipSuccess after the launch */
} rdetr_status;

int rdetr_abi_version(void);
const char *rdetr_status_string(int status);

/* ---------------------------------------------------------------------------------------------
 * Multi-scale deformable attention, forward.
 * Replaces  _C.ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc,
 *           attn_weight, im2col_step)            models/bricks/ops/cuda/ms_deform_attn_cuda.cu:12-72,148-150
 *           (kernel ms_deformable_im2col_gpu_kernel, ms_deform_im2col_cuda.cuh:226-288) and equals
 *           multi_scale_deformable_attn_pytorch  models/bricks/ms_deform_attn.py:159-212.
 *
 *   value          [B, S, H, D]        levels packed along S, row-major (y*W_l + x) inside a level
 *   spatial_shapes [L, 2] int64 (h,w)  level_start_index [L] int64          (device memory)
 *   sampling_loc   [B, Nq, H, L, P, 2] fp32, (x, y) normalised to [0,1]
 *   attn_weight    [B, Nq, H, L, P]    fp32 (already soft-maxed over L*P by the caller)
 *   out            [B, Nq, H*D]        channel = head*D + c
 *
 * Fast path (H = 8, D = 32, P = 4, L <= 8, see rdetr_msda_fast_path()): the query-run kernel of
 * csrc/msda_fwd.hip; any other (H, D, P) runs a generic one-thread-per-output kernel.  There is no im2col_step batch
 * restriction (the reference requires B % min(B, 64) == 0, ms_deform_attn_cuda.cu:42-44).
 * NaN sampling locations contribute zero (the CUDA op's guard, ms_deform_im2col_cuda.cuh:277).
 * The bf16 variant stores value and out as bfloat16 and keeps locations, weights and the
 * accumulation in fp32 (an extension: the reference op is fp32/fp64 only, ms_deform_attn_cuda.cu:56).
 */
int rdetr_msda_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                           const float *sampling_loc, const float *attn_weight, int B, int S, int H, int D,
                           int L, int Nq, int P, float *out, void *stream);

int rdetr_msda_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                            const float *sampling_loc, const float *attn_weight, int B, int S, int H, int D,
                            int L, int Nq, int P, uint16_t *out, void *stream);

/* Same operator with the sampling-location producer fused in.
 * Replaces lines 322-349 + the core call of MultiScaleDeformableAttention.forward
 * (models/bricks/ms_deform_attn.py): the caller passes the RAW outputs of the two query projections,
 *   sampling_offsets [B, Nq, H, L, P, 2]   attn_logits [B, Nq, H, L*P]   (dtype of value: fp32 / bf16)
 *   reference_points [B, Nq, L, ref_dim] fp32, ref_dim 2 (x,y) or 4 (cx,cy,w,h)
 * and the kernel performs softmax over L*P and  loc = ref + off/(W_l,H_l)  (ref_dim 2)  or
 * ref_xy + off/P * ref_wh * 0.5  (ref_dim 4)  in its set-up phase -- locations and weights never
 * exist in HBM.  Fast-path shapes only (rdetr_msda_fast_path() == 1); otherwise RDETR_ERR_UNSUPPORTED
 * and the caller uses rdetr_msda_forward_* with materialised locations / weights. */
int rdetr_msda_forward_fused_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                 const float *sampling_offsets, const float *attn_logits,
                                 const float *reference_points, int ref_dim, int B, int S, int H, int D, int L, int Nq,
                                 int P, float *out, void *stream);

int rdetr_msda_forward_fused_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, const uint16_t *sampling_offsets,
                                  const uint16_t *attn_logits, const float *reference_points, int ref_dim, int B, int S,
                                  int H, int D, int L, int Nq, int P, uint16_t *out, void *stream);

/* General fused-producer form.  `key_padding_mask` (u8 [B, S], non-zero = padded position, may be NULL) is applied inside the
 * gather: a padded pixel's row counts as zero, which is what zero-filling the projected value does
 * (models/bricks/ms_deform_attn.py:316-319) -- without a pass over the [B, S, H*D] tensor.  ROW STRIDES (in elements;
 * 0 = contiguous) of the two projection outputs, so that sampling_offsets and attention_weights can be the column slices [0, 2*H*L*P) and
 * [2*H*L*P, 3*H*L*P) of ONE [rows, 3*H*L*P] GEMM output (one projection GEMM instead of two).  ld_offsets must be even
 * (offsets are read as (x, y) pairs). */
int rdetr_msda_forward_fused_ex_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                    const float *sampling_offsets, int ld_offsets, const float *attn_logits, int ld_logits,
                                    const float *reference_points, int ref_dim, const uint8_t *key_padding_mask, int B,
                                    int S, int H, int D, int L, int Nq, int P, float *out, void *stream);
int rdetr_msda_forward_fused_ex_bf16(const uint16_t *value, const int64_t *spatial_shapes,
                                     const int64_t *level_start_index, const uint16_t *sampling_offsets, int ld_offsets,
                                     const uint16_t *attn_logits, int ld_logits, const float *reference_points, int ref_dim,
                                     const uint8_t *key_padding_mask, int B, int S, int H, int D, int L, int Nq, int P,
                                     uint16_t *out, void *stream);

/* bf16 operator (both producer forms) with the VALUE LAYOUT and the KERNEL CHOICE as explicit arguments -- the library
 * reads no environment variable and keeps no state.
 *   value_layout  RDETR_VALUE_BSHD  value [B, S, H, D]: the reference operator's layout (ms_deform_attn_cuda.cu:12-19);
 *                 RDETR_VALUE_BHSD  value [B, H, S, D]: head-major -- one (image, head) plane is contiguous, so the window
 *                                   kernel fills its LDS windows at the contiguous-row rate.  Written by
 *                                   rdetr_value_to_head_major_bf16 (below); fast-path shapes only.
 *   algo          RDETR_MSDA_AUTO    what the plain entry points do: the direct kernel.  Correct for ANY level table the
 *                                    reference operator accepts (gaps, overlapping or unordered levels, sum(h*w) < S);
 *                 RDETR_MSDA_DIRECT  csrc/msda_fwd.hip -- the query-run kernel (range-checked global gathers), any Nq, L <= 8;
 *                 RDETR_MSDA_AUTO_PACKED  the faster kernel per layout: for RDETR_VALUE_BSHD the window kernel where it
 *                                    applies, else (and for RDETR_VALUE_BHSD) the direct kernel.  Same PRECONDITION as
 *                                    RDETR_MSDA_WINDOW;
 *                 RDETR_MSDA_WINDOW  csrc/msda_win.hip -- LDS-window MFMA kernel for the ENCODER shape: queries are the
 *                                    pyramid's own pixels in level_start order (Nq == S), L == 4, S >= 4096, no padding
 *                                    mask.  PRECONDITION (the caller's promise -- the level table lives in device memory
 *                                    and the library never synchronises, so it cannot check): the levels TILE [0, S)
 *                                    exactly, level_start[l] = sum of h*w of the earlier levels and sum(h*w) == S, and no
 *                                    level is larger than level 0 (the kernel enumerates its queries as the pixels of the
 *                                    levels: with gaps or overlaps output rows would be left unwritten or written twice).
 *                                    rdetr_msda_levels_window_ok() checks a HOST copy of the table.  Per 16 x 12 query tile and level a 32-pixel-wide window of the value plane is
 *                                    copied L2 -> LDS by range-checked LDS-DMA (pixels outside the level arrive as zeros) and
 *                                    gathered from there on the matrix cores; samples outside their window are fetched from
 *                                    global memory, so results never depend on the windows.  RDETR_ERR_UNSUPPORTED for any
 *                                    other shape.
 * Results of the two kernels agree to the rounding of the bf16 output (different summation order). */
#define RDETR_VALUE_BSHD 0
#define RDETR_VALUE_BHSD 1
#define RDETR_MSDA_AUTO 0
#define RDETR_MSDA_DIRECT 1
#define RDETR_MSDA_WINDOW 2
#define RDETR_MSDA_AUTO_PACKED 3
/* 1 if a level table (HOST pointers) meets the precondition of RDETR_MSDA_WINDOW / RDETR_MSDA_AUTO_PACKED for a value tensor
 * with S positions, else 0.  Pure host arithmetic. */
int rdetr_msda_levels_window_ok(const int64_t *host_spatial_shapes, const int64_t *host_level_start_index, int L, long long S);
int rdetr_msda_forward_opt_bf16(const uint16_t *value, int value_layout, const int64_t *spatial_shapes,
                                const int64_t *level_start_index, const float *sampling_loc, const float *attn_weight, int B,
                                int S, int H, int D, int L, int Nq, int P, int algo, uint16_t *out, void *stream);
/* The bf16 operator on the SWEEP kernel (csrc/msda_sweep.hip, round 4) -- the LDS-sourced gather for the ENCODER shape: queries
 * are the pyramid's own pixels in level_start order (Nq == S), L == 4, H == 8, D == 32, P == 4.  Replaces the kernel of
 * ms_deformable_im2col_cuda (ms_deform_im2col_cuda.cuh:226-288, 912-943) for that shape; same tensors as
 * ms_deform_attn_cuda_forward (ms_deform_attn_cuda.cu:12-72) except that the LEVEL TABLE is passed as HOST pointers: the grid
 * and the band height are sized from it and the kernel takes it as arguments (the reference reads spatial_shapes on the host
 * too, ms_deform_attn.py:313).  PRECONDITION as RDETR_MSDA_WINDOW (the levels tile [0, S), checked here on the host copy;
 * the caller promises that the device tensors it built sampling_loc from describe the same levels).  One persistent
 * 1024-thread workgroup per CU slides ring-buffer windows of all four levels along a band of level-0 rows, 8 columns per
 * step: only the new columns are fetched (range-checked LDS-DMA, a step ahead: outside the level = zeros), the corner rows
 * are gathered from LDS by ds_read_b64_tr_b16 into v_mfma_f32_16x16x32_bf16, samples outside their window are fetched from
 * global memory and added in fp32, so results never depend on the windows.  RDETR_ERR_UNSUPPORTED for any other shape
 * (pyramids whose coarser levels are not about half the finer ones included; callers use the direct kernel);
 * sampling_loc must be 16-byte and attn_weight 8-byte aligned.  OPT-IN: measured slower than the direct kernel (DESIGN.md
 * section 4.2 has the numbers and the measured ceiling of the data path). */
int rdetr_msda_forward_sweep_bf16(const uint16_t *value, int value_layout, const int64_t *host_spatial_shapes,
                                  const int64_t *host_level_start_index, const float *sampling_loc, const float *attn_weight,
                                  int B, int S, int H, int D, int L, int Nq, int P, uint16_t *out, void *stream);
/* The bf16 operator on the RESIDENT-LEVELS kernel (csrc/msda_res.hip, round 4), head-major value [B,H,S,D] only.  Same operator
 * (ms_deform_attn_cuda_forward, ms_deform_attn_cuda.cu:12-72; kernel ms_deform_im2col_cuda.cuh:226-288), same per-query
 * arithmetic as the query-run kernel; the points of a query are accumulated in another order (coarse and fine levels
 * alternate), so results agree with rdetr_msda_forward_opt_bf16(..., RDETR_MSDA_DIRECT) to fp32 re-association: the last bit
 * of a bf16 output differs now and then (4e-5 of the outputs at the R50 shape).  One persistent 12-wave (768-thread)
 * workgroup per CU serves one (image, head) plane and keeps the plane's COARSE levels -- as many trailing levels as fit beside the staging area in the CU's 160 KB of LDS (levels 2 and 3
 * at the R50 800 x 1333 shape: half of all samples) -- resident in LDS: samples on those levels read their corner rows with
 * ds_read_b128 instead of through the texture path, whose instruction rate bounds the query-run kernel.
 * The LEVEL TABLE is passed as HOST pointers (the resident set is sized on the host; the reference reads spatial_shapes on
 * the host too, ms_deform_attn.py:313); the levels must tile [0, S).  RDETR_ERR_UNSUPPORTED -- callers then use the
 * query-run kernel -- for: L other than 4 or 5, a level table that does not tile [0, S), not even the coarsest level fitting,
 * inputs that miss the vector-load alignment (sampling_loc / attn_weight 16 bytes at L = 4). */
int rdetr_msda_forward_resident_bf16(const uint16_t *value_bhsd, const int64_t *host_spatial_shapes,
                                     const int64_t *host_level_start_index, const float *sampling_loc, const float *attn_weight,
                                     int B, int S, int H, int D, int L, int Nq, int P, uint16_t *out, void *stream);
/* ... and its fused-producer form (arguments as rdetr_msda_forward_fused_opt_bf16; no key_padding_mask: the head-major
 * value's padded rows are zero already; 2-d reference points only -- ref_dim == 4 is RDETR_ERR_UNSUPPORTED here and runs on the
 * query-run kernel). */
int rdetr_msda_forward_fused_resident_bf16(const uint16_t *value_bhsd, const int64_t *host_spatial_shapes,
                                           const int64_t *host_level_start_index, const uint16_t *sampling_offsets,
                                           int ld_offsets, const uint16_t *attn_logits, int ld_logits,
                                           const float *reference_points, int ref_dim, int B, int S, int H, int D, int L, int Nq,
                                           int P, uint16_t *out, void *stream);
int rdetr_msda_forward_fused_opt_bf16(const uint16_t *value, int value_layout, const int64_t *spatial_shapes,
                                      const int64_t *level_start_index, const uint16_t *sampling_offsets, int ld_offsets,
                                      const uint16_t *attn_logits, int ld_logits, const float *reference_points, int ref_dim,
                                      const uint8_t *key_padding_mask, int B, int S, int H, int D, int L, int Nq, int P,
                                      int algo, uint16_t *out, void *stream);

/* The fused-producer bf16 operator on a ROW-STRIDED value: pixel s of image b starts at value + (b * S + s) * value_ld elements
 * (value_ld >= H * D, a 16-byte multiple; 0 = dense), i.e. `value` may be a 256-column slice of a wider projection output.  Lets
 * the SIX cross-attention value projections of the decoder (models/bricks/relation_transformer.py:464-471 calls value_proj of
 * each layer on the same encoder memory, ms_deform_attn.py:316) run as ONE [S, 256] x [256, 6*256] GEMM whose output each
 * layer's gather reads in place.  [B,S,H,D] layout, direct kernel, fast-path shapes; other arguments as
 * rdetr_msda_forward_fused_ex_bf16. */
int rdetr_msda_forward_fused_strided_bf16(const uint16_t *value, long long value_ld, const int64_t *spatial_shapes,
                                          const int64_t *level_start_index, const uint16_t *sampling_offsets, int ld_offsets,
                                          const uint16_t *attn_logits, int ld_logits, const float *reference_points, int ref_dim,
                                          const uint8_t *key_padding_mask, int B, int S, int H, int D, int L, int Nq, int P,
                                          uint16_t *out, void *stream);

/* Projected value [B, S, H*D] bf16 (rows `ld` elements apart, ld % 8 == 0: the rows may be a column slice of a wider
 * buffer) -> head-major [B, H, S, D], with the rows of padded positions (`key_padding_mask` u8 [B, S], may be NULL)
 * written as zeros -- the zero-fill of models/bricks/ms_deform_attn.py:316-319 folded into the re-layout.  H = 8, D = 32. */
int rdetr_value_to_head_major_bf16(const uint16_t *src, long long ld, const uint8_t *key_padding_mask, int B, int S, int H,
                                   int D, uint16_t *dst, void *stream);

/* MSDA's value projection (models/bricks/ms_deform_attn.py:316-321: value_proj, then zero-fill of the padded rows) written
 * straight into the head-major layout by the hand-written MFMA projection kernel (csrc/linear.hip):
 *   out_hm [B, 8, S, 32] bf16  <-  x [B*S, 256] (rows ldx elements apart) w[256, 256]^T + bias[256] (nullable),
 * rows with row_mask != 0 (u8 [B*S], nullable) stored as zeros.  Same bits as rdetr_linear_k256_bf16 followed by
 * rdetr_value_to_head_major_bf16. */
int rdetr_linear_k256_hm_bf16(const uint16_t *x, long long ldx, const uint16_t *w, const uint16_t *bias, const uint8_t *row_mask,
                              int B, int S, uint16_t *out_hm, void *stream);

/* 1 if (H, D, L, P) is served by the query-run kernel, 0 if by the generic kernel. */
int rdetr_msda_fast_path(int H, int D, int L, int P);

/* ---------------------------------------------------------------------------------------------
 * Multi-scale deformable attention, backward.
 * Replaces  _C.ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc,
 *           attn_weight, grad_output, im2col_step) -> [grad_value, grad_sampling_loc, grad_attn_weight]
 *           models/bricks/ops/cuda/ms_deform_attn_cuda.cu:75-145, ms_deform_im2col_cuda.cuh:290-392.
 * grad_value [B,S,H,D] is accumulated with float atomics and MUST be zero-filled by the caller
 * (the reference zero-fills inside the op, ms_deform_attn_cuda.cu:113-115; the Python wrapper does
 * it here).  grad_sampling_loc / grad_attn_weight are fully overwritten.
 */
int rdetr_msda_backward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                            const float *sampling_loc, const float *attn_weight, const float *grad_out, int B,
                            int S, int H, int D, int L, int Nq, int P, float *grad_value,
                            float *grad_sampling_loc, float *grad_attn_weight, void *stream);

/* The same gradients with a DETERMINISTIC grad_value ("deterministic alternative to atomics"; the reference's
 * backward adds with atomicAdd, ms_deform_im2col_cuda.cuh:290-392, so its bits depend on the run): one (pixel-row key, weight)
 * record per sample corner, a stable radix sort of the records by key, and a per-row sum in sorted = original sample order.
 * grad_sampling_loc / grad_attn_weight are fixed-order sums in both modes.  grad_value is OVERWRITTEN (every row, no
 * zero-initialisation needed).  workspace: rdetr_msda_backward_det_workspace_bytes() bytes, 16-byte aligned (records + sort
 * buffers + the sort's temporary storage; 20 bytes per sample corner: 0.9 GB at B = 4 of the R50 encoder shape); that function
 * returns 0 for empty problems / unsupported shapes and -1 when the record count exceeds 2^31.  H = 8, D = 32, P = 4, L <= 8 only
 * (RDETR_ERR_UNSUPPORTED otherwise).  Measured at the R50 encoder shape: 1.87 ms vs 1.07 ms (B = 1), 5.84 vs 4.24 ms (B = 4) for the
 * atomic kernel (tools/profile_msda_bwd.py). */
long long rdetr_msda_backward_det_workspace_bytes(int B, int S, int H, int D, int L, int Nq, int P);
int rdetr_msda_backward_det_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                const float *sampling_loc, const float *attn_weight, const float *grad_out, int B, int S, int H, int D,
                                int L, int Nq, int P, void *workspace, long long workspace_bytes, float *grad_value,
                                float *grad_sampling_loc, float *grad_attn_weight, void *stream);

/* Fused-producer backward: the gradients of rdetr_msda_forward_fused_* with respect to its own inputs (training mode of the
 * fused path).  Replaces  MultiScaleDeformableAttnFunction.backward            models/bricks/ms_deform_attn.py:35-84
 *           + autograd through the softmax and the sampling-location arithmetic  ms_deform_attn.py:322-370
 *           (_C.ms_deform_attn_backward, ms_deform_attn_cuda.cu:75-145).
 *   value [B,S,H,D], sampling_offsets [B,Nq,H,L,P,2], attn_logits [B,Nq,H,L*P], grad_out [B,Nq,H*D]: value's dtype (fp32 | bf16)
 *   reference_points [B,Nq,L,ref_dim] fp32, ref_dim 2 or 4
 *   grad_value [B,S,H,D] fp32; grad_offsets / grad_logits: the shapes of their inputs, value's dtype;
 *   grad_ref_partial [B,Nq,H,L,ref_dim] fp32 (nullable): one partial per head, the caller sums over H.
 * The softmax weights and locations are recomputed with the forward kernel's arithmetic for the dtype, so the backward
 * differentiates what the forward used.  Points outside their level or at NaN locations contribute nothing.
 * workspace NULL: atomic mode, grad_value accumulated with float atomics and MUST be zero-filled by the caller.  Otherwise
 * deterministic mode: rdetr_msda_backward_det_workspace_bytes() bytes (16-byte aligned), grad_value OVERWRITTEN (every row).
 * grad_offsets / grad_logits / grad_ref_partial are fixed-order sums: the same bits in both modes.  B = 0 or Nq = 0: nothing is
 * written.  H = 8, D = 32, P = 4, L <= 8 only (RDETR_ERR_UNSUPPORTED otherwise). */
int rdetr_msda_backward_fused_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                  const float *sampling_offsets, const float *attn_logits, const float *reference_points, int ref_dim,
                                  const float *grad_out, int B, int S, int H, int D, int L, int Nq, int P, void *workspace,
                                  long long workspace_bytes, float *grad_value, float *grad_offsets, float *grad_logits,
                                  float *grad_ref_partial, void *stream);
int rdetr_msda_backward_fused_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                   const uint16_t *sampling_offsets, const uint16_t *attn_logits, const float *reference_points,
                                   int ref_dim, const uint16_t *grad_out, int B, int S, int H, int D, int L, int Nq, int P,
                                   void *workspace, long long workspace_bytes, float *grad_value, uint16_t *grad_offsets,
                                   uint16_t *grad_logits, float *grad_ref_partial, void *stream);

/* The fused-producer bf16 backward on a HEAD-MAJOR value (training counterpart of the RDETR_VALUE_BHSD forward): arguments as
 * rdetr_msda_backward_fused_bf16 except that
 *   value_bhsd [B,H,S,D] bf16 and grad_value_bhsd [B,H,S,D] fp32 are head-major (what rdetr_value_to_head_major_bf16 writes);
 *   sampling_offsets / attn_logits take row strides ld_offsets / ld_logits (elements; 0 = dense; ld_offsets even: the
 *   convention of rdetr_msda_forward_fused_ex_bf16), and grad_offsets / grad_logits take row strides of their own, so each
 *   pair can be the column slices [0, 2*H*L*P) and [2*H*L*P, 3*H*L*P) of ONE [B*Nq, 3*H*L*P] buffer: the output of the merged
 *   query projection and its gradient.
 * The layout is an addressing matter only: the same kernel body, the same products summed in the same order, so
 * grad_offsets / grad_logits / grad_ref_partial have the bits of rdetr_msda_backward_fused_bf16 on the [B,S,H,D] copy of the
 * value, and so has the deterministic grad_value after the permutation.  Both modes (workspace NULL: float atomics into a
 * zero-filled grad_value; otherwise rdetr_msda_backward_det_workspace_bytes() bytes, every grad_value row overwritten).
 * RDETR_ERR_INVALID_ARG: null / negative / short workspace / a stride below its row length / odd ld_offsets or
 * ld_grad_offsets; RDETR_ERR_UNSUPPORTED: other than H = 8, D = 32, P = 4, L <= 8, or a missed alignment (value, grad_value,
 * reference_points, workspace 16 bytes; offsets 4, logits 2).  B = 0 or Nq = 0: nothing is written. */
int rdetr_msda_backward_fused_hm_bf16(const uint16_t *value_bhsd, const int64_t *spatial_shapes, const int64_t *level_start_index,
                                      const uint16_t *sampling_offsets, int ld_offsets, const uint16_t *attn_logits, int ld_logits,
                                      const float *reference_points, int ref_dim, const uint16_t *grad_out, int B, int S, int H,
                                      int D, int L, int Nq, int P, void *workspace, long long workspace_bytes,
                                      float *grad_value_bhsd, uint16_t *grad_offsets, int ld_grad_offsets, uint16_t *grad_logits,
                                      int ld_grad_logits, float *grad_ref_partial, void *stream);

/* Adjoint of rdetr_value_to_head_major_bf16: grad_hm [B, H, S, D] fp32 -> dst [B*S, H*D] bf16 (rows `ld` elements apart,
 * ld % 8 == 0, 16-byte aligned: dst may be a column slice of a wider buffer), channel = head * D + c, rounded to bf16 once
 * (round-to-nearest-even).  Rows of padded positions (`key_padding_mask` u8 [B, S], may be NULL) are written as zeros without
 * reading their source: the backward of the zero-fill of models/bricks/ms_deform_attn.py:316-319 and the cast of the fp32
 * gradient, in one pass.  H = 8, D = 32. */
int rdetr_grad_value_from_head_major_bf16(const float *grad_hm, const uint8_t *key_padding_mask, int B, int S, int H, int D,
                                          uint16_t *dst, long long ld, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Position-relation bias.
 * Replaces  PositionRelationEmbedding.forward  models/bricks/relation_transformer.py:520-532
 *           = box_rel_encoding (:481-490) -> get_sine_pos_embed (models/bricks/position_encoding.py:115-138)
 *             -> Conv2d(4*F -> Hh, 1x1) + ReLU -> clone.
 *   src [B, N1, 4], tgt [B, N2, 4]   cxcywh boxes, fp32
 *   proj_weight [Hh, 4*F]  (pos_proj.0.weight flattened), proj_bias [Hh] (may be NULL)
 *   out [B, Hh, N1, N2]    fp32, >= 0;  rows = src (queries), cols = tgt (keys)
 * F = num_pos_feats (16 in every relation_detr config), must be even and <= 32; Hh <= 16.
 */
int rdetr_relation_bias_f32(const float *src, const float *tgt, const float *proj_weight, const float *proj_bias,
                            int B, int N1, int N2, int Hh, int F, float scale, float temperature, float eps,
                            float *out, void *stream);

/* Same operator with a caller-provided workspace of (B*N1 + B*N2) * 2*F floats (8-byte aligned): for F = 16, Hh = 8 the
 * two size-ratio coordinates log(w_i/w_j), log(h_i/h_j) take their sine features from per-box tables (angle computed in
 * double precision once per box) by the angle-difference identities instead of evaluating sin / cos per pair -- a third
 * fewer instructions.  Results stay within 1e-4 of both the fp32 and the fp64 evaluation of the reference formula (the
 * fp32 reference itself rounds these angles to ~3e-5 rad).  Any other configuration forwards to rdetr_relation_bias_f32. */
int rdetr_relation_bias_ws_f32(const float *src, const float *tgt, const float *proj_weight, const float *proj_bias,
                               int B, int N1, int N2, int Hh, int F, float scale, float temperature, float eps,
                               float *workspace, float *out, void *stream);

/* Backward of the relation bias with respect to the 1x1 projection -- what autograd computes for
 * PositionRelationEmbedding.pos_proj in training (models/bricks/relation_transformer.py:527-532; the boxes carry no gradient,
 * :527-529):
 *     grad_weight[h][ch] = sum_{b,i,j} g[b,h,i,j] * feat[b,i,j,ch],   grad_bias[h] = sum g,   g = grad_out where active else 0
 * with the 64 sine features REGENERATED from the boxes by the forward's arithmetic (the reference keeps [N1, N2, 64] per image
 * for its backward GEMM: 207 MB at N = 900).
 *   src [B,N1,4], tgt [B,N2,4] fp32 cxcywh (tgt 16-byte aligned); grad_out [B,Hh,N1,N2] fp32; active u8 [B,Hh,N1,N2] = (forward
 *   output > 0), the ReLU's derivative; workspace: rdetr_relation_bias_backward_workspace_bytes(B, N1, N2) bytes;
 *   grad_weight [Hh, 4F] fp32, grad_bias [Hh] fp32 or NULL -- both OVERWRITTEN (no zero-initialisation needed).
 * DETERMINISTIC: per-block partial sums go to the workspace and a second kernel adds them in a fixed order (no float atomics).
 * Hh = 8, F = 16 only (RDETR_ERR_UNSUPPORTED otherwise). */
long long rdetr_relation_bias_backward_workspace_bytes(int B, int N1, int N2);
int rdetr_relation_bias_backward_f32(const float *src, const float *tgt, const float *grad_out, const uint8_t *active, int B, int N1,
                                     int N2, int Hh, int F, float scale, float temperature, float eps, float *workspace,
                                     float *grad_weight, float *grad_bias, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Bias-add + row softmax of decoder self-attention scores, in place.
 * Replaces the softmax(QK^T/sqrt(d) + attn_mask) step of nn.MultiheadAttention as called at
 * models/bricks/relation_transformer.py:452-459 (float mask [B*Hh, N, N] from :372-374).
 *   scores [BH, N1, N2] fp32, overwritten with the probabilities
 *   bias   [BH, N1, N2] fp32 or NULL (may contain -inf)
 *   mask   [N1, N2] uint8 or NULL; non-zero = excluded (the bool attn_mask convention)
 * A fully masked row yields NaN, as torch.softmax does.
 */
int rdetr_bias_softmax_f32(float *scores, const float *bias, const uint8_t *mask, int BH, int N1, int N2,
                           void *stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder self-attention with the relation bias, fused:
 *   out = softmax(Q K^T * scale + bias [, bool mask]) V     per (image, head), bf16 activations, fp32 soft-max.
 * Replaces the attention core of the nn.MultiheadAttention call of the decoder layer
 *           models/bricks/relation_transformer.py:452-461 with the float bias of :369-374 as attn_mask
 * (QK^T GEMM, bias add, softmax, PV GEMM and the dtype copies between them) by one flash-style MFMA kernel.
 *   q [B, N, ..], k / v [B, M, ..]   bf16, head h at columns h*D .. h*D+D-1 of a row; ldq / ldk / ldv = row stride in
 *                                    ELEMENTS (so slices of a packed in-projection output can be passed as they are),
 *                                    image stride = rows * ld
 *   bias  fp32 [B*H, N, M] or NULL (may hold -inf);   bool_mask u8 [N, M] or NULL (non-zero = excluded)
 *   out   bf16 [B, N, ..] with row stride ldo;  D = 32 only (RDETR_ERR_UNSUPPORTED otherwise)
 * A fully masked row yields NaN, as torch.softmax does. */
int rdetr_relation_attention_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                  const float *bias, const uint8_t *bool_mask, int B, int H, int D, int N, int M,
                                  float scale, uint16_t *out, int ldo, void *stream);

/* Swin's shifted-window attention between the qkv and the proj GEMM of a block, one launch (csrc/attn_win.hip; forward only):
 *   out = softmax(Q K^T * scale + relative position bias [+ shift mask]) V    per (image, window, head)
 * Replaces models/backbones/swin.py:133-221 around that product: pad, roll, window partition, the qkv permute, the
 * [B*nW, heads, N, N] scores, bias add, mask add, softmax, P V, window reverse, roll back, unpad.
 *   q, k, v   bf16 [B, H*W, ..] of the UNPADDED map, head h at columns h*D .. h*D+D-1; ldq / ldk / ldv = row stride in elements
 *             (the three column blocks of the qkv GEMM's [B, H*W, 3C] output can be passed as they are); 16-byte aligned,
 *             ld % 8 == 0, ld >= heads * D
 *   k_pad, v_pad   bf16 [heads * D] or NULL: k and v of a padding token (a source position outside H x W once the map is
 *             padded to a multiple of the window) = the qkv linear's bias row, zeros when NULL.  Padding tokens take part as
 *             keys; their own outputs are not stored.  16-byte aligned
 *   table     [(2 wh - 1)(2 ww - 1), heads], fp32 (table_bf16 = 0) or bf16 (1): relative_position_bias_table as it is; the
 *             kernel computes (ri - rj + wh - 1)(2 ww - 1) + (ci - cj + ww - 1) itself
 *   sh, sw    the EFFECTIVE shift (0 in a dimension whose window is >= the padded size): the rolled-frame position (y, x) is the
 *             token of source position ((y + sh) % pH, (x + sw) % pW); with sh + sw > 0, -100 is added between tokens of
 *             different regions (3 hr + wr; hr = 0 below pH - wh, 1 below pH - sh, else 2)
 *   out       bf16 [B, H*W, ..] with row stride ldo, written at the token's SOURCE row (un-windowed, un-rolled, unpadded);
 *             16-byte aligned, ldo % 8 == 0
 * D = 32 and wh * ww <= 144 only (RDETR_ERR_UNSUPPORTED otherwise); wh * ww == 0 or a shift >= its window is
 * RDETR_ERR_INVALID_ARG; B == 0 or H * W == 0 is a no-op. */
int rdetr_window_attention_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                const uint16_t *k_pad, const uint16_t *v_pad, const void *table, int table_bf16, int B,
                                int heads, int D, int H, int W, int wh, int ww, int sh, int sw, float scale,
                                uint16_t *out, int ldo, void *stream);

/* Training forward: the same kernel and the same out bits as rdetr_relation_attention_bf16, plus the per-row log-sum-exp
 *   lse   fp32 [B*H, N], LOG2 domain: lse[bh * N + n] = log2(sum_m exp2((s * scale + bias) * log2(e))) (-inf for a fully masked
 *         row); natural log = lse * ln(2).  rdetr_relation_attention_backward_bf16 takes it as written.
 * B, H, N, M > 0, row strides >= H * D (RDETR_ERR_INVALID_ARG otherwise); D = 32 only. */
int rdetr_relation_attention_train_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                        const float *bias, const uint8_t *bool_mask, int B, int H, int D, int N, int M,
                                        float scale, uint16_t *out, int ldo, float *lse, void *stream);

/* Backward of the training forward (csrc/attn_bwd.hip, FlashAttention-2 shaped, deterministic: no float atomics).
 *   q, k, v, ld*, bias, bool_mask, B, H, D, N, M, scale   as given to the forward;  out / ldo and lse what it wrote
 *   dout  bf16 [B, N, ..] with row stride lddo (16-byte aligned, lddo % 8 == 0)
 *   workspace   rdetr_relation_attention_backward_workspace_bytes(B, H, N) bytes, 16-byte aligned (Di = rowsum(dout o out))
 *   dq [B, N, ..], dk / dv [B, M, ..]   bf16, written with row strides lddq / lddk / lddv (every row, head columns only): dq and
 *         dk may be the two halves of one packed [B, N, 2C] buffer (ld = 2C, dk = dq + C) when N == M
 *   dbias fp32 [B*H, N, M] or NULL: the gradient of the attention logits (= of the bias), every element written once;
 *         0 at -inf bias entries and masked keys
 * A fully masked row contributes nothing to dk / dv; its own dq row and dbias row are 0.  B, H, N, M > 0, row strides
 * >= H * D, a large enough workspace (RDETR_ERR_INVALID_ARG otherwise); D = 32 only. */
long long rdetr_relation_attention_backward_workspace_bytes(int B, int H, int N);
int rdetr_relation_attention_backward_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                           const uint16_t *out, int ldo, const float *lse, const uint16_t *dout, int lddo,
                                           const float *bias, const uint8_t *bool_mask, int B, int H, int D, int N, int M,
                                           float scale, void *workspace, long long workspace_bytes, uint16_t *dq, int lddq,
                                           uint16_t *dk, int lddk, uint16_t *dv, int lddv, float *dbias, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The same attention with the relation bias GENERATED INSIDE the kernel from the boxes (SURVEY.md section 8 f1 as written):
 *   out = softmax(Q K^T * attn_scale + relu(W . sine(box_rel_encoding(src_boxes, tgt_boxes)) + b) [, bool mask]) V
 * Replaces PositionRelationEmbedding.forward (models/bricks/relation_transformer.py:520-532, box_rel_encoding :481-490,
 * get_sine_pos_embed position_encoding.py:115-138) TOGETHER WITH the nn.MultiheadAttention call that consumes its result
 * (:369-374, :452-461): the [B, H, N, M] fp32 bias never exists in HBM.
 *   q, k, v, ld*, bool_mask, out, ldo   as rdetr_relation_attention_bf16
 *   src_boxes [B, N, 4], tgt_boxes [B, M, 4]   fp32 cxcywh (query i <-> src box i, key j <-> tgt box j), 16-byte aligned
 *   proj_weight [H, 4F] fp32 (pos_proj.0.weight), proj_bias [H] fp32 or NULL
 *   H = 8, D = 32, F = 16 only (RDETR_ERR_UNSUPPORTED otherwise -> materialise the bias with rdetr_relation_bias_f32)
 * bf16 inference path: the sine features are rounded to bf16 for the MFMA projection and the angles use the hardware
 * log2 / sin / cos; results are held to the same bound against the fp32 reference as rdetr_relation_attention_bf16. */
int rdetr_relation_attention_boxes_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                        const float *src_boxes, const float *tgt_boxes, const float *proj_weight,
                                        const float *proj_bias, const uint8_t *bool_mask, int B, int H, int D,
                                        int N, int M, int F, float rel_scale, float temperature, float eps, float attn_scale,
                                        uint16_t *out, int ldo, void *stream);

/* Training forward of the kernel above: the same out bits as rdetr_relation_attention_boxes_bf16, plus the per-row
 * log-sum-exp of the logits  Q K^T * attn_scale + relu(bias)  [, mask]
 *   lse   fp32 [B*H, N], LOG2 domain (as rdetr_relation_attention_train_bf16 writes it; -inf for a fully masked row), 4-byte
 *         aligned; rdetr_relation_attention_boxes_backward_bf16 takes it as written.
 * Replaces, for bf16 training, rdetr_relation_bias_f32 + the masked_fill_ of the denoising mask (relation_transformer.py:369-374)
 * + rdetr_relation_attention_train_bf16: neither the [B, H, N, M] bias nor its ReLU mask exists in HBM.  Refusals as the
 * inference entry; a NULL lse and B, N or M = 0 are RDETR_ERR_INVALID_ARG. */
int rdetr_relation_attention_boxes_train_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                              const float *src_boxes, const float *tgt_boxes, const float *proj_weight,
                                              const float *proj_bias, const uint8_t *bool_mask, int B, int H, int D,
                                              int N, int M, int F, float rel_scale, float temperature, float eps, float attn_scale,
                                              uint16_t *out, int ldo, float *lse, void *stream);

/* Backward of that forward (csrc/attn_rel_bwd.hip; deterministic: no float atomics, every output element written once).
 * Replaces rdetr_relation_attention_backward_bf16 with a dbias output followed by rdetr_relation_bias_backward_f32 (autograd of
 * relation_transformer.py:520-532 and :452-461): the bias is regenerated from the boxes with the forward kernel's arithmetic,
 * so the ReLU's active set is the forward's, and the gradient of the 1x1 projection is reduced inside the kernels -- no
 * [B*H, N, M]-sized tensor (bias, ReLU mask, dbias) is read or written.  Boxes carry no gradient (:527-529).
 *   q, k, v, ld*, src_boxes, tgt_boxes, proj_weight, proj_bias, bool_mask, B .. attn_scale   as given to the forward;
 *         out / ldo and lse what it wrote
 *   dout  bf16 [B, N, ..] with row stride lddo (16-byte aligned, lddo % 8 == 0)
 *   workspace   rdetr_relation_attention_boxes_backward_workspace_bytes(B, H, N, M) bytes, 16-byte aligned (Di, one
 *         520-float partial record per image and 16 queries, and from N = 241 on four fp32 [B, M, 2 H D] partials of dk / dv:
 *         linear in N and M); 0 bytes for an empty problem
 *   dq [B, N, ..], dk / dv [B, M, ..]   bf16 with row strides lddq / lddk / lddv, 8-byte aligned, ld % 4 == 0: dq and dk may
 *         be the two halves of one packed [B, N, 2C] buffer (ld = 2C, dk = dq + C) when N == M
 *   grad_weight fp32 [H, 4F], grad_bias fp32 [H] or NULL   overwritten (no zero-fill by the caller), natural units
 * A fully masked row contributes nothing to dk / dv / grad_weight / grad_bias; its dq row is 0.
 * RDETR_ERR_INVALID_ARG: a NULL required pointer, B, H, D, N, M or F <= 0, a row stride below H * D, a short workspace.
 * RDETR_ERR_UNSUPPORTED: H != 8, D != 32, F != 16, a missed alignment.  All checks precede any HIP call. */
long long rdetr_relation_attention_boxes_backward_workspace_bytes(int B, int H, int N, int M);
int rdetr_relation_attention_boxes_backward_bf16(const uint16_t *q, const uint16_t *k, const uint16_t *v, int ldq, int ldk, int ldv,
                                                 const uint16_t *out, int ldo, const float *lse, const uint16_t *dout, int lddo,
                                                 const float *src_boxes, const float *tgt_boxes, const float *proj_weight,
                                                 const float *proj_bias, const uint8_t *bool_mask, int B, int H, int D, int N, int M,
                                                 int F, float rel_scale, float temperature, float eps, float attn_scale,
                                                 void *workspace, long long workspace_bytes, uint16_t *dq, int lddq, uint16_t *dk,
                                                 int lddk, uint16_t *dv, int lddv, float *grad_weight, float *grad_bias,
                                                 void *stream);

/* ---------------------------------------------------------------------------------------------
 * Residual add + LayerNorm over the last dimension, one pass (callers either side of the hot path).
 * Replaces the pairs  x + sublayer(x) -> nn.LayerNorm  of the encoder / decoder layers
 *           models/bricks/relation_transformer.py:262-276 (encoder layer), :452-478 (decoder layer), :360.
 *   x, residual (nullable), out  [rows, C]      gamma, beta [C]      all in one dtype (fp32 / bf16)
 *   out = (x + residual - mean) / sqrt(var + eps) * gamma + beta, statistics in fp32, biased variance
 *   (torch.nn.functional.layer_norm); the sum is not rounded to the storage type before normalising.
 * C = 256 with 16-byte-aligned pointers takes the vectorised kernel; any other C <= 8192 a strided one. */
int rdetr_add_layernorm_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                            long long rows, int C, float eps, float *out, void *stream);
int rdetr_add_layernorm_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma, const uint16_t *beta,
                             long long rows, int C, float eps, uint16_t *out, void *stream);
/* Same with row strides in ELEMENTS (ldx, ldr, ldo >= C): inputs / output may be column slices of wider matrices -- the
 * encoder writes each layer's output straight into its slice of the [rows, 7*C] memory-fusion input
 * (relation_transformer.py:196-214) instead of concatenating afterwards. */
int rdetr_add_layernorm_strided_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                                    long long rows, int C, long long ldx, long long ldr, long long ldo, float eps,
                                    float *out, void *stream);
int rdetr_add_layernorm_strided_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma,
                                     const uint16_t *beta, long long rows, int C, long long ldx, long long ldr,
                                     long long ldo, float eps, uint16_t *out, void *stream);

/* As the strided form, with a second output out2 = out + pos (the next encoder layer's `query + query_pos`,
 * models/bricks/relation_transformer.py:262): computed from the stored (rounded) `out`, i.e. the bits of a separate add.
 * pos / out2: rows ldp / ldo2 elements apart, both required. */
int rdetr_add_layernorm_pos_f32(const float *x, const float *residual, const float *gamma, const float *beta,
                                const float *pos, long long rows, int C, long long ldx, long long ldr, long long ldo,
                                long long ldp, long long ldo2, float eps, float *out, float *out2, void *stream);
int rdetr_add_layernorm_pos_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma,
                                 const uint16_t *beta, const uint16_t *pos, long long rows, int C, long long ldx,
                                 long long ldr, long long ldo, long long ldp, long long ldo2, float eps, uint16_t *out,
                                 uint16_t *out2, void *stream);

/* Training forms, C = 256 only (RDETR_ERR_UNSUPPORTED for any other C, or for operands off the 16-byte grid: pointers, and row
 * strides in bytes; there is no generic-C route -- the caller keeps its own).
 *   ..._train_*     the strided forward, same `out` bits, plus stats[rows, 2] fp32 = {mean, 1/sqrt(var + eps)} of every row.
 *   ..._backward_*  from dy [rows, 256] (rows lddy apart), the forward's x / residual (nullable) and stats:
 *                     xhat = (x + residual - mean) * rstd (the sum in fp32, unrounded),  g = dy * gamma,
 *                     dx [rows, 256] (contiguous) = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat))  -- the gradient of x AND of
 *                     residual;  dgamma = sum_rows dy * xhat,  dbeta = sum_rows dy  ([256], the operands' dtype).
 *                   dgamma and dbeta may both be null (frozen parameters): no workspace is needed and one kernel runs.  Otherwise
 *                   workspace holds per-workgroup fp32 partials that a second kernel adds in index order -- no atomics, the same bits
 *                   on every run; size from the _workspace_bytes function, 16-byte aligned, contents are scratch. */
int rdetr_add_layernorm_train_f32(const float *x, const float *residual, const float *gamma, const float *beta, long long rows,
                                  int C, long long ldx, long long ldr, long long ldo, float eps, float *out, float *stats,
                                  void *stream);
int rdetr_add_layernorm_train_bf16(const uint16_t *x, const uint16_t *residual, const uint16_t *gamma, const uint16_t *beta,
                                   long long rows, int C, long long ldx, long long ldr, long long ldo, float eps, uint16_t *out,
                                   float *stats, void *stream);
long long rdetr_add_layernorm_backward_workspace_bytes(long long rows);
int rdetr_add_layernorm_backward_f32(const float *dy, long long lddy, const float *x, long long ldx, const float *residual,
                                     long long ldr, const float *gamma, const float *stats, long long rows, int C, void *workspace,
                                     long long workspace_bytes, float *dx, float *dgamma, float *dbeta, void *stream);
int rdetr_add_layernorm_backward_bf16(const uint16_t *dy, long long lddy, const uint16_t *x, long long ldx,
                                      const uint16_t *residual, long long ldr, const uint16_t *gamma, const float *stats,
                                      long long rows, int C, void *workspace, long long workspace_bytes, uint16_t *dx,
                                      uint16_t *dgamma, uint16_t *dbeta, void *stream);

/* Mixed-precision training forms (bf16 autocast over fp32 parameters), C = 256 only: x and residual (nullable) are each fp32
 * (x_is_bf16 / r_is_bf16 = 0) or bf16 (1), rows ldx / ldr elements of their own type apart; gamma, beta, out (rows ldo apart), dy,
 * stats, dgamma and dbeta are fp32.  The sum x + residual is formed in fp32 and never stored; the arithmetic is that of the
 * same-dtype forms.  ..._backward_mixed writes dx [rows, 256] fp32 (contiguous) and, in the same pass, dx_bf16 [rows, 256]: the same
 * values rounded to bf16 (RNE) -- each operand's gradient in its own type.  dx_bf16 may be null only when no operand is bf16, dx
 * only when none is fp32 (RDETR_ERR_INVALID_ARG otherwise).  Workspace, the parameter-gradient reduction, its null form and the
 * 16-byte rules are those of rdetr_add_layernorm_backward_f32. */
int rdetr_add_layernorm_train_mixed(const void *x, int x_is_bf16, long long ldx, const void *residual, int r_is_bf16, long long ldr,
                                    const float *gamma, const float *beta, long long rows, int C, float eps, float *out,
                                    long long ldo, float *stats, void *stream);
int rdetr_add_layernorm_backward_mixed(const float *dy, long long lddy, const void *x, int x_is_bf16, long long ldx,
                                       const void *residual, int r_is_bf16, long long ldr, const float *gamma, const float *stats,
                                       long long rows, int C, void *workspace, long long workspace_bytes, float *dx,
                                       uint16_t *dx_bf16, float *dgamma, float *dbeta, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused elementwise steps of the decoder's box bookkeeping (each replaces ~8 torch launches on a [B,N,4] tensor).
 *   rdetr_box_refine_f32   out = sigmoid(delta + inverse_sigmoid(ref)),  inverse_sigmoid as util/misc.py:31-35 (eps 1e-3);
 *                          the iterative box refinement of models/bricks/relation_transformer.py:363-381.
 *                          delta: n values, fp32 (delta_is_bf16 = 0) or bf16 (1); ref, out: n fp32 values.
 *   rdetr_sine_pos_embed   get_sine_pos_embed(pos, num_pos_feats = F, temperature, scale, exchange_xy = True)
 *                          (models/bricks/position_encoding.py:101-138): pos fp32 [rows, n] -> out [rows, n * F] fp32 or bf16,
 *                          coordinate order (y, x, rest), channel = coord * F + 2k + {sin, cos}, F even, <= 128. */
int rdetr_box_refine_f32(const void *delta, int delta_is_bf16, const float *ref, long long n, float eps, float *out,
                         void *stream);
int rdetr_sine_pos_embed(const float *pos, long long rows, int n, int F, float temperature, float scale, void *out,
                         int out_is_bf16, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One-pass steps of the encoder's input / output side (each replaces a torch chain that made 2-3 passes over a [B,S,C] tensor).
 *   rdetr_zero_masked_rows  x.masked_fill_(mask[..., None], 0) in place: the padding fill of the projected value
 *                           (models/bricks/ms_deform_attn.py:316-319).  x: rows of row_bytes bytes, ld_bytes apart (both
 *                           multiples of 16, x 16-byte aligned), mask: one byte per row (non-zero = padded).  Only the padded
 *                           rows are written.
 *   rdetr_row_max           out[r] = max(x[r, 0..C)) (NaN propagates), x fp32 or bf16 [rows, C] with row stride ldx, out
 *                           [rows] in x's type: the class-score maximum of the two-stage query selection
 *                           (models/bricks/relation_transformer.py:105).
 *   rdetr_nchw_to_tokens    one pyramid level src [B, C, P] (P = H*W) -> out[b, p, c] = src[b, c, p] (+ add_vec[c]), i.e.
 *                           x.flatten(2).transpose(1, 2) (+ the level embedding, relation_transformer.py:87-89) written
 *                           straight into the level's rows of the level-packed token tensor (base_transformer.py:17-23):
 *                           `out` points at the level's first row of image 0; rows are ld_out elements apart (>= C), images
 *                           out_image_stride elements.  add_vec nullable.
 *   rdetr_nchw_levels_to_tokens   all L <= 8 levels of a pyramid in ONE launch: out [B, S, C] = cat over the levels of the above,
 *                           `out` pointing at row 0 of image 0.  level_src / level_vec: L HOST pointers to the levels' DEVICE
 *                           tensors [B, C, P_l] and vectors [C] (level_vec or any of its entries may be NULL); level_pixels: L
 *                           host ints P_l.  The tables travel in the kernel's argument block, so the call is one kernel node
 *                           of a captured graph.  Same values as the per-level calls. */
int rdetr_zero_masked_rows(void *x, const unsigned char *mask, long long rows, int row_bytes, long long ld_bytes,
                           void *stream);
int rdetr_row_max(const void *x, int is_bf16, long long rows, int C, long long ldx, void *out, void *stream);

/* Row-wise top-k (largest, sorted) for the two selections on the transformer's dependency chain:
 *   torch.topk(enc_outputs_class.max(-1)[0], 900, dim=1)    models/bricks/relation_transformer.py:93 (and :105 for the hybrid branch)
 *   torch.topk(prob.view(B, -1), 300, dim=1)                models/bricks/post_process.py:30
 *   x [rows, n] fp32 or bf16, contiguous  ->  values [rows, k] fp32, indices [rows, k] int64
 * Order: value descending, equal values by index ascending, NaN above everything (torch.topk leaves the order of equal values
 * unspecified).  1 <= k <= min(n, 1024), n < 2^20.  workspace: rdetr_topk_workspace_bytes(rows, n, k) bytes of scratch, 16-byte
 * aligned. */
long long rdetr_topk_workspace_bytes(int rows, int n, int k);
int rdetr_topk(const void *x, int is_bf16, int rows, int n, int k, void *workspace, float *values, long long *indices, void *stream);

/* The decoder's box head and box refinement in one kernel (bf16 activations, embed_dim 256):
 *   out = sigmoid(W3 relu(W2 relu(W1 x + b1) + b2) + b3 + inverse_sigmoid(reference))
 * Replaces bbox_head[i] = MLP(256, 256, 4, 3) (models/bricks/basic.py:6-24, relation_transformer.py:294) followed by the
 * refinement of relation_transformer.py:363-381 (inverse_sigmoid: util/misc.py:31-35), for the layer's two calls at once:
 *   xa [M, 256] -> out_a [M, 4] (the layer's boxes, from norm(query)),  xb [M, 256] or NULL -> out_b (the next reference points)
 *   pw1, pw2   the hidden weights [256, 256] packed by rdetr_linear_pack_k256_bf16;  b1, b2 [256], w3 [4, 256], b3 [4]   bf16
 *   reference  fp32 [M, 4] (shared by both inputs), eps of inverse_sigmoid;  outputs fp32.  lda / ldb: row strides in elements.
 *   reference_is_logit != 0: the reference is in logit space already and is added as it is -- the two-stage proposal boxes
 *              sigmoid(encoder_bbox_head(output_memory) + output_proposals), relation_transformer.py:88-90
 * Hidden activations and the final delta are rounded to bf16 where the unfused path stores them. */
int rdetr_box_head_k256_bf16(const uint16_t *xa, long long lda, const uint16_t *xb, long long ldb, const uint16_t *pw1,
                             const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2, const uint16_t *w3, const uint16_t *b3,
                             const float *reference, int reference_is_logit, float eps, long long M, float *out_a, float *out_b,
                             void *stream);

/* rdetr_box_head_k256_bf16 plus the layer's class head on input A (class_head[i] = nn.Linear(256, C), relation_transformer.py:358)
 * in the same launch:  out_cls [M, C] = xa Wc^T + bc, bf16, row stride ldc elements (>= C; rows need no alignment beyond 2 bytes).
 *   pwc  class_head[i].weight [C, 256] zero-padded to [256, 256] and packed by rdetr_linear_pack_k256_bf16;  bc [C] bf16
 *   1 <= C <= 256 (anything larger is RDETR_ERR_UNSUPPORTED).  Same products and fp32 accumulation as the GEMM it replaces,
 *   rounded to bf16 once; out_a / out_b are bit for bit what rdetr_box_head_k256_bf16 writes. */
int rdetr_box_head_cls_k256_bf16(const uint16_t *xa, long long lda, const uint16_t *xb, long long ldb, const uint16_t *pw1,
                                 const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2, const uint16_t *w3, const uint16_t *b3,
                                 const float *reference, int reference_is_logit, float eps, const uint16_t *pwc, const uint16_t *bc,
                                 int C, long long M, float *out_a, float *out_b, uint16_t *out_cls, long long ldc, void *stream);

/* The decoder layer's query position in one launch (models/bricks/relation_transformer.py:294-296, 343-347, 452-455):
 *     out_pos = ref_point_head(emb)                      MLP(512, 256, 256, 2) on the sine embedding of the reference boxes
 *     out_pos = out_pos * query_scale(query)             MLP(256, 256, 256, 2), layers >= 1 -- when pv1 / c1 / pv2 / c2 are given
 *     out_qpp = query + out_pos                          the q = k input of the layer's self-attention
 * emb [M, 512], query [M, 256] bf16 (row strides lde / ldq elements, multiples of 8, 16-byte aligned bases); pw1a / pw1b = the
 * K halves [:, :256] / [:, 256:] of ref_point_head.layers[0].weight [256, 512], pw2 = ref_point_head.layers[1].weight, pv1 / pv2 =
 * query_scale's two [256, 256] weights -- each packed by rdetr_linear_pack_k256_bf16; b1, b2, c1, c2 bf16 [256];
 * out_pos, out_qpp [M, 256] bf16 contiguous.  Every intermediate is rounded to bf16 where the unfused sequence (four GEMMs, a
 * product, a sum) stores it. */
int rdetr_query_pos_k256_bf16(const uint16_t *emb, long long lde, const uint16_t *query, long long ldq, const uint16_t *pw1a,
                              const uint16_t *pw1b, const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2, const uint16_t *pv1,
                              const uint16_t *c1, const uint16_t *pv2, const uint16_t *c2, long long M, uint16_t *out_pos,
                              uint16_t *out_qpp, void *stream);

/* rdetr_query_pos_k256_bf16 plus the in-projection of the layer's self-attention (nn.MultiheadAttention's in_proj_weight [768, 256],
 * in_proj_bias [768]; relation_transformer.py:452-455 calls it with q = k = query + query_pos, value = query) in the same launch:
 *     out_qk [M, 512] = out_qpp [Wq ; Wk]^T + bias[:512]          computed from out_qpp as stored (bf16)
 *     out_v  [M, 256] = query Wv^T + bias[512:]
 * pwq / pwk / pwv = in_proj_weight[:256] / [256:512] / [512:], each packed by rdetr_linear_pack_k256_bf16; bias bf16 [768]; outputs
 * bf16 with row strides ldqk >= 512 / ldv >= 256 elements (multiples of 8, 16-byte aligned bases).  out_pos / out_qpp are bit for bit
 * what rdetr_query_pos_k256_bf16 writes. */
int rdetr_query_pos_inproj_k256_bf16(const uint16_t *emb, long long lde, const uint16_t *query, long long ldq, const uint16_t *pw1a,
                                     const uint16_t *pw1b, const uint16_t *b1, const uint16_t *pw2, const uint16_t *b2, const uint16_t *pv1,
                                     const uint16_t *c1, const uint16_t *pv2, const uint16_t *c2, const uint16_t *pwq, const uint16_t *pwk,
                                     const uint16_t *pwv, const uint16_t *bias, long long M, uint16_t *out_pos, uint16_t *out_qpp,
                                     uint16_t *out_qk, long long ldqk, uint16_t *out_v, long long ldv, void *stream);

/* The three input projections of an ENCODER layer's MultiScaleDeformableAttention in one launch
 * (models/bricks/ms_deform_attn.py:315-327; called from relation_transformer.py:262-269 with value = query, query = query + pos):
 *     out_hm [B, 8, S, 32] = head-major(value_proj(x)), rows of padded positions zero        (:315-321)
 *     out_q  [B*S, q_cols] = [sampling_offsets ; attention_weights](xq), raw outputs          (:322-327; the fused gather reads the
 *                                                                                              two column slices in place)
 * q_cols = 3 * heads * levels * points = 384 (4 feature levels) or 480 (5: the FocalNet configuration); anything else is
 * RDETR_ERR_UNSUPPORTED.
 * x, xq [B*S, 256] bf16 (row strides ldx / ldq elements, multiples of 8, 16-byte aligned bases); pwv = value_proj.weight packed by
 * rdetr_linear_pack_k256_bf16; pwq = [sampling_offsets.weight ; attention_weights.weight ; zero rows] = [512, 256] as two packed
 * [256, 256] blocks, one after the other; bv [256] / bq [q_cols] bf16 or NULL; row_mask = key_padding_mask u8 [B*S] or NULL.
 * Replaces rdetr_linear_k256_hm_bf16 + one N = q_cols GEMM: same products, fp32 accumulation, outputs rounded to bf16 once. */
int rdetr_encoder_proj_k256_bf16(const uint16_t *x, long long ldx, const uint16_t *xq, long long ldq, const uint16_t *pwv,
                                 const uint16_t *bv, const uint16_t *pwq, const uint16_t *bq, const uint8_t *row_mask, int B, int S,
                                 int q_cols, uint16_t *out_hm, uint16_t *out_q, void *stream);

/* PostProcess after its top-k (models/bricks/post_process.py:30-44) in one launch: for rank r of image b
 *   out[b][r] = (x1, y1, x2, y2, score, label) with box = boxes[b][index / C] (cxcywh in [0, 1]) converted to xyxy and scaled by the
 *   image's (w, h), label = index % C.   score fp32 [B, K], index int64 [B, K], boxes fp32 [B, N, 4], image_sizes int64 [B, 2] (h, w). */
int rdetr_detections_from_topk(const float *score, const long long *index, const float *boxes, const long long *image_sizes, int B,
                               int N, int C, int K, float *out, void *stream);

/* query_pos = a * scale and query + query_pos (models/bricks/relation_transformer.py:346-347, 452) in one pass over n contiguous
 * elements (fp32 or bf16); the product is rounded to the storage type before the add, as the two torch kernels it replaces do. */
int rdetr_scaled_pos(const void *a, const void *scale, const void *query, long long n, int is_bf16, void *pos, void *qp, void *stream);

/* Entry of a decoder layer (models/bricks/relation_transformer.py:335-343) in one launch:
 *   ref_in [B, N, L, 4] = reference [B, N, 4] * (vr[b][l].x, vr[b][l].y, vr[b][l].x, vr[b][l].y)       valid_ratios vr [B, L, 2]
 *   emb    [B, N, 4 F]  = get_sine_pos_embed(ref_in[:, :, 0, :], F, temperature, scale, exchange_xy=True)  (fp32 or bf16) */
int rdetr_decoder_reference(const float *reference, const float *valid_ratios, int B, int N, int L, int F, float temperature,
                            float scale, float *ref_in, void *emb, int emb_is_bf16, void *stream);

/* Pyramid geometry of the two-stage transformer in two launches (the torch sequences are ~40 small launches per forward):
 *   valid_ratios [B, L, 2]    unpadded fraction of each level's width / height         models/bricks/base_transformer.py:42-51
 *   reference    [B, S, L, 2] every position's centre, scaled by the valid ratios      base_transformer.py:57-70
 *   logit        [B, S, 4]    inverse sigmoid of the position's proposal box (centre, 0.05 * 2^level), +inf where the proposal
 *                             is not inside (0.01, 0.99) or the position is padded      relation_transformer.py:162-176
 *   keep         [B, S]       1 / 0 (fp32 or bf16): the factor the encoder memory is multiplied with before enc_output
 * level_masks: L HOST pointers to the levels' DEVICE bool masks [B, h_l, w_l]; level_hw: 2 L host ints (h, w); pad_mask
 * [B, S] u8 (the flattened masks) or NULL.  L <= 8. */
int rdetr_pyramid_points(const unsigned char *const *level_masks, const int *level_hw, int L, int B, const unsigned char *pad_mask,
                         int keep_is_bf16, float *valid_ratios, float *reference, float *logit, void *keep, void *stream);
int rdetr_nchw_to_tokens(const void *src, const void *add_vec, int is_bf16, int B, int C, int P,
                         long long out_image_stride, long long ld_out, void *out, void *stream);
int rdetr_nchw_levels_to_tokens(const void *const *level_src, const void *const *level_vec, const int *level_pixels, int L,
                                int is_bf16, int B, int C, long long out_image_stride, long long ld_out, void *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Dense projection with K = 256 (embed_dim) for tall bf16 inputs, hand-written MFMA kernel (csrc/linear.hip):
 *   out[M, N] = act(x[M, 256] w[N, 256]^T + bias[N]),  bf16 storage, fp32 accumulation, one rounding.
 * Replaces the library GEMM behind nn.Linear for MSDA's value_proj / output_proj / merged sampling_offsets + attention_weights
 * projection (models/bricks/ms_deform_attn.py:259-262) and the FFN's linear1 + ReLU (models/bricks/relation_transformer.py:226-233).
 *   x: rows ldx elements apart (>= 256), w: [N, 256] contiguous (nn.Linear.weight), bias: [N] or NULL, out: rows ldo apart;
 *   N a multiple of 32, ldx / ldo multiples of 8, bases 16-byte aligned (else RDETR_ERR_UNSUPPORTED); relu: 0 | 1. */
int rdetr_linear_k256_bf16(const uint16_t *x, long long ldx, const uint16_t *w, const uint16_t *bias, long long M, int N,
                           int relu, uint16_t *out, long long ldo, void *stream);

/* MSDA's output_proj with the encoder layer's residual + LayerNorm in its epilogue (csrc/linear.hip):
 *   out[M, 256] = LayerNorm(residual + (x[M, 256] w[256, 256]^T + bias))     (models/bricks/ms_deform_attn.py:372-376 followed by
 *   norm1(query + attn), relation_transformer.py:262-271); the projection is rounded to bf16 before the residual is added, as the
 *   unfused path stores it; fp32 two-pass statistics.  The weight is re-ordered once per weight update by
 *   rdetr_linear_pack_k256_bf16 (`packed`: 65,536 bf16 elements).  Rows ldx / ldr / ldo elements apart (multiples of 8), bases
 *   16-byte aligned; bias nullable; gamma / beta [256] bf16. */
int rdetr_linear_pack_k256_bf16(const uint16_t *w, uint16_t *packed, void *stream);
int rdetr_linear_ln_k256_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *bias,
                              const uint16_t *residual, long long ldr, const uint16_t *gamma, const uint16_t *beta, float eps,
                              long long M, uint16_t *out, long long ldo, void *stream);

/* A decoder layer's attention output projection + residual + LayerNorm in one launch, for SHORT row counts (csrc/rowtail.hip; 32 rows
 * per workgroup where the kernel above has 256-row tiles):
 *   out    [M, 256] = LayerNorm(residual + bf16(x[M, 256] w[256, 256]^T + bias); gamma, beta, eps)
 *   out_pos[M, 256] = out + pos                                   when pos != NULL      (relation_transformer.py:452-463)
 * self_attn.out_proj + norm2 (+ query_pos) and cross_attn.output_proj + norm1 of the decoder layer.
 *   packed  w re-ordered by the pack entry above; row strides in elements, multiples of 8; every base and parameter vector 16-byte
 *   aligned (anything else: RDETR_ERR_UNSUPPORTED); bias nullable; all bf16, fp32 accumulation and statistics.  M == 0: RDETR_OK,
 *   no launch.
 * The projection is rounded to bf16 before the residual is added and the sum is not rounded again: for the same sums `out` has the
 * bits of the add + LayerNorm entries. */
int rdetr_linear_ln_rows_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *bias,
                              const uint16_t *residual, long long ldr, const uint16_t *gamma, const uint16_t *beta, float eps,
                              const uint16_t *pos, long long ldp, long long M, uint16_t *out, long long ldo, uint16_t *out_pos,
                              long long ldop, void *stream);

/* Fused feed-forward block (csrc/ffn.hip): out[M, 256] = relu(x[M, 256] w1[F, 256]^T + b1[F]) w2[256, F]^T + b2[256], i.e.
 * linear2(relu(linear1(x))) of the encoder / decoder layers (models/bricks/relation_transformer.py:226-233, 272-275) without the
 * [M, F] activations ever reaching HBM.  bf16 storage, fp32 accumulation, the hidden activations rounded to bf16 where the unfused
 * path stores them.  The two weight matrices (as nn.Linear keeps them, contiguous) are first re-ordered ONCE per weight update
 * into the order the kernel streams them: rdetr_ffn_k256_pack_bf16 fills `packed` (2 * 256 * F bf16 elements, 16-byte aligned).
 * x / out rows ldx / ldo elements apart (multiples of 8, 16-byte aligned bases); F a multiple of 64, <= 4096 (else
 * RDETR_ERR_UNSUPPORTED). */
int rdetr_ffn_k256_pack_bf16(const uint16_t *w1, const uint16_t *w2, int F, uint16_t *packed, void *stream);
int rdetr_ffn_k256_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                        long long M, int F, uint16_t *out, long long ldo, void *stream);
/* The same block with the layer's closing residual + LayerNorm in its epilogue: out = LayerNorm(x + ffn(x)) with gamma / beta [256]
 * bf16 and eps (relation_transformer.py:272-276; ffn(x) rounded to bf16 first, as the unfused path stores it; fp32 two-pass
 * statistics).  pos / out2 (both or neither, rows ldp / ldo2 apart): out2 = out + pos, the next layer's query + query_pos. */
int rdetr_ffn_ln_k256_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                           const uint16_t *gamma, const uint16_t *beta, float eps, const uint16_t *pos, long long ldp,
                           long long M, int F, uint16_t *out, long long ldo, uint16_t *out2, long long ldo2, void *stream);
/* Training route of the block (bf16).  rdetr_ffn_k256_train_bf16 is rdetr_ffn_k256_bf16 (the same kernel body, the same out bits)
 * that also stores the hidden activations hid[M, F] = relu(bf16(x w1^T + b1)), rows ldh apart.  rdetr_ffn_k256_backward_bf16 is the
 * data gradient from those: dh[M, F] = bf16(dy w2) where hid > 0, else 0 (rows ldd apart), and dx[M, 256] = dh w1, accumulated in
 * fp32 over all of F and rounded once -- the rounding points of autograd over the two library GEMMs.  packed_t is
 * rdetr_ffn_k256_pack_bf16(w2^T [F, 256], w1^T [256, F]) (contiguous transposed copies).  The weight and bias gradients
 * (dy^T hid, dh^T x and the column sums) are left to the caller.  ldh, ldd >= F, multiples of 8, 16-byte aligned bases;
 * M * ldh * 2 and M * ldd * 2 below 2^31 (hid / dh are addressed with 32-bit byte offsets), else RDETR_ERR_UNSUPPORTED.
 * Rows at or beyond M are neither read nor written.  No atomics: two runs agree bit for bit. */
int rdetr_ffn_k256_train_bf16(const uint16_t *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                              long long M, int F, uint16_t *out, long long ldo, uint16_t *hid, long long ldh, void *stream);
int rdetr_ffn_k256_backward_bf16(const uint16_t *dy, long long lddy, const uint16_t *packed_t, const uint16_t *hid, long long ldh,
                                 long long M, int F, uint16_t *dh, long long ldd, uint16_t *dx, long long lddx, void *stream);
/* The training route with fp32 at either end of the block (bf16 autocast over fp32 parameters and an fp32 residual stream).
 *   rdetr_ffn_k256_pack_f32             rdetr_ffn_k256_pack_bf16 from fp32 matrices given by element strides (row, column; >= 1),
 *                                       rounded to bf16 (RNE) on the way: w1 is read as [F, 256], w2 as [256, F].  With the strides
 *                                       exchanged the backward's (w2^T, w1^T) are read in place.  b1 [F], b2 [256] (fp32, contiguous)
 *                                       are rounded into biases_bf16 [F + 256] = (b1, b2); the three are given together or not at all.
 *   rdetr_ffn_k256_train_xf32_bf16      rdetr_ffn_k256_train_bf16 on fp32 rows x (ldx a multiple of 4): they are rounded to bf16 (RNE)
 *                                       as they are loaded and the rounded rows also stored as xlp [M, 256] bf16 (rows ldxl apart, a
 *                                       multiple of 8) -- out and hid have the bits of rdetr_ffn_k256_train_bf16 on xlp.
 *   rdetr_ffn_k256_backward_dxf32_bf16  rdetr_ffn_k256_backward_bf16 whose dx [M, 256] (rows lddx apart, a multiple of 4) is the fp32
 *                                       sum over all of F, not rounded; dh as there.
 * Every base is 16-byte aligned (the fp32 weights and biases of the pack: 4-byte); the limits on F, M * ldh and M * ldd and the
 * status conventions are those of the bf16 entries. */
int rdetr_ffn_k256_pack_f32(const float *w1, long long w1_row_stride, long long w1_col_stride, const float *w2,
                            long long w2_row_stride, long long w2_col_stride, const float *b1, const float *b2, int F,
                            uint16_t *packed, uint16_t *biases_bf16, void *stream);
int rdetr_ffn_k256_train_xf32_bf16(const float *x, long long ldx, const uint16_t *packed, const uint16_t *b1, const uint16_t *b2,
                                   long long M, int F, uint16_t *out, long long ldo, uint16_t *hid, long long ldh, uint16_t *xlp,
                                   long long ldxl, void *stream);
int rdetr_ffn_k256_backward_dxf32_bf16(const uint16_t *dy, long long lddy, const uint16_t *packed_t, const uint16_t *hid,
                                       long long ldh, long long M, int F, uint16_t *dh, long long ldd, float *dx, long long lddx,
                                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training criterion (csrc/criterion.hip): the matcher's cost matrices and the set losses of a STACK of prediction sets.
 * Replaces, per set and image, HungarianMatcher.calculate_cost (models/matcher/hungarian_matcher.py:41-70) and, per set,
 * HybridSetCriterion.loss_labels + SetCriterion.loss_boxes with vari_sigmoid_focal_loss (models/bricks/set_criterion.py:84-106,
 * 178-216, models/bricks/losses.py:15-21) and their autograd.  The assignment itself stays on the host.
 *
 * A stack is R rows of N queries; row r belongs to image r % B (rows = layers x images).  logits [R, N, C] fp32 or bf16 and
 * boxes [R, N, 4] fp32 (cxcywh) are contiguous inside a row, rows ld_logits / ld_boxes ELEMENTS apart (>= N * C, >= N * 4), so a
 * query slice of a taller tensor is taken in place.  The ground truth is padded per image: gt_boxes [B, Gmax, 4] fp32 cxcywh,
 * gt_labels [B, Gmax] int32, gt_count [B] int32.  A label outside [0, C) is never used as an index: its class term is 0.
 * fp32 math; boxes bases 16-byte aligned and ld_boxes a multiple of 4, Gmax <= 2048, R <= 65535 (else RDETR_ERR_UNSUPPORTED).
 *
 * rdetr_match_cost_*: cost [R, N, Gmax] fp32 = w_bbox * L1 + w_class * (focal positive - focal negative cost at the gt's class,
 *   1e-6 inside the logs, 1 - p formed as sigmoid(-x)) + w_giou * (-GIoU); columns g >= gt_count[r % B] are written as 0.
 *
 * rdetr_set_loss_*: match [R, N] int32 holds each query's gt index in its image's table, or -1 (an index >= Gmax counts as -1).
 *   Queries n < n_split form segment 0 (the denoising queries) and are scaled by inv_norm_a, the rest segment 1, by inv_norm_b.
 *     sums      [R, 2, 3] fp32   per row and segment {varifocal class loss, L1, GIoU loss}, each times the segment's inv_norm
 *     dlogits   [R, N, C]        d sums[r, seg, 0] / d logits, in the logits' dtype, contiguous
 *     dbox_l1   [R, N, 4] fp32   d sums[r, seg, 1] / d boxes      dbox_giou [R, N, 4] fp32  d sums[r, seg, 2] / d boxes
 *   (zero rows where unmatched).  The class target is the detached IoU of the matched pair, the focal weight is detached, as in
 *   the reference, so these are the complete gradients.  ws: rdetr_set_loss_workspace_bytes(R, N) bytes of per-workgroup partial
 *   sums, added in a fixed order by a second launch: no atomics, the same bits on every run. */
int rdetr_match_cost_f32(const float *logits, long long ld_logits, const float *boxes, long long ld_boxes, const float *gt_boxes,
                         const int *gt_labels, const int *gt_count, int R, int B, int N, int C, int Gmax, float alpha, float gamma,
                         float w_class, float w_bbox, float w_giou, float *cost, void *stream);
int rdetr_match_cost_bf16(const uint16_t *logits, long long ld_logits, const float *boxes, long long ld_boxes, const float *gt_boxes,
                          const int *gt_labels, const int *gt_count, int R, int B, int N, int C, int Gmax, float alpha, float gamma,
                          float w_class, float w_bbox, float w_giou, float *cost, void *stream);
long long rdetr_set_loss_workspace_bytes(int R, int N);
int rdetr_set_loss_f32(const float *logits, long long ld_logits, const float *boxes, long long ld_boxes, const int *match,
                       const float *gt_boxes, const int *gt_labels, int R, int B, int N, int C, int Gmax, int n_split, float inv_norm_a,
                       float inv_norm_b, float alpha, float gamma, void *ws, long long ws_bytes, float *sums, float *dlogits,
                       float *dbox_l1, float *dbox_giou, void *stream);
int rdetr_set_loss_bf16(const uint16_t *logits, long long ld_logits, const float *boxes, long long ld_boxes, const int *match,
                        const float *gt_boxes, const int *gt_labels, int R, int B, int N, int C, int Gmax, int n_split, float inv_norm_a,
                        float inv_norm_b, float alpha, float gamma, void *ws, long long ws_bytes, float *sums, uint16_t *dlogits,
                        float *dbox_l1, float *dbox_giou, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The matcher's assignment on the device (csrc/assign.hip).  Replaces, per set and image, scipy's linear_sum_assignment in
 * HungarianMatcher.forward (models/matcher/hungarian_matcher.py:72-100) and the host-built match table of the criterion.
 *
 * cost [R, N, Gmax] fp32 contiguous is what rdetr_match_cost_* fills; row r belongs to image r % B (R a multiple of B) and uses
 * the first g = gt_count[r % B] columns (clamped to [0, Gmax]).  One workgroup solves the rectangular assignment of the
 * N x (g * repeat) matrix whose column k is cost column k % g (the hybrid branch's repeated targets, never materialised), by the
 * shortest-augmenting-path method scipy runs, in its arithmetic (fp64 duals and path costs over the fp32 costs): min(N, g *
 * repeat) pairs of minimal total cost, scipy's own pairs wherever the optimum is unique.  Among equal minima a search prefers a
 * free column, then the lower index; the result depends on the inputs alone.  No atomics, no workspace.
 *
 *   match  [R, >= skip + N] int32, rows ld_match elements apart; all of a row's first skip + N entries are written, nothing else:
 *          entry skip + q the gt index (modulo g) of query q or -1; entry grp * dn_max_gt + t of the first skip = dn_groups *
 *          dn_max_gt (the fixed matches of the denoising queries) t where t < g, else -1.  g = 0: the whole row -1.
 *   status [R] int32: 0, or 1 where a cost of the row's used columns is NaN or an infinity (scipy raises there): the row's
 *          matcher entries are then all -1, its denoising entries as above, and every other row is unaffected.
 *
 * Every loop of the kernel is bounded by the sizes, whatever the cost bits.  N <= 2048 and Gmax * repeat <= 2048 (else
 * RDETR_ERR_UNSUPPORTED, nothing launched); bases 4-byte aligned; R = 0 returns RDETR_OK without a launch. */
int rdetr_assign_match(const float *cost, const int *gt_count, int R, int B, int N, int Gmax, int repeat, int skip, int dn_groups,
                       int dn_max_gt, int *match, long long ld_match, int *status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Denoising query generator (csrc/denoising.hip, csrc/cdn_noise.h): GenerateCDNQueries.forward
 * (models/bricks/denoising.py:180-331) without its loops over images and groups, its host-built index tensors and its two
 * scatter assignments.  The caller allocates; nothing here allocates or waits for the device; zero work returns RDETR_OK without
 * a launch.
 *
 * The ground truth of the B images is flat: gt_labels [G] int64, gt_boxes [G, 4] fp32 cxcywh, gt_offset [B + 1] int32 the
 * exclusive prefix sum of the per-image counts G_b (gt_offset[B] = G; G is also passed by value).  max_gt = max G_b,
 * Ndn = 2 * groups * max_gt queries per image, Q = 2 * groups * G flat rows.  Slot (b, j) with i = j / max_gt, t = j % max_gt is
 * padding when t >= G_b (or when the offset table would lead outside [0, G)); else it belongs to flat row r = i * G +
 * gt_offset[b] + t and gt gt_offset[b] + t, a positive copy for even i and a negative one for odd i.
 *
 * rdetr_cdn_queries_*: embed [C, d] fp32 or bf16, d a multiple of 4 (fp32) or 8 (bf16), rows moved as 16-byte vectors.
 *     label_query  [B, Ndn, d]  embed[label], label = label_r[r] if label_u[r] < label_noise_prob * 0.5 else the gt label; a
 *                               zero row for padding and for a label outside [0, C), which is never used as an index
 *     box_query    [B, Ndn, 4]  fp32: corners +- noise, clamp to [0, 1], back to cxcywh, inverse_sigmoid with eps 1e-3, in the
 *                               reference's operation order (only logf may differ from torch in fp32); zeros for padding
 *     noised_label [B, Ndn]     int32, -1 for padding and for a label outside [0, C): what the backward reads
 *   Every element of the three is written.  The noise is either the reference's four draws in its flat layout (keyed = 0):
 *   label_u [Q] fp32 of rand_like, label_r [Q] int64 of randint_like(0, C), box_sign [Q, 4] fp32 in {0, 1} of randint_like(0, 2),
 *   box_u [Q, 4] fp32 of rand_like -- the label pair may be NULL when label_noise_prob <= 0, the box pair when box_noise_scale
 *   <= 0, which also skips the corner round trip -- or (keyed = 1) generated in registers from key as rdetr_cdn_noise writes it.
 *
 * rdetr_cdn_mask: mask [T, T] uint8 / bool, T = groups * group_size + num_queries, group_size = 2 * max_gt:
 *   mask[r, c] = c < Ndn and (r >= Ndn or r / group_size != c / group_size); base 4-byte aligned, T <= 46340.
 *
 * rdetr_cdn_embed_backward_*: grad_embed [C, d] from grad_label_query [rows, d] (contiguous) and noised_label [rows].  All of
 *   grad_embed is written, zero rows for unused classes.  No atomics: each class adds its rows in ascending order into an fp32
 *   accumulator with Kahan compensation (bf16 rounded once at the end), so the result is the same bits on every run.
 *
 * rdetr_cdn_noise: the four draws of key.  Philox4x32-10 under the key's low and high words; counter (r, 0, 0, 0) gives a0..a3,
 *   counter (r, 1, 0, 0) gives b0..b3; label_u = (a0 >> 8) * 2^-24, label_r = (uint64(a1) * C) >> 32, box_sign[k] = bit k of a2,
 *   box_u[k] = (b_k >> 8) * 2^-24.  Q < 2^31. */
int rdetr_cdn_queries_f32(const long long *gt_labels, const float *gt_boxes, const int *gt_offset, int B, int G, int max_gt, int groups,
                          int C, int d, float label_noise_prob, float box_noise_scale, const float *embed, const float *label_u,
                          const long long *label_r, const float *box_sign, const float *box_u, int keyed, unsigned long long key,
                          float *label_query, float *box_query, int *noised_label, void *stream);
int rdetr_cdn_queries_bf16(const long long *gt_labels, const float *gt_boxes, const int *gt_offset, int B, int G, int max_gt, int groups,
                           int C, int d, float label_noise_prob, float box_noise_scale, const uint16_t *embed, const float *label_u,
                           const long long *label_r, const float *box_sign, const float *box_u, int keyed, unsigned long long key,
                           uint16_t *label_query, float *box_query, int *noised_label, void *stream);
int rdetr_cdn_mask(int groups, int group_size, int num_queries, unsigned char *mask, void *stream);
int rdetr_cdn_embed_backward_f32(const float *grad_label_query, const int *noised_label, int rows, int C, int d, float *grad_embed,
                                 void *stream);
int rdetr_cdn_embed_backward_bf16(const uint16_t *grad_label_query, const int *noised_label, int rows, int C, int d, uint16_t *grad_embed,
                                  void *stream);
int rdetr_cdn_noise(unsigned long long key, int Q, int C, float *label_u, long long *label_r, float *box_sign, float *box_u, void *stream);

/* ---- optimizer step: clip_grad_norm_ + AdamW over a whole parameter set (csrc/optim.hip) ---------------------------------------
 * The rest of the reference's step (util/engine.py:57-61, configs/train_config.py:14,42-46) in three launches whatever the tensor
 * count, fp32, no atomics, the same bits on every run.  Three tables in device memory, 8-byte aligned, drive the launches:
 *
 *   tensors   [n_tensors]  built once: addresses of param, exp_avg, exp_avg_sq (fp32, contiguous), numel, and aligned16 != 0 when all
 *                          three addresses are 16-byte aligned
 *   steps     [n_tensors]  rewritten every step: the gradient's address (NULL: no gradient, the tensor is skipped) and the scalars of
 *                          the tensor's parameter group as torch's single-tensor AdamW forms them in doubles, rounded to fp32:
 *                          decay = 1 - lr * wd, 1 - beta1, beta2, 1 - beta2, step_size = lr / (1 - beta1^t), bias2_sqrt =
 *                          sqrt(1 - beta2^t), eps
 *   chunk_map [n_chunks]   chunk c covers elements [first, min(first + chunk, numel)) of tensor `tensor`; first is a multiple of
 *                          chunk, chunk a multiple of 4 (else RDETR_ERR_UNSUPPORTED), so a chunk never crosses a tensor.  An entry
 *                          whose tensor is outside [0, n_tensors) is skipped, never used as an index.
 *
 * Tensors whose three addresses and gradient are 16-byte aligned move as 16-byte vectors with a scalar numel % 4 tail, the others
 * element by element.  One workgroup owns a chunk; the grid is min(n_chunks, max_blocks) workgroups (max_blocks <= 0: 2048) that
 * walk the chunks with a stride, which changes no result.
 *
 * rdetr_optim_workspace_bytes(n_chunks): (n_chunks + 2) floats, the partials and behind them {total_norm, coef}.
 * rdetr_grad_sqnorm_f32: ws[c] = the sum of squares of chunk c's gradient elements (0 without a gradient): a chain per lane and
 *   vector component, then the lanes by shuffle, then the waves through LDS.
 * rdetr_grad_clip_coef: one workgroup adds ws[0 .. n_chunks) in index order in fp64 and writes ws[n_chunks] = total_norm,
 *   ws[n_chunks + 1] = coef = min(1, max_norm / (total_norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s formula.  Nothing goes to the
 *   host.
 * rdetr_adamw_step_f32: per element g = grad * coef (norm_coef[1]; 1 when norm_coef is NULL), param *= decay, exp_avg += (1 - beta1)
 *   (g - exp_avg), exp_avg_sq = exp_avg_sq beta2 + (1 - beta2) g g, param -= step_size exp_avg / (sqrt(exp_avg_sq) / bias2_sqrt + eps).
 *   Writes param, exp_avg and exp_avg_sq; the gradient is only read and keeps its unclipped value. */
typedef struct rdetr_optim_tensor {
    void *param, *exp_avg, *exp_avg_sq;
    long long numel;
    int aligned16, reserved;
} rdetr_optim_tensor;
typedef struct rdetr_optim_step {
    const void *grad;
    float decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bias2_sqrt, eps, reserved;
} rdetr_optim_step;
typedef struct rdetr_optim_chunk {
    long long first;
    int tensor, reserved;
} rdetr_optim_chunk;
long long rdetr_optim_workspace_bytes(int n_chunks);
int rdetr_grad_sqnorm_f32(const rdetr_optim_tensor *tensors, const rdetr_optim_step *steps, const rdetr_optim_chunk *chunk_map, int n_tensors,
                          int n_chunks, int chunk, int max_blocks, void *ws, long long ws_bytes, void *stream);
int rdetr_grad_clip_coef(void *ws, long long ws_bytes, int n_chunks, float max_norm, void *stream);
int rdetr_adamw_step_f32(const rdetr_optim_tensor *tensors, const rdetr_optim_step *steps, const rdetr_optim_chunk *chunk_map, int n_tensors,
                         int n_chunks, int chunk, int max_blocks, const float *norm_coef, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The neck's GroupNorm over a whole pyramid, the per-level padding masks and the sine position encoding (csrc/neck.hip;
 * models/necks/channel_mapper.py, models/detectors/base_detector.py:153-165, models/bricks/position_encoding.py:9-68).
 *
 * Every table argument is a HOST array of L <= 8 entries: pointers to the levels' DEVICE tensors, level_hw 2 L ints (h, w).  The
 * tables travel in the kernels' argument blocks.
 *
 * GroupNorm.  x[l], y[l], dy[l], dx[l]: contiguous [B, C, h_l, w_l], fp32 or bf16; gamma[l], beta[l]: [C] fp32 (the bf16 entry
 * points also take them in bf16, params_bf16 = 1); C % G == 0 and C / G <= 16, else RDETR_ERR_UNSUPPORTED.  mean, rstd: [L][B][G]
 * fp32.  ws: rdetr_neck_workspace_bytes bytes (-1 for sizes the kernels refuse), shared by forward and backward.
 *   forward   launch 1: one workgroup per 4096 elements of one (level, image, group) writes that chunk's (count, mean, M2), the mean
 *             first and M2 about it.  Launch 2: every workgroup combines its group's triples in index order with Chan's formula,
 *             writes y = (x - mean) rstd gamma[c] + beta[c] in x's type and, for chunk 0, mean and rstd = 1 / sqrt(M2 / n + eps).
 *   backward  launch 1: per (level, image, channel, 4096-pixel chunk) sum dy and sum dy xhat, xhat = (x - mean) rstd.  Launch 2:
 *             per group s1 = sum_c gamma_c sum dy, s2 = sum_c gamma_c sum dy xhat in index order, dx = rstd (dy gamma - (s1 + xhat
 *             s2) / n); the workgroups behind them add the partials over chunks, then images, into dgamma, dbeta [L][C] fp32.
 * No atomics and no hand-over inside a launch: the same call gives the same bits.
 *
 * Masks.  mask: the image-level padding mask [B, H, W], bool bytes or fp32 (mask_is_f32), non-zero = padded.  level_masks[l]: bool
 * [B, h_l, w_l] by torch's nearest rule, src = min(floor(dst * (float(in) / float(out))), in - 1).  cum: int32, 2 * B * S entries
 * (S the pixels of all levels): level l's [B, h_l, w_l] inclusive count of valid pixels down the columns at B * (pixels of the levels
 * before l), and along the rows B * S entries further on.  One launch.
 *
 * Position encoding.  out[l]: [B, 2 F, h_l, w_l] fp32 or bf16, channels [0, F) from the column counts and [F, 2 F) from the row
 * counts, 2 k the sine and 2 k + 1 the cosine of a = e / dim_t[k], e = float(count) + offset and, with normalize, e = e /
 * (float(last count of the column / row) + eps) * scale, each step one fp32 operation.  dim_t: F / 2 floats on the device, F even.
 * One launch. */
long long rdetr_neck_workspace_bytes(const int *level_hw, int L, int B, int C, int G);
int rdetr_group_norm_levels_f32(const void *const *x, const void *const *gamma, const void *const *beta, const int *level_hw, int L, int B,
                                int C, int G, float eps, void *ws, long long ws_bytes, void *const *y, float *mean, float *rstd, void *stream);
int rdetr_group_norm_levels_bf16(const void *const *x, const void *const *gamma, const void *const *beta, int params_bf16, const int *level_hw,
                                 int L, int B, int C, int G, float eps, void *ws, long long ws_bytes, void *const *y, float *mean, float *rstd,
                                 void *stream);
int rdetr_group_norm_levels_backward_f32(const void *const *dy, const void *const *x, const void *const *gamma, const float *mean,
                                         const float *rstd, const int *level_hw, int L, int B, int C, int G, void *ws, long long ws_bytes,
                                         void *const *dx, float *dgamma, float *dbeta, void *stream);
int rdetr_group_norm_levels_backward_bf16(const void *const *dy, const void *const *x, const void *const *gamma, int params_bf16,
                                          const float *mean, const float *rstd, const int *level_hw, int L, int B, int C, int G, void *ws,
                                          long long ws_bytes, void *const *dx, float *dgamma, float *dbeta, void *stream);
int rdetr_pyramid_masks(const void *mask, int mask_is_f32, int B, int H, int W, const int *level_hw, int L, void *const *level_masks,
                        int *cum, void *stream);
int rdetr_pyramid_sine_pos_f32(const int *cum, const int *level_hw, int L, int B, int F, const float *dim_t, int normalize, float scale,
                               float eps, float offset, void *const *out, void *stream);
int rdetr_pyramid_sine_pos_bf16(const int *cum, const int *level_hw, int L, int B, int F, const float *dim_t, int normalize, float scale,
                                float eps, float offset, void *const *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The image front end (csrc/images.hip; models/detectors/base_detector.py: EvalResize -> ConvertImageDtype -> Normalize ->
 * image_list_from_tensors -> construct_mask): a list of device images -> the padded batch and its padding mask, one launch.
 *
 * images: a HOST array of B <= RDETR_IMAGE_MAX_IMAGES descriptors, copied into the kernel's argument block.  src: a DEVICE image
 * [3, h, w], uint8 (src_is_u8 = 1) or fp32, unit stride along a row, row_stride and channel_stride in elements (>= 0); (oh, ow): the
 * size it is resized to, (oh, ow) == (h, w) for none.  out: [B, 3, Hp, Wp] fp32 or bf16 (out_bf16), contiguous, or with
 * channels_last = 1 the same tensor stored [B, Hp, Wp, 3]; 16-byte aligned, Wp % 8 == 0.  mask: [B, Hp, Wp] bool bytes, 1 = padded.
 * mean, std: HOST float[3], read when normalize = 1.
 *
 * Per output (b, c, y, x): y >= oh_b or x >= ow_b gives +0 and mask 1.  Otherwise mask 0 and v = sum_j sum_i Wy[y, j] Wx[x, i]
 * src[c, j, i] with torch's antialiased bilinear taps for n_in -> n_out per axis: scale = n_in / n_out, support = max(scale, 1),
 * center = scale (o + 0.5), lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), n_in), w_j = max(0, 1 -
 * |(j - center + 0.5) / support|) over [lo, hi) divided by their sum; the taps in fp64, the two passes (rows first, as torch's CPU
 * kernel) in fp32.  uint8: q = rint(v) (half to even), out = (float(q) / 255 - mean_c) / std_c, three IEEE fp32 operations.  fp32:
 * out = (v - mean_c) / std_c, or v with normalize = 0 (fp32 sources only).  bf16 output rounds the fp32 value to nearest even.
 *
 * RDETR_ERR_INVALID_ARG: a NULL pointer, a size <= 0, a negative stride, B < 0, a flag outside {0, 1}, (oh, ow) beyond (Hp, Wp),
 * a std of 0.  RDETR_ERR_UNSUPPORTED: B > RDETR_IMAGE_MAX_IMAGES, h > RDETR_IMAGE_MAX_DOWNSCALE * oh (or w, ow: the LDS rows of one
 * tile), Wp % 8 != 0, a misaligned out / mask / fp32 src, a uint8 source with normalize = 0.  B == 0 launches nothing. */
#define RDETR_IMAGE_MAX_IMAGES 16
#define RDETR_IMAGE_MAX_DOWNSCALE 8
typedef struct rdetr_image_desc {
    const void *src;
    long long row_stride, channel_stride;
    int h, w, oh, ow;
} rdetr_image_desc;
int rdetr_image_batch(const rdetr_image_desc *images, int B, int src_is_u8, int Hp, int Wp, const float *mean, const float *std,
                      int normalize, int out_bf16, int channels_last, void *out, void *mask, void *stream);

/* The training augmentation's geometry (transforms/presets.py: RandomHorizontalFlip -> RandomShortestSize [-> RandomSizeCrop ->
 * RandomShortestSize]) with the same taps, rounding and tail, one launch:  per image  window(resize(flip(src), (rh, rw))).
 *
 * flip = 1: column x of the image that is resized is source column w - 1 - x; the taps are summed in the flipped image's column
 * order, so the fp32 sum is the one torch forms on image.flip(-1).  (rh, rw): the size of the virtual resized image, == (h, w) for
 * none.  (top, left, oh, ow): the window of it that is produced, 0 <= top, top + oh <= rh, 0 <= left, left + ow <= rw; only tiles
 * of the window are computed and only the source rows its rows touch are filtered.
 *
 * out_mode RDETR_IMAGE_OUT_BATCH: the tail of rdetr_image_batch -- window pixel (y, x) of image b at out[b, :, y, x], everything
 *   at or behind (oh, ow) +0 with mask 1; Hp, Wp, mean, std, normalize, out_bf16, channels_last, out and mask as there.
 * out_mode RDETR_IMAGE_OUT_U8: uint8 sources only; q = rint(v) is stored as uint8, planar, at dst[c * dst_channel_stride + y *
 *   dst_row_stride + x]: the intermediate of the crop branch.  No padding and no mask: Hp, Wp, mean, std, normalize, out_bf16,
 *   channels_last, out and mask are not read.  dst is 16-byte aligned, both strides multiples of 16, dst_row_stride >= ow rounded up
 *   to 16: whole 16-byte pieces are stored, so columns ow .. roundup(ow, 16) - 1 of every row are written too (as 0).
 *
 * Status codes as rdetr_image_batch, and: RDETR_ERR_INVALID_ARG for a window outside the virtual image, a flip or out_mode outside
 * {0, 1}; RDETR_ERR_UNSUPPORTED for h > RDETR_IMAGE_MAX_DOWNSCALE * rh (or w, rw), fp32 sources in U8 mode, a dst off the rules above. */
#define RDETR_IMAGE_OUT_BATCH 0
#define RDETR_IMAGE_OUT_U8 1
typedef struct rdetr_image_window_desc {
    const void *src;
    long long row_stride, channel_stride;
    int h, w, flip, rh, rw, top, left, oh, ow;
    void *dst;
    long long dst_row_stride, dst_channel_stride;
} rdetr_image_window_desc;
int rdetr_augment_image_batch(const rdetr_image_window_desc *images, int B, int src_is_u8, int out_mode, int Hp, int Wp, const float *mean,
                              const float *std, int normalize, int out_bf16, int channels_last, void *out, void *mask, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The ResNet backbone's epilogues (csrc/backbone.hip; models/bricks/misc.py: FrozenBatchNorm2d, models/backbones/resnet.py): what
 * follows each library convolution, in one read and one write.
 *
 * Tensors are [B, C, H, W], dense NCHW, or with channels_last = 1 the same tensor stored [B, H, W, C]; fp32 or bf16 by the entry's
 * suffix, bases 16-byte aligned.  scale, shift: fp32 [C].  An NCHW plane whose H * W is no multiple of the vector width starts off
 * the 16-byte grid; the kernels take its head and tail as scalars.  In channels-last C may be any size.
 *
 * rdetr_frozen_bn_act_*:  out = act(x * scale[c] + shift[c] (+ residual)).  fp32: one rounded multiply, one rounded add, one
 *   rounded add of the residual, never contracted, so the result is torch's relu(x * s + b + r) bit for bit; bf16 computes in fp32 and
 *   rounds once.  relu: 0 | 1, a NaN stays a NaN.  residual: NULL for none.  out == x (in place) is allowed; out overlapping x in any
 *   other way, or overlapping residual, is RDETR_ERR_INVALID_ARG.
 * rdetr_frozen_bn_act_backward_*:  from dy, the saved output y and scale: dx = (dy * [y > 0]) * scale[c] and, with dres != NULL,
 *   dres = dy * [y > 0], in the same launch; relu = 0 makes the mask all ones (y may then be NULL).  fp32: autograd's result for
 *   the operator sequence above, bit for bit.  dx == dy is allowed; dres overlapping dx, or either overlapping y, is
 *   RDETR_ERR_INVALID_ARG.
 * rdetr_stem_pool_*:  out = maxpool 3x3 / stride 2 / padding 1 of relu(x * scale[c] + shift[c]); x [B, C, H, W], out [B, C,
 *   (H - 1) / 2 + 1, (W - 1) / 2 + 1], the same arithmetic rule.  Padding never wins; a window that holds a NaN gives NaN.  out must
 *   not overlap x.
 *
 * RDETR_ERR_INVALID_ARG: a NULL required pointer, B, C, H or W <= 0, a flag outside {0, 1}, a forbidden overlap.
 * RDETR_ERR_UNSUPPORTED: B * C * H * W >= 2^31, a base off the 16-byte grid.  All checks precede any HIP call. */
int rdetr_frozen_bn_act_f32(const void *x, const float *scale, const float *shift, const void *residual, int B, int C, int H, int W,
                            int channels_last, int relu, void *out, void *stream);
int rdetr_frozen_bn_act_bf16(const void *x, const float *scale, const float *shift, const void *residual, int B, int C, int H, int W,
                             int channels_last, int relu, void *out, void *stream);
int rdetr_frozen_bn_act_backward_f32(const void *dy, const void *y, const float *scale, int B, int C, int H, int W, int channels_last,
                                     int relu, void *dx, void *dres, void *stream);
int rdetr_frozen_bn_act_backward_bf16(const void *dy, const void *y, const float *scale, int B, int C, int H, int W, int channels_last,
                                      int relu, void *dx, void *dres, void *stream);
int rdetr_stem_pool_f32(const void *x, const float *scale, const float *shift, int B, int C, int H, int W, int channels_last, void *out,
                        void *stream);
int rdetr_stem_pool_bf16(const void *x, const float *scale, const float *shift, int B, int C, int H, int W, int channels_last, void *out,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RELATION_DETR_AMD_H */
