/*
 * artn.h -- C ABI of libartn_hip.so, the MI355X (gfx950) numerical contraction engine
 * behind artensor's executor entry points.
 *
 * The reference (Fanerst/artensor) has no FFI: its executor is Python calling
 * torch.einsum.  Each entry point below replaces one such call site; the reference
 * file:line it stands in for is cited on the declaration.  All pointers are raw device
 * pointers (hipMalloc'ed / torch `Tensor.data_ptr()`), sizes are in elements unless a
 * name says bytes, `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Every function returns 0 on success and a negative ARTN_E_* code on failure;
 * artn_last_error() then holds a message.  No function allocates or frees device
 * memory, synchronises the device or calls a CPU fallback: work is enqueued on `stream`
 * and the caller owns every buffer (graph-capture safe).
 */
#ifndef ARTN_H
#define ARTN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARTN_ABI_VERSION 9
#define ARTN_MAX_LABELS 96

/* error codes */
#define ARTN_OK 0
#define ARTN_E_INVALID (-1)     /* malformed descriptor / argument            */
#define ARTN_E_UNSUPPORTED (-2) /* valid but not implemented (e.g. dtype)     */
#define ARTN_E_LAUNCH (-3)      /* HIP launch / runtime error                 */
#define ARTN_E_NODEVICE (-4)    /* no gfx950 device visible                   */

/* dtypes (arithmetic type of the contraction) */
#define ARTN_C64 0  /* interleaved (re,im) float32 pairs  -- torch.complex64  */
#define ARTN_C128 1 /* interleaved (re,im) float64 pairs  -- torch.complex128 */
#define ARTN_C64_BF16 2 /* complex64 in memory; operands of the big steps rounded to bfloat16 for the
                           matrix cores, fp32 accumulation: the reduced-precision sampling mode (the
                           reference has no such path; its results define no parity here) */

/*
 * One pairwise contraction step  C[out labels] = sum_{labels not in C} A[...] * B[...]
 * i.e. one `torch.einsum(eq, tensors[i], tensors[j])` of
 *   artensor/contraction.py:70 (dense executor) and
 *   artensor/contraction.py:147,156,163,169,179,181,190 (sparse executor).
 * The einsum string is replaced by label lists so unions of more than 50 labels
 * (the reference's alphabet, contraction.py:9-10) are representable.
 *
 * Label l (0 <= l < n_labels) has `extent[l]` and an element stride in each operand,
 * or -1 where the operand does not carry the label.  A label carried by A and B but
 * not C is contracted; by A (or B) and C only is free; by all three is a batch label
 * (the sparse path's shared label -3, contraction.py:306-308); by A or B alone is
 * summed out (einsum semantics).  C must be dense row-major over its labels in the
 * order implied by stride_c; A and B may be arbitrary non-overlapping strided views.
 */
typedef struct ArtnStepDesc {
  int32_t dtype;
  int32_t n_labels;
  int64_t extent[ARTN_MAX_LABELS];
  int64_t stride_a[ARTN_MAX_LABELS];
  int64_t stride_b[ARTN_MAX_LABELS];
  int64_t stride_c[ARTN_MAX_LABELS];
} ArtnStepDesc;

/* What the planner decided for a step (filled on the host, no GPU needed). */
#define ARTN_KERNEL_GENERIC 0 /* one thread per output element, strided loops       */
#define ARTN_KERNEL_BITS_MFMA 1 /* LDS-tiled bit-permuted complex GEMM on fp32 MFMA */
#define ARTN_KERNEL_GEMM_MFMA 2 /* two-operand LDS GEMM on fp32 MFMA, contracted bits looped in-kernel */
#define ARTN_KERNEL_PGEMM 4     /* big x big steps (complex64: 2^11+ contracted values, 160+ FLOP per byte; bf16 operands: 2^9+): both operands packed in
                                 * tile order into a workspace, then an LDS-DMA GEMM.  ARTN_C64: fp32 images, 3M arithmetic
                                 * (artn_k_pgemm3m; workspace 8 B x (2^(m+k) + 2^(n+k))); ARTN_C64_BF16: bfloat16 images
                                 * (artn_k_pgemm; half of that) */
#define ARTN_KERNEL_XGEMM 5     /* extent-based two-operand GEMM on fp32 MFMA (3M): any extents -- bond dimensions 3, 5, 6 ... --
                                 * flattened mixed-radix indices, offset tables in LDS (artn_k_xgemm) */
typedef struct ArtnStepInfo {
  int32_t kernel;       /* ARTN_KERNEL_*                                        */
  int32_t k_bits;       /* contracted bits handled inside a tile                */
  int32_t m_tile_bits;  /* free A bits inside a tile                            */
  int32_t n_tile_bits;  /* free B bits inside a tile                            */
  int32_t tile_in_bits; /* log2 elements of A staged in LDS per tile            */
  int32_t tile_out_bits;/* log2 elements of C staged in LDS per tile            */
  int32_t run_in_bits;  /* log2 contiguous elements per global read run         */
  int32_t run_out_bits; /* log2 contiguous elements per global write run        */
  int32_t lds_bytes;
  int32_t grid;
  int64_t n_tiles;
  int64_t a_rereads;    /* how many tiles read each A element (outer-N split)   */
  double flops;         /* 8 * prod(all extents) real FLOP (c64 MAC = 8)        */
  double bytes;         /* compulsory: 8|16 * (numel A + numel B + numel C)     */
  int32_t k2_bits;      /* fused pair: contracted bits of the second step (else 0) */
  int32_t n2_tile_bits; /* fused pair: free B2 bits inside a tile                  */
  int32_t tile_mid_bits;/* log2 elements of the tile between the two stages        */
  int32_t arith;        /* 0 fp32 MFMA 4M, 1 fp32 MFMA with 3M stages, 2 bf16 operands, 3 f64 MFMA, -1 no MFMA */
  double mfma_flops;    /* real FLOP the matrix pipe executes: `flops` with 6 instead of 8 per complex
                           multiply-add in every 3M stage (0 for the strided kernel)     */
  int64_t workspace_bytes; /* scratch the step wants from artn_contract_ws (0: none; artn_contract never needs any) */
  int32_t k3_bits;      /* fused triple (development builds only: artn_contract3): contracted bits of the third step (else 0) */
  int32_t stage1_reruns;/* fused pair: how often the first stage of a tile runs (the product of the outer result labels that only the
                           second step brings: each value repeats stage 1 and its reads); 0 or 1 otherwise */
} ArtnStepInfo;

int artn_abi_version(void);
const char *artn_last_error(void);

/* Number of visible gfx950 devices (0 on a CPU-only box; never fails). */
int artn_device_count(void);

/* Host-only: run the planner for `d` and report its decision. */
int artn_contract_query(const ArtnStepDesc *d, ArtnStepInfo *info);
/* Why the step of the last artn_contract_query on this thread was given to the strided
 * kernel ("" if it was not). */
const char *artn_last_plan_note(void);

/* Enqueue one pairwise contraction (replaces torch.einsum at contraction.py:70 etc.). */
int artn_contract(const ArtnStepDesc *d, const void *A, const void *B, void *C, void *stream);

/* The same with `ws_bytes` bytes of device scratch (16-byte aligned; ArtnStepInfo::workspace_bytes of
 * artn_contract_query says how much the step can use): steps that pack their operands first (ARTN_KERNEL_PGEMM:
 * the big x big contractions of plain complex64 AND of the reduced-precision mode) run that way when the scratch
 * is big enough, and exactly like artn_contract otherwise.  The library never allocates. */
int artn_contract_ws(const ArtnStepDesc *d, const void *A, const void *B, void *C, void *ws, int64_t ws_bytes,
                     void *stream);

/*
 * artn_contract with a fused row gather: along `label` (an output label; the batch label of the
 * sparse executor) operand A is read at row rows_a[r] and operand B at row rows_b[r] for output row
 * r (device pointers to int64; NULL = r itself); extent[label] is the number of output rows and
 * stride_a/b[label] the row strides of the SOURCE tensors, which have src_rows_a/b rows.
 * Replaces `tensors[i][batch_i[k]]`, `tensors[j][batch_j[k]]` followed by the batched einsum of
 * artensor/contraction.py:149-156 and :177-179 without materialising the gathered operands.
 * Out-of-range indices read row 0 and set *err_flag (if non-NULL).  Returns ARTN_E_UNSUPPORTED
 * when the step does not fit a tiled kernel; callers then gather with artn_gather_rows.
 * (complex64 only.  Steps with 7+ contracted bits run on the two-operand GEMM kernel, the others on the
 * state-streaming kernel; both resolve the rows inside their tile-offset computation.)
 */
int artn_contract_gather(const ArtnStepDesc *d, const void *A, const void *B, void *C, int label,
                         const int64_t *rows_a, int64_t src_rows_a, const int64_t *rows_b, int64_t src_rows_b,
                         int32_t *err_flag, void *stream);

/*
 * Two consecutive steps on the same big operand in ONE pass over HBM:
 *     C1 = contract(d1; A, B1);  C = contract(d2; C1, B2)
 * i.e. two successive iterations of the loop at artensor/contraction.py:66-70 whose first
 * operand is the same `tensors[i]` (the growing state tensor is always operand 0,
 * contraction.py:41-46).  d2's stride_a must describe d1's dense result C1, which is
 * never written to memory: the second contraction runs on the tile while it is in LDS.
 * artn_contract2_query / artn_contract2 return ARTN_E_UNSUPPORTED when the pair does not
 * fit one LDS tile (artn_last_error() says why); callers then issue two artn_contract.
 * complex64 (fp32 MFMA; bf16 operands under ARTN_C64_BF16) and complex128 (f64 MFMA, tiles of half as
 * many elements); both descriptors must name the same dtype.
 */
int artn_contract2_query(const ArtnStepDesc *d1, const ArtnStepDesc *d2, ArtnStepInfo *info);
int artn_contract2(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const void *A, const void *B1,
                   const void *B2, void *C, void *stream);

/*
 * C += contract(...) in the store phase of the last launch of a slice: the reference's slice loop ends every slice with
 * `collect_tensor += tensor_contraction(...)` (artensor/simulation.py:114); with a dense output the separate add reads the
 * slice's result and the accumulator and writes the accumulator again (3 x the output), the fused form reads and writes the
 * accumulator once and the result never exists in memory.  Every element of C belongs to exactly one lane of one tile
 * of the launch (plain loads and stores; C must not alias A), so C's value does not depend on scheduling.  complex64 state-streaming
 * plans only (artn_k_bits, single steps and fused pairs, register-prefetch tile loop); ARTN_E_UNSUPPORTED (-2) otherwise:
 * the caller then contracts into a temporary and calls artn_axpy_c64.
 */
int artn_contract_acc(const ArtnStepDesc *d, const void *A, const void *B, void *C, void *stream);
int artn_contract2_acc(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const void *A, const void *B1,
                       const void *B2, void *C, void *stream);

/* (ABI 7: artn_contract3 / artn_contract3_query -- three steps in one pass, round 4 -- left the product library: built,
 * parity-green, and shorter on no committed workload.  Development builds (make dev, -DARTN_DEV_BITS3)
 * still export them with the ABI-6 signatures, declared here for those builds only.) */
#ifdef ARTN_DEV_BITS3
int artn_contract3_query(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const ArtnStepDesc *d3, ArtnStepInfo *info);
int artn_contract3(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const ArtnStepDesc *d3, const void *A, const void *B1,
                   const void *B2, const void *B3, void *C, void *stream);
#endif

/*
 * dst[r, :] = src[idx[r], :] for r < nrows, rows of `row_bytes` bytes (multiple of 8).
 * Replaces the batch-row gathers `tensors[i][batch_i[k]]` of
 * artensor/contraction.py:149-150,158-159,165-166,171-172,177-178,187.
 * `idx` is a DEVICE pointer to int64 row indices; src_rows bounds-checks them
 * (out-of-range rows are written as zeros and flagged in *err_flag if non-NULL).
 */
int artn_gather_rows(const void *src, const int64_t *idx, void *dst, int64_t nrows,
                     int64_t row_bytes, int64_t src_rows, int32_t *err_flag, void *stream);

/*
 * Small-step programs.  A circuit scheme is a few big steps plus hundreds of tiny ones (rank <= 16
 * operands) that are pure launch latency when issued one by one -- on the CPU the reference spends
 * 35-65 us per torch.einsum call on them (artensor/contraction.py:66-70; its whole n12 run is that).
 * Here the tiny steps of a scheme are compiled ONCE into a device-resident image and executed by ONE launch:
 * workgroup g runs the steps of group g (steps of different groups must be independent).  Inside a group the
 * steps are sorted into the levels of their dependency tree; the steps of a level run side by side on the 16 waves
 * of the workgroup, one barrier per level; intermediates stay in an LDS arena laid out at build time, only the
 * results flagged in `keep` (read after the program) and what the arena cannot hold go through the caller-provided
 * workspace.  n12 (68 steps, 19 levels) is one launch of a few tens of microseconds.
 *
 *   artn_program_image_bytes(...)  host only: size of the image for these steps (upper bound)
 *   artn_program_build(...)        host only: fills `host_image` from the step descriptors; operand k of step s is
 *                                  the result written at workspace byte offset loc >= 0 by an earlier step, or
 *                                  external pointer number -(loc + 1) when loc < 0; keep[s] != 0 (or keep == NULL):
 *                                  the result of step s must be in the workspace after the launch.  Steps must
 *                                  have dense operands and ONE element type (all complex64 -- small matrix-core
 *                                  steps included -- or all complex128: 16-byte elements, vector ALU only);
 *                                  returns ARTN_E_UNSUPPORTED when a step does not fit a record (the caller then
 *                                  issues artn_contract per step).
 *   artn_program_run(...)          enqueue: `dev_image` is the device copy of the image, `ext` a HOST array of
 *                                  n_ext (<= 256) device pointers, `dtype` the element type the image was built for
 *                                  (ARTN_C64 / ARTN_C64_BF16 / ARTN_C128).
 */
#define ARTN_PROGRAM_MAX_EXT 256
int64_t artn_program_record_bytes(void);
int64_t artn_program_image_bytes(int32_t n_steps, const ArtnStepDesc *const *descs, int32_t n_groups);
int artn_program_build(int32_t n_steps, const ArtnStepDesc *const *descs, const int64_t *loc_a, const int64_t *loc_b,
                       const int64_t *loc_c, const uint8_t *keep, int32_t n_groups, const int32_t *group_start,
                       void *host_image, int64_t image_bytes);
int artn_program_run(const void *dev_image, int32_t n_groups, const void *const *ext, int32_t n_ext, void *workspace,
                     int32_t dtype, void *stream);

/* acc[i] += x[i], i < n complex64 elements: the slice accumulation
 * `collect_tensor += ...` of artensor/simulation.py:114 and :210. */
int artn_axpy_c64(void *acc, const void *x, int64_t n, void *stream);
/* the same for complex128 (the reference's slice loop takes any dtype, artensor/simulation.py:90, :101) */
int artn_axpy_c128(void *acc, const void *x, int64_t n, void *stream);

/* out[g][c] = sum_r in[g][r][c] for complex64 arrays in[n_groups][n_rows][n_cols] (8-byte aligned; 16-byte
 * lanes when n_cols is even and the buffers are 16-byte aligned): sums out the leading label(s) of a dense tensor.  Closes a contraction whose
 * contracted labels exceed one LDS tile: `torch.einsum` at artensor/contraction.py:70 contracts any
 * number of labels in one call; here the slowest ones become a batch label of artn_contract and are
 * summed afterwards.  Applied twice (n_rows = R * n_rows') it is a two-pass tree sum. */
int artn_sum_axis_c64(const void *in, void *out, int64_t n_groups, int64_t n_rows, int64_t n_cols, void *stream);
/* the same for complex128 arrays (any n_cols; 16-byte aligned) */
int artn_sum_axis_c128(const void *in, void *out, int64_t n_groups, int64_t n_rows, int64_t n_cols, void *stream);

/* out[0] = max_i |x[i]| over n complex64 elements (float32, device pointer), then
 * x[i] /= out[0]: the running renormalisation of artensor/contraction.py:197-200
 * (`norm_factor = tensors[i].abs().max(); tensors[i] /= norm_factor`). */
int artn_absmax_normalize_c64(void *x, int64_t n, float *out_absmax, void *stream);
/* the same for complex128 elements (out_absmax: float64 device pointer): the reference renormalises in whatever
 * dtype `TensorNetworkSimulation.contraction(dtype=...)` selected (artensor/simulation.py:90, contraction.py:197-200) */
int artn_absmax_normalize_c128(void *x, int64_t n, double *out_absmax, void *stream);

/* Measurement aid (bench.py): the rate the matrix pipes of this device sustain on back-to-back MFMAs with operands
 * in registers, in TFLOP/s -- kind 0: v_mfma_f32_32x32x2_f32, 1: v_mfma_f32_32x32x16_bf16, 2: v_mfma_f64_16x16x4_f64
 * (the arithmetic of complex128 steps; the roofline of a complex128 run is priced against this measured figure).
 * `scratch4`: 4 bytes of device memory.  Synchronous (runs on the null stream and waits). */
int artn_probe_mfma_rate(int kind, void *scratch4, double *tflops);

/*
 * Born statistics of an amplitude array (ABI 8): what a consumer of `TensorNetworkSimulation.contraction` does next.
 * The reference has no call for any of it; its notebook forms a fidelity with torch expressions
 * (examples/sycamore.ipynb, cell 7: `(full.conj() @ approx.reshape(-1)).abs() / (full.abs().square().sum().sqrt() * ...)`,
 * six passes over memory and several temporaries of the size of the state), and the result it would feed them is the
 * permuted view of artensor/simulation.py:115-116, which the entry points below consume in place: they work on the
 * memory layout, `a` being the n contiguous elements the view covers.
 * All of them accumulate in float64, form each complex64 term in float64 (convert, then square), use no floating-point
 * atomics and give bit-identical results from run to run.  Arrays must be 16-byte aligned; n <= 2^40.
 */
typedef struct ArtnBornPlan {
  int32_t block_bits;      /* blocks of 2^block_bits consecutive elements (10..14)                       */
  int32_t overlap_grid;    /* workgroups of artn_born_overlap: its workspace holds 4 doubles for each    */
  int64_t n_blocks;        /* ceil(n / 2^block_bits): length of block_sum[] and prefix[]                 */
  int64_t workspace_bytes; /* scratch artn_born_overlap wants                                            */
} ArtnBornPlan;
/* Host-only: the block size, block count and workspace for n elements of `dtype` (ARTN_C64 / ARTN_C128). */
int artn_born_plan(int64_t n, int32_t dtype, ArtnBornPlan *plan);
/* out4 (device) = { Re<a|b>, Im<a|b>, sum|a|^2, sum|b|^2 } with <a|b> = sum conj(a[i]) b[i], in ONE pass over both arrays
 * (notebook cell 7).  b == NULL or b == a: one array is read, out4 = { |a|^2, 0, |a|^2, |a|^2 }.  Per-workgroup partials go
 * to `ws`, a second one-workgroup launch adds them in a fixed order. */
int artn_born_overlap(const void *a, const void *b, int64_t n, int32_t dtype, void *ws, int64_t ws_bytes, double *out4,
                      void *stream);
/* block_sum[j] = sum of |a[i]|^2 over block j (n_blocks doubles), and, if `prefix` is not NULL, their inclusive prefix sums:
 * non-decreasing, and prefix[j] > prefix[j-1] only where block_sum[j] > 0. */
int artn_born_block_sums(const void *a, int64_t n, int32_t dtype, double *block_sum, double *prefix, void *stream);
/* Resolves m targets t (device, float64, ASCENDING, in [0, prefix[n_blocks-1]]) against the cumulative distribution of |a|^2:
 * the block is found by bisection of `prefix`, the block is re-read once for all the targets that fall into it with a
 * float64 running sum in a fixed order, and out_index[s] is the smallest flat index whose running sum exceeds t[s].  An
 * element with |a|^2 == 0 is never returned; a target at or beyond the last prefix yields the last non-zero element.
 * out_prob[s] = |a[out_index[s]]|^2.  (out_index[s] = -1 only if every element is zero.) */
int artn_born_pick(const void *a, int64_t n, int32_t dtype, const double *prefix, const double *targets, int64_t m,
                   int64_t *out_index, double *out_prob, void *stream);

/*
 * out[kept multi-index] = sum over the dropped dimensions of |a|^2 for a DENSE tensor (the strides of its dimensions of
 * extent > 1 are a permutation of a contiguous layout: exactly the permuted result of artensor/simulation.py:115-116).
 * `out` is float64, row-major over the kept dimensions in the order they are listed.
 *   ARTN_MARGINAL_STREAM   power-of-two extents, at least 2^12 elements, at most 2^24 KEPT elements: workgroups stream chunks of
 *                          2^12 contiguous elements, kept bits inside a chunk index float64 bins in LDS, kept bits above it
 *                          select a partial row of the workspace; a second launch adds the rows in a fixed order.
 *                          (Power-of-two extents keeping more than 2^24 elements: ARTN_E_UNSUPPORTED.)
 *   ARTN_MARGINAL_GENERIC  any other extents (bond dimensions 3, 6 ...): one thread per output element; correct, not fast.
 */
#define ARTN_MARGINAL_GENERIC 0
#define ARTN_MARGINAL_STREAM 1
typedef struct ArtnMarginalDesc {
  int32_t dtype;
  int32_t n_dims; /* <= ARTN_MAX_LABELS */
  int64_t extent[ARTN_MAX_LABELS];
  int64_t stride[ARTN_MAX_LABELS]; /* in elements */
  int32_t keep[ARTN_MAX_LABELS];   /* non-zero: the dimension stays */
} ArtnMarginalDesc;
typedef struct ArtnMarginalInfo {
  int32_t kernel;     /* ARTN_MARGINAL_*                                   */
  int32_t chunk_bits; /* streaming: log2 elements per chunk                */
  int32_t bin_bits;   /* streaming: log2 float64 bins in LDS               */
  int32_t grid;       /* workgroups of the first launch                    */
  int64_t workspace_bytes;
  int64_t out_elems;
} ArtnMarginalInfo;
/* Host-only: validates the layout (ARTN_E_INVALID when it is not dense), picks the kernel, sizes workspace and output. */
int artn_marginal_query(const ArtnMarginalDesc *d, ArtnMarginalInfo *info);
int artn_marginal(const ArtnMarginalDesc *d, const void *a, double *out, void *ws, int64_t ws_bytes, void *stream);

/*
 * Reduced density matrix (ABI 9): out[i][j] = sum_r a[i, r] conj(a[j, r]) for a DENSE tensor, i and j running over the kept
 * dimensions (in the order they are listed, the first one the most significant digit), r over all the others.  The descriptor
 * and its checks are those of artn_marginal; the diagonal of the result is what artn_marginal returns.  `out` is D x D
 * complex128 as interleaved float64 (16-byte aligned), D the product of the kept extents, at most 1024 (more: ARTN_E_UNSUPPORTED).
 * Unnormalised.  Every product is formed in float64 (complex64 values are converted first), sums are float64 in an order that
 * depends on the descriptor alone, without floating-point atomics: bit-identical from run to run.  The result is exactly
 * Hermitian (the lower triangle is computed, the upper one is its conjugate) and the diagonal's imaginary part is exactly 0.
 *   ARTN_RDM_STREAM   power-of-two extents, at least 2^12 elements, D >= 2 and, where D > 64, at least 16 dropped states:
 *                     lower-triangle tiles of 64 x 64 (D < 64: one tile of max(D, 16) rows) x `splits` ranges of the dropped
 *                     index on v_mfma_f64_16x16x4_f64; one partial tile per workgroup in the workspace, a second launch adds
 *                     them in ascending order.  workspace_bytes = tiles * splits * rows^2 * 16.
 *   ARTN_RDM_GENERIC  anything else: one workgroup per element of the lower triangle, a fixed tree; correct, not fast.
 */
#define ARTN_RDM_GENERIC 0
#define ARTN_RDM_STREAM 1
typedef struct ArtnRdmInfo {
  int32_t kernel;     /* ARTN_RDM_STREAM / ARTN_RDM_GENERIC                             */
  int32_t panel_bits; /* streaming: log2 columns (dropped states) of a panel in LDS     */
  int32_t tiles;      /* streaming: lower-triangle tiles                                */
  int32_t splits;     /* streaming: ranges of the dropped index (partials per element)  */
  int64_t dim;        /* D                                                              */
  int64_t workspace_bytes;
  double flops;       /* real FLOP executed on the matrix cores (0 for the generic form) */
} ArtnRdmInfo;
/* Host-only: validates the layout (ARTN_E_INVALID when it is not dense), picks the form, sizes the workspace. */
int artn_rdm_query(const ArtnMarginalDesc *d, ArtnRdmInfo *info);
/* Host-only: offset[i] (D entries) = the memory offset, in elements, of the kept digits of row i with every dropped index 0,
 * read from the same plan tables the kernels use (row i of `out` sums a[offset[i] + r] over the dropped offsets r). */
int artn_rdm_row_offsets(const ArtnMarginalDesc *d, int64_t *offset);
int artn_rdm(const ArtnMarginalDesc *d, const void *a, double *out /* [D][D][2] */, void *ws, int64_t ws_bytes, void *stream);

/*
 * Expectation values of Pauli strings (additive to ABI 9: look the symbols up before calling).  For a DENSE tensor of
 * power-of-two extents (descriptor and density checks of artn_marginal; dimensions in the caller's order, keep[] ignored), a
 * string gives every dimension one of I, X, Y, Z: `ops` is uint8 [n_terms][n_dims], 0..3 = I, X, Y, Z; X, Y and Z only on
 * dimensions of extent 2.  A dimension of extent 2 and stride 2^b is bit b of the flat memory index; with xmask the bits under
 * X or Y, zmask those under Z or Y and n_y the number of Y,
 *     <psi|P|psi> = sum_i conj(a[i ^ xmask]) * i^n_y * (-1)^popcount(i & zmask) * a[i]        (real)
 * one streaming pass over the amplitudes for up to terms_per_launch strings of equal xmask (a GROUP; groups are numbered in the
 * order they first appear).  A call takes sum over groups of ceil(count / terms_per_launch) launches, each reading every
 * amplitude once.  Terms are formed in float64 (complex64 values are converted first), sums are float64 in an order that depends
 * on the element count and the masks alone, without floating-point atomics: bit-identical from run to run.
 * ARTN_E_INVALID: a layout that is not dense, an operator code above 3, X/Y/Z on an extent other than 2, n_terms < 1, a workspace
 * that is too small.  ARTN_E_UNSUPPORTED: an extent that is no power of two, more than 96 dimensions, more than 2^40 elements.
 */
typedef struct ArtnPauliInfo {
  int32_t n_groups;         /* distinct xmasks                                        */
  int32_t n_launches;       /* passes over the amplitudes                             */
  int32_t terms_per_launch; /* strings one pass serves                                */
  int32_t reserved;
  int64_t workspace_bytes;
  int64_t bytes_read;       /* n_launches * bytes of the state                        */
} ArtnPauliInfo;
/* Host-only: validates, translates every term to memory-bit masks, groups by xmask, sizes the workspace.
 * xmask, zmask, n_y, group: n_terms entries each, any of them may be NULL. */
int artn_pauli_query(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, ArtnPauliInfo *info, uint64_t *xmask,
                     uint64_t *zmask, int32_t *n_y, int32_t *group);
/* out (device, float64 [n_terms + 1]): the raw sums in the caller's term order, out[n_terms] = sum |a|^2 (from the first pass).
 * `a` must be 16-byte aligned.  No allocation, copy or synchronisation: the launches are enqueued on `stream`. */
int artn_pauli_expect(const ArtnMarginalDesc *d, const void *a, const uint8_t *ops, int64_t n_terms, double *out, void *ws,
                      int64_t ws_bytes, void *stream);

/*
 * Applying Pauli strings and sums of them to a state: y = H a, H = sum_k c_k P_k (additive to ABI 9: look the symbols up before
 * calling).  Descriptor, `ops`, masks, checks and refusals are those of artn_pauli_query; `coeff` is float64 [n_terms][2]
 * (Re c_k, Im c_k; NULL: every coefficient 1).  With the masks above,
 *     (P a)[i] = (-i)^n_y * (-1)^popcount(i & zmask) * a[i ^ xmask]
 *     y[i]     = sum over groups g of W_g(i) * a[i ^ xmask_g],   W_g(i) = sum_{k in g} f_k * (-1)^popcount(i & zmask_k)
 * f_k = c_k (-i)^n_y the FOLDED coefficient (exact: a swap and sign changes of Re c_k, Im c_k).  `y` has the memory layout of `a`.
 * ONE launch writes every element of y once and never reads y, whatever the number of groups and terms; `a` is only read.
 * Products and sums are float64 for both dtypes (complex64 values are converted first), a complex64 result is rounded once.
 * SUMMATION ORDER of every output element: the groups sorted by xmask >> 10 (the bits above a tile of 2^10 elements; one fetch of
 * the partner tile serves all the groups that share them), ties in the order the groups first appear in the call; inside a group
 * the terms in the caller's order (they are summed into W_g before the one multiplication by the partner).  No atomics:
 * bit-identical from run to run.
 *
 * TERM TABLE (what artn_pauli_apply_pack writes and the kernel reads; 8-byte little-endian fields, 32-byte records):
 *     record 0                      ArtnPauliApplyHeader   n_groups, n_terms, n_xmask_hi, 0
 *     records 1 .. n_groups         ArtnPauliApplyGroup    in summation order: xmask, first, count, 0 -- the group's terms are the
 *                                                          term records first .. first + count - 1 (numbered from 0)
 *     then n_terms records          ArtnPauliApplyTerm     group by group in summation order, the caller's order inside a group:
 *                                                          zmask, zmask & 3 (the sign CLASS of the four elements a thread owns),
 *                                                          Re f_k, Im f_k as float64
 * table_bytes = 32 * (1 + n_groups + n_terms).
 */
typedef struct ArtnPauliApplyHeader {
  uint64_t n_groups, n_terms, n_xmask_hi, reserved;
} ArtnPauliApplyHeader;
typedef struct ArtnPauliApplyGroup {
  uint64_t xmask, first, count, reserved;
} ArtnPauliApplyGroup;
typedef struct ArtnPauliApplyTerm {
  uint64_t zmask, sign_class;
  double re, im;
} ArtnPauliApplyTerm;
typedef struct ArtnPauliApplyInfo {
  int32_t n_groups;     /* distinct xmasks                                          */
  int32_t n_xmask_hi;   /* distinct xmask >> 10: partner tiles fetched per own tile */
  int32_t n_launches;   /* 1                                                        */
  int32_t reserved;
  int64_t table_bytes;
  int64_t bytes_read;    /* nominal: n * element size (every partner tile is a tile of `a`)  */
  int64_t bytes_written; /* n * element size                                                  */
} ArtnPauliApplyInfo;
/* Host-only: validates, translates, groups and orders.  Per term (n_terms entries each, any may be NULL): xmask, zmask, n_y,
 * group (numbered in the order the groups first appear) and folded (float64 [n_terms][2]).  Per group (n_groups <= n_terms
 * entries each, any may be NULL; indexed by group number): group_xmask and group_pos, the group's position in summation order. */
int artn_pauli_apply_query(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_terms,
                           ArtnPauliApplyInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *group, double *folded,
                           uint64_t *group_xmask, int32_t *group_pos);
/* Host-only: writes the term table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_pauli_apply_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_terms, void *table,
                          int64_t table_bytes);
/* y = H a in one launch on `stream`.  `table` is DEVICE memory holding what artn_pauli_apply_pack wrote for the same descriptor,
 * ops and n_terms (the caller copies it there; 8-byte aligned).  `a` and `y` are 16-byte aligned and their byte ranges do not
 * overlap (ARTN_E_UNSUPPORTED / ARTN_E_INVALID); a table_bytes below the query's is ARTN_E_INVALID.  No allocation, copy or
 * synchronisation.  ARTN_E_NODEVICE without a device. */
int artn_pauli_apply(const ArtnMarginalDesc *d, const void *a, void *y, const uint8_t *ops, int64_t n_terms, const void *table,
                     int64_t table_bytes, void *stream);

/*
 * In-place circuits of Pauli steps (additive to ABI 9: look the symbols up before calling).  A CIRCUIT is an ordered list of
 * n_steps STEPS; step k replaces the state by alpha_k a + beta_k P_k a, P_k a Pauli string (`ops` [n_steps][n_dims] as above),
 * `coeff` float64 [n_steps][4] = Re alpha, Im alpha, Re beta, Im beta.  exp(-i theta P) is (cos theta, -i sin theta), P itself
 * (0, 1), a projector (I +- P) / 2 is (1/2, +-1/2).  Steps are never reordered; `a` is updated in place in its own layout.
 * Descriptor, masks, checks and refusals are those of artn_pauli_query.
 *
 * PLAN.  xmask = xm_lo (bits 0..9, inside a tile of 2^10 elements) + xm_hi.  The circuit is cut greedily, in order, into RUNS:
 * a run is extended while the rank over GF(2) of the xm_hi of its steps stays at or below max_rank (a step with xm_hi = 0 never
 * ends a run; a run always takes its first step with xm_hi != 0, so max_rank = 0 gives one run per such step).  A run of rank r
 * is ONE launch that reads and writes the state once: with b_0 .. b_{r-1} the reduced-echelon basis of the span in ascending
 * order of the pivots (pivot p_j is set in b_j and in no other b), the tiles are split into BLOCKS of 2^r tiles, the orbits of
 * the span.  Block q (0 <= q < tiles >> r) has the representative tile whose index is q with a 0 inserted at every pivot (bit
 * p_j - 10 of the tile index), ascending; SLOT s of the block is the tile (representative << 10 ^ XOR of b_j over the bits j of
 * s) >> 10.  A workgroup holds the 2^r tiles of a block together and applies the run's steps to it; step k pairs slot s with slot
 * s ^ m_k, its SLOT MASK: xm_hi = XOR of b_j over the bits j of m_k.
 * max_rank: -1 selects the default, 64 KiB of LDS per workgroup (3 for complex64, 2 for complex128); the maximum is
 * ARTN_PAULI_EVOLVE_MAX_RANK for complex64 and one less for complex128 (128 KiB); more is ARTN_E_UNSUPPORTED, below -1
 * ARTN_E_INVALID.  States below 2^10 elements: one run, one launch, whatever max_rank.
 *
 * ARITHMETIC of a step, for every element i with partner j = i ^ xmask and the sign s = (-1)^popcount(i & zmask):
 *     b = s * (-i)^n_y * a[j]   (sign changes and a swap of the components: exact)
 *     Re new = Re alpha * Re a[i] - Im alpha * Im a[i] + Re beta * Re b - Im beta * Im b, and Im new likewise,
 * operands converted to float64, the four products accumulated by fma from the last one to the first, a product whose coefficient
 * component is exactly 0 left out, one rounding of each component to the dtype.  Between steps the state is held in the dtype, so
 * the result does not depend on where the runs are cut, bit for bit; (1, 0) leaves finite data unchanged bit for bit and (0, 1)
 * is an exact signed permutation.  No atomics.
 *
 * TABLE (what artn_pauli_evolve_pack writes and the kernels read; 8-byte little-endian fields):
 *     ArtnPauliEvolveHeader   32 bytes     n_runs, n_steps, max_rank (the effective one), 0
 *     n_runs x ArtnPauliEvolveRun   96 bytes each: first, count (its steps are first .. first + count - 1), rank, 0,
 *                                   basis[4] (memory-bit masks, 0 beyond the rank), pivot[4] (memory bit numbers)
 *     n_steps x ArtnPauliEvolveStep 64 bytes each, in circuit order: xm_lo, slot_mask, zmask, n_y, then Re alpha, Im alpha,
 *                                   Re beta, Im beta as float64
 * table_bytes = 32 + 96 * n_runs + 64 * n_steps.
 */
#define ARTN_PAULI_EVOLVE_MAX_RANK 4
typedef struct ArtnPauliEvolveHeader {
  uint64_t n_runs, n_steps, max_rank, reserved;
} ArtnPauliEvolveHeader;
typedef struct ArtnPauliEvolveRun {
  uint64_t first, count, rank, reserved;
  uint64_t basis[ARTN_PAULI_EVOLVE_MAX_RANK];
  uint64_t pivot[ARTN_PAULI_EVOLVE_MAX_RANK];
} ArtnPauliEvolveRun;
typedef struct ArtnPauliEvolveStep {
  uint64_t xm_lo, slot_mask, zmask, n_y;
  double alpha_re, alpha_im, beta_re, beta_im;
} ArtnPauliEvolveStep;
typedef struct ArtnPauliEvolveInfo {
  int32_t n_runs;
  int32_t n_launches;    /* = n_runs                                               */
  int32_t max_rank;      /* the effective one: the request or the default, capped by log2 of the number of tiles */
  int32_t reserved;
  int64_t table_bytes;
  int64_t bytes_read;    /* n_runs * n * element size                              */
  int64_t bytes_written; /* the same                                               */
} ArtnPauliEvolveInfo;
/* Host-only: validates, translates and cuts the runs.  Per step (n_steps entries each, any may be NULL): xmask, zmask, n_y, run
 * (the run of the step) and slot_mask.  Per run (room for n_steps entries each, n_runs are written; any may be NULL): run_rank,
 * run_basis ([.][4] memory-bit masks) and run_pivot ([.][4] bit numbers, -1 beyond the rank). */
int artn_pauli_evolve_query(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_steps, int32_t max_rank,
                            ArtnPauliEvolveInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *run,
                            int32_t *slot_mask, int32_t *run_rank, uint64_t *run_basis, int32_t *run_pivot);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query with the same max_rank). */
int artn_pauli_evolve_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_steps, int32_t max_rank,
                           void *table, int64_t table_bytes);
/* The circuit on `a`, in place: one launch per run on `stream`, in order.  `table` is DEVICE memory holding what
 * artn_pauli_evolve_pack wrote for the same descriptor, ops, n_steps and max_rank (8-byte aligned; a table_bytes below the query's
 * is ARTN_E_INVALID); `a` is 16-byte aligned (ARTN_E_UNSUPPORTED otherwise).  No allocation, copy or synchronisation.
 * ARTN_E_NODEVICE without a device. */
int artn_pauli_evolve(const ArtnMarginalDesc *d, void *a, const uint8_t *ops, int64_t n_steps, int32_t max_rank, const void *table,
                      int64_t table_bytes, void *stream);

/*
 * ADJOINT: the same circuits on TWO arrays with transition elements (additive to ABI 9: look the symbols up before calling).
 * `lam` and `phi` share one descriptor (shape, strides, dtype).  For every step k of the circuit, in order:
 *     1. when the step is flagged in `measure` (uint8 [n_steps], non-zero = flagged; NULL flags every step),
 *            t_k = sum_i conj(lam[i]) * b_i,   b_i = s (-i)^n_y phi[i ^ xmask] = (P_k phi)[i]   (ARITHMETIC above),
 *        on the two arrays as they are immediately before step k: operands converted to float64, products accumulated by fma,
 *        partial sums added in a fixed order -- no atomics, bit-identical from run to run for one plan.  The order follows the
 *        blocks of the run, so t_k may differ in the last bits between max_rank values.  out[k] = Re t_k, Im t_k; 0, 0 for a
 *        step that is not flagged;
 *     2. step k is applied to phi and to lam with the ARITHMETIC above: each array ends bit for bit as artn_pauli_evolve leaves it
 *        alone, for every max_rank and every measure.
 * With lam = (U_K .. U_{k+1})^+ H phi_K and the reversed circuit of U_k^+, dE/dtheta_k = 2 Im t_k for U_k = exp(-i theta_k P_k).
 *
 * PLAN, runs, blocks and slots are those of artn_pauli_evolve at the same effective max_rank; a workgroup holds the 2^r tiles of a
 * block of both arrays, so the ranks lie one lower: -1 selects 2 for complex64 and 1 for complex128 (64 KiB of LDS), the maximum is
 * ARTN_PAULI_ADJOINT_MAX_RANK for complex64 and one less for complex128 (128 KiB); more is ARTN_E_UNSUPPORTED, below -1
 * ARTN_E_INVALID.  One launch per run, then one finish launch.
 *
 * TABLE: the layout of artn_pauli_evolve_pack, same table_bytes; the n_y word of a step record also carries the flags:
 *     bits 0..7   n_y        bit 8   1 when the step is measured        bits 16..23   the rank of the step's run
 * WORKSPACE (device, 16-byte aligned): float64 [n_steps][G][4][2], G = min(max(n >> 10, 1), 2048) -- per step, workgroup and wave
 * the Re and Im of a partial sum, written by plain stores; workspace_bytes = 64 * G * n_steps.  Needs no initialisation.
 */
#define ARTN_PAULI_ADJOINT_MAX_RANK 3
typedef struct ArtnPauliAdjointInfo {
  int32_t n_runs;          /* = the launches before the finish launch                */
  int32_t n_launches;      /* n_runs + 1                                             */
  int32_t max_rank;        /* the effective one, as ArtnPauliEvolveInfo              */
  int32_t n_measured;      /* flagged steps                                          */
  int64_t table_bytes;
  int64_t workspace_bytes;
  int64_t bytes_read;      /* 2 * n_runs * n * element size                          */
  int64_t bytes_written;   /* the same                                               */
} ArtnPauliAdjointInfo;
/* Host-only: as artn_pauli_evolve_query (the same per-step and per-run arrays, run_basis and run_pivot [.][4]) at the two-state
 * ranks. */
int artn_pauli_adjoint_query(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, const uint8_t *measure, int64_t n_steps,
                             int32_t max_rank, ArtnPauliAdjointInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *run,
                             int32_t *slot_mask, int32_t *run_rank, uint64_t *run_basis, int32_t *run_pivot);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query with the same max_rank). */
int artn_pauli_adjoint_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, const uint8_t *measure, int64_t n_steps,
                            int32_t max_rank, void *table, int64_t table_bytes);
/* The circuit on `lam` and `phi`, in place, and out[n_steps][2] (device, 8-byte aligned), on `stream`.  `table` is DEVICE memory
 * holding what artn_pauli_adjoint_pack wrote for the same descriptor, ops, n_steps and max_rank (8-byte aligned).  ARTN_E_INVALID: a
 * null pointer, table_bytes or workspace_bytes below the query's, byte ranges of lam and phi that overlap; ARTN_E_UNSUPPORTED: lam,
 * phi or workspace not 16-byte aligned.  No allocation, copy or synchronisation.  ARTN_E_NODEVICE without a device. */
int artn_pauli_adjoint(const ArtnMarginalDesc *d, void *lam, void *phi, const uint8_t *ops, int64_t n_steps, int32_t max_rank,
                       const void *table, int64_t table_bytes, void *workspace, int64_t workspace_bytes, double *out, void *stream);

/*
 * In-place circuits of dense one- and two-qubit gates (additive to ABI 9: look the symbols up before calling).  A CIRCUIT is an
 * ordered list of n_gates GATES; gate g acts on k[g] (1 or 2) distinct dimensions of extent 2, dims[g][0 .. k-1] (dims is int32
 * [n_gates][2]; the second entry of a one-qubit gate is ignored), with the matrix mat[g] (float64 [n_gates][32]: the 2^k x 2^k
 * matrix row-major, Re and Im interleaved, in the first 2 * 4^k entries).  Any matrix, unitary or not.  The convention is that of
 * artn_rdm: the FIRST listed dimension is the most significant digit of the row and column index,
 *     new[.., i0, .., i1, ..] = sum_{j0, j1} U[2 i0 + i1][2 j0 + j1] a[.., j0, .., j1, ..].
 * Gates are never reordered; `a` is updated in place in its own layout.  Descriptor and density checks are those of
 * artn_pauli_query (keep[] ignored).  ARTN_E_UNSUPPORTED: k outside {1, 2} (and the refusals of artn_pauli_evolve_query);
 * ARTN_E_INVALID: a dimension out of range, repeated or of extent other than 2, a matrix entry that is not finite, n_gates < 1.
 *
 * PLAN.  A target dimension of stride 2^b is memory bit b: bits 0..9 lie inside a tile of 2^10 elements, bits >= 10 are HIGH.
 * The circuit is cut greedily, in order, into RUNS: a run is extended while the distinct high target bits of its gates number at
 * most max_rank (a gate without a high bit never ends a run; a run always takes its first gate with a high bit, so a two-qubit
 * gate on two high bits opens a run of rank 2 when max_rank is 0 or 1 -- the unfused form; such a run still takes gates
 * whose high bits are among its own, which need no larger block, and ends at the first gate that brings a new one).  A run of rank r is ONE
 * launch that reads and writes the state once.  Its PIVOTS p_0 < .. < p_{r-1} are its high target bits; this is the block
 * structure of artn_pauli_evolve with the unit vectors 1 << p_j as basis: block q (0 <= q < tiles >> r) has the representative
 * tile whose index is q with a 0 inserted at every bit p_j - 10, ascending, and SLOT s of the block is the representative with
 * bit p_j - 10 set for every bit j of s.  A gate's SLOT MASK has bit j set when p_j is one of its targets.
 * max_rank: -1 selects the default, 64 KiB of LDS per workgroup (3 for complex64, 2 for complex128); the maximum is
 * ARTN_GATES_MAX_RANK for complex64 and one less for complex128; more is ARTN_E_UNSUPPORTED, below -1 ARTN_E_INVALID.  The
 * effective value is capped by log2 of the number of tiles.  States below 2^10 elements: one run, one launch.
 * A gate is THREAD-LOCAL (no LDS traffic, no barrier) when its matrix is diagonal or all its targets lie in memory bits 0..1.
 *
 * ARITHMETIC of a gate.  With T_0 the LAST listed target and T_1 the first one of a two-qubit gate, the row of element i is
 * r = bit T_0 of i + 2 * bit T_1 of i, and
 *     new a[i] = sum over d = 2^k - 1 down to 0 of U[r][r ^ d] * a[i with T_0 flipped if d & 1, T_1 flipped if d & 2]
 * (the element itself comes last).  Operands are converted to float64; a term adds, by fma into accumulators that start at -0.0,
 * first the two products with Im U (-Im U Im a to the real part, Im U Re a to the imaginary part), then the two with Re U; the
 * two products of a coefficient component that is exactly 0 are left out; one rounding of each component to the dtype.  Between
 * gates the state is held in the dtype, so the result does not depend on where the runs are cut, bit for bit; the identity leaves
 * finite data unchanged bit for bit and a matrix with one entry of {1, -1, i, -i} per row and column is an exact signed
 * permutation.  No atomics.
 *
 * TABLE (what artn_gates_pack writes and the kernels read; 8-byte little-endian fields):
 *     ArtnGatesHeader         32 bytes    n_runs, n_gates, max_rank (the effective one), 0
 *     n_runs x ArtnGatesRun   64 bytes each: first, count (its gates are first .. first + count - 1), rank, 0,
 *                             pivot[4] (memory bit numbers, ascending; 0 beyond the rank)
 *     n_gates x ArtnGatesGate 320 bytes each, in circuit order: k, flags (ARTN_GATE_DIAGONAL | ARTN_GATE_LOCAL), then for
 *                             T_0 and T_1 in this order (all 0 for the absent T_1 of a one-qubit gate): bit[2] the memory bit,
 *                             slot[2] the one bit of the slot mask (0: not high), lo[2] the flip mask inside the tile
 *                             (1 << bit below 10, else 0); then m[4][4][2]: U[r][c] as float64 (Re, Im) at m[r][c], rows
 *                             and columns beyond 2^k zero
 * table_bytes = 32 + 64 * n_runs + 320 * n_gates.
 */
#define ARTN_GATES_MAX_RANK 4
#define ARTN_GATE_DIAGONAL 1
#define ARTN_GATE_LOCAL 2
typedef struct ArtnGatesHeader {
  uint64_t n_runs, n_gates, max_rank, reserved;
} ArtnGatesHeader;
typedef struct ArtnGatesRun {
  uint64_t first, count, rank, reserved;
  uint64_t pivot[ARTN_GATES_MAX_RANK];
} ArtnGatesRun;
typedef struct ArtnGatesGate {
  uint64_t k, flags;
  uint64_t bit[2], slot[2], lo[2];
  double m[4][4][2];
} ArtnGatesGate;
typedef struct ArtnGatesInfo {
  int32_t n_runs;
  int32_t n_launches;    /* = n_runs                                               */
  int32_t max_rank;      /* the effective one: the request or the default, capped by log2 of the number of tiles */
  int32_t reserved;
  int64_t table_bytes;
  int64_t bytes_read;    /* n_runs * n * element size                              */
  int64_t bytes_written; /* the same                                               */
} ArtnGatesInfo;
/* Host-only: validates, translates and cuts the runs.  Per gate (n_gates entries each, any may be NULL): bits ([.][2] the memory
 * bits in the order the dims are listed, -1 for the absent second one), run, slot_mask and local (1: thread-local).  Per run
 * (room for n_gates entries each, n_runs are written; any may be NULL): run_rank and run_pivot ([.][4], -1 beyond the rank). */
int artn_gates_query(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                     int32_t max_rank, ArtnGatesInfo *info, int32_t *bits, int32_t *run, int32_t *slot_mask, int32_t *local,
                     int32_t *run_rank, int32_t *run_pivot);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query with the same max_rank). */
int artn_gates_pack(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                    int32_t max_rank, void *table, int64_t table_bytes);
/* The circuit on `a`, in place: one launch per run on `stream`, in order.  `table` is DEVICE memory holding what artn_gates_pack
 * wrote for the same descriptor, k, dims, n_gates and max_rank (8-byte aligned; a table_bytes below the query's is
 * ARTN_E_INVALID); `mat` may be NULL here (the matrices are in the table); `a` is 16-byte aligned (ARTN_E_UNSUPPORTED otherwise).
 * No allocation, copy or synchronisation.  ARTN_E_NODEVICE without a device. */
int artn_gates_apply(const ArtnMarginalDesc *d, void *a, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                     int32_t max_rank, const void *table, int64_t table_bytes, void *stream);

/*
 * GATE ADJOINT: the same circuits on TWO arrays with transition elements (additive to ABI 9: look the symbols up before calling).
 * `lam` and `phi` share one descriptor (shape, strides, dtype).  Gates, dims and mat are those of artn_gates_query.  For every
 * gate g of the circuit, in order:
 *     1. when the gate is flagged in `measure_flag` (uint8 [n_gates], non-zero = flagged; NULL flags no gate),
 *            t_g = sum_i conj(lam[i]) * (M_g phi)[i]
 *        with the matrix measure_mat[g] (float64 [n_gates][32], laid out as mat; any matrix of the gate's size; read for the
 *        flagged gates only, so measure_mat may be NULL when no gate is flagged), on the dims of the gate and on the two arrays as
 *        they are immediately before gate g.  (M phi)[i] is formed by the ARITHMETIC of artn_gates_apply with the coefficients of
 *        M -- float64, d = 2^k - 1 .. 0, the products of an exactly zero component left out -- and is NOT rounded to the dtype;
 *        conj(lam[i]) (M phi)[i] is formed in float64 with one rounding per Re and Im; partial sums are added in a fixed
 *        order -- no atomics, bit-identical from run to run for one plan.  The order follows the blocks of the run, so t_g may
 *        differ in the last bits between max_rank values.  out[g] = Re t_g, Im t_g; 0, 0 for a gate that is not flagged;
 *     2. gate g is applied to phi and to lam: each array ends bit for bit as artn_gates_apply leaves it alone, for every max_rank
 *        and every measure.
 * With lam = (U_K .. U_{k+1})^+ H phi_K, the reversed circuit of the U_k^+ and M_k = dU_k/dtheta U_k^+, dE/dtheta = 2 Re t_k.
 *
 * PLAN, runs, blocks, slots and pivots are those of artn_gates_query at the same effective max_rank; a workgroup holds the 2^r
 * tiles of a block of both arrays, so the ranks lie one lower: -1 selects 2 for complex64 and 1 for complex128 (64 KiB of LDS),
 * the maximum is ARTN_GATES_ADJOINT_MAX_RANK for complex64 and one less for complex128 (128 KiB); more is ARTN_E_UNSUPPORTED,
 * below -1 ARTN_E_INVALID.  A two-qubit gate on two high bits opens a run of rank 2 whatever max_rank is, as there.  One launch
 * per run, then one finish launch.  ARTN_E_INVALID also: an entry of a flagged measure_mat that is not finite.
 *
 * TABLE: ArtnGatesHeader, n_runs x ArtnGatesRun, then n_gates x ArtnGatesAdjointGate, 592 bytes each: the ArtnGatesGate of
 * artn_gates_pack, mm[4][4][2] = M[r][c] as float64 (Re, Im), zero for a gate that is not flagged, and the `measure` word:
 *     bit 0   1 when the gate is measured      bit 1   1 when M is diagonal      bits 8..15   the rank of the gate's run
 * table_bytes = 32 + 64 * n_runs + 592 * n_gates.
 * WORKSPACE (device, 16-byte aligned): float64 [n_gates][G][4][2], G = min(max(n >> 10, 1), 2048) -- per gate, workgroup and wave
 * the Re and Im of a partial sum, written by plain stores; workspace_bytes = 64 * G * n_gates.  Needs no initialisation.
 */
#define ARTN_GATES_ADJOINT_MAX_RANK 3
typedef struct ArtnGatesAdjointGate {
  ArtnGatesGate g;
  double mm[4][4][2];
  uint64_t measure, reserved;
} ArtnGatesAdjointGate;
typedef struct ArtnGatesAdjointInfo {
  int32_t n_runs;          /* = the launches before the finish launch                */
  int32_t n_launches;      /* n_runs + 1                                             */
  int32_t max_rank;        /* the effective one, as ArtnGatesInfo                    */
  int32_t n_measured;      /* flagged gates                                          */
  int64_t table_bytes;
  int64_t workspace_bytes;
  int64_t bytes_read;      /* 2 * n_runs * n * element size                          */
  int64_t bytes_written;   /* the same                                               */
} ArtnGatesAdjointInfo;
/* Host-only: as artn_gates_query (the same per-gate and per-run arrays, run_pivot [.][4]) at the two-state ranks. */
int artn_gates_adjoint_query(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat,
                             const double *measure_mat, const uint8_t *measure_flag, int64_t n_gates, int32_t max_rank,
                             ArtnGatesAdjointInfo *info, int32_t *bits, int32_t *run, int32_t *slot_mask, int32_t *local,
                             int32_t *run_rank, int32_t *run_pivot);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query with the same max_rank). */
int artn_gates_adjoint_pack(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat,
                            const double *measure_mat, const uint8_t *measure_flag, int64_t n_gates, int32_t max_rank, void *table,
                            int64_t table_bytes);
/* The circuit on `lam` and `phi`, in place, and out[n_gates][2] (device, 8-byte aligned), on `stream`.  `table` is DEVICE memory
 * holding what artn_gates_adjoint_pack wrote for the same descriptor, k, dims, n_gates and max_rank (8-byte aligned).
 * ARTN_E_INVALID: a null pointer, table_bytes or workspace_bytes below the query's, byte ranges of lam and phi that overlap;
 * ARTN_E_UNSUPPORTED: lam, phi or workspace not 16-byte aligned.  No allocation, copy or synchronisation.  ARTN_E_NODEVICE
 * without a device. */
int artn_gates_adjoint(const ArtnMarginalDesc *d, void *lam, void *phi, const int32_t *k, const int32_t *dims, int64_t n_gates,
                       int32_t max_rank, const void *table, int64_t table_bytes, void *workspace, int64_t workspace_bytes,
                       double *out, void *stream);

/*
 * ONE dense gate on one to five qubits, in place, in one launch (additive to ABI 9: look the symbols up before calling).  The
 * gate acts on k (1..5) distinct dimensions of extent 2, dims[0 .. k-1], with the matrix mat (float64 [2 * 4^k]: the 2^k x 2^k
 * matrix row-major, Re and Im interleaved).  Any matrix, unitary or not.  The convention is that of artn_gates_*: the FIRST
 * listed dimension is the most significant digit of the row and column index,
 *     new[.., i0, .., i_{k-1}, ..] = sum_j U[(i0 .. i_{k-1})_2][(j0 .. j_{k-1})_2] a[.., j0, .., j_{k-1}, ..].
 * Descriptor and density checks are those of artn_gates_query.  ARTN_E_UNSUPPORTED: k outside 1..5 (and the layout and dtype
 * refusals of artn_gates_query); ARTN_E_INVALID: k above the number of memory bits of the state, a dimension out of range,
 * repeated or of extent other than 2, a matrix entry that is not finite, a null pointer.
 *
 * PLAN.  A target dimension of stride 2^b is memory bit b.  The state is cut into TILES of 2^TB elements, TB =
 * ARTN_WGATE_TILE_BITS_C64 / _C128 (32 KiB of LDS), or the whole state when it is smaller.  The TILE BITS are the k target bits
 * and the TB - k lowest memory bits that are not targets; tile-local bit j is the j-th tile bit in ascending order.  Memory bits
 * 0 .. TB-k-1 always lie in the tile, so a tile is made of contiguous SEGMENTS of `segment` >= 2^(TB-k) elements (segment = 2^s,
 * s the number of leading tile bits j that are memory bit j); the tile bits above s are all targets, the HIGH targets.  Tile q
 * starts at the element whose index is q << s with a 0 inserted at every high target bit, ascending.
 *
 * IN LDS an element of the tile with row c (bit i of c = the bit of the i-th target counted from the LAST listed one) and
 * GROUP g (its TB - k non-target tile bits, compacted) lies at index ((c << (TB-k)) | g) ^ sw(c), sw(c) = XOR of swizzle[i] over
 * the set bits i of c.  A workgroup loads the tile (16-byte global loads), forms every output from the 2^k members of its group
 * read from LDS, writes the outputs back to LDS once every thread has read, and stores the tile (16-byte global stores): one
 * read and one write of the state.  The swizzle moves the targets among the lowest six tile-local bits to LDS index bits of
 * their own, so that the consecutive elements a wavefront loads or stores spread over the LDS banks whatever the targets.
 *
 * ARITHMETIC: that of artn_gates_apply, stated for any k.  For output row r the accumulators of both components start at -0.0;
 * terms come in the order d = 2^k - 1 .. 0 with column c = r ^ d; a term adds, by fma in float64, first the two products with
 * Im U (-Im U Im a to the real part, Im U Re a to the imaginary part), then the two with Re U; the two products of a coefficient
 * component that is exactly 0 are left out; one rounding of each component to the dtype.  So the identity leaves finite data
 * unchanged bit for bit, a matrix with one entry of {1, -1, i, -i} per row and column is an exact signed permutation, a gate with
 * k <= 2 gives what artn_gates_apply gives bit for bit, and so does a one- or two-qubit matrix kron identities.  No atomics.
 *
 * TABLE (what artn_wgate_pack writes and the kernel reads; 8-byte little-endian fields): ArtnWgateTable, 480 bytes, then the
 * matrix as float64 (Re, Im), row-major, 16 * 4^k bytes.  table_bytes = 480 + 16 * 4^k.
 */
#define ARTN_WGATE_MAX_K 5
#define ARTN_WGATE_TILE_BITS_C64 12
#define ARTN_WGATE_TILE_BITS_C128 11
#define ARTN_WGATE_ROWS 8 /* a thread forms up to this many rows of a group; block_mask is over blocks of ROWS x ROWS entries */
typedef struct ArtnWgateTable {
  uint64_t k, tile_bits, n_tiles, segment;
  uint64_t flags;      /* ARTN_GATE_DIAGONAL                                                                        */
  uint64_t group_bits; /* tile_bits - k                                                                              */
  uint64_t n_high;     /* tile bits at or above log2(segment): all targets                                           */
  uint64_t block_mask; /* bit rb * nb + cb (nb = max(1, 2^k / ROWS)): block (rb, cb) of the matrix has a non-zero    */
  uint64_t target_bit[ARTN_WGATE_MAX_K]; /* the memory bits of the targets in the order listed                       */
  uint64_t target_pos[ARTN_WGATE_MAX_K]; /* their tile-local positions, same order                                   */
  uint64_t high_bit[ARTN_WGATE_MAX_K];   /* the high targets' memory bits, ascending (0 beyond n_high)                */
  uint64_t swizzle[ARTN_WGATE_MAX_K];    /* per ROW bit i (the i-th target from the last listed one), below 2^group_bits */
  uint64_t mem_col[16];                  /* per tile-local bit j: 1 << its memory bit (0 beyond tile_bits): the bit scatter */
  uint64_t lds_col[16];                  /* per tile-local bit j: what it contributes (XOR) to the LDS index             */
} ArtnWgateTable;
typedef struct ArtnWgateInfo {
  int32_t k;
  int32_t tile_bits;   /* TB, or log2 of the state when that is smaller          */
  int32_t diagonal;    /* 1: every off-diagonal entry is exactly 0               */
  int32_t reserved;
  int64_t n_tiles;     /* n_tiles << tile_bits = elements of the state           */
  int64_t segment;     /* elements of a contiguous segment of a tile             */
  int64_t lds_bytes;
  int64_t table_bytes;
  int64_t bytes_read;  /* the state                                              */
  int64_t bytes_written;
} ArtnWgateInfo;
/* Host-only: validates and plans.  target_bits (k entries, the order listed) and tile_bits (info->tile_bits entries, ascending;
 * room for 12) may be NULL. */
int artn_wgate_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, ArtnWgateInfo *info,
                     int32_t *target_bits, int32_t *tile_bits);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_wgate_pack(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, void *table, int64_t table_bytes);
/* The gate on `a`, in place: ONE launch on `stream`.  `table` is DEVICE memory holding what artn_wgate_pack wrote for the same
 * descriptor, k and dims (8-byte aligned; a table_bytes below the query's is ARTN_E_INVALID); `a` is 16-byte aligned
 * (ARTN_E_UNSUPPORTED otherwise).  No allocation, copy or synchronisation.  ARTN_E_NODEVICE without a device. */
int artn_wgate_apply(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, const void *table, int64_t table_bytes,
                     void *stream);

/*
 * ONE dense gate on three to seven qubits, in place, in one launch, on the float64 MATRIX CORES (additive to ABI 9:
 * has("artn_mgate_apply")).  A family beside artn_wgate_*, with an arithmetic contract of its own; the three calls mirror the
 * three artn_wgate_* calls in arguments, error codes and error texts (the wording "matrix gates take ...", and k outside 3..7 is
 * ARTN_E_UNSUPPORTED "matrix gates act on three to seven dimensions").  mat, dims and the convention (the FIRST listed dimension
 * is the most significant digit) are those of artn_wgate_query.
 *
 * PLAN: that of artn_wgate_query, unchanged and for k up to 7 -- tiles of 2^TB elements (TB = ARTN_WGATE_TILE_BITS_C64 / _C128, or
 * the whole state), the tile bits the k targets and the lowest other bits, segments, the tile base with a 0 inserted at every high
 * target, the LDS image ((c << GB) | g) ^ sw(c) with GB = TB - k, and the column tables.  At k = 7 a full tile has 2^5 (complex64)
 * or 2^4 (complex128) groups, so a segment is never below 256 bytes.
 *
 * KERNEL: 256 threads = 4 wavefronts grid-stride over the tiles.  Per tile: (1) 16-byte loads into the LDS image; (2) the complex
 * GEMM Y[2^k x G] = U X[2^k x G] (G = 2^GB groups) as a real one on v_mfma_f64_16x16x4_f64; (3) after a barrier every output
 * component is rounded once to the dtype and written to its place in LDS; (4) 16-byte stores.  One instruction multiplies a ROW
 * BLOCK rb (output rows 8 rb .. 8 rb + 7) and a STEP s (input rows 2 s and 2 s + 1) with a COLUMN BLOCK cb (groups 16 cb ..
 * 16 cb + 15).  A state with fewer than 16 groups reads group (g mod G) for the missing columns and does not write them.
 *
 * ARITHMETIC.  The component (row r, re or im) of group g is a float64 sum of its 2 * 2^k real products: the accumulator starts
 * at +0.0; the steps come in the order s = 0 .. 2^(k-1) - 1; step s adds, in the order the instruction adds its four products,
 * U[r][2s] x[2s], U[r][2s+1] x[2s+1] with (Re U Re x, -Im U Im x) for the real part and (Im U Re x, Re U Im x) for the imaginary
 * part.  One rounding of each component to the dtype.  No atomics: results are bit-identical from run to run and between an eager
 * call and a graph replay.  Where every product and every partial sum is exactly representable (integers below 2^53; below 2^24
 * after the final rounding for complex64) the result is exact whatever the order, so on finite data the identity and signed
 * permutations reproduce their input values under ==.  UNLIKE artn_wgate_apply, zero coefficients are multiplied: the sign of a
 * zero is not preserved, and a non-finite element may make every output of its group non-finite.  The result is not bit for bit
 * artn_wgate_apply's; every component agrees with the exact one within
 *     2^-24 |exact| (complex64: the one rounding) + 4 * 2^k * 2^-53 * sum_c (|Re u| + |Im u|)(|Re x| + |Im x|)
 * (a float64 sum of 2^(k+1) products in any order, with a factor 2 of slack).
 *
 * TABLE (what artn_mgate_pack writes and the kernel reads; 8-byte little-endian fields): ArtnMgateTable, 544 bytes, then the matrix
 * as float64 in FRAGMENT ORDER, 16 * 4^k bytes: the double at index
 *     ((((rb * 2^(k-1) + s) * 8 + n) * 2 + h) * 2 + c)        rb < 2^k / 8, s < 2^(k-1), n < 8, h < 2, c < 2
 * is Re (c = 0) or Im (c = 1) of U[8 rb + n][2 s + h].  Lane l of a wavefront (j = l & 15, q = l >> 4) takes for (rb, s) the
 * entry n = j >> 1, h = q >> 1, c = (j ^ q) & 1, with its sign flipped when j is even and q is odd.  table_bytes = 544 + 16 * 4^k
 * (256 KiB + 544 at k = 7).
 */
#define ARTN_MGATE_MIN_K 3
#define ARTN_MGATE_MAX_K 7
typedef struct ArtnMgateTable {
  uint64_t k, tile_bits, n_tiles, segment;
  uint64_t flags;      /* ARTN_GATE_DIAGONAL                                                                          */
  uint64_t group_bits; /* tile_bits - k                                                                                */
  uint64_t n_high;     /* tile bits at or above log2(segment): all targets                                             */
  uint64_t reserved;
  uint64_t target_bit[ARTN_MGATE_MAX_K]; /* the memory bits of the targets in the order listed                         */
  uint64_t target_pos[ARTN_MGATE_MAX_K]; /* their tile-local positions, same order                                     */
  uint64_t high_bit[ARTN_MGATE_MAX_K];   /* the high targets' memory bits, ascending (0 beyond n_high)                  */
  uint64_t swizzle[ARTN_MGATE_MAX_K];    /* per ROW bit i (the i-th target from the last listed one), below 2^group_bits */
  uint64_t mem_col[16];                  /* per tile-local bit j: 1 << its memory bit (0 beyond tile_bits)               */
  uint64_t lds_col[16];                  /* per tile-local bit j: what it contributes (XOR) to the LDS index             */
} ArtnMgateTable;
typedef ArtnWgateInfo ArtnMgateInfo; /* the same fields; table_bytes = 544 + 16 * 4^k */
/* Host-only: validates and plans.  target_bits (k entries, the order listed) and tile_bits (info->tile_bits entries, ascending;
 * room for 12) may be NULL. */
int artn_mgate_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, ArtnMgateInfo *info,
                     int32_t *target_bits, int32_t *tile_bits);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_mgate_pack(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, void *table, int64_t table_bytes);
/* The gate on `a`, in place: ONE launch on `stream`.  `table` is DEVICE memory holding what artn_mgate_pack wrote for the same
 * descriptor, k and dims (8-byte aligned; a table_bytes below the query's is ARTN_E_INVALID; a table packed for another k makes
 * the launch return without touching memory); `a` is 16-byte aligned (ARTN_E_UNSUPPORTED otherwise).  No allocation, copy or
 * synchronisation.  ARTN_E_NODEVICE without a device. */
int artn_mgate_apply(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, const void *table, int64_t table_bytes,
                     void *stream);

/* ---- the vector algebra of Krylov drivers (additive to ABI 9: has("artn_krylov_combine")) ------------------------------------
 * Vectors are complex64 or complex128 arrays of n elements (1 <= n <= 2^40) in DEVICE memory, 16-byte aligned; every vector of a
 * call has the same dtype and the same dense layout, so the kernels work on the flat memory range.  float64 arithmetic in an
 * order fixed by n alone, no atomics: results are bit-identical from run to run.
 *
 * artn_krylov_dots: out[2j], out[2j + 1] = Re, Im <V_j|w> for j < m and out[2m] = |w|^2 (DEVICE memory, 2m + 1 doubles), each bit
 *   for bit what artn_born_overlap(V_j, w) reports as <a|b> and |b|^2, whatever m is.  The vectors are taken ARTN_KRYLOV_BATCH at a
 *   time: ceil(m / ARTN_KRYLOV_BATCH) streaming launches, each reading w once and its V_j once, and one finish launch.
 * artn_krylov_combine: y <- sum_{j < m} c_j X_j in ONE streaming launch, m <= ARTN_KRYLOV_MAX_VECS, c_j = coeff[2j] + i coeff[2j + 1]
 *   (HOST memory; they travel in the kernel arguments), and out4 (DEVICE memory, 4 doubles, laid out as artn_born_overlap's with
 *   b = NULL: {|y|^2, 0, |y|^2, |y|^2}) = the norm of the values as stored, bit for bit artn_born_overlap(y, NULL) of the result.
 *   Every component is one float64 fma chain over j in the caller's order -- the real part takes c_r x_r then -c_i x_i, the imaginary
 *   part c_r x_i then c_i x_r -- that starts from the first product and is rounded once, at the store.  A term whose coefficient is
 *   exactly 0 + 0i is dropped before the launch (its vector is never read; all dropped: y = 0).  y may BE one of the X_j (the same
 *   pointer); any other overlap of y with an X_j is refused.
 * Both run on `stream` with a caller-supplied workspace and do no allocation, copy or synchronisation.
 * ARTN_E_INVALID: a null pointer, m < 1, m above ARTN_KRYLOV_MAX_VECS (combine), n out of range, a workspace below the query's,
 * a partial overlap, a coefficient that is not finite.  ARTN_E_UNSUPPORTED: another dtype, a pointer that is not 16-byte aligned.
 * ARTN_E_NODEVICE without a device. */
#define ARTN_KRYLOV_BATCH 8     /* vectors per launch of artn_krylov_dots (at most 16; DESIGN section 16 has the register table) */
#define ARTN_KRYLOV_MAX_VECS 64 /* vectors of one artn_krylov_combine                                                          */
typedef struct ArtnKrylovInfo {
  int32_t grid;             /* workgroups of every streaming launch: artn_born_plan's overlap_grid                  */
  int32_t batch;            /* ARTN_KRYLOV_BATCH                                                                     */
  int32_t dots_launches;    /* streaming launches of artn_krylov_dots: ceil(m / batch); one finish launch follows   */
  int32_t combine_launches; /* streaming launches of artn_krylov_combine: 1; one finish launch follows              */
  int64_t dots_workspace_bytes;    /* 32 bytes x grid x (ceil(m / 2) + 1)                                            */
  int64_t combine_workspace_bytes; /* 8 bytes x grid                                                                 */
  int64_t dots_bytes_read;         /* nominal: (m + dots_launches) vectors                                           */
  int64_t combine_bytes_read;      /* nominal: m vectors (terms with a zero coefficient included)                    */
  int64_t combine_bytes_written;   /* one vector                                                                     */
} ArtnKrylovInfo;
/* Host-only: validates n, dtype and m (m >= 1; artn_krylov_combine itself refuses m above ARTN_KRYLOV_MAX_VECS). */
int artn_krylov_query(int64_t n, int32_t dtype, int32_t m, ArtnKrylovInfo *info);
int artn_krylov_dots(const void *const *vecs, int32_t m, const void *w, int64_t n, int32_t dtype, void *ws, int64_t ws_bytes,
                     double *out, void *stream);
int artn_krylov_combine(void *y, const double *coeff, const void *const *xs, int32_t m, int64_t n, int32_t dtype, void *ws,
                        int64_t ws_bytes, double *out4, void *stream);

/* ---- projective measurement, post-selection and reset, in place (additive to ABI 9: has("artn_measure_collapse")) -------------
 * The state is a DENSE tensor of power-of-two extents in DEVICE memory, 16-byte aligned (descriptor, density checks and size
 * limits of artn_pauli_query).  The dimensions with keep[] != 0 are the MEASURED ones, 1 to ARTN_MEASURE_MAX_DIMS of them, each of
 * extent 2; an outcome is the integer whose most significant digit is the first of them in the descriptor's order (the convention
 * of artn_rdm), D = 2^k outcomes.  A measured dimension of stride 2^b is bit b of the flat memory index.
 *
 * artn_measure_choose: one small launch.  q (DEVICE, D float64, what artn_marginal writes for the same descriptor) and `uniform`
 *   (DEVICE, one float64 in [0, 1); may be NULL where forced_outcome >= 0) give the record (DEVICE, 32 bytes, 8-byte aligned):
 *       int64 outcome; float64 probability, total, scale;
 *   total = q[0] + q[1] + ... in ascending order.  forced_outcome < 0: the outcome is the smallest o whose inclusive running sum
 *   (the same additions) exceeds uniform * total, or the last o with q[o] > 0 where rounding leaves none; an o with q[o] == 0 is
 *   never chosen.  forced_outcome >= 0: that outcome (post-selection).  probability = q[o] / total; scale = sqrt(total / q[o])
 *   where renormalize != 0, else 1.  Where total is not finite, total is not > 0 or the forced q[o] is not > 0, nothing can be
 *   observed: outcome = -1, probability = 0, scale = 1.
 * artn_measure_collapse: reads the record from DEVICE memory.  Outcome -1 leaves the state untouched bit for bit.  Otherwise every
 *   element whose measured digits differ from the outcome becomes +0.0 in both components -- written, never read, so -0.0,
 *   denormals and non-finite values there vanish -- and every kept component c becomes fl(float64(c) * scale), one rounding;
 *   under scale == 1 kept elements are unchanged bit for bit.  reset != 0: the kept element a[r, o] * scale lands at [r, 0..0]
 *   instead and every other element becomes +0.0 (two launches: a move that reads only elements with digits o and writes only
 *   elements with digits 0 -- and +0.0 to the second half of a 16-byte vector it stores, where memory bit 0 of complex64 is
 *   measured -- then a zero-fill of everything else; the result does not depend on scheduling, no buffer is used).
 *   One streaming launch (reset: two) over memory order, 16 bytes per lane, plain stores, no atomics.
 * Both run on `stream` and do no allocation, copy or synchronisation.
 * ARTN_E_INVALID: a null pointer, a layout that is not dense, a measured dimension whose extent is not 2, none or more than
 * ARTN_MEASURE_MAX_DIMS of them, D < 1.  ARTN_E_UNSUPPORTED: another dtype, an extent that is no power of two, more than 96
 * dimensions or 2^40 elements, a state that is not 16-byte aligned or a record that is not 8-byte aligned.  ARTN_E_NODEVICE
 * without a device (the query is host-only). */
#define ARTN_MEASURE_MAX_DIMS 10
#define ARTN_MEASURE_RECORD_BYTES 32
typedef struct ArtnMeasureInfo {
  int32_t k;                 /* measured dimensions                                                              */
  int32_t grid;              /* workgroups of a streaming launch                                                 */
  int32_t collapse_launches; /* 1                                                                                */
  int32_t reset_launches;    /* 2: move, clear                                                                   */
  int64_t dim;               /* D = 2^k outcomes                                                                 */
  int64_t n;                 /* elements of the state                                                            */
  int64_t record_bytes;      /* ARTN_MEASURE_RECORD_BYTES                                                        */
  int64_t bytes_read;        /* nominal, collapse and reset alike: the n / D kept elements                       */
  int64_t bytes_written;     /* nominal, collapse and reset alike: all n elements                                */
  int32_t mem_bit[ARTN_MEASURE_MAX_DIMS]; /* memory bit of measured dimension j, in listed order; the rest -1    */
} ArtnMeasureInfo;
/* Host-only: validates the layout and the measured dimensions, reports the plan. */
int artn_measure_query(const ArtnMarginalDesc *d, ArtnMeasureInfo *info);
int artn_measure_choose(const double *q, int64_t D, const double *uniform, int64_t forced_outcome, int32_t renormalize, void *record,
                        void *stream);
int artn_measure_collapse(const ArtnMarginalDesc *d, void *a, const void *record, int32_t reset, void *stream);

/*
 * ONE dense gate on one to five TARGET qubits under any number of CONTROL qubits, optionally under a classical condition read
 * from device memory, in place, in one launch (additive to ABI 9: has("artn_cgate_apply")).  targets[0 .. t-1] (t = 1..5) and
 * controls[0 .. c-1] (c >= 0; NULL where c == 0) are distinct dimensions of extent 2, disjoint from each other; every dimension
 * that is no target may be a control.  control_values[j] is 0 or 1, the digit control j must have (NULL: all 1).  mat is the
 * 2^t x 2^t matrix of artn_wgate_query on the targets, the FIRST listed target the most significant digit; any finite matrix.
 *
 * CONTRACT.  An element is SELECTED when its control digits equal control_values.  A selected element becomes what the
 * ARITHMETIC contract of artn_wgate_apply gives for mat on the targets (terms d = 2^t - 1 .. 0, accumulators from -0.0, float64
 * fma, products of exactly-zero coefficient components left out, one rounding per component).  An UNSELECTED element keeps its
 * bits -- the sign of a zero, NaN payloads, denormals, infinities: no arithmetic touches it; one that shares a tile with selected
 * elements may be loaded and stored back raw, the elements of every other tile are neither read nor written.  So c = 0 and no
 * condition is artn_wgate_apply bit for bit; for c + t <= 5 on finite data the result is artn_wgate_apply of the matrix
 * |v><v| (x) U + (1 - |v><v|) (x) I bit for bit; the identity changes nothing; a signed permutation is exact; the controls count
 * as a set of (dimension, value) pairs.  No atomics: results are bit-identical from run to run.
 * CONDITION.  cond is NULL or points at an int64 o in DEVICE memory (8-byte aligned): the gate is applied iff o >= 0 and
 * (o & cond_mask) == cond_value.  Otherwise every workgroup returns before its first access to the state, which stays untouched
 * bit for bit.  The first 8 bytes of the record of artn_measure_choose are such an int64; its outcome -1 never triggers a gate.
 *
 * PLAN.  A dimension of stride 2^b is memory bit b; LB = 4 (complex64) or 3 (complex128) is the number of index bits of a
 * 128-byte line.  A control below bit LB is a LOW control: skipping it would save no memory traffic, so it stays an ordinary
 * index bit of the tile.  Every other control is a HIGH control and is removed from the index space: the launch walks only the
 * n >> c_high elements whose high control bits are as wanted.  The TILE BITS are the t target bits and the lowest memory bits
 * that are neither targets nor high controls, TB = ARTN_WGATE_TILE_BITS_C64 / _C128 in all or the whole selected sub-state
 * (log2 n - c_high bits) where that is smaller -- one workgroup then; tile-local bit j is the j-th tile bit in ascending order.
 * Bits 0 .. LB-1 always lie in the tile, so it is made of contiguous SEGMENTS of `segment` = 2^s elements, at least 128 bytes
 * where the state has them (s = the number of leading tile bits j that are memory bit j).  The HOLES are the tile bits at or
 * above s and the high controls; tile q starts at the element whose index is q << s with a 0 inserted at every hole bit,
 * ascending, OR high_want.  LDS layout, swizzle, phases and block_mask are those of artn_wgate_apply with k = t; a low control
 * is one of the group bits, and an item whose group index g has (g & group_mask) != group_want is not computed: the LDS image
 * keeps what was loaded and the store phase writes it back raw.
 *
 * TABLE (what artn_cgate_pack writes and the kernel reads; 8-byte little-endian fields): ArtnCgateTable, 1000 bytes, then the
 * matrix as float64 (Re, Im), row-major, 16 * 4^t bytes.  table_bytes = 1000 + 16 * 4^t.
 *
 * ARTN_E_UNSUPPORTED: t outside 1..5, the layout and dtype refusals of artn_wgate_query, a table that is not 8-byte aligned,
 * an array that is not 16-byte aligned, a cond that is not 8-byte aligned.  ARTN_E_INVALID: c < 0, t above the number of memory
 * bits, a dimension out of range, repeated, both target and control, or of extent other than 2, a control value other than 0 / 1,
 * a matrix entry that is not finite, a null pointer, a table smaller than the query's.
 */
#define ARTN_CGATE_MAX_HOLES 64
typedef struct ArtnCgateTable {
  uint64_t t, tile_bits, n_tiles, segment;
  uint64_t flags;        /* ARTN_GATE_DIAGONAL                                                                        */
  uint64_t group_bits;   /* tile_bits - t                                                                              */
  uint64_t segment_bits; /* log2(segment)                                                                              */
  uint64_t block_mask;   /* as ArtnWgateTable's                                                                        */
  uint64_t n_holes;      /* entries of hole_bit                                                                        */
  uint64_t high_want;    /* OR of 1 << b over the high controls b whose wanted value is 1                              */
  uint64_t high_mask;    /* OR of 1 << b over the high controls                                                        */
  uint64_t group_mask;   /* OR of 1 << r over the low controls, r the control's bit of the group index                 */
  uint64_t group_want;   /* the same over the low controls whose wanted value is 1                                     */
  uint64_t target_bit[ARTN_WGATE_MAX_K]; /* the memory bits of the targets in the order listed                        */
  uint64_t target_pos[ARTN_WGATE_MAX_K]; /* their tile-local positions, same order                                    */
  uint64_t swizzle[ARTN_WGATE_MAX_K];    /* per ROW bit i (the i-th target from the last listed one)                  */
  uint64_t mem_col[16];                  /* per tile-local bit j: 1 << its memory bit (0 beyond tile_bits)            */
  uint64_t lds_col[16];                  /* per tile-local bit j: what it contributes (XOR) to the LDS index          */
  uint64_t hole_bit[ARTN_CGATE_MAX_HOLES]; /* ascending: tile bits at or above segment_bits, and the high controls    */
  uint64_t reserved;
} ArtnCgateTable;
typedef struct ArtnCgateInfo {
  int32_t t, c;
  int32_t c_high, c_low;
  int32_t tile_bits;     /* TB, or log2 of the selected sub-state when that is smaller   */
  int32_t diagonal;      /* 1: every off-diagonal entry is exactly 0                      */
  int64_t n_selected;    /* n >> c: the elements the gate acts on                         */
  int64_t n_tiles;       /* n_tiles << tile_bits = n >> c_high                            */
  int64_t segment;       /* elements of a contiguous segment of a tile                    */
  int64_t lds_bytes;
  int64_t table_bytes;
  int64_t bytes_read;    /* (n >> c_high) elements                                        */
  int64_t bytes_written;
} ArtnCgateInfo;
/* Host-only: validates and plans.  target_bits (t entries, the order listed), control_bits (c entries, the order listed) and
 * tile_bits (info->tile_bits entries, ascending; room for 12) may be NULL. */
int artn_cgate_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                     const int32_t *control_values, const double *mat, ArtnCgateInfo *info, int32_t *target_bits,
                     int32_t *control_bits, int32_t *tile_bits);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_cgate_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                    const int32_t *control_values, const double *mat, void *table, int64_t table_bytes);
/* The gate on `a`, in place: ONE launch on `stream`.  `table` is DEVICE memory holding what artn_cgate_pack wrote for the same
 * descriptor, targets, controls and control values.  No allocation, copy or synchronisation.  ARTN_E_NODEVICE without a device. */
int artn_cgate_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                     const int32_t *control_values, const void *table, int64_t table_bytes, const void *cond, int64_t cond_mask,
                     int64_t cond_value, void *stream);

/*
 * NOISE CHANNELS for quantum trajectories: one of m operators on t target qubits is drawn ON THE DEVICE and applied in place
 * (additive to ABI 9: has("artn_channel_apply")).  dims[0 .. t-1] (t = 1..5) are distinct dimensions of extent 2, the FIRST listed
 * one the most significant digit (the convention of artn_wgate_query, artn_marginal and artn_rdm); mats holds the m (1..256)
 * operators as float64 [m][2 * 4^t], each a 2^t x 2^t matrix row-major, Re and Im interleaved.  D = 2^t.
 *
 * FORM (decided by the caller at pack time) says where the weights w_j of the draw come from:
 *   ARTN_CHANNEL_FIXED     weights[m]: w_j = weights[j].  mats are the U_j of a mixture sum_j p_j U_j rho U_j^+ as given; no pass over
 *                          the state is made for the draw, `input` of artn_channel_choose is not read and scale is exactly 1.
 *   ARTN_CHANNEL_DIAGONAL  weights[m][D]: e_j[d] = sum_r |K_j[r,d]|^2 (every K_j has at most one non-zero per column, so K_j^+ K_j is
 *                          diagonal).  input = q, the D float64 artn_marginal writes for dims.  w_j = sum_d e_j[d] q[d]: an fma chain
 *                          from 0.0 over d ascending.  trace = q[0] + q[1] + ... ascending.
 *   ARTN_CHANNEL_DENSE     weights[m][D][D][2]: E_j = K_j^+ K_j row-major (Re, Im).  input = rho, the [D][D][2] float64 artn_rdm writes
 *                          for dims.  w_j = sum_{a,b} Re(E_j[a,b] rho[b,a]): an fma chain from 0.0 over a ascending, inside it b
 *                          ascending, per (a, b) first + Re E Re rho, then - Im E Im rho.  trace = Re rho[0,0] + Re rho[1,1] + ...
 * A w_j below 0 (rounding residue) or NaN counts as 0.
 *
 * artn_channel_choose: ONE workgroup.  Lanes form the w_j, one operator per lane at a time; one lane then applies the choice rule
 *   of artn_measure_choose to them: total = w_0 + w_1 + ... ascending; j is the smallest index whose inclusive running sum (the
 *   same additions) exceeds uniform * total, or the last j with w_j > 0 where rounding leaves none; a j with w_j == 0 is never
 *   chosen.  The RECORD (DEVICE, record_bytes of the query, 8-byte aligned) starts with the 32 bytes of artn_measure_choose's:
 *       int64 j; float64 probability = w_j / total, total, scale;
 *   scale = sqrt(trace / w_j), so that sum |a|^2 after the step equals trace; scale = 1 where renormalize == 0 and in the FIXED
 *   form.  Where total (or, outside the FIXED form, trace) is not finite or not > 0 nothing can be drawn: j = -1, probability 0,
 *   scale 1.  Behind the 32 bytes lies the CURRENT MATRIX, float64 [2 * 4^t]: every component of operator j times scale, one
 *   float64 multiply each (all +0.0 where j = -1).
 * artn_channel_apply: ONE launch, the tile kernel of artn_wgate_apply with the current matrix as its matrix; PLAN, LDS layout and
 *   ARITHMETIC are artn_wgate_apply's, so the state afterwards is bit for bit what artn_wgate_apply gives for the current matrix.
 *   The kernel reads j from the record.  Where j < 0 or j >= m, and where operator j is an exact identity matrix (flagged at pack
 *   time) and scale == 1.0, every workgroup returns before its first access to the state, which stays untouched bit for bit --
 *   non-finite data included, which artn_wgate_apply of the identity promises for finite data only.  The all-zero 8 x 8 blocks of
 *   operator j (its block_mask, from the table) are skipped as artn_wgate_apply skips those of its matrix.
 * Both run on `stream`, take the caller's buffers and do no allocation, copy or synchronisation.  No atomics: results are
 * bit-identical from run to run.
 *
 * TABLE (what artn_channel_pack writes and the kernels read; 8-byte little-endian fields): ArtnChannelTable, 512 bytes -- its
 * first 480 bytes are an ArtnWgateTable for the same descriptor and dims whose block_mask is the OR and whose flags the AND over
 * the operators, so with m = 1 it is what artn_wgate_pack writes for that matrix -- then m ArtnChannelOp (16 bytes each), then the
 * weights (8 * weight_doubles * m bytes), then the m matrices (16 * 4^t bytes each).
 *
 * ARTN_E_UNSUPPORTED: t outside 1..5, the layout and dtype refusals of artn_wgate_query in the wording "channels take ...", a
 * table, record or array that is not aligned (table, record, input, uniform: 8 bytes; the state: 16).  ARTN_E_INVALID: m outside
 * 1..256, an unknown form, t above the number of memory bits, a dimension out of range, repeated or of extent other than 2, a
 * matrix entry or weight that is not finite, a null pointer, a table or record smaller than the query's.  ARTN_E_NODEVICE without a
 * device (query and pack are host-only).
 */
#define ARTN_CHANNEL_MAX_OPS 256
#define ARTN_CHANNEL_FIXED 0
#define ARTN_CHANNEL_DIAGONAL 1
#define ARTN_CHANNEL_DENSE 2
#define ARTN_CHANNEL_OP_DIAGONAL 1 /* ArtnChannelOp.flags: every off-diagonal entry is exactly 0 */
#define ARTN_CHANNEL_OP_IDENTITY 2 /* ArtnChannelOp.flags: the matrix is exactly the identity    */
typedef struct ArtnChannelOp {
  uint64_t block_mask; /* as ArtnWgateTable's, of this operator */
  uint64_t flags;
} ArtnChannelOp;
typedef struct ArtnChannelTable {
  ArtnWgateTable gate;     /* k = t; block_mask: OR over the operators; flags: AND over the operators         */
  uint64_t m;              /* operators                                                                        */
  uint64_t form;           /* ARTN_CHANNEL_FIXED / _DIAGONAL / _DENSE                                         */
  uint64_t weight_doubles; /* float64 per operator in the weights: 1, D or 2 D^2                               */
  uint64_t reserved;
} ArtnChannelTable;
typedef struct ArtnChannelInfo {
  int32_t t, m, form;
  int32_t tile_bits;        /* TB, or log2 of the state when that is smaller                                   */
  int32_t launches[3];      /* per form: the launches of choose + apply (2); the DIAGONAL form adds those of   */
  int32_t reduction[3];     /* artn_marginal, the DENSE form those of artn_rdm -- reduction[form]: 0 none, 1 marginal, 2 rdm */
  int64_t n_tiles, segment, lds_bytes;
  int64_t weight_doubles;   /* float64 per operator the pack reads from `weights`                             */
  int64_t table_bytes;      /* 512 + m * (16 + 8 * weight_doubles + 16 * 4^t)                                  */
  int64_t record_bytes;     /* 32 + 16 * 4^t                                                                   */
  int64_t bytes_read;       /* nominal, of the pass over the state (none under the early return)              */
  int64_t bytes_written;
} ArtnChannelInfo;
/* Host-only: validates and plans.  mats may be NULL (no matrix is scanned then).  target_bits (t entries, the order listed) and
 * tile_bits (info->tile_bits entries, ascending; room for 12) may be NULL. */
int artn_channel_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t m, int32_t form, const double *mats,
                       ArtnChannelInfo *info, int32_t *target_bits, int32_t *tile_bits);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_channel_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t m, int32_t form, const double *mats,
                      const double *weights, void *table, int64_t table_bytes);
/* The draw: one launch of one workgroup on `stream`.  `table` is DEVICE memory holding what artn_channel_pack wrote for t, m and
 * form; `input` (DEVICE; may be NULL in the FIXED form) is q or rho as above; `uniform` is one float64 in [0, 1) in DEVICE memory. */
int artn_channel_choose(const void *table, int64_t table_bytes, int32_t t, int32_t m, int32_t form, const double *input,
                        const double *uniform, int32_t renormalize, void *record, int64_t record_bytes, void *stream);
/* The pass over `a`, in place: one launch on `stream`, reading the record artn_channel_choose wrote. */
int artn_channel_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *dims, int32_t m, const void *table,
                       int64_t table_bytes, const void *record, int64_t record_bytes, void *stream);

/*
 * BATCHED TRAJECTORIES: B states in ONE tensor, measured, reset and sent through noise channels with an outcome, a scale and an
 * operator PER STATE (additive to ABI 9: has("artn_channel_batch_apply")).  batch_dims[0 .. nb-1] (nb >= 0; NULL where nb == 0)
 * are distinct dimensions of any power-of-two extent, disjoint from the measured / target dimensions.  TRAJECTORY b is the
 * mixed-radix integer of their digits, the FIRST listed one the most significant; B is the product of their extents.  Whatever is
 * indexed by trajectory -- uniforms, forced outcomes, q, records -- is row b of a DEVICE array.  RECORDS are B times the 32 bytes
 * of artn_measure_choose's record (int64 outcome or j; float64 probability, total, scale), 8-byte aligned.
 *
 * LAYOUT RULE of the whole family: every memory bit of a batch dimension lies at or above a 128-byte line (bit 4 for complex64,
 * bit 3 for complex128), so neither a 16-byte vector nor a line spans two trajectories.  LIMITS: at most ARTN_BATCH_MAX_BITS batch
 * memory bits; B * D <= 2^24 (D = 2^k outcomes or 2^t rows: what the streaming artn_marginal keeps); k = 1 .. ARTN_MEASURE_MAX_DIMS
 * measured dimensions; t = 1..5 targets and a trajectory of at least 2^t elements.  nb == 0 is B = 1: the calls then give what
 * artn_measure_* / artn_channel_* give, bit for bit, and artn_channel_batch_pack writes the table of artn_channel_pack.
 *
 * PLAN.  Batch dimensions that are adjacent in memory and in order merge into FIELDS (shift, width, pos): b = OR over the fields
 * of ((index >> shift) & (2^width - 1)) << pos, at most ARTN_BATCH_MAX_FIELDS of them.
 *
 * MEASUREMENT.  dims[0 .. k-1] are the measured dimensions (extent 2, the first listed the most significant digit).
 * artn_measure_batch_choose: one lane per trajectory; record[b] is bit for bit what artn_measure_choose writes for q[b, :] (q:
 *   [B][D] float64, what artn_marginal writes for batch_dims then dims) and uniform[b], or, where `forced` is not NULL, for the
 *   forced outcome forced[b] (int64 [B]; `uniform` is not read then, and a forced[b] outside 0 .. D-1 gives outcome -1).
 * artn_measure_batch_collapse: the streaming pass of artn_measure_collapse (reset != 0: its move and clear pair); the trajectory
 *   of a 16-byte vector comes from the batch fields of its index, and outcome, scale and the scale == 1 shortcut from record[b].
 *   Slice b afterwards is bit for bit what artn_measure_collapse leaves on that slice with record[b]; a trajectory with outcome
 *   -1 is neither read nor written.
 *
 * CHANNELS.  Forms ARTN_CHANNEL_FIXED and ARTN_CHANNEL_DIAGONAL; ARTN_CHANNEL_DENSE needs a reduced density matrix per
 * trajectory, which does not exist, and is refused (ARTN_E_UNSUPPORTED).  The table is artn_channel_pack's with the tile fields
 * of its ArtnWgateTable taken from the batch plan: the TILE BITS are the t targets and the lowest other memory bits that are no
 * batch bits, tile_bits = min(TB, log2 n - batch bits) in all, so a tile lies in one trajectory; n_tiles << tile_bits = n; tile q
 * starts at q << log2(segment) with a 0 inserted at every tile bit at or above log2(segment), ascending (n_high counts them; only
 * the first ARTN_WGATE_MAX_K are listed in high_bit, the kernel takes them from its arguments).
 * artn_channel_batch_choose: one lane per trajectory; record[b] is bit for bit the 32-byte head of artn_channel_choose's record
 *   for input[b, :] (DIAGONAL: q [B][D]; FIXED: not read) and uniform[b].  No current matrix is written.
 * artn_channel_batch_apply: ONE launch of the tile kernel of artn_channel_apply.  Per tile it derives b from the tile's first
 *   element and reads record[b]; where j < 0, j >= m, or operator j is a flagged identity and scale == 1.0 it leaves the tile
 *   before its first access to the state; otherwise every coefficient is mats[j][e] * scale, one float64 multiply, under the
 *   table's OR block_mask (a coefficient that is exactly zero is left out term by term, so the bits are those of operator j's own
 *   mask).  Slice b afterwards is bit for bit what artn_wgate_apply gives for K_j * scale; skipped tiles keep every bit.
 * Everything runs on `stream` with the caller's buffers: no allocation, copy, synchronisation or atomics.
 *
 * ARTN_E_INVALID: a batch dimension out of range, repeated, or also measured / a target; a trajectory below 2^t elements; what
 * artn_measure_query / artn_channel_query call invalid.  ARTN_E_UNSUPPORTED: a batch bit below the line, more than
 * ARTN_BATCH_MAX_BITS batch bits, B * D above 2^24, the DENSE form, and the refusals of the unbatched queries.
 */
#define ARTN_BATCH_MAX_BITS 24
#define ARTN_BATCH_MAX_FIELDS 24
typedef struct ArtnBatchInfo {
  int32_t n_fields;       /* batch fields after merging                                                          */
  int32_t batch_bits;     /* log2 B                                                                              */
  int32_t tile_bits;      /* channels: min(TB, log2 n - batch_bits); measurement: 0                              */
  int32_t grid;           /* workgroups of the pass over the state                                               */
  int32_t launches;       /* choose + the pass (2); artn_marginal's come on top where q is needed                */
  int32_t reset_launches; /* measurement: choose + move + clear (3); channels: 0                                 */
  int64_t B, D, n;        /* trajectories; outcomes 2^k or rows 2^t; elements of the whole tensor                */
  int64_t n_tiles, segment, lds_bytes, table_bytes; /* channels (as ArtnChannelInfo's); measurement: 0           */
  int64_t record_bytes;   /* ARTN_MEASURE_RECORD_BYTES * B                                                       */
  int64_t bytes_read;     /* nominal: measurement the n / D kept elements, channels the whole tensor             */
  int64_t bytes_written;  /* nominal: the whole tensor                                                           */
  int32_t field_shift[ARTN_BATCH_MAX_FIELDS]; /* lowest memory bit of field f (the fields in the order listed)  */
  int32_t field_width[ARTN_BATCH_MAX_FIELDS];
  int32_t field_pos[ARTN_BATCH_MAX_FIELDS];   /* lowest bit of b that field f fills                             */
} ArtnBatchInfo;
/* Host-only: validates and plans. */
int artn_measure_batch_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, int32_t nb, const int32_t *batch_dims,
                             ArtnBatchInfo *info);
int artn_measure_batch_choose(const double *q, int64_t B, int64_t D, const double *uniform, const int64_t *forced, int32_t renormalize,
                              void *records, void *stream);
int artn_measure_batch_collapse(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, int32_t nb, const int32_t *batch_dims,
                                const void *records, int32_t reset, void *stream);
/* Host-only: validates and plans.  mats may be NULL; target_bits (t entries) and tile_bits (info->tile_bits entries, ascending;
 * room for 12) may be NULL. */
int artn_channel_batch_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t nb, const int32_t *batch_dims, int32_t m,
                             int32_t form, const double *mats, ArtnBatchInfo *info, int32_t *target_bits, int32_t *tile_bits);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_channel_batch_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t nb, const int32_t *batch_dims, int32_t m,
                            int32_t form, const double *mats, const double *weights, void *table, int64_t table_bytes);
int artn_channel_batch_choose(const void *table, int64_t table_bytes, int32_t t, int32_t m, int32_t form, const double *input,
                              const double *uniform, int64_t B, int32_t renormalize, void *records, void *stream);
int artn_channel_batch_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *dims, int32_t nb, const int32_t *batch_dims,
                             int32_t m, const void *table, int64_t table_bytes, const void *records, void *stream);

/*
 * CONDITIONAL GATES on batched trajectories: a controlled gate CHOSEN PER TRAJECTORY from a table of cases by an int64 in device
 * memory, in place, in one launch (additive to ABI 9: has("artn_cgate_batch_apply")).  targets, controls and control_values are
 * those of artn_cgate_query, batch_dims those of the batched trajectories above (disjoint from targets and controls, every batch
 * bit at or above a 128-byte line, at most ARTN_BATCH_MAX_BITS of them; nb == 0 is B = 1).  The m (1 .. ARTN_CGATE_BATCH_MAX_CASES)
 * CASES are keys[j], distinct integers in 0 .. 2^63 - 1, and mats[j], float64 [m][2 * 4^t], each the 2^t x 2^t matrix of
 * artn_wgate_query on the targets (any finite matrix).  mask is -1 (all bits) or lies in 0 .. 2^63 - 1, and every key lies inside it.
 *
 * SELECTOR.  B int64 words in DEVICE memory, word b at selector + 8 * b * selector_stride bytes (8-byte aligned, stride >= 1):
 * a contiguous int64 [B] has stride 1, the records of artn_measure_batch_choose / artn_channel_batch_choose stride 4.  The host
 * never reads it.
 *
 * CONTRACT.  For trajectory b, o = selector[b].  o < 0 (the -1 of a dead trajectory): untouched.  Otherwise key = o & mask and j
 * is the case with keys[j] == key; no such case: untouched; mats[j] exactly the identity (1.0 on the diagonal, zeros of either sign
 * elsewhere): untouched.  Otherwise slice b becomes bit for bit what artn_cgate_apply leaves on a dense copy of that slice for
 * mats[j], the targets, the controls and the control values.  UNTOUCHED: every bit is kept and no tile of the trajectory is read or
 * written -- non-finite data, NaN payloads and the sign of a zero included.  So nb == 0 with one case is artn_cgate_apply under
 * the condition (cond = selector, cond_mask = mask, cond_value = keys[0]) bit for bit, and one case without controls under a
 * selector that matches everywhere is artn_wgate_apply bit for bit.  Everything runs on `stream` with the caller's buffers: no
 * allocation, copy, synchronisation or atomics; results are bit-identical from run to run.
 *
 * PLAN.  That of artn_cgate_query on an index space without the batch bits: the TILE BITS are the t targets and the lowest memory
 * bits that are neither targets, high controls nor batch bits, tile_bits = min(TB, log2 n - c_high - batch_bits) in all, so a tile
 * lies in one trajectory and holds none of its high controls; n_tiles = 2^(log2 n - c_high - tile_bits).  The HOLES are the tile
 * bits at or above log2(segment) and the high controls; the batch bits are walked by the tile number like any other free bit.
 * Per tile the kernel derives b from the tile's first element by the batch FIELDS, loads selector[b], and leaves the tile before
 * its first access to the state where the trajectory is untouched.  A low control lies below a line and a batch bit at or above
 * it, so the group mask of artn_cgate_apply is unchanged.
 *
 * TABLE (8-byte little-endian fields): ArtnCgateTable (flags and block_mask: the AND of the "diagonal" flags, the OR of the masks),
 * ArtnCgateBatchCases, then the m matrices as float64 (Re, Im), row-major.  table_bytes = 1000 + 400 + m * 16 * 4^t.
 *
 * ARTN_E_INVALID: what artn_cgate_query calls invalid; a batch dimension out of range, repeated, or also a target or a control; m
 * outside 1 .. 16; a key below 0, repeated, or outside the mask; a mask below -1; a matrix entry that is not finite; t + c above
 * the index bits of a trajectory (a trajectory below 2^t elements once the controls are taken out); a selector stride below 1.
 * ARTN_E_UNSUPPORTED: what artn_cgate_query does not support; a batch bit below the line; more than ARTN_BATCH_MAX_BITS batch bits;
 * a selector that is not 8-byte aligned.
 */
#define ARTN_CGATE_BATCH_MAX_CASES 16
#define ARTN_CGATE_CASE_DIAGONAL 1 /* ArtnCgateBatchCases.flags: every off-diagonal entry is exactly 0 */
#define ARTN_CGATE_CASE_IDENTITY 2 /* ... the matrix is exactly the identity                           */
typedef struct ArtnCgateBatchCases {
  uint64_t m;
  uint64_t reserved;
  int64_t key[ARTN_CGATE_BATCH_MAX_CASES];         /* entries at and above m: -1, which no masked selector equals */
  uint64_t flags[ARTN_CGATE_BATCH_MAX_CASES];
  uint64_t block_mask[ARTN_CGATE_BATCH_MAX_CASES]; /* as ArtnWgateTable's, per case                               */
} ArtnCgateBatchCases;
typedef struct ArtnCgateBatchInfo {
  int32_t t, c;
  int32_t c_high, c_low;
  int32_t tile_bits;     /* min(TB, log2 n - c_high - batch_bits)                         */
  int32_t diagonal;      /* 1: every off-diagonal entry of every case is exactly 0        */
  int64_t n_selected;    /* n >> c: the elements whose control digits match               */
  int64_t n_tiles;       /* n_tiles << tile_bits = n >> c_high                            */
  int64_t segment;       /* elements of a contiguous segment of a tile                    */
  int64_t lds_bytes;
  int64_t table_bytes;
  int64_t bytes_read;    /* nominal: (n >> c_high) elements, every trajectory touched     */
  int64_t bytes_written;
  int32_t m;             /* cases                                                         */
  int32_t batch_bits;    /* log2 B                                                        */
  int32_t n_fields;      /* batch fields after merging                                    */
  int32_t grid;          /* workgroups of the launch                                      */
  int64_t B;             /* trajectories                                                  */
  int32_t field_shift[ARTN_BATCH_MAX_FIELDS]; /* as ArtnBatchInfo's */
  int32_t field_width[ARTN_BATCH_MAX_FIELDS];
  int32_t field_pos[ARTN_BATCH_MAX_FIELDS];
} ArtnCgateBatchInfo;
/* Host-only: validates and plans.  keys and mats may be NULL (not checked then); selector may be NULL (its alignment is not
 * checked then; selector_stride always is); target_bits (t entries), control_bits (c entries) and tile_bits (info->tile_bits
 * entries, ascending; room for 12) may be NULL. */
int artn_cgate_batch_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                           const int32_t *control_values, int32_t nb, const int32_t *batch_dims, int32_t m, const int64_t *keys,
                           int64_t mask, const double *mats, const void *selector, int64_t selector_stride, ArtnCgateBatchInfo *info,
                           int32_t *target_bits, int32_t *control_bits, int32_t *tile_bits);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_cgate_batch_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                          const int32_t *control_values, int32_t nb, const int32_t *batch_dims, int32_t m, const int64_t *keys,
                          int64_t mask, const double *mats, void *table, int64_t table_bytes);
/* The chosen gates on `a`, in place: ONE launch on `stream`.  `table` is DEVICE memory holding what artn_cgate_batch_pack wrote
 * for the same descriptor, targets, controls, control values, batch dimensions and m.  ARTN_E_NODEVICE without a device. */
int artn_cgate_batch_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                           const int32_t *control_values, int32_t nb, const int32_t *batch_dims, int32_t m, const void *table,
                           int64_t table_bytes, const void *selector, int64_t selector_stride, int64_t mask, void *stream);

/*
 * PAULI EXPECTATION VALUES PER TRAJECTORY: <psi_b|P|psi_b> of every state b of a batched tensor, one pass over the whole tensor
 * for up to terms_per_launch strings of equal xmask (additive to ABI 9: has("artn_pauli_batch_expect")).  Descriptor, `ops`,
 * global masks, groups and layout refusals are those of artn_pauli_query in the wording "batched Pauli expectations take ...";
 * batch_dims are those of the batched trajectories above (every batch bit at or above a 128-byte line, at most
 * ARTN_BATCH_MAX_BITS of them).  Strings carry I on every batch dimension.  The kernels only read the state.
 *
 * FORMULA.  The tensor has n = 2^L elements and a trajectory M = L - batch_bits LOCAL bits: local bit j is the j-th lowest memory
 * bit that is no batch bit.  The LOCAL MASKS xl, zl are xmask, zmask compressed onto the local bits.  With a_b[l] the element of
 * trajectory b at local index l,
 *     out[b][t] = sum_l conj(a_b[l ^ xl]) * i^n_y * (-1)^popcount(l & zl) * a_b[l]      (real),   out[b][n_terms] = sum_l |a_b[l]|^2
 * in the caller's term order.  Forms, signs and the summation order are functions of M, xl and zl alone: row b does not depend on
 * where the batch bits lie in memory.
 *
 * PLAN.  M >= 10: a local tile is 2^10 consecutive local indices, T = 2^(M-10) of them per trajectory, T / 2 where xl >= 2^10 (the
 * tiles whose highest xl bit is 0, weight 2).  A UNIT is (b, c), 0 <= c < C, C = min(T, max(1, 2048 >> batch_bits)) (`chunks`, and
 * `chunks_halved` from T / 2): chunk c takes the local tiles c, c + C, ... in ascending order, thread t of the workgroup the local
 * elements 4t .. 4t+3 of each, one fixed tree over the workgroup ends the unit, and a second launch adds the C partials of every
 * (b, term) in ascending c and writes out.  M < 10: a workgroup takes 2^(10-M) whole trajectories, 2^(M-2) threads each, and the
 * tree stops below the trajectory; C = 1.  Terms are those of artn_pauli_expect (float64 first, one rounding per Re q and Im q).
 * No floating-point atomics: bit-identical from run to run.
 *
 * EXACTNESS.  nb == 0 is B = 1 and gives artn_pauli_expect's out bit for bit.  For B > 1, row b is bit for bit what
 * artn_pauli_expect gives on a dense copy of trajectory b with its dimensions in local-bit order whenever M >= 10 and
 * B * T <= 2048 (then C = T: every unit is one tile, as every workgroup of the unbatched pass); elsewhere the two differ by the
 * summation order alone.  The norm comes from the call's first pass, as there.
 *
 * LIMITS.  B * (n_terms + 1) <= 2^28 (2 GiB of output).  workspace_bytes = B * chunks * 17 * 8.  Everything runs on `stream` with the
 * caller's buffers: no allocation, copy or synchronisation.
 *
 * ARTN_E_INVALID: what artn_pauli_query calls invalid; X, Y or Z on a batch dimension; a batch dimension out of range or
 * repeated; nb < 0; a workspace smaller than the query reports.  ARTN_E_UNSUPPORTED: a batch bit below the line; more than
 * ARTN_BATCH_MAX_BITS batch bits; B * (n_terms + 1) above 2^28; `a` not 16-byte aligned, `out` or `ws` not 8-byte aligned; the
 * refusals of artn_pauli_query.  ARTN_E_NODEVICE (artn_pauli_batch_expect, once every argument has passed): no device.
 */
typedef struct ArtnPauliBatchInfo {
  int32_t n_groups;         /* distinct xmasks                                                       */
  int32_t n_launches;       /* passes over the tensor; each is followed by one finish launch         */
  int32_t terms_per_launch; /* strings one pass serves                                               */
  int32_t batch_bits;       /* log2 B                                                                */
  int32_t local_bits;       /* M                                                                     */
  int32_t tile_bits;        /* min(10, M)                                                            */
  int32_t n_fields;         /* batch fields after merging                                            */
  int32_t grid;             /* workgroups of a pass with xl < 2^10                                   */
  int64_t chunks;           /* C where xl < 2^10                                                     */
  int64_t chunks_halved;    /* C where xl >= 2^10                                                    */
  int64_t B, n;             /* trajectories; elements of the whole tensor                            */
  int64_t workspace_bytes;
  int64_t out_bytes;        /* B * (n_terms + 1) * 8                                                 */
  int64_t bytes_read;       /* n_launches * bytes of the tensor                                      */
  int32_t field_shift[ARTN_BATCH_MAX_FIELDS]; /* as ArtnBatchInfo's */
  int32_t field_width[ARTN_BATCH_MAX_FIELDS];
  int32_t field_pos[ARTN_BATCH_MAX_FIELDS];
} ArtnPauliBatchInfo;
/* Host-only: validates, translates every term to global and local masks, groups by xmask, splits the work, sizes the workspace.
 * xmask, zmask, n_y, group, local_xmask, local_zmask: n_terms entries each, any of them may be NULL. */
int artn_pauli_batch_query(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, int32_t nb, const int32_t *batch_dims,
                           ArtnPauliBatchInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *group,
                           uint64_t *local_xmask, uint64_t *local_zmask);
/* out (device, float64 [B][n_terms + 1]): row b holds the raw sums of trajectory b in the caller's term order, then its
 * sum |a|^2.  ws: device, at least workspace_bytes. */
int artn_pauli_batch_expect(const ArtnMarginalDesc *d, const void *a, const uint8_t *ops, int64_t n_terms, int32_t nb,
                            const int32_t *batch_dims, double *out, void *ws, int64_t ws_bytes, void *stream);

/*
 * BITSTRING SAMPLING PER TRAJECTORY: S draws from every state b of a batched tensor, B cumulative distributions in one tensor
 * (additive to ABI 9: has("artn_sample_batch")).  It generalises artn_born_block_sums + artn_born_pick above, which draw from
 * ONE array, to the trajectories of BATCHED TRAJECTORIES: the descriptor and the layout refusals are those of the families
 * that index the state by bits, in the wording "batched sampling takes ..."; batch_dims are those of the batched trajectories
 * (every batch bit at or above a 128-byte line, at most ARTN_BATCH_MAX_BITS of them; nb == 0 is B = 1).  The state is only read.
 *
 * CONTRACT.  The tensor has n = 2^L elements and a trajectory M = L - batch_bits LOCAL bits: local bit j is the j-th lowest
 * memory bit that is no batch bit (as for artn_pauli_batch_expect).  The cumulative distribution of trajectory b runs over its
 * 2^M elements IN LOCAL-INDEX ORDER, with exactly the arithmetic of the unbatched entries on an array of 2^M elements: terms
 * |a|^2 formed in float64 with one rounding, 4-element segment sums ((t0 + t1) + t2) + t3, the in-block prefix of
 * artn_born_block_sums, blocks of artn_born_plan(2^M).block_bits bits, the prefix over the nb_t = blocks_per_trajectory block
 * sums that artn_born_block_sums forms for n_blocks = nb_t (a function of nb_t alone; for nb_t <= 1024 the plain ascending
 * running sum).  norm_b is the last prefix entry.  The target of (b, s) is the single multiply uniforms[b][s] * norm_b, and
 * the pick is artn_born_pick's: the smallest local index whose running sum exceeds the target, never an element with
 * |a|^2 == 0, a target at or beyond norm_b the last non-zero element.  A uniform outside [0, 1) is not refused: one at or
 * above 1 takes the last non-zero element, a negative one yields index -1 and probability 0.
 *   Hence row b of the outputs is, bit for bit, what artn_born_block_sums + artn_born_pick give on a dense copy of trajectory b
 * with its dimensions in local-bit order and targets = uniforms[b] * norm_b -- its index deposited into the memory bits that
 * are no batch bits, OR'd with b deposited into the fields; nb == 0 gives those entries' results themselves.  A row depends
 * neither on where the batch bits lie nor on the other rows.  No floating-point atomics: bit-identical from run to run.
 *
 * FORMS.  ARTN_SAMPLE_BATCH_TILED (M >= 10, or B == 1), three launches: block sums, a unit being (b, block j), workgroups
 * looping over units above 2^20 of them; the prefix per trajectory, which also writes out_norm (one 1024-thread workgroup per
 * trajectory where nb_t > 1024, else 1024 / nb_t rows per workgroup); the pick, a unit being (b, j) again: it bisects row b of
 * the uniforms, on the products, for the targets of its block and leaves before touching the amplitudes when it has none.
 * ARTN_SAMPLE_BATCH_SMALL (M < 10 and B > 1), ONE launch: a workgroup takes 2^(10-M) whole trajectories, 2^(M-2) threads
 * each.  The uniforms are sorted, not the targets (multiplying by a positive norm is monotone), so the entry needs nothing
 * that depends on the state.
 *
 * LIMITS.  n <= 2^40; B * n_samples <= 2^28; `a` 16-byte aligned, everything else 8-byte aligned.  workspace_bytes =
 * B * nb_t * 2 * 8 (block sums, then prefix; 0 for SMALL).  Everything runs on `stream` with the caller's buffers: no
 * allocation, copy or synchronisation.  n_samples == 0 succeeds without a launch (out_norm is not written).
 *
 * ARTN_E_INVALID: a malformed descriptor or a tensor that is not dense; a batch dimension out of range or repeated; nb < 0;
 * n_samples < 0; a null pointer; a workspace smaller than the query reports.  ARTN_E_UNSUPPORTED: a dtype other than
 * complex64 / complex128; an extent that is no power of two; more than 2^40 elements; a batch bit below the line; more than
 * ARTN_BATCH_MAX_BITS batch bits; B * n_samples above 2^28; a misaligned pointer.  ARTN_E_NODEVICE (artn_sample_batch, once
 * every argument has passed): no device.
 */
#define ARTN_SAMPLE_BATCH_SMALL 0
#define ARTN_SAMPLE_BATCH_TILED 1
typedef struct ArtnSampleBatchInfo {
  int32_t form;                  /* ARTN_SAMPLE_BATCH_*                                                   */
  int32_t launches;              /* 1 (SMALL) or 3 (TILED); two memsets preset the outputs on top         */
  int32_t batch_bits;            /* log2 B                                                                */
  int32_t local_bits;            /* M                                                                     */
  int32_t block_bits;            /* artn_born_plan(2^M).block_bits                                        */
  int32_t n_fields;              /* batch fields after merging                                            */
  int32_t grid[3];               /* workgroups of the launches (TILED: block sums, prefix, pick)          */
  int32_t reserved;
  int64_t B, n;                  /* trajectories; elements of the whole tensor                            */
  int64_t blocks_per_trajectory; /* nb_t = artn_born_plan(2^M).n_blocks                                   */
  int64_t workspace_bytes;
  int64_t bytes_read_min;        /* one reading of the tensor (the pick re-reads the blocks with targets) */
  int32_t field_shift[ARTN_BATCH_MAX_FIELDS]; /* as ArtnBatchInfo's */
  int32_t field_width[ARTN_BATCH_MAX_FIELDS];
  int32_t field_pos[ARTN_BATCH_MAX_FIELDS];
} ArtnSampleBatchInfo;
/* Host-only: validates, splits the work, sizes the workspace. */
int artn_sample_batch_query(const ArtnMarginalDesc *d, int32_t nb, const int32_t *batch_dims, int64_t n_samples,
                            ArtnSampleBatchInfo *info);
/* uniforms_sorted (device, float64 [B][n_samples], ASCENDING per row).  out_index (device, int64 [B][n_samples]): the MEMORY
 * index of the drawn element, -1 where nothing can be drawn; out_prob: its raw |a|^2; out_norm (device, float64 [B]): norm_b.
 * ws: device, at least workspace_bytes (may be NULL when that is 0). */
int artn_sample_batch(const ArtnMarginalDesc *d, const void *a, int32_t nb, const int32_t *batch_dims, const double *uniforms_sorted,
                      int64_t n_samples, int64_t *out_index, double *out_prob, double *out_norm, void *ws, int64_t ws_bytes,
                      void *stream);

/*
 * DIAGONAL OPERATORS: a classical cost function f(i) = sum_k c_k (-1)^popcount(i & zmask_k) applied as ONE object, one streaming
 * pass per operation whatever the number of terms (additive to ABI 9: has("artn_diag_apply")).  Descriptor, `ops` (uint8
 * [n_terms][n_dims], I and Z only: codes 0 and 3), masks and layout refusals are those of artn_pauli_query in the wording
 * "diagonal operators take ..."; `coeff` is float64 [n_terms] (real).  Repeated strings are allowed and are not merged.
 *
 * PLAN.  The tile is TB = min(10, log2 n) low memory bits; lo_k = zmask_k & (2^TB - 1), hi_k = zmask_k >> TB.  A term with
 * hi_k == 0 is STATIC; the others are DYNAMIC and form GROUPS of equal lo_k, numbered in the order they first appear (a group
 * with lo == 0 is a per-tile constant).  More than ARTN_DIAG_MAX_GROUPS groups: ARTN_E_UNSUPPORTED.
 *
 * VALUE CONTRACT (float64; every c * (+-1) is exact, so these are plain sequential additions, never fused):
 *     S[l]    = ((0.0 + s_1) + s_2) + ...   over the static terms in the caller's order, s_k = +-c_k by popcount(l & lo_k)
 *     w_g(h)  = ((0.0 + s_1) + s_2) + ...   over the terms of group g in the caller's order, s_k = +-c_k by popcount(h & hi_k)
 *     f(h, l) = ((S[l] + sigma_0 w_0(h)) + sigma_1 w_1(h)) + ...   over the groups in order, sigma_g = +-1 by popcount(l & lo_g)
 * for the element at memory index (h << TB) | l.  S is computed by artn_diag_pack on the host; every tile computes its w_g(h) on
 * the device.  f depends on the memory index and the term list alone -- not on the dtype, the grid or the workgroup.
 *
 * OPERATIONS (one launch each on `stream`, plus a one-workgroup finish launch where a sum is returned; 256 threads, the grid
 * min(tiles, 2048) striding over tiles; no atomics, sums in float64 in a fixed order: bit-identical from run to run):
 *   artn_diag_values   out[i] = f(i), float64, n entries in memory order (DEVICE).
 *   artn_diag_expect   out[0..2] = sum p, sum p f, sum (p f) f with p = fma(ar, ar, ai * ai) in float64 (as artn_born_overlap),
 *                      accumulated as fma(p, f, acc) and fma(p f, f, acc).
 *   artn_diag_apply    ARTN_DIAG_PHASE:    a[i] <- a[i] * exp(-i gamma f(i)): phi = gamma * f (one rounding), float64 sincos,
 *                                          Re = fma(ar, c, ai * s), Im = fma(ai, c, -(ar * s)), rounded once to the dtype.
 *                                          gamma == 0 returns without a launch.
 *                      ARTN_DIAG_MULTIPLY: a[i] <- a[i] * f(i): one float64 product per component, rounded once (gamma unused).
 *   artn_diag_pair     lam and phi of one descriptor, byte ranges disjoint.  out[0..1] = Re, Im of sum_i conj(lam_i) f(i) phi_i
 *                      from the values BEFORE the phase: u = conj(lam_i) phi_i (Re = fma(lr, pr, li * pi), Im = fma(lr, pi,
 *                      -(li * pr))), acc = fma(u, f, acc).  ARTN_DIAG_PAIR_EVOLVE: both states take ARTN_DIAG_PHASE in the same
 *                      pass (gamma == 0: nothing is written) and are afterwards bit for bit what artn_diag_apply leaves on each
 *                      alone; ARTN_DIAG_PAIR_TRANSITION: nothing is written.
 * `ops` and n_terms are those of the pack call (the plan is rebuilt from them; the coefficients are in the table).  The calls take
 * the caller's table (DEVICE, 8-byte aligned) and workspace (DEVICE, 8-byte aligned, workspace_bytes of the query) and do no
 * allocation, copy or synchronisation.
 *
 * TABLE (what artn_diag_pack writes and the kernels read; 8-byte little-endian fields): ArtnDiagTable (64 bytes), S as 2^TB
 * float64, n_groups ArtnDiagGroup (32 bytes each, in group order), then n_dynamic ArtnDiagTerm (16 bytes each, group by group,
 * the caller's order inside a group).  table_bytes = 64 + 8 * 2^TB + 32 * n_groups + 16 * n_dynamic.
 *
 * ARTN_E_INVALID: a layout that is not dense, an operator code above 3, X or Y in a term, Z on an extent other than 2, n_terms < 1,
 * a coefficient or gamma that is not finite, an unknown mode, a null pointer, a table or workspace smaller
 * than the query's, byte ranges of lam and phi that overlap.  ARTN_E_UNSUPPORTED: another dtype, an extent that is no power of two,
 * more than 96 dimensions or 2^40 elements, more than ARTN_DIAG_MAX_GROUPS groups or ARTN_DIAG_MAX_TERMS terms, a state that is not 16-byte aligned, a table,
 * workspace or output that is not 8-byte aligned.  ARTN_E_NODEVICE without a device (query and pack are host-only).
 */
#define ARTN_DIAG_MAX_GROUPS 64
#define ARTN_DIAG_MAX_TERMS 65536
#define ARTN_DIAG_TILE_BITS 10
#define ARTN_DIAG_PHASE 0
#define ARTN_DIAG_MULTIPLY 1
#define ARTN_DIAG_PAIR_EVOLVE 0
#define ARTN_DIAG_PAIR_TRANSITION 1
#define ARTN_DIAG_OP_VALUES 0 /* the indices of ArtnDiagInfo.bytes_read / bytes_written */
#define ARTN_DIAG_OP_EXPECT 1
#define ARTN_DIAG_OP_PHASE 2
#define ARTN_DIAG_OP_MULTIPLY 3
#define ARTN_DIAG_OP_PAIR 4
typedef struct ArtnDiagTable {
  uint64_t n_terms, n_static, n_dynamic, n_groups, tile_bits, n_tiles, reserved[2];
} ArtnDiagTable;
typedef struct ArtnDiagGroup {
  uint64_t lo, first, count, reserved; /* the group's terms are the term records first .. first + count - 1 */
} ArtnDiagGroup;
typedef struct ArtnDiagTerm {
  uint64_t hi;
  double c;
} ArtnDiagTerm;
typedef struct ArtnDiagInfo {
  int32_t n_terms, n_static, n_dynamic, n_groups;
  int32_t tile_bits; /* TB */
  int32_t reserved;
  int64_t n_tiles;
  int64_t table_bytes;
  int64_t workspace_bytes;  /* artn_diag_expect and artn_diag_pair: 32 bytes per workgroup of the pass */
  int64_t bytes_read[5];    /* per operation (ARTN_DIAG_OP_*), of the state and the values buffer; nominal */
  int64_t bytes_written[5]; /* (ARTN_DIAG_OP_PAIR: the evolving mode; its transition-only mode writes nothing) */
} ArtnDiagInfo;
/* Host-only: validates, translates and groups.  Per term (n_terms entries each, any may be NULL): zmask, lo, hi and group (-1:
 * static).  Per group (room for ARTN_DIAG_MAX_GROUPS; may be NULL): group_lo. */
int artn_diag_query(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, ArtnDiagInfo *info, uint64_t *zmask,
                    uint64_t *lo, uint64_t *hi, int32_t *group, uint64_t *group_lo);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_diag_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_terms, void *table,
                   int64_t table_bytes);
int artn_diag_values(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, const void *table, int64_t table_bytes,
                     double *out, void *stream);
int artn_diag_expect(const ArtnMarginalDesc *d, const void *a, const uint8_t *ops, int64_t n_terms, const void *table,
                     int64_t table_bytes, void *ws, int64_t ws_bytes, double *out3, void *stream);
int artn_diag_apply(const ArtnMarginalDesc *d, void *a, const uint8_t *ops, int64_t n_terms, const void *table,
                    int64_t table_bytes, int32_t mode, double gamma, void *stream);
int artn_diag_pair(const ArtnMarginalDesc *d, void *lam, void *phi, const uint8_t *ops, int64_t n_terms, const void *table,
                   int64_t table_bytes, int32_t mode, double gamma, void *ws, int64_t ws_bytes, double *out2, void *stream);

/*
 * IN-PLACE PERMUTATIONS OF THE INDEX BITS of a dense state: relayout, qubit remapping, SWAP networks and qubit reversal as pure
 * data movement (additive to ABI 9: has("artn_bitperm_apply")).  The descriptor is a dense layout of n = 2^nb elements under the
 * rules of the other bit-indexed families (power-of-two extents, at most 2^40 elements, a 16-byte aligned array); only n and the
 * dtype matter: the permutation is given on MEMORY bits.  n_bits must equal nb.
 *
 * CONTRACT.  dst_bit[0 .. nb-1] is a permutation of 0 .. nb-1; pi(i) is the index whose bit dst_bit[b] equals bit b of i, for
 * every b.  After the call new[pi(i)] == old[i] BIT FOR BIT for every i -- the sign of a zero, NaN payloads, denormals,
 * infinities: no arithmetic and no conversion touches an element.  No second buffer.  The identity issues no launch.  No atomics.
 *
 * PLAN.  LB = 4 (complex64) or 3 (complex128) index bits of a 128-byte line; TB = ARTN_WGATE_TILE_BITS_C64 / _C128.  The host
 * cuts the permutation into PASSES, one launch each, in order on the stream.  A pass permutes a set M of memory bits among
 * themselves (pass_map); its TILE BITS are M, every bit below LB and the lowest other bits, min(TB, nb) in all, tile-local bit j
 * the j-th of them ascending; so a pass moves any low bits and at most TB - LB = 8 bits at or above LB (any bits when nb <= TB).
 * Passes come from the cycles of what is left of the permutation: a cycle that fits into the free places of the pass is taken
 * whole (all its bits reach their final place), then at most one longer cycle gives an ARC of consecutive bits, starting at a
 * low bit where the cycle has one, which puts all its bits but the first in their final place.  With h moved bits at or above
 * LB: one pass when h <= 8, at most max(1, ceil((h - 1) / 7)) in general, none for the identity.  The launch of a pass walks
 * its n >> tile_bits tiles by the hole insertion of artn_cgate_apply (segment_bits, hole_bit), in 64-bit arithmetic.
 * LDS.  Tile-local index u is kept at LDS index L(u), the XOR of load_col[j] over the set bits j of u, L invertible; the store
 * phase reads L(tau^-1 w) for tile-local w through store_col[j] = load_col[tau^-1 j], tau the pass's map on tile-local bits.
 * load_degree / store_degree are the bank-conflict degrees of the two phases, 2^(dim V - rank): V the lane bits of one LDS
 * service group of the instruction (complex64: 16 lanes of a 64-bit write = tile-local bits 1..4, 32 lanes of a 64-bit read =
 * bits 1..5; complex128: 8 lanes of a 128-bit write = bits 0..2, the 16 lanes {0-3, 12-15, 20-27} of a 128-bit read = the span of
 * bits 0, 1, 2 xor 3, 2 xor 4), rank that of their LDS indices modulo the banks' period in elements (16 / 32; 8 / 16).  The host searches
 * L for load degree 1 and the least store degree.
 *
 * TABLE (what artn_bitperm_pack writes and the kernel reads; 8-byte little-endian fields): ArtnBitpermTable, 64 bytes, then
 * passes x ArtnBitpermPass, 576 bytes each.
 *
 * ARTN_E_UNSUPPORTED: the layout and dtype refusals of the bit-indexed families, a table that is not 8-byte aligned, an array
 * that is not 16-byte aligned.  ARTN_E_INVALID: n_bits other than log2 n, dst_bit not a permutation, a null pointer, a table
 * smaller than the query's.
 */
#define ARTN_BITPERM_MAX_BITS 40
#define ARTN_BITPERM_MAX_PASSES 8
typedef struct ArtnBitpermPass {
  uint64_t tile_bits, n_tiles, segment_bits, n_holes;
  uint64_t moved_mask; /* OR of 1 << b over the memory bits the pass moves                                   */
  uint64_t reserved[3];
  uint64_t mem_col[16];   /* per tile-local bit j: 1 << its memory bit (0 beyond tile_bits)                   */
  uint64_t load_col[16];  /* per tile-local bit j: what it contributes (XOR) to the LDS index, load phase     */
  uint64_t store_col[16]; /* the same for the store phase: load_col[tau^-1 j]                                 */
  uint64_t hole_bit[16];  /* ascending: the tile bits at or above segment_bits                                */
} ArtnBitpermPass;
typedef struct ArtnBitpermTable {
  uint64_t n_passes, n_bits, reserved[6];
} ArtnBitpermTable;
typedef struct ArtnBitpermInfo {
  int32_t n_bits, passes;
  int32_t line_bits;  /* LB                                                            */
  int32_t moved;      /* bits with dst_bit[b] != b                                     */
  int32_t moved_high; /* h: those at or above LB                                       */
  int32_t reserved;
  int64_t table_bytes;
  int64_t lds_bytes;   /* of the largest pass                                           */
  int64_t bytes_moved; /* nominal: 2 x the state x passes                               */
  int32_t tile_bits[ARTN_BITPERM_MAX_PASSES];
  int32_t grid[ARTN_BITPERM_MAX_PASSES];
  int32_t load_degree[ARTN_BITPERM_MAX_PASSES];
  int32_t store_degree[ARTN_BITPERM_MAX_PASSES];
  int64_t n_tiles[ARTN_BITPERM_MAX_PASSES];
  uint64_t moved_mask[ARTN_BITPERM_MAX_PASSES];
} ArtnBitpermInfo;
/* Host-only: validates and plans.  Per pass p (room for ARTN_BITPERM_MAX_PASSES; any may be NULL): pass_map[p * 40 + b], the
 * memory bit that bit b goes to in pass p (b itself outside moved_mask), b < n_bits; tiles[p * 16 + j], the memory bit of
 * tile-local bit j (-1 beyond tile_bits); load_col / store_col [p * 16 + j]. */
int artn_bitperm_query(const ArtnMarginalDesc *d, const int32_t *dst_bit, int32_t n_bits, ArtnBitpermInfo *info, int32_t *pass_map,
                       int32_t *tiles, uint64_t *load_col, uint64_t *store_col);
/* Host-only: writes the table into HOST memory (8-byte aligned, at least table_bytes of the query). */
int artn_bitperm_pack(const ArtnMarginalDesc *d, const int32_t *dst_bit, int32_t n_bits, void *table, int64_t table_bytes);
/* The permutation on `a`, in place: `passes` launches on `stream`, in order.  `table` is DEVICE memory holding what
 * artn_bitperm_pack wrote for the same descriptor and dst_bit.  No allocation, copy or synchronisation.  ARTN_E_NODEVICE
 * without a device. */
int artn_bitperm_apply(const ArtnMarginalDesc *d, void *a, const int32_t *dst_bit, int32_t n_bits, const void *table,
                       int64_t table_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ARTN_H */
