/*
 * fadernets.h - C ABI of libfadernets_hip.so: the MI355X (gfx950) kernels behind the
 * MusicAttrRegGMVAE training / inference path of Music FaderNets.
 *
 * The reference has no FFI: the path is PyTorch module code (gmm_model.py:10-259) driven by
 * trainer_gmm.py:109-303.  Each entry point below replaces the torch operator(s) the reference
 * executes at the cited lines; the Python class in music-fader-nets_amd/gmm_model.py keeps the
 * reference's class surface and calls these through ctypes.
 *
 * Conventions
 *   - every function returns int: 0 = OK, <0 = FN_E_* argument error, >0 = hipError_t;
 *   - all pointers are DEVICE pointers (fp32 unless stated, int32 for token ids), owned by the
 *     caller; nothing is allocated, freed or synchronised inside (graph-capture safe);
 *   - `stream` is a hipStream_t passed as void*; work is stream-ordered;
 *   - functions are re-entrant and thread-safe; the only process-wide state is a handful of write-once caches of immutable facts
 *     (compute-unit count and kernel attributes per device, the run-time binding of librccl), held in atomics / behind
 *     std::call_once; no environment variable is read;
 *   - per-step tensors are TIME-MAJOR: [T][B][...] so that one step is one contiguous slab;
 *     token tensors are batch-major [B][T] int32 exactly as the data loader yields them.
 */
#ifndef FADERNETS_H
#define FADERNETS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FN_OK 0
#define FN_E_NULL (-1)      /* required pointer is NULL                     */
#define FN_E_SHAPE (-2)     /* unsupported / inconsistent sizes             */
#define FN_E_ALIGN (-3)     /* pointer or leading dimension not aligned     */
#define FN_E_WORKSPACE (-4) /* workspace too small                          */
#define FN_E_COUNT (-5)     /* too many scans in one call                   */
#define FN_E_UNSUPPORTED (-6) /* valid arguments, but this single-launch path is not eligible on this device / shape: */
                            /* nothing was enqueued, the caller takes the general path                             */
#define FN_E_COMM (-7)      /* fn_comm_*: librccl could not be loaded / lacks a symbol                             */
#define FN_COMM_ERROR_BASE 2000000  /* fn_comm_*: FN_COMM_ERROR_BASE + ncclResult_t                                 */

#define FN_MAX_SCANS 8

int fn_version(void);                 /* ABI version, currently 6 (round 5: fn_gru_fwd_x6_ok, fn_gru_bwd_x6_ok, fn_comm_count / fn_comm_rank, fn_weight_images kinds 3 / 4, FnGruBwd.variant bit 14;
                                         round 6: FN_GEMM_X6_PERWAVE / _WIDE / _PERTILE, FN_GEMM_BF16X6 on the Linear-forward form, FnGruCell.variant bit 14, fn_weight_images kind 5) */
const char* fn_strerror(int code);    /* static string for FN_E_* / hipError_t */

/* ------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the f32 MFMA (v_mfma_f32_16x16x4_f32), exact-f32 fma chains.
 *   C[M,N] = alpha * opA(A) * opB(B) + beta * C + bias[N]
 *   a_kmajor=1: A is [M,K] row-major (lda)      a_kmajor=0: A is stored [K,M] row-major (lda)
 *   b_kmajor=1: B is [N,K] row-major (ldb) i.e. a torch Linear weight; 0: B is [K,N] row-major
 * Replaces nn.Linear forward (gmm_model.py:86,91,108,113,123,137: a_k=1,b_k=1), its input
 * gradient (a_k=1,b_k=0) and its weight gradient dW = dY^T X (a_k=0,b_k=0).
 * splitk>1 needs ws of fn_gemm_ws_bytes(M,N,splitk) bytes (deterministic slab reduction).
 * splitk | FN_GEMM_LEAN (weight-gradient form a_k=0,b_k=0 and fn_gru_dwhh_f32): the instance whose
 * wavefronts need <= 128 vector registers, so that one of them fits on a SIMD BESIDE a wavefront of a weight-stationary scan
 * (fn_gru_seq_*: 336-376 registers of 512) and the product fills the scan's idle MFMA cycles instead of waiting for its CUs.
 * Same results bit for bit (same k order).
 * The Linear-forward form (a_k=1,b_k=1) with whole 128 x 128 tiles (>= 256 of them), K % 16 == 0, 16-byte aligned operands and no
 * split runs as an LDS-free kernel (MFMA operands straight from memory; k summed in a fixed order that differs from the staged
 * kernel's inside every 16-k step); there FN_GEMM_LEAN selects its <= 128-register instance (four workgroups per CU; fits beside a
 * wavefront of the decoder pipeline's forward scans) - same results as the full instance.
 * ------------------------------------------------------------------------------------------ */
#define FN_GEMM_LEAN 0x10000
/* splitk | FN_GEMM_BF16X6 (weight-gradient form a_k=0,b_k=0 and fn_gru_dwhh_f32): the products run on the bf16 MFMA with every fp32
 * operand value cut EXACTLY into three bf16 pieces (x = hi + mid + lo) and six of the nine exact partial products accumulated in
 * fp32, smallest first (the three dropped ones are <= 2^-24 of |a b| and, with B's pieces rounded, zero-mean).  Against float64 the
 * result is as accurate as the fp32 MFMA chain (tests/test_gpu_parity.py::test_gemm_tn_bf16x6, ::test_bf16x6_adversarial_operands_vs_float64);
 * it is a different summation, so results differ from the fp32-MFMA kernel in the last bits.  Split-K ranges are whole 32-k blocks; the
 * rows of a K tail below 32 (unsplit products, the last range) are multiplied in a zero-padded block. */
#define FN_GEMM_BF16X6 0x20000
/* FN_GEMM_BF16X6 on the Linear-forward form (a_k=1,b_k=1; whole 128 x 128 tiles - at least 128 of them -, K % 32 == 0, 16-byte aligned operands, no
 * split): the same arithmetic through gemm_nt_x6w_kernel (gemm.hip); other shapes of that form ignore the flag and run on the fp32 MFMA. */
/* ... | FN_GEMM_X6_PERWAVE (only with FN_GEMM_BF16X6; tests / A-B measurements): the round-5 kernel in which every wavefront splits its own operands.
 * The default bf16 x 6 kernel has producer wavefronts that split every operand value once per workgroup and consumer wavefronts that only multiply
 * (gemm.hip: gemm_tn_x6w_kernel); both accumulate the same products in the same order, so on K ranges of whole 32-k blocks their results are
 * bit-identical. */
#define FN_GEMM_X6_PERWAVE 0x40000
/* ... | FN_GEMM_X6_WIDE (only with FN_GEMM_BF16X6): 128 x 256 output tiles per workgroup (gemm.hip: gemm_tn_x6v_kernel) instead of 128 x 128: a CU's
 * operand loads, which bound the 128 x 128 kernel, drop from 21 to 16 bytes per MFMA clock.  The caller wants twice the K ranges it would use with
 * 128 x 128 tiles (the same number of workgroups).  Same products in the same order per accumulator: bit-identical to the other two kernels on the
 * same K ranges. */
#define FN_GEMM_X6_WIDE 0x80000
/* ... | FN_GEMM_X6_PERTILE (only with FN_GEMM_BF16X6; tests / A-B measurements): one workgroup per output tile (Linear-forward form) or per (tile, K range)
 * item (weight-gradient form with K ranges in multiples of 8).  Default (round 6): one workgroup per CU walks its items, the next item's first blocks
 * are requested and cut while the finished one is stored.  Same arithmetic per item: bit-identical. */
#define FN_GEMM_X6_PERTILE 0x100000
size_t fn_gemm_ws_bytes(int M, int N, int splitk);
int fn_gemm_f32(int a_kmajor, int b_kmajor, int M, int N, int K, float alpha,
                const float* A, int lda, const float* B, int ldb, float beta, float* C, int ldc,
                const float* bias, int splitk, float* ws, size_t ws_bytes, void* stream);

/* The launch plan of fn_gemm_f32: which kernel instance the call launches, over which K ranges, on which grid, and which slab reduction follows.
 * It is decided by ONE pure host function (csrc/gemm_plan.h: shapes, leading dimensions, the alignment of the addresses, the flag bits and the number
 * of compute units in; this struct out) that fn_gemm_f32 launches from and that fn_gemm_plan hands out, so that a test asks the library what a call
 * reaches instead of restating the decision.  The addresses are inspected for their alignment only and never dereferenced (NULL counts as aligned);
 * `splitk` carries the FN_GEMM_* bits exactly as for fn_gemm_f32; cus > 0 stands for the compute units of the device (nothing touches the device
 * then), cus == 0 asks the current device.  FN_E_NULL without `plan`, FN_E_SHAPE for sizes fn_gemm_f32 refuses or cus < 0.
 * Both entry points are additive: fn_version() stays 6. */
enum FnGemmKernel {              /* FnGemmPlan.kernel; the names of the instances in this order: _lib.GEMM_PLAN_KERNELS */
    FN_PLAN_STAGED_64_64_16 = 0, /* gemm_kernel<BM, BN, BK, ..>: the LDS-staged kernel */
    FN_PLAN_STAGED_64_64_32,
    FN_PLAN_STAGED_32_64_32,
    FN_PLAN_STAGED_64_16_16,
    FN_PLAN_STAGED_128_128_32,
    FN_PLAN_NT_DIRECT_4_2,       /* gemm_nt_direct_kernel<PF, WGS>: the LDS-free Linear-forward kernel */
    FN_PLAN_NT_DIRECT_1_4,
    FN_PLAN_NT_X6W,              /* gemm_nt_x6w_kernel */
    FN_PLAN_TN,                  /* gemm_tn_kernel */
    FN_PLAN_TN_LEAN,             /* gemm_tn_lean_kernel */
    FN_PLAN_TN_X6,               /* gemm_tn_x6_kernel (FN_GEMM_X6_PERWAVE) */
    FN_PLAN_TN_X6W,              /* gemm_tn_x6w_kernel */
    FN_PLAN_TN_X6V,              /* gemm_tn_x6v_kernel (FN_GEMM_X6_WIDE) */
    FN_PLAN_KERNELS
};
enum FnGemmReduce { FN_PLAN_REDUCE_NONE = 0, FN_PLAN_REDUCE_SLAB = 1 /* slab_reduce_kernel */, FN_PLAN_REDUCE_SLAB4 = 2 /* slab_reduce4_kernel */ };
typedef struct FnGemmPlan {
    int32_t kernel;                 /* FnGemmKernel */
    int32_t klen, ranges;           /* K ranges of klen rows (the last one may be short): (ranges - 1) klen < K <= ranges klen */
    int32_t grid_x, grid_y, grid_z; /* tiles x 1 x ranges, or 1-D: tiles * ranges workgroups, or as many as compute units that walk those items */
    int32_t tiles;                  /* output tiles of the instance's tile shape */
    int32_t reduce, reduce_blocks;  /* FnGemmReduce (one exists exactly when ranges > 1) and its grid */
    int32_t msplit;                 /* fn_gru_dwhh_f32 as one launch: rows of the output from here on come from the second source (0: one source) */
} FnGemmPlan;
int fn_gemm_plan(int a_kmajor, int b_kmajor, int M, int N, int K, int lda, int ldb, int ldc, const void* A, const void* B, const void* C,
                 const void* bias, const void* ws, int splitk, int cus, FnGemmPlan* plan);

/* Up to 12 small independent GEMMs in ONE launch, each the sum of up to 4 products over separate operands (the heads of the path are
 * chains of 256-row GEMMs: e.g. mu_r = [h_fwd | h_rev] W^T is two products into one output, gmm_model.py:85-86):
 *   C_j[M,N] = sum_i opA(A_ji) opB(B_ji) + beta_j * C_j + bias_j      (a_kmajor / b_kmajor as in fn_gemm_f32, shared by all jobs) */
typedef struct FnGemmSeg {
    const float* A;
    int32_t lda;
    const float* B;
    int32_t ldb;
    int32_t K;
} FnGemmSeg;
typedef struct FnGemmJob {
    int32_t M, N;
    FnGemmSeg seg[4];
    int32_t n_seg;
    float beta;
    float* C;
    int32_t ldc;
    const float* bias;
} FnGemmJob;
int fn_gemm_multi(int a_kmajor, int b_kmajor, const FnGemmJob* jobs, int n_jobs, void* stream);

/* dst[c*dst_ld + r] = src[r*src_ld + c]  for r < R, c < C */
int fn_transpose_f32(const float* src, int R, int C, int src_ld, float* dst, int dst_ld, void* stream);
/* Column sums of up to FN_COLSUM_MAX_JOBS small matrices in ONE launch: out_j[n] = beta_j*out_j[n] + sum_m X_j[m*ld_j + n].
 * The bias gradients of a step (autograd of every `+ b` on the path, trainer_gmm.py:249) are ~40 column sums over <= 256-row
 * matrices; as separate launch pairs they were 76 launches of a few microseconds each on the critical tail of the step.
 * One workgroup per (job, 64 columns): rows are summed in a fixed order (4 row phases x 4 accumulators, then a fixed
 * tree) - deterministic.  Meant for M <= a few thousand rows; taller matrices belong to fn_colsum_f32. */
#define FN_COLSUM_MAX_JOBS 64
typedef struct FnColsumJob {
    const float* X;
    int32_t M, N, ld;
    float beta;
    float* out;
} FnColsumJob;
int fn_colsum_multi(const FnColsumJob* jobs, int n_jobs, void* stream);

/* out[n] = beta*out[n] + sum_m X[m*ld + n]; ws >= fn_colsum_ws_bytes(M,N) */
size_t fn_colsum_ws_bytes(int M, int N);
int fn_colsum_f32(const float* X, int M, int N, int ld, float beta, float* out, float* ws, size_t ws_bytes,
                  void* stream);
/* y[i] += alpha * x[i] */
int fn_axpy_f32(int64_t n, float alpha, const float* x, float* y, void* stream);
/* out[0] = sum x[0..n) (single workgroup, deterministic order) */
int fn_sum_f32(const float* x, int64_t n, float scale, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * GRU sequence scans (replace nn.GRU / nn.GRUCell loops: gmm_model.py:84,89,109,114,131-136).
 *
 * One call runs up to FN_MAX_SCANS independent scans concurrently: every time step is ONE
 * launch whose grid covers all scans (fused  h W_hh^T  MFMA GEMM + gate epilogue).
 * Gate order r,z,n (torch).  Input-side pre-activation of step p for batch row b:
 *    gx[b,:] = b_ih + gx_dense[p][b,:] + gx_table[tok][:] + gx_rowbias[b,:]     (each optional)
 *    tok = (tau < 0) ? start_token : idx[b*idx_ld + tau],  tau = (reverse ? T-1-p : p) + idx_shift
 * Storage is in PROCESSING order p = 0..T-1 (for reverse scans p=0 is the last time step).
 * H must be a multiple of 32.  The recurrent weights are passed in the FRAGMENT-MAJOR image produced by
 * fn_frag_pack (one contiguous 1 KB run per wave load instruction); frag_ws is caller-owned scratch of
 * 2 * fn_frag_floats(B, H) floats in which the scan ping-pongs the state in the same layout.
 * ------------------------------------------------------------------------------------------ */
/* Bits of FnGruFwd.variant / FnGruBwd.variant (scans[0]'s is used) and FnGruCell.variant.  0 = automatic; the other bits are tuning and
 * test switches, and results never depend on them beyond fp32 rounding (tests/test_gpu_parity.py compares the forms). */
#define FN_GRU_ROWS_MASK 0xFF         /* scans: force this many batch rows per workgroup of the single launch (16/32/64/128; not eligible ->
                                         per-step kernels).  Cells: the forced form 1-18 (see FnGruCell)                                     */
#define FN_GRU_ALT_TILING 0x100       /* scans: the alternative wave tiling of the 64-row configuration                                     */
#define FN_GRU_SYNC_ZEROED 0x200      /* scans: the sync_ws counters are ALREADY zero (the caller zero-fills a pool of regions once and gives
                                         every launch its own region: saves one memset node per launch)                                      */
#define FN_GRU_COMPILER_LOOPS 0x400   /* scans: the compiler-scheduled K loops instead of the hand-placed ones (kloop_asm.h); no ping-pong or
                                         register-stationary form                                                                            */
#define FN_GRU_NO_PINGPONG 0x800      /* scans: the round-3 loops (no ping-pong forward, no register-stationary backward)                    */
#define FN_GRU_SPREAD_XCDS 0x1000     /* scans: the workgroups of every row group are spread over all XCDs instead of sharing one (the
                                         default placement is speed only; the tests run both and compare)                                    */
#define FN_GRU_NO_RS_BWD 0x2000       /* backward scans: not the register-stationary kernel (gru_bwd_rs_kernel) - the 32-slice loop          */
#define FN_GRU_BF16X6 0x4000          /* the bf16 x 6 scans / cell: exact split products on the bf16 MFMA (see below and FN_GEMM_BF16X6)    */
#define FN_GRU_X6_SINGLE_GROUP 0x8000 /* with FN_GRU_BF16X6, forward scans: the single-group kernel instead of the ping-pong form (tests)      */
#define FN_GRU_X6_BWD_32ROWS 0x8000   /* with FN_GRU_BF16X6, backward scans: 32-row groups are eligible too (measured slower than the fp32
                                         kernel: only on request)                                                                            */
typedef struct FnGruFwd {
    int32_t B, T, H;
    int32_t reverse;          /* 1: consume tokens from the end (the *_reverse direction)      */
    const float* w_hh_frag;   /* fn_frag_pack(W_hh [3H][H])                                     */
    const float* b_hh;        /* [3H]                                                          */
    const float* b_ih;        /* [3H] or NULL                                                  */
    const float* h0;          /* [B][H] or NULL (= zeros)                                      */
    const float* gx_dense;    /* [T][B][3H] or NULL                                            */
    const float* gx_table;    /* [V][3H] (= W_ih[:, :V]^T) or NULL                             */
    const int32_t* idx;       /* [B][idx_ld] token ids, required with gx_table                 */
    int32_t idx_ld;
    int32_t idx_shift;        /* -1 for the global decoder (input of step i is token i-1)      */
    int32_t start_token;      /* used when tau < 0                                             */
    const float* gx_rowbias;  /* [B][3H] or NULL (per-sequence constant part, W_ih[:,V:] z)    */
    float* h_all;             /* [T][B][H] state after each step                               */
    float* gates;             /* [T][fn_gru_gates_floats(B,H)] saved r,z,n,(W_hn h + b_hn) in a    */
                              /* private blocked layout (opaque to the caller); NULL = inference */
    float* frag_ws;           /* scratch, 2 * fn_frag_floats(B, H) floats, 16-byte aligned         */
    void* sync_ws;            /* fn_gru_sync_ws_bytes() bytes, zero-filled ONCE by the caller, shared by  */
                              /* the scans of one call (scans[0]'s is used); NULL = per-step launches only */
    int32_t cu_budget;        /* compute units the single launch may occupy (scans[0]'s is used; 0 = all). */
                              /* Launches that can overlap on different streams must share the chip:       */
                              /* the sum of their budgets must not exceed the CU count.                    */
    const float* h0_frag;     /* optional: h0 already in the fragment-major operand layout (fn_frag_floats(B,H)  */
                              /* floats) - saves the packing launch when a scan continues a previous call (time  */
                              /* chunks, step-by-step decoding); h0 is still needed (row-major, gate epilogue)   */
    float* h_last_frag;       /* optional: the final state, fragment-major (the next call's h0_frag)       */
    int32_t variant;          /* 0 = automatic (scans[0]'s is used), else FN_GRU_* bits (above)                                   */
    void* err_ws;             /* optional: sticky error word outside sync_ws (>= 4 bytes, scans[0]'s is used); NULL = the last     */
                              /* 128 bytes of sync_ws                                                                            */
} FnGruFwd;

/* fragment-major operand image: floats needed for a [rows][K] matrix, and the packing kernel
 * (src row-major with leading dimension ld, K % 32 == 0; rows are zero-padded to a multiple of 16) */
/* OPT-IN (FnGruFwd.variant | FN_GRU_BF16X6): the forward scan with exact split products on the bf16 MFMA ("bf16 x 6", see FN_GEMM_BF16X6):
 * w_hh_frag must then be the fn_frag3_pack image of W_hh [3H][H] (bf16 triples hi | mid | lo, hi + mid + lo == W exactly; 3/2 of
 * fn_frag_floats(3H, H) floats) and frag_ws 3 * fn_frag_floats(B, H) floats (the state is exchanged as triples too).  H = 512, every
 * scan in full row groups of 64 (or 128) rows, saved gates, T >= 2 (h0_frag / h_last_frag are then triple images of 3/2 * fn_frag_floats(B, H)
 * floats); anything else returns FN_E_UNSUPPORTED (the caller repeats the call without the bit).  Same gate arithmetic; against the default kernels the states differ by fp32 rounding only
 * (tests/test_gpu_parity.py::test_forward_scan_bf16x6).
 * "Exactly" has a domain: hi + mid + lo == x holds for x == 0 and 2^-110 <= |x| < 2^128 (1 - 2^-9).  Below 2^-110 the last remainder can have a
 * bit under the smallest bf16 subnormal (2^-133), which is dropped; from 2^128 (1 - 2^-9) on (bits 0x7f7f8000) hi rounds to infinity.  Infinities
 * and NaNs have no split.  tests/test_images_reference.py sweeps every mantissa at both ends, tests/test_gpu_images.py checks the kernels on it. */
int fn_frag3_pack(const float* src, int rows, int K, int ld, void* dst, void* stream);
size_t fn_frag_floats(int rows, int K);
int fn_frag_pack(const float* src, int rows, int K, int ld, float* dst, void* stream);

/* All weight images of one optimiser step in ONE launch (the refresh after every Adam update: ~40 small matrices, ~56 with the bf16 triple images).
 *   kind 0: dst [cols][rows] = src^T                       (the one-hot column table W_ih[:, :V]^T; src [rows][cols], leading dim ld)
 *   kind 1: dst = fn_frag_pack image of src [rows][K = cols]  (cols % 32 == 0)
 *   kind 2: dst = fn_frag_pack image of src^T, the [cols][K = rows] matrix (rows % 32 == 0): W_hh^T for the backward scans
 *   kind 3: dst = fn_frag3_pack image (bf16 triples) of src [rows][K = cols]            (bf16 x 6 forward scans, FN_GRU_BF16X6)
 *   kind 4: dst = fn_frag3_pack image of src^T, the [cols][K = rows] matrix              (bf16 x 6 backward scans: W_hh^T)
 *   kind 5: dst [rows][cols] dense = src [rows][cols] (leading dim ld)                   (round 6: 16-byte aligned image of a column slice, W_ih[:, V:])
 * up to 56 jobs; dst of kinds 1 / 2 16-byte aligned with fn_frag_floats(...) floats, of kinds 3 / 4 with 3/2 of that. */
typedef struct FnWeightImage {
    const float* src;
    float* dst;
    int32_t rows, cols, ld, kind;
} FnWeightImage;
int fn_weight_images(const FnWeightImage* jobs, int n_jobs, void* stream);

/* floats per time step of the saved-gates buffer (4*H*ceil16(B)) */
size_t fn_gru_gates_floats(int B, int H);

/* When sync_ws is given, all scans share H <= 512 and sum_s ceil(B_s / rows) * H/16 fits one workgroup per CU, the
 * whole call is ONE weight-stationary launch whose workgroups exchange the state through frag_ws and meet at arrival
 * counters in sync_ws (every spin is bounded).  The last word of sync_ws is a sticky error flag: non-zero after a
 * launch whose workgroups gave up waiting (results of that and later calls are invalid until it is cleared). */
size_t fn_gru_sync_ws_bytes(void);
int fn_gru_seq_fwd(const FnGruFwd* scans, int n_scans, void* stream);
/* 1 when fn_gru_seq_fwd would take this call with FN_GRU_BF16X6 (bf16 x 6) on the current device, else 0 (shapes and gates != NULL only;
 * nothing is enqueued).  A scan that is cut into several calls (time chunks with h_last_frag -> h0_frag hand-over) must run ALL of its
 * calls on one arithmetic - the hand-over images differ (bf16 triples / fp32 fragments) - so the caller asks for every call of the chain first. */
int fn_gru_fwd_x6_ok(const FnGruFwd* scans, int n_scans);

/* ONE GRU cell step for a large batch (nn.GRUCell, gmm_model.py:131-136 in the eval-mode decode loop of thousands of rows):
 *    gi = x W_ih^T + b_ih + gx_table[tok] + gx_rowbias[b]      (every term optional)       gh = h_prev W_hh^T + b_hh
 *    r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h_out = (1 - z) n + z h_prev
 * as ONE MFMA launch with the gates in its epilogue (both products in its K loops: layer 2 of the decoder needs no separate W_ih
 * projection launch and no [B][3H] round trip).  Three kernels: above 512 rows (16-byte aligned operands, K1 % 16 == 0, row strides
 * % 4 == 0) loops whose lanes read their state-row operands straight from the K-contiguous rows - weights likewise, or as an
 * LDS-resident slice (one workgroup of ceil(rows / 512) x 64 rows x 16 units per CU; at K1 = H = 512 filled under the K loops, up to 2048 rows) -, otherwise an LDS-staged GEMM; they sum k in different orders (fp32 rounding apart).  Weights are the torch matrices themselves ([3H][K] row-major),
 * states row-major; h_out must not alias h_prev.  H % 32 == 0.
 * tok = idx ? idx[b * idx_ld] : start_token (point idx at the column of the previous step's tokens). */
typedef struct FnGruCell {
    int32_t B, H;
    const float* x;           /* [B][ldx] dense input, K1 valid columns, or NULL              */
    int32_t ldx, K1;
    const float* w_ih;        /* [3H][ldw_ih], K1 valid columns (required with x)             */
    int32_t ldw_ih;
    const float* gx_table;    /* [V][3H] (= W_ih[:, :V]^T) or NULL                            */
    const int32_t* idx;       /* token of row b at idx[b * idx_ld], or NULL = start_token     */
    int32_t idx_ld, start_token;
    const float* gx_rowbias;  /* [B][3H] or NULL                                              */
    const float* h_prev;      /* [B][ldh]                                                     */
    int32_t ldh;
    const float* w_hh;        /* [3H][ldw_hh]                                                 */
    int32_t ldw_hh;
    const float* b_ih;        /* [3H] or NULL                                                 */
    const float* b_hh;        /* [3H]                                                         */
    float* h_out;             /* [B][ldo]                                                     */
    int32_t ldo;
    int32_t variant;          /* 0 = automatic.  Tuning / tests: 1-3, 8 force a staged tiling (8 = its default: 64 rows x 32 units), 4-7 the LDS-free
                                 loop (4, 6: 128 rows x 32 units per workgroup, 1 / 2 k steps in flight; 5, 7: 64 rows, 4 / 2), 9-12 the loop with
                                 the weight slice in LDS (9, 11: 256 rows x 16 units, 2 steps; 10, 12: 128 rows, 4 / 8; 13, 14: 192 rows, 4 / 2), 15-18 the same with
                                 the slice fills under the K loops (K1 = H = 512; 15, 18: 128 rows, 4 / 2 steps; 16: 192 rows; 17: 256 rows) where eligible.
                                 | FN_GRU_BF16X6 (as in FnGruFwd): the cell on the bf16 MFMA with exact triple splits (gru.hip: gru_cell_x6_kernel) where
                                 B % 128 == 0, H % 32 == 0, K1 % 32 == 0 and the operands are 16-byte aligned; other shapes run as without the bit */
    const uint64_t* idx_best; /* NULL, or the packed argmax words of the previous token (fn_out_argmax_f32): the token of row b is
                                 best_v - 1 - (uint32_t)idx_best[b]; takes precedence over idx                                */
    int32_t best_v;           /* vocabulary size the words were packed with                                                   */
} FnGruCell;
int fn_gru_cell_f32(const FnGruCell* c, void* stream);

/* Output layer of the eval-mode decode with the argmax in its epilogue (gmm_model.py:137 + 73-80 when only the tokens are wanted; the
 * log-softmax is monotone, so argmax(log_softmax(logits)) = argmax(logits)): for every row b
 *     best[b] = max(best[b], max_v pack(h[b] . W[v] + bias[v], v)),   pack(x, v) = (uint64_t)key(x) << 32 | (uint32_t)(V - 1 - v),
 *     key(x)  = bits(x) ^ (bits(x) >> 31 ? 0xffffffff : 0x80000000)                (order-preserving; first index wins a tie)
 * by 64-bit atomic max: ZERO best[0 .. B) before the call; the logits are never written.  h [B][ldh], W [V][ldw] K-contiguous rows
 * (the torch matrix), 16-byte aligned, K % 16 == 0, ldh % 4 == ldw % 4 == 0.  One launch, LDS-free loop (as fn_gru_cell_f32's).
 * fn_best_tokens: tokens[b * tok_ld + t] = V - 1 - (uint32_t)best[t * B + b] for steps x B words. */
int fn_out_argmax_f32(const float* h, int ldh, const float* W, int ldw, const float* bias, int B, int V, int K, uint64_t* best,
                      void* stream);
int fn_best_tokens(const uint64_t* best, int steps, int B, int V, int32_t* tokens, int tok_ld, void* stream);
/* The launch plan of fn_out_argmax_f32 (csrc/decode_plan.h, as fn_gru_cell_plan): status = what the call returns for these arguments (NULL, shape,
 * a span of h or W of 4 GB or more, alignment - in this order); with FN_OK the kernel - the weight slice of a workgroup (48 rows x K) in LDS while
 * it is at most 128 KB, on eight waves when K % 32 == 0, else the LDS-free loop -, its grid, threads and dynamic LDS.  The choice does not depend
 * on the device; nothing touches it, nothing is enqueued.  FN_E_NULL without `plan`. */
enum FnOutArgmaxKernel {         /* FnOutArgmaxPlan.kernel; names: _lib.OUT_ARGMAX_KERNELS */
    FN_OUT_ARGMAX_LDS8 = 0,      /* out_argmax_lds8_kernel<4> */
    FN_OUT_ARGMAX_LDS,           /* out_argmax_lds_kernel<8> */
    FN_OUT_ARGMAX_DIRECT         /* out_argmax_direct_kernel<4> */
};
typedef struct FnOutArgmaxPlan {
    int32_t status;
    int32_t kernel;                 /* FnOutArgmaxKernel */
    int32_t grid, threads, lds_bytes;
} FnOutArgmaxPlan;
int fn_out_argmax_plan(const float* h, int ldh, const float* W, int ldw, const float* bias, int B, int V, int K, const uint64_t* best,
                       FnOutArgmaxPlan* plan);

/* Backward of the same scans (autograd of nn.GRU / GRUCell in loss.backward(), trainer_gmm.py:249).
 *   dh_p = dh_ext[p] (+ dh_last at p = T-1) + carried gradient
 *   outputs: dgx_all [T][B][3H] = d(pre-activations r,z,n) (= d gx, also d(W_hh h + b_hh) for r,z)
 *            dghn_all[T][B][H]  = d(W_hn h + b_hn)
 *            dh0 [B][H]  gradient wrt h0 (NULL = not needed)
 *            dgx_rowsum [B][3H] += sum_p dgx_all[p], dghn_rowsum [B][H] += sum_p dghn_all[p]
 *                        (NULL = not needed; caller zero-fills; their column sums are the bias gradients)
 * w_hh_t_frag = fn_frag_pack(W_hh^T [H][3H]).  scratch: [B][H] floats; frag_ws: 2 * fn_frag_floats(B, 3H) floats. */
typedef struct FnGruBwd {
    int32_t B, T, H;
    const float* w_hh_t_frag; /* fn_frag_pack(W_hh^T [H][3H])                                  */
    const float* h0;          /* [B][H] or NULL                                                */
    const float* h_all;       /* [T][B][H]  from forward                                       */
    const float* gates;       /* [T][fn_gru_gates_floats(B,H)] from forward                    */
    const float* dh_last;     /* [B][H] or NULL                                                */
    const float* dh_ext;      /* [T][B][H] or NULL                                             */
    float* dgx_all;           /* [T][B][3H]                                                    */
    float* dghn_all;          /* [T][B][H]                                                     */
    float* dh0;               /* [B][H] or NULL                                                */
    float* dgx_rowsum;        /* [B][3H] or NULL                                               */
    float* dghn_rowsum;       /* [B][H] or NULL                                                */
    float* scratch;           /* [B][H]                                                        */
    float* frag_ws;           /* 2 * fn_frag_floats(B, 3H) floats, 16-byte aligned             */
    void* sync_ws;            /* as in FnGruFwd (NULL = per-step launches; then scratch is required) */
    int32_t cu_budget;        /* as in FnGruFwd                                                */
    int32_t variant;          /* as in FnGruFwd                                                */
    void* err_ws;             /* as in FnGruFwd                                                */
} FnGruBwd;

int fn_gru_seq_bwd(const FnGruBwd* scans, int n_scans, void* stream);
/* variant | FN_GRU_BF16X6, as in FnGruFwd: the backward scan with exact split products on the bf16 MFMA (gru_bwd_x6_kernel).  w_hh_t_frag must then be
 * the bf16 TRIPLE image of W_hh^T [H][3H] (fn_weight_images kind 4; 3/2 of fn_frag_floats(H, 3H) floats) and frag_ws 3 * fn_frag_floats(B, 3H) floats
 * (the gate gradients are exchanged as triples).  H = 512, every scan in full groups of 64 rows (with FN_GRU_X6_BWD_32ROWS also: of 32 rows - that form
 * measured slower than the fp32 kernel and is not chosen on its own), T >= 2, 9..16 row groups that are all resident at once (the shapes of the
 * register-stationary fp32 kernel); anything else returns FN_E_UNSUPPORTED.  fn_gru_bwd_x6_ok answers without
 * enqueuing anything (1 / 0).  Same element-wise gate arithmetic; gradients differ from the default kernels by fp32 rounding only. */
int fn_gru_bwd_x6_ok(const FnGruBwd* scans, int n_scans);

/* The launch plan of fn_gru_seq_fwd / fn_gru_seq_bwd / fn_gru_cell_f32 (as fn_gemm_plan for the GEMMs): ONE pure host function per entry point
 * (csrc/gru_plan.h: the descriptors and the number of compute units in; these structs out) that the launch goes by and that fn_gru_fwd_plan /
 * fn_gru_bwd_plan / fn_gru_cell_plan hand out.  Addresses are inspected for NULL-ness and alignment only, never dereferenced.
 * A scan plan is an ordered list of at most three candidates: the launch takes the first one whose workgroups are all resident at once (the
 * weight-stationary kernels spin on counters that other workgroups of the launch advance); the per-step candidate needs no residency and is the last
 * one when present.  A bf16 x 6 request has exactly one candidate, or status FN_E_UNSUPPORTED.
 * cus > 0 stands for the compute units of the device (before cu_budget; nothing touches the device then, fits = -1 and chosen = -1 unless the per-step
 * candidate is the only one), cus == 0 asks the current device: fits is what the occupancy query of the launch answers and chosen the candidate the
 * launch takes (-1 with status FN_E_UNSUPPORTED when a bf16 x 6 candidate does not fit).  Nothing is enqueued.  status: what the call returns before
 * anything is enqueued (FN_OK: it launches a candidate).  FN_E_NULL without `plan`, FN_E_SHAPE for cus < 0.
 * The three entry points are additive: fn_version() stays 6. */
enum FnGruKernel {               /* FnGruCandidate.kernel; the names of the instances in this order: _lib.GRU_PLAN_KERNELS */
    FN_GRU_FWD_X6PP_1 = 0,       /* gru_fwd_x6pp_kernel<TH> */
    FN_GRU_FWD_X6PP_2,
    FN_GRU_FWD_X6_1,             /* gru_fwd_x6_kernel<MT> */
    FN_GRU_FWD_X6_2,
    FN_GRU_FWD_PP_1,             /* gru_fwd_pp_kernel<WK> */
    FN_GRU_FWD_PP_2,
    FN_GRU_FWD_WS_4_1_2,         /* gru_fwd_persist_kernel<WM, WK, MT, 4> */
    FN_GRU_FWD_WS_4_1_1,
    FN_GRU_FWD_WS_2_2_2,
    FN_GRU_FWD_WS_2_2_1,
    FN_GRU_FWD_WS_1_4_1,
    FN_GRU_FWD_STEP,             /* gru_fwd_step_kernel<NS, TM, D>, one launch per time step */
    FN_GRU_BWD_X6_1,             /* gru_bwd_x6_kernel<TH> */
    FN_GRU_BWD_X6_2,
    FN_GRU_BWD_RS_1,             /* gru_bwd_rs_kernel<TH> */
    FN_GRU_BWD_RS_2,
    FN_GRU_BWD_WS_4_1_2,         /* gru_bwd_persist_kernel<WM, WK, MT, 8> */
    FN_GRU_BWD_WS_4_1_1,
    FN_GRU_BWD_WS_2_2_2,
    FN_GRU_BWD_WS_2_2_1,
    FN_GRU_BWD_WS_1_4_1,
    FN_GRU_BWD_STEP,             /* gru_bwd_step_kernel<NS, TM, TN, D>, one launch per time step (and one for dh0) */
    FN_GRU_KERNELS
};
enum FnGruAbsent {               /* FnGruPlan.ws_absent: why the plan has no weight-stationary candidate (FN_GRU_WS_PRESENT: it has one) */
    FN_GRU_WS_PRESENT = 0,
    FN_GRU_WS_H_OVER_512,
    FN_GRU_WS_NO_SYNC_WS,
    FN_GRU_WS_MIXED_H,
    FN_GRU_WS_UNALIGNED,         /* an operand of the 16-byte epilogue vectors is not 16-byte aligned */
    FN_GRU_WS_T_BELOW_2,         /* nothing to keep stationary */
    FN_GRU_WS_SLICES_OVER_CUS,
    FN_GRU_WS_NO_ROW_BLOCK       /* no (or not the forced) row block whose groups fit the compute units; bf16 x 6: the shapes are not eligible */
};
typedef struct FnGruCandidate {
    int32_t kernel;                 /* FnGruKernel */
    int32_t rows_per_group, groups; /* weight-stationary: batch rows of a row group, row groups of the launch (sum over the scans) */
    int32_t slices;                 /* weight-stationary: workgroups of a row group; grid = groups * slices */
    int32_t grid, lds_bytes;        /* weight-stationary: workgroups and dynamic LDS of the launch */
    int32_t no_hand;                /* 1: the compiler-scheduled K loops (FN_GRU_COMPILER_LOOPS) */
    int32_t h0_triples;             /* initial states are packed as bf16 triples (1) or as fp32 fragments (0) */
    int32_t resident;               /* 1: every workgroup of the grid must be resident at once */
    int32_t fits;                   /* resident candidates: 1 / 0 as the occupancy query answers, -1 = not asked */
    int32_t tm, tn, d, ns;          /* per-step: template arguments of the FIRST launch (tn = 0: forward) */
    int32_t tiles, launches;        /* per-step: workgroups of the first launch; launches of the call */
} FnGruCandidate;
typedef struct FnGruPlan {
    int32_t status;                 /* FN_OK, or the FN_E_* the call returns before anything is enqueued */
    int32_t n, chosen;              /* candidates; the one the launch takes (-1: not known / none) */
    int32_t cus;                    /* compute units of the launch: the device's, or scans[0].cu_budget when that is smaller */
    int32_t ws_absent;              /* FnGruAbsent */
    FnGruCandidate cand[3];
} FnGruPlan;
int fn_gru_fwd_plan(const FnGruFwd* scans, int n_scans, int cus, FnGruPlan* plan);
int fn_gru_bwd_plan(const FnGruBwd* scans, int n_scans, int cus, FnGruPlan* plan);

enum FnGruCellFamily {           /* FnGruCellPlan.family; names: _lib.GRU_CELL_FAMILIES */
    FN_CELL_STAGED = 0,          /* gru_cell_kernel<BM, WM, WN> */
    FN_CELL_DIRECT,              /* gru_cell_direct_kernel<RT, PF, HAS_TAB, HAS_RB> */
    FN_CELL_WLDS,                /* gru_cell_wlds_kernel<RT, PF, HAS_TAB, HAS_RB> */
    FN_CELL_WLDS_OVL,            /* gru_cell_wlds_ovl_kernel<RT, PF, HAS_TAB, HAS_RB> */
    FN_CELL_X6                   /* gru_cell_x6_kernel<HAS_TAB, HAS_RB> */
};
typedef struct FnGruCellPlan {
    int32_t status;                 /* FN_OK, or the FN_E_* fn_gru_cell_f32 returns for these arguments */
    int32_t family;                 /* FnGruCellFamily */
    int32_t t0, t1, t2;             /* template arguments: BM, WM, WN (staged); RT, PF, 0 (direct, wlds, wlds-overlap); 0 (x6) */
    int32_t has_tab, has_rb;        /* gx_table / gx_rowbias given: the HAS_TAB / HAS_RB instance of the families that have them */
    int32_t kmax;                   /* the longer of the two K loops (H, or K1 with x) */
    int32_t grid, threads, lds_bytes;
    int32_t forced_honoured;        /* 1: variant names a form 1-18 and that form is what runs; 0: automatic choice, bf16 x 6, or the staged default stands in */
} FnGruCellPlan;
int fn_gru_cell_plan(const FnGruCell* c, FnGruCellPlan* plan);

/* Recurrent weight gradient of one scan from its saved gate gradients (autograd of W_hh in nn.GRU / GRUCell,
 * trainer_gmm.py:249):  dW_hh[3H][H] = beta * dW_hh + [dgx[:, 0:2H] | dghn]^T hprev  over `rows` (time x batch) rows;
 * dgx [rows][3H], dghn [rows][H], hprev [rows][H] (the state BEFORE each step).  One split-K launch when 2H % 128 == 0. */
size_t fn_gru_dwhh_ws_bytes(int H, int splitk);
int fn_gru_dwhh_f32(const float* dgx, const float* dghn, const float* hprev, int64_t rows, int H, float beta, float* dW,
                    int splitk, float* ws, size_t ws_bytes, void* stream);
/* The launch plan of fn_gru_dwhh_f32 (see fn_gemm_plan; same treatment of the addresses and of cus): *n_launches = 1 and plans[0] with
 * msplit = 2H for the one split-A launch, or *n_launches = 2 and the plans of the two products - rows [0, 2H) of dW from dgx, rows [2H, 3H) from
 * dghn -, which do not carry FN_GEMM_LEAN on.  FN_E_NULL without n_launches / plans, FN_E_SHAPE as fn_gru_dwhh_f32 or for cus < 0. */
int fn_gru_dwhh_plan(const void* dgx, const void* dghn, const void* hprev, const void* dW, const void* ws, int64_t rows, int H, int splitk, int cus,
                     int32_t* n_launches, FnGemmPlan plans[2]);

/* Gradient of the one-hot columns of W_ih (autograd of  onehot(x) @ W_ih[:, :V]^T, gmm_model.py:84,89,109,114,132-133):
 *   dTable[v][:] = sum over (p,b) with tok(p,b)==v of dgx_all[p][b][:]      (tok defined as in FnGruFwd)
 * Two steps, so that ONE sort of a token matrix serves every scan that consumes it (4 encoder directions + decoder layer 1):
 *   fn_token_sort: idx [B][idx_ld] int32 -> img (fn_token_sort_ints(B*T, V) int32: segment starts, piece starts, positions
 *                  sorted by token, stable); ws >= fn_token_sort_ws_bytes(B*T, V), 16-byte aligned.  Tokens are clamped to [0, V).
 *   fn_embed_grad_sorted: up to 8 jobs (scans) that read the SAME token matrix in one launch pair; per job idx_shift in {0, -1}
 *                  (-1 only with reverse = 0: step p reads token p-1, step 0 the start token).  out is [V][out_ld] (out_ld >= N3),
 *                  or with transposed != 0 the transposed table [N3][out_ld] (out_ld >= V), e.g. dW_ih[:, :V] in place.
 *                  ws >= fn_embed_grad_sorted_ws_bytes(B*T, B, V, N3, n_jobs).  Deterministic (fixed summation order).
 * fn_embed_grad_f32 = both steps for one scan (ws >= fn_embed_grad_ws_bytes(T*B, V, N3)). */
typedef struct FnEmbedGrad {
    const float* dgx_all;     /* [T][B][N3] gate gradients in processing order                    */
    float* out;               /* table, see above                                                  */
    int32_t out_ld;
    int32_t transposed;
    int32_t reverse, idx_shift, start_token;
} FnEmbedGrad;
size_t fn_token_sort_ints(int64_t rows, int V);
size_t fn_token_sort_ws_bytes(int64_t rows, int V);
int fn_token_sort(const int32_t* idx, int B, int T, int idx_ld, int V, int32_t* img, void* ws, size_t ws_bytes, void* stream);
size_t fn_embed_grad_sorted_ws_bytes(int64_t rows, int B, int V, int N3, int n_jobs);
int fn_embed_grad_sorted(const FnEmbedGrad* jobs, int n_jobs, int B, int T, int N3, int V, const int32_t* img, float* ws,
                         size_t ws_bytes, void* stream);
size_t fn_embed_grad_ws_bytes(int64_t rows, int V, int N3);
int fn_embed_grad_f32(const float* dgx_all, int B, int T, int N3, const int32_t* idx, int idx_ld, int idx_shift,
                      int start_token, int reverse, int V, float* out, float* ws, size_t ws_bytes, void* stream);

/* out[m] = sum_t X[t*M + m]   (per-sequence sums over time of the gate gradients; M % 4 == 0, 16-byte aligned) */
int fn_time_sum_f32(const float* X, int T, int64_t M, float* out, void* stream);

/* Greedy autoregressive decode of the global decoder for B <= 2048 sequences (H <= 512) as ONE launch
 * (gmm_model.py:119-149 with model.eval(): layer-1 cell, layer-2 cell (state initialised with the first layer-1 state, :134-135),
 * 512 -> V output layer, log_softmax, feedback = first-index argmax, :73-80,147-148).  Workgroup sets keep the four weight
 * matrices in LDS and hand activations over through L2 (bounded spins, sticky error word as in fn_gru_seq_fwd).  More than 32
 * sequences (the reference's evaluators decode 8 fader values x 100 samples at once, test_class.py:84-85,253) travel through the
 * role workgroups as a pipeline of 32-row blocks (64-row blocks from 353 sequences on: a role's time per block is mostly latency), two
 * replicas of the role set side by side when the device has the CUs. */
typedef struct FnDecode {
    int32_t B, steps, H, V;
    int32_t start_token;      /* input token of step 0 (V - 1)                                       */
    const float* w_hh1_frag;  /* fn_frag_pack(grucell_g.weight_hh [3H][H])                            */
    const float* b_hh1;       /* [3H]                                                                */
    const float* b_ih1;       /* [3H] or NULL                                                        */
    const float* table1;      /* [V][3H] = grucell_g.weight_ih[:, :V]^T (token rows)                  */
    const float* rowbias1;    /* [B][3H] = z @ grucell_g.weight_ih[:, V:]^T, or NULL                  */
    const float* h0;          /* [B][H] = linear_init_global(z)                                       */
    const float* w_ih2_frag;  /* fn_frag_pack(grucell_g_2.weight_ih [3H][H])                          */
    const float* b_ih2;       /* [3H] or NULL                                                        */
    const float* w_hh2_frag;  /* fn_frag_pack(grucell_g_2.weight_hh [3H][H])                          */
    const float* b_hh2;       /* [3H]                                                                */
    const float* w_out_frag;  /* fn_frag_pack(linear_out_g.weight [V][H])                             */
    const float* b_out;       /* [V]                                                                 */
    int32_t* tokens;          /* out [B][tok_ld]: token of every step                                */
    int32_t tok_ld;
    float* logp;              /* out [B][steps][V] log-probabilities, or NULL                        */
    float* ws;                /* fn_decode_ws_bytes(B, H, V) bytes, 16-byte aligned                   */
    void* sync_ws;            /* fn_decode_sync_ws_bytes() bytes, zero-filled once by the caller       */
} FnDecode;
size_t fn_decode_ws_bytes(int B, int H, int V);
size_t fn_decode_sync_ws_bytes(void);
int fn_decode_greedy(const FnDecode* d, void* stream);

/* The same decode with FORCED feedback under a per-step mask: after step i the decoder is fed a given token instead of its own argmax
 * wherever the mask says so.  This is the reference's train-mode loop (gmm_model.py:139-148: `p = torch.rand(1)`, `if p < self.eps:
 * out = sample[:, i]` else `out = self._sampling(out)`) with force[i] = (p_i < eps) and forced = the data tokens, and prompted
 * continuation with force = a prefix of ones.  d->tokens / d->logp keep their meaning: the model's OWN first-index argmax and
 * log-probabilities of every step, forced or not; the stream that was fed back is fed[b][i] = force[i] ? forced[b][i] : tokens[b][i].
 * The mask is read from device memory at every step, so one captured graph serves any mask.  A forced token is clamped to [0, V)
 * (as fn_token_sort clamps).  force[steps-1] is ignored (nothing is fed after the last step).  Shape, alignment and eligibility
 * answers are fn_decode_greedy's; f, f->forced or f->force NULL: FN_E_NULL; forced_ld < steps: FN_E_SHAPE. */
typedef struct FnDecodeForce {
    const int32_t* forced;    /* [B][forced_ld] tokens, forced_ld >= steps                            */
    int32_t forced_ld;
    const uint8_t* force;     /* [steps] DEVICE bytes: force[i] != 0 -> the token fed into step i+1 is forced[b][i],
                                 else the first-index argmax of step i (as fn_decode_greedy)          */
} FnDecodeForce;
int fn_decode_forced(const FnDecode* d, const FnDecodeForce* f, void* stream);

/* The launch plan of fn_decode_greedy (f == NULL) / fn_decode_forced (as fn_gru_fwd_plan for the scans): ONE pure host function (csrc/decode_plan.h:
 * the descriptors and the number of compute units in, this struct out) that the launch goes by.  The kernel spins on counters that other workgroups
 * of the same launch advance, so grid = nrep * per_rep is exactly what fits with one workgroup per compute unit.  status: what the call returns
 * before anything is enqueued - the checks in their order (f's members, d's NULL members, shape, alignment), FN_E_UNSUPPORTED when one role set has
 * more workgroups than the device compute units (no current device counts as 0 compute units), FN_E_SHAPE for more than 32 blocks; the other fields
 * are valid with FN_OK only.  The occupancy query of the launch (does one workgroup with lds_bytes fit a compute unit) is not part of it.
 * cus > 0 stands for the compute units of the device and touches no device, cus == 0 asks the current one.  Nothing is enqueued.
 * FN_E_NULL without `plan`, FN_E_SHAPE for cus < 0.  fn_decode_plan and fn_out_argmax_plan are additive: fn_version() stays 6. */
typedef struct FnDecodePlan {
    int32_t status;
    int32_t forced;                 /* 1: the fn_decode_forced instance of the kernel */
    int32_t mt, block_rows, nblk;   /* row tiles of a block (1 up to 16 sequences, 4 from 353 on, else 2), its rows = 16 mt, blocks = ceil(B / block_rows) */
    int32_t nvt, nslices;           /* output slices ceil(V / 16), hidden slices H / 16 */
    int32_t per_rep, nrep;          /* workgroups of one role set 3 nslices + nvt + 1; replicas of it min(cus / per_rep, nblk): replica r takes blocks r, r + nrep, .. */
    int32_t grid, threads, lds_bytes;
    int64_t x1_off, x2_off, g2_off, logits_off, ws_floats; /* FnDecode.ws in floats: where the four regions start, where the last one ends (<= fn_decode_ws_bytes / 4) */
} FnDecodePlan;
int fn_decode_plan(const FnDecode* d, const FnDecodeForce* f, int cus, FnDecodePlan* plan);

/* ------------------------------------------------------------------------------------------
 * Output heads
 * ------------------------------------------------------------------------------------------ */
/* vocab-axis log_softmax (+ optional fused NLL and its gradient): gmm_model.py:137 + trainer_gmm.py:131.
 * logits [T*B][ld] time-major rows (row = t*B + b), E valid columns.
 *   logp_bt  [B][T][E] or NULL   log-probabilities in the reference's (B,T,E) layout
 *   target   [B][T] int32 or NULL
 *   nll_rows [T*B] or NULL       -logp[target] per row
 *   dlogits  [T*B][ld] or NULL   grad_scale * (softmax - onehot(target))   (may alias logits)  */
int fn_vocab_logsoftmax(const float* logits, int B, int T, int E, int ld, float* logp_bt, const int32_t* target,
                        float* nll_rows, float grad_scale, float* dlogits, void* stream);
/* The same head FUSED with its projection (gmm_model.py:137 `log_softmax(linear_out_g(hx[1]))` + trainer_gmm.py:131-132 `nll_loss` and
 * their autograd): logits = h W^T + bias never reach memory.
 *   h        [T*B][ldh] time-major rows (row = t*B + b), H valid columns (the layer-2 states)
 *   W        [V][ldw]   linear_out_g.weight, bias [V];  V <= 384 (else FN_E_UNSUPPORTED)
 *   target   [B][T] int32
 *   nll_rows [T*B] or NULL       -log_softmax(logits)[target]
 *   dlogits  [T*B][ld] or NULL   grad_scale * (softmax - onehot(target)); ld a multiple of 4, V <= ld <= 384, 16-byte aligned;
 *                                columns [V, ld) are written as zeros
 * With 16-byte aligned operands and H % 16 == 0 the projection runs as an LDS-free loop whose k order inside a 16-k step differs from
 * fn_gemm_f32's (fixed, deterministic); the row sums run in a different order than fn_vocab_logsoftmax's. */
int fn_out_head_f32(const float* h, int ldh, const float* W, int ldw, const float* bias, int B, int T, int V, int H,
                    const int32_t* target, float grad_scale, float* nll_rows, float* dlogits, int ld, void* stream);
/* generic backward of the same log_softmax: dlogits[row] = g - softmax * sum(g), g = gout_bt[b][t][:] */
int fn_vocab_logsoftmax_bwd(const float* logp_bt, const float* gout_bt, int B, int T, int E, int ld, float* dlogits,
                            void* stream);
/* greedy head for inference (gmm_model.py:73-80,137,147-148): log_softmax + argmax (first index on ties)
 * logits [B][ld] -> logp_out [B][E] (row stride logp_ld) or NULL, tok_out[b*tok_ld] */
int fn_vocab_argmax(const float* logits, int B, int E, int ld, float* logp_out, int64_t logp_ld, int32_t* tok_out,
                    int tok_ld, void* stream);

/* Seeded temperature / top-k / top-p draw from the same head (decode.sample_decode).  There is NO reference counterpart: the reference's
 * _sampling (gmm_model.py:73-80) is the argmax above; the definition below is the specification.  Per row b of logits [B][ld], V valid columns,
 * 1 <= V <= FN_SAMPLE_MAX_V:
 *   1. lp[e] = x[e] - lse and the first-index argmax, computed as the greedy head computes them: logp_out [B][V] (row stride logp_ld) and
 *      own_out[b*own_ld], both optional, are bit-identical to the greedy head's outputs on the same logits;
 *   2. descending order by lp, ties to the lower index: rank[e] = #{e' : lp[e'] > lp[e] or (lp[e'] == lp[e] and e' < e)};
 *   3. sorted weights w[rank[e]] = expf((lp[e] - max lp) * inv_temperature), sorted indices idx[rank[e]] = e;
 *   4. inclusive fp32 prefix sums c[j] of w: with per = ceil(V / 64), block l = entries per*l .. per*l + per - 1 is summed in order from 0.0f,
 *      the 64 block totals are scanned inclusively (for o = 1, 2, .. 32: t[l] += t[l - o] for every l >= o, all l at once),
 *      c[j] = (scanned total of block l - 1, 0.0f for l = 0) + (running sum inside block l);
 *   5. the kept set is a prefix of the order: n = top_k ? min(top_k, V) : V;  m = top_p < 1 ? min(n, 1 + #{j < n : c[j] < top_p * c[n-1]}) : n
 *      (fp32 product).  Where c is non-decreasing that is the smallest m with c[m-1] >= top_p * c[n-1]; across a block border of step 4 the
 *      fp32 sums can step down by an ulp, so the COUNT is the definition, here and in step 6;
 *   6. u = (Philox4x32-10(counter = (b, step, offset_lo, offset_hi), key = (seed_lo, seed_hi))[0] >> 8) * 2^-24, in [0, 1);
 *      tok_out[b*tok_ld] = idx[j], j = min(m - 1, #{j < m : not c[j] > u * c[m-1]}) (fp32 product; the first index with c[j] > u c[m-1] where
 *      c is non-decreasing);  u_out[b] = u when given.
 * The draw depends on the row of the batch and on `step` (a launch argument), not on the launch geometry.  The parameters are read from
 * DEVICE memory, so a captured graph serves any seed or setting; as they come from memory they are clamped: top_k to [0, V], top_p to
 * [FN_SAMPLE_MIN_P, 1] (NaN: 1), inv_temperature to [FN_SAMPLE_MIN_INV_T, FN_SAMPLE_MAX_INV_T] (NaN: 1).  Rows that hold NaNs give an
 * unspecified token in [0, V).  logits, params or tok_out NULL: FN_E_NULL; B < 1, V outside [1, FN_SAMPLE_MAX_V], ld < V, step < 0:
 * FN_E_SHAPE; both before any launch. */
#define FN_SAMPLE_MAX_V 1024
#define FN_SAMPLE_MIN_P 1e-30f
#define FN_SAMPLE_MIN_INV_T 1e-30f
#define FN_SAMPLE_MAX_INV_T 1e30f
typedef struct FnSampleParams {      /* 32 bytes */
    uint32_t seed_lo, seed_hi;       /* the Philox key: a 64-bit seed                                                  */
    uint32_t offset_lo, offset_hi;   /* counter words 2, 3: a 64-bit offset (another stream of draws under one seed)   */
    float inv_temperature;           /* 1 / temperature                                                                */
    float top_p;                     /* 1: off                                                                         */
    int32_t top_k;                   /* 0: off                                                                         */
    int32_t reserved;                /* 0                                                                              */
} FnSampleParams;
int fn_vocab_sample(const float* logits, int B, int V, int ld, const FnSampleParams* params_dev, int step, float* logp_out,
                    int64_t logp_ld, int32_t* own_out, int own_ld, int32_t* tok_out, int tok_ld, float* u_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Beam search over the same head (decode.beam_decode): select, state reorder, backtrack.  There is NO reference counterpart: the reference's
 * decode loop (gmm_model.py:73-80,119-149) feeds back the argmax of one stream; these three replace that feedback by the W best streams per
 * latent.  The text below is the specification.  B sequences of W beams: row r = b*W + w of every [B*W][..] matrix is beam w of sequence b.
 *   1 <= W <= min(V, FN_BEAM_MAX_W),  1 <= V <= FN_SAMPLE_MAX_V.
 *
 * fn_beam_step - one decode step, one launch.  logits [B*W][ld], V valid columns; step >= 0; eos in [0, V) or -1 = none;
 * score_prev / token_prev: the previous step's score / token slabs [B][prev_ld] (fp32 / int32, W valid entries; not read at step 0, may then
 * be NULL); score / parent / token: this step's slabs [B][out_ld]; logp_out [B*W][V] (row stride logp_ld) or NULL.  Per sequence b, in fp32:
 *   lp      lp[w][e] = x[e] - lse of row b*W + w, computed as the greedy head computes it: logp_out, when given, is written for EVERY row and is
 *           bit-identical to fn_vocab_argmax's logp_out on the same logits;
 *   beams   beam w is LIVE iff step > 0 || w == 0, FINISHED iff step > 0 && eos >= 0 && token_prev[b][w] == eos.  The logits rows of non-live
 *           and finished beams play no part in score / parent / token (they may hold NaN);
 *   cands   a live, unfinished beam contributes the V candidates (w, e) with s = score_prev[b][w] + lp[w][e] - ONE fp32 add, score_prev taken
 *           as 0.0f at step 0; a finished beam contributes the single candidate (w, eos) with s = score_prev[b][w];
 *   order   candidates are ordered by the 64-bit word pack(s, w*V + e) of fn_out_argmax_f32 with W*V columns: key(s) in the high half,
 *           W*V - 1 - (w*V + e) in the low half, the larger word first - higher score, then lower beam, then lower token (key orders
 *           -0.0f below +0.0f);
 *   output  j = 0 .. W-1 is the j-th candidate: score[b][j] = s, parent[b][j] = w, token[b][j] = e.  W <= V: there are always >= W candidates.
 * A live, unfinished row that holds NaN gives unspecified outputs with parent in [0, W) and token in [0, V).  Every input of a sequence is read
 * before any of its slab outputs is written.  A finished hypothesis is extended by eos at no cost at every later step.
 * logits, score, parent or token NULL, score_prev or token_prev NULL at step > 0: FN_E_NULL; B < 1, W or V outside the limits, ld < V,
 * step < 0, eos >= V or < -1, out_ld < W, prev_ld < W at step > 0: FN_E_SHAPE; both before any launch.
 *
 * fn_beam_gather - reorder up to FN_BEAM_GATHER_MAX_JOBS state matrices by parent in one launch (jobs is a HOST array):
 *   dst_k[r][c] = src_k[(r / W) * W + clamp(parent[r], 0, W-1)][c]    for r < rows (= B*W, a multiple of W), c < cols_k;  parent [rows] int32.
 * 16-byte copies where a job's pointers and leading dimensions allow, scalar copies otherwise; entries beyond cols_k are not touched.
 * dst must not alias src.  jobs, parent, a src or a dst NULL: FN_E_NULL; n_jobs outside [1, FN_BEAM_GATHER_MAX_JOBS]: FN_E_COUNT; rows < 1,
 * W outside [1, FN_BEAM_MAX_W], rows % W != 0, cols < 1, a leading dimension < cols, dst == src: FN_E_SHAPE.
 *
 * fn_beam_backtrack - the W final hypotheses of every sequence from the slabs parent / token / score [steps][B][W] (contiguous), one thread
 * per (b, j):  cur = j;  for t = steps-1 .. 0:  p = clamp(parent[t][b][cur], 0, W-1);  tokens_out[b][j][t] = token[t][b][cur];
 * cum_out[b][j][t] = score[t][b][cur] (the cumulative score along the path);  beam_out[b][j][t] = p - the row of step t's logits / logp_out
 * the hypothesis extended;  cur = p.   len_out[b][j] = 1 + the first t with tokens_out[b][j][t] == eos, or steps (eos = -1: steps);
 * score_out[b][j] = score[steps-1][b][j].  As a finished hypothesis keeps being extended by eos, the positions after its end hold eos and
 * repeat its final score.  tokens_out / beam_out / cum_out [B][W][steps]; beam_out and cum_out may be NULL.
 * A required pointer NULL: FN_E_NULL; steps, B < 1, W outside [1, FN_BEAM_MAX_W], eos < -1: FN_E_SHAPE. */
#define FN_BEAM_MAX_W 16
#define FN_BEAM_GATHER_MAX_JOBS 4
typedef struct FnBeamGatherJob {
    const float* src;         /* [rows][src_ld]                                                */
    int32_t src_ld;
    float* dst;               /* [rows][dst_ld]                                                */
    int32_t dst_ld;
    int32_t cols;
} FnBeamGatherJob;
int fn_beam_step(const float* logits, int B, int W, int V, int ld, int step, int eos, const float* score_prev, const int32_t* token_prev,
                 int prev_ld, float* score, int32_t* parent, int32_t* token, int out_ld, float* logp_out, int64_t logp_ld, void* stream);
int fn_beam_gather(const FnBeamGatherJob* jobs, int n_jobs, int rows, int W, const int32_t* parent, void* stream);
int fn_beam_backtrack(const int32_t* parent, const int32_t* token, const float* score, int steps, int B, int W, int eos,
                      int32_t* tokens_out, int32_t* beam_out, float* cum_out, int32_t* len_out, float* score_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Constrained decode (decode.Constraints): a logit processor in front of the three heads above and a state update behind them.  There is NO
 * reference counterpart (the reference's loop feeds back its argmax, gmm_model.py:73-80,119-149); the text below is the specification.  The heads
 * take -inf logits as they are (lp = -inf, weight 0, a key below every real score), so a ban is a logit of -inf and no head changes.
 *
 * The scalars are read from DEVICE memory (params_dev), so a captured graph serves any setting; as they come from memory they are clamped:
 * n = min(max(n_pitch, 0), 128); token e in [0, V) is the NOTE-ON of pitch p iff p = e - on_lo lies in [0, n), else the NOTE-OFF of pitch p iff
 * p = e - off_lo lies in [0, n) (the ranges are so cut to [0, V); where they overlap the on range has precedence), else neither.
 * held [rows][4] uint32: bit p & 31 of word p >> 5 of row r is set iff pitch p sounds in row r.
 *
 * fn_constrain_apply - in place on logits [rows][ld], V valid columns (1 <= V <= FN_SAMPLE_MAX_V), columns [V, ld) are not touched; step >= 0;
 * bias fp32 or NULL, row r reads bias[r*bias_rs + e] (bias_rs = 0: one shared [V] vector); held or NULL; stuck [rows] int32 or NULL.  Per row r:
 *   1. y[e] = bias ? x[e] + bias[r*bias_rs + e] : x[e]                                  (ONE fp32 add; -inf entries of bias are bans)
 *   2. G = the eos and grammar bans:  {eos} if 0 <= eos < V && step < min_len;  and, with held != NULL && n > 0, c = popcount(held[r]):
 *        the note-off of p for every p NOT sounding    if flags & FN_CONSTRAIN_OFF_NEEDS_ON,
 *        the note-on  of p for every p sounding        if flags & FN_CONSTRAIN_NO_REONSET,
 *        the note-on  of p for every p NOT sounding    if max_poly > 0 && c >= max_poly   (all 128 bits of held[r] count);
 *   3. if no e in [0, V) has y[e] > -inf && e not in G, the row is STUCK: G is dropped for this row at this step and stuck[r], when given, is
 *      incremented (a plain load, add and store by one lane of the row's wavefront; the caller zeroes it);
 *   4. x[e] = (e in G, row not stuck) ? -inf : y[e].
 * A row whose bias alone leaves nothing above -inf, or which holds NaN, is stuck or not - unspecified -, every access stays in bounds.
 * logits or params_dev NULL: FN_E_NULL; rows < 1, V outside [1, FN_SAMPLE_MAX_V], ld < V, step < 0, bias != NULL with bias_rs neither 0 nor
 * >= V: FN_E_SHAPE; both before any launch.
 *
 * fn_constrain_advance - behind the head, one thread per row r; tok = tok_io[r*tok_ld]:
 *   fix-up  only with logits != NULL ([rows][ld], the rows fn_constrain_apply left): if tok is outside [0, V) or logits[r*ld + tok] == -inf then
 *           tok = min(max(fallback[r*fb_ld], 0), V - 1) is written back to tok_io[r*tok_ld] and fixed[r] ([rows] int32 or NULL, zeroed by the
 *           caller) is incremented.  (fn_vocab_sample's draw is a COUNT over fp32 prefix sums that can step down by an ulp across a block border,
 *           so a zero-weight entry behind the last positive one can be counted in when u is the largest uniform; fallback = its own_out, the
 *           first-index argmax of the constrained row, is always allowed.  With fn_vocab_argmax the fix-up never fires.)  Without logits tok_io
 *           is only read.
 *   state   only with held_in != NULL: held_out[r] = held_in[r] with bit p set if tok is the note-on of p, cleared if tok is the note-off of p
 *           (a tok outside [0, V) is neither).  held_out may equal held_in; the four words of a row are read before any is written.
 * tok_io or params_dev NULL, fallback NULL with logits, held_out NULL with held_in: FN_E_NULL; rows < 1, V outside [1, FN_SAMPLE_MAX_V],
 * tok_ld < 1, with logits: ld < V or fb_ld < 1: FN_E_SHAPE; both before any launch. */
#define FN_CONSTRAIN_OFF_NEEDS_ON 1
#define FN_CONSTRAIN_NO_REONSET 2
#define FN_CONSTRAIN_MAX_PITCH 128
typedef struct FnConstrainParams {   /* 32 bytes */
    int32_t on_lo, off_lo, n_pitch;  /* note-on tokens [on_lo, on_lo+n_pitch), note-off [off_lo, off_lo+n_pitch); n_pitch 0 = no grammar, <= 128 */
    int32_t max_poly;                /* 0: off */
    int32_t eos, min_len;            /* eos -1: none; eos is banned while step < min_len */
    uint32_t flags;                  /* FN_CONSTRAIN_OFF_NEEDS_ON = 1, FN_CONSTRAIN_NO_REONSET = 2 */
    int32_t reserved;
} FnConstrainParams;
int fn_constrain_apply(float* logits, int rows, int V, int ld, int step, const FnConstrainParams* params_dev, const float* bias, int64_t bias_rs,
                       const uint32_t* held, int32_t* stuck, void* stream);
int fn_constrain_advance(int32_t* tok_io, int tok_ld, int rows, int V, const FnConstrainParams* params_dev, const float* logits, int ld,
                         const int32_t* fallback, int fb_ld, const uint32_t* held_in, uint32_t* held_out, int32_t* fixed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Controllability metrics of decoded event tokens (attributes.py): rhythm density and note density per row (fn_event_attributes)
 * and the three scores of a fader sweep (fn_sweep_scores).  The reference measures through a MIDI file (test_class.py:124-139); the
 * part that decides the numbers is restated here in integers.  The reference's: the piano-roll fill (the vendored parse_pretty_midi,
 * polyphonic_event_based_v2.py:334-414), convert_pr_to_pitch_lst / pitch_lst_to_rhythm (:13-29, :140-158), get_classes
 * (test_class.py:59-70) and the calculate_* methods (:259-272, :308-321).  OURS: the step from tokens to timed notes - Magenta's
 * performance decoder was not at hand - and the beat grid, which pretty_midi estimates and which is fixed here to a first beat at 0
 * and 120 qpm.
 *
 * fn_event_attributes: tokens [rows][tok_ld] int32, `steps` columns used.  Parameters as read from device memory and clamped:
 * n_pitch to [0, 128], n_shift to [0, 4096], ticks_num to [1, 32768], ticks_den to [1, 256], beat_cells to [1, 64] (so that every n_cells fits
 * an int32); the other fields as they are.  A token e with vocab_size > 0 and e outside [0, vocab_size) belongs to no range.
 *   tokens -> notes   A row is read from column 0 up to, not including, the first token equal to eos (eos < 0: none), or to
 *           `steps`.  A clock t counts ticks of 10 ms from 0.  In this order: a token in [on_lo, on_lo + n_pitch) is the note-on of
 *           pitch p = e - on_lo: if p is open, its note is first closed at t (re-strike); then p is open with t0 = t.  A token in
 *           [off_lo, off_lo + n_pitch) is the note-off of p: the open note of p is closed at t1 = t; ignored if none is open.  A token
 *           in [shift_lo, shift_lo + n_shift) adds e - shift_lo + 1 to t.  Every other token (pad, velocity, ...) is skipped;
 *           velocity is not tracked (the attributes ask pr > 0 only, and every decodable velocity is >= 1).  The end of the row closes
 *           every open note at the final t.  A closed note with t1 == t0 is dropped.
 *   notes -> grid     One cell is ticks_num / ticks_den ticks (25/2: sixteenth notes at 120 qpm).  Onset cell
 *           a = (2*den*t0 + num) / (2*num) (round), end cell b = (den*t1) / num (floor), integer divisions in 64 bits.  t_last = the
 *           largest t1 of a kept note; n_cells = beat_cells * ((t_last*den) / (num*beat_cells) + 1).  Per pitch, in the order the
 *           notes close (polyphonic_event_based_v2.py:394-412): if 0 < a < n_cells and cell a-1 of p is set, it is cleared; if
 *           b < n_cells - 1 and cell b of p is set, b -= 1; cells [a, min(b, n_cells)) of p are set.  The clear happens even when the
 *           note then fills nothing.
 *   grid -> attributes  With S[c] the set of pitches set in cell c: notes[c] = |S[c]|; rhythm[c] = 0 if S[c] is empty, else 1 for
 *           c == 0, else 2 (hold) if S[c] is a subset of S[c-1], else 1 (onset).  onsets = #{c: rhythm[c] == 1}, total = sum notes[c].
 *           r_density = (float)((double)onsets / n_cells), n_density = (float)((double)total / n_cells);
 *           c_r = 0 if 10*onsets < 3*n_cells, 1 if 2*onsets < n_cells, else 2;  c_n = 0 if total <= 2*n_cells, 1 if 2*total <=
 *           7*n_cells, else 2 (get_classes' thresholds 0.3 / 0.5 and 2 / 3.5, decided on the integers).
 *   status  0; FN_ATTR_EMPTY: no kept note - n_cells 0, densities 0, classes 0 (the reference skips such a track);
 *           FN_ATTR_OVERFLOW: n_cells > cells_ld - n_cells is the true count, densities NaN, classes -1.
 * Outputs [rows] each: n_cells, status, r_density, n_density, c_r, c_n; optional (NULL: not wanted) rhythm, notes uint8
 * [rows][cells_ld]: cells [0, n_cells) of a row with status 0, 0 in every other cell up to cells_ld; nothing behind cells_ld.
 * One wavefront per row; dynamic LDS 4*steps + 512*ceil(cells_ld/32) bytes (<= 36 KB).
 * NULL tokens / params_dev / one of the six [rows] outputs: FN_E_NULL; rows < 1, steps outside [1, FN_ATTR_MAX_STEPS], cells_ld
 * outside [1, FN_ATTR_MAX_CELLS], tok_ld < steps: FN_E_SHAPE; both before any launch.
 *
 * fn_sweep_scores (test_class.py:169-175, 259-272, 308-321), everything in fp64: r, n [S][Vn] fp32 densities of S samples at Vn
 * fader values, status [S][Vn], values [Vn] fp64 on the device, which 0: rhythm is swept / 1: note.  A sample with any non-zero
 * status is left out; n_used counts the others.  x = the swept attribute / its std, o = the other one / its std (r_std, n_std):
 *   scores[0] consistency     = 1 - mean_v std_s(x)
 *   scores[1] restrictiveness = 1 - mean_s std_v(o)
 *   scores[2] monotonicity    = mean_s R2_s, R2_s = 1 - SS_res / SS_tot of the least-squares line of the UNSCALED swept density
 *                               against values (slope 0 when the values are all equal); R2_s = 1 where SS_tot == 0, which is what
 *                               LinearRegression().score gives for a flat response
 *   scores[3] variance        = mean_s std_v(x)                       (calculate_variance, :262-263; printed by nobody)
 * std is the population std about the mean.  n_used == 0: four NaN.  Order of the sums, so that a result does not depend on the
 * launch: over values ascending from 0.0; over samples in 16 partial sums - partial j takes the used samples s = j, j + 16, ...
 * ascending from 0.0 - combined as a[i] += a[i + h] for h = 8, 4, 2, 1.
 * One launch of one workgroup of 16 wavefronts.  NULL r / n / status / values / scores / n_used: FN_E_NULL; S outside
 * [1, FN_ATTR_MAX_SAMPLES], Vn outside [2, 64], which outside {0, 1}: FN_E_SHAPE; both before any launch.
 * ------------------------------------------------------------------------------------------ */
#define FN_ATTR_MAX_STEPS 1024
#define FN_ATTR_MAX_CELLS 2048
#define FN_ATTR_MAX_SAMPLES 4096
#define FN_ATTR_EMPTY 1
#define FN_ATTR_OVERFLOW 2
typedef struct FnAttrParams {        /* 48 bytes */
    int32_t on_lo, off_lo, n_pitch;  /* as FnConstrainParams */
    int32_t shift_lo, n_shift;       /* time-shift tokens [shift_lo, shift_lo+n_shift): shift_lo + k = k + 1 ticks */
    int32_t eos;                     /* -1: none */
    int32_t ticks_num, ticks_den;    /* ticks per cell */
    int32_t beat_cells;              /* cells per beat: n_cells is a whole number of beats */
    int32_t vocab_size;              /* <= 0: no cut */
    int32_t reserved[2];
} FnAttrParams;
int fn_event_attributes(const int32_t* tokens, int tok_ld, int rows, int steps, const FnAttrParams* params_dev, int32_t* n_cells, int32_t* status,
                        float* r_density, float* n_density, int32_t* c_r, int32_t* c_n, uint8_t* rhythm, uint8_t* notes, int cells_ld, void* stream);
int fn_sweep_scores(const float* r, const float* n, const int32_t* status, int S, int Vn, const double* values, int which, double r_std,
                    double n_std, double* scores, int32_t* n_used, void* stream);

/* ------------------------------------------------------------------------------------------
 * Event tokens <-> timed notes (notes.py, midi.py): fn_notes_from_tokens publishes the "tokens -> notes" step of fn_event_attributes,
 * with velocity; fn_tokens_from_notes is its inverse, the tokeniser (magenta_encode_midi over windows, ptb_v2.py:217-273).  The
 * reference's: the window cut (slice_midi, ptb_v2.py:60-92, made half-open here: the reference also keeps a note that starts exactly
 * at the window's end, as a zero-length one) and dropping a segment that does not fit (:264; here a status the caller filters by).
 * OURS, pinned against nothing of Magenta's: the walk from tokens to notes, the order of simultaneous events, and the velocity bins,
 * which follow Magenta's performance encoding as far as we know it.  Integers only.
 *
 * Parameters as read from device memory and clamped: on_lo, off_lo, n_pitch, shift_lo, n_shift, eos, vocab_size exactly as FnAttrParams
 * (n_pitch to [0, 128], n_shift to [0, 4096]); n_vel to [0, 128]; default_vel to [1, 127]; the other fields as they are.
 *   velocity  vstep = (127 + n_vel - 1) / n_vel (2 for 64 bins).  Bin k is velocity min(1 + k*vstep, 127); velocity v in [1, 127] is bin
 *           min((v - 1) / vstep, n_vel - 1).  n_vel == 0: velocity is neither read nor written.
 *
 * fn_notes_from_tokens: tokens [rows][tok_ld] int32, `steps` columns used -> notes [rows][notes_ld] FnNote, n_notes, t_end, status [rows].
 *   The walk is the "tokens -> notes" clause of fn_event_attributes word for word (the row's end at the first eos, re-strike, an ignored
 *   unmatched note-off, the row's end closing every open note at the final t, a dropped t1 == t0, the vocab_size cut), and one addition:
 *   the current velocity starts at default_vel, and a token that is in none of the note-on, note-off and time-shift ranges but in
 *   [vel_lo, vel_lo + n_vel) sets it to the velocity of bin e - vel_lo.  A note carries the velocity current at its note-on token.
 *   notes[r] holds the kept notes ascending by (t0, pitch) - unique, two kept notes of one pitch cannot share t0.  n_notes is the true
 *   count; when it exceeds notes_ld the first notes_ld notes of that order are written and status is FN_NOTES_OVERFLOW; n_notes == 0:
 *   FN_NOTES_EMPTY; else 0.  Entries [n_notes, notes_ld) are zeroed, nothing is written behind notes_ld.  t_end is the final t.
 *   notes_ld = steps never overflows (every note has its own note-on token).
 *   One wavefront per row; dynamic LDS 9*steps + 8*P bytes, P = the power of two >= steps (<= 17 KB).
 *   NULL tokens / params_dev / notes / n_notes / t_end / status: FN_E_NULL; rows < 1, steps outside [1, FN_ATTR_MAX_STEPS], tok_ld < steps,
 *   notes_ld < 1: FN_E_SHAPE; both before any launch.
 *
 * fn_tokens_from_notes: notes [n_total] FnNote in any order, spans [rows] FnNoteSpan -> tokens [rows][tok_ld] (`steps` columns written),
 * n_tokens, n_kept, status [rows].  Per row with span (first, count, t_lo, t_hi), differences in 64 bits:
 *   1. count is clamped to [0, FN_NOTES_MAX].  The span is notes[first + k], k < count; a k with first + k outside [0, n_total) is no note.
 *   2. t_hi is clamped to [t_lo, t_lo + FN_NOTES_MAX_TICK].
 *   3. A note is kept iff 0 <= pitch < n_pitch, t_lo <= t0 < t_hi and min(t1, t_hi) > t0.
 *   4. A kept note has the events (t0 - t_lo, ON) and (min(t1, t_hi) - t_lo, OFF); its vel is clamped to [1, 127].
 *   5. The 2 * n_kept events are ordered ascending by (tick, OFF before ON, pitch, k).  OFF first: a note that ends where the next one of
 *      its pitch begins survives the decoder's re-strike rule.
 *   6. The stream starts at clock 0 with no current bin.  Per event, with g = tick - clock: g / n_shift tokens shift_lo + n_shift - 1;
 *      if g % n_shift, the token shift_lo + g % n_shift - 1; for an ON with n_vel > 0 whose bin differs from the current one, vel_lo + bin
 *      (which becomes the current one); then on_lo + pitch or off_lo + pitch.  After the last event eos, if add_eos != 0 and eos >= 0
 *      (a row without a kept note is then eos alone).
 *   7. n_tokens is the stream's true length (eos included; at most 2^22 + 3 * 1024 + 1).  The first min(n_tokens, steps) tokens are written,
 *      the columns from there up to `steps` hold pad; nothing is written behind `steps`.
 *   8. status FN_NOTES_OVERFLOW if n_tokens > steps (the reference drops such a segment), else FN_NOTES_EMPTY if n_kept == 0, else 0.
 *   9. n_shift == 0: time cannot be written; the result is unspecified (here: no time-shift token), every access stays in bounds.
 *   Decoding a row with status 0 gives back the kept notes, times relative to t_lo and velocities snapped to their bins, except where two
 *   kept notes of one pitch overlap or coincide: the decoder's re-strike rule ends the earlier one at the later one's start, and the
 *   later one at the first note-off that follows.
 *   One wavefront per row; static LDS 8.5 KB (1024 event keys of tick:23 | kind:1 | pitch:7 | k:10 in 64 bits, 512 bins).
 *   NULL spans / params_dev / tokens / n_tokens / n_kept / status, or NULL notes with n_total > 0: FN_E_NULL; rows < 1, steps outside
 *   [1, FN_ATTR_MAX_STEPS], tok_ld < steps, n_total < 0: FN_E_SHAPE; both before any launch.
 *
 * fn_notes_stitch (transfer.py): S windows of V pieces back into V note lists - the step from decoded windows to a piece.  OURS; the
 * reference stops at one window.  dec [S*V] rows of FnNote at a stride of dec_rs notes, row = j*V + v, dec_ld slots of a row in use,
 * with dec_n and dec_end [S*V] (n_notes and t_end of fn_notes_from_tokens); src [n_total] FnNote and spans [S] FnNoteSpan as the
 * tokeniser takes them; mode [S*V] int32 -> out [V][out_ld] FnNote, win_first [V][S + 1], out_n, status [V].  Everything but the
 * sizes is read from DEVICE memory.  Per window j of piece v, with spans[j] = (first, count, t_lo, t_hi), all arithmetic in 64 bits:
 *   1. W = t_hi - t_lo clamped to [0, FN_NOTES_MAX_TICK].
 *   2. mode 0, the source passes through: the notes are src[first + k], 0 <= k < count; a k with first + k outside [0, n_total) is no
 *      note; count is NOT capped at FN_NOTES_MAX.  A note is kept iff t_lo <= t0 < t_lo + W, and is written unchanged: absolute
 *      times, t1 not cut.
 *   3. mode 1, decoded and clipped: the notes are dec[row][k], k < dec_n[row] clamped to [0, dec_ld].  A note is kept iff
 *      0 <= t0 < W, and is written as (t_lo + t0, t_lo + min(t1, W), pitch, vel).
 *   4. mode 2, decoded and fitted: when dec_end[row] > W, first t0 <- floor(t0 * W / dec_end) and t1 <- max(t0 + 1, floor(t1 * W /
 *      dec_end)) (floor towards minus infinity; the products reach 2^53), then clause 3; otherwise mode 2 is clause 3.
 *   5. Any other mode: the window holds nothing.
 *   6. In every mode a note whose written t1 <= t0 is dropped, so is one with pitch outside [0, 128) and one whose written times
 *      leave int32; vel is clamped to [1, 127].
 *   7. out[v] holds the kept notes of window 0, then of window 1, ...; inside a window the input order.  Nothing is sorted: the result
 *      ascends by t0 when the spans are ascending and disjoint and the windows' notes ascend, which is the caller's affair.
 *   8. win_first[v][j] is the number of kept notes in front of window j, win_first[v][S] the total: true counts, not clamped to out_ld.
 *      out_n[v] = min(total, out_ld); the first out_n notes of the order are written, entries [out_n, out_ld) are zeroed, nothing is
 *      written behind out_ld.  status FN_NOTES_OVERFLOW if total > out_ld, else FN_NOTES_EMPTY if total == 0, else 0.
 *   Three launches, ordered by their boundaries alone (no workgroup waits for another): one wavefront per (window, piece) counts its
 *   kept notes with a ballot into win_first; one wavefront per piece turns the counts into offsets, 256 windows a pass; one wavefront
 *   per (window, piece) repeats the walk and writes every kept note at offset + the lanes' prefix popcount as one 16-byte store,
 *   and zeroes its share of the tail.  No LDS.
 *   NULL dec / dec_n / dec_end / spans / mode / out / win_first / out_n / status, or NULL src with n_total > 0: FN_E_NULL; S < 1, V < 1,
 *   dec_ld < 1, dec_rs < dec_ld, out_ld < 1, n_total < 0: FN_E_SHAPE; dec, src or out not 16-byte aligned: FN_E_ALIGN; S >
 *   FN_STITCH_MAX_S, V > FN_STITCH_MAX_V, out_ld > FN_STITCH_MAX_OUT, or S * max(n_total, dec_ld) >= 2^31 (a count could leave
 *   int32): FN_E_UNSUPPORTED; all before any launch.
 * ------------------------------------------------------------------------------------------ */
#define FN_NOTES_MAX 512
#define FN_NOTES_MAX_TICK (1 << 22)
#define FN_NOTES_EMPTY 1
#define FN_NOTES_OVERFLOW 2
typedef struct FnNote { int32_t t0, t1, pitch, vel; } FnNote;                /* 16 bytes; ticks of 10 ms; pitch = offset in the note range; vel 1..127 */
typedef struct FnNoteSpan { int32_t first, count, t_lo, t_hi; } FnNoteSpan;  /* 16 bytes */
typedef struct FnNoteParams {        /* 64 bytes, read from DEVICE memory like FnAttrParams, so a captured graph serves any setting */
    int32_t on_lo, off_lo, n_pitch, shift_lo, n_shift, eos, vocab_size;      /* as FnAttrParams */
    int32_t vel_lo, n_vel;           /* velocity tokens [vel_lo, vel_lo + n_vel) */
    int32_t default_vel;             /* the velocity before the first velocity token (100) */
    int32_t pad;                     /* written behind the end of a tokenised row (0) */
    int32_t add_eos;                 /* != 0 and eos >= 0: the tokeniser ends every row with eos */
    int32_t reserved[4];
} FnNoteParams;
int fn_notes_from_tokens(const int32_t* tokens, int tok_ld, int rows, int steps, const FnNoteParams* params_dev, FnNote* notes, int notes_ld,
                         int32_t* n_notes, int32_t* t_end, int32_t* status, void* stream);
int fn_tokens_from_notes(const FnNote* notes, int n_total, const FnNoteSpan* spans, int rows, const FnNoteParams* params_dev, int32_t* tokens,
                         int tok_ld, int steps, int32_t* n_tokens, int32_t* n_kept, int32_t* status, void* stream);
#define FN_STITCH_MAX_S (1 << 16)
#define FN_STITCH_MAX_V 64
#define FN_STITCH_MAX_OUT (1 << 24)
int fn_notes_stitch(const FnNote* dec, int dec_rs, int dec_ld, const int32_t* dec_n, const int32_t* dec_end, const FnNote* src, int n_total,
                    const FnNoteSpan* spans, int S, int V, const int32_t* mode, FnNote* out, int out_ld, int32_t* win_first, int32_t* out_n,
                    int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Latent-side work in front of a decode (latent.py): a draw from the mixture prior and a mix of two pieces' latents.  OURS; the reference has
 * the prior's tables (gmm_model.py:151-183) and the class posterior (approx_qy_x, :194-218) but neither samples the one nor interpolates.  The
 * text below is the specification.  Both entry points are additive: fn_version() stays 6.
 *
 * fn_latent_draw: z ~ N(mu_lk[k], (tau * exp(lv_lk[k] / 2))^2) for `rows` rows, up to FN_DRAW_MAX_JOBS jobs in ONE launch (jobs is a HOST array,
 * read by value; the 32 bytes of params_dev are read from DEVICE memory, so a captured graph serves any seed).  The usual two jobs write z_r into
 * columns [0, Z) and z_n into columns [Z, 2Z) of the decode's own (rows, 2Z+24) rows: a job writes z[b*z_ld + j] for j in [0, Z) and touches no
 * other column.  For job s, row b, column j, with q = j / 4:
 *   1. w[0..3] = Philox4x32-10(counter = (b, (stream_id << 16) | q, offset_lo, offset_hi), key = (seed_lo, seed_hi)), the rounds of fn_vocab_sample
 *      (counter 0, key 0: 6627e8d5 e169c58d bc57ac4c 9b00dbd8).
 *   2. Box-Muller, two pairs per quad.  For h = 0, 1: ua = ((w[2h] >> 8) + 1) * 2^-24 in (0, 1], ub = (w[2h+1] >> 8) * 2^-24 in [0, 1),
 *      r = sqrtf(-2 logf(ua)), n[4q+2h] = r * cospif(2 ub), n[4q+2h+1] = r * sinpif(2 ub) - cos / sin of pi x, as 2 ub is exact in fp32.  A last
 *      quad with fewer than 4 columns drops the rest.  |n| <= sqrt(48 ln 2) = 5.77.
 *   3. The component: k = min(comp[b], K - 1) where comp is given and comp[b] >= 0; otherwise drawn uniformly from the row's own counter
 *      (b, (stream_id << 16) | 0xFFFF, offset_lo, offset_hi): k = ((w'[0] >> 8) * K) >> 24 in 64-bit integers, which is floor(u * K) for
 *      u = (w'[0] >> 8) * 2^-24 without a rounding.  comp_out[b] = k when given.
 *   4. eps = n[j];  z[b*z_ld + j] = mu_lk[k][j] + (tau * expf(0.5f * lv_lk[k][j])) * eps;  eps_out[b*Z + j] = eps when given.
 * tau comes from memory and is clamped to [0, FLT_MAX], NaN -> 1; tau = 0 gives the component mean itself.  A row's numbers depend on (b, j,
 * stream_id, seed, offset) only - not on rows, n_jobs or the launch geometry.  One thread per (row, quad); no LDS.
 *   NULL jobs, params_dev, or a job's mu_lk, lv_lk or z: FN_E_NULL (answered first);  n_jobs outside [1, FN_DRAW_MAX_JOBS]: FN_E_COUNT;  rows < 1,
 *   Z < 1, z_ld < Z, a K < 1, a stream_id outside [0, 65535): FN_E_SHAPE;  Z > FN_DRAW_MAX_Z, a K > FN_DRAW_MAX_K, rows * ceil(Z / 4) >= 2^31:
 *   FN_E_UNSUPPORTED;  a pointer that is not 4-byte aligned: FN_E_ALIGN;  in this order, all before any launch.
 *
 * fn_latent_mix: out row i*P + p (row stride out_ld >= D) is the mix of a[i] and b[i] (row stride ab_ld >= D) at tt = t[p], or t[i*P + p] with
 * t_per_pair != 0; a, b, t in DEVICE memory, segs a HOST array read by value.  tt is any finite value (outside [0, 1]: extrapolation).  The
 * segments are disjoint slices [off, off + len) of [0, D), each slice of each pair mixed on its own; columns in no segment are written as a's,
 * columns [D, out_ld) are not touched.  out must not overlap a or b.  Per segment mode:
 *   FN_MIX_LERP   out = fmaf(tt, b, (1.0f - tt) * a)
 *   FN_MIX_STEP   out = tt < 0.5f ? a : b                                (the chroma columns: halfway between two keys is not a key)
 *   FN_MIX_SLERP  saa = sum a^2, sbb = sum b^2, sab = sum ab over the slice in fp32; na = sqrtf(saa), nb = sqrtf(sbb);
 *                 c = clamp((float)((double)sab / sqrt((double)saa * (double)sbb)), -1, 1) - the cosine sab / (na * nb) with product, root and quotient
 *                 in fp64 and ONE rounding, so that a == b gives c = 1 and a == -b gives c = -1 exactly (the fp32 product na * nb exceeds saa by an
 *                 ulp for about every fourth vector, and the angle of a vector with itself would come out as 4.9e-4);  w = acosf(c), s = sinf(w);
 *                 na == 0, nb == 0, s < FN_MIX_MIN_SIN or s NaN: the slice of this pair is mixed as FN_MIX_LERP; otherwise
 *                 wa = sinf((1.0f - tt) * w) / s, wb = sinf(tt * w) / s, out = fmaf(wb, b, wa * a)   (the raw vectors, as MusicVAE-style models do)
 * omega_out[i*n_segs + g], when given: w of segment g; 0 where the segment is not FN_MIX_SLERP, -1 where the fallback was taken.  In every mode
 * tt == 0 returns a's values and tt == 1 b's exactly (sinf(w) / s is s / s).  The sums are fp32, lane-strided and reduced by an xor butterfly
 * inside one wavefront; one wavefront owns a pair and loops over its P points; no atomics, no LDS, no hand-over between workgroups.
 *   NULL a, b, t, segs or out: FN_E_NULL;  n_segs outside [1, FN_MIX_MAX_SEGS]: FN_E_COUNT;  pairs, D or P < 1, ab_ld or out_ld < D, a segment
 *   with len < 1, one that leaves [0, D), overlaps another or has an unknown mode: FN_E_SHAPE;  pairs * P >= 2^31: FN_E_UNSUPPORTED;  a, b, t, out
 *   or omega_out not 4-byte aligned: FN_E_ALIGN;  in this order, all before any launch.
 * ------------------------------------------------------------------------------------------ */
#define FN_DRAW_MAX_JOBS 4
#define FN_DRAW_MAX_Z 4096
#define FN_DRAW_MAX_K 1024
typedef struct FnDrawParams {      /* 32 bytes, read from DEVICE memory like FnSampleParams */
    uint32_t seed_lo, seed_hi;     /* the Philox key: a 64-bit seed                                                  */
    uint32_t offset_lo, offset_hi; /* counter words 2, 3: a 64-bit offset                                            */
    float tau;                     /* scale of the component's sigma; NaN -> 1, clamped to [0, FLT_MAX]              */
    int32_t reserved[3];           /* 0                                                                              */
} FnDrawParams;
typedef struct FnDrawJob {         /* host memory, by value, like FnBeamGatherJob */
    const float *mu_lk, *lv_lk;    /* [K][Z]                                                                         */
    const int32_t* comp;           /* [rows] or NULL                                                                 */
    float* z;                      /* row stride z_ld (>= Z)                                                         */
    float* eps_out;                /* [rows][Z] or NULL                                                              */
    int32_t* comp_out;             /* [rows] or NULL                                                                 */
    int32_t K, stream_id;          /* stream_id in [0, 65535)                                                        */
} FnDrawJob;
int fn_latent_draw(const FnDrawJob* jobs, int n_jobs, int rows, int Z, int64_t z_ld, const FnDrawParams* params_dev, void* stream);
#define FN_MIX_LERP 0
#define FN_MIX_SLERP 1
#define FN_MIX_STEP 2
#define FN_MIX_MAX_SEGS 4
#define FN_MIX_MIN_SIN 1e-4f
typedef struct FnMixSeg { int32_t off, len, mode, reserved; } FnMixSeg;   /* host memory, by value */
int fn_latent_mix(const float* a, const float* b, int64_t ab_ld, int pairs, int D, const float* t, int P, int t_per_pair,
                  const FnMixSeg* segs, int n_segs, float* out, int64_t out_ld, float* omega_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Importance-weighted log-likelihood (likelihood.py): S draws from the posterior q(z|x) per piece with their densities, and the reduction of the
 * S log-weights per piece (Burda et al., "Importance Weighted Autoencoders").  OURS; the reference reports one reparameterised sample and the
 * analytic KL.  The text below is the specification.  Both entry points are additive: fn_version() stays 6.  LOG_2PI = log(2 pi) in fp64.
 *
 * fn_posterior_draw: S samples of q(z|x) = N(mu, (tau sigma)^2) for each of B source rows, up to FN_DRAW_MAX_JOBS jobs in ONE launch (jobs is a HOST
 * array, read by value; params_dev is fn_latent_draw's FnDrawParams in DEVICE memory).  The usual two jobs (stream 0 rhythm, stream 1 note) write
 * z_r | z_n into the teacher-forced decoder's own (B*S, 2Z+24) latent rows: sample s of source row b is row i = b*S + s, a job writes
 * z[i*z_ld + j] for j in [0, Z) and touches no other column.  For job e, source row b, sample s, column j, with q = j / 4:
 *   1. eps is the normal of fn_latent_draw's steps 1-2 from the counter (b, (stream_id << 16) | q, lo(offset + s), hi(offset + s)) under the key
 *      seed; offset + s is a 64-bit add that wraps.  Sample (b, s) is therefore, bit for bit, row b of fn_latent_draw's eps_out at offset + s, and
 *      depends on neither B, S, n_jobs nor the launch geometry.  (One device function serves both entry points.)
 *   2. sg = tau * expf(pre[b][Z + j]) in fp32 (pre [B][2Z]: mu | v, sigma = expf(v), exactly as fn_latent_fwd reads it; tau from params_dev, clamped
 *      as fn_latent_draw clamps it);  z[i][j] = pre[b][j] + sg * eps;  eps_out[i*Z + j] = eps when given.
 *   3. The densities, functions of the STORED fp32 values z, mu, sg, mu_lk, lv_lk evaluated in fp64 - at the stored z, not at eps: the weight must
 *      be the density ratio at the point the decoder sees.
 *        logq[i] = sum_j -0.5 * (d*d + LOG_2PI) - log((double)sg),  d = ((double)z - (double)mu) / (double)sg
 *        ll_k    = sum_j -0.5 * (dz*dz * exp(-(double)lv_lk[k][j]) + (double)lv_lk[k][j] + LOG_2PI) + log(1.0 / K),  dz = (double)z - (double)mu_lk[k][j]
 *                  (the component log-likelihood of approx_qy_x, gmm_model.py:204-215, as fn_latent_fwd forms it)
 *        logp[i] = m + log(sum_k exp(ll_k - m)),  m = max_k ll_k,  k ascending
 *      Every sum over j: lane l of 64 adds its terms j = l, l + 64, ... ascending from 0.0 (a term is the whole summand, -log sg included), then
 *      s[l] += s[l ^ o] for o = 32, 16, 8, 4, 2, 1.
 * sg == 0 or a non-finite input gives unspecified values for that row; every access stays in bounds.  One wavefront per (b, s) row, blockIdx.y the
 * job; no LDS, no atomics, no hand-over between workgroups; plain dword-wide vector stores, so a job's columns may start at any column of a wider row.
 *   NULL jobs, params_dev, or a job's pre, mu_lk, lv_lk, z, logq or logp: FN_E_NULL (answered first);  n_jobs outside [1, FN_DRAW_MAX_JOBS]:
 *   FN_E_COUNT;  B, S or Z < 1, z_ld < Z, a K < 1, a stream_id outside [0, 65535): FN_E_SHAPE;  a K > FN_POST_MAX_K (fn_latent_fwd's limit),
 *   Z > FN_DRAW_MAX_Z, B * S >= 2^31: FN_E_UNSUPPORTED;  a float pointer (params_dev included) that is not 4-byte aligned, logq or logp not 8-byte
 *   aligned: FN_E_ALIGN;  in this order, all before any launch.
 *
 * fn_iw_reduce: nll_tb is fn_out_head_f32's nll_rows of the B*S decoder rows (step t, row i at nll_tb[t*nll_ld + i]); t0, t1 [B] give the scored
 * span [t0[b], t1[b]) of source row b, clamped to [0, T] on the device, or are both NULL for [0, T); logp_z / logq_z hold the densities of latent e
 * at + e*lat_stride, [B*S] each (fn_posterior_draw's outputs).  One launch, two passes over a piece's samples.  Per row i = b*S + s:
 *   recon = -(sum_t (double)nll), over the span, t ascending from 0.0 (an empty span: 0);
 *   lw[i] = recon + sum_e (logp_e[i] - logq_e[i]), each difference formed first, then added e ascending.  lw [B*S] is a required output: the
 *   per-sample log-weight, and the second pass's input.
 * Per source row b, lane l of 64 taking s = l, l + 64, ... ascending (sums from 0.0, the maximum from -inf), then the xor butterfly of offsets 32 .. 1:
 *   m = max_s lw;  W1 = sum exp(lw - m);  W2 = sum exp(lw - m)^2
 *   out[b][0] = m + log(W1) - log((double)S)      the importance-weighted bound
 *   out[b][1] = (sum_s lw) / S                    the one-sample ELBO, averaged
 *   out[b][2] = W1*W1 / W2                        the effective sample size, in [1, S]
 *   out[b][3] = (sum_s recon) / S
 *   out[b][4+e] = (sum_s (logq_e - logp_e)) / S   the Monte-Carlo KL of latent e
 * m == -inf gives out[b][0] = out[b][1] = -inf and out[b][2] = 0.  A NaN gives unspecified values, in bounds.  One wavefront per b: the first
 * pass writes lw and finds m, the second re-reads lw for W1 and W2 - a lane re-reads only the lw values it wrote itself, and consecutive s are
 * consecutive addresses of nll_tb, so the loads coalesce.  No LDS, no atomics.
 *   NULL nll_tb, logp_z, logq_z, lw or out, one of t0 / t1 without the other: FN_E_NULL;  n_lat outside [1, FN_IW_MAX_LAT]: FN_E_COUNT;  B, S or
 *   T < 1, nll_ld < B*S, lat_stride < B*S, out_ld < FN_IW_COLS + n_lat: FN_E_SHAPE;  B*S >= 2^31: FN_E_UNSUPPORTED;  nll_tb, t0 or t1 not 4-byte,
 *   logp_z, logq_z, lw or out not 8-byte aligned: FN_E_ALIGN;  in this order, all before any launch.
 * ------------------------------------------------------------------------------------------ */
#define FN_POST_MAX_K 8
typedef struct FnPostJob {          /* host memory, by value, like FnDrawJob */
    const float* pre;               /* [B][2Z]: mu | v, sigma = expf(v), exactly as fn_latent_fwd reads it   */
    const float *mu_lk, *lv_lk;     /* [K][Z] prior tables                                                   */
    float* z;                       /* row i = b*S + s, row stride z_ld (>= Z); writes columns [0, Z) only   */
    float* eps_out;                 /* [B*S][Z] or NULL                                                      */
    double *logq, *logp;            /* [B*S] each, required                                                  */
    int32_t K, stream_id;           /* K in [1, 8] (fn_latent_fwd's limit); stream_id in [0, 65535)          */
} FnPostJob;
int fn_posterior_draw(const FnPostJob* jobs, int n_jobs, int B, int S, int Z, int64_t z_ld,
                      const FnDrawParams* params_dev, void* stream);
#define FN_IW_MAX_LAT 4
#define FN_IW_COLS 4        /* iwae, elbo, ess, recon; then one kl column per latent */
int fn_iw_reduce(const float* nll_tb, int T, int64_t nll_ld,           /* nll of step t, row i at nll_tb[t*nll_ld + i]: fn_out_head_f32's nll_rows */
                 const int32_t* t0, const int32_t* t1,                 /* [B] span [t0, t1) of source row b, or both NULL = [0, T)                 */
                 const double* logp_z, const double* logq_z, int n_lat, int64_t lat_stride,   /* latent e at + e*lat_stride, [B*S] each            */
                 int B, int S, double* lw, double* out, int out_ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * Latent disentanglement report (disentangle.py): which posterior dimension holds which attribute - mutual information gap (Chen et al.), separated
 * attribute predictability (Kumar et al.), modularity (Ridgeway & Mozer), the R^2 interpretability score (Adel et al.) and Spearman's rho - from six
 * kernels over a code matrix and a factor matrix.  OURS: the reference's run_through_gmm copies every batch to the host and stops there.  The text
 * below is the specification; csrc/host/disentangle_host.h has the argument checks (shared with the device entry points) and the host twins.  The six
 * entry points are additive: fn_version() stays 6.
 *
 * Limits: 1 <= N <= FN_DIS_MAX_N rows, 1 <= P <= FN_DIS_MAX_D columns, 1 <= Q, A <= FN_DIS_MAX_A factor columns, 1 <= bins <= FN_DIS_MAX_BINS,
 * a cardinality in [0, FN_DIS_MAX_BINS].  In every entry point: a required pointer NULL: FN_E_NULL;  a size < 1, a row stride below the width,
 * n_pad < N, a cardinality outside [0, 64]: FN_E_SHAPE;  a size above its limit: FN_E_UNSUPPORTED;  a float or int32 pointer not 4-byte, a double
 * pointer not 8-byte aligned: FN_E_ALIGN;  in this order, all before any launch.  A matrix is fp32, element (i, c) at x[i*ld + c], ld >= P: a column
 * slice of a wider tensor works.  A "column-major image" holds element (i, c) at img[c*n_pad + i], n_pad >= N; entries i >= N are not touched.
 *
 * fn_column_range: lo[c] = min_i x[i][c], hi[c] = max_i x[i][c] over the FINITE entries, as fp32: exact, so no order is stated; a zero is returned as
 * +0.0f whatever its sign (the kernel compares x + 0.0f).  status[c] = FN_DIS_NONFINITE when the column holds a NaN or an infinity, else 0: the call
 * initialises status (and lo = +inf, hi = -inf, which is what a column without a finite entry keeps).  Workgroups of 4 x 64 threads own 64 columns and
 * FN_DIS_RANGE_CHUNK rows and close with integer atomic min / max on the ordered bit patterns.
 *
 * fn_bin_columns: the bin image, uint8, column-major.  card is HOST memory, [P] int32, read by value, or NULL (every column continuous; required NULL
 * for P > FN_DIS_MAX_A).  card[c] == 0, a continuous column, in fp64 with every operation rounded once and none fused:
 *     t = ((double)x - (double)lo[c]) / ((double)hi[c] - (double)lo[c]) * (double)bins
 *     bin = (int)t for 0 <= t < bins;  bins - 1 for t >= bins (x == hi lands there);  0 for t < 0, for a NaN t and where hi[c] == lo[c]
 * card[c] == C >= 1, a discrete column of the levels 0 .. C-1 stored as floats: bin = (int)x where x is an integer in [0, C); otherwise bin = 0 and
 * FN_DIS_BAD_LEVEL is OR-ed into status[c].  status is not initialised here: hand fn_column_range's over, or zeros.
 *
 * fn_joint_hist: counts[d][a][bz][bf], int32, [D][A][64][64] (the inner extents are padded to 64, so a pair's table is 16 KB): the number of rows i
 * with bz_img[d*ldz + i] == bz and bf_img[a*ldf + i] == bf.  A bin value above 63 counts as value & 63.  The call zeroes counts itself, then one
 * workgroup per (chunk of FN_DIS_HIST_CHUNK rows, a, d) counts in a 16 KB LDS table with integer atomics and adds its non-zero cells to global memory
 * with integer atomics: order-free, so the counts are exact whatever the geometry.  D * A <= 65536 pairs.
 *
 * fn_column_ranks: the mid-rank of every element within its column, rank[i] = #{j : x[j] < x[i]} + (#{j : x[j] == x[i]} + 1) / 2, as fp32 into a
 * column-major image (2 * rank is an integer <= 2N + 1 < 2^24, so the value is exact).  -0.0 == 0.0 is a tie.  The counting form: N^2 compares per
 * column.  A workgroup of 256 threads owns FN_DIS_RANK_ROWS = 1024 rows of one column, four per thread in registers, and walks the column in tiles of
 * FN_DIS_RANK_TILE = 1024 values staged in LDS (4 KB; every lane reads the same four values at a time, a broadcast); a tile's tail is padded with
 * NaN, which is neither below nor equal to anything.  No sort, no hand-over between workgroups.  A NaN in the column gets rank 0.5 and is counted by
 * nobody; an infinity ranks like any value.
 *
 * fn_column_corr: X (N x P) and Y (N x Q, Q <= FN_DIS_MAX_A) with a generic row and column stride each (element (i, c) at x[i*rs + c*cs]; strides in
 * floats, >= 1), so one kernel serves the raw codes (row-major) and the ranks (column-major).  In fp64, two passes, one wavefront per X column:
 *     mean_x[p] = (sum_i (double)x[i][p]) / N,   mean_y[q] likewise;
 *     ss_x[p] = sum_i dx*dx,  ss_y[q] = sum_i dy*dy,  cross[p][q] = sum_i dx*dy,   dx = (double)x[i][p] - mean_x[p],  dy = (double)y[i][q] - mean_y[q]
 * at the STORED means.  Every sum: lane l of 64 adds its rows i = l, l + 64, ... ascending from 0.0 (a term is the whole product, rounded before it is
 * added: nothing is fused), then s[l] += s[l ^ o] for o = 32, 16, 8, 4, 2, 1 (fn_wave_sum_f64).  Every wavefront recomputes the Y sums in this same
 * order; the wavefront of column 0 stores them.
 *
 * fn_mi_scores: from counts, per (d, a) pair, one wavefront per pair, fp64, natural logarithms.  With n = counts[bz][bf], r[bz] = sum_bf n and
 * c[bf] = sum_bz n (integers) and T = sum n (the number of rows counted):
 *     out[pair][0] = I   = sum over the cells with n > 0 of (n / T) * log((double)(n * T) / (double)(r[bz] * c[bf]))      (both products exact: < 2^53)
 *     out[pair][1] = H_z = -sum over r[bz] > 0 of (r / T) * log(r / T),   out[pair][2] = H_f = -sum over c[bf] > 0 of (c / T) * log(c / T)
 *     hits[pair] = sum_bz max_bf n, an integer: the histogram classifier's count of rows it gets right
 * I: lane l owns column bf = l and adds its terms bz = 0 .. 63 ascending from 0.0 (an empty cell adds nothing), then the xor butterfly.  H_z: lane l
 * owns row l, H_f: lane l owns column l, one term each (0.0 for an empty one), then the butterfly; the sign is applied last.  T == 0 gives zeros.
 *
 * fp64 bounds against a float64 restatement in the same orders (tests/helpers_disentangle.py): |device - restatement| <= k * 2^-52 * sum |term|,
 * k counting the roundings on the longest path, each side erring by at most half of it:
 *     means:               ceil(N / 64) lane adds + 6 butterfly adds + 1 division                             k = ceil(N / 64) + 7
 *     ss, cross:           the two differences and the product of a term (3) + ceil(N / 64) + 6 adds          k = ceil(N / 64) + 9
 *     I:                   the product of a term (1) + 2 for its logarithm (one ulp = 2 * 2^-53) + 64 + 6     k = 73
 *     H_z, H_f:            1 + 2 + 1 lane add + 6                                                              k = 10
 * The quotients n / T and (n * T) / (r * c) are single IEEE divisions of exact integers: the same bits on every side, so they add nothing.
 * ------------------------------------------------------------------------------------------ */
#define FN_DIS_MAX_N (1 << 22)
#define FN_DIS_MAX_D 4096
#define FN_DIS_MAX_A 16
#define FN_DIS_MAX_BINS 64
#define FN_DIS_RANGE_CHUNK 1024   /* rows per workgroup of fn_column_range */
#define FN_DIS_HIST_CHUNK 4096    /* rows per workgroup of fn_joint_hist   */
#define FN_DIS_RANK_ROWS 1024
#define FN_DIS_RANK_TILE 1024
#define FN_DIS_NONFINITE 1        /* status bits */
#define FN_DIS_BAD_LEVEL 2
#define FN_DIS_MI_COLS 3          /* I, H_z, H_f */
int fn_column_range(const float* x, int64_t ld, int N, int P, float* lo, float* hi, int32_t* status, void* stream);
int fn_bin_columns(const float* x, int64_t ld, int N, int P, const float* lo, const float* hi, const int32_t* card_host, int bins, uint8_t* img,
                   int64_t n_pad, int32_t* status, void* stream);
int fn_joint_hist(const uint8_t* bz_img, int64_t ldz, int D, const uint8_t* bf_img, int64_t ldf, int A, int N, int32_t* counts, void* stream);
int fn_column_ranks(const float* x, int64_t ld, int N, int P, float* ranks, int64_t n_pad, void* stream);
int fn_column_corr(const float* X, int64_t x_rs, int64_t x_cs, int P, const float* Y, int64_t y_rs, int64_t y_cs, int Q, int N, double* mean_x,
                   double* ss_x, double* mean_y, double* ss_y, double* cross, void* stream);
int fn_mi_scores(const int32_t* counts, int pairs, double* out, int32_t* hits, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reconstruction report (report.py, epochs.evaluation_phase): what the reference's evaluation_phase() computes behind its loss terms
 * (trainer_gmm.py:470-610) - the accuracies.  The reference's: `torch.argmax(a, dim=-1)` (:546) and the per-sample loop of acc() with its
 * np.trim_zeros cut (:549-565).  OURS: the negative log-likelihood and the rank of the target per token, which re-ranking decoded hypotheses
 * and top-k accuracy need and the reference does not report.  Both entry points are additive: fn_version() stays 6.
 *
 * fn_token_score (replaces trainer_gmm.py:546 `torch.argmax(a, dim=-1)` on a materialised (B, T, V) tensor): row (b, t) starts at
 * x + b*stride_b + t*stride_t (strides in floats) and has V valid floats, 1 <= V <= FN_SAMPLE_MAX_V; nothing behind them is read, every logit
 * is read once and nothing of width V is written.  One signature serves the train forward's time-major logits [T*B][ld] (stride_t = B*ld,
 * stride_b = ld), a decode's logp (Bi, steps, V) and the attribute decoders' logp_bt [B][Tr][Cc] (V = Cc).  target [B][tgt_ld] or NULL; the
 * outputs pred, nll, rank [B][out_ld], each optional.  Per row, with tg = target[b][t] clamped to [0, V) as fn_token_sort clamps:
 *   pred[b][t] = the first-index argmax of the row, by comparisons only: fn_vocab_argmax's token on the same floats;
 *   nll[b][t]  = lse - x[tg] in the arithmetic of fn_vocab_logsoftmax: mx = max x; s = sum expf(x - mx), lane l of 64 adding its e = l, l + 64,
 *                ... ascending from 0.0f, then s[l] += s[l ^ o] for o = 32 .. 1; lse = mx + logf(s);
 *   rank[b][t] = #{j : x[j] > x[tg] or (x[j] == x[tg] and j < tg)}: an exact integer, 0 = the target is the argmax.
 * A -inf logit is legal; a target whose logit is -inf has nll = +inf.  A row of only -inf, or a row that holds a NaN, gives unspecified
 * values (every access stays in bounds).  One wavefront per row, 4 rows per workgroup, the row in registers.
 * x NULL, pred, nll and rank all NULL, nll or rank without target: FN_E_NULL; B, T < 1, V outside [1, FN_SAMPLE_MAX_V], out_ld < T,
 * tgt_ld < T with a target: FN_E_SHAPE; both before any launch.
 *
 * fn_match_rows (replaces the loop of acc(), trainer_gmm.py:549-565): pred [rows][pred_ld], target [rows][tgt_ld], T columns used.
 *   trim != 0  the reference's quirk, kept exactly: lead = the number of leading zeros of the target row, len = (last non-zero) + 1 - lead
 *              (np.trim_zeros trims both ends), and the comparison is pred[j] == target[lead + j] for j < len - the reference cuts `a` from
 *              its start (:556) but `b` from its first non-zero (:555).
 *   trim == 0  lead = 0, len = T.
 *   correct = #{j < len : pred[j] == target[lead + j]};  acc = (double)correct / len, one fp64 division;
 *   correct_topk = #{j < len : rank[lead + j] < topk}   (rank [rows][aux_ld]; correct_topk NULL iff rank NULL; topk >= 1);
 *   nll_sum = the fp64 sum of the fp32 nll[lead + j], j < len (nll [rows][aux_ld]; nll_sum NULL iff nll NULL), in this order: lane l of 64 adds
 *             j = l, l + 64, ... ascending from 0.0, then s[l] += s[l ^ o] for o = 32, 16, 8, 4, 2, 1;
 *   status = 0, or FN_MATCH_EMPTY for an all-zero target row under trim: len = 0, lead = T, acc = 0, nll_sum = 0, counts 0 (the reference
 *            divides by zero there).
 * One wavefront per row, no LDS, no cap on T beyond int32.
 * pred, target, lead, len, correct, acc or status NULL, rank without correct_topk or the reverse, nll without nll_sum or the reverse:
 * FN_E_NULL; rows, T < 1, pred_ld or tgt_ld < T, aux_ld < T with nll or rank, topk < 1 with rank: FN_E_SHAPE; both before any launch.
 * ------------------------------------------------------------------------------------------ */
#define FN_MATCH_EMPTY 1
int fn_token_score(const float* x, int64_t stride_b, int64_t stride_t, int B, int T, int V, const int32_t* target, int tgt_ld, int32_t* pred,
                   float* nll, int32_t* rank, int out_ld, void* stream);
int fn_match_rows(const int32_t* pred, int pred_ld, const int32_t* target, int tgt_ld, int rows, int T, int trim, const float* nll,
                  const int32_t* rank, int aux_ld, int topk, int32_t* lead, int32_t* len, int32_t* correct, int32_t* correct_topk, double* acc,
                  double* nll_sum, int32_t* status, void* stream);

/* TIME-axis log_softmax of the sub-decoders (gmm_model.py:110,115; the reference's dim=1 quirk).
 * logits [Tr][B][Cc] time-major.  logp_bt [B][Tr][Cc].  target [B][Tr] or NULL.
 * nll_bc [B][Cc] (sum over t with target==c of -logp) ; dlogits [Tr][B][Cc] = grad_scale * dNLLsum/dlogits. */
int fn_time_logsoftmax(const float* logits, int B, int Tr, int Cc, float* logp_bt, const int32_t* target, float* nll_bc,
                       float grad_scale, float* dlogits, void* stream);
int fn_time_logsoftmax_bwd(const float* logp_bt, const float* gout_bt, int B, int Tr, int Cc, float* dlogits,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Latent block: reparameterised sample + Gaussian-mixture posterior (gmm_model.py:86,91,229-242,
 * 194-218) and the KL / class terms of trainer_gmm.py:150-194.  One wavefront per batch row.
 *   pre [B][2Z]: columns [0,Z) = mu, [Z,2Z) = v (sigma = exp(v));  eps [B][Z]
 *   mu_lk, lv_lk [K][Z] component means / log-variances
 * fwd outputs: sigma [B][Z], z [B][Z], ll [B][K], qy [B][K], y [B] int32,
 *   terms [B][4]: {sum_k qy_k KLmean_k, mean_k(qy log qy), KLmean_{label}, -log softmax(qy)[label]}
 *   (label terms only when labels != NULL).  K <= 8.
 * ------------------------------------------------------------------------------------------ */
int fn_latent_fwd(const float* pre, const float* eps, const float* mu_lk, const float* lv_lk, int B, int Z, int K,
                  const int32_t* labels, float* sigma, float* z, float* ll, float* qy, int32_t* y, float* terms,
                  void* stream);
/* Backward. Upstream gradients (any may be NULL): g_z, g_mu, g_sigma [B][Z]; g_ll, g_qy [B][K].
 * w3 = DEVICE pointer to {w_lat, w_cls, w_clf} (NULL = all zero; written by fn_step_params so that a captured graph never
 * bakes the step-dependent beta into a kernel argument).  Fused loss gradient (trainer_gmm.py:150-194):
 *    L += w_lat * sum_b sum_k qy KLmean_k  + w_cls * sum_b mean_k(qy log qy)          (unsupervised)
 *    L += w_lat * sum_b KLmean_label       + w_clf * sum_b CE(softmax(qy), label)     (labels != NULL)
 * The gradient is that of this formula AT THE GIVEN z and qy (the float32 arrays fn_latent_fwd wrote): the posterior is not
 * recomputed from pre, and the softmax backward q_k (dq_k - sum_j q_j dq_j), dq_k = g_qy_k + dL/dq_k, uses qy as handed over.
 * Near saturation this differs from the gradient of the posterior recomputed in float64 by up to 1e-5 of a tile maximum, because
 * a float32 qy sums to 1 to one ulp only while dq carries KL means of about 1e3; a component with qy == 0 contributes 0 to
 * the entropy gradient.  With labels w_cls is not read, without labels w_clf is not read.
 * outputs: dpre [B][2Z]; dmu_lk_rows [B][K][Z] per-row contributions to d mu_lookup (reduce with
 * fn_colsum_f32 over B; may be NULL). */
int fn_latent_bwd(const float* pre, const float* eps, const float* mu_lk, const float* lv_lk, int B, int Z, int K,
                  const int32_t* labels, const float* z, const float* qy, const float* g_z, const float* g_mu,
                  const float* g_sigma, const float* g_ll, const float* g_qy, const float* w3, float* dpre,
                  float* dmu_lk_rows, void* stream);

/* Pairwise latent regulariser (trainer_gmm.py:199-217): rows [row0,row0+nrows) of the global batch.
 *   attr_all is float64 like the reference's numpy densities (only the sign of a_i - a_j is used).
 *   loss_rows[i] = sum_j (tanh(z0[row0+i]-z0[j]) - sign(a[row0+i]-a[j]))^2
 *   dz0[i]       = grad_scale * 4 * sum_j (tanh(D)-S)(1-tanh(D)^2)     (the exact d/dz0 of sum_ij, by antisymmetry) */
int fn_pairwise_reg(const float* z0_all, const double* attr_all, int n_all, int row0, int nrows, float* loss_rows,
                    float grad_scale, float* dz0, void* stream);

/* Masked probability sums of the GLSR regulariser (trainer_glsr.py:121-139: approx_played_notes / approx_time_separators = the
 * softmax mass of a token range, per decoder step).  logits [rows][ld], E valid columns; two ranges [lo0,hi0), [lo1,hi1).
 *   sums [rows][2] (or NULL) = P_0, P_1;   with w [rows][2] and dlogits [rows][ld] (may alias logits):
 *   dlogits[u] = p_u (w0 [u in range 0] + w1 [u in range 1] - (w0 P_0 + w1 P_1)) = gradient of w0 P_0 + w1 P_1 wrt the logits. */
int fn_masked_prob(const float* logits, int64_t rows, int E, int ld, int lo0, int hi0, int lo1, int hi1, float* sums, const float* w,
                   float* dlogits, void* stream);

/* Adversarial heads of the Fader-Networks sibling (model_v2.py:572-575, trainer_fader.py:105-110), forward + gradient in one pass,
 * one wavefront per row.  For a in {0: rhythm, 1: note}:  pre = w_a . z[b] + b_a ;  o[b][a] = relu(pre) * mask[b][a] (mask = the
 * dropout keep-mask already scaled by 1/(1-p)) ;  loss_rows[b][a] = (o - dens[b][a])^2 ;
 * da[b][a] = lam * 2 (o - dens) * inv_global_batch * mask * [pre > 0]  (lam read from DEVICE memory, fn_step_params out[6]) ;
 * g_z[b][:] -= sum_a da[b][a] w_a   - MINUS: ReverseLayerF hands the encoder the negated gradient (model_v2.py:426-435).
 * z [B][ldz], g_z [B][ldg] (may be NULL), w_a [Z], b_a [1], mask / dens / o / loss_rows / da [B][2]. */
int fn_adv_head(const float* z, int ldz, int Z, int B, const float* w_r, const float* w_n, const float* b_r, const float* b_n,
                const float* mask, const float* dens, const float* lam_dev, float inv_global_batch, float* o, float* loss_rows, float* da,
                float* g_z, int ldg, void* stream);

/* ------------------------------------------------------------------------------------------
 * clip_grad_norm_(., max_norm) + Adam (trainer_gmm.py:250-251, torch.optim.Adam defaults) over a
 * flat fp32 buffer.  fn_sumsq writes sum(g^2) to out[0]; fn_clip_adam reads the (all-reduced)
 * total from sumsq[0] on device, so no host sync is needed.
 *
 * fn_step_params keeps the step counters ON THE DEVICE (counters[0] = training step, counters[1] = Adam t; int64) and
 * derives every step-dependent scalar from them: out[0..2] = {w_lat, w_cls, w_clf} for fn_latent_bwd with
 * beta0 = 0 if step < 1000 else min((step-10000)/10000*beta, beta)  (trainer_gmm.py:125-128), out[3] = lr/(1-beta1^t),
 * out[4] = 1/sqrt(1-beta2^t), out[5] = beta0, out[6] = min(step/2000*1e-4, 1e-4) (adversarial weight of the Fader-Networks
 * sibling, trainer_fader.py:105), out[7] = beta * inv_global_batch (the constant KL weight of trainer_singlevae.py:104); out has
 * 8 floats.  advance != 0 increments both counters (t is advanced BEFORE use, the step AFTER).  fn_clip_adam takes
 * hyper = &out[3].  The whole training step is therefore capturable in one hipGraph.
 * ------------------------------------------------------------------------------------------ */
int fn_step_params(int64_t* counters, float beta, float lr, float beta1, float beta2, int supervised, float inv_global_batch,
                   int advance, float* out, void* stream);
int fn_sumsq_f32(const float* g, int64_t n, float* out, float* ws, size_t ws_bytes, void* stream);
size_t fn_sumsq_ws_bytes(int64_t n);
int fn_clip_adam(float* p, const float* g, float* m, float* v, int64_t n, const float* sumsq, float max_norm,
                 const float* hyper, float beta1, float beta2, float eps, void* stream);

/* one-hot (B,T,V) -> int32 indices (argmax along the last axis); used at the class boundary where callers
 * hand over convert_to_one_hot tensors (trainer_gmm.py:296-303) */
int fn_onehot_to_index(const float* oh, int64_t rows, int V, int32_t* idx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Data parallelism: RCCL collectives on the CALLER's stream (one process per GPU).
 * The reference has no distributed code; the step that must see the REDUCED gradient is
 * clip_grad_norm_ + optimizer.step(), trainer_gmm.py:249-251.  Rank 0 calls fn_comm_unique_id and hands the
 * FN_COMM_ID_BYTES bytes to the other ranks out of band (music-fader-nets_amd/parallel.py uses the torch.distributed
 * store); every rank then calls fn_comm_init with the device it will use CURRENT.  The collectives are ordinary
 * stream-ordered work: they may be captured into a hipGraph together with the kernels of the step, and no helper thread
 * touches the streams.  librccl is bound at run time (dlopen by SONAME: a copy already in the process is reused);
 * FN_E_COMM when it is missing.  In-place SUM all-reduce of fp32; all-gather of raw bytes (recv holds world * bytes_per_rank).
 * ------------------------------------------------------------------------------------------ */
#define FN_COMM_ID_BYTES 128
int fn_comm_unique_id(void* id_out);
int fn_comm_init(void** comm_out, int world, int rank, const void* id);
int fn_comm_destroy(void* comm);
int fn_comm_all_reduce_f32(void* comm, float* buf, size_t n, void* stream);
int fn_comm_all_gather(void* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
/* what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank): bench.py prints them, so that a multi-GPU line
 * proves that its gradient all-reduce (trainer_gmm.py:249-251) ran over N RCCL ranks */
int fn_comm_count(void* comm, int* count_out);
int fn_comm_rank(void* comm, int* rank_out);

/* Diagnostic: `blocks` workgroups that each hold `lds_bytes` of LDS (<= 64 KB) and spin for about `cycles` clock ticks - a stand-in
 * for a foreign kernel (an RCCL channel, another process' launch) that is RESIDENT on some compute units when a weight-stationary
 * launch starts: the scan's remaining workgroups cannot become resident until it leaves, the resident ones spin at their counters
 * (bounded).  tests/test_gpu_parity.py uses it to show that such contention delays a step but never changes its results. */
int fn_occupy_cus(int blocks, int lds_bytes, long long cycles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FADERNETS_H */
