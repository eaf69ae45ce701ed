/* gple_debug.h — diagnostic entry points of libgple_hip.so that are NOT part of the drop-in C-ABI (include/gple.h): they run one
 * internal kernel family on host operands so that tests and probes can check it in isolation.
 *   tests/test_gpu_chol_diag.py, probes/step_probe.py -> gple_debug_potrf_step
 *   tests/test_host_logic.py                          -> gple_debug_chol_layout (no device call)
 *   tests/test_gpu_gemm.py                            -> gple_debug_gemm, gple_debug_gemm_strided
 *   tests/test_gpu_chol_diag.py                       -> gple_debug_side_stream, gple_debug_chol_knobs (the give-up test)
 *   tests/test_gpu_parity.py                          -> gple_debug_predict_knobs
 *   tests/test_gpu_format.py                          -> gple_debug_format_knobs
 *   tests/test_gpu_predict_rows.py                    -> gple_debug_fit_factor
 *   tests/test_gpu_hop_smooth.py                      -> gple_debug_hop_smooth_split (no device call) */
#ifndef GPLE_DEBUG_H
#define GPLE_DEBUG_H
#include "../../include/gple.h"
#ifdef __cplusplus
extern "C"
{
#endif
	/* Layout of the factorisation of an n-column matrix (host logic only): outer block bounds, fork points of the block-row inverse, workspace. */
	int gple_debug_chol_layout(int n, int cap, int* bounds, int* nb, int* forks, int* nf, unsigned long long* work_doubles);
	/* The one-launch panel step (potrf_step_kernel) at block column 1 of an n x n matrix, n = 128 + below (below = 0 | 64); A and T
	 * (n x n, column-major) come back as the first launch leaves them; stamps: 24 slots — shader-clock stamps of workgroup 0, the last slot = `info` (0, or 1 + the first column whose pivot was not positive). */
	int gple_debug_potrf_step(gple_ctx* ctx, double* A, double* T, int pend, int below, long long* stamps, int reps, float* ms_per_launch);
	/* C(m,n) = alpha sum_k A(m,k) B(n,k) + beta C(m,n) by the fp64 MFMA GEMM family (gple_gemm.hip); layouts and k-ranges as GemmDesc
	 * in gple_internal.h; tile = 32 | 64 | 128 | 0 (the library's own choice). */
	int gple_debug_gemm(gple_ctx* ctx, const double* A, long lda, int a_kmajor, const double* B, long ldb, int b_kmajor, double* C, long ldc,
		int c_trans, int M, int N, int K, double alpha, double beta, int krange, int lower_only, int tile);
	/* The same product on windows of larger buffers, as the fits call the family: per operand the whole host buffer with its element count, the
	 * element offset of the window's origin, the leading dimension and the batch stride (0 repeats the operand for every item).  The three buffers
	 * are copied in whole, one launch of `batch` items runs, the whole C buffer is copied back — what lies outside the written windows included.
	 * Offsets, leading dimensions and strides are multiples of 4 doubles (the kernels load 32-byte vectors); a window that leaves its buffer, or
	 * items of C that overlap, are GPLE_ERR_BAD_ARG and nothing is launched. */
	int gple_debug_gemm_strided(gple_ctx* ctx, const double* A, long countA, long offA, long lda, long strideA, int a_kmajor, const double* B, long countB,
		long offB, long ldb, long strideB, int b_kmajor, double* C, long countC, long offC, long ldc, long strideC, int c_trans, int batch, int M, int N, int K,
		double alpha, double beta, int krange, int lower_only, int tile);
	/* The side stream the context's fits run their block-row inverse on (created by the first fit with n >= 1024): how many candidate streams
	 * were tried until one ran beside the main stream, and whether the chosen one did (0: none did, or no fit has needed one yet). */
	int gple_debug_side_stream(gple_ctx* ctx, int* attempts, int* overlaps);
	/* A transport for gple_set_allgather_function() that stands in for a world that is not there: rank r of P on a one-GPU box (bench.py
	 * --emulate-rank r/P).  Pass (void*)(1 + r + 256 * P) as the communicator: this rank's block is copied into its slot of the gathered buffer,
	 * the other slots are zero-filled.  What the rank computes, enqueues and unpacks is what a real rank does; the fabric is missing. */
	int gple_debug_solo_allgather(const void* sendbuff, void* recvbuff, size_t sendcount, int datatype, void* comm, void* hip_stream);
	/* Test knobs of the factorisation on ONE context; a negative argument leaves its knob alone.  scheme: 0 = a launch per panel (what
	 * GPLE_CHOL_SCHEME=step selects process-wide), 1 = one launch per outer block, 2 = back to the environment's; poll_limit: polls before a waiting
	 * wave of the one-launch scheme gives up (0 = the default, 2^23); dag_blocks: workgroups of its launches (0 = one per CU).  giveups / recoveries
	 * (nullable): how often the host has seen info = -1 on this context / repeated a factorisation with a launch per panel because of it. */
	int gple_debug_chol_knobs(gple_ctx* ctx, int scheme, int poll_limit, int dag_blocks, long* giveups, long* recoveries);
	/* Test knobs of the predict path on ONE context; 0 / 1 set a knob, 2 hands it back to the default (1), a negative argument leaves it alone.
	 * rownorm_pipe: the contraction kernel of large predicts — 0 = rownorm2_kernel (a barrier-to-barrier k-step), 1 = rownormp_kernel (the k-steps
	 * of a unit as one pipeline).  fused_small: real fits with N <= 256 — 0 = K* generation, contraction and sums as separate kernels,
	 * 1 = predict_fused256_kernel.  Either pair must agree bit for bit (tests/test_gpu_parity.py). */
	int gple_debug_predict_knobs(gple_ctx* ctx, int rownorm_pipe, int fused_small);
	/* The inverse Cholesky factor T = chol(K)^-1 of a fit, copied to the host exactly as the predict kernels read it: the whole
	 * n_total x n_total buffer with ldt = n_total, padding included.  Exactly one of `real` and `cplx` is set (as in gple_element); both or
	 * neither is GPLE_ERR_BAD_ARG.  Element order: T(n, k) — row n of the factor, the index the contraction's result rows sit on,
	 * column k, the index of K*(row, k) — lies at T[n + k * n_total]: column-major, n fastest.  T(n, k) = 0 for k > n inside the diagonal
	 * 64 x 64 blocks; the 64 x 64 blocks above the diagonal are never written and never read (whatever the memory held, NaN patterns under
	 * GPLE_POISON_T=1).  The complex fit is the real system of [Re; Im]: n_total = 2 n_split, index n_split + i is the imaginary part of point i.
	 * Rows and columns N .. n_split - 1 of either half are padding, where T is the identity.  n_total, n_split (= n_total for a real fit's one
	 * half) and N (each nullable) are always reported; T = NULL with capacity = 0 asks for them alone.  capacity: doubles T has room for — fewer
	 * than n_total^2 is GPLE_ERR_BAD_ARG and nothing is copied.  Like the other getters the call validates the fit first, so a give-up of the
	 * one-launch factorisation is recovered before the copy.  tests/test_gpu_predict_rows.py */
	int gple_debug_fit_factor(const gple_real_fit* real, const gple_complex_fit* cplx, double* T, size_t capacity, int* n_total, int* n_split, int* N);
	/* Name of the kernel the last predict of this context ran its variance contraction on ("" before the first one; bench.py's roofline label). */
	const char* gple_debug_last_contraction_kernel(gple_ctx* ctx);
	/* Test knob of gple_format_g on ONE context: slots = 1 — the size pass keeps every item (16 bytes and a length byte per number) and the write
	 * pass reads them; 0 — the write pass converts again (the default: DESIGN.md §14 has the measurement); negative leaves it alone.  The two must
	 * agree byte for byte (tests/test_gpu_format.py). */
	int gple_debug_format_knobs(gple_ctx* ctx, int slots);
	/* The split of the trajectory index of gple_hop_smooth and gple_hop_smooth_mf (host logic only; DESIGN.md §17, "The ensemble in phase space,
	 * smoothed"): the trajectories of a chunk and the number of chunks, whose partial sums the finish adds in ascending order. */
	int gple_debug_hop_smooth_split(int num_pes, size_t n, size_t n_x, size_t n_p, size_t* chunk, size_t* n_chunks);
#ifdef __cplusplus
}
#endif
#endif
