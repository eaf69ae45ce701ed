/* gple.h — C-ABI of the MI355X-native GPR fit + predict hot path.
 *
 * Drop-in boundary for kaigu1997/gaussian_process_liouville_equation (reference paths are relative to
 * /root/reference/gaussian_process_liouville_equation/ unless they start with test/).
 * The reference has NO FFI of its own: its boundary is the C++ classes of kernel.h / complex_kernel.h /
 * predict.h / opt.h.  Every entry point below names the reference constructor / getter it replaces; the
 * header-only C++ adapters in gaussian_process_liouville_equation_amd/host/ re-create those classes on top
 * of this ABI.
 *
 * Conventions
 *   - all arithmetic is fp64; complex numbers are interleaved (re, im) pairs of doubles;
 *   - phase-space points are 2 x N column-major == interleaved [x0,p0,x1,p1,...]   (stdafx.h:153);
 *   - matrices returned by the *_get calls are column-major (Eigen default)          (stdafx.h:133);
 *   - every function returns GPLE_OK (0) or a GPLE_ERR_* code; numerical breakdown is NOT an error:
 *     like the reference (opt.cpp:420-431, LDLT::info() never checked) non-finite values are returned
 *     in the outputs and `info` is set;
 *   - array arguments are host pointers unless GPLE_IO_DEVICE is set in `flags`, in which case every
 *     array argument of that call (inputs and outputs) is a device pointer on the context's device and
 *     the call is asynchronous on the context's stream except for the scalar result block;
 *   - predict calls are thread-safe on a shared const fit handle (evolve.cpp:392-420 calls the reference
 *     predictors from TBB workers); fit calls on one context must not run concurrently.
 */
#ifndef GPLE_H
#define GPLE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPLE_OK 0
#define GPLE_ERR_BAD_ARG 1
#define GPLE_ERR_HIP 2
#define GPLE_ERR_ALLOC 3
#define GPLE_ERR_COLLECTIVE 5 /* RCCL could not be resolved or a collective failed (gple_ctx_last_error has the text) */
#define GPLE_ERR_STATE 4 /* e.g. derivative output requested from a fit built without GPLE_CALC_DERIVATIVE; call on a destroyed context */
/* The factorisation of a fit runs as ONE launch per block of panels whose workgroups hand tiles to each other through flags; every wait is bounded
 * (2^23 polls, about 5-8 s per waiting launch: gple_chol.hip), and a wave that gives up leaves the launch unfinished.  That never yields a wrong
 * number: on the device everything derived from the unfinished factor becomes NaN, and the first call on the fit that drains the stream
 * (*_fit_create with a scalars struct, *_fit_get_scalars, *_fit_get, a predict with host pointers or labels, the objective and NLML entry points)
 * notices, repeats the factorisation with one launch per panel (no waits between workgroups) and returns the correct result — the caller sees
 * nothing but the delay.  GPLE_ERR_TIMEOUT is returned only (a) by such a draining call when OTHER calls had been enqueued on the fit before it
 * (device pointers, no labels: those never drain the stream) — the call's own outputs are correct, theirs are NaN, the fit is valid from here on,
 * gple_ctx_last_error says how many to repeat; or
 * (b) when the repetition failed as well (it cannot give up: it has no waits). */
#define GPLE_ERR_TIMEOUT 6

/* The three bools of the Training*Kernel constructors (kernel.h:128-134, complex_kernel.h:167-173). */
#define GPLE_CALC_ERROR 0x1u
#define GPLE_CALC_AVERAGE 0x2u
#define GPLE_CALC_DERIVATIVE 0x4u
/* Array arguments of this call are device pointers. */
#define GPLE_IO_DEVICE 0x100u
/* *_predict: contract every test row.  By default a predict first sums K*^2 per test row (the generation's arithmetic without its
 * HBM write), then generates K* and contracts only the rows with |k*|^2 >= 2^-56 sf^2 sn^2 k(x*,x*) (complex: half that): for the
 * others k(x*,x*) - k* K^-1 k*^T rounds to k(x*,x*) whatever the contraction returns — grid points far from every training
 * point, most of a phase-space grid.  The outputs are bit-identical either way.  Pass the flag for measurements that want the
 * full contraction timed, and for test points known to lie on the data, where nothing can be skipped and the extra pass costs
 * 2-13 % (gple_predict_batch, the step loop and the objective evaluations do that themselves). */
#define GPLE_PREDICT_FULL 0x200u

#define GPLE_REAL_NPARAM 4    /* KernelBase::NumTotalParameters        kernel.h:33          */
#define GPLE_COMPLEX_NPARAM 8 /* ComplexKernelBase::NumTotalParameters complex_kernel.h:22  */

typedef struct gple_ctx gple_ctx;
typedef struct gple_real_fit gple_real_fit;       /* TrainingKernel        kernel.h:111-280        */
typedef struct gple_complex_fit gple_complex_fit; /* TrainingComplexKernel complex_kernel.h:150-318 */

/* Scalar getters of TrainingKernel. Fields whose flag was not requested are NaN. */
typedef struct gple_real_fit_scalars {
	double rescale_factor;           /* get_rescale_factor            kernel.h:146, kernel.cpp:279 */
	double magnitude;                /* get_magnitude                 kernel.h:167-179             */
	double error;                    /* get_error (LOOCV)             kernel.cpp:285               */
	double population;               /* get_population                kernel.cpp:286-297           */
	double first_order_average[2];   /* get_1st_order_average         kernel.cpp:298-312           */
	double purity;                   /* get_purity                    kernel.cpp:325-335           */
	double error_derivative[4];      /* get_error_derivative          kernel.cpp:381-400           */
	double population_derivative[4]; /* get_population_derivative     kernel.cpp:401-435           */
	double purity_derivative[4];     /* get_purity_derivative         kernel.cpp:436-477           */
	int info;                        /* 0: factorisation fine; k>0: non-positive pivot met at column k (NaN propagates, as in the reference).  Never -1 in a
	                                    struct a call returned with GPLE_OK: a give-up of the one-launch factorisation is recovered from first (GPLE_ERR_TIMEOUT above) */
} gple_real_fit_scalars;

/* Scalar getters of TrainingComplexKernel. */
typedef struct gple_complex_fit_scalars {
	double rescale_factor;       /* complex_kernel.cpp:262       */
	double magnitude;            /* complex_kernel.h:192-204     */
	double error;                /* complex_kernel.cpp:270-286   */
	double purity;               /* complex_kernel.cpp:357-377   */
	double error_derivative[8];  /* complex_kernel.cpp:444-474   */
	double purity_derivative[8]; /* complex_kernel.cpp:475-590   */
	int info;                    /* as in gple_real_fit_scalars  */
} gple_complex_fit_scalars;

/* Scalar getters of PredictiveKernel / PredictiveComplexKernel (only the first 4 entries of
 * error_derivative are meaningful for the real kernel). NaN when no labels / no derivative were asked. */
typedef struct gple_predict_scalars {
	double error;               /* kernel.cpp:522, complex_kernel.cpp:646         */
	double error_derivative[8]; /* kernel.cpp:524-542, complex_kernel.cpp:648-668 */
} gple_predict_scalars;

/* Arrays that the reference exposes through matrix/vector getters. */
typedef enum gple_real_array {
	GPLE_R_KERNEL = 0,       /* KernelBase::get_kernel,  N*N                kernel.h:82   */
	GPLE_R_INVERSE = 1,      /* get_inverse,             N*N                kernel.h:153  */
	GPLE_R_INVLBL = 2,       /* get_inverse_times_label, N                  kernel.h:160  */
	GPLE_R_INVLBL_DERIV = 3, /* get_inverse_times_label_derivative, 4*N     kernel.h:215  */
	GPLE_R_LABEL = 4,        /* rescaled label, N                           kernel.cpp:280 */
	GPLE_R_INVERSE_DIAG = 5  /* diagonal of get_inverse, N                                */
} gple_real_array;

typedef enum gple_complex_array {
	GPLE_C_KERNEL = 0,  /* get_kernel, N*N real                                 complex_kernel.h:90  */
	GPLE_C_PSEUDO = 1,  /* get_pseudo_kernel, N*N complex                       complex_kernel.h:97  */
	GPLE_C_UPPER_LEFT = 2,  /* get_upper_left_block_of_augmented_inverse, N*N complex   :208 */
	GPLE_C_LOWER_LEFT = 3,  /* get_lower_left_block_of_augmented_inverse, N*N complex   :215 */
	GPLE_C_INVLBL = 4,      /* get_upper_part_of_augmented_inverse_times_label, N complex :222 */
	GPLE_C_INVLBL_DERIV = 5,/* ..._derivative, 8*N complex                               :245 */
	GPLE_C_LABEL = 6        /* rescaled label, N complex                    complex_kernel.cpp:263 */
} gple_complex_array;

/* ---- context ------------------------------------------------------------------------------------- */
/* device: HIP device ordinal; stream: a hipStream_t to run on, or NULL for a stream owned by the context. */
int gple_ctx_create(int device, void* stream, gple_ctx** out);
/* Lifetime rule: every fit / objective handle holds a reference on the context it was created from.  gple_ctx_destroy()
 * drains the stream, CLOSES the context (every entry point that takes `ctx` returns GPLE_ERR_STATE from then on) and drops
 * the creator's reference; device buffers, the stream and the context itself are freed when the last handle created from it
 * is released.  Handle-only calls (*_fit_get_scalars, *_fit_get, *_fit_release, gple_objective_release) therefore stay valid
 * after the destroy and return a status instead of touching freed memory.  A second destroy of a context that handles
 * still keep alive returns GPLE_ERR_STATE; a caller-provided stream must outlive the last handle. */
int gple_ctx_destroy(gple_ctx* ctx);
int gple_ctx_synchronize(gple_ctx* ctx);
/* The context keeps every device buffer it ever needed in a grow-only pool (no hipMalloc on the steady-state path; a single
 * large predict can leave up to 4 GiB of K* scratch behind). This synchronises the stream and frees the buffers that no live
 * fit owns; *bytes_freed (nullable) receives the amount. */
int gple_ctx_trim(gple_ctx* ctx, size_t* bytes_freed);
const char* gple_status_string(int status);
/* Last HIP error text seen by this context (empty string when none). */
const char* gple_ctx_last_error(const gple_ctx* ctx);

/* ---- tracing --------------------------------------------------------------------------------------- */
/* The reference only logs wall-clock seconds per output (output.cpp:246-248). With timing enabled the library
 * brackets its phases with HIP events on the context's stream.  Timing never forces a synchronisation of its own: the
 * intervals are collected at the library's next stream synchronisation (gple_ctx_synchronize, gple_ctx_get_timing, a
 * scalar getter, a call with host outputs). */
typedef enum gple_timer {
	GPLE_TIMER_FIT = 0,            /* whole *_fit_create call (device side)                 */
	GPLE_TIMER_PREDICT = 1,        /* whole *_predict call (device side)                    */
	GPLE_TIMER_PREDICT_KERNEL = 2, /* the MFMA row-norm kernel of *_predict alone; count = its launches */
	GPLE_TIMER_DERIV_GEMM = 3,     /* the dK * K^-1 MFMA GEMM of a GPLE_CALC_DERIVATIVE fit (kernel.cpp:354); count = its launches */
	GPLE_TIMER_WIGNER = 4,         /* the MFMA kernel of gple_wigner alone (all T output times of a call); count = its launches */
	GPLE_TIMER_MQCL = 5,           /* the step kernels of one gple_mqcl_evolve call (all its steps, no set-up), or every block and mask of one gple_mqcl_evolve_absorbing call; count = its calls */
	GPLE_TIMER_RECON = 6,          /* the device work of one gple_nlml_weights / gple_grid_survey / gple_grid_select / gple_grid_reconstruct call (and of their _cross forms); count = calls */
	GPLE_TIMER_FORMAT = 7,         /* the three kernels of one gple_format_g call (no staging, no copy of the text); count = calls */
	GPLE_TIMER_PARSE = 8,          /* the kernels of one gple_parse_g call (three, or two when it only counts; no staging, no copies); count = calls */
	GPLE_TIMER_DVR_POWER = 9,      /* the products of one gple_dvr_propagator call (Horner form of P4 and the binary power; no set-up, no copies); count = calls */
	GPLE_TIMER_DVR_FLUX = 10,      /* the products of one gple_dvr_flux call (P4, the power, the loss matrix and every sandwich; no set-up, no copies); count = calls */
	GPLE_TIMER_DVR_SPECTRUM = 11,  /* the device work of one gple_dvr_spectrum call (P4, the squarings, the thin products, the projection and the reduction; no copies); count = calls */
	GPLE_TIMER_HOP = 12,           /* the step kernel of one gple_hop_evolve or gple_hop_evolve_dc call (all its steps, no staging); count = calls */
	GPLE_TIMER_HOP_BIN = 13,       /* the bin kernel of one gple_hop_bin call (no staging, no clear); count = calls */
	GPLE_TIMER_HOP_GROUPS = 14,    /* the step kernel of one gple_hop_evolve_groups or _groups_dc call (all its steps, no staging); count = calls */
	GPLE_TIMER_HOP_MF = 15,        /* the step kernel of one gple_hop_evolve_mf or gple_hop_evolve_groups_mf call (all its steps, no staging); count = calls */
	GPLE_TIMER_HOP_SQC = 16,       /* the step kernel of one gple_hop_evolve_sqc or gple_hop_evolve_groups_sqc call (all its steps, no staging); count = calls */
	GPLE_TIMER_HOP_MASH = 17,      /* the step kernel of one gple_hop_evolve_mash or gple_hop_evolve_groups_mash call (all its steps, no staging); count = calls */
	GPLE_TIMER_HOP_BIN_MF = 18,    /* the bin kernel of one gple_hop_bin_mf call (no staging, no clear); count = calls */
	GPLE_TIMER_HOP_OUTGOING = 19,  /* the bin kernel of one gple_hop_outgoing, _outgoing_mf or _outgoing_sqc call (no staging, no clear); count = calls */
	GPLE_TIMER_HOP_SMOOTH = 20,    /* the three kernels of one gple_hop_smooth or gple_hop_smooth_mf call (terms, contraction, finish; no staging); count = calls */
	GPLE_TIMER_SCATTER = 21        /* the march kernel of one gple_scatter call (no table of the potential, no staging); count = calls */
} gple_timer;
int gple_ctx_enable_timing(gple_ctx* ctx, int on);
/* Synchronises the stream, then: last = milliseconds of the most recent interval; total / count = accumulated since
 * enable (any may be NULL). */
int gple_ctx_get_timing(gple_ctx* ctx, gple_timer which, double* last_ms, double* total_ms, long* count);
/* Synchronises the stream, then: test rows the pruned predicts contracted / saw, in units of 128 rows (ceil of the live rows of
 * each predict), since the context was created or since the last call with reset != 0 (see GPLE_PREDICT_FULL). */
int gple_ctx_get_prune_stats(gple_ctx* ctx, unsigned long long* contracted_blocks, unsigned long long* seen_blocks, int reset);

/* ---- KernelBase (kernel.h:29-106, kernel.cpp:8-242) ---------------------------------------------- */
/* K = sf^2 (G + sn^2 delta) for theta = (sf, lx, lp, sn), left 2 x R, right 2 x C, K is R x C column-major.
 * same_features != 0 reproduces the `LeftFeature.data() == RightFeature.data()` branch (identity delta,
 * symmetric derivative with zero diagonal); dK (nullable) receives the 4 derivative matrices, 4*R*C. */
int gple_real_gram(gple_ctx* ctx, const double theta[4], const double* left, size_t R, const double* right, size_t C,
	int same_features, unsigned flags, double* K, double* dK);

/* ---- ComplexKernelBase (complex_kernel.h:14-145, complex_kernel.cpp:20-200) ------------------------ */
/* theta = (s, sR, lRx, lRp, sI, lIx, lIp, sn).  K = s^2 (K_R + K_I + sn^2 delta) is R x C real; Kt (nullable) = s^2 (K_R - K_I +
 * 2i K_C), R x C (re,im) pairs; dK (nullable) receives the 8 derivative matrices of K (8*R*C doubles, get_derivative()), dKt
 * (nullable) the 8 of Kt (16*R*C doubles, get_pseudo_derivative()).  same_features as in gple_real_gram. */
int gple_complex_gram(gple_ctx* ctx, const double theta[8], const double* left, size_t R, const double* right, size_t C,
	int same_features, unsigned flags, double* K, double* Kt, double* dK, double* dKt);

/* cutoff_factor<T> (kernel.h:301-332). prediction has M (real) or 2M (complex) doubles. */
int gple_cutoff_factor(gple_ctx* ctx, const double* prediction, int is_complex, const double* variance, size_t M,
	unsigned flags, double* factor);

/* ---- TrainingKernel (kernel.cpp:244-479) ---------------------------------------------------------- */
/* theta = (sf, lx, lp, sn); X = 2N; y: N labels; y_is_complex != 0 means y holds N (re,im) pairs of which
 * the real part is used (ElementTrainingSet = tuple<PhasePoints, VectorXcd>, kernel.h:14, kernel.cpp:280).
 * scalars == NULL defers the scalar members: with device-resident inputs (GPLE_IO_DEVICE) the call then only enqueues
 * work and returns; gple_real_fit_get_scalars() drains the stream when a getter is first needed. */
int gple_real_fit_create(gple_ctx* ctx, const double theta[4], const double* X, const double* y, int y_is_complex,
	size_t N, unsigned flags, gple_real_fit_scalars* scalars, gple_real_fit** out);
/* The scalar getters of TrainingKernel (kernel.h:181-243: rescale factor, magnitude, error, population, <r>, purity and
 * their derivatives); synchronises the context's stream on first use after a deferred create. */
int gple_real_fit_get_scalars(gple_real_fit* fit, gple_real_fit_scalars* scalars);
int gple_real_fit_retain(gple_real_fit* fit);
int gple_real_fit_release(gple_real_fit* fit);
size_t gple_real_fit_size(const gple_real_fit* fit);
/* Copies one array into dst (host pointer, or device pointer with GPLE_IO_DEVICE). Matrices that the hot
 * path does not need (the explicit inverse) are materialised on first request. */
int gple_real_fit_get(gple_real_fit* fit, gple_real_array which, unsigned flags, double* dst);

/* ---- PredictiveKernel (kernel.cpp:481-544) -------------------------------------------------------- */
/* Xs = 2M test points. labels (nullable, M) switches on `error`; GPLE_CALC_DERIVATIVE + labels switches on
 * error_derivative (needs a fit created with GPLE_CALC_DERIVATIVE). prediction (nullable) receives the
 * rescaled mean `Prediction`; variance / cutoff_prediction (nullable) as get_variance / get_cutoff_prediction. */
int gple_real_predict(gple_ctx* ctx, const gple_real_fit* fit, const double* Xs, size_t M, unsigned flags,
	const double* labels, double* prediction, double* variance, double* cutoff_prediction,
	gple_predict_scalars* scalars);

/* ---- TrainingComplexKernel / PredictiveComplexKernel (complex_kernel.cpp:221-670) ------------------ */
/* theta = (s, sR, lRx, lRp, sI, lIx, lIp, sn); y = N (re,im) pairs. */
int gple_complex_fit_create(gple_ctx* ctx, const double theta[8], const double* X, const double* y, size_t N,
	unsigned flags, gple_complex_fit_scalars* scalars, gple_complex_fit** out);
/* complex_kernel.h:214-265; deferred like gple_real_fit_get_scalars when the create call passed scalars == NULL. */
int gple_complex_fit_get_scalars(gple_complex_fit* fit, gple_complex_fit_scalars* scalars);
int gple_complex_fit_retain(gple_complex_fit* fit);
int gple_complex_fit_release(gple_complex_fit* fit);
size_t gple_complex_fit_size(const gple_complex_fit* fit);
int gple_complex_fit_get(gple_complex_fit* fit, gple_complex_array which, unsigned flags, double* dst);
/* labels: M (re,im) pairs or NULL; prediction / cutoff_prediction: M (re,im) pairs; variance: M. */
int gple_complex_predict(gple_ctx* ctx, const gple_complex_fit* fit, const double* Xs, size_t M, unsigned flags,
	const double* labels, double* prediction, double* variance, double* cutoff_prediction,
	gple_predict_scalars* scalars);

/* ---- loose_function (opt.cpp:441-482) -------------------------------------------------------------- */
/* Objective of the NLopt drivers: LOOCV error of the training set + squared error on the extra set, and
 * (grad != NULL) its gradient; n = 4 -> real kernel, n = 8 -> complex kernel. Labels are (re,im) pairs in
 * both cases (the real kernel takes the real part, opt.cpp:451). make_normal (opt.cpp:420-431) is applied. */
int gple_loose_function(gple_ctx* ctx, const double* x, size_t n, const double* X, const double* y, size_t N,
	const double* X_extra, const double* y_extra, size_t M_extra, double* value, double* grad);

/* The same objective with its data resident: ElementTrainingParameters (opt.cpp:16), i.e. the training set and the extra set
 * an NLopt optimiser carries in its `void* params` across hundreds of evaluations, are uploaded once; an evaluation then moves
 * the parameter vector in and the value (+ gradient) out.  X: 2N, y: N (re,im) pairs, extra set likewise (M_extra may be 0). */
typedef struct gple_objective gple_objective;
int gple_objective_create(gple_ctx* ctx, const double* X, const double* y, size_t N, const double* X_extra, const double* y_extra,
	size_t M_extra, gple_objective** out);
/* loose_function(x, grad, params): n = 4 (real element) or 8 (complex element); grad may be NULL. */
int gple_objective_eval(gple_objective* objective, const double* x, size_t n, double* value, double* grad);
/* One rank's share of an evaluation, for a gradient split over the GPUs of a node (configs[3]: the opt.cpp loop on 4 GPUs, where the complex
 * element alone is the whole step): every rank holds the objective (same data) and fits (replicated, like the grid-sharded predict); rank
 * `part` of `nparts` forms the N^3 derivative products of the parameters ip with ip % nparts == part (the cheap first and last parameters on
 * part 0), predicts its contiguous share of the extra points, and returns its partial value and gradient.  The sum over the parts (one
 * all-reduce of n + 1 doubles) is gple_objective_eval's value and gradient up to the rounding of that sum; make_normal (opt.cpp:420-431:
 * NaN / Inf -> DBL_MAX) is applied by the caller AFTER the sum.  nparts == 1 is gple_objective_eval.  One evaluation at a time per context
 * (the parameter split is a state of the context for the duration of the call). */
int gple_objective_eval_part(gple_objective* objective, const double* x, size_t n, int part, int nparts, double* value, double* grad);
int gple_objective_release(gple_objective* objective);

/* ---- grid-sharded predict for C++ callers (output.cpp:181-233 over several GPUs) ---------------------- */
/* One process per GPU; every rank holds the same fit (replicated: DESIGN.md §7) and calls this with the WHOLE grid Xs (2M).
 * The rank predicts its share of the points — the 128-point blocks rank, rank + world, ... (block-cyclic, so that the live
 * blocks of a mostly empty phase-space grid spread over the ranks, see GPLE_PREDICT_FULL) — and the shares are all-gathered
 * with ncclAllGather on the context's stream (RCCL over xGMI), so that prediction / variance / cutoff_prediction (each nullable, full length M resp.
 * 2M for the complex kernel) are complete on every rank when the call returns (host outputs) or when the stream reaches that
 * point (GPLE_IO_DEVICE).  nccl_comm is the caller's ncclComm_t; the RCCL entry points are resolved at first use from the
 * process (the caller links librccl) or from librccl.so.1.  world == 1 with nccl_comm == NULL is the plain predict. */
/* For callers that shard by hand (contiguous slices, what bench.py / parallel.py do): slice [lo, hi) of M points for rank, and
 * the padded slice length `per` every rank allocates. */
int gple_shard_bounds(size_t M, int rank, int world, size_t* lo, size_t* hi, size_t* per);
/* Callers with another transport (MPI, host staging) plug their own all-gather: same signature and semantics as
 * ncclAllGather(sendbuff, recvbuff, sendcount, datatype = 8 (double), comm, hipStream_t), device buffers, 0 = success.
 * NULL restores RCCL.  Process-wide; set it before the first sharded call of any thread. */
int gple_set_allgather_function(void* fn);
int gple_real_predict_sharded(gple_ctx* ctx, const gple_real_fit* fit, const double* Xs, size_t M, unsigned flags, int rank, int world,
	void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction);
int gple_complex_predict_sharded(gple_ctx* ctx, const gple_complex_fit* fit, const double* Xs, size_t M, unsigned flags, int rank,
	int world, void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction);
/* Weighted deal, for plans that give the ranks unequal shares of an element's grid (the elements of TrainingKernels,
 * predict.cpp:290-360, differ 8x in cost, and 3 + 3 elements do not divide 8 GPUs): out of every cycle of S = sum(weights) consecutive
 * 128-point blocks rank r predicts the weights[r] blocks that follow those of the ranks before it.  weights[rank] == 0: the rank takes no
 * part in this element (fit may be NULL) but still enters the all-gather — every rank of the communicator calls this once per element, in
 * the same order — and receives the full result like everyone else.  weights == NULL is the plain deal of gple_*_predict_sharded. */
int gple_real_predict_dealt(gple_ctx* ctx, const gple_real_fit* fit, const double* Xs, size_t M, unsigned flags, int rank, int world,
	const int* weights, void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction);
int gple_complex_predict_dealt(gple_ctx* ctx, const gple_complex_fit* fit, const double* Xs, size_t M, unsigned flags, int rank, int world,
	const int* weights, void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction);
/* Host-only view of a deal (no device call): the number of points of rank's share, the padded share length every rank allocates, and
 * (indices != NULL, n_local entries) the grid indices of the share in the order the rank predicts them. */
int gple_deal_share(size_t M, int rank, int world, const int* weights, size_t* n_local, size_t* per, size_t* indices);

/* ---- batched point-predict ------------------------------------------------------------------ */
/* The reference evaluates its DistributionFunction (stdafx.h:155) one phase-space point at a time: main.cpp:75-101 constructs a
 * Predictive*Kernel per call, evolve.cpp:298 asks for 8 points per sample, mc.cpp:158-172 for one per Metropolis step.  This entry
 * takes all requests of a tick at once: request r wants the cut-off prediction (get_cutoff_prediction().value(), main.cpp:83,94)
 * of element element_of_request[r] at point points[2r .. 2r+1].  elements[e] names the fit of density-matrix element e: exactly one
 * of real / cplx is set, or neither for an element without a kernel (result 0, main.cpp:86-88).  One predict per element that
 * has requests (gather -> predict -> scatter); out receives n_req (re,im) pairs (imaginary part 0 for real elements).
 * Thread-safe; host pointers only. */
typedef struct gple_element
{
	const gple_real_fit* real;
	const gple_complex_fit* cplx;
} gple_element;
int gple_predict_batch(gple_ctx* ctx, const gple_element* elements, size_t n_elements, const double* points, const int* element_of_request,
	size_t n_req, double* out);

/* ---- the searches of Optimization (opt.cpp:333-355, 517-587, 730-800, 940-1015) ------------------------- */
/* Own implementations behind NLopt's C callback ABIs (NLopt is un-vendored and absent): the reference's objective and
 * constraint callbacks plug in unchanged.  options == NULL: the reference's settings (opt.cpp:344-346). */
typedef double (*gple_objective_fn)(unsigned n, const double* x, double* grad, void* data);                                /* nlopt_func  */
typedef void (*gple_constraint_fn)(unsigned m, double* result, unsigned n, const double* x, double* grad, void* data); /* nlopt_mfunc */
typedef struct gple_opt_options
{
	double xtol_rel, ftol_rel, xtol_abs, ftol_abs; /* 1e-5, 1e-5, 1e-15, 1e-15 */
	double initial_step;                           /* 0.5 (derivative-free search only) */
	int max_eval;                                  /* 0: 400 per free dimension (Nelder-Mead) / 2000 (augmented Lagrangian) */
} gple_opt_options;
/* LN_NELDERMEAD stand-in inside the box [lb, ub] (NULL = unbounded; lb[i] == ub[i] fixes x_i).  x: start point in, minimiser out. */
int gple_minimize_neldermead(gple_objective_fn f, void* data, unsigned n, const double* lb, const double* ub, const gple_opt_options* options,
	double* x, double* fmin, int* n_eval);
/* The same search on the resident objective (loose_function, opt.cpp:441-482; n = 4 or 8) with the simplex vertices evaluated
 * concurrently: objectives[k] are handles on the SAME data created on different contexts (one HIP stream each). */
int gple_objective_minimize_neldermead(gple_objective* const* objectives, size_t n_objectives, size_t n, const double* lb, const double* ub,
	const gple_opt_options* options, double* x, double* fmin, int* n_eval);
/* GN_DIRECT_L stand-in — the global tier (opt.h:54, opt.cpp:336, 1344-1365): Gablonsky & Kelley's locally-biased DIRECT inside the finite
 * box [lb, ub] (lb[i] == ub[i] fixes x_i; x on entry only supplies the fixed coordinates).  options->max_eval == 0: the reference's
 * MaximumEvaluations = 100000 (opt.cpp:339); the tolerances stop the search the way NLopt's do (xtol on the rectangles an iteration
 * divides, ftol on an iteration that improves the minimum). */
int gple_minimize_direct_l(gple_objective_fn f, void* data, unsigned n, const double* lb, const double* ub, const gple_opt_options* options,
	double* x, double* fmin, int* n_eval);
/* The same search on the resident objective with all new rectangle centres of an iteration evaluated concurrently (objectives[k]: handles
 * on the SAME data on different contexts).  is_log (nullable, n entries): coordinates that are logarithms of the parameter they stand for —
 * loose_function_global_wrapper, opt.cpp:489-497; lb, ub and x are in those coordinates. */
int gple_objective_minimize_direct_l(gple_objective* const* objectives, size_t n_objectives, size_t n, const double* lb, const double* ub,
	const unsigned char* is_log, const gple_opt_options* options, double* x, double* fmin, int* n_eval);
/* AUGLAG_EQ stand-in: minimise f subject to h(x) = 0 (m equality constraints, row-major m x n gradient) inside the box. */
int gple_minimize_auglag_eq(gple_objective_fn f, void* fdata, gple_constraint_fn h, void* hdata, unsigned m, unsigned n, const double* lb,
	const double* ub, const gple_opt_options* options, double* x, double* fmin, int* n_eval);

/* ---- the step loop around the GP (NumPES = 2, Dim = 1 as the reference instantiates it) ---------------- */
typedef enum gple_pes_model /* pes.h:27-41; the reference's default TestModel is DAC */
{
	GPLE_PES_SAC = 0, /* Tully I:   simple avoided crossing            */
	GPLE_PES_DAC = 1, /* Tully II:  dual avoided crossing               */
	GPLE_PES_ECR = 2  /* Tully III: extended coupling with reflection  */
} gple_pes_model;
/* adiabatic_potential / adiabatic_force / adiabatic_coupling (pes.cpp:98-155) at M positions:
 * out[6 i + {0..5}] = E0, E1, F(0,0), F(1,0), F(1,1), NAC(0,1). */
int gple_pes_adiabatic(gple_ctx* ctx, int model, const double* x, size_t M, unsigned flags, double* out);

/* One tick of evolve() (evolve.cpp:377-423): the points of the three density-matrix elements (0,0), (1,0), (1,1) are propagated
 * (two half steps forward) and their densities rebuilt by the 3-branch back-propagation of non_adiabatic_evolve_predict
 * (evolve.cpp:184-372), with `distribution` = the cut-off prediction of elements[e] (main.cpp:75-101; 0 for an element without
 * a fit).  density[e].r (2 n_e, interleaved) and density[e].rho (n_e (re,im) pairs) are updated in place; host pointers, or
 * device pointers with GPLE_IO_DEVICE.  All 8 * (n_0 + n_1 + n_2) back-propagated points are predicted in three batches. */
typedef struct gple_points
{
	double* r;
	double* rho;
	size_t n;
} gple_points;
/* flags: GPLE_IO_DEVICE, and GPLE_EVOLVE_NEW_POINTS = new_point_predict (evolve.cpp:425-443) for every point instead of a tick:
 * the points stay where they are, rho (input ignored) receives the density the three-branch back-propagation predicts there
 * from the fits alone — no exact density enters — or 0 where the point does not couple (what is_very_small, evolve.cpp:445-478,
 * and new_element_point_selection, mc.cpp:405-537, evaluate for an element that has no points yet). */
#define GPLE_EVOLVE_NEW_POINTS 0x400u
int gple_evolve(gple_ctx* ctx, const gple_element elements[3], int pes_model, double mass, double dt, gple_points density[3],
	unsigned flags);

/* The same for N-level systems — SURVEY.md §8f N3 "extend non_adiabatic_evolve_predict beyond NumPES == 2" (the reference asserts there,
 * evolve.cpp:367-371); num_pes = 2 or 3, elements and density hold NE = num_pes (num_pes + 1) / 2 entries in the reference's packing order
 * (0,0), (1,0), (1,1), (2,0), (2,1), (2,2): real fits on the diagonal, complex ones off it.  The back-propagation is the N-level form of the
 * operator splitting the two-level code implements: NE momentum branches (the eigen-pairs of the off-diagonal force matrix)
 * x NE source elements of predicted densities per point, one batch per element; at num_pes = 2 it reproduces gple_evolve to rounding.
 * pes_model 0-2: pes.cpp's diabatic_potential as it compiles for num_pes levels (Tully's two surfaces; at three levels plus the uncoupled
 * third diabat at V = 0 that the unfilled matrix entries give); 3 (num_pes = 3 only): a three-state avoided-crossing model of this library,
 * V00 = A tanh(B x), V11 = 0, V22 = -A tanh(B x), V01 = V12 = C sech(D x) with A = 0.02, B = 0.8, C = 0.005, D = 0.5 — the reference has no
 * genuinely three-level model; an id >= GPLE_PES_USER: a user model of gple_pes_define (below) with the same num_pes — at two levels this is the
 * entry point that ticks on a user model, gple_evolve has none.  Adiabatic states: ascending energy, last non-zero component of every
 * eigenvector positive. */
int gple_evolve_n(gple_ctx* ctx, int num_pes, const gple_element* elements, int pes_model, double mass, double dt, gple_points* density,
	unsigned flags);
/* adiabatic_potential / adiabatic_force / adiabatic_coupling (pes.cpp:98-155) for num_pes levels at M positions:
 * out[(num_pes + 2 NE) i + ...] = E (num_pes, ascending) | F lower-packed (NE) | NAC lower-packed (NE; NAC(j, k) = F(j, k) / (E_j - E_k), j > k). */
int gple_pes_adiabatic_n(gple_ctx* ctx, int num_pes, int model, const double* x, size_t M, unsigned flags, double* out);

/* ---- user potentials ------------------------------------------------------------------------------------------------- */
/* A user model is a table of the symmetric diabatic matrix V(x_k) and its derivative V'(x_k) = dV/dx on the uniform grid x_k = x_first + dx k,
 * k < n, registered on a context under an id >= GPLE_PES_USER (at most 16 per context).  It is evaluated as a cubic Hermite interpolant, per
 * entry and in exactly this order (IEEE subtraction and division for s; m_k = dx V'_k is formed once, when the model is defined):
 *     s = (x - x_first) / dx,  k = clamp(floor(s), 0, n - 2),  t = s - k,  D = V_{k+1} - V_k,
 *     c2 = 3 D - (2 m_k + m_{k+1}),  c3 = (m_k + m_{k+1}) - 2 D,
 *     V(x) = V_k + t (m_k + t (c2 + t c3)),  V'(x) = (m_k + t (2 c2 + 3 t c3)) / dx,  F = -V'
 * so that at a node (t = 0) the value is the node's own bits.  Outside the table the potential continues linearly (C^1): for s < 0,
 * V = V_0 + V'_0 (x - x_first), V' = V'_0, and for s > n - 1 the same from the last node.  With nodes taken from a smooth function the error is
 * at most dx^4 / 384 max|V''''| for the value and sqrt(3) / 216 dx^3 max|V''''| for the derivative.
 * A user id is accepted, on the context it was defined on and with the num_pes it was defined with (GPLE_ERR_BAD_ARG otherwise), by
 * gple_pes_adiabatic_n, gple_pes_diabatic_n, gple_evolve_n, gple_dvr_hamiltonian, gple_mqcl_transform / _evolve / _observe, gple_hop_sample / _evolve / _observe / _bin / _outgoing (and the _groups, _dc, _mf, _sqc and _mash forms),
 * gple_grid_survey and gple_grid_reconstruct / _cross.  The two-level entry points gple_pes_adiabatic and gple_evolve keep refusing it: they use the reference's closed
 * forms and operation order, of which a table has none; gple_evolve_n at num_pes = 2 reproduces gple_evolve to rounding and takes their place.
 * Where two surfaces of a user model touch (E_j = E_k) with F_jk != 0 the non-adiabatic coupling is infinite, as its formula says: not guarded.
 *
 * gple_pes_define: V and dV are n x num_pes x num_pes, row-major per node; host pointers, or device pointers with GPLE_IO_DEVICE (the same
 * bits either way).  *model receives the id.  GPLE_ERR_BAD_ARG with nothing registered: num_pes not 2 or 3, n < 2 or n > 2^20, dx not finite
 * or not positive, x_first not finite, a non-finite entry (dx V' included), V or dV not exactly symmetric, a 17th model on the context.  The
 * table is copied into device memory the context owns: the caller's arrays are free when the call returns.
 * gple_pes_undefine: drains the context's stream, then frees the table; the id's slot is reused by a later definition.  gple_ctx_destroy frees
 * what is still defined.  The entry points look the id up under the context's call lock, which gple_pes_undefine holds too: a model undefined
 * by another thread is either refused (GPLE_ERR_BAD_ARG) or still alive for everything the call enqueues.  gple_evolve_n takes the lock twice,
 * around its predicts: undefined in between, it returns GPLE_ERR_BAD_ARG with the densities untouched. */
#define GPLE_PES_USER 16 /* first id of a user model; at most 16 per context */
int gple_pes_define(gple_ctx* ctx, int num_pes, double x_first, double dx, size_t n, const double* V, const double* dV, unsigned flags, int* model);
int gple_pes_undefine(gple_ctx* ctx, int model);
/* The diabatic matrix and force of any model (built-in ids included) at M positions: V[num_pes^2 i + num_pes r + c] and F = -dV/dx likewise. */
int gple_pes_diabatic_n(gple_ctx* ctx, int num_pes, int model, const double* x, size_t M, unsigned flags, double* V, double* F);

/* ---- exact DVR dynamics (schrodinger_equation/ of the reference) ------------------------------------------------------- */
/* The reference's exact quantum dynamics of the same models.  The reflective and periodic boundaries are propagated spectrally
 * (gple_dvr_propagate); the absorbing boundary by powers of the one-step RK4 propagator (gple_dvr_absorber, gple_dvr_propagator,
 * gple_dvr_apply below).  num_pes = 2 or 3, models as gple_evolve_n (TSAC = 3 only at three levels); wavefunctions are num_pes n_grids (re, im) pairs with the index m n_grids + a (general.cpp:126, 137);
 * grid x_a = x_first + dx a (main.cpp:108). */
typedef enum gple_dvr_boundary
{
	GPLE_DVR_REFLECTIVE = 0, /* general.h:92; Colbert-Miller kinetic energy, general.cpp:154-175 */
	GPLE_DVR_PERIODIC = 1    /* general.h:91 (the reference's default); general.cpp:176-198.  The absorbing boundary (general.h:88-93) is no value of this enum: its H is the
	                          * reflective one (the reference's switch falls through to it) and its absorber comes from gple_dvr_absorber */
} gple_dvr_boundary;
/* Hamiltonian_construction (general.cpp:106-200) without the absorbing term: H (dim x dim, dim = num_pes n_grids, real symmetric) holds the
 * diabatic potential on the diagonal grid blocks and the kinetic energy on the diagonal surface blocks, every entry in the reference's
 * operation order.  energies (n_grids x num_pes, ascending) and basis (n_grids x num_pes x num_pes, columns = adiabatic states) are the
 * adiabatic states per grid point (adiabatic_energy general.cpp:296-309, diabatic_to_adiabatic pes.cpp:96-120) exactly as
 * gple_pes_adiabatic_n forms them.  Each output is nullable.  n_grids >= 2, dx > 0, mass > 0. */
int gple_dvr_hamiltonian(gple_ctx* ctx, int num_pes, int model, int boundary, double x_first, double dx, size_t n_grids, double mass,
	unsigned flags, double* H, double* energies, double* basis);
/* Evolution::evolve without ABC (general.cpp:205-252) at T times: psi(t) = C (exp(-i E t / hbar) o c0) with C = eigvec (dim x dim row-major,
 * eigvec[r dim + k] = component r of eigenvector k, what numpy.linalg.eigh returns) and E = eigval (dim).  psi0_or_c0 (dim (re, im) pairs)
 * is c0 = C^T psi0, or psi0 itself with GPLE_DVR_PSI0 (general.cpp:225).  basis (nullable, as gple_dvr_hamiltonian returns it): psi is
 * returned in the adiabatic representation, basis^T psi per grid point (main.cpp:221).  psi: T x dim (re, im) pairs. */
#define GPLE_DVR_PSI0 0x800u
int gple_dvr_propagate(gple_ctx* ctx, int num_pes, size_t n_grids, const double* eigvec, const double* eigval, const double* psi0_or_c0,
	const double* times, size_t T, const double* basis, unsigned flags, double* psi);
/* output_phase_space_distribution (general.cpp:324-411) of T wavefunctions psi (T x num_pes n_grids (re, im) pairs, in the representation
 * the caller wants transformed: the reference passes the adiabatic one, main.cpp:225-232) on the momentum grid p (n_p >= 2 values):
 *   P_ij(x_a, p_b) = dx / (pi hbar) sum_k exp(2 i p_b k dx / hbar) psi_i[a - k] conj(psi_j[a + k]),
 * |k| <= min(a, n_grids - 1 - a) (reflective) or |k| <= n_grids / 3 with indices mod n_grids (periodic).  phase (nullable): the phase.txt
 * layout, T x num_pes^2 (i, j row-major) x n_grids x n_p (re, im) pairs.  averages (nullable, T x 3): (E, x, p) of general.cpp:393-410 from
 * the diagonal elements, E weighted by energies (n_grids x num_pes, the adiabatic energies of gple_dvr_hamiltonian; needed with averages)
 * and p^2 / 2 mass; two calls on the same input return the same bits.  Only the elements j <= i are summed, P_ji = conj(P_ij). */
int gple_wigner(gple_ctx* ctx, int num_pes, int boundary, size_t n_grids, double x_first, double dx, const double* p, size_t n_p,
	const double* psi, size_t T, const double* energies, double mass, unsigned flags, double* phase, double* averages);

/* ---- the absorbing boundary (general.h:88-93): classical RK4 on i hbar dpsi/dt = (H - i W) psi as powers of its one-step propagator ------ */
/* absorbing_potential (pes.cpp:64-93) on the grid x_a = x_first + dx a: W = 0 for xmin < x < xmax, otherwise
 *   W = (2 pi hbar / length)^2 2 / mass (1 / (c - xi)^2 + 1 / (c + xi)^2 - 2 / c^2),  c = sqrt(2) K(1 / sqrt(2)),
 * xi = c (x - xmin) / length for x <= xmin and c (x - xmax) / length for x >= xmax, in the reference's operation order.  (The reference sends
 * x == xmin down the right-hand branch, where W < 0: a gain.  Here W >= 0 everywhere and W is exactly 0 at both edges.)  W: n_grids values.
 * GPLE_ERR_BAD_ARG: a non-finite argument, mass <= 0, length <= 0, xmin >= xmax, or a grid that reaches the pole of W
 * (xmin - x_first >= length or x_last - xmax >= length). */
int gple_dvr_absorber(gple_ctx* ctx, double x_first, double dx, size_t n_grids, double mass, double xmin, double xmax, double length,
	unsigned flags, double* W);
/* The propagator of n_steps classical RK4 steps of length dt (the method general.cpp:233-236 documents) with the constant generator
 * A = -(W + i H) dt / hbar:  U = P4(A)^n_steps,  P4(z) = 1 + z + z^2 / 2 + z^3 / 6 + z^4 / 24, which is what n_steps RK4 steps apply to psi.
 * H (dim x dim) as gple_dvr_hamiltonian returns it; W (nullable: 0): one value per grid point, applied on every surface.  P4 is formed in
 * Horner form, the power by left-to-right binary exponentiation; every complex product is four real products on the fp64 MFMA GEMM
 * (timer: GPLE_TIMER_DVR_POWER).  U: two dim x dim planes, Re then Im, each exactly symmetric.  1 <= n_steps <= 2^30, dt finite,
 * dim <= 65472 (GPLE_ERR_BAD_ARG beyond: the work space of 7 planes of dim^2 doubles is 240 GB there). */
int gple_dvr_propagator(gple_ctx* ctx, int num_pes, size_t n_grids, const double* H, const double* W, double dt, size_t n_steps,
	unsigned flags, double* U);
/* psi[k] = U^(k + 1) psi0 for k < T (T <= 4096), one streaming matrix-vector kernel launch per application with a fixed reduction order: two
 * calls on the same input return the same bits, and so does a call continued from another call's last state.  U as gple_dvr_propagator
 * returns it; psi0: dim (re, im) pairs; basis (nullable) as in gple_dvr_propagate; psi: T x dim (re, im) pairs. */
int gple_dvr_apply(gple_ctx* ctx, int num_pes, size_t n_grids, const double* U, const double* psi0, size_t T, const double* basis,
	unsigned flags, double* psi);

/* Where the absorber took the packet: the absorbed population of n_steps RK4 steps, per side of the box and adiabatic surface, as Hermitian
 * quadratic forms psi^H G_c psi ("What the absorber took").  With P = P4(A) and R_k = P^k (complex symmetric: P^H = conj(P)):
 *   L = I - conj(P) P                       the loss of one step, |psi|^2 - |P psi|^2 = psi^H L psi
 *   Pi_c                                    the projector on channel c = side num_pes + k: the grid points a < n_left (side 0) or a >= n_left
 *                                           (side 1) times the adiabatic state k there, column k of `basis` as gple_dvr_hamiltonian returns it
 *   D_c = (Pi_c L + L Pi_c) / 2             sum_c D_c = L to rounding: the channels add up to the norm loss itself
 *   G_c = sum_{k < n_steps} conj(R_k) D_c R_k
 * formed beside the power by the same left-to-right recurrence (G_c += conj(R) (G_c R) before a squaring, G_c += conj(R) (D_c R) before a
 * multiplication by P), every product on the fp64 MFMA GEMM (timer: GPLE_TIMER_DVR_FLUX, which spans the power's products too).  D_c is not
 * positive semidefinite: a channel's figure may be negative by O((|H| dt)^2) of the loss, and is not clamped.
 * G: 2 num_pes channels of two dim x dim planes (Re, then Im), row-major, G_c(r, q) at r dim + q; Re exactly symmetric, Im exactly
 * antisymmetric with an exactly zero diagonal.  U (nullable): the bits of gple_dvr_propagator for the same arguments.  H, W (nullable), dt,
 * n_steps, dim as gple_dvr_propagator; basis (n_grids x num_pes x num_pes) is required; n_left <= n_grids.  Work space: 13 + 4 num_pes
 * planes of dim^2 doubles. */
int gple_dvr_flux(gple_ctx* ctx, int num_pes, size_t n_grids, const double* H, const double* W, double dt, size_t n_steps, const double* basis,
	size_t n_left, unsigned flags, double* U, double* G);
/* absorbed[t 2 num_pes + c] = Re psi_t^H G_c psi_t for the T diabatic states psi (T x dim (re, im) pairs, 1 <= T <= 4096), unscaled (a
 * population is this times dx).  A wave per row of G_c with lane-strided sums in ascending order and a fixed butterfly, the row results summed
 * in a fixed order by a second kernel; no atomics: a state's figures are the same bits whatever T is and wherever it stands in the call.  A
 * sweep over G serves four states; the sweeps of a call run back to back, 64 states per pair of launches. */
int gple_dvr_flux_apply(gple_ctx* ctx, int num_pes, size_t n_grids, const double* G, const double* psi, size_t T, unsigned flags, double* absorbed);

/* The energy-resolved spectrum of one absorbing run ("The spectrum of one packet"): for every total energy E, with
 * theta = E dt / hbar and K = 2^levels, the discrete half-Fourier transform of the first K steps
 *   psi_e(E) = sum_{k < K} e^{i theta k} P^k psi0 = prod_{j < levels} [I + e^{i theta 2^j} P^(2^j)] psi0          P = P4(A) as gple_dvr_propagator forms it
 * one column per energy, by the power's own squarings: R = P, then per level Y += R (Y o e^{i theta 2^j}) and R = R R (the lower-tile products and
 * the mirror of the power; the thin products are four real ones on the fp64 MFMA GEMM).  theta 2^j is exact and the phase is the sine and cosine
 * of that product.  Nothing steps.  What channel c = side num_pes + k (the Pi_c of gple_dvr_flux) absorbed per unit of energy is
 *   density[e 2 num_pes + c] = psi_e^H D_c psi_e = Re[(Pi_c psi_e)^H psi_e - (P Pi_c psi_e)^H (P psi_e)]
 * unscaled: times dx dt / (2 pi hbar) it is a population per unit energy.  No D_c is formed; a figure may be slightly negative, as those of
 * gple_dvr_flux, and is not clamped.  Over the K energies theta_m = 2 pi m / K the mean of density[m][c] is the figure of gple_dvr_flux with
 * n_steps = K on psi0.  Fixed reduction orders, no atomics: two calls with the same arguments return the same bits.
 * H, W (nullable), dt, dim as gple_dvr_propagator; 0 <= levels <= 30; basis (required) and n_left <= n_grids as gple_dvr_flux; psi0: dim
 * (re, im) pairs; energies: n_E finite values, 1 <= n_E <= 4096, in H's own zero of energy.  psi_e (nullable): n_E x dim (re, im) pairs;
 * remaining (nullable): |P^K psi0|^2, one value.  Timer: GPLE_TIMER_DVR_SPECTRUM.  Work space: the 7 planes of the power and
 * (8 num_pes + 6) dim n_E' doubles, n_E' = n_E rounded up to 64. */
int gple_dvr_spectrum(gple_ctx* ctx, int num_pes, size_t n_grids, const double* H, const double* W, double dt, int levels, const double* basis,
	size_t n_left, const double* psi0, const double* energies, size_t n_E, unsigned flags, double* density, double* psi_e, double* remaining);

/* ---- exact MQCLE dynamics (liouville_equation/ of the reference) ------------------------------------------------------- */
/* The mixed quantum-classical Liouville equation on the square (x, p) grid of n points per axis, evolved in the diabatic basis
 * (main.cpp:153).  num_pes = 2 or 3, models as gple_evolve_n (TSAC = 3 only at three levels), 4 <= n <= 4096.  rho: the phase.txt layout,
 * num_pes^2 elements (a, b) row-major, each n x n (re, im) pairs with x major and p fastest.  Only the elements a <= b are read; every
 * output has rho_ba = conj(rho_ab) and diagonal imaginary parts exactly zero.  x, p: the n grid values.  Adiabatic states: the convention
 * of gple_evolve_n (the reference takes dsyev's raw signs); force basis: eigenvectors of the diabatic force (their signs cancel). */
typedef enum gple_mqcl_basis
{
	GPLE_MQCL_DIABATIC = 0,  /* Representation::Diabatic (general.h) */
	GPLE_MQCL_ADIABATIC = 1, /* Representation::Adiabatic */
	GPLE_MQCL_FORCE = 2      /* Representation::ForceBasis */
} gple_mqcl_basis;
/* basis_transform[from][to] (pes.cpp:360-700): through the diabatic basis, every rotation hermitised.  rho_in and rho_out may alias. */
int gple_mqcl_transform(gple_ctx* ctx, int num_pes, int model, const double* x, size_t n, int from, int to, unsigned flags,
	const double* rho_in, double* rho_out);
/* n_steps Trotter steps Q(dt/2) R(dt/2) P(dt) R(dt/2) Q(dt/2) (main.cpp:192-260) in place on the diabatic rho, every launch on the context's
 * stream.  R shifts along x over the length length_x (xmax - xmin), P along p over length_p (pmax - pmin), with the reference's frequency map
 * (bin k -> k for k < n / 2, else k - n) and the hermitisation after every shift.  mass > 0, dt finite. */
int gple_mqcl_evolve(gple_ctx* ctx, int num_pes, int model, const double* x, const double* p, size_t n, double mass, double length_x, double length_p,
	double dt, size_t n_steps, unsigned flags, double* rho);
/* The adiabatic rho of the diabatic rho_dia (rho_adia, nullable) and calculate_average / calculate_population of it (general.cpp:108-164):
 * averages = (E, x, p) with E weighted by the adiabatic energy plus p^2 / 2 mass, populations (num_pes), all times dx dp.  Two calls on the
 * same input return the same bits. */
int gple_mqcl_observe(gple_ctx* ctx, int num_pes, int model, const double* x, const double* p, size_t n, double mass, double dx, double dp,
	unsigned flags, const double* rho_dia, double* rho_adia, double* averages, double* populations);
/* The absorbing boundary of the MQCLE run: a complex absorbing potential -i W(x), a multiple of the identity in surface space,
 * damps every element pointwise at the order of the MQCLE's own truncation, rho(x, p) <- exp(-2 W(x) tau / hbar) rho(x, p), split symmetrically
 * around a block of tau / dt Trotter steps.  g (n values in [0, 1]) is the half-mask, g_i = 1 - exp(-W(x_i) tau / hbar): gple_mqcl_absorb
 * replaces every stored double of the rows with g_i != 0 by (1 - g_i) times itself (the difference rounded once per row, the product once
 * per double: the bits of the host's (1.0 - g) * rho) and leaves the other rows alone.  What it removes is booked where it is removed: the
 * adiabatic diagonal g_i rho^adia_aa(x_i, p_j), added over the rows i < n_left (side 0) and the others (side 1) in ascending row order and
 * then ADDED to absorbed_p, 2 num_pes n doubles [side][a][j], unscaled (times dx dp and summed over j: the absorbed population of the channel;
 * per j: its outgoing momentum distribution).  The caller zeroes absorbed_p once per run.  A figure may be slightly negative, because rho is
 * no positive density; nothing is clamped.  rho: the diabatic state in the phase.txt layout, in place.  No atomics: two calls on the same input
 * return the same bits.  A device g is copied to the host once per call (the list of absorbing rows needs its length there).
 * gple_mqcl_evolve_absorbing runs n_steps / mask_every blocks of absorb(g), mask_every steps of gple_mqcl_evolve, absorb(g) on the context's
 * stream with no host synchronisation between them; its state and accumulator are the bits of that sequence of separate calls.
 * GPLE_TIMER_MQCL spans the whole call.
 * GPLE_ERR_BAD_ARG, with nothing written: num_pes not 2 or 3, a model gple_mqcl_evolve refuses, n outside its range, n_left > n, mask_every
 * zero or not dividing n_steps, a null array, gple_mqcl_evolve's own cases. */
int gple_mqcl_absorb(gple_ctx* ctx, int num_pes, int model, const double* x, size_t n, const double* g, size_t n_left, unsigned flags, double* rho,
	double* absorbed_p);
int gple_mqcl_evolve_absorbing(gple_ctx* ctx, int num_pes, int model, const double* x, const double* p, size_t n, double mass, double length_x,
	double length_p, double dt, size_t n_steps, size_t mask_every, const double* g, size_t n_left, unsigned flags, double* rho, double* absorbed_p);

/* ---- fewest-switches surface hopping (Tully, J. Chem. Phys. 93, 1061 (1990); no code of the reference's) ------------------ */
/* An ensemble of n independent trajectories, one thread each.  A trajectory is x, p, the DIABATIC amplitudes b (num_pes (re, im) pairs), the
 * active adiabatic surface and a status: 0 running, 1 left through x_left, 2 left through x_right.  num_pes = 2 or 3, models as gple_evolve_n
 * (user ids included).  Arrays: x, p of n doubles; b of n x num_pes (re, im) pairs, trajectory-major; surface, status of n int.  Host pointers,
 * or device pointers with GPLE_IO_DEVICE: the same bits either way.  Random numbers: Philox4x32-10 with key (seed low, seed high); the
 * trajectory index of every counter is the global one, trajectory_offset + i, so a slice of an ensemble evolves to the bits it has inside the
 * whole.  GPLE_ERR_BAD_ARG: num_pes not 2 or 3, a model gple_evolve_n would refuse, n == 0, trajectory_offset + n > 2^32, a mass, dt, sigma_x
 * or sigma_p that is not finite and positive, x_left >= x_right (or not finite), surface0 out of range, a null array. */
#define GPLE_HOP_REVERSE 0x2000u /* gple_hop_evolve: a frustrated hop reverses the momentum (default: it changes nothing) */
/* Draws the ensemble: (u0, u1) = unit53 of the words (0, 1) and (2, 3) of counter (index, 0, 1, 0), rho = sqrt(-2 log(1 - u0)),
 * x = x0 + sigma_x rho cospi(2 u1), p = p0 + sigma_p rho sinpi(2 u1); b = column surface0 of the adiabatic states at x, surface = surface0,
 * status = 0. */
int gple_hop_sample(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
	double sigma_x, double sigma_p, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status);
/* n_steps steps of length dt in place, numbered first_step, first_step + 1, ...: velocity Verlet on the active surface, the amplitudes by the
 * exact exponential of the mid-point diabatic matrix, the hop decision from one uniform number of counter (index, step low word, 0, step high
 * word), the momentum rescaled to conserve p^2 / 2 mass + E (DESIGN.md §17 has the step in full).  A trajectory that leaves (x_left, x_right)
 * is finished and never touched again.  The call carries nothing hidden: evolve(a) then evolve(b, first_step = a) gives the bits of
 * evolve(a + b).  n_steps <= 2^40 (0: nothing happens).  Timer: GPLE_TIMER_HOP. */
int gple_hop_evolve(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double mass, double dt,
	size_t first_step, size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* surface, int* status);
/* Sums over the ensemble, taken in a fixed tree order (two calls give the same bits).  out, 4 num_pes + 3 doubles: the counts
 * [status 0 | 1 | 2][surface] (exact integers), sum |c_k|^2 per adiabatic state k (c = C^T b at the trajectory's x), sum x, sum p,
 * sum (p^2 / 2 mass + E_surface). */
int gple_hop_observe(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, unsigned flags, const double* x, const double* p, const double* b,
	const int* surface, const int* status, double* out);
/* The ensemble's adiabatic density matrix on a uniform phase-space grid ("The ensemble in phase space"), in two calls: the
 * trajectories are added into an integer accumulator (gple_hop_bin), which gple_hop_density turns into the phase.txt layout.  Populations come
 * from the active surface and coherences from the amplitudes (Landry, Falk and Subotnik, J. Chem. Phys. 139, 211101 (2013)): with c = C^T b at
 * the trajectory's x, as gple_hop_observe forms it,
 *     rho_aa(cell) = #{i in cell: surface_i = a} / (n_norm dx dp),   rho_ab(cell) = sum_{i in cell} c_a conj(c_b) / (n_norm dx dp)  (a < b),
 * rho_ba = conj(rho_ab), Im rho_aa = 0 exactly.  Grid: x_k = x_first + dx k, k < n_x, and p_j = p_first + dp j, j < n_p; a point belongs to its
 * nearest grid point, k = floor((x - x_first) / dx + 0.5) (one IEEE subtraction, division, addition and floor, compared with 0 and n_x in
 * double: a NaN or a huge value is outside) and the same for p.
 * acc: num_pes + num_pes (num_pes - 1) planes of n_x n_p integers (x major, p fastest), then the two tallies [binned, outside].  The first
 * num_pes planes count the trajectories per active surface; then, per pair a < b in row-major order, two planes hold the sums of
 * rint(2^32 Re c_a conj(c_b)) and rint(2^32 Im c_a conj(c_b)).  Why integers: integer addition is associative, so acc has the same bits on
 * every call, whatever order the atomic adds arrive in, and a slice added to its complement with GPLE_HOP_ACCUMULATE gives the bits of the
 * whole.  Why 2^32: |c_a conj(c_b)| <= 1/2 for a unit vector, a term is at most 2^31 in magnitude, and the 64-bit sum cannot overflow before
 * 2^32 trajectories (the index space of an ensemble) share one cell with the same extreme term; the rounding of a term is at most 2^-33, nine
 * orders of magnitude below the 1 / sqrt(count) noise of the estimator.
 * gple_hop_bin: only running trajectories (status 0) are binned, or the finished ones too with GPLE_HOP_BIN_ALL.  A selected trajectory off
 * the grid adds one to `outside` and nothing else; one whose surface or status is out of range is skipped, as gple_hop_observe skips it.  The
 * call clears acc first, or adds to what is there with GPLE_HOP_ACCUMULATE.  Timer: GPLE_TIMER_HOP_BIN.
 * gple_hop_density: w = (double)n_norm dx dp, left to right; a count becomes (double)count / w and a coherence sum (double)sum 2^-32 / w
 * (conversions to nearest); the lower planes are formed from the negated sums.  rho: num_pes^2 planes of n_x x n_p (re, im) pairs, the
 * rho_adia of gple_mqcl_observe.  With n_norm the size of the whole ensemble, sum_a sum_cells rho_aa dx dp is the fraction binned.
 * GPLE_ERR_BAD_ARG, with nothing written: num_pes not 2 or 3, a model the other hop calls refuse, n == 0 or n > 2^32 (bin), n_norm == 0
 * (density), n_x or n_p zero, n_x n_p > GPLE_HOP_MAX_CELLS, dx or dp (or w) not finite and positive, x_first or p_first not finite, a null array. */
#define GPLE_HOP_ACCUMULATE 0x4000u /* gple_hop_bin: add to acc (default: acc is cleared first) */
#define GPLE_HOP_BIN_ALL 0x8000u    /* gple_hop_bin: finished trajectories are binned too (default: status 0 only) */
#define GPLE_HOP_MAX_CELLS 268435456ul /* 2^28 cells: 9 planes of (re, im) pairs are 36 GiB, and every index fits the kernels' long with room */
int gple_hop_bin(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
	unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status, long long* acc);
int gple_hop_density(gple_ctx* ctx, int num_pes, size_t n_x, size_t n_p, double dx, double dp, size_t n_norm, unsigned flags, const long long* acc,
	double* rho);
/* Grouped ensembles ("A curve in one launch"): n = n_groups n_per_group trajectories in the same five arrays, trajectory i in
 * group i / n_per_group, its counter index trajectory_offset + i as above: a slice made of whole groups keeps the bits it has inside the
 * whole.  Every group has a packet and a time step of its own, so the branching probabilities at n_groups momenta take three launches.
 * packets (n_groups rows x0, p0, sigma_x, sigma_p) and dt (n_groups) are host tables whatever flags says: the call copies them, and they are
 * free again when it returns.  The five arrays and hops follow GPLE_IO_DEVICE; out is a host array.
 * gple_hop_sample_groups: gple_hop_sample's counters and formulas with the group's packet.  A sigma may be 0 here (Tully's convention, every
 * trajectory of a point at x0 with exactly p0): the coordinate is then the centre exactly, by a select.  With both sigmas positive a trajectory
 * has the bits gple_hop_sample gives for the same global index and packet.
 * gple_hop_evolve_groups: gple_hop_evolve's step with dt[group]; the state of group g afterwards is, bit for bit, what gple_hop_evolve gives
 * for that slice with trajectory_offset + g n_per_group and dt[g], and evolve(a) then evolve(b, first_step = a) gives the bits of evolve(a + b).
 * hops (nullable, n x 2 ints): the hops taken and the frustrated hops (step 6's two outcomes) of every trajectory over the steps of the call
 * are ADDED to what is there.  Timer: GPLE_TIMER_HOP_GROUPS.
 * gple_hop_observe_groups: out is n_groups rows of 4 num_pes + 3 sums; row g has the bits of gple_hop_observe on that slice (every group has
 * workgroups of its own and the same fixed tree; no atomics).
 * GPLE_ERR_BAD_ARG, with nothing written: everything the plain calls refuse; n_groups == 0, n_per_group == 0, n_groups > GPLE_HOP_MAX_GROUPS;
 * n_groups n_per_group overflowing, or exceeding 2^32 together with trajectory_offset; a dt[g] that is not finite and positive; a packet entry
 * that is not finite, or a negative sigma; a null table. */
#define GPLE_HOP_MAX_GROUPS 65536ul
int gple_hop_sample_groups(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset, unsigned long long seed,
	const double* packets, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status);
int gple_hop_evolve_groups(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset, unsigned long long seed,
	double mass, const double* dt, size_t first_step, size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b,
	int* surface, int* status, int* hops);
int gple_hop_observe_groups(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, unsigned flags, const double* x,
	const double* p, const double* b, const int* surface, const int* status, double* out);
/* Decoherence corrections ("Decoherence corrections").  Plain fewest-switches hopping never damps the amplitudes of the surfaces
 * a trajectory is not on (overcoherence).  gple_hop_evolve_dc and gple_hop_evolve_groups_dc are gple_hop_evolve and gple_hop_evolve_groups with
 * a step 6a between the hop (step 6) and the bounds (step 7), selected by `decoherence`.  6a acts on c = C^T b of step 4 with the active
 * surface a and the momentum p as step 6 left them:
 *   GPLE_HOP_DC_NONE              nothing: the kernels and the bits of the calls without _dc.
 *   GPLE_HOP_DC_EDC               the energy-based correction of Granucci and Persico, J. Chem. Phys. 126, 134114 (2007) (Zhu and Truhlar's
 *                                 decay of mixing): E_kin = p^2 / 2 mass, w = 1 if edc_c == 0, else E_kin / (E_kin + edc_c); for every k != a
 *                                 f_k = exp(-dt |E_k - E_a| w / hbar), c_k <- f_k c_k; then c_a <- c_a sqrt(1 + L / |c_a|^2) with
 *                                 L = sum_{k != a} |c_k|^2 (1 - f_k^2) of the old c_k: the norm the vector has is conserved (not pulled to 1),
 *                                 and the sum has no cancellation.  The papers' value is edc_c = 0.1 Hartree.
 *   GPLE_HOP_DC_COLLAPSE_HOP      after a hop that was taken (r >= 0): c_a <- c_a / |c_a|, every other c_k <- 0.
 *   GPLE_HOP_DC_COLLAPSE_ATTEMPT  the same after every wanted hop, taken or frustrated (then onto the unchanged a).
 * In every mode |c_a|^2 == 0 skips 6a for that step.  Where 6a changed c, b <- C c: the phase of c_a is kept, so the step stays invariant under
 * the flip of any column of C.  6a precedes step 7: the step on which a trajectory leaves is corrected too.  edc_c is read in mode EDC only.
 * Everything else (arrays, counters, hops, the call identities, the timers GPLE_TIMER_HOP and GPLE_TIMER_HOP_GROUPS) is that of the calls
 * without _dc.  GPLE_ERR_BAD_ARG, with nothing written: everything those calls refuse; decoherence outside 0 ... 3; in mode EDC an edc_c that
 * is negative or not finite. */
#define GPLE_HOP_DC_NONE 0
#define GPLE_HOP_DC_EDC 1
#define GPLE_HOP_DC_COLLAPSE_HOP 2
#define GPLE_HOP_DC_COLLAPSE_ATTEMPT 3
int gple_hop_evolve_dc(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double mass, double dt,
	size_t first_step, size_t n_steps, double x_left, double x_right, int decoherence, double edc_c, unsigned flags, double* x, double* p, double* b,
	int* surface, int* status);
int gple_hop_evolve_groups_dc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset,
	unsigned long long seed, double mass, const double* dt, size_t first_step, size_t n_steps, double x_left, double x_right, int decoherence,
	double edc_c, unsigned flags, double* x, double* p, double* b, int* surface, int* status, int* hops);
/* Ehrenfest (mean-field) trajectories ("Mean-field (Ehrenfest) trajectories"): the other trajectory baseline.  A trajectory is
 * x, p, the diabatic amplitudes b and its status; it has no active surface, no seed, no step counter and no trajectory offset, and nothing is
 * random.  The ensemble is the one gple_hop_sample (_groups) draws (b starts on column surface0 of C(x)); its surface array is not passed.
 * V, Fd = -V' are the diabatic matrix and force.  The force on a trajectory is the average over its amplitudes,
 *     f(x, b) = sum_i |b_i|^2 Fd_ii + 2 sum_{i<j} Fd_ij Re(conj(b_i) b_j),
 * one running sum: the diagonal terms with i ascending, then the pairs (i, j), i < j, ascending.  One step of length dt, running trajectory:
 *     1  p += f(x, b) dt / 2,  x_new = x + p / mass dt
 *     2  b <- W exp(-i lambda dt / hbar) W^T b,  (lambda, W) the Jacobi eigen-system of (V(x) + V(x_new)) / 2, formed entry by entry as step 2
 *        of gple_hop_evolve forms it
 *     3  p += f(x_new, b_new) dt / 2,  x = x_new
 *     4  x < x_left: status 1, x > x_right: status 2; a finished trajectory is never read or written again
 * The step is time-symmetric (second order) and unitary to rounding.  V and Fd at x_new are those at x of the next step, formed at one place of
 * the loop: evolve_mf(a) then evolve_mf(b) gives the bits of evolve_mf(a + b).  n_steps <= 2^40 (0: nothing happens).
 * gple_hop_evolve_groups_mf: the same step with dt[group], group = i / n_per_group; the state of group g afterwards is, bit for bit, what
 * gple_hop_evolve_mf gives for that slice with dt[g].  Timer of both: GPLE_TIMER_HOP_MF.
 * gple_hop_observe_mf: sums in the fixed tree of gple_hop_observe.  out, 3 num_pes + 6 doubles, with c = C^T b at the trajectory's x:
 * the weights [status 0 | 1 | 2][k] = sum of |c_k|^2 over the trajectories of that status; the counts per status (exact integers); sum x,
 * sum p, sum (p^2 / 2 mass + sum_k |c_k|^2 E_k).  A status outside 0 ... 2 adds to no weight and to no count, as gple_hop_observe skips it.
 * gple_hop_observe_groups_mf: n_groups such rows (out is a host array), row g with the bits of gple_hop_observe_mf on that slice.
 * Arrays, GPLE_IO_DEVICE and the dt table as the calls above.  GPLE_ERR_BAD_ARG, with nothing written: everything gple_hop_evolve,
 * gple_hop_evolve_groups, gple_hop_observe and gple_hop_observe_groups refuse that applies here (num_pes, the model, n, the group sizes, mass,
 * dt or an entry of dt not finite and positive, the bounds, n_steps > 2^40, a null array), and the flag GPLE_HOP_REVERSE. */
int gple_hop_evolve_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, double dt, size_t n_steps, double x_left, double x_right,
	unsigned flags, double* x, double* p, double* b, int* status);
int gple_hop_evolve_groups_mf(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt,
	size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* status);
int gple_hop_observe_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, unsigned flags, const double* x, const double* p,
	const double* b, const int* status, double* out);
int gple_hop_observe_groups_mf(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, unsigned flags,
	const double* x, const double* p, const double* b, const int* status, double* out);
/* The ensemble's adiabatic density from the amplitudes alone ("The ensemble in phase space, from the amplitudes"): gple_hop_bin
 * and gple_hop_density for an ensemble without an active surface.  With c = C^T b at the trajectory's x, as gple_hop_observe_mf forms it,
 *     rho_ab(cell) = sum_{i in cell} c_a conj(c_b) / (n_norm dx dp)   for every a and b, the diagonal included,
 * which is the density of a mean-field (Ehrenfest) ensemble, and for a fewest-switches ensemble the second prescription of Landry, Falk and
 * Subotnik (J. Chem. Phys. 139, 211101 (2013)), populations from the amplitudes, beside the mixed one of gple_hop_bin.  surface is not passed.
 * gple_hop_bin_mf, operation for operation:
 *   selection  the one of gple_hop_observe_mf: status 0, or 0 ... 2 with GPLE_HOP_BIN_ALL; a status out of range is skipped (no term, no tally).
 *   cell       gple_hop_bin's: k = floor((x - x_first) / dx + 0.5), compared with 0 and n_x in double (a NaN or a huge value is outside), the
 *              same for p; a selected trajectory off the grid adds one to `outside` and nothing else.
 *   terms      a binned trajectory adds num_pes^2 integers at its cell: rint(2^32 (Re c_a Re c_a + Im c_a Im c_a)) to plane a, for every a;
 *              and, per pair a < b, rint(2^32 Re c_a conj(c_b)) and rint(2^32 Im c_a conj(c_b)) to the pair's two planes, the very terms of
 *              gple_hop_bin; then one to `binned`.
 * acc has the length and the plane order of gple_hop_bin's, (num_pes + num_pes (num_pes - 1)) n_x n_p + 2 integers; only the meaning of the
 * first num_pes planes differs: they hold sums of 2^32 |c_a|^2 and are no counts.  The integers have the same bits whatever order the adds
 * arrive in, and a slice added to its complement with GPLE_HOP_ACCUMULATE gives the bits of the whole.  The result is defined for amplitudes
 * of unit norm to rounding, as gple_hop_bin's is: a weight term is then at most 2^32 (plus rounding), and since n <= 2^31 one call cannot
 * overflow the signed 64-bit sum of a cell.  Across GPLE_HOP_ACCUMULATE calls that bound (2^31 trajectories in all) is the caller's to keep.
 * Flags: GPLE_IO_DEVICE, GPLE_HOP_ACCUMULATE, GPLE_HOP_BIN_ALL, as for gple_hop_bin.  Timer: GPLE_TIMER_HOP_BIN_MF.
 * gple_hop_density_mf: w = (double)n_norm dx dp, left to right; every sum, the diagonal's too, becomes (double)sum 2^-32 / w; Im rho_aa = +0
 * exactly; the lower planes are formed from the negated sums (+0 where the sum is 0), as gple_hop_density forms them.  With n_norm the size
 * of the whole ensemble, sum_a sum_cells rho_aa dx dp is the fraction binned, to the rounding of the terms.
 * GPLE_ERR_BAD_ARG, with nothing written: everything gple_hop_bin and gple_hop_density refuse that applies here; n > 2^31 (bin); a null array. */
int gple_hop_bin_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
	unsigned flags, const double* x, const double* p, const double* b, const int* status, long long* acc);
int gple_hop_density_mf(gple_ctx* ctx, int num_pes, size_t n_x, size_t n_p, double dx, double dp, size_t n_norm, unsigned flags, const long long* acc,
	double* rho);
/* Symmetrical quasi-classical (SQC) trajectories ("Symmetrical quasi-classical trajectories"): the Meyer-Miller-Stock-Thoss
 * mapping Hamiltonian run classically, with the symmetrical windows of Cotton and Miller.  A trajectory is x, p, the diabatic mapping
 * amplitudes b (num_pes complex numbers, NOT normalised) and its status, in the five arrays of every other ensemble; surface is written by the
 * sample (= surface0) and neither read nor passed afterwards.  With c = C^T b at the trajectory's x (formed as gple_hop_observe forms it),
 * e_k = |c_k|^2 and the action n_k = e_k - gamma, gamma being the zero-point parameter:
 *     H = p^2 / 2 mass + b^dagger V b - gamma tr V = p^2 / 2 mass + sum_k (e_k - gamma) E_k
 *     f(x, b) = [the running sum of gple_hop_evolve_mf, in its order] - gamma (Fd_00 + ... + Fd_{NP-1,NP-1}):
 *               the trace is added left to right, the product formed, then subtracted.
 * The amplitudes obey i db/dt = V b: steps 1 to 4 are those of gple_hop_evolve_mf with this f.  No eigen-system of V(x), nothing random in the
 * step; evolve(a) then evolve(b) gives the bits of evolve(a + b); sum_k |b_k|^2 is conserved to rounding and is not 1.
 * Windows, in the adiabatic representation, in terms of e, with F = num_pes and occ = surface0:
 *   GPLE_HOP_WINDOW_SQUARE    0 < gamma < 1/2 (the windows are disjoint); customary gamma = (sqrt(3) - 1) / 2.
 *       start:  e_k = delta_{k,occ} + 2 gamma u_k
 *       final window of state k:  1 <= e_k <= 1 + 2 gamma  and  e_j <= 2 gamma for all j != k
 *   GPLE_HOP_WINDOW_TRIANGLE  any finite gamma >= 0 (gamma enters H only); customary gamma = 1 / 3.
 *       start:  t = (1 - u_occ)^(1/F) (sqrt at two levels, cbrt at three),  e_occ = 2 - t,  e_j = u_j t for j != occ:
 *               the density (2 - e)^(F-1) on [1, 2] for the occupied state, the others uniform on [0, 2 - e_occ]
 *       final window of state k:  e_k >= 1  and  e_k + e_j <= 2 for all j != k
 * A trajectory belongs to the first k ascending whose window holds it, else to none.
 * Random numbers of the sample (Philox4x32-10, key (seed low, seed high), index = trajectory_offset + i): x and p from the counter
 * (index, 0, 1, 0) by the lines of gple_hop_sample: the same bits for the same index, seed and packet, the sigma == 0 select of the grouped
 * form included.  Level k draws (u_k, v_k) = unit53 of the words (0, 1) and (2, 3) of the counter (index, k, 2, 0).  Then
 * c_k = sqrt(e_k) (cospi(2 v_k) + i sinpi(2 v_k)), b = C(x) c, status 0.
 * gple_hop_sample_groups_sqc: the packets table of gple_hop_sample_groups.  gple_hop_evolve_groups_sqc: dt[group]; a group's state has the
 * bits of gple_hop_evolve_sqc on that slice.  Timer of both evolve calls: GPLE_TIMER_HOP_SQC.  n_steps <= 2^40 (0: nothing happens).
 * gple_hop_observe_sqc: sums in the fixed tree of gple_hop_observe.  out, 4 num_pes + 9 doubles:
 *     [s num_pes + k], s = 0, 1, 2   the trajectories of status s in window k (exact integers)
 *     [3 num_pes + s]                the trajectories of status s
 *     [3 num_pes + 3 + s]            the trajectories of status s in no window (windowed + none = the count of the status)
 *     [3 num_pes + 6 + k]            sum of e_k over the trajectories of status 0 ... 2
 *     then sum x, sum p, sum (p^2 / 2 mass + sum_k (e_k - gamma) E_k), k ascending, over the same trajectories
 * A status outside 0 ... 2 adds nowhere.  gple_hop_observe_groups_sqc: n_groups such rows (out is a host array), row g with the bits of
 * gple_hop_observe_sqc on that slice.  Arrays, GPLE_IO_DEVICE and the tables as the calls above.
 * GPLE_ERR_BAD_ARG, with nothing written: everything gple_hop_sample (_groups), gple_hop_evolve_mf (_groups_mf) and gple_hop_observe_mf
 * (_groups_mf) refuse; window not a GPLE_HOP_WINDOW_*; gamma not finite or negative; for the square window gamma outside (0, 1/2); the flag
 * GPLE_HOP_REVERSE. */
#define GPLE_HOP_WINDOW_SQUARE 0
#define GPLE_HOP_WINDOW_TRIANGLE 1
int gple_hop_sample_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
	double sigma_x, double sigma_p, int surface0, int window, double gamma, unsigned flags, double* x, double* p, double* b, int* surface, int* status);
int gple_hop_sample_groups_sqc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset,
	unsigned long long seed, const double* packets, int surface0, int window, double gamma, unsigned flags, double* x, double* p, double* b,
	int* surface, int* status);
int gple_hop_evolve_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, double dt, size_t n_steps, double x_left, double x_right,
	double gamma, unsigned flags, double* x, double* p, double* b, int* status);
int gple_hop_evolve_groups_sqc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt,
	size_t n_steps, double x_left, double x_right, double gamma, unsigned flags, double* x, double* p, double* b, int* status);
int gple_hop_observe_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int window, double gamma, unsigned flags, const double* x,
	const double* p, const double* b, const int* status, double* out);
int gple_hop_observe_groups_sqc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, int window, double gamma,
	unsigned flags, const double* x, const double* p, const double* b, const int* status, double* out);
/* MASH trajectories, the mapping approach to surface hopping (Mannouch and Richardson, J. Chem. Phys. 158, 104111 (2023); DESIGN.md §17, "MASH
 * trajectories"): a two-level method, num_pes = 2 only.  A trajectory is x, p, the diabatic amplitudes b, its active surface and its status: the
 * five arrays and the layout of gple_hop_sample, so gple_hop_observe and gple_hop_observe_groups serve it unchanged.  The active surface is a
 * deterministic function of the amplitudes; with c = C^T b at the trajectory's x (formed as gple_hop_observe forms it)
 *     side(c) = 1 if |c_1|^2 > |c_0|^2 else 0,  |c_k|^2 = re re + im im      (the sign of the mapping spin's S_z).
 * The step draws no random number: all randomness sits in the sampled amplitudes.
 * gple_hop_sample_mash (Philox4x32-10, key (seed low, seed high), index = trajectory_offset + i): x and p from the counter (index, 0, 1, 0) by
 * the lines of gple_hop_sample: the same bits for the same index, seed and packet, the sigma == 0 select of the grouped form included.  A second
 * counter (index, 0, 3, 0) gives w0 = unit53 of the words (0, 1) and w1 = unit53 of the words (2, 3);  s = sqrt(1 - w0), in (0, 1] with the
 * density 2 s: the weight 2 |S_z| of the population-population correlation function, drawn instead of carried, so that populations are plain
 * counts of the active surface.  With a = surface0 and o = 1 - a:
 *     c_a = sqrt((1 + s) / 2) (real),  c_o = sqrt((1 - s) / 2) (cospi(2 w1) + i sinpi(2 w1)),  b = C(x) c,  surface = surface0,  status = 0.
 * gple_hop_sample_groups_mash: the packets table of gple_hop_sample_groups.
 * gple_hop_evolve_mash, one step of length dt for a running trajectory (a the active surface):
 *     1 - 3  steps 1 to 3 of gple_hop_evolve: the half kick on F_aa, the drift, the amplitudes through the mid-point matrix, the states at
 *            x_new, the second half kick
 *     4  c = C^T b, side_new = side(c): formed at one place, at the start point of a call too; side_old is what the step before formed
 *     5  side_new != side_old and side_new != a:  r = p^2 + 2 mass (E_a - E_side_new);
 *        r >= 0: p = sgn(p) sqrt(r), a = side_new (a hop);  r < 0: p = -p, a stays (a frustrated hop; MASH always reflects, there is no flag).
 *        A crossing back to side_new == a (what follows a reflection) changes nothing
 *     6  x < x_left: status 1, x > x_right: status 2; a finished trajectory is never touched again
 * side_old at the start of a call is recomputed from the stored b and C(x): a call carries nothing hidden, evolve_mash(a) then evolve_mash(b)
 * gives the bits of evolve_mash(a + b).  There is no seed, no first_step and no trajectory_offset.  n_steps <= 2^40 (0: nothing happens).
 * gple_hop_evolve_groups_mash: dt[group], group = i / n_per_group; a group's state has the bits of gple_hop_evolve_mash on that slice.  hops
 * (nullable; 2 n ints where the ensemble lives): the hops taken and the frustrated hops of trajectory i during the call are ADDED to
 * hops[2 i] and hops[2 i + 1].  Timer of both evolve calls: GPLE_TIMER_HOP_MASH.  Arrays, GPLE_IO_DEVICE and the tables as the calls above.
 * GPLE_ERR_BAD_ARG, with nothing written: everything gple_hop_sample (_groups), gple_hop_evolve_mf (_groups_mf) refuse, a null surface,
 * num_pes != 2, and the flag GPLE_HOP_REVERSE. */
int gple_hop_sample_mash(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
	double sigma_x, double sigma_p, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status);
int gple_hop_sample_groups_mash(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset,
	unsigned long long seed, const double* packets, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status);
int gple_hop_evolve_mash(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, double dt, size_t n_steps, double x_left, double x_right,
	unsigned flags, double* x, double* p, double* b, int* surface, int* status);
int gple_hop_evolve_groups_mash(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt,
	size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* surface, int* status, int* hops);
/* What left the box ("What left the box"): the finished trajectories of an ensemble, binned by their outgoing momentum or by the
 * energy their method conserves, per channel.  A trajectory with status 1 left on the left and belongs to side 0, one with status 2 left on
 * the right and belongs to side 1; a channel is (side, adiabatic level k).  A finished trajectory keeps the x, p, b (surface) of its last
 * step, so the calls read the state as the sums read it.  The three calls follow the three forms of the sums; with c = C^T b at the
 * trajectory's x and w_k = |c_k|^2, both formed as the form's observe call forms them:
 *   gple_hop_outgoing      (fewest switches with every decoherence mode, MASH)  weight 1 in channel (side, surface_i);
 *                          q_E = p p / 2 / mass + E_a, the energy term of gple_hop_observe
 *   gple_hop_outgoing_mf   (Ehrenfest)  weight w_k in channel (side, k) for every k;
 *                          q_E = p p / 2 / mass + sum_k w_k E_k, the energy term of gple_hop_observe_mf
 *   gple_hop_outgoing_sqc  (SQC)  weight 1 in channel (side, k), k the window gple_hop_observe_sqc finds for (window, gamma); none: see below;
 *                          q_E = p p / 2 / mass + sum_k (w_k - gamma) E_k, the energy term of gple_hop_observe_sqc
 * each q_E in the expression and the order of that observe call.  axis: GPLE_HOP_AXIS_MOMENTUM, q = p, or GPLE_HOP_AXIS_ENERGY, q = q_E.
 * The grid is q_j = first + step j, j < n_bins; a value belongs to its nearest grid point, j = floor((q - first) / step + 0.5): one IEEE
 * subtraction, one division, one addition, one floor, compared with 0 and n_bins in double (a NaN or a huge value is outside), as the cell
 * of gple_hop_bin.
 * acc: 2 num_pes planes of n_bins 64-bit integers, [side][k][j], then the tallies [binned, outside, running, unassigned]:
 * 2 num_pes n_bins + 4 integers.  Per trajectory, the first that applies:
 *   status 0                                           one to `running`, nothing else
 *   status not 1 or 2, or (gple_hop_outgoing) a surface outside 0 ... num_pes - 1: skipped, as the sums skip it
 *   (gple_hop_outgoing_sqc) no window holds it         one to `unassigned`, nothing else
 *   j outside 0 ... n_bins - 1                         one to `outside`, nothing else
 *   otherwise                                          (long long)rint(2^32 weight) to [side][k][j] of each of its channels, which is exactly
 *                                                      2^32 in one plane for the surface and window forms and a term for every k for the
 *                                                      amplitude form; then one to `binned`
 * The sums are integers for the reason gple_hop_bin's are: the same bits in every call whatever order the atomic adds arrive in, and a
 * slice added to its complement with GPLE_HOP_ACCUMULATE gives the bits of the whole.  The call clears acc first, or adds to what is there
 * with GPLE_HOP_ACCUMULATE.  n <= 2^31 (a weight is at most 2^32 to rounding: one call cannot overflow a signed sum; across accumulating
 * calls the bound is the caller's to keep) and n_bins <= GPLE_HOP_MAX_CELLS / 6.  Flags: GPLE_IO_DEVICE (acc too), GPLE_HOP_ACCUMULATE.
 * Timer of all three: GPLE_TIMER_HOP_OUTGOING.
 * GPLE_ERR_BAD_ARG, with nothing written: whatever the form's observe call refuses (num_pes, the model, n == 0, mass not finite and
 * positive, a null array, for _sqc the window, gamma and the flag GPLE_HOP_REVERSE); n > 2^31; an axis other than the two; n_bins == 0 or
 * above its bound; step not finite and positive; first not finite. */
#define GPLE_HOP_AXIS_MOMENTUM 0
#define GPLE_HOP_AXIS_ENERGY 1
int gple_hop_outgoing(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int axis, double first, double step, size_t n_bins, unsigned flags,
	const double* x, const double* p, const double* b, const int* surface, const int* status, long long* acc);
int gple_hop_outgoing_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int axis, double first, double step, size_t n_bins,
	unsigned flags, const double* x, const double* p, const double* b, const int* status, long long* acc);
int gple_hop_outgoing_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int window, double gamma, int axis, double first, double step,
	size_t n_bins, unsigned flags, const double* x, const double* p, const double* b, const int* status, long long* acc);
/* The ensemble's adiabatic density matrix as a smooth field ("The ensemble in phase space, smoothed"): a Gaussian kernel density
 * estimate in x and p, straight from the ensemble to the phase.txt layout with no integer accumulator in between.  gple_hop_smooth is the
 * smooth form of gple_hop_bin + gple_hop_density (populations from the active surface), gple_hop_smooth_mf that of gple_hop_bin_mf +
 * gple_hop_density_mf (populations from the amplitudes, no surface array).
 * Grid: gple_hop_bin's, x_k = x_first + dx k, k < n_x, and p_j = p_first + dp j, j < n_p (one product and one sum each).  Bandwidths: h_x and
 * h_p, finite and positive.
 * Selection: that of the bin call.  gple_hop_smooth: status 0, or 0 ... 2 with GPLE_HOP_BIN_ALL; a status or a surface out of range is
 * skipped.  gple_hop_smooth_mf: the same without a surface.  A selected trajectory whose x or p is not finite adds one to `nonfinite` and
 * nothing else (the analogue of `outside`); every other selected trajectory adds one to `used` and contributes to every cell.
 * Terms of a used trajectory, with c = C^T b at its x as the bin calls form it: for a pair a < b
 *     re = cre_a cre_b + cim_a cim_b,   im = cim_a cre_b - cre_a cim_b;
 * for the diagonal a, u = 1 where surface == a and 0 elsewhere (gple_hop_smooth), u = cre_a^2 + cim_a^2 (gple_hop_smooth_mf): num_pes^2 real
 * weights u_q per trajectory.
 * Field: t_x = (x_k - x_i) / h_x, g_x = exp(-1/2 t_x t_x) (the product as (-0.5 t_x) t_x), the same for p, and
 *     rho_q(k, j) = s sum_i u_qi g_x g_p,   s = 1 / ((double)n_norm 2 pi h_x h_p), the denominator formed left to right.
 * rho: num_pes^2 planes of n_x x n_p (re, im) pairs, the layout of gple_hop_density.  Im rho_aa = +0 exactly; a lower plane is the conjugate
 * of the upper one, formed from the negated sum (+0 where the sum is 0).  tally (nullable, a host array whatever the flags say): two
 * integers [used, nonfinite].
 * Normalisation: with n_norm the size of the ensemble, sum_a sum_cells rho_aa dx dp = used / n_norm, up to the part of the Gaussians that
 * lies off the grid and a quadrature error of 2 exp(-2 pi^2 (h / d)^2) per axis: 1.4e-9 at h = d, 7.9e-6 at h = 0.75 d, at rounding from
 * h = 1.5 d.  For h_x h_p >= hbar / 2 the field is a Husimi-like, positive picture.
 * Determinism: the sum is floating point.  The split of the trajectory index over workgroups and the order in which partial sums are added
 * depend on (n, n_x, n_p, num_pes) alone: two calls give the same bits, and device pointers give the bits of host pointers.  There is no
 * GPLE_HOP_ACCUMULATE form: a slice plus its complement would not be the whole, bit for bit.
 * Flags: GPLE_IO_DEVICE (the five arrays and rho), GPLE_HOP_BIN_ALL.  Timer: GPLE_TIMER_HOP_SMOOTH.
 * GPLE_ERR_BAD_ARG, with nothing written: num_pes not 2 or 3, a model the other hop calls refuse, n == 0, n > 2^31, n_x or n_p zero,
 * n_x n_p > GPLE_HOP_MAX_CELLS, dx or dp not finite and positive, x_first or p_first not finite, h_x or h_p not finite and positive,
 * n_norm == 0, an s that is not finite and positive, the flags GPLE_HOP_ACCUMULATE and GPLE_HOP_REVERSE, a null array (tally excepted). */
int gple_hop_smooth(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
	double h_x, double h_p, size_t n_norm, unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status,
	double* rho, long long* tally);
int gple_hop_smooth_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
	double h_x, double h_p, size_t n_norm, unsigned flags, const double* x, const double* p, const double* b, const int* status, double* rho,
	long long* tally);

/* ---- exact branching probabilities per energy ----------------------------------------------------------------------------
 * The time-independent problem under every trajectory curve: for each total energy E the coupled-channel Schrodinger equation
 *     psi'' = (2 m / hbar^2)(V(x) - E) psi
 * on the diabatic matrix V of `model` (a built-in id or a user table, as every N-level call), solved by the renormalised Numerov method and read
 * at the asymptotes.  No packet, no absorber, no clock, no random number; closed channels are handled; fourth order in the grid spacing; unitary
 * to rounding.
 * Grid: x_n = x_left + n h, n = 0 ... n_steps, h = (x_right - x_left) / n_steps, V_n = V(x_n).  The potential is taken to be CONSTANT beyond both
 * ends, V = V_0 for n <= 0 and V = V_{n_steps} for n >= n_steps: that is the problem solved, so the box has to hold everything but the flat
 * asymptotes (a user table must be flat where the box ends).
 * Method, with c = (h^2 / 12)(2 m / hbar^2): T_n = c (V_n - E I), U_n = 12 (I - T_n)^-1 - 10 I = (I - T_n)^-1 (2 I + 10 T_n), and for
 * F_n = (I - T_n) psi_n Numerov's rule F_{n+1} - U_n F_n + F_{n-1} = 0.  Per end, (eps, C) the Jacobi eigen-system of its matrix,
 * t_j = c (eps_j - E), u_j = 12 / (1 - t_j) - 10, z_j the root of z + 1 / z = u_j that moves or decays to the right: u_j / 2 + i sqrt(1 - u_j^2 / 4)
 * for |u_j| < 2 (an open channel), else the real root with |z_j| <= 1 (closed); s_j = Im z_j.  z_j^n solves the rule in the constant region
 * exactly, so the match is exact for the discrete problem and its flux is conserved to rounding; the only method error is the O(h^4) of the rule.
 * March from the transmitted side: L_{N+1} = C_R diag(1 / z^R) C_R^T; for n = N ... 0: G = L_{n+1}^-1, L_n = U_n - G; for n = N - 1 ... 0:
 * M <- M G.  At the left, Lambda = C_L^T L_0 C_L, Z = diag(z^L), rho = (Z - Lambda)^-1 (Lambda - Z^-1), tau = C_R^T M C_L (I + rho), and for an
 * open incoming channel i
 *     R_{j<-i} = s^L_j |rho_ji|^2 / s^L_i,   T_{j<-i} = s^R_j |tau_ji|^2 / s^L_i,   defect_i = sum_j (R_{j<-i} + T_{j<-i}) - 1.
 * Channels are the adiabatic surfaces of the ends, ascending.  Incidence is from the left.  A closed final channel j is exactly 0; the column of a
 * closed incoming channel i is NaN, and so is its defect.  An energy exactly at a threshold (|u_j| = 2) is unspecified: finite or NaN.
 * energies (n_energies): total energies in the potential's own zero, the convention of gple_dvr_spectrum.
 * prob: [n_energies][incoming i][side: 0 reflected, 1 transmitted][final j], 2 num_pes^2 doubles per energy.  defect (nullable): [n_energies][i].
 * One thread per energy; 2 x 2 and 3 x 3 inverses are explicit adjugates.  Two calls give the same bits, and device pointers (GPLE_IO_DEVICE:
 * energies, prob, defect) give the bits of host pointers.  Timer: GPLE_TIMER_SCATTER (the march alone).
 * GPLE_ERR_BAD_ARG, with nothing written: num_pes not 2 or 3, a model the other N-level calls refuse, n_energies == 0 or > 2^20, n_steps < 2 or
 * > 2^24, mass not finite and positive, x_left or x_right not finite or x_left >= x_right, an energy that is not finite (device energies are looked
 * at on the host first), a null energies or prob, and a grid too coarse for an end channel: c (E_max - eps_min) >= 1/2 with eps_min the lowest
 * eigenvalue of either end. */
int gple_scatter(gple_ctx* ctx, int num_pes, int model, double mass, double x_left, double x_right, size_t n_steps, size_t n_energies,
	const double* energies, unsigned flags, double* prob, double* defect);

/* generate_markov_chain (mc.cpp:118-165) for n walkers at once on the fitted distribution |cut-off prediction| of `element`:
 * num_steps Metropolis steps with uniform displacements in [-max_displacement, max_displacement) per dimension; r (2n) holds
 * the start points and receives the last points, accept_ratio (nullable, n) the accepted fraction per walker.  Random numbers:
 * Philox4x32-10, counter (walker, step, block, 0), key = seed (the reference's generator is seeded from the clock and shared
 * between threads, mc.cpp:17: no stream of it is reproducible).  Host pointers. */
int gple_markov_chain(gple_ctx* ctx, const gple_element* element, size_t num_steps, double max_displacement, unsigned long long seed,
	double* r, size_t n, double* accept_ratio);
/* The same with every chain recorded (the WholeChain of mc.cpp:118-165, what autocorrelation_optimize_steps mc.cpp:167-285 looks at):
 * chain[(step * n + walker) * 2 + d], step = 0 (start point) .. num_steps. */
int gple_markov_chain_trace(gple_ctx* ctx, const gple_element* element, size_t num_steps, double max_displacement,
	unsigned long long seed, double* r, size_t n, double* accept_ratio, double* chain);

/* ---- negative_log_marginal_likelihood / predict (test/gpr.cpp:499-532, 654-706) -------------------- */
/* Kernel = w_d^2 * Diag + w_g^2 * GaussianARD(weights), x = (w_d, w_g, a_x, a_p) with `a` the diagonal ARD
 * weights = inverse lengths (NOCROSS build, test/gpr.cpp:99,323-326). value = y^T K^-1 y / 2 + sum log L_ii;
 * grad (nullable, 4) = tr[(K^-1 - b b^T) dK] / 2 with the reference's dK (test/gpr.cpp:408-468). */
int gple_nlml(gple_ctx* ctx, const double x[4], const double* X, const double* y, size_t N, double* value,
	double* grad);
/* Mean-only prediction k(x*, X) K^-1 y with the noise kernel excluded off the training set
 * (test/gpr.cpp:384-388, 692-700). */
int gple_nlml_predict(gple_ctx* ctx, const double x[4], const double* X, const double* y, size_t N, const double* Xs,
	size_t M, unsigned flags, double* mean);

/* The default (cross-term) build of test/gpr.cpp (:99-103, 313-321, 436-452): the ARD kernel carries the lower-triangular weight
 * matrix W = [[a, 0], [c, b]], k = w_g^2 exp(-|W^T (x - x')|^2 / 2) = w_g^2 exp(-(x - x')^T W W^T (x - x') / 2);
 * x = (w_d, w_g, a, c, b) in the reference's hyper-parameter order ("rowwise parameters", :313-321).  grad (nullable, 5): the same
 * trace formula with dK/da, dK/dc, dK/db scaled as at :436-452.  Shogun's matrix-weight kernel is restated from the formula
 * comment (:356-367): parity unpinned (Shogun). */
int gple_nlml_cross(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, double* value, double* grad);
int gple_nlml_cross_predict(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, const double* Xs,
	size_t M, unsigned flags, double* mean);

/* ---- many NLML problems in one launch, and the hyper-parameter search of several planes in lock-step on it ----------- */
/* B independent problems of gple_nlml (cross == 0: x = (w_d, w_g, a_x, a_p), x[4] ignored) or gple_nlml_cross (cross != 0: x = (w_d, w_g, a, c, b)),
 * one workgroup each, 1 <= N <= GPLE_NLML_BATCH_MAX_N.  values (B); grads (nullable; 4 B or, with cross, 5 B); weights (nullable: B pointers,
 * entries nullable, N doubles each: b = K^-1 y, what gple_nlml_weights returns); info (nullable, B ints): 0, or the 1-based column of the first
 * non-positive pivot — that problem's value, gradient and weights are NaN and no other problem is touched.  flags: GPLE_IO_DEVICE — X, y,
 * values, grads, info and the arrays `weights` points to are device arrays (`problems` and `weights` themselves are host arrays); the call
 * drains the stream either way.  A problem's results depend on that problem alone: the same bits alone, at any position of a batch of any
 * size, beside problems of any N, with or without gradient or weights.  B == 0, N == 0, N > GPLE_NLML_BATCH_MAX_N, null: GPLE_ERR_BAD_ARG. */
typedef struct gple_nlml_problem
{
	double x[5];
	const double* X;
	const double* y;
	size_t N;
} gple_nlml_problem;
#define GPLE_NLML_BATCH_MAX_N 256
int gple_nlml_batch(gple_ctx* ctx, const gple_nlml_problem* problems, size_t B, int cross, unsigned flags, double* values, double* grads,
	double* const* weights, int* info);
/* optimize of test/gpr.cpp:535-643 for P <= GPLE_NLML_FIT_MAX_PLANES planes at once (host arrays): per plane the library's Nelder-Mead on the NLML
 * value from `start` inside [lb, ub], then gple_minimize_auglag_eq with m = 0 on value + gradient from its minimiser (the two kernel-weight
 * gradients doubled: the reference's dK carries w, not 2 w), then the value once more at the result; a non-finite value counts as DBL_MAX, a
 * non-finite gradient component as 0.  4 (cross == 0) or 5 entries of start / lb / ub / x_out per plane are used; x_out has 5 P slots.  One host
 * thread per plane runs the search; their evaluation requests meet at a rendezvous and every round is ONE gple_nlml_batch launch (a Nelder-Mead
 * step asks for its reflection, expansion and both contractions at once); a plane whose search has ended drops out.  Each plane's iterates,
 * result and count are those of the same search on that plane alone.  n_eval (P): evaluations the searches consumed; weights (nullable: P
 * pointers, entries nullable): K^-1 y at the result. */
typedef struct gple_nlml_fit_plane
{
	const double* X;
	const double* y;
	size_t N;
	double start[5], lb[5], ub[5];
} gple_nlml_fit_plane;
#define GPLE_NLML_FIT_MAX_PLANES 9
int gple_nlml_fit_planes(gple_ctx* ctx, const gple_nlml_fit_plane* planes, size_t P, int cross, const gple_opt_options* options, double* x_out,
	double* f_out, int* n_eval, double* const* weights);

/* ---- reconstruction of a gridded density with the NLML GP (test/main_evolve.cpp:56-179, test/gpr.cpp) ------------------- */
/* The experiment the reference runs on the exact solvers' phase.txt: pick points of every density-matrix element weighted by |rho|, fit the
 * NOCROSS kernel of gple_nlml, predict the element back on the whole grid and compare.  rho is the phase.txt layout of gple_wigner /
 * gple_mqcl_observe: num_pes^2 elements (i, j) row-major, each nx x np (x major, p fastest) (re, im) pairs; num_pes = 2 or 3; nx, np >= 2 and
 * independent; only the elements i <= j are read.  The state is seen as num_pes^2 REAL planes (SuperMatrix, test/io.cpp:25-72): plane
 * q = row num_pes + col is Re rho_ii (row == col = i), Re rho_ij (row = i < col = j) or Im rho_ij (row = j > col = i).  read_density's
 * averaging with the transposed block (io.cpp:62-66) is not restated. */
/* b = K^-1 y (N values) of the kernel x = (w_d, w_g, a_x, a_p): the KInvLbl of predict_phase and of the three calculate_*_from_gpr
 * (test/gpr.cpp:692, 736, 788, 874) — the Gram, factorisation and solve gple_nlml_predict runs internally.  1 <= N <= 4096. */
int gple_nlml_weights(gple_ctx* ctx, const double x[4], const double* X, const double* y, size_t N, unsigned flags, double* b);
/* The same for the cross-term kernel of gple_nlml_cross, x = (w_d, w_g, a, c, b): the weights gple_nlml_cross_predict forms internally. */
int gple_nlml_cross_weights(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, unsigned flags, double* b);
/* One pass over the elements i <= j; out[8 q + ...] per plane q: [0] max, [1] min, [2] sum |v| (the `weight` of gpr.cpp:247), [3] row-major
 * index a np + b of the first strict maximum above 0.0 (set_initial_value, gpr.cpp:119-135) as a double, -1 if none; diagonal planes also
 * [4] sum v dx dp, [5] sum_a rowsum_a E_i(x_a) dx dp, [6] sum_b colsum_b p_b^2 / (2 mass) dx dp (calculate_{population, potential_energy,
 * kinetic_energy}_from_grid, gpr.cpp:42-82; zeros off the diagonal); [7] = 0.  E_i: the adiabatic energies of gple_pes_adiabatic_n, rho in the
 * adiabatic representation.  dx, dp are arguments because the reference uses (x[nx - 1] - x[0]) / nx here (main_evolve.cpp:23).  Two calls on
 * the same input return the same bits. */
#define GPLE_SURVEY_STRIDE 8
int gple_grid_survey(gple_ctx* ctx, int num_pes, int model, const double* rho, const double* x, size_t nx, const double* p, size_t np, double mass,
	double dx, double dp, unsigned flags, double* out);
/* generate_training_set (gpr.cpp:215-291) for plane q.  Draw k = 0, 1, ... takes the uniforms u, u' = unit53 of words (0, 1) and (2, 3) of
 * Philox4x32-10 with counter (k, q, 0x5E1EC7, 0) and key = seed.  uniform == 0 (gpr.cpp:243-265): u_k = u W with W = sum |v| as the device's
 * own blocked running sum ends (u_k >= W by rounding is taken one ulp down), the draw selects the first cell in row-major order whose running
 * sum exceeds u_k — never a cell of zero weight.  uniform != 0 (gpr.cpp:232-240): cell (floor(u nx), floor(u' np)).  The result is the set of
 * distinct cells among the first K draws, K the smallest count that yields n_select of them, in ascending (ix, ip) order: cells (2 n_select
 * ints), X (2 n_select: x[ix], p[ip] interleaved), y (n_select plane values), *n_draws = K (host pointer always).  n_select must not exceed
 * the number of cells (weighted: of cells with |v| > 0) nor 4096, else GPLE_ERR_BAD_ARG.  The reference seeds from the clock: no draw stream
 * of it exists to match. */
int gple_grid_select(gple_ctx* ctx, int num_pes, const double* rho, const double* x, size_t nx, const double* p, size_t np, int q, int uniform,
	size_t n_select, unsigned long long seed, unsigned flags, int* cells, double* X, double* y, size_t* n_draws);
/* predict_phase + mean_squared_error + calculate_*_from_grid (gpr.cpp:654-706, 994-1005, 42-82) of all planes in one pass.  planes[q]: the
 * kernel x = (w_d, w_g, a_x, a_p) (host values), the N training points X (2 N) and the weights b (N, gple_nlml_weights) of plane q; N = 0: the
 * plane is predicted as exactly 0 (gpr.cpp:671-681); 1 <= N <= 4096 otherwise.  scale (nullable = 1; host values): c_q multiplies the
 * prediction (obey_conservation's factor, gpr.cpp:949, 983).  The prediction on the tensor grid is the product of two tables,
 * mu(x_a, p_b) = sum_i [c w_g^2 b_i exp(-(a_x (x_a - X_i))^2 / 2)] [exp(-(a_p (p_b - P_i))^2 / 2)], on the fp64 MFMA — a product of two
 * exponentials where gple_nlml_predict takes one exponential of the summed argument.  pred (nullable): the num_pes^2 real planes, nx x np each.
 * sums[6 q + ...]: [0] sum (c mu - v)^2 (mean_squared_error: a sum, not a mean), diagonal planes [1] sum c mu dx dp, [2] sum c mu E_i(x_a) dx dp,
 * [3] sum c mu p_b^2 / (2 mass) dx dp (zeros off the diagonal), [4] sum (c mu)^2, [5] sum c mu v.  No floating-point atomics: two calls on the
 * same input return the same bits, with or without pred. */
typedef struct gple_recon_plane
{
	double x[4];
	const double* X;
	const double* b;
	size_t N;
} gple_recon_plane;
#define GPLE_RECON_SUMS 6
int gple_grid_reconstruct(gple_ctx* ctx, int num_pes, int model, const double* rho, const double* x, size_t nx, const double* p, size_t np, double mass,
	double dx, double dp, const gple_recon_plane* planes, const double* scale, unsigned flags, double* pred, double* sums);
/* The same pass for the cross-term kernel of gple_nlml_cross (the reference's default build), x = (w_d, w_g, a, c, b) per plane with the weights
 * of gple_nlml_cross_weights: mu(x_a, p_b) = sum_i c_q w_g^2 b_i exp(-Q_i / 2), Q_i = (a dx + c dp)^2 + (b dp)^2, dx = x_a - X_i, dp = p_b - P_i.
 * The bilinear term a c dx dp couples the axes, so no pair of tables exists; per 64 x 64 tile with centre (x_c, p_c) taken from the grid,
 * u = x_a - x_c, v = p_b - p_c, g_i = a (x_c - X_i) + c (p_c - P_i), it splits into an operand of (a, i), an operand of (b, i) and a factor
 * exp(-a c u v) of the cell, and the tile is one fp64 MFMA contraction over i whose operands are generated inside the kernel.
 * A tile of a plane with |a| max|u| or |c| max|v| above 6 (a kernel narrower than about five grid spacings, or strongly sheared) takes one
 * exponential of the summed argument per (cell, point) instead: every finite x is served.  Arguments, N = 0 planes, scale, pred, sums, flags,
 * the timer and the bad-argument rules are gple_grid_reconstruct's; two calls on the same input return the same bits, with or without pred. */
typedef struct gple_recon_cross_plane
{
	double x[5];
	const double* X;
	const double* b;
	size_t N;
} gple_recon_cross_plane;
int gple_grid_reconstruct_cross(gple_ctx* ctx, int num_pes, int model, const double* rho, const double* x, size_t nx, const double* p, size_t np,
	double mass, double dx, double dp, const gple_recon_cross_plane* planes, const double* scale, unsigned flags, double* pred, double* sums);

/* ---- text output: "%g" of device-resident doubles ------------------------------------------------------------------------
 * The reference writes its grids through C++ streams of default precision, one number at a time: output_phase_space_distribution
 * (schrodinger_equation/general.cpp:384-392 and its liouville_equation twin) writes ' ' << re << ' ' << im for every grid point of an element,
 * a newline per element and an empty line per output time; output_phase (output.cpp:180-232) writes blank-separated lines of the predicted grid.
 * gple_format_g produces those bytes from `count` doubles: every number as C's "%g" (6 significant digits, correctly rounded for every double,
 * "-0" for -0.0, "inf" / "-inf", "nan" without a sign), each preceded by one blank; '\n' after every per_line numbers; a second '\n' after every
 * lines_per_block lines (0: never).  GPLE_FORMAT_JOIN: the first number of a line has no blank in front (the layout of output_phase).
 * flags: GPLE_IO_DEVICE — values and text are device pointers — and GPLE_FORMAT_JOIN.  With host pointers the numbers are staged through pooled
 * device memory and only *length bytes come back.  length is a host pointer in either case: the call drains the stream to fill it.  capacity
 * (bytes at text) must be at least gple_format_g_bound(count, per_line, lines_per_block) = 14 count + the newlines, which a line of
 * -1.23457e-308 attains; text carries no terminator.  Two calls on the same input give the same bytes (offsets are sums, nothing is atomic).
 * GPLE_ERR_BAD_ARG with nothing written: per_line == 0, count not a multiple of per_line, count above 2^36, capacity below the bound, a null
 * length, null values or text with count > 0.  There is no host formatter: the conversion runs on the device only (timer: GPLE_TIMER_FORMAT). */
#define GPLE_FORMAT_JOIN 0x1000u
size_t gple_format_g_bound(size_t count, size_t per_line, size_t lines_per_block);
int gple_format_g(gple_ctx* ctx, const double* values, size_t count, size_t per_line, size_t lines_per_block, unsigned flags, char* text,
	size_t capacity, size_t* length);

/* ---- text input: the doubles of "%g" text, on the device ---------------------------------------------------------------------
 * The reference's reconstruction experiment reads phase.txt back with stream extraction, one number at a time (read_density, test/io.cpp:25-72).
 * gple_parse_g converts `length` bytes of text: tokens are separated by blanks (' ', \t, \n, \v, \f, \r); token i in file order gives values[i],
 * the correctly rounded double of  [+-] digits [. digits] [(e|E) [+-] digits]  (at least one mantissa digit; "5." and ".5" are valid) or of
 * inf / infinity / nan in any letter case with an optional sign (nan: the quiet NaN 0x7ff8000000000000 whatever the sign); "-0" is -0.0, an
 * exponent beyond the range gives inf or 0.  Everything gple_format_g writes reads back as C's strtod reads it.  Malformed: anything else (hex
 * floats, a lone sign, "1e", letters), a token of more than 64 bytes, a token with more than 19 significant digits between its leading and its
 * trailing zeros (rejected, not rounded approximately).
 * flags: GPLE_IO_DEVICE — text and values are device pointers (text needs no alignment); otherwise both are staged through pooled device memory.
 * count, lines and bad_offset are host pointers and the call drains the stream to fill them; lines and bad_offset may be NULL.  *count: the
 * tokens of the text; *lines: the lines that hold at least one (a last line needs no '\n').  values == NULL with capacity == 0 only counts (and
 * does not look inside the tokens).  Two calls give the same bits.
 * GPLE_ERR_BAD_ARG: a null count, null text with length > 0, null values with capacity > 0, length above 2^40; *count > capacity, with *count set
 * and nothing written; a malformed token, with *bad_offset the smallest byte offset of one, gple_ctx_last_error naming it and values unspecified.
 * On success *bad_offset = (size_t)-1; an empty or all-blank text is a success with *count = 0.  There is no host parser: the conversion runs on
 * the device only (timer: GPLE_TIMER_PARSE). */
int gple_parse_g(gple_ctx* ctx, const char* text, size_t length, unsigned flags, double* values, size_t capacity, size_t* count, size_t* lines,
	size_t* bad_offset);

#ifdef __cplusplus
}
#endif
#endif /* GPLE_H */
