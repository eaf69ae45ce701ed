// gple_kernels.h — launchers of the non-GEMM device kernels (gple_kernels.hip, gple_predict.hip).
#pragma once
#include "gple_internal.h"

namespace gple
{
	// One squared-exponential kernel  amp * (exp(-((dx*rl0)^2 + (dp*rl1)^2)/2) + n2 * delta).
	// `l` keeps the lengths for the bit-faithful (division) form used when a Gram matrix is materialised.
	struct SEParam
	{
		double amp, n2;
		double l0, l1;
		double rl0, rl1;
	};
	// Kernel functions between "typed" points.  The real GP has one type; the complex (widely linear) GP is run as a
	// real GP on [Re; Im] whose 2N x 2N covariance has blocks  [kR + n/2, kC; kC, kI + n/2]  (DESIGN.md §complex):
	// p[type_a + type_b] with type 0 = real part, 1 = imaginary part  ->  p[0] = RR, p[1] = RI (correlation), p[2] = II.
	struct SEParamSet
	{
		SEParam p[3];
	};

	// cutoff_factor, kernel.h:301-332: 1 where |pred|^2 >= 4 var, 0 where |pred|^2 <= var, the cubic in between (one definition for every epilogue)
	__device__ __forceinline__ double cutoff_value(double pred_square, double abs_pred, double var)
	{
		if (pred_square >= 4.0 * var) return 1.0;
		if (pred_square <= var) return 0.0;
		const double a = abs_pred / sqrt(var);
		return (3.0 * 2.0 - 2.0 * a - 1.0) * ((a - 1.0) * (a - 1.0)) / 1.0;
	}
	// the factorisation's info word in the fit's scalar block (gple_capi.h, SDEV_INFO): negative = the one-launch scheme gave up, everything derived
	// from the factor is NaN until the host has repeated it
	__device__ __forceinline__ bool fit_gave_up(const double* s_dev) { return *reinterpret_cast<const int*>(s_dev + 31) < 0; }
	// exp(x) for finite x <= 0 (the argument of a squared-exponential kernel), fp64, < 1 ulp:
	// x = k ln2 + r (Cody-Waite with an FMA), |r| <= ln2/2, degree-12 Taylor/Horner, scaling by v_ldexp_f64 (which
	// handles the gradual underflow for x < -708).  No special-case branches.
	__device__ __forceinline__ double exp_nonpos(double x)
	{
		x = fmax(x, -1100.0); // below that the result is 0 anyway; keeps the int conversion in range
		const double kd = rint(x * 1.4426950408889634074);
		double r = fma(kd, -6.93147180369123816490e-01, x);
		r = fma(kd, -1.90821492927058770002e-10, r);
		double p = 2.08767569878680989792e-09; // 1/12!
		p = fma(p, r, 2.50521083854417187751e-08);
		p = fma(p, r, 2.75573192239858906526e-07);
		p = fma(p, r, 2.75573192239858906526e-06);
		p = fma(p, r, 2.48015873015873015873e-05);
		p = fma(p, r, 1.98412698412698412698e-04);
		p = fma(p, r, 1.38888888888888888889e-03);
		p = fma(p, r, 8.33333333333333333333e-03);
		p = fma(p, r, 4.16666666666666666667e-02);
		p = fma(p, r, 1.66666666666666666667e-01);
		p = fma(p, r, 0.5);
		p = fma(p, r, 1.0);
		p = fma(p, r, 1.0);
		return ldexp(p, static_cast<int>(kd));
	}

	// ---- training side ---------------------------------------------------------------------------------------
	// ys[i] = s * y[i*stride + offset] for i < N (0 for N <= i < Np), s = 10 / max_i |label_i|, written to *s_out.
	// complex_abs != 0: |label| is the complex modulus of the (re,im) pair and both halves are produced:
	// ys[0..Np) = s*re, ys[Np..2Np) = s*im.
	hipError_t launch_prep_labels(hipStream_t s, const double* y, int stride, int complex_abs, int N, int Np, double* ys, double* s_out,
		const double* X, double* Xt, int nscal);
	// K_pad (n_total x n_total, ld) of the typed training set: n_total = Np (real) or 2*Np (complex, split at Np);
	// points Xt (N interleaved); padded rows/cols get the identity.
	// ys != nullptr: K has n_total + 64 rows; row n_total receives ys (length n_total), the 63 rows below it zeros
	hipError_t launch_gram_train(hipStream_t s, const double* Xt, int N, int Np, int n_total, SEParamSet ps, double* K, long ld,
		const double* ys = nullptr);
	// u = T * ys (lower triangular T, n x n): partial sums then reduction. part: (n/256) * n doubles.
	hipError_t launch_trmv_lower(hipStream_t s, const double* T, long ldt, int n, const double* ys, double* part, double* u);
	// v[k] = sum_i T(i,k) u[i],  w[k] = sum_i T(i,k)^2 ; optionally wx[k] = sum_i T(i,k) T(i,k+shift) (complex: diag of Mxy).
	// info != nullptr: a negative *info (the factorisation gave up, gple_chol.hip) turns v, w, wx into NaN
	hipError_t launch_colpass(hipStream_t s, const double* T, long ldt, int n, const double* u, double* v, double* w, int shift,
		double* wx, const int* info = nullptr);
	// raw sums for the real fit: out[0]=sum (v/w)^2, out[1]=sum v, out[2]=sum x v, out[3]=sum p v, out[4]=sum ys v
	// out[0..4]: the five sums of a real fit; qpart != nullptr: also *qout = sum of the nq per-block partials of a quadratic form
	// (launch_quadform_partials), saving the separate reduction launch
	hipError_t launch_real_fit_sums(hipStream_t s, const double* Xt, const double* ys, const double* v, const double* w, int N, double* out,
		const double* qpart = nullptr, int nq = 0, double* qout = nullptr);
	hipError_t launch_quadform_partials(hipStream_t s, const double* Xt, int N, SEParam p, const double* a, const double* b, int fdim, double* part);
	// out[0] = sum_ij a_i k(x_i,x_j) b_j over i,j < N with the bit-faithful SE kernel p (amp folded in, no noise)
	// fdim >= 0 multiplies every entry by ((x_i,d - x_j,d)/l_d)^2 / l_d: the kernel's derivative over l_d (kernel.cpp:99-160)
	hipError_t launch_quadform(hipStream_t s, const double* Xt, int N, SEParam p, const double* a, const double* b, int fdim, double* part,
		double* out);

	// ---- complex derivative path (gple_cderiv.hip): everything in the real [Re; Im] embedding ------------------------
	// One block of a derivative matrix: amp * G(l) * (c0 + c1 * ((x_d - x'_d)/l_d)^2 / l_d); active == 0 -> zero block.
	struct DSpec
	{
		double amp, c0, c1;
		double l0, l1;
		int dim, active;
	};
	// blocks indexed by type_a + type_b: 0 = Re-Re, 1 = Re-Im (both off-diagonal blocks), 2 = Im-Im
	struct DSpecSet
	{
		DSpec b[3];
	};
	// dC (n x n, padded with zeros) of the typed training set
	hipError_t launch_typed_deriv_gram(hipStream_t s, const double* Xt, int N, int Np, int n, DSpecSet spec, double* D);
	// Diagonals of M dC M for a dC with ONE zero diagonal block (every sub-kernel parameter of the complex GP, build_dspecs): with the
	// non-zero diagonal block A and the off-diagonal block B of dC, E = A M_a and F = B M_b (Np x n each; M_a = the rows of M on A's side,
	// M_b the others; roff = first row of M_a) give
	//   diag(M dC M)_i          = sum_j M_a(j, i) (E + 2 F)(j, i)                                   i < n
	//   (M dC M)(i, Np + i)      = sum_j M_a(j, i) (E + F)(j, Np + i) + M_a(j, Np + i) F(j, i)        i < Np
	// out_diag (n) and out_off (Np) receive alpha times these: half the flops of the full product dC M.
	hipError_t launch_cderiv_diag(hipStream_t s, const double* M, long ldm, int roff, const double* E, const double* F, long lde, int Np, int n, double alpha,
		double* out_diag, double* out_off);
	// cnt parameters that share roff in one launch: E, F advance by ef_stride per parameter, the outputs by diag_stride / off_stride
	hipError_t launch_cderiv_diag_batch(hipStream_t s, int cnt, const double* M, long ldm, int roff, const double* E, const double* F, long lde, int Np, int n,
		double alpha, double* out_diag, double* out_off, long ef_stride, long diag_stride, long off_stride);
	// out[ip] (ip = 0..7) = TrainingComplexKernel::ErrorDerivatives (complex_kernel.cpp:444-474) from the embedded quantities:
	// w (weights, n), wd (diag M, n), wx (diag of the Re-Im block, Np) and their derivatives dw (8 x n), dwd (8 x n), dwx (8 x Np)
	hipError_t launch_complex_deriv_sums(hipStream_t s, const double* w, const double* wd, const double* wx, const double* dw, const double* dwd,
		const double* dwx, int N, int Np, double* out8);
	// nine sums of one generated kernel X = amp G(l): out[3 * pair + var], pair in {(a,a), (b,b), (a,b)}, var in {1, f_0, f_1}
	hipError_t launch_multi_quadform(hipStream_t s, const double* Xt, int N, SEParam p, const double* a, const double* b, double* part, double* out9);
	// ya = X a, yb = X b for the generated kernel X (N x N); part: 2 * ceil(N/256) * N doubles
	hipError_t launch_aux_matvec(hipStream_t s, const double* Xt, int N, SEParam p, const double* a, const double* b, double* part, double* ya,
		double* yb);
	// out[4 * ip + q] = (ga.dw_x, gb.dw_y, ga.dw_y, gb.dw_x)[q] for ip = 0..7 with dw_x = dw[ip*n .. ], dw_y = dw[ip*n + Np ..]
	hipError_t launch_aux_dots(hipStream_t s, const double* ga, const double* gb, const double* dw, int N, int Np, int n, double* out32);
	// PredictiveComplexKernel::ErrorDerivatives (complex_kernel.cpp:648-668) from the 15 accumulator planes of the derivative pass
	hipError_t launch_predict_deriv_finish_complex(hipStream_t s, const double* acc, int m_rows, int m_split, const double* q, int M, double self,
		double s0, const double* s_dev, const double* labels, double* part, double* out8);

	// ---- derivative path (gple_deriv.hip) ------------------------------------------------------------------------
	// D0, D1 (n x n, ld = n, padded with zeros): dK/dl_d of the training Gram, zero diagonal (kernel.cpp:123-157, 190)
	hipError_t launch_deriv_gram(hipStream_t s, const double* Xt, int N, int n, SEParam p, double* D0, double* D1);
	// y = alpha * A x for a full column-major n x n matrix (n multiple of 256); part: (n/256) * n doubles
	hipError_t launch_gemv(hipStream_t s, const double* A, long lda, int n, const double* x, double alpha, double* part, double* y);
	// out[i] = alpha * sum_j A(j,i) B(j,i + shift)   (columns i with i + shift < n; shift = 0: plain column dots)
	hipError_t launch_coldot(hipStream_t s, const double* A, long lda, const double* B, long ldb, int n, int shift, double alpha,
		double* out);
	hipError_t launch_scale(hipStream_t s, const double* x, double alpha, int n, double* y);
	// up to three independent items of the above in ONE launch (small matrices: a derivative fit at the sizes the reference runs is a string of 4-5 us launches)
	hipError_t launch_gemv_batch(hipStream_t s, int n, int cnt, const double* const* A, long lda, const double* const* x, const double* alpha, double* part,
		double* const* y); // n <= 1024; part: cnt * (n / 256) * n doubles
	hipError_t launch_coldot_batch(hipStream_t s, int n, int cnt, const double* const* A, long lda, const double* const* B, long ldb, int shift, const double* alpha,
		double* const* out);
	hipError_t launch_scale_batch(hipStream_t s, int cnt, const double* const* x, const double* alpha, const int* n, double* const* y);
	// raw sums of the real derivative path: out[ip] = error derivative (kernel.cpp:381-400), out[4 + ip] = sum_i dv[ip][i]
	hipError_t launch_real_deriv_sums(hipStream_t s, const double* v, const double* w, const double* dv, const double* dwd, int N, int ld,
		double* out);
	// PredictiveKernel::ErrorDerivatives (kernel.cpp:524-542) from the per-row accumulators of the derivative generation pass
	hipError_t launch_predict_deriv_finish_real(hipStream_t s, const double* acc, int m_rows, const double* q, int M, double self, double sf,
		const double* s_dev, const double* labels, double* part, double* out4);

	// ---- KernelBase / cutoff ----------------------------------------------------------------------------------
	// p.amp = sf*sf, p.n2 = sn*sn; sf and sn are passed too because the derivative formulas use them unsquared.
	hipError_t launch_gram_rect(hipStream_t s, const double* L, int R, const double* Rt, int C, int same, SEParam p, double sf, double sn,
		double* K, double* dK);
	// ComplexKernelBase (gple_cgram.hip): K (R x C), K~ (R x C (re,im) pairs, nullable), dK (8 x R x C, nullable), dK~ (8 x R x C pairs, nullable)
	hipError_t launch_complex_gram(hipStream_t s, const double theta[8], const double* L, int R, const double* Rt, int C, int same, double* K,
		double* Kt, double* dK, double* dKt);
	hipError_t launch_sum(hipStream_t s, const double* part, int n, double* out);
	hipError_t launch_cutoff(hipStream_t s, const double* pred, int is_complex, const double* var, int M, double* factor);

	// ---- NLML path of test/gpr.cpp (gple_nlml.hip); x = (w_d, w_g, a, c, b): ARD weight matrix [[a, 0], [c, b]] --------------
	hipError_t launch_nlml_gram(hipStream_t s, const double* Xt, int N, int n, const double x[5], double* K);
	hipError_t launch_nlml_value(hipStream_t s, const double* T, long ldt, const double* y, const double* b, int N, double* out);
	hipError_t launch_nlml_grad(hipStream_t s, const double* Xt, int N, const double* W, long ldw, const double* b, const double x[5], double* part,
		double* out5);
	// part: nlml_predict_ksplit(M, N) * M doubles of partial sums
	int nlml_predict_ksplit(int M, int N);
	hipError_t launch_nlml_predict(hipStream_t s, const double* Xs, int M, const double* Xt, int N, const double* b, const double x[5], double* part, double* mean);

	// ---- B independent NLML problems in one launch, one workgroup each (gple_nlml_batch.hip) ---------------------------------
	constexpr int NLML_BATCH_MAX_N = 256;
	constexpr unsigned NLML_BATCH_GRAD = 1u; // NlmlBatchProblem::flags: this problem's gradient is wanted
	struct NlmlBatchProblem
	{
		double x[5];     // (w_d, w_g, a, c, b)
		const double* X; // device, 2 N
		const double* y; // device, N
		double* weights; // device, N: b = K^-1 y (nullable)
		long work;       // this problem's offset into the work pool, nlml_batch_work_doubles(N) doubles
		int N;
		unsigned flags;
	};
	inline size_t nlml_batch_work_doubles(size_t N)
	{
		const size_t n = round_up(N, CHOL_NB);
		return 2 * n * n; // the Gram that becomes its factor | the inverse factor, transposed
	}
	// values (B) | grads (grad_width = 4: (w_d, w_g, a, b), 5: all; per problem, written for NLML_BATCH_GRAD problems) | info (B): 0 or the
	// 1-based column of the first non-positive pivot, whose problem returns NaN everywhere
	hipError_t launch_nlml_batch(hipStream_t s, const NlmlBatchProblem* problems, int B, double* work, double* values, double* grads, int grad_width,
		int* info);

	// ---- step loop around the GP (gple_evolve.hip): Tully models, MQCLE propagation, Metropolis ---------------------------------
	hipError_t launch_pes(hipStream_t s, const double* x, int M, int model, double* out6);
	// query-list layout of one tick: off[s] = first point of source element s, qoff[e][s] / qlen[e] = rows of target e's list
	void evolve_layout(const int n[3], long qoff[3][3], long qlen[3], int off[3], int new_points = 0);
	hipError_t launch_evolve_prepare(hipStream_t s, const double* r, const int n[3], double mass, double dt, int model, double* r_new,
		unsigned char* coupled, double* const q[3], int new_points = 0);
	hipError_t launch_evolve_combine(hipStream_t s, const double* r_old, const double* r_new, const double* rho_old, const unsigned char* coupled,
		const int n[3], double mass, double dt, int model, const double* const pred[3], double* rho_new, int new_points = 0);
	hipError_t launch_mc_propose(hipStream_t s, const double* r, int n, unsigned step, unsigned long long seed, double d, double* r_prop);
	hipError_t launch_mc_weight(hipStream_t s, const double* pred, int is_complex, int n, double* weight);
	hipError_t launch_mc_accept(hipStream_t s, double* r, const double* r_prop, const double* pred, int is_complex, int n, unsigned step,
		unsigned long long seed, double* weight, unsigned* accepted);

	// ---- predict ------------------------------------------------------------------------------------------------
	struct PredictArgs
	{
		const double* Xs; // test points, M interleaved pairs
		int M;            // number of test points
		int m_rows;       // rows of the (typed) test set: Mh (real) or 2*Mh (complex), Mh = round_up(M, 128)
		int m_split;      // rows >= m_split are imaginary-part rows (== m_rows for the real GP)
		int m_split_few;  // few-points path only: the same boundary in its compact row numbering
		const double* Xt; // training points (N valid, readable up to n_split entries)
		int N;
		int n_total; // Np or 2*Np
		int n_split; // Np
		const double* T;
		long ldt;
		const double* v; // n_total weights (K^-1 y in the typed basis)
		const double* dv; // derivative pass: nparam x n_total derivatives of v (real: 4, complex embedding: 8), or nullptr
		double* dacc;     // derivative pass: accumulator planes of m_rows each
		                  //   real:    7 = [K* v, K* dv_0..3, (dK*/dl_0) v, (dK*/dl_1) v]
		                  //   complex: 15 = [c w, c dw_0..7, dc_1..6 w]
		int complex_deriv;      // 1: use dspec (complex embedding)
		DSpecSet dspec[6];      // derivative blocks of the parameters 1..6 (sub-kernel magnitudes and lengths)
		double* q;       // m_rows: || T k*_m ||^2
		double* mu;      // m_rows: k*_m . v
		SEParamSet ps;
		// What the caller consumes decides how much of the variance contraction has to run (gple_predict.hip, launch_predict_q):
		int mean_only;                   // 1: neither the variance nor the cut-off factor is consumed (PredictiveKernel's Error alone, kernel.cpp:522,
		                                 //    uses the UNCUT mean): no K*, no contraction, q = 0
		double cut_thr;                  // > 0: the variance only decides the cut-off factor (ErrorDerivatives, kernel.cpp:527): a point with
		                                 //    |mu|^2 >= cut_thr = 4 k(x*,x*) >= 4 var has factor 1 whatever q is (kernel.h:301-332) and is not contracted
		double prune_thr;                // > 0: rows with |k*|^2 below it are not contracted (gple_predict.hip, Prune)
		unsigned long long* prune_stats; // device, 4 words: [0] += ceil(live rows / 128), [1] += rows / 128, [2] work-queue counter, [3] live-row count
		// PredictiveKernel's epilogue (kernel.cpp:496-522) for a kernel that can do it itself (predict_fused256_kernel): fin_sdev != nullptr offers it,
		// launch_predict_q says through *finished whether it was taken (q and mu are then not written).  Real GP without labels only.
		const double* fin_sdev; // the fit's scalar block: [0] the label scale, [31] the factorisation's info word
		double fin_self;        // k(x*, x*)
		double *fin_mean, *fin_var, *fin_cut; // M each, nullable
	};
	// Rolling K* scratch of the predict path (HBM): bounded so that M x N never has to exist at once.
	constexpr size_t PREDICT_SCRATCH_BYTES = size_t(4) << 30;
	// doubles of scratch launch_predict_q needs for `a`; *chunk_rows = rows of the typed test set handled per pass
	size_t predict_scratch_doubles(const PredictArgs& a, int* chunk_rows, bool* few_rows);
	// a handful of test points (<= 16 typed rows, no derivatives): triangular mat-vecs with K* generated on the fly
	bool predict_is_few(const PredictArgs& a);
	size_t predict_few_scratch_doubles(const PredictArgs& a);
	hipError_t launch_predict_few(hipStream_t s, const PredictArgs& a, double* scratch);
	// fills a.q and a.mu; per chunk: kstar_gen_kernel then the contraction kernel (bracketed by the context's chunk timers)
	hipError_t launch_predict_q(Ctx* ctx, hipStream_t s, const PredictArgs& a, double* scratch, int chunk_rows, bool few_rows, bool* finished = nullptr);
	// real finish: var = self - q, cutoff, cut = mu*cf/s ; optional labels -> err_out[0] += sum (mu - s t)^2
	hipError_t launch_predict_finish_real(hipStream_t s, const double* q, const double* mu, int M, double self, const double* s_dev,
		const double* labels, double* mean, double* var, double* cut, double* err_out);
	// complex finish: rows [0,M) real part, rows [m_split, m_split+M) imaginary part
	hipError_t launch_predict_finish_complex(hipStream_t s, const double* q, const double* mu, int M, int m_split, double self,
		const double* s_dev, const double* labels, double* mean, double* var, double* cut, double* err_out);
	// ---- the potential a kernel evaluates (gple_pes_n.h): a built-in id (table == nullptr), or a user model of the context's registry with its
	// table in device memory: per node V | V' | dx V' (PES_TABLE_PLANES planes of num_pes^2 doubles, row-major), nodes at x_first + dx k, k < n.
	// Passed by value into the kernels; a built-in id converts implicitly, so the launchers below take either
	constexpr int PES_TABLE_PLANES = 3;
	struct PesModel
	{
		int id, n;
		const double* table;
		double x_first, dx;
		__host__ __device__ PesModel(int builtin = 0): id(builtin), n(0), table(nullptr), x_first(0.0), dx(1.0) {}
	};
	// V and F = -V' of the model at M positions, num_pes^2 doubles each per position (gple_pes_diabatic_n)
	hipError_t launch_pes_diabatic_n(hipStream_t s, int num_pes, const double* x, int M, PesModel model, double* V, double* F);
	// dst (n nodes of the layout above) from V and dV (n x num_pes^2 each); *bad (an int, zeroed by the caller) becomes non-zero when an entry
	// is not finite or a matrix not exactly symmetric
	hipError_t launch_pes_table_build(hipStream_t s, int num_pes, const double* V, const double* dV, size_t n, double dx, double* dst, int* bad);
	// ---- N-level step loop (gple_evolve_n.hip): NumPES = 2 or 3, elements in the packing order (0,0), (1,0), (1,1), (2,0), ... ----
	// adiabatic quantities: out[(NP + 2 NE) i + ...] = E (NP) | F lower-packed (NE) | NAC lower-packed (NE)
	hipError_t launch_pes_n(hipStream_t s, int num_pes, const double* x, int M, PesModel model, double* out);
	// rows of every element's query list: NE branches of every point of every element
	void evolve_layout_n(int num_pes, const int* n, long* qlen);
	hipError_t launch_evolve_prepare_n(hipStream_t s, int num_pes, const double* r, const int* n, double mass, double dt, PesModel model, double* r_new,
		double* const* q, int new_points);
	hipError_t launch_evolve_combine_n(hipStream_t s, int num_pes, const double* r_new, const double* rho_old, const int* n, double mass, double dt, PesModel model,
		const double* const* pred, double* rho_new, int new_points);
	// ---- exact DVR dynamics (gple_dvr.hip): num_pes = 2 or 3, dim = num_pes n, boundary = gple_dvr_boundary ---------------------------
	// H: dim x dim (symmetric); energies: n x num_pes; basis: n x num_pes x num_pes (columns = adiabatic states); either may be null
	hipError_t launch_dvr_hamiltonian(hipStream_t s, int num_pes, PesModel model, int boundary, double x_first, double dx, int n, double mass, double* H);
	size_t dvr_states_work_doubles(int num_pes, int n);
	hipError_t launch_dvr_states(hipStream_t s, int num_pes, PesModel model, double x_first, double dx, int n, double* energies, double* basis, double* work);
	// work layout (doubles, ld = dim rounded up to 64): C (ld x ld, row-major, zero padded) | Z, Y (ld x round_up(2T, 64) each) | input (ld x 64:
	// v = psi0 or c0 (dim (re, im) pairs) split into columns re, im) | c0 (ld x 64).  psi: T x dim (re, im) pairs, adiabatic when basis != null
	size_t dvr_propagate_work_doubles(int num_pes, int n, int T);
	hipError_t launch_dvr_propagate(hipStream_t s, int num_pes, int n, const double* eigval, const double* v, const double* times, int T, const double* basis,
		bool from_psi0, double* work, double* psi);
	// Wigner transform: table = exp(2 i p y / hbar) (wigner_table_doubles), P: T x num_pes^2 x n x np (re, im) pairs, p fastest
	int wigner_half_range(int boundary, int n);
	size_t wigner_table_doubles(int boundary, int n, int np);
	hipError_t launch_wigner_table(hipStream_t s, int boundary, int n, const double* p, int np, double dx, double* table);
	hipError_t launch_wigner(hipStream_t s, int num_pes, int boundary, int n, double dx, const double* table, int np, const double* psi, int T, double* P);
	size_t wigner_avg_work_doubles(int num_pes, int T);
	hipError_t launch_wigner_averages(hipStream_t s, int num_pes, int n, double x_first, double dx, const double* p, int np, const double* energies,
		double mass, const double* P, int T, double* work, double* averages);
	// ---- the absorbing boundary (gple_dvr_power.hip): U = P4(A)^s, A = -(W + i H) dt / hbar, as complex symmetric planes of ld x ld, ld = dim rounded up to 64
	hipError_t launch_dvr_absorber(hipStream_t s, double x_first, double dx, int n, double mass, double xmin, double xmax, double length, double* W);
	// a complex matrix as its (Re, Im) planes, column-major with the leading dimension ld; the planes lie wherever the owner of the memory put them
	struct DvrPlanes
	{
		double *re = nullptr, *im = nullptr;
	};
	// successive pieces of a work buffer, in the order they are taken; with base == nullptr only their total is counted (the dvr_*_work_doubles)
	struct DvrCarve
	{
		double* base;
		size_t used = 0;
		double* take(size_t doubles) { used += doubles; return base ? base + (used - doubles) : nullptr; }
		DvrPlanes planes(size_t plane) { return {take(plane), take(plane)}; } // a braced list is evaluated left to right
	};
	// Z = beta Z + X Y, or conj(X) Y with conj_x: X ld x ld, Y and Z ld x cols.  Four real products through launch_gemm, always in the order
	// Xr Yr, Xi Yi (into Re Z), Xr Yi, Xi Yr (into Im Z); the three-multiplication form costs accuracy.  lower: only the lower tiles of Z (cols == ld;
	// the caller mirrors, launch_dvr_mirror).  Z may alias neither operand
	hipError_t dvr_complex_product(hipStream_t s, DvrPlanes X, DvrPlanes Y, DvrPlanes Z, long ld, long cols, double beta, bool conj_x, bool lower);
	// the lower triangle of Z over the upper one, Z(r, c) <- Z(c, r); hermitian: conj Z(c, r), and the diagonal of Im Z exactly 0
	hipError_t launch_dvr_mirror(hipStream_t s, DvrPlanes Z, long ld, bool hermitian);
	// Z = X X for a complex symmetric X (lower tiles and the mirror): one squaring of the power
	hipError_t launch_dvr_square(hipStream_t s, DvrPlanes X, DvrPlanes Z, long ld);
	// the grid of the kernels that take a thread per row and a block row per column of an ld x ld plane
	inline dim3 dvr_plane_grid(long ld) { return dim3(static_cast<unsigned>((ld + 255) / 256), static_cast<unsigned>(ld)); }
	constexpr long DVR_POWER_MAX_LD = 65472; // ld <= 65535 = the largest gridDim.y (a column per block row in the set-up kernels); 7 ld^2 doubles of work are 240 GB there
	// the work of the power: dvr_power_layout carves it, dvr_power_work_doubles is the end of the same carving
	struct DvrPowerWork
	{
		double* G;        // Im A, ld x ld
		DvrPlanes P;      // P4(A)
		DvrPlanes buf[2]; // the Horner factors, then the squarings and multiplications of the walk in turn
		double* d;        // Re A, a diagonal of ld values
		size_t doubles;
	};
	DvrPowerWork dvr_power_layout(double* work, long ld);
	size_t dvr_power_work_doubles(int num_pes, int n);
	// P4(A) into w.P (H: dim x dim, W: n values or null), by the generator kernel and three Horner steps that use both buffers of w
	hipError_t launch_dvr_p4(hipStream_t s, int num_pes, int n, const double* H, const double* W, double dt, const DvrPowerWork& w);
	// with flux: the quadratic forms of the absorbed population beside the power (gple_dvr_flux.hip)
	struct DvrFlux
	{
		const double* basis; // n x num_pes x num_pes
		int n_left;          // the grid points a < n_left are side 0
		double* work;        // dvr_flux_work_doubles
	};
	// *result: U, planes inside work.  GPLE_TIMER_DVR_POWER of ctx spans the products (the Horner steps and the walk); with flux GPLE_TIMER_DVR_FLUX instead
	hipError_t launch_dvr_power(Ctx* ctx, hipStream_t s, int num_pes, int n, const double* H, const double* W, double dt, long n_steps, double* work,
		DvrPlanes* result, const DvrFlux* flux = nullptr);
	// psi[k] = U^(k + 1) psi0, k < T; U: two dim x dim planes; scratch: T x dim pairs when basis != null (the diabatic states), unused otherwise
	hipError_t launch_dvr_apply(hipStream_t s, int num_pes, int n, const double* U, const double* psi0, int T, const double* basis, double* scratch, double* psi);
	// ---- what the absorber took (gple_dvr_flux.hip): per channel c = (side, surface) the Hermitian G_c, by the recurrence of the power's walk
	struct DvrFluxWork
	{
		DvrPlanes L, D, T; // the loss of one step, one channel's D_c, the inner product of a sandwich
		DvrPlanes G_c[6];  // the 2 num_pes channels
		size_t doubles;
	};
	DvrFluxWork dvr_flux_layout(double* work, long ld, int num_pes);
	size_t dvr_flux_work_doubles(int num_pes, int n);
	// the flux recurrence beside one walk of launch_dvr_power, which calls the three steps below; with flux == nullptr (the plain power) they do nothing
	struct DvrFluxRun
	{
		hipStream_t s;
		int num_pes, n;
		long ld;
		const DvrFlux* flux;
		DvrFluxWork w; // flux->work carved
	};
	hipError_t dvr_flux_first_step(const DvrFluxRun& f, DvrPlanes P);      // L = I - conj(P) P and G_c = D_c: one step
	hipError_t dvr_flux_before_square(const DvrFluxRun& f, DvrPlanes R);   // G_c += conj(R) G_c R: the steps m .. 2m - 1 are the first m seen through R = P^m
	hipError_t dvr_flux_before_multiply(const DvrFluxRun& f, DvrPlanes R); // G_c += conj(R) D_c R: one more step after R
	// channel c of flux.work without its padding, row-major, into out (2 num_pes channels of two dim x dim planes)
	hipError_t launch_dvr_flux_export(hipStream_t s, int num_pes, int n, const DvrFlux& flux, double* out);
	// absorbed[t 2 num_pes + c] = Re psi_t^H G_c psi_t; G as launch_dvr_flux_export writes it; partial: dvr_flux_apply_work_doubles
	constexpr int DVR_FLUX_CHUNK = 64; // states per pair of launches (the row results of a chunk are DVR_FLUX_CHUNK x 2 num_pes x dim doubles)
	size_t dvr_flux_apply_work_doubles(int num_pes, int n, int T);
	hipError_t launch_dvr_flux_apply(hipStream_t s, int num_pes, int n, const double* G, const double* psi, int T, double* partial, double* absorbed);
	// ---- the spectrum of one absorbing run (gple_dvr_spectrum.hip): Y(E) = sum_{k < 2^levels} e^{i E dt k / hbar} P4^k psi0 per energy, by the power's squarings
	struct DvrSpectrum
	{
		int num_pes, n, levels, n_left, n_E;
		const double *H, *W;   // as launch_dvr_p4 (W nullable)
		double dt;
		const double* basis;   // n x num_pes x num_pes
		const double* psi0;    // dim (re, im) pairs
		const double* energies; // n_E
		double* power_work;    // dvr_power_work_doubles: P4 stays in its P, its buf[0] and buf[1] take the squarings
		double* work;          // dvr_spectrum_work_doubles: X = Y | Pi_c Y (two planes of ld x (1 + 2 num_pes) nep), P X (the same), T (two planes of ld x nep)
		double* density;       // n_E x 2 num_pes: Re[(Pi_c Y)^H Y - (P Pi_c Y)^H (P Y)]
		double* psi_e;         // nullable: n_E x dim (re, im) pairs
		double* remaining;     // nullable: |P4^(2^levels) psi0|^2
	};
	size_t dvr_spectrum_work_doubles(int num_pes, int n, int n_E);
	// every pointer a device pointer.  GPLE_TIMER_DVR_SPECTRUM of ctx spans P4, the squarings, the thin products, the projection and the reduction
	hipError_t launch_dvr_spectrum(Ctx* ctx, hipStream_t s, const DvrSpectrum& g);
	// ---- exact MQCLE dynamics (gple_mqcl.hip): num_pes = 2 or 3, 4 <= n <= 4096, rho: num_pes^2 x n x n (re, im) pairs, x major ------------
	// tables (mqcl_table_doubles): per x C | E | U | lambda | Q phases of one Q(tq), then (spectral) chirp (n), twiddles (M / 2), chirp spectrum (M)
	int mqcl_fft_length(int n);
	size_t mqcl_table_doubles(int num_pes, int n);
	hipError_t launch_mqcl_tables(hipStream_t s, int num_pes, PesModel model, const double* x, int n, double tq, bool spectral, double* tables);
	struct MqclEvolveArgs
	{
		int num_pes, n, M;
		long n_steps;
		double* rho;        // the caller's full layout, in place (only the planes a <= b are read)
		double* transposed; // num_pes (num_pes + 1) / 2 x n x n (re, im) pairs
		const double* table;
		const double* p;
		const double *chirp, *tw, *bhat; // filled by launch_mqcl_evolve from table
		double mass, length_x, length_p, dt;
	};
	hipError_t launch_mqcl_evolve(hipStream_t s, const MqclEvolveArgs& g);
	hipError_t launch_mqcl_lower(hipStream_t s, int num_pes, int n, double* rho);
	hipError_t launch_mqcl_transform(hipStream_t s, int num_pes, int n, int from, int to, const double* tables, const double* in, double* out);
	size_t mqcl_observe_work_doubles(int num_pes, int n);
	hipError_t launch_mqcl_observe(hipStream_t s, int num_pes, int n, const double* tables, const double* x, const double* p, double mass, double dxdp,
		const double* rho, double* adia, double* work, double* out);
	// ---- the absorbing boundary of the MQCLE run (gple_mqcl_absorb.hip): rho <- (1 - g_i) rho on the rows with g_i != 0, what leaves booked ----
	// rows (mqcl_absorb_rows_doubles): the ascending list of those rows, written by launch_mqcl_absorb_rows; count: their number (the host's)
	size_t mqcl_absorb_rows_doubles(int n);
	size_t mqcl_absorb_slab_doubles(int num_pes, int n, int count);
	hipError_t launch_mqcl_absorb_rows(hipStream_t s, const double* g, int n, int* rows);
	struct MqclAbsorbArgs
	{
		int num_pes, n, n_left, count;
		PesModel model;
		const double *x, *g; // n each
		const int* rows;
		double* slab;       // mqcl_absorb_slab_doubles: g_i rho^adia_aa(x_i, p_j) as [row][a][j]
		double* rho;        // num_pes^2 x n x n (re, im) pairs, diabatic, masked in place
		double* absorbed_p; // 2 x num_pes x n, [side][a][j]: the slab's rows are added to it
	};
	hipError_t launch_mqcl_absorb(hipStream_t s, const MqclAbsorbArgs& a);

	// ---- trajectory ensembles (gple_hop.hip): num_pes = 2 or 3, one thread per trajectory, every pointer a device pointer ----
	struct HopEnsemble // x, p: n doubles; b: n x num_pes (re, im) pairs; surface, status: n ints; counters use the index offset + i
	{
		int num_pes;
		long n;
		unsigned long long offset, seed;
		double *x, *p, *b;
		int *surface, *status;
	};
	// Fewest switches.  Grouped ensembles ("A curve in one launch"): e.n = n_groups n_per_group, trajectory i belongs to group
	// i / n_per_group.  packets: n_groups rows (x0, p0, sigma_x, sigma_p), a sigma of exactly 0 gives the centre exactly; dt: n_groups time
	// steps; hops (nullable): n x 2 ints, the hops taken and the frustrated hops of the call are added.
	// decoherence ("Decoherence corrections") is a GPLE_HOP_DC_* of include/gple.h: NONE launches the kernels without step 6a,
	// 1 ... 3 the instantiations with it, which read the mode (wave-uniform) at run time; edc_c is read in mode 1 only
	hipError_t launch_hop_sample(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0);
	hipError_t launch_hop_sample_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0);
	hipError_t launch_hop_evolve(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, unsigned long long first_step, long n_steps,
		double x_left, double x_right, bool reverse, int decoherence = GPLE_HOP_DC_NONE, double edc_c = 0.0);
	hipError_t launch_hop_evolve_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, unsigned long long first_step,
		long n_steps, double x_left, double x_right, bool reverse, int* hops, int decoherence = GPLE_HOP_DC_NONE, double edc_c = 0.0);
	// The sums of include/gple.h, per method hop_observe*_width(num_pes) of them: out is one row of sums, from one partial row per wave of the first
	// stage in work (hop_observe_work_doubles(width, 1, n)); the grouped forms give n_groups rows, row g with the bits of the plain launch on the
	// group alone (every group has workgroups of its own), from hop_observe_work_doubles(width, n_groups, n_per_group) of work
	constexpr int hop_observe_width(int num_pes) { return 4 * num_pes + 3; }
	constexpr int hop_observe_mf_width(int num_pes) { return 3 * num_pes + 6; }
	constexpr int hop_observe_sqc_width(int num_pes) { return 4 * num_pes + 9; }
	size_t hop_observe_work_doubles(int width, long n_groups, long n_per_group);
	hipError_t launch_hop_observe(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double* work, double* out);
	hipError_t launch_hop_observe_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, double* work, double* out);
	// Ehrenfest (mean-field) trajectories ("Mean-field (Ehrenfest) trajectories"): of the ensemble only x, p, b and status are read or
	// written (surface may be null; offset and seed are not used).  The force is b^dagger Fd b, the amplitudes move as in launch_hop_evolve
	hipError_t launch_hop_evolve_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right);
	hipError_t launch_hop_evolve_groups_mf(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right);
	hipError_t launch_hop_observe_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double* work, double* out);
	hipError_t launch_hop_observe_groups_mf(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, double* work, double* out);
	// Symmetrical quasi-classical trajectories ("Symmetrical quasi-classical trajectories"): window is a GPLE_HOP_WINDOW_* of
	// include/gple.h, gamma the zero-point parameter.  The samples write all five arrays (surface = surface0); the step and the sums read and
	// write x, p, b and status only (surface may be null), the step being the mean-field one with the force b^dagger Fd b - gamma tr Fd
	hipError_t launch_hop_sample_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0, int window,
		double gamma);
	hipError_t launch_hop_sample_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0, int window,
		double gamma);
	hipError_t launch_hop_evolve_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right, double gamma);
	hipError_t launch_hop_evolve_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right, double gamma);
	hipError_t launch_hop_observe_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, int window, double gamma, double* work, double* out);
	hipError_t launch_hop_observe_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, int window, double gamma,
		double* work, double* out);
	// MASH trajectories ("MASH trajectories"): two levels only (any other num_pes is hipErrorInvalidValue).  The ensemble is the
	// five arrays of launch_hop_sample; the samples draw the amplitudes of their own, the step has no seed, no step counter and no offset, and
	// counts hops taken and frustrated into hops (nullable) as launch_hop_evolve_groups does.  The sums are launch_hop_observe's
	hipError_t launch_hop_sample_mash(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0);
	hipError_t launch_hop_sample_groups_mash(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0);
	hipError_t launch_hop_evolve_mash(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right);
	hipError_t launch_hop_evolve_groups_mash(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right, int* hops);
	// the uniform grid of gple_hop_bin: a point belongs to its nearest grid point, floor((x - x_first) / dx + 0.5) and the same for p
	struct HopGrid
	{
		double x_first, dx, p_first, dp;
		long n_x, n_p;
	};
	// planes of n_x n_p integers in acc, before its two tallies [binned, outside]: num_pes counts, then (re, im) per pair a < b
	constexpr int hop_bin_planes(int num_pes) { return num_pes + num_pes * (num_pes - 1); }
	// adds the selected trajectories (status 0, or every valid status with bin_all) to acc by 64-bit integer atomics: any order, the same bits
	hipError_t launch_hop_bin(hipStream_t s, const HopEnsemble& e, PesModel model, const HopGrid& g, bool bin_all, long long* acc);
	// rho (num_pes^2 planes of n_x n_p (re, im) pairs) from acc: counts / w, coherence sums 2^-32 / w
	hipError_t launch_hop_density(hipStream_t s, int num_pes, long cells, double w, const long long* acc, double* rho);
	// the same two from the amplitudes alone (e.surface is not read): the first num_pes planes of acc are sums of rint(2^32 |c_a|^2), which the
	// density scales by 2^-32 / w as it scales the coherence sums.  A weight is at most 2^32 to rounding: the caller keeps e.n <= 2^31
	hipError_t launch_hop_bin_mf(hipStream_t s, const HopEnsemble& e, PesModel model, const HopGrid& g, bool bin_all, long long* acc);
	hipError_t launch_hop_density_mf(hipStream_t s, int num_pes, long cells, double w, const long long* acc, double* rho);
	// the axis of gple_hop_outgoing: q_j = first + step j, j < n_bins, of the momentum or (energy != 0) of the energy term of the method's sums;
	// a value belongs to its nearest grid point, floor((q - first) / step + 0.5)
	struct HopAxis
	{
		double first, step;
		long n_bins;
		int energy;
	};
	// integers of acc: 2 num_pes planes [side][level] of n_bins, then the tallies [binned, outside, running, unassigned]
	constexpr size_t hop_outgoing_words(int num_pes, size_t n_bins) { return 2 * static_cast<size_t>(num_pes) * n_bins + 4; }
	// adds the finished trajectories to acc by 64-bit integer atomics, in the three forms of the sums (include/gple.h): by the active surface
	// (e.surface is read), by the amplitudes' weights (e.n <= 2^31 is the caller's to keep), by the window that holds them
	hipError_t launch_hop_outgoing(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, const HopAxis& g, long long* acc);
	hipError_t launch_hop_outgoing_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, const HopAxis& g, long long* acc);
	hipError_t launch_hop_outgoing_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, int window, double gamma, const HopAxis& g, long long* acc);
	// The smoothed density of gple_hop_smooth ("The ensemble in phase space, smoothed").  The split of the trajectory index: chunks
	// of `chunk` trajectories (a multiple of 16; the last one shorter), n_chunks of them, npad = n rounded up to 16; a function of
	// (num_pes, n, n_x, n_p) alone.  work: hop_smooth_work_doubles() doubles, the terms (x, p and num_pes^2 weights, npad each) and then the
	// chunks' partial planes, at most max(2^24, num_pes^2 n_x n_p) doubles of them
	struct HopSmoothPlan
	{
		long npad, chunk, n_chunks, tiles_x, tiles_p;
		int groups;
	};
	HopSmoothPlan hop_smooth_plan(int num_pes, long n, long n_x, long n_p);
	size_t hop_smooth_work_doubles(int num_pes, long n, long n_x, long n_p);
	// the terms of every trajectory into work (zeros for the ones that do not contribute) and the tallies [used, nonfinite] added to tally;
	// mean_field: the diagonal weights from the amplitudes and e.surface not read
	hipError_t launch_hop_smooth_terms(hipStream_t s, const HopEnsemble& e, PesModel model, bool mean_field, bool bin_all, double* work, unsigned long long* tally);
	// the contraction and the finish: rho = scale sum_i u_i g_x g_p in the phase.txt layout, from the terms in work
	hipError_t launch_hop_smooth(hipStream_t s, int num_pes, long n, const HopGrid& g, double h_x, double h_p, double scale, double* work, double* rho);

	// ---- coupled-channel scattering (gple_scatter.hip): the renormalised Numerov march of gple_scatter, one thread per energy ----
	// c = (h^2 / 12)(2 m / hbar^2) with h = (x_right - x_left) / n_steps, formed left to right: the factor of T_n = c (V_n - E)
	double scatter_step_constant(double mass, double x_left, double x_right, long n_steps);
	// the table of a call: the upper triangle of V_n, row by row, for n = 0 ... n_steps, then the ascending eigenvalues of V_0 and of V_{n_steps}
	size_t scatter_table_doubles(int num_pes, long n_steps);
	hipError_t launch_scatter_table(hipStream_t s, int num_pes, PesModel model, double x_left, double x_right, long n_steps, double* table);
	// prob: n_E x num_pes (incoming) x 2 (reflected, transmitted) x num_pes (final); defect (nullable): n_E x num_pes.  Device pointers
	hipError_t launch_scatter(hipStream_t s, int num_pes, double c, long n_steps, const double* table, const double* energies, long n_E, double* prob,
		double* defect);

	// ---- reconstruction of a gridded density (gple_recon.hip; test/gpr.cpp): num_pes = 2 or 3, rho: num_pes^2 x nx x np (re, im) ----
	constexpr int RECON_SURVEY_BLOCKS = 64, RECON_SURVEY_VALUES = 7; // row blocks of the survey, values per plane and block
	constexpr int RECON_MAX_PLANES = 9, RECON_MAX_N = 4096, RECON_SUMS = 6;
	constexpr int RECON_SCAN_CHUNK = 4096; // cells per workgroup of the selection's running sum
	size_t recon_survey_work_doubles(int num_pes);
	hipError_t launch_recon_survey(hipStream_t s, int num_pes, PesModel model, const double* rho, const double* x, int nx, const double* p, int np, double mass,
		double dxdp, double* work, double* out);
	// selection: running sum of |v| of plane q (within[c]: inclusive within its chunk; offsets[k]: sum of the chunks before k, offsets[nchunks] = W;
	// counts[nchunks]: cells of non-zero weight), the draws [k0, k0 + nk) with first-occurrence marking in mark (cells ints, INT_MAX = never drawn),
	// the count (state: [0] distinct cells so far, [1] K or 0; chosen: the first n_select distinct cells in draw order) and the gather
	long recon_scan_chunks(long cells);
	hipError_t launch_recon_scan(hipStream_t s, int num_pes, const double* rho, long cells, int q, double* within, double* offsets, long long* count);
	hipError_t launch_recon_draw(hipStream_t s, const double* within, const double* offsets, long cells, int nx, int np, int q, int uniform,
		unsigned long long seed, unsigned k0, unsigned nk, int* draw_cell, int* mark);
	hipError_t launch_recon_count(hipStream_t s, const int* draw_cell, const int* mark, unsigned k0, unsigned nk, int n_select, int* state, int* chosen);
	hipError_t launch_recon_gather(hipStream_t s, int num_pes, const double* rho, const double* x, int nx, const double* p, int np, int q, const int* chosen,
		int n_select, int* cells, double* X, double* y);
	// reconstruction: the two tables of every plane, the MFMA contraction with its epilogue (one record per tile) and the final sum
	struct ReconPlane
	{
		const double* X; // 2 N interleaved
		const double* b; // N
		double* Ax;      // rows_x x Npad, k contiguous (diagonal kernel only)
		double* Ep;      // rows_p x Npad (diagonal kernel only)
		double coef, ax, ap; // c w_g^2, a_x, a_p (cross-term kernel: the diagonal a, b of W = [[a, 0], [c, b]])
		double cross;        // the cross weight c of W (cross-term kernel only)
		int N, Npad;
	};
	struct ReconArgs
	{
		ReconPlane plane[RECON_MAX_PLANES];
		const double* rho;
		const double* x;
		const double* p;
		double* energy; // nx x num_pes adiabatic energies
		double* pred;   // nullable
		double* records;
		double* sums;
		double mass, dxdp;
		PesModel model;
		int num_pes, nx, np, rows_x, rows_p;
	};
	size_t recon_record_doubles(int num_pes, int nx, int np);
	hipError_t launch_recon_tables(hipStream_t s, const ReconArgs& g);
	hipError_t launch_recon_contract(hipStream_t s, const ReconArgs& g);
	// the cross-term kernel: the energies alone, then one contraction that generates its operands per tile around the tile's
	// centre (no tables: Ax, Ep unused), the same records; RECON_CROSS_LIMIT = L of the range rule, tiles beyond it take the plain path
	constexpr double RECON_CROSS_LIMIT = 6.0;
	hipError_t launch_recon_energy(hipStream_t s, const ReconArgs& g);
	hipError_t launch_recon_cross(hipStream_t s, const ReconArgs& g);
	hipError_t launch_recon_final(hipStream_t s, const ReconArgs& g);

	// ---- "%g" text of device doubles (gple_format.hip): every number with its blank, '\n' after per_line numbers, a second '\n'
	// after lines_per_block lines (0: never); join: no blank before the first number of a line.  table: the powers of five of gple_g6.h on the
	// device; work: format_work_bytes() bytes, 16-byte aligned; slots: the second pass reads the items the first one kept instead of converting again.
	// *length: where the device leaves the text's length.  count a multiple of per_line, at most FORMAT_MAX_COUNT
	constexpr int FORMAT_BLOCK = 1024; // numbers per workgroup
	constexpr size_t FORMAT_MAX_COUNT = size_t(1) << 36;
	size_t format_work_bytes(size_t count, bool slots);
	hipError_t launch_format(hipStream_t s, const double* values, size_t count, size_t per_line, size_t lines_per_block, bool join,
		const unsigned long long* table, void* work, bool slots, char* text, const unsigned long long** length);

	// ---- the doubles of device "%g" text (gple_parse.hip): token i of the text in file order -> values[i] (values null: count only;
	// more than `capacity` tokens: nothing is written).  table: as above; work: parse_work_bytes() bytes, 16-byte aligned.  *result: where the device
	// leaves three words — the tokens, the lines that hold one, the byte offset of the first malformed token (all ones: none).  0 < length <=
	// PARSE_MAX_LENGTH; the text pointer needs no alignment
	constexpr int PARSE_CHUNK = 4096; // bytes per workgroup
	constexpr size_t PARSE_MAX_LENGTH = size_t(1) << 40;
	size_t parse_work_bytes(const void* text, size_t length);
	hipError_t launch_parse(hipStream_t s, const char* text, size_t length, const unsigned long long* table, void* work, double* values, size_t capacity,
		const unsigned long long** result);
} // namespace gple
