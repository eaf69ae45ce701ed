// gple_capi.hip — C-ABI entry points of include/gple.h (host orchestration of the HIP kernels).
//
// Data layout in HBM (all fp64):
//   training points  Xt   : 2 x Np interleaved, Np = round_up(N, 256), zero padded
//   typed labels     ys   : n_total   (real GP: Np;  complex GP: [s Re y ; s Im y], 2 Np)
//   inverse factor   T    : n_total x n_total column-major, T = chol(K_pad)^-1 (lower), upper part zero
//   weights          v    : n_total   (K^-1 ys),  diag(K^-1) w : n_total,  complex: diag of the off-diagonal block wx : Np
//   explicit inverse W    : n_total x n_total, built only for get_inverse()/derivatives (W = T^T T)
// A fit handle owns Xt, ys, T, v, w (+ lazily W and the derivative vectors); the Cholesky work matrix, the merge-tree
// workspace and all predict scratch belong to the context's buffer pool and are reused across calls.
#include <algorithm>
#include <cmath>
#include <new>

#include "gple_capi.h"
#include "gple_debug.h"

namespace gple
{
	int record_hip_error(Ctx* ctx, hipError_t e, const char* what, const char* file, int line)
	{
		if (ctx)
		{
			std::lock_guard<std::mutex> lk(ctx->mu);
			ctx->last_error = std::string(hipGetErrorString(e)) + " in " + what + " (" + file + ":" + std::to_string(line) + ")";
		}
		(void)hipGetLastError();
		return e == hipErrorOutOfMemory ? GPLE_ERR_ALLOC : GPLE_ERR_HIP;
	}
	static bool take_event(Ctx* c, hipEvent_t* e)
	{
		if (!c->ev_free.empty())
		{
			*e = c->ev_free.back();
			c->ev_free.pop_back();
			return true;
		}
		return hipEventCreate(e) == hipSuccess;
	}
	void timer_start(Ctx* c, int which)
	{
		if (!c->timing || c->pending.size() >= 8192) return; // nobody collects: stop recording rather than grow
		Ctx::TimedSpan sp{which, nullptr, nullptr};
		if (!take_event(c, &sp.e0)) return;
		if (!take_event(c, &sp.e1))
		{
			c->ev_free.push_back(sp.e0);
			return;
		}
		(void)hipEventRecord(sp.e0, c->stream);
		c->open_span[which] = sp;
	}
	void timer_stop(Ctx* c, int which)
	{
		Ctx::TimedSpan& sp = c->open_span[which];
		if (!sp.e0) return;
		(void)hipEventRecord(sp.e1, c->stream);
		c->pending.push_back(sp);
		sp = Ctx::TimedSpan{};
	}
	void chunk_timer_start(Ctx* c) { timer_start(c, GPLE_TIMER_PREDICT_KERNEL); }
	void chunk_timer_stop(Ctx* c) { timer_stop(c, GPLE_TIMER_PREDICT_KERNEL); }
	void timer_collect(Ctx* c)
	{
		for (const Ctx::TimedSpan& sp : c->pending)
		{
			float ms = 0.f;
			if (hipEventElapsedTime(&ms, sp.e0, sp.e1) == hipSuccess)
			{
				c->t_last[sp.which] = ms;
				c->t_total[sp.which] += ms;
				c->t_count[sp.which] += 1;
			}
			c->ev_free.push_back(sp.e0);
			c->ev_free.push_back(sp.e1);
		}
		c->pending.clear();
	}
} // namespace gple


namespace
{
	SEParam make_se(double amp, double n2, double l0, double l1) { return SEParam{amp, n2, l0, l1, 1.0 / l0, 1.0 / l1}; }

	// kernel.h:285-294
	SEParam purity_aux(double mag, double l0, double l1)
	{
		const double m = mag * mag * std::sqrt(l0 * l1);
		return make_se(m * m, 0.0, std::sqrt(2.0) * l0, std::sqrt(2.0) * l1);
	}
} // namespace

namespace
{
	// K^-1 (explicit) on first request
	int ensure_inverse(FitCommon* f)
	{
		std::lock_guard<std::mutex> lk(f->lazy_mu);
		if (f->W) return GPLE_OK;
		gple_ctx* ctx = f->ctx;
		hipError_t e;
		double* W = ctx->acquire(static_cast<size_t>(f->n_total) * f->n_total * sizeof(double), &e);
		GPLE_HIP(ctx, e);
		e = lauum_full(ctx->stream, f->T, f->n_total, W, f->n_total, f->n_total);
		if (e != hipSuccess)
		{
			ctx->give_back(W);
			GPLE_HIP(ctx, e);
		}
		f->W = W;
		return GPLE_OK;
	}

	int fit_factor(gple_ctx* ctx, FitCommon* f);
	// shared front half of both fits: upload, label scaling, Gram, Cholesky, inverse factor, weights
	int fit_common(gple_ctx* ctx, FitCommon* f, const double* X, const double* y, int y_stride, size_t N, unsigned flags)
	{
		hipStream_t st = ctx->stream;
		const bool dev = flags & GPLE_IO_DEVICE;
		f->ctx = ctx;
		ctx_retain(ctx); // a fit keeps its context alive (released in ~FitCommon)
		f->N = static_cast<int>(N);
		f->Np = static_cast<int>(round_up(N, NPAD));
		f->n_total = f->is_complex ? 2 * f->Np : f->Np;
		f->flags = flags;
		const int Np = f->Np, nt = f->n_total;
		hipError_t e;
		f->Xt = ctx->acquire(2 * static_cast<size_t>(Np) * 8, &e);
		GPLE_HIP(ctx, e);
		f->ys = ctx->acquire(static_cast<size_t>(nt) * 8, &e);
		GPLE_HIP(ctx, e);
		f->T = ctx->acquire(static_cast<size_t>(nt) * nt * 8, &e);
		GPLE_HIP(ctx, e);
		f->v = ctx->acquire(static_cast<size_t>(nt) * 8, &e);
		GPLE_HIP(ctx, e);
		f->w = ctx->acquire(static_cast<size_t>(nt) * 8, &e);
		GPLE_HIP(ctx, e);
		f->sdev = ctx->acquire(SDEV_N * 8, &e);
		GPLE_HIP(ctx, e);
		if (f->is_complex)
		{
			f->wx = ctx->acquire(static_cast<size_t>(Np) * 8, &e);
			GPLE_HIP(ctx, e);
		}
		Scratch ytmp(ctx);
		timer_start(ctx, GPLE_TIMER_FIT);
		const size_t ylen = N * static_cast<size_t>(y_stride);
		GPLE_HIP(ctx, ytmp.get(ylen));

		// device inputs are read in place; host inputs are staged by two copies.  One launch then pads the points, clears the
		// scalar block and rescales the labels (every launch costs 2.9 us on the GPU timeline)
		const double *Xin = X, *yin = y;
		Scratch xtmp(ctx);
		if (!dev)
		{
			GPLE_HIP(ctx, xtmp.get(2 * N));
			GPLE_HIP(ctx, copy_in(st, xtmp.p, X, 2 * N, false));
			GPLE_HIP(ctx, copy_in(st, ytmp.p, y, ylen, false));
			Xin = xtmp.p, yin = ytmp.p;
		}
		GPLE_HIP(ctx, launch_prep_labels(st, yin, y_stride, f->is_complex ? 1 : 0, f->N, Np, f->ys, f->sdev, Xin, f->Xt, SDEV_N));
		return fit_factor(ctx, f);
	}

	// Gram, Cholesky, inverse factor, weights of a fit whose points and scaled labels are in place (fit_common; recover_fit repeats it under the
	// launch-per-panel scheme after a give-up).  The scheme is the calling thread's (CholSchemeScope) or the context's (debug knob).
	int fit_factor(gple_ctx* ctx, FitCommon* f)
	{
		hipStream_t st = ctx->stream;
		const int Np = f->Np, nt = f->n_total;
		CholSchemeScope scheme(ctx->chol_scheme);
		Scratch Lbuf(ctx), work(ctx), u(ctx);
		GPLE_HIP(ctx, Lbuf.get(static_cast<size_t>(nt + CHOL_NB) * nt));
		GPLE_HIP(ctx, work.get(chol_inverse_work_doubles(nt)));
		GPLE_HIP(ctx, u.get(nt));
		// T is lower block-triangular and every consumer keeps to the blocks on and below the diagonal (the diagonal 64-blocks leave the
		// panel step complete, zeros above the diagonal included), so the blocks above are never written and never read: no 8 n^2-byte
		// memset in front of the factorisation (35 us at n = 4096).  GPLE_POISON_T=1 fills T with NaN bit patterns first — the GPU
		// test session runs that way (tests/conftest.py), so a reader of an unwritten block cannot go unnoticed.
		static const bool poison_t = [] {
			const char* e = getenv("GPLE_POISON_T");
			return e != nullptr && atoi(e) != 0;
		}();
		if (poison_t) GPLE_HIP(ctx, hipMemsetAsync(f->T, 0xFF, static_cast<size_t>(nt) * nt * 8, st));
		if (poison_t) GPLE_HIP(ctx, hipMemsetAsync(Lbuf.p, 0xFF, static_cast<size_t>(nt + CHOL_NB) * nt * 8, st)); // likewise the working matrix above its diagonal blocks
		// the scaled labels ride below the matrix as one more block row: its factor is u = L^-1 ys (= T ys, without the two launches)
		const long ldl = nt + CHOL_NB;
		GPLE_HIP(ctx, launch_gram_train(st, f->Xt, f->N, Np, nt, f->ps, Lbuf.p, ldl, f->ys));
		int* info_dev = reinterpret_cast<int*>(f->sdev + 31);
		GPLE_HIP(ctx, chol_inverse_factor(ctx, st, Lbuf.p, ldl, nt, f->T, nt, info_dev, work.p, u.p));
		GPLE_HIP(ctx, launch_colpass(st, f->T, nt, nt, u.p, f->v, f->w, Np, f->wx, info_dev)); // (a give-up of the factorisation: NaN)
		return GPLE_OK;
	}

	// GPLE_DERIV_BATCH=0: a launch per product in the derivative fits of small matrices too (A/B, and the bits check of the batched path)
	static bool deriv_batching()
	{
		static const bool on = [] {
			const char* e = getenv("GPLE_DERIV_BATCH");
			return e == nullptr || atoi(e) != 0;
		}();
		return on;
	}
	// TrainingKernel derivative members (kernel.cpp:337-477) for the real kernel; raw sums land in sdev[16..28]
	int real_fit_derivatives(gple_ctx* ctx, FitCommon* f, double sf, double l0, double l1, double sn, unsigned flags)
	{
		hipStream_t st = ctx->stream;
		const int nt = f->n_total;
		const size_t n2 = static_cast<size_t>(nt) * nt;
		GPLE_TRY(ensure_inverse(f));
		hipError_t e;
		f->dv = ctx->acquire(4 * static_cast<size_t>(nt) * 8, &e);
		GPLE_HIP(ctx, e);
		Scratch D(ctx), C(ctx), part(ctx), tvec(ctx), dwd(ctx), qpart(ctx);
		GPLE_HIP(ctx, D.get(2 * n2));
		GPLE_HIP(ctx, C.get(n2));
		GPLE_HIP(ctx, part.get(static_cast<size_t>(nt / 256) * nt));
		GPLE_HIP(ctx, tvec.get(nt));
		GPLE_HIP(ctx, dwd.get(4 * static_cast<size_t>(nt)));
		double* dv = f->dv;
		GPLE_HIP(ctx, launch_deriv_gram(st, f->Xt, f->N, nt, f->ps.p[0], D.p, D.p + n2));
		if (nt <= 1024 && deriv_batching())
		{
			// Small matrices: the same products, batched into a third of the launches (17 -> 8; a derivative fit at N = 256 is 0.1 ms of 4-5 us kernels).
			// Items of a batch are independent; every item's arithmetic is that of the launch-per-item path below (same bits).
			const double cn = -2.0 * (sf * sf) * sn;
			Scratch tv2(ctx), C2(ctx), part3(ctx);
			GPLE_HIP(ctx, tv2.get(2 * static_cast<size_t>(nt)));
			GPLE_HIP(ctx, part3.get(3 * static_cast<size_t>(nt / 256) * nt));
			{
				const double* x[2] = {f->v, f->w};
				const double al[2] = {-2.0 / sf, -2.0 / sf};
				const int nn[2] = {nt, nt};
				double* y[2] = {dv, dwd.p};
				GPLE_HIP(ctx, launch_scale_batch(st, 2, x, al, nn, y)); // magnitude: dW = -2 W / sf (:349)
			}
			{
				const double* A[3] = {D.p, D.p + n2, f->W};
				const double* x[3] = {f->v, f->v, f->v};
				const double al[3] = {1.0, 1.0, cn};
				double* y[3] = {tv2.p, tv2.p + nt, dv + 3 * static_cast<size_t>(nt)};
				GPLE_HIP(ctx, launch_gemv_batch(st, nt, 3, A, nt, x, al, part3.p, y)); // dK_d v; noise: (dW) y = cn W v (:358)
			}
			{
				const double* A[2] = {f->W, f->W};
				const double* x[2] = {tv2.p, tv2.p + nt};
				const double al[2] = {-1.0, -1.0};
				double* y[2] = {dv + static_cast<size_t>(nt), dv + 2 * static_cast<size_t>(nt)};
				GPLE_HIP(ctx, launch_gemv_batch(st, nt, 2, A, nt, x, al, part3.p, y)); // (dW) y = -W (dK v) (:354)
			}
			int act[2], nact = 0;
			for (int d = 0; d < 2; ++d)
			{
				if (f->deriv_mask >> (1 + d) & 1u) act[nact++] = d;
				else GPLE_HIP(ctx, hipMemsetAsync(dwd.p + static_cast<size_t>(1 + d) * nt, 0, static_cast<size_t>(nt) * sizeof(double), st));
			}
			const double* cA[3];
			const double* cB[3];
			double cal[3];
			double* cy[3];
			int nc = 0;
			if (nact)
			{
				GPLE_HIP(ctx, C2.get(nact * n2));
				GemmDesc g{};
				g.A = D.p + act[0] * n2, g.lda = nt, g.strideA = nact == 2 ? static_cast<long>(n2) : 0, g.B = f->W, g.ldb = nt, g.strideB = 0, g.C = C2.p, g.ldc = nt,
				g.strideC = static_cast<long>(n2);
				g.M = nt, g.N = nt, g.K = nt, g.batch = nact, g.alpha = 1.0, g.beta = 0.0, g.krange = K_FULL, g.lower_only = 0;
				g.a_kmajor = false, g.b_kmajor = false, g.c_trans = false;
				timer_start(ctx, GPLE_TIMER_DERIV_GEMM);
				GPLE_HIP(ctx, launch_gemm(st, g, gemm_pick_tile(nt, nt, 1, false))); // (the tile of ONE product: the items must not change kernel, i.e. bits, with the batch)
				timer_stop(ctx, GPLE_TIMER_DERIV_GEMM);
				for (int a = 0; a < nact; ++a) cA[nc] = f->W, cB[nc] = C2.p + a * n2, cal[nc] = -1.0, cy[nc] = dwd.p + static_cast<size_t>(1 + act[a]) * nt, ++nc;
			}
			cA[nc] = f->W, cB[nc] = f->W, cal[nc] = cn, cy[nc] = dwd.p + 3 * static_cast<size_t>(nt), ++nc;
			GPLE_HIP(ctx, launch_coldot_batch(st, nt, nc, cA, nt, cB, nt, 0, cal, cy)); // diag(dW)_i = -sum_j W(j,i) (dK W)(j,i); noise: cn sum_j W(j,i)^2
		}
		else
		{
		// magnitude: dW = -2 W / sf (:349)
		GPLE_HIP(ctx, launch_scale(st, f->v, -2.0 / sf, nt, dv));
		GPLE_HIP(ctx, launch_scale(st, f->w, -2.0 / sf, nt, dwd.p));
		// lengths: dW = -W dK W (:354): (dW) y = -W (dK v), diag(dW)_i = -sum_j W(j,i) (dK W)(j,i)
		for (int d = 0; d < 2; ++d)
		{
			const double* Dd = D.p + d * n2;
			GPLE_HIP(ctx, launch_gemv(st, Dd, nt, nt, f->v, 1.0, part.p, tvec.p));
			GPLE_HIP(ctx, launch_gemv(st, f->W, nt, nt, tvec.p, -1.0, part.p, dv + static_cast<size_t>(1 + d) * nt));
			if (!(f->deriv_mask >> (1 + d) & 1u)) // another rank forms this parameter's diag(W dK W) (gple_objective_eval_part); (dW) y above is needed by every rank's predict
			{
				GPLE_HIP(ctx, hipMemsetAsync(dwd.p + static_cast<size_t>(1 + d) * nt, 0, static_cast<size_t>(nt) * sizeof(double), st));
				continue;
			}
			GemmDesc g{};
			g.A = Dd, g.lda = nt, g.B = f->W, g.ldb = nt, g.C = C.p, g.ldc = nt;
			g.M = nt, g.N = nt, g.K = nt, g.batch = 1, g.alpha = 1.0, g.beta = 0.0, g.krange = K_FULL, g.lower_only = 0;
			g.a_kmajor = false, g.b_kmajor = false, g.c_trans = false;
			timer_start(ctx, GPLE_TIMER_DERIV_GEMM);
			GPLE_HIP(ctx, launch_gemm(st, g, gemm_pick_tile(nt, nt, 1, false)));
			timer_stop(ctx, GPLE_TIMER_DERIV_GEMM);
			GPLE_HIP(ctx, launch_coldot(st, f->W, nt, C.p, nt, nt, 0, -1.0, dwd.p + static_cast<size_t>(1 + d) * nt));
		}
		// noise: dW = -2 sf^2 sn W W (:358)
		const double cn = -2.0 * (sf * sf) * sn;
		GPLE_HIP(ctx, launch_gemv(st, f->W, nt, nt, f->v, cn, part.p, dv + 3 * static_cast<size_t>(nt)));
		GPLE_HIP(ctx, launch_coldot(st, f->W, nt, f->W, nt, nt, 0, cn, dwd.p + 3 * static_cast<size_t>(nt)));
		}
		GPLE_HIP(ctx, launch_real_deriv_sums(st, f->v, f->w, dv, dwd.p, f->N, nt, f->sdev + 16));
		if (flags & GPLE_CALC_AVERAGE)
		{
			const size_t g = (static_cast<size_t>(f->N) + 63) / 64;
			GPLE_HIP(ctx, qpart.get(g * g));
			const SEParam k1 = purity_aux(sf, l0, l1);
			for (int d = 0; d < 2; ++d) // v^T (dK1/dl'_d) v and dv_d^T K1 v
			{
				GPLE_HIP(ctx, launch_quadform(st, f->Xt, f->N, k1, f->v, f->v, d, qpart.p, f->sdev + 24 + d));
				GPLE_HIP(ctx, launch_quadform(st, f->Xt, f->N, k1, dv + static_cast<size_t>(1 + d) * nt, f->v, -1, qpart.p, f->sdev + 26 + d));
			}
			GPLE_HIP(ctx, launch_quadform(st, f->Xt, f->N, k1, dv + 3 * static_cast<size_t>(nt), f->v, -1, qpart.p, f->sdev + 28));
		}
		return GPLE_OK;
	}

	struct ComplexAux
	{
		double sC, lC[2];
		SEParam k[5]; // purity auxiliary kernels R', I', C', RC, IC (complex_kernel.cpp:287-356)
		double lRC[2], lIC[2];
	};
	ComplexAux complex_aux(const double* th)
	{
		const double sR = th[1], lR0 = th[2], lR1 = th[3], sI = th[4], lI0 = th[5], lI1 = th[6];
		ComplexAux a;
		const double ss0 = lR0 * lR0 + lI0 * lI0, ss1 = lR1 * lR1 + lI1 * lI1;
		a.sC = std::sqrt(sR * sI * ((2.0 * lR0 * lI0 / ss0) * (2.0 * lR1 * lI1 / ss1))); // complex_kernel.cpp:144-157
		a.lC[0] = std::sqrt(ss0 / 2.0), a.lC[1] = std::sqrt(ss1 / 2.0);
		auto mixed = [](double m1, double a0, double a1, double mb, double b0, double b1) { // complex_kernel.cpp:206-219
			const double prod = (0.5 * (1.0 / (a0 * a0) + 1.0 / (b0 * b0))) * (0.5 * (1.0 / (a1 * a1) + 1.0 / (b1 * b1)));
			const double m = m1 * mb / std::sqrt(std::sqrt(prod));
			return make_se(m * m, 0.0, std::sqrt(a0 * a0 + b0 * b0), std::sqrt(a1 * a1 + b1 * b1));
		};
		a.k[0] = purity_aux(sR, lR0, lR1);
		a.k[1] = purity_aux(sI, lI0, lI1);
		a.k[2] = purity_aux(a.sC, a.lC[0], a.lC[1]);
		a.k[3] = mixed(sR, lR0, lR1, a.sC, a.lC[0], a.lC[1]);
		a.k[4] = mixed(sI, lI0, lI1, a.sC, a.lC[0], a.lC[1]);
		a.lRC[0] = a.k[3].l0, a.lRC[1] = a.k[3].l1, a.lIC[0] = a.k[4].l0, a.lIC[1] = a.k[4].l1;
		return a;
	}
	// derivative blocks dC_p (p = 1..6) of the reference's dK / dK~ (complex_kernel.cpp:20-132), without the s^2 factor (sic)
	void build_dspecs(const double* th, DSpecSet* out)
	{
		const ComplexAux a = complex_aux(th);
		const double sR = th[1], sI = th[4];
		const double lR[2] = {th[2], th[3]}, lI[2] = {th[5], th[6]};
		const double aR = sR * sR, aI = sI * sI, aC = a.sC * a.sC;
		auto spec = [](double amp, double c0, double c1, const double* l, int dim) { return DSpec{amp, c0, c1, l[0], l[1], dim, 1}; };
		std::memset(out, 0, 6 * sizeof(DSpecSet));
		out[0].b[0] = spec(aR, 2.0 / sR, 0.0, lR, 0); // d/d sR: dC_xx = 2 KR / sR, dC_xy = KC / sR
		out[0].b[1] = spec(aC, 1.0 / sR, 0.0, a.lC, 0);
		out[3].b[2] = spec(aI, 2.0 / sI, 0.0, lI, 0); // d/d sI: dC_yy = 2 KI / sI, dC_xy = KC / sI
		out[3].b[1] = spec(aC, 1.0 / sI, 0.0, a.lC, 0);
		for (int d = 0; d < 2; ++d)
		{
			out[1 + d].b[0] = spec(aR, 0.0, 1.0, lR, d); // d/d lR_d: dC_xx = DR_d
			out[1 + d].b[1] = spec(aC, 1.0 / lR[d] - lR[d] / (a.lC[d] * a.lC[d]), 0.5 * lR[d] / a.lC[d], a.lC, d);
			out[4 + d].b[2] = spec(aI, 0.0, 1.0, lI, d); // d/d lI_d: dC_yy = DI_d
			out[4 + d].b[1] = spec(aC, 1.0 / lI[d] - lI[d] / (a.lC[d] * a.lC[d]), 0.5 * lI[d] / a.lC[d], a.lC, d);
		}
	}

	// TrainingComplexKernel derivative members (complex_kernel.cpp:379-590); raw sums land in sdev[32..39], [64..108], [128..287]
	int complex_fit_derivatives(gple_ctx* ctx, FitCommon* f, const double* th, unsigned flags)
	{
		hipStream_t st = ctx->stream;
		const int nt = f->n_total, Np = f->Np;
		const size_t n2 = static_cast<size_t>(nt) * nt;
		const double s0 = th[0], sn = th[7];
		GPLE_TRY(ensure_inverse(f));
		hipError_t e;
		f->dv = ctx->acquire(8 * static_cast<size_t>(nt) * 8, &e);
		GPLE_HIP(ctx, e);
		Scratch D(ctx), C(ctx), part(ctx), tvec(ctx), dwd(ctx), dwx(ctx);
		GPLE_HIP(ctx, D.get(n2));
		GPLE_HIP(ctx, C.get(n2));
		GPLE_HIP(ctx, part.get(static_cast<size_t>(nt / 256) * nt));
		GPLE_HIP(ctx, tvec.get(nt));
		GPLE_HIP(ctx, dwd.get(8 * static_cast<size_t>(nt)));
		GPLE_HIP(ctx, dwx.get(8 * static_cast<size_t>(Np)));
		double* dw = f->dv;
		if (nt <= 1024 && deriv_batching() && (f->deriv_mask & 0x7eu) == 0x7eu)
		{
			// Small matrices, every parameter formed here: the launch-per-product sequence below with its independent products batched (55 -> 25 launches;
			// a complex derivative fit at N = 256 is 0.3 ms of 4-5 us kernels).  Every item keeps its arithmetic (same bits).
			Scratch D6(ctx), tv6(ctx), part3(ctx), EF(ctx);
			const size_t ef = 2 * static_cast<size_t>(Np) * nt; // [E | F] of one parameter
			GPLE_HIP(ctx, D6.get(6 * n2));
			GPLE_HIP(ctx, tv6.get(6 * static_cast<size_t>(nt)));
			GPLE_HIP(ctx, part3.get(3 * static_cast<size_t>(nt / 256) * nt));
			GPLE_HIP(ctx, EF.get(6 * ef));
			{
				const double* x[3] = {f->v, f->w, f->wx};
				const double al[3] = {-2.0 / s0, -2.0 / s0, -2.0 / s0};
				const int nn[3] = {nt, nt, Np};
				double* y[3] = {dw, dwd.p, dwx.p};
				GPLE_HIP(ctx, launch_scale_batch(st, 3, x, al, nn, y)); // global magnitude: dM = -2 M / s
			}
			GPLE_HIP(ctx, launch_gemv(st, f->W, nt, nt, f->v, -sn, part.p, dw + 7 * static_cast<size_t>(nt))); // noise: dM = -sn M M
			GPLE_HIP(ctx, launch_coldot(st, f->W, nt, f->W, nt, nt, 0, -sn, dwd.p + 7 * static_cast<size_t>(nt)));
			GPLE_HIP(ctx, launch_coldot(st, f->W, nt, f->W, nt, nt, Np, -sn, dwx.p + 7 * static_cast<size_t>(Np)));
			for (int ip = 1; ip <= 6; ++ip) GPLE_HIP(ctx, launch_typed_deriv_gram(st, f->Xt, f->N, Np, nt, f->dspec[ip - 1], D6.p + (ip - 1) * n2));
			for (int grp = 0; grp < 2; ++grp) // parameters 1..3 (R kernel), 4..6 (I kernel)
			{
				const double *A[3], *x[3];
				double al[3];
				double* y[3];
				for (int z = 0; z < 3; ++z) A[z] = D6.p + (3 * grp + z) * n2, x[z] = f->v, al[z] = 1.0, y[z] = tv6.p + static_cast<size_t>(3 * grp + z) * nt;
				GPLE_HIP(ctx, launch_gemv_batch(st, nt, 3, A, nt, x, al, part3.p, y));
				for (int z = 0; z < 3; ++z) A[z] = f->W, x[z] = tv6.p + static_cast<size_t>(3 * grp + z) * nt, al[z] = -1.0, y[z] = dw + static_cast<size_t>(1 + 3 * grp + z) * nt;
				GPLE_HIP(ctx, launch_gemv_batch(st, nt, 3, A, nt, x, al, part3.p, y));
				// E = A M_a, F = B M_b of the three parameters (the comment at the launch-per-product path below)
				const long ao = grp == 0 ? 0 : Np, bo = grp == 0 ? Np : 0;
				double* E = EF.p + 3 * grp * ef;
				GemmDesc g{};
				g.lda = nt, g.strideA = static_cast<long>(n2), g.B = f->W + ao * static_cast<long>(nt), g.ldb = nt, g.strideB = 0, g.C = E, g.ldc = Np, g.strideC = static_cast<long>(ef);
				g.A = D6.p + 3 * grp * n2 + ao + ao * static_cast<long>(nt);
				g.M = Np, g.N = nt, g.K = Np, g.batch = 3, g.alpha = 1.0, g.beta = 0.0, g.krange = K_FULL, g.lower_only = 0;
				g.a_kmajor = false, g.b_kmajor = false, g.c_trans = false;
				timer_start(ctx, GPLE_TIMER_DERIV_GEMM);
				GPLE_HIP(ctx, launch_gemm(st, g, gemm_pick_tile(Np, nt, 1, false))); // (the tile of ONE product: an item's kernel must not depend on the batch)
				g.A = D6.p + 3 * grp * n2 + ao + bo * static_cast<long>(nt);
				g.B = f->W + bo * static_cast<long>(nt), g.C = E + static_cast<size_t>(Np) * nt;
				GPLE_HIP(ctx, launch_gemm(st, g, gemm_pick_tile(Np, nt, 1, false)));
				timer_stop(ctx, GPLE_TIMER_DERIV_GEMM);
				GPLE_HIP(ctx, launch_cderiv_diag_batch(st, 3, f->W, nt, static_cast<int>(ao), E, E + static_cast<size_t>(Np) * nt, Np, Np, nt, -1.0,
					dwd.p + static_cast<size_t>(1 + 3 * grp) * nt, dwx.p + static_cast<size_t>(1 + 3 * grp) * Np, static_cast<long>(ef), nt, Np));
			}
		}
		else
		{
		// global magnitude: dC = 2 C / s  ->  dM = -2 M / s
		GPLE_HIP(ctx, launch_scale(st, f->v, -2.0 / s0, nt, dw));
		GPLE_HIP(ctx, launch_scale(st, f->w, -2.0 / s0, nt, dwd.p));
		GPLE_HIP(ctx, launch_scale(st, f->wx, -2.0 / s0, Np, dwx.p));
		// noise: dK = 2 sn I, dK~ = 0 (complex_kernel.cpp:49-56, 129)  ->  dC = sn I  ->  dM = -sn M M
		GPLE_HIP(ctx, launch_gemv(st, f->W, nt, nt, f->v, -sn, part.p, dw + 7 * static_cast<size_t>(nt)));
		GPLE_HIP(ctx, launch_coldot(st, f->W, nt, f->W, nt, nt, 0, -sn, dwd.p + 7 * static_cast<size_t>(nt)));
		GPLE_HIP(ctx, launch_coldot(st, f->W, nt, f->W, nt, nt, Np, -sn, dwx.p + 7 * static_cast<size_t>(Np)));
		for (int ip = 1; ip <= 6; ++ip)
		{
			GPLE_HIP(ctx, launch_typed_deriv_gram(st, f->Xt, f->N, Np, nt, f->dspec[ip - 1], D.p));
			GPLE_HIP(ctx, launch_gemv(st, D.p, nt, nt, f->v, 1.0, part.p, tvec.p));
			GPLE_HIP(ctx, launch_gemv(st, f->W, nt, nt, tvec.p, -1.0, part.p, dw + static_cast<size_t>(ip) * nt));
			if (!(f->deriv_mask >> ip & 1u)) // another rank forms this parameter's diagonals (gple_objective_eval_part)
			{
				GPLE_HIP(ctx, hipMemsetAsync(dwd.p + static_cast<size_t>(ip) * nt, 0, static_cast<size_t>(nt) * sizeof(double), st));
				GPLE_HIP(ctx, hipMemsetAsync(dwx.p + static_cast<size_t>(ip) * Np, 0, static_cast<size_t>(Np) * sizeof(double), st));
				continue;
			}
			// Only diag(M dC M) and the diagonal of its Re-Im block are consumed, and every dC of a sub-kernel parameter has one zero
			// diagonal block (build_dspecs: C_yy does not depend on the R kernel's parameters, C_xx not on the I kernel's).  With A the
			// non-zero diagonal block, B the off-diagonal one and M_a / M_b the matching row halves of M,
			//   m_i^T dC m_i' = M_a,i^T (A M_a + B M_b)_i' + M_a,i'^T (B M_b)_i :
			// two products of Np x n x Np (E = A M_a, F = B M_b) instead of one of n x n x n — half the flops of the form before
			// (six n^3 GEMMs were 94 of the 153 ms of a complex objective evaluation at N = 4096).  M symmetric: M(k, c) is read as M(c, k).
			const bool a_is_xx = ip <= 3;                                // ip 1..3: parameters of the R kernel (C_yy' = 0); 4..6: of the I kernel (C_xx' = 0)
			const long ao = a_is_xx ? 0 : Np, bo = a_is_xx ? Np : 0;      // row / column offset of the A side and of the B side
			double *E = C.p, *F = C.p + static_cast<size_t>(Np) * nt;     // Np x n each
			GemmDesc g{};
			g.lda = nt, g.B = f->W + ao * static_cast<long>(nt), g.ldb = nt, g.C = E, g.ldc = Np;
			g.A = D.p + ao + ao * static_cast<long>(nt);                  // A: the non-zero diagonal block of dC
			g.M = Np, g.N = nt, g.K = Np, g.batch = 1, g.alpha = 1.0, g.beta = 0.0, g.krange = K_FULL, g.lower_only = 0;
			g.a_kmajor = false, g.b_kmajor = false, g.c_trans = false;
			timer_start(ctx, GPLE_TIMER_DERIV_GEMM);
			GPLE_HIP(ctx, launch_gemm(st, g, gemm_pick_tile(Np, nt, 1, false)));
			g.A = D.p + ao + bo * static_cast<long>(nt);                  // B: rows on the A side, columns on the other
			g.B = f->W + bo * static_cast<long>(nt), g.C = F;
			GPLE_HIP(ctx, launch_gemm(st, g, gemm_pick_tile(Np, nt, 1, false)));
			timer_stop(ctx, GPLE_TIMER_DERIV_GEMM);
			GPLE_HIP(ctx, launch_cderiv_diag(st, f->W, nt, static_cast<int>(ao), E, F, Np, Np, nt, -1.0, dwd.p + static_cast<size_t>(ip) * nt,
				dwx.p + static_cast<size_t>(ip) * Np));
		}
		}
		GPLE_HIP(ctx, launch_complex_deriv_sums(st, f->v, f->w, f->wx, dw, dwd.p, dwx.p, f->N, Np, f->sdev + 32));
		if (flags & GPLE_CALC_AVERAGE)
		{
			const ComplexAux a = complex_aux(th);
			const size_t g64 = (static_cast<size_t>(f->N) + 63) / 64, g256 = (static_cast<size_t>(f->N) + 255) / 256;
			Scratch qpart(ctx), mpart(ctx), ga(ctx), gb(ctx);
			GPLE_HIP(ctx, qpart.get(9 * g64 * g64));
			GPLE_HIP(ctx, mpart.get(2 * g256 * g256 * 256));
			GPLE_HIP(ctx, ga.get(g256 * 256));
			GPLE_HIP(ctx, gb.get(g256 * 256));
			const double *wr = f->v, *wi = f->v + Np;
			for (int x = 0; x < 5; ++x)
			{
				GPLE_HIP(ctx, launch_multi_quadform(st, f->Xt, f->N, a.k[x], wr, wi, qpart.p, f->sdev + 64 + 9 * x));
				GPLE_HIP(ctx, launch_aux_matvec(st, f->Xt, f->N, a.k[x], wr, wi, mpart.p, ga.p, gb.p));
				GPLE_HIP(ctx, launch_aux_dots(st, ga.p, gb.p, dw, f->N, Np, nt, f->sdev + 128 + 32 * x));
			}
		}
		return GPLE_OK;
	}

	// complex_kernel.cpp:475-590 from the raw sums (weights w = 2 v, so every quadratic form carries 1/4)
	void complex_purity_derivative(const double* th, const double* h, double s, double* out8)
	{
		const ComplexAux a = complex_aux(th);
		const double sR = th[1], sI = th[4];
		const double lR[2] = {th[2], th[3]}, lI[2] = {th[5], th[6]};
		const double GlobalFactor = (2.0 * M_PI) * 2.0 * M_PI; // :497 — no magnitude^4 here (reference quirk, :584 vs :370)
		auto Q = [&](int x, int pair, int var) { return h[64 + 9 * x + 3 * pair + var]; };
		auto Dd = [&](int x, int ip, int q) { return h[128 + 32 * x + 4 * ip + q]; };
		for (int ip = 0; ip < 8; ++ip)
		{
			double c0[5] = {0, 0, 0, 0, 0}, c1[5] = {0, 0, 0, 0, 0};
			int d = 0;
			if (ip == 1)
				c0[0] = 4.0 / sR, c0[2] = 2.0 / sR, c0[3] = 3.0 / sR, c0[4] = 1.0 / sR; // :525-529
			else if (ip == 2 || ip == 3)
			{
				d = ip - 2;
				const double l = lR[d], roc2 = l / (a.lC[d] * a.lC[d]);
				c0[0] = 1.0 / l, c1[0] = std::sqrt(2.0);                                                                 // :534
				c0[2] = 2.0 / l - 3.0 * roc2 / 2.0, c1[2] = 1.0 / std::sqrt(2.0) * (l / a.lC[d]);                          // :536-537
				c0[3] = (2.0 / l - roc2 / 2.0) - 1.5 * (l / a.lRC[d]) / a.lRC[d], c1[3] = 1.5 * (l / a.lRC[d]);             // :538-539
				c0[4] = (1.0 / l - roc2 / 2.0) - (l / a.lIC[d]) / 2.0 / a.lIC[d], c1[4] = (l / a.lIC[d]) / 2.0;             // :540-541
			}
			else if (ip == 4)
				c0[1] = 4.0 / sI, c0[2] = 2.0 / sI, c0[3] = 1.0 / sI, c0[4] = 3.0 / sI; // :548-552
			else if (ip == 5 || ip == 6)
			{
				d = ip - 5;
				const double l = lI[d], ioc2 = l / (a.lC[d] * a.lC[d]);
				c0[1] = 1.0 / l, c1[1] = std::sqrt(2.0);                                                                 // :558
				c0[2] = 2.0 / l - 3.0 * ioc2 / 2.0, c1[2] = 1.0 / std::sqrt(2.0) * (l / a.lC[d]);                          // :559-560
				c0[3] = (1.0 / l - ioc2 / 2.0) - (l / a.lRC[d]) / 2.0 / a.lRC[d], c1[3] = (l / a.lRC[d]) / 2.0;             // :561-562
				c0[4] = (2.0 / l - ioc2 / 2.0) - 1.5 * (l / a.lIC[d]) / a.lIC[d], c1[4] = 1.5 * (l / a.lIC[d]);             // :563-564
			}
			auto dX = [&](int x, int pair) { return c0[x] * Q(x, pair, 0) + c1[x] * Q(x, pair, 1 + d); };
			const double k1c[3] = {1.0, 1.0, 2.0};
			double T1 = 0.0, T2 = 0.0;
			for (int x = 0; x < 3; ++x)
			{
				T1 += k1c[x] * (Dd(x, ip, 0) + Dd(x, ip, 1)); // Re(v^H K1 dv)
				T2 += k1c[x] * (dX(x, 0) + dX(x, 1));         // Re(v^H K1' v)
			}
			const double T3 = (Dd(0, ip, 0) - Dd(1, ip, 0)) - (Dd(0, ip, 1) - Dd(1, ip, 1)) + 2.0 * (Dd(3, ip, 2) + Dd(4, ip, 2))
				+ 2.0 * (Dd(3, ip, 3) + Dd(4, ip, 3));                                                      // Re(v^T K2 dv)
			const double T4 = (dX(0, 0) - dX(1, 0)) - (dX(0, 1) - dX(1, 1)) + 2.0 * 2.0 * (dX(3, 2) + dX(4, 2)); // Re(v^T K2' v)
			out8[ip] = 0.25 * (2.0 * T1 + T2 + 2.0 * T3 + T4) * GlobalFactor / (s * s); // :580-584
		}
	}

	template <typename S>
	void fill_nan_scalars(S* sc)
	{
		double* d = reinterpret_cast<double*>(sc);
		for (size_t i = 0; i < (sizeof(S) - sizeof(int)) / sizeof(double); ++i) d[i] = nan_();
		sc->info = 0;
	}

	// complex raw sums: out[0] = LOOCV error, out[1] = Re(conj(ys).v) (both in the reference's complex convention)
	__global__ void __launch_bounds__(1024) complex_fit_sums_kernel(const double* __restrict__ ys, const double* __restrict__ wv,
		const double* __restrict__ wd, const double* __restrict__ wx, int N, int Np, double* __restrict__ out)
	{
		__shared__ double red[16];
		double s0 = 0.0, s1 = 0.0;
		for (int i = threadIdx.x; i < N; i += 1024)
		{
			// P_ii = (Mxx + Myy)/4, Q_ii = ((Mxx - Myy) - 2i Mxy)/4, v_i = (wx + i wy)/2   
			const double mxx = wd[i], myy = wd[Np + i], mxy = wx[i];
			const double p = 0.25 * (mxx + myy), qr = 0.25 * (mxx - myy), qi = -0.5 * mxy;
			const double vr = 0.5 * wv[i], vi = 0.5 * wv[Np + i];
			// numerator P v - conj(Q v)   (complex_kernel.cpp:281)
			const double qvr = qr * vr - qi * vi, qvi = qr * vi + qi * vr;
			const double nr = p * vr - qvr, ni = p * vi + qvi;
			const double den = p * p - (qr * qr + qi * qi);
			const double dr = nr / den, di = ni / den;
			s0 += dr * dr + di * di;
			s1 += ys[i] * vr + ys[Np + i] * vi;
		}
		for (int q = 0; q < 2; ++q)
		{
			double x = q == 0 ? s0 : s1;
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
			__syncthreads();
			if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
			__syncthreads();
			if (threadIdx.x == 0)
			{
				double tot = 0.0;
				for (int i = 0; i < 16; ++i) tot += red[i];
				out[q] = tot;
			}
		}
	}

	// P / Q blocks of the augmented inverse from the real 2Np x 2Np inverse M (column-major, ld = 2 Np):
	//   P = ((Mxx + Myy) + i (Mxy^T - Mxy)) / 4,   Q = ((Mxx - Myy) - i (Mxy + Mxy^T)) / 4
	__global__ void __launch_bounds__(256) complex_blocks_kernel(const double* __restrict__ Mi, long ld, int N, int Np, int which,
		double* __restrict__ out)
	{
		const int i = blockIdx.x * 64 + (threadIdx.x & 63);
		const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
		if (i >= N || j >= N) return;
		const double mxx = Mi[i + j * ld], myy = Mi[(Np + i) + (Np + j) * ld];
		const double mxy = Mi[i + (Np + j) * ld], mxyT = Mi[j + (Np + i) * ld];
		double re, im;
		if (which == 0) re = 0.25 * (mxx + myy), im = 0.25 * (mxyT - mxy);
		else re = 0.25 * (mxx - myy), im = -0.25 * (mxy + mxyT);
		out[2 * (i + static_cast<long>(j) * N)] = re;
		out[2 * (i + static_cast<long>(j) * N) + 1] = im;
	}
	// K (real) and pseudo-kernel (complex) of the complex training set, regenerated for the getters
	__global__ void __launch_bounds__(256) complex_kernels_kernel(const double* __restrict__ C, long ld, int N, int Np, int which,
		double* __restrict__ out)
	{
		const int i = blockIdx.x * 64 + (threadIdx.x & 63);
		const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
		if (i >= N || j >= N) return;
		const double cxx = C[i + j * ld], cyy = C[(Np + i) + (Np + j) * ld], cxy = C[i + (Np + j) * ld];
		if (which == 0) out[i + static_cast<long>(j) * N] = cxx + cyy; // K = Cxx + Cyy
		else
		{
			out[2 * (i + static_cast<long>(j) * N)] = cxx - cyy; // Re Kt
			out[2 * (i + static_cast<long>(j) * N) + 1] = 2.0 * cxy; // Im Kt
		}
	}
	__global__ void __launch_bounds__(256) halve_pair_kernel(const double* __restrict__ a, int N, int Np, double* __restrict__ out)
	{
		const int i = blockIdx.x * 256 + threadIdx.x;
		if (i < N) out[2 * i] = 0.5 * a[i], out[2 * i + 1] = 0.5 * a[Np + i];
	}
	__global__ void __launch_bounds__(256) pair_kernel(const double* __restrict__ a, int N, int Np, double* __restrict__ out)
	{
		const int i = blockIdx.x * 256 + threadIdx.x;
		if (i < N) out[2 * i] = a[i], out[2 * i + 1] = a[Np + i];
	}
} // namespace

extern "C"
{
	const char* gple_status_string(int status)
	{
		switch (status)
		{
		case GPLE_OK: return "ok";
		case GPLE_ERR_BAD_ARG: return "bad argument";
		case GPLE_ERR_TIMEOUT: return "the factorisation gave up waiting; results enqueued before the synchronisation that noticed are NaN";
		case GPLE_ERR_HIP: return "HIP runtime error";
		case GPLE_ERR_ALLOC: return "device allocation failed";
		case GPLE_ERR_STATE: return "requested output was not computed by this fit (flags), or the context was destroyed";
		case GPLE_ERR_COLLECTIVE: return "RCCL collective failed or librccl could not be resolved";
		default: return "unknown status";
		}
	}

	int gple_ctx_create(int device, void* stream, gple_ctx** out)
	{
		if (!out) return GPLE_ERR_BAD_ARG;
		*out = nullptr;
		int count = 0;
		if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return GPLE_ERR_HIP;
		if (hipSetDevice(device) != hipSuccess) return GPLE_ERR_HIP;
		gple_ctx* c = new (std::nothrow) gple_ctx;
		if (!c) return GPLE_ERR_ALLOC;
		c->device = device;
		if (stream) c->stream = static_cast<hipStream_t>(stream);
		else
		{
			if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
			{
				delete c;
				return GPLE_ERR_HIP;
			}
			c->owns_stream = true;
		}
		if (hipHostMalloc(reinterpret_cast<void**>(&c->host_scalars), 2 * SDEV_N * sizeof(double)) != hipSuccess)
		{
			if (c->owns_stream) (void)hipStreamDestroy(c->stream);
			delete c;
			return GPLE_ERR_ALLOC;
		}
		*out = c;
		return GPLE_OK;
	}
	int gple_ctx_destroy(gple_ctx* ctx)
	{
		if (!ctx) return GPLE_OK;
		if (ctx->closed.exchange(true)) return GPLE_ERR_STATE; // destroyed twice while handles keep it alive
		{
			std::lock_guard<std::mutex> lk(ctx->call_mu); // a call in flight on another thread finishes first
			(void)hipSetDevice(ctx->device);
			(void)hipStreamSynchronize(ctx->stream);
		}
		ctx_drop(ctx);
		return GPLE_OK;
	}
	int gple_ctx_trim(gple_ctx* ctx, size_t* bytes_freed)
	{
		if (!ctx) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // nothing in flight may still be using an idle buffer
		timer_collect(ctx);
		size_t freed = 0;
		{
			std::lock_guard<std::mutex> pl(ctx->pool_mu);
			std::vector<gple_ctx::PoolEntry> kept;
			for (const gple_ctx::PoolEntry& e : ctx->pool)
				if (e.used) kept.push_back(e);
				else
				{
					(void)hipFree(e.p);
					freed += e.bytes;
				}
			ctx->pool.swap(kept);
		}
		if (bytes_freed) *bytes_freed = freed;
		return GPLE_OK;
	}
	int gple_ctx_synchronize(gple_ctx* ctx)
	{
		if (!ctx) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		std::lock_guard<std::mutex> lk(ctx->call_mu);
		GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		timer_collect(ctx);
		return GPLE_OK;
	}
	const char* gple_ctx_last_error(const gple_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

	int gple_ctx_enable_timing(gple_ctx* ctx, int on)
	{
		if (!ctx) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		timer_collect(ctx); // intervals still in flight belong to the old accumulators
		ctx->timing = on != 0;
		for (int w = 0; w < Ctx::NTIMERS; ++w) ctx->t_last[w] = ctx->t_total[w] = 0.0, ctx->t_count[w] = 0;
		return GPLE_OK;
	}
	int gple_ctx_get_prune_stats(gple_ctx* ctx, unsigned long long* contracted_blocks, unsigned long long* seen_blocks, int reset)
	{
		if (!ctx) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		unsigned long long h[2] = {0, 0};
		if (ctx->prune_stats)
		{
			GPLE_HIP(ctx, hipMemcpyAsync(h, ctx->prune_stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
			if (reset) GPLE_HIP(ctx, hipMemsetAsync(ctx->prune_stats, 0, sizeof(h), ctx->stream));
			GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		}
		if (contracted_blocks) *contracted_blocks = h[0];
		if (seen_blocks) *seen_blocks = h[1];
		return GPLE_OK;
	}
	int gple_ctx_get_timing(gple_ctx* ctx, gple_timer which, double* last_ms, double* total_ms, long* count)
	{
		if (!ctx || static_cast<int>(which) < 0 || static_cast<int>(which) >= Ctx::NTIMERS) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		timer_collect(ctx);
		if (last_ms) *last_ms = ctx->t_last[which];
		if (total_ms) *total_ms = ctx->t_total[which];
		if (count) *count = ctx->t_count[which];
		return GPLE_OK;
	}

	// ---- KernelBase --------------------------------------------------------------------------------------------
	int gple_real_gram(gple_ctx* ctx, const double theta[4], const double* left, size_t R, const double* right, size_t C,
		int same_features, unsigned flags, double* K, double* dK)
	{
		if (!ctx || !theta || !K || (R && !left) || (C && !right)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (R == 0 || C == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const SEParam p = make_se(theta[0] * theta[0], theta[3] * theta[3], theta[1], theta[2]);
		Staged l(ctx, dev), r(ctx, dev), k(ctx, dev), dk(ctx, dev);
		GPLE_HIP(ctx, l.in(left, 2 * R));
		GPLE_HIP(ctx, r.in(right, 2 * C));
		GPLE_HIP(ctx, k.out(K, R * C));
		GPLE_HIP(ctx, dk.out(dK, 4 * R * C));
		GPLE_HIP(ctx, launch_gram_rect(ctx->stream, l.p, (int)R, r.p, (int)C, same_features, p, theta[0], theta[3], k.p, dk.p));
		GPLE_HIP(ctx, k.back());
		GPLE_HIP(ctx, dk.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return GPLE_OK;
	}

	// ---- ComplexKernelBase ---------------------------------------------------------------------------------------
	int gple_complex_gram(gple_ctx* ctx, const double theta[8], const double* left, size_t R, const double* right, size_t C, int same_features,
		unsigned flags, double* K, double* Kt, double* dK, double* dKt)
	{
		if (!ctx || !theta || !K || (R && !left) || (C && !right)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (R == 0 || C == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t rc = R * C;
		Staged l(ctx, dev), r(ctx, dev), k(ctx, dev), kt(ctx, dev), dk(ctx, dev), dkt(ctx, dev);
		GPLE_HIP(ctx, l.in(left, 2 * R));
		GPLE_HIP(ctx, r.in(right, 2 * C));
		GPLE_HIP(ctx, k.out(K, rc));
		GPLE_HIP(ctx, kt.out(Kt, 2 * rc));
		GPLE_HIP(ctx, dk.out(dK, 8 * rc));
		GPLE_HIP(ctx, dkt.out(dKt, 16 * rc));
		GPLE_HIP(ctx, launch_complex_gram(ctx->stream, theta, l.p, (int)R, r.p, (int)C, same_features, k.p, kt.p, dk.p, dkt.p));
		for (Staged* o : {&k, &kt, &dk, &dkt}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return GPLE_OK;
	}

	int gple_cutoff_factor(gple_ctx* ctx, const double* prediction, int is_complex, const double* variance, size_t M, unsigned flags,
		double* factor)
	{
		if (!ctx || (M && (!prediction || !variance || !factor))) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (M == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		Staged p(ctx, dev), v(ctx, dev), f(ctx, dev);
		GPLE_HIP(ctx, p.in(prediction, is_complex ? 2 * M : M));
		GPLE_HIP(ctx, v.in(variance, M));
		GPLE_HIP(ctx, f.out(factor, M));
		GPLE_HIP(ctx, launch_cutoff(ctx->stream, p.p, is_complex, v.p, (int)M, f.p));
		GPLE_HIP(ctx, f.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return GPLE_OK;
	}

}

// ---- TrainingKernel / TrainingComplexKernel ------------------------------------------------------------------------
namespace
{
	// what follows the factorisation of a real fit: the raw sums of the scalar members (+ the derivative members); enqueue only
	static int fit_post(gple_ctx* ctx, gple_real_fit* f)
	{
		hipStream_t st = ctx->stream;
		const unsigned flags = f->flags;
		const double sf = f->theta[0], l0 = f->theta[1], l1 = f->theta[2], sn = f->theta[3];
		const size_t N = f->N;
		Scratch part(ctx);
		const size_t g = (N + 63) / 64;
		const bool avg = (flags & GPLE_CALC_AVERAGE) != 0;
		if (avg) // purity: v^T K1 v; its per-block partials are summed by the same launch that forms the other sums
		{
			GPLE_HIP(ctx, part.get(g * g));
			GPLE_HIP(ctx, launch_quadform_partials(st, f->Xt, f->N, purity_aux(sf, l0, l1), f->v, f->v, -1, part.p));
		}
		GPLE_HIP(ctx, launch_real_fit_sums(st, f->Xt, f->ys, f->v, f->w, f->N, f->sdev + 1, avg ? part.p : nullptr, static_cast<int>(g * g), f->sdev + 6));
		if (flags & GPLE_CALC_DERIVATIVE) GPLE_TRY(real_fit_derivatives(ctx, f, sf, l0, l1, sn, flags));
		return GPLE_OK;
	}
	// what follows the factorisation of a complex fit: raw sums, purity quadratic forms (+ the derivative members); enqueue only
	static int fit_post(gple_ctx* ctx, gple_complex_fit* f)
	{
		hipStream_t st = ctx->stream;
		const unsigned flags = f->flags;
		const double* theta = f->theta;
		const size_t N = f->N;
		const double sR = theta[1], lR0 = theta[2], lR1 = theta[3], sI = theta[4], lI0 = theta[5], lI1 = theta[6];
		hipLaunchKernelGGL(complex_fit_sums_kernel, dim3(1), dim3(1024), 0, st, f->ys, f->v, f->w, f->wx, f->N, f->Np, f->sdev + 1);
		GPLE_HIP(ctx, hipGetLastError());
		if (flags & GPLE_CALC_AVERAGE)
		{
			// purity quadratic forms in the [Re; Im] weights w = 2 v (complex_kernel.cpp:287-377):
			// Re(v^H K1 v) + Re(v^T K2 v) = 2 vr'KR'vr + 2 vi'KI'vi + 2 (vr'KC'vr + vi'KC'vi) + 4 vr'(KRC + KIC)vi
			const ComplexAux a = complex_aux(theta);
			Scratch part(ctx);
			const size_t g = (N + 63) / 64;
			GPLE_HIP(ctx, part.get(g * g));
			const SEParam aR = purity_aux(sR, lR0, lR1), aI = purity_aux(sI, lI0, lI1), aC = purity_aux(a.sC, a.lC[0], a.lC[1]);
			const double *wr = f->v, *wi = f->v + f->Np;
			const SEParam ks[6] = {aR, aI, aC, aC, a.k[3], a.k[4]};
			const double* as[6] = {wr, wi, wr, wi, wr, wr};
			const double* bs[6] = {wr, wi, wr, wi, wi, wi};
			for (int q = 0; q < 6; ++q) GPLE_HIP(ctx, launch_quadform(st, f->Xt, f->N, ks[q], as[q], bs[q], -1, part.p, f->sdev + 8 + q));
		}
		if (flags & GPLE_CALC_DERIVATIVE) GPLE_TRY(complex_fit_derivatives(ctx, f, theta, flags));
		return GPLE_OK;
	}

	// A give-up of the one-launch factorisation (info = -1; the stream is drained, call_mu held): the SAME fit again with one launch per panel
	// — the scheme of rounds 2-3, no workgroup of which waits for another — from the Gram on: points, scaled labels and parameters are the
	// handle's, the factorisation is in place so the Gram is regenerated (28 us at n = 4096), and the layout is the one a process started
	// with GPLE_CHOL_SCHEME=step uses, so the recovered fit has that process's bits (tests/test_gpu_chol_diag.py).  Products of the bad
	// factor that were built lazily (W, the derivative vectors) are dropped and rebuilt.
	static int recover_fit(gple_ctx* ctx, FitCommon* f)
	{
		hipStream_t st = ctx->stream;
		f->recovered.store(true);
		for (double** p : {&f->W, &f->dv})
		{
			ctx->give_back(*p);
			*p = nullptr;
		}
		GPLE_HIP(ctx, hipMemsetAsync(f->sdev + SDEV_INFO, 0, sizeof(double), st));
		int status;
		{
			CholSchemeScope step(0);
			const int keep = ctx->chol_scheme;
			ctx->chol_scheme = -1; // (the scope above decides; a context forced to the one-launch scheme by the debug knob recovers like any other)
			status = fit_factor(ctx, f);
			ctx->chol_scheme = keep;
		}
		if (status == GPLE_OK)
			status = f->is_complex ? fit_post(ctx, static_cast<gple_complex_fit*>(f)) : fit_post(ctx, static_cast<gple_real_fit*>(f));
		return status;
	}
	// reads the fit's scalar block back into the pinned host block (drains the stream), looks at the factorisation's info word and recovers
	// from a give-up.  GPLE_ERR_TIMEOUT: the repeated factorisation gave up as well (cannot happen — it has no waits)
	int validate_fit(gple_ctx* ctx, const FitCommon* fc)
	{
		FitCommon* f = const_cast<FitCommon*>(fc);
		hipStream_t st = ctx->stream;
		int info_i = 0;
		for (int attempt = 0;; ++attempt)
		{
			GPLE_HIP(ctx, hipMemcpyAsync(ctx->host_scalars, f->sdev, SDEV_N * 8, hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			std::memcpy(&info_i, ctx->host_scalars + SDEV_INFO, sizeof(int));
			if (info_i >= 0) break;
			GPLE_TRY(note_give_up(ctx, attempt));
			GPLE_TRY(recover_fit(ctx, f));
		}
		f->validated.store(true);
		return GPLE_OK;
	}
	// Every call that drains the stream for a fit ends here (*_fit_create with scalars, *_fit_get_scalars, *_fit_get, a draining predict after
	// its repeated pass): it validates or recovers the fit, and then — the call's own outputs being those of the good fit — returns
	// GPLE_ERR_TIMEOUT if work enqueued on the fit BEFORE it was validated consumed a factor that was then found unfinished: those results are
	// NaN.  On a validated fit: two atomics, no device call.
	int settle_fit(gple_ctx* ctx, const FitCommon* f)
	{
		if (!f->validated.load()) GPLE_TRY(validate_fit(ctx, f));
		if (!f->recovered.load()) return GPLE_OK;
		const int stale = f->stale_uses.exchange(0);
		if (stale == 0) return GPLE_OK;
		std::lock_guard<std::mutex> lk(ctx->mu);
		ctx->last_error = "the one-launch factorisation gave up waiting; the fit has been repeated with one launch per panel and is valid now, but "
			+ std::to_string(stale) + " call(s) enqueued on it before this synchronisation produced NaN: repeat them";
		return GPLE_ERR_TIMEOUT;
	}

	// the closed forms of TrainingKernel's scalar members from the raw sums h
	void closed_form_scalars(gple_real_fit* f, const double* h)
	{
		const unsigned flags = f->flags;
		const size_t N = f->N;
		const double sf = f->theta[0], l0 = f->theta[1], l1 = f->theta[2];
		const double s = h[0];
		gple_real_fit_scalars& sc = f->sc;
		{
			const double within = h[5] / static_cast<double>(N); // kernel.h:169
			sc.magnitude = within < 0 ? std::sqrt(-within) : std::sqrt(within);
		}
		if (flags & GPLE_CALC_ERROR) sc.error = h[1];
		if (flags & GPLE_CALC_AVERAGE)
		{
			const double GlobalFactor = 2.0 * M_PI; // power<Dim>(2 pi), kernel.cpp:291
			const double lprod = l0 * l1;
			sc.population = GlobalFactor * (sf * sf) * lprod * h[2] / s;                 // :293
			sc.first_order_average[0] = GlobalFactor * (sf * sf) * lprod * h[3] / s;     // :308
			sc.first_order_average[1] = GlobalFactor * (sf * sf) * lprod * h[4] / s;
			const double PurityGlobal = (2.0 * M_PI) * M_PI; // PurityFactor * pi^Dim, :330
			sc.purity = PurityGlobal * h[6] / (s * s);        // :331
		}
		if (flags & GPLE_CALC_DERIVATIVE)
		{
			if (flags & GPLE_CALC_ERROR)
				for (int ip = 0; ip < 4; ++ip) sc.error_derivative[ip] = h[16 + ip]; // kernel.cpp:381-400
			if (flags & GPLE_CALC_AVERAGE)
			{
				// kernel.cpp:401-435
				const double ThisTimeFactor = (2.0 * M_PI) * (sf * sf) * (l0 * l1);
				const double ls[2] = {l0, l1};
				sc.population_derivative[0] = 0.0;
				for (int d = 0; d < 2; ++d) sc.population_derivative[1 + d] = ThisTimeFactor * (h[2] / ls[d] + h[21 + d]);
				sc.population_derivative[3] = ThisTimeFactor * h[23];
				for (double& d : sc.population_derivative) d /= s;
				// kernel.cpp:436-477
				const double PurityGlobal = (2.0 * M_PI) * M_PI;
				sc.purity_derivative[0] = 0.0;
				for (int d = 0; d < 2; ++d)
					sc.purity_derivative[1 + d] = ((h[6] / ls[d] + std::sqrt(2.0) * h[24 + d]) + 2.0 * h[26 + d]) * PurityGlobal;
				sc.purity_derivative[3] = 2.0 * PurityGlobal * h[28];
				for (double& d : sc.purity_derivative) d /= s * s;
			}
		}
	}
	// the closed forms of TrainingComplexKernel's scalar members from the raw sums h
	void closed_form_scalars(gple_complex_fit* f, const double* h)
	{
		const unsigned flags = f->flags;
		const size_t N = f->N;
		const double* theta = f->theta;
		const double s0 = theta[0];
		double purity_sums[6];
		for (int q = 0; q < 6; ++q) purity_sums[q] = h[8 + q];
		const double s = h[0];
		gple_complex_fit_scalars& sc = f->sc;
		{
			const double within = h[2] / static_cast<double>(N); // complex_kernel.h:194
			sc.magnitude = within < 0 ? std::sqrt(-within) : std::sqrt(within);
		}
		if (flags & GPLE_CALC_ERROR) sc.error = h[1];
		if (flags & GPLE_CALC_AVERAGE)
		{
			const double GlobalFactor = (2.0 * M_PI) * 2.0 * M_PI; // PurityFactor * 2 pi^Dim, complex_kernel.cpp:369
			const double ThisTimeFactor = GlobalFactor * ((s0 * s0) * (s0 * s0));
			// weights w = 2 v  ->  every quadratic form carries 1/4
			const double qf = 0.25 * (2.0 * purity_sums[0] + 2.0 * purity_sums[1] + 2.0 * (purity_sums[2] + purity_sums[3])
				+ 4.0 * (purity_sums[4] + purity_sums[5]));
			sc.purity = ThisTimeFactor * qf / (s * s); // :373
		}
		if (flags & GPLE_CALC_DERIVATIVE)
		{
			if (flags & GPLE_CALC_ERROR)
				for (int ip = 0; ip < 8; ++ip) sc.error_derivative[ip] = h[32 + ip];
			if (flags & GPLE_CALC_AVERAGE) complex_purity_derivative(theta, h, s, sc.purity_derivative);
		}
	}
	// Host side of the Training*Kernel scalar members: drains the stream, reads the raw device sums back and applies the closed-form factors.
	// Called with the call lock held, either from *_fit_create (scalars requested) or later from *_fit_get_scalars.
	template <typename F>
	int fit_finalize(gple_ctx* ctx, F* f)
	{
		GPLE_TRY(validate_fit(ctx, f)); // the scalar block is in the pinned host block now, of a factorisation that completed
		timer_collect(ctx);
		const double* h = ctx->host_scalars;
		fill_nan_scalars(&f->sc);
		std::memcpy(&f->sc.info, h + SDEV_INFO, sizeof(int));
		f->s_host = f->sc.rescale_factor = h[0];
		closed_form_scalars(f, h);
		f->sc_ready = true;
		return settle_fit(ctx, f);
	}
	// both *_fit_create once the handle's parameters are set (call lock held): factorisation and post enqueued, then the scalars finalized — or
	// left to *_fit_get_scalars when there is no struct to fill; the fit is deleted on an error
	template <typename F>
	int fit_create(gple_ctx* ctx, F* f, const double* X, const double* y, int y_stride, size_t N, unsigned flags, decltype(F::sc)* scalars, F** out)
	{
		int status = fit_common(ctx, f, X, y, y_stride, N, flags);
		if (status == GPLE_OK)
		{
			status = fit_post(ctx, f);
			timer_stop(ctx, GPLE_TIMER_FIT);
		}
		if (status != GPLE_OK)
		{
			(void)hipStreamSynchronize(ctx->stream);
			delete f;
			return status;
		}
		if (scalars) // no struct to fill: everything stays enqueued, *_fit_get_scalars() drains the stream later
		{
			status = fit_finalize(ctx, f); // (nothing was enqueued on the fit before this: never GPLE_ERR_TIMEOUT for stale uses)
			if (status != GPLE_OK)
			{
				delete f;
				return status;
			}
			*scalars = f->sc;
		}
		*out = f;
		return GPLE_OK;
	}
	int fit_retain(FitCommon* fit)
	{
		if (!fit) return GPLE_ERR_BAD_ARG;
		fit->refs.fetch_add(1);
		return GPLE_OK;
	}
} // namespace

namespace gple
{
	int note_give_up(gple_ctx* ctx, int attempt)
	{
		ctx->dag_giveups += 1;
		if (attempt == 1)
		{
			std::lock_guard<std::mutex> lk(ctx->mu);
			ctx->last_error = "the factorisation gave up waiting (info = -1) and so did its repetition with one launch per panel";
			return GPLE_ERR_TIMEOUT;
		}
		ctx->dag_recoveries += 1;
		return GPLE_OK;
	}

	int real_fit_create_masked(gple_ctx* ctx, const double theta[4], const double* X, const double* y, int y_is_complex, size_t N,
		unsigned flags, unsigned deriv_mask, gple_real_fit_scalars* scalars, gple_real_fit** out)
	{
		if (!ctx || !theta || !X || !y || !out || N == 0 || N > (1u << 20)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		*out = nullptr;
		GPLE_CALL(ctx);
		gple_real_fit* f = new (std::nothrow) gple_real_fit;
		if (!f) return GPLE_ERR_ALLOC;
		std::memcpy(f->theta, theta, sizeof(f->theta));
		const double sf = theta[0], sn = theta[3];
		f->ps.p[0] = f->ps.p[1] = f->ps.p[2] = make_se(sf * sf, sn * sn, theta[1], theta[2]);
		f->self = (sf * sf) * (1.0 + (sn * sn) * 1.0); // KernelBase(params, col, col).get_kernel().value(), kernel.cpp:512
		f->sf = sf;
		f->deriv_mask = deriv_mask;
		return fit_create(ctx, f, X, y, y_is_complex ? 2 : 1, N, flags, scalars, out);
	}
	int complex_fit_create_masked(gple_ctx* ctx, const double theta[8], const double* X, const double* y, size_t N, unsigned flags,
		unsigned deriv_mask, gple_complex_fit_scalars* scalars, gple_complex_fit** out)
	{
		if (!ctx || !theta || !X || !y || !out || N == 0 || N > (1u << 19)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		*out = nullptr;
		GPLE_CALL(ctx);
		gple_complex_fit* f = new (std::nothrow) gple_complex_fit;
		if (!f) return GPLE_ERR_ALLOC;
		f->is_complex = true;
		std::memcpy(f->theta, theta, sizeof(f->theta));
		const double s0 = theta[0], sR = theta[1], lR0 = theta[2], lR1 = theta[3], sI = theta[4], lI0 = theta[5], lI1 = theta[6],
					 sn = theta[7];
		// correlation kernel parameters, complex_kernel.cpp:144-157
		const double ss0 = lR0 * lR0 + lI0 * lI0, ss1 = lR1 * lR1 + lI1 * lI1;
		const double sC = std::sqrt(sR * sI * ((2.0 * lR0 * lI0 / ss0) * (2.0 * lR1 * lI1 / ss1)));
		const double lC0 = std::sqrt(ss0 / 2.0), lC1 = std::sqrt(ss1 / 2.0);
		const double m2 = s0 * s0;
		// blocks of the real covariance of [Re; Im]: Cxx = s^2 (kR + sn^2/2 d), Cyy = s^2 (kI + sn^2/2 d), Cxy = s^2 kC
		f->ps.p[0] = make_se(m2 * (sR * sR), (sn * sn) / (2.0 * sR * sR), lR0, lR1);
		f->ps.p[1] = make_se(m2 * (sC * sC), 0.0, lC0, lC1);
		f->ps.p[2] = make_se(m2 * (sI * sI), (sn * sn) / (2.0 * sI * sI), lI0, lI1);
		f->self = m2 * (sR * sR * (1.0 + 0.0) + sI * sI * (1.0 + 0.0) + sn * sn * 1.0); // complex_kernel.cpp:632
		f->s0 = s0;
		build_dspecs(theta, f->dspec);
		f->deriv_mask = deriv_mask;
		return fit_create(ctx, f, X, y, 2, N, flags, scalars, out);
	}
	template <typename F>
	int fit_get_scalars(F* fit, decltype(F::sc)* out)
	{
		if (!fit || !out) return GPLE_ERR_BAD_ARG;
		gple_ctx* ctx = fit->ctx;
		GPLE_CALL(ctx);
		const int status = fit->sc_ready ? settle_fit(ctx, fit) : fit_finalize(ctx, fit);
		if (fit->sc_ready) *out = fit->sc; // (GPLE_ERR_TIMEOUT for earlier work included: these are the good fit's scalars)
		return status;
	}
	template <typename F>
	int fit_release(F* fit)
	{
		if (!fit) return GPLE_OK;
		if (fit->refs.fetch_sub(1) == 1)
		{
			(void)hipSetDevice(fit->ctx->device);
			(void)hipStreamSynchronize(fit->ctx->stream); // work that still reads the fit's buffers
			delete fit;                                   // may drop the last reference on a destroyed context
		}
		return GPLE_OK;
	}
	template int fit_get_scalars(gple_real_fit*, gple_real_fit_scalars*);
	template int fit_get_scalars(gple_complex_fit*, gple_complex_fit_scalars*);
	template int fit_release(gple_real_fit*);
	template int fit_release(gple_complex_fit*);

	// ---- PredictiveKernel --------------------------------------------------------------------------------------
	void predict_scalars_from_host(gple_ctx* ctx, bool has_labels, bool want_deriv, bool cplx, gple_predict_scalars* scalars)
	{
		if (!scalars) return;
		if (has_labels) scalars->error = ctx->host_scalars[HS_PRED_ERR];
		if (want_deriv)
			for (int ip = 0; ip < (cplx ? 8 : 4); ++ip) scalars->error_derivative[ip] = ctx->host_scalars[HS_PRED_DERIV + ip];
	}
	static int predict_pass(gple_ctx* ctx, const FitCommon* f, const double* Xs, size_t M, unsigned flags, const double* labels,
		double* prediction, double* variance, double* cutoff_prediction, gple_predict_scalars* scalars);
	// host outputs (and the error scalar) need the stream drained; device-pointer calls without labels stay asynchronous
	// (pooled scratch is only ever reused by later work on this same stream, which the stream orders)
	static bool predict_drains(unsigned flags, const double* labels) { return !(flags & PREDICT_NO_SYNC) && (!(flags & GPLE_IO_DEVICE) || labels); }
	int predict_common(gple_ctx* ctx, const FitCommon* f, const double* Xs, size_t M, unsigned flags, const double* labels,
		double* prediction, double* variance, double* cutoff_prediction, gple_predict_scalars* scalars)
	{
		if (scalars)
		{
			scalars->error = nan_();
			for (double& d : scalars->error_derivative) d = nan_();
		}
		if (M == 0) return GPLE_OK;
		if ((flags & GPLE_CALC_DERIVATIVE) && labels && !f->dv) return GPLE_ERR_STATE; // needs a fit built with GPLE_CALC_DERIVATIVE
		GPLE_CALL(ctx);
		// A predict that drains the stream on a fit the host has not looked at yet looks at it (validate_fit): if the one-launch factorisation had
		// given up, the fit has been repeated with a launch per panel by then and this predict — whose first pass produced NaN — runs again.
		const bool unvalidated = !f->validated.load();
		GPLE_TRY(predict_pass(ctx, f, Xs, M, flags, labels, prediction, variance, cutoff_prediction, scalars));
		if (!predict_drains(flags, labels)) return GPLE_OK;
		if (unvalidated && f->recovered.load()) GPLE_TRY(predict_pass(ctx, f, Xs, M, flags, labels, prediction, variance, cutoff_prediction, scalars));
		return settle_fit(ctx, f);
	}
	static int predict_pass(gple_ctx* ctx, const FitCommon* f, const double* Xs, size_t M, unsigned flags, const double* labels,
		double* prediction, double* variance, double* cutoff_prediction, gple_predict_scalars* scalars)
	{
		const bool unvalidated = !f->validated.load();
		const bool want_deriv = (flags & GPLE_CALC_DERIVATIVE) && labels;
		hipStream_t st = ctx->stream;
		const bool dev = flags & GPLE_IO_DEVICE;
		const bool cplx = f->is_complex;
		const int Mi = static_cast<int>(M);
		const int Mh = static_cast<int>(round_up(M, 128));
		const int m_rows = cplx ? 2 * Mh : Mh;
		const size_t ow = cplx ? 2 : 1; // doubles per prediction entry
		Scratch q(ctx), mu(ctx), epart(ctx), dacc(ctx), dpart(ctx);
		Staged xs(ctx, dev), lab(ctx, dev), o_mean(ctx, dev), o_var(ctx, dev), o_cut(ctx, dev);
		timer_start(ctx, GPLE_TIMER_PREDICT);
		const double* xs_dev = Xs;
		const bool small_host = !dev && M <= FEW_HOST_POINTS && !(flags & PREDICT_NO_SYNC); // (a deferred call must not leave its inputs in the shared block)
		if (small_host)
		{
			std::memcpy(ctx->host_scalars + HS_FEW_XS, Xs, 2 * M * sizeof(double));
			xs_dev = ctx->host_scalars + HS_FEW_XS;
		}
		else
		{
			GPLE_HIP(ctx, xs.in(Xs, 2 * M));
			xs_dev = xs.p;
		}
		GPLE_HIP(ctx, q.get(m_rows));
		GPLE_HIP(ctx, mu.get(m_rows));
		PredictArgs a{};
		a.Xs = xs_dev, a.M = Mi, a.m_rows = m_rows, a.m_split = cplx ? Mh : m_rows;
		a.Xt = f->Xt, a.N = f->N, a.n_total = f->n_total, a.n_split = cplx ? f->Np : f->n_total;
		a.T = f->T, a.ldt = f->n_total, a.v = f->v, a.q = q.p, a.mu = mu.p, a.ps = f->ps;
		if (!(flags & GPLE_PREDICT_FULL))
		{
			// |k*|^2 below this cannot move the variance (gple_predict.hip, Prune): lambda_min(K) >= amp n2, k(x*,x*) = self.
			// Complex GP in its [Re; Im] embedding: the covariance is a valid (positive semi-definite) cross-covariance of two
			// squared-exponential processes plus s^2 sn^2 / 2 on the whole diagonal (p[0].amp p[0].n2 = p[2].amp p[2].n2), and the
			// variance subtracts the contractions of TWO typed rows per point: half the budget each.
			a.prune_thr = std::ldexp(f->self * f->ps.p[0].amp * f->ps.p[0].n2, cplx ? -57 : -56);
			if (!ctx->prune_stats)
			{
				GPLE_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->prune_stats), 4 * sizeof(unsigned long long))); // [2]: the work-queue counter
				GPLE_HIP(ctx, hipMemsetAsync(ctx->prune_stats, 0, 4 * sizeof(unsigned long long), st));
			}
			a.prune_stats = ctx->prune_stats;
		}
		if (want_deriv)
		{
			GPLE_HIP(ctx, dacc.get((cplx ? 15 : 7) * static_cast<size_t>(m_rows)));
			a.dv = f->dv, a.dacc = dacc.p;
			a.complex_deriv = cplx ? 1 : 0;
			if (cplx) std::memcpy(a.dspec, f->dspec, sizeof(a.dspec));
		}
		// How much of the variance contraction the caller's outputs need.  The objective
		// of opt.cpp:441-482 asks for Error (+ ErrorDerivatives) only: Error uses the UNCUT mean (kernel.cpp:522) — no contraction at all, every
		// value-only evaluation of the derivative-free searches; ErrorDerivatives use the cut one (:527), where the variance only decides the
		// cut-off factor — and a point with |mu|^2 >= 4 k(x*,x*) >= 4 var has factor 1 (kernel.h:301-332) whatever q is.
		if (!variance && !cutoff_prediction)
		{
			if (!want_deriv) a.mean_only = 1;
			else
			{
				a.cut_thr = 4.0 * f->self;
				if (!ctx->prune_stats)
				{
					GPLE_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->prune_stats), 4 * sizeof(unsigned long long)));
					GPLE_HIP(ctx, hipMemsetAsync(ctx->prune_stats, 0, 4 * sizeof(unsigned long long), st));
				}
				a.prune_stats = ctx->prune_stats;
			}
		}
		int chunk_rows = 0;
		bool few_rows = false, late_contraction = false, finished = false;
		Scratch kstar(ctx);
		if (predict_is_few(a)) // one-point predicts of the reference's callers: no padding, no K*, no GEMM
		{
			GPLE_HIP(ctx, kstar.get(predict_few_scratch_doubles(a)));
			GPLE_HIP(ctx, launch_predict_few(st, a, kstar.p));
		}
		else
		{
			GPLE_HIP(ctx, kstar.get(predict_scratch_doubles(a, &chunk_rows, &few_rows)));
			late_contraction = true;
		}
		const double* lab_dev = labels;
		if (labels && small_host)
		{
			std::memcpy(ctx->host_scalars + HS_FEW_LAB, labels, ow * M * sizeof(double));
			lab_dev = ctx->host_scalars + HS_FEW_LAB;
		}
		else
		{
			GPLE_HIP(ctx, lab.in(labels, ow * M));
			lab_dev = lab.p;
		}
		double *d_mean = prediction, *d_var = variance, *d_cut = cutoff_prediction;
		if (small_host)
		{
			if (prediction) d_mean = ctx->host_scalars + HS_FEW_MEAN;
			if (variance) d_var = ctx->host_scalars + HS_FEW_VAR;
			if (cutoff_prediction) d_cut = ctx->host_scalars + HS_FEW_CUT;
		}
		else
		{
			GPLE_HIP(ctx, o_mean.out(prediction, ow * M));
			GPLE_HIP(ctx, o_var.out(variance, M));
			GPLE_HIP(ctx, o_cut.out(cutoff_prediction, ow * M));
			d_mean = o_mean.p, d_var = o_var.p, d_cut = o_cut.p;
		}
		if (late_contraction)
		{
			// (the output buffers are known by now: a kernel that holds a row's mean and q together may write the outputs itself — predict_fused256_kernel)
			if (!cplx && !labels && !want_deriv) a.fin_sdev = f->sdev, a.fin_self = f->self, a.fin_mean = d_mean, a.fin_var = d_var, a.fin_cut = d_cut;
			GPLE_HIP(ctx, launch_predict_q(ctx, st, a, kstar.p, chunk_rows, few_rows, &finished));
		}
		const int nblk = (Mi + 255) / 256;
		double* err_part = nullptr;
		if (labels)
		{
			GPLE_HIP(ctx, epart.get(nblk + 1));
			err_part = epart.p;
		}
		if (finished) {}
		else if (cplx)
			GPLE_HIP(ctx, launch_predict_finish_complex(st, q.p, mu.p, Mi, Mh, f->self, f->sdev, lab_dev, d_mean, d_var, d_cut, err_part));
		else
			GPLE_HIP(ctx, launch_predict_finish_real(st, q.p, mu.p, Mi, f->self, f->sdev, lab_dev, d_mean, d_var, d_cut, err_part));
		if (labels)
		{
			GPLE_HIP(ctx, launch_sum(st, err_part, nblk, err_part + nblk));
			GPLE_HIP(ctx, hipMemcpyAsync(ctx->host_scalars + HS_PRED_ERR, err_part + nblk, 8, hipMemcpyDeviceToHost, st));
		}
		if (want_deriv)
		{
			GPLE_HIP(ctx, dpart.get(8 * static_cast<size_t>(nblk) + 8));
			if (cplx)
				GPLE_HIP(ctx, launch_predict_deriv_finish_complex(st, dacc.p, m_rows, Mh, q.p, Mi, f->self, f->s0, f->sdev, lab_dev, dpart.p,
								  dpart.p + 8 * nblk));
			else
				GPLE_HIP(ctx, launch_predict_deriv_finish_real(st, dacc.p, m_rows, q.p, Mi, f->self, f->sf, f->sdev, lab_dev, dpart.p, dpart.p + 8 * nblk));
			GPLE_HIP(ctx, hipMemcpyAsync(ctx->host_scalars + HS_PRED_DERIV, dpart.p + 8 * nblk, 8 * 8, hipMemcpyDeviceToHost, st));
		}
		for (Staged* o : {&o_mean, &o_var, &o_cut}) GPLE_HIP(ctx, o->back()); // (nothing to copy for device arrays and the pinned block)
		timer_stop(ctx, GPLE_TIMER_PREDICT);
		if (!predict_drains(flags, labels))
		{
			// enqueued only (internal NO_SYNC: the caller drains the stream and reads the scalars itself; device pointers without labels): if the
			// factorisation turns out to have given up, these outputs are NaN and the fit's next draining call says so (settle_fit)
			if (unvalidated) f->stale_uses.fetch_add(1);
			if (flags & PREDICT_NO_SYNC) return GPLE_OK;
		}
		else
		{
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			timer_collect(ctx);
			if (unvalidated) GPLE_TRY(validate_fit(ctx, f)); // (recovered: what this pass computed is NaN, predict_common runs it again)
		}
		if (small_host) // the kernels wrote into the pinned block
		{
			if (prediction) std::memcpy(prediction, ctx->host_scalars + HS_FEW_MEAN, ow * M * sizeof(double));
			if (variance) std::memcpy(variance, ctx->host_scalars + HS_FEW_VAR, M * sizeof(double));
			if (cutoff_prediction) std::memcpy(cutoff_prediction, ctx->host_scalars + HS_FEW_CUT, ow * M * sizeof(double));
		}
		predict_scalars_from_host(ctx, labels != nullptr, want_deriv, cplx, scalars);
		return GPLE_OK;
	}
	// One-point predict with host pointers and no labels — what main.cpp:83,94 issues per call, from as many threads as TBB has.
	// The calls on one context are serialised anyway (one stream); instead of queueing behind each other, the requests that
	// pile up while a predict is in flight ride together on the next one (up to 16 typed rows: the few-points path costs the
	// same for 16 points as for one).  Every caller still returns with its own result; a single-threaded caller sees a batch of one.
	static int predict_point_combined(gple_ctx* ctx, const FitCommon* f, const double* x, double* prediction, double* variance,
		double* cutoff_prediction)
	{
		const size_t ow = f->is_complex ? 2 : 1, cap = FEW_HOST_POINTS / ow;
		FitCommon::PointRequest r{x, prediction, variance, cutoff_prediction, GPLE_OK, false};
		std::unique_lock<std::mutex> lk(f->point_mu);
		f->point_pending.push_back(&r);
		for (;;)
		{
			if (r.done) return r.status;
			if (f->point_leader)
			{
				f->point_cv.wait(lk);
				continue;
			}
			f->point_leader = true; // serve the oldest requests (this thread's own is among the pending ones; FIFO gets to it)
			const size_t nb = std::min(cap, f->point_pending.size());
			FitCommon::PointRequest* batch[FEW_HOST_POINTS];
			double xs[2 * FEW_HOST_POINTS], mean[2 * FEW_HOST_POINTS], var[FEW_HOST_POINTS], cut[2 * FEW_HOST_POINTS];
			for (size_t i = 0; i < nb; ++i)
			{
				batch[i] = f->point_pending[i];
				xs[2 * i] = batch[i]->x[0], xs[2 * i + 1] = batch[i]->x[1];
			}
			f->point_pending.erase(f->point_pending.begin(), f->point_pending.begin() + static_cast<long>(nb));
			lk.unlock();
			const int st = predict_common(ctx, f, xs, nb, 0u, nullptr, mean, var, cut, nullptr);
			lk.lock();
			for (size_t i = 0; i < nb; ++i)
			{
				FitCommon::PointRequest* q = batch[i];
				if (own_outputs_written(st, f))
				{
					if (q->mean) std::memcpy(q->mean, mean + ow * i, ow * sizeof(double));
					if (q->var) *q->var = var[i];
					if (q->cut) std::memcpy(q->cut, cut + ow * i, ow * sizeof(double));
				}
				q->status = st;
				q->done = true;
			}
			f->point_leader = false;
			f->point_cv.notify_all();
		}
	}

	int fit_predict(gple_ctx* ctx, const FitCommon* fit, const double* Xs, size_t M, unsigned flags, const double* labels, double* prediction,
		double* variance, double* cutoff_prediction, gple_predict_scalars* scalars)
	{
		if (!ctx || !fit || (M && !Xs)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (M == 1 && !labels && !(flags & GPLE_IO_DEVICE))
		{
			if (scalars)
			{
				scalars->error = nan_();
				for (double& d : scalars->error_derivative) d = nan_();
			}
			return predict_point_combined(ctx, fit, Xs, prediction, variance, cutoff_prediction);
		}
		return predict_common(ctx, fit, Xs, M, flags, labels, prediction, variance, cutoff_prediction, scalars);
	}
} // namespace gple

extern "C"
{
	int gple_real_fit_create(gple_ctx* ctx, const double theta[4], const double* X, const double* y, int y_is_complex, size_t N,
		unsigned flags, gple_real_fit_scalars* scalars, gple_real_fit** out)
	{
		return real_fit_create_masked(ctx, theta, X, y, y_is_complex, N, flags, 0xFFu, scalars, out);
	}
	int gple_real_fit_get_scalars(gple_real_fit* fit, gple_real_fit_scalars* out) { return fit_get_scalars(fit, out); }
	int gple_real_fit_retain(gple_real_fit* fit) { return fit_retain(fit); }
	int gple_real_fit_release(gple_real_fit* fit) { return fit_release(fit); }
	size_t gple_real_fit_size(const gple_real_fit* fit) { return fit ? fit->N : 0; }

	int gple_real_fit_get(gple_real_fit* f, gple_real_array which, unsigned flags, double* dst)
	{
		if (!f || !dst) return GPLE_ERR_BAD_ARG;
		gple_ctx* ctx = f->ctx;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t N = f->N;
		const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
		if (!f->validated.load()) GPLE_TRY(validate_fit(ctx, f)); // (a getter drains the stream anyway)
		switch (which)
		{
		case GPLE_R_KERNEL:
		{
			Scratch k(ctx);
			GPLE_HIP(ctx, k.get(N * N));
			GPLE_HIP(ctx, launch_gram_rect(st, f->Xt, (int)N, f->Xt, (int)N, 1, f->ps.p[0], f->theta[0], f->theta[3], k.p, nullptr));
			GPLE_HIP(ctx, hipMemcpyAsync(dst, k.p, N * N * 8, kind, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			break;
		}
		case GPLE_R_INVERSE:
			GPLE_TRY(ensure_inverse(f));
			GPLE_HIP(ctx, hipMemcpy2DAsync(dst, N * 8, f->W, static_cast<size_t>(f->n_total) * 8, N * 8, N, kind, st));
			break;
		case GPLE_R_INVLBL: GPLE_HIP(ctx, hipMemcpyAsync(dst, f->v, N * 8, kind, st)); break;
		case GPLE_R_LABEL: GPLE_HIP(ctx, hipMemcpyAsync(dst, f->ys, N * 8, kind, st)); break;
		case GPLE_R_INVERSE_DIAG: GPLE_HIP(ctx, hipMemcpyAsync(dst, f->w, N * 8, kind, st)); break;
		case GPLE_R_INVLBL_DERIV:
			if (!f->dv) return GPLE_ERR_STATE;
			GPLE_HIP(ctx, hipMemcpy2DAsync(dst, N * 8, f->dv, static_cast<size_t>(f->n_total) * 8, N * 8, 4, kind, st));
			break;
		default: return GPLE_ERR_BAD_ARG;
		}
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		return settle_fit(ctx, f);
	}

	int gple_complex_fit_create(gple_ctx* ctx, const double theta[8], const double* X, const double* y, size_t N, unsigned flags,
		gple_complex_fit_scalars* scalars, gple_complex_fit** out)
	{
		return complex_fit_create_masked(ctx, theta, X, y, N, flags, 0xFFu, scalars, out);
	}
	int gple_complex_fit_get_scalars(gple_complex_fit* fit, gple_complex_fit_scalars* out) { return fit_get_scalars(fit, out); }
	int gple_complex_fit_retain(gple_complex_fit* fit) { return fit_retain(fit); }
	int gple_complex_fit_release(gple_complex_fit* fit) { return fit_release(fit); }
	size_t gple_complex_fit_size(const gple_complex_fit* fit) { return fit ? fit->N : 0; }

	int gple_complex_fit_get(gple_complex_fit* f, gple_complex_array which, unsigned flags, double* dst)
	{
		if (!f || !dst) return GPLE_ERR_BAD_ARG;
		gple_ctx* ctx = f->ctx;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t N = f->N;
		const int Np = f->Np, nt = f->n_total;
		const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
		Scratch tmp(ctx), big(ctx);
		const dim3 grid2((N + 63) / 64, (N + 3) / 4), blk(256);
		if (!f->validated.load()) GPLE_TRY(validate_fit(ctx, f)); // (a getter drains the stream anyway)
		switch (which)
		{
		case GPLE_C_KERNEL:
		case GPLE_C_PSEUDO:
		{
			const size_t len = which == GPLE_C_KERNEL ? N * N : 2 * N * N;
			GPLE_HIP(ctx, big.get(static_cast<size_t>(nt) * nt));
			GPLE_HIP(ctx, tmp.get(len));
			GPLE_HIP(ctx, launch_gram_train(st, f->Xt, f->N, Np, nt, f->ps, big.p, nt));
			hipLaunchKernelGGL(complex_kernels_kernel, grid2, blk, 0, st, big.p, nt, (int)N, Np, which == GPLE_C_KERNEL ? 0 : 1, tmp.p);
			GPLE_HIP(ctx, hipGetLastError());
			GPLE_HIP(ctx, hipMemcpyAsync(dst, tmp.p, len * 8, kind, st));
			break;
		}
		case GPLE_C_UPPER_LEFT:
		case GPLE_C_LOWER_LEFT:
			GPLE_TRY(ensure_inverse(f));
			GPLE_HIP(ctx, tmp.get(2 * N * N));
			hipLaunchKernelGGL(complex_blocks_kernel, grid2, blk, 0, st, f->W, nt, (int)N, Np, which == GPLE_C_UPPER_LEFT ? 0 : 1, tmp.p);
			GPLE_HIP(ctx, hipGetLastError());
			GPLE_HIP(ctx, hipMemcpyAsync(dst, tmp.p, 2 * N * N * 8, kind, st));
			break;
		case GPLE_C_INVLBL:
			GPLE_HIP(ctx, tmp.get(2 * N));
			hipLaunchKernelGGL(halve_pair_kernel, dim3((N + 255) / 256), blk, 0, st, f->v, (int)N, Np, tmp.p);
			GPLE_HIP(ctx, hipGetLastError());
			GPLE_HIP(ctx, hipMemcpyAsync(dst, tmp.p, 2 * N * 8, kind, st));
			break;
		case GPLE_C_LABEL:
			GPLE_HIP(ctx, tmp.get(2 * N));
			hipLaunchKernelGGL(pair_kernel, dim3((N + 255) / 256), blk, 0, st, f->ys, (int)N, Np, tmp.p);
			GPLE_HIP(ctx, hipGetLastError());
			GPLE_HIP(ctx, hipMemcpyAsync(dst, tmp.p, 2 * N * 8, kind, st));
			break;
		case GPLE_C_INVLBL_DERIV:
			if (!f->dv) return GPLE_ERR_STATE;
			GPLE_HIP(ctx, tmp.get(16 * N));
			for (int ip = 0; ip < 8; ++ip)
			{
				hipLaunchKernelGGL(halve_pair_kernel, dim3((N + 255) / 256), blk, 0, st, f->dv + static_cast<size_t>(ip) * nt, (int)N, Np, tmp.p + 2 * ip * N);
				GPLE_HIP(ctx, hipGetLastError());
			}
			GPLE_HIP(ctx, hipMemcpyAsync(dst, tmp.p, 16 * N * 8, kind, st));
			break;
		default: return GPLE_ERR_BAD_ARG;
		}
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		return settle_fit(ctx, f);
	}

	int gple_real_predict(gple_ctx* ctx, const gple_real_fit* fit, const double* Xs, size_t M, unsigned flags, const double* labels,
		double* prediction, double* variance, double* cutoff_prediction, gple_predict_scalars* scalars)
	{
		return fit_predict(ctx, fit, Xs, M, flags, labels, prediction, variance, cutoff_prediction, scalars);
	}
	int gple_complex_predict(gple_ctx* ctx, const gple_complex_fit* fit, const double* Xs, size_t M, unsigned flags, const double* labels,
		double* prediction, double* variance, double* cutoff_prediction, gple_predict_scalars* scalars)
	{
		return fit_predict(ctx, fit, Xs, M, flags, labels, prediction, variance, cutoff_prediction, scalars);
	}

	/* gple_debug.h: the layout the factorisation of an n-column matrix will use (host logic only, no device call): outer block bounds
	 * (0 … n), fork points of the block-row inverse, workspace doubles.  Arrays of `cap` ints; counts come back in nb / nf. */
	// test knobs of the factorisation on this context; a negative argument leaves that knob as it is.  scheme: 0 = a launch per panel, 1 = one
	// launch per outer block, 2 = back to GPLE_CHOL_SCHEME; poll_limit: polls before a waiting wave of the one-launch scheme gives up (0: default);
	// dag_blocks: workgroups of its launches (0: one per CU).  giveups / recoveries (nullable): the context's counters so far.
	int gple_debug_chol_knobs(gple_ctx* ctx, int scheme, int poll_limit, int dag_blocks, long* giveups, long* recoveries)
	{
		if (!ctx) return GPLE_ERR_BAD_ARG;
		std::lock_guard<std::mutex> lk(ctx->call_mu);
		if (scheme >= 0) ctx->chol_scheme = scheme >= 2 ? -1 : scheme;
		if (poll_limit >= 0) ctx->dag_poll_limit = poll_limit;
		if (dag_blocks >= 0) ctx->dag_blocks = dag_blocks;
		if (giveups) *giveups = ctx->dag_giveups;
		if (recoveries) *recoveries = ctx->dag_recoveries;
		return GPLE_OK;
	}
	// gple_debug.h: the fit's inverse Cholesky factor as the predict kernels read it (validated first, like every getter)
	int gple_debug_fit_factor(const gple_real_fit* real, const gple_complex_fit* cplx, double* T, size_t capacity, int* n_total, int* n_split, int* N)
	{
		if ((real != nullptr) == (cplx != nullptr)) return GPLE_ERR_BAD_ARG; // exactly one of the two
		FitCommon* f = real ? static_cast<FitCommon*>(const_cast<gple_real_fit*>(real)) : static_cast<FitCommon*>(const_cast<gple_complex_fit*>(cplx));
		gple_ctx* ctx = f->ctx;
		GPLE_CALL(ctx);
		const size_t nt = static_cast<size_t>(f->n_total);
		if (n_total) *n_total = f->n_total;
		if (n_split) *n_split = f->Np;
		if (N) *N = f->N;
		if (!T && capacity == 0) return GPLE_OK; // a question about the sizes only
		if (!T || capacity < nt * nt) return GPLE_ERR_BAD_ARG;
		if (!f->validated.load()) GPLE_TRY(validate_fit(ctx, f)); // (a getter drains the stream anyway)
		GPLE_HIP(ctx, hipMemcpyAsync(T, f->T, nt * nt * 8, hipMemcpyDeviceToHost, ctx->stream));
		GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return settle_fit(ctx, f);
	}
	const char* gple_debug_last_contraction_kernel(gple_ctx* ctx) { return ctx ? ctx->last_contraction : ""; }
	int gple_debug_predict_knobs(gple_ctx* ctx, int rownorm_pipe, int fused_small)
	{
		if (!ctx) return GPLE_ERR_BAD_ARG;
		std::lock_guard<std::mutex> lk(ctx->call_mu);
		if (rownorm_pipe >= 0) ctx->rownorm_pipe = rownorm_pipe >= 2 ? -1 : rownorm_pipe;
		if (fused_small >= 0) ctx->fused_small = fused_small >= 2 ? -1 : fused_small;
		return GPLE_OK;
	}
	int gple_debug_chol_layout(int n, int cap, int* bounds, int* nb, int* forks, int* nf, unsigned long long* work_doubles)
	{
		if (n <= 0 || n % 64 || !bounds || !nb || !forks || !nf || !work_doubles) return GPLE_ERR_BAD_ARG;
		std::vector<int> b, f;
		size_t w = 0;
		chol_layout(n, b, f, w);
		if (static_cast<int>(b.size()) > cap || static_cast<int>(f.size()) > cap) return GPLE_ERR_BAD_ARG;
		std::copy(b.begin(), b.end(), bounds), std::copy(f.begin(), f.end(), forks);
		*nb = static_cast<int>(b.size()), *nf = static_cast<int>(f.size()), *work_doubles = w;
		return GPLE_OK;
	}

	/* gple_debug.h: the outcome of the side stream's queue probing (gple_chol.hip, pick_side_stream) */
	int gple_debug_side_stream(gple_ctx* ctx, int* attempts, int* overlaps)
	{
		if (!ctx || !attempts || !overlaps) return GPLE_ERR_BAD_ARG;
		std::lock_guard<std::mutex> lk(ctx->call_mu);
		*attempts = ctx->side_attempts, *overlaps = ctx->side_overlaps ? 1 : 0;
		return GPLE_OK;
	}

	/* gple_debug.h: instrumented launches of the one-launch panel step (potrf_step_kernel) at block column 1 of an n x n matrix,
	 * n = 128 + below (below = 0 | 64), column-major on the host, overwritten with what the first launch leaves; T (n x n) likewise. */
	int gple_debug_potrf_step(gple_ctx* ctx, double* A, double* T, int pend, int below, long long* stamps, int reps, float* ms_per_launch)
	{
		if (!ctx || !A || !T || !stamps || (below != 0 && below != 64)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		const int n = 128 + below;
		Scratch a(ctx), t(ctx), aux(ctx);
		GPLE_HIP(ctx, a.get(n * n));
		GPLE_HIP(ctx, t.get(n * n));
		GPLE_HIP(ctx, aux.get(40));
		GPLE_HIP(ctx, hipMemsetAsync(aux.p, 0, 40 * 8, st));
		GPLE_HIP(ctx, hipMemsetAsync(t.p, 0, sizeof(double) * n * n, st));
		GPLE_HIP(ctx, copy_in(st, a.p, A, n * n, false));
		hipEvent_t e0, e1;
		GPLE_HIP(ctx, hipEventCreate(&e0));
		GPLE_HIP(ctx, hipEventCreate(&e1));
		GPLE_HIP(ctx, debug_potrf_step(st, a.p, n, t.p, n, reinterpret_cast<int*>(aux.p), reinterpret_cast<long long*>(aux.p + 8), pend, below));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		GPLE_HIP(ctx, hipMemcpy(A, a.p, sizeof(double) * n * n, hipMemcpyDeviceToHost));
		GPLE_HIP(ctx, hipMemcpy(T, t.p, sizeof(double) * n * n, hipMemcpyDeviceToHost));
		GPLE_HIP(ctx, hipEventRecord(e0, st));
		for (int i = 0; i < reps; ++i)
			GPLE_HIP(ctx, debug_potrf_step(st, a.p, n, t.p, n, reinterpret_cast<int*>(aux.p), reinterpret_cast<long long*>(aux.p + 8), pend, below));
		GPLE_HIP(ctx, hipEventRecord(e1, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		float ms = 0.f;
		GPLE_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
		if (ms_per_launch) *ms_per_launch = reps > 0 ? ms / reps : 0.f;
		(void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
		GPLE_HIP(ctx, hipMemcpy(stamps, aux.p + 8, 24 * 8, hipMemcpyDeviceToHost)); // of the last (warm) launch
		{
			int info = 0; // as the first launch left it (atomicCAS from 0): reported in the last stamp slot
			GPLE_HIP(ctx, hipMemcpy(&info, aux.p, sizeof(int), hipMemcpyDeviceToHost));
			stamps[23] = info;
		}
		return GPLE_OK;
	}

	/* gple_debug.h (not part of include/gple.h): one product of the fp64 MFMA GEMM family on host operands, for tests/test_gpu_gemm.py.
	 * C(m,n) = alpha sum_k A(m,k) B(n,k) + beta C(m,n); layouts and k-ranges as GemmDesc (csrc/gple_internal.h);
	 * tile = 32 | 64 | 128 | 0 (the library's own choice for this shape). */
	int gple_debug_gemm(gple_ctx* ctx, const double* A, long lda, int a_kmajor, const double* B, long ldb, int b_kmajor, double* C, long ldc,
		int c_trans, int M, int N, int K, double alpha, double beta, int krange, int lower_only, int tile)
	{
		if (!ctx || !A || !B || !C || M <= 0 || N <= 0 || K <= 0) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		const size_t na = static_cast<size_t>(lda) * (a_kmajor ? M : K), nb = static_cast<size_t>(ldb) * (b_kmajor ? N : K),
					 nc = static_cast<size_t>(ldc) * (c_trans ? M : N);
		Scratch a(ctx), b(ctx), c(ctx);
		GPLE_HIP(ctx, a.get(na));
		GPLE_HIP(ctx, b.get(nb));
		GPLE_HIP(ctx, c.get(nc));
		GPLE_HIP(ctx, copy_in(st, a.p, A, na, false));
		GPLE_HIP(ctx, copy_in(st, b.p, B, nb, false));
		GPLE_HIP(ctx, copy_in(st, c.p, C, nc, false));
		GemmDesc g{};
		g.A = a.p, g.lda = lda, g.B = b.p, g.ldb = ldb, g.C = c.p, g.ldc = ldc;
		g.M = M, g.N = N, g.K = K, g.batch = 1, g.alpha = alpha, g.beta = beta, g.krange = krange, g.lower_only = lower_only;
		g.a_kmajor = a_kmajor != 0, g.b_kmajor = b_kmajor != 0, g.c_trans = c_trans != 0;
		GPLE_HIP(ctx, launch_gemm(st, g, tile ? tile : gemm_pick_tile(M, N, 1, krange != K_FULL || lower_only)));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		GPLE_HIP(ctx, hipMemcpy(C, c.p, nc * 8, hipMemcpyDeviceToHost));
		return GPLE_OK;
	}

	/* gple_debug.h: the same product the way the fits call it — every operand a window of a larger buffer (origin offset, leading dimension beyond
	 * the extent, batch stride; 0 repeats an operand).  The three whole buffers go to the device, one launch runs, the whole C buffer comes back,
	 * so the caller sees what was written outside the windows as well.  Every window is checked against its buffer here: nothing is launched
	 * that would leave one. */
	int gple_debug_gemm_strided(gple_ctx* ctx, const double* A, long countA, long offA, long lda, long strideA, int a_kmajor, const double* B, long countB,
		long offB, long ldb, long strideB, int b_kmajor, double* C, long countC, long offC, long ldc, long strideC, int c_trans, int batch, int M, int N, int K,
		double alpha, double beta, int krange, int lower_only, int tile)
	{
		if (!ctx || !A || !B || !C || M <= 0 || N <= 0 || K <= 0 || batch <= 0) return GPLE_ERR_BAD_ARG;
		// rows x cols window, `fast` contiguous: the last element of the last item must lie inside the buffer; the kernels load 16- and 32-byte vectors
		auto inside = [batch](long count, long off, long ld, long stride, long fast, long slow) {
			if (off < 0 || stride < 0 || ld < fast || count <= 0 || off % 4 || ld % 4 || stride % 4) return false;
			return off + (batch - 1) * stride + (slow - 1) * ld + fast <= count;
		};
		if (!inside(countA, offA, lda, strideA, a_kmajor ? K : M, a_kmajor ? M : K) || !inside(countB, offB, ldb, strideB, b_kmajor ? K : N, b_kmajor ? N : K) ||
			!inside(countC, offC, ldc, strideC, c_trans ? N : M, c_trans ? M : N))
			return GPLE_ERR_BAD_ARG;
		if (batch > 1 && strideC < (c_trans ? M : N) * ldc) return GPLE_ERR_BAD_ARG; // items of C must not overlap
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Scratch a(ctx), b(ctx), c(ctx);
		GPLE_HIP(ctx, a.get(countA));
		GPLE_HIP(ctx, b.get(countB));
		GPLE_HIP(ctx, c.get(countC));
		GPLE_HIP(ctx, copy_in(st, a.p, A, countA, false));
		GPLE_HIP(ctx, copy_in(st, b.p, B, countB, false));
		GPLE_HIP(ctx, copy_in(st, c.p, C, countC, false));
		GemmDesc g{};
		g.A = a.p + offA, g.lda = lda, g.strideA = strideA, g.B = b.p + offB, g.ldb = ldb, g.strideB = strideB, g.C = c.p + offC, g.ldc = ldc, g.strideC = strideC;
		g.M = M, g.N = N, g.K = K, g.batch = batch, g.alpha = alpha, g.beta = beta, g.krange = krange, g.lower_only = lower_only;
		g.a_kmajor = a_kmajor != 0, g.b_kmajor = b_kmajor != 0, g.c_trans = c_trans != 0;
		GPLE_HIP(ctx, launch_gemm(st, g, tile ? tile : gemm_pick_tile(M, N, 1, krange != K_FULL || lower_only))); // (the tile of ONE product, as the fits pick it)
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		GPLE_HIP(ctx, hipMemcpy(C, c.p, static_cast<size_t>(countC) * 8, hipMemcpyDeviceToHost));
		return GPLE_OK;
	}
}
