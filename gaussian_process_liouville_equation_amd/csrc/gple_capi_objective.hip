// gple_capi_objective.hip — C-ABI entry points of include/gple.h: loose_function, the resident objective and the NLML path.
#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "gple_capi.h"

namespace
{
	// One fit of the objective and the predict of its extra points.  The fit's scalars are deferred and the predict leaves its synchronisation
	// to the scalar getter: the whole evaluation is enqueued in one go and the stream is drained once (a synchronisation between fit and predict
	// would idle the GPU for the host's turn).  Releases `fit`; *result / grad: this part's error and gradient.
	template <typename F>
	int loose_fit_eval(gple_ctx* ctx, F* fit, const double* X_extra, const double* labels, size_t M_extra, unsigned flags, unsigned io, unsigned owned,
		int part, double* result, double* grad)
	{
		constexpr int np = sizeof(F::theta) / sizeof(double);
		const bool want_deriv = (flags & GPLE_CALC_DERIVATIVE) && M_extra;
		const unsigned pflags = (flags & GPLE_CALC_DERIVATIVE) | io | PREDICT_NO_SYNC | GPLE_PREDICT_FULL;
		gple_predict_scalars ps;
		decltype(F::sc) sc;
		int st = fit_predict(ctx, fit, X_extra, M_extra, pflags, labels, nullptr, nullptr, nullptr, &ps);
		if (st == GPLE_OK) st = fit_get_scalars(fit, &sc); // drains the stream
		if (st == GPLE_ERR_TIMEOUT && fit->validated.load()) // settle_fit: the factorisation had given up and was repeated, the predict above saw NaN — once more, on the good fit
		{
			st = fit_predict(ctx, fit, X_extra, M_extra, pflags, labels, nullptr, nullptr, nullptr, &ps);
			if (st == GPLE_OK) st = gple_ctx_synchronize(ctx); // (the scalars are cached by now: the getter would not drain the stream)
			if (st == GPLE_OK) st = fit_get_scalars(fit, &sc);
		}
		fit_release(fit);
		GPLE_TRY(st);
		if (M_extra) predict_scalars_from_host(ctx, true, want_deriv, np == 8, &ps);
		*result = (part == 0 ? sc.error : 0.0) + (M_extra ? ps.error : 0.0);
		if (grad)
			for (int i = 0; i < np; ++i) grad[i] = ((owned >> i & 1u) ? sc.error_derivative[i] : 0.0) + (M_extra ? ps.error_derivative[i] : 0.0);
		return GPLE_OK;
	}
} // namespace

extern "C"
{
	// loose_function (opt.cpp:441-482).  io = 0: host pointers; io = GPLE_IO_DEVICE: everything but x / value / grad is resident
	// (lab = real parts of y_extra, the label vector of the real kernel's PredictiveKernel, opt.cpp:451)
	static int loose_eval(gple_ctx* ctx, const double* x, size_t n, const double* X, const double* y, size_t N, const double* X_extra,
		const double* y_extra, const double* lab, size_t M_extra, unsigned io, double* value, double* grad, int part = 0, int nparts = 1)
	{
		// part / nparts > 1 (gple_objective_eval_part): this call forms the N^3 products of the parameters ip with ip % nparts == part (the cheap
		// first and last parameters belong to part 0) and predicts the rows [lo, hi) of the extra set; the LOOCV error counts on part 0; the
		// sum over the parts is the whole objective and gradient, make_normal is the caller's after that sum
		unsigned owned = 0xFFu; // travels with the fit (FitCommon::deriv_mask), not through the context: other threads' fits on this context are not touched
		if (nparts > 1)
		{
			const size_t per = (M_extra + nparts - 1) / nparts, lo = std::min(M_extra, per * part), hi = std::min(M_extra, lo + per);
			X_extra += 2 * lo, y_extra += 2 * lo, lab += lo, M_extra = hi - lo;
			unsigned mask = 0;
			for (size_t ip = 0; ip < n; ++ip)
				if ((ip == 0 || ip == n - 1) ? part == 0 : static_cast<int>(ip % nparts) == part) mask |= 1u << ip;
			owned = mask;
		}
		const unsigned flags = GPLE_CALC_ERROR | (grad ? GPLE_CALC_DERIVATIVE : 0u);
		double result = 0.0;
		if (n == 4)
		{
			gple_real_fit* fit = nullptr;
			GPLE_TRY(real_fit_create_masked(ctx, x, X, y, 1, N, flags | io, owned, nullptr, &fit));
			GPLE_TRY(loose_fit_eval(ctx, fit, X_extra, lab, M_extra, flags, io, owned, part, &result, grad));
		}
		else
		{
			gple_complex_fit* fit = nullptr;
			GPLE_TRY(complex_fit_create_masked(ctx, x, X, y, N, flags | io, owned, nullptr, &fit));
			GPLE_TRY(loose_fit_eval(ctx, fit, X_extra, y_extra, M_extra, flags, io, owned, part, &result, grad));
		}
		// make_normal, opt.cpp:420-431
		auto make_normal = [](double& d) {
			if (std::isnan(d) || std::isinf(d)) d = std::numeric_limits<double>::max();
		};
		if (nparts == 1)
		{
			make_normal(result);
			if (grad)
				for (size_t i = 0; i < n; ++i) make_normal(grad[i]);
		}
		*value = result;
		return GPLE_OK;
	}
	int gple_loose_function(gple_ctx* ctx, const double* x, size_t n, const double* X, const double* y, size_t N, const double* X_extra,
		const double* y_extra, size_t M_extra, double* value, double* grad)
	{
		if (!ctx || !x || !X || !y || !value || (n != 4 && n != 8) || (M_extra && (!X_extra || !y_extra))) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		std::vector<double> lab(M_extra);
		for (size_t i = 0; i < M_extra; ++i) lab[i] = y_extra[2 * i];
		return loose_eval(ctx, x, n, X, y, N, X_extra, y_extra, lab.data(), M_extra, 0u, value, grad);
	}

	// ---- the objective with its data resident (ElementTrainingParameters of opt.cpp:16) ------------------------------------
	struct gple_objective
	{
		gple_ctx* ctx = nullptr;
		size_t N = 0, M = 0;
		double *X = nullptr, *y = nullptr, *Xe = nullptr, *ye = nullptr, *lab = nullptr;
	};
	int gple_objective_create(gple_ctx* ctx, const double* X, const double* y, size_t N, const double* X_extra, const double* y_extra,
		size_t M_extra, gple_objective** out)
	{
		if (!ctx || !X || !y || !out || N == 0 || (M_extra && (!X_extra || !y_extra))) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		*out = nullptr;
		GPLE_CALL(ctx);
		gple_objective* o = new (std::nothrow) gple_objective;
		if (!o) return GPLE_ERR_ALLOC;
		o->ctx = ctx, o->N = N, o->M = M_extra;
		ctx_retain(ctx); // dropped in gple_objective_release
		hipStream_t st = ctx->stream;
		hipError_t e = hipSuccess;
		auto up = [&](double*& dst, const double* src, size_t n) {
			if (e != hipSuccess || n == 0) return;
			dst = ctx->acquire(n * 8, &e);
			if (e == hipSuccess) e = hipMemcpyAsync(dst, src, n * 8, hipMemcpyHostToDevice, st);
		};
		std::vector<double> lab(M_extra);
		for (size_t i = 0; i < M_extra; ++i) lab[i] = y_extra[2 * i];
		up(o->X, X, 2 * N), up(o->y, y, 2 * N), up(o->Xe, X_extra, 2 * M_extra), up(o->ye, y_extra, 2 * M_extra), up(o->lab, lab.data(), M_extra);
		if (e == hipSuccess) e = hipStreamSynchronize(st); // the host arrays may go away once this returns
		if (e != hipSuccess)
		{
			for (double* p : {o->X, o->y, o->Xe, o->ye, o->lab}) ctx->give_back(p);
			delete o;
			const int status = record_hip_error(ctx, e, "objective upload", __FILE_NAME__, __LINE__);
			ctx_drop(ctx);
			return status;
		}
		*out = o;
		return GPLE_OK;
	}
	int gple_objective_eval(gple_objective* o, const double* x, size_t n, double* value, double* grad)
	{
		if (!o || !x || !value || (n != 4 && n != 8)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(o->ctx);
		return loose_eval(o->ctx, x, n, o->X, o->y, o->N, o->Xe, o->ye, o->lab, o->M, GPLE_IO_DEVICE, value, grad);
	}
	int gple_objective_eval_part(gple_objective* o, const double* x, size_t n, int part, int nparts, double* value, double* grad)
	{
		if (!o || !x || !value || (n != 4 && n != 8) || nparts < 1 || part < 0 || part >= nparts) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(o->ctx);
		return loose_eval(o->ctx, x, n, o->X, o->y, o->N, o->Xe, o->ye, o->lab, o->M, GPLE_IO_DEVICE, value, grad, part, nparts);
	}
	int gple_objective_release(gple_objective* o)
	{
		if (!o) return GPLE_OK;
		gple_ctx* ctx = o->ctx;
		(void)hipSetDevice(ctx->device);
		(void)hipStreamSynchronize(ctx->stream);
		for (double* p : {o->X, o->y, o->Xe, o->ye, o->lab}) ctx->give_back(p);
		delete o;
		ctx_drop(ctx);
		return GPLE_OK;
	}

}

namespace gple
{
	// ---- negative_log_marginal_likelihood / predict_phase (test/gpr.cpp:499-532, 654-706) -------------------------------
	// shared: Gram, Cholesky, inverse factor, b = K^-1 y (labels are NOT rescaled on this path).  Enqueue only; `info` (device, one double's
	// slot) receives the factorisation's info word and a negative one turns b into NaN (colpass_kernel), so that nothing derived from an
	// unfinished factor looks like a number; the callers read the word back with their results and repeat the call with one launch per panel.
	int nlml_solve(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, Scratch& Xt, Scratch& yd, Scratch& T, Scratch& bvec,
		Scratch& info, int* n_out, bool dev)
	{
		hipStream_t st = ctx->stream;
		const int n = static_cast<int>(round_up(N, NPAD));
		*n_out = n;
		Scratch L(ctx), work(ctx), part(ctx), u(ctx), w(ctx);
		GPLE_HIP(ctx, Xt.get(2 * static_cast<size_t>(n)));
		GPLE_HIP(ctx, yd.get(n));
		GPLE_HIP(ctx, T.get(static_cast<size_t>(n) * n));
		GPLE_HIP(ctx, bvec.get(n));
		GPLE_HIP(ctx, L.get(static_cast<size_t>(n) * n));
		GPLE_HIP(ctx, work.get(chol_inverse_work_doubles(n)));
		GPLE_HIP(ctx, part.get(static_cast<size_t>(n / 256) * n));
		GPLE_HIP(ctx, u.get(n));
		GPLE_HIP(ctx, w.get(n));
		GPLE_HIP(ctx, info.get(1));
		GPLE_HIP(ctx, hipMemsetAsync(Xt.p, 0, 2 * static_cast<size_t>(n) * 8, st));
		GPLE_HIP(ctx, hipMemsetAsync(yd.p, 0, static_cast<size_t>(n) * 8, st));
		GPLE_HIP(ctx, hipMemsetAsync(info.p, 0, 8, st));
		// (unlike a fit's, this T is cleared: trmv_lower below walks whole 256-column chunks of a row, the blocks above the diagonal 64-blocks
		// included — a fit gets u = L^-1 y from the label row of its factorisation instead; 30 us at n = 4096)
		GPLE_HIP(ctx, hipMemsetAsync(T.p, 0, static_cast<size_t>(n) * n * 8, st));
		GPLE_HIP(ctx, copy_in(st, Xt.p, X, 2 * N, dev));
		GPLE_HIP(ctx, copy_in(st, yd.p, y, N, dev));
		GPLE_HIP(ctx, launch_nlml_gram(st, Xt.p, static_cast<int>(N), n, x, L.p));
		timer_start(ctx, GPLE_TIMER_FIT); // the factorisation + inverse factor: what the NLML workloads of bench.py price against the fp64 MFMA peak
		GPLE_HIP(ctx, chol_inverse_factor(ctx, st, L.p, n, n, T.p, n, reinterpret_cast<int*>(info.p), work.p));
		timer_stop(ctx, GPLE_TIMER_FIT);
		GPLE_HIP(ctx, launch_trmv_lower(st, T.p, n, n, yd.p, part.p, u.p));
		GPLE_HIP(ctx, launch_colpass(st, T.p, n, n, u.p, bvec.p, w.p, 0, nullptr, reinterpret_cast<int*>(info.p)));
		return GPLE_OK;
	}
	// after the caller's synchronisation: did the factorisation of this attempt give up?  (the word was copied to host_scalars[HS_NLML + 8])
	int nlml_gave_up(gple_ctx* ctx, int attempt, bool* again)
	{
		int info_i;
		std::memcpy(&info_i, ctx->host_scalars + HS_NLML + 8, sizeof(int));
		*again = info_i < 0;
		return *again ? note_give_up(ctx, attempt) : GPLE_OK;
	}
} // namespace gple

extern "C"
{
	// n = 4: (w_d, w_g, a_x, a_p), the NOCROSS build; n = 5: (w_d, w_g, a, c, b), the default build's lower-triangular weight matrix
	static void nlml_params(const double* x, size_t n, double x5[5])
	{
		x5[0] = x[0], x5[1] = x[1], x5[2] = x[2];
		x5[3] = n == 5 ? x[3] : 0.0;
		x5[4] = n == 5 ? x[4] : x[3];
	}
	static int nlml_impl(gple_ctx* ctx, const double* x, size_t n, const double* X, const double* y, size_t N, double* value, double* grad)
	{
		if (!ctx || !x || !X || !y || !value || N == 0) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		double x5[5];
		nlml_params(x, n, x5);
		for (int attempt = 0;; ++attempt)
		{
			CholSchemeScope scheme(attempt == 0 ? ctx->chol_scheme : 0); // second attempt: one launch per panel (a give-up of the one-launch scheme)
			Scratch Xt(ctx), yd(ctx), T(ctx), b(ctx), out(ctx), W(ctx), part(ctx), info(ctx);
			int np = 0;
			GPLE_TRY(nlml_solve(ctx, x5, X, y, N, Xt, yd, T, b, info, &np));
			GPLE_HIP(ctx, out.get(8));
			GPLE_HIP(ctx, launch_nlml_value(st, T.p, np, yd.p, b.p, static_cast<int>(N), out.p));
			if (grad)
			{
				const size_t g = (N + 63) / 64;
				GPLE_HIP(ctx, W.get(static_cast<size_t>(np) * np));
				GPLE_HIP(ctx, part.get(5 * g * g));
				GPLE_HIP(ctx, lauum_full(st, T.p, np, W.p, np, np));
				GPLE_HIP(ctx, launch_nlml_grad(st, Xt.p, static_cast<int>(N), W.p, np, b.p, x5, part.p, out.p + 1));
			}
			GPLE_HIP(ctx, hipMemcpyAsync(ctx->host_scalars + HS_NLML, out.p, 6 * 8, hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipMemcpyAsync(ctx->host_scalars + HS_NLML + 8, info.p, 8, hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			timer_collect(ctx);
			bool again;
			GPLE_TRY(nlml_gave_up(ctx, attempt, &again));
			if (!again) break;
		}
		*value = ctx->host_scalars[HS_NLML];
		if (grad)
		{
			const double* g5 = ctx->host_scalars + HS_NLML + 1; // (w_d, w_g, a, c, b)
			if (n == 5)
				for (int i = 0; i < 5; ++i) grad[i] = g5[i];
			else
				grad[0] = g5[0], grad[1] = g5[1], grad[2] = g5[2], grad[3] = g5[4];
		}
		return GPLE_OK;
	}
	static int nlml_predict_impl(gple_ctx* ctx, const double* x, size_t n, const double* X, const double* y, size_t N, const double* Xs, size_t M,
		unsigned flags, double* mean)
	{
		if (!ctx || !x || !X || !y || N == 0 || (M && (!Xs || !mean))) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (M == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		const bool dev = flags & GPLE_IO_DEVICE; // applies to Xs / mean only; the training set is small and host-side
		double x5[5];
		nlml_params(x, n, x5);
		for (int attempt = 0;; ++attempt)
		{
			CholSchemeScope scheme(attempt == 0 ? ctx->chol_scheme : 0);
			Scratch Xt(ctx), yd(ctx), T(ctx), b(ctx), part(ctx), info(ctx);
			Staged xs(ctx, dev), o(ctx, dev);
			int np = 0;
			GPLE_TRY(nlml_solve(ctx, x5, X, y, N, Xt, yd, T, b, info, &np));
			GPLE_HIP(ctx, xs.in(Xs, 2 * M));
			GPLE_HIP(ctx, o.out(mean, M));
			GPLE_HIP(ctx, part.get(static_cast<size_t>(nlml_predict_ksplit(static_cast<int>(M), static_cast<int>(N))) * M));
			timer_start(ctx, GPLE_TIMER_PREDICT);
			GPLE_HIP(ctx, launch_nlml_predict(st, xs.p, static_cast<int>(M), Xt.p, static_cast<int>(N), b.p, x5, part.p, o.p));
			timer_stop(ctx, GPLE_TIMER_PREDICT);
			GPLE_HIP(ctx, o.back());
			GPLE_HIP(ctx, hipMemcpyAsync(ctx->host_scalars + HS_NLML + 8, info.p, 8, hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			timer_collect(ctx);
			bool again;
			GPLE_TRY(nlml_gave_up(ctx, attempt, &again));
			if (!again) break;
		}
		return GPLE_OK;
	}

	int gple_nlml(gple_ctx* ctx, const double x[4], const double* X, const double* y, size_t N, double* value, double* grad)
	{
		return nlml_impl(ctx, x, 4, X, y, N, value, grad);
	}
	int gple_nlml_predict(gple_ctx* ctx, const double x[4], const double* X, const double* y, size_t N, const double* Xs, size_t M, unsigned flags,
		double* mean)
	{
		return nlml_predict_impl(ctx, x, 4, X, y, N, Xs, M, flags, mean);
	}
	int gple_nlml_cross(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, double* value, double* grad)
	{
		return nlml_impl(ctx, x, 5, X, y, N, value, grad);
	}
	int gple_nlml_cross_predict(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, const double* Xs, size_t M,
		unsigned flags, double* mean)
	{
		return nlml_predict_impl(ctx, x, 5, X, y, N, Xs, M, flags, mean);
	}
}
