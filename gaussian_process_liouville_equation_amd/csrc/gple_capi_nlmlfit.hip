// gple_capi_nlmlfit.hip — C-ABI entry points of include/gple.h: the batched NLML evaluation (gple_nlml_batch) and the hyper-parameter search of
// several planes in lock-step on it (gple_nlml_fit_planes); DESIGN.md §13.
#include <cfloat>
#include <climits>
#include <cmath>
#include <thread>

#include "gple_capi.h"

namespace
{
	// x = (w_d, w_g, a_x, a_p) or (w_d, w_g, a, c, b) -> the five parameters of the kernels (nlml_params of gple_capi_objective.hip)
	void params5(const double* x, bool cross, double x5[5])
	{
		x5[0] = x[0], x5[1] = x[1], x5[2] = x[2];
		x5[3] = cross ? x[3] : 0.0;
		x5[4] = cross ? x[4] : x[3];
	}
	// One launch over `probs` (device X / y / weights; the work offsets are filled in here), enqueued on the context's stream.  The caller holds
	// the call lock and keeps `probs` alive until the stream has drained.
	int batch_enqueue(gple_ctx* ctx, std::vector<NlmlBatchProblem>& probs, Scratch& dprobs, Scratch& work, double* values, double* grads, int grad_width,
		int* info)
	{
		size_t total = 0;
		for (NlmlBatchProblem& p : probs) p.work = static_cast<long>(total), total += nlml_batch_work_doubles(p.N);
		const size_t bytes = probs.size() * sizeof(NlmlBatchProblem);
		GPLE_HIP(ctx, dprobs.get((bytes + 7) / 8));
		GPLE_HIP(ctx, work.get(total));
		GPLE_HIP(ctx, hipMemcpyAsync(dprobs.p, probs.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
		GPLE_HIP(ctx, launch_nlml_batch(ctx->stream, reinterpret_cast<const NlmlBatchProblem*>(dprobs.p), static_cast<int>(probs.size()), work.p, values, grads,
			grad_width, info));
		return GPLE_OK;
	}

	// ---- the rendezvous of gple_nlml_fit_planes (the pattern of predict_point_combined: requests that meet ride on one launch) ----------------
	struct EvalRequest
	{
		int plane;
		const double* points; // count x 5
		size_t count;
		bool want_grad, want_weights;
		double* values; // count
		double* grads;  // count x 5, with want_grad
		int status = GPLE_OK;
		bool done = false;
	};
	struct Rendezvous
	{
		std::mutex mu;
		std::condition_variable cv;
		std::vector<EvalRequest*> pending;
		int running = 0; // searches that have not ended
		// a search thread: post and wait.  Never touches the GPU
		int evaluate(EvalRequest& r)
		{
			std::unique_lock<std::mutex> lk(mu);
			pending.push_back(&r);
			cv.notify_all();
			cv.wait(lk, [&] { return r.done; });
			return r.status;
		}
		void leave()
		{
			std::lock_guard<std::mutex> lk(mu);
			--running;
			cv.notify_all();
		}
	};
	struct PlaneOnDevice
	{
		const double *X, *y;
		double* weights;
		size_t N;
	};
	// the owner's side: every posted request in one launch
	int serve(gple_ctx* ctx, const std::vector<EvalRequest*>& batch, const std::vector<PlaneOnDevice>& planes)
	{
		size_t B = 0;
		for (const EvalRequest* r : batch) B += r->count;
		std::vector<NlmlBatchProblem> probs;
		probs.reserve(B);
		for (const EvalRequest* r : batch)
			for (size_t k = 0; k < r->count; ++k)
			{
				const PlaneOnDevice& pl = planes[r->plane];
				NlmlBatchProblem p{};
				std::memcpy(p.x, r->points + 5 * k, sizeof(p.x));
				p.X = pl.X, p.y = pl.y, p.N = static_cast<int>(pl.N);
				p.weights = r->want_weights ? pl.weights : nullptr;
				p.flags = r->want_grad ? NLML_BATCH_GRAD : 0u;
				probs.push_back(p);
			}
		Scratch dprobs(ctx), work(ctx), out(ctx);
		GPLE_HIP(ctx, out.get(6 * B)); // values | gradients
		GPLE_TRY(batch_enqueue(ctx, probs, dprobs, work, out.p, out.p + B, 5, nullptr));
		std::vector<double> host(6 * B);
		GPLE_HIP(ctx, hipMemcpyAsync(host.data(), out.p, 6 * B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
		GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		size_t q = 0;
		for (EvalRequest* r : batch)
			for (size_t k = 0; k < r->count; ++k, ++q)
			{
				r->values[k] = host[q];
				if (r->want_grad) std::memcpy(r->grads + 5 * k, host.data() + B + 5 * q, 5 * sizeof(double));
			}
		return GPLE_OK;
	}

	struct PlaneSearch
	{
		Rendezvous* rv;
		int plane;
		bool cross;
		int evals = 0, status = GPLE_OK;
		// reconstruct.optimize's `value`: a non-finite value is DBL_MAX, a non-finite gradient component 0, the two kernel-weight gradients doubled
		void evaluate(const double* const* xs, size_t count, bool want_grad, bool want_weights, double* values, double* grads)
		{
			const size_t n = cross ? 5 : 4;
			std::vector<double> pts(5 * count), g5(want_grad ? 5 * count : 0);
			for (size_t k = 0; k < count; ++k) params5(xs[k], cross, pts.data() + 5 * k);
			EvalRequest r{plane, pts.data(), count, want_grad, want_weights, values, g5.data()};
			const int st = rv->evaluate(r);
			evals += static_cast<int>(count);
			if (st != GPLE_OK) status = st;
			for (size_t k = 0; k < count; ++k)
			{
				if (st != GPLE_OK || !std::isfinite(values[k])) values[k] = DBL_MAX;
				if (!want_grad) continue;
				const double* g = g5.data() + 5 * k;
				const double gx[5] = {g[0], g[1], g[2], cross ? g[3] : g[4], g[4]};
				for (size_t i = 0; i < n; ++i) grads[n * k + i] = (st == GPLE_OK && std::isfinite(gx[i])) ? gx[i] * (i < 2 ? 2.0 : 1.0) : 0.0;
			}
		}
		static double objective(unsigned, const double* x, double* grad, void* data)
		{
			double v;
			static_cast<PlaneSearch*>(data)->evaluate(&x, 1, grad != nullptr, false, &v, grad);
			return v;
		}
		// gpr.cpp:535-643
		void run(const gple_nlml_fit_plane& pl, const gple_opt_options* options, bool want_weights, double* x_out, double* f_out)
		{
			const unsigned n = cross ? 5 : 4;
			double x[5] = {0, 0, 0, 0, 0}, f = 0.0;
			std::copy(pl.start, pl.start + n, x);
			const PointBatchEval batch = [&](const std::vector<std::vector<double>>& pts, std::vector<double>& vals) {
				std::vector<const double*> xs;
				for (const auto& p : pts) xs.push_back(p.data());
				evaluate(xs.data(), pts.size(), false, false, vals.data(), nullptr);
			};
			int st = neldermead_speculative(batch, n, pl.lb, pl.ub, options, x, &f, nullptr);
			if (st == GPLE_OK) st = gple_minimize_auglag_eq(&PlaneSearch::objective, this, nullptr, nullptr, 0, n, pl.lb, pl.ub, options, x, &f, nullptr);
			if (st != GPLE_OK) status = st;
			const double* at = x;
			evaluate(&at, 1, false, want_weights, f_out, nullptr); // "Best Combination": the value once more at the result (gpr.cpp:633)
			std::copy(x, x + 5, x_out);
			rv->leave();
		}
	};
} // namespace

extern "C"
{
	int gple_nlml_batch(gple_ctx* ctx, const gple_nlml_problem* problems, size_t B, int cross, unsigned flags, double* values, double* grads,
		double* const* weights, int* info)
	{
		if (!ctx || !problems || !values || B == 0 || B > static_cast<size_t>(INT_MAX)) return GPLE_ERR_BAD_ARG;
		size_t points = 0, weighted = 0;
		for (size_t b = 0; b < B; ++b)
		{
			if (!problems[b].X || !problems[b].y || problems[b].N == 0 || problems[b].N > GPLE_NLML_BATCH_MAX_N) return GPLE_ERR_BAD_ARG;
			points += problems[b].N;
			if (weights && weights[b]) weighted += problems[b].N;
		}
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		const bool dev = flags & GPLE_IO_DEVICE;
		const int width = cross ? 5 : 4;
		// host arrays travel as one block each way: X and y of every problem in, the requested weights out
		std::vector<double> pack, wpack(dev ? 0 : weighted);
		if (!dev)
		{
			pack.reserve(3 * points);
			for (size_t b = 0; b < B; ++b)
			{
				pack.insert(pack.end(), problems[b].X, problems[b].X + 2 * problems[b].N);
				pack.insert(pack.end(), problems[b].y, problems[b].y + problems[b].N);
			}
		}
		Staged in(ctx, dev), wout(ctx, dev), vout(ctx, dev), gout(ctx, dev);
		Scratch iout(ctx), dprobs(ctx), work(ctx);
		if (!dev) GPLE_HIP(ctx, in.in(pack.data(), pack.size()));
		if (!dev && weighted) GPLE_HIP(ctx, wout.out(wpack.data(), weighted));
		GPLE_HIP(ctx, vout.out(values, B));
		GPLE_HIP(ctx, gout.out(grads, width * B));
		int* dinfo = info;
		if (info && !dev)
		{
			GPLE_HIP(ctx, iout.get((B + 1) / 2));
			dinfo = reinterpret_cast<int*>(iout.p);
		}
		std::vector<NlmlBatchProblem> probs(B);
		size_t at = 0, wat = 0;
		for (size_t b = 0; b < B; ++b)
		{
			NlmlBatchProblem& p = probs[b];
			const size_t N = problems[b].N;
			params5(problems[b].x, cross != 0, p.x);
			p.X = dev ? problems[b].X : in.p + at, p.y = dev ? problems[b].y : in.p + at + 2 * N;
			at += 3 * N;
			p.weights = nullptr;
			if (weights && weights[b]) p.weights = dev ? weights[b] : wout.p + wat, wat += N;
			p.N = static_cast<int>(N);
			p.flags = grads ? NLML_BATCH_GRAD : 0u;
		}
		GPLE_TRY(batch_enqueue(ctx, probs, dprobs, work, vout.p, gout.p, width, dinfo));
		GPLE_HIP(ctx, vout.back());
		GPLE_HIP(ctx, gout.back());
		GPLE_HIP(ctx, wout.back());
		if (info && !dev) GPLE_HIP(ctx, hipMemcpyAsync(info, dinfo, B * sizeof(int), hipMemcpyDeviceToHost, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st)); // `probs` and the packed host blocks end with this call
		for (size_t b = 0, w = 0; b < B && !dev; ++b)
			if (weights && weights[b]) std::copy(wpack.begin() + w, wpack.begin() + w + problems[b].N, weights[b]), w += problems[b].N;
		return GPLE_OK;
	}

	int gple_nlml_fit_planes(gple_ctx* ctx, const gple_nlml_fit_plane* planes, size_t P, int cross, const gple_opt_options* options, double* x_out,
		double* f_out, int* n_eval, double* const* weights)
	{
		if (!ctx || !planes || !x_out || !f_out || !n_eval || P == 0 || P > GPLE_NLML_FIT_MAX_PLANES) return GPLE_ERR_BAD_ARG;
		size_t points = 0;
		for (size_t q = 0; q < P; ++q)
		{
			if (!planes[q].X || !planes[q].y || planes[q].N == 0 || planes[q].N > GPLE_NLML_BATCH_MAX_N) return GPLE_ERR_BAD_ARG;
			points += planes[q].N;
		}
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx); // this thread owns the context for the whole fit: it alone launches
		hipStream_t st = ctx->stream;
		// the planes' data, resident for the whole search: X | y | weights of every plane in one block
		std::vector<double> pack;
		pack.reserve(3 * points);
		for (size_t q = 0; q < P; ++q)
		{
			pack.insert(pack.end(), planes[q].X, planes[q].X + 2 * planes[q].N);
			pack.insert(pack.end(), planes[q].y, planes[q].y + planes[q].N);
		}
		Scratch data(ctx);
		GPLE_HIP(ctx, data.get(4 * points));
		GPLE_HIP(ctx, hipMemcpyAsync(data.p, pack.data(), pack.size() * sizeof(double), hipMemcpyHostToDevice, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		std::vector<PlaneOnDevice> resident(P);
		for (size_t q = 0, at = 0, wat = 3 * points; q < P; at += 3 * planes[q].N, wat += planes[q].N, ++q)
			resident[q] = {data.p + at, data.p + at + 2 * planes[q].N, data.p + wat, planes[q].N};

		Rendezvous rv;
		rv.running = static_cast<int>(P);
		std::vector<PlaneSearch> searches(P);
		std::vector<std::thread> threads;
		for (size_t q = 0; q < P; ++q)
		{
			searches[q].rv = &rv, searches[q].plane = static_cast<int>(q), searches[q].cross = cross != 0;
			threads.emplace_back(&PlaneSearch::run, &searches[q], std::cref(planes[q]), options, weights && weights[q], x_out + 5 * q, f_out + q);
		}
		int status = GPLE_OK;
		{
			std::unique_lock<std::mutex> lk(rv.mu);
			for (;;)
			{
				rv.cv.wait(lk, [&] { return static_cast<int>(rv.pending.size()) == rv.running; }); // every search still running has posted
				if (rv.running == 0) break;
				std::vector<EvalRequest*> batch;
				batch.swap(rv.pending);
				lk.unlock();
				const int s = serve(ctx, batch, resident);
				lk.lock();
				if (s != GPLE_OK) status = s;
				for (EvalRequest* r : batch) r->status = s, r->done = true;
				rv.cv.notify_all();
			}
		}
		for (std::thread& t : threads) t.join();
		for (size_t q = 0; q < P; ++q)
		{
			n_eval[q] = searches[q].evals;
			if (status == GPLE_OK && searches[q].status != GPLE_OK) status = searches[q].status;
			if (status == GPLE_OK && weights && weights[q]) GPLE_HIP(ctx, hipMemcpyAsync(weights[q], resident[q].weights, planes[q].N * sizeof(double), hipMemcpyDeviceToHost, st));
		}
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		return status;
	}
}
