// gple_capi.h — what the C-ABI files (gple_capi*.hip) share: the context with its buffer pool, the fit handles, the staging of
// caller arrays and the predict / fit functions that more than one of them calls.  Internal: not part of include/gple.h.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <vector>

#include "gple_kernels.h"

using namespace gple;

// ---- context with a grow-only buffer pool ----------------------------------------------------------------
struct gple_ctx: gple::Ctx
{
	struct PoolEntry
	{
		void* p;
		size_t bytes;
		bool used;
	};
	std::vector<PoolEntry> pool;
	std::mutex pool_mu;
	std::mutex call_mu; // serialises fit / predict calls that share the pooled scratch
	// Lifetime: the creator holds one reference, every live fit / objective one more.  gple_ctx_destroy() closes the context
	// (entry points that take it return GPLE_ERR_STATE from then on) and drops the creator's reference; the device buffers,
	// the stream and the struct itself go when the last handle created from it is released.
	std::atomic<int> refs{1};
	std::atomic<bool> closed{false};
	// The user potentials of gple_pes_define: slot k holds the model GPLE_PES_USER + k.  The table is device memory of its own (not pooled),
	// freed by gple_pes_undefine after draining the stream, or with the context.  pes_mu guards the slots; a call copies its descriptor
	// out under it (pes_resolve) once to validate its arguments and again after it has taken the call lock, and enqueues with that copy:
	// gple_pes_undefine holds the call lock and drains the stream before it frees, so the table outlives every kernel enqueued on it.
	struct PesSlot
	{
		double* table = nullptr; // nullptr: free
		int num_pes = 0, n = 0;
		double x_first = 0.0, dx = 1.0;
	};
	static constexpr int PES_SLOTS = 16;
	PesSlot pes[PES_SLOTS];
	std::mutex pes_mu;

	double* acquire(size_t bytes, hipError_t* err)
	{
		std::lock_guard<std::mutex> lk(pool_mu);
		*err = hipSuccess;
		if (bytes == 0) bytes = 8;
		PoolEntry* best = nullptr;
		for (PoolEntry& e : pool)
			if (!e.used && e.bytes >= bytes && e.bytes <= 2 * bytes + 4096 && (!best || e.bytes < best->bytes)) best = &e;
		if (best)
		{
			best->used = true;
			return static_cast<double*>(best->p);
		}
		void* p = nullptr;
		*err = hipMalloc(&p, bytes);
		if (*err != hipSuccess) return nullptr;
		pool.push_back({p, bytes, true});
		return static_cast<double*>(p);
	}
	void give_back(void* p)
	{
		if (!p) return;
		std::lock_guard<std::mutex> lk(pool_mu);
		for (PoolEntry& e : pool)
			if (e.p == p) e.used = false;
	}
};

inline void ctx_retain(gple_ctx* c) { c->refs.fetch_add(1); }
// drops one reference; the last one tears the context down
inline void ctx_drop(gple_ctx* ctx)
{
	if (ctx->refs.fetch_sub(1) != 1) return;
	(void)hipSetDevice(ctx->device);
	(void)hipStreamSynchronize(ctx->stream);
	for (auto& e : ctx->pool) (void)hipFree(e.p);
	for (auto& slot : ctx->pes)
		if (slot.table) (void)hipFree(slot.table);
	if (ctx->host_scalars) (void)hipHostFree(ctx->host_scalars);
	if (ctx->prune_stats) (void)hipFree(ctx->prune_stats);
	if (ctx->format_table) (void)hipFree(ctx->format_table);
	if (ctx->dag_flags) (void)hipFree(ctx->dag_flags);
	timer_collect(ctx);
	for (hipEvent_t e : ctx->ev_free) (void)hipEventDestroy(e);
	if (ctx->side_stream)
	{
		(void)hipStreamSynchronize(ctx->side_stream);
		(void)hipStreamDestroy(ctx->side_stream);
		for (hipEvent_t ev : ctx->side_forks) (void)hipEventDestroy(ev);
		if (ctx->side_join) (void)hipEventDestroy(ctx->side_join);
	}
	if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
	delete ctx;
}
#define GPLE_OPEN(ctx)                                  \
	do                                                  \
	{                                                   \
		if ((ctx)->closed.load()) return GPLE_ERR_STATE; \
	} while (0)
// holds the context's call lock to the end of the enclosing scope and makes its device current (calls that share the stream and the pool)
#define GPLE_CALL(ctx)                                             \
	std::lock_guard<std::mutex> gple_call_lk_((ctx)->call_mu); \
	GPLE_HIP((ctx), hipSetDevice((ctx)->device))

// The potential of a num_pes-level call: a built-in id by the rule the N-level entry points share (models 0-2, TSAC = 3 at three levels only),
// or a user id defined on this context with the same num_pes.  false: the call returns GPLE_ERR_BAD_ARG
inline bool pes_resolve(gple_ctx* ctx, int num_pes, int model, gple::PesModel* out)
{
	if (num_pes != 2 && num_pes != 3) return false;
	if (model >= 0 && model <= (num_pes == 3 ? 3 : 2))
	{
		*out = gple::PesModel(model);
		return true;
	}
	if (model < GPLE_PES_USER || model >= GPLE_PES_USER + gple_ctx::PES_SLOTS) return false;
	std::lock_guard<std::mutex> lk(ctx->pes_mu);
	const gple_ctx::PesSlot& slot = ctx->pes[model - GPLE_PES_USER];
	if (!slot.table || slot.num_pes != num_pes) return false;
	out->id = model, out->n = slot.n, out->table = slot.table, out->x_first = slot.x_first, out->dx = slot.dx;
	return true;
}

namespace gple
{
	// per-fit device scalar block (doubles) and offsets into the context's pinned host block
	constexpr int SDEV_N = 512;        // [0] s, [1..15] base sums, [16..28] real derivative sums, [31] info, [32..39] complex error derivative,
	                                   // [64..108] complex purity quadratic forms (5 kernels x 9), [128..287] aux dots (5 x 8 x 4)
	constexpr int HS_PRED_ERR = 512, HS_PRED_DERIV = 520, HS_NLML = 540;
	constexpr int SDEV_INFO = 31; // the factorisation's info word (an int in the double's slot; the finish kernels read it: gple_kernels.hip, fit_gave_up)
	// a handful of test points with host pointers (the reference's one-point predicts): inputs and outputs go through the pinned
	// block itself (device-visible), not through four hipMemcpyAsync of pageable memory
	constexpr int HS_FEW_XS = 600, HS_FEW_LAB = 640, HS_FEW_MEAN = 680, HS_FEW_VAR = 720, HS_FEW_CUT = 740;
	constexpr size_t FEW_HOST_POINTS = 16;

	// pooled buffer with scope lifetime
	struct Scratch
	{
		gple_ctx* ctx;
		double* p = nullptr;
		explicit Scratch(gple_ctx* c): ctx(c) {}
		Scratch(const Scratch&) = delete;
		~Scratch() { ctx->give_back(p); }
		hipError_t get(size_t doubles)
		{
			hipError_t e;
			p = ctx->acquire(doubles * sizeof(double), &e);
			return e;
		}
	};

	inline double nan_() { return std::numeric_limits<double>::quiet_NaN(); }

	// copies `n` doubles host->device or device->device depending on the IO flag
	inline hipError_t copy_in(hipStream_t s, double* dst, const double* src, size_t n, bool dev)
	{
		if (n == 0) return hipSuccess;
		return hipMemcpyAsync(dst, src, n * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
	}
	inline hipError_t copy_out(hipStream_t s, double* dst, const double* src, size_t n, bool dev)
	{
		if (n == 0 || dst == nullptr) return hipSuccess;
		return hipMemcpyAsync(dst, src, n * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s);
	}

	// A caller's array as the kernels see it, by the call's GPLE_IO_DEVICE bit: a device array is used in place; a host input is copied into
	// pooled memory (in), a host output gets pooled memory (out) that back() copies to the caller.  A null array stays null.
	struct Staged
	{
		Scratch buf;
		const bool dev;
		double* p = nullptr;    // what the kernels read or write
		double* host = nullptr; // a host output: back() copies p here
		size_t n = 0;
		Staged(gple_ctx* c, bool device): buf(c), dev(device) {}
		hipError_t in(const double* src, size_t count)
		{
			p = const_cast<double*>(src);
			if (dev || !src) return hipSuccess;
			hipError_t e = buf.get(count);
			p = buf.p;
			return e == hipSuccess ? copy_in(buf.ctx->stream, p, src, count, false) : e;
		}
		hipError_t out(double* dst, size_t count)
		{
			p = dst;
			if (dev || !dst) return hipSuccess;
			host = dst, n = count;
			hipError_t e = buf.get(count);
			p = buf.p;
			return e;
		}
		hipError_t inout(double* a, size_t count)
		{
			if (!dev && a) host = a, n = count;
			return in(a, count);
		}
		hipError_t back() { return host ? copy_out(buf.ctx->stream, host, p, n, false) : hipSuccess; }
	};
} // namespace gple

// ---- fit handles ---------------------------------------------------------------------------------------------
struct FitCommon
{
	std::atomic<int> refs{1};
	gple_ctx* ctx = nullptr;
	int N = 0, Np = 0, n_total = 0;
	unsigned flags = 0;
	bool is_complex = false;
	double* Xt = nullptr;   // 2*Np
	double* ys = nullptr;   // n_total
	double* T = nullptr;    // n_total^2
	double* v = nullptr;    // n_total
	double* w = nullptr;    // n_total (diag of K^-1)
	double* wx = nullptr;   // Np (complex only)
	double* W = nullptr;    // n_total^2, lazy
	double* dv = nullptr;   // derivatives of v over the parameters, [nparam][n_total] (GPLE_CALC_DERIVATIVE fits only)
	double sf = 1.0;        // real kernel: magnitude (needed unsquared by the derivative formulas)
	double s0 = 1.0;        // complex kernel: global magnitude
	DSpecSet dspec[6];      // complex kernel: derivative blocks of the parameters 1..6 (zero-initialised = inactive)
	double* sdev = nullptr; // [0] rescale factor, [1..] raw sums, [31] info (as int)
	double s_host = 0.0;
	bool sc_ready = false; // host scalars computed (deferred when the caller passed no scalars struct)
	// The one-launch factorisation may give up waiting (info = -1, gple_chol.hip): the device then turns everything derived from T into NaN, and
	// the first host synchronisation on this fit (validate_fit: the scalar getters, every *_fit_get, a predict that drains the stream) repeats
	// the factorisation with a launch per panel.  Calls that consumed the fit before that — enqueued, never synchronised — have produced NaN
	// (settle_fit reports them):
	mutable std::atomic<bool> validated{false}; // the host has seen info >= 0 (or has recovered)
	mutable std::atomic<bool> recovered{false}; // recover_fit repeated the factorisation
	mutable std::atomic<int> stale_uses{0};     // predicts enqueued on the not yet validated fit
	unsigned deriv_mask = 0xFFu; // which parameters' N^3 products a derivative fit forms (bit ip; gple_objective_eval_part splits them over ranks)
	SEParamSet ps{};
	double self = 0.0; // k(x*, x*)
	FitCommon() { std::memset(dspec, 0, sizeof(dspec)); }
	std::mutex lazy_mu;
	// one-point predicts from several host threads on this fit (the reference calls its DistributionFunction from TBB workers,
	// evolve.cpp:392-420, mc.cpp:214-246): requests that arrive while a predict is in flight are served together by the next one
	struct PointRequest
	{
		const double* x;
		double *mean, *var, *cut;
		int status;
		bool done;
	};
	mutable std::mutex point_mu;
	mutable std::condition_variable point_cv;
	mutable std::vector<PointRequest*> point_pending;
	mutable bool point_leader = false;

	~FitCommon()
	{
		if (!ctx) return;
		for (double* p : {Xt, ys, T, v, w, wx, W, dv, sdev}) ctx->give_back(p);
		ctx_drop(ctx); // the reference fit_common() took
	}
};
struct gple_real_fit: FitCommon
{
	double theta[4];
	gple_real_fit_scalars sc;
};
struct gple_complex_fit: FitCommon
{
	double theta[8];
	gple_complex_fit_scalars sc;
};

namespace gple
{
	// internal flag of predict_common (never part of the ABI's flag space): enqueue everything, including the D2H copies of
	// the error scalars, but leave the synchronisation and the scalar read-out to the caller
	constexpr unsigned PREDICT_NO_SYNC = 0x10000u;
	void predict_scalars_from_host(gple_ctx* ctx, bool has_labels, bool want_deriv, bool cplx, gple_predict_scalars* scalars);
	int predict_common(gple_ctx* ctx, const FitCommon* f, const double* Xs, size_t M, unsigned flags, const double* labels, double* prediction,
		double* variance, double* cutoff_prediction, gple_predict_scalars* scalars);
	// a draining call on f that returned `status` has written its own outputs: GPLE_OK, or GPLE_ERR_TIMEOUT for earlier work on the (now good)
	// fit — not the GPLE_ERR_TIMEOUT of a repetition that gave up too, which leaves the fit unvalidated
	inline bool own_outputs_written(int status, const FitCommon* f) { return status == GPLE_OK || (status == GPLE_ERR_TIMEOUT && f->validated.load()); }
	// deriv_mask: which parameters' N^3 products a derivative fit forms (bit ip) — all of them, except for gple_objective_eval_part
	int real_fit_create_masked(gple_ctx* ctx, const double theta[4], const double* X, const double* y, int y_is_complex, size_t N, unsigned flags,
		unsigned deriv_mask, gple_real_fit_scalars* scalars, gple_real_fit** out);
	int complex_fit_create_masked(gple_ctx* ctx, const double theta[8], const double* X, const double* y, size_t N, unsigned flags, unsigned deriv_mask,
		gple_complex_fit_scalars* scalars, gple_complex_fit** out);
	// the real / complex pairs of include/gple.h in one implementation each (F: gple_real_fit or gple_complex_fit)
	int fit_predict(gple_ctx* ctx, const FitCommon* fit, const double* Xs, size_t M, unsigned flags, const double* labels, double* prediction,
		double* variance, double* cutoff_prediction, gple_predict_scalars* scalars);
	template <typename F>
	int fit_get_scalars(F* fit, decltype(F::sc)* out);
	template <typename F>
	int fit_release(F* fit);
	// give-up bookkeeping of the one-launch factorisation (fits and the NLML path): a give-up noticed on `attempt` (0: the first factorisation,
	// 1: its repetition with a launch per panel) is counted; GPLE_OK: repeat with a launch per panel, GPLE_ERR_TIMEOUT: the repetition gave up too
	int note_give_up(gple_ctx* ctx, int attempt);
	// the NLML path's shared front (gple_capi_objective.hip): Gram of x = (w_d, w_g, a, c, b), Cholesky, inverse factor and bvec = K^-1 y, enqueued;
	// X / y are device arrays with dev.  nlml_gave_up: after the caller's synchronisation, with the info word copied to host_scalars[HS_NLML + 8]
	int nlml_solve(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, Scratch& Xt, Scratch& yd, Scratch& T, Scratch& bvec,
		Scratch& info, int* n_out, bool dev = false);
	int nlml_gave_up(gple_ctx* ctx, int attempt, bool* again);
	// gple_opt.hip: the library's Nelder-Mead with each step's candidates evaluated as one batch (points in, values out)
	using PointBatchEval = std::function<void(const std::vector<std::vector<double>>&, std::vector<double>&)>;
	int neldermead_speculative(const PointBatchEval& eval, unsigned n, const double* lb, const double* ub, const gple_opt_options* options, double* x,
		double* fmin, int* n_eval);
} // namespace gple
