// gple_capi_hop.hip — C-ABI entry points of include/gple.h: the trajectory ensembles of gple_hop.hip.  An entry point keeps what
// is its own, its argument checks, its timer and its launch; what every one of them does around the launch is HopStaged.
#include <cmath>

#include "gple_capi.h"
#include "gple_debug.h"

namespace
{
	// the surface / status array of a hop call as the kernels see it (Staged, for ints): a device array in place, a host array through pooled memory
	struct StagedInts
	{
		Scratch buf;
		const bool dev;
		int* p = nullptr;
		int* host = nullptr; // back() copies p here
		size_t n = 0;
		StagedInts(gple_ctx* c, bool device): buf(c), dev(device) {}
		// read: the kernels read the caller's values; written: the caller receives the kernels'
		hipError_t stage(const int* a, size_t count, bool read, bool written)
		{
			p = const_cast<int*>(a);
			if (dev) return hipSuccess;
			hipError_t e = buf.get((count + 1) / 2);
			if (e != hipSuccess) return e;
			p = reinterpret_cast<int*>(buf.p);
			if (written) host = const_cast<int*>(a), n = count;
			return read ? hipMemcpyAsync(p, a, count * sizeof(int), hipMemcpyHostToDevice, buf.ctx->stream) : hipSuccess;
		}
		hipError_t back() { return host ? hipMemcpyAsync(host, p, n * sizeof(int), hipMemcpyDeviceToHost, buf.ctx->stream) : hipSuccess; }
	};

	// The ensemble of a hop call as the kernels see it, between GPLE_CALL and the return: stage() resolves the model again (under the call lock,
	// which gple_pes_undefine takes: the table outlives the enqueue), puts a host table of the grouped calls (their packets or time steps) into
	// pooled device memory, stages the arrays by the call's GPLE_IO_DEVICE bit and builds e; finish() copies back what the kernels wrote and
	// waits where the caller's memory is the host's
	struct HopStaged
	{
		enum Mode
		{
			WRITTEN, // the samples
			UPDATED, // the steps: read and written
			READ     // the sums and the density
		};
		gple_ctx* const ctx;
		const bool dev;
		PesModel pes;
		HopEnsemble e{};
		Staged xs, ps, bs;
		StagedInts su, ss, hs;
		Scratch table;
		HopStaged(gple_ctx* c, unsigned flags): ctx(c), dev(flags & GPLE_IO_DEVICE), xs(c, dev), ps(c, dev), bs(c, dev), su(c, dev), ss(c, dev), hs(c, dev), table(c) {}
		static hipError_t put(Staged& s, const double* a, size_t count, Mode mode)
		{
			double* const w = const_cast<double*>(a);
			return mode == WRITTEN ? s.out(w, count) : mode == UPDATED ? s.inout(w, count) : s.in(a, count);
		}
		// surface: null for the methods without an active surface; hops (UPDATED): null or n x 2 counts; rows: null or the host table of count doubles.
		// The table is the caller's pageable memory whatever the flags say: the copy is waited for, so that the caller may free it when the call returns
		int stage(Mode mode, int num_pes, int model, size_t n, size_t offset, unsigned long long seed, const double* x, const double* p, const double* b,
			const int* surface, const int* status, int* hops = nullptr, const double* rows = nullptr, size_t count = 0)
		{
			GPLE_TRY(begin(num_pes, model, rows, count));
			return arrays(mode, num_pes, n, offset, seed, x, p, b, surface, status, hops);
		}
		// the two halves of stage(), for the sums, which take their work and output memory between them as they always have
		int begin(int num_pes, int model, const double* rows = nullptr, size_t count = 0)
		{
			if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG;
			if (rows)
			{
				GPLE_HIP(ctx, table.get(count));
				GPLE_HIP(ctx, hipMemcpyAsync(table.p, rows, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
				GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
			}
			return GPLE_OK;
		}
		int arrays(Mode mode, int num_pes, size_t n, size_t offset, unsigned long long seed, const double* x, const double* p, const double* b, const int* surface,
			const int* status, int* hops = nullptr)
		{
			const bool read = mode != WRITTEN, written = mode != READ;
			GPLE_HIP(ctx, put(xs, x, n, mode));
			GPLE_HIP(ctx, put(ps, p, n, mode));
			GPLE_HIP(ctx, put(bs, b, 2 * n * num_pes, mode));
			if (surface) GPLE_HIP(ctx, su.stage(surface, n, read, written));
			GPLE_HIP(ctx, ss.stage(status, n, read, written));
			if (hops) GPLE_HIP(ctx, hs.stage(hops, 2 * n, read, written));
			e = HopEnsemble{num_pes, static_cast<long>(n), offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
			return GPLE_OK;
		}
		// host_out: the call has written host memory of its own (the sums of the grouped calls are the host's whatever the flags say)
		int finish(bool host_out = false)
		{
			for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
			for (StagedInts* o : {&su, &ss, &hs}) GPLE_HIP(ctx, o->back());
			if (!dev || host_out) GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
			return GPLE_OK;
		}
	};

	// a launch inside the span of its timer, which is closed on the error path too: no span stays open
	template <typename Launch>
	int hop_timed(gple_ctx* ctx, int timer, Launch&& launch)
	{
		timer_start(ctx, timer);
		const hipError_t launched = launch();
		timer_stop(ctx, timer);
		GPLE_HIP(ctx, launched);
		return GPLE_OK;
	}
	// The sums of one method over the n = n_groups n_per_group trajectories of the caller's arrays (surface: null without an active surface), in the
	// order the entry points have always had: the model, the first stage's partial rows in pooled memory, out (the grouped calls: always the
	// host's), then the ensemble
	template <typename Launch>
	int hop_sums(HopStaged& st, int num_pes, int model, const double* x, const double* p, const double* b, const int* surface, const int* status, int width,
		size_t n_groups, size_t n_per_group, bool grouped, double* out, Launch&& launch)
	{
		gple_ctx* const ctx = st.ctx;
		GPLE_TRY(st.begin(num_pes, model));
		Staged o(ctx, st.dev && !grouped);
		Scratch work(ctx);
		GPLE_HIP(ctx, work.get(hop_observe_work_doubles(width, static_cast<long>(n_groups), static_cast<long>(n_per_group))));
		GPLE_HIP(ctx, o.out(out, n_groups * width));
		GPLE_TRY(st.arrays(HopStaged::READ, num_pes, n_groups * n_per_group, 0, 0, x, p, b, surface, status));
		GPLE_HIP(ctx, launch(work.p, o.p));
		GPLE_HIP(ctx, o.back());
		return st.finish(grouped);
	}

	bool hop_size_ok(gple_ctx* ctx, int num_pes, int model, size_t n, size_t offset, PesModel* pes)
	{
		constexpr size_t LIMIT = size_t(1) << 32; // the trajectory index is one word of the counter
		return pes_resolve(ctx, num_pes, model, pes) && n >= 1 && n <= LIMIT && offset <= LIMIT - n;
	}
	// n = n_groups n_per_group without overflow, within the index space together with the offset
	bool hop_groups_ok(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t offset, PesModel* pes, size_t* n)
	{
		if (n_groups == 0 || n_per_group == 0 || n_groups > GPLE_HOP_MAX_GROUPS || n_per_group > (size_t(1) << 32) / n_groups) return false;
		*n = n_groups * n_per_group;
		return hop_size_ok(ctx, num_pes, model, *n, offset, pes);
	}
	bool hop_positive(double v) { return std::isfinite(v) && v > 0.0; }
	// the rows (x0, p0, sigma_x, sigma_p) of a grouped sample: finite, and no sigma negative (a sigma of 0 is the centre exactly)
	bool hop_packets_ok(const double* packets, size_t n_groups)
	{
		for (size_t g = 0; g < n_groups; ++g)
		{
			const double* row = packets + 4 * g;
			if (!std::isfinite(row[0]) || !std::isfinite(row[1]) || !std::isfinite(row[2]) || !std::isfinite(row[3]) || row[2] < 0.0 || row[3] < 0.0) return false;
		}
		return true;
	}
	// the time steps of a grouped step
	bool hop_dt_ok(const double* dt, size_t n_groups)
	{
		for (size_t g = 0; g < n_groups; ++g)
			if (!hop_positive(dt[g])) return false;
		return true;
	}
	// decoherence is a GPLE_HOP_DC_*, and in mode EDC edc_c is finite and not negative (it is read in that mode only)
	bool hop_decoherence_ok(int decoherence, double edc_c)
	{
		if (decoherence < GPLE_HOP_DC_NONE || decoherence > GPLE_HOP_DC_COLLAPSE_ATTEMPT) return false;
		return decoherence != GPLE_HOP_DC_EDC || (std::isfinite(edc_c) && edc_c >= 0.0);
	}
	// n_x n_p <= GPLE_HOP_MAX_CELLS, without overflow
	bool hop_cells_ok(size_t n_x, size_t n_p) { return n_x >= 1 && n_p >= 1 && n_x <= GPLE_HOP_MAX_CELLS && n_p <= GPLE_HOP_MAX_CELLS / n_x; }
	// what the steps without a seed share: the checks of gple_hop_evolve that apply without a surface, a seed and an offset
	bool hop_mf_evolve_ok(double mass, size_t n_steps, double x_left, double x_right, unsigned flags, const double* x, const double* p, const double* b,
		const int* status)
	{
		return hop_positive(mass) && std::isfinite(x_left) && std::isfinite(x_right) && x_left < x_right && n_steps <= (1ul << 40) && !(flags & GPLE_HOP_REVERSE) &&
			x && p && b && status;
	}
	// gamma of the SQC step, where no window is named: finite and not negative
	bool hop_sqc_gamma_ok(double gamma) { return std::isfinite(gamma) && gamma >= 0.0; }
	// window is a GPLE_HOP_WINDOW_* and gamma fits it: the square windows are disjoint for 0 < gamma < 1/2 only
	bool hop_sqc_window_ok(int window, double gamma)
	{
		if (window != GPLE_HOP_WINDOW_SQUARE && window != GPLE_HOP_WINDOW_TRIANGLE) return false;
		return hop_sqc_gamma_ok(gamma) && (window != GPLE_HOP_WINDOW_SQUARE || (gamma > 0.0 && gamma < 0.5));
	}
	// what the MASH calls share beyond the checks of their models: two levels, no GPLE_HOP_REVERSE (MASH always reflects), five arrays
	bool hop_mash_ok(int num_pes, unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status)
	{
		return num_pes == 2 && !(flags & GPLE_HOP_REVERSE) && x && p && b && surface && status;
	}
	// gple_hop_bin and gple_hop_bin_mf around their launch (surface: null for the call without one; n_max: the call's own bound on n): the
	// checks, the model, a host acc through pooled memory (8 bytes an integer, as a double), the clear or the copy, the timer around the kernel alone
	using HopBinLaunch = hipError_t (*)(hipStream_t, const HopEnsemble&, PesModel, const HopGrid&, bool, long long*);
	int hop_bin_call(gple_ctx* ctx, int num_pes, int model, size_t n, size_t n_max, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
		unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status, long long* acc, int timer, HopBinLaunch launch)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || n > n_max || !hop_cells_ok(n_x, n_p) || !hop_positive(dx) || !hop_positive(dp) ||
			!std::isfinite(x_first) || !std::isfinite(p_first) || !x || !p || !b || !status || !acc)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE, keep = flags & GPLE_HOP_ACCUMULATE;
		const size_t words = static_cast<size_t>(hop_bin_planes(num_pes)) * n_x * n_p + 2;
		GPLE_CALL(ctx);
		hipStream_t stream = ctx->stream;
		HopStaged st(ctx, flags);
		GPLE_TRY(st.begin(num_pes, model));
		Scratch sums(ctx);
		long long* a = acc;
		if (!dev)
		{
			GPLE_HIP(ctx, sums.get(words));
			a = reinterpret_cast<long long*>(sums.p);
		}
		GPLE_TRY(st.arrays(HopStaged::READ, num_pes, n, 0, 0, x, p, b, surface, status));
		if (!keep) GPLE_HIP(ctx, hipMemsetAsync(a, 0, words * sizeof(long long), stream));
		else if (!dev) GPLE_HIP(ctx, hipMemcpyAsync(a, acc, words * sizeof(long long), hipMemcpyHostToDevice, stream));
		const HopGrid g{x_first, dx, p_first, dp, static_cast<long>(n_x), static_cast<long>(n_p)};
		GPLE_TRY(hop_timed(ctx, timer, [&] { return launch(stream, st.e, st.pes, g, (flags & GPLE_HOP_BIN_ALL) != 0, a); }));
		if (!dev) GPLE_HIP(ctx, hipMemcpyAsync(acc, a, words * sizeof(long long), hipMemcpyDeviceToHost, stream));
		return st.finish();
	}
	// gple_hop_outgoing, _mf and _sqc around their launch, as hop_bin_call (surface: null for the two forms without one; ok: what the form's
	// observe call checks beyond the shared checks: its n_max, window and gamma, the flags it refuses)
	template <typename Launch>
	int hop_outgoing_call(gple_ctx* ctx, int num_pes, int model, size_t n, bool ok, double mass, int axis, double first, double step, size_t n_bins, unsigned flags,
		const double* x, const double* p, const double* b, const int* surface, const int* status, long long* acc, Launch&& launch)
	{
		PesModel pes;
		if (!ctx || !ok || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || n > (size_t(1) << 31) || !hop_positive(mass) ||
			(axis != GPLE_HOP_AXIS_MOMENTUM && axis != GPLE_HOP_AXIS_ENERGY) || n_bins == 0 || n_bins > GPLE_HOP_MAX_CELLS / 6 || !hop_positive(step) ||
			!std::isfinite(first) || !x || !p || !b || !status || !acc)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE, keep = flags & GPLE_HOP_ACCUMULATE;
		const size_t words = hop_outgoing_words(num_pes, n_bins);
		GPLE_CALL(ctx);
		hipStream_t stream = ctx->stream;
		HopStaged st(ctx, flags);
		GPLE_TRY(st.begin(num_pes, model));
		Scratch sums(ctx);
		long long* a = acc;
		if (!dev)
		{
			GPLE_HIP(ctx, sums.get(words));
			a = reinterpret_cast<long long*>(sums.p);
		}
		GPLE_TRY(st.arrays(HopStaged::READ, num_pes, n, 0, 0, x, p, b, surface, status));
		if (!keep) GPLE_HIP(ctx, hipMemsetAsync(a, 0, words * sizeof(long long), stream));
		else if (!dev) GPLE_HIP(ctx, hipMemcpyAsync(a, acc, words * sizeof(long long), hipMemcpyHostToDevice, stream));
		const HopAxis g{first, step, static_cast<long>(n_bins), axis == GPLE_HOP_AXIS_ENERGY ? 1 : 0};
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_OUTGOING, [&] { return launch(stream, st.e, st.pes, g, a); }));
		if (!dev) GPLE_HIP(ctx, hipMemcpyAsync(acc, a, words * sizeof(long long), hipMemcpyDeviceToHost, stream));
		return st.finish();
	}
	// gple_hop_density and gple_hop_density_mf around their launch
	using HopDensityLaunch = hipError_t (*)(hipStream_t, int, long, double, const long long*, double*);
	int hop_density_call(gple_ctx* ctx, int num_pes, size_t n_x, size_t n_p, double dx, double dp, size_t n_norm, unsigned flags, const long long* acc, double* rho,
		HopDensityLaunch launch)
	{
		const double w = static_cast<double>(n_norm) * dx * dp; // left to right
		if (!ctx || (num_pes != 2 && num_pes != 3) || !hop_cells_ok(n_x, n_p) || !hop_positive(dx) || !hop_positive(dp) || n_norm == 0 || !hop_positive(w) ||
			!acc || !rho)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t cells = n_x * n_p, words = static_cast<size_t>(hop_bin_planes(num_pes)) * cells + 2;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Staged r(ctx, dev);
		Scratch sums(ctx);
		const long long* a = acc;
		GPLE_HIP(ctx, r.out(rho, 2 * static_cast<size_t>(num_pes) * num_pes * cells));
		if (!dev)
		{
			GPLE_HIP(ctx, sums.get(words));
			GPLE_HIP(ctx, hipMemcpyAsync(sums.p, acc, words * sizeof(long long), hipMemcpyHostToDevice, st));
			a = reinterpret_cast<const long long*>(sums.p);
		}
		GPLE_HIP(ctx, launch(st, num_pes, static_cast<long>(cells), w, a, r.p));
		GPLE_HIP(ctx, r.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}
	// gple_hop_smooth and gple_hop_smooth_mf around their kernels, as hop_bin_call (surface: null for the call without one): the checks, the
	// model, rho by the call's GPLE_IO_DEVICE bit, the terms, the partial planes and the two tallies in pooled memory, the timer around the three
	// kernels alone.  tally is the host's whatever the flags say
	int hop_smooth_call(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p, double h_x,
		double h_p, size_t n_norm, unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status, double* rho,
		long long* tally, bool mean_field)
	{
		PesModel pes;
		const double scale = 1.0 / (static_cast<double>(n_norm) * 6.283185307179586 * h_x * h_p); // the denominator left to right
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || n > (size_t(1) << 31) || !hop_cells_ok(n_x, n_p) || !hop_positive(dx) || !hop_positive(dp) ||
			!std::isfinite(x_first) || !std::isfinite(p_first) || !hop_positive(h_x) || !hop_positive(h_p) || n_norm == 0 || !hop_positive(scale) ||
			(flags & (GPLE_HOP_ACCUMULATE | GPLE_HOP_REVERSE)) || !x || !p || !b || !status || !rho)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		hipStream_t stream = ctx->stream;
		HopStaged st(ctx, flags);
		GPLE_TRY(st.begin(num_pes, model));
		Staged r(ctx, dev);
		Scratch work(ctx), counts(ctx);
		GPLE_HIP(ctx, work.get(hop_smooth_work_doubles(num_pes, static_cast<long>(n), static_cast<long>(n_x), static_cast<long>(n_p))));
		GPLE_HIP(ctx, counts.get(2));
		GPLE_HIP(ctx, r.out(rho, 2 * static_cast<size_t>(num_pes) * num_pes * n_x * n_p));
		GPLE_TRY(st.arrays(HopStaged::READ, num_pes, n, 0, 0, x, p, b, surface, status));
		unsigned long long* const c = reinterpret_cast<unsigned long long*>(counts.p);
		GPLE_HIP(ctx, hipMemsetAsync(c, 0, 2 * sizeof(unsigned long long), stream));
		const HopGrid g{x_first, dx, p_first, dp, static_cast<long>(n_x), static_cast<long>(n_p)};
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_SMOOTH, [&] {
			const hipError_t terms = launch_hop_smooth_terms(stream, st.e, st.pes, mean_field, (flags & GPLE_HOP_BIN_ALL) != 0, work.p, c);
			return terms != hipSuccess ? terms : launch_hop_smooth(stream, num_pes, static_cast<long>(n), g, h_x, h_p, scale, work.p, r.p);
		}));
		GPLE_HIP(ctx, r.back());
		if (tally) GPLE_HIP(ctx, hipMemcpyAsync(tally, c, 2 * sizeof(long long), hipMemcpyDeviceToHost, stream));
		return st.finish(tally != nullptr);
	}
} // namespace

extern "C"
{
	/* ---- fewest-switches surface hopping ------------------------------------------------------------------------------------------------------ */
	int gple_hop_sample(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
		double sigma_x, double sigma_p, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, trajectory_offset, &pes) || !hop_positive(sigma_x) || !hop_positive(sigma_p) || surface0 < 0 ||
			surface0 >= num_pes || !x || !p || !b || !surface || !status)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::WRITTEN, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status));
		GPLE_HIP(ctx, launch_hop_sample(ctx->stream, st.e, st.pes, x0, p0, sigma_x, sigma_p, surface0));
		return st.finish();
	}

	int gple_hop_evolve_dc(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double mass, double dt,
		size_t first_step, size_t n_steps, double x_left, double x_right, int decoherence, double edc_c, unsigned flags, double* x, double* p, double* b,
		int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, trajectory_offset, &pes) || !hop_positive(mass) || !hop_positive(dt) || !std::isfinite(x_left) ||
			!std::isfinite(x_right) || !(x_left < x_right) || n_steps > (1ul << 40) || !x || !p || !b || !surface || !status ||
			!hop_decoherence_ok(decoherence, edc_c))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP, [&] {
			return launch_hop_evolve(ctx->stream, st.e, st.pes, mass, dt, first_step, static_cast<long>(n_steps), x_left, x_right, (flags & GPLE_HOP_REVERSE) != 0,
				decoherence, edc_c);
		}));
		return st.finish();
	}
	int gple_hop_evolve(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double mass, double dt,
		size_t first_step, size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		return gple_hop_evolve_dc(ctx, num_pes, model, n, trajectory_offset, seed, mass, dt, first_step, n_steps, x_left, x_right, GPLE_HOP_DC_NONE, 0.0, flags, x, p,
			b, surface, status);
	}

	int gple_hop_observe(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, unsigned flags, const double* x, const double* p, const double* b,
		const int* surface, const int* status, double* out)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(mass) || !x || !p || !b || !surface || !status || !out) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		return hop_sums(st, num_pes, model, x, p, b, surface, status, hop_observe_width(num_pes), 1, n, false, out,
			[&](double* work, double* sums) { return launch_hop_observe(ctx->stream, st.e, st.pes, mass, work, sums); });
	}

	int gple_hop_bin(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
		unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status, long long* acc)
	{
		if (!surface) return GPLE_ERR_BAD_ARG;
		return hop_bin_call(ctx, num_pes, model, n, size_t(1) << 32, x_first, dx, n_x, p_first, dp, n_p, flags, x, p, b, surface, status, acc, GPLE_TIMER_HOP_BIN,
			launch_hop_bin);
	}

	int gple_hop_density(gple_ctx* ctx, int num_pes, size_t n_x, size_t n_p, double dx, double dp, size_t n_norm, unsigned flags, const long long* acc,
		double* rho)
	{
		return hop_density_call(ctx, num_pes, n_x, n_p, dx, dp, n_norm, flags, acc, rho, launch_hop_density);
	}

	/* ---- the density from the amplitudes ("The ensemble in phase space, from the amplitudes") ------------------------------- */
	int gple_hop_bin_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
		unsigned flags, const double* x, const double* p, const double* b, const int* status, long long* acc)
	{
		// n <= 2^31: a weight term is at most 2^32 to rounding, and one call must not overflow the signed sum of a cell
		return hop_bin_call(ctx, num_pes, model, n, size_t(1) << 31, x_first, dx, n_x, p_first, dp, n_p, flags, x, p, b, nullptr, status, acc, GPLE_TIMER_HOP_BIN_MF,
			launch_hop_bin_mf);
	}

	int gple_hop_density_mf(gple_ctx* ctx, int num_pes, size_t n_x, size_t n_p, double dx, double dp, size_t n_norm, unsigned flags, const long long* acc,
		double* rho)
	{
		return hop_density_call(ctx, num_pes, n_x, n_p, dx, dp, n_norm, flags, acc, rho, launch_hop_density_mf);
	}

	/* ---- what left the box, per channel ("What left the box") ----------------------------------------------------------------- */
	int gple_hop_outgoing(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int axis, double first, double step, size_t n_bins, unsigned flags,
		const double* x, const double* p, const double* b, const int* surface, const int* status, long long* acc)
	{
		return hop_outgoing_call(ctx, num_pes, model, n, surface != nullptr, mass, axis, first, step, n_bins, flags, x, p, b, surface, status, acc,
			[&](hipStream_t s, const HopEnsemble& e, const PesModel& pes, const HopAxis& g, long long* a) { return launch_hop_outgoing(s, e, pes, mass, g, a); });
	}

	int gple_hop_outgoing_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int axis, double first, double step, size_t n_bins, unsigned flags,
		const double* x, const double* p, const double* b, const int* status, long long* acc)
	{
		return hop_outgoing_call(ctx, num_pes, model, n, true, mass, axis, first, step, n_bins, flags, x, p, b, nullptr, status, acc,
			[&](hipStream_t s, const HopEnsemble& e, const PesModel& pes, const HopAxis& g, long long* a) { return launch_hop_outgoing_mf(s, e, pes, mass, g, a); });
	}

	int gple_hop_outgoing_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int window, double gamma, int axis, double first, double step,
		size_t n_bins, unsigned flags, const double* x, const double* p, const double* b, const int* status, long long* acc)
	{
		return hop_outgoing_call(ctx, num_pes, model, n, hop_sqc_window_ok(window, gamma) && !(flags & GPLE_HOP_REVERSE), mass, axis, first, step, n_bins, flags, x,
			p, b, nullptr, status, acc, [&](hipStream_t s, const HopEnsemble& e, const PesModel& pes, const HopAxis& g, long long* a) {
				return launch_hop_outgoing_sqc(s, e, pes, mass, window, gamma, g, a);
			});
	}

	/* ---- the smoothed density ("The ensemble in phase space, smoothed") -------------------------------------------------------- */
	int gple_hop_smooth(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p, double h_x,
		double h_p, size_t n_norm, unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status, double* rho,
		long long* tally)
	{
		if (!surface) return GPLE_ERR_BAD_ARG;
		return hop_smooth_call(ctx, num_pes, model, n, x_first, dx, n_x, p_first, dp, n_p, h_x, h_p, n_norm, flags, x, p, b, surface, status, rho, tally, false);
	}

	int gple_hop_smooth_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
		double h_x, double h_p, size_t n_norm, unsigned flags, const double* x, const double* p, const double* b, const int* status, double* rho, long long* tally)
	{
		return hop_smooth_call(ctx, num_pes, model, n, x_first, dx, n_x, p_first, dp, n_p, h_x, h_p, n_norm, flags, x, p, b, nullptr, status, rho, tally, true);
	}

	int gple_debug_hop_smooth_split(int num_pes, size_t n, size_t n_x, size_t n_p, size_t* chunk, size_t* n_chunks)
	{
		if ((num_pes != 2 && num_pes != 3) || n == 0 || n > (size_t(1) << 31) || !hop_cells_ok(n_x, n_p) || !chunk || !n_chunks) return GPLE_ERR_BAD_ARG;
		const HopSmoothPlan plan = hop_smooth_plan(num_pes, static_cast<long>(n), static_cast<long>(n_x), static_cast<long>(n_p));
		*chunk = static_cast<size_t>(plan.chunk), *n_chunks = static_cast<size_t>(plan.n_chunks);
		return GPLE_OK;
	}

	/* ---- grouped ensembles ("A curve in one launch") ------------------------------------------------------------------------ */
	int gple_hop_sample_groups(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset, unsigned long long seed,
		const double* packets, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, trajectory_offset, &pes, &n) || !packets || surface0 < 0 || surface0 >= num_pes ||
			!x || !p || !b || !surface || !status)
			return GPLE_ERR_BAD_ARG;
		if (!hop_packets_ok(packets, n_groups)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::WRITTEN, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status, nullptr, packets, 4 * n_groups));
		GPLE_HIP(ctx, launch_hop_sample_groups(ctx->stream, st.e, st.pes, static_cast<long>(n_per_group), st.table.p, surface0));
		return st.finish();
	}

	int gple_hop_evolve_groups_dc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset,
		unsigned long long seed, double mass, const double* dt, size_t first_step, size_t n_steps, double x_left, double x_right, int decoherence,
		double edc_c, unsigned flags, double* x, double* p, double* b, int* surface, int* status, int* hops)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, trajectory_offset, &pes, &n) || !hop_positive(mass) || !dt || !std::isfinite(x_left) ||
			!std::isfinite(x_right) || !(x_left < x_right) || n_steps > (1ul << 40) || !x || !p || !b || !surface || !status ||
			!hop_decoherence_ok(decoherence, edc_c))
			return GPLE_ERR_BAD_ARG;
		if (!hop_dt_ok(dt, n_groups)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status, hops, dt, n_groups));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_GROUPS, [&] {
			return launch_hop_evolve_groups(ctx->stream, st.e, st.pes, static_cast<long>(n_per_group), mass, st.table.p, first_step, static_cast<long>(n_steps), x_left,
				x_right, (flags & GPLE_HOP_REVERSE) != 0, st.hs.p, decoherence, edc_c);
		}));
		return st.finish();
	}
	int gple_hop_evolve_groups(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset, unsigned long long seed,
		double mass, const double* dt, size_t first_step, size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b,
		int* surface, int* status, int* hops)
	{
		return gple_hop_evolve_groups_dc(ctx, num_pes, model, n_groups, n_per_group, trajectory_offset, seed, mass, dt, first_step, n_steps, x_left, x_right,
			GPLE_HOP_DC_NONE, 0.0, flags, x, p, b, surface, status, hops);
	}

	int gple_hop_observe_groups(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, unsigned flags, const double* x,
		const double* p, const double* b, const int* surface, const int* status, double* out)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !hop_positive(mass) || !x || !p || !b || !surface || !status || !out)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		return hop_sums(st, num_pes, model, x, p, b, surface, status, hop_observe_width(num_pes), n_groups, n_per_group, true, out, [&](double* work, double* sums) {
			return launch_hop_observe_groups(ctx->stream, st.e, st.pes, static_cast<long>(n_groups), static_cast<long>(n_per_group), mass, work, sums);
		});
	}

	/* ---- Ehrenfest (mean-field) trajectories ("Mean-field (Ehrenfest) trajectories") ------------------------------------------- */
	int gple_hop_evolve_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, double dt, size_t n_steps, double x_left, double x_right, unsigned flags,
		double* x, double* p, double* b, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(dt) || !hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, 0, 0, x, p, b, nullptr, status));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_MF,
			[&] { return launch_hop_evolve_mf(ctx->stream, st.e, st.pes, mass, dt, static_cast<long>(n_steps), x_left, x_right); }));
		return st.finish();
	}

	int gple_hop_evolve_groups_mf(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt, size_t n_steps,
		double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !dt ||
			!hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status))
			return GPLE_ERR_BAD_ARG;
		if (!hop_dt_ok(dt, n_groups)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, 0, 0, x, p, b, nullptr, status, nullptr, dt, n_groups));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_MF, [&] {
			return launch_hop_evolve_groups_mf(ctx->stream, st.e, st.pes, static_cast<long>(n_per_group), mass, st.table.p, static_cast<long>(n_steps), x_left, x_right);
		}));
		return st.finish();
	}

	int gple_hop_observe_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, unsigned flags, const double* x, const double* p, const double* b,
		const int* status, double* out)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(mass) || !x || !p || !b || !status || !out) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		return hop_sums(st, num_pes, model, x, p, b, nullptr, status, hop_observe_mf_width(num_pes), 1, n, false, out,
			[&](double* work, double* sums) { return launch_hop_observe_mf(ctx->stream, st.e, st.pes, mass, work, sums); });
	}

	int gple_hop_observe_groups_mf(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, unsigned flags, const double* x,
		const double* p, const double* b, const int* status, double* out)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !hop_positive(mass) || !x || !p || !b || !status || !out)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		return hop_sums(st, num_pes, model, x, p, b, nullptr, status, hop_observe_mf_width(num_pes), n_groups, n_per_group, true, out, [&](double* work, double* sums) {
			return launch_hop_observe_groups_mf(ctx->stream, st.e, st.pes, static_cast<long>(n_groups), static_cast<long>(n_per_group), mass, work, sums);
		});
	}

	/* ---- symmetrical quasi-classical trajectories ("Symmetrical quasi-classical trajectories") -------------------------------- */
	int gple_hop_sample_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
		double sigma_x, double sigma_p, int surface0, int window, double gamma, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, trajectory_offset, &pes) || !hop_positive(sigma_x) || !hop_positive(sigma_p) || surface0 < 0 ||
			surface0 >= num_pes || !hop_sqc_window_ok(window, gamma) || (flags & GPLE_HOP_REVERSE) || !x || !p || !b || !surface || !status)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::WRITTEN, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status));
		GPLE_HIP(ctx, launch_hop_sample_sqc(ctx->stream, st.e, st.pes, x0, p0, sigma_x, sigma_p, surface0, window, gamma));
		return st.finish();
	}

	int gple_hop_sample_groups_sqc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset,
		unsigned long long seed, const double* packets, int surface0, int window, double gamma, unsigned flags, double* x, double* p, double* b,
		int* surface, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, trajectory_offset, &pes, &n) || !packets || surface0 < 0 || surface0 >= num_pes ||
			!hop_sqc_window_ok(window, gamma) || (flags & GPLE_HOP_REVERSE) || !x || !p || !b || !surface || !status)
			return GPLE_ERR_BAD_ARG;
		if (!hop_packets_ok(packets, n_groups)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::WRITTEN, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status, nullptr, packets, 4 * n_groups));
		GPLE_HIP(ctx, launch_hop_sample_groups_sqc(ctx->stream, st.e, st.pes, static_cast<long>(n_per_group), st.table.p, surface0, window, gamma));
		return st.finish();
	}

	int gple_hop_evolve_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, double dt, size_t n_steps, double x_left, double x_right, double gamma,
		unsigned flags, double* x, double* p, double* b, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(dt) || !hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status) ||
			!hop_sqc_gamma_ok(gamma))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, 0, 0, x, p, b, nullptr, status));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_SQC,
			[&] { return launch_hop_evolve_sqc(ctx->stream, st.e, st.pes, mass, dt, static_cast<long>(n_steps), x_left, x_right, gamma); }));
		return st.finish();
	}

	int gple_hop_evolve_groups_sqc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt, size_t n_steps,
		double x_left, double x_right, double gamma, unsigned flags, double* x, double* p, double* b, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !dt ||
			!hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status) || !hop_sqc_gamma_ok(gamma))
			return GPLE_ERR_BAD_ARG;
		if (!hop_dt_ok(dt, n_groups)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, 0, 0, x, p, b, nullptr, status, nullptr, dt, n_groups));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_SQC, [&] {
			return launch_hop_evolve_groups_sqc(ctx->stream, st.e, st.pes, static_cast<long>(n_per_group), mass, st.table.p, static_cast<long>(n_steps), x_left, x_right,
				gamma);
		}));
		return st.finish();
	}

	int gple_hop_observe_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int window, double gamma, unsigned flags, const double* x,
		const double* p, const double* b, const int* status, double* out)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(mass) || !hop_sqc_window_ok(window, gamma) || (flags & GPLE_HOP_REVERSE) || !x || !p ||
			!b || !status || !out)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		return hop_sums(st, num_pes, model, x, p, b, nullptr, status, hop_observe_sqc_width(num_pes), 1, n, false, out,
			[&](double* work, double* sums) { return launch_hop_observe_sqc(ctx->stream, st.e, st.pes, mass, window, gamma, work, sums); });
	}

	int gple_hop_observe_groups_sqc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, int window, double gamma,
		unsigned flags, const double* x, const double* p, const double* b, const int* status, double* out)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !hop_positive(mass) || !hop_sqc_window_ok(window, gamma) ||
			(flags & GPLE_HOP_REVERSE) || !x || !p || !b || !status || !out)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		return hop_sums(st, num_pes, model, x, p, b, nullptr, status, hop_observe_sqc_width(num_pes), n_groups, n_per_group, true, out, [&](double* work, double* sums) {
			return launch_hop_observe_groups_sqc(ctx->stream, st.e, st.pes, static_cast<long>(n_groups), static_cast<long>(n_per_group), mass, window, gamma, work,
				sums);
		});
	}

	/* ---- MASH trajectories ("MASH trajectories") -------------------------------------------------------------------------------- */
	int gple_hop_sample_mash(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
		double sigma_x, double sigma_p, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_mash_ok(num_pes, flags, x, p, b, surface, status) || !hop_size_ok(ctx, num_pes, model, n, trajectory_offset, &pes) || !hop_positive(sigma_x) ||
			!hop_positive(sigma_p) || surface0 < 0 || surface0 >= num_pes)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::WRITTEN, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status));
		GPLE_HIP(ctx, launch_hop_sample_mash(ctx->stream, st.e, st.pes, x0, p0, sigma_x, sigma_p, surface0));
		return st.finish();
	}

	int gple_hop_sample_groups_mash(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset,
		unsigned long long seed, const double* packets, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_mash_ok(num_pes, flags, x, p, b, surface, status) ||
			!hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, trajectory_offset, &pes, &n) || !packets || surface0 < 0 || surface0 >= num_pes)
			return GPLE_ERR_BAD_ARG;
		if (!hop_packets_ok(packets, n_groups)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::WRITTEN, num_pes, model, n, trajectory_offset, seed, x, p, b, surface, status, nullptr, packets, 4 * n_groups));
		GPLE_HIP(ctx, launch_hop_sample_groups_mash(ctx->stream, st.e, st.pes, static_cast<long>(n_per_group), st.table.p, surface0));
		return st.finish();
	}

	int gple_hop_evolve_mash(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, double dt, size_t n_steps, double x_left, double x_right,
		unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_mash_ok(num_pes, flags, x, p, b, surface, status) || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(dt) ||
			!hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, 0, 0, x, p, b, surface, status));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_MASH,
			[&] { return launch_hop_evolve_mash(ctx->stream, st.e, st.pes, mass, dt, static_cast<long>(n_steps), x_left, x_right); }));
		return st.finish();
	}

	int gple_hop_evolve_groups_mash(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt,
		size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* surface, int* status, int* hops)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_mash_ok(num_pes, flags, x, p, b, surface, status) || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !dt ||
			!hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status))
			return GPLE_ERR_BAD_ARG;
		if (!hop_dt_ok(dt, n_groups)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		HopStaged st(ctx, flags);
		GPLE_TRY(st.stage(HopStaged::UPDATED, num_pes, model, n, 0, 0, x, p, b, surface, status, hops, dt, n_groups));
		GPLE_TRY(hop_timed(ctx, GPLE_TIMER_HOP_MASH, [&] {
			return launch_hop_evolve_groups_mash(ctx->stream, st.e, st.pes, static_cast<long>(n_per_group), mass, st.table.p, static_cast<long>(n_steps), x_left, x_right,
				st.hs.p);
		}));
		return st.finish();
	}
}
