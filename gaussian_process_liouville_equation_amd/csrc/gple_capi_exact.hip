// gple_capi_exact.hip — C-ABI entry points of include/gple.h: the exact DVR and MQCLE solvers and the Wigner transform.
#include <algorithm>
#include <cmath>

#include "gple_capi.h"

extern "C"
{
	/* ---- exact DVR dynamics (gple_dvr.hip; schrodinger_equation/general.cpp of the reference) ---------------------------------------------- */
	static bool dvr_grid_ok(size_t n_grids, double dx) { return n_grids >= 2 && n_grids <= (1u << 16) && dx > 0.0 && std::isfinite(dx); }

	int gple_dvr_hamiltonian(gple_ctx* ctx, int num_pes, int model, int boundary, double x_first, double dx, size_t n_grids, double mass, unsigned flags,
		double* H, double* energies, double* basis)
	{
		PesModel pes;
		if (!ctx || !pes_resolve(ctx, num_pes, model, &pes) || (boundary != GPLE_DVR_REFLECTIVE && boundary != GPLE_DVR_PERIODIC) || !dvr_grid_ok(n_grids, dx) ||
			!std::isfinite(x_first) || !(mass > 0.0))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t dim = static_cast<size_t>(num_pes) * n_grids;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged h(ctx, dev), e(ctx, dev), b(ctx, dev);
		Scratch sw(ctx);
		GPLE_HIP(ctx, h.out(H, dim * dim));
		GPLE_HIP(ctx, e.out(energies, n_grids * num_pes));
		GPLE_HIP(ctx, b.out(basis, n_grids * num_pes * num_pes));
		if (h.p) GPLE_HIP(ctx, launch_dvr_hamiltonian(st, num_pes, pes, boundary, x_first, dx, n, mass, h.p));
		if (e.p || b.p)
		{
			GPLE_HIP(ctx, sw.get(dvr_states_work_doubles(num_pes, n)));
			GPLE_HIP(ctx, launch_dvr_states(st, num_pes, pes, x_first, dx, n, e.p, b.p, sw.p));
		}
		for (Staged* o : {&h, &e, &b}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_dvr_propagate(gple_ctx* ctx, int num_pes, size_t n_grids, const double* eigvec, const double* eigval, const double* psi0_or_c0, const double* times,
		size_t T, const double* basis, unsigned flags, double* psi)
	{
		if (!ctx || (num_pes != 2 && num_pes != 3) || !dvr_grid_ok(n_grids, 1.0) || T > 4096 || (T && (!eigvec || !eigval || !psi0_or_c0 || !times || !psi)))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (T == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t dim = static_cast<size_t>(num_pes) * n_grids, ld = round_up(dim, 64);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Scratch work(ctx);
		Staged e(ctx, dev), v(ctx, dev), t(ctx, dev), b(ctx, dev), o(ctx, dev);
		GPLE_HIP(ctx, work.get(dvr_propagate_work_doubles(num_pes, n, static_cast<int>(T))));
		// C into the zero-padded ld x ld block
		GPLE_HIP(ctx, hipMemsetAsync(work.p, 0, ld * ld * sizeof(double), st));
		GPLE_HIP(ctx, hipMemcpy2DAsync(work.p, ld * sizeof(double), eigvec, dim * sizeof(double), dim * sizeof(double), dim,
			dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
		GPLE_HIP(ctx, e.in(eigval, dim));
		GPLE_HIP(ctx, v.in(psi0_or_c0, 2 * dim));
		GPLE_HIP(ctx, t.in(times, T));
		GPLE_HIP(ctx, b.in(basis, n_grids * num_pes * num_pes));
		GPLE_HIP(ctx, o.out(psi, 2 * dim * T));
		GPLE_HIP(ctx, launch_dvr_propagate(st, num_pes, n, e.p, v.p, t.p, static_cast<int>(T), b.p, (flags & GPLE_DVR_PSI0) != 0, work.p, o.p));
		GPLE_HIP(ctx, o.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_wigner(gple_ctx* ctx, int num_pes, int boundary, size_t n_grids, double x_first, double dx, const double* p, size_t n_p, const double* psi,
		size_t T, const double* energies, double mass, unsigned flags, double* phase, double* averages)
	{
		if (!ctx || (num_pes != 2 && num_pes != 3) || (boundary != GPLE_DVR_REFLECTIVE && boundary != GPLE_DVR_PERIODIC) || !dvr_grid_ok(n_grids, dx) ||
			!std::isfinite(x_first) || n_p < 2 || n_p > (1u << 16) || T * num_pes * (num_pes + 1) / 2 > 65535 || (T && (!p || !psi)) ||
			(averages && (!energies || !(mass > 0.0))))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (T == 0 || (!phase && !averages)) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids), np = static_cast<int>(n_p);
		const size_t dim = static_cast<size_t>(num_pes) * n_grids, pdoubles = 2 * T * num_pes * num_pes * n_grids * n_p;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Scratch table(ctx), avw(ctx), only_avg(ctx);
		Staged pp(ctx, dev), ps(ctx, dev), en(ctx, dev), av(ctx, dev), P(ctx, dev);
		GPLE_HIP(ctx, table.get(wigner_table_doubles(boundary, n, np)));
		GPLE_HIP(ctx, pp.in(p, n_p));
		GPLE_HIP(ctx, ps.in(psi, 2 * dim * T));
		GPLE_HIP(ctx, en.in(averages ? energies : nullptr, n_grids * num_pes));
		GPLE_HIP(ctx, av.out(averages, 3 * T));
		GPLE_HIP(ctx, P.out(phase, pdoubles));
		if (!phase) GPLE_HIP(ctx, only_avg.get(pdoubles)); // the averages alone: the distribution is formed all the same
		double* const Pd = phase ? P.p : only_avg.p;
		GPLE_HIP(ctx, launch_wigner_table(st, boundary, n, pp.p, np, dx, table.p));
		timer_start(ctx, GPLE_TIMER_WIGNER);
		GPLE_HIP(ctx, launch_wigner(st, num_pes, boundary, n, dx, table.p, np, ps.p, static_cast<int>(T), Pd));
		timer_stop(ctx, GPLE_TIMER_WIGNER);
		if (averages)
		{
			GPLE_HIP(ctx, avw.get(wigner_avg_work_doubles(num_pes, static_cast<int>(T))));
			GPLE_HIP(ctx, launch_wigner_averages(st, num_pes, n, x_first, dx, pp.p, np, en.p, mass, Pd, static_cast<int>(T), avw.p, av.p));
		}
		GPLE_HIP(ctx, P.back());
		GPLE_HIP(ctx, av.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- the absorbing boundary (gple_dvr_power.hip): the absorber, the propagator of n_steps RK4 steps as a matrix power, its application ---- */
	// what gple_dvr_propagator, gple_dvr_flux and gple_dvr_spectrum (n_steps = 2^levels) ask of a system and a step count before the power is formed
	static bool dvr_power_args_ok(int num_pes, size_t n_grids, double dt, size_t n_steps)
	{
		return (num_pes == 2 || num_pes == 3) && dvr_grid_ok(n_grids, 1.0) && std::isfinite(dt) && n_steps >= 1 && n_steps <= (1ul << 30) &&
			round_up(static_cast<size_t>(num_pes) * n_grids, 64) <= static_cast<size_t>(DVR_POWER_MAX_LD);
	}
	int gple_dvr_absorber(gple_ctx* ctx, double x_first, double dx, size_t n_grids, double mass, double xmin, double xmax, double length, unsigned flags,
		double* W)
	{
		if (!ctx || !W || !dvr_grid_ok(n_grids, dx) || !std::isfinite(x_first) || !(mass > 0.0) || !std::isfinite(mass) || !std::isfinite(xmin) ||
			!std::isfinite(xmax) || !(xmin < xmax) || !(length > 0.0) || !std::isfinite(length))
			return GPLE_ERR_BAD_ARG;
		// the pole of W lies one absorber length outside the box: an end point at or beyond it is refused
		const double x_last = x_first + dx * static_cast<double>(n_grids - 1);
		if (xmin - x_first >= length || x_last - xmax >= length) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Staged w(ctx, dev);
		GPLE_HIP(ctx, w.out(W, n_grids));
		GPLE_HIP(ctx, launch_dvr_absorber(st, x_first, dx, static_cast<int>(n_grids), mass, xmin, xmax, length, w.p));
		GPLE_HIP(ctx, w.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	// the propagator of gple_dvr_propagator and, with G, the quadratic forms of gple_dvr_flux beside it (basis, n_left: theirs); U nullable with G
	static int dvr_power_call(gple_ctx* ctx, int num_pes, size_t n_grids, const double* H, const double* W, double dt, size_t n_steps, const double* basis,
		size_t n_left, unsigned flags, double* U, double* G)
	{
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t dim = static_cast<size_t>(num_pes) * n_grids, ld = round_up(dim, 64);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Scratch work(ctx), fwork(ctx);
		Staged h(ctx, dev), w(ctx, dev), b(ctx, dev), u(ctx, dev), g(ctx, dev);
		// every allocation before the first launch: one that does not fit leaves the outputs untouched
		GPLE_HIP(ctx, work.get(dvr_power_work_doubles(num_pes, n)));
		if (G) GPLE_HIP(ctx, fwork.get(dvr_flux_work_doubles(num_pes, n)));
		GPLE_HIP(ctx, u.out(U, 2 * dim * dim));
		GPLE_HIP(ctx, g.out(G, 4 * num_pes * dim * dim));
		GPLE_HIP(ctx, h.in(H, dim * dim));
		GPLE_HIP(ctx, w.in(W, n_grids));
		GPLE_HIP(ctx, b.in(basis, n_grids * num_pes * num_pes));
		const DvrFlux flux{b.p, static_cast<int>(n_left), fwork.p};
		DvrPlanes R;
		GPLE_HIP(ctx, launch_dvr_power(ctx, st, num_pes, n, h.p, w.p, dt, static_cast<long>(n_steps), work.p, &R, G ? &flux : nullptr));
		const double* const padded[2] = {R.re, R.im}; // the padded planes, without their padding
		for (size_t plane = 0; u.p && plane < 2; ++plane)
			GPLE_HIP(ctx, hipMemcpy2DAsync(u.p + plane * dim * dim, dim * sizeof(double), padded[plane], ld * sizeof(double), dim * sizeof(double), dim,
				hipMemcpyDeviceToDevice, st));
		if (G) GPLE_HIP(ctx, launch_dvr_flux_export(st, num_pes, n, flux, g.p));
		GPLE_HIP(ctx, u.back());
		GPLE_HIP(ctx, g.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_dvr_propagator(gple_ctx* ctx, int num_pes, size_t n_grids, const double* H, const double* W, double dt, size_t n_steps, unsigned flags, double* U)
	{
		if (!ctx || !dvr_power_args_ok(num_pes, n_grids, dt, n_steps) || !H || !U) return GPLE_ERR_BAD_ARG;
		return dvr_power_call(ctx, num_pes, n_grids, H, W, dt, n_steps, nullptr, 0, flags, U, nullptr);
	}

	int gple_dvr_apply(gple_ctx* ctx, int num_pes, size_t n_grids, const double* U, const double* psi0, size_t T, const double* basis, unsigned flags,
		double* psi)
	{
		if (!ctx || (num_pes != 2 && num_pes != 3) || !dvr_grid_ok(n_grids, 1.0) || T > 4096 || (T && (!U || !psi0 || !psi))) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (T == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t dim = static_cast<size_t>(num_pes) * n_grids;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Scratch dia(ctx);
		Staged u(ctx, dev), v(ctx, dev), b(ctx, dev), o(ctx, dev);
		GPLE_HIP(ctx, u.in(U, 2 * dim * dim));
		GPLE_HIP(ctx, v.in(psi0, 2 * dim));
		GPLE_HIP(ctx, b.in(basis, n_grids * num_pes * num_pes));
		GPLE_HIP(ctx, o.out(psi, 2 * dim * T));
		if (b.p) GPLE_HIP(ctx, dia.get(2 * dim * T));
		GPLE_HIP(ctx, launch_dvr_apply(st, num_pes, n, u.p, v.p, static_cast<int>(T), b.p, dia.p, o.p));
		GPLE_HIP(ctx, o.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- what the absorber took (gple_dvr_flux.hip): the quadratic forms of the absorbed population per channel, and their application ------ */
	int gple_dvr_flux(gple_ctx* ctx, int num_pes, size_t n_grids, const double* H, const double* W, double dt, size_t n_steps, const double* basis,
		size_t n_left, unsigned flags, double* U, double* G)
	{
		if (!ctx || !dvr_power_args_ok(num_pes, n_grids, dt, n_steps) || !H || !G || !basis || n_left > n_grids) return GPLE_ERR_BAD_ARG;
		return dvr_power_call(ctx, num_pes, n_grids, H, W, dt, n_steps, basis, n_left, flags, U, G);
	}

	int gple_dvr_flux_apply(gple_ctx* ctx, int num_pes, size_t n_grids, const double* G, const double* psi, size_t T, unsigned flags, double* absorbed)
	{
		if (!ctx || (num_pes != 2 && num_pes != 3) || !dvr_grid_ok(n_grids, 1.0) || T < 1 || T > 4096 || !G || !psi || !absorbed) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t dim = static_cast<size_t>(num_pes) * n_grids;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Scratch partial(ctx);
		Staged g(ctx, dev), v(ctx, dev), o(ctx, dev);
		GPLE_HIP(ctx, partial.get(dvr_flux_apply_work_doubles(num_pes, n, static_cast<int>(T))));
		GPLE_HIP(ctx, o.out(absorbed, T * 2 * num_pes));
		GPLE_HIP(ctx, g.in(G, 4 * num_pes * dim * dim));
		GPLE_HIP(ctx, v.in(psi, 2 * dim * T));
		GPLE_HIP(ctx, launch_dvr_flux_apply(st, num_pes, n, g.p, v.p, static_cast<int>(T), partial.p, o.p));
		GPLE_HIP(ctx, o.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- the spectrum of one absorbing run (gple_dvr_spectrum.hip): the half-Fourier transform of 2^levels steps per energy, and what each channel took */
	int gple_dvr_spectrum(gple_ctx* ctx, int num_pes, size_t n_grids, const double* H, const double* W, double dt, int levels, const double* basis,
		size_t n_left, const double* psi0, const double* energies, size_t n_E, unsigned flags, double* density, double* psi_e, double* remaining)
	{
		if (!ctx || levels < 0 || levels > 30 || !dvr_power_args_ok(num_pes, n_grids, dt, size_t(1) << levels) || !H || !basis || !psi0 || !energies ||
			!density || n_left > n_grids || n_E < 1 || n_E > 4096)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids), C = 2 * num_pes;
		const size_t dim = static_cast<size_t>(num_pes) * n_grids;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		{ // every energy finite: device energies are looked at on the host first (n_E <= 4096 values)
			std::vector<double> seen;
			const double* e = energies;
			if (dev)
			{
				seen.resize(n_E);
				GPLE_HIP(ctx, hipMemcpyAsync(seen.data(), energies, n_E * sizeof(double), hipMemcpyDeviceToHost, st));
				GPLE_HIP(ctx, hipStreamSynchronize(st));
				e = seen.data();
			}
			for (size_t k = 0; k < n_E; ++k)
				if (!std::isfinite(e[k])) return GPLE_ERR_BAD_ARG;
		}
		Scratch pwork(ctx), work(ctx);
		Staged h(ctx, dev), w(ctx, dev), b(ctx, dev), v(ctx, dev), en(ctx, dev), d(ctx, dev), pe(ctx, dev), rem(ctx, dev);
		// every allocation before the first launch: one that does not fit leaves the outputs untouched
		GPLE_HIP(ctx, pwork.get(dvr_power_work_doubles(num_pes, n)));
		GPLE_HIP(ctx, work.get(dvr_spectrum_work_doubles(num_pes, n, static_cast<int>(n_E))));
		GPLE_HIP(ctx, d.out(density, n_E * C));
		GPLE_HIP(ctx, pe.out(psi_e, n_E * 2 * dim));
		GPLE_HIP(ctx, rem.out(remaining, 1));
		GPLE_HIP(ctx, h.in(H, dim * dim));
		GPLE_HIP(ctx, w.in(W, n_grids));
		GPLE_HIP(ctx, b.in(basis, n_grids * num_pes * num_pes));
		GPLE_HIP(ctx, v.in(psi0, 2 * dim));
		GPLE_HIP(ctx, en.in(energies, n_E));
		DvrSpectrum g{};
		g.num_pes = num_pes, g.n = n, g.levels = levels, g.n_left = static_cast<int>(n_left), g.n_E = static_cast<int>(n_E);
		g.H = h.p, g.W = w.p, g.dt = dt, g.basis = b.p, g.psi0 = v.p, g.energies = en.p, g.power_work = pwork.p, g.work = work.p;
		g.density = d.p, g.psi_e = pe.p, g.remaining = rem.p;
		GPLE_HIP(ctx, launch_dvr_spectrum(ctx, st, g));
		for (Staged* o : {&d, &pe, &rem}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- exact MQCLE dynamics (gple_mqcl.hip; liouville_equation/ of the reference) ------------------------------------------------------ */
	static bool mqcl_size_ok(gple_ctx* ctx, int num_pes, int model, size_t n, PesModel* pes) { return pes_resolve(ctx, num_pes, model, pes) && n >= 4 && n <= 4096; }

	// the per-x tables of gple_mqcl.hip from host or device x (tq: the time of one Q step, spectral: the FFT tables too)
	static int mqcl_tables(gple_ctx* ctx, hipStream_t st, int num_pes, const PesModel& model, const double* x, int n, double tq, bool spectral, Staged& xs,
		Scratch& tables)
	{
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, tables.get(mqcl_table_doubles(num_pes, n)));
		GPLE_HIP(ctx, launch_mqcl_tables(st, num_pes, model, xs.p, n, tq, spectral, tables.p));
		return GPLE_OK;
	}

	int gple_mqcl_transform(gple_ctx* ctx, int num_pes, int model, const double* x, size_t n_grids, int from, int to, unsigned flags, const double* rho_in,
		double* rho_out)
	{
		PesModel pes;
		if (!ctx || !mqcl_size_ok(ctx, num_pes, model, n_grids, &pes) || from < 0 || from > 2 || to < 0 || to > 2 || !x || !rho_in || !rho_out) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t doubles = 2 * static_cast<size_t>(num_pes) * num_pes * n_grids * n_grids;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ri(ctx, dev), ro(ctx, dev);
		Scratch tables(ctx);
		GPLE_TRY(mqcl_tables(ctx, st, num_pes, pes, x, n, 0.0, false, xs, tables));
		GPLE_HIP(ctx, ri.in(rho_in, doubles));
		GPLE_HIP(ctx, ro.out(rho_out, doubles));
		GPLE_HIP(ctx, launch_mqcl_transform(st, num_pes, n, from, to, tables.p, ri.p, ro.p));
		GPLE_HIP(ctx, ro.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_mqcl_evolve(gple_ctx* ctx, int num_pes, int model, const double* x, const double* p, size_t n_grids, double mass, double length_x,
		double length_p, double dt, size_t n_steps, unsigned flags, double* rho)
	{
		PesModel pes;
		if (!ctx || !mqcl_size_ok(ctx, num_pes, model, n_grids, &pes) || !x || !p || !rho || !(mass > 0.0) || !std::isfinite(mass) || !(length_x > 0.0) ||
			!std::isfinite(length_x) || !(length_p > 0.0) || !std::isfinite(length_p) || !std::isfinite(dt) || n_steps > (1ul << 40))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t plane = n_grids * n_grids, doubles = 2 * static_cast<size_t>(num_pes) * num_pes * plane;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), pp(ctx, dev), r(ctx, dev);
		Scratch tables(ctx), tr(ctx);
		GPLE_TRY(mqcl_tables(ctx, st, num_pes, pes, x, n, dt / 2.0, true, xs, tables));
		GPLE_HIP(ctx, tr.get(2 * plane * (num_pes * (num_pes + 1) / 2)));
		GPLE_HIP(ctx, pp.in(p, n_grids));
		GPLE_HIP(ctx, r.inout(rho, doubles));
		MqclEvolveArgs g{};
		g.num_pes = num_pes, g.n = n, g.n_steps = static_cast<long>(n_steps), g.rho = r.p, g.transposed = tr.p, g.table = tables.p, g.p = pp.p;
		g.mass = mass, g.length_x = length_x, g.length_p = length_p, g.dt = dt;
		timer_start(ctx, GPLE_TIMER_MQCL);
		GPLE_HIP(ctx, launch_mqcl_evolve(st, g));
		timer_stop(ctx, GPLE_TIMER_MQCL);
		GPLE_HIP(ctx, launch_mqcl_lower(st, num_pes, n, r.p));
		GPLE_HIP(ctx, r.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_mqcl_observe(gple_ctx* ctx, int num_pes, int model, const double* x, const double* p, size_t n_grids, double mass, double dx, double dp,
		unsigned flags, const double* rho_dia, double* rho_adia, double* averages, double* populations)
	{
		PesModel pes;
		if (!ctx || !mqcl_size_ok(ctx, num_pes, model, n_grids, &pes) || !x || !p || !rho_dia || !averages || !populations || !(mass > 0.0) || !std::isfinite(mass) ||
			!std::isfinite(dx) || !std::isfinite(dp))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t doubles = 2 * static_cast<size_t>(num_pes) * num_pes * n_grids * n_grids;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), pp(ctx, dev), r(ctx, dev), a(ctx, dev);
		Scratch tables(ctx), work(ctx), outd(ctx);
		GPLE_TRY(mqcl_tables(ctx, st, num_pes, pes, x, n, 0.0, false, xs, tables));
		GPLE_HIP(ctx, pp.in(p, n_grids));
		GPLE_HIP(ctx, r.in(rho_dia, doubles));
		GPLE_HIP(ctx, a.out(rho_adia, doubles));
		GPLE_HIP(ctx, work.get(mqcl_observe_work_doubles(num_pes, n)));
		GPLE_HIP(ctx, outd.get(3 + num_pes));
		GPLE_HIP(ctx, launch_mqcl_observe(st, num_pes, n, tables.p, xs.p, pp.p, mass, dx * dp, r.p, a.p, work.p, outd.p));
		if (dev)
		{
			GPLE_HIP(ctx, hipMemcpyAsync(averages, outd.p, 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
			GPLE_HIP(ctx, hipMemcpyAsync(populations, outd.p + 3, num_pes * sizeof(double), hipMemcpyDeviceToDevice, st));
			return GPLE_OK;
		}
		double h[6];
		GPLE_HIP(ctx, hipMemcpyAsync(h, outd.p, (3 + num_pes) * sizeof(double), hipMemcpyDeviceToHost, st));
		GPLE_HIP(ctx, a.back());
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		for (int k = 0; k < 3; ++k) averages[k] = h[k];
		for (int k = 0; k < num_pes; ++k) populations[k] = h[3 + k];
		return GPLE_OK;
	}

	/* ---- fewest-switches surface hopping (gple_hop.hip) --------------------------------------------------------------------- */
	static bool hop_size_ok(gple_ctx* ctx, int num_pes, int model, size_t n, size_t offset, PesModel* pes)
	{
		constexpr size_t LIMIT = size_t(1) << 32; // the trajectory index is one word of the counter
		return pes_resolve(ctx, num_pes, model, pes) && n >= 1 && n <= LIMIT && offset <= LIMIT - n;
	}
	static bool hop_positive(double v) { return std::isfinite(v) && v > 0.0; }
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

	int gple_hop_sample(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
		double sigma_x, double sigma_p, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, trajectory_offset, &pes) || !hop_positive(sigma_x) || !hop_positive(sigma_p) || surface0 < 0 ||
			surface0 >= num_pes || !x || !p || !b || !surface || !status)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		GPLE_HIP(ctx, xs.out(x, n));
		GPLE_HIP(ctx, ps.out(p, n));
		GPLE_HIP(ctx, bs.out(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, false, true));
		GPLE_HIP(ctx, ss.stage(status, n, false, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_sample(st, e, pes, x0, p0, sigma_x, sigma_p, surface0));
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	// decoherence is a GPLE_HOP_DC_*, and in mode EDC edc_c is finite and not negative (it is read in that mode only)
	static bool hop_decoherence_ok(int decoherence, double edc_c)
	{
		if (decoherence < GPLE_HOP_DC_NONE || decoherence > GPLE_HOP_DC_COLLAPSE_ATTEMPT) return false;
		return decoherence != GPLE_HOP_DC_EDC || (std::isfinite(edc_c) && edc_c >= 0.0);
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
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, true, true));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP);
		const hipError_t launched = launch_hop_evolve_dc(st, e, pes, mass, dt, first_step, static_cast<long>(n_steps), x_left, x_right,
			(flags & GPLE_HOP_REVERSE) != 0, decoherence, edc_c); // GPLE_HOP_DC_NONE: the kernels gple_hop_evolve always launched
		timer_stop(ctx, GPLE_TIMER_HOP); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
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
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev), o(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		Scratch work(ctx);
		GPLE_HIP(ctx, work.get(hop_observe_work_doubles(num_pes, static_cast<long>(n))));
		GPLE_HIP(ctx, o.out(out, 4 * num_pes + 3));
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, ps.in(p, n));
		GPLE_HIP(ctx, bs.in(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, true, false));
		GPLE_HIP(ctx, ss.stage(status, n, true, false));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_observe(st, e, pes, mass, work.p, o.p));
		GPLE_HIP(ctx, o.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	// n_x n_p <= GPLE_HOP_MAX_CELLS, without overflow
	static bool hop_cells_ok(size_t n_x, size_t n_p) { return n_x >= 1 && n_p >= 1 && n_x <= GPLE_HOP_MAX_CELLS && n_p <= GPLE_HOP_MAX_CELLS / n_x; }

	int gple_hop_bin(gple_ctx* ctx, int num_pes, int model, size_t n, double x_first, double dx, size_t n_x, double p_first, double dp, size_t n_p,
		unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status, long long* acc)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_cells_ok(n_x, n_p) || !hop_positive(dx) || !hop_positive(dp) ||
			!std::isfinite(x_first) || !std::isfinite(p_first) || !x || !p || !b || !surface || !status || !acc)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE, keep = flags & GPLE_HOP_ACCUMULATE;
		const size_t words = static_cast<size_t>(hop_bin_planes(num_pes)) * n_x * n_p + 2;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		Scratch sums(ctx); // a host acc: the integers in pooled memory (8 bytes each, as a double)
		long long* a = acc;
		if (!dev)
		{
			GPLE_HIP(ctx, sums.get(words));
			a = reinterpret_cast<long long*>(sums.p);
		}
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, ps.in(p, n));
		GPLE_HIP(ctx, bs.in(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, true, false));
		GPLE_HIP(ctx, ss.stage(status, n, true, false));
		if (!keep) GPLE_HIP(ctx, hipMemsetAsync(a, 0, words * sizeof(long long), st));
		else if (!dev) GPLE_HIP(ctx, hipMemcpyAsync(a, acc, words * sizeof(long long), hipMemcpyHostToDevice, st));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, su.p, ss.p};
		const HopGrid g{x_first, dx, p_first, dp, static_cast<long>(n_x), static_cast<long>(n_p)};
		timer_start(ctx, GPLE_TIMER_HOP_BIN);
		const hipError_t launched = launch_hop_bin(st, e, pes, g, (flags & GPLE_HOP_BIN_ALL) != 0, a);
		timer_stop(ctx, GPLE_TIMER_HOP_BIN); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		if (!dev)
		{
			GPLE_HIP(ctx, hipMemcpyAsync(acc, a, words * sizeof(long long), hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
		}
		return GPLE_OK;
	}

	int gple_hop_density(gple_ctx* ctx, int num_pes, size_t n_x, size_t n_p, double dx, double dp, size_t n_norm, unsigned flags, const long long* acc,
		double* rho)
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
		GPLE_HIP(ctx, launch_hop_density(st, num_pes, static_cast<long>(cells), w, a, r.p));
		GPLE_HIP(ctx, r.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- grouped ensembles ("A curve in one launch") ------------------------------------------------------------------------ */
	// n = n_groups n_per_group without overflow, within the index space together with the offset
	static bool hop_groups_ok(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t offset, PesModel* pes, size_t* n)
	{
		if (n_groups == 0 || n_per_group == 0 || n_groups > GPLE_HOP_MAX_GROUPS || n_per_group > (size_t(1) << 32) / n_groups) return false;
		*n = n_groups * n_per_group;
		return hop_size_ok(ctx, num_pes, model, *n, offset, pes);
	}
	// a host table of a grouped call in pooled device memory.  The table is the caller's pageable memory whatever the flags say: the copy is
	// waited for, so that the caller may free it when the call returns
	static hipError_t hop_table(Scratch& t, const double* host, size_t count)
	{
		hipError_t e = t.get(count);
		if (e != hipSuccess) return e;
		e = hipMemcpyAsync(t.p, host, count * sizeof(double), hipMemcpyHostToDevice, t.ctx->stream);
		return e == hipSuccess ? hipStreamSynchronize(t.ctx->stream) : e;
	}

	int gple_hop_sample_groups(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset, unsigned long long seed,
		const double* packets, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, trajectory_offset, &pes, &n) || !packets || surface0 < 0 || surface0 >= num_pes ||
			!x || !p || !b || !surface || !status)
			return GPLE_ERR_BAD_ARG;
		for (size_t g = 0; g < n_groups; ++g)
		{
			const double* row = packets + 4 * g;
			if (!std::isfinite(row[0]) || !std::isfinite(row[1]) || !std::isfinite(row[2]) || !std::isfinite(row[3]) || row[2] < 0.0 || row[3] < 0.0) return GPLE_ERR_BAD_ARG;
		}
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		Scratch table(ctx);
		GPLE_HIP(ctx, hop_table(table, packets, 4 * n_groups));
		GPLE_HIP(ctx, xs.out(x, n));
		GPLE_HIP(ctx, ps.out(p, n));
		GPLE_HIP(ctx, bs.out(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, false, true));
		GPLE_HIP(ctx, ss.stage(status, n, false, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_sample_groups(st, e, pes, static_cast<long>(n_per_group), table.p, surface0));
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
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
		for (size_t g = 0; g < n_groups; ++g)
			if (!hop_positive(dt[g])) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev), hs(ctx, dev);
		Scratch table(ctx);
		GPLE_HIP(ctx, hop_table(table, dt, n_groups));
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, true, true));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		if (hops) GPLE_HIP(ctx, hs.stage(hops, 2 * n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP_GROUPS);
		const hipError_t launched = launch_hop_evolve_groups_dc(st, e, pes, static_cast<long>(n_per_group), mass, table.p, first_step, static_cast<long>(n_steps), x_left,
			x_right, (flags & GPLE_HOP_REVERSE) != 0, hs.p, decoherence, edc_c); // GPLE_HOP_DC_NONE: the kernels gple_hop_evolve_groups always launched
		timer_stop(ctx, GPLE_TIMER_HOP_GROUPS); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss, &hs}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
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
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev), o(ctx, false); // out is a host array whatever the flags say
		StagedInts su(ctx, dev), ss(ctx, dev);
		Scratch work(ctx);
		GPLE_HIP(ctx, work.get(hop_observe_groups_work_doubles(num_pes, static_cast<long>(n_groups), static_cast<long>(n_per_group))));
		GPLE_HIP(ctx, o.out(out, n_groups * (4 * num_pes + 3)));
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, ps.in(p, n));
		GPLE_HIP(ctx, bs.in(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, true, false));
		GPLE_HIP(ctx, ss.stage(status, n, true, false));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_observe_groups(st, e, pes, static_cast<long>(n_groups), static_cast<long>(n_per_group), mass, work.p, o.p));
		GPLE_HIP(ctx, o.back());
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- Ehrenfest (mean-field) trajectories ("Mean-field (Ehrenfest) trajectories") ------------------------------------------- */
	// what the two evolve calls share: the checks of gple_hop_evolve that apply without a surface, a seed and an offset
	static bool hop_mf_evolve_ok(double mass, size_t n_steps, double x_left, double x_right, unsigned flags, const double* x, const double* p, const double* b,
		const int* status)
	{
		return hop_positive(mass) && std::isfinite(x_left) && std::isfinite(x_right) && x_left < x_right && n_steps <= (1ul << 40) && !(flags & GPLE_HOP_REVERSE) &&
			x && p && b && status;
	}

	int gple_hop_evolve_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, double dt, size_t n_steps, double x_left, double x_right, unsigned flags,
		double* x, double* p, double* b, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(dt) || !hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts ss(ctx, dev);
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP_MF);
		const hipError_t launched = launch_hop_evolve_mf(st, e, pes, mass, dt, static_cast<long>(n_steps), x_left, x_right);
		timer_stop(ctx, GPLE_TIMER_HOP_MF); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		GPLE_HIP(ctx, ss.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_hop_evolve_groups_mf(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt, size_t n_steps,
		double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !dt ||
			!hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status))
			return GPLE_ERR_BAD_ARG;
		for (size_t g = 0; g < n_groups; ++g)
			if (!hop_positive(dt[g])) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts ss(ctx, dev);
		Scratch table(ctx);
		GPLE_HIP(ctx, hop_table(table, dt, n_groups));
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP_MF);
		const hipError_t launched = launch_hop_evolve_groups_mf(st, e, pes, static_cast<long>(n_per_group), mass, table.p, static_cast<long>(n_steps), x_left, x_right);
		timer_stop(ctx, GPLE_TIMER_HOP_MF); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		GPLE_HIP(ctx, ss.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_hop_observe_mf(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, unsigned flags, const double* x, const double* p, const double* b,
		const int* status, double* out)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(mass) || !x || !p || !b || !status || !out) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev), o(ctx, dev);
		StagedInts ss(ctx, dev);
		Scratch work(ctx);
		GPLE_HIP(ctx, work.get(hop_observe_mf_work_doubles(num_pes, static_cast<long>(n))));
		GPLE_HIP(ctx, o.out(out, 3 * num_pes + 6));
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, ps.in(p, n));
		GPLE_HIP(ctx, bs.in(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, false));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		GPLE_HIP(ctx, launch_hop_observe_mf(st, e, pes, mass, work.p, o.p));
		GPLE_HIP(ctx, o.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_hop_observe_groups_mf(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, unsigned flags, const double* x,
		const double* p, const double* b, const int* status, double* out)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !hop_positive(mass) || !x || !p || !b || !status || !out)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev), o(ctx, false); // out is a host array whatever the flags say
		StagedInts ss(ctx, dev);
		Scratch work(ctx);
		GPLE_HIP(ctx, work.get(hop_observe_groups_mf_work_doubles(num_pes, static_cast<long>(n_groups), static_cast<long>(n_per_group))));
		GPLE_HIP(ctx, o.out(out, n_groups * (3 * num_pes + 6)));
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, ps.in(p, n));
		GPLE_HIP(ctx, bs.in(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, false));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		GPLE_HIP(ctx, launch_hop_observe_groups_mf(st, e, pes, static_cast<long>(n_groups), static_cast<long>(n_per_group), mass, work.p, o.p));
		GPLE_HIP(ctx, o.back());
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- symmetrical quasi-classical trajectories ("Symmetrical quasi-classical trajectories") -------------------------------- */
	// gamma of the step, where no window is named: finite and not negative
	static bool hop_sqc_gamma_ok(double gamma) { return std::isfinite(gamma) && gamma >= 0.0; }
	// window is a GPLE_HOP_WINDOW_* and gamma fits it: the square windows are disjoint for 0 < gamma < 1/2 only
	static bool hop_sqc_window_ok(int window, double gamma)
	{
		if (window != GPLE_HOP_WINDOW_SQUARE && window != GPLE_HOP_WINDOW_TRIANGLE) return false;
		return hop_sqc_gamma_ok(gamma) && (window != GPLE_HOP_WINDOW_SQUARE || (gamma > 0.0 && gamma < 0.5));
	}

	int gple_hop_sample_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
		double sigma_x, double sigma_p, int surface0, int window, double gamma, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, trajectory_offset, &pes) || !hop_positive(sigma_x) || !hop_positive(sigma_p) || surface0 < 0 ||
			surface0 >= num_pes || !hop_sqc_window_ok(window, gamma) || (flags & GPLE_HOP_REVERSE) || !x || !p || !b || !surface || !status)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		GPLE_HIP(ctx, xs.out(x, n));
		GPLE_HIP(ctx, ps.out(p, n));
		GPLE_HIP(ctx, bs.out(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, false, true));
		GPLE_HIP(ctx, ss.stage(status, n, false, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_sample_sqc(st, e, pes, x0, p0, sigma_x, sigma_p, surface0, window, gamma));
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
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
		for (size_t g = 0; g < n_groups; ++g)
		{
			const double* row = packets + 4 * g;
			if (!std::isfinite(row[0]) || !std::isfinite(row[1]) || !std::isfinite(row[2]) || !std::isfinite(row[3]) || row[2] < 0.0 || row[3] < 0.0) return GPLE_ERR_BAD_ARG;
		}
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		Scratch table(ctx);
		GPLE_HIP(ctx, hop_table(table, packets, 4 * n_groups));
		GPLE_HIP(ctx, xs.out(x, n));
		GPLE_HIP(ctx, ps.out(p, n));
		GPLE_HIP(ctx, bs.out(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, false, true));
		GPLE_HIP(ctx, ss.stage(status, n, false, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_sample_groups_sqc(st, e, pes, static_cast<long>(n_per_group), table.p, surface0, window, gamma));
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
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
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts ss(ctx, dev);
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP_SQC);
		const hipError_t launched = launch_hop_evolve_sqc(st, e, pes, mass, dt, static_cast<long>(n_steps), x_left, x_right, gamma);
		timer_stop(ctx, GPLE_TIMER_HOP_SQC); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		GPLE_HIP(ctx, ss.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_hop_evolve_groups_sqc(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt, size_t n_steps,
		double x_left, double x_right, double gamma, unsigned flags, double* x, double* p, double* b, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !dt ||
			!hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status) || !hop_sqc_gamma_ok(gamma))
			return GPLE_ERR_BAD_ARG;
		for (size_t g = 0; g < n_groups; ++g)
			if (!hop_positive(dt[g])) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts ss(ctx, dev);
		Scratch table(ctx);
		GPLE_HIP(ctx, hop_table(table, dt, n_groups));
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP_SQC);
		const hipError_t launched =
			launch_hop_evolve_groups_sqc(st, e, pes, static_cast<long>(n_per_group), mass, table.p, static_cast<long>(n_steps), x_left, x_right, gamma);
		timer_stop(ctx, GPLE_TIMER_HOP_SQC); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		GPLE_HIP(ctx, ss.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_hop_observe_sqc(gple_ctx* ctx, int num_pes, int model, size_t n, double mass, int window, double gamma, unsigned flags, const double* x,
		const double* p, const double* b, const int* status, double* out)
	{
		PesModel pes;
		if (!ctx || !hop_size_ok(ctx, num_pes, model, n, 0, &pes) || !hop_positive(mass) || !hop_sqc_window_ok(window, gamma) || (flags & GPLE_HOP_REVERSE) || !x || !p ||
			!b || !status || !out)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev), o(ctx, dev);
		StagedInts ss(ctx, dev);
		Scratch work(ctx);
		GPLE_HIP(ctx, work.get(hop_observe_sqc_work_doubles(num_pes, static_cast<long>(n))));
		GPLE_HIP(ctx, o.out(out, 4 * num_pes + 9));
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, ps.in(p, n));
		GPLE_HIP(ctx, bs.in(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, false));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		GPLE_HIP(ctx, launch_hop_observe_sqc(st, e, pes, mass, window, gamma, work.p, o.p));
		GPLE_HIP(ctx, o.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
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
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev), o(ctx, false); // out is a host array whatever the flags say
		StagedInts ss(ctx, dev);
		Scratch work(ctx);
		GPLE_HIP(ctx, work.get(hop_observe_groups_sqc_work_doubles(num_pes, static_cast<long>(n_groups), static_cast<long>(n_per_group))));
		GPLE_HIP(ctx, o.out(out, n_groups * (4 * num_pes + 9)));
		GPLE_HIP(ctx, xs.in(x, n));
		GPLE_HIP(ctx, ps.in(p, n));
		GPLE_HIP(ctx, bs.in(b, 2 * n * num_pes));
		GPLE_HIP(ctx, ss.stage(status, n, true, false));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, nullptr, ss.p};
		GPLE_HIP(ctx, launch_hop_observe_groups_sqc(st, e, pes, static_cast<long>(n_groups), static_cast<long>(n_per_group), mass, window, gamma, work.p, o.p));
		GPLE_HIP(ctx, o.back());
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* ---- MASH trajectories ("MASH trajectories") -------------------------------------------------------------------------------- */
	// what the four calls share beyond the checks of their models: two levels, no GPLE_HOP_REVERSE (MASH always reflects), five arrays
	static bool hop_mash_ok(int num_pes, unsigned flags, const double* x, const double* p, const double* b, const int* surface, const int* status)
	{
		return num_pes == 2 && !(flags & GPLE_HOP_REVERSE) && x && p && b && surface && status;
	}

	int gple_hop_sample_mash(gple_ctx* ctx, int num_pes, int model, size_t n, size_t trajectory_offset, unsigned long long seed, double x0, double p0,
		double sigma_x, double sigma_p, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		if (!ctx || !hop_mash_ok(num_pes, flags, x, p, b, surface, status) || !hop_size_ok(ctx, num_pes, model, n, trajectory_offset, &pes) || !hop_positive(sigma_x) ||
			!hop_positive(sigma_p) || surface0 < 0 || surface0 >= num_pes)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		GPLE_HIP(ctx, xs.out(x, n));
		GPLE_HIP(ctx, ps.out(p, n));
		GPLE_HIP(ctx, bs.out(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, false, true));
		GPLE_HIP(ctx, ss.stage(status, n, false, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_sample_mash(st, e, pes, x0, p0, sigma_x, sigma_p, surface0));
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_hop_sample_groups_mash(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, size_t trajectory_offset,
		unsigned long long seed, const double* packets, int surface0, unsigned flags, double* x, double* p, double* b, int* surface, int* status)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_mash_ok(num_pes, flags, x, p, b, surface, status) ||
			!hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, trajectory_offset, &pes, &n) || !packets || surface0 < 0 || surface0 >= num_pes)
			return GPLE_ERR_BAD_ARG;
		for (size_t g = 0; g < n_groups; ++g)
		{
			const double* row = packets + 4 * g;
			if (!std::isfinite(row[0]) || !std::isfinite(row[1]) || !std::isfinite(row[2]) || !std::isfinite(row[3]) || row[2] < 0.0 || row[3] < 0.0) return GPLE_ERR_BAD_ARG;
		}
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		Scratch table(ctx);
		GPLE_HIP(ctx, hop_table(table, packets, 4 * n_groups));
		GPLE_HIP(ctx, xs.out(x, n));
		GPLE_HIP(ctx, ps.out(p, n));
		GPLE_HIP(ctx, bs.out(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, false, true));
		GPLE_HIP(ctx, ss.stage(status, n, false, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), trajectory_offset, seed, xs.p, ps.p, bs.p, su.p, ss.p};
		GPLE_HIP(ctx, launch_hop_sample_groups_mash(st, e, pes, static_cast<long>(n_per_group), table.p, surface0));
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
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
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev);
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, true, true));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, su.p, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP_MASH);
		const hipError_t launched = launch_hop_evolve_mash(st, e, pes, mass, dt, static_cast<long>(n_steps), x_left, x_right);
		timer_stop(ctx, GPLE_TIMER_HOP_MASH); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_hop_evolve_groups_mash(gple_ctx* ctx, int num_pes, int model, size_t n_groups, size_t n_per_group, double mass, const double* dt,
		size_t n_steps, double x_left, double x_right, unsigned flags, double* x, double* p, double* b, int* surface, int* status, int* hops)
	{
		PesModel pes;
		size_t n = 0;
		if (!ctx || !hop_mash_ok(num_pes, flags, x, p, b, surface, status) || !hop_groups_ok(ctx, num_pes, model, n_groups, n_per_group, 0, &pes, &n) || !dt ||
			!hop_mf_evolve_ok(mass, n_steps, x_left, x_right, flags, x, p, b, status))
			return GPLE_ERR_BAD_ARG;
		for (size_t g = 0; g < n_groups; ++g)
			if (!hop_positive(dt[g])) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), ps(ctx, dev), bs(ctx, dev);
		StagedInts su(ctx, dev), ss(ctx, dev), hs(ctx, dev);
		Scratch table(ctx);
		GPLE_HIP(ctx, hop_table(table, dt, n_groups));
		GPLE_HIP(ctx, xs.inout(x, n));
		GPLE_HIP(ctx, ps.inout(p, n));
		GPLE_HIP(ctx, bs.inout(b, 2 * n * num_pes));
		GPLE_HIP(ctx, su.stage(surface, n, true, true));
		GPLE_HIP(ctx, ss.stage(status, n, true, true));
		if (hops) GPLE_HIP(ctx, hs.stage(hops, 2 * n, true, true));
		const HopEnsemble e{num_pes, static_cast<long>(n), 0, 0, xs.p, ps.p, bs.p, su.p, ss.p};
		timer_start(ctx, GPLE_TIMER_HOP_MASH);
		const hipError_t launched =
			launch_hop_evolve_groups_mash(st, e, pes, static_cast<long>(n_per_group), mass, table.p, static_cast<long>(n_steps), x_left, x_right, hs.p);
		timer_stop(ctx, GPLE_TIMER_HOP_MASH); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		for (Staged* o : {&xs, &ps, &bs}) GPLE_HIP(ctx, o->back());
		for (StagedInts* o : {&su, &ss, &hs}) GPLE_HIP(ctx, o->back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}
}
