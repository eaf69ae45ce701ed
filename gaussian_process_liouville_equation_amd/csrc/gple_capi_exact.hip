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

	/* ---- the absorbing boundary of the MQCLE run (gple_mqcl_absorb.hip) ------------------------------------------------------ */
	// what every mask of a call shares: g on the device, the number of rows with g_i != 0 from the host's copy of g (a device g is copied back
	// once, which drains the stream) and their ascending list
	struct MqclMask
	{
		Staged g;
		Scratch rows, slab;
		int count = 0;
		MqclMask(gple_ctx* ctx, bool dev): g(ctx, dev), rows(ctx), slab(ctx) {}
	};
	static int mqcl_mask_plan(gple_ctx* ctx, hipStream_t st, int num_pes, const double* g, int n, bool dev, MqclMask& m)
	{
		GPLE_HIP(ctx, m.g.in(g, n));
		std::vector<double> copy;
		if (dev)
		{
			copy.resize(n);
			GPLE_HIP(ctx, hipMemcpyAsync(copy.data(), g, n * sizeof(double), hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			g = copy.data();
		}
		for (int i = 0; i < n; ++i) m.count += g[i] != 0.0;
		GPLE_HIP(ctx, m.rows.get(mqcl_absorb_rows_doubles(n)));
		GPLE_HIP(ctx, m.slab.get(mqcl_absorb_slab_doubles(num_pes, n, m.count)));
		if (m.count) GPLE_HIP(ctx, launch_mqcl_absorb_rows(st, m.g.p, n, reinterpret_cast<int*>(m.rows.p)));
		return GPLE_OK;
	}
	static MqclAbsorbArgs mqcl_mask_args(int num_pes, const PesModel& pes, int n, size_t n_left, const double* x, const MqclMask& m, double* rho, double* absorbed_p)
	{
		MqclAbsorbArgs a{};
		a.num_pes = num_pes, a.n = n, a.n_left = static_cast<int>(n_left), a.count = m.count, a.model = pes, a.x = x, a.g = m.g.p;
		a.rows = reinterpret_cast<const int*>(m.rows.p), a.slab = m.slab.p, a.rho = rho, a.absorbed_p = absorbed_p;
		return a;
	}

	int gple_mqcl_absorb(gple_ctx* ctx, int num_pes, int model, const double* x, size_t n_grids, const double* g, size_t n_left, unsigned flags, double* rho,
		double* absorbed_p)
	{
		PesModel pes;
		if (!ctx || !mqcl_size_ok(ctx, num_pes, model, n_grids, &pes) || n_left > n_grids || !x || !g || !rho || !absorbed_p) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t doubles = 2 * static_cast<size_t>(num_pes) * num_pes * n_grids * n_grids;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), r(ctx, dev), acc(ctx, dev);
		MqclMask mask(ctx, dev);
		GPLE_TRY(mqcl_mask_plan(ctx, st, num_pes, g, n, dev, mask));
		GPLE_HIP(ctx, xs.in(x, n_grids));
		GPLE_HIP(ctx, r.inout(rho, doubles));
		GPLE_HIP(ctx, acc.inout(absorbed_p, 2 * static_cast<size_t>(num_pes) * n_grids));
		GPLE_HIP(ctx, launch_mqcl_absorb(st, mqcl_mask_args(num_pes, pes, n, n_left, xs.p, mask, r.p, acc.p)));
		GPLE_HIP(ctx, r.back());
		GPLE_HIP(ctx, acc.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_mqcl_evolve_absorbing(gple_ctx* ctx, int num_pes, int model, const double* x, const double* p, size_t n_grids, double mass, double length_x,
		double length_p, double dt, size_t n_steps, size_t mask_every, const double* g, size_t n_left, unsigned flags, double* rho, double* absorbed_p)
	{
		PesModel pes;
		if (!ctx || !mqcl_size_ok(ctx, num_pes, model, n_grids, &pes) || !x || !p || !rho || !(mass > 0.0) || !std::isfinite(mass) || !(length_x > 0.0) ||
			!std::isfinite(length_x) || !(length_p > 0.0) || !std::isfinite(length_p) || !std::isfinite(dt) || n_steps > (1ul << 40) || mask_every == 0 ||
			n_steps % mask_every != 0 || n_left > n_grids || !g || !absorbed_p)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n_steps == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const int n = static_cast<int>(n_grids);
		const size_t plane = n_grids * n_grids, doubles = 2 * static_cast<size_t>(num_pes) * num_pes * plane;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged xs(ctx, dev), pp(ctx, dev), r(ctx, dev), acc(ctx, dev);
		Scratch tables(ctx), tr(ctx);
		MqclMask mask(ctx, dev);
		GPLE_TRY(mqcl_mask_plan(ctx, st, num_pes, g, n, dev, mask));
		GPLE_TRY(mqcl_tables(ctx, st, num_pes, pes, x, n, dt / 2.0, true, xs, tables));
		GPLE_HIP(ctx, tr.get(2 * plane * (num_pes * (num_pes + 1) / 2)));
		GPLE_HIP(ctx, pp.in(p, n_grids));
		GPLE_HIP(ctx, r.inout(rho, doubles));
		GPLE_HIP(ctx, acc.inout(absorbed_p, 2 * static_cast<size_t>(num_pes) * n_grids));
		MqclEvolveArgs e{};
		e.num_pes = num_pes, e.n = n, e.n_steps = static_cast<long>(mask_every), e.rho = r.p, e.transposed = tr.p, e.table = tables.p, e.p = pp.p;
		e.mass = mass, e.length_x = length_x, e.length_p = length_p, e.dt = dt;
		const MqclAbsorbArgs a = mqcl_mask_args(num_pes, pes, n, n_left, xs.p, mask, r.p, acc.p);
		// per block what gple_mqcl_absorb, gple_mqcl_evolve (mask_every steps), gple_mqcl_absorb enqueue, in that order: the same bits
		timer_start(ctx, GPLE_TIMER_MQCL);
		for (size_t block = 0; block < n_steps / mask_every; ++block)
		{
			GPLE_HIP(ctx, launch_mqcl_absorb(st, a));
			GPLE_HIP(ctx, launch_mqcl_evolve(st, e));
			GPLE_HIP(ctx, launch_mqcl_lower(st, num_pes, n, r.p));
			GPLE_HIP(ctx, launch_mqcl_absorb(st, a));
		}
		timer_stop(ctx, GPLE_TIMER_MQCL);
		GPLE_HIP(ctx, r.back());
		GPLE_HIP(ctx, acc.back());
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
}
