// gple_capi_recon.hip — C-ABI entry points of include/gple.h: the reconstruction of a gridded density with the NLML GP (gple_recon.hip).
#include <algorithm>
#include <cmath>
#include <memory>

#include "gple_capi.h"

namespace
{
	bool recon_grid_ok(size_t nx, size_t np) { return nx >= 2 && np >= 2 && nx <= (1u << 16) && np <= (1u << 16); }
	bool finite4(const double* x) { return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]) && std::isfinite(x[3]); }
	bool finite5(const double* x) { return finite4(x) && std::isfinite(x[4]); }
	// an int array of the caller by the call's GPLE_IO_DEVICE bit (Staged is for doubles)
	struct StagedInts
	{
		Scratch buf;
		const bool dev;
		int* p = nullptr;
		int* host = nullptr;
		size_t n = 0;
		StagedInts(gple_ctx* c, bool device): buf(c), dev(device) {}
		hipError_t out(int* dst, size_t count)
		{
			p = dst;
			if (dev) return hipSuccess;
			host = dst, n = count;
			hipError_t e = buf.get((count + 1) / 2);
			p = reinterpret_cast<int*>(buf.p);
			return e;
		}
		hipError_t back() { return host ? hipMemcpyAsync(host, p, n * sizeof(int), hipMemcpyDeviceToHost, buf.ctx->stream) : hipSuccess; }
	};
	// b = K^-1 y of the kernel x5 = (w_d, w_g, a, c, b) (c = 0: the diagonal kernel), with the give-up protocol of the one-launch factorisation
	int nlml_weights(gple_ctx* ctx, const double x5[5], const double* X, const double* y, size_t N, unsigned flags, double* b)
	{
		if (!ctx || !X || !y || !b || N == 0 || N > static_cast<size_t>(RECON_MAX_N)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		const bool dev = flags & GPLE_IO_DEVICE;
		for (int attempt = 0;; ++attempt)
		{
			CholSchemeScope scheme(attempt == 0 ? ctx->chol_scheme : 0); // second attempt: one launch per panel (a give-up of the one-launch scheme)
			Scratch Xt(ctx), yd(ctx), T(ctx), bv(ctx), info(ctx);
			int np = 0;
			timer_start(ctx, GPLE_TIMER_RECON);
			GPLE_TRY(nlml_solve(ctx, x5, X, y, N, Xt, yd, T, bv, info, &np, dev));
			timer_stop(ctx, GPLE_TIMER_RECON);
			GPLE_HIP(ctx, copy_out(st, b, bv.p, N, dev));
			GPLE_HIP(ctx, hipMemcpyAsync(ctx->host_scalars + HS_NLML + 8, info.p, 8, hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			timer_collect(ctx);
			bool again;
			GPLE_TRY(nlml_gave_up(ctx, attempt, &again));
			if (!again) break;
		}
		return GPLE_OK;
	}

	// one plane of either reconstruction entry point: x has 4 values (w_d, w_g, a_x, a_p) or, for the cross-term kernel, 5 (w_d, w_g, a, c, b)
	struct PlaneIn
	{
		const double* x;
		const double* X;
		const double* b;
		size_t N;
	};
	// both kernels share the arguments' rules, the staging, the energies, the records and the final sum; the diagonal kernel contracts two
	// tables, the cross-term kernel generates its operands inside the contraction (gple_recon.hip)
	int grid_reconstruct(gple_ctx* ctx, int num_pes, int model, const double* rho, const double* x, size_t nx, const double* p, size_t np, double mass,
		double dx, double dp, const PlaneIn* planes, bool cross, const double* scale, unsigned flags, double* pred, double* sums)
	{
		PesModel pes;
		if (!ctx || !pes_resolve(ctx, num_pes, model, &pes) || !recon_grid_ok(nx, np) || !rho || !x || !p || !planes || !sums || !(mass > 0.0) || !std::isfinite(mass) ||
			!std::isfinite(dx) || !std::isfinite(dp))
			return GPLE_ERR_BAD_ARG;
		const int nplanes = num_pes * num_pes;
		for (int q = 0; q < nplanes; ++q)
		{
			const PlaneIn& pl = planes[q];
			if (pl.N > static_cast<size_t>(RECON_MAX_N) || (pl.N && (!pl.X || !pl.b || !(cross ? finite5(pl.x) : finite4(pl.x)))) || (scale && !std::isfinite(scale[q]))) return GPLE_ERR_BAD_ARG;
		}
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t cells = nx * np;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged r(ctx, dev), xs(ctx, dev), ps(ctx, dev), po(ctx, dev), so(ctx, dev);
		std::vector<std::unique_ptr<Staged>> held;
		Scratch tables(ctx), energy(ctx), records(ctx);
		GPLE_HIP(ctx, r.in(rho, 2 * nplanes * cells));
		GPLE_HIP(ctx, xs.in(x, nx));
		GPLE_HIP(ctx, ps.in(p, np));
		GPLE_HIP(ctx, po.out(pred, nplanes * cells));
		GPLE_HIP(ctx, so.out(sums, static_cast<size_t>(GPLE_RECON_SUMS) * nplanes));
		ReconArgs g{};
		g.num_pes = num_pes, g.model = pes, g.nx = static_cast<int>(nx), g.np = static_cast<int>(np);
		g.rows_x = static_cast<int>(round_up(nx, 64)), g.rows_p = static_cast<int>(round_up(np, 64));
		g.rho = r.p, g.x = xs.p, g.p = ps.p, g.pred = po.p, g.sums = so.p, g.mass = mass, g.dxdp = dx * dp;
		size_t table_doubles = 0;
		for (int q = 0; q < nplanes; ++q)
		{
			ReconPlane& P = g.plane[q];
			P.N = static_cast<int>(planes[q].N), P.Npad = static_cast<int>(round_up(planes[q].N, 16));
			if (!cross) table_doubles += static_cast<size_t>(g.rows_x + g.rows_p) * P.Npad;
		}
		GPLE_HIP(ctx, tables.get(table_doubles));
		GPLE_HIP(ctx, energy.get(nx * num_pes));
		GPLE_HIP(ctx, records.get(recon_record_doubles(num_pes, g.nx, g.np)));
		g.energy = energy.p, g.records = records.p;
		double* next = tables.p;
		for (int q = 0; q < nplanes; ++q)
		{
			ReconPlane& P = g.plane[q];
			if (P.N == 0) continue;
			const double* px = planes[q].x;
			P.coef = (scale ? scale[q] : 1.0) * (px[1] * px[1]), P.ax = px[2], P.ap = px[cross ? 4 : 3], P.cross = cross ? px[3] : 0.0;
			if (!cross)
			{
				P.Ax = next, next += static_cast<size_t>(g.rows_x) * P.Npad;
				P.Ep = next, next += static_cast<size_t>(g.rows_p) * P.Npad;
			}
			for (int k = 0; k < 2; ++k)
			{
				held.emplace_back(new Staged(ctx, dev));
				GPLE_HIP(ctx, held.back()->in(k ? planes[q].b : planes[q].X, k ? planes[q].N : 2 * planes[q].N));
				(k ? P.b : P.X) = held.back()->p;
			}
		}
		timer_start(ctx, GPLE_TIMER_RECON);
		if (cross)
		{
			GPLE_HIP(ctx, launch_recon_energy(st, g));
			GPLE_HIP(ctx, launch_recon_cross(st, g));
		}
		else
		{
			GPLE_HIP(ctx, launch_recon_tables(st, g));
			GPLE_HIP(ctx, launch_recon_contract(st, g));
		}
		GPLE_HIP(ctx, launch_recon_final(st, g));
		timer_stop(ctx, GPLE_TIMER_RECON);
		GPLE_HIP(ctx, po.back());
		GPLE_HIP(ctx, so.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}
} // namespace

extern "C"
{
	int gple_nlml_weights(gple_ctx* ctx, const double x[4], const double* X, const double* y, size_t N, unsigned flags, double* b)
	{
		if (!x || !finite4(x)) return GPLE_ERR_BAD_ARG;
		const double x5[5] = {x[0], x[1], x[2], 0.0, x[3]};
		return nlml_weights(ctx, x5, X, y, N, flags, b);
	}
	int gple_nlml_cross_weights(gple_ctx* ctx, const double x[5], const double* X, const double* y, size_t N, unsigned flags, double* b)
	{
		if (!x || !finite5(x)) return GPLE_ERR_BAD_ARG;
		return nlml_weights(ctx, x, X, y, N, flags, b);
	}

	int gple_grid_survey(gple_ctx* ctx, int num_pes, int model, const double* rho, const double* x, size_t nx, const double* p, size_t np, double mass,
		double dx, double dp, unsigned flags, double* out)
	{
		PesModel pes;
		if (!ctx || !pes_resolve(ctx, num_pes, model, &pes) || !recon_grid_ok(nx, np) || !rho || !x || !p || !out || !(mass > 0.0) || !std::isfinite(mass) ||
			!std::isfinite(dx) || !std::isfinite(dp))
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t planes = static_cast<size_t>(num_pes) * num_pes;
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		Staged r(ctx, dev), xs(ctx, dev), ps(ctx, dev), o(ctx, dev);
		Scratch work(ctx);
		GPLE_HIP(ctx, r.in(rho, 2 * planes * nx * np));
		GPLE_HIP(ctx, xs.in(x, nx));
		GPLE_HIP(ctx, ps.in(p, np));
		GPLE_HIP(ctx, o.out(out, GPLE_SURVEY_STRIDE * planes));
		GPLE_HIP(ctx, work.get(recon_survey_work_doubles(num_pes)));
		timer_start(ctx, GPLE_TIMER_RECON);
		GPLE_HIP(ctx, launch_recon_survey(st, num_pes, pes, r.p, xs.p, static_cast<int>(nx), ps.p, static_cast<int>(np), mass, dx * dp, work.p, o.p));
		timer_stop(ctx, GPLE_TIMER_RECON);
		GPLE_HIP(ctx, o.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	int gple_grid_select(gple_ctx* ctx, int num_pes, const double* rho, const double* x, size_t nx, const double* p, size_t np, int q, int uniform,
		size_t n_select, unsigned long long seed, unsigned flags, int* cells, double* X, double* y, size_t* n_draws)
	{
		if (!ctx || (num_pes != 2 && num_pes != 3) || !recon_grid_ok(nx, np) || nx * np > static_cast<size_t>(INT_MAX) || !rho || !x || !p || q < 0 ||
			q >= num_pes * num_pes || n_select == 0 || n_select > static_cast<size_t>(RECON_MAX_N) || n_select > nx * np || !cells || !X || !y || !n_draws)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t planes = static_cast<size_t>(num_pes) * num_pes;
		const long ncells = static_cast<long>(nx * np), nchunks = recon_scan_chunks(ncells);
		const int ns = static_cast<int>(n_select);
		constexpr unsigned FIRST_BATCH = 4096, MAX_BATCH = 1u << 20, MAX_DRAWS = 1u << 30;
		GPLE_CALL(ctx);
		hipStream_t st = ctx->stream;
		Staged r(ctx, dev), xs(ctx, dev), ps(ctx, dev), Xo(ctx, dev), yo(ctx, dev);
		StagedInts co(ctx, dev);
		Scratch within(ctx), offsets(ctx), count(ctx), mark(ctx), draw(ctx), state(ctx), chosen(ctx);
		GPLE_HIP(ctx, r.in(rho, 2 * planes * nx * np));
		GPLE_HIP(ctx, xs.in(x, nx));
		GPLE_HIP(ctx, ps.in(p, np));
		GPLE_HIP(ctx, Xo.out(X, 2 * n_select));
		GPLE_HIP(ctx, yo.out(y, n_select));
		GPLE_HIP(ctx, co.out(cells, 2 * n_select));
		GPLE_HIP(ctx, mark.get((static_cast<size_t>(ncells) + 1) / 2));
		GPLE_HIP(ctx, draw.get(MAX_BATCH / 2));
		GPLE_HIP(ctx, state.get(1));
		GPLE_HIP(ctx, chosen.get((n_select + 1) / 2));
		int* const markp = reinterpret_cast<int*>(mark.p);
		int* const drawp = reinterpret_cast<int*>(draw.p);
		int* const statep = reinterpret_cast<int*>(state.p);
		int* const chosenp = reinterpret_cast<int*>(chosen.p);
		timer_start(ctx, GPLE_TIMER_RECON);
		GPLE_HIP(ctx, hipMemsetAsync(markp, 0x7f, static_cast<size_t>(ncells) * sizeof(int), st)); // 0x7f7f7f7f: above every draw index
		GPLE_HIP(ctx, hipMemsetAsync(statep, 0, 2 * sizeof(int), st));
		if (!uniform)
		{
			GPLE_HIP(ctx, within.get(ncells));
			GPLE_HIP(ctx, offsets.get(nchunks + 1));
			GPLE_HIP(ctx, count.get(nchunks + 1));
			long long* const countp = reinterpret_cast<long long*>(count.p);
			GPLE_HIP(ctx, launch_recon_scan(st, num_pes, r.p, ncells, q, within.p, offsets.p, countp));
			double W = 0.0;
			long long nonzero = 0;
			GPLE_HIP(ctx, hipMemcpyAsync(&W, offsets.p + nchunks, sizeof(double), hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipMemcpyAsync(&nonzero, countp + nchunks, sizeof(long long), hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			if (!(W > 0.0) || !std::isfinite(W) || nonzero < static_cast<long long>(n_select))
			{
				timer_stop(ctx, GPLE_TIMER_RECON);
				return GPLE_ERR_BAD_ARG; // fewer cells of non-zero weight than points asked for: the draws would never end
			}
		}
		int K = 0;
		unsigned k0 = 0, batch = FIRST_BATCH;
		while (K == 0)
		{
			if (k0 >= MAX_DRAWS)
			{
				timer_stop(ctx, GPLE_TIMER_RECON);
				std::lock_guard<std::mutex> lk(ctx->mu);
				ctx->last_error = "gple_grid_select: 2^30 draws did not reach n_select distinct cells";
				return GPLE_ERR_STATE;
			}
			int hs[2] = {0, 0};
			GPLE_HIP(ctx, launch_recon_draw(st, within.p, offsets.p, ncells, static_cast<int>(nx), static_cast<int>(np), q, uniform != 0, seed, k0, batch, drawp, markp));
			GPLE_HIP(ctx, launch_recon_count(st, drawp, markp, k0, batch, ns, statep, chosenp));
			GPLE_HIP(ctx, hipMemcpyAsync(hs, statep, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			K = hs[1];
			k0 += batch;
			batch = std::min(batch * 2, MAX_BATCH);
		}
		// the set's order (std::set of (ix, ip) pairs, gpr.cpp:223, 282): ascending row-major cell index
		std::vector<int> sel(n_select);
		GPLE_HIP(ctx, hipMemcpyAsync(sel.data(), chosenp, n_select * sizeof(int), hipMemcpyDeviceToHost, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		std::sort(sel.begin(), sel.end());
		GPLE_HIP(ctx, hipMemcpyAsync(chosenp, sel.data(), n_select * sizeof(int), hipMemcpyHostToDevice, st));
		GPLE_HIP(ctx, launch_recon_gather(st, num_pes, r.p, xs.p, static_cast<int>(nx), ps.p, static_cast<int>(np), q, chosenp, ns, co.p, Xo.p, yo.p));
		timer_stop(ctx, GPLE_TIMER_RECON);
		GPLE_HIP(ctx, co.back());
		GPLE_HIP(ctx, Xo.back());
		GPLE_HIP(ctx, yo.back());
		GPLE_HIP(ctx, hipStreamSynchronize(st)); // `sel` is read by the upload
		timer_collect(ctx);
		*n_draws = static_cast<size_t>(K);
		return GPLE_OK;
	}

	int gple_grid_reconstruct(gple_ctx* ctx, int num_pes, int model, const double* rho, const double* x, size_t nx, const double* p, size_t np, double mass,
		double dx, double dp, const gple_recon_plane* planes, const double* scale, unsigned flags, double* pred, double* sums)
	{
		if (!planes || (num_pes != 2 && num_pes != 3)) return GPLE_ERR_BAD_ARG;
		PlaneIn in[RECON_MAX_PLANES];
		for (int q = 0; q < num_pes * num_pes; ++q) in[q] = {planes[q].x, planes[q].X, planes[q].b, planes[q].N};
		return grid_reconstruct(ctx, num_pes, model, rho, x, nx, p, np, mass, dx, dp, in, false, scale, flags, pred, sums);
	}
	int gple_grid_reconstruct_cross(gple_ctx* ctx, int num_pes, int model, const double* rho, const double* x, size_t nx, const double* p, size_t np,
		double mass, double dx, double dp, const gple_recon_cross_plane* planes, const double* scale, unsigned flags, double* pred, double* sums)
	{
		if (!planes || (num_pes != 2 && num_pes != 3)) return GPLE_ERR_BAD_ARG;
		PlaneIn in[RECON_MAX_PLANES];
		for (int q = 0; q < num_pes * num_pes; ++q) in[q] = {planes[q].x, planes[q].X, planes[q].b, planes[q].N};
		return grid_reconstruct(ctx, num_pes, model, rho, x, nx, p, np, mass, dx, dp, in, true, scale, flags, pred, sums);
	}
}
