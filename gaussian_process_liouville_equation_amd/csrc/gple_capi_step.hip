// gple_capi_step.hip — C-ABI entry points of include/gple.h: the device step loop (PES, evolve) and the Markov chains.
#include <algorithm>
#include <cmath>
#include <memory>

#include "gple_capi.h"

extern "C"
{
	// ---- step loop (N3) ----------------------------------------------------------------------------------------------------
	int gple_pes_adiabatic(gple_ctx* ctx, int model, const double* x, size_t M, unsigned flags, double* out)
	{
		if (!ctx || model < 0 || model > 2 || (M && (!x || !out))) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (M == 0) return GPLE_OK;
		GPLE_CALL(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		Staged xd(ctx, dev), od(ctx, dev);
		GPLE_HIP(ctx, xd.in(x, M));
		GPLE_HIP(ctx, od.out(out, 6 * M));
		GPLE_HIP(ctx, launch_pes(ctx->stream, xd.p, (int)M, model, od.p));
		GPLE_HIP(ctx, od.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return GPLE_OK;
	}

	// cut-off prediction of `el` at m device points -> out (m doubles, or m (re,im) pairs); out == nullptr on return means "0"
	static int predict_element_cutoff(gple_ctx* ctx, const gple_element& el, const double* pts_dev, size_t m, double* out_dev)
	{
		if (el.real && el.cplx) return GPLE_ERR_BAD_ARG;
		if (m == 0 || (!el.real && !el.cplx)) return GPLE_OK;
		const FitCommon* f = el.real ? static_cast<const FitCommon*>(el.real) : static_cast<const FitCommon*>(el.cplx);
		// (the points of a tick sit on or next to the sampled density: nothing to prune, and the row statistics would cost a second
		// generation pass)
		return predict_common(ctx, f, pts_dev, m, GPLE_IO_DEVICE | GPLE_PREDICT_FULL, nullptr, nullptr, nullptr, out_dev, nullptr);
	}

	int gple_evolve(gple_ctx* ctx, const gple_element elements[3], int pes_model, double mass, double dt, gple_points density[3], unsigned flags)
	{
		if (!ctx || !elements || !density || pes_model < 0 || pes_model > 2 || !(mass > 0.0)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		int n[3];
		size_t total = 0;
		for (int e = 0; e < 3; ++e)
		{
			if (density[e].n > (1u << 28) || (density[e].n && (!density[e].r || !density[e].rho))) return GPLE_ERR_BAD_ARG;
			n[e] = static_cast<int>(density[e].n);
			total += density[e].n;
		}
		if (total == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		long qoff[3][3], qlen[3];
		int off[3];
		const int new_points = (flags & GPLE_EVOLVE_NEW_POINTS) ? 1 : 0;
		evolve_layout(n, qoff, qlen, off, new_points);
		hipStream_t st = ctx->stream;
		Scratch r_old(ctx), rho_old(ctx), r_new(ctx), rho_new(ctx), cpl(ctx), q0(ctx), q1(ctx), q2(ctx), p0(ctx), p1(ctx), p2(ctx);
		Scratch* q[3] = {&q0, &q1, &q2};
		Scratch* pr[3] = {&p0, &p1, &p2};
		{
			GPLE_CALL(ctx);
			GPLE_HIP(ctx, r_old.get(2 * total));
			GPLE_HIP(ctx, rho_old.get(2 * total));
			GPLE_HIP(ctx, r_new.get(2 * total));
			GPLE_HIP(ctx, rho_new.get(2 * total));
			GPLE_HIP(ctx, cpl.get(total / 8 + 1));
			for (int e = 0; e < 3; ++e)
			{
				GPLE_HIP(ctx, q[e]->get(2 * static_cast<size_t>(qlen[e]) + 2));
				GPLE_HIP(ctx, pr[e]->get(2 * static_cast<size_t>(qlen[e]) + 2));
				// the points of the three elements back to back
				GPLE_HIP(ctx, copy_in(st, r_old.p + 2 * off[e], density[e].r, 2 * density[e].n, dev));
				GPLE_HIP(ctx, copy_in(st, rho_old.p + 2 * off[e], density[e].rho, 2 * density[e].n, dev));
			}
			double* const qp[3] = {q0.p, q1.p, q2.p};
			GPLE_HIP(ctx, launch_evolve_prepare(st, r_old.p, n, mass, dt, pes_model, r_new.p, reinterpret_cast<unsigned char*>(cpl.p), qp, new_points));
		}
		// one batched predict per density-matrix element over everything that was back-propagated into it
		const double* pred[3] = {nullptr, nullptr, nullptr};
		for (int e = 0; e < 3; ++e)
		{
			if (qlen[e] == 0 || (!elements[e].real && !elements[e].cplx)) continue;
			if ((e == 1) != (elements[e].cplx != nullptr)) return GPLE_ERR_BAD_ARG; // (1,0) is the complex element, the diagonal ones are real
			GPLE_TRY(predict_element_cutoff(ctx, elements[e], q[e]->p, static_cast<size_t>(qlen[e]), pr[e]->p));
			pred[e] = pr[e]->p;
		}
		GPLE_CALL(ctx);
		GPLE_HIP(ctx, launch_evolve_combine(st, r_old.p, r_new.p, rho_old.p, reinterpret_cast<const unsigned char*>(cpl.p), n, mass, dt, pes_model, pred, rho_new.p, new_points));
		for (int e = 0; e < 3; ++e)
		{
			GPLE_HIP(ctx, copy_out(st, density[e].r, r_new.p + 2 * off[e], 2 * density[e].n, dev));
			GPLE_HIP(ctx, copy_out(st, density[e].rho, rho_new.p + 2 * off[e], 2 * density[e].n, dev));
		}
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}

	/* N-level form of gple_evolve / gple_pes_adiabatic (gple_evolve_n.hip): num_pes = 2 or 3, NE = num_pes (num_pes + 1) / 2 elements in the
	 * packing order (0,0), (1,0), (1,1), (2,0), (2,1), (2,2) */
	int gple_pes_adiabatic_n(gple_ctx* ctx, int num_pes, int model, const double* x, size_t M, unsigned flags, double* out)
	{
		PesModel pes;
		if (!ctx || !pes_resolve(ctx, num_pes, model, &pes) || (M && (!x || !out)) || M > (1u << 28)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (M == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t width = static_cast<size_t>(num_pes) + 2 * static_cast<size_t>(num_pes * (num_pes + 1) / 2);
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		Staged xd(ctx, dev), od(ctx, dev);
		GPLE_HIP(ctx, xd.in(x, M));
		GPLE_HIP(ctx, od.out(out, width * M));
		GPLE_HIP(ctx, launch_pes_n(ctx->stream, num_pes, xd.p, static_cast<int>(M), pes, od.p));
		GPLE_HIP(ctx, od.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return GPLE_OK;
	}

	/* ---- user potentials: a table of V and dV/dx on a uniform grid, registered on the context under an id >= GPLE_PES_USER ---- */
	int gple_pes_define(gple_ctx* ctx, int num_pes, double x_first, double dx, size_t n, const double* V, const double* dV, unsigned flags, int* model)
	{
		if (!ctx || (num_pes != 2 && num_pes != 3) || n < 2 || n > (size_t(1) << 20) || !std::isfinite(dx) || !(dx > 0.0) || !std::isfinite(x_first) || !V ||
			!dV || !model)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		{
			std::lock_guard<std::mutex> lk(ctx->pes_mu);
			bool room = false;
			for (const auto& slot : ctx->pes) room = room || !slot.table;
			if (!room) return GPLE_ERR_BAD_ARG;
		}
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t entries = n * static_cast<size_t>(num_pes * num_pes);
		hipStream_t st = ctx->stream;
		Staged vs(ctx, dev), ds(ctx, dev);
		Scratch bad(ctx);
		GPLE_HIP(ctx, vs.in(V, entries));
		GPLE_HIP(ctx, ds.in(dV, entries));
		GPLE_HIP(ctx, bad.get(1));
		GPLE_HIP(ctx, hipMemsetAsync(bad.p, 0, sizeof(double), st));
		double* table = nullptr;
		GPLE_HIP(ctx, hipMalloc(&table, PES_TABLE_PLANES * entries * sizeof(double)));
		int found = 0;
		hipError_t e = launch_pes_table_build(st, num_pes, vs.p, ds.p, n, dx, table, reinterpret_cast<int*>(bad.p));
		if (e == hipSuccess) e = hipMemcpyAsync(&found, bad.p, sizeof(int), hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		if (e != hipSuccess || found)
		{
			(void)hipFree(table);
			if (e != hipSuccess) GPLE_HIP(ctx, e);
			return GPLE_ERR_BAD_ARG; // a non-finite entry or an asymmetric matrix
		}
		std::lock_guard<std::mutex> lk(ctx->pes_mu);
		for (int k = 0; k < gple_ctx::PES_SLOTS; ++k)
		{
			gple_ctx::PesSlot& slot = ctx->pes[k];
			if (slot.table) continue;
			slot.table = table, slot.num_pes = num_pes, slot.n = static_cast<int>(n), slot.x_first = x_first, slot.dx = dx;
			*model = GPLE_PES_USER + k;
			return GPLE_OK;
		}
		(void)hipFree(table); // (unreachable: defines hold the call lock, and only they fill slots)
		return GPLE_ERR_BAD_ARG;
	}

	int gple_pes_undefine(gple_ctx* ctx, int model)
	{
		if (!ctx || model < GPLE_PES_USER || model >= GPLE_PES_USER + gple_ctx::PES_SLOTS) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		GPLE_CALL(ctx);
		double* table = nullptr;
		{
			std::lock_guard<std::mutex> lk(ctx->pes_mu);
			gple_ctx::PesSlot& slot = ctx->pes[model - GPLE_PES_USER];
			if (!slot.table) return GPLE_ERR_BAD_ARG;
			table = slot.table;
			slot = gple_ctx::PesSlot();
		}
		GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // enqueued kernels may still read the table
		GPLE_HIP(ctx, hipFree(table));
		return GPLE_OK;
	}

	int gple_pes_diabatic_n(gple_ctx* ctx, int num_pes, int model, const double* x, size_t M, unsigned flags, double* V, double* F)
	{
		PesModel pes;
		if (!ctx || !pes_resolve(ctx, num_pes, model, &pes) || (M && (!x || !V || !F)) || M > (1u << 28)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (M == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const size_t width = static_cast<size_t>(num_pes * num_pes);
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		Staged xd(ctx, dev), vd(ctx, dev), fd(ctx, dev);
		GPLE_HIP(ctx, xd.in(x, M));
		GPLE_HIP(ctx, vd.out(V, width * M));
		GPLE_HIP(ctx, fd.out(F, width * M));
		GPLE_HIP(ctx, launch_pes_diabatic_n(ctx->stream, num_pes, xd.p, static_cast<int>(M), pes, vd.p, fd.p));
		GPLE_HIP(ctx, vd.back());
		GPLE_HIP(ctx, fd.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return GPLE_OK;
	}

	int gple_evolve_n(gple_ctx* ctx, int num_pes, const gple_element* elements, int pes_model, double mass, double dt, gple_points* density, unsigned flags)
	{
		PesModel pes;
		if (!ctx || !elements || !density || !pes_resolve(ctx, num_pes, pes_model, &pes) || !(mass > 0.0)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const int NE = num_pes * (num_pes + 1) / 2;
		int n[6] = {0, 0, 0, 0, 0, 0}, off[6];
		bool diagonal[6];
		size_t total = 0;
		for (int i = 0, e = 0; i < num_pes; ++i)
			for (int j = 0; j <= i; ++j, ++e) diagonal[e] = i == j;
		for (int e = 0; e < NE; ++e)
		{
			if (density[e].n > (1u << 26) || (density[e].n && (!density[e].r || !density[e].rho))) return GPLE_ERR_BAD_ARG;
			if (elements[e].real && elements[e].cplx) return GPLE_ERR_BAD_ARG;
			if ((elements[e].real && !diagonal[e]) || (elements[e].cplx && diagonal[e])) return GPLE_ERR_BAD_ARG; // real GPs on the diagonal, complex ones off it
			n[e] = static_cast<int>(density[e].n), off[e] = static_cast<int>(total);
			total += density[e].n;
		}
		if (total == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		const int new_points = (flags & GPLE_EVOLVE_NEW_POINTS) ? 1 : 0;
		long qlen[6];
		evolve_layout_n(num_pes, n, qlen);
		hipStream_t st = ctx->stream;
		Scratch r_old(ctx), rho_old(ctx), r_new(ctx), rho_new(ctx);
		std::vector<std::unique_ptr<Scratch>> q, pr;
		double* qp[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
		{
			GPLE_CALL(ctx);
			if (!pes_resolve(ctx, num_pes, pes_model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
			GPLE_HIP(ctx, r_old.get(2 * total));
			GPLE_HIP(ctx, rho_old.get(2 * total));
			GPLE_HIP(ctx, r_new.get(2 * total));
			GPLE_HIP(ctx, rho_new.get(2 * total));
			for (int e = 0; e < NE; ++e)
			{
				q.emplace_back(new Scratch(ctx)), pr.emplace_back(new Scratch(ctx));
				GPLE_HIP(ctx, q[e]->get(2 * static_cast<size_t>(qlen[e]) + 2));
				GPLE_HIP(ctx, pr[e]->get(2 * static_cast<size_t>(qlen[e]) + 2));
				qp[e] = q[e]->p;
				GPLE_HIP(ctx, copy_in(st, r_old.p + 2 * off[e], density[e].r, 2 * density[e].n, dev));
				GPLE_HIP(ctx, copy_in(st, rho_old.p + 2 * off[e], density[e].rho, 2 * density[e].n, dev));
			}
			GPLE_HIP(ctx, launch_evolve_prepare_n(st, num_pes, r_old.p, n, mass, dt, pes, r_new.p, qp, new_points));
		}
		// one batched predict per density-matrix element over everything that was back-propagated into it
		const double* pred[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
		for (int e = 0; e < NE; ++e)
		{
			if (qlen[e] == 0 || (!elements[e].real && !elements[e].cplx)) continue;
			GPLE_TRY(predict_element_cutoff(ctx, elements[e], q[e]->p, static_cast<size_t>(qlen[e]), pr[e]->p));
			pred[e] = pr[e]->p;
		}
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, pes_model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		GPLE_HIP(ctx, launch_evolve_combine_n(st, num_pes, r_new.p, rho_old.p, n, mass, dt, pes, pred, rho_new.p, new_points));
		for (int e = 0; e < NE; ++e)
		{
			GPLE_HIP(ctx, copy_out(st, density[e].r, r_new.p + 2 * off[e], 2 * density[e].n, dev));
			GPLE_HIP(ctx, copy_out(st, density[e].rho, rho_new.p + 2 * off[e], 2 * density[e].n, dev));
		}
		GPLE_HIP(ctx, hipStreamSynchronize(st)); // the scratch lists go back to the pool when this returns
		return GPLE_OK;
	}

	static int markov_chain_impl(gple_ctx* ctx, const gple_element* element, size_t num_steps, double max_displacement, unsigned long long seed, double* r,
		size_t n, double* accept_ratio, double* chain)
	{
		if (!ctx || !element || (n && !r) || n > (1u << 28) || (element->real && element->cplx)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		if (n == 0) return GPLE_OK;
		hipStream_t st = ctx->stream;
		const int ni = static_cast<int>(n), cplx = element->cplx ? 1 : 0;
		const bool has_fit = element->real || element->cplx;
		Scratch rd(ctx), rp(ctx), pred(ctx), weight(ctx), acc(ctx), trace(ctx);
		{
			GPLE_CALL(ctx);
			if (chain) GPLE_HIP(ctx, trace.get((num_steps + 1) * 2 * n)); // the whole chains, [step][walker][2]
			GPLE_HIP(ctx, rd.get(2 * n));
			GPLE_HIP(ctx, rp.get(2 * n));
			GPLE_HIP(ctx, pred.get(2 * n));
			GPLE_HIP(ctx, weight.get(n));
			GPLE_HIP(ctx, acc.get(n / 2 + 1));
			GPLE_HIP(ctx, copy_in(st, rd.p, r, 2 * n, false));
			GPLE_HIP(ctx, hipMemsetAsync(acc.p, 0, (n / 2 + 1) * 8, st));
			if (chain) GPLE_HIP(ctx, hipMemcpyAsync(trace.p, rd.p, 2 * n * 8, hipMemcpyDeviceToDevice, st));
		}
		GPLE_TRY(predict_element_cutoff(ctx, *element, rd.p, n, pred.p));
		{
			std::lock_guard<std::mutex> lk(ctx->call_mu);
			GPLE_HIP(ctx, launch_mc_weight(st, has_fit ? pred.p : nullptr, cplx, ni, weight.p)); // mc.cpp:131
		}
		for (size_t step = 0; step < num_steps; ++step)
		{
			{
				std::lock_guard<std::mutex> lk(ctx->call_mu);
				GPLE_HIP(ctx, launch_mc_propose(st, rd.p, ni, static_cast<unsigned>(step), seed, max_displacement, rp.p));
			}
			GPLE_TRY(predict_element_cutoff(ctx, *element, rp.p, n, pred.p));
			std::lock_guard<std::mutex> lk(ctx->call_mu);
			GPLE_HIP(ctx, launch_mc_accept(st, rd.p, rp.p, has_fit ? pred.p : nullptr, cplx, ni, static_cast<unsigned>(step), seed, weight.p,
							  reinterpret_cast<unsigned*>(acc.p)));
			if (chain) GPLE_HIP(ctx, hipMemcpyAsync(trace.p + (step + 1) * 2 * n, rd.p, 2 * n * 8, hipMemcpyDeviceToDevice, st));
		}
		std::lock_guard<std::mutex> lk(ctx->call_mu);
		GPLE_HIP(ctx, copy_out(st, r, rd.p, 2 * n, false));
		if (chain) GPLE_HIP(ctx, copy_out(st, chain, trace.p, (num_steps + 1) * 2 * n, false));
		std::vector<unsigned> counts(accept_ratio ? n : 0);
		if (accept_ratio) GPLE_HIP(ctx, hipMemcpyAsync(counts.data(), acc.p, n * sizeof(unsigned), hipMemcpyDeviceToHost, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		if (accept_ratio)
			for (size_t i = 0; i < n; ++i) accept_ratio[i] = num_steps ? static_cast<double>(counts[i]) / static_cast<double>(num_steps) : 0.0;
		return GPLE_OK;
	}

	int gple_markov_chain(gple_ctx* ctx, const gple_element* element, size_t num_steps, double max_displacement, unsigned long long seed, double* r,
		size_t n, double* accept_ratio)
	{
		return markov_chain_impl(ctx, element, num_steps, max_displacement, seed, r, n, accept_ratio, nullptr);
	}
	int gple_markov_chain_trace(gple_ctx* ctx, const gple_element* element, size_t num_steps, double max_displacement, unsigned long long seed,
		double* r, size_t n, double* accept_ratio, double* chain)
	{
		if (!chain) return GPLE_ERR_BAD_ARG;
		return markov_chain_impl(ctx, element, num_steps, max_displacement, seed, r, n, accept_ratio, chain);
	}
}
