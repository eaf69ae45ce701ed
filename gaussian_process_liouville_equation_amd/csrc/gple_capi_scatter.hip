// gple_capi_scatter.hip — C-ABI entry point of include/gple.h: the coupled-channel scattering solver of gple_scatter.hip.
#include <algorithm>
#include <cmath>

#include "gple_capi.h"

extern "C"
{
	int gple_scatter(gple_ctx* ctx, int num_pes, int model, double mass, double x_left, double x_right, size_t n_steps, size_t n_energies,
		const double* energies, unsigned flags, double* prob, double* defect)
	{
		PesModel pes;
		if (!ctx || !pes_resolve(ctx, num_pes, model, &pes) || n_energies == 0 || n_energies > (size_t(1) << 20) || n_steps < 2 || n_steps > (size_t(1) << 24) ||
			!std::isfinite(mass) || !(mass > 0.0) || !std::isfinite(x_left) || !std::isfinite(x_right) || !(x_left < x_right) || !energies || !prob)
			return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		const bool dev = flags & GPLE_IO_DEVICE;
		const long N = static_cast<long>(n_steps);
		GPLE_CALL(ctx);
		if (!pes_resolve(ctx, num_pes, model, &pes)) return GPLE_ERR_BAD_ARG; // under the call lock, which gple_pes_undefine takes: the table outlives the enqueue
		hipStream_t st = ctx->stream;
		double e_max = 0.0;
		{ // every energy finite, and the largest: device energies are looked at on the host first (n_energies <= 2^20 values)
			std::vector<double> seen;
			const double* e = energies;
			if (dev)
			{
				seen.resize(n_energies);
				GPLE_HIP(ctx, hipMemcpyAsync(seen.data(), energies, n_energies * sizeof(double), hipMemcpyDeviceToHost, st));
				GPLE_HIP(ctx, hipStreamSynchronize(st));
				e = seen.data();
			}
			for (size_t k = 0; k < n_energies; ++k)
				if (!std::isfinite(e[k])) return GPLE_ERR_BAD_ARG;
			e_max = *std::max_element(e, e + n_energies);
		}
		Scratch table(ctx);
		Staged en(ctx, dev), pr(ctx, dev), df(ctx, dev);
		// every allocation before the first launch: one that does not fit leaves the outputs untouched
		const size_t doubles = scatter_table_doubles(num_pes, N);
		GPLE_HIP(ctx, table.get(doubles));
		GPLE_HIP(ctx, pr.out(prob, n_energies * 2 * num_pes * num_pes));
		GPLE_HIP(ctx, df.out(defect, n_energies * num_pes));
		GPLE_HIP(ctx, en.in(energies, n_energies));
		GPLE_HIP(ctx, launch_scatter_table(st, num_pes, pes, x_left, x_right, N, table.p));
		// a grid too coarse for an end channel: c (E_max - eps_min) >= 1/2, eps_min the lowest eigenvalue of either end (the first of each ascending triple)
		double eps[6];
		GPLE_HIP(ctx, hipMemcpyAsync(eps, table.p + (doubles - 2 * num_pes), 2 * num_pes * sizeof(double), hipMemcpyDeviceToHost, st));
		GPLE_HIP(ctx, hipStreamSynchronize(st));
		const double c = scatter_step_constant(mass, x_left, x_right, N);
		if (!(c * (e_max - std::min(eps[0], eps[num_pes])) < 0.5)) return GPLE_ERR_BAD_ARG;
		timer_start(ctx, GPLE_TIMER_SCATTER);
		const hipError_t launched = launch_scatter(st, num_pes, c, N, table.p, en.p, static_cast<long>(n_energies), pr.p, df.p);
		timer_stop(ctx, GPLE_TIMER_SCATTER); // on the error path too: no span stays open
		GPLE_HIP(ctx, launched);
		GPLE_HIP(ctx, pr.back());
		GPLE_HIP(ctx, df.back());
		if (!dev) GPLE_HIP(ctx, hipStreamSynchronize(st));
		return GPLE_OK;
	}
}
