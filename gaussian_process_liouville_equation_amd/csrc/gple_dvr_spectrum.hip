// gple_dvr_spectrum.hip — the energy-resolved channel spectrum of one absorbing DVR run (gple_dvr_spectrum; DESIGN.md §11, "The spectrum of one
// packet").  With P = P4(A) the one-step propagator of gple_dvr_power.hip, psi_k = P^k psi0, theta = E dt / hbar and K = 2^J,
//   Y(E) = sum_{k < K} e^{i theta k} psi_k = prod_{j < J} (I + e^{i theta 2^j} P^(2^j)) psi0,
// one column per energy, by the power's own squarings: R = P; per level T = Y o e^{i theta 2^j}, Y += R T, R = R R.  Nothing steps.
//
//   dvr_spectrum_start_kernel    every column of Y = psi0, in the padded two-plane layout (ld x nep per plane, column-major, nep = n_E rounded up to
//                                64; zero beyond dim and beyond n_E); WIDE = false: psi0 in column 0 of 64 (what is left: P^K psi0 as one thin product)
//   dvr_spectrum_phase_kernel    T = Y o e^{i theta 2^j}: theta 2^j is exact (a scaling by a power of two), the phase is sincos of that product,
//                                never a squared z; padding written as exact zeros
//   dvr_complex_product          Y += R T, P^K psi0 and P X: the power's four real products on full tiles and fewer columns, beta = 1 (0 for the
//                                last two); T's planes lie ld nep apart, those of Y and P X a whole X plane
//   dvr_spectrum_project_kernel  Q_c = Pi_c Y for every channel c = (side, adiabatic surface) at once: block diagonal in x, a mix of num_pes rows with
//                                `basis`, the operation order of dvr_channel_kernel's mix
//   dvr_spectrum_reduce_kernel   a_c(E) = Re[Q_c^H Y - (P Q_c)^H (P Y)] per (energy, channel): thread-strided sums in ascending order and a fixed
//                                tree; no floating-point atomics, no flags between workgroups.  The same kernel sums |P^K psi0|^2
//   dvr_spectrum_export_kernel   the columns of Y as the caller's n_E x dim (re, im) pairs
#include "gple_dvr_device.h"
#include "gple_kernels.h"

namespace gple
{
	namespace
	{
		using namespace dvr;

		// Y(r, e) = psi0[r] for r < dim, e < n_E (WIDE) or e == 0 (!WIDE); zero elsewhere.  blockIdx.y = e < columns
		template <bool WIDE>
		__global__ void __launch_bounds__(256) dvr_spectrum_start_kernel(const double* __restrict__ psi0, int dim, long ld, int n_E, double* __restrict__ Yr,
			double* __restrict__ Yi)
		{
			const long r = blockIdx.x * 256L + threadIdx.x, e = blockIdx.y;
			if (r >= ld) return;
			const bool in = r < dim && (WIDE ? e < n_E : e == 0);
			const d2 v = in ? *reinterpret_cast<const d2*>(psi0 + 2 * r) : (d2){0.0, 0.0};
			Yr[r + e * ld] = v.x;
			Yi[r + e * ld] = v.y;
		}

		// T(r, e) = Y(r, e) (cos t + i sin t), t = (E_e dt / hbar) scale with scale = 2^j
		__global__ void __launch_bounds__(256) dvr_spectrum_phase_kernel(const double* __restrict__ Yr, const double* __restrict__ Yi,
			const double* __restrict__ energies, double dt, double scale, int dim, long ld, int n_E, double* __restrict__ Tr, double* __restrict__ Ti)
		{
#pragma clang fp contract(off)
			const long r = blockIdx.x * 256L + threadIdx.x, e = blockIdx.y;
			if (r >= ld) return;
			double re = 0.0, im = 0.0;
			if (r < dim && e < n_E)
			{
				const double theta = energies[e] * dt / HBAR_D;
				double sn, cs;
				sincos(theta * scale, &sn, &cs);
				const double a = Yr[r + e * ld], b = Yi[r + e * ld];
				re = a * cs - b * sn;
				im = a * sn + b * cs;
			}
			Tr[r + e * ld] = re;
			Ti[r + e * ld] = im;
		}

		// Q_c((m, a), e) = [a on side] sum_j (b(a; m, k) b(a; j, k)) Y((j, a), e) for c = side NP + k = blockIdx.z; Q_c follows Y at (1 + c) nep columns
		template <int NP>
		__global__ void __launch_bounds__(256) dvr_spectrum_project_kernel(double* __restrict__ Xr, double* __restrict__ Xi, const double* __restrict__ basis,
			int n, int n_left, long ld, int n_E, long nep)
		{
#pragma clang fp contract(off)
			const long r = blockIdx.x * 256L + threadIdx.x, e = blockIdx.y;
			const int c = blockIdx.z, side = c / NP, k = c % NP;
			if (r >= ld) return;
			double re = 0.0, im = 0.0;
			if (r < static_cast<long>(NP) * n && e < n_E)
			{
				const int m = static_cast<int>(r / n), a = static_cast<int>(r % n);
				if ((a < n_left) == (side == 0)) projector_mix<NP>(basis + static_cast<long>(a) * NP * NP, m, k, Xr, Xi, a + e * ld, n, re, im);
			}
			const long to = r + ((1 + c) * nep + e) * ld;
			Xr[to] = re;
			Xi[to] = im;
		}

		// out[e C + c] = sum_{r < dim} Re conj(Q_c(r, e)) Y(r, e) - Re conj((P Q_c)(r, e)) (P Y)(r, e): thread i sums the rows i, i + 256, ... in
		// ascending order, then a fixed tree.  DIFF = false: out[0] = sum_r |X(r, 0)|^2 of the first plane pair alone (C = 1, one block)
		template <bool DIFF>
		__global__ void __launch_bounds__(256) dvr_spectrum_reduce_kernel(const double* __restrict__ X, const double* __restrict__ PX, int dim, long ld, long nep,
			int C, double* __restrict__ out)
		{
#pragma clang fp contract(off)
			const long e = blockIdx.x / C, c = blockIdx.x % C, plane = ld * (1 + C) * nep;
			const long y = e * ld, q = DIFF ? ((1 + c) * nep + e) * ld : y;
			double acc = 0.0;
			for (int r = threadIdx.x; r < dim; r += 256)
			{
				double term = X[q + r] * X[y + r] + X[plane + q + r] * X[plane + y + r];
				if (DIFF) term -= PX[q + r] * PX[y + r] + PX[plane + q + r] * PX[plane + y + r];
				acc += term;
			}
			const double sum = block_sum_256(acc);
			if (threadIdx.x == 0) out[blockIdx.x] = sum;
		}

		// psi_e[e][r] = (Yr, Yi)(r, e); blockIdx.y = e < n_E
		__global__ void __launch_bounds__(256) dvr_spectrum_export_kernel(const double* __restrict__ Yr, const double* __restrict__ Yi, int dim, long ld,
			double* __restrict__ out)
		{
			const long r = blockIdx.x * 256L + threadIdx.x, e = blockIdx.y;
			if (r >= dim) return;
			*reinterpret_cast<d2*>(out + 2 * (e * dim + r)) = (d2){Yr[r + e * ld], Yi[r + e * ld]};
		}

		hipError_t run(hipStream_t s, const DvrSpectrum& g)
		{
			const int dim = g.num_pes * g.n, C = 2 * g.num_pes;
			const long ld = static_cast<long>(round_up(dim, 64));
			const DvrPowerWork pw = dvr_power_layout(g.power_work, ld); // P4 stays in pw.P, the squarings take pw.buf in turn
			const long nep = static_cast<long>(round_up(g.n_E, 64)), cols = (1 + C) * nep;
			DvrCarve work{g.work};
			const DvrPlanes X = work.planes(ld * cols);  // Y | Q_0 .. Q_{C-1}: ld x cols per plane
			const DvrPlanes PX = work.planes(ld * cols); // P X, the same layout
			const DvrPlanes T = work.planes(ld * nep);   // ld x nep per plane
			const unsigned rows = static_cast<unsigned>((ld + 255) / 256);
			const dim3 block(256), wide(rows, static_cast<unsigned>(nep));
			hipError_t err;
			if ((err = launch_dvr_p4(s, g.num_pes, g.n, g.H, g.W, g.dt, pw)) != hipSuccess) return err;
			hipLaunchKernelGGL(dvr_spectrum_start_kernel<true>, wide, block, 0, s, g.psi0, dim, ld, g.n_E, X.re, X.im);
			if ((err = hipGetLastError()) != hipSuccess) return err;
			DvrPlanes R = pw.P;
			int next = 0;
			auto square = [&]() -> hipError_t { // R = R R
				const DvrPlanes Z = pw.buf[next];
				next ^= 1;
				const hipError_t e = launch_dvr_square(s, R, Z, ld);
				R = Z;
				return e;
			};
			double scale = 1.0;
			for (int j = 0; j < g.levels; ++j, scale *= 2.0)
			{
				if (j > 0 && (err = square()) != hipSuccess) return err;
				hipLaunchKernelGGL(dvr_spectrum_phase_kernel, wide, block, 0, s, X.re, X.im, g.energies, g.dt, scale, dim, ld, g.n_E, T.re, T.im);
				if ((err = hipGetLastError()) != hipSuccess) return err;
				if ((err = dvr_complex_product(s, R, T, X, ld, nep, 1.0, false, false)) != hipSuccess) return err; // Y += R T
			}
			if (g.remaining) // |P^K psi0|^2: the last squaring, one product of 64 columns, the reduction's sum
			{
				if (g.levels > 0 && (err = square()) != hipSuccess) return err;
				hipLaunchKernelGGL(dvr_spectrum_start_kernel<false>, dim3(rows, 64), block, 0, s, g.psi0, dim, ld, 1, T.re, T.im);
				if ((err = hipGetLastError()) != hipSuccess) return err;
				if ((err = dvr_complex_product(s, R, T, PX, ld, 64, 0.0, false, false)) != hipSuccess) return err;
				hipLaunchKernelGGL(dvr_spectrum_reduce_kernel<false>, dim3(1), block, 0, s, PX.re, PX.re, dim, ld, nep, C, g.remaining);
				if ((err = hipGetLastError()) != hipSuccess) return err;
			}
			const dim3 pgrid(rows, static_cast<unsigned>(nep), static_cast<unsigned>(C));
			const auto project = g.num_pes == 2 ? dvr_spectrum_project_kernel<2> : dvr_spectrum_project_kernel<3>;
			hipLaunchKernelGGL(project, pgrid, block, 0, s, X.re, X.im, g.basis, g.n, g.n_left, ld, g.n_E, nep);
			if ((err = hipGetLastError()) != hipSuccess) return err;
			if ((err = dvr_complex_product(s, pw.P, X, PX, ld, cols, 0.0, false, false)) != hipSuccess) return err;
			hipLaunchKernelGGL(dvr_spectrum_reduce_kernel<true>, dim3(static_cast<unsigned>(g.n_E * C)), block, 0, s, X.re, PX.re, dim, ld, nep, C, g.density);
			if ((err = hipGetLastError()) != hipSuccess) return err;
			if (g.psi_e)
				hipLaunchKernelGGL(dvr_spectrum_export_kernel, dim3((dim + 255) / 256, static_cast<unsigned>(g.n_E)), block, 0, s, X.re, X.im, dim, ld, g.psi_e);
			return hipGetLastError();
		}
	} // namespace

	size_t dvr_spectrum_work_doubles(int num_pes, int n, int n_E)
	{
		const size_t ld = round_up(static_cast<size_t>(num_pes) * n, 64), nep = round_up(static_cast<size_t>(n_E), 64);
		return (4 * (1 + 2 * static_cast<size_t>(num_pes)) + 2) * ld * nep; // X and P X (two planes of ld x (1 + 2 num_pes) nep each), T (two of ld x nep)
	}

	hipError_t launch_dvr_spectrum(Ctx* ctx, hipStream_t s, const DvrSpectrum& g)
	{
		if ((g.num_pes != 2 && g.num_pes != 3) || g.levels < 0 || g.levels > 30 || g.n_E < 1) return hipErrorInvalidValue;
		if (ctx) timer_start(ctx, GPLE_TIMER_DVR_SPECTRUM);
		const hipError_t err = run(s, g);
		if (ctx) timer_stop(ctx, GPLE_TIMER_DVR_SPECTRUM); // on the error path too: no span stays open
		return err;
	}
} // namespace gple
