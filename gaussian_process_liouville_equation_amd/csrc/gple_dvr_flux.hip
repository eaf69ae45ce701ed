// gple_dvr_flux.hip — what the absorber of the exact DVR dynamics took (gple_dvr_flux, gple_dvr_flux_apply): per channel
// c = (side of the box, adiabatic surface) the Hermitian G_c with psi^H G_c psi = the population channel c absorbs over s steps, by the recurrence
// of the power's own walk (launch_dvr_power of gple_dvr_power.hip calls the three dvr_flux_* steps; nothing steps).
//
//   dvr_loss_kernel         L = I - conj(P) P from the Hermitian product conj(P) P (the loss of one step).
//   dvr_channel_kernel      D_c = (Pi_c L + L Pi_c) / 2: Pi_c is num_pes x num_pes per grid point, a mix of num_pes rows and num_pes columns.
//   sandwich                G_c += conj(R) (X R): T = X R on full tiles, conj(R) T on the lower tiles (dvr_complex_product twice), then the
//                           Hermitian mirror (upper Re copied, upper Im negated, Im diagonal exactly 0).
//   dvr_flux_export_kernel  the padded column-major G_c as the caller's row-major planes (G(r, q) = conj G(q, r): contiguous both sides).
//   dvr_flux_rows_kernel    psi_r^* (G_c psi)_r for four states at a time, a wave per row, the reduction of dvr_apply_kernel;
//   dvr_flux_sum_kernel     the rows summed per (state, channel) in a fixed order.  No atomics, no flags.
#include <algorithm>

#include "gple_dvr_device.h"
#include "gple_kernels.h"

namespace gple
{
	namespace
	{
		using namespace dvr;

		// Z = conj(P) P (its lower tiles) -> L = I - Z, zero beyond dim (Z is zero there: P is zero padded); the Hermitian mirror follows
		__global__ void __launch_bounds__(256) dvr_loss_kernel(double* __restrict__ Lr, double* __restrict__ Li, int dim, long ld)
		{
			const long r = blockIdx.x * 256L + threadIdx.x, c = blockIdx.y;
			if (r >= ld) return;
			Lr[r + c * ld] = ((r == c && r < dim) ? 1.0 : 0.0) - Lr[r + c * ld];
			Li[r + c * ld] = -Li[r + c * ld];
		}

		// D_c = (Pi_c L + L Pi_c) / 2 for the channel (side, k), Pi_c[(m, a), (m', a)] = [a on side] basis(a; m, k) basis(a; m', k):
		//   (Pi_c L)(r, c) = [a on side] b(a; m, k) sum_j b(a; j, k) L((j, a), c),   (L Pi_c)(r, c) = [a' on side] sum_j L(r, (j, a')) b(a'; j, k) b(a'; m', k)
		// for r = (m, a), c = (m', a'); zero beyond dim
		template <int NP>
		__global__ void __launch_bounds__(256) dvr_channel_kernel(const double* __restrict__ Lr, const double* __restrict__ Li, const double* __restrict__ basis,
			int n, int n_left, int side, int k, long ld, double* __restrict__ Dr, double* __restrict__ Di)
		{
#pragma clang fp contract(off)
			const long r = blockIdx.x * 256L + threadIdx.x, c = blockIdx.y;
			if (r >= ld) return;
			double re = 0.0, im = 0.0;
			if (r < static_cast<long>(NP) * n && c < static_cast<long>(NP) * n)
			{
				const int m = static_cast<int>(r / n), a = static_cast<int>(r % n), mp = static_cast<int>(c / n), ap = static_cast<int>(c % n);
				if ((a < n_left) == (side == 0)) projector_mix<NP>(basis + static_cast<long>(a) * NP * NP, m, k, Lr, Li, a + c * ld, n, re, im);
				if ((ap < n_left) == (side == 0)) projector_mix<NP>(basis + static_cast<long>(ap) * NP * NP, mp, k, Lr, Li, r + ap * ld, n * ld, re, im);
				re *= 0.5, im *= 0.5;
			}
			Dr[r + c * ld] = re;
			Di[r + c * ld] = im;
		}

		// out(r, q) at r dim + q from the column-major padded plane: G(r, q) = conj G(q, r) reads along column r.  blockIdx.y = r, blockIdx.z = plane
		__global__ void __launch_bounds__(256) dvr_flux_export_kernel(const double* __restrict__ Gr, const double* __restrict__ Gi, int dim, long ld,
			double* __restrict__ out)
		{
			const long q = blockIdx.x * 256L + threadIdx.x, r = blockIdx.y;
			if (q >= dim) return;
			if (blockIdx.z == 0) out[r * dim + q] = Gr[q + r * ld];
			else out[static_cast<long>(dim) * dim + r * dim + q] = q == r ? 0.0 : -Gi[q + r * ld];
		}

		// partial[(t C + c) dim + row] = Re conj(psi_t[row]) (G_c psi_t)[row] for the states t < T of one pass (T <= DVR_FLUX_CHUNK), four states per
		// sweep of the row; a sweep past the last state repeats it and writes nothing, so a state's operations do not depend on T or on its place
		constexpr int FLUX_GROUP = 4;
		__global__ void __launch_bounds__(256) dvr_flux_rows_kernel(const double* __restrict__ G, int dim, const double* __restrict__ psi, int T,
			double* __restrict__ partial)
		{
#pragma clang fp contract(off)
			const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), c = blockIdx.y, C = gridDim.y;
			if (row >= dim) return;
			const long plane = static_cast<long>(dim) * dim;
			const double* __restrict__ gr = G + 2 * c * plane + static_cast<long>(row) * dim;
			const double* __restrict__ gi = gr + plane;
			for (int t0 = 0; t0 < T; t0 += FLUX_GROUP)
			{
				const double* v[FLUX_GROUP];
				double re[FLUX_GROUP], im[FLUX_GROUP];
#pragma unroll
				for (int g = 0; g < FLUX_GROUP; ++g) v[g] = psi + 2L * dim * min(t0 + g, T - 1), re[g] = im[g] = 0.0;
				for (int q = lane; q < dim; q += 64)
				{
					const double a = gr[q], b = gi[q];
#pragma unroll
					for (int g = 0; g < FLUX_GROUP; ++g)
					{
						const d2 u = *reinterpret_cast<const d2*>(v[g] + 2L * q);
						re[g] += a * u.x - b * u.y;
						im[g] += a * u.y + b * u.x;
					}
				}
#pragma unroll
				for (int g = 0; g < FLUX_GROUP; ++g)
				{
					wave_sum(re[g], im[g]);
					if (lane == 0 && t0 + g < T)
					{
						const d2 w = *reinterpret_cast<const d2*>(v[g] + 2L * row);
						partial[(static_cast<long>(t0 + g) * C + c) * dim + row] = w.x * re[g] + w.y * im[g];
					}
				}
			}
		}
		// absorbed[b] = sum_row partial[b dim + row]: thread i sums the rows i, i + 256, ... in ascending order, then a fixed tree
		__global__ void __launch_bounds__(256) dvr_flux_sum_kernel(const double* __restrict__ partial, int dim, double* __restrict__ absorbed)
		{
#pragma clang fp contract(off)
			const double* p = partial + static_cast<long>(blockIdx.x) * dim;
			double acc = 0.0;
			for (int r = threadIdx.x; r < dim; r += 256) acc += p[r];
			const double sum = block_sum_256(acc);
			if (threadIdx.x == 0) absorbed[blockIdx.x] = sum;
		}

		// D_c = (Pi_c L + L Pi_c) / 2 into D
		hipError_t channel(const DvrFluxRun& f, int c, DvrPlanes D)
		{
			const auto kernel = f.num_pes == 2 ? dvr_channel_kernel<2> : dvr_channel_kernel<3>;
			hipLaunchKernelGGL(kernel, dvr_plane_grid(f.ld), dim3(256), 0, f.s, f.w.L.re, f.w.L.im, f.flux->basis, f.n, f.flux->n_left, c / f.num_pes, c % f.num_pes,
				f.ld, D.re, D.im);
			const hipError_t err = hipGetLastError();
			return err != hipSuccess ? err : launch_dvr_mirror(f.s, D, f.ld, true);
		}
		// G += conj(R) (X R), R symmetric: T = X R on full tiles, conj(R) T on the lower ones, the Hermitian mirror
		hipError_t sandwich(const DvrFluxRun& f, DvrPlanes X, DvrPlanes R, DvrPlanes G)
		{
			hipError_t err;
			if ((err = dvr_complex_product(f.s, X, R, f.w.T, f.ld, f.ld, 0.0, false, false)) != hipSuccess) return err;
			if ((err = dvr_complex_product(f.s, R, f.w.T, G, f.ld, f.ld, 1.0, true, true)) != hipSuccess) return err;
			return launch_dvr_mirror(f.s, G, f.ld, true);
		}
	} // namespace

	DvrFluxWork dvr_flux_layout(double* work, long ld, int num_pes)
	{
		const size_t plane = static_cast<size_t>(ld) * ld;
		DvrCarve c{work};
		DvrFluxWork w{};
		w.L = c.planes(plane);
		w.D = c.planes(plane);
		w.T = c.planes(plane);
		for (int ch = 0; ch < 2 * num_pes; ++ch) w.G_c[ch] = c.planes(plane);
		w.doubles = c.used;
		return w;
	}
	size_t dvr_flux_work_doubles(int num_pes, int n)
	{
		return dvr_flux_layout(nullptr, static_cast<long>(round_up(static_cast<size_t>(num_pes) * n, 64)), num_pes).doubles;
	}

	hipError_t dvr_flux_first_step(const DvrFluxRun& f, DvrPlanes P)
	{
		if (!f.flux) return hipSuccess;
		hipError_t err;
		if ((err = dvr_complex_product(f.s, P, P, f.w.L, f.ld, f.ld, 0.0, true, true)) != hipSuccess) return err;
		hipLaunchKernelGGL(dvr_loss_kernel, dvr_plane_grid(f.ld), dim3(256), 0, f.s, f.w.L.re, f.w.L.im, f.num_pes * f.n, f.ld);
		if ((err = hipGetLastError()) != hipSuccess) return err;
		if ((err = launch_dvr_mirror(f.s, f.w.L, f.ld, true)) != hipSuccess) return err;
		for (int c = 0; c < 2 * f.num_pes; ++c)
			if ((err = channel(f, c, f.w.G_c[c])) != hipSuccess) return err;
		return hipSuccess;
	}
	hipError_t dvr_flux_before_square(const DvrFluxRun& f, DvrPlanes R)
	{
		if (!f.flux) return hipSuccess;
		hipError_t err;
		for (int c = 0; c < 2 * f.num_pes; ++c)
			if ((err = sandwich(f, f.w.G_c[c], R, f.w.G_c[c])) != hipSuccess) return err;
		return hipSuccess;
	}
	hipError_t dvr_flux_before_multiply(const DvrFluxRun& f, DvrPlanes R)
	{
		if (!f.flux) return hipSuccess;
		hipError_t err;
		for (int c = 0; c < 2 * f.num_pes; ++c)
		{
			if ((err = channel(f, c, f.w.D)) != hipSuccess) return err;
			if ((err = sandwich(f, f.w.D, R, f.w.G_c[c])) != hipSuccess) return err;
		}
		return hipSuccess;
	}

	hipError_t launch_dvr_flux_export(hipStream_t s, int num_pes, int n, const DvrFlux& flux, double* out)
	{
		const int dim = num_pes * n;
		const long ld = static_cast<long>(round_up(dim, 64));
		const DvrFluxWork w = dvr_flux_layout(flux.work, ld, num_pes);
		const dim3 grid((dim + 255) / 256, dim, 2);
		for (int c = 0; c < 2 * num_pes; ++c)
			hipLaunchKernelGGL(dvr_flux_export_kernel, grid, dim3(256), 0, s, w.G_c[c].re, w.G_c[c].im, dim, ld, out + 2L * c * dim * dim);
		return hipGetLastError();
	}
	size_t dvr_flux_apply_work_doubles(int num_pes, int n, int T)
	{
		return static_cast<size_t>(std::min(T, DVR_FLUX_CHUNK)) * 2 * num_pes * num_pes * n;
	}
	hipError_t launch_dvr_flux_apply(hipStream_t s, int num_pes, int n, const double* G, const double* psi, int T, double* partial, double* absorbed)
	{
		if (num_pes != 2 && num_pes != 3) return hipErrorInvalidValue;
		const int dim = num_pes * n, C = 2 * num_pes;
		for (int t0 = 0; t0 < T; t0 += DVR_FLUX_CHUNK) // the launches of a stream are ordered, so the chunks share `partial`
		{
			const int count = std::min(DVR_FLUX_CHUNK, T - t0);
			hipLaunchKernelGGL(dvr_flux_rows_kernel, dim3((dim + 3) / 4, C), dim3(256), 0, s, G, dim, psi + 2L * dim * t0, count, partial);
			hipLaunchKernelGGL(dvr_flux_sum_kernel, dim3(count * C), dim3(256), 0, s, partial, dim, absorbed + static_cast<long>(t0) * C);
		}
		return hipGetLastError();
	}
} // namespace gple
