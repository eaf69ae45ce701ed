// gple_mqcl_absorb.hip — the absorbing boundary of the exact MQCLE run ("The absorbing boundary"): the half-mask
// M: rho(x_i, .) <- (1 - g_i) rho(x_i, .) on the rows of the absorber, with what it removes booked per side of the box, adiabatic surface and
// momentum index.  gple_mqcl.hip's kernels are not touched: a block of Trotter steps runs between two masks through launch_mqcl_evolve.
//
//   State: the num_pes^2 x n x n phase.txt layout of gple_mqcl.hip (element (a, b) row-major, x major, p fastest), diabatic.
//   mqcl_absorb_rows_kernel   the ascending list of the rows with g_i != 0, once per call (one workgroup; the host knows their number).
//   mqcl_absorb_mask_kernel   one workgroup per listed row: the adiabatic diagonal sum_cd C_ca rho_cd C_da of every column from the upper planes
//                             (C from gple_pes_n.h at x_i), g_i times it into the slab [row][a][j], then every stored double of the row, all
//                             num_pes^2 planes, times 1 - g_i: one rounded difference per row and one rounded product per double, no fma, so the
//                             state is (1.0 - g) * rho of the host to the bit and stays exactly Hermitian with exactly real diagonals.
//   mqcl_absorb_fold_kernel   per (a, j): the slab's rows added in ascending order, rows i < n_left to side 0 and the others to side 1, and
//                             each sum added to the caller's accumulator [side][a][j] with one addition.  No atomics: the same bits every call.
#include "gple_kernels.h"
#include "gple_pes_n.h"

namespace gple
{
	namespace
	{
		__global__ void __launch_bounds__(256) mqcl_absorb_rows_kernel(const double* __restrict__ g, int n, int* __restrict__ rows)
		{
			__shared__ int seen[256];
			const int per = (n + 255) / 256, lo = min(n, static_cast<int>(threadIdx.x) * per), hi = min(n, lo + per);
			int mine = 0;
			for (int i = lo; i < hi; ++i) mine += g[i] != 0.0;
			seen[threadIdx.x] = mine;
			__syncthreads();
			for (int off = 1; off < 256; off <<= 1)
			{
				const int before = static_cast<int>(threadIdx.x) >= off ? seen[threadIdx.x - off] : 0;
				__syncthreads();
				seen[threadIdx.x] += before;
				__syncthreads();
			}
			int at = seen[threadIdx.x] - mine; // the listed rows below lo
			for (int i = lo; i < hi; ++i)
				if (g[i] != 0.0) rows[at++] = i;
		}

		template <int NP, typename PES>
		__global__ void __launch_bounds__(256) mqcl_absorb_mask_kernel(PES model, const double* __restrict__ x, const double* __restrict__ g,
			const int* __restrict__ rows, int n, double2* __restrict__ rho, double* __restrict__ slab)
		{
#pragma clang fp contract(off)
			__shared__ double Cs[NP][NP];
			const int i = rows[blockIdx.x];
			if (threadIdx.x == 0)
			{
				double E[NP];
				Mat<NP> C, Fd;
				adiabatic_states_n<NP>(x[i], model, E, C, Fd);
#pragma unroll
				for (int c = 0; c < NP; ++c)
#pragma unroll
					for (int a = 0; a < NP; ++a) Cs[c][a] = C.a[c][a];
			}
			__syncthreads();
			double C[NP][NP];
#pragma unroll
			for (int c = 0; c < NP; ++c)
#pragma unroll
				for (int a = 0; a < NP; ++a) C[c][a] = Cs[c][a];
			const double gi = g[i];
			const double keep = 1.0 - gi;
			const long plane = static_cast<long>(n) * n, base = static_cast<long>(i) * n;
			double* out = slab + static_cast<long>(blockIdx.x) * NP * n;
			for (int j = threadIdx.x; j < n; j += 256)
			{
				double2 R[NP][NP];
#pragma unroll
				for (int c = 0; c < NP; ++c)
#pragma unroll
					for (int d = 0; d < NP; ++d) R[c][d] = rho[(c * NP + d) * plane + base + j];
				// Re (C^T rho C)_aa from the upper triangle: rho_dc = conj(rho_cd)
#pragma unroll
				for (int a = 0; a < NP; ++a)
				{
					double s = 0.0;
#pragma unroll
					for (int c = 0; c < NP; ++c)
					{
						double t = 0.0;
#pragma unroll
						for (int d = 0; d < NP; ++d) t += (c <= d ? R[c][d].x : R[d][c].x) * C[d][a];
						s += t * C[c][a];
					}
					out[a * n + j] = gi * s;
				}
#pragma unroll
				for (int c = 0; c < NP; ++c)
#pragma unroll
					for (int d = 0; d < NP; ++d) rho[(c * NP + d) * plane + base + j] = make_double2(keep * R[c][d].x, keep * R[c][d].y);
			}
		}

		template <int NP>
		__global__ void __launch_bounds__(256) mqcl_absorb_fold_kernel(const double* __restrict__ slab, const int* __restrict__ rows, int count, int n, int n_left,
			double* __restrict__ absorbed_p)
		{
#pragma clang fp contract(off)
			const int e = blockIdx.x * 256 + threadIdx.x; // a n + j
			if (e >= NP * n) return;
			double side[2] = {0.0, 0.0};
			int r = 0;
			for (; r < count && rows[r] < n_left; ++r) side[0] += slab[static_cast<long>(r) * NP * n + e];
			for (; r < count; ++r) side[1] += slab[static_cast<long>(r) * NP * n + e];
			absorbed_p[e] += side[0];
			absorbed_p[NP * n + e] += side[1];
		}
	} // namespace

	size_t mqcl_absorb_rows_doubles(int n) { return (static_cast<size_t>(n) + 1) / 2; }
	size_t mqcl_absorb_slab_doubles(int num_pes, int n, int count) { return static_cast<size_t>(count) * num_pes * n; }
	hipError_t launch_mqcl_absorb_rows(hipStream_t s, const double* g, int n, int* rows)
	{
		hipLaunchKernelGGL(mqcl_absorb_rows_kernel, dim3(1), dim3(256), 0, s, g, n, rows);
		return hipGetLastError();
	}
	hipError_t launch_mqcl_absorb(hipStream_t s, const MqclAbsorbArgs& a)
	{
		if (a.count == 0) return hipSuccess; // no absorbing row: the state and the accumulator stay as they are
		double2* rho = reinterpret_cast<double2*>(a.rho);
		const dim3 fold((a.num_pes * a.n + 255) / 256);
		if (a.num_pes == 2)
		{
			with_model(a.model, [&](auto m) { hipLaunchKernelGGL((mqcl_absorb_mask_kernel<2, decltype(m)>), dim3(a.count), dim3(256), 0, s, m, a.x, a.g, a.rows, a.n, rho, a.slab); });
			hipLaunchKernelGGL(mqcl_absorb_fold_kernel<2>, fold, dim3(256), 0, s, a.slab, a.rows, a.count, a.n, a.n_left, a.absorbed_p);
		}
		else if (a.num_pes == 3)
		{
			with_model(a.model, [&](auto m) { hipLaunchKernelGGL((mqcl_absorb_mask_kernel<3, decltype(m)>), dim3(a.count), dim3(256), 0, s, m, a.x, a.g, a.rows, a.n, rho, a.slab); });
			hipLaunchKernelGGL(mqcl_absorb_fold_kernel<3>, fold, dim3(256), 0, s, a.slab, a.rows, a.count, a.n, a.n_left, a.absorbed_p);
		}
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
} // namespace gple
