// gple_scatter.hip — exact branching probabilities per energy: the coupled-channel Schrodinger equation psi'' = (2 m / hbar^2)(V(x) - E) psi on the
// diabatic matrix of gple_pes_n.h, solved per total energy by the renormalised Numerov method and read at the asymptotes (gple_scatter,
// include/gple.h).  No packet, no absorber, no clock, no random number.
//
//   scatter_table_kernel<NP, M>   the upper triangle of V_n = V(x_left + n h), n = 0 ... N, once per call, and the eigenvalues of both ends (the host
//                                 looks at them before the march: a grid too coarse for an end channel is refused)
//   scatter_kernel<NP>            the march, one thread per energy.  With c = (h^2 / 12)(2 m / hbar^2):
//       A_n = I - T_n,  T_n = c (V_n - E I)             real symmetric
//       U_n = 12 A_n^-1 - 10 I                          = (I - T_n)^-1 (2 I + 10 T_n), formed from the one inverse; real symmetric
//       Numerov's rule for F_n = (I - T_n) psi_n:       F_{n+1} - U_n F_n + F_{n-1} = 0
//     Ends: V = V_0 for n <= 0 and V = V_N for n >= N.  With (eps, C) the Jacobi eigen-system of the end's matrix, t_j = c (eps_j - E),
//     u_j = 12 / (1 - t_j) - 10 and z_j the root of z + 1 / z = u_j that moves or decays to the right (|u_j| < 2, open: u_j / 2 + i sqrt(1 - u_j^2 / 4);
//     else the real root within the unit circle), z_j^n solves the rule in the constant region exactly: the match is exact for the discrete problem,
//     its flux Im(F_n^H F_{n+1}) = sum_j s_j |a_j|^2 (s_j = Im z_j) is conserved to rounding, and the only method error is the O(h^4) of the rule.
//     March from the transmitted side with L_n = F_{n-1} F_n^-1 (complex symmetric):
//       L_{N+1} = C_R diag(1 / z^R) C_R^T;   n = N ... 0:  G = L_{n+1}^-1,  L_n = U_n - G;   n = N - 1 ... 0:  M <- M G   (M = F_N F_0^-1 at the end)
//     Every L^-1 contracts a closed channel: the stable direction.  Match at the left, all incoming channels at once (columns):
//       Lambda = C_L^T L_0 C_L,  rho = (Z - Lambda)^-1 (Lambda - Z^-1),  tau = C_R^T M C_L (I + rho),  Z = diag(z^L)
//       R_{j<-i} = s^L_j |rho_ji|^2 / s^L_i,   T_{j<-i} = s^R_j |tau_ji|^2 / s^L_i;  0 exactly for a closed j, NaN for a closed i
//
// A symmetric matrix is held by its upper triangle, row by row (NE = NP (NP + 1) / 2 entries); its inverse is the adjugate on those entries, so it
// is symmetric exactly.  L, G and M stay in registers for all N + 1 steps.  Every lane reads the same V_n at a step (a uniform load, fetched one
// step ahead); nothing in the march diverges.  The asymptotes and the match are the only divergent code, open against closed.  No LDS, no atomics.
//
// Workgroup: one wave.  A thread is one serial chain of N + 1 dependent steps, so the time of a call is that of one chain for as long as every wave
// has a SIMD of its own; 4096 energies are 64 waves, and as workgroups of one wave they are spread over 64 compute units where workgroups of 256 would
// sit on 16.  tests/scatter_numpy.py restates the march operation for operation.
#include <hip/hip_runtime.h>

#include "gple_kernels.h"
#include "gple_pes_n.h"

namespace gple
{
	namespace
	{
		constexpr int SCATTER_BLOCK = 64, SCATTER_TABLE_BLOCK = 256;
		constexpr double HBAR_SCATTER = 1.0;

		struct Cx
		{
			double re, im;
		};
		__device__ __forceinline__ Cx operator+(Cx a, Cx b) { return {a.re + b.re, a.im + b.im}; }
		__device__ __forceinline__ Cx operator-(Cx a, Cx b) { return {a.re - b.re, a.im - b.im}; }
		__device__ __forceinline__ Cx operator-(Cx a) { return {-a.re, -a.im}; }
		__device__ __forceinline__ Cx operator*(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
		__device__ __forceinline__ Cx operator*(double a, Cx b) { return {a * b.re, a * b.im}; }
		__device__ __forceinline__ double abs2(Cx a) { return a.re * a.re + a.im * a.im; }
		__device__ __forceinline__ double reciprocal(double d) { return 1.0 / d; }
		// conj(d) / |d|^2, one division
		__device__ __forceinline__ Cx reciprocal(Cx d)
		{
			const double r = 1.0 / abs2(d);
			return {d.re * r, -d.im * r};
		}

		template <int NP>
		constexpr int NE = NP * (NP + 1) / 2;
		// the place of entry (i, j) in the upper triangle, row by row
		template <int NP>
		__host__ __device__ constexpr int tri(int i, int j)
		{
			return i <= j ? i * NP - i * (i - 1) / 2 + (j - i) : j * NP - j * (j - 1) / 2 + (i - j);
		}

		// the inverse of a symmetric matrix by its adjugate, on the upper triangle: exactly symmetric
		template <int NP, typename T>
		__device__ __forceinline__ void sym_inverse(const T (&a)[NE<NP>], T (&o)[NE<NP>])
		{
			static_assert(NP == 2 || NP == 3);
			if constexpr (NP == 2)
			{
				const T r = reciprocal(a[0] * a[2] - a[1] * a[1]);
				o[0] = a[2] * r, o[1] = (-a[1]) * r, o[2] = a[0] * r;
			}
			else
			{
				const T a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
				const T c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
				const T c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
				const T r = reciprocal(a00 * c00 + a01 * c01 + a02 * c02);
				o[0] = c00 * r, o[1] = c01 * r, o[2] = c02 * r, o[3] = c11 * r, o[4] = c12 * r, o[5] = c22 * r;
			}
		}

		template <int NP, typename M>
		__global__ void __launch_bounds__(SCATTER_TABLE_BLOCK) scatter_table_kernel(M model, double x_left, double h, long n_steps, double* __restrict__ table)
		{
			const long n = static_cast<long>(blockIdx.x) * SCATTER_TABLE_BLOCK + threadIdx.x;
			if (n > n_steps) return;
			Mat<NP> V, F;
			diabatic_n<NP>(x_left + static_cast<double>(n) * h, model, V, F);
			double* const node = table + n * NE<NP>;
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = i; j < NP; ++j) node[tri<NP>(i, j)] = V.a[i][j];
			if (n != 0 && n != n_steps) return;
			double eps[NP];
			jacobi_eig<NP>(V, eps, F);
			double* const end = table + (n_steps + 1) * NE<NP> + (n == 0 ? 0 : NP);
#pragma unroll
			for (int j = 0; j < NP; ++j) end[j] = eps[j];
		}

		// the channels of one end: z, 1 / z and s = Im z per eigenvalue, the eigenvectors in the columns of C
		template <int NP>
		struct ScatterEnd
		{
			Cx z[NP], zinv[NP];
			Mat<NP> C;
		};
		template <int NP>
		__device__ __forceinline__ void scatter_end(const double* __restrict__ node, double E, double c, ScatterEnd<NP>& end)
		{
			Mat<NP> V;
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = 0; j < NP; ++j) V.a[i][j] = node[tri<NP>(i, j)];
			double eps[NP];
			jacobi_eig<NP>(V, eps, end.C);
#pragma unroll
			for (int j = 0; j < NP; ++j)
			{
				const double t = c * (eps[j] - E);
				const double u = 12.0 / (1.0 - t) - 10.0;
				const double half = u / 2.0;
				Cx z;
				if (fabs(u) < 2.0) z = {half, sqrt((1.0 - half) * (1.0 + half))};
				else
				{
					const double a = fabs(half);
					z = {copysign(1.0 / (a + sqrt((a - 1.0) * (a + 1.0))), u), 0.0};
				}
				end.z[j] = z, end.zinv[j] = reciprocal(z);
			}
		}

		template <int NP>
		__global__ void __launch_bounds__(SCATTER_BLOCK) scatter_kernel(const double* __restrict__ table, long n_steps, double c, const double* __restrict__ energies,
			long n_E, double* __restrict__ prob, double* __restrict__ defect)
		{
			constexpr int S = NE<NP>;
			const long e = static_cast<long>(blockIdx.x) * SCATTER_BLOCK + threadIdx.x;
			if (e >= n_E) return;
			const double E = energies[e];
			ScatterEnd<NP> left, right;
			scatter_end<NP>(table, E, c, left);
			scatter_end<NP>(table + n_steps * S, E, c, right);

			// L_{N+1} = C_R diag(1 / z^R) C_R^T
			Cx L[S], G[S], M[NP][NP];
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = i; j < NP; ++j)
				{
					Cx acc = {0.0, 0.0};
#pragma unroll
					for (int k = 0; k < NP; ++k) acc = acc + (right.C.a[i][k] * right.C.a[j][k]) * right.zinv[k];
					L[tri<NP>(i, j)] = acc;
				}
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = 0; j < NP; ++j) M[i][j] = {i == j ? 1.0 : 0.0, 0.0};

			double v[S], ahead[S];
#pragma unroll
			for (int k = 0; k < S; ++k) ahead[k] = table[n_steps * S + k];
			for (long n = n_steps; n >= 0; --n)
			{
#pragma unroll
				for (int k = 0; k < S; ++k) v[k] = ahead[k];
				const double* const next = table + (n > 0 ? n - 1 : 0) * S; // the same address in every lane
#pragma unroll
				for (int k = 0; k < S; ++k) ahead[k] = next[k];
				sym_inverse<NP>(L, G);
				if (n < n_steps)
				{
					Cx P[NP][NP];
#pragma unroll
					for (int i = 0; i < NP; ++i)
#pragma unroll
						for (int j = 0; j < NP; ++j)
						{
							Cx acc = M[i][0] * G[tri<NP>(0, j)];
#pragma unroll
							for (int k = 1; k < NP; ++k) acc = acc + M[i][k] * G[tri<NP>(k, j)];
							P[i][j] = acc;
						}
#pragma unroll
					for (int i = 0; i < NP; ++i)
#pragma unroll
						for (int j = 0; j < NP; ++j) M[i][j] = P[i][j];
				}
				double A[S], Ainv[S];
#pragma unroll
				for (int i = 0; i < NP; ++i)
#pragma unroll
					for (int j = i; j < NP; ++j) A[tri<NP>(i, j)] = i == j ? 1.0 - c * (v[tri<NP>(i, i)] - E) : -(c * v[tri<NP>(i, j)]);
				sym_inverse<NP>(A, Ainv);
#pragma unroll
				for (int i = 0; i < NP; ++i)
#pragma unroll
					for (int j = i; j < NP; ++j)
					{
						const int k = tri<NP>(i, j);
						const double u = i == j ? 12.0 * Ainv[k] - 10.0 : 12.0 * Ainv[k];
						L[k] = {u - G[k].re, -G[k].im};
					}
			}

			// the match at the left: Lambda = C_L^T L_0 C_L
			const Mat<NP>& CL = left.C;
			const Mat<NP>& CR = right.C;
			Cx P[NP][NP], Lam[S], B[S], Binv[S], rhs[S];
#pragma unroll
			for (int k = 0; k < NP; ++k)
#pragma unroll
				for (int j = 0; j < NP; ++j)
				{
					Cx acc = CL.a[0][j] * L[tri<NP>(k, 0)];
#pragma unroll
					for (int l = 1; l < NP; ++l) acc = acc + CL.a[l][j] * L[tri<NP>(k, l)];
					P[k][j] = acc;
				}
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = i; j < NP; ++j)
				{
					Cx acc = CL.a[0][i] * P[0][j];
#pragma unroll
					for (int k = 1; k < NP; ++k) acc = acc + CL.a[k][i] * P[k][j];
					const int q = tri<NP>(i, j);
					Lam[q] = acc;
					B[q] = i == j ? left.z[i] - acc : -acc;
					rhs[q] = i == j ? acc - left.zinv[i] : acc;
				}
			sym_inverse<NP>(B, Binv);
			Cx rho[NP][NP], W[NP][NP], Q[NP][NP], Y[NP][NP], tau[NP][NP];
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = 0; j < NP; ++j)
				{
					Cx acc = Binv[tri<NP>(i, 0)] * rhs[tri<NP>(0, j)];
#pragma unroll
					for (int k = 1; k < NP; ++k) acc = acc + Binv[tri<NP>(i, k)] * rhs[tri<NP>(k, j)];
					rho[i][j] = acc;
					W[i][j] = i == j ? Cx{acc.re + 1.0, acc.im} : acc;
				}
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = 0; j < NP; ++j)
				{
					Cx acc = CL.a[i][0] * W[0][j];
#pragma unroll
					for (int k = 1; k < NP; ++k) acc = acc + CL.a[i][k] * W[k][j];
					Q[i][j] = acc;
				}
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = 0; j < NP; ++j)
				{
					Cx acc = M[i][0] * Q[0][j];
#pragma unroll
					for (int k = 1; k < NP; ++k) acc = acc + M[i][k] * Q[k][j];
					Y[i][j] = acc;
				}
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = 0; j < NP; ++j)
				{
					Cx acc = CR.a[0][i] * Y[0][j];
#pragma unroll
					for (int k = 1; k < NP; ++k) acc = acc + CR.a[k][i] * Y[k][j];
					tau[i][j] = acc;
				}

			// probabilities of incoming i: [reflected | transmitted][final j]
			const double nan = __builtin_nan("");
			double* const out = prob + e * (2 * NP * NP);
#pragma unroll
			for (int i = 0; i < NP; ++i)
			{
				const double s_in = left.z[i].im;
				const bool open_in = s_in > 0.0;
				double total = 0.0;
#pragma unroll
				for (int side = 0; side < 2; ++side)
#pragma unroll
					for (int j = 0; j < NP; ++j)
					{
						const double s_out = side == 0 ? left.z[j].im : right.z[j].im;
						const double p = s_out > 0.0 ? s_out * abs2(side == 0 ? rho[j][i] : tau[j][i]) / s_in : 0.0;
						out[(i * 2 + side) * NP + j] = open_in ? p : nan;
						total += p;
					}
				if (defect) defect[e * NP + i] = open_in ? total - 1.0 : nan;
			}
		}
	} // namespace

	double scatter_step_constant(double mass, double x_left, double x_right, long n_steps)
	{
		const double h = (x_right - x_left) / static_cast<double>(n_steps);
		return h * h / 12.0 * (2.0 * mass / (HBAR_SCATTER * HBAR_SCATTER));
	}
	size_t scatter_table_doubles(int num_pes, long n_steps)
	{
		return (static_cast<size_t>(n_steps) + 1) * static_cast<size_t>(num_pes * (num_pes + 1) / 2) + 2 * static_cast<size_t>(num_pes);
	}
	hipError_t launch_scatter_table(hipStream_t s, int num_pes, PesModel model, double x_left, double x_right, long n_steps, double* table)
	{
		if ((num_pes != 2 && num_pes != 3) || n_steps < 1) return hipErrorInvalidValue;
		const double h = (x_right - x_left) / static_cast<double>(n_steps);
		const dim3 grid(static_cast<unsigned>((n_steps + SCATTER_TABLE_BLOCK) / SCATTER_TABLE_BLOCK)), block(SCATTER_TABLE_BLOCK);
		with_model(model, [&](auto m) {
			if (num_pes == 2) hipLaunchKernelGGL((scatter_table_kernel<2, decltype(m)>), grid, block, 0, s, m, x_left, h, n_steps, table);
			else hipLaunchKernelGGL((scatter_table_kernel<3, decltype(m)>), grid, block, 0, s, m, x_left, h, n_steps, table);
		});
		return hipGetLastError();
	}
	hipError_t launch_scatter(hipStream_t s, int num_pes, double c, long n_steps, const double* table, const double* energies, long n_E, double* prob,
		double* defect)
	{
		if ((num_pes != 2 && num_pes != 3) || n_steps < 1 || n_E < 1) return hipErrorInvalidValue;
		const dim3 grid(static_cast<unsigned>((n_E + SCATTER_BLOCK - 1) / SCATTER_BLOCK)), block(SCATTER_BLOCK);
		if (num_pes == 2) hipLaunchKernelGGL(scatter_kernel<2>, grid, block, 0, s, table, n_steps, c, energies, n_E, prob, defect);
		else hipLaunchKernelGGL(scatter_kernel<3>, grid, block, 0, s, table, n_steps, c, energies, n_E, prob, defect);
		return hipGetLastError();
	}
} // namespace gple
