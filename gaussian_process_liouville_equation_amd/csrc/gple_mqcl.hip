// gple_mqcl.hip — exact mixed quantum-classical Liouville (MQCLE) dynamics on the (x, p) grid: the reference's liouville_equation/ in the
// diabatic evolve basis (main.cpp:153, general.cpp:171-510).
//
//   State: the num_pes^2 x n x n phase.txt layout of the caller (element (a, b) row-major, x major, p fastest); only the P_u = NP (NP + 1) / 2
//   planes a <= b are read and evolved, rho_ba = conj(rho_ab) is written at the end of a call (mqcl_lower_kernel).
//   mqcl_pes_kernel      per x: adiabatic C, E (gple_pes_n.h, the library's sign convention), force basis U, lambda (eigenvectors of the
//                        diabatic force; signs cancel), and the phase factors exp(i (E_b - E_a) t_q / hbar) of one Q(dt/2).
//   mqcl_chirp_kernel    Bluestein chirp b_m = exp(i pi m^2 / n) and FFT twiddles exp(-2 pi i k / M), both from integer indices reduced modulo
//                        their period (sincospi).  mqcl_bhat_kernel: FFT_M of the wrapped chirp, kept in the bit-reversed order of the DIF FFT.
//   shift_row            one row of length n: DFT -> psi multiplier -> inverse DFT (general.cpp:266-510 followed by the hermitisation of
//                        matrix.cpp:414-428, folded into psi: DESIGN.md §12) as four radix-2 FFTs of length M through one LDS buffer.
//                        Forward FFTs are decimation in frequency (natural in, bit-reversed out), inverse ones decimation in time, so no
//                        permutation is ever done; the zero half of every Bluestein input and the pointwise products are fused into the
//                        adjacent butterfly stages.  No spectrum leaves LDS.
//   mqcl_ppass_kernel    P(dt): a workgroup owns an x row and every plane (registers): to the force basis, shift each plane, back.
//   mqcl_xpass_kernel    R(dt/2) Q(dt/2) | Q(dt/2) R(dt/2) between two P passes (one Q at the ends of a call), on the transposed planes.
//   mqcl_transpose_kernel  32 x 32 LDS-tiled transpose between the caller's planes and the compact transposed copy the X pass reads.
//   mqcl_observe_*       adiabatic rho, (E, x, p) and populations (general.cpp:108-164) in a fixed reduction order.
#include <algorithm>

#include "gple_kernels.h"
#include "gple_pes_n.h"

namespace gple
{
	namespace
	{
		constexpr double PI_D = 3.141592653589793116; // acos(-1.0) (general.h:20)
		constexpr double HBAR_D = 1.0;                 // general.h:21

		__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
		__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
		__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
		__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); } // a conj(b)
		__device__ __forceinline__ double2 cscale(double2 a, double s) { return make_double2(a.x * s, a.y * s); }

		// the element pairs (a, b), a <= b, of the stored planes, row-major
		template <int NP>
		struct Pairs
		{
			static constexpr int NU = NP * (NP + 1) / 2;
			__device__ static constexpr int a(int u) { return NP == 2 ? (u < 2 ? 0 : 1) : (u < 3 ? 0 : (u < 5 ? 1 : 2)); }
			__device__ static constexpr int b(int u) { return NP == 2 ? (u == 0 ? 0 : 1) : (u < 3 ? u : (u < 5 ? u - 2 : 2)); }
		};
		// per-x table: C (NP^2) | E (NP) | U (NP^2) | lambda (NP) | cos, sin of the Q phase per pair a < b
		template <int NP>
		struct PesRow
		{
			static constexpr int C = 0, E = NP * NP, U = E + NP, L = U + NP * NP, Q = L + NP, STRIDE = Q + NP * (NP - 1);
		};
		__host__ __device__ constexpr int pes_stride(int np) { return 2 * np * np + 2 * np + np * (np - 1); }

		// the reference's frequency of DFT bin k (general.cpp:339-346): k for k < n / 2, else k - n
		__device__ __forceinline__ int ref_freq(int k, int n) { return k < n / 2 ? k : k - n; }

		// rho -> B^T rho B (to_basis) or B rho B^T (from basis), B real, rho Hermitian given by its upper triangle; the result's upper triangle
		// with the diagonal's imaginary parts zero (the hermitisation of matrix.cpp:414-428 on the stored triangle)
		template <int NP>
		__device__ __forceinline__ void rotate(double2 (&u)[Pairs<NP>::NU], const double* __restrict__ B, bool to_basis)
		{
			double2 R[NP][NP];
#pragma unroll
			for (int k = 0; k < Pairs<NP>::NU; ++k)
			{
				const int a = Pairs<NP>::a(k), b = Pairs<NP>::b(k);
				R[a][b] = u[k];
				R[b][a] = make_double2(u[k].x, -u[k].y);
			}
			double Bm[NP][NP];
#pragma unroll
			for (int c = 0; c < NP; ++c)
#pragma unroll
				for (int d = 0; d < NP; ++d) Bm[c][d] = to_basis ? B[c * NP + d] : B[d * NP + c]; // to_basis: B; else B^T (so that the product is Bm^T R Bm)
#pragma unroll
			for (int k = 0; k < Pairs<NP>::NU; ++k)
			{
				const int a = Pairs<NP>::a(k), b = Pairs<NP>::b(k);
				double2 s = make_double2(0.0, 0.0);
#pragma unroll
				for (int c = 0; c < NP; ++c)
				{
					double2 t = make_double2(0.0, 0.0);
#pragma unroll
					for (int d = 0; d < NP; ++d) t = cadd(t, cscale(R[c][d], Bm[d][b]));
					s = cadd(s, cscale(t, Bm[c][a]));
				}
				if (a == b) s.y = 0.0;
				u[k] = s;
			}
		}

		// Q(t) of general.cpp:184-209 at one grid point: to the adiabatic basis, rho_ab *= exp(i (E_b - E_a) t / hbar) for a < b, back
		template <int NP>
		__device__ __forceinline__ void quantum_step(double2 (&u)[Pairs<NP>::NU], const double* __restrict__ row)
		{
			rotate<NP>(u, row + PesRow<NP>::C, true);
			int q = 0;
#pragma unroll
			for (int k = 0; k < Pairs<NP>::NU; ++k)
				if (Pairs<NP>::a(k) != Pairs<NP>::b(k))
				{
					u[k] = cmul(u[k], make_double2(row[PesRow<NP>::Q + 2 * q], row[PesRow<NP>::Q + 2 * q + 1]));
					++q;
				}
			rotate<NP>(u, row + PesRow<NP>::C, false);
		}

		__global__ void __launch_bounds__(256) mqcl_chirp_kernel(int n, int M, double2* __restrict__ chirp, double2* __restrict__ tw)
		{
			const int k = blockIdx.x * 256 + threadIdx.x;
			if (k < n)
			{
				const long m2 = (static_cast<long>(k) * k) % (2L * n); // b_k = exp(i pi k^2 / n), period 2n in k^2
				double s, c;
				sincospi(static_cast<double>(m2) / static_cast<double>(n), &s, &c);
				chirp[k] = make_double2(c, s);
			}
			if (k < M / 2)
			{
				double s, c;
				sincospi(-2.0 * static_cast<double>(k) / static_cast<double>(M), &s, &c); // exact argument: M is a power of two
				tw[k] = make_double2(c, s);
			}
		}

		template <int NP, typename PES>
		__global__ void __launch_bounds__(128) mqcl_pes_kernel(PES model, const double* __restrict__ x, int n, double tq, double* __restrict__ table)
		{
#pragma clang fp contract(off)
			const int i = blockIdx.x * 128 + threadIdx.x;
			if (i >= n) return;
			double E[NP], lam[NP];
			Mat<NP> C, Fd, U;
			adiabatic_states_n<NP>(x[i], model, E, C, Fd);
			jacobi_eig<NP>(Fd, lam, U);
			double* r = table + static_cast<long>(i) * PesRow<NP>::STRIDE;
#pragma unroll
			for (int a = 0; a < NP; ++a)
			{
				r[PesRow<NP>::E + a] = E[a], r[PesRow<NP>::L + a] = lam[a];
#pragma unroll
				for (int b = 0; b < NP; ++b) r[PesRow<NP>::C + a * NP + b] = C.a[a][b], r[PesRow<NP>::U + a * NP + b] = U.a[a][b];
			}
			int q = 0;
#pragma unroll
			for (int a = 0; a < NP; ++a)
#pragma unroll
				for (int b = a + 1; b < NP; ++b)
				{
					const double th = (E[b] - E[a]) * tq / HBAR_D; // general.cpp:202
					r[PesRow<NP>::Q + 2 * q] = cos(th), r[PesRow<NP>::Q + 2 * q + 1] = sin(th);
					++q;
				}
		}

		// ---- the LDS FFT ------------------------------------------------------------------------------------------------------------------
		// tw[k] = exp(-2 pi i k / M), k < M / 2.  Stages of half-size h touch (i0, i0 + h), i0 = (t / h) 2h + t % h for butterfly t < M / 2.
		template <int NT>
		__device__ __forceinline__ void dif_stages(double2* L, int M, int h_hi, int h_lo, const double2* __restrict__ tw)
		{
			for (int h = h_hi; h >= h_lo; h >>= 1)
			{
				const int lh = __ffs(h) - 1, step = M / (2 * h);
				for (int t = threadIdx.x; t < M / 2; t += NT)
				{
					const int j = t & (h - 1), i0 = ((t >> lh) << (lh + 1)) + j;
					const double2 a = L[i0], b = L[i0 + h];
					L[i0] = cadd(a, b);
					L[i0 + h] = cmul(csub(a, b), tw[j * step]);
				}
				__syncthreads();
			}
		}
		template <int NT>
		__device__ __forceinline__ void dit_stages(double2* L, int M, int h_lo, int h_hi, const double2* __restrict__ tw)
		{
			for (int h = h_lo; h <= h_hi; h <<= 1)
			{
				const int lh = __ffs(h) - 1, step = M / (2 * h);
				for (int t = threadIdx.x; t < M / 2; t += NT)
				{
					const int j = t & (h - 1), i0 = ((t >> lh) << (lh + 1)) + j;
					const double2 a = L[i0], b = cmulc(L[i0 + h], tw[j * step]);
					L[i0] = cadd(a, b);
					L[i0 + h] = csub(a, b);
				}
				__syncthreads();
			}
		}
		// last DIF stage (h = 1), times the chirp spectrum (conjugated for the inverse chirp), first DIT stage (h = 1): one pass, same thread
		template <int NT>
		__device__ __forceinline__ void spectrum_product(double2* L, int M, const double2* __restrict__ bhat, bool conj_bhat)
		{
			for (int t = threadIdx.x; t < M / 2; t += NT)
			{
				const double2 a = L[2 * t], b = L[2 * t + 1];
				double2 h0 = bhat[2 * t], h1 = bhat[2 * t + 1];
				if (conj_bhat) h0.y = -h0.y, h1.y = -h1.y;
				const double2 A = cmul(cadd(a, b), h0), B = cmul(csub(a, b), h1);
				L[2 * t] = cadd(A, B);
				L[2 * t + 1] = csub(A, B);
			}
			__syncthreads();
		}

		struct ShiftTables
		{
			const double2* chirp; // n
			const double2* tw;    // M / 2
			const double2* bhat;  // M, bit-reversed order
			int n, M;
		};

		// One row v (slot r holds index tid + r NT, < n) through DFT, w_k = psi_k V_k, inverse DFT with 1 / n.  Bluestein:
		//   V_k = conj(b_k) (a * h)_k with a_i = v_i conj(b_i), h the wrapped chirp;  w_i = b_i / n ((psi o (a * h)) * conj(h))_i,
		// the forward and inverse chirps cancelling in the middle.  psi(r) returns psi at index tid + r NT (< n).
		template <int NT, typename PsiF>
		__device__ __forceinline__ void shift_row(double2 (&v)[4], double2* L, const ShiftTables& T, PsiF psi)
		{
			const int n = T.n, M = T.M, half = M / 2;
			// load, fused with the first DIF stage (the upper half of the input is zero: n <= M / 2)
#pragma unroll
			for (int r = 0; r < 4; ++r)
			{
				const int j = threadIdx.x + r * NT;
				if (j < half)
				{
					const double2 a = j < n ? cmulc(v[r], T.chirp[j]) : make_double2(0.0, 0.0);
					L[j] = a;
					L[j + half] = cmul(a, T.tw[j]);
				}
			}
			__syncthreads();
			dif_stages<NT>(L, M, M / 4, 2, T.tw);
			spectrum_product<NT>(L, M, T.bhat, false);
			dit_stages<NT>(L, M, 2, M / 4, T.tw);
			// last DIT stage (natural order, only k < n), psi_k / M, first DIF stage of the second convolution
			const double inv_m = 1.0 / static_cast<double>(M);
#pragma unroll
			for (int r = 0; r < 4; ++r)
			{
				const int j = threadIdx.x + r * NT;
				if (j < half)
				{
					double2 c = make_double2(0.0, 0.0);
					if (j < n) c = cscale(cmul(cadd(L[j], cmulc(L[j + half], T.tw[j])), psi(r)), inv_m);
					L[j] = c;
					L[j + half] = cmul(c, T.tw[j]);
				}
			}
			__syncthreads();
			dif_stages<NT>(L, M, M / 4, 2, T.tw);
			spectrum_product<NT>(L, M, T.bhat, true);
			dit_stages<NT>(L, M, 2, M / 4, T.tw);
			const double sc = 1.0 / (static_cast<double>(n) * static_cast<double>(M));
#pragma unroll
			for (int r = 0; r < 4; ++r)
			{
				const int j = threadIdx.x + r * NT;
				if (j < n) v[r] = cscale(cmul(cadd(L[j], cmulc(L[j + half], T.tw[j])), T.chirp[j]), sc);
			}
			__syncthreads(); // L is reused by the next row
		}

		// psi_k = (phi_k + conj(phi_{(n - k) mod n})) / 2, phi_k = exp(i theta(f_k)): the hermitised shift
		template <typename ThetaF>
		__device__ __forceinline__ double2 psi_at(int k, int n, ThetaF theta)
		{
			double s0, c0, s1, c1;
			sincos(theta(ref_freq(k, n)), &s0, &c0);
			sincos(theta(ref_freq(k == 0 ? 0 : n - k, n)), &s1, &c1);
			return make_double2(0.5 * (c0 + c1), 0.5 * (s0 - s1));
		}

		// full bluestein FFT of the wrapped chirp, one workgroup
		template <int NT>
		__global__ void __launch_bounds__(NT) mqcl_bhat_kernel(ShiftTables T, double2* __restrict__ bhat)
		{
			__shared__ double2 L[8192];
			const int n = T.n, M = T.M;
			for (int m = threadIdx.x; m < M; m += NT)
			{
				double2 h = make_double2(0.0, 0.0);
				if (m < n) h = T.chirp[m];
				else if (m > M - n) h = T.chirp[M - m];
				L[m] = h;
			}
			__syncthreads();
			dif_stages<NT>(L, M, M / 2, 1, T.tw);
			for (int m = threadIdx.x; m < M; m += NT) bhat[m] = L[m];
		}

		// P(dt), general.cpp:388-510: per x row, rho -> U^T rho U, shift every plane along p with exp(-(lambda_a + lambda_b) f pi i / L_p dt),
		// -> U rho U^T.  rho: the caller's full layout (planes a NP + b), n x n each.
		template <int NP, int NT>
		__global__ void __launch_bounds__(NT) mqcl_ppass_kernel(double2* __restrict__ rho, const double* __restrict__ table, ShiftTables T, double length_p, double dt)
		{
			__shared__ double2 L[8 * NT];
			constexpr int NU = Pairs<NP>::NU;
			const int n = T.n, i = blockIdx.x;
			const long plane = static_cast<long>(n) * n, base = static_cast<long>(i) * n;
			const double* row = table + static_cast<long>(i) * PesRow<NP>::STRIDE;
			double2 v[NU][4];
#pragma unroll
			for (int r = 0; r < 4; ++r)
			{
				const int j = threadIdx.x + r * NT;
				double2 u[NU];
#pragma unroll
				for (int k = 0; k < NU; ++k) u[k] = j < n ? rho[(Pairs<NP>::a(k) * NP + Pairs<NP>::b(k)) * plane + base + j] : make_double2(0.0, 0.0);
				rotate<NP>(u, row + PesRow<NP>::U, true);
#pragma unroll
				for (int k = 0; k < NU; ++k) v[k][r] = u[k];
			}
#pragma unroll
			for (int k = 0; k < NU; ++k)
			{
				const double s = row[PesRow<NP>::L + Pairs<NP>::a(k)] + row[PesRow<NP>::L + Pairs<NP>::b(k)];
				auto theta = [=](int f) {
#pragma clang fp contract(off)
					return -s * static_cast<double>(f) * PI_D / length_p * dt; // general.cpp:469, 473
				};
				shift_row<NT>(v[k], L, T, [&](int r) { return psi_at(threadIdx.x + r * NT, n, theta); });
				if (Pairs<NP>::a(k) == Pairs<NP>::b(k))
#pragma unroll
					for (int r = 0; r < 4; ++r) v[k][r].y = 0.0;
			}
#pragma unroll
			for (int r = 0; r < 4; ++r)
			{
				const int j = threadIdx.x + r * NT;
				double2 u[NU];
#pragma unroll
				for (int k = 0; k < NU; ++k) u[k] = v[k][r];
				rotate<NP>(u, row + PesRow<NP>::U, false);
				if (j < n)
#pragma unroll
					for (int k = 0; k < NU; ++k) rho[(Pairs<NP>::a(k) * NP + Pairs<NP>::b(k)) * plane + base + j] = u[k];
			}
		}

		// lead: R(t) first; nq: Q(t) once or twice; trail: R(t) last.  Tt: the compact transposed planes, Tt[k][j n + i] = rho_k(x_i, p_j).
		// R(t), general.cpp:266-380: shift along x with exp(-p_j / m 2 f pi i / L_x t).
		template <int NP, int NT>
		__global__ void __launch_bounds__(NT) mqcl_xpass_kernel(double2* __restrict__ Tt, const double* __restrict__ table, const double* __restrict__ p,
			ShiftTables T, double mass, double length_x, double t, int lead, int nq, int trail)
		{
			__shared__ double2 L[8 * NT];
			constexpr int NU = Pairs<NP>::NU;
			const int n = T.n, j = blockIdx.x;
			const long plane = static_cast<long>(n) * n, base = static_cast<long>(j) * n;
			const double pj = p[j];
			auto theta = [=](int f) {
#pragma clang fp contract(off)
				return -pj / mass * 2.0 * static_cast<double>(f) * PI_D / length_x * t; // general.cpp:341, 345
			};
			double2 psi[4];
#pragma unroll
			for (int r = 0; r < 4; ++r)
			{
				const int k = threadIdx.x + r * NT;
				psi[r] = k < n ? psi_at(k, n, theta) : make_double2(0.0, 0.0);
			}
			double2 v[NU][4];
#pragma unroll
			for (int k = 0; k < NU; ++k)
#pragma unroll
				for (int r = 0; r < 4; ++r)
				{
					const int i = threadIdx.x + r * NT;
					v[k][r] = i < n ? Tt[k * plane + base + i] : make_double2(0.0, 0.0);
				}
			auto shift_all = [&]() {
#pragma unroll
				for (int k = 0; k < NU; ++k)
				{
					shift_row<NT>(v[k], L, T, [&](int r) { return psi[r]; });
					if (Pairs<NP>::a(k) == Pairs<NP>::b(k))
#pragma unroll
						for (int r = 0; r < 4; ++r) v[k][r].y = 0.0;
				}
			};
			if (lead) shift_all();
#pragma unroll
			for (int r = 0; r < 4; ++r)
			{
				const int i = threadIdx.x + r * NT;
				if (i < n)
				{
					const double* row = table + static_cast<long>(i) * PesRow<NP>::STRIDE;
					double2 u[NU];
#pragma unroll
					for (int k = 0; k < NU; ++k) u[k] = v[k][r];
					for (int q = 0; q < nq; ++q) quantum_step<NP>(u, row);
#pragma unroll
					for (int k = 0; k < NU; ++k) v[k][r] = u[k];
				}
			}
			if (trail) shift_all();
#pragma unroll
			for (int k = 0; k < NU; ++k)
#pragma unroll
				for (int r = 0; r < 4; ++r)
				{
					const int i = threadIdx.x + r * NT;
					if (i < n) Tt[k * plane + base + i] = v[k][r];
				}
		}

		// to_t: full-layout planes (a NP + b) -> compact transposed planes k; else back
		template <int NP>
		__global__ void __launch_bounds__(256) mqcl_transpose_kernel(double2* __restrict__ full, double2* __restrict__ Tt, int n, int to_t)
		{
			__shared__ double2 tile[32][33];
			const int k = blockIdx.z, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
			const long plane = static_cast<long>(n) * n;
			double2* F = full + (Pairs<NP>::a(k) * NP + Pairs<NP>::b(k)) * plane;
			double2* G = Tt + k * plane;
			const double2* src = to_t ? F : G;
			double2* dst = to_t ? G : F;
			const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
			for (int y = ty; y < 32; y += 8)
				if (r0 + y < n && c0 + tx < n) tile[y][tx] = src[static_cast<long>(r0 + y) * n + c0 + tx];
			__syncthreads();
			for (int y = ty; y < 32; y += 8)
				if (c0 + y < n && r0 + tx < n) dst[static_cast<long>(c0 + y) * n + r0 + tx] = tile[tx][y];
		}

		// rho_ba = conj(rho_ab) for a < b, from the stored upper planes
		template <int NP>
		__global__ void __launch_bounds__(256) mqcl_lower_kernel(double2* __restrict__ rho, int n)
		{
			const long plane = static_cast<long>(n) * n, e = blockIdx.x * 256L + threadIdx.x;
			if (e >= plane) return;
#pragma unroll
			for (int a = 0; a < NP; ++a)
#pragma unroll
				for (int b = a + 1; b < NP; ++b)
				{
					const double2 v = rho[(a * NP + b) * plane + e];
					rho[(b * NP + a) * plane + e] = make_double2(v.x, -v.y);
				}
		}

		// basis_transform[from][to] (pes.cpp:360-700): through the diabatic basis, each rotation hermitised.  0 diabatic, 1 adiabatic, 2 force.
		template <int NP>
		__global__ void __launch_bounds__(256) mqcl_transform_kernel(const double2* __restrict__ in, double2* __restrict__ out, const double* __restrict__ table,
			int n, int from, int to)
		{
			constexpr int NU = Pairs<NP>::NU;
			const long plane = static_cast<long>(n) * n, e = blockIdx.x * 256L + threadIdx.x;
			if (e >= plane) return;
			const double* row = table + (e / n) * PesRow<NP>::STRIDE;
			double2 u[NU];
#pragma unroll
			for (int k = 0; k < NU; ++k) u[k] = in[(Pairs<NP>::a(k) * NP + Pairs<NP>::b(k)) * plane + e];
			if (from == to)
#pragma unroll
				for (int k = 0; k < NU; ++k)
					if (Pairs<NP>::a(k) == Pairs<NP>::b(k)) u[k].y = 0.0;
			if (from != to && from != 0) rotate<NP>(u, row + (from == 1 ? PesRow<NP>::C : PesRow<NP>::U), false);
			if (from != to && to != 0) rotate<NP>(u, row + (to == 1 ? PesRow<NP>::C : PesRow<NP>::U), true);
#pragma unroll
			for (int k = 0; k < NU; ++k)
			{
				const int a = Pairs<NP>::a(k), b = Pairs<NP>::b(k);
				out[(a * NP + b) * plane + e] = u[k];
				if (a != b) out[(b * NP + a) * plane + e] = make_double2(u[k].x, -u[k].y);
			}
		}

		// per x row: adiabatic rho (optional) and the row sums of sum_a rho_aa (E_a + p^2 / 2m), x, p, rho_aa (general.cpp:108-164), in a fixed order
		template <int NP>
		__global__ void __launch_bounds__(256) mqcl_observe_row_kernel(const double2* __restrict__ rho, double2* __restrict__ adia, const double* __restrict__ table,
			const double* __restrict__ x, const double* __restrict__ p, int n, double mass, double* __restrict__ partial)
		{
#pragma clang fp contract(off)
			constexpr int NU = Pairs<NP>::NU, NS = 3 + NP;
			__shared__ double red[NS][256];
			const int i = blockIdx.x;
			const long plane = static_cast<long>(n) * n, base = static_cast<long>(i) * n;
			const double* row = table + static_cast<long>(i) * PesRow<NP>::STRIDE;
			const double xi = x[i];
			double acc[NS] = {};
			for (int j = threadIdx.x; j < n; j += 256)
			{
				double2 u[NU];
#pragma unroll
				for (int k = 0; k < NU; ++k) u[k] = rho[(Pairs<NP>::a(k) * NP + Pairs<NP>::b(k)) * plane + base + j];
				rotate<NP>(u, row + PesRow<NP>::C, true);
				if (adia)
#pragma unroll
					for (int k = 0; k < NU; ++k)
					{
						const int a = Pairs<NP>::a(k), b = Pairs<NP>::b(k);
						adia[(a * NP + b) * plane + base + j] = u[k];
						if (a != b) adia[(b * NP + a) * plane + base + j] = make_double2(u[k].x, -u[k].y);
					}
				const double pj = p[j];
				int d = 0;
#pragma unroll
				for (int k = 0; k < NU; ++k)
					if (Pairs<NP>::a(k) == Pairs<NP>::b(k))
					{
						const double ppl = u[k].x;
						acc[0] += ppl * (row[PesRow<NP>::E + d] + pj * pj / 2.0 / mass);
						acc[1] += ppl * xi;
						acc[2] += ppl * pj;
						acc[3 + d] += ppl;
						++d;
					}
			}
#pragma unroll
			for (int s = 0; s < NS; ++s) red[s][threadIdx.x] = acc[s];
			__syncthreads();
			for (int w = 128; w > 0; w >>= 1)
			{
				if (threadIdx.x < w)
#pragma unroll
					for (int s = 0; s < NS; ++s) red[s][threadIdx.x] += red[s][threadIdx.x + w];
				__syncthreads();
			}
			if (threadIdx.x < NS) partial[static_cast<long>(i) * NS + threadIdx.x] = red[threadIdx.x][0];
		}
		__global__ void __launch_bounds__(256) mqcl_observe_final_kernel(const double* __restrict__ partial, int n, int ns, double dxdp, double* __restrict__ out)
		{
			__shared__ double red[256];
			for (int s = 0; s < ns; ++s)
			{
				double acc = 0.0;
				for (int i = threadIdx.x; i < n; i += 256) acc += partial[static_cast<long>(i) * ns + s];
				red[threadIdx.x] = acc;
				__syncthreads();
				for (int w = 128; w > 0; w >>= 1)
				{
					if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
					__syncthreads();
				}
				if (threadIdx.x == 0) out[s] = red[0] * dxdp;
				__syncthreads();
			}
		}

		int mqcl_threads(int n) { return n <= 256 ? 64 : n <= 1024 ? 256 : n <= 2048 ? 512 : 1024; }
		template <int NP, int NT>
		hipError_t launch_passes(hipStream_t s, const MqclEvolveArgs& g)
		{
			const ShiftTables T{reinterpret_cast<const double2*>(g.chirp), reinterpret_cast<const double2*>(g.tw), reinterpret_cast<const double2*>(g.bhat), g.n, g.M};
			double2* rho = reinterpret_cast<double2*>(g.rho);
			double2* Tt = reinterpret_cast<double2*>(g.transposed);
			const int tb = (g.n + 31) / 32;
			const dim3 tgrid(tb, tb, Pairs<NP>::NU);
			const double th = g.dt / 2.0;
			auto xpass = [&](int lead, int nq, int trail) {
				hipLaunchKernelGGL(mqcl_transpose_kernel<NP>, tgrid, dim3(256), 0, s, rho, Tt, g.n, 1);
				hipLaunchKernelGGL((mqcl_xpass_kernel<NP, NT>), dim3(g.n), dim3(NT), 0, s, Tt, g.table, g.p, T, g.mass, g.length_x, th, lead, nq, trail);
				hipLaunchKernelGGL(mqcl_transpose_kernel<NP>, tgrid, dim3(256), 0, s, rho, Tt, g.n, 0);
			};
			// Q R | P | R Q Q R | P | ... | P | R Q   (main.cpp:192-260 for n_steps steps)
			xpass(0, 1, 1);
			for (long k = 0; k < g.n_steps; ++k)
			{
				hipLaunchKernelGGL((mqcl_ppass_kernel<NP, NT>), dim3(g.n), dim3(NT), 0, s, rho, g.table, T, g.length_p, g.dt);
				if (k + 1 < g.n_steps) xpass(1, 2, 1);
				else xpass(1, 1, 0);
			}
			return hipGetLastError();
		}
		template <int NP>
		hipError_t launch_passes_np(hipStream_t s, const MqclEvolveArgs& g)
		{
			switch (mqcl_threads(g.n))
			{
			case 64: return launch_passes<NP, 64>(s, g);
			case 256: return launch_passes<NP, 256>(s, g);
			case 512: return launch_passes<NP, 512>(s, g);
			default: return launch_passes<NP, 1024>(s, g);
			}
		}
	} // namespace

	int mqcl_fft_length(int n)
	{
		int M = 1;
		while (M < 2 * n - 1) M <<= 1;
		return M;
	}
	size_t mqcl_table_doubles(int num_pes, int n)
	{
		const size_t M = static_cast<size_t>(mqcl_fft_length(n));
		return static_cast<size_t>(pes_stride(num_pes)) * n + 2 * (static_cast<size_t>(n) + M / 2 + M);
	}
	hipError_t launch_mqcl_tables(hipStream_t s, int num_pes, PesModel model, const double* x, int n, double tq, bool spectral, double* tables)
	{
		const int M = mqcl_fft_length(n);
		double* chirp = tables + static_cast<size_t>(pes_stride(num_pes)) * n;
		double* tw = chirp + 2 * static_cast<size_t>(n);
		double* bhat = tw + M;
		if (num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((mqcl_pes_kernel<2, decltype(m)>), dim3((n + 127) / 128), dim3(128), 0, s, m, x, n, tq, tables); });
		else with_model(model, [&](auto m) { hipLaunchKernelGGL((mqcl_pes_kernel<3, decltype(m)>), dim3((n + 127) / 128), dim3(128), 0, s, m, x, n, tq, tables); });
		if (!spectral) return hipGetLastError();
		hipLaunchKernelGGL(mqcl_chirp_kernel, dim3((std::max(n, M / 2) + 255) / 256), dim3(256), 0, s, n, M, reinterpret_cast<double2*>(chirp),
			reinterpret_cast<double2*>(tw));
		const ShiftTables T{reinterpret_cast<const double2*>(chirp), reinterpret_cast<const double2*>(tw), nullptr, n, M};
		hipLaunchKernelGGL(mqcl_bhat_kernel<256>, dim3(1), dim3(256), 0, s, T, reinterpret_cast<double2*>(bhat));
		return hipGetLastError();
	}
	hipError_t launch_mqcl_evolve(hipStream_t s, const MqclEvolveArgs& g)
	{
		const size_t stride = static_cast<size_t>(pes_stride(g.num_pes)) * g.n;
		MqclEvolveArgs a = g;
		a.M = mqcl_fft_length(g.n);
		a.chirp = g.table + stride;
		a.tw = a.chirp + 2 * static_cast<size_t>(g.n);
		a.bhat = a.tw + a.M;
		if (g.num_pes == 2) return launch_passes_np<2>(s, a);
		if (g.num_pes == 3) return launch_passes_np<3>(s, a);
		return hipErrorInvalidValue;
	}
	hipError_t launch_mqcl_lower(hipStream_t s, int num_pes, int n, double* rho)
	{
		const long plane = static_cast<long>(n) * n;
		const dim3 grid(static_cast<unsigned>((plane + 255) / 256));
		if (num_pes == 2) hipLaunchKernelGGL(mqcl_lower_kernel<2>, grid, dim3(256), 0, s, reinterpret_cast<double2*>(rho), n);
		else hipLaunchKernelGGL(mqcl_lower_kernel<3>, grid, dim3(256), 0, s, reinterpret_cast<double2*>(rho), n);
		return hipGetLastError();
	}
	hipError_t launch_mqcl_transform(hipStream_t s, int num_pes, int n, int from, int to, const double* tables, const double* in, double* out)
	{
		const long plane = static_cast<long>(n) * n;
		const dim3 grid(static_cast<unsigned>((plane + 255) / 256));
		const double2* i2 = reinterpret_cast<const double2*>(in);
		double2* o2 = reinterpret_cast<double2*>(out);
		if (num_pes == 2) hipLaunchKernelGGL(mqcl_transform_kernel<2>, grid, dim3(256), 0, s, i2, o2, tables, n, from, to);
		else hipLaunchKernelGGL(mqcl_transform_kernel<3>, grid, dim3(256), 0, s, i2, o2, tables, n, from, to);
		return hipGetLastError();
	}
	size_t mqcl_observe_work_doubles(int num_pes, int n) { return static_cast<size_t>(n) * (3 + num_pes); }
	hipError_t launch_mqcl_observe(hipStream_t s, int num_pes, int n, const double* tables, const double* x, const double* p, double mass, double dxdp,
		const double* rho, double* adia, double* work, double* out)
	{
		const double2* r2 = reinterpret_cast<const double2*>(rho);
		double2* a2 = reinterpret_cast<double2*>(adia);
		if (num_pes == 2) hipLaunchKernelGGL(mqcl_observe_row_kernel<2>, dim3(n), dim3(256), 0, s, r2, a2, tables, x, p, n, mass, work);
		else hipLaunchKernelGGL(mqcl_observe_row_kernel<3>, dim3(n), dim3(256), 0, s, r2, a2, tables, x, p, n, mass, work);
		hipLaunchKernelGGL(mqcl_observe_final_kernel, dim3(1), dim3(256), 0, s, work, n, 3 + num_pes, dxdp, out);
		return hipGetLastError();
	}
} // namespace gple
