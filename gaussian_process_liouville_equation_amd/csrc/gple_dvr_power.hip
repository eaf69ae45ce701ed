// gple_dvr_power.hip — the absorbing boundary of the exact DVR dynamics (schrodinger_equation/ of the reference, general.h:88-93):
// classical RK4 on i hbar dpsi/dt = (H - i W) psi (the method general.cpp:233-236 documents) as powers of its one-step propagator.
//
//   dvr_absorber_kernel     absorbing_potential (pes.cpp:64-93) on the grid, x <= xmin on the left-hand branch (W >= 0 everywhere).
//   dvr_generator_kernel    A = -(W + i H) dt / hbar: Re A is diagonal (a vector), Im A = G an ld x ld plane, ld = dim rounded up to 64, zero padded.
//   dvr_horner_*            P4(A) = I + A (I + A/2 (I + A/3 (I + A/4))): a product with A/k is a row scaling by Re A / k (with the identity added,
//                           dvr_horner_scale_kernel) plus two real GEMMs with G (alpha = -+ 1/k, beta = 1).
//   complex_product         Z = X Y on (Re, Im) planes as four real products through launch_gemm (alpha = +-1, accumulated into Z); every matrix here
//                           is a polynomial in the complex symmetric A, so only the lower tiles are computed and dvr_mirror_kernel copies the lower
//                           triangle over the upper one: every intermediate, and U, is exactly symmetric.
//   launch_dvr_power        R = P4; for every lower bit of s from the top: R = R R, and R = R P4 if the bit is set.
//   dvr_apply_kernel        psi <- U psi: a wave per row, both planes read once, lane-strided partial sums and a fixed butterfly: the same bits on
//                           every repeat.  One launch per application; no flags, no atomics.
// What the absorber took (gple_dvr_flux): per channel c = (side of the box, adiabatic surface) the Hermitian G_c with
// psi^H G_c psi = the population channel c absorbs over s steps, by the power's own recurrence.
//   dvr_loss_kernel         L = I - conj(P) P from the Hermitian product conj(P) P (the loss of one step).
//   dvr_channel_kernel      D_c = (Pi_c L + L Pi_c) / 2: Pi_c is num_pes x num_pes per grid point, a mix of num_pes rows and num_pes columns.
//   sandwich                G_c += conj(R) (X R): T = X R on full tiles (four real products), conj(R) T on the lower tiles (four more),
//                           then the Hermitian form of dvr_mirror_kernel (upper Re copied, upper Im negated, Im diagonal exactly 0).
//   dvr_flux_export_kernel  the padded column-major G_c as the caller's row-major planes (G(r, q) = conj G(q, r): contiguous both sides).
//   dvr_flux_rows_kernel    psi_r^* (G_c psi)_r for four states at a time, a wave per row, the reduction of dvr_apply_kernel;
//   dvr_flux_sum_kernel     the rows summed per (state, channel) in a fixed order.  No atomics, no flags.
#include <algorithm>

#include "gple_kernels.h"

namespace gple
{
	namespace
	{
		typedef double d2 __attribute__((ext_vector_type(2)));
		constexpr double PI_D = 3.141592653589793116; // acos(-1.0) (general.h:34)
		constexpr double HBAR_D = 1.0;                 // general.h:35
		constexpr double ABS_C = 0x1.4f9f94f9f50b1p+1; // sqrt(2) * comp_ellint_1(1 / sqrt(2)) as pes.cpp:61 evaluates it (2.62205755429212)

		// the grid of gple_dvr.hip: x_first + dx * a, rounded twice
		__device__ __forceinline__ double grid_x(double x_first, double dx, long a)
		{
#pragma clang fp contract(off)
			return x_first + dx * static_cast<double>(a);
		}

		__global__ void __launch_bounds__(256) dvr_absorber_kernel(double x_first, double dx, int n, double mass, double xmin, double xmax, double length,
			double* __restrict__ W)
		{
#pragma clang fp contract(off)
			const int a = blockIdx.x * 256 + threadIdx.x;
			if (a >= n) return;
			const double x = grid_x(x_first, dx, a);
			double w = 0.0;
			if (!(x > xmin && x < xmax)) // pes.cpp:86-93
			{
				const double xx = ABS_C * (x <= xmin ? x - xmin : x - xmax) / length;
				const double q = 2.0 * PI_D * HBAR_D / length, cm = ABS_C - xx, cp = ABS_C + xx;
				w = q * q * 2.0 / mass * (1.0 / (cm * cm) + 1.0 / (cp * cp) - 2.0 / (ABS_C * ABS_C));
			}
			W[a] = w;
		}

		// column-major planes: element (r, c) at r + c ld.  G(r, c) = -H(r, c) dt / hbar, d[r] = -W[r mod n] dt / hbar; zero beyond dim
		__global__ void __launch_bounds__(256) dvr_generator_kernel(const double* __restrict__ H, const double* __restrict__ W, int dim, int n, long ld, double dt,
			double* __restrict__ G, double* __restrict__ d)
		{
#pragma clang fp contract(off)
			const long r = blockIdx.x * 256L + threadIdx.x, c = blockIdx.y;
			if (r >= ld) return;
			const bool in = r < dim && c < dim;
			G[r + c * ld] = in ? -H[c * dim + r] * dt / HBAR_D : 0.0; // H is symmetric: either order reads the same
			if (c == 0) d[r] = (r < dim && W) ? -W[r % n] * dt / HBAR_D : 0.0;
		}

		// Q = I + A / 4 (the innermost Horner factor)
		__global__ void __launch_bounds__(256) dvr_horner_first_kernel(const double* __restrict__ G, const double* __restrict__ d, int dim, long ld,
			double* __restrict__ Qr, double* __restrict__ Qi)
		{
#pragma clang fp contract(off)
			const long r = blockIdx.x * 256L + threadIdx.x, c = blockIdx.y;
			if (r >= ld) return;
			Qr[r + c * ld] = (r == c && r < dim) ? 1.0 + d[r] / 4.0 : 0.0;
			Qi[r + c * ld] = G[r + c * ld] / 4.0;
		}

		// N = I + (Re A / k) Q: row r scaled by d[r] / k, the identity added to the real plane (the GEMMs with Im A follow)
		__global__ void __launch_bounds__(256) dvr_horner_scale_kernel(const double* __restrict__ Qr, const double* __restrict__ Qi, const double* __restrict__ d,
			double k, int dim, long ld, double* __restrict__ Nr, double* __restrict__ Ni)
		{
#pragma clang fp contract(off)
			const long r = blockIdx.x * 256L + threadIdx.x, c = blockIdx.y;
			if (r >= ld) return;
			const double f = d[r] / k, one = (r == c && r < dim) ? 1.0 : 0.0;
			Nr[r + c * ld] = one + f * Qr[r + c * ld];
			Ni[r + c * ld] = f * Qi[r + c * ld];
		}

		// (r, c) <- (c, r) for r < c, both planes (blockIdx.z): a 32 x 32 tile of the lower triangle goes through LDS, so that the read (along the
		// column of the lower tile) and the write (along the column of the upper one) are both contiguous.  ld is a multiple of 64: no edges
		// HERM: the Hermitian form: the upper half of the imaginary plane is negated and its diagonal written as exact zero
		template <bool HERM>
		__global__ void __launch_bounds__(256) dvr_mirror_kernel(double* __restrict__ Zr, double* __restrict__ Zi, long ld)
		{
			if (blockIdx.x > blockIdx.y) return; // tile rows r0.., tile columns c0.. of the upper triangle, diagonal tiles included
			__shared__ double tile[32][33];
			double* Z = blockIdx.z ? Zi : Zr;
			const long r0 = blockIdx.x * 32L, c0 = blockIdx.y * 32L;
			const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
#pragma unroll
			for (int q = 0; q < 4; ++q) tile[y + 8 * q][x] = Z[(c0 + x) + (r0 + y + 8 * q) * ld]; // (c0 + x, r0 + y'): the lower tile, x along its column
			__syncthreads();
#pragma unroll
			for (int q = 0; q < 4; ++q)
			{
				const long r = r0 + x, c = c0 + y + 8 * q;
				if (r < c) Z[r + c * ld] = (HERM && blockIdx.z) ? -tile[x][y + 8 * q] : tile[x][y + 8 * q];
				else if (HERM && blockIdx.z && r == c) Z[r + c * ld] = 0.0;
			}
		}

		// C (+)= alpha X Y on column-major ld x ld planes, the lower tiles only
		hipError_t real_product(hipStream_t s, const double* X, const double* Y, double* C, long ld, double alpha, double beta, bool lower = true)
		{
			GemmDesc g{};
			g.A = X, g.lda = ld, g.a_kmajor = false; // A(m, k) = X(m, k) at m + k ld
			g.B = Y, g.ldb = ld, g.b_kmajor = true;  // B(n, k) = Y(k, n) at k + n ld
			g.C = C, g.ldc = ld, g.c_trans = false;
			g.M = g.N = g.K = static_cast<int>(ld), g.batch = 1, g.alpha = alpha, g.beta = beta, g.krange = K_FULL, g.lower_only = lower;
			return launch_gemm(s, g, gemm_pick_tile(ld, ld, 1, lower));
		}
		hipError_t mirror(hipStream_t s, double* Zr, double* Zi, long ld, bool hermitian = false)
		{
			const dim3 grid(static_cast<unsigned>(ld / 32), static_cast<unsigned>(ld / 32), 2);
			if (hermitian) hipLaunchKernelGGL(dvr_mirror_kernel<true>, grid, dim3(256), 0, s, Zr, Zi, ld);
			else hipLaunchKernelGGL(dvr_mirror_kernel<false>, grid, dim3(256), 0, s, Zr, Zi, ld);
			return hipGetLastError();
		}
		// Z = X Y: Re Z = Xr Yr - Xi Yi, Im Z = Xr Yi + Xi Yr (four products: the three-multiplication form costs accuracy); Z may alias neither
		hipError_t complex_product(hipStream_t s, const double* X, const double* Y, double* Z, long ld)
		{
			const long pl = ld * ld;
			hipError_t err;
			if ((err = real_product(s, X, Y, Z, ld, 1.0, 0.0)) != hipSuccess) return err;
			if ((err = real_product(s, X + pl, Y + pl, Z, ld, -1.0, 1.0)) != hipSuccess) return err;
			if ((err = real_product(s, X, Y + pl, Z + pl, ld, 1.0, 0.0)) != hipSuccess) return err;
			if ((err = real_product(s, X + pl, Y, Z + pl, ld, 1.0, 1.0)) != hipSuccess) return err;
			return mirror(s, Z, Z + pl, ld);
		}

		// out[row] = sum_c U(row, c) in[c]: a wave per row, lane l sums the columns l, l + 64, ... in ascending order, then a fixed butterfly
		__global__ void __launch_bounds__(256) dvr_apply_kernel(const double* __restrict__ Ur, const double* __restrict__ Ui, int dim, const double* __restrict__ in,
			double* __restrict__ out)
		{
			const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
			if (row >= dim) return;
			const double* __restrict__ ur = Ur + static_cast<long>(row) * dim;
			const double* __restrict__ ui = Ui + static_cast<long>(row) * dim;
			double re = 0.0, im = 0.0;
#pragma unroll 4
			for (int c = lane; c < dim; c += 64)
			{
				const double a = ur[c], b = ui[c];
				const d2 v = *reinterpret_cast<const d2*>(in + 2 * static_cast<long>(c));
				re += a * v.x - b * v.y;
				im += a * v.y + b * v.x;
			}
#pragma unroll
			for (int off = 32; off > 0; off >>= 1)
			{
				re += __shfl_xor(re, off, 64);
				im += __shfl_xor(im, off, 64);
			}
			if (lane == 0) *reinterpret_cast<d2*>(out + 2 * static_cast<long>(row)) = (d2){re, im};
		}

		// psi_adia[t][k n + a] = sum_j basis(a; j, k) psi_dia[t][j n + a]   (main.cpp:221), (re, im) pairs on both sides
		template <int NP>
		__global__ void __launch_bounds__(256) dvr_adiabatic_kernel(const double* __restrict__ dia, int n, const double* __restrict__ basis, double* __restrict__ psi)
		{
			const int a = blockIdx.x * 256 + threadIdx.x;
			if (a >= n) return;
			const long base = static_cast<long>(blockIdx.y) * 2 * NP * n;
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				double re = 0.0, im = 0.0;
#pragma unroll
				for (int j = 0; j < NP; ++j)
				{
					const double b = basis[(static_cast<long>(a) * NP + j) * NP + k];
					const d2 v = *reinterpret_cast<const d2*>(dia + base + 2 * (static_cast<long>(j) * n + a));
					re += b * v.x, im += b * v.y;
				}
				*reinterpret_cast<d2*>(psi + base + 2 * (static_cast<long>(k) * n + a)) = (d2){re, im};
			}
		}

		// ---- what the absorber took ----------------------------------------------------------------------------------------------------------
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
				if ((a < n_left) == (side == 0))
				{
					const double* b = basis + static_cast<long>(a) * NP * NP;
#pragma unroll
					for (int j = 0; j < NP; ++j)
					{
						const double w = b[m * NP + k] * b[j * NP + k];
						const long at = (static_cast<long>(j) * n + a) + c * ld;
						re += w * Lr[at], im += w * Li[at];
					}
				}
				if ((ap < n_left) == (side == 0))
				{
					const double* b = basis + static_cast<long>(ap) * NP * NP;
#pragma unroll
					for (int j = 0; j < NP; ++j)
					{
						const double w = b[mp * NP + k] * b[j * NP + k];
						const long at = r + (static_cast<long>(j) * n + ap) * ld;
						re += w * Lr[at], im += w * Li[at];
					}
				}
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
			const long pl = static_cast<long>(dim) * dim;
			const double* __restrict__ gr = G + 2 * c * pl + static_cast<long>(row) * dim;
			const double* __restrict__ gi = gr + pl;
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
#pragma unroll
					for (int off = 32; off > 0; off >>= 1)
					{
						re[g] += __shfl_xor(re[g], off, 64);
						im[g] += __shfl_xor(im[g], off, 64);
					}
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
			__shared__ double sums[256];
			const double* p = partial + static_cast<long>(blockIdx.x) * dim;
			double acc = 0.0;
			for (int r = threadIdx.x; r < dim; r += 256) acc += p[r];
			sums[threadIdx.x] = acc;
			__syncthreads();
			for (int half = 128; half > 0; half >>= 1)
			{
				if (static_cast<int>(threadIdx.x) < half) sums[threadIdx.x] += sums[threadIdx.x + half];
				__syncthreads();
			}
			if (threadIdx.x == 0) absorbed[blockIdx.x] = sums[0];
		}
	} // namespace

	hipError_t launch_dvr_absorber(hipStream_t s, double x_first, double dx, int n, double mass, double xmin, double xmax, double length, double* W)
	{
		hipLaunchKernelGGL(dvr_absorber_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x_first, dx, n, mass, xmin, xmax, length, W);
		return hipGetLastError();
	}

	hipError_t launch_dvr_square(hipStream_t s, const double* X, double* Z, long ld) { return complex_product(s, X, X, Z, ld); }

	size_t dvr_power_work_doubles(int num_pes, int n)
	{
		const size_t ld = round_up(static_cast<size_t>(num_pes) * n, 64);
		return 7 * ld * ld + ld;
	}
	hipError_t launch_dvr_power(Ctx* ctx, hipStream_t s, int num_pes, int n, const double* H, const double* W, double dt, long n_steps, double* work,
		const double** result, const DvrFlux* flux)
	{
		if ((num_pes != 2 && num_pes != 3) || n_steps < 1) return hipErrorInvalidValue;
		const int dim = num_pes * n;
		const long ld = static_cast<long>(round_up(dim, 64)), pl = ld * ld;
		if (ld > DVR_POWER_MAX_LD) return hipErrorInvalidValue; // the set-up kernels take a column per blockIdx.y
		double* G = work;
		double* P = G + pl;
		double* buf[2] = {P + 2 * pl, P + 4 * pl};
		double* d = P + 6 * pl;
		const dim3 grid(static_cast<unsigned>((ld + 255) / 256), static_cast<unsigned>(ld)), block(256);
		hipError_t err;
		hipLaunchKernelGGL(dvr_generator_kernel, grid, block, 0, s, H, W, dim, n, ld, dt, G, d);
		if ((err = hipGetLastError()) != hipSuccess) return err;
		const double* R = P;
		// what the absorber took: G_c += conj(Rm) (X Rm), T = X Rm on full tiles, the Hermitian product on the lower ones
		const int channels = 2 * num_pes;
		double* const fL = flux ? flux->work : nullptr;
		double* const fD = flux ? fL + 2 * pl : nullptr;
		double* const fT = flux ? fL + 4 * pl : nullptr;
		double* const fG = flux ? fL + 6 * pl : nullptr;
		auto hermitian_product = [&](const double* X, const double* Y, double* Z, double beta) -> hipError_t { // Z = beta Z + conj(X) Y, X symmetric
			if ((err = real_product(s, X, Y, Z, ld, 1.0, beta)) != hipSuccess) return err;
			if ((err = real_product(s, X + pl, Y + pl, Z, ld, 1.0, 1.0)) != hipSuccess) return err;
			if ((err = real_product(s, X, Y + pl, Z + pl, ld, 1.0, beta)) != hipSuccess) return err;
			return real_product(s, X + pl, Y, Z + pl, ld, -1.0, 1.0);
		};
		auto sandwich = [&](const double* X, const double* Rm, double* Gc) -> hipError_t {
			if ((err = real_product(s, X, Rm, fT, ld, 1.0, 0.0, false)) != hipSuccess) return err;
			if ((err = real_product(s, X + pl, Rm + pl, fT, ld, -1.0, 1.0, false)) != hipSuccess) return err;
			if ((err = real_product(s, X, Rm + pl, fT + pl, ld, 1.0, 0.0, false)) != hipSuccess) return err;
			if ((err = real_product(s, X + pl, Rm, fT + pl, ld, 1.0, 1.0, false)) != hipSuccess) return err;
			if ((err = hermitian_product(Rm, fT, Gc, 1.0)) != hipSuccess) return err;
			return mirror(s, Gc, Gc + pl, ld, true);
		};
		auto channel = [&](int c, double* D) -> hipError_t { // D_c into D
			if (num_pes == 2) hipLaunchKernelGGL(dvr_channel_kernel<2>, grid, block, 0, s, fL, fL + pl, flux->basis, n, flux->n_left, c / 2, c % 2, ld, D, D + pl);
			else hipLaunchKernelGGL(dvr_channel_kernel<3>, grid, block, 0, s, fL, fL + pl, flux->basis, n, flux->n_left, c / 3, c % 3, ld, D, D + pl);
			if ((err = hipGetLastError()) != hipSuccess) return err;
			return mirror(s, D, D + pl, ld, true);
		};
		auto products = [&]() -> hipError_t {
		// Horner: Q1 = I + A/4 -> buf[0]; Q2 = I + A/3 Q1 -> buf[1]; Q3 = I + A/2 Q2 -> buf[0]; P4 = I + A Q3 -> P
		hipLaunchKernelGGL(dvr_horner_first_kernel, grid, block, 0, s, G, d, dim, ld, buf[0], buf[0] + pl);
		if ((err = hipGetLastError()) != hipSuccess) return err;
		const double* Q = buf[0];
		double* const target[3] = {buf[1], buf[0], P};
		for (int step = 0; step < 3; ++step)
		{
			const double k = 3.0 - step;
			double* N = target[step];
			hipLaunchKernelGGL(dvr_horner_scale_kernel, grid, block, 0, s, Q, Q + pl, d, k, dim, ld, N, N + pl);
			if ((err = hipGetLastError()) != hipSuccess) return err;
			// (i G / k) (Qr + i Qi) = -(G Qi) / k + i (G Qr) / k
			if ((err = real_product(s, G, Q + pl, N, ld, -1.0 / k, 1.0)) != hipSuccess) return err;
			if ((err = real_product(s, G, Q, N + pl, ld, 1.0 / k, 1.0)) != hipSuccess) return err;
			if ((err = mirror(s, N, N + pl, ld)) != hipSuccess) return err;
			Q = N;
		}
		// left-to-right binary power: R = P; per lower bit from the top R = R R, and R = R P where the bit is set
		int top = 0;
		while ((n_steps >> (top + 1)) != 0) ++top;
		int next = 0;
		if (flux) // L = I - conj(P) P, G_c = D_c: one step
		{
			if ((err = hermitian_product(P, P, fL, 0.0)) != hipSuccess) return err;
			hipLaunchKernelGGL(dvr_loss_kernel, grid, block, 0, s, fL, fL + pl, dim, ld);
			if ((err = hipGetLastError()) != hipSuccess) return err;
			if ((err = mirror(s, fL, fL + pl, ld, true)) != hipSuccess) return err;
			for (int c = 0; c < channels; ++c)
				if ((err = channel(c, fG + 2 * c * pl)) != hipSuccess) return err;
		}
		for (int bit = top - 1; bit >= 0; --bit)
		{
			for (int c = 0; flux && c < channels; ++c) // the steps m .. 2m - 1 are the first m seen through R = P^m
				if ((err = sandwich(fG + 2 * c * pl, R, fG + 2 * c * pl)) != hipSuccess) return err;
			if ((err = complex_product(s, R, R, buf[next], ld)) != hipSuccess) return err;
			R = buf[next], next ^= 1;
			if ((n_steps >> bit) & 1)
			{
				for (int c = 0; flux && c < channels; ++c) // one more step after R
				{
					if ((err = channel(c, fD)) != hipSuccess) return err;
					if ((err = sandwich(fD, R, fG + 2 * c * pl)) != hipSuccess) return err;
				}
				if ((err = complex_product(s, R, P, buf[next], ld)) != hipSuccess) return err;
				R = buf[next], next ^= 1;
			}
		}
		return hipSuccess;
		};
		const int timer = flux ? GPLE_TIMER_DVR_FLUX : GPLE_TIMER_DVR_POWER;
		if (ctx) timer_start(ctx, timer);
		err = products();
		if (ctx) timer_stop(ctx, timer); // on the error path too: no span stays open
		*result = R;
		return err;
	}

	size_t dvr_flux_work_doubles(int num_pes, int n)
	{
		const size_t ld = round_up(static_cast<size_t>(num_pes) * n, 64);
		return (6 + 4 * static_cast<size_t>(num_pes)) * ld * ld;
	}
	hipError_t launch_dvr_flux_export(hipStream_t s, int num_pes, int n, const DvrFlux& flux, double* out)
	{
		const int dim = num_pes * n;
		const long ld = static_cast<long>(round_up(dim, 64)), pl = ld * ld;
		const dim3 grid((dim + 255) / 256, dim, 2);
		for (int c = 0; c < 2 * num_pes; ++c)
		{
			const double* Gc = flux.work + (6 + 2 * c) * pl;
			hipLaunchKernelGGL(dvr_flux_export_kernel, grid, dim3(256), 0, s, Gc, Gc + pl, dim, ld, out + 2L * c * dim * dim);
		}
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

	hipError_t launch_dvr_apply(hipStream_t s, int num_pes, int n, const double* U, const double* psi0, int T, const double* basis, double* scratch, double* psi)
	{
		if (num_pes != 2 && num_pes != 3) return hipErrorInvalidValue;
		const int dim = num_pes * n;
		double* dia = basis ? scratch : psi;
		const double* in = psi0;
		for (int k = 0; k < T; ++k)
		{
			double* out = dia + static_cast<long>(k) * 2 * dim;
			hipLaunchKernelGGL(dvr_apply_kernel, dim3((dim + 3) / 4), dim3(256), 0, s, U, U + static_cast<long>(dim) * dim, dim, in, out);
			in = out;
		}
		hipError_t err = hipGetLastError();
		if (err != hipSuccess || !basis) return err;
		const dim3 grid((n + 255) / 256, T);
		if (num_pes == 2) hipLaunchKernelGGL(dvr_adiabatic_kernel<2>, grid, dim3(256), 0, s, dia, n, basis, psi);
		else hipLaunchKernelGGL(dvr_adiabatic_kernel<3>, grid, dim3(256), 0, s, dia, n, basis, psi);
		return hipGetLastError();
	}
} // namespace gple
