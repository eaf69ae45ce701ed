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
				if (r < c) Z[r + c * ld] = tile[x][y + 8 * q];
			}
		}

		// C (+)= alpha X Y on column-major ld x ld planes, the lower tiles only
		hipError_t real_product(hipStream_t s, const double* X, const double* Y, double* C, long ld, double alpha, double beta)
		{
			GemmDesc g{};
			g.A = X, g.lda = ld, g.a_kmajor = false; // A(m, k) = X(m, k) at m + k ld
			g.B = Y, g.ldb = ld, g.b_kmajor = true;  // B(n, k) = Y(k, n) at k + n ld
			g.C = C, g.ldc = ld, g.c_trans = false;
			g.M = g.N = g.K = static_cast<int>(ld), g.batch = 1, g.alpha = alpha, g.beta = beta, g.krange = K_FULL, g.lower_only = 1;
			return launch_gemm(s, g, gemm_pick_tile(ld, ld, 1, true));
		}
		hipError_t mirror(hipStream_t s, double* Zr, double* Zi, long ld)
		{
			hipLaunchKernelGGL(dvr_mirror_kernel, dim3(static_cast<unsigned>(ld / 32), static_cast<unsigned>(ld / 32), 2), dim3(256), 0, s, Zr, Zi, ld);
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
	} // namespace

	hipError_t launch_dvr_absorber(hipStream_t s, double x_first, double dx, int n, double mass, double xmin, double xmax, double length, double* W)
	{
		hipLaunchKernelGGL(dvr_absorber_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x_first, dx, n, mass, xmin, xmax, length, W);
		return hipGetLastError();
	}

	size_t dvr_power_work_doubles(int num_pes, int n)
	{
		const size_t ld = round_up(static_cast<size_t>(num_pes) * n, 64);
		return 7 * ld * ld + ld;
	}
	hipError_t launch_dvr_power(Ctx* ctx, hipStream_t s, int num_pes, int n, const double* H, const double* W, double dt, long n_steps, double* work,
		const double** result)
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
		for (int bit = top - 1; bit >= 0; --bit)
		{
			if ((err = complex_product(s, R, R, buf[next], ld)) != hipSuccess) return err;
			R = buf[next], next ^= 1;
			if ((n_steps >> bit) & 1)
			{
				if ((err = complex_product(s, R, P, buf[next], ld)) != hipSuccess) return err;
				R = buf[next], next ^= 1;
			}
		}
		return hipSuccess;
		};
		if (ctx) timer_start(ctx, GPLE_TIMER_DVR_POWER);
		err = products();
		if (ctx) timer_stop(ctx, GPLE_TIMER_DVR_POWER); // on the error path too: no span stays open
		*result = R;
		return err;
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
