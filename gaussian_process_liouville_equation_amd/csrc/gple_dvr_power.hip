// gple_dvr_power.hip — the absorbing boundary of the exact DVR dynamics (schrodinger_equation/ of the reference, general.h:88-93):
// classical RK4 on i hbar dpsi/dt = (H - i W) psi (the method general.cpp:233-236 documents) as powers of its one-step propagator.
//
//   dvr_absorber_kernel     absorbing_potential (pes.cpp:64-93) on the grid, x <= xmin on the left-hand branch (W >= 0 everywhere).
//   dvr_generator_kernel    A = -(W + i H) dt / hbar: Re A is diagonal (a vector), Im A = G an ld x ld plane, ld = dim rounded up to 64, zero padded.
//   dvr_horner_*            P4(A) = I + A (I + A/2 (I + A/3 (I + A/4))): a product with A/k is a row scaling by Re A / k (with the identity added,
//                           dvr_horner_scale_kernel) plus two real GEMMs with G (alpha = -+ 1/k, beta = 1).  launch_dvr_p4 is the generator and these.
//   dvr_complex_product     Z = beta Z + X Y or conj(X) Y on (Re, Im) planes as four real products through launch_gemm (alpha = +-1, accumulated into
//                           Z), on the lower tiles or on all: the one complex product of the power, the flux (gple_dvr_flux.hip) and the spectrum
//                           (gple_dvr_spectrum.hip).  Every matrix of the power is a polynomial in the complex symmetric A, so launch_dvr_square and the
//                           walk compute only the lower tiles and dvr_mirror_kernel copies the lower triangle over the upper one: every
//                           intermediate, and U, is exactly symmetric.
//   launch_dvr_power        R = P4; for every lower bit of s from the top: R = R R, and R = R P4 if the bit is set (walk); the flux recurrence of
//                           gple_dvr_flux.hip rides along at three places of the walk.
//   dvr_apply_kernel        psi <- U psi: a wave per row, both planes read once, lane-strided partial sums and a fixed butterfly: the same bits on
//                           every repeat.  One launch per application; no flags, no atomics.
#include "gple_dvr_device.h"
#include "gple_kernels.h"

namespace gple
{
	namespace
	{
		using namespace dvr;
		constexpr double ABS_C = 0x1.4f9f94f9f50b1p+1; // sqrt(2) * comp_ellint_1(1 / sqrt(2)) as pes.cpp:61 evaluates it (2.62205755429212)

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

		// C = beta C + alpha X Y on column-major planes: X ld x ld, Y and C ld x cols (leading dimension ld); lower: the lower tiles only
		hipError_t real_product(hipStream_t s, const double* X, const double* Y, double* C, long ld, long cols, double alpha, double beta, bool lower)
		{
			GemmDesc g{};
			g.A = X, g.lda = ld, g.a_kmajor = false; // A(m, k) = X(m, k) at m + k ld
			g.B = Y, g.ldb = ld, g.b_kmajor = true;  // B(n, k) = Y(k, n) at k + n ld
			g.C = C, g.ldc = ld, g.c_trans = false;
			g.M = g.K = static_cast<int>(ld), g.N = static_cast<int>(cols), g.batch = 1, g.alpha = alpha, g.beta = beta, g.krange = K_FULL, g.lower_only = lower;
			return launch_gemm(s, g, gemm_pick_tile(ld, cols, 1, lower));
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
			wave_sum(re, im);
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

		// dim and ld of a system, if the set-up kernels can take it (a column per blockIdx.y)
		bool power_dims(int num_pes, int n, int* dim, long* ld)
		{
			*dim = num_pes * n;
			*ld = static_cast<long>(round_up(*dim, 64));
			return (num_pes == 2 || num_pes == 3) && *ld <= DVR_POWER_MAX_LD;
		}

		hipError_t generator(hipStream_t s, int dim, int n, long ld, const double* H, const double* W, double dt, const DvrPowerWork& w)
		{
			hipLaunchKernelGGL(dvr_generator_kernel, dvr_plane_grid(ld), dim3(256), 0, s, H, W, dim, n, ld, dt, w.G, w.d);
			return hipGetLastError();
		}
		// Q1 = I + A/4 -> buf[0]; Q2 = I + A/3 Q1 -> buf[1]; Q3 = I + A/2 Q2 -> buf[0]; P4 = I + A Q3 -> P
		hipError_t horner(hipStream_t s, int dim, long ld, const DvrPowerWork& w)
		{
			const dim3 grid = dvr_plane_grid(ld), block(256);
			hipError_t err;
			hipLaunchKernelGGL(dvr_horner_first_kernel, grid, block, 0, s, w.G, w.d, dim, ld, w.buf[0].re, w.buf[0].im);
			if ((err = hipGetLastError()) != hipSuccess) return err;
			DvrPlanes Q = w.buf[0];
			const DvrPlanes target[3] = {w.buf[1], w.buf[0], w.P};
			for (int step = 0; step < 3; ++step)
			{
				const double k = 3.0 - step;
				const DvrPlanes N = target[step];
				hipLaunchKernelGGL(dvr_horner_scale_kernel, grid, block, 0, s, Q.re, Q.im, w.d, k, dim, ld, N.re, N.im);
				if ((err = hipGetLastError()) != hipSuccess) return err;
				// (i G / k) (Qr + i Qi) = -(G Qi) / k + i (G Qr) / k
				if ((err = real_product(s, w.G, Q.im, N.re, ld, ld, -1.0 / k, 1.0, true)) != hipSuccess) return err;
				if ((err = real_product(s, w.G, Q.re, N.im, ld, ld, 1.0 / k, 1.0, true)) != hipSuccess) return err;
				if ((err = launch_dvr_mirror(s, N, ld, false)) != hipSuccess) return err;
				Q = N;
			}
			return hipSuccess;
		}

		// Z = X Y for complex symmetric X and Y that commute: the lower tiles, then the mirror
		hipError_t symmetric_product(hipStream_t s, DvrPlanes X, DvrPlanes Y, DvrPlanes Z, long ld)
		{
			const hipError_t err = dvr_complex_product(s, X, Y, Z, ld, ld, 0.0, false, true);
			return err != hipSuccess ? err : launch_dvr_mirror(s, Z, ld, false);
		}

		// left-to-right binary power: R = P; per lower bit of n_steps from the top R = R R, and R = R P where the bit is set.  The dvr_flux_* calls
		// are the flux recurrence beside it (f.flux null: none, they do nothing).  *R follows the walk, also where it stops at an error
		hipError_t walk(const DvrFluxRun& f, const DvrPowerWork& w, long n_steps, DvrPlanes* R)
		{
			int top = 0;
			while ((n_steps >> (top + 1)) != 0) ++top;
			int next = 0;
			hipError_t err;
			if ((err = dvr_flux_first_step(f, w.P)) != hipSuccess) return err;
			for (int bit = top - 1; bit >= 0; --bit)
			{
				if ((err = dvr_flux_before_square(f, *R)) != hipSuccess) return err;
				if ((err = symmetric_product(f.s, *R, *R, w.buf[next], f.ld)) != hipSuccess) return err;
				*R = w.buf[next], next ^= 1;
				if ((n_steps >> bit) & 1)
				{
					if ((err = dvr_flux_before_multiply(f, *R)) != hipSuccess) return err;
					if ((err = symmetric_product(f.s, *R, w.P, w.buf[next], f.ld)) != hipSuccess) return err;
					*R = w.buf[next], next ^= 1;
				}
			}
			return hipSuccess;
		}
	} // namespace

	hipError_t launch_dvr_absorber(hipStream_t s, double x_first, double dx, int n, double mass, double xmin, double xmax, double length, double* W)
	{
		hipLaunchKernelGGL(dvr_absorber_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x_first, dx, n, mass, xmin, xmax, length, W);
		return hipGetLastError();
	}

	hipError_t dvr_complex_product(hipStream_t s, DvrPlanes X, DvrPlanes Y, DvrPlanes Z, long ld, long cols, double beta, bool conj_x, bool lower)
	{
		const double sign = conj_x ? -1.0 : 1.0; // Re Z = Xr Yr -+ Xi Yi, Im Z = Xr Yi +- Xi Yr
		hipError_t err;
		if ((err = real_product(s, X.re, Y.re, Z.re, ld, cols, 1.0, beta, lower)) != hipSuccess) return err;
		if ((err = real_product(s, X.im, Y.im, Z.re, ld, cols, -sign, 1.0, lower)) != hipSuccess) return err;
		if ((err = real_product(s, X.re, Y.im, Z.im, ld, cols, 1.0, beta, lower)) != hipSuccess) return err;
		return real_product(s, X.im, Y.re, Z.im, ld, cols, sign, 1.0, lower);
	}
	hipError_t launch_dvr_mirror(hipStream_t s, DvrPlanes Z, long ld, bool hermitian)
	{
		const dim3 grid(static_cast<unsigned>(ld / 32), static_cast<unsigned>(ld / 32), 2);
		if (hermitian) hipLaunchKernelGGL(dvr_mirror_kernel<true>, grid, dim3(256), 0, s, Z.re, Z.im, ld);
		else hipLaunchKernelGGL(dvr_mirror_kernel<false>, grid, dim3(256), 0, s, Z.re, Z.im, ld);
		return hipGetLastError();
	}
	hipError_t launch_dvr_square(hipStream_t s, DvrPlanes X, DvrPlanes Z, long ld) { return symmetric_product(s, X, X, Z, ld); }

	DvrPowerWork dvr_power_layout(double* work, long ld)
	{
		const size_t plane = static_cast<size_t>(ld) * ld;
		DvrCarve c{work};
		DvrPowerWork w{};
		w.G = c.take(plane);
		w.P = c.planes(plane);
		w.buf[0] = c.planes(plane);
		w.buf[1] = c.planes(plane);
		w.d = c.take(ld);
		w.doubles = c.used;
		return w;
	}
	size_t dvr_power_work_doubles(int num_pes, int n) { return dvr_power_layout(nullptr, static_cast<long>(round_up(static_cast<size_t>(num_pes) * n, 64))).doubles; }

	hipError_t launch_dvr_p4(hipStream_t s, int num_pes, int n, const double* H, const double* W, double dt, const DvrPowerWork& w)
	{
		int dim;
		long ld;
		if (!power_dims(num_pes, n, &dim, &ld)) return hipErrorInvalidValue;
		const hipError_t err = generator(s, dim, n, ld, H, W, dt, w);
		return err != hipSuccess ? err : horner(s, dim, ld, w);
	}

	hipError_t launch_dvr_power(Ctx* ctx, hipStream_t s, int num_pes, int n, const double* H, const double* W, double dt, long n_steps, double* work,
		DvrPlanes* result, const DvrFlux* flux)
	{
		int dim;
		long ld;
		if (!power_dims(num_pes, n, &dim, &ld) || n_steps < 1) return hipErrorInvalidValue;
		const DvrPowerWork w = dvr_power_layout(work, ld);
		hipError_t err = generator(s, dim, n, ld, H, W, dt, w); // before the timer's span: it times the products
		if (err != hipSuccess) return err;
		const DvrFluxRun f{s, num_pes, n, ld, flux, flux ? dvr_flux_layout(flux->work, ld, num_pes) : DvrFluxWork{}};
		const int timer = flux ? GPLE_TIMER_DVR_FLUX : GPLE_TIMER_DVR_POWER;
		*result = w.P;
		if (ctx) timer_start(ctx, timer);
		if ((err = horner(s, dim, ld, w)) == hipSuccess) err = walk(f, w, n_steps, result);
		if (ctx) timer_stop(ctx, timer); // on the error path too: no span stays open
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
