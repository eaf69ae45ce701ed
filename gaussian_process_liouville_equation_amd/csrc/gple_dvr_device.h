// gple_dvr_device.h — what the kernels of the exact DVR dynamics share (gple_dvr.hip, gple_dvr_power.hip, gple_dvr_flux.hip, gple_dvr_spectrum.hip):
// the constants of the reference, its grid, and the fixed-order reductions.
//
// Floating-point contraction is a property of the function body an expression is written in, and it stays with the expression when the body is
// inlined.  grid_x and projector_mix hold products and are written with contraction off, like every kernel that calls them; wave_sum and
// block_sum_256 only add, so that they serve kernels of either setting.
#pragma once
#include <hip/hip_runtime.h>

namespace gple
{
	namespace dvr
	{
		typedef double d2 __attribute__((ext_vector_type(2)));
		constexpr double PI_D = 3.141592653589793116; // acos(-1.0) (general.h:34)
		constexpr double HBAR_D = 1.0;                 // general.h:35

		// x grid of the reference (main.cpp:108 without absorbing region): x_first + dx * a, rounded twice (never contracted to an fma, so that a
		// grid built on the host with the same two operations has the same bits)
		__device__ __forceinline__ double grid_x(double x_first, double dx, long a)
		{
#pragma clang fp contract(off)
			return x_first + dx * static_cast<double>(a);
		}

		// the complex (re, im) summed over the 64 lanes of a wave, on every lane: a fixed butterfly, the same bits on every repeat
		__device__ __forceinline__ void wave_sum(double& re, double& im)
		{
#pragma unroll
			for (int off = 32; off > 0; off >>= 1)
			{
				re += __shfl_xor(re, off, 64);
				im += __shfl_xor(im, off, 64);
			}
		}

		// the sum of one value per thread of a 256-thread block, by a fixed tree through LDS; every thread calls, thread 0 has the result
		__device__ __forceinline__ double block_sum_256(double acc)
		{
			__shared__ double sums[256];
			sums[threadIdx.x] = acc;
			__syncthreads();
			for (int half = 128; half > 0; half >>= 1)
			{
				if (static_cast<int>(threadIdx.x) < half) sums[threadIdx.x] += sums[threadIdx.x + half];
				__syncthreads();
			}
			return sums[0];
		}

		// (re, im) += sum_j (b[m NP + k] b[j NP + k]) X[first + j step]: the projector onto the adiabatic surface k at one grid point (b: its
		// NP x NP block of the basis) mixing the NP rows (step = n) or columns (step = n ld) of that grid point, for the component m
		template <int NP>
		__device__ __forceinline__ void projector_mix(const double* b, int m, int k, const double* Xr, const double* Xi, long first, long step, double& re,
			double& im)
		{
#pragma clang fp contract(off)
#pragma unroll
			for (int j = 0; j < NP; ++j)
			{
				const double w = b[m * NP + k] * b[j * NP + k];
				const long at = first + j * step;
				re += w * Xr[at], im += w * Xi[at];
			}
		}
	} // namespace dvr
} // namespace gple
