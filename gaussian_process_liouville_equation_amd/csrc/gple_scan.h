// gple_scan.h — the workgroup-wide exclusive prefix sum of 64-bit integers that the text kernels share (gple_format.hip, gple_parse.hip): sums of
// integers in thread order, nothing atomic.
#pragma once
#include <hip/hip_runtime.h>

namespace gple
{
	using u64 = unsigned long long;
	__device__ inline u64 shfl_up64(u64 v, int delta)
	{
		const unsigned lo = __shfl_up(static_cast<unsigned>(v), delta), hi = __shfl_up(static_cast<unsigned>(v >> 32), delta);
		return (static_cast<u64>(hi) << 32) | lo;
	}
	// exclusive prefix of v over the workgroup's threads in thread order, and the workgroup's total; wave_sums: THREADS / 64 words of LDS
	template <int THREADS>
	__device__ inline u64 block_exclusive_scan(u64 v, u64* wave_sums, u64* total)
	{
		const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
		u64 inclusive = v;
		for (int d = 1; d < 64; d <<= 1)
		{
			const u64 up = shfl_up64(inclusive, d);
			if (lane >= d) inclusive += up;
		}
		if (lane == 63) wave_sums[wave] = inclusive;
		__syncthreads();
		u64 before = 0, all = 0;
		for (int w = 0; w < THREADS / 64; ++w)
		{
			const u64 s = wave_sums[w];
			if (w < wave) before += s;
			all += s;
		}
		__syncthreads(); // wave_sums may be written again
		*total = all;
		return before + inclusive - v;
	}
} // namespace gple
