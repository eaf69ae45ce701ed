// gple_philox.h — the counter-based random numbers of the library as device functions, shared by the Monte-Carlo kernels (gple_evolve.hip)
// and the point selection of the reconstruction (gple_recon.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gple
{
	// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) -------------------
	__device__ __forceinline__ void philox4x32(unsigned (&c)[4], unsigned k0, unsigned k1)
	{
#pragma unroll
		for (int round = 0; round < 10; ++round)
		{
			const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
			const unsigned hi0 = static_cast<unsigned>(p0 >> 32), lo0 = static_cast<unsigned>(p0), hi1 = static_cast<unsigned>(p1 >> 32), lo1 = static_cast<unsigned>(p1);
			const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
			c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
			k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
		}
	}
	__device__ __forceinline__ double unit53(unsigned hi, unsigned lo)
	{
		return static_cast<double>(((static_cast<unsigned long long>(hi) << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
	}
} // namespace gple
