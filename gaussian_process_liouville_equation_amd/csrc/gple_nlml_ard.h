// gple_nlml_ard.h — the ARD kernel of the NLML path as its device kernels evaluate it (gple_nlml.hip, gple_nlml_batch.hip): one definition,
// so that the single-problem and the batched evaluation form the same Gram entries.
#pragma once
#include <hip/hip_runtime.h>

namespace gple
{
	// lower-triangular ARD weight matrix W = [[a, 0], [c, b]]; u = W^T (x - y): u0 = a e0 + c e1, u1 = b e1
	struct ArdW
	{
		double a, c, b;
	};
	__device__ __forceinline__ double ard(double a0, double a1, double b0, double b1, ArdW w, double* u0 = nullptr, double* u1 = nullptr)
	{
		const double e0 = __dsub_rn(a0, b0), e1 = __dsub_rn(a1, b1);
		const double d0 = __dadd_rn(__dmul_rn(w.a, e0), __dmul_rn(w.c, e1)), d1 = __dmul_rn(w.b, e1);
		if (u0) *u0 = d0, *u1 = d1;
		return exp(__ddiv_rn(-__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), 2.0));
	}
} // namespace gple
