// gple_pes_n.h — the N-level potentials and their adiabatic states as device functions, shared by the step loop (gple_evolve_n.hip) and
// the exact DVR dynamics (gple_dvr.hip): pes.cpp's diabatic_potential for models 0-2 (at three levels plus the uncoupled third diabat at
// V = 0), the three-level TSAC model of this library (model 3), a cyclic Jacobi eigen-solver and the library's sign convention of the
// adiabatic states (ascending energy, last non-zero component of every eigenvector positive; pes.cpp:73-96 at two levels).
//
// A user model (id >= GPLE_PES_USER) is a table on a uniform grid, evaluated by table_diabatic_n: a cubic Hermite interpolant of the
// diabatic matrix from its values and derivatives at the nodes, continued linearly beyond both ends.  The functions here
// and the kernels that call them take the model as a type M: int for a built-in id, PesModel (gple_kernels.h) for a table.  Two instantiations,
// because one that carried both cost the step loop's kernels registers and scratch; with_model picks at the launch.
#pragma once
#include <hip/hip_runtime.h>

#include "gple_kernels.h"

namespace gple
{
	template <int NP>
	struct Mat
	{
		double a[NP][NP];
	};
	__device__ __forceinline__ double sgn_n(double v) { return static_cast<double>((v > 0.0) - (v < 0.0)); }

	// The tabulated model at x: s = (x - x_first) / dx, node k = clamp(floor(s), 0, n - 2), t = s - k, and per entry with m = dx V' and
	// D = V_{k+1} - V_k:  c2 = 3 D - (2 m_k + m_{k+1}), c3 = (m_k + m_{k+1}) - 2 D,  V = V_k + t (m_k + t (c2 + t c3)),
	// V' = (m_k + t (2 c2 + 3 t c3)) / dx, F = -V'; for s < 0 and s > n - 1 the tangent at the end node.  At t = 0 the value is the node's
	// bits.  The node index is clamped as a double, so no x (NaN and infinities included) reads outside the table.
	template <int NP>
	__device__ __forceinline__ void table_diabatic_n(double x, const PesModel& pes, Mat<NP>& V, Mat<NP>& F)
	{
		constexpr int S = NP * NP, NODE = PES_TABLE_PLANES * S;
		const double s = (x - pes.x_first) / pes.dx;
		const double last = static_cast<double>(pes.n - 1);
		if (s < 0.0 || s > last)
		{
			const int k = s < 0.0 ? 0 : pes.n - 1;
			const double* node = pes.table + static_cast<long>(NODE) * k;
			const double h = x - (pes.x_first + pes.dx * static_cast<double>(k));
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int j = 0; j <= i; ++j)
				{
					const double v0 = node[NP * i + j], d0 = node[S + NP * i + j];
					V.a[i][j] = V.a[j][i] = v0 + d0 * h;
					F.a[i][j] = F.a[j][i] = -d0;
				}
			return;
		}
		const double kf = fmin(fmax(floor(s), 0.0), last - 1.0);
		const double t = s - kf;
		const double* n0 = pes.table + static_cast<long>(NODE) * static_cast<long>(kf);
		const double* n1 = n0 + NODE;
#pragma unroll
		for (int i = 0; i < NP; ++i)
#pragma unroll
			for (int j = 0; j <= i; ++j)
			{
				const double v0 = n0[NP * i + j], v1 = n1[NP * i + j], m0 = n0[2 * S + NP * i + j], m1 = n1[2 * S + NP * i + j];
				const double delta = v1 - v0;
				const double c2 = 3.0 * delta - (2.0 * m0 + m1), c3 = (m0 + m1) - 2.0 * delta;
				V.a[i][j] = V.a[j][i] = v0 + t * (m0 + t * (c2 + t * c3));
				F.a[i][j] = F.a[j][i] = -((m0 + t * (2.0 * c2 + 3.0 * t * c3)) / pes.dx);
			}
	}

	template <int NP>
	__device__ __forceinline__ void diabatic_n(double x, const PesModel& pes, Mat<NP>& V, Mat<NP>& F)
	{
		table_diabatic_n<NP>(x, pes, V, F);
	}
	// f(model.id) for a built-in model, f(model) for a table: the launchers instantiate their kernel for the type f receives
	template <typename Fn>
	void with_model(const PesModel& model, Fn&& f)
	{
		if (model.table) f(model);
		else f(model.id);
	}

	template <int NP>
	__device__ __forceinline__ void diabatic_n(double x, int model, Mat<NP>& V, Mat<NP>& F)
	{
#pragma unroll
		for (int i = 0; i < NP; ++i)
#pragma unroll
			for (int j = 0; j < NP; ++j) V.a[i][j] = 0.0, F.a[i][j] = 0.0;
		if (model == 0) // SAC, pes.cpp:40-44, 58-62
		{
			constexpr double A = 0.01, B = 1.6, C = 0.005, D = 1.0;
			const double e = exp(-sgn_n(x) * B * x);
			V.a[0][0] = sgn_n(x) * A * (1.0 - e), V.a[1][1] = -V.a[0][0], V.a[0][1] = V.a[1][0] = C * exp(-D * x * x);
			F.a[0][0] = -A * B * e, F.a[1][1] = -F.a[0][0], F.a[0][1] = F.a[1][0] = 2.0 * C * D * x * exp(-D * x * x);
		}
		else if (model == 1) // DAC
		{
			constexpr double A = 0.10, B = 0.28, C = 0.015, D = 0.06, E = 0.05;
			V.a[1][1] = E - A * exp(-B * x * x), V.a[0][1] = V.a[1][0] = C * exp(-D * x * x);
			F.a[1][1] = -2 * A * B * x * exp(-B * x * x), F.a[0][1] = F.a[1][0] = 2 * C * D * x * exp(-D * x * x);
		}
		else if (model == 2) // ECR
		{
			constexpr double A = 6e-4, B = 0.10, C = 0.90;
			const double e = exp(-sgn_n(x) * C * x);
			V.a[0][0] = A, V.a[1][1] = -A, V.a[0][1] = V.a[1][0] = B * (1 - sgn_n(x) * (e - 1));
			F.a[0][1] = F.a[1][0] = -B * C * e;
		}
		else if constexpr (NP == 3) // TSAC (ours)
		{
			constexpr double A = 0.02, B = 0.8, C = 0.005, D = 0.5;
			const double t = tanh(B * x), g = 1.0 / cosh(D * x), th = tanh(D * x);
			V.a[0][0] = A * t, V.a[2][2] = -A * t;
			V.a[0][1] = V.a[1][0] = V.a[1][2] = V.a[2][1] = C * g;
			F.a[0][0] = -A * B * (1.0 - t * t), F.a[2][2] = A * B * (1.0 - t * t);
			F.a[0][1] = F.a[1][0] = F.a[1][2] = F.a[2][1] = C * D * g * th;
		}
	}

	// Cyclic Jacobi for a symmetric NP x NP matrix (destroyed): eigenvalues ascending in lam, eigenvectors in the columns of W.  A pair
	// whose off-diagonal entry is exactly zero is not rotated, so a decoupled level keeps exact zeros in its row and column.
	template <int NP>
	__device__ __forceinline__ void jacobi_eig(Mat<NP>& A, double (&lam)[NP], Mat<NP>& W)
	{
#pragma unroll
		for (int i = 0; i < NP; ++i)
#pragma unroll
			for (int j = 0; j < NP; ++j) W.a[i][j] = i == j ? 1.0 : 0.0;
		for (int sweep = 0; sweep < 8; ++sweep)
		{
#pragma unroll
			for (int p = 0; p < NP - 1; ++p)
#pragma unroll
				for (int q = p + 1; q < NP; ++q)
				{
					const double apq = A.a[p][q];
					if (apq == 0.0) continue;
					const double theta = (A.a[q][q] - A.a[p][p]) / (2.0 * apq);
					const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
					const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
					A.a[p][p] -= t * apq, A.a[q][q] += t * apq, A.a[p][q] = A.a[q][p] = 0.0;
#pragma unroll
					for (int r = 0; r < NP; ++r)
					{
						if (r != p && r != q)
						{
							const double arp = A.a[r][p], arq = A.a[r][q];
							A.a[r][p] = A.a[p][r] = c * arp - s * arq;
							A.a[r][q] = A.a[q][r] = s * arp + c * arq;
						}
						const double wrp = W.a[r][p], wrq = W.a[r][q];
						W.a[r][p] = c * wrp - s * wrq, W.a[r][q] = s * wrp + c * wrq;
					}
				}
		}
#pragma unroll
		for (int i = 0; i < NP; ++i) lam[i] = A.a[i][i];
		// ascending (selection sort on NP <= 3 entries, columns move with their eigenvalue)
#pragma unroll
		for (int i = 0; i < NP - 1; ++i)
#pragma unroll
			for (int j = i + 1; j < NP; ++j)
				if (lam[j] < lam[i])
				{
					const double tl = lam[i];
					lam[i] = lam[j], lam[j] = tl;
#pragma unroll
					for (int r = 0; r < NP; ++r)
					{
						const double tw = W.a[r][i];
						W.a[r][i] = W.a[r][j], W.a[r][j] = tw;
					}
				}
	}

	// the library's sign convention of the adiabatic states (columns of C): last non-zero component positive
	template <int NP>
	__device__ __forceinline__ void adiabatic_sign_n(Mat<NP>& C)
	{
#pragma unroll
		for (int k = 0; k < NP; ++k)
		{
			double last = 0.0;
#pragma unroll
			for (int i = 0; i < NP; ++i)
				if (C.a[i][k] != 0.0) last = C.a[i][k];
			if (last < 0.0)
#pragma unroll
				for (int i = 0; i < NP; ++i) C.a[i][k] = -C.a[i][k];
		}
	}
	// E (ascending) and the adiabatic states C (columns) of the diabatic potential at x, with the sign convention above; Fd receives the
	// diabatic force (the caller may ignore it)
	template <int NP, typename PES>
	__device__ __forceinline__ void adiabatic_states_n(double x, const PES& model, double (&E)[NP], Mat<NP>& C, Mat<NP>& Fd)
	{
		Mat<NP> V;
		diabatic_n<NP>(x, model, V, Fd);
		jacobi_eig<NP>(V, E, C);
		adiabatic_sign_n<NP>(C);
	}
} // namespace gple
