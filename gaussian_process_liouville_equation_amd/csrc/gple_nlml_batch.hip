// gple_nlml_batch.hip — B independent NLML problems (test/gpr.cpp:499-532 with the derivative matrices of :408-468) in ONE launch, one
// workgroup of four waves per problem; 1 <= N <= 256.  The hyper-parameter search of the reconstruction evaluates problems of
// N = 200 by the thousand: as a chain of whole-GPU launches each of them occupies a handful of compute units and costs launch and
// synchronisation latency; here a problem is one compute unit's work and a batch fills the chip.  No workgroup waits for another (no flags,
// no spinning, no cooperative launch), every sum runs in an order fixed by the problem alone and there are no floating-point atomics: a
// problem returns the same bits alone, at any position of any batch, beside problems of any size.
//
// Per problem, n = N rounded up to 64 with the identity on the padding, matrices column-major in this problem's slice of the
// work pool (L2-resident: 2 x 512 KB at n = 256), ld = n:
//   Gram      lower block triangle of K = w_d^2 I + w_g^2 exp(-Q / 2) with the arithmetic of nlml_gram_kernel (gple_nlml_ard.h)
//   Cholesky  right-looking, 64-wide panels: wave 0 factors the diagonal block in LDS with a matrix row per lane (no barrier on the
//             chain) and inverts it in place by substitution with a column per lane; the panel is L21 = A21 T_jj^T and the
//             trailing update A22 -= L21 L21^T on v_mfma_f64_16x16x4_f64, operands straight from L2; the labels ride along as one more
//             row (u = L^-1 y, kept in LDS)
//   value     u.u / 2 + sum log L_ii
//   gradient  T = L^-1 by block rows (kept transposed: every later operand read is contiguous), b = T^T u, and per 16 x 16 tile of the
//             lower triangle W = T^T T in MFMA accumulators, contracted on the spot with the dK of nlml_grad_kernel: W is never stored
// A non-positive pivot turns the problem's value, gradient and weights into NaN and sets its info word; nothing else is touched.
#include "gple_kernels.h"
#include "gple_nlml_ard.h"

namespace gple
{
	namespace
	{
		typedef double d4 __attribute__((ext_vector_type(4)));
		constexpr int NB = CHOL_NB;  // 64
		constexpr int SLD = NB + 1;  // LDS row stride of the 64 x 64 block: lanes along a column hit distinct banks
		constexpr int MAXN = NLML_BATCH_MAX_N;

		__device__ __forceinline__ double wave_sum(double x)
		{
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
			return x;
		}
		// the value of lane `src` (a constant or wave-uniform index) as a scalar
		__device__ __forceinline__ double read_lane(double v, int src)
		{
			const long long bits = __double_as_longlong(v);
			const unsigned lo = __builtin_amdgcn_readlane(static_cast<int>(bits), src), hi = __builtin_amdgcn_readlane(static_cast<int>(bits >> 32), src);
			return __longlong_as_double(static_cast<long long>(static_cast<unsigned long long>(hi) << 32 | lo));
		}
		// acc[t] (16 x 16, MFMA result layout: row (lane >> 4) + 4 reg, column lane & 15) += P_t(16 x K) Q(K x 16), K a multiple of 16:
		// P_t(i, k) = p[(16 t + i) psi + k psk], Q(k, j) = q[k qsk + j qsj]  (fragment maps: gple_gemm.hip)
		template <int NT>
		__device__ __forceinline__ void tile_gemm(d4 (&acc)[NT], const double* p, long psi, long psk, const double* q, long qsk, long qsj, int K, int lane)
		{
			const double* pp = p + (lane & 15) * psi + (lane >> 4) * psk;
			const double* qq = q + (lane >> 4) * qsk + (lane & 15) * qsj;
			for (int k0 = 0; k0 < K; k0 += 16)
			{
				double x[NT][4], y[4];
#pragma unroll
				for (int s = 0; s < 4; ++s)
				{
					y[s] = qq[(k0 + 4 * s) * qsk];
#pragma unroll
					for (int t = 0; t < NT; ++t) x[t][s] = pp[16 * t * psi + (k0 + 4 * s) * psk];
				}
#pragma unroll
				for (int s = 0; s < 4; ++s)
#pragma unroll
					for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[t][s], y[s], acc[t], 0, 0, 0);
			}
		}

		// the 64 x 64 diagonal block at A (column-major, ld), by ONE wave, in LDS (S, row-major) with a matrix row per lane and no barrier: the wave
		// runs in lockstep and the LDS serves its requests in order.  L = chol(block) 16 columns at a time (the sub-panel's row in registers, the
		// multipliers L_ck as LDS broadcasts through col, 64 doubles), then T = L^-1 by substitution with a column per lane, row i of T taking the
		// place of row i of L, which nothing needs after it.  Leaves T in S (zeros above the diagonal) and, transposed, in Tt; the diagonal of L in
		// ldiag.  -> 0 or the 1-based local column of the first pivot that is not positive (everything after it is NaN)
		__device__ __forceinline__ int factor_diagonal(const double* A, long ld, double* S, double* col, double* Tt, double* ldiag, int lane)
		{
			for (int k = 0; k < NB; ++k) S[lane * SLD + k] = A[lane + k * ld];
			int bad = 0;
			for (int base = 0; base < NB; base += 16)
			{
				double p[16];
#pragma unroll
				for (int k = 0; k < 16; ++k) p[k] = S[lane * SLD + base + k];
#pragma unroll
				for (int k = 0; k < 16; ++k)
				{
					const double d = read_lane(p[k], base + k);
					const bool ok = d > 0.0;
					bad = (!ok && bad == 0) ? base + k + 1 : bad;
					const double l = ok ? sqrt(d) : __builtin_nan("");
					const double r = 1.0 / l;
					p[k] = lane == base + k ? l : p[k] * r;
					col[lane] = p[k];
#pragma unroll
					for (int c = k + 1; c < 16; ++c) p[c] = fma(-p[k], col[base + c], p[c]);
				}
#pragma unroll
				for (int k = 0; k < 16; ++k) S[lane * SLD + base + k] = p[k]; // (rows above the sub-panel write entries above the diagonal: never read)
				for (int c = base + 16; c < NB; ++c) // the columns right of the sub-panel
				{
					double s = S[lane * SLD + c];
#pragma unroll
					for (int k = 0; k < 16; ++k) s = fma(-p[k], S[c * SLD + base + k], s);
					S[lane * SLD + c] = s;
				}
			}
			ldiag[lane] = S[lane * SLD + lane];
			for (int i = 0; i < NB; ++i) // t_i = (delta_i,lane - sum_{k < i} L_ik t_k) / L_ii, t_k = S[k][lane] by now
			{
				double s = i == lane ? 1.0 : 0.0;
				for (int k = 0; k < i; ++k) s = fma(-S[i * SLD + k], S[k * SLD + lane], s);
				const double t = s / S[i * SLD + i];
				S[i * SLD + lane] = t, Tt[lane + i * ld] = t;
			}
			return bad;
		}

		__global__ void __launch_bounds__(256, 2) nlml_batch_kernel(const NlmlBatchProblem* __restrict__ problems, double* work, double* values,
			double* grads, int grad_width, int* info)
		{
			__shared__ double S[NB * SLD];                              // the diagonal block: L_jj, then T_jj; later the product M of a T block
			__shared__ double Xs[2 * MAXN], yv[MAXN], uv[MAXN], ldiag[MAXN], bv[MAXN]; // points, labels (updated in place), u = L^-1 y, diag L, b
			__shared__ double red[4][6], col[NB];
			__shared__ int first_bad;
			const NlmlBatchProblem pr = problems[blockIdx.x];
			const int N = pr.N, n = (N + NB - 1) / NB * NB, nb = n / NB, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
			const int fr = lane & 15, fk = lane >> 4;
			const long ld = n;
			double* const A = work + pr.work;
			double* const Tt = A + ld * n; // Tt[c + r ld] = T(r, c)
			const double wd = pr.x[0], wg = pr.x[1];
			const ArdW w{pr.x[2], pr.x[3], pr.x[4]};
			const bool want_grad = pr.flags & NLML_BATCH_GRAD, need_T = want_grad || pr.weights;

			if (tid == 0) first_bad = 0;
			if (tid < n)
			{
				const bool in = tid < N;
				Xs[2 * tid] = in ? pr.X[2 * tid] : 0.0, Xs[2 * tid + 1] = in ? pr.X[2 * tid + 1] : 0.0;
				yv[tid] = in ? pr.y[tid] : 0.0;
			}
			__syncthreads();
			// ---- Gram: row tid, every column up to the end of the row's diagonal block ------------------------------------------------------
			if (tid < n)
			{
				const int i = tid, jend = (i | (NB - 1)) + 1;
				const double x0 = Xs[2 * i], x1 = Xs[2 * i + 1];
				for (int j = 0; j < jend; ++j)
				{
					double val = i == j ? 1.0 : 0.0;
					if (i < N && j < N)
					{
						val = __dmul_rn(__dmul_rn(wg, wg), ard(x0, x1, Xs[2 * j], Xs[2 * j + 1], w));
						if (i == j) val = __dadd_rn(val, __dmul_rn(wd, wd));
					}
					A[i + j * ld] = val;
				}
			}
			__syncthreads();
			// ---- Cholesky -------------------------------------------------------------------------------------------------------------------
			for (int jb = 0; jb < nb; ++jb)
			{
				const int j0 = NB * jb, below = n - j0 - NB; // rows under the diagonal block
				double* const Ajj = A + j0 + j0 * ld;
				if (wave == 0)
				{
					const int bad = factor_diagonal(Ajj, ld, S, col, Tt + j0 + j0 * ld, ldiag + j0, lane);
					if (lane == 0 && bad && first_bad == 0) first_bad = j0 + bad;
				}
				__syncthreads();
				if (tid < NB) // the label row: u_j = y_j T_jj^T
				{
					double s = 0.0;
					for (int k = 0; k <= tid; ++k) s = fma(yv[j0 + k], S[tid * SLD + k], s);
					uv[j0 + tid] = s;
				}
				for (int strip = wave; strip < below / 16; strip += 4) // L21 = A21 T_jj^T, 16 rows at a time, in place
				{
					double* const rows = Ajj + NB + 16 * strip;
					d4 acc[4] = {};
					tile_gemm<4>(acc, S, SLD, 1, rows, ld, 1, NB, lane); // D(c, r) = sum_k T(c, k) A21(r, k)
#pragma unroll
					for (int t = 0; t < 4; ++t)
#pragma unroll
						for (int r = 0; r < 4; ++r) rows[fr + (16 * t + fk + 4 * r) * ld] = acc[t][r];
				}
				__syncthreads();
				// trailing update of the lower block triangle: 16 rows x 64 columns per item, items dealt to the waves in turn
				double* const A22 = Ajj + NB + NB * ld;
				int item = 0;
				for (int strip = 0; strip < below / 16; ++strip)
					for (int cb = 0; cb <= strip / 4; ++cb, ++item)
					{
						if ((item & 3) != wave) continue;
						d4 acc[4] = {};
						tile_gemm<4>(acc, Ajj + NB + NB * cb, 1, ld, Ajj + NB + 16 * strip, ld, 1, NB, lane); // D(c, r) = sum_k L21(c, k) L21(r, k)
						double* const out = A22 + 16 * strip + NB * cb * ld;
#pragma unroll
						for (int t = 0; t < 4; ++t)
#pragma unroll
							for (int r = 0; r < 4; ++r) out[fr + (16 * t + fk + 4 * r) * ld] -= acc[t][r];
					}
				if (tid < below) // and of the label row
				{
					double s = yv[j0 + NB + tid];
					for (int c = 0; c < NB; ++c) s = fma(-Ajj[NB + tid + c * ld], uv[j0 + c], s);
					yv[j0 + NB + tid] = s;
				}
				__syncthreads();
			}
			// ---- value ----------------------------------------------------------------------------------------------------------------------
			{
				const double term = tid < n ? fma(0.5 * uv[tid], uv[tid], log(ldiag[tid])) : 0.0;
				const double ws = wave_sum(term);
				if (lane == 0) red[wave][5] = ws;
			}
			__syncthreads();
			const bool failed = first_bad != 0;
			if (tid == 0)
			{
				values[blockIdx.x] = failed ? __builtin_nan("") : ((red[0][5] + red[1][5]) + (red[2][5] + red[3][5]));
				if (info) info[blockIdx.x] = first_bad;
			}
			if (!need_T) return; // (uniform)
			// ---- T = L^-1 by block rows: T(i, c) = -T_ii sum_{c <= k < i} L(i, k) T(k, c), through LDS ---------------------------------------
			for (int ib = 1; ib < nb; ++ib)
				for (int cb = 0; cb < ib; ++cb)
				{
					d4 acc[4] = {};
					// M(r, c') = sum_k L(64 ib + r, 64 cb + k) T(64 cb + k, 64 cb + c'): this wave's 16 columns
					tile_gemm<4>(acc, A + NB * ib + NB * cb * ld, 1, ld, Tt + NB * cb + 16 * wave + NB * cb * ld, ld, 1, NB * (ib - cb), lane);
#pragma unroll
					for (int t = 0; t < 4; ++t)
#pragma unroll
						for (int r = 0; r < 4; ++r) S[(16 * t + fk + 4 * r) * SLD + 16 * wave + fr] = acc[t][r];
					__syncthreads();
					d4 out[4] = {};
					tile_gemm<4>(out, Tt + NB * ib + NB * ib * ld, ld, 1, S + 16 * wave, SLD, 1, NB, lane); // D(r, c') = sum_k T_ii(r, k) M(k, c')
#pragma unroll
					for (int t = 0; t < 4; ++t)
#pragma unroll
						for (int r = 0; r < 4; ++r) Tt[NB * cb + 16 * wave + fr + (NB * ib + 16 * t + fk + 4 * r) * ld] = -out[t][r];
					__syncthreads();
				}
			// ---- b = T^T u ------------------------------------------------------------------------------------------------------------------
			if (tid < n)
			{
				double s = 0.0;
				for (int k = tid; k < n; ++k) s = fma(Tt[tid + k * ld], uv[k], s);
				s = failed ? __builtin_nan("") : s;
				bv[tid] = s;
				if (pr.weights && tid < N) pr.weights[tid] = s;
			}
			__syncthreads();
			if (!want_grad) return; // (uniform)
			// ---- gradient: sum_ij (W_ij - b_i b_j) dK_ij / 2 over 16 x 16 tiles of the lower triangle, off-diagonal tiles counted twice ----------
			double g[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
			{
				const int tiles = (N + 15) / 16;
				int item = 0;
				for (int ti = 0; ti < tiles; ++ti)
					for (int gb = 0; gb <= ti / 4; ++gb, ++item)
					{
						if ((item & 3) != wave) continue;
						d4 acc[4] = {};
						const int k0 = 16 * ti; // T(k, I) = 0 for k < I
						tile_gemm<4>(acc, Tt + NB * gb + k0 * ld, 1, ld, Tt + 16 * ti + k0 * ld, ld, 1, n - k0, lane); // D(J, I) = sum_k T(k, J) T(k, I)
						const int I = 16 * ti + fr;
						const double x0 = Xs[2 * I], x1 = Xs[2 * I + 1], bi = bv[I];
#pragma unroll
						for (int t = 0; t < 4; ++t)
						{
							const int tj = 4 * gb + t;
							const double twice = tj < ti ? 2.0 : 1.0;
#pragma unroll
							for (int r = 0; r < 4; ++r)
							{
								const int J = 16 * tj + fk + 4 * r;
								const bool live = tj <= ti && I < N && J < N;
								const double y0 = Xs[2 * J], y1 = Xs[2 * J + 1];
								double u0, u1;
								const double gk = ard(x0, x1, y0, y1, w, &u0, &u1);
								const double m = live ? twice * (acc[t][r] - bi * bv[J]) : 0.0;
								const double e0 = x0 - y0, e1 = x1 - y1;
								g[0] += m * (I == J ? wd : 0.0);
								g[1] += m * (wg * gk);
								g[2] += m * (wg * wg * (-gk * u0 * e0));
								g[3] += m * (wg * wg * (-gk * u0 * e1));
								g[4] += m * (wg * wg * (-gk * u1 * e1));
							}
						}
					}
			}
#pragma unroll
			for (int ip = 0; ip < 5; ++ip)
			{
				const double ws = wave_sum(g[ip]);
				if (lane == 0) red[wave][ip] = ws;
			}
			__syncthreads();
			if (tid == 0)
			{
				double g5[5];
				for (int ip = 0; ip < 5; ++ip) g5[ip] = failed ? __builtin_nan("") : ((red[0][ip] + red[1][ip]) + (red[2][ip] + red[3][ip])) / 2.0;
				double* const out = grads + static_cast<long>(grad_width) * blockIdx.x;
				out[0] = g5[0], out[1] = g5[1], out[2] = g5[2];
				if (grad_width == 5) out[3] = g5[3], out[4] = g5[4];
				else out[3] = g5[4];
			}
		}
	} // namespace

	hipError_t launch_nlml_batch(hipStream_t s, const NlmlBatchProblem* problems, int B, double* work, double* values, double* grads, int grad_width,
		int* info)
	{
		hipLaunchKernelGGL(nlml_batch_kernel, dim3(B), dim3(256), 0, s, problems, work, values, grads, grad_width, info);
		return hipGetLastError();
	}
} // namespace gple
