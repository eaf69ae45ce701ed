// gple_dvr.hip — exact DVR wavepacket dynamics of the model the GP method is judged against (schrodinger_equation/ of the reference,
// the reflective and periodic boundaries of general.h:86-97; the absorbing one is gple_dvr_power.hip: DESIGN.md §11).
// The constants, the grid and the fixed reductions that the DVR files share are in gple_dvr_device.h.
//
//   dvr_hamiltonian_kernel  Hamiltonian_construction (general.cpp:106-200) without the absorbing term: dense real symmetric dim x dim,
//                           dim = NP n, index m n + a; the diabatic potential on the diagonal a = a' blocks, the kinetic energy
//                           (Colbert-Miller / periodic) on the diagonal m = m' blocks, each entry in the reference's operation order.
//   dvr_states_kernel       per grid point: the adiabatic states of the diabatic potential (gple_pes_n.h, the functions
//                           gple_pes_adiabatic_n uses); the energies come from gple_pes_adiabatic_n's own kernel (launch_pes_n).
//   dvr_phase_kernel +      Evolution::evolve without ABC (general.cpp:241-252) for T times at once: psi(t) = C (exp(-i E t) o c0) as one
//   launch_gemm             real GEMM with 2T right-hand columns; c0 = C^T psi0 as another.
//   dvr_finish_kernel       psi(t) out, optionally in the adiabatic basis (basis^T psi per grid point, main.cpp:221, pes.cpp:96-120).
//   wigner_kernel           output_phase_space_distribution (general.cpp:324-411) as a GEMM over the displacement k on the fp64 MFMA:
//                           P_ij(x_a, p_b) = dx/(pi hbar) sum_k A_ij(a, k) E(b, k),  A_ij(a, k) = psi_i[a - k] conj(psi_j[a + k]),
//                           E(b, k) = exp(2 i p_b k dx / hbar).  A is generated while its operands are staged (never stored), E is a
//                           table built once per call.  Only j <= i is computed; P_ji = conj(P_ij) is written from the same tile.
//   wigner_avg_*            the averages of general.cpp:393-410 in a fixed reduction order.
#include <cstdio>

#include "gple_dvr_device.h"
#include "gple_kernels.h"
#include "gple_pes_n.h"

namespace gple
{
	namespace
	{
		typedef double d4 __attribute__((ext_vector_type(4)));
		using namespace dvr;

		__device__ __forceinline__ double pow_minus_one(long n) { return n % 2 == 0 ? 1.0 : -1.0; } // general.cpp:38-41

		// one thread per entry (r, c) of the row-major dim x dim matrix (symmetric, so column-major reads the same)
		template <int NP, typename PES>
		__global__ void __launch_bounds__(256) dvr_hamiltonian_kernel(PES model, int boundary, double x_first, double dx, int n, double mass, double* __restrict__ H)
		{
#pragma clang fp contract(off)
			const long dim = static_cast<long>(NP) * n;
			const long c = blockIdx.x * 256L + threadIdx.x, r = blockIdx.y;
			if (c >= dim) return;
			const int m = static_cast<int>(r / n), a = static_cast<int>(r % n), mm = static_cast<int>(c / n), aa = static_cast<int>(c % n);
			double h = 0.0;
			if (a == aa) // 1. V_{mm'}(x_n)   (general.cpp:128-140)
			{
				Mat<NP> V, F;
				diabatic_n<NP>(grid_x(x_first, dx, a), model, V, F);
				h += V.a[m][mm];
			}
			if (m == mm) // 2. kinetic energy
			{
				if (boundary == GPLE_DVR_REFLECTIVE) // general.cpp:154-175
				{
					if (a == aa)
					{
						const double q = PI_D * HBAR_D / dx;
						h += q * q / 6.0 / mass;
					}
					else
					{
						const double q = HBAR_D / dx / static_cast<double>(aa - a);
						h += pow_minus_one(aa - a) * (q * q) / mass;
					}
				}
				else // general.cpp:176-198
				{
					const double L = grid_x(x_first, dx, n - 1) - grid_x(x_first, dx, 0);
					if (a == aa)
					{
						const double q = PI_D * HBAR_D / L;
						h += q * q / 6.0 / mass * static_cast<double>(n * n - 1);
					}
					else
					{
						const double diff = static_cast<double>(a - aa) * PI_D / static_cast<double>(n);
						const double q = PI_D * HBAR_D / L / sin(diff);
						h += pow_minus_one(aa - a) * cos(diff) * (q * q) / mass;
					}
				}
			}
			H[r * dim + c] = h;
		}

		// basis[(a NP + row) NP + col] = C(row, col), columns = adiabatic states
		template <int NP, typename PES>
		__global__ void __launch_bounds__(128) dvr_states_kernel(PES model, double x_first, double dx, int n, double* __restrict__ basis)
		{
			const int a = blockIdx.x * 128 + threadIdx.x;
			if (a >= n) return;
			double E[NP];
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(grid_x(x_first, dx, a), model, E, C, Fd);
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int k = 0; k < NP; ++k) basis[(static_cast<long>(a) * NP + i) * NP + k] = C.a[i][k];
		}
		__global__ void __launch_bounds__(256) dvr_grid_kernel(double x_first, double dx, int n, double* __restrict__ x)
		{
			const int a = blockIdx.x * 256 + threadIdx.x;
			if (a < n) x[a] = grid_x(x_first, dx, a);
		}
		// energies[a NP + k] = E_k(x_a) out of the rows of launch_pes_n (width NP + NP (NP + 1))
		__global__ void __launch_bounds__(256) dvr_take_energies_kernel(const double* __restrict__ pes, int np_, int n, double* __restrict__ energies)
		{
			const int a = blockIdx.x * 256 + threadIdx.x;
			if (a >= n) return;
			for (int k = 0; k < np_; ++k) energies[static_cast<long>(a) * np_ + k] = pes[static_cast<long>(a) * (np_ + np_ * (np_ + 1)) + k];
		}

		// Z(:, 2t) + i Z(:, 2t+1) = exp(-i E t / hbar) o c0   (general.cpp:249), columns of length ld; c0: columns 0 (re) and 1 (im)
		__global__ void __launch_bounds__(256) dvr_phase_kernel(const double* __restrict__ eigval, const double* __restrict__ c0, const double* __restrict__ times,
			int dim, long ld, double* __restrict__ Z)
		{
#pragma clang fp contract(off)
			const int k = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
			if (k >= dim) return;
			const double th = -eigval[k] * times[t] / HBAR_D, cr = cos(th), ci = sin(th), ar = c0[k], ai = c0[ld + k];
			Z[2 * t * ld + k] = cr * ar - ci * ai;
			Z[(2 * t + 1) * ld + k] = cr * ai + ci * ar;
		}

		// (re, im) pairs -> the first two columns of an ld x 64 block (the rest zero)
		__global__ void __launch_bounds__(256) dvr_split_kernel(const double* __restrict__ v, int dim, long ld, double* __restrict__ out)
		{
			const long k = blockIdx.x * 256L + threadIdx.x;
			if (k >= ld) return;
			const d2 z = k < dim ? *reinterpret_cast<const d2*>(v + 2 * k) : (d2){0.0, 0.0};
			out[k] = z.x, out[ld + k] = z.y;
		}

		// psi[t][r] = Y(r, 2t) + i Y(r, 2t+1); with basis: psi_adia[t][k n + a] = sum_j basis(a; j, k) psi_dia[t][j n + a]
		template <int NP>
		__global__ void __launch_bounds__(256) dvr_finish_kernel(const double* __restrict__ Y, long ld, int n, const double* __restrict__ basis, double* __restrict__ psi)
		{
			const int a = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
			if (a >= n) return;
			const double* yr = Y + 2 * t * ld;
			const double* yi = Y + (2 * t + 1) * ld;
			double* out = psi + static_cast<long>(t) * 2 * NP * n;
			if (!basis)
			{
#pragma unroll
				for (int m = 0; m < NP; ++m)
					*reinterpret_cast<d2*>(out + 2 * (static_cast<long>(m) * n + a)) = (d2){yr[static_cast<long>(m) * n + a], yi[static_cast<long>(m) * n + a]};
				return;
			}
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				double re = 0.0, im = 0.0;
#pragma unroll
				for (int j = 0; j < NP; ++j)
				{
					const double b = basis[(static_cast<long>(a) * NP + j) * NP + k];
					re += b * yr[static_cast<long>(j) * n + a], im += b * yi[static_cast<long>(j) * n + a];
				}
				*reinterpret_cast<d2*>(out + 2 * (static_cast<long>(k) * n + a)) = (d2){re, im};
			}
		}

		// ---- Wigner transform -----------------------------------------------------------------------------------------------------------------
		constexpr int WBM = 64, WBN = 64, WBK = 16; // x rows, p columns, k depth of a workgroup tile
		constexpr int WES = WBN + 8;                // LDS row stride of the E tile (doubles)
		constexpr int WPW = WBM + WBK;              // staged psi window (complex values)

		// E table: Ere / Eim[kk * ldE + b] = cos / sin(2 p_b y_k / hbar), y_k = (kk - kh) dx; zero for kk >= 2 kh + 1 or b >= np
		__global__ void __launch_bounds__(256) wigner_table_kernel(const double* __restrict__ p, int np, int kh, int nkp, long ldE, double dx,
			double* __restrict__ Ere, double* __restrict__ Eim)
		{
#pragma clang fp contract(off)
			const long b = blockIdx.x * 256L + threadIdx.x;
			const int kk = blockIdx.y;
			if (b >= ldE) return;
			double re = 0.0, im = 0.0;
			if (b < np && kk <= 2 * kh)
			{
				const double y = static_cast<double>(kk - kh) * dx;
				const double arg = 2.0 * p[b] * y / HBAR_D; // general.cpp:368-369, 376-377
				re = cos(arg), im = sin(arg);
			}
			Ere[kk * ldE + b] = re, Eim[kk * ldE + b] = im;
		}

		struct WignerArgs
		{
			const double* psi; // T x NP x n complex
			const double* Ere;
			const double* Eim;
			double* P; // T x NP^2 x n x np complex
			long ldE;
			int n, np, kh, nkb; // nkb: k blocks of the table
			int boundary;
			double scale; // dx / (pi hbar)
		};

		// Fragment maps of v_mfma_f64_16x16x4_f64 (gple_gemm.hip): first operand X[i = lane & 15][k = lane >> 4], second Y[k = lane >> 4][j = lane & 15],
		// result D[i = (lane >> 4) + 4 reg][j = lane & 15].  X = A (rows x), Y = E (columns p): a lane's results are (re, im) pairs of 16 consecutive p.
		// One workgroup = 4 waves (2 x 2) on a 64 x 64 tile of one (t, i >= j) element; each wave a 32 x 32 sub-tile in 2 x 2 fragments x (re, im).
		template <int NP>
		__global__ void __launch_bounds__(256, 2) wigner_kernel(const WignerArgs g)
		{
			constexpr int NE = NP * (NP + 1) / 2;
			__shared__ __attribute__((aligned(16))) double Es[2][WBK * WES]; // re, im
			__shared__ __attribute__((aligned(16))) double Pw[2][2 * WPW];   // psi_i window, psi_j window: (re, im)
			const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
			const int a0 = blockIdx.x * WBM, b0 = blockIdx.y * WBN;
			const int tt = blockIdx.z / NE, e = blockIdx.z % NE;
			int ie = 0;
			while ((ie + 1) * (ie + 2) / 2 <= e) ++ie;
			const int je = e - ie * (ie + 1) / 2; // element (ie, je), je <= ie, in the packing order (0,0), (1,0), (1,1), (2,0), ...
			const int n = g.n;
			const double* __restrict__ psi_i = g.psi + 2 * (static_cast<long>(tt) * NP + ie) * n;
			const double* __restrict__ psi_j = g.psi + 2 * (static_cast<long>(tt) * NP + je) * n;

			// k blocks this row block needs: all of them (periodic), or those inside |k| <= max_a min(a, n - 1 - a) (reflective: the
			// valid (a, k) region is a diamond; blocks outside it are skipped, entries outside it inside a block are zeros of the window)
			int kb0 = 0, kb1 = g.nkb;
			if (g.boundary == GPLE_DVR_REFLECTIVE)
			{
				const int a1 = min(a0 + WBM, n) - 1;
				const int kmax = (a0 <= (n - 1) / 2 && a1 >= (n - 1) / 2) ? (n - 1) / 2 : (a1 < (n - 1) / 2 ? a1 : n - 1 - a0);
				kb0 = (g.kh - kmax) / WBK, kb1 = (g.kh + kmax) / WBK + 1;
			}

			// staging: E rows kk0 .. kk0 + 15, columns b0 .. b0 + 63 (2 d2 per thread and part); psi windows (one complex per thread, 2 x 80)
			d2 ev[2][2], pv = (d2){0.0, 0.0};
			auto load = [&](int kb) {
				const int kk0 = kb * WBK;
#pragma unroll
				for (int q = 0; q < 2; ++q)
				{
					const int i = t + 256 * q, row = i / (WBN / 2), col = (i % (WBN / 2)) * 2;
					const long off = static_cast<long>(kk0 + row) * g.ldE + b0 + col;
					ev[0][q] = *reinterpret_cast<const d2*>(g.Ere + off);
					ev[1][q] = *reinterpret_cast<const d2*>(g.Eim + off);
				}
				if (t < 2 * WPW)
				{
					const int k0 = kk0 - g.kh, which = t / WPW, o = t % WPW;
					// psi_i[a - k] for a - k in [a0 - k0 - 15, a0 + 63 - k0]; psi_j[a + k] for a + k in [a0 + k0, a0 + 63 + k0 + 15]
					long idx = which == 0 ? static_cast<long>(a0) - k0 - (WBK - 1) + o : static_cast<long>(a0) + k0 + o;
					const double* src = which == 0 ? psi_i : psi_j;
					pv = (d2){0.0, 0.0};
					if (g.boundary == GPLE_DVR_PERIODIC) idx = ((idx % n) + n) % n;
					if (idx >= 0 && idx < n) pv = *reinterpret_cast<const d2*>(src + 2 * idx);
				}
			};
			auto store = [&]() {
#pragma unroll
				for (int q = 0; q < 2; ++q)
				{
					const int i = t + 256 * q, row = i / (WBN / 2), col = (i % (WBN / 2)) * 2;
					*reinterpret_cast<d2*>(&Es[0][row * WES + col]) = ev[0][q];
					*reinterpret_cast<d2*>(&Es[1][row * WES + col]) = ev[1][q];
				}
				if (t < 2 * WPW) *reinterpret_cast<d2*>(&Pw[t / WPW][2 * (t % WPW)]) = pv;
			};

			d4 acc[2][2][2]; // [re / im][fragment row][fragment column]
#pragma unroll
			for (int c = 0; c < 2; ++c)
#pragma unroll
				for (int i = 0; i < 2; ++i)
#pragma unroll
					for (int j = 0; j < 2; ++j) acc[c][i][j] = (d4){0.0, 0.0, 0.0, 0.0};

			const int fk = lane >> 4, fr = lane & 15;
			if (kb0 < kb1)
			{
				load(kb0);
				store();
			}
			__syncthreads();
			for (int kb = kb0; kb < kb1; ++kb)
			{
				if (kb + 1 < kb1) load(kb + 1);
#pragma unroll
				for (int kk = 0; kk < WBK; kk += 4)
				{
					const int kl = kk + fk; // k - k0 of this lane's fragment column
					double ar[2], ai[2], er[2], ei[2];
#pragma unroll
					for (int i = 0; i < 2; ++i)
					{
						const int al = wm * 32 + i * 16 + fr; // a - a0
						const d2 u = *reinterpret_cast<const d2*>(&Pw[0][2 * (al - kl + WBK - 1)]);
						const d2 v = *reinterpret_cast<const d2*>(&Pw[1][2 * (al + kl)]);
						ar[i] = u.x * v.x + u.y * v.y; // psi_i conj(psi_j)
						ai[i] = u.y * v.x - u.x * v.y;
					}
#pragma unroll
					for (int j = 0; j < 2; ++j)
					{
						const int bl = wn * 32 + j * 16 + fr;
						er[j] = Es[0][kl * WES + bl];
						ei[j] = Es[1][kl * WES + bl];
					}
					// Re P += A_re E_re - A_im E_im,  Im P += A_re E_im + A_im E_re; the 8 accumulators are independent within each half
#pragma unroll
					for (int i = 0; i < 2; ++i)
#pragma unroll
						for (int j = 0; j < 2; ++j)
						{
							acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], er[j], acc[0][i][j], 0, 0, 0);
							acc[1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], ei[j], acc[1][i][j], 0, 0, 0);
						}
#pragma unroll
					for (int i = 0; i < 2; ++i)
#pragma unroll
						for (int j = 0; j < 2; ++j)
						{
							acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai[i], ei[j], acc[0][i][j], 0, 0, 0);
							acc[1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], er[j], acc[1][i][j], 0, 0, 0);
						}
				}
				__syncthreads();
				if (kb + 1 < kb1)
				{
					store();
					__syncthreads();
				}
			}

			// P_ij and (i != j) P_ji = conj(P_ij), p fastest, (re, im) interleaved
			const long slab = static_cast<long>(n) * g.np;
			double* __restrict__ Pij = g.P + 2 * (static_cast<long>(tt) * NP * NP + ie * NP + je) * slab;
			double* __restrict__ Pji = g.P + 2 * (static_cast<long>(tt) * NP * NP + je * NP + ie) * slab;
#pragma unroll
			for (int i = 0; i < 2; ++i)
#pragma unroll
				for (int j = 0; j < 2; ++j)
#pragma unroll
					for (int r = 0; r < 4; ++r)
					{
						const int a = a0 + wm * 32 + i * 16 + fk + 4 * r, b = b0 + wn * 32 + j * 16 + fr;
						if (a >= n || b >= g.np) continue;
						const double re = acc[0][i][j][r] * g.scale, im = acc[1][i][j][r] * g.scale;
						const long o = 2 * (static_cast<long>(a) * g.np + b);
						*reinterpret_cast<d2*>(Pij + o) = (d2){re, im};
						if (ie != je) *reinterpret_cast<d2*>(Pji + o) = (d2){re, -im};
					}
		}

		// ---- averages (general.cpp:393-410) ---------------------------------------------------------------------------------------------------
		constexpr int AVG_BLOCKS = 64;
		// partial[((t NP + i) AVG_BLOCKS + blk) 4 + {0..3}] = sums over the rows of block blk of Re P_ii weighted by x, V_i(x), p, p^2 / 2m
		template <int NP>
		__global__ void __launch_bounds__(256) wigner_avg_partial_kernel(const double* __restrict__ P, int n, int np, double x_first, double dx,
			const double* __restrict__ p, const double* __restrict__ energies, double mass, double* __restrict__ partial)
		{
#pragma clang fp contract(off)
			const int blk = blockIdx.x, i = blockIdx.y, tt = blockIdx.z, t = threadIdx.x;
			const long slab = static_cast<long>(n) * np;
			const double* Pii = P + 2 * (static_cast<long>(tt) * NP * NP + i * NP + i) * slab;
			const int rows = (n + AVG_BLOCKS - 1) / AVG_BLOCKS, r0 = blk * rows, r1 = min(n, r0 + rows);
			double s[4] = {0.0, 0.0, 0.0, 0.0};
			for (int a = r0; a < r1; ++a)
			{
				double row = 0.0;
				for (int b = t; b < np; b += 256)
				{
					const double v = Pii[2 * (static_cast<long>(a) * np + b)];
					const double pb = p[b];
					row += v;
					s[2] += v * pb;
					s[3] += v * (pb * pb / 2.0 / mass);
				}
				s[0] += row * grid_x(x_first, dx, a);
				s[1] += row * energies[static_cast<long>(a) * NP + i];
			}
			__shared__ double red[4][256];
#pragma unroll
			for (int q = 0; q < 4; ++q) red[q][t] = s[q];
			__syncthreads();
			for (int h = 128; h > 0; h >>= 1)
			{
				if (t < h)
#pragma unroll
					for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + h];
				__syncthreads();
			}
			if (t < 4) partial[((static_cast<long>(tt) * NP + i) * AVG_BLOCKS + blk) * 4 + t] = red[t][0];
		}
		// averages[3 t + {0, 1, 2}] = (E, x, p) dx dp
		template <int NP>
		__global__ void __launch_bounds__(64) wigner_avg_final_kernel(const double* __restrict__ partial, int T, int np, double dx, const double* __restrict__ p,
			double* __restrict__ averages)
		{
#pragma clang fp contract(off)
			const int tt = blockIdx.x * 64 + threadIdx.x;
			if (tt >= T) return;
			const double dp = (p[np - 1] - p[0]) / static_cast<double>(np - 1); // general.cpp:337
			double sx = 0.0, sv = 0.0, sp = 0.0, sk = 0.0;
			for (int i = 0; i < NP; ++i)
				for (int blk = 0; blk < AVG_BLOCKS; ++blk)
				{
					const double* q = partial + ((static_cast<long>(tt) * NP + i) * AVG_BLOCKS + blk) * 4;
					sx += q[0], sv += q[1], sp += q[2], sk += q[3];
				}
			averages[3 * tt] = (sv + sk) * dx * dp;
			averages[3 * tt + 1] = sx * dx * dp;
			averages[3 * tt + 2] = sp * dx * dp;
		}
	} // namespace

	hipError_t launch_dvr_hamiltonian(hipStream_t s, int num_pes, PesModel model, int boundary, double x_first, double dx, int n, double mass, double* H)
	{
		const long dim = static_cast<long>(num_pes) * n;
		const dim3 grid(static_cast<unsigned>((dim + 255) / 256), static_cast<unsigned>(dim));
		if (num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((dvr_hamiltonian_kernel<2, decltype(m)>), grid, dim3(256), 0, s, m, boundary, x_first, dx, n, mass, H); });
		else if (num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((dvr_hamiltonian_kernel<3, decltype(m)>), grid, dim3(256), 0, s, m, boundary, x_first, dx, n, mass, H); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	size_t dvr_states_work_doubles(int num_pes, int n) { return static_cast<size_t>(n) * (1 + num_pes + num_pes * (num_pes + 1)); }
	// energies: the adiabatic energies of gple_pes_adiabatic_n's own kernel at the grid points (the same bits); basis from the same device functions
	hipError_t launch_dvr_states(hipStream_t s, int num_pes, PesModel model, double x_first, double dx, int n, double* energies, double* basis, double* work)
	{
		if (num_pes != 2 && num_pes != 3) return hipErrorInvalidValue;
		if (energies)
		{
			double* x = work;
			double* pes = work + n;
			hipLaunchKernelGGL(dvr_grid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x_first, dx, n, x);
			hipError_t err = launch_pes_n(s, num_pes, x, n, model, pes);
			if (err != hipSuccess) return err;
			hipLaunchKernelGGL(dvr_take_energies_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pes, num_pes, n, energies);
		}
		if (basis)
		{
			const dim3 grid((n + 127) / 128);
			if (num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((dvr_states_kernel<2, decltype(m)>), grid, dim3(128), 0, s, m, x_first, dx, n, basis); });
			else with_model(model, [&](auto m) { hipLaunchKernelGGL((dvr_states_kernel<3, decltype(m)>), grid, dim3(128), 0, s, m, x_first, dx, n, basis); });
		}
		return hipGetLastError();
	}

	size_t dvr_propagate_work_doubles(int num_pes, int n, int T)
	{
		const long dim = static_cast<long>(num_pes) * n, ld = static_cast<long>(round_up(dim, 64)), nc = static_cast<long>(round_up(2 * T, 64));
		return static_cast<size_t>(ld * ld + 2 * ld * nc + ld * 64 + ld * 64);
	}
	// work: dvr_propagate_work_doubles; Cp (ld x ld, row-major eigenvectors, zero padded) must already hold C; v: psi0 or c0, dim (re, im) pairs
	hipError_t launch_dvr_propagate(hipStream_t s, int num_pes, int n, const double* eigval, const double* v, const double* times, int T, const double* basis,
		bool from_psi0, double* work, double* psi)
	{
		const long dim = static_cast<long>(num_pes) * n, ld = static_cast<long>(round_up(dim, 64)), nc = static_cast<long>(round_up(2 * T, 64));
		double* Cp = work;
		double* Z = Cp + ld * ld;
		double* Y = Z + ld * nc;
		double* in = Y + ld * nc;
		double* c0 = in + ld * 64;
		hipError_t err;
		if ((err = hipMemsetAsync(in, 0, sizeof(double) * ld * 64, s)) != hipSuccess) return err;
		hipLaunchKernelGGL(dvr_split_kernel, dim3(static_cast<unsigned>((ld + 255) / 256)), dim3(256), 0, s, v, static_cast<int>(dim), ld, in);
		if ((err = hipGetLastError()) != hipSuccess) return err;
		if (from_psi0) // c0(k) = sum_r C(r, k) psi0(r)   (general.cpp:225)
		{
			GemmDesc d{};
			d.A = Cp, d.lda = ld, d.a_kmajor = false; // A(m = k, r) at k + r ld
			d.B = in, d.ldb = ld, d.b_kmajor = true;  // B(n, r) at r + n ld
			d.C = c0, d.ldc = ld, d.c_trans = false;
			d.M = static_cast<int>(ld), d.N = 64, d.K = static_cast<int>(ld), d.batch = 1, d.alpha = 1.0, d.beta = 0.0, d.krange = K_FULL;
			if ((err = launch_gemm(s, d, 64)) != hipSuccess) return err;
		}
		else c0 = in;
		if ((err = hipMemsetAsync(Z, 0, sizeof(double) * ld * nc, s)) != hipSuccess) return err;
		hipLaunchKernelGGL(dvr_phase_kernel, dim3(static_cast<unsigned>((dim + 255) / 256), T), dim3(256), 0, s, eigval, c0, times, static_cast<int>(dim), ld, Z);
		if ((err = hipGetLastError()) != hipSuccess) return err;
		GemmDesc d{};
		d.A = Cp, d.lda = ld, d.a_kmajor = true; // A(m = r, k) at k + r ld
		d.B = Z, d.ldb = ld, d.b_kmajor = true;  // B(n = column, k) at k + n ld
		d.C = Y, d.ldc = ld, d.c_trans = false;
		d.M = static_cast<int>(ld), d.N = static_cast<int>(nc), d.K = static_cast<int>(ld), d.batch = 1, d.alpha = 1.0, d.beta = 0.0, d.krange = K_FULL;
		if ((err = launch_gemm(s, d, gemm_pick_tile(ld, nc, 1, false) == 128 ? 128 : 64)) != hipSuccess) return err;
		const dim3 grid((n + 255) / 256, T);
		if (num_pes == 2) hipLaunchKernelGGL(dvr_finish_kernel<2>, grid, dim3(256), 0, s, Y, ld, n, basis, psi);
		else hipLaunchKernelGGL(dvr_finish_kernel<3>, grid, dim3(256), 0, s, Y, ld, n, basis, psi);
		return hipGetLastError();
	}

	// the displacement range of the Wigner sum: |k| <= kh
	int wigner_half_range(int boundary, int n) { return boundary == GPLE_DVR_REFLECTIVE ? (n - 1) / 2 : n / 3; }
	size_t wigner_table_doubles(int boundary, int n, int np)
	{
		const long kh = wigner_half_range(boundary, n), nkp = static_cast<long>(round_up(2 * kh + 1, WBK)), ldE = static_cast<long>(round_up(np, WBN));
		return static_cast<size_t>(2 * nkp * ldE);
	}
	hipError_t launch_wigner_table(hipStream_t s, int boundary, int n, const double* p, int np, double dx, double* table)
	{
		const int kh = wigner_half_range(boundary, n), nkp = static_cast<int>(round_up(2 * kh + 1, WBK));
		const long ldE = static_cast<long>(round_up(np, WBN));
		hipLaunchKernelGGL(wigner_table_kernel, dim3(static_cast<unsigned>((ldE + 255) / 256), nkp), dim3(256), 0, s, p, np, kh, nkp, ldE, dx, table, table + nkp * ldE);
		return hipGetLastError();
	}
	hipError_t launch_wigner(hipStream_t s, int num_pes, int boundary, int n, double dx, const double* table, int np, const double* psi, int T, double* P)
	{
		WignerArgs g;
		g.kh = wigner_half_range(boundary, n);
		const int nkp = static_cast<int>(round_up(2 * g.kh + 1, WBK));
		g.ldE = static_cast<long>(round_up(np, WBN));
		g.Ere = table, g.Eim = table + nkp * g.ldE;
		g.psi = psi, g.P = P, g.n = n, g.np = np, g.nkb = nkp / WBK, g.boundary = boundary;
		g.scale = dx / (PI_D * HBAR_D); // general.cpp:383
		const int ne = num_pes * (num_pes + 1) / 2;
		const dim3 grid((n + WBM - 1) / WBM, static_cast<unsigned>(g.ldE / WBN), T * ne);
		if (num_pes == 2) hipLaunchKernelGGL(wigner_kernel<2>, grid, dim3(256), 0, s, g);
		else if (num_pes == 3) hipLaunchKernelGGL(wigner_kernel<3>, grid, dim3(256), 0, s, g);
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	size_t wigner_avg_work_doubles(int num_pes, int T) { return static_cast<size_t>(T) * num_pes * AVG_BLOCKS * 4; }
	hipError_t launch_wigner_averages(hipStream_t s, int num_pes, int n, double x_first, double dx, const double* p, int np, const double* energies,
		double mass, const double* P, int T, double* work, double* averages)
	{
		const dim3 grid(AVG_BLOCKS, num_pes, T);
		if (num_pes == 2)
		{
			hipLaunchKernelGGL(wigner_avg_partial_kernel<2>, grid, dim3(256), 0, s, P, n, np, x_first, dx, p, energies, mass, work);
			hipLaunchKernelGGL(wigner_avg_final_kernel<2>, dim3((T + 63) / 64), dim3(64), 0, s, work, T, np, dx, p, averages);
		}
		else if (num_pes == 3)
		{
			hipLaunchKernelGGL(wigner_avg_partial_kernel<3>, grid, dim3(256), 0, s, P, n, np, x_first, dx, p, energies, mass, work);
			hipLaunchKernelGGL(wigner_avg_final_kernel<3>, dim3((T + 63) / 64), dim3(64), 0, s, work, T, np, dx, p, averages);
		}
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
} // namespace gple
