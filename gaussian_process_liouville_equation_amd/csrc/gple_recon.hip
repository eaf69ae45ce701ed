// gple_recon.hip — reconstruction of a gridded phase-space density with the NLML GP (test/main_evolve.cpp:56-179, test/gpr.cpp):
//   recon_survey_*     max / min / sum |v| / first maximum per plane and the from-grid observables (gpr.cpp:42-82, 119-135, 197-210, 247)
//   recon_scan_* ...   generate_training_set (gpr.cpp:215-291): a blocked running sum of |v|, a binary search per draw, first-occurrence marking
//   recon_tables_kernel / recon_contract_kernel / recon_final_kernel
//                      predict_phase (gpr.cpp:654-706) on the tensor grid as the product of two tables on the fp64 MFMA, with
//                      mean_squared_error (gpr.cpp:994-1005) and the from-grid observables of the prediction as its epilogue
//   recon_cross_kernel the same for the cross-term kernel W = [[a, 0], [c, b]] (gpr.cpp:99-103, 313-321): the bilinear term factorises per tile
//                      around the tile's centre, so the two operand slabs are generated inside the contraction
// The state is num_pes^2 real planes (SuperMatrix, test/io.cpp:25-72): plane (r, c) is Re rho_rc for r <= c and Im rho_cr for r > c, all taken
// from the elements i <= j of the (re, im) interleaved state.
#include <climits>

#include "gple_kernels.h"
#include "gple_pes_n.h"
#include "gple_philox.h"

namespace gple
{
	namespace
	{
		typedef double d4 __attribute__((ext_vector_type(4)));
		typedef double d2 __attribute__((ext_vector_type(2)));

		// upper element e (row-major over i <= j) -> (i, j)
		__device__ __forceinline__ void upper_element(int np_, int e, int& i, int& j)
		{
			i = 0;
			while (e >= np_ - i) e -= np_ - i, ++i;
			j = i + e;
		}
		// plane q = r num_pes + c -> its element's first double and the component (0: re, 1: im)
		__device__ __forceinline__ const double* plane_source(const double* rho, int np_, long cells, int q, int& comp)
		{
			const int r = q / np_, c = q % np_;
			comp = r > c;
			const int i = r > c ? c : r, j = r > c ? r : c;
			return rho + 2 * (static_cast<long>(i) * np_ + j) * cells;
		}

		// ---- survey ---------------------------------------------------------------------------------------------------------------------------
		constexpr double NO_INDEX = 1e300;
		__device__ __forceinline__ double tree_sum(double v, double* red)
		{
			const int t = threadIdx.x;
			__syncthreads();
			red[t] = v;
			__syncthreads();
			for (int h = 128; h > 0; h >>= 1)
			{
				if (t < h) red[t] += red[t + h];
				__syncthreads();
			}
			return red[0];
		}
		// the larger value wins, the smaller index among equal values (sign = -1: the smaller value)
		__device__ __forceinline__ void tree_extreme(double& v, double& idx, double sign, double* red, double* redi)
		{
			const int t = threadIdx.x;
			__syncthreads();
			red[t] = v, redi[t] = idx;
			__syncthreads();
			for (int h = 128; h > 0; h >>= 1)
			{
				if (t < h)
				{
					const double a = red[t], b = red[t + h];
					if (sign * b > sign * a || (b == a && redi[t + h] < redi[t])) red[t] = b, redi[t] = redi[t + h];
				}
				__syncthreads();
			}
			v = red[0], idx = redi[0];
		}

		// work[(q SB + blk) 7 + ...] = max, min, sum |v|, first index of max, sum v, sum v E_i(x_a), sum v p_b^2 / 2m  over the rows of block blk
		template <int NP, typename PES>
		__global__ void __launch_bounds__(256) recon_survey_kernel(PES model, const double* __restrict__ rho, const double* __restrict__ x, int nx,
			const double* __restrict__ p, int np, double mass, double* __restrict__ work)
		{
#pragma clang fp contract(off)
			__shared__ double red[256], redi[256];
			__shared__ double e_row;
			const int blk = blockIdx.x, t = threadIdx.x;
			int ie, je;
			upper_element(NP, blockIdx.y, ie, je);
			const long cells = static_cast<long>(nx) * np;
			const double* __restrict__ el = rho + 2 * (static_cast<long>(ie) * NP + je) * cells;
			const int rows = (nx + RECON_SURVEY_BLOCKS - 1) / RECON_SURVEY_BLOCKS, r0 = blk * rows, r1 = min(nx, r0 + rows);
			const int ncomp = ie == je ? 1 : 2;
			const double inf = __builtin_huge_val();
			double mx[2] = {-inf, -inf}, mn[2] = {inf, inf}, ix[2] = {NO_INDEX, NO_INDEX}, in[2] = {NO_INDEX, NO_INDEX}, sa[2] = {0.0, 0.0};
			double pop = 0.0, pot = 0.0, kin = 0.0;
			for (int a = r0; a < r1; ++a)
			{
				if (ie == je)
				{
					__syncthreads();
					if (t == 0)
					{
						double E[NP];
						Mat<NP> C, Fd;
						adiabatic_states_n<NP>(x[a], model, E, C, Fd);
						e_row = E[ie];
					}
					__syncthreads();
				}
				for (int b = t; b < np; b += 256)
				{
					const long cell = static_cast<long>(a) * np + b;
					const d2 z = *reinterpret_cast<const d2*>(el + 2 * cell);
					const double v[2] = {z.x, z.y};
#pragma unroll
					for (int c = 0; c < 2; ++c)
					{
						if (c >= ncomp) break;
						if (v[c] > mx[c]) mx[c] = v[c], ix[c] = static_cast<double>(cell);
						if (v[c] < mn[c]) mn[c] = v[c], in[c] = static_cast<double>(cell);
						sa[c] += fabs(v[c]);
					}
					if (ie == je)
					{
						const double pb = p[b];
						pop += v[0], pot += v[0] * e_row, kin += v[0] * (pb * pb / 2.0 / mass);
					}
				}
			}
			for (int c = 0; c < ncomp; ++c)
			{
				tree_extreme(mx[c], ix[c], 1.0, red, redi);
				tree_extreme(mn[c], in[c], -1.0, red, redi);
				const double s = tree_sum(sa[c], red);
				const int q = c == 0 ? ie * NP + je : je * NP + ie;
				double* w = work + (static_cast<long>(q) * RECON_SURVEY_BLOCKS + blk) * RECON_SURVEY_VALUES;
				if (t == 0) w[0] = mx[c], w[1] = mn[c], w[2] = s, w[3] = ix[c], w[4] = 0.0, w[5] = 0.0, w[6] = 0.0;
			}
			if (ie == je)
			{
				const double s0 = tree_sum(pop, red), s1 = tree_sum(pot, red), s2 = tree_sum(kin, red);
				double* w = work + (static_cast<long>(ie * NP + ie) * RECON_SURVEY_BLOCKS + blk) * RECON_SURVEY_VALUES;
				if (t == 0) w[4] = s0, w[5] = s1, w[6] = s2;
			}
		}
		// out[8 q + ...]: the blocks in ascending order
		__global__ void __launch_bounds__(64) recon_survey_final_kernel(int nplanes, const double* __restrict__ work, double dxdp, double* __restrict__ out)
		{
#pragma clang fp contract(off)
			const int q = threadIdx.x;
			if (q >= nplanes) return;
			double mx = -__builtin_huge_val(), mn = __builtin_huge_val(), ix = NO_INDEX, sa = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
			for (int blk = 0; blk < RECON_SURVEY_BLOCKS; ++blk)
			{
				const double* w = work + (static_cast<long>(q) * RECON_SURVEY_BLOCKS + blk) * RECON_SURVEY_VALUES;
				if (w[0] > mx) mx = w[0], ix = w[3]; // blocks hold ascending rows: the first block with the maximum has its first cell
				if (w[1] < mn) mn = w[1];
				sa += w[2], s0 += w[4], s1 += w[5], s2 += w[6];
			}
			double* o = out + 8 * q;
			o[0] = mx, o[1] = mn, o[2] = sa, o[3] = (mx > 0.0 && ix != NO_INDEX) ? ix : -1.0;
			o[4] = s0 * dxdp, o[5] = s1 * dxdp, o[6] = s2 * dxdp, o[7] = 0.0;
		}

		// ---- selection ------------------------------------------------------------------------------------------------------------------------
		constexpr int SCAN_PER_THREAD = RECON_SCAN_CHUNK / 256;
		// within[c] = ex_t + (sum of |v| from the thread's first cell to c), ex_(t + 1) = ex_t + (the thread's sum): a cell of zero weight repeats
		// its predecessor's value bit for bit, so the running sum never decreases and a search for "first value above u" never lands on such a cell
		__global__ void __launch_bounds__(256) recon_scan_kernel(int np_, const double* __restrict__ rho, long cells, int q, double* __restrict__ within,
			double* __restrict__ offsets, long long* __restrict__ count)
		{
#pragma clang fp contract(off)
			__shared__ double tot[256];
			__shared__ int cnt[256];
			const int t = threadIdx.x;
			int comp;
			const double* __restrict__ el = plane_source(rho, np_, cells, q, comp);
			const long c0 = static_cast<long>(blockIdx.x) * RECON_SCAN_CHUNK + static_cast<long>(t) * SCAN_PER_THREAD;
			double run[SCAN_PER_THREAD];
			double s = 0.0;
			int nz = 0;
#pragma unroll
			for (int k = 0; k < SCAN_PER_THREAD; ++k)
			{
				const long c = c0 + k;
				const double a = c < cells ? fabs(el[2 * c + comp]) : 0.0;
				s += a, nz += a > 0.0;
				run[k] = s;
			}
			tot[t] = s, cnt[t] = nz;
			__syncthreads();
			if (t == 0)
			{
				double ex = 0.0;
				int n = 0;
				for (int i = 0; i < 256; ++i)
				{
					const double ti = tot[i];
					tot[i] = ex, ex += ti, n += cnt[i];
				}
				offsets[blockIdx.x + 1] = ex; // the chunk's sum; recon_offsets_kernel turns the sums into offsets
				count[blockIdx.x] = n;
			}
			__syncthreads();
			const double ex = tot[t];
#pragma unroll
			for (int k = 0; k < SCAN_PER_THREAD; ++k)
				if (c0 + k < cells) within[c0 + k] = ex + run[k];
		}
		__global__ void __launch_bounds__(64) recon_offsets_kernel(long nchunks, double* __restrict__ offsets, long long* __restrict__ count)
		{
#pragma clang fp contract(off)
			if (threadIdx.x != 0) return;
			double s = 0.0;
			long long n = 0;
			offsets[0] = 0.0;
			for (long k = 0; k < nchunks; ++k)
			{
				s += offsets[k + 1], offsets[k + 1] = s;
				n += count[k];
			}
			count[nchunks] = n;
		}
		__global__ void __launch_bounds__(256) recon_draw_kernel(const double* __restrict__ within, const double* __restrict__ offsets, long cells, int nx, int np,
			int q, int uniform, unsigned long long seed, unsigned k0, unsigned nk, int* __restrict__ draw_cell, int* __restrict__ mark)
		{
#pragma clang fp contract(off)
			const unsigned i = blockIdx.x * 256u + threadIdx.x;
			if (i >= nk) return;
			const unsigned k = k0 + i;
			unsigned c[4] = {k, static_cast<unsigned>(q), 0x5E1EC7u, 0u};
			philox4x32(c, static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32));
			const double u = unit53(c[0], c[1]), u2 = unit53(c[2], c[3]);
			long cell;
			if (uniform)
			{
				const int ix = min(static_cast<int>(u * nx), nx - 1), ip = min(static_cast<int>(u2 * np), np - 1);
				cell = static_cast<long>(ix) * np + ip;
			}
			else
			{
				const long nchunks = (cells + RECON_SCAN_CHUNK - 1) / RECON_SCAN_CHUNK;
				const double W = offsets[nchunks];
				double uk = u * W;
				if (uk >= W) uk = nextafter(W, 0.0);
				long lo = -1, hi = cells - 1; // running sum <= uk at lo (0 in front of the grid), > uk at hi (W at the last cell)
				while (hi - lo > 1)
				{
					const long mid = lo + (hi - lo) / 2;
					if (offsets[mid / RECON_SCAN_CHUNK] + within[mid] > uk) hi = mid;
					else lo = mid;
				}
				cell = hi;
			}
			draw_cell[i] = static_cast<int>(cell);
			atomicMin(&mark[cell], static_cast<int>(k));
		}
		// one workgroup: the draws of the batch in order; state[0] = distinct cells so far, state[1] = K once n_select are reached
		__global__ void __launch_bounds__(1024) recon_count_kernel(const int* __restrict__ draw_cell, const int* __restrict__ mark, unsigned k0, unsigned nk,
			int n_select, int* __restrict__ state, int* __restrict__ chosen)
		{
			__shared__ int part[1024];
			const int t = threadIdx.x;
			const int base = state[0];
			const unsigned per = (nk + 1023u) / 1024u, i0 = min(nk, t * per), i1 = min(nk, i0 + per);
			int n = 0;
			for (unsigned i = i0; i < i1; ++i) n += mark[draw_cell[i]] == static_cast<int>(k0 + i);
			part[t] = n;
			__syncthreads();
			if (t == 0)
			{
				int ex = 0;
				for (int i = 0; i < 1024; ++i)
				{
					const int v = part[i];
					part[i] = ex, ex += v;
				}
				state[0] = base + ex;
			}
			__syncthreads();
			int have = base + part[t];
			for (unsigned i = i0; i < i1 && have < n_select; ++i)
				if (mark[draw_cell[i]] == static_cast<int>(k0 + i))
				{
					chosen[have++] = draw_cell[i];
					if (have == n_select) state[1] = static_cast<int>(k0 + i + 1u);
				}
		}
		__global__ void __launch_bounds__(256) recon_gather_kernel(int np_, const double* __restrict__ rho, const double* __restrict__ x, int nx,
			const double* __restrict__ p, int np, int q, const int* __restrict__ chosen, int n_select, int* __restrict__ cells, double* __restrict__ X,
			double* __restrict__ y)
		{
			const int i = blockIdx.x * 256 + threadIdx.x;
			if (i >= n_select) return;
			int comp;
			const double* __restrict__ el = plane_source(rho, np_, static_cast<long>(nx) * np, q, comp);
			const int c = chosen[i], ix = c / np, ip = c % np;
			cells[2 * i] = ix, cells[2 * i + 1] = ip;
			X[2 * i] = x[ix], X[2 * i + 1] = p[ip];
			y[i] = el[2 * static_cast<long>(c) + comp];
		}

		// ---- reconstruction -------------------------------------------------------------------------------------------------------------------
		constexpr int RBM = 64, RBN = 64, RBK = 16; // x rows, p columns, k depth of a workgroup tile
		constexpr int RLS = RBK + 2;                // LDS row stride (doubles): the 16 rows a fragment read touches fall into 16 different bank pairs

		// Ax[a Npad + i] = coef b_i exp(-(a_x (x_a - X_i))^2 / 2), Ep[b Npad + i] = exp(-(a_p (p_b - P_i))^2 / 2); exact zeros for i >= N and on the padded rows
		__global__ void __launch_bounds__(256) recon_tables_kernel(const ReconArgs g)
		{
#pragma clang fp contract(off)
			const ReconPlane& P = g.plane[blockIdx.z];
			if (P.N == 0) return;
			const int which = blockIdx.y;
			const long rows = which ? g.rows_p : g.rows_x, idx = blockIdx.x * 256L + threadIdx.x;
			if (idx >= rows * P.Npad) return;
			const int row = static_cast<int>(idx / P.Npad), i = static_cast<int>(idx % P.Npad);
			double val = 0.0;
			if (i < P.N && row < (which ? g.np : g.nx))
			{
				const double d = which ? P.ap * (g.p[row] - P.X[2 * i + 1]) : P.ax * (g.x[row] - P.X[2 * i]);
				const double e = exp(-(d * d) / 2.0);
				val = which ? e : P.coef * P.b[i] * e;
			}
			(which ? P.Ep : P.Ax)[idx] = val;
		}
		template <int NP, typename PES>
		__global__ void __launch_bounds__(256) recon_energy_kernel(PES model, const double* __restrict__ x, int nx, double* __restrict__ energy)
		{
			const int a = blockIdx.x * 256 + threadIdx.x;
			if (a >= nx) return;
			double E[NP];
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x[a], model, E, C, Fd);
#pragma unroll
			for (int i = 0; i < NP; ++i) energy[static_cast<long>(a) * NP + i] = E[i];
		}

		// The epilogue of a 64 x 64 tile of element (ie, je) held in the MFMA result layout by four waves (2 x 2): the six terms of every cell of
		// this lane, in the order (fragment row, fragment column, register), reduced over the wave, then over the waves, into the tile's record
		template <int NP>
		__device__ __forceinline__ void recon_epilogue(const ReconArgs& g, const d4 (&acc)[2][2][2], int ie, int je, int a0, int b0, double (*red)[2 * RECON_SUMS])
		{
#pragma clang fp contract(off)
			const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
			const int fk = lane >> 4, fr = lane & 15;
			const int nplanes = ie == je ? 1 : 2;
			const int qs[2] = {ie * NP + je, je * NP + ie};
			const long cells = static_cast<long>(g.nx) * g.np;
			const double* __restrict__ el = g.rho + 2 * (static_cast<long>(ie) * NP + je) * cells;
			double s[2][RECON_SUMS];
#pragma unroll
			for (int c = 0; c < 2; ++c)
#pragma unroll
				for (int k = 0; k < RECON_SUMS; ++k) s[c][k] = 0.0;
#pragma unroll
			for (int i = 0; i < 2; ++i)
#pragma unroll
				for (int j = 0; j < 2; ++j)
#pragma unroll
					for (int r = 0; r < 4; ++r)
					{
						const int a = a0 + wm * 32 + i * 16 + fk + 4 * r, b = b0 + wn * 32 + j * 16 + fr;
						if (a >= g.nx || b >= g.np) continue;
						const long cell = static_cast<long>(a) * g.np + b;
						const d2 z = *reinterpret_cast<const d2*>(el + 2 * cell);
						const double v[2] = {z.x, z.y};
#pragma unroll
						for (int c = 0; c < 2; ++c)
						{
							if (c >= nplanes) break;
							const double mu = acc[c][i][j][r], d = mu - v[c];
							s[c][0] += d * d, s[c][4] += mu * mu, s[c][5] += mu * v[c];
							if (g.pred) g.pred[static_cast<long>(qs[c]) * cells + cell] = mu;
						}
						if (ie == je)
						{
							const double mu = acc[0][i][j][r], pb = g.p[b];
							s[0][1] += mu, s[0][2] += mu * g.energy[static_cast<long>(a) * NP + ie], s[0][3] += mu * (pb * pb / 2.0 / g.mass);
						}
					}
#pragma unroll
			for (int c = 0; c < 2; ++c)
#pragma unroll
				for (int k = 0; k < RECON_SUMS; ++k)
				{
					double val = s[c][k];
#pragma unroll
					for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o);
					if (lane == 0) red[w][c * RECON_SUMS + k] = val;
				}
			__syncthreads();
			if (t < 2 * RECON_SUMS)
			{
				const long tile = (static_cast<long>(blockIdx.z) * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y;
				g.records[tile * (2 * RECON_SUMS) + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
			}
		}

		// Fragment maps of v_mfma_f64_16x16x4_f64 (gple_gemm.hip): first operand X[i = lane & 15][k = lane >> 4], second Y[k = lane >> 4][j = lane & 15],
		// result D[i = (lane >> 4) + 4 reg][j = lane & 15].  X = Ax (rows x), Y = Ep^T (columns p): a lane's results are 16 consecutive p of one x.
		// One workgroup = 4 waves (2 x 2) on a 64 x 64 tile of one element i <= j; each wave a 32 x 32 sub-tile in 2 x 2 fragments, for the element's
		// one (diagonal) or two (Re, Im) planes one after the other; the epilogue reads the exact (re, im) pairs once.
		template <int NP>
		__global__ void __launch_bounds__(256, 2) recon_contract_kernel(const ReconArgs g)
		{
			__shared__ __attribute__((aligned(16))) double As[RBM * RLS], Es[RBN * RLS];
			__shared__ double red[4][2 * RECON_SUMS];
			const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
			const int fk = lane >> 4, fr = lane & 15;
			const int a0 = blockIdx.x * RBM, b0 = blockIdx.y * RBN;
			int ie, je;
			upper_element(NP, blockIdx.z, ie, je);
			const int nplanes = ie == je ? 1 : 2;
			const int qs[2] = {ie * NP + je, je * NP + ie};

			d4 acc[2][2][2]; // [plane][fragment row][fragment column]
#pragma unroll
			for (int c = 0; c < 2; ++c)
#pragma unroll
				for (int i = 0; i < 2; ++i)
#pragma unroll
					for (int j = 0; j < 2; ++j) acc[c][i][j] = (d4){0.0, 0.0, 0.0, 0.0};

			const int srow = t >> 3, scol = (t & 7) * 2; // staging: rows srow and srow + 32, two doubles at k = scol
#pragma unroll
			for (int c = 0; c < 2; ++c)
			{
				if (c >= nplanes) break;
				const ReconPlane& P = g.plane[qs[c]];
				const int nkb = P.N > 0 ? P.Npad / RBK : 0;
				const double* __restrict__ ax = P.Ax + static_cast<long>(a0 + srow) * P.Npad + scol;
				const double* __restrict__ ep = P.Ep + static_cast<long>(b0 + srow) * P.Npad + scol;
				const long half = 32L * P.Npad;
				d2 av[2], ev[2];
				auto load = [&](int kb) {
					av[0] = *reinterpret_cast<const d2*>(ax + kb * RBK), av[1] = *reinterpret_cast<const d2*>(ax + half + kb * RBK);
					ev[0] = *reinterpret_cast<const d2*>(ep + kb * RBK), ev[1] = *reinterpret_cast<const d2*>(ep + half + kb * RBK);
				};
				auto store = [&]() {
					*reinterpret_cast<d2*>(&As[srow * RLS + scol]) = av[0], *reinterpret_cast<d2*>(&As[(srow + 32) * RLS + scol]) = av[1];
					*reinterpret_cast<d2*>(&Es[srow * RLS + scol]) = ev[0], *reinterpret_cast<d2*>(&Es[(srow + 32) * RLS + scol]) = ev[1];
				};
				__syncthreads(); // the previous plane's last reads of the tiles
				if (nkb > 0)
				{
					load(0);
					store();
				}
				__syncthreads();
				for (int kb = 0; kb < nkb; ++kb)
				{
					if (kb + 1 < nkb) load(kb + 1);
#pragma unroll
					for (int kk = 0; kk < RBK; kk += 4)
					{
						double af[2], ef[2];
#pragma unroll
						for (int i = 0; i < 2; ++i) af[i] = As[(wm * 32 + i * 16 + fr) * RLS + kk + fk];
#pragma unroll
						for (int j = 0; j < 2; ++j) ef[j] = Es[(wn * 32 + j * 16 + fr) * RLS + kk + fk];
#pragma unroll
						for (int i = 0; i < 2; ++i)
#pragma unroll
							for (int j = 0; j < 2; ++j) acc[c][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], ef[j], acc[c][i][j], 0, 0, 0);
					}
					__syncthreads();
					if (kb + 1 < nkb)
					{
						store();
						__syncthreads();
					}
				}
			}

			recon_epilogue<NP>(g, acc, ie, je, a0, b0, red);
		}

		// ---- the cross-term kernel on the grid -------------------------------------------------------------------------------------------------
		// k = w_g^2 exp(-Q / 2), Q = (a dx + c dp)^2 + (b dp)^2 with dx = x_a - X_i, dp = p_b - P_i (W = [[a, 0], [c, b]]).  Around a tile centre
		// (x_c, p_c) taken from the grid, with u = x_a - x_c, v = p_b - p_c, s_i = x_c - X_i, t_i = p_c - P_i, g_i = a s_i + c t_i:
		//   -Q / 2 = [-(a u + g_i)^2 / 2 + g_i^2 / 4] + [-(c v + g_i)^2 / 2 + g_i^2 / 4 - (b (v + t_i))^2 / 2] - a c u v
		// an x operand (a, i), a p operand (b, i) and a factor of the cell.  With A_U = |a| max|u| and C_V = |c| max|v| over the tile at most
		// L = RECON_CROSS_LIMIT the operand exponents stay below L^2 / 2 and the cell's inside +-L^2; a (tile, plane) beyond L takes the plain
		// path, one exponential of the summed argument per (cell, point) into the same accumulators.  The per-point values live in LDS, RCH
		// points at a time: (g_i, g_i^2 / 4, t_i, coef b_i) for the centred form, (X_i, -, P_i, coef b_i) for the plain one; zeros for i >= N.
		constexpr int RCH = 512;
		// exp of an exponent that is never above L^2: below -800 the result is 0 either way, and a NaN from inf - inf of a far point's squares is 0 too
		__device__ __forceinline__ double exp_floor(double e) { return exp(fmax(e, -800.0)); }

		template <int NP>
		__global__ void __launch_bounds__(256, 2) recon_cross_kernel(const ReconArgs g)
		{
#pragma clang fp contract(off)
			__shared__ __attribute__((aligned(16))) double As[RBM * RLS], Es[RBN * RLS];
			__shared__ __attribute__((aligned(16))) double pg[RCH], pq[RCH], pt[RCH], pw[RCH];
			__shared__ double red[4][2 * RECON_SUMS];
			__shared__ double span[2]; // max |u|, max |v| over the tile's cells inside the grid
			const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
			const int fk = lane >> 4, fr = lane & 15;
			const int a0 = blockIdx.x * RBM, b0 = blockIdx.y * RBN;
			int ie, je;
			upper_element(NP, blockIdx.z, ie, je);
			const int nplanes = ie == je ? 1 : 2;
			const int qs[2] = {ie * NP + je, je * NP + ie};
			const int ac = min(a0 + RBM / 2, g.nx - 1), bc = min(b0 + RBN / 2, g.np - 1);
			const double xc = g.x[ac], pc = g.p[bc];

			if (w < 2)
			{
				const int r = (w ? b0 : a0) + lane;
				double d = r < (w ? g.np : g.nx) ? fabs(w ? g.p[r] - pc : g.x[r] - xc) : 0.0;
#pragma unroll
				for (int o = 32; o > 0; o >>= 1) d = fmax(d, __shfl_xor(d, o));
				if (lane == 0) span[w] = d;
			}

			d4 acc[2][2][2]; // [plane][fragment row][fragment column]
#pragma unroll
			for (int c = 0; c < 2; ++c)
#pragma unroll
				for (int i = 0; i < 2; ++i)
#pragma unroll
					for (int j = 0; j < 2; ++j) acc[c][i][j] = (d4){0.0, 0.0, 0.0, 0.0};

			// staging: this thread generates rows srow and srow + 32 of both slabs at k = scol, scol + 1; rows beyond the grid are exact zeros
			const int srow = t >> 3, scol = (t & 7) * 2;
			double us[2], vs[2];
			bool inx[2], inp[2];
#pragma unroll
			for (int r = 0; r < 2; ++r)
			{
				const int a = a0 + srow + 32 * r, b = b0 + srow + 32 * r;
				inx[r] = a < g.nx, inp[r] = b < g.np;
				us[r] = g.x[inx[r] ? a : ac] - xc, vs[r] = g.p[inp[r] ? b : bc] - pc;
			}
			// the plain path: the coordinates of this lane's cells in the MFMA result layout
			double xa[2][4], pb[2];
#pragma unroll
			for (int i = 0; i < 2; ++i)
#pragma unroll
				for (int r = 0; r < 4; ++r) xa[i][r] = g.x[min(a0 + wm * 32 + i * 16 + fk + 4 * r, g.nx - 1)];
#pragma unroll
			for (int j = 0; j < 2; ++j) pb[j] = g.p[min(b0 + wn * 32 + j * 16 + fr, g.np - 1)];
			__syncthreads(); // span

			bool centred[2] = {false, false};
#pragma unroll
			for (int c = 0; c < 2; ++c)
			{
				if (c >= nplanes) break;
				const ReconPlane& P = g.plane[qs[c]];
				const double wa = P.ax, wc = P.cross, wb = P.ap;
				centred[c] = fabs(wa) * span[0] <= RECON_CROSS_LIMIT && fabs(wc) * span[1] <= RECON_CROSS_LIMIT;
				const double au[2] = {wa * us[0], wa * us[1]}, cv[2] = {wc * vs[0], wc * vs[1]};
				const int npts = P.N > 0 ? P.Npad : 0;
				for (int i0 = 0; i0 < npts; i0 += RCH)
				{
					const int len = min(RCH, npts - i0);
					__syncthreads(); // the previous chunk's last reads of the point values and of the slabs
					for (int k = t; k < len; k += 256)
					{
						const int i = i0 + k;
						double gi = 0.0, qi = 0.0, ti = 0.0, wi = 0.0;
						if (i < P.N)
						{
							const double Xi = P.X[2 * i], Pi = P.X[2 * i + 1];
							wi = P.coef * P.b[i];
							if (centred[c])
							{
								ti = pc - Pi;
								gi = wa * (xc - Xi) + wc * ti;
								qi = 0.25 * (gi * gi);
							}
							else gi = Xi, ti = Pi;
						}
						pg[k] = gi, pq[k] = qi, pt[k] = ti, pw[k] = wi;
					}
					__syncthreads();
					if (centred[c])
					{
						const int nkb = len / RBK;
						d2 av[2], ev[2];
						auto generate = [&](int kb) {
							const int k = kb * RBK + scol;
							const d2 gk = *reinterpret_cast<const d2*>(&pg[k]), qk = *reinterpret_cast<const d2*>(&pq[k]);
							const d2 tk = *reinterpret_cast<const d2*>(&pt[k]), wk = *reinterpret_cast<const d2*>(&pw[k]);
#pragma unroll
							for (int r = 0; r < 2; ++r)
#pragma unroll
								for (int h = 0; h < 2; ++h)
								{
									const double mx = au[r] + gk[h], mp = cv[r] + gk[h], d = wb * (vs[r] + tk[h]);
									const double ex = -0.5 * (mx * mx) + qk[h];
									const double ep = (-0.5 * (mp * mp) + qk[h]) - 0.5 * (d * d);
									av[r][h] = inx[r] ? wk[h] * exp_floor(ex) : 0.0;
									ev[r][h] = (inp[r] && i0 + k + h < P.N) ? exp_floor(ep) : 0.0;
								}
						};
						auto store = [&]() {
							*reinterpret_cast<d2*>(&As[srow * RLS + scol]) = av[0], *reinterpret_cast<d2*>(&As[(srow + 32) * RLS + scol]) = av[1];
							*reinterpret_cast<d2*>(&Es[srow * RLS + scol]) = ev[0], *reinterpret_cast<d2*>(&Es[(srow + 32) * RLS + scol]) = ev[1];
						};
						generate(0);
						store();
						__syncthreads();
						for (int kb = 0; kb < nkb; ++kb)
						{
							if (kb + 1 < nkb) generate(kb + 1);
#pragma unroll
							for (int kk = 0; kk < RBK; kk += 4)
							{
								double af[2], ef[2];
#pragma unroll
								for (int i = 0; i < 2; ++i) af[i] = As[(wm * 32 + i * 16 + fr) * RLS + kk + fk];
#pragma unroll
								for (int j = 0; j < 2; ++j) ef[j] = Es[(wn * 32 + j * 16 + fr) * RLS + kk + fk];
#pragma unroll
								for (int i = 0; i < 2; ++i)
#pragma unroll
									for (int j = 0; j < 2; ++j) acc[c][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], ef[j], acc[c][i][j], 0, 0, 0);
							}
							__syncthreads();
							if (kb + 1 < nkb)
							{
								store();
								__syncthreads();
							}
						}
					}
					else
					{
						const int n = min(len, P.N - i0);
						for (int k = 0; k < n; ++k)
						{
							const double Xi = pg[k], Pi = pt[k], wi = pw[k];
#pragma unroll
							for (int j = 0; j < 2; ++j)
							{
								const double dp = pb[j] - Pi, cd = wc * dp, bd = wb * dp, bb = bd * bd;
#pragma unroll
								for (int i = 0; i < 2; ++i)
#pragma unroll
									for (int r = 0; r < 4; ++r)
									{
										const double m = wa * (xa[i][r] - Xi) + cd;
										acc[c][i][j][r] += wi * exp_floor(-0.5 * (m * m + bb));
									}
							}
						}
					}
				}
				// the cell factor exp(-a c u v) of the centred form
				if (centred[c])
				{
					const double ac2 = wa * wc;
#pragma unroll
					for (int j = 0; j < 2; ++j)
					{
						const double v = pb[j] - pc;
#pragma unroll
						for (int i = 0; i < 2; ++i)
#pragma unroll
							for (int r = 0; r < 4; ++r) acc[c][i][j][r] *= exp(-(ac2 * (xa[i][r] - xc) * v));
					}
				}
			}
			recon_epilogue<NP>(g, acc, ie, je, a0, b0, red);
		}
		// sums[6 q + k]: one workgroup adds the tile records of every plane in a fixed order (a strided pass per thread, then a tree)
		template <int NP>
		__global__ void __launch_bounds__(256) recon_final_kernel(const ReconArgs g, long tiles)
		{
#pragma clang fp contract(off)
			__shared__ double red[RECON_SUMS][256];
			const int t = threadIdx.x;
			for (int q = 0; q < NP * NP; ++q)
			{
				const int r = q / NP, c = q % NP;
				const int i = r > c ? c : r, j = r > c ? r : c, comp = r > c;
				int e = j - i;
				for (int k = 0; k < i; ++k) e += NP - k;
				const double* rec = g.records + static_cast<long>(e) * tiles * (2 * RECON_SUMS) + comp * RECON_SUMS;
				double s[RECON_SUMS];
#pragma unroll
				for (int k = 0; k < RECON_SUMS; ++k) s[k] = 0.0;
				for (long tile = t; tile < tiles; tile += 256)
#pragma unroll
					for (int k = 0; k < RECON_SUMS; ++k) s[k] += rec[tile * (2 * RECON_SUMS) + k];
				__syncthreads(); // the previous plane's result has been read
#pragma unroll
				for (int k = 0; k < RECON_SUMS; ++k) red[k][t] = s[k];
				__syncthreads();
				for (int h = 128; h > 0; h >>= 1)
				{
					if (t < h)
#pragma unroll
						for (int k = 0; k < RECON_SUMS; ++k) red[k][t] += red[k][t + h];
					__syncthreads();
				}
				if (t < RECON_SUMS) g.sums[RECON_SUMS * q + t] = (t >= 1 && t <= 3) ? red[t][0] * g.dxdp : red[t][0];
			}
		}
	} // namespace

	size_t recon_survey_work_doubles(int num_pes) { return static_cast<size_t>(num_pes) * num_pes * RECON_SURVEY_BLOCKS * RECON_SURVEY_VALUES; }
	hipError_t launch_recon_survey(hipStream_t s, int num_pes, PesModel model, const double* rho, const double* x, int nx, const double* p, int np, double mass,
		double dxdp, double* work, double* out)
	{
		const dim3 grid(RECON_SURVEY_BLOCKS, num_pes * (num_pes + 1) / 2);
		if (num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((recon_survey_kernel<2, decltype(m)>), grid, dim3(256), 0, s, m, rho, x, nx, p, np, mass, work); });
		else if (num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((recon_survey_kernel<3, decltype(m)>), grid, dim3(256), 0, s, m, rho, x, nx, p, np, mass, work); });
		else return hipErrorInvalidValue;
		hipLaunchKernelGGL(recon_survey_final_kernel, dim3(1), dim3(64), 0, s, num_pes * num_pes, work, dxdp, out);
		return hipGetLastError();
	}

	long recon_scan_chunks(long cells) { return (cells + RECON_SCAN_CHUNK - 1) / RECON_SCAN_CHUNK; }
	hipError_t launch_recon_scan(hipStream_t s, int num_pes, const double* rho, long cells, int q, double* within, double* offsets, long long* count)
	{
		const long nchunks = recon_scan_chunks(cells);
		hipLaunchKernelGGL(recon_scan_kernel, dim3(static_cast<unsigned>(nchunks)), dim3(256), 0, s, num_pes, rho, cells, q, within, offsets, count);
		hipLaunchKernelGGL(recon_offsets_kernel, dim3(1), dim3(64), 0, s, nchunks, offsets, count);
		return hipGetLastError();
	}
	hipError_t launch_recon_draw(hipStream_t s, const double* within, const double* offsets, long cells, int nx, int np, int q, int uniform,
		unsigned long long seed, unsigned k0, unsigned nk, int* draw_cell, int* mark)
	{
		hipLaunchKernelGGL(recon_draw_kernel, dim3((nk + 255u) / 256u), dim3(256), 0, s, within, offsets, cells, nx, np, q, uniform, seed, k0, nk, draw_cell, mark);
		return hipGetLastError();
	}
	hipError_t launch_recon_count(hipStream_t s, const int* draw_cell, const int* mark, unsigned k0, unsigned nk, int n_select, int* state, int* chosen)
	{
		hipLaunchKernelGGL(recon_count_kernel, dim3(1), dim3(1024), 0, s, draw_cell, mark, k0, nk, n_select, state, chosen);
		return hipGetLastError();
	}
	hipError_t launch_recon_gather(hipStream_t s, int num_pes, const double* rho, const double* x, int nx, const double* p, int np, int q, const int* chosen,
		int n_select, int* cells, double* X, double* y)
	{
		hipLaunchKernelGGL(recon_gather_kernel, dim3((n_select + 255) / 256), dim3(256), 0, s, num_pes, rho, x, nx, p, np, q, chosen, n_select, cells, X, y);
		return hipGetLastError();
	}

	size_t recon_record_doubles(int num_pes, int nx, int np)
	{
		return static_cast<size_t>(num_pes * (num_pes + 1) / 2) * ((nx + RBM - 1) / RBM) * ((np + RBN - 1) / RBN) * (2 * RECON_SUMS);
	}
	hipError_t launch_recon_energy(hipStream_t s, const ReconArgs& g)
	{
		if (g.num_pes == 2) with_model(g.model, [&](auto m) { hipLaunchKernelGGL((recon_energy_kernel<2, decltype(m)>), dim3((g.nx + 255) / 256), dim3(256), 0, s, m, g.x, g.nx, g.energy); });
		else if (g.num_pes == 3) with_model(g.model, [&](auto m) { hipLaunchKernelGGL((recon_energy_kernel<3, decltype(m)>), dim3((g.nx + 255) / 256), dim3(256), 0, s, m, g.x, g.nx, g.energy); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_recon_tables(hipStream_t s, const ReconArgs& g)
	{
		int npad = 0;
		for (int q = 0; q < g.num_pes * g.num_pes; ++q)
			if (g.plane[q].N > 0) npad = g.plane[q].Npad > npad ? g.plane[q].Npad : npad;
		if (hipError_t e = launch_recon_energy(s, g); e != hipSuccess) return e;
		if (npad > 0)
		{
			const long rows = g.rows_x > g.rows_p ? g.rows_x : g.rows_p;
			const dim3 grid(static_cast<unsigned>((rows * npad + 255) / 256), 2, g.num_pes * g.num_pes);
			hipLaunchKernelGGL(recon_tables_kernel, grid, dim3(256), 0, s, g);
		}
		return hipGetLastError();
	}
	hipError_t launch_recon_contract(hipStream_t s, const ReconArgs& g)
	{
		const dim3 grid(g.rows_x / RBM, g.rows_p / RBN, g.num_pes * (g.num_pes + 1) / 2);
		if (g.num_pes == 2) hipLaunchKernelGGL(recon_contract_kernel<2>, grid, dim3(256), 0, s, g);
		else if (g.num_pes == 3) hipLaunchKernelGGL(recon_contract_kernel<3>, grid, dim3(256), 0, s, g);
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_recon_cross(hipStream_t s, const ReconArgs& g)
	{
		const dim3 grid(g.rows_x / RBM, g.rows_p / RBN, g.num_pes * (g.num_pes + 1) / 2);
		if (g.num_pes == 2) hipLaunchKernelGGL(recon_cross_kernel<2>, grid, dim3(256), 0, s, g);
		else if (g.num_pes == 3) hipLaunchKernelGGL(recon_cross_kernel<3>, grid, dim3(256), 0, s, g);
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_recon_final(hipStream_t s, const ReconArgs& g)
	{
		const long tiles = static_cast<long>(g.rows_x / RBM) * (g.rows_p / RBN);
		if (g.num_pes == 2) hipLaunchKernelGGL(recon_final_kernel<2>, dim3(1), dim3(256), 0, s, g, tiles);
		else if (g.num_pes == 3) hipLaunchKernelGGL(recon_final_kernel<3>, dim3(1), dim3(256), 0, s, g, tiles);
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
} // namespace gple
