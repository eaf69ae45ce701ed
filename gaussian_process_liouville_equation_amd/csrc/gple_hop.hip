// gple_hop.hip — independent-trajectory ensembles on the N-level potentials of gple_pes_n.h, built-in or tabulated: fewest-switches
// surface hopping (Tully, J. Chem. Phys. 93, 1061 (1990)) with its decoherence corrections, Ehrenfest (mean-field), symmetrical quasi-classical
// (SQC) and MASH trajectories.  The reference has no trajectory code: these are the methods its three models were made to test.
//
// One thread per trajectory; x, p, the diabatic amplitudes b, the active surface a and everything derived from them stay in registers for all
// the steps of a launch.  No LDS, no device globals, and no atomics but the integer ones of hop_bin_kernel, hop_bin_mf_kernel and hop_outgoing_kernel below.  Every piece that more than
// one method uses is one device function, stated once here; a method is a sampler, a force and a crossing rule on top of them.
//
// The shared pieces (V, Fd = -V', E, C: the diabatic matrix and force, the adiabatic energies and states; F = C^T Fd C, symmetrised as in
// gple_evolve_n.hip; c = C^T b the adiabatic amplitudes):
//     packet     (hop_draw_packet) x = x0 + sigma_x rho cospi(2 u1), p = p0 + sigma_p rho sinpi(2 u1), rho = sqrt(-2 log(1 - u0)), (u0, u1) = unit53
//                of the words (0, 1) and (2, 3) of Philox4x32-10, counter (offset + i, 0, 1, 0), key (seed low, seed high).  The grouped samples
//                (ZERO) leave the centre exactly where a sigma is exactly 0, by a select and not by 0 * rho.  Every sampler calls it: x and p of
//                one index, seed and packet have the same bits in every method
//     amplitudes (hop_amplitude_step) b <- W exp(-i lambda dt / hbar) W^T b, (lambda, W) the Jacobi eigen-system of the mid-point matrix
//                (V(x) + V(x_new)) / 2, U formed entry by entry: exactly unitary, no coupling needed.  The fewest-switches and the MASH step call
//                it, with the product of U b that is fused written out per method; the mapping step holds the same lines in plain form (see there)
//     b = C c    (diabatic_amplitudes) the samplers that draw c, and the decoherence correction
//     boundary   x < x_left: status 1, x > x_right: status 2; a finished trajectory is never read or written again
//     start      every step loop has a pass s = -1 that only forms what the first step needs at x (V, the forces, MASH's side).  What a step
//                forms at x_new is what the next step needs at x, so it is formed at one place of the loop, by the same instructions, whether
//                a launch starts there or arrives there: evolve(a) then evolve(b) = evolve(a + b), bit for bit, for every method
//     groups     ("A curve in one launch") trajectory i of n_groups n_per_group belongs to group i / n_per_group, which has a
//                packet and a time step of its own.  The plain and the grouped kernels call the same device function per trajectory, so the
//                state of a group is, bit for bit, what the plain call gives for that slice
//     sums       (hop_observe_kernel, hop_observe_groups_kernel) the terms of a trajectory, a Terms policy of the method, are added over each
//                wave by a butterfly, one row of partial sums per wave, and a second kernel adds the rows of a column.  Every group has workgroups
//                of its own, so its rows are those of a plain launch over the group alone: the same tree, the same bits
//
// Fewest switches (hop_sample_one, hop_evolve_one, HopSurfaceTerms; numpy restatement: tests/hop_numpy.py).  The sample: the packet, b = column
// surface0 of C(x).  One step of length dt for a running trajectory:
//     1  p += F_aa(x) dt / 2,  x_new = x + p / m dt
//     2  the amplitudes
//     3  E, C, F at x_new,  p += F_aa(x_new) dt / 2
//     4  c = C^T b;  g_k = max(0, 2 dt (p / m) d_ak Re(conj(c_a) c_k) / |c_a|^2),  d_ak = F_ak / (E_a - E_k)  (0 where F_ak is exactly 0, or |c_a|^2 is)
//     5  xi = unit53 of the words (0, 1) of Philox4x32-10, counter (trajectory, step low, 0, step high), key (seed low, seed high);
//        hop to the first k != a (ascending) with xi < g_1 + ... + g_k
//     6  r = p^2 + 2 m (E_a - E_k):  r >= 0: p = sgn(p) sqrt(r), a = k;  r < 0: frustrated, nothing changes (reverse: p = -p)
//     6a (the instantiations with DC only; DESIGN.md §17, "Decoherence corrections") with a and p as step 6 left them, where |c_a|^2 != 0:
//        EDC: w = 1 if edc_c == 0 else Ekin / (Ekin + edc_c), Ekin = p^2 / 2 m;  k != a: f_k = exp(-dt |E_k - E_a| w / hbar), c_k <- f_k c_k;
//             c_a <- c_a sqrt(1 + sum_{k != a} |c_k|^2 (1 - f_k^2) / |c_a|^2)  (the old c_k: the norm the vector has is kept, no cancellation)
//        COLLAPSE_HOP after a hop taken, COLLAPSE_ATTEMPT after every hop wanted: c_a <- c_a / |c_a|, every other c_k <- 0
//        then b = C c (the phase of c_a kept: invariant under the flip of a column of C)
//     7  the boundary
// Everything is invariant under flipping a column of C, so the sign convention of the adiabatic states (which flips along x) needs no tracking.
//
// Mapping trajectories without an active surface (hop_evolve_mapping_one; numpy restatements: tests/hop_mf_numpy.py, tests/hop_sqc_numpy.py): no
// seed, no step counter, no offset and no eigen-system of V(x); a trajectory is x, p, b and its status and moves on a force f(x, b), a functor:
//     1  p += f(x, b) dt / 2,  x_new = x + p / m dt
//     2  the amplitudes
//     3  p += f(x_new, b_new) dt / 2,  x = x_new
//     4  the boundary
// Time-symmetric (second order) and unitary to rounding; nothing is random.
//   Ehrenfest (MeanFieldForce, HopMeanFieldTerms; DESIGN.md §17, "Mean-field (Ehrenfest) trajectories"): the force averaged over b,
//     f(x, b) = sum_i |b_i|^2 Fd_ii + 2 sum_{i<j} Fd_ij Re(conj(b_i) b_j)   (i ascending, then the pairs (i, j) ascending, i first)
//   sampled as fewest switches.  Its kernels have no gamma and read none.
//   SQC (hop_sample_sqc_one, SqcForce, HopSqcTerms; DESIGN.md §17, "Symmetrical quasi-classical trajectories"): the Meyer-Miller-Stock-Thoss mapping
//   Hamiltonian with the windows of Cotton and Miller.  b is not normalised: with e_k = |c_k|^2 and the action n_k = e_k - gamma,
//   H = p^2 / 2m + b^dagger V b - gamma tr V, and
//     f(x, b) = [the mean-field running sum] - gamma (Fd_00 + ... + Fd_{NP-1,NP-1})   (the trace left to right, the product, then the difference)
//   The sample: the packet and, for level k, (u_k, v_k) = unit53 of the words (0, 1) and (2, 3) of the counter (index, k, 2, 0);
//   c_k = sqrt(e_k) (cospi(2 v_k) + i sinpi(2 v_k)), b = C(x) c, with occ = surface0 and F = NP
//     square   (window 0):  e_k = delta_{k,occ} + 2 gamma u_k
//     triangle (window 1):  t = (1 - u_occ)^(1/F) (sqrt, cbrt),  e_occ = 2 - t,  e_j = u_j t  (j != occ)
//   The sums bin e into the final windows: a trajectory belongs to the first k ascending with
//     square:    1 <= e_k <= 1 + 2 gamma  and  e_j <= 2 gamma  for all j != k
//     triangle:  e_k >= 1  and  e_k + e_j <= 2  for all j != k
//   else to none.
//
// MASH (hop_sample_mash_one, hop_evolve_mash_one; Mannouch and Richardson, J. Chem. Phys. 158, 104111 (2023); DESIGN.md §17, "MASH trajectories";
// numpy restatement: tests/hop_mash_numpy.py), two levels only: the layout and the sums of fewest switches, but the active surface is a function
// of the amplitudes, side(c) = 1 if |c_1|^2 > |c_0|^2 else 0, and the step draws no random number.  The sample: the packet and
// (w0, w1) = unit53 of the words (0, 1) and (2, 3) of the counter (index, 0, 3, 0):
//     s = sqrt(1 - w0)  (density 2 s on (0, 1]: the weight 2 |S_z| drawn, so that populations are counts of the active surface)
//     a = surface0, o = 1 - a:  c_a = sqrt((1 + s) / 2),  c_o = sqrt((1 - s) / 2) (cospi(2 w1) + i sinpi(2 w1)),  b = C(x) c
// One step: steps 1 to 3 of fewest switches, then
//     4  c = C^T b, side_new = side(c), in every pass (s = -1 too); side_old is the pass before's
//     5  side_new != side_old and side_new != a:  r = p^2 + 2 m (E_a - E_side_new);  r >= 0: p = sgn(p) sqrt(r), a = side_new (a hop);
//        r < 0: p = -p, a stays (a frustrated hop: always reflected).  A crossing back to side_new == a changes nothing
//     6  the boundary
//
// A new method adds its sampler (hop_draw_packet, its own amplitudes, hop_store), its force functor for hop_evolve_mapping_one or its crossing rule
// in a loop of the shape of hop_evolve_one, a Terms policy where its sums differ, and the launchers, which go through hop_dispatch.
#include <type_traits>

#include "gple_kernels.h"
#include "gple_pes_n.h"
#include "gple_philox.h"

namespace gple
{
	namespace
	{
		constexpr int HOP_BLOCK = 256, HOP_WAVE = 64;
		constexpr double HBAR_HOP = 1.0;

		// v[a] for a run-time a: a chain of selects, since a run-time index would put the array into scratch
		template <int NP>
		__device__ __forceinline__ double pick(const double (&v)[NP], int a)
		{
			static_assert(NP == 2 || NP == 3);
			const double v0 = v[0], v1 = v[1], v2 = v[NP - 1];
			return a == 0 ? v0 : NP == 2 || a == 1 ? v1 : v2;
		}

		template <int NP>
		struct HopStates
		{
			Mat<NP> V, C, F; // diabatic matrix, adiabatic states (columns), adiabatic force matrix
			double E[NP];
		};
		// adiabatic_states_n with V kept, and F = C^T Fd C (pes.cpp:98-155 at N levels, as adiabatic_n of gple_evolve_n.hip forms it)
		template <int NP, typename M>
		__device__ __forceinline__ void hop_states(double x, const M& model, HopStates<NP>& s)
		{
			Mat<NP> Fd, A, FC;
			diabatic_n<NP>(x, model, s.V, Fd);
			A = s.V;
			jacobi_eig<NP>(A, s.E, s.C);
			adiabatic_sign_n<NP>(s.C);
#pragma unroll
			for (int i = 0; i < NP; ++i)
#pragma unroll
				for (int k = 0; k < NP; ++k)
				{
					double acc = 0.0;
#pragma unroll
					for (int j = 0; j < NP; ++j) acc += Fd.a[i][j] * s.C.a[j][k];
					FC.a[i][k] = acc;
				}
#pragma unroll
			for (int k = 0; k < NP; ++k)
#pragma unroll
				for (int l = 0; l <= k; ++l)
				{
					double a1 = 0.0, a2 = 0.0;
#pragma unroll
					for (int i = 0; i < NP; ++i) a1 += s.C.a[i][k] * FC.a[i][l], a2 += s.C.a[i][l] * FC.a[i][k];
					s.F.a[k][l] = s.F.a[l][k] = 0.5 * (a1 + a2);
				}
		}

		// c = C^T b
		template <int NP>
		__device__ __forceinline__ void adiabatic_amplitudes(const Mat<NP>& C, const double (&bre)[NP], const double (&bim)[NP], double (&cre)[NP], double (&cim)[NP])
		{
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				double re = 0.0, im = 0.0;
#pragma unroll
				for (int i = 0; i < NP; ++i) re += C.a[i][k] * bre[i], im += C.a[i][k] * bim[i];
				cre[k] = re, cim[k] = im;
			}
		}
		// b = C c
		template <int NP>
		__device__ __forceinline__ void diabatic_amplitudes(const Mat<NP>& C, const double (&cre)[NP], const double (&cim)[NP], double (&bre)[NP], double (&bim)[NP])
		{
#pragma unroll
			for (int r = 0; r < NP; ++r)
			{
				double re = 0.0, im = 0.0;
#pragma unroll
				for (int k = 0; k < NP; ++k) re += C.a[r][k] * cre[k], im += C.a[r][k] * cim[k];
				bre[r] = re, bim[r] = im;
			}
		}

		// The registers of trajectory i, at the head and the foot of a step or sample function (the surface, where a method has one, is the caller's)
		template <int NP>
		__device__ __forceinline__ void hop_load_b(const HopEnsemble& e, long i, double (&bre)[NP], double (&bim)[NP])
		{
			const double* const b = e.b + 2 * NP * i;
#pragma unroll
			for (int k = 0; k < NP; ++k) bre[k] = b[2 * k], bim[k] = b[2 * k + 1];
		}
		template <int NP>
		__device__ __forceinline__ void hop_load(const HopEnsemble& e, long i, double& x, double& p, double (&bre)[NP], double (&bim)[NP])
		{
			x = e.x[i], p = e.p[i];
			hop_load_b<NP>(e, i, bre, bim);
		}
		template <int NP>
		__device__ __forceinline__ void hop_store(const HopEnsemble& e, long i, double x, double p, const double (&bre)[NP], const double (&bim)[NP], int status)
		{
			e.x[i] = x, e.p[i] = p, e.status[i] = status;
			double* const b = e.b + 2 * NP * i;
#pragma unroll
			for (int k = 0; k < NP; ++k) b[2 * k] = bre[k], b[2 * k + 1] = bim[k];
		}
		// b, and E and c = C^T b at x: what the sums and the density take from a stored trajectory
		template <int NP, typename M>
		__device__ __forceinline__ void hop_adiabatic(const HopEnsemble& e, const M& model, long i, double x, double (&E)[NP], double (&cre)[NP], double (&cim)[NP])
		{
			double bre[NP], bim[NP];
			hop_load_b<NP>(e, i, bre, bim);
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			adiabatic_amplitudes<NP>(C, bre, bim, cre, cim);
		}

		// The packet: x and p of trajectory i of every sampler
		template <bool ZERO>
		__device__ __forceinline__ void hop_draw_packet(const HopEnsemble& e, long i, double x0, double p0, double sigma_x, double sigma_p, double& x, double& p)
		{
			const unsigned long long index = e.offset + static_cast<unsigned long long>(i);
			unsigned c[4] = {static_cast<unsigned>(index), 0u, 1u, 0u};
			philox4x32(c, static_cast<unsigned>(e.seed), static_cast<unsigned>(e.seed >> 32));
			const double u0 = unit53(c[0], c[1]), u1 = unit53(c[2], c[3]);
			const double rho = sqrt(-2.0 * log(1.0 - u0));
			double sn, cs;
			sincospi(2.0 * u1, &sn, &cs);
			x = x0 + sigma_x * rho * cs, p = p0 + sigma_p * rho * sn;
			if constexpr (ZERO) x = sigma_x == 0.0 ? x0 : x, p = sigma_p == 0.0 ? p0 : p;
		}

		// The amplitudes through the mid-point matrix of Vx = V(x) and Vn = V(x_new), U = W exp(-i lambda dt / hbar) W^T entry by entry.  In U b
		// one product of each part is fused into the sum and the other is rounded first, and which one changes the last bit.  Left to the compiler
		// the choice went by the surrounding code: Re by its first product in both callers, Im by Im U Re b in the fewest-switches kernels and by
		// Re U Im b (IM_URE) in the MASH kernels.  It is written out, so that both keep the bits they have had wherever the function is called
		template <int NP, bool IM_URE>
		__device__ __forceinline__ void hop_amplitude_step(const Mat<NP>& Vx, const Mat<NP>& Vn, double dt, double (&bre)[NP], double (&bim)[NP])
		{
			Mat<NP> Vm, W;
			double lam[NP], cs[NP], sn[NP];
#pragma unroll
			for (int r = 0; r < NP; ++r)
#pragma unroll
				for (int q = 0; q < NP; ++q) Vm.a[r][q] = 0.5 * (Vx.a[r][q] + Vn.a[r][q]);
			jacobi_eig<NP>(Vm, lam, W);
#pragma unroll
			for (int k = 0; k < NP; ++k) sincos(lam[k] * dt / HBAR_HOP, &sn[k], &cs[k]);
			double nre[NP], nim[NP];
#pragma unroll
			for (int r = 0; r < NP; ++r)
			{
				double re = 0.0, im = 0.0;
#pragma unroll
				for (int q = 0; q < NP; ++q)
				{
					double ure = 0.0, uim = 0.0;
#pragma unroll
					for (int k = 0; k < NP; ++k)
					{
						const double ww = W.a[r][k] * W.a[q][k];
						ure += ww * cs[k], uim -= ww * sn[k];
					}
					re += fma(ure, bre[q], -(uim * bim[q]));
					im += IM_URE ? fma(ure, bim[q], uim * bre[q]) : fma(uim, bre[q], ure * bim[q]);
				}
				nre[r] = re, nim[r] = im;
			}
#pragma unroll
			for (int r = 0; r < NP; ++r) bre[r] = nre[r], bim[r] = nim[r];
		}

		// ---- fewest switches ---------------------------------------------------------------------------------------------------------------------
		// One trajectory of the sample: the packet, and column surface0 of C(x)
		template <int NP, typename M, bool ZERO>
		__device__ __forceinline__ void hop_sample_one(const HopEnsemble& e, const M& model, long i, double x0, double p0, double sigma_x, double sigma_p, int surface0)
		{
			double x, p, E[NP], bre[NP], bim[NP];
			hop_draw_packet<ZERO>(e, i, x0, p0, sigma_x, sigma_p, x, p);
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				double row[NP];
#pragma unroll
				for (int r = 0; r < NP; ++r) row[r] = C.a[k][r];
				bre[k] = pick<NP>(row, surface0), bim[k] = 0.0;
			}
			e.surface[i] = surface0;
			hop_store<NP>(e, i, x, p, bre, bim, 0);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_sample_kernel(HopEnsemble e, M model, double x0, double p0, double sigma_x, double sigma_p, int surface0)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n) return;
			hop_sample_one<NP, M, false>(e, model, i, x0, p0, sigma_x, sigma_p, surface0);
		}
		// The grouped sample: trajectory i draws from the row (x0, p0, sigma_x, sigma_p) of its group in packets
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_sample_groups_kernel(HopEnsemble e, M model, long n_per_group, const double* __restrict__ packets, int surface0)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n) return;
			const double* const row = packets + 4 * (i / n_per_group);
			hop_sample_one<NP, M, true>(e, model, i, row[0], row[1], row[2], row[3], surface0);
		}

		// All the steps of a launch for the running trajectory i.  COUNT (the grouped call): step 6's two outcomes are counted in registers and
		// added to hops[2 i], hops[2 i + 1] at the end, where hops is not null.  DC: step 6a, mode (a GPLE_HOP_DC_* other than NONE) being
		// uniform over the launch; without DC neither mode nor edc_c is read
		template <int NP, typename M, bool COUNT, bool DC>
		__device__ __forceinline__ void hop_evolve_one(const HopEnsemble& e, const M& model, long i, double mass, double dt, unsigned long long first_step, long n_steps,
			double x_left, double x_right, int reverse, int* hops, int mode, double edc_c)
		{
			double x, p, bre[NP], bim[NP];
			hop_load<NP>(e, i, x, p, bre, bim);
			int taken = 0, frustrated = 0;
			int a = e.surface[i], status = 0;
			const unsigned index = static_cast<unsigned>(e.offset + static_cast<unsigned long long>(i));
			const unsigned key0 = static_cast<unsigned>(e.seed), key1 = static_cast<unsigned>(e.seed >> 32);
			Mat<NP> Vx; // V(x) and the diagonal of F(x): set by the pass s = -1, which only forms the states at the start point
			double Fx[NP];
			for (long s = -1; s < n_steps && status == 0; ++s)
			{
				double xn = x;
				if (s >= 0)
				{
					p += pick<NP>(Fx, a) * dt / 2.0;
					xn = x + p / mass * dt;
				}
				HopStates<NP> st;
				hop_states<NP>(xn, model, st);
				if (s >= 0)
				{
					// 2
					hop_amplitude_step<NP, false>(Vx, st.V, dt, bre, bim);
					// 3
					double Fdiag[NP], Fa[NP];
#pragma unroll
					for (int k = 0; k < NP; ++k)
					{
						Fdiag[k] = st.F.a[k][k];
						double column[NP];
#pragma unroll
						for (int r = 0; r < NP; ++r) column[r] = st.F.a[r][k];
						Fa[k] = pick<NP>(column, a);
					}
					p += pick<NP>(Fdiag, a) * dt / 2.0;
					x = xn;
					// 4, 5
					double cre[NP], cim[NP];
					adiabatic_amplitudes<NP>(st.C, bre, bim, cre, cim);
					const double are = pick<NP>(cre, a), aim = pick<NP>(cim, a), na = are * are + aim * aim, Ea = pick<NP>(st.E, a);
					const unsigned long long step = first_step + static_cast<unsigned long long>(s);
					unsigned c[4] = {index, static_cast<unsigned>(step), 0u, static_cast<unsigned>(step >> 32)};
					philox4x32(c, key0, key1);
					const double xi = unit53(c[0], c[1]), v = p / mass;
					double sum = 0.0;
					int target = -1;
#pragma unroll
					for (int k = 0; k < NP; ++k)
						if (k != a)
						{
							double g = 0.0;
							if (na != 0.0 && Fa[k] != 0.0)
							{
								const double d = Fa[k] / (Ea - st.E[k]);
								g = fmax(0.0, 2.0 * dt * v * d * (are * cre[k] + aim * cim[k]) / na);
							}
							sum += g;
							if (target < 0 && xi < sum) target = k;
						}
					// 6
					if (target >= 0)
					{
						const double r = p * p + 2.0 * mass * (Ea - pick<NP>(st.E, target));
						if (r >= 0.0) p = sgn_n(p) * sqrt(r), a = target;
						else if (reverse) p = -p;
						if constexpr (COUNT) taken += r >= 0.0 ? 1 : 0, frustrated += r >= 0.0 ? 0 : 1;
					}
					// 6a
					if constexpr (DC)
					{
						const double nre = pick<NP>(cre, a), nim = pick<NP>(cim, a), nn = nre * nre + nim * nim; // c_a of the surface step 6 left
						bool changed = false;
						if (nn != 0.0)
						{
							if (mode == GPLE_HOP_DC_EDC)
							{
								const double kinetic = p * p / 2.0 / mass, w = edc_c == 0.0 ? 1.0 : kinetic / (kinetic + edc_c), En = pick<NP>(st.E, a);
								double lost = 0.0;
#pragma unroll
								for (int k = 0; k < NP; ++k)
									if (k != a)
									{
										const double f = exp(-dt * fabs(st.E[k] - En) * w / HBAR_HOP);
										lost += (cre[k] * cre[k] + cim[k] * cim[k]) * (1.0 - f * f);
										cre[k] = f * cre[k], cim[k] = f * cim[k];
									}
								const double grow = sqrt(1.0 + lost / nn);
#pragma unroll
								for (int k = 0; k < NP; ++k) cre[k] = k == a ? cre[k] * grow : cre[k], cim[k] = k == a ? cim[k] * grow : cim[k];
								changed = true;
							}
							else if (target >= 0 && (mode == GPLE_HOP_DC_COLLAPSE_ATTEMPT || a == target)) // a == target: the hop was taken (target was not a before)
							{
								const double length = sqrt(nn);
#pragma unroll
								for (int k = 0; k < NP; ++k) cre[k] = k == a ? cre[k] / length : 0.0, cim[k] = k == a ? cim[k] / length : 0.0;
								changed = true;
							}
						}
						if (changed) diabatic_amplitudes<NP>(st.C, cre, cim, bre, bim);
					}
					// 7
					if (x < x_left) status = 1;
					else if (x > x_right) status = 2;
				}
				Vx = st.V;
#pragma unroll
				for (int k = 0; k < NP; ++k) Fx[k] = st.F.a[k][k];
			}
			e.surface[i] = a;
			hop_store<NP>(e, i, x, p, bre, bim, status);
			if constexpr (COUNT)
				if (hops) hops[2 * i] += taken, hops[2 * i + 1] += frustrated;
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_kernel(HopEnsemble e, M model, double mass, double dt, unsigned long long first_step, long n_steps,
			double x_left, double x_right, int reverse)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_one<NP, M, false, false>(e, model, i, mass, dt, first_step, n_steps, x_left, x_right, reverse, nullptr, 0, 0.0);
		}
		// The grouped step: the same trajectory code with the time step of the trajectory's group, dt[i / n_per_group], one load
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_groups_kernel(HopEnsemble e, M model, long n_per_group, double mass, const double* __restrict__ dt,
			unsigned long long first_step, long n_steps, double x_left, double x_right, int reverse, int* hops)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_one<NP, M, true, false>(e, model, i, mass, dt[i / n_per_group], first_step, n_steps, x_left, x_right, reverse, hops, 0, 0.0);
		}
		// The two step kernels with step 6a: the mode is a kernel argument, the same for every lane
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_dc_kernel(HopEnsemble e, M model, double mass, double dt, unsigned long long first_step, long n_steps,
			double x_left, double x_right, int reverse, int mode, double edc_c)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_one<NP, M, false, true>(e, model, i, mass, dt, first_step, n_steps, x_left, x_right, reverse, nullptr, mode, edc_c);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_groups_dc_kernel(HopEnsemble e, M model, long n_per_group, double mass, const double* __restrict__ dt,
			unsigned long long first_step, long n_steps, double x_left, double x_right, int reverse, int* hops, int mode, double edc_c)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_one<NP, M, true, true>(e, model, i, mass, dt[i / n_per_group], first_step, n_steps, x_left, x_right, reverse, hops, mode, edc_c);
		}

		// ---- the sums ----------------------------------------------------------------------------------------------------------------------------
		// every term added over the wave by a butterfly of lane exchanges (every lane of a launched wave takes part); lane 0 writes the row
		template <int WIDTH>
		__device__ __forceinline__ void hop_wave_sums(const double (&t)[WIDTH], double* __restrict__ row)
		{
			const int lane = threadIdx.x % HOP_WAVE;
#pragma unroll
			for (int q = 0; q < WIDTH; ++q)
			{
				double v = t[q];
#pragma unroll
				for (int m = HOP_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, HOP_WAVE);
				if (lane == 0) row[q] = v;
			}
		}
		// column q of `rows` partial rows: lane l adds the rows l, l + 64, ... in ascending order, then the same butterfly
		__device__ __forceinline__ double hop_column_sum(const double* __restrict__ partial, long rows, int width, int q, int lane)
		{
			double v = 0.0;
			for (long r = lane; r < rows; r += HOP_WAVE) v += partial[r * width + q];
#pragma unroll
			for (int m = HOP_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, HOP_WAVE);
			return v;
		}

		// The Terms policies: the arguments of a method's sums beyond the ensemble and the model, and the width(num_pes) terms of trajectory i.
		// The 4 NP + 3 terms of gple_hop_observe (include/gple.h): fewest switches and MASH
		struct HopSurfaceTerms
		{
			double mass;
			static constexpr int width(int num_pes) { return hop_observe_width(num_pes); }
			template <int NP, typename M>
			__device__ __forceinline__ void fill(const HopEnsemble& e, const M& model, long i, double (&t)[4 * NP + 3]) const
			{
				const double x = e.x[i], p = e.p[i];
				const int a = e.surface[i], status = e.status[i];
				double cre[NP], cim[NP], E[NP];
				hop_adiabatic<NP>(e, model, i, x, E, cre, cim);
				const int cell = status >= 0 && status <= 2 && a >= 0 && a < NP ? status * NP + a : -1;
#pragma unroll
				for (int q = 0; q < 3 * NP; ++q) t[q] = q == cell ? 1.0 : 0.0;
#pragma unroll
				for (int k = 0; k < NP; ++k) t[3 * NP + k] = cre[k] * cre[k] + cim[k] * cim[k];
				t[4 * NP] = x, t[4 * NP + 1] = p, t[4 * NP + 2] = p * p / 2.0 / mass + pick<NP>(E, a);
			}
		};
		// The 3 NP + 6 terms of gple_hop_observe_mf: there is no active surface, so a channel is weighted by |c_k|^2.  A status out of range adds
		// to no weight and to no count
		struct HopMeanFieldTerms
		{
			double mass;
			static constexpr int width(int num_pes) { return hop_observe_mf_width(num_pes); }
			template <int NP, typename M>
			__device__ __forceinline__ void fill(const HopEnsemble& e, const M& model, long i, double (&t)[3 * NP + 6]) const
			{
				const double x = e.x[i], p = e.p[i];
				const int status = e.status[i];
				double cre[NP], cim[NP], E[NP];
				hop_adiabatic<NP>(e, model, i, x, E, cre, cim);
				double potential = 0.0;
#pragma unroll
				for (int k = 0; k < NP; ++k)
				{
					const double w = cre[k] * cre[k] + cim[k] * cim[k];
					potential += w * E[k];
#pragma unroll
					for (int s = 0; s < 3; ++s) t[s * NP + k] = s == status ? w : 0.0;
				}
#pragma unroll
				for (int s = 0; s < 3; ++s) t[3 * NP + s] = s == status ? 1.0 : 0.0;
				t[3 * NP + 3] = x, t[3 * NP + 4] = p, t[3 * NP + 5] = p * p / 2.0 / mass + potential;
			}
		};
		// The 4 NP + 9 terms of gple_hop_observe_sqc: e_k = |c_k|^2, and the first window (k ascending) that holds e, else none.  A status out of
		// range adds nowhere
		struct HopSqcTerms
		{
			double mass;
			int window;
			double gamma;
			static constexpr int width(int num_pes) { return hop_observe_sqc_width(num_pes); }
			template <int NP, typename M>
			__device__ __forceinline__ void fill(const HopEnsemble& e, const M& model, long i, double (&t)[4 * NP + 9]) const
			{
				const double x = e.x[i], p = e.p[i];
				const int status = e.status[i];
				double cre[NP], cim[NP], E[NP], w[NP];
				hop_adiabatic<NP>(e, model, i, x, E, cre, cim);
				double potential = 0.0;
#pragma unroll
				for (int k = 0; k < NP; ++k)
				{
					w[k] = cre[k] * cre[k] + cim[k] * cim[k];
					potential += (w[k] - gamma) * E[k];
				}
				int found = -1;
#pragma unroll
				for (int k = NP - 1; k >= 0; --k) // descending, so that the least k that holds is what stays
				{
					bool square = w[k] >= 1.0 && w[k] <= 1.0 + 2.0 * gamma, triangle = w[k] >= 1.0;
#pragma unroll
					for (int j = 0; j < NP; ++j)
						if (j != k) square = square && w[j] <= 2.0 * gamma, triangle = triangle && w[k] + w[j] <= 2.0;
					if (window == GPLE_HOP_WINDOW_SQUARE ? square : triangle) found = k;
				}
				const bool counted = status >= 0 && status <= 2;
#pragma unroll
				for (int s = 0; s < 3; ++s)
				{
#pragma unroll
					for (int k = 0; k < NP; ++k) t[s * NP + k] = s == status && k == found ? 1.0 : 0.0;
					t[3 * NP + s] = s == status ? 1.0 : 0.0;
					t[3 * NP + 3 + s] = s == status && found < 0 ? 1.0 : 0.0;
				}
#pragma unroll
				for (int k = 0; k < NP; ++k) t[3 * NP + 6 + k] = counted ? w[k] : 0.0;
				t[4 * NP + 6] = counted ? x : 0.0, t[4 * NP + 7] = counted ? p : 0.0, t[4 * NP + 8] = counted ? p * p / 2.0 / mass + potential : 0.0;
			}
		};

		// First stage of the sums: the terms of trajectory i (zeros where there is none: lanes beyond the ensemble or the group), added over the wave
		template <int NP, typename M, typename Terms>
		__device__ __forceinline__ void hop_observe_wave(const HopEnsemble& e, const M& model, const Terms& terms, bool present, long i, double* __restrict__ row)
		{
			constexpr int WIDTH = Terms::width(NP);
			double t[WIDTH];
#pragma unroll
			for (int q = 0; q < WIDTH; ++q) t[q] = 0.0;
			if (present) terms.template fill<NP>(e, model, i, t);
			hop_wave_sums<WIDTH>(t, row);
		}
		template <int NP, typename M, typename Terms>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_kernel(HopEnsemble e, M model, Terms terms, double* __restrict__ partial)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			hop_observe_wave<NP>(e, model, terms, i < e.n, i, partial + (i / HOP_WAVE) * Terms::width(NP));
		}
		// Second stage, one wave per column
		__global__ void __launch_bounds__(HOP_WAVE) hop_observe_finish_kernel(const double* __restrict__ partial, long rows, int width, double* __restrict__ out)
		{
			const double v = hop_column_sum(partial, rows, width, blockIdx.x, threadIdx.x);
			if (threadIdx.x == 0) out[blockIdx.x] = v;
		}
		// The grouped sums: every group has blocks_per_group workgroups of its own, so its trajectory j sits in the wave and lane it has in a plain
		// launch over the group alone, and its rows_per_group = 4 blocks_per_group partial rows are the rows of that launch
		template <int NP, typename M, typename Terms>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_groups_kernel(HopEnsemble e, M model, long n_per_group, unsigned blocks_per_group, Terms terms,
			double* __restrict__ partial)
		{
			const long group = blockIdx.x / blocks_per_group;
			const long j = static_cast<long>(blockIdx.x % blocks_per_group) * HOP_BLOCK + threadIdx.x;
			hop_observe_wave<NP>(e, model, terms, j < n_per_group, group * n_per_group + j,
				partial + (group * blocks_per_group * (HOP_BLOCK / HOP_WAVE) + j / HOP_WAVE) * Terms::width(NP));
		}
		// one wave per group and column: block g width + q
		__global__ void __launch_bounds__(HOP_WAVE) hop_observe_finish_groups_kernel(const double* __restrict__ partial, long rows_per_group, int width, double* __restrict__ out)
		{
			const long group = blockIdx.x / width;
			const double v = hop_column_sum(partial + group * rows_per_group * width, rows_per_group, width, blockIdx.x % width, threadIdx.x);
			if (threadIdx.x == 0) out[blockIdx.x] = v;
		}

		// ---- mapping trajectories without an active surface: Ehrenfest and SQC ------------------------------------------------------------------------
		// f(x, b) = b^dagger Fd b, one running sum: the diagonal terms with i ascending, then 2 Fd_ij Re(conj(b_i) b_j) over the pairs i < j ascending
		struct MeanFieldForce
		{
			template <int NP>
			__device__ __forceinline__ double operator()(const Mat<NP>& Fd, const double (&bre)[NP], const double (&bim)[NP]) const
			{
				double f = 0.0;
#pragma unroll
				for (int i = 0; i < NP; ++i) f += (bre[i] * bre[i] + bim[i] * bim[i]) * Fd.a[i][i];
#pragma unroll
				for (int i = 0; i < NP; ++i)
#pragma unroll
					for (int j = i + 1; j < NP; ++j) f += 2.0 * Fd.a[i][j] * (bre[i] * bre[j] + bim[i] * bim[j]);
				return f;
			}
		};
		// f(x, b) = b^dagger Fd b - gamma tr Fd: the mean-field running sum, the trace left to right, the product, then the difference
		struct SqcForce
		{
			double gamma;
			template <int NP>
			__device__ __forceinline__ double operator()(const Mat<NP>& Fd, const double (&bre)[NP], const double (&bim)[NP]) const
			{
				double trace = Fd.a[0][0];
#pragma unroll
				for (int i = 1; i < NP; ++i) trace += Fd.a[i][i];
				return MeanFieldForce{}(Fd, bre, bim) - gamma * trace;
			}
		};
		// All the steps of a launch for the running trajectory i, on the force of the method.  Step 2 and the load and store of the trajectory stand
		// here in the plain expressions these kernels have always had, not as calls of hop_amplitude_step, hop_load and hop_store: which product of
		// U b the compiler fuses goes by the surrounding code, and with those calls the last bits of b moved ("One copy of each
		// shared piece").  As written the kernels compile to the instructions they had before the step became a template
		template <int NP, typename M, typename Force>
		__device__ __forceinline__ void hop_evolve_mapping_one(const HopEnsemble& e, const M& model, long i, double mass, double dt, long n_steps, double x_left,
			double x_right, const Force force)
		{
			double x = e.x[i], p = e.p[i], bre[NP], bim[NP];
			int status = 0;
			double* const b = e.b + 2 * NP * i;
#pragma unroll
			for (int k = 0; k < NP; ++k) bre[k] = b[2 * k], bim[k] = b[2 * k + 1];
			Mat<NP> Vx, Fx; // V(x) and Fd(x): set by the pass s = -1, which only forms them at the start point
			for (long s = -1; s < n_steps && status == 0; ++s)
			{
				double xn = x;
				if (s >= 0)
				{
					p += force(Fx, bre, bim) * dt / 2.0;
					xn = x + p / mass * dt;
				}
				Mat<NP> Vn, Fn;
				diabatic_n<NP>(xn, model, Vn, Fn);
				if (s >= 0)
				{
					// 2: the amplitudes through the mid-point matrix, U = W exp(-i lambda dt / hbar) W^T entry by entry
					Mat<NP> Vm, W;
					double lam[NP], cs[NP], sn[NP];
#pragma unroll
					for (int r = 0; r < NP; ++r)
#pragma unroll
						for (int q = 0; q < NP; ++q) Vm.a[r][q] = 0.5 * (Vx.a[r][q] + Vn.a[r][q]);
					jacobi_eig<NP>(Vm, lam, W);
#pragma unroll
					for (int k = 0; k < NP; ++k) sincos(lam[k] * dt / HBAR_HOP, &sn[k], &cs[k]);
					double nre[NP], nim[NP];
#pragma unroll
					for (int r = 0; r < NP; ++r)
					{
						double re = 0.0, im = 0.0;
#pragma unroll
						for (int q = 0; q < NP; ++q)
						{
							double ure = 0.0, uim = 0.0;
#pragma unroll
							for (int k = 0; k < NP; ++k)
							{
								const double ww = W.a[r][k] * W.a[q][k];
								ure += ww * cs[k], uim -= ww * sn[k];
							}
							re += ure * bre[q] - uim * bim[q], im += ure * bim[q] + uim * bre[q];
						}
						nre[r] = re, nim[r] = im;
					}
#pragma unroll
					for (int r = 0; r < NP; ++r) bre[r] = nre[r], bim[r] = nim[r];
					// 3
					p += force(Fn, bre, bim) * dt / 2.0;
					x = xn;
					// 4
					if (x < x_left) status = 1;
					else if (x > x_right) status = 2;
				}
				Vx = Vn, Fx = Fn;
			}
			e.x[i] = x, e.p[i] = p, e.status[i] = status;
#pragma unroll
			for (int k = 0; k < NP; ++k) b[2 * k] = bre[k], b[2 * k + 1] = bim[k];
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_mf_kernel(HopEnsemble e, M model, double mass, double dt, long n_steps, double x_left, double x_right)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_mapping_one<NP>(e, model, i, mass, dt, n_steps, x_left, x_right, MeanFieldForce{});
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_groups_mf_kernel(HopEnsemble e, M model, long n_per_group, double mass, const double* __restrict__ dt,
			long n_steps, double x_left, double x_right)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_mapping_one<NP>(e, model, i, mass, dt[i / n_per_group], n_steps, x_left, x_right, MeanFieldForce{});
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_sqc_kernel(HopEnsemble e, M model, double mass, double dt, long n_steps, double x_left, double x_right,
			double gamma)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_mapping_one<NP>(e, model, i, mass, dt, n_steps, x_left, x_right, SqcForce{gamma});
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_groups_sqc_kernel(HopEnsemble e, M model, long n_per_group, double mass, const double* __restrict__ dt,
			long n_steps, double x_left, double x_right, double gamma)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_mapping_one<NP>(e, model, i, mass, dt[i / n_per_group], n_steps, x_left, x_right, SqcForce{gamma});
		}

		// One trajectory of the SQC sample: the packet, then the energies e on the start window and the angles
		template <int NP, typename M, bool ZERO>
		__device__ __forceinline__ void hop_sample_sqc_one(const HopEnsemble& e, const M& model, long i, double x0, double p0, double sigma_x, double sigma_p, int surface0,
			int window, double gamma)
		{
			const unsigned long long index = e.offset + static_cast<unsigned long long>(i);
			const unsigned key0 = static_cast<unsigned>(e.seed), key1 = static_cast<unsigned>(e.seed >> 32);
			double x, p, E[NP];
			hop_draw_packet<ZERO>(e, i, x0, p0, sigma_x, sigma_p, x, p);
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			double u[NP], v[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				unsigned w[4] = {static_cast<unsigned>(index), static_cast<unsigned>(k), 2u, 0u};
				philox4x32(w, key0, key1);
				u[k] = unit53(w[0], w[1]), v[k] = unit53(w[2], w[3]);
			}
			const double root = 1.0 - pick<NP>(u, surface0), t = NP == 2 ? sqrt(root) : cbrt(root);
			double cre[NP], cim[NP], bre[NP], bim[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				const bool occupied = k == surface0;
				const double square = (occupied ? 1.0 : 0.0) + 2.0 * gamma * u[k], triangle = occupied ? 2.0 - t : u[k] * t;
				const double length = sqrt(window == GPLE_HOP_WINDOW_SQUARE ? square : triangle);
				double sn, cs;
				sincospi(2.0 * v[k], &sn, &cs);
				cre[k] = length * cs, cim[k] = length * sn;
			}
			diabatic_amplitudes<NP>(C, cre, cim, bre, bim);
			e.surface[i] = surface0;
			hop_store<NP>(e, i, x, p, bre, bim, 0);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_sample_sqc_kernel(HopEnsemble e, M model, double x0, double p0, double sigma_x, double sigma_p, int surface0,
			int window, double gamma)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n) return;
			hop_sample_sqc_one<NP, M, false>(e, model, i, x0, p0, sigma_x, sigma_p, surface0, window, gamma);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_sample_groups_sqc_kernel(HopEnsemble e, M model, long n_per_group, const double* __restrict__ packets, int surface0,
			int window, double gamma)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n) return;
			const double* const row = packets + 4 * (i / n_per_group);
			hop_sample_sqc_one<NP, M, true>(e, model, i, row[0], row[1], row[2], row[3], surface0, window, gamma);
		}

		// ---- the ensemble in phase space -------------------------------------------------------------------------------------------------------------
		// The ensemble's adiabatic density on a grid ("The ensemble in phase space"), first as integers: one thread per trajectory
		// adds 1 to the count plane of its active surface and rint(2^32 c_a conj(c_b)) (re, then im) to the two planes of every pair a < b, at the
		// cell of its nearest grid point, by no-return 64-bit integer atomics at agent scope.  Integer addition is associative: acc has the same
		// bits whatever order the adds arrive in.  A signed term is added as its two's complement.  The two tallies are counted over the wave by a
		// ballot first: one atomic per wave and tally
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_bin_kernel(HopEnsemble e, M model, HopGrid g, int bin_all, unsigned long long* __restrict__ acc)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			const long cells = g.n_x * g.n_p;
			bool binned = false, outside = false;
			if (i < e.n)
			{
				const int a = e.surface[i], status = e.status[i];
				if (status >= 0 && status <= 2 && a >= 0 && a < NP && (status == 0 || bin_all))
				{
					const double x = e.x[i], p = e.p[i];
					// in double before the conversion, and written so that a NaN or a huge value is outside
					const double fx = floor((x - g.x_first) / g.dx + 0.5), fp = floor((p - g.p_first) / g.dp + 0.5);
					binned = fx >= 0.0 && fx < static_cast<double>(g.n_x) && fp >= 0.0 && fp < static_cast<double>(g.n_p);
					outside = !binned;
					if (binned)
					{
						const long cell = static_cast<long>(fx) * g.n_p + static_cast<long>(fp);
						double cre[NP], cim[NP], E[NP];
						hop_adiabatic<NP>(e, model, i, x, E, cre, cim);
						atomicAdd(acc + a * cells + cell, 1ull);
						unsigned long long* plane = acc + NP * cells + cell;
#pragma unroll
						for (int k = 0; k < NP; ++k)
#pragma unroll
							for (int l = k + 1; l < NP; ++l)
							{
								const double re = cre[k] * cre[l] + cim[k] * cim[l], im = cim[k] * cre[l] - cre[k] * cim[l];
								atomicAdd(plane, static_cast<unsigned long long>(static_cast<long long>(rint(4294967296.0 * re))));
								atomicAdd(plane + cells, static_cast<unsigned long long>(static_cast<long long>(rint(4294967296.0 * im))));
								plane += 2 * cells;
							}
					}
				}
			}
			const unsigned long long in = __ballot(binned), out = __ballot(outside);
			if (threadIdx.x % HOP_WAVE == 0)
			{
				unsigned long long* tally = acc + hop_bin_planes(NP) * cells;
				if (in) atomicAdd(tally, static_cast<unsigned long long>(__popcll(in)));
				if (out) atomicAdd(tally + 1, static_cast<unsigned long long>(__popcll(out)));
			}
		}
		// The density of an ensemble without an active surface, or the second prescription of Landry, Falk and Subotnik for one that has one
		// ("The ensemble in phase space, from the amplitudes"): hop_bin_kernel with the populations from the amplitudes too.
		// e.surface is not read (the mean-field calls pass none).  A binned trajectory adds rint(2^32 |c_a|^2) to plane a for every a, so the
		// first NP planes hold weights in fixed point and no counts, and the coherence terms of hop_bin_kernel to the planes behind them: NP^2
		// no-return atomics.  A weight is at most 2^32 (to rounding) for a unit vector: 2^31 of them cannot overflow the signed sum of a cell.
		// The cell, the coherence terms and the tallies are hop_bin_kernel's lines, copied: shared as device functions they left that kernel
		// its registers but not its instructions, and its bits are pinned
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_bin_mf_kernel(HopEnsemble e, M model, HopGrid g, int bin_all, unsigned long long* __restrict__ acc)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			const long cells = g.n_x * g.n_p;
			bool binned = false, outside = false;
			if (i < e.n)
			{
				const int status = e.status[i];
				if (status >= 0 && status <= 2 && (status == 0 || bin_all))
				{
					const double x = e.x[i], p = e.p[i];
					const double fx = floor((x - g.x_first) / g.dx + 0.5), fp = floor((p - g.p_first) / g.dp + 0.5);
					binned = fx >= 0.0 && fx < static_cast<double>(g.n_x) && fp >= 0.0 && fp < static_cast<double>(g.n_p);
					outside = !binned;
					if (binned)
					{
						const long cell = static_cast<long>(fx) * g.n_p + static_cast<long>(fp);
						double cre[NP], cim[NP], E[NP];
						hop_adiabatic<NP>(e, model, i, x, E, cre, cim);
#pragma unroll
						for (int a = 0; a < NP; ++a)
						{
							const double w = cre[a] * cre[a] + cim[a] * cim[a];
							atomicAdd(acc + a * cells + cell, static_cast<unsigned long long>(static_cast<long long>(rint(4294967296.0 * w))));
						}
						unsigned long long* plane = acc + NP * cells + cell;
#pragma unroll
						for (int k = 0; k < NP; ++k)
#pragma unroll
							for (int l = k + 1; l < NP; ++l)
							{
								const double re = cre[k] * cre[l] + cim[k] * cim[l], im = cim[k] * cre[l] - cre[k] * cim[l];
								atomicAdd(plane, static_cast<unsigned long long>(static_cast<long long>(rint(4294967296.0 * re))));
								atomicAdd(plane + cells, static_cast<unsigned long long>(static_cast<long long>(rint(4294967296.0 * im))));
								plane += 2 * cells;
							}
					}
				}
			}
			const unsigned long long in = __ballot(binned), out = __ballot(outside);
			if (threadIdx.x % HOP_WAVE == 0)
			{
				unsigned long long* tally = acc + hop_bin_planes(NP) * cells;
				if (in) atomicAdd(tally, static_cast<unsigned long long>(__popcll(in)));
				if (out) atomicAdd(tally + 1, static_cast<unsigned long long>(__popcll(out)));
			}
		}
		// One thread per cell: the num_pes^2 planes of the phase.txt layout from the integers.  The lower triangle is formed from the negated
		// sum (exactly the conjugate, and +0 where the sum is 0).  WEIGHTS: the accumulator of hop_bin_mf_kernel, whose first NP planes are sums
		// of 2^32 |c_a|^2 and are scaled as the coherence sums are
		template <int NP, bool WEIGHTS>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_density_kernel(long cells, double w, const long long* __restrict__ acc, double* __restrict__ rho)
		{
			const long cell = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (cell >= cells) return;
			constexpr double SCALE = 1.0 / 4294967296.0;
#pragma unroll
			for (int a = 0; a < NP; ++a)
			{
				double* d = rho + 2 * ((a * NP + a) * cells + cell);
				const double sum = static_cast<double>(acc[a * cells + cell]);
				d[0] = (WEIGHTS ? sum * SCALE : sum) / w, d[1] = 0.0;
			}
			const long long* plane = acc + NP * cells + cell;
#pragma unroll
			for (int a = 0; a < NP; ++a)
#pragma unroll
				for (int b = a + 1; b < NP; ++b)
				{
					const long long re = plane[0], im = plane[cells];
					double *up = rho + 2 * ((a * NP + b) * cells + cell), *lo = rho + 2 * ((b * NP + a) * cells + cell);
					up[0] = lo[0] = static_cast<double>(re) * SCALE / w;
					up[1] = static_cast<double>(im) * SCALE / w, lo[1] = static_cast<double>(-im) * SCALE / w;
					plane += 2 * cells;
				}
		}

		// ---- what left the box ------------------------------------------------------------------------------------------------------------------------
		// The outgoing momentum or energy per channel (side, adiabatic level) of the finished trajectories ("What left the box";
		// include/gple.h, gple_hop_outgoing).  A form is the Terms policy of a method's sums and what a finished trajectory's terms say of its
		// channel: channel() returns the level k of a trajectory that sits in one plane (-1: in none) and fills w where WEIGHTED spreads it over
		// every level.  The terms are fill()'s own, so the weights and the energy are the expressions the sums add.  Every index into t is a
		// constant after unrolling: nothing goes to scratch
		// the level k whose count term [status][k], one of the first 3 NP terms of the surface and the window sums, is set; -1: none is
		template <int NP, int WIDTH>
		__device__ __forceinline__ int hop_counted_level(const double (&t)[WIDTH], int status)
		{
			int found = -1;
#pragma unroll
			for (int s = 1; s <= 2; ++s)
#pragma unroll
				for (int k = 0; k < NP; ++k) found = s == status && t[s * NP + k] != 0.0 ? k : found;
			return found;
		}
		struct HopOutSurface
		{
			using Terms = HopSurfaceTerms;
			static constexpr bool WEIGHTED = false, TALLY_NONE = false; // a surface out of range is skipped, as the sums skip it
			Terms terms;
			template <int NP>
			__device__ __forceinline__ static int channel(const double (&t)[Terms::width(NP)], int status, double (&)[NP])
			{
				return hop_counted_level<NP>(t, status);
			}
		};
		struct HopOutMeanField
		{
			using Terms = HopMeanFieldTerms;
			static constexpr bool WEIGHTED = true, TALLY_NONE = false;
			Terms terms;
			template <int NP>
			__device__ __forceinline__ static int channel(const double (&t)[Terms::width(NP)], int status, double (&w)[NP])
			{
#pragma unroll
				for (int k = 0; k < NP; ++k) w[k] = status == 1 ? t[NP + k] : t[2 * NP + k];
				return 0;
			}
		};
		struct HopOutSqc
		{
			using Terms = HopSqcTerms;
			static constexpr bool WEIGHTED = false, TALLY_NONE = true; // no window: the tally `unassigned`
			Terms terms;
			template <int NP>
			__device__ __forceinline__ static int channel(const double (&t)[Terms::width(NP)], int status, double (&)[NP])
			{
				return hop_counted_level<NP>(t, status);
			}
		};
		// One thread per trajectory.  A finished one (status 1: side 0, status 2: side 1) on the grid adds 2^32 to the plane of its channel, or
		// rint(2^32 w_k) to every plane of its side, at the bin of its nearest grid point, by the no-return 64-bit integer atomics at agent scope
		// of hop_bin_kernel: any order, the same bits.  The four tallies are counted over the wave by a ballot first, one atomic per wave and tally
		template <int NP, typename M, typename Form>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_outgoing_kernel(HopEnsemble e, M model, Form form, HopAxis g, unsigned long long* __restrict__ acc)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			bool binned = false, outside = false, running = false, unassigned = false;
			if (i < e.n)
			{
				const int status = e.status[i];
				running = status == 0;
				if (status == 1 || status == 2)
				{
					constexpr int WIDTH = Form::Terms::width(NP);
					double t[WIDTH], w[NP];
					form.terms.template fill<NP>(e, model, i, t);
					const int k = Form::template channel<NP>(t, status, w);
					unassigned = Form::TALLY_NONE && k < 0;
					if (k >= 0)
					{
						const double q = g.energy ? t[WIDTH - 1] : e.p[i];
						// in double before the conversion, and written so that a NaN or a huge value is outside
						const double f = floor((q - g.first) / g.step + 0.5);
						binned = f >= 0.0 && f < static_cast<double>(g.n_bins);
						outside = !binned;
						if (binned)
						{
							unsigned long long* const side = acc + (status - 1) * NP * g.n_bins + static_cast<long>(f);
							if constexpr (Form::WEIGHTED)
							{
#pragma unroll
								for (int l = 0; l < NP; ++l)
									atomicAdd(side + l * g.n_bins, static_cast<unsigned long long>(static_cast<long long>(rint(4294967296.0 * w[l]))));
							}
							else atomicAdd(side + k * g.n_bins, 4294967296ull);
						}
					}
				}
			}
			const unsigned long long in = __ballot(binned), out = __ballot(outside), on = __ballot(running), none = __ballot(unassigned);
			if (threadIdx.x % HOP_WAVE == 0)
			{
				unsigned long long* tally = acc + 2 * NP * g.n_bins;
				if (in) atomicAdd(tally, static_cast<unsigned long long>(__popcll(in)));
				if (out) atomicAdd(tally + 1, static_cast<unsigned long long>(__popcll(out)));
				if (on) atomicAdd(tally + 2, static_cast<unsigned long long>(__popcll(on)));
				if (none) atomicAdd(tally + 3, static_cast<unsigned long long>(__popcll(none)));
			}
		}

		// ---- MASH ------------------------------------------------------------------------------------------------------------------------------------
		// side(c): the adiabatic state with the larger population, 1 if |c_1|^2 > |c_0|^2 else 0 (the sign of the mapping spin's S_z)
		__device__ __forceinline__ int mash_side(const double (&cre)[2], const double (&cim)[2])
		{
			return cre[1] * cre[1] + cim[1] * cim[1] > cre[0] * cre[0] + cim[0] * cim[0] ? 1 : 0;
		}
		// One trajectory of the sample: the packet, then s = |S_z| with the density 2 s and the angle of the other amplitude
		template <int NP, typename M, bool ZERO>
		__device__ __forceinline__ void hop_sample_mash_one(const HopEnsemble& e, const M& model, long i, double x0, double p0, double sigma_x, double sigma_p, int surface0)
		{
			static_assert(NP == 2, "MASH is a two-level method");
			const unsigned long long index = e.offset + static_cast<unsigned long long>(i);
			double x, p, E[NP];
			hop_draw_packet<ZERO>(e, i, x0, p0, sigma_x, sigma_p, x, p);
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			unsigned w[4] = {static_cast<unsigned>(index), 0u, 3u, 0u};
			philox4x32(w, static_cast<unsigned>(e.seed), static_cast<unsigned>(e.seed >> 32));
			const double w0 = unit53(w[0], w[1]), w1 = unit53(w[2], w[3]);
			const double s = sqrt(1.0 - w0), active = sqrt((1.0 + s) / 2.0), other = sqrt((1.0 - s) / 2.0);
			double sn, cs;
			sincospi(2.0 * w1, &sn, &cs);
			double cre[NP], cim[NP], bre[NP], bim[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k) cre[k] = k == surface0 ? active : other * cs, cim[k] = k == surface0 ? 0.0 : other * sn;
			diabatic_amplitudes<NP>(C, cre, cim, bre, bim);
			e.surface[i] = surface0;
			hop_store<NP>(e, i, x, p, bre, bim, 0);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_sample_mash_kernel(HopEnsemble e, M model, double x0, double p0, double sigma_x, double sigma_p, int surface0)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n) return;
			hop_sample_mash_one<NP, M, false>(e, model, i, x0, p0, sigma_x, sigma_p, surface0);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_sample_groups_mash_kernel(HopEnsemble e, M model, long n_per_group, const double* __restrict__ packets, int surface0)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n) return;
			const double* const row = packets + 4 * (i / n_per_group);
			hop_sample_mash_one<NP, M, true>(e, model, i, row[0], row[1], row[2], row[3], surface0);
		}

		// All the steps of a launch for the running trajectory i.  COUNT (the grouped call): the two outcomes of a crossing are counted in registers
		// and added to hops[2 i], hops[2 i + 1] at the end, where hops is not null
		template <int NP, typename M, bool COUNT>
		__device__ __forceinline__ void hop_evolve_mash_one(const HopEnsemble& e, const M& model, long i, double mass, double dt, long n_steps, double x_left, double x_right,
			int* hops)
		{
			static_assert(NP == 2, "MASH is a two-level method");
			double x, p, bre[NP], bim[NP];
			hop_load<NP>(e, i, x, p, bre, bim);
			int taken = 0, frustrated = 0;
			int a = e.surface[i], status = 0, side = 0;
			Mat<NP> Vx; // V(x), the diagonal of F(x) and side(c): set by the pass s = -1, which only forms the states and the side at the start point
			double Fx[NP];
			for (long s = -1; s < n_steps && status == 0; ++s)
			{
				double xn = x;
				if (s >= 0)
				{
					p += pick<NP>(Fx, a) * dt / 2.0;
					xn = x + p / mass * dt;
				}
				HopStates<NP> st;
				hop_states<NP>(xn, model, st);
				if (s >= 0)
				{
					// 2
					hop_amplitude_step<NP, true>(Vx, st.V, dt, bre, bim);
					// 3
					double Fdiag[NP];
#pragma unroll
					for (int k = 0; k < NP; ++k) Fdiag[k] = st.F.a[k][k];
					p += pick<NP>(Fdiag, a) * dt / 2.0;
					x = xn;
				}
				// 4: the side of the amplitudes at this point, in every pass: the start of a launch forms it as the end of the launch before did
				double cre[NP], cim[NP];
				adiabatic_amplitudes<NP>(st.C, bre, bim, cre, cim);
				const int side_new = mash_side(cre, cim);
				if (s >= 0)
				{
					// 5: the crossing: the amplitudes changed side, away from the active surface
					if (side_new != side && side_new != a)
					{
						const double r = p * p + 2.0 * mass * (pick<NP>(st.E, a) - pick<NP>(st.E, side_new));
						if (r >= 0.0) p = sgn_n(p) * sqrt(r), a = side_new;
						else p = -p;
						if constexpr (COUNT) taken += r >= 0.0 ? 1 : 0, frustrated += r >= 0.0 ? 0 : 1;
					}
					// 6
					if (x < x_left) status = 1;
					else if (x > x_right) status = 2;
				}
				side = side_new;
				Vx = st.V;
#pragma unroll
				for (int k = 0; k < NP; ++k) Fx[k] = st.F.a[k][k];
			}
			e.surface[i] = a;
			hop_store<NP>(e, i, x, p, bre, bim, status);
			if constexpr (COUNT)
				if (hops) hops[2 * i] += taken, hops[2 * i + 1] += frustrated;
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_mash_kernel(HopEnsemble e, M model, double mass, double dt, long n_steps, double x_left, double x_right)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_mash_one<NP, M, false>(e, model, i, mass, dt, n_steps, x_left, x_right, nullptr);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_groups_mash_kernel(HopEnsemble e, M model, long n_per_group, double mass, const double* __restrict__ dt,
			long n_steps, double x_left, double x_right, int* hops)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_mash_one<NP, M, true>(e, model, i, mass, dt[i / n_per_group], n_steps, x_left, x_right, hops);
		}

		// ---- the launchers' shared parts ---------------------------------------------------------------------------------------------------------------
		inline unsigned hop_blocks(long n) { return static_cast<unsigned>((n + HOP_BLOCK - 1) / HOP_BLOCK); }

		// launch(np, m) with np an std::integral_constant of e.num_pes (2 ... MAX_NP) and m the model as with_model hands it over: the launchers
		// instantiate their kernel for <np, decltype(m)>.  Any other num_pes is hipErrorInvalidValue
		template <int MAX_NP = 3, typename Launch>
		hipError_t hop_dispatch(const HopEnsemble& e, const PesModel& model, Launch&& launch)
		{
			if (e.num_pes < 2 || e.num_pes > MAX_NP) return hipErrorInvalidValue;
			if (e.num_pes == 2) with_model(model, [&](auto m) { launch(std::integral_constant<int, 2>{}, m); });
			if constexpr (MAX_NP >= 3)
				if (e.num_pes == 3) with_model(model, [&](auto m) { launch(std::integral_constant<int, 3>{}, m); });
			return hipGetLastError();
		}
		// a kernel with one thread per trajectory
		template <typename Kernel, typename... Args>
		void hop_launch(hipStream_t s, long n, Kernel kernel, const Args&... args)
		{
			hipLaunchKernelGGL(kernel, dim3(hop_blocks(n)), dim3(HOP_BLOCK), 0, s, args...);
		}
		// Both stages of the sums of a method, plain (one row of sums over the whole ensemble: n_groups = 1, n_per_group = e.n) or grouped
		template <typename Terms>
		hipError_t hop_observe(hipStream_t s, const HopEnsemble& e, const PesModel& model, bool grouped, long n_groups, long n_per_group, const Terms& terms,
			double* work, double* out)
		{
			if (n_groups <= 0 || n_per_group <= 0 || e.n != n_groups * n_per_group) return hipErrorInvalidValue;
			const unsigned per_group = hop_blocks(n_per_group);
			if (static_cast<unsigned long long>(n_groups) * per_group > 0x7FFFFFFFull) return hipErrorInvalidValue;
			const dim3 grid(static_cast<unsigned>(n_groups * per_group)), block(HOP_BLOCK);
			const hipError_t err = hop_dispatch(e, model, [&](auto np, auto m) {
				if (grouped) hipLaunchKernelGGL((hop_observe_groups_kernel<np(), decltype(m), Terms>), grid, block, 0, s, e, m, n_per_group, per_group, terms, work);
				else hipLaunchKernelGGL((hop_observe_kernel<np(), decltype(m), Terms>), grid, block, 0, s, e, m, terms, work);
			});
			if (err != hipSuccess) return err;
			const int width = Terms::width(e.num_pes);
			const long rows_per_group = static_cast<long>(per_group) * (HOP_BLOCK / HOP_WAVE);
			if (grouped) hipLaunchKernelGGL(hop_observe_finish_groups_kernel, dim3(static_cast<unsigned>(n_groups * width)), dim3(HOP_WAVE), 0, s, work, rows_per_group, width, out);
			else hipLaunchKernelGGL(hop_observe_finish_kernel, dim3(width), dim3(HOP_WAVE), 0, s, work, rows_per_group, width, out);
			return hipGetLastError();
		}
	} // namespace

	hipError_t launch_hop_sample(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0)
	{
		if (e.n <= 0) return hipSuccess;
		return hop_dispatch(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_sample_kernel<np(), decltype(m)>, e, m, x0, p0, sigma_x, sigma_p, surface0); });
	}
	hipError_t launch_hop_sample_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		return hop_dispatch(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_sample_groups_kernel<np(), decltype(m)>, e, m, n_per_group, packets, surface0); });
	}
	hipError_t launch_hop_evolve(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, unsigned long long first_step, long n_steps,
		double x_left, double x_right, bool reverse, int decoherence, double edc_c)
	{
		if (decoherence < GPLE_HOP_DC_NONE || decoherence > GPLE_HOP_DC_COLLAPSE_ATTEMPT) return hipErrorInvalidValue;
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		const int rev = reverse ? 1 : 0;
		return hop_dispatch(e, model, [&](auto np, auto m) {
			if (decoherence == GPLE_HOP_DC_NONE) hop_launch(s, e.n, hop_evolve_kernel<np(), decltype(m)>, e, m, mass, dt, first_step, n_steps, x_left, x_right, rev);
			else hop_launch(s, e.n, hop_evolve_dc_kernel<np(), decltype(m)>, e, m, mass, dt, first_step, n_steps, x_left, x_right, rev, decoherence, edc_c);
		});
	}
	hipError_t launch_hop_evolve_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, unsigned long long first_step,
		long n_steps, double x_left, double x_right, bool reverse, int* hops, int decoherence, double edc_c)
	{
		if (decoherence < GPLE_HOP_DC_NONE || decoherence > GPLE_HOP_DC_COLLAPSE_ATTEMPT) return hipErrorInvalidValue;
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		const int rev = reverse ? 1 : 0;
		return hop_dispatch(e, model, [&](auto np, auto m) {
			if (decoherence == GPLE_HOP_DC_NONE)
				hop_launch(s, e.n, hop_evolve_groups_kernel<np(), decltype(m)>, e, m, n_per_group, mass, dt, first_step, n_steps, x_left, x_right, rev, hops);
			else
				hop_launch(s, e.n, hop_evolve_groups_dc_kernel<np(), decltype(m)>, e, m, n_per_group, mass, dt, first_step, n_steps, x_left, x_right, rev, hops, decoherence,
					edc_c);
		});
	}
	size_t hop_observe_work_doubles(int width, long n_groups, long n_per_group)
	{
		return static_cast<size_t>(n_groups) * hop_blocks(n_per_group) * (HOP_BLOCK / HOP_WAVE) * width;
	}
	hipError_t launch_hop_observe(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double* work, double* out)
	{
		return hop_observe(s, e, model, false, 1, e.n, HopSurfaceTerms{mass}, work, out);
	}
	hipError_t launch_hop_observe_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, double* work, double* out)
	{
		return hop_observe(s, e, model, true, n_groups, n_per_group, HopSurfaceTerms{mass}, work, out);
	}

	hipError_t launch_hop_evolve_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right)
	{
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		return hop_dispatch(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_evolve_mf_kernel<np(), decltype(m)>, e, m, mass, dt, n_steps, x_left, x_right); });
	}
	hipError_t launch_hop_evolve_groups_mf(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		return hop_dispatch(e, model, [&](auto np, auto m) {
			hop_launch(s, e.n, hop_evolve_groups_mf_kernel<np(), decltype(m)>, e, m, n_per_group, mass, dt, n_steps, x_left, x_right);
		});
	}
	hipError_t launch_hop_observe_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double* work, double* out)
	{
		return hop_observe(s, e, model, false, 1, e.n, HopMeanFieldTerms{mass}, work, out);
	}
	hipError_t launch_hop_observe_groups_mf(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, double* work, double* out)
	{
		return hop_observe(s, e, model, true, n_groups, n_per_group, HopMeanFieldTerms{mass}, work, out);
	}

	hipError_t launch_hop_sample_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0, int window,
		double gamma)
	{
		if (e.n <= 0) return hipSuccess;
		return hop_dispatch(e, model, [&](auto np, auto m) {
			hop_launch(s, e.n, hop_sample_sqc_kernel<np(), decltype(m)>, e, m, x0, p0, sigma_x, sigma_p, surface0, window, gamma);
		});
	}
	hipError_t launch_hop_sample_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0, int window,
		double gamma)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		return hop_dispatch(e, model, [&](auto np, auto m) {
			hop_launch(s, e.n, hop_sample_groups_sqc_kernel<np(), decltype(m)>, e, m, n_per_group, packets, surface0, window, gamma);
		});
	}
	hipError_t launch_hop_evolve_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right, double gamma)
	{
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		return hop_dispatch(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_evolve_sqc_kernel<np(), decltype(m)>, e, m, mass, dt, n_steps, x_left, x_right, gamma); });
	}
	hipError_t launch_hop_evolve_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right, double gamma)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		return hop_dispatch(e, model, [&](auto np, auto m) {
			hop_launch(s, e.n, hop_evolve_groups_sqc_kernel<np(), decltype(m)>, e, m, n_per_group, mass, dt, n_steps, x_left, x_right, gamma);
		});
	}
	hipError_t launch_hop_observe_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, int window, double gamma, double* work, double* out)
	{
		return hop_observe(s, e, model, false, 1, e.n, HopSqcTerms{mass, window, gamma}, work, out);
	}
	hipError_t launch_hop_observe_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, int window, double gamma,
		double* work, double* out)
	{
		return hop_observe(s, e, model, true, n_groups, n_per_group, HopSqcTerms{mass, window, gamma}, work, out);
	}

	hipError_t launch_hop_sample_mash(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0)
	{
		if (e.num_pes != 2) return hipErrorInvalidValue;
		if (e.n <= 0) return hipSuccess;
		return hop_dispatch<2>(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_sample_mash_kernel<np(), decltype(m)>, e, m, x0, p0, sigma_x, sigma_p, surface0); });
	}
	hipError_t launch_hop_sample_groups_mash(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0)
	{
		if (e.num_pes != 2 || e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		return hop_dispatch<2>(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_sample_groups_mash_kernel<np(), decltype(m)>, e, m, n_per_group, packets, surface0); });
	}
	hipError_t launch_hop_evolve_mash(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right)
	{
		if (e.num_pes != 2) return hipErrorInvalidValue;
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		return hop_dispatch<2>(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_evolve_mash_kernel<np(), decltype(m)>, e, m, mass, dt, n_steps, x_left, x_right); });
	}
	hipError_t launch_hop_evolve_groups_mash(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right, int* hops)
	{
		if (e.num_pes != 2 || e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		return hop_dispatch<2>(e, model, [&](auto np, auto m) {
			hop_launch(s, e.n, hop_evolve_groups_mash_kernel<np(), decltype(m)>, e, m, n_per_group, mass, dt, n_steps, x_left, x_right, hops);
		});
	}

	hipError_t launch_hop_bin(hipStream_t s, const HopEnsemble& e, PesModel model, const HopGrid& g, bool bin_all, long long* acc)
	{
		if (e.n <= 0 || g.n_x <= 0 || g.n_p <= 0) return hipErrorInvalidValue;
		unsigned long long* const words = reinterpret_cast<unsigned long long*>(acc);
		const int all = bin_all ? 1 : 0;
		return hop_dispatch(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_bin_kernel<np(), decltype(m)>, e, m, g, all, words); });
	}
	hipError_t launch_hop_density(hipStream_t s, int num_pes, long cells, double w, const long long* acc, double* rho)
	{
		if (cells <= 0) return hipErrorInvalidValue;
		if (num_pes == 2) hop_launch(s, cells, hop_density_kernel<2, false>, cells, w, acc, rho);
		else if (num_pes == 3) hop_launch(s, cells, hop_density_kernel<3, false>, cells, w, acc, rho);
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}

	hipError_t launch_hop_bin_mf(hipStream_t s, const HopEnsemble& e, PesModel model, const HopGrid& g, bool bin_all, long long* acc)
	{
		if (e.n <= 0 || g.n_x <= 0 || g.n_p <= 0) return hipErrorInvalidValue;
		unsigned long long* const words = reinterpret_cast<unsigned long long*>(acc);
		const int all = bin_all ? 1 : 0;
		return hop_dispatch(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_bin_mf_kernel<np(), decltype(m)>, e, m, g, all, words); });
	}
	hipError_t launch_hop_density_mf(hipStream_t s, int num_pes, long cells, double w, const long long* acc, double* rho)
	{
		if (cells <= 0) return hipErrorInvalidValue;
		if (num_pes == 2) hop_launch(s, cells, hop_density_kernel<2, true>, cells, w, acc, rho);
		else if (num_pes == 3) hop_launch(s, cells, hop_density_kernel<3, true>, cells, w, acc, rho);
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}

	namespace
	{
		template <typename Form>
		hipError_t hop_outgoing(hipStream_t s, const HopEnsemble& e, const PesModel& model, const Form& form, const HopAxis& g, long long* acc)
		{
			if (e.n <= 0 || g.n_bins <= 0) return hipErrorInvalidValue;
			unsigned long long* const words = reinterpret_cast<unsigned long long*>(acc);
			return hop_dispatch(e, model, [&](auto np, auto m) { hop_launch(s, e.n, hop_outgoing_kernel<np(), decltype(m), Form>, e, m, form, g, words); });
		}
	} // namespace
	hipError_t launch_hop_outgoing(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, const HopAxis& g, long long* acc)
	{
		return hop_outgoing(s, e, model, HopOutSurface{{mass}}, g, acc);
	}
	hipError_t launch_hop_outgoing_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, const HopAxis& g, long long* acc)
	{
		return hop_outgoing(s, e, model, HopOutMeanField{{mass}}, g, acc);
	}
	hipError_t launch_hop_outgoing_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, int window, double gamma, const HopAxis& g, long long* acc)
	{
		return hop_outgoing(s, e, model, HopOutSqc{{mass, window, gamma}}, g, acc);
	}

	// ---- the ensemble in phase space, smoothed -------------------------------------------------------------------------------------------------------
	// The Gaussian sum of gple_hop_smooth and gple_hop_smooth_mf (include/gple.h; DESIGN.md §17, "The ensemble in phase space, smoothed"):
	// rho_q = s A_q B with A_q[k, i] = u_qi g_x(x_k - x_i) and B[i, j] = g_p(p_j - p_i), a GEMM over the trajectory index whose operands are
	// generated in LDS and never stored, on v_mfma_f64_16x16x4_f64 as wigner_kernel of gple_dvr.hip.  Three kernels: the terms (one thread per
	// trajectory), the contraction (a workgroup per 64 x 64 tile, trajectory chunk and plane group) and the finish (one thread per cell)
	namespace
	{
		typedef double sm4 __attribute__((ext_vector_type(4)));
		constexpr int SMT = 64;       // grid lines of a tile, in x and in p
		constexpr int SMK = 16;       // trajectories of a k block
		constexpr int SML = SMT + 8;  // LDS row stride of the g_x and g_p blocks (doubles)
		constexpr long SM_MIN_CHUNK = 256;              // trajectories: below this a chunk is not worth a workgroup
		constexpr long SM_WORKGROUPS = 1024;            // the split aims at this many workgroups: four to each of the chip's 256 CUs
		constexpr long SM_PARTIAL_DOUBLES = 1L << 24;   // the partial tiles of all chunks stay below this (128 MiB), or at one chunk
		constexpr int hop_smooth_group(int num_pes) { return num_pes == 2 ? 4 : 3; } // planes a workgroup accumulates: 4 of 4, or 3 of 9

		// One thread per trajectory of the padded index space: x_i, p_i and the num_pes^2 weights u_qi of a used trajectory, zeros for every
		// other one (unselected, skipped, not finite, padding): the contraction needs no mask and never sees a NaN.  Planes: u_a for the
		// diagonal a, then (re, im) per pair a < b in row-major order.  MF: the diagonal from the amplitudes and no surface, as hop_bin_mf_kernel;
		// otherwise 1 on the active surface, as hop_bin_kernel.  The two tallies go by ballot, one atomic per wave and tally
		template <int NP, typename M, bool MF>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_smooth_terms_kernel(HopEnsemble e, M model, int bin_all, long npad, double* __restrict__ xs,
			double* __restrict__ ps, double* __restrict__ u, unsigned long long* __restrict__ tally)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			bool used = false, nonfinite = false;
			double x = 0.0, p = 0.0, w[NP * NP];
#pragma unroll
			for (int q = 0; q < NP * NP; ++q) w[q] = 0.0;
			if (i < e.n)
			{
				int a = 0;
				if constexpr (!MF) a = e.surface[i];
				const int status = e.status[i];
				if (status >= 0 && status <= 2 && a >= 0 && a < NP && (status == 0 || bin_all))
				{
					const double xi = e.x[i], pi = e.p[i];
					used = isfinite(xi) && isfinite(pi);
					nonfinite = !used;
					if (used)
					{
						x = xi, p = pi;
						double cre[NP], cim[NP], E[NP];
						hop_adiabatic<NP>(e, model, i, xi, E, cre, cim);
#pragma unroll
						for (int k = 0; k < NP; ++k) w[k] = MF ? cre[k] * cre[k] + cim[k] * cim[k] : (a == k ? 1.0 : 0.0);
						int q = NP;
#pragma unroll
						for (int k = 0; k < NP; ++k)
#pragma unroll
							for (int l = k + 1; l < NP; ++l)
							{
								w[q] = cre[k] * cre[l] + cim[k] * cim[l], w[q + 1] = cim[k] * cre[l] - cre[k] * cim[l];
								q += 2;
							}
					}
				}
			}
			if (i < npad)
			{
				xs[i] = x, ps[i] = p;
#pragma unroll
				for (int q = 0; q < NP * NP; ++q) u[q * npad + i] = w[q];
			}
			const unsigned long long in = __ballot(used), bad = __ballot(nonfinite);
			if (threadIdx.x % HOP_WAVE == 0)
			{
				if (in) atomicAdd(tally, static_cast<unsigned long long>(__popcll(in)));
				if (bad) atomicAdd(tally + 1, static_cast<unsigned long long>(__popcll(bad)));
			}
		}

		struct HopSmoothArgs
		{
			const double *xs, *ps, *u; // npad each; u: num_pes^2 planes of npad
			double* partial;           // [chunk][plane][n_x][n_p]
			double x_first, dx, p_first, dp, h_x, h_p;
			long n_x, n_p, npad, chunk; // chunk: trajectories of a chunk, a multiple of SMK
			int tiles_p, planes;
		};

		// Fragment maps of v_mfma_f64_16x16x4_f64 (gple_gemm.hip): first operand X[i = lane & 15][k = lane >> 4], second Y[k = lane >> 4][j = lane & 15],
		// result D[i = (lane >> 4) + 4 reg][j = lane & 15].  X = u_q g_x (rows x), Y = g_p (columns p).  One workgroup = 4 waves (2 x 2) on a 64 x 64
		// tile of PG planes over one trajectory chunk; each wave a 32 x 32 sub-tile in 2 x 2 fragments per plane.  A k block is 16 trajectories:
		// the 256 threads form its 16 x 64 values of g_x and of g_p (one division and one exp each, shared by the PG planes) into the LDS buffer
		// the MFMAs do not read, so a block costs one barrier.  Lines beyond the grid are computed (finite, or 0) and never stored
		template <int PG>
		__global__ void __launch_bounds__(256, 2) hop_smooth_kernel(const HopSmoothArgs g)
		{
			__shared__ double Gx[2][SMK * SML], Gp[2][SMK * SML], U[2][PG * SMK];
			const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
			const long a0 = static_cast<long>(blockIdx.x / g.tiles_p) * SMT, b0 = static_cast<long>(blockIdx.x % g.tiles_p) * SMT;
			const long c = blockIdx.y;
			const int q0 = blockIdx.z * PG;
			const long i_first = c * g.chunk, i_last = i_first + g.chunk < g.npad ? i_first + g.chunk : g.npad;
			const int nkb = static_cast<int>((i_last - i_first) / SMK);

			double xk, pj;
			{
#pragma clang fp contract(off)
				xk = g.x_first + g.dx * static_cast<double>(a0 + lane);
				pj = g.p_first + g.dp * static_cast<double>(b0 + lane);
			}
			auto generate = [&](int kb, int buf) {
#pragma clang fp contract(off)
				const long i0 = i_first + static_cast<long>(kb) * SMK;
				double xi[4], pi[4];
#pragma unroll
				for (int r = 0; r < 4; ++r) xi[r] = g.xs[i0 + w + 4 * r], pi[r] = g.ps[i0 + w + 4 * r];
				double uv = 0.0;
				if (t < PG * SMK) uv = g.u[(q0 + t / SMK) * g.npad + i0 + t % SMK];
#pragma unroll
				for (int r = 0; r < 4; ++r)
				{
					const double tx = (xk - xi[r]) / g.h_x, tp = (pj - pi[r]) / g.h_p;
					Gx[buf][(w + 4 * r) * SML + lane] = exp(-0.5 * tx * tx);
					Gp[buf][(w + 4 * r) * SML + lane] = exp(-0.5 * tp * tp);
				}
				if (t < PG * SMK) U[buf][t] = uv;
			};

			sm4 acc[PG][2][2];
#pragma unroll
			for (int q = 0; q < PG; ++q)
#pragma unroll
				for (int i = 0; i < 2; ++i)
#pragma unroll
					for (int j = 0; j < 2; ++j) acc[q][i][j] = (sm4){0.0, 0.0, 0.0, 0.0};

			const int fk = lane >> 4, fr = lane & 15;
			if (nkb > 0) generate(0, 0);
			__syncthreads();
			for (int kb = 0; kb < nkb; ++kb)
			{
				const int buf = kb & 1;
				if (kb + 1 < nkb) generate(kb + 1, buf ^ 1);
#pragma unroll
				for (int kk = 0; kk < SMK; kk += 4)
				{
					const int kl = kk + fk;
					double gx[2], gp[2];
#pragma unroll
					for (int i = 0; i < 2; ++i) gx[i] = Gx[buf][kl * SML + wm * 32 + i * 16 + fr];
#pragma unroll
					for (int j = 0; j < 2; ++j) gp[j] = Gp[buf][kl * SML + wn * 32 + j * 16 + fr];
#pragma unroll
					for (int q = 0; q < PG; ++q)
					{
						const double uq = U[buf][q * SMK + kl];
#pragma unroll
						for (int i = 0; i < 2; ++i)
						{
							const double a = uq * gx[i];
#pragma unroll
							for (int j = 0; j < 2; ++j) acc[q][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, gp[j], acc[q][i][j], 0, 0, 0);
						}
					}
				}
				__syncthreads();
			}

			const long cells = g.n_x * g.n_p;
#pragma unroll
			for (int q = 0; q < PG; ++q)
			{
				double* __restrict__ out = g.partial + (c * g.planes + q0 + q) * cells;
#pragma unroll
				for (int i = 0; i < 2; ++i)
#pragma unroll
					for (int j = 0; j < 2; ++j)
#pragma unroll
						for (int r = 0; r < 4; ++r)
						{
							const long a = a0 + wm * 32 + i * 16 + fk + 4 * r, b = b0 + wn * 32 + j * 16 + fr;
							if (a < g.n_x && b < g.n_p) out[a * g.n_p + b] = acc[q][i][j][r];
						}
			}
		}

		// One thread per cell: the chunks' partial sums added in ascending order, times s, in the phase.txt layout.  Im rho_aa is +0, and a
		// lower plane is formed from the negated sum (exactly the conjugate, and +0 where the sum is 0)
		template <int NP>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_smooth_finish_kernel(long cells, long n_chunks, double s, const double* __restrict__ partial,
			double* __restrict__ rho)
		{
			const long cell = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (cell >= cells) return;
			double sum[NP * NP];
#pragma unroll
			for (int q = 0; q < NP * NP; ++q) sum[q] = partial[q * cells + cell];
			for (long c = 1; c < n_chunks; ++c)
#pragma unroll
				for (int q = 0; q < NP * NP; ++q) sum[q] += partial[(c * NP * NP + q) * cells + cell];
#pragma unroll
			for (int a = 0; a < NP; ++a)
			{
				double* d = rho + 2 * ((a * NP + a) * cells + cell);
				d[0] = s * sum[a], d[1] = 0.0;
			}
			int q = NP;
#pragma unroll
			for (int a = 0; a < NP; ++a)
#pragma unroll
				for (int b = a + 1; b < NP; ++b)
				{
					double *up = rho + 2 * ((a * NP + b) * cells + cell), *lo = rho + 2 * ((b * NP + a) * cells + cell);
					up[0] = lo[0] = s * sum[q];
					up[1] = s * sum[q + 1], lo[1] = s * (0.0 - sum[q + 1]);
					q += 2;
				}
		}
	} // namespace

	// The split of the trajectory index: a function of (num_pes, n, n_x, n_p) alone, so that two calls add the same partial sums in the same order
	HopSmoothPlan hop_smooth_plan(int num_pes, long n, long n_x, long n_p)
	{
		HopSmoothPlan plan{};
		const long planes = static_cast<long>(num_pes) * num_pes, cells = n_x * n_p;
		plan.groups = static_cast<int>(planes / hop_smooth_group(num_pes));
		plan.tiles_x = (n_x + SMT - 1) / SMT, plan.tiles_p = (n_p + SMT - 1) / SMT;
		const long tiles = plan.tiles_x * plan.tiles_p * plan.groups;
		const long most = std::max(1L, std::min(SM_WORKGROUPS / tiles, SM_PARTIAL_DOUBLES / (planes * cells)));
		const long even = ((n + most - 1) / most + SMK - 1) / SMK * SMK;
		plan.chunk = std::max(SM_MIN_CHUNK, even);
		plan.n_chunks = (n + plan.chunk - 1) / plan.chunk;
		plan.npad = (n + SMK - 1) / SMK * SMK;
		return plan;
	}
	size_t hop_smooth_work_doubles(int num_pes, long n, long n_x, long n_p)
	{
		const HopSmoothPlan plan = hop_smooth_plan(num_pes, n, n_x, n_p);
		const size_t planes = static_cast<size_t>(num_pes) * num_pes;
		return (2 + planes) * static_cast<size_t>(plan.npad) + static_cast<size_t>(plan.n_chunks) * planes * static_cast<size_t>(n_x) * static_cast<size_t>(n_p);
	}
	hipError_t launch_hop_smooth_terms(hipStream_t s, const HopEnsemble& e, PesModel model, bool mean_field, bool bin_all, double* work, unsigned long long* tally)
	{
		if (e.n <= 0) return hipErrorInvalidValue;
		const long npad = (e.n + SMK - 1) / SMK * SMK;
		double *xs = work, *ps = work + npad, *u = work + 2 * npad;
		const int all = bin_all ? 1 : 0;
		return hop_dispatch(e, model, [&](auto np, auto m) {
			if (mean_field) hop_launch(s, npad, hop_smooth_terms_kernel<np(), decltype(m), true>, e, m, all, npad, xs, ps, u, tally);
			else hop_launch(s, npad, hop_smooth_terms_kernel<np(), decltype(m), false>, e, m, all, npad, xs, ps, u, tally);
		});
	}
	hipError_t launch_hop_smooth(hipStream_t s, int num_pes, long n, const HopGrid& g, double h_x, double h_p, double scale, double* work, double* rho)
	{
		if ((num_pes != 2 && num_pes != 3) || n <= 0 || g.n_x <= 0 || g.n_p <= 0) return hipErrorInvalidValue;
		const HopSmoothPlan plan = hop_smooth_plan(num_pes, n, g.n_x, g.n_p);
		const int planes = num_pes * num_pes;
		double* const partial = work + (2 + planes) * plan.npad;
		const HopSmoothArgs a{work, work + plan.npad, work + 2 * plan.npad, partial, g.x_first, g.dx, g.p_first, g.dp, h_x, h_p, g.n_x, g.n_p, plan.npad, plan.chunk,
			static_cast<int>(plan.tiles_p), planes};
		const dim3 grid(static_cast<unsigned>(plan.tiles_x * plan.tiles_p), static_cast<unsigned>(plan.n_chunks), static_cast<unsigned>(plan.groups));
		const long cells = g.n_x * g.n_p;
		if (num_pes == 2)
		{
			hipLaunchKernelGGL(hop_smooth_kernel<hop_smooth_group(2)>, grid, dim3(256), 0, s, a);
			hop_launch(s, cells, hop_smooth_finish_kernel<2>, cells, plan.n_chunks, scale, partial, rho);
		}
		else
		{
			hipLaunchKernelGGL(hop_smooth_kernel<hop_smooth_group(3)>, grid, dim3(256), 0, s, a);
			hop_launch(s, cells, hop_smooth_finish_kernel<3>, cells, plan.n_chunks, scale, partial, rho);
		}
		return hipGetLastError();
	}
} // namespace gple
