// gple_hop.hip — fewest-switches surface hopping (Tully, J. Chem. Phys. 93, 1061 (1990)) for an ensemble of independent trajectories on the
// N-level potentials of gple_pes_n.h, built-in or tabulated (numpy restatement: tests/hop_numpy.py).  The reference has no
// trajectory code: this is the method its three models were made to test.
//
// One thread per trajectory; x, p, the diabatic amplitudes b, the active surface a and everything derived from them stay in registers for all
// the steps of a launch.  No LDS, no device globals, and no atomics but the integer ones of hop_bin_kernel below.  One step of length dt for a running trajectory (V, Fd = -V', E, C: the
// diabatic matrix and force, the adiabatic energies and states; F = C^T Fd C, symmetrised as in gple_evolve_n.hip):
//     1  p += F_aa(x) dt / 2,  x_new = x + p / m dt
//     2  b <- W exp(-i lambda dt / hbar) W^T b,  (lambda, W) the Jacobi eigen-system of (V(x) + V(x_new)) / 2: exactly unitary, no coupling needed
//     3  E, C, F at x_new,  p += F_aa(x_new) dt / 2
//     4  c = C^T b;  g_k = max(0, 2 dt (p / m) d_ak Re(conj(c_a) c_k) / |c_a|^2),  d_ak = F_ak / (E_a - E_k)  (0 where F_ak is exactly 0, or |c_a|^2 is)
//     5  xi = unit53 of the words (0, 1) of Philox4x32-10, counter (trajectory, step low, 0, step high), key (seed low, seed high);
//        hop to the first k != a (ascending) with xi < g_1 + ... + g_k
//     6  r = p^2 + 2 m (E_a - E_k):  r >= 0: p = sgn(p) sqrt(r), a = k;  r < 0: frustrated, nothing changes (reverse: p = -p)
//     6a (the instantiations with DC only; DESIGN.md §17, "Decoherence corrections") with a and p as step 6 left them, where |c_a|^2 != 0:
//        EDC: w = 1 if edc_c == 0 else Ekin / (Ekin + edc_c), Ekin = p^2 / 2 m;  k != a: f_k = exp(-dt |E_k - E_a| w / hbar), c_k <- f_k c_k;
//             c_a <- c_a sqrt(1 + sum_{k != a} |c_k|^2 (1 - f_k^2) / |c_a|^2)  (the old c_k: the norm the vector has is kept, no cancellation)
//        COLLAPSE_HOP after a hop taken, COLLAPSE_ATTEMPT after every hop wanted: c_a <- c_a / |c_a|, every other c_k <- 0
//        then b <- C c (the phase of c_a kept: invariant under the flip of a column of C)
//     7  x < x_left: status 1, x > x_right: status 2; a finished trajectory is never touched again
// Everything is invariant under flipping a column of C, so the sign convention of the adiabatic states (which flips along x) needs no tracking.
// The states at x_new are the states at x of the next step: they are formed at one place of the loop only, so that a launch which starts at x
// forms them with the same instructions as the launch that arrived there (evolve(a) then evolve(b) = evolve(a + b), bit for bit).
// Grouped ensembles ("A curve in one launch"): trajectory i of n_groups n_per_group belongs to group i / n_per_group, which has
// a packet and a time step of its own.  The plain and the grouped kernels call the same device functions per trajectory (hop_sample_one,
// hop_evolve_one, hop_observe_terms), so the state of a group is, bit for bit, what the plain call gives for that slice.
//
// Ehrenfest (mean-field) trajectories ("Mean-field (Ehrenfest) trajectories"; numpy restatement: tests/hop_mf_numpy.py): the same
// ensemble without an active surface, a seed, a step counter or an offset.  A trajectory is x, p, b and its status, and moves on the force
// averaged over b, which in the diabatic representation needs no eigen-system of V(x):
//     f(x, b) = sum_i |b_i|^2 Fd_ii + 2 sum_{i<j} Fd_ij Re(conj(b_i) b_j)   (i ascending, then the pairs (i, j) ascending, i first)
// One step of length dt for a running trajectory:
//     1  p += f(x, b) dt / 2,  x_new = x + p / m dt
//     2  b <- W exp(-i lambda dt / hbar) W^T b,  (lambda, W) the Jacobi eigen-system of (V(x) + V(x_new)) / 2, entry by entry as step 2 above
//     3  p += f(x_new, b_new) dt / 2,  x = x_new
//     4  x < x_left: status 1, x > x_right: status 2; a finished trajectory is never read or written again
// Time-symmetric (second order) and unitary to rounding; nothing is random.  V and Fd at x_new are those at x of the next step and are formed
// at one place of the loop, by the same s = -1 pass, so evolve_mf(a) then evolve_mf(b) = evolve_mf(a + b), bit for bit.  The plain and the
// grouped kernels call hop_evolve_mf_one and hop_observe_mf_terms per trajectory.
//
// Symmetrical quasi-classical (SQC) trajectories ("Symmetrical quasi-classical trajectories"; numpy restatement:
// tests/hop_sqc_numpy.py): the Meyer-Miller-Stock-Thoss mapping Hamiltonian with the windows of Cotton and Miller.  b is not normalised:
// with c = C^T b, e_k = |c_k|^2 and the action n_k = e_k - gamma, H = p^2 / 2m + b^dagger V b - gamma tr V, and the force is
//     f(x, b) = [the mean-field running sum above] - gamma (Fd_00 + ... + Fd_{NP-1,NP-1})   (the trace left to right, the product, then the difference)
// The step is the mean-field step with this f: i db/dt = V b, no eigen-system of V(x), nothing random, the same s = -1 pass.  The sample draws
// x and p by the lines of hop_sample_one (counter (index, 0, 1, 0)) and, for level k, (u_k, v_k) = unit53 of the words (0, 1) and (2, 3) of the
// counter (index, k, 2, 0);  c_k = sqrt(e_k) (cospi(2 v_k) + i sinpi(2 v_k)), b = C(x) c, with occ = surface0 and F = NP
//     square   (window 0):  e_k = delta_{k,occ} + 2 gamma u_k
//     triangle (window 1):  t = (1 - u_occ)^(1/F) (sqrt, cbrt),  e_occ = 2 - t,  e_j = u_j t  (j != occ)
// The sums bin e into the final windows: a trajectory belongs to the first k ascending with
//     square:    1 <= e_k <= 1 + 2 gamma  and  e_j <= 2 gamma  for all j != k
//     triangle:  e_k >= 1  and  e_k + e_j <= 2  for all j != k
// else to none.  The plain and the grouped kernels call hop_sample_sqc_one, hop_evolve_sqc_one and hop_observe_sqc_terms per trajectory.
//
// MASH trajectories (Mannouch and Richardson, J. Chem. Phys. 158, 104111 (2023); DESIGN.md §17, "MASH trajectories"; numpy restatement:
// tests/hop_mash_numpy.py), two levels only: the layout of fewest switches (x, p, b, surface, status), but the active surface is a function of
// the amplitudes, side(c) = 1 if |c_1|^2 > |c_0|^2 else 0 with c = C^T b, and the step draws no random number.  The sample draws x and p by the
// lines of hop_sample_one (counter (index, 0, 1, 0)) and (w0, w1) = unit53 of the words (0, 1) and (2, 3) of the counter (index, 0, 3, 0):
//     s = sqrt(1 - w0)  (density 2 s on (0, 1]: the weight 2 |S_z| drawn, so that populations are counts of the active surface)
//     a = surface0, o = 1 - a:  c_a = sqrt((1 + s) / 2),  c_o = sqrt((1 - s) / 2) (cospi(2 w1) + i sinpi(2 w1)),  b = C(x) c
// One step of length dt for a running trajectory: steps 1 to 3 of the fewest-switches step, then
//     4  c = C^T b, side_new = side(c), at one place of the loop and in every pass (s = -1 too); side_old is the pass before's
//     5  side_new != side_old and side_new != a:  r = p^2 + 2 m (E_a - E_side_new);  r >= 0: p = sgn(p) sqrt(r), a = side_new (a hop);
//        r < 0: p = -p, a stays (a frustrated hop: always reflected).  A crossing back to side_new == a changes nothing
//     6  step 7 above
// side_old of a launch's first step is formed from the stored b and C(x) by the instructions that formed it at the end of the launch before:
// evolve_mash(a) then evolve_mash(b) = evolve_mash(a + b), bit for bit.  The plain and the grouped kernels call hop_sample_mash_one and
// hop_evolve_mash_one per trajectory; the sums are hop_observe_kernel's.
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

		// One trajectory of the sample.  ZERO (the grouped call): a sigma of exactly 0 leaves the centre exactly, by a select and not by 0 * rho
		template <int NP, typename M, bool ZERO>
		__device__ __forceinline__ void hop_sample_one(const HopEnsemble& e, const M& model, long i, double x0, double p0, double sigma_x, double sigma_p, int surface0)
		{
			const unsigned long long index = e.offset + static_cast<unsigned long long>(i);
			unsigned c[4] = {static_cast<unsigned>(index), 0u, 1u, 0u};
			philox4x32(c, static_cast<unsigned>(e.seed), static_cast<unsigned>(e.seed >> 32));
			const double u0 = unit53(c[0], c[1]), u1 = unit53(c[2], c[3]);
			const double rho = sqrt(-2.0 * log(1.0 - u0));
			double sn, cs;
			sincospi(2.0 * u1, &sn, &cs);
			double x = x0 + sigma_x * rho * cs, p = p0 + sigma_p * rho * sn;
			if constexpr (ZERO) x = sigma_x == 0.0 ? x0 : x, p = sigma_p == 0.0 ? p0 : p;
			double E[NP];
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			e.x[i] = x, e.p[i] = p, e.surface[i] = surface0, e.status[i] = 0;
			double* b = e.b + 2 * NP * i;
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				double row[NP];
#pragma unroll
				for (int r = 0; r < NP; ++r) row[r] = C.a[k][r];
				b[2 * k] = pick<NP>(row, surface0), b[2 * k + 1] = 0.0;
			}
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_sample_kernel(HopEnsemble e, M model, double x0, double p0, double sigma_x, double sigma_p, int surface0)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n) return;
			hop_sample_one<NP, M, false>(e, model, i, x0, p0, sigma_x, sigma_p, surface0);
		}
		// The grouped sample ("A curve in one launch"): trajectory i belongs to group i / n_per_group and draws from that group's row
		// (x0, p0, sigma_x, sigma_p) of packets
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
		// uniform over the launch; without DC neither mode nor edc_c is read, and the code is what it was before 6a existed
		template <int NP, typename M, bool COUNT, bool DC>
		__device__ __forceinline__ void hop_evolve_one(const HopEnsemble& e, const M& model, long i, double mass, double dt, unsigned long long first_step, long n_steps,
			double x_left, double x_right, int reverse, int* hops, int mode, double edc_c)
		{
			double x = e.x[i], p = e.p[i], bre[NP], bim[NP];
			int taken = 0, frustrated = 0;
			int a = e.surface[i], status = 0;
			double* const b = e.b + 2 * NP * i;
#pragma unroll
			for (int k = 0; k < NP; ++k) bre[k] = b[2 * k], bim[k] = b[2 * k + 1];
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
					// 2: the amplitudes through the mid-point matrix, U = W exp(-i lambda dt / hbar) W^T entry by entry
					Mat<NP> Vm, W;
					double lam[NP], cs[NP], sn[NP];
#pragma unroll
					for (int r = 0; r < NP; ++r)
#pragma unroll
						for (int q = 0; q < NP; ++q) Vm.a[r][q] = 0.5 * (Vx.a[r][q] + st.V.a[r][q]);
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
						if (changed)
#pragma unroll
							for (int r = 0; r < NP; ++r)
							{
								double re = 0.0, im = 0.0;
#pragma unroll
								for (int k = 0; k < NP; ++k) re += st.C.a[r][k] * cre[k], im += st.C.a[r][k] * cim[k];
								bre[r] = re, bim[r] = im;
							}
					}
					// 7
					if (x < x_left) status = 1;
					else if (x > x_right) status = 2;
				}
				Vx = st.V;
#pragma unroll
				for (int k = 0; k < NP; ++k) Fx[k] = st.F.a[k][k];
			}
			e.x[i] = x, e.p[i] = p, e.surface[i] = a, e.status[i] = status;
#pragma unroll
			for (int k = 0; k < NP; ++k) b[2 * k] = bre[k], b[2 * k + 1] = bim[k];
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

		// The 4 NP + 3 terms of trajectory i (include/gple.h, gple_hop_observe)
		template <int NP, typename M>
		__device__ __forceinline__ void hop_observe_terms(const HopEnsemble& e, const M& model, double mass, long i, double (&t)[4 * NP + 3])
		{
			const double x = e.x[i], p = e.p[i];
			const int a = e.surface[i], status = e.status[i];
			double bre[NP], bim[NP], cre[NP], cim[NP], E[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k) bre[k] = e.b[2 * (NP * i + k)], bim[k] = e.b[2 * (NP * i + k) + 1];
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			adiabatic_amplitudes<NP>(C, bre, bim, cre, cim);
			const int cell = status >= 0 && status <= 2 && a >= 0 && a < NP ? status * NP + a : -1;
#pragma unroll
			for (int q = 0; q < 3 * NP; ++q) t[q] = q == cell ? 1.0 : 0.0;
#pragma unroll
			for (int k = 0; k < NP; ++k) t[3 * NP + k] = cre[k] * cre[k] + cim[k] * cim[k];
			t[4 * NP] = x, t[4 * NP + 1] = p, t[4 * NP + 2] = p * p / 2.0 / mass + pick<NP>(E, a);
		}
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

		// First stage of the sums: the 4 NP + 3 terms of every trajectory, added over each wave (lanes beyond n hold zeros), one row of partial per wave
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_kernel(HopEnsemble e, M model, double mass, double* __restrict__ partial)
		{
			constexpr int WIDTH = 4 * NP + 3;
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			double t[WIDTH];
#pragma unroll
			for (int q = 0; q < WIDTH; ++q) t[q] = 0.0;
			if (i < e.n) hop_observe_terms<NP>(e, model, mass, i, t);
			hop_wave_sums<WIDTH>(t, partial + (i / HOP_WAVE) * WIDTH);
		}
		// Second stage, one wave per column
		__global__ void __launch_bounds__(HOP_WAVE) hop_observe_finish_kernel(const double* __restrict__ partial, long rows, int width, double* __restrict__ out)
		{
			const double v = hop_column_sum(partial, rows, width, blockIdx.x, threadIdx.x);
			if (threadIdx.x == 0) out[blockIdx.x] = v;
		}
		// The grouped sums: every group has blocks_per_group workgroups of its own, so its trajectory j sits in the wave and lane it has in a plain
		// launch over the group alone, and its rows_per_group = 4 blocks_per_group partial rows are the rows of that launch: the same tree, the same bits
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_groups_kernel(HopEnsemble e, M model, long n_per_group, unsigned blocks_per_group, double mass,
			double* __restrict__ partial)
		{
			constexpr int WIDTH = 4 * NP + 3;
			const long group = blockIdx.x / blocks_per_group;
			const long j = static_cast<long>(blockIdx.x % blocks_per_group) * HOP_BLOCK + threadIdx.x;
			double t[WIDTH];
#pragma unroll
			for (int q = 0; q < WIDTH; ++q) t[q] = 0.0;
			if (j < n_per_group) hop_observe_terms<NP>(e, model, mass, group * n_per_group + j, t);
			hop_wave_sums<WIDTH>(t, partial + (group * blocks_per_group * (HOP_BLOCK / HOP_WAVE) + j / HOP_WAVE) * WIDTH);
		}
		// one wave per group and column: block g width + q
		__global__ void __launch_bounds__(HOP_WAVE) hop_observe_finish_groups_kernel(const double* __restrict__ partial, long rows_per_group, int width, double* __restrict__ out)
		{
			const long group = blockIdx.x / width;
			const double v = hop_column_sum(partial + group * rows_per_group * width, rows_per_group, width, blockIdx.x % width, threadIdx.x);
			if (threadIdx.x == 0) out[blockIdx.x] = v;
		}

		// ---- Ehrenfest (mean-field) trajectories: the step and the sums stated at the head of this file ------------------------------------------
		// f(x, b) = b^dagger Fd b, one running sum: the diagonal terms with i ascending, then 2 Fd_ij Re(conj(b_i) b_j) over the pairs i < j ascending
		template <int NP>
		__device__ __forceinline__ double mean_field_force(const Mat<NP>& Fd, const double (&bre)[NP], const double (&bim)[NP])
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
		// All the steps of a launch for the running trajectory i.  Step 2 is hop_evolve_one's, line for line: a copy, so that the kernels above
		// keep the code they had
		template <int NP, typename M>
		__device__ __forceinline__ void hop_evolve_mf_one(const HopEnsemble& e, const M& model, long i, double mass, double dt, long n_steps, double x_left, double x_right)
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
					p += mean_field_force<NP>(Fx, bre, bim) * dt / 2.0;
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
					p += mean_field_force<NP>(Fn, bre, bim) * dt / 2.0;
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
			hop_evolve_mf_one<NP, M>(e, model, i, mass, dt, n_steps, x_left, x_right);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_groups_mf_kernel(HopEnsemble e, M model, long n_per_group, double mass, const double* __restrict__ dt,
			long n_steps, double x_left, double x_right)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_mf_one<NP, M>(e, model, i, mass, dt[i / n_per_group], n_steps, x_left, x_right);
		}

		// The 3 NP + 6 terms of trajectory i (include/gple.h, gple_hop_observe_mf): there is no active surface, so a channel is weighted by
		// |c_k|^2, c = C^T b at the trajectory's x as hop_observe_terms forms it.  A status out of range adds to no weight and to no count
		template <int NP, typename M>
		__device__ __forceinline__ void hop_observe_mf_terms(const HopEnsemble& e, const M& model, double mass, long i, double (&t)[3 * NP + 6])
		{
			const double x = e.x[i], p = e.p[i];
			const int status = e.status[i];
			double bre[NP], bim[NP], cre[NP], cim[NP], E[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k) bre[k] = e.b[2 * (NP * i + k)], bim[k] = e.b[2 * (NP * i + k) + 1];
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			adiabatic_amplitudes<NP>(C, bre, bim, cre, cim);
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
		// the two first stages of the sums with these terms: the launch shapes and the tree of hop_observe_kernel and hop_observe_groups_kernel
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_mf_kernel(HopEnsemble e, M model, double mass, double* __restrict__ partial)
		{
			constexpr int WIDTH = 3 * NP + 6;
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			double t[WIDTH];
#pragma unroll
			for (int q = 0; q < WIDTH; ++q) t[q] = 0.0;
			if (i < e.n) hop_observe_mf_terms<NP>(e, model, mass, i, t);
			hop_wave_sums<WIDTH>(t, partial + (i / HOP_WAVE) * WIDTH);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_groups_mf_kernel(HopEnsemble e, M model, long n_per_group, unsigned blocks_per_group, double mass,
			double* __restrict__ partial)
		{
			constexpr int WIDTH = 3 * NP + 6;
			const long group = blockIdx.x / blocks_per_group;
			const long j = static_cast<long>(blockIdx.x % blocks_per_group) * HOP_BLOCK + threadIdx.x;
			double t[WIDTH];
#pragma unroll
			for (int q = 0; q < WIDTH; ++q) t[q] = 0.0;
			if (j < n_per_group) hop_observe_mf_terms<NP>(e, model, mass, group * n_per_group + j, t);
			hop_wave_sums<WIDTH>(t, partial + (group * blocks_per_group * (HOP_BLOCK / HOP_WAVE) + j / HOP_WAVE) * WIDTH);
		}

		// ---- Symmetrical quasi-classical trajectories: the sample, the step and the sums stated at the head of this file ------------------------------
		// One trajectory of the sample.  x and p by hop_sample_one's lines (the same bits); then the energies e on the start window and the angles
		template <int NP, typename M, bool ZERO>
		__device__ __forceinline__ void hop_sample_sqc_one(const HopEnsemble& e, const M& model, long i, double x0, double p0, double sigma_x, double sigma_p, int surface0,
			int window, double gamma)
		{
			const unsigned long long index = e.offset + static_cast<unsigned long long>(i);
			const unsigned key0 = static_cast<unsigned>(e.seed), key1 = static_cast<unsigned>(e.seed >> 32);
			unsigned c[4] = {static_cast<unsigned>(index), 0u, 1u, 0u};
			philox4x32(c, key0, key1);
			const double u0 = unit53(c[0], c[1]), u1 = unit53(c[2], c[3]);
			const double rho = sqrt(-2.0 * log(1.0 - u0));
			double sn, cs;
			sincospi(2.0 * u1, &sn, &cs);
			double x = x0 + sigma_x * rho * cs, p = p0 + sigma_p * rho * sn;
			if constexpr (ZERO) x = sigma_x == 0.0 ? x0 : x, p = sigma_p == 0.0 ? p0 : p;
			double E[NP];
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
			double cre[NP], cim[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k)
			{
				const bool occupied = k == surface0;
				const double square = (occupied ? 1.0 : 0.0) + 2.0 * gamma * u[k], triangle = occupied ? 2.0 - t : u[k] * t;
				const double length = sqrt(window == GPLE_HOP_WINDOW_SQUARE ? square : triangle);
				sincospi(2.0 * v[k], &sn, &cs);
				cre[k] = length * cs, cim[k] = length * sn;
			}
			e.x[i] = x, e.p[i] = p, e.surface[i] = surface0, e.status[i] = 0;
			double* b = e.b + 2 * NP * i;
#pragma unroll
			for (int r = 0; r < NP; ++r)
			{
				double re = 0.0, im = 0.0;
#pragma unroll
				for (int k = 0; k < NP; ++k) re += C.a[r][k] * cre[k], im += C.a[r][k] * cim[k];
				b[2 * r] = re, b[2 * r + 1] = im;
			}
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

		// f(x, b) = b^dagger Fd b - gamma tr Fd: the mean-field running sum, the trace left to right, the product, then the difference
		template <int NP>
		__device__ __forceinline__ double sqc_force(const Mat<NP>& Fd, const double (&bre)[NP], const double (&bim)[NP], double gamma)
		{
			double trace = Fd.a[0][0];
#pragma unroll
			for (int i = 1; i < NP; ++i) trace += Fd.a[i][i];
			return mean_field_force<NP>(Fd, bre, bim) - gamma * trace;
		}
		// All the steps of a launch for the running trajectory i: hop_evolve_mf_one's lines with sqc_force (a copy, so that the kernels above keep
		// the code they had)
		template <int NP, typename M>
		__device__ __forceinline__ void hop_evolve_sqc_one(const HopEnsemble& e, const M& model, long i, double mass, double dt, long n_steps, double x_left, double x_right,
			double gamma)
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
					p += sqc_force<NP>(Fx, bre, bim, gamma) * dt / 2.0;
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
					p += sqc_force<NP>(Fn, bre, bim, gamma) * dt / 2.0;
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
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_sqc_kernel(HopEnsemble e, M model, double mass, double dt, long n_steps, double x_left, double x_right,
			double gamma)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_sqc_one<NP, M>(e, model, i, mass, dt, n_steps, x_left, x_right, gamma);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_evolve_groups_sqc_kernel(HopEnsemble e, M model, long n_per_group, double mass, const double* __restrict__ dt,
			long n_steps, double x_left, double x_right, double gamma)
		{
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (i >= e.n || e.status[i] != 0) return;
			hop_evolve_sqc_one<NP, M>(e, model, i, mass, dt[i / n_per_group], n_steps, x_left, x_right, gamma);
		}

		// The 4 NP + 9 terms of trajectory i (include/gple.h, gple_hop_observe_sqc): c = C^T b at the trajectory's x as hop_observe_terms forms
		// it, e_k = |c_k|^2, and the first window (k ascending) that holds e, else none.  A status out of range adds nowhere
		template <int NP, typename M>
		__device__ __forceinline__ void hop_observe_sqc_terms(const HopEnsemble& e, const M& model, double mass, int window, double gamma, long i, double (&t)[4 * NP + 9])
		{
			const double x = e.x[i], p = e.p[i];
			const int status = e.status[i];
			double bre[NP], bim[NP], cre[NP], cim[NP], E[NP], w[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k) bre[k] = e.b[2 * (NP * i + k)], bim[k] = e.b[2 * (NP * i + k) + 1];
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			adiabatic_amplitudes<NP>(C, bre, bim, cre, cim);
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
		// the two first stages of the sums with these terms: the launch shapes and the tree of hop_observe_kernel and hop_observe_groups_kernel
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_sqc_kernel(HopEnsemble e, M model, double mass, int window, double gamma, double* __restrict__ partial)
		{
			constexpr int WIDTH = 4 * NP + 9;
			const long i = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			double t[WIDTH];
#pragma unroll
			for (int q = 0; q < WIDTH; ++q) t[q] = 0.0;
			if (i < e.n) hop_observe_sqc_terms<NP>(e, model, mass, window, gamma, i, t);
			hop_wave_sums<WIDTH>(t, partial + (i / HOP_WAVE) * WIDTH);
		}
		template <int NP, typename M>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_observe_groups_sqc_kernel(HopEnsemble e, M model, long n_per_group, unsigned blocks_per_group, double mass, int window,
			double gamma, double* __restrict__ partial)
		{
			constexpr int WIDTH = 4 * NP + 9;
			const long group = blockIdx.x / blocks_per_group;
			const long j = static_cast<long>(blockIdx.x % blocks_per_group) * HOP_BLOCK + threadIdx.x;
			double t[WIDTH];
#pragma unroll
			for (int q = 0; q < WIDTH; ++q) t[q] = 0.0;
			if (j < n_per_group) hop_observe_sqc_terms<NP>(e, model, mass, window, gamma, group * n_per_group + j, t);
			hop_wave_sums<WIDTH>(t, partial + (group * blocks_per_group * (HOP_BLOCK / HOP_WAVE) + j / HOP_WAVE) * WIDTH);
		}

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
						double bre[NP], bim[NP], cre[NP], cim[NP], E[NP];
#pragma unroll
						for (int k = 0; k < NP; ++k) bre[k] = e.b[2 * (NP * i + k)], bim[k] = e.b[2 * (NP * i + k) + 1];
						Mat<NP> C, Fd;
						adiabatic_states_n<NP>(x, model, E, C, Fd);
						adiabatic_amplitudes<NP>(C, bre, bim, cre, cim);
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
		// One thread per cell: the num_pes^2 planes of the phase.txt layout from the integers.  The lower triangle is formed from the negated
		// sum (exactly the conjugate, and +0 where the sum is 0)
		template <int NP>
		__global__ void __launch_bounds__(HOP_BLOCK) hop_density_kernel(long cells, double w, const long long* __restrict__ acc, double* __restrict__ rho)
		{
			const long cell = static_cast<long>(blockIdx.x) * HOP_BLOCK + threadIdx.x;
			if (cell >= cells) return;
			constexpr double SCALE = 1.0 / 4294967296.0;
#pragma unroll
			for (int a = 0; a < NP; ++a)
			{
				double* d = rho + 2 * ((a * NP + a) * cells + cell);
				d[0] = static_cast<double>(acc[a * cells + cell]) / w, d[1] = 0.0;
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

		// ---- MASH trajectories: the sample and the step stated at the head of this file -----------------------------------------------------------
		// side(c): the adiabatic state with the larger population, 1 if |c_1|^2 > |c_0|^2 else 0 (the sign of the mapping spin's S_z)
		__device__ __forceinline__ int mash_side(const double (&cre)[2], const double (&cim)[2])
		{
			return cre[1] * cre[1] + cim[1] * cim[1] > cre[0] * cre[0] + cim[0] * cim[0] ? 1 : 0;
		}
		// One trajectory of the sample.  x and p by hop_sample_one's lines (the same bits); then s = |S_z| with the density 2 s and the angle of
		// the other amplitude from the counter (index, 0, 3, 0)
		template <int NP, typename M, bool ZERO>
		__device__ __forceinline__ void hop_sample_mash_one(const HopEnsemble& e, const M& model, long i, double x0, double p0, double sigma_x, double sigma_p, int surface0)
		{
			static_assert(NP == 2, "MASH is a two-level method");
			const unsigned long long index = e.offset + static_cast<unsigned long long>(i);
			const unsigned key0 = static_cast<unsigned>(e.seed), key1 = static_cast<unsigned>(e.seed >> 32);
			unsigned c[4] = {static_cast<unsigned>(index), 0u, 1u, 0u};
			philox4x32(c, key0, key1);
			const double u0 = unit53(c[0], c[1]), u1 = unit53(c[2], c[3]);
			const double rho = sqrt(-2.0 * log(1.0 - u0));
			double sn, cs;
			sincospi(2.0 * u1, &sn, &cs);
			double x = x0 + sigma_x * rho * cs, p = p0 + sigma_p * rho * sn;
			if constexpr (ZERO) x = sigma_x == 0.0 ? x0 : x, p = sigma_p == 0.0 ? p0 : p;
			double E[NP];
			Mat<NP> C, Fd;
			adiabatic_states_n<NP>(x, model, E, C, Fd);
			unsigned w[4] = {static_cast<unsigned>(index), 0u, 3u, 0u};
			philox4x32(w, key0, key1);
			const double w0 = unit53(w[0], w[1]), w1 = unit53(w[2], w[3]);
			const double s = sqrt(1.0 - w0), active = sqrt((1.0 + s) / 2.0), other = sqrt((1.0 - s) / 2.0);
			sincospi(2.0 * w1, &sn, &cs);
			double cre[NP], cim[NP];
#pragma unroll
			for (int k = 0; k < NP; ++k) cre[k] = k == surface0 ? active : other * cs, cim[k] = k == surface0 ? 0.0 : other * sn;
			e.x[i] = x, e.p[i] = p, e.surface[i] = surface0, e.status[i] = 0;
			double* b = e.b + 2 * NP * i;
#pragma unroll
			for (int r = 0; r < NP; ++r)
			{
				double re = 0.0, im = 0.0;
#pragma unroll
				for (int k = 0; k < NP; ++k) re += C.a[r][k] * cre[k], im += C.a[r][k] * cim[k];
				b[2 * r] = re, b[2 * r + 1] = im;
			}
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

		// All the steps of a launch for the running trajectory i.  Steps 1 to 3 and 7 are hop_evolve_one's, line for line: a copy, so that the
		// kernels above keep the code they had.  COUNT (the grouped call): the two outcomes of a crossing are counted in registers and added to
		// hops[2 i], hops[2 i + 1] at the end, where hops is not null
		template <int NP, typename M, bool COUNT>
		__device__ __forceinline__ void hop_evolve_mash_one(const HopEnsemble& e, const M& model, long i, double mass, double dt, long n_steps, double x_left, double x_right,
			int* hops)
		{
			static_assert(NP == 2, "MASH is a two-level method");
			double x = e.x[i], p = e.p[i], bre[NP], bim[NP];
			int taken = 0, frustrated = 0;
			int a = e.surface[i], status = 0, side = 0;
			double* const b = e.b + 2 * NP * i;
#pragma unroll
			for (int k = 0; k < NP; ++k) bre[k] = b[2 * k], bim[k] = b[2 * k + 1];
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
					// 2: the amplitudes through the mid-point matrix, U = W exp(-i lambda dt / hbar) W^T entry by entry
					Mat<NP> Vm, W;
					double lam[NP], cs[NP], sn[NP];
#pragma unroll
					for (int r = 0; r < NP; ++r)
#pragma unroll
						for (int q = 0; q < NP; ++q) Vm.a[r][q] = 0.5 * (Vx.a[r][q] + st.V.a[r][q]);
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
					double Fdiag[NP];
#pragma unroll
					for (int k = 0; k < NP; ++k) Fdiag[k] = st.F.a[k][k];
					p += pick<NP>(Fdiag, a) * dt / 2.0;
					x = xn;
				}
				// the side of the amplitudes at this point, in every pass: the start of a launch forms it as the end of the launch before did
				double cre[NP], cim[NP];
				adiabatic_amplitudes<NP>(st.C, bre, bim, cre, cim);
				const int side_new = mash_side(cre, cim);
				if (s >= 0)
				{
					// the crossing: the amplitudes changed side, away from the active surface
					if (side_new != side && side_new != a)
					{
						const double r = p * p + 2.0 * mass * (pick<NP>(st.E, a) - pick<NP>(st.E, side_new));
						if (r >= 0.0) p = sgn_n(p) * sqrt(r), a = side_new;
						else p = -p;
						if constexpr (COUNT) taken += r >= 0.0 ? 1 : 0, frustrated += r >= 0.0 ? 0 : 1;
					}
					// 7
					if (x < x_left) status = 1;
					else if (x > x_right) status = 2;
				}
				side = side_new;
				Vx = st.V;
#pragma unroll
				for (int k = 0; k < NP; ++k) Fx[k] = st.F.a[k][k];
			}
			e.x[i] = x, e.p[i] = p, e.surface[i] = a, e.status[i] = status;
#pragma unroll
			for (int k = 0; k < NP; ++k) b[2 * k] = bre[k], b[2 * k + 1] = bim[k];
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

		inline unsigned hop_blocks(long n) { return static_cast<unsigned>((n + HOP_BLOCK - 1) / HOP_BLOCK); }
	} // namespace

	hipError_t launch_hop_sample_mash(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0)
	{
		if (e.num_pes != 2) return hipErrorInvalidValue;
		if (e.n <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_sample_mash_kernel<2, decltype(m)>), grid, block, 0, s, e, m, x0, p0, sigma_x, sigma_p, surface0); });
		return hipGetLastError();
	}
	hipError_t launch_hop_sample_groups_mash(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0)
	{
		if (e.num_pes != 2 || e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_sample_groups_mash_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, packets, surface0); });
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_mash(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right)
	{
		if (e.num_pes != 2) return hipErrorInvalidValue;
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_evolve_mash_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, dt, n_steps, x_left, x_right); });
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_groups_mash(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right, int* hops)
	{
		if (e.num_pes != 2 || e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		with_model(model, [&](auto m) {
			hipLaunchKernelGGL((hop_evolve_groups_mash_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, n_steps, x_left, x_right, hops);
		});
		return hipGetLastError();
	}

	hipError_t launch_hop_sample(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0)
	{
		if (e.n <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_sample_kernel<2, decltype(m)>), grid, block, 0, s, e, m, x0, p0, sigma_x, sigma_p, surface0); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_sample_kernel<3, decltype(m)>), grid, block, 0, s, e, m, x0, p0, sigma_x, sigma_p, surface0); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, unsigned long long first_step, long n_steps,
		double x_left, double x_right, bool reverse)
	{
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		const int rev = reverse ? 1 : 0;
		if (e.num_pes == 2)
			with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_evolve_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, dt, first_step, n_steps, x_left, x_right, rev); });
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_evolve_kernel<3, decltype(m)>), grid, block, 0, s, e, m, mass, dt, first_step, n_steps, x_left, x_right, rev); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_sample_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_sample_groups_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, packets, surface0); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_sample_groups_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, packets, surface0); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, unsigned long long first_step,
		long n_steps, double x_left, double x_right, bool reverse, int* hops)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		const int rev = reverse ? 1 : 0;
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, first_step, n_steps, x_left, x_right, rev, hops);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, first_step, n_steps, x_left, x_right, rev, hops);
			});
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_dc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, unsigned long long first_step, long n_steps,
		double x_left, double x_right, bool reverse, int decoherence, double edc_c)
	{
		if (decoherence == GPLE_HOP_DC_NONE) return launch_hop_evolve(s, e, model, mass, dt, first_step, n_steps, x_left, x_right, reverse);
		if (decoherence < GPLE_HOP_DC_NONE || decoherence > GPLE_HOP_DC_COLLAPSE_ATTEMPT) return hipErrorInvalidValue;
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		const int rev = reverse ? 1 : 0;
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_dc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, dt, first_step, n_steps, x_left, x_right, rev, decoherence, edc_c);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_dc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, mass, dt, first_step, n_steps, x_left, x_right, rev, decoherence, edc_c);
			});
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_groups_dc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt,
		unsigned long long first_step, long n_steps, double x_left, double x_right, bool reverse, int* hops, int decoherence, double edc_c)
	{
		if (decoherence == GPLE_HOP_DC_NONE) return launch_hop_evolve_groups(s, e, model, n_per_group, mass, dt, first_step, n_steps, x_left, x_right, reverse, hops);
		if (decoherence < GPLE_HOP_DC_NONE || decoherence > GPLE_HOP_DC_COLLAPSE_ATTEMPT) return hipErrorInvalidValue;
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		const int rev = reverse ? 1 : 0;
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_dc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, first_step, n_steps, x_left, x_right, rev,
					hops, decoherence, edc_c);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_dc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, first_step, n_steps, x_left, x_right, rev,
					hops, decoherence, edc_c);
			});
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	size_t hop_observe_groups_work_doubles(int num_pes, long n_groups, long n_per_group)
	{
		return static_cast<size_t>(n_groups) * hop_blocks(n_per_group) * (HOP_BLOCK / HOP_WAVE) * (4 * num_pes + 3);
	}
	hipError_t launch_hop_observe_groups(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, double* work, double* out)
	{
		if (n_groups <= 0 || n_per_group <= 0 || e.n != n_groups * n_per_group) return hipErrorInvalidValue;
		const unsigned per_group = hop_blocks(n_per_group);
		if (static_cast<unsigned long long>(n_groups) * per_group > 0x7FFFFFFFull) return hipErrorInvalidValue;
		const dim3 grid(static_cast<unsigned>(n_groups * per_group)), block(HOP_BLOCK);
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_groups_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, per_group, mass, work); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_groups_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, per_group, mass, work); });
		else return hipErrorInvalidValue;
		hipError_t err = hipGetLastError();
		if (err != hipSuccess) return err;
		const int width = 4 * e.num_pes + 3;
		hipLaunchKernelGGL(hop_observe_finish_groups_kernel, dim3(static_cast<unsigned>(n_groups * width)), dim3(HOP_WAVE), 0, s, work,
			static_cast<long>(per_group) * (HOP_BLOCK / HOP_WAVE), width, out);
		return hipGetLastError();
	}
	size_t hop_observe_work_doubles(int num_pes, long n) { return static_cast<size_t>(hop_blocks(n)) * (HOP_BLOCK / HOP_WAVE) * (4 * num_pes + 3); }
	hipError_t launch_hop_observe(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double* work, double* out)
	{
		if (e.n <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, work); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_kernel<3, decltype(m)>), grid, block, 0, s, e, m, mass, work); });
		else return hipErrorInvalidValue;
		hipError_t err = hipGetLastError();
		if (err != hipSuccess) return err;
		const int width = 4 * e.num_pes + 3;
		hipLaunchKernelGGL(hop_observe_finish_kernel, dim3(width), dim3(HOP_WAVE), 0, s, work, static_cast<long>(grid.x) * (HOP_BLOCK / HOP_WAVE), width, out);
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right)
	{
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2)
			with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_evolve_mf_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, dt, n_steps, x_left, x_right); });
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_evolve_mf_kernel<3, decltype(m)>), grid, block, 0, s, e, m, mass, dt, n_steps, x_left, x_right); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_groups_mf(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_mf_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, n_steps, x_left, x_right);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_mf_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, n_steps, x_left, x_right);
			});
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	size_t hop_observe_mf_work_doubles(int num_pes, long n) { return static_cast<size_t>(hop_blocks(n)) * (HOP_BLOCK / HOP_WAVE) * (3 * num_pes + 6); }
	hipError_t launch_hop_observe_mf(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double* work, double* out)
	{
		if (e.n <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_mf_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, work); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_mf_kernel<3, decltype(m)>), grid, block, 0, s, e, m, mass, work); });
		else return hipErrorInvalidValue;
		hipError_t err = hipGetLastError();
		if (err != hipSuccess) return err;
		const int width = 3 * e.num_pes + 6;
		hipLaunchKernelGGL(hop_observe_finish_kernel, dim3(width), dim3(HOP_WAVE), 0, s, work, static_cast<long>(grid.x) * (HOP_BLOCK / HOP_WAVE), width, out);
		return hipGetLastError();
	}
	size_t hop_observe_groups_mf_work_doubles(int num_pes, long n_groups, long n_per_group)
	{
		return static_cast<size_t>(n_groups) * hop_blocks(n_per_group) * (HOP_BLOCK / HOP_WAVE) * (3 * num_pes + 6);
	}
	hipError_t launch_hop_observe_groups_mf(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, double* work, double* out)
	{
		if (n_groups <= 0 || n_per_group <= 0 || e.n != n_groups * n_per_group) return hipErrorInvalidValue;
		const unsigned per_group = hop_blocks(n_per_group);
		if (static_cast<unsigned long long>(n_groups) * per_group > 0x7FFFFFFFull) return hipErrorInvalidValue;
		const dim3 grid(static_cast<unsigned>(n_groups * per_group)), block(HOP_BLOCK);
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_groups_mf_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, per_group, mass, work); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_groups_mf_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, per_group, mass, work); });
		else return hipErrorInvalidValue;
		hipError_t err = hipGetLastError();
		if (err != hipSuccess) return err;
		const int width = 3 * e.num_pes + 6;
		hipLaunchKernelGGL(hop_observe_finish_groups_kernel, dim3(static_cast<unsigned>(n_groups * width)), dim3(HOP_WAVE), 0, s, work,
			static_cast<long>(per_group) * (HOP_BLOCK / HOP_WAVE), width, out);
		return hipGetLastError();
	}
	hipError_t launch_hop_sample_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double x0, double p0, double sigma_x, double sigma_p, int surface0, int window,
		double gamma)
	{
		if (e.n <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_sample_sqc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, x0, p0, sigma_x, sigma_p, surface0, window, gamma);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_sample_sqc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, x0, p0, sigma_x, sigma_p, surface0, window, gamma);
			});
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_sample_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, const double* packets, int surface0, int window,
		double gamma)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_sample_groups_sqc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, packets, surface0, window, gamma);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_sample_groups_sqc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, packets, surface0, window, gamma);
			});
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, double dt, long n_steps, double x_left, double x_right, double gamma)
	{
		if (e.n <= 0 || n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2)
			with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_evolve_sqc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, dt, n_steps, x_left, x_right, gamma); });
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_evolve_sqc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, mass, dt, n_steps, x_left, x_right, gamma); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_evolve_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_per_group, double mass, const double* dt, long n_steps,
		double x_left, double x_right, double gamma)
	{
		if (e.n <= 0 || n_per_group <= 0) return hipErrorInvalidValue;
		if (n_steps <= 0) return hipSuccess;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_sqc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, n_steps, x_left, x_right, gamma);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_evolve_groups_sqc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, mass, dt, n_steps, x_left, x_right, gamma);
			});
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	size_t hop_observe_sqc_work_doubles(int num_pes, long n) { return static_cast<size_t>(hop_blocks(n)) * (HOP_BLOCK / HOP_WAVE) * (4 * num_pes + 9); }
	hipError_t launch_hop_observe_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, double mass, int window, double gamma, double* work, double* out)
	{
		if (e.n <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_sqc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, mass, window, gamma, work); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_observe_sqc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, mass, window, gamma, work); });
		else return hipErrorInvalidValue;
		hipError_t err = hipGetLastError();
		if (err != hipSuccess) return err;
		const int width = 4 * e.num_pes + 9;
		hipLaunchKernelGGL(hop_observe_finish_kernel, dim3(width), dim3(HOP_WAVE), 0, s, work, static_cast<long>(grid.x) * (HOP_BLOCK / HOP_WAVE), width, out);
		return hipGetLastError();
	}
	size_t hop_observe_groups_sqc_work_doubles(int num_pes, long n_groups, long n_per_group)
	{
		return static_cast<size_t>(n_groups) * hop_blocks(n_per_group) * (HOP_BLOCK / HOP_WAVE) * (4 * num_pes + 9);
	}
	hipError_t launch_hop_observe_groups_sqc(hipStream_t s, const HopEnsemble& e, PesModel model, long n_groups, long n_per_group, double mass, int window, double gamma,
		double* work, double* out)
	{
		if (n_groups <= 0 || n_per_group <= 0 || e.n != n_groups * n_per_group) return hipErrorInvalidValue;
		const unsigned per_group = hop_blocks(n_per_group);
		if (static_cast<unsigned long long>(n_groups) * per_group > 0x7FFFFFFFull) return hipErrorInvalidValue;
		const dim3 grid(static_cast<unsigned>(n_groups * per_group)), block(HOP_BLOCK);
		if (e.num_pes == 2)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_observe_groups_sqc_kernel<2, decltype(m)>), grid, block, 0, s, e, m, n_per_group, per_group, mass, window, gamma, work);
			});
		else if (e.num_pes == 3)
			with_model(model, [&](auto m) {
				hipLaunchKernelGGL((hop_observe_groups_sqc_kernel<3, decltype(m)>), grid, block, 0, s, e, m, n_per_group, per_group, mass, window, gamma, work);
			});
		else return hipErrorInvalidValue;
		hipError_t err = hipGetLastError();
		if (err != hipSuccess) return err;
		const int width = 4 * e.num_pes + 9;
		hipLaunchKernelGGL(hop_observe_finish_groups_kernel, dim3(static_cast<unsigned>(n_groups * width)), dim3(HOP_WAVE), 0, s, work,
			static_cast<long>(per_group) * (HOP_BLOCK / HOP_WAVE), width, out);
		return hipGetLastError();
	}
	hipError_t launch_hop_bin(hipStream_t s, const HopEnsemble& e, PesModel model, const HopGrid& g, bool bin_all, long long* acc)
	{
		if (e.n <= 0 || g.n_x <= 0 || g.n_p <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(e.n)), block(HOP_BLOCK);
		unsigned long long* const words = reinterpret_cast<unsigned long long*>(acc);
		const int all = bin_all ? 1 : 0;
		if (e.num_pes == 2) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_bin_kernel<2, decltype(m)>), grid, block, 0, s, e, m, g, all, words); });
		else if (e.num_pes == 3) with_model(model, [&](auto m) { hipLaunchKernelGGL((hop_bin_kernel<3, decltype(m)>), grid, block, 0, s, e, m, g, all, words); });
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
	hipError_t launch_hop_density(hipStream_t s, int num_pes, long cells, double w, const long long* acc, double* rho)
	{
		if (cells <= 0) return hipErrorInvalidValue;
		const dim3 grid(hop_blocks(cells)), block(HOP_BLOCK);
		if (num_pes == 2) hipLaunchKernelGGL(hop_density_kernel<2>, grid, block, 0, s, cells, w, acc, rho);
		else if (num_pes == 3) hipLaunchKernelGGL(hop_density_kernel<3>, grid, block, 0, s, cells, w, acc, rho);
		else return hipErrorInvalidValue;
		return hipGetLastError();
	}
} // namespace gple
