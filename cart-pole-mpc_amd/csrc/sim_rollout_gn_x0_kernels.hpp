// sim_rollout_gn_x0_kernels.hpp -- the FORWARD mode of the plant rollout in the INITIAL STATE, and the Gauss-Newton normal
// equations of an output-error fit of x0 over the window, in one kernel: with x_{t+1} = Step(x_t, u_t, dt) as
// sim_rollout_kernel runs it and Phi_t = dx_t/dx0,
//     Phi_0 = I,  Phi_{t+1} = A_t Phi_t,            A_t = dx_{t+1}/dx_t of the tick
//     r_t     = wrap(x_obs[t] - x_{t+1}),           om_t = tick_w ? tick_w[t] : 1,  W = diag(w)
//     cost    = 1/2 sum_t om_t r_t^T W r_t
//     g       = -sum_t om_t Phi_{t+1}^T W r_t       = dcost/dx0
//     H       =  sum_t om_t Phi_{t+1}^T W Phi_{t+1} the Gauss-Newton matrix; the step is -H^-1 g
// A tick is sim_jac_tick.inc's sub-step loop -- rk4_step_jac_m, wrap_angles, step_jac_apply a column at a time -- with Phi
// carried over the tick boundary instead of starting from I, and without gamma.  The `for` statement is the kernel's own; what
// it does to Phi is not: phi_identity and phi_entry (sim_window.hpp) and the text sim_phi_step.inc are the ones sim_jac_tick.inc
// and sim_jac_kernel use, so Phi_final of one tick is that kernel's A by construction.  No per-tick A_t is formed and Phi never
// goes to memory except as Phi_final.
//
// The closed-form columns (models.hpp: trivial_cols) stay closed-form across ticks, because their pattern is closed under the
// product: a position column stays e_c, a velocity column stays e_c + t_sum e_{c-NQ} with t_sum the sub-steps' lengths added
// up over the WHOLE window.  They are neither stored nor propagated, and the sums below take their entries as the 0, 1 and
// t_sum they are: a structural zero is not multiplied, a one is not a product.
//
// One problem per lane.  Phi, x, t_sum and cost stay in registers over the ticks; H (packed lower triangle) and g live in
// lane-private LDS, acc[field][threadIdx.x], read and written once per tick and never by another lane: no barrier anywhere
// (the layout of sim_rollout_gn_kernel, and its texts: sim_window_residual.inc, sim_normal_eq.inc -- here with PhiZero, the
// structural zeros of the closed-form columns -- and sim_store_sym.inc).  The accumulation runs where any of cost, g, H is asked for (a wave-uniform
// choice) and is the same statements whichever of them are stored, so each is bitwise the same whatever else is asked for.
// n_sub == 0 is the identity map: Phi stays I and x_final = x0; H = sum_t om_t W and g = -sum_t om_t W r_t come from the
// same statements.  Not differentiated: the parameters (sim_rollout_gn_kernel), the external forces and dt; the wrap has
// unit derivative.
#pragma once
#include "sim_rollout_gn_kernels.hpp"

namespace cpmpc {

// Outputs, each written only where its pointer is given: cost [B]; g [NX][B]; H [NX*NX][B], full, (j, k) and (k, j) from the
// one accumulated value; Phi_final [NX*NX][B], element (r, c) at field r*NX + c as sim_jac_kernel's A; x_final [NX][B].
// x_obs [T][NX][B] is read only where cost, g or H is given.  PER_LANE as sim_jac_kernel's.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_rollout_gn_x0_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg,
                                                                ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last,
                                                                int T, const R* x0, const R* u, const R* x_obs,
                                                                StateWeights<R, M::NX> sw, const R* tick_w, R* cost, R* g,
                                                                R* H, R* Phi_final, R* x_final) {
  constexpr int NX = M::NX, NQ = M::NQ;
  constexpr unsigned TRIV = trivial_cols<NX, NQ>(JaZeroCols<M>::value);  // sim_jac_kernel's closed-form columns
  constexpr int NH = tri(NX, 0);  // H's lower triangle, (j, k <= j) at tri(j, k); g behind it
  __shared__ R acc[NH + NX][64];
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);

  const bool fit = cost || g || H;
  R xs[NX], Phi[NX][NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) xs[r] = x0[r * B + p];
  phi_identity<R, M>(Phi);
#pragma unroll
  for (int f = 0; f < NH + NX; ++f) acc[f][lane] = R(0);
  R t_sum = R(0);  // entry (c - NQ, c) of a trivial velocity column: the sub-steps' lengths of every tick so far
  R cost_sum = R(0);

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const R uu = u[(int64_t)t * B + p];
    {
      const R internal_dt = R(0.001);
      typename M::StepCache chain;
#pragma unroll 1
      for (int i = 0; i < n_sub; ++i) {
        const R h = (i + 1 == n_sub) ? h_last : internal_dt;
        R A[NX][NX], Bv[NX];
        rk4_step_jac_m<R, M, true>(k, h, xs, uu, fe, A, Bv, chain);
        wrap_angles<R, M>(xs);
#include "sim_phi_step.inc"  // Phi is carried, not reset
        if (TRIV != 0u) t_sum += h;
      }
    }
    if (fit) {
#include "sim_window_residual.inc"  // res, om; adds to cost_sum
      R col[NX][NX];  // col[j][q] = Phi(q, j), the closed-form columns as they are known; structural zeros are never read
#pragma unroll
      for (int j = 0; j < NX; ++j)
#pragma unroll
        for (int q = 0; q < NX; ++q) {
          if (struct_zero<NX, NQ>(TRIV, q, j)) continue;
          if ((TRIV >> j) & 1u) col[j][q] = (q == j) ? R(1) : t_sum;
          else col[j][q] = Phi[q][j];
        }
      constexpr int NC = NX;
      using Zero = PhiZero<NX, NQ, TRIV>;
#include "sim_normal_eq.inc"
    }
  }

  if (cost) cost[p] = cost_sum;
  if (g)
#pragma unroll
    for (int j = 0; j < NX; ++j) g[j * B + p] = acc[NH + j][lane];
  if (H) {
    constexpr int NS = NX;
    R* const out = H;
#include "sim_store_sym.inc"
  }
  if (Phi_final)
#pragma unroll
    for (int r = 0; r < NX; ++r)
#pragma unroll
      for (int c = 0; c < NX; ++c) Phi_final[(r * NX + c) * B + p] = phi_entry<R, M>(Phi, t_sum, r, c);
  if (x_final)
#pragma unroll
    for (int r = 0; r < NX; ++r) x_final[r * B + p] = xs[r];
}

}  // namespace cpmpc
