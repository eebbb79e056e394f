// sim_rollout_gn_kernels.hpp -- the FORWARD mode of the plant rollout in the dynamics parameters, and the Gauss-Newton normal
// equations of an output-error fit over the window, in one kernel: with x_{t+1} = Step(x_t, u_t, dt) as sim_rollout_kernel runs
// it and S_t = dx_t/dp (S_0 = 0; x0 is not a function of the parameters),
//     S_{t+1} = A_t S_t + P_t,                      A_t = dx_{t+1}/dx_t,  P_t the tick's own dx_{t+1}/dp
//     r_t     = wrap(x_obs[t] - x_{t+1}),           om_t = tick_w ? tick_w[t] : 1,  W = diag(w)
//     cost    = 1/2 sum_t om_t r_t^T W r_t
//     g       = -sum_t om_t S_{t+1}^T W r_t         = dcost/dp
//     H       =  sum_t om_t S_{t+1}^T W S_{t+1}     the Gauss-Newton matrix; the step is -H^-1 g
// No A_t is formed.  rk4_step_param_m (sim_param_kernels.hpp) carries tangent columns through the RK4 stages with
// dk = K t + Jp[:, j]: fed the tangents the last tick left instead of zeros, the same statements do A_i t and + P_i at once.  So
// a tick here is sim_param_tick.inc's sub-step loop with the tangents carried over the tick boundary -- the kernel keeps its
// own loop for that, as sim_kernel and sim_rollout_kernel keep theirs -- and the dependent chain is walked once per tick.
//
// One problem per lane.  S [NP][NX], x and cost stay in registers over the ticks; H (packed lower triangle) and g live in
// lane-private LDS, acc[field][threadIdx.x], read and written once per tick and never by another lane: no barrier anywhere.
// In registers they put three of the eight instantiations into scratch.  S never goes to memory except as
// S_final.  The accumulation runs where any of cost, g, H is asked for (a wave-uniform choice) and is the same statements
// whichever of them are stored, so each is bitwise the same whatever else is asked for.  The tick's residual, its share of
// the normal equations and the store of H are the texts sim_rollout_gn_x0_kernel includes too: sim_window_residual.inc,
// sim_normal_eq.inc (here with dense columns, NeverZero) and sim_store_sym.inc.
// n_sub == 0 is the identity map: S stays 0, so H = 0, g = 0, S_final = 0, x_final = x0, and cost is the weighted residual of
// x0 against every x_obs[t].  Not differentiated: the external forces, dt and x0; the wrap has unit derivative.
#pragma once
#include "sim_param_kernels.hpp"
#include "sim_window.hpp"

namespace cpmpc {

// Outputs, each written only where its pointer is given: cost [B]; g [NP][B]; H [NP*NP][B], full, (j, k) and (k, j) from the one
// accumulated value; S_final [NX*NP][B], element (r, j) at field r*NP + j as P; x_final [NX][B].  x_obs [T][NX][B] is read only
// where cost, g or H is given.  PER_LANE as sim_param_jac_kernel's.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_rollout_gn_kernel(int64_t B, typename M::Consts k_shared, RawParams<R, M::NP> raw,
                                                             const R* dyn, ExtForce<R> fe_shared, const R* fext, int n_sub,
                                                             R h_last, int T, const R* x0, const R* u, const R* x_obs,
                                                             StateWeights<R, M::NX> sw, const R* tick_w, R* cost, R* g, R* H,
                                                             R* S_final, R* x_final) {
  constexpr int NX = M::NX, NP = M::NP;
  constexpr int NH = tri(NP, 0);  // H's lower triangle, (j, k <= j) at tri(j, k); g behind it
  __shared__ R acc[NH + NP][64];
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
  R prm[NP];
  typename M::Consts k = k_shared;
#include "sim_param_load.inc"
  if constexpr (PER_LANE) k = M::template make<R>(prm);

  const bool fit = cost || g || H;
  R xs[NX], S[NP][NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) xs[r] = x0[r * B + p];
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int r = 0; r < NX; ++r) S[j][r] = R(0);
#pragma unroll
  for (int f = 0; f < NH + NP; ++f) acc[f][lane] = R(0);
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
        rk4_step_param_m<R, M, true, 0, NP>(k, prm, h, xs, uu, fe, S, chain);  // S is carried, not reset
        wrap_angles<R, M>(xs);
      }
    }
    if (fit) {
#include "sim_window_residual.inc"  // res, om; adds to cost_sum
      constexpr int NC = NP;
      const R (&col)[NP][NX] = S;  // the columns, under the names sim_normal_eq.inc reads
      using Zero = NeverZero;
#include "sim_normal_eq.inc"
    }
  }

  if (cost) cost[p] = cost_sum;
  if (g)
#pragma unroll
    for (int j = 0; j < NP; ++j) g[j * B + p] = acc[NH + j][lane];
  if (H) {
    constexpr int NS = NP;
    R* const out = H;
#include "sim_store_sym.inc"
  }
  if (S_final)
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int r = 0; r < NX; ++r) S_final[(r * NP + j) * B + p] = S[j][r];
  if (x_final)
#pragma unroll
    for (int r = 0; r < NX; ++r) x_final[r * B + p] = xs[r];
}

}  // namespace cpmpc
