// sim_jac_kernels.hpp -- the plant step with its first derivatives: Simulator::Step (simulator.cc:11-36) as sim_kernel runs
// it -- 1 ms RK4 sub-steps with the control held, the last one h_last, the pole angles wrapped after each -- together with
//     Phi = dx+/dx  (NX x NX)  and  gamma = dx+/du  (NX)
// of the whole step, accumulated FORWARD over the sub-steps as linearize_kernel accumulates an interval:
//     Phi <- A_i Phi,   gamma <- A_i gamma + B_i,   Phi_0 = I, gamma_0 = 0,
// with A_i, B_i from rk4_step_jac_m (external forces included).  The wrap has unit derivative.  Nothing per sub-step is
// stored, whatever their number.  One problem per lane, no LDS; the state is read only.  The accumulation over a tick is
// sim_jac_tick.inc and the product Phi^T g is sim_jac_vjp.inc: texts that pass A of sim_rollout_vjp_kernel includes too.
//
// Outputs, each written only where its pointer is given (a wave-uniform choice): x_new [NX][B], A = Phi [NX*NX][B] (element
// (r, c) at field r*NX + c, the layout of rk4_kernel), Bu = gamma [NX][B] and, for a cotangent gbar [NX][B], the products
// gx = Phi^T gbar [NX][B] and gu = gamma . gbar [B] contracted in registers.  Derivatives with respect to the state and the
// control only: the dynamics parameters have sim_param_kernels.hpp; none for the external forces or the step length.
#pragma once
#include "sim_window.hpp"

namespace cpmpc {

// PER_LANE: per-problem dynamics parameters (plant_kernels.hpp: PlantConsts); the default is the shared set.
template <typename R, typename M, bool PER_LANE = false>
__global__ __launch_bounds__(64) void sim_jac_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg,
                                                      ExtForce<R> fe_shared, const R* fext,
                                                      int n_sub, R h_last, const R* state, const R* u, R* x_new, R* A_out,
                                                      R* Bu, const R* gbar, R* gx, R* gu) {
  constexpr int NX = M::NX, NQ = M::NQ;
  // Columns of every A_i known in closed form (models.hpp: trivial_cols).  Their pattern is closed under the product: column
  // c of Phi stays e_c, plus the time integrated so far in row c - NQ when c is a velocity -- neither stored nor multiplied.
  constexpr unsigned TRIV = trivial_cols<NX, NQ>(JaZeroCols<M>::value);
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
  R xs[NX];
#pragma unroll
  for (int t = 0; t < NX; ++t) xs[t] = state[t * B + p];
  const R uu = u[p];

#include "sim_jac_tick.inc"  // Phi, gam, t_sum of the tick; xs becomes x+

  if (x_new)
#pragma unroll
    for (int t = 0; t < NX; ++t) x_new[t * B + p] = xs[t];
  if (A_out)
#pragma unroll
    for (int r = 0; r < NX; ++r)
#pragma unroll
      for (int c = 0; c < NX; ++c) A_out[(r * NX + c) * B + p] = phi_entry<R, M>(Phi, t_sum, r, c);
  if (Bu)
#pragma unroll
    for (int r = 0; r < NX; ++r) Bu[r * B + p] = gam[r];
  if (gbar) {
    R g[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) g[r] = gbar[r * B + p];
    if (n_sub == 0) {  // the identity map: the cotangent itself, not its products with ones and zeros
      if (gx)
#pragma unroll
        for (int c = 0; c < NX; ++c) gx[c * B + p] = g[c];
      if (gu) gu[p] = R(0);
      return;
    }
    if (gx) {
#define CPMPC_PHI_T_G(c) gx[(c) * B + p]
#include "sim_jac_vjp.inc"
#undef CPMPC_PHI_T_G
    }
    if (gu) {
      R acc = gam[0] * g[0];
#pragma unroll
      for (int r = 1; r < NX; ++r) acc += gam[r] * g[r];
      gu[p] = acc;
    }
  }
}

}  // namespace cpmpc
