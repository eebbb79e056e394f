// sim_ekf_kernels.hpp -- the extended Kalman filter of B plants over T ticks in one kernel: with x_{t+1} = Step(x_t, u_t, dt)
// as sim_rollout_kernel runs it, A_t = dx_{t+1}/dx_t of the tick at the FILTERED state, q the process-noise variances added
// once a tick and w the inverse variances of the measurement (StateWeights: the weights of sim_rollout_gn_x0_kernel),
//     predict     x- = Step(x, u_t, dt),     P- = A_t P A_t^T + diag(q)
//     update      one measured state i at a time, in index order, where rho_i = om_t w_i > 0 (om_t = tick_w ? tick_w[t] : 1):
//                     s = P_ii + 1/rho_i,    nu = wrap_i(y[t][i] - x_i),    K = P[:, i] / s
//                     x += K nu,    P_jk -= K_j P_ki (j, k != i),    P_ji = P_ij = K_j / rho_i,    nis += nu^2 / s
//                 then wrap_angles(x) where an update acted
// No matrix is inverted: a diagonal measurement covariance makes the joint update the sequence of scalar ones.  Row and
// column i are formed as K_j / rho_i, which is P_ji - K_j P_ii without the cancellation.
//
// A tick's prediction is sim_jac_tick.inc's sub-step loop -- rk4_step_jac_m, step_jac_apply a column at a time, Phi from I,
// the closed-form columns (models.hpp: trivial_cols) closed-form -- without gamma, and with the STATE advanced by
// plant_sub_step, the function sim_rollout_kernel's loop calls, from the same point: the predicted state is that kernel's bit
// for bit (see the loop).  The `for` statement is the kernel's own, as sim_rollout_gn_x0_kernel's is; Phi = I (phi_identity) and
// Phi <- A Phi (sim_phi_step.inc) are the pieces of sim_jac_tick.inc, and P_final leaves by sim_store_sym.inc.  The body is
// sim_ekf_body.inc, one text for the filter and for the smoother's recording forward pass.  The tick's A stays in
// registers and never goes to memory.  The products A P and (A P) A^T take the closed-form columns' entries as the 0, 1 and
// t_sum they are: a structural zero is not multiplied, a one is not a product.  Only the lower triangle of P is computed and
// kept, (j, k <= j) at tri(j, k) (sim_window.hpp).
//
// One problem per lane, no barrier.  P lives in lane-private LDS, acc[field][threadIdx.x], while the sub-step loop runs, so
// what is live there is sim_rollout_gn_x0_kernel's set: the tick's Phi and the sub-step's A.  Everything is computed
// whichever outputs are stored (wave-uniform pointer tests), so each is bitwise the same whatever else is asked for.  A lane
// with rho_i = 0 for every i of a tick (state not measured, sample missing) keeps the x and P the prediction left, bit for bit;
// y is not read there.  n_sub == 0 is the identity plant: A = I, and the same statements are the linear Kalman filter of a
// constant state.  Not modelled: noise on the control, the parameters and the forces.
#pragma once
#include "sim_rollout_gn_x0_kernels.hpp"

namespace cpmpc {

// s (+)= A(r, c) v for the tick's A = Phi with its closed-form columns: nothing for a structural zero, v itself for the one
// on the diagonal of a closed-form column, t_sum v for its entry in row c - NQ
template <typename R, int NX, int NQ, unsigned TRIV>
__device__ __forceinline__ void ekf_add_term(const R (&Phi)[NX][NX], R t_sum, int r, int c, R v, bool& have, R& s) {
  if (struct_zero<NX, NQ>(TRIV, r, c)) return;
  R term;
  if ((TRIV >> c) & 1u) term = (r == c) ? v : t_sum * v;
  else term = Phi[r][c] * v;
  s = have ? s + term : term;
  have = true;
}

// Outputs, each written only where its pointer is given: x_final [NX][B]; P_final [NX*NX][B], full, (j, k) and (k, j) from the
// one kept value; xs [T][NX][B], the filtered state after every tick; nis [B], the normalised squared innovations added up.
// P0 [NX*NX][B]: its lower triangle (fields j*NX + k, k <= j) is read.  y [T][NX][B] is read only where rho_i > 0.  sw: the
// measurements' inverse variances; q: the process-noise variances.  PER_LANE as sim_jac_kernel's.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_ekf_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg,
                                                      ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
                                                      const R* x0, const R* P0, const R* u, const R* y,
                                                      StateWeights<R, M::NX> sw, StateWeights<R, M::NX> q, const R* tick_w,
                                                      R* x_final, R* P_final, R* xs_out, R* nis) {
  constexpr bool RECORD = false;
  R* const work = nullptr;
#include "sim_ekf_body.inc"
}

// The same filter as the forward pass of the smoother (sim_rts_kernels.hpp): the same body, which additionally stores per tick
// x-, P- before the update, the rows of A P, and the filtered x and P into work [T * RtsRecord<NX>::ROWS][B] -- what the tick
// already has in registers.  The other outputs are sim_ekf_kernel's bit for bit.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_ekf_record_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg,
                                                             ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
                                                             const R* x0, const R* P0, const R* u, const R* y,
                                                             StateWeights<R, M::NX> sw, StateWeights<R, M::NX> q,
                                                             const R* tick_w, R* x_final, R* P_final, R* xs_out, R* nis,
                                                             R* work) {
  constexpr bool RECORD = true;
#include "sim_ekf_body.inc"
}

}  // namespace cpmpc
