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
// Phi <- A Phi (sim_phi_step.inc) are the pieces of sim_jac_tick.inc, and P_final leaves by sim_store_sym.inc.  The tick's A stays in
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
  constexpr int NX = M::NX, NQ = M::NQ;
  constexpr unsigned TRIV = trivial_cols<NX, NQ>(JaZeroCols<M>::value);  // sim_jac_kernel's closed-form columns
  constexpr int NH = tri(NX, 0);  // P's lower triangle, (j, k <= j) at tri(j, k)
  __shared__ R acc[NH][64];
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);

  R xs[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) xs[r] = x0[r * B + p];
#pragma unroll
  for (int j = 0; j < NX; ++j)
#pragma unroll
    for (int kk = 0; kk <= j; ++kk) acc[tri(j, kk)][lane] = P0[(j * NX + kk) * B + p];
  R nis_sum = R(0);

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const R uu = u[(int64_t)t * B + p];
    // ---- predict: the tick's sub-step loop, Phi from I
    R Phi[NX][NX];
    phi_identity<R, M>(Phi);
    R t_sum = R(0);  // entry (c - NQ, c) of a trivial velocity column: the sub-steps' lengths of this tick
    {
      const R internal_dt = R(0.001);
      typename M::StepCache chain, chain_x;
#pragma unroll 1
      for (int i = 0; i < n_sub; ++i) {
        const R h = (i + 1 == n_sub) ? h_last : internal_dt;
        R A[NX][NX], Bv[NX], xj[NX];
        // The state moves by sim_rollout_kernel's own sub-step, so that a lane on which no update acts follows that kernel
        // bit for bit: rk4_step_jac_m evaluates the same stages beside their Jacobians, and the compiler contracts the two
        // texts differently (1 - 2 ulps a tick for the 6-state model).  A is the sub-step's Jacobian from the same state,
        // taken through an empty asm so that the two evaluations share no sub-expression and the state's stays the text
        // sim_rollout_kernel compiles; the state rk4_step_jac_m leaves in xj is dead.
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          xj[r] = xs[r];
          asm("" : "+v"(xj[r]));
        }
        plant_sub_step<R, M>(k, fe, i, n_sub, h_last, uu, xs, chain_x);
        rk4_step_jac_m<R, M, true>(k, h, xj, uu, fe, A, Bv, chain);
#include "sim_phi_step.inc"
        if (TRIV != 0u) t_sum += h;
      }
    }

    // ---- P- = A P A^T + diag(q), a row of A P at a time; P is (j, k) -> Pm[tri_sym(j, k)]
    R Pm[NH], Pn[NH];
#pragma unroll
    for (int f = 0; f < NH; ++f) Pm[f] = acc[f][lane];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R row[NX];  // row j of A P
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        bool have = false;
        R s = R(0);
#pragma unroll
        for (int l = 0; l < NX; ++l)
          ekf_add_term<R, NX, NQ, TRIV>(Phi, t_sum, j, l, Pm[tri_sym(l, c)], have, s);
        row[c] = s;
      }
#pragma unroll
      for (int kk = 0; kk <= j; ++kk) {
        bool have = false;
        R s = R(0);
#pragma unroll
        for (int l = 0; l < NX; ++l) ekf_add_term<R, NX, NQ, TRIV>(Phi, t_sum, kk, l, row[l], have, s);
        Pn[tri(j, kk)] = (kk == j) ? s + q.w[j] : s;
      }
    }

    // ---- update: the measured states one at a time
    const R om = tick_w ? tick_w[(int64_t)t * B + p] : R(1);
    bool acted = false;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const R rho = om * sw.w[i];
      if (rho > R(0)) {
        const R rv = R(1) / rho;
        const R s = Pn[tri(i, i)] + rv;
        R res[NX];
#pragma unroll
        for (int m = 0; m < NX; ++m) res[m] = R(0);
        res[i] = y[((int64_t)t * NX + i) * B + p] - xs[i];
        wrap_residual<R, M>(res);
        const R nu = res[i];
        R gain[NX];
#pragma unroll
        for (int j = 0; j < NX; ++j) gain[j] = Pn[tri_sym(j, i)] / s;
#pragma unroll
        for (int j = 0; j < NX; ++j) xs[j] += gain[j] * nu;
        nis_sum += nu * nu / s;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          if (j == i) continue;
#pragma unroll
          for (int kk = 0; kk <= j; ++kk) {
            if (kk == i) continue;
            Pn[tri(j, kk)] -= gain[j] * Pn[tri_sym(kk, i)];
          }
        }
#pragma unroll
        for (int j = 0; j < NX; ++j) Pn[tri_sym(j, i)] = gain[j] * rv;
        acted = true;
      }
    }
    if (acted) wrap_angles<R, M>(xs);  // not where nothing acted: the wrap of a wrapped angle is not always that angle

#pragma unroll
    for (int f = 0; f < NH; ++f) acc[f][lane] = Pn[f];
    if (xs_out)
#pragma unroll
      for (int r = 0; r < NX; ++r) xs_out[((int64_t)t * NX + r) * B + p] = xs[r];
  }

  if (x_final)
#pragma unroll
    for (int r = 0; r < NX; ++r) x_final[r * B + p] = xs[r];
  if (P_final) {
    constexpr int NS = NX;
    R* const out = P_final;
#include "sim_store_sym.inc"
  }
  if (nis) nis[p] = nis_sum;
}

}  // namespace cpmpc
