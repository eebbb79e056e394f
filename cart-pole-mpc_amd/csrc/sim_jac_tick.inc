// sim_jac_tick.inc -- one tick of the plant with Phi = dx+/dx and gamma = dx+/du of the whole tick, accumulated forward over
// its sub-steps (sim_jac_kernels.hpp): Phi <- A_i Phi, gamma <- A_i gamma + B_i from Phi = I, gamma = 0.  Included by
// sim_jac_kernel and by pass A of sim_rollout_vjp_kernel: one text, and so the same instructions in both.
// Phi = I and Phi <- A_i Phi are phi_identity (sim_window.hpp) and sim_phi_step.inc, which sim_rollout_gn_x0_kernel and
// sim_ekf_kernel use for their own Phi.
// Expects in scope: R, M, NX, TRIV (the closed-form columns), k, fe, n_sub, h_last, uu and the state xs (advanced in place).
// Declares: Phi, gam and t_sum.
  R Phi[NX][NX], gam[NX];
  phi_identity<R, M>(Phi);
#pragma unroll
  for (int r = 0; r < NX; ++r) gam[r] = R(0);
  R t_sum = R(0);  // entry (c - NQ, c) of a trivial velocity column: the sub-steps' lengths added up
  {
    const R internal_dt = R(0.001);
    typename M::StepCache chain;
#pragma unroll 1
    for (int i = 0; i < n_sub; ++i) {
      const R h = (i + 1 == n_sub) ? h_last : internal_dt;
      R A[NX][NX], Bv[NX];
      rk4_step_jac_m<R, M, true>(k, h, xs, uu, fe, A, Bv, chain);
      wrap_angles<R, M>(xs);
#include "sim_phi_step.inc"
      {
        R y[NX];
        step_jac_apply<R, M>(A, h, gam, y);
#pragma unroll
        for (int r = 0; r < NX; ++r) gam[r] = y[r] + Bv[r];
      }
      if (TRIV != 0u) t_sum += h;
    }
  }
