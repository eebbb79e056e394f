// sim_param_tick.inc -- one tick of the plant carrying the tangents Tn[g] = dx+/dp_{J0 + g} of the whole tick through its
// sub-steps from Tn = 0 (sim_param_kernels.hpp: rk4_step_param_m).  Included by sim_param_jac_kernel and by pass B of
// sim_rollout_vjp_kernel: one text, and so the same instructions in both.
// Expects in scope: R, M, NX, J0, NG (the group of columns), k, prm, fe, n_sub, h_last, uu and the state xs (advanced in place).
// Declares: Tn.
  R Tn[NG][NX];
#pragma unroll
  for (int gI = 0; gI < NG; ++gI)
#pragma unroll
    for (int r = 0; r < NX; ++r) Tn[gI][r] = R(0);
  {
    const R internal_dt = R(0.001);
    typename M::StepCache chain;
#pragma unroll 1
    for (int i = 0; i < n_sub; ++i) {
      const R h = (i + 1 == n_sub) ? h_last : internal_dt;
      rk4_step_param_m<R, M, true, J0, NG>(k, prm, h, xs, uu, fe, Tn, chain);
      wrap_angles<R, M>(xs);
    }
  }
