// sim_jac_tick.inc -- one tick of the plant with Phi = dx+/dx and gamma = dx+/du of the whole tick, accumulated forward over
// its sub-steps (sim_jac_kernels.hpp): Phi <- A_i Phi, gamma <- A_i gamma + B_i from Phi = I, gamma = 0.  Included by
// sim_jac_kernel and by pass A of sim_rollout_vjp_kernel: one text, and so the same instructions in both.
// Expects in scope: R, M, NX, TRIV (the closed-form columns), k, fe, n_sub, h_last, uu and the state xs (advanced in place).
// Declares: Phi, gam and t_sum.
  R Phi[NX][NX], gam[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) {
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (!((TRIV >> c) & 1u)) Phi[r][c] = (r == c) ? R(1) : R(0);
    gam[r] = R(0);
  }
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
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        if ((TRIV >> c) & 1u) continue;
        R v[NX], y[NX];
#pragma unroll
        for (int m = 0; m < NX; ++m) v[m] = Phi[m][c];
        step_jac_apply<R, M>(A, h, v, y);
#pragma unroll
        for (int r = 0; r < NX; ++r) Phi[r][c] = y[r];
      }
      {
        R y[NX];
        step_jac_apply<R, M>(A, h, gam, y);
#pragma unroll
        for (int r = 0; r < NX; ++r) gam[r] = y[r] + Bv[r];
      }
      if (TRIV != 0u) t_sum += h;
    }
  }
