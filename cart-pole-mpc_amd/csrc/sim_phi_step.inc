// sim_phi_step.inc -- Phi <- A Phi for the Jacobian A of one sub-step of length h, a column at a time by step_jac_apply; the
// closed-form columns of Phi (sim_window.hpp: phi_identity) are neither stored nor propagated.  Included by sim_jac_tick.inc,
// sim_rollout_gn_x0_kernel and sim_ekf_body.inc: one text, the same instructions in all (as a function: DESIGN.md 5l).
// Expects in scope: R, M, NX, TRIV, A, h and Phi.
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
