// sim_jac_vjp.inc -- Phi^T g for the Phi of sim_jac_tick.inc, the closed-form columns as they are known.  Not for n_sub == 0,
// where nothing was accumulated: the callers copy g instead.  Included by sim_jac_kernel and by pass A of
// sim_rollout_vjp_kernel.  Expects in scope: R, NX, NQ, TRIV, Phi, t_sum and the cotangent g, and CPMPC_PHI_T_G(c) defined: where
// element c of the product goes (an array in global memory in the one, registers in the other).
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    R acc;
    if ((TRIV >> c) & 1u) {
      acc = g[c];
      if (c >= NQ) acc += t_sum * g[c - NQ];
    } else {
      acc = Phi[0][c] * g[0];
#pragma unroll
      for (int r = 1; r < NX; ++r) acc += Phi[r][c] * g[r];
    }
    CPMPC_PHI_T_G(c) = acc;
  }
