// sim_window_residual.inc -- tick t of a window fit against the recording: res = wrap(x_obs[t] - xs), its tick weight om, and
// cost_sum += 1/2 om res^T W res.  Included by sim_rollout_gn_kernel and sim_rollout_gn_x0_kernel (as a function: DESIGN.md 5l).
// Expects in scope: R, M, NX, B, p, t, x_obs, tick_w, sw, the state xs and cost_sum.  Declares: res and om.
      R res[NX];
#pragma unroll
      for (int q = 0; q < NX; ++q) res[q] = x_obs[((int64_t)t * NX + q) * B + p] - xs[q];
      wrap_residual<R, M>(res);
      const R om = tick_w ? tick_w[(int64_t)t * B + p] : R(1);
      R wr[NX];  // W r
#pragma unroll
      for (int q = 0; q < NX; ++q) wr[q] = sw.w[q] * res[q];
      R c = wr[0] * res[0];
#pragma unroll
      for (int q = 1; q < NX; ++q) c += wr[q] * res[q];
      cost_sum += (R(0.5) * om) * c;
