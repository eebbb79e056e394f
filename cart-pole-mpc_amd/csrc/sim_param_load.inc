// sim_param_load.inc -- the raw dynamics parameters of a lane into prm [NP]: dyn [NP][B] read per lane (PER_LANE), else the
// shared set's `raw`.  Included by sim_param_jac_kernel and, twice, by sim_rollout_vjp_kernel.
// Expects in scope: R, NP, PER_LANE, raw, dyn, B, p and prm.
  if constexpr (PER_LANE) {
#pragma unroll
    for (int i = 0; i < NP; ++i) prm[i] = dyn[i * B + p];
  } else {
#pragma unroll
    for (int i = 0; i < NP; ++i) prm[i] = raw.p[i];
  }
