// sim_store_sym.inc -- the NS x NS symmetric matrix whose lower triangle the lane keeps in its LDS fields, acc[tri(j, k)][lane],
// to out [NS*NS][B] in full: (j, k) and (k, j) from the one kept value.  Included for H by sim_rollout_gn_kernel and
// sim_rollout_gn_x0_kernel and for P_final by sim_ekf_body.inc (as a function: more spill reloads in the tick loops, DESIGN.md 5l).
// Expects in scope: R, NS, out, B, p, acc and lane.
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int kk = 0; kk <= j; ++kk) {
        const R v = acc[tri(j, kk)][lane];
        out[(j * NS + kk) * B + p] = v;
        if (kk != j) out[(kk * NS + j) * B + p] = v;
      }
