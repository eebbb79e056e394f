// sim_roll_ticks.inc -- the plant rolled over T ticks from x0, one problem per lane: the whole body of sim_rollout_kernel,
// sim_rollout_fb_kernel (sim_track_kernels.hpp), sim_ilqr_forward_kernel and sim_ilqr_search_kernel (sim_ilqr_kernels.hpp).  One
// text, with three parts chosen where it is included, so the four kernels' states are the same bits by construction and a part
// compiled out leaves no instruction behind:
//   CPMPC_ROLL_LAW     the tick's control is formed at the tick's start and held over its sub-steps,
//                          u_t = clamp(u_nom[t] + alpha kff[t] + K[t] . wrap_residual(x_t - x_nom_t), +-u_limit)   -> us_out[t]
//                      kff, K and alpha_in each nullable (alpha: 1); x0_nom and xs_nom are read only where K is given, row T-1
//                      never.  Without the part the control is u_nom[t] as it stands.
//   CPMPC_ROLL_COST    J of sim_ilqr_kernels.hpp is summed, a tick's term at its start and the terminal one after the roll -> cost_out
//   CPMPC_ROLL_SEARCH  (needs both others) the roll is the body of a per-lane trial loop: alpha starts at 1 and is halved until
//                      the roll's J passes the Armijo test against cost_nom and dV, at most `trials` times; the roll stores xs_out
//                      and us_out as it goes, so an accepted trial's are in place, and a lane that accepted none copies its
//                      nominal.  alpha is the loop's own (there is no alpha_in) and x_nom_0 is x0 itself (no x0_nom).
// Expects in scope: R, M, PER_LANE, B, k_arg, fe_shared, fext, n_sub, h_last, T, x0, u_nom, xs_out, x_final; with the law kff, K,
// x0_nom, xs_nom, alpha_in, u_limit, us_out; with the cost x0_ref, xs_ref, u_ref, q, rw, PT, qf, cost_out; with the search
// cost_nom, dV, trials, armijo, alpha_out (and neither x0_nom nor alpha_in).  The three macros are defined, 0 or 1, by the file
// that includes this one, and undefined here.
  constexpr int NX = M::NX;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
#if CPMPC_ROLL_SEARCH
  const R* const x0_nom = x0;
  const R J_nom = cost_nom[p], dV1 = dV[p], dV2 = dV[B + p];
  R alpha = R(1);
  bool accepted = false;
#elif CPMPC_ROLL_LAW
  const R alpha = alpha_in ? alpha_in[p] : R(1);
#endif
#if CPMPC_ROLL_COST
  // the terminal weights wait in vector registers for the end of the roll: as kernel arguments they would sit in scalar
  // registers beside the folded plant constants through the whole tick loop, and the double 6-state form runs out of those
  R qfv[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) {
    qfv[r] = qf.w[r];
    asm("" : "+v"(qfv[r]));
  }
#endif
  R xs[NX];
#if CPMPC_ROLL_COST
  R J;
#endif
#if CPMPC_ROLL_SEARCH
  // an ordinary per-lane loop: a lane that has decided leaves it, and the wave goes on with the lanes that have not
  const int64_t p_lane = p;
#pragma unroll 1
  for (int trial = 0; trial < trials; ++trial) {
    // the lane's index as a value the compiler cannot see through: each trial forms its addresses from it afresh and steps them
    // in place as the forward kernel does, where otherwise every array's start would stay live beside its running pointer
    int64_t p = p_lane;
    asm("" : "+v"(p));
#endif
#pragma unroll
  for (int r = 0; r < NX; ++r) xs[r] = x0[r * B + p];
#if CPMPC_ROLL_COST
  J = R(0);
#endif
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    R uu = u_nom[(int64_t)t * B + p];
#if CPMPC_ROLL_LAW
    if (kff) uu = Math<R>::fma(alpha, kff[(int64_t)t * B + p], uu);
    if (K) {
      const R* xn = (t == 0) ? x0_nom : xs_nom + (int64_t)(t - 1) * NX * B;
      R d[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) d[r] = xs[r] - xn[r * B + p];
      wrap_residual<R, M>(d);
#pragma unroll
      for (int r = 0; r < NX; ++r) uu = Math<R>::fma(K[((int64_t)t * NX + r) * B + p], d[r], uu);
    }
    uu = clampr(uu, -u_limit, u_limit);
    if (us_out) us_out[(int64_t)t * B + p] = uu;
#endif
#if CPMPC_ROLL_COST
    {  // the tick's cost, at its start
      const R* xr = (t == 0) ? x0_ref : xs_ref + (int64_t)(t - 1) * NX * B;
      R e[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) e[r] = xs[r] - xr[r * B + p];
      wrap_residual<R, M>(e);
      const R du = uu - (u_ref ? u_ref[(int64_t)t * B + p] : R(0));
      R c = rw * du * du;
#pragma unroll
      for (int r = 0; r < NX; ++r) c += q.w[r] * e[r] * e[r];
      J += c;
    }
#endif
    typename M::StepCache chain;
#pragma unroll 1
    for (int i = 0; i < n_sub; ++i) plant_sub_step<R, M>(k, fe, i, n_sub, h_last, uu, xs, chain);
    if (xs_out)
#pragma unroll
      for (int r = 0; r < NX; ++r) xs_out[((int64_t)t * NX + r) * B + p] = xs[r];
  }
#if !CPMPC_ROLL_SEARCH
  if (x_final)
#pragma unroll
    for (int r = 0; r < NX; ++r) x_final[r * B + p] = xs[r];
#endif
#if CPMPC_ROLL_COST
  {  // the terminal cost
    constexpr int NH = tri(NX, 0);
    R e[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) e[r] = xs[r] - xs_ref[((int64_t)(T - 1) * NX + r) * B + p];
    wrap_residual<R, M>(e);
    R Pm[NH];
#pragma unroll
    for (int j = 0; j < NX; ++j)
#pragma unroll
      for (int kk = 0; kk <= j; ++kk) Pm[tri(j, kk)] = PT ? PT[(j * NX + kk) * B + p] : (kk == j ? qfv[j] : R(0));
    J += ilqr_quad_tri<R, NX>(Pm, e);
  }
#endif
#if CPMPC_ROLL_SEARCH
    // alpha is a power of two, so both products of pred are exact and pred rounds once, contracted or not.  The two sides of
    // the test are a difference and a product of values already rounded, each rounded on its own: nothing there can contract
    const R pred = dV1 * alpha + dV2 * alpha * alpha;
    const R gain = J - J_nom, bound = armijo * pred;
    accepted = pred < R(0) && gain <= bound;
    if (accepted) break;
    alpha *= R(0.5);
  }
  if (!accepted) {  // no step: the nominal comes back by copy (a NaN in kff, K or dV has failed the lane, not poisoned it)
    if (us_out)
#pragma unroll 1
      for (int t = 0; t < T; ++t) us_out[(int64_t)t * B + p] = u_nom[(int64_t)t * B + p];
    if (xs_out)
#pragma unroll 1
      for (int64_t i = 0; i < (int64_t)T * NX; ++i) xs_out[i * B + p] = xs_nom[i * B + p];
#pragma unroll
    for (int r = 0; r < NX; ++r) xs[r] = xs_nom[((int64_t)(T - 1) * NX + r) * B + p];
    J = J_nom;
    alpha = R(0);
  }
  if (alpha_out) alpha_out[p] = alpha;
  if (x_final)
#pragma unroll
    for (int r = 0; r < NX; ++r) x_final[r * B + p] = xs[r];
#endif
#if CPMPC_ROLL_COST
  if (cost_out) cost_out[p] = J;
#endif
#undef CPMPC_ROLL_LAW
#undef CPMPC_ROLL_COST
#undef CPMPC_ROLL_SEARCH
