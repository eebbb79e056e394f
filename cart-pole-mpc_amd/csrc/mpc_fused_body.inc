// mpc_fused_body.inc -- the body of the fused SQP kernel, included by mpc_fused.hpp once with the spacing SP a
// compile-time constant and the LDS arrays static (the tuned variants), once with SP = a.SP at run time and the same
// arrays carved from dynamic LDS.  Expects: R, M, L, SHARED, NX, PPW, SP, lds_u, lds_du, lds_G, lds_gw, lds_id (or the slim
// layout's CPMPC_ID_SET / CPMPC_ID_GET on registers and lds_gw aliased to lds_du), CPMPC_SWEEP_PRAGMA, a,
// max_iters in scope and CPMPC_FUSED_MAT2_POW(matrix, exponent) defined; REFINE (bool): the double kernels' full refinement.
  using W = typename WideOf<R>::type;  // the type the terminal Schur complement is carried in (wide.hpp)
  // column i of my Gamma_s: lds_G is an array of 16-byte (8-byte: float / NX = 6) pieces, piece p of column i at
  // [(i * 64 + lane) * fused_g_pieces + p] (fused_g_ld / fused_g_st)
#define G_LD(I) (fused_g_ld<R, NX>(lds_G, (I), lane))
#define G_ST(I, V) (fused_g_st<R, NX>(lds_G, (I), lane, (V)))
  using WO = Wide<W>;
  constexpr bool kWidened = !std::is_same<W, R>::value;
  // Float kernels, REFINE = true (CPMPC_CREATE_WIDE_QP; round 5; compiled specialisations; default for the 6-state model): everything
  // between the linearisation and the multipliers' effect on the step -- the Psi products across the intervals, the columns
  // w_k of W = U^-1 R^T, psi = Psi^T q and y = -(gw + W q) -- is carried in double as well (type Q), not only the NX x NX
  // system.  A CPU model of the elimination (tools/long_horizon_cpu_study.py 40 300 f32) puts the error of one float QP step
  // at 1.3e-4 median / 3e-3 p99 with S in double and 2.3e-5 / 1.6e-4 with these pieces too; on the GPU the headline's cold
  // starts end 8.4e-5 (median) / 4.9e-3 (p99) from the double check instead of 2.4e-4 / 0.11 -- exactly where the float CPU
  // check ends -- for 2.7 % of the kernel's time; for the 6-state model 4.2e-2 / 8.0 -> 5.7e-4 / 9.3e-3 for 0 - 5 % (HISTORY.md).
  // (Only the REFINE instantiation carries it: hipcc 7.2's register allocator crashes on the 4-state run-time-spacing
  // kernel's SHARED = true instantiation with Q = double.)
  constexpr bool kWideQP = REFINE && kWidened;
  using Q = std::conditional_t<kWideQP, W, R>;
  // one step of iterative refinement of the WHOLE QP solution, residuals from the original data (double kernels; see the
  // block after sweep 2)
  constexpr bool kFullRefine = REFINE && sizeof(R) == 8 && !kWidened;
  // Round 6, the 6-state kernels (the double one: 512 registers and 290 spilled dwords in round 5, nearly all of them around the
  // combine step below): the terminal system S = sum_k w_k w_k^T / d_k is accumulated from the TRUE columns
  // w_k = Psi_s wt_k + e_k w_in in a second pass down the block after the boundary chain, instead of as the block-local Gram
  // matrix St of the wt_k in the first pass and the congruence Psi St Psi^T + corrections after it.  Same multiply-adds
  // (84 against 87 per control), but St, Psi St (2 x NX x NX) and the t~, r~, eps, sigma sums never exist: the peak of live
  // values falls by ~90 doubles: 9.7 % of the fp64 kernel time.  The 4-state and full-refinement kernels keep the one pass.
  // structural zeros of Phi and Psi (models.hpp: struct_zero): entries of the columns of a step Jacobian that are known in
  // closed form; SZ(r, c) is false everywhere for a model without such columns (the 4-state one)
  constexpr unsigned kTriv = trivial_cols<NX, M::NQ>(JaZeroCols<M>::value);
#define SZ(r_, c_) (struct_zero<NX, M::NQ>(kTriv, (r_), (c_)))
  constexpr bool kTwoPass = NX > 4 && !kFullRefine;
  // Round 7, the float 4-state kernels (two waves per SIMD): a control that a loop over the block's steps reads from LDS is
  // read one step ahead, under the RK4 step before it, instead of being waited for a few instructions after the read is
  // issued -- the linearisation's u and the line search's trial control (DESIGN.md section 5b).  Same values, same
  // operations in the same order: results keep their bits (tests/test_gpu_fused_lds_order.py).  The double and 6-state
  // kernels (one wave per SIMD, at their register limit) keep the order they had.
  constexpr bool kUAhead = sizeof(R) == 4 && NX <= 4;
  CPMPC_TICK_INIT();
  CPMPC_CLOCK_BEGIN();
  const int lane = threadIdx.x;
  const int s = lane % L;            // my shooting interval
  const int gbase = lane - s;        // first lane of my group
  int64_t pp = (int64_t)blockIdx.x * PPW + lane / L;
  const bool in_group = lane / L < PPW;  // 64 % L lanes at the end of the wave hold no whole group: they ride along
  if (!in_group) pp = (int64_t)blockIdx.x * PPW;
  bool valid;
  int budget = max_iters;            // SQP iterations of this launch
  if (a.active_list != nullptr) {    // a later stage: my problem comes from the compacted list of active ones
    const int64_t n_active = *a.active_count;
    if ((int64_t)blockIdx.x * PPW >= n_active) return;  // block-uniform: nothing left for this wave
    valid = in_group && pp < n_active;
    pp = a.active_list[valid ? pp : n_active - 1];
    // once the active set fits one round of resident waves, further compaction cannot shorten anything: finish
    // here (every problem stops at its own iteration cap), the stages still to come find an empty list
    if (n_active <= a.run_out_below) budget = a.iter_cap;
    // likewise when hardly anybody has stopped since the previous compaction and little is left to run (a cold
    // start with few iterations): another stage would cost a launch and buy nothing
    const int64_t n_prev = a.prev_count ? (int64_t)*a.prev_count : a.prev_total;
    if (n_active * 10 >= n_prev * 9 && a.remaining <= (2 * max_iters > 3 ? 2 * max_iters : 3)) budget = a.iter_cap;
  } else {
    valid = in_group && pp < a.B;
    if (pp >= a.B) pp = a.B - 1;     // compute redundantly, never store: keeps the shuffles well defined
  }
  const unsigned p = (unsigned)pp;
  const int64_t st = a.stride;
  const int N = a.N;
  typename M::Consts k_lane;
  if constexpr (!SHARED) k_lane = load_consts(a, p);
  const typename M::Consts& k = SHARED ? a.consts : k_lane;
  const ExtForce<R> fe{R(0), R(0), R(0)};
  const R wu2 = a.wu * a.wu, wd2 = a.wd * a.wd;

  // ---- per-problem state, replicated in the L lanes of the group -------------------------------------
  int status = a.ist[IS_STATUS * st + p];
  if (!in_group) status = kTermMaxIterations;  // riding lanes never keep the wave's loops alive (and never store)
  int iters = a.ist[IS_ITERS * st + p], evals_tot = a.ist[IS_LS_EVALS * st + p], failed = a.ist[IS_FAILED * st + p];
  R lam = a.sc[SC_LAMBDA * st + p], mu = a.sc[SC_MU * st + p], a_start = a.sc[SC_ALPHA * st + p];
  R f_last = a.sc[SC_F_LAST * st + p], cn_last = a.sc[SC_CN_LAST * st + p];
  bool have_trial = a.sc[SC_TRIAL * st + p] != R(0);  // f_last / cn_last are the line search's evaluation of this iterate
  const R u_prev = a.sc[SC_UPREV * st + p];
  R tgt[NX], xm[NX], Rw[NX], Dg[NX];  // (Dg is dead after the next few lines when kDgMask: the compiler drops it)
#pragma unroll
  for (int t = 0; t < NX; ++t) {
    tgt[t] = a.term_tgt[t];
    xm[t] = a.x0[t * a.B + p];
  }
  load_terminal<R, M>(a, p, Rw, Dg);
  // which terminal rows are cost rows, as one bit mask instead of NX 0 / 1 values held in registers for the whole launch
  // (the double 6-state kernel: 12 fewer persistent registers, 173 -> 132 spilled dwords, 2.5 % of its time)
  constexpr bool kDgMask = NX > 4 && sizeof(R) == 8;
  int dgm = 0;
  if constexpr (kDgMask) {
#pragma unroll
    for (int t = 0; t < NX; ++t) dgm |= (Dg[t] != R(0)) ? (1 << t) : 0;
  }
#define IS_COST(t_) (kDgMask ? (((dgm >> (t_)) & 1) != 0) : (Dg[t_] != R(0)))
  if (a.set_point) tgt[0] = a.set_point[p];

  // ---- my piece of the iterate --------------------------------------------------------------------------
  R xs[NX], xe[NX];  // node s, node s+1 (a copy, or the terminal node itself for s = L-1)
  unpack<R, NX>(a.zx[(int64_t)s * st + p], xs);
  unpack<R, NX>(a.zx[(int64_t)(s + 1) * st + p], xe);
#pragma unroll
  for (int i = 0; i < SP; ++i) lds_u[i * 64 + lane] = a.zu[(int64_t)(s * SP + i) * st + p];

  for (int it = 0; it < budget; ++it) {
    const bool live = (status == kTermNone) && (iters < a.iter_cap);  // frozen once terminated or at max_iterations
    if (!__any(live)) break;

    CPMPC_TICK(7);
    // ================= linearise my interval (optimization.cc:99-160) ==================================
    R Phi[NX][NX], cdef[NX];
    {
      R x[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        x[r] = xs[r];
#pragma unroll
        for (int c = 0; c < NX; ++c) Phi[r][c] = (r == c) ? R(1) : R(0);
      }
      typename M::StepCache chain;  // what the stages of a step share (models.hpp)
      {
        // kUAhead: the control of step i + 1 is read under step i's RK4 (the last step reads its own again: no branch)
        R u_lin = R(0);
        if constexpr (kUAhead) u_lin = lds_u[0 * 64 + lane];
#pragma unroll 1
        for (int i = 0; i < SP; ++i) {
          R u;
          if constexpr (kUAhead) {
            u = u_lin;
            u_lin = lds_u[((i + 1 < SP) ? i + 1 : i) * 64 + lane];
          } else {
            u = lds_u[i * 64 + lane];
          }
          R A[NX][NX], Bv[NX];
          rk4_step_jac_m<R, M, false>(k, a.dt, x, u, fe, A, Bv, chain);
          if constexpr (JaZeroCols<M>::value != 0u) {
            // Phi <- A Phi a column at a time through step_jac_apply (models.hpp): the columns of A that are known in closed
            // form are not multiplied through
  #pragma unroll
            for (int c = 0; c < NX; ++c) {
              if ((kTriv >> c) & 1u) continue;  // stays e_c (+ t e_{c-NQ}): written once, after the loop
              R col[NX], ncol[NX];
  #pragma unroll
              for (int r = 0; r < NX; ++r) col[r] = Phi[r][c];
              step_jac_apply<R, M>(A, a.dt, col, ncol);
  #pragma unroll
              for (int r = 0; r < NX; ++r) Phi[r][c] = ncol[r];
            }
          } else {
          R T[NX][NX];
  #pragma unroll
          for (int r = 0; r < NX; ++r)
  #pragma unroll
            for (int c = 0; c < NX; ++c) {
              R acc = A[r][0] * Phi[0][c];
  #pragma unroll
              for (int m = 1; m < NX; ++m) acc += A[r][m] * Phi[m][c];
              T[r][c] = acc;
            }
  #pragma unroll
          for (int r = 0; r < NX; ++r)
  #pragma unroll
            for (int c = 0; c < NX; ++c) Phi[r][c] = T[r][c];
          }
          // Gamma_j <- A Gamma_j for the earlier controls, Gamma_i = B (forward accumulation, in LDS)
          if constexpr (sizeof(R) == 8) {
            // one column ahead: the read of column j+1 is in flight while column j is multiplied -- with one wave per
            // SIMD, the fp64 case, nothing else covers the LDS round trip of a read that is used at once (with two waves
            // the other one does, and the extra branch and move per column cost fp32 1.5 %)
            XV<R, NX> g_next = G_LD(0);  // column 0 (stale and unused when i = 0)
  #pragma unroll 1
            for (int j = 0; j < i; ++j) {
              R g[NX], gn[NX];
              unpack<R, NX>(g_next, g);
              if (j + 1 < i) g_next = G_LD(j + 1);
              if constexpr (JaZeroCols<M>::value != 0u) {
                step_jac_apply<R, M>(A, a.dt, g, gn);
              } else {
  #pragma unroll
              for (int r = 0; r < NX; ++r) {
                R acc = A[r][0] * g[0];
  #pragma unroll
                for (int m = 1; m < NX; ++m) acc += A[r][m] * g[m];
                gn[r] = acc;
              }
              }
              G_ST(j, (pack<R, NX>(gn)));
            }
          } else {
  #pragma unroll 1
            for (int j = 0; j < i; ++j) {
              R g[NX], gn[NX];
              unpack<R, NX>(G_LD(j), g);
              if constexpr (JaZeroCols<M>::value != 0u) {
                step_jac_apply<R, M>(A, a.dt, g, gn);
              } else {
  #pragma unroll
              for (int r = 0; r < NX; ++r) {
                R acc = A[r][0] * g[0];
  #pragma unroll
                for (int m = 1; m < NX; ++m) acc += A[r][m] * g[m];
                gn[r] = acc;
              }
              }
              G_ST(j, (pack<R, NX>(gn)));
            }
          }
          G_ST(i, (pack<R, NX>(Bv)));
        }
      }
      // the columns of Phi that are known in closed form after SP steps of size h: e_c, and SP h in row c - NQ of a velocity
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (((kTriv >> c) & 1u) && c >= M::NQ) Phi[c - M::NQ][c] = R(SP) * a.dt;
      wrap_angles<R, M>(x);
#pragma unroll
      for (int t = 0; t < NX; ++t) cdef[t] = x[t] - xe[t];
      wrap_angles<R, M>(cdef);
    }

    CPMPC_TICK(0);
    // neighbours' boundary controls (u_{k-1} of my first control, u_{k+1} of my last one)
    const R u_first = lds_u[0 * 64 + lane], u_last = lds_u[(SP - 1) * 64 + lane];
    R u_left = lane_left<R, L>(u_last);
    if (s == 0) u_left = u_prev;
    const R u_right = lane_right<R, L>(u_first);  // unused for s = L-1

    // ================= block-parallel sweeps ===============================================================
    // All three sweeps of the structured QP are linear recurrences in k, so every lane first solves its own
    // block in block-local coordinates (carry-in = 0) together with the scalar chain e_k that says how a
    // carry-in would propagate; a short chain over the L lanes then fixes the true block-boundary values and
    // each lane corrects its block locally:
    //     w_k  = Psi_s wt_k + e_k w_in,      gw_k = gwt_k + e_k gw_in,      e_k = -ups_k e_{k+1}
    //     wt_k = Gamma_k - ups_k wt_{k+1},   gwt_k = g_k - ups_k gwt_{k+1}  (wt, gwt = 0 and e = 1 past the block)
    // with Psi_s = diag(w) Phi_{S-2} ... Phi_{s+1} constant inside a block.

    // ---- pivots d_k = diag_k - wd2^2 / d_{k+1} of T = U D U^T ---------------------------------------------------
    // They depend on (lambda, weights) only.  Scaled by b = wu2 + lambda + 2 wd2 the recurrence is the Moebius map
    //     delta_k = 1 - gamma / delta_{k+1},   gamma = (wd2 / b)^2 <= 1/4,   delta_{N-1} = (b - wd2) / b
    // i.e. (p, q)_k = [[1, -gamma], [1, 0]] (p, q)_{k+1} with delta = p / q: a constant 2x2 matrix whose powers
    // (by squaring; all entries stay <= 1) jump straight to the block boundaries, so no lane walks the whole
    // horizon: each one starts its own SP pivots from its boundary value inside the sweep-1 pass below.
    R id_right = R(0);  // 1/d of the first control after my block (unused for s = L-1)
    {
      const R bdiag = wu2 + lam + R(2) * wd2;
      const R rb = Math<R>::div(R(1), bdiag);
      const R gam = (wd2 * rb) * (wd2 * rb);
      const Mat2<R> Tm{R(1), -gam, R(1), R(0)};
      const Mat2<R> Tsp = CPMPC_FUSED_MAT2_POW(Tm, SP);
      const Mat2<R> Tsp1 = CPMPC_FUSED_MAT2_POW(Tm, SP - 1);
      // (p, q) at the first control of the last block, then one block further down per step
      R pq0 = Tsp1.a * ((bdiag - wd2) * rb) + Tsp1.b;
      R pq1 = Tsp1.c * ((bdiag - wd2) * rb) + Tsp1.d;
      R myp = R(1), myq = R(0);
#pragma unroll
      for (int sb = L - 2; sb >= 0; --sb) {
        if (sb == s) {
          myp = pq0;
          myq = pq1;
        }
        const R n0 = Tsp.a * pq0 + Tsp.b * pq1;
        const R n1 = Tsp.c * pq0 + Tsp.d * pq1;
        // delta = p / q is scale invariant: renormalise, or (p, q) ~ 2^-k would leave the fp32 range on long horizons
        pq0 = n0 * Math<R>::rcp(n1);
        pq1 = R(1);
      }
      id_right = Math<R>::div(myq * rb, myp);  // 1 / (b delta)
    }
    bool pd_ok = true;

    CPMPC_TICK(1);
    // ---- sweep 1, local pass down my block ---------------------------------------------------------------
    W Sm[NX][NX], rho[NX], ha[NX];  // everything that feeds the NX x NX terminal system is carried in W (wide.hpp)
    // kept for the full refinement (dead otherwise): Psi t~ and eps of the combine, the LDL^T factors
    W PT_keep[NX], eps_keep = WO::of(R(0)), Lm_keep[NX][NX], idv_keep[NX];
    R f_part = R(0), cn_part = R(0);
    Q wt[NX];
    R gwt = R(0), e_blk = R(1);  // after the pass: wt_0, gwt_0, e_0 of my block
    Q Psi[NX][NX], w_in[NX];
    R gw_in = R(0);  // my block's carry-in (exact after the boundary chain)
    R ci[NX], e_term[NX];
    {
      W St[NX][NX], tt[NX], rr[NX], eps = WO::of(R(0)), sig = WO::of(R(0));
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        wt[i] = Q(0);
        tt[i] = WO::of(R(0));
        rr[i] = WO::of(R(0));
#pragma unroll
        for (int j = 0; j < NX; ++j) St[i][j] = WO::of(R(0));
      }
      R u_hi = u_right;
      R u_cur = lds_u[(SP - 1) * 64 + lane];
      R idn = id_right;
CPMPC_SWEEP_PRAGMA
      for (int i = SP - 1; i >= 0; --i) {
        CPMPC_SWEEP_FENCE();
        const int kk = s * SP + i;
        const R u_lo = (i > 0) ? lds_u[(i - 1) * 64 + lane] : u_left;
        const R ru = a.wu * u_cur, rd = a.wd * (u_lo - u_cur);
        f_part += ru * ru + rd * rd;
        R g = wu2 * u_cur + wd2 * (u_cur - u_lo);
        if (kk < N - 1) g += wd2 * (u_cur - u_hi);
        const R ups = (kk < N - 1) ? (-wd2 * idn) : R(0);
        const R dk = (wu2 + lam + wd2 * ((kk < N - 1 ? R(1) : R(0)) + R(1))) + wd2 * ups;
        if (!(dk > R(0))) pd_ok = false;
        const R idk = Math<R>::rcp(dk);
        CPMPC_ID_SET(i, idk);
        R Gi[NX];
        unpack<R, NX>(G_LD(i), Gi);
#pragma unroll
        for (int r = 0; r < NX; ++r) wt[r] = Q(Gi[r]) - Q(ups) * wt[r];
        gwt = g - ups * gwt;
        e_blk = -ups * e_blk;
        lds_gw[i * 64 + lane] = gwt;  // (the du slot when the layout is lean: du of the last iteration is dead by now)
        // the products are exact in W (float x float fits a double, double x double by fma), so the sums are those of
        // the Gram matrix of the rounded columns to the precision of W
        if constexpr (!kTwoPass) {
        const W ei = WO::prod(e_blk, idk);
        eps += ei * e_blk;
        sig += ei * gwt;
#pragma unroll
        for (int i2 = 0; i2 < NX; ++i2) {
          const W wi = (W)wt[i2] * (W)idk;
          tt[i2] += wi * e_blk;
          rr[i2] += wi * gwt;
#pragma unroll
          for (int j2 = 0; j2 <= i2; ++j2) St[i2][j2] += wi * wt[j2];
        }
        }
        idn = idk;
        u_hi = u_cur;
        u_cur = u_lo;
      }
#pragma unroll
      for (int t = 0; t < NX; ++t) cn_part += Math<R>::fabs(cdef[t]);

      CPMPC_TICK(2);
      // ---- initial-state residual (node 0) and terminal residual (node S-1), replicated ---------------------
      {
        R x0n[NX], xT[NX];
#pragma unroll
        for (int t = 0; t < NX; ++t) {
          x0n[t] = group_first<R, L>(xs[t], gbase);
          xT[t] = group_last<R, L>(xe[t], gbase);
          ci[t] = x0n[t] - xm[t];
          e_term[t] = xT[t] - tgt[t];
        }
        wrap_angles<R, M>(ci);
        wrap_angles<R, M>(e_term);
      }
      // ---- boundary chain, down the lanes: Psi_s, w_in, gw_in ---------------------------------------------
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        w_in[r] = Q(0);
#pragma unroll
        for (int c = 0; c < NX; ++c) Psi[r][c] = (r == c) ? Q(Rw[r]) : Q(0);
      }
#pragma unroll 1
      for (int round = 0; round + 1 < L; ++round) {
        // my block's values at its first control, from my current carry-in (exact once the carry-in is)
        const bool edge = (s == L - 1);
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          Q wo = Q(e_blk) * w_in[r];
#pragma unroll
          for (int m = 0; m < NX; ++m)
            if (!SZ(r, m)) wo += Psi[r][m] * wt[m];
          const Q v = lane_right<Q, L>(wo);
          w_in[r] = edge ? w_in[r] : v;
        }
        {
          const R v = lane_right<R, L>(gwt + e_blk * gw_in);
          gw_in = edge ? gw_in : v;
        }
        Q T[NX][NX];
#pragma unroll
        for (int r = 0; r < NX; ++r)
#pragma unroll
          for (int c = 0; c < NX; ++c) {
            if (SZ(r, c)) continue;  // an exact zero of the product: Psi keeps the 0 it was given
            bool have = false;
            Q acc = Q(0);
#pragma unroll
            for (int m = 0; m < NX; ++m) {
              if (SZ(r, m) || SZ(m, c)) continue;
              acc = have ? acc + Psi[r][m] * Q(Phi[m][c]) : Psi[r][m] * Q(Phi[m][c]);
              have = true;
            }
            T[r][c] = acc;
          }
#pragma unroll
        for (int r = 0; r < NX; ++r)
#pragma unroll
          for (int c = 0; c < NX; ++c) {
            if (SZ(r, c)) continue;
            const Q v = lane_right<Q, L>(T[r][c]);
            Psi[r][c] = edge ? Psi[r][c] : v;
          }
      }
      // ---- combine: S_s = sum_k w_k w_k^T / d_k,  rho_s = sum_k w_k gw_k / d_k,  ha_s = Psi_s c_s ----------------
      {
        R hvv[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          bool have = false;
          R acc = R(0);
#pragma unroll
          for (int m = 0; m < NX; ++m) {
            if (SZ(r, m)) continue;
            acc = have ? acc + Phi[r][m] * ci[m] : Phi[r][m] * ci[m];
            have = true;
          }
          hvv[r] = cdef[r] - ((s == 0) ? acc : R(0));  // dx_0 = -c_init enters through interval 0
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          bool have = false;
          W acc = WO::of(R(0));
#pragma unroll
          for (int m = 0; m < NX; ++m) {
            if (SZ(r, m)) continue;
            acc = have ? acc + (W)Psi[r][m] * (W)hvv[m] : (W)Psi[r][m] * (W)hvv[m];
            have = true;
          }
          ha[r] = acc;
        }
      }
      if constexpr (kTwoPass) {
        // second pass down my block with the exact carry-ins: w_k = Psi_s wt_k + e_k w_in, gw_k = gwt_k + e_k gw_in
        Q wt2[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          wt2[i] = Q(0);
          rho[i] = WO::of(R(0));
#pragma unroll
          for (int j = 0; j <= i; ++j) Sm[i][j] = WO::of(R(0));
        }
        R e2 = R(1), idn2 = id_right;
CPMPC_SWEEP_PRAGMA
        for (int i = SP - 1; i >= 0; --i) {
          CPMPC_SWEEP_FENCE();
          const int kk = s * SP + i;
          const R idk = CPMPC_ID_GET(i);
          const R ups = (kk < N - 1) ? (-wd2 * idn2) : R(0);
          R Gi[NX];
          unpack<R, NX>(G_LD(i), Gi);
#pragma unroll
          for (int r = 0; r < NX; ++r) wt2[r] = Q(Gi[r]) - Q(ups) * wt2[r];
          e2 = -ups * e2;
          const R gwk = lds_gw[i * 64 + lane] + e2 * gw_in;
          // (in Q: a float kernel without the wide QP forms the column in float and S is the Gram matrix of the ROUNDED columns,
          //  exact products in W = double: positive semi-definite by construction, wide.hpp)
          W wk[NX];
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            Q acc = Q(e2) * w_in[r];
#pragma unroll
            for (int m = 0; m < NX; ++m)
              if (!SZ(r, m)) acc += Psi[r][m] * wt2[m];
            wk[r] = (W)acc;
          }
#pragma unroll
          for (int i2 = 0; i2 < NX; ++i2) {
            const W wi = wk[i2] * (W)idk;
            rho[i2] += wi * gwk;
#pragma unroll
            for (int j2 = 0; j2 <= i2; ++j2) Sm[i2][j2] += wi * wk[j2];
          }
          idn2 = idk;
        }
      } else {
      W PT[NX], PS[NX][NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        W acc = Psi[i][0] * tt[0];
        W acr = Psi[i][0] * rr[0];
#pragma unroll
        for (int m = 1; m < NX; ++m) {
          acc += Psi[i][m] * tt[m];
          acr += Psi[i][m] * rr[m];
        }
        PT[i] = acc;
        rho[i] = acr + acc * gw_in + w_in[i] * (sig + eps * gw_in);
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          W v = Psi[i][0] * (j <= 0 ? St[0][j] : St[j][0]);
#pragma unroll
          for (int m = 1; m < NX; ++m) v += Psi[i][m] * (j <= m ? St[m][j] : St[j][m]);
          PS[i][j] = v;
        }
      }
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          W v = PS[i][0] * Psi[j][0];
#pragma unroll
          for (int m = 1; m < NX; ++m) v += PS[i][m] * Psi[j][m];
          Sm[i][j] = v + PT[i] * w_in[j] + w_in[i] * (PT[j] + eps * w_in[j]);
        }
      if constexpr (kFullRefine) {
#pragma unroll
        for (int i = 0; i < NX; ++i) PT_keep[i] = PT[i];
        eps_keep = eps;
      }
      }
    }

    CPMPC_TICK(3);
    // ---- group sums, terminal rows ------------------------------------------------------------------------
    R f = group_sum<R, L>(f_part), cn = group_sum<R, L>(cn_part);
    pd_ok = (group_sum<R, L>(pd_ok ? R(0) : R(1)) == R(0));  // every lane checked the pivots of its own block
    W hv[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      rho[i] = group_sum<W, L>(rho[i]);
      hv[i] = group_sum<W, L>(ha[i]);
#pragma unroll
      for (int j = 0; j <= i; ++j) Sm[i][j] = group_sum<W, L>(Sm[i][j]);
    }
#pragma unroll
    for (int t = 0; t < NX; ++t) {
      cn += Math<R>::fabs(ci[t]);
      if (IS_COST(t)) {
        const R r = Rw[t] * e_term[t];
        f += r * r;
      } else {
        cn += Math<R>::fabs(e_term[t]);
      }
      hv[t] += WO::prod(Rw[t], e_term[t]);
    }
    f *= R(0.5);
    if (live && (!Math<R>::finite(f) || !Math<R>::finite(cn))) status = kTermNonFinite;
    // The merit at the iterate, evaluated the way the trials are (see qp_ls_kernel): the iterate is the last accepted
    // trial point bit for bit, so phi_0 takes that trial's own f and |c|_1 instead of the linearisation's
    if (have_trial) {
      f = f_last;
      cn = cn_last;
    }

    // ================= NX x NX LDL^T (every lane of the group, identical inputs) ==========================
    Q q[NX];
    {
      W Lm[NX][NX], dv[NX], idv[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) Sm[i][i] += kDgMask ? (IS_COST(i) ? WO::of(R(1)) : WO::of(R(0))) : WO::of(Dg[i]);
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        W dj = Sm[j][j];
#pragma unroll
        for (int m = 0; m < j; ++m) dj -= Lm[j][m] * Lm[j][m] * dv[m];
        if (!(dj > W(0))) pd_ok = false;
        dv[j] = dj;
        const W inv = wide_inv<R, W>(dj);
        idv[j] = inv;
#pragma unroll
        for (int i = j + 1; i < NX; ++i) {
          W v = Sm[i][j];
#pragma unroll
          for (int m = 0; m < j; ++m) v -= Lm[i][m] * Lm[j][m] * dv[m];
          Lm[i][j] = v * inv;
        }
      }
      // L D L^T x = b
      auto ldl_solve = [&](const W (&b)[NX], W (&x)[NX]) {
        W y[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          W v = b[i];
#pragma unroll
          for (int m = 0; m < i; ++m) v -= Lm[i][m] * y[m];
          y[i] = v;
        }
#pragma unroll
        for (int i = NX - 1; i >= 0; --i) {
          W v = y[i] * idv[i];
#pragma unroll
          for (int m = i + 1; m < NX; ++m) v -= Lm[m][i] * x[m];
          x[i] = v;
        }
      };
      if constexpr (kFullRefine) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          idv_keep[i] = idv[i];
#pragma unroll
          for (int j = 0; j < i; ++j) Lm_keep[i][j] = Lm[i][j];
        }
      }
      W rhs[NX], qw[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) rhs[i] = hv[i] - rho[i];
      ldl_solve(rhs, qw);
#pragma unroll
      for (int i = 0; i < NX; ++i) q[i] = (Q)qw[i];
      // ---- one step of iterative refinement of q, the residual taken through the FACTORED operator ----------
      // S = W^T D^-1 W is a normal-equations matrix: forming it squares the conditioning of the terminal
      // sensitivities (measured on the benchmark distribution: the step du from the formed S is 20-40x less accurate
      // in the tail than a dense KKT solve with pivoting, 2e-9 against 6e-11).  The residual
      //     r = (h - rho) - Dg q - sum_k w_k (w_k . q) / d_k
      // evaluated term by term from the columns (never through the rounded S) recovers that: one correction
      // solve with the same factors brings du to 4e-12.  w_k . q = psi . wt_k + e_k (w_in . q) as in sweep 1b.
      // Horizons of more than four intervals (L = 8, 16: the states are eliminated through up to 1.6 s of an unstable
      // plant) take a second pass: one lane in a hundred at N = 160 was still 2e-5 from a full-space KKT solve with pivoting.
      // The float kernels carry the system in double (kWidened, wide.hpp), so the rounding of S the pass repairs is gone
      // there and they leave it out (round 4: median gap to the fp64 solve 2.44e-4 without it, 2.61e-4 with it).
      constexpr int kRefinePasses = kWidened ? 0 : (sizeof(R) == 8 && L > 4 ? 2 : 1);
#pragma unroll 1
      for (int refine = 0; refine < kRefinePasses; ++refine) {
        R psi[NX], wq_in = R(0);
#pragma unroll
        for (int c = 0; c < NX; ++c) {
          bool have = false;
          R acc = R(0);
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            if (SZ(r, c)) continue;
            acc = have ? acc + Psi[r][c] * q[r] : Psi[r][c] * q[r];
            have = true;
          }
          psi[c] = acc;
          wq_in += w_in[c] * q[c];
        }
        R wv[NX], acc_t[NX], acc_e = R(0), om = R(0), e = R(1);
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          wv[r] = R(0);
          acc_t[r] = R(0);
        }
        R idn = id_right;
CPMPC_SWEEP_PRAGMA
        for (int i = SP - 1; i >= 0; --i) {
          CPMPC_SWEEP_FENCE();
          const int kk = s * SP + i;
          R Gi[NX];
          unpack<R, NX>(G_LD(i), Gi);
          const R idk = CPMPC_ID_GET(i);
          const R ups = (kk < N - 1) ? (-wd2 * idn) : R(0);
          R pg = psi[0] * Gi[0];
#pragma unroll
          for (int m = 1; m < NX; ++m) pg += psi[m] * Gi[m];
          om = pg - ups * om;   // psi . wt_k
          e = -ups * e;         // e_k
          const R t = (om + e * wq_in) * idk;  // (w_k . q) / d_k
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            wv[r] = Gi[r] - ups * wv[r];  // wt_k
            acc_t[r] += wv[r] * t;
          }
          acc_e += e * t;
          idn = idk;
        }
        W rq[NX], dq[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          R v = w_in[r] * acc_e;
#pragma unroll
          for (int m = 0; m < NX; ++m)
            if (!SZ(r, m)) v += Psi[r][m] * acc_t[m];
          rq[r] = rhs[r] - (kDgMask ? (IS_COST(r) ? (W)q[r] : WO::of(R(0))) : (W)Dg[r] * (W)q[r]) - WO::of(group_sum<R, L>(v));
        }
        ldl_solve(rq, dq);
#pragma unroll
        for (int r = 0; r < NX; ++r) q[r] = (R)(WO::of(q[r]) + dq[r]);  // the residual was that of the ROUNDED q
      }
    }
    if (live && status == kTermNone && !pd_ok) status = kTermQpIndefinite;

    // ================= sweep 1b, local pass down my block: v_k = -(gw_k + w_k . q) / d_k ====================
    //   w_k . q = psi . wt_k + e_k (w_in . q),  psi = Psi_s^T q,  and  psi . wt_k  obeys wt's recurrence, so W is
    //   never stored.  v_k is parked in lds_du[k]; sweep 2 turns it into du_k in place.
    {
      Q psi[NX];
      Q om_in = Q(gw_in);  // gw_in + w_in . q: what a unit of e_k carries into (gw_k + w_k . q)
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        bool have = false;
        Q acc = Q(0);
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          if (SZ(r, c)) continue;
          acc = have ? acc + Psi[r][c] * q[r] : Psi[r][c] * q[r];
          have = true;
        }
        psi[c] = acc;
        om_in += w_in[c] * q[c];
      }
      Q om = Q(0);
      R e = R(1);
      R idn = id_right;
CPMPC_SWEEP_PRAGMA
      for (int i = SP - 1; i >= 0; --i) {
        CPMPC_SWEEP_FENCE();
        const int kk = s * SP + i;
        R Gi[NX];
        unpack<R, NX>(G_LD(i), Gi);
        Q pg = psi[0] * Q(Gi[0]);
#pragma unroll
        for (int m = 1; m < NX; ++m) pg += psi[m] * Q(Gi[m]);
        const R idk = CPMPC_ID_GET(i);
        const R ups = (kk < N - 1) ? (-wd2 * idn) : R(0);
        om = pg - Q(ups) * om;
        e = -ups * e;
        lds_du[i * 64 + lane] = (R)(-(Q(lds_gw[i * 64 + lane]) + om + Q(e) * om_in) * Q(idk));
        idn = idk;
      }
    }

    CPMPC_TICK(4);
    // ================= sweep 2, up the blocks: du_k = v_k - ups_{k-1} du_{k-1},  dx_{s+1} = Phi dx_s + Gamma du + c ====
    //   local:  dut_k = v_k - ups_{k-1} dut_{k-1},  et_k = -ups_{k-1} et_{k-1}  (dut = 0, et = 1 before the block),
    //           du_k = dut_k + et_k du_in;  ups_{k-1} = -wd2 / d_k uses my own pivots only
    R dxs[NX], dxe[NX];
    R gd_part = R(0), curv_part = R(0);
    R dz_part = R(0);  // |dz|_inf over my piece of the step (nan_max drops a NaN component: see models.hpp)
    R du_in = R(0);  // du of the control before my block (0 for interval 0: u_prev is fixed)
    {
      R Gt[NX], Ht[NX], dut = R(0), et = R(1);
#pragma unroll
      for (int t = 0; t < NX; ++t) {
        Gt[t] = cdef[t];
        Ht[t] = R(0);
      }
CPMPC_SWEEP_PRAGMA
      for (int i = 0; i < SP; ++i) {
        CPMPC_SWEEP_FENCE();
        const int kk = s * SP + i;
        const R upm = (kk > 0) ? (-wd2 * CPMPC_ID_GET(i)) : R(0);
        dut = lds_du[i * 64 + lane] - upm * dut;
        et = -upm * et;
        lds_du[i * 64 + lane] = dut;
        R Gi[NX];
        unpack<R, NX>(G_LD(i), Gi);
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          Gt[r] += Gi[r] * dut;
          Ht[r] += Gi[r] * et;
        }
      }
      // boundary chain, up the lanes: dx_s and du_in
#pragma unroll
      for (int t = 0; t < NX; ++t) dxs[t] = -ci[t];  // interval 0's start; the others receive theirs below
#pragma unroll 1
      for (int round = 0; round < L; ++round) {
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          R v = Gt[r] + Ht[r] * du_in;
#pragma unroll
          for (int m = 0; m < NX; ++m)
            if (!SZ(r, m)) v += Phi[r][m] * dxs[m];
          dxe[r] = v;
        }
        if (round + 1 < L) {
          const bool edge = (s == 0);
#pragma unroll
          for (int t = 0; t < NX; ++t) {
            const R v = lane_left<R, L>(dxe[t]);
            dxs[t] = edge ? dxs[t] : v;
          }
          const R v1 = lane_left<R, L>(dut + et * du_in);
          du_in = edge ? du_in : v1;
        }
      }
      if constexpr (kFullRefine) {
        // ============ one step of iterative refinement of the whole QP solution =================================
        // State elimination is not backward stable: with weak control costs or long horizons the tail of a batch is
        // 100-1000x less accurate than a full-space KKT solve with pivoting (CPU model, relative error of dz, 150
        // problems each: w_u = 0, w_du = 0.1: 1.6e-10 against 3e-13; w_u = 0.01, w_du = 0: 4.6e-9 against 3e-11), and
        // five SQP iterations on a sensitive cold start amplify that: a fuzz over 200 random problem definitions x
        // 2 048 lanes had the GPU beyond 1e-5 on 18 lanes where the extended-precision arbiter sided with the CPU
        // check.  The cure is the classical one: evaluate the residuals of the QP's optimality conditions at (du, dx) in
        // the ORIGINAL data --
        //     terminal rows      r_T = Rw (dx_T + e_T)                (cost rows: the residual, = their multiplier;
        //                                                              equality rows: the violation)
        //     stationarity       rs  = T du + g + Gamma^T lambda,     lambda_s = Psi_s^T mult  (the adjoint through the
        //                                                              intervals is the Psi_s this lane already holds)
        // -- and solve once more with the factors at hand (same U D U^T, same LDL^T of S): du += ddu, dx += ddx.  That
        // brings the condensed solve BELOW the dense one's error (same CPU model: 3e-14 and 3e-12 worst in the two cases
        // above, 6e-15 against 5e-13 at the reference's weights).  Four more passes over the block's controls, no new
        // factorisation.
        {  // the step so far, materialised: du_k = dut_k + et_k du_in
          R et2 = R(1);
CPMPC_SWEEP_PRAGMA
          for (int i = 0; i < SP; ++i) {
            CPMPC_SWEEP_FENCE();
            const int kk = s * SP + i;
            const R upm = (kk > 0) ? (-wd2 * CPMPC_ID_GET(i)) : R(0);
            et2 = -upm * et2;
            lds_du[i * 64 + lane] += et2 * du_in;
          }
        }
        // a.refine_qp passes (1; 2 beyond the parity horizon, round 6: from the second pass on the refined condensed solve is more
        // accurate than a dense pivoted one on the worst cold starts, DESIGN.md section 8): each pass measures the residuals at
        // the corrected (du, dx, q) and solves once more with the same factors
#pragma unroll 1
        for (int refine_pass = 0; refine_pass < (a.refine_qp > 1 ? a.refine_qp : 1); ++refine_pass) {
        R viol[NX], lamv[NX];
        {
          R mult[NX];
#pragma unroll
          for (int t = 0; t < NX; ++t) {
            const R rT = Rw[t] * (group_last<R, L>(dxe[t], gbase) + e_term[t]);
            const bool cost = IS_COST(t);
            mult[t] = cost ? rT : q[t];
            viol[t] = cost ? R(0) : rT;
          }
#pragma unroll
          for (int c = 0; c < NX; ++c) {
            R acc = Psi[0][c] * mult[0];
#pragma unroll
            for (int r = 1; r < NX; ++r) acc += Psi[r][c] * mult[r];
            lamv[c] = acc;
          }
        }
        // down my block: the stationarity residual of each control and, with it as the gradient, the block-local
        // recurrences of sweep 1 (wt, e as before; gw and the sums that depend on the right-hand side anew)
        R rr2[NX], sig2 = R(0), gwt2 = R(0), e2 = R(1);
        {
          R wt2[NX];
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            wt2[r] = R(0);
            rr2[r] = R(0);
          }
          const R du_right = lane_right<R, L>(lds_du[0 * 64 + lane]);  // first du of the next block (unused for s = L-1)
          R idn = id_right;
          R du_hi = du_right, du_cur = lds_du[(SP - 1) * 64 + lane];
          R u_hi = u_right, u_cur = lds_u[(SP - 1) * 64 + lane];
CPMPC_SWEEP_PRAGMA
          for (int i = SP - 1; i >= 0; --i) {
            CPMPC_SWEEP_FENCE();
            const int kk = s * SP + i;
            const bool inner = kk < N - 1;  // a control after mine exists
            const R du_lo = (i > 0) ? lds_du[(i - 1) * 64 + lane] : du_in;  // (0 before control 0: u_prev is fixed)
            const R u_lo = (i > 0) ? lds_u[(i - 1) * 64 + lane] : u_left;
            R g = wu2 * u_cur + wd2 * (u_cur - u_lo);
            if (inner) g += wd2 * (u_cur - u_hi);
            R Gi[NX];
            unpack<R, NX>(G_LD(i), Gi);
            R rstat = (wu2 + lam + wd2 * ((inner ? R(1) : R(0)) + R(1))) * du_cur - wd2 * du_lo + g;
            if (inner) rstat -= wd2 * du_hi;
#pragma unroll
            for (int m = 0; m < NX; ++m) rstat += Gi[m] * lamv[m];
            const R idk = CPMPC_ID_GET(i);
            const R ups = inner ? (-wd2 * idn) : R(0);
#pragma unroll
            for (int r = 0; r < NX; ++r) wt2[r] = Gi[r] - ups * wt2[r];
            gwt2 = rstat - ups * gwt2;
            e2 = -ups * e2;
            lds_gw[i * 64 + lane] = gwt2;
            sig2 += (e2 * idk) * gwt2;
#pragma unroll
            for (int r = 0; r < NX; ++r) rr2[r] += (wt2[r] * idk) * gwt2;
            idn = idk;
            du_hi = du_cur;
            du_cur = du_lo;
            u_hi = u_cur;
            u_cur = u_lo;
          }
        }
        // boundary chain, down the lanes: the carry-in of gw alone (Psi, w_in and e are those of the first solve)
        R gw_in2 = R(0);
#pragma unroll 1
        for (int round = 0; round + 1 < L; ++round) {
          const R v = lane_right<R, L>(gwt2 + e2 * gw_in2);
          gw_in2 = (s == L - 1) ? gw_in2 : v;
        }
        // (S + Dg) dq = viol - rho', rho' = sum_k w_k gw'_k / d_k, with the LDL^T factors of the first solve
        R dq[NX];
        {
          R y[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) {
            R acr = Psi[i][0] * rr2[0];
#pragma unroll
            for (int m = 1; m < NX; ++m) acr += Psi[i][m] * rr2[m];
            const R rho2 = group_sum<R, L>(acr + PT_keep[i] * gw_in2 + w_in[i] * (sig2 + eps_keep * gw_in2));
            R v = viol[i] - rho2;
#pragma unroll
            for (int m = 0; m < i; ++m) v -= Lm_keep[i][m] * y[m];
            y[i] = v;
          }
#pragma unroll
          for (int i = NX - 1; i >= 0; --i) {
            R v = y[i] * idv_keep[i];
#pragma unroll
            for (int m = i + 1; m < NX; ++m) v -= Lm_keep[m][i] * dq[m];
            dq[i] = v;
          }
        }
        {  // sweep 1b with (gw', dq): v'_k in place of gw'_k
          R psi2[NX], om_in2 = gw_in2;
#pragma unroll
          for (int c = 0; c < NX; ++c) {
            R acc = Psi[0][c] * dq[0];
#pragma unroll
            for (int r = 1; r < NX; ++r) acc += Psi[r][c] * dq[r];
            psi2[c] = acc;
            om_in2 += w_in[c] * dq[c];
          }
          R om = R(0), e = R(1), idn = id_right;
CPMPC_SWEEP_PRAGMA
          for (int i = SP - 1; i >= 0; --i) {
            CPMPC_SWEEP_FENCE();
            const int kk = s * SP + i;
            R Gi[NX];
            unpack<R, NX>(G_LD(i), Gi);
            R pg = psi2[0] * Gi[0];
#pragma unroll
            for (int m = 1; m < NX; ++m) pg += psi2[m] * Gi[m];
            const R idk = CPMPC_ID_GET(i);
            const R ups = (kk < N - 1) ? (-wd2 * idn) : R(0);
            om = pg - ups * om;
            e = -ups * e;
            lds_gw[i * 64 + lane] = -(lds_gw[i * 64 + lane] + om + e * om_in2) * idk;
            idn = idk;
          }
        }
        {  // sweep 2 with v': the correction of the step, then apply it
          R Gt2[NX], Ht2[NX], ddxs[NX], ddxe[NX], dut2 = R(0), et2 = R(1), ddu_in = R(0);
#pragma unroll
          for (int t = 0; t < NX; ++t) {
            Gt2[t] = R(0);
            Ht2[t] = R(0);
            ddxs[t] = R(0);  // dx_0 = -c_init is exact: no correction enters interval 0
          }
CPMPC_SWEEP_PRAGMA
          for (int i = 0; i < SP; ++i) {
            CPMPC_SWEEP_FENCE();
            const int kk = s * SP + i;
            const R upm = (kk > 0) ? (-wd2 * CPMPC_ID_GET(i)) : R(0);
            dut2 = lds_gw[i * 64 + lane] - upm * dut2;
            et2 = -upm * et2;
            lds_gw[i * 64 + lane] = dut2;
            R Gi[NX];
            unpack<R, NX>(G_LD(i), Gi);
#pragma unroll
            for (int r = 0; r < NX; ++r) {
              Gt2[r] += Gi[r] * dut2;
              Ht2[r] += Gi[r] * et2;
            }
          }
#pragma unroll 1
          for (int round = 0; round < L; ++round) {
#pragma unroll
            for (int r = 0; r < NX; ++r) {
              R v = Gt2[r] + Ht2[r] * ddu_in;
#pragma unroll
              for (int m = 0; m < NX; ++m) v += Phi[r][m] * ddxs[m];
              ddxe[r] = v;
            }
            if (round + 1 < L) {
              const bool edge = (s == 0);
#pragma unroll
              for (int t = 0; t < NX; ++t) {
                const R v = lane_left<R, L>(ddxe[t]);
                ddxs[t] = edge ? ddxs[t] : v;
              }
              const R v1 = lane_left<R, L>(dut2 + et2 * ddu_in);
              ddu_in = edge ? ddu_in : v1;
            }
          }
          et2 = R(1);
CPMPC_SWEEP_PRAGMA
          for (int i = 0; i < SP; ++i) {
            CPMPC_SWEEP_FENCE();
            const int kk = s * SP + i;
            const R upm = (kk > 0) ? (-wd2 * CPMPC_ID_GET(i)) : R(0);
            et2 = -upm * et2;
            lds_du[i * 64 + lane] += lds_gw[i * 64 + lane] + et2 * ddu_in;
          }
#pragma unroll
          for (int t = 0; t < NX; ++t) {
            dxs[t] += ddxs[t];
            dxe[t] += ddxe[t];
          }
          du_in += ddu_in;
        }
#pragma unroll
        for (int t = 0; t < NX; ++t) q[t] += dq[t];  // the multipliers the next pass's adjoint starts from
        }
      }
      // local correction du_k = dut_k + et_k du_in, slope and curvature of the control rows
#pragma unroll
      for (int t = 0; t < NX; ++t) {  // |dz|_inf of my piece: both nodes of my interval and (below) my controls
        dz_part = nan_max(dz_part, nan_max(Math<R>::fabs(dxs[t]), Math<R>::fabs(dxe[t])));
      }
      R du_prev = du_in;
      R u_lo = u_left;
      R u_cur = lds_u[0 * 64 + lane];
      et = R(1);
CPMPC_SWEEP_PRAGMA
      for (int i = 0; i < SP; ++i) {
        CPMPC_SWEEP_FENCE();
        const int kk = s * SP + i;
        const R upm = (kk > 0) ? (-wd2 * CPMPC_ID_GET(i)) : R(0);
        et = -upm * et;
        R du;
        if constexpr (kFullRefine) {
          du = lds_du[i * 64 + lane];  // already complete (and refined)
        } else {
          du = lds_du[i * 64 + lane] + et * du_in;
          lds_du[i * 64 + lane] = du;
        }
        dz_part = nan_max(dz_part, Math<R>::fabs(du));
        // control-cost gradient g_k, recomputed from u exactly as in sweep 1
        const R u_hi = (i + 1 < SP) ? lds_u[(i + 1) * 64 + lane] : u_right;
        R g = wu2 * u_cur + wd2 * (u_cur - u_lo);
        if (kk < N - 1) g += wd2 * (u_cur - u_hi);
        gd_part += g * du;
        const R jd = a.wd * (du_prev - du);
        curv_part += wu2 * du * du + jd * jd + lam * du * du;
        du_prev = du;
        u_lo = u_cur;
        u_cur = u_hi;
      }
    }
    R gd = group_sum<R, L>(gd_part), curv = group_sum<R, L>(curv_part);
    const R dz_inf = group_max<R, L>(dz_part);
    {
      R dxT[NX];
#pragma unroll
      for (int t = 0; t < NX; ++t) dxT[t] = group_last<R, L>(dxe[t], gbase);
#pragma unroll
      for (int t = 0; t < NX; ++t) {
        if (IS_COST(t)) {
          const R jd = Rw[t] * dxT[t];
          gd += (Rw[t] * e_term[t]) * jd;
          curv += jd * jd;
        }
      }
    }
    if (live && status == kTermNone && (!Math<R>::finite(gd) || !Math<R>::finite(curv))) status = kTermQpIndefinite;
    // du of my left neighbour's last control, for the (u_{k-1} - u_k) row of my first control
    const R du_left = du_in;

    CPMPC_TICK(5);
    // ================= penalty, merit slope ==================================================================
    if (cn > R(0)) {
      const R mu_req = Math<R>::div(gd + R(0.5) * curv, (R(1) - a.rho) * cn);
      if (mu < mu_req) mu = mu_req;
    }
    const R D = gd - mu * cn;
    const R phi0 = f + mu * cn;
    // equality residuals at the rounding floor of the rollout count as zero in the exit test (DESIGN.md section 4); the
    // size of the states is taken at the terminal node (target and distance to it) times the number of intervals: group-
    // uniform values every lane holds already (a sum over the nodes cost the double kernel 56 more spilled registers, 1.5 %)
    bool first_order;
    // The double kernels leave the floor out: at 3e-14 it could change an exit decision only where |D| is within
    // mu x 3e-14 of the tolerance, and carrying it costs the fp64 fused kernel 1.6 % (4.845 -> 4.925 ms at B = 262 144).
    if constexpr (sizeof(R) == 4) {
      R x_l1 = R(0);
#pragma unroll
      for (int t = 0; t < NX; ++t) x_l1 += Math<R>::fabs(tgt[t]) + Math<R>::fabs(e_term[t]);
      const R D_exit = gd - mu * (cn > a.cn_floor_scale * R(L) * x_l1 ? cn : R(0));
      first_order = Math<R>::fabs(D_exit) < a.fo_tol;
    } else {
      first_order = Math<R>::fabs(D) < a.fo_tol;
    }

    // ================= Armijo line search: every lane rolls out its own interval ============================
    // Local convergence safeguard (DESIGN.md section 4): a QP step that is tiny in every component is taken in full
    // without the merit test
    // (only the undamped step: one that is small because lambda is large is no sign of convergence)
    const bool tiny = dz_inf <= a.full_step_below && lam == R(0);
    // converged (first-order test and a tiny undamped step): the full step, no merit evaluation -- nothing depends on its
    // value any more and it is a whole rollout (DESIGN.md section 4); f_last / cn_last stay those of the iterate the step
    // was computed from.  A wave whose problems are all there skips the line-search loop altogether.
    const bool skip_merit = CPMPC_SKIP_MERIT && tiny && first_order;
    bool active = live && (status == kTermNone) && !skip_merit;
    bool accepted = live && (status == kTermNone) && skip_merit;
    R alpha = tiny ? R(1) : a_start, phi_t = R(0), f_t = f, cn_t = cn;
    int evals = 0;
    for (int t = 0; t < a.max_ls; ++t) {
      if (!__any(active)) break;
      // (inactive groups ride along: their alpha is whatever it was, results are discarded)
      R x[NX], xn[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        x[r] = xs[r] + alpha * dxs[r];
        xn[r] = xe[r] + alpha * dxe[r];
      }
      x[0] = clampr(x[0], -a.bx_lim, a.bx_lim);
      xn[0] = clampr(xn[0], -a.bx_lim, a.bx_lim);
      wrap_angles<R, M>(x);
      wrap_angles<R, M>(xn);
      R fp = R(0), cp = R(0);
      if (s == 0) {  // initial-state rows on the trial node 0
        R d[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) d[r] = x[r] - xm[r];
        wrap_angles<R, M>(d);
#pragma unroll
        for (int r = 0; r < NX; ++r) cp += Math<R>::fabs(d[r]);
      }
      R u_before = (s == 0) ? u_prev : clampr(u_left + alpha * du_left, -a.u_lim, a.u_lim);
      typename M::StepCache chain;
      // kUAhead: the trial control of step i + 1 is read and formed before step i's RK4, as prepare_kernel reads its
      // u_next; the last step forms its own again instead of branching.  (Carrying the two loaded values themselves does
      // not survive the optimiser: it folds a phi of loads back into one load at the top of the step.)
      R u_nx = R(0);
      if constexpr (kUAhead) u_nx = clampr(lds_u[0 * 64 + lane] + alpha * lds_du[0 * 64 + lane], -a.u_lim, a.u_lim);
#pragma unroll 1
      for (int i = 0; i < SP; ++i) {
        R u;
        if constexpr (kUAhead) {
          u = u_nx;
          const int in = (i + 1 < SP) ? i + 1 : i;
          u_nx = clampr(lds_u[in * 64 + lane] + alpha * lds_du[in * 64 + lane], -a.u_lim, a.u_lim);
        } else {
          u = clampr(lds_u[i * 64 + lane] + alpha * lds_du[i * 64 + lane], -a.u_lim, a.u_lim);
        }
        const R ru = a.wu * u, rd = a.wd * (u_before - u);
        fp += ru * ru + rd * rd;
        u_before = u;
        rk4_step_m<R, M, false>(k, a.dt, x, u, fe, chain);
      }
      wrap_angles<R, M>(x);
      {
        R d[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) d[r] = x[r] - xn[r];
        wrap_angles<R, M>(d);
#pragma unroll
        for (int r = 0; r < NX; ++r) cp += Math<R>::fabs(d[r]);
      }
      if (s == L - 1) {  // terminal rows on the trial terminal node
        R d[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) d[r] = xn[r] - tgt[r];
        wrap_angles<R, M>(d);
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          if (IS_COST(r)) {
            const R rr = Rw[r] * d[r];
            fp += rr * rr;
          } else {
            cp += Math<R>::fabs(d[r]);
          }
        }
      }
      const R ft = R(0.5) * group_sum<R, L>(fp);
      const R ct = group_sum<R, L>(cp);
      if (active) {
        ++evals;
        phi_t = ft + mu * ct;
        if (phi_t <= phi0 + a.c1 * alpha * D || (tiny && Math<R>::finite(phi_t))) {
          accepted = true;
          active = false;
          f_t = ft;
          cn_t = ct;
        } else {
          const R denom = R(2) * (phi_t - phi0 - D * alpha);
          R a_new = (denom > R(0)) ? Math<R>::div(-D * alpha * alpha, denom) : (a.shrink_max * alpha);
          // a diverged trial (merit NaN / inf) is an overlong step like a finite astronomically large one: lower safeguard
          if (!Math<R>::finite(phi_t)) a_new = a.shrink_min * alpha;
          if (!(a_new >= a.shrink_min * alpha)) a_new = a.shrink_min * alpha;
          if (a_new > a.shrink_max * alpha) a_new = a.shrink_max * alpha;
          alpha = a_new;
        }
      }
    }

    CPMPC_TICK(6);
    // ================= accept / reject, step-length memory, damping, termination ===========================
    if (live && status == kTermNone) {
      a_start = R(1);
      if (accepted && a.alpha_growth > R(0)) {
        a_start = (evals > 1 ? a.alpha_growth_bt : a.alpha_growth) * alpha;
        if (!(a_start < R(1))) a_start = R(1);
      }
      if (accepted) {
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          xs[r] += alpha * dxs[r];
          xe[r] += alpha * dxe[r];
        }
        xs[0] = clampr(xs[0], -a.bx_lim, a.bx_lim);
        xe[0] = clampr(xe[0], -a.bx_lim, a.bx_lim);
        wrap_angles<R, M>(xs);
        wrap_angles<R, M>(xe);
#pragma unroll
        for (int i = 0; i < SP; ++i)
          lds_u[i * 64 + lane] = clampr(lds_u[i * 64 + lane] + alpha * lds_du[i * 64 + lane], -a.u_lim, a.u_lim);
        lam *= a.lam_down;
        if (lam < a.lam_min) lam = R(0);
      }
      if (first_order) {
        status = kTermFirstOrder;
      } else if (accepted) {
        if (a.rel_tol > R(0) && (phi0 - phi_t) < a.rel_tol * phi0) status = kTermRelTol;
      } else {
        ++failed;
        lam = (lam > R(0)) ? lam * a.lam_up : a.lam_fail_init;
        if (lam > a.lam_max) status = kTermMaxLambda;
      }
    }
    if (live) {
      if (status != kTermNonFinite) iters += 1;
      evals_tot += evals;
      f_last = f_t;   // accepted: the trial's pieces; else f, cn as used above (the iterate has not moved)
      cn_last = cn_t;
      if (accepted && status != kTermNonFinite) have_trial = !skip_merit;  // (skipped: f_last is not the new iterate's)
    }
  }

  CPMPC_TICK(7);
  // ---- write the iterate (= warm start) and the per-problem solver state back -------------------------------
  if (valid) {
    a.zx[(int64_t)s * st + p] = pack<R, NX>(xs);
    if (s == L - 1) a.zx[(int64_t)L * st + p] = pack<R, NX>(xe);
#pragma unroll
    for (int i = 0; i < SP; ++i) a.zu[(int64_t)(s * SP + i) * st + p] = lds_u[i * 64 + lane];
    if (s == 0) {
      a.sc[SC_LAMBDA * st + p] = lam;
      a.sc[SC_MU * st + p] = mu;
      a.sc[SC_F_LAST * st + p] = f_last;
      a.sc[SC_CN_LAST * st + p] = cn_last;
      a.sc[SC_ALPHA * st + p] = a_start;
      a.sc[SC_TRIAL * st + p] = have_trial ? R(1) : R(0);
      a.ist[IS_STATUS * st + p] = status;
      a.ist[IS_ITERS * st + p] = iters;
      a.ist[IS_LS_EVALS * st + p] = evals_tot;
      a.ist[IS_FAILED * st + p] = failed;
    }
  }
  CPMPC_TICK(7);
  CPMPC_TICK_FLUSH();
  CPMPC_CLOCK_END();
#undef G_LD
#undef G_ST
#undef SZ
#undef IS_COST
