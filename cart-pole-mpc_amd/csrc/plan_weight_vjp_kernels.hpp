// plan_weight_vjp_kernels.hpp -- the gradient of a loss on the planned controls with respect to the COST WEIGHTS of the
// controller: for a cotangent gbar = dL/du+ on the controls u+ = u + du of the undamped, unclamped Gauss-Newton QP at z,
//
//     g_tw [NX] (the terminal weights),     g_wu (u_cost_weight),     g_wdu (u_derivative_cost_weight)     per problem,
//
// and, on request, the primal QP step du itself.  One problem per lane, no LDS, the workspace layout of mpc_kernels.hpp and
// the notation of feedback_kernels.hpp / plan_vjp_kernels.hpp.
//
// Every cost row is r_i = w_i e_i, J_i = w_i a_i with e_i, a_i free of the weights, so with the QP's solution dz, its
// linearised residual rho = r + J dz and the adjoint y = (KKT^-1 [E gbar; 0])_z the gradient with respect to the weight of row i
// is  -(2 / w_i) (J_i y) rho_i = -2 w_i (a_i . y) (e_i + a_i . dz).  Two solves of one system, both in condensed form:
//
//   primal   qp_ls_kernel's sweep 1 at lambda = 0: g_k from u, u_prev, w_u, w_du; gw = U^-1 g; rho = W^T D^-1 gw; the weighted
//            free response of the defects and of c_init = z_0 - x0; q_p = (S + Dg)^-1 (h - rho);  U^T du = -D^-1 (gw + W q_p)
//   adjoint  plan_vjp_kernel's: eta = U^-1 gbar, a = W^T D^-1 eta; q_a = (S + Dg)^-1 a;  U^T y = D^-1 (eta - W q_a)
//
// sharing d_k, upsilon_k, w_k, Psi, S and ONE LDL^T.  What is NOT taken over from qp_ls_kernel: its double form refines q once
// through the factored operator and then the whole QP solution (refine_qp_pass); neither solve here is refined, so du agrees
// with the split pipeline's undamped full step to rounding times the conditioning of S + Dg, not bitwise.
// The multiplier of a terminal COST row is that row's linearised residual -- q_p[t] = w_t (e_t + dx_{S-1,t}), q_a[t] = w_t yx_t -- so
//
//     g_tw[t] = -2 q_a[t] q_p[t] / w_t      (exactly 0 for an equality row and for w_t = 0)
//
// needs no state recovery, and the ascending pass forms du_k and y_k together for
//
//     g_wu  = -2 w_u  sum_k y_k v_k,                         v_k = u_k + du_k,  v_{-1} = u_prev,  y_{-1} = 0
//     g_wdu = -2 w_du sum_k (y_{k-1} - y_k) (v_{k-1} - v_k).
//
// Like K these belong to the LAST QP: they are not derivatives through the line search, the retraction clamps or the SQP's
// earlier iterations.  Unlike K they DO depend on x0, the set-point and u_prev.
//
//   sweep 1 (k descending)  w_k, upsilon_k, 1 / d_k, S, and beside them g_k, gw_k, rho, the free response (primal) and eta_k,
//                           a (adjoint).  Rows k below the ascending pass's bound leave w_k in Wk and {gw_k, upsilon_k, 1 / d_k,
//                           eta_k} in Tk -- scratch every step recomputes; nothing else of the workspace is written.
//   LDL^T of S + Dg         once (condensed_qp.hpp), two solves.
//   ascending pass          rows 0 .. N-1 when g_wu or g_wdu is asked for, rows 0 .. n_rows-1 when only du is, none otherwise
//                           (a wave-uniform choice: the output pointers are kernel arguments).
// WIDEQ (float handles with cpmpc_wide_qp()): Psi and w_k are double and w_k is never stored; a descending pass "1b" forms
// w_k . q_p and w_k . q_a in double, as plan_sensitivity_kernel's does for its two scalars, and leaves -(gw_k + w_k . q_p) and
// eta_k - w_k . q_a in the .x / .w lanes of the Tk element.
// In float handles eta, a, S, rho, the free response, the LDL^T, both solves and the ascending pass are carried in the wide
// type of wide.hpp.  One kernel in all eight instantiations: the double 6-state form holds both solves without scratch
// (DESIGN.md section 5d has the resource lines), so the two-kernel split was not needed.
// Sweep 1 uses the pieces of condensed_qp.hpp that plan_vjp_kernel uses, except sweep1_init: the set-up of S, Psi and w
// stays written out here (the note at that set-up says why).  Pass 1b uses the column step that plan_sensitivity_kernel
// uses for its two scalars.  The primal quantities beside them restate qp_ls_kernel's sweep 1 (that kernel shares none of
// it: its figures are in condensed_qp.hpp), and the loop over the controls and the rank-one update of S, here in one loop
// with rho and a, are this kernel's own text.
// A lane whose d_k or LDL^T pivot is not positive (or not a number) reports ok = 0 and gets NaN in every output; nothing
// of a lane depends on its neighbours.
#pragma once
#include "mpc_kernels.hpp"

namespace cpmpc {

// wrap_angles for the two residuals this kernel reads, c_init = z_0 - x0 and the terminal error: an angle already in
// (-pi, pi] is left as it is.  mod_pi sends a negative one through + 2 pi, - 2 pi, which changes nothing in exact arithmetic
// and costs half an ulp of 2 pi -- 2.4e-7 in float -- on a difference of two floats that was exact.  The solver never sees
// that (its QP is as well posed around the moved residual), but g_tw of a pole-angle row is proportional to that row's
// residual: in the float handles its error was five times that of the other outputs ("Feedback gains").
// The cut is mod_pi's: -pi itself and everything outside the interval still go through it.
template <typename R, typename M>
__device__ __forceinline__ void wrap_angles_in_place(R (&x)[M::NX]) {
  constexpr R pi = static_cast<R>(3.14159265358979323846);
#pragma unroll
  for (int t = 1; t < M::NQ; ++t) x[t] = (x[t] > -pi && x[t] <= pi) ? x[t] : mod_pi(x[t]);
}

template <typename R, typename M, bool WIDEQ>
__global__ __launch_bounds__(64) void plan_weight_vjp_kernel(const SolverArgs<R, M> a, const XV<R, M::NX>* __restrict__ zx_in,
                                                              const R* __restrict__ zu_in, const R* __restrict__ u_prev_in,
                                                              const int n_rows, const R* __restrict__ gbar,
                                                              R* __restrict__ gtw_out, R* __restrict__ gwu_out,
                                                              R* __restrict__ gwdu_out, R* __restrict__ du_out,
                                                              int32_t* __restrict__ ok_out) {
  using V4 = typename VecT<R>::V4;
  using XVn = XV<R, M::NX>;
  using W = typename WideOf<R>::type;
  using WO = Wide<W>;
  constexpr bool kWidened = !std::is_same<W, R>::value;
  constexpr bool kWideQP = WIDEQ && kWidened;
  using Q = std::conditional_t<kWideQP, W, R>;
  constexpr int NX = M::NX;
  const unsigned p = blockIdx.x * 64u + threadIdx.x;
  if (p >= a.B) return;
  const int64_t st = a.stride;
  const int N = a.N, S = a.S, SP = a.SP;
  const R wu2 = a.wu * a.wu, wd2 = a.wd * a.wd;
  const bool want_sums = gwu_out != nullptr || gwdu_out != nullptr;  // wave-uniform
  const int n_asc = want_sums ? N : (du_out != nullptr ? n_rows : 0);
  const R u_prev = (u_prev_in != nullptr) ? u_prev_in[p] : R(0);
  R Rw[NX], Dg[NX];
  load_terminal<R, M>(a, p, Rw, Dg);

  // ---- residuals at z: the initial-state rows and the terminal rows (qp_ls_kernel, phase 1) -----------------------------
  R ci[NX];
  W hv[NX];
  {
    R z0[NX], zt[NX], e_term[NX];
    unpack<R, NX>(zx_in[p], z0);
#pragma unroll
    for (int t = 0; t < NX; ++t) ci[t] = z0[t] - a.x0[t * a.B + p];
    wrap_angles_in_place<R, M>(ci);
    unpack<R, NX>(zx_in[(int64_t)(S - 1) * st + p], zt);
#pragma unroll
    for (int t = 0; t < NX; ++t) e_term[t] = zt[t] - a.term_tgt[t];
    if (a.set_point) e_term[0] = zt[0] - a.set_point[p];
    wrap_angles_in_place<R, M>(e_term);
#pragma unroll
    for (int t = 0; t < NX; ++t) hv[t] = WO::prod(Rw[t], e_term[t]);  // + the weighted free response, added after sweep 1
  }

  // ---- sweep 1 (k descending), lambda = 0, primal and adjoint recurrences side by side -------------------------------
  // (not sweep1_init: with it AND psi_times_phi the double 4-state form keeps Psi as one vector value, the multiply-adds
  // pair up differently and g_wu, g_wdu, g_tw and du move by up to 4e-11, 6e-11, 4e-15 and 4e-12 -- measured on an MI355X)
  W Sm[NX][NX], rho[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    rho[i] = WO::of(R(0));
#pragma unroll
    for (int j = 0; j < NX; ++j) Sm[i][j] = WO::of(R(0));
  }
  bool pd_ok = true;
  W av[NX];  // a = sum_k w_k eta_k / d_k
#pragma unroll
  for (int r = 0; r < NX; ++r) av[r] = W(0);
  {
    Q Psi[NX][NX];
#pragma unroll
    for (int r = 0; r < NX; ++r)
#pragma unroll
      for (int c = 0; c < NX; ++c) Psi[r][c] = (r == c) ? Q(Rw[r]) : Q(0);
    Q wk[NX];  // w_{k+1}, then w_k
    W ha[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      wk[r] = Q(0);
      ha[r] = WO::of(R(0));
    }
    R gwprev = R(0);
    W eta = W(0);  // eta_{k+1}, then eta_k
    R d_next = R(1);
    const XVn* __restrict__ gam_p = a.Gam + p;
    const R* __restrict__ zu_p = zu_in + p;
    const R* __restrict__ gbar_p = gbar + p;
    R u_hi = R(0);                          // u_{k+1}
    R u_cur = zu_p[(int64_t)(N - 1) * st];  // u_k
    // software pipeline: the loads of column k-1 are issued before column k is consumed
    XVn G_nx = gam_p[(int64_t)(N - 1) * st];
    R u_nx = (N > 1) ? zu_p[(int64_t)(N - 2) * st] : u_prev;
    R gb_nx = (gbar != nullptr && N - 1 < n_rows) ? gbar_p[(int64_t)(N - 1) * a.B] : R(0);  // (wave-uniform)
    int kk = N - 1;
    for (int s = S - 2; s >= 0; --s) {
      for (int i = SP - 1; i >= 0; --i, --kk) {
        R gk[NX];
        unpack<R, NX>(G_nx, gk);
        const R u_lo = u_nx;  // u_{k-1} (u_prev for k = 0)
        const W gb = (W)gb_nx;
        if (kk > 0) {
          G_nx = gam_p[(int64_t)(kk - 1) * st];
          u_nx = (kk > 1) ? zu_p[(int64_t)(kk - 2) * st] : u_prev;
          gb_nx = (gbar != nullptr && kk - 1 < n_rows) ? gbar_p[(int64_t)(kk - 1) * a.B] : R(0);
        }
        // the control-cost gradient g_k at z
        R g = wu2 * u_cur + wd2 * (u_cur - u_lo);
        if (kk < N - 1) g += wd2 * (u_cur - u_hi);
        // U D U^T recurrence of the tridiagonal control-cost Hessian (off-diagonal -wd2), undamped
        R ups, dk, inv_d;
        tridiag_pivot(kk, N, wu2, wd2, R(0), d_next, ups, dk, inv_d);
        if (!(dk > R(0))) pd_ok = false;
        d_next = dk;
        // m_k = Psi Gamma_k ; w_k = m_k - ups w_{k+1}
#pragma unroll
        for (int r = 0; r < NX; ++r) wk[r] = dot<Q>(Psi[r], gk) - Q(ups) * wk[r];
        const R gw = g - ups * gwprev;
        // eta_k = gbar_k - ups eta_{k+1}
        eta = gb - (W)ups * eta;
        if (kWideQP || kk < n_asc) {  // (wave-uniform) pass 1b reads every row of Tk, the ascending pass these rows only
          if constexpr (!kWideQP) {
            R wk_r[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) wk_r[r] = (R)wk[r];
            a.Wk[(int64_t)kk * st + p] = pack<R, NX>(wk_r);
          }
          a.Tk[(int64_t)kk * st + p] = mk4<R>(gw, ups, inv_d, (R)eta);
        }
        const W e = eta * (W)inv_d;
#pragma unroll
        for (int i2 = 0; i2 < NX; ++i2) {
          const W wi = (W)wk[i2] * (W)inv_d;
          rho[i2] += wi * gw;
          av[i2] += (W)wk[i2] * e;
#pragma unroll
          for (int j2 = 0; j2 <= i2; ++j2) Sm[i2][j2] += wi * (W)wk[j2];
        }
        gwprev = gw;
        u_hi = u_cur;
        u_cur = u_lo;
      }
      // the defect of this interval, propagated to the last node with its weights: Psi_s c_s
      {
        R c[NX];
        unpack<R, NX>(a.cs[(int64_t)s * st + p], c);
#pragma unroll
        for (int r = 0; r < NX; ++r) ha[r] += dot<W>(Psi[r], c);
      }
      psi_times_phi(Psi, a.Phi, s, st, p);
    }
    // Psi is now diag(w) Phi_{S-2} ... Phi_0: the contribution of dx_0 = -c_init
#pragma unroll
    for (int r = 0; r < NX; ++r) hv[r] += ha[r] - dot<W>(Psi[r], ci);
  }

  // ---- one LDL^T of S + Dg on the lower triangle, two solves ---------------------------------------------------------
  W qp[NX], qa[NX];  // the multipliers of the terminal rows, primal and adjoint
  {
#pragma unroll
    for (int i = 0; i < NX; ++i) Sm[i][i] += WO::of(Dg[i]);
    TerminalLDL<R, NX> ldl;
    if (!ldl.factor(Sm)) pd_ok = false;
    W rhs[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) rhs[i] = hv[i] - rho[i];
    ldl.solve(rhs, qp);
    ldl.solve(av, qa);
  }

  if (ok_out != nullptr) ok_out[p] = pd_ok ? 1 : 0;
  const R qnan = R(__builtin_nan(""));
  if (gtw_out != nullptr) {  // a cost row's multiplier is its linearised residual: -2 (w yx) (w (e + dx)) / w
#pragma unroll
    for (int t = 0; t < NX; ++t) {
      const bool live = Dg[t] != R(0) && Rw[t] > R(0);
      const W g = live ? W(-2) * qa[t] * qp[t] / (W)Rw[t] : W(0);
      gtw_out[(int64_t)t * a.B + p] = pd_ok ? (R)g : qnan;
    }
  }
  if (n_asc == 0) return;  // (wave-uniform)

  // ---- wide QP only (k descending): w_k . q_p and w_k . q_a in double; -(gw_k + w_k . q_p) and eta_k - w_k . q_a left in
  // the .x / .w lanes of Tk ---------------------------------------------------------------------------------------------
  if constexpr (kWideQP) {
    W psx[NX][2];
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      psx[c][0] = (W)Rw[c] * qp[c];
      psx[c][1] = (W)Rw[c] * qa[c];
    }
    W omx[2];
    omx[0] = omx[1] = W(0);
    int kk = N - 1;
    for (int s = S - 2; s >= 0; --s) {
      for (int i = SP - 1; i >= 0; --i, --kk) {
        R gk[NX];
        unpack<R, NX>(a.Gam[(int64_t)kk * st + p], gk);
        V4 T = a.Tk[(int64_t)kk * st + p];
        pass1b_step(psx, gk, (W)T.y, omx);
        if (kk < n_asc) {
          T.x = (R)(-((W)T.x + omx[0]));
          T.w = (R)((W)T.w - omx[1]);
          a.Tk[(int64_t)kk * st + p] = T;
        }
      }
      if (s == 0) break;
      phi_transpose_times(a.Phi, s, st, p, psx);  // for the interval below
    }
  }

  // ---- ascending pass: du_k and y_k together, the two sums ------------------------------------------------------------
  W du_prev = W(0), y_prev = W(0), ups_prev = W(0);
  W v_prev = (W)u_prev;  // v_{k-1} = u_{k-1} + du_{k-1}; u_prev before the first control
  W s_u = W(0), s_d = W(0);
  for (int kk = 0; kk < n_asc; ++kk) {
    const V4 T = a.Tk[(int64_t)kk * st + p];
    W yp, ya;
    if constexpr (kWideQP) {
      yp = (W)T.x;
      ya = (W)T.w;
    } else {
      R wr[NX];
      unpack<R, NX>(a.Wk[(int64_t)kk * st + p], wr);
      yp = -((W)T.x + dot<W>(wr, qp));
      ya = (W)T.w - dot<W>(wr, qa);
    }
    const W du = yp * (W)T.z - ups_prev * du_prev;
    const W yk = ya * (W)T.z - ups_prev * y_prev;
    if (du_out != nullptr && kk < n_rows) du_out[(int64_t)kk * a.B + p] = pd_ok ? (R)du : qnan;
    if (want_sums) {
      const W v = (W)zu_in[(int64_t)kk * st + p] + du;
      s_u += yk * v;
      s_d += (y_prev - yk) * (v_prev - v);
      v_prev = v;
    }
    du_prev = du;
    y_prev = yk;
    ups_prev = (W)T.y;
  }
  if (gwu_out != nullptr) gwu_out[p] = pd_ok ? (R)(W(-2) * (W)a.wu * s_u) : qnan;
  if (gwdu_out != nullptr) gwdu_out[p] = pd_ok ? (R)(W(-2) * (W)a.wd * s_d) : qnan;
}

}  // namespace cpmpc
