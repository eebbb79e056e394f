// plan_vjp_kernels.hpp -- the reverse mode of plan_sensitivity_kernels.hpp: a cotangent gbar = dL/du on the planned
// controls pulled back to the three inputs that change between two re-plans,
//
//     g_x0 = K^T gbar [NX],     g_sp = k_sp^T gbar,     g_up = k_up^T gbar       per problem,
//
// without K, k_sp or k_up ever being formed.  One problem per lane, no LDS, the workspace layout of mpc_kernels.hpp and
// the notation of feedback_kernels.hpp / plan_sensitivity_kernels.hpp.
//
// With op(v) = U^-T D^-1 W v the adjoint is op^T gbar = W^T D^-1 U^-1 gbar, and U^-1 runs in the direction of sweep 1: next
// to w_k, upsilon_k, 1 / d_k and S the descending sweep carries
//
//     eta_k = gbar_k - upsilon_k eta_{k+1}          (gbar_k = 0 for k >= n_rows, eta_N = 0)
//     a    += w_k (eta_k / d_k)                     [NX]
//
// and ends with w_0, 1 / d_0, eta_0 and Psi_0 in hand.  Then one LDL^T of S + Dg, ONE solve q = (S + Dg)^-1 a, and
//
//     g_x0 = - Psi_0^T q,       g_sp = Rw[0] q_0,       g_up = (w_du^2 / d_0) (eta_0 - w_0 . q).
//
// Like K, k_sp and k_up these belong to the UNDAMPED, UNCLAMPED Gauss-Newton QP at the linearisation point z: they are not
// derivatives of the converged NLP solution, and they do not depend on x0, the set-point's value, u_prev's value, the
// residuals or the defects.
//
// No ascending pass, no pass 1b, and nothing is written to Wk, Tk or any other workspace array: the kernel reads Phi, Gamma
// and gbar [n_rows][B] (rows at or beyond n_rows are an implicit zero, never a load) and writes the outputs whose pointer is
// not null (a wave-uniform choice: the pointers are kernel arguments).  eta, a, q and the three products are carried in
// the wide type of wide.hpp; with WIDEQ on a float handle Psi and w_k are double in sweep 1 already, so the wide form
// needs no second pass.
// Sweep 1 is made of the pieces of condensed_qp.hpp that plan_sensitivity_kernel uses (the set-up of S, Psi and w,
// tridiag_pivot, Psi <- Psi Phi_s, the TerminalLDL); the loop over the controls, which here prefetches gbar's row beside
// Gamma's column, and the rank-one update of S are this kernel's own text (condensed_qp.hpp says why).
// A lane whose d_k or LDL^T pivot is not positive (or not a number) reports ok = 0 and gets NaN in every output; nothing
// of a lane depends on its neighbours.
#pragma once
#include "mpc_kernels.hpp"

namespace cpmpc {

template <typename R, typename M, bool WIDEQ>
__global__ __launch_bounds__(64) void plan_vjp_kernel(const SolverArgs<R, M> a, const int n_rows,
                                                       const R* __restrict__ gbar, R* __restrict__ gx0_out,
                                                       R* __restrict__ gsp_out, R* __restrict__ gup_out,
                                                       int32_t* __restrict__ ok_out) {
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
  R Rw[NX], Dg[NX];
  load_terminal<R, M>(a, p, Rw, Dg);

  // ---- sweep 1 (k descending), lambda = 0, with the adjoint recurrence ---------------------------------
  W Sm[NX][NX];
  Q Psi[NX][NX];
  Q wk[NX];  // w_{k+1}, then w_k; w_0 when the sweep ends
  sweep1_init(Rw, Sm, Psi, wk);
  bool pd_ok = true;
  R inv_d0 = R(0);  // 1 / d_0 when the sweep ends
  W eta = W(0);     // eta_{k+1}, then eta_k; eta_0 when the sweep ends
  W av[NX];         // a = sum_k w_k eta_k / d_k
#pragma unroll
  for (int r = 0; r < NX; ++r) av[r] = W(0);
  {
    R d_next = R(1);
    const XVn* __restrict__ gam_p = a.Gam + p;
    const R* __restrict__ gbar_p = gbar + p;
    XVn G_nx = gam_p[(int64_t)(N - 1) * st];  // software pipeline: column k-1 is loaded before column k is consumed
    R gb_nx = (N - 1 < n_rows) ? gbar_p[(int64_t)(N - 1) * a.B] : R(0);  // (wave-uniform) and so is gbar's row
    int kk = N - 1;
    for (int s = S - 2; s >= 0; --s) {
      for (int i = SP - 1; i >= 0; --i, --kk) {
        R gk[NX];
        unpack<R, NX>(G_nx, gk);
        const W gb = (W)gb_nx;
        if (kk > 0) {
          G_nx = gam_p[(int64_t)(kk - 1) * st];
          gb_nx = (kk - 1 < n_rows) ? gbar_p[(int64_t)(kk - 1) * a.B] : R(0);
        }
        // U D U^T recurrence of the tridiagonal control-cost Hessian (off-diagonal -wd2), undamped
        R ups, dk, inv_d;
        tridiag_pivot(kk, N, wu2, wd2, R(0), d_next, ups, dk, inv_d);
        if (!(dk > R(0))) pd_ok = false;
        d_next = dk;
        inv_d0 = inv_d;
        // m_k = Psi Gamma_k ; w_k = m_k - ups w_{k+1}
#pragma unroll
        for (int r = 0; r < NX; ++r) wk[r] = dot<Q>(Psi[r], gk) - Q(ups) * wk[r];
        // eta_k = gbar_k - ups eta_{k+1} ; a += w_k eta_k / d_k
        eta = gb - (W)ups * eta;
        const W e = eta * (W)inv_d;
#pragma unroll
        for (int r = 0; r < NX; ++r) av[r] += (W)wk[r] * e;
#pragma unroll
        for (int i2 = 0; i2 < NX; ++i2) {
          const W wi = (W)wk[i2] * (W)inv_d;
#pragma unroll
          for (int j2 = 0; j2 <= i2; ++j2) Sm[i2][j2] += wi * (W)wk[j2];
        }
      }
      psi_times_phi(Psi, a.Phi, s, st, p);
    }
  }

  // ---- LDL^T of S + Dg on the lower triangle, the one solve q = (S + Dg)^-1 a ---------------------------
  W q[NX];
  {
#pragma unroll
    for (int i = 0; i < NX; ++i) Sm[i][i] += WO::of(Dg[i]);
    TerminalLDL<R, NX> ldl;
    if (!ldl.factor(Sm)) pd_ok = false;
    ldl.solve(av, q);
  }

  // ---- the products that were asked for ------------------------------------------------------------------
  if (ok_out != nullptr) ok_out[p] = pd_ok ? 1 : 0;
  const R qnan = R(__builtin_nan(""));
  if (gx0_out != nullptr) {  // - Psi_0^T q
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      W acc = (W)Psi[0][j] * q[0];
#pragma unroll
      for (int i = 1; i < NX; ++i) acc += (W)Psi[i][j] * q[i];
      gx0_out[(int64_t)j * a.B + p] = pd_ok ? (R)(-acc) : qnan;
    }
  }
  if (gsp_out != nullptr) gsp_out[p] = pd_ok ? (R)((W)Rw[0] * q[0]) : qnan;  // Rw[0] q_0
  if (gup_out != nullptr) {  // (w_du^2 / d_0) (eta_0 - w_0 . q)
    const W f0 = (W)wd2 * (W)inv_d0;
    gup_out[p] = pd_ok ? (R)(f0 * (eta - dot<W>(wk, q))) : qnan;
  }
}

}  // namespace cpmpc
