// feedback_kernels.hpp -- the feedback gains of the MPC plan, K = du / dx0 (N x NX per problem), and their use between
// two re-plans.  One problem per lane, no LDS, the workspace layout of mpc_kernels.hpp.
//
// The QP of an SQP iteration (qp_ls_kernel, mpc_kernels.hpp) is linear in its initial-state row c_init = z_0 - x0.  With
// the states eliminated through the shooting recursion, T = U D U^T the tridiagonal control-cost Hessian AT LAMBDA = 0,
// R = diag(w) M the NX terminal rows (w from load_terminal), W = U^-1 R^T, S = W^T D^-1 W, Dg = 1 on cost rows and 0 on
// equality rows, and Psi_0 = diag(w) Phi_{S-2} ... Phi_0 (what Psi holds at the end of sweep 1):
//
//     K = - U^-T D^-1 W (S + Dg)^-1 Psi_0,         u(x0 + delta) ~ u + K delta.
//
// It is the gain of the UNDAMPED, UNCLAMPED QP at the linearisation point z: no +-u_limit / +-b_x_limit retraction, no
// Levenberg-Marquardt term.  K does not depend on x0, the set-point, u_prev, the residuals or the defects: only on z
// (through Phi and Gamma, which launch_linearize has left in the workspace), the dynamics parameters, the terminal
// weights and the two control-cost weights.
//
//   sweep 1 (k descending)  as in qp_ls_kernel: upsilon_k, 1 / d_k, w_k = Psi Gamma_k - upsilon_k w_{k+1}, S += w_k w_k^T / d_k,
//                           Psi <- Psi Phi_s.  Only the rows the caller asked for (k < n_rows) are stored.
//   LDL^T of S + Dg         in the wide type of wide.hpp, then NX solves: Q = (S + Dg)^-1 Psi_0.
//   ascending pass          k_row_k = - (w_k . Q) / d_k - upsilon_{k-1} k_row_{k-1}, which stops after n_rows rows.
// WIDEQ (float handles with cpmpc_wide_qp()): Psi and w_k are carried in double, as in qp_ls_kernel's wide form, and W is
// never read back in float -- a pass of its own (k descending, NX right-hand sides at once) forms
//     w_k . Q = psi_s Gamma_k - upsilon_k (w_{k+1} . Q),   psi_s = Phi_{s+1}^T psi_{s+1},   psi_{S-2} = diag(w) Q
// in double and leaves the rows the caller asked for in the slots of W.
// What is shared (condensed_qp.hpp): with qp_ls_kernel the pivot step of sweep 1, the LDL^T with its solves and the adjoint
// product psi <- Phi_s^T psi; with the three other sensitivity kernels (plan_sensitivity_kernels.hpp, plan_vjp_kernels.hpp,
// plan_weight_vjp_kernels.hpp) also the set-up of S, Psi and w, Psi <- Psi Phi_s and the column step of pass 1b (which
// plan_sensitivity_kernel restates: it runs slower with the function); gain_row below is the gain rows of the ascending
// pass, plan_sensitivity_kernel's too.  What is not: the loop over the controls
// (Gamma's software pipeline, the w_k row, the stores), which differs from kernel to kernel in what it carries, and the
// rank-one update of S, which costs the 6-state instantiations a wave as a function (the figures are in condensed_qp.hpp).
// A lane whose d_k or LDL^T pivot is not positive (or not a number: a poisoned parameter set) reports ok = 0 and gets
// NaN rows; nothing of a lane depends on its neighbours.
#pragma once
#include "mpc_kernels.hpp"

namespace cpmpc {

// Row k of the gains from row k-1 (ascending pass): k_row_k = - (w_k . Q) / d_k - upsilon_{k-1} k_row_{k-1}, NaN for a lane that
// is not ok.  wr is w_k from the slots of W -- in the wide QP w_k . Q itself, which pass 1b left there.  Shared with
// plan_sensitivity_kernel.
template <bool kWideQP, typename R, typename W, int NX>
__device__ __forceinline__ void gain_row(const R (&wr)[NX], const W (&Qm)[NX][NX], const W inv_d, const W ups_prev,
                                         W (&kprev)[NX], const bool pd_ok, R* __restrict__ K_out, const int kk, const int64_t B,
                                         const unsigned p) {
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    W wq;
    if constexpr (kWideQP) wq = (W)wr[j];
    else wq = dot<W>(wr, Qm[j]);
    const W kr = -(wq * inv_d) - ups_prev * kprev[j];
    kprev[j] = kr;
    K_out[((int64_t)kk * NX + j) * B + p] = pd_ok ? (R)kr : R(__builtin_nan(""));
  }
}

template <typename R, typename M, bool WIDEQ>
__global__ __launch_bounds__(64) void feedback_gain_kernel(const SolverArgs<R, M> a, const int n_rows, R* __restrict__ K_out,
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
  R Rw[NX], Dg[NX];
  load_terminal<R, M>(a, p, Rw, Dg);

  // ---- sweep 1 (k descending), lambda = 0 ---------------------------------------------------------
  W Sm[NX][NX];
  Q Psi[NX][NX];
  Q wk[NX];  // w_{k+1}, then w_k
  sweep1_init(Rw, Sm, Psi, wk);
  bool pd_ok = true;
  {
    R d_next = R(1);
    const XVn* __restrict__ gam_p = a.Gam + p;
    XVn G_nx = gam_p[(int64_t)(N - 1) * st];  // software pipeline: column k-1 is loaded before column k is consumed
    int kk = N - 1;
    for (int s = S - 2; s >= 0; --s) {
      for (int i = SP - 1; i >= 0; --i, --kk) {
        R gk[NX];
        unpack<R, NX>(G_nx, gk);
        if (kk > 0) G_nx = gam_p[(int64_t)(kk - 1) * st];
        // U D U^T recurrence of the tridiagonal control-cost Hessian (off-diagonal -wd2), undamped
        R ups, dk, inv_d;
        tridiag_pivot(kk, N, wu2, wd2, R(0), d_next, ups, dk, inv_d);
        if (!(dk > R(0))) pd_ok = false;
        d_next = dk;
        // m_k = Psi Gamma_k ; w_k = m_k - ups w_{k+1}
#pragma unroll
        for (int r = 0; r < NX; ++r) wk[r] = dot<Q>(Psi[r], gk) - Q(ups) * wk[r];
        if (kk < n_rows) {  // (wave-uniform) the ascending pass reads these rows only
          if constexpr (!kWideQP) {
            R wk_r[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) wk_r[r] = (R)wk[r];
            a.Wk[(int64_t)kk * st + p] = pack<R, NX>(wk_r);
          }
        }
        if (kWideQP || kk < n_rows) a.Tk[(int64_t)kk * st + p] = mk4<R>(R(0), ups, inv_d, R(0));
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

  // ---- (S + Dg) Q = Psi_0 by LDL^T on the lower triangle, NX right-hand sides ----------------------
  W Qm[NX][NX];  // Qm[j]: the solution for column j of Psi_0
  {
#pragma unroll
    for (int i = 0; i < NX; ++i) Sm[i][i] += WO::of(Dg[i]);
    TerminalLDL<R, NX> ldl;
    if (!ldl.factor(Sm)) pd_ok = false;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      W b[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) b[i] = (W)Psi[i][j];
      ldl.solve(b, Qm[j]);
    }
  }

  // ---- wide QP only (k descending): w_k . Q in double, the rows asked for left in the slots of W ---------------------
  if constexpr (kWideQP) {
    W psi[NX][NX];  // psi[c][j] = (Psi_s^T Q)[c][j]
#pragma unroll
    for (int c = 0; c < NX; ++c)
#pragma unroll
      for (int j = 0; j < NX; ++j) psi[c][j] = (W)Rw[c] * Qm[j][c];
    W om[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) om[j] = W(0);
    int kk = N - 1;
    for (int s = S - 2; s >= 0; --s) {
      for (int i = SP - 1; i >= 0; --i, --kk) {
        R gk[NX];
        unpack<R, NX>(a.Gam[(int64_t)kk * st + p], gk);
        const V4 T = a.Tk[(int64_t)kk * st + p];
        pass1b_step(psi, gk, (W)T.y, om);
        R wq[NX];
#pragma unroll
        for (int j = 0; j < NX; ++j) wq[j] = (R)om[j];
        if (kk < n_rows) a.Wk[(int64_t)kk * st + p] = pack<R, NX>(wq);
      }
      if (s == 0) break;
      phi_transpose_times(a.Phi, s, st, p, psi);  // for the interval below
    }
  }

  // ---- ascending pass: U^T K = - D^-1 W Q, the first n_rows rows -------------------------------------
  if (ok_out != nullptr) ok_out[p] = pd_ok ? 1 : 0;
  W kprev[NX];
#pragma unroll
  for (int j = 0; j < NX; ++j) kprev[j] = W(0);
  W ups_prev = W(0);
  for (int kk = 0; kk < n_rows; ++kk) {
    R wr[NX];
    unpack<R, NX>(a.Wk[(int64_t)kk * st + p], wr);
    const V4 T = a.Tk[(int64_t)kk * st + p];
    gain_row<kWideQP>(wr, Qm, (W)T.z, ups_prev, kprev, pd_ok, K_out, kk, a.B, p);
    ups_prev = (W)T.y;
  }
}

// u_out = clamp(u_nom + K0 . wrap(x - x_nom), +-u_limit): the first row of the gains applied to the deviation of the
// measured state from the state the plan was made for, the pole angles' differences wrapped.  Arrays packed [field][B].
template <typename R, typename M>
__global__ __launch_bounds__(256) void feedback_apply_kernel(const int64_t B, const R* __restrict__ u_nom,
                                                              const R* __restrict__ K0, const R* __restrict__ x_nom,
                                                              const R* __restrict__ x, const R u_limit,
                                                              R* __restrict__ u_out) {
  constexpr int NX = M::NX;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  R dx[NX];
#pragma unroll
  for (int t = 0; t < NX; ++t) dx[t] = x[t * B + p] - x_nom[t * B + p];
  wrap_angles<R, M>(dx);
  R u = u_nom[p];
#pragma unroll
  for (int t = 0; t < NX; ++t) u = Math<R>::fma(K0[t * B + p], dx[t], u);
  u_out[p] = clampr(u, -u_limit, u_limit);
}

}  // namespace cpmpc
