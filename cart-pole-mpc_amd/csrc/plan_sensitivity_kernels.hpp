// plan_sensitivity_kernels.hpp -- how the planned controls move with the three inputs that change between two re-plans, and
// the first-order update of the whole plan made from them.  One problem per lane, no LDS, the workspace layout of
// mpc_kernels.hpp; the companion of feedback_kernels.hpp, whose notation this keeps.
//
// The QP of an SQP iteration (qp_ls_kernel) is linear in its initial-state row c_init = z_0 - x0, in the target of the
// b_x terminal row (the set-point) and in u_prev, which enters the control-cost gradient through the row
// w_du (u_0 - u_prev) only: g_0 holds - w_du^2 u_prev.  With T = U D U^T, W = U^-1 R^T, S = W^T D^-1 W, Dg and Psi_0 as in
// feedback_kernels.hpp and  op(v) = U^-T D^-1 W v,  op(v)_k = (w_k . v) / d_k - upsilon_{k-1} op(v)_{k-1}:
//
//     K    = du / dx0        = - op((S + Dg)^-1 Psi_0)                       NX columns
//     k_sp = du / dset_point = + op((S + Dg)^-1 Rw[0] e_0)                   Rw[0]: the b_x terminal row's weight (1: equality)
//     k_up = du / du_prev    =   U^-T D^-1 (w_du^2 e_0 - W dq),              dq = (w_du^2 / d_0) (S + Dg)^-1 w_0
//
// all of the UNDAMPED, UNCLAMPED QP at the linearisation point z, and all independent of x0, the set-point's value,
// u_prev's value, the residuals and the defects.
//
//   sweep 1 (k descending)  as in feedback_gain_kernel, at lambda = 0; w_0 and 1 / d_0 are what the sweep ends with, so dq
//                           needs nothing stored.
//   LDL^T of S + Dg         once (condensed_qp.hpp), then up to NX + 2 solves: only the outputs the caller asked for
//                           (a wave-uniform choice: the output pointers are kernel arguments).
//   ascending pass          one pass writes rows 0 .. n_rows-1 of every output asked for.
// WIDEQ (float handles with cpmpc_wide_qp()): as in feedback_gain_kernel the descending pass "1b" forms w_k . v in double
// for the NX gain columns and leaves them in the slots of W; the two further scalars per control, w_k . q_sp and w_k . dq,
// go to the .x and .w lanes of the Tk element, which that kernel leaves unused: no new workspace.
// The pieces of sweep 1 are condensed_qp.hpp's, the gain rows of the ascending pass are gain_row of feedback_kernels.hpp:
// the code feedback_gain_kernel runs, so K asked for here is the K of that kernel.  The loop over the controls and the
// rank-one update of S are this kernel's own text (condensed_qp.hpp says why), and so is the column step of pass 1b, which
// restates pass1b_step of condensed_qp.hpp: with that function the two wide float forms compile smaller (4-state 148 -> 128
// VGPRs, 6-state 256 + 22 AGPRs -> 246) and the 6-state one runs 4 - 6 % slower on an MI355X (65 536 problems, all outputs,
// n_rows = N: 0.223 -> 0.236 ms; the 4-state one 2 - 5 % faster).  A fix to pass1b_step is to be carried over here.
// A lane whose d_k or LDL^T pivot is not positive (or not a number) reports ok = 0 and gets NaN in every output; nothing
// of a lane depends on its neighbours.
#pragma once
#include "feedback_kernels.hpp"

namespace cpmpc {

template <typename R, typename M, bool WIDEQ>
__global__ __launch_bounds__(64) void plan_sensitivity_kernel(const SolverArgs<R, M> a, const int n_rows,
                                                               R* __restrict__ K_out, R* __restrict__ ksp_out,
                                                               R* __restrict__ kup_out, int32_t* __restrict__ ok_out) {
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
  const bool want_K = K_out != nullptr, want_sp = ksp_out != nullptr, want_up = kup_out != nullptr;  // wave-uniform
  R Rw[NX], Dg[NX];
  load_terminal<R, M>(a, p, Rw, Dg);

  // ---- sweep 1 (k descending), lambda = 0 ---------------------------------------------------------
  W Sm[NX][NX];
  Q Psi[NX][NX];
  Q wk[NX];  // w_{k+1}, then w_k; w_0 when the sweep ends
  sweep1_init(Rw, Sm, Psi, wk);
  bool pd_ok = true;
  R inv_d0 = R(0);  // 1 / d_0 when the sweep ends
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
        inv_d0 = inv_d;
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

  // ---- LDL^T of S + Dg on the lower triangle, then the solves that were asked for ------------------
  W Qm[NX][NX];  // Qm[j]: (S + Dg)^-1 (column j of Psi_0)
  W qx[2][NX];   // qx[0] = (S + Dg)^-1 Rw[0] e_0,  qx[1] = dq = (w_du^2 / d_0) (S + Dg)^-1 w_0
#pragma unroll
  for (int j = 0; j < NX; ++j)
#pragma unroll
    for (int i = 0; i < NX; ++i) Qm[j][i] = W(0);
#pragma unroll
  for (int i = 0; i < NX; ++i) qx[0][i] = qx[1][i] = W(0);
  {
#pragma unroll
    for (int i = 0; i < NX; ++i) Sm[i][i] += WO::of(Dg[i]);
    TerminalLDL<R, NX> ldl;
    if (!ldl.factor(Sm)) pd_ok = false;
    if (want_K) {
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        W b[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) b[i] = (W)Psi[i][j];
        ldl.solve(b, Qm[j]);
      }
    }
    if (want_sp) {
      W b[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) b[i] = (i == 0) ? (W)Rw[0] : W(0);
      ldl.solve(b, qx[0]);
    }
    if (want_up) {
      const W f0 = (W)wd2 * (W)inv_d0;
      W b[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) b[i] = f0 * (W)wk[i];
      ldl.solve(b, qx[1]);
    }
  }

  // ---- wide QP only (k descending): w_k . v in double; the gain columns left in the slots of W, the two further
  // scalars in the .x / .w lanes of Tk -------------------------------------------------------------------------------
  if constexpr (kWideQP) {
    W psi[NX][NX];  // psi[c][j] = (Psi_s^T Q)[c][j]
#pragma unroll
    for (int c = 0; c < NX; ++c)
#pragma unroll
      for (int j = 0; j < NX; ++j) psi[c][j] = (W)Rw[c] * Qm[j][c];
    W psx[NX][2];  // the same for q_sp and dq
#pragma unroll
    for (int c = 0; c < NX; ++c)
#pragma unroll
      for (int j = 0; j < 2; ++j) psx[c][j] = (W)Rw[c] * qx[j][c];
    W om[NX], omx[2];
#pragma unroll
    for (int j = 0; j < NX; ++j) om[j] = W(0);
    omx[0] = omx[1] = W(0);
    const bool want_x = want_sp || want_up;
    int kk = N - 1;
    for (int s = S - 2; s >= 0; --s) {
      for (int i = SP - 1; i >= 0; --i, --kk) {
        R gk[NX];
        unpack<R, NX>(a.Gam[(int64_t)kk * st + p], gk);
        V4 T = a.Tk[(int64_t)kk * st + p];
        if (want_K) {
          R wq[NX];
#pragma unroll
          for (int j = 0; j < NX; ++j) {
            W pg = psi[0][j] * (W)gk[0];
#pragma unroll
            for (int m = 1; m < NX; ++m) pg += psi[m][j] * (W)gk[m];
            om[j] = pg - (W)T.y * om[j];
            wq[j] = (R)om[j];
          }
          if (kk < n_rows) a.Wk[(int64_t)kk * st + p] = pack<R, NX>(wq);
        }
        if (want_x) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            W pg = psx[0][j] * (W)gk[0];
#pragma unroll
            for (int m = 1; m < NX; ++m) pg += psx[m][j] * (W)gk[m];
            omx[j] = pg - (W)T.y * omx[j];
          }
          if (kk < n_rows) {
            T.x = (R)omx[0];
            T.w = (R)omx[1];
            a.Tk[(int64_t)kk * st + p] = T;
          }
        }
      }
      if (s == 0) break;
      if (want_K) phi_transpose_times(a.Phi, s, st, p, psi);  // for the interval below
      if (want_x) phi_transpose_times(a.Phi, s, st, p, psx);
    }
  }

  // ---- ascending pass: the first n_rows rows of every output asked for -------------------------------
  if (ok_out != nullptr) ok_out[p] = pd_ok ? 1 : 0;
  const R qnan = R(__builtin_nan(""));
  W kprev[NX];
#pragma unroll
  for (int j = 0; j < NX; ++j) kprev[j] = W(0);
  W sp_prev = W(0), up_prev = W(0);
  W ups_prev = W(0);
  for (int kk = 0; kk < n_rows; ++kk) {
    R wr[NX];
    const V4 T = a.Tk[(int64_t)kk * st + p];
    if (!kWideQP || want_K) unpack<R, NX>(a.Wk[(int64_t)kk * st + p], wr);
    if (want_K) gain_row<kWideQP>(wr, Qm, (W)T.z, ups_prev, kprev, pd_ok, K_out, kk, a.B, p);
    if (want_sp) {
      W wq;
      if constexpr (kWideQP) wq = (W)T.x;
      else wq = dot<W>(wr, qx[0]);
      const W kr = wq * (W)T.z - ups_prev * sp_prev;
      sp_prev = kr;
      ksp_out[(int64_t)kk * a.B + p] = pd_ok ? (R)kr : qnan;
    }
    if (want_up) {
      W wq;
      if constexpr (kWideQP) wq = (W)T.w;
      else wq = dot<W>(wr, qx[1]);
      const W y = (kk == 0 ? (W)wd2 : W(0)) - wq;  // (w_du^2 e_0 - W dq)_k
      const W kr = y * (W)T.z - ups_prev * up_prev;
      up_prev = kr;
      kup_out[(int64_t)kk * a.B + p] = pd_ok ? (R)kr : qnan;
    }
    ups_prev = (W)T.y;
  }
}

// u_out[k] = clamp(u_nom[k] + K[k] . wrap(x - x_nom) + k_sp[k] (sp - sp_nom) + k_up[k] (u_prev - u_prev_nom), +-u_limit) for
// the rows k < n_rows: the first-order re-plan of the whole horizon.  Elementwise over (row = blockIdx.y, problem); a term
// whose sensitivity pointer is null is absent.  Arrays packed [field][B]; u_out may alias u_nom (an element is read and
// written by its own thread only).  The gain term is feedback_apply_kernel's, multiply-add by multiply-add.
template <typename R, typename M>
__global__ __launch_bounds__(256) void plan_update_kernel(const int64_t B, const R* u_nom, const R* __restrict__ K,
                                                           const R* __restrict__ x_nom, const R* __restrict__ x,
                                                           const R* __restrict__ k_sp, const R* __restrict__ sp_nom,
                                                           const R* __restrict__ sp, const R* __restrict__ k_up,
                                                           const R* __restrict__ u_prev_nom,
                                                           const R* __restrict__ u_prev, const R u_limit, R* u_out) {
  constexpr int NX = M::NX;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const int64_t k = blockIdx.y;
  R u = u_nom[k * B + p];
  if (K != nullptr) {
    R dx[NX];
#pragma unroll
    for (int t = 0; t < NX; ++t) dx[t] = x[t * B + p] - x_nom[t * B + p];
    wrap_angles<R, M>(dx);
#pragma unroll
    for (int t = 0; t < NX; ++t) u = Math<R>::fma(K[(k * NX + t) * B + p], dx[t], u);
  }
  if (k_sp != nullptr) u = Math<R>::fma(k_sp[k * B + p], sp[p] - sp_nom[p], u);
  if (k_up != nullptr) u = Math<R>::fma(k_up[k * B + p], u_prev[p] - u_prev_nom[p], u);
  u_out[k * B + p] = clampr(u, -u_limit, u_limit);
}

}  // namespace cpmpc
