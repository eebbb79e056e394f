// condensed_qp.hpp -- the blocks of the condensed QP that qp_ls_kernel (mpc_kernels.hpp) and the four sensitivity kernels
// (feedback_kernels.hpp, plan_sensitivity_kernels.hpp, plan_vjp_kernels.hpp, plan_weight_vjp_kernels.hpp) share.
//
// Every piece is a __forceinline__ function (or a struct of registers with two of them) on the caller's own fixed-size
// arrays.  The order of operations of each piece is qp_ls_kernel's: the sums start from their first product where that
// kernel's did, from zero where its did, so no result moves by a bit.  Sections 1 to 3 are used by all five kernels,
// section 4 by the four sensitivity kernels only.  What is NOT here, and why, is at the head of section 4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "cartpole_device.hpp"
#include "wide.hpp"
#include "workspace_layout.hpp"

namespace cpmpc {

// a . b in T, the first product then one multiply-add per further term
template <typename T, typename A, typename B, int NX>
__device__ __forceinline__ T dot(const A (&a)[NX], const B (&b)[NX]) {
  T acc = (T)a[0] * (T)b[0];
#pragma unroll
  for (int m = 1; m < NX; ++m) acc += (T)a[m] * (T)b[m];
  return acc;
}

// reciprocal of a pivot of the terminal system in its wide type W; W == R keeps the kernel's own division
template <typename R, typename W>
__device__ __forceinline__ W wide_inv(const W d) {
  if constexpr (std::is_same<W, R>::value) return Math<R>::div(R(1), d);
  else return Math<double>::div(1.0, d);
}

// ---- 1. the terminal system: LDL^T of S + Dg on the lower triangle, in registers, in the wide type of wide.hpp ----------
// A widened kernel (float) inverts each pivot once in double and multiplies by the inverse; a kernel in its own type
// (double) divides, in the factorisation by R(1) / d and in the solve by y / d.
template <typename R, int NX>
struct TerminalLDL {
  using W = typename WideOf<R>::type;
  static constexpr bool kWidened = !std::is_same<W, R>::value;
  W Lm[NX][NX], dv[NX], idv[NX];

  // false when a pivot is not positive (or not a number)
  __device__ __forceinline__ bool factor(const W (&Sm)[NX][NX]) {
    bool pd_ok = true;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      W dj = Sm[j][j];
#pragma unroll
      for (int m = 0; m < j; ++m) dj -= Lm[j][m] * Lm[j][m] * dv[m];
      if (!(dj > W(0))) pd_ok = false;
      dv[j] = dj;
      W inv;
      if constexpr (kWidened) inv = wide_inv<R, W>(dj);
      else inv = R(1) / dj;
      idv[j] = inv;
#pragma unroll
      for (int i = j + 1; i < NX; ++i) {
        W v = Sm[i][j];
#pragma unroll
        for (int m = 0; m < j; ++m) v -= Lm[i][m] * Lm[j][m] * dv[m];
        Lm[i][j] = v * inv;
      }
    }
    return pd_ok;
  }

  __device__ __forceinline__ void solve(const W (&b)[NX], W (&x)[NX]) const {
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
      W v;
      if constexpr (kWidened) v = y[i] * idv[i];
      else v = y[i] / dv[i];
#pragma unroll
      for (int m = i + 1; m < NX; ++m) v -= Lm[m][i] * x[m];
      x[i] = v;
    }
  }
};

// ---- 2. the adjoint product ------------------------------------------------------------------------------------------
// psi <- Phi_s^T psi for NC columns at once (psi[r][j]: row r of column j), row by row of Phi_s from the workspace
template <typename Q, typename R, int NX, int NC>
__device__ __forceinline__ void phi_transpose_times(const XV<R, NX>* Phi, const int s, const int64_t st, const unsigned p,
                                                    Q (&psi)[NX][NC]) {
  Q pn[NX][NC];
#pragma unroll
  for (int c = 0; c < NX; ++c)
#pragma unroll
    for (int j = 0; j < NC; ++j) pn[c][j] = Q(0);
#pragma unroll
  for (int r = 0; r < NX; ++r) {
    R row[NX];
    unpack<R, NX>(Phi[(int64_t)(NX * s + r) * st + p], row);
#pragma unroll
    for (int c = 0; c < NX; ++c)
#pragma unroll
      for (int j = 0; j < NC; ++j) pn[c][j] += Q(row[c]) * psi[r][j];
  }
#pragma unroll
  for (int c = 0; c < NX; ++c)
#pragma unroll
    for (int j = 0; j < NC; ++j) psi[c][j] = pn[c][j];
}

template <typename Q, typename R, int NX>
__device__ __forceinline__ void phi_transpose_times(const XV<R, NX>* Phi, const int s, const int64_t st, const unsigned p,
                                                    Q (&psi)[NX]) {
  Q col[NX][1];
#pragma unroll
  for (int c = 0; c < NX; ++c) col[c][0] = psi[c];
  phi_transpose_times(Phi, s, st, p, col);
#pragma unroll
  for (int c = 0; c < NX; ++c) psi[c] = col[c][0];
}

// ---- 3. the pivot step of sweep 1 ----------------------------------------------------------------------------------
// one step (k descending) of T = U D U^T, T the tridiagonal control-cost Hessian with off-diagonal -wd2; d_next = d_{k+1}.
// The caller tests d_k > 0.
template <typename R>
__device__ __forceinline__ void tridiag_pivot(const int kk, const int N, const R wu2, const R wd2, const R lam,
                                              const R d_next, R& ups, R& dk, R& inv_d) {
  const R nd = (kk < N - 1 ? R(1) : R(0)) + R(1);  // du rows touching u_k
  const R diag = wu2 + lam + wd2 * nd;
  ups = (kk < N - 1) ? (-wd2 / d_next) : R(0);
  dk = diag + wd2 * ups;
  inv_d = R(1) / dk;
}

// ---- 4. the other pieces of sweep 1 and of pass 1b, for the sensitivity kernels only ---------------------------------
// feedback_gain_kernel, plan_sensitivity_kernel, plan_vjp_kernel and plan_weight_vjp_kernel are made of these (the last
// without sweep1_init: plan_weight_vjp_kernels.hpp says why); each keeps its own loop over the controls (the Gamma
// prefetch with whatever else it prefetches, the w_k row, its stores).
// W: the wide type S is carried in; Q: the type of Psi and w_k (W in the wide QP, else R).
// Three things stay restated, measured with -Rpass-analysis=kernel-resource-usage under the product's flags:
//  * qp_ls_kernel uses none of this section.  Tried one at a time in that kernel, the rank-one update of S as a function
//    cost its float instantiations a wave per SIMD (4 states 166 -> 170 VGPRs, 3 -> 2 waves; 6 states 256 -> 256 + 96 AGPRs,
//    2 -> 1) and Psi <- Psi Phi_s the 6-state one (256 -> 256 + 14, 2 -> 1), with no arithmetic opcode changed.
//  * The rank-one update S += w_k w_k^T / d_k stays written out in the four sensitivity kernels too.  As a function
//    (W (&Sm)[NX][NX], const Q (&wk)[NX], R inv_d; also with __restrict__, with a rectangular guarded inner loop, with the
//    bound passed as an argument) every 4-state instantiation keeps its registers, but every 6-state one carries the lower
//    triangle of S twice through both loops (two sets of 21 phi nodes that no pass merges; the arithmetic is unchanged):
//    feedback_gain_kernel float plain 154 -> 213 VGPRs (3 -> 2 waves), float wide 242 -> 256 + 52 AGPRs (2 -> 1), double
//    256 + 4 -> 256 + 46; plan_vjp_kernel float 166 -> 225 (3 -> 2) and 244 -> 256 + 52 (2 -> 1); plan_weight_vjp_kernel float
//    plain 239 -> 256 + 82 (2 -> 1); plan_sensitivity_kernel float wide 256 + 22 -> 256 + 50 with 2 VGPRs spilled.  A fix to
//    that loop is to be made in five places: those four kernels and qp_ls_kernel.
//  * plan_sensitivity_kernel restates pass1b_step for its NX and its 2 columns (feedback_gain_kernel and
//    plan_weight_vjp_kernel call it): its figures are in plan_sensitivity_kernels.hpp.

// S = 0, Psi = diag(w) (Psi_{S-1}: the terminal rows themselves), w_N = 0
template <typename R, typename W, typename Q, int NX>
__device__ __forceinline__ void sweep1_init(const R (&Rw)[NX], W (&Sm)[NX][NX], Q (&Psi)[NX][NX], Q (&wk)[NX]) {
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int j = 0; j < NX; ++j) Sm[i][j] = Wide<W>::of(R(0));
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = 0; c < NX; ++c) Psi[r][c] = (r == c) ? Q(Rw[r]) : Q(0);
#pragma unroll
  for (int r = 0; r < NX; ++r) wk[r] = Q(0);
}

// Psi <- Psi Phi_s, row by row of Phi_s from the workspace, the sums from zero
template <typename Q, typename R, int NX>
__device__ __forceinline__ void psi_times_phi(Q (&Psi)[NX][NX], const XV<R, NX>* Phi, const int s, const int64_t st,
                                              const unsigned p) {
  Q T[NX][NX];
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = 0; c < NX; ++c) T[r][c] = Q(0);
#pragma unroll
  for (int m = 0; m < NX; ++m) {
    R row[NX];
    unpack<R, NX>(Phi[(int64_t)(NX * s + m) * st + p], row);
#pragma unroll
    for (int r = 0; r < NX; ++r)
#pragma unroll
      for (int c = 0; c < NX; ++c) T[r][c] += Psi[r][m] * Q(row[c]);
  }
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = 0; c < NX; ++c) Psi[r][c] = T[r][c];
}

// one control of pass 1b (wide QP, k descending) for NC right-hand sides at once: om_j <- psi_j . Gamma_k - upsilon_k om_j,
// which is w_k . v_j when psi_j = Psi_s^T v_j and om_j was w_{k+1} . v_j
template <typename W, typename R, int NX, int NC>
__device__ __forceinline__ void pass1b_step(const W (&psi)[NX][NC], const R (&gk)[NX], const W ups, W (&om)[NC]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    W pg = psi[0][j] * (W)gk[0];
#pragma unroll
    for (int m = 1; m < NX; ++m) pg += psi[m][j] * (W)gk[m];
    om[j] = pg - ups * om[j];
  }
}

}  // namespace cpmpc
