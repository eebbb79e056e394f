// condensed_qp.hpp -- the blocks of the condensed QP that qp_ls_kernel (mpc_kernels.hpp) and feedback_gain_kernel
// (feedback_kernels.hpp) share.
//
// Every piece is a __forceinline__ function (or a struct of registers with two of them) on fixed-size arrays.  The order
// of operations of each piece is qp_ls_kernel's: the sums start from their first product where that kernel's did, from
// zero where its did, so the split pipeline's results do not move by a bit.  (The rest of sweep 1 is not here: see
// feedback_kernels.hpp.)
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

}  // namespace cpmpc
