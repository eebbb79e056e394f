// sim_window.hpp -- what the plant's derivative and window kernels do alike, one definition each.  Here the
// register-only pieces, as __forceinline__ functions.  The pieces that address memory are TEXTS, each naming what it expects
// in scope, because as functions they moved registers, spills and occupancy of kernels at the register limit:
// sim_phi_step.inc (Phi <- A Phi), sim_window_residual.inc, sim_normal_eq.inc (g, H of a tick), sim_store_sym.inc.
#pragma once
#include "plant_kernels.hpp"

namespace cpmpc {

// Entry (j, k <= j) of a symmetric matrix kept as its lower triangle, row after row; tri_sym takes the pair in either order.
__host__ __device__ constexpr int tri(int j, int k) { return j * (j + 1) / 2 + k; }
__host__ __device__ constexpr int tri_sym(int a, int b) { return a >= b ? tri(a, b) : tri(b, a); }

// What the Kalman filter's recording form stores per tick for the smoother's backward pass, as rows of B numbers from the
// tick's base row t * ROWS: x- (NX), P- before the update (packed triangle, NH), A P (NX*NX, row j at AP + j*NX), the
// filtered x (NX) and the filtered P (NH).  ROWS = 2 NX + 2 NH + NX^2: 44 for the 4-state model, 90 for the 6-state model.
template <int NX>
struct RtsRecord {
  static constexpr int NH = tri(NX, 0);
  static constexpr int XM = 0, PM = NX, AP = NX + NH, XF = NX + NH + NX * NX, PF = XF + NX, ROWS = PF + NH;
};

// the residual weights of the states, in the kernel's scalar type
template <typename R, int NX>
struct StateWeights {
  R w[NX];
};

// The pole angles of a residual to [-pi, pi], by the NEAREST multiple of 2 pi: a residual inside that range, which is every one
// of a sensible fit, comes back bit for bit.  (wrap_angles sends a small negative angle through + 2 pi - 2 pi, which costs a
// residual of 0.05 rad five of a float's digits: mod_pi is made for angles, where an error of eps pi is the format's own.)
template <typename R, typename M>
__device__ __forceinline__ void wrap_residual(R (&r)[M::NX]) {
  constexpr R two_pi = static_cast<R>(2 * 3.14159265358979323846);
  constexpr R inv_two_pi = static_cast<R>(0.15915494309189533577);
#pragma unroll
  for (int t = 1; t < M::NQ; ++t) {
    R n;
    if constexpr (sizeof(R) == 4) n = __builtin_rintf(r[t] * inv_two_pi);
    else n = __builtin_rint(r[t] * inv_two_pi);
    r[t] = Math<R>::fma(-n, two_pi, r[t]);
  }
}

// The predicates of sim_normal_eq.inc, "entry q of column j is an exact zero": NeverZero for dense columns, PhiZero for a
// product of step Jacobians with the closed-form columns TRIV (models.hpp: struct_zero)
struct NeverZero {
  static constexpr bool zero(int, int) { return false; }
};
template <int NX, int NQ, unsigned TRIV>
struct PhiZero {
  static constexpr bool zero(int q, int j) { return struct_zero<NX, NQ>(TRIV, q, j); }
};

// Phi = dx/dx of a product of step Jacobians of model M.  Its closed-form columns (models.hpp: trivial_cols) are neither
// stored nor propagated: column c stays e_c, plus t_sum -- the sub-steps' lengths added up by the caller -- in row c - NQ
// when c is a velocity.  phi_identity: the other columns to those of I.
template <typename R, typename M>
__device__ __forceinline__ void phi_identity(R (&Phi)[M::NX][M::NX]) {
  constexpr int NX = M::NX;
  constexpr unsigned TRIV = trivial_cols<NX, M::NQ>(JaZeroCols<M>::value);
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (!((TRIV >> c) & 1u)) Phi[r][c] = (r == c) ? R(1) : R(0);
}

// Entry (r, c) of Phi, the closed-form columns as they are known: for the stores of Phi in full, [NX*NX][B] with element
// (r, c) at field r*NX + c (the layout of rk4_kernel); r and c are the constants of an unrolled loop
template <typename R, typename M>
__device__ __forceinline__ R phi_entry(const R (&Phi)[M::NX][M::NX], const R t_sum, int r, int c) {
  constexpr int NX = M::NX, NQ = M::NQ;
  constexpr unsigned TRIV = trivial_cols<NX, NQ>(JaZeroCols<M>::value);
  if ((TRIV >> c) & 1u) return (r == c) ? R(1) : ((c >= NQ && r == c - NQ) ? t_sum : R(0));
  return Phi[r][c];
}

}  // namespace cpmpc
