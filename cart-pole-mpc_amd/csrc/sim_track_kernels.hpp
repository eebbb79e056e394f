// sim_track_kernels.hpp -- tracking a plant trajectory between two re-plans: the time-varying LQR gains along it in one kernel,
// and the plant rolled under an affine feedback law in one kernel.  The plant has ONE input, so the discrete Riccati recursion
// inverts no matrix: a tick's gain is a vector divided by a scalar.
//
// sim_lqr_kernel: REVERSE over the ticks, FORWARD inside a tick, as sim_rollout_vjp_kernel is organised.  With
// x_t = (t == 0) ? x0 : xs[t-1] (a forward call's checkpoints; row T-1 is never loaded), Phi_t = dx+/dx and gamma_t = dx+/du of
// the tick at (x_t, u[t]) from sim_jac_tick.inc, the state weights q, the control weight r > 0 and the terminal cost P_T,
//     P = P_T
//     for t = T-1 .. 0:
//         v   = P gamma_t
//         s   = r + gamma_t . v
//         k_t = -(Phi_t^T v) / s                          -> K[t]: u = u_nom + k_t . d
//         Acl = Phi_t + gamma_t k_t^T
//         P   = diag(q) + r k_t k_t^T + Acl^T P Acl        the lower triangle only
//     P0 = P
// This is the Joseph-like form of the Riccati step: a sum of positive semidefinite terms, so P stays positive semidefinite in
// rounded arithmetic where the textbook form P - (..)(..)^T / s subtracts two nearly equal matrices.  Only the lower triangle
// of P is computed and kept, (j, k <= j) at tri(j, k) (sim_window.hpp), so P is symmetric by construction; the products
// Phi^T v and Phi + gamma k^T take the closed-form columns of Phi as the 0, 1 and t_sum they are (ekf_add_term).  P lives in
// lane-private LDS, acc[field][threadIdx.x], while the sub-step loop runs, as the filter's P does: what is live there is
// sim_jac_kernel's set.  Everything is computed whichever outputs are stored (wave-uniform pointer tests), so each is bitwise the
// same whatever else is asked for, and a window of T1 + T2 ticks is bitwise the T2-tick tail's P0 fed as PT into the T1-tick
// head: P0 leaves by sim_store_sym.inc from the triangle PT's is read into.  n_sub == 0 is the identity plant with gamma = 0:
// k_t = 0 and P += diag(q), written as that.  Not modelled: the clamp of the control, feedback inside a tick, cross terms of
// the cost.
//
// sim_rollout_fb_kernel: sim_rollout_kernel's loop with the tick's control formed at the tick's start and held over its
// sub-steps,
//     d   = wrap_residual(x_t - x_nom_t)                  x_nom_0 = x0_nom, x_nom_t = xs_nom[t-1]; row T-1 is never loaded
//     u_t = clamp(u_nom[t] + K[t] . d, +-u_limit)         -> us[t]
//     x_{t+1} = Step(x_t, u_t, dt)                        plant_sub_step, the function sim_rollout_kernel's loop calls
// With K == NULL the nominal trajectory is not read and u_t = clamp(u_nom[t]); with u_limit = +inf the clamp returns its
// argument, so that call is sim_rollout_kernel bit for bit.  With x0 == x0_nom and the nominal trajectory's own parameters d is
// exactly 0 at every tick, K[t] . 0 adds nothing to a non-zero u_nom[t], and the call reproduces the nominal rollout bit for bit.
// A NaN control stays a NaN: clampr's comparisons are false for it.
#pragma once
#include "sim_ekf_kernels.hpp"

namespace cpmpc {

// q: the state weights; qf: the terminal diagonal, read where PT is NULL.  PT [NX*NX][B]: its lower triangle (fields
// j*NX + k, k <= j) is read.  Outputs, each written only where its pointer is given: K [T][NX][B], row t the gain of tick t;
// P0 [NX*NX][B], full, (j, k) and (k, j) from the one kept value.  PER_LANE as sim_jac_kernel's.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_lqr_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg,
                                                      ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
                                                      const R* x0, const R* u, const R* xs_in, StateWeights<R, M::NX> q, R rw,
                                                      const R* PT, StateWeights<R, M::NX> qf, R* K_out, R* P0_out) {
  constexpr int NX = M::NX, NQ = M::NQ;
  constexpr unsigned TRIV = trivial_cols<NX, NQ>(JaZeroCols<M>::value);  // sim_jac_kernel's closed-form columns
  constexpr int NH = tri(NX, 0);  // P's lower triangle, (j, k <= j) at tri(j, k)
  __shared__ R acc[NH][64];
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);

#pragma unroll
  for (int j = 0; j < NX; ++j)
#pragma unroll
    for (int kk = 0; kk <= j; ++kk)
      acc[tri(j, kk)][lane] = PT ? PT[(j * NX + kk) * B + p] : (kk == j ? qf.w[j] : R(0));

#pragma unroll 1
  for (int t = T - 1; t >= 0; --t) {
    if (n_sub == 0) {  // the identity plant, gamma = 0: no gain, and P takes the tick's state cost
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        if (K_out) K_out[((int64_t)t * NX + j) * B + p] = R(0);
        acc[tri(j, j)][lane] += q.w[j];
      }
      continue;
    }
    const R* xt = (t == 0) ? x0 : xs_in + (int64_t)(t - 1) * NX * B;
    const R uu = u[(int64_t)t * B + p];
    R xs[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) xs[r] = xt[r * B + p];
#include "sim_jac_tick.inc"  // Phi, gam, t_sum of the tick

    R Pm[NH];
#pragma unroll
    for (int f = 0; f < NH; ++f) Pm[f] = acc[f][lane];
    // ---- v = P gamma, s = r + gamma . v, k = -(Phi^T v) / s
    R v[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R a = Pm[tri_sym(j, 0)] * gam[0];
#pragma unroll
      for (int l = 1; l < NX; ++l) a += Pm[tri_sym(j, l)] * gam[l];
      v[j] = a;
    }
    R s = rw;
#pragma unroll
    for (int l = 0; l < NX; ++l) s += gam[l] * v[l];
    R kt[NX];
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      bool have = false;
      R w = R(0);
#pragma unroll
      for (int l = 0; l < NX; ++l) ekf_add_term<R, NX, NQ, TRIV>(Phi, t_sum, l, c, v[l], have, w);
      kt[c] = -(w / s);
    }
    if (K_out)
#pragma unroll
      for (int c = 0; c < NX; ++c) K_out[((int64_t)t * NX + c) * B + p] = kt[c];
    // ---- Acl = Phi + gamma k^T, dense
    R Acl[NX][NX];
#pragma unroll
    for (int l = 0; l < NX; ++l)
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        const R g = gam[l] * kt[c];
        Acl[l][c] = struct_zero<NX, NQ>(TRIV, l, c) ? g : phi_entry<R, M>(Phi, t_sum, l, c) + g;
      }
    // ---- P = diag(q) + r k k^T + Acl^T P Acl, a row of Acl^T P at a time
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R row[NX];  // row j of Acl^T P
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        R a = Acl[0][j] * Pm[tri_sym(0, c)];
#pragma unroll
        for (int l = 1; l < NX; ++l) a += Acl[l][j] * Pm[tri_sym(l, c)];
        row[c] = a;
      }
#pragma unroll
      for (int kk = 0; kk <= j; ++kk) {
        R a = row[0] * Acl[0][kk];
#pragma unroll
        for (int l = 1; l < NX; ++l) a += row[l] * Acl[l][kk];
        a += rw * kt[j] * kt[kk];
        acc[tri(j, kk)][lane] = (kk == j) ? a + q.w[j] : a;
      }
    }
  }

  if (P0_out) {
    constexpr int NS = NX;
    R* const out = P0_out;
#include "sim_store_sym.inc"
  }
}

// K [T][NX][B] or NULL; x0_nom [NX][B] and xs_nom [T][NX][B] are read only where K is given.  Outputs, each written only where
// its pointer is given: xs_out [T][NX][B], x_final [NX][B], us_out [T][B] the controls applied.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_rollout_fb_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg,
                                                             ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
                                                             const R* x0, const R* u_nom, const R* K, const R* x0_nom,
                                                             const R* xs_nom, R u_limit, R* xs_out, R* x_final, R* us_out) {
  constexpr int NX = M::NX;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
  R xs[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) xs[r] = x0[r * B + p];
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    R uu = u_nom[(int64_t)t * B + p];
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
    typename M::StepCache chain;
#pragma unroll 1
    for (int i = 0; i < n_sub; ++i) plant_sub_step<R, M>(k, fe, i, n_sub, h_last, uu, xs, chain);
    if (xs_out)
#pragma unroll
      for (int r = 0; r < NX; ++r) xs_out[((int64_t)t * NX + r) * B + p] = xs[r];
  }
  if (x_final)
#pragma unroll
    for (int r = 0; r < NX; ++r) x_final[r * B + p] = xs[r];
}

}  // namespace cpmpc
