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
// the cost.  The step's arithmetic is written once, as the parts of sim_riccati.inc, and sim_ilqr_backward_kernel
// (sim_ilqr_kernels.hpp) is made of the same parts: with no regularisation and no limit the iLQR's K and P0 are this kernel's bit for bit because they
// are this kernel's text, and a change to the step (a gT beside PT) is made in one place.
//
// sim_rollout_fb_kernel: sim_rollout_kernel's body, sim_roll_ticks.inc, with its law compiled in: the
// tick's control is formed at the tick's start and held over its sub-steps,
//     d   = wrap_residual(x_t - x_nom_t)                  x_nom_0 = x0_nom, x_nom_t = xs_nom[t-1]; row T-1 is never loaded
//     u_t = clamp(u_nom[t] + K[t] . d, +-u_limit)         -> us[t]
//     x_{t+1} = Step(x_t, u_t, dt)                        plant_sub_step, in the one loop all three forward kernels run
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
#define CPMPC_RICCATI_V_S0
#include "sim_riccati.inc"
    const R s = s0;
#define CPMPC_RICCATI_GAIN(k) (k)
#define CPMPC_RICCATI_GAIN_ACL
#include "sim_riccati.inc"
#undef CPMPC_RICCATI_GAIN
#define CPMPC_RICCATI_UPDATE
#include "sim_riccati.inc"
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
  const R *const kff = nullptr, *const alpha_in = nullptr;  // the iLQR's feedforward term: none here
#define CPMPC_ROLL_LAW 1
#define CPMPC_ROLL_COST 0
#define CPMPC_ROLL_SEARCH 0
#include "sim_roll_ticks.inc"
}

}  // namespace cpmpc
