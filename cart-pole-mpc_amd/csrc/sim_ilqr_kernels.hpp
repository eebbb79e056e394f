// sim_ilqr_kernels.hpp -- one iteration of an iterative LQR on the plant's own tick map, as two kernels and a third that runs
// the line search between them in one launch: the backward Riccati
// pass with a feedforward term, the exact treatment of the control's box limit and the predicted cost change; and the forward
// pass that applies alpha . k_t and sums the cost on the device.  The plant has ONE input, so the box QP of control-limited DDP
// is a scalar clamp and, as in sim_lqr_kernel (sim_track_kernels.hpp), no matrix is inverted.
//
// The cost, sim_lqr's convention with no factor 1/2: with e_t = wrap_residual(x_t - xref_t), x_0 = x0, x_t = xs[t-1],
// xref_0 = x0_ref, xref_t = xs_ref[t-1] (row T-1 of xs_ref IS read: it is the terminal target),
//     J = sum_{t<T} (e_t^T diag(q) e_t + r (u_t - uref_t)^2) + e_T^T P_T e_T
//
// sim_ilqr_backward_kernel: sim_lqr_kernel's walk -- REVERSE over the ticks, FORWARD inside a tick, Phi_t and gamma_t from
// sim_jac_tick.inc at (x_t, u[t]) -- with g, HALF the gradient of the cost-to-go, carried beside P:
//     P = P_T ;  g = P_T e_T ;  dV1 = dV2 = 0 ;  hmax = 0
//     for t = T-1 .. 0:
//         v   = P gamma_t ;  s0 = r + gamma_t . v ;  s = s0 + mu            mu >= 0 per lane, NULL: 0
//         h   = r (u_t - uref_t) + gamma_t . g
//         k   = clamp(u_t - h / s, +-u_limit) - u_t                          -> kff[t]
//         K_t = (the clamp changed u_t - h / s) ? 0 : -(Phi_t^T v) / s        -> K[t]
//         dV1 += 2 k h ;  dV2 += k^2 s0 ;  hmax = max(hmax, |k| s)
//         Acl = Phi_t + gamma_t K_t^T
//         g   = q o e_t + r (u_t - uref_t + k) K_t + Acl^T (g + v k)
//         P   = diag(q) + r K_t K_t^T + Acl^T P Acl                           the lower triangle only, as sim_lqr_kernel
//     P0 = P ;  g0 = g
// alpha dV1 + alpha^2 dV2 is the predicted change of J for a step alpha.  The P and g updates are the cost of the affine policy
// du = k + K_t dx in the linear-quadratic model and hold for ANY k and K_t, so P stays a sum of positive semidefinite terms
// under mu and under the clamp.  The P and K arithmetic is sim_lqr_kernel's own text, the parts of
// sim_riccati.inc; what is written here is the iLQR's alone: g, h, the scalar box QP, the three sums, the reference's loads
// and the zero gain of a held control.  So with mu NULL and no limit K and P0 are sim_lqr's bit for bit.
// x_T is xs[T-1]; where xs is NULL (allowed for T == 1) it is rolled from x0 by plant_sub_step, the rollout's own function.
// P's triangle, g, and the three running sums live in lane-private LDS, acc[field][threadIdx.x], while the sub-step loop runs:
// what is live there is sim_jac_kernel's set; x_t is loaded again after the tick for e_t.  Everything is computed whichever
// outputs are stored (wave-uniform pointer tests).  n_sub == 0 is the identity plant with gamma = 0: K_t = 0,
// k = clamp(u - (u - uref) r / (r + mu)) - u, g += q o e_t, P += diag(q), written as that.  Not modelled: second-order terms of
// the dynamics (this is Gauss-Newton), cross terms of the cost, feedback inside a tick.
//
// sim_ilqr_forward_kernel: the one body of the forward kernels, sim_roll_ticks.inc, with its law and
// its cost both compiled in -- sim_rollout_fb_kernel's loop with a per-lane step on the feedforward term and the cost summed,
//     u_t = clamp(u_nom[t] + alpha[p] kff[t] + K[t] . wrap_residual(x_t - x_nom_t), +-u_limit)
//     x_{t+1} = Step(x_t, u_t, dt)                                            plant_sub_step
//     cost = J of (x0, xs, us) against the reference
// kff and K are each nullable; with both NULL and u_limit = +inf it is sim_rollout_kernel bit for bit, with its cost.  alpha
// NULL means 1.  From the nominal start with alpha = 0 the deviation is exactly 0 at every tick and the nominal controls (a
// forward call's own, already inside the limit) and states come back bit for bit.
//
// sim_ilqr_search_kernel: the same body with its third part compiled in -- the whole line search of an iteration in one launch,
// one problem per lane, nothing crossing lanes.  The nominal start is x0 itself (a line search compares costs from one start):
//     alpha = 1 ; accepted = false
//     for j in 0 .. trials-1 while not accepted:
//         roll T ticks under the law above, summing J_try           the roll stores xs, us as it goes, for this lane only
//         pred = dV1 alpha + dV2 alpha^2
//         accepted = pred < 0 and J_try - cost_nom <= armijo pred
//         if not accepted: alpha = alpha / 2
//     accepted: xs, us, x_final are in place ; cost = J_try ; alpha_out = alpha
//     else:     xs = xs_nom, us = u_nom, x_final = xs_nom[T-1], cost = cost_nom, alpha_out = 0            (a copy)
// The ladder only halves, so alpha is a power of two: dV1 alpha and dV2 alpha alpha are exact and pred rounds once whether or
// not the compiler contracts it; J_try - cost_nom and armijo pred are each rounded on their own and compared.  The decision is
// therefore, bit for bit, the one a ladder of sim_ilqr_forward_kernel calls with elementwise arithmetic between them takes,
// and an accepted lane's outputs are that kernel's at the lane's alpha.  A decided lane is masked off and the wave leaves with
// its last lane; trials <= 32 bounds the run time.  Outputs may not overlap inputs, so a rejected trial's stores are simply
// overwritten.  A FAILED LANE KEEPS ITS NOMINAL BY COPY: for finite data that is what a forward call with alpha = 0 yields (the
// identity above); it differs on purpose where kff, K or dV of a lane is not finite while its nominal is: alpha = 0 would
// poison such a lane through 0 . NaN, the search fails it and it keeps its trajectory for a retry under a larger mu.  A lane
// whose nominal or cost_nom is itself non-finite returns that.  No lane affects another.
#pragma once
#include "sim_track_kernels.hpp"

namespace cpmpc {

// m = max(m, a), a NaN kept: the lane's stationarity measure is then a NaN too
template <typename R>
__device__ __forceinline__ void ilqr_running_max(R& m, R a) {
  if (!(a <= m)) m = a;
}

// x0, u [T][B], xs_in [T][NX][B] (NULL allowed for T == 1): the trajectory.  x0_ref [NX][B], xs_ref [T][NX][B], u_ref [T][B] or
// NULL (zeros): the reference.  mu [B] or NULL.  PT [NX*NX][B] (lower triangle read) or NULL: diag(qf).  Outputs, each written
// only where its pointer is given: K [T][NX][B], kff [T][B], dV [2][B], P0 [NX*NX][B] full, g0 [NX][B], hmax [B].
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_ilqr_backward_kernel(
    int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg, ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
    const R* x0, const R* u, const R* xs_in, const R* x0_ref, const R* xs_ref, const R* u_ref, StateWeights<R, M::NX> q, R rw,
    const R* PT, StateWeights<R, M::NX> qf, const R* mu_in, R u_limit, R* K_out, R* kff_out, R* dV_out, R* P0_out, R* g0_out,
    R* hmax_out) {
  constexpr int NX = M::NX, NQ = M::NQ;
  constexpr unsigned TRIV = trivial_cols<NX, NQ>(JaZeroCols<M>::value);  // sim_jac_kernel's closed-form columns
  constexpr int NH = tri(NX, 0);  // P's lower triangle, (j, k <= j) at tri(j, k); then g, then dV1, dV2, hmax
  constexpr int F_G = NH, F_DV1 = NH + NX, F_DV2 = NH + NX + 1, F_HMAX = NH + NX + 2;
  __shared__ R acc[NH + NX + 3][64];
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
  const R mu = mu_in ? mu_in[p] : R(0);

  {  // P = P_T, g = P_T e_T
    R e[NX];
    if (xs_in) {
#pragma unroll
      for (int r = 0; r < NX; ++r) e[r] = xs_in[((int64_t)(T - 1) * NX + r) * B + p];
    } else {  // T == 1: x_1 by the rollout's own sub-step
#pragma unroll
      for (int r = 0; r < NX; ++r) e[r] = x0[r * B + p];
      const R uu = u[p];
      typename M::StepCache chain;
#pragma unroll 1
      for (int i = 0; i < n_sub; ++i) plant_sub_step<R, M>(k, fe, i, n_sub, h_last, uu, e, chain);
    }
#pragma unroll
    for (int r = 0; r < NX; ++r) e[r] -= xs_ref[((int64_t)(T - 1) * NX + r) * B + p];
    wrap_residual<R, M>(e);
    R Pm[NH];
#pragma unroll
    for (int j = 0; j < NX; ++j)
#pragma unroll
      for (int kk = 0; kk <= j; ++kk) {
        Pm[tri(j, kk)] = PT ? PT[(j * NX + kk) * B + p] : (kk == j ? qf.w[j] : R(0));
        acc[tri(j, kk)][lane] = Pm[tri(j, kk)];
      }
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R a = Pm[tri_sym(j, 0)] * e[0];
#pragma unroll
      for (int l = 1; l < NX; ++l) a += Pm[tri_sym(j, l)] * e[l];
      acc[F_G + j][lane] = a;
    }
    acc[F_DV1][lane] = R(0);
    acc[F_DV2][lane] = R(0);
    acc[F_HMAX][lane] = R(0);
  }

#pragma unroll 1
  for (int t = T - 1; t >= 0; --t) {
    const R* xt = (t == 0) ? x0 : xs_in + (int64_t)(t - 1) * NX * B;
    const R* xr = (t == 0) ? x0_ref : xs_ref + (int64_t)(t - 1) * NX * B;
    const R uu = u[(int64_t)t * B + p];
    if (n_sub == 0) {  // the identity plant, gamma = 0: no gain, the control's own quadratic, and P, g take the tick's state cost
      const R du = uu - (u_ref ? u_ref[(int64_t)t * B + p] : R(0));
      const R s = rw + mu, h = rw * du;
      const R un = uu - du * rw / s;
      const R kf = clampr(un, -u_limit, u_limit) - uu;
      if (kff_out) kff_out[(int64_t)t * B + p] = kf;
      acc[F_DV1][lane] += R(2) * kf * h;
      acc[F_DV2][lane] += kf * kf * rw;
      ilqr_running_max(acc[F_HMAX][lane], Math<R>::fabs(kf) * s);
      R e[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) e[r] = xt[r * B + p] - xr[r * B + p];
      wrap_residual<R, M>(e);
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        if (K_out) K_out[((int64_t)t * NX + j) * B + p] = R(0);
        acc[tri(j, j)][lane] += q.w[j];
        acc[F_G + j][lane] += q.w[j] * e[j];
      }
      continue;
    }
    R xs[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) xs[r] = xt[r * B + p];
#include "sim_jac_tick.inc"  // Phi, gam, t_sum of the tick

    R Pm[NH];
#pragma unroll
    for (int f = 0; f < NH; ++f) Pm[f] = acc[f][lane];
    R gv[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) gv[j] = acc[F_G + j][lane];
    const R du = uu - (u_ref ? u_ref[(int64_t)t * B + p] : R(0));
    // ---- v = P gamma, s0 = r + gamma . v, s = s0 + mu, h = r du + gamma . g
#define CPMPC_RICCATI_V_S0
#include "sim_riccati.inc"
    const R s = s0 + mu;
    R h = rw * du;
#pragma unroll
    for (int l = 0; l < NX; ++l) h += gam[l] * gv[l];
    // ---- the scalar box QP: the unconstrained minimiser clamped; a control on its limit takes no feedback
    const R un = uu - h / s;
    const R uc = clampr(un, -u_limit, u_limit);
    const bool held = uc != un;
    const R kf = uc - uu;
    if (kff_out) kff_out[(int64_t)t * B + p] = kf;
    acc[F_DV1][lane] += R(2) * kf * h;
    acc[F_DV2][lane] += kf * kf * s0;
    ilqr_running_max(acc[F_HMAX][lane], Math<R>::fabs(kf) * s);
#define CPMPC_RICCATI_GAIN(k) (held ? R(0) : (k))
#define CPMPC_RICCATI_GAIN_ACL
#include "sim_riccati.inc"
#undef CPMPC_RICCATI_GAIN
    // ---- g = q o e_t + r (du + k) K + Acl^T (g + v k)
    {
      R e[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) e[r] = xt[r * B + p] - xr[r * B + p];
      wrap_residual<R, M>(e);
      const R ru = rw * (du + kf);
#pragma unroll
      for (int l = 0; l < NX; ++l) gv[l] += v[l] * kf;
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        R a = Acl[0][c] * gv[0];
#pragma unroll
        for (int l = 1; l < NX; ++l) a += Acl[l][c] * gv[l];
        acc[F_G + c][lane] = q.w[c] * e[c] + ru * kt[c] + a;
      }
    }
#define CPMPC_RICCATI_UPDATE
#include "sim_riccati.inc"
  }

  if (g0_out)
#pragma unroll
    for (int j = 0; j < NX; ++j) g0_out[j * B + p] = acc[F_G + j][lane];
  if (dV_out) {
    dV_out[p] = acc[F_DV1][lane];
    dV_out[B + p] = acc[F_DV2][lane];
  }
  if (hmax_out) hmax_out[p] = acc[F_HMAX][lane];
  if (P0_out) {
    constexpr int NS = NX;
    R* const out = P0_out;
#include "sim_store_sym.inc"
  }
}

// e^T P e with P's lower triangle in Pm (tri), or sum qf e^2 where there is no tensor: the terminal cost of sim_roll_ticks.inc
template <typename R, int NX>
__device__ __forceinline__ R ilqr_quad_tri(const R (&Pm)[tri(NX, 0)], const R (&e)[NX]) {
  R a = R(0);
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    R row = R(0);
#pragma unroll
    for (int kk = 0; kk < j; ++kk) row += Pm[tri(j, kk)] * e[kk];
    a += e[j] * (R(2) * row + Pm[tri(j, j)] * e[j]);
  }
  return a;
}

// kff [T][B], K [T][NX][B], alpha [B]: each or NULL; x0_nom [NX][B] and xs_nom [T][NX][B] are read only where K is given (row
// T-1 never).  The reference and the weights as the backward kernel's.  Outputs, each written only where its pointer is given:
// xs_out [T][NX][B], x_final [NX][B], us_out [T][B] the controls applied, cost_out [B].
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_ilqr_forward_kernel(
    int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg, ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
    const R* x0, const R* u_nom, const R* kff, const R* K, const R* x0_nom, const R* xs_nom, const R* alpha_in, R u_limit,
    const R* x0_ref, const R* xs_ref, const R* u_ref, StateWeights<R, M::NX> q, R rw, const R* PT, StateWeights<R, M::NX> qf,
    R* xs_out, R* x_final, R* us_out, R* cost_out) {
#define CPMPC_ROLL_LAW 1
#define CPMPC_ROLL_COST 1
#define CPMPC_ROLL_SEARCH 0
#include "sim_roll_ticks.inc"
}

// The nominal trajectory x0, u_nom [T][B], xs_nom [T][NX][B] (ALWAYS required: row T-1 is read for a failed lane's copy) and its
// cost cost_nom [B]; the backward pass's kff [T][B], K [T][NX][B] or NULL, dV [2][B]; the reference and the weights as the
// forward kernel's; trials in 1..32 and armijo by value.  Outputs, each written only where its pointer is given and none
// overlapping an input: xs_out [T][NX][B], x_final [NX][B], us_out [T][B], cost_out [B], alpha_out [B] the step taken, 0: none.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_ilqr_search_kernel(
    int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg, ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
    const R* x0, const R* u_nom, const R* xs_nom, const R* cost_nom, const R* kff, const R* K, const R* dV, int trials, R armijo,
    R u_limit, const R* x0_ref, const R* xs_ref, const R* u_ref, StateWeights<R, M::NX> q, R rw, const R* PT,
    StateWeights<R, M::NX> qf, R* xs_out, R* x_final, R* us_out, R* cost_out, R* alpha_out) {
#define CPMPC_ROLL_LAW 1
#define CPMPC_ROLL_COST 1
#define CPMPC_ROLL_SEARCH 1
#include "sim_roll_ticks.inc"
}

}  // namespace cpmpc
