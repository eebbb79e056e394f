// sim_rollout_kernels.hpp -- the plant over T ticks in one kernel, and its adjoint in one kernel:
//     x_{t+1} = Step(x_t, u_t, dt),  t = 0 .. T-1,
// Step being Simulator::Step (simulator.cc:11-36) exactly as sim_kernel runs it -- n_sub sub-steps of 1 ms, the last one
// h_last, the control held over the tick, the pole angles wrapped after each sub-step.  dt, the external forces and the
// dynamics parameters are those of every tick.  One problem per lane, no LDS; the tick loop stays on the device.
//
// sim_rollout_kernel: a tick is n_sub calls of plant_sub_step (plant_kernels.hpp), the function sim_kernel's loop calls; after
// tick t it stores x_{t+1} to xs [T][NX][B] (field t*NX + r) and after the last one to x_final [NX][B], each where its pointer
// is given (a wave-uniform choice).  Its body is sim_roll_ticks.inc, written once for this kernel, sim_rollout_fb_kernel
// (sim_track_kernels.hpp: the loop under a feedback law) and sim_ilqr_forward_kernel (sim_ilqr_kernels.hpp: the law and the
// cost); the law and the cost are compile-time parts of that text, and this kernel compiles neither.
//
// sim_rollout_vjp_kernel: REVERSE over the ticks, FORWARD inside a tick.  With the cotangents gbar [T][NX][B] on every
// x_{t+1} and / or gbar_final [NX][B] on x_T,
//     lambda = 0, gp = 0
//     for t = T-1 .. 0:
//         lambda += gbar[t]  (+= gbar_final at t = T-1)
//         x_t = (t == 0) ? x0 : xs[t-1]                       -- a forward call's checkpoints; row T-1 is never loaded
//         pass B: sim_param_tick.inc from x_t, every column         -> gp += P^T lambda   (where g_p is given)
//         pass A: sim_jac_tick.inc from x_t, then sim_jac_vjp.inc    -> g_u[t] = gamma . lambda,  lambda <- Phi^T lambda
//     g_x0 = lambda, g_p = gp
// lambda and gp stay in registers across the ticks.  The passes run one after the other (B before A, so that one copy of
// lambda serves both), so what is live at once is the larger of the two existing kernels' sets plus lambda and gp.
// Nothing per sub-step is stored; the adjoint of RK4 inside a tick is not built.  n_sub == 0 is the identity
// map: g_x0 is the cotangents added up in that order, g_u and g_p are zeros.  Not differentiated: the external forces and
// dt; the wrap has unit derivative.
//
// The two passes are the texts sim_param_jac_kernel and sim_jac_kernel are made of, included here (the .inc files say what
// they expect in scope); written as functions the same statements compile to other registers and spills.
#pragma once
#include "sim_param_kernels.hpp"

namespace cpmpc {

template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_rollout_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg,
                                                          ExtForce<R> fe_shared, const R* fext, int n_sub, R h_last, int T,
                                                          const R* x0, const R* u_nom, R* xs_out, R* x_final) {
#define CPMPC_ROLL_LAW 0
#define CPMPC_ROLL_COST 0
#define CPMPC_ROLL_SEARCH 0
#include "sim_roll_ticks.inc"
}

// PER_LANE: the parameters are dyn [NP][B], read per lane (sim_param_load.inc), and the constants are M::make<R> of them in
// the kernel, as sim_param_jac_kernel does; else `k_shared` and `raw` are the shared set's.
template <typename R, typename M, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_rollout_vjp_kernel(int64_t B, typename M::Consts k_shared, RawParams<R, M::NP> raw,
                                                              const R* dyn, ExtForce<R> fe_shared, const R* fext, int n_sub,
                                                              R h_last, int T, const R* x0, const R* u, const R* xs_in,
                                                              const R* gbar, const R* gbar_final, R* g_x0, R* g_u, R* g_p) {
  constexpr int NX = M::NX, NQ = M::NQ, NP = M::NP;
  constexpr unsigned TRIV = trivial_cols<NX, NQ>(JaZeroCols<M>::value);  // sim_jac_kernel's closed-form columns
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
  typename M::Consts k = k_shared;
  if constexpr (PER_LANE) {
    R prm[NP];  // not held: pass B reads them again
#include "sim_param_load.inc"
    k = M::template make<R>(prm);
  }

  R lam[NX], gp[NP];
#pragma unroll
  for (int r = 0; r < NX; ++r) lam[r] = R(0);
#pragma unroll
  for (int j = 0; j < NP; ++j) gp[j] = R(0);

#pragma unroll 1
  for (int t = T - 1; t >= 0; --t) {
    if (gbar)
#pragma unroll
      for (int r = 0; r < NX; ++r) lam[r] += gbar[((int64_t)t * NX + r) * B + p];
    if (gbar_final && t == T - 1)
#pragma unroll
      for (int r = 0; r < NX; ++r) lam[r] += gbar_final[r * B + p];
    if (n_sub == 0) {  // the identity map: the cotangent itself, not its products with ones and zeros
      if (g_u) g_u[(int64_t)t * B + p] = R(0);
      continue;
    }
    const R* xt = (t == 0) ? x0 : xs_in + (int64_t)(t - 1) * NX * B;
    const R uu = u[(int64_t)t * B + p];

    // ---- pass B: the parameter tangents of the tick, every column.  It runs FIRST: it needs the lambda pass A replaces,
    // and so no second copy of lambda is live beside the tangents --------------------------------------------------------
    if (g_p) {
      R prm[NP];  // the raw parameters, read here every tick rather than held across pass A
#include "sim_param_load.inc"
      R xs[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) xs[r] = xt[r * B + p];
      constexpr int J0 = 0, NG = NP;  // every column
#include "sim_param_tick.inc"  // Tn [NP][NX] of the tick
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        R acc = Tn[j][0] * lam[0];
#pragma unroll
        for (int r = 1; r < NX; ++r) acc += Tn[j][r] * lam[r];
        gp[j] += acc;
      }
    }
    // ---- pass A: Phi and gamma of the tick; lambda <- Phi^T lambda -----------------------------------------------------
    {
      R xs[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) xs[r] = xt[r * B + p];
#include "sim_jac_tick.inc"  // Phi, gam, t_sum of the tick
      const R (&g)[NX] = lam;  // the cotangent of the tick, under the name sim_jac_vjp.inc reads
      R lam_new[NX];
#define CPMPC_PHI_T_G(c) lam_new[c]
#include "sim_jac_vjp.inc"
#undef CPMPC_PHI_T_G
      if (g_u) {
        R acc = gam[0] * lam[0];
#pragma unroll
        for (int r = 1; r < NX; ++r) acc += gam[r] * lam[r];
        g_u[(int64_t)t * B + p] = acc;
      }
#pragma unroll
      for (int r = 0; r < NX; ++r) lam[r] = lam_new[r];
    }
  }

  if (g_x0)
#pragma unroll
    for (int r = 0; r < NX; ++r) g_x0[r * B + p] = lam[r];
  if (g_p)
#pragma unroll
    for (int j = 0; j < NP; ++j) g_p[j * B + p] = gp[j];
}

}  // namespace cpmpc
