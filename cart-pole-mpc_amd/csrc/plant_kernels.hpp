// plant_kernels.hpp -- the plant on its own, outside the SQP pipeline (mpc_kernels.hpp): the dynamics and one RK4 step as
// stand-alone kernels, and Simulator::Step for a batch with what the plant's derivative and window kernels (sim_*.hpp)
// build on: PlantConsts, load_ext_force, plant_sub_step.  One problem per lane, arrays packed [field][B].
#pragma once
#include "models.hpp"

namespace cpmpc {

// ------------------------------------------------------------------------------------------------
// stand-alone pieces (parity tests, callers that want them); arrays packed [field][B]
// ------------------------------------------------------------------------------------------------
template <typename R, typename M>
__global__ __launch_bounds__(64) void dynamics_kernel(int64_t B, typename M::Consts k, ExtForce<R> fe,
                                                       const R* x, const R* u, R* f, R* Jx, R* Ju) {
  constexpr int NX = M::NX, NQ = M::NQ;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  R xs[NX], acc[NQ], Ja[NQ][NX], Jua[NQ];
#pragma unroll
  for (int t = 0; t < NX; ++t) xs[t] = x[t * B + p];
  M::template accel<true, true>(k, xs, u[p], fe, acc, Ja, Jua);
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    f[i * B + p] = xs[NQ + i];
    f[(NQ + i) * B + p] = acc[i];
  }
  if (Jx) {
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        Jx[(i * NX + c) * B + p] = (c == NQ + i) ? R(1) : R(0);
        Jx[((NQ + i) * NX + c) * B + p] = Ja[i][c];
      }
  }
  if (Ju) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      Ju[i * B + p] = R(0);
      Ju[(NQ + i) * B + p] = Jua[i];
    }
  }
}

template <typename R, typename M>
__global__ __launch_bounds__(64) void rk4_kernel(int64_t B, typename M::Consts k, ExtForce<R> fe, R h,
                                                  const R* x, const R* u, R* xn, R* A, R* Bm) {
  constexpr int NX = M::NX;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  R xs[NX];
#pragma unroll
  for (int t = 0; t < NX; ++t) xs[t] = x[t * B + p];
  if (A != nullptr || Bm != nullptr) {
    R Am[NX][NX], Bv[NX];
    rk4_step_jac_m<R, M, true>(k, h, xs, u[p], fe, Am, Bv);
    if (A)
#pragma unroll
      for (int r = 0; r < NX; ++r)
#pragma unroll
        for (int c = 0; c < NX; ++c) A[(r * NX + c) * B + p] = Am[r][c];
    if (Bm)
#pragma unroll
      for (int r = 0; r < NX; ++r) Bm[r * B + p] = Bv[r];
  } else {
    rk4_step_m<R, M, true>(k, h, xs, u[p], fe);
  }
#pragma unroll
  for (int t = 0; t < NX; ++t) xn[t * B + p] = xs[t];
}

// The plant kernels' dynamics constants: the shared set's, folded on the host (a kernel argument, as it has always been), or
// -- PER_LANE -- per-problem parameters dyn [NP][B], read by each lane and folded in the kernel as load_consts does.
template <typename R, typename M, bool PER_LANE>
struct PlantConsts {
  using Arg = typename M::Consts;
  __device__ __forceinline__ static const Arg& get(const Arg& k, int64_t, int64_t) { return k; }
};
template <typename R, typename M>
struct PlantConsts<R, M, true> {
  using Arg = const R*;
  __device__ __forceinline__ static typename M::Consts get(const R* dyn, int64_t B, int64_t p) {
    R prm[M::NP];
#pragma unroll
    for (int i = 0; i < M::NP; ++i) prm[i] = dyn[i * B + p];
    return M::template make<R>(prm);
  }
};

// The external forces of a lane: `fe` holds the shared set's and -- where fext [4][B] is given -- takes the lane's own (row 1
// is not read).  In place: returned by value, the same loads come out as other instructions in some instantiations.
template <typename R>
__device__ __forceinline__ void load_ext_force(const R* fext, int64_t B, int64_t p, ExtForce<R>& fe) {
  if (fext) {
    fe.fbx = fext[p];
    fe.fmx = fext[2 * B + p];
    fe.fmy = fext[3 * B + p];
  }
}

// Sub-step i of n_sub of one tick of the plant, Simulator::Step (simulator.cc:11-36): an RK4 step of 1 ms, the last one of
// h_last, the control held, the angles wrapped.  The host evaluates the reference's `while (dt > 0) { SubStep(min(dt, 0.001));
// dt -= 0.001; }` in double and passes the count and the last step, so f32 and f64 take the same sub-steps.  `chain` is the
// tick's: a fresh StepCache before sub-step 0.
template <typename R, typename M>
__device__ __forceinline__ void plant_sub_step(const typename M::Consts& k, const ExtForce<R>& fe, int i, int n_sub, R h_last,
                                               R uu, R (&xs)[M::NX], typename M::StepCache& chain) {
  const R internal_dt = R(0.001);
  const R h = (i + 1 == n_sub) ? h_last : internal_dt;
  if (i % 8 == 0) chain.invalidate();  // (dead store: see TrigBase::valid)
  rk4_step_m<R, M, true>(k, h, xs, uu, fe, chain);
  wrap_angles<R, M>(xs);
}

template <typename R, typename M, bool PER_LANE = false>
__global__ __launch_bounds__(64) void sim_kernel(int64_t B, typename PlantConsts<R, M, PER_LANE>::Arg k_arg, ExtForce<R> fe_shared,
                                                  const R* fext, int n_sub, R h_last, const R* u, R* state) {
  constexpr int NX = M::NX;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const typename M::Consts k = PlantConsts<R, M, PER_LANE>::get(k_arg, B, p);
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
  R xs[NX];
#pragma unroll
  for (int t = 0; t < NX; ++t) xs[t] = state[t * B + p];
  const R uu = u[p];
  typename M::StepCache chain;
  for (int i = 0; i < n_sub; ++i) plant_sub_step<R, M>(k, fe, i, n_sub, h_last, uu, xs, chain);
#pragma unroll
  for (int t = 0; t < NX; ++t) state[t * B + p] = xs[t];
}

}  // namespace cpmpc
