// sim_ekf_body.inc -- the body of the Kalman filter's kernel over T ticks: one text for sim_ekf_kernel (RECORD false) and for
// sim_ekf_record_kernel (RECORD true), the smoother's forward pass, which additionally stores per tick what the backward pass
// reads (sim_window.hpp: RtsRecord) into work [T * ROWS][B].  The stores are the only difference, so x_final, P_final, xs and
// nis of the two are the same bit for bit by construction.
// Expects in scope: R, M, PER_LANE, the kernel's arguments of sim_ekf_kernel, the constant RECORD, and work (read only where
// RECORD).
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

  R xs[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) xs[r] = x0[r * B + p];
#pragma unroll
  for (int j = 0; j < NX; ++j)
#pragma unroll
    for (int kk = 0; kk <= j; ++kk) acc[tri(j, kk)][lane] = P0[(j * NX + kk) * B + p];
  R nis_sum = R(0);

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const R uu = u[(int64_t)t * B + p];
    // ---- predict: the tick's sub-step loop, Phi from I
    R Phi[NX][NX];
    phi_identity<R, M>(Phi);
    R t_sum = R(0);  // entry (c - NQ, c) of a trivial velocity column: the sub-steps' lengths of this tick
    {
      const R internal_dt = R(0.001);
      typename M::StepCache chain, chain_x;
#pragma unroll 1
      for (int i = 0; i < n_sub; ++i) {
        const R h = (i + 1 == n_sub) ? h_last : internal_dt;
        R A[NX][NX], Bv[NX], xj[NX];
        // The state moves by sim_rollout_kernel's own sub-step, so that a lane on which no update acts follows that kernel
        // bit for bit: rk4_step_jac_m evaluates the same stages beside their Jacobians, and the compiler contracts the two
        // texts differently (1 - 2 ulps a tick for the 6-state model).  A is the sub-step's Jacobian from the same state,
        // taken through an empty asm so that the two evaluations share no sub-expression and the state's stays the text
        // sim_rollout_kernel compiles; the state rk4_step_jac_m leaves in xj is dead.
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          xj[r] = xs[r];
          asm("" : "+v"(xj[r]));
        }
        plant_sub_step<R, M>(k, fe, i, n_sub, h_last, uu, xs, chain_x);
        rk4_step_jac_m<R, M, true>(k, h, xj, uu, fe, A, Bv, chain);
#include "sim_phi_step.inc"
        if (TRIV != 0u) t_sum += h;
      }
    }

    [[maybe_unused]] R* const rec = RECORD ? work + (int64_t)t * RtsRecord<NX>::ROWS * B + p : nullptr;  // the tick's record
    if constexpr (RECORD)
#pragma unroll
      for (int r = 0; r < NX; ++r) rec[(RtsRecord<NX>::XM + r) * B] = xs[r];

    // ---- P- = A P A^T + diag(q), a row of A P at a time; P is (j, k) -> Pm[tri_sym(j, k)]
    R Pm[NH], Pn[NH];
#pragma unroll
    for (int f = 0; f < NH; ++f) Pm[f] = acc[f][lane];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R row[NX];  // row j of A P
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        bool have = false;
        R s = R(0);
#pragma unroll
        for (int l = 0; l < NX; ++l)
          ekf_add_term<R, NX, NQ, TRIV>(Phi, t_sum, j, l, Pm[tri_sym(l, c)], have, s);
        row[c] = s;
        if constexpr (RECORD) rec[(RtsRecord<NX>::AP + j * NX + c) * B] = s;
      }
#pragma unroll
      for (int kk = 0; kk <= j; ++kk) {
        bool have = false;
        R s = R(0);
#pragma unroll
        for (int l = 0; l < NX; ++l) ekf_add_term<R, NX, NQ, TRIV>(Phi, t_sum, kk, l, row[l], have, s);
        Pn[tri(j, kk)] = (kk == j) ? s + q.w[j] : s;
      }
    }

    if constexpr (RECORD)
#pragma unroll
      for (int f = 0; f < NH; ++f) rec[(RtsRecord<NX>::PM + f) * B] = Pn[f];

    // ---- update: the measured states one at a time
    const R om = tick_w ? tick_w[(int64_t)t * B + p] : R(1);
    bool acted = false;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const R rho = om * sw.w[i];
      if (rho > R(0)) {
        const R rv = R(1) / rho;
        const R s = Pn[tri(i, i)] + rv;
        R res[NX];
#pragma unroll
        for (int m = 0; m < NX; ++m) res[m] = R(0);
        res[i] = y[((int64_t)t * NX + i) * B + p] - xs[i];
        wrap_residual<R, M>(res);
        const R nu = res[i];
        R gain[NX];
#pragma unroll
        for (int j = 0; j < NX; ++j) gain[j] = Pn[tri_sym(j, i)] / s;
#pragma unroll
        for (int j = 0; j < NX; ++j) xs[j] += gain[j] * nu;
        nis_sum += nu * nu / s;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          if (j == i) continue;
#pragma unroll
          for (int kk = 0; kk <= j; ++kk) {
            if (kk == i) continue;
            Pn[tri(j, kk)] -= gain[j] * Pn[tri_sym(kk, i)];
          }
        }
#pragma unroll
        for (int j = 0; j < NX; ++j) Pn[tri_sym(j, i)] = gain[j] * rv;
        acted = true;
      }
    }
    if (acted) wrap_angles<R, M>(xs);  // not where nothing acted: the wrap of a wrapped angle is not always that angle

#pragma unroll
    for (int f = 0; f < NH; ++f) acc[f][lane] = Pn[f];
    if constexpr (RECORD) {
#pragma unroll
      for (int r = 0; r < NX; ++r) rec[(RtsRecord<NX>::XF + r) * B] = xs[r];
#pragma unroll
      for (int f = 0; f < NH; ++f) rec[(RtsRecord<NX>::PF + f) * B] = Pn[f];
    }
    if (xs_out)
#pragma unroll
      for (int r = 0; r < NX; ++r) xs_out[((int64_t)t * NX + r) * B + p] = xs[r];
  }

  if (x_final)
#pragma unroll
    for (int r = 0; r < NX; ++r) x_final[r * B + p] = xs[r];
  if (P_final) {
    constexpr int NS = NX;
    R* const out = P_final;
#include "sim_store_sym.inc"
  }
  if (nis) nis[p] = nis_sum;
