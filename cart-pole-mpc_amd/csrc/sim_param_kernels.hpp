// sim_param_kernels.hpp -- the plant step's derivative in the DYNAMICS PARAMETERS: Simulator::Step (simulator.cc:11-36) as
// sim_kernel runs it -- 1 ms RK4 sub-steps with the control held, the last one h_last, the pole angles wrapped after each --
// together with
//     P = dx+/dp  (NX x NP)
// of the whole step.  Only FIRST derivatives of the accelerations are needed: Jpa = da/dp (NQ x NP) beside the Ja = da/dx the
// kernels already form.  (The controller's derivative in p needs dPhi/dp and dGamma/dp, second derivatives of the RK4 chain:
// that stays ruled out)
//
// Column j of P is a tangent t carried through the stages of every sub-step (a JVP; no step Jacobian A_i is formed):
//     dk_1 = K_1 t + Jp_1[:, j],   dk_{m+1} = K_{m+1} (t + a_m dk_m) + Jp_{m+1}[:, j],   a = {h/2, h/2, h}
//     t+   = t + h/6 (dk_1 + 2 dk_2 + 2 dk_3 + dk_4),          K = [[0 I],[Ja]],  Jp = [0; Jpa]
// from t = 0 before the first sub-step; the products skip the columns of Ja that vanish identically (JaZeroCols), and the
// wrap has unit derivative.  Per column 3 NX numbers live across a stage (t, the running sum, the last dk) and a stage costs
// NQ NX multiply-adds.  One problem per lane, no LDS; the state is read only.
//
// The parameter columns are processed in compile-time groups [J0, J0 + NG), one launch per group, each recomputing the primal
// step (engine_impl.hpp: sim_param_jac_impl; the group widths are the largest without scratch).  With a
// cotangent gbar [NX][B] a group contracts its rows of gp = P^T gbar [NP][B] in registers and P never goes to memory.
// The tangents of a tick are sim_param_tick.inc and the raw parameters' load is sim_param_load.inc: texts that pass B of
// sim_rollout_vjp_kernel includes too.
#pragma once
#include "double_pendulum_param_gen.hpp"
#include "sim_jac_kernels.hpp"

namespace cpmpc {

// the raw dynamics parameters of a problem, in the kernel's scalar type, beside the folded Consts
template <typename R, int NP>
struct RawParams {
  R p[NP];
};

// ------------------------------------------------------------------------------------------------
// cart + single pole: cartpole_accel_sc's accelerations and Ja, and Jpa[2][9] = da/d{m_b, m_1, l_1, g, mu_b, v_mu_b, c_d_1,
// x_s, k_s}, the equations differentiated as they are evaluated there:
//     a = N / den,   da/dp = (dN/dp - a dden/dp) / den,   N_x = F_b + (s/L) F_th,   N_th = (s/L) F_b + kap F_th
// v_mu_b enters through max(v_mu_b, 1e-6): its column is 0 where the clamp is active.  The bumper columns use F_s's own
// strict comparisons: exactly zero off the bumpers.  External forces included.
// ------------------------------------------------------------------------------------------------
template <typename R, bool HAS_EXT>
__device__ __forceinline__ void cartpole_accel_param_sc(const CartPoleConsts<R>& k, const R (&prm)[9], const R bx, const R s,
                                                        const R c, const R v, const R w, const R u, const ExtForce<R>& fe,
                                                        R& a_x, R& a_th, R (&Ja)[2][4], R (&Jpa)[2][9]) {
  // ---- the primal and Ja: cartpole_accel_sc<R, true, HAS_EXT>, statement for statement --------------------------------
  const R e_r = bx - k.xs;
  const R e_l = -(bx + k.xs);
  const bool on_r = R(0) < e_r;
  const bool on_l = R(0) < e_l;
  const R spring = (on_l ? e_l : R(0)) - (on_r ? e_r : R(0));
  const R F_s = k.ks * spring;

  const R den = k.mt - k.m_1 * s * s;
  R tv, inv_den, sech2 = R(0);
  if constexpr (Math<R>::kMergedReciprocals) {
    R num, dt, e2;
    Math<R>::tanh_parts(v * k.inv_v_mu, num, dt, e2);
    const R r = Math<R>::rcp(den * dt);
    inv_den = r * dt;
    const R idt = r * den;
    const R q = num * idt;
    sech2 = R(4) * e2 * (idt * idt);
    tv = __builtin_copysign(q, v);
  } else {
    tv = Math<R>::tanh_scaled(v, k.inv_v_mu, k.tanh_k2);
    inv_den = Math<R>::rcp(den);
    sech2 = R(1) - tv * tv;
  }
  const R F_f = tv * k.fr;

  const R Lw = k.L * w;
  const R vx = v - Lw * s;
  const R vy = Lw * c;
  const R n2 = vx * vx + vy * vy;
  R n, inv_n;
  Math<R>::sqrt_inv(n2, n, inv_n);
  const R e = Lw - s * v;
  const R Dx = k.half_cd * n * vx;
  const R Dth = k.half_cd_L * n * e;

  R F_b = u + F_f + F_s - Dx + k.m1L * w * w * c;
  R F_th = -k.gm1L * c - Dth;
  R ext_th = R(0);  // (f_my c - f_mx s): the external torque per unit pole length
  if (HAS_EXT) {
    F_b += fe.fbx + fe.fmx;
    ext_th = fe.fmy * c - fe.fmx * s;
    F_th += k.L * ext_th;
  }

  const R sl = s * k.inv_L;
  const R N_x = F_b + sl * F_th;
  const R N_th = sl * F_b + k.kap * F_th;
  a_x = N_x * inv_den;
  a_th = N_th * inv_den;

  {
    const R dn0 = -(vy * v) * inv_n;
    const R dn1 = vx * inv_n;
    const R dn2 = (k.L * e) * inv_n;
    const R dDx0 = k.half_cd * (dn0 * vx - n * vy);
    const R dDx1 = k.half_cd * (dn1 * vx + n);
    const R dDx2 = k.half_cd * (dn2 * vx - n * (k.L * s));
    const R dDt0 = k.half_cd_L * (dn0 * e - n * (c * v));
    const R dDt1 = k.half_cd_L * (dn1 * e - n * s);
    const R dDt2 = k.half_cd_L * (dn2 * e + n * k.L);
    const R dFf_dv = sech2 * k.fr_vmu;
    const R dFs_dbx = k.ks * ((on_l ? R(-1) : R(0)) - (on_r ? R(1) : R(0)));

    const R dFb0 = -dDx0 - k.m1L * w * w * s;
    const R dFb1 = dFf_dv - dDx1;
    const R dFb2 = -dDx2 + k.two_m1L * w * c;
    R dFt0 = k.gm1L * s - dDt0;
    if (HAS_EXT) dFt0 += k.L * (-fe.fmx * c - fe.fmy * s);
    const R dFt1 = -dDt1;
    const R dFt2 = -dDt2;

    const R dden = R(-2) * k.m_1 * s * c;
    const R cl = c * k.inv_L;
    const R dNx0 = dFb0 + cl * F_th + sl * dFt0;
    const R dNx1 = dFb1 + sl * dFt1;
    const R dNx2 = dFb2 + sl * dFt2;
    const R dNt0 = cl * F_b + sl * dFb0 + k.kap * dFt0;
    const R dNt1 = sl * dFb1 + k.kap * dFt1;
    const R dNt2 = sl * dFb2 + k.kap * dFt2;

    Ja[0][0] = dFs_dbx * inv_den;
    Ja[0][1] = (dNx0 - a_x * dden) * inv_den;
    Ja[0][2] = dNx1 * inv_den;
    Ja[0][3] = dNx2 * inv_den;
    Ja[1][0] = sl * dFs_dbx * inv_den;
    Ja[1][1] = (dNt0 - a_th * dden) * inv_den;
    Ja[1][2] = dNt1 * inv_den;
    Ja[1][3] = dNt2 * inv_den;
  }

  // ---- Jpa: each parameter's dF_b, dF_th, d(s/L), dkap, dden; terms that vanish identically are not formed ----------------
  const R m_1 = prm[1], L = prm[2], g = prm[3], mu = prm[4], v_mu_in = prm[5];
  const R mt = prm[0] + m_1;
  const R ww_c = w * w * c;
  const R inv_m1L2 = k.inv_L * k.inv_L * Math<R>::rcp(m_1);  // 1 / (m_1 L^2) = dkap / dm_b
  // m_b: m_t' = 1, den' = 1, fr' = -mu g, kap' = 1 / (m_1 L^2)
  {
    const R dFb = tv * (-(mu * g));
    const R dNx = dFb;
    const R dNt = sl * dFb + inv_m1L2 * F_th;
    Jpa[0][0] = (dNx - a_x) * inv_den;
    Jpa[1][0] = (dNt - a_th) * inv_den;
  }
  // m_1: m_t' = 1, den' = 1 - s^2, fr' = -mu g, kap' = -m_b / (m_1^2 L^2)
  {
    const R dFb = tv * (-(mu * g)) + L * ww_c;
    const R dFt = -(g * L) * c;
    const R dkap = -(prm[0] * Math<R>::rcp(m_1)) * inv_m1L2;
    const R dden = R(1) - s * s;
    const R dNx = dFb + sl * dFt;
    const R dNt = sl * dFb + dkap * F_th + k.kap * dFt;
    Jpa[0][1] = (dNx - a_x * dden) * inv_den;
    Jpa[1][1] = (dNt - a_th * dden) * inv_den;
  }
  // l_1: v_x' = -w s, v_y' = w c, e' = w, (s/L)' = -s / L^2, kap' = -2 kap / L
  {
    const R dvx = -(w * s), dvy = w * c;
    const R dn = (vx * dvx + vy * dvy) * inv_n;
    const R hcd = k.half_cd;
    const R dDx = hcd * (dn * vx + n * dvx);
    const R dDt = hcd * (n * e + L * (dn * e + n * w));
    const R dFb = -dDx + m_1 * ww_c;
    R dFt = -(g * m_1) * c - dDt;
    if (HAS_EXT) dFt += ext_th;
    const R dsl = -(sl * k.inv_L);
    const R dkap = R(-2) * k.kap * k.inv_L;
    const R dNx = dFb + dsl * F_th + sl * dFt;
    const R dNt = dsl * F_b + sl * dFb + dkap * F_th + k.kap * dFt;
    Jpa[0][2] = dNx * inv_den;
    Jpa[1][2] = dNt * inv_den;
  }
  // g: fr' = -m_t mu, F_th' = -m_1 L c
  {
    const R dFb = tv * (-(mt * mu));
    const R dFt = -k.m1L * c;
    Jpa[0][3] = (dFb + sl * dFt) * inv_den;
    Jpa[1][3] = (sl * dFb + k.kap * dFt) * inv_den;
  }
  // mu_b: fr' = -m_t g
  {
    const R dFb = tv * (-(mt * g));
    Jpa[0][4] = dFb * inv_den;
    Jpa[1][4] = sl * dFb * inv_den;
  }
  // v_mu_b, through max(v_mu_b, 1e-6): tanh(v / v_mu)' = -sech^2 v / v_mu^2; 0 where the clamp is active
  {
    const bool free_ = R(1.0e-6) < v_mu_in;
    const R dtv = -(sech2 * v) * (k.inv_v_mu * k.inv_v_mu);
    const R dFb = free_ ? k.fr * dtv : R(0);
    Jpa[0][5] = dFb * inv_den;
    Jpa[1][5] = sl * dFb * inv_den;
  }
  // c_d_1: D_x' = n v_x / 2, D_th' = L n e / 2
  {
    const R dFb = -(R(0.5) * n * vx);
    const R dFt = -(R(0.5) * L * n * e);
    Jpa[0][6] = (dFb + sl * dFt) * inv_den;
    Jpa[1][6] = (sl * dFb + k.kap * dFt) * inv_den;
  }
  // x_s: e_r' = -1, e_l' = -1 where the spring is on
  {
    const R dFb = k.ks * ((on_r ? R(1) : R(0)) - (on_l ? R(1) : R(0)));
    Jpa[0][7] = dFb * inv_den;
    Jpa[1][7] = sl * dFb * inv_den;
  }
  // k_s
  {
    Jpa[0][8] = spring * inv_den;
    Jpa[1][8] = sl * spring * inv_den;
  }
}

// ------------------------------------------------------------------------------------------------
// The models' accelerations at stage STAGE of an RK4 step with Ja and Jpa (no Jua: the control is held, not differentiated)
// ------------------------------------------------------------------------------------------------
template <typename R, typename M>
struct ParamAccel;

template <typename R>
struct ParamAccel<R, SingleModelHandWritten<R>> {
  using M = SingleModelHandWritten<R>;
  template <bool HAS_EXT, int STAGE>
  __device__ __forceinline__ static void accel_stage(const typename M::Consts& k, const R (&prm)[9], const R (&x)[4], const R u,
                                                     const ExtForce<R>& fe, R (&a)[2], R (&Ja)[2][4], R (&Jpa)[2][9],
                                                     typename M::StepCache& sc) {
    R s, c;
    stage_sincos<R, STAGE>(sc, x[1], s, c);
    cartpole_accel_param_sc<R, HAS_EXT>(k, prm, x[0], s, c, x[2], x[3], u, fe, a[0], a[1], Ja, Jpa);
  }
};

// the same model on the generated code (-DCPMPC_GENERATED_SINGLE=1): the generator emits no parameter partials for it, so the
// parameter kernel of that build runs the hand-written equations, their constants folded from the raw parameters per stage
template <typename R>
struct ParamAccel<R, SingleModelGenerated<R>> {
  using M = SingleModelGenerated<R>;
  template <bool HAS_EXT, int STAGE>
  __device__ __forceinline__ static void accel_stage(const typename M::Consts&, const R (&prm)[9], const R (&x)[4], const R u,
                                                     const ExtForce<R>& fe, R (&a)[2], R (&Ja)[2][4], R (&Jpa)[2][9],
                                                     typename M::StepCache& sc) {
    R s, c;
    stage_sincos<R, STAGE>(sc, x[1], s, c);
    const CartPoleConsts<R> k = make_consts<R, R>(prm);
    cartpole_accel_param_sc<R, HAS_EXT>(k, prm, x[0], s, c, x[2], x[3], u, fe, a[0], a[1], Ja, Jpa);
  }
};

// cart + double pole: a = M^-1 F and Ja as DoubleModel::accel_sc, then da/dp_j = M^-1 (dF/dp_j - dM/dp_j a) with the same
// LDL^T and the generated dF/dp, dM/dp (double_pendulum_param_gen.hpp), identically-zero entries left out
template <typename R>
struct ParamAccel<R, DoubleModel<R>> {
  using M = DoubleModel<R>;
  using Sp = DoublePendulumGenSparsity;
  using Pp = DoublePendulumParamSparsity;
  template <bool HAS_EXT, int STAGE>
  __device__ __forceinline__ static void accel_stage(const typename M::Consts& k, const R (&prm)[6], const R (&x)[6], const R u,
                                                     const ExtForce<R>&, R (&a)[3], R (&Ja)[3][6], R (&Jpa)[3][6],
                                                     typename M::StepCache& sc) {
    R s1, c1, s2, c2;
    stage_sincos<R, STAGE>(sc.t1, x[1], s1, c1);
    stage_sincos<R, STAGE>(sc.t2, x[2], s2, c2);
    R Mm[9], F[3], dFdx[18], dM1[9], dM2[9], L[3], id[3];
    double_pendulum_terms_sc<R>(k.g, s1, c1, s2, c2, x, u, Mm, F, dFdx, dM1, dM2);
    M::factor(Mm, k.inv_m00, L, id);
    M::solve(L, id, F[0], F[1], F[2], a);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      if ((Sp::ja_zero_cols >> c) & 1u) {
        Ja[0][c] = R(0);
        Ja[1][c] = R(0);
        Ja[2][c] = R(0);
        continue;
      }
      R r[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        bool have = Sp::dFdx[i * 6 + c];
        R v = have ? dFdx[i * 6 + c] : R(0);
        if (c == 1 || c == 2) {
          const R* dM = (c == 1) ? dM1 : dM2;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const bool nz = (c == 1) ? Sp::dM1[i * 3 + j] : Sp::dM2[i * 3 + j];
            if (nz) {
              v = have ? v - dM[i * 3 + j] * a[j] : -(dM[i * 3 + j] * a[j]);
              have = true;
            }
          }
        }
        r[i] = v;
      }
      R y[3];
      M::solve(L, id, r[0], r[1], r[2], y);
      Ja[0][c] = y[0];
      Ja[1][c] = y[1];
      Ja[2][c] = y[2];
    }
    R dFdp[18], dMdp[54];
    double_pendulum_param_terms_sc<R>(prm, s1, c1, s2, c2, x, u, dFdp, dMdp);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      R r[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        bool have = Pp::dFdp[i * 6 + j];
        R v = have ? dFdp[i * 6 + j] : R(0);
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
          if (Pp::dMdp[j * 9 + i * 3 + kk]) {
            v = have ? v - dMdp[j * 9 + i * 3 + kk] * a[kk] : -(dMdp[j * 9 + i * 3 + kk] * a[kk]);
            have = true;
          }
        r[i] = v;
      }
      R y[3];
      M::solve(L, id, r[0], r[1], r[2], y);
      Jpa[0][j] = y[0];
      Jpa[1][j] = y[1];
      Jpa[2][j] = y[2];
    }
  }
};

// dk = K arg + Jp[:, j] for the tangent columns of a group: the top NQ rows of K arg are arg's velocities, the bottom NQ
// are Ja arg, the columns of Ja that vanish identically (ZMASK) neither multiplied nor added
template <typename R, int NX, int NQ, int NP, unsigned ZMASK, int J0, int NG>
__device__ __forceinline__ void param_stage_tangent(const R (&Ja)[NQ][NX], const R (&Jpa)[NQ][NP], const R (&arg)[NG][NX],
                                                    R (&dk)[NG][NX]) {
  constexpr int k0 = first_nonzero_col<NX>(ZMASK);
#pragma unroll
  for (int gI = 0; gI < NG; ++gI) {
    R out[NX];
#pragma unroll
    for (int r = 0; r < NQ; ++r) {
      out[r] = arg[gI][NQ + r];
      R acc = Ja[r][k0] * arg[gI][k0];
#pragma unroll
      for (int kk = k0 + 1; kk < NX; ++kk)
        if (!((ZMASK >> kk) & 1u)) acc += Ja[r][kk] * arg[gI][kk];
      out[NQ + r] = acc + Jpa[r][J0 + gI];
    }
#pragma unroll
    for (int r = 0; r < NX; ++r) dk[gI][r] = out[r];
  }
}

// One RK4 step of the state x (in place, as rk4_step_m) carrying the tangents T[g] = dx/dp_{J0 + g} through it
template <typename R, typename M, bool HAS_EXT, int J0, int NG>
__device__ __forceinline__ void rk4_step_param_m(const typename M::Consts& k, const R (&prm)[M::NP], const R h, R (&x)[M::NX],
                                                 const R u, const ExtForce<R>& fe, R (&T)[NG][M::NX],
                                                 typename M::StepCache& sc) {
  constexpr int NX = M::NX, NQ = M::NQ, NP = M::NP;
  constexpr unsigned ZM = JaZeroCols<M>::value;
  using PA = ParamAccel<R, M>;
  const R hh = h / R(2);
  R Ja[NQ][NX], Jpa[NQ][NP];
  R a1[NQ], a2[NQ], a3[NQ], a4[NQ], v2[NQ], v3[NQ], v4[NQ], xt[NX];
  R dk[NG][NX], S[NG][NX], arg[NG][NX];

  // stage 1
  PA::template accel_stage<HAS_EXT, 1>(k, prm, x, u, fe, a1, Ja, Jpa, sc);
  param_stage_tangent<R, NX, NQ, NP, ZM, J0, NG>(Ja, Jpa, T, dk);
#pragma unroll
  for (int gI = 0; gI < NG; ++gI)
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      S[gI][r] = dk[gI][r];
      arg[gI][r] = T[gI][r] + hh * dk[gI][r];
    }
  // stage 2
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    v2[i] = x[NQ + i] + a1[i] * hh;
    xt[i] = x[i] + x[NQ + i] * hh;
    xt[NQ + i] = v2[i];
  }
  PA::template accel_stage<HAS_EXT, 2>(k, prm, xt, u, fe, a2, Ja, Jpa, sc);
  param_stage_tangent<R, NX, NQ, NP, ZM, J0, NG>(Ja, Jpa, arg, dk);
#pragma unroll
  for (int gI = 0; gI < NG; ++gI)
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      S[gI][r] += dk[gI][r] * R(2);
      arg[gI][r] = T[gI][r] + hh * dk[gI][r];
    }
  // stage 3
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    v3[i] = x[NQ + i] + a2[i] * hh;
    xt[i] = x[i] + v2[i] * hh;
    xt[NQ + i] = v3[i];
  }
  PA::template accel_stage<HAS_EXT, 3>(k, prm, xt, u, fe, a3, Ja, Jpa, sc);
  param_stage_tangent<R, NX, NQ, NP, ZM, J0, NG>(Ja, Jpa, arg, dk);
#pragma unroll
  for (int gI = 0; gI < NG; ++gI)
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      S[gI][r] += dk[gI][r] * R(2);
      arg[gI][r] = T[gI][r] + h * dk[gI][r];
    }
  // stage 4
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    v4[i] = x[NQ + i] + a3[i] * h;
    xt[i] = x[i] + v3[i] * h;
    xt[NQ + i] = v4[i];
  }
  PA::template accel_stage<HAS_EXT, 4>(k, prm, xt, u, fe, a4, Ja, Jpa, sc);
  param_stage_tangent<R, NX, NQ, NP, ZM, J0, NG>(Ja, Jpa, arg, dk);
  const R h6 = h / R(6);
#pragma unroll
  for (int gI = 0; gI < NG; ++gI)
#pragma unroll
    for (int r = 0; r < NX; ++r) T[gI][r] += h6 * (S[gI][r] + dk[gI][r]);
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const R v1 = x[NQ + i];
    x[i] += h6 * (v1 + v2[i] * R(2) + v3[i] * R(2) + v4[i]);
    x[NQ + i] += h6 * (a1[i] + a2[i] * R(2) + a3[i] * R(2) + a4[i]);
  }
}

// Outputs, each written only where its pointer is given (a wave-uniform choice): x_new [NX][B]; the group's columns of
// P [NX*NP][B] (element (r, j) at field r*NP + j); for a cotangent gbar [NX][B] the group's rows of gp = P^T gbar [NP][B].
// PER_LANE: the parameters are dyn [NP][B], read per lane, and the constants are M::make<R> of them in the kernel, as
// load_consts does (mpc_kernels.hpp); else `k` and `raw` are the shared set's.
template <typename R, typename M, int J0, int NG, bool PER_LANE>
__global__ __launch_bounds__(64) void sim_param_jac_kernel(int64_t B, typename M::Consts k_shared, RawParams<R, M::NP> raw,
                                                            const R* dyn, ExtForce<R> fe_shared, const R* fext, int n_sub,
                                                            R h_last, const R* state, const R* u, R* x_new, R* P,
                                                            const R* gbar, R* gp) {
  constexpr int NX = M::NX, NP = M::NP;
  static_assert(J0 >= 0 && NG >= 1 && J0 + NG <= NP, "a group of parameter columns");
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  ExtForce<R> fe = fe_shared;
  load_ext_force<R>(fext, B, p, fe);
  R prm[NP];
  typename M::Consts k = k_shared;
#include "sim_param_load.inc"
  if constexpr (PER_LANE) k = M::template make<R>(prm);
  R xs[NX];
#pragma unroll
  for (int t = 0; t < NX; ++t) xs[t] = state[t * B + p];
  const R uu = u[p];

#include "sim_param_tick.inc"  // Tn of the tick; xs becomes x+

  if (x_new)
#pragma unroll
    for (int t = 0; t < NX; ++t) x_new[t * B + p] = xs[t];
  if (P)
#pragma unroll
    for (int gI = 0; gI < NG; ++gI)
#pragma unroll
      for (int r = 0; r < NX; ++r) P[(r * NP + J0 + gI) * B + p] = Tn[gI][r];
  if (gp) {
    if (n_sub == 0) {  // the identity map has no parameters: zeros, not products of zeros with the cotangent
#pragma unroll
      for (int gI = 0; gI < NG; ++gI) gp[(J0 + gI) * B + p] = R(0);
      return;
    }
    R g[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) g[r] = gbar[r * B + p];
#pragma unroll
    for (int gI = 0; gI < NG; ++gI) {
      R acc = Tn[gI][0] * g[0];
#pragma unroll
      for (int r = 1; r < NX; ++r) acc += Tn[gI][r] * g[r];
      gp[(J0 + gI) * B + p] = acc;
    }
  }
}

}  // namespace cpmpc
