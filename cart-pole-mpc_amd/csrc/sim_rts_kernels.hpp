// sim_rts_kernels.hpp -- the backward pass of the Rauch-Tung-Striebel smoother of B plants over T ticks in one kernel, behind
// the recording form of the Kalman filter (sim_ekf_kernels.hpp: sim_ekf_record_kernel).  State index 0 is x0 / P0, index t is
// after tick t; with x-, P- the prediction of tick t (index t + 1 before its update) and A_t P_t the rows the filter formed,
//     x^s_T = x_T,  P^s_T = P_T,  and for t = T-1 .. 0
//         G_t   = (A_t P_t)^T (P-_{t+1})^-1                       P- symmetric
//         d     = wrap_residual(x^s_{t+1} - x-_{t+1})
//         x^s_t = x_t + G_t d                                     then wrap_angles, only where G_t d has a non-zero entry
//         P^s_t = P_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T          lower triangle computed, stored exactly symmetric
// There is no plant in it: everything it reads is the record (sim_window.hpp: RtsRecord), x0 and P0's lower triangle.
//
// One problem per lane, no barrier; x^s and P^s are carried in registers over the ticks.  Per tick: the Cholesky factor of the
// diagonally scaled P- (unit diagonal) in registers, the NX rows of G by forward and back substitution (no inverse is
// formed) into lane-private LDS, acc[field][threadIdx.x], then the two updates.  A tick whose P- is not positive definite --
// a diagonal entry not positive, or a pivot of the scaled matrix not above 8 NX eps (sim_estimate_state's floor) or not
// finite -- takes G_t = 0: that index's smoothed values are its filtered ones, the recursion goes on from them, and the
// lane's ok is 0.  That is the answer for P0 = 0, "the start is known".  Everything is computed whichever outputs are stored
// (wave-uniform pointer tests), so each is bitwise the same whatever else is asked for.  Where nothing was measured
// P^s_{t+1} - P-_{t+1} and d are exact zeros, and the smoothed values are the filtered ones bit for bit.
#pragma once
#include <limits>

#include "sim_window.hpp"

namespace cpmpc {

// Outputs, each written only where its pointer is given: xs_smooth [T+1][NX][B]; Ps_smooth [T+1][NX*NX][B], full, (j, k) and
// (k, j) from the one kept value; x0_smooth [NX][B] and P0_smooth [NX*NX][B], index 0 alone; ok [B].  work: the T records of
// sim_ekf_record_kernel.  x0 [NX][B]; P0 [NX*NX][B], its lower triangle (fields j*NX + k, k <= j) is read.
// (Asking for two waves per SIMD, __launch_bounds__(64, 2), puts the float 6-state form into 212 bytes of scratch: it stays at the
// 306 the float units' scheduler spends and one wave per SIMD, as the double 6-state form.)
template <typename R, typename M>
__global__ __launch_bounds__(64) void sim_rts_kernel(int64_t B, int T, const R* x0, const R* P0, const R* work, R* xs_smooth,
                                                      R* Ps_smooth, R* x0_smooth, R* P0_smooth, int32_t* ok_out) {
  constexpr int NX = M::NX;
  constexpr int NH = tri(NX, 0);
  using Rec = RtsRecord<NX>;
  __shared__ R acc[NX * NX][64];  // G, (i, j) at field i*NX + j
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const R floor_pivot = R(8 * NX) * std::numeric_limits<R>::epsilon();

  // ---- index T: the filtered state and covariance the last tick left
  R xsm[NX], Ps[NH];
  {
    const R* const last = work + (int64_t)(T - 1) * Rec::ROWS * B + p;
#pragma unroll
    for (int r = 0; r < NX; ++r) xsm[r] = last[(Rec::XF + r) * B];
#pragma unroll
    for (int f = 0; f < NH; ++f) Ps[f] = last[(Rec::PF + f) * B];
  }
  bool ok = true;

#pragma unroll 1
  for (int t = T;; --t) {
    // ---- store index t
    if (xs_smooth)
#pragma unroll
      for (int r = 0; r < NX; ++r) xs_smooth[((int64_t)t * NX + r) * B + p] = xsm[r];
    if (Ps_smooth) {
      R* const out = Ps_smooth + (int64_t)t * (NX * NX) * B + p;
#pragma unroll
      for (int j = 0; j < NX; ++j)
#pragma unroll
        for (int kk = 0; kk <= j; ++kk) {
          out[(j * NX + kk) * B] = Ps[tri(j, kk)];
          if (kk != j) out[(kk * NX + j) * B] = Ps[tri(j, kk)];
        }
    }
    // a state that is not finite is not an estimate: the lane's ok says so whatever its covariances were
#pragma unroll
    for (int r = 0; r < NX; ++r) ok = ok && (Math<R>::fabs(xsm[r]) <= std::numeric_limits<R>::max());
    if (t == 0) break;

    // ---- index t - 1 from index t: the record of tick t - 1
    const R* const rec = work + (int64_t)(t - 1) * Rec::ROWS * B + p;
    R Pm[NH], sc[NX];
#pragma unroll
    for (int f = 0; f < NH; ++f) Pm[f] = rec[(Rec::PM + f) * B];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const R d = Pm[tri(j, j)];
      const bool pos = d > R(0);
      bad = bad || !pos;
      R root;
      if constexpr (sizeof(R) == 4) root = __builtin_sqrtf(pos ? d : R(1));
      else root = __builtin_sqrt(pos ? d : R(1));
      sc[j] = R(1) / root;
    }
    // the Cholesky factor of the scaled matrix; the diagonal holds the pivots' inverse roots
    R L[NH];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R d = Pm[tri(j, j)] * sc[j] * sc[j];
#pragma unroll
      for (int q = 0; q < j; ++q) d -= L[tri(j, q)] * L[tri(j, q)];
      bad = bad || !(d > floor_pivot) || !(d <= std::numeric_limits<R>::max());
      R root;
      if constexpr (sizeof(R) == 4) root = __builtin_sqrtf(d > R(0) ? d : R(1));
      else root = __builtin_sqrt(d > R(0) ? d : R(1));
      const R ip = R(1) / root;
      L[tri(j, j)] = ip;
#pragma unroll
      for (int i = j + 1; i < NX; ++i) {
        R v = Pm[tri(i, j)] * sc[i] * sc[j];
#pragma unroll
        for (int q = 0; q < j; ++q) v -= L[tri(i, q)] * L[tri(j, q)];
        L[tri(i, j)] = v * ip;
      }
    }

    // d = wrap(x^s_t - x-_t), and G d beside the rows of G
    R dx[NX], delta[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) dx[r] = xsm[r] - rec[(Rec::XM + r) * B];
    wrap_residual<R, M>(dx);
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      // row i of G solves P- g = column i of A P
      R z[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        R v = rec[(Rec::AP + j * NX + i) * B] * sc[j];
#pragma unroll
        for (int q = 0; q < j; ++q) v -= L[tri(j, q)] * z[q];
        z[j] = v * L[tri(j, j)];
      }
#pragma unroll
      for (int j = NX - 1; j >= 0; --j) {
        R v = z[j];
#pragma unroll
        for (int q = j + 1; q < NX; ++q) v -= L[tri(q, j)] * z[q];
        z[j] = v * L[tri(j, j)];
      }
      R s = R(0);
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        const R g = z[j] * sc[j];
        acc[i * NX + j][lane] = g;
        s = (j == 0) ? g * dx[j] : s + g * dx[j];
      }
      delta[i] = s;
    }

    // the filtered state and covariance of index t - 1
    R xf[NX], Pf[NH];
    if (t == 1) {
#pragma unroll
      for (int r = 0; r < NX; ++r) xf[r] = x0[r * B + p];
#pragma unroll
      for (int j = 0; j < NX; ++j)
#pragma unroll
        for (int kk = 0; kk <= j; ++kk) Pf[tri(j, kk)] = P0[(j * NX + kk) * B + p];
    } else {
      const R* const prev = rec - (int64_t)Rec::ROWS * B;
#pragma unroll
      for (int r = 0; r < NX; ++r) xf[r] = prev[(Rec::XF + r) * B];
#pragma unroll
      for (int f = 0; f < NH; ++f) Pf[f] = prev[(Rec::PF + f) * B];
    }

    // x^s = x + G d
    {
      bool moved = false;
      R xw[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        moved = moved || (delta[r] != R(0));
        xw[r] = xf[r] + delta[r];
      }
      wrap_angles<R, M>(xw);  // not where nothing moved: the wrap of a wrapped angle is not always that angle
#pragma unroll
      for (int r = 0; r < NX; ++r) xsm[r] = (bad || !moved) ? xf[r] : xw[r];
    }

    // P^s = P + G (P^s - P-) G^T, a row of G (P^s - P-) at a time
#pragma unroll
    for (int f = 0; f < NH; ++f) Pm[f] = Ps[f] - Pm[f];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R gj[NX], w[NX];
#pragma unroll
      for (int l = 0; l < NX; ++l) gj[l] = acc[j * NX + l][lane];
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        R s = gj[0] * Pm[tri_sym(0, c)];
#pragma unroll
        for (int l = 1; l < NX; ++l) s += gj[l] * Pm[tri_sym(l, c)];
        w[c] = s;
      }
#pragma unroll
      for (int kk = 0; kk <= j; ++kk) {
        R s = w[0] * ((kk == j) ? gj[0] : acc[kk * NX][lane]);
#pragma unroll
        for (int l = 1; l < NX; ++l) s += w[l] * ((kk == j) ? gj[l] : acc[kk * NX + l][lane]);
        const R keep = Pf[tri(j, kk)];
        Ps[tri(j, kk)] = bad ? keep : keep + s;
      }
    }
    ok = ok && !bad;

    if (t == 1) {
      if (x0_smooth)
#pragma unroll
        for (int r = 0; r < NX; ++r) x0_smooth[r * B + p] = xsm[r];
      if (P0_smooth)
#pragma unroll
        for (int j = 0; j < NX; ++j)
#pragma unroll
          for (int kk = 0; kk <= j; ++kk) {
            P0_smooth[(j * NX + kk) * B + p] = Ps[tri(j, kk)];
            if (kk != j) P0_smooth[(kk * NX + j) * B + p] = Ps[tri(j, kk)];
          }
    }
  }
  if (ok_out) ok_out[p] = ok ? 1 : 0;
}

}  // namespace cpmpc
