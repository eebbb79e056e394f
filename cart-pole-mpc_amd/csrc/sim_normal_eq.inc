// sim_normal_eq.inc -- a tick's share of the normal equations of a window fit, for NC sensitivity columns col[j][q] = d x_q /
// d unknown_j, into the lane's LDS fields acc[.][lane]:
//     acc[NH + j]     -= sum_q om w_q col[j][q] res[q]           g
//     acc[tri(j, k)]  += sum_q om w_q col[j][q] col[k][q]        H, k <= j
// Zero::zero(q, j) (sim_window.hpp) says at compile time that entry q of column j is an exact zero: it is neither read nor
// multiplied.  Each sum runs over the q that are zero in neither column, the first product and then the adds in index order.
// Included by sim_rollout_gn_kernel (NeverZero) and sim_rollout_gn_x0_kernel (PhiZero); as a function: scratch (DESIGN.md 5l).
// Expects in scope: R, NX, NC, NH = tri(NC, 0), col, Zero, res, om, sw, acc and lane.
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        R ws[NX];  // om W col[j]
#pragma unroll
        for (int q = 0; q < NX; ++q)
          if (!Zero::zero(q, j)) ws[q] = om * (sw.w[q] * col[j][q]);
        {
          bool have = false;
          R gj = R(0);
#pragma unroll
          for (int q = 0; q < NX; ++q) {
            if (Zero::zero(q, j)) continue;
            gj = have ? gj + ws[q] * res[q] : ws[q] * res[q];
            have = true;
          }
          acc[NH + j][lane] -= gj;
        }
#pragma unroll
        for (int kk = 0; kk <= j; ++kk) {
          bool have = false;
          R h = R(0);
#pragma unroll
          for (int q = 0; q < NX; ++q) {
            if (Zero::zero(q, j) || Zero::zero(q, kk)) continue;
            h = have ? h + ws[q] * col[kk][q] : ws[q] * col[kk][q];
            have = true;
          }
          if (have) acc[tri(j, kk)][lane] += h;  // no common row: an exact zero stays the zero it was set to
        }
      }
