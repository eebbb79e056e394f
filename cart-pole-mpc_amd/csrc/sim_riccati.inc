// sim_riccati.inc -- the arithmetic of the Riccati step of sim_lqr_kernel (sim_track_kernels.hpp) and of
// sim_ilqr_backward_kernel (sim_ilqr_kernels.hpp), which carries a half-gradient and a box limit beside it: one text, in the
// three parts the iLQR's own statements go between, so the P and K arithmetic of the two kernels is one and stays one -- K and
// P0 of an iLQR step without regularisation and limit are sim_lqr's bit for bit because they are the same statements.  A part is
// chosen by defining its macro in front of the #include, which undefines it.  As functions the same statements are fused into
// other multiply-adds and the results change in the last place: hence a text.  P's initialisation, the identity plant's tick
// and the load of P stay written in each kernel: as parts of this text they put the iLQR's own statements in another order,
// and its double 4-state form then ran 1 - 4 % longer (both measured, DESIGN.md 5n).  With these three parts every
// instantiation of both kernels is the instructions it was when each kernel had its own copy.
// Expects in scope everywhere: R, NX, NH = tri(NX, 0), lane, and acc, the lane's LDS column acc[field][lane] with P's lower
// triangle, (j, k <= j) at tri(j, k), in its first NH fields.
#if defined(CPMPC_RICCATI_V_S0)
// Expects gam, rw and Pm [NH], P as loaded from the lane's column.  Declares v = P gamma and s0 = r + gamma . v.
    R v[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      R a = Pm[tri_sym(j, 0)] * gam[0];
#pragma unroll
      for (int l = 1; l < NX; ++l) a += Pm[tri_sym(j, l)] * gam[l];
      v[j] = a;
    }
    R s0 = rw;
#pragma unroll
    for (int l = 0; l < NX; ++l) s0 += gam[l] * v[l];
#undef CPMPC_RICCATI_V_S0
#elif defined(CPMPC_RICCATI_GAIN_ACL)
// Expects M, NQ, TRIV, B, p, Phi, t_sum, gam, v, s, t, K_out, and CPMPC_RICCATI_GAIN(k): what becomes of the gain k = -(Phi^T v) / s
// (the iLQR drops it for a control held on its limit).  Declares kt, stored to K[t], and Acl = Phi + gamma kt^T, dense.
    R kt[NX];
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      bool have = false;
      R w = R(0);
#pragma unroll
      for (int l = 0; l < NX; ++l) ekf_add_term<R, NX, NQ, TRIV>(Phi, t_sum, l, c, v[l], have, w);
      kt[c] = CPMPC_RICCATI_GAIN(-(w / s));
    }
    if (K_out)
#pragma unroll
      for (int c = 0; c < NX; ++c) K_out[((int64_t)t * NX + c) * B + p] = kt[c];
    R Acl[NX][NX];
#pragma unroll
    for (int l = 0; l < NX; ++l)
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        const R g = gam[l] * kt[c];
        Acl[l][c] = struct_zero<NX, NQ>(TRIV, l, c) ? g : phi_entry<R, M>(Phi, t_sum, l, c) + g;
      }
#undef CPMPC_RICCATI_GAIN_ACL
#elif defined(CPMPC_RICCATI_UPDATE)
// P = diag(q) + r kt kt^T + Acl^T P Acl into the lane's column, a row of Acl^T P at a time.  Expects Pm, kt, Acl, q, rw.
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
#undef CPMPC_RICCATI_UPDATE
#else
#error "sim_riccati.inc: define the part to include"
#endif
