// linearize_interval.inc -- the body of linearize_kernel and linearize_dyn_kernel (mpc_kernels.hpp): one shooting interval of
// one problem.  A text, not a function: as a __forceinline__ function of the kernel's arguments the same statements came out
// with other registers and schedules in every instantiation (one or two VGPRs and tens of instructions, either way).
// Expects in scope: R, M, the kernel's arguments, SP (the spacing: a constant or a.SP), kInRegs (Gamma of the interval in
// registers: SP is a constant) and SPC (the bound of that register block).
  constexpr int NX = M::NX;
  const int64_t gid = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int s = (int)(gid / a.B);
  const unsigned p = (unsigned)(gid - (int64_t)s * a.B);
  if (s >= a.S - 1) return;
  const int64_t st = a.stride;
  if (status != nullptr && status[IS_STATUS * st + p] != kTermNone) return;
  const typename M::Consts k = load_consts(a, p);
  const ExtForce<R> fe{R(0), R(0), R(0)};

  R x[NX], xe[NX];
  unpack<R, NX>(zx_in[(int64_t)s * st + p], x);
  unpack<R, NX>(zx_in[(int64_t)(s + 1) * st + p], xe);
  R Phi[NX][NX];
  R Gam[kInRegs ? SPC : 1][NX];
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = 0; c < NX; ++c) Phi[r][c] = (r == c) ? R(1) : R(0);
  if constexpr (kInRegs) {  // (loops, not `= {}`, which comes out as other instructions)
#pragma unroll
    for (int j = 0; j < SPC; ++j)
#pragma unroll
      for (int r = 0; r < NX; ++r) Gam[j][r] = R(0);
  }

  const int64_t first = kInRegs ? (int64_t)(s * SP) * st : (int64_t)s * SP * st;  // (each kernel its own form, as it was)
  const R* zu = zu_in + first;
  XV<R, NX>* gam = a.Gam + first;
  R u_next = kInRegs ? zu[p] : R(0);
  typename M::StepCache chain;  // the stages of a step share the sine / cosine base (models.hpp)
#pragma unroll 1
  for (int i = 0; i < SP; ++i) {
    R u = u_next;
    if constexpr (kInRegs) {
      if (i + 1 < SP) u_next = zu[(int64_t)(i + 1) * st + p];  // prefetch the next control
    } else {
      u = zu[(int64_t)i * st + p];
    }
    R A[NX][NX], Bv[NX];
    rk4_step_jac_m<R, M, false>(k, a.dt, x, u, fe, A, Bv, chain);
    // Phi <- A Phi
    R T[NX][NX];
#pragma unroll
    for (int r = 0; r < NX; ++r)
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        R acc = A[r][0] * Phi[0][c];
#pragma unroll
        for (int m = 1; m < NX; ++m) acc += A[r][m] * Phi[m][c];
        T[r][c] = acc;
      }
#pragma unroll
    for (int r = 0; r < NX; ++r)
#pragma unroll
      for (int c = 0; c < NX; ++c) Phi[r][c] = T[r][c];
    // Gamma columns: j < i propagate, j == i is the new control's column
    if constexpr (kInRegs) {
      // `i` is uniform over the wave, so these are scalar branches and the register indices stay static
#pragma unroll
      for (int j = 0; j < SPC; ++j) {
        if (j < i) {
          R g[NX];
#pragma unroll
          for (int m = 0; m < NX; ++m) g[m] = Gam[j][m];
#pragma unroll
          for (int r = 0; r < NX; ++r) {
            R acc = A[r][0] * g[0];
#pragma unroll
            for (int m = 1; m < NX; ++m) acc += A[r][m] * g[m];
            Gam[j][r] = acc;
          }
        } else if (j == i) {
#pragma unroll
          for (int r = 0; r < NX; ++r) Gam[j][r] = Bv[r];
        }
      }
    } else {
#pragma unroll 1
      for (int j = 0; j < i; ++j) {
        R g[NX], gn[NX];
        unpack<R, NX>(gam[(int64_t)j * st + p], g);
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          R acc = A[r][0] * g[0];
#pragma unroll
          for (int m = 1; m < NX; ++m) acc += A[r][m] * g[m];
          gn[r] = acc;
        }
        gam[(int64_t)j * st + p] = pack<R, NX>(gn);
      }
      gam[(int64_t)i * st + p] = pack<R, NX>(Bv);
    }
  }
  // wrap the angles once at the end of the interval, then the defect (optimization.cc:139,156-157)
  wrap_angles<R, M>(x);
  R c[NX];
#pragma unroll
  for (int t = 0; t < NX; ++t) c[t] = x[t] - xe[t];
  wrap_angles<R, M>(c);
  a.cs[(int64_t)s * st + p] = pack<R, NX>(c);
#pragma unroll
  for (int r = 0; r < NX; ++r) a.Phi[(int64_t)(NX * s + r) * st + p] = pack<R, NX>(Phi[r]);
  if constexpr (kInRegs) {
#pragma unroll
    for (int j = 0; j < SPC; ++j) a.Gam[(int64_t)(s * SP + j) * st + p] = pack<R, NX>(Gam[j]);
  }
