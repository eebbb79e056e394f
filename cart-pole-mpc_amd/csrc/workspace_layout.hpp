// workspace_layout.hpp -- indices of the per-problem solver scalars kept in the workspace between kernels and the vector
// elements its fields are made of; shared by the kernels (mpc_kernels.hpp) and by the host code that sizes the workspace
// (cpmpc_api.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace cpmpc {

// per-problem real scalars kept in the workspace (index into `sc`)
// SC_TRIAL: 1 when SC_F_LAST / SC_CN_LAST are the merit pieces of the CURRENT iterate as the line search evaluated
// them (the accepted trial point IS the new iterate, bit for bit), 0 when no trial has been accepted yet
enum { SC_LAMBDA = 0, SC_MU, SC_F_LAST, SC_CN_LAST, SC_UPREV, SC_ALPHA, SC_TRIAL, SC_COUNT };
// per-problem int scalars (index into `ist`)
enum { IS_STATUS = 0, IS_ITERS, IS_LS_EVALS, IS_FAILED, IS_COUNT };
// bins of the histogram of SQP iterations per problem that finalize_kernel leaves for the host (the last bin collects
// every larger count) -- what the host plans the next step's stages of the fused pipeline from
constexpr int kFbBins = 16;
// at most this many workgroups of finalize_kernel report (every fb_stride-th one: a sample spread evenly over the batch)
constexpr int kFbReporters = 256;

// ---- the vector elements of the workspace ----
template <typename R>
struct VecT;
template <>
struct VecT<float> {
  using V4 = float4;
};
template <>
struct VecT<double> {
  using V4 = double4;
};

template <typename R>
__device__ __forceinline__ typename VecT<R>::V4 mk4(R a, R b, R c, R d) {
  typename VecT<R>::V4 v;
  v.x = a;
  v.y = b;
  v.z = c;
  v.w = d;
  return v;
}

// storage element of an NX-vector: ceil(NX/4) 4-vectors
template <typename R, int NX>
struct XV {
  typename VecT<R>::V4 v[(NX + 3) / 4];
};

template <typename R, int NX>
__device__ __forceinline__ void unpack(const XV<R, NX>& s, R (&x)[NX]) {
  x[0] = s.v[0].x;
  x[1] = s.v[0].y;
  x[2] = s.v[0].z;
  x[3] = s.v[0].w;
  if constexpr (NX > 4) {
    x[4] = s.v[1].x;
    x[5] = s.v[1].y;
  }
}
template <typename R, int NX>
__device__ __forceinline__ XV<R, NX> pack(const R (&x)[NX]) {
  XV<R, NX> s;
  s.v[0] = mk4<R>(x[0], x[1], x[2], x[3]);
  if constexpr (NX > 4) s.v[1] = mk4<R>(x[4], x[5], R(0), R(0));
  return s;
}

}  // namespace cpmpc
