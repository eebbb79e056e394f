// mpc_fused.hpp -- all SQP iterations of a batch in ONE kernel, a problem spread over L = S-1 lanes.
//
// The split pipeline (mpc_kernels.hpp) streams the sensitivities Gamma/Phi and the QP factors W/T through
// HBM between its kernels (measured 6.6 KB per problem and iteration, 40 % of the HBM peak, profiles/).
// Here lane s of a group of L consecutive lanes owns shooting interval s of one problem for the whole
// solve: its node x_s, Phi_s and defect live in registers; its SP controls, the step, Gamma_s and the
// per-control QP factors {1/d_k, (U^-1 g)_k} in lane-private LDS (80 scalars per lane = 20 KB per wave, so 8
// waves per CU = 2 per SIMD, which is also what the ~185 VGPRs allow); nothing of it reaches memory.
// Per iteration:
//   linearise      every lane integrates its own interval (RK4 + forward sensitivities), in parallel
//   QP sweeps      T = U D U^T, W = U^-1 R^T, gw = U^-1 g (down the horizon), then U^-T and the state recovery
//                  (up) are linear recurrences in k.  Every lane solves its own block in block-local
//                  coordinates (carry-in = 0) plus the scalar chain that says how a carry-in propagates; a
//                  chain of L-1 steps over the lanes (DPP row shifts) fixes the true block-boundary values
//                  {Psi_s, w_in, gw_in} / {dx_s, du_in}; each lane then corrects its block locally.  The
//                  pivots d_k depend on (lambda, weights) only: a Moebius recurrence whose block-boundary
//                  values come from powers of one 2x2 matrix, so no lane walks the whole horizon.
//   NX x NX LDL^T  every lane of the group solves the same small system (bitwise identical inputs: group
//                  sums are commutative butterflies over quad permutes)
//   line search    every lane rolls out its own interval of the trial point; the merit is a group sum
// 64/L problems share a wave, so the lock-step line search pays the maximum trial count over 16 (L = 4)
// problems instead of 64.  prepare_kernel / finalize_kernel of mpc_kernels.hpp run before / after,
// unchanged: the workspace fields zx, zu (iterate = warm start), sc and ist are this kernel's only global
// traffic.
//
// Same algorithm as the split pipeline (same QP, same line search, same decisions); the sweeps associate
// their sums differently, so results agree to rounding (fp64: 1e-9), not bitwise.
#pragma once
#include "kernel_shapes.hpp"
#include "mpc_kernels.hpp"

namespace cpmpc {

// ---- 2x2 matrices for the pivot recurrence (compile-time exponent, by squaring) -----------------------------
template <typename R>
struct Mat2 {
  R a, b, c, d;  // [[a, b], [c, d]]
};
template <typename R>
__device__ __forceinline__ Mat2<R> mat2_mul(const Mat2<R>& x, const Mat2<R>& y) {
  return Mat2<R>{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}
template <typename R, int E>
__device__ __forceinline__ Mat2<R> mat2_pow(const Mat2<R>& t) {
  if constexpr (E <= 0) {
    return Mat2<R>{R(1), R(0), R(0), R(1)};
  } else if constexpr (E == 1) {
    return t;
  } else if constexpr (E % 2 == 0) {
    const Mat2<R> h = mat2_pow<R, E / 2>(t);
    return mat2_mul<R>(h, h);
  } else {
    return mat2_mul<R>(mat2_pow<R, E - 1>(t), t);
  }
}

template <typename R>
__device__ __forceinline__ Mat2<R> mat2_pow_rt(const Mat2<R>& t, int e) {  // run-time exponent, e >= 0
  Mat2<R> acc{R(1), R(0), R(0), R(1)}, base = t;
  while (e > 0) {
    if (e & 1) acc = mat2_mul<R>(acc, base);
    base = mat2_mul<R>(base, base);
    e >>= 1;
  }
  return acc;
}

// ---- lane traffic inside a group ------------------------------------------------------------------------
// Groups are L consecutive lanes with L | 16, so they never straddle a 16-lane DPP row: neighbour moves are
// row shifts and, for L = 4 (one quad) and L = 2, sums and broadcasts are quad permutes.  DPP moves are VALU
// operand modifiers: no trip through the LDS crossbar as for ds_bpermute (__shfl), which matters in the
// boundary chains where every move is on the critical path.
template <int CTRL>
__device__ __forceinline__ int dpp32(int v) {
  // every lane is written (all rows and banks enabled; a lane whose source falls off its row reads 0), so there is no
  // previous value to preserve and no `v_mov_b32 dst, 0` in front of the move
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, dpp32<CTRL>(__builtin_bit_cast(int, v)));
}
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const unsigned lo = (unsigned)dpp32<CTRL>((int)(unsigned)(b & 0xffffffffll));
  const unsigned hi = (unsigned)dpp32<CTRL>((int)(unsigned)((unsigned long long)b >> 32));
  return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}
constexpr int kDppQuadXor1 = 1 | (0 << 2) | (3 << 4) | (2 << 6);  // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 2 | (3 << 2) | (0 << 4) | (1 << 6);  // quad_perm:[2,3,0,1]
constexpr int kDppRowShl1 = 0x101;                                // lane i reads lane i+1 (inside its row)
constexpr int kDppRowShr1 = 0x111;                                // lane i reads lane i-1 (inside its row)

// sum over the group, bitwise identical in all its lanes: a commutative butterfly when L is a power of two, else
// (groups of 5, 10, ... lanes) every lane adds the group's values in the same fixed order
template <typename R, int L>
__device__ __forceinline__ R group_sum(R v) {
  if constexpr (L == 4) {
    v += dpp<kDppQuadXor1>(v);
    v += dpp<kDppQuadXor2>(v);
  } else if constexpr (L == 2) {
    v += dpp<kDppQuadXor1>(v);
  } else if constexpr ((L & (L - 1)) == 0) {
#pragma unroll
    for (int off = 1; off < L; off <<= 1) v += __shfl_xor(v, off);
  } else {
    const int gb = (int)threadIdx.x - (int)threadIdx.x % L;
    R acc = __shfl(v, gb);
#pragma unroll
    for (int j = 1; j < L; ++j) acc += __shfl(v, gb + j);
    v = acc;
  }
  return v;
}
// maximum over the group, identical in all its lanes (a NaN operand is dropped, like nan_max)
template <typename R, int L>
__device__ __forceinline__ R group_max(R v) {
  if constexpr (L == 4) {
    v = nan_max(v, dpp<kDppQuadXor1>(v));
    v = nan_max(v, dpp<kDppQuadXor2>(v));
  } else if constexpr (L == 2) {
    v = nan_max(v, dpp<kDppQuadXor1>(v));
  } else if constexpr ((L & (L - 1)) == 0) {
#pragma unroll
    for (int off = 1; off < L; off <<= 1) v = nan_max(v, __shfl_xor(v, off));
  } else {
    const int gb = (int)threadIdx.x - (int)threadIdx.x % L;
    R acc = __shfl(v, gb);
#pragma unroll
    for (int j = 1; j < L; ++j) acc = nan_max(acc, __shfl(v, gb + j));
    v = acc;
  }
  return v;
}
// value of my right / left neighbour lane; callers discard it at the group edge.  Groups whose size divides 16
// never straddle a DPP row; the others go through the wave shuffle.
template <typename R, int L>
__device__ __forceinline__ R lane_right(R v) {
  if constexpr (16 % L == 0) return dpp<kDppRowShl1>(v);
  else return __shfl(v, (int)threadIdx.x + 1);
}
template <typename R, int L>
__device__ __forceinline__ R lane_left(R v) {
  if constexpr (16 % L == 0) return dpp<kDppRowShr1>(v);
  else return __shfl(v, (int)threadIdx.x - 1);
}
// value held by the first / last lane of my group
template <typename R, int L>
__device__ __forceinline__ R group_first(R v, int gbase) {
  if constexpr (L == 4) return dpp<0x00>(v);                              // quad_perm:[0,0,0,0]
  else if constexpr (L == 2) return dpp<(0 | (0 << 2) | (2 << 4) | (2 << 6))>(v);  // quad_perm:[0,0,2,2]
  else return __shfl(v, gbase);
}
template <typename R, int L>
__device__ __forceinline__ R group_last(R v, int gbase) {
  if constexpr (L == 4) return dpp<0xff>(v);                              // quad_perm:[3,3,3,3]
  else if constexpr (L == 2) return dpp<(1 | (1 << 2) | (3 << 4) | (3 << 6))>(v);  // quad_perm:[1,1,3,3]
  else return __shfl(v, gbase + L - 1);
}

// Waves per SIMD the register allocator must leave room for.  The sweeps are latency chains (LDS round trips,
// lane shuffles), so a second resident wave is worth a few spilled dwords in fp32 (measured +15%); fp64 values
// take two registers each and stay at one wave.
constexpr int kFusedWavesF32 = 2;
#define CPMPC_FUSED_BOUNDS __launch_bounds__(64, ((sizeof(R) == 4 && M::NX <= 4) ? kFusedWavesF32 : 1))
// unroll factor of the block-local sweep passes (LDS reads of several controls in flight)
constexpr int kFusedSweepUnroll = 5;

// Debug build only (-DCPMPC_FUSED_TIMING): shader-clock cycles per phase, summed over waves, read back by
// cpmpc_debug_phase_cycles().  Not part of the product library.
#ifdef CPMPC_FUSED_TIMING
static __device__ unsigned long long g_fused_phase_cycles[8];  // one copy per translation unit
#define CPMPC_TICK_INIT() unsigned long long tick_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tick_last = __builtin_readcyclecounter()
#define CPMPC_TICK(IDX)                                              \
  do {                                                               \
    __builtin_amdgcn_sched_barrier(0);                               \
    const unsigned long long tick_now = __builtin_readcyclecounter(); \
    tick_acc[IDX] += tick_now - tick_last;                           \
    tick_last = tick_now;                                            \
  } while (0)
#define CPMPC_TICK_FLUSH()                                                                       \
  do {                                                                                           \
    if (threadIdx.x == 0)                                                                        \
      for (int ti = 0; ti < 8; ++ti) atomicAdd(&g_fused_phase_cycles[ti], tick_acc[ti]);         \
  } while (0)
#else
#define CPMPC_TICK_INIT() do { } while (0)
#define CPMPC_TICK(IDX) do { } while (0)
#define CPMPC_TICK_FLUSH() do { } while (0)
#endif

// Debug build only (-DCPMPC_FUSED_CLOCK): every wave stamps the shader clock (s_memtime) and the constant 100 MHz
// counter (s_memrealtime) once on entry and once on exit; the sums over waves give the clock the part holds while this
// kernel runs (MI355X_MICROARCH.md, DVFS give-back item 6).  The stamps go to a buffer of their own that nothing else
// reads; read back by cpmpc_debug_kernel_clock().  Not part of the product library.
#ifdef CPMPC_FUSED_CLOCK
static __device__ unsigned long long g_fused_clock[4];  // sum of shader cycles, sum of 100 MHz ticks, waves, max cycles
#define CPMPC_CLOCK_BEGIN()                                                  \
  const unsigned long long clk_c0 = __builtin_amdgcn_s_memtime();           \
  const unsigned long long clk_r0 = __builtin_amdgcn_s_memrealtime()
#define CPMPC_CLOCK_END()                                                                          \
  do {                                                                                             \
    const unsigned long long clk_c1 = __builtin_amdgcn_s_memtime();                                \
    const unsigned long long clk_r1 = __builtin_amdgcn_s_memrealtime();                            \
    if (threadIdx.x == 0) {                                                                        \
      atomicAdd(&g_fused_clock[0], clk_c1 - clk_c0);                                               \
      atomicAdd(&g_fused_clock[1], clk_r1 - clk_r0);                                               \
      atomicAdd(&g_fused_clock[2], 1ull);                                                          \
      atomicMax(&g_fused_clock[3], clk_c1 - clk_c0);                                               \
    }                                                                                              \
  } while (0)
#else
#define CPMPC_CLOCK_BEGIN() do { } while (0)
#define CPMPC_CLOCK_END() do { } while (0)
#endif

// ---- LDS layout: kernel_shapes.hpp (the slim rule, Gamma's pieces, bytes per wave; why it is what it is) ----------------
template <int BYTES>
struct alignas(BYTES) GPieceT {
  unsigned w[BYTES / 4];
};
template <typename R, int NX>
using GPieceOf = GPieceT<fused_g_piece_bytes(sizeof(R), NX)>;
template <typename R, int NX>
__device__ __forceinline__ XV<R, NX> fused_g_ld(const GPieceOf<R, NX>* g, int i, int lane) {
  constexpr int K = fused_g_pieces(sizeof(R), NX);
  XV<R, NX> v;
  GPieceOf<R, NX> pc[K];
#pragma unroll
  for (int p = 0; p < K; ++p) pc[p] = g[(i * 64 + lane) * K + p];
  __builtin_memcpy(&v, pc, sizeof pc <= sizeof v ? sizeof pc : sizeof v);  // (the padding of v, if any, is never read)
  return v;
}
template <typename R, int NX>
__device__ __forceinline__ void fused_g_st(GPieceOf<R, NX>* g, int i, int lane, const XV<R, NX> v) {
  constexpr int K = fused_g_pieces(sizeof(R), NX);
  GPieceOf<R, NX> pc[K];
  __builtin_memcpy(pc, &v, sizeof pc <= sizeof v ? sizeof pc : sizeof v);
#pragma unroll
  for (int p = 0; p < K; ++p) g[(i * 64 + lane) * K + p] = pc[p];
}

// SHARED: the batch shares one parameter set -> the model constants stay wave-uniform (scalar registers)
// REFINE (double kernels only; CPMPC_CREATE_REFINE_QP): one step of iterative refinement of the whole QP solution with
// residuals from the original data (the block after sweep 2 in mpc_fused_body.inc)
template <typename R, typename M, int SP, int L, bool SHARED, bool REFINE>
__global__ CPMPC_FUSED_BOUNDS void fused_sqp_kernel(const SolverArgs<R, M> a, const int max_iters) {
  constexpr int NX = M::NX;
  constexpr int PPW = 64 / L;  // problems per wave
  constexpr bool kSlim = fused_slim(sizeof(R), NX, SP, REFINE);
  __shared__ R lds_u[SP * 64];
  __shared__ R lds_du[SP * 64];
  __shared__ GPieceOf<R, NX> lds_G[SP * 64 * fused_g_pieces(sizeof(R), NX)];  // column i of my Gamma_s (fused_g_ld / fused_g_st)
  __shared__ R lds_gw_own[kSlim ? 1 : SP * 64];  // (U^-1 g)_k of my controls
  __shared__ R lds_id[kSlim ? 1 : SP * 64];      // 1/d_k of my controls
  // (the slim form's two one-element placeholders aside, exactly what the host is told a wave takes)
  static_assert(sizeof lds_u + sizeof lds_du + sizeof lds_G + sizeof lds_gw_own + sizeof lds_id ==
                    fused_static_lds_bytes(sizeof(R), NX, SP, REFINE) + (kSlim ? 2 * sizeof(R) : 0),
                "the __shared__ arrays and kernel_shapes.hpp's layout disagree");
  R* const lds_gw = kSlim ? lds_du : lds_gw_own;
  R id_reg[kSlim ? SP : 1];
  constexpr int kSweepUnroll = kSlim ? SP : kFusedSweepUnroll;  // register-held 1/d_k need static indices: full unroll
#define CPMPC_ID_SET(I, V)                  \
  do {                                      \
    if constexpr (kSlim) id_reg[I] = (V);   \
    else lds_id[(I) * 64 + lane] = (V);     \
  } while (0)
#define CPMPC_ID_GET(I) (kSlim ? id_reg[kSlim ? (I) : 0] : lds_id[kSlim ? 0 : (I) * 64 + lane])
#define CPMPC_SWEEP_PRAGMA _Pragma("unroll kSweepUnroll")
// with the sweeps fully unrolled the scheduler hoists all ten controls' LDS reads to the top and spills; a scheduling
// barrier per control keeps the live ranges those of the rolled loop
#define CPMPC_SWEEP_FENCE()                                   \
  do {                                                        \
    if constexpr (kSlim) __builtin_amdgcn_sched_barrier(0);   \
  } while (0)
#define CPMPC_FUSED_MAT2_POW(T, E) mat2_pow<R, (E)>(T)
#include "mpc_fused_body.inc"
#undef CPMPC_FUSED_MAT2_POW
#undef CPMPC_SWEEP_PRAGMA
#undef CPMPC_SWEEP_FENCE
#undef CPMPC_ID_SET
#undef CPMPC_ID_GET
}

// The same kernel for a state spacing without a compiled specialisation: SP is a.SP at run time, the LDS arrays are
// carved from dynamic shared memory (fused_dyn_lds_bytes), the matrix powers use a run-time exponent.
template <typename R, typename M, int L, bool SHARED, bool REFINE>
__global__ CPMPC_FUSED_BOUNDS void fused_sqp_dyn_kernel(const SolverArgs<R, M> a, const int max_iters) {
  constexpr int NX = M::NX;
  constexpr int PPW = 64 / L;
  const int SP = a.SP;
  extern __shared__ __align__(32) unsigned char fused_dyn_lds[];
  GPieceOf<R, NX>* lds_G = reinterpret_cast<GPieceOf<R, NX>*>(fused_dyn_lds);   // widest elements first: stays aligned
  R* lds_u = reinterpret_cast<R*>(lds_G + (size_t)SP * 64 * fused_g_pieces(sizeof(R), NX));
  R* lds_du = lds_u + (size_t)SP * 64;
  R* lds_gw = lds_du + (size_t)SP * 64;
  R* lds_id = lds_gw + (size_t)SP * 64;
#define CPMPC_ID_SET(I, V) lds_id[(I) * 64 + lane] = (V)
#define CPMPC_ID_GET(I) (lds_id[(I) * 64 + lane])
#define CPMPC_SWEEP_PRAGMA _Pragma("unroll kFusedSweepUnroll")
#define CPMPC_SWEEP_FENCE() do { } while (0)
#define CPMPC_FUSED_MAT2_POW(T, E) mat2_pow_rt<R>(T, (E))
#include "mpc_fused_body.inc"
#undef CPMPC_FUSED_MAT2_POW
#undef CPMPC_SWEEP_PRAGMA
#undef CPMPC_SWEEP_FENCE
#undef CPMPC_ID_SET
#undef CPMPC_ID_GET
}

}  // namespace cpmpc
