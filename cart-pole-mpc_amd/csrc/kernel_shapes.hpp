// kernel_shapes.hpp -- which forms of the SQP kernels are compiled, and what LDS a wave of the fused kernel takes: each
// written ONCE, in plain C++17 with no device code, so that the C-ABI units (what use_fused() picks and
// cpmpc_set_pipeline(FUSED) accepts: engine.hpp, cpmpc_api.hip), the launches (engine_impl.hpp) and the kernels themselves
// (mpc_fused.hpp) read the same lists and the same arithmetic.
#pragma once
#include <cstddef>
#include <type_traits>
#include <utility>

namespace cpmpc {

// ---- the compiled forms ------------------------------------------------------------------------------------------------
// linearize_kernel<R, M, SP>: state spacings with the interval's Gamma in registers; any other spacing runs
// linearize_dyn_kernel (run-time spacing, Gamma accumulated in the workspace)
using LinearizeSpacings = std::integer_sequence<int, 1, 2, 4, 5, 8, 10, 20>;

// fused_sqp_kernel<R, M, SP, L, ...>: the (L = S-1 lanes per problem, SP) pairs of the default horizon's spacings (N = 40)
// and of N = 20 ...
template <int L_, int SP_>
struct FusedPair {
  static constexpr int L = L_, SP = SP_;
};
template <typename... Pairs>
struct FusedPairList {};
using FusedStaticPairs = FusedPairList<FusedPair<4, 10>, FusedPair<8, 5>, FusedPair<2, 10>, FusedPair<4, 5>, FusedPair<2, 20>,
                                       FusedPair<5, 8>, FusedPair<10, 4>>;
// ... and fused_sqp_dyn_kernel<R, M, L, ...> (run-time spacing, dynamic LDS) for any other spacing with one of these
// interval counts whose per-wave LDS fits a dynamic allocation
using FusedDynamicGroups = std::integer_sequence<int, 2, 4, 5, 8, 10, 16>;

// Dispatch over those lists: f(std::integral_constant<int, V>) for the V of the sequence that equals v, f(FusedPair<L, SP>)
// for the pair of the list that equals (L, SP) -> whether there was one.  The launches (engine_impl.hpp) instantiate their
// kernels through these; the predicates are the same folds with nothing to do.
template <int... V, typename F>
constexpr bool dispatch_value(int v, std::integer_sequence<int, V...>, F f) {
  return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
}
template <typename... P, typename F>
constexpr bool dispatch_pair(int L, int SP, FusedPairList<P...>, F f) {
  return ((L == P::L && SP == P::SP ? (f(P{}), true) : false) || ...);
}
constexpr bool linearize_specialised(int sp) { return dispatch_value(sp, LinearizeSpacings{}, [](auto) {}); }
constexpr bool fused_static(int L, int SP) { return dispatch_pair(L, SP, FusedStaticPairs{}, [](auto) {}); }
constexpr bool fused_dynamic_group(int L) { return dispatch_value(L, FusedDynamicGroups{}, [](auto) {}); }

// ---- LDS: the limits, then Gamma's columns, the slim rule and the bytes of a wave -------------------------------------
constexpr size_t kMaxDynamicLdsBytes = 64 * 1024;  // what a launch may ask for as dynamic shared memory
constexpr size_t kCuLdsBytes = 160 * 1024;         // LDS of a compute unit (gfx950)

// A column of Gamma_s is an NX-vector: 16 bytes (float, NX = 4), 24 (float, NX = 6), 32 (double, NX = 4) or 48 (double,
// NX = 6), stored as the pieces it fills at [(i * 64 + lane) * pieces + p].  Round 5 dropped the padding of the 6-state
// columns to 32 / 64 bytes: Gamma is 30 KB instead of 40 KB per wave for the double 6-state kernel, three waves per CU
// instead of two (and four with the slim layout below).  Lane-consecutive 16-byte planes, [(i * pieces + p) * 64 + lane],
// remove the 2-way LDS bank conflicts of the wider columns (SQ_LDS_BANK_CONFLICT 7 800 -> 0 cycles per wave) but were
// 0.5 % slower (round 4, fp64: 4.832 vs 4.805 ms; profiles/r04_f64_{planes,noplanes}_pmc_summary.json): the lone wave
// never waited on the conflicts, and the second address per access cost more than they did.
// A piece is 16 bytes where the column is a whole number of them (float / NX = 4: one; double / NX = 4: two; double /
// NX = 6: three) and 8 bytes otherwise (float / NX = 6: 24 bytes = three pieces of 8 instead of the padded 32: 15 KB of Gamma
// per wave instead of 20, which is what lets the float 6-state kernel's LDS fit eight waves per CU, round 5).
constexpr int fused_g_piece_bytes(size_t esize, int nx) { return (nx * esize) % 16 != 0 ? 8 : 16; }
constexpr int fused_g_pieces(size_t esize, int nx) {
  return (int)((nx * esize + fused_g_piece_bytes(esize, nx) - 1) / fused_g_piece_bytes(esize, nx));
}
constexpr size_t fused_g_bytes(size_t esize, int nx) {  // LDS bytes of one column
  return (size_t)fused_g_pieces(esize, nx) * fused_g_piece_bytes(esize, nx);
}

// Slim layout for the double kernel of the 6-state model (round 5): with (U^-1 g)_k in the slot of du_k (the previous step
// is dead when sweep 1 writes it; sweep 1b turns it into v_k in place) and the 1/d_k of a lane's controls in registers, a
// wave needs u + du + Gamma = (8 + 8 + 48) x SP x 64 bytes = 40 KB at SP = 10 instead of 60 KB: four waves per CU -- one per
// SIMD, all the 512-register kernel can use -- instead of two.  Not for the REFINE instantiation
// (its second solve needs gw and du side by side).  For a third wave per SIMD the fp32 4-state kernel with (U^-1 g)_k in the
// slot of du_k measured 108.4 M re-plans/s against 116.3 M, and 99.0 M with the 1/d_k in registers too (round 3); the float
// 6-state kernel in the slim layout at two waves per SIMD spilled 533 dwords, 33 against 51 M (round 5).
// (of fused_sqp_kernel, the compiled pairs, only: the run-time-spacing kernel always takes the full layout)
constexpr bool fused_slim(size_t esize, int nx, int sp, bool refine) { return esize == 8 && nx > 4 && !refine && sp <= 10; }

// Bytes per wave: u, du, (U^-1 g), 1/d per control and lane (slim: u and du only) plus a column of Gamma per control and lane
constexpr size_t fused_static_lds_bytes(size_t esize, int nx, int sp, bool refine) {
  return (size_t)sp * 64 * ((fused_slim(esize, nx, sp, refine) ? 2 : 4) * esize + fused_g_bytes(esize, nx));
}
constexpr size_t fused_dyn_lds_bytes(size_t esize, int nx, int sp) {
  return (size_t)sp * 64 * (4 * esize + fused_g_bytes(esize, nx));
}

}  // namespace cpmpc
