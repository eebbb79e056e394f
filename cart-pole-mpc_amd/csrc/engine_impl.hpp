// engine_impl.hpp -- host side of the kernels of ONE (dtype, model) pair: argument set-up, launches, staging of the
// host-pointer calls.  Included by engine_<dtype>_<model>.hip only, which instantiates everything for its pair and
// exports it as an `Engine` table (engine.hpp); the C-ABI unit never sees device code.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>

#include "engine.hpp"
#include "mpc_kernels.hpp"
#include "mpc_fused.hpp"
#include "feedback_kernels.hpp"
#include "plant_kernels.hpp"
#include "plan_sensitivity_kernels.hpp"
#include "plan_vjp_kernels.hpp"
#include "plan_weight_vjp_kernels.hpp"
#include "sim_jac_kernels.hpp"
#include "sim_param_kernels.hpp"
#include "sim_rollout_kernels.hpp"
#include "sim_rollout_gn_kernels.hpp"
#include "sim_rollout_gn_x0_kernels.hpp"
#include "sim_ekf_kernels.hpp"
#include "sim_rts_kernels.hpp"
#include "sim_track_kernels.hpp"
#include "sim_ilqr_kernels.hpp"

using namespace cpmpc;

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
static inline dim3 grid_for(int64_t threads) { return dim3((unsigned)((threads + 63) / 64)); }

template <typename R, typename M>
static void fill_args(const cpmpc_solver* s, int64_t B, SolverArgs<R, M>& a, int64_t col0 = 0) {
  const cpmpc_params& p = s->params;
  const cpmpc_solver_opts& o = s->opts;
  memset((void*)&a, 0, sizeof a);
  a.B = B;
  a.stride = s->cap;
  a.N = s->N;
  a.S = s->S;
  a.SP = s->SP;
  a.iter_cap = (int)p.max_iterations;
  a.dt = (R)p.control_dt;
  // rows exist only for strictly positive weights (optimization.cc:270,296)
  a.wu = (R)(p.u_cost_weight > 0.0 ? p.u_cost_weight : 0.0);
  a.wd = (R)(p.u_derivative_cost_weight > 0.0 ? p.u_derivative_cost_weight : 0.0);
  // terminal rows in BuildProblem order (optimization.cc:236-267).  For the double pendulum (no optimizer
  // in the reference) th_final / th_dot_final apply to both poles, both targets are upright.
  a.term_is_cost = 0;
  for (int t = 0; t < M::NX; ++t) {
    double w, tgt;
    if (t == 0) {
      w = p.b_x_final_cost_weight;
      tgt = 0.0;
    } else if (t < M::NQ) {
      w = p.th_final_cost_weight;
      tgt = M_PI / 2;
    } else if (t == M::NQ) {
      w = p.b_x_dot_final_cost_weight;
      tgt = 0.0;
    } else {
      w = p.th_dot_final_cost_weight;
      tgt = 0.0;
    }
    const bool is_cost = w >= 0.0;
    a.term_w[t] = (R)(is_cost ? w : 1.0);
    a.term_tgt[t] = (R)tgt;
    if (is_cost) a.term_is_cost |= (1 << t);
  }
  a.max_ls = o.max_line_search_iterations;
  a.c1 = (R)o.armijo_c1;
  a.shrink_max = (R)o.ls_shrink_max;
  a.shrink_min = (R)o.ls_shrink_min;
  a.alpha_growth = (R)o.ls_alpha_growth;
  a.alpha_growth_bt = (R)o.ls_alpha_growth_backtracked;
  a.full_step_below = (R)o.full_step_below;
  a.cn_floor_scale = (R)(o.exit_defect_floor * (double)s->SP * (double)std::numeric_limits<R>::epsilon());
  a.rho = (R)o.penalty_rho;
  a.lam_init = (R)o.lambda_initial;
  a.lam_fail_init = (R)o.lambda_failure_init;
  a.lam_up = (R)o.lambda_scale_up;
  a.lam_down = (R)o.lambda_scale_down;
  a.lam_min = (R)o.lambda_min;
  a.lam_max = (R)o.lambda_max;
  a.bx_lim = (R)o.b_x_limit;
  a.u_lim = (R)o.u_limit;
  a.rel_tol = (R)p.relative_exit_tol;
  a.fo_tol = (R)p.absolute_first_derivative_tol;
  a.mu_init = (R)p.equality_penalty_initial;
  // problems [col0, col0 + B) of the workspace: every field is [field][cap] with the problem index fastest, so the call
  // works on a column range by offsetting the field bases (a chunk of a pipelined host-pointer step)
  a.prev_B = s->prev_B - col0 < 0 ? 0 : (s->prev_B - col0 > B ? B : s->prev_B - col0);
  a.refine_qp = s->refine_qp ? s->refine_passes : 0;
  using V4 = typename VecT<R>::V4;
  using XVn = XV<R, M::NX>;
  a.zx = (XVn*)s->zx + col0;
  a.zu = (R*)s->zu + col0;
  a.dzx = (XVn*)s->dzx + col0;
  a.dzu = (R*)s->dzu + col0;
  a.Phi = (XVn*)s->Phi + col0;
  a.Gam = (XVn*)s->Gam + col0;
  a.cs = (XVn*)s->cs + col0;
  a.Wk = (XVn*)s->Wk + col0;
  a.Tk = (V4*)s->Tk + col0;
  a.sc = (R*)s->sc + col0;
  a.ist = s->ist + col0;
  a.sin_table = (const R*)s->sin_table;
}

template <typename R, typename M>
static void launch_linearize(const SolverArgs<R, M>& a, int SP, const XV<R, M::NX>* zx_in, const R* zu_in,
                             const int32_t* status, hipStream_t stream) {
  const dim3 grid = grid_for(a.B * (a.S - 1));
  const bool specialised = dispatch_value(SP, LinearizeSpacings{}, [&](auto sp) {
    hipLaunchKernelGGL((linearize_kernel<R, M, decltype(sp)::value>), grid, dim3(64), 0, stream, a, zx_in, zu_in, status);
  });
  if (!specialised)  // no register-resident specialisation: run-time spacing, Gamma accumulated in the workspace
    hipLaunchKernelGGL((linearize_dyn_kernel<R, M>), grid, dim3(64), 0, stream, a, zx_in, zu_in, status);
}

// The instantiation of a fused kernel a launch takes, f(SHARED, REFINE) as std::bool_constants:
// REFINE: the double kernels' refinement of the whole QP solution (CPMPC_CREATE_REFINE_QP), the float kernels' QP in double
// (CPMPC_CREATE_WIDE_QP); constants through vector registers there (SHARED = false).
// SHARED, the shared-parameters specialisation (model constants wave-uniform, in SGPRs), is used in fp32 only: the fp64
// kernel already sits at the SGPR limit with its VGPR/AGPR file exhausted, and with the constants added to the
// scalar pressure hipcc 7.2 produced wrong results for it (caught by the fp64 parity tests); there the constants
// go through load_consts() into vector registers like per-problem parameters do.
template <typename R, typename F>
static auto with_fused_form(bool refine, bool shared_params, F f) {
  if (refine) return f(std::false_type{}, std::true_type{});
  if constexpr (sizeof(R) == 4) {
    if (shared_params) return f(std::true_type{}, std::false_type{});
  }
  return f(std::false_type{}, std::false_type{});
}

// -> whether a kernel was launched: the compiled (L, SP) pair, else the run-time-spacing kernel of the group size L
template <typename R, typename M>
static bool launch_fused(const SolverArgs<R, M>& a, int L, int SP, int max_iters, bool refine, hipStream_t stream) {
  const int ppw = 64 / L;
  const dim3 grid((unsigned)((a.B + ppw - 1) / ppw));
  return with_fused_form<R>(refine, a.dyn == nullptr, [&](auto shared, auto refined) {
    constexpr bool SH = decltype(shared)::value, RF = decltype(refined)::value;
    return dispatch_pair(L, SP, FusedStaticPairs{}, [&](auto pair) {
      using P = decltype(pair);
      hipLaunchKernelGGL((fused_sqp_kernel<R, M, P::SP, P::L, SH, RF>), grid, dim3(64), 0, stream, a, max_iters);
    }) || dispatch_value(L, FusedDynamicGroups{}, [&](auto group) {  // no specialisation for this spacing: run-time SP
      hipLaunchKernelGGL((fused_sqp_dyn_kernel<R, M, decltype(group)::value, SH, RF>), grid, dim3(64),
                         fused_dyn_lds_bytes(sizeof(R), M::NX, SP), stream, a, max_iters);
    });
  });
}

template <typename R, typename M>
static int step_batch_impl(cpmpc_solver* s, int64_t B, const cpmpc_step_inputs* in, const cpmpc_step_outputs* out,
                           hipStream_t stream, int64_t col0, int slot) {
  SolverArgs<R, M> a;
  fill_args<R, M>(s, B, a, col0);
  a.x0 = (const R*)in->x0;
  a.dyn = (const R*)in->dyn;
  a.set_point = (const R*)in->set_point;
  a.term_w_pp = (const R*)in->terminal_weights;
  if (in->dyn == nullptr) a.consts = M::template make<double>(in->dyn_shared_host);
  a.term_tgt[0] = (R)in->set_point_shared;
  if (out) {
    a.u_out = (R*)out->u;
    a.pred_out = (R*)out->predicted;
    a.status_out = out->status;
    a.iters_out = out->iterations;
    a.ls_out = out->ls_evals;
    a.cost_out = (R*)out->final_cost;
    a.eq_out = (R*)out->final_eq_l1;
    a.guess_out = (R*)out->guess;
    a.sol_out = (R*)out->solution;
  }
  const dim3 gridB = grid_for(B);
  ProfSpan sp;
  // float handles: the QP with its terminal part in double (CPMPC_CREATE_WIDE_QP).  A property of the HANDLE, never of the step:
  // round 6 tried "wide on cold-start steps only" as the 4-state default and withdrew it -- whether a call is a cold start
  // depends on which problems share the call, so a sharded handle (whose last shard may be all cold) and a single one (partly
  // warm) then ran different kernels on the same problem and batch-position independence was gone
  // (test_sharded_device_step_takes_per_problem_inputs...: bitwise equality across shardings)
  const bool wide_step = s->wide_qp;

  // (the first compaction's counter: cleared by prepare_kernel whether or not this step turns out to be staged)
  a.stage_count0 = (use_fused(s) && s->active != nullptr) ? s->active + s->cap + 3 * slot : nullptr;
  span_begin(s, CPMPC_KERNEL_PREPARE, stream, &sp);
  hipLaunchKernelGGL((prepare_kernel<R, M>), dim3((unsigned)((B + kPfBlock - 1) / kPfBlock)), dim3(kPfBlock), 0, stream, a);
  span_end(s, stream, &sp);

  if (use_fused(s)) {
    // With exit tolerances enabled problems stop after different numbers of iterations, and a wave lives as long
    // as its slowest problem (closed loop, measured: 4.3 iterations per problem, 7.7 per wave of 16).  The kernel
    // is restartable -- all solver state is in the workspace between launches -- so it runs in stages and the
    // problems still iterating are compacted into dense waves in between.  Results are bitwise those of a single
    // launch: a problem's arithmetic does not depend on the lanes it occupies.  Where the stages end is planned per
    // step (cpmpc_plan_stages: an explicit cpmpc_set_compaction, or from how many iterations the problems of an earlier
    // step needed).
    const int total = (int)s->params.max_iterations;
    const bool exits = s->params.relative_exit_tol > 0.0 || s->params.absolute_first_derivative_tol > 0.0;
    int bounds[kMaxStages + 1];
    const int n_stages = cpmpc_plan_stages(s, slot, B, exits, bounds);
    a.active_list = nullptr;
    a.active_count = nullptr;
    a.iter_cap = total;
    a.run_out_below = (int64_t)2048 * (64 / (s->S - 1));  // problems in one round of resident waves (2 per SIMD)
    // (cannot be reached: launch_fused dispatches over the very lists fused_built() reads, kernel_shapes.hpp.  Should the
    // two ever part, the step fails here instead of handing back the guess as a solution)
    auto not_launched = [&] {
      return fail(CPMPC_ERR_UNSUPPORTED, "no fused SQP kernel is compiled for L = S-1 = %d, SP = %d", s->S - 1, s->SP);
    };
    span_begin(s, CPMPC_KERNEL_FUSED, stream, &sp);
    bool launched = launch_fused<R, M>(a, s->S - 1, s->SP, bounds[1], sizeof(R) == 8 ? s->refine_qp : wide_step, stream);
    span_end(s, stream, &sp);
    if (!launched) return not_launched();
    for (int stage = 0; stage + 1 < n_stages; ++stage) {
      const int done = bounds[stage + 1];
      // three counters per host slot (chunks of a pipelined host step run concurrently), rotating: this compaction's, the
      // one before (prev_count), and the next one's, which this compaction clears; prepare_kernel cleared counters[0]
      int32_t* const counters = s->active + s->cap + 3 * slot;
      int32_t* count = counters + stage % 3;
      a.prev_count = stage ? counters + (stage - 1) % 3 : nullptr;
      a.prev_total = B;
      a.remaining = total - done;
      span_begin(s, CPMPC_KERNEL_FUSED, stream, &sp);
      hipLaunchKernelGGL((compact_active_kernel<M>), dim3((unsigned)((B + 1023) / 1024)), dim3(1024), 0, stream,
                         (const int32_t*)(a.ist + (size_t)IS_STATUS * (size_t)s->cap),
                         (const int32_t*)(a.ist + (size_t)IS_ITERS * (size_t)s->cap), total, B, s->active + col0, count,
                         counters + (stage + 1) % 3);
      a.active_list = s->active + col0;
      a.active_count = count;
      const int k = bounds[stage + 2] - done;
      launched = launch_fused<R, M>(a, s->S - 1, s->SP, k, sizeof(R) == 8 ? s->refine_qp : wide_step, stream);
      span_end(s, stream, &sp);
      if (!launched) return not_launched();
    }
  } else {
    for (int it = 0; it < (int)s->params.max_iterations; ++it) {
      span_begin(s, CPMPC_KERNEL_LINEARIZE, stream, &sp);
      launch_linearize<R, M>(a, s->SP, a.zx, a.zu, a.ist, stream);
      span_end(s, stream, &sp);
      span_begin(s, CPMPC_KERNEL_QP_LS, stream, &sp);
      if (sizeof(R) == 4 && wide_step)   // float handle with the QP's terminal part in double (CPMPC_CREATE_WIDE_QP)
        hipLaunchKernelGGL((qp_ls_kernel<R, M, true>), gridB, dim3(64), 0, stream, a);
      else
        hipLaunchKernelGGL((qp_ls_kernel<R, M, false>), gridB, dim3(64), 0, stream, a);
      span_end(s, stream, &sp);
    }
  }

  // the histogram of iterations per problem goes back to the host for the plan of a later step (default staging only)
  if (use_fused(s) && s->stage_auto && s->fb_host != nullptr && s->active != nullptr &&
      (s->params.relative_exit_tol > 0.0 || s->params.absolute_first_derivative_tol > 0.0)) {
    const int64_t groups = (B + kPfBlock - 1) / kPfBlock;
    a.fb_stride = (int)((groups + kFbReporters - 1) / kFbReporters);
    a.fb_host = s->fb_host_dev + (size_t)slot * kFbReporters * (kFbBins + 1);
    // sequence numbers 1 .. 2^30 and round again (0 = "no report yet"); compared modulo 2^30 in cpmpc_plan_stages
    s->fb_seq[slot] = s->fb_seq[slot] >= (1 << 30) ? 1 : s->fb_seq[slot] + 1;
    a.fb_seq = s->fb_seq[slot];
    s->fb_reporters[slot] = (int)((groups + a.fb_stride - 1) / a.fb_stride);
  }
  span_begin(s, CPMPC_KERNEL_FINALIZE, stream, &sp);
  hipLaunchKernelGGL((finalize_kernel<R, M>), dim3((unsigned)((B + kPfBlock - 1) / kPfBlock)), dim3(kPfBlock), 0, stream, a);
  span_end(s, stream, &sp);

  HIP_TRY(hipGetLastError());
  if (col0 + B > s->prev_B) s->prev_B = col0 + B;  // previous_solution_ = solver_->variables()  (optimization.cc:85), per problem
  return CPMPC_OK;
}

// ---- host-pointer steps: one chunk of problems through one staging slot ------------------------------------------------
// Staging layout of a chunk of Bc problems, identical on the device and in the pinned mirror:
//   [x0 | dyn? | set_point? | terminal_weights? | u | cost | eq | status | iters | solution? | predicted?]
// (inputs first: one copy in; outputs after them: one copy back, the optional tails last)
struct HostChunkLayout {
  size_t off_dyn = 0, off_sp = 0, off_tw = 0, off_u = 0, off_cost = 0, off_eq = 0, off_status = 0, off_iters = 0, off_sol = 0,
         off_pred = 0, end = 0;  // bytes
};

template <typename R, typename M>
static HostChunkLayout host_chunk_layout(const cpmpc_solver* s, int64_t Bc, bool per_dyn, bool per_sp, bool per_tw) {
  const size_t nB = (size_t)Bc, e = sizeof(R);
  HostChunkLayout L;
  L.off_dyn = (size_t)M::NX * nB * e;
  L.off_sp = L.off_dyn + (per_dyn ? (size_t)M::NP * nB * e : 0);
  L.off_tw = L.off_sp + (per_sp ? nB * e : 0);
  L.off_u = L.off_tw + (per_tw ? (size_t)M::NX * nB * e : 0);
  L.off_cost = L.off_u + (size_t)s->N * nB * e;
  L.off_eq = L.off_cost + nB * e;
  L.off_status = L.off_eq + nB * e;
  L.off_iters = L.off_status + nB * sizeof(int32_t);
  L.off_sol = (L.off_iters + nB * sizeof(int32_t) + 7) & ~(size_t)7;  // the real-typed tail starts 8-byte aligned
  L.off_pred = L.off_sol + (size_t)s->dim * nB * e;
  L.end = L.off_pred + (size_t)M::NX * (size_t)s->N * nB * e;
  return L;
}

// rows of the caller's [rows][ld] double array, columns [g0, g0 + n)  <->  [rows][n] of R in the pinned mirror, the rows
// spread over the library's worker threads (a 262 144-problem fp64 step returns 420 MB: one thread copies ~10 GB/s)
template <typename R>
struct RowCopy {
  const double* src_d;
  double* dst_d;
  R* mir;
  size_t ld, g0, n;
  bool to_mirror;
  static void run(int64_t r, void* ctx) {
    const RowCopy& c = *(const RowCopy*)ctx;
    R* m = c.mir + (size_t)r * c.n;
    if (c.to_mirror) {
      const double* src = c.src_d + (size_t)r * c.ld + c.g0;
      for (size_t i = 0; i < c.n; ++i) m[i] = (R)src[i];
    } else {
      double* dst = c.dst_d + (size_t)r * c.ld + c.g0;
      if constexpr (sizeof(R) == 8) memcpy(dst, m, c.n * 8);
      else for (size_t i = 0; i < c.n; ++i) dst[i] = (double)m[i];
    }
  }
};

template <typename R, typename M>
static int host_chunk_begin(cpmpc_solver* s, int slot_i, int64_t c0, int64_t Bc, int64_t g0, int64_t ld,
                            const cpmpc_step_host_inputs& in, const cpmpc_step_host_outputs& ho, bool direct) {
  const size_t nB = (size_t)Bc;
  const bool per_dyn = in.dyn != nullptr, per_sp = in.set_point != nullptr, per_tw = in.terminal_weights != nullptr;
  const bool want_pred = ho.predicted != nullptr, want_sol = ho.solution != nullptr;
  const HostChunkLayout L = host_chunk_layout<R, M>(s, Bc, per_dyn, per_sp, per_tw);
  int rc = ensure_slot(s, slot_i, L.end + 64);
  if (rc) return rc;
  HostSlot& sl = s->slot[slot_i];
  char* d_base = (char*)sl.dev;
  char* h_base = (char*)sl.pin;
  const hipStream_t st = sl.stream;
  // from here on work is in flight on `st` that reads the pinned mirror and writes the staging buffer: every early
  // return drains the stream first, so that the next call never reuses them under a running copy
  auto bail = [&](int code) {
    (void)hipStreamSynchronize(st);
    return code;
  };
  auto stage_in = [&](const double* src, size_t off, size_t rows) {
    RowCopy<R> c{src, nullptr, (R*)(h_base + off), (size_t)ld, (size_t)g0, nB, true};
    if (rows * nB < 65536) for (size_t r = 0; r < rows; ++r) RowCopy<R>::run((int64_t)r, &c);
    else host_parallel_for((int64_t)rows, &RowCopy<R>::run, &c);
  };
  stage_in(in.x0, 0, (size_t)M::NX);
  if (per_dyn) stage_in(in.dyn, L.off_dyn, (size_t)M::NP);
  if (per_sp) stage_in(in.set_point, L.off_sp, 1);
  if (per_tw) stage_in(in.terminal_weights, L.off_tw, (size_t)M::NX);
  hipError_t e = hipMemcpyAsync(d_base, h_base, L.off_u, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return bail(fail(CPMPC_ERR_HIP, "hipMemcpyAsync (inputs) failed: %s", hipGetErrorString(e)));

  cpmpc_step_inputs di;
  memset(&di, 0, sizeof di);
  di.x0 = d_base;
  di.dyn_shared_host = per_dyn ? nullptr : in.dyn_shared;
  di.dyn = per_dyn ? d_base + L.off_dyn : nullptr;
  di.set_point_shared = in.set_point_shared;
  di.set_point = per_sp ? d_base + L.off_sp : nullptr;
  di.terminal_weights = per_tw ? d_base + L.off_tw : nullptr;
  cpmpc_step_outputs out;
  memset(&out, 0, sizeof out);
  out.u = d_base + L.off_u;
  out.predicted = want_pred ? d_base + L.off_pred : nullptr;
  out.status = (int32_t*)(d_base + L.off_status);
  out.iterations = (int32_t*)(d_base + L.off_iters);
  out.final_cost = d_base + L.off_cost;
  out.final_eq_l1 = d_base + L.off_eq;
  out.solution = want_sol ? d_base + L.off_sol : nullptr;
  rc = step_batch_impl<R, M>(s, Bc, &di, &out, st, c0, slot_i);
  if (rc) return bail(rc);

  // Copy back.  A double handle whose real-typed output arrays the caller has pinned (hipHostMalloc / hipHostRegister /
  // cpmpc_host_register) gets them by DMA straight into those arrays, no pass of the CPU over the data; everything else
  // comes back into the mirror in one copy and is scattered by host_chunk_end.
  direct = direct && sizeof(R) == 8;
  if (direct) {
    auto d2h = [&](double* dst, size_t off, size_t rows) -> hipError_t {
      if (!dst) return hipSuccess;
      return hipMemcpy2DAsync(dst + (size_t)g0, (size_t)ld * 8, d_base + off, nB * 8, nB * 8, rows, hipMemcpyDeviceToHost, st);
    };
    e = d2h(ho.u, L.off_u, (size_t)s->N);
    if (e == hipSuccess) e = d2h(ho.solution, L.off_sol, (size_t)s->dim);
    if (e == hipSuccess) e = d2h(ho.predicted, L.off_pred, (size_t)M::NX * (size_t)s->N);
    if (e == hipSuccess)  // the small arrays still go through the mirror: cost, eq, status, iterations
      e = hipMemcpyAsync(h_base + L.off_cost, d_base + L.off_cost, L.off_iters + nB * sizeof(int32_t) - L.off_cost,
                         hipMemcpyDeviceToHost, st);
  } else {
    const size_t end = want_pred ? L.end : (want_sol ? L.off_pred : L.off_iters + nB * sizeof(int32_t));
    e = hipMemcpyAsync(h_base + L.off_u, d_base + L.off_u, end - L.off_u, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipEventRecord(sl.done, st);
  if (e != hipSuccess) return bail(fail(CPMPC_ERR_HIP, "copy back of a host-pointer step failed: %s", hipGetErrorString(e)));
  sl.busy = true;
  sl.c0 = c0;
  sl.Bc = Bc;
  sl.g0 = g0;
  sl.want_pred = want_pred;
  sl.want_sol = want_sol;
  sl.direct = direct;
  // the layout depends on which per-problem inputs were given: remember it through the flags host_chunk_end recomputes from
  sl.per_dyn = per_dyn;
  sl.per_sp = per_sp;
  sl.per_tw = per_tw;
  return CPMPC_OK;
}

template <typename R, typename M>
static int host_chunk_end(cpmpc_solver* s, int slot_i, int64_t ld, const cpmpc_step_host_outputs& ho) {
  HostSlot& sl = s->slot[slot_i];
  if (!sl.busy) return CPMPC_OK;
  sl.busy = false;
  HIP_TRY(hipEventSynchronize(sl.done));
  const size_t nB = (size_t)sl.Bc;
  const HostChunkLayout L = host_chunk_layout<R, M>(s, sl.Bc, sl.per_dyn, sl.per_sp, sl.per_tw);
  char* h_base = (char*)sl.pin;
  auto fetch = [&](size_t off, double* hdst, size_t rows) {
    if (!hdst) return;
    RowCopy<R> c{nullptr, hdst, (R*)(h_base + off), (size_t)ld, (size_t)sl.g0, nB, false};
    if (rows * nB < 65536) for (size_t r = 0; r < rows; ++r) RowCopy<R>::run((int64_t)r, &c);
    else host_parallel_for((int64_t)rows, &RowCopy<R>::run, &c);
  };
  if (!sl.direct) {
    fetch(L.off_u, ho.u, (size_t)s->N);
    if (sl.want_sol) fetch(L.off_sol, ho.solution, (size_t)s->dim);
    if (sl.want_pred) fetch(L.off_pred, ho.predicted, (size_t)M::NX * (size_t)s->N);
  }
  fetch(L.off_cost, ho.final_cost, 1);
  fetch(L.off_eq, ho.final_eq_l1, 1);
  if (ho.status) memcpy(ho.status + sl.g0, h_base + L.off_status, nB * sizeof(int32_t));
  if (ho.iterations) memcpy(ho.iterations + sl.g0, h_base + L.off_iters, nB * sizeof(int32_t));
  return CPMPC_OK;
}

template <typename R>
static ExtForce<R> ext_from_host(const double* fext_host) {
  ExtForce<R> fe{R(0), R(0), R(0)};
  if (fext_host) {
    fe.fbx = (R)fext_host[0];
    fe.fmx = (R)fext_host[2];
    fe.fmy = (R)fext_host[3];
  }
  return fe;
}

// ---- the remaining entry points of the table ----------------------------------------------------------------------
template <typename R, typename M>
static void pack_z_impl(cpmpc_solver* s, int64_t B, const void* z, hipStream_t stream) {
  hipLaunchKernelGGL((pack_z_kernel<R, M::NX>), grid_for(B), dim3(64), 0, stream, B, s->cap, s->S, s->N, (const R*)z,
                     (XV<R, M::NX>*)s->zx, (R*)s->zu);
}
template <typename R, typename M>
static void unpack_z_impl(cpmpc_solver* s, int64_t B, void* z_out, hipStream_t stream) {
  hipLaunchKernelGGL((unpack_z_kernel<R, M::NX>), grid_for(B), dim3(64), 0, stream, B, s->cap, s->S, s->N,
                     (const XV<R, M::NX>*)s->zx, (const R*)s->zu, (R*)z_out);
}
template <typename R, typename M>
static void dynamics_impl(int64_t B, const double* dyn_shared_host, const double* fext_host, const void* x, const void* u,
                          void* f, void* Jx, void* Ju, hipStream_t stream) {
  hipLaunchKernelGGL((dynamics_kernel<R, M>), grid_for(B), dim3(64), 0, stream, B,
                     M::template make<double>(dyn_shared_host), ext_from_host<R>(fext_host), (const R*)x, (const R*)u,
                     (R*)f, (R*)Jx, (R*)Ju);
}
template <typename R, typename M>
static void rk4_impl(int64_t B, const double* dyn_shared_host, const double* fext_host, double h, const void* x,
                     const void* u, void* x_new, void* A, void* Bm, hipStream_t stream) {
  hipLaunchKernelGGL((rk4_kernel<R, M>), grid_for(B), dim3(64), 0, stream, B, M::template make<double>(dyn_shared_host),
                     ext_from_host<R>(fext_host), (R)h, (const R*)x, (const R*)u, (R*)x_new, (R*)A, (R*)Bm);
}
template <typename R, typename M>
static void sim_impl(int64_t B, const double* dyn_shared_host, const double* fext_host, const void* fext, int n_sub,
                     double h_last, const void* u, void* state, hipStream_t stream) {
  hipLaunchKernelGGL((sim_kernel<R, M>), grid_for(B), dim3(64), 0, stream, B, M::template make<double>(dyn_shared_host),
                     ext_from_host<R>(fext_host), (const R*)fext, n_sub, (R)h_last, (const R*)u, (R*)state);
}
template <typename R, typename M>
static void sim_jac_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, const cpmpc_sim_jac* a,
                         hipStream_t stream) {
  hipLaunchKernelGGL((sim_jac_kernel<R, M>), grid_for(B), dim3(64), 0, stream, B, M::template make<double>(dyn_shared_host),
                     ext_from_host<R>(a->fext_host), (const R*)a->fext, n_sub, (R)h_last, (const R*)a->state,
                     (const R*)a->u, (R*)a->x_new, (R*)a->A, (R*)a->Bu, (const R*)a->gbar, (R*)a->gx, (R*)a->gu);
}

// ---- per-problem plant parameters, and the plant step's derivative in them (sim_param_kernels.hpp) ---------------------
// dyn [NP][B] on the device: the PER_LANE instantiations of the plant kernels.  A call that takes either set chooses the
// instantiation once, f(std::true_type) or f(std::false_type), and writes its argument list once:
template <typename F>
static void with_per_lane(bool per_lane, F f) {
  if (per_lane) f(std::true_type{});
  else f(std::false_type{});
}
// ... the kernels' first argument (plant_kernels.hpp: PlantConsts): the per-problem array, or the shared set folded here
template <typename R, typename M, bool PER_LANE>
static typename PlantConsts<R, M, PER_LANE>::Arg plant_consts_arg(const double* dyn_shared_host, const void* dyn) {
  if constexpr (PER_LANE) return (const R*)dyn;
  else return M::template make<double>(dyn_shared_host);
}
// ... and for the kernels that want the raw parameters too: the shared set folded and in R, or zeros that PER_LANE never reads
template <typename R, typename M>
struct SharedPlantParams {
  typename M::Consts k{};
  RawParams<R, M::NP> raw{};
};
template <typename R, typename M, bool PER_LANE>
static SharedPlantParams<R, M> shared_plant_params(const double* dyn_shared_host) {
  SharedPlantParams<R, M> s;
  if constexpr (!PER_LANE) {
    s.k = M::template make<double>(dyn_shared_host);
    for (int i = 0; i < M::NP; ++i) s.raw.p[i] = (R)dyn_shared_host[i];
  }
  return s;
}

template <typename R, typename M>
static void sim_dyn_impl(int64_t B, const void* dyn, const double* fext_host, const void* fext, int n_sub, double h_last,
                         const void* u, void* state, hipStream_t stream) {
  hipLaunchKernelGGL((sim_kernel<R, M, true>), grid_for(B), dim3(64), 0, stream, B, (const R*)dyn, ext_from_host<R>(fext_host),
                     (const R*)fext, n_sub, (R)h_last, (const R*)u, (R*)state);
}

// Width of a group of parameter columns of sim_param_jac_kernel: the largest for which no instantiation of the unit has
// scratch (-Rpass-analysis=kernel-resource-usage under the unit's flags; the table is in DESIGN.md 5f).  That is every
// column for all four (dtype, model) pairs, so a call is one launch; a pair that ever needs scratch specialises this.
template <typename R, typename M>
struct ParamGroupWidth {
  static constexpr int value = M::NP;
};

template <typename R, typename M, int J0, bool PER_LANE>
static void launch_param_groups(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, const cpmpc_sim_param_jac* a,
                                hipStream_t stream) {
  constexpr int W = ParamGroupWidth<R, M>::value;
  constexpr int NG = (J0 + W <= M::NP) ? W : M::NP - J0;
  R* x_new = (J0 == 0) ? (R*)a->x_new : nullptr;  // the primal step is every group's; the first one writes it
  if (x_new || a->P || a->gp) {
    const SharedPlantParams<R, M> sp = shared_plant_params<R, M, PER_LANE>(dyn_shared_host);
    hipLaunchKernelGGL((sim_param_jac_kernel<R, M, J0, NG, PER_LANE>), grid_for(B), dim3(64), 0, stream, B, sp.k, sp.raw,
                       (const R*)a->dyn, ext_from_host<R>(a->fext_host), (const R*)a->fext, n_sub, (R)h_last,
                       (const R*)a->state, (const R*)a->u, x_new, (R*)a->P, (const R*)(a->gp ? a->gbar : nullptr), (R*)a->gp);
  }
  if constexpr (J0 + NG < M::NP) launch_param_groups<R, M, J0 + NG, PER_LANE>(B, dyn_shared_host, n_sub, h_last, a, stream);
}

// gx / gu: sim_jac_kernel (the shared set: the instantiation cpmpc_sim_step_jac_batch launches); x_new, P, gp: the groups
template <typename R, typename M>
static void sim_param_jac_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, const cpmpc_sim_param_jac* a,
                               hipStream_t stream) {
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    if (a->gx || a->gu)
      hipLaunchKernelGGL((sim_jac_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                         plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host),
                         (const R*)a->fext, n_sub, (R)h_last, (const R*)a->state, (const R*)a->u, (R*)nullptr, (R*)nullptr,
                         (R*)nullptr, (const R*)a->gbar, (R*)a->gx, (R*)a->gu);
    if (a->x_new || a->P || a->gp) launch_param_groups<R, M, 0, PL>(B, dyn_shared_host, n_sub, h_last, a, stream);
  });
}

// ---- the plant over T ticks and its adjoint, one launch each (sim_rollout_kernels.hpp) ----------------------------------
template <typename R, typename M>
static void sim_rollout_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                             const cpmpc_sim_rollout* a, hipStream_t stream) {
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_rollout_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u, (R*)a->xs, (R*)a->x_final);
  });
}

template <typename R, typename M>
static void sim_rollout_vjp_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                                 const cpmpc_sim_rollout_vjp* a, hipStream_t stream) {
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    const SharedPlantParams<R, M> sp = shared_plant_params<R, M, PL>(dyn_shared_host);
    hipLaunchKernelGGL((sim_rollout_vjp_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B, sp.k, sp.raw, (const R*)a->dyn,
                       ext_from_host<R>(a->fext_host), (const R*)a->fext, n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u,
                       (const R*)a->xs, (const R*)a->gbar, (const R*)a->gbar_final, (R*)a->g_x0, (R*)a->g_u, (R*)a->g_p);
  });
}

// A host vector of per-state weights or variances as the kernels take it; NULL: `dflt` for every state
template <typename R, int NX>
static StateWeights<R, NX> state_weights(const double* v, double dflt) {
  StateWeights<R, NX> sw;
  for (int q = 0; q < NX; ++q) sw.w[q] = (R)(v ? v[q] : dflt);
  return sw;
}

// ---- the rollout's forward mode with the normal equations of the window, one launch (sim_rollout_gn_kernels.hpp) -------
template <typename R, typename M>
static void sim_rollout_gn_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                                const cpmpc_sim_rollout_gn* a, hipStream_t stream) {
  const StateWeights<R, M::NX> sw = state_weights<R, M::NX>(a->w_host, 1.0);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    const SharedPlantParams<R, M> sp = shared_plant_params<R, M, PL>(dyn_shared_host);
    hipLaunchKernelGGL((sim_rollout_gn_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B, sp.k, sp.raw, (const R*)a->dyn,
                       ext_from_host<R>(a->fext_host), (const R*)a->fext, n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u,
                       (const R*)a->x_obs, sw, (const R*)a->tick_w, (R*)a->cost, (R*)a->g, (R*)a->H, (R*)a->S_final,
                       (R*)a->x_final);
  });
}

// ---- the rollout's forward mode in the initial state with the normal equations, one launch (sim_rollout_gn_x0_kernels.hpp)
template <typename R, typename M>
static void sim_rollout_gn_x0_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                                   const cpmpc_sim_rollout_gn_x0* a, hipStream_t stream) {
  const StateWeights<R, M::NX> sw = state_weights<R, M::NX>(a->w_host, 1.0);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_rollout_gn_x0_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u, (const R*)a->x_obs, sw, (const R*)a->tick_w,
                       (R*)a->cost, (R*)a->g, (R*)a->H, (R*)a->Phi_final, (R*)a->x_final);
  });
}

// ---- the extended Kalman filter over T ticks, one launch (sim_ekf_kernels.hpp) ----------------------------------------
template <typename R, typename M>
static void sim_ekf_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T, const cpmpc_sim_ekf* a,
                         hipStream_t stream) {
  const StateWeights<R, M::NX> sw = state_weights<R, M::NX>(a->w_host, 1.0), q = state_weights<R, M::NX>(a->q_host, 0.0);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_ekf_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->P0, (const R*)a->u, (const R*)a->y, sw, q,
                       (const R*)a->tick_w, (R*)a->x_final, (R*)a->P_final, (R*)a->xs, (R*)a->nis);
  });
}

// ---- the Rauch-Tung-Striebel smoother over T ticks, two launches (sim_ekf_record_kernel, sim_rts_kernel) ---------------
template <typename R, typename M>
static void sim_rts_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T, const cpmpc_sim_rts* a,
                         hipStream_t stream) {
  const StateWeights<R, M::NX> sw = state_weights<R, M::NX>(a->w_host, 1.0), q = state_weights<R, M::NX>(a->q_host, 0.0);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_ekf_record_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->P0, (const R*)a->u, (const R*)a->y, sw, q,
                       (const R*)a->tick_w, (R*)a->x_final, (R*)a->P_final, (R*)a->xs, (R*)a->nis, (R*)a->work);
  });
  if (a->xs_smooth || a->Ps_smooth || a->x0_smooth || a->P0_smooth || a->ok)
    hipLaunchKernelGGL((sim_rts_kernel<R, M>), grid_for(B), dim3(64), 0, stream, B, T, (const R*)a->x0, (const R*)a->P0,
                       (const R*)a->work, (R*)a->xs_smooth, (R*)a->Ps_smooth, (R*)a->x0_smooth, (R*)a->P0_smooth, a->ok);
}

// ---- tracking a plant trajectory: its LQR gains, and the plant under them, one launch each (sim_track_kernels.hpp) --------
// The weights of the tracking cost as sim_lqr and the two iLQR passes take them: q, NULL: ones; and qf, the terminal diagonal
// where PT is NULL: qf_host, else q_host, else ones
template <typename R, int NX>
struct TrackWeights {
  StateWeights<R, NX> q, qf;
  TrackWeights(const double* q_host, const double* qf_host)
      : q(state_weights<R, NX>(q_host, 1.0)), qf(state_weights<R, NX>(qf_host ? qf_host : q_host, 1.0)) {}
};

template <typename R, typename M>
static void sim_lqr_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T, const cpmpc_sim_lqr* a,
                         hipStream_t stream) {
  const TrackWeights<R, M::NX> w(a->q_host, a->qf_host);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_lqr_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u, (const R*)a->xs, w.q, (R)a->r, (const R*)a->PT,
                       w.qf, (R*)a->K, (R*)a->P0);
  });
}

template <typename R, typename M>
static void sim_rollout_fb_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                                const cpmpc_sim_rollout_fb* a, hipStream_t stream) {
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_rollout_fb_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u_nom, (const R*)a->K, (const R*)a->x0_nom,
                       (const R*)a->xs_nom, (R)a->u_limit, (R*)a->xs, (R*)a->x_final, (R*)a->us);
  });
}

// ---- one iLQR iteration on the plant's tick map: the backward and the forward pass, one launch each (sim_ilqr_kernels.hpp) ----
template <typename R, typename M>
static void sim_ilqr_backward_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                                   const cpmpc_sim_ilqr_backward* a, hipStream_t stream) {
  const TrackWeights<R, M::NX> w(a->q_host, a->qf_host);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_ilqr_backward_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u, (const R*)a->xs, (const R*)a->x0_ref,
                       (const R*)a->xs_ref, (const R*)a->u_ref, w.q, (R)a->r, (const R*)a->PT, w.qf, (const R*)a->mu,
                       (R)a->u_limit, (R*)a->K, (R*)a->kff, (R*)a->dV, (R*)a->P0, (R*)a->g0, (R*)a->hmax);
  });
}

template <typename R, typename M>
static void sim_ilqr_forward_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                                  const cpmpc_sim_ilqr_forward* a, hipStream_t stream) {
  const TrackWeights<R, M::NX> w(a->q_host, a->qf_host);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_ilqr_forward_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u_nom, (const R*)a->kff, (const R*)a->K,
                       (const R*)a->x0_nom, (const R*)a->xs_nom, (const R*)a->alpha, (R)a->u_limit, (const R*)a->x0_ref,
                       (const R*)a->xs_ref, (const R*)a->u_ref, w.q, (R)a->r, (const R*)a->PT, w.qf, (R*)a->xs, (R*)a->x_final,
                       (R*)a->us, (R*)a->cost);
  });
}

template <typename R, typename M>
static void sim_ilqr_search_impl(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                                 const cpmpc_sim_ilqr_search* a, hipStream_t stream) {
  const TrackWeights<R, M::NX> w(a->q_host, a->qf_host);
  with_per_lane(a->dyn != nullptr, [&](auto per_lane) {
    constexpr bool PL = decltype(per_lane)::value;
    hipLaunchKernelGGL((sim_ilqr_search_kernel<R, M, PL>), grid_for(B), dim3(64), 0, stream, B,
                       plant_consts_arg<R, M, PL>(dyn_shared_host, a->dyn), ext_from_host<R>(a->fext_host), (const R*)a->fext,
                       n_sub, (R)h_last, T, (const R*)a->x0, (const R*)a->u_nom, (const R*)a->xs_nom, (const R*)a->cost_nom,
                       (const R*)a->kff, (const R*)a->K, (const R*)a->dV, (int)a->trials, (R)a->armijo, (R)a->u_limit,
                       (const R*)a->x0_ref, (const R*)a->xs_ref, (const R*)a->u_ref, w.q, (R)a->r, (const R*)a->PT, w.qf,
                       (R*)a->xs, (R*)a->x_final, (R*)a->us, (R*)a->cost, (R*)a->alpha);
  });
}

// ---- feedback gains and the sensitivities of the plan ----------------------------------------------------------------
// All four calls start alike: the arguments of a linearisation at z, then launch_linearize (a caller's z goes through the
// step buffers dzx / dzu, which hold no state between calls; z == NULL: the warm start itself, read only), then one lane
// per problem over Phi and Gamma.  Each call writes Phi,
// Gamma and cs, and the rows of Wk and Tk its kernel stores: scratch that every step recomputes before it reads it.
template <typename R, typename M>
static SolverArgs<R, M> gain_args(const cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in) {
  SolverArgs<R, M> a;
  fill_args<R, M>(s, B, a);
  a.dyn = (const R*)in->dyn;
  a.term_w_pp = (const R*)in->terminal_weights;
  if (in->dyn == nullptr) a.consts = M::template make<double>(in->dyn_shared_host);
  return a;
}

// the linearisation point of a call, as its kernel reads it
template <typename R, typename M>
struct PlanPoint {
  const XV<R, M::NX>* zx;
  const R* zu;
};

template <typename R, typename M>
static PlanPoint<R, M> linearize_at(const cpmpc_solver* s, const SolverArgs<R, M>& a, const void* z, hipStream_t st) {
  PlanPoint<R, M> at = {a.zx, a.zu};
  if (z != nullptr) {
    hipLaunchKernelGGL((pack_z_kernel<R, M::NX>), grid_for(a.B), dim3(64), 0, st, a.B, s->cap, s->S, s->N, (const R*)z,
                       a.dzx, a.dzu);
    at = {a.dzx, a.dzu};
  }
  launch_linearize<R, M>(a, s->SP, at.zx, at.zu, nullptr, st);
  return at;
}

// the linearisation at a caller's z, unpacked from the workspace
template <typename R, typename M>
static void linearize_batch_impl(cpmpc_solver* s, int64_t B, const double* dyn_shared_host, const void* z, void* c,
                                 void* Phi, void* Gamma, hipStream_t st) {
  SolverArgs<R, M> a;
  fill_args<R, M>(s, B, a);
  a.consts = M::template make<double>(dyn_shared_host);
  linearize_at<R, M>(s, a, z, st);
  hipLaunchKernelGGL((unpack_lin_kernel<R, M>), grid_for(B), dim3(64), 0, st, a, (R*)c, (R*)Phi, (R*)Gamma);
}

// KERNEL<R, M, WIDEQ> of the enclosing template's R and M, one lane per problem: the wide form for a float handle s with
// cpmpc_wide_qp(), else the plain one.  Undefined again below plan_weight_vjp_impl, its last user.
#define CPMPC_LAUNCH_WIDE_OR_PLAIN(KERNEL, s, B, st, ...)                                                \
  do {                                                                                                   \
    if (sizeof(R) == 4 && (s)->wide_qp)                                                                  \
      hipLaunchKernelGGL((KERNEL<R, M, true>), grid_for(B), dim3(64), 0, st, __VA_ARGS__);               \
    else                                                                                                 \
      hipLaunchKernelGGL((KERNEL<R, M, false>), grid_for(B), dim3(64), 0, st, __VA_ARGS__);              \
  } while (0)

template <typename R, typename M>
static void feedback_gain_impl(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K, int32_t* ok,
                               hipStream_t st) {
  const SolverArgs<R, M> a = gain_args<R, M>(s, B, in);
  linearize_at<R, M>(s, a, in->z, st);
  CPMPC_LAUNCH_WIDE_OR_PLAIN(feedback_gain_kernel, s, B, st, a, n_rows, (R*)K, ok);
}

template <typename R, typename M>
static void feedback_apply_impl(int64_t B, const void* u_nom, const void* K0, const void* x_nom, const void* x,
                                double u_limit, void* u_out, hipStream_t st) {
  hipLaunchKernelGGL((feedback_apply_kernel<R, M>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B,
                     (const R*)u_nom, (const R*)K0, (const R*)x_nom, (const R*)x, (R)u_limit, (R*)u_out);
}

// plan_sensitivity_kernel for the outputs that are not null
template <typename R, typename M>
static void plan_sensitivity_impl(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K, void* k_sp,
                                  void* k_up, int32_t* ok, hipStream_t st) {
  const SolverArgs<R, M> a = gain_args<R, M>(s, B, in);
  linearize_at<R, M>(s, a, in->z, st);
  CPMPC_LAUNCH_WIDE_OR_PLAIN(plan_sensitivity_kernel, s, B, st, a, n_rows, (R*)K, (R*)k_sp, (R*)k_up, ok);
}

template <typename R, typename M>
static void plan_update_impl(int64_t B, int n_rows, const cpmpc_plan_update* u, hipStream_t st) {
  hipLaunchKernelGGL((plan_update_kernel<R, M>), dim3((unsigned)((B + 255) / 256), (unsigned)n_rows), dim3(256), 0, st, B,
                     (const R*)u->u_nom, (const R*)u->K, (const R*)u->x_nom, (const R*)u->x, (const R*)u->k_sp,
                     (const R*)u->sp_nom, (const R*)u->sp, (const R*)u->k_up, (const R*)u->u_prev_nom,
                     (const R*)u->u_prev, (R)u->u_limit, (R*)u->u_out);
}

// reverse mode: plan_vjp_kernel for the outputs that are not null.  The kernel itself writes no workspace array.
template <typename R, typename M>
static void plan_vjp_impl(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, const void* gbar, void* g_x0,
                          void* g_sp, void* g_up, int32_t* ok, hipStream_t st) {
  const SolverArgs<R, M> a = gain_args<R, M>(s, B, in);
  linearize_at<R, M>(s, a, in->z, st);
  CPMPC_LAUNCH_WIDE_OR_PLAIN(plan_vjp_kernel, s, B, st, a, n_rows, (const R*)gbar, (R*)g_x0, (R*)g_sp, (R*)g_up, ok);
}

// weight gradients: plan_weight_vjp_kernel for the outputs that are not null, with the inputs the primal solve needs
// (x0, the set-point, u_prev) where a step has them
template <typename R, typename M>
static void plan_weight_vjp_impl(cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows, const void* gbar,
                                 void* g_tw, void* g_wu, void* g_wdu, void* du, int32_t* ok, hipStream_t st) {
  SolverArgs<R, M> a = gain_args<R, M>(s, B, &in->lin);
  a.x0 = (const R*)in->x0;
  a.set_point = (const R*)in->set_point;
  a.term_tgt[0] = (R)in->set_point_shared;
  const PlanPoint<R, M> at = linearize_at<R, M>(s, a, in->lin.z, st);
  CPMPC_LAUNCH_WIDE_OR_PLAIN(plan_weight_vjp_kernel, s, B, st, a, at.zx, at.zu, (const R*)in->u_prev, n_rows, (const R*)gbar,
                             (R*)g_tw, (R*)g_wu, (R*)g_wdu, (R*)du, ok);
}
#undef CPMPC_LAUNCH_WIDE_OR_PLAIN

// debug builds: this unit's copies of the counters (every translation unit has its own __device__ variables)
static int debug_read_impl(int which, unsigned long long* out) {
#ifdef CPMPC_FUSED_TIMING
  if (which == 0) {
    unsigned long long v[8], zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(cpmpc::g_fused_phase_cycles), sizeof v) != hipSuccess) return -1;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(cpmpc::g_fused_phase_cycles), zero, sizeof zero);
    for (int i = 0; i < 8; ++i) out[i] += v[i];
    return 0;
  }
#endif
#ifdef CPMPC_FUSED_CLOCK
  if (which == 1) {
    unsigned long long v[4], zero[4] = {0, 0, 0, 0};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(cpmpc::g_fused_clock), sizeof v) != hipSuccess) return -1;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(cpmpc::g_fused_clock), zero, sizeof zero);
    out[0] += v[0];
    out[1] += v[1];
    out[2] += v[2];
    if (v[3] > out[3]) out[3] = v[3];
    return 0;
  }
#endif
  (void)which;
  (void)out;
  return -1;
}

// The table of a (dtype, model) pair, its members filled by name: neighbours of one signature (the sim_* entries) cannot be
// swapped unseen, and the order of engine.hpp's declarations is free.  A new member gets a line here.
#define CPMPC_DEFINE_ENGINE(NAME, R, M)                                                                               \
  const Engine* NAME() {                                                                                              \
    static_assert(sizeof(Engine) == 30 * sizeof(void*), "an entry point of engine.hpp has no line below");            \
    static const Engine e = [] {                                                                                      \
      Engine t{};                                                                                                     \
      t.step_batch = &step_batch_impl<R, M>;              t.host_chunk_begin = &host_chunk_begin<R, M>;               \
      t.host_chunk_end = &host_chunk_end<R, M>;           t.pack_z = &pack_z_impl<R, M>;                              \
      t.unpack_z = &unpack_z_impl<R, M>;                  t.dynamics = &dynamics_impl<R, M>;                          \
      t.rk4 = &rk4_impl<R, M>;                            t.sim = &sim_impl<R, M>;                                    \
      t.sim_jac = &sim_jac_impl<R, M>;                    t.linearize_batch = &linearize_batch_impl<R, M>;            \
      t.debug_read = &debug_read_impl;                    t.feedback_gain = &feedback_gain_impl<R, M>;                \
      t.feedback_apply = &feedback_apply_impl<R, M>;      t.plan_sensitivity = &plan_sensitivity_impl<R, M>;          \
      t.plan_update = &plan_update_impl<R, M>;            t.plan_vjp = &plan_vjp_impl<R, M>;                          \
      t.plan_weight_vjp = &plan_weight_vjp_impl<R, M>;    t.sim_dyn = &sim_dyn_impl<R, M>;                            \
      t.sim_param_jac = &sim_param_jac_impl<R, M>;        t.sim_rollout = &sim_rollout_impl<R, M>;                    \
      t.sim_rollout_vjp = &sim_rollout_vjp_impl<R, M>;    t.sim_rollout_gn = &sim_rollout_gn_impl<R, M>;              \
      t.sim_rollout_gn_x0 = &sim_rollout_gn_x0_impl<R, M>; t.sim_ekf = &sim_ekf_impl<R, M>;                           \
      t.sim_rts = &sim_rts_impl<R, M>;                    t.sim_lqr = &sim_lqr_impl<R, M>;                            \
      t.sim_rollout_fb = &sim_rollout_fb_impl<R, M>;      t.sim_ilqr_backward = &sim_ilqr_backward_impl<R, M>;        \
      t.sim_ilqr_forward = &sim_ilqr_forward_impl<R, M>;  t.sim_ilqr_search = &sim_ilqr_search_impl<R, M>;            \
      return t;                                                                                                       \
    }();                                                                                                              \
    return &e;                                                                                                        \
  }
