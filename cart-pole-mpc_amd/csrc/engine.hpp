// engine.hpp -- what the C-ABI translation units (cpmpc_api.hip, cpmpc_host.hip, cpmpc_sharded.hip) and the four kernel
// units (engine_<dtype>_<model>.hip) share: the solver handle, the error / profiling / staging helpers the API owns, and the
// table of entry points through which the API reaches the kernels of one (dtype, model) pair.  The library is built
// from seven objects compiled in parallel; only the engine units contain device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/cpmpc.h"
#include "kernel_shapes.hpp"
#include "workspace_layout.hpp"

using namespace cpmpc;

#define CPMPC_HIDDEN __attribute__((visibility("hidden")))

// thread-local error text (cpmpc_last_error); returns `code`
CPMPC_HIDDEN int cpmpc_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define fail cpmpc_fail

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(CPMPC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                  __FILE__, __LINE__);                                                      \
  } while (0)

struct ProfSpan {
  int kernel;
  hipEvent_t start, stop;
};

// Staging of the host-pointer entry points: a device buffer, its pinned host mirror, a stream and an event.  A handle
// owns kHostSlots of them so that a large host-pointer step runs as a pipeline of chunks: while the CPU scatters chunk k's
// results into the caller's arrays, chunk k+1 is copying back and chunk k+2 is in the kernels.
constexpr int kHostSlots = 3;
constexpr int kMaxStages = 16;  // launches of the fused kernel per step at most (the plan of a step's stages)
struct HostSlot {
  void* dev = nullptr;
  void* pin = nullptr;
  size_t bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // the copy back of the chunk in flight has landed in `pin`
  // the chunk in flight (host_chunk_begin -> host_chunk_end)
  bool busy = false;
  int64_t c0 = 0, Bc = 0, g0 = 0;   // first problem in the handle's workspace, problems, first column in the caller's arrays
  bool want_pred = false, want_sol = false;
  bool direct = false;              // real-typed outputs were copied straight into the caller's (pinned) arrays
  bool per_dyn = false, per_sp = false, per_tw = false;  // which per-problem inputs the chunk carried (staging layout)
};

// the last plan made from a histogram, per host slot (cpmpc_plan_stages)
struct PlanCache {
  int seq = 0;
  int64_t B = 0;
  double n_hist = 0.0;
  int n = 0;
  int bounds[kMaxStages + 1] = {0};
  // the last two different histograms the host has seen on the slot, as fractions of problems per bin
  int seen_seq = 0;
  double seen[kFbBins] = {0};
  bool have_prev = false, stationary = false;
};

struct cpmpc_solver {
  cpmpc_params params;
  cpmpc_solver_opts opts;
  int dtype;
  int model;
  int device;
  int64_t cap;  // workspace stride (capacity rounded up to a multiple of 64)
  int N, S, SP, NX, NP, dim;
  size_t esize;
  // one allocation, carved into fields
  void* ws = nullptr;
  size_t ws_bytes = 0;
  char *zx, *zu, *dzx, *dzu, *Phi, *Gam, *cs, *Wk, *Tk, *sc;
  int32_t* ist;
  void* sin_table = nullptr;
  int64_t prev_B = 0;  // problems [0, prev_B) hold a previous solution; Reset() -> 0
  // staging for the *_host entry points (lazily allocated, grown on demand, owned by the handle)
  HostSlot slot[kHostSlots];
  int64_t host_chunk = -1;       // problems per chunk of a pipelined host-pointer step (cpmpc_set_host_chunk); -1 = by batch size
  hipEvent_t ev_last = nullptr;  // end of the last device-pointer call on a caller's stream; the slot streams wait on it
  bool ev_pending = false;
  // profiling
  int profiling = 0;
  std::vector<ProfSpan> spans;
  std::vector<ProfSpan> free_spans;
  double prof_ms[CPMPC_KERNEL_COUNT] = {0, 0, 0, 0, 0};
  int64_t prof_n[CPMPC_KERNEL_COUNT] = {0, 0, 0, 0, 0};
  int pipeline = CPMPC_PIPELINE_AUTO;
  bool refine_qp = false;  // CPMPC_CREATE_REFINE_QP: the double fused kernels refine the whole QP solution once
  bool beyond_parity = false;  // window_length * control_dt > cpmpc_max_parity_horizon(): cpmpc_horizon_beyond_parity()
  int refine_passes = 0;   // double, both pipelines: passes of that refinement (1; 2 beyond the parity horizon: cpmpc_api.hip; SolverArgs::refine_qp)
  bool wide_qp = false;    // CPMPC_CREATE_WIDE_QP (default for the 6-state model): the float fused kernels (compiled spacings) carry the QP's terminal part in double
  // staged fused pipeline (compaction of the still-active problems between stages); 0/0 = single launch
  // default 2 / 1 (round 4, tools/steady_state.py): in the warm-started closed loop most problems stop after one or two
  // iterations, so compacting after two pays (fp32 at the reference's tolerances 1.47 -> 1.34 ms per tick, the swing-up
  // transient -4 %); a stage that finds nobody left costs one empty launch (7 us)
  int stage_first = 2, stage_next = 1;
  bool stage_auto = true;  // default: stage only batches larger than one round of resident waves
  int32_t* active = nullptr;  // [cap] compacted problem indices, then two counters
  // the stages of the fused pipeline, planned per step (stage_auto) from the histogram of iterations per problem that
  // finalize_kernel left in host-mapped memory after an earlier step: per host slot, kFbReporters blocks of kFbBins + 1
  // ints (a reporting workgroup's counts + the sequence number of its step)
  int32_t* fb_host = nullptr;
  int32_t* fb_host_dev = nullptr;  // the device's address of fb_host
  int fb_seq[kHostSlots] = {0, 0, 0};
  int fb_reporters[kHostSlots] = {0, 0, 0};  // reporting workgroups of the last step launched on the slot
  int last_plan[kMaxStages + 1] = {0};  // boundaries of the stages of the last step (cpmpc_get_stage_plan)
  int last_plan_n = 0;
  PlanCache plan_cache[kHostSlots];
};


// owned by the C-ABI units (cpmpc_api.hip: spans, plan; cpmpc_host.hip: slots, threads)
CPMPC_HIDDEN void span_begin(cpmpc_solver* s, int kernel, hipStream_t stream, ProfSpan* cur);
CPMPC_HIDDEN void span_end(cpmpc_solver* s, hipStream_t stream, ProfSpan* cur);
CPMPC_HIDDEN int ensure_slot(cpmpc_solver* s, int slot, size_t bytes);
// the stages of the fused pipeline for a step of B problems: bounds[0] = 0 < ... < bounds[n] = max_iterations, returns n
CPMPC_HIDDEN int cpmpc_plan_stages(cpmpc_solver* s, int slot, int64_t B, bool exits, int* bounds);
// run fn(i) for i in [0, n) on the library's worker threads (the calling thread takes part); returns when all are done
CPMPC_HIDDEN void host_parallel_for(int64_t n, void (*fn)(int64_t i, void* ctx), void* ctx);

// fused pipeline: compiled specialisations for some (L = S-1, SP) pairs, and a run-time-spacing variant (dynamic LDS) for
// any other spacing with a compiled interval count whose per-wave LDS (80 scalars per lane and control for NX = 4) fits a
// dynamic allocation (kernel_shapes.hpp: the lists and the layout)
static inline bool fused_built(const cpmpc_solver* s) {
  return fused_static(s->S - 1, s->SP) ||
         (fused_dynamic_group(s->S - 1) && fused_dyn_lds_bytes(s->esize, s->NX, s->SP) <= kMaxDynamicLdsBytes);
}
// LDS a wave of the fused kernel takes for this handle: the compiled pair's layout (slim or not), else the dynamic one
static inline size_t fused_wave_lds_bytes(const cpmpc_solver* s) {
  return fused_static(s->S - 1, s->SP) ? fused_static_lds_bytes(s->esize, s->NX, s->SP, s->refine_qp)
                                       : fused_dyn_lds_bytes(s->esize, s->NX, s->SP);
}

static inline bool use_fused(const cpmpc_solver* s) {
  if (s->pipeline == CPMPC_PIPELINE_SPLIT) return false;
  if (!fused_built(s)) return false;
  // AUTO: the double kernel of the 6-state model, which holds all 512 registers (one wave per SIMD at best), runs fused
  // where at least three of its waves fit a CU's 160 KB of LDS: 40 KB per wave at
  // state_spacing 10 since round 5 (four per CU: 23.4 M re-plans/s at B = 65 536 against 13.7 M split; with the padded
  // 60 KB layout of rounds 1-4, two per CU, it was 14.4 M and AUTO kept the split pipeline), 100 KB at spacing 20 (one per
  // CU: split).
  // (the other kernels keep what rounds 1-4 measured for them: fused wherever built)
  if (s->pipeline == CPMPC_PIPELINE_AUTO && s->model == CPMPC_MODEL_DOUBLE && s->dtype == CPMPC_F64 &&
      3 * fused_wave_lds_bytes(s) > kCuLdsBytes)
    return false;
  // AUTO beyond the parity horizon (fp64; round 6): the split pipeline, whose QP kernel runs TWO refinement passes there -- from
  // the second pass on the refined condensed solve is more accurate than a dense pivoted LU on the worst cold starts
  // (kernels at fault on 1 lane of 8 192 at 1.6 s, like the CPU check; the fused kernel's one pass: 3).
  // Throughput is not the bar there; cpmpc_set_pipeline(FUSED) is the caller's to choose.
  if (s->pipeline == CPMPC_PIPELINE_AUTO && s->beyond_parity && s->dtype == CPMPC_F64 && s->refine_qp) return false;
  return true;
}

// Entry points of one (dtype, model) pair; every function launches the kernels of its own translation unit.
struct Engine {
  // Optimization::Step for B problems on `stream` (optimization.cc:39-97)
  // (col0: first problem of the handle's workspace the call works on; slot: which pair of compaction counters)
  int (*step_batch)(cpmpc_solver* s, int64_t B, const cpmpc_step_inputs* in, const cpmpc_step_outputs* out,
                    hipStream_t stream, int64_t col0, int slot);
  // one chunk of a host-pointer step in two halves: `begin` converts and uploads problems [c0, c0 + Bc) of the handle
  // (columns [g0, g0 + Bc) of the caller's [field][ld] arrays), queues the kernels and the copy back on the slot's
  // stream; `end` waits for it and scatters the results into the caller's arrays
  // (direct: copy the real-typed outputs by DMA straight into the caller's pinned arrays -- decided once per call)
  int (*host_chunk_begin)(cpmpc_solver* s, int slot, int64_t c0, int64_t Bc, int64_t g0, int64_t ld,
                          const cpmpc_step_host_inputs& in, const cpmpc_step_host_outputs& out, bool direct);
  int (*host_chunk_end)(cpmpc_solver* s, int slot, int64_t ld, const cpmpc_step_host_outputs& out);
  // packed z [dim][B] (MapKey order) <-> workspace
  void (*pack_z)(cpmpc_solver* s, int64_t B, const void* z, hipStream_t stream);
  void (*unpack_z)(cpmpc_solver* s, int64_t B, void* z_out, hipStream_t stream);
  // stand-alone pieces
  void (*dynamics)(int64_t B, const double* dyn_shared_host, const double* fext_host, const void* x, const void* u,
                   void* f, void* Jx, void* Ju, hipStream_t stream);
  void (*rk4)(int64_t B, const double* dyn_shared_host, const double* fext_host, double h, const void* x, const void* u,
              void* x_new, void* A, void* Bm, hipStream_t stream);
  void (*sim)(int64_t B, const double* dyn_shared_host, const double* fext_host, const void* fext, int n_sub,
              double h_last, const void* u, void* state, hipStream_t stream);
  // the same step from a read-only state, with Phi = dx+/dx and gamma = dx+/du accumulated over its sub-steps
  // (sim_jac_kernels.hpp): the outputs of `a` that are not null.  n_sub = 0 is the identity map
  void (*sim_jac)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, const cpmpc_sim_jac* a,
                  hipStream_t stream);
  void (*linearize_batch)(cpmpc_solver* s, int64_t B, const double* dyn_shared_host, const void* z, void* c, void* Phi,
                          void* Gamma, hipStream_t stream);
  // debug builds (-DCPMPC_FUSED_TIMING / -DCPMPC_FUSED_CLOCK): read and clear this unit's counters, ADDING them to out
  // (which = 0: eight phase counters, 1: {cycles, 100 MHz ticks, waves, max cycles}); -1 when not built in
  int (*debug_read)(int which, unsigned long long* out);
  // K = du / dx0 of the QP at z (in->z, or the handle's previous solution): linearisation into the workspace, then
  // feedback_gain_kernel (feedback_kernels.hpp); K [n_rows][NX][B], ok [B] nullable
  void (*feedback_gain)(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K, int32_t* ok,
                        hipStream_t stream);
  // u_out = clamp(u_nom + K0 . wrap(x - x_nom), +-u_limit), elementwise
  void (*feedback_apply)(int64_t B, const void* u_nom, const void* K0, const void* x_nom, const void* x, double u_limit,
                         void* u_out, hipStream_t stream);
  // K, k_sp = du / dset_point, k_up = du / du_prev of the QP at z, those that are not null (plan_sensitivity_kernels.hpp):
  // K [n_rows][NX][B], k_sp / k_up [n_rows][B], ok [B] nullable
  void (*plan_sensitivity)(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K, void* k_sp,
                           void* k_up, int32_t* ok, hipStream_t stream);
  // the first-order update of rows 0 .. n_rows-1 of the plan, elementwise (plan_update_kernel)
  void (*plan_update)(int64_t B, int n_rows, const cpmpc_plan_update* u, hipStream_t stream);
  // g_x0 = K^T gbar [NX][B], g_sp = k_sp^T gbar [B], g_up = k_up^T gbar [B] of the QP at z, those that are not null, for
  // the cotangent gbar [n_rows][B] (plan_vjp_kernels.hpp); ok [B] nullable.  Writes the linearisation scratch only
  void (*plan_vjp)(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, const void* gbar, void* g_x0,
                   void* g_sp, void* g_up, int32_t* ok, hipStream_t stream);
  // the gradients of gbar . (u + du) with respect to the cost weights, g_tw [NX][B], g_wu [B], g_wdu [B], and the primal QP
  // step du [n_rows][B] of the QP at z, those that are not null (plan_weight_vjp_kernels.hpp); ok [B] nullable.  Writes the
  // linearisation scratch and the rows of W and T only
  void (*plan_weight_vjp)(cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows, const void* gbar,
                          void* g_tw, void* g_wu, void* g_wdu, void* du, int32_t* ok, hipStream_t stream);
  // the plant step with per-problem parameters dyn [NP][B] (sim_kernel's PER_LANE instantiation)
  void (*sim_dyn)(int64_t B, const void* dyn, const double* fext_host, const void* fext, int n_sub, double h_last,
                  const void* u, void* state, hipStream_t stream);
  // the plant step with P = dx+/dp, or gp = P^T gbar, in groups of parameter columns (sim_param_kernels.hpp), and the
  // state / control cotangents gx, gu of sim_jac_kernel with shared or per-problem parameters: the outputs of `a` that are
  // not null
  void (*sim_param_jac)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, const cpmpc_sim_param_jac* a,
                        hipStream_t stream);
  // T ticks of the plant step in one launch, xs [T][NX][B] and / or x_final [NX][B] (sim_rollout_kernels.hpp), with shared
  // or per-problem parameters.  n_sub = 0 copies x0
  void (*sim_rollout)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T, const cpmpc_sim_rollout* a,
                      hipStream_t stream);
  // the adjoint of that rollout in one launch: g_x0, g_u [T][B], g_p of `a` that are not null (sim_rollout_vjp_kernel)
  void (*sim_rollout_vjp)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                          const cpmpc_sim_rollout_vjp* a, hipStream_t stream);
  // the forward mode of that rollout in the parameters and the Gauss-Newton normal equations of the window in one launch:
  // cost, g, H, S_final, x_final of `a` that are not null (sim_rollout_gn_kernels.hpp)
  void (*sim_rollout_gn)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                         const cpmpc_sim_rollout_gn* a, hipStream_t stream);
  // the forward mode of that rollout in the initial state and the normal equations of the fit of x0 in one launch: cost, g,
  // H, Phi_final, x_final of `a` that are not null (sim_rollout_gn_x0_kernels.hpp)
  void (*sim_rollout_gn_x0)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                            const cpmpc_sim_rollout_gn_x0* a, hipStream_t stream);
  // the extended Kalman filter over T ticks in one launch: x_final, P_final, xs, nis of `a` that are not null
  // (sim_ekf_kernels.hpp)
  void (*sim_ekf)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T, const cpmpc_sim_ekf* a,
                  hipStream_t stream);
  // the Rauch-Tung-Striebel smoother over T ticks in two launches: the filter's recording form into a->work, then the
  // backward pass over the record (sim_ekf_kernels.hpp: sim_ekf_record_kernel; sim_rts_kernels.hpp); the outputs of `a`
  // that are not null
  void (*sim_rts)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T, const cpmpc_sim_rts* a,
                  hipStream_t stream);
  // the backward Riccati recursion along a plant trajectory in one launch: K, P0 of `a` that are not null
  // (sim_track_kernels.hpp)
  void (*sim_lqr)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T, const cpmpc_sim_lqr* a,
                  hipStream_t stream);
  // T ticks of the plant under u_nom[t] + K[t] . wrap(x_t - x_nom_t), clamped, in one launch: xs, x_final, us of `a` that are
  // not null (sim_track_kernels.hpp)
  void (*sim_rollout_fb)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                         const cpmpc_sim_rollout_fb* a, hipStream_t stream);
  // one iLQR backward pass along a plant trajectory in one launch: K, kff, dV, P0, g0, hmax of `a` that are not null
  // (sim_ilqr_kernels.hpp)
  void (*sim_ilqr_backward)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                            const cpmpc_sim_ilqr_backward* a, hipStream_t stream);
  // T ticks of the plant under u_nom[t] + alpha kff[t] + K[t] . wrap(x_t - x_nom_t), clamped, with the cost summed, in one
  // launch: xs, x_final, us, cost of `a` that are not null (sim_ilqr_kernels.hpp)
  void (*sim_ilqr_forward)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                           const cpmpc_sim_ilqr_forward* a, hipStream_t stream);
  // the line search of one iLQR iteration in one launch, each problem halving its own step until its rolled cost passes the
  // Armijo test: xs, x_final, us, cost, alpha of `a` that are not null (sim_ilqr_kernels.hpp)
  void (*sim_ilqr_search)(int64_t B, const double* dyn_shared_host, int n_sub, double h_last, int T,
                          const cpmpc_sim_ilqr_search* a, hipStream_t stream);
};
// (functions, not namespace-scope tables: hipcc would emit a constant table for the device side as well)
CPMPC_HIDDEN const Engine* cpmpc_engine_f32_single();
CPMPC_HIDDEN const Engine* cpmpc_engine_f64_single();
CPMPC_HIDDEN const Engine* cpmpc_engine_f32_double();
CPMPC_HIDDEN const Engine* cpmpc_engine_f64_double();
static inline const Engine* engine_for(int dtype, int model) {
  if (model == CPMPC_MODEL_SINGLE) return dtype == CPMPC_F32 ? cpmpc_engine_f32_single() : cpmpc_engine_f64_single();
  return dtype == CPMPC_F32 ? cpmpc_engine_f32_double() : cpmpc_engine_f64_double();
}
static inline const Engine* engine_of(const cpmpc_solver* s) { return engine_for(s->dtype, s->model); }
