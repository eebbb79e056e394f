// cpmpc_api.hip -- C-ABI (include/cpmpc.h) over the gfx950 kernels.
//
// Host side of the batched cart-pole MPC hot path.  There is no CPU compute path in this library:
// every entry point that computes launches HIP kernels and fails with CPMPC_ERR_NO_DEVICE when no
// gfx950 device is usable.  The C-ABI is three translation units with no device code: this one (error text, defaults,
// devices, the handle's life cycle and options, profiling, the stage planner, the device-pointer step and warm start, the
// stand-alone pieces), cpmpc_host.hip (the host-pointer pipeline) and cpmpc_sharded.hip (several GPUs from one process);
// what they share is declared in api_internal.hpp.  The kernels of each (dtype, model) pair live in their own translation
// unit (engine_<dtype>_<model>.hip) and are reached through its `Engine` table (engine.hpp).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "api_internal.hpp"

// ------------------------------------------------------------------------------------------------
// error text
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int cpmpc_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char* cpmpc_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// defaults
// ------------------------------------------------------------------------------------------------
extern "C" void cpmpc_default_params(cpmpc_params* p) {  // optimization/optimization.hpp:12-48
  p->control_dt = 0.01;
  p->window_length = 40;
  p->state_spacing = 10;
  p->max_iterations = 8;
  p->relative_exit_tol = 1.0e-5;
  p->absolute_first_derivative_tol = 1.0e-6;
  p->equality_penalty_initial = 1.0;
  p->u_guess_sinusoid_amplitude = 10.0;
  p->u_cost_weight = 0.1;
  p->u_derivative_cost_weight = 0.1;
  p->b_x_final_cost_weight = 150.0;
  p->th_final_cost_weight = -1.0;
  p->b_x_dot_final_cost_weight = -1.0;
  p->th_dot_final_cost_weight = -1.0;
}

extern "C" void cpmpc_default_solver_opts(cpmpc_solver_opts* o) {
  o->max_line_search_iterations = 5;  // optimization.cc:76
  o->armijo_c1 = 1.0e-4;
  o->ls_shrink_max = 0.5;
  o->ls_shrink_min = 0.1;
  o->ls_alpha_growth = 2.0;
  o->penalty_rho = 0.1;
  o->lambda_initial = 0.0;
  o->lambda_failure_init = 1.0e-2;
  o->lambda_scale_up = 10.0;
  o->lambda_scale_down = 0.1;
  o->lambda_min = 1.0e-8;
  o->lambda_max = 1.0e6;
  o->b_x_limit = 5.0;  // optimization.cc:320
  o->u_limit = 300.0;  // optimization.cc:327
  o->ls_alpha_growth_backtracked = 2.0;
  o->full_step_below = 1.0e-4;
  o->exit_defect_floor = 2.0;
}

// ------------------------------------------------------------------------------------------------
// device discovery
// ------------------------------------------------------------------------------------------------
bool device_is_gfx950(int dev) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
  return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

extern "C" int cpmpc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; ++i)
    if (device_is_gfx950(i)) ++ok;
  return ok;
}

static int check_device(int dev) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(CPMPC_ERR_NO_DEVICE,
                "no HIP device visible; this library has no CPU fallback (libcpmpc needs a gfx950 GPU)");
  if (dev < 0 || dev >= n) return fail(CPMPC_ERR_NO_DEVICE, "device %d out of range (%d visible)", dev, n);
  if (!device_is_gfx950(dev))
    return fail(CPMPC_ERR_NO_DEVICE, "device %d is not gfx950; kernels are built for gfx950 only", dev);
  return CPMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// models
// ------------------------------------------------------------------------------------------------
static int model_nx(int model) { return model == CPMPC_MODEL_DOUBLE ? 6 : 4; }
static int model_np(int model) { return model == CPMPC_MODEL_DOUBLE ? 6 : 9; }
extern "C" int cpmpc_model_state_dim(int model) {
  return (model == CPMPC_MODEL_SINGLE || model == CPMPC_MODEL_DOUBLE) ? model_nx(model) : -1;
}
extern "C" int cpmpc_model_num_params(int model) {
  return (model == CPMPC_MODEL_SINGLE || model == CPMPC_MODEL_DOUBLE) ? model_np(model) : -1;
}

// ------------------------------------------------------------------------------------------------
// the handle
// ------------------------------------------------------------------------------------------------
// 2: a register-resident linearisation is compiled for this spacing; 1: served by the generic kernel
// (run-time spacing, O(spacing^2) workspace traffic per interval); 0: not a spacing
extern "C" int cpmpc_supported_state_spacing(int spacing) {
  if (spacing < 1) return 0;
  return linearize_specialised(spacing) ? 2 : 1;
}

static int validate_params(const cpmpc_params* p) {
  // the constructor's preconditions, optimization.cc:13-22
  if (!(p->control_dt > 0)) return fail(CPMPC_ERR_INVALID_ARG, "control_dt must be > 0 (optimization.cc:14)");
  if (!(p->window_length >= 1)) return fail(CPMPC_ERR_INVALID_ARG, "window_length must be >= 1 (optimization.cc:15)");
  if (p->state_spacing == 0 || p->window_length % p->state_spacing != 0)
    return fail(CPMPC_ERR_INVALID_ARG,
                "state_spacing (%llu) must divide into window_length (%llu) cleanly (optimization.cc:16-18)",
                (unsigned long long)p->state_spacing, (unsigned long long)p->window_length);
  if (!(p->max_iterations >= 1)) return fail(CPMPC_ERR_INVALID_ARG, "max_iterations must be >= 1 (optimization.cc:19)");
  if (!(p->u_cost_weight >= 0.0)) return fail(CPMPC_ERR_INVALID_ARG, "u_cost_weight must be >= 0 (optimization.cc:20)");
  if (!(p->u_derivative_cost_weight >= 0.0))
    return fail(CPMPC_ERR_INVALID_ARG, "u_derivative_cost_weight must be >= 0 (optimization.cc:21)");
  if (p->window_length > 4096) return fail(CPMPC_ERR_UNSUPPORTED, "window_length > 4096 is not supported");
  return CPMPC_OK;
}

// Horizon (window_length * control_dt, seconds) up to which the condensed QP is held to 1e-5 of a full-space KKT solve on
// every problem (include/cpmpc.h: cpmpc_max_parity_horizon)
static const double kMaxParityHorizon = 1.0;
// u_cost_weight below which the fp64 fused kernels refine the whole QP solution by default (half the reference's 0.1)
static const double kRefineBelowUCostWeight = 0.05;
extern "C" double cpmpc_max_parity_horizon(void) { return kMaxParityHorizon; }

static int create_impl(const cpmpc_params* params, const cpmpc_solver_opts* opts, size_t opts_size, int dtype,
                       int64_t max_batch, int device, int model, uint32_t flags, cpmpc_solver** out) {
  if (!params || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (dtype != CPMPC_F32 && dtype != CPMPC_F64) return fail(CPMPC_ERR_INVALID_ARG, "dtype must be CPMPC_F32 or CPMPC_F64");
  if (model != CPMPC_MODEL_SINGLE && model != CPMPC_MODEL_DOUBLE) return fail(CPMPC_ERR_INVALID_ARG, "unknown model");
  if (max_batch < 1 || max_batch > (1ll << 30)) return fail(CPMPC_ERR_INVALID_ARG, "max_batch must be in [1, 2^30]");
  int rc = validate_params(params);
  if (rc) return rc;
  if ((flags & ~(uint32_t)(CPMPC_CREATE_ALLOW_LONG_HORIZON | CPMPC_CREATE_REFINE_QP | CPMPC_CREATE_NO_REFINE_QP |
                           CPMPC_CREATE_STRICT_HORIZON | CPMPC_CREATE_WIDE_QP | CPMPC_CREATE_NO_WIDE_QP)) != 0)
    return fail(CPMPC_ERR_INVALID_ARG, "unknown creation flags 0x%x", flags);
  if ((flags & CPMPC_CREATE_REFINE_QP) && (flags & CPMPC_CREATE_NO_REFINE_QP))
    return fail(CPMPC_ERR_INVALID_ARG, "CPMPC_CREATE_REFINE_QP and CPMPC_CREATE_NO_REFINE_QP exclude each other");
  if ((flags & CPMPC_CREATE_WIDE_QP) && (flags & CPMPC_CREATE_NO_WIDE_QP))
    return fail(CPMPC_ERR_INVALID_ARG, "CPMPC_CREATE_WIDE_QP and CPMPC_CREATE_NO_WIDE_QP exclude each other");
  // the struct in some release: the leading int (padded to 8) and a whole number of doubles, from the shortest layout that is
  // a PREFIX of today's struct -- 13 doubles, through u_limit: 112 bytes -- to this one's.  (The 104-byte struct of the very
  // first commit had no ls_alpha_growth, which was inserted mid-struct before any release: read as today's prefix it would
  // shift every later field by one slot, so it is refused, like a size that splits a field: ADVICE r4, r5.)
  if (opts != nullptr && (opts_size < 112 || opts_size > sizeof(cpmpc_solver_opts) || opts_size % 8 != 0))
    return fail(CPMPC_ERR_INVALID_ARG, "opts_size %zu is not the size of any cpmpc_solver_opts this library knows (8 + 8 k "
                "bytes, 112 .. %zu)", opts_size, sizeof(cpmpc_solver_opts));
  {
    // Every horizon the reference's constructor accepts is accepted (optimization.cc:13-22: this is a drop-in); beyond
    // cpmpc_max_parity_horizon() the first handle of the process says so once, and CPMPC_CREATE_STRICT_HORIZON refuses.
    const double horizon = (double)params->window_length * params->control_dt;
    if (horizon > kMaxParityHorizon * (1.0 + 1e-9)) {
      if (flags & CPMPC_CREATE_STRICT_HORIZON)
        return fail(CPMPC_ERR_UNSUPPORTED,
                    "horizon window_length * control_dt = %.3f s exceeds %.1f s, the longest the condensed QP is held to 1e-5 of a "
                    "full-space solve on every problem (state elimination through an unstable plant loses ~3 digits per QP at "
                    "1.6 s; 2 of 16384 cold starts are beyond 1e-5 at 1.2 s), and CPMPC_CREATE_STRICT_HORIZON was given",
                    horizon, kMaxParityHorizon);
      static std::atomic<bool> warned{false};
      if (!(flags & CPMPC_CREATE_ALLOW_LONG_HORIZON) && !warned.exchange(true))
        fprintf(stderr,
                "cpmpc: horizon window_length * control_dt = %.3f s is beyond %.1f s (cpmpc_max_parity_horizon): solved as "
                "asked, but cold starts far from the optimum may differ from a full-space solve by more than 1e-5 on a "
                "few problems in 10^4 (include/cpmpc.h, CPMPC_CREATE_STRICT_HORIZON).  Said once per process.\n",
                horizon, kMaxParityHorizon);
    }
  }
  // defaults first, then as many leading bytes as the caller's struct has: a caller compiled against an earlier header
  // (a shorter struct: fields are only ever appended) keeps this library's defaults for the options it does not know
  cpmpc_solver_opts merged;
  cpmpc_default_solver_opts(&merged);
  if (opts) memcpy(&merged, opts, opts_size);
  if (!(merged.full_step_below >= 0.0) || !(merged.exit_defect_floor >= 0.0) || !std::isfinite(merged.full_step_below) ||
      !std::isfinite(merged.exit_defect_floor))   // the two thresholds that switch a rule off at 0 (NaN fails both tests)
    return fail(CPMPC_ERR_INVALID_ARG, "full_step_below and exit_defect_floor must be finite and >= 0 (0 disables the rule)");
  rc = check_device(device);
  if (rc) return rc;
  DeviceGuard guard(device);

  cpmpc_solver* s = new (std::nothrow) cpmpc_solver();
  if (!s) return fail(CPMPC_ERR_ALLOC, "out of host memory");
  s->params = *params;
  s->opts = merged;
  s->dtype = dtype;
  s->beyond_parity = (double)params->window_length * params->control_dt > kMaxParityHorizon * (1.0 + 1e-9);
  // default: refine where the control cost is weak (measured: include/cpmpc.h, CPMPC_CREATE_REFINE_QP) and, since round 6,
  // beyond the parity horizon: there AUTO takes the split pipeline with two passes of refinement with residuals from the
  // original data (refine_passes below), and the lanes on which the kernels (not the CPU check) are at fault go from 34 of
  // 8 192 to 1 at N = 160, as many as the CPU check (profiles/r06_long_horizon_probe_{8192,16384}.json)
  // and for the 6-state model where the pole angles are cost rows while their rates are equalities: there the condensed solve
  // of the first QP of a cold start is 7e-9 from an extended-precision solve where the CPU check's dense one is 2e-10 and the
  // refined one 7e-12, and four iterations carry that to 5e-5 on a lane on which the CPU check stays within 2e-8
  // (tests/test_gpu_double_parity.py, 40/8; include/cpmpc.h, CPMPC_CREATE_REFINE_QP)
  const bool angle_cost_rate_equality =
      model == CPMPC_MODEL_DOUBLE && params->th_final_cost_weight >= 0.0 && params->th_dot_final_cost_weight < 0.0;
  s->refine_qp = (flags & CPMPC_CREATE_REFINE_QP) != 0 ||
                 (!(flags & CPMPC_CREATE_NO_REFINE_QP) &&
                  (params->u_cost_weight < kRefineBelowUCostWeight || s->beyond_parity || angle_cost_rate_equality));
  // split pipeline: one pass; two beyond the parity horizon (tools/long_horizon_refine_study.py, first QP of 300 cold starts at
  // 1.6 s against a long-double solve: worst lane 3.5e-5 condensed, 1.6e-11 after one pass, 1.2e-13 after two -- the dense
  // pivoted LU of the CPU check: 1.1e-12; further passes change nothing)
  s->refine_passes = s->beyond_parity ? 2 : 1;
  if (const char* e = getenv("CPMPC_QP_REFINE_PASSES")) {   // diagnostic (tools/long_horizon_gpu_probe.py): passes of the split pipeline
    const int n = atoi(e);
    if (n >= 1 && n <= 16) s->refine_passes = n;
  }
  // default: on for the 6-state model (measured: include/cpmpc.h, CPMPC_CREATE_WIDE_QP), off for the 4-state one
  s->wide_qp = dtype == CPMPC_F32 && ((flags & CPMPC_CREATE_WIDE_QP) != 0 ||
                                      (!(flags & CPMPC_CREATE_NO_WIDE_QP) && model == CPMPC_MODEL_DOUBLE));
  s->model = model;
  s->device = device;
  s->esize = dtype == CPMPC_F32 ? 4 : 8;
  s->NX = model_nx(model);
  s->NP = model_np(model);
  s->N = (int)params->window_length;
  s->SP = (int)params->state_spacing;
  s->S = s->N / s->SP + 1;  // optimization.hpp:52
  s->dim = s->NX * s->S + s->N;  // optimization.cc:204-205
  s->cap = (max_batch + 63) / 64 * 64;

  // scalars of the dtype per problem; an NX-vector field occupies XW = 4 or 8 scalars
  const size_t XW = s->NX > 4 ? 8 : 4;
  const size_t n_xv = (size_t)2 * s->S + (size_t)s->NX * (s->S - 1) + s->N + (s->S - 1) + s->N;  // zx dzx Phi Gam cs Wk
  const size_t fields_real = XW * n_xv + 4 * (size_t)s->N + 2 * (size_t)s->N + SC_COUNT;
  const size_t bytes_real = fields_real * (size_t)s->cap * s->esize;
  const size_t bytes_int = (size_t)IS_COUNT * (size_t)s->cap * sizeof(int32_t);
  s->ws_bytes = bytes_real + bytes_int;
  hipError_t e = hipMalloc(&s->ws, s->ws_bytes);
  if (e != hipSuccess) {
    delete s;
    return fail(CPMPC_ERR_ALLOC, "hipMalloc of %zu bytes of workspace failed: %s", bytes_real + bytes_int,
                hipGetErrorString(e));
  }
  (void)hipMemset(s->ws, 0, s->ws_bytes);
  char* pch = (char*)s->ws;
  auto carve = [&](size_t nfields) {
    char* r = pch;
    pch += nfields * (size_t)s->cap * s->esize;
    return r;
  };
  // vector fields first so that every one of them is 16/32-byte aligned (cap is a multiple of 64)
  s->zx = carve(XW * s->S);
  s->dzx = carve(XW * s->S);
  s->Phi = carve(XW * s->NX * (s->S - 1));
  s->Gam = carve(XW * s->N);
  s->cs = carve(XW * (s->S - 1));
  s->Wk = carve(XW * s->N);
  s->Tk = carve(4 * s->N);
  s->zu = carve(s->N);
  s->dzu = carve(s->N);
  s->sc = carve(SC_COUNT);
  s->ist = (int32_t*)pch;

  // sinusoid cold-start table, evaluated on the host in double exactly as optimization.cc:63-67
  std::vector<double> tab(s->N);
  for (int k = 0; k < s->N; ++k)
    tab[k] = params->u_guess_sinusoid_amplitude *
             std::sin(static_cast<double>(k) / static_cast<double>(s->N) * 2 * M_PI);
  e = hipMalloc(&s->sin_table, (size_t)s->N * s->esize);
  if (e != hipSuccess) {
    (void)hipFree(s->ws);
    delete s;
    return fail(CPMPC_ERR_ALLOC, "hipMalloc failed: %s", hipGetErrorString(e));
  }
  if (dtype == CPMPC_F32) {
    std::vector<float> tf(tab.begin(), tab.end());
    e = hipMemcpy(s->sin_table, tf.data(), tf.size() * 4, hipMemcpyHostToDevice);
  } else {
    e = hipMemcpy(s->sin_table, tab.data(), tab.size() * 8, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)hipFree(s->ws);
    (void)hipFree(s->sin_table);
    delete s;
    return fail(CPMPC_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(e));
  }
  // index list of the staged fused pipeline (4 bytes per problem + three counters per host slot): allocated here, never in a step
  if (hipMalloc((void**)&s->active, ((size_t)s->cap + 3 * kHostSlots) * sizeof(int32_t)) != hipSuccess) {
    (void)hipGetLastError();
    s->active = nullptr;  // staging stays off for this handle (same results, single launch)
  }
  // histogram of iterations per problem, device -> host through mapped memory (the plan of the stages; optional as well)
  const size_t fb_bytes = (size_t)kHostSlots * kFbReporters * (kFbBins + 1) * sizeof(int32_t);
  if (s->active != nullptr &&
      hipHostMalloc((void**)&s->fb_host, fb_bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
      hipHostGetDevicePointer((void**)&s->fb_host_dev, s->fb_host, 0) == hipSuccess) {
    memset(s->fb_host, 0, fb_bytes);
  } else {
    (void)hipGetLastError();
    if (s->fb_host) (void)hipHostFree(s->fb_host);
    s->fb_host = s->fb_host_dev = nullptr;  // the fixed plan (2 iterations, then 1 at a time) for every step
  }
  *out = s;
  return CPMPC_OK;
}

extern "C" int cpmpc_create_model(const cpmpc_params* params, const cpmpc_solver_opts* opts, int dtype,
                                  int64_t max_batch, int device, int model, cpmpc_solver** out) {
  return create_impl(params, opts, CPMPC_SOLVER_OPTS_SIZE_POSITIONAL, dtype, max_batch, device, model, 0, out);
}

extern "C" int cpmpc_create(const cpmpc_params* params, const cpmpc_solver_opts* opts, int dtype,
                            int64_t max_batch, int device, cpmpc_solver** out) {
  return create_impl(params, opts, CPMPC_SOLVER_OPTS_SIZE_POSITIONAL, dtype, max_batch, device, CPMPC_MODEL_SINGLE, 0, out);
}

extern "C" int cpmpc_create_ex(const cpmpc_create_info* info, cpmpc_solver** out) {
  if (!info || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (info->struct_size != sizeof(cpmpc_create_info))
    return fail(CPMPC_ERR_INVALID_ARG, "cpmpc_create_info.struct_size is %u, this library's is %zu (set it to sizeof(cpmpc_create_info))",
                info->struct_size, sizeof(cpmpc_create_info));
  const size_t osz = info->opts_size ? (size_t)info->opts_size : sizeof(cpmpc_solver_opts);
  return create_impl(info->params, info->opts, osz, info->dtype, info->max_batch, info->device, info->model, info->flags, out);
}

extern "C" void cpmpc_destroy(cpmpc_solver* s) {
  if (!s) return;
  DeviceGuard guard(s->device);
  for (auto& sp : s->spans) {
    (void)hipEventDestroy(sp.start);
    (void)hipEventDestroy(sp.stop);
  }
  for (auto& sp : s->free_spans) {
    (void)hipEventDestroy(sp.start);
    (void)hipEventDestroy(sp.stop);
  }
  if (s->ws) (void)hipFree(s->ws);
  if (s->sin_table) (void)hipFree(s->sin_table);
  for (HostSlot& sl : s->slot) {
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.pin) (void)hipHostFree(sl.pin);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.stream) (void)hipStreamDestroy(sl.stream);
  }
  if (s->ev_last) (void)hipEventDestroy(s->ev_last);
  if (s->active) (void)hipFree(s->active);
  if (s->fb_host) (void)hipHostFree(s->fb_host);
  delete s;
}

extern "C" int cpmpc_dim(const cpmpc_solver* s) { return s ? s->dim : -1; }
extern "C" int cpmpc_num_states(const cpmpc_solver* s) { return s ? s->S : -1; }
extern "C" int cpmpc_dtype(const cpmpc_solver* s) { return s ? s->dtype : -1; }
extern "C" int cpmpc_model(const cpmpc_solver* s) { return s ? s->model : -1; }
extern "C" int cpmpc_refines_qp(const cpmpc_solver* s) { return s ? (s->refine_qp && s->dtype == CPMPC_F64 ? 1 : 0) : -1; }
// what a handle actually uses: defaults merged with as much of the caller's struct as its constructor read (the
// positional constructors read 128 bytes, so a later field -- exit_defect_floor -- set through them is NOT taken)
extern "C" int cpmpc_get_solver_opts(const cpmpc_solver* s, cpmpc_solver_opts* out, size_t out_size) {
  if (!s || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (out_size < 112 || out_size > sizeof(cpmpc_solver_opts) || out_size % 8 != 0)
    return fail(CPMPC_ERR_INVALID_ARG, "out_size %zu is not the size of any cpmpc_solver_opts this library knows", out_size);
  memcpy(out, &s->opts, out_size);
  return CPMPC_OK;
}
extern "C" int cpmpc_horizon_beyond_parity(const cpmpc_solver* s) { return s ? (s->beyond_parity ? 1 : 0) : -1; }
extern "C" int cpmpc_wide_qp(const cpmpc_solver* s) {
  return s ? (s->wide_qp ? 1 : 0) : -1;  // either pipeline since round 6 (qp_ls_kernel<R, M, true>)
}
extern "C" int cpmpc_has_previous_solution(const cpmpc_solver* s) { return (s && s->prev_B > 0) ? 1 : 0; }
extern "C" int64_t cpmpc_previous_solution_batch(const cpmpc_solver* s) { return s ? s->prev_B : 0; }

extern "C" int cpmpc_reset(cpmpc_solver* s) {  // Optimization::Reset, optimization.hpp:83
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null solver");
  s->prev_B = 0;
  return CPMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// profiling spans
// ------------------------------------------------------------------------------------------------
static const char* kKernelNames[CPMPC_KERNEL_COUNT] = {"prepare_kernel", "linearize_kernel", "qp_ls_kernel",
                                                       "finalize_kernel", "fused_sqp_kernel"};
extern "C" const char* cpmpc_kernel_name(int kernel) {
  return (kernel >= 0 && kernel < CPMPC_KERNEL_COUNT) ? kKernelNames[kernel] : "?";
}

void span_begin(cpmpc_solver* s, int kernel, hipStream_t stream, ProfSpan* cur) {
  if (!s->profiling) return;
  if (!s->free_spans.empty()) {
    *cur = s->free_spans.back();
    s->free_spans.pop_back();
  } else {
    (void)hipEventCreate(&cur->start);
    (void)hipEventCreate(&cur->stop);
  }
  cur->kernel = kernel;
  (void)hipEventRecord(cur->start, stream);
}
void span_end(cpmpc_solver* s, hipStream_t stream, ProfSpan* cur) {
  if (!s->profiling) return;
  (void)hipEventRecord(cur->stop, stream);
  s->spans.push_back(*cur);
}

static void collect_spans(cpmpc_solver* s) {
  for (auto& sp : s->spans) {
    float ms = 0.f;
    if (hipEventSynchronize(sp.stop) == hipSuccess && hipEventElapsedTime(&ms, sp.start, sp.stop) == hipSuccess) {
      s->prof_ms[sp.kernel] += ms;
      s->prof_n[sp.kernel] += 1;
    }
    s->free_spans.push_back(sp);
  }
  s->spans.clear();
}

extern "C" int cpmpc_profile_enable(cpmpc_solver* s, int on) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null solver");
  s->profiling = on ? 1 : 0;
  return CPMPC_OK;
}
extern "C" int cpmpc_profile_reset(cpmpc_solver* s) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null solver");
  DeviceGuard guard(s->device);
  collect_spans(s);
  for (int i = 0; i < CPMPC_KERNEL_COUNT; ++i) {
    s->prof_ms[i] = 0;
    s->prof_n[i] = 0;
  }
  return CPMPC_OK;
}
extern "C" int cpmpc_profile_read(cpmpc_solver* s, int kernel, double* total_ms, int64_t* launches) {
  if (!s || kernel < 0 || kernel >= CPMPC_KERNEL_COUNT) return fail(CPMPC_ERR_INVALID_ARG, "bad argument");
  DeviceGuard guard(s->device);
  collect_spans(s);
  if (total_ms) *total_ms = s->prof_ms[kernel];
  if (launches) *launches = s->prof_n[kernel];
  return CPMPC_OK;
}

// Host-pointer entry points run on the handle's own stream.  Once one has been used, every device-pointer call on a
// caller's stream leaves an event behind so that the next host-pointer call is ordered after it.
static void track_caller_stream(cpmpc_solver* s, hipStream_t stream) {
  bool own = false;
  for (const HostSlot& sl : s->slot) own = own || (sl.stream != nullptr && stream == sl.stream);
  if (s->ev_last != nullptr && !own) {
    (void)hipEventRecord(s->ev_last, stream);
    s->ev_pending = true;
  }
}

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
extern "C" int cpmpc_set_pipeline(cpmpc_solver* s, int mode) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null solver");
  if (mode != CPMPC_PIPELINE_AUTO && mode != CPMPC_PIPELINE_SPLIT && mode != CPMPC_PIPELINE_FUSED)
    return fail(CPMPC_ERR_INVALID_ARG, "unknown pipeline mode");
  if (mode == CPMPC_PIPELINE_FUSED && !fused_built(s))
    return fail(CPMPC_ERR_UNSUPPORTED, "the fused pipeline is not built for model %d with S-1 = %d, state_spacing = %d",
                s->model, s->S - 1, s->SP);
  s->pipeline = mode;
  return CPMPC_OK;
}
extern "C" int cpmpc_set_compaction(cpmpc_solver* s, int first_iterations, int next_iterations) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null solver");
  if (first_iterations < 0 || next_iterations < 0) return fail(CPMPC_ERR_INVALID_ARG, "iteration counts must be >= 0");
  s->stage_first = first_iterations;
  s->stage_next = next_iterations;
  s->stage_auto = false;  // an explicit setting applies to every batch size
  return CPMPC_OK;
}
// ---- the stages of the fused pipeline for one step ---------------------------------------------------------------------
// The kernel runs bounds[i+1] - bounds[i] iterations per launch; between launches the problems still iterating are
// compacted into dense waves (engine_impl.hpp: step_batch_impl).  Where to cut is a question of speed only.
//  * exits disabled, or a batch of at most one round of resident waves: one launch;
//  * an explicit cpmpc_set_compaction(first, next): first, then next at a time;
//  * default: from the histogram of iterations per problem of the most recent step whose finalize_kernel has finished
//    (host-mapped memory, read without synchronisation; a step queued but not finished simply does not count yet), by
//    dynamic programming over the cuts with this cost model, in units of one wave's time for one iteration:
//      - a stage from iteration a to b runs surv(a) / ppw waves (surv(j) = problems that need more than j iterations);
//        a wave lasts until the slowest of its ppw problems stops: sum over j of 1 - (1 - surv(a+j) / surv(a))^ppw;
//      - the stage takes max(wave-iterations / resident waves, its longest wave) + one launch and compaction (7 us);
//      - a stage with at most one round of resident waves left runs to the end (the kernel's own rule);
//    a plan that comes out as ONE launch although the histogram says nearly everybody (99.9 %) stops early gets one cut
//    where they do: in a settled closed loop (everybody stops after the first iteration) that is a second, empty launch
//    per tick (7 us), and it is what keeps a tick in which some controllers are disturbed from being bound by waves
//    that one disturbed problem in sixteen keeps alive.  Before the first histogram, and when the only histogram there is
//    is old and the counts are moving (see below): 2 iterations, then 1 at a time.
// the plan from a histogram (hist[b] = problems that ran b iterations, the last bin collecting every larger count):
// bounds[0] = 0 < ... < bounds[n] = T, returns n.  resident = waves of the fused kernel the machine holds (1 / 2 per SIMD)
static int plan_from_histogram(const double* hist, double n_hist, int64_t B, int T, int ppw, double resident, int window,
                               int* bounds) {
  // surv[j]: expected problems of THIS batch needing more than j iterations, j = 0 .. T
  double surv[kMaxStages + 1];
  const double scale = (double)B / n_hist;
  for (int j = 0; j <= T; ++j) {
    double above = 0.0;
    for (int b = j + 1; b < kFbBins; ++b) above += hist[b];
    surv[j] = j < T ? above * scale : 0.0;
  }
  surv[0] = (double)B;
  const double launch = 0.14 * 40.0 / (double)window;        // 7 us in units of one wave-iteration (50 us at N = 40)
  const double run_out = 2048.0 * (double)ppw;                // the kernel's run_out_below
  double best[kMaxStages + 2];
  int next_cut[kMaxStages + 2];
  best[T] = 0.0;
  for (int a = T - 1; a >= 0; --a) {
    best[a] = 1e300;
    next_cut[a] = T;
    // a stage that starts at a, by the iteration b it ends at (ascending, the sums carried along)
    double wave_iters = 0.0, longest = 0.0;
    for (int b = a + 1; b <= T; ++b) {
      const int j = b - 1 - a;
      const double q = surv[a] > 0.0 ? surv[a + j] / surv[a] : 0.0;
      wave_iters += 1.0 - std::pow(1.0 - (q > 1.0 ? 1.0 : q), (double)ppw);
      if (surv[a + j] >= 1.0) longest = (double)(j + 1);
      if (a > 0 && surv[a] <= run_out && b != T) continue;   // such a stage runs to the end by itself
      const double thr = wave_iters * surv[a] / (double)ppw / resident;
      const double cost = (thr > longest ? thr : longest) + launch + (b < T ? best[b] : 0.0);
      if (cost < best[a] - 1e-12 || (b == T && cost <= best[a] + 1e-12)) {   // ties: the fewer launches
        best[a] = cost;
        next_cut[a] = b;
      }
    }
  }
  int n = 0;
  bounds[0] = 0;
  for (int a = 0; a < T && n < kMaxStages; a = next_cut[a]) bounds[++n] = next_cut[a];
  bounds[n] = T;
  if (n == 1) {  // the insurance cut (see above)
    for (int j = 1; j < T; ++j)
      if (surv[j] <= 0.001 * (double)B) {
        bounds[1] = j;
        bounds[2] = T;
        n = 2;
        break;
      }
  }
  return n;
}

// the planner alone, for tests and tools (no device, no handle): hist[16] as finalize_kernel reports it
extern "C" int cpmpc_plan_stages_from_histogram(const int64_t* hist, int64_t B, int max_iterations, int intervals, int dtype,
                                                int window_length, int32_t* bounds, int capacity) {
  // (max_iterations <= kFbBins - 1: with more, the last bin -- "this many or more" -- would stand for problems that
  // stopped early as well as for those that ran to the cap, and surv[] could not tell them apart)
  if (!hist || !bounds || B < 1 || max_iterations < 1 || max_iterations > kFbBins - 1 || intervals < 1 || intervals > 64 ||
      window_length < 1 || capacity < max_iterations + 1 || (dtype != CPMPC_F32 && dtype != CPMPC_F64))
    return -1;
  double h[kFbBins], n_hist = 0.0;
  for (int b = 0; b < kFbBins; ++b) {
    if (hist[b] < 0) return -1;
    h[b] = (double)hist[b];
    n_hist += h[b];
  }
  if (n_hist <= 0.0) return -1;
  int bnd[kMaxStages + 1];
  const int n = plan_from_histogram(h, n_hist, B, max_iterations, 64 / intervals, dtype == CPMPC_F64 ? 1024.0 : 2048.0,
                                    window_length, bnd);
  for (int i = 0; i <= n; ++i) bounds[i] = bnd[i];
  return n;
}

int cpmpc_plan_stages(cpmpc_solver* s, int slot, int64_t B, bool exits, int* bounds) {
  const int T = (int)s->params.max_iterations;
  const int L = s->S - 1, ppw = 64 / L;
  auto finish = [&](int n) {
    s->last_plan_n = n;
    for (int i = 0; i <= n; ++i) s->last_plan[i] = bounds[i];
    return n;
  };
  bounds[0] = 0;
  bounds[1] = T;
  if (!exits || s->active == nullptr || T < 2) return finish(1);
  auto fixed = [&](int first, int next) {  // `first` iterations, then `next` at a time (the last launch takes what is left)
    if (first <= 0 || next <= 0 || T <= first) return finish(1);
    int n = 1;
    bounds[1] = first;
    while (bounds[n] < T && n < kMaxStages) {
      bounds[n + 1] = bounds[n] + next < T ? bounds[n] + next : T;
      ++n;
    }
    bounds[n] = T;
    return finish(n);
  };
  if (!s->stage_auto) return fixed(s->stage_first, s->stage_next);
  // default: only batches beyond one round of resident waves (2 per SIMD) are staged at all -- a smaller one ends with
  // its slowest wave either way
  if ((B * (int64_t)L + 63) / 64 <= 2048) return finish(1);
  if (s->fb_host == nullptr || T > kFbBins - 1) return fixed(s->stage_first, s->stage_next);  // (the last bin must mean "the cap")
  // the counts of the reporting workgroups that carry the same step's stamp as the first one (a step still running has
  // stamped only some: they wait for a later plan)
  const int32_t* fb = s->fb_host + (size_t)slot * kFbReporters * (kFbBins + 1);
  // Relaxed loads on purpose: the kernel publishes with relaxed system-scope stores (a release there writes the L2 back,
  // 29 -> 94 us of finalize), so no ordering is promised and none is pretended here.  A reporter's stamp is read before
  // AND after its counts; a block whose stamp moved in between (the next step's finalize is writing it) is left out, like
  // one that has not been written yet.  What can still slip through is a block whose counts belong to a newer step than
  // its stamp: a hint that is one step off costs speed, never results -- the plan decides only where the launches are cut.
  const int seq = __atomic_load_n(&fb[kFbBins], __ATOMIC_RELAXED);
  double hist[kFbBins], n_hist = 0.0;
  for (int b = 0; b < kFbBins; ++b) hist[b] = 0.0;
  for (int r = 0; seq != 0 && r < s->fb_reporters[slot]; ++r) {
    const int32_t* rep = fb + (size_t)r * (kFbBins + 1);
    if (__atomic_load_n(&rep[kFbBins], __ATOMIC_RELAXED) != seq) continue;
    double c[kFbBins];
    for (int b = 0; b < kFbBins; ++b) c[b] = (double)__atomic_load_n(&rep[b], __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_ACQUIRE);  // (host-side only: keeps the compiler and the CPU from hoisting the re-read)
    if (__atomic_load_n(&rep[kFbBins], __ATOMIC_RELAXED) != seq) continue;
    for (int b = 0; b < kFbBins; ++b) {
      hist[b] += c[b];
      n_hist += c[b];
    }
  }
  if (seq == 0 || n_hist <= 0.0) return fixed(s->stage_first, s->stage_next);  // nothing to plan from yet
  // How old may the histogram be?  A caller that synchronises every tick (a controller acting on u) plans from the tick
  // before.  One that queues ticks ahead plans from whatever has finished, many ticks back: right while the iteration
  // counts hold still, wrong in a transient (a swing-up queued ahead ran 2.0 -> 2.7 ms per tick on plans made for ticks
  // long gone).  So: a histogram at most two steps old is used as it is; an older one only if it agrees with the one seen
  // before it (no bin's share moved by more than 2 % of the batch); otherwise the fixed pattern.
  PlanCache& pc = s->plan_cache[slot];
  if (pc.seen_seq != seq) {
    double moved = 0.0;
    for (int b = 0; b < kFbBins; ++b) {
      const double share = hist[b] / n_hist, d = share - pc.seen[b];
      moved = (d < 0.0 ? -d : d) > moved ? (d < 0.0 ? -d : d) : moved;
      pc.seen[b] = share;
    }
    pc.stationary = pc.have_prev && moved <= 0.02;
    pc.have_prev = true;
    pc.seen_seq = seq;
  }
  const int age = s->fb_seq[slot] >= seq ? s->fb_seq[slot] - seq : s->fb_seq[slot] + (1 << 30) - seq;  // steps launched since
  const bool fresh = age <= 2;
  if (!fresh && !pc.stationary) return fixed(s->stage_first, s->stage_next);
  // the same histogram and batch as the last plan made on this slot: the same plan
  if (pc.seq == seq && pc.B == B && pc.n_hist == n_hist && pc.n > 0) {
    for (int i = 0; i <= pc.n; ++i) bounds[i] = pc.bounds[i];
    return finish(pc.n);
  }
  const int n = plan_from_histogram(hist, n_hist, B, T, ppw, s->esize == 8 ? 1024.0 : 2048.0, s->N, bounds);
  pc.seq = seq;
  pc.B = B;
  pc.n_hist = n_hist;
  pc.n = n;
  for (int i = 0; i <= n; ++i) pc.bounds[i] = bounds[i];
  return finish(n);
}

extern "C" int cpmpc_get_stage_plan(const cpmpc_solver* s, int32_t* bounds, int capacity) {
  if (!s || !bounds || capacity < 2) return -1;
  const int n = s->last_plan_n < capacity - 1 ? s->last_plan_n : capacity - 1;
  for (int i = 0; i <= n; ++i) bounds[i] = s->last_plan[i];
  return n;
}

extern "C" int cpmpc_get_pipeline(const cpmpc_solver* s) {
  if (!s) return -1;
  return use_fused(s) ? CPMPC_PIPELINE_FUSED : CPMPC_PIPELINE_SPLIT;
}
extern "C" int cpmpc_step_batch(cpmpc_solver* s, int64_t B, const cpmpc_step_inputs* in,
                                const cpmpc_step_outputs* out, void* stream) {
  if (!s || !in) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  if (B > s->cap) return fail(CPMPC_ERR_BATCH, "B=%lld exceeds the capacity %lld given to cpmpc_create", (long long)B, (long long)s->cap);
  if (!in->x0) return fail(CPMPC_ERR_INVALID_ARG, "x0 is required");
  if ((in->dyn_shared_host == nullptr) == (in->dyn == nullptr))
    return fail(CPMPC_ERR_INVALID_ARG, "exactly one of dyn_shared_host / dyn must be given");
  if (!in->set_point && !std::isfinite(in->set_point_shared))
    return fail(CPMPC_ERR_INVALID_ARG, "set_point_shared must be finite");
  DeviceGuard guard(s->device);
  int rc = CPMPC_OK;
  rc = engine_of(s)->step_batch(s, B, in, out, (hipStream_t)stream, 0, 0);
  track_caller_stream(s, (hipStream_t)stream);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// warm-start state
// ------------------------------------------------------------------------------------------------
extern "C" int cpmpc_set_previous_solution(cpmpc_solver* s, int64_t B, const void* z, void* stream) {
  if (!s || !z) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (B < 1 || B > s->cap) return fail(CPMPC_ERR_BATCH, "B out of range");
  DeviceGuard guard(s->device);
  // packed [dim][B] (MapKey order) -> workspace layout
  engine_of(s)->pack_z(s, B, z, (hipStream_t)stream);  // packed [dim][B] (MapKey order) -> workspace layout
  HIP_TRY(hipGetLastError());
  if (B > s->prev_B) s->prev_B = B;
  track_caller_stream(s, (hipStream_t)stream);
  return CPMPC_OK;
}

extern "C" int cpmpc_get_solution(cpmpc_solver* s, int64_t B, void* z_out, void* stream) {
  if (!s || !z_out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (B < 1 || B > s->cap) return fail(CPMPC_ERR_BATCH, "B out of range");
  DeviceGuard guard(s->device);
  engine_of(s)->unpack_z(s, B, z_out, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  // this read of zx/zu on the caller's stream must finish before a later host-pointer call (on the handle's own
  // stream) overwrites them
  track_caller_stream(s, (hipStream_t)stream);
  return CPMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// stand-alone pieces
// ------------------------------------------------------------------------------------------------
int current_device_ok() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess)
    return fail(CPMPC_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
  return check_device(dev);
}

static int check_model_dtype_batch(int model, int dtype, int64_t B) {
  if (model != CPMPC_MODEL_SINGLE && model != CPMPC_MODEL_DOUBLE) return fail(CPMPC_ERR_INVALID_ARG, "unknown model");
  if (dtype != CPMPC_F32 && dtype != CPMPC_F64) return fail(CPMPC_ERR_INVALID_ARG, "bad dtype");
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  return CPMPC_OK;
}

static int check_piece_args(int model, int dtype, int64_t B) {
  int rc = check_model_dtype_batch(model, dtype, B);
  return rc ? rc : current_device_ok();
}

extern "C" int cpmpc_dynamics_batch_model(int model, int dtype, int64_t B, const double* dyn_shared_host,
                                          const void* x, const void* u, const double* fext_host, void* f, void* Jx,
                                          void* Ju, void* stream) {
  if (!dyn_shared_host || !x || !u || !f) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = check_piece_args(model, dtype, B);
  if (rc) return rc;
  engine_for(dtype, model)->dynamics(B, dyn_shared_host, fext_host, x, u, f, Jx, Ju, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return CPMPC_OK;
}
extern "C" int cpmpc_dynamics_batch(int dtype, int64_t B, const double* dyn_shared_host, const void* x,
                                    const void* u, const double* fext_host, void* f, void* Jx, void* Ju,
                                    void* stream) {
  return cpmpc_dynamics_batch_model(CPMPC_MODEL_SINGLE, dtype, B, dyn_shared_host, x, u, fext_host, f, Jx, Ju, stream);
}

extern "C" int cpmpc_rk4_batch_model(int model, int dtype, int64_t B, const double* dyn_shared_host, const void* x,
                                     const void* u, double h, const double* fext_host, void* x_new, void* A,
                                     void* Bm, void* stream) {
  if (!dyn_shared_host || !x || !u || !x_new) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = check_piece_args(model, dtype, B);
  if (rc) return rc;
  engine_for(dtype, model)->rk4(B, dyn_shared_host, fext_host, h, x, u, x_new, A, Bm, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return CPMPC_OK;
}
extern "C" int cpmpc_rk4_batch(int dtype, int64_t B, const double* dyn_shared_host, const void* x, const void* u,
                               double h, const double* fext_host, void* x_new, void* A, void* Bm, void* stream) {
  return cpmpc_rk4_batch_model(CPMPC_MODEL_SINGLE, dtype, B, dyn_shared_host, x, u, h, fext_host, x_new, A, Bm,
                               stream);
}

extern "C" int cpmpc_linearize_batch(cpmpc_solver* s, int64_t B, const double* dyn_shared_host, const void* z,
                                     void* c, void* Phi, void* Gamma, void* stream) {
  if (!s || !dyn_shared_host || !z || !c || !Phi || !Gamma) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  if (B > s->cap) return fail(CPMPC_ERR_BATCH, "B exceeds capacity");
  DeviceGuard guard(s->device);
  // the caller's z is packed into the step buffers (dzx/dzu), which hold no state between calls, so the
  // warm start (zx/zu) is untouched; the linearisation lands in the workspace and is unpacked
  engine_of(s)->linearize_batch(s, B, dyn_shared_host, z, c, Phi, Gamma, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  track_caller_stream(s, (hipStream_t)stream);  // the step buffers of the workspace were used on the caller's stream
  return CPMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// the plant calls: one step, the step with its derivatives, the rollout and its adjoint.  Each has its own argument rules;
// what they check alike and how they end is below.
// ------------------------------------------------------------------------------------------------
// simulator.cc:18-22 evaluated in double: the number of sub-steps of a plant step of length dt and the size of the last one
// (n_sub = 0 for dt = 0).  Shared by every plant call, so all take the same sub-steps.
static int sim_sub_steps(double dt, int* n_sub_out, double* h_last_out) {
  const double internal_dt = 0.001;
  int n_sub = 0;
  double h_last = internal_dt;
  double rem = dt;
  while (rem > 0.0) {
    h_last = rem < internal_dt ? rem : internal_dt;
    ++n_sub;
    rem -= internal_dt;
    if (n_sub > 100000000) return fail(CPMPC_ERR_INVALID_ARG, "dt too large");
  }
  *n_sub_out = n_sub;
  *h_last_out = h_last;
  return CPMPC_OK;
}

// The checks every plant call makes (no device needed).  Two functions, not one, because the calls with an argument struct
// test their own rules between the two, and the order of the tests is part of what a caller sees.
static int check_plant_dt(double dt) {
  if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(CPMPC_ERR_INVALID_ARG, "dt must be finite and >= 0 (simulator.cc:13)");
  return CPMPC_OK;
}
// ... and check_model_dtype_batch above.  `what` names the argument struct:
static int check_struct_size(const char* what, uint64_t struct_size, size_t size_here) {
  if (struct_size != size_here)
    return fail(CPMPC_ERR_INVALID_ARG, "%s.struct_size is %llu, this library's is %zu (set it to sizeof(%s))", what,
                (unsigned long long)struct_size, size_here, what);
  return CPMPC_OK;
}

struct ArraySpan {
  const void* p;  // NULL: not given, overlaps nothing
  size_t rows;    // of B numbers each
  const char* name;
};
// Lanes run in any order, and a lane reads its inputs before it writes but another lane's may not have been read yet: an
// output that overlaps an array the call only reads is refused.  `row` is the size of B numbers in bytes.
template <int N_OUT, int N_IN>
static int check_no_overlap(const ArraySpan (&outs)[N_OUT], const ArraySpan (&ins)[N_IN], size_t row) {
  for (const ArraySpan& o : outs)
    for (const ArraySpan& in : ins) {
      if (!o.p || !in.p) continue;
      const char *o0 = (const char*)o.p, *i0 = (const char*)in.p;
      if (o0 < i0 + in.rows * row && i0 < o0 + o.rows * row)
        return fail(CPMPC_ERR_INVALID_ARG, "%s overlaps %s, which the call only reads (give another array)", o.name, in.name);
    }
  return CPMPC_OK;
}
static size_t row_bytes(int dtype, int64_t B) { return (size_t)B * (dtype == CPMPC_F64 ? 8 : 4); }

// How every plant call ends once its arguments are accepted: the device, the sub-steps of dt, the engine call as
// launch(n_sub, h_last).  skip_empty: the call has nothing to write for dt = 0 and launches nothing then.
template <typename Launch>
static int run_plant_call(double dt, bool skip_empty, Launch launch) {
  int rc = current_device_ok();
  if (rc) return rc;
  int n_sub = 0;
  double h_last = 0.0;
  rc = sim_sub_steps(dt, &n_sub, &h_last);
  if (rc) return rc;
  if (skip_empty && n_sub == 0) return CPMPC_OK;
  launch(n_sub, h_last);
  HIP_TRY(hipGetLastError());
  return CPMPC_OK;
}

extern "C" int cpmpc_sim_step_batch_model(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                                          const void* u, const double* fext_host, const void* fext, void* state,
                                          void* stream) {
  if (!dyn_shared_host || !u || !state) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = check_plant_dt(dt);
  if (rc) return rc;
  rc = check_model_dtype_batch(model, dtype, B);
  if (rc) return rc;
  return run_plant_call(dt, true, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim(B, dyn_shared_host, fext_host, fext, n_sub, h_last, u, state, (hipStream_t)stream);
  });
}
extern "C" int cpmpc_sim_step_batch(int dtype, int64_t B, const double* dyn_shared_host, double dt, const void* u,
                                    const double* fext_host, const void* fext, void* state, void* stream) {
  return cpmpc_sim_step_batch_model(CPMPC_MODEL_SINGLE, dtype, B, dyn_shared_host, dt, u, fext_host, fext, state,
                                    stream);
}

// The argument checks of cpmpc_sim_step_jac_batch (no device needed)
static int check_sim_jac_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, const cpmpc_sim_jac* a) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (cpmpc_sim_jac)");
  int rc = check_struct_size("cpmpc_sim_jac", a->struct_size, sizeof(cpmpc_sim_jac));
  if (rc) return rc;
  if (!dyn_shared_host || !a->state || !a->u) return fail(CPMPC_ERR_INVALID_ARG, "null argument (dyn, state, u)");
  rc = check_plant_dt(dt);
  if (rc) return rc;
  if ((a->gx || a->gu) && !a->gbar) return fail(CPMPC_ERR_INVALID_ARG, "gx / gu are given without gbar");
  if (a->gbar && !a->gx && !a->gu) return fail(CPMPC_ERR_INVALID_ARG, "gbar is given with neither gx nor gu");
  if (!a->x_new && !a->A && !a->Bu && !a->gx && !a->gu) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  rc = check_model_dtype_batch(model, dtype, B);
  if (rc) return rc;
  const size_t nx = (size_t)model_nx(model);
  const ArraySpan outs[3] = {{a->x_new, nx, "x_new"}, {a->gx, nx, "gx"}, {a->A, nx * nx, "A"}};
  const ArraySpan ins[2] = {{a->state, nx, "state"}, {a->gbar, nx, "gbar"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

// Simulator::Step with A = dx+/dx and Bu = dx+/du, or their products with a cotangent (sim_jac_kernels.hpp)
extern "C" int cpmpc_sim_step_jac_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                                        const cpmpc_sim_jac* a, void* stream) {
  int rc = check_sim_jac_args(model, dtype, B, dyn_shared_host, dt, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_jac(B, dyn_shared_host, n_sub, h_last, a, (hipStream_t)stream);
  });
}

// The plant step with per-problem parameters: dyn == NULL is cpmpc_sim_step_batch_model itself
extern "C" int cpmpc_sim_step_dyn_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, const void* dyn,
                                        double dt, const void* u, const double* fext_host, const void* fext, void* state,
                                        void* stream) {
  if (!dyn) return cpmpc_sim_step_batch_model(model, dtype, B, dyn_shared_host, dt, u, fext_host, fext, state, stream);
  if (!u || !state) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = check_plant_dt(dt);
  if (rc) return rc;
  rc = check_model_dtype_batch(model, dtype, B);
  if (rc) return rc;
  // the kernel updates the state in place while other lanes still read their parameters
  const ArraySpan outs[1] = {{state, (size_t)model_nx(model), "state"}};
  const ArraySpan ins[1] = {{dyn, (size_t)model_np(model), "dyn"}};
  rc = check_no_overlap(outs, ins, row_bytes(dtype, B));
  if (rc) return rc;
  return run_plant_call(dt, true, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_dyn(B, dyn, fext_host, fext, n_sub, h_last, u, state, (hipStream_t)stream);
  });
}

// The argument checks of cpmpc_sim_step_param_jac_batch (no device needed)
static int check_sim_param_jac_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                                    const cpmpc_sim_param_jac* a) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (cpmpc_sim_param_jac)");
  int rc = check_struct_size("cpmpc_sim_param_jac", a->struct_size, sizeof(cpmpc_sim_param_jac));
  if (rc) return rc;
  if (!a->state || !a->u) return fail(CPMPC_ERR_INVALID_ARG, "null argument (state, u)");
  if (!dyn_shared_host && !a->dyn) return fail(CPMPC_ERR_INVALID_ARG, "null argument (neither dyn_shared_host nor dyn is given)");
  rc = check_plant_dt(dt);
  if (rc) return rc;
  if ((a->gp || a->gx || a->gu) && !a->gbar) return fail(CPMPC_ERR_INVALID_ARG, "gp / gx / gu are given without gbar");
  if (a->gbar && !a->gp && !a->gx && !a->gu) return fail(CPMPC_ERR_INVALID_ARG, "gbar is given with none of gp, gx, gu");
  if (!a->x_new && !a->P && !a->gp && !a->gx && !a->gu) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  rc = check_model_dtype_batch(model, dtype, B);
  if (rc) return rc;
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model);
  const ArraySpan outs[5] = {{a->x_new, nx, "x_new"}, {a->P, nx * np, "P"}, {a->gp, np, "gp"}, {a->gx, nx, "gx"}, {a->gu, 1, "gu"}};
  const ArraySpan ins[3] = {{a->state, nx, "state"}, {a->gbar, nx, "gbar"}, {a->dyn, np, "dyn"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

// Simulator::Step with P = dx+/dp, or its product with a cotangent, and the state / control cotangents (sim_param_kernels.hpp)
extern "C" int cpmpc_sim_step_param_jac_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                                              const cpmpc_sim_param_jac* a, void* stream) {
  int rc = check_sim_param_jac_args(model, dtype, B, dyn_shared_host, dt, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_param_jac(B, dyn_shared_host, n_sub, h_last, a, (hipStream_t)stream);
  });
}

// ---- the plant over T ticks and its adjoint (sim_rollout_kernels.hpp) ------------------------------------------------
// What the two rollout calls check alike (no device needed); `what` names the struct
static int check_rollout_common(const char* what, uint64_t struct_size, size_t size_here, const void* x0, const void* u,
                                const double* dyn_shared_host, const void* dyn, double dt, int T, int model, int dtype,
                                int64_t B) {
  int rc = check_struct_size(what, struct_size, size_here);
  if (rc) return rc;
  if (!x0 || !u) return fail(CPMPC_ERR_INVALID_ARG, "null argument (x0, u)");
  if (!dyn_shared_host && !dyn) return fail(CPMPC_ERR_INVALID_ARG, "null argument (neither dyn_shared_host nor dyn is given)");
  rc = check_plant_dt(dt);
  if (rc) return rc;
  if (T < 1) return fail(CPMPC_ERR_INVALID_ARG, "T must be >= 1");
  return check_model_dtype_batch(model, dtype, B);
}

static int check_sim_rollout_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                  const cpmpc_sim_rollout* a) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (cpmpc_sim_rollout)");
  int rc = check_rollout_common("cpmpc_sim_rollout", a->struct_size, sizeof(cpmpc_sim_rollout), a->x0, a->u, dyn_shared_host,
                                a->dyn, dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->xs && !a->x_final) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  const ArraySpan outs[2] = {{a->xs, nt * nx, "xs"}, {a->x_final, nx, "x_final"}};
  const ArraySpan ins[4] = {{a->x0, nx, "x0"}, {a->u, nt, "u"}, {a->fext, 4, "fext"}, {a->dyn, np, "dyn"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_rollout_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                       const cpmpc_sim_rollout* a, void* stream) {
  int rc = check_sim_rollout_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_rollout(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

static int check_sim_rollout_vjp_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                      const cpmpc_sim_rollout_vjp* a) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (cpmpc_sim_rollout_vjp)");
  int rc = check_rollout_common("cpmpc_sim_rollout_vjp", a->struct_size, sizeof(cpmpc_sim_rollout_vjp), a->x0, a->u,
                                dyn_shared_host, a->dyn, dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->g_x0 && !a->g_u && !a->g_p) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  if (!a->gbar && !a->gbar_final) return fail(CPMPC_ERR_INVALID_ARG, "neither gbar nor gbar_final is given");
  if (T > 1 && !a->xs) return fail(CPMPC_ERR_INVALID_ARG, "xs (a forward call's checkpoints) is required when T > 1");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  const ArraySpan outs[3] = {{a->g_x0, nx, "g_x0"}, {a->g_u, nt, "g_u"}, {a->g_p, np, "g_p"}};
  const ArraySpan ins[7] = {{a->x0, nx, "x0"},           {a->u, nt, "u"},
                            {a->fext, 4, "fext"},        {a->dyn, np, "dyn"},
                            {a->xs, nt * nx, "xs"},      {a->gbar, nt * nx, "gbar"},
                            {a->gbar_final, nx, "gbar_final"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_rollout_vjp_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                           const cpmpc_sim_rollout_vjp* a, void* stream) {
  int rc = check_sim_rollout_vjp_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_rollout_vjp(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// ---- the window calls on top of the rollout: the two Gauss-Newton fits and the Kalman filter ---------------------------
// A host vector of n weights or variances, NULL for its default: every entry finite and >= 0
static int check_host_weights(const char* name, const double* v, size_t n) {
  if (v)
    for (size_t q = 0; q < n; ++q)
      if (!(v[q] >= 0.0) || !std::isfinite(v[q])) return fail(CPMPC_ERR_INVALID_ARG, "%s[%zu] must be finite and >= 0", name, q);
  return CPMPC_OK;
}

// The argument checks of the two Gauss-Newton calls (no device needed): their structs `what` differ in the output
// `final_field`, `final_name` [final_extent][B], and in n_unknowns, the length of g and the order of H
template <typename Args>
static int check_sim_rollout_gn_args(const char* what, const Args* a, void* Args::*final_field, const char* final_name,
                                     size_t final_extent, size_t n_unknowns, int model, int dtype, int64_t B,
                                     const double* dyn_shared_host, double dt, int T) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (%s)", what);
  int rc = check_rollout_common(what, a->struct_size, sizeof(Args), a->x0, a->u, dyn_shared_host, a->dyn, dt, T, model, dtype, B);
  if (rc) return rc;
  void* const final_out = a->*final_field;
  if (!a->cost && !a->g && !a->H && !final_out && !a->x_final)
    return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  if ((a->cost || a->g || a->H) && !a->x_obs) return fail(CPMPC_ERR_INVALID_ARG, "cost / g / H are given without x_obs");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  rc = check_host_weights("w_host", a->w_host, nx);
  if (rc) return rc;
  const ArraySpan outs[5] = {{a->cost, 1, "cost"}, {a->g, n_unknowns, "g"}, {a->H, n_unknowns * n_unknowns, "H"},
                             {final_out, final_extent, final_name}, {a->x_final, nx, "x_final"}};
  const ArraySpan ins[6] = {{a->x0, nx, "x0"},     {a->u, nt, "u"},
                            {a->fext, 4, "fext"},  {a->dyn, np, "dyn"},
                            {a->x_obs, nt * nx, "x_obs"}, {a->tick_w, nt, "tick_w"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

// the rollout's forward mode in the parameters and the normal equations of their fit (sim_rollout_gn_kernels.hpp)
extern "C" int cpmpc_sim_rollout_gn_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                          const cpmpc_sim_rollout_gn* a, void* stream) {
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model);
  int rc = check_sim_rollout_gn_args("cpmpc_sim_rollout_gn", a, &cpmpc_sim_rollout_gn::S_final, "S_final", nx * np, np, model, dtype, B,
                                     dyn_shared_host, dt, T);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_rollout_gn(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// the rollout's forward mode in the initial state and the normal equations of the fit of x0 (sim_rollout_gn_x0_kernels.hpp)
extern "C" int cpmpc_sim_rollout_gn_x0_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                             const cpmpc_sim_rollout_gn_x0* a, void* stream) {
  const size_t nx = (size_t)model_nx(model);
  int rc = check_sim_rollout_gn_args("cpmpc_sim_rollout_gn_x0", a, &cpmpc_sim_rollout_gn_x0::Phi_final, "Phi_final", nx * nx, nx, model,
                                     dtype, B, dyn_shared_host, dt, T);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_rollout_gn_x0(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// ---- the extended Kalman filter over T ticks (sim_ekf_kernels.hpp) and the smoother behind it (sim_rts_kernels.hpp) -------
// What the filter's and the smoother's structs `what` are checked for alike (no device needed): the rollout's rules, P0, an
// output, the host vectors, and y where a state is measured
template <typename Args>
static int check_ekf_inputs(const char* what, const Args* a, bool any_output, int model, int dtype, int64_t B,
                            const double* dyn_shared_host, double dt, int T) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (%s)", what);
  int rc = check_rollout_common(what, a->struct_size, sizeof(Args), a->x0, a->u, dyn_shared_host, a->dyn, dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->P0) return fail(CPMPC_ERR_INVALID_ARG, "null argument (P0)");
  if (!any_output) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  const size_t nx = (size_t)model_nx(model);
  rc = check_host_weights("w_host", a->w_host, nx);
  if (!rc) rc = check_host_weights("q_host", a->q_host, nx);
  if (rc) return rc;
  bool measured = !a->w_host;  // NULL: ones
  for (size_t i = 0; i < nx && !measured; ++i) measured = a->w_host[i] > 0.0;
  if (measured && !a->y) return fail(CPMPC_ERR_INVALID_ARG, "a state is measured (w_host > 0) without y");
  return CPMPC_OK;
}

static int check_sim_ekf_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                              const cpmpc_sim_ekf* a) {
  int rc = check_ekf_inputs("cpmpc_sim_ekf", a, a && (a->x_final || a->P_final || a->xs || a->nis), model, dtype, B,
                            dyn_shared_host, dt, T);
  if (rc) return rc;
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  const ArraySpan outs[4] = {{a->x_final, nx, "x_final"}, {a->P_final, nx * nx, "P_final"}, {a->xs, nt * nx, "xs"},
                             {a->nis, 1, "nis"}};
  const ArraySpan ins[7] = {{a->x0, nx, "x0"},      {a->P0, nx * nx, "P0"}, {a->u, nt, "u"},          {a->fext, 4, "fext"},
                            {a->dyn, np, "dyn"},    {a->y, nt * nx, "y"},   {a->tick_w, nt, "tick_w"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_ekf_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                   const cpmpc_sim_ekf* a, void* stream) {
  int rc = check_sim_ekf_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_ekf(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// rows of B numbers the smoother's forward pass records: T (2 NX + 2 NH + NX^2) (sim_window.hpp: RtsRecord)
extern "C" int64_t cpmpc_sim_rts_work_rows(int model, int T) {
  if ((model != CPMPC_MODEL_SINGLE && model != CPMPC_MODEL_DOUBLE) || T < 1) return 0;
  const int64_t nx = model_nx(model);
  return (int64_t)T * (2 * nx + nx * (nx + 1) + nx * nx);
}

static int check_sim_rts_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                              const cpmpc_sim_rts* a) {
  const bool any = a && (a->x_final || a->P_final || a->xs || a->nis || a->xs_smooth || a->Ps_smooth || a->x0_smooth ||
                         a->P0_smooth || a->ok);
  int rc = check_ekf_inputs("cpmpc_sim_rts", a, any, model, dtype, B, dyn_shared_host, dt, T);
  if (rc) return rc;
  if (!a->work) return fail(CPMPC_ERR_INVALID_ARG, "null argument (work)");
  const int64_t need = cpmpc_sim_rts_work_rows(model, T);
  if (a->work_rows < need)
    return fail(CPMPC_ERR_INVALID_ARG, "work_rows is %lld, T = %d ticks need %lld (cpmpc_sim_rts_work_rows)",
                (long long)a->work_rows, T, (long long)need);
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T, row = row_bytes(dtype, B);
  // ok holds B int32: at most one row of either dtype
  const ArraySpan outs[9] = {{a->x_final, nx, "x_final"},     {a->P_final, nx * nx, "P_final"},
                             {a->xs, nt * nx, "xs"},          {a->nis, 1, "nis"},
                             {a->xs_smooth, (nt + 1) * nx, "xs_smooth"}, {a->Ps_smooth, (nt + 1) * nx * nx, "Ps_smooth"},
                             {a->x0_smooth, nx, "x0_smooth"}, {a->P0_smooth, nx * nx, "P0_smooth"},
                             {a->ok, 1, "ok"}};
  const ArraySpan ins[7] = {{a->x0, nx, "x0"},      {a->P0, nx * nx, "P0"}, {a->u, nt, "u"},          {a->fext, 4, "fext"},
                            {a->dyn, np, "dyn"},    {a->y, nt * nx, "y"},   {a->tick_w, nt, "tick_w"}};
  rc = check_no_overlap(outs, ins, row);
  if (rc) return rc;
  // the workspace is written by the first launch and read by the second while inputs are read and outputs written
  const char* const w0 = (const char*)a->work;
  const size_t w_bytes = (size_t)need * row;
  auto over_work = [&](const ArraySpan& s) {
    const char* const s0 = (const char*)s.p;
    return s.p && s0 < w0 + w_bytes && w0 < s0 + s.rows * row;
  };
  for (const ArraySpan& s : ins)
    if (over_work(s)) return fail(CPMPC_ERR_INVALID_ARG, "work overlaps %s (give the workspace an array of its own)", s.name);
  for (const ArraySpan& s : outs)
    if (over_work(s)) return fail(CPMPC_ERR_INVALID_ARG, "work overlaps %s (give the workspace an array of its own)", s.name);
  return CPMPC_OK;
}

extern "C" int cpmpc_sim_rts_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                   const cpmpc_sim_rts* a, void* stream) {
  int rc = check_sim_rts_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_rts(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// ---- tracking a plant trajectory: its LQR gains and the plant under them (sim_track_kernels.hpp) -----------------------
// The weights of the tracking cost, which sim_lqr and the two iLQR passes check alike: r, then q_host, then qf_host
static int check_track_weights(double r, const double* q_host, const double* qf_host, size_t nx) {
  if (!(r > 0.0) || !std::isfinite(r)) return fail(CPMPC_ERR_INVALID_ARG, "r must be finite and > 0");
  int rc = check_host_weights("q_host", q_host, nx);
  if (!rc) rc = check_host_weights("qf_host", qf_host, nx);
  return rc;
}

static int check_sim_lqr_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                              const cpmpc_sim_lqr* a) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (cpmpc_sim_lqr)");
  int rc = check_rollout_common("cpmpc_sim_lqr", a->struct_size, sizeof(cpmpc_sim_lqr), a->x0, a->u, dyn_shared_host, a->dyn,
                                dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->K && !a->P0) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  if (T > 1 && !a->xs) return fail(CPMPC_ERR_INVALID_ARG, "xs (a forward call's checkpoints) is required when T > 1");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  rc = check_track_weights(a->r, a->q_host, a->qf_host, nx);
  if (rc) return rc;
  const ArraySpan outs[2] = {{a->K, nt * nx, "K"}, {a->P0, nx * nx, "P0"}};
  const ArraySpan ins[6] = {{a->x0, nx, "x0"},     {a->u, nt, "u"},        {a->fext, 4, "fext"},
                            {a->dyn, np, "dyn"},   {a->xs, nt * nx, "xs"}, {a->PT, nx * nx, "PT"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_lqr_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                   const cpmpc_sim_lqr* a, void* stream) {
  int rc = check_sim_lqr_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_lqr(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// What the two calls that roll the plant under a feedback law (the fb rollout, the iLQR's forward pass) check first: the
// struct `what`, u_nom by its own name, then the rollout's rules
template <typename Args>
static int check_fb_rollout_common(const char* what, const Args* a, const double* dyn_shared_host, double dt, int T, int model,
                                   int dtype, int64_t B) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (%s)", what);
  int rc = check_struct_size(what, a->struct_size, sizeof(Args));
  if (rc) return rc;
  if (!a->u_nom) return fail(CPMPC_ERR_INVALID_ARG, "null argument (u_nom)");
  return check_rollout_common(what, a->struct_size, sizeof(Args), a->x0, a->u_nom, dyn_shared_host, a->dyn, dt, T, model, dtype, B);
}

// ... and last before the overlaps: K needs the nominal trajectory it is a gain about.  `law`: the spans of K and of that
// trajectory, which is read only where K is given
template <typename Args>
static int check_feedback_law(const Args* a, int T, size_t nx, size_t nt, ArraySpan (&law)[3]) {
  if (a->K && !a->x0_nom) return fail(CPMPC_ERR_INVALID_ARG, "K is given without x0_nom");
  if (a->K && T > 1 && !a->xs_nom)
    return fail(CPMPC_ERR_INVALID_ARG, "K is given without xs_nom (the nominal checkpoints), required when T > 1");
  law[0] = {a->K, nt * nx, "K"};
  law[1] = {a->K ? a->x0_nom : nullptr, nx, "x0_nom"};
  law[2] = {a->K ? a->xs_nom : nullptr, nt * nx, "xs_nom"};
  return CPMPC_OK;
}

static int check_sim_rollout_fb_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                     const cpmpc_sim_rollout_fb* a) {
  int rc = check_fb_rollout_common("cpmpc_sim_rollout_fb", a, dyn_shared_host, dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->xs && !a->x_final && !a->us) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  if (!(a->u_limit > 0.0)) return fail(CPMPC_ERR_INVALID_ARG, "u_limit must be > 0 (infinity: no clamp)");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  ArraySpan law[3];
  rc = check_feedback_law(a, T, nx, nt, law);
  if (rc) return rc;
  const ArraySpan outs[3] = {{a->xs, nt * nx, "xs"}, {a->x_final, nx, "x_final"}, {a->us, nt, "us"}};
  const ArraySpan ins[7] = {{a->x0, nx, "x0"}, {a->u_nom, nt, "u_nom"}, {a->fext, 4, "fext"}, {a->dyn, np, "dyn"},
                            law[0],            law[1],                  law[2]};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_rollout_fb_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                          const cpmpc_sim_rollout_fb* a, void* stream) {
  int rc = check_sim_rollout_fb_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_rollout_fb(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// ---- iterative LQR on the plant's tick map: the backward and the forward pass (sim_ilqr_kernels.hpp) ---------------------
// what the two calls share beyond check_rollout_common: the cost's weights, the limit and the reference
template <typename Args>
static int check_sim_ilqr_cost(const Args* a, size_t nx) {
  int rc = check_track_weights(a->r, a->q_host, a->qf_host, nx);
  if (rc) return rc;
  if (!(a->u_limit > 0.0)) return fail(CPMPC_ERR_INVALID_ARG, "u_limit must be > 0 (infinity: no limit)");
  if (!a->x0_ref || !a->xs_ref)
    return fail(CPMPC_ERR_INVALID_ARG, "null argument (x0_ref, xs_ref: the reference; row T-1 of xs_ref is the terminal target)");
  return CPMPC_OK;
}

static int check_sim_ilqr_backward_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                        const cpmpc_sim_ilqr_backward* a) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument (cpmpc_sim_ilqr_backward)");
  int rc = check_rollout_common("cpmpc_sim_ilqr_backward", a->struct_size, sizeof(cpmpc_sim_ilqr_backward), a->x0, a->u,
                                dyn_shared_host, a->dyn, dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->K && !a->kff && !a->dV && !a->P0 && !a->g0 && !a->hmax)
    return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  if (T > 1 && !a->xs) return fail(CPMPC_ERR_INVALID_ARG, "xs (a forward call's checkpoints) is required when T > 1");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  rc = check_sim_ilqr_cost(a, nx);
  if (rc) return rc;
  const ArraySpan outs[6] = {{a->K, nt * nx, "K"},     {a->kff, nt, "kff"}, {a->dV, 2, "dV"},
                             {a->P0, nx * nx, "P0"},   {a->g0, nx, "g0"},   {a->hmax, 1, "hmax"}};
  const ArraySpan ins[10] = {{a->x0, nx, "x0"},         {a->u, nt, "u"},
                             {a->fext, 4, "fext"},      {a->dyn, np, "dyn"},
                             {a->xs, nt * nx, "xs"},    {a->x0_ref, nx, "x0_ref"},
                             {a->xs_ref, nt * nx, "xs_ref"}, {a->u_ref, nt, "u_ref"},
                             {a->PT, nx * nx, "PT"},    {a->mu, 1, "mu"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_ilqr_backward_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                                             int T, const cpmpc_sim_ilqr_backward* a, void* stream) {
  int rc = check_sim_ilqr_backward_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_ilqr_backward(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

static int check_sim_ilqr_forward_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                       const cpmpc_sim_ilqr_forward* a) {
  int rc = check_fb_rollout_common("cpmpc_sim_ilqr_forward", a, dyn_shared_host, dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->xs && !a->x_final && !a->us && !a->cost) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  rc = check_sim_ilqr_cost(a, nx);
  if (rc) return rc;
  ArraySpan law[3];
  rc = check_feedback_law(a, T, nx, nt, law);
  if (rc) return rc;
  const ArraySpan outs[4] = {{a->xs, nt * nx, "xs"}, {a->x_final, nx, "x_final"}, {a->us, nt, "us"}, {a->cost, 1, "cost"}};
  const ArraySpan ins[13] = {{a->x0, nx, "x0"},         {a->u_nom, nt, "u_nom"},         {a->fext, 4, "fext"},
                             {a->dyn, np, "dyn"},       {a->kff, nt, "kff"},             law[0],
                             law[1],                    law[2],                          {a->alpha, 1, "alpha"},
                             {a->x0_ref, nx, "x0_ref"}, {a->xs_ref, nt * nx, "xs_ref"},  {a->u_ref, nt, "u_ref"},
                             {a->PT, nx * nx, "PT"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_ilqr_forward_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                            const cpmpc_sim_ilqr_forward* a, void* stream) {
  int rc = check_sim_ilqr_forward_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_ilqr_forward(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

static int check_sim_ilqr_search_args(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                      const cpmpc_sim_ilqr_search* a) {
  int rc = check_fb_rollout_common("cpmpc_sim_ilqr_search", a, dyn_shared_host, dt, T, model, dtype, B);
  if (rc) return rc;
  if (!a->xs && !a->x_final && !a->us && !a->cost && !a->alpha)
    return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  const size_t nx = (size_t)model_nx(model), np = (size_t)model_np(model), nt = (size_t)T;
  rc = check_sim_ilqr_cost(a, nx);
  if (rc) return rc;
  if (!a->xs_nom) return fail(CPMPC_ERR_INVALID_ARG, "null argument (xs_nom: always required, row T-1 is a failed problem's x_final)");
  if (!a->cost_nom) return fail(CPMPC_ERR_INVALID_ARG, "null argument (cost_nom)");
  if (!a->kff) return fail(CPMPC_ERR_INVALID_ARG, "null argument (kff)");
  if (!a->dV) return fail(CPMPC_ERR_INVALID_ARG, "null argument (dV)");
  if (a->trials < 1 || a->trials > 32) return fail(CPMPC_ERR_INVALID_ARG, "trials is %d, must be in 1..32", (int)a->trials);
  if (a->reserved != 0) return fail(CPMPC_ERR_INVALID_ARG, "reserved is %d, must be 0", (int)a->reserved);
  if (!(a->armijo > 0.0 && a->armijo < 1.0)) return fail(CPMPC_ERR_INVALID_ARG, "armijo must be finite and in (0, 1)");
  // xs and us are written during the trials: every input is still read after the first store
  const ArraySpan outs[5] = {{a->xs, nt * nx, "xs"}, {a->x_final, nx, "x_final"}, {a->us, nt, "us"}, {a->cost, 1, "cost"},
                             {a->alpha, 1, "alpha"}};
  const ArraySpan ins[13] = {{a->x0, nx, "x0"},         {a->u_nom, nt, "u_nom"},        {a->fext, 4, "fext"},
                             {a->dyn, np, "dyn"},       {a->xs_nom, nt * nx, "xs_nom"}, {a->cost_nom, 1, "cost_nom"},
                             {a->kff, nt, "kff"},       {a->K, nt * nx, "K"},           {a->dV, 2, "dV"},
                             {a->x0_ref, nx, "x0_ref"}, {a->xs_ref, nt * nx, "xs_ref"}, {a->u_ref, nt, "u_ref"},
                             {a->PT, nx * nx, "PT"}};
  return check_no_overlap(outs, ins, row_bytes(dtype, B));
}

extern "C" int cpmpc_sim_ilqr_search_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                           const cpmpc_sim_ilqr_search* a, void* stream) {
  int rc = check_sim_ilqr_search_args(model, dtype, B, dyn_shared_host, dt, T, a);
  if (rc) return rc;
  return run_plant_call(dt, false, [&](int n_sub, double h_last) {
    engine_for(dtype, model)->sim_ilqr_search(B, dyn_shared_host, n_sub, h_last, T, a, (hipStream_t)stream);
  });
}

// ------------------------------------------------------------------------------------------------
// feedback gains
// ------------------------------------------------------------------------------------------------
int check_gain_args(const cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, const void* K) {
  if (!s || !in || !K) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (in->struct_size != sizeof(cpmpc_gain_inputs))
    return fail(CPMPC_ERR_INVALID_ARG, "cpmpc_gain_inputs.struct_size is %llu, this library's is %zu (set it to sizeof(cpmpc_gain_inputs))",
                (unsigned long long)in->struct_size, sizeof(cpmpc_gain_inputs));
  if (n_rows < 1 || n_rows > s->N) return fail(CPMPC_ERR_INVALID_ARG, "n_rows must be in [1, window_length = %d]", s->N);
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  if (B > s->cap) return fail(CPMPC_ERR_BATCH, "B=%lld exceeds the capacity %lld given to cpmpc_create", (long long)B, (long long)s->cap);
  if ((in->dyn_shared_host == nullptr) == (in->dyn == nullptr))
    return fail(CPMPC_ERR_INVALID_ARG, "exactly one of dyn_shared_host / dyn must be given");
  if (in->z == nullptr && B > s->prev_B)
    return fail(CPMPC_ERR_INVALID_ARG, "z is NULL and the handle holds a previous solution for %lld problems only, not %lld",
                (long long)s->prev_B, (long long)B);
  return CPMPC_OK;
}

extern "C" int cpmpc_feedback_gain_batch(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K,
                                         int32_t* ok, void* stream) {
  int rc = check_gain_args(s, B, in, n_rows, K);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  engine_of(s)->feedback_gain(s, B, in, n_rows, K, ok, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  track_caller_stream(s, (hipStream_t)stream);  // the workspace (warm start read, scratch written) was used on the caller's stream
  return CPMPC_OK;
}

extern "C" int cpmpc_feedback_apply_batch(int dtype, int model, int64_t B, const void* u_nom, const void* K0,
                                          const void* x_nom, const void* x, double u_limit, void* u_out, void* stream) {
  if (!u_nom || !K0 || !x_nom || !x || !u_out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (!(u_limit > 0.0)) return fail(CPMPC_ERR_INVALID_ARG, "u_limit must be > 0 (infinity: no clamp)");
  int rc = check_piece_args(model, dtype, B);
  if (rc) return rc;
  engine_for(dtype, model)->feedback_apply(B, u_nom, K0, x_nom, x, u_limit, u_out, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return CPMPC_OK;
}

// ------------------------------------------------------------------------------------------------
// plan sensitivities, plan update
// ------------------------------------------------------------------------------------------------
extern "C" int cpmpc_plan_sensitivity_batch(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K,
                                            void* k_sp, void* k_up, int32_t* ok, void* stream) {
  // the gain call's checks, on whichever output was asked for (none: a null argument)
  int rc = check_gain_args(s, B, in, n_rows, K ? K : (k_sp ? k_sp : k_up));
  if (rc) return rc;
  DeviceGuard guard(s->device);
  engine_of(s)->plan_sensitivity(s, B, in, n_rows, K, k_sp, k_up, ok, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  track_caller_stream(s, (hipStream_t)stream);  // the workspace (warm start read, scratch written) was used on the caller's stream
  return CPMPC_OK;
}

// g_x0 = K^T gbar, g_sp = k_sp^T gbar, g_up = k_up^T gbar (plan_vjp_kernels.hpp)
extern "C" int cpmpc_plan_vjp_batch(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, const void* gbar,
                                    void* g_x0, void* g_sp, void* g_up, int32_t* ok, void* stream) {
  if (!gbar) return fail(CPMPC_ERR_INVALID_ARG, "null argument (gbar)");
  // the gain call's checks, on whichever output was asked for (none: a null argument)
  int rc = check_gain_args(s, B, in, n_rows, g_x0 ? g_x0 : (g_sp ? g_sp : g_up));
  if (rc) return rc;
  DeviceGuard guard(s->device);
  engine_of(s)->plan_vjp(s, B, in, n_rows, gbar, g_x0, g_sp, g_up, ok, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  track_caller_stream(s, (hipStream_t)stream);  // the workspace (warm start read, scratch written) was used on the caller's stream
  return CPMPC_OK;
}

// The argument checks of cpmpc_plan_weight_vjp_batch[_host], the ones that need no handle first.  A null handle with
// otherwise well-formed arguments is CPMPC_ERR_NO_DEVICE where no usable device is visible (no handle can exist there: the
// product has no CPU path), CPMPC_ERR_INVALID_ARG otherwise.
int check_weight_vjp_args(const cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows, const void* gbar,
                          const void* g_tw, const void* g_wu, const void* g_wdu, const void* du) {
  if (!in) return fail(CPMPC_ERR_INVALID_ARG, "null argument (in)");
  if (in->struct_size != sizeof(cpmpc_weight_vjp_inputs))
    return fail(CPMPC_ERR_INVALID_ARG,
                "cpmpc_weight_vjp_inputs.struct_size is %llu, this library's is %zu (set it to sizeof(cpmpc_weight_vjp_inputs))",
                (unsigned long long)in->struct_size, sizeof(cpmpc_weight_vjp_inputs));
  if (!g_tw && !g_wu && !g_wdu && !du) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  if (n_rows < 1) return fail(CPMPC_ERR_INVALID_ARG, "n_rows must be >= 1");
  if (!in->x0) return fail(CPMPC_ERR_INVALID_ARG, "null argument (x0)");
  if (!gbar && (g_tw || g_wu || g_wdu)) return fail(CPMPC_ERR_INVALID_ARG, "null argument (gbar, with a gradient output)");
  if (!s) {
    const int rc = current_device_ok();
    return rc ? rc : fail(CPMPC_ERR_INVALID_ARG, "null argument (handle)");
  }
  return check_gain_args(s, B, &in->lin, n_rows, in);
}

// g_tw, g_wu, g_wdu = d(gbar . u+)/d(cost weights) and the primal QP step du (plan_weight_vjp_kernels.hpp)
extern "C" int cpmpc_plan_weight_vjp_batch(cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows,
                                           const void* gbar, void* g_tw, void* g_wu, void* g_wdu, void* du, int32_t* ok,
                                           void* stream) {
  int rc = check_weight_vjp_args(s, B, in, n_rows, gbar, g_tw, g_wu, g_wdu, du);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  engine_of(s)->plan_weight_vjp(s, B, in, n_rows, gbar, g_tw, g_wu, g_wdu, du, ok, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  track_caller_stream(s, (hipStream_t)stream);  // the workspace (warm start read, scratch written) was used on the caller's stream
  return CPMPC_OK;
}

extern "C" int cpmpc_plan_update_batch(int dtype, int model, int64_t B, int n_rows, const cpmpc_plan_update* a,
                                       void* stream) {
  if (!a) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (a->struct_size != sizeof(cpmpc_plan_update))
    return fail(CPMPC_ERR_INVALID_ARG, "cpmpc_plan_update.struct_size is %llu, this library's is %zu (set it to sizeof(cpmpc_plan_update))",
                (unsigned long long)a->struct_size, sizeof(cpmpc_plan_update));
  if (!a->u_nom || !a->u_out) return fail(CPMPC_ERR_INVALID_ARG, "null argument (u_nom, u_out)");
  if (a->K && (!a->x_nom || !a->x)) return fail(CPMPC_ERR_INVALID_ARG, "K is given without x_nom and x");
  if (a->k_sp && (!a->sp_nom || !a->sp)) return fail(CPMPC_ERR_INVALID_ARG, "k_sp is given without sp_nom and sp");
  if (a->k_up && (!a->u_prev_nom || !a->u_prev)) return fail(CPMPC_ERR_INVALID_ARG, "k_up is given without u_prev_nom and u_prev");
  if (!(a->u_limit > 0.0)) return fail(CPMPC_ERR_INVALID_ARG, "u_limit must be > 0 (infinity: no clamp)");
  if (n_rows < 1 || n_rows > 65535) return fail(CPMPC_ERR_INVALID_ARG, "n_rows must be in [1, 65535]");
  int rc = check_piece_args(model, dtype, B);
  if (rc) return rc;
  engine_for(dtype, model)->plan_update(B, n_rows, a, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return CPMPC_OK;
}

// debug builds only (-DCPMPC_FUSED_TIMING / -DCPMPC_FUSED_CLOCK): the counters of fused_sqp_kernel, summed over the
// kernel translation units (each has its own copies), read and cleared
static int debug_read_all(int which, unsigned long long* out, int n) {
  (void)hipDeviceSynchronize();
  for (int i = 0; i < n; ++i) out[i] = 0;
  int ok = -1;
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int model = 0; model < 2; ++model)
      if (engine_for(dtype, model)->debug_read(which, out) == 0) ok = 0;
  return ok;
}
#ifdef CPMPC_FUSED_TIMING
extern "C" int cpmpc_debug_phase_cycles(unsigned long long* out8) { return debug_read_all(0, out8, 8); }
#endif
#ifdef CPMPC_FUSED_CLOCK
extern "C" int cpmpc_debug_kernel_clock(unsigned long long* out4) { return debug_read_all(1, out4, 4); }
#endif
