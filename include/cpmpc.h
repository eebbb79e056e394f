/*
 * cpmpc.h -- C-ABI of the MI355X-native batched cart-pole MPC hot path (libcpmpc.so).
 *
 * The reference (gareth-cross/cart-pole-mpc) has NO plugin/FFI boundary for this path: the hot
 * path is the C++ class API
 *     pendulum::Optimization   optimization/optimization.hpp:73-108
 *     pendulum::Simulator      optimization/simulator.hpp:10-29
 * linked statically into the nanobind module `pypendulum` (wrapper/wrapper.cc:40-102).  This header
 * is the boundary a maintainer would bind instead: plain pointers and sizes, int return codes, no
 * exceptions, caller owns every buffer, the handle owns the device-resident warm-start state
 * (the batched counterpart of Optimization::previous_solution_, optimization.hpp:107).
 * Each entry point names the reference interface it replaces.
 *
 * Data layout: every batched array is structure-of-arrays, [field][B] with the batch index
 * fastest, in the handle's dtype (float or double), in DEVICE memory unless the name ends in
 * `_host`.  Variable layout of the solution vector z follows MapKey (optimization.cc:27-37):
 *     z[4*s + t]  state t of shooting node s   (t: 0=b_x 1=th_1 2=b_x_dot 3=th_1_dot; key.hpp:8-19)
 *     z[4*S + k]  control u_k                  (S = window_length/state_spacing + 1, k < N)
 */
#ifndef CPMPC_H
#define CPMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPMPC_STATE_DIM 4
#define CPMPC_NUM_DYN_PARAMS 9

/* ---- return codes ---------------------------------------------------------------------------- */
enum {
  CPMPC_OK = 0,
  CPMPC_ERR_INVALID_ARG = 1,  /* violates a precondition the reference asserts (F_ASSERT*) */
  CPMPC_ERR_UNSUPPORTED = 2,  /* valid in the reference but not built into this library */
  CPMPC_ERR_NO_DEVICE = 3,    /* no HIP device / wrong architecture: there is NO CPU fallback */
  CPMPC_ERR_HIP = 4,          /* a HIP runtime call failed; see cpmpc_last_error() */
  CPMPC_ERR_ALLOC = 5,
  CPMPC_ERR_BATCH = 6         /* B exceeds the capacity given to cpmpc_create */
};

enum { CPMPC_F32 = 0, CPMPC_F64 = 1 };

/* Per-problem termination state, written to `status`.  Names and meaning follow
 * mini_opt::NLSTerminationState as the reference uses it (optimization_test.cc:44-46). */
enum {
  CPMPC_TERM_NONE = 0,
  CPMPC_TERM_MAX_ITERATIONS = 1,
  CPMPC_TERM_SATISFIED_ABSOLUTE_TOL = 2,
  CPMPC_TERM_SATISFIED_RELATIVE_TOL = 3,
  CPMPC_TERM_SATISFIED_FIRST_ORDER_TOL = 4,
  CPMPC_TERM_QP_INDEFINITE = 5,
  CPMPC_TERM_USER_CALLBACK = 6,
  CPMPC_TERM_MAX_LAMBDA = 7,
  CPMPC_TERM_NON_FINITE = 8
};

/* ---- parameters ------------------------------------------------------------------------------ */

/* pendulum::OptimizationParams, field for field (optimization/optimization.hpp:12-53). */
typedef struct cpmpc_params {
  double control_dt;
  uint64_t window_length;
  uint64_t state_spacing;
  uint64_t max_iterations;
  double relative_exit_tol;
  double absolute_first_derivative_tol;
  double equality_penalty_initial;
  double u_guess_sinusoid_amplitude;
  double u_cost_weight;
  double u_derivative_cost_weight;
  double b_x_final_cost_weight;
  double th_final_cost_weight;
  double b_x_dot_final_cost_weight;
  double th_dot_final_cost_weight;
} cpmpc_params;

/* Knobs of the SQP that stands where mini_opt::ConstrainedNonlinearLeastSquares stands
 * (optimization.cc:73-81).  Only max_line_search_iterations (=5, optimization.cc:76) and the two
 * clamps (optimization.cc:320,327) come from the reference; see DESIGN.md section 4. */
typedef struct cpmpc_solver_opts {
  int32_t max_line_search_iterations;
  double armijo_c1;
  double ls_shrink_max;
  double ls_shrink_min;
  double ls_alpha_growth;
  double penalty_rho;
  double lambda_initial;
  double lambda_failure_init;
  double lambda_scale_up;
  double lambda_scale_down;
  double lambda_min;
  double lambda_max;
  double b_x_limit;
  double u_limit;
  double ls_alpha_growth_backtracked; /* growth used instead of ls_alpha_growth when the accepted search backtracked */
  double full_step_below; /* an UNDAMPED QP step (lambda = 0) with |dz|_inf <= this is taken in full without the merit
                           * test (local convergence safeguard; default 1e-4, 0 disables) */
  double exit_defect_floor; /* the first-order exit test |g.dz - mu |c|_1| < absolute_first_derivative_tol counts |c|_1 as
                             * zero when it is at most exit_defect_floor * state_spacing * eps * (S - 1) * sum_t (|target_t| +
                             * |x_{S-1,t} - target_t|) -- the size of the states, taken at the terminal node, times the number of
                             * intervals (eps of the kernels' arithmetic): equality residuals of that size are the rounding of
                             * the rollout itself -- state_spacing RK4 steps -- and no iteration can remove them.  In fp64
                             * that floor would be 3e-14: the rule is a SINGLE-PRECISION rule -- CPMPC_F64 handles ignore this
                             * option (their kernels do not carry the test, and neither does the double CPU check: one exit
                             * rule in the parity dtype); in fp32 it is 1.5e-5, and it is what lets settled
                             * controllers leave after one iteration at the reference's tolerance of 1e-6 instead of
                             * iterating on noise (DESIGN.md sections 4 and 6.4; default 2, 0 disables; appended in round 4).
                             * Measured, fp32, 65 536 settled controllers: 0 -> 2.8 iterations per tick, 2 -> 1.8, 8 -> 1.0,
                             * the same closed-loop accuracy throughout */
} cpmpc_solver_opts;

void cpmpc_default_params(cpmpc_params* p);           /* optimization.hpp:12-48 defaults */
void cpmpc_default_solver_opts(cpmpc_solver_opts* o); /* DESIGN.md section 4 defaults */

/* Thread-local text of the last failure on this thread. */
const char* cpmpc_last_error(void);

/* Number of usable gfx950 devices (0 if none); does not create a context. */
int cpmpc_device_count(void);

/* ---- the solver handle: replaces `pendulum::Optimization` ---------------------------------- */

typedef struct cpmpc_solver cpmpc_solver;

/* Replaces Optimization::Optimization(const OptimizationParams&) (optimization.cc:13-22), for a
 * batch of up to `max_batch` independent controllers on HIP device `device`.  The reference's
 * constructor preconditions give CPMPC_ERR_INVALID_ARG.  Any state_spacing that divides window_length is
 * accepted (optimization.cc:16-18); which ones have specialised kernels: cpmpc_supported_state_spacing(). */
int cpmpc_create(const cpmpc_params* params, const cpmpc_solver_opts* opts /*nullable*/, int dtype,
                 int64_t max_batch, int device, cpmpc_solver** out);
void cpmpc_destroy(cpmpc_solver* s);

/* The same constructor with its arguments in a size-versioned struct, plus what the positional forms cannot express:
 *   flags      CPMPC_CREATE_STRICT_HORIZON: refuse (CPMPC_ERR_UNSUPPORTED) a horizon window_length * control_dt beyond
 *              cpmpc_max_parity_horizon().  By DEFAULT every horizon the reference's constructor accepts
 *              (optimization.cc:13-22) is accepted, by every entry point -- the library is a drop-in -- and the first
 *              such handle of a process writes one warning to stderr (CPMPC_CREATE_ALLOW_LONG_HORIZON, the opt-in of
 *              round 4 when the refusal was the default, is still accepted and now only silences that warning).  What the
 *              bound means: the QP is solved by eliminating the states through the shooting recursion, and through more than
 *              ~1 s of the default pole (unstable at e^{6.3 t}) that loses digits against a full-space KKT solve with
 *              pivoting -- measured at control_dt 0.01 (profiles/r04_parity_sweep.json): window_length 80 and 100 keep
 *              every one of 32 768 cold-start problems within 3e-6 / 4e-7 of the CPU check (three to eight iterations);
 *              at 120, 2 of 16 384 are beyond 1e-5 (worst 1.6e-5); at 160, 0.4 % are (worst 1e-2 .. 0.4 depending on
 *              the sample).  Warm-started closed loops are not affected in practice, cold starts far from the optimum
 *              are; a caller that needs the 1e-5 bar on every problem asks for the refusal.
 *   opts_size  sizeof(cpmpc_solver_opts) as the CALLER was compiled (0 = this header's).  Option fields are only ever
 *              appended; a caller built against an earlier header passes its shorter size and keeps the library's
 *              defaults for the fields it does not know (full_step_below was appended in round 3, exit_defect_floor in
 *              round 4).  Must be the size of the struct in some release: 8 + 8 k bytes, 112 (the fields through u_limit) <= size <= this header's.
 *              Always start from cpmpc_default_solver_opts: a zero-initialised struct is NOT the defaults.
 *              The positional constructors (cpmpc_create, cpmpc_create_model, cpmpc_sharded_create) cannot be told the
 *              caller's size: they read CPMPC_SOLVER_OPTS_SIZE_POSITIONAL bytes -- the struct as it was when they were
 *              frozen, i.e. up to and including full_step_below -- and take the library's defaults for everything
 *              appended since (exit_defect_floor); newer options are set through cpmpc_create_ex.
 *   flags      CPMPC_CREATE_REFINE_QP / CPMPC_CREATE_NO_REFINE_QP: force on / off one step of iterative refinement of the
 *              whole QP solution in the fused CPMPC_F64 kernels -- residuals evaluated in the original data (terminal rows
 *              through the recovered states, stationarity through the adjoint), solved again with the factors at hand.
 *              It brings the condensed solve below the error of a dense KKT solve with pivoting (CPU model, worst of
 *              150 problems: 3e-14 against 3e-13 at w_u = 0, w_du = 0.1) and costs 7 % of the step (50.2 -> 46.7 M
 *              re-plans/s at B = 262 144).  DEFAULT (neither flag): on when u_cost_weight < 0.05, half the reference's
 *              0.1.  Measured (profiles/r04_fuzz_sweep_2000*.json: 2 000 random problem definitions x 2 048 lanes, the
 *              extended-precision arbiter on every lane that is off; "at fault" = beyond 1e-5 and more than twice as far
 *              from the extended-precision answer as the double CPU check):
 *                 u_cost_weight >= 0.05:  0 of 1 798 144 lanes at fault, refined or not;
 *                 u_cost_weight <  0.05:  144 of 1 374 208 without the refinement, 9 with it (two definitions whose
 *                                         controls run into the +-300 N clamp, where the retraction is not smooth);
 *                 and, whatever the weights, definitions whose friction the explicit RK4 cannot follow (v_mu_b = 1e-7
 *                 with mu_b > 0: a slope of 1e5..1e6 1/s against a stability limit of 280 1/s at 10 ms; |Phi| reaches
 *                 1e4 per interval, the terminal system's condition 1e18): 281 of 923 648 lanes, 72 with it.
 *              And for CPMPC_MODEL_DOUBLE when th_final_cost_weight >= 0 with th_dot_final_cost_weight < 0 (the pole angles
 *              cost rows, their rates equalities): the first QP of a cold start is 7e-9 from an extended-precision solve
 *              without the refinement (the CPU check: 2e-10) and 7e-12 with it, and on a lane on which the CPU check ends
 *              within 2e-8 of that solve after four iterations the kernels end 5e-5 from it without and 1e-7 with it
 *              (40 steps, spacing 8; tests/test_gpu_double_parity.py).  The rule reads the handle's parameters: a caller
 *              who sets such rows per problem (terminal_weights) on a handle whose own rows are not of that kind passes
 *              CPMPC_CREATE_REFINE_QP.
 *              Both pipelines; ignored by CPMPC_F32 handles.  cpmpc_refines_qp() tells what a handle does. */
#define CPMPC_CREATE_ALLOW_LONG_HORIZON 1u /* accepted; silences the long-horizon warning */
#define CPMPC_CREATE_REFINE_QP 2u
#define CPMPC_CREATE_NO_REFINE_QP 4u
#define CPMPC_CREATE_STRICT_HORIZON 8u
#define CPMPC_CREATE_WIDE_QP 16u
#define CPMPC_CREATE_NO_WIDE_QP 32u
typedef struct cpmpc_create_info {
  uint32_t struct_size; /* = sizeof(cpmpc_create_info) */
  uint32_t flags;
  int32_t dtype;  /* CPMPC_F32 / CPMPC_F64 */
  int32_t model;  /* CPMPC_MODEL_* */
  int32_t device; /* HIP device */
  int32_t reserved; /* 0 */
  int64_t max_batch;
  const cpmpc_params* params;
  const cpmpc_solver_opts* opts; /* nullable */
  uint64_t opts_size;
} cpmpc_create_info;
int cpmpc_create_ex(const cpmpc_create_info* info, cpmpc_solver** out);
/* bytes of cpmpc_solver_opts the positional constructors read (the struct through full_step_below) */
#define CPMPC_SOLVER_OPTS_SIZE_POSITIONAL 128u
int cpmpc_refines_qp(const cpmpc_solver* s); /* 1: this handle's kernels refine the QP solution (CPMPC_CREATE_REFINE_QP) */
/* The solver options a handle actually uses -- this library's defaults overlaid with as many leading bytes of the caller's
 * struct as its constructor read: the positional constructors (cpmpc_create, cpmpc_create_model, cpmpc_sharded_create) read
 * CPMPC_SOLVER_OPTS_SIZE_POSITIONAL bytes, so a field appended later (exit_defect_floor) set through them is NOT taken and
 * keeps its default; cpmpc_create_ex reads opts_size.  out_size: sizeof of the caller's struct (112 .. sizeof here, 8 + 8 k).
 * A struct shorter than 112 bytes (the 13 doubles through u_limit: the shortest layout that is a prefix of today's) is
 * refused by every constructor. */
int cpmpc_get_solver_opts(const cpmpc_solver* s, cpmpc_solver_opts* out, size_t out_size);
/* CPMPC_CREATE_WIDE_QP / CPMPC_CREATE_NO_WIDE_QP (CPMPC_F32 handles; ignored by CPMPC_F64 ones): force on / off that the fused
 * kernels carry the whole terminal part of the QP in double -- the products of transition matrices across the shooting
 * intervals, the columns of U^-1 R^T, the multipliers and their effect on the step -- not only the NX x NX system.  It is
 * the precision of the QP solve, not the hardware's sin / cos / exp, that separates a float handle from the double CPU
 * check: with it the kernels end where the float build of that check (its KKT solve in double) ends.  Measured (round 5,
 * cold starts, 5 iterations, max |du| per problem against the double check: median / 99th percentile / share within 1e-2):
 *   4-state model, B = 262 144:  2.4e-4 / 0.11 / 93.0 %  ->  8.4e-5 / 4.9e-3 / 99.5 %   (float CPU check 8.0e-5 / 4.9e-3 / 99.3 %)
 *                                for 3.8 % of the cold-start throughput (122.5 -> 117.9 M re-plans/s) and 7 - 9 % of a
 *                                closed-loop tick, where it changes nothing that matters (warm-started iterations near the
 *                                optimum: same iteration counts, same final pole error);
 *   6-state model, B = 65 536:   4.2e-2 / 8.0 / 19.8 %   ->  5.7e-4 / 9.3e-3 / 99.1 %   (float CPU check 5.2e-4 / 8.7e-3 / 99.2 %)
 *                                for 0 - 5 % (51.0 -> 50.8 M near upright, 50.9 -> 48.3 M from within 0.5 rad).
 * DEFAULT (neither flag): ON for the 6-state model -- without it four of five float solves of that model are off by more
 * than 0.01 N after five iterations -- and OFF for the 4-state one (the reference's model: speed first, the bar of this
 * path is met by CPMPC_F64 handles; a caller who re-plans from cold starts in single precision should pass the flag: 3.8 %
 * of the throughput for 93.7 -> 99.4 % of the problems within 1e-2 of the double answer).  The option belongs to the handle,
 * not to the step: "on for cold-start steps only" was tried in round 6 and withdrawn (a problem's arithmetic would then depend
 * on which other problems share its call).  Both pipelines since round 6: a float handle that AUTO or cpmpc_set_pipeline() sends to
 * the split pipeline (state spacings the fused kernel is not built for) runs qp_ls_kernel's wide form -- the same quantities
 * in double, one more pass over the workspace -- and lands where the fused one does (tests/test_gpu_round6.py: the 6-state
 * model at state_spacing 20 against the float CPU check).  cpmpc_wide_qp() tells what a handle does, in either pipeline. */
int cpmpc_wide_qp(const cpmpc_solver* s);
/* seconds: the longest horizon held to 1e-5 of the CPU check on every problem (1.0) */
double cpmpc_max_parity_horizon(void);
/* 1: this handle's horizon window_length * control_dt is beyond cpmpc_max_parity_horizon() -- a PER-HANDLE status (round 6;
 * the once-per-process line on stderr is easy to miss in a notebook): such a handle is solved as asked, with the QP
 * refinement of CPMPC_CREATE_REFINE_QP on by default (CPMPC_F64) and, under CPMPC_PIPELINE_AUTO, by the split pipeline with
 * two refinement passes; on a few cold starts in 10^4 far from the optimum its controls may still differ from a full-space
 * solve by more than 1e-5 (measured at 1.6 s, three iterations: 1 of 8 192 lanes with the kernels at fault by the
 * extended-precision arbiter and 1 with the CPU check at fault, 34 / 0 without the refinement; a dense pivoted solve in
 * double is itself up to 6.6e-5 from the extended-precision answer there).  pendulum::Optimization::HorizonBeyondParity(), the
 * `horizon_beyond_parity` attribute of pypendulum.Optimization and a line in solver_summary() carry it to the caller.
 * 0: within the bound; -1: null handle.  Replaces nothing in the reference (optimization.cc:13-22 accepts any horizon). */
int cpmpc_horizon_beyond_parity(const cpmpc_solver* s);

/* 2: register-resident linearisation compiled for this spacing (1,2,4,5,8,10,20); 1: served by the generic
 * run-time-spacing kernel; 0: not a valid spacing */
int cpmpc_supported_state_spacing(int spacing);

/* Inputs of one batched re-plan.  Exactly one of dyn_shared_host / dyn must be non-NULL. */
typedef struct cpmpc_step_inputs {
  const void* x0;                /* [4][B]  measured states (Step's current_state) */
  const double* dyn_shared_host; /* HOST [9] SingleCartPoleParams shared by the batch, or NULL */
  const void* dyn;               /* [9][B]  per-problem SingleCartPoleParams, or NULL */
  double set_point_shared;       /* b_x_set_point shared by the batch (used if set_point NULL) */
  const void* set_point;         /* [B]     per-problem b_x_set_point, or NULL */
  /* [NX][B] per-problem terminal weights in state order {b_x, th.., b_x', th'..}, replacing the four *_final_cost_weight
   * parameters for this call: >= 0 a cost row with that weight, < 0 an equality row (optimization.cc:236-267; the
   * per-controller toggles of viz/src/application.ts:279-342).  NULL: the handle's parameters apply to every problem. */
  const void* terminal_weights;
} cpmpc_step_inputs;

/* Outputs; every pointer is nullable. */
typedef struct cpmpc_step_outputs {
  void* u;             /* [N][B]     OptimizationOutputs::u                (optimization.hpp:66) */
  void* predicted;     /* [N][4][B]  OptimizationOutputs::predicted_states (optimization.hpp:69) */
  int32_t* status;     /* [B]        solver_outputs.termination_state */
  int32_t* iterations; /* [B]        QP solves performed */
  int32_t* ls_evals;   /* [B]        merit evaluations performed */
  void* final_cost;    /* [B]        1/2 |r|^2 at the returned solution's last evaluation.  A problem that leaves with
                        *            SATISFIED_FIRST_ORDER_TOL after a tiny undamped step took that step without a merit
                        *            evaluation: its final_cost / final_eq_l1 are those of the iterate the
                        *            step was computed from, one (tiny: |dz|_inf <= full_step_below) step behind u / solution */
  void* final_eq_l1;   /* [B]        |c|_1 there */
  void* guess;         /* [dim][B]   the initial guess handed to the solver */
  void* solution;      /* [dim][B]   the solution z = solver_->variables() (optimization.cc:85), MapKey order: what the
                        *            next Step reports as OptimizationOutputs::previous_solution (optimization.cc:84) */
} cpmpc_step_outputs;

/* Replaces Optimization::Step (optimization.cc:39-97) for B problems in lock-step.  Warm start
 * (shift of the previous solution, optimization.cc:50-57) is used when the handle holds one, else
 * the sinusoid cold start (optimization.cc:58-68).  Asynchronous on `stream` (a hipStream_t, NULL
 * = the default stream); all pointers must stay valid until the stream reaches this point. */
int cpmpc_step_batch(cpmpc_solver* s, int64_t B, const cpmpc_step_inputs* in,
                     const cpmpc_step_outputs* out, void* stream);

/* Replaces Optimization::Reset (optimization.hpp:83). */
int cpmpc_reset(cpmpc_solver* s);
/* Replaces Optimization::SetPreviousSolution (optimization.hpp:86-89); z is [dim][B]. */
int cpmpc_set_previous_solution(cpmpc_solver* s, int64_t B, const void* z, void* stream);
/* Reads the warm-start state (the reference exposes it as OptimizationOutputs::previous_solution
 * of the NEXT step, optimization.cc:84); z_out is [dim][B]. */
int cpmpc_get_solution(cpmpc_solver* s, int64_t B, void* z_out, void* stream);
int cpmpc_has_previous_solution(const cpmpc_solver* s);
/* Warm-start state is per problem, as one Optimization object per controller is in the reference
 * (optimization.cc:46-68: a controller without a previous solution starts from the sinusoid guess): problems
 * [0, n) hold a previous solution, n = the largest B stepped or set since the last cpmpc_reset; a later step with a
 * larger B warm-starts those and cold-starts the rest. */
int64_t cpmpc_previous_solution_batch(const cpmpc_solver* s);

int cpmpc_dim(const cpmpc_solver* s);        /* 4*S + N (optimization.cc:204-205) */
int cpmpc_num_states(const cpmpc_solver* s); /* OptimizationParams::NumStates (optimization.hpp:52) */
int cpmpc_dtype(const cpmpc_solver* s);

/* Host-pointer convenience used by the C++ facade (cart-pole-mpc_amd/host): same semantics as
 * cpmpc_step_batch with HOST double arrays in the same SoA layouts; copies in, runs on the GPU,
 * copies out, synchronises.  There is no CPU compute path behind it. */
int cpmpc_step_batch_host(cpmpc_solver* s, int64_t B, const double* x0_host,
                          const double* dyn_shared_host, double set_point, double* u_host,
                          double* predicted_host, int32_t* status_host, int32_t* iterations_host,
                          double* final_cost_host, double* final_eq_l1_host);
/* The same with the outputs in a struct of HOST pointers (every one nullable), including the solution z, so that
 * Optimization::Step (which also keeps previous_solution_, optimization.cc:85) is ONE round trip: one copy in, the
 * kernels, one copy out, one synchronisation, on the handle's own stream and pinned staging. */
typedef struct cpmpc_step_host_outputs {
  double* u;             /* [N][B] */
  double* predicted;     /* [N][4][B] */
  int32_t* status;       /* [B] */
  int32_t* iterations;   /* [B] */
  double* final_cost;    /* [B] */
  double* final_eq_l1;   /* [B] */
  double* solution;      /* [dim][B] */
} cpmpc_step_host_outputs;
int cpmpc_step_batch_host_ex(cpmpc_solver* s, int64_t B, const double* x0_host, const double* dyn_shared_host,
                             double set_point, const cpmpc_step_host_outputs* out);
/* The general form: cpmpc_step_inputs with HOST double arrays, including the per-problem parameters, set-points and
 * terminal rows (optimization.cc:236-267).  Exactly one of dyn_shared / dyn must be non-NULL. */
typedef struct cpmpc_step_host_inputs {
  const double* x0;               /* [4][B] */
  const double* dyn_shared;       /* [9] shared by the batch, or NULL */
  const double* dyn;              /* [9][B] per problem, or NULL */
  double set_point_shared;        /* used if set_point is NULL */
  const double* set_point;        /* [B] or NULL */
  const double* terminal_weights; /* [4][B] (>= 0 cost row, < 0 equality row) or NULL */
} cpmpc_step_host_inputs;
int cpmpc_step_batch_host_in(cpmpc_solver* s, int64_t B, const cpmpc_step_host_inputs* in,
                             const cpmpc_step_host_outputs* out);
/* How the host-pointer calls run (round 4).  A step of more than 1.5 x `problems` problems is split into chunks that
 * rotate through three staging slots on three streams: while the CPU scatters chunk k's results into the caller's arrays
 * (on the library's worker threads; CPMPC_HOST_THREADS, default 8), chunk k+1 is copying back and chunk k+2 is in the
 * kernels.  Results are bitwise those of the unsplit call (a problem's arithmetic does not depend on its neighbours).
 * -1 (default): eight chunks of at least 16 384 problems (sixteen of at least 8 192 when the results go by DMA into
 * pinned caller arrays); 0 = never split.  Measured at B = 262 144, fp64: see INTEGRATION.md section 4. */
int cpmpc_set_host_chunk(cpmpc_solver* s, int64_t problems);
/* Pin a host array the caller keeps (page-locks it and maps it for DMA: hipHostRegister).  When a CPMPC_F64 handle's
 * host-pointer step asks for the predicted states and its real-typed output arrays (u, predicted, solution) are all
 * pinned -- by this call, hipHostMalloc or hipHostRegister -- the results are copied by DMA straight into them and no CPU
 * pass over the data remains.  The array must stay allocated until cpmpc_host_unregister. */
int cpmpc_host_register(void* ptr, uint64_t bytes);
int cpmpc_host_unregister(void* ptr);
int cpmpc_set_previous_solution_host(cpmpc_solver* s, int64_t B, const double* z_host);
int cpmpc_get_solution_host(cpmpc_solver* s, int64_t B, double* z_host);

/* ---- pieces of the path, exposed for callers and for parity tests ----------------------------- */

/* gen::single_pendulum_dynamics (single_pendulum_dynamics.hpp:13-186), batched.
 * fext_host = {f_base.x, f_base.y, f_mass.x, f_mass.y} shared, NULL = zero.
 * f [4][B]; Jx [16][B] row-major 4x4, nullable; Ju [4][B], nullable. */
int cpmpc_dynamics_batch(int dtype, int64_t B, const double* dyn_shared_host, const void* x,
                         const void* u, const double* fext_host, void* f, void* Jx, void* Ju,
                         void* stream);

/* runge_kutta_4th_order<4> (integration.hpp:13-49) when A/Bm are given, else
 * runge_kutta_4th_order_no_jacobians<4> (integration.hpp:52-62).  A [16][B], Bm [4][B]. */
int cpmpc_rk4_batch(int dtype, int64_t B, const double* dyn_shared_host, const void* x,
                    const void* u, double h, const double* fext_host, void* x_new, void* A,
                    void* Bm, void* stream);

/* The shooting constraints of BuildProblem (optimization.cc:99-160,208-225) linearised at z:
 * defect c [4*(S-1)][B], Phi [16*(S-1)][B] (row-major 4x4 per interval), Gamma [4*N][B]
 * (element (r, k) at field 4*k + r).  Runs the same kernel cpmpc_step_batch runs. */
int cpmpc_linearize_batch(cpmpc_solver* s, int64_t B, const double* dyn_shared_host, const void* z,
                          void* c, void* Phi, void* Gamma, void* stream);

/* Simulator::Step (simulator.cc:11-36), batched: state [4][B] in/out, u [B];
 * fext_host shared {f_base.x, f_base.y, f_mass.x, f_mass.y} or NULL; fext [4][B] per-problem or
 * NULL (takes precedence).  dt < 0 or non-finite -> CPMPC_ERR_INVALID_ARG (simulator.cc:13). */
int cpmpc_sim_step_batch(int dtype, int64_t B, const double* dyn_shared_host, double dt,
                         const void* u, const double* fext_host, const void* fext, void* state,
                         void* stream);

/* ---- models ----------------------------------------------------------------------------------- */
/* CPMPC_MODEL_SINGLE: the reference's cart + single pole (4 states, 9 parameters), everything above.
 * CPMPC_MODEL_DOUBLE: cart + double pole of symbolic/dynamics_double.py:25-148 (BASELINE config 5):
 *   state {b_x, th_1, th_2, b_x', th_1', th_2'} (6), parameters {m_b, m_1, m_2, l_1, l_2, g} (6), no
 *   dissipation / external forces.  The reference has no optimizer for it (optimization.cc:197-199
 *   hard-codes 4 states); here the same OptimizationParams apply with th_final / th_dot_final acting on
 *   both poles and both poles' targets upright, variables laid out by MapKey<6>.
 * With a model argument every array's leading extent 4 becomes the model's state dimension and the
 * parameter vector its parameter count. */
enum { CPMPC_MODEL_SINGLE = 0, CPMPC_MODEL_DOUBLE = 1 };
int cpmpc_model_state_dim(int model);  /* 4 or 6; -1 for an unknown model */
int cpmpc_model_num_params(int model); /* 9 or 6 */
int cpmpc_create_model(const cpmpc_params* params, const cpmpc_solver_opts* opts /*nullable*/, int dtype,
                       int64_t max_batch, int device, int model, cpmpc_solver** out);
int cpmpc_model(const cpmpc_solver* s);
int cpmpc_dynamics_batch_model(int model, int dtype, int64_t B, const double* dyn_shared_host, const void* x,
                               const void* u, const double* fext_host, void* f, void* Jx, void* Ju,
                               void* stream);
int cpmpc_rk4_batch_model(int model, int dtype, int64_t B, const double* dyn_shared_host, const void* x,
                          const void* u, double h, const double* fext_host, void* x_new, void* A, void* Bm,
                          void* stream);
int cpmpc_sim_step_batch_model(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                               const void* u, const double* fext_host, const void* fext, void* state,
                               void* stream);

/* Host-pointer convenience for Simulator::Step (fp64 on the GPU; used by the C++ facade):
 * state_host [4][B] in/out, u_host [B], fext_host shared or NULL.  No CPU compute path. */
int cpmpc_sim_step_batch_host(int64_t B, const double* dyn_shared_host, double dt,
                              const double* u_host, const double* fext_host, double* state_host);

/* ---- the plant step with its first derivatives ----------------------------------------------------------------- */
/* Simulator::Step as cpmpc_sim_step_batch_model runs it -- the same sub-steps (1 ms, a shorter last one), the control held,
 * the pole angles wrapped after each -- from a state that is only READ, together with
 *     A = dx+/dx  [NX*NX][B] (element (r, c) at field r*NX + c, as cpmpc_rk4_batch)   and   Bu = dx+/du  [NX][B]
 * of the whole step: A <- A_i A, Bu <- A_i Bu + B_i over the sub-steps' RK4 Jacobians A_i, B_i (external forces included;
 * the wrap has unit derivative), accumulated in registers whatever the number of sub-steps.  With a cotangent gbar [NX][B]
 * on x+ the call returns gx = A^T gbar [NX][B] and gu = Bu . gbar [B] instead of, or beside, the matrices; A is then never
 * written to memory.  Every output is nullable, only those given are computed, at least one must be given; gx and gu need
 * gbar, and gbar needs one of them.  x_new, A and gx must not alias state or gbar.  Each output is bitwise the same
 * whichever others are asked for with it; x_new agrees with cpmpc_sim_step_batch_model's to rounding, not bitwise (the
 * step that also forms the Jacobians is compiled separately).  dt = 0: x_new = state, A = I, Bu = 0, gx = gbar, gu = 0.
 * A problem with a non-finite state has non-finite outputs; no other problem is affected.
 * What this call does NOT differentiate: the dynamics parameters (cpmpc_sim_step_param_jac_batch below does), the
 * external forces and dt.
 * Device pointers in `dtype`; asynchronous on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite,
 * a wrong struct_size and the pointer rules above -> CPMPC_ERR_INVALID_ARG, before any device is needed. */
typedef struct cpmpc_sim_jac {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_jac) */
  const void* state;      /* [NX][B], read only */
  const void* u;          /* [B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  void* x_new;            /* [NX][B] or NULL */
  void* A;                /* [NX*NX][B] or NULL */
  void* Bu;               /* [NX][B] or NULL */
  const void* gbar;       /* [NX][B] or NULL */
  void* gx;               /* [NX][B] or NULL; needs gbar */
  void* gu;               /* [B] or NULL; needs gbar */
} cpmpc_sim_jac;
int cpmpc_sim_step_jac_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                             const cpmpc_sim_jac* a, void* stream);
/* A and Bu of the same step with HOST doubles (fp64 on the GPU; synchronous; used by the C++ facade,
 * pendulum::Simulator::StepJacobian): state_host [NX][B] read only, u_host [B], fext_host shared or NULL, A_host
 * [NX*NX][B] and Bu_host [NX][B], at least one of them given. */
int cpmpc_sim_step_jac_batch_host(int model, int64_t B, const double* dyn_shared_host, double dt,
                                  const double* state_host, const double* u_host, const double* fext_host,
                                  double* A_host /*nullable*/, double* Bu_host /*nullable*/);

/* ---- per-problem plant parameters, and the plant step's derivative in them ------------------------------------- */
/* cpmpc_sim_step_batch_model with per-problem dynamics parameters: dyn [NP][B] on the device in `dtype` (NULL: the shared
 * host set dyn_shared_host, and then the call IS cpmpc_sim_step_batch_model, bitwise -- the same kernel); dyn takes
 * precedence where both are given, and one of them must be.  A lane's constants are folded from its parameters in the
 * kernel, in `dtype`, as the solver's per-problem dyn are.  state [NX][B] in/out. */
int cpmpc_sim_step_dyn_batch(int model, int dtype, int64_t B, const double* dyn_shared_host,
                             const void* dyn /*[NP][B] device, nullable, takes precedence*/, double dt, const void* u,
                             const double* fext_host, const void* fext, void* state, void* stream);

/* The plant step of cpmpc_sim_step_jac_batch -- the same sub-steps, from a state that is only READ -- with its derivative in
 * the DYNAMICS PARAMETERS,
 *     P = dx+/dp  [NX*NP][B]  (element (r, j) at field r*NP + j),
 * p = {m_b, m_1, l_1, g, mu_b, v_mu_b, c_d_1, x_s, k_s} (NP = 9) for the 4-state model and {m_b, m_1, m_2, l_1, l_2, g}
 * (NP = 6) for the 6-state one.  Only first derivatives of the accelerations enter (da/dp beside da/dx): each column of P
 * is a tangent carried through the RK4 stages of every sub-step, the control and the external forces held, the wrap with
 * unit derivative.  v_mu_b enters through max(v_mu_b, 1e-6): its column is 0 where the clamp is active; the x_s and k_s
 * columns are exactly 0 for a problem that stays off the bumpers.  With a cotangent gbar [NX][B] on x+ the call returns
 * gp = P^T gbar [NP][B] -- P is then never written to memory -- and, for the same cotangent, gx = A^T gbar [NX][B] and
 * gu = Bu . gbar [B] as cpmpc_sim_step_jac_batch does (they are here because cpmpc_sim_jac has no dyn; with dyn == NULL
 * they are bitwise that call's).  dyn [NP][B]: per-problem parameters (NULL: dyn_shared_host, which must be given then).
 * Every output is nullable, only those given are computed, at least one must be given; gp, gx and gu need gbar, and gbar
 * needs one of them.  No output may overlap state, gbar or dyn.  Each output is bitwise the same whichever others are asked
 * for with it.  dt = 0: x_new = state, P = 0, gp = 0, gx = gbar, gu = 0.  A problem with a non-finite state or parameter has
 * non-finite outputs; no other problem is affected.  x_new, P and gp come from one kernel launch (the parameter columns are
 * computed in compile-time groups, one launch per group, and one group holds them all), gx / gu from the kernel of
 * cpmpc_sim_step_jac_batch: a call is at most two launches on `stream`, no host synchronisation, no allocation.
 * What is NOT differentiated: the external forces and dt; and nothing of the CONTROLLER in p (that needs second derivatives
 * of the dynamics).  dt < 0 or non-finite, a wrong struct_size and the pointer rules above -> CPMPC_ERR_INVALID_ARG, before
 * any device is needed. */
typedef struct cpmpc_sim_param_jac {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_param_jac) */
  const void* state;      /* [NX][B], read only */
  const void* u;          /* [B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  void* x_new;            /* [NX][B] or NULL */
  void* P;                /* [NX*NP][B] or NULL */
  const void* gbar;       /* [NX][B] or NULL */
  void* gp;               /* [NP][B] or NULL; needs gbar */
  void* gx;               /* [NX][B] or NULL; needs gbar */
  void* gu;               /* [B] or NULL; needs gbar */
} cpmpc_sim_param_jac;
int cpmpc_sim_step_param_jac_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt,
                                   const cpmpc_sim_param_jac* a, void* stream);
/* P (and optionally x+) of the same step with HOST doubles and the shared parameter set (fp64 on the GPU; synchronous; used
 * by the C++ facade, pendulum::Simulator::StepParamJacobian): state_host [NX][B] read only, u_host [B], fext_host shared or
 * NULL, P_host [NX*NP][B], x_new_host [NX][B] or NULL. */
int cpmpc_sim_step_param_jac_batch_host(int model, int64_t B, const double* dyn_shared_host, double dt,
                                        const double* state_host, const double* u_host, const double* fext_host,
                                        double* P_host, double* x_new_host /*nullable*/);

/* ---- the plant over T ticks in one launch, and its adjoint in one launch ---------------------------------------- */
/* x_{t+1} = Step(x_t, u_t, dt) for t = 0 .. T-1, Step being cpmpc_sim_step_dyn_batch's -- the same sub-steps, the control
 * u [T][B] held over its tick, the pole angles wrapped after each sub-step; dt, the external forces and the parameters
 * (dyn [NP][B], or dyn_shared_host where dyn is NULL; one of them must be given) are those of every tick.  x0 is only
 * READ.  xs [T][NX][B] receives x_{t+1} at field t*NX + r, x_final [NX][B] receives x_T; each is nullable, at least one must
 * be given, and each is bitwise the same whether or not the other is asked for.  A tick runs the plant step's own code:
 * xs[t] is what t + 1 cpmpc_sim_step_dyn_batch calls leave.  dt = 0: every xs[t] and x_final are x0.  No output may overlap
 * x0, u, fext or dyn.  A problem with non-finite data has non-finite outputs; no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1,
 * a wrong struct_size and the pointer rules above -> CPMPC_ERR_INVALID_ARG, before any device is needed. */
typedef struct cpmpc_sim_rollout {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_rollout) */
  const void* x0;         /* [NX][B], read only */
  const void* u;          /* [T][B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  void* xs;               /* [T][NX][B] or NULL */
  void* x_final;          /* [NX][B] or NULL */
} cpmpc_sim_rollout;
int cpmpc_sim_rollout_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                            const cpmpc_sim_rollout* a, void* stream);

/* The adjoint of that rollout: cotangents gbar [T][NX][B] on every x_{t+1} and / or gbar_final [NX][B] on x_T (at least one
 * must be given) pulled back to x0, to the T controls and to the parameters,
 *     g_x0 [NX][B],   g_u [T][B],   g_p [NP][B]
 * (g_p per problem, also where the parameters are the shared set: sum over the batch for its gradient).  Reverse over the
 * ticks, forward inside a tick: from the last tick down to the first the kernel adds the tick's cotangent to lambda, takes
 * x_t from x0 (t = 0) or from row t-1 of xs -- a cpmpc_sim_rollout_batch call's, required when T > 1; row T-1 is never read
 * -- forms the tick's A and Bu as cpmpc_sim_step_jac_batch does and its P as cpmpc_sim_step_param_jac_batch does, and
 * contracts them with lambda in registers: g_u[t] = Bu . lambda, g_p += P^T lambda, lambda <- A^T lambda.  Nothing per
 * sub-step or per tick is stored.  Every output is nullable, only those given are computed, at least one must be given, and
 * each is bitwise the same whichever others are asked for.  dt = 0: g_x0 is the cotangents added up (gbar[T-1], gbar_final,
 * gbar[T-2], ...), g_u = 0, g_p = 0.  No output may overlap x0, u, fext, dyn, xs, gbar or gbar_final.
 * What is NOT differentiated: the external forces and dt; the wrap of the pole angles has unit derivative.  A problem with
 * non-finite data has non-finite outputs; no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1,
 * a wrong struct_size and the pointer rules above -> CPMPC_ERR_INVALID_ARG, before any device is needed. */
typedef struct cpmpc_sim_rollout_vjp {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_rollout_vjp) */
  const void* x0;         /* [NX][B], read only */
  const void* u;          /* [T][B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* xs;         /* [T][NX][B]: a forward call's; required when T > 1 */
  const void* gbar;       /* [T][NX][B] or NULL */
  const void* gbar_final; /* [NX][B] or NULL */
  void* g_x0;             /* [NX][B] or NULL */
  void* g_u;              /* [T][B] or NULL */
  void* g_p;              /* [NP][B] or NULL */
} cpmpc_sim_rollout_vjp;
int cpmpc_sim_rollout_vjp_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                const cpmpc_sim_rollout_vjp* a, void* stream);

/* The FORWARD mode of that rollout in the parameters, and the Gauss-Newton normal equations of an output-error fit of the
 * window to a recording x_obs [T][NX][B] (x_obs[t] is the recorded x_{t+1}), in one launch.  With S_t = dx_t/dp, S_0 = 0,
 *     S_{t+1} = A_t S_t + P_t                        (A_t, P_t the tick's, as cpmpc_sim_step_jac_batch / ..._param_jac_batch)
 *     r_t     = wrap(x_obs[t] - x_{t+1}),   om_t = tick_w ? tick_w[t] : 1,   W = diag(w_host), ones where w_host is NULL
 *     cost [B]        = 1/2 sum_t om_t r_t^T W r_t
 *     g    [NP][B]    = -sum_t om_t S_{t+1}^T W r_t
 *     H    [NP*NP][B] =  sum_t om_t S_{t+1}^T W S_{t+1}     (full and exactly symmetric: field j*NP + k)
 *     S_final [NX*NP][B] = dx_T/dp, element (r, j) at field r*NP + j as P;   x_final [NX][B] = x_T.
 * SIGN CONVENTION: g = dcost/dp, H is the Gauss-Newton approximation of d2cost/dp2, and the Gauss-Newton step is -H^-1 g.
 * No A_t is formed and S never goes to memory: the tick's tangent propagation starts from the tangents the last tick left.
 * A weight of 0 in w_host says that state was not measured, a tick weight of 0 that the sample is missing; x_obs must still
 * hold finite numbers there.  x_obs is required where cost, g or H is asked for, and not read otherwise.  Every output is
 * nullable, only those given are computed, at least one must be given, and each is bitwise the same whichever others are
 * asked for.  dt = 0: S_final = 0, H = 0, g = 0, x_final = x0 and cost is the weighted residual of x0 against every
 * x_obs[t].  No output may overlap x0, u, fext, dyn, x_obs or tick_w.  What is NOT differentiated: the external forces, dt
 * and x0 (its gradient is cpmpc_sim_rollout_vjp_batch's g_x0); the wrap of the pole angles has unit derivative.  A problem
 * with non-finite data has non-finite outputs; no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1,
 * a wrong struct_size, a negative or non-finite w_host entry and the pointer rules above -> CPMPC_ERR_INVALID_ARG, before
 * any device is needed. */
typedef struct cpmpc_sim_rollout_gn {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_rollout_gn) */
  const void* x0;         /* [NX][B], read only */
  const void* u;          /* [T][B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* x_obs;      /* [T][NX][B] the recorded x_{t+1}; required where cost, g or H is asked for */
  const double* w_host;   /* NX residual weights >= 0, or NULL: ones (zeros = that state was not measured) */
  const void* tick_w;     /* [T][B] per-sample weights or NULL: ones (0 = that sample is missing) */
  void* cost;             /* [B] or NULL */
  void* g;                /* [NP][B] or NULL */
  void* H;                /* [NP*NP][B] or NULL */
  void* S_final;          /* [NX*NP][B] or NULL */
  void* x_final;          /* [NX][B] or NULL */
} cpmpc_sim_rollout_gn;
int cpmpc_sim_rollout_gn_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                               const cpmpc_sim_rollout_gn* a, void* stream);

/* The FORWARD mode of that rollout in the INITIAL STATE, and the Gauss-Newton normal equations of an output-error fit of x0
 * to a recording x_obs [T][NX][B] (x_obs[t] is the recorded x_{t+1}), in one launch: the state-estimation half of the call
 * above.  With Phi_t = dx_t/dx0, Phi_0 = I,
 *     Phi_{t+1} = A_t Phi_t                          (A_t the tick's dx_{t+1}/dx_t, as cpmpc_sim_step_jac_batch's A)
 *     r_t     = wrap(x_obs[t] - x_{t+1}),   om_t = tick_w ? tick_w[t] : 1,   W = diag(w_host), ones where w_host is NULL
 *     cost [B]        = 1/2 sum_t om_t r_t^T W r_t
 *     g    [NX][B]    = -sum_t om_t Phi_{t+1}^T W r_t
 *     H    [NX*NX][B] =  sum_t om_t Phi_{t+1}^T W Phi_{t+1} (full and exactly symmetric: field j*NX + k)
 *     Phi_final [NX*NX][B] = dx_T/dx0, element (r, c) at field r*NX + c as A;   x_final [NX][B] = x_T.
 * SIGN CONVENTION: g = dcost/dx0, H is the Gauss-Newton approximation of d2cost/dx0^2, and the Gauss-Newton step is
 * -H^-1 g.  No A_t is formed and Phi never goes to memory: the tick's tangent propagation starts from the tangents the last
 * tick left; the columns of Phi that are known in closed form are neither stored nor propagated.
 * A weight of 0 in w_host says that state was not measured (positions only: 1, 1, 0, 0), a tick weight of 0 that the sample
 * is missing; x_obs must still hold finite numbers there.  x_obs is required where cost, g or H is asked for, and not read
 * otherwise.  Every output is nullable, only those given are computed, at least one must be given, and each is bitwise the
 * same whichever others are asked for.  dt = 0: Phi_final = I, x_final = x0, H = sum_t om_t W, g = -sum_t om_t W r_t.
 * No output may overlap x0, u, fext, dyn, x_obs or tick_w.  What is NOT differentiated: the parameters
 * (cpmpc_sim_rollout_gn_batch), the external forces and dt; the wrap of the pole angles has unit derivative.  A problem with
 * non-finite data has non-finite outputs; no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1,
 * a wrong struct_size, a negative or non-finite w_host entry and the pointer rules above -> CPMPC_ERR_INVALID_ARG, before
 * any device is needed. */
typedef struct cpmpc_sim_rollout_gn_x0 {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_rollout_gn_x0) */
  const void* x0;         /* [NX][B], read only: the point the fit is linearised at */
  const void* u;          /* [T][B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* x_obs;      /* [T][NX][B] the recorded x_{t+1}; required where cost, g or H is asked for */
  const double* w_host;   /* NX residual weights >= 0, or NULL: ones (zeros = that state was not measured) */
  const void* tick_w;     /* [T][B] per-sample weights or NULL: ones (0 = that sample is missing) */
  void* cost;             /* [B] or NULL */
  void* g;                /* [NX][B] or NULL */
  void* H;                /* [NX*NX][B] or NULL */
  void* Phi_final;        /* [NX*NX][B] or NULL */
  void* x_final;          /* [NX][B] or NULL */
} cpmpc_sim_rollout_gn_x0;
int cpmpc_sim_rollout_gn_x0_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                  const cpmpc_sim_rollout_gn_x0* a, void* stream);

/* The EXTENDED KALMAN FILTER of B plants over T ticks in one launch: the recursive counterpart of the call above.  From the
 * state x0 [NX][B] and its covariance P0 [NX*NX][B] (element (j, k) at field j*NX + k; ONLY THE LOWER TRIANGLE, k <= j, IS
 * READ), per tick t = 0 .. T-1
 *     predict   x- = Step(x, u[t], dt),   P- = A_t P A_t^T + diag(q_host)      (A_t the tick's dx+/dx at the filtered x,
 *                                                                               as cpmpc_sim_step_jac_batch's A)
 *     update    for every state i in index order with rho_i = om_t w_host[i] > 0,  om_t = tick_w ? tick_w[t] : 1:
 *                   s = P_ii + 1/rho_i,   nu = wrap_i(y[t][i] - x_i),   K = P[:, i] / s
 *                   x += K nu,   P -= K P[i, :],   nis += nu^2 / s
 *               then the pole angles of x are wrapped (where an update acted).
 * w_host are the INVERSE VARIANCES of the measurement y [T][NX][B] (y[t] is the measured x_{t+1}), the convention of the
 * weights of cpmpc_sim_rollout_gn_x0_batch; NULL: ones.  A weight of 0 says that state is not measured (positions only with
 * 0.01 rms noise: 1e4, 1e4, 0, 0), a tick weight of 0 that the sample is missing: there x and P stay bitwise what the
 * prediction left and y is not read.  q_host are NX process-noise VARIANCES >= 0, added to P's diagonal once a tick; NULL:
 * zeros.  The measurement covariance is diagonal, so the scalar updates in sequence ARE the joint update; no matrix is
 * inverted.  The tick's A stays in registers and the covariance on the device: nothing per tick goes to memory but xs.
 *     x_final [NX][B], P_final [NX*NX][B] (full and exactly symmetric), xs [T][NX][B] the filtered state after every
 *     tick, nis [B] the normalised squared innovations added up (about one per scalar measurement where q and w are
 *     consistent with the data; far more where a sensor has failed).
 * Every output is nullable, only those given are stored, at least one must be given, and each is bitwise the same
 * whichever others are asked for.  T = 1 is the per-tick filter (x_final and P_final may be handed back as the next call's
 * x0 and P0) and the arrival-cost update of a moving horizon.  y is required where some w_host[i] > 0.  dt = 0: A = I, the
 * linear Kalman filter of a constant state.  No output may overlap x0, P0, u, fext, dyn, y or tick_w.  A problem with
 * non-finite data has non-finite outputs; no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1,
 * a wrong struct_size, a negative or non-finite w_host or q_host entry and the pointer rules above -> CPMPC_ERR_INVALID_ARG,
 * before any device is needed. */
typedef struct cpmpc_sim_ekf {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_ekf) */
  const void* x0;         /* [NX][B], read only: the filtered state before the first tick */
  const void* P0;         /* [NX*NX][B], read only: its covariance; the lower triangle is read */
  const void* u;          /* [T][B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* y;          /* [T][NX][B] the measured x_{t+1}; required where some w_host[i] > 0 */
  const void* tick_w;     /* [T][B] per-sample weights or NULL: ones (0 = that sample is missing) */
  const double* w_host;   /* NX inverse variances of the measurement >= 0, or NULL: ones (0 = not measured) */
  const double* q_host;   /* NX process-noise variances >= 0 added once a tick, or NULL: zeros */
  void* x_final;          /* [NX][B] or NULL */
  void* P_final;          /* [NX*NX][B] or NULL */
  void* xs;               /* [T][NX][B] or NULL */
  void* nis;              /* [B] or NULL */
} cpmpc_sim_ekf;
int cpmpc_sim_ekf_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                        const cpmpc_sim_ekf* a, void* stream);

/* The RAUCH-TUNG-STRIEBEL SMOOTHER of B plants over T ticks: every state of the window given ALL of the window's measurements,
 * with its covariance.  Forward it is the filter above, unchanged; state index 0 is x0 / P0 and index t is after tick t.  With
 * x-_{t+1}, P-_{t+1} the prediction of tick t before its update and A_t its dx+/dx, backward from x^s_T = x_T, P^s_T = P_T
 *     for t = T-1 .. 0:
 *         G_t   = P_t A_t^T (P-_{t+1})^-1
 *         d     = wrap(x^s_{t+1} - x-_{t+1})                    pole angles to the nearest turn
 *         x^s_t = x_t + G_t d                                    then the pole angles are wrapped (where G_t d is not zero)
 *         P^s_t = P_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T         exactly symmetric
 * No inverse is formed: the rows of G_t come from the Cholesky factor of the diagonally scaled P-_{t+1}.  A tick whose P- is NOT
 * POSITIVE DEFINITE (a diagonal entry not positive, or a pivot of the scaled matrix not above 8 NX eps or not finite) takes
 * G_t = 0: index t's smoothed values are its filtered ones, the recursion goes on from them, and the problem's ok is 0.  That
 * is the answer for P0 = 0 (the start is known).
 * The inputs are cpmpc_sim_ekf's, with the same meaning, and a WORKSPACE `work` of work_rows rows of B numbers in `dtype`,
 * work_rows >= cpmpc_sim_rts_work_rows(model, T) = T (2 NX + 2 NH + NX^2), NH = NX (NX + 1) / 2: 44 T rows for the 4-state
 * model, 90 T for the 6-state model.  The forward pass stores there per tick x-, P-, A_t P_t and the filtered x and P; its
 * contents after the call are not specified.
 *     x_final, P_final, xs, nis: the filter's, bitwise cpmpc_sim_ekf_batch's on the same inputs;
 *     xs_smooth [T+1][NX][B], Ps_smooth [T+1][NX*NX][B] (full and exactly symmetric): index T is x_final / P_final;
 *     x0_smooth [NX][B], P0_smooth [NX*NX][B]: index 0 alone, for callers that want only the window's first state;
 *     ok [B] int32: 1 where every tick's P- was positive definite.
 * Every output is nullable, at least one must be given, and each is bitwise the same whichever others are asked for.  No
 * output may overlap an input, and work may overlap nothing.  A problem with non-finite data has non-finite outputs and
 * ok = 0; no other problem is affected.
 * Device pointers in `dtype`; TWO launches on `stream` (one where only the filter's outputs are asked for), no host
 * synchronisation, no allocation.  The rules of cpmpc_sim_ekf_batch, work == NULL, work_rows too small and the pointer rules
 * above -> CPMPC_ERR_INVALID_ARG, before any device is needed. */
typedef struct cpmpc_sim_rts {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_rts) */
  const void* x0;         /* [NX][B], read only: the filtered state before the first tick */
  const void* P0;         /* [NX*NX][B], read only: its covariance; the lower triangle is read */
  const void* u;          /* [T][B] */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* y;          /* [T][NX][B] the measured x_{t+1}; required where some w_host[i] > 0 */
  const void* tick_w;     /* [T][B] per-sample weights or NULL: ones (0 = that sample is missing) */
  const double* w_host;   /* NX inverse variances of the measurement >= 0, or NULL: ones (0 = not measured) */
  const double* q_host;   /* NX process-noise variances >= 0 added once a tick, or NULL: zeros */
  void* work;             /* [work_rows][B] workspace, required */
  int64_t work_rows;      /* >= cpmpc_sim_rts_work_rows(model, T) */
  void* x_final;          /* [NX][B] or NULL */
  void* P_final;          /* [NX*NX][B] or NULL */
  void* xs;               /* [T][NX][B] or NULL */
  void* nis;              /* [B] or NULL */
  void* xs_smooth;        /* [T+1][NX][B] or NULL */
  void* Ps_smooth;        /* [T+1][NX*NX][B] or NULL */
  void* x0_smooth;        /* [NX][B] or NULL */
  void* P0_smooth;        /* [NX*NX][B] or NULL */
  int32_t* ok;            /* [B] or NULL */
} cpmpc_sim_rts;
/* rows of B numbers of cpmpc_sim_rts.work for T ticks of `model`; 0 for an unknown model or T < 1 */
int64_t cpmpc_sim_rts_work_rows(int model, int T);
int cpmpc_sim_rts_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                        const cpmpc_sim_rts* a, void* stream);

/* ---- tracking a plant trajectory between two re-plans: its LQR gains, and the plant under them, one launch each ---- */
/* The TIME-VARYING LQR GAINS along a plant trajectory in one launch: the backward Riccati recursion of the cost
 *     sum_{t<T} (d_t^T diag(q_host) d_t + r du_t^2) + d_T^T P_T d_T        d_t = x_t - x_nom_t, du_t = u_t - u_nom[t]
 * linearised along the trajectory x0, u [T][B], xs [T][NX][B] -- a cpmpc_sim_rollout_batch call's on the same inputs,
 * required when T > 1; row T-1 is never read.  The plant has one input, so no matrix is inverted.  Reverse over the ticks,
 * forward inside a tick: with x_t = (t == 0) ? x0 : xs[t-1] and Phi_t = dx+/dx, gamma_t = dx+/du of the tick at (x_t, u[t])
 * as cpmpc_sim_step_jac_batch's A and Bu,
 *     P = P_T
 *     for t = T-1 .. 0:
 *         v   = P gamma_t
 *         s   = r + gamma_t . v
 *         k_t = -(Phi_t^T v) / s
 *         Acl = Phi_t + gamma_t k_t^T
 *         P   = diag(q_host) + r k_t k_t^T + Acl^T P Acl
 *     P0 = P
 * SIGN CONVENTION: K[t] = k_t is applied as u_t = u_nom[t] + k_t . (x_t - x_nom_t) -- what cpmpc_sim_rollout_fb_batch does
 * -- and d^T P0 d is the cost-to-go of a deviation d at the window's start.  The update is the Joseph-like form: a sum of
 * positive semidefinite terms, so P stays positive semidefinite in rounded arithmetic.  Only P's lower triangle is computed.
 * P_T is PT [NX*NX][B] (element (j, k) at field j*NX + k; ONLY THE LOWER TRIANGLE, k <= j, IS READ: a call's P0 chains
 * windows, and T1 + T2 ticks are bitwise the T2-tick tail's P0 given as PT to the T1-tick head), else diag(qf_host), else
 * diag(q_host).  q_host: NX weights >= 0, NULL: ones.  r: finite and > 0.
 *     K [T][NX][B], row t the gain of tick t;   P0 [NX*NX][B], full and exactly symmetric.
 * Each output is nullable, at least one must be given, and each is bitwise the same whether or not the other is asked for.
 * The gains belong to the PLANT's map at dt (its sub-steps of 1 ms, the control held over the tick), not to a controller's
 * model of it.  dt = 0: K = 0 and P0 = P_T + T diag(q_host).  NOT modelled: a clamp of the control, feedback inside a tick,
 * cross terms of the cost.  No output may overlap x0, u, xs, fext, dyn or PT.  A problem with non-finite data has non-finite
 * outputs; no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1,
 * a wrong struct_size, r not finite and > 0, a negative or non-finite q_host or qf_host entry, xs == NULL with T > 1 and the
 * pointer rules above -> CPMPC_ERR_INVALID_ARG, before any device is needed. */
typedef struct cpmpc_sim_lqr {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_lqr) */
  const void* x0;         /* [NX][B], read only: the start of the trajectory */
  const void* u;          /* [T][B] the trajectory's controls */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* xs;         /* [T][NX][B]: a forward call's; required when T > 1 */
  const double* q_host;   /* NX state weights >= 0, or NULL: ones */
  double r;               /* the control weight, finite and > 0 */
  const void* PT;         /* [NX*NX][B] terminal cost or NULL; the lower triangle is read */
  const double* qf_host;  /* NX terminal weights >= 0 used where PT is NULL, or NULL: q_host's */
  void* K;                /* [T][NX][B] or NULL */
  void* P0;               /* [NX*NX][B] or NULL */
} cpmpc_sim_lqr;
int cpmpc_sim_lqr_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                        const cpmpc_sim_lqr* a, void* stream);

/* The plant under an AFFINE FEEDBACK LAW for T ticks in one launch: cpmpc_sim_rollout_batch's loop with the tick's control
 * formed on the device at the tick's start and held over its sub-steps,
 *     d   = wrap(x_t - x_nom_t)                       x_nom_0 = x0_nom, x_nom_t = xs_nom[t-1]; pole angles to the nearest turn
 *     u_t = clamp(u_nom[t] + K[t] . d, +-u_limit)
 *     x_{t+1} = Step(x_t, u_t, dt)
 * SIGN CONVENTION: K [T][NX][B] is cpmpc_sim_lqr_batch's.  K == NULL: no feedback, u_t = clamp(u_nom[t]), and the nominal
 * trajectory is not read.  x0_nom [NX][B] is required where K is given, xs_nom [T][NX][B] also when T > 1; row T-1 of xs_nom
 * is never read.  u_limit > 0; +infinity: no clamp.  The parameters and forces are THE CALL'S OWN and may differ from those
 * the nominal trajectory and the gains were made with (model mismatch).
 *     xs [T][NX][B], x_final [NX][B], us [T][B] the controls applied;
 * each is nullable and at least one must be given; each is bitwise the same whichever others are asked for.  Two identities
 * hold BITWISE: with K == NULL and u_limit = +infinity, xs and x_final are cpmpc_sim_rollout_batch's on u_nom; with
 * x0 == x0_nom, the nominal trajectory's parameters, finite K and non-zero u_nom, d is exactly 0 at every tick and the call
 * reproduces the nominal rollout.  There is NO feedback inside a tick, and cpmpc_sim_lqr_batch does not know of the clamp.
 * No output may overlap x0, u_nom, K, x0_nom, xs_nom, fext or dyn.  A problem with non-finite data has non-finite outputs;
 * no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1,
 * a wrong struct_size, u_limit not > 0, K without x0_nom (or without xs_nom when T > 1) and the pointer rules above ->
 * CPMPC_ERR_INVALID_ARG, before any device is needed. */
typedef struct cpmpc_sim_rollout_fb {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_rollout_fb) */
  const void* x0;         /* [NX][B], read only */
  const void* u_nom;      /* [T][B] the nominal controls */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* K;          /* [T][NX][B] gains or NULL: no feedback */
  const void* x0_nom;     /* [NX][B] the nominal start; required where K is given */
  const void* xs_nom;     /* [T][NX][B] the nominal checkpoints; required where K is given and T > 1 */
  double u_limit;         /* > 0; +infinity: no clamp */
  void* xs;               /* [T][NX][B] or NULL */
  void* x_final;          /* [NX][B] or NULL */
  void* us;               /* [T][B] or NULL */
} cpmpc_sim_rollout_fb;
int cpmpc_sim_rollout_fb_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                               const cpmpc_sim_rollout_fb* a, void* stream);

/* ---- iterative LQR on the plant's own tick map: the backward and the forward pass of one iteration, one launch each ---- */
/* THE COST of both calls, cpmpc_sim_lqr_batch's convention with NO factor 1/2: with e_t = wrap(x_t - xref_t) (pole angles to
 * the nearest turn), x_0 = x0, x_t = xs[t-1], xref_0 = x0_ref, xref_t = xs_ref[t-1] and uref_t = u_ref[t] (NULL: zeros),
 *     J = sum_{t<T} (e_t^T diag(q_host) e_t + r (u_t - uref_t)^2) + e_T^T P_T e_T
 * Row T-1 of xs_ref IS read: it is the terminal target.  P_T is PT [NX*NX][B] (ONLY THE LOWER TRIANGLE, k <= j, IS READ), else
 * diag(qf_host), else diag(q_host).  q_host: NX weights >= 0, NULL: ones.  r: finite and > 0.
 *
 * The BACKWARD PASS along the trajectory x0, u [T][B], xs [T][NX][B] -- a forward call's on the same inputs, required when
 * T > 1; with xs == NULL and T == 1 the call rolls x_1 itself.  Reverse over the ticks, forward inside a tick, Phi_t and
 * gamma_t of the tick at (x_t, u[t]) as cpmpc_sim_step_jac_batch's A and Bu; g is HALF the gradient of the cost-to-go:
 *     P = P_T ;  g = P_T e_T ;  dV1 = dV2 = 0
 *     for t = T-1 .. 0:
 *         v   = P gamma_t ;  s0 = r + gamma_t . v ;  s = s0 + mu              mu [B] >= 0 per problem, NULL: 0
 *         h   = r (u_t - uref_t) + gamma_t . g
 *         k_t = clamp(u_t - h / s, +-u_limit) - u_t
 *         K_t = (the clamp changed u_t - h / s) ? 0 : -(Phi_t^T v) / s
 *         dV1 += 2 k_t h ;  dV2 += k_t^2 s0
 *         Acl = Phi_t + gamma_t K_t^T
 *         g   = q o e_t + r (u_t - uref_t + k_t) K_t + Acl^T (g + v k_t)
 *         P   = diag(q_host) + r K_t K_t^T + Acl^T P Acl
 * The plant has one input, so the box QP of control-limited DDP is the scalar clamp above, solved exactly, and no matrix is
 * inverted.  SIGN CONVENTION: the improved control is u_t + alpha k_t + K_t . wrap(x - x_t), what cpmpc_sim_ilqr_forward_batch
 * applies; alpha dV[0] + alpha^2 dV[1] is the predicted CHANGE of J (negative: a decrease) for a step alpha; x^T P0 x + 2 g0 . x
 * is the model's cost-to-go of a deviation x at the start, up to its constant.  The P and g updates are the cost of the affine
 * policy in the linear-quadratic model and hold for any k_t and K_t: P stays positive semidefinite under mu and under the clamp.
 * With mu == NULL and u_limit = +infinity, K and P0 are cpmpc_sim_lqr_batch's; with the reference equal to the trajectory, kff
 * and dV are exactly 0.
 *     K [T][NX][B];  kff [T][B] the k_t;  dV [2][B] = dV1, dV2;  P0 [NX*NX][B] full and exactly symmetric;  g0 [NX][B];
 *     hmax [B] = max_t |k_t| (s0 + mu), the stationarity measure: 0 where no control would move.
 * Each output is nullable, at least one must be given, and each is bitwise the same whichever others are asked for.
 * dt = 0 (the identity plant, gamma = 0): K = 0, k_t = clamp(u_t - (u_t - uref_t) r / (r + mu)) - u_t, g0 = P_T e_T + sum_t
 * q o e_t, P0 = P_T + T diag(q_host).  NOT modelled: second-order terms of the dynamics (Gauss-Newton, not full DDP), cross
 * terms or a control-rate term of the cost, feedback inside a tick.  u_limit > 0, +infinity: none; the trajectory's controls
 * are expected inside it.  No output may overlap an input array.  A problem with non-finite data has non-finite outputs; no
 * other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1, a
 * wrong struct_size, r not finite and > 0, a negative or non-finite q_host or qf_host entry, u_limit not > 0, xs == NULL with
 * T > 1, x0_ref or xs_ref == NULL, no output, and the pointer rules above -> CPMPC_ERR_INVALID_ARG, before any device is
 * needed. */
typedef struct cpmpc_sim_ilqr_backward {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_ilqr_backward) */
  const void* x0;         /* [NX][B], read only: the start of the trajectory */
  const void* u;          /* [T][B] the trajectory's controls */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* xs;         /* [T][NX][B]: a forward call's; required when T > 1 */
  const void* x0_ref;     /* [NX][B] the target of x0 */
  const void* xs_ref;     /* [T][NX][B] the targets of xs; row T-1 is the terminal target */
  const void* u_ref;      /* [T][B] the controls' targets or NULL: zeros */
  const double* q_host;   /* NX state weights >= 0, or NULL: ones */
  double r;               /* the control weight, finite and > 0 */
  const void* PT;         /* [NX*NX][B] terminal cost or NULL; the lower triangle is read */
  const double* qf_host;  /* NX terminal weights >= 0 used where PT is NULL, or NULL: q_host's */
  const void* mu;         /* [B] regularisation >= 0 added to s, or NULL: none */
  double u_limit;         /* > 0; +infinity: no limit */
  void* K;                /* [T][NX][B] or NULL */
  void* kff;              /* [T][B] or NULL */
  void* dV;               /* [2][B] or NULL */
  void* P0;               /* [NX*NX][B] or NULL */
  void* g0;               /* [NX][B] or NULL */
  void* hmax;             /* [B] or NULL */
} cpmpc_sim_ilqr_backward;
int cpmpc_sim_ilqr_backward_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                  const cpmpc_sim_ilqr_backward* a, void* stream);

/* The FORWARD PASS: cpmpc_sim_rollout_fb_batch's loop with a per-problem step on the feedforward term and the cost J above
 * summed on the device,
 *     d   = wrap(x_t - x_nom_t)                       x_nom_0 = x0_nom, x_nom_t = xs_nom[t-1]; row T-1 of xs_nom is never read
 *     u_t = clamp(u_nom[t] + alpha kff[t] + K[t] . d, +-u_limit)
 *     x_{t+1} = Step(x_t, u_t, dt)
 *     cost = J of (x0, the states passed, the controls applied) against x0_ref, xs_ref, u_ref
 * kff [T][B], K [T][NX][B]: cpmpc_sim_ilqr_backward_batch's, each or NULL (that term is absent); K needs x0_nom, and xs_nom
 * when T > 1.  alpha [B]: a step per problem, a DEVICE array, NULL: 1.  With kff == K == NULL this is the plain clamped rollout
 * with its cost -- how a loop gets its first trajectory -- and with u_limit = +infinity its xs are cpmpc_sim_rollout_batch's
 * bit for bit.  With x0 == x0_nom, the nominal's parameters, alpha = 0 and finite kff, K, the call reproduces the nominal xs
 * and us (a forward call's own) and their cost bit for bit.
 *     xs [T][NX][B], x_final [NX][B], us [T][B] the controls applied, cost [B];
 * each is nullable, at least one must be given, and each is bitwise the same whichever others are asked for.  dt = 0: the
 * state stays, us and cost as written.  There is NO feedback inside a tick.  No output may overlap an input array.  A problem
 * with non-finite data has non-finite outputs; no other problem is affected.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  dt < 0 or non-finite, T < 1, a
 * wrong struct_size, r not finite and > 0, a negative or non-finite q_host or qf_host entry, u_limit not > 0, x0_ref or xs_ref
 * == NULL, K without x0_nom (or without xs_nom when T > 1), no output, and the pointer rules above -> CPMPC_ERR_INVALID_ARG,
 * before any device is needed. */
typedef struct cpmpc_sim_ilqr_forward {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_ilqr_forward) */
  const void* x0;         /* [NX][B], read only */
  const void* u_nom;      /* [T][B] the nominal controls */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* kff;        /* [T][B] feedforward terms or NULL */
  const void* K;          /* [T][NX][B] gains or NULL: no feedback */
  const void* x0_nom;     /* [NX][B] the nominal start; required where K is given */
  const void* xs_nom;     /* [T][NX][B] the nominal checkpoints; required where K is given and T > 1 */
  const void* alpha;      /* [B] the step on kff per problem, or NULL: 1 */
  double u_limit;         /* > 0; +infinity: no clamp */
  const void* x0_ref;     /* [NX][B] the target of x0 */
  const void* xs_ref;     /* [T][NX][B] the targets of xs; row T-1 is the terminal target */
  const void* u_ref;      /* [T][B] the controls' targets or NULL: zeros */
  const double* q_host;   /* NX state weights >= 0, or NULL: ones */
  double r;               /* the control weight, finite and > 0 */
  const void* PT;         /* [NX*NX][B] terminal cost or NULL; the lower triangle is read */
  const double* qf_host;  /* NX terminal weights >= 0 used where PT is NULL, or NULL: q_host's */
  void* xs;               /* [T][NX][B] or NULL */
  void* x_final;          /* [NX][B] or NULL */
  void* us;               /* [T][B] or NULL */
  void* cost;             /* [B] or NULL */
} cpmpc_sim_ilqr_forward;
int cpmpc_sim_ilqr_forward_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                 const cpmpc_sim_ilqr_forward* a, void* stream);

/* The LINE SEARCH of one iteration in ONE launch: every problem walks its own trial ladder on the forward pass above, from the
 * nominal trajectory (x0, u_nom, xs_nom) with cost cost_nom, under cpmpc_sim_ilqr_backward_batch's kff, K (or NULL) and dV.
 * The nominal start is x0 itself -- there is no x0_nom, a line search compares costs from one start:
 *     alpha = 1 ; accepted = false
 *     for j in 0 .. trials-1 while not accepted:
 *         roll T ticks under u_t = clamp(u_nom[t] + alpha kff[t] + K[t] . wrap(x_t - x_nom_t), +-u_limit), summing J_try
 *         pred = dV[0] alpha + dV[1] alpha^2
 *         accepted = pred < 0 and J_try - cost_nom <= armijo pred
 *         if not accepted: alpha = alpha / 2
 *     accepted: xs, us, x_final of that roll ; cost = J_try ; alpha = the step taken
 *     else:     xs = xs_nom, us = u_nom, x_final = xs_nom[T-1], cost = cost_nom, alpha = 0              (a COPY)
 * SIGN CONVENTION of dV: the backward pass's, alpha dV[0] + alpha^2 dV[1] is the predicted CHANGE of J (negative: a decrease);
 * a problem whose prediction is not negative takes no step.  The ladder only halves, so alpha is a power of two, pred is
 * rounded once and the two sides of the test are each rounded on their own: THE DECISIONS ARE THOSE OF THE TRIAL LADDER written
 * with cpmpc_sim_ilqr_forward_batch calls and elementwise arithmetic in `dtype` between them, bit for bit, and an accepted
 * problem's xs, x_final, us and cost are that call's at its alpha, bit for bit.  A problem leaves the ladder when it has
 * decided; one launch costs between one roll (every problem of a wave accepts at once) and `trials` rolls.
 * A FAILED PROBLEM KEEPS ITS NOMINAL BY COPY.  For finite data that is what a forward call with alpha = 0 returns.  It differs
 * on purpose where kff, K or dV of a problem is NOT FINITE while its nominal is finite: a forward call with alpha = 0 would
 * poison the problem through 0 . NaN; the search fails it (alpha = 0) and it keeps its trajectory, for a retry under a larger
 * mu.  A problem whose nominal or cost_nom is itself non-finite returns that.  No other problem is affected.
 *     xs [T][NX][B], x_final [NX][B], us [T][B], cost [B], alpha [B] (0: no step);
 * each is nullable, at least one must be given, and each is bitwise the same whichever others are asked for.  xs_nom is ALWAYS
 * required, for T = 1 too: row T-1 is read for the copy.  xs and us are written during the trials, so NO OUTPUT MAY OVERLAP AN
 * INPUT ARRAY.  dt = 0: the state stays, us and cost as written.
 * Device pointers in `dtype`; ONE launch on `stream`, no host synchronisation, no allocation.  Everything the forward call
 * refuses, and xs_nom, cost_nom, kff or dV == NULL, trials outside 1..32, reserved != 0, armijo not finite or not in (0, 1), no output ->
 * CPMPC_ERR_INVALID_ARG, before any device is needed. */
typedef struct cpmpc_sim_ilqr_search {
  uint64_t struct_size;   /* = sizeof(cpmpc_sim_ilqr_search) */
  const void* x0;         /* [NX][B], read only: the start, of the nominal too */
  const void* u_nom;      /* [T][B] the nominal controls */
  const double* fext_host;/* shared {fb.x, fb.y, fm.x, fm.y} or NULL */
  const void* fext;       /* [4][B] or NULL (takes precedence) */
  const void* dyn;        /* [NP][B] per-problem parameters or NULL (then dyn_shared_host) */
  const void* xs_nom;     /* [T][NX][B] the nominal states; always required */
  const void* cost_nom;   /* [B] the nominal's cost */
  const void* kff;        /* [T][B] feedforward terms */
  const void* K;          /* [T][NX][B] gains or NULL: no feedback */
  const void* dV;         /* [2][B] the predicted change's two coefficients */
  int32_t trials;         /* 1..32 */
  int32_t reserved;       /* must be 0: the padding behind trials, spelled out */
  double armijo;         /* in (0, 1): the share of the prediction a step must reach */
  double u_limit;         /* > 0; +infinity: no clamp */
  const void* x0_ref;     /* [NX][B] the target of x0 */
  const void* xs_ref;     /* [T][NX][B] the targets of xs; row T-1 is the terminal target */
  const void* u_ref;      /* [T][B] the controls' targets or NULL: zeros */
  const double* q_host;   /* NX state weights >= 0, or NULL: ones */
  double r;               /* the control weight, finite and > 0 */
  const void* PT;         /* [NX*NX][B] terminal cost or NULL; the lower triangle is read */
  const double* qf_host;  /* NX terminal weights >= 0 used where PT is NULL, or NULL: q_host's */
  void* xs;               /* [T][NX][B] or NULL */
  void* x_final;          /* [NX][B] or NULL */
  void* us;               /* [T][B] or NULL */
  void* cost;             /* [B] or NULL */
  void* alpha;            /* [B] or NULL */
} cpmpc_sim_ilqr_search;
int cpmpc_sim_ilqr_search_batch(int model, int dtype, int64_t B, const double* dyn_shared_host, double dt, int T,
                                const cpmpc_sim_ilqr_search* a, void* stream);

/* ---- several GPUs from ONE process ------------------------------------------------------------------ */
/* The reference is single-threaded and single-device; a batch of independent controllers shards
 * embarrassingly, so this is new surface: one `cpmpc_sharded` owns one solver handle + one stream per shard, a shard
 * living on one HIP device.  A step splits the batch contiguously (shard i owns columns
 * [i*B/n + min(i, B%n), ...) -- the same rule as cart-pole-mpc_amd/sharding.py: shard_range), runs every shard
 * concurrently, and assembles the outputs in global problem order.  No data-path collective: the only traffic between
 * devices is the scatter of x0 and the gather of the results, point-to-point copies to/from the root device (shard 0's)
 * over xGMI, or through each shard's pinned staging for the host-pointer call.  `devices` may name a device more than
 * once (two shards on one GPU: how the tests run it on a one-GPU box; results are bitwise those of one handle).
 * pendulum::ShardedOptimization (cart-pole-mpc_amd/host/sharded_optimization.hpp) is the C++ class over it. */
typedef struct cpmpc_sharded cpmpc_sharded;
/* devices == NULL: every visible gfx950 device, one shard each (n_devices ignored).  max_batch is the TOTAL batch. */
int cpmpc_sharded_create(const cpmpc_params* params, const cpmpc_solver_opts* opts /*nullable*/, int dtype,
                         int64_t max_batch, const int* devices, int n_devices, cpmpc_sharded** out);
/* the same from a cpmpc_create_info (its `device` is ignored, its max_batch is the TOTAL batch): any model, creation flags */
int cpmpc_sharded_create_ex(const cpmpc_create_info* info, const int* devices, int n_devices, cpmpc_sharded** out);
void cpmpc_sharded_destroy(cpmpc_sharded* s);
int cpmpc_sharded_num_shards(const cpmpc_sharded* s);
int cpmpc_sharded_device(const cpmpc_sharded* s, int shard);          /* HIP device of a shard; -1 if out of range */
/* What cpmpc_sharded_create saw for this shard's device: 1 peer access between it and the root device (shard 0's) is
 * mapped in both directions (or it IS the root device) -- its slices travel device to device over xGMI; 0 not -- the
 * runtime stages those copies through host memory (slower, still correct); -1 out of range. */
int cpmpc_sharded_peer_access(const cpmpc_sharded* s, int shard);
cpmpc_solver* cpmpc_sharded_handle(cpmpc_sharded* s, int shard);      /* the shard's own solver (options, profiling) */
/* columns [*lo, *hi) of a B-problem batch that shard `shard` solves */
int cpmpc_sharded_range(const cpmpc_sharded* s, int shard, int64_t B, int64_t* lo, int64_t* hi);
int cpmpc_sharded_reset(cpmpc_sharded* s);                             /* Optimization::Reset on every shard */

/* Warm starts and the batch size.  Which shard owns a column depends on B, so the shards' previous solutions are tied to
 * the B of the call that produced them.  The rule, checked on every step / set / get:
 *   - a call with the same B as the last one uses the warm starts in place;
 *   - a call with another B first HANDS THE WARM START OVER to the new split (the solutions of the warm columns are
 *     gathered on the root device, every shard is reset, and each receives the columns it owns under the new B):
 *     columns [0, min(B, n)) stay warm, n = cpmpc_sharded_previous_solution_batch(); columns beyond B are dropped
 *     (a single handle would keep them: include/cpmpc.h, cpmpc_previous_solution_batch), new columns start cold;
 *   - a step that fails part-way resets every shard (no mixture of old and new solutions survives).
 * Never a silent misalignment.  The hand-over is synchronous and costs one gather + one scatter of [dim][n] scalars. */
int64_t cpmpc_sharded_previous_solution_batch(const cpmpc_sharded* s);
/* cpmpc_horizon_beyond_parity() of the sharded handle (its shards share one parameter set); -1: null handle */
int cpmpc_sharded_horizon_beyond_parity(const cpmpc_sharded* s);
/* Optimization::SetPreviousSolution over all shards (optimization.hpp:86-89): z [dim][B] on the ROOT device in the
 * handle's dtype (asynchronous on `stream`, a stream of the root device), or HOST doubles.  Replaces every warm start. */
int cpmpc_sharded_set_previous_solution(cpmpc_sharded* s, int64_t B, const void* z, void* stream);
int cpmpc_sharded_set_previous_solution_host(cpmpc_sharded* s, int64_t B, const double* z_host);
/* The warm start of columns [0, B), B <= cpmpc_sharded_previous_solution_batch() (what the next step reports as
 * OptimizationOutputs::previous_solution, optimization.cc:84): z_out [dim][B]. */
int cpmpc_sharded_get_solution(cpmpc_sharded* s, int64_t B, void* z_out, void* stream);
int cpmpc_sharded_get_solution_host(cpmpc_sharded* s, int64_t B, double* z_host);

/* cpmpc_step_batch_host_in over all shards: HOST arrays in the global layouts ([4][B] in, [N][B] etc. out), per-problem
 * parameters / set-points / terminal rows included; every shard's chunks are in flight together (cpmpc_set_host_chunk
 * on a shard's handle changes its chunk size). */
int cpmpc_sharded_step_batch_host_in(cpmpc_sharded* s, int64_t B, const cpmpc_step_host_inputs* in,
                                     const cpmpc_step_host_outputs* out);
/* shared parameters only (round 3's form) */
int cpmpc_sharded_step_batch_host(cpmpc_sharded* s, int64_t B, const double* x0_host, const double* dyn_shared_host,
                                  double set_point, const cpmpc_step_host_outputs* out);
/* cpmpc_step_batch over all shards with the data resident in HBM: every array of `in` (x0 [4][B]; dyn [9][B], set_point
 * [B], terminal_weights [4][B] when given) and every non-NULL output ([N][B] u, [N][4][B] predicted, [B] status /
 * iterations / ls_evals / final_cost / final_eq_l1, [dim][B] guess / solution) lives on the ROOT device (shard 0's), in
 * the handle's dtype.  Asynchronous on `stream` (a stream of the root device): slices travel to and from the other
 * shards' devices by peer copies ordered with events; on a failure part-way the call waits for the copies of the shards
 * already started before it returns the error. */
int cpmpc_sharded_step_batch_ex(cpmpc_sharded* s, int64_t B, const cpmpc_step_inputs* in,
                                const cpmpc_step_outputs* out, void* stream);
/* shared parameters only (round 3's form) */
int cpmpc_sharded_step_batch(cpmpc_sharded* s, int64_t B, const void* x0, const double* dyn_shared_host,
                             double set_point, const cpmpc_step_outputs* out, void* stream);

/* ---- feedback gains of the plan ----------------------------------------------------------------- */
/* K = du / dx0: how the planned controls move with the measured state, to first order,
 *     u(x0 + delta) ~ u + K delta,        K [N][NX] per problem.
 * The QP an SQP iteration solves is linear in its initial-state row z_0 - x0, so K is one more solve with the factors that
 * QP builds anyway ("Feedback gains").  K[0] is the time-varying linear feedback law of the real-time-iteration
 * scheme: it lets a caller run an inner loop faster than the re-plan (cpmpc_feedback_apply_batch), compensate the solve's
 * latency, or propagate measurement noise through a batch of controllers without re-solving.
 * What it is NOT: it is the gain of the UNCLAMPED, UNDAMPED QP at the linearisation point z -- no +-u_limit / +-b_x_limit
 * retraction, Levenberg-Marquardt term 0 whatever damping the last step ended with -- and it knows nothing of a line
 * search.  It depends on z, the dynamics parameters, the terminal weights and u_cost_weight / u_derivative_cost_weight
 * only: not on x0, the set-point, u_prev, the residuals or the defects.  Replaces nothing in the reference (which has
 * one controller and re-plans every tick). */
typedef struct cpmpc_gain_inputs {
  uint64_t struct_size;          /* = sizeof(cpmpc_gain_inputs) */
  const double* dyn_shared_host; /* HOST [NP] parameters shared by the batch, or NULL  } exactly one */
  const void* dyn;               /* [NP][B] per-problem parameters, or NULL            } of the two  */
  const void* terminal_weights;  /* [NX][B] per-problem terminal weights (cpmpc_step_inputs), or NULL: the handle's */
  const void* z;                 /* [dim][B] linearisation point (MapKey order), or NULL: the handle's previous solution --
                                  * the un-shifted z of the last step, what cpmpc_get_solution returns -- which must cover
                                  * B (cpmpc_previous_solution_batch), else CPMPC_ERR_INVALID_ARG.  A z given here goes through
                                  * the step buffers like cpmpc_linearize_batch's: the warm start is untouched either way */
} cpmpc_gain_inputs;
/* K [n_rows][NX][B] (batch fastest, the handle's dtype), rows 0 .. n_rows-1 of the gain, 1 <= n_rows <= N; row 0 alone
 * costs one linearisation and one pass over it.  ok [B], nullable: 1, or 0 for a problem whose control-cost pivots or
 * terminal system are not positive definite (or not numbers: a poisoned parameter set) -- its rows are NaN, its
 * neighbours are not affected.  Float handles carry the NX x NX terminal system in double; with cpmpc_wide_qp() the
 * products of transition matrices and the columns of U^-1 R^T as well.  Asynchronous on `stream`; writes only scratch of
 * the workspace that every step recomputes (a step's results do not depend on gain calls made in between). */
int cpmpc_feedback_gain_batch(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K,
                              int32_t* ok /*nullable*/, void* stream);
/* The same with HOST doubles (every pointer of `in`, K_host [n_rows][NX][B], ok_host [B] nullable); synchronous.  Used by
 * the C++ facade (pendulum::Optimization::FeedbackGain). */
int cpmpc_feedback_gain_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, double* K_host,
                                   int32_t* ok_host /*nullable*/);
/* u_out [B] = clamp(u_nom + K0 . wrap(x - x_nom), +-u_limit): the first row of the gains (K0 [NX][B]) applied to the
 * deviation of the state x [NX][B] from the state x_nom [NX][B] the plan was made for, the differences of the pole angles
 * wrapped to (-pi, pi]; u_nom [B].  u_limit > 0 (infinity: no clamp).  One elementwise launch, asynchronous on `stream`;
 * u_out may alias u_nom. */
int cpmpc_feedback_apply_batch(int dtype, int model, int64_t B, const void* u_nom, const void* K0, const void* x_nom,
                               const void* x, double u_limit, void* u_out, void* stream);

/* ---- sensitivities of the plan to the set-point and to u_prev, and the update of the whole plan ---- */
/* The QP that gives K is just as linear in the other two inputs that change between two re-plans:
 *     k_sp = du / dset_point   [N] per problem   (the b_x set-point of cpmpc_step_inputs, N/m),
 *     k_up = du / du_prev      [N] per problem   (the control applied before the plan starts, the u_prev of the row
 *                                                 u_derivative_cost_weight (u_0 - u_prev); dimensionless),
 * so that, to first order,
 *     u(x0 + dx, sp + dsp, u_prev + dup) ~ u + K dx + k_sp dsp + k_up dup.
 * What they are: like K, sensitivities of the UNDAMPED, UNCLAMPED QP at the linearisation point z (Gauss-Newton: the
 * second derivatives of the dynamics are not in them).  What they are NOT: derivatives of the converged NLP solution --
 * one SQP step from z with the moved input lands where they say, a re-plan run to convergence lands near it.  k_sp acts
 * through the b_x terminal row only (weight b_x_final_cost_weight, or the equality row); with that row's weight 0 it is 0.
 * They depend on z, the dynamics parameters, the terminal weights and the two control-cost weights only: not on x0, the
 * set-point's value, u_prev's value, the residuals or the defects.
 *
 * K [n_rows][NX][B], k_sp [n_rows][B], k_up [n_rows][B] in the handle's dtype, batch fastest; each is nullable and only
 * those given are computed; at least one must be given.  1 <= n_rows <= N.  `in`, ok, the preconditions, the error codes,
 * the precision split of float handles and the scratch written are those of cpmpc_feedback_gain_batch; a problem with
 * ok = 0 gets NaN in every output.  K asked for here -- alone or with the others -- is BITWISE the K of
 * cpmpc_feedback_gain_batch for the same handle and inputs (the kernel restates that one's arithmetic), and every output
 * is bitwise the same whichever others are asked for with it.  Asynchronous on `stream`. */
int cpmpc_plan_sensitivity_batch(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, void* K /*nullable*/,
                                 void* k_sp /*nullable*/, void* k_up /*nullable*/, int32_t* ok /*nullable*/, void* stream);
/* The same with HOST doubles (every pointer of `in`, K_host, k_sp_host, k_up_host, ok_host); synchronous.  Used by the
 * C++ facade (pendulum::Optimization::PlanSensitivity). */
int cpmpc_plan_sensitivity_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows,
                                      double* K_host /*nullable*/, double* k_sp_host /*nullable*/,
                                      double* k_up_host /*nullable*/, int32_t* ok_host /*nullable*/);
/* ---- reverse mode: a cotangent on the planned controls pulled back to x0, the set-point and u_prev ---- */
/* For a caller who differentiates through the controller -- a cost shaped on the planned controls, a policy that feeds x0
 * or the set-point, a state estimator upstream: given gbar = dL/du [n_rows] per problem (rows at and beyond n_rows are
 * zero), the vector-Jacobian products
 *     g_x0 = K^T gbar     [NX] per problem   = - Psi_0^T q,
 *     g_sp = k_sp^T gbar  scalar             =   Rw[0] q_0,
 *     g_up = k_up^T gbar  scalar             =   (w_du^2 / d_0) (eta_0 - w_0 . q),
 * with  eta_k = gbar_k - upsilon_k eta_{k+1}  and  a = sum_k w_k eta_k / d_k  carried through the one descending sweep that
 * builds S, and  q = (S + Dg)^-1 a  (notation: DESIGN.md section 5d).  K, k_sp and k_up are never formed: one
 * linearisation, one pass over Phi and Gamma, one terminal solve, whatever n_rows is.
 * What the gradients are: those of the UNDAMPED, UNCLAMPED Gauss-Newton QP at the linearisation point z, exactly the
 * transposes of what cpmpc_plan_sensitivity_batch returns.  What they are NOT: derivatives of the converged NLP solution,
 * of a clamped control, or with respect to the dynamics parameters, the weights (cpmpc_plan_weight_vjp_batch has those) or
 * z.  They do not depend on x0, the
 * set-point's value, u_prev's value, the residuals or the defects.
 *
 * gbar [n_rows][B], g_x0 [NX][B], g_sp [B], g_up [B] in the handle's dtype, batch fastest; each output is nullable and
 * only those given are computed; at least one must be given, gbar must be given, 1 <= n_rows <= N.  `in`, ok, the
 * preconditions and the error codes are those of cpmpc_plan_sensitivity_batch; a problem with ok = 0 gets NaN in every
 * output.  Float handles carry eta, a, q and the three products in double; with cpmpc_wide_qp() Psi and w_k as well.
 * Every output is bitwise the same whichever others are asked for with it, and n_rows < N gives bitwise what n_rows = N
 * gives for gbar padded with zeros.  Asynchronous on `stream`; the call writes only the linearisation scratch of the
 * workspace (Phi, Gamma, the defects; a z given in `in` goes through the step buffers), which every step recomputes before
 * it reads it: a step's results do not depend on calls made in between. */
int cpmpc_plan_vjp_batch(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows,
                         const void* gbar /* [n_rows][B] */, void* g_x0 /* [NX][B], nullable */,
                         void* g_sp /* [B], nullable */, void* g_up /* [B], nullable */, int32_t* ok /* nullable */,
                         void* stream);
/* The same with HOST doubles (every pointer of `in`, gbar_host, g_x0_host, g_sp_host, g_up_host, ok_host); synchronous.
 * Used by the C++ facade (pendulum::Optimization::PlanVjp). */
int cpmpc_plan_vjp_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows,
                              const double* gbar_host /* [n_rows][B] */, double* g_x0_host /* nullable */,
                              double* g_sp_host /* nullable */, double* g_up_host /* nullable */,
                              int32_t* ok_host /* nullable */);
/* ---- weight gradients: a cotangent on the planned controls pulled back to the cost weights ---- */
/* For a caller who tunes the controller itself: given gbar = dL/du+ [n_rows] per problem on the controls u+ = u + du that
 * the QP at z plans (rows at and beyond n_rows are zero), the gradients of L with respect to the cost weights
 *     g_tw [NX] per problem   the terminal weights in state order: -2 w_t yx_t (x_{S-1,t} + dx_{S-1,t} - target_t) for a cost
 *                             row with w_t > 0; exactly 0 for an equality row (w_t < 0) and for w_t = 0,
 *     g_wu      scalar        u_cost_weight:             -2 w_u  sum_k y_k (u_k + du_k),
 *     g_wdu     scalar        u_derivative_cost_weight:  -2 w_du [y_0 (u_0 + du_0 - u_prev)
 *                                                                 + sum_{k<N-1} (y_k - y_{k+1}) (u_k + du_k - u_{k+1} - du_{k+1})],
 * and, on request, du [n_rows] itself: the primal step of that QP (one undamped SQP step without a line search).  dz is the
 * QP's solution and y the solution of the same KKT system with gbar in the control rows; both are solved in condensed
 * form in one kernel over Phi and Gamma with one LDL^T.  w_u and w_du are the handle's weights,
 * clamped at 0 as in a step.
 * What the gradients are: those of the UNDAMPED, UNCLAMPED Gauss-Newton QP linearised at z.  At a converged z (dz -> 0) they
 * are the implicit-function derivative of the Gauss-Newton stationarity condition.  What they are NOT: derivatives through
 * the line search, the +-u_limit / +-b_x_limit retraction or the earlier iterations of the SQP, and there are none with
 * respect to the dynamics parameters.  Unlike K, k_sp and k_up they DO depend on x0, the set-point and u_prev, which is why
 * this call takes them.
 *
 * gbar [n_rows][B], g_tw [NX][B], g_wu [B], g_wdu [B], du [n_rows][B] in the handle's dtype, batch fastest; every output is
 * nullable and only those given are computed; at least one must be given; gbar may be NULL only when du is the only
 * output; 1 <= n_rows <= N.  ok, the preconditions on `lin` and the error codes are those of cpmpc_plan_vjp_batch; a problem
 * with ok = 0 gets NaN in every output.  Float handles carry eta, a, S, the LDL^T, both solves and the sums in double; with
 * cpmpc_wide_qp() Psi and w_k as well.  Every output is bitwise the same whichever others are asked for with it, and
 * n_rows < N gives bitwise what n_rows = N gives for gbar padded with zeros.  Asynchronous on `stream`; the call writes only
 * scratch that every step recomputes before it reads it (the linearisation's Phi, Gamma and defects, the rows of W and T; a z
 * given in `lin` goes through the step buffers): a step's results do not depend on calls made in between. */
typedef struct cpmpc_weight_vjp_inputs {
  uint64_t struct_size;     /* = sizeof(cpmpc_weight_vjp_inputs) */
  cpmpc_gain_inputs lin;    /* dyn, terminal_weights, z: as cpmpc_plan_vjp_batch (lin.struct_size = sizeof(cpmpc_gain_inputs)) */
  const void* x0;           /* [NX][B] the states the plan starts from, required */
  double set_point_shared;  /* the b_x set-point of every problem, used when set_point is NULL */
  const void* set_point;    /* [B] per-problem set-points, or NULL: as cpmpc_step_inputs */
  const void* u_prev;       /* [B] the control before u_0 (the row w_du (u_0 - u_prev)), or NULL: 0 for every problem */
} cpmpc_weight_vjp_inputs;
int cpmpc_plan_weight_vjp_batch(cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows,
                                const void* gbar /* [n_rows][B] */, void* g_tw /* [NX][B], nullable */,
                                void* g_wu /* [B], nullable */, void* g_wdu /* [B], nullable */,
                                void* du /* [n_rows][B], nullable */, int32_t* ok /* nullable */, void* stream);
/* The same with HOST doubles (every pointer of `in`, gbar_host and the outputs); synchronous.  Used by the C++ facade
 * (pendulum::Optimization::PlanWeightVjp). */
int cpmpc_plan_weight_vjp_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows,
                                     const double* gbar_host /* [n_rows][B] */, double* g_tw_host /* nullable */,
                                     double* g_wu_host /* nullable */, double* g_wdu_host /* nullable */,
                                     double* du_host /* nullable */, int32_t* ok_host /* nullable */);
/* The first-order re-plan of the whole horizon, one elementwise pass over rows k < n_rows:
 *     u_out[k] = clamp(u_nom[k] + K[k] . wrap(x - x_nom) + k_sp[k] (sp - sp_nom) + k_up[k] (u_prev - u_prev_nom), +-u_limit).
 * A step re-rolls every state of its initial guess from x0 and the controls, so the updated controls are a complete warm
 * start.  Device pointers in `dtype`; a term is absent when its sensitivity is NULL, and a sensitivity given without both
 * its nominal and its actual array is CPMPC_ERR_INVALID_ARG. */
typedef struct cpmpc_plan_update {
  uint64_t struct_size;   /* = sizeof(cpmpc_plan_update) */
  const void* u_nom;      /* [n_rows][B] the plan */
  const void* K;          /* [n_rows][NX][B], or NULL */
  const void* x_nom;      /* [NX][B] the state the plan was made for */
  const void* x;          /* [NX][B] the state now; the pole angles' differences are wrapped to (-pi, pi] */
  const void* k_sp;       /* [n_rows][B], or NULL */
  const void* sp_nom;     /* [B] the set-point the plan was made for */
  const void* sp;         /* [B] the set-point now */
  const void* k_up;       /* [n_rows][B], or NULL */
  const void* u_prev_nom; /* [B] the u_prev the plan was made for */
  const void* u_prev;     /* [B] the control actually applied before the plan starts */
  double u_limit;         /* > 0; infinity: no clamp */
  void* u_out;            /* [n_rows][B]; may alias u_nom */
} cpmpc_plan_update;
/* 1 <= n_rows <= 65535 (rows of the arrays given: the call knows no handle and no N; a row is one index of the launch
 * grid's second dimension, hence the upper limit -- more is CPMPC_ERR_INVALID_ARG).  Asynchronous on `stream`. */
int cpmpc_plan_update_batch(int dtype, int model, int64_t B, int n_rows, const cpmpc_plan_update* a, void* stream);

/* ---- measurement ------------------------------------------------------------------------------ */

enum {
  CPMPC_KERNEL_PREPARE = 0,   /* guess + FillInitialGuess */
  CPMPC_KERNEL_LINEARIZE = 1, /* RK4 + Jacobians over every shooting interval */
  CPMPC_KERNEL_QP_LS = 2,     /* structured QP + merit line search */
  CPMPC_KERNEL_FINALIZE = 3,  /* ComputePredictedStates + outputs */
  CPMPC_KERNEL_FUSED = 4,     /* all SQP iterations in one launch (fused pipeline) */
  CPMPC_KERNEL_COUNT = 5
};

/* Two implementations of the SQP iterations, same algorithm and decisions (results agree to rounding):
 *   CPMPC_PIPELINE_SPLIT  linearize_kernel + qp_ls_kernel per iteration, one problem per lane, the
 *                         sensitivities stream through HBM between the kernels (any configuration);
 *   CPMPC_PIPELINE_FUSED  one launch for all iterations, a problem spread over its S-1 shooting intervals' lanes,
 *                         sensitivities and QP factors in registers and LDS.  Both models; any state_spacing whose
 *                         interval count S-1 is one of 2, 4, 5, 8, 10, 16 and whose per-wave LDS fits 64 KB;
 *   CPMPC_PIPELINE_AUTO   fused where built, else split (default).  Two exceptions, both fp64: the 6-state model where fewer
 *                         than three of its fused waves fit a CU's LDS (state_spacing 20), and -- round 6 -- any handle whose
 *                         horizon is beyond cpmpc_max_parity_horizon(): the split QP kernel runs two refinement passes there
 *                         (cpmpc_horizon_beyond_parity).
 * The handle's options hold in either pipeline: cpmpc_refines_qp(), cpmpc_wide_qp() and cpmpc_get_solver_opts() tell what it
 * uses, cpmpc_get_pipeline() which pipeline its next step takes.
 * Returns CPMPC_ERR_UNSUPPORTED if FUSED is requested for a configuration it is not built for. */
enum { CPMPC_PIPELINE_AUTO = 0, CPMPC_PIPELINE_SPLIT = 1, CPMPC_PIPELINE_FUSED = 2 };
int cpmpc_set_pipeline(cpmpc_solver* s, int mode);
/* Fused pipeline with exit tolerances enabled: run `first_iterations` SQP iterations on every problem, then
 * compact the problems that are still iterating into dense waves before every further `next_iterations` (default
 * 2 and 1, applied to batches larger than one round of resident waves; an explicit call applies to every batch size;
 * 0 disables and gives the single launch).  A speed setting only: results do not change.  Which staging is fastest
 * depends on how the iteration counts are spread: tools/steady_state.py measures a workload under each. */
int cpmpc_set_compaction(cpmpc_solver* s, int first_iterations, int next_iterations);
/* Without an explicit cpmpc_set_compaction the stages are planned per step from how many iterations the problems of the
 * most recent FINISHED step needed (a histogram finalize leaves in host-mapped memory; read without synchronisation):
 * a settled closed loop, where every controller stops after one iteration, runs two launches instead of seven; a batch
 * whose iteration counts spread gets a cut wherever enough problems have stopped to pay for a compaction.  Speed only:
 * results never depend on the plan, but the SEQUENCE OF LAUNCHES of a default-staged step does depend on unsynchronised
 * timing (which earlier step's counts have reached host memory), so kernel counts in a trace differ from run to run, and
 * a HIP-graph capture bakes in the plan of the moment and the step's stamp -- a tick captured during a transient replays
 * its seven launches for ever, one captured when settled is bound by its stragglers after a disturbance.  Before capturing
 * a graph, or for reproducible traces, fix the pattern with cpmpc_set_compaction.  max_iterations above 15 always takes
 * the fixed pattern (the histogram has 16 bins, the last one standing for "ran to the cap").
 * This reads back the plan of the last step: bounds[0] = 0 < ... < bounds[n] = max_iterations, returns n (the number of
 * launches of the fused kernel), -1 on a bad argument. */
int cpmpc_get_stage_plan(const cpmpc_solver* s, int32_t* bounds, int capacity);
/* The planner alone (no device, no handle; for tests and tools): hist[16], hist[k] = problems that ran k iterations (the
 * last bin collects every larger count), for a batch of B problems with `intervals` = S - 1 shooting intervals.  Writes
 * bounds[0 .. n], returns n; -1 on a bad argument (max_iterations must be 1 .. 15, capacity >= max_iterations + 1). */
int cpmpc_plan_stages_from_histogram(const int64_t* hist, int64_t B, int max_iterations, int intervals, int dtype,
                                     int window_length, int32_t* bounds, int capacity);
int cpmpc_get_pipeline(const cpmpc_solver* s); /* the one a step will actually use: SPLIT or FUSED */

/* When enabled, every kernel launch of cpmpc_step_batch is bracketed by HIP events on the launch
 * stream; cpmpc_profile_read synchronises those events and returns the accumulated device time. */
int cpmpc_profile_enable(cpmpc_solver* s, int on);
int cpmpc_profile_reset(cpmpc_solver* s);
int cpmpc_profile_read(cpmpc_solver* s, int kernel, double* total_ms, int64_t* launches);
const char* cpmpc_kernel_name(int kernel);

#ifdef __cplusplus
}
#endif
#endif
