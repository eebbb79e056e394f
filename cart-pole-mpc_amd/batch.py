"""Batched host API over the C-ABI: torch tensors (device memory + streams only) in, tensors out.

Names follow the reference's interface for this path (optimization/optimization.hpp:73-108,
optimization/simulator.hpp:10-29): Optimization -> BatchOptimization with step / reset /
set_previous_solution; Simulator -> BatchSimulator with step / get_state / set_state.
Every array is structure-of-arrays, [field, B].  All compute happens in libcpmpc.so's HIP kernels;
this module raises if the library or a gfx950 device is missing.
"""
import ctypes as C

import torch

from . import capi

_CAPI_DTYPE = {torch.float32: capi.F32, torch.float64: capi.F64}


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_cuda_tensor(t, name, dtype, shape=None, contiguous=True):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a GPU tensor" % name)
    if t.dtype != dtype:
        raise TypeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))
    if contiguous and not t.is_contiguous():
        raise ValueError("%s must be contiguous ([field, B], batch fastest)" % name)
    if shape is not None and t.shape != shape:   # shape: a tuple (torch.Size is one)
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _want_tuple(want, names, allow_empty=False, message=None):
    """`want` (one name or several) as a tuple, in the order given; ValueError where it names something outside `names` or,
    unless allow_empty, nothing.  Runs before any tensor is looked at."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in names for w in want) or not (want or allow_empty):
        raise ValueError(message or "want must name at least one of %s" % ", ".join(repr(n) for n in names))
    return want


def _alloc_outputs(a, want, table, dtype, device):
    """{name: torch.empty tensor} for the names in `want`, with table[name] = (field, shape); where a struct `a` is given the
    tensor's pointer goes into a.field, and the fields of the names not wanted stay null."""
    res = {}
    for name in want:
        field, shape = table[name]
        res[name] = torch.empty(shape, dtype=dtype, device=device)
        if a is not None:
            setattr(a, field, res[name].data_ptr())
    return res


class BatchOutputs:
    """Batched OptimizationOutputs (optimization/optimization.hpp:55-70)."""

    def __init__(self):
        self.u = None                 # [N, B]
        self.predicted_states = None  # [N, 4, B]
        self.status = None            # [B] int32, termination state
        self.iterations = None        # [B] int32
        self.ls_evals = None          # [B] int32
        self.final_cost = None        # [B]
        self.final_eq_l1 = None       # [B]
        self.guess = None             # [dim, B]
        self.horizon_beyond_parity = False   # cpmpc_horizon_beyond_parity() of the handle that filled these outputs

    def solver_summary(self):
        """Batch summary in the spirit of NLSSolverOutputs::ToString (wrapper/wrapper.cc:82-83)."""
        st = self.status.cpu()
        lines = ["batch of %d problems" % st.numel()]
        if getattr(self, "horizon_beyond_parity", False):
            lines.append("  horizon beyond %.1f s (cpmpc_max_parity_horizon): a few cold starts in 10^4 may differ from a "
                         "full-space solve by more than 1e-5" % capi.load().cpmpc_max_parity_horizon())
        for code in sorted(set(st.tolist())):
            lines.append("  %-28s %d" % (capi.TERM_NAMES.get(code, str(code)), int((st == code).sum())))
        if self.iterations is not None:
            it = self.iterations.cpu().float()
            lines.append("  iterations: mean %.2f max %d" % (it.mean().item(), int(it.max().item())))
        if self.final_eq_l1 is not None:
            lines.append("  max |c|_1: %.3e" % self.final_eq_l1.abs().max().item())
        return "\n".join(lines)

    def lane_json(self, lane, initial_state, previous_solution=None):
        """One problem of the batch in the JSON log format of OptimizationOutputs (optimization/wasm.cc:46-65,
        toJson :104-105): keys sorted, compact, as nlohmann::json::dump() prints them.  `initial_state` is the
        [4, B] tensor passed to step(); `previous_solution` the [dim, B] tensor of get_solution() (optional).
        solver_outputs carries this repo's fields (mini_opt's serialisation is not available)."""
        import json

        def col(t):
            return [float(v) for v in t[..., lane].double().cpu().reshape(-1)]

        names = ("b_x", "th_1", "b_x_dot", "th_1_dot")
        pred = self.predicted_states[:, :, lane].double().cpu().tolist()
        obj = {
            "initial_state": dict(zip(names, col(initial_state))),
            "previous_solution": col(previous_solution) if previous_solution is not None else [],
            "solver_outputs": {
                "termination_state": capi.TERM_NAMES[int(self.status[lane])],
                "iterations": int(self.iterations[lane]) if self.iterations is not None else 0,
                "final_cost": float(self.final_cost[lane]) if self.final_cost is not None else 0.0,
                "final_equality_l1": float(self.final_eq_l1[lane]) if self.final_eq_l1 is not None else 0.0,
            },
            "u": col(self.u),
            "predicted_states": [dict(zip(names, row)) for row in pred],
        }
        return json.dumps(obj, sort_keys=True, separators=(",", ":"))


class BatchOptimization:
    """B independent pendulum::Optimization controllers solved in lock-step on one GPU."""

    def __init__(self, params, max_batch, dtype=torch.float32, device=None, opts=None, model="single",
                 allow_long_horizon=False, refine_qp=None, strict_horizon=False, wide_qp=None):
        """strict_horizon: refuse (CpmpcError(ERR_UNSUPPORTED)) window_length * control_dt beyond
        cpmpc_max_parity_horizon() (1.0 s), where the condensed QP is no longer held to 1e-5 of a full-space solve on
        every problem (include/cpmpc.h, CPMPC_CREATE_STRICT_HORIZON).  By default every horizon the reference accepts is
        accepted, with one warning per process; allow_long_horizon=True silences the warning.
        refine_qp: True / False force on / off the refinement of the whole QP solution in the fp64 fused kernels
        (CPMPC_CREATE_[NO_]REFINE_QP: 7 % slower); None = the library's default: on when u_cost_weight < 0.05 and, for
        the 6-state model, when th_final_cost_weight >= 0 with th_dot_final_cost_weight < 0 (include/cpmpc.h).
        wide_qp: True / False force on / off that float32 handles carry the QP's whole terminal part in double
        (CPMPC_CREATE_[NO_]WIDE_QP: cold starts end where a float solve can -- 3x to 20x closer to the double check for the
        4-state model at 3.8 % of the throughput, 70x to 900x for the 6-state one at 0 - 5 %); None = the library's
        default: on for the 6-state model, off for the 4-state one."""
        lib = capi.load()
        self.model = capi.MODELS[model]
        self.nx = lib.cpmpc_model_state_dim(self.model)
        self.np = lib.cpmpc_model_num_params(self.model)
        if dtype not in _CAPI_DTYPE:
            raise TypeError("dtype must be torch.float32 or torch.float64")
        if device is None:
            device = torch.cuda.current_device()
        self.params = params
        self.opts = opts
        self.dtype = dtype
        self.device = int(device)
        self._dev = torch.device("cuda", self.device)
        self.max_batch = int(max_batch)
        self._h = C.c_void_p()
        info = capi.CreateInfo(struct_size=C.sizeof(capi.CreateInfo),
                               flags=(capi.CREATE_ALLOW_LONG_HORIZON if allow_long_horizon else 0)
                               | (capi.CREATE_STRICT_HORIZON if strict_horizon else 0)
                               | (0 if wide_qp is None else (capi.CREATE_WIDE_QP if wide_qp else capi.CREATE_NO_WIDE_QP))
                               | (0 if refine_qp is None else (capi.CREATE_REFINE_QP if refine_qp else capi.CREATE_NO_REFINE_QP)),
                               dtype=_CAPI_DTYPE[dtype], model=self.model, device=self.device, reserved=0,
                               max_batch=self.max_batch, params=C.pointer(params),
                               opts=C.pointer(opts) if opts is not None else None,
                               opts_size=C.sizeof(capi.SolverOpts) if opts is not None else 0)
        capi.check(lib.cpmpc_create_ex(C.byref(info), C.byref(self._h)))
        self.N = int(params.window_length)
        self.S = lib.cpmpc_num_states(self._h)
        self.dim = lib.cpmpc_dim(self._h)
        self._keep = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            capi.load().cpmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- marshalling --------------------------------------------------------------------------
    def _batch_of(self, x0):
        """B of the initial states x0 [nx, B], checked."""
        _require_cuda_tensor(x0, "x0", self.dtype)
        shape = x0.shape
        if len(shape) != 2 or shape[0] != self.nx:
            raise ValueError("x0 must be [%d, B]" % self.nx)
        return shape[1]

    def _set_dyn(self, inp, B, dyn, terminal_weights):
        """dyn (np floats, shared, or an [np, B] tensor) and terminal_weights (None or an [nx, B] tensor) checked and set on
        `inp`, a StepInputs or a GainInputs: both name these fields alike.  What is not given is set to null, so a reused
        struct is safe -> what the call reads, as a list: the caller holds it until the call has returned (the host array)
        or, for an asynchronous launch, longer (step)."""
        if isinstance(dyn, torch.Tensor):
            _require_cuda_tensor(dyn, "dyn", self.dtype, (self.np, B))
            inp.dyn, inp.dyn_shared_host = dyn.data_ptr(), None
            keep = [dyn]
        else:
            keep = [capi.dbl_array(dyn, self.np)]
            inp.dyn, inp.dyn_shared_host = None, C.cast(keep[0], C.POINTER(C.c_double))
        if terminal_weights is not None:
            _require_cuda_tensor(terminal_weights, "terminal_weights", self.dtype, (self.nx, B))
            inp.terminal_weights = terminal_weights.data_ptr()
            keep.append(terminal_weights)
        else:
            inp.terminal_weights = None
        return keep

    def _set_set_point(self, inp, B, set_point):
        """set_point (a float, shared, or a [B] tensor) checked and set on `inp`, a StepInputs or a WeightVjpInputs -> the
        tensor to keep, as a list."""
        if isinstance(set_point, torch.Tensor):
            _require_cuda_tensor(set_point, "set_point", self.dtype, (B,))
            inp.set_point, inp.set_point_shared = set_point.data_ptr(), 0.0
            return [set_point]
        inp.set_point, inp.set_point_shared = None, float(set_point)
        return []

    def _linearisation_point(self, inp, who, dyn, z, terminal_weights, B=None):
        """The point a plan call of the method `who` linearises at, resolved and set on the GainInputs `inp`: z a [dim, B]
        tensor, or None = the handle's previous solution with B = previous_solution_batch().  A caller that has B from
        elsewhere (plan_weight_vjp: from x0) passes it, having checked z against it -> (B, what the caller holds until the
        call has returned: _set_dyn)."""
        if B is None:
            if z is not None:
                _require_cuda_tensor(z, "z", self.dtype)
                if z.dim() != 2 or z.shape[0] != self.dim:
                    raise ValueError("z must be [dim=%d, B]" % self.dim)
                B = int(z.shape[1])
            else:
                B = self.previous_solution_batch()
                if B < 1:
                    raise ValueError("%s(z=None) needs a previous solution: step() first, or pass z" % who)
        inp.struct_size = C.sizeof(capi.GainInputs)
        keep = self._set_dyn(inp, B, dyn, terminal_weights)
        inp.z = z.data_ptr() if z is not None else None
        return B, keep

    def _cotangent_rows(self, gbar, B):
        """n_rows of a cotangent gbar [n_rows, B] on the planned controls, checked."""
        _require_cuda_tensor(gbar, "gbar", self.dtype)
        if gbar.dim() != 2 or gbar.shape[1] != B:
            raise ValueError("gbar must be [n_rows, B=%d]" % B)
        return int(gbar.shape[0])

    # -- Optimization::Step -------------------------------------------------------------------
    def step(self, x0, dyn, set_point=0.0, want_predicted=True, want_stats=True, want_guess=False,
             out=None, terminal_weights=None):
        """x0: [nx, B] tensor.  dyn: np floats (shared) or an [np, B] tensor.  set_point: float or [B].
        terminal_weights: optional [nx, B] tensor of per-problem terminal weights in state order (>= 0 cost row,
        < 0 equality row; optimization.cc:236-267), overriding the four *_final_cost_weight parameters."""
        lib = capi.load()
        dev = self._dev
        B = self._batch_of(x0)
        inp = capi.StepInputs()
        inp.x0 = x0.data_ptr()
        keep = [x0] + self._set_dyn(inp, B, dyn, terminal_weights) + self._set_set_point(inp, B, set_point)

        o = out if out is not None else BatchOutputs()

        def reusable(t, shape, dtype):
            # a buffer handed back in `out` is written by the kernels as `dtype` on `dev`: anything else (another
            # optimizer's outputs of the other precision, another device) must be replaced, never written through
            return t is not None and t.shape == shape and t.dtype == dtype and t.device == dev and t.is_contiguous()
        if not reusable(o.u, (self.N, B), self.dtype):
            o.u = torch.empty((self.N, B), dtype=self.dtype, device=dev)
        if want_predicted and not reusable(o.predicted_states, (self.N, self.nx, B), self.dtype):
            o.predicted_states = torch.empty((self.N, self.nx, B), dtype=self.dtype, device=dev)
        if not reusable(o.status, (B,), torch.int32):
            o.status = torch.empty((B,), dtype=torch.int32, device=dev)
        if want_stats and not (reusable(o.iterations, (B,), torch.int32) and reusable(o.ls_evals, (B,), torch.int32)
                               and reusable(o.final_cost, (B,), self.dtype) and reusable(o.final_eq_l1, (B,), self.dtype)):
            o.iterations = torch.empty((B,), dtype=torch.int32, device=dev)
            o.ls_evals = torch.empty((B,), dtype=torch.int32, device=dev)
            o.final_cost = torch.empty((B,), dtype=self.dtype, device=dev)
            o.final_eq_l1 = torch.empty((B,), dtype=self.dtype, device=dev)
        if want_guess:
            o.guess = torch.empty((self.dim, B), dtype=self.dtype, device=dev)
        outp = capi.StepOutputs()
        outp.u = o.u.data_ptr()
        outp.predicted = o.predicted_states.data_ptr() if want_predicted else None
        outp.status = o.status.data_ptr()
        if want_stats:
            outp.iterations = o.iterations.data_ptr()
            outp.ls_evals = o.ls_evals.data_ptr()
            outp.final_cost = o.final_cost.data_ptr()
            outp.final_eq_l1 = o.final_eq_l1.data_ptr()
        outp.guess = o.guess.data_ptr() if want_guess else None
        with torch.cuda.device(self.device):
            capi.check(lib.cpmpc_step_batch(self._h, B, C.byref(inp), C.byref(outp), _stream_ptr()))
        self._keep = keep  # inputs must outlive the asynchronous launch
        o.horizon_beyond_parity = self.horizon_beyond_parity
        return o

    # -- Optimization::Reset / SetPreviousSolution ---------------------------------------------
    def reset(self):
        capi.check(capi.load().cpmpc_reset(self._h))

    def has_previous_solution(self):
        return bool(capi.load().cpmpc_has_previous_solution(self._h))

    def previous_solution_batch(self):
        """Problems [0, n) hold a previous solution (warm start); the others cold-start at the next step."""
        return int(capi.load().cpmpc_previous_solution_batch(self._h))

    def set_previous_solution(self, z):
        _require_cuda_tensor(z, "z", self.dtype)
        if z.dim() != 2 or z.shape[0] != self.dim:
            raise ValueError("z must be [dim=%d, B]" % self.dim)
        with torch.cuda.device(self.device):
            capi.check(capi.load().cpmpc_set_previous_solution(self._h, int(z.shape[1]), _ptr(z),
                                                               _stream_ptr()))

    def get_solution(self, B):
        z = torch.empty((self.dim, int(B)), dtype=self.dtype, device=self._dev)
        with torch.cuda.device(self.device):
            capi.check(capi.load().cpmpc_get_solution(self._h, int(B), _ptr(z), _stream_ptr()))
        return z

    # -- pieces -------------------------------------------------------------------------------
    def linearize(self, z, dyn):
        """Shooting constraints linearised at z [dim, B] -> (c [4(S-1), B], Phi [S-1,4,4,B],
        Gamma [N,4,B] with Gamma[k, r] = d x_end[r] / d u_k)."""
        _require_cuda_tensor(z, "z", self.dtype)
        B = int(z.shape[1])
        dev = z.device
        nx = self.nx
        c = torch.empty((nx * (self.S - 1), B), dtype=self.dtype, device=dev)
        Phi = torch.empty((self.S - 1, nx, nx, B), dtype=self.dtype, device=dev)
        Gam = torch.empty((self.N, nx, B), dtype=self.dtype, device=dev)
        arr = capi.dbl_array(dyn, self.np)
        with torch.cuda.device(self.device):
            capi.check(capi.load().cpmpc_linearize_batch(self._h, B, arr, _ptr(z), _ptr(c), _ptr(Phi),
                                                         _ptr(Gam), _stream_ptr()))
        return c, Phi, Gam

    def feedback_gain(self, dyn, n_rows=1, z=None, terminal_weights=None, want_ok=False):
        """K = du / dx0 of the plan, rows 0 .. n_rows-1: tensor [n_rows, nx, B] with u(x0 + d) ~ u + K d (include/cpmpc.h:
        cpmpc_feedback_gain_batch).  The gain of the unclamped, undamped QP at z: z None = the handle's previous solution
        (B = previous_solution_batch()), else a [dim, B] tensor; the warm start is untouched either way.  dyn: np floats
        (shared) or an [np, B] tensor; terminal_weights: optional [nx, B] tensor as in step().  want_ok: also return the
        [B] int32 tensor that is 0 for a problem whose QP is not positive definite (its rows are NaN)."""
        dev = self._dev
        inp = capi.GainInputs()
        B, _held = self._linearisation_point(inp, "feedback_gain", dyn, z, terminal_weights)   # _held: until the call is back
        n_rows = int(n_rows)
        K = torch.empty((max(n_rows, 0), self.nx, B), dtype=self.dtype, device=dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev) if want_ok else None
        with torch.cuda.device(self.device):
            capi.check(capi.load().cpmpc_feedback_gain_batch(self._h, B, C.byref(inp), n_rows, _ptr(K), _ptr(ok),
                                                             _stream_ptr()))
        return (K, ok) if want_ok else K

    def plan_sensitivity(self, dyn, n_rows=1, z=None, terminal_weights=None, want=("K", "k_sp", "k_up"), want_ok=False):
        """How the plan moves with the three inputs that change between two re-plans, rows 0 .. n_rows-1 (include/cpmpc.h:
        cpmpc_plan_sensitivity_batch): a dict with the entries named in `want` --
            "K"    [n_rows, nx, B]  du / dx0 (what feedback_gain returns, bitwise),
            "k_sp" [n_rows, B]      du / dset_point,
            "k_up" [n_rows, B]      du / du_prev (the control applied before the plan starts),
        and "ok" [B] int32 with want_ok (0: the problem's QP is not positive definite, its outputs are NaN).  Sensitivities
        of the unclamped, undamped QP at z, not of the converged solution; arguments as feedback_gain's.  Only what is
        named is computed; plan_update() applies them to the whole plan."""
        want = _want_tuple(want, ("K", "k_sp", "k_up"))
        dev = self._dev
        inp = capi.GainInputs()
        B, _held = self._linearisation_point(inp, "plan_sensitivity", dyn, z, terminal_weights)
        n_rows = int(n_rows)
        rows = max(n_rows, 0)
        res = _alloc_outputs(None, want, {"K": (None, (rows, self.nx, B)), "k_sp": (None, (rows, B)), "k_up": (None, (rows, B))},
                             self.dtype, dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev) if want_ok else None
        with torch.cuda.device(self.device):
            capi.check(capi.load().cpmpc_plan_sensitivity_batch(self._h, B, C.byref(inp), n_rows, _ptr(res.get("K")),
                                                                _ptr(res.get("k_sp")), _ptr(res.get("k_up")), _ptr(ok),
                                                                _stream_ptr()))
        if want_ok:
            res["ok"] = ok
        return res

    def plan_vjp(self, dyn, gbar, z=None, terminal_weights=None, want=("x0", "set_point", "u_prev"), want_ok=False):
        """The reverse mode of plan_sensitivity (include/cpmpc.h: cpmpc_plan_vjp_batch): a cotangent gbar = dL/du
        [n_rows, B] on the planned controls (rows at and beyond n_rows = gbar.shape[0] are zero) pulled back to the inputs
        named in `want` -- a dict with
            "x0"        [nx, B]  K^T gbar,
            "set_point" [B]      k_sp^T gbar,
            "u_prev"    [B]      k_up^T gbar,
        and "ok" [B] int32 with want_ok (0: the problem's QP is not positive definite, its outputs are NaN).  K, k_sp and
        k_up are never formed: one linearisation and one pass over it.  Gradients of the unclamped, undamped Gauss-Newton QP
        at z, not of the converged solution; arguments as feedback_gain's.  Only what is named is computed."""
        want = _want_tuple(want, ("x0", "set_point", "u_prev"))
        dev = self._dev
        inp = capi.GainInputs()
        B, _held = self._linearisation_point(inp, "plan_vjp", dyn, z, terminal_weights)
        n_rows = self._cotangent_rows(gbar, B)
        res = _alloc_outputs(None, want, {"x0": (None, (self.nx, B)), "set_point": (None, (B,)), "u_prev": (None, (B,))},
                             self.dtype, dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev) if want_ok else None
        with torch.cuda.device(self.device):
            capi.check(capi.load().cpmpc_plan_vjp_batch(self._h, B, C.byref(inp), n_rows, _ptr(gbar), _ptr(res.get("x0")),
                                                        _ptr(res.get("set_point")), _ptr(res.get("u_prev")), _ptr(ok),
                                                        _stream_ptr()))
        if want_ok:
            res["ok"] = ok
        return res

    def plan_weight_vjp(self, x0, dyn, gbar, set_point=0.0, u_prev=None, z=None, terminal_weights=None,
                        want=("terminal", "u", "du_dt"), want_du=False, want_ok=False):
        """The gradients of a loss on the planned controls with respect to the cost weights (include/cpmpc.h:
        cpmpc_plan_weight_vjp_batch): for a cotangent gbar = dL/du+ [n_rows, B] on the controls u+ = u + du of the QP at z
        (rows at and beyond n_rows = gbar.shape[0] are zero), a dict with the entries named in `want`,
            "terminal" [nx, B]  dL/d(terminal weights), state order; exactly 0 for an equality row and a zero weight,
            "u"        [B]      dL/d(u_cost_weight),
            "du_dt"    [B]      dL/d(u_derivative_cost_weight),
        "du" [n_rows, B] with want_du -- the primal step of that QP, one undamped SQP step without a line search -- and "ok"
        [B] int32 with want_ok (0: the problem's QP is not positive definite, its outputs are NaN).  x0 [nx, B], set_point
        (a float or [B]) and u_prev ([B]; None: 0) are what a step from z would see: unlike plan_vjp's, these gradients
        depend on them.  Gradients of the unclamped, undamped Gauss-Newton QP at z, not through the line search, the clamps
        or earlier iterations; none with respect to the dynamics parameters.  dyn, z, terminal_weights as feedback_gain's.
        want may be empty when want_du is set (gbar is then only read for its shape and may be None with n_rows = N)."""
        want = _want_tuple(want, ("terminal", "u", "du_dt"), allow_empty=want_du,
                           message="want must name some of 'terminal', 'u', 'du_dt' (or nothing, with want_du)")
        dev = self._dev
        B = self._batch_of(x0)
        if z is not None:
            _require_cuda_tensor(z, "z", self.dtype, (self.dim, B))
        elif self.previous_solution_batch() < B:
            raise ValueError("plan_weight_vjp(z=None) needs a previous solution for every problem: step() first, or pass z")
        if gbar is None:
            if want:
                raise ValueError("gbar may be None only when du is the only output")
            n_rows = self.N
        else:
            n_rows = self._cotangent_rows(gbar, B)
        inp = capi.WeightVjpInputs(struct_size=C.sizeof(capi.WeightVjpInputs))
        _, _held = self._linearisation_point(inp.lin, "plan_weight_vjp", dyn, z, terminal_weights, B=B)
        inp.x0 = x0.data_ptr()
        self._set_set_point(inp, B, set_point)
        if u_prev is not None:
            _require_cuda_tensor(u_prev, "u_prev", self.dtype, (B,))
            inp.u_prev = u_prev.data_ptr()
        res = _alloc_outputs(None, want + (("du",) if want_du else ()),
                             {"terminal": (None, (self.nx, B)), "u": (None, (B,)), "du_dt": (None, (B,)),
                              "du": (None, (n_rows, B))}, self.dtype, dev)
        ok = torch.empty((B,), dtype=torch.int32, device=dev) if want_ok else None
        with torch.cuda.device(self.device):
            capi.check(capi.load().cpmpc_plan_weight_vjp_batch(self._h, B, C.byref(inp), n_rows, _ptr(gbar),
                                                               _ptr(res.get("terminal")), _ptr(res.get("u")),
                                                               _ptr(res.get("du_dt")), _ptr(res.get("du")), _ptr(ok),
                                                               _stream_ptr()))
        if want_ok:
            res["ok"] = ok
        return res

    def step_differentiable(self, x0, dyn, set_point=0.0, n_rows=None, terminal_weights=None, weight_grad=False, **step_kw):
        """step() with a backward: returns (u, outputs), `outputs` what step(x0, dyn, set_point, ...) returns -- outputs.u is
        bitwise step's -- and u = outputs.u[:n_rows] (n_rows None: all N rows) attached to the autograd graph of x0 and,
        when it is a [B] tensor, set_point.

        Which derivative: that of the LAST QP of the step -- the undamped, unclamped Gauss-Newton QP linearised at the
        step's solution z (plan_vjp; include/cpmpc.h: cpmpc_plan_vjp_batch).  It is not the derivative of the converged NLP
        solution, it ignores the +-u_limit / +-b_x_limit retraction, and nothing flows to dyn, terminal_weights or the
        parameters.  Backward is one plan_vjp call on the current stream and is differentiable once only.  The forward
        keeps its own copy of z, dyn and terminal_weights, so later steps on this handle do not change an earlier graph's
        backward.  A problem whose QP is not positive definite (plan_vjp's ok = 0) gets gradient 0, not NaN.  The graph
        holds this handle, whose workspace backward uses: it must stay open until backward has run (after close() backward
        raises CpmpcError, a null handle).

        weight_grad=True (with a terminal_weights tensor that requires grad): backward makes one further call,
        plan_weight_vjp at the step's z, x0, set-point and the u_prev the step's row w_du (u_0 - u_prev) saw -- control 0 of
        the previous solution for a problem that had one, 0 for a cold start -- and returns its "terminal" gradient for
        terminal_weights (0 for a lane with ok = 0).  u_cost_weight and u_derivative_cost_weight are parameters of the
        handle, not tensors: their gradients are available from plan_weight_vjp only.  With weight_grad=False this is the
        function it was before the argument existed, graph included."""
        n_rows = self.N if n_rows is None else int(n_rows)
        if not 1 <= n_rows <= self.N:   # before the step: a refused call leaves the warm start where it was
            raise ValueError("n_rows must be in [1, window_length = %d]" % self.N)
        if weight_grad and not isinstance(terminal_weights, torch.Tensor):
            raise ValueError("weight_grad=True needs a terminal_weights tensor")
        u_prev = None
        if weight_grad:   # what prepare_kernel reads before the previous solution is overwritten (optimization.cc:288-291)
            B = self._batch_of(x0)
            warm = min(self.previous_solution_batch(), B)
            u_prev = torch.zeros((B,), dtype=self.dtype, device=self._dev)
            if warm > 0:   # (the C-ABI reads a solution whole: one [dim, warm] copy, of which row nx S is control 0)
                u_prev[:warm] = self.get_solution(warm)[self.nx * self.S]
        o = self.step(x0, dyn, set_point, terminal_weights=terminal_weights, **step_kw)
        B = int(x0.shape[1])
        z = self.get_solution(B)
        dyn_kept = dyn.detach().clone() if isinstance(dyn, torch.Tensor) else [float(v) for v in dyn]
        tw_kept = None if terminal_weights is None else terminal_weights.detach().clone()
        sp_t = set_point if isinstance(set_point, torch.Tensor) else None
        if weight_grad:
            sp_kept = set_point.detach().clone() if sp_t is not None else float(set_point)
            u = _PlanWeightVjpFunction.apply(self, o.u, n_rows, z, dyn_kept, tw_kept, x0.detach().clone(), sp_kept, u_prev,
                                             x0, sp_t, terminal_weights)
        else:
            u = _PlanVjpFunction.apply(self, o.u, n_rows, z, dyn_kept, tw_kept, x0, sp_t)
        return u, o

    # -- pipeline selection --------------------------------------------------------------------
    def set_pipeline(self, mode):
        """'auto' | 'split' | 'fused' (include/cpmpc.h: CPMPC_PIPELINE_*)."""
        capi.check(capi.load().cpmpc_set_pipeline(self._h, capi.PIPELINES[mode]))

    @property
    def horizon_beyond_parity(self):
        """True: window_length * control_dt exceeds cpmpc_max_parity_horizon() (include/cpmpc.h: cpmpc_horizon_beyond_parity)."""
        return bool(capi.load().cpmpc_horizon_beyond_parity(self._h))

    @property
    def refines_qp(self):
        return bool(capi.load().cpmpc_refines_qp(self._h))

    @property
    def wide_qp(self):
        """True: this float handle's steps carry the QP's terminal part in double (include/cpmpc.h: CPMPC_CREATE_WIDE_QP)."""
        return bool(capi.load().cpmpc_wide_qp(self._h))

    def set_compaction(self, first_iterations=2, next_iterations=1):
        """Staging of the fused pipeline when exit tolerances are enabled (0, 0 = one launch).  Speed only."""
        capi.check(capi.load().cpmpc_set_compaction(self._h, int(first_iterations), int(next_iterations)))

    def stage_plan(self):
        """Boundaries [0, ..., max_iterations] of the launches of the fused kernel in the last step (cpmpc_get_stage_plan)."""
        buf = (C.c_int32 * 32)()
        n = capi.load().cpmpc_get_stage_plan(self._h, buf, 32)
        return [int(buf[i]) for i in range(n + 1)] if n >= 0 else []

    def pipeline(self):
        return {capi.PIPELINE_SPLIT: "split", capi.PIPELINE_FUSED: "fused"}[capi.load().cpmpc_get_pipeline(self._h)]

    # -- measurement --------------------------------------------------------------------------
    def profile_enable(self, on=True):
        capi.check(capi.load().cpmpc_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        capi.check(capi.load().cpmpc_profile_reset(self._h))

    def profile_read(self):
        """{kernel name: (total_ms, launches)} accumulated since the last reset."""
        lib = capi.load()
        res = {}
        for kid in range(capi.KERNEL_COUNT):
            ms, n = C.c_double(), C.c_int64()
            capi.check(lib.cpmpc_profile_read(self._h, kid, C.byref(ms), C.byref(n)))
            res[lib.cpmpc_kernel_name(kid).decode()] = (ms.value, n.value)
        return res


def _needing_grad(ctx, inputs, names):
    """Those of `names` that need a gradient, each looked up at its own position among the forward's `inputs`."""
    return [n for n in names if ctx.needs_input_grad[inputs.index(n)]]


def _masked_plan_vjp(ctx, gbar, want):
    """One plan_vjp call at what the forward kept on ctx, for the inputs in `want` (none: no call); a problem whose QP is
    not positive definite (ok = 0) gets gradient 0, not NaN -> {name: gradient}."""
    if not want:
        return {}
    res = ctx.opt.plan_vjp(ctx.dyn, gbar, z=ctx.z, terminal_weights=ctx.terminal_weights, want=want, want_ok=True)
    live = res["ok"] != 0
    return {name: torch.where(live, res[name], torch.zeros_like(res[name])) for name in want}


class _PlanVjpFunction(torch.autograd.Function):
    """u[:n_rows] of a finished step as a function of x0 and the [B] set-point: backward is one plan_vjp call at the step's
    own solution (BatchOptimization.step_differentiable)."""

    INPUTS = ("opt", "u_all", "n_rows", "z", "dyn", "tw_kept", "x0", "set_point")   # forward's, in its order

    @staticmethod
    def forward(ctx, opt, u_all, n_rows, z, dyn, tw_kept, x0, set_point):
        ctx.opt, ctx.z, ctx.dyn, ctx.terminal_weights = opt, z, dyn, tw_kept
        return u_all[:n_rows].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gbar):
        inputs = _PlanVjpFunction.INPUTS
        grads = _masked_plan_vjp(ctx, gbar.contiguous(), _needing_grad(ctx, inputs, ("x0", "set_point")))
        return tuple(grads.get(name) for name in inputs)


class _PlanWeightVjpFunction(torch.autograd.Function):
    """_PlanVjpFunction with terminal_weights as a third differentiable input: backward adds one plan_weight_vjp call at the
    step's z, x0, set-point and u_prev (BatchOptimization.step_differentiable(weight_grad=True))."""

    INPUTS = ("opt", "u_all", "n_rows", "z", "dyn", "tw_kept", "x0_kept", "sp_kept", "u_prev", "x0", "set_point",
              "terminal_weights")   # forward's, in its order

    @staticmethod
    def forward(ctx, opt, u_all, n_rows, z, dyn, tw_kept, x0_kept, sp_kept, u_prev, x0, set_point, terminal_weights):
        ctx.opt, ctx.z, ctx.dyn, ctx.terminal_weights = opt, z, dyn, tw_kept
        ctx.x0, ctx.set_point, ctx.u_prev = x0_kept, sp_kept, u_prev
        return u_all[:n_rows].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gbar):
        inputs = _PlanWeightVjpFunction.INPUTS
        gbar = gbar.contiguous()
        grads = _masked_plan_vjp(ctx, gbar, _needing_grad(ctx, inputs, ("x0", "set_point")))
        if _needing_grad(ctx, inputs, ("terminal_weights",)):
            res = ctx.opt.plan_weight_vjp(ctx.x0, ctx.dyn, gbar, set_point=ctx.set_point, u_prev=ctx.u_prev, z=ctx.z,
                                          terminal_weights=ctx.terminal_weights, want=("terminal",), want_ok=True)
            grads["terminal_weights"] = torch.where(res["ok"] != 0, res["terminal"], torch.zeros_like(res["terminal"]))
        return tuple(grads.get(name) for name in inputs)


def _fext(fext):
    return None if fext is None else capi.dbl_array(fext, 4)


def _model_dims(model):
    lib = capi.load()
    m = capi.MODELS[model]
    return m, lib.cpmpc_model_state_dim(m), lib.cpmpc_model_num_params(m)


def dynamics_batch(dyn, x, u, fext=None, jacobians=True, model="single"):
    """Forward dynamics batched (gen::single_pendulum_dynamics or the generated double pendulum):
    x [nx,B], u [B] -> f [nx,B] (+ Jx [nx,nx,B], Ju [nx,B])."""
    m, nx, npar = _model_dims(model)
    dt = x.dtype
    _require_cuda_tensor(x, "x", dt)
    B = int(x.shape[1])
    if x.shape[0] != nx:
        raise ValueError("x must be [%d, B]" % nx)
    _require_cuda_tensor(u, "u", dt, (B,))
    f = torch.empty_like(x)
    Jx = torch.empty((nx, nx, B), dtype=dt, device=x.device) if jacobians else None
    Ju = torch.empty((nx, B), dtype=dt, device=x.device) if jacobians else None
    with torch.cuda.device(x.device):
        capi.check(capi.load().cpmpc_dynamics_batch_model(m, _CAPI_DTYPE[dt], B, capi.dbl_array(dyn, npar), _ptr(x),
                                                          _ptr(u), _fext(fext), _ptr(f), _ptr(Jx), _ptr(Ju),
                                                          _stream_ptr()))
    return (f, Jx, Ju) if jacobians else f


def rk4_batch(dyn, x, u, h, fext=None, jacobians=True, model="single"):
    """runge_kutta_4th_order<D> (or _no_jacobians) batched: -> x_new [nx,B] (+ A [nx,nx,B], B [nx,B])."""
    m, nx, npar = _model_dims(model)
    dt = x.dtype
    _require_cuda_tensor(x, "x", dt)
    B = int(x.shape[1])
    if x.shape[0] != nx:
        raise ValueError("x must be [%d, B]" % nx)
    _require_cuda_tensor(u, "u", dt, (B,))
    xn = torch.empty_like(x)
    A = torch.empty((nx, nx, B), dtype=dt, device=x.device) if jacobians else None
    Bm = torch.empty((nx, B), dtype=dt, device=x.device) if jacobians else None
    with torch.cuda.device(x.device):
        capi.check(capi.load().cpmpc_rk4_batch_model(m, _CAPI_DTYPE[dt], B, capi.dbl_array(dyn, npar), _ptr(x),
                                                     _ptr(u), float(h), _fext(fext), _ptr(xn), _ptr(A), _ptr(Bm),
                                                     _stream_ptr()))
    return (xn, A, Bm) if jacobians else xn


def feedback_apply(u_nom, K0, x_nom, x, u_limit=300.0, model="single", out=None):
    """u [B] = clamp(u_nom + K0 . wrap(x - x_nom), +-u_limit): row 0 of BatchOptimization.feedback_gain() applied to the
    deviation of the state x [nx, B] from the state x_nom [nx, B] the plan was made for (pole-angle differences wrapped);
    u_nom [B], K0 [nx, B].  One elementwise launch (cpmpc_feedback_apply_batch)."""
    m, nx, _ = _model_dims(model)
    dt = x.dtype
    _require_cuda_tensor(x, "x", dt)
    if x.dim() != 2 or x.shape[0] != nx:
        raise ValueError("x must be [%d, B]" % nx)
    B = int(x.shape[1])
    _require_cuda_tensor(x_nom, "x_nom", dt, (nx, B))
    _require_cuda_tensor(K0, "K0", dt, (nx, B))
    _require_cuda_tensor(u_nom, "u_nom", dt, (B,))
    if out is None:
        out = torch.empty((B,), dtype=dt, device=x.device)
    else:
        _require_cuda_tensor(out, "out", dt, (B,))
    with torch.cuda.device(x.device):
        capi.check(capi.load().cpmpc_feedback_apply_batch(_CAPI_DTYPE[dt], m, B, _ptr(u_nom), _ptr(K0), _ptr(x_nom),
                                                          _ptr(x), float(u_limit), _ptr(out), _stream_ptr()))
    return out


def plan_update(u_nom, K=None, x_nom=None, x=None, k_sp=None, sp_nom=None, sp=None, k_up=None, u_prev_nom=None, u_prev=None,
                u_limit=300.0, model="single", out=None):
    """The first-order re-plan of the whole horizon from BatchOptimization.plan_sensitivity()'s outputs, rows k < n_rows:
    u [n_rows, B] = clamp(u_nom + K . wrap(x - x_nom) + k_sp (sp - sp_nom) + k_up (u_prev - u_prev_nom), +-u_limit).
    u_nom [n_rows, B]; K [n_rows, nx, B] with x_nom, x [nx, B]; k_sp [n_rows, B] with sp_nom, sp [B]; k_up [n_rows, B] with
    u_prev_nom, u_prev [B].  A term whose sensitivity is None is absent; out may be u_nom.  One elementwise launch
    (cpmpc_plan_update_batch)."""
    m, nx, _ = _model_dims(model)
    dt = u_nom.dtype
    _require_cuda_tensor(u_nom, "u_nom", dt)
    if u_nom.dim() != 2:
        raise ValueError("u_nom must be [n_rows, B]")
    n_rows, B = int(u_nom.shape[0]), int(u_nom.shape[1])
    a = capi.PlanUpdate(struct_size=C.sizeof(capi.PlanUpdate), u_limit=float(u_limit))
    a.u_nom = u_nom.data_ptr()

    def give(name, t, shape):
        if t is not None:
            _require_cuda_tensor(t, name, dt, shape)
            setattr(a, name, t.data_ptr())
    give("K", K, (n_rows, nx, B))
    give("x_nom", x_nom, (nx, B))
    give("x", x, (nx, B))
    give("k_sp", k_sp, (n_rows, B))
    give("sp_nom", sp_nom, (B,))
    give("sp", sp, (B,))
    give("k_up", k_up, (n_rows, B))
    give("u_prev_nom", u_prev_nom, (B,))
    give("u_prev", u_prev, (B,))
    if out is None:
        out = torch.empty((n_rows, B), dtype=dt, device=u_nom.device)
    else:
        _require_cuda_tensor(out, "out", dt, (n_rows, B))
    a.u_out = out.data_ptr()
    with torch.cuda.device(u_nom.device):
        capi.check(capi.load().cpmpc_plan_update_batch(_CAPI_DTYPE[dt], m, B, n_rows, C.byref(a), _stream_ptr()))
    return out


def _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a=None, ticks=False, u_field="u"):
    """What every plant call reads, checked: state [nx, B]; u [B], or with `ticks` [T, B], T >= 1; fext None or [4, B];
    params np floats or an [np, B] tensor (None: the caller marshals them itself), for dims = _model_dims(model).  Where a
    struct `a` is given they are set on it: the step structs call the state `state`, the rollout structs `x0`; the controls
    go to `u_field` (cpmpc_sim_rollout_fb calls them u_nom).
    -> (B, T, host params or None, device pointer of the params or None, the shared forces as the host array that the call
    reads before it returns: the caller holds it, and the host params, until then)."""
    _, nx, npar = dims
    dtp = state.dtype
    _require_cuda_tensor(state, "state", dtp)
    shape = state.shape
    if len(shape) != 2 or shape[0] != nx:
        raise ValueError("state must be [%d, B]" % nx)
    B, T = shape[1], 1
    if ticks:
        _require_cuda_tensor(u, u_field, dtp)
        if u.dim() != 2 or u.shape[0] < 1 or u.shape[1] != B:
            raise ValueError("%s must be [T, B] with T >= 1" % u_field)
        T = u.shape[0]
    else:
        _require_cuda_tensor(u, "u", dtp, (B,))
    if fext is not None:
        _require_cuda_tensor(fext, "fext", dtp, (4, B))
    host = dev = None
    if isinstance(params, torch.Tensor):
        _require_cuda_tensor(params, "params", dtp, (npar, B))
        dev = params.data_ptr()
    elif params is not None:
        host = capi.dbl_array(params, npar)
    shared = capi.dbl_array([f_base[0], f_base[1], f_mass[0], f_mass[1]], 4)
    if a is not None:
        setattr(a, "x0" if ticks else "state", state.data_ptr())
        setattr(a, u_field, u.data_ptr())
        a.fext_host = C.cast(shared, C.POINTER(C.c_double))
        if fext is not None:
            a.fext = fext.data_ptr()
        if dev is not None:
            a.dyn = dev
    return B, T, host, dev, shared


def _sim_jac_call(params, dt, state, u, fext, f_base, f_mass, model, gbar, names):
    """One cpmpc_sim_step_jac_batch call on the current stream for the outputs in `names` (fields of cpmpc_sim_jac)."""
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimJac(struct_size=C.sizeof(capi.SimJac))
    B, _, _, _, _held = _plant_inputs(dims, state, u, None, fext, f_base, f_mass, a)   # the call takes shared params only
    if gbar is not None:
        _require_cuda_tensor(gbar, "gbar", dtp, (nx, B))
        a.gbar = gbar.data_ptr()
    res = _alloc_outputs(a, names, {"x_new": ("x_new", (nx, B)), "A": ("A", (nx, nx, B)), "Bu": ("Bu", (nx, B)),
                                    "gx": ("gx", (nx, B)), "gu": ("gu", (B,))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_step_jac_batch(m, _CAPI_DTYPE[dtp], B, capi.dbl_array(params, npar), float(dt),
                                                        C.byref(a), _stream_ptr()))
    return res


def sim_step_jacobian(params, dt, state, u, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single",
                      want=("x_new", "A", "Bu")):
    """BatchSimulator.step's map x+ = plant(x, u) with its first derivatives (include/cpmpc.h: cpmpc_sim_step_jac_batch):
    for state [nx, B] (read, not changed) and u [B] a dict with the entries named in `want`,
        "x_new" [nx, B]      the state after dt (the simulator's sub-steps: 1 ms, a shorter last one, angles wrapped),
        "A"     [nx, nx, B]  dx+/dx,
        "Bu"    [nx, B]      dx+/du, the control held over the step,
    the product of the sub-steps' RK4 Jacobians.  params, dt, f_base / f_mass / fext as BatchSimulator.step's.  Not
    differentiated here: the dynamics parameters (sim_step_param_jacobian does that), the external forces and dt.  Only
    what is named is computed."""
    want = _want_tuple(want, ("x_new", "A", "Bu"))
    return _sim_jac_call(params, dt, state, u, fext, f_base, f_mass, model, None, want)


def sim_step_vjp(params, dt, state, u, gbar, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single",
                 want=("x", "u")):
    """The reverse mode of sim_step_jacobian: a cotangent gbar = dL/dx+ [nx, B] on the state after the step pulled back to
    the inputs named in `want` -- a dict with
        "x" [nx, B]  A^T gbar,
        "u" [B]      Bu . gbar.
    A and Bu are contracted in registers and never written to memory: one kernel.  Not differentiated here: the dynamics
    parameters (sim_step_param_vjp does that), the external forces and dt.  Other arguments as sim_step_jacobian's."""
    want = _want_tuple(want, ("x", "u"))
    res = _sim_jac_call(params, dt, state, u, fext, f_base, f_mass, model, gbar, ["g" + w for w in want])
    return {w: res["g" + w] for w in want}


def _plant_step(dims, dt, state, u, params, fext, f_base, f_mass, out):
    """The plant step from `state` under u, in place on `out` (`state` itself, or a copy of it): np floats ->
    cpmpc_sim_step_batch_model, as ever; an [np, B] tensor -> cpmpc_sim_step_dyn_batch (per-problem parameters)."""
    B, _, host, dev, shared = _plant_inputs(dims, state, u, params, fext, f_base, f_mass)
    dtype = _CAPI_DTYPE[state.dtype]
    with torch.cuda.device(state.device):
        if dev is not None:
            capi.check(capi.load().cpmpc_sim_step_dyn_batch(dims[0], dtype, B, None, C.c_void_p(dev), float(dt), _ptr(u),
                                                            shared, _ptr(fext), _ptr(out), _stream_ptr()))
        else:
            capi.check(capi.load().cpmpc_sim_step_batch_model(dims[0], dtype, B, host, float(dt), _ptr(u), shared,
                                                              _ptr(fext), _ptr(out), _stream_ptr()))


def _sim_param_call(params, dt, state, u, fext, f_base, f_mass, model, gbar, names):
    """One cpmpc_sim_step_param_jac_batch call on the current stream for the outputs in `names` (fields of
    cpmpc_sim_param_jac)."""
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimParamJac(struct_size=C.sizeof(capi.SimParamJac))
    B, _, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a)
    if gbar is not None:
        _require_cuda_tensor(gbar, "gbar", dtp, (nx, B))
        a.gbar = gbar.data_ptr()
    res = _alloc_outputs(a, names, {"x_new": ("x_new", (nx, B)), "P": ("P", (nx, npar, B)), "gp": ("gp", (npar, B)),
                                    "gx": ("gx", (nx, B)), "gu": ("gu", (B,))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_step_param_jac_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), C.byref(a),
                                                              _stream_ptr()))
    return res


def sim_step_param_jacobian(params, dt, state, u, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single",
                            want=("x_new", "P")):
    """The plant step's derivative in the dynamics parameters (include/cpmpc.h: cpmpc_sim_step_param_jac_batch): for state
    [nx, B] (read, not changed) and u [B] a dict with the entries named in `want`,
        "x_new" [nx, B]      the state after dt,
        "P"     [nx, np, B]  dx+/dp, p in the order of the parameter vector (9 numbers for the 4-state model, 6 for the
                             6-state one).
    params: np floats (one plant for all) or an [np, B] tensor (a plant per problem).  First derivatives of the accelerations
    only; the control and the external forces are held, the wrap has unit derivative.  Not differentiated: the external
    forces and dt."""
    want = _want_tuple(want, ("x_new", "P"))
    return _sim_param_call(params, dt, state, u, fext, f_base, f_mass, model, None, want)


def sim_step_param_vjp(params, dt, state, u, gbar, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single",
                       want=("p", "x", "u")):
    """The reverse mode of sim_step_param_jacobian and sim_step_jacobian in one call: a cotangent gbar = dL/dx+ [nx, B]
    pulled back to the inputs named in `want` -- a dict with
        "p" [np, B]  P^T gbar (per problem, also where params is one shared set: sum over the batch for its gradient),
        "x" [nx, B]  A^T gbar,
        "u" [B]      Bu . gbar.
    P, A and Bu are contracted in registers and never written to memory.  params as sim_step_param_jacobian's."""
    want = _want_tuple(want, ("p", "x", "u"))
    res = _sim_param_call(params, dt, state, u, fext, f_base, f_mass, model, gbar, ["g" + w for w in want])
    return {w: res["g" + w] for w in want}


_PLANT_INPUTS = ("state", "u", "params", "dt", "fext", "f_base", "f_mass", "model")   # forward's, of both plant functions
_PLANT_GRADS = {"state": "x", "u": "u", "params": "p"}   # a differentiable input -> its name in the vjp calls' `want`


def _freeze_plant_args(ctx, params, dt, fext, f_base, f_mass, model):
    """The forward's own copies of what its backward passes on beside (state, u): later changes by the caller do not reach
    an earlier graph."""
    ctx.args = (params.detach().clone() if isinstance(params, torch.Tensor) else [float(v) for v in params], float(dt),
                None if fext is None else fext.detach().clone(), tuple(f_base), tuple(f_mass), model)


def _plant_backward(ctx, vjp):
    """The gradients of a plant function from one `vjp` call for those of its differentiable inputs that need one (none: no
    call; parameters given as numbers never do), as backward's return value."""
    want = [_PLANT_GRADS[n] for n in _needing_grad(ctx, _PLANT_INPUTS, _PLANT_GRADS)]
    res = vjp(want) if want else {}
    return tuple(res.get(_PLANT_GRADS.get(name)) for name in _PLANT_INPUTS)


class _SimStepFunction(torch.autograd.Function):
    """The plant step as a function of (state, u) and, where params is a tensor, of the parameters: forward is the
    simulator's own kernel on a copy, backward one sim_step_vjp (or, with a params tensor, sim_step_param_vjp) call at the
    saved inputs (sim_step)."""

    @staticmethod
    def forward(ctx, state, u, params, dt, fext, f_base, f_mass, model):
        _freeze_plant_args(ctx, params, dt, fext, f_base, f_mass, model)
        ctx.save_for_backward(state.detach().clone(), u.detach().clone())
        out = state.detach().clone()
        _plant_step(_model_dims(model), dt, state, u, params, fext, f_base, f_mass, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gbar):
        state, u = ctx.saved_tensors
        params, dt, fext, f_base, f_mass, model = ctx.args
        # per-problem parameters: one sim_step_param_vjp call for every gradient asked for
        call = sim_step_param_vjp if isinstance(params, torch.Tensor) else sim_step_vjp
        return _plant_backward(ctx, lambda want: call(params, dt, state, u, gbar.contiguous(), fext=fext, f_base=f_base,
                                                      f_mass=f_mass, model=model, want=want))


def sim_step(params, dt, state, u, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single"):
    """BatchSimulator.step as a differentiable function: returns the state [nx, B] after dt, bitwise what
    BatchSimulator.step leaves in a simulator set to `state` (the same kernel, on a copy; `state` is not changed),
    attached to the autograd graph of state and u.  Backward is one sim_step_vjp call on the current stream at the
    forward's own copies of (state, u) and is differentiable once only.  The wrap of the pole angles has unit derivative.

    params: np floats -- gradients flow to state and u alone, everything bitwise as before -- or an [np, B] tensor of
    per-problem parameters (cpmpc_sim_step_dyn_batch).  When that tensor requires grad, backward makes one
    sim_step_param_vjp call and returns dL/dp [np, B] for it beside the gradients for state and u.  A SHARED parameter
    set that should receive a gradient is passed as p.expand(np, B).contiguous() of an [np, 1] tensor p by the caller:
    autograd then sums the per-problem gradients over the batch.  The external forces and dt are not differentiated."""
    return _SimStepFunction.apply(state, u, params, dt, fext, f_base, f_mass, model)


def sim_rollout_states(params, dt, state, u, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single", want=("xs",)):
    """T ticks of BatchSimulator.step in ONE launch (include/cpmpc.h: cpmpc_sim_rollout_batch): from state [nx, B] (read, not
    changed) under the controls u [T, B], u[t] held over tick t, a dict with the entries named in `want`,
        "xs"      [T, nx, B]  xs[t] = the state after tick t, what t + 1 step() calls leave,
        "x_final" [nx, B]     the state after the last tick.
    params, dt, f_base / f_mass / fext as BatchSimulator.step's, the same for every tick.  No autograd: sim_rollout has it."""
    want = _want_tuple(want, ("xs", "x_final"))
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimRollout(struct_size=C.sizeof(capi.SimRollout))
    B, T, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a, ticks=True)
    res = _alloc_outputs(a, want, {"xs": ("xs", (T, nx, B)), "x_final": ("x_final", (nx, B))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_rollout_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a), _stream_ptr()))
    return res


def sim_rollout_vjp(params, dt, state, u, xs, gbar=None, gbar_final=None, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0),
                    model="single", want=("x", "u", "p")):
    """The reverse mode of sim_rollout_states in ONE launch (include/cpmpc.h: cpmpc_sim_rollout_vjp_batch): cotangents
    gbar [T, nx, B] on every xs[t] and / or gbar_final [nx, B] on the last state pulled back to the inputs named in `want`
    -- a dict with
        "x" [nx, B]  dL/dstate,
        "u" [T, B]   dL/du,
        "p" [np, B]  dL/dparams (per problem, also where params is one shared set: sum over the batch for its gradient).
    xs [T, nx, B] is a sim_rollout_states call's at the same inputs (its last row is not read; None is allowed for T = 1).
    Reverse over the ticks, forward inside a tick; the tick's A, Bu and P are contracted in registers and nothing per tick
    goes to memory.  Not differentiated: the external forces and dt.  Other arguments as sim_rollout_states'."""
    want = _want_tuple(want, ("x", "u", "p"))
    if gbar is None and gbar_final is None:
        raise ValueError("one of gbar, gbar_final must be given")
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimRolloutVjp(struct_size=C.sizeof(capi.SimRolloutVjp))
    B, T, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a, ticks=True)
    if xs is not None:
        _require_cuda_tensor(xs, "xs", dtp, (T, nx, B))
        a.xs = xs.data_ptr()
    elif T > 1:
        raise ValueError("xs (a sim_rollout_states call's) is required when T > 1")
    if gbar is not None:
        _require_cuda_tensor(gbar, "gbar", dtp, (T, nx, B))
        a.gbar = gbar.data_ptr()
    if gbar_final is not None:
        _require_cuda_tensor(gbar_final, "gbar_final", dtp, (nx, B))
        a.gbar_final = gbar_final.data_ptr()
    res = _alloc_outputs(a, want, {"x": ("g_x0", (nx, B)), "u": ("g_u", (T, B)), "p": ("g_p", (npar, B))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_rollout_vjp_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a),
                                                           _stream_ptr()))
    return res


class _SimRolloutFunction(torch.autograd.Function):
    """T plant ticks as a function of (state, u) and, where params is a tensor, of the parameters: forward is one
    sim_rollout_states launch, backward one sim_rollout_vjp launch at the saved inputs and checkpoints (sim_rollout)."""

    @staticmethod
    def forward(ctx, state, u, params, dt, fext, f_base, f_mass, model):
        _freeze_plant_args(ctx, params, dt, fext, f_base, f_mass, model)
        x0, uu = state.detach().clone(), u.detach().clone()
        xs = sim_rollout_states(ctx.args[0], dt, x0, uu, fext=fext, f_base=f_base, f_mass=f_mass, model=model)["xs"]
        ctx.save_for_backward(x0, uu, xs)
        return xs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gbar):
        state, u, xs = ctx.saved_tensors
        params, dt, fext, f_base, f_mass, model = ctx.args
        return _plant_backward(ctx, lambda want: sim_rollout_vjp(params, dt, state, u, xs, gbar=gbar.contiguous(), fext=fext,
                                                                 f_base=f_base, f_mass=f_mass, model=model, want=want))


def sim_rollout(params, dt, state, u, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single"):
    """T ticks of BatchSimulator.step as ONE differentiable function: returns xs [T, nx, B], xs[t] the state after tick t
    under the controls u [T, B] (sim_rollout_states; `state` is not changed), attached to the autograd graph of state and u.
    Forward is one launch; backward is one sim_rollout_vjp launch on the current stream at the forward's own copies of
    (state, u) and its xs, and is differentiable once only.  A loss on the last state alone reads xs[-1].  The wrap of the
    pole angles has unit derivative.

    params: np floats -- gradients flow to state and u alone -- or an [np, B] tensor of per-problem parameters.  When that
    tensor requires grad, the same backward launch returns dL/dp [np, B] for it beside the gradients for state and u.  A
    SHARED parameter set that should receive a gradient is passed as p.expand(np, B).contiguous() of an [np, 1] tensor p by
    the caller: autograd then sums the per-problem gradients over the batch.  The external forces and dt are not
    differentiated."""
    return _SimRolloutFunction.apply(state, u, params, dt, fext, f_base, f_mass, model)


def _window_inputs(a, field, rec, weights, tick_weights, dtp, T, nx, B):
    """What the window calls read beside the plant's inputs, checked and set on the struct `a`: the recording `rec` [T, nx, B]
    as `field` ("x_obs" / "y"), weights (nx numbers) as w_host, tick_weights [T, B] as tick_w, each or None -> the weights as the
    host array that the call reads before it returns (the caller holds it until then), or None."""
    if rec is not None:
        _require_cuda_tensor(rec, field, dtp, (T, nx, B))
        setattr(a, field, rec.data_ptr())
    w_host = None
    if weights is not None:
        w_host = capi.dbl_array(weights, nx)
        a.w_host = C.cast(w_host, C.POINTER(C.c_double))
    if tick_weights is not None:
        _require_cuda_tensor(tick_weights, "tick_weights", dtp, (T, B))
        a.tick_w = tick_weights.data_ptr()
    return w_host


def _gauss_newton_call(struct, symbol, final, in_params, params, dt, state, u, x_obs, weights, tick_weights, fext, f_base, f_mass,
                       model, want):
    """`symbol`, a Gauss-Newton window call, on the current stream with a `struct`: the unknowns are the np parameters
    (in_params) or the initial state, `final` names d(last state)/d(unknowns)."""
    want = _want_tuple(want, ("cost", "g", "H", final, "x_final"))
    m, nx, npar = dims = _model_dims(model)
    n = npar if in_params else nx
    dtp = state.dtype
    a = struct(struct_size=C.sizeof(struct))
    B, T, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a, ticks=True)
    if x_obs is None and any(w in ("cost", "g", "H") for w in want):
        raise ValueError("x_obs (the recorded states) is required for cost, g and H")
    _w_held = _window_inputs(a, "x_obs", x_obs, weights, tick_weights, dtp, T, nx, B)
    res = _alloc_outputs(a, want, {"cost": ("cost", (B,)), "g": ("g", (n, B)), "H": ("H", (n, n, B)),
                                   final: (final, (nx, n, B)), "x_final": ("x_final", (nx, B))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(getattr(capi.load(), symbol)(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a), _stream_ptr()))
    return res


def sim_rollout_gauss_newton(params, dt, state, u, x_obs, weights=None, tick_weights=None, fext=None, f_base=(0.0, 0.0),
                             f_mass=(0.0, 0.0), model="single", want=("cost", "g", "H")):
    """The forward mode of sim_rollout_states in the parameters and the Gauss-Newton normal equations of an output-error fit
    of the window, in ONE launch (include/cpmpc.h: cpmpc_sim_rollout_gn_batch).  x_obs [T, nx, B] is the recording, x_obs[t]
    the measured state after tick t; with S = dx/dp carried over the ticks, r_t = wrap(x_obs[t] - xs[t]), W = diag(weights)
    and om_t = tick_weights[t], a dict with the entries named in `want`,
        "cost"    [B]          1/2 sum_t om_t r_t^T W r_t,
        "g"       [np, B]      dcost/dp = -sum_t om_t S_t^T W r_t,
        "H"       [np, np, B]  sum_t om_t S_t^T W S_t, exactly symmetric; the Gauss-Newton step is -H^-1 g,
        "S_final" [nx, np, B]  d(last state)/dp,
        "x_final" [nx, B]      the last state.
    weights: nx numbers >= 0 or None (ones); 0 says that state was not measured (positions only: (1, 1, 0, 0)).
    tick_weights: [T, B] or None (ones); 0 says that sample is missing.  x_obs holds finite numbers there all the same, and
    may be None where none of cost, g, H is asked for.  S never goes to memory and no per-tick Jacobian is formed.  params
    (np numbers or an [np, B] tensor; g and H are per problem either way), dt and the forces as sim_rollout_states'.
    Not differentiated: the external forces, dt and the state (sim_rollout_vjp has its gradient).

    Several recorded windows of one plant: lay them side by side as columns (2 B columns for two windows, the parameters
    repeated) and add the windows' cost, g and H in torch before solving; the kernel knows nothing of it."""
    return _gauss_newton_call(capi.SimRolloutGn, "cpmpc_sim_rollout_gn_batch", "S_final", True, params, dt, state, u, x_obs,
                              weights, tick_weights, fext, f_base, f_mass, model, want)

def _cholesky_solve_lanes(Hs, gs, pivot_floor=0.0):
    """x = H^-1 g per lane for k x k systems given as lists of [B] tensors (Hs[j][i], i <= j, is read), solved on the
    diagonally scaled matrix by a Cholesky factorisation written out elementwise -> (x as k tensors, pd [B] bool).  pd is
    False where a pivot is not positive (or not a number); x is meaningless there.  pivot_floor: a pivot of the scaled
    matrix (unit diagonal) at or below it counts as not positive -- what rounding leaves of an exactly singular H."""
    k = len(gs)
    pd = torch.ones_like(gs[0], dtype=torch.bool)
    one = torch.ones_like(gs[0])
    s = []
    for j in range(k):
        pd = pd & (Hs[j][j] > 0)
        s.append(torch.rsqrt(torch.where(Hs[j][j] > 0, Hs[j][j], one)))
    L = [[None] * k for _ in range(k)]
    for j in range(k):
        d = Hs[j][j] * s[j] * s[j]
        for q in range(j):
            d = d - L[j][q] * L[j][q]
        pd = pd & (d > pivot_floor)
        L[j][j] = torch.sqrt(torch.where(d > 0, d, one))
        for i in range(j + 1, k):
            v = Hs[i][j] * s[i] * s[j]
            for q in range(j):
                v = v - L[i][q] * L[j][q]
            L[i][j] = v / L[j][j]
    y = []
    for j in range(k):
        v = gs[j] * s[j]
        for q in range(j):
            v = v - L[j][q] * y[q]
        y.append(v / L[j][j])
    x = [None] * k
    for j in range(k - 1, -1, -1):
        v = y[j]
        for q in range(j + 1, k):
            v = v - L[q][j] * x[q]
        x[j] = v / L[j][j]
    return [x[j] * s[j] for j in range(k)], pd


def sim_identify(params, dt, state, u, x_obs, columns, iterations=8, damping=0.0, weights=None, tick_weights=None, fext=None,
                 f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single"):
    """Identifies the parameters named by `columns` (indices into the parameter vector, k <= np of them) of B plants from a
    recorded window each, all B in lock-step on the device: the output-error fit  min_p 1/2 sum_t om_t r_t^T W r_t  of
    sim_rollout_gauss_newton by Gauss-Newton (damping = 0) or Levenberg-Marquardt (damping > 0).  params (np numbers or an
    [np, B] tensor, not changed) is the starting point; the other parameters stay as given.

    Per iteration one sim_rollout_gauss_newton launch at the trial parameters, then per lane the k x k sub-system of
    `columns` solved by a Cholesky factorisation written in elementwise torch (Python loops over k, no batched-LAPACK
    backend, no host synchronisation).  damping = 0: every step is taken.  damping > 0: the step solves
    (H + mu diag(H)) d = -g with a per-lane mu that starts at `damping`; a lane takes its step only where its cost falls and
    then divides mu by 10, else it stays and multiplies mu by 10 -- so a rejected step spends its iteration and one more to
    win mu back: give a damped run about twice the iterations of an undamped one.  iterations + 1 launches in all.

    Returns a dict: "params" [np, B], "cost" [B] at those parameters, "ok" [B] int32 -- 0 where the sub-block of H was not
    positive definite or the lane's data were not finite.  Such a lane stops there and keeps the parameters it had (those
    given, if that was at the first iteration); no other lane is affected.  weights, tick_weights and the remaining
    arguments as sim_rollout_gauss_newton's, where several windows per plant are described too."""
    m, nx, npar = _model_dims(model)
    cols = [int(c) for c in columns]
    if not cols or len(set(cols)) != len(cols) or any(c < 0 or c >= npar for c in cols):
        raise ValueError("columns must name between 1 and %d distinct parameters in [0, %d)" % (npar, npar))
    if not (float(damping) >= 0.0):
        raise ValueError("damping must be >= 0")
    dtp = state.dtype
    _require_cuda_tensor(state, "state", dtp)
    B = int(state.shape[-1])
    if isinstance(params, torch.Tensor):
        _require_cuda_tensor(params, "params", dtp, (npar, B))
        p = params.detach().clone()
    else:
        p = torch.tensor(list(capi.dbl_array(params, npar)), dtype=dtp, device=state.device).reshape(npar, 1).repeat(1, B)

    def evaluate(q):
        return sim_rollout_gauss_newton(q, dt, state, u, x_obs, weights=weights, tick_weights=tick_weights, fext=fext,
                                        f_base=f_base, f_mass=f_mass, model=model)

    p, cur, live = _gauss_newton_lanes(evaluate, p, cols, iterations, damping, ("cost", "g", "H"))
    return {"params": p, "cost": cur["cost"], "ok": live.to(torch.int32)}


def _gauss_newton_lanes(evaluate, p, cols, iterations, damping, names, pivot_floor=0.0):
    """The accept / reject loop of sim_identify and sim_estimate_state: B independent fits in lock-step, rows `cols` of the
    unknowns p [n, B] moving.  evaluate(q) -> a dict with "cost" [B], "g" [n, B], "H" [n, n, B] and whatever else `names`
    lists, at the trial point q; one call before the loop and one per iteration.  Per iteration the len(cols)-square
    sub-system per lane through _cholesky_solve_lanes, (H + mu diag(H)) d = -g with the per-lane mu of sim_identify's
    docstring where damping > 0.  A lane whose data are not finite or whose sub-block of H is not positive definite stops
    and keeps what it had; pivot_floor as _cholesky_solve_lanes'.  -> (p, the entries `names` at p, live [B] bool)."""
    cur = evaluate(p)
    live = torch.isfinite(cur["cost"])
    mu = torch.full_like(cur["cost"], float(damping))
    for _ in range(int(iterations)):
        H, g = cur["H"], cur["g"]
        Hs = [[H[cj, ci] * (1.0 + mu) if ci == cj else H[cj, ci] for ci in cols] for cj in cols]
        delta, pd = _cholesky_solve_lanes(Hs, [g[c] for c in cols], pivot_floor)
        for d in delta:
            pd = pd & torch.isfinite(d)
        live = live & pd
        trial = p.clone()
        for c, d in zip(cols, delta):
            trial[c] = torch.where(live, p[c] - d, p[c])
        new = evaluate(trial)
        if damping > 0.0:
            take = live & (new["cost"] < cur["cost"])
            mu = torch.where(take, mu * 0.1, mu * 10.0)
        else:
            take = live & torch.isfinite(new["cost"])
            live = take
        p = torch.where(take, trial, p)
        cur = {name: torch.where(take, new[name], cur[name]) for name in names}
    return p, cur, live


def sim_rollout_gauss_newton_x0(params, dt, state, u, x_obs, weights=None, tick_weights=None, fext=None, f_base=(0.0, 0.0),
                                f_mass=(0.0, 0.0), model="single", want=("cost", "g", "H")):
    """The forward mode of sim_rollout_states in the INITIAL STATE and the Gauss-Newton normal equations of an output-error
    fit of it over the window, in ONE launch (include/cpmpc.h: cpmpc_sim_rollout_gn_x0_batch): the state-estimation half of
    sim_rollout_gauss_newton.  x_obs [T, nx, B] is the recording, x_obs[t] the measured state after tick t; with
    Phi_t = dxs[t]/dstate carried over the ticks, r_t = wrap(x_obs[t] - xs[t]), W = diag(weights) and om_t = tick_weights[t], a
    dict with the entries named in `want`,
        "cost"      [B]          1/2 sum_t om_t r_t^T W r_t,
        "g"         [nx, B]      dcost/dstate = -sum_t om_t Phi_t^T W r_t,
        "H"         [nx, nx, B]  sum_t om_t Phi_t^T W Phi_t, exactly symmetric; the Gauss-Newton step is -H^-1 g,
        "Phi_final" [nx, nx, B]  d(last state)/dstate, the product of the ticks' sim_step_jacobian A,
        "x_final"   [nx, B]      the last state.
    weights: nx numbers >= 0 or None (ones); 0 says that state was not measured (positions only: (1, 1, 0, 0)).
    tick_weights: [T, B] or None (ones); 0 says that sample is missing.  x_obs holds finite numbers there all the same, and
    may be None where none of cost, g, H is asked for.  Phi never goes to memory and no per-tick Jacobian is formed.  params
    (np numbers or an [np, B] tensor), dt and the forces as sim_rollout_states'.  Not differentiated: the parameters
    (sim_rollout_gauss_newton), the external forces and dt."""
    return _gauss_newton_call(capi.SimRolloutGnX0, "cpmpc_sim_rollout_gn_x0_batch", "Phi_final", False, params, dt, state, u,
                              x_obs, weights, tick_weights, fext, f_base, f_mass, model, want)

def _wrap_pole_angles(d, nx):
    """d [nx, B], a difference of states: its pole angles to the nearest multiple of 2 pi, as the kernels wrap a residual"""
    nq = nx // 2
    if nq > 1:
        d = d.clone()
        d[1:nq] = d[1:nq] - 2.0 * 3.14159265358979323846 * torch.round(d[1:nq] / (2.0 * 3.14159265358979323846))
    return d


def sim_estimate_state(params, dt, state, u, x_obs, iterations=8, damping=0.0, weights=None, tick_weights=None, prior=None,
                       prior_info=None, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single"):
    """Estimates the state at the START of a recorded window of B plants, all B in lock-step on the device: the output-error
    fit  min_x0 1/2 sum_t om_t r_t^T W r_t (+ the arrival cost)  of sim_rollout_gauss_newton_x0 by Gauss-Newton
    (damping = 0) or Levenberg-Marquardt (damping > 0).  `state` [nx, B] (not changed) is the starting guess of x0; u [T, B]
    the controls that were applied and x_obs [T, nx, B] the measurements after every tick; weights says which states were
    measured (positions only: (1, 1, 0, 0) -- the unmeasured rows of x_obs are not used but must be finite).

    Per iteration one sim_rollout_gauss_newton_x0 launch at the trial x0, then the nx x nx system per lane by the Cholesky
    factorisation of sim_identify, with its accept / reject rule and per-lane mu (the loop is the same function);
    iterations + 1 launches in all, no host synchronisation.  Give a damped run about twice the iterations.

    The arrival cost 1/2 (x0 - prior)^T Pi (x0 - prior), with prior [nx, B] and Pi = prior_info [nx, B] (a diagonal) or
    [nx, nx, B] (symmetric), both or neither: the pole angles of the difference are wrapped, and it is added to cost, g and H
    in torch; the kernel knows nothing of it.

    Returns a dict: "x0" [nx, B] the estimate of the window's first state, "x_final" [nx, B] the state after the window's last
    tick from there -- the estimate of the CURRENT state, which is what a controller wants (ClosedLoop.set_state) -- "cost"
    [B], "H" [nx, nx, B] at the estimate with the prior included (its inverse is the estimate's covariance in units of the
    measurement variance) and "ok" [B] int32 -- 0 where H was not positive definite (a pivot of the diagonally scaled H at or below
    8 nx eps: the window does not determine x0) or the lane's data were not finite.  Such a lane keeps its guess; no other
    lane is affected.  The remaining arguments as sim_rollout_gauss_newton_x0's."""
    m, nx, npar = _model_dims(model)
    if not (float(damping) >= 0.0):
        raise ValueError("damping must be >= 0")
    if (prior is None) != (prior_info is None):
        raise ValueError("prior and prior_info are given together or not at all")
    dtp = state.dtype
    _require_cuda_tensor(state, "state", dtp)
    if state.dim() != 2 or state.shape[0] != nx:
        raise ValueError("state must be [%d, B]" % nx)
    B = int(state.shape[1])
    diag = None
    if prior is not None:
        _require_cuda_tensor(prior, "prior", dtp, (nx, B))
        _require_cuda_tensor(prior_info, "prior_info", dtp)
        if tuple(prior_info.shape) not in ((nx, B), (nx, nx, B)):
            raise ValueError("prior_info must be [%d, B] or [%d, %d, B]" % (nx, nx, nx))
        diag = prior_info.dim() == 2
        info = torch.diag_embed(prior_info.t()).permute(1, 2, 0).contiguous() if diag else prior_info

    def evaluate(q):
        res = sim_rollout_gauss_newton_x0(params, dt, q, u, x_obs, weights=weights, tick_weights=tick_weights, fext=fext,
                                          f_base=f_base, f_mass=f_mass, model=model, want=("cost", "g", "H", "x_final"))
        if prior is not None:
            d = _wrap_pole_angles(q - prior, nx)
            pd = prior_info * d if diag else torch.einsum("jkb,kb->jb", prior_info, d)
            res["cost"] = res["cost"] + 0.5 * (d * pd).sum(dim=0)
            res["g"] = res["g"] + pd
            res["H"] = res["H"] + info
        return res

    # an unobservable window (one tick of positions only) has an exactly singular H, of which rounding leaves pivots of
    # either sign at the size of 1 ulp of the scaled matrix's unit diagonal: those count as not positive
    x0, cur, live = _gauss_newton_lanes(evaluate, state.detach().clone(), list(range(nx)), iterations, damping,
                                        ("cost", "g", "H", "x_final"), pivot_floor=8 * nx * torch.finfo(dtp).eps)
    return {"x0": x0, "x_final": cur["x_final"], "cost": cur["cost"], "H": cur["H"], "ok": live.to(torch.int32)}


def sim_ekf(params, dt, state, cov, u, y, weights, process_noise=None, tick_weights=None, fext=None, f_base=(0.0, 0.0),
            f_mass=(0.0, 0.0), model="single", want=("x_final", "P_final")):
    """The extended Kalman filter of B plants over the T ticks of u [T, B], in ONE launch (include/cpmpc.h:
    cpmpc_sim_ekf_batch): the recursive counterpart of sim_estimate_state.  From `state` [nx, B] with covariance `cov`
    [nx, nx, B] (its lower triangle cov[j, k], k <= j, is what is read; neither is changed), per tick
        predict   x- = the plant's tick from x under u[t],   P- = A P A^T + diag(process_noise),  A the tick's
                  sim_step_jacobian A at the filtered x,
        update    one measured state i at a time, where rho_i = tick_weights[t] weights[i] > 0:
                  s = P_ii + 1 / rho_i,  nu = wrap(y[t][i] - x_i),  x += P[:, i] nu / s,  P -= P[:, i] P[i, :] / s.
    weights: nx numbers >= 0 (None: ones), the INVERSE VARIANCES of the measurements y [T, nx, B] (y[t] is what was measured
    after tick t) -- the convention of sim_rollout_gauss_newton_x0's weights; 0 says that state is not measured (encoders with
    0.01 rms noise: (1e4, 1e4, 0, 0)).  process_noise: nx variances >= 0 added to P's diagonal once a tick (None: zeros).
    tick_weights: [T, B] or None (ones); 0 says that sample is missing: x and P stay bitwise what the prediction left.  y may
    be None where every weight is 0.  The tick's A and the covariance stay on the device; no matrix is inverted.

    Returns a dict with the entries named in `want`,
        "x_final" [nx, B]      the filtered state after the last tick -- what ClosedLoop.set_state() takes,
        "P_final" [nx, nx, B]  its covariance, exactly symmetric,
        "xs"      [T, nx, B]   the filtered state after every tick,
        "nis"     [B]          the normalised squared innovations nu^2 / s added up: about one per scalar measurement where
                               weights and process_noise fit the data, far more where a sensor has failed.
    T = 1 is the per-tick filter (StateFilter) and the arrival-cost update of a moving horizon (WindowEstimator's prior_cov).
    params (np numbers or an [np, B] tensor), dt and the forces as sim_rollout_states'."""
    want = _want_tuple(want, ("x_final", "P_final", "xs", "nis"))
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimEkf(struct_size=C.sizeof(capi.SimEkf))
    B, T, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a, ticks=True)
    _require_cuda_tensor(cov, "cov", dtp, (nx, nx, B))
    a.P0 = cov.data_ptr()
    w_host = _window_inputs(a, "y", y, weights, tick_weights, dtp, T, nx, B)
    if y is None and (w_host is None or any(v > 0 for v in w_host)):
        raise ValueError("y (the measurements) is required where a weight is > 0")
    if process_noise is not None:
        q_host = capi.dbl_array(process_noise, nx)   # read by the call itself, before it returns
        a.q_host = C.cast(q_host, C.POINTER(C.c_double))
    res = _alloc_outputs(a, want, {"x_final": ("x_final", (nx, B)), "P_final": ("P_final", (nx, nx, B)),
                                   "xs": ("xs", (T, nx, B)), "nis": ("nis", (B,))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_ekf_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a), _stream_ptr()))
    return res


_RTS_OUTPUTS = ("xs_smooth", "Ps_smooth", "x0_smooth", "P0_smooth", "ok", "x_final", "P_final", "xs", "nis")


def _sim_rts_work_rows(model, ticks):
    """Rows of B numbers of sim_rts's workspace for `ticks` ticks, from the library's own cpmpc_sim_rts_work_rows (44 a tick for
    the 4-state model and 90 for the 6-state model): the record's layout is written down in one place."""
    m, _, _ = _model_dims(model)
    return int(capi.load().cpmpc_sim_rts_work_rows(m, int(ticks)))


def sim_rts(params, dt, state, cov, u, y, weights, process_noise=None, tick_weights=None, fext=None, f_base=(0.0, 0.0),
            f_mass=(0.0, 0.0), model="single", want=("xs_smooth", "x0_smooth", "P0_smooth"), work=None):
    """The Rauch-Tung-Striebel smoother of B plants over the T ticks of u [T, B], in TWO launches (include/cpmpc.h:
    cpmpc_sim_rts_batch): every state of the window given ALL of the window's measurements, with its covariance.  Forward it
    is sim_ekf on the same arguments, unchanged; index 0 is `state` / `cov` and index t is after tick t.  Backward from
    x^s_T = x_T, P^s_T = P_T, for t = T-1 .. 0, with x-, P- the prediction of tick t and A its Jacobian,
        G = P_t A^T (P-)^-1,   x^s_t = x_t + G wrap(x^s_{t+1} - x-),   P^s_t = P_t + G (P^s_{t+1} - P-) G^T.
    No inverse is formed (the Cholesky factor of the diagonally scaled P-, per lane in registers).  A tick whose P- is not
    positive definite (a pivot of the scaled matrix at or below 8 nx eps: sim_estimate_state's floor) takes G = 0: index t's
    smoothed values are its filtered ones, the recursion goes on from them and the lane's "ok" is 0 -- the answer for
    cov = 0, "the start is known".

    Returns a dict with the entries named in `want`,
        "xs_smooth" [T + 1, nx, B]      the smoothed states, index T is the filtered x_final,
        "Ps_smooth" [T + 1, nx, nx, B]  their covariances, exactly symmetric, index T is P_final,
        "x0_smooth" [nx, B], "P0_smooth" [nx, nx, B]   index 0 alone: the window's first state given the whole window,
        "ok"        [B] int32           1 where every tick's P- was positive definite,
        "x_final", "P_final", "xs", "nis"   sim_ekf's, bit for bit.
    Each is bitwise the same whichever others are asked for.

    THE WORKSPACE: the forward pass stores per tick what the backward pass reads -- the predicted state and covariance, the
    rows of A P, the filtered state and covariance: cpmpc_sim_rts_work_rows(model, T) rows of B numbers, 44 T for the 4-state and
    90 T for the 6-state model.  At B = 262 144, T = 100, 6-state fp64 that is 18.9 GB; at B = 4096 it is 0.29 GB.
    work=None allocates it for the call; a caller's contiguous tensor of `state`'s dtype with at least that many numbers
    per lane, [rows, B], is used instead and holds nothing of meaning afterwards.  The other arguments as sim_ekf's."""
    want = _want_tuple(want, _RTS_OUTPUTS)
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimRts(struct_size=C.sizeof(capi.SimRts))
    B, T, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a, ticks=True)
    _require_cuda_tensor(cov, "cov", dtp, (nx, nx, B))
    a.P0 = cov.data_ptr()
    w_host = _window_inputs(a, "y", y, weights, tick_weights, dtp, T, nx, B)
    if y is None and (w_host is None or any(v > 0 for v in w_host)):
        raise ValueError("y (the measurements) is required where a weight is > 0")
    if process_noise is not None:
        q_host = capi.dbl_array(process_noise, nx)   # read by the call itself, before it returns
        a.q_host = C.cast(q_host, C.POINTER(C.c_double))
    rows = _sim_rts_work_rows(model, T)
    if work is None:
        work = torch.empty((rows, B), dtype=dtp, device=state.device)
    else:
        _require_cuda_tensor(work, "work", dtp)
        if work.dim() != 2 or work.shape[1] != B or work.shape[0] < rows:
            raise ValueError("work must be [rows, B] with rows >= %d (cpmpc_sim_rts_work_rows), got %s" % (rows, tuple(work.shape)))
    a.work, a.work_rows = work.data_ptr(), int(work.shape[0])
    res = _alloc_outputs(a, [w for w in want if w != "ok"],
                         {"xs_smooth": ("xs_smooth", (T + 1, nx, B)), "Ps_smooth": ("Ps_smooth", (T + 1, nx, nx, B)),
                          "x0_smooth": ("x0_smooth", (nx, B)), "P0_smooth": ("P0_smooth", (nx, nx, B)),
                          "x_final": ("x_final", (nx, B)), "P_final": ("P_final", (nx, nx, B)),
                          "xs": ("xs", (T, nx, B)), "nis": ("nis", (B,))}, dtp, state.device)
    if "ok" in want:
        res["ok"] = torch.empty((B,), dtype=torch.int32, device=state.device)
        a.ok = res["ok"].data_ptr()
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_rts_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a), _stream_ptr()))
    return {name: res[name] for name in want}


def sim_lqr(params, dt, state, u, xs, q, r, terminal=None, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single",
            want=("K", "P0")):
    """The time-varying LQR gains along a plant trajectory in ONE launch (include/cpmpc.h: cpmpc_sim_lqr_batch): the backward
    Riccati recursion of the cost sum_t (d_t^T diag(q) d_t + r du_t^2) + d_T^T P_T d_T along the trajectory state [nx, B],
    u [T, B], xs [T, nx, B] -- a sim_rollout_states call's at the same inputs (its last row is not read; None is allowed for
    T = 1).  Per tick, last to first, with Phi and gamma the tick's sim_step_jacobian A and Bu at (x_t, u[t]):
        v = P gamma,  s = r + gamma . v,  k_t = -(Phi^T v) / s,  Acl = Phi + gamma k_t^T,
        P = diag(q) + r k_t k_t^T + Acl^T P Acl.
    The plant has one input: no matrix is inverted.  q: nx weights >= 0 (None: ones); r: the control weight, > 0.
    terminal: a tensor [nx, nx, B] for P_T (its lower triangle terminal[j, k], k <= j, is what is read: a call's "P0" chains
    windows), a list of nx weights >= 0 for a diagonal P_T, or None: diag(q).

    Returns a dict with the entries named in `want`,
        "K"  [T, nx, B]   K[t] = k_t, applied as u = u_nom[t] + K[t] . (x_t - x_nom_t): what sim_rollout_feedback takes,
        "P0" [nx, nx, B]  the cost-to-go at the window's start, exactly symmetric.
    The gains belong to the PLANT's map at dt (1 ms sub-steps, the control held over the tick), not to a controller's model of
    it; the clamp of the control and feedback inside a tick are not modelled.  dt = 0: K = 0, P0 = P_T + T diag(q).
    params (np numbers or an [np, B] tensor), dt and the forces as sim_rollout_states'."""
    want = _want_tuple(want, ("K", "P0"))
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimLqr(struct_size=C.sizeof(capi.SimLqr), r=float(r))
    B, T, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a, ticks=True)
    if xs is not None:
        _require_cuda_tensor(xs, "xs", dtp, (T, nx, B))
        a.xs = xs.data_ptr()
    elif T > 1:
        raise ValueError("xs (a sim_rollout_states call's) is required when T > 1")
    if q is not None:
        q_host = capi.dbl_array(q, nx)   # read by the call itself, before it returns
        a.q_host = C.cast(q_host, C.POINTER(C.c_double))
    if isinstance(terminal, torch.Tensor):
        _require_cuda_tensor(terminal, "terminal", dtp, (nx, nx, B))
        a.PT = terminal.data_ptr()
    elif terminal is not None:
        qf_host = capi.dbl_array(terminal, nx)
        a.qf_host = C.cast(qf_host, C.POINTER(C.c_double))
    res = _alloc_outputs(a, want, {"K": ("K", (T, nx, B)), "P0": ("P0", (nx, nx, B))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_lqr_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a), _stream_ptr()))
    return res


def sim_rollout_feedback(params, dt, state, u_nom, K, x0_nom, xs_nom, u_limit=float("inf"), fext=None, f_base=(0.0, 0.0),
                         f_mass=(0.0, 0.0), model="single", want=("xs", "us")):
    """T plant ticks under an affine feedback law in ONE launch (include/cpmpc.h: cpmpc_sim_rollout_fb_batch): from
    state [nx, B] (read, not changed), per tick
        d = wrap(x_t - x_nom_t),  u_t = clamp(u_nom[t] + K[t] . d, +-u_limit),  x_{t+1} = the plant's tick from x_t under u_t,
    with x_nom_0 = x0_nom [nx, B], x_nom_t = xs_nom[t - 1] (xs_nom [T, nx, B]: a sim_rollout_states call's; its last row is not
    read; None is allowed for T = 1) and the pole-angle differences wrapped to the nearest turn.  u_nom [T, B]; K [T, nx, B]
    is sim_lqr's "K", or None: no feedback (x0_nom and xs_nom are then not read).  u_limit > 0, infinity: no clamp.  The
    control is formed at the tick's start and held over it: there is no feedback inside a tick, and sim_lqr does not know of
    the clamp.  params and the forces are THIS call's own plant and may differ from those the nominal trajectory and the gains
    were made with: model mismatch is the point.

    Returns a dict with the entries named in `want`,
        "xs"      [T, nx, B]  the state after every tick,
        "x_final" [nx, B]     the state after the last tick,
        "us"      [T, B]      the controls applied.
    With K None and u_limit infinite, xs is sim_rollout_states' bit for bit; with state == x0_nom and the nominal trajectory's
    own parameters the call reproduces the nominal rollout bit for bit."""
    want = _want_tuple(want, ("xs", "x_final", "us"))
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimRolloutFb(struct_size=C.sizeof(capi.SimRolloutFb), u_limit=float(u_limit))
    B, T, host, _, _held = _plant_inputs(dims, state, u_nom, params, fext, f_base, f_mass, a, ticks=True, u_field="u_nom")
    if K is not None:
        _require_cuda_tensor(K, "K", dtp, (T, nx, B))
        a.K = K.data_ptr()
        if x0_nom is None:
            raise ValueError("x0_nom (the nominal start) is required where K is given")
        if xs_nom is None and T > 1:
            raise ValueError("xs_nom (a sim_rollout_states call's) is required where K is given and T > 1")
    if x0_nom is not None:
        _require_cuda_tensor(x0_nom, "x0_nom", dtp, (nx, B))
        a.x0_nom = x0_nom.data_ptr()
    if xs_nom is not None:
        _require_cuda_tensor(xs_nom, "xs_nom", dtp, (T, nx, B))
        a.xs_nom = xs_nom.data_ptr()
    res = _alloc_outputs(a, want, {"xs": ("xs", (T, nx, B)), "x_final": ("x_final", (nx, B)), "us": ("us", (T, B))}, dtp,
                         state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_rollout_fb_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a),
                                                          _stream_ptr()))
    return res


def _ilqr_reference(x_ref, T, nx, B, dtype, device):
    """x_ref -> a contiguous [T + 1, nx, B] tensor: row 0 the target of the start, row t of the state after tick t - 1 (row T
    the terminal target).  [T + 1, nx, B] is taken as it is; nx numbers (or an [nx] tensor) and [nx, B] are a constant target,
    expanded."""
    if not isinstance(x_ref, torch.Tensor):
        x_ref = torch.tensor([float(v) for v in x_ref], dtype=dtype, device=device)
    _require_cuda_tensor(x_ref, "x_ref", dtype, contiguous=False)
    if x_ref.shape == (T + 1, nx, B):
        return x_ref if x_ref.is_contiguous() else x_ref.contiguous()
    if x_ref.shape == (nx,):
        return x_ref.reshape(1, nx, 1).expand(T + 1, nx, B).contiguous()
    if x_ref.shape == (nx, B):
        return x_ref.reshape(1, nx, B).expand(T + 1, nx, B).contiguous()
    raise ValueError("x_ref must be [T + 1, %d, B] = [%d, %d, %d], [%d, B] or %d numbers" % (nx, T + 1, nx, B, nx, nx))


def _ilqr_cost(a, nx, B, T, dtp, device, x_ref, u_ref, q, terminal):
    """The cost's fields of the two iLQR structs (reference, weights, terminal cost) set on `a` -> what must stay alive until
    the call has returned."""
    ref = _ilqr_reference(x_ref, T, nx, B, dtp, device)
    a.x0_ref = ref[0].data_ptr()
    a.xs_ref = ref[1:].data_ptr()
    held = [ref]
    if u_ref is not None:
        _require_cuda_tensor(u_ref, "u_ref", dtp, (T, B))
        a.u_ref = u_ref.data_ptr()
    if q is not None:
        q_host = capi.dbl_array(q, nx)   # read by the call itself, before it returns
        a.q_host = C.cast(q_host, C.POINTER(C.c_double))
        held.append(q_host)
    if isinstance(terminal, torch.Tensor):
        _require_cuda_tensor(terminal, "terminal", dtp, (nx, nx, B))
        a.PT = terminal.data_ptr()
    elif terminal is not None:
        qf_host = capi.dbl_array(terminal, nx)
        a.qf_host = C.cast(qf_host, C.POINTER(C.c_double))
        held.append(qf_host)
    return held


def sim_ilqr_backward(params, dt, state, u, xs, x_ref, u_ref, q, r, terminal=None, mu=None, u_limit=float("inf"), fext=None,
                      f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single", want=("K", "kff", "dV")):
    """The backward pass of one iLQR iteration on the plant's tick map in ONE launch (include/cpmpc.h:
    cpmpc_sim_ilqr_backward_batch), along the trajectory state [nx, B], u [T, B], xs [T, nx, B] (a sim_ilqr_forward or
    sim_rollout_states call's; None is allowed for T = 1) for the cost, with no factor 1/2,
        J = sum_{t<T} (e_t^T diag(q) e_t + r (u_t - u_ref[t])^2) + e_T^T P_T e_T,    e_t = wrap(x_t - x_ref[t]).
    x_ref: [T + 1, nx, B] (row T the terminal target), or [nx, B] / nx numbers for a constant target; u_ref [T, B] or None:
    zeros; q, r and terminal as sim_lqr's; mu [B] >= 0 or None: the regularisation added to the control's curvature per
    problem; u_limit > 0: the box limit, handled inside the recursion (the plant has one input: a scalar clamp, exact), with
    no feedback on a control that sits on it.  Per tick, last to first, with g HALF the gradient of the cost-to-go:
        v = P gamma,  s0 = r + gamma . v,  s = s0 + mu,  h = r (u_t - u_ref[t]) + gamma . g,
        k_t = clamp(u_t - h / s) - u_t,  K_t = clamped ? 0 : -(Phi^T v) / s,  dV1 += 2 k_t h,  dV2 += k_t^2 s0,
        Acl = Phi + gamma K_t^T,  g = q o e_t + r (u_t - u_ref[t] + k_t) K_t + Acl^T (g + v k_t),
        P = diag(q) + r K_t K_t^T + Acl^T P Acl.

    Returns a dict with the entries named in `want`,
        "K"    [T, nx, B]  the gains, sim_lqr's convention,      "kff"  [T, B]  the feedforward terms k_t,
        "dV"   [2, B]      alpha dV[0] + alpha^2 dV[1] is the predicted change of J for a step alpha,
        "P0"   [nx, nx, B] and "g0" [nx, B]  the model's cost-to-go at the start, x^T P0 x + 2 g0 . x,
        "hmax" [B]         max_t |k_t| (s0 + mu): 0 at a stationary trajectory.
    With mu None and no limit, K and P0 are sim_lqr's; with x_ref the trajectory itself, kff and dV are exactly 0.  Gauss-Newton:
    second-order terms of the dynamics are not modelled.  params, dt and the forces as sim_rollout_states'."""
    names = ("K", "kff", "dV", "P0", "g0", "hmax")
    want = _want_tuple(want, names)
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimIlqrBackward(struct_size=C.sizeof(capi.SimIlqrBackward), r=float(r), u_limit=float(u_limit))
    B, T, host, _, _held = _plant_inputs(dims, state, u, params, fext, f_base, f_mass, a, ticks=True)
    if xs is not None:
        _require_cuda_tensor(xs, "xs", dtp, (T, nx, B))
        a.xs = xs.data_ptr()
    elif T > 1:
        raise ValueError("xs (a forward call's) is required when T > 1")
    _cost_held = _ilqr_cost(a, nx, B, T, dtp, state.device, x_ref, u_ref, q, terminal)
    if mu is not None:
        _require_cuda_tensor(mu, "mu", dtp, (B,))
        a.mu = mu.data_ptr()
    res = _alloc_outputs(a, want, {"K": ("K", (T, nx, B)), "kff": ("kff", (T, B)), "dV": ("dV", (2, B)),
                                   "P0": ("P0", (nx, nx, B)), "g0": ("g0", (nx, B)), "hmax": ("hmax", (B,))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_ilqr_backward_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a),
                                                             _stream_ptr()))
    return res


def sim_ilqr_forward(params, dt, state, u_nom, kff, K, x0_nom, xs_nom, x_ref, u_ref, q, r, terminal=None, alpha=None,
                     u_limit=float("inf"), fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single",
                     want=("xs", "us", "cost")):
    """The forward pass of one iLQR iteration in ONE launch (include/cpmpc.h: cpmpc_sim_ilqr_forward_batch): from
    state [nx, B] (read, not changed), per tick
        d = wrap(x_t - x_nom_t),  u_t = clamp(u_nom[t] + alpha kff[t] + K[t] . d, +-u_limit),  x_{t+1} = the plant's tick,
    with the cost J of sim_ilqr_backward summed on the device over the states passed and the controls applied.  kff [T, B] and
    K [T, nx, B] are sim_ilqr_backward's, each or None (K needs x0_nom [nx, B] and, for T > 1, xs_nom [T, nx, B], as
    sim_rollout_feedback); alpha [B]: the step on kff per problem, None: 1.  x_ref, u_ref, q, r, terminal: the cost, as
    sim_ilqr_backward's.  With kff and K None it is the plain clamped rollout with its cost.

    Returns a dict with the entries named in `want`,
        "xs" [T, nx, B],  "x_final" [nx, B],  "us" [T, B] the controls applied,  "cost" [B].
    With kff, K None and no limit, xs is sim_rollout_states' bit for bit; from the nominal start with alpha = 0 the nominal xs,
    us (a forward call's own) and cost come back bit for bit."""
    want = _want_tuple(want, ("xs", "x_final", "us", "cost"))
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimIlqrForward(struct_size=C.sizeof(capi.SimIlqrForward), r=float(r), u_limit=float(u_limit))
    B, T, host, _, _held = _plant_inputs(dims, state, u_nom, params, fext, f_base, f_mass, a, ticks=True, u_field="u_nom")
    if kff is not None:
        _require_cuda_tensor(kff, "kff", dtp, (T, B))
        a.kff = kff.data_ptr()
    if K is not None:
        _require_cuda_tensor(K, "K", dtp, (T, nx, B))
        a.K = K.data_ptr()
        if x0_nom is None:
            raise ValueError("x0_nom (the nominal start) is required where K is given")
        if xs_nom is None and T > 1:
            raise ValueError("xs_nom (the nominal trajectory) is required where K is given and T > 1")
    if x0_nom is not None:
        _require_cuda_tensor(x0_nom, "x0_nom", dtp, (nx, B))
        a.x0_nom = x0_nom.data_ptr()
    if xs_nom is not None:
        _require_cuda_tensor(xs_nom, "xs_nom", dtp, (T, nx, B))
        a.xs_nom = xs_nom.data_ptr()
    if alpha is not None:
        _require_cuda_tensor(alpha, "alpha", dtp, (B,))
        a.alpha = alpha.data_ptr()
    _cost_held = _ilqr_cost(a, nx, B, T, dtp, state.device, x_ref, u_ref, q, terminal)
    res = _alloc_outputs(a, want, {"xs": ("xs", (T, nx, B)), "x_final": ("x_final", (nx, B)), "us": ("us", (T, B)),
                                   "cost": ("cost", (B,))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_ilqr_forward_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a),
                                                            _stream_ptr()))
    return res


ILQR_ARMIJO = 1e-4   # a step is accepted where the cost falls by at least this share of the model's prediction


def sim_ilqr_search(params, dt, state, u_nom, xs_nom, cost_nom, kff, K, dV, x_ref, u_ref, q, r, terminal=None, trials=6,
                    armijo=ILQR_ARMIJO, u_limit=float("inf"), fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single",
                    want=("xs", "us", "cost", "alpha")):
    """The line search of one iLQR iteration in ONE launch (include/cpmpc.h: cpmpc_sim_ilqr_search_batch): every problem walks
    its own trial ladder on sim_ilqr_forward's roll, from the nominal trajectory state [nx, B] (the start, of the nominal too:
    there is no x0_nom), u_nom [T, B], xs_nom [T, nx, B] (always required) with cost cost_nom [B], under sim_ilqr_backward's
    kff [T, B], K [T, nx, B] (or None) and dV [2, B]:
        alpha = 1; up to `trials` (1..32) times: roll under u_t = clamp(u_nom[t] + alpha kff[t] + K[t] . wrap(x_t - x_nom_t)),
        accept where pred = dV[0] alpha + dV[1] alpha^2 < 0 and J_try - cost_nom <= armijo pred, else halve alpha.
    A problem leaves the ladder when it has decided, so the launch costs between one roll and `trials` rolls.  The decisions
    are those of the ladder of sim_ilqr_forward calls that sim_ilqr's default loop runs, bit for bit, and an accepted problem's
    xs, x_final, us and cost are sim_ilqr_forward's at its alpha, bit for bit.  A failed problem keeps its nominal BY COPY
    (alpha 0): what a forward call with alpha = 0 returns for finite data; where kff, K or dV of a problem is not finite while
    its nominal is, that call would poison it through 0 . NaN, and the search instead fails it and leaves its trajectory for a
    retry under a larger mu.  A problem whose nominal or cost_nom is itself non-finite returns that; no other problem is
    affected.  x_ref, u_ref, q, r, terminal: the cost, as sim_ilqr_backward's; params, dt and the forces as
    sim_rollout_states'.

    Returns a dict with the entries named in `want`,
        "xs" [T, nx, B],  "x_final" [nx, B],  "us" [T, B],  "cost" [B],  "alpha" [B] the step taken, 0: none."""
    want = _want_tuple(want, ("xs", "x_final", "us", "cost", "alpha"))
    m, nx, npar = dims = _model_dims(model)
    dtp = state.dtype
    a = capi.SimIlqrSearch(struct_size=C.sizeof(capi.SimIlqrSearch), r=float(r), u_limit=float(u_limit), trials=int(trials),
                           armijo=float(armijo))
    B, T, host, _, _held = _plant_inputs(dims, state, u_nom, params, fext, f_base, f_mass, a, ticks=True, u_field="u_nom")
    for name, t, shape in (("xs_nom", xs_nom, (T, nx, B)), ("cost_nom", cost_nom, (B,)), ("kff", kff, (T, B)), ("dV", dV, (2, B))):
        if t is None:
            raise ValueError("%s is required" % name)
        _require_cuda_tensor(t, name, dtp, shape)
        setattr(a, name, t.data_ptr())
    if K is not None:
        _require_cuda_tensor(K, "K", dtp, (T, nx, B))
        a.K = K.data_ptr()
    _cost_held = _ilqr_cost(a, nx, B, T, dtp, state.device, x_ref, u_ref, q, terminal)
    res = _alloc_outputs(a, want, {"xs": ("xs", (T, nx, B)), "x_final": ("x_final", (nx, B)), "us": ("us", (T, B)),
                                   "cost": ("cost", (B,)), "alpha": ("alpha", (B,))}, dtp, state.device)
    with torch.cuda.device(state.device):
        capi.check(capi.load().cpmpc_sim_ilqr_search_batch(m, _CAPI_DTYPE[dtp], B, host, float(dt), T, C.byref(a),
                                                           _stream_ptr()))
    return res


def sim_ilqr(params, dt, state, u_init, x_ref, q, r, terminal=None, u_ref=None, u_limit=float("inf"), iterations=10, trials=6,
             mu_init=0.0, fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), model="single", search="trials"):
    """Iterative LQR on the plant's own tick map, every problem in lock-step with its own line search and regularisation: fixed
    counts, elementwise torch between the launches, NO host synchronisation.  From state [nx, B] and the controls
    u_init [T, B] (clamped to +-u_limit by the first rollout), for the cost of sim_ilqr_backward:
        the first trajectory and its cost J: sim_ilqr_forward without kff and K;
        per iteration: ONE sim_ilqr_backward (with the problem's mu); then `trials` sim_ilqr_forward calls for the cost alone,
        alpha starting at 1: a problem ACCEPTS where dV[0] alpha + dV[1] alpha^2 < 0 and J_try - J <= 1e-4 of that prediction,
        and keeps its alpha from then on (it recomputes the same bits on the later trials); one that has not accepted halves
        alpha, and after the last trial gets alpha = 0; one more sim_ilqr_forward with the final alpha gives every problem's
        new trajectory -- a failed problem's is its old one bit for bit; mu: accepted -> mu / 10, and 0 once below 1e-6,
        failed -> max(10 mu, 1e-3).
    So J never increases on any problem.  A closing sim_ilqr_backward at the returned trajectory (with the returned mu) gives
    the gains that track it and its stationarity measure.
    search="trials" (the default) is that loop; search="fused" replaces the `trials` + 1 forward calls of an iteration and the
    torch between them by ONE sim_ilqr_search call (`trials` <= 32 there), in which a problem stops rolling once it has
    decided: the same decisions and the same entries bit for bit on finite data; where a problem's kff, K or dV is not finite
    the fused search fails it and keeps its trajectory (sim_ilqr_search).  The mu update is the same torch in both.

    Returns a dict: "u" [T, B], "xs" [T, nx, B], "K" [T, nx, B], "cost" [B], "cost_history" [iterations + 1, B] (row 0: of
    u_init), "hmax" [B], "mu" [B], "accepted" [iterations, B] bool."""
    iterations, trials = int(iterations), int(trials)
    if iterations < 0 or trials < 1:
        raise ValueError("iterations must be >= 0 and trials >= 1")
    if not float(mu_init) >= 0.0:
        raise ValueError("mu_init must be >= 0")
    if search not in ("trials", "fused"):
        raise ValueError("search must be 'trials' or 'fused'")
    if search == "fused" and trials > 32:
        raise ValueError("search='fused' takes trials <= 32")
    _, nx, _ = _model_dims(model)
    _require_cuda_tensor(state, "state", state.dtype)
    _require_cuda_tensor(u_init, "u_init", state.dtype)
    if state.dim() != 2 or u_init.dim() != 2:
        raise ValueError("state must be [%d, B] and u_init [T, B]" % nx)
    T, B = u_init.shape
    dtp, dev = state.dtype, state.device
    ref = _ilqr_reference(x_ref, T, nx, B, dtp, dev)
    cost_kw = dict(terminal=terminal, u_limit=u_limit, fext=fext, f_base=f_base, f_mass=f_mass, model=model)
    first = sim_ilqr_forward(params, dt, state, u_init, None, None, None, None, ref, u_ref, q, r, want=("xs", "us", "cost"),
                             **cost_kw)
    u, xs, J = first["us"], first["xs"], first["cost"]
    mu = torch.full((B,), float(mu_init), dtype=dtp, device=dev)
    history, accepted = [J], []
    for _ in range(iterations):
        bw = sim_ilqr_backward(params, dt, state, u, xs, ref, u_ref, q, r, mu=mu, want=("K", "kff", "dV"), **cost_kw)
        if search == "fused":
            fin = sim_ilqr_search(params, dt, state, u, xs, J, bw["kff"], bw["K"], bw["dV"], ref, u_ref, q, r, trials=trials,
                                  want=("xs", "us", "cost", "alpha"), **cost_kw)
            done = fin["alpha"] > 0
        else:
            dV1, dV2 = bw["dV"][0], bw["dV"][1]
            alpha = torch.ones((B,), dtype=dtp, device=dev)
            done = torch.zeros((B,), dtype=torch.bool, device=dev)
            for _ in range(trials):
                J_try = sim_ilqr_forward(params, dt, state, u, bw["kff"], bw["K"], state, xs, ref, u_ref, q, r, alpha=alpha,
                                         want="cost", **cost_kw)["cost"]
                pred = dV1 * alpha + dV2 * alpha * alpha
                done = done | ((pred < 0) & (J_try - J <= ILQR_ARMIJO * pred))
                alpha = torch.where(done, alpha, 0.5 * alpha)
            alpha = torch.where(done, alpha, torch.zeros_like(alpha))
            fin = sim_ilqr_forward(params, dt, state, u, bw["kff"], bw["K"], state, xs, ref, u_ref, q, r, alpha=alpha,
                                   want=("xs", "us", "cost"), **cost_kw)
        u, xs, J = fin["us"], fin["xs"], fin["cost"]
        down = mu / 10.0
        mu = torch.where(done, torch.where(down < 1e-6, torch.zeros_like(mu), down), torch.clamp(10.0 * mu, min=1e-3))
        history.append(J)
        accepted.append(done)
    last = sim_ilqr_backward(params, dt, state, u, xs, ref, u_ref, q, r, mu=mu, want=("K", "hmax"), **cost_kw)
    return {"u": u, "xs": xs, "K": last["K"], "cost": J, "cost_history": torch.stack(history), "hmax": last["hmax"], "mu": mu,
            "accepted": torch.stack(accepted) if accepted else torch.zeros((0, B), dtype=torch.bool, device=dev)}


def _full_covariance(cov, nx, batch, dtype, name):
    """cov [nx, B] (a diagonal) or [nx, nx, B] -> a fresh [nx, nx, B] tensor"""
    _require_cuda_tensor(cov, name, dtype)
    if tuple(cov.shape) == (nx, batch):
        return torch.diag_embed(cov.t()).permute(1, 2, 0).contiguous()
    if tuple(cov.shape) == (nx, nx, batch):
        return cov.detach().clone()
    raise ValueError("%s must be [%d, B] or [%d, %d, B]" % (name, nx, nx, nx))


class StateFilter:
    """A recursive state estimator for B plants: the extended Kalman filter, one sim_ekf launch of one tick per push() -- the
    recursive counterpart of WindowEstimator, at the cost of about one plant tick with its Jacobian.  Per tick the caller
    push()es the control it applied and what it then measured and gets the current state [nx, B] -- what
    ClosedLoop.set_state() takes; .state and .cov hold the current state and its covariance [nx, nx, B], .nis [B] the last
    tick's normalised squared innovations.  Nothing here waits for the device."""

    def __init__(self, params, dt, batch, cov0, weights, process_noise, state=None, dtype=torch.float64, device=None,
                 model="single", fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0)):
        """cov0: the covariance of the first state, [nx, B] (a diagonal) or [nx, nx, B].  weights: the measurements' inverse
        variances, process_noise: the variances added per tick (sim_ekf).  state [nx, B]: the first state (default: the
        plants hanging at rest, BatchSimulator's initial state).  params, dt and the forces are those of every tick."""
        self.model = model
        _, self.nx, self.np = _model_dims(model)
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.dtype, self.batch = dtype, int(batch)
        self.params, self.dt, self.weights, self.process_noise = params, float(dt), weights, process_noise
        self.forces = dict(fext=fext, f_base=f_base, f_mass=f_mass)
        if state is None:
            state = BatchSimulator(self.batch, dtype=dtype, device=self.device.index, model=model).get_state()
        _require_cuda_tensor(state, "state", dtype, (self.nx, self.batch))
        self.state = state.detach().clone()
        self.cov = _full_covariance(cov0, self.nx, self.batch, dtype, "cov0")
        self.nis = None

    def push(self, u, y, tick_weight=None):
        """One more tick: u [B] the control held over it, y [nx, B] the measurement after it (the rows of states whose
        weight is 0 are not read), tick_weight [B] or None (ones; 0: the sample is missing, the tick is a prediction).
        Returns the current state [nx, B], which .state holds too."""
        _require_cuda_tensor(u, "u", self.dtype, (self.batch,))
        _require_cuda_tensor(y, "y", self.dtype, (self.nx, self.batch))
        if tick_weight is not None:
            _require_cuda_tensor(tick_weight, "tick_weight", self.dtype, (self.batch,))
            tick_weight = tick_weight.reshape(1, self.batch)
        res = sim_ekf(self.params, self.dt, self.state, self.cov, u.reshape(1, self.batch), y.reshape(1, self.nx, self.batch),
                      self.weights, process_noise=self.process_noise, tick_weights=tick_weight, model=self.model,
                      want=("x_final", "P_final", "nis"), **self.forces)
        self.state, self.cov, self.nis = res["x_final"], res["P_final"], res["nis"]
        return self.state


def _invert_spd_lanes(P):
    """P [n, n, B], symmetric positive definite per lane (its lower triangle is read) -> P^-1 [n, n, B], symmetric: n unit
    right-hand sides through _cholesky_solve_lanes.  A lane whose P is not positive definite gets NaNs."""
    n = P.shape[0]
    Hs = [[P[j, i] for i in range(n)] for j in range(n)]
    zero, one = torch.zeros_like(P[0, 0]), torch.ones_like(P[0, 0])
    cols = []
    ok = None
    for c in range(n):
        x, pd = _cholesky_solve_lanes(Hs, [one if j == c else zero for j in range(n)])
        cols.append(torch.stack(x))
        ok = pd if ok is None else ok & pd
    inv = torch.stack(cols, dim=1)
    inv = 0.5 * (inv + inv.transpose(0, 1))
    return torch.where(ok, inv, torch.full_like(inv, float("nan"))).contiguous()


class WindowEstimator:
    """A moving-horizon state estimator for B plants: the last T controls and measurements on the device, and
    sim_estimate_state over them.  Per tick the caller push()es the control it applied and what it then measured, and
    estimate() returns the current state [nx, B] -- what ClosedLoop.set_state() takes.

    The fit's unknown is the state at the START of the window.  It is warm-started from the previous estimate, advanced by
    one plant tick (one sim_rollout_states launch) whenever a full window drops its oldest sample; before the window is
    full the estimator fits the ticks it has.

    The rolling prior (prior_cov given): the estimator keeps a prior mean and covariance of the window's first state -- at
    first the constructor's `state` and prior_cov -- and, whenever a full window drops its oldest tick, advances them over
    the dropped control, measurement and tick weight by one extended-Kalman-filter step (one sim_ekf launch of one tick):
    what the dropped samples said is kept as the arrival cost, which estimate() hands to sim_estimate_state as `prior` and
    prior_info = the covariance's inverse.  `weights` are then the measurements' inverse variances (sim_ekf).  Without
    prior_cov no arrival cost is carried from window to window and everything is as it was.  Either way estimate() passes
    a caller's own prior / prior_info through, and they take precedence.  Nothing here waits for the device."""

    def __init__(self, params, dt, batch, window, state=None, dtype=torch.float64, device=None, model="single", weights=None,
                 fext=None, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), prior_cov=None, process_noise=None):
        """window: T >= 1 ticks.  state [nx, B]: the first guess of the state before the first pushed tick (default: the
        plants hanging at rest, BatchSimulator's initial state).  params, dt, the forces and weights are those of every
        sim_estimate_state call.  prior_cov: None, or the covariance of `state`, [nx, B] (a diagonal) or [nx, nx, B]: the
        rolling prior; process_noise: the nx variances its step adds per tick (None: zeros)."""
        self.model = model
        _, self.nx, self.np = _model_dims(model)
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.dtype, self.batch, self.window = dtype, int(batch), int(window)
        if self.window < 1:
            raise ValueError("window must be >= 1")
        self.params, self.dt, self.weights = params, float(dt), weights
        self.forces = dict(fext=fext, f_base=f_base, f_mass=f_mass)
        if state is None:
            state = BatchSimulator(self.batch, dtype=dtype, device=self.device.index, model=model).get_state()
        _require_cuda_tensor(state, "state", dtype, (self.nx, self.batch))
        self.x0 = state.detach().clone()          # the guess of the state at the start of the window
        self.u = torch.zeros((self.window, self.batch), dtype=dtype, device=self.device)
        self.y = torch.zeros((self.window, self.nx, self.batch), dtype=dtype, device=self.device)
        self.w = torch.zeros((self.window, self.batch), dtype=dtype, device=self.device)
        self.count = 0                            # ticks held, at most `window` (a host counter: nothing is read back)
        self.process_noise = process_noise
        self.prior_mean = self.prior_cov = None   # the rolling prior of the window's first state
        if prior_cov is not None:
            self.prior_cov = _full_covariance(prior_cov, self.nx, self.batch, dtype, "prior_cov")
            self.prior_mean = state.detach().clone()

    def push(self, u, y, tick_weight=None):
        """One more tick: u [B] the control held over it, y [nx, B] the measurement after it (the rows of states that the
        weights leave out are not used but must be finite), tick_weight [B] or None (ones; 0: the sample is missing).  A
        full window drops its oldest tick, and the guess of its first state moves one tick on under the dropped control."""
        _require_cuda_tensor(u, "u", self.dtype, (self.batch,))
        _require_cuda_tensor(y, "y", self.dtype, (self.nx, self.batch))
        if tick_weight is not None:
            _require_cuda_tensor(tick_weight, "tick_weight", self.dtype, (self.batch,))
        if self.count == self.window:
            if self.prior_cov is not None:   # the dropped tick goes into the arrival cost
                res = sim_ekf(self.params, self.dt, self.prior_mean, self.prior_cov, self.u[:1], self.y[:1], self.weights,
                              process_noise=self.process_noise, tick_weights=self.w[:1], model=self.model, **self.forces)
                self.prior_mean, self.prior_cov = res["x_final"], res["P_final"]
            self.x0 = sim_rollout_states(self.params, self.dt, self.x0, self.u[:1], model=self.model, want="x_final",
                                         **self.forces)["x_final"]
            self.u, self.y, self.w = torch.roll(self.u, -1, 0), torch.roll(self.y, -1, 0), torch.roll(self.w, -1, 0)
            at = self.window - 1
        else:
            at = self.count
            self.count += 1
        self.u[at] = u
        self.y[at] = y
        if tick_weight is None:
            self.w[at] = 1.0
        else:
            self.w[at] = tick_weight

    def held(self):
        """The window as estimate() hands it to sim_estimate_state: (the guess [nx, B], u [n, B], y [n, nx, B], tick weights
        [n, B]) for the n = min(ticks pushed, window) ticks held -- views of the estimator's own tensors."""
        if self.count == 0:
            raise ValueError("WindowEstimator: no tick has been pushed yet")
        n = self.count
        return self.x0, self.u[:n], self.y[:n], self.w[:n]

    def smooth(self, want=("xs_smooth", "x0_smooth", "P0_smooth"), work=None):
        """sim_rts over the ticks held, from the rolling prior's mean and covariance: the smoothed states of the window in
        two launches (sim_rts's dict for `want`).  Needs prior_cov (ValueError without); changes nothing the estimator
        holds."""
        if self.prior_cov is None:
            raise ValueError("WindowEstimator.smooth needs the rolling prior: give prior_cov to the constructor")
        _, u, y, w = self.held()
        return sim_rts(self.params, self.dt, self.prior_mean, self.prior_cov, u, y, self.weights,
                       process_noise=self.process_noise, tick_weights=w, model=self.model, want=want, work=work, **self.forces)

    def estimate(self, iterations=2, damping=0.0, prior=None, prior_info=None, want_result=False):
        """sim_estimate_state over the ticks held, from the warm start, with the rolling prior as the arrival cost where
        the estimator keeps one; the estimate of the window's first state is the next call's guess.  Returns the current state [nx, B]; with want_result, (that, sim_estimate_state's dict)."""
        x0, u, y, w = self.held()
        if prior is None and prior_info is None and self.prior_cov is not None:
            prior, prior_info = self.prior_mean, _invert_spd_lanes(self.prior_cov)
        res = sim_estimate_state(self.params, self.dt, x0, u, y, iterations=iterations, damping=damping, weights=self.weights,
                                 tick_weights=w, prior=prior, prior_info=prior_info, model=self.model, **self.forces)
        self.x0 = res["x0"]
        return (res["x_final"], res) if want_result else res["x_final"]


class BatchSimulator:
    """B independent pendulum::Simulator plants (optimization/simulator.hpp:10-29)."""

    def __init__(self, batch, dtype=torch.float32, device=None, model="single"):
        self.model, self.nx, self.np = self._dims = _model_dims(model)
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", int(device))
        self.dtype = dtype
        hang = -3.14159265358979323846 / 2  # poles hanging, at rest (simulator.hpp:28)
        init = torch.tensor([0.0] + [hang] * (self.nx // 2 - 1) + [0.0] * (self.nx // 2), dtype=dtype)
        self.state = init.to(self.device).reshape(self.nx, 1).repeat(1, int(batch)).contiguous()

    def get_state(self):
        return self.state

    def set_state(self, state, stream=None):
        """The plants' state becomes a copy of state [nx, B].  stream None: the copy is queued on the current stream.  With a
        torch.cuda.Stream the copy (contiguous; `state` may then be a strided view, a column range) is queued on, and
        belongs to the pool of, that stream, and both `state` and the replaced tensor are recorded on it: the caller's
        allocator hands neither out while that stream may still read it.  Making that stream wait for whatever produced
        `state` is the caller's part (ClosedLoop.set_state)."""
        _require_cuda_tensor(state, "state", self.dtype, tuple(self.state.shape), contiguous=stream is None)
        if stream is None:
            self.state = state.clone()
            return
        old = self.state
        with torch.cuda.stream(stream):
            self.state = state.clone(memory_format=torch.contiguous_format)
        state.record_stream(stream)   # `state` is read there: its memory is not reused before that copy
        old.record_stream(stream)     # the plant of the last tick may still be reading the replaced tensor

    def step(self, params, dt, u, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), fext=None):
        """u: [B] tensor.  f_base/f_mass shared (x, y) pairs, or fext a [4, B] tensor
        {f_base.x, f_base.y, f_mass.x, f_mass.y}.  params: np floats (one plant for all), or an [np, B] tensor: a plant
        per problem (cpmpc_sim_step_dyn_batch)."""
        _plant_step(self._dims, dt, self.state, u, params, fext, f_base, f_mass, self.state)

    def step_differentiable(self, params, dt, u, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), fext=None):
        """step() with a backward: the state after the step is sim_step(params, dt, self.state, u, ...) -- bitwise what
        step() computes -- becomes self.state and is returned, attached to the autograd graph of the state before the step
        and of u -- and of params, where that is an [np, B] tensor requiring grad (sim_step).  The external forces and dt
        are not differentiated."""
        self.state = sim_step(params, dt, self.state, u, fext=fext, f_base=f_base, f_mass=f_mass, model=self.model)
        return self.state

    def rollout(self, params, dt, u, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), fext=None):
        """T step() calls in one launch (sim_rollout_states): u [T, B], u[t] held over tick t.  The state becomes the one
        after the last tick; returns xs [T, nx, B], the state after every tick."""
        res = sim_rollout_states(params.detach() if isinstance(params, torch.Tensor) else params, dt, self.state, u, fext=fext,
                                 f_base=f_base, f_mass=f_mass, model=self.model, want=("xs", "x_final"))
        self.state = res["x_final"]
        return res["xs"]

    def rollout_feedback(self, params, dt, u_nom, K, x0_nom, xs_nom, u_limit=float("inf"), f_base=(0.0, 0.0), f_mass=(0.0, 0.0),
                         fext=None):
        """T step() calls under u_nom[t] + K[t] . wrap(x_t - x_nom_t), clamped to +-u_limit, in one launch
        (sim_rollout_feedback): the state becomes the one after the last tick; returns (xs [T, nx, B], us [T, B]), the state
        after every tick and the controls applied."""
        res = sim_rollout_feedback(params.detach() if isinstance(params, torch.Tensor) else params, dt, self.state, u_nom, K,
                                   x0_nom, xs_nom, u_limit=u_limit, fext=fext, f_base=f_base, f_mass=f_mass, model=self.model,
                                   want=("xs", "x_final", "us"))
        self.state = res["x_final"]
        return res["xs"], res["us"]

    def ilqr(self, params, dt, u_init, x_ref, q, r, terminal=None, u_ref=None, u_limit=float("inf"), iterations=10, trials=6,
             mu_init=0.0, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), fext=None, search="trials"):
        """sim_ilqr from the simulator's own state, which is read and NOT advanced: a plan for the T ticks ahead (its dict)."""
        return sim_ilqr(params.detach() if isinstance(params, torch.Tensor) else params, dt, self.state, u_init, x_ref, q, r,
                        terminal=terminal, u_ref=u_ref, u_limit=u_limit, iterations=iterations, trials=trials, mu_init=mu_init,
                        fext=fext, f_base=f_base, f_mass=f_mass, model=self.model, search=search)

    def rollout_differentiable(self, params, dt, u, f_base=(0.0, 0.0), f_mass=(0.0, 0.0), fext=None):
        """rollout() with a backward: xs = sim_rollout(params, dt, self.state, u, ...) is returned, attached to the autograd
        graph of the state before the rollout, of u and -- where it is an [np, B] tensor requiring grad -- of params;
        self.state becomes a copy of xs[-1], attached likewise (a copy: step() works in place, and xs is what the backward
        reads).  The external forces and dt are not differentiated."""
        xs = sim_rollout(params, dt, self.state, u, fext=fext, f_base=f_base, f_mass=f_mass, model=self.model)
        self.state = xs[-1].clone()
        return xs


class ClosedLoop:
    """B controllers and their plants in closed loop on one GPU, all state resident on the device: per tick, for every
    controller, Optimization::Step on the plant's state (optimization.cc:39-97, warm-started after the first tick), the first
    control applied, Simulator::Step(control_dt) (simulator.cc:11-36) -- optimization_test.cc:39-61 for a batch.

    `ranges` > 1 holds the batch as that many independent column ranges, each with its own solver handle, plant and
    stream, ticked one after the other without any synchronisation between them.  Nothing couples two controllers, so the
    results are bitwise those of one range (a problem's arithmetic never depends on the lanes it occupies), and the ranges
    drift out of phase: while one range is in its fused SQP kernel -- one wave per SIMD in fp64, which leaves a fifth of the
    SIMD's issue slots idle -- another range's `prepare` / plant / `finalize` (no LDS, about 110 registers) runs beside it.
    Measured, 262 144 settled fp64 controllers (round 5): 0.843 ms per tick as one range, 0.80 as two; fp32 0.677 / 0.632
    (three).  A caller that needs every control of a tick before the next one starts synchronises the streams itself
    (`synchronize()`); the loop as such never does."""

    def __init__(self, params, batch, dtype=torch.float64, device=None, ranges=1, opts=None, model="single", pipeline="auto",
                 feedback=False):
        """feedback=True: tick() computes the first row K[0] of the feedback gains after every re-plan
        (BatchOptimization.feedback_gain) and applies u_0 + K[0] . wrap(x - x0) instead of u_0, on the plant's current
        state in each of tick(substeps=m)'s m plant steps of dt / m: an inner loop m times faster than the re-plan.
        feedback=False (default): the loop of the reference, unchanged."""
        self.feedback = bool(feedback)
        self.model = model
        self.u_limit = float(opts.u_limit) if opts is not None else float(capi.default_solver_opts().u_limit)
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", int(device))
        self.batch, self.dtype = int(batch), dtype
        ranges = max(1, min(int(ranges), self.batch))
        self.bounds = [self.batch * i // ranges for i in range(ranges + 1)]
        self.sims, self.opts, self.outs, self.streams = [], [], [], []
        for i in range(ranges):
            n = self.bounds[i + 1] - self.bounds[i]
            self.sims.append(BatchSimulator(n, dtype=dtype, device=device, model=model))
            o = BatchOptimization(params, max_batch=n, dtype=dtype, device=device, opts=opts, model=model)
            o.set_pipeline(pipeline)
            self.opts.append(o)
            self.outs.append(BatchOutputs())
            # one range: the caller's stream, like BatchOptimization alone; several: a stream each
            self.streams.append(torch.cuda.Stream(device=self.device) if ranges > 1 else None)
        self.applied = [None] * ranges  # feedback=True: per range, the control [n] applied in the last sub-step of the last tick
        self.ticks = 0
        self._inputs_dirty = len(self.sims) > 1   # the plants' initial states were written on the caller's stream

    def set_state(self, state):
        """state: [nx, B] tensor, columns in the caller's order.  May be called at any tick (a disturbance, a reset): with
        several ranges the copy is made ON each range's stream after that stream has waited for the caller's, so neither the
        range's solver / plant can read the new state before it has landed nor the caller's allocator hand the old one out
        while the range's plant is still reading it (BatchSimulator.set_state(stream=...)).  The whole tensor is
        checked before anything is touched -- a GPU tensor of the loop's dtype, exactly [nx, B] -- so a refused call leaves
        every range as it was."""
        _require_cuda_tensor(state, "state", self.dtype, (self.sims[0].nx, self.batch), contiguous=False)
        cur = torch.cuda.current_stream(self.device)
        for i, s in enumerate(self.sims):
            part = state[:, self.bounds[i]:self.bounds[i + 1]]
            st = self.streams[i]
            if st is None:
                s.set_state(part.contiguous())
                continue
            st.wait_stream(cur)                      # whatever produced `state` on the caller's stream comes first
            s.set_state(part, stream=st)
        self._inputs_dirty = len(self.sims) > 1

    def _on(self, i):
        st = self.streams[i]
        return torch.cuda.stream(st) if st is not None else torch.cuda.stream(torch.cuda.current_stream(self.device))

    def tick(self, dyn, set_point=0.0, dt=0.01, want_stats=True, substeps=1, fext=None, set_point_inner=None, plant_dyn=None):
        """One MPC tick of every controller (queued, not waited for).  With feedback=True the plant advances in `substeps`
        steps of dt / substeps, each under u_0 + K[0] . wrap(x - x0) of its current state; fext: optional callable
        (range index, sub-step) -> [4, n] tensor of external forces on that range's plants for that sub-step.
        set_point_inner (feedback=True; a float or a [B] tensor): the set-point as it stands during the sub-steps, where it
        has moved since the plan was made for `set_point`; the sub-steps then apply
        u_0 + K[0] . wrap(x - x0) + k_sp[0] (set_point_inner - set_point) (BatchOptimization.plan_sensitivity).
        plant_dyn: the PLANTS' parameters where they differ from what the controllers believe (`dyn`): np floats, or an
        [np, B] tensor, a plant per problem, split over the ranges as the states are (model mismatch, domain
        randomisation).  With plant_dyn given, dyn may be an [np, B] tensor too (per-problem controllers); without it dyn
        is the plants' parameter set as well and must be the np numbers."""
        if not self.feedback and (int(substeps) != 1 or fext is not None or set_point_inner is not None):
            raise ValueError("ClosedLoop.tick: substeps / fext / set_point_inner belong to the feedback loop "
                             "(ClosedLoop(..., feedback=True))")
        if int(substeps) < 1:
            raise ValueError("substeps must be >= 1")
        if isinstance(dyn, torch.Tensor) and plant_dyn is None:
            raise TypeError("ClosedLoop.tick: dyn is the plant's parameter set too (cpmpc_sim_step_batch takes shared host "
                            "parameters): pass the %d numbers, not a tensor" % self.sims[0].np)
        tensors = [t for t in (set_point, set_point_inner, plant_dyn, dyn) if isinstance(t, torch.Tensor)]
        if len(self.sims) > 1 and (self._inputs_dirty or tensors):
            # whatever prepared the states -- or this tick's per-problem parameters / set-points -- on the caller's stream
            # comes first.  Shared (host) parameters and no set_state since the last tick: no wait, the ranges run free.
            cur = torch.cuda.current_stream(self.device)
            for st in self.streams:
                st.wait_stream(cur)
                for t in tensors:
                    t.record_stream(st)
            self._inputs_dirty = False
        one = len(self.sims) == 1
        for i, (s, o, out) in enumerate(zip(self.sims, self.opts, self.outs)):
            lo, hi = self.bounds[i], self.bounds[i + 1]
            with self._on(i):
                # per-problem set-points [B]: this range's columns (copied on the range's stream)
                sp = set_point if one or not isinstance(set_point, torch.Tensor) else set_point[lo:hi].contiguous()
                dyn_i = dyn if one or not isinstance(dyn, torch.Tensor) else dyn[:, lo:hi].contiguous()
                pd = dyn_i if plant_dyn is None else plant_dyn
                if isinstance(pd, torch.Tensor) and not one and plant_dyn is not None:
                    pd = pd[:, lo:hi].contiguous()
                if self.feedback:
                    spi = set_point_inner
                    if isinstance(spi, torch.Tensor) and not one:
                        spi = spi[lo:hi].contiguous()
                    self._tick_feedback(i, s, o, out, dyn_i, sp, dt, want_stats, int(substeps), fext, spi, pd)
                    continue
                r = o.step(s.get_state(), dyn_i, sp, want_predicted=False, want_stats=want_stats, out=out)
                s.step(pd, dt, r.u[0].contiguous())
        self.ticks += 1

    def tick_hold(self, dyn, m, q, r, set_point=0.0, dt=0.01, want_stats=True, fext=None, plant_dyn=None, terminal=None):
        """One re-plan, then m plant ticks of dt that TRACK it (queued, not waited for): per range, on the range's stream,
            1. Optimization::Step on the plant's state x0, as tick() makes it;
            2. the nominal trajectory of the plan's first m controls from x0, sim_rollout_states with the CONTROLLER's
               parameters `dyn` and the plant's tick map (1 ms sub-steps over dt), without the external forces;
            3. sim_lqr along it with the state weights q (nx numbers), the control weight r and `terminal` (sim_lqr's: an
               [nx, nx, B] tensor, nx numbers, or None: diag(q));
            4. BatchSimulator.rollout_feedback on the plants (plant_dyn, else dyn) under u_k + K[k] . wrap(x - x_nom_k),
               clamped to the handle's u_limit -- one launch for the m ticks;
            5. the warm start's controls shifted by m - 1 more places, the last one duplicated: the next step's own shift by
               one then starts from u_m, and its u_prev is u_{m-1}, the last nominal control applied.
        ticks advances by m.  m = 1 leaves the plants and the warm start bitwise as tick() does (the deviation from the
        nominal start is exactly 0).  1 <= m <= window_length.  The gains belong to the plant's map at dt, not to the
        controller's RK4 at control_dt; there is no feedback inside a tick, and the Riccati recursion does not know of the
        clamp.  fext: optional callable (range index) -> [4, n] tensor of external forces on that range's plants, the same
        for the m ticks; the nominal trajectory does not see them.  dyn, plant_dyn, set_point as tick()'s.  Not for
        feedback=True loops: their gain is the QP's du_0/dx0 applied at sub-step rate, another law for the same ticks."""
        if self.feedback:
            raise ValueError("ClosedLoop.tick_hold: the loop was made with feedback=True, whose tick() applies the QP's own "
                             "gain; make the loop with feedback=False to track with the Riccati gains")
        m = int(m)
        if not 1 <= m <= self.opts[0].N:
            raise ValueError("m must be in [1, window_length = %d]" % self.opts[0].N)
        if isinstance(dyn, torch.Tensor) and plant_dyn is None:
            raise TypeError("ClosedLoop.tick_hold: dyn is the plant's parameter set too: pass the %d numbers, not a tensor, or "
                            "give plant_dyn" % self.sims[0].np)
        tensors = [t for t in (set_point, plant_dyn, dyn, terminal) if isinstance(t, torch.Tensor)]
        if len(self.sims) > 1 and (self._inputs_dirty or tensors):
            cur = torch.cuda.current_stream(self.device)   # as tick(): what prepared the inputs on the caller's stream comes first
            for st in self.streams:
                st.wait_stream(cur)
                for t in tensors:
                    t.record_stream(st)
            self._inputs_dirty = False
        one = len(self.sims) == 1

        def cols(t, lo, hi):   # this range's columns of a per-problem tensor [..., B]
            return t if one or not isinstance(t, torch.Tensor) else t[..., lo:hi].contiguous()
        for i, (s, o, out) in enumerate(zip(self.sims, self.opts, self.outs)):
            lo, hi = self.bounds[i], self.bounds[i + 1]
            with self._on(i):
                dyn_i = cols(dyn, lo, hi)
                pd = dyn_i if plant_dyn is None else cols(plant_dyn, lo, hi)
                x0 = s.get_state()   # rollout_feedback gives the plant a new tensor: this one stays the plan's x0
                res = o.step(x0, dyn_i, cols(set_point, lo, hi), want_predicted=False, want_stats=want_stats, out=out)
                u_nom = res.u[:m]
                xs_nom = sim_rollout_states(dyn_i, dt, x0, u_nom, model=self.model)["xs"]
                K = sim_lqr(dyn_i, dt, x0, u_nom, xs_nom, q, r, terminal=cols(terminal, lo, hi), model=self.model, want="K")["K"]
                s.rollout_feedback(pd, dt, u_nom, K, x0, xs_nom, u_limit=self.u_limit, fext=None if fext is None else fext(i))
                if m > 1:
                    n = hi - lo
                    z = o.get_solution(n)
                    zu = z[o.dim - o.N:]
                    z[o.dim - o.N:] = torch.cat([zu[m - 1:], zu[-1:].expand(m - 1, n)])
                    o.set_previous_solution(z)
        self.ticks += m

    def _tick_feedback(self, i, s, o, out, dyn, sp, dt, want_stats, substeps, fext, sp_inner=None, plant_dyn=None):
        plant_dyn = dyn if plant_dyn is None else plant_dyn   # the plants' parameters (tick: plant_dyn)
        x0 = s.get_state().clone()  # the state the plan is made for: the plant's own tensor moves under the sub-steps
        r = o.step(x0, dyn, sp, want_predicted=False, want_stats=want_stats, out=out)
        if sp_inner is not None:
            self._substeps_with_set_point(i, s, o, r, x0, dyn, sp, sp_inner, dt, substeps, fext, plant_dyn)
            return
        K, ok = o.feedback_gain(dyn, n_rows=1, want_ok=True)
        # a controller whose QP is not positive definite has no gain (NaN rows): it holds the plan's u_0, as the plain loop does
        K0 = torch.where(ok.bool().unsqueeze(0), K[0], torch.zeros_like(K[0]))
        u_nom = r.u[0].contiguous()
        for m in range(substeps):
            u = feedback_apply(u_nom, K0, x0, s.get_state(), u_limit=self.u_limit, model=self.model)
            s.step(plant_dyn, dt / substeps, u, fext=None if fext is None else fext(i, m))
        self.applied[i] = u  # the control of the last sub-step

    def _substeps_with_set_point(self, i, s, o, r, x0, dyn, sp, sp_inner, dt, substeps, fext, plant_dyn=None):
        """The sub-steps of a tick whose set-point has moved since the plan: K[0] and k_sp[0] from one call, applied by
        plan_update on row 0.  A lane with ok = 0 holds the plan's u_0."""
        n = int(x0.shape[1])
        plant_dyn = dyn if plant_dyn is None else plant_dyn

        def per_problem(v):
            return v if isinstance(v, torch.Tensor) else torch.full((n,), float(v), dtype=self.dtype, device=x0.device)
        sens = o.plan_sensitivity(dyn, n_rows=1, want=("K", "k_sp"), want_ok=True)
        live = sens["ok"].bool()
        K = torch.where(live.reshape(1, 1, n), sens["K"], torch.zeros_like(sens["K"]))
        k_sp = torch.where(live.reshape(1, n), sens["k_sp"], torch.zeros_like(sens["k_sp"]))
        u_nom = r.u[:1].contiguous()
        sp_nom, sp_now = per_problem(sp), per_problem(sp_inner)
        for m in range(substeps):
            u = plan_update(u_nom, K=K, x_nom=x0, x=s.get_state(), k_sp=k_sp, sp_nom=sp_nom, sp=sp_now,
                            u_limit=self.u_limit, model=self.model)[0]
            s.step(plant_dyn, dt / substeps, u, fext=None if fext is None else fext(i, m))
        self.applied[i] = u  # the control of the last sub-step

    def synchronize(self):
        """Make the caller's stream wait for everything queued on the ranges' streams."""
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            if st is not None:
                cur.wait_stream(st)

    def state(self):
        self.synchronize()
        return torch.cat([s.get_state() for s in self.sims], dim=1)

    def controls(self):
        """u [N, B] of the last tick."""
        self.synchronize()
        return torch.cat([o.u for o in self.outs], dim=1)

    def iterations(self):
        self.synchronize()
        return torch.cat([o.iterations for o in self.outs])

    def status(self):
        self.synchronize()
        return torch.cat([o.status for o in self.outs])

    def stage_plan(self):
        return self.opts[0].stage_plan()

    def close(self):
        for o in self.opts:
            o.close()
