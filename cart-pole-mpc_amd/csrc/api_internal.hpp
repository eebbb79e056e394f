// api_internal.hpp -- what the three C-ABI translation units share (host code only): cpmpc_api.hip (the handle, the
// device-pointer calls, the stand-alone pieces), cpmpc_host.hip (the host-pointer pipeline) and cpmpc_sharded.hip (several
// GPUs from one process).  The functions are hidden: the library exports the C-ABI of include/cpmpc.h, not these.
#pragma once
#include <vector>

#include "engine.hpp"

// the current device is `dev` for the guard's lifetime (a type, not marked: its inline members keep the visibility they
// have always had)
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
      if (hipSetDevice(dev) == hipSuccess) switched = true;
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};
// (cpmpc_api.hip)
CPMPC_HIDDEN bool device_is_gfx950(int dev);
// CPMPC_OK, or CPMPC_ERR_NO_DEVICE (with the error text) when the current device is not a usable gfx950
CPMPC_HIDDEN int current_device_ok();
// the argument checks of cpmpc_feedback_gain_batch[_host] (no device needed)
CPMPC_HIDDEN int check_gain_args(const cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, const void* K);
// the argument checks of cpmpc_plan_weight_vjp_batch[_host] (no device needed unless the handle is null)
CPMPC_HIDDEN int check_weight_vjp_args(const cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows,
                                       const void* gbar, const void* g_tw, const void* g_wu, const void* g_wdu,
                                       const void* du);

// (cpmpc_host.hip) Grows the device buffer *dev -- and its pinned host mirror *pin when `pin` is given -- to at least
// `bytes` (*cap: their size); never shrinks, allocates at least 4 096 bytes.  `stream` is synchronised before the old
// buffers are freed (work queued there may still use them).  CPMPC_ERR_ALLOC when an allocation fails.
CPMPC_HIDDEN int grow_staging(void** dev, void** pin, size_t* cap, size_t bytes, hipStream_t stream);

// (cpmpc_host.hip) One chunk of a host-pointer step: problems [c0, c0 + Bc) of handle h = columns [g0, g0 + Bc) of the
// caller's arrays
struct HostWork {
  cpmpc_solver* h;
  int64_t c0, Bc, g0;
};
CPMPC_HIDDEN int check_host_inputs(const cpmpc_step_host_inputs* in, const cpmpc_step_host_outputs* out);
// whether the real-typed outputs go by DMA straight into the caller's arrays (decided once per call)
CPMPC_HIDDEN bool host_direct_outputs(const cpmpc_solver* s, const cpmpc_step_host_outputs& out);
// the chunks of problems [0, Bh) of handle h (its columns start at g_base in the caller's arrays), appended to per_handle
CPMPC_HIDDEN void host_chunks_of(cpmpc_solver* h, int64_t Bh, int64_t g_base, bool direct,
                                 std::vector<std::vector<HostWork>>& per_handle);
// runs the chunks of every handle as one pipeline; returns after every chunk has landed
CPMPC_HIDDEN int run_host_pipeline(const std::vector<std::vector<HostWork>>& per_handle, int64_t ld,
                                   const cpmpc_step_host_inputs& in, const cpmpc_step_host_outputs& out, bool direct);
// the warm start of problems [0, n) of s <-> columns [g0, g0 + n) of the caller's double array [dim][ld]; synchronous
CPMPC_HIDDEN int set_prev_host_cols(cpmpc_solver* s, int64_t n, const double* z_host, int64_t ld, int64_t g0);
CPMPC_HIDDEN int get_sol_host_cols(cpmpc_solver* s, int64_t n, double* z_host, int64_t ld, int64_t g0);
