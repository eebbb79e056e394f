// cpmpc_sharded.hip -- several GPUs from one process (the cpmpc_sharded_* calls of include/cpmpc.h): one handle + stream
// per shard, a contiguous split of the batch, concurrent shards.  The device-pointer calls fan out through
// sharded_fan_out and move column blocks with copy_cols; the host-pointer calls run the host pipeline of cpmpc_host.hip
// over the shards' handles.  No device code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "api_internal.hpp"

struct Shard {
  cpmpc_solver* h = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;   // device-pointer steps of this shard run here
  hipEvent_t done = nullptr;      // shard stream -> root stream (results have landed on the root device)
  void* buf = nullptr;            // per-shard device staging of the device-pointer step and of the warm-start hand-over
  size_t buf_bytes = 0;
  int peer = 1;                   // what cpmpc_sharded_create saw: 1 root <-> this device mapped both ways (or the same device), 0 not
};

struct cpmpc_sharded {
  std::vector<Shard> shards;
  int dtype = CPMPC_F64;
  int N = 0, NX = 4, NP = 9, dim = 0;
  size_t esize = 8;
  int64_t cap = 0;
  hipEvent_t ready = nullptr;  // on the ROOT device: the caller's inputs are there (root stream -> every shard stream)
  // Warm-start bookkeeping.  The split of a batch depends on its size, so the shards' previous solutions are those of
  // columns [0, warm_total) split as a batch of dist_B problems is split; a step (or set / get) with another size first
  // hands the warm start over to the new split (sharded_align).
  int64_t dist_B = 0;
  int64_t warm_total = 0;
};

static void shard_range(int64_t total, int i, int n, int64_t* lo, int64_t* hi) {
  const int64_t base = total / n, rem = total % n;
  *lo = (int64_t)i * base + (i < rem ? i : rem);
  *hi = *lo + base + (i < rem ? 1 : 0);
}

extern "C" void cpmpc_sharded_destroy(cpmpc_sharded* s) {
  if (!s) return;
  for (auto& sh : s->shards) {
    DeviceGuard guard(sh.device);
    if (sh.stream) (void)hipStreamSynchronize(sh.stream);
    if (sh.h) cpmpc_destroy(sh.h);
    if (sh.buf) (void)hipFree(sh.buf);
    if (sh.done) (void)hipEventDestroy(sh.done);
    if (sh.stream) (void)hipStreamDestroy(sh.stream);
  }
  if (s->ready && !s->shards.empty()) {
    DeviceGuard guard(s->shards[0].device);
    (void)hipEventDestroy(s->ready);
  }
  delete s;
}

extern "C" int cpmpc_sharded_create_ex(const cpmpc_create_info* info, const int* devices, int n_devices,
                                       cpmpc_sharded** out) {
  if (!info || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (info->struct_size != sizeof(cpmpc_create_info))
    return fail(CPMPC_ERR_INVALID_ARG, "cpmpc_create_info.struct_size is %u, this library's is %zu", info->struct_size,
                sizeof(cpmpc_create_info));
  std::vector<int> devs;
  if (devices == nullptr) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
      return fail(CPMPC_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    for (int i = 0; i < n; ++i)
      if (device_is_gfx950(i)) devs.push_back(i);
    if (devs.empty()) return fail(CPMPC_ERR_NO_DEVICE, "no gfx950 device visible");
  } else {
    if (n_devices < 1 || n_devices > 64) return fail(CPMPC_ERR_INVALID_ARG, "n_devices must be in [1, 64]");
    devs.assign(devices, devices + n_devices);
  }
  const int n = (int)devs.size();
  if (info->max_batch < n) return fail(CPMPC_ERR_INVALID_ARG, "max_batch must be at least the number of shards");
  cpmpc_sharded* s = new (std::nothrow) cpmpc_sharded();
  if (!s) return fail(CPMPC_ERR_ALLOC, "out of host memory");
  s->dtype = info->dtype;
  s->esize = info->dtype == CPMPC_F32 ? 4 : 8;
  s->cap = info->max_batch;
  s->shards.resize(n);
  for (int i = 0; i < n; ++i) {
    Shard& sh = s->shards[i];
    sh.device = devs[i];
    int64_t lo, hi;
    shard_range(info->max_batch, i, n, &lo, &hi);
    cpmpc_create_info one = *info;
    one.device = sh.device;
    one.max_batch = hi - lo + 1;  // +1: a smaller B may shift a remainder here
    int rc = cpmpc_create_ex(&one, &sh.h);
    if (rc == CPMPC_OK) {
      DeviceGuard guard(sh.device);
      if (hipStreamCreateWithFlags(&sh.stream, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&sh.done, hipEventDisableTiming) != hipSuccess)
        rc = fail(CPMPC_ERR_HIP, "stream / event creation failed on device %d", sh.device);
    }
    if (rc != CPMPC_OK) {
      cpmpc_sharded_destroy(s);
      return rc;
    }
  }
  s->N = s->shards[0].h->N;
  s->NX = s->shards[0].h->NX;
  s->NP = s->shards[0].h->NP;
  s->dim = s->shards[0].h->dim;
  const int root = s->shards[0].device;
  {  // an event may only be recorded on a stream of the device it was created on: `ready` belongs to the ROOT device
    DeviceGuard guard(root);
    if (hipEventCreateWithFlags(&s->ready, hipEventDisableTiming) != hipSuccess) {
      cpmpc_sharded_destroy(s);
      return fail(CPMPC_ERR_HIP, "event creation failed on device %d", root);
    }
  }
  // peer access between the root device and every other shard's device (both directions); a pair that cannot be
  // mapped still works, the copies then go through host memory
  for (int i = 1; i < n; ++i) {
    const int d = s->shards[i].device;
    if (d == root) continue;
    int can = 0, both = 0;
    if (hipDeviceCanAccessPeer(&can, root, d) == hipSuccess && can) {
      DeviceGuard guard(root);
      const hipError_t pe = hipDeviceEnablePeerAccess(d, 0);
      both += (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled);
    }
    if (hipDeviceCanAccessPeer(&can, d, root) == hipSuccess && can) {
      DeviceGuard guard(d);
      const hipError_t pe = hipDeviceEnablePeerAccess(root, 0);
      both += (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled);
    }
    s->shards[i].peer = both == 2;
    (void)hipGetLastError();  // "already enabled" is fine
  }
  *out = s;
  return CPMPC_OK;
}

extern "C" int cpmpc_sharded_create(const cpmpc_params* params, const cpmpc_solver_opts* opts, int dtype,
                                    int64_t max_batch, const int* devices, int n_devices, cpmpc_sharded** out) {
  if (!params || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  cpmpc_create_info info;
  memset(&info, 0, sizeof info);
  info.struct_size = sizeof info;
  info.dtype = dtype;
  info.model = CPMPC_MODEL_SINGLE;
  info.max_batch = max_batch;
  info.params = params;
  info.opts = opts;
  info.opts_size = opts ? CPMPC_SOLVER_OPTS_SIZE_POSITIONAL : 0;  // a positional constructor: the struct as it was frozen
  return cpmpc_sharded_create_ex(&info, devices, n_devices, out);
}

extern "C" int cpmpc_sharded_num_shards(const cpmpc_sharded* s) { return s ? (int)s->shards.size() : -1; }
extern "C" int cpmpc_sharded_peer_access(const cpmpc_sharded* s, int shard) {
  return (s && shard >= 0 && shard < (int)s->shards.size()) ? s->shards[shard].peer : -1;
}
extern "C" int cpmpc_sharded_device(const cpmpc_sharded* s, int shard) {
  return (s && shard >= 0 && shard < (int)s->shards.size()) ? s->shards[shard].device : -1;
}
extern "C" cpmpc_solver* cpmpc_sharded_handle(cpmpc_sharded* s, int shard) {
  return (s && shard >= 0 && shard < (int)s->shards.size()) ? s->shards[shard].h : nullptr;
}
extern "C" int cpmpc_sharded_range(const cpmpc_sharded* s, int shard, int64_t B, int64_t* lo, int64_t* hi) {
  if (!s || !lo || !hi || shard < 0 || shard >= (int)s->shards.size() || B < 0)
    return fail(CPMPC_ERR_INVALID_ARG, "bad argument");
  shard_range(B, shard, (int)s->shards.size(), lo, hi);
  return CPMPC_OK;
}
extern "C" int cpmpc_sharded_reset(cpmpc_sharded* s) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null solver");
  for (auto& sh : s->shards) cpmpc_reset(sh.h);
  s->dist_B = 0;
  s->warm_total = 0;
  return CPMPC_OK;
}
extern "C" int64_t cpmpc_sharded_previous_solution_batch(const cpmpc_sharded* s) { return s ? s->warm_total : 0; }
// every shard was created from the same parameters: the status of shard 0 is the handle's
extern "C" int cpmpc_sharded_horizon_beyond_parity(const cpmpc_sharded* s) {
  return (s && !s->shards.empty()) ? cpmpc_horizon_beyond_parity(s->shards[0].h) : -1;
}

static int sharded_check(const cpmpc_sharded* s, int64_t B) {
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  if (B > s->cap) return fail(CPMPC_ERR_BATCH, "B=%lld exceeds the capacity %lld given to cpmpc_sharded_create", (long long)B, (long long)s->cap);
  return CPMPC_OK;
}

// the shard's device staging (the device-pointer step, the warm-start hand-over), grown to at least `bytes`
static int ensure_shard_buf(Shard& sh, size_t bytes) {
  return grow_staging(&sh.buf, nullptr, &sh.buf_bytes, bytes, sh.stream);
}

// Columns [src_lo, src_lo + n) of the [rows][src_ld] array src -> columns [dst_lo, dst_lo + n) of the [rows][dst_ld]
// array dst (scalars of `es` bytes), queued on `stream`; nothing when either array is absent (NULL).  hipMemcpyDefault:
// either side may be on any device, with or without peer access.
static hipError_t copy_cols(void* dst, int64_t dst_ld, int64_t dst_lo, const void* src, int64_t src_ld, int64_t src_lo,
                            int64_t n, size_t rows, size_t es, hipStream_t stream) {
  if (!dst || !src) return hipSuccess;
  return hipMemcpy2DAsync((char*)dst + (size_t)dst_lo * es, (size_t)dst_ld * es, (const char*)src + (size_t)src_lo * es,
                          (size_t)src_ld * es, (size_t)n * es, rows, hipMemcpyDefault, stream);
}

// Shard i's columns [lo, lo + n_i) of a batch of B problems: returns n_i
static int64_t batch_cols(int64_t B, int i, int n, int64_t* lo) {
  int64_t hi;
  shard_range(B, i, n, lo, &hi);
  return hi - *lo;
}

// How many of shard i's problems, split as a batch of `dist` problems is split, lie in columns [0, warm)
static int64_t warm_in_shard(int64_t dist, int i, int n, int64_t warm, int64_t* lo_out) {
  int64_t lo, hi;
  shard_range(dist, i, n, &lo, &hi);
  if (lo_out) *lo_out = lo;
  const int64_t w = warm - lo;
  return w < 0 ? 0 : (w > hi - lo ? hi - lo : w);
}

// The shards hold the previous solutions of columns [0, warm_total) split as a batch of dist_B problems is split.  A call
// with another batch size B would pair every shard's warm start with other columns: hand the warm start over to B's
// split first -- gather z of the warm columns on the root device, reset, scatter by the new ranges.  Columns beyond B
// are dropped (a single handle would keep them; a sharded one has nowhere to put them).  Rare and synchronous.
static int sharded_align(cpmpc_sharded* s, int64_t B) {
  if (s->warm_total == 0 || s->dist_B == B) {
    if (s->warm_total == 0) s->dist_B = B;
    return CPMPC_OK;
  }
  const int n = (int)s->shards.size();
  const int64_t W = s->warm_total;
  const size_t es = s->esize, dim = (size_t)s->dim;
  const int root = s->shards[0].device;
  void* tmp = nullptr;
  {
    DeviceGuard guard(root);
    HIP_TRY(hipMalloc(&tmp, dim * (size_t)W * es));
  }
  int rc = CPMPC_OK;
  auto body = [&]() -> int {
    for (int i = 0; i < n; ++i) {  // gather [dim][n_i] of every shard into columns [lo_i, lo_i + n_i) of tmp [dim][W]
      int64_t lo;
      const int64_t ni = warm_in_shard(s->dist_B, i, n, W, &lo);
      if (ni == 0) continue;
      Shard& sh = s->shards[i];
      DeviceGuard guard(sh.device);
      int r = ensure_shard_buf(sh, dim * (size_t)ni * es);
      if (r) return r;
      r = cpmpc_get_solution(sh.h, ni, sh.buf, sh.stream);
      if (r) return r;
      HIP_TRY(copy_cols(tmp, W, lo, sh.buf, ni, 0, ni, dim, es, sh.stream));
      HIP_TRY(hipStreamSynchronize(sh.stream));
    }
    for (auto& sh : s->shards) cpmpc_reset(sh.h);
    const int64_t keep = W < B ? W : B;
    for (int i = 0; i < n; ++i) {
      int64_t lo;
      const int64_t ni = warm_in_shard(B, i, n, keep, &lo);
      if (ni == 0) continue;
      Shard& sh = s->shards[i];
      DeviceGuard guard(sh.device);
      int r = ensure_shard_buf(sh, dim * (size_t)ni * es);
      if (r) return r;
      HIP_TRY(copy_cols(sh.buf, ni, 0, tmp, W, lo, ni, dim, es, sh.stream));
      r = cpmpc_set_previous_solution(sh.h, ni, sh.buf, sh.stream);
      if (r) return r;
      HIP_TRY(hipStreamSynchronize(sh.stream));
    }
    s->dist_B = B;
    s->warm_total = keep;
    return CPMPC_OK;
  };
  rc = body();
  {
    DeviceGuard guard(root);
    for (auto& sh : s->shards) (void)hipStreamSynchronize(sh.stream);
    (void)hipFree(tmp);
  }
  if (rc != CPMPC_OK) {  // half-moved warm starts are worse than none
    for (auto& sh : s->shards) cpmpc_reset(sh.h);
    s->dist_B = B;
    s->warm_total = 0;
  }
  return rc;
}

// The fan-out of the device-pointer calls.  For every shard to which cols(i, &lo) gives columns [lo, lo + n_i) of this
// call, on the shard's device: grow its staging to bytes(n_i), make its stream wait until the root stream has passed this
// call, and queue work(shard, lo, n_i) there.  Then the root stream waits for every shard used.  On failure the shard
// streams given work are drained (their copies may still be writing the caller's arrays) and the first error returned.
template <class Cols, class Bytes, class Work>
static int sharded_fan_out(cpmpc_sharded* s, hipStream_t root_stream, Cols cols, Bytes bytes, Work work) {
  const int root = s->shards[0].device;
  {  // ONE event of the root device, every shard stream waits on it (an event is recorded on a stream of its own device)
    DeviceGuard guard(root);
    HIP_TRY(hipEventRecord(s->ready, root_stream));
  }
  std::vector<int> used;
  auto one = [&](int i) -> int {
    int64_t lo;
    const int64_t ni = cols(i, &lo);
    if (ni == 0) return CPMPC_OK;
    Shard& sh = s->shards[i];
    DeviceGuard guard(sh.device);
    const int r = ensure_shard_buf(sh, bytes(ni));
    if (r) return r;
    used.push_back(i);  // from here on work of this call is (or may be) in flight on sh.stream
    HIP_TRY(hipStreamWaitEvent(sh.stream, s->ready, 0));
    if (const int rw = work(sh, lo, ni)) return rw;
    HIP_TRY(hipEventRecord(sh.done, sh.stream));
    return CPMPC_OK;
  };
  int rc = CPMPC_OK;
  for (int i = 0; i < (int)s->shards.size() && rc == CPMPC_OK; ++i) rc = one(i);
  if (rc != CPMPC_OK) {
    for (int i : used) {
      DeviceGuard guard(s->shards[i].device);
      (void)hipStreamSynchronize(s->shards[i].stream);
    }
    return rc;
  }
  DeviceGuard guard(root);
  for (int i : used) HIP_TRY(hipStreamWaitEvent(root_stream, s->shards[i].done, 0));
  return CPMPC_OK;
}

extern "C" int cpmpc_sharded_step_batch_host_in(cpmpc_sharded* s, int64_t B, const cpmpc_step_host_inputs* in,
                                                const cpmpc_step_host_outputs* out) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = check_host_inputs(in, out);
  if (rc) return rc;
  rc = sharded_check(s, B);
  if (rc) return rc;
  rc = sharded_align(s, B);
  if (rc) return rc;
  const int n = (int)s->shards.size();
  // every shard's chunks -- upload, kernels, download on its own streams -- are in flight together
  std::vector<std::vector<HostWork>> work;
  bool direct;
  {
    DeviceGuard guard(s->shards[0].device);
    direct = host_direct_outputs(s->shards[0].h, *out);
  }
  for (int i = 0; i < n; ++i) {
    int64_t lo, hi;
    shard_range(B, i, n, &lo, &hi);
    if (hi > lo) host_chunks_of(s->shards[i].h, hi - lo, lo, direct, work);
  }
  rc = run_host_pipeline(work, B, *in, *out, direct);
  if (rc == CPMPC_OK) s->warm_total = B;
  else cpmpc_sharded_reset(s);  // some shards stepped, others did not: no consistent warm start is left
  return rc;
}

extern "C" int cpmpc_sharded_step_batch_host(cpmpc_sharded* s, int64_t B, const double* x0_host,
                                             const double* dyn_shared_host, double set_point,
                                             const cpmpc_step_host_outputs* out) {
  if (!s || !x0_host || !dyn_shared_host || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (!std::isfinite(set_point)) return fail(CPMPC_ERR_INVALID_ARG, "set_point must be finite");
  const cpmpc_step_host_inputs in = {x0_host, dyn_shared_host, nullptr, set_point, nullptr, nullptr};
  return cpmpc_sharded_step_batch_host_in(s, B, &in, out);
}

extern "C" int cpmpc_sharded_step_batch_ex(cpmpc_sharded* s, int64_t B, const cpmpc_step_inputs* in,
                                           const cpmpc_step_outputs* out, void* stream) {
  if (!s || !in || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (!in->x0) return fail(CPMPC_ERR_INVALID_ARG, "x0 is required");
  if ((in->dyn_shared_host == nullptr) == (in->dyn == nullptr))
    return fail(CPMPC_ERR_INVALID_ARG, "exactly one of dyn_shared_host / dyn must be given");
  if (!in->set_point && !std::isfinite(in->set_point_shared))
    return fail(CPMPC_ERR_INVALID_ARG, "set_point_shared must be finite");
  int rc = sharded_check(s, B);
  if (rc) return rc;
  rc = sharded_align(s, B);
  if (rc) return rc;
  const int n = (int)s->shards.size();
  const size_t es = s->esize;
  const size_t NX = (size_t)s->NX, N = (size_t)s->N, NP = (size_t)s->NP, dim = (size_t)s->dim;
  // The caller's arrays, [rows][B] each on the root device: the inputs, then the outputs.  A shard stages its columns of
  // every present one on its own device, in 256-byte aligned pieces in this order (absent arrays take no room).
  enum { kX0, kDyn, kSetPoint, kTermW, kU, kPred, kCost, kEqL1, kStatus, kIters, kLsEvals, kGuess, kSol, kArrays };
  const struct {
    const void* a;
    size_t rows, es;
  } arr[kArrays] = {{in->x0, NX, es}, {in->dyn, NP, es}, {in->set_point, 1, es}, {in->terminal_weights, NX, es},
                    {out->u, N, es}, {out->predicted, N * NX, es}, {out->final_cost, 1, es}, {out->final_eq_l1, 1, es},
                    {out->status, 1, 4}, {out->iterations, 1, 4}, {out->ls_evals, 1, 4}, {out->guess, dim, es},
                    {out->solution, dim, es}};
  // where the pieces of a shard's ni columns start; off[kArrays]: the bytes of its staging
  auto layout = [&](int64_t ni, size_t* off) {
    off[0] = 0;
    for (int k = 0; k < kArrays; ++k)
      off[k + 1] = off[k] + (arr[k].a ? (arr[k].rows * (size_t)ni * arr[k].es + 255) & ~(size_t)255 : 0);
    return off[kArrays];
  };
  auto step_shard = [&](Shard& sh, int64_t lo, int64_t ni) -> int {
    size_t off[kArrays + 1];
    layout(ni, off);
    void* at[kArrays];  // the shard's copy of each array (NULL: absent)
    for (int k = 0; k < kArrays; ++k) at[k] = arr[k].a ? (char*)sh.buf + off[k] : nullptr;
    for (int k = kX0; k < kU; ++k)  // scatter: my columns of the inputs -> [rows][ni] here
      HIP_TRY(copy_cols(at[k], ni, 0, arr[k].a, B, lo, ni, arr[k].rows, arr[k].es, sh.stream));
    cpmpc_step_inputs si = *in;
    si.x0 = at[kX0];
    si.dyn = at[kDyn];
    si.set_point = at[kSetPoint];
    si.terminal_weights = at[kTermW];
    cpmpc_step_outputs o;
    memset(&o, 0, sizeof o);
    o.u = at[kU];
    o.predicted = at[kPred];
    o.status = (int32_t*)at[kStatus];
    o.iterations = (int32_t*)at[kIters];
    o.ls_evals = (int32_t*)at[kLsEvals];
    o.final_cost = at[kCost];
    o.final_eq_l1 = at[kEqL1];
    o.guess = at[kGuess];
    o.solution = at[kSol];
    const int r = cpmpc_step_batch(sh.h, ni, &si, &o, sh.stream);
    if (r) return r;
    for (int k = kU; k < kArrays; ++k)  // gather: the outputs back into my columns of the caller's arrays
      HIP_TRY(copy_cols((void*)arr[k].a, B, lo, at[k], ni, 0, ni, arr[k].rows, arr[k].es, sh.stream));
    return CPMPC_OK;
  };
  auto bytes = [&](int64_t ni) {
    size_t off[kArrays + 1];
    return layout(ni, off);
  };
  rc = sharded_fan_out(s, (hipStream_t)stream, [&](int i, int64_t* lo) { return batch_cols(B, i, n, lo); }, bytes,
                       step_shard);
  if (rc != CPMPC_OK) {
    cpmpc_sharded_reset(s);  // some shards stepped, others did not
    return rc;
  }
  s->warm_total = B;
  return CPMPC_OK;
}

extern "C" int cpmpc_sharded_step_batch(cpmpc_sharded* s, int64_t B, const void* x0, const double* dyn_shared_host,
                                        double set_point, const cpmpc_step_outputs* out, void* stream) {
  if (!s || !x0 || !dyn_shared_host || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  cpmpc_step_inputs in;
  memset(&in, 0, sizeof in);
  in.x0 = x0;
  in.dyn_shared_host = dyn_shared_host;
  in.set_point_shared = set_point;
  return cpmpc_sharded_step_batch_ex(s, B, &in, out, stream);
}

// Optimization::SetPreviousSolution over all shards (optimization.hpp:86-89): z is [dim][B] on the root device, in the
// handle's dtype.  Replaces whatever warm start the shards held; the caller may reuse z once its stream passes this call.
extern "C" int cpmpc_sharded_set_previous_solution(cpmpc_sharded* s, int64_t B, const void* z, void* stream) {
  if (!s || !z) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = sharded_check(s, B);
  if (rc) return rc;
  cpmpc_sharded_reset(s);
  const int n = (int)s->shards.size();
  const size_t es = s->esize, dim = (size_t)s->dim;
  rc = sharded_fan_out(s, (hipStream_t)stream, [&](int i, int64_t* lo) { return batch_cols(B, i, n, lo); },
                       [&](int64_t ni) { return dim * (size_t)ni * es; },
                       [&](Shard& sh, int64_t lo, int64_t ni) -> int {
                         HIP_TRY(copy_cols(sh.buf, ni, 0, z, B, lo, ni, dim, es, sh.stream));
                         return cpmpc_set_previous_solution(sh.h, ni, sh.buf, sh.stream);
                       });
  if (rc != CPMPC_OK) {
    cpmpc_sharded_reset(s);
    return rc;
  }
  s->dist_B = B;
  s->warm_total = B;
  return CPMPC_OK;
}

// The warm start of columns [0, B), B <= cpmpc_sharded_previous_solution_batch(): z_out is [dim][B] on the root device.
// A failed read leaves the warm start as it was.
extern "C" int cpmpc_sharded_get_solution(cpmpc_sharded* s, int64_t B, void* z_out, void* stream) {
  if (!s || !z_out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = sharded_check(s, B);
  if (rc) return rc;
  if (B > s->warm_total)
    return fail(CPMPC_ERR_BATCH, "only %lld problems hold a previous solution, %lld asked for", (long long)s->warm_total, (long long)B);
  const int n = (int)s->shards.size();
  const size_t es = s->esize, dim = (size_t)s->dim;
  // (the shards' columns follow dist_B's split)
  return sharded_fan_out(s, (hipStream_t)stream, [&](int i, int64_t* lo) { return warm_in_shard(s->dist_B, i, n, B, lo); },
                         [&](int64_t ni) { return dim * (size_t)ni * es; },
                         [&](Shard& sh, int64_t lo, int64_t ni) -> int {
                           const int r = cpmpc_get_solution(sh.h, ni, sh.buf, sh.stream);
                           if (r) return r;
                           HIP_TRY(copy_cols(z_out, B, lo, sh.buf, ni, 0, ni, dim, es, sh.stream));
                           return CPMPC_OK;
                         });
}

extern "C" int cpmpc_sharded_set_previous_solution_host(cpmpc_sharded* s, int64_t B, const double* z_host) {
  if (!s || !z_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = sharded_check(s, B);
  if (rc) return rc;
  cpmpc_sharded_reset(s);
  const int n = (int)s->shards.size();
  for (int i = 0; i < n; ++i) {
    int64_t lo, hi;
    shard_range(B, i, n, &lo, &hi);
    if (hi == lo) continue;
    rc = set_prev_host_cols(s->shards[i].h, hi - lo, z_host, B, lo);
    if (rc) {
      cpmpc_sharded_reset(s);
      return rc;
    }
  }
  s->dist_B = B;
  s->warm_total = B;
  return CPMPC_OK;
}

extern "C" int cpmpc_sharded_get_solution_host(cpmpc_sharded* s, int64_t B, double* z_host) {
  if (!s || !z_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = sharded_check(s, B);
  if (rc) return rc;
  if (B > s->warm_total)
    return fail(CPMPC_ERR_BATCH, "only %lld problems hold a previous solution, %lld asked for", (long long)s->warm_total, (long long)B);
  const int n = (int)s->shards.size();
  for (int i = 0; i < n; ++i) {
    int64_t lo;
    const int64_t ni = warm_in_shard(s->dist_B, i, n, B, &lo);
    if (ni == 0) continue;
    rc = get_sol_host_cols(s->shards[i].h, ni, z_host, B, lo);
    if (rc) return rc;
  }
  return CPMPC_OK;
}
