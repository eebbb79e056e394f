// cpmpc_host.hip -- the host-pointer entry points of the C-ABI (include/cpmpc.h): staging slots, worker threads, the
// chunk pipeline (run_host_pipeline, which the sharded host-pointer step runs as well: cpmpc_sharded.hip), the host warm
// start and the handle-less plant step.  No device code: the kernels are reached through the handle's Engine (engine.hpp).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "api_internal.hpp"

int grow_staging(void** dev, void** pin, size_t* cap, size_t bytes, hipStream_t stream) {
  if (*cap >= bytes) return CPMPC_OK;
  HIP_TRY(hipStreamSynchronize(stream));
  if (*dev) (void)hipFree(*dev);
  if (pin && *pin) (void)hipHostFree(*pin);
  *dev = nullptr;
  if (pin) *pin = nullptr;
  *cap = 0;
  const size_t want = bytes < 4096 ? 4096 : bytes;
  hipError_t e = hipMalloc(dev, want);
  if (e != hipSuccess) {
    *dev = nullptr;
    return fail(CPMPC_ERR_ALLOC, "hipMalloc of %zu staging bytes failed: %s", want, hipGetErrorString(e));
  }
  if (pin) {
    e = hipHostMalloc(pin, want, hipHostMallocDefault);
    if (e != hipSuccess) {
      (void)hipFree(*dev);
      *dev = *pin = nullptr;
      return fail(CPMPC_ERR_ALLOC, "hipHostMalloc of %zu staging bytes failed: %s", want, hipGetErrorString(e));
    }
  }
  *cap = want;
  return CPMPC_OK;
}

int ensure_slot(cpmpc_solver* s, int k, size_t bytes) {
  HostSlot& sl = s->slot[k];
  if (sl.stream == nullptr) {
    hipError_t e = hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(CPMPC_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
    if (e == hipSuccess && s->ev_last == nullptr) e = hipEventCreateWithFlags(&s->ev_last, hipEventDisableTiming);
    if (e != hipSuccess) return fail(CPMPC_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
    // device-pointer calls made before the first host-pointer call were not tracked by ev_last: order after them once;
    // a slot stream created later orders itself after whatever the other slots have queued the same way
    HIP_TRY(hipDeviceSynchronize());
  }
  if (s->ev_pending) {  // a device-pointer call on a caller's stream came in between: every slot stream runs after it
    for (int i = 0; i < kHostSlots; ++i)
      if (s->slot[i].stream) HIP_TRY(hipStreamWaitEvent(s->slot[i].stream, s->ev_last, 0));
    s->ev_pending = false;
  }
  return grow_staging(&sl.dev, &sl.pin, &sl.bytes, bytes, sl.stream);
}

// Worker threads for the CPU side of large host-pointer steps (conversion and scatter of the results: a 262 144-problem
// fp64 step returns 420 MB, which one thread moves at ~10 GB/s while PCIe delivers 55).  Created on first use, never
// destroyed (a process-lifetime pool; CPMPC_HOST_THREADS overrides the count, 1 = the calling thread alone).
namespace {
struct HostPool {
  std::mutex m;
  std::condition_variable cv_work, cv_done;
  void (*fn)(int64_t, void*) = nullptr;
  void* ctx = nullptr;
  int64_t n = 0;
  std::atomic<int64_t> next{0};
  uint64_t generation = 0;
  int running = 0;
  int workers = 0;
  std::mutex call;  // one parallel_for at a time
};
HostPool* g_pool = nullptr;
std::once_flag g_pool_once;

void pool_worker(HostPool* p) {
  uint64_t seen = 0;
  for (;;) {
    std::unique_lock<std::mutex> lk(p->m);
    p->cv_work.wait(lk, [&] { return p->generation != seen; });
    seen = p->generation;
    void (*fn)(int64_t, void*) = p->fn;
    void* ctx = p->ctx;
    const int64_t n = p->n;
    lk.unlock();
    for (int64_t i = p->next.fetch_add(1); i < n; i = p->next.fetch_add(1)) fn(i, ctx);
    lk.lock();
    if (--p->running == 0) p->cv_done.notify_all();
  }
}
}  // namespace

void host_parallel_for(int64_t n, void (*fn)(int64_t, void*), void* ctx) {
  std::call_once(g_pool_once, [] {
    g_pool = new HostPool();
    int want = 0;
    if (const char* e = getenv("CPMPC_HOST_THREADS")) want = atoi(e);
    if (want <= 0) {
      const unsigned hw = std::thread::hardware_concurrency();
      want = hw >= 16 ? 8 : (hw >= 4 ? (int)hw / 2 : 1);
    }
    g_pool->workers = want - 1;
    for (int i = 0; i < g_pool->workers; ++i) std::thread(pool_worker, g_pool).detach();
  });
  HostPool* p = g_pool;
  if (p->workers == 0 || n <= 1) {
    for (int64_t i = 0; i < n; ++i) fn(i, ctx);
    return;
  }
  std::lock_guard<std::mutex> one(p->call);
  {
    std::lock_guard<std::mutex> lk(p->m);
    p->fn = fn;
    p->ctx = ctx;
    p->n = n;
    p->next.store(0);
    p->running = p->workers;
    ++p->generation;
  }
  p->cv_work.notify_all();
  for (int64_t i = p->next.fetch_add(1); i < n; i = p->next.fetch_add(1)) fn(i, ctx);
  std::unique_lock<std::mutex> lk(p->m);
  p->cv_done.wait(lk, [&] { return p->running == 0; });
}

extern "C" int cpmpc_host_register(void* ptr, uint64_t bytes) {
  if (!ptr || bytes == 0) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  const hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault);
  if (e != hipSuccess) return fail(CPMPC_ERR_HIP, "hipHostRegister of %llu bytes failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
  return CPMPC_OK;
}
extern "C" int cpmpc_host_unregister(void* ptr) {
  if (!ptr) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  const hipError_t e = hipHostUnregister(ptr);
  if (e != hipSuccess) return fail(CPMPC_ERR_HIP, "hipHostUnregister failed: %s", hipGetErrorString(e));
  return CPMPC_OK;
}

extern "C" int cpmpc_set_host_chunk(cpmpc_solver* s, int64_t problems) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null solver");
  if (problems < -1) return fail(CPMPC_ERR_INVALID_ARG, "chunk size must be >= 0 (0 = never split), or -1 for the default");
  s->host_chunk = problems <= 0 ? problems : (problems + 63) / 64 * 64;
  return CPMPC_OK;
}

static bool host_ptr_is_pinned(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // an ordinary (pageable) host pointer is reported as an error
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// DMA straight into the caller's arrays pays when the predicted states are asked for (160 of the 200 rows a problem
// returns) and every real-typed output array is pinned; for u alone the worker threads' scatter of the mirror is hidden
// behind the kernels and the strided device-to-host copies are not (measured, profiles/r04_host_path.json).
bool host_direct_outputs(const cpmpc_solver* s, const cpmpc_step_host_outputs& out) {
  if (s->dtype != CPMPC_F64 || out.predicted == nullptr) return false;
  if (!host_ptr_is_pinned(out.predicted) || !host_ptr_is_pinned(out.u)) return false;
  if (out.solution && !host_ptr_is_pinned(out.solution)) return false;
  return true;
}

// the chunks of problems [0, Bh) of handle h (its columns start at g_base in the caller's arrays), appended to `work`
void host_chunks_of(cpmpc_solver* h, int64_t Bh, int64_t g_base, bool direct,
                           std::vector<std::vector<HostWork>>& per_handle) {
  std::vector<HostWork> w;
  int64_t n = 1;
  // default: eight chunks of at least 16 384 problems; sixteen of at least 8 192 when the results travel by DMA into the
  // caller's arrays (no CPU scatter to amortise: smaller chunks shorten the drain of the pipeline)
  int64_t chunk = h->host_chunk;
  if (chunk < 0) chunk = direct ? (Bh / 16 > 8192 ? Bh / 16 : 8192) : (Bh / 8 > 16384 ? Bh / 8 : 16384);
  if (chunk > 0 && Bh > chunk + chunk / 2) n = (Bh + chunk - 1) / chunk;
  const int64_t step = ((Bh + n - 1) / n + 63) / 64 * 64;
  for (int64_t c0 = 0; c0 < Bh; c0 += step) w.push_back(HostWork{h, c0, (Bh - c0 < step ? Bh - c0 : step), g_base + c0});
  per_handle.push_back(std::move(w));
}

// Runs the chunks as a pipeline: a handle's chunks rotate through its kHostSlots staging slots, so that while the CPU
// scatters one chunk's results the next is copying back and the one after is in the kernels; the chunks of several
// handles (the shards of cpmpc_sharded_*) are issued round-robin.  Results do not depend on the chunking: a problem's
// arithmetic does not depend on the lanes it occupies or on its neighbours.  Returns after every chunk has landed.
int run_host_pipeline(const std::vector<std::vector<HostWork>>& per_handle, int64_t ld,
                             const cpmpc_step_host_inputs& in, const cpmpc_step_host_outputs& out, bool direct) {
  struct Flight {
    cpmpc_solver* h;
    int slot;
  };
  std::deque<Flight> inflight;
  int first_rc = CPMPC_OK;
  auto end_front = [&]() {
    const Flight f = inflight.front();
    inflight.pop_front();
    DeviceGuard guard(f.h->device);
    if (first_rc == CPMPC_OK) {
      const int rc = engine_of(f.h)->host_chunk_end(f.h, f.slot, ld, out);
      if (rc != CPMPC_OK) first_rc = rc;
    } else {  // after a failure: drain what was started, deliver nothing more
      (void)hipStreamSynchronize(f.h->slot[f.slot].stream);
      f.h->slot[f.slot].busy = false;
    }
  };
  size_t rounds = 0;
  for (const auto& w : per_handle) rounds = w.size() > rounds ? w.size() : rounds;
  for (size_t k = 0; k < rounds && first_rc == CPMPC_OK; ++k) {
    for (const auto& w : per_handle) {
      if (k >= w.size() || first_rc != CPMPC_OK) continue;
      const HostWork& c = w[k];
      const int slot = (int)(k % kHostSlots);
      while (c.h->slot[slot].busy && !inflight.empty()) end_front();  // oldest first: it is the one most likely done
      if (first_rc != CPMPC_OK) break;
      DeviceGuard guard(c.h->device);
      const int rc = engine_of(c.h)->host_chunk_begin(c.h, slot, c.c0, c.Bc, c.g0, ld, in, out, direct);
      if (rc != CPMPC_OK) {
        first_rc = rc;
        break;
      }
      inflight.push_back(Flight{c.h, slot});
    }
  }
  while (!inflight.empty()) end_front();
  return first_rc;
}

int check_host_inputs(const cpmpc_step_host_inputs* in, const cpmpc_step_host_outputs* out) {
  if (!in || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (!in->x0) return fail(CPMPC_ERR_INVALID_ARG, "x0 is required");
  if ((in->dyn_shared == nullptr) == (in->dyn == nullptr))
    return fail(CPMPC_ERR_INVALID_ARG, "exactly one of dyn_shared / dyn must be given");
  if (!in->set_point && !std::isfinite(in->set_point_shared))
    return fail(CPMPC_ERR_INVALID_ARG, "set_point_shared must be finite");
  return CPMPC_OK;
}

extern "C" int cpmpc_step_batch_host_in(cpmpc_solver* s, int64_t B, const cpmpc_step_host_inputs* in,
                                        const cpmpc_step_host_outputs* out) {
  if (!s) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  int rc = check_host_inputs(in, out);
  if (rc) return rc;
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  if (B > s->cap) return fail(CPMPC_ERR_BATCH, "B exceeds capacity");
  std::vector<std::vector<HostWork>> work;
  DeviceGuard guard(s->device);
  const bool direct = host_direct_outputs(s, *out);
  host_chunks_of(s, B, 0, direct, work);
  return run_host_pipeline(work, B, *in, *out, direct);
}

extern "C" int cpmpc_step_batch_host_ex(cpmpc_solver* s, int64_t B, const double* x0_host,
                                        const double* dyn_shared_host, double set_point,
                                        const cpmpc_step_host_outputs* out) {
  if (!s || !x0_host || !dyn_shared_host || !out) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (!std::isfinite(set_point)) return fail(CPMPC_ERR_INVALID_ARG, "set_point must be finite");
  const cpmpc_step_host_inputs in = {x0_host, dyn_shared_host, nullptr, set_point, nullptr, nullptr};
  return cpmpc_step_batch_host_in(s, B, &in, out);
}

extern "C" int cpmpc_step_batch_host(cpmpc_solver* s, int64_t B, const double* x0_host,
                                     const double* dyn_shared_host, double set_point, double* u_host,
                                     double* predicted_host, int32_t* status_host, int32_t* iterations_host,
                                     double* final_cost_host, double* final_eq_l1_host) {
  const cpmpc_step_host_outputs out = {u_host, predicted_host, status_host, iterations_host, final_cost_host,
                                       final_eq_l1_host, nullptr};
  return cpmpc_step_batch_host_ex(s, B, x0_host, dyn_shared_host, set_point, &out);
}

// packed z [dim][n] in the handle's dtype <-> rows [dim] of the caller's double array [dim][ld] at column g0
int set_prev_host_cols(cpmpc_solver* s, int64_t n, const double* z_host, int64_t ld, int64_t g0) {
  DeviceGuard guard(s->device);
  const size_t cnt = (size_t)s->dim * (size_t)n;
  int rc = ensure_slot(s, 0, cnt * s->esize);
  if (rc) return rc;
  HostSlot& sl = s->slot[0];
  for (int r = 0; r < s->dim; ++r) {
    const double* src = z_host + (size_t)r * (size_t)ld + (size_t)g0;
    if (s->dtype == CPMPC_F32) {
      float* h = (float*)sl.pin + (size_t)r * (size_t)n;
      for (int64_t i = 0; i < n; ++i) h[i] = (float)src[i];
    } else {
      memcpy((double*)sl.pin + (size_t)r * (size_t)n, src, (size_t)n * 8);
    }
  }
  HIP_TRY(hipMemcpyAsync(sl.dev, sl.pin, cnt * s->esize, hipMemcpyHostToDevice, sl.stream));
  rc = cpmpc_set_previous_solution(s, n, sl.dev, sl.stream);
  const hipError_t e = hipStreamSynchronize(sl.stream);  // also on failure: the copy above still reads the pinned mirror
  if (rc) return rc;
  if (e != hipSuccess) return fail(CPMPC_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
  return CPMPC_OK;
}

int get_sol_host_cols(cpmpc_solver* s, int64_t n, double* z_host, int64_t ld, int64_t g0) {
  DeviceGuard guard(s->device);
  const size_t cnt = (size_t)s->dim * (size_t)n;
  int rc = ensure_slot(s, 0, cnt * s->esize);
  if (rc) return rc;
  HostSlot& sl = s->slot[0];
  rc = cpmpc_get_solution(s, n, sl.dev, sl.stream);
  if (rc) return rc;
  {
    const hipError_t e = hipMemcpyAsync(sl.pin, sl.dev, cnt * s->esize, hipMemcpyDeviceToHost, sl.stream);
    const hipError_t e2 = hipStreamSynchronize(sl.stream);  // also on failure: the unpack kernel is in flight
    if (e != hipSuccess) return fail(CPMPC_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(CPMPC_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e2));
  }
  for (int r = 0; r < s->dim; ++r) {
    double* dst = z_host + (size_t)r * (size_t)ld + (size_t)g0;
    if (s->dtype == CPMPC_F32) {
      const float* h = (const float*)sl.pin + (size_t)r * (size_t)n;
      for (int64_t i = 0; i < n; ++i) dst[i] = (double)h[i];
    } else {
      memcpy(dst, (const double*)sl.pin + (size_t)r * (size_t)n, (size_t)n * 8);
    }
  }
  return CPMPC_OK;
}

extern "C" int cpmpc_set_previous_solution_host(cpmpc_solver* s, int64_t B, const double* z_host) {
  if (!s || !z_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (B < 1 || B > s->cap) return fail(CPMPC_ERR_BATCH, "B out of range");
  return set_prev_host_cols(s, B, z_host, B, 0);
}

extern "C" int cpmpc_get_solution_host(cpmpc_solver* s, int64_t B, double* z_host) {
  if (!s || !z_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (B < 1 || B > s->cap) return fail(CPMPC_ERR_BATCH, "B out of range");
  return get_sol_host_cols(s, B, z_host, B, 0);
}

// One call of the sensitivity family with HOST doubles, arguments checked by the caller: one staging slot,
// [the inputs that are given, in order | the outputs that are asked for, in order | ok] in the handle's dtype, one copy in,
// `launch` on the slot's stream with the device addresses (NULL where the host pointer is), one copy out, one
// synchronisation -- also when `launch` fails: the copy in still reads the pinned mirror.
template <int NI, int NO, typename Launch>
static int staged_host_call(cpmpc_solver* s, int64_t B, const void* const (&src)[NI], const size_t (&n_in)[NI],
                            double* const (&dst)[NO], const size_t (&n_out)[NO], int32_t* ok_host, Launch launch) {
  DeviceGuard guard(s->device);
  const size_t nB = (size_t)B, e = s->esize;
  size_t first_in[NI], first_out[NO], n_ins = 0, n_outs = 0;
  for (int i = 0; i < NI; ++i) {
    first_in[i] = n_ins;
    if (src[i]) n_ins += n_in[i];
  }
  for (int i = 0; i < NO; ++i) {
    first_out[i] = n_outs;
    if (dst[i]) n_outs += n_out[i];
  }
  const size_t off_out = n_ins * e, off_ok = off_out + n_outs * e;
  int rc = ensure_slot(s, 0, off_ok + nB * sizeof(int32_t));
  if (rc) return rc;
  HostSlot& sl = s->slot[0];
  for (int i = 0; i < NI; ++i) {
    if (!src[i]) continue;
    const double* d = (const double*)src[i];
    if (s->dtype == CPMPC_F32) {
      float* h = (float*)sl.pin + first_in[i];
      for (size_t j = 0; j < n_in[i]; ++j) h[j] = (float)d[j];
    } else {
      memcpy((double*)sl.pin + first_in[i], d, n_in[i] * 8);
    }
  }
  if (off_out) HIP_TRY(hipMemcpyAsync(sl.dev, sl.pin, off_out, hipMemcpyHostToDevice, sl.stream));
  char* const d_base = (char*)sl.dev;
  const void* d_in[NI];
  void* d_o[NO];
  for (int i = 0; i < NI; ++i) d_in[i] = src[i] ? d_base + first_in[i] * e : nullptr;
  for (int i = 0; i < NO; ++i) d_o[i] = dst[i] ? d_base + off_out + first_out[i] * e : nullptr;
  rc = launch(d_in, d_o, (int32_t*)(d_base + off_ok), sl.stream);
  hipError_t e1 = hipSuccess;
  if (rc == CPMPC_OK)
    e1 = hipMemcpyAsync((char*)sl.pin + off_out, d_base + off_out, n_outs * e + nB * sizeof(int32_t), hipMemcpyDeviceToHost,
                        sl.stream);
  const hipError_t e2 = hipStreamSynchronize(sl.stream);
  if (rc) return rc;
  if (e1 != hipSuccess) return fail(CPMPC_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e1));
  if (e2 != hipSuccess) return fail(CPMPC_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e2));
  for (int i = 0; i < NO; ++i) {
    if (!dst[i]) continue;
    const char* base = (const char*)sl.pin + off_out;
    if (s->dtype == CPMPC_F32) {
      const float* h = (const float*)base + first_out[i];
      for (size_t j = 0; j < n_out[i]; ++j) dst[i][j] = (double)h[j];
    } else {
      memcpy(dst[i], (const double*)base + first_out[i], n_out[i] * 8);
    }
  }
  if (ok_host) memcpy(ok_host, (const char*)sl.pin + off_ok, nB * sizeof(int32_t));
  return CPMPC_OK;
}

// Feedback gains, plan sensitivities and their reverse mode with HOST doubles: the inputs are [dyn? | terminal_weights? | z? |
// gbar?].  What the three outputs are depends on the call:
//   kGain         cpmpc_feedback_gain_batch:    out0 = K [n_rows][NX][B]; out1, out2 and gbar absent
//   kSensitivity  cpmpc_plan_sensitivity_batch: out0 = K [n_rows][NX][B], out1 = k_sp [n_rows][B], out2 = k_up [n_rows][B]
//   kVjp          cpmpc_plan_vjp_batch:         gbar [n_rows][B] travels in with the inputs; out0 = g_x0 [NX][B],
//                                               out1 = g_sp [B], out2 = g_up [B] -- one row each
enum class HostSensCall { kGain, kSensitivity, kVjp };
static int sensitivities_host(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows, HostSensCall call,
                              const double* gbar_host, double* K_host, double* k_sp_host, double* k_up_host,
                              int32_t* ok_host) {
  const size_t nB = (size_t)B;
  const bool vjp = call == HostSensCall::kVjp;
  const size_t out_rows = vjp ? 1 : (size_t)n_rows;
  const void* const src[4] = {in->dyn, in->terminal_weights, in->z, vjp ? gbar_host : nullptr};
  const size_t n_in[4] = {(size_t)s->NP * nB, (size_t)s->NX * nB, (size_t)s->dim * nB, (size_t)n_rows * nB};
  double* const dst[3] = {K_host, k_sp_host, k_up_host};
  const size_t n_out[3] = {out_rows * (size_t)s->NX * nB, out_rows * nB, out_rows * nB};
  return staged_host_call(s, B, src, n_in, dst, n_out, ok_host,
                          [&](const void* const* d_in, void* const* d_o, int32_t* d_ok, hipStream_t stream) {
                            cpmpc_gain_inputs di = *in;
                            di.dyn = d_in[0];
                            di.terminal_weights = d_in[1];
                            di.z = d_in[2];
                            switch (call) {
                              case HostSensCall::kGain:
                                return cpmpc_feedback_gain_batch(s, B, &di, n_rows, d_o[0], d_ok, stream);
                              case HostSensCall::kSensitivity:
                                return cpmpc_plan_sensitivity_batch(s, B, &di, n_rows, d_o[0], d_o[1], d_o[2], d_ok, stream);
                              case HostSensCall::kVjp:
                                break;
                            }
                            return cpmpc_plan_vjp_batch(s, B, &di, n_rows, d_in[3], d_o[0], d_o[1], d_o[2], d_ok, stream);
                          });
}

extern "C" int cpmpc_feedback_gain_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows,
                                              double* K_host, int32_t* ok_host) {
  const int rc = check_gain_args(s, B, in, n_rows, K_host);
  if (rc) return rc;
  return sensitivities_host(s, B, in, n_rows, HostSensCall::kGain, nullptr, K_host, nullptr, nullptr, ok_host);
}

extern "C" int cpmpc_plan_sensitivity_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows,
                                                 double* K_host, double* k_sp_host, double* k_up_host, int32_t* ok_host) {
  const int rc = check_gain_args(s, B, in, n_rows, K_host ? K_host : (k_sp_host ? k_sp_host : k_up_host));
  if (rc) return rc;
  return sensitivities_host(s, B, in, n_rows, HostSensCall::kSensitivity, nullptr, K_host, k_sp_host, k_up_host, ok_host);
}

extern "C" int cpmpc_plan_vjp_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_gain_inputs* in, int n_rows,
                                         const double* gbar_host, double* g_x0_host, double* g_sp_host, double* g_up_host,
                                         int32_t* ok_host) {
  if (!gbar_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument (gbar)");
  const int rc = check_gain_args(s, B, in, n_rows, g_x0_host ? g_x0_host : (g_sp_host ? g_sp_host : g_up_host));
  if (rc) return rc;
  return sensitivities_host(s, B, in, n_rows, HostSensCall::kVjp, gbar_host, g_x0_host, g_sp_host, g_up_host, ok_host);
}

// The weight gradients with HOST doubles: the inputs are [dyn? | terminal_weights? | z? | x0 | set_point? | u_prev? | gbar?], the
// outputs [g_tw? | g_wu? | g_wdu? | du?] (staged_host_call).
extern "C" int cpmpc_plan_weight_vjp_batch_host(cpmpc_solver* s, int64_t B, const cpmpc_weight_vjp_inputs* in, int n_rows,
                                                const double* gbar_host, double* g_tw_host, double* g_wu_host,
                                                double* g_wdu_host, double* du_host, int32_t* ok_host) {
  const int rc = check_weight_vjp_args(s, B, in, n_rows, gbar_host, g_tw_host, g_wu_host, g_wdu_host, du_host);
  if (rc) return rc;
  const size_t nB = (size_t)B;
  const void* const src[7] = {in->lin.dyn, in->lin.terminal_weights, in->lin.z, in->x0, in->set_point, in->u_prev, gbar_host};
  const size_t n_in[7] = {(size_t)s->NP * nB, (size_t)s->NX * nB, (size_t)s->dim * nB, (size_t)s->NX * nB, nB, nB,
                          (size_t)n_rows * nB};
  double* const dst[4] = {g_tw_host, g_wu_host, g_wdu_host, du_host};
  const size_t n_out[4] = {(size_t)s->NX * nB, nB, nB, (size_t)n_rows * nB};
  return staged_host_call(s, B, src, n_in, dst, n_out, ok_host,
                          [&](const void* const* d_in, void* const* d_o, int32_t* d_ok, hipStream_t stream) {
                            cpmpc_weight_vjp_inputs di = *in;
                            di.lin.dyn = d_in[0];
                            di.lin.terminal_weights = d_in[1];
                            di.lin.z = d_in[2];
                            di.x0 = d_in[3];
                            di.set_point = d_in[4];
                            di.u_prev = d_in[5];
                            return cpmpc_plan_weight_vjp_batch(s, B, &di, n_rows, d_in[6], d_o[0], d_o[1], d_o[2], d_o[3], d_ok,
                                                               stream);
                          });
}

// Staging of the handle-less host-pointer plant step: per host thread and device, grown on demand and kept (a
// Simulator::Step per 10 ms tick must not allocate; simulator.cc:11-36 has no allocation either).
struct SimStage {
  int device = -1;
  void* dev = nullptr;
  void* pin = nullptr;
  size_t bytes = 0;
  hipStream_t stream = nullptr;
  // never freed: at thread/process exit the HIP runtime may already be gone (a few KB per calling thread)
};
static thread_local SimStage g_sim_stage;

static int ensure_sim_stage(size_t bytes) {
  SimStage& g = g_sim_stage;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (g.device != dev) {
    if (g.dev) (void)hipFree(g.dev);
    if (g.pin) (void)hipHostFree(g.pin);
    if (g.stream) (void)hipStreamDestroy(g.stream);
    g.dev = g.pin = nullptr;
    g.stream = nullptr;
    g.bytes = 0;
    g.device = dev;
  }
  if (g.stream == nullptr) HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  return grow_staging(&g.dev, &g.pin, &g.bytes, bytes, g.stream);
}

extern "C" int cpmpc_sim_step_batch_host(int64_t B, const double* dyn_shared_host, double dt, const double* u_host,
                                         const double* fext_host, double* state_host) {
  if (!dyn_shared_host || !u_host || !state_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  for (int64_t i = 0; i < B; ++i)
    if (!std::isfinite(u_host[i])) return fail(CPMPC_ERR_INVALID_ARG, "u = %g is not finite (simulator.cc:14)", u_host[i]);
  int rc = current_device_ok();
  if (rc) return rc;
  const size_t nB = (size_t)B;
  rc = ensure_sim_stage(5 * nB * sizeof(double));
  if (rc) return rc;
  SimStage& g = g_sim_stage;
  // [state 4B | u B]: one copy in, the kernel, one copy out, one synchronisation
  double* h = (double*)g.pin;
  double* d = (double*)g.dev;
  memcpy(h, state_host, 4 * nB * sizeof(double));
  memcpy(h + 4 * nB, u_host, nB * sizeof(double));
  HIP_TRY(hipMemcpyAsync(d, h, 5 * nB * sizeof(double), hipMemcpyHostToDevice, g.stream));
  rc = cpmpc_sim_step_batch(CPMPC_F64, B, dyn_shared_host, dt, d + 4 * nB, fext_host, nullptr, d, g.stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h, d, 4 * nB * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_TRY(hipStreamSynchronize(g.stream));
  memcpy(state_host, h, 4 * nB * sizeof(double));
  return CPMPC_OK;
}

// A = dx+/dx and Bu = dx+/du of the same step with host doubles (pendulum::Simulator::StepJacobian): the staging of the plant
// step above, [state NX B | u B | A NX NX B | Bu NX B]; one copy in, the kernel, one copy out, one synchronisation.
extern "C" int cpmpc_sim_step_jac_batch_host(int model, int64_t B, const double* dyn_shared_host, double dt,
                                             const double* state_host, const double* u_host, const double* fext_host,
                                             double* A_host, double* Bu_host) {
  if (!dyn_shared_host || !state_host || !u_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (!A_host && !Bu_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument (no output asked for)");
  if (model != CPMPC_MODEL_SINGLE && model != CPMPC_MODEL_DOUBLE) return fail(CPMPC_ERR_INVALID_ARG, "unknown model");
  if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(CPMPC_ERR_INVALID_ARG, "dt must be finite and >= 0 (simulator.cc:13)");
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  for (int64_t i = 0; i < B; ++i)
    if (!std::isfinite(u_host[i])) return fail(CPMPC_ERR_INVALID_ARG, "u = %g is not finite (simulator.cc:14)", u_host[i]);
  int rc = current_device_ok();
  if (rc) return rc;
  const size_t nB = (size_t)B, nx = (size_t)cpmpc_model_state_dim(model);
  const size_t n_in = (nx + 1) * nB, n_out = (nx * nx + nx) * nB;
  rc = ensure_sim_stage((n_in + n_out) * sizeof(double));
  if (rc) return rc;
  SimStage& g = g_sim_stage;
  double* h = (double*)g.pin;
  double* d = (double*)g.dev;
  memcpy(h, state_host, nx * nB * sizeof(double));
  memcpy(h + nx * nB, u_host, nB * sizeof(double));
  HIP_TRY(hipMemcpyAsync(d, h, n_in * sizeof(double), hipMemcpyHostToDevice, g.stream));
  cpmpc_sim_jac a;
  memset(&a, 0, sizeof a);
  a.struct_size = sizeof a;
  a.state = d;
  a.u = d + nx * nB;
  a.fext_host = fext_host;
  a.A = d + n_in;
  a.Bu = d + n_in + nx * nx * nB;
  rc = cpmpc_sim_step_jac_batch(model, CPMPC_F64, B, dyn_shared_host, dt, &a, g.stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h + n_in, d + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_TRY(hipStreamSynchronize(g.stream));
  if (A_host) memcpy(A_host, h + n_in, nx * nx * nB * sizeof(double));
  if (Bu_host) memcpy(Bu_host, h + n_in + nx * nx * nB, nx * nB * sizeof(double));
  return CPMPC_OK;
}

// P = dx+/dp (and x+) of the same step with host doubles and the shared parameter set (pendulum::Simulator::StepParamJacobian):
// the same staging, [state NX B | u B | P NX NP B | x_new NX B].
extern "C" int cpmpc_sim_step_param_jac_batch_host(int model, int64_t B, const double* dyn_shared_host, double dt,
                                                   const double* state_host, const double* u_host, const double* fext_host,
                                                   double* P_host, double* x_new_host) {
  if (!dyn_shared_host || !state_host || !u_host || !P_host) return fail(CPMPC_ERR_INVALID_ARG, "null argument");
  if (model != CPMPC_MODEL_SINGLE && model != CPMPC_MODEL_DOUBLE) return fail(CPMPC_ERR_INVALID_ARG, "unknown model");
  if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(CPMPC_ERR_INVALID_ARG, "dt must be finite and >= 0 (simulator.cc:13)");
  if (B < 1) return fail(CPMPC_ERR_INVALID_ARG, "B must be >= 1");
  for (int64_t i = 0; i < B; ++i)
    if (!std::isfinite(u_host[i])) return fail(CPMPC_ERR_INVALID_ARG, "u = %g is not finite (simulator.cc:14)", u_host[i]);
  int rc = current_device_ok();
  if (rc) return rc;
  const size_t nB = (size_t)B, nx = (size_t)cpmpc_model_state_dim(model), np = (size_t)cpmpc_model_num_params(model);
  const size_t n_in = (nx + 1) * nB, n_out = (nx * np + nx) * nB;
  rc = ensure_sim_stage((n_in + n_out) * sizeof(double));
  if (rc) return rc;
  SimStage& g = g_sim_stage;
  double* h = (double*)g.pin;
  double* d = (double*)g.dev;
  memcpy(h, state_host, nx * nB * sizeof(double));
  memcpy(h + nx * nB, u_host, nB * sizeof(double));
  HIP_TRY(hipMemcpyAsync(d, h, n_in * sizeof(double), hipMemcpyHostToDevice, g.stream));
  cpmpc_sim_param_jac a;
  memset(&a, 0, sizeof a);
  a.struct_size = sizeof a;
  a.state = d;
  a.u = d + nx * nB;
  a.fext_host = fext_host;
  a.P = d + n_in;
  a.x_new = d + n_in + nx * np * nB;
  rc = cpmpc_sim_step_param_jac_batch(model, CPMPC_F64, B, dyn_shared_host, dt, &a, g.stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h + n_in, d + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_TRY(hipStreamSynchronize(g.stream));
  memcpy(P_host, h + n_in, nx * np * nB * sizeof(double));
  if (x_new_host) memcpy(x_new_host, h + n_in + nx * np * nB, nx * nB * sizeof(double));
  return CPMPC_OK;
}
