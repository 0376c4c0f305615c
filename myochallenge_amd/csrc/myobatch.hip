// myobatch.hip — libmyobatch (C ABI in include/myobatch.h): the HIP backend, the gfx950 kernels and the entry points that launch them.
//   hipcc --offload-arch=gfx950  -> libmyobatch.so   (the product; no CPU path)
// One workgroup = one wavefront = one environment; grid = number of environments.
// The host side it shares with the test tooling (model tables, batch records, myo_batch_create, the kernel variant of a batch, the record
// accessors and every env-path entry point) is csrc/myo_host.h, written over the backend primitives defined here; the lane-serial
// emulation of the same kernel SOURCE is another translation unit (csrc/myobatch_emu.cpp + csrc/emu_host.h), not a path of this one.
#include <hip/hip_runtime.h>
#include <utility>
#include <vector>
#define MYO_BACKEND_NAME "gfx950"
#define MYO_BACKEND_DENSE_NEWTON 0
#define MYO_BACKEND_BATCH_FIELDS hipEvent_t ev0, ev1; std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
#define MYO_BACKEND_RENDER_ENVS_MAX 65535      /* (gridDim.y of the ray cast) */
// every launch entry point runs on the batch's own device, whatever the caller's current device is
struct DeviceGuard {
  int prev = -1; bool switched = false;
  explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess); }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#include "myo_host.h"

// ------------------------------------------------------------------------------------------ backend
static int be_malloc(void** p, size_t n) { return (int)hipMalloc(p, n ? n : 1); }
static void be_free(void* p) { (void)hipFree(p); }
static int be_h2d(void* d, const void* h, size_t n) { return (int)hipMemcpy(d, h, n, hipMemcpyHostToDevice); }
static int be_set_device(int dev) { return (int)hipSetDevice(dev); }
static const char* be_errstr(int e) { return hipGetErrorString((hipError_t)e); }

// Model / task parameters live in __constant__ memory (scalar loads in every phase function).  __constant__
// symbols exist once PER DEVICE, so what is bound is tracked per device; they are (re)uploaded on the launch
// stream whenever a different batch launches on that device.  If the batch bound before launched on another
// stream, the upload first waits for that stream's work (its kernels may still be reading the constants).
#define MYO_MAX_DEVICES 64
struct BoundDev { const myo_batch* b = nullptr; hipStream_t last = nullptr; bool have_last = false; hipEvent_t ev = nullptr; };
static BoundDev g_bound[MYO_MAX_DEVICES];
static std::mutex g_bound_mu;
// The workspace blocks (TaskDev::ctrl_ws, myo_physics.h): MYO_WS_SLOTS x MYO_ENVWS_N doubles (~60 MB) and their owner flags
// (myo_ws_acquire / myo_ws_release, wave.h) per DEVICE, shared by every fp64 batch on it — a workgroup owns a block while it holds an
// env, so kernels of different batches, even on different streams, never meet in one.  Allocated with the first such batch, freed
// with the last.
struct SlotWs { double* p = nullptr; int* map = nullptr; int users = 0; char* big = nullptr; int big_users = 0; };
static SlotWs g_slot_ws[MYO_MAX_DEVICES];
static bool slot_workspace_acquire(int device, double** ws, int** map) {
  if (device < 0 || device >= MYO_MAX_DEVICES) return false;
  std::lock_guard<std::mutex> lk(g_bound_mu);
  SlotWs& w = g_slot_ws[device];
  if (!w.p) {
    void *q = nullptr, *mp = nullptr;
    const size_t bytes = sizeof(double) * (size_t)MYO_WS_SLOTS * MYO_ENVWS_N, mbytes = sizeof(int) * (size_t)MYO_WS_SLOTS;      // (the blocks' owner flags: 0 = free)
    if (hipMalloc(&q, bytes) != hipSuccess) return false;
    if (hipMalloc(&mp, mbytes) != hipSuccess) { (void)hipFree(q); return false; }
    if (hipMemset(q, 0, bytes) != hipSuccess || hipMemset(mp, 0, mbytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      (void)hipFree(q); (void)hipFree(mp);
      return false;
    }
    w.p = (double*)q; w.map = (int*)mp; w.users = 0;
  }
  w.users++;
  *ws = w.p; *map = w.map;
  return true;
}
static void slot_workspace_release(int device) {
  if (device < 0 || device >= MYO_MAX_DEVICES) return;
  std::lock_guard<std::mutex> lk(g_bound_mu);
  SlotWs& w = g_slot_ws[device];
  if (w.users > 0 && --w.users == 0) { (void)hipFree(w.p); (void)hipFree(w.map); w.p = nullptr; w.map = nullptr; }
}
// ... and the blocks of the 48-slot fp64 scratch (TaskDev::big_ws: contact records + wrap results, MYO_BIGWS_BYTES per dense slot index,
// ~200 MB): allocated with the first batch that needs them (a die, extended collision pairs, condim 4 / 6), freed with the last
static char* big_workspace_acquire(int device) {
  if (device < 0 || device >= MYO_MAX_DEVICES) return nullptr;
  std::lock_guard<std::mutex> lk(g_bound_mu);
  SlotWs& w = g_slot_ws[device];
  if (!w.big) {
    void* q = nullptr;
    const size_t bytes = (size_t)MYO_WS_SLOTS * MYO_BIGWS_BYTES;
    if (hipMalloc(&q, bytes) != hipSuccess) return nullptr;
    if (hipMemset(q, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(q); return nullptr; }
    w.big = (char*)q; w.big_users = 0;
  }
  w.big_users++;
  return w.big;
}
static void big_workspace_release(int device) {
  if (device < 0 || device >= MYO_MAX_DEVICES) return;
  std::lock_guard<std::mutex> lk(g_bound_mu);
  SlotWs& w = g_slot_ws[device];
  if (w.big_users > 0 && --w.big_users == 0) { (void)hipFree(w.big); w.big = nullptr; }
}
static void unbind(const myo_batch* b, int device) {
  std::lock_guard<std::mutex> lk(g_bound_mu);
  if (device >= 0 && device < MYO_MAX_DEVICES && g_bound[device].b == b) g_bound[device].b = nullptr;
}
static int bind_constants(myo_batch* b, hipStream_t st) {
  if (b->device < 0 || b->device >= MYO_MAX_DEVICES) return fail(MYO_E_ARG, "device index out of range");
  std::lock_guard<std::mutex> lk(g_bound_mu);
  BoundDev& g = g_bound[b->device];
  if (g.b == b) { g.last = st; g.have_last = true; return 0; }
  hipError_t e = hipSuccess;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  if (g.b && g.have_last && g.last != st && cap == hipStreamCaptureStatusNone) {
    if (!g.ev) e = hipEventCreateWithFlags(&g.ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(g.ev, g.last);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, g.ev, 0);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipSuccess; }    // the other stream may be gone: nothing left to wait for
  }
  if (b->dtype == MYO_F64) e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_model_d), &b->Md, sizeof b->Md, 0, hipMemcpyHostToDevice, st);
  else e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_model_f), &b->Mf, sizeof b->Mf, 0, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_task), &b->K, sizeof b->K, 0, hipMemcpyHostToDevice, st);
#ifdef MYO_STAGECOUNT
  { static int rep; const char* r = getenv("MYO_DBG_REPEAT"); rep = r ? atoi(r) : 0; if (e == hipSuccess) e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_dbg_repeat), &rep, sizeof rep, 0, hipMemcpyHostToDevice, st); }
#endif
  if (e != hipSuccess) return fail(MYO_E_DEVICE, "binding model constants failed: %s", hipGetErrorString(e));
  g.b = b; g.last = st; g.have_last = true;
  return 0;
}

// ------------------------------------------------------------------------------------------ kernels
#ifdef MYO_PROF
__device__ unsigned long long g_prof[MYO_NPROF];
extern "C" int myo_debug_read_prof(double* out16, int reset) {     /* out16: MYO_NPROF (32) doubles */
  unsigned long long h[MYO_NPROF];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_prof), sizeof h) != hipSuccess) return -1;
  for (int k = 0; k < MYO_NPROF; ++k) out16[k] = (double)h[k];
  if (reset) { memset(h, 0, sizeof h); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prof), h, sizeof h); }
  return 0;
}
#endif
// RK4 stage storage of this workgroup: behind the scratch in LDS where MYO_RK_IN_LDS says so (csrc/myo_host.h: variant_lds_bytes sizes
// the launch by the same macros), in global memory otherwise
static_assert(MYO_LDS_ALIGN(sizeof(Scratch<float, MYO_NCON_MAX>)) + sizeof(RkScratch<float>) <= 20480, "RK4 stage storage next to the scratch: eight workgroups per CU");
template <typename T, bool RK, int NC>
__device__ __forceinline__ RkScratch<T>* rk_storage() {
  if constexpr (!RK) return nullptr;
  else if constexpr (MYO_RK_IN_LDS(T, NC)) return reinterpret_cast<RkScratch<T>*>(myo_lds + MYO_LDS_ALIGN(sizeof(Scratch<T, NC>)));
  else return reinterpret_cast<RkScratch<T>*>(c_task.rk_ws) + blockIdx.x;
}
#ifdef MYO_WGTIME
// developer diagnostic (tools/dev/gpu_wgtime.py): start / end of every workgroup of the last k_step launch on the 100 MHz wall clock
__device__ unsigned long long g_wg_time[2 * 16384];
extern "C" int myo_debug_read_wgtime(unsigned long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_time), sizeof(unsigned long long) * 2 * (size_t)(n < 16384 ? n : 16384)) == hipSuccess ? 0 : -1;
}
#endif
// ---- launch order of the env steps.  A step of 4096 envs is two rounds over the chip's 2048 one-wave slots, and an env step
// takes 0.8 .. 1.6 x the mean (contacts, Newton iterations): in index order the second job of a slot starts whenever its first
// ends, the slot sums spread, and the launch waits for the worst one — measured (tools/dev/gpu_wgtime.py): 28 % of slots x
// makespan idle, the last quarter of the launch running on a fraction of the chip.  The dispatcher hands workgroups to freed
// slots in blockIdx order, so the ORDER is the only lever a one-env-per-workgroup kernel has: longest predicted first — the long
// jobs start at once, the short ones fill the slots as they free up (list scheduling, LPT).  Prediction = exponentially smoothed
// duration of the env's own last steps (k_step times every env on the 100 MHz wall clock; the step-to-step correlation of the
// durations is ~0.5, the smoothing keeps the persistent half).  The results of a step do not depend on the order.
// k_step_order: ONE block; cost <- (cost + ticks) / 2, 256 cost buckets between the batch minimum and maximum, counting sort
// (descending) -> order.  Which env comes first inside a bucket is left to the LDS atomics: irrelevant to the results.
__global__ void __launch_bounds__(1024) k_step_order(const unsigned int* __restrict__ ticks, float* __restrict__ cost, int n, int* __restrict__ order,
                                                     int* __restrict__ step_gen) {
  __shared__ float s_lo[16], s_hi[16];
  __shared__ unsigned int s_cnt[256], s_off[256];
  const int t = threadIdx.x;
  if (step_gen && t == 0) step_gen[0] = (int)((unsigned)step_gen[0] + 1u);          // the next launch is the next generation of the part protocol
  if (!order) return;
  float lo = 3.4e38f, hi = 0.f;
  for (int i = t; i < n; i += 1024) {
    const float tk = (float)ticks[i], c0 = cost[i];
    const float c = c0 > 0.f ? 0.5f * (c0 + tk) : tk;
    cost[i] = c;
    lo = fminf(lo, c); hi = fmaxf(hi, c);
  }
  for (int off = 32; off >= 1; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off, 64)); hi = fmaxf(hi, __shfl_xor(hi, off, 64)); }
  if ((t & 63) == 0) { s_lo[t >> 6] = lo; s_hi[t >> 6] = hi; }
  if (t < 256) s_cnt[t] = 0;
  __syncthreads();
  lo = s_lo[0]; hi = s_hi[0];
  for (int k = 1; k < 16; ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); }
  const float scale = hi > lo ? 255.99f / (hi - lo) : 0.f;
  for (int i = t; i < n; i += 1024) atomicAdd(&s_cnt[255 - (int)((cost[i] - lo) * scale)], 1u);
  __syncthreads();
  if (t == 0) { unsigned a = 0; for (int k = 0; k < 256; ++k) { s_off[k] = a; a += s_cnt[k]; } }
  __syncthreads();
  for (int i = t; i < n; i += 1024) order[atomicAdd(&s_off[255 - (int)((cost[i] - lo) * scale)], 1u)] = i;
}
// ---- env steps in parts.  Even in the best order a slot's two jobs add up their spreads and the launch ends with one job-long
// tail on a draining chip.  The tail is as long as the LAST job of a slot: so an env step is cut into P jobs of decreasing
// length (default 7 + 3 substeps), blocks p n .. (p+1) n - 1 running part p, handed over through the env record in HBM.  In
// dispatch order every part p is placed before any part p + 1, the long jobs run with the chip full, and what drains at the
// end is the short jobs' tail (simulated with the measured duration spread: makespan 2.50 -> 2.20 ms for 7 + 3; measured
// 2.82 -> 2.45 ms, 2.39 with the launch order above; the states are bit-identical).
// Protocol (placement- and dispatch-order-independent; MI355X_MICROARCH.md "inter-workgroup visibility").  part_state[env] =
// 16 g + 2 q: parts < q of step g are published; + 1: part q is claimed and running.  A workgroup of part p polls (relaxed,
// agent scope): a state past "part p claimed" -> nothing left to do, exit; 16 g + 2 q with q <= p -> claim q (agent-scope CAS)
// and run parts q .. p back to back (q < p only if an earlier part's block has not been placed yet: that block then finds
// its part taken and exits); 16 g + 2 q + 1 with q < p -> the producer is RUNNING somewhere: sleep and poll again — no
// workgroup ever waits for one that is not running.  Taking over a record another workgroup published: ONE agent acquire fence
// after the poll, then plain loads.  Publishing: store the record, drain the stores, agent release fence, drain, relaxed
// agent-scope store of the new state (16 (g + 1) after the last part: the next launch's generation).
template <typename T, bool RK, int NC>
__global__ void __launch_bounds__(64, 2) k_step(EnvRecordLayout L, double* rec, const float* act,
                                             float* obs, float* rew, unsigned char* done, unsigned char* trunc,
                                             float* term_obs, float* comps, float* ep_info, unsigned char* bad_state,
                                             const int* __restrict__ order, unsigned int* __restrict__ ticks,
                                             int* part_state, const int* __restrict__ step_gen, StepPlan plan) {
  Scratch<T, NC>& s = *reinterpret_cast<Scratch<T, NC>*>(myo_lds);
  s.rk = rk_storage<T, RK, NC>();
  const DevModel<T>& M = myo_cmodel<T>();
  const TaskDev& K = c_task;
  const int nparts = part_state ? plan.nparts : 1;
  const int nenv = (int)gridDim.x / nparts;
  const int p = (int)blockIdx.x / nenv;
  const int slot = (int)blockIdx.x - p * nenv;
  const int env = order ? order[slot] : slot;
  const unsigned long long t_start = ticks ? wall_clock64() : 0ull;
#ifdef MYO_WGTIME
  if (threadIdx.x == 0 && blockIdx.x < 16384) g_wg_time[2 * blockIdx.x] = wall_clock64();
#endif
#ifdef MYO_PROF
  if (threadIdx.x == 0) { for (int k = 0; k < MYO_NPROF; ++k) s.prof[k] = 0; s.prof_t = clock64(); }
  __syncthreads();
#endif
  int q = 0;                                   // first part this workgroup runs
  int* st = nullptr;
  unsigned base = 0;
  int last = 1;
  if (part_state) {
    base = 16u * (unsigned)step_gen[0];     // (all state arithmetic is modulo 2^32: the generation counter may wrap)
    st = part_state + env;
    int from = -1;                             // decided by lane 0: the part to start from, -1 = nothing to do
    if (threadIdx.x == 0) {
      for (;;) {
        const int v = __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned j = (unsigned)v - base;
        if (j > 2u * (unsigned)p) {             // part p is claimed or done: exit.  A state of ANOTHER generation (neither a part of this
          // step nor its final 16 (g + 1)) means step_gen and part_state have come apart — a failed launch, two streams stepping one
          // batch: the step would silently write nothing, so it is counted (myo_batch_protocol_errors) and the env flagged
          if (j > 2u * (unsigned)nparts && j != 16u) { if (K.health) atomicAdd(K.health, 1); if (bad_state) bad_state[env] = 1; }
          break;
        }
        if ((j & 1) == 0) {
          int expect = v;
          if (__hip_atomic_compare_exchange_strong(st, &expect, (int)((unsigned)v + 1u), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { from = (int)(j >> 1); break; }
          continue;
        }
        __builtin_amdgcn_s_sleep(32);           // an earlier part is running
      }
    }
    from = __builtin_amdgcn_readfirstlane(from);
    if (from < 0) return;
    q = from;
    if (q > 0) {                               // the record was published by another workgroup of this launch
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    last = p == nparts - 1;
  }
  // ONE call site — the kernel holds one copy of the step: substeps k_lo .. k_hi of the frame_skip (a launch without a plan: the whole step)
  const int k_lo = part_state ? plan.k[q] : 0, k_hi = (part_state && !last) ? plan.k[p + 1] : -1, pub = (part_state && plan.wt && !last) ? 1 : 0;
  env_step<T, RK ? 1 : 0>(M, K, L, rec + (size_t)env * L.stride, s, env, act, obs, rew, done, trunc, term_obs, comps, ep_info, bad_state, k_lo, k_hi, pub);
  if (part_state) {
    // (the duration is added BEFORE the part is published: the next part's workgroup may run, and add its own, the moment it is)
    if (ticks && threadIdx.x == 0) {
      const unsigned int d = (unsigned int)(wall_clock64() - t_start) + (q > 0 ? ticks[env] : 0u);
      if (plan.wt) __hip_atomic_store(ticks + env, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else ticks[env] = d;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      if (!last && !plan.wt) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
      __hip_atomic_store(st, (int)(last ? base + 16u : base + 2u * (unsigned)p + 2u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
    if (ticks && threadIdx.x == 0) ticks[env] = (unsigned int)(wall_clock64() - t_start);
  }
#ifdef MYO_WGTIME
  if (threadIdx.x == 0 && blockIdx.x < 16384) g_wg_time[2 * blockIdx.x + 1] = wall_clock64();
#endif
#ifdef MYO_PROF
  PROF(s, 0)
  __syncthreads();
  if (threadIdx.x < MYO_NPROF) atomicAdd(&g_prof[threadIdx.x], s.prof[threadIdx.x]);
#endif
}
// Every other env-path launch: block blockIdx.x runs job J (csrc/myo_task.h, myo_sense.h, myo_render.h: the entry point's arguments and the
// job_run that maps the block to its env and calls the env_* function).  Keyed like k_step, arithmetic x integrator x contact capacity;
// a job that never integrates (Job::RK = false) has RK = false whatever the batch's integrator, and a null s.rk.  The job comes before
// n_envs among the kernel arguments: its fields lie where the separate arguments of a written-out wrapper would.
template <typename T, bool RK, int NC, typename Job>
__global__ void __launch_bounds__(64, 2) k_env(EnvRecordLayout L, double* rec, Job J, int n_envs) {
  Scratch<T, NC>& s = *reinterpret_cast<Scratch<T, NC>*>(myo_lds);
  s.rk = rk_storage<T, RK, NC>();
  const DevModel<T>& M = myo_cmodel<T>();
  const TaskDev& K = c_task;
  job_run(J, KernelVariant<T, RK, NC>{}, M, K, L, rec, s, (int)blockIdx.x, n_envs);
}
// render ray cast: workgroup (tile, env row) of 256 threads, one pixel each; the item table in dynamic LDS
__global__ void __launch_bounds__(MYO_RTILE * MYO_RTILE) k_render(const double* __restrict__ items, int nitem, const double* __restrict__ cams,
                                                                  int ncams, int W, int H, int flags, unsigned char* rgb, float* depth, int* seg) {
  RItem* lds = reinterpret_cast<RItem*>(myo_lds);
  const int tid = threadIdx.x, tiles_x = (W + MYO_RTILE - 1) / MYO_RTILE, e = blockIdx.y;
  const int tx0 = (int)(blockIdx.x % tiles_x) * MYO_RTILE, ty0 = (int)(blockIdx.x / tiles_x) * MYO_RTILE;
  const double* cam = cams + (size_t)(ncams == 1 ? 0 : e) * MYO_RCAM_N;
  render_stage(tid, lds, items + (size_t)e * nitem * MYO_RENDER_ITEM_N, nitem, cam, flags);
  __syncthreads();
  render_cull(tid, lds, nitem, cam, W, H, tx0, ty0);
  __syncthreads();
  render_pixel(lds, nitem, cam, W, H, tx0 + tid % MYO_RTILE, ty0 + tid / MYO_RTILE, flags, (size_t)e, rgb, depth, seg);
}
// layered ray cast (RLayers, csrc/myo_render.h): the tables take turns in LDS and are traced into the same per-pixel hit, which is then
// shaded from the hit items' global rows.  Serves every call that draws tendons or contacts; k_render stays the plain call's kernel
// (48 VGPRs against 80: folding it in here would cost every plain render occupancy).
__global__ void __launch_bounds__(MYO_RTILE * MYO_RTILE) k_render_layers(RLayers Y, const double* __restrict__ cams, int ncams, int W, int H, int flags,
                                                                         unsigned char* rgb, float* depth, int* seg) {
  RItem* lds = reinterpret_cast<RItem*>(myo_lds);
  const int tid = threadIdx.x, tiles_x = (W + MYO_RTILE - 1) / MYO_RTILE, e = blockIdx.y;
  const int tx0 = (int)(blockIdx.x % tiles_x) * MYO_RTILE, ty0 = (int)(blockIdx.x / tiles_x) * MYO_RTILE;
  const int px = tx0 + tid % MYO_RTILE, py = ty0 + tid / MYO_RTILE;
  const double* cam = cams + (size_t)(ncams == 1 ? 0 : e) * MYO_RCAM_N;
  const bool inside = px < W && py < H;
  float d[3];
  RHit h;
  render_ray(cam, W, H, px, py, d, h);
  for (int j = 0, base = 0; j < Y.nl; base += Y.l[j++].n) {
    const int n = Y.l[j].n;
    // (the camera through a pointer the compiler takes as new in every turn: hoisted out of the loop, the cull's fp32 camera and tile
    //  terms — fp64 -> fp32 conversions are vector instructions — stay in VGPRs across all three phases, 94 VGPRs and 5 waves / SIMD;
    //  rebuilt per layer, as the three written-out blocks did, 66 and 7)
    const double* camj = cam;
    asm volatile("" : "+s"(camj));
    render_stage(tid, lds, Y.l[j].rows + (size_t)e * n * MYO_RENDER_ITEM_N, n, camj, flags, j == 0 ? Y.ngeom : 0, Y.geom_alpha);
    __syncthreads();
    render_cull(tid, lds, n, camj, W, H, tx0, ty0);
    __syncthreads();
    if (inside) render_trace(lds, n, base, d, h);
    __syncthreads();
  }
  render_layers_finish(Y, cam, W, H, px, py, flags, (size_t)e, h, d, rgb, depth, seg);
}
// ... and the order that follows from the census: positions sorted by count, most engaged first (ties keep their order), written back
// into the batch's own tables — gw_elem[k] = path element of position k, wr_i[8 w + 6] = position of element w — and the counts
// cleared.  One wave; ngw <= 128 (two positions per lane).  Each wrap's arithmetic is its own: the order changes no result bit.
__global__ void __launch_bounds__(64) k_wrap_reorder(int ngw, int* cnt, int* gw_elem, int* wr_i) {
  __shared__ int c[128], e[128];
  const int lane = threadIdx.x;
  for (int k = lane; k < 128; k += 64) { c[k] = k < ngw ? cnt[k] : -1; e[k] = k < ngw ? gw_elem[k] : 0; }
  __syncthreads();
  for (int k = lane; k < ngw; k += 64) {
    int rank = 0;
    for (int j = 0; j < ngw; ++j) rank += (c[j] > c[k]) || (c[j] == c[k] && j < k);
    gw_elem[rank] = e[k];
    wr_i[8 * e[k] + 6] = rank;
    cnt[k] = 0;
  }
}
// state gather/scatter: one thread per scalar
__global__ void k_state(double* rec, int stride, int off, int cnt, int n, double* ext, int to_ext) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * cnt) return;
  const int e = (int)(i / cnt), k = (int)(i % cnt);
  if (to_ext) ext[i] = rec[(size_t)e * stride + off + k]; else rec[(size_t)e * stride + off + k] = ext[i];
}
__global__ void k_state_i(double* rec, int stride, int off, int cnt, int n, int* ext, int to_ext) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * cnt) return;
  const int e = (int)(i / cnt), k = (int)(i % cnt);
  if (to_ext) ext[i] = (int)rec[(size_t)e * stride + off + k]; else rec[(size_t)e * stride + off + k] = (double)ext[i];
}
#define LAUNCH_CHECK(b) { if (int _rc = be_launch_status()) return _rc; }      /* (the PPO-side entry points below) */
static void timing_begin(myo_batch* b, hipStream_t st) {
  if (!b->timing) return;
  hipEvent_t a, c;
  (void)hipEventCreate(&a); (void)hipEventCreate(&c);
  (void)hipEventRecord(a, st);
  b->pending.push_back({a, c});
}
static void timing_end(myo_batch* b, hipStream_t st) {
  if (!b->timing) return;
  (void)hipEventRecord(b->pending.back().second, st);
}

static unsigned lds_dyn(const myo_batch* b) {
#ifdef MYO_LDS_PAD_EXPERIMENT
  static int pad = -1;
  if (pad < 0) { const char* e = getenv("MYO_LDS_PAD"); pad = e ? atoi(e) : 0; }
  if (b->dtype != MYO_F64) return (unsigned)(MYO_LDS_ALIGN(sizeof(Scratch<float>)) + pad);
#endif
  return (unsigned)MYO_LDS_ALIGN(myo_batch_lds_bytes(b));
}
#define BIND_OR_RETURN(b, st) DeviceGuard _guard((b)->device); { int _rc = bind_constants(b, st); if (_rc) return _rc; }

// ---- the backend functions myo_host.h declares (myo_batch_create / _destroy call them)
static int be_batch_workspaces(myo_batch* b, int n_envs, int device) {
  (void)n_envs;
  int rc = 0;
    if (!slot_workspace_acquire(device, &b->K.ctrl_ws, &b->K.slot_map)) rc |= (int)hipErrorOutOfMemory; else b->has_slot_ws = true;
    if (!rc && b->ncap > MYO_NCON_MAX) {           // the 48-slot scratch keeps its contact records and wrap results in global memory (Scratch::SPILL)
      b->K.big_ws = big_workspace_acquire(device);
      if (!b->K.big_ws) rc |= (int)hipErrorOutOfMemory; else b->has_big_ws = true;
    }
  return rc;
}
static int be_batch_launch_state(myo_batch* b, const myo_model* m, int n_envs, int rc) {
  if (!rc) { rc |= (int)hipEventCreate(&b->ev0); rc |= (int)hipEventCreate(&b->ev1); }
  {
    // launch order of the env steps (k_step_order): opt-in, MYO_STEP_ORDER=1 — worth 3 % on whole-step launches, nothing once the
    // steps run in parts (2.239 vs 2.234 ms), where its 1024-thread sort per step costs what it gains
    const char* e = getenv("MYO_STEP_ORDER");
    if (!rc && b->K.kind && e && e[0] == '1') {
      std::vector<int> ident(n_envs);
      for (int i = 0; i < n_envs; ++i) ident[i] = i;
      int* po = dev_upload(b->allocs, rc, ident);
      float* pc = dev_alloc<float>(b->allocs, rc, n_envs);
      unsigned* pt = dev_alloc<unsigned>(b->allocs, rc, n_envs);
      if (!rc) { rc |= (int)hipMemset(pc, 0, sizeof(float) * (size_t)n_envs); rc |= (int)hipMemset(pt, 0, sizeof(unsigned) * (size_t)n_envs); }
      if (!rc) { b->order = po; b->cost = pc; b->ticks = pt; }
    }
    if (!rc && b->plan.nparts >= 2) {
      const int zero[4] = {0, 0, 0, 0};
      int* ps = dev_alloc<int>(b->allocs, rc, n_envs);
      int* pg = dev_upload(b->allocs, rc, zero, 4);
      if (!rc) rc |= (int)hipMemset(ps, 0, sizeof(int) * (size_t)n_envs);
      if (!rc) { b->part_state = ps; b->step_gen = pg; } else b->plan.nparts = 1;
    }
    if (!rc && m->ngw > 64 && !getenv("MYO_NO_WRAP_ORDER")) {        // (more than one pass of the wrap solver: worth ordering, see env_wrap_census)
      int wrc = 0;                                                   // (a batch without the census still steps: not an error of the create)
      int* pw = dev_alloc<int>(b->allocs, wrc, m->ngw);
      if (!wrc && hipMemset(pw, 0, sizeof(int) * (size_t)m->ngw) == hipSuccess) b->wrap_cnt = pw;
    }
  }
  return rc;
}
static void be_batch_release(myo_batch* b, int device, int destroying) {
  if (!destroying) {      // a failed myo_batch_create: only the shared workspaces were taken
    if (b->has_slot_ws) slot_workspace_release(device);
    if (b->has_big_ws) big_workspace_release(device);
    return;
  }
  unbind(b, b->device);
  DeviceGuard guard(b->device);
  for (auto& pr : b->pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  (void)hipEventDestroy(b->ev0); (void)hipEventDestroy(b->ev1);
  if (b->has_slot_ws) { (void)hipDeviceSynchronize(); slot_workspace_release(b->device); }
  if (b->has_big_ws) big_workspace_release(b->device);
}

static void be_xfer(myo_batch* b, int off, int cnt, double* ext, int to_ext, void* stream) {
  if (!ext) return;
  DeviceGuard guard(b->device);
  const long long tot = (long long)b->n * cnt;
  hipLaunchKernelGGL(k_state, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, b->rec, b->L.stride, off, cnt, b->n, ext, to_ext);
}
static void be_xfer_i(myo_batch* b, int off, int cnt, int* ext, int to_ext, void* stream) {
  if (!ext) return;
  DeviceGuard guard(b->device);
  const long long tot = (long long)b->n * cnt;
  hipLaunchKernelGGL(k_state_i, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, b->rec, b->L.stride, off, cnt, b->n, ext, to_ext);
}
static int be_capturing(void* stream) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing((hipStream_t)stream, &cap);
  return cap != hipStreamCaptureStatusNone;
}
static int be_launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MYO_OK : fail(MYO_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
}
static void be_task_changed(myo_batch* b) {
  (void)hipStreamSynchronize((hipStream_t)0);
  unbind(b, b->device);              // the task block in __constant__ memory is re-uploaded at the next launch
}

static int be_bind(myo_batch* b, void* stream) {
  DeviceGuard guard(b->device);
  return bind_constants(b, (hipStream_t)stream);
}
// k_env over a job (the device is current and the constants are bound)
template <typename Job>
static void env_launch(myo_batch* b, const Job& J, int nblocks, hipStream_t st) {
  with_variant(b, [&](auto v) {
    using V = decltype(v);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_env<typename V::T, V::RK && Job::RK, V::NC, Job>), dim3(nblocks), dim3(64), lds_dyn(b), st, b->L, b->rec, J, b->n);
  });
}
template <typename Job>
static int be_run(myo_batch* b, const Job& J, int nblocks, void* stream, int timed) {
  hipStream_t st = (hipStream_t)stream;
  BIND_OR_RETURN(b, st)
  if (timed) timing_begin(b, st);
  env_launch(b, J, nblocks, st);
  if (timed) timing_end(b, st);
  return be_launch_status();
}
static void wrap_order_launch(myo_batch* b, hipStream_t st) {
  if (!b->wrap_cnt) return;
  int* gw = const_cast<int*>(b->dtype == MYO_F64 ? b->Md.gw_elem.p : b->Mf.gw_elem.p);
  int* wr = const_cast<int*>(b->dtype == MYO_F64 ? b->Md.wr_i.p : b->Mf.wr_i.p);
  const int ngw = b->dtype == MYO_F64 ? b->Md.ngw : b->Mf.ngw;
  env_launch(b, CensusJob{b->wrap_cnt}, b->n, st);
  hipLaunchKernelGGL(k_wrap_reorder, dim3(1), dim3(64), 0, st, ngw, b->wrap_cnt, gw, wr);
}
static int be_wrap_order(myo_batch* b, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  BIND_OR_RETURN(b, st)
  wrap_order_launch(b, st);
  return be_launch_status();
}

static int be_step(myo_batch* b, const float* act, float* obs, float* rew, uint8_t* done, uint8_t* trunc, float* term_obs, float* comps,
                   float* ep_info, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  BIND_OR_RETURN(b, st)
  timing_begin(b, st);
  with_variant(b, [&](auto v) {
    using V = decltype(v);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_step<typename V::T, V::RK, V::NC>), dim3(b->plan.nparts * b->n), dim3(64), lds_dyn(b), st, b->L, b->rec, act, obs, rew, done, trunc, term_obs, comps, ep_info, b->bad_state, b->order, b->ticks, b->part_state, b->step_gen, b->plan);
  });
  timing_end(b, st);
  if (int rc = be_launch_status()) return rc;      // the generation below only advances behind a k_step that was launched
  if (b->wrap_cnt && --b->wrap_tune_in <= 0) {       // the wrap order follows the states the envs are in (env_wrap_census)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    if (cap == hipStreamCaptureStatusNone) { wrap_order_launch(b, st); b->wrap_tune_in = 256; }      // (never baked into a captured graph of steps)
    else b->wrap_tune_in = 1;
  }
  if (b->order || b->step_gen) hipLaunchKernelGGL(k_step_order, dim3(1), dim3(b->order ? 1024 : 64), 0, st, (const unsigned int*)b->ticks, b->cost, b->n, b->order, b->step_gen);
  return be_launch_status();
}

static int be_set_step_generation(myo_batch* b, unsigned int gen) {
  DeviceGuard guard(b->device);
  std::vector<int> st((size_t)b->n, (int)(16u * gen));
  const int g4[4] = {(int)gen, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess || be_h2d(b->part_state, st.data(), sizeof(int) * st.size()) || be_h2d(b->step_gen, g4, sizeof g4))
    return fail(MYO_E_DEVICE, "myo_batch_set_step_generation: copy failed");
  return MYO_OK;
}
static int be_health(myo_batch* b, int out[4]) {
  DeviceGuard guard(b->device);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, b->K.health, 4 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(MYO_E_DEVICE, "myo_batch_health: copy failed");
  return MYO_OK;
}

// the probe of myo_debug_wave_slots (csrc/myo_host.h)
__global__ void __launch_bounds__(64, 2) k_wave_slot_probe(int* occ, int* seen, int* out) {
  if (threadIdx.x != 0) return;
  const unsigned slot = myo_wave_slot(0);
  if (atomicAdd(occ + slot, 1) != 0) atomicAdd(out, 1);
  if (atomicExch(seen + slot, 1) == 0) atomicAdd(out + 1, 1);
  atomicMax(out + 2, (int)slot);
  atomicOr(out + 3, 1 << (slot >> 14));
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < 2000ull) __builtin_amdgcn_s_sleep(8);
  atomicSub(occ + slot, 1);
}
static int be_wave_slots(int device, int n_workgroups, int lds_bytes, int32_t out[4]) {
  DeviceGuard guard(device);
  int *occ = nullptr, *seen = nullptr, *o = nullptr;
  const size_t nb = sizeof(int) * (size_t)MYO_WAVE_SLOTS;
  int rc = (int)hipMalloc((void**)&occ, nb) | (int)hipMalloc((void**)&seen, nb) | (int)hipMalloc((void**)&o, 4 * sizeof(int));
  if (!rc) rc = (int)hipMemset(occ, 0, nb) | (int)hipMemset(seen, 0, nb) | (int)hipMemset(o, 0, 4 * sizeof(int));
  if (!rc) {
    if (lds_bytes > 0) (void)hipFuncSetAttribute((const void*)k_wave_slot_probe, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    hipLaunchKernelGGL(k_wave_slot_probe, dim3(n_workgroups), dim3(64), (unsigned)lds_bytes, 0, occ, seen, o);
    rc = (int)hipGetLastError() | (int)hipDeviceSynchronize();
  }
  if (!rc) rc = (int)hipMemcpy(out, o, 4 * sizeof(int), hipMemcpyDeviceToHost);
  (void)hipFree(occ); (void)hipFree(seen); (void)hipFree(o);
  if (rc) return fail(MYO_E_DEVICE, "myo_debug_wave_slots: %s", hipGetErrorString((hipError_t)rc));
  return MYO_OK;
}

__global__ void k_copy_envs(double* dst, const int* __restrict__ dst_idx, int n_dst, const double* src, const int* __restrict__ src_idx, int n_src, int stride) {
  const int d = dst_idx[blockIdx.x], s = src_idx[blockIdx.x];
  if (d < 0 || d >= n_dst || s < 0 || s >= n_src) return;
  for (int i = threadIdx.x; i < stride; i += blockDim.x) dst[(size_t)d * stride + i] = src[(size_t)s * stride + i];
}
static int be_copy_envs(myo_batch* dst, const int* dst_idx, const myo_batch* src, const int* src_idx, int k, void* stream) {
  DeviceGuard guard(dst->device);
  hipLaunchKernelGGL(k_copy_envs, dim3(k), dim3(64), 0, (hipStream_t)stream, dst->rec, dst_idx, dst->n, src->rec, src_idx, src->n, dst->L.stride);
  return be_launch_status();
}

static int be_camera_upload(myo_batch* b, double* dst, std::vector<double>& cam_tab, void* stream) {
  b->cam_host.swap(cam_tab);      // (kept until the next call: the asynchronous copy reads it)
  const hipError_t e = hipMemcpyAsync(dst, b->cam_host.data(), b->cam_host.size() * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream);
  return e == hipSuccess ? MYO_OK : fail(MYO_E_DEVICE, "myo_batch_render: camera upload failed: %s", hipGetErrorString(e));
}
static int be_cast(myo_batch* b, const RenderPlan& p, int k, int ncams, int width, int height, int flags, uint8_t* rgb, float* depth,
                   int32_t* segid, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const double* ws = b->render_ws;
  const dim3 grid((unsigned)(((width + MYO_RTILE - 1) / MYO_RTILE) * ((height + MYO_RTILE - 1) / MYO_RTILE)), (unsigned)k);
  const unsigned lds = (unsigned)(p.nmax * sizeof(RItem));
  if (p.layered) {
    hipLaunchKernelGGL(k_render_layers, grid, dim3(MYO_RTILE * MYO_RTILE), lds, st, render_layers(b, p, ws), ws + p.cams, ncams, width, height, flags, rgb, depth, segid);
  } else {
    hipLaunchKernelGGL(k_render, grid, dim3(MYO_RTILE * MYO_RTILE), lds, st, ws, b->nitem, ws + p.cams, ncams, width, height, flags, rgb, depth, segid);
  }
  return be_launch_status();
}

static double be_kernel_ms(myo_batch* b) {
  double sum = 0;
  int cnt = 0;
  for (auto& pr : b->pending) {
    (void)hipEventSynchronize(pr.second);
    float ms = 0;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { sum += ms; cnt++; }
    (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
  }
  b->pending.clear();
  return cnt ? sum / cnt : -1.0;
}


// ------------------------------------------------------------------------------------------ PPO loss
// Elementwise part of one PPO minibatch step (SB3 PPO.train semantics) in one launch:
// Gaussian log-prob, ratio, clipped surrogate, value loss and their gradients.  A block owns 64
// consecutive rows: the [64,A] tiles of mean / actions are staged through LDS with coalesced loads
// (row stride A is odd for the hand, A = 39, so the per-row reads are conflict-free), dmean leaves
// the same way.  acc[2A+3] = {d loss/d log_std[A] (without the entropy term), pl, vl,
// sum_i dmean[i,:] (bias grad of the action head), sum_i dvalue[i] (bias grad of the value head)}.
__device__ __forceinline__ unsigned short myo_f2bf(float x) {   // round-to-nearest-even, as torch's .to(bfloat16)
  unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
#include "myo_act.h"          // myo_act_tanh: the one tanh statement of the MLP paths
template <bool IN_BF16>
__global__ void __launch_bounds__(64) k_ppo_loss(const float* __restrict__ mean, const float* __restrict__ values,
                                                 const float* __restrict__ actions, const float* __restrict__ old_logp,
                                                 const float* __restrict__ adv, const float* __restrict__ returns,
                                                 const float* __restrict__ log_std, const float* __restrict__ adv_stats,
                                                 int B, int A, float clip, float vf_coef, float* __restrict__ dmean,
                                                 float* __restrict__ dvalue, float* __restrict__ acc,
                                                 unsigned short* __restrict__ dmean_h, unsigned short* __restrict__ dvalue_h,
                                                 float* __restrict__ part, const float* __restrict__ hp) {
  __shared__ float t_mean[64 * 64], t_act[64 * 64], s_ls[64], s_inv[64];
  if (hp) clip = hp[MYO_HP_CLIP];          // the device-resident hyper-parameters (include/myobatch.h) override the launch scalar
  const int lane = threadIdx.x, r0 = blockIdx.x * 64;
  const int rows = (B - r0) < 64 ? (B - r0) : 64;
  const int n = rows * A;
  const size_t base = (size_t)r0 * A;
  const unsigned short* mean_h = reinterpret_cast<const unsigned short*>(mean);
  for (int k = lane; k < n; k += 64) {
    t_mean[k] = IN_BF16 ? __uint_as_float(((unsigned)mean_h[base + k]) << 16) : mean[base + k];
    t_act[k] = actions[base + k];
  }
  if (lane < A) { const float ls = log_std[lane]; s_ls[lane] = ls; s_inv[lane] = __expf(-ls); }
  __syncthreads();
  const int i = r0 + lane;
  const bool on = lane < rows;
  float pl_i = 0.f, vl_i = 0.f, dlogp = 0.f, dv_i = 0.f, kl_i = 0.f, cf_i = 0.f, el_i = 0.f;
  if (on) {
    float logp = 0.f, ent = 0.f;
    for (int a = 0; a < A; ++a) {
      const float z = (t_act[lane * A + a] - t_mean[lane * A + a]) * s_inv[a];
      logp += -0.5f * z * z - s_ls[a] - 0.9189385332046727f;
      ent += s_ls[a] + 1.4189385332046727f;
    }
    const float an = (adv[i] - adv_stats[0]) / (adv_stats[1] + 1e-8f);
    const float lr_i = logp - old_logp[i];
    const float ratio = __expf(lr_i);
    kl_i = ((ratio - 1.f) - lr_i) / B;                            // SB3's approx_kl, clip_fraction and entropy_loss terms of this row
    cf_i = (fabsf(ratio - 1.f) > clip ? 1.f : 0.f) / B;
    el_i = -ent / B;
    const float s1 = an * ratio;
    const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
    const float s2 = an * rc;
    pl_i = -fminf(s1, s2) / B;
    const bool inside = (ratio > 1.f - clip) && (ratio < 1.f + clip);
    dlogp = -(an * ratio) * ((s1 <= s2) ? 1.f : (inside ? 1.f : 0.f)) / B;
    const float val = IN_BF16 ? __uint_as_float(((unsigned)reinterpret_cast<const unsigned short*>(values)[i]) << 16) : values[i];
    const float dv = val - returns[i];
    vl_i = dv * dv / B;
    dv_i = vf_coef * 2.f / B * dv;
    dvalue[i] = dv_i;
    if (dvalue_h) dvalue_h[i] = myo_f2bf(dv_i);
  }
  // per-row gradient tiles: dmean into t_mean, dlogp (z^2-1) into t_act (own row only: no hazard)
  if (on) {
    for (int a = 0; a < A; ++a) {
      const float inv = s_inv[a];
      const float z = (t_act[lane * A + a] - t_mean[lane * A + a]) * inv;
      t_mean[lane * A + a] = dlogp * z * inv;
      t_act[lane * A + a] = dlogp * (z * z - 1.f);
    }
  }
  __syncthreads();
  float my_ls = 0.f, my_db = 0.f;     // lane a: column sums of action dim a over the block's rows
  if (lane < A)
    for (int r = 0; r < rows; ++r) { my_ls += t_act[r * A + lane]; my_db += t_mean[r * A + lane]; }
  for (int k = lane; k < n; k += 64) {
    const float v = t_mean[k];
    dmean[base + k] = v;
    if (dmean_h) dmean_h[base + k] = myo_f2bf(v);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    pl_i += __shfl_xor(pl_i, off, 64); vl_i += __shfl_xor(vl_i, off, 64); dv_i += __shfl_xor(dv_i, off, 64);
  }
  // per-block partial sums (column-major: part[c, block]); k_colmajor_finish adds them up
  // in a fixed order (deterministic, no float atomics)
  const int W = 2 * A + 3, NB = gridDim.x;
  if (lane < A) { part[(size_t)lane * NB + blockIdx.x] = my_ls; part[(size_t)(A + 2 + lane) * NB + blockIdx.x] = my_db; }
  if (lane == 0) {
    part[(size_t)A * NB + blockIdx.x] = pl_i; part[(size_t)(A + 1) * NB + blockIdx.x] = vl_i;
    part[(size_t)(2 * A + 2) * NB + blockIdx.x] = dv_i;
  }
  if (hp) {                // three more columns: what the diagnostics and the KL stop of the hyper-parameter block are made of
    for (int off = 32; off >= 1; off >>= 1) {
      kl_i += __shfl_xor(kl_i, off, 64); cf_i += __shfl_xor(cf_i, off, 64); el_i += __shfl_xor(el_i, off, 64);
    }
    if (lane == 0) {
      part[(size_t)W * NB + blockIdx.x] = kl_i; part[(size_t)(W + 1) * NB + blockIdx.x] = cf_i;
      part[(size_t)(W + 2) * NB + blockIdx.x] = el_i;
    }
  }
}
// One finished minibatch loss entered into the hyper-parameter block (layout: include/myobatch.h) by ONE thread of the kernel that
// finishes the loss sums.  Returns true when the optimizer step that follows must not be applied: the stop flag was already up
// (sticky: nothing is recorded, the flag and the diagnostics of the minibatch that raised it stay), or this minibatch's
// approx_kl exceeds the limit (its diagnostics are recorded, as SB3 appends them before it breaks).
// (in two halves: the six words it reads, requested together — a kernel may ask for them long before its sums are ready, the
// recording thread being the block's only reader and writer in the launch — and the update from them)
struct MyoHpWords { int stop, count; float sum_kl, sum_cf, sum_el, lim; };
__device__ __forceinline__ MyoHpWords myo_hp_load(const float* hp) {
  const int* hi = reinterpret_cast<const int*>(hp);
  MyoHpWords w;
  w.stop = hi[MYO_HP_STOP]; w.count = hi[MYO_HP_COUNT];
  w.sum_kl = hp[MYO_HP_SUM_KL]; w.sum_cf = hp[MYO_HP_SUM_CLIPFRAC]; w.sum_el = hp[MYO_HP_SUM_ENTLOSS]; w.lim = hp[MYO_HP_KL_LIMIT];
  return w;
}
__device__ __forceinline__ bool myo_hp_apply(float* hp, const MyoHpWords& w, float pl, float vl, float kl, float cf, float el) {
  int* hi = reinterpret_cast<int*>(hp);
  if (w.stop) return true;
  hp[MYO_HP_SUM_KL] = w.sum_kl + kl; hp[MYO_HP_SUM_CLIPFRAC] = w.sum_cf + cf; hp[MYO_HP_SUM_ENTLOSS] = w.sum_el + el;
  hi[MYO_HP_COUNT] = w.count + 1;
  hp[MYO_HP_LAST_KL] = kl; hp[MYO_HP_LAST_PL] = pl; hp[MYO_HP_LAST_VL] = vl;
  if (w.lim > 0.f && kl > w.lim) { hi[MYO_HP_STOP] = 1; return true; }
  return false;
}
__device__ __forceinline__ bool myo_hp_record(float* hp, float pl, float vl, float kl, float cf, float el) {
  return myo_hp_apply(hp, myo_hp_load(hp), pl, vl, kl, cf, el);
}
// sum over blocks of column c of the loss partials, by one wave: the order k_colmajor_finish adds them in
__device__ __forceinline__ float myo_col_sum(const float* __restrict__ part, int c, int NB, int lane) {
  float a = 0.f;
  for (int b = lane; b < NB; b += 64) a += part[(size_t)c * NB + b];
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
  return a;
}
// acc[c] = sum over blocks of part[c, block] (fixed order: deterministic); one wave per column.
// A separate launch instead of a last-block epilogue: an in-kernel release fence writes back the
// whole L2 of the XCD on this chip (measured: +90 us), a kernel boundary is cheaper.
__global__ void __launch_bounds__(64) k_colmajor_finish(const float* __restrict__ part, float* __restrict__ acc, int NB, int A,
                                                        float ent_coef, float* __restrict__ g_log_std,
                                                        float* __restrict__ g_bias_pi, float* __restrict__ g_bias_vf,
                                                        float* __restrict__ hp) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c == 2 * A + 3) {       // (launched with a hyper-parameter block only) diagnostics and the KL stop
    const float pl = myo_col_sum(part, A, NB, lane), vl = myo_col_sum(part, A + 1, NB, lane);
    const float kl = myo_col_sum(part, c, NB, lane), cf = myo_col_sum(part, c + 1, NB, lane), el = myo_col_sum(part, c + 2, NB, lane);
    if (lane == 0) (void)myo_hp_record(hp, pl, vl, kl, cf, el);
    return;
  }
  float a = 0.f;
  for (int b = lane; b < NB; b += 64) a += part[(size_t)c * NB + b];
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
  if (lane == 0) {
    acc[c] = a;
    if (g_log_std && c < A) g_log_std[c] = a - ent_coef;          // d(-ent_coef * entropy)/d log_std = -ent_coef
    if (g_bias_pi && c >= A + 2 && c < 2 * A + 2) g_bias_pi[c - A - 2] = a;
    if (g_bias_vf && c == 2 * A + 2) g_bias_vf[0] = a;
  }
}
extern "C" int myo_ppo_loss_grad(const float* mean, const float* values, const float* actions, const float* old_logp,
                                 const float* adv, const float* returns, const float* log_std, const float* adv_stats,
                                 int B, int A, float clip, float vf_coef, float* dmean, float* dvalue, float* acc,
                                 uint16_t* dmean_bf16, uint16_t* dvalue_bf16, float* work, int in_bf16, float ent_coef,
                                 float* g_log_std, float* g_bias_pi, float* g_bias_vf, float* hp, void* stream) {
  if (!mean || !values || !actions || !old_logp || !adv || !returns || !log_std || !adv_stats || !dmean || !dvalue || !acc ||
      !work || B <= 0 || A <= 0 || A > 64)
    return fail(MYO_E_ARG, "myo_ppo_loss_grad: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (B + 63) / 64;
  if (in_bf16)
    hipLaunchKernelGGL(k_ppo_loss<true>, dim3(nblk), dim3(64), 0, st, mean, values, actions, old_logp, adv, returns,
                       log_std, adv_stats, B, A, clip, vf_coef, dmean, dvalue, acc, dmean_bf16, dvalue_bf16, work, (const float*)hp);
  else
    hipLaunchKernelGGL(k_ppo_loss<false>, dim3(nblk), dim3(64), 0, st, mean, values, actions, old_logp, adv, returns,
                       log_std, adv_stats, B, A, clip, vf_coef, dmean, dvalue, acc, dmean_bf16, dvalue_bf16, work, (const float*)hp);
  hipLaunchKernelGGL(k_colmajor_finish, dim3(2 * A + 3 + (hp ? 1 : 0)), dim3(64), 0, st, work, acc, nblk, A, ent_coef, g_log_std, g_bias_pi,
                     g_bias_vf, hp);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

// the same stage for state-dependent exploration (csrc/myo_sde_loss.h)
#include "myo_sde_loss.h"
extern "C" int myo_ppo_sde_loss_supported(int L, int A) { return (L >= 1 && L <= SDE_LMAX && A >= 1 && A <= SDE_AMAX) ? 1 : 0; }
extern "C" long long myo_ppo_sde_loss_work_floats(int B, int L, int A) {
  if (B < 1 || L < 1 || A < 1) return 0;
  return (long long)sde_blocks(B) * ((long long)L * A + SDE_COLS(A));
}
extern "C" int myo_ppo_sde_loss_grad(const uint16_t* mean_bf16, const uint16_t* value_bf16, const uint16_t* latent_bf16,
                                     const float* actions, const float* old_logp, const float* adv, const float* returns,
                                     const float* log_std, const float* adv_stats, int B, int L, int A, float clip, float vf_coef,
                                     float ent_coef, float sde_eps, uint16_t* dmean_bf16, uint16_t* dvalue_bf16, float* g_log_std,
                                     float* g_bias_pi, float* g_bias_vf, float* acc, float* work, float* hp, void* stream) {
  if (!mean_bf16 || !value_bf16 || !latent_bf16 || !actions || !old_logp || !adv || !returns || !log_std || !adv_stats || !dmean_bf16 ||
      !dvalue_bf16 || !g_log_std || !g_bias_pi || !g_bias_vf || !acc || !work)
    return fail(MYO_E_ARG, "myo_ppo_sde_loss_grad: null argument");
  if (B < 1 || B > (1 << 24) || L < 1 || A < 1)
    return fail(MYO_E_ARG, "myo_ppo_sde_loss_grad: size out of range (B %d, L %d, A %d)", B, L, A);
  if (!myo_ppo_sde_loss_supported(L, A))
    return fail(MYO_E_UNSUPPORTED, "myo_ppo_sde_loss_grad: needs latent <= %d, act <= %d (got %d, %d)", SDE_LMAX, SDE_AMAX, L, A);
  const int NB = sde_blocks(B);
  SdeArgs a;
  a.mean = mean_bf16; a.value = value_bf16; a.lat = latent_bf16; a.actions = actions; a.old_logp = old_logp; a.adv = adv;
  a.returns = returns; a.log_std = log_std; a.adv_stats = adv_stats; a.hp = hp; a.dmean = dmean_bf16; a.dvalue = dvalue_bf16;
  a.gpart = work; a.part = work + (size_t)NB * L * A;
  a.B = B; a.L = L; a.A = A; a.LS = sde_lat_stride(L); a.tpb = sde_tiles_per_block(B);
  a.clip = clip; a.vf_coef = vf_coef; a.ent_coef = ent_coef; a.eps = sde_eps;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (A <= 16) rc = sde_launch<4>(a, NB, st);
  else if (A <= 32) rc = sde_launch<8>(a, NB, st);
  else if (A <= 48) rc = sde_launch<12>(a, NB, st);
  else rc = sde_launch<16>(a, NB, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sde_finish, dim3((L * A + 255) / 256 + 1), dim3(256), 0, st, (const float*)a.gpart, (const float*)a.part, log_std, NB, B, L,
                     A, g_log_std, g_bias_pi, g_bias_vf, acc, hp);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

// ------------------------------------------------------------------------------------------ split-K
// out[g, j] = sum_k part[g, k, j]: the reduction that finishes a split-K weight-gradient bmm
// (bf16 partial products, fp32 sum).  torch's generic reduce over a middle dimension takes 37 us on
// a [2,32,256,256] tensor; this is one coalesced pass.
template <bool BF16>
__global__ void __launch_bounds__(256) k_splitk_reduce(const unsigned* __restrict__ part, float2* __restrict__ out, int splits,
                                                       int n2, int total2) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;   // index of an element pair in the output
  if (j >= total2) return;
  const int g = j / n2, c = j - g * n2;
  float a0 = 0.f, a1 = 0.f;
  if (BF16) {
    const unsigned* src = part + (size_t)g * splits * n2 + c;
#pragma unroll 8
    for (int k = 0; k < splits; ++k) {
      const unsigned u = src[(size_t)k * n2];
      a0 += __uint_as_float(u << 16);
      a1 += __uint_as_float(u & 0xffff0000u);
    }
  } else {
    const float2* src = reinterpret_cast<const float2*>(part) + (size_t)g * splits * n2 + c;
#pragma unroll 8
    for (int k = 0; k < splits; ++k) { const float2 v = src[(size_t)k * n2]; a0 += v.x; a1 += v.y; }
  }
  out[j] = make_float2(a0, a1);
}
// dy <- dy * act'(.) from the layer's OUTPUT act (bf16 in place) and per-block column sums of the result: partial[blk, c] over the
// block's 32 rows.  ReLU: dy * (act > 0); tanh: bf16(dy * (1 - act^2)), one rounding of the product.  cols/2 must divide 256
// (cols = 256: one column pair per thread, two row phases).  Followed by k_splitk_reduce<false> for the bias gradient.
template <int ACT>
__global__ void __launch_bounds__(256) k_act_bwd_colsum(unsigned* __restrict__ dy, const unsigned* __restrict__ act, int P,
                                                        float2* __restrict__ partial) {
  __shared__ float2 red[256];
  const int t = threadIdx.x, cp = t % P, rph = t / P, nph = 256 / P;
  const size_t row0 = (size_t)blockIdx.x * 32;
  float a0 = 0.f, a1 = 0.f;
  for (int r = rph; r < 32; r += nph) {
    const size_t i = (row0 + r) * P + cp;
    const unsigned g = dy[i], a = act[i];
    unsigned lo, hi;
    if (ACT == MYO_ACT_TANH) {
      const float h0 = __uint_as_float(a << 16), h1 = __uint_as_float(a & 0xffff0000u);
      lo = (unsigned)myo_f2bf(__uint_as_float(g << 16) * fmaf(-h0, h0, 1.f));
      hi = (unsigned)myo_f2bf(__uint_as_float(g & 0xffff0000u) * fmaf(-h1, h1, 1.f)) << 16;
    } else {
      // bf16 > 0  <=>  sign bit clear and magnitude non-zero
      lo = ((a & 0x8000u) == 0 && (a & 0x7fffu) != 0) ? (g & 0xffffu) : 0u;
      hi = ((a & 0x80000000u) == 0 && (a & 0x7fff0000u) != 0) ? (g & 0xffff0000u) : 0u;
    }
    dy[i] = lo | hi;
    a0 += __uint_as_float(lo << 16);
    a1 += __uint_as_float(hi);
  }
  red[t] = make_float2(a0, a1);
  __syncthreads();
  if (t < P) {
    float2 v = red[t];
    for (int k = 1; k < nph; ++k) { v.x += red[t + k * P].x; v.y += red[t + k * P].y; }
    partial[(size_t)blockIdx.x * P + t] = v;
  }
}
// h <- act(h + bias) in place (ReLU or tanh, one rounding), bf16 [G, R, C] with bias [G, C] (the epilogue of a batched GEMM).
template <int ACT>
__global__ void __launch_bounds__(256) k_bias_act(unsigned* __restrict__ h, const unsigned* __restrict__ bias, int P, size_t RP,
                                                  size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t g = i / RP;
  const int cp = (int)(i % P);
  const unsigned x = h[i], b = bias[g * P + cp];
  const float slo = __uint_as_float(x << 16) + __uint_as_float(b << 16), shi = __uint_as_float(x & 0xffff0000u) + __uint_as_float(b & 0xffff0000u);
  const float lo = ACT == MYO_ACT_TANH ? myo_act_tanh(slo) : fmaxf(slo, 0.f);
  const float hi = ACT == MYO_ACT_TANH ? myo_act_tanh(shi) : fmaxf(shi, 0.f);
  h[i] = (unsigned)myo_f2bf(lo) | ((unsigned)myo_f2bf(hi) << 16);
}
// Minibatch gather of one PPO optimiser step: rows idx[0..bs) of the rollout arrays -> contiguous
// minibatch arrays (obs as `copies` stacked bf16 copies: the GEMM operand of the stacked actor /
// critic trunks), plus mean and unbiased std of the gathered advantages (block-wise mean / M2, merged
// by k_moments_finish in block order: deterministic).  Replaces 5 index kernels, 3 casts/copies and
// the var_mean reduction.
#define MYO_GATHER_ROWS 16
// (the body of a gather block: output rows r0 .. r0 + rows take the rollout rows s_idx[0 .. rows), which the caller has put into LDS)
__device__ __forceinline__ void myo_gather_block(const float* __restrict__ obs, const float* __restrict__ act,
                                                 const float* __restrict__ oldlp, const float* __restrict__ adv,
                                                 const float* __restrict__ ret, const long long* s_idx, int rows, int r0, int bs,
                                                 int O, int A, unsigned short* __restrict__ obs_h, int copies,
                                                 float* __restrict__ act_mb, float* __restrict__ oldlp_mb,
                                                 float* __restrict__ adv_mb, float* __restrict__ ret_mb, float* __restrict__ part) {
  const int t = threadIdx.x;
#pragma unroll 2
  for (int e = t; e < rows * O; e += 256) {
    const int r = e / O, c = e - r * O;
    const unsigned short v = myo_f2bf(obs[(size_t)s_idx[r] * O + c]);
    for (int k = 0; k < copies; ++k) obs_h[((size_t)k * bs + r0 + r) * O + c] = v;
  }
#pragma unroll 2
  for (int e = t; e < rows * A; e += 256) {
    const int r = e / A, c = e - r * A;
    act_mb[(size_t)(r0 + r) * A + c] = act[(size_t)s_idx[r] * A + c];
  }
  if (t < 64) {
    float a = 0.f;
    if (t < rows) {
      const size_t src = (size_t)s_idx[t];
      a = adv[src];
      oldlp_mb[r0 + t] = oldlp[src]; adv_mb[r0 + t] = a; ret_mb[r0 + t] = ret[src];
    }
    float sum = a;
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const float mean = sum / rows;
    const float d = (t < rows) ? (a - mean) : 0.f;
    float m2 = d * d;
    for (int off = 32; off >= 1; off >>= 1) m2 += __shfl_xor(m2, off, 64);
    if (t == 0) { part[2 * blockIdx.x] = mean; part[2 * blockIdx.x + 1] = m2; }
  }
}
__global__ void __launch_bounds__(256) k_ppo_gather(const float* __restrict__ obs, const float* __restrict__ act,
                                                    const float* __restrict__ oldlp, const float* __restrict__ adv,
                                                    const float* __restrict__ ret, const long long* __restrict__ idx, int bs,
                                                    int O, int A, unsigned short* __restrict__ obs_h, int copies,
                                                    float* __restrict__ act_mb, float* __restrict__ oldlp_mb,
                                                    float* __restrict__ adv_mb, float* __restrict__ ret_mb,
                                                    float* __restrict__ part) {
  constexpr int R = MYO_GATHER_ROWS;
  __shared__ long long s_idx[R];
  const int t = threadIdx.x, r0 = blockIdx.x * R;
  const int rows = (bs - r0) < R ? (bs - r0) : R;
  if (t < rows) s_idx[t] = idx[r0 + t];
  __syncthreads();
  myo_gather_block(obs, act, oldlp, adv, ret, s_idx, rows, r0, bs, O, A, obs_h, copies, act_mb, oldlp_mb, adv_mb, ret_mb, part);
}
// The same gather for a minibatch of m CHUNKS of L consecutive steps (recurrent PPO with seq_len): chunk[j] = s * N + n names steps
// [s L, (s + 1) L) of env n, output row r = t m + j takes rollout row (s L + t) N + n.  The first nb blocks are gather blocks as
// above (same partition, same moments) and also leave keep = 1 - starts of their rows; the blocks behind them fetch the LSTM state
// that entered each chunk from the rollout's snapshots, times keep of the chunk's first step: 8 elements = one 16-byte load of h,
// two of c per thread.
struct GatherSeq {
  const float *obs, *act, *oldlp, *adv, *ret, *starts, *c_snap;
  const unsigned short* h_snap;
  const long long* chunk;
  int N, L, m, S, G, H, O, A, copies, nb;
  unsigned short *obs_h, *hm0, *cm0;
  float *act_mb, *oldlp_mb, *adv_mb, *ret_mb, *keep, *c0_32, *part;
};
__device__ __forceinline__ unsigned short myo_bf_mul(unsigned short x, float k) { return myo_f2bf(__uint_as_float((unsigned)x << 16) * k); }
__global__ void __launch_bounds__(256) k_ppo_gather_seq(GatherSeq a) {
  constexpr int R = MYO_GATHER_ROWS;
  __shared__ long long s_idx[R];
  const int t = threadIdx.x;
  const long long items = (long long)a.N * a.S;
  if ((int)blockIdx.x < a.nb) {                       // block-uniform branch
    const int bs = a.L * a.m, r0 = blockIdx.x * R;
    const int rows = (bs - r0) < R ? (bs - r0) : R;
    if (t < rows) {
      const int r = r0 + t, tt = r / a.m, j = r - tt * a.m;
      long long c = a.chunk[j];
      c = c < 0 ? 0 : (c >= items ? items - 1 : c);   // (a permutation of the items never leaves the range)
      const long long s = c / a.N, n = c - s * a.N;
      const long long src = (s * a.L + tt) * a.N + n;
      s_idx[t] = src;
      a.keep[r] = 1.f - a.starts[src];
    }
    __syncthreads();
    myo_gather_block(a.obs, a.act, a.oldlp, a.adv, a.ret, s_idx, rows, r0, bs, a.O, a.A, a.obs_h, a.copies, a.act_mb, a.oldlp_mb,
                     a.adv_mb, a.ret_mb, a.part);
    return;
  }
  const int H8 = a.H / 8;
  const long long v = (long long)(blockIdx.x - a.nb) * 256 + t;          // vector of 8 of the [G, m, H] outputs
  if (v >= (long long)a.G * a.m * H8) return;
  const int hv = (int)(v % H8), j = (int)((v / H8) % a.m), g = (int)(v / ((long long)H8 * a.m));
  long long c = a.chunk[j];
  c = c < 0 ? 0 : (c >= items ? items - 1 : c);
  const long long s = c / a.N, n = c - s * a.N;
  const float k0 = 1.f - a.starts[(s * a.L) * a.N + n];
  const size_t src = (((size_t)s * a.G + g) * a.N + n) * a.H + 8 * hv, dst = (size_t)v * 8;
  const uint4 h = *reinterpret_cast<const uint4*>(a.h_snap + src);
  const float4 c_lo = *reinterpret_cast<const float4*>(a.c_snap + src), c_hi = *reinterpret_cast<const float4*>(a.c_snap + src + 4);
  const unsigned hw[4] = {h.x, h.y, h.z, h.w};
  const float cw[8] = {c_lo.x * k0, c_lo.y * k0, c_lo.z * k0, c_lo.w * k0, c_hi.x * k0, c_hi.y * k0, c_hi.z * k0, c_hi.w * k0};
  unsigned ho[4], co[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ho[i] = (unsigned)myo_bf_mul((unsigned short)(hw[i] & 0xffffu), k0) | ((unsigned)myo_bf_mul((unsigned short)(hw[i] >> 16), k0) << 16);
    co[i] = (unsigned)myo_f2bf(cw[2 * i]) | ((unsigned)myo_f2bf(cw[2 * i + 1]) << 16);
  }
  *reinterpret_cast<uint4*>(a.hm0 + dst) = make_uint4(ho[0], ho[1], ho[2], ho[3]);
  *reinterpret_cast<uint4*>(a.cm0 + dst) = make_uint4(co[0], co[1], co[2], co[3]);
  *reinterpret_cast<float4*>(a.c0_32 + dst) = make_float4(cw[0], cw[1], cw[2], cw[3]);
  *reinterpret_cast<float4*>(a.c0_32 + dst + 4) = make_float4(cw[4], cw[5], cw[6], cw[7]);
}
// LSTM state entering a chunk of the rollout (recurrent PPO with seq_len), taken inside the per-step graph: the step index is read
// on the device, steps that open no chunk return at once.  A thread moves 8 elements: one 16-byte vector of h, two of c.
__global__ void __launch_bounds__(256) k_state_snapshot(const uint4* __restrict__ h, const float4* __restrict__ c32, size_t n8,
                                                        const int* __restrict__ t_idx, int seq_len, int S,
                                                        uint4* __restrict__ h_snap, float4* __restrict__ c_snap) {
  const int t = *t_idx;
  if (t < 0 || t % seq_len) return;
  const int slot = t / seq_len;
  if (slot >= S) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  h_snap[(size_t)slot * n8 + i] = h[i];
  c_snap[((size_t)slot * n8 + i) * 2] = c32[2 * i];
  c_snap[((size_t)slot * n8 + i) * 2 + 1] = c32[2 * i + 1];
}
// merges the block moments of k_ppo_gather in block order (Chan): mean and unbiased std
__global__ void __launch_bounds__(64) k_moments_finish(const float* __restrict__ part, int nb, int bs, float* __restrict__ adv_stats) {
  constexpr int R = MYO_GATHER_ROWS;
  const int t = threadIdx.x;
  float wsum = 0.f;
  for (int b = t; b < nb; b += 64) {
    const int n_b = (bs - b * R) < R ? (bs - b * R) : R;
    wsum += n_b * part[2 * b];
  }
  for (int off = 32; off >= 1; off >>= 1) wsum += __shfl_xor(wsum, off, 64);
  const float mean = wsum / bs;
  float m2 = 0.f;
  for (int b = t; b < nb; b += 64) {
    const int n_b = (bs - b * R) < R ? (bs - b * R) : R;
    const float dm = part[2 * b] - mean;
    m2 += part[2 * b + 1] + n_b * dm * dm;
  }
  for (int off = 32; off >= 1; off >>= 1) m2 += __shfl_xor(m2, off, 64);
  if (t == 0) { adv_stats[0] = mean; adv_stats[1] = sqrtf(m2 / (bs > 1 ? bs - 1 : 1)); }
}
// Tall fp32 reduction out[g, c] = sum_k part[g, k, c] for few columns and many splits (bias gradients):
// a block owns 32 column pairs, 8 split phases per pair, combined through LDS in phase order.
__global__ void __launch_bounds__(256) k_colsum_finish(const float2* __restrict__ part, float2* __restrict__ out, int splits, int n2) {
  __shared__ float2 red[256];
  const int t = threadIdx.x, cl = t & 31, ph = t >> 5;
  const int j = blockIdx.x * 32 + cl;                 // output pair index (over groups * n2)
  const int g = j / n2, c = j - g * n2;
  const float2* src = part + (size_t)g * splits * n2 + c;
  float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
  for (int k = ph; k < splits; k += 8) { const float2 v = src[(size_t)k * n2]; a0 += v.x; a1 += v.y; }
  red[t] = make_float2(a0, a1);
  __syncthreads();
  if (ph == 0) {
    float2 v = red[cl];
    for (int k = 1; k < 8; ++k) { v.x += red[cl + 32 * k].x; v.y += red[cl + 32 * k].y; }
    out[j] = v;
  }
}
// Two independent split reductions in ONE launch (the weight-gradient partials of a layer and its bias
// partials; the two head gradients): blocks [0, nbA) run job A, the rest job B, each with the code of the
// stand-alone kernels above (mode 0: bf16 partials, 1: tall fp32 through LDS, 2: fp32 partials).
struct ReduceJob { const void* part; float2* out; int splits, n2, total2, mode, nblocks; };
__device__ __forceinline__ void myo_reduce_job(const ReduceJob& J, int vb, float2* red) {
  const int t = threadIdx.x;
  if (J.mode == 1) {
    const int cl = t & 31, ph = t >> 5;
    const int j = vb * 32 + cl;
    const int g = j / J.n2, c = j - g * J.n2;
    const float2* src = reinterpret_cast<const float2*>(J.part) + (size_t)g * J.splits * J.n2 + c;
    float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
    for (int k = ph; k < J.splits; k += 8) { const float2 v = src[(size_t)k * J.n2]; a0 += v.x; a1 += v.y; }
    red[t] = make_float2(a0, a1);
    __syncthreads();
    if (ph == 0) {
      float2 v = red[cl];
      for (int k = 1; k < 8; ++k) { v.x += red[cl + 32 * k].x; v.y += red[cl + 32 * k].y; }
      J.out[j] = v;
    }
    return;
  }
  const int j = vb * 256 + t;
  if (j >= J.total2) return;
  const int g = j / J.n2, c = j - g * J.n2;
  float a0 = 0.f, a1 = 0.f;
  if (J.mode == 0) {
    const unsigned* src = reinterpret_cast<const unsigned*>(J.part) + (size_t)g * J.splits * J.n2 + c;
#pragma unroll 8
    for (int k = 0; k < J.splits; ++k) {
      const unsigned u = src[(size_t)k * J.n2];
      a0 += __uint_as_float(u << 16);
      a1 += __uint_as_float(u & 0xffff0000u);
    }
  } else {
    const float2* src = reinterpret_cast<const float2*>(J.part) + (size_t)g * J.splits * J.n2 + c;
#pragma unroll 8
    for (int k = 0; k < J.splits; ++k) { const float2 v = src[(size_t)k * J.n2]; a0 += v.x; a1 += v.y; }
  }
  J.out[j] = make_float2(a0, a1);
}
__global__ void __launch_bounds__(256) k_reduce_pair(ReduceJob A, ReduceJob B) {
  __shared__ float2 red[256];
  if ((int)blockIdx.x < A.nblocks) myo_reduce_job(A, blockIdx.x, red);      // block-uniform branch
  else myo_reduce_job(B, blockIdx.x - A.nblocks, red);
}
static bool myo_act_known(int activation) { return activation == MYO_ACT_RELU || activation == MYO_ACT_TANH; }
extern "C" int myo_bias_act_bf16(uint16_t* h, const uint16_t* bias, int groups, int rows, int cols, int activation, void* stream) {
  if (!h || !bias || groups <= 0 || rows <= 0 || cols <= 0 || (cols & 1)) return fail(MYO_E_ARG, "myo_bias_act_bf16: bad arguments");
  if (!myo_act_known(activation)) return fail(MYO_E_ARG, "myo_bias_act_bf16: unknown activation code %d", activation);
  const size_t P = cols / 2, RP = (size_t)rows * P, total = RP * groups;
  hipLaunchKernelGGL(activation == MYO_ACT_TANH ? k_bias_act<MYO_ACT_TANH> : k_bias_act<MYO_ACT_RELU>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (unsigned*)h, (const unsigned*)bias, (int)P, RP, total);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_bias_relu_bf16(uint16_t* h, const uint16_t* bias, int groups, int rows, int cols, void* stream) {
  return myo_bias_act_bf16(h, bias, groups, rows, cols, MYO_ACT_RELU, stream);
}
extern "C" int myo_ppo_gather(const float* obs, const float* act, const float* oldlp, const float* adv, const float* ret,
                              const int64_t* idx, int bs, int obs_dim, int act_dim, uint16_t* obs_bf16, int copies,
                              float* act_mb, float* oldlp_mb, float* adv_mb, float* ret_mb, float* adv_stats, float* work,
                              void* stream) {
  if (!obs || !act || !oldlp || !adv || !ret || !idx || !obs_bf16 || !act_mb || !oldlp_mb || !adv_mb || !ret_mb ||
      !work || bs <= 0 || obs_dim <= 0 || act_dim <= 0 || copies <= 0)
    return fail(MYO_E_ARG, "myo_ppo_gather: bad arguments");
  hipLaunchKernelGGL(k_ppo_gather, dim3((bs + MYO_GATHER_ROWS - 1) / MYO_GATHER_ROWS), dim3(256), 0, (hipStream_t)stream, obs, act, oldlp, adv, ret,
                     (const long long*)idx, bs, obs_dim, act_dim, obs_bf16, copies, act_mb, oldlp_mb, adv_mb, ret_mb, work);
  if (adv_stats)      // NULL: the caller supplies the advantage moments itself (cross-rank moments, or no normalisation)
    hipLaunchKernelGGL(k_moments_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, work,
                       (bs + MYO_GATHER_ROWS - 1) / MYO_GATHER_ROWS, bs, adv_stats);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_ppo_gather_seq(const float* obs, const float* act, const float* oldlp, const float* adv, const float* ret,
                                  const float* starts, const void* h_snap, const float* c_snap, const int64_t* chunk, int T, int N,
                                  int L, int m, int G, int H, int obs_dim, int act_dim, uint16_t* obs_bf16, int copies, float* act_mb,
                                  float* oldlp_mb, float* adv_mb, float* ret_mb, float* keep, uint16_t* hm0, uint16_t* cm0,
                                  float* c0_32, float* adv_stats, float* work, void* stream) {
  if (!obs || !act || !oldlp || !adv || !ret || !starts || !h_snap || !c_snap || !chunk || !obs_bf16 || !act_mb || !oldlp_mb ||
      !adv_mb || !ret_mb || !keep || !hm0 || !cm0 || !c0_32 || !work || T < 1 || N < 1 || L < 1 || m < 1 || T % L || G < 1 || H < 8 ||
      (H & 7) || obs_dim <= 0 || act_dim <= 0 || copies <= 0 || (long long)L * m > 0x7fffffffLL)
    return fail(MYO_E_ARG, "myo_ppo_gather_seq: bad arguments");
  GatherSeq a;
  a.obs = obs; a.act = act; a.oldlp = oldlp; a.adv = adv; a.ret = ret; a.starts = starts; a.c_snap = c_snap;
  a.h_snap = (const unsigned short*)h_snap; a.chunk = (const long long*)chunk;
  a.N = N; a.L = L; a.m = m; a.S = T / L; a.G = G; a.H = H; a.O = obs_dim; a.A = act_dim; a.copies = copies;
  const int bs = L * m;
  a.nb = (bs + MYO_GATHER_ROWS - 1) / MYO_GATHER_ROWS;
  a.obs_h = obs_bf16; a.hm0 = hm0; a.cm0 = cm0; a.act_mb = act_mb; a.oldlp_mb = oldlp_mb; a.adv_mb = adv_mb; a.ret_mb = ret_mb;
  a.keep = keep; a.c0_32 = c0_32; a.part = work;
  const long long vecs = (long long)G * m * (H / 8);
  hipLaunchKernelGGL(k_ppo_gather_seq, dim3((unsigned)(a.nb + (vecs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  if (adv_stats)      // NULL: the caller supplies the advantage moments itself, as for myo_ppo_gather
    hipLaunchKernelGGL(k_moments_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, work, a.nb, bs, adv_stats);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_rollout_state_snapshot(const void* h, const float* c32, int G, int N, int H, const int32_t* t_idx, int seq_len, int S,
                                          void* h_snap, float* c_snap, void* stream) {
  const long long n = (long long)G * N * H;
  if (!h || !c32 || !t_idx || !h_snap || !c_snap || G < 1 || N < 1 || H < 1 || seq_len < 1 || S < 1 || (n & 7))
    return fail(MYO_E_ARG, "myo_rollout_state_snapshot: bad arguments");
  const size_t n8 = (size_t)(n / 8);
  hipLaunchKernelGGL(k_state_snapshot, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)h,
                     (const float4*)c32, n8, t_idx, seq_len, S, (uint4*)h_snap, (float4*)c_snap);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

static ReduceJob make_reduce_job(const void* part, int part_is_bf16, float* out, int groups, int splits, int n) {
  ReduceJob J;
  J.part = part; J.out = (float2*)out; J.splits = splits; J.n2 = n / 2; J.total2 = groups * (n / 2);
  if (part_is_bf16) { J.mode = 0; J.nblocks = (J.total2 + 255) / 256; }
  else if (J.n2 % 32 == 0 && splits >= 64) { J.mode = 1; J.nblocks = J.total2 / 32; }
  else { J.mode = 2; J.nblocks = (J.total2 + 255) / 256; }
  return J;
}
extern "C" int myo_splitk_reduce2(const void* part_a, int a_is_bf16, float* out_a, int groups_a, int splits_a, int n_a,
                                  const void* part_b, int b_is_bf16, float* out_b, int groups_b, int splits_b, int n_b, void* stream) {
  if (!part_a || !out_a || groups_a <= 0 || splits_a <= 0 || n_a <= 0 || (n_a & 1) || !part_b || !out_b || groups_b <= 0 ||
      splits_b <= 0 || n_b <= 0 || (n_b & 1))
    return fail(MYO_E_ARG, "myo_splitk_reduce2: bad arguments");
  const ReduceJob A = make_reduce_job(part_a, a_is_bf16, out_a, groups_a, splits_a, n_a);
  const ReduceJob B = make_reduce_job(part_b, b_is_bf16, out_b, groups_b, splits_b, n_b);
  hipLaunchKernelGGL(k_reduce_pair, dim3(A.nblocks + B.nblocks), dim3(256), 0, (hipStream_t)stream, A, B);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_splitk_reduce(const void* part, int part_is_bf16, float* out, int groups, int splits, int n, void* stream) {
  if (!part || !out || groups <= 0 || splits <= 0 || n <= 0 || (n & 1)) return fail(MYO_E_ARG, "myo_splitk_reduce: bad arguments");
  const int total2 = groups * (n / 2);
  if (part_is_bf16)
    hipLaunchKernelGGL(k_splitk_reduce<true>, dim3((total2 + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned*)part, (float2*)out, splits, n / 2, total2);
  else if ((n / 2) % 32 == 0 && splits >= 64)
    hipLaunchKernelGGL(k_colsum_finish, dim3(total2 / 32), dim3(256), 0, (hipStream_t)stream, (const float2*)part, (float2*)out,
                       splits, n / 2);
  else
    hipLaunchKernelGGL(k_splitk_reduce<false>, dim3((total2 + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned*)part, (float2*)out, splits, n / 2, total2);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_act_bwd_colsum_bf16(uint16_t* dy, const uint16_t* act, int rows, int cols, float* partial, int activation, void* stream) {
  if (!dy || !act || !partial || rows <= 0 || cols <= 0 || (rows % 32) || (cols & 1) || (256 % (cols / 2)) || cols / 2 < 8)
    return fail(MYO_E_ARG, "myo_act_bwd_colsum_bf16: rows must be a multiple of 32 and cols/2 a divisor of 256 (>= 8)");
  if (!myo_act_known(activation)) return fail(MYO_E_ARG, "myo_act_bwd_colsum_bf16: unknown activation code %d", activation);
  hipLaunchKernelGGL(activation == MYO_ACT_TANH ? k_act_bwd_colsum<MYO_ACT_TANH> : k_act_bwd_colsum<MYO_ACT_RELU>, dim3(rows / 32), dim3(256), 0,
                     (hipStream_t)stream, (unsigned*)dy, (const unsigned*)act, cols / 2, (float2*)partial);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_relu_bwd_colsum_bf16(uint16_t* dy, const uint16_t* act, int rows, int cols, float* partial, void* stream) {
  return myo_act_bwd_colsum_bf16(dy, act, rows, cols, partial, MYO_ACT_RELU, stream);
}

// ------------------------------------------------------------------------------------------ rollout
// The per-step plumbing between two env kernels (policy input, action sampling, VecNormalize, rollout
// buffer writes) as a handful of launches instead of ~80 small framework kernels.  `t_idx` is a
// DEVICE int32 holding the rollout-buffer row of the current step, so the same launches replay from a
// hipGraph for every step.
// obs (f32 [N,O]) -> obs_buf[t] (f32) and `copies` stacked bf16 copies (GEMM operand of the trunks)
__global__ void __launch_bounds__(256) k_obs_prepare(const float* __restrict__ obs, size_t n, float* __restrict__ obs_buf,
                                                     unsigned short* __restrict__ x_h, int copies, const int* __restrict__ t_idx) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = obs[i];
  if (obs_buf) obs_buf[(size_t)(*t_idx) * n + i] = v;
  const unsigned short h = myo_f2bf(v);
  for (int k = 0; k < copies; ++k) x_h[(size_t)k * n + i] = h;
}
// DiagGaussian sampling (SB3 DiagGaussianDistribution: a = mu + exp(log_std) eps; log-prob summed over
// dims) for N rows, one wave per 64 rows x loop over action dims; Philox4x32-10 keyed by (seed, rollout
// step counter), Box-Muller.  Writes act_buf[t], val_buf[t], logp_buf[t] and the clipped actions.
// 16 lanes per env, lane g = the four actions 4g..4g+3 (one Philox block each, counter (env, g, draw)): the rows of act_buf /
// clipped are written 16 B per lane, contiguous across the 16 lanes, and log pi is a 16-lane shuffle sum.  (One lane per env
// walked the ten Philox blocks of a 39-action row serially and stored with a 156 B stride: 12 us for 4096 envs.)
#define MYO_SAMPLE_ROWS 16
__global__ void __launch_bounds__(16 * MYO_SAMPLE_ROWS) k_sample_actions(const unsigned short* __restrict__ mean_h, const unsigned short* __restrict__ value_h,
                                                       const float* __restrict__ log_std, int N, int A, unsigned long long seed,
                                                       unsigned long long* __restrict__ draw_counter, const int* __restrict__ t_idx,
                                                       float* __restrict__ act_buf, float* __restrict__ val_buf,
                                                       float* __restrict__ logp_buf, float* __restrict__ clipped, int deterministic) {
  const int i = blockIdx.x * MYO_SAMPLE_ROWS + (threadIdx.x >> 4), g0 = threadIdx.x & 15;
  const size_t t = (size_t)(*t_idx);
  const unsigned long long ctr = *draw_counter;
  float logp = 0.f;
  if (i < N) {
    for (int a0 = 4 * g0; a0 < A; a0 += 64) {
      unsigned int c[4] = {(unsigned int)i, (unsigned int)(a0 >> 2), (unsigned int)ctr, (unsigned int)(ctr >> 32)};
      unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
      for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
      float z[4];
      for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float rad = sqrtf(-2.0f * __logf(u1));
        float sn, cs;
        __sincosf(6.283185307179586f * u2, &sn, &cs);
        z[2 * h] = rad * cs; z[2 * h + 1] = rad * sn;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int a = a0 + k;
        if (a < A) {
          const float ls = log_std[a];
          const float mu = __uint_as_float(((unsigned)mean_h[(size_t)i * A + a]) << 16);
          const float act = deterministic ? mu : mu + __expf(ls) * z[k];
          const float zz = (act - mu) * __expf(-ls);
          logp += -0.5f * zz * zz - ls - 0.9189385332046727f;
          act_buf[(t * N + i) * A + a] = act;
          clipped[(size_t)i * A + a] = fminf(fmaxf(act, -1.f), 1.f);
        }
      }
    }
  }
  for (int off = 8; off >= 1; off >>= 1) logp += __shfl_xor(logp, off, 16);
  if (i < N && g0 == 0) {
    logp_buf[t * N + i] = logp;
    val_buf[t * N + i] = __uint_as_float(((unsigned)value_h[i]) << 16);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) draw_counter[1] = ctr + 1;   // committed by k_rollout_advance
}
// VecNormalize.step_wait (SB3 1.6.2), kernel 1 of 3: per-block fp64 moments of the raw
// observation columns over 128-row chunks, discounted-return update ret = ret*gamma + r and its moments.
#define MYO_VN_ROWS 128
__global__ void __launch_bounds__(128) k_vecnorm_moments(const float* __restrict__ obs, const float* __restrict__ rew, int N, int O,
                                                         double* __restrict__ returns, double gamma, int training,
                                                         double* __restrict__ part) {
  __shared__ double red[128];
  const int t = threadIdx.x, r0 = blockIdx.x * MYO_VN_ROWS;
  const int rows = (N - r0) < MYO_VN_ROWS ? (N - r0) : MYO_VN_ROWS;
  double* mine = part + (size_t)blockIdx.x * 2 * (O + 1);
  // column c of the chunk: thread pair (2c', 2c'+1) -> each half walks alternate rows with 4 independent
  // accumulators (the loads of a pass are in flight together), halves meet through a lane shuffle
  const int half = t & 1;
  for (int c = t >> 1; c < O; c += 64) {
    const float* col = obs + (size_t)r0 * O + c;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int r = half;
#pragma unroll 4
    for (; r + 6 < rows; r += 8) {
      a0 += (double)col[(size_t)r * O]; a1 += (double)col[(size_t)(r + 2) * O];
      a2 += (double)col[(size_t)(r + 4) * O]; a3 += (double)col[(size_t)(r + 6) * O];
    }
    for (; r < rows; r += 2) a0 += (double)col[(size_t)r * O];
    double sum = (a0 + a1) + (a2 + a3);
    sum += __shfl_xor(sum, 1);
    const double mean = sum / rows;
    a0 = a1 = a2 = a3 = 0;
    r = half;
#pragma unroll 4
    for (; r + 6 < rows; r += 8) {
      const double d0 = (double)col[(size_t)r * O] - mean, d1 = (double)col[(size_t)(r + 2) * O] - mean;
      const double d2 = (double)col[(size_t)(r + 4) * O] - mean, d3 = (double)col[(size_t)(r + 6) * O] - mean;
      a0 += d0 * d0; a1 += d1 * d1; a2 += d2 * d2; a3 += d3 * d3;
    }
    for (; r < rows; r += 2) { const double d = (double)col[(size_t)r * O] - mean; a0 += d * d; }
    double m2 = (a0 + a1) + (a2 + a3);
    m2 += __shfl_xor(m2, 1);
    if (!half) { mine[2 * c] = mean; mine[2 * c + 1] = m2; }
  }
  double v = 0;
  if (t < rows) {
    v = returns[r0 + t];
    if (training) { v = v * gamma + (double)rew[r0 + t]; returns[r0 + t] = v; }
  }
  red[t] = (t < rows) ? v : 0.0;
  __syncthreads();
  for (int sft = 64; sft >= 1; sft >>= 1) { if (t < sft) red[t] += red[t + sft]; __syncthreads(); }
  const double mean = red[0] / rows;
  __syncthreads();
  const double d = (t < rows) ? (v - mean) : 0.0;
  red[t] = d * d;
  __syncthreads();
  for (int sft = 64; sft >= 1; sft >>= 1) { if (t < sft) red[t] += red[t + sft]; __syncthreads(); }
  if (t == 0) { mine[2 * O] = mean; mine[2 * O + 1] = red[0]; }
}
// kernel 2 of 3 (one block): merge the block moments in block order -> batch mean / variance, then the
// running statistics by Chan's parallel update (RunningMeanStd.update_from_moments), in place.
__global__ void __launch_bounds__(128) k_vecnorm_merge(const double* __restrict__ part, int nb, int N, int O, double* __restrict__ obs_mean,
                                                       double* __restrict__ obs_var, double* __restrict__ obs_count,
                                                       double* __restrict__ ret_stats, int upd_obs, int upd_ret) {
  const int t = threadIdx.x;
  const double oc = *obs_count, rc = ret_stats[2];
  __syncthreads();
  for (int c = t; c <= O; c += 128) {
    if ((c < O && !upd_obs) || (c == O && !upd_ret)) continue;
    // (the block moments are fetched eight blocks at a time, all loads of a group in flight before the first add: one
    // dependent L2 round trip per block was 13 us for the 32 blocks of 4096 envs; the additions keep their order)
    double wsum = 0;
    for (int b0 = 0; b0 < nb; b0 += 8) {
      double pm[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) pm[k] = (b0 + k < nb) ? part[((size_t)(b0 + k) * (O + 1) + c) * 2] : 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int b = b0 + k;
        const int n_b = (N - b * MYO_VN_ROWS) < MYO_VN_ROWS ? (N - b * MYO_VN_ROWS) : MYO_VN_ROWS;
        if (b < nb) wsum += n_b * pm[k];
      }
    }
    const double bmean = wsum / N;
    double m2 = 0;
    for (int b0 = 0; b0 < nb; b0 += 8) {
      double pm[8], pv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        pm[k] = (b0 + k < nb) ? part[((size_t)(b0 + k) * (O + 1) + c) * 2] : 0.0;
        pv[k] = (b0 + k < nb) ? part[((size_t)(b0 + k) * (O + 1) + c) * 2 + 1] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int b = b0 + k;
        const int n_b = (N - b * MYO_VN_ROWS) < MYO_VN_ROWS ? (N - b * MYO_VN_ROWS) : MYO_VN_ROWS;
        const double dm = pm[k] - bmean;
        if (b < nb) m2 += pv[k] + n_b * dm * dm;
      }
    }
    const double bvar = m2 / N;
    double* mean = c < O ? obs_mean + c : ret_stats;
    double* var = c < O ? obs_var + c : ret_stats + 1;
    const double cnt = c < O ? oc : rc;
    const double delta = bmean - *mean, tot = cnt + N;
    const double new_mean = *mean + delta * N / tot;
    const double M2 = *var * cnt + bvar * N + delta * delta * cnt * N / tot;
    *mean = new_mean; *var = M2 / tot;
  }
  if (t == 0) { if (upd_obs) *obs_count = oc + N; if (upd_ret) ret_stats[2] = rc + N; }
}
// ---- the same update split at the point where N ranks exchange their batch moments (all-reduce
// (n, sum x, sum x^2) so that N ranks reproduce ONE VecNormalize over all envs).  k_vecnorm_batch turns the block
// moments of this rank into additive sums batch[0] = n, batch[1 + c] = sum x_c, batch[2 + O + c] = sum x_c^2 (column
// O = the discounted returns); after the caller's all-reduce(SUM) k_vecnorm_merge_batch does Chan's update from them.
__global__ void __launch_bounds__(128) k_vecnorm_batch(const double* __restrict__ part, int nb, int N, int O, double* __restrict__ batch) {
  const int t = threadIdx.x;
  for (int c = t; c <= O; c += 128) {
    double s1 = 0, s2 = 0;
    for (int b = 0; b < nb; ++b) {
      const int n_b = (N - b * MYO_VN_ROWS) < MYO_VN_ROWS ? (N - b * MYO_VN_ROWS) : MYO_VN_ROWS;
      const double m = part[((size_t)b * (O + 1) + c) * 2];
      s1 += n_b * m;
      s2 += part[((size_t)b * (O + 1) + c) * 2 + 1] + n_b * m * m;
    }
    batch[1 + c] = s1; batch[2 + O + c] = s2;
  }
  if (t == 0) batch[0] = (double)N;
}
__global__ void __launch_bounds__(128) k_vecnorm_merge_batch(const double* __restrict__ batch, int O, double* __restrict__ obs_mean,
                                                             double* __restrict__ obs_var, double* __restrict__ obs_count,
                                                             double* __restrict__ ret_stats, int upd_obs, int upd_ret) {
  const int t = threadIdx.x;
  const double oc = *obs_count, rc = ret_stats[2], n = batch[0];
  __syncthreads();
  for (int c = t; c <= O; c += 128) {
    if ((c < O && !upd_obs) || (c == O && !upd_ret)) continue;
    const double bmean = batch[1 + c] / n;
    double bvar = batch[2 + O + c] / n - bmean * bmean;
    bvar = bvar < 0 ? 0 : bvar;
    double* mean = c < O ? obs_mean + c : ret_stats;
    double* var = c < O ? obs_var + c : ret_stats + 1;
    const double cnt = c < O ? oc : rc;
    const double delta = bmean - *mean, tot = cnt + n;
    const double new_mean = *mean + delta * n / tot;
    const double M2 = *var * cnt + bvar * n + delta * delta * cnt * n / tot;
    *mean = new_mean; *var = M2 / tot;
  }
  if (t == 0) { if (upd_obs) *obs_count = oc + n; if (upd_ret) ret_stats[2] = rc + n; }
}
// kernel 3 of 3: normalise observation, terminal observation and reward with the UPDATED statistics,
// zero the returns of finished episodes, and write the rollout buffer rows of step t.
__global__ void __launch_bounds__(256) k_vecnorm_apply(const float* __restrict__ obs, const float* __restrict__ rew,
                                                       const unsigned char* __restrict__ done, const unsigned char* __restrict__ trunc,
                                                       const float* __restrict__ term, int N, int O, const double* __restrict__ obs_mean,
                                                       const double* __restrict__ obs_var, const double* __restrict__ ret_stats,
                                                       double* __restrict__ returns, double eps, double clip_obs, double clip_rew,
                                                       int norm_obs, int norm_rew, float* __restrict__ nobs, float* __restrict__ starts,
                                                       const int* __restrict__ t_idx, float* __restrict__ rew_buf,
                                                       float* __restrict__ start_buf, float* __restrict__ term_buf,
                                                       float* __restrict__ trunc_buf) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)N * O, tt = (size_t)(*t_idx);
  if (i < n) {
    const int c = (int)(i % O);
    double o = obs[i], q = term[i];
    if (norm_obs) {
      const double sd = sqrt(obs_var[c] + eps), mu = obs_mean[c];
      o = fmin(fmax((o - mu) / sd, -clip_obs), clip_obs);
      q = fmin(fmax((q - mu) / sd, -clip_obs), clip_obs);
    }
    nobs[i] = (float)o;
    if (term_buf) term_buf[tt * n + i] = (float)q;
  }
  if (i < (size_t)N) {
    double r = rew[i];
    if (norm_rew) r = fmin(fmax(r / sqrt(ret_stats[1] + eps), -clip_rew), clip_rew);
    rew_buf[tt * N + i] = (float)r;
    start_buf[tt * N + i] = starts[i];          // episode_starts of the step that produced this transition
    const unsigned char dn = done[i];
    starts[i] = dn ? 1.f : 0.f;
    if (trunc_buf) trunc_buf[tt * N + i] = trunc[i] ? 1.f : 0.f;
    if (dn) returns[i] = 0.0;
  }
}
// gSDE action sampling (SB3 StateDependentNoiseDistribution): one 64-lane block per env, lane j =
// action j.  noise_j = sum_l latent_l W[n][l][j] with the env's own exploration matrix W (drawn once per rollout),
// sigma_j = sqrt(sum_l latent_l^2 exp(log_std[l][j])^2 + 1e-6); action = mean + noise (unclipped, as stored by SB3),
// clipped copy for the env, log pi = sum_j log N(action_j; mean_j, sigma_j).  W rows are read coalesced (A contiguous).
__global__ void __launch_bounds__(64) k_sample_sde(const float* __restrict__ mean, const float* __restrict__ latent,
                                                   const float* __restrict__ W, const float* __restrict__ log_std, int N, int L, int A,
                                                   float* __restrict__ actions, float* __restrict__ clipped, float* __restrict__ logp,
                                                   int deterministic) {
  const int n = blockIdx.x, t = threadIdx.x;
  float lp_part = 0.f;
  for (int j = t; j < A; j += 64) {
    const float* w = W + (size_t)n * L * A + j;
    const float* lat = latent + (size_t)n * L;
    float noise = 0.f, var = 0.f;
    for (int l = 0; l < L; ++l) {
      const float x = lat[l], sd = __expf(log_std[(size_t)l * A + j]);
      noise = fmaf(x, w[(size_t)l * A], noise);
      var = fmaf(x * x, sd * sd, var);
    }
    const float mu = mean[(size_t)n * A + j], sg = sqrtf(var + 1e-6f);
    const float a = deterministic ? mu : mu + noise;
    actions[(size_t)n * A + j] = a;
    clipped[(size_t)n * A + j] = fminf(fmaxf(a, -1.f), 1.f);
    const float z = (a - mu) / sg;
    lp_part += -0.5f * z * z - logf(sg) - 0.9189385332046727f;
  }
  for (int off = 32; off >= 1; off >>= 1) lp_part += __shfl_xor(lp_part, off, 64);
  if (t == 0) logp[n] = lp_part;
}
__global__ void k_rollout_advance(int* t_idx, int T, unsigned long long* draw_counter) {
  *t_idx = (*t_idx + 1) % T;
  draw_counter[0] = draw_counter[1];
}
extern "C" int myo_rollout_policy_input(const float* obs, int N, int O, float* obs_buf, uint16_t* x_bf16, int copies,
                                        const int32_t* t_idx, void* stream) {
  if (!obs || !x_bf16 || !t_idx || N <= 0 || O <= 0 || copies <= 0) return fail(MYO_E_ARG, "myo_rollout_policy_input: bad arguments");
  const size_t n = (size_t)N * O;
  hipLaunchKernelGGL(k_obs_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, obs, n, obs_buf, x_bf16, copies, t_idx);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_rollout_sample(const uint16_t* mean_bf16, const uint16_t* value_bf16, const float* log_std, int N, int A,
                                  uint64_t seed, uint64_t* draw_counter, const int32_t* t_idx, float* act_buf, float* val_buf,
                                  float* logp_buf, float* clipped, int deterministic, void* stream) {
  if (!mean_bf16 || !value_bf16 || !log_std || !draw_counter || !t_idx || !act_buf || !val_buf || !logp_buf || !clipped || N <= 0 || A <= 0)
    return fail(MYO_E_ARG, "myo_rollout_sample: bad arguments");
  hipLaunchKernelGGL(k_sample_actions, dim3((N + MYO_SAMPLE_ROWS - 1) / MYO_SAMPLE_ROWS), dim3(16 * MYO_SAMPLE_ROWS), 0, (hipStream_t)stream, mean_bf16, value_bf16, log_std, N, A,
                     (unsigned long long)seed, (unsigned long long*)draw_counter, t_idx, act_buf, val_buf, logp_buf, clipped, deterministic);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_vecnorm_step(const float* obs, const float* rew, const uint8_t* done, const uint8_t* trunc, const float* term_obs,
                                int N, int O, double* obs_mean, double* obs_var, double* obs_count, double* ret_stats,
                                double* returns, double gamma, double eps, double clip_obs, double clip_rew, int training,
                                int norm_obs, int norm_reward, float* nobs, float* starts, const int32_t* t_idx, float* rew_buf,
                                float* start_buf, float* term_buf, float* trunc_buf, double* work, void* stream) {
  if (!obs || !rew || !done || !trunc || !term_obs || !obs_mean || !obs_var || !obs_count || !ret_stats || !returns || !nobs ||
      !starts || !t_idx || !rew_buf || !start_buf || !work || N <= 0 || O <= 0)
    return fail(MYO_E_ARG, "myo_vecnorm_step: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (N + MYO_VN_ROWS - 1) / MYO_VN_ROWS;
  hipLaunchKernelGGL(k_vecnorm_moments, dim3(nb), dim3(128), 0, st, obs, rew, N, O, returns, gamma, training, work);
  if (training)
    hipLaunchKernelGGL(k_vecnorm_merge, dim3(1), dim3(128), 0, st, work, nb, N, O, obs_mean, obs_var, obs_count, ret_stats,
                       (int)(training && norm_obs), (int)(training != 0));
  const size_t n = (size_t)N * O;
  hipLaunchKernelGGL(k_vecnorm_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, obs, rew, done, trunc, term_obs, N, O,
                     obs_mean, obs_var, ret_stats, returns, eps, clip_obs, clip_rew, norm_obs, norm_reward, nobs, starts, t_idx,
                     rew_buf, start_buf, term_buf, trunc_buf);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_rollout_sample_sde(const float* mean, const float* latent, const float* exploration_mat, const float* log_std,
                                      int N, int L, int A, float* actions, float* clipped, float* logp, int deterministic, void* stream) {
  if (!mean || !latent || !exploration_mat || !log_std || !actions || !clipped || !logp || N <= 0 || L <= 0 || A <= 0)
    return fail(MYO_E_ARG, "myo_rollout_sample_sde: bad arguments");
  hipLaunchKernelGGL(k_sample_sde, dim3(N), dim3(64), 0, (hipStream_t)stream, mean, latent, exploration_mat, log_std, N, L, A, actions,
                     clipped, logp, deterministic);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_vecnorm_batch_moments(const float* obs, const float* rew, int N, int O, double* returns, double gamma, int training,
                                         double* work, double* batch, void* stream) {
  if (!obs || !rew || !returns || !work || !batch || N <= 0 || O <= 0) return fail(MYO_E_ARG, "myo_vecnorm_batch_moments: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (N + MYO_VN_ROWS - 1) / MYO_VN_ROWS;
  hipLaunchKernelGGL(k_vecnorm_moments, dim3(nb), dim3(128), 0, st, obs, rew, N, O, returns, gamma, training, work);
  hipLaunchKernelGGL(k_vecnorm_batch, dim3(1), dim3(128), 0, st, work, nb, N, O, batch);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_vecnorm_finish(const float* obs, const float* rew, const uint8_t* done, const uint8_t* trunc, const float* term_obs,
                                  int N, int O, double* obs_mean, double* obs_var, double* obs_count, double* ret_stats,
                                  double* returns, double eps, double clip_obs, double clip_rew, int training, int norm_obs,
                                  int norm_reward, float* nobs, float* starts, const int32_t* t_idx, float* rew_buf, float* start_buf,
                                  float* term_buf, float* trunc_buf, const double* batch, void* stream) {
  if (!obs || !rew || !done || !trunc || !term_obs || !obs_mean || !obs_var || !obs_count || !ret_stats || !returns || !nobs ||
      !starts || !t_idx || !rew_buf || !start_buf || !batch || N <= 0 || O <= 0)
    return fail(MYO_E_ARG, "myo_vecnorm_finish: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (training)
    hipLaunchKernelGGL(k_vecnorm_merge_batch, dim3(1), dim3(128), 0, st, batch, O, obs_mean, obs_var, obs_count, ret_stats,
                       (int)(training && norm_obs), (int)(training != 0));
  const size_t n = (size_t)N * O;
  hipLaunchKernelGGL(k_vecnorm_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, obs, rew, done, trunc, term_obs, N, O,
                     obs_mean, obs_var, ret_stats, returns, eps, clip_obs, clip_rew, norm_obs, norm_reward, nobs, starts, t_idx,
                     rew_buf, start_buf, term_buf, trunc_buf);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_rollout_advance(int32_t* t_idx, int T, uint64_t* draw_counter, void* stream) {
  if (!t_idx || !draw_counter || T <= 0) return fail(MYO_E_ARG, "myo_rollout_advance: bad arguments");
  hipLaunchKernelGGL(k_rollout_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, t_idx, T, (unsigned long long*)draw_counter);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

// ------------------------------------------------------------------------------------------ LSTM cell
// One time step of G stacked one-layer LSTMs (PyTorch gate order i, f, g, o) around the recurrent GEMM,
// forward and backward (RecurrentActorCriticPolicy's lstm_actor / lstm_critic).  Rows
// r = g * N + n.  The episode-start mask of the NEXT step is folded in: the forward kernel emits the unmasked
// h (the sequence output) and the masked h, c that feed the next step's GEMM / cell; the backward kernel
// applies the same mask to the incoming state gradients.  E = float or bf16 storage, fp32 arithmetic.
template <typename E> __device__ __forceinline__ float myo_ld(const E* p, size_t i);
template <> __device__ __forceinline__ float myo_ld<float>(const float* p, size_t i) { return p[i]; }
template <> __device__ __forceinline__ float myo_ld<unsigned short>(const unsigned short* p, size_t i) { return __uint_as_float((unsigned)p[i] << 16); }
template <typename E> __device__ __forceinline__ void myo_st(E* p, size_t i, float v);
template <> __device__ __forceinline__ void myo_st<float>(float* p, size_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void myo_st<unsigned short>(unsigned short* p, size_t i, float v) { p[i] = myo_f2bf(v); }
__device__ __forceinline__ float myo_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }
template <typename E>
__global__ void __launch_bounds__(256) k_lstm_cell_fwd(const E* __restrict__ gx, const E* __restrict__ gh, const E* __restrict__ c_prev,
                                                       const float* __restrict__ keep_next, int R, int N, int H, E* __restrict__ out_h,
                                                       E* __restrict__ hm_next, E* __restrict__ cm_next, E* __restrict__ c_new,
                                                       E* __restrict__ ws) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)R * H) return;
  const int r = (int)(idx / H), j = (int)(idx % H);
  const size_t g0 = (size_t)r * 4 * H + j;
  const float i = myo_sigmoid(myo_ld(gx, g0) + myo_ld(gh, g0));
  const float f = myo_sigmoid(myo_ld(gx, g0 + H) + myo_ld(gh, g0 + H));
  const float g = tanhf(myo_ld(gx, g0 + 2 * H) + myo_ld(gh, g0 + 2 * H));
  const float o = myo_sigmoid(myo_ld(gx, g0 + 3 * H) + myo_ld(gh, g0 + 3 * H));
  const float c = f * myo_ld(c_prev, idx) + i * g;
  const float h = o * tanhf(c);
  const float k = keep_next ? keep_next[r % N] : 1.f;
  myo_st(out_h, idx, h);
  myo_st(c_new, idx, c);
  myo_st(hm_next, idx, h * k);
  myo_st(cm_next, idx, c * k);
  myo_st(ws, g0, i); myo_st(ws, g0 + H, f); myo_st(ws, g0 + 2 * H, g); myo_st(ws, g0 + 3 * H, o);
}
template <typename E>
__global__ void __launch_bounds__(256) k_lstm_cell_bwd(const E* __restrict__ dout, const E* __restrict__ dhm_next, const E* __restrict__ dcm_next,
                                                       const float* __restrict__ keep_next, const E* __restrict__ c_prev,
                                                       const E* __restrict__ c_new, const E* __restrict__ ws, int R, int N, int H,
                                                       E* __restrict__ dgates, E* __restrict__ dc_prev) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)R * H) return;
  const int r = (int)(idx / H), j = (int)(idx % H);
  const size_t g0 = (size_t)r * 4 * H + j;
  const float k = keep_next ? keep_next[r % N] : 1.f;
  const float dh = (dout ? myo_ld(dout, idx) : 0.f) + (dhm_next ? k * myo_ld(dhm_next, idx) : 0.f);
  const float dc_in = dcm_next ? k * myo_ld(dcm_next, idx) : 0.f;
  const float i = myo_ld(ws, g0), f = myo_ld(ws, g0 + H), g = myo_ld(ws, g0 + 2 * H), o = myo_ld(ws, g0 + 3 * H);
  const float tc = tanhf(myo_ld(c_new, idx));
  const float dct = dc_in + dh * o * (1.f - tc * tc);
  myo_st(dgates, g0, dct * g * i * (1.f - i));
  myo_st(dgates, g0 + H, dct * myo_ld(c_prev, idx) * f * (1.f - f));
  myo_st(dgates, g0 + 2 * H, dct * i * (1.f - g * g));
  myo_st(dgates, g0 + 3 * H, dh * tc * o * (1.f - o));
  myo_st(dc_prev, idx, dct * f);
}
extern "C" int myo_lstm_cell_fwd(const void* gx, const void* gh, const void* c_prev, const float* keep_next, int R, int N, int H,
                                 int is_bf16, void* out_h, void* hm_next, void* cm_next, void* c_new, void* ws, void* stream) {
  if (!gx || !gh || !c_prev || !out_h || !hm_next || !cm_next || !c_new || !ws || R <= 0 || N <= 0 || H <= 0 || R % N)
    return fail(MYO_E_ARG, "myo_lstm_cell_fwd: bad arguments");
  const unsigned nb = (unsigned)(((size_t)R * H + 255) / 256);
  if (is_bf16)
    hipLaunchKernelGGL(k_lstm_cell_fwd<unsigned short>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)gx,
                       (const unsigned short*)gh, (const unsigned short*)c_prev, keep_next, R, N, H, (unsigned short*)out_h,
                       (unsigned short*)hm_next, (unsigned short*)cm_next, (unsigned short*)c_new, (unsigned short*)ws);
  else
    hipLaunchKernelGGL(k_lstm_cell_fwd<float>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const float*)gx, (const float*)gh,
                       (const float*)c_prev, keep_next, R, N, H, (float*)out_h, (float*)hm_next, (float*)cm_next, (float*)c_new,
                       (float*)ws);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_lstm_cell_bwd(const void* dout, const void* dhm_next, const void* dcm_next, const float* keep_next,
                                 const void* c_prev, const void* c_new, const void* ws, int R, int N, int H, int is_bf16,
                                 void* dgates, void* dc_prev, void* stream) {
  if (!c_prev || !c_new || !ws || !dgates || !dc_prev || R <= 0 || N <= 0 || H <= 0 || R % N)
    return fail(MYO_E_ARG, "myo_lstm_cell_bwd: bad arguments");
  const unsigned nb = (unsigned)(((size_t)R * H + 255) / 256);
  if (is_bf16)
    hipLaunchKernelGGL(k_lstm_cell_bwd<unsigned short>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)dout,
                       (const unsigned short*)dhm_next, (const unsigned short*)dcm_next, keep_next, (const unsigned short*)c_prev,
                       (const unsigned short*)c_new, (const unsigned short*)ws, R, N, H, (unsigned short*)dgates,
                       (unsigned short*)dc_prev);
  else
    hipLaunchKernelGGL(k_lstm_cell_bwd<float>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const float*)dout, (const float*)dhm_next,
                       (const float*)dcm_next, keep_next, (const float*)c_prev, (const float*)c_new, (const float*)ws, R, N, H,
                       (float*)dgates, (float*)dc_prev);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

// ------------------------------------------------------------------------------------------ GAE
// compute_returns_and_advantage of SB3's RolloutBuffer: backward scan over T with
// the episode_starts[t+1] mask; one thread per env, coalesced over envs.  [T,N] row-major.
__global__ void k_gae(const float* __restrict__ rew, const float* __restrict__ val, const float* __restrict__ starts,
                      const float* __restrict__ last_val, const float* __restrict__ last_done, int T, int N, float gamma,
                      float lam, float* __restrict__ adv, float* __restrict__ ret) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  float last = 0.f, nextv = last_val[e], nonterm = 1.f - last_done[e];
  for (int t = T - 1; t >= 0; --t) {
    const size_t i = (size_t)t * N + e;
    const float v = val[i];
    const float delta = rew[i] + gamma * nextv * nonterm - v;
    last = delta + gamma * lam * nonterm * last;
    adv[i] = last;
    ret[i] = last + v;
    nextv = v;
    nonterm = 1.f - starts[i];
  }
}
extern "C" int myo_gae(const float* rew, const float* val, const float* starts, const float* last_val, const float* last_done,
                       int T, int N, float gamma, float lam, float* adv, float* ret, void* stream) {
  if (!rew || !val || !starts || !last_val || !last_done || !adv || !ret || T <= 0 || N <= 0) return fail(MYO_E_ARG, "myo_gae: bad arguments");
  hipLaunchKernelGGL(k_gae, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, rew, val, starts, last_val, last_done, T, N,
                     gamma, lam, adv, ret);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

#include "myo_ppo_mlp.h"      // (ahead of Adam: k_adam mirrors the parameters into the fused MLP step's operand images)

// ------------------------------------------------------------------------------------------ Adam
// clip_grad_norm_(max_norm) + torch.optim.Adam step (no weight decay / amsgrad) over ONE flat fp32
// parameter vector: 2 launches instead of ~12 multi-tensor ones.  scratch[0] = sum g^2 (after
// grad_scale), step = device-side step counter (incremented here).  SB3 semantics: SURVEY.md C.5.
#define MYO_SQN_BLOCKS 64
// scratch[0..63] <- per-block sums of (g*gs)^2 (fixed order inside a block: no float atomics);
// step[0] <- committed step count, step[1] <- pending (= this step's ordinal)
__global__ void __launch_bounds__(256) k_grad_sqnorm(const float* __restrict__ g, int n, float gs, float* __restrict__ part,
                                                     int* __restrict__ step, const float* __restrict__ hp) {
  float acc = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += MYO_SQN_BLOCKS * 256) { const float x = g[i] * gs; acc += x * x; }
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    // (hyper-parameter block with its stop flag up: this step is not taken, the counter stays)
    if (blockIdx.x == 0 && !(hp && reinterpret_cast<const int*>(hp)[MYO_HP_STOP])) { const int done = step[1]; step[0] = done; step[1] = done + 1; }
  }
}
__global__ void __launch_bounds__(256) k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, int n, float lr, float b1, float b2, float eps,
                                              float max_norm, float gs, const int* __restrict__ step,
                                              const float* __restrict__ part, unsigned short* __restrict__ p_bf16, int nparts,
                                              float* __restrict__ hp, MlpImgTarget tgt) {
  if (hp) {       // lr from the hyper-parameter block; stop flag up: p, m, v, the bf16 shadow and the images stay as they are
    if (reinterpret_cast<const int*>(hp)[MYO_HP_STOP]) return;
    lr = hp[MYO_HP_LR];
  }
  // |g|^2 from the partial sums: every block adds them in the same tree order (256 lanes, strided, then halving) — a serial
  // loop over them was one dependent scalar load per partial, 4 us for 64 and 21 us for 337
  __shared__ float sq_red[256];
  {
    float a = 0.f;
    for (int k = threadIdx.x; k < nparts; k += 256) a += part[k];
    sq_red[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) { if ((int)threadIdx.x < w) sq_red[threadIdx.x] += sq_red[threadIdx.x + w]; __syncthreads(); }
  }
  const float sq = sq_red[0];
  const int t = step[1];
  const float norm = sqrtf(sq);
  const float clip = (max_norm > 0.f) ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
  const float bc1 = 1.f - powf(b1, (float)t), bc2 = 1.f - powf(b2, (float)t);
  const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float gi = g[i] * gs * clip;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float pn = p[i] - step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    p[i] = pn;
    if (p_bf16) p_bf16[i] = myo_f2bf(pn);          // the bf16 shadow the GEMMs read: no separate cast pass
    if (tgt.img.W1p) mlp_img_store(tgt, i, pn);    // and the fused MLP step's operand images: no prep launch per step
  }
  if (hp && blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int*>(hp)[MYO_HP_APPLIED] += 1;
}
// (the host side, myo_adam_step, stands below the fused MLP step: it places the images from that step's descriptor)

// ------------------------------------------------------------------------------------------ fused MLP PPO step
struct MlpWs { MlpImages img; unsigned short *XT, *H1T, *H2T, *dH1T, *dH2T, *dOT; float *part, *slab, *advpart; size_t bytes; };
static MlpWs mlp_carve(unsigned char* base, int B, int OP, int A, long long G) {
  MlpWs w;
  size_t o = 0;
  w.img = mlp_images_carve(base, OP, &o);
  auto take = [&](size_t n) { unsigned char* p = base ? base + o : nullptr; o += (n + 255) / 256 * 256; return p; };
  const size_t H = MLP_H;
  w.XT = (unsigned short*)take((size_t)128 * B * 2);
  w.H1T = (unsigned short*)take(2 * H * (size_t)B * 2); w.H2T = (unsigned short*)take(2 * H * (size_t)B * 2);
  w.dH1T = (unsigned short*)take(2 * H * (size_t)B * 2); w.dH2T = (unsigned short*)take(2 * H * (size_t)B * 2);
  w.dOT = (unsigned short*)take((size_t)256 * B * 2);
  w.part = (float*)take((size_t)(2 * A + 6) * (B / MLP_BM) * 4);       // (+ 3 columns: approx_kl, clip fraction, entropy loss)
  w.slab = (float*)take((size_t)MLP_SPLITK * G * 4);
  w.advpart = (float*)take(3 * MLP_ADV_BLOCKS * 4);            // slices of the advantage moments
  w.bytes = o;
  return w;
}
static int mlp_shape_ok(int B, int O, int A, int hidden) {
  return hidden == MLP_H && O >= 1 && O <= MLP_OPMAX && A >= 1 && A <= MLP_APM && B >= 64 * MLP_SPLITK && B % (64 * MLP_SPLITK) == 0;
}
static int mlp_shape_check(const myo_ppo_mlp_desc* d, const char* who) {
  if (mlp_shape_ok(d->B, d->O, d->A, d->hidden)) return MYO_OK;
  return fail(MYO_E_UNSUPPORTED, "%s: needs hidden = %d, obs <= %d, act <= %d, batch a multiple of %d", who, MLP_H, MLP_OPMAX, MLP_APM, 64 * MLP_SPLITK);
}
extern "C" long long myo_ppo_mlp_workspace_bytes(int B, int obs_dim, int act_dim, int hidden, long long G) {
  if (!mlp_shape_ok(B, obs_dim, act_dim, hidden) || G <= 0) return -1;
  return (long long)mlp_carve(nullptr, B, (obs_dim + 31) / 32 * 32, act_dim, G).bytes;
}
extern "C" int myo_ppo_mlp_sqnorm_parts(int act_dim) {
  return MLP_RF_BLOCKS + 2 * act_dim + 3;
}
// The image pass: the images of the flat parameters `p` laid out by `lay`; adv_nb > 0: and the merge of that many slices of the
// advantage moments of B rows (k_mlp_prep's last block)
static void mlp_launch_prep(const float* p, const myo_mlp_layout& lay, int O, int A, const MlpImages& img, const float* adv_part, float* adv_stats,
                            int adv_nb, int B, hipStream_t st) {
  MlpPrepArgs pp;
  pp.p = p; pp.O = O; pp.OP = (O + 31) / 32 * 32; pp.Ah[0] = A; pp.Ah[1] = 1; pp.img = img;
  for (int k = 0; k < 2; ++k) {
    pp.off_W1[k] = lay.off_W1[k]; pp.off_b1[k] = lay.off_b1[k]; pp.off_W2[k] = lay.off_W2[k]; pp.off_b2[k] = lay.off_b2[k];
    pp.off_Wh[k] = lay.off_Wh[k]; pp.off_bh[k] = lay.off_bh[k];
  }
  pp.adv_part = adv_part; pp.adv_stats = adv_stats; pp.adv_nb = adv_nb; pp.B = B;
  hipLaunchKernelGGL(k_mlp_prep, dim3(256), dim3(256), 0, st, pp);
}
// resident: the operand images at the front of the workspace are current (myo_ppo_mlp_images once, then the Adam kernel of
// myo_adam_step with `images` after every step) and the advantage moments are the caller's: neither k_adv_moments nor k_mlp_prep runs
static int mlp_step(const myo_ppo_mlp_desc* d, void* stream, bool resident, int activation, const char* who) {
  if (!d || !d->obs || !d->act || !d->oldlp || !d->adv || !d->ret || !d->idx || !d->params || !d->grads || !d->adv_stats || !d->acc ||
      !d->workspace)
    return fail(MYO_E_ARG, "%s: null argument", who);
  if (!myo_act_known(activation)) return fail(MYO_E_ARG, "%s: unknown activation code %d", who, activation);
  const int B = d->B, O = d->O, A = d->A, OP = (O + 31) / 32 * 32;
  const myo_mlp_layout& lay = d->layout;
  if (int rc = mlp_shape_check(d, who)) return rc;
  if (resident && d->compute_adv_stats) return fail(MYO_E_ARG, "%s: the advantage moments are the caller's (compute_adv_stats = 0)", who);
  const MlpWs w = mlp_carve((unsigned char*)d->workspace, B, OP, A, d->G);
  if ((long long)w.bytes > d->workspace_bytes) return fail(MYO_E_ARG, "%s: workspace too small (%zu bytes needed)", who, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  const bool tanh_act = activation == MYO_ACT_TANH;
  void (*const fwdbwd)(MlpArgs) = tanh_act ? k_mlp_fwdbwd<MYO_ACT_TANH> : k_mlp_fwdbwd<MYO_ACT_RELU>;
  static bool lds_set[2] = {false, false};
  if (!lds_set[tanh_act]) {
    if (hipFuncSetAttribute((const void*)fwdbwd, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_FWDBWD_LDS) != hipSuccess)
      return fail(MYO_E_DEVICE, "%s: cannot reserve %d bytes of LDS", who, (int)MLP_FWDBWD_LDS);
    lds_set[tanh_act] = true;
  }
  if (!resident) {
    if (d->compute_adv_stats) hipLaunchKernelGGL(k_adv_moments, dim3(MLP_ADV_BLOCKS), dim3(256), 0, st, d->adv, (const long long*)d->idx, B, w.advpart);
    mlp_launch_prep(d->params, lay, O, A, w.img, w.advpart, d->adv_stats, d->compute_adv_stats ? MLP_ADV_BLOCKS : 0, B, st);
  }
  MlpArgs a;
  a.obs = d->obs; a.act = d->act; a.oldlp = d->oldlp; a.adv = d->adv; a.ret = d->ret; a.idx = (const long long*)d->idx;
  a.log_std = d->params + lay.off_log_std; a.adv_stats = d->adv_stats; a.img = w.img;
  a.XT = w.XT; a.H1T = w.H1T; a.H2T = w.H2T; a.dH1T = w.dH1T; a.dH2T = w.dH2T; a.dOT = w.dOT; a.part = w.part;
  a.B = B; a.O = O; a.A = A; a.OP = OP; a.NB = B / MLP_BM; a.clip = d->clip; a.vf_coef = d->vf_coef; a.hp = d->hp;
  hipLaunchKernelGGL(fwdbwd, dim3(B / MLP_BM, 2), dim3(256), MLP_FWDBWD_LDS, st, a);
  MlpWgradArgs g;
  g.njobs = 0; g.B = B; g.rows_per_split = B / MLP_SPLITK; g.G = d->G; g.slab = w.slab;
  const size_t HB = (size_t)MLP_H * B;
  for (int net = 0; net < 2; ++net) {
    for (int m0 = 0; m0 < MLP_H; m0 += 128) {
      for (int n0 = 0; n0 < MLP_H; n0 += 128)
        g.job[g.njobs++] = MlpWgradJob{w.dH2T + net * HB, w.H1T + net * HB, MLP_H, MLP_H, MLP_H, m0, n0, lay.off_W2[net], n0 == 0 ? lay.off_b2[net] : -1};
      g.job[g.njobs++] = MlpWgradJob{w.dH1T + net * HB, w.XT, MLP_H, O, O, m0, 0, lay.off_W1[net], lay.off_b1[net]};
    }
    for (int n0 = 0; n0 < MLP_H; n0 += 128)
      g.job[g.njobs++] = MlpWgradJob{w.dOT + (size_t)net * 128 * B, w.H2T + net * HB, net == 0 ? A : 1, MLP_H, MLP_H, 0, n0, lay.off_Wh[net], -1};
  }
  hipLaunchKernelGGL(k_mlp_wgrad, dim3(g.njobs * MLP_SPLITK), dim3(256), 0, st, g);
  if (d->sqnorm_part && d->adam_step) {
    MlpRfArgs rf;
    rf.slab = w.slab; rf.g = d->grads; rf.G = d->G; rf.splits = MLP_SPLITK; rf.part = w.part; rf.acc = d->acc; rf.NB = B / MLP_BM; rf.A = A;
    rf.ent_coef = d->ent_coef; rf.off_log_std = lay.off_log_std; rf.off_bh0 = lay.off_bh[0]; rf.off_bh1 = lay.off_bh[1];
    rf.sq_part = d->sqnorm_part; rf.adam_step = d->adam_step; rf.hp = d->hp;
    hipLaunchKernelGGL(k_mlp_reduce_finish, dim3(MLP_RF_BLOCKS + 2 * A + 3), dim3(256), 0, st, rf);
  } else {
    hipLaunchKernelGGL(k_mlp_reduce, dim3((unsigned)((d->G + 255) / 256)), dim3(256), 0, st, (const float*)w.slab, d->grads, d->G, MLP_SPLITK);
    hipLaunchKernelGGL(k_colmajor_finish, dim3(2 * A + 3 + (d->hp ? 1 : 0)), dim3(64), 0, st, (const float*)w.part, d->acc, B / MLP_BM, A, d->ent_coef,
                       d->grads + lay.off_log_std, d->grads + lay.off_bh[0], d->grads + lay.off_bh[1], d->hp);
  }
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_ppo_mlp_step_act(const myo_ppo_mlp_desc* d, int resident, int activation, void* stream) {
  return mlp_step(d, stream, resident != 0, activation, "myo_ppo_mlp_step_act");
}
extern "C" int myo_ppo_mlp_step(const myo_ppo_mlp_desc* d, void* stream) { return mlp_step(d, stream, false, MYO_ACT_RELU, "myo_ppo_mlp_step"); }
extern "C" int myo_ppo_mlp_step_resident(const myo_ppo_mlp_desc* d, void* stream) { return mlp_step(d, stream, true, MYO_ACT_RELU, "myo_ppo_mlp_step_resident"); }
// the checks the image calls share (the fields of `d` that place the images); *img <- the images in d's workspace
static int mlp_images_ok(const myo_ppo_mlp_desc* d, const char* who, MlpImages* img) {
  if (!d || !d->params || !d->workspace) return fail(MYO_E_ARG, "%s: null argument", who);
  if (int rc = mlp_shape_check(d, who)) return rc;
  const MlpWs w = mlp_carve((unsigned char*)d->workspace, d->B, (d->O + 31) / 32 * 32, d->A, d->G);
  if ((long long)w.bytes > d->workspace_bytes) return fail(MYO_E_ARG, "%s: workspace too small (%zu bytes needed)", who, w.bytes);
  *img = w.img;
  return MYO_OK;
}
extern "C" int myo_ppo_mlp_images(const myo_ppo_mlp_desc* d, void* stream) {
  MlpImages img;
  if (int rc = mlp_images_ok(d, "myo_ppo_mlp_images", &img)) return rc;
  mlp_launch_prep(d->params, d->layout, d->O, d->A, img, nullptr, nullptr, 0, d->B, (hipStream_t)stream);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

// k_adam's image target from the fused step's descriptor (k_adam indexes the flat vector with an int: every tensor offset has to
// lie inside its n elements)
static int mlp_img_target(const myo_ppo_mlp_desc* d, int n, const char* who, MlpImgTarget* T) {
  if (int rc = mlp_images_ok(d, who, &T->img)) return rc;
  if (d->G != n) return fail(MYO_E_ARG, "%s: the descriptor's parameter vector has %lld elements, this one %d", who, (long long)d->G, n);
  bool inside = true;
  auto put = [&](int (&dst)[2], const int64_t (&src)[2]) {
    for (int k = 0; k < 2; ++k) { inside = inside && src[k] >= 0 && src[k] < n; dst[k] = (int)src[k]; }
  };
  const myo_mlp_layout& lay = d->layout;
  put(T->off_W1, lay.off_W1); put(T->off_b1, lay.off_b1); put(T->off_W2, lay.off_W2); put(T->off_b2, lay.off_b2);
  put(T->off_Wh, lay.off_Wh); put(T->off_bh, lay.off_bh);
  if (!inside) return fail(MYO_E_ARG, "%s: a tensor offset lies outside the %d parameters", who, n);
  T->O = d->O; T->OP = (d->O + 31) / 32 * 32; T->A = d->A;
  return MYO_OK;
}
// clip_grad_norm_ + Adam over the flat vector (k_grad_sqnorm, k_adam above), one entry point: a->nparts == 0 takes the squares
// of g here (MYO_SQN_BLOCKS partial sums) and advances `step`; > 0 finds both done.  a->images: k_adam mirrors into its images.
extern "C" int myo_adam_step(const myo_adam_desc* a, void* stream) {
  if (!a || !a->p || !a->g || !a->m || !a->v || !a->step || !a->scratch || a->n <= 0 || a->nparts < 0) return fail(MYO_E_ARG, "myo_adam_step: bad arguments");
  const int n = a->n;
  MlpImgTarget T = {};
  if (a->images)
    if (int rc = mlp_img_target(a->images, n, "myo_adam_step", &T)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  if (a->nparts == 0)
    hipLaunchKernelGGL(k_grad_sqnorm, dim3(MYO_SQN_BLOCKS), dim3(256), 0, st, a->g, n, a->grad_scale, a->scratch, (int*)a->step, (const float*)a->hp);
  hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(256), 0, st, a->p, a->g, a->m, a->v, n, a->lr, a->b1, a->b2, a->eps, a->max_norm, a->grad_scale,
                     (const int*)a->step, (const float*)a->scratch, (unsigned short*)a->p_bf16, a->nparts ? a->nparts : MYO_SQN_BLOCKS, a->hp, T);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_ppo_adv_moments_epoch(const float* adv, const int64_t* idx, int B, int n_mb, float* stats, float* scratch, void* stream) {
  if (!adv || !idx || !stats || !scratch || B <= 0 || n_mb <= 0 || n_mb > 65535) return fail(MYO_E_ARG, "myo_ppo_adv_moments_epoch: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adv_moments, dim3(MLP_ADV_BLOCKS, n_mb), dim3(256), 0, st, adv, (const long long*)idx, B, scratch);
  hipLaunchKernelGGL(k_adv_merge, dim3(n_mb), dim3(256), 0, st, (const float*)scratch, MLP_ADV_BLOCKS, B, stats);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

extern "C" long long myo_ppo_mlp_rollout_workspace_bytes(int obs_dim, int act_dim, int hidden) {
  if (hidden != MLP_H || obs_dim < 1 || obs_dim > MLP_OPMAX || act_dim < 1 || act_dim > MLP_APM) return -1;
  size_t bytes;
  mlp_images_carve(nullptr, (obs_dim + 31) / 32 * 32, &bytes);
  return (long long)bytes;
}
// the checks the rollout calls share; *img <- the rollout's own images in d's workspace
static int mlp_rollout_images(const myo_ppo_mlp_rollout_desc* d, const char* who, MlpImages* img) {
  if (!(d->hidden == MLP_H && d->O >= 1 && d->O <= MLP_OPMAX && d->A >= 1 && d->A <= MLP_APM && d->N >= MLP_BM && d->N % MLP_BM == 0))
    return fail(MYO_E_UNSUPPORTED, "myo_ppo_mlp_rollout: needs hidden = %d, obs <= %d, act <= %d, envs a multiple of %d", MLP_H, MLP_OPMAX, MLP_APM, MLP_BM);
  size_t bytes;
  *img = mlp_images_carve((unsigned char*)d->workspace, (d->O + 31) / 32 * 32, &bytes);
  if ((long long)bytes > d->workspace_bytes) return fail(MYO_E_ARG, "%s: workspace too small (%zu bytes needed)", who, bytes);
  return MYO_OK;
}
extern "C" int myo_ppo_mlp_rollout_refresh(const myo_ppo_mlp_rollout_desc* d, void* stream) {
  if (!d || !d->params || !d->workspace) return fail(MYO_E_ARG, "myo_ppo_mlp_rollout_refresh: null argument");
  MlpImages img;
  if (int rc = mlp_rollout_images(d, "myo_ppo_mlp_rollout_refresh", &img)) return rc;
  mlp_launch_prep(d->params, d->layout, d->O, d->A, img, nullptr, nullptr, 0, 0, (hipStream_t)stream);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
static int mlp_rollout(const myo_ppo_mlp_rollout_desc* d, int activation, void* stream, const char* who) {
  if (!d || !d->obs || !d->params || !d->draw_counter || !d->t_idx || !d->act_buf || !d->val_buf || !d->logp_buf || !d->clipped || !d->workspace)
    return fail(MYO_E_ARG, "%s: null argument", who);
  if (!myo_act_known(activation)) return fail(MYO_E_ARG, "%s: unknown activation code %d", who, activation);
  MlpPolicyArgs a;
  if (int rc = mlp_rollout_images(d, who, &a.img)) return rc;
  a.obs = d->obs; a.log_std = d->params + d->layout.off_log_std;
  a.obs_buf = d->obs_buf; a.act_buf = d->act_buf; a.val_buf = d->val_buf; a.logp_buf = d->logp_buf; a.clipped = d->clipped;
  a.t_idx = d->t_idx; a.draw_counter = (unsigned long long*)d->draw_counter; a.seed = d->seed;
  a.N = d->N; a.O = d->O; a.A = d->A; a.OP = (d->O + 31) / 32 * 32; a.deterministic = d->deterministic;
  hipLaunchKernelGGL(activation == MYO_ACT_TANH ? k_mlp_policy<MYO_ACT_TANH> : k_mlp_policy<MYO_ACT_RELU>, dim3(d->N / MLP_BM, 2), dim3(256), MLP_POLICY_LDS,
                     (hipStream_t)stream, a);
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_ppo_mlp_rollout_act(const myo_ppo_mlp_rollout_desc* d, int activation, void* stream) {
  return mlp_rollout(d, activation, stream, "myo_ppo_mlp_rollout_act");
}
extern "C" int myo_ppo_mlp_rollout(const myo_ppo_mlp_rollout_desc* d, void* stream) { return mlp_rollout(d, MYO_ACT_RELU, stream, "myo_ppo_mlp_rollout"); }

// ------------------------------------------------------------------------------------------ fused LSTM time step
#include "myo_lstm_step.h"
extern "C" int myo_lstm_step_supported(int H) { return (H == 32 || H == 64 || H == 128 || H == 256) ? 1 : 0; }
extern "C" int myo_lstm_step_fwd(const void* gx, long long gx_sg, long long gx_sr, const void* h_prev, const void* c_prev, const void* w_hh,
                                 const float* keep_next, int G, int N, int H, void* out_h, long long out_sg, void* hm_next, void* cm_next,
                                 void* c_new, void* ws, const float* c_prev32, float* cm_next32, void* stream) {
  if (!gx || !h_prev || (!c_prev && !c_prev32) || !w_hh || !out_h || !hm_next || (!cm_next && !cm_next32) || G <= 0 || N <= 0 || H <= 0 || (gx_sg & 3) || (gx_sr & 3) || (out_sg & 3))
    return fail(MYO_E_ARG, "myo_lstm_step_fwd: bad arguments");
  if (!myo_lstm_step_supported(H)) return fail(MYO_E_UNSUPPORTED, "myo_lstm_step_fwd: hidden size %d (32, 64, 128 or 256)", H);
  typedef const unsigned short* cu;
  typedef unsigned short* mu;
#define MYO_LSTM_FWD(HH)                                                                                                              \
  lstm_step_fwd_launch<HH>((cu)gx, gx_sg, gx_sr, (cu)h_prev, (cu)c_prev, (cu)w_hh, keep_next, G, N, (mu)out_h, out_sg, (mu)hm_next,   \
                           (mu)cm_next, (mu)c_new, (mu)ws, c_prev32, cm_next32, (hipStream_t)stream)
  switch (H) {
    case 32: MYO_LSTM_FWD(32); break;
    case 64: MYO_LSTM_FWD(64); break;
    case 128: MYO_LSTM_FWD(128); break;
    default: MYO_LSTM_FWD(256); break;
  }
#undef MYO_LSTM_FWD
  LAUNCH_CHECK(0)
  return MYO_OK;
}
extern "C" int myo_lstm_step_bwd(const void* dout, long long dout_sg, const void* dgates_next, const void* dcm_next, const void* w_hh_t,
                                 const float* keep_next, const void* c_prev, const void* c_new, const void* ws, int G, int N, int H,
                                 void* dgates, void* dc_prev, void* stream) {
  if (!c_prev || !c_new || !ws || !dgates || !dc_prev || (dgates_next && !w_hh_t) || G <= 0 || N <= 0 || H <= 0 || (dout_sg & 3))
    return fail(MYO_E_ARG, "myo_lstm_step_bwd: bad arguments");
  if (!myo_lstm_step_supported(H)) return fail(MYO_E_UNSUPPORTED, "myo_lstm_step_bwd: hidden size %d (32, 64, 128 or 256)", H);
  typedef const unsigned short* cu;
  typedef unsigned short* mu;
#define MYO_LSTM_BWD(HH)                                                                                                               \
  lstm_step_bwd_launch<HH>((cu)dout, dout_sg, (cu)dgates_next, (cu)dcm_next, (cu)w_hh_t, keep_next, (cu)c_prev, (cu)c_new, (cu)ws, G, N, \
                           (mu)dgates, (mu)dc_prev, (hipStream_t)stream)
  switch (H) {
    case 32: MYO_LSTM_BWD(32); break;
    case 64: MYO_LSTM_BWD(64); break;
    case 128: MYO_LSTM_BWD(128); break;
    default: MYO_LSTM_BWD(256); break;
  }
#undef MYO_LSTM_BWD
  LAUNCH_CHECK(0)
  return MYO_OK;
}

// ------------------------------------------------------------------------------------------ ensemble acting step
#include "myo_ensemble.h"
extern "C" int myo_ensemble_supported(int H, int O, int A) {
  return ((H == 128 || H == 256) && O >= 1 && O <= ENS_OPMAX && A >= 1 && A <= ENS_APM) ? 1 : 0;
}
extern "C" int myo_ensemble_act(const myo_ensemble_desc* d, void* stream) {
  if (!d) return fail(MYO_E_ARG, "myo_ensemble_act: null descriptor");
  if (d->N <= 0 || d->O <= 0 || d->A <= 0 || d->H <= 0 || d->M0 <= 0 || d->M1 < 0)
    return fail(MYO_E_ARG, "myo_ensemble_act: non-positive size (N %d, O %d, A %d, H %d, M0 %d, M1 %d)", d->N, d->O, d->A, d->H, d->M0, d->M1);
  if (!d->obs || !d->mean || !d->var || !d->w_gates || !d->w_a || !d->b_gates || !d->b_a || !d->h || !d->c || !d->start0 || !d->act ||
      (d->M1 > 0 && (!d->start1 || !d->use_group1)))
    return fail(MYO_E_ARG, "myo_ensemble_act: null argument");
  if (!myo_ensemble_supported(d->H, d->O, d->A))
    return fail(MYO_E_UNSUPPORTED, "myo_ensemble_act: needs hidden 128 or 256, obs <= %d, act <= %d (got %d, %d, %d)", ENS_OPMAX, ENS_APM, d->H, d->O, d->A);
  EnsArgs a;
  a.obs = d->obs; a.mean = d->mean; a.var = d->var; a.eps = d->eps; a.clip = d->clip;
  a.w_gates = d->w_gates; a.w_a = d->w_a; a.b_gates = d->b_gates; a.b_a = d->b_a; a.h = d->h; a.c = d->c;
  a.start0 = d->start0; a.start1 = d->start1; a.use_group1 = d->use_group1; a.act = d->act; a.member_act = d->member_act;
  a.N = d->N; a.O = d->O; a.OP = (d->O + 31) / 32 * 32; a.A = d->A; a.M0 = d->M0; a.M1 = d->M1;
  if (d->H == 128) ensemble_launch<128>(a, (hipStream_t)stream);
  else ensemble_launch<256>(a, (hipStream_t)stream);
  LAUNCH_CHECK(0)
  return MYO_OK;
}

// whole sequences in one launch per direction (csrc/myo_lstm_seq.h)
#include "myo_lstm_seq.h"
extern "C" int myo_lstm_seq_supported(int H) { return (H == 128 || H == 256) ? 1 : 0; }
// row_split RS: a workgroup owns 16 / RS sequences (1, 2, or 4 at H = 256); the weight fragments and the tile-major arrays are laid out for it
static int lstm_seq_rs_ok(int H, int rs) { return rs == 1 || rs == 2 || (rs == 4 && H == 256); }
extern "C" int myo_lstm_seq_fwd(const void* gx, long long gx_st, long long gx_sg, long long gx_sr, void* hm, void* cm, const void* w_frag,
                                const float* keep, int G, int N, int H, int T, int row_split, void* out_h, long long out_sg, long long out_st,
                                void* c_new, void* ws, const float* c0_32, void* stream) {
  if (!gx || !hm || !cm || !w_frag || !keep || !out_h || !c_new || !ws || G <= 0 || N <= 0 || H <= 0 || T <= 0 || (gx_st & 7) || (gx_sg & 7) ||
      (gx_sr & 7) || (out_sg & 7) || (out_st & 7) || (N & 15))
    return fail(MYO_E_ARG, "myo_lstm_seq_fwd: bad arguments (N must be a multiple of 16, strides of 8)");
  if (!myo_lstm_seq_supported(H) || !lstm_seq_rs_ok(H, row_split))
    return fail(MYO_E_UNSUPPORTED, "myo_lstm_seq_fwd: hidden size %d (128 or 256) with row split %d (1, 2; 4 at 256)", H, row_split);
  typedef const unsigned short* cu;
  typedef unsigned short* mu;
#define MYO_SEQ_FWD(HH, RR) lstm_seq_fwd_launch<HH, RR>((cu)gx, gx_st, gx_sg, gx_sr, (mu)hm, (mu)cm, (cu)w_frag, keep, G, N, T, (mu)out_h, out_sg, out_st, \
                                                        (mu)c_new, (mu)ws, c0_32, (hipStream_t)stream)
  const int rc = H == 128 ? (row_split == 1 ? MYO_SEQ_FWD(128, 1) : MYO_SEQ_FWD(128, 2))
                          : (row_split == 1 ? MYO_SEQ_FWD(256, 1) : row_split == 2 ? MYO_SEQ_FWD(256, 2) : MYO_SEQ_FWD(256, 4));
#undef MYO_SEQ_FWD
  return rc ? fail(MYO_E_DEVICE, "myo_lstm_seq_fwd: launch failed") : MYO_OK;
}
extern "C" int myo_lstm_seq_bwd(const void* dout, long long dout_sg, long long dout_st, const void* wt_frag, const float* keep, const void* cm,
                                const void* c_new, const void* ws, int G, int N, int H, int T, int row_split, void* dgates, void* stream) {
  if (!dout || !wt_frag || !keep || !cm || !c_new || !ws || !dgates || G <= 0 || N <= 0 || H <= 0 || T <= 0 || (dout_sg & 7) || (dout_st & 7) || (N & 15))
    return fail(MYO_E_ARG, "myo_lstm_seq_bwd: bad arguments (N must be a multiple of 16, strides of 8)");
  if (!myo_lstm_seq_supported(H) || !lstm_seq_rs_ok(H, row_split))
    return fail(MYO_E_UNSUPPORTED, "myo_lstm_seq_bwd: hidden size %d (128 or 256) with row split %d (1, 2; 4 at 256)", H, row_split);
  typedef const unsigned short* cu;
#define MYO_SEQ_BWD(HH, RR) lstm_seq_bwd_launch<HH, RR>((cu)dout, dout_sg, dout_st, (cu)wt_frag, keep, (cu)cm, (cu)c_new, (cu)ws, G, N, T, \
                                                        (unsigned short*)dgates, (hipStream_t)stream)
  const int rc = H == 128 ? (row_split == 1 ? MYO_SEQ_BWD(128, 1) : MYO_SEQ_BWD(128, 2))
                          : (row_split == 1 ? MYO_SEQ_BWD(256, 1) : row_split == 2 ? MYO_SEQ_BWD(256, 2) : MYO_SEQ_BWD(256, 4));
#undef MYO_SEQ_BWD
  return rc ? fail(MYO_E_DEVICE, "myo_lstm_seq_bwd: launch failed") : MYO_OK;
}
