// emu_host.h — TEST TOOLING: the host side of the lane-serial emulation build (tests/emu/libmyobatch_emu.so = csrc/myobatch_emu.cpp).
// The kernel SOURCE (wave.h / myo_physics.h / myo_task.h, compiled with -DMYO_EMU: a phase's lanes run one after the other) is stepped
// env by env on the CPU, through the same records, layouts and task blocks as the product (csrc/myo_host.h), so that the wave-parallel
// algorithm can be checked against the oracle without a GPU.  The env-path entry points are the product's own (csrc/myo_host.h: checks,
// early returns, plans and workspaces); this file holds only the backend primitives under them — be_run and be_step loop over blocks
// where the product launches k_env and k_step, be_cast loops over tiles and threads where it launches the ray cast.  The PPO-side
// kernels have no CPU twin.  Nothing here is compiled into libmyobatch.so.
#pragma once
// ------------------------------------------------------------------------------------------ backend
static int be_malloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? 0 : -1; }
static void be_free(void* p) { free(p); }
static int be_h2d(void* d, const void* h, size_t n) { memcpy(d, h, n); return 0; }
static int be_set_device(int) { return 0; }
static const char* be_errstr(int) { return "emu"; }

static int be_batch_workspaces(myo_batch* b, int n_envs, int device) {
  (void)device;
  int rc = 0;
  b->K.ctrl_ws = dev_alloc<double>(b->allocs, rc, (size_t)n_envs * MYO_ENVWS_N);             // (emulation: one workspace per env)
  if (b->ncap > MYO_NCON_MAX) b->K.big_ws = dev_alloc<char>(b->allocs, rc, (size_t)n_envs * MYO_BIGWS_BYTES);
  return rc;
}
static int be_batch_launch_state(myo_batch* b, const myo_model* m, int n_envs, int rc) { (void)b; (void)m; (void)n_envs; return rc; }
static void be_batch_release(myo_batch* b, int device, int destroying) { (void)b; (void)device; (void)destroying; }

static void be_xfer(myo_batch* b, int off, int cnt, double* ext, int to_ext, void*) {
  if (!ext) return;
  for (int e = 0; e < b->n; ++e)
    for (int k = 0; k < cnt; ++k) {
      double* r = b->rec + (size_t)e * b->L.stride + off + k;
      if (to_ext) ext[(size_t)e * cnt + k] = *r; else *r = ext[(size_t)e * cnt + k];
    }
}
static void be_xfer_i(myo_batch* b, int off, int cnt, int* ext, int to_ext, void*) {
  if (!ext) return;
  for (int e = 0; e < b->n; ++e)
    for (int k = 0; k < cnt; ++k) {
      double* r = b->rec + (size_t)e * b->L.stride + off + k;
      if (to_ext) ext[(size_t)e * cnt + k] = (int)*r; else *r = (double)ext[(size_t)e * cnt + k];
    }
}
static int be_capturing(void*) { return 0; }
static int be_launch_status() { return MYO_OK; }
static void be_task_changed(myo_batch*) {}

// One zeroed scratch of the batch's kernel variant (with_variant, csrc/myo_host.h) with its RK4 stage block, handed together with the
// variant and its model to f(variant, model, scratch): what a workgroup has in LDS, here on the heap and used for one env after the other
template <typename F>
static void with_scratch(myo_batch* b, F&& f) {
  with_variant(b, [&](auto v) {
    using V = decltype(v);
    using T = typename V::T;
    Scratch<T, V::NC>* s = new Scratch<T, V::NC>();
    memset(s, 0, sizeof *s);
    RkScratch<T>* rk = new RkScratch<T>();
    s->rk = rk;
    if constexpr (sizeof(T) == sizeof(double)) f(v, b->Md, *s); else f(v, b->Mf, *s);
    delete s; delete rk;
  });
}
// the blocks of a k_env launch one after the other
template <typename Job>
static int be_run(myo_batch* b, const Job& J, int nblocks, void*, int) {
  with_scratch(b, [&](auto v, auto& M, auto& s) { for (int r = 0; r < nblocks; ++r) job_run(J, v, M, b->K, b->L, b->rec, s, r, b->n); });
  return MYO_OK;
}
// the parts of the step plan one after the other, each through the env record like the workgroups of k_step
static int be_step(myo_batch* b, const float* act, float* obs, float* rew, uint8_t* done, uint8_t* trunc, float* term_obs, float* comps,
                   float* ep_info, void*) {
  with_scratch(b, [&](auto, auto& M, auto& s) {
    for (int p = 0; p < b->plan.nparts; ++p) {
      const int k_lo = b->plan.k[p], k_hi = p == b->plan.nparts - 1 ? -1 : b->plan.k[p + 1];
      for (int env = 0; env < b->n; ++env)
        env_step(M, b->K, b->L, b->rec + (size_t)env * b->L.stride, s, env, act, obs, rew, done, trunc, term_obs, comps, ep_info, b->bad_state, k_lo, k_hi);
    }
  });
  return MYO_OK;
}
static int be_bind(myo_batch*, void*) { return MYO_OK; }
static int be_wrap_order(myo_batch*, void*) { return MYO_OK; }
static int be_set_step_generation(myo_batch*, unsigned int) { return MYO_OK; }
static double be_kernel_ms(myo_batch*) { return -1.0; }
static int be_wave_slots(int, int, int, int32_t*) { return fail(MYO_E_UNSUPPORTED, "myo_debug_wave_slots: no wave slots in the emulation build"); }
static int be_health(myo_batch* b, int out[4]) { memcpy(out, b->K.health, 4 * sizeof(int)); return MYO_OK; }
static int be_copy_envs(myo_batch* dst, const int* dst_idx, const myo_batch* src, const int* src_idx, int k, void*) {
  for (int r = 0; r < k; ++r) {
    const int d = dst_idx[r], s = src_idx[r];
    if (d < 0 || d >= dst->n || s < 0 || s >= src->n) continue;
    memcpy(dst->rec + (size_t)d * dst->L.stride, src->rec + (size_t)s * src->L.stride, sizeof(double) * (size_t)dst->L.stride);
  }
  return MYO_OK;
}
static int be_camera_upload(myo_batch*, double* dst, std::vector<double>& cam_tab, void*) { memcpy(dst, cam_tab.data(), cam_tab.size() * sizeof(double)); return MYO_OK; }
// the ray cast tile by tile, a kernel's thread phases (what lies between two barriers) one after the other, in the device's workspace
// layout (render_plan): the plain arm is k_render, the layered arm k_render_layers
static int be_cast(myo_batch* b, const RenderPlan& p, int k, int ncams, int width, int height, int flags, uint8_t* rgb, float* depth,
                   int32_t* segid, void*) {
  const double* ws = b->render_ws;
  const RLayers Y = render_layers(b, p, ws);
  std::vector<RItem> lds((size_t)p.nmax);
  std::vector<RHit> hits(MYO_RTILE * MYO_RTILE);
  std::vector<float> dirs(3 * MYO_RTILE * MYO_RTILE);
  const int tiles_x = (width + MYO_RTILE - 1) / MYO_RTILE, tiles_y = (height + MYO_RTILE - 1) / MYO_RTILE, nt = MYO_RTILE * MYO_RTILE;
  for (int e = 0; e < k; ++e) {
    const double* cam = ws + p.cams + (size_t)(ncams == 1 ? 0 : e) * MYO_RCAM_N;
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        const int tx0 = tx * MYO_RTILE, ty0 = ty * MYO_RTILE;
        auto PX = [&](int t) { return tx0 + t % MYO_RTILE; };
        auto PY = [&](int t) { return ty0 + t / MYO_RTILE; };
        if (!p.layered) {
          for (int t = 0; t < nt; ++t) render_stage(t, lds.data(), ws + (size_t)e * b->nitem * MYO_RENDER_ITEM_N, b->nitem, cam, flags);
          for (int t = 0; t < nt; ++t) render_cull(t, lds.data(), b->nitem, cam, width, height, tx0, ty0);
          for (int t = 0; t < nt; ++t) render_pixel(lds.data(), b->nitem, cam, width, height, PX(t), PY(t), flags, (size_t)e, rgb, depth, segid);
          continue;
        }
        for (int t = 0; t < nt; ++t) render_ray(cam, width, height, PX(t), PY(t), &dirs[3 * t], hits[t]);
        for (int j = 0, base = 0; j < Y.nl; base += Y.l[j++].n) {
          const int n = Y.l[j].n;
          for (int t = 0; t < nt; ++t) render_stage(t, lds.data(), Y.l[j].rows + (size_t)e * n * MYO_RENDER_ITEM_N, n, cam, flags, j == 0 ? Y.ngeom : 0, Y.geom_alpha);
          for (int t = 0; t < nt; ++t) render_cull(t, lds.data(), n, cam, width, height, tx0, ty0);
          for (int t = 0; t < nt; ++t) if (PX(t) < width && PY(t) < height) render_trace(lds.data(), n, base, &dirs[3 * t], hits[t]);
        }
        for (int t = 0; t < nt; ++t) render_layers_finish(Y, cam, width, height, PX(t), PY(t), flags, (size_t)e, hits[t], &dirs[3 * t], rgb, depth, segid);
      }
  }
  return MYO_OK;
}
