// emu_host.h — TEST TOOLING: the host side of the lane-serial emulation build (tests/emu/libmyobatch_emu.so = csrc/myobatch_emu.cpp).
// The kernel SOURCE (wave.h / myo_physics.h / myo_task.h, compiled with -DMYO_EMU: a phase's lanes run one after the other) is stepped
// env by env on the CPU, through the same records, layouts and task blocks as the product (csrc/myo_host.h), so that the wave-parallel
// algorithm can be checked against the oracle without a GPU.  It implements the env-path entry points of include/myobatch.h only;
// the PPO-side kernels have no CPU twin.  The renderer runs on what the product's runs on: the pass structs and per-thread functions of
// csrc/myo_render.h, and the plan, workspace layout and RLayers of csrc/myo_host.h (render_plan); only the loops over envs, tiles and
// threads are its own.  Nothing here is compiled into libmyobatch.so.
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
  void* w = nullptr;             // (emulation: one workspace per env)
  rc |= be_malloc(&w, sizeof(double) * (size_t)n_envs * MYO_ENVWS_N);
  b->K.ctrl_ws = (double*)w;
  if (w) b->allocs.push_back(w);
  if (b->ncap > MYO_NCON_MAX) {
    void* g = nullptr;
    rc |= be_malloc(&g, (size_t)n_envs * MYO_BIGWS_BYTES);
    b->K.big_ws = (char*)g;
    if (g) b->allocs.push_back(g);
  }
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
static int be_launch_status() { return MYO_OK; }
static void be_task_changed(myo_batch*) {}

// One zeroed scratch of the batch's kernel variant (with_variant, csrc/myo_host.h) with its RK4 stage block, handed together with the
// variant's model to f(model, scratch): what a workgroup has in LDS, here on the heap and used for one env after the other
template <typename F>
static void with_scratch(myo_batch* b, F&& f) {
  with_variant(b, [&](auto v) {
    using V = decltype(v);
    using T = typename V::T;
    Scratch<T, V::NC>* s = new Scratch<T, V::NC>();
    memset(s, 0, sizeof *s);
    RkScratch<T>* rk = new RkScratch<T>();
    s->rk = rk;
    if constexpr (sizeof(T) == sizeof(double)) f(b->Md, *s); else f(b->Mf, *s);
    delete s; delete rk;
  });
}
static double* env_rec(myo_batch* b, int env) { return b->rec + (size_t)env * b->L.stride; }

extern "C" int myo_batch_bind_constants(myo_batch* b, void*) { return batch_check(b); }
extern "C" int myo_batch_tune_wrap_order(myo_batch* b, void*) { return batch_check(b); }
extern "C" int myo_batch_set_step_generation(myo_batch* b, unsigned int) { return batch_check(b); }
extern "C" double myo_batch_kernel_ms(myo_batch*) { return -1.0; }
extern "C" int myo_debug_wave_slots(int, int n_workgroups, int lds_bytes, int32_t out[4]) {
  if (!out || n_workgroups <= 0 || lds_bytes < 0 || lds_bytes > 65536) return fail(MYO_E_ARG, "bad argument");
  return fail(MYO_E_UNSUPPORTED, "myo_debug_wave_slots: no wave slots in the emulation build");
}

extern "C" int myo_batch_reset(myo_batch* b, const uint8_t* mask, float* obs, void*) {
  if (int rc = reset_check(b)) return rc;
  with_scratch(b, [&](auto& M, auto& s) { for (int env = 0; env < b->n; ++env) env_reset(M, b->K, b->L, env_rec(b, env), s, env, mask, obs); });
  return MYO_OK;
}

extern "C" int myo_batch_step(myo_batch* b, const float* act, float* obs, float* rew, uint8_t* done, uint8_t* trunc,
                              float* term_obs, float* comps, float* ep_info, void*) {
  if (int rc = step_check(b, act, obs, rew, done)) return rc;
  // (the parts of the step plan one after the other, each through the env record like the workgroups of k_step)
  with_scratch(b, [&](auto& M, auto& s) {
    for (int p = 0; p < b->plan.nparts; ++p) {
      const int k_lo = b->plan.k[p], k_hi = p == b->plan.nparts - 1 ? -1 : b->plan.k[p + 1];
      for (int env = 0; env < b->n; ++env) env_step(M, b->K, b->L, env_rec(b, env), s, env, act, obs, rew, done, trunc, term_obs, comps, ep_info, b->bad_state, k_lo, k_hi);
    }
  });
  return MYO_OK;
}

extern "C" int myo_batch_health(myo_batch* b, int out[4]) {
  int empty = 0;
  int rc = health_check(b, out, &empty);
  if (rc || empty) return rc;
  memcpy(out, b->K.health, 4 * sizeof(int));
  return MYO_OK;
}

extern "C" int myo_batch_step_inner(myo_batch* b, const uint8_t* mask, const float* act, float* obs, uint8_t* done, void*) {
  if (int rc = step_inner_check(b, act, obs)) return rc;
  with_scratch(b, [&](auto& M, auto& s) { for (int env = 0; env < b->n; ++env) env_step_inner(M, b->K, b->L, env_rec(b, env), s, env, mask, act, obs, done); });
  return MYO_OK;
}

extern "C" int myo_batch_step_inner_idx(myo_batch* b, const int* idx, int n_idx, const float* act, float* obs, uint8_t* done, void*) {
  if (int rc = step_inner_idx_check(b, idx, n_idx, act, obs)) return rc;
  with_scratch(b, [&](auto& M, auto& s) {
    for (int r = 0; r < n_idx; ++r) {
      const int e = idx[r];
      if (e >= 0 && e < b->n) env_step_inner(M, b->K, b->L, env_rec(b, e), s, e, (const unsigned char*)nullptr, act, obs, done, r);
    }
  });
  return MYO_OK;
}

extern "C" int myo_batch_copy_envs(myo_batch* dst, const int* dst_idx, const myo_batch* src, const int* src_idx, int k, void*) {
  int empty = 0;
  int rc = copy_envs_check(dst, dst_idx, src, src_idx, k, &empty);
  if (rc || empty) return rc;
  for (int r = 0; r < k; ++r) {
    const int d = dst_idx[r], s = src_idx[r];
    if (d < 0 || d >= dst->n || s < 0 || s >= src->n) continue;
    memcpy(dst->rec + (size_t)d * dst->L.stride, src->rec + (size_t)s * src->L.stride, sizeof(double) * (size_t)dst->L.stride);
  }
  return MYO_OK;
}

extern "C" int myo_batch_physics_step(myo_batch* b, const double* ctrl, int nsub, void*) {
  if (int rc = physics_step_check(b, nsub)) return rc;
  with_scratch(b, [&](auto& M, auto& s) { for (int env = 0; env < b->n; ++env) env_physics(M, b->K, b->L, env_rec(b, env), s, env, ctrl, nsub); });
  return MYO_OK;
}

extern "C" int myo_batch_forward_dump(myo_batch* b, const double* ctrl, double* out, void*) {
  if (int rc = forward_dump_check(b, out)) return rc;
  with_scratch(b, [&](auto& M, auto& s) { for (int env = 0; env < b->n; ++env) env_forward_dump(M, b->K, b->L, env_rec(b, env), s, env, ctrl, b->D, out); });
  return MYO_OK;
}

extern "C" int myo_batch_sense(myo_batch* b, const myo_sense_out* out, void*) {
  if (int rc = sense_check(b, out)) return rc;
  const SenseDev O = sense_dev(b, out);
  with_scratch(b, [&](auto& M, auto& s) { for (int env = 0; env < b->n; ++env) env_sense(M, b->K, b->L, env_rec(b, env), s, env, O); });
  return MYO_OK;
}

// rendering: an item pass env by env (k_items) ...
template <typename Pass>
static void emu_items(myo_batch* b, const int32_t* env_idx, int k, const Pass& P, double* out) {
  with_scratch(b, [&](auto& M, auto& s) {
    for (int r = 0; r < k; ++r) {
      const int e = env_idx[r];
      double* o = out + (size_t)r * P.rows * MYO_RENDER_ITEM_N;
      if (e < 0 || e >= b->n) memset(o, 0, sizeof(double) * (size_t)P.rows * MYO_RENDER_ITEM_N);
      else pass_run(P, M, b->K, b->L, env_rec(b, e), s, e, r, o);
    }
  });
}
extern "C" int myo_batch_geom_poses(myo_batch* b, const int32_t* env_idx, int k, double* out, void*) {
  int rc = render_check_items(b, env_idx, k, "myo_batch_geom_poses");
  if (rc) return rc;
  if (!out) return fail(MYO_E_ARG, "myo_batch_geom_poses: null output");
  emu_items(b, env_idx, k, geom_pass(b), out);
  return MYO_OK;
}
extern "C" int myo_batch_tendon_paths(myo_batch* b, const int32_t* env_idx, int k, double* out, void*) {
  int rc = items_check(b, env_idx, k, out, "myo_batch_tendon_paths");
  if (rc || k == 0 || b->ntitem == 0) return rc;
  emu_items(b, env_idx, k, tendon_pass(b), out);
  return MYO_OK;
}
extern "C" int myo_batch_contact_items(myo_batch* b, const int32_t* env_idx, int k, double* out, void*) {
  int rc = items_check(b, env_idx, k, out, "myo_batch_contact_items");
  if (rc || k == 0) return rc;
  if ((rc = render_workspace(b, contact_tmp_doubles(b, k)))) return rc;
  emu_items(b, env_idx, k, contact_pass(b, k, b->render_ws), out);
  return MYO_OK;
}
// ... and the ray cast tile by tile, a kernel's thread phases (what lies between two barriers) one after the other, in the device's
// workspace layout (render_plan): the plain arm is k_render, the layered arm k_render_layers
extern "C" int myo_batch_render(myo_batch* b, const int32_t* env_idx, int k, const myo_render_camera* cams, int ncams, int width, int height,
                                int flags, uint8_t* rgb, float* depth, int32_t* segid, void*) {
  std::vector<double> cam_tab;
  int rc = render_check(b, env_idx, k, cams, ncams, width, height, flags, rgb, depth, segid, cam_tab);
  if (rc) return rc;
  const RenderPlan p = render_plan(b, k, flags, cam_tab.size());
  if ((rc = render_workspace(b, p.total))) return rc;
  double* ws = b->render_ws;
  memcpy(ws + p.cams, cam_tab.data(), cam_tab.size() * sizeof(double));
  emu_items(b, env_idx, k, geom_pass(b), ws);
  if (p.ntitem > 0) emu_items(b, env_idx, k, tendon_pass(b), ws + p.tendons);
  if (p.ncitem > 0) emu_items(b, env_idx, k, contact_pass(b, k, ws + p.tmp), ws + p.contacts);
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
