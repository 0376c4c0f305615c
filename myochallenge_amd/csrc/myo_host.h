// myo_host.h — the host side both builds of libmyobatch share: error reporting, the host model (blob -> tables), the batch
// (records, layouts, task block), myo_batch_create / _destroy, the kernel variant of a batch (with_variant) with its LDS footprint,
// and EVERY env-path entry point of include/myobatch.h: argument checks, plans and workspaces are written once, over the few backend
// primitives declared below (be_run: one job over the blocks of a launch; be_step; the ray cast; ...).  Included by csrc/myobatch.hip
// (the product: the HIP backend, the kernels, the PPO side) and by csrc/myobatch_emu.cpp (test tooling: csrc/emu_host.h runs the same
// kernel SOURCE lane by lane on the CPU).  The including file defines, before the include:
//   MYO_BACKEND_NAME             "gfx950" | "MYO_EMU lane-serial test build"   (myo_version)
//   MYO_BACKEND_DENSE_NEWTON     0 | 1: factor the Newton system densely (no block-arrow tables)
//   MYO_BACKEND_BATCH_FIELDS     members the backend keeps in struct myo_batch
//   MYO_BACKEND_RENDER_ENVS_MAX  envs one myo_batch_render call may list
//   struct DeviceGuard           DeviceGuard g(device): the device is current while g lives
// and, after it, the backend functions declared below.
#pragma once
#include "../../include/myobatch.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/myo_model_blob.h"
#include "myo_mjb.h"
#include "myo_task.h"
#include "myo_sense.h"
#include "myo_data.h"
#include "myo_jac.h"
#include "myo_static_opt.h"
#include "myo_ik.h"
#include "myo_simulate.h"
#include "myo_render.h"


// ------------------------------------------------------------------------------------------ backend (defined by the including file)
struct myo_batch;
struct myo_model;
static int be_malloc(void** p, size_t n);
static void be_free(void* p);
static int be_h2d(void* d, const void* h, size_t n);
static int be_set_device(int dev);
static const char* be_errstr(int e);
static int be_batch_workspaces(myo_batch* b, int n_envs, int device);                      // the fp64 stepper's workspaces (TaskDev::ctrl_ws / big_ws); returns error bits
static int be_batch_launch_state(myo_batch* b, const myo_model* m, int n_envs, int rc);    // what the launches need beside the records; returns rc | its own error bits
static void be_batch_release(myo_batch* b, int device, int destroying);                    // ... and their release (destroying = 0: a failed myo_batch_create)
// record gather / scatter: field [off, off + cnt) of every env's record <-> ext[n, cnt] (to_ext = 1: record -> ext); a null ext is skipped.
// `stream` is the ABI's (a hipStream_t, or unused)
static void be_xfer(myo_batch* b, int off, int cnt, double* ext, int to_ext, void* stream);
static void be_xfer_i(myo_batch* b, int off, int cnt, int* ext, int to_ext, void* stream);   // ... of a field that holds integers
static int be_capturing(void* stream);                                                       // 1 while `stream` records a graph (allocations and frees are not to happen then)
static int be_launch_status();                                                             // MYO_OK, or what became of the launches just issued (MYO_E_DEVICE)
static void be_task_changed(myo_batch* b);                                                 // the host's task block (b->K) changed: what was issued is waited for, the next launch uploads it again
// the launches of the env path (`stream` as above).  be_run: job J (csrc/myo_task.h) for blocks 0 .. nblocks - 1 of the batch's kernel
// variant, with the model and task constants bound; timed: between the batch's timing events when timing is on.  Returns the launch status.
template <typename Job> static int be_run(myo_batch* b, const Job& J, int nblocks, void* stream, int timed = 0);
static int be_step(myo_batch* b, const float* act, float* obs, float* rew, uint8_t* done, uint8_t* trunc, float* term_obs, float* comps,
                   float* ep_info, void* stream);                                          // one env step of every env, by the batch's step plan
static int be_bind(myo_batch* b, void* stream);                                            // the batch's constants become the device's
static int be_wrap_order(myo_batch* b, void* stream);                                      // census of the wraps, then their new order (a batch without wrap_cnt: nothing)
struct RenderPlan;
static int be_camera_upload(myo_batch* b, double* dst, std::vector<double>& cam_tab, void* stream);   // cam_tab -> dst; may keep cam_tab's storage (b->cam_host)
static int be_cast(myo_batch* b, const RenderPlan& p, int k, int ncams, int width, int height, int flags, uint8_t* rgb, float* depth,
                   int32_t* segid, void* stream);                                          // the ray cast over the plan's tables in b->render_ws
static int be_copy_envs(myo_batch* dst, const int* dst_idx, const myo_batch* src, const int* src_idx, int k, void* stream);
static int be_health(myo_batch* b, int out[4]);                                            // out <- b->K.health (waits for the device)
static int be_set_step_generation(myo_batch* b, unsigned int gen);
static double be_kernel_ms(myo_batch* b);
static int be_wave_slots(int device, int n_workgroups, int lds_bytes, int32_t out[4]);

static thread_local char g_err[4096] = "";      // (room for a loader report that lists every unsupported feature of a model)
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
extern "C" const char* myo_last_error(void) { return g_err; }
#ifndef MYO_BUILD_ID
#define MYO_BUILD_ID "unknown"
#endif
extern "C" const char* myo_version(void) {      // "... build <hash of the native sources>" (myochallenge_amd/build.py:source_id)
  return "myobatch 0.1 (" MYO_BACKEND_NAME ") build " MYO_BUILD_ID;
}

// ------------------------------------------------------------------------------------------ host model
// myo_model_from_blob is a sequence of stages on the model, in an order that is part of the contract: a blob with several defects is
// reported by the first stage that meets one.
//   read_fields          required fields (MYO_BLOB_*_FIELDS), optional fields with their defaults, sizes and options
//   check_untrusted      sizes, array lengths and every id, before anything is indexed with them
//   order_pairs          npair_std: primitive pairs first
//   check_capacity       the stepper's capacities and feature gates that need no derived table
//   build_tree_tables    body_depth .. dof_prevmask, dof_Madr / M_*, mv_*
//   build_wrap_records, build_path_elements, build_actuator_gather
//                        tendon_dofmask, wrap_side; wr_*, gw_elem; te_*, the staging-area limits; actuator_tendon, aq_*, act_*
//   build_muscle_constants   act_pre
//   build_lane_records   bk_*, jk_i, dk_i, dof_spr, dof_submask
//   build_pair_records   pc_*, pair_mg, any_rot, any_gen
//   build_frames         body_imat, geom_mat, nlead
//   resolve_solver_params    (solref, solimp) -> what sol_param reads, in place
//   build_ldl_tables, build_arrow_tables, set_feature_flags, render_vis_table, render_tendon_table
// A capacity check that guards a table sits in that table's builder, before the first write it guards.
struct myo_model {
  int nq, nv, nu, na, nbody, njnt, ngeom, nsite, ntendon, nwrap, npair, nM, maxdepth;
  int integrator, iterations, disableflags, any_damping, any_tendon_passive, nlead, ngw, nte, npair_std, ld_nfq, ld_nsq, arrow_nf, any_rot, any_gen, any_floss;
  unsigned long long arrow_pad;
  double timestep, tolerance, impratio, gravity[3], meaninertia;
#define X(n) std::vector<int> n;
  MYO_MODEL_INT_ARRAYS(X)
#undef X
#define X(n) std::vector<unsigned long long> n;
  MYO_MODEL_U64_ARRAYS(X)
#undef X
#define X(n) std::vector<double> n;
  MYO_MODEL_REAL_ARRAYS(X)
#undef X
  // rendering (csrc/myo_render.h): per item (ngeom geoms, then nsite sites) rgba[4], site radius, optional, 0, 0 (render_vis_table);
  // the free camera's default lookat / distance (myo_model_default_camera)
  std::vector<float> vis;
  int has_visual;
  // tendon items (myo_batch_tendon_paths; render_tendon_table): per tendon base rgba[4], radius, colouring activation (-1), 0, 0; per path
  // element its first item slot; the item slots per env (1 per site -> site element, 3 per element around a wrap geom)
  std::vector<float> tvis;
  std::vector<int> titem_adr;
  int ntendon_item;
  double cam_lookat[3], cam_distance;
};

static const myo_blob_field* blob_find(const void* blob, const char* name) {
  const myo_blob_header* h = (const myo_blob_header*)blob;
  const myo_blob_field* f = (const myo_blob_field*)((const char*)blob + sizeof(myo_blob_header));
  for (uint32_t i = 0; i < h->n_fields; ++i)
    if (strncmp(f[i].name, name, MYO_BLOB_NAME_LEN) == 0) return &f[i];
  return nullptr;
}
template <typename U>
static bool blob_get(const void* blob, size_t nbytes, const char* name, uint32_t dtype, std::vector<U>& out) {
  const myo_blob_field* f = blob_find(blob, name);
  if (!f || f->dtype != dtype || f->offset + (unsigned long long)sizeof(U) * f->count > nbytes) return false;
  const U* p = (const U*)((const char*)blob + f->offset);
  out.assign(p, p + f->count);
  return true;
}
static bool get_i(const void* blob, size_t nbytes, const char* name, std::vector<int>& out) { return blob_get(blob, nbytes, name, MYO_BLOB_I32, out); }
static bool get_d(const void* blob, size_t nbytes, const char* name, std::vector<double>& out) { return blob_get(blob, nbytes, name, MYO_BLOB_F64, out); }
static void quat2mat_h(const double* q, double* R) {
  double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
}

// Item tables of the level-parallel tree-sparse L'DL (csrc/myo_sparse_ldl.h; mj_factorM / mj_solveM order of operations per
// entry, scheduled by depth in the dof tree).  ld_fac word: e_ij | e_ki << 8 | e_kj << 16 | e_kk << 24 (indices into qM's
// dof_Madr layout) for  M[i,j] -= M[k,i] M[k,j] / M[k,k];  ld_sol word: e_ij | i << 8 | j << 16, j a strict ancestor of i.
// Levels deepest first, each padded to whole 64-item chunks with no-ops (e_ij = 255).  Rows >= nlead are diagonal by
// construction and get no items.  A tree that needs more chunks than the kernel preloads keeps the dense solves.
static void build_ldl_tables(myo_model* m) {
  const int nv = m->nv;
  std::vector<int> depth(nv, 0);
  int maxd = 0;
  for (int i = 0; i < nv; ++i) { depth[i] = m->dof_parentid[i] < 0 ? 0 : depth[m->dof_parentid[i]] + 1; if (depth[i] > maxd) maxd = depth[i]; }
  std::vector<int> fac, sol;
  const int nop = 255;
  for (int L = maxd; L >= 1; --L) {
    size_t f0 = fac.size(), s0 = sol.size();
    for (int k = 0; k < nv && k < m->nlead; ++k) {
      if (depth[k] != L) continue;
      std::vector<int> anc;                               // strict ancestors of k, nearest first
      for (int a = m->dof_parentid[k]; a >= 0; a = m->dof_parentid[a]) anc.push_back(a);
      const int ek = m->dof_Madr[k];
      for (size_t p = 0; p < anc.size(); ++p) {
        sol.push_back((ek + 1 + (int)p) | (k << 8) | (anc[p] << 16));
        for (size_t q = p; q < anc.size(); ++q)           // i = anc[p], j = anc[q] (j = i or an ancestor of i)
          fac.push_back((m->dof_Madr[anc[p]] + (int)(q - p)) | ((ek + 1 + (int)p) << 8) | ((ek + 1 + (int)q) << 16) | (ek << 24));
      }
    }
    if (fac.size() > f0) while (fac.size() % 64) fac.push_back(nop);
    if (sol.size() > s0) while (sol.size() % 64) sol.push_back(nop);
  }
  m->ld_nfq = (int)fac.size() / 64; m->ld_nsq = (int)sol.size() / 64;
  if (m->ld_nfq > MYO_LD_FQ || m->ld_nsq > MYO_LD_SQ || m->nM >= nop || getenv("MYO_DENSE_MSOLVE")) { m->ld_nfq = 0; m->ld_nsq = -1; fac.clear(); sol.clear(); }   // ld_nsq < 0: dense
  fac.resize((size_t)MYO_LD_FQ * 64, nop); sol.resize((size_t)MYO_LD_SQ * 64, nop);
  m->ld_fac = fac; m->ld_sol = sol;
}

// Block-arrow structure of the Newton system H = M + J'DJ (csrc/myo_arrow_chol.h).  Leaf blocks: subtrees of the dof tree with at
// most MYO_ARROW_B dofs that no constraint couples to another block — M couples a dof with its ancestors and descendants only, a
// tendon-limit row couples the dofs its tendon moves, a contact the dofs that move either body (the hand: five 4-dof fingers; the
// wrist and the free balls / die couple everything and form the separator).  hperm[dof] = row of the permuted system: separator
// rows 0..15, block f at 16 + 4 f; rows without a dof are identity (arrow_pad).  M_pkh[e] = packed-H offset of M's entry e in that
// order.  arrow_nf = 0 (structure absent, separator too large, MYO_DENSE_NEWTON set, emulation build): identity order, dense path.
static void build_arrow_tables(myo_model* m) {
  const int nv = m->nv;
  m->hperm.assign(MYO_NV_MAX, 0);
  for (int d = 0; d < MYO_NV_MAX; ++d) m->hperm[d] = d;
  m->arrow_nf = 0; m->arrow_pad = 0;
  auto finish = [&]() {
    m->M_pkh.assign(MYO_NM_MAX, 0);
    for (int e = 0; e < m->nM; ++e) {
      const int a = m->hperm[m->M_i[e]], b = m->hperm[m->M_j[e]], hi = a > b ? a : b, lo = a > b ? b : a;
      const int q = hi >> 2;
      m->M_pkh[e] = ((q * (q + 1)) << 3) + (((hi & 3) * (q + 1)) << 2) + lo;      // MYO_HIDX(hi, lo)
    }
    if (!m->arrow_nf) for (int d = nv; d < MYO_NV_MAX; ++d) m->arrow_pad |= 1ull << d;
  };
  if (MYO_BACKEND_DENSE_NEWTON) { finish(); return; }      // (the lane-serial emulation factors H densely: no MFMA there)
  if (getenv("MYO_DENSE_NEWTON") || nv > MYO_NV_MAX) { finish(); return; }
  // subtree sizes; candidate blocks = maximal subtrees of <= MYO_ARROW_B dofs
  std::vector<int> size(nv, 1), block(nv, -1);
  for (int d = nv - 1; d >= 0; --d) if (m->dof_parentid[d] >= 0) size[m->dof_parentid[d]] += size[d];
  std::vector<std::vector<int>> blocks;
  for (int d = 0; d < nv; ++d) {
    const int par = m->dof_parentid[d];
    if (size[d] <= MYO_ARROW_B && (par < 0 || size[par] > MYO_ARROW_B)) {
      std::vector<int> mem;
      for (int e = d; e < nv; ++e) { int a = e; while (a >= 0 && a != d) a = m->dof_parentid[a]; if (a == d) { mem.push_back(e); block[e] = (int)blocks.size(); } }
      blocks.push_back(mem);
    }
  }
  // constraint couplings between blocks; the most-coupled block goes to the separator until none is left (a free ball's
  // trailing dofs form a candidate block that every finger touches: it goes, the fingers stay)
  std::vector<unsigned long long> sets;
  for (int t = 0; t < m->ntendon; ++t) sets.push_back(m->tendon_dofmask[t]);
  for (int p = 0; p < m->npair; ++p) sets.push_back(m->pc_mask[2 * (size_t)p] | m->pc_mask[2 * (size_t)p + 1]);
  const size_t nblk = blocks.size();
  std::vector<std::vector<char>> adj(nblk, std::vector<char>(nblk, 0));
  for (unsigned long long mk : sets) {
    std::vector<int> bs;
    for (int d = 0; d < nv; ++d) if (((mk >> d) & 1ull) && block[d] >= 0 && std::find(bs.begin(), bs.end(), block[d]) == bs.end()) bs.push_back(block[d]);
    for (int a : bs) for (int b : bs) if (a != b) adj[a][b] = 1;
  }
  std::vector<char> demote(nblk, 0);
  for (;;) {
    int worst = -1, wdeg = 0;
    for (size_t a = 0; a < nblk; ++a) {
      if (demote[a]) continue;
      int deg = 0;
      for (size_t b = 0; b < nblk; ++b) if (!demote[b] && adj[a][b]) deg++;
      if (deg > wdeg) { wdeg = deg; worst = (int)a; }
    }
    if (worst < 0) break;
    demote[worst] = 1;
  }
  // keep the largest blocks (at most MYO_ARROW_NF); everything else is separator
  std::vector<int> keep;
  for (size_t b = 0; b < blocks.size(); ++b) if (!demote[b]) keep.push_back((int)b);
  std::stable_sort(keep.begin(), keep.end(), [&](int a, int b) { return blocks[a].size() > blocks[b].size(); });
  if ((int)keep.size() > MYO_ARROW_NF) keep.resize(MYO_ARROW_NF);
  std::vector<char> in_keep(blocks.size(), 0);
  for (int b : keep) in_keep[b] = 1;
  int nsep = 0;
  for (int d = 0; d < nv; ++d) if (block[d] < 0 || !in_keep[block[d]]) nsep++;
  if (keep.size() < 2 || nsep > MYO_ARROW_S) { finish(); return; }
  std::sort(keep.begin(), keep.end());
  unsigned long long used = 0;
  int ns = 0;
  for (int d = 0; d < nv; ++d) if (block[d] < 0 || !in_keep[block[d]]) { m->hperm[d] = ns; used |= 1ull << ns; ns++; }
  for (size_t f = 0; f < keep.size(); ++f)
    for (size_t t = 0; t < blocks[keep[f]].size(); ++t) { const int r = MYO_ARROW_S + MYO_ARROW_B * (int)f + (int)t; m->hperm[blocks[keep[f]][t]] = r; used |= 1ull << r; }
  m->arrow_nf = (int)keep.size();
  m->arrow_pad = ~used & ((1ull << MYO_NV_MAX) - 1ull);
  finish();
}

// what sol_param (myo_physics.h) needs of a (solref[2], solimp[5]) pair, resolved once: ref2 <- (K, B) with refsafe applied; imp5 <- (d0, d1,
// 1 / width — 0 when the impedance does not depend on the position —, midpoint, power), clamped as MuJoCo's getsolparam / getimpedance clamp them
static void sol_precompute(double* ref2, double* imp5, double timestep, int disableflags) {
  auto clamp = [](double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); };
  const double d0 = clamp(imp5[0], 0.0001, 0.9999), d1 = clamp(imp5[1], 0.0001, 0.9999);
  const double width = imp5[2] < 0 ? 0.0 : imp5[2];
  const double mid = clamp(imp5[3], 0.0001, 0.9999), power = imp5[4] < 1 ? 1.0 : imp5[4];
  double tc = ref2[0];
  const double dr = ref2[1];
  double K, B;
  if (tc > 0) {
    if (!(disableflags & (1 << 11)) && tc < 2 * timestep) tc = 2 * timestep;
    K = 1.0 / std::max(1e-15, d1 * d1 * tc * tc * dr * dr);
    B = 2.0 / std::max(1e-15, d1 * tc);
  } else { K = -tc / (d1 * d1); B = -dr / d1; }
  ref2[0] = K; ref2[1] = B;
  imp5[0] = d0; imp5[1] = d1; imp5[2] = (d0 == d1 || width <= 1e-15) ? 0.0 : 1.0 / width; imp5[3] = mid; imp5[4] = power;
}

// Visual table of the render items and the default camera (include/myobatch.h, myo_batch_render).  With geom_rgba in the blob (a real
// .mjb: both model routes carry geom_rgba / geom_group / geom_matid / mat_rgba / site_rgba / site_size / site_group / stat): MuJoCo's rule,
// groups 0-2 and alpha > 0 are drawn, mat_rgba where matid >= 0.  Without it (the synthetic models) the colours are derived: colliding
// geoms skin, the geoms of free-joint bodies one palette colour per body, non-colliding geoms of a body welded to the world translucent
// (the die's target), wrap-only geoms (non-colliding, named by a sphere / cylinder wrap) hidden.  Sites are optional (drawn with
// MYO_RENDER_SITES) and grey, 5 mm.  Default camera: lookat = stat.center, distance = 1.5 stat.extent; without stat, the bounding
// sphere (centre c, radius r) of the drawn geoms at qpos0 (the body_pos / body_quat chain) with extent = 2 r.
// Visual table of the tendon items (include/myobatch.h, myo_batch_tendon_paths).  With visual data in the blob: radius tendon_width,
// colour tendon_rgba (mat_rgba where tendon_matid >= 0), groups 0-2 and alpha > 0 drawn.  Without it: MYO_RTEN_RADIUS and MYO_RTEN_BASE_*.
// A tendon that is the transmission target of a muscle actuator (dyntype muscle, with an activation state; the first such actuator) is
// coloured by that activation.  Called after render_vis_table (has_visual).
#define MYO_RTEN_RADIUS 0.002f
#define MYO_RTEN_BASE_R 0.30f
#define MYO_RTEN_BASE_G 0.35f
#define MYO_RTEN_BASE_B 0.75f
// (the stepper's capacity — path elements that fit the length staging, wrap geoms of the big workspace — keeps every model that loads
// within the renderer's second LDS pass; render_check still refuses, never truncates)
static_assert((MYO_H_SIZE - MYO_NB_MAX * 10) * sizeof(float) / sizeof(double) + 2 * MYO_BIGWS_GW <= MYO_RTEN_MAX, "tendon items of a loadable model fit MYO_RTEN_MAX");
static void render_tendon_table(myo_model* m, const void* blob, size_t nbytes, const std::vector<int>& trntype) {
  const int nt = m->ntendon;
  m->tvis.assign(8 * (size_t)(nt > 0 ? nt : 1), 0.f);
  std::vector<double> trgba, twidth, mrgba;
  std::vector<int> tgroup, tmat;
  const bool vt = m->has_visual && get_d(blob, nbytes, "tendon_rgba", trgba) && trgba.size() == 4 * (size_t)nt &&
                  get_d(blob, nbytes, "tendon_width", twidth) && twidth.size() == (size_t)nt;
  if (vt) get_d(blob, nbytes, "mat_rgba", mrgba);
  const bool tg = vt && get_i(blob, nbytes, "tendon_group", tgroup) && tgroup.size() == (size_t)nt;
  const bool tm = vt && get_i(blob, nbytes, "tendon_matid", tmat) && tmat.size() == (size_t)nt;
  for (int t = 0; t < nt; ++t) {
    float* v = &m->tvis[8 * (size_t)t];
    if (vt) {
      const double* c = &trgba[4 * (size_t)t];
      const int mid = tm ? tmat[t] : -1;
      if (mid >= 0 && 4 * (size_t)mid + 4 <= mrgba.size()) c = &mrgba[4 * (size_t)mid];
      for (int k = 0; k < 4; ++k) v[k] = (float)c[k];
      if (tg && (tgroup[t] < 0 || tgroup[t] > 2)) v[3] = 0.f;
      v[4] = (float)twidth[t];
    } else { v[0] = MYO_RTEN_BASE_R; v[1] = MYO_RTEN_BASE_G; v[2] = MYO_RTEN_BASE_B; v[3] = 1.f; v[4] = MYO_RTEN_RADIUS; }
    v[5] = -1.f;
  }
  for (int i = m->nu - 1; i >= 0; --i) {      // (descending: the first muscle of a tendon wins)
    const int ia = i - (m->nu - m->na), t = m->actuator_tendon[i];
    if (ia >= 0 && m->actuator_dyntype[i] == 3 && (size_t)i < trntype.size() && trntype[i] == MYO_TRN_TENDON && t >= 0 && t < nt) m->tvis[8 * (size_t)t + 5] = (float)ia;
  }
  m->titem_adr.assign(m->nte > 0 ? m->nte : 1, 0);
  int n = 0;
  for (int e = 0; e < m->nte; ++e) { m->titem_adr[e] = n; n += m->te_i[4 * (size_t)e + 2] >= 0 ? 3 : 1; }
  m->ntendon_item = n;
}
static void render_vis_table(myo_model* m, const void* blob, size_t nbytes) {
  const int ng = m->ngeom, ns = m->nsite;
  m->vis.assign(8 * (size_t)(ng + ns), 0.f);
  std::vector<double> grgba, mrgba, srgba, ssize, stat;
  std::vector<int> ggroup, gmat, sgroup, contype, conaff, weld;
  m->has_visual = get_d(blob, nbytes, "geom_rgba", grgba) && grgba.size() == 4 * (size_t)ng;
  const bool ok_i = get_i(blob, nbytes, "geom_contype", contype) && get_i(blob, nbytes, "geom_conaffinity", conaff) &&
                    get_i(blob, nbytes, "body_weldid", weld) && contype.size() == (size_t)ng && conaff.size() == (size_t)ng &&
                    weld.size() == (size_t)m->nbody;
  if (m->has_visual) {
    get_d(blob, nbytes, "mat_rgba", mrgba);
    const bool gg = get_i(blob, nbytes, "geom_group", ggroup) && ggroup.size() == (size_t)ng;
    const bool gm = get_i(blob, nbytes, "geom_matid", gmat) && gmat.size() == (size_t)ng;
    for (int g = 0; g < ng; ++g) {
      const double* c = &grgba[4 * (size_t)g];
      const int mid = gm ? gmat[g] : -1;
      if (mid >= 0 && 4 * (size_t)mid + 4 <= mrgba.size()) c = &mrgba[4 * (size_t)mid];
      const int grp = gg ? ggroup[g] : 0;
      for (int k = 0; k < 4; ++k) m->vis[8 * (size_t)g + k] = (float)c[k];
      if (grp < 0 || grp > 2) m->vis[8 * (size_t)g + 3] = 0.f;
    }
  } else {
    static const float pal[4][3] = {{0.85f, 0.25f, 0.2f}, {0.2f, 0.45f, 0.85f}, {0.9f, 0.75f, 0.2f}, {0.35f, 0.7f, 0.35f}};
    std::vector<int> wrap_geom(ng, 0), free_ord(m->nbody, -1);
    for (int w = 0; w < m->nwrap; ++w)
      if ((m->wrap_type[w] == MYO_WRAP_SPHERE || m->wrap_type[w] == MYO_WRAP_CYLINDER) && m->wrap_objid[w] >= 0 && m->wrap_objid[w] < ng) wrap_geom[m->wrap_objid[w]] = 1;
    int nfree = 0;
    for (int b = 0; b < m->nbody; ++b)
      if (m->body_jntnum[b] > 0 && m->jnt_type[m->body_jntadr[b]] == MYO_JNT_FREE) free_ord[b] = nfree++;
    for (int g = 0; g < ng; ++g) {
      float* v = &m->vis[8 * (size_t)g];
      const int b = m->geom_bodyid[g];
      const bool coll = ok_i && (contype[g] != 0 || conaff[g] != 0);
      int root = b;
      while (root > 0 && free_ord[root] < 0) root = m->body_parentid[root];
      float c[4] = {0.8f, 0.62f, 0.52f, 1.f};                                    // skin
      if (root > 0 && free_ord[root] >= 0) { for (int k = 0; k < 3; ++k) c[k] = pal[free_ord[root] % 4][k]; }
      else if (!coll && wrap_geom[g]) c[3] = 0.f;                                 // wrap-only
      else if (!coll && ok_i && weld[b] == 0) { c[0] = 0.3f; c[1] = 0.85f; c[2] = 0.4f; c[3] = 0.35f; }      // translucent marker
      for (int k = 0; k < 4; ++k) v[k] = c[k];
    }
  }
  {
    const bool vs = m->has_visual && get_d(blob, nbytes, "site_rgba", srgba) && srgba.size() == 4 * (size_t)ns;
    const bool vz = get_d(blob, nbytes, "site_size", ssize) && ssize.size() == 3 * (size_t)ns;
    const bool vg = get_i(blob, nbytes, "site_group", sgroup) && sgroup.size() == (size_t)ns;
    for (int j = 0; j < ns; ++j) {
      float* v = &m->vis[8 * (size_t)(ng + j)];
      for (int k = 0; k < 4; ++k) v[k] = vs ? (float)srgba[4 * (size_t)j + k] : (k == 3 ? 1.f : 0.5f);
      if (vg && (sgroup[j] < 0 || sgroup[j] > 2)) v[3] = 0.f;
      v[4] = vz ? (float)ssize[3 * (size_t)j] : 0.005f;
      v[5] = 1.f;
    }
  }
  if (get_d(blob, nbytes, "stat", stat) && stat.size() == 4 && stat[3] > 0) {
    for (int k = 0; k < 3; ++k) m->cam_lookat[k] = stat[k];
    m->cam_distance = 1.5 * stat[3];
    return;
  }
  std::vector<double> xp(3 * (size_t)m->nbody, 0.0), xm(9 * (size_t)m->nbody, 0.0);
  xm[0] = xm[4] = xm[8] = 1;
  for (int b = 1; b < m->nbody; ++b) {
    const int p = m->body_parentid[b];
    double Rl[9], R[9];
    quat2mat_h(&m->body_quat[4 * (size_t)b], Rl);
    for (int i = 0; i < 3; ++i) {
      double t = 0;
      for (int k = 0; k < 3; ++k) t += xm[9 * (size_t)p + 3 * i + k] * m->body_pos[3 * (size_t)b + k];
      xp[3 * (size_t)b + i] = xp[3 * (size_t)p + i] + t;
      for (int j = 0; j < 3; ++j) { double u = 0; for (int k = 0; k < 3; ++k) u += xm[9 * (size_t)p + 3 * i + k] * Rl[3 * k + j]; R[3 * i + j] = u; }
    }
    for (int k = 0; k < 9; ++k) xm[9 * (size_t)b + k] = R[k];
  }
  std::vector<double> gp;
  std::vector<double> gr;
  for (int g = 0; g < ng; ++g) {
    if (m->vis[8 * (size_t)g + 3] <= 0.f || m->geom_type[g] == MYO_GEOM_PLANE) continue;
    const int b = m->geom_bodyid[g];
    for (int i = 0; i < 3; ++i) {
      double t = xp[3 * (size_t)b + i];
      for (int k = 0; k < 3; ++k) t += xm[9 * (size_t)b + 3 * i + k] * m->geom_pos[3 * (size_t)g + k];
      gp.push_back(t);
    }
    gr.push_back(m->geom_rbound[g]);
  }
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, r = 0;
  for (size_t i = 0; i < gr.size(); ++i)
    for (int k = 0; k < 3; ++k) {
      lo[k] = i ? std::min(lo[k], gp[3 * i + k] - gr[i]) : gp[3 * i + k] - gr[i];
      hi[k] = i ? std::max(hi[k], gp[3 * i + k] + gr[i]) : gp[3 * i + k] + gr[i];
    }
  for (int k = 0; k < 3; ++k) m->cam_lookat[k] = 0.5 * (lo[k] + hi[k]);
  for (size_t i = 0; i < gr.size(); ++i) {
    double d2 = 0;
    for (int k = 0; k < 3; ++k) d2 += (gp[3 * i + k] - m->cam_lookat[k]) * (gp[3 * i + k] - m->cam_lookat[k]);
    r = std::max(r, sqrt(d2) + gr[i]);
  }
  m->cam_distance = 1.5 * 2.0 * (r > 0 ? r : 1.0);
}

// ---- the loader's stages (the list at the head of this file)
// The required blob fields that the model keeps under their own name: X(name, least number of elements), the counts in terms of
// check_untrusted's nq_ .. nu_.  read_fields and check_untrusted's length check both expand from these two lists.
#define MYO_BLOB_INT_FIELDS(X)                                                                                                  \
  X(body_parentid, nb_) X(body_rootid, nb_) X(body_jntnum, nb_) X(body_jntadr, nb_) X(body_dofnum, nb_) X(body_dofadr, nb_)      \
  X(jnt_type, nj_) X(jnt_qposadr, nj_) X(jnt_dofadr, nj_) X(jnt_bodyid, nj_) X(jnt_limited, nj_)                                 \
  X(dof_bodyid, nv_) X(dof_jntid, nv_) X(dof_parentid, nv_) X(geom_type, ng_) X(geom_bodyid, ng_) X(geom_priority, ng_)          \
  X(site_bodyid, ns_) X(tendon_adr, nt_) X(tendon_num, nt_) X(tendon_limited, nt_) X(wrap_type, nw_) X(wrap_objid, nw_)          \
  X(actuator_dyntype, nu_) X(actuator_gaintype, nu_) X(actuator_biastype, nu_) X(actuator_ctrllimited, nu_) X(actuator_forcelimited, nu_)
#define MYO_BLOB_REAL_FIELDS(X)                                                                                                 \
  X(qpos0, nq_) X(qpos_spring, nq_) X(body_pos, 3 * nb_) X(body_quat, 4 * nb_) X(body_ipos, 3 * nb_) X(body_mass, nb_)           \
  X(body_inertia, 3 * nb_) X(body_invweight0, 2 * nb_) X(jnt_solref, 2 * nj_) X(jnt_solimp, 5 * nj_) X(jnt_pos, 3 * nj_)         \
  X(jnt_axis, 3 * nj_) X(jnt_stiffness, nj_) X(jnt_range, 2 * nj_) X(jnt_margin, nj_) X(dof_armature, nv_) X(dof_damping, nv_)   \
  X(dof_invweight0, nv_) X(geom_solmix, ng_) X(geom_solref, 2 * ng_) X(geom_solimp, 5 * ng_) X(geom_size, 3 * ng_)               \
  X(geom_rbound, ng_) X(geom_pos, 3 * ng_) X(geom_friction, 3 * ng_) X(geom_margin, ng_) X(geom_gap, ng_) X(site_pos, 3 * ns_)   \
  X(tendon_solref_lim, 2 * nt_) X(tendon_solimp_lim, 5 * nt_) X(tendon_range, 2 * nt_) X(tendon_margin, nt_) X(tendon_stiffness, nt_) \
  X(tendon_damping, nt_) X(tendon_lengthspring, nt_) X(tendon_invweight0, nt_) X(wrap_prm, nw_) X(actuator_dynprm, 10 * nu_)     \
  X(actuator_gainprm, 10 * nu_) X(actuator_biasprm, 10 * nu_) X(actuator_ctrlrange, 2 * nu_) X(actuator_forcerange, 2 * nu_)     \
  X(actuator_gear, 6 * nu_) X(actuator_acc0, nu_) X(actuator_lengthrange, 2 * nu_)

// blob arrays that the table builders read and the model does not keep
struct BlobOnly {
  std::vector<int> trntype, trnid, geom_condim, pair_sub, pair_xp, xp_dim;
  std::vector<double> body_iquat, geom_quat, xp_margin, xp_gap, xp_solref, xp_solimp, xp_friction;
};

static int corrupt(const char* fmt, ...) {
  char why[160] = "";
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(why, sizeof why, fmt, ap);
  va_end(ap);
  return fail(MYO_E_ARG, "corrupt model: %s", why);
}
static int over_capacity(const char* what) { return fail(MYO_E_UNSUPPORTED, "model exceeds stepper capacity: %s", what); }
static int popcount64(unsigned long long x) { return __builtin_popcountll(x); }
// entry k of a row of 16-bit entries, two per word (the even entry in the low half); the row starts out zeroed
static void pack16(int* row, int k, unsigned ent) {
  unsigned& w = reinterpret_cast<unsigned&>(row[k / 2]);
  w |= (k & 1) ? (ent << 16) : ent;
}

static int read_fields(const void* blob, size_t nbytes, myo_model& m, BlobOnly& x) {
  std::vector<int> sizes, opt_i;
  std::vector<double> opt_d;
  bool ok = get_i(blob, nbytes, "sizes", sizes) && sizes.size() >= 10 && get_i(blob, nbytes, "opt_int", opt_i) &&
            opt_i.size() >= 4 && get_d(blob, nbytes, "opt_f64", opt_d) && opt_d.size() >= 8;
  const char* missing = nullptr;
#define X(n, cnt) if (ok && !get_i(blob, nbytes, #n, m.n)) { ok = false; missing = #n; }
  MYO_BLOB_INT_FIELDS(X)
#undef X
#define X(n, cnt) if (ok && !get_d(blob, nbytes, #n, m.n)) { ok = false; missing = #n; }
  MYO_BLOB_REAL_FIELDS(X)
#undef X
  if (ok) ok = get_i(blob, nbytes, "actuator_trntype", x.trntype) && get_i(blob, nbytes, "actuator_trnid", x.trnid) &&
               get_d(blob, nbytes, "body_iquat", x.body_iquat) && get_d(blob, nbytes, "geom_quat", x.geom_quat) &&
               get_i(blob, nbytes, "x_pair_geom1", m.pair_geom1) && get_i(blob, nbytes, "x_pair_geom2", m.pair_geom2);
  if (!ok) return fail(MYO_E_ARG, "model blob lacks field %s", missing ? missing : "(sizes/opt/derived)");
  if (!get_i(blob, nbytes, "x_pair_sub", x.pair_sub)) x.pair_sub.assign(m.pair_geom1.size(), 0);      // (older blobs: no box-box candidates)
  if (!get_i(blob, nbytes, "geom_condim", x.geom_condim)) x.geom_condim.clear();                        // (older blobs: condim 3 everywhere)
  // explicit <contact><pair> parameters (older blobs: none)
  if (!get_i(blob, nbytes, "x_pair_explicit", x.pair_xp) || x.pair_xp.size() != m.pair_geom1.size()) x.pair_xp.assign(m.pair_geom1.size(), -1);
  const bool have = get_i(blob, nbytes, "x_xp_dim", x.xp_dim) && get_d(blob, nbytes, "x_xp_margin", x.xp_margin) && get_d(blob, nbytes, "x_xp_gap", x.xp_gap) &&
                    get_d(blob, nbytes, "x_xp_solref", x.xp_solref) && get_d(blob, nbytes, "x_xp_solimp", x.xp_solimp) && get_d(blob, nbytes, "x_xp_friction", x.xp_friction);
  const size_t nx = have ? x.xp_dim.size() : 0;
  if (have && (x.xp_margin.size() != nx || x.xp_gap.size() != nx || x.xp_solref.size() != 2 * nx || x.xp_solimp.size() != 5 * nx || x.xp_friction.size() != 3 * nx))
    return fail(MYO_E_ARG, "corrupt model: explicit contact pair arrays differ in length");
  for (int v : x.pair_xp) if (v < -1 || v >= (int)nx) return fail(MYO_E_ARG, "corrupt model: explicit contact pair index %d", v);
  // friction loss: optional fields (older blobs: none), MuJoCo's default solver parameters
  const size_t nv0 = sizes[1] > 0 && sizes[1] <= 4096 ? sizes[1] : 0, nt0 = sizes[8] > 0 && sizes[8] <= 4096 ? sizes[8] : 0;     // (untrusted sizes: capacity checks follow)
  auto opt = [&](const char* name, std::vector<double>& v, size_t cnt, std::initializer_list<double> def) {
    if (!get_d(blob, nbytes, name, v) || v.size() < cnt * def.size()) { v.clear(); for (size_t i = 0; i < cnt; ++i) v.insert(v.end(), def); }
  };
  opt("dof_frictionloss", m.dof_frictionloss, nv0, {0.0}); opt("dof_solref", m.dof_solref, nv0, {0.02, 1.0});
  opt("dof_solimp", m.dof_solimp, nv0, {0.9, 0.95, 0.001, 0.5, 2.0});
  opt("tendon_frictionloss", m.tendon_frictionloss, nt0, {0.0}); opt("tendon_solref_fri", m.tendon_solref_fri, nt0, {0.02, 1.0});
  opt("tendon_solimp_fri", m.tendon_solimp_fri, nt0, {0.9, 0.95, 0.001, 0.5, 2.0});
  m.nq = sizes[0]; m.nv = sizes[1]; m.nu = sizes[2]; m.na = sizes[3]; m.nbody = sizes[4]; m.njnt = sizes[5];
  m.ngeom = sizes[6]; m.nsite = sizes[7]; m.ntendon = sizes[8]; m.nwrap = sizes[9];
  m.npair = (int)m.pair_geom1.size();
  m.npair_std = 0;
  m.integrator = opt_i[0]; m.iterations = opt_i[2]; m.disableflags = opt_i[3];
  m.timestep = opt_d[0]; m.tolerance = opt_d[1]; m.impratio = opt_d[2];
  m.gravity[0] = opt_d[3]; m.gravity[1] = opt_d[4]; m.gravity[2] = opt_d[5]; m.meaninertia = opt_d[7];
  for (int k = 0; k < 10; ++k) if (sizes[k] < 0) return corrupt("negative size %d", k);
  return MYO_OK;
}

// ---- the blob is untrusted input: sizes, array lengths and every id are checked before anything is indexed with them
static int check_untrusted(const myo_model& m, BlobOnly& x) {
  if (m.nbody < 1 || m.na > m.nu) return corrupt("nbody < 1 or na > nu");
  if (m.pair_geom1.size() != m.pair_geom2.size() || x.pair_sub.size() != m.pair_geom1.size()) return corrupt("pair arrays differ in length");
  for (int v : x.pair_sub) if (v < 0 || v > 17) return corrupt("collision pair sub-index %d", v);
  const size_t nq_ = m.nq, nb_ = m.nbody, nj_ = m.njnt, nv_ = m.nv, ng_ = m.ngeom, ns_ = m.nsite, nt_ = m.ntendon, nw_ = m.nwrap, nu_ = m.nu;
  const char* short_arr = nullptr;
  size_t has = 0, needs = 0;
#define X(n, cnt) if (!short_arr && m.n.size() < (size_t)(cnt)) { short_arr = #n; has = m.n.size(); needs = (size_t)(cnt); }
  MYO_BLOB_INT_FIELDS(X) MYO_BLOB_REAL_FIELDS(X)
#undef X
  if (short_arr) return corrupt("array %s has %zu entries, needs %zu", short_arr, has, needs);
  if (x.geom_condim.empty()) x.geom_condim.assign(ng_, 3);
  if (x.geom_condim.size() < ng_) return corrupt("geom_condim too short");
  if (x.trntype.size() < nu_ || x.trnid.size() < 2 * nu_ || x.body_iquat.size() < 4 * nb_ || x.geom_quat.size() < 4 * ng_) return corrupt("actuator_trn* / body_iquat / geom_quat too short");
  if (m.body_parentid[0] != 0) return corrupt("body_parentid[0] != 0");
  for (int b = 0; b < m.nbody; ++b) {
    if (b > 0 && (m.body_parentid[b] < 0 || m.body_parentid[b] >= b)) return corrupt("body_parentid[%d] = %d", b, m.body_parentid[b]);
    if (m.body_rootid[b] < 0 || m.body_rootid[b] >= m.nbody) return corrupt("body_rootid[%d] = %d", b, m.body_rootid[b]);
    const int jn = m.body_jntnum[b], ja = m.body_jntadr[b], dn = m.body_dofnum[b], da = m.body_dofadr[b];
    if (jn < 0 || (jn > 0 && (ja < 0 || ja > m.njnt || jn > m.njnt - ja))) return corrupt("body_jntadr/num[%d] = %d/%d", b, ja, jn);
    if (dn < 0 || (dn > 0 && (da < 0 || da > m.nv || dn > m.nv - da))) return corrupt("body_dofadr/num[%d] = %d/%d", b, da, dn);
  }
  for (int j = 0; j < m.njnt; ++j) {
    const int ty = m.jnt_type[j], nqj = ty == MYO_JNT_FREE ? 7 : (ty == MYO_JNT_BALL ? 4 : 1), nvj = ty == MYO_JNT_FREE ? 6 : (ty == MYO_JNT_BALL ? 3 : 1);
    if (ty < 0 || ty > 3) return corrupt("jnt_type[%d] = %d", j, ty);
    if (m.jnt_qposadr[j] < 0 || m.jnt_qposadr[j] > m.nq - nqj) return corrupt("jnt_qposadr[%d] = %d", j, m.jnt_qposadr[j]);
    if (m.jnt_dofadr[j] < 0 || m.jnt_dofadr[j] > m.nv - nvj) return corrupt("jnt_dofadr[%d] = %d", j, m.jnt_dofadr[j]);
    if (m.jnt_bodyid[j] < 0 || m.jnt_bodyid[j] >= m.nbody) return corrupt("jnt_bodyid[%d] = %d", j, m.jnt_bodyid[j]);
  }
  for (int d = 0; d < m.nv; ++d) {
    if (m.dof_bodyid[d] < 0 || m.dof_bodyid[d] >= m.nbody) return corrupt("dof_bodyid[%d] = %d", d, m.dof_bodyid[d]);
    if (m.dof_jntid[d] < 0 || m.dof_jntid[d] >= m.njnt) return corrupt("dof_jntid[%d] = %d", d, m.dof_jntid[d]);
    if (m.dof_parentid[d] < -1 || m.dof_parentid[d] >= d) return corrupt("dof_parentid[%d] = %d", d, m.dof_parentid[d]);
  }
  for (int g = 0; g < m.ngeom; ++g) {
    if (m.geom_bodyid[g] < 0 || m.geom_bodyid[g] >= m.nbody) return corrupt("geom_bodyid[%d] = %d", g, m.geom_bodyid[g]);
    if (m.geom_type[g] < 0 || m.geom_type[g] > MYO_GEOM_MESH) return corrupt("geom_type[%d] = %d", g, m.geom_type[g]);
  }
  for (int k = 0; k < m.nsite; ++k) if (m.site_bodyid[k] < 0 || m.site_bodyid[k] >= m.nbody) return corrupt("site_bodyid[%d] = %d", k, m.site_bodyid[k]);
  for (int t = 0; t < m.ntendon; ++t) {
    const int a = m.tendon_adr[t], c = m.tendon_num[t];
    if (a < 0 || c < 0 || a > m.nwrap || c > m.nwrap - a) return corrupt("tendon_adr/num[%d] = %d/%d", t, a, c);
  }
  for (int w = 0; w < m.nwrap; ++w) {
    const int ty = m.wrap_type[w], id = m.wrap_objid[w];
    if (ty == MYO_WRAP_SITE && (id < 0 || id >= m.nsite)) return corrupt("wrap_objid[%d] = %d (site)", w, id);
    if (ty == MYO_WRAP_SPHERE || ty == MYO_WRAP_CYLINDER) {
      if (id < 0 || id >= m.ngeom) return corrupt("wrap_objid[%d] = %d (geom)", w, id);
      if (m.wrap_prm[w] >= 0 && !(m.wrap_prm[w] < (double)m.nsite)) return corrupt("wrap_prm[%d]: side site out of range", w);
    }
  }
  for (int i = 0; i < m.nu; ++i) if (x.trntype[i] == MYO_TRN_TENDON && (x.trnid[2 * i] < 0 || x.trnid[2 * i] >= m.ntendon)) return corrupt("actuator_trnid[%d] = %d", i, x.trnid[2 * i]);
  for (size_t p = 0; p < m.pair_geom1.size(); ++p)
    if (m.pair_geom1[p] < 0 || m.pair_geom1[p] >= m.ngeom || m.pair_geom2[p] < 0 || m.pair_geom2[p] >= m.ngeom) return corrupt("collision pair %zu names a geom out of range", p);
  if (!(m.timestep > 0) || !std::isfinite(m.timestep) || m.iterations < 0) return corrupt("opt.timestep / opt.iterations");
  return MYO_OK;
}

// pairs of the primitive narrow phases first, the extended ones (csrc/myo_physics.h:collide_pair_ext) after them
static int order_pairs(myo_model& m) {
  auto is_std = [&](int p) {
    const int t1 = m.geom_type[m.pair_geom1[p]], t2 = m.geom_type[m.pair_geom2[p]];
    return (t1 == MYO_GEOM_PLANE && (t2 == MYO_GEOM_SPHERE || t2 == MYO_GEOM_CAPSULE)) || (t1 == MYO_GEOM_SPHERE && (t2 == MYO_GEOM_SPHERE || t2 == MYO_GEOM_CAPSULE || t2 == MYO_GEOM_BOX)) ||
           (t1 == MYO_GEOM_CAPSULE && t2 == MYO_GEOM_CAPSULE);
  };
  int k = 0;
  while (k < m.npair && is_std(k)) k++;
  m.npair_std = k;
  for (; k < m.npair; ++k)
    if (is_std(k)) return fail(MYO_E_ARG, "corrupt model: collision pairs are not ordered (primitive pairs first)");
  return MYO_OK;
}

// ---- capacity / feature checks that need no derived table
static int check_capacity(const myo_model& m, const BlobOnly& x) {
  const struct { int n, cap; const char* what; } sizes[] = {{m.nbody, MYO_NB_MAX, "nbody"}, {m.njnt, MYO_NJ_MAX, "njnt"}, {m.nv, MYO_NV_MAX, "nv"},
                                                           {m.nq, MYO_NQ_MAX, "nq"}, {m.ntendon, MYO_NT_MAX, "ntendon"}, {m.nu, MYO_NU_MAX, "nu"}};
  for (const auto& s : sizes) if (s.n > s.cap) return over_capacity(s.what);
  if (m.nbody > 64 || m.njnt > 64 || m.ntendon > 64 || m.nu > 64) return over_capacity("more than 64 bodies/joints/tendons/actuators");
  for (int i = 0; i < m.nu; ++i) if (x.trntype[i] != MYO_TRN_TENDON) return over_capacity("only tendon transmissions are supported");
  for (int j = 0; j < m.njnt; ++j) if (m.jnt_type[j] == MYO_JNT_BALL) return over_capacity("ball joints");
  return MYO_OK;
}

// ---- derived tables
static int build_tree_tables(myo_model& m) {
  const int nb = m.nbody, nv = m.nv;
  m.body_depth.assign(nb, 0);
  m.maxdepth = 0;
  for (int b = 1; b < nb; ++b) { m.body_depth[b] = m.body_depth[m.body_parentid[b]] + 1; if (m.body_depth[b] > m.maxdepth) m.maxdepth = m.body_depth[b]; }
  m.dof_rootbody.resize(nv);
  for (int d = 0; d < nv; ++d) m.dof_rootbody[d] = m.body_rootid[m.dof_bodyid[d]];
  m.body_dofmask.assign(nb, 0ull);
  for (int b = 1; b < nb; ++b) {
    unsigned long long mk = m.body_dofmask[m.body_parentid[b]];
    for (int k = 0; k < m.body_dofnum[b]; ++k) mk |= 1ull << (m.body_dofadr[b] + k);
    m.body_dofmask[b] = mk;
  }
  m.body_submask.assign(nb, 0ull);
  for (int b = nb - 1; b >= 1; --b) {
    m.body_submask[b] |= 1ull << b;
    if (m.body_parentid[b] > 0) m.body_submask[m.body_parentid[b]] |= m.body_submask[b];
  }
  m.dof_prevmask.assign(nv, 0ull);
  for (int d = 0; d < nv; ++d) {
    const int j = m.dof_jntid[d], b = m.dof_bodyid[d];
    unsigned long long below = (d == 0) ? 0ull : ((1ull << d) - 1ull);
    if (m.jnt_type[j] == MYO_JNT_FREE) {
      const int da = m.jnt_dofadr[j];
      if (d < da + 3) m.dof_prevmask[d] = 1ull << 63;  // translational: cdof_dot = 0
      else m.dof_prevmask[d] = (m.body_dofmask[b] & ((da == 0) ? 0ull : ((1ull << da) - 1ull))) | (7ull << da);
    } else m.dof_prevmask[d] = m.body_dofmask[b] & below;
  }
  // tree-sparse M (MuJoCo's dof_Madr order: row i holds (i,i),(i,parent),(i,grandparent),...)
  m.dof_Madr.resize(nv);
  m.M_i.clear(); m.M_j.clear();
  for (int i = 0; i < nv; ++i) {
    m.dof_Madr[i] = (int)m.M_i.size();
    for (int j = i; j >= 0; j = m.dof_parentid[j]) { m.M_i.push_back(i); m.M_j.push_back(j); }
  }
  m.nM = (int)m.M_i.size();
  if (m.nM > MYO_NM_MAX) return over_capacity("nM");
  // packed entry table: row | column << 8 | body of the row dof << 16 (one load per entry of the sparse M)
  m.M_pk.assign(MYO_NM_MAX, 0);
  for (int e = 0; e < m.nM; ++e)
    m.M_pk[e] = m.M_i[e] | (m.M_j[e] << 8) | (m.dof_bodyid[m.M_i[e]] << 16);
  std::vector<std::vector<std::pair<int, int>>> rows(nv);
  for (int e = 0; e < m.nM; ++e) {
    rows[m.M_i[e]].push_back({m.M_j[e], e});
    if (m.M_i[e] != m.M_j[e]) rows[m.M_j[e]].push_back({m.M_i[e], e});
  }
  m.mv_adr.assign(nv + 1, 0);
  for (int i = 0; i < nv; ++i) {
    m.mv_adr[i] = (int)m.mv_col.size();
    for (auto& pr : rows[i]) { m.mv_col.push_back(pr.first); m.mv_e.push_back(pr.second); }
  }
  m.mv_adr[nv] = (int)m.mv_col.size();
  // the same rows packed for one wide load per dof: 16-bit entries (qM index << 6 | column), two per word
  m.mv_pack.assign((size_t)nv * (MYO_MV_ROW / 2), 0);
  m.mv_len.assign(nv, 0);
  for (int i = 0; i < nv; ++i) {
    const int len = m.mv_adr[i + 1] - m.mv_adr[i];
    if (len > MYO_MV_ROW) return over_capacity("a row of the inertia matrix has more than MYO_MV_ROW non-zeros");
    m.mv_len[i] = len;
    for (int k = 0; k < len; ++k)
      pack16(&m.mv_pack[(size_t)i * (MYO_MV_ROW / 2)], k, ((unsigned)m.mv_e[m.mv_adr[i] + k] << 6) | (unsigned)m.mv_col[m.mv_adr[i] + k]);
  }
  return MYO_OK;
}

// tendons: dofs each one can move; side sites
static int build_wrap_records(myo_model& m, const BlobOnly& x) {
  m.tendon_dofmask.assign(m.ntendon, 0ull);
  m.wrap_side.assign(m.nwrap, -1);
  for (int t = 0; t < m.ntendon; ++t) {
    unsigned long long mk = 0;
    for (int w = m.tendon_adr[t]; w < m.tendon_adr[t] + m.tendon_num[t]; ++w) {
      const int ty = m.wrap_type[w];
      if (ty == MYO_WRAP_SITE) mk |= m.body_dofmask[m.site_bodyid[m.wrap_objid[w]]];
      else if (ty == MYO_WRAP_SPHERE || ty == MYO_WRAP_CYLINDER) {
        mk |= m.body_dofmask[m.geom_bodyid[m.wrap_objid[w]]];
        m.wrap_side[w] = m.wrap_prm[w] >= 0 ? (int)lround(m.wrap_prm[w]) : -1;
      } else if (ty != MYO_WRAP_PULLEY) return over_capacity("fixed (joint) tendons");
    }
    m.tendon_dofmask[t] = mk;
    if (popcount64(mk) > MYO_TJ_MAX) return over_capacity("a tendon moves more than MYO_TJ_MAX dofs");
  }
  // resolved wrap records: everything the tendon stage needs about wrap object w behind ONE level of
  // indexing (the stage is bound by dependent table loads otherwise: type -> objid -> bodyid -> pos):
  //   wr_i[8w..]  = type, body (site / geom body), geom id (-1), side-site body (-1), root body of
  //                 `body`, root body of the side-site body, 0, 0
  //   wr_p[4w..]  = local position (site_pos / geom_pos), pulley divisor
  //   wr_m[12w..] = geom_mat (9), side-site local position (3)
  //   wr_mask[w]  = body_dofmask[body]
  m.wr_i.assign(8 * (size_t)m.nwrap, 0);
  m.wr_p.assign(4 * (size_t)m.nwrap, 0.0);
  m.wr_m.assign(12 * (size_t)m.nwrap, 0.0);
  m.wr_mask.assign(m.nwrap, 0ull);
  for (int w = 0; w < m.nwrap; ++w) {
    const int ty = m.wrap_type[w], id = m.wrap_objid[w];
    int* I = &m.wr_i[8 * (size_t)w];
    I[0] = ty; I[1] = -1; I[2] = -1; I[3] = -1; I[4] = 0; I[5] = 0;
    if (ty == MYO_WRAP_SITE) {
      I[1] = m.site_bodyid[id];
      for (int k = 0; k < 3; ++k) m.wr_p[4 * (size_t)w + k] = m.site_pos[3 * id + k];
    } else if (ty == MYO_WRAP_SPHERE || ty == MYO_WRAP_CYLINDER) {
      I[1] = m.geom_bodyid[id]; I[2] = id;
      for (int k = 0; k < 3; ++k) m.wr_p[4 * (size_t)w + k] = m.geom_pos[3 * id + k];
      double gm[9];
      quat2mat_h(&x.geom_quat[4 * id], gm);
      for (int k = 0; k < 9; ++k) m.wr_m[12 * (size_t)w + k] = gm[k];
      const int sid = m.wrap_side[w];
      if (sid >= 0) {
        I[3] = m.site_bodyid[sid]; I[5] = m.body_rootid[I[3]];
        for (int k = 0; k < 3; ++k) m.wr_m[12 * (size_t)w + 9 + k] = m.site_pos[3 * sid + k];
      }
    } else if (ty == MYO_WRAP_PULLEY) m.wr_p[4 * (size_t)w + 3] = m.wrap_prm[w];
    if (I[1] >= 0) { I[4] = m.body_rootid[I[1]]; m.wr_mask[w] = m.body_dofmask[I[1]]; }
  }
  // geom wraps, enumerated: gw_elem[k] = path element of the k-th sphere/cylinder wrap; wr_i[8w+6] = k
  m.gw_elem.clear();
  for (int w = 0; w < m.nwrap; ++w) {
    m.wr_i[8 * (size_t)w + 6] = -1;
    if (m.wrap_type[w] == MYO_WRAP_SPHERE || m.wrap_type[w] == MYO_WRAP_CYLINDER) {
      m.wr_i[8 * (size_t)w + 6] = (int)m.gw_elem.size();
      m.gw_elem.push_back(w);
    }
  }
  m.ngw = (int)m.gw_elem.size();
  if (m.gw_elem.empty()) m.gw_elem.push_back(0);
  return MYO_OK;
}

// path elements, enumerated (the walk mj_tendon makes along each tendon, resolved once): element e runs from the site
// te_i[4e] to the site te_i[4e+1], around the wrap geom te_i[4e+2] (-1: straight), belongs to tendon te_i[4e+3] and
// counts with 1 / te_div[e] (the last pulley before it).  The tendon stage gives each element its own lane.
static int build_path_elements(myo_model& m) {
  m.te_i.clear(); m.te_div.clear();
  m.tendon_eadr.assign(m.ntendon, 0); m.tendon_enum.assign(m.ntendon, 0);
  for (int t = 0; t < m.ntendon; ++t) {
    const int adr = m.tendon_adr[t], num = m.tendon_num[t];
    double divisor = 1.0;
    m.tendon_eadr[t] = (int)m.te_div.size();
    for (int j = 0; j < num - 1;) {
      const int ty0 = m.wrap_type[adr + j], ty1 = m.wrap_type[adr + j + 1];
      if (ty0 == MYO_WRAP_PULLEY || ty1 == MYO_WRAP_PULLEY) {
        if (ty0 == MYO_WRAP_PULLEY) divisor = m.wrap_prm[adr + j];
        j++;
        continue;
      }
      const int is_geom = (ty1 == MYO_WRAP_SPHERE || ty1 == MYO_WRAP_CYLINDER);
      if (is_geom && j + 2 >= num) return over_capacity("a tendon path ends on a wrap geom");
      const int end = j + (is_geom ? 2 : 1);
      m.te_i.push_back(adr + j); m.te_i.push_back(adr + end); m.te_i.push_back(is_geom ? adr + j + 1 : -1); m.te_i.push_back(t);
      m.te_div.push_back(divisor);
      j = end;
    }
    m.tendon_enum[t] = (int)m.te_div.size() - m.tendon_eadr[t];
  }
  m.nte = (int)m.te_div.size();
  // element lengths are staged (HP) in the part of H that is free during the tendon stage (behind cinert)
  if ((size_t)m.nte * sizeof(double) > (size_t)(MYO_H_SIZE - MYO_NB_MAX * 10) * sizeof(float)) return over_capacity("tendon path elements (length staging)");
  if (m.te_div.empty()) { m.te_i.assign(4, 0); m.te_div.push_back(1.0); }
  // staging area of the tendon stage.  Mixed stepper: T path points in con[], then (8-byte aligned) 7 HP wrap results per geom wrap,
  // running on through the limit-row, efc_* and solver vectors up to rk.  fp64 stepper: the wrap results only, up to the solver
  // vectors (where its body poses live during the position stage)
  typedef Scratch<double, MYO_NCON_F64> ScratchD;
  // (... and not beyond efc_jv, where that stepper accumulates the tendon moment arms meanwhile)
  if (7 * (size_t)m.ngw * sizeof(double) > offsetof(ScratchD, efc_jv) - offsetof(ScratchD, con) ||
      m.ngw > MYO_BIGWS_GW ||                     /* (the 48-slot fp64 scratch: in the big workspace, TaskDev::big_ws) */
      ((3 * (size_t)m.nwrap * sizeof(float) + 7) & ~(size_t)7) + 7 * (size_t)m.ngw * sizeof(double) >
          offsetof(Scratch<float>, rk) - offsetof(Scratch<float>, con))
    return over_capacity("tendon path elements / wrap geoms (staging area of the tendon stage)");
  return MYO_OK;
}

static int build_actuator_gather(myo_model& m, const BlobOnly& x) {
  const int nv = m.nv;
  m.actuator_tendon.resize(m.nu);
  for (int i = 0; i < m.nu; ++i) m.actuator_tendon[i] = x.trnid[2 * i];
  // qfrc_actuator gather, dof-major: for dof d the (ten_J offset << 6 | actuator) pairs of every
  // actuator whose tendon moves d, in actuator order; 16-bit entries, two per word (one wide load per dof)
  m.aq_pack.assign((size_t)nv * (MYO_AQ_ROW / 2), 0);
  m.aq_len.assign(nv, 0);
  for (int d = 0; d < nv; ++d) {
    int len = 0;
    for (int i = 0; i < m.nu; ++i) {
      const int t = m.actuator_tendon[i];
      const unsigned long long mk = m.tendon_dofmask[t];
      if (!((mk >> d) & 1ull)) continue;
      if (len >= MYO_AQ_ROW) return over_capacity("more than MYO_AQ_ROW actuators act on one dof");
      const int slot = popcount64(mk & ((1ull << d) - 1ull));      // the tendon's moving dofs below d
      pack16(&m.aq_pack[(size_t)d * (MYO_AQ_ROW / 2)], len, ((unsigned)(t * MYO_TJ_MAX + slot) << 6) | (unsigned)i);
      len++;
    }
    m.aq_len[d] = len;
  }
  // actuator-major copies for the moment-transpose gather, zero-padded to MYO_NU_MAX so the loop
  // runs in unconditional groups of 8 (scalar loads merge into s_load_dwordx8/x16)
  m.act_dofmask.assign(MYO_NU_MAX, 0ull);
  m.act_tj.assign(MYO_NU_MAX, 0);
  m.act_gear0.assign(MYO_NU_MAX, 0.0);
  m.act_sd.assign((size_t)MYO_NU_MAX * MYO_TJ_MAX, -1);      // dof of slot k of actuator i's tendon (-1: the tendon moves fewer dofs)
  for (int i = 0; i < m.nu; ++i) {
    m.act_dofmask[i] = m.tendon_dofmask[m.actuator_tendon[i]];
    m.act_tj[i] = m.actuator_tendon[i] * MYO_TJ_MAX;
    m.act_gear0[i] = m.actuator_gear[6 * i];
    { int k = 0; for (int d = 0; d < nv && k < MYO_TJ_MAX; ++d) if ((m.act_dofmask[i] >> d) & 1ull) m.act_sd[(size_t)i * MYO_TJ_MAX + k++] = d; }
  }
  return MYO_OK;
}

// muscle constants of every actuator (fwd_actuation: what mju_muscleGain / mju_muscleBias / mju_muscleDynamics derive from the
// parameters alone, with every constant denominator turned into a reciprocal): MYO_ACT_PRE doubles per actuator, see myo_physics.h
static void build_muscle_constants(myo_model& m) {
  m.act_pre.assign((size_t)MYO_NU_MAX * MYO_ACT_PRE, 0.0);
  for (int i = 0; i < m.nu; ++i) {
    double* P = &m.act_pre[(size_t)i * MYO_ACT_PRE];
    const double* gp = &m.actuator_gainprm[10 * (size_t)i];
    const double* bp = &m.actuator_biasprm[10 * (size_t)i];
    const double* dp = &m.actuator_dynprm[10 * (size_t)i];
    const double lr0 = m.actuator_lengthrange[2 * (size_t)i], lr1 = m.actuator_lengthrange[2 * (size_t)i + 1], acc0 = m.actuator_acc0[i];
    const double tiny = 1e-15;
    {   // gain
      const double force = gp[2] < 0 ? gp[3] / std::max(tiny, acc0) : gp[2];
      const double L0 = (lr1 - lr0) / std::max(tiny, gp[1] - gp[0]);
      const double lmin = gp[4], lmax = gp[5], a = 0.5 * (lmin + 1), b = 0.5 * (1 + lmax), y = gp[8] - 1;
      P[0] = force; P[1] = gp[0]; P[2] = 1.0 / std::max(tiny, L0); P[3] = lr0; P[4] = 1.0 / std::max(tiny, L0 * gp[6]);
      P[5] = lmin; P[6] = lmax; P[7] = a; P[8] = b;
      P[9] = 1.0 / std::max(tiny, a - lmin); P[10] = 1.0 / std::max(tiny, 1 - a); P[11] = 1.0 / std::max(tiny, b - 1); P[12] = 1.0 / std::max(tiny, lmax - b);
      P[13] = y; P[14] = 1.0 / std::max(tiny, y); P[15] = gp[8];
    }
    {   // bias
      const double force = bp[2] < 0 ? bp[3] / std::max(tiny, acc0) : bp[2];
      const double L0 = (lr1 - lr0) / std::max(tiny, bp[1] - bp[0]);
      const double b = 0.5 * (1 + bp[5]);
      P[16] = force; P[17] = bp[0]; P[18] = 1.0 / std::max(tiny, L0); P[19] = b; P[20] = 1.0 / std::max(tiny, b - 1); P[21] = bp[7];
    }
    // activation dynamics: 1 / tau_deact when tau = tau_deact / (0.5 + 1.5 act) can never reach the floor (act in [0, 1]); else 0: the formula as written
    P[22] = dp[1] / 2.0 >= tiny ? 1.0 / dp[1] : 0.0;
  }
}

// per-lane records (myo_model_dev.h: bk_i / bk_f / jk_i / dk_i / dof_spr / dof_submask): what a body / joint / dof lane reads in a
// stage, behind ONE index instead of body -> joint -> qpos chains of dependent vector loads
static int build_lane_records(myo_model& m) {
  const int nb = m.nbody, nv = m.nv, njnt = m.njnt;
  m.bk_i.assign((size_t)MYO_BK_I * (nb > 0 ? nb : 1), 0);
  m.bk_f.assign((size_t)MYO_BK_F * (nb > 0 ? nb : 1), 0.0);
  for (int b = 0; b < nb; ++b) {
    int* I = &m.bk_i[(size_t)MYO_BK_I * b];
    double* F = &m.bk_f[(size_t)MYO_BK_F * b];
    const int jn = m.body_jntnum[b], ja = m.body_jntadr[b];
    const bool is_free = jn == 1 && m.jnt_type[ja] == MYO_JNT_FREE;
    if (jn > MYO_BK_NJ) return over_capacity("more than three joints on one body");
    I[0] = m.body_depth[b]; I[1] = m.body_parentid[b]; I[2] = jn; I[3] = ja; I[4] = is_free ? 1 : 0;
    for (int k = 0; k < 3; ++k) F[k] = m.body_pos[3 * (size_t)b + k];
    for (int k = 0; k < 4; ++k) F[3 + k] = m.body_quat[4 * (size_t)b + k];
    for (int k = 0; k < jn && k < MYO_BK_NJ; ++k) {
      const int j = ja + k, qa = m.jnt_qposadr[j];
      I[5 + k] = qa; I[8 + k] = m.jnt_type[j];
      for (int e = 0; e < 3; ++e) { F[7 + 7 * k + e] = m.jnt_pos[3 * (size_t)j + e]; F[10 + 7 * k + e] = m.jnt_axis[3 * (size_t)j + e]; }
      F[13 + 7 * k] = m.qpos0[qa];
    }
  }
  m.jk_i.assign((size_t)4 * (njnt > 0 ? njnt : 1), 0);
  for (int j = 0; j < njnt; ++j) {
    int* I = &m.jk_i[(size_t)4 * j];
    I[0] = m.jnt_bodyid[j]; I[1] = m.jnt_dofadr[j]; I[2] = m.jnt_type[j]; I[3] = m.body_rootid[m.jnt_bodyid[j]];
  }
  m.dk_i.assign((size_t)2 * (nv > 0 ? nv : 1), 0);
  m.dof_spr.assign((size_t)2 * (nv > 0 ? nv : 1), 0.0);
  m.dof_submask.assign(nv > 0 ? nv : 1, 0ull);
  for (int d = 0; d < nv; ++d) {
    const int j = m.dof_jntid[d], qa = m.jnt_qposadr[j];
    m.dk_i[(size_t)2 * d] = qa;
    const bool spring = m.jnt_type[j] != MYO_JNT_FREE && m.jnt_stiffness[j] != 0;
    m.dof_spr[(size_t)2 * d] = spring ? m.jnt_stiffness[j] : 0.0;
    m.dof_spr[(size_t)2 * d + 1] = m.qpos_spring[qa];
    m.dof_submask[d] = m.body_submask[m.dof_bodyid[d]];
  }
  return MYO_OK;
}

// MuJoCo's mix of two geoms' solver parameters (mj_contactParam): all of the higher-priority geom's, else by solmix
static double pair_solmix(const myo_model& m, int g1, int g2) {
  const int pr1 = m.geom_priority[g1], pr2 = m.geom_priority[g2];
  if (pr1 != pr2) return pr1 > pr2 ? 1.0 : 0.0;
  const double x1 = m.geom_solmix[g1], x2 = m.geom_solmix[g2];
  const double tiny = 1e-15;      // MYO_MINVAL
  if (x1 >= tiny && x2 >= tiny) return x1 / (x1 + x2);
  if (x1 < tiny && x2 < tiny) return 0.5;
  return x1 < tiny ? 0.0 : 1.0;
}
// per-pair contact records: everything mj_contactParam / the constraint build derive from the two geoms
// alone is resolved here (the device stage was a chain of dependent table loads per contact):
//   pc_i[8p..]  = body1, body2, root body 1, root body 2, nsup, box-box candidate (0 none; 1 + v: vertex v of geom 1 against
//                 geom 2, 9 + v: vertex v of geom 2 against geom 1, 17: the edge-edge candidate), 0, friction selector (0 max, 1 geom1, 2 geom2)
//   pc_sup[4p..] = the dofs either body can move (<= 16 bytes, ascending)
//   pc_f[16p..] = margin, margin - gap, (K, B) and (d0, d1, 1 / width, mid, power) of the mixed solref[2] / solimp[5] (sol_precompute), friction1[3], friction2[3], invweight sum
//   pc_mask[2p..] = ancestor-dof masks of the two bodies
static int build_pair_records(myo_model& m, const BlobOnly& x) {
  const int np = m.npair > 0 ? m.npair : 1;
  m.pc_i.assign(8 * (size_t)np, 0); m.pc_sup.assign(4 * (size_t)np, 0);
  m.pc_f.assign(16 * (size_t)np, 0.0); m.pc_mask.assign(2 * (size_t)np, 0ull);
  m.pair_mg.assign(2 * (size_t)np, 0.0);     // margin, margin - gap per pair row (HP copy on the device: the general narrow-phase path reads them)
  m.any_rot = 0; m.any_gen = 0;
  for (int p = 0; p < m.npair; ++p) {
    const int g1 = m.pair_geom1[p], g2 = m.pair_geom2[p];
    const int b1 = m.geom_bodyid[g1], b2 = m.geom_bodyid[g2];
    const unsigned long long m1 = m.body_dofmask[b1], m2 = m.body_dofmask[b2];
    unsigned long long mk = m1 | m2;
    const int cnt = popcount64(mk);
    if (cnt > MYO_CS_MAX) return over_capacity("a contact pair moves more than MYO_CS_MAX dofs");
    int* I = &m.pc_i[8 * (size_t)p];
    I[0] = b1; I[1] = b2; I[2] = m.body_rootid[b1]; I[3] = m.body_rootid[b2]; I[4] = cnt; I[5] = x.pair_sub[p];
    unsigned char* sup = reinterpret_cast<unsigned char*>(&m.pc_sup[4 * (size_t)p]);
    // (bit 6 / bit 7 of an entry: ancestor dof of body 1 / body 2 — ContactRec::sup)
    { int ns = 0; for (int d = 0; d < 64 && ns < MYO_CS_MAX; ++d) if ((mk >> d) & 1ull) sup[ns++] = (unsigned char)(d | (int)((m1 >> d) & 1ull) << 6 | (int)((m2 >> d) & 1ull) << 7); }
    m.pc_mask[2 * (size_t)p] = m1; m.pc_mask[2 * (size_t)p + 1] = m2;
    const int pr1 = m.geom_priority[g1], pr2 = m.geom_priority[g2];
    const double mix = pair_solmix(m, g1, g2);
    double* F = &m.pc_f[16 * (size_t)p];
    const double margin = std::max(m.geom_margin[g1], m.geom_margin[g2]);
    F[0] = margin; F[1] = margin - std::max(m.geom_gap[g1], m.geom_gap[g2]);
    const double *r1 = &m.geom_solref[2 * g1], *r2 = &m.geom_solref[2 * g2];
    for (int e = 0; e < 2; ++e) F[2 + e] = (r1[0] > 0 && r2[0] > 0) ? mix * r1[e] + (1 - mix) * r2[e] : std::min(r1[e], r2[e]);
    for (int e = 0; e < 5; ++e) F[4 + e] = mix * m.geom_solimp[5 * g1 + e] + (1 - mix) * m.geom_solimp[5 * g2 + e];
    for (int e = 0; e < 3; ++e) { F[9 + e] = m.geom_friction[3 * g1 + e]; F[12 + e] = m.geom_friction[3 * g2 + e]; }
    F[15] = m.body_invweight0[2 * b1] + m.body_invweight0[2 * b2];
    I[7] = (pr1 == pr2) ? 0 : (pr1 > pr2 ? 1 : 2);
    // condim of the contact (mj_contactParam): the higher-priority geom's, the larger of the two at equal priority
    const int d1 = x.geom_condim[g1], d2 = x.geom_condim[g2];
    I[6] = (pr1 == pr2) ? std::max(d1, d2) : (pr1 > pr2 ? d1 : d2);
    double mg0 = margin, mg1 = F[1];
    if (x.pair_xp[p] >= 0) {                  // an explicit <pair>: its own margin / gap / solref / solimp / friction / condim, nothing mixed, no per-env friction
      const int xi = x.pair_xp[p];
      mg0 = x.xp_margin[xi]; mg1 = x.xp_margin[xi] - x.xp_gap[xi];
      F[0] = mg0; F[1] = mg1;
      for (int e = 0; e < 2; ++e) F[2 + e] = x.xp_solref[2 * xi + e];
      for (int e = 0; e < 5; ++e) F[4 + e] = x.xp_solimp[5 * xi + e];
      for (int e = 0; e < 3; ++e) { F[9 + e] = x.xp_friction[3 * xi + e]; F[12 + e] = x.xp_friction[3 * xi + e]; }
      I[6] = x.xp_dim[xi] | 0x100;
      I[7] = 0;
      m.any_gen = 1;                          // (the general path reads the pair's own margin and skips the per-env friction patch)
    }
    m.pair_mg[2 * (size_t)p] = mg0; m.pair_mg[2 * (size_t)p + 1] = mg1;
    sol_precompute(F + 2, F + 4, m.timestep, m.disableflags);      // pc_f[2..8]: (K, B), (d0, d1, 1 / width, mid, power) — what sol_param reads
    const int dim = I[6] & 255;
    if (dim != 1 && dim != 3 && dim != 4 && dim != 6) return over_capacity("contact dimension (condim) other than 1, 3, 4, 6");
    if (dim > 3) m.any_rot = 1;
    if (dim != 3) m.any_gen = 1;
  }
  return MYO_OK;
}

static void build_frames(myo_model& m, const BlobOnly& x) {
  const int nb = m.nbody;
  m.body_imat.resize(9 * nb);
  for (int b = 0; b < nb; ++b) quat2mat_h(&x.body_iquat[4 * b], &m.body_imat[9 * b]);
  m.geom_mat.resize(9 * (size_t)m.ngeom);
  for (int g = 0; g < m.ngeom; ++g) quat2mat_h(&x.geom_quat[4 * g], &m.geom_mat[9 * g]);
  // trailing dofs whose row of M is diagonal by construction: a free joint on a leaf body whose
  // inertial frame coincides with the body frame (M = diag(m,m,m,Ixx,Iyy,Izz)); nlead = first of them
  m.nlead = m.nv;
  for (int j = m.njnt - 1; j >= 0; --j) {
    const int b = m.jnt_bodyid[j];
    bool leaf = true;
    for (int o = 1; o < nb; ++o) if (m.body_parentid[o] == b) leaf = false;
    const double* iq = &x.body_iquat[4 * b]; const double* ip = &m.body_ipos[3 * b];
    const bool aligned = fabs(fabs(iq[0]) - 1.0) < 1e-12 && fabs(ip[0]) + fabs(ip[1]) + fabs(ip[2]) < 1e-14;
    if (m.jnt_type[j] == MYO_JNT_FREE && leaf && aligned && m.body_jntnum[b] == 1 && m.jnt_dofadr[j] + 6 == m.nlead)
      m.nlead = m.jnt_dofadr[j];
    else break;
  }
}

// the rows' solver parameters in the form sol_param reads them (in place: same names, same sizes)
static void resolve_solver_params(myo_model& m) {
  for (int j = 0; j < m.njnt; ++j) sol_precompute(&m.jnt_solref[2 * (size_t)j], &m.jnt_solimp[5 * (size_t)j], m.timestep, m.disableflags);
  for (int t = 0; t < m.ntendon; ++t) {
    sol_precompute(&m.tendon_solref_lim[2 * (size_t)t], &m.tendon_solimp_lim[5 * (size_t)t], m.timestep, m.disableflags);
    sol_precompute(&m.tendon_solref_fri[2 * (size_t)t], &m.tendon_solimp_fri[5 * (size_t)t], m.timestep, m.disableflags);
  }
  for (int d = 0; d < m.nv; ++d) sol_precompute(&m.dof_solref[2 * (size_t)d], &m.dof_solimp[5 * (size_t)d], m.timestep, m.disableflags);
}

static int set_feature_flags(myo_model& m) {
  m.any_floss = 0;
  int nfr = 0;
  for (int d = 0; d < m.nv; ++d) if (m.dof_frictionloss[d] > 0) { m.any_floss = 1; nfr++; }
  for (int t = 0; t < m.ntendon; ++t) if (m.tendon_frictionloss[t] > 0) { m.any_floss = 1; nfr++; }
  if (nfr > MYO_NLIM_MAX / 2) return over_capacity("friction-loss rows (more than half of the limit-row capacity)");
  for (int d = 0; d < m.nv; ++d)
    if (m.dof_frictionloss[d] > 0 && m.jnt_type[m.dof_jntid[d]] == MYO_JNT_FREE) return over_capacity("friction loss on the dofs of a free joint");
  m.any_damping = 0;
  for (int d = 0; d < m.nv; ++d) if (m.dof_damping[d] > 0) m.any_damping = 1;
  m.any_tendon_passive = 0;
  for (int t = 0; t < m.ntendon; ++t) if (m.tendon_stiffness[t] != 0 || m.tendon_damping[t] != 0) m.any_tendon_passive = 1;
  return MYO_OK;
}

static int model_from_blob_impl(const void* blob, size_t nbytes, myo_model** out) {
  if (!blob || !out || nbytes < sizeof(myo_blob_header)) return fail(MYO_E_ARG, "null or short blob");
  const myo_blob_header* h = (const myo_blob_header*)blob;
  if (h->magic != MYO_BLOB_MAGIC || h->version != MYO_BLOB_VERSION || h->total_bytes != nbytes ||
      sizeof(myo_blob_header) + (size_t)h->n_fields * sizeof(myo_blob_field) > nbytes)
    return fail(MYO_E_ARG, "bad model blob header");
  std::unique_ptr<myo_model> owner(new myo_model());
  myo_model& m = *owner;
  BlobOnly x;
  if (int rc = read_fields(blob, nbytes, m, x)) return rc;
  if (int rc = check_untrusted(m, x)) return rc;
  if (int rc = order_pairs(m)) return rc;
  if (int rc = check_capacity(m, x)) return rc;
  if (int rc = build_tree_tables(m)) return rc;
  if (int rc = build_wrap_records(m, x)) return rc;
  if (int rc = build_path_elements(m)) return rc;
  if (int rc = build_actuator_gather(m, x)) return rc;
  build_muscle_constants(m);
  if (int rc = build_lane_records(m)) return rc;
  if (int rc = build_pair_records(m, x)) return rc;
  build_frames(m, x);
  resolve_solver_params(m);
  build_ldl_tables(&m);
  build_arrow_tables(&m);
  if (int rc = set_feature_flags(m)) return rc;
  render_vis_table(&m, blob, nbytes);
  render_tendon_table(&m, blob, nbytes, x.trntype);
  *out = owner.release();
  return MYO_OK;
}
extern "C" int myo_model_from_blob(const void* blob, size_t nbytes, myo_model** out) {
  try { return model_from_blob_impl(blob, nbytes, out); }          // no C++ exception crosses the C ABI
  catch (const std::exception& e) { return fail(MYO_E_ARG, "model blob rejected: %s", e.what()); }
}

extern "C" int myo_model_load_mjb(const char* path, int integrator, int unsupported_contacts, myo_model** out) {
  if (!path || !out) return fail(MYO_E_ARG, "myo_model_load_mjb: null argument");
  FILE* fh = fopen(path, "rb");
  if (!fh) return fail(MYO_E_ARG, "cannot open %s", path);
  try {                                   // the file is untrusted; no C++ exception crosses the C ABI
    std::vector<unsigned char> raw;
    unsigned char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, fh)) > 0) {
      raw.insert(raw.end(), buf, buf + k);
      if (raw.size() > ((size_t)1 << 31)) { fclose(fh); return fail(MYO_E_ARG, "%s: larger than 2 GiB", path); }
    }
    const int rd_err = ferror(fh);
    fclose(fh);
    if (rd_err) return fail(MYO_E_ARG, "%s: read error", path);
    myo_mjb::File f;
    std::string err;
    if (!myo_mjb::parse(raw.data(), raw.size(), f, err)) return fail(MYO_E_ARG, "%s: %s", path, err.c_str());
    std::vector<unsigned char> blob;
    int unsupported = 0;
    if (!myo_mjb::to_blob(f, integrator, unsupported_contacts, blob, err, &unsupported))
      return fail(unsupported ? MYO_E_UNSUPPORTED : MYO_E_ARG, "%s: %s", path, err.c_str());
    return myo_model_from_blob(blob.data(), blob.size(), out);
  } catch (const std::exception& e) {
    return fail(MYO_E_ARG, "%s: rejected (%s)", path, e.what());
  }
}
extern "C" void myo_model_destroy(myo_model* m) { delete m; }
extern "C" int myo_model_size(const myo_model* m, const char* n) {
  if (!m || !n) return -1;
#define S(x) if (!strcmp(n, #x)) return m->x;
  S(nq) S(nv) S(nu) S(na) S(nbody) S(njnt) S(ngeom) S(nsite) S(ntendon) S(nwrap) S(npair) S(nM) S(maxdepth)
  S(integrator) S(iterations) S(disableflags) S(any_damping) S(any_tendon_passive) S(nlead) S(ngw) S(nte) S(npair_std) S(ld_nfq) S(ld_nsq) S(arrow_nf)
  S(any_rot) S(any_gen) S(any_floss) S(has_visual) S(ntendon_item)
#undef S
  return -1;
}
// read access to the tables (include/myobatch.h): pointers into the model, nothing copied, no device touched
static int table_dtype(const int*) { return MYO_TABLE_I32; }
static int table_dtype(const unsigned long long*) { return MYO_TABLE_U64; }
static int table_dtype(const float*) { return MYO_TABLE_F32; }
static int table_dtype(const double*) { return MYO_TABLE_F64; }
extern "C" int myo_model_table(const myo_model* m, const char* name, const void** data, size_t* bytes, int* dtype) {
  if (!m || !name || !data || !bytes || !dtype) return fail(MYO_E_ARG, "myo_model_table: null argument");
  bool found = false;
  auto hit = [&](auto* p, size_t count) { *data = p; *bytes = count * sizeof *p; *dtype = table_dtype(p); found = true; };
#define X(n) if (!found && !strcmp(name, #n)) hit(m->n.data(), m->n.size());
  MYO_MODEL_INT_ARRAYS(X) MYO_MODEL_U64_ARRAYS(X) MYO_MODEL_REAL_ARRAYS(X) X(vis) X(tvis) X(titem_adr)
#undef X
  if (!found && !strcmp(name, "timestep")) hit(&m->timestep, 1);
  if (!found && !strcmp(name, "tolerance")) hit(&m->tolerance, 1);
  if (!found && !strcmp(name, "impratio")) hit(&m->impratio, 1);
  if (!found && !strcmp(name, "gravity")) hit(m->gravity, 3);
  if (!found && !strcmp(name, "meaninertia")) hit(&m->meaninertia, 1);
  if (!found && !strcmp(name, "cam_lookat")) hit(m->cam_lookat, 3);
  if (!found && !strcmp(name, "cam_distance")) hit(&m->cam_distance, 1);
  if (!found && !strcmp(name, "arrow_pad")) hit(&m->arrow_pad, 1);
  return found ? MYO_OK : fail(MYO_E_ARG, "myo_model_table: no table named %s", name);
}

// ------------------------------------------------------------------------------------------ batch
#define MYO_PARTS_MAX 8
struct StepPlan { int nparts; int k[MYO_PARTS_MAX + 1]; int wt; };   // wt: parts publish their record with write-through stores instead of an agent release fence      // part p = substeps [k[p], k[p+1]); nparts = 1: whole steps
struct myo_batch;
struct myo_batch {
  int n, device, dtype, nobs;
  int ncap;                    // contact capacity of the scratch: MYO_NCON_MAX, or MYO_NCON_BIG for models with extended pairs / a die
  myo_task_cfg cfg;
  TaskDev K;
  EnvRecordLayout L;
  DumpLayout D;
  double* rec;                 // dev [n, L.stride]
  std::vector<void*> allocs;   // every device allocation (model arrays, records)
  std::vector<double> geom_friction;   // host copy of the model's (nominal values of an object group)
  DevModel<double> Md;
  DevModel<float> Mf;
  int nq, nv, nu, na, nbody, nsite, ntendon, ngeom, integrator;
  unsigned char* bad_state;    // caller-owned dev uint8[n] or null (myo_batch_set_bad_state_buffer)
  // launch order of myo_batch_step (longest-predicted-first, see k_step_order): order[blockIdx] = env, cost[env] = smoothed duration
  // of the env's last steps, ticks[env] = duration of its last step (100 MHz ticks).  order = null: identity.
  int* order;
  float* cost;
  unsigned int* ticks;
  // env steps in parts (k_step): part_state[env] = 16 g + 2 q (parts < q of step g published) or + 1 (part q claimed, running);
  // step_gen[0] = g, advanced on the stream after every step; a workgroup that meets a state of another generation counts it in
  // K.health[0] (myo_batch_health).  plan = substep boundaries of the parts.
  int* part_state;
  int* step_gen;
  StepPlan plan;
  int timing;
  double ms_sum;
  int ms_cnt;
  int wrap_tune_in = 16;       // steps until the next census of the wraps (myo_batch_step: 16 steps after a reset of all envs, then every 256)
  int* wrap_cnt = nullptr;     // dev int[ngw]: engagement counts of the wrap census (CensusJob / k_wrap_reorder); null = one pass of wraps, nothing to order
  bool has_slot_ws = false;    // K.ctrl_ws is the device's shared wave-slot workspace (slot_workspace_acquire / _release)
  bool has_big_ws = false;     // ... and K.big_ws its block of the 48-slot fp64 scratch's records / wrap results
  float* vis = nullptr;        // dev [nitem, 8]: the model's visual table with this task's targets drawn (myo_batch_geom_poses)
  int nitem = 0;               // render items: ngeom + nsite
  float* tvis = nullptr;       // dev [ntendon, 8] and dev int[nte]: the model's tendon tables (myo_batch_tendon_paths)
  int* titem_adr = nullptr;
  int ntitem = 0;              // tendon item slots per env
  double cam_lookat[3] = {0, 0, 0}, cam_distance = 1;      // the model's default camera (myo_model_default_camera)
  double* render_ws = nullptr; // dev: item poses and cameras of myo_batch_render, grown on demand (not in allocs)
  size_t render_ws_bytes = 0;
  double* so_ws = nullptr;     // dev [n, MYO_SO_WS_N]: the system matrices of myo_batch_static_opt, allocated by its first solve (not in allocs)
  double* ik_ws = nullptr;     // dev [n, MYO_IK_WS_N]: system matrix, Jacobian and site points of myo_batch_ik, allocated by its first call (not in allocs)
  double* sim_ws = nullptr;    // dev [rows, stride + RK4 stage block]: the shadow records of myo_batch_simulate, grown on demand (not in allocs)
  size_t sim_ws_bytes = 0;
  unsigned long long act_reach = 0;      // dofs some actuator's moment row can reach: myo_batch_static_opt's default weight
  std::vector<double> cam_host;      // the cameras of the last myo_batch_render (source of its asynchronous upload)
  // how contact items are drawn (myo_batch_set_render_style; the defaults of include/myobatch.h)
  myo_render_style style = {sizeof(myo_render_style), 0.003, 0.0005, 0.001, 0.02, {0.9f, 0.6f, 0.2f, 1.f}, {0.7f, 0.9f, 0.9f, 1.f}, 1.0};
  MYO_BACKEND_BATCH_FIELDS     // what the backend keeps per batch (the HIP backend: its timing events)
};

// ---- the kernel variant of a batch.  Every kernel that works on an env, and the lane-serial emulation of it, exists per arithmetic T,
// per integrator (RK: the model integrates with RK4 and the variant has the stage storage) and per contact capacity NC of the scratch
// (each arithmetic's base capacity, or MYO_NCON_BIG for models with extended collision pairs or a die: myo_batch::ncap).  with_variant
// is the one place that maps a batch to its variant: f(KernelVariant<T, RK, NC>{}) is called with the batch's, and its result returned.
template <typename T_, bool RK_, int NC_>
struct KernelVariant { using T = T_; static constexpr bool RK = RK_; static constexpr int NC = NC_; };
template <typename F>
static auto with_variant(const myo_batch* b, F&& f) {
  const bool rk = b->integrator == 1, big = b->ncap > MYO_NCON_MAX;
  if (b->dtype == MYO_F64) {
    if (big) return rk ? f(KernelVariant<double, true, MYO_NCON_BIG>{}) : f(KernelVariant<double, false, MYO_NCON_BIG>{});
    return rk ? f(KernelVariant<double, true, MYO_NCON_F64>{}) : f(KernelVariant<double, false, MYO_NCON_F64>{});
  }
  if (big) return rk ? f(KernelVariant<float, true, MYO_NCON_BIG>{}) : f(KernelVariant<float, false, MYO_NCON_BIG>{});
  return rk ? f(KernelVariant<float, true, MYO_NCON_MAX>{}) : f(KernelVariant<float, false, MYO_NCON_MAX>{});
}
// Dynamic LDS of a variant's workgroup: the scratch, and behind it (aligned) the RK4 stage storage where that lives in LDS — the mixed
// stepper with the base contact capacity (16,384 + 1,360 B: still eight workgroups per CU; the per-workgroup block in global memory
// cost a global round trip in each of the ~5 bookkeeping phases of a stage); elsewhere it is in global memory (fp64: 31.6 KB + 1.8 KB
// would lose the fifth workgroup per CU).  The kernels' rk_storage() places the block by the same two macros.
#define MYO_LDS_ALIGN(n) (((n) + 15) / 16 * 16)
#define MYO_RK_IN_LDS(T, NC) (sizeof(T) == 4 && (NC) == MYO_NCON_MAX)
template <typename T, bool RK, int NC>
constexpr size_t variant_lds_bytes() {
  return RK && MYO_RK_IN_LDS(T, NC) ? MYO_LDS_ALIGN(sizeof(Scratch<T, NC>)) + sizeof(RkScratch<T>) : sizeof(Scratch<T, NC>);
}

// ---- device memory of a batch.  Every allocation goes through these two: `count` elements of U (never zero bytes), recorded in
// `allocs` (what release_allocs frees), the pointer returned (null: the allocation failed).  `rc` accumulates the backend's error
// bits over a whole create; dev_upload copies only while rc is clean, so one failure leaves the rest allocated, unfilled and reported.
template <typename U>
static U* dev_alloc(std::vector<void*>& allocs, int& rc, size_t count) {
  void* p = nullptr;
  rc |= be_malloc(&p, count * sizeof(U));
  if (p) allocs.push_back(p);
  return (U*)p;
}
template <typename U>
static U* dev_upload(std::vector<void*>& allocs, int& rc, const U* host, size_t count) {
  U* p = dev_alloc<U>(allocs, rc, count);
  if (!rc && count) rc |= be_h2d(p, host, count * sizeof(U));
  return p;
}
template <typename U>
static U* dev_upload(std::vector<void*>& allocs, int& rc, const std::vector<U>& host) { return dev_upload(allocs, rc, host.data(), host.size()); }
static void release_allocs(std::vector<void*>& allocs) {
  for (void* q : allocs) be_free(q);
  allocs.clear();
}

template <typename T>
static int upload_model(const myo_model* m, DevModel<T>& D, std::vector<void*>& allocs) {
  D.nq = m->nq; D.nv = m->nv; D.nu = m->nu; D.na = m->na; D.nbody = m->nbody; D.njnt = m->njnt; D.ngeom = m->ngeom;
  D.nsite = m->nsite; D.ntendon = m->ntendon; D.nwrap = m->nwrap; D.npair = m->npair; D.nM = m->nM; D.maxdepth = m->maxdepth;
  D.integrator = m->integrator; D.iterations = m->iterations; D.disableflags = m->disableflags;
  D.any_damping = m->any_damping; D.any_tendon_passive = m->any_tendon_passive; D.nlead = m->nlead; D.ngw = m->ngw; D.nte = m->nte; D.npair_std = m->npair_std;
  D.ld_nfq = m->ld_nfq; D.ld_nsq = m->ld_nsq; D.arrow_nf = m->arrow_nf; D.arrow_pad = m->arrow_pad; D.any_rot = m->any_rot; D.any_gen = m->any_gen; D.any_floss = m->any_floss;
  D.h_timestep = m->timestep;
  D.timestep = (T)m->timestep; D.tolerance = (T)m->tolerance; D.impratio = (T)m->impratio;
  D.isqrt_impratio = (T)(1.0 / sqrt(m->impratio));
  for (int k = 0; k < 3; ++k) D.gravity[k] = (T)m->gravity[k];
  D.meaninertia = (T)m->meaninertia;
  int rc = 0;
#define X(n) D.n.p = dev_upload(allocs, rc, m->n);
  MYO_MODEL_INT_ARRAYS(X)
  MYO_MODEL_U64_ARRAYS(X)
#undef X
#define X(n) D.n.p = dev_upload(allocs, rc, std::vector<T>(m->n.begin(), m->n.end()));
  MYO_MODEL_REAL_ARRAYS(X)
#undef X
  // HP tables: the fp64 stepper's ordinary tables; separate fp64 copies for the mixed stepper
#define X(n) D.h_##n.p = sizeof(T) == sizeof(double) ? (const double*)(const void*)D.n.p : dev_upload(allocs, rc, m->n);
  MYO_MODEL_HP_ARRAYS(X)
#undef X
  return rc;
}

static void make_taskdev(const myo_task_cfg* c, uint64_t seed, TaskDev& K) {
  memset(&K, 0, sizeof K);
  K.kind = MYO_TASK_NONE; K.frame_skip = 1; K.max_episode_steps = 1 << 30;
  K.obj1_sid = K.obj2_sid = K.target1_sid = K.target2_sid = -1;
  K.obj1_bid = K.obj2_bid = K.obj1_gid = K.obj2_gid = -1;
  K.objg_gid0 = K.objg_gidn = -1;
  K.seed = seed;
  if (!c) return;
  K.kind = c->kind; K.frame_skip = c->frame_skip; K.max_episode_steps = c->max_episode_steps; K.n_hand = c->n_hand;
  K.obj1_sid = c->obj1_sid; K.obj2_sid = c->obj2_sid; K.target1_sid = c->target1_sid; K.target2_sid = c->target2_sid;
  K.obj1_bid = c->obj1_bid; K.obj2_bid = c->obj2_bid; K.obj1_gid = c->obj1_gid; K.obj2_gid = c->obj2_gid;
  K.task_choice = c->task_choice; K.enable_rsi = c->enable_rsi; K.balls_overlap = c->balls_overlap;
  K.limit_init_angle_on = c->limit_init_angle_on; K.beta_init_angle_on = c->beta_init_angle_on;
  K.beta_ball_size_on = c->beta_ball_size_on; K.beta_ball_mass_on = c->beta_ball_mass_on;
  K.drop_th = c->drop_th; K.proximity_th = c->proximity_th;
  memcpy(K.center_pos, c->center_pos, sizeof K.center_pos); memcpy(K.weights, c->weights, sizeof K.weights);
  memcpy(K.goal_time_period, c->goal_time_period, 16); memcpy(K.goal_xrange, c->goal_xrange, 16);
  memcpy(K.goal_yrange, c->goal_yrange, 16);
  K.rsi_probability = c->rsi_probability; K.overlap_probability = c->overlap_probability;
  K.noise_palm = c->noise_palm; K.noise_fingers = c->noise_fingers; K.noise_balls = c->noise_balls;
  K.limit_init_angle = c->limit_init_angle;
  memcpy(K.beta_init_angle, c->beta_init_angle, 16); memcpy(K.beta_ball_size, c->beta_ball_size, 16);
  memcpy(K.beta_ball_mass, c->beta_ball_mass, 16); memcpy(K.obj_size_range, c->obj_size_range, 16);
  memcpy(K.obj_mass_range, c->obj_mass_range, 16); memcpy(K.obj_friction_change, c->obj_friction_change, 24);
  K.init_qpos0 = c->init_qpos0;
  K.muscle_condition = c->muscle_condition; K.reaf_src = c->reaf_src; K.reaf_dst = c->reaf_dst;
  K.fatigue_F = c->fatigue_F; K.fatigue_R = c->fatigue_R; K.fatigue_r = c->fatigue_r;
  if (c->kind == MYO_TASK_REORIENT) {
    // the Baoding per-ball overrides (mass / size / friction by body and geom id) must not fire: the die is the object GROUP
    K.ro_obj_bid = c->obj1_bid; K.objg_gid0 = c->obj1_gid; K.objg_gidn = c->obj2_gid;
    K.obj1_bid = K.obj2_bid = K.obj1_gid = K.obj2_gid = -1;
    memcpy(K.ro_weights, c->ro_weights, sizeof K.ro_weights); memcpy(K.ro_goal_pos, c->ro_goal_pos, 16);
    memcpy(K.ro_goal_rot, c->ro_goal_rot, 16); memcpy(K.ro_rot_choice, c->ro_rot_choice, sizeof K.ro_rot_choice);
    for (int k = 0; k < 3; ++k) K.ro_n_rot_choice[k] = c->ro_n_rot_choice[k];
    K.ro_obj_size_change = c->ro_obj_size_change; K.ro_pos_th = c->ro_pos_th; K.ro_rot_th = c->ro_rot_th;
    memcpy(K.ro_goal_init_pos, c->ro_goal_init_pos, 24); memcpy(K.ro_goal_obj_offset, c->ro_goal_obj_offset, 24);
  }
  if (c->kind == MYO_TASK_POSE) {
    memcpy(K.pose_weights, c->pose_weights, sizeof K.pose_weights);
    K.pose_thd = c->pose_thd; K.pose_far_th = c->pose_far_th; K.pose_sds_distance = c->pose_sds_distance;
    K.pose_target_distance = c->pose_target_distance; K.pose_reset_type = c->pose_reset_type; K.pose_target_type = c->pose_target_type;
    memcpy(K.pose_init_qpos, c->pose_init_qpos, sizeof K.pose_init_qpos); memcpy(K.pose_target_value, c->pose_target_value, sizeof K.pose_target_value);
    memcpy(K.pose_target_range, c->pose_target_range, sizeof K.pose_target_range); memcpy(K.pose_reset_range, c->pose_reset_range, sizeof K.pose_reset_range);
  }
}
static_assert(MYO_TASK_REORIENT == MYO_TASK_REORIENT_K && MYO_TASK_POSE == MYO_TASK_POSE_K, "task kind ids");
static_assert(MYO_MUSCLE_FATIGUE == MYO_MUSCLE_FATIGUE_K && MYO_MUSCLE_REAFFERENTATION == MYO_MUSCLE_REAF_K, "muscle condition ids");
// the muscle_condition fields of a task cfg against the model (include/myobatch.h); a cfg without a task layer has no action map to condition
static int muscle_condition_check(const myo_model* m, const myo_task_cfg* cfg) {
  const int mc = cfg ? cfg->muscle_condition : MYO_MUSCLE_NONE;
  if (mc == MYO_MUSCLE_NONE) return MYO_OK;
  if (mc != MYO_MUSCLE_FATIGUE && mc != MYO_MUSCLE_REAFFERENTATION) return fail(MYO_E_ARG, "unknown muscle_condition %d", mc);
  if (cfg->kind == MYO_TASK_NONE) return fail(MYO_E_ARG, "muscle_condition needs a task layer (it acts between the action and ctrl)");
  if (mc == MYO_MUSCLE_REAFFERENTATION) {
    if (cfg->reaf_src < 0 || cfg->reaf_src >= m->nu || cfg->reaf_dst < 0 || cfg->reaf_dst >= m->nu || cfg->reaf_src == cfg->reaf_dst)
      return fail(MYO_E_ARG, "reafferentation: reaf_src / reaf_dst must be two different actuators of the model (nu = %d)", m->nu);
    return MYO_OK;
  }
  if (!(std::isfinite(cfg->fatigue_F) && cfg->fatigue_F >= 0 && std::isfinite(cfg->fatigue_R) && cfg->fatigue_R >= 0 && std::isfinite(cfg->fatigue_r) && cfg->fatigue_r >= 0))
    return fail(MYO_E_ARG, "fatigue: fatigue_F, fatigue_R and fatigue_r must be finite and >= 0");
  if (m->nu > 64) return fail(MYO_E_UNSUPPORTED, "fatigue: one lane per actuator, at most 64");
  for (int i = 0; i < m->nu; ++i)
    if (!(m->actuator_dynprm[10 * (size_t)i] > 0 && m->actuator_dynprm[10 * (size_t)i + 1] > 0))
      return fail(MYO_E_UNSUPPORTED, "fatigue: actuator %d has no activation / deactivation time constants (dynprm[0], dynprm[1] > 0): not a muscle", i);
  return MYO_OK;
}
static int task_nobs_host(const myo_task_cfg* c, int na) {
  if (c->kind == MYO_TASK_POSE) return 3 * c->n_hand;
  return c->kind == MYO_TASK_REORIENT ? 2 * c->n_hand + 18 + na : c->n_hand + 24 + na;
}

// ---- myo_batch_create, step by step
// a task cfg against the model, per kind, and its muscle_condition fields
static int task_cfg_check(const myo_model* m, const myo_task_cfg* cfg) {
  if (cfg && cfg->kind != MYO_TASK_NONE) {
    if (cfg->kind != MYO_TASK_BAODING_P1 && cfg->kind != MYO_TASK_BAODING_P2 && cfg->kind != MYO_TASK_REORIENT && cfg->kind != MYO_TASK_POSE)
      return fail(MYO_E_ARG, "unknown task kind");
    if (cfg->kind == MYO_TASK_POSE) {
      if (cfg->n_hand != m->nq || m->nv != m->nq || m->nq > MYO_POSE_NQ_MAX || task_nobs_host(cfg, m->na) > MYO_OBS_MAX)
        return fail(MYO_E_UNSUPPORTED, "joint-pose task needs a model of hinge / slide joints only (nq = nv = n_hand <= %d)", MYO_POSE_NQ_MAX);
      if (cfg->pose_reset_type < MYO_POSE_RESET_INIT || cfg->pose_reset_type > MYO_POSE_RESET_SDS) return fail(MYO_E_ARG, "pose_reset_type");
      if (cfg->pose_target_type != MYO_POSE_TARGET_GENERATE && cfg->pose_target_type != MYO_POSE_TARGET_FIXED) return fail(MYO_E_ARG, "pose_target_type");
    } else if (cfg->kind == MYO_TASK_REORIENT) {
      if (cfg->obj1_sid < 0 || cfg->obj1_sid >= m->nsite || cfg->target1_sid < 0 || cfg->target1_sid >= m->nsite ||
          cfg->obj1_bid <= 0 || cfg->obj1_bid >= m->nbody || cfg->obj1_gid < 0 || cfg->obj2_gid <= cfg->obj1_gid || cfg->obj2_gid > m->ngeom)
        return fail(MYO_E_ARG, "task ids out of range");
      if (cfg->obj2_gid - cfg->obj1_gid > MYO_OBJG_MAX) return fail(MYO_E_UNSUPPORTED, "the die has more than %d geoms", MYO_OBJG_MAX);
      if (cfg->n_hand + 7 != m->nq || m->nv < 6 || task_nobs_host(cfg, m->na) > MYO_OBS_MAX)
        return fail(MYO_E_UNSUPPORTED, "reorient task needs nq = n_hand + 7 (the die's free joint last) and an observation of <= %d numbers", MYO_OBS_MAX);
      for (int k = 0; k < 3; ++k)
        if (cfg->ro_n_rot_choice[k] < 0 || cfg->ro_n_rot_choice[k] > MYO_ROT_CHOICE_MAX) return fail(MYO_E_ARG, "goal_rot_x/y/z: at most %d ranges", MYO_ROT_CHOICE_MAX);
    } else {
      if (cfg->obj1_sid < 0 || cfg->obj1_sid >= m->nsite || cfg->obj2_sid < 0 || cfg->obj2_sid >= m->nsite ||
          cfg->target1_sid < 0 || cfg->target1_sid >= m->nsite || cfg->target2_sid < 0 || cfg->target2_sid >= m->nsite ||
          cfg->obj1_bid <= 0 || cfg->obj1_bid >= m->nbody || cfg->obj2_bid <= 0 || cfg->obj2_bid >= m->nbody ||
          cfg->obj1_gid < 0 || cfg->obj1_gid >= m->ngeom || cfg->obj2_gid < 0 || cfg->obj2_gid >= m->ngeom)
        return fail(MYO_E_ARG, "task ids out of range");
      if (cfg->n_hand + 14 != m->nq || m->nv < 12 || cfg->n_hand + 24 + m->na > MYO_OBS_MAX)
        return fail(MYO_E_UNSUPPORTED, "Baoding task needs nq = n_hand + 14 (two free balls last)");
    }
    if (cfg->frame_skip <= 0 || cfg->max_episode_steps <= 0) return fail(MYO_E_ARG, "frame_skip / max_episode_steps");
  }
  return muscle_condition_check(m, cfg);
}

// the env record of this batch (b->L; b->K.fat_off): a pose batch has its pose block, a batch with fatigue its muscle states
static int record_layout(myo_batch* b, const myo_model* m) {
  EnvRecordLayout& L = b->L;
  L.nq = m->nq; L.nv = m->nv; L.na = m->na;
  int o = 0;
  L.off_qpos = o; o += m->nq; L.off_qvel = o; o += m->nv; L.off_act = o; o += m->na; L.off_warm = o; o += m->nv;
  L.off_time = o; o += 1; L.off_taskd = o; o += MYO_TASKD_N; L.off_balld = o; o += MYO_BALLD_N; L.off_misc = o; o += MYO_MISC_N;
  L.off_objfric = o; o += 3 * MYO_OBJG_MAX;
  L.off_pose = o; if (b->K.kind == MYO_TASK_POSE) o += 2 * m->nq;     // (the other kinds' records keep their size)
  b->K.fat_off = o; if (b->K.muscle_condition == MYO_MUSCLE_FATIGUE) o += 3 * m->nu;      // (a batch without fatigue keeps its record's size)
  // (store_env writes qpos | qvel | act | warm | time as one run: the order above is part of the kernels' contract)
  if (L.off_qvel != L.off_qpos + m->nq || L.off_act != L.off_qvel + m->nv || L.off_warm != L.off_act + m->na || L.off_time != L.off_warm + m->nv) return fail(MYO_E_STATE, "record layout");
  L.stride = (o + 15) / 16 * 16;      // whole 128-byte lines per env: no line is shared by two workgroups
  b->K.objf_off = L.off_objfric - L.off_warm;      // (Scratch::SPILL reads the object group's friction in the record)
  return MYO_OK;
}
static void dump_layout(DumpLayout& D, const myo_model* m) {
  int o = 0;
  D.ten_length = o; o += m->ntendon; D.ten_J = o; o += m->ntendon * m->nv; D.M = o; o += m->nv * m->nv;
  D.qfrc_bias = o; o += m->nv; D.qfrc_passive = o; o += m->nv; D.qfrc_actuator = o; o += m->nv;
  D.qacc_smooth = o; o += m->nv; D.qacc = o; o += m->nv; D.actuator_force = o; o += m->nu; D.act_dot = o; o += m->na;
  D.counts = o; o += 4; D.efc_aref = o; o += MYO_NLIM_MAX + 4 * MYO_NCON_BIG; D.efc_D = o; o += MYO_NLIM_MAX + 4 * MYO_NCON_BIG;
  D.site_xpos = o; o += 3 * m->nsite; D.subtree_com = o; o += 3 * m->nbody; D.xpos = o; o += 3 * m->nbody; D.total = o;
}

// initial record of an env (r: L.stride zeros): qpos0, zero velocity; model ball parameters; target sites at their model xy;
// start angles per _setup (baoding.py:246-247 P1; :349-354 P2 decided per env at reset time here)
static void initial_record(const myo_model* m, const TaskDev& K, const EnvRecordLayout& L, double* r) {
  for (int i = 0; i < m->nq; ++i) r[L.off_qpos + i] = m->qpos0[i];
  double* td = r + L.off_taskd; double* bd = r + L.off_balld; double* mi = r + L.off_misc;
  if (K.muscle_condition == MYO_MUSCLE_FATIGUE) for (int i = 0; i < m->nu; ++i) r[K.fat_off + m->nu + i] = 1.0;      // rested muscles: (MA, MR, MF) = (0, 1, 0)
  td[0] = 3.0 * MYO_PI / 4.0; td[1] = -MYO_PI / 4.0; td[2] = 0.025; td[3] = 0.028; td[4] = 5.0;
  mi[0] = MYO_WHICH_CCW;
  if (K.kind == MYO_TASK_REORIENT) {
    // goal at its setup pose, identity orientation, nominal die; reset() draws the episode's values
    memset(td, 0, sizeof(double) * MYO_TASKD_N); mi[0] = 0;
    for (int k = 0; k < 3; ++k) td[k] = K.ro_goal_init_pos[k];
    td[3] = 1.0;
    for (int j = 0; j < 3 * (K.objg_gidn - K.objg_gid0); ++j) r[L.off_objfric + j] = m->geom_friction[3 * K.objg_gid0 + j];
  } else if (K.kind == MYO_TASK_POSE) {
    // the init pose and the pseudo target of CustomPoseEnv._setup (pose.py:38-43: the mean of each target range); reset() draws the episode's
    memset(td, 0, sizeof(double) * MYO_TASKD_N); mi[0] = 0;
    for (int i = 0; i < m->nq; ++i) {
      const double tv = K.pose_target_type == MYO_POSE_TARGET_FIXED ? K.pose_target_value[i]
                                                                     : 0.5 * (K.pose_target_range[i][0] + K.pose_target_range[i][1]);
      r[L.off_qpos + i] = K.pose_init_qpos[i];
      r[L.off_pose + i] = tv; r[L.off_pose + m->nq + i] = K.pose_init_qpos[i];
    }
  } else if (K.kind) {
    td[2] = 0.5 * (K.goal_xrange[0] + K.goal_xrange[1]); td[3] = 0.5 * (K.goal_yrange[0] + K.goal_yrange[1]);
    td[4] = 0.5 * (K.goal_time_period[0] + K.goal_time_period[1]);
    if (K.kind == MYO_TASK_BAODING_P2 && !(K.overlap_probability >= 1.0)) { td[0] = MYO_PI / 4.0; td[1] = MYO_PI / 4.0 - MYO_PI; }
    td[5] = m->site_pos[3 * K.target1_sid]; td[6] = m->site_pos[3 * K.target1_sid + 1];
    td[7] = m->site_pos[3 * K.target2_sid]; td[8] = m->site_pos[3 * K.target2_sid + 1];
    bd[0] = m->body_mass[K.obj1_bid]; bd[1] = m->body_mass[K.obj2_bid];
    for (int k = 0; k < 3; ++k) { bd[2 + k] = m->geom_friction[3 * K.obj1_gid + k]; bd[5 + k] = m->geom_friction[3 * K.obj2_gid + k]; }
    bd[8] = m->geom_size[3 * K.obj1_gid]; bd[9] = m->geom_size[3 * K.obj2_gid];
    if (K.task_choice == MYO_CHOICE_CW) mi[0] = MYO_WHICH_CW;
  }
}

// the parts of an env step (k_step): MYO_STEP_SPLIT = "7,3" (substeps per part; "0" or one number = whole steps; A/B switch
// of the tools and of the bit-identity tests).  The emulation build runs the parts one after the other through the record.
// `parts`: the batch has a task layer (a physics-only batch steps whole)
static StepPlan step_plan(int frame_skip, bool parts) {
  StepPlan whole = {}, pl = {};
  whole.nparts = 1; whole.k[1] = frame_skip;
  { const char* pm = getenv("MYO_PUBLISH"); pl.wt = pm && !strcmp(pm, "fence") ? 0 : 1; }     // A/B switch: "wt" (default) | "fence"
  if (!parts || frame_skip < 2) return whole;
  const char* sp = getenv("MYO_STEP_SPLIT");
  if (sp) {
    int acc = 0;
    for (const char* q = sp; *q && pl.nparts < MYO_PARTS_MAX;) {
      const int v = atoi(q);
      if (v <= 0) break;
      acc += v; pl.k[++pl.nparts] = acc;
      while (*q && *q != ',') ++q;
      if (*q == ',') ++q;
    }
    if (acc != frame_skip) pl.nparts = 0;
  } else {
    // parts of decreasing length, 4 : 3 : 2 : 1 of the frame_skip (measured at 4096 envs, frame_skip 10, k_step ms:
    // whole 2.73, 7+3 2.33, 6+3+1 2.27, 5+3+2 2.27, 4+3+2+1 2.24, 5+3+1+1 2.25, 3+3+2+1+1 2.26)
    const int f = frame_skip, np = f < 4 ? f : 4;
    static const int w[4] = {4, 3, 2, 1};
    int wsum = 0, acc = 0;
    for (int i = 0; i < np; ++i) wsum += w[i];
    for (int i = 0; i < np; ++i) {
      int len = i == np - 1 ? f - acc : (f * w[i] + wsum / 2) / wsum;
      const int room = f - acc - (np - 1 - i);        // every later part keeps at least one substep
      len = len < 1 ? 1 : (len > room ? room : len);
      acc += len; pl.k[i + 1] = acc;
    }
    pl.nparts = np;
  }
  return pl.nparts >= 2 ? pl : whole;
}

// render items: the task's target sites are always drawn (the Baoding targets; the die's target is a body); the tendon tables; the default camera
static int upload_render_tables(myo_batch* b, const myo_model* m, int rc) {
  std::vector<float> vis = m->vis;
  const int ts[2] = {b->K.target1_sid, b->K.target2_sid};
  if (b->K.kind == MYO_TASK_BAODING_P1 || b->K.kind == MYO_TASK_BAODING_P2)
    for (int j : ts)
      if (j >= 0 && j < m->nsite) {
        float* v = &vis[8 * (size_t)(m->ngeom + j)];
        v[5] = 0.f;
        if (!m->has_visual) { v[0] = 0.2f; v[1] = 0.85f; v[2] = 0.3f; v[3] = 1.f; v[4] = 0.01f; }
      }
  b->vis = dev_upload(b->allocs, rc, vis);
  b->nitem = m->ngeom + m->nsite;
  b->tvis = dev_upload(b->allocs, rc, m->tvis);
  b->titem_adr = dev_upload(b->allocs, rc, m->titem_adr);
  b->ntitem = m->ntendon_item;
  for (int k = 0; k < 3; ++k) b->cam_lookat[k] = m->cam_lookat[k];
  b->cam_distance = m->cam_distance;
  return rc;
}

// the one release of a batch: a finished one (myo_batch_destroy), or what a failed myo_batch_create has built so far (destroying = 0)
static void batch_release(myo_batch* b, int destroying) {
  be_batch_release(b, b->device, destroying);
  release_allocs(b->allocs);
  if (b->render_ws) be_free(b->render_ws);
  if (b->so_ws) be_free(b->so_ws);
  if (b->ik_ws) be_free(b->ik_ws);
  if (b->sim_ws) be_free(b->sim_ws);
  delete b;
}

extern "C" int myo_batch_create(const myo_model* m, const myo_task_cfg* cfg, int n_envs, int device, uint64_t seed,
                                int dtype, myo_batch** out) {
  if (!m || !out || n_envs <= 0) return fail(MYO_E_ARG, "bad arguments to myo_batch_create");
  if (dtype != MYO_F64 && dtype != MYO_F32) return fail(MYO_E_ARG, "dtype must be MYO_F64 or MYO_F32");
  if (int crc = task_cfg_check(m, cfg)) return crc;
  int rc = be_set_device(device);
  if (rc) return fail(MYO_E_DEVICE, "hipSetDevice(%d): %s", device, be_errstr(rc));
  myo_batch* b = new myo_batch();
  b->n = n_envs; b->device = device; b->dtype = dtype; b->bad_state = nullptr; b->timing = 0; b->ms_sum = 0; b->ms_cnt = 0;
  b->integrator = m->integrator;
  // contact capacity of the per-env scratch: the Baoding hand (39 candidate pairs, 11 contacts at most in the bench workload) keeps
  // the base; models with extended pairs (boxes, cylinders, ellipsoids) and the die task get the larger scratch (one workgroup
  // per CU less: 21.9 KB instead of 20.2 KB of LDS)
  // (a condim-4 / 6 contact takes two / three slots of the scratch: models that have such pairs get the big one too)
  b->ncap = (m->npair > m->npair_std || m->any_rot || (cfg && cfg->kind == MYO_TASK_REORIENT)) ? MYO_NCON_BIG : MYO_NCON_MAX;
  b->geom_friction = m->geom_friction;
  b->nq = m->nq; b->nv = m->nv; b->nu = m->nu; b->na = m->na; b->nbody = m->nbody; b->nsite = m->nsite; b->ntendon = m->ntendon; b->ngeom = m->ngeom;
  for (int i = 0; i < m->nu; ++i) b->act_reach |= m->act_dofmask[i];
  if (cfg) b->cfg = *cfg; else memset(&b->cfg, 0, sizeof b->cfg);
  make_taskdev(cfg && cfg->kind != MYO_TASK_NONE ? cfg : nullptr, seed, b->K);
  b->nobs = b->K.kind ? task_nobs_host(cfg, m->na) : 0;
  b->order = nullptr; b->cost = nullptr; b->ticks = nullptr; b->part_state = nullptr; b->step_gen = nullptr;
  memset(&b->Md, 0, sizeof b->Md); memset(&b->Mf, 0, sizeof b->Mf);
  rc = (dtype == MYO_F64) ? upload_model<double>(m, b->Md, b->allocs) : upload_model<float>(m, b->Mf, b->allocs);
  if (int lrc = record_layout(b, m)) { batch_release(b, 0); return lrc; }
  dump_layout(b->D, m);
  std::vector<double> host((size_t)n_envs * b->L.stride, 0.0);
  for (int e = 0; e < n_envs; ++e) initial_record(m, b->K, b->L, &host[(size_t)e * b->L.stride]);
  b->rec = dev_upload(b->allocs, rc, host);
  if (b->K.muscle_condition == MYO_MUSCLE_FATIGUE) {      // the muscles' time constants in fp64, whatever the stepper's arithmetic (fatigue_ctrl, csrc/myo_task.h)
    std::vector<double> tau(2 * (size_t)m->nu);
    for (int i = 0; i < m->nu; ++i) { tau[2 * i] = m->actuator_dynprm[10 * (size_t)i]; tau[2 * i + 1] = m->actuator_dynprm[10 * (size_t)i + 1]; }
    b->K.fatigue_tau = dev_upload(b->allocs, rc, tau);
  }
  const int zero4[4] = {0, 0, 0, 0};           // health counters (myo_batch_health), zeroed
  b->K.health = dev_upload(b->allocs, rc, zero4, 4);
  if (dtype == MYO_F64) rc |= be_batch_workspaces(b, n_envs, device);      // the fp64 stepper keeps controls, moment arms and the warm start in global memory (ScratchPoses<double>::ctrl_g)
  if (m->integrator == 1) {        // RK4 stage storage, one RkScratch per env (global memory)
    const size_t each = dtype == MYO_F64 ? sizeof(RkScratch<double>) : sizeof(RkScratch<float>);
    b->K.rk_ws = dev_alloc<char>(b->allocs, rc, each * (size_t)n_envs * MYO_PARTS_MAX);      // indexed by workgroup: a step in P parts launches P n of them
  }
  b->plan = step_plan(cfg ? cfg->frame_skip : 0, b->K.kind != MYO_TASK_NONE);
  if (!rc) rc = upload_render_tables(b, m, rc);
  rc = be_batch_launch_state(b, m, n_envs, rc);      // (the HIP backend: timing events, launch order, the step plan's state, the wrap census)
  if (rc) {
    const int r2 = fail(MYO_E_DEVICE, "device allocation/upload failed: %s", be_errstr(rc));
    batch_release(b, 0);
    return r2;
  }
  *out = b;
  return MYO_OK;
}

extern "C" void myo_batch_destroy(myo_batch* b) {
  if (b) batch_release(b, 1);
}
// ---- rendering (include/myobatch.h; csrc/myo_render.h): checks, cameras, style and workspace; the entry points are further down
extern "C" int myo_model_default_camera(const myo_model* m, myo_render_camera* out) {
  if (!m || !out) return fail(MYO_E_ARG, "myo_model_default_camera: null argument");
  for (int k = 0; k < 3; ++k) out->lookat[k] = m->cam_lookat[k];
  out->distance = m->cam_distance;
  out->azimuth = 90.0; out->elevation = -45.0; out->fovy = 45.0;      // MuJoCo 2.1's mjVisual.global defaults [3P-RECALL]
  return MYO_OK;
}
// myo_batch_tendon_paths / _contact_items (`fn`): null output / k < 0 / null list are refused before any device call; k = 0, or a
// model without tendon items, is then an empty result (the caller's test)
static int items_check(const myo_batch* b, const int32_t* env_idx, int k, const double* out, const char* fn) {
  if (!b) return fail(MYO_E_ARG, "%s: null batch", fn);
  if (k < 0) return fail(MYO_E_ARG, "%s: k must be >= 0, got %d", fn, k);
  if (!out) return fail(MYO_E_ARG, "%s: null output", fn);
  if (k > 0 && !env_idx) return fail(MYO_E_ARG, "%s: null env_idx", fn);
  return MYO_OK;
}
static int render_check_items(const myo_batch* b, const int32_t* env_idx, int k, const char* fn) {
  if (!b) return fail(MYO_E_ARG, "%s: null batch", fn);
  if (!env_idx || k <= 0) return fail(MYO_E_ARG, "%s: env_idx must list k >= 1 envs", fn);
  if (b->nitem > MYO_RITEM_MAX) return fail(MYO_E_UNSUPPORTED, "%s: %d geoms + sites, at most %d can be drawn", fn, b->nitem, MYO_RITEM_MAX);
  return MYO_OK;
}
// cameras -> the device table's layout (MYO_RCAM_N doubles: pos, forward, right, up, focal length in pixels), MuJoCo's free camera:
// forward = (cos el cos az, cos el sin az, sin el), up = (-sin el cos az, -sin el sin az, cos el), pos = lookat - distance forward
static int render_cameras(const myo_render_camera* cams, int ncams, int height, std::vector<double>& out) {
  out.assign((size_t)ncams * MYO_RCAM_N, 0.0);
  for (int c = 0; c < ncams; ++c) {
    const myo_render_camera& C = cams[c];
    const double d2r = 3.14159265358979323846 / 180.0;
    bool finite = std::isfinite(C.distance) && std::isfinite(C.azimuth) && std::isfinite(C.elevation) && std::isfinite(C.fovy);
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(C.lookat[k]);
    if (!finite || !(C.distance > 0) || !(C.fovy > 0 && C.fovy < 180) || fabs(C.elevation) > 90)
      return fail(MYO_E_ARG, "myo_batch_render: camera %d: distance must be > 0, fovy in (0, 180), |elevation| <= 90, all finite", c);
    const double ca = cos(C.azimuth * d2r), sa = sin(C.azimuth * d2r), ce = cos(C.elevation * d2r), se = sin(C.elevation * d2r);
    const double fw[3] = {ce * ca, ce * sa, se}, up[3] = {-se * ca, -se * sa, ce};
    const double rt[3] = {fw[1] * up[2] - fw[2] * up[1], fw[2] * up[0] - fw[0] * up[2], fw[0] * up[1] - fw[1] * up[0]};
    double* o = &out[(size_t)c * MYO_RCAM_N];
    for (int k = 0; k < 3; ++k) { o[k] = C.lookat[k] - C.distance * fw[k]; o[3 + k] = fw[k]; o[6 + k] = rt[k]; o[9 + k] = up[k]; }
    o[12] = 0.5 * height / tan(0.5 * C.fovy * d2r);
  }
  return MYO_OK;
}
// the style of the contact items: held per batch, read by the next contact item pass / render with MYO_RENDER_CONTACTS
extern "C" int myo_batch_set_render_style(myo_batch* b, const myo_render_style* st) {
  if (!b || !st) return fail(MYO_E_ARG, "myo_batch_set_render_style: null batch or style");
  if (st->size != sizeof(myo_render_style)) return fail(MYO_E_ARG, "myo_batch_set_render_style: myo_render_style.size is %zu, this library's struct has %zu bytes", st->size, sizeof(myo_render_style));
  const double len[4] = {st->disc_radius, st->disc_half_height, st->force_radius, st->metres_per_newton};
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(len[k]) || len[k] < 0) return fail(MYO_E_ARG, "myo_batch_set_render_style: radii, half height and metres_per_newton must be finite and >= 0");
  bool ok = st->geom_alpha >= 0 && st->geom_alpha <= 1;
  for (int k = 0; k < 4; ++k) ok = ok && st->point_rgba[k] >= 0.f && st->point_rgba[k] <= 1.f && st->force_rgba[k] >= 0.f && st->force_rgba[k] <= 1.f;
  if (!ok) return fail(MYO_E_ARG, "myo_batch_set_render_style: colour components and geom_alpha must be in [0, 1]");
  b->style = *st;
  return MYO_OK;
}
extern "C" int myo_batch_get_render_style(const myo_batch* b, myo_render_style* st) {
  if (!b || !st) return fail(MYO_E_ARG, "myo_batch_get_render_style: null batch or style");
  if (st->size != sizeof(myo_render_style)) return fail(MYO_E_ARG, "myo_batch_get_render_style: myo_render_style.size is %zu, this library's struct has %zu bytes", st->size, sizeof(myo_render_style));
  *st = b->style;
  return MYO_OK;
}
// the render workspace (laid out by render_plan below), in doubles; grown on demand
static int render_workspace(myo_batch* b, size_t doubles) {
  if (b->render_ws_bytes >= doubles * sizeof(double)) return MYO_OK;
  if (b->render_ws) { be_free(b->render_ws); b->render_ws = nullptr; b->render_ws_bytes = 0; }
  void* p = nullptr;
  const int e = be_malloc(&p, doubles * sizeof(double));
  if (e || !p) return fail(MYO_E_DEVICE, "myo_batch_render: workspace allocation failed: %s", be_errstr(e));
  b->render_ws = (double*)p; b->render_ws_bytes = doubles * sizeof(double);
  return MYO_OK;
}
extern "C" int myo_batch_num_envs(const myo_batch* b) { return b ? b->n : -1; }
extern "C" int myo_batch_obs_dim(const myo_batch* b) { return b ? b->nobs : -1; }
extern "C" int myo_batch_lds_bytes(const myo_batch* b) {
  if (!b) return -1;
  return with_variant(b, [](auto v) { using V = decltype(v); return (int)variant_lds_bytes<typename V::T, V::RK, V::NC>(); });
}
extern "C" int myo_batch_dump_size(const myo_batch* b) { return b ? b->D.total : -1; }
extern "C" int myo_batch_dump_offset(const myo_batch* b, const char* n) {
  if (!b || !n) return -1;
#define S(x) if (!strcmp(n, #x)) return b->D.x;
  S(ten_length) S(ten_J) S(M) S(qfrc_bias) S(qfrc_passive) S(qfrc_actuator) S(qacc_smooth) S(qacc) S(actuator_force)
  S(act_dot) S(counts) S(efc_aref) S(efc_D) S(site_xpos) S(subtree_com) S(xpos)
#undef S
  return -1;
}

// ---- the entry points that only read or write env records: the same in both backends (include/myobatch.h documents them)
static int batch_check(const myo_batch* b) { return b ? MYO_OK : fail(MYO_E_ARG, "null batch"); }
extern "C" int myo_batch_get_state(myo_batch* b, double* qpos, double* qvel, double* act, double* time, void* stream) {
  if (int rc = batch_check(b)) return rc;
  be_xfer(b, b->L.off_qpos, b->nq, qpos, 1, stream); be_xfer(b, b->L.off_qvel, b->nv, qvel, 1, stream);
  be_xfer(b, b->L.off_act, b->na, act, 1, stream); be_xfer(b, b->L.off_time, 1, time, 1, stream);
  return be_launch_status();
}
extern "C" int myo_batch_set_state(myo_batch* b, const double* qpos, const double* qvel, const double* act,
                                   const double* time, void* stream) {
  if (int rc = batch_check(b)) return rc;
  be_xfer(b, b->L.off_qpos, b->nq, (double*)qpos, 0, stream); be_xfer(b, b->L.off_qvel, b->nv, (double*)qvel, 0, stream);
  be_xfer(b, b->L.off_act, b->na, (double*)act, 0, stream); be_xfer(b, b->L.off_time, 1, (double*)time, 0, stream);
  return be_launch_status();
}
extern "C" int myo_batch_set_bad_state_buffer(myo_batch* b, uint8_t* bad_state) {
  if (int rc = batch_check(b)) return rc;
  b->bad_state = bad_state;
  return MYO_OK;
}
extern "C" int myo_batch_warmstart(myo_batch* b, double* get_w, const double* set_w, void* stream) {
  if (int rc = batch_check(b)) return rc;
  be_xfer(b, b->L.off_warm, b->nv, get_w, 1, stream); be_xfer(b, b->L.off_warm, b->nv, (double*)set_w, 0, stream);
  return be_launch_status();
}
// task_i, task_d and ball_d of myo_batch_set_task / _get_task; what task_d is depends on the task kind
static void task_xfer(myo_batch* b, int32_t* task_i, double* task_d, double* ball_d, int to_ext, void* stream) {
  be_xfer_i(b, b->L.off_misc, 2, (int*)task_i, to_ext, stream);
  if (b->K.kind == MYO_TASK_POSE) be_xfer(b, b->L.off_pose, 2 * b->nq, task_d, to_ext, stream);     // target_qpos | init_qpos
  else be_xfer(b, b->L.off_taskd, MYO_TASKD_N, task_d, to_ext, stream);
  be_xfer(b, b->L.off_balld, MYO_BALLD_N, ball_d, to_ext, stream);
}
extern "C" int myo_batch_set_task(myo_batch* b, const int32_t* task_i, const double* task_d, const double* ball_d, void* stream) {
  if (int rc = batch_check(b)) return rc;
  task_xfer(b, (int32_t*)task_i, (double*)task_d, (double*)ball_d, 0, stream);
  return be_launch_status();
}
extern "C" int myo_batch_get_task(myo_batch* b, int32_t* task_i, double* task_d, double* ball_d, void* stream) {
  if (int rc = batch_check(b)) return rc;
  task_xfer(b, task_i, task_d, ball_d, 1, stream);
  return be_launch_status();
}
extern "C" int myo_batch_set_object_group(myo_batch* b, int gid0, int gidn) {
  if (int rc = batch_check(b)) return rc;
  if (!(gid0 == -1 && gidn == -1) && (gid0 < 0 || gidn <= gid0 || gidn > b->ngeom)) return fail(MYO_E_ARG, "bad geom range");
  if (b->K.kind != MYO_TASK_NONE) return fail(MYO_E_STATE, "object groups are for physics-only batches (the reorient task owns its own; the Baoding tasks have the two balls)");
  if (gidn - gid0 > MYO_OBJG_MAX) return fail(MYO_E_UNSUPPORTED, "an object group holds at most %d geoms", MYO_OBJG_MAX);
  b->K.objg_gid0 = gid0; b->K.objg_gidn = gidn;
  std::vector<void*> tmp;      // (the upload lives until the scatter has run: be_task_changed waits for it)
  if (gidn > 0) {   // every env starts from the model's friction of the group's geoms
    const int cnt = 3 * (gidn - gid0);
    std::vector<double> host((size_t)b->n * cnt);
    for (int e = 0; e < b->n; ++e) for (int j = 0; j < cnt; ++j) host[(size_t)e * cnt + j] = b->geom_friction[3 * gid0 + j];
    int rc = 0;
    double* dev = dev_upload(tmp, rc, host);
    if (rc) { release_allocs(tmp); return fail(MYO_E_DEVICE, "object group upload failed: %s", be_errstr(rc)); }
    be_xfer(b, b->L.off_objfric, cnt, dev, 0, nullptr);
  }
  be_task_changed(b);
  release_allocs(tmp);
  return MYO_OK;
}
extern "C" int myo_batch_object_friction(myo_batch* b, const double* set_fric, double* get_fric, void* stream) {
  if (int rc = batch_check(b)) return rc;
  if (b->K.objg_gidn <= 0) return fail(MYO_E_STATE, "batch has no object group");
  const int cnt = 3 * (b->K.objg_gidn - b->K.objg_gid0);
  be_xfer(b, b->L.off_objfric, cnt, (double*)set_fric, 0, stream); be_xfer(b, b->L.off_objfric, cnt, get_fric, 1, stream);
  return be_launch_status();
}
extern "C" int myo_batch_fatigue(myo_batch* b, const double* set_state, double* get_state, void* stream) {
  if (int rc = batch_check(b)) return rc;
  if (b->K.muscle_condition != MYO_MUSCLE_FATIGUE) return fail(MYO_E_ARG, "myo_batch_fatigue: the batch was made without muscle_condition = MYO_MUSCLE_FATIGUE");
  be_xfer(b, b->K.fat_off, 3 * b->nu, (double*)set_state, 0, stream); be_xfer(b, b->K.fat_off, 3 * b->nu, get_state, 1, stream);
  return be_launch_status();
}
extern "C" int myo_batch_enable_timing(myo_batch* b, int on) {
  if (int rc = batch_check(b)) return rc;
  b->timing = on;
  return MYO_OK;
}

// ---- the entry points that launch: each written once, over the backend primitives (be_run and the others declared at the top)
static int task_layer_check(const myo_batch* b) { return b->K.kind ? MYO_OK : fail(MYO_E_STATE, "batch has no task layer"); }
extern "C" int myo_batch_bind_constants(myo_batch* b, void* stream) {
  if (int rc = batch_check(b)) return rc;
  return be_bind(b, stream);
}
// census of the wraps over the envs' present states, then the new order (both on the stream: usable between any two steps, also while
// a graph of steps exists — the tables are rewritten in place)
extern "C" int myo_batch_tune_wrap_order(myo_batch* b, void* stream) {
  if (int rc = batch_check(b)) return rc;
  return be_wrap_order(b, stream);
}
extern "C" int myo_batch_reset(myo_batch* b, const uint8_t* mask, float* obs, void* stream) {
  if (int rc = batch_check(b)) return rc;
  if (int rc = task_layer_check(b)) return rc;
  if (int rc = be_run(b, ResetJob{mask, obs}, b->n, stream)) return rc;
  if (mask) return MYO_OK;
  b->wrap_tune_in = 16;                 // a reset of every env: the wrap order from the reset states, again 16 steps on
  return be_wrap_order(b, stream);
}
extern "C" int myo_batch_step(myo_batch* b, const float* act, float* obs, float* rew, uint8_t* done, uint8_t* trunc,
                              float* term_obs, float* comps, float* ep_info, void* stream) {
  if (!b || !act || !obs || !rew || !done) return fail(MYO_E_ARG, "myo_batch_step: act/obs/rew/done are required");
  if (int rc = task_layer_check(b)) return rc;
  return be_step(b, act, obs, rew, done, trunc, term_obs, comps, ep_info, stream);
}
// test hook: put the step plan's generation counter (and every env's state, consistently) at `gen` — the counter wraps after
// 2^28 steps and the protocol's arithmetic is modulo 2^32 (tests/test_step_parts.py steps across the wrap)
extern "C" int myo_batch_set_step_generation(myo_batch* b, unsigned int gen) {
  if (int rc = batch_check(b)) return rc;
  return b->part_state ? be_set_step_generation(b, gen) : MYO_OK;
}
// Health counters of a batch (synchronises the device).  out[0]: k_step workgroups that found their env's hand-off state in another
// generation than the launch's (see the protocol comment at k_step); out[1]: substeps in which an env had more contacts than its
// scratch holds (the surplus was dropped); out[2]: the same for limit rows; out[3]: the most contact slots such a substep asked for.
// All 0 in a healthy batch, and in one without counters.
extern "C" int myo_batch_health(myo_batch* b, int out[4]) {
  if (!b || !out) return fail(MYO_E_ARG, "null argument");
  for (int k = 0; k < 4; ++k) out[k] = 0;
  return b->K.health ? be_health(b, out) : MYO_OK;
}
// Device check of what the per-slot workspace rests on (myo_wave_slot, wave.h): `n_workgroups` one-wave workgroups with `lds_bytes` of
// dynamic LDS (k_step's footprint: the same residency) each take their slot's occupancy counter, stay for ~20 us, and leave.
// out[0]: workgroups that found their slot occupied (must be 0); out[1]: distinct slots seen; out[2]: largest slot index; out[3]: bit mask of XCC ids.
extern "C" int myo_debug_wave_slots(int device, int n_workgroups, int lds_bytes, int32_t out[4]) {
  if (!out || n_workgroups <= 0 || lds_bytes < 0 || lds_bytes > 65536) return fail(MYO_E_ARG, "bad argument");
  return be_wave_slots(device, n_workgroups, lds_bytes, out);
}
extern "C" int myo_batch_step_inner(myo_batch* b, const uint8_t* mask, const float* act, float* obs, uint8_t* done, void* stream) {
  if (!b || !act || !obs) return fail(MYO_E_ARG, "myo_batch_step_inner: act/obs are required");
  if (int rc = task_layer_check(b)) return rc;
  return be_run(b, StepInnerJob{mask, act, obs, done}, b->n, stream);
}
// Compact form of myo_batch_step_inner: the envs idx[0 .. n_idx) (dev int32; -1 = empty slot) take one unwrapped env step with
// row r of act [n_idx, nu]; row r of obs [n_idx, obs_dim] and done [n_idx] (may be NULL) receive env idx[r]'s results.  An env
// must not be listed twice.  MixtureModelBaodingEnv's base phase runs the few envs that were just reset this way.
extern "C" int myo_batch_step_inner_idx(myo_batch* b, const int* idx, int n_idx, const float* act, float* obs, uint8_t* done, void* stream) {
  if (!b || !idx || !act || !obs || n_idx <= 0) return fail(MYO_E_ARG, "myo_batch_step_inner_idx: idx/act/obs are required");
  if (int rc = task_layer_check(b)) return rc;
  return be_run(b, StepInnerIdxJob{idx, act, obs, done}, n_idx, stream);
}
// Whole env records from one batch into another (same model, same task kind): dst env dst_idx[r] <- src env src_idx[r], r < k.
// The record is everything an env is between two steps (state, warm start, task scalars, per-episode draws, counters), so the
// destination env continues exactly where the source env stood.  MixtureModelBaodingEnv hands pre-played episodes (reset + base
// phase, done in bulk on a pool batch) to the envs that have just finished.  k = 0 is an empty copy.
extern "C" int myo_batch_copy_envs(myo_batch* dst, const int* dst_idx, const myo_batch* src, const int* src_idx, int k, void* stream) {
  if (!dst || !src || !dst_idx || !src_idx || k < 0) return fail(MYO_E_ARG, "myo_batch_copy_envs: null argument");
  if (dst->L.stride != src->L.stride || dst->nq != src->nq || dst->nv != src->nv || dst->na != src->na || dst->K.kind != src->K.kind || dst->device != src->device ||
      dst->K.muscle_condition != src->K.muscle_condition)
    return fail(MYO_E_ARG, "myo_batch_copy_envs: the two batches differ in model, task kind, muscle condition or device");
  return k ? be_copy_envs(dst, dst_idx, src, src_idx, k, stream) : MYO_OK;
}
extern "C" int myo_batch_physics_step(myo_batch* b, const double* ctrl, int nsub, void* stream) {
  if (!b || nsub < 0) return fail(MYO_E_ARG, "bad arguments");
  return be_run(b, PhysicsJob{ctrl, nsub}, b->n, stream, 1);
}
extern "C" int myo_batch_forward_dump(myo_batch* b, const double* ctrl, double* out, void* stream) {
  if (!b || !out) return fail(MYO_E_ARG, "bad arguments");
  return be_run(b, DumpJob{ctrl, b->D, out}, b->n, stream);
}
// the sense rows of the variant table: SenseJob / env_sense exist per arithmetic and contact capacity, keyed as k_step is (the integrator
// does not enter: a forward pass integrates nothing); a row's capacity is its scratch's record slots
static int sense_capacity(const myo_batch* b) {
  return with_variant(b, [](auto v) { using V = decltype(v); return (int)Scratch<typename V::T, V::NC>::NREC; });
}
static SenseDev sense_dev(const myo_batch* b, const myo_sense_out* o) {
  SenseDev d;
  d.ncon = o->ncon; d.con_geom = o->con_geom; d.con_d = o->con_d; d.body_wrench = o->body_wrench; d.qfrc_constraint = o->qfrc_constraint;
  d.act_length = o->act_length; d.act_velocity = o->act_velocity; d.act_force = o->act_force; d.activation = o->activation;
  d.ten_length = o->ten_length; d.ten_velocity = o->ten_velocity;
  d.cap = sense_capacity(b);
  return d;
}
extern "C" int myo_batch_contact_capacity(const myo_batch* b) { return b ? sense_capacity(b) : -1; }
// the compact temporaries of a contact item pass over k envs (csrc/myo_render.h env_contact_items), in doubles at `base`:
// con_d [k, cap, 13], then ncon int32 [k]
static size_t contact_tmp_doubles(const myo_batch* b, int k) { return (size_t)k * sense_capacity(b) * MYO_SENSE_CON_N + ((size_t)k + 1) / 2; }
static SenseDev contact_tmp(const myo_batch* b, int k, double* base) {
  SenseDev d = {};
  d.cap = sense_capacity(b);
  d.con_d = base;
  d.ncon = (int*)(base + (size_t)k * d.cap * MYO_SENSE_CON_N);
  return d;
}
// the three item passes of a batch (csrc/myo_render.h) over the envs idx[0 .. k) into `out`; tmp: the contact pass's temporaries,
// contact_tmp_doubles(b, k) doubles
static GeomPass geom_pass(const myo_batch* b, const int* idx, double* out) { return {idx, out, b->nitem, b->vis}; }
static TendonPass tendon_pass(const myo_batch* b, const int* idx, double* out) { return {idx, out, b->ntitem, b->tvis, b->titem_adr}; }
static ContactPass contact_pass(const myo_batch* b, const int* idx, int k, double* tmp, double* out) {
  return {idx, out, 2 * sense_capacity(b), contact_tmp(b, k, tmp), b->style};
}
// What a myo_batch_render call of k envs runs, and its workspace (offsets in doubles, the same on both backends): the geoms' table
// [k, nitem], the tendons' [k, ntitem] (ntitem = 0: not drawn — no flag, or a model without tendon items), the contacts' [k, ncitem]
// (0: no MYO_RENDER_CONTACTS), the cameras, the contact pass's temporaries.  A table of n > 0 rows has its item pass run.  layered:
// the cast (be_cast) is the layered one over the tables that are there (render_layers), else the plain one over the geoms'; nmax sizes
// the cast's LDS table.
struct RenderPlan { size_t tendons, contacts, cams, tmp, total; int ntitem, ncitem, nmax; bool layered; };
static RenderPlan render_plan(const myo_batch* b, int k, int flags, size_t ncam_doubles) {
  RenderPlan p;
  const bool contacts = (flags & MYO_RENDER_CONTACTS) != 0;
  p.ntitem = (flags & MYO_RENDER_TENDONS) ? b->ntitem : 0;
  p.ncitem = contacts ? 2 * sense_capacity(b) : 0;
  p.nmax = std::max(b->nitem, std::max(p.ntitem, p.ncitem));
  p.layered = p.ntitem > 0 || contacts;
  p.tendons = (size_t)k * b->nitem * MYO_RENDER_ITEM_N;
  p.contacts = p.tendons + (size_t)k * p.ntitem * MYO_RENDER_ITEM_N;
  p.cams = p.contacts + (size_t)k * p.ncitem * MYO_RENDER_ITEM_N;
  p.tmp = p.cams + ncam_doubles;
  p.total = p.tmp + (contacts ? contact_tmp_doubles(b, k) : 0);
  return p;
}
// the layers of a layered plan whose workspace is at `ws`; without contacts the geoms stay opaque (x * 1.0f is exact)
static RLayers render_layers(const myo_batch* b, const RenderPlan& p, const double* ws) {
  RLayers Y = {};
  Y.l[Y.nl++] = {ws, b->nitem, 0};
  if (p.ntitem > 0) Y.l[Y.nl++] = {ws + p.tendons, p.ntitem, b->nitem};
  if (p.ncitem > 0) Y.l[Y.nl++] = {ws + p.contacts, p.ncitem, b->nitem + b->ntendon};
  Y.ngeom = b->ngeom;
  Y.geom_alpha = p.ncitem > 0 ? (float)b->style.geom_alpha : 1.f;
  return Y;
}
// myo_batch_sense (csrc/myo_sense.h): the struct's size is its version.  A k_step launch runs every part of an env step, so a call that is
// stream-ordered behind the steps never meets an env between two parts of one.
extern "C" int myo_batch_sense(myo_batch* b, const myo_sense_out* out, void* stream) {
  if (!b || !out) return fail(MYO_E_BADARG, "myo_batch_sense: null batch or output struct");
  if (out->size != sizeof(myo_sense_out)) return fail(MYO_E_BADARG, "myo_batch_sense: myo_sense_out.size is %zu, this library's struct has %zu bytes", out->size, sizeof(myo_sense_out));
  return be_run(b, SenseJob{sense_dev(b, out)}, b->n, stream);
}
// myo_batch_data (csrc/myo_data.h): the last stage a non-null pointer needs travels in the job; a struct without one launches nothing
extern "C" int myo_batch_data(myo_batch* b, const double* ctrl, const myo_data_out* out, void* stream) {
  if (!b || !out) return fail(MYO_E_BADARG, "myo_batch_data: null batch or output struct");
  if (out->size != sizeof(myo_data_out)) return fail(MYO_E_BADARG, "myo_batch_data: myo_data_out.size is %zu, this library's struct has %zu bytes", out->size, sizeof(myo_data_out));
  DataDev d = {out->xpos, out->xquat, out->xmat, out->xipos, out->subtree_com, out->geom_xpos, out->geom_xmat, out->site_xpos, out->cvel, out->qM,
               out->ten_J, out->actuator_moment, out->qfrc_bias, out->qfrc_passive, out->qfrc_actuator, out->qacc_smooth, out->qacc, out->act_dot, ctrl, -1};
  if (d.xpos || d.xquat || d.xmat || d.xipos || d.subtree_com || d.geom_xpos || d.geom_xmat || d.site_xpos || d.ten_J || d.actuator_moment) d.stage = MYO_DATA_POS;
  if (d.qM) d.stage = MYO_DATA_INERTIA;
  if (d.cvel || d.qfrc_bias || d.qfrc_passive) d.stage = MYO_DATA_VEL;
  if (d.qfrc_actuator || d.act_dot) d.stage = MYO_DATA_ACT;
  if (d.qacc_smooth) d.stage = MYO_DATA_SMOOTH;
  if (d.qacc) d.stage = MYO_DATA_CONSTRAINED;
  if (d.stage < 0) return MYO_OK;
  return be_run(b, DataJob{d}, b->n, stream);
}
// myo_batch_jac / myo_batch_inverse (csrc/myo_jac.h): JacJob / InverseJob are rows of the variant table like SenseJob / DataJob, keyed
// without the integrator.  The per-body ancestor-dof masks env_jac selects columns by are the model's body_dofmask (built with the
// other derived tables above, uploaded with the model).  The object ids live on the device: an id outside the model gets zero blocks.
static_assert((int)MYO_JAC_BODY == (int)MYO_JAC_K_BODY && (int)MYO_JAC_BODYCOM == (int)MYO_JAC_K_BODYCOM && (int)MYO_JAC_SITE == (int)MYO_JAC_K_SITE &&
              (int)MYO_JAC_GEOM == (int)MYO_JAC_K_GEOM && (int)MYO_JAC_SUBTREECOM == (int)MYO_JAC_K_SUBTREECOM, "object types of include/myobatch.h and csrc/myo_jac.h");
extern "C" int myo_batch_jac(myo_batch* b, int objtype, const int32_t* obj_ids, int k, const double* points, const myo_jac_out* out, void* stream) {
  if (!b || !out) return fail(MYO_E_BADARG, "myo_batch_jac: null batch or output struct");
  if (out->size != sizeof(myo_jac_out)) return fail(MYO_E_BADARG, "myo_batch_jac: myo_jac_out.size is %zu, this library's struct has %zu bytes", out->size, sizeof(myo_jac_out));
  if (objtype < MYO_JAC_BODY || objtype > MYO_JAC_SUBTREECOM) return fail(MYO_E_ARG, "myo_batch_jac: unknown object type %d", objtype);
  if (k < 0 || (k > 0 && !obj_ids)) return fail(MYO_E_ARG, "myo_batch_jac: k must be >= 0 and obj_ids non-null");
  if (points && objtype != MYO_JAC_BODY) return fail(MYO_E_ARG, "myo_batch_jac: points go with MYO_JAC_BODY only");
  if (objtype == MYO_JAC_SUBTREECOM && out->jacr) return fail(MYO_E_ARG, "myo_batch_jac: MYO_JAC_SUBTREECOM has no jacr");
  if ((long long)k * 3 * b->nv > (1ll << 31) - 1) return fail(MYO_E_ARG, "myo_batch_jac: k * 3 * nv exceeds 2^31");
  if ((!out->jacp && !out->jacr) || k == 0) return MYO_OK;
  return be_run(b, JacJob{{objtype, k, obj_ids, points, out->jacp, out->jacr}}, b->n, stream);
}
extern "C" int myo_batch_inverse(myo_batch* b, const double* qacc, const myo_inverse_out* out, void* stream) {
  if (!b || !out) return fail(MYO_E_BADARG, "myo_batch_inverse: null batch or output struct");
  if (out->size != sizeof(myo_inverse_out)) return fail(MYO_E_BADARG, "myo_batch_inverse: myo_inverse_out.size is %zu, this library's struct has %zu bytes", out->size, sizeof(myo_inverse_out));
  if (!qacc) return fail(MYO_E_BADARG, "myo_batch_inverse: qacc is required");
  if (!out->qfrc_inverse && !out->qfrc_constraint) return MYO_OK;
  return be_run(b, InverseJob{{qacc, out->qfrc_inverse, out->qfrc_constraint}}, b->n, stream);
}
// myo_batch_static_opt (csrc/myo_static_opt.h): StaticOptJob is a row of the variant table like InverseJob.  The default weight is a
// structural property of the model (act_reach, built with the batch); the system matrices live in a workspace of the batch's own,
// allocated by the first call that solves.  Every array lives on the device: the host refuses what it can see.
static_assert((int)MYO_STATIC_OPT_CAP == (int)MYO_SO_ST_CAP && (int)MYO_STATIC_OPT_PINNED == (int)MYO_SO_ST_PINNED, "status bits of include/myobatch.h and csrc/myo_static_opt.h");
extern "C" int myo_batch_static_opt(myo_batch* b, const myo_static_opt_in* in, const myo_static_opt_out* out, void* stream) {
  if (!b || !in || !out) return fail(MYO_E_BADARG, "myo_batch_static_opt: null batch, input or output struct");
  if (in->size != sizeof(myo_static_opt_in)) return fail(MYO_E_BADARG, "myo_batch_static_opt: myo_static_opt_in.size is %zu, this library's struct has %zu bytes", in->size, sizeof(myo_static_opt_in));
  if (out->size != sizeof(myo_static_opt_out)) return fail(MYO_E_BADARG, "myo_batch_static_opt: myo_static_opt_out.size is %zu, this library's struct has %zu bytes", out->size, sizeof(myo_static_opt_out));
  const bool solve = out->u || out->force || out->qfrc || out->residual || out->kkt || out->iters || out->status;
  if (!solve && !out->gain && !out->bias) return MYO_OK;
  StaticOptDev d{};
  d.gain = out->gain; d.bias = out->bias; d.lower = in->lower; d.upper = in->upper; d.u_ref = in->u_ref;
  d.reg = 1; d.max_iter = 1;
  if (solve) {
    if (!in->qfrc) return fail(MYO_E_BADARG, "myo_batch_static_opt: qfrc is required");
    if (!(in->reg > 0) || !std::isfinite(in->reg)) return fail(MYO_E_ARG, "myo_batch_static_opt: reg must be finite and > 0");
    if (in->max_iter < 1) return fail(MYO_E_ARG, "myo_batch_static_opt: max_iter must be >= 1");
    if (!b->so_ws) {
      void* p = nullptr;
      const int e = be_malloc(&p, (size_t)b->n * MYO_SO_WS_N * sizeof(double));
      if (e || !p) return fail(MYO_E_DEVICE, "myo_batch_static_opt: workspace allocation failed: %s", be_errstr(e));
      b->so_ws = (double*)p;
    }
    d.qfrc = in->qfrc; d.weight = in->weight; d.weight_per_env = in->weight && in->weight_per_env ? 1 : 0;
    d.u = out->u; d.force = out->force; d.qfrc_out = out->qfrc; d.residual = out->residual; d.kkt = out->kkt; d.iters = out->iters; d.status = out->status;
    d.ws = b->so_ws; d.reach = b->act_reach; d.reg = in->reg; d.max_iter = in->max_iter; d.solve = 1;
  }
  return be_run(b, StaticOptJob{d}, b->n, stream);
}
// myo_batch_ik (csrc/myo_ik.h): IkJob is a row of the variant table like StaticOptJob; the system matrix, the Jacobian and the site
// points of the accepted iterate live in a workspace of the batch's own, allocated by the first call.  Every array lives on the
// device: the host refuses what it can see.
static_assert((int)MYO_IK_CAP == (int)MYO_IK_ST_CAP && (int)MYO_IK_STALL == (int)MYO_IK_ST_STALL && (int)MYO_IK_PINNED == (int)MYO_IK_ST_PINNED, "status bits of include/myobatch.h and csrc/myo_ik.h");
extern "C" int myo_batch_ik(myo_batch* b, const myo_ik_in* in, const myo_ik_out* out, void* stream) {
  if (!b || !in || !out) return fail(MYO_E_BADARG, "myo_batch_ik: null batch, input or output struct");
  if (in->size != sizeof(myo_ik_in)) return fail(MYO_E_BADARG, "myo_batch_ik: myo_ik_in.size is %zu, this library's struct has %zu bytes", in->size, sizeof(myo_ik_in));
  if (out->size != sizeof(myo_ik_out)) return fail(MYO_E_BADARG, "myo_batch_ik: myo_ik_out.size is %zu, this library's struct has %zu bytes", out->size, sizeof(myo_ik_out));
  if (!out->qpos && !out->site_xpos && !out->residual && !out->cost && !out->kkt && !out->iters && !out->status) return MYO_OK;
  if (in->k < 0 || in->k > MYO_IK_K_MAX) return fail(MYO_E_ARG, "myo_batch_ik: k must be in [0, %d], got %d", MYO_IK_K_MAX, in->k);
  if (in->k > 0 && !in->site_ids) return fail(MYO_E_ARG, "myo_batch_ik: site_ids is NULL with k = %d", in->k);
  if (in->k > 0 && !in->targets) return fail(MYO_E_BADARG, "myo_batch_ik: targets is required");
  if (!(in->reg > 0) || !std::isfinite(in->reg)) return fail(MYO_E_ARG, "myo_batch_ik: reg must be finite and > 0");
  if (!(in->tol > 0)) return fail(MYO_E_ARG, "myo_batch_ik: tol must be > 0");
  if (in->max_iter < 1) return fail(MYO_E_ARG, "myo_batch_ik: max_iter must be >= 1");
  if (!b->ik_ws) {
    void* p = nullptr;
    const int e = be_malloc(&p, (size_t)b->n * MYO_IK_WS_N * sizeof(double));
    if (e || !p) return fail(MYO_E_DEVICE, "myo_batch_ik: workspace allocation failed: %s", be_errstr(e));
    b->ik_ws = (double*)p;
  }
  IkDev d{};
  d.site_ids = in->site_ids; d.targets = in->targets; d.weight = in->weight; d.q_init = in->q_init; d.q_ref = in->q_ref;
  d.lower = in->lower; d.upper = in->upper;
  d.qpos = out->qpos; d.site_xpos = out->site_xpos; d.residual = out->residual; d.cost = out->cost; d.kkt = out->kkt;
  d.iters = out->iters; d.status = out->status;
  d.ws = b->ik_ws; d.active = in->active; d.reg = in->reg; d.tol = in->tol;
  d.k = in->k; d.weight_per_env = in->weight && in->weight_per_env ? 1 : 0; d.max_iter = in->max_iter;
  return be_run(b, IkJob{d}, b->n, stream);
}
// myo_batch_simulate (csrc/myo_simulate.h): SimJob is a row of the variant table like PhysicsJob, keyed with the integrator, over
// k S blocks.  The shadow records (and, where the variant keeps its RK4 stage storage in global memory, one stage block per row: the
// batch's own is indexed by workgroup and sized for n envs) live in a workspace of the batch's own, grown on demand.  Every array
// lives on the device: the host refuses what it can see.
extern "C" int myo_batch_simulate(myo_batch* b, const myo_sim_in* in, const myo_sim_out* out, void* stream) {
  if (!b || !in || !out) return fail(MYO_E_BADARG, "myo_batch_simulate: null batch, input or output struct");
  if (in->size != sizeof(myo_sim_in)) return fail(MYO_E_BADARG, "myo_batch_simulate: myo_sim_in.size is %zu, this library's struct has %zu bytes", in->size, sizeof(myo_sim_in));
  if (out->size != sizeof(myo_sim_out)) return fail(MYO_E_BADARG, "myo_batch_simulate: myo_sim_out.size is %zu, this library's struct has %zu bytes", out->size, sizeof(myo_sim_out));
  if (in->k < 0 || in->S < 1 || in->T < 1) return fail(MYO_E_ARG, "myo_batch_simulate: k must be >= 0, S and T >= 1, got k = %d, S = %d, T = %d", in->k, in->S, in->T);
  if (!in->env_idx && in->k > b->n) return fail(MYO_E_ARG, "myo_batch_simulate: env_idx is NULL with k = %d beyond the batch's %d envs", in->k, b->n);
  if (in->nsub < 0) return fail(MYO_E_ARG, "myo_batch_simulate: nsub must be >= 0, got %d", in->nsub);
  if (in->every < 1 || in->T % in->every) return fail(MYO_E_ARG, "myo_batch_simulate: every must be >= 1 and divide T, got T = %d, every = %d", in->T, in->every);
  if (in->ns < 0 || in->ns > MYO_SIM_NS_MAX) return fail(MYO_E_ARG, "myo_batch_simulate: ns must be in [0, %d], got %d", MYO_SIM_NS_MAX, in->ns);
  if (out->site_xpos && in->ns > 0 && !in->site_ids) return fail(MYO_E_ARG, "myo_batch_simulate: site_ids is NULL with ns = %d", in->ns);
  if ((long long)in->k * in->S > (1ll << 31) - 1) return fail(MYO_E_ARG, "myo_batch_simulate: k * S = %lld exceeds 2^31 - 1", (long long)in->k * in->S);
  if (in->k == 0 || (!out->qpos && !out->qvel && !out->act && !out->time && !out->site_xpos && !out->bad && !out->steps)) return MYO_OK;
  const int rows = in->k * in->S;
  const int rkd = with_variant(b, [](auto v) {
    using V = decltype(v);
    return V::RK && !MYO_RK_IN_LDS(typename V::T, V::NC) ? (int)((sizeof(RkScratch<typename V::T>) + 7) / 8) : 0;
  });
  const int rk_off = rkd ? (b->L.stride + 1) / 2 * 2 : 0;      // (16-byte aligned behind the record)
  const int ws_stride = ((rkd ? rk_off + rkd : b->L.stride) + 1) / 2 * 2;
  const size_t need = (size_t)rows * ws_stride * sizeof(double);
  if (b->sim_ws_bytes < need) {
    if (be_capturing(stream)) return fail(MYO_E_STATE, "myo_batch_simulate: the workspace has to grow to %zu bytes while the stream is capturing; size it with an eager call of the same k * S first", need);
    if (b->sim_ws) { be_free(b->sim_ws); b->sim_ws = nullptr; b->sim_ws_bytes = 0; }
    void* p = nullptr;
    const int e = be_malloc(&p, need);
    if (e || !p) return fail(MYO_E_DEVICE, "myo_batch_simulate: workspace allocation of %zu bytes failed: %s", need, be_errstr(e));
    b->sim_ws = (double*)p; b->sim_ws_bytes = need;
  }
  SimDev d{};
  d.env_idx = in->env_idx; d.ctrl = in->ctrl; d.qpos0 = in->qpos0; d.qvel0 = in->qvel0; d.act0 = in->act0; d.site_ids = in->site_ids;
  d.qpos = out->qpos; d.qvel = out->qvel; d.act = out->act; d.time = out->time; d.site_xpos = in->ns > 0 ? out->site_xpos : nullptr;
  d.bad = out->bad; d.steps = out->steps; d.ws = b->sim_ws;
  d.S = in->S; d.T = in->T; d.nsub = in->nsub ? in->nsub : (b->K.frame_skip > 0 ? b->K.frame_skip : 1); d.every = in->every; d.ns = in->ns;
  d.ctrl_per_sample = in->ctrl && in->ctrl_per_sample ? 1 : 0; d.ws_stride = ws_stride; d.rk_off = rk_off;
  return be_run(b, SimJob{d}, rows, stream);
}
extern "C" int myo_batch_geom_poses(myo_batch* b, const int32_t* env_idx, int k, double* out, void* stream) {
  if (int rc = render_check_items(b, env_idx, k, "myo_batch_geom_poses")) return rc;
  if (!out) return fail(MYO_E_ARG, "myo_batch_geom_poses: null output");
  return be_run(b, geom_pass(b, env_idx, out), k, stream);
}
extern "C" int myo_batch_tendon_paths(myo_batch* b, const int32_t* env_idx, int k, double* out, void* stream) {
  int rc = items_check(b, env_idx, k, out, "myo_batch_tendon_paths");
  if (rc || k == 0 || b->ntitem == 0) return rc;
  return be_run(b, tendon_pass(b, env_idx, out), k, stream);
}
extern "C" int myo_batch_contact_items(myo_batch* b, const int32_t* env_idx, int k, double* out, void* stream) {
  int rc = items_check(b, env_idx, k, out, "myo_batch_contact_items");
  if (rc || k == 0) return rc;
  DeviceGuard guard(b->device);
  if ((rc = render_workspace(b, contact_tmp_doubles(b, k)))) return rc;
  return be_run(b, contact_pass(b, env_idx, k, b->render_ws, out), k, stream);
}
extern "C" int myo_batch_render(myo_batch* b, const int32_t* env_idx, int k, const myo_render_camera* cams, int ncams, int width, int height,
                                int flags, uint8_t* rgb, float* depth, int32_t* segid, void* stream) {
  int rc = render_check_items(b, env_idx, k, "myo_batch_render");
  if (rc) return rc;
  if (!cams || (ncams != 1 && ncams != k)) return fail(MYO_E_ARG, "myo_batch_render: ncams must be 1 or k (%d), got %d", k, ncams);
  if (width <= 0 || height <= 0 || (long long)width * height > MYO_RENDER_MAX_PIXELS)
    return fail(MYO_E_ARG, "myo_batch_render: width and height must be >= 1 with width * height <= %d", MYO_RENDER_MAX_PIXELS);
  if (flags & ~(MYO_RENDER_RGB | MYO_RENDER_DEPTH | MYO_RENDER_SEG | MYO_RENDER_SITES | MYO_RENDER_TENDONS | MYO_RENDER_CONTACTS)) return fail(MYO_E_ARG, "myo_batch_render: unknown flag bits 0x%x", flags);
  if (!(flags & (MYO_RENDER_RGB | MYO_RENDER_DEPTH | MYO_RENDER_SEG))) return fail(MYO_E_ARG, "myo_batch_render: no output requested");
  if ((flags & MYO_RENDER_TENDONS) && b->ntitem > MYO_RTEN_MAX)
    return fail(MYO_E_ARG, "myo_batch_render: MYO_RENDER_TENDONS: %d tendon items, at most %d can be drawn", b->ntitem, MYO_RTEN_MAX);
  if (((flags & MYO_RENDER_RGB) && !rgb) || ((flags & MYO_RENDER_DEPTH) && !depth) || ((flags & MYO_RENDER_SEG) && !segid))
    return fail(MYO_E_ARG, "myo_batch_render: a requested output buffer is NULL");
  if ((long long)k * width * height > (1ll << 31)) return fail(MYO_E_ARG, "myo_batch_render: k * width * height exceeds 2^31 pixels");
  std::vector<double> cam_tab;
  if ((rc = render_cameras(cams, ncams, height, cam_tab))) return rc;
  if (k > MYO_BACKEND_RENDER_ENVS_MAX) return fail(MYO_E_ARG, "myo_batch_render: at most %d envs per call", MYO_BACKEND_RENDER_ENVS_MAX);
  DeviceGuard guard(b->device);
  const RenderPlan p = render_plan(b, k, flags, cam_tab.size());
  if ((rc = render_workspace(b, p.total))) return rc;
  double* ws = b->render_ws;
  if ((rc = be_camera_upload(b, ws + p.cams, cam_tab, stream))) return rc;
  if ((rc = be_run(b, geom_pass(b, env_idx, ws), k, stream))) return rc;
  if (p.ntitem > 0 && (rc = be_run(b, tendon_pass(b, env_idx, ws + p.tendons), k, stream))) return rc;
  if (p.ncitem > 0 && (rc = be_run(b, contact_pass(b, env_idx, k, ws + p.tmp, ws + p.contacts), k, stream))) return rc;
  return be_cast(b, p, k, ncams, width, height, flags, rgb, depth, segid, stream);
}
extern "C" double myo_batch_kernel_ms(myo_batch* b) { return b ? be_kernel_ms(b) : -1.0; }
