// myo_render.h — rendering of env states (include/myobatch.h: myo_batch_geom_poses / _tendon_paths / _contact_items, myo_batch_render).
//   item passes  one wave per listed env writes one table of MYO_RENDER_ITEM_N-double rows.  A pass is a small struct (GeomPass,
//                TendonPass, ContactPass: the env list, the output, its host-built tables and its rows per env) with a job_run that calls
//                the pass's env_* function: a job like every env-path entry point's (csrc/myo_task.h), run by k_env / be_run.
//     env_geom_poses     load_env + the stepper's own kinematics, then one lane per item (geoms, then sites) writes its world pose, the
//                        env's geometry (geom_size0_hp / geom_lpos_hp ...), its type and colour.  Reads the record only.
//     env_tendon_paths   load_env + kinematics, then one lane per tendon path element (the host-resolved te_i walk) runs the stepper's
//                        wrap_geom and writes the element's straight pieces as capsule items.
//     env_contact_items  env_sense (csrc/myo_sense.h) into a compact temporary of the render workspace, then one lane per contact slot
//                        writes the slot's point (a disc) and force (a capsule shaft) items.
//   ray casts    one workgroup of 256 threads per (env, 16x16 tile).  A table's items are staged in LDS in fp32 relative to the camera, a
//                per-tile cull on each item's bounding sphere marks the items the tile can see (the flag is the same for every thread
//                of the tile: the loop over items stays uniform), then one thread per pixel intersects its ray with them.
//     k_render          one table (geoms + sites); the pixel is finished from LDS (render_pixel).
//     k_render_layers   RLayers: two or three tables — geoms, tendon items if drawn, contact items if drawn — take turns in the same LDS
//                       table and are traced into the same per-pixel hit; the hit items are then shaded from their global rows
//                       (render_layers_finish).  The LDS allocation is the largest table's, not the sum.
// Which passes and which cast a myo_batch_render call runs, and where their tables lie in the workspace: render_plan (csrc/myo_host.h).
// The per-thread functions take the thread index, so the emulation build (csrc/emu_host.h) runs the same code thread by thread.
#pragma once

#define MYO_RTILE 16                 // tile edge (pixels); 256 threads per tile
#define MYO_RITEM_MAX 512            // items (ngeom + nsite) the LDS table holds
#define MYO_RTEN_MAX MYO_RITEM_MAX    // tendon items the second LDS pass holds
#define MYO_RCAM_N 16                // doubles per camera of the device camera table: pos[3] fwd[3] right[3] up[3] focal (pixels) pad[3]

// ---------------------------------------------------------------------------------------------------------------- pose pass
// vis: per item 8 floats (host-built, csrc/myo_host.h render_vis_table): rgba[4], site radius, optional (1: a site drawn only with
// MYO_RENDER_SITES), 0, 0
template <typename T, int NC>
DEV void env_geom_poses(const DevModel<T>& M_in, const TaskDev& K_in, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s_in, int env,
                        const float* vis, double* out) {
  MYO_BIND_M(T) MYO_BIND_K MYO_BIND_S(T)
  WAVE_FN_K
  load_env(M, K, L, rec, s, env);
  kinematics(M, s);
  const int goal_b = (K.kind == MYO_TASK_REORIENT_K && K.target1_sid >= 0) ? M.site_bodyid[K.target1_sid] : -1;
  const int baoding = (K.kind == 1 || K.kind == 2) && K.target1_sid >= 0 && K.target2_sid >= 0;
  PHASE {
    for (int i = lane; i < M.ngeom + M.nsite; i += 64) {
      double* o = out + (size_t)i * MYO_RENDER_ITEM_N;
      const int is_site = i >= M.ngeom, id = is_site ? i - M.ngeom : i;
      const int b = is_site ? M.site_bodyid[id] : M.geom_bodyid[id];
      HP B[9], xp[3], l[3], p[3], R[9], sz[3];
      if (b == goal_b) {      // the die's target body: at the episode's goal pose (reorient.py sets body_pos / body_quat of `target`)
        const HP* q = s.goal_quat;
        const HP n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const HP qn[4] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n};
        quat2mat(B, qn);
        for (int k = 0; k < 3; ++k) xp[k] = s.goal_pos[k];
      } else {
        quat2mat(B, S_XQUAT(s) + 4 * b);
        for (int k = 0; k < 3; ++k) xp[k] = S_XPOS(s)[3 * b + k];
      }
      const float* v = vis + 8 * (size_t)i;
      int type;
      if (is_site) {
        for (int k = 0; k < 3; ++k) l[k] = M.h_site_pos[3 * id + k];
        if (baoding && id == K.target1_sid) { l[0] = s.target_xy[0]; l[1] = s.target_xy[1]; }      // (as baoding_obs_reward places them)
        if (baoding && id == K.target2_sid) { l[0] = s.target_xy[2]; l[1] = s.target_xy[3]; }
        for (int k = 0; k < 9; ++k) R[k] = B[k];
        sz[0] = sz[1] = sz[2] = (HP)v[4];
        type = MYO_GEOM_SPHERE;
      } else {
        geom_lpos_hp(M, K, s, id, l);
        mulmat3(R, B, M.h_geom_mat + 9 * id);
        sz[0] = geom_size0_hp(M, K, s, id); sz[1] = geom_size1_hp(M, K, s, id); sz[2] = geom_size2_hp(M, K, s, id);
        type = M.geom_type[id];
      }
      mulmatvec3(p, B, l);
      for (int k = 0; k < 3; ++k) o[k] = p[k] + xp[k];
      for (int k = 0; k < 9; ++k) o[3 + k] = R[k];
      for (int k = 0; k < 3; ++k) o[12 + k] = sz[k];
      o[15] = type;
      for (int k = 0; k < 4; ++k) o[16 + k] = v[k];
      HP rb;
      switch (type) {
        case MYO_GEOM_SPHERE: rb = sz[0]; break;
        case MYO_GEOM_CAPSULE: rb = sz[0] + sz[1]; break;
        case MYO_GEOM_CYLINDER: rb = sqrt(sz[0] * sz[0] + sz[1] * sz[1]); break;
        case MYO_GEOM_ELLIPSOID: rb = sz[0] > sz[1] ? (sz[0] > sz[2] ? sz[0] : sz[2]) : (sz[1] > sz[2] ? sz[1] : sz[2]); break;
        case MYO_GEOM_BOX: rb = sqrt(sz[0] * sz[0] + sz[1] * sz[1] + sz[2] * sz[2]); break;
        case MYO_GEOM_PLANE: rb = (sz[0] > 0 && sz[1] > 0) ? sqrt(sz[0] * sz[0] + sz[1] * sz[1]) : (HP)-1; break;     // -1: unbounded
        default: rb = 0;
      }
      o[20] = rb; o[21] = v[5]; o[22] = 0; o[23] = 0;
    }
  }
  SYNC();
  ws_release(K, s);
}

// ---------------------------------------------------------------------------------------------------------------- path pass
#define MYO_RTEN_ACT_R 1.00      // the "active" colour a muscle's tendon is blended toward by its activation (include/myobatch.h)
#define MYO_RTEN_ACT_G 0.90
#define MYO_RTEN_ACT_B 0.10
// one straight piece a -> b as a capsule item: midpoint, z axis along the piece, size [radius, half length, 0]; [22] = tendon + 1,
// [23] = the piece's contribution to the tendon's length
DEV void tendon_item(double* o, const HP* a, const HP* b, HP radius, const HP* rgba, int t, HP contrib) {
  HP z[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const HP n = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  if (n > 0) { z[0] /= n; z[1] /= n; z[2] /= n; } else { z[0] = 0; z[1] = 0; z[2] = 1; }
  // x: the coordinate axis z is least aligned with, made orthogonal to z; y = z x x
  const HP az[3] = {fabs(z[0]), fabs(z[1]), fabs(z[2])};
  const int im = az[0] <= az[1] ? (az[0] <= az[2] ? 0 : 2) : (az[1] <= az[2] ? 1 : 2);
  const HP ax[3] = {im == 0 ? (HP)1 : (HP)0, im == 1 ? (HP)1 : (HP)0, im == 2 ? (HP)1 : (HP)0};
  HP x[3], y[3];
  cross3(x, ax, z);
  normalize3(x);
  cross3(y, z, x);
  for (int k = 0; k < 3; ++k) {
    o[k] = (HP)0.5 * (a[k] + b[k]);
    o[3 + 3 * k] = x[k]; o[4 + 3 * k] = y[k]; o[5 + 3 * k] = z[k];
  }
  o[12] = radius; o[13] = (HP)0.5 * n; o[14] = 0;
  o[15] = MYO_GEOM_CAPSULE;
  for (int k = 0; k < 4; ++k) o[16 + k] = rgba[k];
  o[20] = radius + (HP)0.5 * n; o[21] = 0; o[22] = t + 1; o[23] = contrib;
}
// tvis: per tendon 8 floats (host-built, csrc/myo_host.h render_tendon_table): base rgba[4], radius, index of the activation that
// colours it (-1: none), 0, 0.  tadr[e]: first item slot of path element e (1 slot for site -> site, 3 around a wrap geom).
template <typename T, int NC>
DEV void env_tendon_paths(const DevModel<T>& M_in, const TaskDev& K_in, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s_in, int env,
                          const float* tvis, const int* tadr, double* out) {
  MYO_BIND_M(T) MYO_BIND_K MYO_BIND_S(T)
  WAVE_FN_K
  load_env(M, K, L, rec, s, env);
  kinematics(M, s);
  PHASE {
    for (int e = lane; e < M.nte; e += 64) {
      const int i0 = M.te_i[4 * e], iend = M.te_i[4 * e + 1], ig = M.te_i[4 * e + 2], t = M.te_i[4 * e + 3];
      const HP div = (HP)M.te_div[e];
      double* o = out + (size_t)tadr[e] * MYO_RENDER_ITEM_N;
      const float* v = tvis + 8 * (size_t)t;
      HP rgba[4] = {(HP)v[0], (HP)v[1], (HP)v[2], (HP)v[3]};
      const int ia = (int)v[5];
      if (ia >= 0 && ia < M.na) {      // rgb = (1 - a) base + a active, a = the muscle's activation clamped to [0, 1]
        HP a = S_ACT(M, s)[ia];
        a = a < 0 ? (HP)0 : (a > 1 ? (HP)1 : a);
        const HP act[3] = {(HP)MYO_RTEN_ACT_R, (HP)MYO_RTEN_ACT_G, (HP)MYO_RTEN_ACT_B};
        for (int k = 0; k < 3; ++k) rgba[k] = ((HP)1 - a) * rgba[k] + a * act[k];
      }
      const HP radius = (HP)v[4];
      HP q0[3], q1[3];
      body_point_hp(s, M.wr_i[8 * i0 + 1], M.h_wr_p + 4 * i0, q0);
      body_point_hp(s, M.wr_i[8 * iend + 1], M.h_wr_p + 4 * iend, q1);
      HP wlen = -1, pts[6] = {0, 0, 0, 0, 0, 0};
      if (ig >= 0) {       // the stepper's wrap solver on the same operands as its tendon_wrap_pass (absolute positions here)
        const int body = M.wr_i[8 * ig + 1], side_body = M.wr_i[8 * ig + 3];
        HP gmat[9], bm[9], side[3] = {0, 0, 0}, gp[3];
        quat2mat(bm, S_XQUAT(s) + 4 * body);
        mulmat3(gmat, bm, M.h_wr_m + 12 * ig);
        if (side_body >= 0) body_point_hp(s, side_body, M.h_wr_m + 12 * ig + 9, side);
        body_point_hp(s, body, M.h_wr_p + 4 * ig, gp);
        wlen = wrap_geom(pts, q0, q1, gp, gmat, geom_size0_hp(M, K, s, M.wr_i[8 * ig + 2]), M.wr_i[8 * ig], side, side_body >= 0);
      }
      if (wlen >= 0) {
        HP d0[3], d1[3];
        for (int k = 0; k < 3; ++k) { d0[k] = pts[k] - q0[k]; d1[k] = q1[k] - pts[3 + k]; }
        tendon_item(o, q0, pts, radius, rgba, t, norm3(d0) / div);
        tendon_item(o + MYO_RENDER_ITEM_N, pts, pts + 3, radius, rgba, t, wlen / div);       // the chord stands for the arc
        tendon_item(o + 2 * MYO_RENDER_ITEM_N, pts + 3, q1, radius, rgba, t, norm3(d1) / div);
      } else {
        HP d0[3];
        for (int k = 0; k < 3; ++k) d0[k] = q1[k] - q0[k];
        tendon_item(o, q0, q1, radius, rgba, t, norm3(d0) / div);
        if (ig >= 0) for (int k = 0; k < 2 * MYO_RENDER_ITEM_N; ++k) o[MYO_RENDER_ITEM_N + k] = 0;      // the wrap's two unused slots
      }
    }
  }
  SYNC();
  ws_release(K, s);
}

// ---------------------------------------------------------------------------------------------------------------- contact item pass
// the two items of contact slot c from its con_d row (dist, pos[3], normal[3], force[6]): o[0 .. 24) the point, o[24 .. 48) the force
DEV void contact_slot_items(double* o, const double* cd, int c, const myo_render_style& st) {
  const HP pos[3] = {cd[1], cd[2], cd[3]}, nrm[3] = {cd[4], cd[5], cd[6]};
  // the contact frame as the stepper builds it: make_frame on a copy of the normal, the record's six numbers, the second tangent
  struct { HP nrm[3], tinv; } cf;
  HP fr[6] = {nrm[0], nrm[1], nrm[2], 0, 0, 0}, t2[3];
  cf.tinv = make_frame(fr);
  for (int k = 0; k < 3; ++k) cf.nrm[k] = fr[k];
  con_frame(cf, fr);
  con_t2(fr, t2);
  const HP r = (HP)st.disc_radius, h = (HP)st.disc_half_height;
  for (int k = 0; k < 3; ++k) {
    o[k] = pos[k];
    o[3 + 3 * k] = fr[3 + k]; o[4 + 3 * k] = t2[k]; o[5 + 3 * k] = nrm[k];
  }
  o[12] = r; o[13] = h; o[14] = 0;
  o[15] = MYO_GEOM_CYLINDER;
  for (int k = 0; k < 4; ++k) o[16 + k] = (HP)st.point_rgba[k];
  o[20] = sqrt(r * r + h * h); o[21] = 0; o[22] = c + 1; o[23] = cd[0];
  // the world force on geom2's body and its shaft from the contact point
  HP F[3], tip[3];
  for (int k = 0; k < 3; ++k) F[k] = nrm[k] * cd[7] + fr[3 + k] * cd[8] + t2[k] * cd[9];
  const HP fn = norm3(F);
  double* o2 = o + MYO_RENDER_ITEM_N;
  if (fn > 0) {
    const HP rgba[4] = {(HP)st.force_rgba[0], (HP)st.force_rgba[1], (HP)st.force_rgba[2], (HP)st.force_rgba[3]};
    for (int k = 0; k < 3; ++k) tip[k] = pos[k] + (HP)st.metres_per_newton * F[k];
    tendon_item(o2, pos, tip, (HP)st.force_radius, rgba, c, fn);
  } else {
    for (int k = 0; k < MYO_RENDER_ITEM_N; ++k) o2[k] = 0;
  }
}
// row `row` of the call (env `env` of the batch): tmp = the call's compact temporaries ncon [k], con_d [k, cap, 13].  env_sense indexes
// its outputs by batch env, so it is handed pointers offset by (row - env) strides: its stores land in row `row`.
template <typename T, int NC>
DEV void env_contact_items(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s, int env, int row,
                           const SenseDev& tmp, const myo_render_style& st, double* out) {
  WAVE_FN_K
  const int cap = tmp.cap;
  const long long shift = (long long)row - (long long)env;
  SenseDev O;
  O.con_geom = nullptr; O.body_wrench = nullptr; O.qfrc_constraint = nullptr;
  O.act_length = nullptr; O.act_velocity = nullptr; O.act_force = nullptr; O.activation = nullptr; O.ten_length = nullptr; O.ten_velocity = nullptr;
  O.cap = cap;
  O.ncon = tmp.ncon + shift;
  O.con_d = tmp.con_d + shift * (long long)(cap * MYO_SENSE_CON_N);
  env_sense(M, K, L, rec, s, env, O);
  SYNC_G();      // (the rows below are read by other lanes than the ones that stored them)
  const double* cd = tmp.con_d + (size_t)row * cap * MYO_SENSE_CON_N;
  PHASE {
    const int ncon = tmp.ncon[row];
    for (int c = lane; c < cap; c += 64) {
      double* o = out + (size_t)c * 2 * MYO_RENDER_ITEM_N;
      if (c < ncon) contact_slot_items(o, cd + (size_t)c * MYO_SENSE_CON_N, c, st);
      else for (int k = 0; k < 2 * MYO_RENDER_ITEM_N; ++k) o[k] = 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the three passes
// Jobs (csrc/myo_task.h) over a LIST of envs: block r writes the `rows` items of env idx[r] to row r of `out` [k, rows, MYO_RENDER_ITEM_N];
// a listed index outside [0, n_envs) gets an all-zero row (nothing drawn).  Keyed without the integrator: no pass integrates (load_env,
// kinematics and the env_* passes never read s.rk).
struct GeomPass { static constexpr bool RK = false; const int* idx; double* out; int rows; const float* vis; };                      // rows = ngeom + nsite
struct TendonPass { static constexpr bool RK = false; const int* idx; double* out; int rows; const float *tvis; const int* tadr; };  // rows = the model's tendon items
struct ContactPass { static constexpr bool RK = false; const int* idx; double* out; int rows; SenseDev tmp; myo_render_style style; };   // rows = 2 * tmp.cap
// row `block` of a pass's table and its env; null, with the row zeroed, for an index outside the batch
template <typename Pass>
DEV double* pass_row(const Pass& P, int block, int n_envs, int& env) {
  WAVE_FN
  const int n = P.rows * MYO_RENDER_ITEM_N;
  double* o = P.out + (size_t)block * n;
  env = P.idx[block];
  if (env >= 0 && env < n_envs) return o;
  PHASE { for (int i = lane; i < n; i += 64) o[i] = 0.0; }
  return nullptr;
}
MYO_JOB_RUN(GeomPass) { int env; if (double* o = pass_row(J, block, n_envs, env)) env_geom_poses(M, K, L, MYO_ENV_REC(env), s, env, J.vis, o); }
MYO_JOB_RUN(TendonPass) { int env; if (double* o = pass_row(J, block, n_envs, env)) env_tendon_paths(M, K, L, MYO_ENV_REC(env), s, env, J.tvis, J.tadr, o); }
MYO_JOB_RUN(ContactPass) { int env; if (double* o = pass_row(J, block, n_envs, env)) env_contact_items(M, K, L, MYO_ENV_REC(env), s, env, block, J.tmp, J.style, o); }

// ---------------------------------------------------------------------------------------------------------------- ray cast
struct RItem {      // one item in LDS: fp32, relative to the camera position
  float c[3], R[9], sz[3], rgba[4], rb;
  int type, draw;    // draw: drawn in this tile (cull result)
};

// stage items i = tid, tid + 256, ... of one env (pose pass output `it`) relative to the camera
DEV void render_load(RItem& r, const double* o, const double* cam, int flags) {
  for (int k = 0; k < 3; ++k) r.c[k] = (float)(o[k] - cam[k]);
  for (int k = 0; k < 9; ++k) r.R[k] = (float)o[3 + k];
  for (int k = 0; k < 3; ++k) r.sz[k] = (float)o[12 + k];
  for (int k = 0; k < 4; ++k) r.rgba[k] = (float)o[16 + k];
  r.rb = (float)o[20];
  r.type = (int)o[15];
  r.draw = r.rgba[3] > 0.f && (o[21] == 0.0 || (flags & MYO_RENDER_SITES));
}
// (ngeom, geom_alpha: the layered cast's translucent geoms — the alpha of items < ngeom is scaled; the sites keep theirs)
DEV void render_stage(int tid, RItem* lds, const double* it, int nitem, const double* cam, int flags, int ngeom = 0, float geom_alpha = 1.f) {
  for (int i = tid; i < nitem; i += MYO_RTILE * MYO_RTILE) {
    RItem& r = lds[i];
    render_load(r, it + (size_t)i * MYO_RENDER_ITEM_N, cam, flags);
    if (i < ngeom) { r.rgba[3] *= geom_alpha; if (!(r.rgba[3] > 0.f)) r.draw = 0; }
  }
}

// per-tile cull: the item's bounding sphere against the tile's four side planes through the camera and the camera plane
DEV void render_cull(int tid, RItem* lds, int nitem, const double* cam, int W, int H, int tx0, int ty0) {
  const float f = (float)cam[12];
  const float fw[3] = {(float)cam[3], (float)cam[4], (float)cam[5]}, rt[3] = {(float)cam[6], (float)cam[7], (float)cam[8]},
              up[3] = {(float)cam[9], (float)cam[10], (float)cam[11]};
  const float xa = ((float)tx0 - 0.5f * (float)W) / f, xb = ((float)(tx0 + MYO_RTILE) - 0.5f * (float)W) / f;
  const float yb = (0.5f * (float)H - (float)(ty0 + MYO_RTILE)) / f, ya = (0.5f * (float)H - (float)ty0) / f;
  for (int i = tid; i < nitem; i += MYO_RTILE * MYO_RTILE) {
    RItem& r = lds[i];
    if (!r.draw || r.rb < 0.f) continue;     // hidden, or an unbounded plane (always tested)
    const float cz = r.c[0] * fw[0] + r.c[1] * fw[1] + r.c[2] * fw[2], cx = r.c[0] * rt[0] + r.c[1] * rt[1] + r.c[2] * rt[2],
                cy = r.c[0] * up[0] + r.c[1] * up[1] + r.c[2] * up[2];
    const float rb = r.rb * 1.0001f + 1e-6f;       // (margin for the fp32 rounding of the tests below)
    const bool in = cz > -rb && (cx - xa * cz) >= -rb * sqrtf(1.f + xa * xa) && (xb * cz - cx) >= -rb * sqrtf(1.f + xb * xb) &&
                    (cy - yb * cz) >= -rb * sqrtf(1.f + yb * yb) && (ya * cz - cy) >= -rb * sqrtf(1.f + ya * ya);
    r.draw = in ? 1 : 0;
  }
}

// smallest t > 0 where the ray o + t d meets |x|^2 = r2 in the first `dim` coordinates (a sphere, dim 3; an infinite cylinder, dim 2);
// INF if none.  Solved about the point of the ray closest to the centre, which keeps fp32's cancellation of |o|^2 - r^2 out of it.
DEV float rsolve(const float* o, const float* d, int dim, float r2) {
  float a = 0.f, b = 0.f;
  for (int k = 0; k < dim; ++k) { a += d[k] * d[k]; b += o[k] * d[k]; }
  if (a <= 0.f) return INFINITY;
  const float tc = -b / a;
  float c = -r2;
  for (int k = 0; k < dim; ++k) { const float p = o[k] + tc * d[k]; c += p * p; }
  if (c > 0.f) return INFINITY;
  const float w = sqrtf(-c / a), t0 = tc - w, t1 = tc + w;
  return t0 > 0.f ? t0 : (t1 > 0.f ? t1 : INFINITY);
}

// intersection of the ray o + t d (item-local frame) with the item; returns t (INF: miss) and the local normal
DEV float render_hit(int type, const float* sz, const float* o, const float* d, float* n) {
  float t = INFINITY;
  n[0] = 0.f; n[1] = 0.f; n[2] = 1.f;
  switch (type) {
    case MYO_GEOM_SPHERE: {
      t = rsolve(o, d, 3, sz[0] * sz[0]);
      for (int k = 0; k < 3; ++k) n[k] = o[k] + t * d[k];
      break;
    }
    case MYO_GEOM_ELLIPSOID: {
      const float os[3] = {o[0] / sz[0], o[1] / sz[1], o[2] / sz[2]}, ds[3] = {d[0] / sz[0], d[1] / sz[1], d[2] / sz[2]};
      t = rsolve(os, ds, 3, 1.f);
      for (int k = 0; k < 3; ++k) n[k] = (o[k] + t * d[k]) / (sz[k] * sz[k]);
      break;
    }
    case MYO_GEOM_CAPSULE:
    case MYO_GEOM_CYLINDER: {
      const float r = sz[0], h = sz[1];
      const float tc = rsolve(o, d, 2, r * r);
      if (tc < INFINITY && fabsf(o[2] + tc * d[2]) <= h) { t = tc; n[0] = o[0] + tc * d[0]; n[1] = o[1] + tc * d[1]; n[2] = 0.f; }
      for (int e = -1; e <= 1; e += 2) {
        const float zc = (float)e * h;
        if (type == MYO_GEOM_CAPSULE) {      // the two end spheres
          const float oz = o[2] - zc, oc[3] = {o[0], o[1], oz};
          const float ts = rsolve(oc, d, 3, r * r);
          if (ts < t) { t = ts; n[0] = o[0] + ts * d[0]; n[1] = o[1] + ts * d[1]; n[2] = oz + ts * d[2]; }
        } else if (d[2] != 0.f) {            // the two caps
          const float tp = (zc - o[2]) / d[2];
          const float x = o[0] + tp * d[0], y = o[1] + tp * d[1];
          if (tp > 0.f && tp < t && x * x + y * y <= r * r) { t = tp; n[0] = 0.f; n[1] = 0.f; n[2] = (float)e; }
        }
      }
      break;
    }
    case MYO_GEOM_BOX: {
      float tn = -INFINITY, tf = INFINITY;
      int ax = 0;
      float sg = 1.f;
      for (int k = 0; k < 3; ++k) {
        if (d[k] == 0.f) {
          if (fabsf(o[k]) > sz[k]) return INFINITY;
          continue;
        }
        const float ta = (-sz[k] - o[k]) / d[k], tb = (sz[k] - o[k]) / d[k];
        const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
        if (lo > tn) { tn = lo; ax = k; sg = d[k] > 0.f ? -1.f : 1.f; }
        tf = fminf(tf, hi);
      }
      if (tn > tf || tf <= 0.f) return INFINITY;
      t = tn > 0.f ? tn : tf;
      n[0] = ax == 0 ? sg : 0.f; n[1] = ax == 1 ? sg : 0.f; n[2] = ax == 2 ? sg : 0.f;
      break;
    }
    case MYO_GEOM_PLANE: {
      if (d[2] == 0.f) return INFINITY;
      const float tp = -o[2] / d[2];
      const float x = o[0] + tp * d[0], y = o[1] + tp * d[1];
      if (tp > 0.f && (sz[0] <= 0.f || sz[1] <= 0.f || (fabsf(x) <= sz[0] && fabsf(y) <= sz[1]))) t = tp;
      break;
    }
    default: break;
  }
  return t;
}

#define MYO_RBG_R 0.12f      // background colour
#define MYO_RBG_G 0.14f
#define MYO_RBG_B 0.18f

DEV float render_shade(const RItem& r, const float* nl, const float* d, float* rgb) {
  float n[3];
  for (int k = 0; k < 3; ++k) n[k] = r.R[3 * k] * nl[0] + r.R[3 * k + 1] * nl[1] + r.R[3 * k + 2] * nl[2];      // world = R nl
  const float nn = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), dd = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const float cs = nn > 0.f ? fabsf(n[0] * d[0] + n[1] * d[1] + n[2] * d[2]) / (nn * dd) : 1.f;
  const float lam = 0.3f + 0.7f * fminf(cs, 1.f);
  for (int k = 0; k < 3; ++k) rgb[k] = r.rgba[k] * lam;
  return r.rgba[3];
}

// the nearest opaque and the nearest translucent hit of one pixel's ray; item indices count from `base` of the table traced
struct RHit { float to, tt, no[3], nt[3]; int io, it; };
DEV void render_ray(const double* cam, int W, int H, int px, int py, float* d, RHit& h) {
  const float f = (float)cam[12];
  const float tx = ((float)px + 0.5f - 0.5f * (float)W) / f, ty = (0.5f * (float)H - ((float)py + 0.5f)) / f;
  for (int k = 0; k < 3; ++k) d[k] = (float)cam[3 + k] + tx * (float)cam[6 + k] + ty * (float)cam[9 + k];     // forward component 1: t = depth
  h.to = INFINITY; h.tt = INFINITY; h.io = -1; h.it = -1;
  h.no[0] = 0.f; h.no[1] = 0.f; h.no[2] = 1.f; h.nt[0] = 0.f; h.nt[1] = 0.f; h.nt[2] = 1.f;
}
DEV void render_trace(const RItem* lds, int nitem, int base, const float* d, RHit& h) {
  for (int i = 0; i < nitem; ++i) {
    const RItem& r = lds[i];
    if (!r.draw) continue;
    float ol[3], dl[3], nl[3];
    for (int k = 0; k < 3; ++k) {       // local = R^T (x - c)
      ol[k] = -(r.R[k] * r.c[0] + r.R[3 + k] * r.c[1] + r.R[6 + k] * r.c[2]);
      dl[k] = r.R[k] * d[0] + r.R[3 + k] * d[1] + r.R[6 + k] * d[2];
    }
    const float t = render_hit(r.type, r.sz, ol, dl, nl);
    if (r.rgba[3] >= 1.f) {
      if (t < h.to) { h.to = t; h.io = base + i; h.no[0] = nl[0]; h.no[1] = nl[1]; h.no[2] = nl[2]; }
    } else if (t < h.tt) { h.tt = t; h.it = base + i; h.nt[0] = nl[0]; h.nt[1] = nl[1]; h.nt[2] = nl[2]; }
  }
}
// the pixel's outputs from its hits: ro / rt the opaque / translucent item hit (read only where h.io / h.it >= 0), so / st their ids
DEV void render_write(const RItem* ro, const RItem* rt, int so, int st, const RHit& h, const float* d, int flags, size_t pix,
                      unsigned char* rgb, float* depth, int* seg) {
  const bool front_t = h.it >= 0 && h.tt < h.to;
  if (flags & MYO_RENDER_RGB) {
    float c[3] = {MYO_RBG_R, MYO_RBG_G, MYO_RBG_B};
    if (h.io >= 0) render_shade(*ro, h.no, d, c);
    if (front_t) {
      float ct[3];
      const float a = render_shade(*rt, h.nt, d, ct);
      for (int k = 0; k < 3; ++k) c[k] = a * ct[k] + (1.f - a) * c[k];
    }
    for (int k = 0; k < 3; ++k) rgb[3 * pix + k] = (unsigned char)fminf(255.f, fmaxf(0.f, floorf(c[k] * 255.f + 0.5f)));
  }
  if (flags & MYO_RENDER_DEPTH) depth[pix] = front_t ? h.tt : h.to;
  if (flags & MYO_RENDER_SEG) seg[pix] = front_t ? st : so;
}

// one pixel (row py from the top, column px) of env row `e` of the output
DEV void render_pixel(const RItem* lds, int nitem, const double* cam, int W, int H, int px, int py, int flags, size_t e,
                      unsigned char* rgb, float* depth, int* seg) {
  if (px >= W || py >= H) return;
  float d[3];
  RHit h;
  render_ray(cam, W, H, px, py, d, h);
  render_trace(lds, nitem, 0, d, h);
  const size_t pix = (e * (size_t)H + (size_t)py) * (size_t)W + (size_t)px;
  render_write(lds + (h.io >= 0 ? h.io : 0), lds + (h.it >= 0 ? h.it : 0), h.io, h.it, h, d, flags, pix, rgb, depth, seg);
}
// The layered cast (k_render_layers): l[0] is the geoms' table, staged with geom_alpha on the alpha of the geoms (1: opaque as they
// are); then the tendon items if drawn, then the contact items if drawn.  rows: the call's [k, n, MYO_RENDER_ITEM_N] table.  Hit indices
// run on through the layers in order; the id of an item of layer 0 is its index, of a later layer id_base + its [22] - 1 (id_base:
// ngeom + nsite for tendons, ngeom + nsite + ntendon for contact slots).
struct RLayer { const double* rows; int n, id_base; };
struct RLayers { RLayer l[3]; int nl, ngeom; float geom_alpha; };
// after every layer was traced into h the hit items come from their global rows (the LDS table holds the last layer by now)
DEV int render_layer_item(RItem& r, const RLayers& Y, size_t e, int idx, const double* cam, int flags) {
  int j = 0, base = 0;
  while (j + 1 < Y.nl && idx >= base + Y.l[j].n) base += Y.l[j++].n;
  const double* o = Y.l[j].rows + (e * (size_t)Y.l[j].n + (size_t)(idx - base)) * MYO_RENDER_ITEM_N;
  render_load(r, o, cam, flags);
  if (idx < Y.ngeom) r.rgba[3] *= Y.geom_alpha;
  return j == 0 ? idx : Y.l[j].id_base + (int)o[22] - 1;
}
DEV void render_layers_finish(const RLayers& Y, const double* cam, int W, int H, int px, int py, int flags, size_t e, const RHit& h, const float* d,
                              unsigned char* rgb, float* depth, int* seg) {
  if (px >= W || py >= H) return;
  RItem ro, rt;
  int so = h.io, st = h.it;
  if (h.io >= 0) so = render_layer_item(ro, Y, e, h.io, cam, flags);
  if (h.it >= 0) st = render_layer_item(rt, Y, e, h.it, cam, flags);
  const size_t pix = (e * (size_t)H + (size_t)py) * (size_t)W + (size_t)px;
  render_write(&ro, &rt, so, st, h, d, flags, pix, rgb, depth, seg);
}
