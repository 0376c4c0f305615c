// myo_simulate.h — read-only open-loop simulation (include/myobatch.h: myo_batch_simulate).
//
// What happens from this state under these controls?  S control sequences per listed env, T control steps of nsub substeps each, in
// one launch of k S workgroups: block r = e S + j is sample j of env env_idx[e] (envs may repeat).  A job of the env path's wrapper
// kernel beside env_ik / env_static_opt, keyed WITH the integrator (Euler and RK4 batches both work).  It reads the env record and
// writes NOTHING back to it: the envs do not move.
//
// The shadow record.  The block copies the env's whole record (L.stride doubles, lanes over the run) into row r of a library-grown
// global workspace (myo_batch::sim_ws), with qpos / qvel / act replaced by the caller's start state where one is given, and calls
// load_env on THAT row; everything after reads and writes the shadow only.  This is not a convenience: load_env points warm_g at the
// record's warm start, and the 48-slot variant (Scratch::SPILL: the die) uses act and the object group's friction IN PLACE in the
// record (S_ACT / act_set / S_OBJF) — a rollout on the env's own record would move the env, and the samples of one env would race.
// The shadow carries the env's warm start, time, per-episode ball / object parameters and task block, so P2-randomised and die envs
// simulate with their own masses, frictions and sizes.  Where the RK4 stage storage lives in global memory it is indexed by
// workgroup and sized for the batch's own launches (TaskDev::rk_ws); a launch of k S workgroups has its stage blocks behind the
// shadow rows instead (SimDev::rk_off).
//
// The step loop: ctrl_set from the caller's controls, nsub x mj_step (the stepper's own function: k_step's instantiations do not
// change), and on every `every`-th step the new qpos / qvel / act / time go to row t / every - 1 of the outputs; with site outputs
// one extra position pass (kinematics) at the new state first, and the listed sites' world positions as env_data computes
// site_xpos (the task-owned target sites with the env's own geometry).  No action map, no fatigue advance, no task layer: the
// controls are muscle controls, exactly as myo_batch_physics_step takes them.  A sample whose state blows up (s.bad: mj_checkPos /
// mj_checkVel / mj_checkAcc, and the same test of the state a step leaves) stops stepping: bad[r] = 1, steps[r] = the steps it
// completed, its remaining output rows NaN.  No reset: this is physics level, like env_physics.
//
// All stores are plain vector stores, lanes over elements; no atomics; each sample's arithmetic is its own: the same bits on every
// run, whatever S and whoever the neighbours are, and the lane-serial emulation runs the same source.
#pragma once

/* MYO_SIM_NS_MAX, site outputs per call, is include/myobatch.h's */
struct SimDev {
  const int* env_idx;                          // [k] (null: env e is e)
  const double* ctrl;                          // [k, S, T, nu] (ctrl_per_sample) or [k, T, nu]; null: 0
  const double *qpos0, *qvel0, *act0;          // [k, S, nq / nv / na] or null: the env's own
  const int* site_ids;                         // [ns]
  double *qpos, *qvel, *act, *time, *site_xpos;      // [k, S, R, .] with R = T / every; any may be null
  int *bad, *steps;                            // [k, S]
  double* ws;                                  // [k S, ws_stride]: the shadow records (and RK4 stage blocks)
  int S, T, nsub, every, ns, ctrl_per_sample;
  int ws_stride, rk_off;                       // doubles per workspace row; doubles from a row's start to its RK4 stage block (0: none)
};

// rows [row0, R) of sample r's outputs: NaN
template <typename T>
DEV void sim_fill_nan(const DevModel<T>& M, const SimDev& O, size_t r, int row0, int R) {
  WAVE_FN_K
  const double nan = (double)NAN;
  const int nq = M.nq, nv = M.nv, na = M.na, ns = O.ns;
  PHASE {
    for (int row = row0; row < R; ++row) {
      const size_t o = r * R + row;
      if (O.qpos) for (int i = lane; i < nq; i += 64) O.qpos[o * nq + i] = nan;
      if (O.qvel) for (int i = lane; i < nv; i += 64) O.qvel[o * nv + i] = nan;
      if (O.act) for (int i = lane; i < na; i += 64) O.act[o * na + i] = nan;
      if (O.site_xpos) for (int i = lane; i < 3 * ns; i += 64) O.site_xpos[o * 3 * ns + i] = nan;
      if (O.time && lane == 0) O.time[o] = nan;
    }
  }
}

template <typename T, int RKM, int NC>
DEV void env_simulate(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec0, Scratch<T, NC>& s, int block, int n_envs,
                      const SimDev& O) {
  WAVE_FN_K
  const int nq = M.nq, nv = M.nv, na = M.na, nu = M.nu, ns = O.ns, S = O.S, R = O.T / O.every;
  const size_t r = (size_t)block, e = r / (size_t)S;
  const int env = O.env_idx ? O.env_idx[e] : (int)e;
  if (env < 0 || env >= n_envs) {      // a listed index outside the batch: nothing to simulate
    sim_fill_nan(M, O, r, 0, R);
    PHASE { if (lane == 0) { if (O.bad) O.bad[r] = 1; if (O.steps) O.steps[r] = 0; } }
    return;
  }
  // ---- the shadow record: the env's, with the caller's start state (one store per element)
  GPTR(const double) src = (GPTR(const double))rec0 + (size_t)env * L.stride;
  GPTR(double) sh = (GPTR(double))O.ws + r * (size_t)O.ws_stride;
  PHASE {
    for (int i = lane; i < L.stride; i += 64) {
      double v = src[i];
      if (O.qpos0 && i >= L.off_qpos && i < L.off_qpos + nq) v = O.qpos0[r * nq + (i - L.off_qpos)];
      if (O.qvel0 && i >= L.off_qvel && i < L.off_qvel + nv) v = O.qvel0[r * nv + (i - L.off_qvel)];
      if (O.act0 && i >= L.off_act && i < L.off_act + na) v = O.act0[r * na + (i - L.off_act)];
      sh[i] = v;
    }
  }
  if constexpr (RKM == 1) {
    if (O.rk_off) { PHASE { s.rk = reinterpret_cast<RkScratch<T>*>((double*)sh + O.rk_off); } }
  }
  SYNC_G();      // (load_env's lanes read what other lanes copied)
  load_env(M, K, L, (double*)sh, s, env);
  const int goal_b = (K.kind == MYO_TASK_REORIENT_K && K.target1_sid >= 0) ? M.site_bodyid[K.target1_sid] : -1;
  const int baoding = (K.kind == 1 || K.kind == 2) && K.target1_sid >= 0 && K.target2_sid >= 0;
  // ---- the step loop
  static_assert(MYO_NQ_MAX <= 64, "one qpos entry per lane");
  LANE_VAR(HP, qkeep);
  int done = 0;
  for (int t = 0; t < O.T; ++t) {
    PHASE {
      const size_t c0 = ((O.ctrl_per_sample ? r : e) * O.T + t) * nu;
      for (int i = lane; i < nu; i += 64) ctrl_set(s, i, O.ctrl ? (T)O.ctrl[c0 + i] : (T)0);
    }
    SYNC_G();
    for (int k = 0; k < O.nsub && !s.bad; ++k) mj_step<T, RKM>(M, K, s);      // (a blown-up state is not stepped further)
    check_state(M, s, 0);      // (the state this step leaves: a later step would find it, the last one has none)
    SYNC_G();                  // (SPILL: act went to the shadow record in global memory, other lanes may read it below)
    if (s.bad) break;
    ++done;
    if ((t + 1) % O.every) continue;
    const size_t o = r * R + (size_t)((t + 1) / O.every - 1);
    PHASE {
      if (O.qpos) for (int i = lane; i < nq; i += 64) O.qpos[o * nq + i] = (double)s.qpos[i];
      if (O.qvel) for (int i = lane; i < nv; i += 64) O.qvel[o * nv + i] = (double)s.qvel[i];
      if (O.act) for (int i = lane; i < na; i += 64) O.act[o * na + i] = (double)S_ACT(M, s)[i];
      if (O.time && lane == 0) O.time[o] = (double)s.time;
    }
    if (O.site_xpos && ns > 0) {
      // the position pass at the new state; the next substep starts with its own.  kinematics normalises the free joints' quaternions
      // IN qpos (as mj_kinematics does), and a third normalisation is not the second's bits: qpos is put back as the step left it,
      // so a recorded step leaves the trajectory what it is without one
      PHASE { LV(qkeep) = lane < nq ? s.qpos[lane] : (HP)0; }
      SYNC();
      kinematics(M, s);
      PHASE {
        if (lane < nq) s.qpos[lane] = LV(qkeep);
        for (int j = lane; j < ns; j += 64) {
          const int sid = O.site_ids[j];
          HP p[3] = {(HP)NAN, (HP)NAN, (HP)NAN};
          if (sid >= 0 && sid < M.nsite) {      // (env_data's site point)
            HP xp[3], q[4], B[9], l[3];
            data_body_pose(s, M.site_bodyid[sid], goal_b, xp, q);
            quat2mat(B, q);
            for (int c = 0; c < 3; ++c) l[c] = M.h_site_pos[3 * sid + c];
            if (baoding && sid == K.target1_sid) { l[0] = s.target_xy[0]; l[1] = s.target_xy[1]; }
            if (baoding && sid == K.target2_sid) { l[0] = s.target_xy[2]; l[1] = s.target_xy[3]; }
            mulmatvec3(p, B, l);
            for (int c = 0; c < 3; ++c) p[c] += xp[c];
          }
          for (int c = 0; c < 3; ++c) O.site_xpos[(o * ns + j) * 3 + c] = (double)p[c];
        }
      }
      SYNC();
    }
  }
  // ---- a blown-up sample: the rows it did not reach are NaN
  const int bad = done < O.T;
  if (bad) sim_fill_nan(M, O, r, done / O.every, R);
  PHASE { if (lane == 0) { if (O.bad) O.bad[r] = bad; if (O.steps) O.steps[r] = done; } }
  SYNC();
  ws_release(K, s);
}

// the job of myo_batch_simulate (jobs: csrc/myo_task.h); keyed with the integrator: the rollout integrates
struct SimJob { static constexpr bool RK = true; SimDev O; };
MYO_JOB_RUN(SimJob) { env_simulate<T, V::RK ? 1 : 0>(M, K, L, rec, s, block, n_envs, J.O); }
