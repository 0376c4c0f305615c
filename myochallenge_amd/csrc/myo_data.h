// myo_data.h — the per-env kinematics and dynamics read-out (include/myobatch.h: myo_batch_data).
//
// env_data is one forward pass at the env's PRESENT state, made of the stepper's own stages in the stepper's own order (forward(),
// myo_physics.h) and seeded like env_sense (csrc/myo_sense.h): load_env — the record's qacc_warmstart, the env's ball / die
// parameters — and an optional ctrl.  It publishes, under MuJoCo's names and in MuJoCo's conventions (world frame, doubles), what
// k_step computes and throws away: body, geom and site poses, subtree centres of mass, body velocities, the mass matrix, tendon and
// actuator moment arms, the bias / passive / actuator joint forces and the accelerations.  It reads the env record and writes NOTHING
// back to it (no store_env).
//
// The pass ends after the last stage the call needs (DataDev::stage, computed by the host from the non-null pointers; the same for
// every lane of every env of the launch): a position-only call runs no CRB, no collision and no solver; only qacc needs the constraint
// rows, the collision passes and the Newton solve.  Each stage's results are published BEFORE the next stage runs: in the fp64 stepper
// the body poses and the tendon lengths share storage with vectors the later stages write, and the force vectors share LDS with the
// system matrix.  Every stage function called is the shared code; k_step's instantiations do not change.
#pragma once

enum { MYO_DATA_POS = 0, MYO_DATA_INERTIA, MYO_DATA_VEL, MYO_DATA_ACT, MYO_DATA_SMOOTH, MYO_DATA_CONSTRAINED };

// where a call publishes to: caller-owned arrays of include/myobatch.h's myo_data_out (any may be null), in its order
struct DataDev {
  double *xpos, *xquat, *xmat, *xipos, *subtree_com, *geom_xpos, *geom_xmat, *site_xpos, *cvel, *qM, *ten_J, *actuator_moment,
      *qfrc_bias, *qfrc_passive, *qfrc_actuator, *qacc_smooth, *qacc, *act_dot;
  const double* ctrl;      // dev [N, nu] (null: 0)
  int stage;               // the last stage the call needs (MYO_DATA_*)
};

// world pose of body b as MuJoCo holds it: the kinematics stage's, except for the die's goal body, which the task keeps at the
// episode's goal pose (reorient.py writes body_pos / body_quat of `target`; env_geom_poses draws it there)
template <typename T, int NC>
DEV void data_body_pose(const Scratch<T, NC>& s, int b, int goal_b, HP* xp, HP* q) {
  if (b == goal_b) {
    const HP* g = s.goal_quat;
    const HP n = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3]);
    for (int k = 0; k < 4; ++k) q[k] = g[k] / n;
    for (int k = 0; k < 3; ++k) xp[k] = s.goal_pos[k];
  } else {
    for (int k = 0; k < 4; ++k) q[k] = S_XQUAT(s)[4 * b + k];
    for (int k = 0; k < 3; ++k) xp[k] = S_XPOS(s)[3 * b + k];
  }
}
// ... and of its inertial frame's origin
template <typename T, int NC>
DEV void data_body_ipos(const DevModel<T>& M, const Scratch<T, NC>& s, int b, int goal_b, HP* out) {
  HP xp[3], q[4], R[9];
  data_body_pose(s, b, goal_b, xp, q);
  quat2mat(R, q);
  const HP ip[3] = {(HP)M.body_ipos[3 * b], (HP)M.body_ipos[3 * b + 1], (HP)M.body_ipos[3 * b + 2]};
  mulmatvec3(out, R, ip);
  for (int k = 0; k < 3; ++k) out[k] += xp[k];
}

template <typename T, int NC>
DEV void env_data(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s, int env, const DataDev& O) {
  WAVE_FN_K
  const int nb = M.nbody, nv = M.nv, nu = M.nu, ng = M.ngeom, ns = M.nsite, nt = M.ntendon, stage = O.stage;
  const size_t e = (size_t)env;
  GPTR(double) qM = O.qM ? (GPTR(double))O.qM + e * nv * nv : (GPTR(double))0;
  GPTR(double) tJ = O.ten_J ? (GPTR(double))O.ten_J + e * nt * nv : (GPTR(double))0;
  GPTR(double) aM = O.actuator_moment ? (GPTR(double))O.actuator_moment + e * nu * nv : (GPTR(double))0;
  load_env(M, K, L, rec, s, env);
  PHASE {
    for (int i = lane; i < nu; i += 64) ctrl_set(s, i, O.ctrl ? (T)O.ctrl[e * nu + i] : (T)0);
    // the dense arrays: zero outside the pattern
    if (qM) for (int i = lane; i < nv * nv; i += 64) qM[i] = 0;
    if (tJ) for (int i = lane; i < nt * nv; i += 64) tJ[i] = 0;
    if (aM) for (int i = lane; i < nu * nv; i += 64) aM[i] = 0;
  }
  SYNC_G();      // (other lanes write the same rows below)
  // ---- position stage: forward()'s sequence
  kinematics(M, s);
  com_pos(M, K, s);
  {
    const int goal_b = (K.kind == MYO_TASK_REORIENT_K && K.target1_sid >= 0) ? M.site_bodyid[K.target1_sid] : -1;
    const int baoding = (K.kind == 1 || K.kind == 2) && K.target1_sid >= 0 && K.target2_sid >= 0;
    PHASE {
      const int b = lane;
      if (b < nb) {
        HP xp[3], q[4], R[9], ip[3];
        data_body_pose(s, b, goal_b, xp, q);
        quat2mat(R, q);
        data_body_ipos(M, s, b, goal_b, ip);
        for (int k = 0; k < 3; ++k) {
          if (O.xpos) O.xpos[(e * nb + b) * 3 + k] = xp[k];
          if (O.xipos) O.xipos[(e * nb + b) * 3 + k] = ip[k];
        }
        for (int k = 0; k < 4; ++k) if (O.xquat) O.xquat[(e * nb + b) * 4 + k] = q[k];
        for (int k = 0; k < 9; ++k) if (O.xmat) O.xmat[(e * nb + b) * 9 + k] = R[k];
      }
      for (int g = lane; g < ng; g += 64) {
        HP xp[3], q[4], B[9], l[3], p[3], R[9];
        data_body_pose(s, M.geom_bodyid[g], goal_b, xp, q);
        quat2mat(B, q);
        geom_lpos_hp(M, K, s, g, l);      // (the die's geoms move outward by the env's size delta)
        mulmatvec3(p, B, l);
        mulmat3(R, B, M.h_geom_mat + 9 * g);
        for (int k = 0; k < 3; ++k) if (O.geom_xpos) O.geom_xpos[(e * ng + g) * 3 + k] = p[k] + xp[k];
        for (int k = 0; k < 9; ++k) if (O.geom_xmat) O.geom_xmat[(e * ng + g) * 9 + k] = R[k];
      }
      if (O.site_xpos)
        for (int sid = lane; sid < ns; sid += 64) {
          HP xp[3], q[4], B[9], l[3], p[3];
          data_body_pose(s, M.site_bodyid[sid], goal_b, xp, q);
          quat2mat(B, q);
          for (int k = 0; k < 3; ++k) l[k] = M.h_site_pos[3 * sid + k];
          if (baoding && sid == K.target1_sid) { l[0] = s.target_xy[0]; l[1] = s.target_xy[1]; }      // (as baoding_obs_reward places them)
          if (baoding && sid == K.target2_sid) { l[0] = s.target_xy[2]; l[1] = s.target_xy[3]; }
          mulmatvec3(p, B, l);
          for (int k = 0; k < 3; ++k) O.site_xpos[(e * ns + sid) * 3 + k] = p[k] + xp[k];
        }
    }
    SYNC();
    if (O.subtree_com) {
      // mj_comPos's subtree sums for EVERY body (the stepper keeps the tree roots' only, S_COM): mass-weighted xipos summed up the
      // tree, one lane per component, in doubles.  Staged from bvec on: body vectors and constraint rows are not live before the
      // tendon stage.
      typedef Scratch<T, NC> S;
      static_assert(offsetof(S, efc_force) - offsetof(S, bvec) >= 4 * MYO_NB_MAX * sizeof(double) && offsetof(S, bvec) % 8 == 0, "subtree sums fit in bvec, efc_jv");
      double* const acc = reinterpret_cast<double*>(s.bvec);
      PHASE {
        const int b = lane;
        if (b < nb) {
          HP ip[3];
          data_body_ipos(M, s, b, goal_b, ip);
          const double m = (double)body_mass_of(M, K, s, b);
          for (int k = 0; k < 3; ++k) acc[4 * b + k] = m * ip[k];
          acc[4 * b + 3] = m;
        }
      }
      SYNC();
      PHASE {
        if (lane < 4)
          for (int b = nb - 1; b > 0; --b) acc[4 * M.body_parentid[b] + lane] += acc[4 * b + lane];
      }
      SYNC();
      PHASE {
        const int b = lane;
        if (b < nb) {
          HP ip[3];
          data_body_ipos(M, s, b, goal_b, ip);
          const double m = acc[4 * b + 3];
          for (int k = 0; k < 3; ++k) O.subtree_com[(e * nb + b) * 3 + k] = m < (double)MYO_MINVAL ? ip[k] : acc[4 * b + k] / m;
        }
      }
      SYNC();
    }
  }
  tendon(M, K, s);
  for (int base = 0; base < M.ngw; base += 64) tendon_wrap_pass(M, K, s, base);
  for (int base = 0; base < M.nte; base += 64) tendon_element_pass(M, K, s, base);
  tendon_length_sums(M, s);
  PHASE {
    if (tJ)
      for (int t = lane; t < nt; t += 64) {
        unsigned long long m = M.tendon_dofmask[t];
        int slot = 0;
        while (m) { const int d = myo_ffsll(m); m &= m - 1; tJ[t * nv + d] = (double)tenj_get(s, t, slot); slot++; }
      }
    if (aM)
      for (int i = lane; i < nu; i += 64) {      // mj_transmission, tendon transmissions: gear times the tendon's row
        const int t = M.actuator_tendon[i];
        const T gear = M.actuator_gear[6 * i];
        unsigned long long m = M.tendon_dofmask[t];
        int slot = 0;
        while (m) { const int d = myo_ffsll(m); m &= m - 1; aM[i * nv + d] = (double)(gear * tenj_get(s, t, slot)); slot++; }
      }
  }
  SYNC();
  do {
    if (stage < MYO_DATA_INERTIA) break;
    // ---- inertia
    crb(M, s);
    PHASE {
      if (qM)
        for (int k = lane; k < M.nM; k += 64) {
          const int i = M.M_i[k], j = M.M_j[k];
          const double v = (double)s.qM[k];
          qM[i * nv + j] = v;
          qM[j * nv + i] = v;
        }
    }
    SYNC();
    if (stage < MYO_DATA_VEL) break;
    // ---- the constraint set: only the constrained acceleration needs it (nefc stays 0 otherwise, load_env)
    if (stage >= MYO_DATA_CONSTRAINED) {
      if (M.any_floss) friction_rows(M, K, s, 0);
      constraint_limits(M, K, s);
      if (M.any_floss) friction_rows(M, K, s, 1);
      if (M.any_gen) {
        for (int base = 0; base < M.npair_std; base += 64) collision_pass<true>(M, K, s, base);
        for (int base = M.npair_std; base < M.npair; base += 64) collision_pass_ext<true>(M, K, s, base - M.npair_std);
      } else {
        for (int base = 0; base < M.npair_std; base += 64) collision_pass<false>(M, K, s, base);
        for (int base = M.npair_std; base < M.npair; base += 64) collision_pass_ext<false>(M, K, s, base - M.npair_std);
      }
      contacts_clamp(K, s);      // (a surplus is counted in the batch's health counters, as for a substep)
    }
    // ---- velocity
    body_vectors(M, s, LOFF(s, S_QVELT(s)), LOFF(s, S_CVEL(s)));
    fwd_velocity(M, K, s);
    PHASE {      // (the body velocities live in the solver's vectors, the force vectors in the system matrix)
      if (O.cvel) for (int i = lane; i < 6 * nb; i += 64) O.cvel[e * nb * 6 + i] = (double)S_CVEL(s)[i];
      for (int i = lane; i < nv; i += 64) {
        if (O.qfrc_bias) O.qfrc_bias[e * nv + i] = (double)S_QFRC_BIAS(s)[i];
        if (O.qfrc_passive) O.qfrc_passive[e * nv + i] = (double)S_QFRC_PASSIVE(s)[i];
      }
    }
    SYNC();
    if (stage < MYO_DATA_ACT) break;
    // ---- actuation
    if (stage >= MYO_DATA_CONSTRAINED) efc_reference(M, s);
    fwd_actuation(M, s);
    PHASE {
      for (int i = lane; i < nv; i += 64) if (O.qfrc_actuator) O.qfrc_actuator[e * nv + i] = (double)S_QFRC_ACTUATOR(s)[i];
      for (int i = lane; i < M.na; i += 64) if (O.act_dot) O.act_dot[e * M.na + i] = (double)S_ACT_DOT(s)[i];
    }
    SYNC();
    if (stage < MYO_DATA_SMOOTH) break;
    // ---- acceleration: fwd_acceleration's unconstrained solve alone, or all of it (the Newton solve from the env's warm start)
    if (stage >= MYO_DATA_CONSTRAINED) fwd_acceleration(M, s);
    else {
      PHASE { const int c = lane; if (c < nv) s.qacc_smooth[c] = s.qfrc_smooth[c]; }
      SYNC();
      solve_M(M, s, s.qacc_smooth, 0);
    }
    PHASE {
      for (int i = lane; i < nv; i += 64) {
        if (O.qacc_smooth) O.qacc_smooth[e * nv + i] = (double)s.qacc_smooth[i];
        if (O.qacc && stage >= MYO_DATA_CONSTRAINED) O.qacc[e * nv + i] = (double)s.qacc[i];
      }
    }
    SYNC();
  } while (0);
  ws_release(K, s);
}

// the job of myo_batch_data (jobs: csrc/myo_task.h); keyed without the integrator, a forward pass integrates nothing
struct DataJob { static constexpr bool RK = false; DataDev O; };
MYO_JOB_RUN(DataJob) { env_data(M, K, L, MYO_ENV_REC(block), s, block, J.O); }
