// myo_jac.h — per-env Jacobians and inverse dynamics (include/myobatch.h: myo_batch_jac, myo_batch_inverse).
//
// Two read-outs of their own beside env_data (csrc/myo_data.h), each one pass at the env's PRESENT state made of the stepper's own
// stages, seeded by load_env like env_sense / env_data, with ctrl = 0.  Both read the env record and write NOTHING back to it (no
// store_env).  Every stage function called is the shared code; k_step's instantiations do not change.
//
// env_jac      mj_jacBody / mj_jacBodyCom / mj_jacSite / mj_jacGeom / mj_jac / mj_jacSubtreeCom: the position stage alone
//              (kinematics, com_pos), then lanes = (object, dof) pairs.  Column i of an object on body b at world point p is
//                jacp = cdof_lin(i) + cdof_ang(i) x (p - subtree_com[root(b)]),  jacr = cdof_ang(i)      if dof i moves b, else 0
//              — membership is bit i of the model's per-body ancestor-dof mask (body_dofmask, built once on the host: myo_host.h),
//              no tree walk.  The points are the ones env_data publishes (data_body_pose, data_body_ipos, geom_lpos_hp, the Baoding
//              target sites where the task puts them).  What com_pos leaves is read in place: s.cdof, the tree reference points
//              (S_COM + S_ORIGIN) and — fp64 stepper — the body poses inside the solver's seven dof vectors, which nothing here writes;
//              the per-object points are staged from bvec on (dead until the velocity stage, as env_data's subtree sums).
// env_inverse  mj_inverse: env_data's constraint-carrying pass (MYO_DATA_CONSTRAINED) up to and including efc_reference, without the
//              actuation stage, then what newton_solve does before its first iteration with the caller's qacc in the place of the
//              warm start: jar = J qacc - aref, M qacc, one update_constraint -> efc_force, qfrc_constraint.  No Newton solve.
//              qfrc_bias / qfrc_passive live in the system matrix H, which only the Newton system overwrites: they are still there at
//              the end.  The caller's qacc is loaded AFTER efc_reference, into `search` (M qacc -> Mv): the body velocities that
//              efc_reference reads (S_CVEL) live in qfrc_constraint .. Mv until then.
#pragma once

enum { MYO_JAC_K_BODY = 0, MYO_JAC_K_BODYCOM, MYO_JAC_K_SITE, MYO_JAC_K_GEOM, MYO_JAC_K_SUBTREECOM };      // == MYO_JAC_* of include/myobatch.h (checked in myo_host.h)
#define MYO_JAC_CHUNK 32      /* objects whose points are staged at a time (4 doubles each, from bvec on) */

// what a call asks for: k objects of one type (ids: dev int32[k]), optional world points [N, k, 3] (BODY only), outputs [N, k, 3, nv]
struct JacDev {
  int objtype, k;
  const int* ids;
  const double* points;
  double *jacp, *jacr;
};

template <typename T, int NC>
DEV void env_jac(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s, int env, const JacDev& O) {
  WAVE_FN_K
  const int nb = M.nbody, nv = M.nv, ng = M.ngeom, ns = M.nsite, k = O.k, objtype = O.objtype;
  const size_t e = (size_t)env;
  GPTR(double) jp = O.jacp ? (GPTR(double))O.jacp + e * k * 3 * nv : (GPTR(double))0;
  GPTR(double) jr = O.jacr ? (GPTR(double))O.jacr + e * k * 3 * nv : (GPTR(double))0;
  GPTR(const int) ids = (GPTR(const int))O.ids;
  GPTR(const double) pts = O.points ? (GPTR(const double))O.points + e * k * 3 : (GPTR(const double))0;
  load_env(M, K, L, rec, s, env);
  // ---- position stage: forward()'s sequence
  kinematics(M, s);
  com_pos(M, K, s);
  const int goal_b = (K.kind == MYO_TASK_REORIENT_K && K.target1_sid >= 0) ? M.site_bodyid[K.target1_sid] : -1;
  const int baoding = (K.kind == 1 || K.kind == 2) && K.target1_sid >= 0 && K.target2_sid >= 0;
  // staging: 4 doubles per object (or per body) from bvec on — body vectors and constraint rows are not live before the velocity stage
  typedef Scratch<T, NC> S;
  static_assert(offsetof(S, efc_force) - offsetof(S, bvec) >= 4 * MYO_JAC_CHUNK * sizeof(double) &&
                offsetof(S, efc_force) - offsetof(S, bvec) >= 4 * MYO_NB_MAX * sizeof(double) && offsetof(S, bvec) % 8 == 0, "jac staging fits in bvec, efc_jv");
  double* const stg = reinterpret_cast<double*>(s.bvec);
  if (objtype == MYO_JAC_K_SUBTREECOM) {
    // per body: offset of its inertial frame's origin from its tree's reference point, and its mass (the env's own for the balls)
    PHASE {
      const int b = lane;
      if (b < nb) {
        HP ip[3];
        data_body_ipos(M, s, b, goal_b, ip);
        const int root = M.body_rootid[b];
        for (int c = 0; c < 3; ++c) stg[4 * b + c] = ip[c] - ((HP)S_COM(s)[3 * root + c] + S_ORIGIN(s)[c]);
        stg[4 * b + 3] = (double)body_mass_of(M, K, s, b);
      }
    }
    SYNC();
    // lanes = (object, dof): the mass-weighted sum of the bodycom columns over the object's subtree, in doubles, in body order
    PHASE {
      for (int idx = lane; idx < k * nv; idx += 64) {
        const int o = idx / nv, i = idx - o * nv;
        const int id = ids[o];
        const bool valid = id >= 0 && id < nb;
        const int b = valid ? id : 0;
        const unsigned long long sub = b == 0 ? ~0ull : M.body_submask[b];      // (the world's subtree is every body)
        const double a[3] = {(double)s.cdof[6 * i], (double)s.cdof[6 * i + 1], (double)s.cdof[6 * i + 2]};
        const double l[3] = {(double)s.cdof[6 * i + 3], (double)s.cdof[6 * i + 4], (double)s.cdof[6 * i + 5]};
        double acc[3] = {0, 0, 0}, mass = 0;
        for (int c = 1; c < nb; ++c) {
          const bool in = (sub >> c) & 1ull, on = (M.body_dofmask[c] >> i) & 1ull;
          const double m = in ? stg[4 * c + 3] : 0.0;
          const double r[3] = {stg[4 * c], stg[4 * c + 1], stg[4 * c + 2]};
          double t[3];
          cross3(t, a, r);
          mass += m;
          if (on) for (int q = 0; q < 3; ++q) acc[q] += m * (l[q] + t[q]);
        }
        if (mass < (double)MYO_MINVAL) {      // a massless subtree: subtree_com is the body's own xipos (env_data)
          const bool on = (M.body_dofmask[b] >> i) & 1ull;
          const double r[3] = {stg[4 * b], stg[4 * b + 1], stg[4 * b + 2]};
          double t[3];
          cross3(t, a, r);
          for (int q = 0; q < 3; ++q) acc[q] = on ? l[q] + t[q] : 0.0;
          mass = 1;
        }
        const size_t row = (size_t)o * 3 * nv + i;
        for (int q = 0; q < 3; ++q) jp[row + (size_t)q * nv] = valid ? acc[q] / mass : 0.0;
      }
    }
    SYNC();
  } else {
    for (int o0 = 0; o0 < k; o0 += MYO_JAC_CHUNK) {
      const int nc = k - o0 < MYO_JAC_CHUNK ? k - o0 : MYO_JAC_CHUNK;
      // lanes = objects of the chunk: the point's offset from its tree's reference point, and its body (-1: an id outside the model)
      PHASE {
        const int o = lane;
        if (o < nc) {
          const int id = ids[o0 + o];
          int body = -1;
          HP p[3] = {0, 0, 0};
          if (objtype == MYO_JAC_K_BODY) {
            if (id >= 0 && id < nb) {
              body = id;
              if (pts) { for (int c = 0; c < 3; ++c) p[c] = pts[(size_t)(o0 + o) * 3 + c]; }
              else { HP q[4]; data_body_pose(s, id, goal_b, p, q); }
            }
          } else if (objtype == MYO_JAC_K_BODYCOM) {
            if (id >= 0 && id < nb) { body = id; data_body_ipos(M, s, id, goal_b, p); }
          } else if (objtype == MYO_JAC_K_SITE) {
            if (id >= 0 && id < ns) {
              body = M.site_bodyid[id];
              HP xp[3], q[4], B[9], l[3];
              data_body_pose(s, body, goal_b, xp, q);
              quat2mat(B, q);
              for (int c = 0; c < 3; ++c) l[c] = M.h_site_pos[3 * id + c];
              if (baoding && id == K.target1_sid) { l[0] = s.target_xy[0]; l[1] = s.target_xy[1]; }      // (as env_data places them)
              if (baoding && id == K.target2_sid) { l[0] = s.target_xy[2]; l[1] = s.target_xy[3]; }
              mulmatvec3(p, B, l);
              for (int c = 0; c < 3; ++c) p[c] += xp[c];
            }
          } else {
            if (id >= 0 && id < ng) {
              body = M.geom_bodyid[id];
              HP xp[3], q[4], B[9], l[3];
              data_body_pose(s, body, goal_b, xp, q);
              quat2mat(B, q);
              geom_lpos_hp(M, K, s, id, l);      // (the die's geoms move outward by the env's size delta)
              mulmatvec3(p, B, l);
              for (int c = 0; c < 3; ++c) p[c] += xp[c];
            }
          }
          const int root = body >= 0 ? M.body_rootid[body] : 0;
          for (int c = 0; c < 3; ++c) stg[4 * o + c] = p[c] - ((HP)S_COM(s)[3 * root + c] + S_ORIGIN(s)[c]);
          stg[4 * o + 3] = (double)body;
        }
      }
      SYNC();
      // lanes = (object, dof), consecutive lanes on consecutive dofs of one output row
      PHASE {
        for (int idx = lane; idx < nc * nv; idx += 64) {
          const int o = idx / nv, i = idx - o * nv;
          const int body = (int)stg[4 * o + 3];
          const bool on = body >= 0 && ((M.body_dofmask[body >= 0 ? body : 0] >> i) & 1ull);
          const double a[3] = {(double)s.cdof[6 * i], (double)s.cdof[6 * i + 1], (double)s.cdof[6 * i + 2]};
          const double l[3] = {(double)s.cdof[6 * i + 3], (double)s.cdof[6 * i + 4], (double)s.cdof[6 * i + 5]};
          const double r[3] = {stg[4 * o], stg[4 * o + 1], stg[4 * o + 2]};
          double t[3];
          cross3(t, a, r);
          const size_t row = (size_t)(o0 + o) * 3 * nv + i;
          if (jp) for (int q = 0; q < 3; ++q) jp[row + (size_t)q * nv] = on ? l[q] + t[q] : 0.0;
          if (jr) for (int q = 0; q < 3; ++q) jr[row + (size_t)q * nv] = on ? a[q] : 0.0;
        }
      }
      SYNC();
    }
  }
  ws_release(K, s);
}

// the job of myo_batch_jac (jobs: csrc/myo_task.h); keyed without the integrator, a position pass integrates nothing
struct JacJob { static constexpr bool RK = false; JacDev O; };
MYO_JOB_RUN(JacJob) { env_jac(M, K, L, MYO_ENV_REC(block), s, block, J.O); }

// ---- inverse dynamics
struct InverseDev {
  const double* qacc;      // dev [N, nv]
  double *qfrc_inverse, *qfrc_constraint;
};

template <typename T, int NC>
DEV void env_inverse(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s, int env, const InverseDev& O) {
  WAVE_FN_K
  const int nv = M.nv, nu = M.nu;
  const size_t e = (size_t)env;
  load_env(M, K, L, rec, s, env);
  PHASE { for (int i = lane; i < nu; i += 64) ctrl_set(s, i, (T)0); }
  SYNC_G();
  // ---- position and inertia stages: forward()'s sequence
  kinematics(M, s);
  com_pos(M, K, s);
  tendon(M, K, s);
  for (int base = 0; base < M.ngw; base += 64) tendon_wrap_pass(M, K, s, base);
  for (int base = 0; base < M.nte; base += 64) tendon_element_pass(M, K, s, base);
  tendon_length_sums(M, s);
  crb(M, s);
  // ---- the constraint set
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
  // ---- velocity, reference accelerations; no actuation stage
  body_vectors(M, s, LOFF(s, S_QVELT(s)), LOFF(s, S_CVEL(s)));
  fwd_velocity(M, K, s);
  efc_reference(M, s);
  // ---- the caller's acceleration (the body velocities that lived in qfrc_constraint .. Mv are dead now), through the three products
  // of a Newton iteration on the very vectors the solver uses for its search direction: M a -> Mv, body vectors -> bvec, J a -> efc_jv
  PHASE { const int c = lane; if (c < nv) s.search[c] = (T)O.qacc[e * nv + c]; }
  SYNC();
  mul_M(M, s, LOFF(s, s.Mv), LOFF(s, s.search));
  body_vectors(M, s, LOFF(s, s.search), LOFF(s, s.bvec));
  J_times(M, s, LOFF(s, s.search), LOFF(s, s.bvec), LOFF(s, s.efc_jv));
  const int nefc = s.nefc;
  PHASE { for (int r = lane; r < nefc; r += 64) s.efc_jar[r] = s.efc_jv[r] - S_AREF(s)[r]; }      // (aref lives in efc_jar: in place)
  SYNC();
  // one constraint update: efc_force, qfrc_constraint = J' efc_force.  (Its cost and gradient read Ma, qacc, qfrc_smooth and qacc_smooth,
  // which this pass never fills: both results are dropped, and the gradient it leaves in `search` is not used.)
  (void)update_constraint(M, s);
  PHASE {      // (the bias and passive forces are still in the system matrix: no Newton system was loaded)
    for (int i = lane; i < nv; i += 64) {
      const double fc = (double)s.qfrc_constraint[i];
      if (O.qfrc_constraint) O.qfrc_constraint[e * nv + i] = fc;
      if (O.qfrc_inverse) O.qfrc_inverse[e * nv + i] = (double)s.Mv[i] + (double)S_QFRC_BIAS(s)[i] - (double)S_QFRC_PASSIVE(s)[i] - fc;
    }
  }
  SYNC();
  ws_release(K, s);
}

// the job of myo_batch_inverse
struct InverseJob { static constexpr bool RK = false; InverseDev O; };
MYO_JOB_RUN(InverseJob) { env_inverse(M, K, L, MYO_ENV_REC(block), s, block, J.O); }
