// myo_sense.h — the per-env contact and muscle read-out (include/myobatch.h: myo_batch_sense).
//
// env_sense is one forward pass at the env's PRESENT state, made of the stepper's own stages in the stepper's own order (forward(),
// myo_physics.h) and seeded like the next substep would be (load_env: the record's qacc_warmstart, the env's ball / die parameters),
// that publishes what k_step computes and throws away: the contact list with MuJoCo's mj_contactForce decoding of the solved
// pyramidal efc_force, the net contact wrench per body, qfrc_constraint, and the muscle-tendon lengths, velocities and forces.
// It reads the env record and writes NOTHING back to it (no store_env): the warm start, the step plan's generation and the wrap order
// stay what they were.  Controls are not part of an env's state between two steps: the pass runs with ctrl = 0, which enters the
// activation RATES only — no published quantity depends on it for actuators with an activation state (the muscles).
//
// The two collision passes are the only stage with a sense twin (sense_collision_pass): a contact record keeps neither the geom pair
// nor the distance (they are consumed where the record is built), so the twin runs the same narrow phase and the same contacts_emit
// and then publishes pair, distance, point and normal from the lane that found the contact.  Everything it calls is the shared code;
// k_step's instantiations do not change.
#pragma once

// where a call publishes to: caller-owned arrays of include/myobatch.h's myo_sense_out (any may be null), `cap` contact slots per env
struct SenseDev {
  int* ncon; int* con_geom; double* con_d; double* body_wrench; double* qfrc_constraint;
  double *act_length, *act_velocity, *act_force, *activation, *ten_length, *ten_velocity;
  int cap;
};
#define MYO_SENSE_CON_N 13      /* doubles per contact of con_d: dist, pos[3], normal[3], force[6] */

// One pass over 64 candidate pairs: collision_pass / collision_pass_ext (EXT) with the read-out behind the emission.  cg / cd: the env's
// rows of con_geom / con_d (null: not asked for).  nct = contacts published by the passes before this one; returns the new count.
// A contact is published when its FIRST slot fits the capacity (the slots beyond it are never written: contacts_clamp), at the index
// MuJoCo would give it among the kept ones: contacts in pair order, which is also the order of their slots.
template <bool GEN, bool EXT, typename T, int NC>
DEVFN int sense_collision_pass(const DevModel<T>& M_in, const TaskDev& K_in, Scratch<T, NC>& s_in, int base, int* cg_in, double* cd_in, int nct) {
  MYO_BIND_M(T) MYO_BIND_K MYO_BIND_S(T)
  WAVE_FN
  GPTR(int) cg = (GPTR(int))cg_in;
  GPTR(double) cd = (GPTR(double))cd_in;
  const int nlim = s.nl + s.ntl, ncon0 = s.ncon;
  const int p0 = EXT ? M.npair_std + base : base, pend = EXT ? M.npair : M.npair_std;
  int ncon = ncon0;
  LANE_VAR(ContactTmp, ct);
  PHASE {
    const int p = p0 + lane;
    LV(ct).n = 0;
    if (p < pend) {
      const int g1 = M.pair_geom1[p], g2 = M.pair_geom2[p];
      const HP margin = GEN ? M.h_pair_mg[2 * p] : tmax(M.h_geom_margin[g1], M.h_geom_margin[g2]);
      if (!pair_far_apart(M, K, s, g1, g2, margin)) {
        if constexpr (EXT) collide_pair_ext(M, K, s, g1, g2, M.pc_i[8 * p + 5], margin, LV(ct));
        else collide_pair(M, K, s, g1, g2, margin, LV(ct));
        pair_keep_included(M, g1, g2, margin, LV(ct), GEN ? p : -1);
      }
    }
  }
  contacts_emit<GEN>(M, K, s, p0, ct, ncon);      // (leaves the lanes' slot prefix in S_NPRE)
  // the lanes' CONTACT prefix (a contact of condim 4 / 6 takes two / three slots): behind the slot prefix
  int* const cpre = S_NPRE(s) + 64;
  static_assert(128 * sizeof(int) <= (MYO_NLIM_MAX + 4 * NC) * sizeof(T), "two lane prefixes fit in efc_jv");
  int total = 0;
  WAVE_EXSCAN(LV(ct).n, cpre, total);
  const int cap = tmin((int)Scratch<T, NC>::NREC, (MYO_NLIM_MAX + 4 * NC - nlim) >> 2);
  PHASE {
    const int p = p0 + lane, n = LV(ct).n;
    const int pp = n > 0 ? p : 0;                 // (lanes without a contact read pair 0: a valid address)
    const int g1 = M.pair_geom1[pp], g2 = M.pair_geom2[pp];
    const int dim = GEN ? (M.pc_i[8 * pp + 6] & 255) : 3, per = dim == 6 ? 3 : (dim == 4 ? 2 : 1);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k >= n || ncon0 + S_NPRE(s)[lane] + k * per >= cap) break;
      const int ci = nct + cpre[lane] + k;        // (<= its first slot's index < cap)
      if (cg) { cg[2 * ci] = g1; cg[2 * ci + 1] = g2; }
      if (cd) {
        cd[MYO_SENSE_CON_N * ci] = (double)LV(ct).dist[k];
        for (int e = 0; e < 3; ++e) { cd[MYO_SENSE_CON_N * ci + 1 + e] = (double)LV(ct).pos[3 * k + e]; cd[MYO_SENSE_CON_N * ci + 4 + e] = (double)LV(ct).nrm[3 * k + e]; }
      }
    }
    if (lane == 0) { s.ncon = ncon; s.nefc = nlim + 4 * ncon; }
  }
  SYNC();
  return nct + total;
}

template <typename T, int NC>
DEV void env_sense(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s, int env, const SenseDev& O) {
  WAVE_FN_K
  const int cap = O.cap, nb = M.nbody, nv = M.nv;
  GPTR(int) cg = O.con_geom ? (GPTR(int))O.con_geom + (size_t)env * cap * 2 : (GPTR(int))0;
  GPTR(double) cd = O.con_d ? (GPTR(double))O.con_d + (size_t)env * cap * MYO_SENSE_CON_N : (GPTR(double))0;
  GPTR(double) bw = O.body_wrench ? (GPTR(double))O.body_wrench + (size_t)env * nb * 6 : (GPTR(double))0;
  load_env(M, K, L, rec, s, env);
  PHASE {
    if (cg) for (int i = lane; i < 2 * cap; i += 64) cg[i] = -1;
    if (cd) for (int i = lane; i < MYO_SENSE_CON_N * cap; i += 64) cd[i] = 0;
  }
  SYNC_G();      // (other lanes write the same rows below)
  // ---- position stage: forward()'s sequence
  kinematics(M, s);
  com_pos(M, K, s);
  tendon(M, K, s);
  for (int base = 0; base < M.ngw; base += 64) tendon_wrap_pass(M, K, s, base);
  for (int base = 0; base < M.nte; base += 64) tendon_element_pass(M, K, s, base);
  tendon_length_sums(M, s);
  crb(M, s);
  if (M.any_floss) friction_rows(M, K, s, 0);
  constraint_limits(M, K, s);
  if (M.any_floss) friction_rows(M, K, s, 1);
  {
    int nct = 0;
    int* const cgp = (int*)cg; double* const cdp = (double*)cd;
    if (M.any_gen) {
      for (int base = 0; base < M.npair_std; base += 64) nct = sense_collision_pass<true, false>(M, K, s, base, cgp, cdp, nct);
      for (int base = M.npair_std; base < M.npair; base += 64) nct = sense_collision_pass<true, true>(M, K, s, base - M.npair_std, cgp, cdp, nct);
    } else {
      for (int base = 0; base < M.npair_std; base += 64) nct = sense_collision_pass<false, false>(M, K, s, base, cgp, cdp, nct);
      for (int base = M.npair_std; base < M.npair; base += 64) nct = sense_collision_pass<false, true>(M, K, s, base - M.npair_std, cgp, cdp, nct);
    }
  }
  contacts_clamp(K, s);      // (a surplus is counted in the batch's health counters, as for a substep)
  // what lives in storage the later stages take over: the tendon lengths, and — the body poses and the trees' reference points share
  // the solver's vectors in the fp64 stepper — per body the offset from its frame origin to its tree's reference point, which turns a
  // contact record's r1 / r2 into the arm about xpos.  Staged in the wrench rows themselves until the forces are known.
  PHASE {
    for (int t = lane; t < M.ntendon; t += 64) {
      const double len = (double)S_TEN_LENGTH(s)[t];
      if (O.ten_length) O.ten_length[(size_t)env * M.ntendon + t] = len;
    }
    for (int i = lane; i < M.nu; i += 64) {
      const int tid = M.actuator_tendon[i];
      const T gear = M.actuator_gear[6 * i];
      if (O.act_length) O.act_length[(size_t)env * M.nu + i] = (double)((HP)gear * S_TEN_LENGTH(s)[tid]);
    }
    for (int i = lane; i < M.na; i += 64) if (O.activation) O.activation[(size_t)env * M.na + i] = (double)S_ACT(M, s)[i];
    if (bw)
      for (int b = lane; b < nb; b += 64)
        for (int k = 0; k < 3; ++k) bw[6 * b + k] = ((double)S_COM(s)[3 * M.body_rootid[b] + k] + (double)S_ORIGIN(s)[k]) - (double)S_XPOS(s)[3 * b + k];
  }
  SYNC_G();
  // ---- velocity, actuation
  body_vectors(M, s, LOFF(s, S_QVELT(s)), LOFF(s, S_CVEL(s)));
  fwd_velocity(M, K, s);
  efc_reference(M, s);
  fwd_actuation(M, s);
  PHASE {      // (tendon velocities and actuator forces live in the solver's vectors)
    for (int t = lane; t < M.ntendon; t += 64) if (O.ten_velocity) O.ten_velocity[(size_t)env * M.ntendon + t] = (double)S_TEN_VEL(s)[t];
    for (int i = lane; i < M.nu; i += 64) {
      const int tid = M.actuator_tendon[i];
      const T gear = M.actuator_gear[6 * i], tv = S_TEN_VEL(s)[tid], f = S_ACT_FORCE(s)[i];
      if (O.act_velocity) O.act_velocity[(size_t)env * M.nu + i] = (double)(gear * tv);
      if (O.act_force) O.act_force[(size_t)env * M.nu + i] = (double)f;
    }
  }
  SYNC();
  // ---- acceleration: the Newton solve from the env's warm start
  fwd_acceleration(M, s);
  const int ncon = s.ncon, nlim = s.nl + s.ntl;
  T* const acc = S_SOLVE_STAGE(s);               // per-body wrench sums [body][force, torque]: bvec is free once the system is solved
  int* const first = S_NPRE(s);                  // (efc_jv: J v of the last line search is dead)
  PHASE {
    for (int i = lane; i < nv; i += 64) if (O.qfrc_constraint) O.qfrc_constraint[(size_t)env * nv + i] = (double)s.qfrc_constraint[i];
    for (int i = lane; i < 6 * nb; i += 64) acc[i] = 0;
  }
  SYNC();
  // a contact's index among the kept ones = the first slots (kind 0 or 3) in front of its own
  LANE_VAR(int, isfirst);
  PHASE {
    const int kd = lane < ncon ? con_kind(CON(s, lane)) : 1;
    LV(isfirst) = kd == 0 || kd == 3;
  }
  int nfirst = 0;
  WAVE_EXSCAN(LV(isfirst), first, nfirst);
  static_assert(MYO_NCON_BIG <= 64, "one contact slot per lane");
  PHASE {
    const int ci = lane;
    if (ci < ncon) {
      // the slot's record and rows, requested together
      const auto& c = CON(s, ci);
      const int kind = con_kind(c), b1 = con_b1(c), b2 = con_b2(c);
      const T muA = c.muA, muB = c.muB;
      const T r1[3] = {c.r1[0], c.r1[1], c.r1[2]}, r2[3] = {c.r2[0], c.r2[1], c.r2[2]};
      const T* fe = s.efc_force + nlim + 4 * ci;
      const T f0 = fe[0], f1 = fe[1], f2 = fe[2], f3 = fe[3];
      T fr[6], t2[3];
      con_frame(c, fr);
      con_t2(fr, t2);
      double d1[3] = {0, 0, 0}, d2[3] = {0, 0, 0};
      if (bw) for (int k = 0; k < 3; ++k) { d1[k] = bw[6 * b1 + k]; d2[k] = bw[6 * b2 + k]; }
      // mj_contactForce on the slot's rows: the normal force is the sum of the edge forces (padding rows carry none), component i of
      // the pair (f[2i], f[2i+1]) is their difference times the pair's friction coefficient
      const T fn = f0 + f1 + f2 + f3, fa = muA * (f0 - f1), fb = muB * (f2 - f3);
      // world force on body 2 at the contact point (- on body 1); slots whose pairs are rotations carry a world torque instead
      T Fw[3], Tq[3];
      for (int k = 0; k < 3; ++k) {
        Fw[k] = fr[k] * fn + (kind == 0 ? fr[3 + k] * fa + t2[k] * fb : (T)0);
        Tq[k] = kind == 1 ? fr[k] * fa + fr[3 + k] * fb : (kind == 2 ? t2[k] * fa : (kind == 4 ? fr[k] * fa : (T)0));
      }
      if (bw) {
        const T a1[3] = {(T)((double)r1[0] + d1[0]), (T)((double)r1[1] + d1[1]), (T)((double)r1[2] + d1[2])};
        const T a2[3] = {(T)((double)r2[0] + d2[0]), (T)((double)r2[1] + d2[1]), (T)((double)r2[2] + d2[2])};
        T m1[3], m2[3];
        cross3(m1, a1, Fw);
        cross3(m2, a2, Fw);
        for (int k = 0; k < 3; ++k) {
          lds_add(&acc[6 * b2 + k], Fw[k]); lds_add(&acc[6 * b2 + 3 + k], m2[k] + Tq[k]);
          lds_add(&acc[6 * b1 + k], -Fw[k]); lds_add(&acc[6 * b1 + 3 + k], -(m1[k] + Tq[k]));
        }
      }
      if (cd && LV(isfirst)) {
        // force[6] in the contact frame, MuJoCo's order: normal, tangent 1, tangent 2, torsional, rolling 1, rolling 2.  The lane of a
        // contact's first slot adds the later slots of the same contact (condim 4: kind 4; condim 6: kinds 1 and 2)
        T out[6] = {fn, fa, fb, 0, 0, 0};
        for (int j = 1; j < 3; ++j) {
          if (ci + j >= ncon) break;
          const auto& cj = CON(s, ci + j);
          const int kj = con_kind(cj);
          if (kj == 0 || kj == 3) break;
          const T* fj = s.efc_force + nlim + 4 * (ci + j);
          out[0] += fj[0] + fj[1] + fj[2] + fj[3];
          if (kj == 2) out[5] = cj.muA * (fj[0] - fj[1]);
          else { out[3] = cj.muA * (fj[0] - fj[1]); if (kj == 1) out[4] = cj.muB * (fj[2] - fj[3]); }
        }
        const int cidx = first[lane];
        for (int k = 0; k < 6; ++k) cd[MYO_SENSE_CON_N * cidx + 7 + k] = (double)out[k];
      }
    }
    if (lane == 0 && O.ncon) O.ncon[env] = nfirst;
  }
  SYNC();
  PHASE {
    if (bw) for (int i = lane; i < 6 * nb; i += 64) bw[i] = (double)acc[i];
  }
  SYNC();
  ws_release(K, s);
}

// the job of myo_batch_sense (jobs: csrc/myo_task.h); keyed without the integrator, a forward pass integrates nothing
struct SenseJob { static constexpr bool RK = false; SenseDev O; };
MYO_JOB_RUN(SenseJob) { env_sense(M, K, L, MYO_ENV_REC(block), s, block, J.O); }
