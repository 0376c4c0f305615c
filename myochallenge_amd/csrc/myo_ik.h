// myo_ik.h — per-env inverse kinematics (include/myobatch.h: myo_batch_ik).
//
// Which joint pose puts k sites on k world targets?  Per env the box-constrained, weighted nonlinear least-squares problem
//   minimise  f(q) = 1/2 sum_o w_o |site_xpos_o(q) - t_o|^2 + 1/2 reg sum_a (q_a - q_ref_a)^2     s.t.  lo_a <= q_a <= hi_a
// over the ACTIVE joints a (hinge and slide joints, or the subset the caller names; every other qpos entry stays at its start
// value).  One wave per env, a job of the env path's wrapper kernel beside env_jac / env_static_opt, seeded by load_env; it reads
// the env record and writes NOTHING back to it (no store_env).  float64 whatever the batch's dtype; lanes = dofs (a hinge or slide
// joint has one dof and one qpos entry: jnt_qposadr of the dof's joint).
//
// The method: projected Levenberg-Marquardt.  At the iterate q, with e the stacked residual, J [3k, nv] the sites' jacp (columns
// of inactive dofs 0), g = J'We + reg (q - q_ref) and H = J'WJ + reg I, the step d solves the box QP
//   min 1/2 d'(H + mu I) d + g'd     over  lo - q <= d <= hi - q
// by projected Newton — the scheme of csrc/myo_static_opt.h (mju_boxQP: clamped set from the gradient's sign, Cholesky with the
// clamped rows and columns replaced by identity, projected Armijo on the exact decrease, a working set and the ratio-test
// fallback), restated here in the variable d: static optimisation's loop is interleaved with its own problem's storage, and its
// outputs are pinned bit for bit, so it is left as it is and this file carries its own copy.  The trial q + d gets a fresh position
// pass; it is accepted when f(q) - f(q + d) >= MYO_IK_ACCEPT * -(g'd + 1/2 d'Hd).  mu follows the gain ratio (Nielsen's update): it
// shrinks by up to 3 after a step the model predicted well, and grows by 2, 4, 8, ... over consecutive rejections.
//
// The position pass is the stepper's own stage (kinematics, com_pos: the shared code, k_step's instantiations do not change) at
// the trial qpos written into the scratch; the site points and the Jacobian columns are env_data's / env_jac's expressions
// (data_body_pose, cdof, the ancestor-dof mask body_dofmask: no tree walk).
//
// Storage.  Between a position pass and the next solve nothing of the pass is live, and between a solve and the next pass nothing
// of the solve: both use the scratch from H on (the pass's small vectors inside H itself, which com_pos's cinert leaves free once
// cdof is built; the factor as static optimisation places it).  What survives both lives in lane variables (q, q_ref, the box, the
// gradient, the step: a dozen doubles) or in a library-grown global workspace of MYO_IK_WS_N doubles per env (myo_batch::ik_ws):
// H (packed lower triangle, built by lanes over (i, j) pairs in index order), J and the site points of the accepted iterate.  The
// lane's row of H + mu I is read into registers for the solve alone (MYO_NV_MAX doubles, dead across the position pass).  No
// atomics, no cross-lane intrinsics, sums in index order by loops every lane runs alike: the same bits on every run, and the
// lane-serial emulation runs the same source.  All stores are plain vector stores.
#pragma once

/* MYO_IK_K_MAX, targets per call (48 rows), is include/myobatch.h's */
#define MYO_IK_ROWS (3 * MYO_IK_K_MAX)
#define MYO_IK_NTRI (MYO_NV_MAX * (MYO_NV_MAX + 1) / 2)
#define MYO_IK_WS_H 0                                               /* workspace: H, packed lower triangle */
#define MYO_IK_WS_J ((MYO_IK_NTRI + 15) / 16 * 16)                  /* J [MYO_IK_ROWS][MYO_NV_MAX] */
#define MYO_IK_WS_X (MYO_IK_WS_J + MYO_IK_ROWS * MYO_NV_MAX)        /* site points of the accepted iterate [MYO_IK_ROWS] */
#define MYO_IK_WS_N ((MYO_IK_WS_X + MYO_IK_ROWS + 15) / 16 * 16)    /* doubles per env */
#define MYO_IK_LDS_N (MYO_IK_NTRI + 5 * MYO_NV_MAX)                 /* doubles of the scratch the solve uses, from Scratch::H on */
#define MYO_IK_PASS_N (6 * MYO_IK_K_MAX + 2 * MYO_IK_K_MAX + MYO_NV_MAX) /* doubles of Scratch::H the pass's vectors use */
#define MYO_IK_TRI(i) ((i) * ((i) + 1) / 2)
#define MYO_IK_HIDX(i, j) ((i) >= (j) ? MYO_IK_TRI(i) + (j) : MYO_IK_TRI(j) + (i))
// Levenberg-Marquardt: damping and acceptance (DESIGN.md §5.14 restates them)
#define MYO_IK_MU0 1e-3         /* mu starts at MYO_IK_MU0 * max diag(J'WJ) at the start point */
#define MYO_IK_MU_DOWN (1.0 / 3) /* accepted step with gain ratio rho = actual / predicted decrease: mu *= max(MYO_IK_MU_DOWN, 1 - (2 rho - 1)^3), nu = MYO_IK_MU_UP */
#define MYO_IK_MU_UP 2.0         /* rejected step: mu = max(mu * nu, MYO_IK_MU_FLOOR * (max diag(J'WJ) at the start + reg)), then nu *= 2 (Nielsen's update) */
#define MYO_IK_MU_FLOOR 1e-9
#define MYO_IK_MU_CAP 1e12      /* mu beyond MYO_IK_MU_CAP * (max diag(J'WJ) at the start + reg): MYO_IK_STALL */
#define MYO_IK_ACCEPT 1e-4      /* actual decrease >= MYO_IK_ACCEPT * predicted decrease */
// the box QP of a step
#define MYO_IK_QP_ITER 30       /* projected-Newton steps per QP at most */
#define MYO_IK_QP_TOL 1e-6      /* QP's projected gradient <= MYO_IK_QP_TOL * the outer projected gradient (floor: 1e-16 (1 + |g|)) */
#define MYO_IK_ARMIJO 0.1
#define MYO_IK_BACKTRACKS 6
enum { MYO_IK_ST_CAP = 1, MYO_IK_ST_STALL = 2, MYO_IK_ST_PINNED = 4 };      // == MYO_IK_* of include/myobatch.h (checked in myo_host.h)
static_assert(MYO_NV_MAX <= 64 && MYO_IK_K_MAX <= 64, "one lane per dof, one per target");

// what a call reads and where it publishes: caller-owned device arrays of include/myobatch.h's structs (outputs: any may be null)
struct IkDev {
  const int* site_ids;                                       // [k]
  const double *targets, *weight, *q_init, *q_ref, *lower, *upper;      // [N, k, 3]; [k] or [N, k] or null; [N, nq] or null (twice); [N, nv] or null (twice)
  double *qpos, *site_xpos, *residual, *cost, *kkt;
  int *iters, *status;
  double* ws;                                                // [N, MYO_IK_WS_N]
  unsigned long long active;                                 // dof mask; 0: every hinge / slide dof
  double reg, tol;
  int k, weight_per_env, max_iter;
};

template <typename T, int NC>
DEV void env_ik(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s, int env, const IkDev& O) {
  WAVE_FN_K
  const int nv = M.nv, nq = M.nq, ns = M.nsite, k = O.k;
  const size_t e = (size_t)env;
  load_env(M, K, L, rec, s, env);
  typedef Scratch<T, NC> S;
  static_assert(offsetof(S, rk) - offsetof(S, H) >= MYO_IK_LDS_N * sizeof(double) && offsetof(S, H) % 8 == 0, "the factor and the shared vectors fit between H and rk");
  static_assert(sizeof(T) * MYO_H_SIZE >= MYO_IK_PASS_N * sizeof(double), "the pass's vectors fit in H");
  // the solve's storage (from H on; dead during a position pass)
  double* const Lf = reinterpret_cast<double*>(s.H);      // packed lower triangle: H + mu I with the clamped rows / columns replaced, then its factor below the diagonal
  double* const Ld = Lf + MYO_IK_NTRI;                    // reciprocals of the factor's diagonal
  double* const xa = Ld + MYO_NV_MAX;                     // shared dof-indexed vectors
  double* const xb = xa + MYO_NV_MAX;
  double* const xd = xb + MYO_NV_MAX;
  double* const wd = xd + MYO_NV_MAX;
  // the pass's storage (inside H: cinert is dead once com_pos has built cdof; dead during a solve)
  double* const pt = reinterpret_cast<double*>(s.H);      // [k][3] site point minus its tree's reference point
  double* const px = pt + 3 * MYO_IK_K_MAX;               // [k][3] site point, world
  double* const bd = px + 3 * MYO_IK_K_MAX;               // [k] the site's body (-1: an id outside the model)
  double* const cw = bd + MYO_IK_K_MAX;                   // [k] w_o |p - t|^2, then w_o
  double* const dv = cw + MYO_IK_K_MAX;                   // [nv] dof-indexed terms of a sum
  GPTR(double) Hg = (GPTR(double))O.ws + e * MYO_IK_WS_N + MYO_IK_WS_H;
  GPTR(double) Jg = (GPTR(double))O.ws + e * MYO_IK_WS_N + MYO_IK_WS_J;
  GPTR(double) Xg = (GPTR(double))O.ws + e * MYO_IK_WS_N + MYO_IK_WS_X;
  GPTR(const int) ids = (GPTR(const int))O.site_ids;
  const double reg = O.reg;
  const int goal_b = (K.kind == MYO_TASK_REORIENT_K && K.target1_sid >= 0) ? M.site_bodyid[K.target1_sid] : -1;
  const int baoding = (K.kind == 1 || K.kind == 2) && K.target1_sid >= 0 && K.target2_sid >= 0;
  // the active dofs: hinge (3) and slide (2) joints, of the caller's mask if there is one (uniform: every lane runs the loop)
  unsigned long long amask = 0;
  for (int j = 0; j < nv; ++j) { const int ty = M.jnt_type[M.dof_jntid[j]]; if (ty == 2 || ty == 3) amask |= 1ull << j; }
  if (O.active) amask &= O.active;
  // target o's component c and weight, read where they are used (lanes = targets; not held in registers across the passes)
#define IK_TG(o, c) O.targets[(e * k + (o)) * 3 + (c)]
#define IK_W(o) (O.weight ? tmax(O.weight[(O.weight_per_env ? e * k : (size_t)0) + (o)], 0.0) : 1.0)
  // ---- lanes = dofs: the box, the start point projected into it, the regularisation centre
  LANE_VAR(double, q); LANE_VAR(double, qt); LANE_VAR(double, qref); LANE_VAR(double, lo); LANE_VAR(double, hi); LANE_VAR(double, gr);
  LANE_VAR(int, qa); LANE_VAR(int, on); LANE_VAR(int, pinflag);
  if (O.q_init) {      // the caller's start point, frozen entries included
    PHASE { for (int i = lane; i < nq; i += 64) s.qpos[i] = O.q_init[e * nq + i]; }
    SYNC();
  }
  PHASE {
    const int i = lane;
    LV(on) = 0; LV(pinflag) = 0; LV(qa) = 0; LV(q) = LV(qt) = LV(qref) = LV(lo) = LV(hi) = LV(gr) = 0;
    if (i < nv && ((amask >> i) & 1ull)) {
      const int j = M.dof_jntid[i], a = M.jnt_qposadr[j];
      double l = M.jnt_limited[j] ? (double)M.h_jnt_range[2 * j] : -(double)INFINITY;
      double h = M.jnt_limited[j] ? (double)M.h_jnt_range[2 * j + 1] : (double)INFINITY;
      if (O.lower) l = O.lower[e * nv + i];
      if (O.upper) h = O.upper[e * nv + i];
      if (l > h) { LV(pinflag) = 1; h = l; }      // pinned at lower, and the status says so
      const double q0 = s.qpos[a];
      LV(on) = 1; LV(qa) = a; LV(lo) = l; LV(hi) = h;
      LV(qref) = O.q_ref ? O.q_ref[e * nq + a] : q0;
      LV(q) = LV(qt) = tclamp(q0, l, h);
    }
    if (i < MYO_NV_MAX) xb[i] = (double)LV(pinflag);
  }
  SYNC();
  int pinned = 0;
  for (int j = 0; j < nv; ++j) pinned |= xb[j] != 0.0;
  SYNC();
  // ---- projected Levenberg-Marquardt
  int it = 0, status = 0, first = 1;
  double f = 0, pg = 0, pred = 0, mu = 0, nu = MYO_IK_MU_UP, scale0 = 0, tol_abs = 0;
  LANE_VAR(double, Hrow)[MYO_NV_MAX];      // the lane's row of H + mu I (full, symmetric) during a solve, entries beyond nv are 0
  LANE_VAR(double, d); LANE_VAR(double, dlo); LANE_VAR(double, dhi); LANE_VAR(double, gq); LANE_VAR(double, dir); LANE_VAR(double, uc);
  LANE_VAR(double, dl); LANE_VAR(double, ratio);
  for (;;) {
    // -- the position pass at the trial point qt, the site points, the cost
    PHASE { if (LV(on)) s.qpos[LV(qa)] = LV(qt); }
    SYNC();
    kinematics(M, s);
    com_pos(M, K, s);
    PHASE {
      const int o = lane;
      if (o < k) {
        const int id = ids[o];
        int body = -1;
        HP p[3] = {0, 0, 0};
        if (id >= 0 && id < ns) {      // (env_data's / env_jac's site point)
          body = M.site_bodyid[id];
          HP xp[3], qq[4], B[9], l[3];
          data_body_pose(s, body, goal_b, xp, qq);
          quat2mat(B, qq);
          for (int c = 0; c < 3; ++c) l[c] = M.h_site_pos[3 * id + c];
          if (baoding && id == K.target1_sid) { l[0] = s.target_xy[0]; l[1] = s.target_xy[1]; }
          if (baoding && id == K.target2_sid) { l[0] = s.target_xy[2]; l[1] = s.target_xy[3]; }
          mulmatvec3(p, B, l);
          for (int c = 0; c < 3; ++c) p[c] += xp[c];
        }
        const int root = body >= 0 ? M.body_rootid[body] : 0;
        double c2 = 0;
        for (int c = 0; c < 3; ++c) {
          pt[3 * o + c] = p[c] - ((HP)S_COM(s)[3 * root + c] + S_ORIGIN(s)[c]);
          px[3 * o + c] = (double)p[c];
          const double r = body >= 0 ? (double)p[c] - IK_TG(o, c) : 0.0;
          c2 += r * r;
        }
        bd[o] = (double)body;
        cw[o] = IK_W(o) * c2;
      }
      if (lane < nv) { const double r = LV(on) ? LV(qt) - LV(qref) : 0.0; dv[lane] = r * r; }
    }
    SYNC();
    double ft = 0, fr = 0;
    for (int o = 0; o < k; ++o) ft += cw[o];
    for (int j = 0; j < nv; ++j) fr += dv[j];
    ft = 0.5 * ft + 0.5 * reg * fr;
    const int accept = first || (pred > 0 && f - ft >= MYO_IK_ACCEPT * pred);
    if (accept) {
      const double rho = first ? 1.0 : (f - ft) / pred;
      f = ft;
      // -- the accepted iterate: its site points and Jacobian to the workspace, lanes = (site, dof)
      PHASE {
        LV(q) = LV(qt);
        if (lane < 3 * k) Xg[lane] = bd[lane / 3] >= 0 ? px[lane] : 0.0;
        for (int idx = lane; idx < k * nv; idx += 64) {
          const int o = idx / nv, i = idx - o * nv;
          const int body = (int)bd[o];
          const bool col = body >= 0 && ((M.body_dofmask[body >= 0 ? body : 0] >> i) & 1ull) && ((amask >> i) & 1ull);
          const double a[3] = {(double)s.cdof[6 * i], (double)s.cdof[6 * i + 1], (double)s.cdof[6 * i + 2]};
          const double l[3] = {(double)s.cdof[6 * i + 3], (double)s.cdof[6 * i + 4], (double)s.cdof[6 * i + 5]};
          const double r[3] = {pt[3 * o], pt[3 * o + 1], pt[3 * o + 2]};
          double t[3];
          cross3(t, a, r);
          for (int c = 0; c < 3; ++c) Jg[(size_t)(3 * o + c) * MYO_NV_MAX + i] = col ? l[c] + t[c] : 0.0;
        }
      }
      SYNC();
      // the weighted residual rows W e into pt (the offsets are consumed), the weights into cw
      PHASE {
        const int o = lane;
        if (o < k) {
          const bool valid = bd[o] >= 0;
          for (int c = 0; c < 3; ++c) pt[3 * o + c] = valid ? IK_W(o) * (px[3 * o + c] - IK_TG(o, c)) : 0.0;
          cw[o] = valid ? IK_W(o) : 0.0;
        }
      }
      SYNC_G();      // (other lanes read J's entries below)
      // g = J'We + reg (q - q_ref), lanes = dofs, rows in index order
      PHASE {
        const int i = lane;
        if (i < nv) {
          double acc = 0;
          for (int r = 0; r < 3 * k; ++r) acc += Jg[(size_t)r * MYO_NV_MAX + i] * pt[r];
          dv[i] = fabs(acc);
          LV(gr) = LV(on) ? acc + reg * (LV(q) - LV(qref)) : 0.0;
        }
      }
      // H = J'WJ + reg I into the workspace, lanes = (i, j) pairs, rows in index order
      PHASE {
        for (int idx = lane; idx < nv * nv; idx += 64) {
          const int i = idx / nv, j = idx - i * nv;
          if (j <= i) {
            double acc = 0;
            for (int r = 0; r < 3 * k; ++r) acc += cw[r / 3] * Jg[(size_t)r * MYO_NV_MAX + i] * Jg[(size_t)r * MYO_NV_MAX + j];
            Hg[MYO_IK_TRI(i) + j] = i == j ? acc + reg : acc;
          }
        }
      }
      SYNC_G();      // (the solve's lanes read H's rows)
      if (first) {
        double amax = 0;
        for (int j = 0; j < nv; ++j) amax = tmax(amax, dv[j]);
        tol_abs = O.tol * (1 + amax);
        SYNC();
        PHASE { if (lane < nv) dv[lane] = Hg[MYO_IK_TRI(lane) + lane] - reg; }
        SYNC();
        for (int j = 0; j < nv; ++j) scale0 = tmax(scale0, dv[j]);
        mu = MYO_IK_MU0 * scale0;
      } else { const double t3 = 2 * rho - 1; mu *= tmax(MYO_IK_MU_DOWN, 1 - t3 * t3 * t3); nu = MYO_IK_MU_UP; }
      // the projected gradient's max-norm
      SYNC();
      PHASE {
        const int i = lane;
        if (i < nv) {
          const bool pinned_i = !LV(on) || LV(lo) >= LV(hi), at_lo = LV(q) <= LV(lo), at_hi = LV(q) >= LV(hi);
          dv[i] = pinned_i ? 0.0 : (at_lo ? tmax(-LV(gr), 0.0) : (at_hi ? tmax(LV(gr), 0.0) : fabs(LV(gr))));
        }
      }
      SYNC();
      pg = 0;
      for (int j = 0; j < nv; ++j) pg = tmax(pg, dv[j]);
      SYNC();
      first = 0;
      if (pg <= tol_abs) break;
    } else {
      mu = tmax(mu * nu, MYO_IK_MU_FLOOR * (scale0 + reg));
      nu *= 2;
      if (!(mu <= MYO_IK_MU_CAP * (scale0 + reg))) { status |= MYO_IK_ST_STALL; break; }
    }
    if (it >= O.max_iter) { status |= MYO_IK_ST_CAP; break; }
    ++it;
    // -- the step: min 1/2 d'(H + mu I) d + g'd over the box around q, projected Newton from d = 0
    PHASE {
      const int i = lane;
      if (i < nv) {
#pragma unroll
        for (int j = 0; j < MYO_NV_MAX; ++j) LV(Hrow)[j] = j < nv ? Hg[MYO_IK_HIDX(i, j)] + (j == i ? mu : 0.0) : 0.0;
      }
      LV(d) = 0; LV(dlo) = LV(lo) - LV(q); LV(dhi) = LV(hi) - LV(q);
      if (i < MYO_NV_MAX) xa[i] = xb[i] = xd[i] = wd[i] = Ld[i] = 0;
    }
    SYNC();
    {
      const double tolq = tmax(MYO_IK_QP_TOL * pg, 1e-16 * (1 + pg));
      int qit = 0, have_factor = 0;
      unsigned long long W = 0, fmask = 0;
      for (;;) {
        PHASE { if (lane < nv) xa[lane] = LV(d); }
        SYNC();
        PHASE {
          const int i = lane;
          if (i < nv) {
            double acc = LV(gr);
#pragma unroll
            for (int j = 0; j < MYO_NV_MAX; ++j) acc += LV(Hrow)[j] * xa[j];
            LV(gq) = acc;
            const bool pinned_i = !LV(on) || LV(dlo) >= LV(dhi), at_lo = LV(d) <= LV(dlo), at_hi = LV(d) >= LV(dhi);
            xb[i] = pinned_i ? 0.0 : (at_lo ? tmax(-acc, 0.0) : (at_hi ? tmax(acc, 0.0) : fabs(acc)));      // the projected gradient
            xd[i] = (pinned_i || (at_lo && acc > -tolq) || (at_hi && acc < tolq)) ? 1.0 : 0.0;               // the sign rule keeps it clamped
            wd[i] = fabs(acc);
          }
        }
        SYNC();
        unsigned long long keep = 0;
        double qpg = 0;
        for (int j = 0; j < nv; ++j) { qpg = tmax(qpg, xb[j]); if (xd[j] != 0.0) keep |= 1ull << j; }
        if (qit == 0) W = keep;
        if (qpg < tolq || qit >= MYO_IK_QP_ITER) break;
        double gfree = 0;
        for (int j = 0; j < nv; ++j) if (!((W >> j) & 1ull)) gfree = tmax(gfree, wd[j]);
        if (gfree < tolq) W &= keep;      // the minimiser on W's face: release
        if (!have_factor || W != fmask) {
          PHASE {
            const int i = lane;
            if (i < nv) {
#pragma unroll
              for (int j = 0; j < MYO_NV_MAX; ++j)
                if (j <= i) Lf[MYO_IK_TRI(i) + j] = (((W >> i) | (W >> j)) & 1ull) ? (i == j ? 1.0 : 0.0) : LV(Hrow)[j];
            }
          }
          SYNC();
          for (int j = 0; j < nv; ++j) {
            PHASE {
              const int i = lane;
              if (i >= j && i < nv) {
                double sjj = Lf[MYO_IK_TRI(j) + j], sij = Lf[MYO_IK_TRI(i) + j];
                for (int c = 0; c < j; ++c) { const double ljk = Lf[MYO_IK_TRI(j) + c]; sjj -= ljk * ljk; sij -= Lf[MYO_IK_TRI(i) + c] * ljk; }
                const double ip = 1.0 / sqrt(tmax(sjj, 1e-300));
                if (i == j) Ld[j] = ip; else Lf[MYO_IK_TRI(i) + j] = sij * ip;
              }
            }
            SYNC();
          }
          have_factor = 1; fmask = W;
        }
        // the Newton direction on the free set: L L' dir = -gradient (0 on the clamped set)
        PHASE { if (lane < nv) xa[lane] = ((W >> lane) & 1ull) ? 0.0 : -LV(gq); }
        SYNC();
        for (int j = 0; j < nv - 1; ++j) {
          PHASE { const int i = lane; if (i > j && i < nv) xa[i] -= Lf[MYO_IK_TRI(i) + j] * (xa[j] * Ld[j]); }
          SYNC();
        }
        PHASE { if (lane < nv) xa[lane] *= Ld[lane]; }
        SYNC();
        for (int j = nv - 1; j > 0; --j) {
          PHASE { const int i = lane; if (i < j) xa[i] -= Lf[MYO_IK_TRI(j) + i] * (xa[j] * Ld[j]); }
          SYNC();
        }
        // ... and how far each variable can go along it (the ratio test)
        PHASE {
          const int i = lane;
          if (i < nv) {
            const double dd = ((W >> i) & 1ull) ? 0.0 : xa[i] * Ld[i];
            LV(dir) = dd;
            LV(ratio) = dd < 0 ? (LV(dlo) - LV(d)) / dd : (dd > 0 ? (LV(dhi) - LV(d)) / dd : (double)INFINITY);
            xb[i] = LV(ratio);
          }
        }
        SYNC();
        double a1 = (double)INFINITY;
        for (int j = 0; j < nv; ++j) a1 = tmin(a1, xb[j]);
        // projected Armijo backtracking over the steps that bend (alpha > a1) on the exact decrease g'dl + 1/2 dl'H dl
        double alpha = 1;
        int accepted = 0;
        for (int ls = 0; ls < MYO_IK_BACKTRACKS && alpha > a1 && !accepted; ++ls) {
          PHASE {
            if (lane < nv) {
              LV(uc) = LV(ratio) <= alpha ? (LV(dir) < 0 ? LV(dlo) : LV(dhi)) : tclamp(LV(d) + alpha * LV(dir), LV(dlo), LV(dhi));
              LV(dl) = LV(uc) - LV(d);
              xa[lane] = LV(dl);
            }
          }
          SYNC();
          PHASE {
            const int i = lane;
            if (i < nv) {
              double hd = 0;
#pragma unroll
              for (int j = 0; j < MYO_NV_MAX; ++j) hd += LV(Hrow)[j] * xa[j];
              xb[i] = LV(dl) * (LV(gq) + 0.5 * hd);
              xd[i] = LV(dl) * LV(gq);
            }
          }
          SYNC();
          double dcost = 0, slope = 0;
          for (int j = 0; j < nv; ++j) { dcost += xb[j]; slope += xd[j]; }
          if (dcost <= MYO_IK_ARMIJO * slope) accepted = 1; else alpha *= 0.5;
        }
        if (!accepted) alpha = tmin(1.0, a1);
        PHASE {
          if (lane < nv) {
            const bool hit = LV(ratio) <= alpha;
            LV(d) = hit ? (LV(dir) < 0 ? LV(dlo) : LV(dhi)) : tclamp(LV(d) + alpha * LV(dir), LV(dlo), LV(dhi));
            xb[lane] = hit ? 1.0 : 0.0;
          }
        }
        SYNC();
        for (int j = 0; j < nv; ++j) if (xb[j] != 0.0) W |= 1ull << j;
        ++qit;
      }
    }
    // the trial point (exactly on a bound where the step is) and the decrease the model without mu predicts: -(g'd + 1/2 d'Hd)
    PHASE { if (lane < nv) xa[lane] = LV(d); }
    SYNC();
    PHASE {
      const int i = lane;
      if (i < nv) {
        double hd = 0;
#pragma unroll
        for (int j = 0; j < MYO_NV_MAX; ++j) hd += LV(Hrow)[j] * xa[j];
        hd -= mu * LV(d);
        xb[i] = LV(d) * (LV(gr) + 0.5 * hd);
        if (LV(on)) LV(qt) = LV(d) <= LV(dlo) ? LV(lo) : (LV(d) >= LV(dhi) ? LV(hi) : tclamp(LV(q) + LV(d), LV(lo), LV(hi)));
        if (LV(d) == 0.0) LV(qt) = LV(q);
      }
    }
    SYNC();
    pred = 0;
    for (int j = 0; j < nv; ++j) pred += xb[j];
    pred = -pred;
    SYNC();
  }
  // ---- publish: q of the last accepted iterate (frozen entries from the start point, bit for bit), its site points and residuals
  // (the solve's storage is free: the active entries' values and a flag per qpos entry go through it, one store per entry)
  PHASE { for (int i = lane; i < nq; i += 64) Lf[64 + i] = 0.0; }
  SYNC();
  PHASE { if (LV(on)) { Lf[LV(qa)] = LV(q); Lf[64 + LV(qa)] = 1.0; } }
  SYNC();
  PHASE {
    if (O.qpos)
      for (int i = lane; i < nq; i += 64) O.qpos[e * nq + i] = Lf[64 + i] != 0.0 ? Lf[i] : (O.q_init ? O.q_init[e * nq + i] : rec[L.off_qpos + i]);
    const int o = lane;
    if (o < k) {
      const int id = ids[o];
      const bool valid = id >= 0 && id < ns;
      for (int c = 0; c < 3; ++c) {
        const double x = Xg[3 * o + c];
        if (O.site_xpos) O.site_xpos[(e * k + o) * 3 + c] = x;
        if (O.residual) O.residual[(e * k + o) * 3 + c] = valid ? x - IK_TG(o, c) : 0.0;
      }
    }
    if (lane == 0) {
      if (O.cost) O.cost[e] = f;
      if (O.kkt) O.kkt[e] = pg;
      if (O.iters) O.iters[e] = it;
      if (O.status) O.status[e] = status | (pinned ? MYO_IK_ST_PINNED : 0);
    }
  }
  SYNC();
  ws_release(K, s);
#undef IK_TG
#undef IK_W
}

// the job of myo_batch_ik (jobs: csrc/myo_task.h); keyed without the integrator, the pass integrates nothing
struct IkJob { static constexpr bool RK = false; IkDev O; };
MYO_JOB_RUN(IkJob) { env_ik(M, K, L, MYO_ENV_REC(block), s, block, J.O); }
