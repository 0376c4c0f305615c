// myo_static_opt.h — per-env static optimisation (include/myobatch.h: myo_batch_static_opt).
//
// Which actuator inputs deliver a given generalised force at the env's PRESENT state?  The actuation stage (P9, fwd_actuation) is
// affine in the input — force_i = gain_i(len, vel) u_i + bias_i(len), u = a muscle's activation or the ctrl of an actuator without an
// activation state — so with R = actuator_moment [nu, nv] the question is the box-constrained least-squares problem
//   minimise  1/2 sum_d w_d (sum_i R[i,d] (g_i u_i + b_i) - qfrc_d)^2 + 1/2 reg sum_i (u_i - u_ref_i)^2     s.t.  lo_i <= u_i <= hi_i
// per env: strictly convex (reg > 0), nu <= 40 unknowns.  One wave per env, a job of the env path's wrapper kernel beside env_data /
// env_jac / env_inverse, seeded by load_env; it reads the env record and writes NOTHING back to it (no store_env).
//
// The pass.  Position, inertia and velocity stages exactly as env_data runs them (the shared code; k_step's instantiations do not
// change) — the gain needs tendon length and velocity.  Then, lanes = actuators:
//   gain, bias   P9's two curves restated (same constants, same types, same order of operations as fwd_actuation; tests pin
//                gain * activation + bias against sensors()'s actuator_force)
//   the box      the caller's or the default bounds, tightened to the interval on which a force limit is inactive (exact: the force is
//                affine and monotone in u).  A variable with an empty interval, with lo > hi or with gain 0 is PINNED: it enters the
//                problem with gain 0 and its (clamped) force as bias, lo = hi = its value, so nothing below treats it specially
//   H, q         H = A'A + reg I, A = sqrt(W) R' diag(g): every actuator reaches <= MYO_TJ_MAX dofs, entry (i, j) sums over the dofs
//                both reach (bit masks, slot = popcount below the bit); q = A' sqrt(W) c - reg u_ref, c = R' b - qfrc.
//                cost(u) = 1/2 u'Hu + q'u + const, gradient H u + q
//   the solve    projected Newton, the scheme of MuJoCo's mju_boxQP (Tassa, Mansard, Todorov 2014): clamped set from the sign of the
//                gradient at the bounds; Cholesky of H with clamped rows and columns replaced by identity (fixed size, no gather);
//                Newton step on the free set; projected Armijo backtracking on the EXACT decrease g'd + 1/2 d'Hd (no difference of
//                two costs); until the projected gradient's max-norm is below 1e-12 (1 + max|A'c|) — the clamped set is then the
//                sign rule's and stays — or max_iter.  The clamped set is kept as a WORKING set and a rejected line search ends in
//                a ratio-test step: see the comment at the loop
// Everything a lane needs from another lane goes through LDS and is read back either by lanes or by a plain loop that every lane runs
// alike (sums, maxima and the clamped-set mask are wave-uniform by construction and summed in index order): no atomics, no cross-lane
// intrinsics, the same bits on every run, and the lane-serial emulation runs the same source.
//
// Storage.  The factor (820 packed doubles), its diagonal and four shared vectors live in the scratch from H on — after the velocity
// stage and the lane-private reads above, nothing from there on is live (static_assert below); no variant's LDS grows.  H is built
// by lanes over (i, j) pairs into a library-grown global workspace, 820 packed doubles per env (myo_batch::so_ws), and read back ONCE:
// lane i keeps row i in registers (40 doubles, every loop over them unrolled) — the products H x of the gradient and the line
// search and the copy into the factor's storage then touch no global memory (a first cut read H from the workspace in every
// product: 6.8 ms for 4096 hand envs, one dependent global load per term).  All stores are plain vector stores.
#pragma once

#define MYO_SO_NTRI (MYO_NU_MAX * (MYO_NU_MAX + 1) / 2)       /* packed lower triangle of H / of its factor */
#define MYO_SO_WS_N ((MYO_SO_NTRI + 15) / 16 * 16)            /* doubles per env of the global workspace */
#define MYO_SO_LDS_N (MYO_SO_NTRI + 5 * MYO_NU_MAX)           /* doubles of the scratch the solve uses, from Scratch::H on */
#define MYO_SO_ARMIJO 0.1
#define MYO_SO_BACKTRACKS 6
#define MYO_SO_TRI(i) ((i) * ((i) + 1) / 2)
#define MYO_SO_HIDX(i, j) ((i) >= (j) ? MYO_SO_TRI(i) + (j) : MYO_SO_TRI(j) + (i))
enum { MYO_SO_ST_CAP = 1, MYO_SO_ST_PINNED = 4 };            // == MYO_STATIC_OPT_* of include/myobatch.h (checked in myo_host.h)
static_assert(MYO_NU_MAX <= 64 && MYO_NV_MAX <= MYO_NU_MAX, "one lane per actuator, one per dof; the dof-indexed shared vectors have MYO_NU_MAX entries");

// what a call reads and where it publishes: caller-owned device arrays of include/myobatch.h's structs (outputs: any may be null)
struct StaticOptDev {
  const double *qfrc, *weight, *u_ref, *lower, *upper;      // [N, nv]; [nv] or [N, nv] or null; [N, nu] or null (three times)
  double *u, *force, *qfrc_out, *residual, *gain, *bias, *kkt;
  int *iters, *status;
  double* ws;                                               // [N, MYO_SO_WS_N]: H of every env (null when nothing asks for a solve)
  unsigned long long reach;                                 // dofs some actuator's moment row can reach: the default weight
  double reg;
  int weight_per_env, max_iter, solve;
};

template <typename T, int NC>
DEV void env_static_opt(const DevModel<T>& M, const TaskDev& K, const EnvRecordLayout& L, double* rec, Scratch<T, NC>& s, int env, const StaticOptDev& O) {
  WAVE_FN_K
  const int nv = M.nv, nu = M.nu;
  const size_t e = (size_t)env;
  load_env(M, K, L, rec, s, env);
  // ---- position, inertia and velocity stages: forward()'s sequence, as env_data runs it for a call that ends before the actuation
  kinematics(M, s);
  com_pos(M, K, s);
  tendon(M, K, s);
  for (int base = 0; base < M.ngw; base += 64) tendon_wrap_pass(M, K, s, base);
  for (int base = 0; base < M.nte; base += 64) tendon_element_pass(M, K, s, base);
  tendon_length_sums(M, s);
  crb(M, s);
  body_vectors(M, s, LOFF(s, S_QVELT(s)), LOFF(s, S_CVEL(s)));
  fwd_velocity(M, K, s);
  // ---- lanes = actuators: everything a lane takes from the stages, into lane variables (the solve's storage overlaps the stages')
  LANE_VAR(double, g); LANE_VAR(double, b); LANE_VAR(double, ge); LANE_VAR(double, be); LANE_VAR(double, lo); LANE_VAR(double, hi);
  LANE_VAR(double, uref); LANE_VAR(double, fr0); LANE_VAR(double, fr1); LANE_VAR(double, q); LANE_VAR(double, u); LANE_VAR(double, gr);
  LANE_VAR(double, dir); LANE_VAR(double, uc); LANE_VAR(double, dl);
  LANE_VAR(double, Rk)[MYO_TJ_MAX];
  LANE_VAR(double, Hrow)[MYO_NU_MAX];      // the lane's row of H (full, symmetric), entries beyond nu are 0
  LANE_VAR(unsigned long long, dmask);
  LANE_VAR(int, flim); LANE_VAR(int, pinflag);
  PHASE {
    const int i = lane;
    if (i < nu) {
      // P9 restated: mju_muscleGain / mju_muscleBias from the host-resolved constants (act_pre), lengths in HP, the velocity factor in T
      const int dyntype = M.actuator_dyntype[i], tid = M.actuator_tendon[i], gaintype = M.actuator_gaintype[i], biastype = M.actuator_biastype[i];
      const T gear = M.actuator_gear[6 * i];
      HP ap[MYO_ACT_PRE];
      for (int k = 0; k < MYO_ACT_PRE; ++k) ap[k] = M.h_act_pre[MYO_ACT_PRE * i + k];
      const HP ten_len = S_TEN_LENGTH(s)[tid];
      const T ten_vel = S_TEN_VEL(s)[tid];
      const HP lenh = (HP)gear * ten_len;
      const T len = (T)lenh, vel = gear * ten_vel;
      T gain, bias = 0;
      if (gaintype == 1) {
        const HP Ln = ap[1] + (lenh - ap[3]) * ap[2];
        const T V = vel * (T)ap[4];
        const HP lmin = ap[5], lmax = ap[6], a = ap[7], bm = ap[8];
        HP FLh;
        if (Ln < lmin || Ln > lmax) FLh = 0;
        else if (Ln <= a) { const HP x = (Ln - lmin) * ap[9]; FLh = (HP)0.5 * x * x; }
        else if (Ln <= 1) { const HP x = (1 - Ln) * ap[10]; FLh = 1 - (HP)0.5 * x * x; }
        else if (Ln <= bm) { const HP x = (Ln - 1) * ap[11]; FLh = 1 - (HP)0.5 * x * x; }
        else { const HP x = (lmax - Ln) * ap[12]; FLh = (HP)0.5 * x * x; }
        const T FL = (T)FLh, y = (T)ap[13], fvmax = (T)ap[15];
        T FV;
        if (V <= -1) FV = 0;
        else if (V <= 0) FV = (V + 1) * (V + 1);
        else if (V <= y) FV = fvmax - (y - V) * (y - V) * (T)ap[14];
        else FV = fvmax;
        gain = -(T)ap[0] * FL * FV;
      } else gain = M.actuator_gainprm[10 * i];
      if (biastype == 2) {
        const HP Ln = ap[17] + (lenh - ap[3]) * ap[18];
        const HP bm = ap[19];
        const T force = (T)ap[16], fpmax = (T)ap[21];
        if (Ln <= 1) bias = 0;
        else if (Ln <= bm) { const T x = (T)((Ln - 1) * ap[20]); bias = -force * fpmax * (T)0.5 * x * x; }
        else { const T x = (T)((Ln - bm) * ap[20]); bias = -force * fpmax * ((T)0.5 + x); }
      } else if (biastype == 1) {
        bias = M.actuator_biasprm[10 * i] + M.actuator_biasprm[10 * i + 1] * len + M.actuator_biasprm[10 * i + 2] * vel;
      }
      LV(g) = (double)gain; LV(b) = (double)bias;
      LV(flim) = M.actuator_forcelimited[i];
      LV(fr0) = (double)M.actuator_forcerange[2 * i]; LV(fr1) = (double)M.actuator_forcerange[2 * i + 1];
      // the moment row (mj_transmission: gear times the tendon's row, as env_data publishes it) and the dofs it reaches
      LV(dmask) = M.act_dofmask[i];
      for (int k = 0; k < MYO_TJ_MAX; ++k) LV(Rk)[k] = M.act_sd[i * MYO_TJ_MAX + k] >= 0 ? (double)(gear * tenj_get(s, tid, k)) : 0.0;
      // the box: the caller's, or [0, 1] for a muscle's activation, ctrlrange for a limited ctrl, unbounded otherwise
      double l = dyntype == 3 ? 0.0 : (M.actuator_ctrllimited[i] ? (double)M.actuator_ctrlrange[2 * i] : -(double)INFINITY);
      double h = dyntype == 3 ? 1.0 : (M.actuator_ctrllimited[i] ? (double)M.actuator_ctrlrange[2 * i + 1] : (double)INFINITY);
      if (O.lower) l = O.lower[e * nu + i];
      if (O.upper) h = O.upper[e * nu + i];
      const double r = O.u_ref ? O.u_ref[e * nu + i] : 0.0;
      const double gd = (double)gain, bd = (double)bias;
      bool pin = false, flag = false;
      double pv = 0;
      if (l > h) { pin = flag = true; pv = l; }
      else if (gd == 0) { pin = true; pv = tclamp(r, l, h); }
      else if (LV(flim)) {      // the interval of u on which fr0 <= g u + b <= fr1
        double a = (LV(fr0) - bd) / gd, c = (LV(fr1) - bd) / gd;
        if (a > c) { const double t = a; a = c; c = t; }
        const double nl = tmax(l, a), nh = tmin(h, c);
        if (nl > nh) { pin = flag = true; pv = a > h ? h : l; }      // empty: the nearer end of the caller's box
        else { l = nl; h = nh; }
      }
      if (pin) {
        double f = gd * pv + bd;
        if (LV(flim)) f = tclamp(f, LV(fr0), LV(fr1));
        LV(ge) = 0; LV(be) = f; l = h = pv;
      } else { LV(ge) = gd; LV(be) = bd; }
      LV(lo) = l; LV(hi) = h; LV(uref) = r; LV(pinflag) = flag ? 1 : 0;
      if (O.gain) O.gain[e * nu + i] = gd;
      if (O.bias) O.bias[e * nu + i] = bd;
    }
  }
  SYNC();
  if (!O.solve) { ws_release(K, s); return; }
  // ---- the solve's storage: from H on, nothing of the scratch is live any more
  typedef Scratch<T, NC> S;
  static_assert(offsetof(S, rk) - offsetof(S, H) >= MYO_SO_LDS_N * sizeof(double) && offsetof(S, H) % 8 == 0, "the factor and the shared vectors fit between H and rk");
  static_assert(MYO_NU_MAX * MYO_TJ_MAX <= MYO_SO_NTRI, "the moment rows are staged where the factor goes");
  double* const Lf = reinterpret_cast<double*>(s.H);      // packed lower triangle: H with the clamped rows / columns replaced, then its factor below the diagonal
  double* const Ld = Lf + MYO_SO_NTRI;                    // reciprocals of the factor's diagonal (the triangle keeps H's)
  double* const xa = Ld + MYO_NU_MAX;                     // shared vectors, actuator- or dof-indexed
  double* const xb = xa + MYO_NU_MAX;
  double* const xd = xb + MYO_NU_MAX;
  double* const wd = xd + MYO_NU_MAX;
  double* const Rs = Lf;                                  // [nu][MYO_TJ_MAX] moment rows (times the gain), before the first factor and after the last
  GPTR(double) Hg = (GPTR(double))O.ws + e * MYO_SO_WS_N;
  const double reg = O.reg;
  PHASE {
    const int i = lane;
    if (i < nu) {
      for (int k = 0; k < MYO_TJ_MAX; ++k) Rs[i * MYO_TJ_MAX + k] = LV(Rk)[k];
      xa[i] = LV(be);
      xb[i] = (double)LV(pinflag);
    } else if (i < MYO_NU_MAX) xa[i] = xb[i] = xd[i] = Ld[i] = 0;      // (the unrolled products below run over all MYO_NU_MAX entries)
    if (i < nv) {
      double w = (double)((O.reach >> i) & 1ull);
      if (O.weight) w = tmax(O.weight[(O.weight_per_env ? e * nv : (size_t)0) + i], 0.0);
      wd[i] = w;
    }
  }
  SYNC();
  int pinned = 0;
  for (int j = 0; j < nu; ++j) pinned |= xb[j] != 0.0;
  // c = R' b - qfrc, lanes = dofs: actuator i reaches dof d in slot popcount(mask_i below d)
  PHASE {
    const int d = lane;
    if (d < nv) {
      double acc = 0;
      for (int i = 0; i < nu; ++i) {
        const unsigned long long m = M.act_dofmask[i];
        const int k = myo_popcll(m & ((1ull << d) - 1ull));
        if (((m >> d) & 1ull) && k < MYO_TJ_MAX) acc += Rs[i * MYO_TJ_MAX + k] * xa[i];
      }
      xd[d] = wd[d] * (acc - O.qfrc[e * nv + d]);
    }
  }
  SYNC();
  // q = A' sqrt(W) c - reg u_ref, and A's rows in the place of R's
  PHASE {
    const int i = lane;
    if (i < nu) {
      double acc = 0;
      for (int k = 0; k < MYO_TJ_MAX; ++k) { const int d = M.act_sd[i * MYO_TJ_MAX + k]; if (d >= 0) acc += LV(Rk)[k] * xd[d]; }
      acc *= LV(ge);
      LV(q) = acc - reg * LV(uref);
      xb[i] = fabs(acc);
      for (int k = 0; k < MYO_TJ_MAX; ++k) Rs[i * MYO_TJ_MAX + k] = LV(ge) * LV(Rk)[k];
    }
  }
  SYNC();
  double amax = 0;
  for (int j = 0; j < nu; ++j) amax = tmax(amax, xb[j]);
  const double tol = 1e-12 * (1 + amax);
  // H = A'A + reg I into the workspace, row by row, lanes = columns
  for (int i = 0; i < nu; ++i) {
    const unsigned long long mi = M.act_dofmask[i];
    PHASE {
      const int j = lane;
      if (j <= i) {
        unsigned long long c = mi & LV(dmask);
        double acc = j == i ? reg : 0.0;
        while (c) {
          const int d = myo_ffsll(c);
          c &= c - 1;
          const unsigned long long below = (1ull << d) - 1ull;
          const int ki = myo_popcll(mi & below), kj = myo_popcll(LV(dmask) & below);
          if (ki < MYO_TJ_MAX && kj < MYO_TJ_MAX) acc += wd[d] * Rs[i * MYO_TJ_MAX + ki] * Rs[j * MYO_TJ_MAX + kj];
        }
        Hg[MYO_SO_TRI(i) + j] = acc;
      }
    }
  }
  PHASE { if (lane < nu) LV(u) = tclamp(LV(uref), LV(lo), LV(hi)); }
  SYNC_G();      // (other lanes read H's rows below)
  // ... once: lane i keeps row i in registers from here on (every loop over it is unrolled: constant indices)
  PHASE {
    const int i = lane;
    if (i < nu) {
#pragma unroll
      for (int j = 0; j < MYO_NU_MAX; ++j) LV(Hrow)[j] = j < nu ? Hg[MYO_SO_HIDX(i, j)] : 0.0;
    }
  }
  // ---- projected Newton
  // The working set W (clamped variables) starts as the sign rule's set at the start point.  A variable that a step brings to a bound
  // joins W and stays until the iterate minimises the cost on W's face; only there does the sign rule let go of the variables whose
  // multiplier has the wrong sign.  And a step that no backtrack makes acceptable before it stops bending goes exactly to the first
  // bound on the Newton line.  Without the two, the plain scheme crawls on this problem: nu > nv leaves directions whose only
  // curvature is reg (cond(H) ~ 1e9 on the hand), the Newton step along them crosses bounds at tiny alpha, and a variable that sits at
  // a bound with an inward gradient but an outward Newton direction is never clamped (measured: 239 iterations on one test env).
  int it = 0, capped = 1, have_factor = 0;
  unsigned long long W = 0, fmask = 0;
  double pg = 0;
  LANE_VAR(double, ratio);
  for (;;) {
    PHASE { if (lane < nu) xa[lane] = LV(u); }
    SYNC();
    PHASE {
      const int i = lane;
      if (i < nu) {
        double acc = LV(q);
#pragma unroll
        for (int j = 0; j < MYO_NU_MAX; ++j) acc += LV(Hrow)[j] * xa[j];
        LV(gr) = acc;
        const bool pinned_i = LV(lo) >= LV(hi), at_lo = LV(u) <= LV(lo), at_hi = LV(u) >= LV(hi);
        xb[i] = pinned_i ? 0.0 : (at_lo ? tmax(-acc, 0.0) : (at_hi ? tmax(acc, 0.0) : fabs(acc)));      // the projected gradient
        xd[i] = (pinned_i || (at_lo && acc > -tol) || (at_hi && acc < tol)) ? 1.0 : 0.0;              // the sign rule keeps it clamped
        wd[i] = fabs(acc);
      }
    }
    SYNC();
    unsigned long long keep = 0;
    pg = 0;
    for (int j = 0; j < nu; ++j) { pg = tmax(pg, xb[j]); if (xd[j] != 0.0) keep |= 1ull << j; }
    if (it == 0) W = keep;
    if (pg < tol) { capped = 0; break; }
    if (it >= O.max_iter) break;
    double gfree = 0;
    for (int j = 0; j < nu; ++j) if (!((W >> j) & 1ull)) gfree = tmax(gfree, wd[j]);
    if (gfree < tol) W &= keep;      // the minimiser on W's face: release
    if (!have_factor || W != fmask) {
      // H with the clamped rows and columns replaced by identity, then its Cholesky factor: column j, lanes = rows.  Every lane forms the
      // pivot itself from row j (it reads that row anyway), so a column is one phase; the pivot's reciprocal goes to Ld, nobody overwrites what
      // another lane of the phase reads.
      PHASE {
        const int i = lane;
        if (i < nu) {
#pragma unroll
          for (int j = 0; j < MYO_NU_MAX; ++j)
            if (j <= i) Lf[MYO_SO_TRI(i) + j] = (((W >> i) | (W >> j)) & 1ull) ? (i == j ? 1.0 : 0.0) : LV(Hrow)[j];
        }
      }
      SYNC();
      for (int j = 0; j < nu; ++j) {
        PHASE {
          const int i = lane;
          if (i >= j && i < nu) {
            double sjj = Lf[MYO_SO_TRI(j) + j], sij = Lf[MYO_SO_TRI(i) + j];
            for (int k = 0; k < j; ++k) { const double ljk = Lf[MYO_SO_TRI(j) + k]; sjj -= ljk * ljk; sij -= Lf[MYO_SO_TRI(i) + k] * ljk; }
            const double ip = 1.0 / sqrt(tmax(sjj, 1e-300));
            if (i == j) Ld[j] = ip; else Lf[MYO_SO_TRI(i) + j] = sij * ip;
          }
        }
        SYNC();
      }
      have_factor = 1; fmask = W;
    }
    // the Newton direction on the free set: L L' dir = -gradient (0 on the clamped set), column-oriented, lanes = rows
    PHASE { if (lane < nu) xa[lane] = ((W >> lane) & 1ull) ? 0.0 : -LV(gr); }
    SYNC();
    for (int j = 0; j < nu - 1; ++j) {
      PHASE { const int i = lane; if (i > j && i < nu) xa[i] -= Lf[MYO_SO_TRI(i) + j] * (xa[j] * Ld[j]); }
      SYNC();
    }
    PHASE { if (lane < nu) xa[lane] *= Ld[lane]; }
    SYNC();
    for (int j = nu - 1; j > 0; --j) {
      PHASE { const int i = lane; if (i < j) xa[i] -= Lf[MYO_SO_TRI(j) + i] * (xa[j] * Ld[j]); }
      SYNC();
    }
    // ... and how far each variable can go along it (the ratio test)
    PHASE {
      const int i = lane;
      if (i < nu) {
        const double d = ((W >> i) & 1ull) ? 0.0 : xa[i] * Ld[i];
        LV(dir) = d;
        LV(ratio) = d < 0 ? (LV(lo) - LV(u)) / d : (d > 0 ? (LV(hi) - LV(u)) / d : (double)INFINITY);
        xb[i] = LV(ratio);
      }
    }
    SYNC();
    double a1 = (double)INFINITY;
    for (int j = 0; j < nu; ++j) a1 = tmin(a1, xb[j]);
    // projected Armijo backtracking over the steps that bend (alpha > a1); the decrease of the quadratic along
    // d = clip(u + alpha dir) - u is g'd + 1/2 d'Hd exactly.  A straight step (alpha <= min(1, a1)) always passes: Hd = -g on the face.
    double alpha = 1;
    int accepted = 0;
    for (int ls = 0; ls < MYO_SO_BACKTRACKS && alpha > a1 && !accepted; ++ls) {
      PHASE {
        if (lane < nu) {
          LV(uc) = LV(ratio) <= alpha ? (LV(dir) < 0 ? LV(lo) : LV(hi)) : tclamp(LV(u) + alpha * LV(dir), LV(lo), LV(hi));
          LV(dl) = LV(uc) - LV(u);
          xa[lane] = LV(dl);
        }
      }
      SYNC();
      PHASE {
        const int i = lane;
        if (i < nu) {
          double hd = 0;
#pragma unroll
          for (int j = 0; j < MYO_NU_MAX; ++j) hd += LV(Hrow)[j] * xa[j];
          xb[i] = LV(dl) * (LV(gr) + 0.5 * hd);
          xd[i] = LV(dl) * LV(gr);
        }
      }
      SYNC();
      double dcost = 0, slope = 0;
      for (int j = 0; j < nu; ++j) { dcost += xb[j]; slope += xd[j]; }
      if (dcost <= MYO_SO_ARMIJO * slope) accepted = 1; else alpha *= 0.5;
    }
    if (!accepted) alpha = tmin(1.0, a1);
    PHASE {
      if (lane < nu) {
        const bool hit = LV(ratio) <= alpha;
        LV(u) = hit ? (LV(dir) < 0 ? LV(lo) : LV(hi)) : tclamp(LV(u) + alpha * LV(dir), LV(lo), LV(hi));
        xb[lane] = hit ? 1.0 : 0.0;
      }
    }
    SYNC();
    for (int j = 0; j < nu; ++j) if (xb[j] != 0.0) W |= 1ull << j;
    ++it;
  }
  // ---- publish: the input, the (clamped) force, R' force and its distance from the target
  PHASE {
    const int i = lane;
    if (i < nu) {
      double f = LV(g) * LV(u) + LV(b);
      if (LV(flim)) f = tclamp(f, LV(fr0), LV(fr1));
      if (O.u) O.u[e * nu + i] = LV(u);
      if (O.force) O.force[e * nu + i] = f;
      xa[i] = f;
      for (int k = 0; k < MYO_TJ_MAX; ++k) Rs[i * MYO_TJ_MAX + k] = LV(Rk)[k];
    }
  }
  SYNC();
  PHASE {
    const int d = lane;
    if (d < nv) {
      double acc = 0;
      for (int i = 0; i < nu; ++i) {
        const unsigned long long m = M.act_dofmask[i];
        const int k = myo_popcll(m & ((1ull << d) - 1ull));
        if (((m >> d) & 1ull) && k < MYO_TJ_MAX) acc += Rs[i * MYO_TJ_MAX + k] * xa[i];
      }
      if (O.qfrc_out) O.qfrc_out[e * nv + d] = acc;
      if (O.residual) O.residual[e * nv + d] = acc - O.qfrc[e * nv + d];
    }
    if (lane == 0) {
      if (O.kkt) O.kkt[e] = pg;
      if (O.iters) O.iters[e] = it;
      if (O.status) O.status[e] = (capped ? MYO_SO_ST_CAP : 0) | (pinned ? MYO_SO_ST_PINNED : 0);
    }
  }
  SYNC();
  ws_release(K, s);
}

// the job of myo_batch_static_opt (jobs: csrc/myo_task.h); keyed without the integrator, the pass integrates nothing
struct StaticOptJob { static constexpr bool RK = false; StaticOptDev O; };
MYO_JOB_RUN(StaticOptJob) { env_static_opt(M, K, L, MYO_ENV_REC(block), s, block, J.O); }
