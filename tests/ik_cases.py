"""Cases of the inverse-kinematics solve (myo_batch_ik, csrc/myo_ik.h) shared by the emulation (CPU) and HIP (GPU) tests of
tests/test_ik.py.  Every case goes through the C ABI.  The references are algorithm-independent: the projected gradient recomputed
from data()'s site_xpos and jac("site") of a SECOND batch set to the returned qpos (read-outs pinned by tests/data_cases.py and
tests/jac_cases.py), and scipy.optimize.least_squares (trf, bounds, every tolerance 1e-15) from the same start.

The problem, per env, a = active joints (hinge / slide):
  f(q) = 1/2 sum_o w_o |x_o(q) - t_o|^2 + 1/2 reg sum_a (q_a - q_ref_a)^2,   g = J_a' W e + reg (q_a - q_ref_a),   lo <= q_a <= hi

Bounds (eps = 2^-52; `mul` = TOL[dtype] / TOL[f64] of tests/data_cases.py for another dtype than f64, as tests/jac_cases.py does).
  feasibility          lo <= q <= hi exactly; frozen qpos entries bit for bit the start's.
  descent              f(q) <= f(projected start) (1 + 64 eps): both sides evaluated here from the second batch's read-outs (64 eps: two
                       evaluations of one sum of <= 3 k + n_act non-negative terms, when no step was taken).
  KKT                  the recomputed projected gradient's max-norm <= 2 tol (1 + |J'We|_inf at the start) + 64 eps max_a sum |J| |We|
                       (the solver's stop rule twice — another evaluation of the same gradient — plus that sum's rounding).
  optimality           f - f_scipy <= 4 n_act kkt^2 / (2 reg) + 64 eps f: strong convexity (modulus reg) of the regularised problem on
                       the free set; one-sided, scipy is the less converged of the two at bounds.
  consistency          site_xpos / residual within 1e-13 of data() at the returned qpos; cost within 64 eps of its definition.
"""
import ctypes as C
import os

import numpy as np

import data_cases as dc
import jac_cases as jc
import sensor_cases as sc
from helpers import Mem, oracle_for
from myochallenge_amd import native

EPS = np.finfo(np.float64).eps
HEALTHY = sc.HEALTHY
KEYS = native.IK_KEYS
REG, TOLK = 1e-6, 1e-10
F64 = native.MYO_F64


def mul(dtype):
    return dc.TOL[dtype] / dc.TOL[F64]


# ---------------------------------------------------------------------------------------------------------------- plumbing
def ik_all(b, mem, ids, targets, want=KEYS, weight=None, q_init=None, q_ref=None, lower=None, upper=None, active=0, reg=REG, tol=TOLK,
           max_iter=50):
    """host copies of the outputs of every env; the outputs are pre-filled (NaN / -7) and no fill may survive"""
    ids = np.asarray(ids, np.int32)
    sh = b.ik_shapes(len(ids))
    out = {k: mem.arr(np.full((b.n,) + sh[k][0], np.nan if sh[k][1] is np.float64 else -7), sh[k][1]) for k in want}
    opt = lambda x: None if x is None else mem.arr(x)
    b.ik(mem.arr(ids, np.int32), mem.arr(np.asarray(targets, float).reshape(b.n, len(ids), 3)), opt(weight),
         weight is not None and np.ndim(weight) == 2, opt(q_init), opt(q_ref), opt(lower), opt(upper), active, reg, tol, max_iter, **out)
    res = {k: mem.host(v).copy() for k, v in out.items()}
    for k, v in res.items():
        assert not (np.isnan(v).any() if v.dtype == np.float64 else (v == -7).any()), k
    return res


def readouts(ref, mem, om, qpos, ids):
    """site_xpos [N, k, 3] and jacp [N, k, 3, nv] of the sites at qpos [N, nq], from the second batch's data() and jac("site")"""
    n = ref.n
    ref.set_state(mem.arr(qpos), mem.zeros((n, om.nv)), mem.zeros((n, om.na)), mem.zeros(n))
    x = dc.data_all(ref, mem, ["site_xpos"])["site_xpos"]
    ids = np.asarray(ids)
    ok = (ids >= 0) & (ids < x.shape[1])
    J = jc.jac_all(ref, mem, "site", ids, want=("jacp",))["jacp"]
    return np.where(ok[None, :, None], x[:, np.where(ok, ids, 0)], 0.0), J


def tip_sites(cm):
    """the last site on every childless body that no free joint carries: one per finger"""
    f = cm.fields
    par, sb, jt, jb = (np.asarray(f[k]) for k in ("body_parentid", "site_bodyid", "jnt_type", "jnt_bodyid"))
    free = set(jb[jt == 0].tolist())
    return [int(np.flatnonzero(sb == b)[-1]) for b in range(1, len(par)) if not (par[1:] == b).any() and b not in free and (sb == b).any()]


class Problem:
    """the problems of a batch in numpy float64"""

    def __init__(self, cm, n, ids, targets, weight=None, reg=REG, q_ref=None, lower=None, upper=None, active=None):
        f = cm.fields
        jt, qadr, dadr = (np.asarray(f[k]) for k in ("jnt_type", "jnt_qposadr", "jnt_dofadr"))
        lim, rng = np.asarray(f["jnt_limited"]), np.asarray(f["jnt_range"], float).reshape(-1, 2)
        hs = [j for j in range(len(jt)) if jt[j] in (2, 3) and (active is None or int(dadr[j]) in active)]
        self.dofs, self.qadr = dadr[hs].astype(int), qadr[hs].astype(int)
        self.lo = np.tile(np.where(lim[hs] != 0, rng[hs, 0], -np.inf), (n, 1)) if lower is None else np.asarray(lower)[:, self.dofs]
        self.hi = np.tile(np.where(lim[hs] != 0, rng[hs, 1], np.inf), (n, 1)) if upper is None else np.asarray(upper)[:, self.dofs]
        self.pin = self.lo > self.hi
        self.hi = np.where(self.pin, self.lo, self.hi)
        ids = np.asarray(ids)
        self.t = np.asarray(targets, float).reshape(n, len(ids), 3)
        w = np.ones((n, len(ids))) if weight is None else np.broadcast_to(np.maximum(np.asarray(weight, float), 0), (n, len(ids)))
        self.w = w * ((ids >= 0) & (ids < len(f["site_bodyid"])))[None]
        self.reg, self.q_ref, self.n = reg, q_ref, n

    def cost(self, e, q, x):
        return 0.5 * (self.w[e] * ((x - self.t[e]) ** 2).sum(1)).sum() + 0.5 * self.reg * ((q[self.qadr] - self.q_ref[e][self.qadr]) ** 2).sum()

    def grad(self, e, q, x, J):
        """(gradient over the active joints, |J'We|_inf, max_a sum |J| |We|)"""
        Ja = J[:, :, self.dofs].reshape(-1, len(self.dofs))
        We = (self.w[e][:, None] * (x - self.t[e])).reshape(-1)
        jwe = Ja.T @ We
        return jwe + self.reg * (q[self.qadr] - self.q_ref[e][self.qadr]), np.abs(jwe).max(initial=0.0), (np.abs(Ja).T @ np.abs(We)).max(initial=0.0)

    def kkt(self, e, q, g):
        qa, lo, hi = q[self.qadr], self.lo[e], self.hi[e]
        at_lo, at_hi = qa <= lo, qa >= hi
        v = np.where(at_lo & at_hi, 0.0, np.where(at_lo, np.maximum(-g, 0), np.where(at_hi, np.maximum(g, 0), np.abs(g))))
        return float(v.max(initial=0.0))

    def scipy(self, e, q0, evaluate):
        """scipy's trust-region reflective least squares on the augmented residual from q0 [nq]; evaluate(q) -> (x [k, 3], J [k, 3, nv])"""
        from scipy.optimize import least_squares
        sw, sr, ref = np.sqrt(self.w[e]), np.sqrt(self.reg), self.q_ref[e][self.qadr]
        cache = {}

        def both(z):
            key = z.tobytes()
            if key not in cache:
                cache.clear()
                q = q0.copy()
                q[self.qadr] = z
                cache[key] = evaluate(q)
            return cache[key]
        fun = lambda z: np.concatenate([(sw[:, None] * (both(z)[0] - self.t[e])).reshape(-1), sr * (z - ref)])
        jac = lambda z: np.vstack([(sw[:, None, None] * both(z)[1][:, :, self.dofs]).reshape(-1, len(self.dofs)), sr * np.eye(len(self.dofs))])
        r = least_squares(fun, q0[self.qadr], jac=jac, bounds=(self.lo[e], self.hi[e]), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
        return r.x, float(r.cost)


class Setup:
    """a batch to solve on, a second batch of the same model for the read-outs, a one-env batch for scipy, start points and targets"""

    def __init__(self, lib, dtype, which, seed=0, n=None, spread=0.3, task=True):
        from myochallenge_amd.mjb import load_mjb
        from myochallenge_amd.synth_hand import synthetic_hand_pose
        self.mem = mem = Mem(lib)
        self.which, self.dtype = which, dtype
        rng = np.random.RandomState(seed + 17)
        if which == "finger":
            mj = load_mjb(os.path.join(dc.GOLDEN, "myo_finger_v0.mjb"))
            self.cm, self.om, _ = oracle_for(mj)
            self.n, cfg = n or 4, None
            self.ids = [list(self.cm.names["site"]).index("IFtip")]
        elif which == "pose":
            from myochallenge_amd.envs.pose import make_pose_cfg
            self.cm, self.om, _ = oracle_for(synthetic_hand_pose())
            self.n, cfg = n or 3, make_pose_cfg("CustomMyoHandPoseRandom", self.cm)
            self.ids = tip_sites(self.cm)
        else:
            from myochallenge_amd.envs.config import make_task_cfg
            self.cm, self.om = sc.hand_model()
            self.n, cfg = n or 2, make_task_cfg("CustomMyoBaodingBallsP2", self.cm)
            self.ids = tip_sites(self.cm)
        cm, om, n = self.cm, self.om, self.n
        model = native.Model(cm, lib)
        self.b = native.Batch(model, cfg if task else None, n, 0, seed, dtype)
        self.ref = native.Batch(model, None, n, 0, 0, dtype)
        self.one = native.Batch(model, None, 1, 0, 0, dtype)
        if cfg is not None and task:
            self.b.reset(None, mem.zeros((n, self.b.obs_dim), np.float32))
        present = mem.zeros((n, om.nq))
        self.b.get_state(present, None, None, None)
        present = mem.host(present).copy()
        base = Problem(cm, n, self.ids, np.zeros((n, len(self.ids), 3)))
        self.dofs, self.qadr = base.dofs, base.qadr
        # start = qpos0 + U(-0.1, 0.1) on the active joints, clipped to range; the other entries are the env's present ones
        q0 = present.copy()
        q0[:, self.qadr] = np.clip(np.asarray(cm.fields["qpos0"], float)[self.qadr][None] + rng.uniform(-0.1, 0.1, (n, len(self.qadr))), base.lo, base.hi)
        self.q0 = q0
        # targets = the sites at the start + U(-spread, spread) on the active joints, clipped
        qt = q0.copy()
        qt[:, self.qadr] = np.clip(q0[:, self.qadr] + rng.uniform(-spread, spread, (n, len(self.qadr))), base.lo, base.hi)
        self.targets = readouts(self.ref, mem, om, qt, self.ids)[0]
        self.explicit_start = which == "hand"
        if not self.explicit_start:      # the finger and the pose hand start from the env's present qpos, the Baoding hand from q_init
            self.b.set_state(mem.arr(q0), None, None, None)

    def start(self):
        return self.q0 if self.explicit_start else None

    def evaluate_one(self, ids):
        def f(q):
            x, J = readouts(self.one, self.mem, self.om, q[None], ids)
            return x[0], J[0]
        return f

    def close(self):
        for x in (self.b, self.ref, self.one):
            x.close()


def check(S, out, P, ids, q_start, label, tol=TOLK, kkt=True, expect_status=0, scipy=False):
    """assertions 1-6 on one call's outputs; q_start: the start point [N, nq] as given to the call.  Returns the recomputed kkt norms."""
    m = mul(S.dtype)
    n, q = S.n, out["qpos"]
    proj = q_start.copy()
    proj[:, P.qadr] = np.clip(q_start[:, P.qadr], P.lo, P.hi)
    x0, J0 = readouts(S.ref, S.mem, S.om, proj, ids)
    x, J = readouts(S.ref, S.mem, S.om, q, ids)
    frozen = np.setdiff1d(np.arange(S.om.nq), P.qadr)
    norms = []
    for e in range(n):
        qa = q[e][P.qadr]
        assert (qa >= P.lo[e]).all() and (qa <= P.hi[e]).all(), (label, e)                                   # 1. feasibility
        assert np.array_equal(q[e][frozen], q_start[e][frozen]), (label, e)
        f0, f1 = P.cost(e, proj[e], x0[e]), P.cost(e, q[e], x[e])
        g0, jwe0, _ = P.grad(e, proj[e], x0[e], J0[e])
        g, _, noise = P.grad(e, q[e], x[e], J[e])
        own = P.kkt(e, q[e], g)
        bound = 2 * tol * (1 + jwe0) + 64 * EPS * noise
        print(f"    {label} env {e}: cost {out['cost'][e]:.6e} (start {f0:.6e}) kkt {out['kkt'][e]:.3e} (own {own:.3e}, bound {bound:.3e}) "
              f"iters {out['iters'][e]} status {out['status'][e]} at bounds {int(((qa == P.lo[e]) | (qa == P.hi[e])).sum())}")
        assert f1 <= f0 * (1 + 64 * EPS), (label, e, f1, f0)                                                   # 2. descent
        if expect_status is not None:
            assert out["status"][e] == expect_status, (label, e, out["status"][e])                            # 3. convergence
        assert 0 <= out["iters"][e]
        if kkt and not out["status"][e] & (native.IK_CAP | native.IK_STALL):
            assert own <= bound * m, (label, e, own, bound)                                                    # 4. KKT
        assert np.abs(out["site_xpos"][e] - x[e]).max(initial=0.0) <= 1e-13 * m, (label, e)                   # 6. consistency
        okrow = (P.w[e] > 0) | ((np.asarray(ids) >= 0) & (np.asarray(ids) < len(S.cm.fields["site_bodyid"])))
        assert np.abs(out["residual"][e] - np.where(okrow[:, None], x[e] - P.t[e], 0.0)).max(initial=0.0) <= 1e-13 * m, (label, e)
        own_cost = P.cost(e, q[e], np.where(okrow[:, None], out["residual"][e] + P.t[e], 0.0))
        assert abs(out["cost"][e] - own_cost) <= 64 * EPS * max(own_cost, 1e-300), (label, e, out["cost"][e], own_cost)
        if scipy:                                                                                              # 5. optimality
            zs, fs = P.scipy(e, proj[e], S.evaluate_one(ids))
            slack = 4 * len(P.dofs) * own ** 2 / (2 * P.reg) + 64 * EPS * f1
            print(f"        scipy cost {fs:.6e}: cost - scipy {f1 - fs:.3e} (bound {slack:.3e}), |q - scipy|_inf {np.abs(qa - zs).max():.3e}")
            assert f1 - fs <= slack * m, (label, e, f1, fs, slack)
        norms.append(own)
    return norms


# ---------------------------------------------------------------------------------------------------------------- 1.-6. the reachable sets
def case_solve(lib, dtype, which, spread=0.3, scipy=True):
    S = Setup(lib, dtype, which, spread=spread)
    out = ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.start())
    P = Problem(S.cm, S.n, S.ids, S.targets, q_ref=S.q0)
    assert (out["iters"] <= 50).all()
    check(S, out, P, S.ids, S.q0, f"{which} spread {spread}", scipy=scipy)
    assert S.b.health() == HEALTHY
    S.close()


# ---------------------------------------------------------------------------------------------------------------- 7. unreachable target
def case_unreachable(lib, dtype=F64):
    """the finger's wide set pushed 8 cm in +z: converged (KKT as above, status 0) with a residual that stays.  How far a pushed target
    is out of reach is a property of the inputs, so it is taken from scipy alone: with these inputs its minimum leaves 8.0 cm in env 2
    and 1.3 cm in env 3 and under 5 mm in the other two (the finger reaches them by extending); the solver's residual must agree with
    scipy's in every env and exceed 1 cm in those where scipy's does, and there must be two such envs."""
    S = Setup(lib, dtype, "finger", spread=1.0)
    t = S.targets.copy()
    t[:, :, 2] += 0.08
    out = ik_all(S.b, S.mem, S.ids, t)
    P = Problem(S.cm, S.n, S.ids, t, q_ref=S.q0)
    check(S, out, P, S.ids, S.q0, "finger unreachable")
    far = 0
    for e in range(S.n):
        zs, fs = P.scipy(e, S.q0[e], S.evaluate_one(S.ids))
        qs = S.q0[e].copy()
        qs[P.qadr] = zs
        rs = np.linalg.norm(S.evaluate_one(S.ids)(qs)[0] - t[e], axis=1)
        r = np.linalg.norm(out["residual"][e], axis=1)
        print(f"    env {e}: residual {r} scipy {rs}")
        assert np.abs(r - rs).max() <= 1e-6, (e, r, rs)
        if (rs > 0.01).all():
            far += 1
            assert (r > 0.01).all(), (e, r)
    assert far >= 2, "the inputs leave fewer than two targets out of reach"
    S.close()


# ---------------------------------------------------------------------------------------------------------------- 8. caps
def case_caps(lib, dtype=F64):
    S = Setup(lib, dtype, "pose")
    out = ik_all(S.b, S.mem, S.ids, S.targets, max_iter=1)
    P = Problem(S.cm, S.n, S.ids, S.targets, q_ref=S.q0)
    assert (out["status"] == native.IK_CAP).all() and (out["iters"] == 1).all(), (out["status"], out["iters"])
    check(S, out, P, S.ids, S.q0, "pose max_iter 1", kkt=False, expect_status=native.IK_CAP)
    # lower > upper on one dof of env 1: pinned at lower, and the status says so
    lo, hi = np.full((S.n, S.om.nv), -np.inf), np.full((S.n, S.om.nv), np.inf)
    lo[:, P.dofs], hi[:, P.dofs] = P.lo, P.hi
    d = int(P.dofs[3])
    lo[1, d], hi[1, d] = 0.2, 0.1
    out = ik_all(S.b, S.mem, S.ids, S.targets, lower=lo, upper=hi)
    assert out["qpos"][1, P.qadr[3]] == 0.2
    # (the pin leaves env 1's targets out of reach: a Gauss-Newton model converges slowly there, so only the flag is asked of it)
    assert out["status"][1] & native.IK_PINNED and (np.delete(out["status"], 1) == 0).all(), out["status"]
    P2 = Problem(S.cm, S.n, S.ids, S.targets, q_ref=S.q0, lower=lo, upper=hi)
    assert P2.pin[1, 3] and P2.pin.sum() == 1
    check(S, out, P2, S.ids, S.q0, "pose pinned", expect_status=None)
    S.close()


# ---------------------------------------------------------------------------------------------------------------- 9. options
def case_options(lib, dtype=F64):
    S = Setup(lib, dtype, "hand")
    cm, n, nq = S.cm, S.n, S.om.nq
    # a subset of the joints moves nothing else
    sub = [int(d) for d in S.dofs[[0, 2, 5, 6, 7]]]
    mask = sum(1 << d for d in sub)
    out = ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.q0, active=mask)
    P = Problem(cm, n, S.ids, S.targets, q_ref=S.q0, active=sub)
    assert len(P.dofs) == 5
    check(S, out, P, S.ids, S.q0, "hand subset", expect_status=None)      # (five joints do not reach the targets: convergence is not asked)
    assert not np.array_equal(out["qpos"], S.q0)
    # ... and bits of the balls' free joints in the mask are ignored
    free_bits = sum(1 << d for d in range(S.om.nv) if d not in set(S.dofs.tolist()))
    again = ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.q0, active=mask | free_bits)
    for k in KEYS:
        assert np.array_equal(out[k], again[k]), k
    # a target of weight 0 leaves KKT satisfied for the others, whatever its target is (shared and per-env weights: the same bits)
    w = np.ones(len(S.ids))
    w[1] = 0
    t2 = S.targets.copy()
    t2[:, 1] += 5.0
    a, b2 = ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.q0, weight=w), ik_all(S.b, S.mem, S.ids, t2, q_init=S.q0, weight=np.tile(w, (n, 1)))
    for k in ("qpos", "site_xpos", "cost", "kkt", "iters", "status"):
        assert np.array_equal(a[k], b2[k]), k
    check(S, a, Problem(cm, n, S.ids, S.targets, weight=w, q_ref=S.q0), S.ids, S.q0, "hand weight 0")
    wn = w.copy()
    wn[1] = -2.0      # negative weights count as 0
    assert np.array_equal(ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.q0, weight=wn)["qpos"], a["qpos"])
    # k = 0: q is clip(q_ref) within tol
    P0 = Problem(cm, n, [], np.zeros((n, 0, 3)), q_ref=S.q0)
    rng = np.random.RandomState(5)
    qref = S.q0.copy()
    qref[:, S.qadr] += rng.uniform(-3, 3, (n, len(S.qadr)))
    out = ik_all(S.b, S.mem, [], np.zeros((n, 0, 3)), q_init=S.q0, q_ref=qref)
    assert (out["status"] == 0).all() and np.abs(out["qpos"][:, S.qadr] - np.clip(qref[:, S.qadr], P0.lo, P0.hi)).max() <= TOLK
    assert out["site_xpos"].shape == (n, 0, 3)
    # a site on a ball (no active dof above it): a constant residual, no NaN; an id outside the model: zero rows
    ball = list(cm.names["site"]).index("ball1_site")
    ids = [S.ids[0], ball, len(cm.fields["site_bodyid"]) + 3, S.ids[3], -1]
    t5 = np.zeros((n, 5, 3))
    t5[:, 0], t5[:, 3] = S.targets[:, 0], S.targets[:, 3]
    t5[:, 1] = 0.5
    out = ik_all(S.b, S.mem, ids, t5, q_init=S.q0)
    P5 = Problem(cm, n, ids, t5, q_ref=S.q0)
    check(S, out, P5, ids, S.q0, "hand ball site")
    xb = readouts(S.ref, S.mem, S.om, S.q0, [ball])[0][:, 0]
    assert np.abs(out["residual"][:, 1] - (xb - 0.5)).max() <= 1e-13 * mul(dtype)
    assert not out["site_xpos"][:, [2, 4]].any() and not out["residual"][:, [2, 4]].any()
    assert S.b.health() == HEALTHY
    S.close()


# ---------------------------------------------------------------------------------------------------------------- 10. read-only
def _fatigue(b, mem, om):
    st = mem.zeros((b.n, 3, om.nu))
    b.fatigue(None, st)
    return mem.host(st).copy()


def _run(lib, mem, dtype, n, seed, nsteps, call_between, condition=None):
    from myochallenge_amd.envs.config import make_task_cfg
    cm, om = sc.hand_model()
    kw = {} if condition is None else dict(muscle_condition=condition)
    b = native.Batch(native.Model(cm, lib), make_task_cfg("CustomMyoBaodingBallsP2", cm, **kw), n, 0, seed, dtype)
    obs, rew, done = mem.zeros((n, b.obs_dim), np.float32), mem.zeros(n, np.float32), mem.zeros(n, np.uint8)
    b.reset(None, obs)
    rng, rng_t = np.random.RandomState(seed), np.random.RandomState(seed + 1)
    ids = tip_sites(cm)
    trace = []
    for i in range(nsteps):
        if call_between and i >= nsteps - 2:
            before = sc.device_state(b, mem, om) + list(dc.task_arrays(b, mem)) + ([_fatigue(b, mem, om)] if condition == "fatigue" else [])
            x = dc.data_all(b, mem, ["site_xpos"])["site_xpos"][:, ids]
            out = ik_all(b, mem, ids, x + rng_t.uniform(-0.02, 0.02, x.shape), max_iter=6)
            assert np.isfinite(out["cost"]).all()
            after = sc.device_state(b, mem, om) + list(dc.task_arrays(b, mem)) + ([_fatigue(b, mem, om)] if condition == "fatigue" else [])
            for p, q in zip(before, after):
                assert np.array_equal(p, q)
        b.step(mem.arr(np.clip(rng.normal(0, 0.5, (n, om.nu)), -1, 1), np.float32), obs, rew, done)
        trace.append([mem.host(x).copy() for x in (obs, rew, done)])
    return b, trace


def case_read_only(lib, dtype, n=2, seed=5, nsteps=4, condition=None):
    """two batches of one seed; one solves before each of the last 2 steps, the other never: state, warm start, task state, fatigue
    state, observations and health are the same bits"""
    mem = Mem(lib)
    _, om = sc.hand_model()
    a, ta = _run(lib, mem, dtype, n, seed, nsteps, True, condition)
    b, tb = _run(lib, mem, dtype, n, seed, nsteps, False, condition)
    for x, y in zip(sc.device_state(a, mem, om) + list(dc.task_arrays(a, mem)), sc.device_state(b, mem, om) + list(dc.task_arrays(b, mem))):
        assert np.array_equal(x, y)
    if condition == "fatigue":
        assert np.array_equal(_fatigue(a, mem, om), _fatigue(b, mem, om))
    for sa, sb in zip(ta, tb):
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)
    assert a.health() == b.health() == HEALTHY
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 11. determinism
def case_determinism(lib, dtype, which="hand"):
    S = Setup(lib, dtype, which)
    a, b = (ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.start()) for _ in range(2))
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    # a single output gives the bits the full call gives
    for k in ("qpos", "status"):
        assert np.array_equal(ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.start(), want=(k,))[k], a[k]), k
    S.close()


# ---------------------------------------------------------------------------------------------------------------- the large batch (GPU)
def case_batch_130(lib, dtype=F64, n=130):
    """an odd count past two waves' worth of blocks of reachable problems: every env converged (assertions 1-4, 6); the first envs are
    a small batch's, bit for bit (what an indexing error would break)"""
    S = Setup(lib, dtype, "hand", n=n, task=False)
    out = ik_all(S.b, S.mem, S.ids, S.targets, q_init=S.q0)
    P = Problem(S.cm, n, S.ids, S.targets, q_ref=S.q0)
    norms = check(S, out, P, S.ids, S.q0, "hand 130")
    assert (out["iters"] <= 50).all()
    assert len(norms) == n
    small = Setup(lib, dtype, "hand", n=2, task=False)
    small.q0[:], small.targets[:] = S.q0[:2], S.targets[:2]
    o2 = ik_all(small.b, small.mem, small.ids, small.targets, q_init=small.q0)
    for k in KEYS:
        assert np.array_equal(o2[k], out[k][:2]), k
    small.close()
    S.close()


# ---------------------------------------------------------------------------------------------------------------- 12. bad arguments
def case_bad_args(lib):
    """struct sizes of another version, NULLs and bad scalars are refused before any device call (MYO_E_BADARG = MYO_E_ARG = -1): the
    NaN-filled outputs stay untouched; all-NULL outputs launch nothing"""
    mem = Mem(lib)
    b = sc.baoding_batch(lib, mem, native.MYO_MIXED, 1, 0, 0)
    nq, L, P = b.model.size("nq"), lib.L, native._ptr
    ids, tg, q = mem.arr([4, 5], np.int32), mem.zeros((1, 2, 3)), mem.arr(np.full((1, nq), np.nan))
    si, so = C.sizeof(native.IkIn), C.sizeof(native.IkOut)
    assert si == 112 and so == 64
    i, o = native.IkIn(), native.IkOut()
    i.size, i.site_ids, i.k, i.targets, i.reg, i.tol, i.max_iter = si, P(ids), 2, P(tg), 1e-6, 1e-10, 50
    o.size, o.qpos = so, P(q)
    call = lambda bb=b.h, ii=i, oo=o: L.myo_batch_ik(bb, None if ii is None else C.byref(ii), None if oo is None else C.byref(oo), None)
    for size in (0, si - 8, si + 8):
        i.size = size
        assert call() == -1 and b"size" in L.myo_last_error()
    i.size = si
    for size in (0, so - 8, so + 8):
        o.size = size
        assert call() == -1 and b"size" in L.myo_last_error()
    o.size = so
    assert call(bb=None) == -1 and call(ii=None) == -1 and call(oo=None) == -1
    i.targets = None
    assert call() == -1 and b"targets" in L.myo_last_error()
    i.targets = P(tg)
    for k in (-1, native.IK_K_MAX + 1):
        i.k = k
        assert call() == -1 and b"k must" in L.myo_last_error()
    i.k, i.site_ids = 2, None
    assert call() == -1 and b"site_ids" in L.myo_last_error()
    i.site_ids = P(ids)
    for reg in (0.0, -1e-6, float("nan"), float("inf")):
        i.reg = reg
        assert call() == -1 and b"reg" in L.myo_last_error()
    i.reg = 1e-6
    for tol in (0.0, -1.0, float("nan")):
        i.tol = tol
        assert call() == -1 and b"tol" in L.myo_last_error()
    i.tol = 1e-10
    for mi in (0, -5):
        i.max_iter = mi
        assert call() == -1 and b"max_iter" in L.myo_last_error()
    i.max_iter = 50
    assert np.isnan(mem.host(q)).all()
    none = native.IkOut()
    none.size = so
    i.reg = -1.0
    assert call(oo=none) == 0                                   # all NULL: a no-op, nothing is looked at
    i.reg = 1e-6
    assert np.isnan(mem.host(q)).all()
    assert call() == 0 and not np.isnan(mem.host(q)).any()
    i.k, i.site_ids, i.targets = 0, None, None                  # k = 0 needs neither
    assert call() == 0
    with np.testing.assert_raises(KeyError):
        b.ik(ids, tg, no_such_key=q)
    assert b.health() == HEALTHY
    b.close()
