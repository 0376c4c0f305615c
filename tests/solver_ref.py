"""Float64 / long-double references of the three linear solves of a substep (tests/test_solver_paths.py).  Plain numpy.

Everything the references are made of comes from the ORACLE's forward pass at the state: M (dense and symmetric there; its pattern
is checked against dof_parentid: M[i, j] != 0 only where j is an ancestor of i), qfrc_bias, qfrc_passive, qfrc_actuator, qacc_smooth,
qacc, the constraint rows; dof_damping, timestep, tolerance and meaninertia from the compiled model.  The solves themselves are a
hand-written Cholesky in np.longdouble (<= 36 x 36).

Bounds (eps = 2^-52 for the fp64 stepper, 2^-23 for the mixed one; cond_2 and lambda_min of the oracle's matrix, computed here):
  M solve        |qacc_smooth - ref|_inf <= nv eps cond_2(M) |ref|_inf,  ref = solve_ld(M, qfrc_passive - qfrc_bias + qfrc_actuator):
                 the forward-error bound of a Cholesky solve.  Mixed: the smaller of that and the project's 1e-4 |ref|_inf.
  damped solve   one Euler substep: |qvel' - ref|_inf <= h (nv eps cond_2(M + hB) |x|_inf + stop / lambda_min(M + hB)),
                 x = solve_ld(M + hB, M qacc_oracle), ref = qvel + h x; stop = tolerance meaninertia nv is what the Newton solver's
                 stop rule (scale |grad| < tolerance, scale = 1 / (meaninertia nv)) leaves of M (qacc - qacc_oracle).  Mixed: the smaller
                 of that and 1e-4 |ref|_inf.
  Newton solve   qacc against the oracle's: rel_err < 1e-9 (fp64) / 1e-4 (mixed), the project's standing bounds.
                 KKT residual r = M qacc + qfrc_bias - qfrc_passive - qfrc_actuator - qfrc_constraint(qacc), the last from
                 Batch.inverse (one constraint update, no solve): |r|_2 <= stop.  Only states where the oracle's own qacc meets that
                 bound count (one that does not has run into the iteration cap); none of the zoo's states is dropped.
                 The mixed stepper evaluates the constraint force and its own gradient in fp32, so there the residual carries the
                 rounding of that evaluation, and even the oracle's qacc misses the bare stop bound.  Its bound is stop + gamma |m|_1,
                 gamma = n 2^-24 the worst-case error factor of an n-term fp32 sum (n = the longest sum: MYO_MV_ROW = 24 entries of
                 a row of M, or the nefc rows of a column of J), m = |M| |qacc| + |qfrc_bias| + |qfrc_passive| + |qfrc_actuator|
                 + |J|' (|efc_force| + D (|J| |qacc| + |aref|)) from the oracle's rows: reasoning from the number format, not from
                 measurements; it is a weak bound (1e-5 .. 1e-3) that catches gross errors only.
  cross-path     the same state with and without MYO_DENSE_NEWTON / MYO_DENSE_MSOLVE: rel_err < 1e-9 / 1e-4 on qacc_smooth and qacc.

Measured worst values over the zoo (12 models x 3 envs x {no switch, MYO_DENSE_NEWTON, MYO_DENSE_MSOLVE}; warm-start cases included):
                                                   emulation            MI355X
                                                   fp64      mixed      fp64      mixed
  M solve       err / (eps cond_2 |ref|)           2.1       1.8        2.1       2.3
                err / bound                        0.13      0.36       0.19      0.14
  damped solve  err / (h eps cond_2 |x|)           17        5.3        16        7.9       (the Newton term carries it)
                err / bound                        2.8e-5    0.35       3.6e-5    0.88      (mixed: the 1e-4 |ref|_inf cap is the bound)
  Newton        rel_err(qacc) / (1e-9 | 1e-4)      9.8e-6    5.2e-2     4.8e-5    2.5e-2
                |r|_2 / bound                      1.5e-4    6.7e-2     2.5e-4    8.0e-2    (fp64: |r|_2 <= 7.2e-14 against stop 1.3e-11 .. 2.9e-9)
  cross-path    rel_err                            1.4e-15   0          2.3e-15   2.1e-6    (emulation, mixed: both sides run the same code)
  20 substeps   rel_err(qpos)                      6.1e-16   -          1.1e-15   -
No state is dropped by the oracle's own residual.
"""
import numpy as np

LD = np.longdouble
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23


def cholesky_ld(A):
    """lower Cholesky factor of a symmetric positive definite matrix, in long double"""
    A = np.array(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert d > 0, "not positive definite"
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def solve_ld(A, b):
    """A x = b by Cholesky in long double; the result rounded to float64"""
    L = cholesky_ld(A)
    n = L.shape[0]
    y = np.zeros(n, LD)
    for i in range(n):
        y[i] = (LD(b[i]) - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x.astype(np.float64)


def dense_M(M, dof_parentid):
    """the oracle's M [nv * nv] as a matrix, its pattern checked against the dof tree"""
    nv = len(dof_parentid)
    M = np.array(M, float).reshape(nv, nv)
    assert np.array_equal(M, M.T)
    anc = np.eye(nv, dtype=bool)
    for i in range(nv):
        a = int(dof_parentid[i])
        while a >= 0:
            anc[i, a] = True
            a = int(dof_parentid[a])
    assert not M[~(anc | anc.T)].any()
    return M


class Ref:
    """the oracle's forward pass at one state and what the bounds need of it"""

    def __init__(self, cm, om, qpos, qvel, act, warm=None):
        from oracle.oracle import OracleData
        f = cm.fields
        d = OracleData(om)
        d.reset()
        d.qpos[:], d.qvel[:], d.act[:] = qpos, qvel, act
        if warm is not None:
            d.arr("qacc_warmstart")[:] = warm
        d.ctrl[:] = 0
        d.forward()
        self.d, self.nv = d, om.nv
        nv = self.nv
        self.h, self.tolerance, self.meaninertia = float(f["opt_f64"][0]), float(f["opt_f64"][1]), float(f["opt_f64"][7])
        self.stop = self.tolerance * self.meaninertia * nv
        self.M = dense_M(d.M, f["dof_parentid"])
        self.B = np.asarray(f["dof_damping"], float)
        self.qvel = np.array(qvel, float)
        for k in ("qfrc_bias", "qfrc_passive", "qfrc_actuator", "qacc_smooth", "qacc", "qfrc_constraint"):
            setattr(self, k, np.array(d.arr(k)))
        self.ncon, self.nefc, self.nl = d.ncon, d.nefc, d.nl
        self.J = np.array(d.efc_J)[:d.nefc * nv].reshape(d.nefc, nv)
        self.D, self.aref, self.efc_force = np.array(d.efc_D)[:d.nefc], np.array(d.efc_aref)[:d.nefc], np.array(d.efc_force)[:d.nefc]
        self.cond_M = float(np.linalg.cond(self.M))
        self.smooth = self.qfrc_passive - self.qfrc_bias + self.qfrc_actuator
        self.ref_smooth = solve_ld(self.M, self.smooth)
        Mh = self.M + self.h * np.diag(self.B)
        self.cond_Mh, self.lmin_Mh = float(np.linalg.cond(Mh)), float(np.linalg.eigvalsh(Mh)[0])
        self.x_damped = solve_ld(Mh, self.M @ self.qacc)
        self.ref_qvel = self.qvel + self.h * self.x_damped

    # ---- bounds
    def msolve_bound(self, eps):
        b = self.nv * eps * self.cond_M * np.abs(self.ref_smooth).max()
        return min(b, 1e-4 * np.abs(self.ref_smooth).max()) if eps == EPS32 else b

    def damped_bound(self, eps):
        b = self.h * (self.nv * eps * self.cond_Mh * np.abs(self.x_damped).max() + self.stop / self.lmin_Mh)
        return min(b, 1e-4 * np.abs(self.ref_qvel).max()) if eps == EPS32 else b

    def kkt(self, qacc, qfrc_constraint):
        """|r|_2 of the stationarity residual at qacc, with the device's qfrc_constraint(qacc)"""
        r = self.M @ qacc + self.qfrc_bias - self.qfrc_passive - self.qfrc_actuator - qfrc_constraint
        return float(np.linalg.norm(r))

    def kkt_bound(self, eps, qacc):
        if eps == EPS64:
            return self.stop
        aJ = np.abs(self.J)
        mag = (np.abs(self.M) @ np.abs(qacc) + np.abs(self.qfrc_bias) + np.abs(self.qfrc_passive) + np.abs(self.qfrc_actuator)
               + aJ.T @ (np.abs(self.efc_force) + self.D * (aJ @ np.abs(qacc) + np.abs(self.aref))))
        return self.stop + max(24, self.nefc) * 2.0 ** -24 * float(mag.sum())

    # ---- the solver's choice of starting point (myo_physics.h newton_solve: the cheaper of qacc_warmstart and qacc_smooth)
    def cost(self, x):
        jar = self.J @ x - self.aref
        dx = x - self.qacc_smooth
        return 0.5 * float((self.D * np.minimum(jar, 0) ** 2).sum()) + 0.5 * float(dx @ self.M @ dx)

    def uses_warm(self, warm):
        return self.cost(np.asarray(warm, float)) < self.cost(self.qacc_smooth)


# worst ratios of a run, {(backend, dtype, kind): value}: the tests fill it and print it (-s); the table above is copied from there
WORST = {}


def record(backend, dtype, kind, value):
    key = (backend, dtype, kind)
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    return value
