"""Cases of the Jacobian and inverse-dynamics read-outs (myo_batch_jac / myo_batch_inverse, csrc/myo_jac.h) shared by the emulation
(CPU) and HIP (GPU) tests of tests/test_jac_inverse.py.  Every case goes through the C ABI.  No oracle code: the references are
finite differences of read-outs that tests/data_cases.py pins to the oracle (poses), and identities between existing read-outs.

Bounds.
  finite differences   |jac . d - (x+ - x-) / 2 eps| <= 1e-7 max(1, |value|) per element, eps = 1e-6: the poses carry ~1e-15 absolute
                       rounding, so the quotient is good to ~2e-9; truncation is O(eps^2).
  identities           1e-12 max(1, |value|): both sides are fp64 sums of <= 35 terms of the same numbers.
  forward / inverse    |qfrc_inverse - qfrc_actuator|_inf <= 4 |r|_inf + 1e-10 max|qfrc_*|, r = the forward solver's own stationarity
                       residual from read-outs that exist without this feature (4: summation order — the constraint force is continuous
                       and piecewise linear in jar; the floor: fp64 rounding of a 35-term sum).  The residual itself: |r|_2 <= tolerance
                       meaninertia nv, what the Newton solver's stop rule (scale |grad| < tolerance, scale = 1 / (meaninertia nv)) promises.
  other dtypes         tests/data_cases.py's TOL[dtype], relative to the array's largest magnitude, against the fp64 stepper."""
import ctypes as C
import os

import numpy as np

import data_cases as dc
import sensor_cases as sc
from helpers import Mem, oracle_for, rel_err
from myochallenge_amd import native

TOL = dc.TOL
HEALTHY = sc.HEALTHY
EPS = 1e-6
KINDS = ("body", "bodycom", "site", "geom", "subtreecom")
POINT_KEY = {"body": "xpos", "bodycom": "xipos", "site": "site_xpos", "geom": "geom_xpos", "subtreecom": "subtree_com"}


# ---------------------------------------------------------------------------------------------------------------- plumbing
def count(b, kind):
    return b.model.size({"site": "nsite", "geom": "ngeom"}.get(kind, "nbody"))


def jac_all(b, mem, kind, ids=None, points=None, want=("jacp", "jacr")):
    """host copies of the Jacobians of every env, {jacp, jacr: [N, k, 3, nv]}; the outputs are pre-filled with NaN and none may survive"""
    ids = np.arange(count(b, kind)) if ids is None else np.asarray(ids)
    want = [w for w in want if not (w == "jacr" and kind == "subtreecom")]
    out = {w: mem.arr(np.full((b.n, len(ids), 3, b.model.size("nv")), np.nan)) for w in want}
    b.jac(kind, mem.arr(ids, np.int32), out.get("jacp"), out.get("jacr"), None if points is None else mem.arr(points))
    res = {w: mem.host(v).copy() for w, v in out.items()}
    for w, v in res.items():
        assert not np.isnan(v).any(), (kind, w)
    return res


def inverse_all(b, mem, qacc, want=("qfrc_inverse", "qfrc_constraint")):
    out = {w: mem.arr(np.full((b.n, b.model.size("nv")), np.nan)) for w in want}
    b.inverse(mem.arr(qacc), out.get("qfrc_inverse"), out.get("qfrc_constraint"))
    res = {w: mem.host(v).copy() for w, v in out.items()}
    for w, v in res.items():
        assert not np.isnan(v).any(), w
    return res


def tree(cm):
    """anc [nbody, nv]: dof i moves body b; sub [nbody, nbody]: body c is in body b's subtree; root [nbody]"""
    f = cm.fields
    par, dof_body = np.asarray(f["body_parentid"]), np.asarray(f["dof_bodyid"])
    nb, nv = len(par), len(dof_body)
    anc, sub = np.zeros((nb, nv), bool), np.zeros((nb, nb), bool)
    for b in range(nb):
        c = b
        while True:
            sub[c, b] = True
            anc[b] |= dof_body == c
            if c == 0:
                break
            c = par[c]
    return anc, sub, np.asarray(f["body_rootid"])


def body_of(cm, kind):
    f = cm.fields
    return np.asarray(f["site_bodyid"] if kind == "site" else f["geom_bodyid"] if kind == "geom" else np.arange(len(f["body_parentid"])))


def integrate(cm, q, d, eps):
    """mj_integratePos in numpy: q [nq] moved by eps * d [nv] (hinge / slide: q += eps d; free joint: pos += eps d[0:3], quat <- quat (x)
    exp(eps d[3:6]), the rotation in the local frame)"""
    f = cm.fields
    q = np.array(q, float)
    for j, ty in enumerate(np.asarray(f["jnt_type"])):
        qa, da = int(f["jnt_qposadr"][j]), int(f["jnt_dofadr"][j])
        if ty == 0:
            q[qa:qa + 3] += eps * d[da:da + 3]
            v = eps * d[da + 3:da + 6]
            a = np.linalg.norm(v)
            w, x, y, z = q[qa + 3:qa + 7]
            rw, (rx, ry, rz) = np.cos(a / 2), (np.sin(a / 2) / a * v if a > 0 else 0 * v)
            q[qa + 3:qa + 7] = [w * rw - x * rx - y * ry - z * rz, w * rx + x * rw + y * rz - z * ry,
                                w * ry - x * rz + y * rw + z * rx, w * rz + x * ry - y * rx + z * rw]
        else:
            assert ty in (2, 3)
            q[qa] += eps * d[da]
    return q


def close(got, ref, tol):
    return np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref))


def stepped(b, mem, nu, nsteps, seed):
    obs, rew, done = mem.zeros((b.n, b.obs_dim), np.float32), mem.zeros(b.n, np.float32), mem.zeros(b.n, np.uint8)
    b.reset(None, obs)
    rng = np.random.RandomState(seed)
    for _ in range(nsteps):
        b.step(mem.arr(np.clip(rng.normal(0, 0.5, (b.n, nu)), -1, 1), np.float32), obs, rew, done)
        assert not mem.host(done).any()
    return b


def die_batch(lib, mem, dtype, n=3, seed=0, nsteps=3, name="CustomMyoReorientP2"):
    from myochallenge_amd.envs.reorient import make_reorient_cfg
    from myochallenge_amd.synth_hand import synthetic_hand_die
    cm, om, _ = oracle_for(synthetic_hand_die())
    b = native.Batch(native.Model(cm, lib), make_reorient_cfg(name, cm, max_episode_steps=200), n, 0, seed, dtype)
    return cm, om, stepped(b, mem, om.nu, nsteps, seed)


def finger_batch(lib, mem, dtype, n=3, seed=3):
    from myochallenge_amd.mjb import load_mjb
    mj = load_mjb(os.path.join(dc.GOLDEN, "myo_finger_v0.mjb"))
    cm, om, _ = oracle_for(mj)
    b = native.Batch(native.Model(cm, lib), None, n, 0, 0, dtype)
    rng = np.random.RandomState(seed)
    b.set_state(mem.arr(np.asarray(mj.qpos0)[None] + rng.uniform(-0.3, 0.3, (n, om.nq))), mem.arr(rng.uniform(-1, 1, (n, om.nv))),
                mem.arr(rng.uniform(0.1, 0.9, (n, om.na))), mem.zeros(n))
    b.physics_step(mem.arr(rng.uniform(0.2, 0.8, (n, om.nu))), 3)
    return cm, om, b


def hand_batch(lib, mem, dtype, n=3, seed=1, nsteps=3):
    cm, om = sc.hand_model()
    return cm, om, sc.baoding_batch(lib, mem, dtype, n, seed, nsteps)


MODELS = {"finger": finger_batch, "hand": hand_batch, "die": die_batch}


# ---------------------------------------------------------------------------------------------------------------- 1. finite differences
def case_finite_differences(lib, which, ndir=6, seed=11):
    """jacp . d and jacr . d of all five kinds and every object against central differences of the pinned poses, 6 dense tangent
    directions per env; each env is perturbed and compared within its own index"""
    mem = Mem(lib)
    cm, om, b = MODELS[which](lib, mem, native.MYO_F64)
    n, nv = b.n, om.nv
    st = sc.device_state(b, mem, om)
    q0 = st[0]
    J = {kind: jac_all(b, mem, kind) for kind in KINDS}
    keys = sorted(set(POINT_KEY.values())) + ["xmat"]
    rng = np.random.RandomState(seed)
    worst = 0.0
    for _ in range(ndir):
        d = rng.uniform(-1, 1, (n, nv))
        d /= np.abs(d).max(1, keepdims=True)
        x = []
        for sg in (+1, -1):
            b.set_state(mem.arr(np.stack([integrate(cm, q0[e], d[e], sg * EPS) for e in range(n)])))
            x.append(dc.data_all(b, mem, keys))
        b.set_state(mem.arr(q0))
        for kind in KINDS:
            fd = (x[0][POINT_KEY[kind]] - x[1][POINT_KEY[kind]]) / (2 * EPS)                  # [N, k, 3]
            got = np.einsum("nkri,ni->nkr", J[kind]["jacp"], d)
            worst = max(worst, float((np.abs(got - fd) / np.maximum(1.0, np.abs(fd))).max()))
            assert close(got, fd, 1e-7).all(), (which, kind, np.abs(got - fd).max())
        Rp, Rm = (v["xmat"].reshape(n, -1, 3, 3) for v in x)
        W = (Rp @ Rm.transpose(0, 1, 3, 2) - Rm @ Rp.transpose(0, 1, 3, 2)) / (4 * EPS)
        fd = np.stack([W[..., 2, 1], W[..., 0, 2], W[..., 1, 0]], -1)
        got = np.einsum("nkri,ni->nkr", J["body"]["jacr"], d)
        worst = max(worst, float((np.abs(got - fd) / np.maximum(1.0, np.abs(fd))).max()))
        assert close(got, fd, 1e-7).all(), (which, "jacr", np.abs(got - fd).max())
    print(f"    {which}: worst |jac.d - fd| / max(1, |fd|) = {worst:.3e}")
    # something moved: the check is not 0 == 0
    assert np.abs(J["site"]["jacp"]).max() > 1e-3 and np.abs(J["body"]["jacr"]).max() > 0.5
    # the rotational block of a body's inertial frame, a site, a geom is its body's
    assert np.array_equal(J["bodycom"]["jacr"], J["body"]["jacr"])
    for kind in ("site", "geom"):
        assert np.array_equal(J[kind]["jacr"], J["body"]["jacr"][:, body_of(cm, kind)]), kind
    # the state is what it was
    assert np.array_equal(sc.device_state(b, mem, om)[0], q0)
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 2. identities
def body_identities(cm, om, b, mem, tol=1e-12):
    """jacr . qvel = cvel[:3]; jacp_body . qvel = cvel[3:] + cvel[:3] x (xpos - subtree_com[root])"""
    _, _, root = tree(cm)
    qvel = sc.device_state(b, mem, om)[1]
    h = dc.data_all(b, mem, ["cvel", "xpos", "subtree_com"])
    J = jac_all(b, mem, "body")
    w, v = h["cvel"][..., :3], h["cvel"][..., 3:]
    assert close(np.einsum("nkri,ni->nkr", J["jacr"], qvel), w, tol).all()
    ref = v + np.cross(w, h["xpos"] - h["subtree_com"][:, root])
    got = np.einsum("nkri,ni->nkr", J["jacp"], qvel)
    assert close(got, ref, tol).all(), np.abs(got - ref).max()
    assert np.abs(ref).max() > 1e-3
    return J


def case_identities(lib):
    mem = Mem(lib)
    cm, om, b = hand_batch(lib, mem, native.MYO_F64)
    body_identities(cm, om, b, mem)
    # subtreecom = the mass-weighted sum of the bodycom Jacobians over the subtree (P1: the compiled model's masses)
    _, sub, _ = tree(cm)
    mass = np.asarray(cm.fields["body_mass"], float)
    Jc, Js = jac_all(b, mem, "bodycom")["jacp"], jac_all(b, mem, "subtreecom")["jacp"]
    ref = np.einsum("bc,nc...->nb...", sub * mass[None, :], Jc) / (sub * mass[None, :]).sum(1)[None, :, None, None]
    assert close(Js, ref, 1e-12).all(), np.abs(Js - ref).max()
    assert np.abs(ref[:, 0]).max() > 1e-3          # the world's subtree is the whole model
    # mj_jac with points = site_xpos on the sites' bodies is kind "site"
    sx = dc.data_all(b, mem, ["site_xpos"])["site_xpos"]
    Jsite = jac_all(b, mem, "site")
    Jpt = jac_all(b, mem, "body", ids=body_of(cm, "site"), points=sx)
    for w in ("jacp", "jacr"):
        assert close(Jpt[w], Jsite[w], 1e-12).all(), w
    assert b.health() == HEALTHY
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3. structure
def case_structure(lib):
    mem = Mem(lib)
    cm, om, b = hand_batch(lib, mem, native.MYO_F64)
    anc, sub, _ = tree(cm)
    nv = om.nv
    full = {kind: jac_all(b, mem, kind) for kind in KINDS}
    for kind in ("body", "bodycom", "site", "geom"):
        off = ~anc[body_of(cm, kind)]                                       # [k, nv]
        for w in ("jacp", "jacr"):
            assert not full[kind][w][:, off[:, None, :].repeat(3, 1)].any(), (kind, w)      # exactly 0.0
    # subtreecom: only dofs that move some body of the subtree
    moved = (sub[:, :, None] & anc[None, :, :]).any(1)
    assert not full["subtreecom"]["jacp"][:, (~moved)[:, None, :].repeat(3, 1)].any()
    names = cm.names
    f = cm.fields
    b1, b2 = names["body"].index("ball1"), names["body"].index("ball2")
    d1, d2 = int(f["body_dofadr"][b1]), int(f["body_dofadr"][b2])
    assert not full["body"]["jacp"][:, b1, :, d2:d2 + 6].any() and np.abs(full["body"]["jacp"][:, b1, :, d1:d1 + 6]).max() == 1.0
    tip = names["body"].index("distph2")
    tip_sites = np.nonzero(body_of(cm, "site") == tip)[0]
    assert len(tip_sites) and not full["site"]["jacp"][:, tip_sites][..., [d1, d1 + 3, d2, d2 + 5]].any()
    assert np.abs(full["site"]["jacp"][:, tip_sites]).max() > 1e-3
    # the world body and what sits on it
    assert not full["body"]["jacp"][:, 0].any() and not full["body"]["jacr"][:, 0].any() and not full["bodycom"]["jacp"][:, 0].any()
    for kind in ("site", "geom"):
        on_world = np.nonzero(body_of(cm, kind) == 0)[0]
        assert not full[kind]["jacp"][:, on_world].any() and not full[kind]["jacr"][:, on_world].any()
    # k = 1; k = all sites (215 x 35 pairs: many 64-lane trips, several staging chunks); repeated, unordered ids
    ns = count(b, "site")
    assert ns * nv > 64 * 64 and ns > 64
    for ids in ([ns - 1], [5, 3, 3, ns - 1, 0, 5] + list(range(40, 0, -1))):
        part = jac_all(b, mem, "site", ids)
        for w in ("jacp", "jacr"):
            assert np.array_equal(part[w], full["site"][w][:, ids]), (ids, w)
    for kind in ("body", "subtreecom"):
        ids = [b2, 0, b1, b1, 3]
        assert np.array_equal(jac_all(b, mem, kind, ids)["jacp"], full[kind]["jacp"][:, ids]), kind
    # one output alone
    for kind in ("body", "geom"):
        assert np.array_equal(jac_all(b, mem, kind, want=("jacp",))["jacp"], full[kind]["jacp"])
        assert np.array_equal(jac_all(b, mem, kind, want=("jacr",))["jacr"], full[kind]["jacr"])
    # an id outside the model: zero blocks (the documented rule), the others what they are
    for kind in KINDS:
        ids = [1, -1, count(b, kind), 2]
        part = jac_all(b, mem, kind, ids)
        for w in part:
            assert not part[w][:, 1:3].any() and np.array_equal(part[w][:, [0, 3]], full[kind][w][:, [1, 2]]), (kind, w)
    b.jac("body", mem.arr([], np.int32), None, None)                       # k = 0, no outputs: nothing to do, no error
    assert b.health() == HEALTHY
    b.close()
    # the die's `target` goal body, its sites and geoms: no dof above them
    cm, om, b = die_batch(lib, mem, native.MYO_F64)
    tb = cm.names["body"].index("target")
    assert int(cm.fields["body_parentid"][tb]) == 0 and int(cm.fields["body_dofnum"][tb]) == 0
    for kind in ("body", "bodycom", "site", "geom"):
        on = np.nonzero(body_of(cm, kind) == tb)[0]
        assert len(on)
        J = jac_all(b, mem, kind)
        assert not J["jacp"][:, on].any() and not J["jacr"][:, on].any() and J["jacp"].any(), kind
    assert not jac_all(b, mem, "subtreecom")["jacp"][:, tb].any()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. forward / inverse
def forward_inverse(b, mem, label):
    """inverse(data.qacc) against the forward pass's own forces; returns (|r|_inf, |qfrc_inverse - qfrc_actuator|_inf) per env"""
    h = dc.data_all(b, mem, ["qacc", "qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator"])
    fc = sc.sense_all(b, mem, ["qfrc_constraint"])["qfrc_constraint"]
    inv = inverse_all(b, mem, h["qacc"])
    r = np.einsum("nij,nj->ni", h["qM"], h["qacc"]) + h["qfrc_bias"] - h["qfrc_passive"] - h["qfrc_actuator"] - fc
    rn = np.abs(r).max(1)
    dn = np.abs(inv["qfrc_inverse"] - h["qfrc_actuator"]).max(1)
    cn = np.abs(inv["qfrc_constraint"] - fc).max(1)
    scale = np.max([np.abs(h[k]).max(1) for k in ("qfrc_bias", "qfrc_passive", "qfrc_actuator")] + [np.abs(fc).max(1)], 0)
    for e in range(b.n):
        print(f"    {label} env {e}: |r| {rn[e]:.3e}  |qfrc_inverse - qfrc_actuator| {dn[e]:.3e}  |dqfrc_constraint| {cn[e]:.3e}  scale {scale[e]:.3e}")
    opt = np.asarray(b.model.compiled.fields["opt_f64"], float)          # timestep, tolerance, ..., meaninertia
    stop = opt[1] * opt[7] * b.model.size("nv")
    assert (np.linalg.norm(r, axis=1) <= stop).all(), (label, np.linalg.norm(r, axis=1), stop)
    bound = 4 * rn + 1e-10 * scale
    assert (dn <= bound).all(), (label, dn, bound)
    assert (cn <= bound).all(), (label, cn, bound)
    return rn, dn, fc


def case_forward_inverse(lib, seed=1):
    """Baoding P1, reset + 3 random steps of seed 1: every env has the balls on the palm (ncon >= 2); then the die"""
    mem = Mem(lib)
    cm, om, b = hand_batch(lib, mem, native.MYO_F64, 3, seed, 3)
    ncon = dc.sensed_ncon(b, mem)
    assert (ncon >= 2).all(), ncon
    _, _, fc = forward_inverse(b, mem, "baoding")
    assert np.abs(fc).max(1).min() > 1e-3          # the constraint forces are there
    assert b.health() == HEALTHY
    b.close()
    cm, om, b = die_batch(lib, mem, native.MYO_F64)
    print("    die ncon", dc.sensed_ncon(b, mem))
    forward_inverse(b, mem, "die")
    assert b.health() == HEALTHY
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. no constraints
def case_inverse_unconstrained(lib, n=3, seed=7):
    """the joint-pose hand at mid-range: no colliding pair, no friction loss, no limit within its margin"""
    from myochallenge_amd.envs.pose import make_pose_cfg
    from myochallenge_amd.synth_hand import synthetic_hand_pose
    mem = Mem(lib)
    cm, om, _ = oracle_for(synthetic_hand_pose())
    f = cm.fields
    assert not np.asarray(f["dof_frictionloss"]).any() and not np.asarray(f["tendon_frictionloss"]).any()
    b = native.Batch(native.Model(cm, lib), make_pose_cfg("CustomMyoHandPoseRandom", cm), n, 0, 3, native.MYO_F64)
    stepped(b, mem, om.nu, 1, seed)
    rng = np.random.RandomState(seed)
    q = np.tile(np.asarray(f["qpos0"], float), (n, 1))
    rg = np.asarray(f["jnt_range"], float).reshape(-1, 2)
    for j in range(len(f["jnt_type"])):
        if int(f["jnt_limited"][j]):
            q[:, int(f["jnt_qposadr"][j])] = rg[j].mean()
    b.set_state(mem.arr(q), mem.arr(rng.uniform(-0.5, 0.5, (n, om.nv))))
    assert not sc.sense_all(b, mem, ["qfrc_constraint"])["qfrc_constraint"].any()      # else the case proves nothing
    h = dc.data_all(b, mem, ["qM", "qfrc_bias", "qfrc_passive"])
    for _ in range(3):
        qacc = rng.normal(0, 10, (n, om.nv))
        inv = inverse_all(b, mem, qacc)
        ref = np.einsum("nij,nj->ni", h["qM"], qacc) + h["qfrc_bias"] - h["qfrc_passive"]
        assert rel_err(inv["qfrc_inverse"], ref) < 1e-12, rel_err(inv["qfrc_inverse"], ref)
        assert not inv["qfrc_constraint"].any()
    # one output alone
    one = inverse_all(b, mem, qacc, want=("qfrc_inverse",))
    assert np.array_equal(one["qfrc_inverse"], inv["qfrc_inverse"])
    assert b.health() == HEALTHY
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 6. other dtypes
def copy_env_state(src, dst, mem, om, nd=9):
    st = sc.device_state(src, mem, om)
    dst.set_state(*[mem.arr(x) for x in st[:4]])
    dst.warmstart(None, mem.arr(st[4]))
    ti, td, bd = dc.task_arrays(src, mem, nd)
    dst.set_task(mem.arr(ti, np.int32), mem.arr(td), mem.arr(bd))


def case_dtype(lib, dtype, which):
    """a batch of another arithmetic at the fp64 batch's state: jac and inverse within data_cases' TOL[dtype] of the fp64 results"""
    mem = Mem(lib)
    cm, om, ref = MODELS[which](lib, mem, native.MYO_F64)
    _, _, b = MODELS[which](lib, mem, dtype)
    if which == "finger":
        st = sc.device_state(ref, mem, om)
        b.set_state(*[mem.arr(x) for x in st[:4]])
    else:
        copy_env_state(ref, b, mem, om)
    tol = TOL[dtype]
    for kind in KINDS:
        a, r = jac_all(b, mem, kind), jac_all(ref, mem, kind)
        for w in r:
            err = rel_err(a[w], r[w])
            print(f"    {which} {kind} {w}: rel_err {err:.3e}")
            assert err < tol, (kind, w, err)
            assert np.array_equal(a[w] == 0, r[w] == 0) or dtype != native.MYO_F64
    qacc = dc.data_all(ref, mem, ["qacc"])["qacc"]
    a, r = inverse_all(b, mem, qacc), inverse_all(ref, mem, qacc)
    for w in r:
        if np.abs(r[w]).max() > 0:
            err = rel_err(a[w], r[w])
            print(f"    {which} {w}: rel_err {err:.3e}")
            assert err < tol, (w, err)
        else:
            assert not a[w].any(), w
    b.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------- 7. read-only
def _run(lib, mem, dtype, n, seed, nsteps, read_between):
    cm, om = sc.hand_model()
    from myochallenge_amd.envs.config import make_task_cfg
    b = native.Batch(native.Model(cm, lib), make_task_cfg("CustomMyoBaodingBallsP2", cm), n, 0, seed, dtype)
    obs, rew, done = mem.zeros((n, b.obs_dim), np.float32), mem.zeros(n, np.float32), mem.zeros(n, np.uint8)
    b.reset(None, obs)
    rng, rng_q = np.random.RandomState(seed), np.random.RandomState(seed + 1)
    trace = []
    for i in range(nsteps):
        if read_between and i >= nsteps - 5:
            before = (dc.data_all(b, mem), sc.sense_all(b, mem))
            for kind in KINDS:
                jac_all(b, mem, kind)
            inverse_all(b, mem, rng_q.normal(0, 10, (n, om.nv)) if i % 2 else before[0]["qacc"])
            after = (dc.data_all(b, mem), sc.sense_all(b, mem))
            for x, y in zip(before, after):
                for k in x:
                    assert np.array_equal(x[k], y[k]), k
        b.step(mem.arr(np.clip(rng.normal(0, 0.5, (n, om.nu)), -1, 1), np.float32), obs, rew, done)
        trace.append([mem.host(x).copy() for x in (obs, rew, done)])
    return b, trace


def case_read_only(lib, dtype, n=3, seed=5, nsteps=8):
    """two batches of one seed; one calls jac (all kinds) and inverse before each of the last 5 steps, the other never: states,
    observations and health are the same bits, and data() / sensors() around the calls do not move"""
    mem = Mem(lib)
    _, om = sc.hand_model()
    a, ta = _run(lib, mem, dtype, n, seed, nsteps, True)
    b, tb = _run(lib, mem, dtype, n, seed, nsteps, False)
    for x, y in zip(sc.device_state(a, mem, om) + list(dc.task_arrays(a, mem)), sc.device_state(b, mem, om) + list(dc.task_arrays(b, mem))):
        assert np.array_equal(x, y)
    for sa, sb in zip(ta, tb):
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)
    assert a.health() == b.health() == HEALTHY
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 8. edges
def case_batch_sizes(lib, dtype=native.MYO_F64):
    """N = 1, 63 and 65: the body identities and the forward / inverse bound on every env"""
    mem = Mem(lib)
    for n in (1, 63, 65):
        cm, om, b = hand_batch(lib, mem, dtype, n, 2, 2)
        body_identities(cm, om, b, mem)
        h = dc.data_all(b, mem, ["qacc", "qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator"])
        fc = sc.sense_all(b, mem, ["qfrc_constraint"])["qfrc_constraint"]
        inv = inverse_all(b, mem, h["qacc"])
        r = np.einsum("nij,nj->ni", h["qM"], h["qacc"]) + h["qfrc_bias"] - h["qfrc_passive"] - h["qfrc_actuator"] - fc
        scale = np.max([np.abs(h[k]).max(1) for k in ("qfrc_bias", "qfrc_passive", "qfrc_actuator")] + [np.abs(fc).max(1)], 0)
        assert (np.abs(inv["qfrc_inverse"] - h["qfrc_actuator"]).max(1) <= 4 * np.abs(r).max(1) + 1e-10 * scale).all(), n
        b.close()


def case_bad_args(lib):
    """struct sizes of another version, NULLs and argument combinations that do not exist are refused before any device call
    (MYO_E_BADARG = MYO_E_ARG = -1): the NaN-filled outputs stay untouched"""
    mem = Mem(lib)
    b = sc.baoding_batch(lib, mem, native.MYO_MIXED, 1, 0, 0)
    nv, L = b.model.size("nv"), lib.L
    ids, jp, jr = mem.arr([1, 2], np.int32), mem.arr(np.full((1, 2, 3, nv), np.nan)), mem.arr(np.full((1, 2, 3, nv), np.nan))
    pts = mem.zeros((1, 2, 3))
    P = native._ptr
    out = native.JacOut()
    out.jacp, out.jacr = P(jp), P(jr)
    assert C.sizeof(native.JacOut) == 24 and C.sizeof(native.InverseOut) == 24
    for size in (0, 16, 32):
        out.size = size
        assert L.myo_batch_jac(b.h, 0, P(ids), 2, None, C.byref(out), None) == -1 and b"size" in L.myo_last_error()
    out.size = 24
    assert L.myo_batch_jac(None, 0, P(ids), 2, None, C.byref(out), None) == -1
    assert L.myo_batch_jac(b.h, 0, P(ids), 2, None, None, None) == -1
    assert L.myo_batch_jac(b.h, 0, None, 2, None, C.byref(out), None) == -1
    assert L.myo_batch_jac(b.h, 0, P(ids), -1, None, C.byref(out), None) == -1
    assert L.myo_batch_jac(b.h, 5, P(ids), 2, None, C.byref(out), None) == -1 and L.myo_batch_jac(b.h, -1, P(ids), 2, None, C.byref(out), None) == -1
    assert L.myo_batch_jac(b.h, native.JAC_SUBTREECOM, P(ids), 2, None, C.byref(out), None) == -1 and b"jacr" in L.myo_last_error()
    for kind in (native.JAC_BODYCOM, native.JAC_SITE, native.JAC_GEOM, native.JAC_SUBTREECOM):
        assert L.myo_batch_jac(b.h, kind, P(ids), 2, P(pts), C.byref(out), None) == -1
    assert np.isnan(mem.host(jp)).all() and np.isnan(mem.host(jr)).all()
    none = native.JacOut()
    none.size = 24
    assert L.myo_batch_jac(b.h, 0, P(ids), 2, None, C.byref(none), None) == 0          # both NULL: a no-op
    assert L.myo_batch_jac(b.h, 0, P(ids), 2, P(pts), C.byref(out), None) == 0 and not np.isnan(mem.host(jp)).any()
    qacc, fi = mem.zeros((1, nv)), mem.arr(np.full((1, nv), np.nan))
    io = native.InverseOut()
    io.qfrc_inverse = P(fi)
    for size in (0, 16, 32):
        io.size = size
        assert L.myo_batch_inverse(b.h, P(qacc), C.byref(io), None) == -1 and b"size" in L.myo_last_error()
    io.size = 24
    assert L.myo_batch_inverse(None, P(qacc), C.byref(io), None) == -1
    assert L.myo_batch_inverse(b.h, P(qacc), None, None) == -1
    assert L.myo_batch_inverse(b.h, None, C.byref(io), None) == -1 and b"qacc" in L.myo_last_error()
    assert np.isnan(mem.host(fi)).all()
    nio = native.InverseOut()
    nio.size = 24
    assert L.myo_batch_inverse(b.h, P(qacc), C.byref(nio), None) == 0                   # both NULL: a no-op
    assert L.myo_batch_inverse(b.h, P(qacc), C.byref(io), None) == 0 and not np.isnan(mem.host(fi)).any()
    with np.testing.assert_raises(KeyError):
        b.jac("no_such_kind", ids, jp, jr)
    assert b.health() == HEALTHY
    b.close()
