"""Read-only open-loop simulation (myo_batch_simulate; BaodingVecEnv.simulate / linearize): every case of tests/simulate_cases.py on the
lane-serial emulation (CPU) and on the HIP kernels (-m gpu), then the Python surface and the finite-difference linearisation."""
import numpy as np
import pytest

import simulate_cases as sim
from helpers import make_env
from myochallenge_amd import native

F64, MIXED = native.MYO_F64, native.MYO_MIXED
DTYPES = [pytest.param(F64, id="f64"), pytest.param(MIXED, id="mixed")]
# (dtype, model, integrator): the fp64 and the mixed stepper, Euler and RK4, the Baoding hand and the die (the 48-slot variant, whose
# activations and object friction live in the record)
VARIANTS = [pytest.param(F64, "hand", None, id="f64-hand-euler"), pytest.param(MIXED, "hand", None, id="mixed-hand-euler"),
            pytest.param(F64, "hand", 1, id="f64-hand-rk4"), pytest.param(MIXED, "hand", 1, id="mixed-hand-rk4"),
            pytest.param(F64, "die", None, id="f64-die-euler"), pytest.param(MIXED, "die", None, id="mixed-die-euler")]
ORACLE = [pytest.param(F64, "hand", None, id="f64-hand-euler"), pytest.param(MIXED, "hand", None, id="mixed-hand-euler"),
          pytest.param(F64, "hand", 1, id="f64-hand-rk4"), pytest.param(F64, "die", None, id="f64-die-euler")]


# ---------------------------------------------------------------------------------------------------------------- emulation (CPU)
@pytest.mark.parametrize("dtype,which,integrator", VARIANTS)
def test_composed_path_on_emulation(emu_lib, dtype, which, integrator):
    sim.case_composed(emu_lib, dtype, which, integrator)


def test_composed_path_without_start_states_on_emulation(emu_lib):
    sim.case_composed(emu_lib, F64, "hand", None, override=False)


@pytest.mark.parametrize("dtype,which,integrator", ORACLE)
def test_oracle_on_emulation(emu_lib, dtype, which, integrator):
    sim.case_oracle(emu_lib, dtype, which, integrator)


@pytest.mark.parametrize("which", ["hand", "die"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_read_only_on_emulation(emu_lib, dtype, which):
    sim.case_read_only(emu_lib, dtype, which)


@pytest.mark.parametrize("dtype", DTYPES)
def test_independence_on_emulation(emu_lib, dtype):
    sim.case_independence(emu_lib, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_blow_up_on_emulation(emu_lib, dtype):
    sim.case_blow_up(emu_lib, dtype)


def test_bad_args_on_emulation(emu_lib):
    sim.case_bad_args(emu_lib)


# ---------------------------------------------------------------------------------------------------------------- HIP (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,which,integrator", VARIANTS)
def test_composed_path_on_gpu(hip_lib, dtype, which, integrator):
    sim.case_composed(hip_lib, dtype, which, integrator)


@pytest.mark.gpu
def test_composed_path_without_start_states_on_gpu(hip_lib):
    sim.case_composed(hip_lib, F64, "hand", None, override=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,which,integrator", ORACLE)
def test_oracle_on_gpu(hip_lib, dtype, which, integrator):
    sim.case_oracle(hip_lib, dtype, which, integrator)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hand", "die"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_read_only_on_gpu(hip_lib, dtype, which):
    sim.case_read_only(hip_lib, dtype, which)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,integrator", [pytest.param(F64, None, id="f64"), pytest.param(MIXED, None, id="mixed"), pytest.param(F64, 1, id="f64-rk4")])
def test_independence_on_gpu(hip_lib, dtype, integrator):
    sim.case_independence(hip_lib, dtype, integrator)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_blow_up_on_gpu(hip_lib, dtype):
    sim.case_blow_up(hip_lib, dtype)


@pytest.mark.gpu
def test_bad_args_on_gpu(hip_lib):
    sim.case_bad_args(hip_lib)


@pytest.mark.gpu
def test_large_call_on_gpu(hip_lib):
    sim.case_large(hip_lib)


@pytest.mark.gpu
def test_captured_call_on_gpu(hip_lib):
    sim.case_graph(hip_lib)


# ---------------------------------------------------------------------------------------------------------------- Python surface
def case_python_surface(lib):
    import torch
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    env = make_env("CustomMyoBaodingBallsP1", lib, num_envs=3, seed=1, dtype="f64")
    env.reset()
    n, m = env.num_envs, env._model
    nq, nv, na, nu = m.size("nq"), m.size("nv"), m.size("na"), env.act_dim
    rng = np.random.RandomState(0)
    ctrl = rng.uniform(0, 1, (3, 3, 4, nu))
    before = [x.clone() for x in env.get_state()]
    sites = ["ball1_site", env.site_names().index("target1_site")]
    out = env.simulate(ctrl, nsub=2, every=2, sites=sites, indices=[2, 0, 2])
    assert set(out) == set(native.SIM_KEYS)
    shapes = {"qpos": (3, 3, 2, nq), "qvel": (3, 3, 2, nv), "act": (3, 3, 2, na), "time": (3, 3, 2), "site_xpos": (3, 3, 2, 2, 3), "bad": (3, 3), "steps": (3, 3)}
    for key, v in out.items():
        assert tuple(v.shape) == shapes[key] and v.device == env.device, key
        assert v.dtype == (torch.int32 if key in ("bad", "steps") else torch.float64), key
    assert bool((out["bad"] == 0).all()) and bool((out["steps"] == 4).all()) and bool(torch.isfinite(out["qpos"]).all())
    for x, y in zip(before, env.get_state()):      # the envs did not move
        assert torch.equal(x, y)
    # the C ABI's cases run on this route too: the same bits as the batch-level call of simulate_cases
    mem = sim.Mem(lib)
    st = type("S", (), {"b": env.batch, "mem": mem})
    raw = sim.simulate_all(st, [2, 0, 2], ctrl=ctrl, sites=[env.site_names().index(s) if isinstance(s, str) else s for s in sites])
    for key in out:
        assert np.array_equal(raw[key], out[key].cpu().numpy()), key
    # rank 3 is shared by the samples; samples must agree with a rank-4 ctrl; numpy and tensors are both accepted
    shared = env.simulate(ctrl[:, 0], samples=3, nsub=2, every=2, indices=[2, 0, 2], keys=["qpos"])
    tiled = env.simulate(torch.as_tensor(np.repeat(ctrl[:, :1], 3, 1)), nsub=2, every=2, indices=[2, 0, 2], keys=["qpos", "bad"])
    assert set(shared) == {"qpos"} and set(tiled) == {"qpos", "bad"} and torch.equal(shared["qpos"], tiled["qpos"])
    # all envs by default, the task's frame_skip by default, start states given
    q0 = before[0][:, None].repeat(1, 2, 1)
    every = env.simulate(ctrl[:, :2, :2], qpos=q0, qvel=torch.zeros((n, 2, nv), dtype=torch.float64), act=np.full((n, 2, na), 0.25))
    named = env.simulate(ctrl[:, :2, :2], nsub=int(env._cfg.frame_skip), qpos=q0, qvel=np.zeros((n, 2, nv)), act=np.full((n, 2, na), 0.25), indices=[0, 1, 2])
    assert "site_xpos" not in every and tuple(every["qpos"].shape) == (n, 2, 2, nq)
    for key in every:
        assert torch.equal(every[key], named[key]), key
    # refusals, each with its text
    for kw, exc, text in ((dict(indices=[0, 3]), IndexError, "env index 3 outside [0, 3)"), (dict(indices=[-1]), IndexError, "env index -1"),
                          (dict(sites=["no_such_site"]), KeyError, "unknown site name"), (dict(sites=[len(env.site_names())]), KeyError, "site id"),
                          (dict(sites=[0] * (native.SIM_NS_MAX + 1)), ValueError, "at most 16 sites"), (dict(every=3), ValueError, "divide the number of control steps"),
                          (dict(every=0), ValueError, "every must be >= 1"), (dict(samples=2), ValueError, "samples = 2"), (dict(nsub=0), ValueError, "nsub"),
                          (dict(keys=["no_such_key"]), KeyError, "unknown simulation key"), (dict(qpos=np.zeros((n, 3, nq + 1))), ValueError, "qpos must have shape"),
                          (dict(qvel=np.zeros((n, 2, nv))), ValueError, "qvel must have shape"), (dict(act=np.zeros((n, na))), ValueError, "act must have shape")):
        with pytest.raises(exc) as ei:
            env.simulate(ctrl, **kw) if "indices" not in kw else env.simulate(ctrl[:len(kw["indices"])], **kw)
        assert text in str(ei.value), (kw, str(ei.value))
    for bad in (ctrl[:2], ctrl[..., :-1], ctrl[0, 0, 0]):
        with pytest.raises(ValueError):
            env.simulate(bad)
    # VecNormalize forwards both
    vn = VecNormalize(env)
    assert torch.equal(vn.simulate(ctrl, nsub=2, every=2, indices=[2, 0, 2], keys=["qvel"])["qvel"], out["qvel"])
    lin = vn.linearize(nsub=1, indices=[1])
    assert tuple(lin["A"].shape) == (1, 2 * nv + na, 2 * nv + na) and tuple(lin["B"].shape) == (1, 2 * nv + na, nu) and tuple(lin["x_next"].shape) == (1, nq + nv + na)
    for x, y in zip(before, env.get_state()):
        assert torch.equal(x, y)
    env.close()


def test_python_surface_on_emulation(emu_lib):
    case_python_surface(emu_lib)


@pytest.mark.gpu
def test_python_surface_on_gpu(hip_lib):
    case_python_surface(hip_lib)


def _pose_env(lib, n=2):
    from helpers import _on_cpu
    from myochallenge_amd.envs.pose import PoseVecEnv
    return (_on_cpu(PoseVecEnv) if lib.is_emulation else PoseVecEnv)("CustomMyoHandPoseRandom", n, {}, lib=lib, seed=1, dtype="f64")


def case_inherited(lib):
    import torch
    die = make_env("CustomMyoReorientP1", lib, num_envs=2, seed=1)
    die.reset()
    before = [x.clone() for x in die.get_state()]
    out = die.simulate(np.full((2, 2, die.act_dim), 0.3), samples=2, nsub=1, sites=[0])
    assert tuple(out["qpos"].shape) == (2, 2, 2, die._model.size("nq")) and bool((out["bad"] == 0).all()) and bool(torch.isfinite(out["site_xpos"]).all())
    assert torch.equal(out["qpos"][:, 0], out["qpos"][:, 1])
    for x, y in zip(before, die.get_state()):
        assert torch.equal(x, y)
    die.close()
    pose = _pose_env(lib)
    pose.reset()
    out = pose.simulate(np.full((2, 3, pose.act_dim), 0.3), every=3)
    assert tuple(out["qvel"].shape) == (2, 1, 1, pose._model.size("nv")) and bool((out["steps"] == 3).all())
    pose.close()


def test_inherited_by_die_and_pose_envs_on_emulation(emu_lib):
    case_inherited(emu_lib)


@pytest.mark.gpu
def test_inherited_by_die_and_pose_envs_on_gpu(hip_lib):
    case_inherited(hip_lib)


# ---------------------------------------------------------------------------------------------------------------- 7. linearize
def test_tangent_space_helpers():
    """integrate_pos / differentiate_pos (torch) are inverse to each other on hinge, slide, ball and free joints, rotate a free joint's
    quaternion by the LOCAL-frame rotation vector, and agree with the numpy restatement the oracle recipe uses"""
    import torch
    from myochallenge_amd.mathutil import differentiate_pos, integrate_pos
    tabs = (np.array([3, 0, 2, 1]), np.array([0, 1, 8, 9]), np.array([0, 1, 7, 8]))
    rng = np.random.RandomState(0)
    q = rng.normal(size=(5, 13))
    q[:, 4:8] /= np.linalg.norm(q[:, 4:8], axis=1, keepdims=True)
    q[:, 9:13] /= np.linalg.norm(q[:, 9:13], axis=1, keepdims=True)
    dq = rng.uniform(-0.5, 0.5, (5, 11))
    q1 = integrate_pos(torch.as_tensor(q), torch.as_tensor(dq), *tabs)
    assert np.abs(q1.numpy() - sim_np_integrate(q, dq, *tabs)).max() < 1e-15
    back = differentiate_pos(q1, torch.as_tensor(q), *tabs)
    assert np.abs(back.numpy() - dq).max() < 1e-14 and np.abs(sim_np_differentiate(q1.numpy(), q, *tabs) - dq).max() < 1e-14
    assert np.abs(np.linalg.norm(q1.numpy()[:, 4:8], axis=1) - 1).max() < 1e-15
    # local frame: a quarter turn about x, then a rotation vector along z, is a turn about the body's z = the world's -y... checked as q * dq
    qx = np.zeros((1, 13)); qx[0, 4], qx[0, 5], qx[0, 9] = np.cos(np.pi / 4), np.sin(np.pi / 4), 1
    dz = np.zeros((1, 11)); dz[0, 6] = 0.2
    got = integrate_pos(torch.as_tensor(qx), torch.as_tensor(dz), *tabs).numpy()[0, 4:8]
    from myochallenge_amd.mathutil import quat_mul
    assert np.abs(got - quat_mul(qx[0, 4:8], [np.cos(0.1), 0, 0, np.sin(0.1)])).max() < 1e-15
    zero = integrate_pos(torch.as_tensor(q), torch.zeros((5, 11), dtype=torch.float64), *tabs)
    assert np.abs(zero.numpy() - q).max() < 1e-15 and not differentiate_pos(torch.as_tensor(q), torch.as_tensor(q), *tabs).abs().max() > 1e-15


def _np_quat_mul(a, b):
    return np.stack([a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2],
                     a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1],
                     a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]], -1)


def sim_np_integrate(q, dq, jt, qadr, dadr):
    """mj_integratePos with dt = 1 (numpy)"""
    out = np.array(q, float)

    def rot(qq, w):
        ang = np.linalg.norm(w, axis=-1, keepdims=True)
        ax = w / np.where(ang > 0, ang, 1.0)
        r = _np_quat_mul(qq, np.concatenate([np.cos(ang / 2), ax * np.sin(ang / 2)], -1))
        r = np.where(ang > 0, r, qq)
        return r / np.linalg.norm(r, axis=-1, keepdims=True)
    for ty, qa, da in zip(jt, qadr, dadr):
        if ty == 0:
            out[..., qa:qa + 3] = q[..., qa:qa + 3] + dq[..., da:da + 3]
            out[..., qa + 3:qa + 7] = rot(q[..., qa + 3:qa + 7], dq[..., da + 3:da + 6])
        elif ty == 1:
            out[..., qa:qa + 4] = rot(q[..., qa:qa + 4], dq[..., da:da + 3])
        else:
            out[..., qa] = q[..., qa] + dq[..., da]
    return out


def sim_np_differentiate(q1, q0, jt, qadr, dadr):
    """mj_differentiatePos with dt = 1 (numpy): the tangent vector from q0 to q1"""
    nv = max(int(da) + (6 if ty == 0 else 3 if ty == 1 else 1) for ty, da in zip(jt, dadr))
    out = np.zeros(np.shape(q1)[:-1] + (nv,))

    def sub(qb, qa):
        d = _np_quat_mul(qa * np.array([1.0, -1, -1, -1]), qb)
        s = np.linalg.norm(d[..., 1:], axis=-1, keepdims=True)
        ang = 2 * np.arctan2(s, d[..., :1])
        ang = np.where(ang > np.pi, ang - 2 * np.pi, ang)
        return d[..., 1:] / np.where(s > 0, s, 1.0) * ang
    for ty, qa, da in zip(jt, qadr, dadr):
        if ty == 0:
            out[..., da:da + 3] = q1[..., qa:qa + 3] - q0[..., qa:qa + 3]
            out[..., da + 3:da + 6] = sub(q1[..., qa + 3:qa + 7], q0[..., qa + 3:qa + 7])
        elif ty == 1:
            out[..., da:da + 3] = sub(q1[..., qa:qa + 4], q0[..., qa:qa + 4])
        else:
            out[..., da] = q1[..., qa] - q0[..., qa]
    return out


class _OracleStep:
    """one control step of the oracle from a state of env e: x = (qpos, qvel, act), u -> x' (the env's warm start, time and parameters)"""

    def __init__(self, env, om, prepare, nsub):
        from oracle.oracle import OracleData
        self.om, self.nsub, self.prepare = om, nsub, prepare
        self.d = OracleData(om)
        mem = sim.Mem(env.batch.lib)
        self.state = sim.sc.device_state(env.batch, mem, om)
        f = env.compiled.fields
        self.tabs = tuple(np.asarray(f[key]).astype(int) for key in ("jnt_type", "jnt_qposadr", "jnt_dofadr"))

    def __call__(self, e, q, v, a, u):
        d = self.d
        d.reset()
        d.qpos[:], d.qvel[:], d.act[:] = q, v, a
        d.arr("time")[0] = self.state[3][e]
        d.arr("qacc_warmstart")[:] = self.state[4][e]
        if self.prepare is not None:
            self.prepare(e)(d)
        d.ctrl[:] = u
        for _ in range(self.nsub):
            d.step()
        return np.array(d.qpos), np.array(d.qvel), np.array(d.act)

    def tangent(self, hi, lo):
        return np.concatenate([sim_np_differentiate(hi[0], lo[0], *self.tabs), hi[1] - lo[1], hi[2] - lo[2]])

    def linearize(self, e, u, eps):
        """the recipe of BaodingVecEnv.linearize (centred) restated in numpy over oracle steps: A [nx, nx], B [nx, nu], x'"""
        q, v, a = (self.state[i][e] for i in range(3))
        nv, na, nu = len(v), len(a), len(u)
        nx = 2 * nv + na
        J = np.zeros((nx, nx + nu))
        for i in range(nx + nu):
            ends = []
            for sg in (1.0, -1.0):
                d = np.zeros(nx + nu)
                d[i] = sg * eps
                ends.append(self(e, sim_np_integrate(q, d[:nv], *self.tabs), v + d[nv:2 * nv], a + d[2 * nv:nx], u + d[nx:]))
            J[:, i] = self.tangent(ends[0], ends[1]) / (2 * eps)
        return J[:, :nx], J[:, nx:], self(e, q, v, a, u)


def _interior_state(env, seed=0):
    """a state away from every kink of the step: joints mid-range, small velocities, activations and controls inside (0, 1)"""
    f = env.compiled.fields
    rng = np.random.RandomState(seed)
    n, m = env.num_envs, env._model
    jt, qadr = np.asarray(f["jnt_type"]), np.asarray(f["jnt_qposadr"]).astype(int)
    lim, rg = np.asarray(f["jnt_limited"]), np.asarray(f["jnt_range"], float).reshape(-1, 2)
    q = env.get_state()[0].cpu().numpy().copy()
    for j in range(len(jt)):
        if jt[j] in (2, 3):
            mid, half = (rg[j].mean(), 0.1 * (rg[j, 1] - rg[j, 0])) if lim[j] else (0.0, 0.1)
            q[:, qadr[j]] = mid + rng.uniform(-half, half, n)
    env.set_state(q, rng.uniform(-0.05, 0.05, (n, m.size("nv"))), rng.uniform(0.3, 0.7, (n, m.size("na"))))
    return rng.uniform(0.3, 0.7, (n, env.act_dim))


EPS_FD = 1e-6


def case_linearize_parity(lib, which):
    """7a. A and B against the numpy restatement of the same recipe over oracle steps, same eps.  The bound is derived: one step of
    the fp64 stepper matches the oracle's within delta = 1e-9 max(1, |x'|_inf) (parity_cases' bound); a centred difference takes two
    such values and divides their difference by 2 eps, so an entry may differ by delta / eps."""
    from helpers import oracle_for
    if which == "pose":
        from myochallenge_amd.synth_hand import synthetic_hand_pose
        env = _pose_env(lib)
        env.reset()
        _, om, _ = oracle_for(synthetic_hand_pose())
        assert om.nv == 23
        u = _interior_state(env)
        prepare = None
    else:      # the Baoding hand, the balls resting in the palm: contacts in the step
        from myochallenge_amd.envs.config import task_ids
        from oracle.oracle import make_cfg
        env = make_env("CustomMyoBaodingBallsP1", lib, num_envs=2, seed=1, dtype="f64")
        env.reset()
        for _ in range(3):
            env.step(np.zeros((2, env.act_dim), np.float32))
        _, om = sim.sc.hand_model()
        u = np.random.RandomState(1).uniform(0.3, 0.7, (2, env.act_dim))
        task = sim.dc.task_arrays(env.batch, sim.Mem(lib))
        ocfg = make_cfg(task_ids(env.compiled))
        prepare = lambda e: sim.dc.baoding_prepare(ocfg, task[1][e], task[2][e])
        ncon = env.sensors(["ncon"])["ncon"].cpu().numpy()
        assert (ncon >= 2).all(), ncon
    lin = env.linearize(ctrl=u, eps=EPS_FD, nsub=1)
    assert not bool(lin["bad"].any())
    orc = _OracleStep(env, om, prepare, 1)
    worst = 0.0
    for e in range(env.num_envs):
        A, B, xn = orc.linearize(e, u[e], EPS_FD)
        xn = np.concatenate(xn)
        assert np.abs(lin["x_next"][e].cpu().numpy() - xn).max() <= 1e-9 * max(1.0, np.abs(xn).max())
        bound = 1e-9 * max(1.0, np.abs(xn).max()) / EPS_FD
        dA, dB = np.abs(lin["A"][e].cpu().numpy() - A).max(), np.abs(lin["B"][e].cpu().numpy() - B).max()
        print(f"    {which} env {e}: max |A - A_oracle| = {dA:.3e}, max |B - B_oracle| = {dB:.3e} (bound {bound:.3e}; |A|_max {np.abs(A).max():.3e}, |B|_max {np.abs(B).max():.3e})")
        worst = max(worst, dA, dB)
        assert dA <= bound and dB <= bound, (which, e, dA, dB, bound)
        assert np.abs(A).max() > 0.5 and np.abs(B).max() > 0      # (not a comparison of zeros: dq'/dq is near the identity)
    env.close()
    return worst


@pytest.mark.parametrize("which", ["pose", "baoding"])
def test_linearize_against_oracle_recipe_on_emulation(emu_lib, which):
    case_linearize_parity(emu_lib, which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["pose", "baoding"])
def test_linearize_against_oracle_recipe_on_gpu(hip_lib, which):
    case_linearize_parity(hip_lib, which)


def case_linearize_second_order(lib):
    """7b. on the pose hand, x'(x + dx, u + du) - x' - A dx - B du shrinks about 4x when the perturbation halves: the median ratio
    over 8 draws of size 1e-4 lies in [3, 5].  The draws are the first 8 of 24 seeded candidates for which the oracle recipe itself
    (oracle steps, the oracle's A and B) stays inside that band — chosen on the CPU, before the device is asked."""
    import torch
    from helpers import oracle_for
    from myochallenge_amd.mathutil import differentiate_pos, integrate_pos
    from myochallenge_amd.synth_hand import synthetic_hand_pose
    env = _pose_env(lib, 1)
    env.reset()
    _, om, _ = oracle_for(synthetic_hand_pose())
    u = _interior_state(env)
    orc = _OracleStep(env, om, None, 1)
    nv, na, nu = om.nv, om.na, om.nu
    nx = 2 * nv + na
    q, v, a = (orc.state[i][0] for i in range(3))
    Ao, Bo, xo = orc.linearize(0, u[0], EPS_FD)

    def oracle_residual(d):
        end = orc(0, sim_np_integrate(q, d[:nv], *orc.tabs), v + d[nv:2 * nv], a + d[2 * nv:nx], u[0] + d[nx:])
        return np.linalg.norm(orc.tangent(end, xo) - Ao @ d[:nx] - Bo @ d[nx:])
    draws = []
    for seed in range(24):
        d = np.random.RandomState(100 + seed).uniform(-1e-4, 1e-4, nx + nu)
        ratio = oracle_residual(d) / oracle_residual(d / 2)
        if 3 <= ratio <= 5:
            draws.append(d)
        if len(draws) == 8:
            break
    assert len(draws) == 8, len(draws)
    lin = env.linearize(ctrl=u, eps=EPS_FD, nsub=1)
    A, B = lin["A"][0], lin["B"][0]
    tabs = env._tangent_tables()
    D = torch.as_tensor(np.stack([h * d for d in draws for h in (1.0, 0.5)]), dtype=torch.float64, device=env.device)      # [16, nx + nu]
    q0, v0, a0, _ = env.get_state()
    S = D.shape[0]
    out = env.simulate((torch.as_tensor(u, device=env.device)[:, None] + D[None, :, nx:])[:, :, None], nsub=1,
                       qpos=integrate_pos(q0[:, None].expand(1, S, -1), D[None, :, :nv], *tabs), qvel=v0[:, None] + D[None, :, nv:2 * nv],
                       act=a0[:, None] + D[None, :, 2 * nv:nx])
    xn = lin["x_next"][0]
    nq = q0.shape[1]
    dx = torch.cat([differentiate_pos(out["qpos"][0, :, 0], xn[None, :nq].expand(S, -1), *tabs), out["qvel"][0, :, 0] - xn[nq:nq + nv], out["act"][0, :, 0] - xn[nq + nv:]], -1)
    res = (dx - D[:, :nx] @ A.T - D[:, nx:] @ B.T).norm(dim=1).cpu().numpy()
    ratios = res[0::2] / res[1::2]
    print(f"    residual ratios full / half perturbation: {np.round(ratios, 3)} (median {np.median(ratios):.3f}); residuals {res[0::2]}")
    assert 3 <= np.median(ratios) <= 5, ratios
    env.close()


def test_linearize_is_second_order_on_emulation(emu_lib):
    case_linearize_second_order(emu_lib)


@pytest.mark.gpu
def test_linearize_is_second_order_on_gpu(hip_lib):
    case_linearize_second_order(hip_lib)


# ---------------------------------------------------------------------------------------------------------------- main_eval
def test_main_eval_record_simulate_on_emulation(emu_lib, golden_dir, tmp_path, capsys):
    """main_eval --record-simulate T: the .npz gains sim_qpos [T_steps, n, nq] / sim_bad [T_steps, n], the final qpos of the T-step
    zero-control prediction from each recorded state; without the switch the file is what it was"""
    import os
    from myochallenge_amd.main_eval import evaluate, main
    model, pkl = os.path.join(golden_dir, "phase1_final.zip"), os.path.join(golden_dir, "normalized_env_phase1_final.pkl")
    base = {"qpos", "qvel", "act", "actuator_length", "actuator_velocity", "actuator_force", "ncon", "object_wrench", "object_body_ids"}
    files = {}
    for tag, horizon in (("with", 2), ("without", 0)):
        env = make_env("CustomMyoBaodingBallsP1", emu_lib, num_envs=2, seed=3, max_episode_steps=3)
        rec = tmp_path / tag
        res, _ = evaluate(model, pkl, "CustomMyoBaodingBallsP1", config={}, num_episodes=2, num_envs=2, seed=3, verbose=False,
                          record_dir=str(rec), env=env, record_simulate=horizon)
        files[tag] = (dict(np.load(rec / "batch00000.npz")), int(res["lengths"].max()), env._model.size("nq"))
        if horizon:      # the last recorded prediction is the one from the final state
            last = env.simulate(np.zeros((2, horizon, env.act_dim)), every=horizon, keys=["qpos"])["qpos"][:, 0, 0]
            assert np.array_equal(files[tag][0]["sim_qpos"][-1], last.cpu().numpy())
        env.close()
    z, T, nq = files["with"]
    assert set(z) == base | {"sim_qpos", "sim_bad"}
    assert z["sim_qpos"].shape == (T, 2, nq) and z["sim_bad"].shape == (T, 2) and z["sim_qpos"].dtype == np.float64 and z["sim_bad"].dtype == np.int32
    assert (z["sim_bad"] == 0).all() and np.isfinite(z["sim_qpos"]).all() and not np.array_equal(z["sim_qpos"], z["qpos"])
    z0 = files["without"][0]
    assert set(z0) == base and all(np.array_equal(z0[k], z[k]) for k in base)          # the prediction changes nothing about the run
    env = make_env("CustomMyoBaodingBallsP1", emu_lib, num_envs=2, seed=3, max_episode_steps=3)
    with pytest.raises(ValueError):
        evaluate(model, pkl, "CustomMyoBaodingBallsP1", config={}, num_episodes=2, num_envs=2, seed=3, verbose=False, env=env, record_simulate=2)
    env.close()
    with pytest.raises(SystemExit):
        main(["--help"])
    assert "--record-simulate" in capsys.readouterr().out
    with pytest.raises(SystemExit):          # the switch needs --record-dir
        main(["--model", model, "--env-path", pkl, "--record-simulate", "2"])
