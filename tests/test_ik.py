"""Inverse kinematics (myo_batch_ik; BaodingVecEnv.inverse_kinematics): every case of tests/ik_cases.py on the lane-serial emulation
(CPU) and on the HIP kernels (-m gpu), then the Python surface."""
import numpy as np
import pytest

import ik_cases as ik
from helpers import make_env
from myochallenge_amd import native

DTYPES = [pytest.param(native.MYO_F64, id="f64"), pytest.param(native.MYO_MIXED, id="mixed")]
F64 = native.MYO_F64
# (model, spread of the targets around the start, in joint space)
SETS = [pytest.param("finger", 0.3, id="finger"), pytest.param("finger", 1.0, id="finger-wide"), pytest.param("pose", 0.3, id="pose"),
        pytest.param("hand", 0.3, id="hand")]


# ---------------------------------------------------------------------------------------------------------------- emulation (CPU)
@pytest.mark.parametrize("which,spread", SETS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_on_emulation(emu_lib, dtype, which, spread):
    """measured (emulation, f64): at most 22 steps, kkt <= 1.0e-10, cost - scipy's <= 1.8e-14"""
    ik.case_solve(emu_lib, dtype, which, spread)


def test_unreachable_target_on_emulation(emu_lib):
    ik.case_unreachable(emu_lib)


def test_caps_on_emulation(emu_lib):
    ik.case_caps(emu_lib)


def test_options_on_emulation(emu_lib):
    ik.case_options(emu_lib)


@pytest.mark.parametrize("dtype", DTYPES)
def test_read_only_on_emulation(emu_lib, dtype):
    ik.case_read_only(emu_lib, dtype)


def test_read_only_with_fatigue_on_emulation(emu_lib):
    ik.case_read_only(emu_lib, F64, condition="fatigue")


@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism_on_emulation(emu_lib, dtype):
    ik.case_determinism(emu_lib, dtype)


def test_bad_args_on_emulation(emu_lib):
    ik.case_bad_args(emu_lib)


# ---------------------------------------------------------------------------------------------------------------- HIP (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("which,spread", SETS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_solve_on_gpu(hip_lib, dtype, which, spread):
    ik.case_solve(hip_lib, dtype, which, spread)


@pytest.mark.gpu
def test_unreachable_target_on_gpu(hip_lib):
    ik.case_unreachable(hip_lib)


@pytest.mark.gpu
def test_caps_on_gpu(hip_lib):
    ik.case_caps(hip_lib)


@pytest.mark.gpu
def test_options_on_gpu(hip_lib):
    ik.case_options(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_read_only_on_gpu(hip_lib, dtype):
    ik.case_read_only(hip_lib, dtype)


@pytest.mark.gpu
def test_read_only_with_fatigue_on_gpu(hip_lib):
    ik.case_read_only(hip_lib, F64, condition="fatigue")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism_on_gpu(hip_lib, dtype):
    ik.case_determinism(hip_lib, dtype)


@pytest.mark.gpu
def test_batch_of_130_on_gpu(hip_lib):
    ik.case_batch_130(hip_lib)


@pytest.mark.gpu
def test_bad_args_on_gpu(hip_lib):
    ik.case_bad_args(hip_lib)


# ---------------------------------------------------------------------------------------------------------------- Python surface
def _reachable_targets(env, ids, seed=2, spread=0.1):
    """(the envs' present qpos, the sites' positions at a pose `spread` away in joint space, inside the joint ranges: reachable targets)"""
    import torch
    n = env.num_envs
    P = ik.Problem(env.compiled, n, ids, np.zeros((n, len(ids), 3)))
    present = torch.zeros((n, env._model.size("nq")), dtype=torch.float64, device=env.device)
    env.batch.get_state(present, None, None, None)
    q = present.cpu().numpy().copy()
    q[:, P.qadr] = np.clip(q[:, P.qadr] + np.random.RandomState(seed).uniform(-spread, spread, (n, len(P.qadr))), P.lo, P.hi)
    env.batch.set_state(torch.as_tensor(q, device=env.device), None, None, None)
    targets = env.data(["site_xpos"])["site_xpos"][:, ids].clone()
    env.batch.set_state(present, None, None, None)
    return present, targets


def case_python_surface(lib):
    import torch
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    env = make_env("CustomMyoBaodingBallsP1", lib, num_envs=3, seed=1, dtype="f64")
    env.reset()
    n, m = env.num_envs, env._model
    nq, nv = m.size("nq"), m.size("nv")
    names = env.site_names()
    sites = [names[i] for i in ik.tip_sites(env.compiled)]
    ids = [names.index(s) for s in sites]
    k = len(sites)
    assert k == 5
    present, targets = _reachable_targets(env, ids)
    x0 = env.data(["site_xpos"])["site_xpos"][:, ids]
    out = env.inverse_kinematics(sites, targets)
    assert set(out) == set(native.IK_KEYS)
    shapes = {"qpos": (n, nq), "site_xpos": (n, k, 3), "residual": (n, k, 3), "cost": (n,), "kkt": (n,), "iters": (n,), "status": (n,)}
    for key, v in out.items():
        assert tuple(v.shape) == shapes[key] and v.device == env.device, key
        assert v.dtype == (torch.int32 if key in ("iters", "status") else torch.float64), key
    assert bool((out["status"] == 0).all())
    assert float(out["residual"].abs().max()) < float((targets - x0).abs().max())
    # the envs did not move
    assert torch.equal(env.data(["site_xpos"])["site_xpos"][:, ids], x0)
    # names and ids are both accepted, numpy targets too
    by_id = env.inverse_kinematics(ids, targets.cpu().numpy())
    for key in out:
        assert torch.equal(by_id[key], out[key]), key
    # keys and indices select
    part = env.inverse_kinematics(sites, targets, indices=[2, 0], keys=["qpos", "status"])
    assert set(part) == {"qpos", "status"} and tuple(part["qpos"].shape) == (2, nq)
    assert torch.equal(part["qpos"][0], out["qpos"][2]) and torch.equal(part["qpos"][1], out["qpos"][0])
    # a joint subset by name or id: nothing else moves; a free joint is refused
    jn = list(env.compiled.names["jnt"])
    f = env.compiled.fields
    sub = env.inverse_kinematics(sites, targets, joints=[jn[5], 6], keys=["qpos"])["qpos"]
    moved = (sub != present).any(0).cpu().numpy()
    assert set(np.flatnonzero(moved)) <= {int(f["jnt_qposadr"][5]), int(f["jnt_qposadr"][6])} and moved.any()
    free = int(np.flatnonzero(np.asarray(f["jnt_type"]) == 0)[0])
    with pytest.raises(ValueError):
        env.inverse_kinematics(sites, targets, joints=[free])
    with pytest.raises(KeyError):
        env.inverse_kinematics(sites, targets, joints=["no_such_joint"])
    with pytest.raises(KeyError):
        env.inverse_kinematics(["no_such_site"], targets[:, :1])
    with pytest.raises(KeyError):
        env.inverse_kinematics(sites, targets, keys=["no_such_key"])
    # shape errors raise
    for bad in (dict(targets=targets[:1]), dict(targets=targets[:, :2]), dict(weight=np.ones(k + 1)), dict(q_init=np.zeros((n, nq + 1))),
                dict(q_ref=np.zeros(nq)), dict(lower=np.zeros((n, nq + 5))), dict(lower=np.ones((n, nv)), upper=np.zeros((n, nv)))):
        kw = dict(targets=targets)
        kw.update(bad)
        with pytest.raises(ValueError):
            env.inverse_kinematics(sites, **kw)
    with pytest.raises(ValueError):
        env.inverse_kinematics(ids * 4, torch.zeros((n, 4 * k, 3), dtype=torch.float64))
    for kw in (dict(reg=0.0), dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(native.MyoError):
            env.inverse_kinematics(sites, targets, **kw)
    # weights shared or per env; q_init = the present state is the default
    w = np.array([1.0, 0.5, 2.0, 1.0, 0.0])
    assert torch.equal(env.inverse_kinematics(sites, targets, weight=w)["qpos"], env.inverse_kinematics(sites, targets, weight=np.tile(w, (n, 1)))["qpos"])
    assert torch.equal(env.inverse_kinematics(sites, targets, q_init=present)["qpos"], out["qpos"])
    # VecNormalize forwards
    assert torch.equal(VecNormalize(env).inverse_kinematics(sites, targets)["qpos"], out["qpos"])
    # applying the result puts the sites where the call said they would be
    env.batch.set_state(out["qpos"].contiguous(), None, None, None)
    x1 = env.data(["site_xpos"])["site_xpos"][:, ids]
    assert float((x1 - out["site_xpos"]).abs().max()) <= 1e-13
    env.close()


def test_python_surface_on_emulation(emu_lib):
    case_python_surface(emu_lib)


@pytest.mark.gpu
def test_python_surface_on_gpu(hip_lib):
    case_python_surface(hip_lib)


def case_inherited(lib):
    import torch
    die = make_env("CustomMyoReorientP1", lib, num_envs=2, seed=1)
    die.reset()
    ids = ik.tip_sites(die.compiled)
    out = die.inverse_kinematics(ids, _reachable_targets(die, ids)[1])
    assert tuple(out["qpos"].shape) == (2, die._model.size("nq")) and bool((out["status"] == 0).all())
    die.close()
    from helpers import _on_cpu
    from myochallenge_amd.envs.pose import PoseVecEnv
    pose = (_on_cpu(PoseVecEnv) if lib.is_emulation else PoseVecEnv)("CustomMyoHandPoseRandom", 2, {}, lib=lib, seed=1)
    pose.reset()
    ids = ik.tip_sites(pose.compiled)
    out = pose.inverse_kinematics(ids, _reachable_targets(pose, ids)[1])
    assert tuple(out["residual"].shape) == (2, len(ids), 3) and bool((out["status"] == 0).all())
    assert bool(torch.isfinite(out["cost"]).all())
    pose.close()


def test_inherited_by_die_and_pose_envs_on_emulation(emu_lib):
    case_inherited(emu_lib)


@pytest.mark.gpu
def test_inherited_by_die_and_pose_envs_on_gpu(hip_lib):
    case_inherited(hip_lib)


def test_workspace_size_matches_the_kernel_header():
    """native.IK_WS_DOUBLES and native.IK_K_MAX restate csrc/myo_ik.h's MYO_IK_WS_N and include/myobatch.h's MYO_IK_K_MAX"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    read = lambda *p: open(os.path.join(root, *p)).read()
    nv = int(re.search(r"#define MYO_NV_MAX (\d+)", read("myochallenge_amd", "csrc", "myo_model_dev.h")).group(1))
    kmax = int(re.search(r"#define MYO_IK_K_MAX (\d+)", read("include", "myobatch.h")).group(1))
    assert "#define MYO_IK_K_MAX" not in read("myochallenge_amd", "csrc", "myo_ik.h")      # defined once
    up = lambda x: (x + 15) // 16 * 16
    assert native.IK_K_MAX == kmax
    assert native.IK_WS_DOUBLES == up(up(nv * (nv + 1) // 2) + 3 * kmax * nv + 3 * kmax)


def test_header_struct_sizes():
    """myo_ik_in / _out: a size word first; the symbol is in both lists; the structs that were there are what they were"""
    import ctypes as C
    assert C.sizeof(native.IkIn) == 112 and C.sizeof(native.IkOut) == 64
    assert native.IkIn._fields_[0][0] == native.IkOut._fields_[0][0] == "size"
    assert C.sizeof(native.StaticOptIn) == 72 and C.sizeof(native.StaticOptOut) == 80
    assert "myo_batch_ik" in native.EXPORTED_SYMBOLS and "myo_batch_ik" in native.ENV_PATH_SYMBOLS
    assert (native.IK_CAP, native.IK_STALL, native.IK_PINNED, native.IK_K_MAX) == (1, 2, 4, 16)
