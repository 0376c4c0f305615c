"""Per-env Jacobians and inverse dynamics (myo_batch_jac / myo_batch_inverse; BaodingVecEnv.jac / .inverse): every case of
tests/jac_cases.py on the lane-serial emulation (CPU) and on the HIP kernels (-m gpu), then the Python surface."""
import numpy as np
import pytest

import jac_cases as jc
from helpers import make_env
from myochallenge_amd import native

DTYPES = [pytest.param(native.MYO_F64, id="f64"), pytest.param(native.MYO_MIXED, id="mixed")]
MODELS = ["finger", "hand", "die"]


# ---------------------------------------------------------------------------------------------------------------- emulation (CPU)
@pytest.mark.parametrize("which", MODELS)
def test_finite_differences_on_emulation(emu_lib, which):
    jc.case_finite_differences(emu_lib, which)


def test_identities_on_emulation(emu_lib):
    jc.case_identities(emu_lib)


def test_structure_on_emulation(emu_lib):
    jc.case_structure(emu_lib)


def test_forward_inverse_on_emulation(emu_lib):
    """measured (emulation): see DESIGN.md 5.12"""
    jc.case_forward_inverse(emu_lib)


def test_inverse_unconstrained_on_emulation(emu_lib):
    jc.case_inverse_unconstrained(emu_lib)


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dtype_on_emulation(emu_lib, dtype, which):
    jc.case_dtype(emu_lib, dtype, which)


@pytest.mark.parametrize("dtype", DTYPES)
def test_read_only_on_emulation(emu_lib, dtype):
    jc.case_read_only(emu_lib, dtype)


def test_batch_sizes_on_emulation(emu_lib):
    jc.case_batch_sizes(emu_lib)


def test_bad_args_on_emulation(emu_lib):
    jc.case_bad_args(emu_lib)


# ---------------------------------------------------------------------------------------------------------------- HIP (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("which", MODELS)
def test_finite_differences_on_gpu(hip_lib, which):
    jc.case_finite_differences(hip_lib, which)


@pytest.mark.gpu
def test_identities_on_gpu(hip_lib):
    jc.case_identities(hip_lib)


@pytest.mark.gpu
def test_structure_on_gpu(hip_lib):
    jc.case_structure(hip_lib)


@pytest.mark.gpu
def test_forward_inverse_on_gpu(hip_lib):
    """measured (gfx950): see DESIGN.md 5.12"""
    jc.case_forward_inverse(hip_lib)


@pytest.mark.gpu
def test_inverse_unconstrained_on_gpu(hip_lib):
    jc.case_inverse_unconstrained(hip_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dtype_on_gpu(hip_lib, dtype, which):
    jc.case_dtype(hip_lib, dtype, which)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_read_only_on_gpu(hip_lib, dtype):
    jc.case_read_only(hip_lib, dtype)


@pytest.mark.gpu
def test_batch_sizes_on_gpu(hip_lib):
    jc.case_batch_sizes(hip_lib)


@pytest.mark.gpu
def test_bad_args_on_gpu(hip_lib):
    jc.case_bad_args(hip_lib)


# ---------------------------------------------------------------------------------------------------------------- Python surface
def _stepped_env(lib, name="CustomMyoBaodingBallsP1", n=3, steps=2, **kw):
    env = make_env(name, lib, num_envs=n, seed=1, **kw)
    env.reset()
    rng = np.random.RandomState(1)
    for _ in range(steps):
        env.step(np.clip(rng.normal(0, 0.5, (n, env.act_dim)), -1, 1).astype(np.float32))
    return env


def case_python_surface(lib):
    import torch
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    env = _stepped_env(lib, dtype="f64")
    n, m = env.num_envs, env._model
    nb, nv, ng, ns = (m.size(k) for k in ("nbody", "nv", "ngeom", "nsite"))
    assert set(native.JAC_KINDS) == set(jc.KINDS)
    for kind, k in (("body", nb), ("bodycom", nb), ("site", ns), ("geom", ng), ("subtreecom", nb)):
        J = env.jac(kind)
        assert set(J) == ({"jacp"} if kind == "subtreecom" else {"jacp", "jacr"}), kind
        for v in J.values():
            assert tuple(v.shape) == (n, k, 3, nv) and v.dtype == torch.float64 and v.device == env.device and bool(torch.isfinite(v).all())
    full = env.jac("site")
    assert set(env.jac("site", jacr=False)) == {"jacp"}
    # objects by name or id, repeated and unordered; indices select env rows as data() does
    names = env.site_names()
    tip, ball = names.index("s20"), names.index("ball1_site")
    part = env.jac("site", ["s20", ball, "s20"], indices=[2, 0])
    assert tuple(part["jacp"].shape) == (2, 3, 3, nv)
    assert torch.equal(part["jacp"][0, 0], full["jacp"][2, tip]) and torch.equal(part["jacp"][1, 1], full["jacp"][0, ball])
    assert torch.equal(part["jacr"][0, 2], full["jacr"][2, tip])
    assert torch.equal(env.jac("body", "ball2")["jacp"][:, 0], env.jac("body")["jacp"][:, env.body_names.index("ball2")])
    assert torch.equal(env.jac("geom", [env.geom_names[3]])["jacp"][:, 0], env.jac("geom")["jacp"][:, 3])
    # jacp @ qvel is the site's velocity: against a finite difference along the env's own velocity is the job of jac_cases; here
    # the task-space use — mj_jac at the sites' positions on the sites' bodies is the site Jacobian
    sx = env.data(["site_xpos"])["site_xpos"]
    sb = [int(b) for b in np.asarray(env.compiled.fields["site_bodyid"])]
    P = env.jac("body", [sb[tip], sb[ball]], points=sx[:, [tip, ball]])
    assert (P["jacp"] - full["jacp"][:, [tip, ball]]).abs().max() < 1e-12
    assert torch.equal(env.jac("body", [sb[tip]], points=sx[:, [tip]].cpu().numpy())["jacp"], P["jacp"][:, :1])
    with pytest.raises(KeyError):
        env.jac("no_such_kind")
    with pytest.raises(KeyError):
        env.jac("site", ["no_such_site"])
    with pytest.raises(KeyError):
        env.jac("body", [nb])
    with pytest.raises(ValueError):
        env.jac("body", [1, 2], points=sx[:, :3])
    with pytest.raises(ValueError):
        env.jac("site", [1], points=sx[:, :1])
    # inverse dynamics
    d = env.data(["qacc", "qfrc_actuator"])
    inv = env.inverse(d["qacc"])
    assert set(inv) == {"qfrc_inverse", "qfrc_constraint"}
    for v in inv.values():
        assert tuple(v.shape) == (n, nv) and v.dtype == torch.float64 and v.device == env.device
    assert torch.equal(inv["qfrc_constraint"], env.inverse(d["qacc"].cpu().numpy())["qfrc_constraint"])
    assert (inv["qfrc_inverse"] - d["qfrc_actuator"]).abs().max() < 1e-6 * max(1.0, float(d["qfrc_actuator"].abs().max()))
    one = env.inverse(d["qacc"], indices=[1])
    assert tuple(one["qfrc_inverse"].shape) == (1, nv) and torch.equal(one["qfrc_inverse"][0], inv["qfrc_inverse"][1])
    for bad in (d["qacc"][:1], d["qacc"][:, :-1], d["qacc"][0]):
        with pytest.raises(ValueError):
            env.inverse(bad)
    # VecNormalize forwards both calls
    venv = VecNormalize(env)
    assert torch.equal(venv.jac("site", ["s20"])["jacp"], full["jacp"][:, [tip]])
    assert torch.equal(venv.inverse(d["qacc"])["qfrc_inverse"], inv["qfrc_inverse"])
    # data(), sensors() and get_attr are what they were
    assert set(env.data()) == set(native.DATA_KEYS) and "jacp" not in env.sensors()
    env.close()


def test_python_surface_on_emulation(emu_lib):
    case_python_surface(emu_lib)


@pytest.mark.gpu
def test_python_surface_on_gpu(hip_lib):
    case_python_surface(hip_lib)


def test_inherited_by_die_and_pose_envs_on_emulation(emu_lib):
    die = _stepped_env(emu_lib, "CustomMyoReorientP1", n=2, steps=1)
    nv = die._model.size("nv")
    J = die.jac("body", ["Object", "target"])
    assert tuple(J["jacp"].shape) == (2, 2, 3, nv) and bool(J["jacp"][:, 0].any()) and not bool(J["jacp"][:, 1].any()) and not bool(J["jacr"][:, 1].any())
    assert tuple(die.inverse(np.zeros((2, nv)))["qfrc_inverse"].shape) == (2, nv)
    die.close()
    from helpers import _on_cpu
    from myochallenge_amd.envs.pose import PoseVecEnv
    pose = _on_cpu(PoseVecEnv)("CustomMyoHandPoseRandom", 2, {}, lib=emu_lib, seed=1)
    pose.reset()
    pose.step(np.zeros((2, pose.act_dim), np.float32))
    nv = pose._model.size("nv")
    assert tuple(pose.jac("site")["jacr"].shape) == (2, pose._model.size("nsite"), 3, nv)
    assert tuple(pose.inverse(np.ones((2, nv)))["qfrc_constraint"].shape) == (2, nv)
    pose.close()


def test_header_struct_sizes():
    """myo_jac_out / myo_inverse_out: a size word and two pointers; data()'s struct and keys are what they were"""
    import ctypes as C
    assert C.sizeof(native.JacOut) == C.sizeof(native.InverseOut) == 24
    assert C.sizeof(native.DataOut) == 8 * (1 + len(native.DATA_KEYS)) and len(native.DATA_KEYS) == 18
    for sym in ("myo_batch_jac", "myo_batch_inverse"):
        assert sym in native.EXPORTED_SYMBOLS and sym in native.ENV_PATH_SYMBOLS
