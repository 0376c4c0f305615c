"""``muscle_condition=`` on every env family (MyoSuite's BaseV0._setup kwarg [3P-RECALL]): sarcopenia (a model edit), reafferentation
(the EIP -> EPL tendon transfer in the action map) and fatigue (the 3CC-r state advanced inside the step kernel).  The cases and the
numpy restatement of the spec are in muscle_condition_cases.py; the emulation build runs them on the CPU, the same cases run on the GPU
(``-m gpu``), where the split-step case adds both publish forms of the real launch.

Bounds.  One-step fatigue map: no accumulation — the restatement is fed the device's own previous state — so only rounding and FMA
contraction separate the two: quantities up to 1 / dt = 100, about ten roundings of 1.1e-16 relative, times dt: absolute 1e-13.
Physics against the oracle twins: the project's 1e-9 on the fp64 state, 5e-7 absolute on float32 observations (pose_cases' bounds).
Sarcopenia: 1e-12 relative (the active force is linear in the peak force)."""
import numpy as np
import pytest

import muscle_condition_cases as mc
from helpers import make_env
from myochallenge_amd import native

P1, DIE = "CustomMyoBaodingBallsP1", "CustomMyoReorientP1"
DTYPES = [native.MYO_F64, native.MYO_MIXED]
IDS = ["f64", "mixed"]


# ------------------------------------------------------------------------------------------ the cases, on a library
def case_fatigue_map(lib, dtype, env_name):
    cm, _ = mc.compiled("die" if env_name == DIE else "hand")
    R = mc.rollout(lib, dtype, env_name)
    dyn = np.asarray(cm.fields["actuator_dynprm"], float).reshape(-1, 10)
    # the clip's lower side binds only if LR |TL - MA| can exceed MA / dt - F MA, i.e. (0.5 + 1.5) / td > 1 / dt - F at MA = 1: true for
    # the Baoding envs (dt = 0.02, td = 0.04: 50 > 49.7), impossible for the die (dt = 0.01: 50 < 99.7) — worked out from the spec
    reachable = bool((2.0 / dyn[:, 1] > 1.0 / R["dt"] - mc.PRM["F"]).any())
    assert reachable == (env_name != DIE)
    r = mc.check_fatigue_map(R, cm, want_clip_lo=reachable)
    print(env_name, "fatigue one-step map:", r)
    assert r["tied_share"] <= 0.01, r
    assert not r["missing"], r                                   # coverage: every branch, both rR values, the reachable clip sides
    assert r["err"] <= 1e-13, r
    assert r["sum_err"] <= 1e-12 and r["lo"] >= -1e-15 and r["hi"] <= 1 + 1e-15, r
    assert r["reset_exact"] and r["resets"] >= 2 * 3, r          # horizon 15, 40 steps: every env auto-resets at least twice
    h = R["health"]
    assert h["protocol_errors"] == 0 and h["limit_row_overflows"] == 0, h


def case_split(lib, dtype, publishes=(None,)):
    whole = mc.rollout_bytes(mc.rollout(lib, dtype, P1, split="0"))
    assert any(w.dtype == np.uint8 and w.any() for w in whole), "the rollout should cross an episode end"
    mc.same_bits(whole, mc.rollout_bytes(mc.rollout(lib, dtype, P1, split="4,3,2,1")))
    for pub in publishes:
        mc.same_bits(whole, mc.rollout_bytes(mc.rollout(lib, dtype, P1, split=None, publish=pub)))      # the default plan (4 + 3 + 2 + 1)


def case_physics_used(lib):
    cm, om = mc.compiled("hand")
    R = mc.rollout(lib, native.MYO_F64, P1)
    r = mc.check_physics_used(R, om, lambda s, e: s["after"][e][0], cm.size("nq") - 14)
    print("fatigue, physics against twins stepped with the reported MA:", r)
    assert r["compared"] >= 30 * 2, r
    assert r["qpos"] <= 1e-9 and r["obs"] <= 5e-7, r


def case_reafferentation(lib):
    cm, om = mc.compiled("hand")
    R = mc.rollout(lib, native.MYO_F64, P1, condition="reafferentation", n=2, nsteps=20, horizon=200)
    r = mc.check_physics_used(R, om, mc.reaf_ctrl(cm), cm.size("nq") - 14)
    print("reafferentation, physics against twins stepped with the swapped ctrl:", r)
    assert r["compared"] >= 30, r
    assert r["qpos"] <= 1e-9 and r["obs"] <= 5e-7, r
    plain = mc.check_physics_used(R, om, lambda s, e: mc.ctrl_of(s["a"][e]), cm.size("nq") - 14)
    assert plain["qpos"] > 1e-6, plain                           # (and the swap is what the device did: the plain map is far off)


def case_sarcopenia(lib, dtype):
    r = mc.check_sarcopenia(lib, dtype)
    print("sarcopenia:", r)
    assert r["active_scale"] > 1.0, r                            # newtons: the muscles do pull in the probed states
    assert r["active"] <= 1e-12 and r["passive"] <= 1e-12, r


class _Ident:
    training = True

    def normalize_obs(self, o):
        return o


def case_surface(lib):
    """every env family takes the kwarg and steps; the fatigue accessors through VecNormalize; the C entry point's refusal"""
    import torch
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    torch.manual_seed(1)
    kw = dict(num_envs=2, seed=5, muscle_condition="fatigue", fatigue_params=dict(F=0.3, R=0.02))
    families = [(P1, {}), ("CustomMyoBaodingBallsP2", {}), (DIE, {}), ("CustomMyoHandPoseFixed", {}),
                ("MixtureModelBaodingEnv", dict(base_model_path=None, base_env_path=None, base_policy=ActorCriticPolicy(86, 39, (16,), (16,), lstm_hidden_size=8),
                                                base_normalizer=_Ident(), n_steps_base_model=2))]
    for name, extra in families:
        if name.startswith("CustomMyoHandPose"):
            from helpers import _on_cpu
            from myochallenge_amd.envs.pose import PoseVecEnv
            cls = _on_cpu(PoseVecEnv) if lib.is_emulation else PoseVecEnv
            env = cls(name, 2, dict(muscle_condition="fatigue", fatigue_params=dict(F=0.3, R=0.02)), seed=5, lib=lib)
        else:
            env = make_env(name, lib, **kw, **extra)
        venv = VecNormalize(env, training=False)
        venv.reset_tensor()
        f = venv.fatigue_state()
        nu = env.act_dim
        assert set(f) == {"MA", "MR", "MF"} and all(tuple(v.shape) == (2, nu) and v.dtype == torch.float64 for v in f.values())
        if name != "MixtureModelBaodingEnv":                       # (the mixture env's reset has already played its base policy)
            assert float(f["MA"].abs().max()) == 0 and float((f["MR"] - 1).abs().max()) == 0 and float(f["MF"].abs().max()) == 0
        venv.set_fatigue_state(*(torch.full((2, nu), v, dtype=torch.float64) for v in mc.FATIGUED))
        mf = venv.get_attr("muscle_fatigue")
        assert len(mf) == 2 and mf[0].shape == (nu,) and np.all(mf[1] == 0.7)
        assert venv.get_attr("muscle_fatigue", [1])[0].shape == (nu,)
        venv.step_tensor(torch.zeros((2, nu), dtype=torch.float32, device=env.device))
        g = env.fatigue_state()
        assert float((g["MA"] + g["MR"] + g["MF"] - 1).abs().max()) <= 1e-12 and float((g["MF"] - 0.7).abs().max()) > 0
        for cond in ("sarcopenia", "reafferentation", ""):
            if name == "MixtureModelBaodingEnv":
                break
            if name.startswith("CustomMyoHandPose"):
                e2 = cls(name, 2, dict(muscle_condition=cond), seed=5, lib=lib)
            else:
                e2 = make_env(name, lib, num_envs=2, seed=5, muscle_condition=cond)
            e2.reset_tensor()
            e2.step_tensor(torch.zeros((2, nu), dtype=torch.float32, device=e2.device))
            with pytest.raises(native.MyoError):
                e2.fatigue_state()
            e2.close()
        env.close()
    with pytest.raises(ValueError):
        make_env(P1, lib, num_envs=2, muscle_condition="tired")
    # the C entry point on a batch without fatigue: the argument error, with a message
    cm, _ = mc.compiled("hand")
    b = native.Batch(native.Model(cm, lib), mc.make_cfg(P1, cm), 2, 0, 0, native.MYO_F64)
    assert lib.L.myo_batch_fatigue(b.h, None, None, None) == -1 and b"fatigue" in lib.L.myo_last_error()
    assert lib.L.myo_batch_fatigue(None, None, None, None) == -1
    b.close()


# ------------------------------------------------------------------------------------------ CPU: configuration, refusals, emulation
def test_conditions_are_lowered_and_refused():
    from myochallenge_amd.envs.config import MYOSUITE_MUSCLE, make_task_cfg
    from myochallenge_amd.model import apply_muscle_condition, compile_model
    from myochallenge_amd.synth_hand import synthetic_hand
    cm, _ = mc.compiled("hand")
    c = make_task_cfg(P1, cm)
    assert c.muscle_condition == native.MUSCLE_NONE
    assert (c.fatigue_F, c.fatigue_R, c.fatigue_r) == (0.00912, 0.000094, 150.0) == tuple(MYOSUITE_MUSCLE["fatigue_params"][k] for k in "FRr")
    c = make_task_cfg(P1, cm, muscle_condition="fatigue", fatigue_params=dict(F=0.3))
    assert c.muscle_condition == native.MUSCLE_FATIGUE and (c.fatigue_F, c.fatigue_R, c.fatigue_r) == (0.3, 0.000094, 150.0)
    c = make_task_cfg(P1, cm, muscle_condition="reafferentation")
    assert c.muscle_condition == native.MUSCLE_REAFFERENTATION
    assert (c.reaf_src, c.reaf_dst) == (cm.names["actuator"].index("EIP"), cm.names["actuator"].index("EPL"))
    assert make_task_cfg(P1, cm, muscle_condition="sarcopenia").muscle_condition == native.MUSCLE_NONE       # a model edit, no switch
    assert make_task_cfg(P1, cm, muscle_condition="").muscle_condition == native.MUSCLE_NONE
    for bad in (dict(muscle_condition="tired"), dict(muscle_condition="fatigue", fatigue_params=dict(tau=1.0))):
        with pytest.raises(ValueError):
            make_task_cfg(P1, cm, **bad)
    # a model without EPL
    mj = synthetic_hand()
    mj.names["actuator"] = ["thumb_x" if n == "EPL" else n for n in mj.names["actuator"]]
    with pytest.raises(ValueError):
        make_task_cfg(P1, compile_model(mj), muscle_condition="reafferentation")
    # sarcopenia: an edited COPY, gainprm[:, 2] halved, biasprm untouched; the two refusals
    mj = synthetic_hand()
    ms = apply_muscle_condition(mj, "sarcopenia")
    gp, gs = np.asarray(mj.arrays["actuator_gainprm"]), np.asarray(ms.arrays["actuator_gainprm"])
    assert np.array_equal(gs[:, 2], 0.5 * gp[:, 2]) and np.array_equal(np.delete(gs, 2, 1), np.delete(gp, 2, 1))
    assert np.array_equal(ms.arrays["actuator_biasprm"], mj.arrays["actuator_biasprm"]) and gp[:, 2].min() > 0
    for cond in (None, "", "fatigue", "reafferentation"):
        assert np.array_equal(apply_muscle_condition(mj, cond).arrays["actuator_gainprm"], gp)
    mj.arrays["actuator_gainprm"][3, 2] = -1.0
    with pytest.raises(ValueError, match="auto"):
        apply_muscle_condition(mj, "sarcopenia")
    with pytest.raises(ValueError):
        apply_muscle_condition(synthetic_hand(), "tired")
    with pytest.raises(ValueError, match="before compiling"):
        apply_muscle_condition(cm, "sarcopenia")


def test_compiled_model_with_sarcopenia_is_refused(emu_lib):
    cm, _ = mc.compiled("hand")
    with pytest.raises(ValueError, match="before compiling"):
        make_env(P1, emu_lib, num_envs=2, model=cm, muscle_condition="sarcopenia")


def test_batch_create_validates_the_muscle_fields(emu_lib):
    import ctypes as C
    cm, _ = mc.compiled("hand")
    model = native.Model(cm, emu_lib)

    def create(cfg):
        h = C.c_void_p()
        rc = emu_lib.L.myo_batch_create(model.h, C.byref(cfg), 2, 0, 0, native.MYO_F64, C.byref(h))
        if rc == 0:
            emu_lib.L.myo_batch_destroy(h)
        return rc
    good = mc.make_cfg(P1, cm, muscle_condition="fatigue")
    assert create(good) == 0
    for field, value in (("muscle_condition", 7), ("fatigue_F", -1.0), ("fatigue_R", float("nan"))):
        c = mc.make_cfg(P1, cm, muscle_condition="fatigue")
        setattr(c, field, value)
        assert create(c) == -1, field
    c = mc.make_cfg(P1, cm, muscle_condition="reafferentation")
    c.reaf_dst = c.reaf_src
    assert create(c) == -1
    c.reaf_dst = 39
    assert create(c) == -1
    c = mc.make_cfg(P1, cm, muscle_condition="fatigue")
    c.kind = native.TASK_NONE
    assert create(c) == -1 and b"task layer" in emu_lib.L.myo_last_error()


def test_record_and_lds_of_other_batches_are_unchanged(emu_lib):
    """A batch without fatigue keeps its record (myo_batch_copy_envs refuses to copy between records of different strides, so a
    fatigue batch and a plain one differing is visible through the ABI) and every batch kind its LDS footprint."""
    cm, _ = mc.compiled("hand")
    model = native.Model(cm, emu_lib)
    plain, reaf, fat = (native.Batch(model, mc.make_cfg(P1, cm, muscle_condition=c), 2, 0, 0, native.MYO_F64) for c in (None, "reafferentation", "fatigue"))
    assert plain.lds_bytes == reaf.lds_bytes == fat.lds_bytes
    idx = np.arange(2, dtype=np.int32)
    L = emu_lib.L
    assert L.myo_batch_copy_envs(fat.h, idx.ctypes.data, plain.h, idx.ctypes.data, 2, None) == -1      # another record, another condition
    assert L.myo_batch_copy_envs(reaf.h, idx.ctypes.data, plain.h, idx.ctypes.data, 2, None) == -1     # same record, another condition
    # the fatigue state travels with the env's record
    fat2 = native.Batch(model, mc.make_cfg(P1, cm, muscle_condition="fatigue"), 2, 0, 1, native.MYO_F64)
    f = np.tile(np.array(mc.FATIGUED)[None, :, None], (2, 1, 39))
    fat.fatigue(f, None)
    fat2.copy_envs_from(fat, idx[::-1].copy(), idx)
    g = np.zeros((2, 3, 39))
    fat2.fatigue(None, g)
    assert np.array_equal(g, f)
    for b in (plain, reaf, fat, fat2):
        b.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fatigue_one_step_map_on_emulation(emu_lib, dtype):
    case_fatigue_map(emu_lib, dtype, P1)


def test_fatigue_one_step_map_of_the_die_on_emulation(emu_lib):
    case_fatigue_map(emu_lib, native.MYO_F64, DIE)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fatigue_split_step_gives_the_whole_steps_bits_on_emulation(emu_lib, dtype):
    case_split(emu_lib, dtype)


def test_fatigue_physics_used_the_reported_ctrl_on_emulation(emu_lib):
    case_physics_used(emu_lib)


def test_reafferentation_on_emulation(emu_lib):
    case_reafferentation(emu_lib)


def test_sarcopenia_on_emulation(emu_lib):
    case_sarcopenia(emu_lib, native.MYO_F64)


def test_fatigue_masked_reset_and_inner_steps_on_emulation(emu_lib):
    """myo_batch_reset with a mask rests the selected envs only; myo_batch_step_inner / _idx advance the state like a step;
    myo_batch_physics_step, whose caller gives ctrl, leaves it alone."""
    cm, _ = mc.compiled("hand")
    n, nu = 3, 39
    b = native.Batch(native.Model(cm, emu_lib), mc.make_cfg(P1, cm, muscle_condition="fatigue", fatigue_params=mc.PRM), n, 0, 3, native.MYO_F64)
    obs = np.zeros((n, b.obs_dim), np.float32)
    b.reset(None, obs)
    start = np.tile(np.array(mc.FATIGUED)[None, :, None], (n, 1, nu))
    rest = np.tile(np.array([0.0, 1.0, 0.0])[None, :, None], (n, 1, nu))
    got = np.zeros((n, 3, nu))
    b.fatigue(start, None)
    b.reset(np.array([0, 1, 0], np.uint8), obs)
    b.fatigue(None, got)
    assert np.array_equal(got[1], rest[1]) and np.array_equal(got[[0, 2]], start[[0, 2]])
    b.physics_step(np.full((n, nu), 0.3), 2)
    after = np.zeros((n, 3, nu))
    b.fatigue(None, after)
    assert np.array_equal(after, got)
    dyn = np.asarray(cm.fields["actuator_dynprm"], float).reshape(-1, 10)
    dt = 10 * float(cm.fields["opt_f64"][0])
    a = np.random.RandomState(2).uniform(-1, 1, (n, nu)).astype(np.float32)
    b.step_inner(np.array([1, 0, 1], np.uint8), a, obs, None)
    b.fatigue(None, after)
    want = [np.stack(mc.fatigue_ref(*got[e], mc.ctrl_of(a[e]), dyn[:, 0], dyn[:, 1], dt, **mc.PRM)[:3]) for e in range(n)]
    assert np.abs(after[0] - want[0]).max() <= 1e-13 and np.abs(after[2] - want[2]).max() <= 1e-13 and np.array_equal(after[1], got[1])
    got = after.copy()
    b.step_inner_idx(np.array([1, -1], np.int32), a[:2].copy(), obs[:2].copy(), None)
    b.fatigue(None, after)
    want = np.stack(mc.fatigue_ref(*got[1], mc.ctrl_of(a[0]), dyn[:, 0], dyn[:, 1], dt, **mc.PRM)[:3])
    assert np.abs(after[1] - want).max() <= 1e-13 and np.array_equal(after[[0, 2]], got[[0, 2]])
    b.close()


def test_surface_on_emulation(emu_lib):
    case_surface(emu_lib)


def test_main_eval_has_the_switches():
    import inspect
    from myochallenge_amd import main_eval
    assert {"muscle_condition", "fatigue_params"} <= set(inspect.signature(main_eval.evaluate).parameters)
    with pytest.raises(SystemExit):
        main_eval.main(["--model", "m", "--env-path", "e", "--fatigue-F", "0.3"])         # needs --muscle-condition fatigue


# ------------------------------------------------------------------------------------------ GPU: the same cases on libmyobatch.so
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fatigue_one_step_map_on_gpu(hip_lib, dtype):
    case_fatigue_map(hip_lib, dtype, P1)


@pytest.mark.gpu
def test_fatigue_one_step_map_of_the_die_on_gpu(hip_lib):
    case_fatigue_map(hip_lib, native.MYO_F64, DIE)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fatigue_split_step_gives_the_whole_steps_bits_on_gpu(hip_lib, dtype):
    """... and both ways a part hands its record on: write-through stores (the default) and the agent release fence"""
    case_split(hip_lib, dtype, publishes=(None, "wt", "fence"))


@pytest.mark.gpu
def test_fatigue_physics_used_the_reported_ctrl_on_gpu(hip_lib):
    case_physics_used(hip_lib)


@pytest.mark.gpu
def test_reafferentation_on_gpu(hip_lib):
    case_reafferentation(hip_lib)


@pytest.mark.gpu
def test_sarcopenia_on_gpu(hip_lib):
    case_sarcopenia(hip_lib, native.MYO_F64)


@pytest.mark.gpu
def test_surface_on_gpu(hip_lib):
    case_surface(hip_lib)


@pytest.mark.gpu
def test_fatigue_at_full_size_on_gpu(hip_lib):
    """4096 envs, Baoding P1, fp64 stepper, 20 steps under fatigue: the invariants of the one-step case hold for every env and muscle,
    and the batch is healthy (no hand-off state of another generation, nothing dropped)."""
    import torch
    n, nu = 4096, 39
    env = make_env(P1, hip_lib, num_envs=n, seed=3, dtype="f64", muscle_condition="fatigue", fatigue_params=mc.PRM)
    env.reset_tensor()
    g = torch.Generator(device="cpu").manual_seed(7)
    env.set_fatigue_state(*(torch.full((n, nu), v, dtype=torch.float64) for v in mc.FATIGUED))
    for _ in range(20):
        env.step_tensor((torch.rand((n, nu), generator=g) * 2 - 1).to(env.device))
        f = env.fatigue_state()
        tot = f["MA"] + f["MR"] + f["MF"]
        assert float((tot - 1).abs().max()) <= 1e-12
        assert all(float(v.min()) >= -1e-15 and float(v.max()) <= 1 + 1e-15 for v in f.values())
    h = env.batch.health()
    assert h["protocol_errors"] == 0 and h["contact_overflows"] == 0 and h["limit_row_overflows"] == 0, h
    env.close()
