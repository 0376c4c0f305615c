"""Batched joint-pose environment on the MyoHand — ``CustomPoseEnv`` (/root/reference/src/envs/pose.py:6-117) with the
registrations ``CustomMyoHandPoseFixed``, ``CustomMyoHandPose{0..9}Fixed`` (the ten ASL numerals) and
``CustomMyoHandPoseRandom`` (/root/reference/src/envs/__init__.py:171-228).

The whole env step runs inside libmyobatch's step kernel (task kind ``MYO_TASK_POSE``, csrc/myo_task.h), one environment
per wavefront like the Baoding and die tasks: action map, frame_skip physics substeps of the hand, observation, reward
dictionary, TimeLimit(100) and the auto-reset with the per-episode draws (target pose, random start pose).  This module
lowers the kwargs to the C task configuration.  What is pinned and what is recalled:

* held by the reference: ``CustomPoseEnv._setup / reset / get_target_pose`` (target first — fixed or U(target_jnt_range)
  per joint, blended toward init_qpos by target_distance — then the state by reset_type: init / random = U(jnt_range) /
  sds = (1 - sds_distance) target + sds_distance init_qpos), every registration kwarg, ``jnt_namesHand``, ``ASL_qpos`` and
  the ``Rpos`` ranges derived from it; ``step`` puts the reward dictionary into ``info`` (pose.py:99-101);
* restated from MyoSuite 1.x ``PoseEnvV0`` / ``BaseV0``, which the reference inherits and does not contain: everything in
  ``MYOSUITE_POSE`` below [3P-RECALL].  A later check against MyoSuite changes that table (and, for the observation layout
  and the 1.5 bonus factor, the kernel's pose_obs_reward).

``reset_type="none"`` (keep the last state) and ``weight_bodyname`` / ``weight_range`` (a per-episode body mass, used by no
hand registration) are refused rather than half-implemented.  The model is the synthetic hand without objects
(synth_hand.synthetic_hand_pose, the labelled stand-in for ``myo_hand_pose.mjb``); a real ``.mjb`` may be passed as ``model=``.
"""
from __future__ import annotations

import math

import numpy as np

from .. import native
from ..synth_hand import JNT_NAMES_HAND
from .baoding import BaodingVecEnv
from .config import MUSCLE_DEFAULTS, lower_muscle_condition

# ---- [3P-RECALL] MyoSuite 1.x PoseEnvV0 / BaseV0 — not in the reference, restated here in ONE place
MYOSUITE_POSE = dict(
    obs_keys=("qpos", "qvel", "pose_err"),        # PoseEnvV0.DEFAULT_OBS_KEYS; obs qvel = sim.data.qvel * dt, dt = timestep * frame_skip
    weighted_reward_keys={"pose": 1.0, "bonus": 4.0, "act_reg": 1.0, "penalty": 50.0},   # PoseEnvV0.DEFAULT_RWD_KEYS_AND_WEIGHTS
    far_th=4 * math.pi / 2,                       # get_reward_dict: penalty / done when pose_dist > far_th
    bonus_factors=(1.0, 1.5),                     # bonus = (pose_dist < thd) + (pose_dist < 1.5 thd) (the kernel's constant)
    frame_skip=10,                                # BaseV0
)
RWD_KEYS = ("pose", "bonus", "penalty", "act_reg", "sparse", "solved", "done", "dense")     # comps[:, k]

# ---- the reference's registration data (src/envs/__init__.py:171-228)
POSE_FIXED_TARGET = np.array([0, 0, 0, -0.0904, 0.0824475, -0.681555, -0.514888, 0, -0.013964, -0.0458132, 0, 0.67553, -0.020944,
                              0.76979, 0.65982, 0, 0, 0, 0, 0.479155, -0.099484, 0.95831, 0], float)
ASL_QPOS = np.array([
    [0, 0, 0, 0.5624, 0.28272, -0.75573, -1.309, 1.30045, -0.006982, 1.45492, 0.998897, 1.26466, 0, 1.40604, 0.227795, 1.07614,
     -0.020944, 1.46103, 0.06284, 0.83263, -0.14399, 1.571, 1.38248],
    [0, 0, 0, 0.0248, 0.04536, -0.7854, -1.309, 0.366605, 0.010473, 0.269258, 0.111722, 1.48459, 0, 1.45318, 1.44532, 1.44532,
     -0.204204, 1.46103, 1.44532, 1.48459, -0.2618, 1.47674, 1.48459],
    [0, 0, 0, 0.0248, 0.04536, -0.7854, -1.13447, 0.514973, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 1.44532,
     -0.204204, 1.46103, 1.44532, 1.48459, -0.2618, 1.47674, 1.48459],
    [0, 0, 0, 0.3384, 0.25305, 0.01569, -0.0262045, 0.645885, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 1.571,
     -0.036652, 1.52387, 1.45318, 1.40604, -0.068068, 1.39033, 1.571],
    [0, 0, 0, 0.6392, -0.147495, -0.7854, -1.309, 0.637158, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 0.306345,
     -0.010472, 0.400605, 0.133535, 0.21994, -0.068068, 0.274925, 0.01571],
    [0, 0, 0, 0.3384, 0.25305, 0.01569, -0.0262045, 0.645885, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 0.306345,
     -0.010472, 0.400605, 0.133535, 0.21994, -0.068068, 0.274925, 0.01571],
    [0, 0, 0, 0.6392, -0.147495, -0.7854, -1.309, 0.637158, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 0.306345,
     -0.010472, 0.400605, 0.133535, 1.1861, -0.2618, 1.35891, 1.48459],
    [0, 0, 0, 0.524, 0.01569, -0.7854, -1.309, 0.645885, -0.006982, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 1.28036,
     -0.115192, 1.52387, 1.45318, 0.432025, -0.068068, 0.18852, 0.149245],
    [0, 0, 0, 0.428, 0.22338, -0.7854, -1.309, 0.645885, -0.006982, 0.128305, 0.194636, 1.39033, 0, 1.08399, 0.573415, 0.667675,
     -0.020944, 0, 0.06284, 0.432025, -0.068068, 0.18852, 0.149245],
    [0, 0, 0, 0.5624, 0.28272, -0.75573, -1.309, 1.30045, -0.006982, 1.45492, 0.998897, 0.39275, 0, 0.18852, 0.227795, 0.667675,
     -0.020944, 0, 0.06284, 0.432025, -0.068068, 0.18852, 0.149245],
], float)
# ASL train env: per joint, the range the ten numerals span (__init__.py:214-219)
RPOS = {n: (float(np.min(ASL_QPOS[:, i])), float(np.max(ASL_QPOS[:, i]))) for i, n in enumerate(JNT_NAMES_HAND)}

_FIXED = dict(pose_thd=0.7, reset_type="init", target_type="fixed", normalize_act=True)
REGISTRATION = {
    "CustomMyoHandPoseFixed": dict(max_episode_steps=100, kwargs=dict(target_jnt_value=POSE_FIXED_TARGET, **_FIXED)),
    **{f"CustomMyoHandPose{k}Fixed": dict(max_episode_steps=100, kwargs=dict(target_jnt_value=ASL_QPOS[k], **_FIXED)) for k in range(10)},
    "CustomMyoHandPoseRandom": dict(max_episode_steps=100, kwargs=dict(target_jnt_range=RPOS, pose_thd=0.8, reset_type="random",
                                                                       target_type="generate", normalize_act=True)),
}
SETUP_DEFAULTS = dict(   # CustomPoseEnv._setup (pose.py:7-22) + BaseV0's frame_skip
    viz_site_targets=None, target_jnt_range=None, target_jnt_value=None, reset_type="init", target_type="generate",
    obs_keys=MYOSUITE_POSE["obs_keys"], weighted_reward_keys=MYOSUITE_POSE["weighted_reward_keys"], pose_thd=0.35,
    weight_bodyname=None, weight_range=None, sds_distance=0, target_distance=1, frame_skip=MYOSUITE_POSE["frame_skip"],
    normalize_act=True, **MUSCLE_DEFAULTS)
_RESET = {"init": native.POSE_RESET_INIT, "random": native.POSE_RESET_RANDOM, "sds": native.POSE_RESET_SDS}
_TARGET = {"generate": native.POSE_TARGET_GENERATE, "fixed": native.POSE_TARGET_FIXED}


def resolve_pose_kwargs(env_name: str, **kwargs) -> dict:
    """Registration kwargs over the _setup defaults, then the caller's (gym.make(id, **kwargs))."""
    if env_name not in REGISTRATION:
        raise ValueError("Environment name not recognized:", env_name)
    reg = REGISTRATION[env_name]
    p = dict(SETUP_DEFAULTS)
    p.update(reg["kwargs"])
    horizon = kwargs.pop("max_episode_steps", None)
    for k, v in kwargs.items():
        if k not in p and k not in ("model_path", "seed"):
            raise TypeError(f"{env_name}: unexpected keyword argument {k!r}")
        p[k] = v
    p["max_episode_steps"] = int(reg["max_episode_steps"] if horizon is None else horizon)
    return p


def make_pose_cfg(env_name: str, compiled, **kwargs) -> native.TaskCfg:
    p = resolve_pose_kwargs(env_name, **kwargs)
    if not p["normalize_act"]:
        raise ValueError("normalize_act=False is not supported (every registration of the reference sets it)")
    if p["weight_bodyname"] is not None or p["weight_range"] is not None:
        raise NotImplementedError("weight_bodyname / weight_range (a per-episode body mass) are not supported: no hand-pose "
                                  "registration of the reference uses them")
    if p["reset_type"] not in _RESET:
        raise ValueError(f"reset_type {p['reset_type']!r} is not supported (init, random, sds; 'none' is refused)")
    if p["target_type"] not in _TARGET:
        raise ValueError(f"target_type {p['target_type']!r} is not supported (generate, fixed)")
    if tuple(p["obs_keys"]) != MYOSUITE_POSE["obs_keys"]:
        raise ValueError(f"obs_keys: only the default {MYOSUITE_POSE['obs_keys']} is supported")
    nq, nv = compiled.size("nq"), compiled.size("nv")
    if nq != nv or nq > native.POSE_NQ_MAX:
        raise ValueError(f"the joint-pose task needs a model of hinge / slide joints only (nq = nv <= {native.POSE_NQ_MAX})")
    f = compiled.fields
    jnt_names = list(compiled.names.get("jnt", []))
    c = native.TaskCfg()
    c.kind, c.frame_skip, c.max_episode_steps, c.n_hand = native.TASK_POSE, int(p["frame_skip"]), int(p["max_episode_steps"]), nq
    for k in ("obj1_sid", "obj2_sid", "target1_sid", "target2_sid", "obj1_bid", "obj2_bid", "obj1_gid", "obj2_gid"):
        setattr(c, k, -1)
    w = p["weighted_reward_keys"]
    for k in w:
        if k not in RWD_KEYS[:-1]:
            raise KeyError(f"unknown reward key {k!r}")
    for i, k in enumerate(RWD_KEYS[:-1]):
        c.pose_weights[i] = float(w.get(k, 0.0))
    c.pose_thd, c.pose_far_th = float(p["pose_thd"]), float(MYOSUITE_POSE["far_th"])
    c.pose_sds_distance, c.pose_target_distance = float(p["sds_distance"]), float(p["target_distance"])
    c.pose_reset_type, c.pose_target_type = _RESET[p["reset_type"]], _TARGET[p["target_type"]]
    init_qpos = np.asarray(f["qpos0"], float).reshape(-1)            # BaseV0's init_qpos: the model's initial configuration [3P-RECALL]
    jnt_range = np.asarray(f["jnt_range"], float).reshape(-1, 2)
    for i in range(nq):
        c.pose_init_qpos[i] = float(init_qpos[i])
        c.pose_reset_range[i][0], c.pose_reset_range[i][1] = float(jnt_range[i, 0]), float(jnt_range[i, 1])
    if p["target_jnt_range"] is None and p["target_jnt_value"] is None:
        raise ValueError("a joint-pose env needs target_jnt_range or target_jnt_value")
    if p["target_jnt_value"] is not None:
        v = np.asarray(p["target_jnt_value"], float).reshape(-1)
        if v.shape != (nq,):
            raise ValueError(f"target_jnt_value must have {nq} entries (one per joint), not {v.size}")
        for i in range(nq):
            c.pose_target_value[i] = float(v[i])
    rng = p["target_jnt_range"]
    if rng is not None:
        # _setup (pose.py:33-42): with a range, the fixed target is the range's mean and target_jnt_value is ignored.  The reference
        # stacks the ranges in dict order and compares that vector with qpos elementwise, which means joint by joint only when the dict
        # lists every joint in model order — the hand registrations do; anything else is refused
        if list(rng.keys()) != jnt_names[:nq]:
            raise ValueError("target_jnt_range must list every joint of the model, in model order")
        for i, n in enumerate(jnt_names[:nq]):
            lo, hi = rng[n]
            c.pose_target_range[i][0], c.pose_target_range[i][1] = float(lo), float(hi)
            c.pose_target_value[i] = 0.5 * (float(lo) + float(hi))
    elif p["target_type"] == "generate":
        raise ValueError("target_type 'generate' needs target_jnt_range")
    lower_muscle_condition(c, compiled, p)
    return c


class PoseVecEnv(BaodingVecEnv):
    """``num_envs`` joint-pose environments on one GPU: the tensor / SB3-VecEnv API of BaodingVecEnv."""

    rwd_keys = RWD_KEYS

    @staticmethod
    def _resolve(env_name, config):
        return resolve_pose_kwargs(env_name, **config)

    @staticmethod
    def _default_model():
        from ..synth_hand import synthetic_hand_pose
        return synthetic_hand_pose()

    @staticmethod
    def _make_cfg(env_name, compiled, config):
        return make_pose_cfg(env_name, compiled, **config)

    def __init__(self, env_name, num_envs, config=None, **kw):
        super().__init__(env_name, num_envs, config, **kw)
        self.nq, self.frame_skip = self._model.size("nq"), int(self._cfg.frame_skip)

    def task_state(self) -> dict:
        """Per-env target pose of the episode and the state it started from (task_d of myo_batch_get_task)."""
        t = self.torch
        ti = t.zeros((self.num_envs, 2), dtype=t.int32, device=self.device)
        td = t.zeros((self.num_envs, 2 * self.nq), dtype=t.float64, device=self.device)
        self.batch.get_task(ti, td, None, self._stream())
        return dict(target_qpos=td[:, :self.nq], init_qpos=td[:, self.nq:], step=ti[:, 1])

    def step_wait(self):
        obs, rew, done, infos = super().step_wait()
        for info in infos:
            info.update(info["rwd_dict"])                 # pose.py:99-101
        return obs, rew, done, infos

    def get_attr(self, attr_name, indices=None):
        idx = range(self.num_envs) if indices is None else indices
        if attr_name == "target_jnt_value":
            v = self.task_state()["target_qpos"].cpu().numpy()
            return [v[i].copy() for i in idx]
        return super().get_attr(attr_name, indices)
