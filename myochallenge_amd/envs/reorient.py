"""Batched die-reorient environment — ``CustomReorientEnv`` (/root/reference/src/envs/reorient.py:11-212,
registrations ``CustomMyoChallengeDieReorientP1/P2-v0``, src/envs/__init__.py:24-55).

The whole env step runs inside libmyobatch's step kernel (task kind ``MYO_TASK_REORIENT``, csrc/myo_task.h), one
environment per wavefront exactly like the Baoding task: action map, frame_skip = 5 physics substeps of the hand +
die model, observation, the reward dictionary with its shaping state, TimeLimit, and the auto-reset with the
reference's per-episode draws (goal pose, per-geom die friction, die size).  This class only lowers the kwargs
to the C task configuration.  What is pinned and what is recalled:

* ``get_reward_dict`` (reorient.py:12-56) is pinned by goldens produced by calling the reference function itself
  (tools/make_golden.py -> tests/golden/reorient_reward_goldens.npz): the oracle's ``orc_reorient_reward`` and the
  torch mirror below are checked against them, the kernel against the oracle;
* ``reset`` / ``set_orientation`` (:124-205): goal position = initial + U(goal_pos)^3, Euler angles U(range) per axis
  with the optional ``goal_rot_x/y/z`` range lists, an independent friction triple for EVERY die geom, one size
  delta (every die geom moves outward by it, edge capsules grow by it — the reference's geometry update);
* ``enable_rsi`` (:150-176) rewrites ``body_pos`` / ``body_quat`` of the Object body.  That body carries the die's
  free joint, whose pose MuJoCo takes from qpos (``robot.reset(init_qpos)``), never from body_pos — the reference's
  RSI branch therefore starts the episode from exactly the state of the plain reset, and so does this env;
* the observation layout is MyoSuite 1.2.3's ``ReorientEnvV0`` [3P-RECALL, no artifact pins it]:
  hand_qpos 23, hand_qvel 23 (x dt), obj_pos 3, goal_pos 3, pos_err 3, obj_rot 3, goal_rot 3, rot_err 3,
  act 39 = 103; Euler angles by the mujoco-py ``rotations.py`` convention MyoSuite copies.

The die of the synthetic model is a rounded cube made of corner spheres and edge capsules (synth_hand.py).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import native
from ..model import compile_model
from .baoding import BaodingVecEnv
from .config import MUSCLE_DEFAULTS, lower_muscle_condition

REGISTRATION = {      # src/envs/__init__.py:24-55
    "CustomMyoReorientP1": dict(max_episode_steps=150, kwargs=dict(normalize_act=True, frame_skip=5, goal_pos=(-0.010, 0.010),
                                                                   goal_rot=(-1.57, 1.57))),
    "CustomMyoReorientP2": dict(max_episode_steps=150, kwargs=dict(normalize_act=True, frame_skip=5, goal_pos=(-0.020, 0.020),
                                                                   goal_rot=(-3.14, 3.14), obj_size_change=0.007,
                                                                   obj_friction_change=(0.2, 0.001, 0.00002))),
}
SETUP_DEFAULTS = dict(   # reorient.py:58-76; DEFAULT_RWD_KEYS_AND_WEIGHTS of ReorientEnvV0 [3P-RECALL]
    weighted_reward_keys={"pos_dist": 100.0, "rot_dist": 1.0}, goal_pos=(0.0, 0.0), goal_rot=(0.785, 0.785), obj_size_change=0,
    obj_friction_change=(0, 0, 0), pos_th=0.025, rot_th=0.262, drop_th=0.200, enable_rsi=False, rsi_distance_pos=0,
    rsi_distance_rot=0, goal_rot_x=None, goal_rot_y=None, goal_rot_z=None, frame_skip=5, normalize_act=True, **MUSCLE_DEFAULTS)
RWD_KEYS = ("pos_dist", "rot_dist", "pos_dist_diff", "rot_dist_diff", "alive", "act_reg", "sparse", "solved", "done", "dense")


# ---- rotations (mujoco-py rotations.py convention, as in myosuite.utils.quat_math) [3P-RECALL]
def euler2quat(e: torch.Tensor) -> torch.Tensor:
    ai, aj, ak = e[..., 2] / 2, -e[..., 1] / 2, e[..., 0] / 2
    si, sj, sk = torch.sin(ai), torch.sin(aj), torch.sin(ak)
    ci, cj, ck = torch.cos(ai), torch.cos(aj), torch.cos(ak)
    cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
    return torch.stack([cj * cc + sj * ss, cj * cs - sj * sc, -(cj * ss + sj * cc), cj * sc - sj * cs], -1)


def quat2mat(q: torch.Tensor) -> torch.Tensor:
    q = q / torch.clamp(torch.linalg.norm(q, dim=-1, keepdim=True), min=1e-30)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def mat2euler(m: torch.Tensor) -> torch.Tensor:
    cy = torch.sqrt(m[..., 2, 2] ** 2 + m[..., 1, 2] ** 2)
    cond = cy > 8.881784197001252e-16         # _EPS4
    ez = torch.where(cond, -torch.atan2(m[..., 0, 1], m[..., 0, 0]), -torch.atan2(-m[..., 1, 0], m[..., 1, 1]))
    ey = -torch.atan2(-m[..., 0, 2], cy)
    ex = torch.where(cond, -torch.atan2(m[..., 1, 2], m[..., 2, 2]), torch.zeros_like(cy))
    return torch.stack([ex, ey, ez], -1)


def get_reward_dict(obs_pos_err, obs_rot_err, act, prev_pos_dist, prev_rot_dist, na, drop_th, pos_th, rot_th, weights):
    """reorient.py:12-56 on batched float64 tensors.  Returns the OrderedDict's entries as a dict of [N] tensors."""
    pos_dist_new = torch.abs(torch.linalg.norm(obs_pos_err, dim=-1))
    rot_dist_new = torch.abs(torch.linalg.norm(obs_rot_err, dim=-1))
    act_mag = torch.linalg.norm(act, dim=-1) / na if na != 0 else torch.zeros_like(pos_dist_new)
    drop = pos_dist_new > drop_th
    d = {
        "pos_dist": -1.0 * pos_dist_new, "rot_dist": -1.0 * rot_dist_new,
        "pos_dist_diff": prev_pos_dist - pos_dist_new, "rot_dist_diff": prev_rot_dist - rot_dist_new,
        "alive": (~drop).to(pos_dist_new.dtype), "act_reg": -1.0 * act_mag, "sparse": -rot_dist_new - 10.0 * pos_dist_new,
        "solved": ((pos_dist_new < pos_th) & (rot_dist_new < rot_th) & (~drop)).to(pos_dist_new.dtype),
        "done": drop.to(pos_dist_new.dtype),
    }
    d["dense"] = sum(float(w) * d[k] for k, w in weights.items())
    return d, pos_dist_new, rot_dist_new




def resolve_reorient_kwargs(env_name: str, **kwargs) -> dict:
    if env_name not in REGISTRATION:
        raise ValueError("Environment name not recognized:", env_name)
    reg = REGISTRATION[env_name]
    p = dict(SETUP_DEFAULTS)
    p.update(reg["kwargs"])
    horizon = kwargs.pop("max_episode_steps", None)
    for k, v in kwargs.items():
        if k not in p and k not in ("obs_keys", "model_path"):
            raise TypeError(f"{env_name}: unexpected keyword argument {k!r}")
        p[k] = v
    p["max_episode_steps"] = int(reg["max_episode_steps"] if horizon is None else horizon)
    return p


def reorient_ids(compiled) -> dict:
    """The ids CustomReorientEnv._setup resolves by name (reorient.py:78-108)."""
    gb = np.asarray(compiled.fields["geom_bodyid"]).reshape(-1)
    obj = compiled.name2id("body", "Object")
    die = np.nonzero(gb == obj)[0]
    assert len(die) and int(die[-1]) + 1 - int(die[0]) == len(die), "die geoms must be contiguous"
    return dict(object_sid=compiled.name2id("site", "object_o"), goal_sid=compiled.name2id("site", "target_o"),
                object_bid=obj, goal_bid=compiled.name2id("body", "target"), object_gid0=int(die[0]), object_gidn=int(die[-1]) + 1)


def make_reorient_cfg(env_name: str, compiled, **kwargs) -> native.TaskCfg:
    p = resolve_reorient_kwargs(env_name, **kwargs)
    if not p["normalize_act"]:
        raise ValueError("normalize_act=False is not supported (every registration of the reference sets it)")
    c, ids = native.TaskCfg(), reorient_ids(compiled)
    c.kind, c.frame_skip, c.max_episode_steps = native.TASK_REORIENT, int(p["frame_skip"]), int(p["max_episode_steps"])
    c.n_hand = compiled.size("nq") - 7
    c.obj1_sid, c.target1_sid, c.obj1_bid = ids["object_sid"], ids["goal_sid"], ids["object_bid"]
    c.obj1_gid, c.obj2_gid = ids["object_gid0"], ids["object_gidn"]
    c.obj2_sid = c.target2_sid = c.obj2_bid = -1
    w = p["weighted_reward_keys"]
    for k in w:
        if k not in RWD_KEYS[:-1]:
            raise KeyError(f"unknown reward key {k!r}")
    for i, k in enumerate(RWD_KEYS[:-1]):
        c.ro_weights[i] = float(w.get(k, 0.0))
    c.ro_goal_pos[0], c.ro_goal_pos[1] = (float(x) for x in p["goal_pos"])
    c.ro_goal_rot[0], c.ro_goal_rot[1] = (float(x) for x in p["goal_rot"])
    for ax, name in enumerate(("goal_rot_x", "goal_rot_y", "goal_rot_z")):
        ch = p[name]
        if ch is None:
            continue
        if not 0 < len(ch) <= native.ROT_CHOICE_MAX:
            raise ValueError(f"{name}: between 1 and {native.ROT_CHOICE_MAX} (low, high) ranges")
        c.ro_n_rot_choice[ax] = len(ch)
        for j, (lo, hi) in enumerate(ch):
            c.ro_rot_choice[ax][j][0], c.ro_rot_choice[ax][j][1] = float(lo), float(hi)
    c.ro_obj_size_change = float(p["obj_size_change"])
    for i in range(3):
        c.obj_friction_change[i] = float(p["obj_friction_change"][i])
    c.ro_pos_th, c.ro_rot_th, c.drop_th = float(p["pos_th"]), float(p["rot_th"]), float(p["drop_th"])
    c.enable_rsi = int(bool(p["enable_rsi"]))
    c.ro_rsi_distance_pos, c.ro_rsi_distance_rot = float(p["rsi_distance_pos"]), float(p["rsi_distance_rot"])
    # goal_init_pos / goal_obj_offset: site positions of the model's initial configuration (reorient.py:82-86); the target
    # body hangs off the world, the Object body's pose is its free joint's qpos0
    f = compiled.fields
    body_pos, site_pos = np.asarray(f["body_pos"]).reshape(-1, 3), np.asarray(f["site_pos"]).reshape(-1, 3)
    body_quat = np.asarray(f["body_quat"]).reshape(-1, 4)
    qpos0 = np.asarray(f["qpos0"]).reshape(-1)
    rot = lambda q, v: quat2mat(torch.as_tensor(np.asarray(q, np.float64))).numpy() @ np.asarray(v, np.float64)
    goal0 = body_pos[ids["goal_bid"]] + rot(body_quat[ids["goal_bid"]], site_pos[ids["goal_sid"]])
    obj0 = qpos0[-7:-4] + rot(qpos0[-4:], site_pos[ids["object_sid"]])
    # The observation's obj_rot / goal_rot are mat2euler(site_xmat) in MyoSuite; the kernel and the oracle take the BODY
    # orientation, which is the same thing only for sites whose own frame is the identity: anything else is refused
    sq = np.asarray(f["site_quat"]).reshape(-1, 4) if "site_quat" in f else None
    for sid in (ids["object_sid"], ids["goal_sid"]):
        if sq is not None and not np.allclose(np.abs(sq[sid] / np.linalg.norm(sq[sid])), [1, 0, 0, 0], atol=1e-12):
            raise ValueError("die reorient: the object_o / target_o sites must have an identity orientation (site_quat) in this stepper")
    for i in range(3):
        # reorient.py:82,125-129: goal_init_pos is the target SITE's world position at set-up, and reset() writes
        # goal_init_pos + U(goal_pos) into body_pos[target] — for a site that sits off the body origin the goal therefore
        # starts displaced by the site's offset, a quirk of the reference that is kept
        c.ro_goal_init_pos[i] = float(goal0[i])
        c.ro_goal_obj_offset[i] = float(goal0[i] - obj0[i])
    c.init_qpos0 = -1.5                                                   # reorient.py:120-121
    lower_muscle_condition(c, compiled, p)
    return c


class ReorientVecEnv(BaodingVecEnv):
    """``num_envs`` die-reorient environments on one GPU: the tensor / SB3-VecEnv API of BaodingVecEnv."""

    rwd_keys = ("pos_dist", "rot_dist", "act_reg", "alive", "sparse", "solved", "done", "dense")     # comps[:, k]

    @staticmethod
    def _resolve(env_name, config):
        return resolve_reorient_kwargs(env_name, **config)

    @staticmethod
    def _default_model():
        from ..synth_hand import synthetic_hand_die
        return synthetic_hand_die()

    # (_compile is BaodingVecEnv's: unsupported_contacts="error" by default — the synthetic die, 12 edge capsules + 3 box slabs as
    # reorient.py:143-145 indexes the real one, compiles without dropping a pair since the capsule-box and box-box narrow phases exist)

    @staticmethod
    def _make_cfg(env_name, compiled, config):
        return make_reorient_cfg(env_name, compiled, **config)

    def __init__(self, env_name, num_envs, config=None, **kw):
        # The die is stepped by the fp64 stepper unless the caller asks otherwise (round 6): the mixed stepper takes
        # active-set decisions of the die's many simultaneous contacts in fp32 — 3e-5 of local error per env step on edge active sets,
        # 9-12 of 16 whole-episode streams inside north_star's 1e-4 — so for this env it is an opt-in variant, not an offer.
        if kw.get("dtype") is None:
            kw["dtype"] = "f64"
        elif kw["dtype"] in ("mixed", "f32"):
            import warnings
            warnings.warn("CustomMyoReorient*: the mixed stepper does not hold the 1e-4 trajectory tolerance on the die (DESIGN.md §4); "
                          "dtype='f64' is this env's default", stacklevel=3)
        super().__init__(env_name, num_envs, config, **kw)
        self.ids = reorient_ids(self.compiled)
        self.object_gid0, self.object_gidn = self.ids["object_gid0"], self.ids["object_gidn"]
        self.n_hand, self.frame_skip = int(self._cfg.n_hand), int(self._cfg.frame_skip)
        self.goal_init_pos = torch.tensor(list(self._cfg.ro_goal_init_pos), dtype=torch.float64)
        self.goal_obj_offset = torch.tensor(list(self._cfg.ro_goal_obj_offset), dtype=torch.float64)
        self.physical_randomisation_applied = bool(self._cfg.ro_obj_size_change) or any(float(x) != 0 for x in self._cfg.obj_friction_change)
        # the two shaping terms (pos_dist_diff, rot_dist_diff) enter `dense` on the device but are not among the 8 exported
        # reward components; when somebody wants the full dictionary (TensorboardCallback, step_wait infos) the env keeps the
        # previous step's distances and forms them on the side (one small state read per step)
        self.track_rwd_dict = False
        self._dists = self._diffs = None

    # ---- per-env task state (tests, logging): goal pose, shaping distances, the episode's die
    def task_state(self) -> dict:
        t, n, d = torch, self.num_envs, self.device
        ti, td, bd = t.zeros((n, 2), dtype=t.int32, device=d), t.zeros((n, 9), dtype=t.float64, device=d), t.zeros((n, 10), dtype=t.float64, device=d)
        fr = t.zeros((n, self.object_gidn - self.object_gid0, 3), dtype=t.float64, device=d)
        self.batch.get_task(ti, td, bd, self._stream())
        self.batch.object_friction(None, fr, self._stream())
        return dict(goal_pos=td[:, 0:3], goal_quat=td[:, 3:7], pos_dist=td[:, 7], rot_dist=td[:, 8], size_delta=bd[:, 8], friction=fr)

    def _read_dists(self):
        td = torch.zeros((self.num_envs, 9), dtype=torch.float64, device=self.device)
        self.batch.get_task(None, td, None, self._stream())
        return td[:, 7:9].clone()

    def reset_tensor(self):
        out = super().reset_tensor()
        self._dists = None
        return out

    def step_tensor(self, actions):
        if not self.track_rwd_dict:
            return super().step_tensor(actions)
        prev = self._read_dists() if self._dists is None else self._dists
        out = super().step_tensor(actions)
        self._diffs = prev + self._comps[:, :2].double()          # prev - new, with new = -comps[:, :2]
        self._dists = self._read_dists()                          # after the step: reset distances where an episode ended
        return out

    @property
    def rwd_dict(self):
        """reorient.py:29-52's dictionary for the last step (tensors [N]); the *_diff entries need `track_rwd_dict`."""
        d = {k: self._comps[:, j] for j, k in enumerate(self.rwd_keys)}
        if self._diffs is not None:
            d["pos_dist_diff"], d["rot_dist_diff"] = self._diffs[:, 0], self._diffs[:, 1]
        return d

    def step_wait(self):
        self.track_rwd_dict = True                                # the numpy protocol reports the whole dictionary, like info.update(rwd_dict)
        obs, rew, done, infos = super().step_wait()
        if self._diffs is not None:
            dh = self._diffs.cpu().numpy()
            for i, info in enumerate(infos):
                info["rwd_dict"].update(pos_dist_diff=float(dh[i, 0]), rot_dist_diff=float(dh[i, 1]))
                info.update(info["rwd_dict"])                     # reorient.py:211
        return obs, rew, done, infos

    def get_attr(self, attr_name, indices=None):
        idx = range(self.num_envs) if indices is None else indices
        if attr_name in ("pos_dist", "rot_dist"):
            v = self.task_state()[attr_name].cpu().numpy()
            return [float(v[i]) for i in idx]
        return super().get_attr(attr_name, indices)
